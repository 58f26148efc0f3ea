// ivf_kernels.h -- host-callable launchers of the IVF kernel files (ivf_scan.hip, ivf_select.hip, ivf_build.hip) and the few
// constants the host side needs to size their buffers and choose among them.  This is all ivf.hip sees of them: it holds no
// device code, and the kernel files know nothing of IvfState.  Every launcher enqueues on `s`, owns its grid arithmetic and
// its dynamic-LDS attribute, and returns SQE_OK or the error it set.
#pragma once

#include "common.h"

namespace sqe {

#pragma GCC visibility push(hidden)   // calls between the IVF layer's own files: the library exports none of these

// ------------------------------------------------------------------ list scan (ivf_scan.hip)
constexpr int LS_ROWS = 256;              // rows of a tile: of the ring kernels' LDS stage and of the list-ordered int8 copy
constexpr int LS_Q = 64;                  // queries per pass of the ring kernels (the query copies are padded by as many rows)
constexpr int ST_Q = 32;                  // queries of a list resident in LDS per pass (more: the unit's rows are streamed again)
constexpr int ST_RING = 16;               // 1-KiB row fragments in flight per wave
constexpr int ST_FR = 4;                  // fragments (16 rows each) of a wave per K slice: 4 waves x 64 rows = a 256-row tile
constexpr int ST_SL = ST_RING / ST_FR;    // K slices the ring holds
constexpr int ST_UNIT_TILES = 5;
constexpr int ST_THREADS = 256;
constexpr int ST_PATCH_PITCH = 68;        // floats per query row of a wave's transpose patch: 64 rows + 4 (16-byte rows of different queries on different banks)
constexpr int ST_PATCH_ROWS = 36;         // query rows of patch per wave: four tiles of <= 8 (padded: 9) queries, one tile of 32

// dynamic LDS of the streaming kernel: the query block, the unit's row scales, pairs and query scales, the waves' patches
constexpr size_t ivf_stream_lds(int dim) {
    return (size_t)ST_Q * (dim + 128) + ST_UNIT_TILES * LS_ROWS * 4 + ST_Q * 8 + (ST_THREADS / 64) * ST_PATCH_ROWS * ST_PATCH_PITCH * 4;
}

// what every list scan reads and writes: the lists, the (query, probe) pairs bucketed by list (launch_ivf_bucket), the strips
struct ListScan {
    int nlist;
    const int64_t* offsets;    // [nlist + 1] start of each list in the list order
    const int* lcount;         // [nlist] pairs that probe each list
    const int* lq;             // [nlist, cap] those pairs (query * nprobe + probe)
    int cap, nprobe, dim, max_len;
    float* pair_scores;        // [B * nprobe, max_len] the strips
};
// the list-ordered int8 copy of the rows and the quantised queries (quant.hip)
struct ListScanI8 {
    const int8_t* rows; int64_t tile_stride; const uint32_t* sxi;      // tile t at t * tile_stride, row scales [tiles * 256]
    const int8_t* q8; int q8_pitch; const uint32_t* sqi;               // query rows at q8_pitch bytes, their scales
    float unit2;                                                       // i8_scale_unit(dim) squared
    const int64_t* tile_off;                                           // [nlist + 1] tiles in front of each list
};
// COLLECT (r04b): the scores are not written to strips.  A sample pass (the streaming kernel in strip mode over the FIRST tile of every list,
// ~10 % of the rows) and ivf_threshold_kernel have given every query a threshold that a few hundred of its ~78 k probed rows reach;
// the pass over the other tiles keeps only the (score, row) keys at or above it: they wait in an LDS buffer of the workgroup and go to
// the query's list (one global atomic per key) behind the unit's last load.  ivf_select_list_kernel ranks the list.  The 320 MB of
// strips per batch of 1024 and the pass that re-read them are gone (what is left of them: the sample's 32 MB).
struct StCollect {
    const float* thr;          // [B] per-query threshold on the estimated cosine
    int* cnt;                  // [B] keys appended to a query's list (may exceed list_cap: overflow -> the fallback)
    uint64_t* list;            // [B, list_cap]
    int list_cap;
    const int* order;          // row id of every list position
};

// (query, probe) pairs bucketed by list: lcount [nlist] (zeroed by the caller), lq [nlist, B]
int launch_ivf_bucket(const int64_t* probes, int B, int nprobe, int* lcount, int* lq, hipStream_t s);
// one workgroup per list, exact fp32 cosines from the master (knobs build: SQE_IVF_FP32=1)
int launch_ivf_list_scan_f32(const float* master, const float* qn, const int* order, const ListScan& a, hipStream_t s);
// one workgroup per list, rows gathered from the bf16 scan copy by `order`
int launch_ivf_list_scan_bf16(const bf16_t* scan, int pitch, const bf16_t* qb, int qpitch, const int* order, const ListScan& a, hipStream_t s);
// the staged int8 kernel; n_pairs > 0: pair mode, `split` workgroups per (query, probe) pair of `probes`, else one workgroup per list
int launch_ivf_list_scan_i8(const ListScanI8& c, const ListScan& a, const int64_t* probes, int n_pairs, int split, hipStream_t s);
// The streaming int8 kernel over a unit table (or, pair_probes != null, over pairs x pair_tiles tiles).  col == null: scores to the
// strips, else collect mode.  gate != null: nothing runs unless *gate != 0.  queue != null: `persistent` workgroups take the
// n_units units from that counter (zeroed by the caller), else one workgroup per unit.
int launch_ivf_list_stream_i8(const ListScanI8& c, const ListScan& a, const int4* units, int n_units, const StCollect* col, const int* gate,
                              int* queue, int persistent, const int64_t* pair_probes, int pair_tiles, hipStream_t s);

// ------------------------------------------------------------------ selects (ivf_select.hip)
constexpr int IVF_LIST_CAP = 8192;      // keys of a query's list: a whole cluster of near-ties (2,441 rows in SURVEY 8(d)'s set) must fit

// top-nprobe lists of b queries from their dense coarse scores [b, nlist], re-scored in fp32 (raw rows against the centroids)
int launch_ivf_probe_select(const float* scores, int b, int nlist, int nprobe, const float* rows, const float* cent, int dim, int64_t* probes,
                            float* probes_cos, hipStream_t s);
// collect thresholds thr [B] from the sample strips; opens the key lists: cnt [2 B] (keys listed, rows probed), list [B, IVF_LIST_CAP]
int launch_ivf_threshold(const int64_t* probes, const int64_t* offsets, const int* order, const float* pair_scores, int B, int nprobe, int max_len,
                         int kp, float* thr, int* cnt, uint64_t* list, hipStream_t s);
// what both final selects share: the fp32 re-score of the kp best estimates against the master and the top-k they write
struct IvfSelectOut {
    int k, kp;
    int64_t id_base;
    const float* master;
    const float* qn;           // [B, dim] normalised queries
    int dim;
    float* cos_out;            // [B, k]
    int64_t* id_out;
};
// top-k of each query from its strips; gate != null: nothing runs unless *gate != 0
int launch_ivf_select(const int64_t* probes, const int64_t* offsets, const int* order, const float* pair_scores, int B, int nprobe, int max_len,
                      const IvfSelectOut& o, const int* gate, hipStream_t s);
// top-k of each query from its key list (cnt [2 B] as launch_ivf_threshold left it); *fallback = 1 if some list cannot answer
int launch_ivf_select_list(const int* cnt, const uint64_t* list, int B, const IvfSelectOut& o, int* fallback, hipStream_t s);

// ------------------------------------------------------------------ k-means and list building (ivf_build.hip)
int launch_gather_rows(const float* x, const int64_t* idx, int n, int dim, float* out, hipStream_t s);
// sums[assign[r]] += x[r], counts[assign[r]]++; then centroid = sums / ||sums|| where the list is non-empty
int launch_kmeans_accum(const float* x, const int64_t* assign, int64_t n, int dim, float* sums, int* counts, hipStream_t s);
int launch_kmeans_finish(float* centroids, const float* sums, const int* counts, int nlist, int dim, hipStream_t s);
int launch_ivf_store_assign(const int64_t* ids, int64_t n, int* assign, hipStream_t s);
int launch_ivf_scatter_assign(const int* lists, const int64_t* rows, int64_t n, int* assign, hipStream_t s);
int launch_ivf_count(const int* assign, int64_t n, int* counts, hipStream_t s);
int launch_ivf_scatter(const int* assign, int64_t n, const int64_t* offsets, const int64_t* tile_off, int* cursor, int* order, int* dpos,
                       hipStream_t s);

#pragma GCC visibility pop

}  // namespace sqe
