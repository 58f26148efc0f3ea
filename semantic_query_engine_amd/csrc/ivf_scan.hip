// ivf_scan.hip -- the list-scan kernels of the IVF search (S6) and their launchers (ivf_kernels.h).  Every kernel scores
// the rows of the probed lists against the queries that probe them and leaves the scores in per-(query, probe) strips (or,
// the streaming kernel in collect mode, the keys at or above a query's threshold in its list):
//   ivf_list_scan_kernel          fp32 from the master, one workgroup per list (knobs build only)
//   ivf_list_scan_mfma_kernel     bf16 rows gathered by id through a 3-stage LDS ring, one workgroup per list
//   ivf_list_scan_i8_kernel       the same ring (list_scan_ring, written once) over the list-ordered tiled int8 copy: per
//                                 list, or per (query, probe) pair and segment of its list
//   ivf_list_stream_i8_kernel     int8 rows straight into the MFMA operand registers, one workgroup per unit of a list's tiles
// and ivf_bucket_kernel groups the (query, probe) pairs by list for all of them.  Called from ivf.hip only, which picks
// the kernel and the grid (ivf_route_plan).
#include "ivf_kernels.h"

namespace sqe {

namespace {

// (query, probe) pairs bucketed by list
__global__ void ivf_bucket_kernel(const int64_t* __restrict__ probes, int B, int nprobe, int* __restrict__ lcount,
                                  int* __restrict__ lq, int cap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * nprobe) return;
    const int64_t L = probes[i];
    if (L < 0) return;
    const int slot = atomicAdd(lcount + L, 1);
    if (slot < cap) lq[(size_t)L * cap + slot] = i;
}

constexpr int IVF_QG = 8;               // queries per pass of the list scan
constexpr int IVF_QLDS = 8192;          // floats of LDS for the query group

// S6: one workgroup per list; exact fp32 cosines of the list's rows against the queries probing it
__global__ __launch_bounds__(256) void ivf_list_scan_kernel(const float* __restrict__ master, const float* __restrict__ qn,
                                                            const int* __restrict__ order,
                                                            const int64_t* __restrict__ offsets,
                                                            const int* __restrict__ lcount, const int* __restrict__ lq,
                                                            int cap, int nprobe, int K, int max_len,
                                                            float* __restrict__ pair_scores) {
    __shared__ __attribute__((aligned(16))) float sq[IVF_QLDS];
    __shared__ int spair[IVF_QG];
    const int L = blockIdx.x;
    const int m = min(lcount[L], cap);
    const int64_t off = offsets[L];
    const int len = (int)(offsets[L + 1] - off);
    if (m == 0 || len == 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qg = min(IVF_QG, IVF_QLDS / K);
    const int nvec = K >> 2;
    for (int g0 = 0; g0 < m; g0 += qg) {
        const int gq = min(qg, m - g0);
        __syncthreads();
        if (tid < gq) spair[tid] = lq[(size_t)L * cap + g0 + tid];
        __syncthreads();
        for (int i = tid; i < gq * K; i += 256) {
            const int j = i / K, d = i - j * K;
            sq[i] = qn[(size_t)(spair[j] / nprobe) * K + d];
        }
        __syncthreads();
        if (K == 1024) {
            // fast path for the reference dimension: two rows per wave in flight, all eight 1-KiB
            // row loads issued before the first use, query fragments read once for both rows
            for (int i = wave * 2; i < len; i += 8) {
                const bool two = i + 1 < len;
                const float4* r0 = reinterpret_cast<const float4*>(master + (size_t)order[off + i] * 1024);
                const float4* r1 = reinterpret_cast<const float4*>(master + (size_t)order[off + (two ? i + 1 : i)] * 1024);
                float4 a0[4], a1[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) { a0[t] = r0[lane + 64 * t]; a1[t] = r1[lane + 64 * t]; }
                float acc0[IVF_QG], acc1[IVF_QG];
#pragma unroll
                for (int j = 0; j < IVF_QG; ++j) {
                    acc0[j] = 0.f; acc1[j] = 0.f;
                    if (j < gq) {
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const float4 b = *reinterpret_cast<const float4*>(&sq[j * 1024 + (lane + 64 * t) * 4]);
                            acc0[j] = fmaf(a0[t].x, b.x, acc0[j]); acc0[j] = fmaf(a0[t].y, b.y, acc0[j]);
                            acc0[j] = fmaf(a0[t].z, b.z, acc0[j]); acc0[j] = fmaf(a0[t].w, b.w, acc0[j]);
                            acc1[j] = fmaf(a1[t].x, b.x, acc1[j]); acc1[j] = fmaf(a1[t].y, b.y, acc1[j]);
                            acc1[j] = fmaf(a1[t].z, b.z, acc1[j]); acc1[j] = fmaf(a1[t].w, b.w, acc1[j]);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < IVF_QG; ++j) {
                    if (j < gq) {
                        const float s0 = wave_sum(acc0[j]) + 0.0f, s1 = wave_sum(acc1[j]) + 0.0f;
                        if (lane == 0) {
                            pair_scores[(size_t)spair[j] * max_len + i] = s0;
                            if (two) pair_scores[(size_t)spair[j] * max_len + i + 1] = s1;
                        }
                    }
                }
            }
            continue;
        }
        for (int i = wave; i < len; i += 4) {
            const float4* rv = reinterpret_cast<const float4*>(master + (size_t)order[off + i] * K);
            float acc[IVF_QG];
#pragma unroll
            for (int j = 0; j < IVF_QG; ++j) acc[j] = 0.f;
            for (int v = lane; v < nvec; v += 64) {
                const float4 a = rv[v];
#pragma unroll
                for (int j = 0; j < IVF_QG; ++j) {
                    if (j < gq) {
                        const float4 b = *reinterpret_cast<const float4*>(&sq[j * K + v * 4]);
                        acc[j] = fmaf(a.x, b.x, acc[j]); acc[j] = fmaf(a.y, b.y, acc[j]);
                        acc[j] = fmaf(a.z, b.z, acc[j]); acc[j] = fmaf(a.w, b.w, acc[j]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < IVF_QG; ++j) {
                if (j < gq) {
                    const float s = wave_sum(acc[j]) + 0.0f;
                    if (lane == 0) pair_scores[(size_t)spair[j] * max_len + i] = s;
                }
            }
        }
    }
}

// S6 (MFMA form), the RING kernel: list_scan_ring below, instantiated for bf16 (ivf_list_scan_mfma_kernel) and int8
// (ivf_list_scan_i8_kernel) operands.  256 rows x up to 64 of the queries that probe the list per tile, 128 bytes of
// every row per K step, 3-stage LDS ring (two K steps in flight).  Scores go to the same per-(query, probe) strips as
// the fp32 kernel above; ivf_select_kernel re-scores the best of them in fp32.  HBM-bound: every probed row is read once
// per group of 64 queries.
constexpr int LS_NST = 3, LS_SEG = 4096;
constexpr int LS_STAGE = (LS_ROWS + LS_Q) * 128;
constexpr int LS_LDS = LS_NST * LS_STAGE + LS_SEG * 4 + LS_Q * 4;

// Stores through inline asm: a store hipcc knows about would make it guard the ring's invisible DMA pieces with
// vmcnt(0).  hipcc pads no hazard whose producer or consumer sits inside an asm string, so the two software wait-state
// rules that touch this store are met INSIDE it ("asm stores"):
//   (a) XDL (MFMA) write of a VGPR -> VMEM read of it as store data: 11 wait states behind an 8-pass MFMA
//       (v_mfma_f32_16x16x32_bf16) -- mfma_results_to_vmem() below, once per epilogue, tied to the accumulators;
//   (b) a VMEM store of more than 8 bytes reads its data registers up to two wait states after it issued: nothing
//       may write them before -- the s_nop 1 that ends the string (a nop in FRONT of the store, r02's encoder attempt,
//       covers nothing: the next v_cvt_pk_bf16_f32 overwrote the registers of the store just issued).
__device__ __forceinline__ void global_store_f4_asm(float* p, f32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
// 12 wait states between the MFMAs that produced `acc` and whatever follows (the "+v" operands keep those MFMAs above)
template <int N, int M>
__device__ __forceinline__ void mfma_results_to_vmem(f32x4 (&acc)[N][M]) {
    static_assert(N == 2 && M == 4, "the list-scan tile: 2 x 4 fragments per wave");
    asm volatile("s_nop 11"
                 : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[0][3]), "+v"(acc[1][0]), "+v"(acc[1][1]),
                   "+v"(acc[1][2]), "+v"(acc[1][3]));
}

typedef __attribute__((ext_vector_type(4))) int i32x4_t;
constexpr int LS_LDS_I8 = LS_NST * LS_STAGE + LS_SEG * 4 + LS_SEG * 4 + LS_Q * 4 + LS_Q * 4;
static_assert(LS_LDS_I8 <= 160 * 1024, "LDS budget of the int8 list scan");

// What the two instantiations of the ring kernel differ in: the operand type and its MFMA, the elements of a 128-byte K
// step, how the global address of a tile row is formed, the LDS arrays behind the ring, the epilogue, and whether the
// pair grid exists.  A traits object holds its kernel's own arguments and LDS pointers.
//
// bf16: rows of the list are gathered from the flat index's bf16 scan copy by their ids (the LDS-DMA takes a per-lane
// source address, so a gather costs nothing extra), v_mfma_f32_16x16x32_bf16; the strips receive the bf16 cosines.
struct RingBf16 {
    typedef bf16x8 vec_t;
    typedef f32x4 acc_t;
    static constexpr int STEP_ELEMS = 64;             // K elements of a step: 128 B per row
    static constexpr size_t STEP_STRIDE = 128;        // bytes from a row's step to its next
    static constexpr bool PAIRS = false;
    const char* scan;
    int pitch;
    const int* order;
    int* sorder;                                      // [LS_SEG] row ids of the segment

    __device__ __forceinline__ int* carve(char* lds) {                       // -> spair
        sorder = reinterpret_cast<int*>(lds);
        return sorder + LS_SEG;
    }
    __device__ __forceinline__ void begin_segment(int L, int seg0) {}
    __device__ __forceinline__ void load_row(int64_t seg_off, int i) { sorder[i] = order[seg_off + i]; }      // (seg_off: the segment in the list order)
    __device__ __forceinline__ void load_query(int tid, int pr, int nprobe) {}
    // global byte offset of 16-byte chunk c of row rr of the segment (in tile i_tile), first K step
    __device__ __forceinline__ size_t row_addr(int i_tile, int rr, int c) const { return (size_t)sorder[rr] * pitch + (c << 4); }
    static __device__ __forceinline__ acc_t mfma(vec_t a, vec_t b, acc_t acc) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0); }
    // the accumulators go to the asm store as they are: rule (a) above global_store_f4_asm
    static __device__ __forceinline__ void results_to_vmem(acc_t (&acc)[2][4]) { mfma_results_to_vmem(acc); }
    __device__ __forceinline__ float query_scale(int col) const { return 0.f; }
    __device__ __forceinline__ f32x4 scores(acc_t acc, int tile_row0, int r, float qs) const { return acc; }
};

// int8 (r03): the same tile, ring and LDS image -- a K step is 128 int8 elements = 128 B per row -- over an int8 copy with
// per-row scales (quant.hip) kept in LIST order: every list is a run of whole 256-row tiles in the flat scan's tiled layout
// (64-B K slices, 16 KiB apart), so a K step of a tile is 32 contiguous KiB -- a stream, where the bf16 form gathers rows
// by id, 128 B at a time -- v_mfma_i32_16x16x64_i8, half the bytes per probed row.  The strips receive ESTIMATED cosines
// (acc x row scale x query scale); ivf_select_kernel re-scores the best of them in fp32 exactly as before.  IVF answers are
// approximate by nature (no certificate): the int8 estimate (error ~2e-3 at most on Gaussian-like rows) only decides which
// kp = max(32, 4k) rows are re-scored.
struct RingI8 {
    typedef i32x4_t vec_t;
    typedef i32x4_t acc_t;
    static constexpr int STEP_ELEMS = 128;            // 128 int8 elements = 128 B per row per K step: the bf16 form's LDS image
    static constexpr size_t STEP_STRIDE = 32768;      // two 64-byte slices of the tile, 16 KiB each
    static constexpr bool PAIRS = true;
    const char* scan;
    int64_t tile_stride;
    const uint32_t* sxi;
    const uint32_t* sqi;
    float unit2;
    const int64_t* tile_off;
    float* sscale;                                    // [LS_SEG] row scales (sxi) of the segment's rows
    float* sqscale;                                   // [LS_Q] unit^2 * sqi of the group's queries
    int64_t tile0;                                    // first tile of the segment in the copy

    __device__ __forceinline__ int* carve(char* lds) {                       // -> spair
        sscale = reinterpret_cast<float*>(reinterpret_cast<int*>(lds) + LS_SEG);      // (behind the bf16 form's [LS_SEG] ids)
        int* spair = reinterpret_cast<int*>(sscale + LS_SEG);
        sqscale = reinterpret_cast<float*>(spair + LS_Q);
        return spair;
    }
    __device__ __forceinline__ void begin_segment(int L, int seg0) { tile0 = tile_off[L] + seg0 / LS_ROWS; }
    __device__ __forceinline__ void load_row(int64_t seg_off, int i) { sscale[i] = (float)sxi[tile0 * LS_ROWS + i]; }
    __device__ __forceinline__ void load_query(int tid, int pr, int nprobe) { sqscale[tid] = unit2 * (float)sqi[pr / nprobe]; }
    // the lane's 16 bytes of a K step: chunk c of the row's 128 B = bytes (c & 3) * 16 of its 64-B slice 2 ks + (c >> 2)
    __device__ __forceinline__ size_t row_addr(int i_tile, int rr, int c) const {
        return (size_t)(tile0 + i_tile) * tile_stride + (size_t)(c >> 2) * 16384 + (rr - i_tile * LS_ROWS) * 64 + (c & 3) * 16;
    }
    static __device__ __forceinline__ acc_t mfma(vec_t a, vec_t b, acc_t acc) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0); }
    static __device__ __forceinline__ void results_to_vmem(acc_t (&acc)[2][4]) {}
    __device__ __forceinline__ float query_scale(int col) const { return sqscale[col]; }
    // estimated cosines: acc * (sxi[row] unit) * (sqi[query] unit); the conversions are VALU instructions hipcc sees (it
    // pads the MFMA -> VALU distance), their results feed the asm store
    __device__ __forceinline__ f32x4 scores(acc_t acc, int tile_row0, int r, float qs) const {
        const f32x4 rs = *reinterpret_cast<const f32x4*>(sscale + tile_row0 + r);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)acc[e] * rs[e] * qs;
        return v;
    }
};

// Two grids.  List mode (n_pairs == 0): one workgroup per list, every query that probes it.  Pair mode (T::PAIRS; a handful of
// queries: fewer probed lists than CUs, and a CU takes in ~25 GB/s): one workgroup per (query, probe) pair and SEGMENT of its
// list -- `split` workgroups share a list's tiles, so one query's 32 lists are read by a few hundred CUs instead of 32.
// (The loop that stages a segment's rows stays here, with load_row per row, and scores() takes the tile's first row and the
// row inside it apart: either way round hipcc shapes these two places differently -- profiles/ivf_split/NOTES.md.)
template <class T>
__device__ __forceinline__ void list_scan_ring(T t, const char* qb_b, int qpitch, const int64_t* __restrict__ offsets,
                                               const int* __restrict__ lcount, const int* __restrict__ lq, int cap, int nprobe, int K,
                                               int max_len, float* __restrict__ pair_scores, const int64_t* __restrict__ probes,
                                               int n_pairs, int split) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* spair = t.carve(smem + LS_NST * LS_STAGE);
    const bool pair_mode = T::PAIRS && n_pairs > 0;
    int L, m, seg = 0, pair0 = 0;
    if (pair_mode) {
        pair0 = (int)blockIdx.x / split;
        seg = (int)blockIdx.x % split;
        const int64_t l64 = probes[pair0];
        if (l64 < 0) return;
        L = (int)l64;
        m = 1;
    } else {
        L = blockIdx.x;
        m = min(lcount[L], cap);
    }
    const int64_t off = offsets[L];
    const int len_all = (int)(offsets[L + 1] - off);
    if (m == 0 || len_all == 0) return;
    int row_lo = 0, row_hi = len_all;
    if (pair_mode && split > 1) {
        const int nt_all = (len_all + LS_ROWS - 1) / LS_ROWS, per = (nt_all + split - 1) / split;
        row_lo = min(len_all, seg * per * LS_ROWS);
        row_hi = min(len_all, (seg + 1) * per * LS_ROWS);
        if (row_lo >= row_hi) return;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int KS = K / T::STEP_ELEMS;
    const int chunk_lo = lane & 7, r_in_piece = lane >> 3;

    for (int seg0 = row_lo; seg0 < row_hi; seg0 += LS_SEG) {
        const int len = min(LS_SEG, row_hi - seg0);
        __syncthreads();
        t.begin_segment(L, seg0);
        for (int i = tid; i < len; i += 512) t.load_row(off + seg0, i);
        const int n_tiles = (len + LS_ROWS - 1) / LS_ROWS;
        for (int g0 = 0; g0 < m; g0 += LS_Q) {
            const int gq = min(LS_Q, m - g0);
            __syncthreads();
            if (tid < LS_Q) {
                const int pr = pair_mode ? pair0 : lq[(size_t)L * cap + g0 + min(tid, gq - 1)];
                spair[tid] = pr;
                t.load_query(tid, pr, nprobe);
            }
            __syncthreads();
            // this lane's query row of the one Q piece its wave issues per stage
            const int qj = wave * 8 + r_in_piece;
            const size_t qoff = (size_t)(spair[qj] / nprobe) * qpitch + ((chunk_lo ^ ((qj >> 1) & 7)) << 4);

            const int total = n_tiles * KS;
            int i_tile = -1, i_ks = KS - 1;                 // issue cursor
            size_t aoff[4];
            auto issue = [&](int s) {
                if (++i_ks == KS) {                         // the cursor enters a new tile: its rows' addresses
                    i_ks = 0;
                    ++i_tile;
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        const int r = (wave + 8 * it) * 8 + r_in_piece;
                        const int rr = min(i_tile * LS_ROWS + r, len - 1);          // rows past the end repeat the last one (same tile)
                        aoff[it] = t.row_addr(i_tile, rr, chunk_lo ^ ((r >> 1) & 7));
                    }
                }
                char* buf = smem + (s % LS_NST) * LS_STAGE;
#pragma unroll
                for (int it = 0; it < 4; ++it) lds_dma16(t.scan + aoff[it] + (size_t)i_ks * T::STEP_STRIDE, buf + (wave + 8 * it) * 1024);
                lds_dma16(qb_b + qoff + (size_t)i_ks * 128, buf + LS_ROWS * 128 + wave * 1024);
            };
            for (int s = 0; s < LS_NST - 1 && s < total; ++s) issue(s);
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);

            typename T::acc_t acc[2][4];
            int ks = 0, tile = 0;
            for (int s = 0; s < total; ++s) {
                const bool more = s + LS_NST - 1 < total;
                if (more) issue(s + LS_NST - 1);
                if (ks == 0) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[i][j] = typename T::acc_t{0, 0, 0, 0};
                }
                const char* tA = smem + (s % LS_NST) * LS_STAGE;
                const char* tB = tA + LS_ROWS * 128;
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    typename T::vec_t a[2], b[4];
                    const int c = kk * 4 + (lane >> 4);
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int r = wave * 32 + i * 16 + (lane & 15);
                        a[i] = *reinterpret_cast<const typename T::vec_t*>(tA + r * 128 + ((c ^ ((r >> 1) & 7)) << 4));
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = j * 16 + (lane & 15);
                        b[j] = *reinterpret_cast<const typename T::vec_t*>(tB + r * 128 + ((c ^ ((r >> 1) & 7)) << 4));
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[i][j] = T::mfma(a[i], b[j], acc[i][j]);
                }
                if (++ks == KS) {
                    // scores of this tile: a lane holds 4 consecutive rows of one query per fragment
                    T::results_to_vmem(acc);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int col = j * 16 + (lane & 15);
                        if (col < gq) {
                            float* strip = pair_scores + (size_t)spair[col] * max_len + seg0 + tile * LS_ROWS;
                            const float qs = t.query_scale(col);
#pragma unroll
                            for (int i = 0; i < 2; ++i) {
                                const int r = wave * 32 + i * 16 + (lane >> 4) * 4;
                                if (tile * LS_ROWS + r < len)      // len and max_len are padded reads, not padded strips:
                                    global_store_f4_asm(strip + r, t.scores(acc[i][j], tile * LS_ROWS, r, qs));
                            }
                        }
                    }
                    ks = 0;
                    ++tile;
                }
                if (more) asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

__global__ __launch_bounds__(512) void ivf_list_scan_mfma_kernel(const bf16_t* __restrict__ scan, int pitch,
                                                                 const bf16_t* __restrict__ qb, int qpitch,
                                                                 const int* __restrict__ order,
                                                                 const int64_t* __restrict__ offsets,
                                                                 const int* __restrict__ lcount, const int* __restrict__ lq,
                                                                 int cap, int nprobe, int K, int max_len,
                                                                 float* __restrict__ pair_scores) {
    list_scan_ring(RingBf16{reinterpret_cast<const char*>(scan), pitch, order, nullptr}, reinterpret_cast<const char*>(qb), qpitch, offsets,
                   lcount, lq, cap, nprobe, K, max_len, pair_scores, nullptr, 0, 1);
}

__global__ __launch_bounds__(512) void ivf_list_scan_i8_kernel(const int8_t* __restrict__ scan, int64_t tile_stride, const uint32_t* __restrict__ sxi,
                                                               const int8_t* __restrict__ qb, int qpitch, const uint32_t* __restrict__ sqi, float unit2,
                                                               const int64_t* __restrict__ tile_off,
                                                               const int64_t* __restrict__ offsets,
                                                               const int* __restrict__ lcount, const int* __restrict__ lq,
                                                               int cap, int nprobe, int K, int max_len,
                                                               float* __restrict__ pair_scores,
                                                               const int64_t* __restrict__ probes, int n_pairs, int split) {
    list_scan_ring(RingI8{reinterpret_cast<const char*>(scan), tile_stride, sxi, sqi, unit2, tile_off, nullptr, nullptr, 0},
                   reinterpret_cast<const char*>(qb), qpitch, offsets, lcount, lq, cap, nprobe, K, max_len, pair_scores, probes, n_pairs, split);
}

// r04: STREAMING form of the int8 list scan -- the rows never touch LDS.  The tiled int8 copy keeps the 64-byte K slice h of
// tile row r at h * 16 KiB + r * 64, so the A operand of v_mfma_i32_16x16x64_i8 for 16 consecutive rows and one slice -- lane l:
// row l & 15, bytes (l >> 4) * 16 .. + 15 -- is ONE contiguous KiB: a wave loads it with a single global_load_dwordx4 straight into
// the operand registers.  No staging ring, no DMA pieces, no workgroup barrier in the loop: every wave streams its own 64 rows of
// each tile through a register ring of ST_RING fragments (16 KiB in flight per wave; workgroups of four waves, two or more per CU:
// one loads its queries while the other streams; hipcc counts the vmcnt waits -- the loads are plain loads), and only the few queries
// that probe the list (8 on average at batch 1024, nprobe 32 of 4096) sit in LDS, loaded once per unit.  The staged kernel above kept 2 x 40 KiB in flight per CU behind one
// barrier per K step and re-sent the query block with every step: 0.50 of HBM at batch 1024 (profiles/r03_configs/cfg_ivf.json).
// A workgroup takes one UNIT: up to ST_UNIT_TILES consecutive tiles of one list (table built with the lists), so long lists
// spread over several CUs and the grid is a few thousand even units.  Strips receive estimated cosines as before.

// issue cursor of a wave's stream: the next K slice (its ST_FR fragments)
struct StCursor {
    const char* tile;                     // base of the cursor's tile (+ the wave's rows)
    int h;                                // its K slice
    // r04c: a list ends inside its last tile (2,441 rows on average = 9.5 tiles: 5 % of the copy is padding).  The wave's fragments of
    // that tile that lie wholly behind the list's end are read from `dummy` -- a KiB every unit keeps hot in L2 (the head of the query
    // block) -- instead of from HBM: their scores are dropped by the row < len tests anyway.  A select on the address, no branch.
    const char* last;                     // the list's last tile if it is partial and belongs to this unit (else null)
    int nvalid;                           // fragments of this wave in it that hold rows of the list
    const char* dummy;
};
__device__ __forceinline__ void st_issue_slice(StCursor& c, int HS, int64_t tile_stride, unsigned aoff, i32x4_t* r) {
    const char* p = c.tile + (size_t)c.h * 16384 + aoff;
    const bool pad = c.tile == c.last;
#pragma unroll
    for (int f = 0; f < ST_FR; ++f) {
        const char* pf = (pad && f >= c.nvalid) ? c.dummy + aoff : p + f * 1024;
#ifdef SQE_ST_NO_NT              // (timing build: default cache policy)
        r[f] = *reinterpret_cast<const i32x4_t*>(pf);
#else
        r[f] = __builtin_nontemporal_load(reinterpret_cast<const i32x4_t*>(pf));
#endif
    }
    if (++c.h == HS) { c.h = 0; c.tile += tile_stride; }
}
// ST_SL K slices: the fragments of the ring against the query fragments of slices hb .. hb + ST_SL - 1 (bq: this lane's query
// row in LDS + hb * 64).  ISSUE: a slice's registers are refilled, as soon as they have been read, with the slice ST_SL ahead.
// The refill is unconditional inside this body and the LAST group of a unit (ISSUE = false) is code of its own behind the loop: with
// a branch around the loads hipcc has to assume the path without them at every join and waits for vmcnt(0) in front of each use --
// the ring drained at every step (first version of this kernel); this way it counts vmcnt(12) in the steady state.
template <bool ISSUE>
__device__ __forceinline__ void st_group(i32x4_t (&ring)[ST_RING], i32x4_t (&acc)[ST_FR][2], const char* bq, int qrow, int bcq, int bsw, StCursor& c,
                                         int HS, int64_t tile_stride, unsigned aoff) {
#pragma unroll
    for (int e = 0; e < ST_SL; ++e) {
        const int boff = ((e * 4 + bcq) ^ bsw) << 4;
        const i32x4_t b0 = *reinterpret_cast<const i32x4_t*>(bq + boff);
        const i32x4_t b1 = *reinterpret_cast<const i32x4_t*>(bq + 16 * qrow + boff);
#pragma unroll
        for (int f = 0; f < ST_FR; ++f) {
            acc[f][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ring[e * ST_FR + f], b0, acc[f][0], 0, 0, 0);
            acc[f][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ring[e * ST_FR + f], b1, acc[f][1], 0, 0, 0);
        }
        if (ISSUE) st_issue_slice(c, HS, tile_stride, aoff, &ring[e * ST_FR]);
    }
}

constexpr int ST_CBUF = 1024;  // keys a workgroup can hold back per unit and pass (~40 expected)
template <bool COLLECT>
__global__ __launch_bounds__(ST_THREADS) void ivf_list_stream_i8_kernel(const int8_t* __restrict__ scan, int64_t tile_stride, const uint32_t* __restrict__ sxi,
                                                                        const int8_t* __restrict__ qb, int qpitch, const uint32_t* __restrict__ sqi, float unit2,
                                                                        const int4* __restrict__ units, const int64_t* __restrict__ tile_off,
                                                                        const int64_t* __restrict__ offsets, const int* __restrict__ lcount,
                                                                        const int* __restrict__ lq, int cap, int nprobe, int K, int max_len,
                                                                        float* __restrict__ pair_scores, StCollect col, const int* __restrict__ gate,
                                                                        int* __restrict__ queue, int n_units,
                                                                        const int64_t* __restrict__ pair_probes, int pair_tiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_next;
    if (gate && *gate == 0) return;                            // (the strip-mode fallback of a collect search: only if some query asked for it)
    // queue != null: PERSISTENT workgroups (two per CU) take units from a counter -- ~12 k workgroups of ~100 us each otherwise, and the
    // stream read at 5.5 TB/s where the flat small-batch kernel, persistent, reads at 6.5
    for (int unit = blockIdx.x;;) {
    if (queue) {
        __syncthreads();                                       // (the previous unit is done with LDS)
        if (threadIdx.x == 0) s_next = atomicAdd(queue, 1);
        __syncthreads();
        unit = s_next;
    }
    if (unit >= n_units) return;
    const int qrow = K + 128;                                  // LDS pitch of a query row: rows r and r + 1 start 32 banks apart
    float* sscale = reinterpret_cast<float*>(smem + ST_Q * qrow);          // [ST_UNIT_TILES * 256] row scales of the unit
    int* spair = reinterpret_cast<int*>(sscale + ST_UNIT_TILES * LS_ROWS);
    float* sqscale = reinterpret_cast<float*>(spair + ST_Q);
    // per wave: ST_PATCH_ROWS query rows of [64 rows + 4] floats: the transposed scores of finished tiles, waiting for their stores
    float* spatch = sqscale + ST_Q + (threadIdx.x >> 6) * (ST_PATCH_ROWS * ST_PATCH_PITCH);
    // COLLECT: the patch region holds the workgroup's key buffer instead: [ST_CBUF] keys, [ST_CBUF] query columns, a counter, thresholds
    uint64_t* cbuf_key = reinterpret_cast<uint64_t*>(sqscale + ST_Q);
    unsigned char* cbuf_col = reinterpret_cast<unsigned char*>(cbuf_key + ST_CBUF);
    int* cbuf_n = reinterpret_cast<int*>(cbuf_col + ST_CBUF);
    float* sthr = reinterpret_cast<float*>(cbuf_n + 4);        // [ST_Q]
    // pair_probes != null (a handful of queries, no queue): the grid is (query, probe) pair x tile of its list -- a few hundred workgroups
    // that all have work.  The unit table of single tiles it replaces is ~40 k workgroups for 10 M rows, of which one query uses 320:
    // handing the others their table entry and list count took most of the 72 us this launch lasted (r04c).
    int4 u;
    int m;
    if (pair_probes) {
        const int pair = unit / pair_tiles;
        const int64_t Lp = pair_probes[pair];
        if (Lp < 0) return;
        u = make_int4((int)Lp, unit - pair * pair_tiles, 1, pair);
        if (u.y >= (int)(tile_off[Lp + 1] - tile_off[Lp])) return;
        m = 1;
    } else {
        u = units[unit];
        m = min(lcount[u.x], cap);
    }
    const int L = u.x, ntiles = u.z;
    if (m == 0) {                                              // nobody probes this list
        if (!queue) return;
        continue;
    }
    const int64_t loff = offsets[L];
    const int len_all = (int)(offsets[L + 1] - loff);
    const int row0 = u.y * LS_ROWS;                            // first row of the unit inside its list
    const int64_t gt0 = tile_off[L] + u.y;                     // ... and its first tile in the copy
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int HS = K >> 6;                                     // 64-byte K slices per row (a multiple of ST_SL: the launcher checks)
    const int GPT = HS / ST_SL;                                // groups per tile
    // this lane's 16 bytes of a fragment: row (lane & 15) of a 16-row block, bytes (lane >> 4) * 16 of its slice
    const char* abase = reinterpret_cast<const char*>(scan) + gt0 * tile_stride + wave * (ST_FR * 1024);
    // (StCursor: the wave's fragments behind the end of the list, when the list's partial last tile is this unit's last)
    const int list_tiles = (len_all + LS_ROWS - 1) / LS_ROWS;
    const int pad_nvalid = min(ST_FR, max(0, (len_all - (list_tiles - 1) * LS_ROWS - wave * (ST_FR * 16) + 15) >> 4));
    const char* pad_tile = (u.y + ntiles == list_tiles && pad_nvalid < ST_FR) ? abase + (int64_t)(ntiles - 1) * tile_stride : nullptr;
#ifdef SQE_ST_NATURAL            // (timing build, results wrong: lane-contiguous addresses -- what a fragment-major copy would read)
    const unsigned aoff = (unsigned)(lane * 16);
#else
    const unsigned aoff = (unsigned)((lane & 15) * 64 + (lane >> 4) * 16);
#endif
    // ... and of a query fragment in LDS: row j * 16 + (lane & 15), chunk (h * 4 + (lane >> 4)) ^ ((row >> 1) & 7)
    const int br = lane & 15, bsw = (br >> 1) & 7, bcq = lane >> 4;
    const char* bbase = smem + br * qrow;
    for (int i = tid; i < ntiles * LS_ROWS; i += ST_THREADS) sscale[i] = (float)sxi[gt0 * LS_ROWS + i];

    for (int g0 = 0; g0 < m; g0 += ST_Q) {
        const int gq = min(ST_Q, m - g0);
        __syncthreads();                                       // the previous pass is done with the query block
        if (tid < ST_Q) {
            const int pr = pair_probes ? u.w : lq[(size_t)L * cap + g0 + min(tid, gq - 1)];
            spair[tid] = pr;
            sqscale[tid] = unit2 * (float)sqi[pr / nprobe];
            if (COLLECT) sthr[tid] = tid < gq ? col.thr[pr / nprobe] : INFINITY;
        }
        if (COLLECT && tid == 0) *cbuf_n = 0;
        __syncthreads();
        {
            const int cpr = K >> 4;                            // 16-byte chunks per query row
            for (int c = tid; c < gq * cpr; c += ST_THREADS) {   // (rows >= gq keep stale bytes: their columns are never stored or compared)
                const int r = c / cpr, cc = c - r * cpr;
                const i32x4_t v = *reinterpret_cast<const i32x4_t*>(qb + (size_t)(spair[r] / nprobe) * qpitch + cc * 16);
                *reinterpret_cast<i32x4_t*>(smem + r * qrow + ((cc ^ ((r >> 1) & 7)) << 4)) = v;
            }
        }
        __syncthreads();

        // ---- the stream: group g = slices (g % GPT) * ST_SL .. of tile g / GPT; the ring holds group g while group g + 1 is on its way
        i32x4_t ring[ST_RING];
        StCursor cur{abase, 0, pad_tile, pad_nvalid, reinterpret_cast<const char*>(qb)};
#pragma unroll
        for (int e = 0; e < ST_SL; ++e) st_issue_slice(cur, HS, tile_stride, aoff, &ring[e * ST_FR]);
        i32x4_t acc[ST_FR][2];
#pragma unroll
        for (int i = 0; i < ST_FR; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = i32x4_t{0, 0, 0, 0};
        // Scores of a finished tile.  A lane holds 4 consecutive rows of ONE query per fragment: the wave transposes its 64 rows x gq
        // queries through a private LDS patch, so that 16 lanes hold the 256 contiguous bytes of one query's 64 rows (four queries per
        // store instruction).  WHEN the stores leave matters more than their shape: vector-memory operations retire in issue order, so a
        // row fragment loaded behind a store cannot be consumed before that store has been acknowledged -- a stall of one store latency
        // per tile (measured: 2.03 ms with the stores behind every tile, in 64-byte segments or 256-byte runs alike, 1.61 ms without
        // stores; profiles/r04_configs/ivf_stream_ablation.log).  The patches of up to four tiles therefore wait in LDS (as many as fit:
        // 36 query rows of 64 scores per wave) and leave together -- for the usual handful of probing queries once per unit, behind
        // its last load.
        const int gq_pad = (gq + 3) & ~3;
        const int max_slots = ST_PATCH_ROWS / gq_pad;          // tiles whose patches fit (gq <= 32: at least one)
        int nslot = 0, slot_t0 = 0;
        auto flush = [&]() {
            const int r4 = (lane & 15) * 4;                    // this lane's 4 rows of the wave's 64
            for (int sl = 0; sl < nslot; ++sl) {
                const int wrow = row0 + (slot_t0 + sl) * LS_ROWS + wave * (ST_FR * 16) + r4;   // row inside the list
                const float* patch = spatch + sl * gq_pad * ST_PATCH_PITCH;
                for (int c0 = 0; c0 < gq; c0 += 4) {
                    const int col = c0 + (lane >> 4);
                    if (col < gq && wrow < len_all) {          // (strips are padded to 4 floats: max_len)
                        const f32x4 v = *reinterpret_cast<const f32x4*>(patch + col * ST_PATCH_PITCH + r4);
#ifdef SQE_ST_NO_STORE           // (timing build, results wrong: no strip stores unless a score is NaN)
                        if (v[0] != v[0])
#endif
                        *reinterpret_cast<f32x4*>(pair_scores + (size_t)spair[col] * max_len + wrow) = v;
                    }
                }
            }
            nslot = 0;
        };
        auto write_tile = [&](int t, bool last) {
            if (COLLECT) {
                // keys at or above the query's threshold into the workgroup's buffer (LDS atomics: nothing here enters the vector-memory queue)
                const int trow = row0 + t * LS_ROWS + wave * (ST_FR * 16);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int c = j * 16 + (lane & 15);
                    const float qs = sqscale[c], th = sthr[c];
#pragma unroll
                    for (int i = 0; i < ST_FR; ++i) {
                        const int r = i * 16 + (lane >> 4) * 4;
                        const f32x4 rs = *reinterpret_cast<const f32x4*>(sscale + t * LS_ROWS + wave * (ST_FR * 16) + r);
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = (float)acc[i][j][e] * rs[e] * qs;
                        const float m4 = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
                        if (__any(m4 >= th)) {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (v[e] >= th && trow + r + e < len_all) {
                                    const int at = atomicAdd(cbuf_n, 1);
                                    if (at < ST_CBUF) {
                                        cbuf_key[at] = make_key(v[e], (uint32_t)(trow + r + e));     // (row = position inside the list, for now)
                                        cbuf_col[at] = (unsigned char)c;
                                    } else {
                                        // the buffer is full (a crowd: every row of the unit passes for some query): straight to the list -- the
                                        // atomic's return drains this wave's ring, once in a long while
                                        const int q = spair[c] / nprobe;
                                        const int slot = atomicAdd(col.cnt + q, 1);
                                        if (slot < col.list_cap)
                                            col.list[(size_t)q * col.list_cap + slot] = make_key(v[e], (uint32_t)col.order[loff + trow + r + e]);
                                    }
                                }
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < ST_FR; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = i32x4_t{0, 0, 0, 0};
                return;
            }
            if (nslot == 0) slot_t0 = t;
            float* patch = spatch + nslot * gq_pad * ST_PATCH_PITCH;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = j * 16 + (lane & 15);
                if (col < gq_pad) {
                    const float qs = sqscale[col];
#pragma unroll
                    for (int i = 0; i < ST_FR; ++i) {
                        const int r = i * 16 + (lane >> 4) * 4;    // row inside the wave's 64
                        const f32x4 rs = *reinterpret_cast<const f32x4*>(sscale + t * LS_ROWS + wave * (ST_FR * 16) + r);
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = (float)acc[i][j][e] * rs[e] * qs;
                        *reinterpret_cast<f32x4*>(patch + col * ST_PATCH_PITCH + r) = v;
                    }
                }
            }
            // (wave-private patches: the LDS operations of a wave execute in order, no barrier)
            if (++nslot == max_slots || last) flush();
#pragma unroll
            for (int i = 0; i < ST_FR; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = i32x4_t{0, 0, 0, 0};
        };
        const int n_grp = ntiles * GPT;
        int gt = 0, t = 0;                                     // group inside its tile, tile
        for (int g = 0; g + 1 < n_grp; ++g) {
            st_group<true>(ring, acc, bbase + gt * ST_SL * 64, qrow, bcq, bsw, cur, HS, tile_stride, aoff);
            if (++gt == GPT) {
                write_tile(t, false);
                gt = 0;
                ++t;
            }
        }
        st_group<false>(ring, acc, bbase + gt * ST_SL * 64, qrow, bcq, bsw, cur, HS, tile_stride, aoff);
        write_tile(t, true);
        if (COLLECT) {
            __syncthreads();                                   // every wave's keys are in the buffer; no load is in flight any more
            const int n = *cbuf_n;
            const int64_t off = loff;
            for (int i = tid; i < min(n, ST_CBUF); i += ST_THREADS) {
                const uint64_t key = cbuf_key[i];
                const int q = spair[cbuf_col[i]] / nprobe;
                const int slot = atomicAdd(col.cnt + q, 1);
                if (slot < col.list_cap) col.list[(size_t)q * col.list_cap + slot] = make_key(key_score(key), (uint32_t)col.order[off + key_row(key)]);
            }
        }
    }
    if (!queue) return;
    }
}

}  // namespace

int launch_ivf_bucket(const int64_t* probes, int B, int nprobe, int* lcount, int* lq, hipStream_t s) {
    hipLaunchKernelGGL(ivf_bucket_kernel, dim3((B * nprobe + 255) / 256), dim3(256), 0, s, probes, B, nprobe, lcount, lq, B);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_ivf_list_scan_f32(const float* master, const float* qn, const int* order, const ListScan& a, hipStream_t s) {
    hipLaunchKernelGGL(ivf_list_scan_kernel, dim3(a.nlist), dim3(256), 0, s, master, qn, order, a.offsets, a.lcount, a.lq, a.cap, a.nprobe,
                       a.dim, a.max_len, a.pair_scores);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_ivf_list_scan_bf16(const bf16_t* scan, int pitch, const bf16_t* qb, int qpitch, const int* order, const ListScan& a, hipStream_t s) {
    SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(ivf_list_scan_mfma_kernel), LS_LDS));
    hipLaunchKernelGGL(ivf_list_scan_mfma_kernel, dim3(a.nlist), dim3(512), LS_LDS, s, scan, pitch, qb, qpitch, order, a.offsets, a.lcount,
                       a.lq, a.cap, a.nprobe, a.dim, a.max_len, a.pair_scores);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_ivf_list_scan_i8(const ListScanI8& c, const ListScan& a, const int64_t* probes, int n_pairs, int split, hipStream_t s) {
    SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(ivf_list_scan_i8_kernel), LS_LDS_I8));
    hipLaunchKernelGGL(ivf_list_scan_i8_kernel, dim3(n_pairs ? n_pairs * split : a.nlist), dim3(512), LS_LDS_I8, s, c.rows, c.tile_stride,
                       c.sxi, c.q8, c.q8_pitch, c.sqi, c.unit2, c.tile_off, a.offsets, a.lcount, a.lq, a.cap, a.nprobe, a.dim, a.max_len,
                       a.pair_scores, probes, n_pairs, split);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_ivf_list_stream_i8(const ListScanI8& c, const ListScan& a, const int4* units, int n_units, const StCollect* col, const int* gate,
                              int* queue, int persistent, const int64_t* pair_probes, int pair_tiles, hipStream_t s) {
    if (a.dim % (64 * ST_SL) != 0) return fail(SQE_ERR_INVALID, "ivf stream scan: dim must be a multiple of 256");
    const size_t lds = ivf_stream_lds(a.dim);
    auto kern = col ? ivf_list_stream_i8_kernel<true> : ivf_list_stream_i8_kernel<false>;
    SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), (int)lds));
    hipLaunchKernelGGL(kern, dim3(queue ? persistent : n_units), dim3(ST_THREADS), lds, s, c.rows, c.tile_stride, c.sxi, c.q8, c.q8_pitch,
                       c.sqi, c.unit2, units, c.tile_off, a.offsets, a.lcount, a.lq, a.cap, a.nprobe, a.dim, a.max_len, a.pair_scores,
                       col ? *col : StCollect{}, gate, queue, n_units, pair_probes, pair_tiles);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

}  // namespace sqe
