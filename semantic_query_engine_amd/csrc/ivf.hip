// ivf.hip -- IVF-flat on top of the flat index (BASELINE config 5: nlist = 4096, nprobe = 32).  Host code only: the
// kernels are in ivf_scan.hip, ivf_select.hip and ivf_build.hip behind the launchers of ivf_kernels.h; the quantisers of
// the int8 copy are in quant.hip.  Every call runs under the base index's lock, on the stream it is given (internal.h).
//
//   train   spherical k-means (Lloyd): assignment = cosine top-1 of the sample against the current centroids
//           (ivf_coarse_topk, S7 "assign"), update = segmented sum by fp32 atomics + renormalise (S7 "update")
//   add     rows are stored by the base flat index (fp32 master + bf16 copy); each row is assigned to its best
//           centroid; the inverted lists (row ids grouped by list), the unit tables of the streaming scan and the
//           list-ordered int8 copy are rebuilt lazily, by the first search after a change
//   search  S5 coarse quantise: the [B, nlist] scores as one small bf16 GEMM, a radix select and an fp32 re-score of the
//           best nprobe + 8 lists (the flat index over the centroids where nlist does not allow the GEMM).
//           S6 list scan: ESTIMATED cosines of the probed lists' rows, by the route ivf_route_plan picks:
//             int8 streaming (dim a multiple of 256 whose query block fits the LDS of two workgroups per CU): the rows of
//               the list-ordered int8 copy go straight into the MFMA operand registers, one workgroup per unit of <= 5
//               tiles of a list.  More than 512 (query, probe) pairs: COLLECT mode -- a sample pass over the first tile
//               of every list gives each query a threshold, the pass over the other tiles keeps only the keys at or above
//               it, and ivf_select_list_kernel ranks each query's list; a query whose list cannot answer raises a flag
//               and two gated launches redo the batch through the strips.  Up to 512 pairs: scores to per-(query, probe)
//               strips, over a grid of pairs x tiles (or single-tile units when one list is very long);
//             int8 staged (other dims from 256 that are multiples of 128): the same copy through a 3-stage LDS ring, one
//               workgroup per list, or per pair and segment of its list for up to 512 pairs;
//             bf16 (every other dim): rows gathered from the flat index's bf16 scan copy by id through the same ring.
//           Select: per query, the kp = max(32, 4 k) best estimates are re-scored in fp32 against the master and the
//           top-k by (fp32 cosine desc, row id asc) returned.  IVF answers are approximate by nature (no certificate):
//           the estimate only decides which kp rows are re-scored.
//
// The list scan is HBM-bound: with B = 1024 and nprobe = 32 nearly every list is probed, so one batch reads the int8
// copy about once (10 GB at N = 10M, dim 1024).
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "internal.h"
#include "ivf_kernels.h"

namespace sqe {

namespace {

uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace

struct IvfState {
    sqe_index* coarse = nullptr;       // flat index over the centroids
    bool trained = false;
    bool lists_dirty = true;
    bool cent_dirty = true;            // dense bf16 copy of the centroids (coarse GEMM) is stale
    int64_t n_assigned = 0;            // rows of the base index that have an assignment
    int max_len = 0;
    DevBuf centroids, assign, order, offsets, counts, cursor;   // device
    // int8 list scan (r03): int8 copy of the base rows IN LIST ORDER at i8_pitch bytes + per-row scales, (re)built lazily
    DevBuf i8rows, i8sxi, q8, q8sqi, tile_off, dpos;
    int64_t i8_cap = 0, i8_done = 0, total_tiles = 0;    // i8_cap: tiles allocated
    int64_t i8_tile_stride = 0;
    bool use_i8 = true;              // knobs build: SQE_IVF_I8=0 keeps the bf16 list scan (A/B)
    DevBuf units4, units1;           // work units of the streaming list scan: (list, first tile in the list, tiles, 0), <= ST_UNIT_TILES tiles / 1 tile each
    int n_units4 = 0, n_units1 = 0;
    DevBuf unitsS, unitsR;           // collect mode: the first tile of every list (the sample) / the other tiles in runs of <= 4
    int n_unitsS = 0, n_unitsR = 0;
    DevBuf cthr, ccnt, clist;        // collect mode, per search: thresholds [B], list lengths [B], lists [B, IVF_LIST_CAP]
    DevBuf qn, qb, qd, cent_bf16, cscores, probes_cos, probes_ids, lcount, lq, pair_scores, tmp_ids, tmp_cos, sums;
    std::vector<int64_t> h_offsets;
    // test-only record of the last search piece (sqe_index_ivf_state[_read]): written by the host branches that launch
    sqe_ivf_state_t rec{};
    bool rec_valid = false;
    int coarse_route = 0;            // SQE_IVF_COARSE_* of the last ivf_coarse_topk
};

// Top-kk lists of b rows (raw fp32, normalised here) against the centroids.  A few thousand centroids are too
// few rows for the streaming scan (its chunks could not even fill the global-bound table), so when nlist
// allows it the whole [b, nlist] score matrix is one small GEMM (dense bf16 copies of both sides, fp32 out,
// the encoder's ring GEMM) followed by a per-row radix select; otherwise the flat index over the centroids.
static int ivf_coarse_topk(sqe_index* base, IvfState* st, const float* rows_dev, int64_t b, int kk, int64_t* ids_out,
                           float* cos_out, hipStream_t s) {
    sqe_ctx* ctx = base->ctx;
    const int nlist = base->nlist, dim = base->dim;
    const bool dense = nlist % 128 == 0 && (size_t)nlist * 4 <= 64 * 1024 && kk + 8 <= MAX_KP;
    if (!dense) {
        st->coarse_route = SQE_IVF_COARSE_FLAT;
        return index_search_impl(st->coarse, rows_dev, (int)b, kk, 0, cos_out, ids_out, s);
    }
    st->coarse_route = SQE_IVF_COARSE_DENSE;
    if (st->cent_dirty) {
        SQE_TRY(st->cent_bf16.ensure((size_t)nlist * dim * 2));
        SQE_TRY(launch_normalize_rows(st->coarse->master, nlist, dim, dim, nullptr, st->cent_bf16.as<bf16_t>(), dim, nullptr, nullptr, s));
        st->cent_dirty = false;
    }
    const int64_t step = 16384;
    const int64_t cap = std::min(step, (b + 127) / 128 * 128);
    SQE_TRY(st->qd.ensure((size_t)cap * dim * 2));
    SQE_TRY(st->cscores.ensure((size_t)cap * nlist * 4));
    for (int64_t off = 0; off < b; off += step) {
        const int m = (int)std::min(step, b - off);
        const int t_pad = (m + 127) / 128 * 128;
        // (rows m .. t_pad of qd keep whatever they held: the GEMM computes their scores and stores none of them)
        SQE_TRY(launch_normalize_rows(rows_dev + (size_t)off * dim, m, dim, dim, nullptr, st->qd.as<bf16_t>(), dim, nullptr, nullptr, s));
        SQE_TRY(launch_scores_gemm(st->cent_bf16.as<bf16_t>(), st->qd.as<bf16_t>(), st->cscores.as<float>(), nlist, dim, m, t_pad,
                                   ctx->cu_count, s));
        SQE_TRY(launch_ivf_probe_select(st->cscores.as<float>(), m, nlist, kk, rows_dev + (size_t)off * dim, st->coarse->master, dim,
                                        ids_out + off * kk, cos_out + off * kk, s));
    }
    return SQE_OK;
}

static int ivf_assign_rows(sqe_index* base, IvfState* st, const float* rows_dev, int64_t n, int* assign_out,
                           int64_t* ids64_out /* optional [n] */, hipStream_t s) {
    // cosine top-1 of `rows_dev` against the centroids, in batches
    const int dim = base->dim;
    const int64_t batch = 65536;
    SQE_TRY(st->tmp_ids.ensure((size_t)std::min(batch, n) * 8));
    SQE_TRY(st->tmp_cos.ensure((size_t)std::min(batch, n) * 4));
    for (int64_t off = 0; off < n; off += batch) {
        const int b = (int)std::min(batch, n - off);
        SQE_TRY(ivf_coarse_topk(base, st, rows_dev + (size_t)off * dim, b, 1, st->tmp_ids.as<int64_t>(), st->tmp_cos.as<float>(), s));
        if (assign_out) SQE_TRY(launch_ivf_store_assign(st->tmp_ids.as<int64_t>(), b, assign_out + off, s));
        if (ids64_out)
            SQE_HIP(hipMemcpyAsync(ids64_out + off, st->tmp_ids.p, (size_t)b * 8, hipMemcpyDeviceToDevice, s));
    }
    return SQE_OK;
}

int ivf_create(sqe_index* base, IvfState** out) {
    IvfState* st = new (std::nothrow) IvfState;   // (struct defined above)
    if (!st) return fail(SQE_ERR_OOM, "ivf: host allocation failed");
    int rc = index_create_impl(base->ctx, base->dim, SQE_INDEX_FLAT, 0, true, &st->coarse);
    if (rc != SQE_OK) { delete st; return rc; }
    *out = st;
    return SQE_OK;
}

void ivf_destroy(IvfState* st) {
    if (!st) return;
    if (st->coarse) sqe_index_destroy(st->coarse);
    delete st;
}

int ivf_rows_added(sqe_index* base, IvfState* st, hipStream_t s) {
    // assign rows [n_assigned, rows) once the centroids exist
    if (!st->trained) return SQE_OK;
    const int64_t n = base->n.load();
    if (n <= st->n_assigned) return SQE_OK;
    if ((size_t)n * 4 > st->assign.bytes) {
        // grows geometrically: an index fed 64 rows at a time must not copy the whole array on every add
        DevBuf grown;
        SQE_TRY(grown.ensure((size_t)std::max<int64_t>(n, (int64_t)(st->assign.bytes / 4) * 3 / 2) * 4));
        if (st->n_assigned > 0)
            SQE_HIP(hipMemcpyAsync(grown.p, st->assign.p, (size_t)st->n_assigned * 4, hipMemcpyDeviceToDevice, s));
        SQE_HIP(hipStreamSynchronize(s));
        std::swap(grown.p, st->assign.p);
        std::swap(grown.bytes, st->assign.bytes);
    }
    SQE_TRY(ivf_assign_rows(base, st, base->master + (size_t)st->n_assigned * base->dim, n - st->n_assigned,
                            st->assign.as<int>() + st->n_assigned, nullptr, s));
    st->n_assigned = n;
    st->lists_dirty = true;
    return SQE_OK;
}

// sqe_index_update overwrote `n` stored rows (ids on the device): only those are re-assigned
int ivf_rows_updated(sqe_index* base, IvfState* st, const int64_t* rows_dev, int64_t n, hipStream_t s) {
    if (!st->trained || n <= 0) return SQE_OK;
    SQE_TRY(ivf_rows_added(base, st, s));                 // rows appended since the last search get their list first
    const int dim = base->dim;
    DevBuf rows, lists;
    SQE_TRY(rows.ensure((size_t)n * dim * 4));
    SQE_TRY(lists.ensure((size_t)n * 4));
    SQE_TRY(launch_gather_rows(base->master, rows_dev, (int)n, dim, rows.as<float>(), s));
    SQE_TRY(ivf_assign_rows(base, st, rows.as<float>(), n, lists.as<int>(), nullptr, s));
    SQE_TRY(launch_ivf_scatter_assign(lists.as<int>(), rows_dev, n, st->assign.as<int>(), s));
    SQE_HIP(hipStreamSynchronize(s));                     // the temporaries die here
    st->lists_dirty = true;
    st->i8_done = 0;                                      // the int8 copy is rebuilt from the master by the next search
    return SQE_OK;
}

static int ivf_build_lists(sqe_index* base, IvfState* st, hipStream_t s) {
    const int nlist = base->nlist;
    const int64_t n = st->n_assigned;
    SQE_TRY(st->counts.ensure((size_t)nlist * 4));
    SQE_TRY(st->cursor.ensure((size_t)nlist * 4));
    SQE_TRY(st->offsets.ensure((size_t)(nlist + 1) * 8));
    SQE_TRY(st->order.ensure((size_t)std::max<int64_t>(n, 1) * 4));
    SQE_HIP(hipMemsetAsync(st->counts.p, 0, (size_t)nlist * 4, s));
    SQE_HIP(hipMemsetAsync(st->cursor.p, 0, (size_t)nlist * 4, s));
    SQE_TRY(launch_ivf_count(st->assign.as<int>(), n, st->counts.as<int>(), s));
    std::vector<int> h_counts(nlist);
    SQE_HIP(hipMemcpyAsync(h_counts.data(), st->counts.p, (size_t)nlist * 4, hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));
    st->h_offsets.assign(nlist + 1, 0);
    st->max_len = 0;
    for (int i = 0; i < nlist; ++i) {
        st->h_offsets[i + 1] = st->h_offsets[i] + h_counts[i];
        st->max_len = std::max(st->max_len, h_counts[i]);
    }
    SQE_HIP(hipMemcpyAsync(st->offsets.p, st->h_offsets.data(), (size_t)(nlist + 1) * 8, hipMemcpyHostToDevice, s));
    std::vector<int64_t> h_tile_off(nlist + 1, 0);
    for (int i = 0; i < nlist; ++i) h_tile_off[i + 1] = h_tile_off[i] + (h_counts[i] + 255) / 256;
    st->total_tiles = h_tile_off[nlist];
    if (st->total_tiles * 256 > 0x7fffffffLL) return fail(SQE_ERR_INVALID, "ivf: too many rows for one index shard");
    SQE_TRY(st->tile_off.ensure((size_t)(nlist + 1) * 8));
    SQE_TRY(st->dpos.ensure((size_t)std::max<int64_t>(n, 1) * 4));
    SQE_HIP(hipMemcpyAsync(st->tile_off.p, h_tile_off.data(), (size_t)(nlist + 1) * 8, hipMemcpyHostToDevice, s));
    SQE_TRY(launch_ivf_scatter(st->assign.as<int>(), n, st->offsets.as<int64_t>(), st->tile_off.as<int64_t>(), st->cursor.as<int>(),
                               st->order.as<int>(), st->dpos.as<int>(), s));
    {
        // work units of the streaming list scan (ivf_list_stream_i8_kernel): runs of <= ST_UNIT_TILES tiles of one list, and single tiles
        // (the grid of a search with a handful of queries, where few lists are probed and every CU should get some of them)
        std::vector<int4> u4, u1, uS, uR;
        for (int i = 0; i < nlist; ++i) {
            const int nt = (h_counts[i] + 255) / 256;
            // (tiles [lo, nt) of a list in nearly equal runs of <= ST_UNIT_TILES: a unit pays its query load and the fill and drain of
            // its register ring once, so 9 tiles are 5 + 4, not 4 + 4 + 1)
            auto split = [&](std::vector<int4>& out, int lo) {
                const int rem = nt - lo;
                if (rem <= 0) return;
                const int nu = (rem + ST_UNIT_TILES - 1) / ST_UNIT_TILES;
                for (int u = 0, t0 = lo; u < nu; ++u) {
                    const int len = rem / nu + (u < rem % nu ? 1 : 0);
                    out.push_back(make_int4(i, t0, len, 0));
                    t0 += len;
                }
            };
            split(u4, 0);
            for (int t0 = 0; t0 < nt; ++t0) u1.push_back(make_int4(i, t0, 1, 0));
            if (nt > 0) uS.push_back(make_int4(i, 0, 1, 0));
            split(uR, 1);
        }
        // the unit queue hands units out in table order: longest first, so that the launch ends on its shortest units
        auto longer = [](const int4& a, const int4& b) { return a.z > b.z; };
        std::stable_sort(u4.begin(), u4.end(), longer);
        std::stable_sort(uR.begin(), uR.end(), longer);
        st->n_units4 = (int)u4.size(); st->n_units1 = (int)u1.size(); st->n_unitsS = (int)uS.size(); st->n_unitsR = (int)uR.size();
        SQE_TRY(st->units4.ensure(std::max<size_t>(1, u4.size()) * sizeof(int4)));
        SQE_TRY(st->units1.ensure(std::max<size_t>(1, u1.size()) * sizeof(int4)));
        SQE_TRY(st->unitsS.ensure(std::max<size_t>(1, uS.size()) * sizeof(int4)));
        SQE_TRY(st->unitsR.ensure(std::max<size_t>(1, uR.size()) * sizeof(int4)));
        if (!u4.empty()) SQE_HIP(hipMemcpyAsync(st->units4.p, u4.data(), u4.size() * sizeof(int4), hipMemcpyHostToDevice, s));
        if (!u1.empty()) SQE_HIP(hipMemcpyAsync(st->units1.p, u1.data(), u1.size() * sizeof(int4), hipMemcpyHostToDevice, s));
        if (!uS.empty()) SQE_HIP(hipMemcpyAsync(st->unitsS.p, uS.data(), uS.size() * sizeof(int4), hipMemcpyHostToDevice, s));
        if (!uR.empty()) SQE_HIP(hipMemcpyAsync(st->unitsR.p, uR.data(), uR.size() * sizeof(int4), hipMemcpyHostToDevice, s));
        SQE_HIP(hipStreamSynchronize(s));                 // (host vectors)
    }
    SQE_HIP(hipStreamSynchronize(s));
    st->lists_dirty = false;
    st->i8_done = 0;                                      // the int8 copy follows the list order
    return SQE_OK;
}

int ivf_train(sqe_index* base, IvfState* st, const float* x_dev, int64_t n, int iters, uint64_t seed, hipStream_t s) {
    const int nlist = base->nlist, dim = base->dim;
    if (n < nlist) return fail(SQE_ERR_INVALID, "sqe_index_train: need at least nlist training rows");
    if (iters < 1) iters = 1;
    // normalised copy of the sample
    DevBuf xs, pick, assign64;
    SQE_TRY(xs.ensure((size_t)n * dim * 4));
    SQE_TRY(launch_normalize_rows(x_dev, n, dim, dim, xs.as<float>(), nullptr, dim, nullptr, nullptr, s));
    // initial centroids: nlist distinct rows of the sample (seeded partial Fisher-Yates)
    std::vector<int64_t> perm(n);
    for (int64_t i = 0; i < n; ++i) perm[i] = i;
    uint64_t rs = seed ^ 0x5eed5eedULL;
    for (int i = 0; i < nlist; ++i) std::swap(perm[i], perm[i + (int64_t)(splitmix(rs) % (uint64_t)(n - i))]);
    SQE_TRY(pick.ensure((size_t)nlist * 8));
    SQE_HIP(hipMemcpyAsync(pick.p, perm.data(), (size_t)nlist * 8, hipMemcpyHostToDevice, s));
    SQE_TRY(st->centroids.ensure((size_t)nlist * dim * 4));
    SQE_TRY(launch_gather_rows(xs.as<float>(), pick.as<int64_t>(), nlist, dim, st->centroids.as<float>(), s));
    SQE_HIP(hipStreamSynchronize(s));      // perm is a host buffer
    SQE_TRY(assign64.ensure((size_t)n * 8));
    SQE_TRY(st->sums.ensure((size_t)nlist * dim * 4));
    SQE_TRY(st->counts.ensure((size_t)nlist * 4));
    for (int it = 0; it < iters; ++it) {
        st->coarse->n.store(0);
        SQE_TRY(index_add_impl(st->coarse, st->centroids.as<float>(), nlist, dim, false, s));
        st->cent_dirty = true;
        SQE_TRY(ivf_assign_rows(base, st, xs.as<float>(), n, nullptr, assign64.as<int64_t>(), s));
        SQE_HIP(hipMemsetAsync(st->sums.p, 0, (size_t)nlist * dim * 4, s));
        SQE_HIP(hipMemsetAsync(st->counts.p, 0, (size_t)nlist * 4, s));
        SQE_TRY(launch_kmeans_accum(xs.as<float>(), assign64.as<int64_t>(), n, dim, st->sums.as<float>(), st->counts.as<int>(), s));
        SQE_TRY(launch_kmeans_finish(st->centroids.as<float>(), st->sums.as<float>(), st->counts.as<int>(), nlist, dim, s));
    }
    st->coarse->n.store(0);
    SQE_TRY(index_add_impl(st->coarse, st->centroids.as<float>(), nlist, dim, false, s));
    SQE_HIP(hipStreamSynchronize(s));
    st->trained = true;
    st->cent_dirty = true;
    st->n_assigned = 0;                    // (re)assign everything stored so far
    st->lists_dirty = true;
    return ivf_rows_added(base, st, s);
}

// ---------------------------------------------------------------- the route of a search piece
namespace {

// The knobs build's A/B switches (knob_env returns null in the shipped library: every flag is false there).
struct IvfKnobs {
    bool fp32;          // SQE_IVF_FP32=1: the fp32 list scan
    bool i8_off;        // SQE_IVF_I8=0: the bf16 list scan
    bool staged;        // SQE_IVF_STAGED=1: the r03 kernel
    bool few_table;     // SQE_IVF_FEW_TABLE=1: the single-tile unit table for a handful of queries
    bool strips_only;   // SQE_IVF_STRIPS=1: r04a's form, no collect mode
    bool no_queue;      // SQE_IVF_QUEUE=0: one workgroup per unit
};
const IvfKnobs& ivf_knobs() {
    static const IvfKnobs v = [] {
        auto is = [](const char* name, char c) { const char* e = knob_env(name); return e && e[0] == c; };
        return IvfKnobs{is("SQE_IVF_FP32", '1'), is("SQE_IVF_I8", '0'), is("SQE_IVF_STAGED", '1'), is("SQE_IVF_FEW_TABLE", '1'),
                        is("SQE_IVF_STRIPS", '1'), is("SQE_IVF_QUEUE", '0')};
    }();
    return v;
}

// Which list-scan kernel a piece takes and over which grid.  A pure function of the shapes: ivf_search's branches launch
// what it names (and write the record themselves, as they launch).
struct IvfPlan {
    int list_kernel;    // SQE_IVF_KERNEL_*
    int grid;           // SQE_IVF_GRID_*
    int split;          // SQE_IVF_GRID_PAIR: workgroups per (query, probe) pair, else 0
    int pair_tiles;     // SQE_IVF_GRID_PAIR_GRID: tiles of the longest list
    int persistent;     // workgroups of a launch on the unit queue: two per CU
    bool no_queue;
    // a streaming launch over n_units units takes them from the unit queue (persistent workgroups) when there are more than those
    bool queued(int n_units) const { return !(no_queue || n_units <= persistent); }
};

IvfPlan ivf_route_plan(int dim, int B, int nprobe, int max_len, int n_units1, int n_units4, int n_unitsR, bool use_i8, int cu_count,
                       const IvfKnobs& knobs) {
    IvfPlan p{SQE_IVF_KERNEL_BF16_MFMA, SQE_IVF_GRID_LIST, 0, 0, 2 * cu_count, knobs.no_queue};
    if (knobs.fp32) {
        p.list_kernel = SQE_IVF_KERNEL_FP32;
        return p;
    }
    const bool i8_lists = use_i8 && dim >= 256 && dim % 128 == 0 && !knobs.i8_off;
    if (!i8_lists) return p;
    const bool few = B * nprobe <= 512;                  // a handful of queries
    const bool streaming = !knobs.staged && dim % (64 * ST_SL) == 0 && ivf_stream_lds(dim) <= 80 * 1024 && n_units4 > 0;      // (two workgroups per CU)
    if (!streaming) {
        // a handful of queries: pair mode (the kernel's comment), up to 16 workgroups per probed list
        p.list_kernel = SQE_IVF_KERNEL_I8_STAGED;
        if (few) {
            p.grid = SQE_IVF_GRID_PAIR;
            p.split = std::max(1, std::min(16, 512 / (B * nprobe)));
        }
        return p;
    }
    // streaming form: one workgroup per unit of <= 4 tiles (single tiles when only a handful of lists are probed)
    p.list_kernel = SQE_IVF_KERNEL_I8_STREAM;
    if (!few) {
        // collect mode (r04b) where the threshold kernel can hold a query's sample: nprobe <= 32
        p.grid = !knobs.strips_only && nprobe <= 32 && n_unitsR > 0 ? SQE_IVF_GRID_COLLECT : SQE_IVF_GRID_UNITS4;
        return p;
    }
    // a handful of queries through the streaming scan: one workgroup per (query, probe) pair and tile -- no per-list query buckets needed
    // (... unless one list is so long that a grid of pairs x tiles-of-the-longest-list would be mostly empty: the unit table then)
    p.pair_tiles = (max_len + LS_ROWS - 1) / LS_ROWS;
    const bool pair_grid = !knobs.few_table && (int64_t)B * nprobe * p.pair_tiles <= std::max<int64_t>(8192, 2 * (int64_t)n_units1);
    p.grid = pair_grid ? SQE_IVF_GRID_PAIR_GRID : SQE_IVF_GRID_UNITS1;
    return p;
}

// ---------------------------------------------------------------- stages of a search piece
// The values of one piece (the whole batch, or a sub-batch under STRIP_BUDGET) that its stages share.
struct Piece {
    sqe_index* base;
    IvfState* st;
    hipStream_t s;
    const float* q_dev;          // [B, dim] raw queries
    int B, k, kp, nprobe, max_len;
    float* cos_out;              // [B, k] on the device
    int64_t* id_out;
    IvfPlan plan;
    ListScanI8 i8;               // int8 routes: ensure_i8_operands

    ListScan lists() const {
        return ListScan{base->nlist, st->offsets.as<int64_t>(), st->lcount.as<int>(), st->lq.as<int>(), B, nprobe, base->dim, max_len,
                        st->pair_scores.as<float>()};
    }
    IvfSelectOut select_out() const {
        return IvfSelectOut{k, kp, search_id_base(base), base->master, st->qn.as<float>(), base->dim, cos_out, id_out};
    }
};

int grow_piece_buffers(const Piece& p) {
    IvfState* st = p.st;
    const int nlist = p.base->nlist;
    SQE_TRY(st->qn.ensure((size_t)p.B * p.base->dim * 4));
    SQE_TRY(st->qb.ensure((size_t)(p.B + LS_Q) * p.base->pitch));
    SQE_TRY(st->probes_cos.ensure((size_t)p.B * p.nprobe * 4));
    SQE_TRY(st->probes_ids.ensure((size_t)p.B * p.nprobe * 8));
    SQE_TRY(st->lcount.ensure((size_t)(nlist + 4) * 4));      // (+ 4 ints behind the list counts: the collect mode's flag and unit counters)
    SQE_TRY(st->lq.ensure((size_t)nlist * p.B * 4));
    SQE_TRY(st->pair_scores.ensure((size_t)p.B * p.nprobe * p.max_len * 4));
    return SQE_OK;
}

// the record of this piece, up to the route fields (those are written by the branches that launch)
void open_record(const Piece& p) {
    IvfState* st = p.st;
    sqe_ivf_state_t& rec = st->rec;
    st->rec_valid = false;                                  // (until this piece's launches are all recorded)
    rec = sqe_ivf_state_t{};
    rec.n_assigned = st->n_assigned; rec.total_tiles = st->total_tiles;
    rec.B = p.B; rec.nprobe = p.nprobe; rec.k = p.k; rec.kp = p.kp; rec.max_len = p.max_len; rec.nlist = p.base->nlist; rec.dim = p.base->dim;
    rec.scan_pitch = p.base->pitch; rec.coarse = st->coarse_route;
    rec.n_units1 = st->n_units1; rec.n_units4 = st->n_units4; rec.n_unitsS = st->n_unitsS; rec.n_unitsR = st->n_unitsR;
    rec.sub_batches = 1; rec.list_cap = IVF_LIST_CAP; rec.persistent = p.plan.persistent;
}

// int8 list scan: half the bytes per probed row, every list a run of whole 256-row tiles in the flat scan's tiled
// layout (a K step of a tile is 32 contiguous KiB).  The copy is in list order, so it is rebuilt from the master whenever
// the lists were (rows added, rows overwritten): ivf_build_lists / ivf_rows_updated reset i8_done.  ~12 ms per 10 M rows,
// on the first search after the change.  The queries of the piece are quantised with every search.
int ensure_i8_operands(Piece& p) {
    IvfState* st = p.st;
    const sqe_index* base = p.base;
    const int dim = base->dim;
    const int64_t n = st->n_assigned;
    const int p8 = dim + 128;                          // (pitch of the quantised QUERY rows)
    const int64_t tile_stride = (int64_t)(dim / 64) * 16384 + 2048;
    if (st->i8_cap < st->total_tiles || st->i8_tile_stride != tile_stride) {
        const int64_t cap = std::max<int64_t>(st->total_tiles, (base->cap + 255) / 256 + base->nlist);
        SQE_TRY(st->i8rows.ensure((size_t)cap * tile_stride));
        SQE_TRY(st->i8sxi.ensure((size_t)cap * 256 * 4));
        st->i8_cap = cap;
        st->i8_tile_stride = tile_stride;
        st->i8_done = 0;
    }
    if (st->i8_done != n) {
        SQE_TRY(launch_quantize_gather_i8(base->master, st->order.as<int>(), st->dpos.as<int>(), n, dim, st->i8rows.as<int8_t>(), tile_stride,
                                          st->i8sxi.as<uint32_t>(), p.s));
        st->i8_done = n;
    }
    SQE_TRY(st->q8.ensure((size_t)(p.B + LS_Q) * p8));
    SQE_TRY(st->q8sqi.ensure((size_t)(p.B + LS_Q) * 4));
    SQE_TRY(launch_quantize_queries_i8(st->qn.as<float>(), p.B, dim, st->q8.as<int8_t>(), p8, nullptr, st->q8sqi.as<uint32_t>(), nullptr, p.s));
    const float unit = i8_scale_unit(dim);
    p.i8 = ListScanI8{st->i8rows.as<int8_t>(), tile_stride, st->i8sxi.as<uint32_t>(), st->q8.as<int8_t>(), p8, st->q8sqi.as<uint32_t>(),
                      unit * unit, st->tile_off.as<int64_t>()};
    st->rec.i8_tile_stride = tile_stride; st->rec.q8_pitch = p8;
    return SQE_OK;
}

// Every launch of the streaming kernel.  queue: the launch's counter behind the list counts (null: never queued); it is used,
// and `queued_bit` recorded, where the plan's rule says so.
int launch_stream(const Piece& p, const DevBuf& units, int n_units, const StCollect* col, const int* gate, int* queue, int queued_bit,
                  const int64_t* pair_probes = nullptr, int pair_tiles = 0) {
    if (!p.plan.queued(n_units)) queue = nullptr;
    if (queue) p.st->rec.queued |= queued_bit;
    return launch_ivf_list_stream_i8(p.i8, p.lists(), units.as<int4>(), n_units, col, gate, queue, p.plan.persistent, pair_probes, pair_tiles,
                                     p.s);
}

int select_from_strips(const Piece& p, const int* gate) {
    const IvfState* st = p.st;
    return launch_ivf_select(st->probes_ids.as<int64_t>(), st->offsets.as<int64_t>(), st->order.as<int>(), st->pair_scores.as<float>(), p.B,
                             p.nprobe, p.max_len, p.select_out(), gate, p.s);
}

// Collect mode (r04b): sample pass over the first tile of every list -> per-query thresholds -> the other tiles keep only
// the keys at or above them -> the lists are ranked.  Any query whose list cannot answer sets the flag, and the two gated
// launches at the end redo the batch through the strips (they return at once otherwise).
int collect_scan_select(const Piece& p) {
    IvfState* st = p.st;
    SQE_TRY(st->cthr.ensure((size_t)p.B * 4));
    SQE_TRY(st->ccnt.ensure((size_t)p.B * 8));      // (list lengths [B], rows in the probed lists [B])
    SQE_TRY(st->clist.ensure((size_t)p.B * IVF_LIST_CAP * 8));
    int* cflag = st->lcount.as<int>() + p.base->nlist;      // [0] fallback flag, [1..3] unit counters: zeroed with the list counts
    st->rec.grid = SQE_IVF_GRID_COLLECT;
    SQE_TRY(launch_stream(p, st->unitsS, st->n_unitsS, nullptr, nullptr, cflag + 1, SQE_IVF_QUEUED_SAMPLE));
    SQE_TRY(launch_ivf_threshold(st->probes_ids.as<int64_t>(), st->offsets.as<int64_t>(), st->order.as<int>(), st->pair_scores.as<float>(), p.B,
                                 p.nprobe, p.max_len, p.kp, st->cthr.as<float>(), st->ccnt.as<int>(), st->clist.as<uint64_t>(), p.s));
    const StCollect col{st->cthr.as<float>(), st->ccnt.as<int>(), st->clist.as<uint64_t>(), IVF_LIST_CAP, st->order.as<int>()};
    SQE_TRY(launch_stream(p, st->unitsR, st->n_unitsR, &col, nullptr, cflag + 2, SQE_IVF_QUEUED_COLLECT));
    SQE_TRY(launch_ivf_select_list(st->ccnt.as<int>(), st->clist.as<uint64_t>(), p.B, p.select_out(), cflag, p.s));
    SQE_TRY(launch_stream(p, st->units4, st->n_units4, nullptr, cflag, cflag + 3, SQE_IVF_QUEUED_FALLBACK));
    return select_from_strips(p, cflag);
}

// S6 by the plan, then the select.  The route fields of the record are written here, branch by branch.
int scan_and_select(const Piece& p) {
    IvfState* st = p.st;
    const sqe_index* base = p.base;
    sqe_ivf_state_t& rec = st->rec;
    switch (p.plan.list_kernel) {
        case SQE_IVF_KERNEL_FP32:
            rec.list_kernel = SQE_IVF_KERNEL_FP32; rec.grid = SQE_IVF_GRID_LIST;
            SQE_TRY(launch_ivf_list_scan_f32(base->master, st->qn.as<float>(), st->order.as<int>(), p.lists(), p.s));
            break;
        case SQE_IVF_KERNEL_BF16_MFMA:
            rec.list_kernel = SQE_IVF_KERNEL_BF16_MFMA; rec.grid = SQE_IVF_GRID_LIST;
            SQE_TRY(launch_ivf_list_scan_bf16(base->scan, base->pitch, st->qb.as<bf16_t>(), base->pitch, st->order.as<int>(), p.lists(), p.s));
            break;
        case SQE_IVF_KERNEL_I8_STAGED: {
            const int n_pairs = p.plan.grid == SQE_IVF_GRID_PAIR ? p.B * p.nprobe : 0;
            rec.list_kernel = SQE_IVF_KERNEL_I8_STAGED; rec.grid = n_pairs ? SQE_IVF_GRID_PAIR : SQE_IVF_GRID_LIST;
            rec.split = p.plan.split;
            SQE_TRY(launch_ivf_list_scan_i8(p.i8, p.lists(), st->probes_ids.as<int64_t>(), n_pairs, std::max(1, p.plan.split), p.s));
            break;
        }
        case SQE_IVF_KERNEL_I8_STREAM:
            rec.list_kernel = SQE_IVF_KERNEL_I8_STREAM;
            switch (p.plan.grid) {
                case SQE_IVF_GRID_COLLECT:
                    return collect_scan_select(p);
                case SQE_IVF_GRID_PAIR_GRID:
                    // a handful of queries: one workgroup per (query, probe) pair and tile of its list (the lists of different queries
                    // are read separately; at most 512 pairs)
                    rec.grid = SQE_IVF_GRID_PAIR_GRID;
                    SQE_TRY(launch_stream(p, st->units1, p.B * p.nprobe * p.plan.pair_tiles, nullptr, nullptr, nullptr, 0,
                                          st->probes_ids.as<int64_t>(), p.plan.pair_tiles));
                    break;
                case SQE_IVF_GRID_UNITS1:
                    rec.grid = SQE_IVF_GRID_UNITS1;
                    SQE_TRY(launch_stream(p, st->units1, st->n_units1, nullptr, nullptr, nullptr, 0));
                    break;
                default:
                    rec.grid = SQE_IVF_GRID_UNITS4;
                    SQE_TRY(launch_stream(p, st->units4, st->n_units4, nullptr, nullptr, nullptr, 0));
                    break;
            }
            break;
    }
    return select_from_strips(p, nullptr);
}

// One piece, a complete search of its queries: buffers -> normalise -> S5 coarse probes -> route plan -> pair buckets ->
// int8 operands -> S6 list scan -> select.
int search_piece(Piece& p) {
    IvfState* st = p.st;
    sqe_index* base = p.base;
    const int nlist = base->nlist, dim = base->dim;
    SQE_TRY(grow_piece_buffers(p));
    SQE_TRY(launch_normalize_rows(p.q_dev, p.B, dim, dim, st->qn.as<float>(), st->qb.as<bf16_t>(), base->pitch / 2, nullptr, nullptr, p.s));
    // S5: coarse quantise
    SQE_TRY(ivf_coarse_topk(base, st, p.q_dev, p.B, p.nprobe, st->probes_ids.as<int64_t>(), st->probes_cos.as<float>(), p.s));
    p.plan = ivf_route_plan(dim, p.B, p.nprobe, p.max_len, st->n_units1, st->n_units4, st->n_unitsR, st->use_i8, base->ctx->cu_count,
                            ivf_knobs());
    open_record(p);
    if (p.plan.grid != SQE_IVF_GRID_PAIR_GRID) {
        SQE_HIP(hipMemsetAsync(st->lcount.p, 0, (size_t)(nlist + 4) * 4, p.s));
        SQE_TRY(launch_ivf_bucket(st->probes_ids.as<int64_t>(), p.B, p.nprobe, st->lcount.as<int>(), st->lq.as<int>(), p.s));
    }
    if (p.plan.list_kernel == SQE_IVF_KERNEL_I8_STAGED || p.plan.list_kernel == SQE_IVF_KERNEL_I8_STREAM) SQE_TRY(ensure_i8_operands(p));
    SQE_TRY(scan_and_select(p));
    st->rec_valid = true;
    return SQE_OK;
}

}  // namespace

int ivf_search(sqe_index* base, IvfState* st, const float* q_dev, int B, int k, int nprobe, float* cos_out, int64_t* id_out,
               hipStream_t s) {
    if (!st->trained) return fail(SQE_ERR_STATE, "sqe_index_search: IVF index is not trained (sqe_index_train)");
    const int nlist = base->nlist, dim = base->dim;
    if (nprobe <= 0) nprobe = 32;
    nprobe = std::min(std::min(nprobe, nlist), MAX_KP);
    SQE_TRY(ivf_rows_added(base, st, s));
    if (st->lists_dirty) SQE_TRY(ivf_build_lists(base, st, s));
    const int max_len = (std::max(st->max_len, 1) + 3) / 4 * 4;        // strips are written 4 floats at a time
    // The score strips are [queries, nprobe, longest list] floats.  One over-long list (duplicate-heavy or
    // tightly clustered data) must not turn that into terabytes: the batch is cut into sub-batches whose
    // strips fit a fixed budget, each a complete search of its queries.
    constexpr size_t STRIP_BUDGET = 6ull << 30;
    const size_t per_query = (size_t)nprobe * max_len * 4;
    const int sub = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, STRIP_BUDGET / per_query));
    const int kp = std::min(MAX_KP, std::max(32, 4 * k));
    for (int off = 0; off < B; off += sub) {
        Piece p{base, st, s, q_dev + (size_t)off * dim, std::min(sub, B - off), k, kp, nprobe, max_len, cos_out + (size_t)off * k,
                id_out + (size_t)off * k, IvfPlan{}, ListScanI8{}};
        SQE_TRY(search_piece(p));
    }
    st->rec.sub_batches = (B + sub - 1) / sub;              // (the record describes the last piece)
    return SQE_OK;
}

// sqe_index_ivf_state: the record of the last search piece; the collect mode's fallback flag is read from the device here
int ivf_state(sqe_index* base, IvfState* st, sqe_ivf_state_t* out, hipStream_t s) {
    if (!st->rec_valid) return fail(SQE_ERR_STATE, "sqe_index_ivf_state: no IVF search yet");
    (void)base;
    *out = st->rec;
    out->fallback = 0;
    if (st->rec.grid == SQE_IVF_GRID_COLLECT)
        SQE_HIP(hipMemcpyAsync(&out->fallback, st->lcount.as<int>() + st->rec.nlist, 4, hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));
    return SQE_OK;
}

int ivf_state_read(sqe_index* base, IvfState* st, int what, int64_t offset, void* out_host, int64_t bytes, hipStream_t s) {
    if (!st->rec_valid) return fail(SQE_ERR_STATE, "sqe_index_ivf_state_read: no IVF search yet");
    const sqe_ivf_state_t& r = st->rec;
    const bool i8 = r.list_kernel == SQE_IVF_KERNEL_I8_STAGED || r.list_kernel == SQE_IVF_KERNEL_I8_STREAM;
    const bool coll = r.grid == SQE_IVF_GRID_COLLECT;
    const int64_t B = r.B, pairs = B * r.nprobe;
    // rows the record speaks of that the base index still holds (a delete since the search shortens both)
    const int64_t rows = std::min<int64_t>(r.n_assigned, base->n.load());
    const void* src = nullptr;
    int64_t size = 0;
    switch (what) {
        case SQE_IVF_PROBES: src = st->probes_ids.p; size = pairs * 8; break;
        case SQE_IVF_PROBES_COS: src = st->probes_cos.p; size = pairs * 4; break;
        case SQE_IVF_STRIPS: src = st->pair_scores.p; size = pairs * r.max_len * 4; break;
        case SQE_IVF_ORDER: src = st->order.p; size = r.n_assigned * 4; break;
        case SQE_IVF_OFFSETS: src = st->offsets.p; size = ((int64_t)r.nlist + 1) * 8; break;
        case SQE_IVF_TILE_OFF: src = st->tile_off.p; size = ((int64_t)r.nlist + 1) * 8; break;
        case SQE_IVF_SCAN_BF16: src = base->scan; size = rows * r.scan_pitch; break;
        case SQE_IVF_ROWS_F32: src = base->master; size = rows * r.dim * 4; break;
        case SQE_IVF_I8_ROWS: src = i8 ? st->i8rows.p : nullptr; size = r.total_tiles * r.i8_tile_stride; break;
        case SQE_IVF_I8_ROW_SCALES: src = i8 ? st->i8sxi.p : nullptr; size = r.total_tiles * 256 * 4; break;
        case SQE_IVF_Q8: src = i8 ? st->q8.p : nullptr; size = B * r.q8_pitch; break;
        case SQE_IVF_Q8_SCALES: src = i8 ? st->q8sqi.p : nullptr; size = B * 4; break;
        case SQE_IVF_QN: src = st->qn.p; size = B * r.dim * 4; break;
        case SQE_IVF_QB: src = st->qb.p; size = B * r.scan_pitch; break;
        case SQE_IVF_THRESHOLDS: src = coll ? st->cthr.p : nullptr; size = B * 4; break;
        case SQE_IVF_COUNTS: src = coll ? st->ccnt.p : nullptr; size = B * 8; break;
        case SQE_IVF_KEY_LISTS: src = coll ? st->clist.p : nullptr; size = B * IVF_LIST_CAP * 8; break;
        default: return fail(SQE_ERR_INVALID, "sqe_index_ivf_state_read: unknown buffer");
    }
    if (!src || size == 0) return fail(SQE_ERR_STATE, "sqe_index_ivf_state_read: the last search did not use that buffer");
    if (offset < 0 || bytes < 0 || offset + bytes > size) return fail(SQE_ERR_INVALID, "sqe_index_ivf_state_read: range outside the buffer");
    if (bytes == 0) return SQE_OK;
    SQE_HIP(hipMemcpyAsync(out_host, static_cast<const char*>(src) + offset, (size_t)bytes, hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));
    return SQE_OK;
}

void ivf_invalidate(IvfState* st) { st->n_assigned = 0; st->lists_dirty = true; }

void ivf_assignments(IvfState* st, int** assign, int64_t* n_assigned) {
    const bool any = st->trained && st->n_assigned > 0;
    *assign = any ? st->assign.as<int>() : nullptr;
    *n_assigned = any ? st->n_assigned : 0;
}

// sqe_index_delete compacted the assignments together with the rows (compact.hip): the lists and their int8 copy rebuild lazily
void ivf_rows_deleted(IvfState* st, int64_t n_assigned) {
    if (!st->trained) return;
    st->n_assigned = n_assigned;
    st->lists_dirty = true;
    st->i8_done = 0;
}
sqe_index* ivf_coarse(IvfState* st) { return st->coarse; }

bool ivf_trained(IvfState* st) { return st->trained; }

// sqe_index_load: centroids (normalised, as exported) and the per-row list assignment of a saved index
int ivf_restore(sqe_index* base, IvfState* st, const float* centroids_dev, const int32_t* assign_dev, int64_t n, hipStream_t s) {
    const int nlist = base->nlist;
    st->coarse->n.store(0);
    SQE_TRY(index_add_impl(st->coarse, centroids_dev, nlist, base->dim, true, s));
    SQE_TRY(st->assign.ensure((size_t)std::max<int64_t>(n, 1) * 4));
    if (n > 0) SQE_HIP(hipMemcpyAsync(st->assign.p, assign_dev, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    SQE_HIP(hipStreamSynchronize(s));
    st->trained = true;
    st->cent_dirty = true;
    st->n_assigned = n;
    st->lists_dirty = true;
    return SQE_OK;
}

// introspection for tests / tools: centroids and assignments as stored
int ivf_export(sqe_index* base, IvfState* st, float* centroids_host, int32_t* assign_host, hipStream_t s) {
    if (!st->trained) return fail(SQE_ERR_STATE, "ivf export: not trained");
    SQE_TRY(ivf_rows_added(base, st, s));
    if (centroids_host)
        SQE_HIP(hipMemcpyAsync(centroids_host, st->coarse->master, (size_t)base->nlist * base->dim * 4,
                               hipMemcpyDeviceToHost, s));
    if (assign_host && st->n_assigned > 0)
        SQE_HIP(hipMemcpyAsync(assign_host, st->assign.p, (size_t)st->n_assigned * 4, hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));
    return SQE_OK;
}

}  // namespace sqe
