// where_mask.hip -- the mask route of sqe_index_search_where (FLAT indexes): the k nearest rows among those a field predicate
// selects, found by searching the WHOLE index and masking the hits, where the gather route (filter.hip) copies the selected rows
// into a scratch index first.  Copying is cheap for a narrow predicate and costs more than the search itself for a broad one;
// fields.hip chooses per call ("where_route") once the predicate's map is written and its count M has come back.
//
//   Stage A, per pass of at most 1,024 queries: the unchanged certified search over row positions at one depth d for the whole
//     call (fieldpred.h: where_depth, the smallest d at which a query whose selected rows fell independently of it has fewer than
//     k of them among its d nearest with probability <= 2^-10; "where_mask_depth" overrides it).  deny_drop_kernel<DenyBitmap>
//     (deny_kernels.h; one wave per query) walks the hits 64 at a time, tests bit p of the map per lane, compacts the survivors
//     by ballot and prefix popcount and writes the first k into the caller's row.  A query with fewer than k survivors although
//     the index holds more rows than were fetched is flagged.
//   Stage B, the flagged queries: sweep.hip's sweep (sweep_flagged) with deny_merge_kernel<DenyBitmap>, exactly as exclusion
//     search runs it with its table probe: per slot a running list of at most k (cosine, position) entries in the caller's row
//     and its k-th cosine as the threshold; the keys a range collected at threshold - eps are re-scored in fp32 by rescore_row
//     (the chain of the search: same bits), the rows whose bit is clear dropped, the rest merged by block_select.h's select.
//     Dropping a row below the k-th of k selected rows never changes the answer, so the result is the exact top-k of the
//     selected rows whatever d was: a predicate correlated with the queries costs flagged queries and a sweep, never an answer.
//   Positions -> ids through the index's id map, then id_base.
// The map is the filtered search's (FilterState::bits), read and never written here: neither the plain search nor the sweep
// touches a FilterState, so it stands until the last merge.  The owner's search state is left as a plain search of depth d
// leaves it (on a large index that includes the lazy int8 copy).  Synchronisations: one after stage A for the number of flagged
// queries, one per row range of the sweep.
#include <math.h>

#include <algorithm>

#include "deny_kernels.h"
#include "internal.h"

namespace sqe {

struct WhereMaskState {
    DevBuf hits;       // stage A of a pass: cos [bs, d] (16-B rounded) | positions [bs, d]
    DevBuf flags;      // [B] int: the query is incomplete
    SweepBufs sw;      // stage B
    std::atomic<int64_t> swept{0};
};

void where_mask_destroy(WhereMaskState* w) { delete w; }

int index_search_where_mask(sqe_index* idx, const uint32_t* bits, int d, const float* q_dev, int B, int k, float* cos_out_dev,
                            int64_t* id_out_dev, int64_t* swept_out, hipStream_t s, bool as_positions) {
    const int64_t n = idx->n.load();
    const int K = idx->dim;
    if (idx->ivf || n <= 0 || n > (int64_t)UINT32_MAX || d < k || d > MAX_KP)
        return fail(SQE_ERR_STATE, "sqe_index_search_where: the mask route serves FLAT indexes of 1 to 2^32 rows at a depth in [k, 256]");
    if (!idx->where_mask) idx->where_mask = new (std::nothrow) WhereMaskState;
    WhereMaskState* st = idx->where_mask;
    if (!st) return fail(SQE_ERR_OOM, "sqe_index_search_where: host allocation failed");
    SQE_TRY(st->flags.ensure((size_t)B * 4));
    const int pass_max = std::min(B, SWEEP_MAX_PASS);
    const size_t cb = round16((size_t)pass_max * d * 4);
    SQE_TRY(st->hits.ensure(cb + (size_t)pass_max * d * 8));
    float* hc = st->hits.as<float>();
    int64_t* hp = reinterpret_cast<int64_t*>(st->hits.as<char>() + cb);
    // ---- stage A
    for (int off = 0; off < B; off += SWEEP_MAX_PASS) {
        const int bs = std::min(SWEEP_MAX_PASS, B - off);
        SQE_TRY(index_search_positions(idx, q_dev + (size_t)off * K, bs, d, 0, hc, hp, s));
        StageTimer t(idx->ctx->prof, s, ST_SELECT);
        DropArgs<DenyBitmap> a;
        a.hit_cos = hc; a.hit_pos = hp; a.kd = d; a.k = k; a.cls = nullptr; a.deny = {bits};
        a.id_sub = search_id_base(idx); a.n_rows = n; a.cos_out = cos_out_dev + (size_t)off * k; a.pos_out = id_out_dev + (size_t)off * k;
        a.flags = st->flags.as<int>() + off;
        hipLaunchKernelGGL(deny_drop_kernel<DenyBitmap>, dim3(bs), dim3(64), 0, s, a);
        SQE_HIP(hipGetLastError());
    }
    // ---- stage B: the sweep of the flagged queries
    SweepBufs& b = st->sw;
    SQE_TRY(sweep_flagged(idx, b, st->flags.as<int>(), q_dev, B, k, cos_out_dev, id_out_dev, nullptr, st->swept,
                          [&](int off, const int* qidx, int hs, int64_t r0) -> int {
                              StageTimer t(idx->ctx->prof, s, ST_SELECT);
                              MergeArgs<DenyBitmap> a;
                              a.master = idx->master; a.qn = b.qn.as<float>(); a.K = K; a.qidx = qidx;
                              a.keys = b.keys.as<uint64_t>(); a.key_cnt = b.key_cnt.as<int>(); a.row_off = r0; a.k = k;
                              a.deny = {bits};
                              a.q_resid = b.q_resid.as<float>(); a.resid_max = idx->resid_max.as<uint32_t>();
                              a.thr = b.thr.as<float>(); a.kth = b.kth.as<float>(); a.lcnt = b.lcnt.as<int>();
                              a.cos_out = cos_out_dev + (size_t)off * k; a.pos_out = id_out_dev + (size_t)off * k;
                              hipLaunchKernelGGL(deny_merge_kernel<DenyBitmap>, dim3(hs), dim3(DENY_MERGE_THREADS), 0, s, a);
                              SQE_HIP(hipGetLastError());
                              return SQE_OK;
                          },
                          s));
    *swept_out = st->swept.load();
    // positions -> ids (+ id_base)
    return as_positions ? SQE_OK : index_positions_to_ids(idx, id_out_dev, (int64_t)B * k, s);
}

}  // namespace sqe
