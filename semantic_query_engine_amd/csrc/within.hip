// within.hip -- radial, collapsed and MMR search within a row set (sqe_index_range_search_where, _search_collapsed_where,
// _search_mmr_where): the row set S of sqe_index_search_where -- the live rows a field predicate selects, intersected with an
// optional allow-list -- restricts the three searches that so far took none.  Each call returns bit for bit what the
// unrestricted call of its kind returns on a copy of the index from which every row outside S was deleted.
//
//   Row set: the preparation every consumer of a row set shares (rowset.hip: rowset_map, then rowset_positions for the ascending
//     positions and their number M): the one added synchronisation.  M == 0: padded outputs, zero counts.
//   Gather route (M <= "filter_gather_rows", one chunk of the filtered search's scratch sub-index): filter_gather_sub copies the
//     fp32 and bf16 rows of S, and for collapsed search their keys by position, into the sub-index, which then IS the index
//     "with every row outside S deleted": the unchanged impl of the kind runs on it, launch_translate_ids maps its positions to
//     owner positions, and the owner's id map and id_base are applied once.  Nothing gathered survives the call.
//   Mask route (FLAT and IVF; every larger S, or "within_route" 2): the impl of the kind runs on the owner with the map as a
//     denial policy of its deciding kernels (deny_kernels.h: DenyBitmap where the unrestricted path instantiates DenyNone):
//       radial     range_merge_kernel counts and lists a row iff s >= t and its bit is set.  The collect scan, the overflow plan
//                  and the walk know nothing of the map: a denied row may fill a buffer and cost a walk, never a count.
//       collapsed  stage A (FLAT) fetches d = sqe_where_depth(collapse_depth_of(k), M, live) rows (256 where that answers 0);
//                  collapse_walk_kernel passes over a head whose bit is clear and flags the query when fewer than k groups were
//                  found although d < live; collapse_merge_kernel in the sweep drops rows whose bit is clear before the per-key
//                  reduction.  collapse.hip's argument holds with "row" read as "row of S": a dropped row is not in S, and the
//                  threshold is the k-th group of rows in S.
//   MMR adds no route: mmr.hip takes its candidates from index_search_where_impl at depth n (whichever route "where_route" gives
//     that call) as positions and runs Gram and select unchanged.
// Device groups (group.hip): every shard restricts its own rows, each by its own route; only the allow-list is routed, and the
// existing part merges combine the shards.
// The C entry points stand with their kinds (range.hip, collapse.hip, mmr.hip): one host and one device body each serve the plain
// and the _where export.
#include <algorithm>

#include "fieldpred.h"
#include "internal.h"

namespace sqe {

static_assert(sizeof(sqe_within_last_t) == 40, "sqe.h layouts");

namespace {

// The row set's map, positions and size M.  *f_out is null and M is 0 where nothing can be selected (an empty index or an empty
// list).  One synchronisation of s, which also ends the reads of a host allow-list.
int within_rows(sqe_index* idx, const RowSet& set, FilterState** f_out, int64_t* M_out, hipStream_t s) {
    int64_t words;
    *f_out = nullptr;
    *M_out = 0;
    if (idx->n.load() == 0 || set.n_allow == 0) return SQE_OK;
    SQE_TRY(rowset_map(idx, set, f_out, &words, s));
    return rowset_positions(idx, set, *f_out, words, M_out, s);
}

bool gathers(const sqe_index* idx, int64_t M) { return idx->within_route != 2 && M <= idx->filter_gather_rows; }

sqe_within_last_t record(int kind, int64_t M, int64_t live) {
    sqe_within_last_t last{};
    last.kind = kind;
    last.selected = M;
    last.live = live;
    return last;
}

}  // namespace

int index_range_search_within(sqe_index* idx, const float* q_dev, int B, const float* min_cos_dev, int m, const RowSet& set,
                              int64_t* count_dev, float* cos_dev, int64_t* id_dev, hipStream_t s) {
    if (B <= 0) return SQE_OK;
    FilterState* f;
    int64_t M;
    SQE_TRY(within_rows(idx, set, &f, &M, s));
    sqe_within_last_t last = record(SQE_WITHIN_RADIAL, M, idx->n.load());
    if (M == 0) {
        // what the unrestricted call writes on an index without rows: zero counts and the padding
        SQE_HIP(hipMemsetAsync(count_dev, 0, (size_t)B * 8, s));
        SQE_TRY(launch_pad_hits(cos_dev, id_dev, nullptr, (int64_t)B * m, s));
    } else if (gathers(idx, M)) {
        last.route = SQE_WHERE_ROUTE_GATHER;
        sqe_index* sub;
        const int64_t* pos;
        SQE_TRY(filter_gather_sub(idx, f, M, false, &sub, &pos, s));
        SQE_TRY(index_range_search_impl(sub, q_dev, B, min_cos_dev, m, count_dev, cos_dev, id_dev, s, nullptr, &last.swept));
        SQE_TRY(launch_translate_ids(id_dev, (int64_t)B * m, pos, 0, s));
        SQE_TRY(index_positions_to_ids(idx, id_dev, (int64_t)B * m, s));
    } else {
        last.route = SQE_WHERE_ROUTE_MASK;
        SQE_TRY(index_range_search_impl(idx, q_dev, B, min_cos_dev, m, count_dev, cos_dev, id_dev, s, filter_bitmap(f), &last.swept));
    }
    idx->within_last = last;
    return SQE_OK;
}

int index_search_collapsed_within(sqe_index* idx, const float* q_dev, int B, int k, const RowSet& set, float* cos_dev, int64_t* id_dev,
                                  int64_t* key_dev, hipStream_t s) {
    if (B <= 0) return SQE_OK;
    const int64_t bk = (int64_t)B * k, n = idx->n.load();
    FilterState* f;
    int64_t M;
    SQE_TRY(within_rows(idx, set, &f, &M, s));
    sqe_within_last_t last = record(SQE_WITHIN_COLLAPSED, M, n);
    if (M == 0) {
        idx->ctx->collapse_swept.store(0);
        SQE_TRY(launch_pad_hits(cos_dev, id_dev, key_dev, bk, s));
    } else if (gathers(idx, M)) {
        last.route = SQE_WHERE_ROUTE_GATHER;
        sqe_index* sub;
        const int64_t* pos;
        SQE_TRY(filter_gather_sub(idx, f, M, true, &sub, &pos, s));
        last.depth = collapse_depth_of(sub, k);
        SQE_TRY(index_search_collapsed_impl(sub, q_dev, B, k, cos_dev, id_dev, key_dev, s));
        SQE_TRY(launch_translate_ids(id_dev, bk, pos, 0, s));
        SQE_TRY(index_positions_to_ids(idx, id_dev, bk, s));
        last.swept = idx->ctx->collapse_swept.load();
    } else {
        last.route = SQE_WHERE_ROUTE_MASK;
        int d = 0;
        if (!idx->ivf) {
            const int w = where_depth(collapse_depth_of(idx, k), M, n);
            d = w > 0 ? w : WHERE_MAX_DEPTH;
        }
        last.depth = d;
        SQE_TRY(index_search_collapsed_impl(idx, q_dev, B, k, cos_dev, id_dev, key_dev, s, filter_bitmap(f), d));
        last.swept = idx->ctx->collapse_swept.load();
    }
    idx->within_last = last;
    return SQE_OK;
}

int index_search_mmr_within(sqe_index* idx, const float* q_dev, int B, int k, int n, const float* lam_dev, const RowSet& set,
                            float* cos_dev, int64_t* id_dev, float* mmr_dev, hipStream_t s) {
    if (B <= 0) return SQE_OK;
    SQE_TRY(index_search_mmr_impl(idx, q_dev, B, k, n, lam_dev, 0, cos_dev, id_dev, mmr_dev, s, &set));
    sqe_within_last_t last = record(SQE_WITHIN_MMR, 0, idx->n.load());
    if (idx->n.load() > 0) {        // the record of the last pass's candidate call
        last.route = idx->where_last.route;
        last.selected = idx->where_last.selected;
        last.swept = idx->where_last.swept;
    }
    last.depth = n;
    idx->within_last = last;
    return SQE_OK;
}

}  // namespace sqe

// ================================================================ C ABI
using namespace sqe;

extern "C" {

int sqe_index_within_last(sqe_index* idx, sqe_within_last_t* out) {
    if (!idx || !out) return fail(SQE_ERR_INVALID, "sqe_index_within_last: null argument");
    if (idx->group) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_within_last: single-device indexes only");
    std::lock_guard<std::mutex> lk(idx->ord.mu);
    if (idx->within_last.live < 0) return fail(SQE_ERR_STATE, "sqe_index_within_last: no restricted search ran on this index yet");
    *out = idx->within_last;
    return SQE_OK;
}

}  // extern "C"
