// within.hip -- radial, collapsed and MMR search within a row set (sqe_index_range_search_where, _search_collapsed_where,
// _search_mmr_where): the row set S of sqe_index_search_where -- the live rows a field predicate selects, intersected with an
// optional allow-list -- restricts the three searches that so far took none.  Each call returns bit for bit what the
// unrestricted call of its kind returns on a copy of the index from which every row outside S was deleted.
//
//   Row set: prepared exactly as index_search_where_impl prepares it (filter_bitmap_ensure, filter_bitmap_mark for the list, the
//     field match kernel ANDed into it, index_bitmap_positions for the ascending positions and their number M): the one added
//     synchronisation.  M == 0: padded outputs, zero counts.
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
#include <math.h>
#include <cmath>

#include <algorithm>
#include <vector>

#include "fieldpred.h"
#include "internal.h"

namespace sqe {

static_assert(sizeof(sqe_within_last_t) == 40, "sqe.h layouts");

struct WithinState {
    DevBuf stage;      // host entry points: queries, thresholds / weights and results
    DevBuf lam;        // the MMR weights of the _device form
};

void within_destroy(WithinState* w) { delete w; }

namespace {

WithinState* within_state(sqe_index* idx) {
    if (!idx->within) idx->within = new (std::nothrow) WithinState;
    return idx->within;
}

// The row set's map, positions and size, as index_search_where_impl builds them.  *f_out is null where nothing can be selected
// (an empty index or an empty list).  One synchronisation of s.
int within_rows(sqe_index* idx, const RowSet& set, FilterState** f_out, int64_t* M_out, hipStream_t s) {
    const int64_t n = idx->n.load();
    *f_out = nullptr;
    *M_out = 0;
    if (n == 0 || set.n_allow == 0) return SQE_OK;
    FilterState* f;
    int64_t words;
    SQE_TRY(filter_bitmap_ensure(idx, &f, &words));
    {
        StageTimer t(idx->ctx->prof, s, ST_PREP);
        if (set.n_allow > 0) {
            const int64_t* allow_dev = set.allow;
            if (set.allow_on_host) SQE_TRY(stage_allow_ids(f, set.allow, set.n_allow, s, &allow_dev));
            SQE_TRY(filter_bitmap_mark(idx, f, words, allow_dev, set.n_allow, s));
        }
        // without a list the kernel writes every word of the map, the padding included
        SQE_TRY(fields_bitmap_eval(idx, set.pr, filter_bitmap(f), set.n_allow > 0, s));
    }
    // the synchronisation inside also ends the reads of a host allow-list
    SQE_TRY(index_bitmap_positions(idx, f, words, set.n_allow > 0 ? std::min(set.n_allow, n) : n, M_out, s));
    *f_out = f;
    return SQE_OK;
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

namespace {

// the row-set arguments, checked as sqe_index_search_where checks them; one[2] receives the offsets of the one predicate
int set_args_ok(const char* who, const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set, const void* allow,
                int64_t n_allow, int64_t* one) {
    if (n_clauses < 0 || n_clauses > FIELD_MAX_CLAUSES) return fail(SQE_ERR_INVALID, std::string(who) + ": between 0 and 8 clauses");
    one[0] = 0;
    one[1] = n_clauses;
    SQE_TRY(fields_args_ok(who, FieldPreds{clauses, one, 1, set_values, n_set}));
    if (n_allow < -1 || (n_allow > 0 && !allow)) return fail(SQE_ERR_INVALID, std::string(who) + ": bad allow-list");
    return SQE_OK;
}

int radial_args_ok(sqe_index* idx, const void* q, int B, const void* min_cos, int max_hits, const void* counts, const void* cos, const void* ids) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (B < 0 || max_hits < 0 || max_hits > RANGE_MAX_HITS)
        return fail(SQE_ERR_INVALID, "sqe_index_range_search_where: need B >= 0 and 0 <= max_hits <= 10000");
    if (B > 0 && (!q || !min_cos || !counts)) return fail(SQE_ERR_INVALID, "sqe_index_range_search_where: null buffer");
    if (B > 0 && max_hits > 0 && (!cos || !ids)) return fail(SQE_ERR_INVALID, "sqe_index_range_search_where: null result buffer");
    return SQE_OK;
}

int thresholds_ok(const float* t, int B) {
    for (int b = 0; b < B; ++b)
        if (std::isnan(t[b])) return fail(SQE_ERR_INVALID, "sqe_index_range_search_where: threshold " + std::to_string(b) + " is NaN");
    return SQE_OK;
}

int collapsed_args_ok(sqe_index* idx, const void* q, int B, int k, const void* cos, const void* ids, const void* keys) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (B < 0 || k < 1 || k > MAX_KP) return fail(SQE_ERR_INVALID, "sqe_index_search_collapsed_where: need B >= 0 and 1 <= k <= 256");
    if (B > 0 && (!q || !cos || !ids || !keys)) return fail(SQE_ERR_INVALID, "sqe_index_search_collapsed_where: null buffer");
    return SQE_OK;
}

int mmr_args_ok(sqe_index* idx, const void* q, int B, int k, int n_cand, const float* lam, const void* cos, const void* ids, const void* mmr) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (B < 0 || k < 1 || k > MMR_MAX_N) return fail(SQE_ERR_INVALID, "sqe_index_search_mmr_where: need B >= 0 and 1 <= k <= 256");
    if (n_cand != 0 && (n_cand < k || n_cand > MMR_MAX_N))
        return fail(SQE_ERR_INVALID, "sqe_index_search_mmr_where: need n_cand == 0 (automatic) or k <= n_cand <= 256");
    if (B > 0 && (!q || !lam || !cos || !ids || !mmr)) return fail(SQE_ERR_INVALID, "sqe_index_search_mmr_where: null buffer");
    for (int b = 0; b < B; ++b)
        if (!(lam[b] >= 0.f && lam[b] <= 1.f)) return fail(SQE_ERR_INVALID, "sqe_index_search_mmr_where: lambda must be in [0, 1]");
    return SQE_OK;
}

// the allow-list of a _device call on a device group comes to the host, where the shards are planned
int group_allow(sqe_index* idx, const int64_t* allow_dev, int64_t n_allow, std::vector<int64_t>& out) {
    const int64_t one_list[2] = {0, std::max<int64_t>(n_allow, 0)};
    return list_ids_to_host(idx->ctx, allow_dev, one_list, 1, out);
}

}  // namespace

extern "C" {

int sqe_index_range_search_where(sqe_index* idx, const float* q_host, int B, const float* min_cos_host, int max_hits,
                                 const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                                 const int64_t* allow_ids_host, int64_t n_allow, int64_t* count_out_host, float* cos_out_host,
                                 int64_t* id_out_host) {
    int64_t one[2];
    SQE_TRY(radial_args_ok(idx, q_host, B, min_cos_host, max_hits, count_out_host, cos_out_host, id_out_host));
    SQE_TRY(set_args_ok("sqe_index_range_search_where", clauses, n_clauses, set_values, n_set, allow_ids_host, n_allow, one));
    if (B == 0) return SQE_OK;
    SQE_TRY(thresholds_ok(min_cos_host, B));
    const RowSet set{FieldPreds{clauses, one, 1, set_values, n_set}, allow_ids_host, n_allow, true};
    if (idx->group)
        return group_index_range_search(idx, q_host, B, min_cos_host, max_hits, count_out_host, cos_out_host, id_out_host, false, &set);
    OpScope op(idx->ctx, idx->ord, true);
    WithinState* w = within_state(idx);
    if (!w) return fail(SQE_ERR_OOM, "sqe_index_range_search_where: host allocation failed");
    const int64_t bm = (int64_t)B * max_hits;
    const size_t qb = round16((size_t)B * idx->dim * 4), tb = round16((size_t)B * 4), nb = (size_t)B * 8;
    const size_t cb = round16((size_t)bm * 4), ib = (size_t)bm * 8;
    SQE_TRY(w->stage.ensure(qb + tb + nb + cb + ib));
    char* p = w->stage.as<char>();
    float* q_dev = reinterpret_cast<float*>(p);
    float* t_dev = reinterpret_cast<float*>(p + qb);
    int64_t* n_dev = reinterpret_cast<int64_t*>(p + qb + tb);
    float* c_dev = reinterpret_cast<float*>(p + qb + tb + nb);
    int64_t* i_dev = reinterpret_cast<int64_t*>(p + qb + tb + nb + cb);
    SQE_HIP(hipMemcpyAsync(q_dev, q_host, (size_t)B * idx->dim * 4, hipMemcpyHostToDevice, op.s));
    SQE_HIP(hipMemcpyAsync(t_dev, min_cos_host, (size_t)B * 4, hipMemcpyHostToDevice, op.s));
    SQE_TRY(index_range_search_within(idx, q_dev, B, t_dev, max_hits, set, n_dev, c_dev, i_dev, op.s));
    SQE_HIP(hipMemcpyAsync(count_out_host, n_dev, nb, hipMemcpyDeviceToHost, op.s));
    if (bm > 0) {
        SQE_HIP(hipMemcpyAsync(cos_out_host, c_dev, (size_t)bm * 4, hipMemcpyDeviceToHost, op.s));
        SQE_HIP(hipMemcpyAsync(id_out_host, i_dev, ib, hipMemcpyDeviceToHost, op.s));
    }
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_range_search_where_device(sqe_index* idx, const float* q_dev, int B, const float* min_cos_dev, int max_hits,
                                        const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                                        const int64_t* allow_ids_dev, int64_t n_allow, int64_t* count_out_dev, float* cos_out_dev,
                                        int64_t* id_out_dev) {
    int64_t one[2];
    SQE_TRY(radial_args_ok(idx, q_dev, B, min_cos_dev, max_hits, count_out_dev, cos_out_dev, id_out_dev));
    SQE_TRY(set_args_ok("sqe_index_range_search_where", clauses, n_clauses, set_values, n_set, allow_ids_dev, n_allow, one));
    if (B == 0) return SQE_OK;
    // the thresholds come to the host first (after the caller's work on the context stream): NaN check and group planning
    std::vector<float> t((size_t)B);
    {
        sqe_ctx* c = idx->ctx;
        SQE_HIP(hipSetDevice(c->device));
        hipStream_t s = c->stream.load();
        SQE_HIP(hipMemcpyAsync(t.data(), min_cos_dev, (size_t)B * 4, hipMemcpyDeviceToHost, s));
        SQE_HIP(hipStreamSynchronize(s));
    }
    SQE_TRY(thresholds_ok(t.data(), B));
    const FieldPreds pr{clauses, one, 1, set_values, n_set};
    if (idx->group) {
        std::vector<int64_t> allow;
        SQE_TRY(group_allow(idx, allow_ids_dev, n_allow, allow));
        const RowSet set{pr, allow.data(), n_allow, true};
        return group_index_range_search(idx, q_dev, B, t.data(), max_hits, count_out_dev, cos_out_dev, id_out_dev, true, &set);
    }
    OpScope op(idx->ctx, idx->ord, false);
    return index_range_search_within(idx, q_dev, B, min_cos_dev, max_hits, RowSet{pr, allow_ids_dev, n_allow, false}, count_out_dev,
                                     cos_out_dev, id_out_dev, op.s);
}

int sqe_index_search_collapsed_where(sqe_index* idx, const float* q_host, int B, int k, const sqe_field_clause_t* clauses, int n_clauses,
                                     const int64_t* set_values, int64_t n_set, const int64_t* allow_ids_host, int64_t n_allow,
                                     float* cos_out_host, int64_t* id_out_host, int64_t* key_out_host) {
    int64_t one[2];
    SQE_TRY(collapsed_args_ok(idx, q_host, B, k, cos_out_host, id_out_host, key_out_host));
    SQE_TRY(set_args_ok("sqe_index_search_collapsed_where", clauses, n_clauses, set_values, n_set, allow_ids_host, n_allow, one));
    if (B == 0) return SQE_OK;
    const RowSet set{FieldPreds{clauses, one, 1, set_values, n_set}, allow_ids_host, n_allow, true};
    if (idx->group) return group_index_search_collapsed(idx, q_host, B, k, cos_out_host, id_out_host, key_out_host, false, &set);
    OpScope op(idx->ctx, idx->ord, true);
    WithinState* w = within_state(idx);
    if (!w) return fail(SQE_ERR_OOM, "sqe_index_search_collapsed_where: host allocation failed");
    const int64_t bk = (int64_t)B * k;
    const size_t qb = round16((size_t)B * idx->dim * 4), cb = round16((size_t)bk * 4), ib = (size_t)bk * 8;
    SQE_TRY(w->stage.ensure(qb + cb + 2 * ib));
    char* p = w->stage.as<char>();
    float* q_dev = reinterpret_cast<float*>(p);
    float* c_dev = reinterpret_cast<float*>(p + qb);
    int64_t* i_dev = reinterpret_cast<int64_t*>(p + qb + cb);
    int64_t* k_dev = reinterpret_cast<int64_t*>(p + qb + cb + ib);
    SQE_HIP(hipMemcpyAsync(q_dev, q_host, (size_t)B * idx->dim * 4, hipMemcpyHostToDevice, op.s));
    SQE_TRY(index_search_collapsed_within(idx, q_dev, B, k, set, c_dev, i_dev, k_dev, op.s));
    SQE_HIP(hipMemcpyAsync(cos_out_host, c_dev, (size_t)bk * 4, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(id_out_host, i_dev, ib, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(key_out_host, k_dev, ib, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_search_collapsed_where_device(sqe_index* idx, const float* q_dev, int B, int k, const sqe_field_clause_t* clauses,
                                            int n_clauses, const int64_t* set_values, int64_t n_set, const int64_t* allow_ids_dev,
                                            int64_t n_allow, float* cos_out_dev, int64_t* id_out_dev, int64_t* key_out_dev) {
    int64_t one[2];
    SQE_TRY(collapsed_args_ok(idx, q_dev, B, k, cos_out_dev, id_out_dev, key_out_dev));
    SQE_TRY(set_args_ok("sqe_index_search_collapsed_where", clauses, n_clauses, set_values, n_set, allow_ids_dev, n_allow, one));
    if (B == 0) return SQE_OK;
    const FieldPreds pr{clauses, one, 1, set_values, n_set};
    if (idx->group) {
        std::vector<int64_t> allow;
        SQE_TRY(group_allow(idx, allow_ids_dev, n_allow, allow));
        const RowSet set{pr, allow.data(), n_allow, true};
        return group_index_search_collapsed(idx, q_dev, B, k, cos_out_dev, id_out_dev, key_out_dev, true, &set);
    }
    OpScope op(idx->ctx, idx->ord, false);
    return index_search_collapsed_within(idx, q_dev, B, k, RowSet{pr, allow_ids_dev, n_allow, false}, cos_out_dev, id_out_dev, key_out_dev,
                                         op.s);
}

int sqe_index_search_mmr_where(sqe_index* idx, const float* q_host, int B, int k, int n_cand, const float* lambda_host, int nprobe,
                               const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                               const int64_t* allow_ids_host, int64_t n_allow, float* cos_out_host, int64_t* id_out_host,
                               float* mmr_out_host) {
    int64_t one[2];
    SQE_TRY(mmr_args_ok(idx, q_host, B, k, n_cand, lambda_host, cos_out_host, id_out_host, mmr_out_host));
    SQE_TRY(set_args_ok("sqe_index_search_mmr_where", clauses, n_clauses, set_values, n_set, allow_ids_host, n_allow, one));
    if (B == 0) return SQE_OK;
    const int n = mmr_depth_of(k, n_cand);
    const RowSet set{FieldPreds{clauses, one, 1, set_values, n_set}, allow_ids_host, n_allow, true};
    if (idx->group)
        return group_index_search_mmr(idx, q_host, B, k, n, lambda_host, nprobe, cos_out_host, id_out_host, mmr_out_host, false, &set);
    OpScope op(idx->ctx, idx->ord, true);
    WithinState* w = within_state(idx);
    if (!w) return fail(SQE_ERR_OOM, "sqe_index_search_mmr_where: host allocation failed");
    const MmrOut O = MmrOut::of(B, k);
    const size_t qb = round16((size_t)B * idx->dim * 4), lb = round16((size_t)B * 4);
    SQE_TRY(w->stage.ensure(qb + lb + O.total));
    char* p = w->stage.as<char>();
    float* q_dev = reinterpret_cast<float*>(p);
    float* l_dev = reinterpret_cast<float*>(p + qb);
    char* o_dev = p + qb + lb;
    SQE_HIP(hipMemcpyAsync(q_dev, q_host, (size_t)B * idx->dim * 4, hipMemcpyHostToDevice, op.s));
    SQE_HIP(hipMemcpyAsync(l_dev, lambda_host, (size_t)B * 4, hipMemcpyHostToDevice, op.s));
    SQE_TRY(index_search_mmr_within(idx, q_dev, B, k, n, l_dev, set, reinterpret_cast<float*>(o_dev + O.cos_off),
                                    reinterpret_cast<int64_t*>(o_dev + O.id_off), reinterpret_cast<float*>(o_dev + O.mmr_off), op.s));
    SQE_HIP(hipMemcpyAsync(cos_out_host, o_dev + O.cos_off, O.cos_bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(id_out_host, o_dev + O.id_off, O.id_bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(mmr_out_host, o_dev + O.mmr_off, O.cos_bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_search_mmr_where_device(sqe_index* idx, const float* q_dev, int B, int k, int n_cand, const float* lambda_host, int nprobe,
                                      const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                                      const int64_t* allow_ids_dev, int64_t n_allow, float* cos_out_dev, int64_t* id_out_dev,
                                      float* mmr_out_dev) {
    int64_t one[2];
    SQE_TRY(mmr_args_ok(idx, q_dev, B, k, n_cand, lambda_host, cos_out_dev, id_out_dev, mmr_out_dev));
    SQE_TRY(set_args_ok("sqe_index_search_mmr_where", clauses, n_clauses, set_values, n_set, allow_ids_dev, n_allow, one));
    if (B == 0) return SQE_OK;
    const int n = mmr_depth_of(k, n_cand);
    const FieldPreds pr{clauses, one, 1, set_values, n_set};
    if (idx->group) {
        std::vector<int64_t> allow;
        SQE_TRY(group_allow(idx, allow_ids_dev, n_allow, allow));
        const RowSet set{pr, allow.data(), n_allow, true};
        return group_index_search_mmr(idx, q_dev, B, k, n, lambda_host, nprobe, cos_out_dev, id_out_dev, mmr_out_dev, true, &set);
    }
    OpScope op(idx->ctx, idx->ord, false);
    WithinState* w = within_state(idx);
    if (!w) return fail(SQE_ERR_OOM, "sqe_index_search_mmr_where: host allocation failed");
    // the weights are host memory: the copy is staged before the call returns, and nothing is read back
    SQE_TRY(w->lam.ensure((size_t)B * 4));
    SQE_HIP(hipMemcpyAsync(w->lam.p, lambda_host, (size_t)B * 4, hipMemcpyHostToDevice, op.s));
    return index_search_mmr_within(idx, q_dev, B, k, n, w->lam.as<float>(), RowSet{pr, allow_ids_dev, n_allow, false}, cos_out_dev, id_out_dev,
                                   mmr_out_dev, op.s);
}

int sqe_index_within_last(sqe_index* idx, sqe_within_last_t* out) {
    if (!idx || !out) return fail(SQE_ERR_INVALID, "sqe_index_within_last: null argument");
    if (idx->group) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_within_last: single-device indexes only");
    std::lock_guard<std::mutex> lk(idx->ord.mu);
    if (idx->within_last.live < 0) return fail(SQE_ERR_STATE, "sqe_index_within_last: no restricted search ran on this index yet");
    *out = idx->within_last;
    return SQE_OK;
}

}  // extern "C"
