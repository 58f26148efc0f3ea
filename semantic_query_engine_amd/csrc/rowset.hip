// rowset.hip -- the row set (internal.h: RowSet) that sqe_index_search_where, sqe_index_aggregate_fields, sqe_index_sort_fields and
// the _where forms of radial, collapsed and MMR search restrict their work to: the live rows a field predicate selects,
// intersected with an optional allow-list.  Here are the one check of its six C arguments, the one way a device list of a
// "_device" call reaches the host for a device group, and its preparation on the device in two steps:
//   rowset_map        the filter's map (filter.hip) sized for the index as it stands, the list marked in it, the field match kernel
//                     (fields.hip) written over it or, behind a list, ANDed into it.  Synchronises nothing.
//   rowset_positions  the map's set bits as ascending positions in the filter state, and their number M: one synchronisation.
// What an empty set (no rows, the empty list, M == 0) answers differs per call and stays with each caller.
#include <algorithm>
#include <vector>

#include "fieldpred.h"
#include "internal.h"

namespace sqe {

int rowset_args_ok(const char* who, const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                   const void* allow, int64_t n_allow, int64_t* one) {
    if (n_clauses < 0 || n_clauses > FIELD_MAX_CLAUSES) return fail(SQE_ERR_INVALID, std::string(who) + ": between 0 and 8 clauses");
    one[0] = 0;
    one[1] = n_clauses;
    SQE_TRY(fields_args_ok(who, FieldPreds{clauses, one, 1, set_values, n_set}));
    if (n_allow < -1 || (n_allow > 0 && !allow)) return fail(SQE_ERR_INVALID, std::string(who) + ": bad allow-list");
    return SQE_OK;
}

int rowset_allow_to_host(sqe_index* idx, const int64_t* allow_dev, int64_t n_allow, std::vector<int64_t>& out) {
    const int64_t one_list[2] = {0, std::max<int64_t>(n_allow, 0)};
    return list_ids_to_host(idx->ctx, allow_dev, one_list, 1, out);
}

int rowset_map(sqe_index* idx, const RowSet& set, FilterState** f_out, int64_t* words_out, hipStream_t s) {
    SQE_TRY(filter_bitmap_ensure(idx, f_out, words_out));
    FilterState* f = *f_out;
    StageTimer t(idx->ctx->prof, s, ST_PREP);
    if (set.n_allow > 0) {
        const int64_t* allow_dev = set.allow;
        if (set.allow_on_host) SQE_TRY(stage_allow_ids(f, set.allow, set.n_allow, s, &allow_dev));
        SQE_TRY(filter_bitmap_mark(idx, f, *words_out, allow_dev, set.n_allow, s));
    }
    // without a list the kernel writes every word of the map, the padding included
    return fields_bitmap_eval(idx, set.pr, filter_bitmap(f), set.n_allow > 0, s);
}

int rowset_positions(sqe_index* idx, const RowSet& set, FilterState* f, int64_t words, int64_t* M_out, hipStream_t s) {
    const int64_t n = idx->n.load();
    return index_bitmap_positions(idx, f, words, set.n_allow > 0 ? std::min(set.n_allow, n) : n, M_out, s);
}

}  // namespace sqe
