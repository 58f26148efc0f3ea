// fieldpred.cpp -- host-only code of the field predicates: see fieldpred.h.
#include "fieldpred.h"

namespace sqe {

const char* fieldpred_check(const FieldClause* clauses, const int64_t* pred_offsets, int64_t n_preds, const int64_t* set_values,
                            int64_t n_set) {
    if (n_preds < 0 || n_preds > FIELD_MAX_PREDS) return "between 0 and 64 predicates per call";
    if (n_set < 0 || n_set > FIELD_MAX_SET) return "between 0 and 4096 set values per call";
    if (n_set > 0 && !set_values) return "null set_values";
    if (n_preds == 0) return nullptr;
    if (!pred_offsets) return "null pred_offsets";
    if (pred_offsets[0] != 0) return "pred_offsets must start at 0";
    for (int64_t j = 0; j < n_preds; ++j) {
        if (pred_offsets[j + 1] < pred_offsets[j]) return "pred_offsets decrease";
        if (pred_offsets[j + 1] - pred_offsets[j] > FIELD_MAX_CLAUSES) return "more than 8 clauses in a predicate";
    }
    const int64_t nc = pred_offsets[n_preds];
    if (nc > 0 && !clauses) return "null clauses";
    for (int64_t c = 0; c < nc; ++c) {
        const FieldClause& cl = clauses[c];
        if (cl.field < 0 || cl.field >= FIELD_MAX) return "a clause names a field slot outside 0..7";
        const int32_t op = cl.op & ~FIELD_OP_NOT;
        if (op != FIELD_OP_RANGE && op != FIELD_OP_IN) return "unknown clause op";
        if (op == FIELD_OP_IN) {
            if (cl.lo < 0 || cl.hi < cl.lo || cl.hi > n_set) return "an IN clause's slice lies outside set_values";
            for (int64_t i = cl.lo + 1; i < cl.hi; ++i)
                if (set_values[i] <= set_values[i - 1]) return "an IN clause's values are not strictly ascending";
        }
    }
    return nullptr;
}

void fieldpred_plan(const FieldClause* clauses, const int64_t* pred_offsets, int n_preds, FieldPlan& out) {
    out.clauses.clear();
    for (int f = 0; f < FIELD_MAX; ++f) {
        out.first[f] = (int)out.clauses.size();
        for (int j = 0; j < n_preds; ++j)
            for (int64_t c = pred_offsets[j]; c < pred_offsets[j + 1]; ++c)
                if (clauses[c].field == f) out.clauses.push_back({clauses[c].lo, clauses[c].hi, f, clauses[c].op, j, 0});
    }
    out.first[FIELD_MAX] = (int)out.clauses.size();
}

}  // namespace sqe
