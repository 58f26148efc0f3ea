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

int where_depth(int k, int64_t selected, int64_t live) {
    if (k < 1 || k > WHERE_MAX_DEPTH || live <= 0 || selected < k) return 0;
    const double f = selected >= live ? 1.0 : (double)selected / (double)live;
    // p[i] = P[Binomial(d, f) = i] for i < k, carried from d - 1 to d: only sums and products of non-negative numbers, so the
    // tail keeps a relative error of a few hundred ulps whatever f is (an entry that underflows is below 1e-308 of a tail
    // that is compared with 2^-10)
    double p[WHERE_MAX_DEPTH] = {0};
    p[0] = 1.0;
    for (int d = 1; d <= WHERE_MAX_DEPTH; ++d) {
        for (int i = (d < k ? d : k - 1); i > 0; --i) p[i] = p[i] * (1.0 - f) + p[i - 1] * f;
        p[0] *= 1.0 - f;
        if (d < k) continue;
        double tail = 0.0;
        for (int i = k - 1; i >= 0; --i) tail += p[i];
        if (tail <= WHERE_FLAG_RATE) return d;
    }
    return 0;
}

// a bf16 search of every live row at depth d (b = the batch as a fraction of a pass): the scan keeps 64, 128 or 256 candidates
// per chunk and query, and beyond 128 its cost grows with every further row of depth
static double where_cost_bf16(double b, int d) {
    if (d <= 64) return WHERE_COST_BF16_64 + WHERE_COST_BF16_64_B * b;
    double c = WHERE_COST_BF16_128 + WHERE_COST_BF16_128_B * b;
    if (d > 128) c += (double)(d - 128) * (WHERE_COST_DEEP + WHERE_COST_DEEP_B * b);
    return c;
}

bool where_mask_cheaper(int64_t live, int64_t selected, int B, int k, int d, bool i8) {
    if (live <= 0 || selected <= 0) return false;
    const double f = selected >= live ? 1.0 : (double)selected / (double)live;
    const double b = (double)(B < 1024 ? (B > 0 ? B : 0) : 1024) / 1024.0;      // larger batches run in passes of 1,024 on both routes
    // gather: the copy of the selected rows, then a bf16 search of them at depth k (chunk by chunk, merged: dearer beyond 64)
    const double gather = f * (WHERE_COST_COPY + where_cost_bf16(b, k) * (k > 64 ? WHERE_COST_GATHER_DEEP : 1.0));
    // mask: the search of every row at depth d, and the sweep of the one query a full pass is expected to flag
    const double mask = (i8 ? WHERE_COST_I8 + WHERE_COST_I8_B * b : where_cost_bf16(b, d)) + WHERE_COST_SWEEP * b;
    return mask < gather;
}

}  // namespace sqe

extern "C" int sqe_where_depth(int k, int64_t selected, int64_t live) { return sqe::where_depth(k, selected, live); }
