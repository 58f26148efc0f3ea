// fieldpred.h -- host-only code of the field predicates (fieldpred.cpp): the checks of the clause tables as they arrive through
// the C ABI and the plan the match kernel reads.  Plain C++ (no HIP header), so it also builds with g++ under the sanitizers
// (make fieldpred_asan).
#pragma once

#include <stdint.h>

#include <vector>

namespace sqe {

constexpr int FIELD_MAX = 8;               // field slots of an index (SQE_MAX_FIELDS)
constexpr int FIELD_MAX_PREDS = 64;        // predicates of one call
constexpr int FIELD_MAX_CLAUSES = 8;       // clauses of one predicate
constexpr int FIELD_MAX_SET = 4096;        // set values of one call
constexpr int64_t FIELD_NONE = INT64_MIN;  // SQE_FIELD_NONE: a row without a value
constexpr int FIELD_OP_RANGE = 0, FIELD_OP_IN = 1, FIELD_OP_NOT = 0x100;

struct FieldClause {       // sqe_field_clause_t
    int32_t field, op;
    int64_t lo, hi;
};

// Predicate j owns the clauses pred_offsets[j] .. pred_offsets[j + 1].  0 <= n_preds <= 64; the offsets start at 0, do not
// decrease and give no predicate more than 8 clauses; 0 <= n_set <= 4096; every clause names a slot in [0, 8) and an op RANGE or
// IN, with or without NOT; an IN clause's [lo, hi) lies in [0, n_set] and its slice of set_values is strictly ascending.
// Returns null when the tables are well formed, else a static text that names the fault; reads nothing past a fault (the
// clauses are not touched when the offsets are malformed, the set values only inside a checked slice).
const char* fieldpred_check(const FieldClause* clauses, const int64_t* pred_offsets, int64_t n_preds, const int64_t* set_values,
                            int64_t n_set);

struct FieldPlanClause {   // 32 bytes, as the kernel stages them
    int64_t lo, hi;
    int32_t field, op, pred, pad;
};
struct FieldPlan {
    std::vector<FieldPlanClause> clauses;      // sorted by field (stable): the kernel reads a column once for all its clauses
    int first[FIELD_MAX + 1];                  // the clauses of field f are [first[f], first[f + 1])
};
// the plan of checked tables
void fieldpred_plan(const FieldClause* clauses, const int64_t* pred_offsets, int n_preds, FieldPlan& out);

}  // namespace sqe
