// fieldpred.h -- host-only code of the field predicates (fieldpred.cpp): the checks of the clause tables as they arrive through
// the C ABI, the plan the match kernel reads and the depth rule of the mask route.  Plain C++ (no HIP header), so it also builds with g++ under the sanitizers
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

// The depth of the first stage of the mask route of sqe_index_search_where (where_mask.hip): with f = selected / live, the
// smallest d in [k, 256] for which P[Binomial(d, f) < k] <= 2^-10 in double arithmetic -- if the rows a predicate selects were
// drawn independently of the query, a pass of 1,024 queries then expects at most one query with fewer than k selected rows among
// its d nearest -- and 0 when there is none, when selected < k, or when k is outside 1..256.
constexpr int WHERE_MAX_DEPTH = 256;
constexpr double WHERE_FLAG_RATE = 1.0 / 1024.0;
int where_depth(int k, int64_t selected, int64_t live);

// The cost rule of the automatic route: whether searching all `live` rows at depth d (int8 or bf16 first pass) and masking the
// hits is expected to be cheaper than gathering the `selected` rows and searching those.  Both routes stream rows, so both costs
// are taken per live row and the index's size and dimension cancel: with f = selected / live and b = min(B, 1024) / 1024,
//   bf16(b, d) = BF16_64 + BF16_64_B b                                   for d <= 64
//                BF16_128 + BF16_128_B b + max(0, d - 128) (DEEP + DEEP_B b)   beyond
//   gather = f (COPY + bf16(b, k) (GATHER_DEEP if k > 64))
//   mask   = (I8 + I8_B b  or  bf16(b, d)) + SWEEP b
// in milliseconds of the 10 M x 1024 measurement the constants were fitted to (profiles/where_mask/NOTES.md has the fit).
constexpr double WHERE_COST_COPY = 21.8, WHERE_COST_GATHER_DEEP = 2.2;
constexpr double WHERE_COST_I8 = 1.9, WHERE_COST_I8_B = 7.6;
constexpr double WHERE_COST_BF16_64 = 3.4, WHERE_COST_BF16_64_B = 16.0, WHERE_COST_BF16_128 = 6.9, WHERE_COST_BF16_128_B = 51.0;
constexpr double WHERE_COST_DEEP = 0.008, WHERE_COST_DEEP_B = 0.75, WHERE_COST_SWEEP = 6.0;
bool where_mask_cheaper(int64_t live, int64_t selected, int B, int k, int d, bool i8);

}  // namespace sqe

extern "C" int sqe_where_depth(int k, int64_t selected, int64_t live);      // the same through the C ABI (include/sqe.h)
