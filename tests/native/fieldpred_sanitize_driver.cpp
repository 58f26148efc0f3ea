// Sanitizer driver for the host-only code of the field predicates, csrc/fieldpred.cpp (test infrastructure): fieldpred_check and
// fieldpred_plan under -fsanitize=address,undefined.  Built by `make -C semantic_query_engine_amd/csrc fieldpred_asan` with g++
// -- no HIP code is involved.  The clause tables arrive through the C ABI from callers the library does not trust: offsets that do
// not start at 0 or decrease, too many predicates, clauses or set values, slots and ops out of range and IN slices outside the set
// values or out of order must be refused before anything indexes with them.
//
//   fieldpred_asan <cases file> <out file>
// cases file: repeated { int64 n_preds; int64 no; int64 offsets[no]; int64 nc; clause[nc] (int32 field, int32 op, int64 lo,
// int64 hi); int64 n_set; int64 ns; int64 set_values[ns] }.  no, nc and ns are what the WRITER of the case allocated, not what the
// tables claim: every array is handed over as an exact-size heap copy, so a read past it is a heap-buffer-overflow ASan reports.
// out, per case: int32 status (0 well formed, 1 refused); for a well-formed case the plan: int32 first[9]; int32 n; then per
// planned clause int32 field, op, pred and int64 lo, hi.  tests/test_fields_cpu.py compares all of it with a NumPy restatement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fieldpred.h"

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) { fprintf(stderr, "REQUIRE failed: %s (line %d)\n", #c, __LINE__); exit(3); } \
    } while (0)

template <typename T>
static T* exact_copy(const char* src, size_t count) {
    T* p = (T*)malloc(count ? count * sizeof(T) : 1);
    if (count) memcpy(p, src, count * sizeof(T));
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s cases out\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    REQUIRE(f);
    std::vector<char> cases;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) cases.insert(cases.end(), buf, buf + got);
    fclose(f);

    // the checks themselves
    const int64_t z[2] = {0, 0};
    REQUIRE(sqe::fieldpred_check(nullptr, nullptr, 0, nullptr, 0) == nullptr);       // no predicate needs no table
    REQUIRE(sqe::fieldpred_check(nullptr, nullptr, 1, nullptr, 0) != nullptr);
    REQUIRE(sqe::fieldpred_check(nullptr, z, 1, nullptr, 0) == nullptr);             // one empty predicate
    REQUIRE(sqe::fieldpred_check(nullptr, z, -1, nullptr, 0) != nullptr);
    REQUIRE(sqe::fieldpred_check(nullptr, z, 1, nullptr, 1) != nullptr);             // set values announced, none given
    static_assert(sizeof(sqe::FieldClause) == 24 && sizeof(sqe::FieldPlanClause) == 32, "table layouts");

    FILE* out = fopen(argv[2], "wb");
    REQUIRE(out);
    size_t pos = 0, n_cases = 0;
    const auto read64 = [&]() {
        int64_t v;
        REQUIRE(pos + 8 <= cases.size());
        memcpy(&v, cases.data() + pos, 8);
        pos += 8;
        return v;
    };
    sqe::FieldPlan plan;
    while (pos < cases.size()) {
        const int64_t n_preds = read64();
        const int64_t no = read64();
        REQUIRE(no >= 0 && pos + (size_t)no * 8 <= cases.size());
        int64_t* offsets = exact_copy<int64_t>(cases.data() + pos, (size_t)no);
        pos += (size_t)no * 8;
        const int64_t nc = read64();
        REQUIRE(nc >= 0 && pos + (size_t)nc * 24 <= cases.size());
        sqe::FieldClause* clauses = exact_copy<sqe::FieldClause>(cases.data() + pos, (size_t)nc);
        pos += (size_t)nc * 24;
        const int64_t n_set = read64();
        const int64_t ns = read64();
        REQUIRE(ns >= 0 && pos + (size_t)ns * 8 <= cases.size());
        int64_t* sets = exact_copy<int64_t>(cases.data() + pos, (size_t)ns);
        pos += (size_t)ns * 8;
        // a case never announces more than it allocated, except where the announcement itself must be refused first
        const char* why = sqe::fieldpred_check(clauses, offsets, n_preds, sets, n_set);
        const int32_t status = why ? 1 : 0;
        fwrite(&status, 4, 1, out);
        if (!why) {
            REQUIRE(n_preds == 0 || (no == n_preds + 1 && offsets[n_preds] <= nc));
            REQUIRE(n_set <= ns);
            sqe::fieldpred_plan(clauses, offsets, (int)n_preds, plan);
            REQUIRE(plan.first[0] == 0 && plan.first[sqe::FIELD_MAX] == (int)plan.clauses.size());
            fwrite(plan.first, 4, sqe::FIELD_MAX + 1, out);
            const int32_t n = (int32_t)plan.clauses.size();
            fwrite(&n, 4, 1, out);
            for (const sqe::FieldPlanClause& c : plan.clauses) {
                fwrite(&c.field, 4, 1, out);
                fwrite(&c.op, 4, 1, out);
                fwrite(&c.pred, 4, 1, out);
                fwrite(&c.lo, 8, 1, out);
                fwrite(&c.hi, 8, 1, out);
            }
        }
        free(offsets);
        free(clauses);
        free(sets);
        ++n_cases;
    }
    fclose(out);
    printf("ok %zu cases\n", n_cases);
    return 0;
}
