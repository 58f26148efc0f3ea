// Stand-alone driver of the host-only field sort code (csrc/fieldsort.cpp) for the AddressSanitizer + UndefinedBehaviorSanitizer
// build (make fieldsort_asan).  Every table lives in a heap block of exactly its size, so a read past a fault is an error.
// It reads cases from stdin and prints one line per case; tests/test_sort_cpu.py compares the lines with the Python model.
//   check  n_sort k n_given  field flags ...          -> "check ok" | "check <fault text>"     (n_given pairs follow; 0: a null spec)
//   image  flags v                                    -> "image <u>"
//   cursor n_sort  field flags ...  v ...             -> "cursor <u> ..."
//   less   n_sort  u ... id   u ... id                -> "less 0|1"
//   merge  n_sort k  field flags ...  n_lists  { m  (id v ...) x m } x n_lists   -> "merge id ... | v ..."
#include <stdio.h>

#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "fieldsort.h"

using namespace sqe;

static std::unique_ptr<FieldSort[]> read_spec(int n) {
    std::unique_ptr<FieldSort[]> s(n > 0 ? new FieldSort[n] : nullptr);
    for (int j = 0; j < n; ++j) std::cin >> s[j].field >> s[j].flags;
    return s;
}

int main() {
    std::string op;
    while (std::cin >> op) {
        if (op == "check") {
            long long n_sort, k;
            int given;
            std::cin >> n_sort >> k >> given;
            auto spec = read_spec(given);
            const char* why = fieldsort_check(spec.get(), n_sort, k);
            printf("check %s\n", why ? why : "ok");
        } else if (op == "image") {
            int flags;
            long long v;
            std::cin >> flags >> v;
            printf("image %llu\n", (unsigned long long)sort_image((int64_t)v, flags));
        } else if (op == "cursor") {
            int n;
            std::cin >> n;
            auto spec = read_spec(n);
            std::unique_ptr<int64_t[]> v(new int64_t[n]);
            std::unique_ptr<uint64_t[]> u(new uint64_t[n]);
            for (int j = 0; j < n; ++j) {
                long long x;
                std::cin >> x;
                v[j] = x;
            }
            fieldsort_cursor(spec.get(), n, v.get(), u.get());
            printf("cursor");
            for (int j = 0; j < n; ++j) printf(" %llu", (unsigned long long)u[j]);
            printf("\n");
        } else if (op == "less") {
            int n;
            std::cin >> n;
            SortTuple t[2] = {};
            for (auto& x : t) {
                for (int j = 0; j < n; ++j) {
                    unsigned long long u;
                    std::cin >> u;
                    x.u[j] = u;
                }
                long long id;
                std::cin >> id;
                x.id = id;
            }
            printf("less %d\n", fieldsort_less(t[0], t[1], n) ? 1 : 0);
        } else if (op == "merge") {
            int n, k, n_lists;
            std::cin >> n >> k;
            auto spec = read_spec(n);
            std::cin >> n_lists;
            std::vector<std::vector<int64_t>> ids((size_t)n_lists), values((size_t)n_lists);
            for (int p = 0; p < n_lists; ++p) {
                int m;
                std::cin >> m;
                for (int i = 0; i < m; ++i) {
                    long long x;
                    std::cin >> x;
                    ids[(size_t)p].push_back(x);
                    for (int j = 0; j < n; ++j) {
                        std::cin >> x;
                        values[(size_t)p].push_back(x);
                    }
                }
                ids[(size_t)p].shrink_to_fit();
                values[(size_t)p].shrink_to_fit();
            }
            std::unique_ptr<int64_t[]> id_out(new int64_t[k]), value_out(new int64_t[(size_t)k * n]);
            fieldsort_merge(spec.get(), n, k, ids, values, id_out.get(), value_out.get());
            printf("merge");
            for (int i = 0; i < k; ++i) printf(" %lld", (long long)id_out[i]);
            printf(" |");
            for (int i = 0; i < k * n; ++i) printf(" %lld", (long long)value_out[i]);
            printf("\n");
        } else {
            fprintf(stderr, "unknown op %s\n", op.c_str());
            return 2;
        }
    }
    return 0;
}
