// fieldsort.cpp -- host-only code of the field sort: see fieldsort.h.
#include "fieldsort.h"

#include <algorithm>

namespace sqe {

const char* fieldsort_check(const FieldSort* sort, int64_t n_sort, int64_t k) {
    if (n_sort < 1 || n_sort > SORT_MAX_KEYS) return "between 1 and 4 sort keys";
    if (!sort) return "null sort";
    if (k < 1 || k > SORT_MAX_K) return "need 1 <= k <= 256";
    unsigned seen = 0;
    for (int64_t j = 0; j < n_sort; ++j) {
        if (sort[j].field < 0 || sort[j].field >= SORT_FIELD_SLOTS) return "a sort key names a field slot outside 0..7";
        if (sort[j].flags & ~(SORT_DESC | SORT_MISSING_FIRST)) return "unknown sort flag bits";
        if (seen & (1u << sort[j].field)) return "a field slot is named by two sort keys";
        seen |= 1u << sort[j].field;
    }
    return nullptr;
}

void fieldsort_cursor(const FieldSort* sort, int n_sort, const int64_t* after_values, uint64_t* image_out) {
    for (int j = 0; j < n_sort; ++j) image_out[j] = sort_image(after_values[j], sort[j].flags);
}

bool fieldsort_less(const SortTuple& a, const SortTuple& b, int n_sort) {
    for (int j = 0; j < n_sort; ++j)
        if (a.u[j] != b.u[j]) return a.u[j] < b.u[j];
    return a.id < b.id;
}

void fieldsort_merge(const FieldSort* sort, int n_sort, int k, const std::vector<std::vector<int64_t>>& ids,
                     const std::vector<std::vector<int64_t>>& values, int64_t* id_out, int64_t* value_out) {
    struct Entry { SortTuple t; size_t list, at; };
    std::vector<Entry> all;
    for (size_t p = 0; p < ids.size(); ++p)
        for (size_t i = 0; i < ids[p].size(); ++i) {
            Entry e{};
            for (int j = 0; j < n_sort; ++j) e.t.u[j] = sort_image(values[p][i * (size_t)n_sort + (size_t)j], sort[j].flags);
            e.t.id = ids[p][i];
            e.list = p;
            e.at = i;
            all.push_back(e);
        }
    std::sort(all.begin(), all.end(), [n_sort](const Entry& a, const Entry& b) { return fieldsort_less(a.t, b.t, n_sort); });
    for (int i = 0; i < k; ++i) {
        const bool have = (size_t)i < all.size();
        id_out[i] = have ? all[(size_t)i].t.id : -1;
        for (int j = 0; j < n_sort; ++j)
            value_out[(size_t)i * (size_t)n_sort + (size_t)j] =
                have ? values[all[(size_t)i].list][all[(size_t)i].at * (size_t)n_sort + (size_t)j] : SORT_FIELD_NONE;
    }
}

}  // namespace sqe
