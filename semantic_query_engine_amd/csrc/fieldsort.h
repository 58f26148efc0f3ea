// fieldsort.h -- host-only code of the field sort (fieldsort.cpp; sqe_index_sort_fields): the checks of the sort spec as it
// arrives through the C ABI, the order images, the tuple comparator and the exact merge of the shards' lists on a device group.
// Plain C++ (no HIP header), so it also builds with g++ under the sanitizers (make fieldsort_asan); sort.hip includes it and
// uses the same image function on the device.
#pragma once

#include <stdint.h>

#include <vector>

#ifdef __HIPCC__
#define SQE_SORT_HD __host__ __device__
#else
#define SQE_SORT_HD
#endif

namespace sqe {

constexpr int SORT_MAX_KEYS = 4;           // sort keys of one call
constexpr int SORT_MAX_K = 256;            // rows a call returns at most (MAX_KP)
constexpr int SORT_FIELD_SLOTS = 8;        // SQE_MAX_FIELDS
constexpr int64_t SORT_FIELD_NONE = INT64_MIN;     // SQE_FIELD_NONE
constexpr int SORT_DESC = 1, SORT_MISSING_FIRST = 2;       // SQE_SORT_DESC, SQE_SORT_MISSING_FIRST

struct FieldSort {         // sqe_field_sort_t
    int32_t field, flags;
};

// The order image of a raw value: rows sort by their images ASCENDING, whatever the direction and the missing placement.
// b = v ^ 2^63 lies in [1, 2^64 - 1] for a present value (never INT64_MIN), so the 2^64 - 1 values and "missing" fill the
// 64 bits exactly:             present           missing
//   asc,  missing last         b - 1             2^64 - 1
//   asc,  missing first        b                 0
//   desc, missing last         ~b                2^64 - 1
//   desc, missing first        -b                0
SQE_SORT_HD inline uint64_t sort_image(int64_t v, int flags) {
    const bool first = (flags & SORT_MISSING_FIRST) != 0;
    if (v == SORT_FIELD_NONE) return first ? 0ull : ~0ull;
    const uint64_t b = (uint64_t)v ^ 0x8000000000000000ull;
    if (flags & SORT_DESC) return first ? 0ull - b : ~b;
    return first ? b : b - 1;
}

// 1 <= n_sort <= 4, every slot in 0..7 and named once, no flag bit beyond DESC | MISSING_FIRST, 1 <= k <= 256.  Returns null
// when the spec is well formed, else a static text that names the fault; reads nothing past a fault.
const char* fieldsort_check(const FieldSort* sort, int64_t n_sort, int64_t k);

// the images of a cursor's raw values (SQE_FIELD_NONE: missing) under a checked spec
void fieldsort_cursor(const FieldSort* sort, int n_sort, const int64_t* after_values, uint64_t* image_out);

struct SortTuple {         // a row as the order sees it: images of its values in the sort slots, then its id
    uint64_t u[SORT_MAX_KEYS];
    int64_t id;
};
// a before b in the order (u_0, ..., u_{n_sort - 1}, id) ascending; the order is total over distinct ids
bool fieldsort_less(const SortTuple& a, const SortTuple& b, int n_sort);

// Device groups: list p holds ids[p] / values[p] (n_sort raw values per id), each at most k entries in any order.  The first
// min(k, all entries) of their union in the order go to id_out [k] and value_out [k, n_sort], the rest is padded with
// (-1, SQE_FIELD_NONE).  Exact: a group's first k rows are among its shards' first k rows each.
void fieldsort_merge(const FieldSort* sort, int n_sort, int k, const std::vector<std::vector<int64_t>>& ids,
                     const std::vector<std::vector<int64_t>>& values, int64_t* id_out, int64_t* value_out);

}  // namespace sqe
