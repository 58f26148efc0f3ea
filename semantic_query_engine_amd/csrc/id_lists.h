// id_lists.h -- the device side of every call that takes row ids from the caller (delete, filtered, per-query filtered and
// exclusion search): id -> row position, and a set of 32-bit positions per list.
//
// The set is an open-addressing table of uint32 slots, linear probing, POS_SET_EMPTY in a free slot (the host clears a table
// with memset 0xFF).  pos_set_slots sizes it: load <= 0.5, so a probe meets its position or a free slot long before it has
// seen every slot.  Both probe loops nevertheless end after mask + 1 steps: a table that was sized or cleared wrongly gives a
// wrong answer, which a test catches, never a workgroup that does not end.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace sqe {

// position of `id` in the strictly increasing map[0, n) (first position with map[pos] >= id, a hit if equal), or -1;
// without a map a row's id is its position
__device__ __forceinline__ int64_t resolve_id(const int64_t* __restrict__ map, int64_t n, int64_t id) {
    if (!map) return id >= 0 && id < n ? id : -1;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (map[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && map[lo] == id ? lo : -1;
}

// deleted positions below or at i (del sorted ascending, m entries); *hit = i is deleted
__device__ __forceinline__ int64_t del_rank(const int64_t* __restrict__ del, int64_t m, int64_t i, bool* hit) {
    int64_t lo = 0, hi = m;                       // first index with del[idx] > i
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (del[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    *hit = lo > 0 && del[lo - 1] == i;
    return lo;
}

constexpr uint32_t POS_SET_EMPTY = 0xFFFFFFFFu;          // never a position: an index holds fewer than 2^32 rows
constexpr int64_t POS_SET_MAX_SLOTS = (int64_t)1 << 32;  // a larger table has no 32-bit mask: a list of more than 2^31 entries

// slots of the table of a list of `len` entries: the power of two >= 2 len, at least 2
constexpr int64_t pos_set_slots(int64_t len) {
    int64_t cap = 2;
    while (cap < 2 * len) cap <<= 1;
    return cap;
}
static_assert(pos_set_slots(0) == 2 && pos_set_slots(1) == 2 && pos_set_slots(2) == 4 && pos_set_slots(3) == 8, "table sizes");
static_assert(pos_set_slots(4) == 8 && pos_set_slots(5) == 16, "table sizes");
static_assert(pos_set_slots(((int64_t)1 << 31) - 1) == POS_SET_MAX_SLOTS, "table sizes");

// the product's high half folded into the bits a mask keeps
__device__ __forceinline__ uint32_t pos_set_hash(uint32_t p) {
    const uint32_t h = p * 0x9E3779B1u;
    return h ^ (h >> 16);
}

// p into the table of mask + 1 slots: true if this call claimed the slot, false for a repeat (or a table without a free slot)
__device__ __forceinline__ bool pos_set_insert(uint32_t* __restrict__ tab, uint32_t mask, uint32_t p) {
    for (uint32_t h = pos_set_hash(p), left = mask;; ++h, --left) {
        const uint32_t old = atomicCAS(tab + (h & mask), POS_SET_EMPTY, p);
        if (old == POS_SET_EMPTY) return true;
        if (old == p || left == 0) return false;
    }
}

// is p in the table?
__device__ __forceinline__ bool pos_set_has(const uint32_t* __restrict__ tab, uint32_t mask, uint32_t p) {
    for (uint32_t h = pos_set_hash(p), left = mask;; ++h, --left) {
        const uint32_t v = tab[h & mask];
        if (v == p) return true;
        if (v == POS_SET_EMPTY || left == 0) return false;
    }
}

}  // namespace sqe
