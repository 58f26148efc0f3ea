// deny_kernels.h -- the two kernels that exclusion search (exclude.hip) and the mask route of sqe_index_search_where
// (where_mask.hip) share, templated over the test that denies a row:
//   deny_drop_kernel   stage A, one wave per query: the hits of a plain search in rank order, 64 at a time, minus the denied
//                      ones; the first k survivors to the query's output row, (-inf, -1) behind them; the query is flagged if it
//                      ends with fewer than k although the index holds more rows than were fetched.
//   deny_merge_kernel  stage B, one workgroup per slot of the sweep (sweep.hip): the keys a range collected re-scored in fp32 by
//                      rescore_row, the rows below the running k-th cosine and the denied ones dropped, the rest merged with
//                      the running list by block_select.h's select; the thresholds of the next range written on the device.
// A denial policy D is a trivially copyable struct that travels in the kernel arguments:
//   D::DENSE                      stage A's slot j is query j of the pass (else the class table cls names it)
//   D::Probe D::of(int q) const   what query q of the pass tests its rows with (wave-uniform)
//   bool Probe::denied(uint32_t p) const    row position p is not to be returned
// DenyTable: the query's deny-list as a position set (id_lists.h), no list denying nothing.  DenyBitmap: bit p of one map of the
// filtered search's layout (u32 words, bit p & 31 of word p >> 5) is clear.  DenyNone: nothing is denied; it instantiates the paths
// that take no restriction (range.hip, collapse.hip): same argument layout, registers and LDS as before the policy, the same
// instructions up to the compiler's scheduling (profiles/within/NOTES.md).
#pragma once

#include <math.h>

#include "block_select.h"
#include "id_lists.h"
#include "kernels.h"

namespace sqe {

constexpr int DENY_CAP = EXACT_CAP;            // keys per slot and collect launch: the collect scan's buffer stride
constexpr int DENY_MERGE_THREADS = 256;

// one deny-list on the device: its entries [entry_off, entry_off + len) of the id array, its table at tab_off
struct ExList {
    int64_t entry_off, tab_off;
    uint32_t tab_mask;
};

struct DenyTable {
    static constexpr bool DENSE = false;
    const int32_t* loq;        // [pass] list of the query, -1: none
    const ExList* lists;
    const uint32_t* tab;
    struct Probe {
        const uint32_t* tab;
        uint32_t mask;
        __device__ __forceinline__ bool denied(uint32_t p) const { return tab && pos_set_has(tab, mask, p); }
    };
    __device__ __forceinline__ Probe of(int q) const {
        const int f = loq[q];
        Probe pr{nullptr, 0};
        if (f >= 0) {
            pr.tab = tab + lists[f].tab_off;
            pr.mask = lists[f].tab_mask;
        }
        return pr;
    }
};

struct DenyBitmap {
    static constexpr bool DENSE = true;
    const uint32_t* bits;      // one map for every query of the call; the hits and keys name live rows only, so p lies inside the map
    struct Probe {
        const uint32_t* bits;
        __device__ __forceinline__ bool denied(uint32_t p) const { return ((bits[p >> 5] >> (p & 31)) & 1u) == 0; }
    };
    __device__ __forceinline__ Probe of(int) const { return Probe{bits}; }
};

struct DenyNone {
    static constexpr bool DENSE = true;
    struct Probe {
        __device__ __forceinline__ bool denied(uint32_t) const { return false; }
    };
    __device__ __forceinline__ Probe of(int) const { return Probe{}; }
};

template <typename D>
struct DropArgs {
    const float* hit_cos;      // [nq, kd] best first
    const int64_t* hit_pos;    // [nq, kd] positions + id_sub, ended by -1
    int kd, k;
    const int* cls;            // class slot -> query of the pass (unused by a DENSE policy)
    D deny;
    int64_t id_sub, n_rows;
    float* cos_out;            // [pass, k]
    int64_t* pos_out;
    int* flags;                // [pass]; null: nothing is flagged
};

template <typename D>
__global__ __launch_bounds__(64) void deny_drop_kernel(DropArgs<D> a) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const int q = D::DENSE ? j : a.cls[j];
    const typename D::Probe probe = a.deny.of(q);
    const float* c = a.hit_cos + (size_t)j * a.kd;
    const int64_t* d = a.hit_pos + (size_t)j * a.kd;
    float* co = a.cos_out + (size_t)q * a.k;
    int64_t* po = a.pos_out + (size_t)q * a.k;
    int found = 0;
    for (int base = 0; base < a.kd && found < a.k; base += 64) {
        const int e = base + lane;
        bool keep = false;
        int64_t p = -1;
        if (e < a.kd) {
            const int64_t id = d[e];
            if (id >= 0) {
                p = id - a.id_sub;
                keep = !probe.denied((uint32_t)p);
            }
        }
        const unsigned long long m = __ballot(keep);
        const int slot = found + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && slot < a.k) {
            co[slot] = c[e];
            po[slot] = p;
        }
        found += __popcll(m);
    }
    found = min(found, a.k);
    for (int s = found + lane; s < a.k; s += 64) {
        co[s] = -INFINITY;
        po[s] = -1;
    }
    if (a.flags && lane == 0) a.flags[q] = (found < a.k && (int64_t)a.kd < a.n_rows) ? 1 : 0;
}

template <typename D>
struct MergeArgs {
    const float* master;       // [n, K] fp32 rows
    const float* qn;           // [pass] normalised queries
    int K;
    const int* qidx;           // slot -> query of the pass
    const uint64_t* keys;      // [G, DENY_CAP] collected keys, rows relative to row_off
    const int* key_cnt;        // [G], none above DENY_CAP (the host checked)
    int64_t row_off;
    int k;
    D deny;
    const float* q_resid;      // [pass]
    const uint32_t* resid_max;
    float* thr;                // [G] collect threshold of the next range
    float* kth;                // [G]
    int* lcnt;                 // [G]
    float* cos_out;            // [pass, k] running lists, best first
    int64_t* pos_out;
};

// One workgroup per slot: the running list and the undenied re-scored rows of the range that reach its k-th cosine, as rank
// keys in LDS; the best k of them (radix select, rank by counting) are the new running list.
template <typename D>
__global__ __launch_bounds__(DENY_MERGE_THREADS) void deny_merge_kernel(MergeArgs<D> a) {
    __shared__ uint64_t rk[DENY_CAP + MAX_KP];
    __shared__ uint64_t top[MAX_KP];
    __shared__ int hist[256];
    __shared__ int s_new;
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.key_cnt[i];
    const int q = a.qidx[i];
    const float t = a.kth[i];
    const int nr = a.lcnt[i];
    const typename D::Probe probe = a.deny.of(q);
    float* co = a.cos_out + (size_t)q * a.k;
    int64_t* po = a.pos_out + (size_t)q * a.k;
    if (tid == 0) s_new = 0;
    for (int j = tid; j < nr; j += DENY_MERGE_THREADS) rk[j] = make_key(co[j], (uint32_t)po[j]);
    __syncthreads();
    // fp32 re-score, one wave per row; a row below the k-th cosine of the running list cannot enter it
    const float4* qv = reinterpret_cast<const float4*>(a.qn + (size_t)q * a.K);
    const int nvec = a.K >> 2;
    const uint64_t* keys = a.keys + (size_t)i * DENY_CAP;
    for (int e = wave; e < n; e += DENY_MERGE_THREADS / 64) {
        const int64_t row = a.row_off + key_row(keys[e]);
        const float4* rv = reinterpret_cast<const float4*>(a.master + (size_t)row * a.K);
        const float s = rescore_row(rv, qv, nvec, lane);
        if (lane == 0 && s >= t && !probe.denied((uint32_t)row)) rk[nr + atomicAdd(&s_new, 1)] = make_key(s, (uint32_t)row);
    }
    __syncthreads();
    if (s_new == 0) return;                     // nothing new: list and thresholds stand
    const int T = nr + s_new;
    auto visit = each_key<DENY_MERGE_THREADS>([&](int e) { return rk[e]; }, T);
    const uint64_t Tk = T > a.k ? block_select_kth<DENY_MERGE_THREADS, uint64_t, false>(visit, a.k, hist) : 0ull;
    const int m = min(block_collect_top(visit, Tk, top), a.k);      // the keys are unique: exactly k reach Tk
    block_rank_write<DENY_MERGE_THREADS>(top, m, a.k, co, po, [](uint32_t row) { return (int64_t)row; });
    if (tid == 0) {
        a.lcnt[i] = m;
        if (m >= a.k) {
            uint64_t low = top[0];
            for (int j = 1; j < m; ++j) low = top[j] < low ? top[j] : low;
            const float kc = key_score(low);
            a.kth[i] = kc;
            a.thr[i] = nextafterf(kc - scan_eps(a.q_resid[q], __uint_as_float(*a.resid_max), a.K), -INFINITY);
        }
    }
}

}  // namespace sqe
