// block_select.h -- the one top-k primitive of the exact paths: per query, ONE workgroup finds the kth largest key by an
// MSB-first byte-wise radix select over a 256-bin LDS histogram (block_select_kth), collects the keys at or above it
// (block_collect_top), ranks them by counting and writes k places, (-inf, -1) in the unused ones (block_rank_write).
//
// Keys reach the functions through a visitor: visit(f) calls f(key) for each key of the CALLING thread; the threads of the
// block together visit every key once, in every call the same keys.  each_key<THREADS>(get, n) is the visitor of a flat
// array; ivf_select_kernel walks (probe, position) strips with one of its own.  A key of 0 is "no key" (make_key never
// gives 0: that would take row 0xFFFFFFFF).  Every thread of the block calls, from uniform control flow.
#pragma once

#include "kernels.h"

namespace sqe {

// Radix-select step: hist[256] is complete (caller synchronised) and every thread of the block (>= 256 threads) calls.
// Finds the bin that holds the `remaining`-th largest entry counting down from bin 255: bin (or -1 when the histogram
// holds fewer than `remaining` entries), what is left to find inside it and, with COUNT, how many entries the bin holds
// (a caller could not read hist[bin] itself: the next pass clears hist behind the trailing barrier).  One thread per bin
// and a suffix scan (shuffles inside a wave, four wave totals through LDS) instead of one thread walking down from bin 255.
// The results are block-uniform.
template <bool COUNT>
__device__ __forceinline__ void hist_locate(const int* hist, int remaining, int& bin, int& rem, int& count) {
    __shared__ int s_wave_total[4];
    __shared__ int s_found[COUNT ? 3 : 2];
    const int tid = threadIdx.x;
    if (tid == 0) s_found[0] = -1;
    int h = 0, incl = 0;
    if (tid < 256) {
        const int ln = tid & 63;
        h = hist[tid];
        incl = h;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_down(incl, off, 64);
            if (ln + off < 64) incl += v;
        }
        if (ln == 0) s_wave_total[tid >> 6] = incl;
    }
    __syncthreads();
    if (tid < 256) {
        int above = 0;
        for (int w = (tid >> 6) + 1; w < 4; ++w) above += s_wave_total[w];
        const int excl = above + incl - h;          // entries in the bins above this one
        if (excl < remaining && excl + h >= remaining) {
            s_found[0] = tid;
            s_found[1] = remaining - excl;
            if (COUNT) s_found[2] = h;
        }
    }
    __syncthreads();
    bin = s_found[0];
    rem = bin < 0 ? remaining : s_found[1];
    if constexpr (COUNT) count = s_found[2];
    else count = 0;
    __syncthreads();                                // the next call resets s_found
}

// visitor of a flat array: thread t sees get(t), get(t + THREADS), ... below n
template <int THREADS, typename Get>
__device__ __forceinline__ auto each_key(Get get, int n) {
    return [=](auto f) {
        for (int e = threadIdx.x; e < n; e += THREADS) f(get(e));
    };
}

// The `kth` largest of the visited keys (Key: uint32_t, four byte passes, or uint64_t, eight), to every thread; 0 when
// there are fewer than kth keys: everything qualifies.  (Only the first pass can find too few: a located bin holds at
// least what is still wanted.)  With EARLY_EXIT the pass after which the located bin holds exactly the keys still wanted
// is the last, and the low bytes of the result are 0: for UNIQUE keys, the keys >= the result are still the kth best, but
// the result is no longer a key.  hist: int[256] of LDS.
template <int THREADS, typename Key, bool EARLY_EXIT, typename Visit>
__device__ __forceinline__ Key block_select_kth(Visit visit, int kth, int* hist) {
    static_assert(THREADS >= 256, "hist_locate: one thread per histogram bin");
    constexpr int TOP = (int)sizeof(Key) - 1;
    const int tid = threadIdx.x;
    Key prefix = 0;           // determined high bytes
    int remaining = kth;
    for (int byte = TOP; byte >= 0; --byte) {
        if (THREADS == 256 || tid < 256) hist[tid] = 0;
        __syncthreads();
        const int shift = byte * 8;
        visit([&](Key key) {
            if (key == 0) return;
            const bool match = (byte == TOP) || ((key >> (shift + 8)) == (prefix >> (shift + 8)));
            if (match) atomicAdd(&hist[(int)((key >> shift) & 0xff)], 1);
        });
        __syncthreads();
        int bin, rem, count;
        hist_locate<EARLY_EXIT>(hist, remaining, bin, rem, count);      // ends with a barrier: hist may be cleared again
        if (bin < 0) return 0;                       // fewer than `remaining` keys in total
        prefix |= ((Key)bin << shift);
        remaining = rem;
        if (EARLY_EXIT && count == rem) break;
    }
    return prefix;
}

// The visited keys >= T into top[] (the first MAX_KP that arrive are kept, in no order); returns how many there are.
// At most one call per kernel and visitor type: the count lives in one LDS word that the next call would reset while threads
// still read this one's result.
template <typename Visit>
__device__ __forceinline__ int block_collect_top(Visit visit, uint64_t T, uint64_t* top) {
    __shared__ int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    visit([&](uint64_t key) {
        if (key != 0 && key >= T) {
            const int slot = atomicAdd(&s_n, 1);
            if (slot < MAX_KP) top[slot] = key;
        }
    });
    __syncthreads();
    return s_n;
}

// top[0 .. m) are unique keys, complete (caller synchronised): the key with `rank` larger ones goes to place rank < k as
// (key_score, id_of(key_row)); the places [min(m, k), k) get (-inf, -1).
template <int THREADS, typename IdOf>
__device__ __forceinline__ void block_rank_write(const uint64_t* top, int m, int k, float* cos_out, int64_t* id_out, IdOf id_of) {
    for (int i = threadIdx.x; i < m; i += THREADS) {
        const uint64_t ki = top[i];
        int rank = 0;
        for (int j = 0; j < m; ++j) rank += top[j] > ki ? 1 : 0;
        if (rank < k) {
            cos_out[rank] = key_score(ki);
            id_out[rank] = id_of(key_row(ki));
        }
    }
    for (int i = min(m, k) + threadIdx.x; i < k; i += THREADS) {
        cos_out[i] = -INFINITY;
        id_out[i] = -1;
    }
}

}  // namespace sqe
