// aggregate.hip -- aggregations over the numeric fields (sqe_index_aggregate_fields): stats, terms and histogram facets of the
// rows a field predicate (and an optional allow-list) selects, without an id or a value leaving the device.
//
// The row set is the bitmap of sqe_index_search_where (rowset.hip: rowset_map); the kernels here read it.
//   1. agg_stats_kernel: one grid-stride pass over the 64-row units, one row per lane.  A lane reads its bit and its value in every
//      column the call names (a column named by several aggregations is read once) and keeps count, min, max and the two partial
//      sums per column; wave shuffles, then LDS, give one partial per block and agg_fold_kernel (one block) folds them.  The host
//      reads the folded stats and the selected count back: the one synchronisation that plans the routes.
//   2. counting.  Dense route (TERMS over a span of at most 16,384 values, every HISTOGRAM): agg_dense_kernel keeps a private LDS
//      table of u32 counters per workgroup, bumps it with LDS atomics and adds its non-zero counters into the global table of the
//      span.  Hash route (every other TERMS): agg_hash_kernel inserts into an open-addressing table in HBM (64-bit CAS on the key,
//      linear probing, atomicAdd on the count; capacity a power of two >= 2 x count, so the load stays <= 0.5).
//   3. select, shared by both routes: the table is an array of (value, count) slots; agg_select_kernel picks the best `size` of
//      each block of 16,384 slots by (count desc, value asc) with the block radix select (block_select.h) and counts the occupied
//      slots, agg_merge_kernel (one block) picks among the blocks' candidates, ranks them and writes the buckets, n_buckets and
//      other.  A HISTOGRAM skips the select: agg_hist_write_kernel writes its counters out in bucket order.
// Device groups (group.hip: group_index_aggregate_fields): index_aggregate_shard runs steps 1 and 2 on a shard and brings ALL of
// its buckets to the host -- a histogram's counters, a TERMS table's occupied slots through agg_compact_kernel (at most 65,536) --
// where the leader merges exactly.
// Integers only: no result depends on the order in which rows, waves or blocks arrive.
#include <string.h>

#include <algorithm>
#include <vector>

#include "block_select.h"
#include "fieldpred.h"
#include "internal.h"

namespace sqe {

namespace {

constexpr int AGG_MAX = 8;                     // aggregations of one call
constexpr int AGG_DENSE_SPAN = 16384;          // counters of the dense route's LDS table (64 KiB), the histogram's bucket limit
constexpr int AGG_SELECT_BLOCK = 16384;        // slots one select workgroup ranks
constexpr int AGG_MAX_SIZE = 256;              // buckets a TERMS aggregation returns at most (MAX_KP)
constexpr int AGG_STATS_BLOCKS = 1024;         // workgroups of the stats and hash passes (they stride over the units): 16 waves per CU
constexpr int AGG_DENSE_BLOCKS = 512;          // workgroups of the dense pass: each one flushes a table of the span at its end
constexpr int STAT_WORDS = 5;                  // count, min, max, sum_lo, sum_hi
constexpr int PART_WORDS = 1 + FIELD_MAX * STAT_WORDS;      // selected rows, then the stats of up to 8 columns
static_assert(AGG_MAX_SIZE <= MAX_KP, "the block select keeps at most MAX_KP keys");

// how word i of a partial joins: 0 sum, 1 min, 2 max
__host__ __device__ constexpr int stat_op(int i) { return i == 0 ? 0 : ((i - 1) % STAT_WORDS == 1 ? 1 : ((i - 1) % STAT_WORDS == 2 ? 2 : 0)); }
__host__ __device__ constexpr int64_t stat_identity(int op) { return op == 0 ? 0 : (op == 1 ? INT64_MAX : FIELD_NONE); }
__device__ __forceinline__ int64_t stat_join(int op, int64_t a, int64_t b) { return op == 0 ? a + b : (op == 1 ? (a < b ? a : b) : (a > b ? a : b)); }

// the first n_words of acc of every thread of the block (256) -> out[i * stride]; red: LDS [4][PART_WORDS]
__device__ __forceinline__ void block_fold_store(int64_t (&acc)[PART_WORDS], int n_words, int64_t (*red)[PART_WORDS], int64_t* out, int stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < PART_WORDS; ++i) {
        if (i >= n_words) continue;            // block-uniform: the words of columns the call does not name are not reduced
        int64_t v = acc[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = stat_join(stat_op(i), v, __shfl_xor(v, off, 64));
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < n_words) {
        const int i = threadIdx.x, op = stat_op(i);
        out[(int64_t)i * stride] = stat_join(op, stat_join(op, red[0][i], red[1][i]), stat_join(op, red[2][i], red[3][i]));
    }
}

struct AggStatsArgs {
    const uint64_t* bits;                      // the row set: bit (p & 63) of word p >> 6
    int64_t units;                             // 64-row units of the map
    const int64_t* col[FIELD_MAX];             // the n_cols distinct columns the call names
    int n_cols;
    int64_t* part;                             // [PART_WORDS, AGG_STATS_BLOCKS]: word i of block b at i * AGG_STATS_BLOCKS + b
};

__global__ __launch_bounds__(256) void agg_stats_kernel(AggStatsArgs a) {
    __shared__ int64_t red[4][PART_WORDS];
    const int lane = threadIdx.x & 63;
    int64_t acc[PART_WORDS];
#pragma unroll
    for (int i = 0; i < PART_WORDS; ++i) acc[i] = stat_identity(stat_op(i));
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < a.units; u += (int64_t)gridDim.x * 4) {
        const uint64_t w = a.bits[u];
        if (w == 0) continue;                  // wave-uniform: no row of the unit is selected, no column is read
        const bool on = (w >> lane) & 1;       // a set bit is a live row: p < n, inside every column
        const int64_t p = u * 64 + lane;
        acc[0] += on ? 1 : 0;
#pragma unroll
        for (int c = 0; c < FIELD_MAX; ++c) {
            if (c >= a.n_cols) continue;
            const int64_t v = on ? a.col[c][p] : FIELD_NONE;      // the one read of this column for this row
            if (v == FIELD_NONE) continue;
            constexpr int W = STAT_WORDS;
            acc[1 + c * W] += 1;
            acc[2 + c * W] = v < acc[2 + c * W] ? v : acc[2 + c * W];
            acc[3 + c * W] = v > acc[3 + c * W] ? v : acc[3 + c * W];
            acc[4 + c * W] += (int64_t)(uint32_t)v;      // the low word, unsigned
            acc[5 + c * W] += v >> 32;                   // the high word, arithmetic
        }
    }
    block_fold_store(acc, 1 + a.n_cols * STAT_WORDS, red, a.part + blockIdx.x, AGG_STATS_BLOCKS);
}

// one block: the first n_words words of n_parts partials (word-major, so consecutive threads read consecutive blocks) -> out
__global__ __launch_bounds__(256) void agg_fold_kernel(const int64_t* __restrict__ part, int n_parts, int n_words, int64_t* __restrict__ out) {
    __shared__ int64_t red[4][PART_WORDS];
    int64_t acc[PART_WORDS];
#pragma unroll
    for (int i = 0; i < PART_WORDS; ++i) acc[i] = stat_identity(stat_op(i));
    for (int b = threadIdx.x; b < n_parts; b += 256) {
#pragma unroll
        for (int i = 0; i < PART_WORDS; ++i)
            if (i < n_words) acc[i] = stat_join(stat_op(i), acc[i], part[(int64_t)i * AGG_STATS_BLOCKS + b]);
    }
    block_fold_store(acc, n_words, red, out, 1);
}

enum { SLOTS_HASH = 0, SLOTS_TERMS = 1, SLOTS_HISTOGRAM = 2 };

// the table of a call, cleared: every count 0; keys SQE_FIELD_NONE (hash), base + i (dense terms) or bucket base + i's key (histogram)
__global__ __launch_bounds__(256) void agg_slots_init_kernel(int64_t* __restrict__ keys, uint32_t* __restrict__ counts, int64_t slots, int mode,
                                                             int64_t base, int64_t interval, int64_t offset) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= slots) return;
    counts[i] = 0;
    keys[i] = mode == SLOTS_HASH ? FIELD_NONE : (mode == SLOTS_TERMS ? base + i : agg_bucket_key(base + i, interval, offset));
}

struct AggCountArgs {
    const uint64_t* bits;
    int64_t units;
    const int64_t* col;
    int64_t base;                              // dense: the value (TERMS) or bucket (HISTOGRAM) of counter 0
    int64_t interval, offset;                  // HISTOGRAM (interval 0: TERMS)
    int span;                                  // dense: counters
    uint64_t mask;                             // hash: capacity - 1
    int64_t* keys;                             // hash
    uint32_t* counts;
};

__global__ __launch_bounds__(256) void agg_dense_kernel(AggCountArgs a) {
    extern __shared__ __align__(16) uint32_t tab[];        // [span] private counters
    for (int i = threadIdx.x; i < a.span; i += 256) tab[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < a.units; u += (int64_t)gridDim.x * 4) {
        const uint64_t w = a.bits[u];
        if (w == 0) continue;
        const int64_t v = ((w >> lane) & 1) ? a.col[u * 64 + lane] : FIELD_NONE;
        if (v == FIELD_NONE) continue;
        const int64_t i = (a.interval ? agg_bucket(v, a.interval, a.offset) : v) - a.base;
        if ((uint64_t)i < (uint64_t)a.span) atomicAdd(&tab[i], 1u);       // always true: base and span come from this row set's min and max
    }
    __syncthreads();
    for (int i = threadIdx.x; i < a.span; i += 256) {
        const uint32_t c = tab[i];
        if (c) atomicAdd(a.counts + i, c);
    }
}

// murmur3's 64-bit finaliser: every input bit reaches every output bit
__device__ __forceinline__ uint64_t agg_mix(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// `add` more rows of value v into the global table (hashed h = agg_mix(v))
__device__ __forceinline__ void hash_insert(const AggCountArgs& a, int64_t v, uint64_t hashed, uint32_t add) {
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(a.keys);
    uint64_t h = hashed & a.mask;
    // the load is at most half, so an empty slot ends every probe sequence; the bound only keeps a broken table from spinning
    for (uint64_t probe = 0; probe <= a.mask; ++probe, h = (h + 1) & a.mask) {
        int64_t k = (int64_t)__hip_atomic_load(keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == FIELD_NONE) k = (int64_t)atomicCAS(keys + h, (unsigned long long)FIELD_NONE, (unsigned long long)v);
        if (k == FIELD_NONE || k == v) {           // the slot was empty and is ours now, or held v already (a key never changes once set)
            atomicAdd(a.counts + h, add);
            return;
        }
    }
}

// A workgroup counts in front of the global table, in a direct-mapped LDS table of 2,048 (value, count) places addressed by the
// hash's top bits: the first value to claim a place owns it for the workgroup, every other value of that place goes to the
// global table at once, and the places are added into the global table at the end.  A value that many rows hold claims its place
// early, so its rows cost LDS atomics and one global add per workgroup instead of one global atomic each on ONE address
// (profiles/aggregate/NOTES.md: 0.40 ms against 29.6 ms for 10 M rows of a skewed column).  Every row is still counted exactly once.
constexpr int HASH_FRONT = 2048;
__global__ __launch_bounds__(256) void agg_hash_kernel(AggCountArgs a) {
    __shared__ unsigned long long front_k[HASH_FRONT];
    __shared__ uint32_t front_c[HASH_FRONT];
    for (int i = threadIdx.x; i < HASH_FRONT; i += 256) {
        front_k[i] = (unsigned long long)FIELD_NONE;
        front_c[i] = 0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < a.units; u += (int64_t)gridDim.x * 4) {
        const uint64_t w = a.bits[u];
        if (w == 0) continue;
        const int64_t v = ((w >> lane) & 1) ? a.col[u * 64 + lane] : FIELD_NONE;
        if (v == FIELD_NONE) continue;
        const uint64_t hashed = agg_mix((uint64_t)v);
        const int place = (int)(hashed >> 53);     // 11 bits the global table's index (the low bits) does not use below 2^53 slots
        int64_t k = (int64_t)__hip_atomic_load(front_k + place, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == FIELD_NONE) k = (int64_t)atomicCAS(front_k + place, (unsigned long long)FIELD_NONE, (unsigned long long)v);
        if (k == FIELD_NONE || k == v) atomicAdd(front_c + place, 1u);
        else hash_insert(a, v, hashed, 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < HASH_FRONT; i += 256) {
        const uint32_t c = front_c[i];
        if (c) hash_insert(a, (int64_t)front_k[i], agg_mix(front_k[i]), c);
    }
}

// falls as v rises and is never 0 (v is never SQE_FIELD_NONE): the u64 key of "lower value first" for the block select
__device__ __forceinline__ uint64_t value_key(int64_t v) { return 0 - ((uint64_t)v ^ 0x8000000000000000ull); }

// The best `size` of the slots [0, n) by (count desc, value asc), slots of count 0 being empty: out_k / out_c [size] get them in no
// order, the unused places (SQE_FIELD_NONE, 0).  Returns the occupied slots.  Every thread of the block (256) calls, from uniform
// control flow; at most one call per kernel.
__device__ __forceinline__ int select_best(const int64_t* keys, const uint32_t* counts, int n, int size, int64_t* out_k, uint32_t* out_c) {
    __shared__ int hist[256];
    __shared__ int s_above, s_occ, s_m;
    if (threadIdx.x == 0) s_above = s_occ = s_m = 0;       // the select's barriers order this before the first use
    // the size-th largest count; 0: fewer than `size` slots are occupied and all of them go out
    const uint32_t T = block_select_kth<256, uint32_t, false>(each_key<256>([&](int e) { return counts[e]; }, n), size, hist);
    int above = 0, occ = 0;
    for (int e = threadIdx.x; e < n; e += 256) {
        const uint32_t c = counts[e];
        above += c > T ? 1 : 0;
        occ += c > 0 ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) {
        above += __shfl_xor(above, off, 64);
        occ += __shfl_xor(occ, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_above, above);
        atomicAdd(&s_occ, occ);
    }
    __syncthreads();
    // among the slots AT the size-th count the lowest values fill what is left: values are distinct, so the cut is exact
    uint64_t T2 = 0;
    if (T > 0)
        T2 = block_select_kth<256, uint64_t, false>(each_key<256>([&](int e) { return counts[e] == T ? value_key(keys[e]) : 0ull; }, n),
                                                    size - s_above, hist);
    for (int e = threadIdx.x; e < n; e += 256) {
        const uint32_t c = counts[e];
        if (c > T || (T > 0 && c == T && value_key(keys[e]) >= T2)) {
            const int slot = atomicAdd(&s_m, 1);
            if (slot < size) {
                out_k[slot] = keys[e];
                out_c[slot] = c;
            }
        }
    }
    __syncthreads();
    for (int i = min(s_m, size) + threadIdx.x; i < size; i += 256) {
        out_k[i] = FIELD_NONE;
        out_c[i] = 0;
    }
    return s_occ;
}

// block b: the best `size` of slots [b * 16384, ...) -> cand_k / cand_c [b, size], occ[b] = its occupied slots
__global__ __launch_bounds__(256) void agg_select_kernel(const int64_t* __restrict__ keys, const uint32_t* __restrict__ counts, int64_t slots,
                                                         int size, int64_t* __restrict__ cand_k, uint32_t* __restrict__ cand_c,
                                                         int* __restrict__ occ) {
    const int64_t first = (int64_t)blockIdx.x * AGG_SELECT_BLOCK;
    const int n = slots - first < AGG_SELECT_BLOCK ? (int)(slots - first) : AGG_SELECT_BLOCK;
    const int o = select_best(keys + first, counts + first, n, size, cand_k + (int64_t)blockIdx.x * size, cand_c + (int64_t)blockIdx.x * size);
    if (threadIdx.x == 0) occ[blockIdx.x] = o;
}

// one block: the best `size` of the blocks' candidates, ranked, to key_out / count_out [size] (padded); tail[0] = the distinct
// values (the blocks' occupied slots), tail[1] = count - the returned counts, tail[2] = the blocks that hold an occupied slot
__global__ __launch_bounds__(256) void agg_merge_kernel(const int64_t* __restrict__ cand_k, const uint32_t* __restrict__ cand_c,
                                                        const int* __restrict__ occ, int n_blocks, int size, int64_t count,
                                                        int64_t* __restrict__ key_out, int64_t* __restrict__ count_out,
                                                        int64_t* __restrict__ tail) {
    __shared__ int64_t top_k[AGG_MAX_SIZE];
    __shared__ uint32_t top_c[AGG_MAX_SIZE];
    __shared__ unsigned long long s_distinct, s_returned;
    __shared__ int s_blocks;
    if (threadIdx.x == 0) {
        s_distinct = s_returned = 0;
        s_blocks = 0;
    }
    const int m = min(select_best(cand_k, cand_c, n_blocks * size, size, top_k, top_c), size);      // every occupied candidate is a bucket
    __syncthreads();
    unsigned long long d = 0;
    int nonempty = 0;
    for (int b = threadIdx.x; b < n_blocks; b += 256) {
        d += (unsigned long long)occ[b];
        nonempty += occ[b] > 0 ? 1 : 0;
    }
    if (d) {
        atomicAdd(&s_distinct, d);
        atomicAdd(&s_blocks, nonempty);
    }
    for (int i = threadIdx.x; i < size; i += 256) {
        if (i < m) {
            const int64_t ki = top_k[i];
            const uint32_t ci = top_c[i];
            int rank = 0;
            for (int j = 0; j < m; ++j) rank += (top_c[j] > ci || (top_c[j] == ci && top_k[j] < ki)) ? 1 : 0;
            key_out[rank] = ki;
            count_out[rank] = (int64_t)ci;
            atomicAdd(&s_returned, (unsigned long long)ci);
        } else {
            key_out[i] = FIELD_NONE;
            count_out[i] = 0;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        tail[0] = (int64_t)s_distinct;
        tail[1] = count - (int64_t)s_returned;
        tail[2] = s_blocks;
    }
}

// a histogram's counters out in bucket order
__global__ __launch_bounds__(256) void agg_hist_write_kernel(const int64_t* __restrict__ keys, const uint32_t* __restrict__ counts, int nb,
                                                             int64_t* __restrict__ key_out, int64_t* __restrict__ count_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    key_out[i] = keys[i];
    count_out[i] = (int64_t)counts[i];
}

// the occupied slots of a table, in no order, to out_k / out_c [cap]; *n counts them all, the ones past cap included
__global__ __launch_bounds__(256) void agg_compact_kernel(const int64_t* __restrict__ keys, const uint32_t* __restrict__ counts, int64_t slots,
                                                          int cap, int64_t* __restrict__ out_k, uint32_t* __restrict__ out_c, int* __restrict__ n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= slots) return;
    const uint32_t c = counts[i];
    if (c == 0) return;
    const int j = atomicAdd(n, 1);
    if (j < cap) {
        out_k[j] = keys[i];
        out_c[j] = c;
    }
}

__global__ __launch_bounds__(256) void agg_pad_kernel(int64_t* __restrict__ key_out, int64_t* __restrict__ count_out, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    key_out[i] = FIELD_NONE;
    count_out[i] = 0;
}

}  // namespace

struct AggState {
    DevBuf part;                   // i64 [PART_WORDS, AGG_STATS_BLOCKS] the blocks' partials, word-major, then [PART_WORDS] the folded stats
    DevBuf keys, counts;           // the table of one aggregation: i64 [slots], u32 [slots]
    DevBuf cand_k, cand_c, occ;    // the select blocks' candidates [blocks, size] and occupied slots [blocks]
    DevBuf out;                    // keys i64 [n_aggs, dcap] | counts i64 [n_aggs, dcap] | tail i64 [n_aggs, 3]
    sqe_agg_last_t last{};         // the routes of the last call (sqe_index_aggregate_last)
    bool has_last = false;
};

void aggregate_destroy(AggState* a) { delete a; }

namespace {

struct Stats { int64_t count = 0, min = INT64_MAX, max = FIELD_NONE, sum_lo = 0, sum_hi = 0; };

struct AggCall {
    const RowSet& set;             // a host list, if any
    const sqe_field_agg_t* aggs;
    int n_aggs;
    int64_t bucket_cap;
    int64_t* selected_out;
    sqe_field_agg_result_t* result_out;
    int64_t* key_out;
    int64_t* count_out;
    AggShardResult* shard;         // a shard of a device group: stats and ALL buckets go here, the four outputs above are unused
};

void write_stats(sqe_field_agg_result_t& r, const Stats& st) {
    r.count = st.count; r.min = st.min; r.max = st.max; r.sum_lo = st.sum_lo; r.sum_hi = st.sum_hi;
    r.n_buckets = 0; r.other = 0;
}

void pad_buckets(const AggCall& c, int j, int64_t from) {
    for (int64_t i = from; i < c.bucket_cap; ++i) {
        c.key_out[(int64_t)j * c.bucket_cap + i] = FIELD_NONE;
        c.count_out[(int64_t)j * c.bucket_cap + i] = 0;
    }
}

// A shard of a device group: every bucket of the table just counted to the host.  A histogram's counters in bucket order (the
// leader places them by a.base); of a TERMS table the occupied slots, compacted in no order, at most AGG_GROUP_MAX_DISTINCT.
int shard_buckets(AggState* st, const sqe_field_agg_t& g, int64_t slots, AggShardAgg& a, hipStream_t s) {
    const int64_t* keys = st->keys.as<int64_t>();
    const uint32_t* counts = st->counts.as<uint32_t>();
    int64_t m = slots;
    if (g.kind == SQE_AGG_TERMS) {
        SQE_TRY(st->cand_k.ensure((size_t)AGG_GROUP_MAX_DISTINCT * 8));
        SQE_TRY(st->cand_c.ensure((size_t)AGG_GROUP_MAX_DISTINCT * 4));
        SQE_TRY(st->occ.ensure(16));
        SQE_HIP(hipMemsetAsync(st->occ.p, 0, 4, s));
        hipLaunchKernelGGL(agg_compact_kernel, dim3(grid_of(slots, 256)), dim3(256), 0, s, keys, counts, slots, (int)AGG_GROUP_MAX_DISTINCT,
                           st->cand_k.as<int64_t>(), st->cand_c.as<uint32_t>(), st->occ.as<int>());
        SQE_HIP(hipGetLastError());
        int distinct = 0;
        SQE_HIP(hipMemcpyAsync(&distinct, st->occ.p, 4, hipMemcpyDeviceToHost, s));
        SQE_HIP(hipStreamSynchronize(s));
        if (distinct > AGG_GROUP_MAX_DISTINCT)
            return fail(SQE_ERR_UNSUPPORTED, "sqe_index_aggregate_fields: a shard of the device group holds " + std::to_string(distinct) +
                                                 " distinct values of a TERMS field (at most 65536 per shard on a group)");
        keys = st->cand_k.as<int64_t>();
        counts = st->cand_c.as<uint32_t>();
        m = distinct;
    }
    std::vector<uint32_t> c32((size_t)m);
    a.keys.resize((size_t)m);
    a.counts.resize((size_t)m);
    if (m > 0) {
        SQE_HIP(hipMemcpyAsync(a.keys.data(), keys, (size_t)m * 8, hipMemcpyDeviceToHost, s));
        SQE_HIP(hipMemcpyAsync(c32.data(), counts, (size_t)m * 4, hipMemcpyDeviceToHost, s));
        SQE_HIP(hipStreamSynchronize(s));
    }
    for (int64_t i = 0; i < m; ++i) a.counts[(size_t)i] = (int64_t)c32[(size_t)i];
    return SQE_OK;
}

int aggregate_impl(sqe_index* idx, AggState* st, const AggCall& c, hipStream_t s) {
    const int64_t n = idx->n.load();
    sqe_agg_last_t last{};
    last.n_aggs = c.n_aggs;
    if (c.shard) *c.shard = AggShardResult{};
    if ((n == 0 || c.set.n_allow == 0) && c.shard) return SQE_OK;
    if (n == 0 || c.set.n_allow == 0) {
        *c.selected_out = 0;
        for (int j = 0; j < c.n_aggs; ++j) {
            write_stats(c.result_out[j], Stats{});
            pad_buckets(c, j, 0);
        }
        st->last = last;
        st->has_last = true;
        return SQE_OK;
    }
    // ---- the row set's map (rowset_map); its positions are not wanted
    FilterState* f;
    int64_t words;
    SQE_TRY(rowset_map(idx, c.set, &f, &words, s));
    const uint64_t* bits = reinterpret_cast<const uint64_t*>(filter_bitmap(f));
    const int64_t units = words / 2;
    // ---- the stats of every column the call names, each read once
    int col_of_slot[FIELD_MAX];
    AggStatsArgs sa{};
    sa.bits = bits;
    sa.units = units;
    for (int fslot = 0; fslot < FIELD_MAX; ++fslot) col_of_slot[fslot] = -1;
    for (int j = 0; j < c.n_aggs; ++j) {
        const int fslot = c.aggs[j].field;
        const int64_t* col = fields_column(idx, fslot);
        if (col && col_of_slot[fslot] < 0) {
            col_of_slot[fslot] = sa.n_cols;
            sa.col[sa.n_cols++] = col;
        }
    }
    const int grid = (int)std::min<int64_t>(AGG_STATS_BLOCKS, (units + 3) / 4);
    SQE_TRY(st->part.ensure((size_t)(AGG_STATS_BLOCKS + 1) * PART_WORDS * 8));
    sa.part = st->part.as<int64_t>();
    int64_t* folded = sa.part + (int64_t)AGG_STATS_BLOCKS * PART_WORDS;
    const int n_words = 1 + sa.n_cols * STAT_WORDS;
    int64_t host_stats[PART_WORDS];
    {
        StageTimer t(idx->ctx->prof, s, ST_SCAN);
        hipLaunchKernelGGL(agg_stats_kernel, dim3(grid), dim3(256), 0, s, sa);
        hipLaunchKernelGGL(agg_fold_kernel, dim3(1), dim3(256), 0, s, sa.part, grid, n_words, folded);
        SQE_HIP(hipGetLastError());
    }
    SQE_HIP(hipMemcpyAsync(host_stats, folded, (size_t)n_words * 8, hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));            // the one read-back: the stats choose every route (and the allow-list may go)
    // ---- plan
    struct Plan { int route = SQE_AGG_ROUTE_NONE, mode = 0; int64_t base = 0, slots = 0, span = 0, nb = 0; };
    Plan plan[AGG_MAX];
    Stats stats[AGG_MAX];
    const int64_t dcap = c.shard ? AGG_DENSE_SPAN : std::min<int64_t>(c.bucket_cap, AGG_DENSE_SPAN);
    std::string too_many;
    for (int j = 0; j < c.n_aggs; ++j) {
        const sqe_field_agg_t& g = c.aggs[j];
        const int ci = col_of_slot[g.field];
        if (ci >= 0) {
            const int64_t* h = host_stats + 1 + ci * STAT_WORDS;
            stats[j] = Stats{h[0], h[1], h[2], h[3], h[4]};
        }
        Plan& p = plan[j];
        if (g.kind == SQE_AGG_STATS || stats[j].count == 0) continue;
        if (g.kind == SQE_AGG_HISTOGRAM) {
            const int64_t kmin = agg_bucket(stats[j].min, g.interval, g.offset), kmax = agg_bucket(stats[j].max, g.interval, g.offset);
            const uint64_t nb1 = (uint64_t)kmax - (uint64_t)kmin;         // n_buckets - 1: exact, kmax >= kmin
            p.nb = nb1 >= (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)nb1 + 1;
            if (p.nb > dcap) {
                if (c.shard) c.shard->agg[j].skipped = true;      // the group's histogram is at least as wide: the leader refuses
                else if (too_many.empty())
                    too_many = "sqe_index_aggregate_fields: too_many_buckets: the histogram of aggregation " + std::to_string(j) + " has " +
                               std::to_string(nb1 + 1) + " buckets (at most min(bucket_cap, 16384) = " + std::to_string(dcap) + ")";
                continue;
            }
            p.route = SQE_AGG_ROUTE_DENSE; p.mode = SLOTS_HISTOGRAM; p.base = kmin; p.slots = p.span = p.nb;
        } else {
            const uint64_t span1 = (uint64_t)stats[j].max - (uint64_t)stats[j].min;      // span - 1
            p.span = span1 >= (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)span1 + 1;
            if (p.span <= AGG_DENSE_SPAN) {
                p.route = SQE_AGG_ROUTE_DENSE; p.mode = SLOTS_TERMS; p.base = stats[j].min; p.slots = p.span;
            } else {
                p.route = SQE_AGG_ROUTE_HASH; p.mode = SLOTS_HASH; p.slots = 1024;
                while (p.slots < 2 * stats[j].count) p.slots <<= 1;
            }
        }
    }
    if (c.shard) {
        c.shard->selected = host_stats[0];
        for (int j = 0; j < c.n_aggs; ++j) {
            AggShardAgg& a = c.shard->agg[j];
            a.count = stats[j].count; a.min = stats[j].min; a.max = stats[j].max; a.sum_lo = stats[j].sum_lo; a.sum_hi = stats[j].sum_hi;
            a.base = plan[j].base;
        }
    } else {
        *c.selected_out = host_stats[0];
        for (int j = 0; j < c.n_aggs; ++j) {
            write_stats(c.result_out[j], stats[j]);
            if (c.aggs[j].kind == SQE_AGG_HISTOGRAM) c.result_out[j].n_buckets = plan[j].nb;
        }
    }
    if (!too_many.empty()) return fail(SQE_ERR_INVALID, too_many);
    // ---- count and select, one aggregation after the other through the same table
    const size_t kb = (size_t)c.n_aggs * dcap * 8;
    SQE_TRY(st->out.ensure(2 * kb + (size_t)c.n_aggs * 24 + 16));
    int64_t* key_dev = st->out.as<int64_t>();
    int64_t* count_dev = key_dev + (size_t)c.n_aggs * dcap;
    int64_t* tail_dev = count_dev + (size_t)c.n_aggs * dcap;
    bool any = false;
    for (int j = 0; j < c.n_aggs; ++j) any |= plan[j].route != SQE_AGG_ROUTE_NONE;
    if (any && !c.shard) {
        hipLaunchKernelGGL(agg_pad_kernel, dim3(grid_of((int64_t)c.n_aggs * dcap, 256)), dim3(256), 0, s, key_dev, count_dev,
                           (int64_t)c.n_aggs * dcap);
        SQE_HIP(hipMemsetAsync(tail_dev, 0, (size_t)c.n_aggs * 24, s));
    }
    for (int j = 0; j < c.n_aggs; ++j) {
        const sqe_field_agg_t& g = c.aggs[j];
        Plan& p = plan[j];
        last.agg[j].route = p.route;
        last.agg[j].span = p.span;
        last.agg[j].slots = p.slots;
        if (p.route == SQE_AGG_ROUTE_NONE) continue;
        SQE_TRY(st->keys.ensure((size_t)p.slots * 8));
        SQE_TRY(st->counts.ensure((size_t)p.slots * 4));
        AggCountArgs ca{};
        ca.bits = bits; ca.units = units; ca.col = sa.col[col_of_slot[g.field]];
        ca.base = p.base; ca.span = (int)p.span; ca.mask = (uint64_t)p.slots - 1;
        ca.keys = st->keys.as<int64_t>(); ca.counts = st->counts.as<uint32_t>();
        if (g.kind == SQE_AGG_HISTOGRAM) { ca.interval = g.interval; ca.offset = g.offset; }
        {
            StageTimer t(idx->ctx->prof, s, ST_SCAN);
            hipLaunchKernelGGL(agg_slots_init_kernel, dim3(grid_of(p.slots, 256)), dim3(256), 0, s, ca.keys, ca.counts, p.slots, p.mode, p.base,
                               g.interval, g.offset);
            if (p.route == SQE_AGG_ROUTE_DENSE) {
                const int dgrid = (int)std::min<int64_t>(AGG_DENSE_BLOCKS, (units + 3) / 4);
                hipLaunchKernelGGL(agg_dense_kernel, dim3(dgrid), dim3(256), (size_t)round_up(p.span * 4, 16), s, ca);     // at most 64 KiB
            } else {
                hipLaunchKernelGGL(agg_hash_kernel, dim3(grid), dim3(256), 0, s, ca);
            }
            SQE_HIP(hipGetLastError());
        }
        if (c.shard) {
            SQE_TRY(shard_buckets(st, g, p.slots, c.shard->agg[j], s));
            continue;
        }
        StageTimer t(idx->ctx->prof, s, ST_SELECT);
        int64_t* kj = key_dev + (size_t)j * dcap;
        int64_t* cj = count_dev + (size_t)j * dcap;
        if (g.kind == SQE_AGG_HISTOGRAM) {
            hipLaunchKernelGGL(agg_hist_write_kernel, dim3(grid_of(p.nb, 256)), dim3(256), 0, s, ca.keys, ca.counts, (int)p.nb, kj, cj);
        } else {
            const int64_t blocks = (p.slots + AGG_SELECT_BLOCK - 1) / AGG_SELECT_BLOCK;
            last.agg[j].select_blocks = (int32_t)blocks;
            SQE_TRY(st->cand_k.ensure((size_t)blocks * g.size * 8));
            SQE_TRY(st->cand_c.ensure((size_t)blocks * g.size * 4));
            SQE_TRY(st->occ.ensure((size_t)blocks * 4));
            hipLaunchKernelGGL(agg_select_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ca.keys, ca.counts, p.slots, g.size,
                               st->cand_k.as<int64_t>(), st->cand_c.as<uint32_t>(), st->occ.as<int>());
            hipLaunchKernelGGL(agg_merge_kernel, dim3(1), dim3(256), 0, s, st->cand_k.as<int64_t>(), st->cand_c.as<uint32_t>(),
                               st->occ.as<int>(), (int)blocks, g.size, stats[j].count, kj, cj, tail_dev + 3 * j);
        }
        SQE_HIP(hipGetLastError());
    }
    if (c.shard) return SQE_OK;
    if (any) {
        std::vector<int64_t> host(2 * (size_t)c.n_aggs * dcap + 3 * (size_t)c.n_aggs);
        SQE_HIP(hipMemcpyAsync(host.data(), key_dev, host.size() * 8, hipMemcpyDeviceToHost, s));
        SQE_HIP(hipStreamSynchronize(s));
        const int64_t* hk = host.data();
        const int64_t* hc = hk + (size_t)c.n_aggs * dcap;
        const int64_t* ht = hc + (size_t)c.n_aggs * dcap;
        for (int j = 0; j < c.n_aggs; ++j) {
            if (dcap > 0) {
                memcpy(c.key_out + (size_t)j * c.bucket_cap, hk + (size_t)j * dcap, (size_t)dcap * 8);
                memcpy(c.count_out + (size_t)j * c.bucket_cap, hc + (size_t)j * dcap, (size_t)dcap * 8);
            }
            pad_buckets(c, j, dcap);
            if (c.aggs[j].kind == SQE_AGG_TERMS && plan[j].route != SQE_AGG_ROUTE_NONE) {
                c.result_out[j].n_buckets = ht[3 * j];
                c.result_out[j].other = ht[3 * j + 1];
                last.agg[j].occupied_blocks = (int32_t)ht[3 * j + 2];
            }
        }
    } else {
        for (int j = 0; j < c.n_aggs; ++j) pad_buckets(c, j, 0);
    }
    st->last = last;
    st->has_last = true;
    return SQE_OK;
}

}  // namespace

int index_aggregate_shard(sqe_index* sh, const RowSet& set, const sqe_field_agg_t* aggs, int n_aggs, AggShardResult* out, hipStream_t s) {
    if (!sh->agg) sh->agg = new (std::nothrow) AggState;
    if (!sh->agg) return fail(SQE_ERR_OOM, "sqe_index_aggregate_fields: host allocation failed");
    const AggCall call{set, aggs, n_aggs, 0, nullptr, nullptr, nullptr, nullptr, out};
    const int rc = aggregate_impl(sh, sh->agg, call, s);
    if (rc != SQE_OK) (void)hipStreamSynchronize(s);         // the staged allow-list is host memory of the caller
    return rc;
}

}  // namespace sqe

// ================================================================ C ABI
using namespace sqe;

static_assert(sizeof(sqe_field_agg_t) == 32 && sizeof(sqe_field_agg_result_t) == 56 && sizeof(sqe_agg_last_t) == 8 + 8 * 32, "sqe.h layouts");

extern "C" {

int sqe_index_aggregate_fields(sqe_index* idx, const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                               const int64_t* allow_ids_host, int64_t n_allow, const sqe_field_agg_t* aggs, int n_aggs, int64_t bucket_cap,
                               int64_t* selected_out, sqe_field_agg_result_t* result_out, int64_t* key_out, int64_t* count_out) {
    const std::string who = "sqe_index_aggregate_fields: ";
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    int64_t one[2];
    SQE_TRY(rowset_args_ok("sqe_index_aggregate_fields", clauses, n_clauses, set_values, n_set, allow_ids_host, n_allow, one));
    const RowSet set{FieldPreds{clauses, one, 1, set_values, n_set}, allow_ids_host, n_allow, true};
    if (n_aggs < 1 || n_aggs > AGG_MAX || !aggs) return fail(SQE_ERR_INVALID, who + "between 1 and 8 aggregations");
    if (bucket_cap < 0) return fail(SQE_ERR_INVALID, who + "bucket_cap < 0");
    if (!selected_out || !result_out || (bucket_cap > 0 && (!key_out || !count_out))) return fail(SQE_ERR_INVALID, who + "null buffer");
    for (int j = 0; j < n_aggs; ++j) {
        const sqe_field_agg_t& g = aggs[j];
        const std::string at = who + "aggregation " + std::to_string(j) + ": ";
        if (g.kind != SQE_AGG_STATS && g.kind != SQE_AGG_TERMS && g.kind != SQE_AGG_HISTOGRAM) return fail(SQE_ERR_INVALID, at + "unknown kind");
        if (g.field < 0 || g.field >= FIELD_MAX) return fail(SQE_ERR_INVALID, at + "field slots are 0..7");
        if (g.kind == SQE_AGG_TERMS && (g.size < 1 || g.size > AGG_MAX_SIZE || g.size > bucket_cap))
            return fail(SQE_ERR_INVALID, at + "need 1 <= size <= 256 and size <= bucket_cap");
        if (g.kind == SQE_AGG_HISTOGRAM && (g.interval < 1 || g.offset < 0 || g.offset >= g.interval))
            return fail(SQE_ERR_INVALID, at + "need interval >= 1 and 0 <= offset < interval");
    }
    if (idx->group) return group_index_aggregate_fields(idx, set, aggs, n_aggs, bucket_cap, selected_out, result_out, key_out, count_out);
    OpScope op(idx->ctx, idx->ord, true);
    if (!idx->agg) idx->agg = new (std::nothrow) AggState;
    if (!idx->agg) return fail(SQE_ERR_OOM, who + "host allocation failed");
    const AggCall call{set, aggs, n_aggs, bucket_cap, selected_out, result_out, key_out, count_out, nullptr};
    const int rc = aggregate_impl(idx, idx->agg, call, op.s);
    if (rc != SQE_OK) (void)hipStreamSynchronize(op.s);      // the staged allow-list is host memory of the caller
    return rc;
}

int sqe_index_aggregate_last(sqe_index* idx, sqe_agg_last_t* out) {
    if (!idx || !out) return fail(SQE_ERR_INVALID, "sqe_index_aggregate_last: null argument");
    if (idx->group) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_aggregate_last: single-device indexes only");
    std::lock_guard<std::mutex> lk(idx->ord.mu);
    if (!idx->agg || !idx->agg->has_last) return fail(SQE_ERR_STATE, "sqe_index_aggregate_last: no aggregation ran on this index yet");
    *out = idx->agg->last;
    return SQE_OK;
}

}  // extern "C"
