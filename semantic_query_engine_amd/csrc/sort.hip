// sort.hip -- sorting on the numeric fields (sqe_index_sort_fields): the first k rows, in the order of 1..4 field keys, of the
// rows a field predicate (and an optional allow-list) selects, with a search_after cursor.  Integers only: every answer is
// defined exactly by the tuple (u_0, ..., u_{n_sort - 1}, id) ascending, u_j the order image of the row's value in sort slot j
// (fieldsort.h: sort_image), and does not depend on the order in which rows, waves or workgroups arrive.
//
// The row set is the bitmap of sqe_index_search_where (rowset.hip: rowset_map); the kernels read it.
//   1. sort_slab_kernel: one 256-thread workgroup per slab of 16,384 row positions (256 bitmap units).  A wave takes a 64-row
//      unit, one row per lane; a zero bitmap word is skipped wave-uniformly and no column is read for it.  A row is ALIVE if its
//      bit is set and its tuple lies strictly after the cursor's.  The set bits add into the call's total BEFORE the cursor test.
//      A slab without an alive row writes a zero count and leaves; one with at most k alive rows sends them all; every other slab
//      runs the lexicographic select (sort_cascade) and writes its k candidates: position and the n_sort images.
//   2. sort_merge_kernel: one workgroup per group of up to fan_in candidate lists (64 x 256 = 16,384 tuples), the same cascade
//      over tuples; levels repeat until one list is left (10 M rows: 611 slabs -> 10 -> 1).  The last level ranks its <= k
//      winners by counting with the full tuple comparison and writes ids (through the id map) and the raw values (through the
//      columns, by position), then the padding.
// sort_cascade, level j: T = the (still wanted)-th smallest u_j among the alive items, by block_select_kth over ~u_j.  The block
// select finds the LARGEST keys and reads key 0 as "no key"; ~u is 0 exactly for u = 2^64 - 1, the one image it cannot see -- and
// then it answers 0 ("fewer keys than wanted"), whose complement 2^64 - 1 is the right T: the wanted-th smallest IS that image
// (or there are fewer alive items than wanted, and all of them win).  Items below T win; if they and the items equal to T are
// no more than what is wanted the equal ones win too and the select is over; else the equal ones are the alive set of level
// j + 1 with what is left wanted.  The level after the last key is the row position, which is unique, so the cut there is exact:
// the lowest positions win, and ids ascend with positions (internal.h, sqe_index::idmap: "strictly increasing over [0, n)";
// without a map the id is the position), so that is the id tie-break.  Alive and winner sets are two 2 KiB LDS bitmaps; a
// bitmap word belongs to one wave during a pass, so no pass needs an atomic on them.
// The columns are re-read from L2 / HBM by every byte pass of a level (coalesced 8-byte loads of the alive rows' units only).
// Device groups (group.hip: group_index_sort_fields): index_sort_shard runs all of this on a shard with ids mapped to global
// ids (local * P + p) on the device, so the cursor compares global ids; the leader merges the shards' k best (fieldsort_merge).
#include <string.h>

#include <algorithm>
#include <vector>

#include "block_select.h"
#include "fieldpred.h"
#include "fieldsort.h"
#include "internal.h"

static_assert(sizeof(sqe_field_sort_t) == sizeof(sqe::FieldSort) && SQE_SORT_DESC == sqe::SORT_DESC &&
                  SQE_SORT_MISSING_FIRST == sqe::SORT_MISSING_FIRST && SQE_MAX_FIELDS == sqe::SORT_FIELD_SLOTS,
              "sqe.h and fieldsort.h agree");
static_assert(sizeof(sqe_sort_last_t) == 24, "sqe.h layouts");

namespace sqe {

namespace {

constexpr int SORT_SLAB_UNITS = 256;                       // 64-row bitmap units of a slab
constexpr int SORT_SLAB = SORT_SLAB_UNITS * 64;            // row positions of a slab, and the items a cascade ranks at most
constexpr int SORT_WORDS = SORT_SLAB / 64;                 // words of an LDS item bitmap: one per thread
static_assert(SORT_MAX_K <= MAX_KP && SORT_MAX_K <= 256 && SORT_MAX_FAN_IN * SORT_MAX_K <= SORT_SLAB, "a merge group fits a cascade");
static_assert(SORT_MAX_KEYS == 4 && FIELD_NONE == SORT_FIELD_NONE, "fieldsort.h and fieldpred.h agree");

struct SortCols {
    const int64_t* col[SORT_MAX_KEYS];     // the column of sort key j by row position; null: the slot was never set, every row is missing
    int flags[SORT_MAX_KEYS];
    int n_sort;
    const int64_t* map;                    // position -> local id; null: the id is the position
    int64_t id_mul, id_add;                // the id a caller sees = local id * id_mul + id_add (a shard of a device group: P, p)
};

__device__ __forceinline__ uint64_t row_image(const SortCols& c, int j, int64_t p) {
    return sort_image(c.col[j] ? c.col[j][p] : FIELD_NONE, c.flags[j]);
}
__device__ __forceinline__ int64_t row_id(const SortCols& c, int64_t p) { return (c.map ? c.map[p] : p) * c.id_mul + c.id_add; }

struct SortLds {
    uint64_t alive[SORT_WORDS], win[SORT_WORDS];
    int hist[256];
    int cnt[2];
};

// The lexicographic select over the items [0, n_items) whose bit is set in L.alive: the `wanted` first of them in the order of
// get(0, e), ..., get(n_levels - 1, e) ascending get their bit set in L.win (all of them when there are fewer).  The keys of the
// last level are unique.  L.alive is complete and L.win zero (caller synchronised); every thread of the block (256) calls, from
// uniform control flow; ends synchronised.  Item e belongs to thread e % 256, so word e / 64 to one wave.
template <typename Get>
__device__ __forceinline__ void sort_cascade(Get get, int n_items, int n_levels, int wanted, SortLds& L) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int n_round = (n_items + 63) & ~63;
    for (int level = 0; level < n_levels; ++level) {
        const uint64_t Tk = block_select_kth<256, uint64_t, false>(
            [&](auto f) {
                for (int e = tid; e < n_round; e += 256) {
                    const uint64_t word = L.alive[e >> 6];
                    if (word == 0) continue;               // wave-uniform: nothing of these 64 items is alive, nothing is read
                    f(((word >> lane) & 1) ? ~get(level, e) : 0ull);
                }
            },
            wanted, L.hist);
        const uint64_t T = ~Tk;
        if (tid == 0) L.cnt[0] = L.cnt[1] = 0;
        __syncthreads();
        int below = 0, eq = 0;
        for (int e = tid; e < n_round; e += 256) {
            const int w = e >> 6;
            const uint64_t word = L.alive[w];
            if (word == 0) continue;
            const bool on = (word >> lane) & 1;
            const uint64_t u = on ? get(level, e) : 0ull;
            const uint64_t mb = __ballot((int)(on && u < T)), me = __ballot((int)(on && u == T));
            if (lane == 0) {
                L.win[w] |= mb;
                L.alive[w] = me;
                below += __popcll(mb);
                eq += __popcll(me);
            }
        }
        if (lane == 0 && (below | eq)) {
            atomicAdd(&L.cnt[0], below);
            atomicAdd(&L.cnt[1], eq);
        }
        __syncthreads();
        below = L.cnt[0];
        eq = L.cnt[1];
        if (below + eq <= wanted) {                        // block-uniform
            L.win[tid] |= L.alive[tid];
            __syncthreads();
            return;
        }
        wanted -= below;
        __syncthreads();                                   // everyone has read cnt before the next level clears it
    }
}

struct SortSlabArgs {
    const uint64_t* bits;                  // the row set: bit (p & 63) of word p >> 6
    int64_t units;                         // 64-row units of the map
    SortCols c;
    int k, has_cursor;
    uint64_t cur_u[SORT_MAX_KEYS];         // the cursor's images
    int64_t cur_id;
    int* cnt;                              // [slabs] candidates of each slab
    int64_t* pos;                          // [slabs, k]
    uint64_t* u;                           // [slabs, k, n_sort]
    unsigned long long* tail;              // [0] the selected rows, [1] the slabs that hold an alive row, [2] the candidates written
};

__device__ __forceinline__ bool after_cursor(const SortSlabArgs& a, int64_t p) {
    for (int j = 0; j < a.c.n_sort; ++j) {
        const uint64_t u = row_image(a.c, j, p);
        if (u != a.cur_u[j]) return u > a.cur_u[j];
    }
    return row_id(a.c, p) > a.cur_id;                      // strictly after: the cursor's own row does not come again
}

__global__ __launch_bounds__(256) void sort_slab_kernel(SortSlabArgs a) {
    __shared__ SortLds L;
    __shared__ int s_alive, s_sel, s_m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t unit0 = (int64_t)blockIdx.x * SORT_SLAB_UNITS, p0 = unit0 * 64;
    if (tid == 0) s_alive = s_sel = s_m = 0;
    L.win[tid] = 0;
    __syncthreads();
    int sel = 0, n_alive = 0;
    for (int w = wave; w < SORT_WORDS; w += 4) {
        const uint64_t word = unit0 + w < a.units ? a.bits[unit0 + w] : 0ull;
        uint64_t m = 0;
        if (word) {                                        // wave-uniform: a set bit is a live row, p < n, inside every column
            bool on = (word >> lane) & 1;
            if (on && a.has_cursor) on = after_cursor(a, p0 + (int64_t)w * 64 + lane);
            m = __ballot((int)on);
            sel += __popcll(word);                         // the total counts the rows before the cursor test
            n_alive += __popcll(m);
        }
        if (lane == 0) L.alive[w] = m;
    }
    if (lane == 0 && sel) {
        atomicAdd(&s_sel, sel);
        atomicAdd(&s_alive, n_alive);
    }
    __syncthreads();
    if (tid == 0 && s_sel) atomicAdd(a.tail, (unsigned long long)s_sel);
    n_alive = s_alive;
    if (n_alive == 0) {                                    // block-uniform
        if (tid == 0) a.cnt[blockIdx.x] = 0;
        return;
    }
    auto get = [&](int level, int e) -> uint64_t { return level < a.c.n_sort ? row_image(a.c, level, p0 + e) : (uint64_t)(p0 + e); };
    if (n_alive <= a.k) {
        L.win[tid] = L.alive[tid];
        __syncthreads();
    } else {
        sort_cascade(get, SORT_SLAB, a.c.n_sort + 1, a.k, L);
    }
    const int64_t out0 = (int64_t)blockIdx.x * a.k;
    for (int e = tid; e < SORT_SLAB; e += 256) {
        const uint64_t word = L.win[e >> 6];
        if (word == 0 || !((word >> lane) & 1)) continue;
        const int slot = atomicAdd(&s_m, 1);
        if (slot >= a.k) continue;                         // never: the cascade selects at most k
        a.pos[out0 + slot] = p0 + e;
        for (int j = 0; j < a.c.n_sort; ++j) a.u[(out0 + slot) * a.c.n_sort + j] = row_image(a.c, j, p0 + e);
    }
    __syncthreads();
    if (tid == 0) {
        const int m = min(s_m, a.k);
        a.cnt[blockIdx.x] = m;
        atomicAdd(a.tail + 1, 1ull);
        atomicAdd(a.tail + 2, (unsigned long long)m);
    }
}

struct SortMergeArgs {
    const int* cnt_in;                     // [n_lists]
    const int64_t* pos_in;                 // [n_lists, k]
    const uint64_t* u_in;                  // [n_lists, k, n_sort]
    int n_lists, fan_in, k, final;
    int* cnt_out;                          // not final: [groups], [groups, k], [groups, k, n_sort]
    int64_t* pos_out;
    uint64_t* u_out;
    SortCols c;                            // final: the columns and the id map behind the answer
    int64_t* id_out;                       // final: [k]
    int64_t* value_out;                    // final: [k, n_sort]
};

__global__ __launch_bounds__(256) void sort_merge_kernel(SortMergeArgs a) {
    __shared__ SortLds L;
    __shared__ int s_alive, s_m;
    __shared__ int64_t top_pos[SORT_MAX_K];
    __shared__ uint64_t top_u[SORT_MAX_KEYS][SORT_MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_sort = a.c.n_sort;
    const int l0 = blockIdx.x * a.fan_in;
    const int nl = min(a.fan_in, a.n_lists - l0);
    const int n_items = nl * a.k;                          // at most 16,384: item e is entry e % k of list l0 + e / k
    const int64_t first = (int64_t)l0 * a.k;
    if (tid == 0) s_alive = s_m = 0;
    L.win[tid] = 0;
    __syncthreads();
    int n_alive = 0;
    for (int w = wave; w < SORT_WORDS; w += 4) {
        const int e = w * 64 + lane;
        const bool on = e < n_items && (e % a.k) < a.cnt_in[l0 + e / a.k];
        const uint64_t m = __ballot((int)on);
        if (lane == 0) L.alive[w] = m;
        n_alive += __popcll(m);
    }
    if (lane == 0 && n_alive) atomicAdd(&s_alive, n_alive);
    __syncthreads();
    n_alive = s_alive;
    auto get = [&](int level, int e) -> uint64_t {
        return level < n_sort ? a.u_in[(first + e) * n_sort + level] : (uint64_t)a.pos_in[first + e];
    };
    if (n_alive <= a.k) {
        L.win[tid] = L.alive[tid];
        __syncthreads();
    } else {
        sort_cascade(get, n_items, n_sort + 1, a.k, L);
    }
    const int n_round = (n_items + 63) & ~63;
    const int64_t out0 = (int64_t)blockIdx.x * a.k;
    for (int e = tid; e < n_round; e += 256) {
        const uint64_t word = L.win[e >> 6];
        if (word == 0 || !((word >> lane) & 1)) continue;
        const int slot = atomicAdd(&s_m, 1);
        if (slot >= a.k) continue;                         // never: the cascade selects at most k
        if (a.final) {
            top_pos[slot] = a.pos_in[first + e];
            for (int j = 0; j < n_sort; ++j) top_u[j][slot] = get(j, e);
        } else {
            a.pos_out[out0 + slot] = a.pos_in[first + e];
            for (int j = 0; j < n_sort; ++j) a.u_out[(out0 + slot) * n_sort + j] = get(j, e);
        }
    }
    __syncthreads();
    const int m = min(s_m, a.k);
    if (!a.final) {
        if (tid == 0) a.cnt_out[blockIdx.x] = m;
        return;
    }
    // the winners in order: the rank of one is the number of winners before it (positions are unique, so the ranks are 0 .. m - 1)
    for (int i = tid; i < a.k; i += 256) {
        if (i < m) {
            const int64_t pi = top_pos[i];
            int rank = 0;
            for (int o = 0; o < m; ++o) {
                bool before = false, decided = false;
                for (int j = 0; j < n_sort; ++j) {
                    if (decided) continue;
                    const uint64_t uo = top_u[j][o], ui = top_u[j][i];
                    if (uo != ui) {
                        before = uo < ui;
                        decided = true;
                    }
                }
                if (!decided) before = top_pos[o] < pi;
                rank += before ? 1 : 0;
            }
            a.id_out[rank] = row_id(a.c, pi);
            for (int j = 0; j < n_sort; ++j) a.value_out[rank * n_sort + j] = a.c.col[j] ? a.c.col[j][pi] : FIELD_NONE;
        } else {
            a.id_out[i] = -1;
            for (int j = 0; j < n_sort; ++j) a.value_out[i * n_sort + j] = FIELD_NONE;
        }
    }
}

}  // namespace

struct SortState {
    DevBuf cnt[2], pos[2], u[2];   // candidate lists, ping-pong over the merge levels: i32 [lists], i64 [lists, k], u64 [lists, k, n_sort]
    DevBuf out;                    // ids i64 [k] | values i64 [k, n_sort] | tail u64 [3]
    sqe_sort_last_t last{};        // the last call (sqe_index_sort_last)
    bool has_last = false;
};

void sort_destroy(SortState* s) { delete s; }

namespace {

struct SortCall {
    const RowSet& set;             // a host list, if any
    const FieldSort* sort;
    int n_sort, k;
    const int64_t* after_values;   // null: no cursor
    int64_t after_id;
    int64_t id_mul, id_add;
    int64_t* total_out;            // host
    int64_t* id_out;               // host [k]
    int64_t* value_out;            // host [k, n_sort]
};

int sort_impl(sqe_index* idx, SortState* st, const SortCall& c, hipStream_t s) {
    const int64_t n = idx->n.load();
    const int k = c.k, n_sort = c.n_sort;
    sqe_sort_last_t last{};
    last.fan_in = idx->sort_fan_in;
    if (n == 0 || c.set.n_allow == 0) {
        *c.total_out = 0;
        for (int i = 0; i < k; ++i) c.id_out[i] = -1;
        for (int i = 0; i < k * n_sort; ++i) c.value_out[i] = FIELD_NONE;
        st->last = last;
        st->has_last = true;
        return SQE_OK;
    }
    // ---- the row set's map (rowset_map); its positions are not wanted
    FilterState* f;
    int64_t words;
    SQE_TRY(rowset_map(idx, c.set, &f, &words, s));
    const int slabs = (int)((n + SORT_SLAB - 1) / SORT_SLAB);
    const int fan = idx->sort_fan_in;
    const int groups1 = (slabs + fan - 1) / fan;
    SQE_TRY(st->cnt[0].ensure((size_t)slabs * 4));
    SQE_TRY(st->pos[0].ensure((size_t)slabs * k * 8));
    SQE_TRY(st->u[0].ensure((size_t)slabs * k * n_sort * 8));
    SQE_TRY(st->cnt[1].ensure((size_t)groups1 * 4));
    SQE_TRY(st->pos[1].ensure((size_t)groups1 * k * 8));
    SQE_TRY(st->u[1].ensure((size_t)groups1 * k * n_sort * 8));
    const size_t ob = (size_t)k * 8 * (1 + n_sort);
    SQE_TRY(st->out.ensure(ob + 24));
    int64_t* id_dev = st->out.as<int64_t>();
    int64_t* value_dev = id_dev + k;
    unsigned long long* tail_dev = reinterpret_cast<unsigned long long*>(value_dev + (size_t)k * n_sort);
    SortCols cols{};
    cols.n_sort = n_sort;
    for (int j = 0; j < n_sort; ++j) {
        cols.col[j] = fields_column(idx, c.sort[j].field);
        cols.flags[j] = c.sort[j].flags;
    }
    cols.map = idx->has_map ? idx->idmap.as<int64_t>() : nullptr;
    cols.id_mul = c.id_mul;
    cols.id_add = c.id_add;
    int levels = 0;
    {
        StageTimer t(idx->ctx->prof, s, ST_SELECT);
        SQE_HIP(hipMemsetAsync(tail_dev, 0, 24, s));
        SortSlabArgs sa{};
        sa.bits = reinterpret_cast<const uint64_t*>(filter_bitmap(f));
        sa.units = words / 2;
        sa.c = cols;
        sa.k = k;
        sa.has_cursor = c.after_values ? 1 : 0;
        if (c.after_values) fieldsort_cursor(c.sort, n_sort, c.after_values, sa.cur_u);
        sa.cur_id = c.after_id;
        sa.cnt = st->cnt[0].as<int>();
        sa.pos = st->pos[0].as<int64_t>();
        sa.u = st->u[0].as<uint64_t>();
        sa.tail = tail_dev;
        hipLaunchKernelGGL(sort_slab_kernel, dim3((unsigned)slabs), dim3(256), 0, s, sa);
        int lists = slabs, from = 0;
        for (;;) {
            const int groups = (lists + fan - 1) / fan;
            SortMergeArgs ma{};
            ma.cnt_in = st->cnt[from].as<int>();
            ma.pos_in = st->pos[from].as<int64_t>();
            ma.u_in = st->u[from].as<uint64_t>();
            ma.n_lists = lists;
            ma.fan_in = fan;
            ma.k = k;
            ma.final = groups == 1 ? 1 : 0;
            ma.cnt_out = st->cnt[from ^ 1].as<int>();
            ma.pos_out = st->pos[from ^ 1].as<int64_t>();
            ma.u_out = st->u[from ^ 1].as<uint64_t>();
            ma.c = cols;
            ma.id_out = id_dev;
            ma.value_out = value_dev;
            hipLaunchKernelGGL(sort_merge_kernel, dim3((unsigned)groups), dim3(256), 0, s, ma);
            ++levels;
            if (groups == 1) break;
            lists = groups;
            from ^= 1;
        }
        SQE_HIP(hipGetLastError());
    }
    std::vector<int64_t> host((size_t)k * (1 + n_sort) + 3);
    SQE_HIP(hipMemcpyAsync(host.data(), id_dev, host.size() * 8, hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));                        // the one synchronisation (the staged allow-list may go, too)
    memcpy(c.id_out, host.data(), (size_t)k * 8);
    memcpy(c.value_out, host.data() + k, (size_t)k * n_sort * 8);
    const int64_t* tail = host.data() + (size_t)k * (1 + n_sort);
    *c.total_out = tail[0];
    last.slabs = slabs;
    last.slabs_occupied = (int32_t)tail[1];
    last.merge_levels = levels;
    last.candidates = tail[2];
    st->last = last;
    st->has_last = true;
    return SQE_OK;
}

SortState* sort_state(sqe_index* idx) {
    if (!idx->sort) idx->sort = new (std::nothrow) SortState;
    return idx->sort;
}

}  // namespace

int index_sort_shard(sqe_index* sh, const RowSet& set, const sqe_field_sort_t* sort, int n_sort, int k, const int64_t* after_values,
                     int64_t after_id, int64_t id_mul, int64_t id_add, int64_t* total_out, int64_t* id_out, int64_t* value_out, hipStream_t s) {
    SortState* st = sort_state(sh);
    if (!st) return fail(SQE_ERR_OOM, "sqe_index_sort_fields: host allocation failed");
    const SortCall call{set, reinterpret_cast<const FieldSort*>(sort), n_sort, k, after_values, after_id, id_mul, id_add, total_out, id_out,
                        value_out};
    const int rc = sort_impl(sh, st, call, s);
    if (rc != SQE_OK) (void)hipStreamSynchronize(s);         // the staged allow-list is host memory of the caller
    return rc;
}

}  // namespace sqe

// ================================================================ C ABI
using namespace sqe;

extern "C" {

int sqe_index_sort_fields(sqe_index* idx, const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                          const int64_t* allow_ids_host, int64_t n_allow, const sqe_field_sort_t* sort, int n_sort, int k,
                          const int64_t* after_values, int64_t after_id, int64_t* total_out, int64_t* id_out, int64_t* value_out) {
    const std::string who = "sqe_index_sort_fields: ";
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    int64_t one[2];
    SQE_TRY(rowset_args_ok("sqe_index_sort_fields", clauses, n_clauses, set_values, n_set, allow_ids_host, n_allow, one));
    const RowSet set{FieldPreds{clauses, one, 1, set_values, n_set}, allow_ids_host, n_allow, true};
    const char* why = fieldsort_check(reinterpret_cast<const FieldSort*>(sort), n_sort, k);
    if (why) return fail(SQE_ERR_INVALID, who + why);
    if (!total_out || !id_out || !value_out) return fail(SQE_ERR_INVALID, who + "null buffer");
    if (idx->group) return group_index_sort_fields(idx, set, sort, n_sort, k, after_values, after_id, total_out, id_out, value_out);
    OpScope op(idx->ctx, idx->ord, true);
    return index_sort_shard(idx, set, sort, n_sort, k, after_values, after_id, 1, idx->id_base, total_out, id_out, value_out, op.s);
}

int sqe_index_sort_last(sqe_index* idx, sqe_sort_last_t* out) {
    if (!idx || !out) return fail(SQE_ERR_INVALID, "sqe_index_sort_last: null argument");
    if (idx->group) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_sort_last: single-device indexes only");
    std::lock_guard<std::mutex> lk(idx->ord.mu);
    if (!idx->sort || !idx->sort->has_last) return fail(SQE_ERR_STATE, "sqe_index_sort_last: no field sort ran on this index yet");
    *out = idx->sort->last;
    return SQE_OK;
}

}  // extern "C"
