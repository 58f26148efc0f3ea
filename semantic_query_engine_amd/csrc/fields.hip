// fields.hip -- numeric fields (sqe_index_set_field / get_field) and the predicates over them (sqe_index_match_fields,
// sqe_index_search_where, sqe_index_search_where_each).
//
// A field is one int64 column indexed by row position, SQE_FIELD_NONE where a row has no value and past n; it lives as the group
// keys do: allocated by the first set_field of its slot, grown with the rows, compacted by a delete (a kernel of its own per
// column, out of place, from the delete's sorted position list), never saved.
//
// A predicate is the AND of at most 8 clauses (RANGE or IN over one field, either negated).  field_match_kernel evaluates all
// predicates of a call in one pass over the rows and writes one bitmap per predicate in the layout the filtered search compacts
// (filter.hip): the rest of every call -- count, scan, write, gather, search -- is that code, unchanged.
//   * one wave handles 64 consecutive positions, one row per lane;
//   * the host sorts the clauses by field (fieldpred_plan), so the kernel walks the 8 slots, loads the column's value of its row
//     once into a register (a coalesced 8-byte load) and applies every clause of every predicate that names the slot: P
//     predicates read a column once, not P times, and no register array is indexed at run time;
//   * a lane keeps one bit per predicate ("still holds"); a clause that fails clears its predicate's bit;
//   * the clause table and the set values are staged in LDS, IN is a binary search there;
//   * one ballot per predicate gives the 64 rows' result, which lane 0 stores (ANDed into the map when an allow-list filled it).
#include <string.h>

#include <algorithm>
#include <vector>

#include "fieldpred.h"
#include "id_lists.h"
#include "internal.h"

static_assert(sizeof(sqe_field_clause_t) == sizeof(sqe::FieldClause) && SQE_MAX_FIELDS == sqe::FIELD_MAX, "sqe.h and fieldpred.h agree");
static_assert(sizeof(sqe_where_last_t) == 40, "sqe.h layouts");
static_assert(SQE_FOP_RANGE == sqe::FIELD_OP_RANGE && SQE_FOP_IN == sqe::FIELD_OP_IN && SQE_FOP_NOT == sqe::FIELD_OP_NOT, "ops agree");

namespace sqe {

struct FieldState {
    DevBuf col[FIELD_MAX];         // i64 [cap]: column of slot f by row position; p == null: the slot was never set
    int64_t col_cap = 0;           // rows every allocated column holds
    DevBuf tab;                    // the plan of a call: header | clauses [n_clauses] x 32 B | set values [n_set]
    DevBuf bits;                   // u32 [n_preds, words]: one map per predicate (match_fields, search_where_each)
    DevBuf counts;                 // per predicate: i32 [nb] | i64 [nb] | i64 total
    DevBuf totals;                 // i64 [n_preds]
    DevBuf pos;                    // i64 [n]: one predicate's positions (match_fields)
    DevBuf lists;                  // i64: the position lists of search_where_each, one after the other
    DevBuf stage;                  // host entry points: queries in, results out
};

namespace {

constexpr int WORDS_PER_BLOCK = 1024;      // the filtered search's map block (filter.hip)
constexpr int MATCH_MAX_BLOCKS = 2048;     // workgroups of the match kernel (they stride over the rows)

// What the kernel stages in LDS, as one run of 8-byte words: the header, the planned clauses, the set values.
struct FieldMatchHeader {
    const int64_t* col[FIELD_MAX];         // null: never set, every row reads SQE_FIELD_NONE
    int first[FIELD_MAX + 1];              // clauses of slot f: [first[f], first[f + 1])
    int pad;
};
constexpr int HEADER_WORDS = sizeof(FieldMatchHeader) / 8;
static_assert(sizeof(FieldMatchHeader) % 8 == 0 && sizeof(FieldPlanClause) == 32, "the staged table is a run of 8-byte words");

struct FieldMatchArgs {
    const int64_t* tab;                    // header | clauses [n_clauses] sorted by slot | set values [n_set]
    int n_clauses, n_set, n_preds, and_into;
    int64_t n;                             // live rows
    int64_t units;                         // 64-row units of a map = words / 2
    uint64_t* bits;                        // [n_preds, units]
};

__global__ __launch_bounds__(256) void field_match_kernel(FieldMatchArgs a) {
    extern __shared__ __align__(16) int64_t lds[];
    const int tab_words = HEADER_WORDS + a.n_clauses * 4 + a.n_set;
    for (int i = threadIdx.x; i < tab_words; i += 256) lds[i] = a.tab[i];
    __syncthreads();
    const FieldMatchHeader* hd = reinterpret_cast<const FieldMatchHeader*>(lds);
    const FieldPlanClause* cl = reinterpret_cast<const FieldPlanClause*>(lds + HEADER_WORDS);
    const int64_t* sv = lds + HEADER_WORDS + a.n_clauses * 4;
    const int lane = threadIdx.x & 63;
    const uint64_t all = a.n_preds >= 64 ? ~0ull : (1ull << a.n_preds) - 1;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < a.units; u += (int64_t)gridDim.x * 4) {
        const int64_t p = u * 64 + lane;
        const bool live = p < a.n;
        uint64_t holds = live ? all : 0;                   // bit j: predicate j still holds for this lane's row
        for (int f = 0; f < FIELD_MAX; ++f) {
            const int c0 = __builtin_amdgcn_readfirstlane(hd->first[f]), c1 = __builtin_amdgcn_readfirstlane(hd->first[f + 1]);
            if (c0 == c1) continue;                        // no clause names the slot: its column is not read
            const int64_t* col = hd->col[f];
            const int64_t v = (live && col) ? col[p] : FIELD_NONE;     // the one read of this column for this row
            const bool has = v != FIELD_NONE;
            for (int c = c0; c < c1; ++c) {
                const FieldPlanClause k = cl[c];
                bool r;
                if ((k.op & 0xFF) == FIELD_OP_IN) {
                    int lo = (int)k.lo, hi = (int)k.hi;      // first value >= v in sv[lo, hi)
                    const int end = hi;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (sv[mid] < v) lo = mid + 1;
                        else hi = mid;
                    }
                    r = has && lo < end && sv[lo] == v;
                } else {
                    r = has && k.lo <= v && v <= k.hi;
                }
                if (k.op & FIELD_OP_NOT) r = !r;
                if (!r) holds &= ~(1ull << k.pred);
            }
        }
        for (int j = 0; j < a.n_preds; ++j) {
            const uint64_t m = __ballot((int)((holds >> j) & 1));
            if (lane == 0) {
                uint64_t* w = a.bits + (int64_t)j * a.units + u;
                *w = a.and_into ? (*w & m) : m;
            }
        }
    }
}

__global__ __launch_bounds__(256) void field_fill_kernel(int64_t* __restrict__ p, int64_t n, int64_t value) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = value;
}

__global__ __launch_bounds__(256) void field_scatter_kernel(int64_t* __restrict__ col, const int64_t* __restrict__ pos,
                                                            const int64_t* __restrict__ val, int64_t m) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < m) col[pos[j]] = val[j];
}

__global__ __launch_bounds__(256) void field_gather_kernel(const int64_t* __restrict__ col, const int64_t* __restrict__ pos,
                                                           int64_t* __restrict__ out, int64_t m) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < m) out[j] = col[pos[j]];
}

// a delete, out of place: dst[i - (deleted positions below i)] = src[i] for the rows that stay, SQE_FIELD_NONE from n_new on
__global__ __launch_bounds__(256) void field_compact_kernel(const int64_t* __restrict__ src, int64_t* __restrict__ dst,
                                                            const int64_t* __restrict__ del, int64_t m, int64_t n_old, int64_t cap) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    if (i >= n_old - m) dst[i] = FIELD_NONE;              // nobody else writes at or beyond n_new
    if (i >= n_old) return;
    bool hit;
    const int64_t below = del_rank(del, m, i, &hit);
    if (!hit) dst[i - below] = src[i];
}

// count_out[j] = the total of predicate j's scan
__global__ __launch_bounds__(64) void field_totals_kernel(const char* __restrict__ counts, int64_t stride, int64_t total_off, int n_preds,
                                                          int64_t* __restrict__ out) {
    const int j = threadIdx.x;
    if (j < n_preds) out[j] = *reinterpret_cast<const int64_t*>(counts + j * stride + total_off);
}

// out[i] = the id of pos[i] for i < min(*total, cap), -1 beyond
__global__ __launch_bounds__(256) void field_emit_kernel(const int64_t* __restrict__ pos, const int64_t* __restrict__ total, int64_t cap,
                                                         const int64_t* __restrict__ map, int64_t id_base, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    if (i < *total) {
        const int64_t p = pos[i];
        out[i] = (map ? map[p] : p) + id_base;
    } else {
        out[i] = -1;
    }
}

int fill(int64_t* p, int64_t n, int64_t value, hipStream_t s) {
    if (n <= 0) return SQE_OK;
    hipLaunchKernelGGL(field_fill_kernel, dim3(grid_of(n, 256)), dim3(256), 0, s, p, n, value);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

FieldState* field_state(sqe_index* idx) {
    if (!idx->fields) idx->fields = new (std::nothrow) FieldState;
    return idx->fields;
}

struct MapLayout {         // the maps and count buffers of n_preds predicates over the index as it stands
    int64_t words, nb, units, cstride, offs_off, total_off;
    explicit MapLayout(int64_t n) {
        words = round_up((n + 31) / 32, WORDS_PER_BLOCK);
        nb = words / WORDS_PER_BLOCK;
        units = words / 2;
        offs_off = round_up(nb * 4, 8);
        total_off = offs_off + nb * 8;
        cstride = round_up(total_off + 8, 16);
    }
};

// the plan of pr to the device and the match kernel over rows [0, n): bits [pr.n_preds, words]
int fields_eval(sqe_index* idx, FieldState* st, const FieldPreds& pr, const MapLayout& L, uint32_t* bits, bool and_into, hipStream_t s) {
    FieldPlan plan;
    fieldpred_plan(reinterpret_cast<const FieldClause*>(pr.clauses), pr.offsets, pr.n_preds, plan);
    FieldMatchHeader hd{};
    for (int f = 0; f < FIELD_MAX; ++f) hd.col[f] = st->col[f].as<int64_t>();
    memcpy(hd.first, plan.first, sizeof hd.first);
    const size_t hb = sizeof hd, cb = plan.clauses.size() * sizeof(FieldPlanClause), sb = (size_t)pr.n_set * 8;
    std::vector<char> host(hb + cb + sb);
    memcpy(host.data(), &hd, hb);
    if (cb) memcpy(host.data() + hb, plan.clauses.data(), cb);
    if (sb) memcpy(host.data() + hb + cb, pr.set_values, sb);
    SQE_TRY(st->tab.ensure(host.size()));
    // the tables are host memory: the copy is staged before the call returns
    SQE_HIP(hipMemcpyAsync(st->tab.p, host.data(), host.size(), hipMemcpyHostToDevice, s));
    FieldMatchArgs a;
    a.tab = st->tab.as<int64_t>();
    a.n_clauses = (int)plan.clauses.size(); a.n_set = (int)pr.n_set; a.n_preds = pr.n_preds; a.and_into = and_into ? 1 : 0;
    a.n = idx->n.load(); a.units = L.units; a.bits = reinterpret_cast<uint64_t*>(bits);
    const unsigned grid = (unsigned)std::min<int64_t>(MATCH_MAX_BLOCKS, (L.units + 3) / 4);
    hipLaunchKernelGGL(field_match_kernel, dim3(grid), dim3(256), host.size(), s, a);      // at most 104 B + 16 KiB + 32 KiB of LDS
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int ensure_column(sqe_index* idx, FieldState* st, int field, hipStream_t s) {
    if (st->col[field].p) return SQE_OK;
    const int64_t cap = std::max<int64_t>(idx->cap, 1);
    SQE_TRY(st->col[field].ensure((size_t)cap * 8));
    st->col_cap = cap;
    return fill(st->col[field].as<int64_t>(), cap, FIELD_NONE, s);
}

}  // namespace

void fields_destroy(FieldState* f) { delete f; }

int fields_bitmap_eval(sqe_index* idx, const FieldPreds& pr, uint32_t* bits, bool and_into, hipStream_t s) {
    FieldState* st = field_state(idx);
    if (!st) return fail(SQE_ERR_OOM, "field predicate: host allocation failed");
    return fields_eval(idx, st, pr, MapLayout(idx->n.load()), bits, and_into, s);
}

const int64_t* fields_column(const sqe_index* idx, int field) { return idx->fields ? idx->fields->col[field].as<int64_t>() : nullptr; }

int fields_args_ok(const char* who, const FieldPreds& pr) {
    const char* why = fieldpred_check(reinterpret_cast<const FieldClause*>(pr.clauses), pr.offsets, pr.n_preds, pr.set_values, pr.n_set);
    if (why) return fail(SQE_ERR_INVALID, std::string(who) + ": " + why);
    return SQE_OK;
}

int fields_grow(sqe_index* idx, int64_t n, int64_t new_cap, hipStream_t s) {
    FieldState* st = idx->fields;
    DevBuf fresh[FIELD_MAX];
    bool any = false;
    for (int f = 0; f < FIELD_MAX; ++f) {
        if (!st->col[f].p) continue;
        any = true;
        SQE_TRY(fresh[f].ensure((size_t)new_cap * 8));
        SQE_TRY(fill(fresh[f].as<int64_t>() + n, new_cap - n, FIELD_NONE, s));
        if (n > 0) SQE_HIP(hipMemcpyAsync(fresh[f].p, st->col[f].p, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    }
    if (!any) return SQE_OK;
    SQE_HIP(hipStreamSynchronize(s));                       // nothing reads the old columns any more
    for (int f = 0; f < FIELD_MAX; ++f) {
        if (!fresh[f].p) continue;
        std::swap(fresh[f].p, st->col[f].p);
        std::swap(fresh[f].bytes, st->col[f].bytes);
    }
    st->col_cap = new_cap;
    return SQE_OK;
}

int fields_rows_deleted(sqe_index* idx, const int64_t* del_dev, int64_t m, int64_t n_old, hipStream_t s) {
    FieldState* st = idx->fields;
    DevBuf fresh[FIELD_MAX];
    bool any = false;
    for (int f = 0; f < FIELD_MAX; ++f) {
        if (!st->col[f].p) continue;
        any = true;
        SQE_TRY(fresh[f].ensure((size_t)st->col_cap * 8));
        hipLaunchKernelGGL(field_compact_kernel, dim3(grid_of(st->col_cap, 256)), dim3(256), 0, s, st->col[f].as<int64_t>(),
                           fresh[f].as<int64_t>(), del_dev, m, n_old, st->col_cap);
        SQE_HIP(hipGetLastError());
    }
    if (!any) return SQE_OK;
    SQE_HIP(hipStreamSynchronize(s));
    for (int f = 0; f < FIELD_MAX; ++f) {
        if (!fresh[f].p) continue;
        std::swap(fresh[f].p, st->col[f].p);
        std::swap(fresh[f].bytes, st->col[f].bytes);
    }
    return SQE_OK;
}

int index_set_field_at(sqe_index* idx, int field, const std::vector<int64_t>& pos, const int64_t* values_host, hipStream_t s) {
    // a position that repeats keeps its last value: the scatter below then writes every position once
    std::vector<std::pair<int64_t, int64_t>> order(pos.size());
    bool any_value = false;
    for (size_t j = 0; j < pos.size(); ++j) {
        order[j] = {pos[j], (int64_t)j};
        any_value |= values_host[j] != FIELD_NONE;
    }
    if (!(idx->fields && idx->fields->col[field].p) && !any_value) return SQE_OK;      // nothing to remove
    FieldState* st = field_state(idx);
    if (!st) return fail(SQE_ERR_OOM, "sqe_index_set_field: host allocation failed");
    std::sort(order.begin(), order.end());
    std::vector<int64_t> up;
    up.reserve(pos.size() * 2);
    for (size_t j = 0; j < order.size(); ++j)
        if (j + 1 == order.size() || order[j + 1].first != order[j].first) up.push_back(order[j].first);
    const size_t m = up.size();
    for (size_t j = 0; j < order.size(); ++j)
        if (j + 1 == order.size() || order[j + 1].first != order[j].first) up.push_back(values_host[order[j].second]);
    SQE_TRY(ensure_column(idx, st, field, s));
    if (m == 0) return SQE_OK;
    DevBuf tmp;
    SQE_TRY(tmp.ensure(m * 16));
    SQE_HIP(hipMemcpyAsync(tmp.p, up.data(), m * 16, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(field_scatter_kernel, dim3(grid_of((int64_t)m, 256)), dim3(256), 0, s, st->col[field].as<int64_t>(),
                       tmp.as<int64_t>(), tmp.as<int64_t>() + m, (int64_t)m);
    SQE_HIP(hipGetLastError());
    SQE_HIP(hipStreamSynchronize(s));                       // the upload buffer dies here
    return SQE_OK;
}

int index_get_field_at(sqe_index* idx, int field, const std::vector<int64_t>& pos, int64_t* values_out_host, hipStream_t s) {
    const size_t m = pos.size();
    if (m == 0) return SQE_OK;
    if (!idx->fields || !idx->fields->col[field].p) {
        for (size_t j = 0; j < m; ++j) values_out_host[j] = FIELD_NONE;
        return SQE_OK;
    }
    DevBuf tmp;
    SQE_TRY(tmp.ensure(m * 16));
    SQE_HIP(hipMemcpyAsync(tmp.p, pos.data(), m * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(field_gather_kernel, dim3(grid_of((int64_t)m, 256)), dim3(256), 0, s, idx->fields->col[field].as<int64_t>(),
                       tmp.as<int64_t>(), tmp.as<int64_t>() + m, (int64_t)m);
    SQE_HIP(hipGetLastError());
    SQE_HIP(hipMemcpyAsync(values_out_host, tmp.as<int64_t>() + m, m * 8, hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));
    return SQE_OK;
}

void index_field_info(sqe_index* idx, int* n_fields, int64_t* bytes) {
    *n_fields = 0;
    *bytes = 0;
    if (!idx->fields) return;
    for (int f = 0; f < FIELD_MAX; ++f)
        if (idx->fields->col[f].p) {
            ++*n_fields;
            *bytes += (int64_t)idx->fields->col[f].bytes;
        }
}

int index_match_fields_impl(sqe_index* idx, const FieldPreds& pr, int64_t cap, int64_t* count_dev, int64_t* id_dev, hipStream_t s) {
    const int P = pr.n_preds;
    if (P == 0) return SQE_OK;
    const int64_t n = idx->n.load();
    if (n == 0) {
        SQE_HIP(hipMemsetAsync(count_dev, 0, (size_t)P * 8, s));
        return fill(id_dev, (int64_t)P * cap, -1, s);
    }
    FieldState* st = field_state(idx);
    if (!st) return fail(SQE_ERR_OOM, "sqe_index_match_fields: host allocation failed");
    const MapLayout L(n);
    SQE_TRY(st->bits.ensure((size_t)P * L.words * 4));
    SQE_TRY(st->counts.ensure((size_t)P * L.cstride));
    if (cap > 0) SQE_TRY(st->pos.ensure((size_t)n * 8));
    uint32_t* bits = st->bits.as<uint32_t>();
    char* counts = st->counts.as<char>();
    {
        StageTimer t(idx->ctx->prof, s, ST_SCAN);
        SQE_TRY(fields_eval(idx, st, pr, L, bits, false, s));
    }
    StageTimer t(idx->ctx->prof, s, ST_SELECT);
    const int64_t* map = idx->has_map ? idx->idmap.as<int64_t>() : nullptr;
    for (int j = 0; j < P; ++j) {
        char* cj = counts + (size_t)j * L.cstride;
        int64_t* offs = reinterpret_cast<int64_t*>(cj + L.offs_off);
        int64_t* total = reinterpret_cast<int64_t*>(cj + L.total_off);
        const uint32_t* bj = bits + (size_t)j * L.words;
        SQE_TRY(launch_bitmap_count(bj, L.nb, reinterpret_cast<int*>(cj), offs, total, s));
        if (cap > 0) {
            // the list of one predicate at a time: the lowest `cap` of it leave as ids before the next one overwrites it
            SQE_TRY(launch_bitmap_write(bj, L.nb, offs, st->pos.as<int64_t>(), s));
            hipLaunchKernelGGL(field_emit_kernel, dim3(grid_of(cap, 256)), dim3(256), 0, s, st->pos.as<int64_t>(), total, cap, map,
                               idx->id_base, id_dev + (size_t)j * cap);
        }
    }
    hipLaunchKernelGGL(field_totals_kernel, dim3(1), dim3(64), 0, s, counts, L.cstride, L.total_off, P, count_dev);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

// The route of a sqe_index_search_where call that selects M of n live rows: the depth of the mask route's first stage
// (where_mask.hip), or 0 for the gather route.  "where_route" 1: always gather; 2: mask whenever the index is FLAT, at the depth
// of the rule (fieldpred.h: where_depth; "where_mask_depth" overrides it) or 256 where the rule has none; 0: mask only where
// the answer's bits cannot depend on it ("certify"), the rule has a depth, M >= "where_mask_min_rows" and the cost rule
// (where_mask_cheaper) expects the whole-index search at that depth to be cheaper than gathering M rows.
static int where_mask_plan(const sqe_index* idx, int B, int k, int64_t M, int64_t n) {
    if (idx->ivf || idx->where_route == 1 || n > (int64_t)UINT32_MAX) return 0;
    const int rule = where_depth(k, M, n);
    const int d = idx->where_mask_depth > 0 ? std::max(idx->where_mask_depth, k) : rule;
    if (idx->where_route == 2) return d > 0 ? d : WHERE_MAX_DEPTH;
    if (!idx->certify || rule == 0 || M < idx->where_mask_min_rows) return 0;
    // whether a plain search of depth d takes the int8 first pass (search.hip: admit_i8, but for the quality of the copy)
    const bool i8 = idx->scan_mode == SQE_SCAN_INT8_RESCORE && idx->dim >= 256 && idx->dim % 128 == 0 && d <= idx->i8_sample_m &&
                    n >= idx->i8_min_rows;
    return where_mask_cheaper(n, M, B, k, d, i8) ? d : 0;
}

int index_search_where_impl(sqe_index* idx, const float* q_dev, int B, int k, const RowSet& set, float* cos_out_dev, int64_t* id_out_dev,
                            hipStream_t s, bool as_positions) {
    const int64_t n = idx->n.load();
    if (n == 0 || set.n_allow == 0) {
        idx->where_last = sqe_where_last_t{};
        idx->where_last.live = n;
        return launch_pad_hits(cos_out_dev, id_out_dev, nullptr, (int64_t)B * k, s);
    }
    // the count comes back (the one synchronisation of the gather route), then the route: the gather route's launches and their
    // order are what index_search_bitmap runs; the mask route leaves the position list it wrote unused
    FilterState* f;
    int64_t words, M = 0;
    SQE_TRY(rowset_map(idx, set, &f, &words, s));
    SQE_TRY(rowset_positions(idx, set, f, words, &M, s));
    sqe_where_last_t last{};
    last.selected = M;
    last.live = n;
    const int d = M > 0 ? where_mask_plan(idx, B, k, M, n) : 0;
    if (d > 0) {
        last.route = SQE_WHERE_ROUTE_MASK;
        last.depth = d;
        SQE_TRY(index_search_where_mask(idx, filter_bitmap(f), d, q_dev, B, k, cos_out_dev, id_out_dev, &last.swept, s, as_positions));
        last.first_pass_i8 = idx->last_i8 ? 1 : 0;
    } else {
        last.route = M > 0 ? SQE_WHERE_ROUTE_GATHER : SQE_WHERE_ROUTE_NONE;
        SQE_TRY(index_search_gathered(idx, f, M, q_dev, B, k, cos_out_dev, id_out_dev, s, as_positions));
    }
    idx->where_last = last;
    if (set.allow_on_host) SQE_HIP(hipStreamSynchronize(s));     // the host list is not retained past return
    return SQE_OK;
}

int index_search_where_each_impl(sqe_index* idx, const float* q_dev, int B, int k, const FieldPreds& pr, const int32_t* pred_of_query,
                                 float* cos_out_dev, int64_t* id_out_dev, hipStream_t s) {
    if (B <= 0) return SQE_OK;
    const int P = pr.n_preds;
    const int64_t n = idx->n.load();
    FieldState* st = field_state(idx);
    if (!st) return fail(SQE_ERR_OOM, "sqe_index_search_where_each: host allocation failed");
    std::vector<int64_t> offsets((size_t)P + 1, 0), totals((size_t)P, 0);
    const MapLayout L(n);
    if (n > 0) {
        SQE_TRY(st->bits.ensure((size_t)P * L.words * 4));
        SQE_TRY(st->counts.ensure((size_t)P * L.cstride));
        SQE_TRY(st->totals.ensure((size_t)P * 8));
        {
            StageTimer t(idx->ctx->prof, s, ST_PREP);
            SQE_TRY(fields_eval(idx, st, pr, L, st->bits.as<uint32_t>(), false, s));
            for (int j = 0; j < P; ++j) {
                char* cj = st->counts.as<char>() + (size_t)j * L.cstride;
                SQE_TRY(launch_bitmap_count(st->bits.as<uint32_t>() + (size_t)j * L.words, L.nb, reinterpret_cast<int*>(cj),
                                            reinterpret_cast<int64_t*>(cj + L.offs_off), reinterpret_cast<int64_t*>(cj + L.total_off), s));
            }
            hipLaunchKernelGGL(field_totals_kernel, dim3(1), dim3(64), 0, s, st->counts.as<char>(), L.cstride, L.total_off, P,
                               st->totals.as<int64_t>());
            SQE_HIP(hipGetLastError());
            SQE_HIP(hipMemcpyAsync(totals.data(), st->totals.p, (size_t)P * 8, hipMemcpyDeviceToHost, s));
        }
        SQE_HIP(hipStreamSynchronize(s));                    // the one read-back: the counts size the lists
    }
    // the lists of the predicates some query names, one after the other (a predicate nobody names gets an empty list)
    std::vector<char> named((size_t)P, 0);
    for (int b = 0; b < B; ++b) named[(size_t)pred_of_query[b]] = 1;
    for (int j = 0; j < P; ++j) offsets[(size_t)j + 1] = offsets[(size_t)j] + (named[(size_t)j] ? totals[(size_t)j] : 0);
    const int64_t sum = offsets[(size_t)P];
    SQE_TRY(st->lists.ensure((size_t)std::max<int64_t>(sum, 1) * 8));
    int64_t* lists = st->lists.as<int64_t>();
    if (sum > 0) {
        StageTimer t(idx->ctx->prof, s, ST_PREP);
        for (int j = 0; j < P; ++j) {
            if (offsets[(size_t)j + 1] == offsets[(size_t)j]) continue;
            const char* cj = st->counts.as<char>() + (size_t)j * L.cstride;
            SQE_TRY(launch_bitmap_write(st->bits.as<uint32_t>() + (size_t)j * L.words, L.nb, reinterpret_cast<const int64_t*>(cj + L.offs_off),
                                        lists + offsets[(size_t)j], s));
        }
        // positions -> the LOCAL ids the per-query filtered search resolves (it adds id_base itself at the end)
        if (idx->has_map) SQE_TRY(launch_translate_ids(lists, sum, idx->idmap.as<int64_t>(), 0, s));
    }
    return index_search_filtered_each_impl(idx, q_dev, B, k, lists, offsets.data(), P, pred_of_query, cos_out_dev, id_out_dev, s);
}

}  // namespace sqe

// ================================================================ C ABI
using namespace sqe;

// host queries in, host results out around `run` (device pointers, the index's stream)
template <typename Run>
static int where_host_call(sqe_index* idx, const float* q_host, int B, int k, float* cos_out_host, int64_t* id_out_host, Run&& run) {
    OpScope op(idx->ctx, idx->ord, true);
    FieldState* st = field_state(idx);
    if (!st) return fail(SQE_ERR_OOM, "sqe_index_search_where: host allocation failed");
    const size_t qb = round16((size_t)B * idx->dim * 4), cb = round16((size_t)B * k * 4), ib = (size_t)B * k * 8;
    SQE_TRY(st->stage.ensure(qb + cb + ib));
    float* q_dev = st->stage.as<float>();
    float* cos_dev = reinterpret_cast<float*>(st->stage.as<char>() + qb);
    int64_t* id_dev = reinterpret_cast<int64_t*>(st->stage.as<char>() + qb + cb);
    SQE_HIP(hipMemcpyAsync(q_dev, q_host, (size_t)B * idx->dim * 4, hipMemcpyHostToDevice, op.s));
    SQE_TRY(run(q_dev, cos_dev, id_dev, op.s));
    SQE_HIP(hipMemcpyAsync(cos_out_host, cos_dev, (size_t)B * k * 4, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(id_out_host, id_dev, ib, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

extern "C" {

static int field_slot_ok(const char* who, sqe_index* idx, int field) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (field < 0 || field >= FIELD_MAX) return fail(SQE_ERR_INVALID, std::string(who) + ": field slots are 0..7");
    return SQE_OK;
}

int sqe_index_set_field(sqe_index* idx, int field, const int64_t* ids_host, const int64_t* values_host, int64_t n) {
    SQE_TRY(field_slot_ok("sqe_index_set_field", idx, field));
    if (n < 0 || (n > 0 && (!ids_host || !values_host))) return fail(SQE_ERR_INVALID, "sqe_index_set_field: bad arguments");
    if (n == 0) return SQE_OK;
    if (idx->group) return group_index_set_field(idx, field, ids_host, values_host, n);
    OpScope op(idx->ctx, idx->ord, true);
    std::vector<int64_t> pos;
    SQE_TRY(index_resolve_ids(idx, ids_host, n, pos, op.s, "sqe_index_set_field"));
    return index_set_field_at(idx, field, pos, values_host, op.s);
}

int sqe_index_get_field(sqe_index* idx, int field, const int64_t* ids_host, int64_t n, int64_t* values_out_host) {
    SQE_TRY(field_slot_ok("sqe_index_get_field", idx, field));
    if (n < 0 || (n > 0 && (!ids_host || !values_out_host))) return fail(SQE_ERR_INVALID, "sqe_index_get_field: bad arguments");
    if (n == 0) return SQE_OK;
    if (idx->group) return group_index_get_field(idx, field, ids_host, n, values_out_host);
    OpScope op(idx->ctx, idx->ord, true);
    std::vector<int64_t> pos;
    SQE_TRY(index_resolve_ids(idx, ids_host, n, pos, op.s, "sqe_index_get_field"));
    return index_get_field_at(idx, field, pos, values_out_host, op.s);
}

int sqe_index_field_info(sqe_index* idx, int* n_fields_out, int64_t* device_bytes_out) {
    if (!idx || !n_fields_out || !device_bytes_out) return fail(SQE_ERR_INVALID, "sqe_index_field_info: null argument");
    if (idx->group) return group_index_field_info(idx, n_fields_out, device_bytes_out);
    std::lock_guard<std::mutex> lk(idx->ord.mu);
    index_field_info(idx, n_fields_out, device_bytes_out);
    return SQE_OK;
}

static int match_args_ok(sqe_index* idx, const FieldPreds& pr, int64_t cap, const void* counts, const void* ids) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (cap < 0) return fail(SQE_ERR_INVALID, "sqe_index_match_fields: cap < 0");
    SQE_TRY(fields_args_ok("sqe_index_match_fields", pr));
    if (pr.n_preds > 0 && (!counts || (cap > 0 && !ids))) return fail(SQE_ERR_INVALID, "sqe_index_match_fields: null buffer");
    return SQE_OK;
}

int sqe_index_match_fields(sqe_index* idx, const sqe_field_clause_t* clauses, const int64_t* pred_offsets, int n_preds,
                           const int64_t* set_values, int64_t n_set, int64_t cap, int64_t* count_out_host, int64_t* id_out_host) {
    const FieldPreds pr{clauses, pred_offsets, n_preds, set_values, n_set};
    SQE_TRY(match_args_ok(idx, pr, cap, count_out_host, id_out_host));
    if (n_preds == 0) return SQE_OK;
    if (idx->group) return group_index_match_fields(idx, pr, cap, count_out_host, id_out_host, false);
    OpScope op(idx->ctx, idx->ord, true);
    FieldState* st = field_state(idx);
    if (!st) return fail(SQE_ERR_OOM, "sqe_index_match_fields: host allocation failed");
    const size_t cb = (size_t)n_preds * 8, ib = (size_t)n_preds * cap * 8;
    SQE_TRY(st->stage.ensure(cb + ib));
    int64_t* c_dev = st->stage.as<int64_t>();
    int64_t* i_dev = c_dev + n_preds;
    SQE_TRY(index_match_fields_impl(idx, pr, cap, c_dev, i_dev, op.s));
    SQE_HIP(hipMemcpyAsync(count_out_host, c_dev, cb, hipMemcpyDeviceToHost, op.s));
    if (ib) SQE_HIP(hipMemcpyAsync(id_out_host, i_dev, ib, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_match_fields_device(sqe_index* idx, const sqe_field_clause_t* clauses, const int64_t* pred_offsets, int n_preds,
                                  const int64_t* set_values, int64_t n_set, int64_t cap, int64_t* count_out_dev, int64_t* id_out_dev) {
    const FieldPreds pr{clauses, pred_offsets, n_preds, set_values, n_set};
    SQE_TRY(match_args_ok(idx, pr, cap, count_out_dev, id_out_dev));
    if (n_preds == 0) return SQE_OK;
    if (idx->group) return group_index_match_fields(idx, pr, cap, count_out_dev, id_out_dev, true);
    OpScope op(idx->ctx, idx->ord, false);
    return index_match_fields_impl(idx, pr, cap, count_out_dev, id_out_dev, op.s);
}

static int where_args_ok(const char* who, sqe_index* idx, const void* q, int B, int k, const void* cos, const void* ids) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (B < 0 || k < 1 || k > MAX_KP) return fail(SQE_ERR_INVALID, std::string(who) + ": need B >= 0 and 1 <= k <= 256");
    if (B > 0 && (!q || !cos || !ids)) return fail(SQE_ERR_INVALID, std::string(who) + ": null buffer");
    return SQE_OK;
}

int sqe_index_search_where(sqe_index* idx, const float* q_host, int B, int k, const sqe_field_clause_t* clauses, int n_clauses,
                           const int64_t* set_values, int64_t n_set, const int64_t* allow_ids_host, int64_t n_allow, float* cos_out_host,
                           int64_t* id_out_host) {
    int64_t one[2];
    SQE_TRY(where_args_ok("sqe_index_search_where", idx, q_host, B, k, cos_out_host, id_out_host));
    SQE_TRY(rowset_args_ok("sqe_index_search_where", clauses, n_clauses, set_values, n_set, allow_ids_host, n_allow, one));
    if (B == 0) return SQE_OK;
    const RowSet set{FieldPreds{clauses, one, 1, set_values, n_set}, allow_ids_host, n_allow, true};
    if (idx->group) return group_index_search_where(idx, q_host, B, k, set, cos_out_host, id_out_host, false);
    return where_host_call(idx, q_host, B, k, cos_out_host, id_out_host, [&](const float* q, float* cos, int64_t* ids, hipStream_t s) {
        return index_search_where_impl(idx, q, B, k, set, cos, ids, s);
    });
}

int sqe_index_search_where_device(sqe_index* idx, const float* q_dev, int B, int k, const sqe_field_clause_t* clauses, int n_clauses,
                                  const int64_t* set_values, int64_t n_set, const int64_t* allow_ids_dev, int64_t n_allow, float* cos_out_dev,
                                  int64_t* id_out_dev) {
    int64_t one[2];
    SQE_TRY(where_args_ok("sqe_index_search_where", idx, q_dev, B, k, cos_out_dev, id_out_dev));
    SQE_TRY(rowset_args_ok("sqe_index_search_where", clauses, n_clauses, set_values, n_set, allow_ids_dev, n_allow, one));
    if (B == 0) return SQE_OK;
    const FieldPreds pr{clauses, one, 1, set_values, n_set};
    if (idx->group) {
        std::vector<int64_t> allow;
        SQE_TRY(rowset_allow_to_host(idx, allow_ids_dev, n_allow, allow));
        return group_index_search_where(idx, q_dev, B, k, RowSet{pr, allow.data(), n_allow, true}, cos_out_dev, id_out_dev, true);
    }
    OpScope op(idx->ctx, idx->ord, false);
    return index_search_where_impl(idx, q_dev, B, k, RowSet{pr, allow_ids_dev, n_allow, false}, cos_out_dev, id_out_dev, op.s);
}

int sqe_index_where_last(sqe_index* idx, sqe_where_last_t* out) {
    if (!idx || !out) return fail(SQE_ERR_INVALID, "sqe_index_where_last: null argument");
    if (idx->group) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_where_last: single-device indexes only");
    std::lock_guard<std::mutex> lk(idx->ord.mu);
    if (idx->where_last.live < 0) return fail(SQE_ERR_STATE, "sqe_index_where_last: no sqe_index_search_where ran on this index yet");
    *out = idx->where_last;
    return SQE_OK;
}

static int where_each_args_ok(sqe_index* idx, const void* q, int B, int k, const FieldPreds& pr, const int32_t* pred_of_query, const void* cos,
                              const void* ids) {
    SQE_TRY(where_args_ok("sqe_index_search_where_each", idx, q, B, k, cos, ids));
    SQE_TRY(fields_args_ok("sqe_index_search_where_each", pr));
    if (B > 0 && !pred_of_query) return fail(SQE_ERR_INVALID, "sqe_index_search_where_each: null pred_of_query");
    for (int b = 0; b < B; ++b)
        if (pred_of_query[b] < 0 || pred_of_query[b] >= pr.n_preds)
            return fail(SQE_ERR_INVALID, "sqe_index_search_where_each: pred_of_query[" + std::to_string(b) + "] names no predicate");
    return SQE_OK;
}

int sqe_index_search_where_each(sqe_index* idx, const float* q_host, int B, int k, const sqe_field_clause_t* clauses,
                                const int64_t* pred_offsets, int n_preds, const int64_t* set_values, int64_t n_set,
                                const int32_t* pred_of_query_host, float* cos_out_host, int64_t* id_out_host) {
    const FieldPreds pr{clauses, pred_offsets, n_preds, set_values, n_set};
    SQE_TRY(where_each_args_ok(idx, q_host, B, k, pr, pred_of_query_host, cos_out_host, id_out_host));
    if (B == 0) return SQE_OK;
    if (idx->group) return group_index_search_where_each(idx, q_host, B, k, pr, pred_of_query_host, cos_out_host, id_out_host, false);
    return where_host_call(idx, q_host, B, k, cos_out_host, id_out_host, [&](const float* q, float* cos, int64_t* ids, hipStream_t s) {
        return index_search_where_each_impl(idx, q, B, k, pr, pred_of_query_host, cos, ids, s);
    });
}

int sqe_index_search_where_each_device(sqe_index* idx, const float* q_dev, int B, int k, const sqe_field_clause_t* clauses,
                                       const int64_t* pred_offsets, int n_preds, const int64_t* set_values, int64_t n_set,
                                       const int32_t* pred_of_query_host, float* cos_out_dev, int64_t* id_out_dev) {
    const FieldPreds pr{clauses, pred_offsets, n_preds, set_values, n_set};
    SQE_TRY(where_each_args_ok(idx, q_dev, B, k, pr, pred_of_query_host, cos_out_dev, id_out_dev));
    if (B == 0) return SQE_OK;
    if (idx->group) return group_index_search_where_each(idx, q_dev, B, k, pr, pred_of_query_host, cos_out_dev, id_out_dev, true);
    OpScope op(idx->ctx, idx->ord, false);
    return index_search_where_each_impl(idx, q_dev, B, k, pr, pred_of_query_host, cos_out_dev, id_out_dev, op.s);
}

}  // extern "C"
