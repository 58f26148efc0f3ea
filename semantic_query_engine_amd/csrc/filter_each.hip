// filter_each.hip -- per-query filtered k-NN search (sqe_index_search_filtered_each): query b is answered over its own
// allow-list, list_of_query[b], in one call.
//
// A list of a few thousand rows does not need the bf16 scan, the certificate or the scratch index of filter.hip: every
// allowed row is scored directly in fp32 with the chain of rescore_row (common.h), the chain whose bits sqe_index_search
// returns, so the answer is exact by construction, with or without "certify".  Two routes, chosen per list on the host
// from the two host arrays (no read-back):
//
//   direct    a list of at most "filter_each_direct_rows" entries that at most "filter_each_direct_queries" queries name.
//     1. resolve  one launch over the entries of every direct list of the pass: id -> owner position (the id itself
//                 without an id map, a binary search of the map with one: resolve_id), then a claim in the list's own
//                 position set (id_lists.h): the first claimant of a position keeps it, a later equal one and every id
//                 that names no live row become DEAD.  Nothing waits for another workgroup.
//     2. score    one workgroup per (list, tile of 64 entries), one wave per 16 of them: the float4s of 4 rows are loaded
//                 into registers before the first use (dim <= 1024; larger dims re-read the row per query from L1/L2),
//                 then every query that names the list (read from L2; kept in registers when it is the only one) is
//                 scored against the 4 rows and make_key(s, position) goes to entry e of the query's key array (0 for a
//                 DEAD entry).  The master copy is read in place.
//     3. select   one workgroup per query: the k best of the query's keys by the block's radix select (block_select.h)
//                 (unique once repeats are gone), k places with (-inf, -1) padding, positions -> ids (idmap / id_base).
//     The key scratch of a pass is the sum over its queries of their list's length; "filter_each_key_budget" bounds it,
//     and more keys run as several passes (a list named by many queries may be split between passes: it is resolved again).
//     Everything runs on the caller's stream; the call synchronises nothing itself and reads nothing back.  The planning
//     tables of a pass reach the device by one copy from pageable host memory (as lambda_host of the MMR search): the
//     runtime may finish that copy, and with it the stream's earlier work, before it returns.
//   gathered  every other list: the queries that name it are compacted and answered by index_search_filtered_impl
//             (filter.hip), unchanged, with its one synchronisation per list.  With "certify" = 0 this route is as
//             approximate as the search it runs; with "certify" = 1 both routes return the same bits.
//
// The direct route reads master and idmap only; the owner's search state (int8 copy, candidate and fallback buffers,
// qn, i8_last) and the single-list FilterState are never touched by it.  An index that never gets this call allocates
// nothing for it.
#include <string.h>

#include <algorithm>
#include <vector>

#include "block_select.h"
#include "id_lists.h"
#include "internal.h"

namespace sqe {

struct FilterEachState {
    DevBuf qn;        // [B, dim] fp32 normalised queries (its own: idx->qn belongs to sqe_index_search)
    DevBuf meta;      // a pass's EachList | EachQuery | EachTile tables
    DevBuf csr;       // i32 [B] queries ordered by list
    DevBuf pos;       // u32 [entries of the pass] resolved positions
    DevBuf tab;       // u32 claim tables of the pass
    DevBuf keys;      // u64 [keys of the pass]
    DevBuf gq;        // gathered route: [nq, dim] compacted raw queries
    DevBuf gout;      // gathered route: cos [nq, k] (16-B rounded) | ids [nq, k]
    DevBuf hq, hallow, hout;   // staging of the host entry point
};

namespace {

constexpr uint32_t DEAD = POS_SET_EMPTY;   // no position: a dead id or a repeat
constexpr int TILE = 64;                   // entries per score workgroup (16 per wave)
constexpr int ROWS = 4;                    // rows in flight per wave

struct EachList {
    int64_t entry_off;     // first entry in the caller's id array
    int64_t pos_off;       // first entry in the pass's position array
    int64_t tab_off;       // first slot of the list's claim table
    int32_t len;
    uint32_t tab_mask;     // table size - 1
    int32_t q0, nq;        // the pass's queries [q0, q0 + nq) name this list
};
struct EachQuery {
    int64_t key_off;       // first key in the pass's key array
    int32_t query;         // row of the call's batch
    int32_t len;           // its list's length
};
struct EachTile { int32_t list, first; };

struct EachResolveArgs {
    const int64_t* ids; const EachList* lists; const EachTile* tiles; int n_tiles;
    const int64_t* map; int64_t n; uint32_t* pos; uint32_t* tab;
};

// one wave per tile, one lane per entry
__global__ __launch_bounds__(256) void each_resolve_kernel(EachResolveArgs a) {
    const int ti = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ti >= a.n_tiles) return;
    const EachTile t = a.tiles[ti];
    const EachList L = a.lists[t.list];
    const int e = t.first + (threadIdx.x & 63);
    if (e >= L.len) return;
    const int64_t p = resolve_id(a.map, a.n, a.ids[L.entry_off + e]);
    a.pos[L.pos_off + e] = p >= 0 && pos_set_insert(a.tab + L.tab_off, L.tab_mask, (uint32_t)p) ? (uint32_t)p : DEAD;
}

struct EachScoreArgs {
    const float* master; const float* qn; int dim;
    const EachList* lists; const EachQuery* queries; const EachTile* tiles;
    const uint32_t* pos; uint64_t* keys;
};

// U = float4s per lane and row held in registers (dim <= 256 U); U == 0: any dim, rows re-read per query
template <int U>
__global__ __launch_bounds__(256) void each_score_kernel(EachScoreArgs a) {
    constexpr int UU = U > 0 ? U : 1;
    const EachTile t = a.tiles[blockIdx.x];
    const EachList L = a.lists[t.list];
    const int lane = threadIdx.x & 63;
    const int nvec = a.dim >> 2;
    const int e_end = min(min(t.first + TILE, L.len), t.first + ((int)(threadIdx.x >> 6) + 1) * (TILE / 4));
    const uint32_t* pos = a.pos + L.pos_off;
    float4 y0[UU];                                  // the list's only query stays in registers
    if (U > 0 && L.nq == 1) {
        const float4* qv = reinterpret_cast<const float4*>(a.qn) + (size_t)a.queries[L.q0].query * nvec;
#pragma unroll
        for (int u = 0; u < UU; ++u) y0[u] = u * 64 + lane < nvec ? qv[u * 64 + lane] : float4{0.f, 0.f, 0.f, 0.f};
    }
    for (int e0 = t.first + (int)(threadIdx.x >> 6) * (TILE / 4); e0 < e_end; e0 += ROWS) {
        uint32_t p[ROWS];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) p[i] = e0 + i < e_end ? pos[e0 + i] : DEAD;
        float4 r[ROWS][UU];
        if (U > 0) {
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                const float4* rv = reinterpret_cast<const float4*>(a.master) + (size_t)(p[i] != DEAD ? p[i] : 0) * nvec;
#pragma unroll
                for (int u = 0; u < UU; ++u)
                    r[i][u] = (p[i] != DEAD && u * 64 + lane < nvec) ? rv[u * 64 + lane] : float4{0.f, 0.f, 0.f, 0.f};
            }
        }
        for (int j = 0; j < L.nq; ++j) {
            const EachQuery Q = a.queries[L.q0 + j];
            const float4* qv = reinterpret_cast<const float4*>(a.qn) + (size_t)Q.query * nvec;
            float4 y[UU];
            if (U > 0) {
#pragma unroll
                for (int u = 0; u < UU; ++u) {
                    if (L.nq == 1) y[u] = y0[u];
                    else y[u] = u * 64 + lane < nvec ? qv[u * 64 + lane] : float4{0.f, 0.f, 0.f, 0.f};
                }
            }
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                float s = 0.f;
                if (U > 0) {
                    // rescore_row's chain: elements lane, lane + 64, ... in order
#pragma unroll
                    for (int u = 0; u < UU; ++u) {
                        if (u * 64 + lane < nvec) {
                            const float4 x = r[i][u], w = y[u];
                            s = fmaf(x.x, w.x, s); s = fmaf(x.y, w.y, s); s = fmaf(x.z, w.z, s); s = fmaf(x.w, w.w, s);
                        }
                    }
                    s = wave_sum(s) + 0.0f;
                } else {
                    s = p[i] != DEAD ? rescore_row(reinterpret_cast<const float4*>(a.master) + (size_t)p[i] * nvec, qv, nvec, lane) : 0.f;
                }
                if (lane == 0 && e0 + i < e_end) a.keys[Q.key_off + e0 + i] = p[i] != DEAD ? make_key(s, p[i]) : 0ull;
            }
        }
    }
}

struct EachSelectArgs {
    const EachQuery* queries; const uint64_t* keys; int k;
    float* cos_out; int64_t* id_out; const int64_t* map; int64_t id_base;
};

// One workgroup per query: the k largest of its keys (0 = no row) by the block's radix select, ranked, positions -> ids.
__global__ __launch_bounds__(256) void each_select_kernel(EachSelectArgs p) {
    __shared__ int hist[256];
    __shared__ uint64_t top[MAX_KP];
    const EachQuery Q = p.queries[blockIdx.x];
    const uint64_t* keys = p.keys + Q.key_off;
    auto visit = each_key<256>([&](int e) { return keys[e]; }, Q.len);
    const uint64_t T = Q.len > p.k ? block_select_kth<256, uint64_t, false>(visit, p.k, hist) : 0ull;
    const int m = min(block_collect_top(visit, T, top), p.k);
    block_rank_write<256>(top, m, p.k, p.cos_out + (size_t)Q.query * p.k, p.id_out + (size_t)Q.query * p.k,
                          [&](uint32_t row) { return (p.map ? p.map[row] : (int64_t)row) + p.id_base; });
}

// gathered route: dst row j = src row idx[j] (raw queries in), or dst row idx[j] = src row j (results out)
__global__ __launch_bounds__(256) void each_rows_kernel(const char* __restrict__ src, char* __restrict__ dst, const int* __restrict__ idx,
                                                        int rows, int row_bytes, int scatter) {
    const int per_row = row_bytes >> 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)rows * per_row) return;
    const int j = (int)(t / per_row), w = (int)(t - (int64_t)j * per_row);
    const size_t s_row = scatter ? (size_t)j : (size_t)idx[j], d_row = scatter ? (size_t)idx[j] : (size_t)j;
    reinterpret_cast<uint32_t*>(dst + d_row * row_bytes)[w] = reinterpret_cast<const uint32_t*>(src + s_row * row_bytes)[w];
}

FilterEachState* each_state(sqe_index* idx) {
    if (!idx->filter_each) idx->filter_each = new (std::nothrow) FilterEachState;
    return idx->filter_each;
}

// a unit of a pass: queries [q_begin, q_end) of the CSR that name list `list`
struct Unit { int list, q_begin, q_end; };

int run_direct_pass(sqe_index* idx, FilterEachState* st, const std::vector<Unit>& units, const int64_t* allow_dev,
                    const int64_t* offsets, const std::vector<int>& csr, int k, float* cos_out_dev, int64_t* id_out_dev, hipStream_t s) {
    sqe_ctx* c = idx->ctx;
    std::vector<EachList> lists;
    std::vector<EachQuery> queries;
    std::vector<EachTile> tiles;
    int64_t n_pos = 0, n_tab = 0, n_keys = 0;
    for (const Unit& u : units) {
        const int64_t len = offsets[u.list + 1] - offsets[u.list];
        const int64_t tab = pos_set_slots(len);
        if (tab > POS_SET_MAX_SLOTS) return fail(SQE_ERR_INVALID, "sqe_index_search_filtered_each: a list of more than 2^31 entries");
        EachList L;
        L.entry_off = offsets[u.list]; L.pos_off = n_pos; L.tab_off = n_tab; L.len = (int32_t)len; L.tab_mask = (uint32_t)(tab - 1);
        L.q0 = (int32_t)queries.size(); L.nq = u.q_end - u.q_begin;
        for (int j = u.q_begin; j < u.q_end; ++j) {
            queries.push_back({n_keys, csr[(size_t)j], (int32_t)len});
            n_keys += len;
        }
        for (int64_t e = 0; e < len; e += TILE) tiles.push_back({(int32_t)lists.size(), (int32_t)e});
        lists.push_back(L);
        n_pos += len;
        n_tab += tab;
    }
    const size_t lb = round16(lists.size() * sizeof(EachList)), qb = round16(queries.size() * sizeof(EachQuery)),
                 tb = round16(tiles.size() * sizeof(EachTile));
    std::vector<char> host(lb + qb + tb);
    memcpy(host.data(), lists.data(), lists.size() * sizeof(EachList));
    memcpy(host.data() + lb, queries.data(), queries.size() * sizeof(EachQuery));
    if (!tiles.empty()) memcpy(host.data() + lb + qb, tiles.data(), tiles.size() * sizeof(EachTile));
    SQE_TRY(st->meta.ensure(host.size()));
    SQE_TRY(st->pos.ensure((size_t)std::max<int64_t>(n_pos, 1) * 4));
    SQE_TRY(st->tab.ensure((size_t)n_tab * 4));
    SQE_TRY(st->keys.ensure((size_t)std::max<int64_t>(n_keys, 1) * 8));
    // the tables are host memory: the copy is staged before the call returns, and nothing is read back
    SQE_HIP(hipMemcpyAsync(st->meta.p, host.data(), host.size(), hipMemcpyHostToDevice, s));
    const EachList* d_lists = st->meta.as<EachList>();
    const EachQuery* d_queries = reinterpret_cast<const EachQuery*>(st->meta.as<char>() + lb);
    const EachTile* d_tiles = reinterpret_cast<const EachTile*>(st->meta.as<char>() + lb + qb);
    const int n_tiles = (int)tiles.size();
    const int64_t* map = idx->has_map ? idx->idmap.as<int64_t>() : nullptr;
    if (n_tiles > 0) {
        {
            StageTimer t(c->prof, s, ST_PREP);
            SQE_HIP(hipMemsetAsync(st->tab.p, 0xFF, (size_t)n_tab * 4, s));
            EachResolveArgs a{allow_dev, d_lists, d_tiles, n_tiles, map, idx->n.load(), st->pos.as<uint32_t>(), st->tab.as<uint32_t>()};
            hipLaunchKernelGGL(each_resolve_kernel, dim3(grid_of(n_tiles, 4)), dim3(256), 0, s, a);
            SQE_HIP(hipGetLastError());
        }
        {
            StageTimer t(c->prof, s, ST_SCAN);
            EachScoreArgs a{idx->master, st->qn.as<float>(), idx->dim, d_lists, d_queries, d_tiles, st->pos.as<uint32_t>(), st->keys.as<uint64_t>()};
            const int nvec = idx->dim >> 2;
            const dim3 grid((unsigned)n_tiles), block(256);
            if (nvec <= 64) hipLaunchKernelGGL(each_score_kernel<1>, grid, block, 0, s, a);
            else if (nvec <= 128) hipLaunchKernelGGL(each_score_kernel<2>, grid, block, 0, s, a);
            else if (nvec <= 192) hipLaunchKernelGGL(each_score_kernel<3>, grid, block, 0, s, a);
            else if (nvec <= 256) hipLaunchKernelGGL(each_score_kernel<4>, grid, block, 0, s, a);
            else hipLaunchKernelGGL(each_score_kernel<0>, grid, block, 0, s, a);
            SQE_HIP(hipGetLastError());
        }
    }
    {
        StageTimer t(c->prof, s, ST_SELECT);
        EachSelectArgs a{d_queries, st->keys.as<uint64_t>(), k, cos_out_dev, id_out_dev, map, idx->id_base};
        hipLaunchKernelGGL(each_select_kernel, dim3((unsigned)queries.size()), dim3(256), 0, s, a);
        SQE_HIP(hipGetLastError());
    }
    return SQE_OK;
}

}  // namespace

void filter_each_destroy(FilterEachState* f) { delete f; }

int launch_each_rows(const void* src, void* dst, const int* idx, int rows, int row_bytes, int scatter, hipStream_t s) {
    hipLaunchKernelGGL(each_rows_kernel, dim3(grid_of((int64_t)rows * (row_bytes >> 2), 256)), dim3(256), 0, s,
                       reinterpret_cast<const char*>(src), reinterpret_cast<char*>(dst), idx, rows, row_bytes, scatter);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

// Caller holds the index lock and has validated the host arrays; everything runs on stream s.  allow_dev: the ids of all
// lists on the device; offsets [n_lists + 1] and list_of_query [B] on the host; outputs [B, k] on the device.
int index_search_filtered_each_impl(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* allow_dev, const int64_t* offsets,
                                    int n_lists, const int32_t* list_of_query, float* cos_out_dev, int64_t* id_out_dev, hipStream_t s) {
    if (B <= 0) return SQE_OK;
    if (idx->dim % 4 != 0) return fail(SQE_ERR_INVALID, "sqe_index_search_filtered_each: dim must be a multiple of 4");
    FilterEachState* st = each_state(idx);
    if (!st) return fail(SQE_ERR_OOM, "sqe_index_search_filtered_each: host allocation failed");
    sqe_ctx* c = idx->ctx;
    const int K = idx->dim;
    // queries by list (counting sort keeps the batch order inside a list)
    std::vector<int> q_off((size_t)n_lists + 1, 0), csr((size_t)B);
    for (int b = 0; b < B; ++b) q_off[(size_t)list_of_query[b] + 1]++;
    for (int f = 0; f < n_lists; ++f) q_off[(size_t)f + 1] += q_off[(size_t)f];
    {
        std::vector<int> fill(q_off.begin(), q_off.end() - 1);
        for (int b = 0; b < B; ++b) csr[(size_t)fill[(size_t)list_of_query[b]]++] = b;
    }
    std::vector<int> direct, gathered;
    for (int f = 0; f < n_lists; ++f) {
        const int nq = q_off[(size_t)f + 1] - q_off[(size_t)f];
        if (nq == 0) continue;
        const int64_t len = offsets[f + 1] - offsets[f];
        (len <= idx->filter_each_direct_rows && nq <= idx->filter_each_direct_queries ? direct : gathered).push_back(f);
    }
    // ---- direct route
    if (!direct.empty()) {
        SQE_TRY(st->qn.ensure((size_t)B * K * 4));
        {
            StageTimer t(c->prof, s, ST_PREP);
            SQE_TRY(launch_normalize_rows(q_dev, B, K, K, st->qn.as<float>(), nullptr, K, nullptr, nullptr, s));
        }
        const int64_t budget = idx->filter_each_key_budget;
        std::vector<Unit> units;
        size_t li = 0;
        int taken = 0;                         // queries of list direct[li] that earlier passes answered
        while (li < direct.size()) {
            units.clear();
            int64_t keys = 0;
            while (li < direct.size()) {
                const int f = direct[li];
                const int64_t len = offsets[f + 1] - offsets[f];
                const int left = q_off[(size_t)f + 1] - q_off[(size_t)f] - taken;
                int64_t fit = len == 0 ? left : (budget - keys) / len;
                if (fit <= 0) {
                    if (!units.empty()) break;
                    fit = 1;                   // one query's keys are the least a pass holds
                }
                const int take = (int)std::min<int64_t>(left, fit);
                units.push_back({f, q_off[(size_t)f] + taken, q_off[(size_t)f] + taken + take});
                keys += (int64_t)take * len;
                taken += take;
                if (taken < q_off[(size_t)f + 1] - q_off[(size_t)f]) break;     // the pass is full
                ++li;
                taken = 0;
            }
            SQE_TRY(run_direct_pass(idx, st, units, allow_dev, offsets, csr, k, cos_out_dev, id_out_dev, s));
        }
        c->search_calls++;
    }
    // ---- gathered route: one filtered search per list over its compacted queries
    if (!gathered.empty()) {
        SQE_TRY(st->csr.ensure((size_t)B * 4));
        SQE_HIP(hipMemcpyAsync(st->csr.p, csr.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
        for (int f : gathered) {
            const int nq = q_off[(size_t)f + 1] - q_off[(size_t)f];
            const int* qidx = st->csr.as<int>() + q_off[(size_t)f];
            const size_t cb = round16((size_t)nq * k * 4);
            SQE_TRY(st->gq.ensure((size_t)nq * K * 4));
            SQE_TRY(st->gout.ensure(cb + (size_t)nq * k * 8));
            float* gcos = st->gout.as<float>();
            int64_t* gids = reinterpret_cast<int64_t*>(st->gout.as<char>() + cb);
            SQE_TRY(launch_each_rows(q_dev, st->gq.p, qidx, nq, K * 4, 0, s));
            SQE_TRY(index_search_filtered_impl(idx, st->gq.as<float>(), nq, k, allow_dev + offsets[f], offsets[f + 1] - offsets[f], gcos, gids, s));
            SQE_TRY(launch_each_rows(gcos, cos_out_dev, qidx, nq, k * 4, 1, s));
            SQE_TRY(launch_each_rows(gids, id_out_dev, qidx, nq, k * 8, 1, s));
        }
    }
    return SQE_OK;
}

// the same with host ids, staged in the state's own buffer; synchronises s before it returns (allow_host is not retained)
int index_search_filtered_each_host_ids(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* allow_host, const int64_t* offsets,
                                        int n_lists, const int32_t* list_of_query, float* cos_out_dev, int64_t* id_out_dev, hipStream_t s) {
    FilterEachState* st = each_state(idx);
    if (!st) return fail(SQE_ERR_OOM, "sqe_index_search_filtered_each: host allocation failed");
    const int64_t* allow_dev;
    SQE_TRY(stage_host_ids(st->hallow, allow_host, n_lists > 0 ? offsets[n_lists] : 0, s, &allow_dev));
    SQE_TRY(index_search_filtered_each_impl(idx, q_dev, B, k, allow_dev, offsets, n_lists, list_of_query, cos_out_dev, id_out_dev, s));
    SQE_HIP(hipStreamSynchronize(s));
    return SQE_OK;
}

}  // namespace sqe

// ================================================================ C ABI
using namespace sqe;

extern "C" {

static int each_args_ok(sqe_index* idx, const void* q, int B, int k, const void* allow, const int64_t* offsets, int n_lists,
                        const int32_t* list_of_query, const void* cos, const void* ids) {
    return list_args_ok("sqe_index_search_filtered_each: ", "allow_ids", 0, idx, q, B, k, allow, offsets, n_lists, list_of_query, cos, ids);
}

int sqe_index_search_filtered_each(sqe_index* idx, const float* q_host, int B, int k, const int64_t* allow_ids_host,
                                   const int64_t* list_offsets_host, int n_lists, const int32_t* list_of_query_host, float* cos_out_host,
                                   int64_t* id_out_host) {
    SQE_TRY(each_args_ok(idx, q_host, B, k, allow_ids_host, list_offsets_host, n_lists, list_of_query_host, cos_out_host, id_out_host));
    if (B == 0) return SQE_OK;
    if (idx->group)
        return group_index_search_filtered_each(idx, q_host, B, k, allow_ids_host, list_offsets_host, n_lists, list_of_query_host,
                                                cos_out_host, id_out_host, false);
    OpScope op(idx->ctx, idx->ord, true);
    FilterEachState* st = each_state(idx);
    if (!st) return fail(SQE_ERR_OOM, "sqe_index_search_filtered_each: host allocation failed");
    const size_t qbytes = (size_t)B * idx->dim * 4, cb = (size_t)B * k * 4, ib = (size_t)B * k * 8;
    SQE_TRY(st->hq.ensure(qbytes));
    SQE_TRY(st->hout.ensure(round16(cb) + ib));
    float* cos_dev = st->hout.as<float>();
    int64_t* id_dev = reinterpret_cast<int64_t*>(st->hout.as<char>() + round16(cb));
    SQE_HIP(hipMemcpyAsync(st->hq.p, q_host, qbytes, hipMemcpyHostToDevice, op.s));
    SQE_TRY(index_search_filtered_each_host_ids(idx, st->hq.as<float>(), B, k, allow_ids_host, list_offsets_host, n_lists, list_of_query_host,
                                                cos_dev, id_dev, op.s));
    SQE_HIP(hipMemcpyAsync(cos_out_host, cos_dev, cb, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(id_out_host, id_dev, ib, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_search_filtered_each_device(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* allow_ids_dev,
                                          const int64_t* list_offsets_host, int n_lists, const int32_t* list_of_query_host, float* cos_out_dev,
                                          int64_t* id_out_dev) {
    SQE_TRY(each_args_ok(idx, q_dev, B, k, allow_ids_dev, list_offsets_host, n_lists, list_of_query_host, cos_out_dev, id_out_dev));
    if (B == 0) return SQE_OK;
    if (idx->group) {
        std::vector<int64_t> allow;              // the shards are planned on the host
        SQE_TRY(list_ids_to_host(idx->ctx, allow_ids_dev, list_offsets_host, n_lists, allow));
        return group_index_search_filtered_each(idx, q_dev, B, k, allow.data(), list_offsets_host, n_lists, list_of_query_host, cos_out_dev,
                                                id_out_dev, true);
    }
    OpScope op(idx->ctx, idx->ord, false);
    return index_search_filtered_each_impl(idx, q_dev, B, k, allow_ids_dev, list_offsets_host, n_lists, list_of_query_host, cos_out_dev,
                                           id_out_dev, op.s);
}

}  // extern "C"
