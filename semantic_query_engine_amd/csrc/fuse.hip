// fuse.hip -- fused multi-query search (sqe_index_search_fused): G logical queries, each a group of up to 32 sub-queries, one
// ranked list per group by reciprocal rank fusion or by the best cosine.
//
// Definition (include/sqe.h has the full text).  List j of a group is what sqe_index_search(q_j, k = n) returns, in its order;
// a row's rank in a list is its 1-based place.  RRF: fused_int(x) = sum over the lists that hold x of
// llrint(2^40 w_j / (c + r_j(x))) in IEEE double arithmetic, an unsigned 64-bit integer below 2^50.  MAX: the largest cosine of
// x over the lists that hold it.  Ranking: the fused score descending, ties to the lowest id.
//
//   Stage 1: the unchanged search over all Bs sub-queries at depth n into scratch of this file (index_search_impl: ids as the
//     caller sees them; on a device group the group's plain search and merge, global ids on the leader).
//   Stage 2 (fuse_lists_kernel): one workgroup of 256 threads per logical query.
//     * Its m n (id, rank, cos, w) entries go into an open-addressing table in LDS keyed by the 64-bit id: 4096 slots for at
//       most 2048 entries (load <= 1/2), linear probing from a multiplicative hash of the whole id (large id_base and the gaps
//       deletes leave hash like any other id), a slot claimed with a 64-bit compare-and-swap (-1, the padding id, marks "empty").
//     * The slot's score grows by a 64-bit integer LDS add of the entry's term, its best cosine by an unsigned max of the
//       order-preserving integer image of the float: no floating-point accumulation exists, so no order of arrival shows.
//     * Select key of a slot = score + 1 (RRF) or image(best cosine, -0 read as +0) + 1 (MAX), 0 for an empty slot; the k-th
//       largest key comes from block_select_kth's uint64_t path (keys repeat: rows tie on a fused score all the time in RRF).
//     * The slots at or above the k-th key -- all ties at the k-th score included -- are listed, ranked by counting over
//       (key descending, id ascending) and the first k written; (-inf, -1, -inf) fills what is left.
//   LDS: ids 32 KiB + scores 32 KiB + cosines 16 KiB + survivor list 4 KiB = 84 KiB dynamic (attribute set once per device), plus
//   the 1 KiB histogram and the few words of block_select.h.
// Hybrid search (sqe_index_search_hybrid): every group has one more list, the top-n of its lexical query from a sqe_lex
// (lexical.hip), searched on the same stream into FuseState::lex_hits.  fuse_lists_kernel<true> inserts it after the vector lists
// -- the same table, the same T(w, r) with the group's lexical weight, the place in the list as the rank -- and keeps the bits of
// the row's BM25 score in one more LDS array (16 KiB: 100 KiB dynamic); a row no vector list holds reports cos = -inf, a row the
// lexical list does not hold bm25 = -inf.  RRF only.  fuse_lists_kernel<false> is the fused search's kernel unchanged.
// offsets [G + 1] and weights [Bs] are host tables, copied per call from a buffer the state owns.  Nothing is read back and
// nothing synchronises.  The search is booked under scan_ms, the fuse kernel under select_ms.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "block_select.h"
#include "internal.h"

namespace sqe {

constexpr int FUSE_THREADS = 256;
constexpr int FUSE_SLOTS = 2 * FUSE_MAX_ENTRIES;          // load <= 1/2
constexpr int FUSE_LDS = FUSE_SLOTS * (8 + 8 + 4) + FUSE_MAX_ENTRIES * 2;
constexpr int FUSE_LDS_LEX = FUSE_LDS + FUSE_SLOTS * 4;   // hybrid: one more array, the row's lexical score
constexpr unsigned long long FUSE_EMPTY = ~0ull;          // id -1: padding, never inserted

struct FuseState {
    DevBuf stage;                  // host entry points: queries | results
    DevBuf tables;                 // offsets [G + 1] int64 | weights [Bs] fp32
    std::vector<char> tables_host; // what the last call copied from.  The _device form returns right after hipMemcpyAsync from this
                                   //   pageable vector and the next call overwrites it: that is safe because HIP has read an unpinned
                                   //   host-to-device source (into its staging buffers) before the call returns -- the property
                                   //   lambda_host of the MMR search relies on too
    DevBuf hits;                   // stage 1: cos [Bs, n] (16-B rounded) | ids [Bs, n]
    DevBuf lex_hits;               // hybrid, stage 1 of the lexical side: scores [G, n] (16-B rounded) | ids [G, n]
};

namespace {

struct FuseArgs {
    const float* cos;              // [Bs, n]
    const int64_t* ids;            // [Bs, n], -1: padding
    const int64_t* offsets;        // [G + 1]
    const float* w;                // [Bs] (RRF only)
    int n, k, mode, c;
    float* fused_out;              // [G, k]
    int64_t* id_out;
    float* cos_out;
    // hybrid (fuse_lists_kernel<true>) only: one more list per group from the lexical index
    const float* lex_sc;           // [G, n_lex] BM25 scores (> 0), best first
    const int64_t* lex_ids;        // [G, n_lex], -1: padding (at the tail only)
    const float* lex_w;            // [G]
    int n_lex;
    float* lex_out;                // [G, k]
};

__device__ __forceinline__ unsigned long long rrf_term(float w, int c_plus_r) {
    return (unsigned long long)__double2ll_rn(((double)w / (double)c_plus_r) * 0x1p40);      // exact scaling
}

// LEX = false is the kernel of the fused search as it was before the hybrid search existed (same registers, same LDS): every
// hybrid step sits under `if constexpr (LEX)`.
template <bool LEX>
__global__ __launch_bounds__(FUSE_THREADS) void fuse_lists_kernel(FuseArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fuse_lds[];
    unsigned long long* t_id = reinterpret_cast<unsigned long long*>(fuse_lds);      // [FUSE_SLOTS] id, FUSE_EMPTY
    unsigned long long* t_sc = t_id + FUSE_SLOTS;                                    // [FUSE_SLOTS] fused_int, then the select key
    uint32_t* t_cos = reinterpret_cast<uint32_t*>(t_sc + FUSE_SLOTS);                // [FUSE_SLOTS] orderable best cosine
    uint16_t* surv = reinterpret_cast<uint16_t*>(t_cos + FUSE_SLOTS);                // [FUSE_MAX_ENTRIES] slots at or above the k-th key
    uint32_t* t_lex = reinterpret_cast<uint32_t*>(surv + FUSE_MAX_ENTRIES);          // LEX: [FUSE_SLOTS] bits of the lexical score, 0: none
    __shared__ int hist[256];
    __shared__ int s_nsurv;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int64_t o0 = a.offsets[g];
    const int m = (int)(a.offsets[g + 1] - o0);
    const bool rrf = a.mode == SQE_FUSE_RRF;
    for (int s = tid; s < FUSE_SLOTS; s += FUSE_THREADS) {
        t_id[s] = FUSE_EMPTY;
        t_sc[s] = 0;
        t_cos[s] = 0;              // below the image of every float
        if constexpr (LEX) t_lex[s] = 0;
    }
    if (tid == 0) s_nsurv = 0;
    __syncthreads();
    // ---- insert: entry e = (list j, place r); consecutive threads read consecutive places of one list
    const int total = m * a.n;     // <= FUSE_MAX_ENTRIES (checked by the entry points); 0 on an empty index
    for (int e = tid; e < total; e += FUSE_THREADS) {
        const int j = e / a.n, r = e - j * a.n;           // rank = place r + 1: the search pads only at the tail of a list, so the
                                                          //   place counts the non-padding entries before it (a source with holes would not do)
        const size_t at = (size_t)(o0 + j) * a.n + r;
        const int64_t id = a.ids[at];
        if (id < 0) continue;
        const unsigned long long key = (unsigned long long)id;
        int slot = (int)((key * 0x9E3779B97F4A7C15ull) >> 52);      // top 12 bits: FUSE_SLOTS = 4096
        for (;;) {                 // at most 2048 distinct ids in 4096 slots: an empty slot is always reached
            const unsigned long long prev = atomicCAS(&t_id[slot], FUSE_EMPTY, key);
            if (prev == FUSE_EMPTY || prev == key) break;
            slot = (slot + 1) & (FUSE_SLOTS - 1);
        }
        atomicMax(&t_cos[slot], f32_orderable(a.cos[at]));
        if (rrf) atomicAdd(&t_sc[slot], rrf_term(a.w[o0 + j], a.c + r + 1));
    }
    if constexpr (LEX) {           // the lexical list: one more list of the group, at most n_lex entries (total + n_lex <= FUSE_MAX_ENTRIES)
        for (int r = tid; r < a.n_lex; r += FUSE_THREADS) {
            const size_t at = (size_t)g * a.n_lex + r;
            const int64_t id = a.lex_ids[at];
            if (id < 0) continue;
            const unsigned long long key = (unsigned long long)id;
            int slot = (int)((key * 0x9E3779B97F4A7C15ull) >> 52);
            for (;;) {
                const unsigned long long prev = atomicCAS(&t_id[slot], FUSE_EMPTY, key);
                if (prev == FUSE_EMPTY || prev == key) break;
                slot = (slot + 1) & (FUSE_SLOTS - 1);
            }
            t_lex[slot] = __float_as_uint(a.lex_sc[at]);      // an id stands once in the list: one writer per slot
            atomicAdd(&t_sc[slot], rrf_term(a.lex_w[g], a.c + r + 1));
        }
    }
    __syncthreads();
    // ---- select keys: 0 = empty
    for (int s = tid; s < FUSE_SLOTS; s += FUSE_THREADS) {
        if (t_id[s] == FUSE_EMPTY) continue;
        if (rrf) {
            t_sc[s] += 1;
        } else {
            const float c = f32_from_orderable(t_cos[s]);
            t_sc[s] = (unsigned long long)f32_orderable(c == 0.f ? 0.f : c) + 1;      // compared as a float: -0 == +0
        }
    }
    __syncthreads();
    const uint64_t T = block_select_kth<FUSE_THREADS, uint64_t, false>(
        each_key<FUSE_THREADS>([&](int s) { return (uint64_t)t_sc[s]; }, FUSE_SLOTS), a.k, hist);
    for (int s = tid; s < FUSE_SLOTS; s += FUSE_THREADS) {
        const unsigned long long key = t_sc[s];
        if (key != 0 && key >= T) {
            const int at = atomicAdd(&s_nsurv, 1);
            if (at < FUSE_MAX_ENTRIES) surv[at] = (uint16_t)s;      // always: at most FUSE_MAX_ENTRIES slots are occupied
        }
    }
    __syncthreads();
    const int S = min(s_nsurv, FUSE_MAX_ENTRIES);
    float* fo = a.fused_out + (size_t)g * a.k;
    int64_t* io = a.id_out + (size_t)g * a.k;
    float* co = a.cos_out + (size_t)g * a.k;
    for (int i = tid; i < S; i += FUSE_THREADS) {
        const int si = surv[i];
        const unsigned long long ki = t_sc[si], di = t_id[si];
        int rank = 0;
        for (int j = 0; j < S; ++j) {
            const int sj = surv[j];
            const unsigned long long kj = t_sc[sj];
            rank += (kj > ki || (kj == ki && t_id[sj] < di)) ? 1 : 0;
        }
        if (rank < a.k) {
            float c = f32_from_orderable(t_cos[si]);
            if constexpr (LEX) {
                if (t_cos[si] == 0) c = -INFINITY;      // in no vector list
                a.lex_out[(size_t)g * a.k + rank] = t_lex[si] ? __uint_as_float(t_lex[si]) : -INFINITY;
            }
            fo[rank] = rrf ? (float)((double)(ki - 1) * 0x1p-40) : c;
            io[rank] = (int64_t)di;
            co[rank] = c;
        }
    }
    for (int i = min(S, a.k) + tid; i < a.k; i += FUSE_THREADS) {
        fo[i] = -INFINITY;
        io[i] = -1;
        co[i] = -INFINITY;
        if constexpr (LEX) a.lex_out[(size_t)g * a.k + i] = -INFINITY;
    }
}

FuseState* fuse_state(sqe_index* idx) {
    if (!idx->fuse) idx->fuse = new (std::nothrow) FuseState;
    return idx->fuse;
}

}  // namespace

void fuse_destroy(FuseState* f) { delete f; }

int fuse_depth_of(int k, int n, int mode) {
    if (n > 0) return n;
    return mode == SQE_FUSE_MAX ? k : std::min(FUSE_MAX_N, std::max(32, 4 * k));
}

int fuse_hits(sqe_index* idx, int Bs, int n, float** cos, int64_t** ids) {
    FuseState* f = fuse_state(idx);
    if (!f) return fail(SQE_ERR_OOM, "sqe_index_search_fused: host allocation failed");
    const size_t cnt = (size_t)Bs * n, cb = round16(cnt * 4);
    SQE_TRY(f->hits.ensure(cb + cnt * 8 + 16));
    *cos = f->hits.as<float>();
    *ids = reinterpret_cast<int64_t*>(f->hits.as<char>() + cb);
    return SQE_OK;
}

int fuse_lex_hits(sqe_index* idx, int G, int n, float** score, int64_t** ids) {
    FuseState* f = fuse_state(idx);
    if (!f) return fail(SQE_ERR_OOM, "sqe_index_search_hybrid: host allocation failed");
    const size_t cnt = (size_t)G * n, sb = round16(cnt * 4);
    SQE_TRY(f->lex_hits.ensure(sb + cnt * 8 + 16));
    *score = f->lex_hits.as<float>();
    *ids = reinterpret_cast<int64_t*>(f->lex_hits.as<char>() + sb);
    return SQE_OK;
}

int fuse_lists(sqe_index* idx, const float* cos, const int64_t* ids, int G, int Bs, const int64_t* offsets, int k, int n, int mode, int c,
               const float* weights, float* fused_dev, int64_t* id_dev, float* cos_dev, hipStream_t s, const FuseLex* lx) {
    if (G <= 0) return SQE_OK;
    FuseState* f = fuse_state(idx);
    if (!f) return fail(SQE_ERR_OOM, "sqe_index_search_fused: host allocation failed");
    // weights [Bs], and with a lexical source [Bs + G]: one more per group
    const size_t ob = (size_t)(G + 1) * 8, nw = mode == SQE_FUSE_RRF ? (size_t)Bs + (lx ? (size_t)G : 0) : 0, wb = nw * 4;
    f->tables_host.resize(ob + wb + 4);
    memcpy(f->tables_host.data(), offsets, ob);
    float* w = reinterpret_cast<float*>(f->tables_host.data() + ob);
    for (size_t j = 0; j < nw; ++j) w[j] = weights ? weights[j] : 1.f;
    SQE_TRY(f->tables.ensure(ob + wb + 4));
    SQE_HIP(hipMemcpyAsync(f->tables.p, f->tables_host.data(), ob + wb, hipMemcpyHostToDevice, s));
    StageTimer t(idx->ctx->prof, s, ST_SELECT);
    FuseArgs a;
    a.cos = cos; a.ids = ids; a.offsets = f->tables.as<int64_t>(); a.w = reinterpret_cast<const float*>(f->tables.as<char>() + ob);
    a.n = n; a.k = k; a.mode = mode; a.c = c;
    a.fused_out = fused_dev; a.id_out = id_dev; a.cos_out = cos_dev;
    a.lex_sc = nullptr; a.lex_ids = nullptr; a.lex_w = nullptr; a.n_lex = 0; a.lex_out = nullptr;
    if (lx) {
        a.lex_sc = lx->score; a.lex_ids = lx->ids; a.lex_w = a.w + Bs; a.n_lex = lx->n; a.lex_out = lx->out;
        SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(fuse_lists_kernel<true>), FUSE_LDS_LEX));
        hipLaunchKernelGGL(fuse_lists_kernel<true>, dim3(G), dim3(FUSE_THREADS), FUSE_LDS_LEX, s, a);
    } else {
        SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(fuse_lists_kernel<false>), FUSE_LDS));
        hipLaunchKernelGGL(fuse_lists_kernel<false>, dim3(G), dim3(FUSE_THREADS), FUSE_LDS, s, a);
    }
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

// Caller holds the index lock; everything runs on stream s.
int index_search_fused_impl(sqe_index* idx, const float* q_dev, int G, int Bs, const int64_t* offsets, int k, int n, int mode, int c,
                            const float* weights, int nprobe, float* fused_dev, int64_t* id_dev, float* cos_dev, hipStream_t s) {
    if (G <= 0) return SQE_OK;
    // no sub-query or no row: every list is empty, the kernel reads none (depth 0) and pads
    if (Bs == 0 || idx->n.load() == 0)
        return fuse_lists(idx, nullptr, nullptr, G, Bs, offsets, k, 0, mode, c, weights, fused_dev, id_dev, cos_dev, s);
    float* hc;
    int64_t* hi;
    SQE_TRY(fuse_hits(idx, Bs, n, &hc, &hi));
    SQE_TRY(index_search_impl(idx, q_dev, Bs, n, nprobe, hc, hi, s));
    return fuse_lists(idx, hc, hi, G, Bs, offsets, k, n, mode, c, weights, fused_dev, id_dev, cos_dev, s);
}

// Hybrid: the vector lists as above, the lexical list of every group from lex at the same depth, one fuse kernel over both.
// Caller holds the index lock (the lexical index is locked inside lex_search_on_stream) and has validated every argument.
int index_search_hybrid_impl(sqe_index* idx, sqe_lex* lex, const float* q_dev, int G, int Bs, const int64_t* offsets, const int64_t* qoff,
                             const int32_t* qterms, int k, int n, int c, const float* weights, int nprobe, float* fused_dev, int64_t* id_dev,
                             float* cos_dev, float* lex_dev, hipStream_t s) {
    if (G <= 0) return SQE_OK;
    float* ls;
    int64_t* li;
    SQE_TRY(fuse_lex_hits(idx, G, n, &ls, &li));
    SQE_TRY(lex_search_on_stream(lex, qoff, qterms, G, n, ls, li, s));
    const FuseLex lx{ls, li, n, lex_dev};
    float* hc = nullptr;
    int64_t* hi = nullptr;
    int nv = 0;                    // no sub-query or no row: the kernel reads no vector list
    if (Bs > 0 && idx->n.load() > 0) {
        SQE_TRY(fuse_hits(idx, Bs, n, &hc, &hi));
        SQE_TRY(index_search_impl(idx, q_dev, Bs, n, nprobe, hc, hi, s));
        nv = n;
    }
    return fuse_lists(idx, hc, hi, G, Bs, offsets, k, nv, SQE_FUSE_RRF, c, weights, fused_dev, id_dev, cos_dev, s, &lx);
}

}  // namespace sqe

// ================================================================ C ABI
using namespace sqe;

// everything is checked before anything is written; *n_out = the depth, *Bs_out = the number of sub-queries
static int fused_args_ok(sqe_index* idx, const void* q, int G, const int64_t* offsets, int k, int n, int mode, int c, const float* weights,
                         const void* fused, const void* ids, const void* cos, int* n_out, int* Bs_out) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (mode != SQE_FUSE_MAX && mode != SQE_FUSE_RRF) return fail(SQE_ERR_INVALID, "sqe_index_search_fused: mode must be SQE_FUSE_MAX or SQE_FUSE_RRF");
    if (G < 0 || k < 1 || k > FUSE_MAX_N) return fail(SQE_ERR_INVALID, "sqe_index_search_fused: need G >= 0 and 1 <= k <= 256");
    if (n != 0 && (n < k || n > FUSE_MAX_N)) return fail(SQE_ERR_INVALID, "sqe_index_search_fused: need n == 0 (automatic) or k <= n <= 256");
    if (mode == SQE_FUSE_MAX && weights) return fail(SQE_ERR_INVALID, "sqe_index_search_fused: weights must be NULL with SQE_FUSE_MAX");
    if (mode == SQE_FUSE_RRF && (c < 1 || c > 10000)) return fail(SQE_ERR_INVALID, "sqe_index_search_fused: rank_constant must be in [1, 10000]");
    *n_out = fuse_depth_of(k, n, mode);
    *Bs_out = 0;
    if (G == 0) return SQE_OK;
    if (!offsets || !fused || !ids || !cos) return fail(SQE_ERR_INVALID, "sqe_index_search_fused: null buffer");
    if (offsets[0] != 0) return fail(SQE_ERR_INVALID, "sqe_index_search_fused: offsets must start at 0");
    for (int g = 0; g < G; ++g) {
        const int64_t m = offsets[g + 1] - offsets[g];
        if (m < 0) return fail(SQE_ERR_INVALID, "sqe_index_search_fused: offsets must not decrease");
        if (m > FUSE_MAX_LISTS) return fail(SQE_ERR_INVALID, "sqe_index_search_fused: at most 32 sub-queries per logical query");
        if (m * *n_out > FUSE_MAX_ENTRIES) return fail(SQE_ERR_INVALID, "sqe_index_search_fused: sub-queries x depth must not exceed 2048");
    }
    const int64_t Bs = offsets[G];           // <= 32 G
    if (Bs > 0 && !q) return fail(SQE_ERR_INVALID, "sqe_index_search_fused: null buffer");
    if (weights)
        for (int64_t j = 0; j < Bs; ++j)
            if (!(weights[j] > 0.f && weights[j] <= 64.f)) return fail(SQE_ERR_INVALID, "sqe_index_search_fused: weights must be in (0, 64]");
    if (Bs > INT32_MAX) return fail(SQE_ERR_INVALID, "sqe_index_search_fused: too many sub-queries");
    *Bs_out = (int)Bs;
    return SQE_OK;
}

// the hybrid call's checks: those of the fused search in RRF mode with one more list per group, then the lexical queries'
static int hybrid_args_ok(sqe_index* idx, sqe_lex* lex, const void* q, int G, const int64_t* offsets, const int64_t* qoff, const int32_t* qterms,
                          int k, int n, int c, const float* weights, const void* fused, const void* ids, const void* cos, const void* lexo,
                          int* n_out, int* Bs_out) {
    if (!lex) return fail(SQE_ERR_INVALID, "sqe_index_search_hybrid: null lexical index");
    SQE_TRY(fused_args_ok(idx, q, G, offsets, k, n, SQE_FUSE_RRF, c, nullptr, fused, ids, cos, n_out, Bs_out));
    if (lex_ctx(lex) != idx->ctx) return fail(SQE_ERR_INVALID, "sqe_index_search_hybrid: the two indexes belong to different contexts");
    if (G == 0) return SQE_OK;
    if (!lexo) return fail(SQE_ERR_INVALID, "sqe_index_search_hybrid: null buffer");
    for (int g = 0; g < G; ++g) {
        const int64_t m = offsets[g + 1] - offsets[g];
        if (m > FUSE_MAX_LISTS - 1) return fail(SQE_ERR_INVALID, "sqe_index_search_hybrid: at most 31 vector sub-queries per group");
        if ((m + 1) * *n_out > FUSE_MAX_ENTRIES) return fail(SQE_ERR_INVALID, "sqe_index_search_hybrid: (sub-queries + 1) x depth must not exceed 2048");
    }
    if (weights)
        for (int64_t j = 0; j < (int64_t)*Bs_out + G; ++j)
            if (!(weights[j] > 0.f && weights[j] <= 64.f)) return fail(SQE_ERR_INVALID, "sqe_index_search_hybrid: weights must be in (0, 64]");
    return lex_query_check("sqe_index_search_hybrid", lex, qoff, qterms, G);
}

extern "C" {

int sqe_index_search_hybrid(sqe_index* idx, sqe_lex* lex, const float* q_host, int G, const int64_t* offsets_host, const int64_t* qoffsets_host,
                            const int32_t* qterms_host, int k, int n, int rank_constant, const float* weights_host, int nprobe,
                            float* fused_out_host, int64_t* id_out_host, float* cos_out_host, float* lex_out_host) {
    int Bs = 0;
    SQE_TRY(hybrid_args_ok(idx, lex, q_host, G, offsets_host, qoffsets_host, qterms_host, k, n, rank_constant, weights_host, fused_out_host,
                           id_out_host, cos_out_host, lex_out_host, &n, &Bs));
    if (G == 0) return SQE_OK;
    if (idx->group) {
        const GroupHybrid hy{lex, qoffsets_host, qterms_host, lex_out_host};
        return group_index_search_fused(idx, q_host, G, Bs, offsets_host, k, n, SQE_FUSE_RRF, rank_constant, weights_host, nprobe, fused_out_host,
                                        id_out_host, cos_out_host, false, &hy);
    }
    OpScope op(idx->ctx, idx->ord, true);
    FuseState* f = fuse_state(idx);
    if (!f) return fail(SQE_ERR_OOM, "sqe_index_search_hybrid: host allocation failed");
    const FusedOut O = FusedOut::of(G, k);
    const size_t qb = round16((size_t)Bs * idx->dim * 4);
    SQE_TRY(f->stage.ensure(qb + O.total + O.f32_bytes));
    char* p = f->stage.as<char>();
    float* q_dev = reinterpret_cast<float*>(p);
    char* o_dev = p + qb;
    float* lex_dev = reinterpret_cast<float*>(o_dev + O.total);
    if (Bs > 0) SQE_HIP(hipMemcpyAsync(q_dev, q_host, (size_t)Bs * idx->dim * 4, hipMemcpyHostToDevice, op.s));
    SQE_TRY(index_search_hybrid_impl(idx, lex, q_dev, G, Bs, offsets_host, qoffsets_host, qterms_host, k, n, rank_constant, weights_host, nprobe,
                                     reinterpret_cast<float*>(o_dev + O.fused_off), reinterpret_cast<int64_t*>(o_dev + O.id_off),
                                     reinterpret_cast<float*>(o_dev + O.cos_off), lex_dev, op.s));
    SQE_HIP(hipMemcpyAsync(fused_out_host, o_dev + O.fused_off, O.f32_bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(id_out_host, o_dev + O.id_off, O.id_bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(cos_out_host, o_dev + O.cos_off, O.f32_bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(lex_out_host, lex_dev, O.f32_bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_search_hybrid_device(sqe_index* idx, sqe_lex* lex, const float* q_dev, int G, const int64_t* offsets_host,
                                   const int64_t* qoffsets_host, const int32_t* qterms_host, int k, int n, int rank_constant,
                                   const float* weights_host, int nprobe, float* fused_out_dev, int64_t* id_out_dev, float* cos_out_dev,
                                   float* lex_out_dev) {
    int Bs = 0;
    SQE_TRY(hybrid_args_ok(idx, lex, q_dev, G, offsets_host, qoffsets_host, qterms_host, k, n, rank_constant, weights_host, fused_out_dev,
                           id_out_dev, cos_out_dev, lex_out_dev, &n, &Bs));
    if (G == 0) return SQE_OK;
    if (idx->group) {
        const GroupHybrid hy{lex, qoffsets_host, qterms_host, lex_out_dev};
        return group_index_search_fused(idx, q_dev, G, Bs, offsets_host, k, n, SQE_FUSE_RRF, rank_constant, weights_host, nprobe, fused_out_dev,
                                        id_out_dev, cos_out_dev, true, &hy);
    }
    OpScope op(idx->ctx, idx->ord, false);
    return index_search_hybrid_impl(idx, lex, q_dev, G, Bs, offsets_host, qoffsets_host, qterms_host, k, n, rank_constant, weights_host, nprobe,
                                    fused_out_dev, id_out_dev, cos_out_dev, lex_out_dev, op.s);
}

int sqe_index_search_fused(sqe_index* idx, const float* q_host, int G, const int64_t* offsets_host, int k, int n, int mode, int rank_constant,
                           const float* weights_host, int nprobe, float* fused_out_host, int64_t* id_out_host, float* cos_out_host) {
    int Bs = 0;
    SQE_TRY(fused_args_ok(idx, q_host, G, offsets_host, k, n, mode, rank_constant, weights_host, fused_out_host, id_out_host, cos_out_host, &n,
                          &Bs));
    if (G == 0) return SQE_OK;
    if (idx->group)
        return group_index_search_fused(idx, q_host, G, Bs, offsets_host, k, n, mode, rank_constant, weights_host, nprobe, fused_out_host,
                                        id_out_host, cos_out_host, false);
    OpScope op(idx->ctx, idx->ord, true);
    FuseState* f = fuse_state(idx);
    if (!f) return fail(SQE_ERR_OOM, "sqe_index_search_fused: host allocation failed");
    const FusedOut O = FusedOut::of(G, k);
    const size_t qb = round16((size_t)Bs * idx->dim * 4);
    SQE_TRY(f->stage.ensure(qb + O.total));
    char* p = f->stage.as<char>();
    float* q_dev = reinterpret_cast<float*>(p);
    char* o_dev = p + qb;
    if (Bs > 0) SQE_HIP(hipMemcpyAsync(q_dev, q_host, (size_t)Bs * idx->dim * 4, hipMemcpyHostToDevice, op.s));
    SQE_TRY(index_search_fused_impl(idx, q_dev, G, Bs, offsets_host, k, n, mode, rank_constant, weights_host, nprobe,
                                    reinterpret_cast<float*>(o_dev + O.fused_off), reinterpret_cast<int64_t*>(o_dev + O.id_off),
                                    reinterpret_cast<float*>(o_dev + O.cos_off), op.s));
    SQE_HIP(hipMemcpyAsync(fused_out_host, o_dev + O.fused_off, O.f32_bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(id_out_host, o_dev + O.id_off, O.id_bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(cos_out_host, o_dev + O.cos_off, O.f32_bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_search_fused_device(sqe_index* idx, const float* q_dev, int G, const int64_t* offsets_host, int k, int n, int mode,
                                  int rank_constant, const float* weights_host, int nprobe, float* fused_out_dev, int64_t* id_out_dev,
                                  float* cos_out_dev) {
    int Bs = 0;
    SQE_TRY(fused_args_ok(idx, q_dev, G, offsets_host, k, n, mode, rank_constant, weights_host, fused_out_dev, id_out_dev, cos_out_dev, &n, &Bs));
    if (G == 0) return SQE_OK;
    if (idx->group)
        return group_index_search_fused(idx, q_dev, G, Bs, offsets_host, k, n, mode, rank_constant, weights_host, nprobe, fused_out_dev,
                                        id_out_dev, cos_out_dev, true);
    OpScope op(idx->ctx, idx->ord, false);
    return index_search_fused_impl(idx, q_dev, G, Bs, offsets_host, k, n, mode, rank_constant, weights_host, nprobe, fused_out_dev, id_out_dev,
                                   cos_out_dev, op.s);
}

}  // extern "C"
