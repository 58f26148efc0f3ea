// mmr.hip -- MMR k-NN search (sqe_index_search_mmr): per query a greedy, diversified choice of k rows among the exact top-n.
//
// Definition (include/sqe.h has the full text).  The candidates are what sqe_index_search(q, k = n) returns, in its order:
// cosines c_0 >= c_1 >= ..., ties to the lowest id.  s(i, j) is the fp32 dot product of the stored master rows of candidates
// i and j.  With pen = 0 at the start, step t picks the not yet chosen candidate with the largest
// obj(i) = lam c_i - (1 - lam) pen(i) (fp32, ties to the lower rank) and then sets pen(j) = s(j, i) at t = 0, else
// max(pen(j), s(j, i)).
//
//   Stage A: the unchanged search over row positions at depth n into scratch of this file (index_search_positions).
//   Gram stage (mmr_gram_kernel, the hot path): per query G = R R^T over its n candidate rows in fp32 on
//     v_mfma_f32_32x32x2_f32, whose result is bit for bit a k-ordered fmaf chain.  A workgroup of four waves owns one 64 x 64
//     tile of the upper triangle of G (tiles ti <= tj: the select stage reads G[min][max] only), a wave one 32 x 32 quarter; a
//     diagonal tile loads its 64 rows once for both operands and leaves out the quarter below the diagonal.
//     Rows are read through an index table (base pointer + element offset per candidate, -1 = no row: zeros), so the same
//     kernel reads the master copy on a single device and the gathered parts on a group leader.  K runs in slices of 32
//     through LDS: 16-byte global loads (8 lanes cover the 128 bytes of a row's slice), stored k-major at a row stride of 65
//     dwords.  Stores: the 32 lanes of a group write banks (4 c + e + r) mod 32 over c < 8, r < 4: all distinct.  Operand
//     reads: lane l reads [k0 + (l >> 5)][row0 + (l & 31)], 32 consecutive dwords per half wave: conflict-free ds_read_b32.
//     The next slice's global loads are in flight while the MFMAs of this one run.  Element (i, j) is ALWAYS the chain over
//     k = 0 .. dim-1 in that order, whatever the batch, the pass or the tile it falls in.
//   Select stage (mmr_select_kernel): one wave per query, lane l owns candidates l, l + 64, ...; k steps of a wave arg-max
//     (ties to the lower rank) and a max-update from the chosen row of G; writes the three outputs and maps positions to
//     ids (id map, then id_base).
// Batches run in passes of "mmr_row_budget" / n queries (mmr_pass_queries), which bounds the scratch: per pass query
// n (n + 5) 4 bytes.  Nothing is read back and nothing synchronises.  Both stages are booked under select_ms.
// Device groups: group.hip's MMR kind calls index_mmr_candidates_impl on every shard and mmr_merge_parts on the leader.
#include <math.h>

#include <algorithm>
#include <new>

#include "internal.h"

namespace sqe {

constexpr int GRAM_TILE = 64;          // rows / columns of G per workgroup
constexpr int GRAM_KS = 32;            // k per LDS slice
constexpr int GRAM_LDS_STRIDE = 65;    // dwords between k-rows of a slice (GRAM_TILE + 1: see the bank note above)
constexpr int MMR_PER_LANE = MMR_MAX_N / 64;

struct MmrState {
    DevBuf stage;      // host entry points: queries | weights | results
    DevBuf lam;        // device entry point: [B] weights
    DevBuf hits;       // per pass: cos [bp, n] (16-B rounded) | ids [bp, n] (16-B rounded) | row offsets [bp, n]
    DevBuf gram;       // per pass: [bp, n, n] fp32, upper triangle
};

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void mmr_pad_kernel(float* __restrict__ cos, int64_t* __restrict__ ids, float* __restrict__ mmr,
                                                      int64_t count) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < count) {
        cos[j] = -INFINITY;
        ids[j] = -1;
        if (mmr) mmr[j] = -INFINITY;
    }
}

// single device: the index table of a pass from the positions of its hits (id - id_sub; -1: no candidate)
__global__ __launch_bounds__(256) void mmr_table_kernel(const int64_t* __restrict__ ids, int64_t count, int64_t id_sub, int dim,
                                                        int64_t* __restrict__ roff) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= count) return;
    const int64_t id = ids[j];
    roff[j] = id >= 0 ? (id - id_sub) * dim : -1;
}

// a shard of a device group: the master rows of its hits (by position) into its part; one workgroup per hit
__global__ __launch_bounds__(64) void mmr_gather_kernel(const float* __restrict__ master, const int64_t* __restrict__ ids, int64_t id_sub,
                                                        int dim, float* __restrict__ rows) {
    const int64_t j = blockIdx.x;
    const int64_t id = ids[j];
    if (id < 0) return;
    const float4* src = reinterpret_cast<const float4*>(master + (size_t)(id - id_sub) * dim);
    float4* dst = reinterpret_cast<float4*>(rows + (size_t)j * dim);
    for (int v = threadIdx.x; v < dim / 4; v += 64) dst[v] = src[v];
}

__device__ __forceinline__ int64_t shfl_i64(int64_t v, int src) {
    const int lo = __shfl((int)(uint32_t)(uint64_t)v, src, 64);
    const int hi = __shfl((int)(uint32_t)((uint64_t)v >> 32), src, 64);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// Group leader, one wave per query: the P lists of the parts (each best first, ties to its lowest id, ended by id -1) into
// the global top-n.  Lane p holds the head of list p; the wave takes the best head (cosine descending, then the lowest
// global id l P + p) n times.  Written: the cosine, the global id (without id_base) and where the row lies in the gather
// buffer (element offset from its start); (-inf, -1, -1) once every list is spent.
struct MergeArgs {
    const char* parts;
    int64_t part_bytes;
    size_t cos_off, id_off, row_off;
    int P, n, dim;
    float* cos;
    int64_t* ids;
    int64_t* roff;
};

__global__ __launch_bounds__(64) void mmr_merge_kernel(MergeArgs a) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const bool active = lane < a.P;
    const char* part = a.parts + (active ? lane : 0) * a.part_bytes;
    const float* c = reinterpret_cast<const float*>(part + a.cos_off) + (size_t)q * a.n;
    const int64_t* d = reinterpret_cast<const int64_t*>(part + a.id_off) + (size_t)q * a.n;
    int h = 0;
    bool valid = false;
    float hc = -INFINITY;
    int64_t hg = 0;
    auto load_head = [&]() {
        valid = false;
        if (active && h < a.n) {
            const int64_t id = d[h];
            if (id >= 0) {
                valid = true;
                hc = c[h];
                hg = id * a.P + lane;
            }
        }
    };
    load_head();
    for (int t = 0; t < a.n; ++t) {
        bool bv = valid;
        float bc = hc;
        int64_t bg = hg;
        int bl = lane;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const bool ov = __shfl_xor((int)bv, off, 64) != 0;
            const float oc = __shfl_xor(bc, off, 64);
            const int ol = __shfl_xor(bl, off, 64);
            const int64_t og = shfl_i64(bg, (lane ^ off));
            const bool take = ov && (!bv || oc > bc || (oc == bc && (og < bg || (og == bg && ol < bl))));
            if (take) { bv = ov; bc = oc; bg = og; bl = ol; }
        }
        const size_t o = (size_t)q * a.n + t;
        if (!bv) {                        // every list is spent: the same for all lanes
            if (lane == 0) { a.cos[o] = -INFINITY; a.ids[o] = -1; a.roff[o] = -1; }
            continue;
        }
        if (lane == bl) {
            a.cos[o] = bc;
            a.ids[o] = bg;
            a.roff[o] = (int64_t)lane * (a.part_bytes / 4) + (int64_t)(a.row_off / 4) + ((int64_t)q * a.n + h) * a.dim;
            ++h;
            load_head();
        }
    }
}

// G = R R^T of one query per blockIdx.y, one upper-triangle tile pair per blockIdx.x (see the head of the file).
struct GramArgs {
    const float* base;         // rows lie at base + roff[...]
    const int64_t* roff;       // [B, n] element offsets, -1: no row (reads as zeros)
    float* G;                  // [B, n, n]
    int n, dim, tiles;         // tiles = ceil(n / 64)
};

__global__ __launch_bounds__(256) void mmr_gram_kernel(GramArgs a) {
    __shared__ float lds[2][GRAM_KS * GRAM_LDS_STRIDE];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int ti = 0, rem = blockIdx.x;
    while (rem >= a.tiles - ti) { rem -= a.tiles - ti; ++ti; }
    const int tj = ti + rem;
    const int wi = wave >> 1, wj = wave & 1;
    const bool diag = ti == tj;                  // both operands are the same 64 rows: one copy in LDS serves as A and as B
    // loads: this thread brings float4 c of rows lr and lr + 32 of both tiles
    const int lr = tid >> 3, c = tid & 7;
    const int64_t* ro = a.roff + (size_t)b * a.n;
    const float* pa[2];
    const float* pb[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int ra = ti * GRAM_TILE + lr + 32 * u, rb = tj * GRAM_TILE + lr + 32 * u;
        const int64_t oa = ra < a.n ? ro[ra] : -1, ob = rb < a.n ? ro[rb] : -1;
        pa[u] = oa >= 0 ? a.base + oa + 4 * c : nullptr;
        pb[u] = ob >= 0 && !diag ? a.base + ob + 4 * c : nullptr;
    }
    float4 va[2], vb[2] = {};
    auto gload = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            va[u] = pa[u] ? *reinterpret_cast<const float4*>(pa[u] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (!diag) vb[u] = pb[u] ? *reinterpret_cast<const float4*>(pb[u] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto sstore = [&]() {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = lr + 32 * u;
            float* da = &lds[0][(4 * c) * GRAM_LDS_STRIDE + r];
            float* db = &lds[1][(4 * c) * GRAM_LDS_STRIDE + r];
            da[0] = va[u].x; da[GRAM_LDS_STRIDE] = va[u].y; da[2 * GRAM_LDS_STRIDE] = va[u].z; da[3 * GRAM_LDS_STRIDE] = va[u].w;
            if (!diag) { db[0] = vb[u].x; db[GRAM_LDS_STRIDE] = vb[u].y; db[2 * GRAM_LDS_STRIDE] = vb[u].z; db[3 * GRAM_LDS_STRIDE] = vb[u].w; }
        }
    };
    // a wave whose quarter lies wholly past n, or below the diagonal (never read), only helps with the loads
    const int row0 = ti * GRAM_TILE + wi * 32, col0 = tj * GRAM_TILE + wj * 32;
    const bool live = row0 < a.n && col0 < a.n && row0 <= col0;
    const float* la = &lds[0][(lane >> 5) * GRAM_LDS_STRIDE + wi * 32 + (lane & 31)];
    const float* lb = &lds[diag ? 0 : 1][(lane >> 5) * GRAM_LDS_STRIDE + wj * 32 + (lane & 31)];
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    gload(0);
    for (int k0 = 0; k0 < a.dim; k0 += GRAM_KS) {
        sstore();
        __syncthreads();
        if (k0 + GRAM_KS < a.dim) gload(k0 + GRAM_KS);
        if (live) {
#pragma unroll
            for (int kk = 0; kk < GRAM_KS; kk += 2)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(la[kk * GRAM_LDS_STRIDE], lb[kk * GRAM_LDS_STRIDE], acc, 0, 0, 0);
        }
        __syncthreads();
    }
    if (!live) return;
    const int col = col0 + (lane & 31);
    if (col >= a.n) return;
    float* g = a.G + (size_t)b * a.n * a.n;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < a.n) g[(size_t)row * a.n + col] = acc[r];
    }
}

// The greedy choice, one wave per query (see the head of the file).  ids [B, n] are positions + id_sub (single device) or
// global ids (group leader: id_sub = 0, no map); output id = (map ? map[id - id_sub] : id - id_sub) + id_add.
struct SelectArgs {
    const float* cos;          // [B, n]
    const int64_t* ids;        // [B, n], -1: no candidate
    const float* G;            // [B, n, n], upper triangle valid
    const float* lam;          // [B]
    int n, k;
    const int64_t* map;
    int64_t id_sub, id_add;
    float* cos_out;
    int64_t* id_out;
    float* mmr_out;
};

__global__ __launch_bounds__(64) void mmr_select_kernel(SelectArgs a) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const float* cq = a.cos + (size_t)q * a.n;
    const int64_t* dq = a.ids + (size_t)q * a.n;
    const float* g = a.G + (size_t)q * a.n * a.n;
    const float lam = a.lam[q], oml = __fsub_rn(1.f, lam);
    float c[MMR_PER_LANE], pen[MMR_PER_LANE];
    bool valid[MMR_PER_LANE], avail[MMR_PER_LANE];
#pragma unroll
    for (int u = 0; u < MMR_PER_LANE; ++u) {
        const int j = lane + 64 * u;
        valid[u] = j < a.n && dq[j] >= 0;
        c[u] = valid[u] ? cq[j] : 0.f;
        pen[u] = 0.f;
        avail[u] = valid[u];
    }
    constexpr int NONE = 0x7fffffff;
    int found = 0;
    for (int t = 0; t < a.k; ++t) {
        float bo = -INFINITY;
        int bj = NONE;
#pragma unroll
        for (int u = 0; u < MMR_PER_LANE; ++u) {
            if (!avail[u]) continue;
            const float o = __fsub_rn(__fmul_rn(lam, c[u]), __fmul_rn(oml, pen[u]));
            if (bj == NONE || o > bo) { bo = o; bj = lane + 64 * u; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float oo = __shfl_xor(bo, off, 64);
            const int oj = __shfl_xor(bj, off, 64);
            if (oj != NONE && (bj == NONE || oo > bo || (oo == bo && oj < bj))) { bo = oo; bj = oj; }
        }
        if (bj == NONE) break;
        if (lane == 0) {
            const size_t o = (size_t)q * a.k + t;
            const int64_t p = dq[bj] - a.id_sub;
            a.cos_out[o] = cq[bj];
            a.id_out[o] = (a.map ? a.map[p] : p) + a.id_add;
            a.mmr_out[o] = bo;
        }
        ++found;
#pragma unroll
        for (int u = 0; u < MMR_PER_LANE; ++u) {
            const int j = lane + 64 * u;
            if (j == bj) avail[u] = false;
            if (valid[u]) {
                const float s = g[(size_t)min(j, bj) * a.n + max(j, bj)];
                pen[u] = t == 0 ? s : fmaxf(pen[u], s);
            }
        }
    }
    for (int j = found + lane; j < a.k; j += 64) {
        const size_t o = (size_t)q * a.k + j;
        a.cos_out[o] = -INFINITY;
        a.id_out[o] = -1;
        a.mmr_out[o] = -INFINITY;
    }
}

MmrState* mmr_state(sqe_index* idx) {
    if (!idx->mmr) idx->mmr = new (std::nothrow) MmrState;
    return idx->mmr;
}

// the per-pass scratch: cos | ids | row offsets of bp queries at depth n, and their Gram products
struct PassBufs {
    float* cos;
    int64_t* ids;
    int64_t* roff;
    float* gram;
};

int pass_bufs(MmrState* m, int bp, int n, PassBufs* out) {
    const size_t cnt = (size_t)bp * n, cb = round16(cnt * 4), ib = round16(cnt * 8);
    SQE_TRY(m->hits.ensure(cb + 2 * ib));
    SQE_TRY(m->gram.ensure(cnt * n * 4));
    char* p = m->hits.as<char>();
    out->cos = reinterpret_cast<float*>(p);
    out->ids = reinterpret_cast<int64_t*>(p + cb);
    out->roff = reinterpret_cast<int64_t*>(p + cb + ib);
    out->gram = m->gram.as<float>();
    return SQE_OK;
}

// Gram + select of bs queries whose candidates (cos, ids, row offsets from `base`) are in `pb`
int gram_and_select(sqe_ctx* ctx, const float* base, const PassBufs& pb, int bs, int n, int k, int dim, const float* lam_dev,
                    const int64_t* map, int64_t id_sub, int64_t id_add, float* cos_dev, int64_t* id_dev, float* mmr_dev, hipStream_t s) {
    StageTimer t(ctx->prof, s, ST_SELECT);
    GramArgs ga;
    ga.base = base; ga.roff = pb.roff; ga.G = pb.gram; ga.n = n; ga.dim = dim; ga.tiles = (n + GRAM_TILE - 1) / GRAM_TILE;
    hipLaunchKernelGGL(mmr_gram_kernel, dim3(ga.tiles * (ga.tiles + 1) / 2, bs), dim3(256), 0, s, ga);
    SQE_HIP(hipGetLastError());
    SelectArgs sa;
    sa.cos = pb.cos; sa.ids = pb.ids; sa.G = pb.gram; sa.lam = lam_dev; sa.n = n; sa.k = k;
    sa.map = map; sa.id_sub = id_sub; sa.id_add = id_add;
    sa.cos_out = cos_dev; sa.id_out = id_dev; sa.mmr_out = mmr_dev;
    hipLaunchKernelGGL(mmr_select_kernel, dim3(bs), dim3(64), 0, s, sa);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_pad(float* cos, int64_t* ids, float* mmr, int64_t count, hipStream_t s) {
    if (count <= 0) return SQE_OK;
    hipLaunchKernelGGL(mmr_pad_kernel, dim3(grid_of(count, 256)), dim3(256), 0, s, cos, ids, mmr, count);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

}  // namespace

void mmr_destroy(MmrState* m) { delete m; }

int mmr_depth_of(int k, int n_cand) { return n_cand > 0 ? n_cand : std::min(MMR_MAX_N, std::max(32, 4 * k)); }

int mmr_pass_queries(int64_t row_budget, int n, int P) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(1 << 20, row_budget / ((int64_t)n * P)));
}

// Caller holds the index lock; everything runs on stream s.
// set (within.hip): the candidates are the exact top-n of that row set, sqe_index_search_where at depth n (no nprobe); it
// synchronises s once per pass, and once more per pass for a host allow-list.
int index_search_mmr_impl(sqe_index* idx, const float* q_dev, int B, int k, int n, const float* lam_dev, int nprobe, float* cos_dev,
                          int64_t* id_dev, float* mmr_dev, hipStream_t s, const RowSet* set) {
    if (B <= 0) return SQE_OK;
    if (idx->n.load() == 0) return launch_pad(cos_dev, id_dev, mmr_dev, (int64_t)B * k, s);
    MmrState* m = mmr_state(idx);
    if (!m) return fail(SQE_ERR_OOM, "sqe_index_search_mmr: host allocation failed");
    const int dim = idx->dim;
    const int bp = std::min(B, mmr_pass_queries(idx->mmr_row_budget, n, 1));
    PassBufs pb;
    SQE_TRY(pass_bufs(m, bp, n, &pb));
    for (int off = 0; off < B; off += bp) {
        const int bs = std::min(bp, B - off);
        if (set)
            SQE_TRY(index_search_where_impl(idx, q_dev + (size_t)off * dim, bs, n, *set, pb.cos, pb.ids, s, true));
        else
            SQE_TRY(index_search_positions(idx, q_dev + (size_t)off * dim, bs, n, nprobe, pb.cos, pb.ids, s));
        const int64_t id_sub = set ? 0 : search_id_base(idx);
        {
            StageTimer t(idx->ctx->prof, s, ST_SELECT);
            hipLaunchKernelGGL(mmr_table_kernel, dim3(grid_of((int64_t)bs * n, 256)), dim3(256), 0, s, pb.ids, (int64_t)bs * n, id_sub, dim,
                               pb.roff);
            SQE_HIP(hipGetLastError());
        }
        SQE_TRY(gram_and_select(idx->ctx, idx->master, pb, bs, n, k, dim, lam_dev + off, idx->has_map ? idx->idmap.as<int64_t>() : nullptr,
                                id_sub, idx->id_base, cos_dev + (size_t)off * k, id_dev + (size_t)off * k, mmr_dev + (size_t)off * k, s));
    }
    return SQE_OK;
}

int index_mmr_candidates_impl(sqe_index* idx, const float* q_dev, int B, int n, int nprobe, float* cos_dev, int64_t* id_dev,
                              float* rows_dev, hipStream_t s, const RowSet* set) {
    if (B <= 0) return SQE_OK;
    const int64_t cnt = (int64_t)B * n;
    if (idx->n.load() == 0) return launch_pad(cos_dev, id_dev, nullptr, cnt, s);
    if (set)
        SQE_TRY(index_search_where_impl(idx, q_dev, B, n, *set, cos_dev, id_dev, s, true));
    else
        SQE_TRY(index_search_positions(idx, q_dev, B, n, nprobe, cos_dev, id_dev, s));
    {
        StageTimer t(idx->ctx->prof, s, ST_SELECT);
        hipLaunchKernelGGL(mmr_gather_kernel, dim3((unsigned)cnt), dim3(64), 0, s, idx->master, id_dev, set ? 0 : search_id_base(idx), idx->dim,
                           rows_dev);
        SQE_HIP(hipGetLastError());
    }
    if (set) return index_positions_to_ids(idx, id_dev, cnt, s);
    return index_translate_ids(idx, id_dev, cnt, s);
}

int mmr_merge_parts(sqe_index* idx, const char* parts, int P, int B, int k, int n, const float* lam_dev, float* cos_dev,
                    int64_t* id_dev, float* mmr_dev, hipStream_t s) {
    if (B <= 0) return SQE_OK;
    MmrState* m = mmr_state(idx);
    if (!m) return fail(SQE_ERR_OOM, "sqe_index_search_mmr: host allocation failed");
    PassBufs pb;
    SQE_TRY(pass_bufs(m, B, n, &pb));
    const MmrPart L = MmrPart::of(B, n, idx->dim);
    {
        StageTimer t(idx->ctx->prof, s, ST_SELECT);
        MergeArgs a;
        a.parts = parts; a.part_bytes = (int64_t)L.total; a.cos_off = L.cos_off; a.id_off = L.id_off; a.row_off = L.row_off;
        a.P = P; a.n = n; a.dim = idx->dim; a.cos = pb.cos; a.ids = pb.ids; a.roff = pb.roff;
        hipLaunchKernelGGL(mmr_merge_kernel, dim3(B), dim3(64), 0, s, a);
        SQE_HIP(hipGetLastError());
    }
    return gram_and_select(idx->ctx, reinterpret_cast<const float*>(parts), pb, B, n, k, idx->dim, lam_dev, nullptr, 0, idx->id_base, cos_dev,
                           id_dev, mmr_dev, s);
}

}  // namespace sqe

// ================================================================ C ABI
using namespace sqe;

// who: the entry point's name in the messages
static int mmr_args_ok(const char* who, sqe_index* idx, const void* q, int B, int k, int n_cand, const float* lam, const void* cos,
                       const void* ids, const void* mmr) {
    const std::string w(who);
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (B < 0 || k < 1 || k > MMR_MAX_N) return fail(SQE_ERR_INVALID, w + ": need B >= 0 and 1 <= k <= 256");
    if (n_cand != 0 && (n_cand < k || n_cand > MMR_MAX_N)) return fail(SQE_ERR_INVALID, w + ": need n_cand == 0 (automatic) or k <= n_cand <= 256");
    if (B > 0 && (!q || !lam || !cos || !ids || !mmr)) return fail(SQE_ERR_INVALID, w + ": null buffer");
    for (int b = 0; b < B; ++b)
        if (!(lam[b] >= 0.f && lam[b] <= 1.f)) return fail(SQE_ERR_INVALID, w + ": lambda must be in [0, 1]");
    return SQE_OK;
}

// sqe_index_search_mmr (set == null) and sqe_index_search_mmr_where, host form; arguments checked, B > 0.  set: a host list, if any
static int mmr_host(const char* who, sqe_index* idx, const float* q_host, int B, int k, int n_cand, const float* lambda_host, int nprobe,
                    const RowSet* set, float* cos_out_host, int64_t* id_out_host, float* mmr_out_host) {
    const int n = mmr_depth_of(k, n_cand);
    if (idx->group)
        return group_index_search_mmr(idx, q_host, B, k, n, lambda_host, nprobe, cos_out_host, id_out_host, mmr_out_host, false, set);
    OpScope op(idx->ctx, idx->ord, true);
    MmrState* m = mmr_state(idx);
    if (!m) return fail(SQE_ERR_OOM, std::string(who) + ": host allocation failed");
    const MmrOut O = MmrOut::of(B, k);
    const size_t qb = round16((size_t)B * idx->dim * 4), lb = round16((size_t)B * 4);
    SQE_TRY(m->stage.ensure(qb + lb + O.total));
    char* p = m->stage.as<char>();
    float* q_dev = reinterpret_cast<float*>(p);
    float* l_dev = reinterpret_cast<float*>(p + qb);
    char* o_dev = p + qb + lb;
    float* c_dev = reinterpret_cast<float*>(o_dev + O.cos_off);
    int64_t* i_dev = reinterpret_cast<int64_t*>(o_dev + O.id_off);
    float* m_dev = reinterpret_cast<float*>(o_dev + O.mmr_off);
    SQE_HIP(hipMemcpyAsync(q_dev, q_host, (size_t)B * idx->dim * 4, hipMemcpyHostToDevice, op.s));
    SQE_HIP(hipMemcpyAsync(l_dev, lambda_host, (size_t)B * 4, hipMemcpyHostToDevice, op.s));
    if (set) SQE_TRY(index_search_mmr_within(idx, q_dev, B, k, n, l_dev, *set, c_dev, i_dev, m_dev, op.s));
    else SQE_TRY(index_search_mmr_impl(idx, q_dev, B, k, n, l_dev, nprobe, c_dev, i_dev, m_dev, op.s));
    SQE_HIP(hipMemcpyAsync(cos_out_host, c_dev, O.cos_bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(id_out_host, i_dev, O.id_bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(mmr_out_host, m_dev, O.cos_bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

// the _device forms; set: a device list, if any, which a device group brings to the host first
static int mmr_device(const char* who, sqe_index* idx, const float* q_dev, int B, int k, int n_cand, const float* lambda_host, int nprobe,
                      const RowSet* set, float* cos_out_dev, int64_t* id_out_dev, float* mmr_out_dev) {
    const int n = mmr_depth_of(k, n_cand);
    if (idx->group && set) {
        std::vector<int64_t> allow;
        SQE_TRY(rowset_allow_to_host(idx, set->allow, set->n_allow, allow));
        const RowSet on_host{set->pr, allow.data(), set->n_allow, true};
        return group_index_search_mmr(idx, q_dev, B, k, n, lambda_host, nprobe, cos_out_dev, id_out_dev, mmr_out_dev, true, &on_host);
    }
    if (idx->group) return group_index_search_mmr(idx, q_dev, B, k, n, lambda_host, nprobe, cos_out_dev, id_out_dev, mmr_out_dev, true);
    OpScope op(idx->ctx, idx->ord, false);
    MmrState* m = mmr_state(idx);
    if (!m) return fail(SQE_ERR_OOM, std::string(who) + ": host allocation failed");
    // the weights are host memory: the copy is staged before the call returns, and nothing is read back
    SQE_TRY(m->lam.ensure((size_t)B * 4));
    SQE_HIP(hipMemcpyAsync(m->lam.p, lambda_host, (size_t)B * 4, hipMemcpyHostToDevice, op.s));
    if (set) return index_search_mmr_within(idx, q_dev, B, k, n, m->lam.as<float>(), *set, cos_out_dev, id_out_dev, mmr_out_dev, op.s);
    return index_search_mmr_impl(idx, q_dev, B, k, n, m->lam.as<float>(), nprobe, cos_out_dev, id_out_dev, mmr_out_dev, op.s);
}

extern "C" {

int sqe_index_search_mmr(sqe_index* idx, const float* q_host, int B, int k, int n_cand, const float* lambda_host, int nprobe,
                         float* cos_out_host, int64_t* id_out_host, float* mmr_out_host) {
    SQE_TRY(mmr_args_ok("sqe_index_search_mmr", idx, q_host, B, k, n_cand, lambda_host, cos_out_host, id_out_host, mmr_out_host));
    if (B == 0) return SQE_OK;
    return mmr_host("sqe_index_search_mmr", idx, q_host, B, k, n_cand, lambda_host, nprobe, nullptr, cos_out_host, id_out_host, mmr_out_host);
}

int sqe_index_search_mmr_device(sqe_index* idx, const float* q_dev, int B, int k, int n_cand, const float* lambda_host, int nprobe,
                                float* cos_out_dev, int64_t* id_out_dev, float* mmr_out_dev) {
    SQE_TRY(mmr_args_ok("sqe_index_search_mmr", idx, q_dev, B, k, n_cand, lambda_host, cos_out_dev, id_out_dev, mmr_out_dev));
    if (B == 0) return SQE_OK;
    return mmr_device("sqe_index_search_mmr", idx, q_dev, B, k, n_cand, lambda_host, nprobe, nullptr, cos_out_dev, id_out_dev, mmr_out_dev);
}

int sqe_index_search_mmr_where(sqe_index* idx, const float* q_host, int B, int k, int n_cand, const float* lambda_host, int nprobe,
                               const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                               const int64_t* allow_ids_host, int64_t n_allow, float* cos_out_host, int64_t* id_out_host,
                               float* mmr_out_host) {
    const char* who = "sqe_index_search_mmr_where";
    int64_t one[2];
    SQE_TRY(mmr_args_ok(who, idx, q_host, B, k, n_cand, lambda_host, cos_out_host, id_out_host, mmr_out_host));
    SQE_TRY(rowset_args_ok(who, clauses, n_clauses, set_values, n_set, allow_ids_host, n_allow, one));
    if (B == 0) return SQE_OK;
    const RowSet set{FieldPreds{clauses, one, 1, set_values, n_set}, allow_ids_host, n_allow, true};
    return mmr_host(who, idx, q_host, B, k, n_cand, lambda_host, nprobe, &set, cos_out_host, id_out_host, mmr_out_host);
}

int sqe_index_search_mmr_where_device(sqe_index* idx, const float* q_dev, int B, int k, int n_cand, const float* lambda_host, int nprobe,
                                      const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                                      const int64_t* allow_ids_dev, int64_t n_allow, float* cos_out_dev, int64_t* id_out_dev,
                                      float* mmr_out_dev) {
    const char* who = "sqe_index_search_mmr_where";
    int64_t one[2];
    SQE_TRY(mmr_args_ok(who, idx, q_dev, B, k, n_cand, lambda_host, cos_out_dev, id_out_dev, mmr_out_dev));
    SQE_TRY(rowset_args_ok(who, clauses, n_clauses, set_values, n_set, allow_ids_dev, n_allow, one));
    if (B == 0) return SQE_OK;
    const RowSet set{FieldPreds{clauses, one, 1, set_values, n_set}, allow_ids_dev, n_allow, false};
    return mmr_device(who, idx, q_dev, B, k, n_cand, lambda_host, nprobe, &set, cos_out_dev, id_out_dev, mmr_out_dev);
}

}  // extern "C"
