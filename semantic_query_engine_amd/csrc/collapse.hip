// collapse.hip -- group keys (sqe_index_set_keys / get_keys) and collapsed k-NN search (sqe_index_search_collapsed): per query
// the k best GROUPS of the exact ranking and each group's best row.  A row's group is its int64 key; a row without a key
// (SQE_KEY_NONE) is a group by itself.  Walking the exact ranking (fp32 cosine descending, ties to the lowest id) and keeping
// the first row of every key gives the answer; the two stages below compute exactly that.
//
//   Stage A (FLAT indexes): the unchanged certified search at depth k' ("collapse_depth", automatic min(256, max(64, 4 k)))
//     into scratch of this file, then collapse_walk_kernel (one wave per query) walks the k' hits in order, reads each hit's
//     key by position, keeps the first hit of every key and writes the first k.  A query that found fewer than k groups
//     although the index holds more than k' rows is flagged incomplete.
//   Stage B (the incomplete queries; every query of an IVF index): sweep.hip's sweep over all live rows (sweep_flagged: the
//     compaction of the flags, the one read-back of their number, the walk over row ranges), which computes a query's whole
//     answer from nothing.  Per slot a running list of at most k (cosine, position, key) entries -- the caller's output rows
//     -- and a threshold, the list's k-th cosine (-inf while it holds fewer than k groups).  The keys a range collected
//     at threshold - eps are re-scored in fp32 by common.h's rescore_row (the chain of the search: same bits), reduced
//     to the best row per key together with the running list and the best k groups written back
//     (collapse_merge_kernel).  The maximum over a group is associative and a row that is dropped lies strictly below k
//     groups that are each represented by a row at least as good, so ranges may come in any order and size.  The threshold
//     is recomputed on the device after every range and only rises.  Memory is bounded by "range_key_budget" as for radial
//     search (slots per sweep = budget / 4096).
//   Positions -> ids through the index's id map, then id_base.
// The owner's search state is left as a plain search of depth k' leaves it; stage B reads the rows, the keys and the
// residual maximum and writes only buffers of this file and the caller's outputs.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "deny_kernels.h"
#include "internal.h"

namespace sqe {

constexpr int COLLAPSE_CAP = EXACT_CAP;        // keys per slot and collect launch: the collect scan's buffer stride
constexpr int CMERGE_THREADS = 512;
constexpr int CMERGE_SLOTS = 8192;             // power of two >= COLLAPSE_CAP + MAX_KP
constexpr int CMERGE_PER_THREAD = CMERGE_SLOTS / CMERGE_THREADS;
constexpr int CMERGE_LDS = CMERGE_SLOTS * 16;  // int64 group keys | u64 rank keys
constexpr int64_t KEY_NONE = SQE_KEY_NONE;
static_assert(COLLAPSE_CAP + MAX_KP <= CMERGE_SLOTS, "merge buffer");

struct CollapseState {
    DevBuf stage;      // host entry points: queries and results
    DevBuf hits;       // stage A: cos [B, k'] (16-B rounded) | positions [B, k']
    DevBuf flags;      // [B] int: the query is incomplete
    SweepBufs sw;      // stage B
};

namespace {

__global__ __launch_bounds__(256) void fill_i64_kernel(int64_t* __restrict__ p, int64_t n, int64_t v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

__global__ __launch_bounds__(256) void keys_scatter_kernel(int64_t* __restrict__ tab, const int64_t* __restrict__ pos,
                                                           const int64_t* __restrict__ keys, int64_t m) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < m) tab[pos[j]] = keys[j];
}

__global__ __launch_bounds__(256) void keys_gather_kernel(const int64_t* __restrict__ tab, const int64_t* __restrict__ pos,
                                                          int64_t* __restrict__ out, int64_t m) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < m) out[j] = tab[pos[j]];
}

// The walk over ranked hits, one wave per query.  P lists ("parts": cos [B, kin] at cos_off, ids [B, kin] at id_off, keys
// [B, kin] at key_off of part p = parts + p * part_bytes), each best first with ties to its lowest id and ended by id -1.
// Lane p holds the head of list p; the wave takes the best head (cosine descending, then the lowest global id), keeps it
// unless its key was kept before, and goes on until k rows are kept or every list is spent.
//   stage A: P = 1, by_pos: an id is position + id_sub and its key is keytab[position] (null keytab: no row has a key); the
//            position is written, and flags[q] = fewer than k groups were found although the index holds more than kin rows.
//   device groups: id l of part p is global id l * P + p; id_add (id_base) is added on output.
//   restricted search (within.hip): D = DenyBitmap; a by_pos head whose row D denies is passed over as if it were not listed.
template <typename D>
struct WalkArgs {
    const char* parts;
    int64_t part_bytes;
    size_t cos_off, id_off, key_off;
    int P, kin, k;
    int by_pos;
    const int64_t* keytab;
    int64_t id_sub, id_add, n_rows;
    float* cos_out;
    int64_t* id_out;
    int64_t* key_out;
    int* flags;
    [[no_unique_address]] D deny;      // last and without an address of its own: DenyNone leaves the layout as it was
};

__device__ __forceinline__ int64_t shfl_i64(int64_t v, int src) {
    const int lo = __shfl((int)(uint32_t)(uint64_t)v, src, 64);
    const int hi = __shfl((int)(uint32_t)((uint64_t)v >> 32), src, 64);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

template <typename D>
__global__ __launch_bounds__(64) void collapse_walk_kernel(WalkArgs<D> a) {
    __shared__ int64_t kept[MAX_KP];
    const int q = blockIdx.x, lane = threadIdx.x;
    const bool active = lane < a.P;
    const typename D::Probe probe = a.deny.of(q);
    const char* part = a.parts + (active ? lane : 0) * a.part_bytes;
    const float* c = reinterpret_cast<const float*>(part + a.cos_off) + (size_t)q * a.kin;
    const int64_t* d = reinterpret_cast<const int64_t*>(part + a.id_off) + (size_t)q * a.kin;
    const int64_t* gk = reinterpret_cast<const int64_t*>(part + a.key_off) + (size_t)q * a.kin;
    int h = 0, found = 0;
    bool valid = false;
    float hc = -INFINITY;
    int64_t hg = 0, hkey = KEY_NONE;
    auto load_head = [&]() {
        valid = false;
        while (active && h < a.kin) {
            const int64_t id = d[h];
            if (id < 0) break;
            if (a.by_pos && probe.denied((uint32_t)(id - a.id_sub))) {      // outside the row set: the next entry of the list
                ++h;
                continue;
            }
            valid = true;
            hc = c[h];
            if (a.by_pos) {
                hg = id - a.id_sub;
                hkey = a.keytab ? a.keytab[hg] : KEY_NONE;
            } else {
                hg = id * a.P + lane;
                hkey = gk[h];
            }
            break;
        }
    };
    load_head();
    while (found < a.k) {
        // the best head of the wave
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
        if (!bv) break;
        const int64_t wkey = shfl_i64(hkey, bl);
        bool dup = false;
        if (wkey != KEY_NONE)
            for (int j = lane; j < found; j += 64) dup |= kept[j] == wkey;
        dup = __any(dup);
        if (!dup) {
            if (lane == 0) {
                const size_t o = (size_t)q * a.k + found;
                a.cos_out[o] = bc;
                a.id_out[o] = bg + a.id_add;
                a.key_out[o] = wkey;
                kept[found] = wkey;
            }
            ++found;
        }
        __syncthreads();
        if (lane == bl) {
            ++h;
            load_head();
        }
    }
    for (int j = found + lane; j < a.k; j += 64) {
        const size_t o = (size_t)q * a.k + j;
        a.cos_out[o] = -INFINITY;
        a.id_out[o] = -1;
        a.key_out[o] = KEY_NONE;
    }
    if (a.flags && lane == 0) a.flags[q] = (found < a.k && (int64_t)a.kin < a.n_rows) ? 1 : 0;
}

template <typename D>
struct CMergeArgs {
    const float* master;       // [n, K] fp32 rows
    const float* qn;           // [pass] normalised queries
    int K;
    const int* qidx;           // slot -> query of the pass
    const uint64_t* keys;      // [G, COLLAPSE_CAP] collected keys, rows relative to row_off
    const int* key_cnt;        // [G], none above COLLAPSE_CAP (the host checked)
    int64_t row_off;
    int k;
    const int64_t* keytab;     // group key by position; null: no row has a key
    const float* q_resid;      // [pass]
    const uint32_t* resid_max;
    float* thr;                // [G] collect threshold of the next range
    float* kth;                // [G]
    int* lcnt;                 // [G]
    float* cos_out;            // [pass, k] running lists, best first
    int64_t* pos_out;
    int64_t* key_out;
    [[no_unique_address]] D deny;      // rows dropped before the per-key reduction (DenyNone: none, and the layout as it was)
};

// (group key, rank key) order of the first sort: real entries before pads (rank key 0), then by group key, inside a group the
// best rank key first
__device__ __forceinline__ bool cm_before(int64_t ga, uint64_t ra, int64_t gb, uint64_t rb) {
    if (ra == 0ull || rb == 0ull) return ra != 0ull && rb == 0ull;
    if (ga != gb) return ga < gb;
    return ra > rb;
}

template <typename D>
__global__ __launch_bounds__(CMERGE_THREADS) void collapse_merge_kernel(CMergeArgs<D> a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    __shared__ int s_n, s_h;
    int64_t* gk = reinterpret_cast<int64_t*>(lds);     // [CMERGE_SLOTS] group keys; later the heads' rank keys
    uint64_t* rk = lds + CMERGE_SLOTS;                  // [CMERGE_SLOTS] rank keys make_key(cosine, position)
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.key_cnt[i];
    const int q = a.qidx[i];
    const float t = a.kth[i];
    const int nr = a.lcnt[i];
    const typename D::Probe probe = a.deny.of(q);
    float* co = a.cos_out + (size_t)q * a.k;
    int64_t* po = a.pos_out + (size_t)q * a.k;
    int64_t* ko = a.key_out + (size_t)q * a.k;
    if (tid == 0) { s_n = 0; s_h = 0; }
    for (int j = tid; j < nr; j += CMERGE_THREADS) {
        gk[j] = ko[j];
        rk[j] = make_key(co[j], (uint32_t)po[j]);
    }
    __syncthreads();
    // fp32 re-score, one wave per row; a row below the k-th cosine of the running list cannot enter it
    const float4* qv = reinterpret_cast<const float4*>(a.qn + (size_t)q * a.K);
    const int nvec = a.K >> 2;
    const uint64_t* keys = a.keys + (size_t)i * COLLAPSE_CAP;
    for (int e = wave; e < n; e += CMERGE_THREADS / 64) {
        const int64_t row = a.row_off + key_row(keys[e]);
        const float4* rv = reinterpret_cast<const float4*>(a.master + (size_t)row * a.K);
        // the row's bit: one dword by lane 0, issued ahead of the re-score it does not depend on
        const bool denied = lane == 0 && probe.denied((uint32_t)row);
        const float s = rescore_row(rv, qv, nvec, lane);
        if (lane == 0 && s >= t && !denied) {
            const int slot = nr + atomicAdd(&s_n, 1);
            gk[slot] = a.keytab ? a.keytab[row] : KEY_NONE;
            rk[slot] = make_key(s, (uint32_t)row);
        }
    }
    __syncthreads();
    const int T = nr + s_n;
    if (s_n == 0) return;                       // nothing new: list and thresholds stand
    int p2 = 1;
    while (p2 < T) p2 <<= 1;
    for (int e = T + tid; e < p2; e += CMERGE_THREADS) { gk[e] = 0; rk[e] = 0ull; }
    __syncthreads();
    for (int size = 2; size <= p2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = tid; e < (p2 >> 1); e += CMERGE_THREADS) {
                const int lo = 2 * e - (e & (stride - 1)), hi = lo + stride;
                const bool fwd = (lo & size) == 0;
                const int64_t gx = gk[lo], gy = gk[hi];
                const uint64_t rx = rk[lo], ry = rk[hi];
                if (cm_before(gy, ry, gx, rx) == fwd) { gk[lo] = gy; gk[hi] = gx; rk[lo] = ry; rk[hi] = rx; }
            }
            __syncthreads();
        }
    }
    // the first entry of every key (every entry without a key) is its group's best row
    uint64_t mine[CMERGE_PER_THREAD];
#pragma unroll
    for (int u = 0; u < CMERGE_PER_THREAD; ++u) {
        const int e = tid + u * CMERGE_THREADS;
        mine[u] = 0ull;
        if (e < T) {
            const int64_t g = gk[e];
            if (g == KEY_NONE || e == 0 || gk[e - 1] != g) mine[u] = rk[e];
        }
    }
    __syncthreads();
    uint64_t* hk = lds;
#pragma unroll
    for (int u = 0; u < CMERGE_PER_THREAD; ++u)
        if (mine[u] != 0ull) hk[atomicAdd(&s_h, 1)] = mine[u];
    __syncthreads();
    const int H = s_h;
    p2 = 1;
    while (p2 < H) p2 <<= 1;
    for (int e = H + tid; e < p2; e += CMERGE_THREADS) hk[e] = 0ull;
    __syncthreads();
    for (int size = 2; size <= p2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = tid; e < (p2 >> 1); e += CMERGE_THREADS) {
                const int lo = 2 * e - (e & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const uint64_t x = hk[lo], y = hk[hi];
                if ((x < y) == desc) { hk[lo] = y; hk[hi] = x; }
            }
            __syncthreads();
        }
    }
    const int keep = min(H, a.k);
    for (int j = tid; j < keep; j += CMERGE_THREADS) {
        const uint64_t x = hk[j];
        const uint32_t row = key_row(x);
        co[j] = key_score(x);
        po[j] = row;
        ko[j] = a.keytab ? a.keytab[row] : KEY_NONE;
    }
    if (tid == 0) {
        a.lcnt[i] = keep;
        if (H >= a.k) {
            const float kc = key_score(hk[a.k - 1]);
            a.kth[i] = kc;
            a.thr[i] = nextafterf(kc - scan_eps(a.q_resid[q], __uint_as_float(*a.resid_max), a.K), -INFINITY);
        }
    }
}

CollapseState* collapse_state(sqe_index* idx) {
    if (!idx->collapse) idx->collapse = new (std::nothrow) CollapseState;
    return idx->collapse;
}

template <typename D>
int launch_walk(const WalkArgs<D>& a, int B, hipStream_t s) {
    hipLaunchKernelGGL(collapse_walk_kernel<D>, dim3(B), dim3(64), 0, s, a);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

// collapse_merge_kernel over the keys a range collected for the hs slots qidx of the pass whose output rows are cos / pos / keys
template <typename D>
int launch_cmerge(sqe_index* idx, SweepBufs& b, const int* qidx, int hs, int64_t r0, int k, float* cos, int64_t* pos, int64_t* keys,
                  D deny, hipStream_t s) {
    StageTimer t(idx->ctx->prof, s, ST_SELECT);
    CMergeArgs<D> a;
    a.deny = deny;
    a.master = idx->master; a.qn = b.qn.as<float>(); a.K = idx->dim; a.qidx = qidx;
    a.keys = b.keys.as<uint64_t>(); a.key_cnt = b.key_cnt.as<int>(); a.row_off = r0; a.k = k;
    a.keytab = idx->has_keys ? idx->keys.as<int64_t>() : nullptr;
    a.q_resid = b.q_resid.as<float>(); a.resid_max = idx->resid_max.as<uint32_t>();
    a.thr = b.thr.as<float>(); a.kth = b.kth.as<float>(); a.lcnt = b.lcnt.as<int>();
    a.cos_out = cos; a.pos_out = pos; a.key_out = keys;
    SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(collapse_merge_kernel<D>), CMERGE_LDS));
    hipLaunchKernelGGL(collapse_merge_kernel<D>, dim3(hs), dim3(CMERGE_THREADS), CMERGE_LDS, s, a);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

}  // namespace

int collapse_depth_of(const sqe_index* idx, int k) {
    const int d = idx->collapse_depth > 0 ? idx->collapse_depth : std::max(64, 4 * k);
    return std::min(MAX_KP, std::max(d, k));
}

void collapse_destroy(CollapseState* c) { delete c; }

int launch_keys_gather(const int64_t* tab, const int64_t* pos, int64_t* out, int64_t m, hipStream_t s) {
    if (m <= 0) return SQE_OK;
    hipLaunchKernelGGL(keys_gather_kernel, dim3(grid_of(m, 256)), dim3(256), 0, s, tab, pos, out, m);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_fill_i64(int64_t* p, int64_t n, int64_t value, hipStream_t s) {
    if (n <= 0) return SQE_OK;
    hipLaunchKernelGGL(fill_i64_kernel, dim3(grid_of(n, 256)), dim3(256), 0, s, p, n, value);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int index_ensure_keys(sqe_index* idx, hipStream_t s) {
    if (idx->has_keys) return SQE_OK;
    const int64_t cap = std::max<int64_t>(idx->cap, 1);
    SQE_TRY(idx->keys.ensure((size_t)cap * 8));
    SQE_TRY(launch_fill_i64(idx->keys.as<int64_t>(), cap, KEY_NONE, s));
    idx->has_keys = true;
    return SQE_OK;
}

int index_set_keys_at(sqe_index* idx, const std::vector<int64_t>& pos, const int64_t* keys_host, hipStream_t s) {
    // a position that repeats keeps its last key: the scatter below then writes every position once
    std::vector<std::pair<int64_t, int64_t>> order(pos.size());
    bool any_key = false;
    for (size_t j = 0; j < pos.size(); ++j) {
        order[j] = {pos[j], (int64_t)j};
        any_key |= keys_host[j] != KEY_NONE;
    }
    if (!idx->has_keys && !any_key) return SQE_OK;          // nothing to remove
    std::sort(order.begin(), order.end());
    std::vector<int64_t> up;
    up.reserve(pos.size() * 2);
    for (size_t j = 0; j < order.size(); ++j)
        if (j + 1 == order.size() || order[j + 1].first != order[j].first) up.push_back(order[j].first);
    const size_t m = up.size();
    for (size_t j = 0; j < order.size(); ++j)
        if (j + 1 == order.size() || order[j + 1].first != order[j].first) up.push_back(keys_host[order[j].second]);
    SQE_TRY(index_ensure_keys(idx, s));
    if (m == 0) return SQE_OK;
    DevBuf tmp;
    SQE_TRY(tmp.ensure(m * 16));
    SQE_HIP(hipMemcpyAsync(tmp.p, up.data(), m * 16, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(keys_scatter_kernel, dim3(grid_of((int64_t)m, 256)), dim3(256), 0, s, idx->keys.as<int64_t>(), tmp.as<int64_t>(),
                       tmp.as<int64_t>() + m, (int64_t)m);
    SQE_HIP(hipGetLastError());
    SQE_HIP(hipStreamSynchronize(s));                       // the upload buffer dies here
    return SQE_OK;
}

int index_get_keys_at(sqe_index* idx, const std::vector<int64_t>& pos, int64_t* keys_out_host, hipStream_t s) {
    const size_t m = pos.size();
    if (m == 0) return SQE_OK;
    if (!idx->has_keys) {
        for (size_t j = 0; j < m; ++j) keys_out_host[j] = KEY_NONE;
        return SQE_OK;
    }
    DevBuf tmp;
    SQE_TRY(tmp.ensure(m * 16));
    SQE_HIP(hipMemcpyAsync(tmp.p, pos.data(), m * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(keys_gather_kernel, dim3(grid_of((int64_t)m, 256)), dim3(256), 0, s, idx->keys.as<int64_t>(), tmp.as<int64_t>(),
                       tmp.as<int64_t>() + m, (int64_t)m);
    SQE_HIP(hipGetLastError());
    SQE_HIP(hipMemcpyAsync(keys_out_host, tmp.as<int64_t>() + m, m * 8, hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));
    return SQE_OK;
}

int launch_collapse_merge_parts(const char* parts, int P, int B, int k, int64_t id_base, float* cos, int64_t* ids, int64_t* keys,
                                hipStream_t s) {
    if (B <= 0) return SQE_OK;
    const CollapsePart L = CollapsePart::of(B, k);
    WalkArgs<DenyNone> a{};
    a.parts = parts; a.part_bytes = (int64_t)L.total;
    a.cos_off = L.cos_off; a.id_off = L.id_off; a.key_off = L.key_off;
    a.P = P; a.kin = k; a.k = k; a.by_pos = 0; a.keytab = nullptr; a.id_sub = 0; a.id_add = id_base; a.n_rows = 0;
    a.cos_out = cos; a.id_out = ids; a.key_out = keys; a.flags = nullptr;
    return launch_walk(a, B, s);
}

namespace {

// The two stages under one denial policy (DenyNone: the unrestricted search); kd: the depth of stage A.
template <typename D>
int collapsed_stages(sqe_index* idx, CollapseState* c, const float* q_dev, int B, int k, int kd, D deny, float* cos_dev, int64_t* id_dev,
                     int64_t* key_dev, hipStream_t s) {
    sqe_ctx* ctx = idx->ctx;
    const int64_t n = idx->n.load();
    const int64_t* keytab = idx->has_keys ? idx->keys.as<int64_t>() : nullptr;
    const int* flags = nullptr;
    if (!idx->ivf) {
        // ---- stage A: the certified search at depth kd, then the walk over its hits
        const size_t cb = round_up((int64_t)B * kd * 4, 16);
        SQE_TRY(c->hits.ensure(cb + (size_t)B * kd * 8));
        SQE_TRY(c->flags.ensure((size_t)B * 4));
        SQE_TRY(index_search_positions(idx, q_dev, B, kd, 0, c->hits.as<float>(), reinterpret_cast<int64_t*>(c->hits.as<char>() + cb), s));
        StageTimer t(ctx->prof, s, ST_SELECT);
        WalkArgs<D> a{};
        a.deny = deny;
        a.parts = c->hits.as<char>(); a.part_bytes = 0; a.cos_off = 0; a.id_off = cb; a.key_off = 0;
        a.P = 1; a.kin = kd; a.k = k; a.by_pos = 1; a.keytab = keytab; a.id_sub = search_id_base(idx); a.id_add = 0; a.n_rows = n;
        a.cos_out = cos_dev; a.id_out = id_dev; a.key_out = key_dev; a.flags = c->flags.as<int>();
        SQE_TRY(launch_walk(a, B, s));
        flags = c->flags.as<int>();
    }
    // ---- stage B: the sweep of the incomplete queries
    return sweep_flagged(idx, c->sw, flags, q_dev, B, k, cos_dev, id_dev, key_dev, ctx->collapse_swept,
                         [&](int off, const int* qidx, int hs, int64_t r0) {
                             return launch_cmerge(idx, c->sw, qidx, hs, r0, k, cos_dev + (size_t)off * k, id_dev + (size_t)off * k,
                                                  key_dev + (size_t)off * k, deny, s);
                         },
                         s);
}

}  // namespace

// Caller holds the index lock; everything runs on stream s.  bits (within.hip; a map of the filtered search's layout over the index
// as it stands): the ranking walked is that of the rows whose bit is set, and stage A fetches `depth` rows (0: "collapse_depth").
int index_search_collapsed_impl(sqe_index* idx, const float* q_dev, int B, int k, float* cos_dev, int64_t* id_dev, int64_t* key_dev,
                                hipStream_t s, const uint32_t* bits, int depth) {
    sqe_ctx* ctx = idx->ctx;
    const int64_t n = idx->n.load();
    if (B <= 0) return SQE_OK;
    ctx->collapse_swept.store(0);
    const int64_t bk = (int64_t)B * k;
    if (n == 0) return launch_pad_hits(cos_dev, id_dev, key_dev, bk, s);
    if (n > (int64_t)UINT32_MAX) return fail(SQE_ERR_INVALID, "sqe_index_search_collapsed: more than 2^32 rows");
    CollapseState* c = collapse_state(idx);
    if (!c) return fail(SQE_ERR_OOM, "sqe_index_search_collapsed: host allocation failed");
    const int kd = depth > 0 ? std::min(MAX_KP, std::max(depth, k)) : collapse_depth_of(idx, k);
    if (bits) SQE_TRY(collapsed_stages(idx, c, q_dev, B, k, kd, DenyBitmap{bits}, cos_dev, id_dev, key_dev, s));
    else SQE_TRY(collapsed_stages(idx, c, q_dev, B, k, kd, DenyNone{}, cos_dev, id_dev, key_dev, s));
    // positions -> ids (+ id_base)
    return index_positions_to_ids(idx, id_dev, bk, s);
}

}  // namespace sqe

// ================================================================ C ABI
using namespace sqe;

extern "C" {

int sqe_index_set_keys(sqe_index* idx, const int64_t* ids_host, const int64_t* keys_host, int64_t n) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (n < 0 || (n > 0 && (!ids_host || !keys_host))) return fail(SQE_ERR_INVALID, "sqe_index_set_keys: bad arguments");
    if (n == 0) return SQE_OK;
    if (idx->group) return group_index_set_keys(idx, ids_host, keys_host, n);
    OpScope op(idx->ctx, idx->ord, true);
    std::vector<int64_t> pos;
    SQE_TRY(index_resolve_ids(idx, ids_host, n, pos, op.s, "sqe_index_set_keys"));
    return index_set_keys_at(idx, pos, keys_host, op.s);
}

int sqe_index_get_keys(sqe_index* idx, const int64_t* ids_host, int64_t n, int64_t* keys_out_host) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (n < 0 || (n > 0 && (!ids_host || !keys_out_host))) return fail(SQE_ERR_INVALID, "sqe_index_get_keys: bad arguments");
    if (n == 0) return SQE_OK;
    if (idx->group) return group_index_get_keys(idx, ids_host, n, keys_out_host);
    OpScope op(idx->ctx, idx->ord, true);
    std::vector<int64_t> pos;
    SQE_TRY(index_resolve_ids(idx, ids_host, n, pos, op.s, "sqe_index_get_keys"));
    return index_get_keys_at(idx, pos, keys_out_host, op.s);
}

}  // extern "C"

// who: the entry point's name in the messages
static int collapsed_args_ok(const char* who, sqe_index* idx, const void* q, int B, int k, const void* cos, const void* ids, const void* keys) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (B < 0 || k < 1 || k > MAX_KP) return fail(SQE_ERR_INVALID, std::string(who) + ": need B >= 0 and 1 <= k <= 256");
    if (B > 0 && (!q || !cos || !ids || !keys)) return fail(SQE_ERR_INVALID, std::string(who) + ": null buffer");
    return SQE_OK;
}

// sqe_index_search_collapsed (set == null) and sqe_index_search_collapsed_where, host form; arguments checked, B > 0.  set: a
// host list, if any
static int collapsed_host(const char* who, sqe_index* idx, const float* q_host, int B, int k, const RowSet* set, float* cos_out_host,
                          int64_t* id_out_host, int64_t* key_out_host) {
    if (idx->group) return group_index_search_collapsed(idx, q_host, B, k, cos_out_host, id_out_host, key_out_host, false, set);
    OpScope op(idx->ctx, idx->ord, true);
    CollapseState* c = collapse_state(idx);
    if (!c) return fail(SQE_ERR_OOM, std::string(who) + ": host allocation failed");
    const int64_t bk = (int64_t)B * k;
    const size_t qb = round_up((int64_t)B * idx->dim * 4, 16), cb = round_up(bk * 4, 16), ib = (size_t)bk * 8;
    SQE_TRY(c->stage.ensure(qb + cb + 2 * ib));
    char* p = c->stage.as<char>();
    float* q_dev = reinterpret_cast<float*>(p);
    float* c_dev = reinterpret_cast<float*>(p + qb);
    int64_t* i_dev = reinterpret_cast<int64_t*>(p + qb + cb);
    int64_t* k_dev = reinterpret_cast<int64_t*>(p + qb + cb + ib);
    SQE_HIP(hipMemcpyAsync(q_dev, q_host, (size_t)B * idx->dim * 4, hipMemcpyHostToDevice, op.s));
    if (set) SQE_TRY(index_search_collapsed_within(idx, q_dev, B, k, *set, c_dev, i_dev, k_dev, op.s));
    else SQE_TRY(index_search_collapsed_impl(idx, q_dev, B, k, c_dev, i_dev, k_dev, op.s));
    SQE_HIP(hipMemcpyAsync(cos_out_host, c_dev, (size_t)bk * 4, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(id_out_host, i_dev, ib, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(key_out_host, k_dev, ib, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

// the _device forms; set: a device list, if any, which a device group brings to the host first
static int collapsed_device(sqe_index* idx, const float* q_dev, int B, int k, const RowSet* set, float* cos_out_dev, int64_t* id_out_dev,
                            int64_t* key_out_dev) {
    if (idx->group && set) {
        std::vector<int64_t> allow;
        SQE_TRY(rowset_allow_to_host(idx, set->allow, set->n_allow, allow));
        const RowSet on_host{set->pr, allow.data(), set->n_allow, true};
        return group_index_search_collapsed(idx, q_dev, B, k, cos_out_dev, id_out_dev, key_out_dev, true, &on_host);
    }
    if (idx->group) return group_index_search_collapsed(idx, q_dev, B, k, cos_out_dev, id_out_dev, key_out_dev, true);
    OpScope op(idx->ctx, idx->ord, false);
    if (set) return index_search_collapsed_within(idx, q_dev, B, k, *set, cos_out_dev, id_out_dev, key_out_dev, op.s);
    return index_search_collapsed_impl(idx, q_dev, B, k, cos_out_dev, id_out_dev, key_out_dev, op.s);
}

extern "C" {

int sqe_index_search_collapsed(sqe_index* idx, const float* q_host, int B, int k, float* cos_out_host, int64_t* id_out_host,
                               int64_t* key_out_host) {
    SQE_TRY(collapsed_args_ok("sqe_index_search_collapsed", idx, q_host, B, k, cos_out_host, id_out_host, key_out_host));
    if (B == 0) return SQE_OK;
    return collapsed_host("sqe_index_search_collapsed", idx, q_host, B, k, nullptr, cos_out_host, id_out_host, key_out_host);
}

int sqe_index_search_collapsed_device(sqe_index* idx, const float* q_dev, int B, int k, float* cos_out_dev, int64_t* id_out_dev,
                                      int64_t* key_out_dev) {
    SQE_TRY(collapsed_args_ok("sqe_index_search_collapsed", idx, q_dev, B, k, cos_out_dev, id_out_dev, key_out_dev));
    if (B == 0) return SQE_OK;
    return collapsed_device(idx, q_dev, B, k, nullptr, cos_out_dev, id_out_dev, key_out_dev);
}

int sqe_index_search_collapsed_where(sqe_index* idx, const float* q_host, int B, int k, const sqe_field_clause_t* clauses, int n_clauses,
                                     const int64_t* set_values, int64_t n_set, const int64_t* allow_ids_host, int64_t n_allow,
                                     float* cos_out_host, int64_t* id_out_host, int64_t* key_out_host) {
    const char* who = "sqe_index_search_collapsed_where";
    int64_t one[2];
    SQE_TRY(collapsed_args_ok(who, idx, q_host, B, k, cos_out_host, id_out_host, key_out_host));
    SQE_TRY(rowset_args_ok(who, clauses, n_clauses, set_values, n_set, allow_ids_host, n_allow, one));
    if (B == 0) return SQE_OK;
    const RowSet set{FieldPreds{clauses, one, 1, set_values, n_set}, allow_ids_host, n_allow, true};
    return collapsed_host(who, idx, q_host, B, k, &set, cos_out_host, id_out_host, key_out_host);
}

int sqe_index_search_collapsed_where_device(sqe_index* idx, const float* q_dev, int B, int k, const sqe_field_clause_t* clauses,
                                            int n_clauses, const int64_t* set_values, int64_t n_set, const int64_t* allow_ids_dev,
                                            int64_t n_allow, float* cos_out_dev, int64_t* id_out_dev, int64_t* key_out_dev) {
    const char* who = "sqe_index_search_collapsed_where";
    int64_t one[2];
    SQE_TRY(collapsed_args_ok(who, idx, q_dev, B, k, cos_out_dev, id_out_dev, key_out_dev));
    SQE_TRY(rowset_args_ok(who, clauses, n_clauses, set_values, n_set, allow_ids_dev, n_allow, one));
    if (B == 0) return SQE_OK;
    const RowSet set{FieldPreds{clauses, one, 1, set_values, n_set}, allow_ids_dev, n_allow, false};
    return collapsed_device(idx, q_dev, B, k, &set, cos_out_dev, id_out_dev, key_out_dev);
}

}  // extern "C"
