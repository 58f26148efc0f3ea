// range.hip -- radial k-NN search (sqe_index_range_search): per query b, the live rows whose fp32 cosine is >= min_cos[b],
// their exact number and the best max_hits of them.
//
// The search's certificate already rests on the bound  |bf16 scan score - fp32 cosine| <= eps  (kernels.h: scan_eps).  A row
// whose cosine is >= t therefore has a scan score >= t - eps, so a bf16 collect scan with the fixed threshold t - eps gathers
// every match (and the rows of the error band), and an fp32 re-score of what it gathered decides each row exactly.
//   1. collect: the unchanged collect scan of the certified fallback (scan.hip, COLLECT mode) over the whole index, all the
//      queries of a group at once.  Its per-query buffers hold RANGE_CAP keys; the count goes on past that.
//   2. merge (range_merge_kernel, one workgroup per query): every gathered row is re-scored with the chain of the search's
//      re-score (one fmaf chain per lane over the float4 elements lane, lane + 64, ..., then wave_sum + 0.0f), so the cosine
//      is bit for bit the one sqe_index_search returns; rows with c >= t are counted, sorted in LDS and merged into the
//      query's running best-m list (ranks by binary search, ties to the lowest position).  A query whose buffer overflowed
//      is skipped here.
//   3. overflow plan: the key counts come back to the host once per group.  A query with more than RANGE_CAP candidates is
//      scanned again over row ranges by sweep.hip's walk (collect, read the counts back, halve the range if a query
//      overflowed it, else merge and go on), which starts where the first pass's count predicts 2048 keys.
//   4. positions -> ids through the index's id map, then id_base.
// Memory: one group holds range_key_budget / RANGE_CAP queries (at least 1, at most 1024), i.e. at most range_key_budget keys,
// whatever the number of matches.  Nothing else grows with the data: the running lists are the caller's output buffers.
// The owner's search buffers (candidate lists, fallback buffers, int8 state, staging) are never touched.
#include <math.h>
#include <cmath>
#include <string.h>

#include <algorithm>
#include <vector>

#include "deny_kernels.h"
#include "internal.h"

namespace sqe {

constexpr int RANGE_CAP = EXACT_CAP;        // keys per query and collect launch: the collect scan's buffer stride
constexpr int RANGE_MAX_PASS = SWEEP_MAX_PASS;
constexpr int MERGE_THREADS = 512;
constexpr int MERGE_LDS = (RANGE_CAP + RANGE_MAX_HITS) * 8;

struct RangeState {
    DevBuf stage;      // host entry points: queries, thresholds, counts and results
    SweepBufs sw;      // qb also serves the first pass: the collect scan reads the pass's query rows in place
};

namespace {

__global__ __launch_bounds__(256) void range_pad_kernel(int64_t* __restrict__ counts, int B, float* __restrict__ cos,
                                                        int64_t* __restrict__ ids, int64_t count) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < B) counts[j] = 0;
    if (j < count) {
        cos[j] = -INFINITY;
        ids[j] = -1;
    }
}

// One workgroup per slot i of the group: collect threshold min_cos - eps (one ulp lower still, +inf stays +inf), the key
// count reset, and with qidx the bf16 row of query qidx[i] copied to row i of qb_out.  Block 0 also stores the batch size.
__global__ __launch_bounds__(64) void range_prep_kernel(const float* __restrict__ min_cos, const float* __restrict__ q_resid,
                                                        const uint32_t* __restrict__ resid_max, int K, int G, const int* __restrict__ qidx,
                                                        int q0, const char* __restrict__ qb, char* __restrict__ qb_out, int pitch,
                                                        float* __restrict__ thr, int* __restrict__ key_cnt, int* __restrict__ batch) {
    const int i = blockIdx.x;
    const int q = qidx ? qidx[i] : q0 + i;
    if (threadIdx.x == 0) {
        const float t = min_cos[q];
        float v = INFINITY;
        if (t != INFINITY) v = nextafterf(t - scan_eps(q_resid[q], __uint_as_float(*resid_max), K), -INFINITY);
        thr[i] = v;
        key_cnt[i] = 0;
        if (i == 0) *batch = G;
    }
    if (qidx) {
        const uint4* src = reinterpret_cast<const uint4*>(qb + (size_t)q * pitch);
        uint4* dst = reinterpret_cast<uint4*>(qb_out + (size_t)i * pitch);
        for (int v = threadIdx.x; v < K / 8; v += 64) dst[v] = src[v];
    }
}

template <typename D>
struct RangeMergeArgs {
    const float* master;     // [n, K] fp32 rows
    const float* qn;         // [pass] normalised queries
    int K;
    const int* qidx;         // slot -> query of the pass; null: query q0 + slot
    int q0;
    const float* min_cos;    // [pass]
    const uint64_t* keys;    // [G, RANGE_CAP] collected keys, rows relative to row_off
    const int* key_cnt;      // [G]
    int64_t row_off;
    int m;                   // max_hits
    int64_t* counts;         // [pass]
    float* cos_out;          // [pass, m] running list, best first; positions in pos_out
    int64_t* pos_out;
    [[no_unique_address]] D deny;      // rows that neither count nor enter the list (deny_kernels.h; DenyNone: the unrestricted search)
};

// first index of the descending list a[0, n) whose key is not above x = number of keys above x
__device__ __forceinline__ int above(const uint64_t* a, int n, uint64_t x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] > x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <typename D>
__global__ __launch_bounds__(MERGE_THREADS) void range_merge_kernel(RangeMergeArgs<D> a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];     // [RANGE_CAP] new matches | [m] running list
    __shared__ int s_n;
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.key_cnt[i];
    if (n > RANGE_CAP) return;                  // incomplete: the host scans this query again over row ranges
    const int q = a.qidx ? a.qidx[i] : a.q0 + i;
    const float t = a.min_cos[q];
    const int64_t prev = a.counts[q];
    const typename D::Probe probe = a.deny.of(q);
    if (tid == 0) s_n = 0;
    __syncthreads();
    uint64_t* nk = lds;
    // fp32 re-score, one wave per row: the chain of select.hip / exact.hip (common.h: rescore_row)
    const float4* qv = reinterpret_cast<const float4*>(a.qn + (size_t)q * a.K);
    const int nvec = a.K >> 2;
    const uint64_t* keys = a.keys + (size_t)i * RANGE_CAP;
    for (int e = wave; e < n; e += MERGE_THREADS / 64) {
        const int64_t row = a.row_off + key_row(keys[e]);
        const float4* rv = reinterpret_cast<const float4*>(a.master + (size_t)row * a.K);
        // the row's bit: one dword by lane 0, issued ahead of the re-score it does not depend on
        const bool denied = lane == 0 && probe.denied((uint32_t)row);
        const float s = rescore_row(rv, qv, nvec, lane);
        if (lane == 0 && s >= t && !denied) {
            const int slot = atomicAdd(&s_n, 1);
            if (a.m > 0) nk[slot] = make_key(s, (uint32_t)row);
        }
    }
    __syncthreads();
    const int nm = s_n;
    if (tid == 0) a.counts[q] = prev + nm;
    if (a.m == 0 || nm == 0) return;
    // bitonic sort, descending, over a power of two >= nm (zero pads: no key of a real score is zero)
    int p2 = 1;
    while (p2 < nm) p2 <<= 1;
    for (int e = nm + tid; e < p2; e += MERGE_THREADS) nk[e] = 0ull;
    __syncthreads();
    for (int size = 2; size <= p2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = tid; e < (p2 >> 1); e += MERGE_THREADS) {
                const int lo = 2 * e - (e & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const uint64_t x = nk[lo], y = nk[hi];
                if ((x < y) == desc) { nk[lo] = y; nk[hi] = x; }
            }
            __syncthreads();
        }
    }
    // the running list into LDS (it is overwritten below), then every entry of both lists to its rank in the union
    const int nr = (int)min<int64_t>(prev, (int64_t)a.m);
    uint64_t* rk = lds + RANGE_CAP;
    float* co = a.cos_out + (size_t)q * a.m;
    int64_t* po = a.pos_out + (size_t)q * a.m;
    for (int j = tid; j < nr; j += MERGE_THREADS) rk[j] = make_key(co[j], (uint32_t)po[j]);
    __syncthreads();
    for (int e = tid; e < nm; e += MERGE_THREADS) {
        const uint64_t x = nk[e];
        const int rank = e + above(rk, nr, x);
        if (rank < a.m) { co[rank] = key_score(x); po[rank] = key_row(x); }
    }
    for (int j = tid; j < nr; j += MERGE_THREADS) {
        const uint64_t x = rk[j];
        const int rank = j + above(nk, nm, x);
        if (rank < a.m) { co[rank] = key_score(x); po[rank] = key_row(x); }
    }
}

// Device groups: P parts [counts | cos | local ids] (RangePart, internal.h), each best first with ties to the lowest local id,
// i.e. to the lowest global id l * P + p.  One workgroup per query; every valid entry goes to its rank in the union.
__global__ __launch_bounds__(256) void range_parts_kernel(const char* __restrict__ parts, int64_t part_bytes, int P, int B, int m,
                                                          int64_t id_base, int64_t* __restrict__ counts_out, float* __restrict__ cos_out,
                                                          int64_t* __restrict__ id_out) {
    const int q = blockIdx.x, tid = threadIdx.x;
    const size_t cos_off = (size_t)B * 8, id_off = cos_off + ((size_t)B * m * 4 + 15) / 16 * 16;
    auto cnt = [&](int p) { return reinterpret_cast<const int64_t*>(parts + p * part_bytes)[q]; };
    auto cs = [&](int p) { return reinterpret_cast<const float*>(parts + p * part_bytes + cos_off) + (size_t)q * m; };
    auto is = [&](int p) { return reinterpret_cast<const int64_t*>(parts + p * part_bytes + id_off) + (size_t)q * m; };
    int64_t total = 0;
    int valid = 0;
    for (int p = 0; p < P; ++p) {
        total += cnt(p);
        valid += (int)min<int64_t>(cnt(p), (int64_t)m);
    }
    if (tid == 0) counts_out[q] = total;
    if (m == 0) return;
    for (int p = 0; p < P; ++p) {
        const int np = (int)min<int64_t>(cnt(p), (int64_t)m);
        const float* c = cs(p);
        const int64_t* d = is(p);
        for (int j = tid; j < np; j += 256) {
            const float x = c[j];
            const int64_t gx = d[j] * P + p;
            int rank = j;
            for (int o = 0; o < P; ++o) {
                if (o == p) continue;
                const int no = (int)min<int64_t>(cnt(o), (int64_t)m);
                const float* co = cs(o);
                const int64_t* dd = is(o);
                int lo = 0, hi = no;             // entries of part o better than (x, gx): a prefix of its list
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const float y = co[mid];
                    const bool better = y > x || (y == x && dd[mid] * P + o < gx);
                    if (better) lo = mid + 1;
                    else hi = mid;
                }
                rank += lo;
            }
            if (rank < m) {
                cos_out[(size_t)q * m + rank] = x;
                id_out[(size_t)q * m + rank] = gx + id_base;
            }
        }
    }
    for (int j = min(valid, m) + tid; j < m; j += 256) {
        cos_out[(size_t)q * m + j] = -INFINITY;
        id_out[(size_t)q * m + j] = -1;
    }
}

int launch_prep(sqe_index* idx, SweepBufs* r, const float* min_cos, const int* qidx, int q0, int G, hipStream_t s) {
    int* key_cnt = r->key_cnt.as<int>();
    hipLaunchKernelGGL(range_prep_kernel, dim3(G), dim3(64), 0, s, min_cos, r->q_resid.as<float>(), idx->resid_max.as<uint32_t>(),
                       idx->dim, G, qidx, q0, r->qb.as<char>(), qidx ? r->qb_h.as<char>() : nullptr, idx->pitch, r->thr.as<float>(),
                       key_cnt, key_cnt + RANGE_MAX_PASS);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

template <typename D>
int launch_merge_with(sqe_index* idx, SweepBufs* r, const float* min_cos, const int* qidx, int q0, int G, int64_t row_off, int m,
                      int64_t* counts, float* cos, int64_t* pos, D deny, hipStream_t s) {
    StageTimer t(idx->ctx->prof, s, ST_SELECT);
    RangeMergeArgs<D> a;
    a.master = idx->master; a.qn = r->qn.as<float>(); a.K = idx->dim; a.qidx = qidx; a.q0 = q0; a.min_cos = min_cos;
    a.keys = r->keys.as<uint64_t>(); a.key_cnt = r->key_cnt.as<int>(); a.row_off = row_off; a.m = m;
    a.counts = counts; a.cos_out = cos; a.pos_out = pos; a.deny = deny;
    SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(range_merge_kernel<D>), MERGE_LDS));
    hipLaunchKernelGGL(range_merge_kernel<D>, dim3(G), dim3(MERGE_THREADS), m > 0 ? (RANGE_CAP + m) * 8 : 0, s, a);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

// bits: the map of a restricted search (within.hip), null for the unrestricted one
int launch_merge(sqe_index* idx, SweepBufs* r, const float* min_cos, const int* qidx, int q0, int G, int64_t row_off, int m,
                 int64_t* counts, float* cos, int64_t* pos, const uint32_t* bits, hipStream_t s) {
    if (bits) return launch_merge_with(idx, r, min_cos, qidx, q0, G, row_off, m, counts, cos, pos, DenyBitmap{bits}, s);
    return launch_merge_with(idx, r, min_cos, qidx, q0, G, row_off, m, counts, cos, pos, DenyNone{}, s);
}

RangeState* range_state(sqe_index* idx) {
    if (!idx->range) idx->range = new (std::nothrow) RangeState;
    return idx->range;
}

// one pass of at most RANGE_MAX_PASS queries, already normalised into r->qn / r->qb / r->q_resid
int range_pass(sqe_index* idx, SweepBufs* r, int B, const float* min_cos, int m, int64_t* counts, float* cos, int64_t* pos, int G,
               const uint32_t* bits, int64_t* walked, hipStream_t s) {
    const int64_t n = idx->n.load();
    std::vector<int> heavy, heavy_cnt, kc;
    // ---- first pass: every row, the queries in groups of G
    for (int g0 = 0; g0 < B; g0 += G) {
        const int gs = std::min(G, B - g0);
        SQE_TRY(launch_prep(idx, r, min_cos, nullptr, g0, gs, s));
        SQE_TRY(launch_sweep_collect(idx, r->qb.as<bf16_t>() + (size_t)g0 * (idx->pitch / 2), r->thr.as<float>(), r->keys.as<uint64_t>(),
                                     r->key_cnt.as<int>(), r->dummy.p, gs, 0, n, s));
        SQE_TRY(launch_merge(idx, r, min_cos, nullptr, g0, gs, 0, m, counts, cos, pos, bits, s));
        kc.resize((size_t)gs);
        SQE_HIP(hipMemcpyAsync(kc.data(), r->key_cnt.p, (size_t)gs * 4, hipMemcpyDeviceToHost, s));
        SQE_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < gs; ++i)
            if (kc[(size_t)i] > RANGE_CAP) { heavy.push_back(g0 + i); heavy_cnt.push_back(kc[(size_t)i]); }
    }
    if (walked) *walked += (int64_t)heavy.size();
    // ---- queries whose buffer overflowed: the walk over row ranges (sweep.hip), each merged only when it fitted for the whole group
    for (size_t h0 = 0; h0 < heavy.size(); h0 += (size_t)G) {
        const int hs = (int)std::min<size_t>((size_t)G, heavy.size() - h0);
        SQE_HIP(hipMemcpyAsync(r->qidx.p, heavy.data() + h0, (size_t)hs * 4, hipMemcpyHostToDevice, s));
        SQE_TRY(launch_prep(idx, r, min_cos, r->qidx.as<int>(), 0, hs, s));
        int64_t most = 1;
        for (int i = 0; i < hs; ++i) most = std::max<int64_t>(most, heavy_cnt[h0 + (size_t)i]);
        const int64_t L0 = std::max<int64_t>(SCAN_BM, n * (RANGE_CAP / 2) / most / SCAN_BM * SCAN_BM);
        SQE_TRY(sweep_walk(idx, *r, hs, L0, RANGE_CAP,
                           [&](int64_t r0) { return launch_merge(idx, r, min_cos, r->qidx.as<int>(), 0, hs, r0, m, counts, cos, pos, bits, s); }, s));
    }
    return SQE_OK;
}

}  // namespace

void range_destroy(RangeState* r) { delete r; }

int launch_range_merge_parts(const char* parts, int P, int B, int m, int64_t id_base, int64_t* counts, float* cos, int64_t* ids, hipStream_t s) {
    if (B <= 0) return SQE_OK;
    hipLaunchKernelGGL(range_parts_kernel, dim3(B), dim3(256), 0, s, parts, (int64_t)RangePart::of(B, m).total, P, B, m, id_base, counts, cos, ids);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

// Caller holds the index lock; everything runs on stream s.  q_dev [B, dim] raw queries, min_cos_dev [B] (no NaN: checked by
// the entry points); outputs on the device: counts [B], cos / ids [B, m].  Synchronises s once per group of queries and once
// per row range of the queries that overflowed their buffer.  bits (within.hip; a map of the filtered search's layout over the
// index as it stands): only rows whose bit is set count and are returned; walked_out: the queries that took the walk.
int index_range_search_impl(sqe_index* idx, const float* q_dev, int B, const float* min_cos_dev, int m, int64_t* count_dev,
                            float* cos_dev, int64_t* id_dev, hipStream_t s, const uint32_t* bits, int64_t* walked_out) {
    if (walked_out) *walked_out = 0;
    const int64_t n = idx->n.load();
    const int K = idx->dim;
    if (B <= 0) return SQE_OK;
    hipLaunchKernelGGL(range_pad_kernel, dim3(grid_of(std::max<int64_t>((int64_t)B * m, B), 256)), dim3(256), 0, s, count_dev, B, cos_dev,
                       id_dev, (int64_t)B * m);
    SQE_HIP(hipGetLastError());
    if (n == 0) return SQE_OK;
    if (n > (int64_t)UINT32_MAX) return fail(SQE_ERR_INVALID, "sqe_index_range_search: more than 2^32 rows");
    RangeState* r = range_state(idx);
    if (!r) return fail(SQE_ERR_OOM, "sqe_index_range_search: host allocation failed");
    const int G = sweep_slots_of(idx);
    SweepBufs* sw = &r->sw;
    SQE_TRY(sw->ensure(idx, B, G, true, s));
    for (int off = 0; off < B; off += RANGE_MAX_PASS) {
        const int bs = std::min(RANGE_MAX_PASS, B - off);
        {
            StageTimer t(idx->ctx->prof, s, ST_PREP);
            SQE_TRY(launch_normalize_rows(q_dev + (size_t)off * K, bs, K, K, sw->qn.as<float>(), sw->qb.as<bf16_t>(), idx->pitch / 2,
                                          sw->q_resid.as<float>(), nullptr, s));
        }
        SQE_TRY(range_pass(idx, sw, bs, min_cos_dev + off, m, count_dev + off, cos_dev + (size_t)off * m, id_dev + (size_t)off * m, G, bits,
                           walked_out, s));
    }
    // positions -> ids (+ id_base)
    return index_positions_to_ids(idx, id_dev, (int64_t)B * m, s);
}

}  // namespace sqe

// ================================================================ C ABI
using namespace sqe;

// who: the entry point's name in the messages
static int range_args_ok(const char* who, sqe_index* idx, const void* q, int B, const void* min_cos, int max_hits, const void* counts,
                         const void* cos, const void* ids) {
    const std::string w(who);
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (B < 0 || max_hits < 0 || max_hits > RANGE_MAX_HITS) return fail(SQE_ERR_INVALID, w + ": need B >= 0 and 0 <= max_hits <= 10000");
    if (B > 0 && (!q || !min_cos || !counts)) return fail(SQE_ERR_INVALID, w + ": null buffer");
    if (B > 0 && max_hits > 0 && (!cos || !ids)) return fail(SQE_ERR_INVALID, w + ": null result buffer");
    return SQE_OK;
}

static int thresholds_ok(const char* who, const float* t, int B) {
    for (int b = 0; b < B; ++b)
        if (std::isnan(t[b])) return fail(SQE_ERR_INVALID, std::string(who) + ": threshold " + std::to_string(b) + " is NaN");
    return SQE_OK;
}

// sqe_index_range_search (set == null) and sqe_index_range_search_where, host form; arguments checked, B > 0.  set: a host list, if any
static int range_host(const char* who, sqe_index* idx, const float* q_host, int B, const float* min_cos_host, int max_hits, const RowSet* set,
                      int64_t* count_out_host, float* cos_out_host, int64_t* id_out_host) {
    SQE_TRY(thresholds_ok(who, min_cos_host, B));
    if (idx->group)
        return group_index_range_search(idx, q_host, B, min_cos_host, max_hits, count_out_host, cos_out_host, id_out_host, false, set);
    OpScope op(idx->ctx, idx->ord, true);
    RangeState* r = range_state(idx);
    if (!r) return fail(SQE_ERR_OOM, std::string(who) + ": host allocation failed");
    const int64_t bm = (int64_t)B * max_hits;
    const size_t qb = round_up((int64_t)B * idx->dim * 4, 16), tb = round_up((int64_t)B * 4, 16), nb = (size_t)B * 8;
    const size_t cb = round_up(bm * 4, 16), ib = (size_t)bm * 8;
    SQE_TRY(r->stage.ensure(qb + tb + nb + cb + ib));
    char* p = r->stage.as<char>();
    float* q_dev = reinterpret_cast<float*>(p);
    float* t_dev = reinterpret_cast<float*>(p + qb);
    int64_t* n_dev = reinterpret_cast<int64_t*>(p + qb + tb);
    float* c_dev = reinterpret_cast<float*>(p + qb + tb + nb);
    int64_t* i_dev = reinterpret_cast<int64_t*>(p + qb + tb + nb + cb);
    SQE_HIP(hipMemcpyAsync(q_dev, q_host, (size_t)B * idx->dim * 4, hipMemcpyHostToDevice, op.s));
    SQE_HIP(hipMemcpyAsync(t_dev, min_cos_host, (size_t)B * 4, hipMemcpyHostToDevice, op.s));
    if (set) SQE_TRY(index_range_search_within(idx, q_dev, B, t_dev, max_hits, *set, n_dev, c_dev, i_dev, op.s));
    else SQE_TRY(index_range_search_impl(idx, q_dev, B, t_dev, max_hits, n_dev, c_dev, i_dev, op.s));
    SQE_HIP(hipMemcpyAsync(count_out_host, n_dev, nb, hipMemcpyDeviceToHost, op.s));
    if (bm > 0) {
        SQE_HIP(hipMemcpyAsync(cos_out_host, c_dev, (size_t)bm * 4, hipMemcpyDeviceToHost, op.s));
        SQE_HIP(hipMemcpyAsync(id_out_host, i_dev, ib, hipMemcpyDeviceToHost, op.s));
    }
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

// the _device forms; set: a device list, if any, which a device group brings to the host first
static int range_device(const char* who, sqe_index* idx, const float* q_dev, int B, const float* min_cos_dev, int max_hits, const RowSet* set,
                        int64_t* count_out_dev, float* cos_out_dev, int64_t* id_out_dev) {
    // the thresholds come to the host first (after the caller's work on the context stream): NaN check and group planning
    std::vector<float> t((size_t)B);
    {
        sqe_ctx* c = idx->ctx;
        SQE_HIP(hipSetDevice(c->device));
        hipStream_t s = c->stream.load();
        SQE_HIP(hipMemcpyAsync(t.data(), min_cos_dev, (size_t)B * 4, hipMemcpyDeviceToHost, s));
        SQE_HIP(hipStreamSynchronize(s));
    }
    SQE_TRY(thresholds_ok(who, t.data(), B));
    if (idx->group && set) {
        std::vector<int64_t> allow;
        SQE_TRY(rowset_allow_to_host(idx, set->allow, set->n_allow, allow));
        const RowSet on_host{set->pr, allow.data(), set->n_allow, true};
        return group_index_range_search(idx, q_dev, B, t.data(), max_hits, count_out_dev, cos_out_dev, id_out_dev, true, &on_host);
    }
    if (idx->group) return group_index_range_search(idx, q_dev, B, t.data(), max_hits, count_out_dev, cos_out_dev, id_out_dev, true);
    OpScope op(idx->ctx, idx->ord, false);
    if (set) return index_range_search_within(idx, q_dev, B, min_cos_dev, max_hits, *set, count_out_dev, cos_out_dev, id_out_dev, op.s);
    return index_range_search_impl(idx, q_dev, B, min_cos_dev, max_hits, count_out_dev, cos_out_dev, id_out_dev, op.s);
}

extern "C" {

int sqe_index_range_search(sqe_index* idx, const float* q_host, int B, const float* min_cos_host, int max_hits, int64_t* count_out_host,
                           float* cos_out_host, int64_t* id_out_host) {
    SQE_TRY(range_args_ok("sqe_index_range_search", idx, q_host, B, min_cos_host, max_hits, count_out_host, cos_out_host, id_out_host));
    if (B == 0) return SQE_OK;
    return range_host("sqe_index_range_search", idx, q_host, B, min_cos_host, max_hits, nullptr, count_out_host, cos_out_host, id_out_host);
}

int sqe_index_range_search_device(sqe_index* idx, const float* q_dev, int B, const float* min_cos_dev, int max_hits, int64_t* count_out_dev,
                                  float* cos_out_dev, int64_t* id_out_dev) {
    SQE_TRY(range_args_ok("sqe_index_range_search", idx, q_dev, B, min_cos_dev, max_hits, count_out_dev, cos_out_dev, id_out_dev));
    if (B == 0) return SQE_OK;
    return range_device("sqe_index_range_search", idx, q_dev, B, min_cos_dev, max_hits, nullptr, count_out_dev, cos_out_dev, id_out_dev);
}

int sqe_index_range_search_where(sqe_index* idx, const float* q_host, int B, const float* min_cos_host, int max_hits,
                                 const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                                 const int64_t* allow_ids_host, int64_t n_allow, int64_t* count_out_host, float* cos_out_host,
                                 int64_t* id_out_host) {
    const char* who = "sqe_index_range_search_where";
    int64_t one[2];
    SQE_TRY(range_args_ok(who, idx, q_host, B, min_cos_host, max_hits, count_out_host, cos_out_host, id_out_host));
    SQE_TRY(rowset_args_ok(who, clauses, n_clauses, set_values, n_set, allow_ids_host, n_allow, one));
    if (B == 0) return SQE_OK;
    const RowSet set{FieldPreds{clauses, one, 1, set_values, n_set}, allow_ids_host, n_allow, true};
    return range_host(who, idx, q_host, B, min_cos_host, max_hits, &set, count_out_host, cos_out_host, id_out_host);
}

int sqe_index_range_search_where_device(sqe_index* idx, const float* q_dev, int B, const float* min_cos_dev, int max_hits,
                                        const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                                        const int64_t* allow_ids_dev, int64_t n_allow, int64_t* count_out_dev, float* cos_out_dev,
                                        int64_t* id_out_dev) {
    const char* who = "sqe_index_range_search_where";
    int64_t one[2];
    SQE_TRY(range_args_ok(who, idx, q_dev, B, min_cos_dev, max_hits, count_out_dev, cos_out_dev, id_out_dev));
    SQE_TRY(rowset_args_ok(who, clauses, n_clauses, set_values, n_set, allow_ids_dev, n_allow, one));
    if (B == 0) return SQE_OK;
    const RowSet set{FieldPreds{clauses, one, 1, set_values, n_set}, allow_ids_dev, n_allow, false};
    return range_device(who, idx, q_dev, B, min_cos_dev, max_hits, &set, count_out_dev, cos_out_dev, id_out_dev);
}

}  // extern "C"
