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
//      scanned again over row ranges: a range is collected, its counts read back, and it is merged only when no query of
//      the group overflowed it -- else it is halved and collected again.  A range of 256 rows can never overflow, so the
//      walk always ends; it starts where the first pass's count predicts 2048 keys and doubles after ranges that came in
//      under 1024.
//   4. positions -> ids through the index's id map, then id_base.
// Memory: one group holds range_key_budget / RANGE_CAP queries (at least 1, at most 1024), i.e. at most range_key_budget keys,
// whatever the number of matches.  Nothing else grows with the data: the running lists are the caller's output buffers.
// The owner's search buffers (candidate lists, fallback buffers, int8 state, staging) are never touched.
#include <math.h>
#include <cmath>
#include <string.h>

#include <algorithm>
#include <vector>

#include "internal.h"

namespace sqe {

constexpr int RANGE_CAP = EXACT_CAP;        // keys per query and collect launch: the collect scan's buffer stride
constexpr int RANGE_MAX_PASS = 1024;        // queries normalised at once (larger batches run in passes, as search)
constexpr int MERGE_THREADS = 512;
constexpr int MERGE_LDS = (RANGE_CAP + RANGE_MAX_HITS) * 8;

struct RangeState {
    DevBuf stage;      // host entry points: queries, thresholds, counts and results
    DevBuf qn;         // [RANGE_MAX_PASS, dim] fp32 normalised queries of the pass
    DevBuf qb;         // [RANGE_MAX_PASS + 256] bf16 query rows at the index pitch (the collect scan reads whole query blocks)
    DevBuf q_resid;    // [RANGE_MAX_PASS]
    DevBuf qb_h;       // [G + 256] bf16 rows of the queries re-scanned over row ranges
    DevBuf thr;        // [G] collect thresholds of the group's slots
    DevBuf keys;       // [G, RANGE_CAP] u64
    DevBuf key_cnt;    // [G] int, then the group size (the collect scan reads its batch from the device)
    DevBuf qidx;       // [G] slot -> query of the pass
    DevBuf dummy;      // candidate / bound pointers of the collect launch (COLLECT mode never reads or writes them)
};

namespace {

unsigned grid_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

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

struct MergeArgs {
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

__global__ __launch_bounds__(MERGE_THREADS) void range_merge_kernel(MergeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];     // [RANGE_CAP] new matches | [m] running list
    __shared__ int s_n;
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.key_cnt[i];
    if (n > RANGE_CAP) return;                  // incomplete: the host scans this query again over row ranges
    const int q = a.qidx ? a.qidx[i] : a.q0 + i;
    const float t = a.min_cos[q];
    const int64_t prev = a.counts[q];
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
        const float s = rescore_row(rv, qv, nvec, lane);
        if (lane == 0 && s >= t) {
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

__global__ __launch_bounds__(256) void range_offset_ids_kernel(int64_t* __restrict__ ids, int64_t count, int64_t base) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < count && ids[j] >= 0) ids[j] += base;
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

int launch_prep(sqe_index* idx, RangeState* r, const float* min_cos, const int* qidx, int q0, int G, hipStream_t s) {
    int* key_cnt = r->key_cnt.as<int>();
    hipLaunchKernelGGL(range_prep_kernel, dim3(G), dim3(64), 0, s, min_cos, r->q_resid.as<float>(), idx->resid_max.as<uint32_t>(),
                       idx->dim, G, qidx, q0, r->qb.as<char>(), qidx ? r->qb_h.as<char>() : nullptr, idx->pitch, r->thr.as<float>(),
                       key_cnt, key_cnt + RANGE_MAX_PASS);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

// the collect scan of G queries (bf16 rows at qb, thresholds r->thr) over rows [r0, r1) of the index
int launch_collect(sqe_index* idx, RangeState* r, const bf16_t* qb, int G, int64_t r0, int64_t r1, hipStream_t s) {
    sqe_ctx* c = idx->ctx;
    StageTimer t(c->prof, s, ST_SCAN);
    ScanArgs a;
    a.db = reinterpret_cast<const bf16_t*>(reinterpret_cast<const char*>(idx->scan) + (size_t)r0 * idx->pitch);
    a.q = qb; a.n_rows = r1 - r0; a.K = idx->dim; a.B = G;
    a.db_pitch = idx->pitch; a.q_pitch = idx->pitch;
    a.cand = r->dummy.as<uint64_t>(); a.cand_cnt = r->dummy.as<int>(); a.gmax = r->dummy.as<uint32_t>();
    a.collect_thr = r->thr.as<float>(); a.collect_keys = r->keys.as<uint64_t>(); a.collect_cnt = r->key_cnt.as<int>();
    a.unc_count = r->key_cnt.as<int>() + RANGE_MAX_PASS;
    a.collect_lo = 1; a.collect_hi = 1 << 30;
    const ScanPlan plan = make_scan_plan(r1 - r0, G, 16, c->cu_count);
    return launch_scan_collect(plan, a, s);
}

int launch_merge(sqe_index* idx, RangeState* r, const float* min_cos, const int* qidx, int q0, int G, int64_t row_off, int m,
                 int64_t* counts, float* cos, int64_t* pos, hipStream_t s) {
    StageTimer t(idx->ctx->prof, s, ST_SELECT);
    MergeArgs a;
    a.master = idx->master; a.qn = r->qn.as<float>(); a.K = idx->dim; a.qidx = qidx; a.q0 = q0; a.min_cos = min_cos;
    a.keys = r->keys.as<uint64_t>(); a.key_cnt = r->key_cnt.as<int>(); a.row_off = row_off; a.m = m;
    a.counts = counts; a.cos_out = cos; a.pos_out = pos;
    SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(range_merge_kernel), MERGE_LDS));
    hipLaunchKernelGGL(range_merge_kernel, dim3(G), dim3(MERGE_THREADS), m > 0 ? (RANGE_CAP + m) * 8 : 0, s, a);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int read_counts(RangeState* r, int G, std::vector<int>& out, hipStream_t s) {
    out.resize((size_t)G);
    SQE_HIP(hipMemcpyAsync(out.data(), r->key_cnt.p, (size_t)G * 4, hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));
    return SQE_OK;
}

RangeState* range_state(sqe_index* idx) {
    if (!idx->range) idx->range = new (std::nothrow) RangeState;
    return idx->range;
}

// one pass of at most RANGE_MAX_PASS queries, already normalised into r->qn / r->qb / r->q_resid
int range_pass(sqe_index* idx, RangeState* r, int B, const float* min_cos, int m, int64_t* counts, float* cos, int64_t* pos, int G,
               hipStream_t s) {
    const int64_t n = idx->n.load();
    std::vector<int> heavy, heavy_cnt, kc;
    // ---- first pass: every row, the queries in groups of G
    for (int g0 = 0; g0 < B; g0 += G) {
        const int gs = std::min(G, B - g0);
        SQE_TRY(launch_prep(idx, r, min_cos, nullptr, g0, gs, s));
        SQE_TRY(launch_collect(idx, r, r->qb.as<bf16_t>() + (size_t)g0 * (idx->pitch / 2), gs, 0, n, s));
        SQE_TRY(launch_merge(idx, r, min_cos, nullptr, g0, gs, 0, m, counts, cos, pos, s));
        SQE_TRY(read_counts(r, gs, kc, s));
        for (int i = 0; i < gs; ++i)
            if (kc[(size_t)i] > RANGE_CAP) { heavy.push_back(g0 + i); heavy_cnt.push_back(kc[(size_t)i]); }
    }
    // ---- queries whose buffer overflowed: row ranges, each merged only when it fitted for the whole group
    for (size_t h0 = 0; h0 < heavy.size(); h0 += (size_t)G) {
        const int hs = (int)std::min<size_t>((size_t)G, heavy.size() - h0);
        SQE_HIP(hipMemcpyAsync(r->qidx.p, heavy.data() + h0, (size_t)hs * 4, hipMemcpyHostToDevice, s));
        SQE_TRY(launch_prep(idx, r, min_cos, r->qidx.as<int>(), 0, hs, s));
        int64_t most = 1;
        for (int i = 0; i < hs; ++i) most = std::max<int64_t>(most, heavy_cnt[h0 + (size_t)i]);
        int64_t L = std::max<int64_t>(SCAN_BM, n * (RANGE_CAP / 2) / most / SCAN_BM * SCAN_BM);
        for (int64_t r0 = 0; r0 < n;) {
            const int64_t r1 = std::min(n, r0 + L);
            SQE_HIP(hipMemsetAsync(r->key_cnt.p, 0, (size_t)hs * 4, s));
            SQE_TRY(launch_collect(idx, r, r->qb_h.as<bf16_t>(), hs, r0, r1, s));
            SQE_TRY(read_counts(r, hs, kc, s));
            const int top = *std::max_element(kc.begin(), kc.end());
            if (top > RANGE_CAP) {              // 256 rows never overflow: the walk ends
                L = std::max<int64_t>(SCAN_BM, L / 2 / SCAN_BM * SCAN_BM);
                continue;
            }
            SQE_TRY(launch_merge(idx, r, min_cos, r->qidx.as<int>(), 0, hs, r0, m, counts, cos, pos, s));
            r0 = r1;
            if (top <= RANGE_CAP / 4) L *= 2;
        }
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
// per row range of the queries that overflowed their buffer.
int index_range_search_impl(sqe_index* idx, const float* q_dev, int B, const float* min_cos_dev, int m, int64_t* count_dev,
                            float* cos_dev, int64_t* id_dev, hipStream_t s) {
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
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(RANGE_MAX_PASS, idx->range_key_budget / RANGE_CAP));
    const int pass = std::min(B, RANGE_MAX_PASS);
    SQE_TRY(r->qn.ensure((size_t)pass * K * 4));
    if ((size_t)(RANGE_MAX_PASS + 256) * idx->pitch > r->qb.bytes) {
        SQE_TRY(r->qb.ensure((size_t)(RANGE_MAX_PASS + 256) * idx->pitch));
        SQE_HIP(hipMemsetAsync(r->qb.p, 0, r->qb.bytes, s));          // query rows past a block's batch read as zero
    }
    if ((size_t)(G + 256) * idx->pitch > r->qb_h.bytes) {
        SQE_TRY(r->qb_h.ensure((size_t)(G + 256) * idx->pitch));
        SQE_HIP(hipMemsetAsync(r->qb_h.p, 0, r->qb_h.bytes, s));
    }
    SQE_TRY(r->q_resid.ensure((size_t)RANGE_MAX_PASS * 4));
    SQE_TRY(r->thr.ensure((size_t)RANGE_MAX_PASS * 4));
    SQE_TRY(r->keys.ensure((size_t)G * RANGE_CAP * 8));
    SQE_TRY(r->key_cnt.ensure((size_t)(RANGE_MAX_PASS + 4) * 4));
    SQE_TRY(r->qidx.ensure((size_t)RANGE_MAX_PASS * 4));
    SQE_TRY(r->dummy.ensure(256));
    for (int off = 0; off < B; off += RANGE_MAX_PASS) {
        const int bs = std::min(RANGE_MAX_PASS, B - off);
        {
            StageTimer t(idx->ctx->prof, s, ST_PREP);
            SQE_TRY(launch_normalize_rows(q_dev + (size_t)off * K, bs, K, K, r->qn.as<float>(), r->qb.as<bf16_t>(), idx->pitch / 2,
                                          r->q_resid.as<float>(), nullptr, s));
        }
        SQE_TRY(range_pass(idx, r, bs, min_cos_dev + off, m, count_dev + off, cos_dev + (size_t)off * m, id_dev + (size_t)off * m, G, s));
    }
    // positions -> ids (+ id_base)
    const int64_t bm = (int64_t)B * m;
    if (bm == 0) return SQE_OK;
    if (idx->has_map) return launch_translate_ids(id_dev, bm, idx->idmap.as<int64_t>(), idx->id_base, s);
    if (idx->id_base != 0) {
        hipLaunchKernelGGL(range_offset_ids_kernel, dim3(grid_of(bm, 256)), dim3(256), 0, s, id_dev, bm, idx->id_base);
        SQE_HIP(hipGetLastError());
    }
    return SQE_OK;
}

}  // namespace sqe

// ================================================================ C ABI
using namespace sqe;

extern "C" {

static int range_args_ok(sqe_index* idx, const void* q, int B, const void* min_cos, int max_hits, const void* counts, const void* cos,
                         const void* ids) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (B < 0 || max_hits < 0 || max_hits > RANGE_MAX_HITS)
        return fail(SQE_ERR_INVALID, "sqe_index_range_search: need B >= 0 and 0 <= max_hits <= 10000");
    if (B > 0 && (!q || !min_cos || !counts)) return fail(SQE_ERR_INVALID, "sqe_index_range_search: null buffer");
    if (B > 0 && max_hits > 0 && (!cos || !ids)) return fail(SQE_ERR_INVALID, "sqe_index_range_search: null result buffer");
    return SQE_OK;
}

static int thresholds_ok(const float* t, int B) {
    for (int b = 0; b < B; ++b)
        if (std::isnan(t[b])) return fail(SQE_ERR_INVALID, "sqe_index_range_search: threshold " + std::to_string(b) + " is NaN");
    return SQE_OK;
}

int sqe_index_range_search(sqe_index* idx, const float* q_host, int B, const float* min_cos_host, int max_hits, int64_t* count_out_host,
                           float* cos_out_host, int64_t* id_out_host) {
    SQE_TRY(range_args_ok(idx, q_host, B, min_cos_host, max_hits, count_out_host, cos_out_host, id_out_host));
    if (B == 0) return SQE_OK;
    SQE_TRY(thresholds_ok(min_cos_host, B));
    if (idx->group)
        return group_index_range_search(idx, q_host, B, min_cos_host, max_hits, count_out_host, cos_out_host, id_out_host, false);
    OpScope op(idx->ctx, idx->ord, true);
    RangeState* r = range_state(idx);
    if (!r) return fail(SQE_ERR_OOM, "sqe_index_range_search: host allocation failed");
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
    SQE_TRY(index_range_search_impl(idx, q_dev, B, t_dev, max_hits, n_dev, c_dev, i_dev, op.s));
    SQE_HIP(hipMemcpyAsync(count_out_host, n_dev, nb, hipMemcpyDeviceToHost, op.s));
    if (bm > 0) {
        SQE_HIP(hipMemcpyAsync(cos_out_host, c_dev, (size_t)bm * 4, hipMemcpyDeviceToHost, op.s));
        SQE_HIP(hipMemcpyAsync(id_out_host, i_dev, ib, hipMemcpyDeviceToHost, op.s));
    }
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_range_search_device(sqe_index* idx, const float* q_dev, int B, const float* min_cos_dev, int max_hits, int64_t* count_out_dev,
                                  float* cos_out_dev, int64_t* id_out_dev) {
    SQE_TRY(range_args_ok(idx, q_dev, B, min_cos_dev, max_hits, count_out_dev, cos_out_dev, id_out_dev));
    if (B == 0) return SQE_OK;
    // the thresholds come to the host first (after the caller's work on the context stream): NaN check and group planning
    std::vector<float> t((size_t)B);
    {
        sqe_ctx* c = idx->ctx;
        SQE_HIP(hipSetDevice(c->device));
        hipStream_t s = c->stream.load();
        SQE_HIP(hipMemcpyAsync(t.data(), min_cos_dev, (size_t)B * 4, hipMemcpyDeviceToHost, s));
        SQE_HIP(hipStreamSynchronize(s));
    }
    SQE_TRY(thresholds_ok(t.data(), B));
    if (idx->group) return group_index_range_search(idx, q_dev, B, t.data(), max_hits, count_out_dev, cos_out_dev, id_out_dev, true);
    OpScope op(idx->ctx, idx->ord, false);
    return index_range_search_impl(idx, q_dev, B, min_cos_dev, max_hits, count_out_dev, cos_out_dev, id_out_dev, op.s);
}

}  // extern "C"
