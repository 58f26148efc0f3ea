// sweep.hip -- the device-side sweep that radial (range.hip), collapsed (collapse.hip) and exclusion search (exclude.hip) fall
// back to when a plain search at a fixed depth cannot answer a query.  A group of at most G slots (queries) walks over all live
// rows in ranges:
//   1. collect: the unchanged COLLECT-mode bf16 scan (scan.hip) over the range at each slot's threshold - eps (kernels.h:
//      scan_eps; a row whose cosine reaches t has a scan score >= t - eps), at most EXACT_CAP keys per slot, the count going on
//      past that;
//   2. the per-slot key counts come back to the host: the one read-back and stream synchronisation per range;
//   3. a slot overflowed: the range is halved (a multiple of SCAN_BM rows, at least SCAN_BM) and collected again.  SCAN_BM rows
//      never overflow EXACT_CAP keys, so the walk always ends;
//   4. otherwise the feature's merge kernel re-scores the keys in fp32 and merges them into the slots' running results (it may
//      raise the thresholds), and the next range is twice as long if this one came in under a quarter of the buffer.
// The three merge kernels differ and live with their features; this file holds what they share: the buffers (SweepBufs), the
// collect launch, the walk, and -- for the two searches that sweep the queries their first stage flagged -- the compaction of the
// flags into dense slots, the reset of a slot and the pass loop around the walk.
#include <math.h>

#include <algorithm>

#include "internal.h"

namespace sqe {

namespace {

// One workgroup per pass of SWEEP_MAX_PASS queries: the flagged queries of the pass (all of them without flags), in
// query order, to dense slots qidx[pass * SWEEP_MAX_PASS + slot] = query of the pass; pass_cnt[pass] = their number.
__global__ __launch_bounds__(SWEEP_MAX_PASS) void sweep_compact_kernel(const int* __restrict__ flags, int B, int* __restrict__ qidx,
                                                                       int* __restrict__ pass_cnt) {
    __shared__ int s_tot[SWEEP_MAX_PASS / 64];
    const int pass = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = pass * SWEEP_MAX_PASS + tid;
    const bool f = q < B && (flags ? flags[q] != 0 : true);
    const unsigned long long m = __ballot(f);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_tot[wave] = __popcll(m);
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < SWEEP_MAX_PASS / 64; ++w) {
        if (w < wave) base += s_tot[w];
        total += s_tot[w];
    }
    if (f) qidx[pass * SWEEP_MAX_PASS + base + before] = tid;
    if (tid == 0) pass_cnt[pass] = total;
}

// One workgroup per slot i of a sweep: the bf16 row of its query to row i of qb_out, thresholds -inf, an empty running
// list (the query's output rows are reset to padding: the sweep computes the answer from nothing; key_out may be null).
// Block 0 stores the batch size.
__global__ __launch_bounds__(64) void sweep_prep_kernel(const int* __restrict__ qidx, int G, const char* __restrict__ qb,
                                                        char* __restrict__ qb_out, int pitch, int K, int k, float* __restrict__ thr,
                                                        float* __restrict__ kth, int* __restrict__ lcnt, int* __restrict__ key_cnt,
                                                        int* __restrict__ batch, float* __restrict__ cos_out,
                                                        int64_t* __restrict__ pos_out, int64_t* __restrict__ key_out) {
    const int i = blockIdx.x, q = qidx[i];
    if (threadIdx.x == 0) {
        thr[i] = -INFINITY;
        kth[i] = -INFINITY;
        lcnt[i] = 0;
        key_cnt[i] = 0;
        if (i == 0) *batch = G;
    }
    const uint4* src = reinterpret_cast<const uint4*>(qb + (size_t)q * pitch);
    uint4* dst = reinterpret_cast<uint4*>(qb_out + (size_t)i * pitch);
    for (int v = threadIdx.x; v < K / 8; v += 64) dst[v] = src[v];
    for (int j = threadIdx.x; j < k; j += 64) {
        const size_t o = (size_t)q * k + j;
        cos_out[o] = -INFINITY;
        pos_out[o] = -1;
        if (key_out) key_out[o] = SQE_KEY_NONE;
    }
}

}  // namespace

int SweepBufs::ensure(sqe_index* idx, int B, int G, bool radial, hipStream_t s) {
    const size_t pitch = (size_t)idx->pitch;
    SQE_TRY(qn.ensure((size_t)std::min(B, SWEEP_MAX_PASS) * idx->dim * 4));
    if (!radial) {
        SQE_TRY(qb.ensure((size_t)SWEEP_MAX_PASS * pitch));
        SQE_TRY(kth.ensure((size_t)SWEEP_MAX_PASS * 4));
        SQE_TRY(lcnt.ensure((size_t)SWEEP_MAX_PASS * 4));
    } else if ((size_t)(SWEEP_MAX_PASS + 256) * pitch > qb.bytes) {      // radial search scans the pass's rows in place
        SQE_TRY(qb.ensure((size_t)(SWEEP_MAX_PASS + 256) * pitch));
        SQE_HIP(hipMemsetAsync(qb.p, 0, qb.bytes, s));                    // query rows past a block's batch read as zero
    }
    if ((size_t)(G + 256) * pitch > qb_h.bytes) {
        SQE_TRY(qb_h.ensure((size_t)(G + 256) * pitch));
        SQE_HIP(hipMemsetAsync(qb_h.p, 0, qb_h.bytes, s));
    }
    SQE_TRY(q_resid.ensure((size_t)SWEEP_MAX_PASS * 4));
    SQE_TRY(thr.ensure((size_t)SWEEP_MAX_PASS * 4));
    SQE_TRY(keys.ensure((size_t)G * EXACT_CAP * 8));
    SQE_TRY(key_cnt.ensure((size_t)(SWEEP_MAX_PASS + 4) * 4));
    SQE_TRY(qidx.ensure((size_t)SWEEP_MAX_PASS * 4));
    SQE_TRY(dummy.ensure(256));
    return SQE_OK;
}

int sweep_slots_of(const sqe_index* idx) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(SWEEP_MAX_PASS, idx->range_key_budget / EXACT_CAP));
}

int launch_sweep_collect(sqe_index* idx, const bf16_t* qb_h, const float* thr, uint64_t* keys, int* key_cnt, void* dummy, int G, int64_t r0,
                         int64_t r1, hipStream_t s) {
    sqe_ctx* ctx = idx->ctx;
    StageTimer t(ctx->prof, s, ST_SCAN);
    ScanArgs a;
    a.db = reinterpret_cast<const bf16_t*>(reinterpret_cast<const char*>(idx->scan) + (size_t)r0 * idx->pitch);
    a.q = qb_h; a.n_rows = r1 - r0; a.K = idx->dim; a.B = G;
    a.db_pitch = idx->pitch; a.q_pitch = idx->pitch;
    a.cand = reinterpret_cast<uint64_t*>(dummy); a.cand_cnt = reinterpret_cast<int*>(dummy); a.gmax = reinterpret_cast<uint32_t*>(dummy);
    a.collect_thr = thr; a.collect_keys = keys; a.collect_cnt = key_cnt;
    a.unc_count = key_cnt + SWEEP_MAX_PASS;
    a.collect_lo = 1; a.collect_hi = 1 << 30;
    const ScanPlan plan = make_scan_plan(r1 - r0, G, 16, ctx->cu_count);
    return launch_scan_collect(plan, a, s);
}

int launch_sweep_compact(const int* flags, int B, int* qidx, int* pass_cnt, hipStream_t s) {
    const int passes = (B + SWEEP_MAX_PASS - 1) / SWEEP_MAX_PASS;
    hipLaunchKernelGGL(sweep_compact_kernel, dim3(passes), dim3(SWEEP_MAX_PASS), 0, s, flags, B, qidx, pass_cnt);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int sweep_walk(sqe_index* idx, SweepBufs& b, int hs, int64_t L0, int cap, const SweepMerge& merge, hipStream_t s) {
    const int64_t n = idx->n.load();
    std::vector<int> kc((size_t)hs);
    int64_t L = L0;
    for (int64_t r0 = 0; r0 < n;) {
        const int64_t r1 = std::min(n, r0 + L);
        SQE_HIP(hipMemsetAsync(b.key_cnt.p, 0, (size_t)hs * 4, s));
        SQE_TRY(launch_sweep_collect(idx, b.qb_h.as<bf16_t>(), b.thr.as<float>(), b.keys.as<uint64_t>(), b.key_cnt.as<int>(), b.dummy.p, hs,
                                     r0, r1, s));
        SQE_HIP(hipMemcpyAsync(kc.data(), b.key_cnt.p, (size_t)hs * 4, hipMemcpyDeviceToHost, s));
        SQE_HIP(hipStreamSynchronize(s));
        const int top = *std::max_element(kc.begin(), kc.end());
        if (top > cap) {                        // SCAN_BM rows never overflow: the walk ends
            L = std::max<int64_t>(SCAN_BM, L / 2 / SCAN_BM * SCAN_BM);
            continue;
        }
        SQE_TRY(merge(r0));
        r0 = r1;
        if (top <= cap / 4) L *= 2;
    }
    return SQE_OK;
}

int sweep_flagged(sqe_index* idx, SweepBufs& b, const int* flags, const float* q_dev, int B, int k, float* cos, int64_t* pos, int64_t* keys,
                  std::atomic<int64_t>& swept_out, const SweepPassMerge& merge, hipStream_t s) {
    sqe_ctx* ctx = idx->ctx;
    const int K = idx->dim;
    const int passes = (B + SWEEP_MAX_PASS - 1) / SWEEP_MAX_PASS;
    SQE_TRY(b.qidx.ensure((size_t)passes * SWEEP_MAX_PASS * 4));
    SQE_TRY(b.pass_cnt.ensure((size_t)passes * 4));
    SQE_TRY(launch_sweep_compact(flags, B, b.qidx.as<int>(), b.pass_cnt.as<int>(), s));
    std::vector<int> pass_cnt((size_t)passes);
    SQE_HIP(hipMemcpyAsync(pass_cnt.data(), b.pass_cnt.p, (size_t)passes * 4, hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));
    int64_t swept = 0;
    for (int v : pass_cnt) swept += v;
    swept_out.store(swept);
    if (swept == 0) return SQE_OK;
    const int G = sweep_slots_of(idx);
    SQE_TRY(b.ensure(idx, B, G, false, s));
    for (int pi = 0; pi < passes; ++pi) {
        const int cnt = pass_cnt[(size_t)pi];
        if (cnt == 0) continue;
        const int off = pi * SWEEP_MAX_PASS, bs = std::min(SWEEP_MAX_PASS, B - off);
        {
            StageTimer t(ctx->prof, s, ST_PREP);
            SQE_TRY(launch_normalize_rows(q_dev + (size_t)off * K, bs, K, K, b.qn.as<float>(), b.qb.as<bf16_t>(), idx->pitch / 2,
                                          b.q_resid.as<float>(), nullptr, s));
        }
        for (int h0 = 0; h0 < cnt; h0 += G) {
            const int hs = std::min(G, cnt - h0);
            const int* qidx = b.qidx.as<int>() + off + h0;
            int* key_cnt = b.key_cnt.as<int>();
            hipLaunchKernelGGL(sweep_prep_kernel, dim3(hs), dim3(64), 0, s, qidx, hs, b.qb.as<char>(), b.qb_h.as<char>(), idx->pitch, K, k,
                               b.thr.as<float>(), b.kth.as<float>(), b.lcnt.as<int>(), key_cnt, key_cnt + SWEEP_MAX_PASS,
                               cos + (size_t)off * k, pos + (size_t)off * k, keys ? keys + (size_t)off * k : nullptr);
            SQE_HIP(hipGetLastError());
            SQE_TRY(sweep_walk(idx, b, hs, EXACT_CAP / 2, EXACT_CAP, [&](int64_t r0) { return merge(off, qidx, hs, r0); }, s));
        }
    }
    return SQE_OK;
}

}  // namespace sqe
