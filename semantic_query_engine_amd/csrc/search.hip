// search.hip -- the flat search pipeline behind index_search_impl (internal.h): every flat search the library answers
// (plain top-k, the scratch index of a filtered search, each shard of a device group, the IVF coarse quantiser's own
// index) runs search_positions below.  Host code only: the kernels are in scan*.hip, select*.hip, exact.hip, quant.hip.
// The caller holds the index lock and names the stream (internal.h).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <tuple>
#include <utility>

#include "internal.h"

namespace sqe {

__global__ void add_count_kernel(int* acc, const int* v) { *acc += *v; }

namespace {

int auto_kp(const sqe_index* idx, int k) {
    if (idx->rescore_k > 0) return std::min(MAX_KP, std::max(idx->rescore_k, k));
    // The certificate needs the kp-th scan score to sit more than eps (~2.5e-3 at dim 1024) below the
    // k-th true cosine.  On 10M random rows the 10th -> 32nd gap is only ~3 sigma above eps (a few
    // queries per 1024 would need the fp32 rescan); 10th -> 64th makes that a 1e-5 event.
    // kp <= 64 keeps the cross-chunk bound of the scan filter (64 table columns), which halves the scan
    // time, so with the certificate guarding exactness kp stays 64 up to k = 32; beyond that the candidate
    // set has to grow with k and the scan runs on per-chunk thresholds only.
    // 128 candidates (compaction window 128) up to k = 128.  Above that the 512-slot lists leave a window of
    // only 256 - kp entries, so kp = k exactly (largest window; the certificate then fails and the collect
    // pass supplies the answer) -- far outside the reference's k = 3.
    if (idx->certify) return k <= 32 ? 64 : k <= 128 ? 128 : k;
    return std::min(MAX_KP, std::max(32, 4 * k));
}

// The values of one pass (at most MAX_PASS queries) that its stages share.
struct Pass {
    sqe_index* idx;
    hipStream_t s;
    int64_t n_rows;
    int B, k, kp;
    ScanPlan plan;
    float* cos_out;              // [B, k] on the device
    int64_t* id_out;             // [B, k] row positions
    int pass_index;              // which pass of a batch above MAX_PASS
    bool certify;                // prepare_pass: the certificate and the collect pass run
    int* unc_count;              // ... and their device buffers (null without the certificate)
    float* collect_thr;
    int step8, m8;               // the sample plan in effect (int8 first pass)
};

// ---------------------------------------------------------------- reporting of the knobs build
// knob_env returns null in the shipped library: nothing below runs there and no environment variable is read.
bool i8_stamps_wanted() {
    static const bool want_stamps = [] { const char* e = knob_env("SQE_I8_STAMPS"); return e && e[0] == '1'; }();   // knobs build only
    return want_stamps;
}

bool scan_counters_wanted() {
    static const bool want = [] { const char* e = knob_env("SQE_DBG"); return e && (atoi(e) & 32); }();   // knobs build only
    return want;
}

// zeroed counters / stamps of the next scan launch, which receives them through *slot
int arm_dbg(sqe_index* idx, hipStream_t s, unsigned long long** slot) {
    SQE_TRY(idx->dbg.ensure(8192));
    SQE_HIP(hipMemsetAsync(idx->dbg.p, 0, 8192, s));
    *slot = idx->dbg.as<unsigned long long>();
    return SQE_OK;
}

// int8 tile stamps of the collect scan that has just been launched (SQE_I8_STAMPS=1)
int report_i8_stamps(sqe_index* idx, hipStream_t s) {
    unsigned long long h[256];
    SQE_HIP(hipMemcpyAsync(h, idx->dbg.p, sizeof(h), hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));
    int wall_khz = 0;
    (void)hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, idx->ctx->device);
    for (int blk = 0; blk < 2; ++blk) {
        const unsigned long long* o = h + blk * 128;
        int prev = -1;
        for (int sl = 0; sl < 32; ++sl) {
            if (!o[sl * 3]) continue;
            if (prev >= 0 && o[sl * 3] > o[prev * 3]) {
                const double tiles = (double)(o[sl * 3] - o[prev * 3]);
                const double us = (double)(o[sl * 3 + 1] - o[prev * 3 + 1]) / (wall_khz / 1e3);
                const double cyc = (double)(o[sl * 3 + 2] - o[prev * 3 + 2]);
                fprintf(stderr, "[sqe i8 stamps] wg %3d tiles %5llu..%5llu: %7.2f us per tile, %7.0f core cycles per tile, %5.0f MHz\n",
                        blk ? 100 : 0, o[prev * 3], o[sl * 3], us / tiles, cyc / tiles, us > 0 ? cyc / us : 0.0);
            }
            prev = sl;
        }
    }
    idx->dbg.release();
    return SQE_OK;
}

// SQE_DBG bit 32: counters and phase stamps of the bf16 scan of this pass (nothing unless the index holds armed counters)
int report_scan_counters(const Pass& p) {
    sqe_index* idx = p.idx;
    const ScanPlan& plan = p.plan;
    hipStream_t s = p.s;
    if (!idx->dbg.p) return SQE_OK;
    unsigned long long h[1024];
    SQE_HIP(hipMemcpyAsync(h, idx->dbg.p, 8192, hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));
    int wall_khz = 0;
    (void)hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, idx->ctx->device);
    fprintf(stderr, "[sqe dbg] appends=%llu slow_path_entries=%llu compactions=%llu block0_core_ticks=%llu wall_ticks=%llu core_mhz=%.0f\n",
            h[0], h[1], h[2], h[4], h[5], h[5] ? (double)h[4] / (double)h[5] * wall_khz / 1e3 : 0.0);
    // ping-pong scan, counters build: core cycles per steady-state phase, per wave of workgroups 0 and 100
    for (int blk = 0; blk < 2; ++blk)
        for (int w = 0; w < 8; ++w) {
            const unsigned long long* o = h + 8 + blk * 64 + w * 8;
            if (!o[0]) continue;
            const double n = (double)o[0];
            fprintf(stderr, "[sqe dbg] wg %d wave %d: phases=%llu  cmp %.0f  barrier after cmp %.0f | mem: dma issue %.0f  lds reads issue %.0f  waitcnt %.0f  barrier after mem %.0f\n",
                    blk ? 100 : 0, w, o[0], o[1] / n, o[2] / n, o[3] / n, o[4] / n, o[5] / n, o[6] / n);
        }
    for (int blk = 0; blk < 2; ++blk) {
        const unsigned long long* o = h + 8 + 128 + blk * 16;
        if (!o[11]) continue;
        const double t = (double)o[11];
        fprintf(stderr, "[sqe dbg] wg %d wave 0, cycles per tile: first cmp %.0f + barrier %.0f, mem %.0f + barrier %.0f | last cmp (fast-path test) %.0f + barrier %.0f, "
                        "mem of next tile %.0f + barrier %.0f, tile_end %.0f | %.2f general middle half-steps per tile at %.0f cycles each\n",
                blk ? 100 : 0, o[0] / t, o[1] / t, o[2] / t, o[3] / t, o[4] / t, o[5] / t, o[6] / t, o[7] / t, o[8] / t, o[10] / t,
                o[10] ? (double)o[9] / (double)o[10] : 0.0);
    }
    for (int g = 0; g < 2; ++g) {
        const unsigned long long* o = h + 300 + g * 8;
        if (!o[4]) continue;
        const double n = (double)o[4];
        fprintf(stderr, "[sqe dbg] wg 0 group %d general memory phase x %llu: bookkeeping before %.0f, pieces + reads %.0f, wait %.0f, bookkeeping after %.0f\n",
                g, o[4], o[0] / n, o[1] / n, o[2] / n, o[3] / n);
    }
    // drift between the workgroups that share a DB chunk (STAMPS build): spread of their arrival at two tiles
    if (h[512] && plan.qblocks > 1 && plan.n_chunks * plan.qblocks <= 256) {
        const int G = plan.n_chunks * plan.qblocks;
        double worst[2] = {0, 0}, mean[2] = {0, 0};
        for (int c = 0; c < plan.n_chunks; ++c)
            for (int t = 0; t < 2; ++t) {
                unsigned long long lo = ~0ull, hi = 0;
                for (int qb = 0; qb < plan.qblocks; ++qb) {
                    const int logical = c * plan.qblocks + qb;
                    const int blk = (G & 7) == 0 ? (logical % (G >> 3)) * 8 + logical / (G >> 3) : logical;   // inverse of the kernel's remap
                    const unsigned long long v = h[512 + blk * 2 + t];
                    lo = std::min(lo, v); hi = std::max(hi, v);
                }
                const double d = (double)(hi - lo) / (wall_khz / 1e3);      // microseconds
                worst[t] = std::max(worst[t], d); mean[t] += d / plan.n_chunks;
            }
        fprintf(stderr, "[sqe dbg] spread between the %d workgroups of a chunk when they finish tile 100 / 400: mean %.1f / %.1f us, worst %.1f / %.1f us (one tile = ~30 us)\n",
                plan.qblocks, mean[0], mean[1], worst[0], worst[1]);
    }
    for (int blk = 0; blk < 2; ++blk)
        for (int w = 0; w < 8; ++w) {
            const unsigned long long* o = h + 8 + 160 + blk * 48 + w * 6;
            if (!o[5]) continue;
            const double n = (double)o[5];
            fprintf(stderr, "[sqe dbg] wg %d wave %d tile_end x %llu: mark read %.0f, own slow path %.0f (flagged in %.0f %%), barrier %.0f, entry_sync %.0f\n",
                    blk ? 100 : 0, w, o[5], o[0] / n, o[1] / n, 100.0 * o[4] / n, o[2] / n, o[3] / n);
        }
    return SQE_OK;
}

// ---------------------------------------------------------------- stages of a pass
// The int8 copy of the stored rows (scan_mode INT8) is derived data, filled lazily: the first search after an add
// quantises rows [i8_rows, n) from the fp32 master (one streaming pass, ~5 KiB per row).  Tiles are independent, so a
// grown index keeps what it has.
int ensure_i8_copy(sqe_index* idx, hipStream_t s) {
    const int K = idx->dim;
    const int64_t n_rows = idx->n.load();
    const int64_t cap_tiles = idx->cap / SCAN_BM;
    const int64_t stride = (int64_t)(K / 64) * 16384 + 2048;     // + 2 KiB: chunk streams do not start at the same address modulo 256 KiB
    if (idx->i8_cap_tiles != cap_tiles || idx->i8_tile_stride != stride) {
        DevBuf nd, ns;
        // The copy is derived data (+1 byte per element): an index that fits without it must keep answering.  SQE_ERR_OOM here
        // sends THIS search and every later one to the bf16 scan, which needs no extra memory (admit_i8).
        if (nd.ensure((size_t)cap_tiles * stride) != SQE_OK || ns.ensure((size_t)cap_tiles * SCAN_BM * 4) != SQE_OK) {
            (void)hipGetLastError();
            return SQE_ERR_OOM;
        }
        SQE_HIP(hipMemsetAsync(nd.p, 0, nd.bytes, s));            // rows past n read as zero vectors
        SQE_HIP(hipMemsetAsync(ns.p, 0, ns.bytes, s));
        if (idx->i8_rows > 0 && idx->i8_tile_stride == stride) {
            const int64_t tiles = (idx->i8_rows + SCAN_BM - 1) / SCAN_BM;
            SQE_HIP(hipMemcpyAsync(nd.p, idx->i8db.p, (size_t)tiles * stride, hipMemcpyDeviceToDevice, s));
            SQE_HIP(hipMemcpyAsync(ns.p, idx->i8sxi.p, (size_t)tiles * SCAN_BM * 4, hipMemcpyDeviceToDevice, s));
        } else {
            idx->i8_rows = 0;
        }
        SQE_HIP(hipStreamSynchronize(s));                         // the old buffers die here
        std::swap(nd.p, idx->i8db.p); std::swap(nd.bytes, idx->i8db.bytes);
        std::swap(ns.p, idx->i8sxi.p); std::swap(ns.bytes, idx->i8sxi.bytes);
        idx->i8_cap_tiles = cap_tiles;
        idx->i8_tile_stride = stride;
    }
    if (!idx->i8resid_max.p) {
        SQE_TRY(idx->i8resid_max.ensure(16));
        SQE_HIP(hipMemsetAsync(idx->i8resid_max.p, 0, 16, s));
    }
    if (idx->i8_rows < n_rows) {
        StageTimer t(idx->ctx->prof, s, ST_ADD);
        SQE_TRY(launch_quantize_rows_i8(idx->master, nullptr, idx->i8_rows, n_rows - idx->i8_rows, n_rows, K, idx->i8db.as<int8_t>(), stride,
                                        idx->i8sxi.as<uint32_t>(), idx->i8resid_max.as<uint32_t>(), s));
        idx->i8_rows = n_rows;
        idx->i8_dx_stale = true;
    }
    if (idx->i8_dx_stale) {
        // one 4-byte read-back per batch of newly quantised (or overwritten) rows: the host decides from it whether the
        // int8 bound is worth using at all (admit_i8)
        uint32_t bits = 0;
        SQE_HIP(hipMemcpyAsync(&bits, idx->i8resid_max.p, 4, hipMemcpyDeviceToHost, s));
        SQE_HIP(hipStreamSynchronize(s));
        memcpy(&idx->i8_dx, &bits, 4);
        idx->i8_dx_stale = false;
    }
    return SQE_OK;
}

// Buffers of a pass, the normalised queries (fp32 + bf16) and the zeroed tables of the first pass.
int prepare_pass(Pass& p, const float* q_dev) {
    sqe_index* idx = p.idx;
    sqe_ctx* c = idx->ctx;
    const ScanPlan& plan = p.plan;
    hipStream_t s = p.s;
    const int K = idx->dim, B = p.B;
    SQE_TRY(idx->qn.ensure((size_t)B * K * 4));
    SQE_TRY(idx->qb.ensure((size_t)plan.b_pad * idx->pitch));
    SQE_TRY(idx->cand.ensure((size_t)plan.n_chunks * plan.b_pad * CAND_CAP * 8));
    SQE_TRY(idx->cand_cnt.ensure((size_t)plan.n_chunks * plan.b_pad * 4));
    const size_t gmax_bytes = (size_t)plan.b_pad * plan.ngroups * GMAX_COLS * 4;
    SQE_TRY(idx->gmax.ensure(gmax_bytes));
    // knobs build, timing experiments whose scan scores are wrong on purpose (SQE_DBG=8192): no certificate, no collect pass
    static const bool no_collect = [] { const char* e = knob_env("SQE_NO_COLLECT"); return e && atoi(e) != 0; }();
    p.certify = idx->certify && p.n_rows > 0 && !no_collect;
    SQE_TRY(idx->q_resid.ensure((size_t)B * 4));
    if (p.certify) {
        SQE_TRY(idx->unc.ensure(16 + (size_t)plan.b_pad * 4));
        SQE_TRY(idx->fb_keys.ensure((size_t)B * EXACT_CAP * 8));
        SQE_TRY(idx->fb_cnt.ensure((size_t)B * 4));
        SQE_TRY(idx->unc_ids.ensure((size_t)B * 4));
        SQE_TRY(idx->thr_c.ensure((size_t)(plan.b_pad + 256) * 4));
        if ((size_t)(plan.b_pad + 256) * idx->pitch > idx->qb_c.bytes) {
            SQE_TRY(idx->qb_c.ensure((size_t)(plan.b_pad + 256) * idx->pitch));
            SQE_HIP(hipMemsetAsync(idx->qb_c.p, 0, idx->qb_c.bytes, s));     // rows past the count read as zero
        }
    }
    {
        StageTimer t(c->prof, s, ST_PREP);
        if (plan.b_pad > B)
            SQE_HIP(hipMemsetAsync(idx->qb.as<char>() + (size_t)B * idx->pitch, 0, (size_t)(plan.b_pad - B) * idx->pitch, s));
        SQE_TRY(launch_normalize_rows(q_dev, B, K, K, idx->qn.as<float>(), idx->qb.as<bf16_t>(), idx->pitch / 2,
                                      idx->q_resid.as<float>(), nullptr, s));
        if (p.certify) {
            SQE_HIP(hipMemsetAsync(idx->unc.p, 0, 16, s));
            SQE_HIP(hipMemsetAsync(idx->fb_cnt.p, 0, (size_t)B * 4, s));
        }
        SQE_HIP(hipMemsetAsync(idx->gmax.p, 0, gmax_bytes, s));
    }
    p.unc_count = p.certify ? idx->unc.as<int>() : nullptr;
    p.collect_thr = p.certify ? reinterpret_cast<float*>(idx->unc.as<int>() + 4) : nullptr;
    return SQE_OK;
}

// The sample (every step-th tile, the m-th best of it) that the int8 threshold pass takes from an index of n_rows rows,
// given the options i8_sample_step / i8_sample_m.
std::pair<int, int> sample_plan(int64_t n_rows, int step8, int m8) {
    // The bf16 kernels of the threshold pass exchange their bounds between chunks only when the sample has at least 64
    // chunks (scan.hip: make_scan_plan); below that every workgroup keeps a quarter of its rows and the pass takes three
    // times as long (1.25 M rows -- an eighth of the 10 M-row index, one shard of eight: 0.72 ms against 0.22 ms at
    // 2.5 M).  Small indexes therefore sample MORE tiles (at least 128) and take a deeper place of the sample in proportion,
    // which leaves the expected number of collected rows (~ step x m) where the options put it.
    const int64_t tiles = (n_rows + SCAN_BM - 1) / SCAN_BM;
    const int min_tiles = 2 * GMAX_COLS;
    if (tiles / step8 < min_tiles && tiles / min_tiles >= 1 && tiles / min_tiles < step8) {
        // (the place is capped at 64: the step does not go below what keeps step x m)
        const int step_e = (int)std::max<int64_t>(std::max(1, (step8 * m8 + 63) / 64), tiles / min_tiles);
        const int m_e = std::min(64, std::max(m8, (step8 * m8 + step_e - 1) / step_e));
        step8 = step_e;
        m8 = m_e;
    }
    return {step8, m8};
}

// Whether this pass may take the int8 first pass (*use); fills the int8 copy of the rows when it may.
int admit_i8(const Pass& p, bool* use) {
    sqe_index* idx = p.idx;
    const int K = idx->dim;
    *use = idx->scan_mode == SQE_SCAN_INT8_RESCORE && p.certify && K >= 256 && K % 128 == 0 && p.k <= p.m8 &&
           p.n_rows >= idx->i8_min_rows && p.n_rows >= (int64_t)p.step8 * SCAN_BM * 4;
    if (!*use) return SQE_OK;
    const int rc8 = ensure_i8_copy(idx, p.s);
    if (rc8 == SQE_ERR_OOM) {
        if (!idx->i8_oom_logged) fprintf(stderr, "[sqe] no memory for the int8 copy of the rows: this index answers with the bf16 scan\n");
        idx->i8_oom_logged = true;
        idx->scan_mode = SQE_SCAN_BF16_RESCORE;
        *use = false;
    } else {
        SQE_TRY(rc8);
        *use = idx->i8_dx <= (float)idx->i8_max_resid;  // else: the bf16 first pass
    }
    return SQE_OK;
}

// what the bf16 scan launches of a pass share: the rows, the query block `q`, the candidate lists and the bound table
ScanArgs bf16_scan_args(const Pass& p, const bf16_t* q) {
    sqe_index* idx = p.idx;
    ScanArgs a;
    a.db = idx->scan; a.q = q; a.n_rows = p.n_rows; a.K = idx->dim; a.B = p.B;
    a.db_pitch = idx->pitch; a.q_pitch = idx->pitch;
    a.cand = idx->cand.as<uint64_t>(); a.cand_cnt = idx->cand_cnt.as<int>(); a.gmax = idx->gmax.as<uint32_t>();
    return a;
}

// Second pass for the queries whose certificate failed (bf16 or int8 first pass alike): they are compacted into a
// dense batch on the device, a bf16 collect scan gathers every row whose scan score can still reach the query's k-th
// cosine (collect_thr[q] = that cosine - bf16 eps, +inf for certified queries) and the gathered rows are re-scored in fp32.
int run_collect_fallback(const Pass& p) {
    sqe_index* idx = p.idx;
    sqe_ctx* c = idx->ctx;
    hipStream_t s = p.s;
    const int K = idx->dim, B = p.B;
    {
        StageTimer t(c->prof, s, ST_SELECT);
        SQE_TRY(launch_compact_uncertified(p.collect_thr, B, idx->qb.as<bf16_t>(), idx->pitch, K * 2, idx->unc_ids.as<int>(),
                                           idx->thr_c.as<float>(), p.plan.b_pad + 256, idx->qb_c.as<bf16_t>(), p.unc_count, s));
    }
    {
        // The collect scans are scans: they are booked under scan_ms (scan_calls counts the main launches
        // only).  One launch per range of counts is enqueued, each planned like a search of that batch size
        // and returning at once unless the count is in its range (and at once when it is 0).
        StageTimer t(c->prof, s, ST_COLLECT);
        ScanArgs a = bf16_scan_args(p, idx->qb_c.as<bf16_t>());
        a.collect_thr = idx->thr_c.as<float>(); a.collect_keys = idx->fb_keys.as<uint64_t>(); a.collect_cnt = idx->fb_cnt.as<int>();
        a.unc_count = p.unc_count;
        const int bounds[5] = {0, 64, 256, 512, 1 << 30};
        for (int r = 0; r < 4 && bounds[r] < B; ++r) {
            const int hi = std::min(bounds[r + 1], B);
            const ScanPlan cp = make_scan_plan(p.n_rows, hi, p.kp, c->cu_count);
            a.collect_lo = bounds[r] + 1;
            a.collect_hi = r == 3 ? (1 << 30) : bounds[r + 1];
            SQE_TRY(launch_scan_collect(cp, a, s));
        }
    }
    {
        // ... and re-score them in fp32
        StageTimer t(c->prof, s, ST_SELECT);
        ExactArgs e;
        e.master = idx->master; e.qn = idx->qn.as<float>(); e.K = K; e.B = B; e.k = p.k;
        e.collect_thr = p.collect_thr; e.keys = idx->fb_keys.as<uint64_t>(); e.key_cnt = idx->fb_cnt.as<int>();
        e.unc_ids = idx->unc_ids.as<int>(); e.unc_count = p.unc_count;
        e.cos_out = p.cos_out; e.id_out = p.id_out; e.id_base = search_id_base(idx);
        SQE_TRY(launch_collect_rescore(e, s));
    }
    // the count goes to a buffer the CONTEXT owns (sqe_stats reads it long after this index may be gone); the
    // passes of a batch above MAX_PASS add up (r02: the last pass's count overwrote the others)
    if (p.pass_index == 0) SQE_HIP(hipMemcpyAsync(c->unc_last.p, p.unc_count, 4, hipMemcpyDeviceToDevice, s));
    else hipLaunchKernelGGL(add_count_kernel, dim3(1), dim3(1), 0, s, c->unc_last.as<int>(), p.unc_count);
    c->unc_valid.store(true);
    return SQE_OK;
}

// Threshold pass of the int8 first pass: per query the integer collect threshold (i8thr_int / i8thr_eff) and the best
// true cosines of the row sample (i8cos_s / i8ids_s).  *chunks_used: chunks of the int8 form (0 in the bf16 form).
int i8_threshold_pass(const Pass& p, int b_pad_s, int n_tiles_i8s, bool sample_i8, int* chunks_used) {
    sqe_index* idx = p.idx;
    sqe_ctx* c = idx->ctx;
    const ScanPlan& plan = p.plan;
    hipStream_t s = p.s;
    const int K = idx->dim, B = p.B, step8 = p.step8, m8 = p.m8;
    *chunks_used = 0;
    if (sample_i8) {
        // threshold pass in int8 (r03c): the collect scan's own tile loop over every step-th tile, two best scores per lane,
        // then per query the m-th largest of them (scan_i8.hip: sample_i8_pp_kernel; select_i8.hip: i8_sample_select_kernel)
        StageTimer t(c->prof, s, ST_SAMPLE);
        const int qblocks_s = b_pad_s / 256;
        const int chunks_s = std::max(1, std::min(std::min(c->cu_count / qblocks_s, 256), n_tiles_i8s));
        *chunks_used = chunks_s;
        SQE_TRY(idx->i8samp.ensure((size_t)chunks_s * b_pad_s * 16 * 8));
        I8SampleArgs sp;
        sp.db8 = idx->i8db.as<int8_t>(); sp.tile_stride = idx->i8_tile_stride; sp.sxi = idx->i8sxi.as<uint32_t>();
        sp.q8t = idx->q8t.as<int8_t>(); sp.K = K; sp.b_pad = b_pad_s; sp.n_tiles_s = n_tiles_i8s; sp.step = step8;
        sp.n_chunks = chunks_s; sp.out = idx->i8samp.p;
        SQE_TRY(launch_sample_i8(sp, s));
        I8SampleSelectArgs ss;
        ss.cand = idx->i8samp.p; ss.n_chunks = chunks_s; ss.b_pad_s = b_pad_s; ss.m = m8; ss.k = p.k; ss.B = B; ss.b_pad = plan.b_pad; ss.K = K;
        ss.sqi = idx->q8sqi.as<uint32_t>(); ss.master = idx->master; ss.qn = idx->qn.as<float>();
        ss.thr_int = idx->i8thr_int.as<int>(); ss.thr_eff = idx->i8thr_eff.as<float>();
        ss.sample_cos = idx->i8cos_s.as<float>(); ss.sample_ids = idx->i8ids_s.as<int64_t>();
        ss.q_resid8 = idx->q8resid.as<float>(); ss.db_resid8_max = idx->i8resid_max.as<uint32_t>();
        ss.margin = (float)idx->i8_anchor_margin; ss.step = step8; ss.key_budget = idx->i8_key_budget;
        SQE_TRY(launch_i8_sample_select(ss, s));
    } else {
        // threshold pass: the bf16 scan + fp32 re-score of the row sample, top-m true cosines per query
        StageTimer t(c->prof, s, ST_SAMPLE);
        const int n_tiles_s = (plan.n_tiles + step8 - 1) / step8;
        const ScanPlan ps = make_scan_plan((int64_t)n_tiles_s * SCAN_BM, B, auto_kp(idx, m8), c->cu_count, m8);
        ScanArgs a = bf16_scan_args(p, idx->qb.as<bf16_t>());
        a.q_resid = idx->q_resid.as<float>(); a.db_resid_max = idx->resid_max.as<uint32_t>();
        a.tile_step = step8;
        SQE_TRY(launch_scan_bf16(ps, a, s));
        SelectArgs sa;
        sa.cand = idx->cand.as<uint64_t>(); sa.cand_cnt = idx->cand_cnt.as<int>();
        sa.n_chunks = ps.n_chunks; sa.b_pad = ps.b_pad; sa.kp = ps.kp;
        sa.master = idx->master; sa.qn = idx->qn.as<float>(); sa.K = K; sa.B = B; sa.k = m8;
        sa.cos_out = idx->i8cos_s.as<float>(); sa.id_out = idx->i8ids_s.as<int64_t>();
        SQE_TRY(launch_select_rescore(sa, s));
        SQE_TRY(launch_i8_thresholds(idx->i8cos_s.as<float>(), m8, idx->q8sqi.as<uint32_t>(), K, B, plan.b_pad,
                                     idx->i8thr_int.as<int>(), idx->i8thr_eff.as<float>(), s));
    }
    return SQE_OK;
}

// int8 collect scan over all rows at the fixed thresholds, then the staged fp32 re-score with the certificate
// keep_trace: null, or [B][4] for select_i8_kernel's per-query trace ("i8_keep_select")
int i8_scan_select(const Pass& p, int q8_pitch, int* keep_trace) {
    sqe_index* idx = p.idx;
    sqe_ctx* c = idx->ctx;
    const ScanPlan& plan = p.plan;
    hipStream_t s = p.s;
    const int K = idx->dim, B = p.B;
    {
        StageTimer t(c->prof, s, ST_SCAN);
        I8ScanArgs ia;
        ia.db8 = idx->i8db.as<int8_t>(); ia.tile_stride = idx->i8_tile_stride; ia.sxi = idx->i8sxi.as<uint32_t>();
        ia.q8 = idx->q8.as<int8_t>(); ia.q_pitch = q8_pitch; ia.q8t = idx->q8t.as<int8_t>(); ia.thr_int = idx->i8thr_int.as<int>();
        ia.n_rows = p.n_rows; ia.K = K; ia.B = B; ia.b_pad = plan.b_pad; ia.n_tiles = plan.n_tiles; ia.n_chunks = plan.n_chunks;
        ia.qblocks = plan.qblocks; ia.bn = plan.bn; ia.cand = idx->cand.as<uint64_t>(); ia.cand_cnt = idx->cand_cnt.as<int>();
        ia.ovf = idx->i8ovf.as<uint64_t>(); ia.ovf_cnt = idx->i8ovf_cnt.as<int>();
        idx->i8_launch.kernel = 0; ia.kernel = &idx->i8_launch.kernel;        // the launcher says which kernel it picked
        if (i8_stamps_wanted()) SQE_TRY(arm_dbg(idx, s, &ia.stamps));
        static const int deep_max = [] { const char* e = knob_env("SQE_I8_DEEP_MAX"); return e ? atoi(e) : 1; }();   // knobs build: A/B of the cut
        if (plan.bn == 256 && plan.qblocks <= deep_max) SQE_TRY(launch_scan_i8_deep(ia, s));      // (scan_i8_deep.hip)
        else SQE_TRY(launch_scan_i8(ia, s));
        if (i8_stamps_wanted()) SQE_TRY(report_i8_stamps(idx, s));
    }
    {
        StageTimer t(c->prof, s, ST_SELECT);
        I8SelectArgs sa;
        sa.cand = idx->cand.as<uint64_t>(); sa.cand_cnt = idx->cand_cnt.as<int>(); sa.n_chunks = plan.n_chunks; sa.b_pad = plan.b_pad;
        sa.master = idx->master; sa.qn = idx->qn.as<float>(); sa.K = K; sa.B = B; sa.k = p.k;
        sa.scan16 = idx->scan; sa.pitch16 = idx->pitch;
        sa.sxi = idx->i8sxi.as<uint32_t>(); sa.sqi = idx->q8sqi.as<uint32_t>();
        sa.q_resid8 = idx->q8resid.as<float>(); sa.db_resid8_max = idx->i8resid_max.as<uint32_t>();
        sa.q_resid16 = idx->q_resid.as<float>(); sa.db_resid16_max = idx->resid_max.as<uint32_t>();
        sa.thr_eff = idx->i8thr_eff.as<float>();
        sa.sample_cos = idx->i8cos_s.as<float>(); sa.sample_ids = idx->i8ids_s.as<int64_t>(); sa.sample_m = p.m8;
        sa.cos_out = p.cos_out; sa.id_out = p.id_out; sa.id_base = search_id_base(idx);
        sa.unc_count = p.unc_count; sa.collect_thr = p.collect_thr;
        sa.stats = idx->i8stats.as<unsigned long long>();
        sa.ovf = idx->i8ovf.as<uint64_t>(); sa.ovf_cnt = idx->i8ovf_cnt.as<int>();
        sa.trace = keep_trace;
        SQE_TRY(launch_select_i8(sa, s));
    }
    return SQE_OK;
}

// ---- int8 first pass (scan_mode INT8): threshold pass on a row sample (bf16 kernels, every step-th tile) -> fixed
// per-query collect thresholds -> int8 collect scan over all rows -> staged fp32 re-score + certificate -> the bf16
// collect pass for what is left.  Small indexes give the sample nothing to estimate from: they stay with the bf16 scan.
int i8_first_pass(const Pass& p) {
    sqe_index* idx = p.idx;
    sqe_ctx* c = idx->ctx;
    const ScanPlan& plan = p.plan;
    hipStream_t s = p.s;
    const int K = idx->dim, B = p.B, step8 = p.step8, m8 = p.m8;
    const int q8_pitch = K + 128;
    // the int8 threshold pass runs on query blocks of 256 whatever the batch (1 % of the tiles: padding costs nothing)
    const int b_pad_s = (B + 255) / 256 * 256;
    const int b_pad_q = std::max(plan.b_pad, b_pad_s);
    const int64_t full_tiles = p.n_rows / SCAN_BM;
    const int n_tiles_i8s = (int)(full_tiles / step8);          // sampled tiles t * step8, whole tiles only
    const bool sample_i8 = idx->i8_sample_int8 != 0 && n_tiles_i8s >= 1;
    SQE_TRY(idx->q8.ensure((size_t)b_pad_q * q8_pitch));
    const size_t q8t_block = (size_t)256 * K;                   // the tiled copy: whole 256-query blocks
    const size_t q8t_blocks = ((size_t)b_pad_q + 255) / 256;
    SQE_TRY(idx->q8t.ensure(q8t_blocks * q8t_block));
    SQE_TRY(idx->q8sqi.ensure((size_t)b_pad_q * 4));
    SQE_TRY(idx->q8resid.ensure((size_t)plan.b_pad * 4));
    SQE_TRY(idx->i8thr_int.ensure((size_t)plan.b_pad * 4));
    SQE_TRY(idx->i8thr_eff.ensure((size_t)plan.b_pad * 4));
    SQE_TRY(idx->i8cos_s.ensure((size_t)B * m8 * 4));
    SQE_TRY(idx->i8ids_s.ensure((size_t)B * m8 * 8));
    SQE_TRY(idx->i8stats.ensure(64));
    SQE_TRY(idx->i8ovf.ensure((size_t)plan.b_pad * I8_OVF_CAP * 8));
    SQE_TRY(idx->i8ovf_cnt.ensure((size_t)plan.b_pad * 4));
    {
        StageTimer t(c->prof, s, ST_PREP);
        SQE_HIP(hipMemsetAsync(idx->i8ovf_cnt.p, 0, (size_t)plan.b_pad * 4, s));
        if (b_pad_q > B)
            SQE_HIP(hipMemsetAsync(idx->q8.as<char>() + (size_t)B * q8_pitch, 0, (size_t)(b_pad_q - B) * q8_pitch, s));
        if (B % 256 != 0)                                       // the block the last queries share with padding (and any block behind it)
            SQE_HIP(hipMemsetAsync(idx->q8t.as<char>() + (size_t)(B / 256) * q8t_block, 0, (q8t_blocks - (size_t)(B / 256)) * q8t_block, s));
        SQE_TRY(launch_quantize_queries_i8(idx->qn.as<float>(), B, K, idx->q8.as<int8_t>(), q8_pitch, idx->q8t.as<int8_t>(),
                                           idx->q8sqi.as<uint32_t>(), idx->q8resid.as<float>(), s));
        SQE_HIP(hipMemsetAsync(idx->i8stats.p, 0, 64, s));
    }
    int chunks_s_used = 0;
    SQE_TRY(i8_threshold_pass(p, b_pad_s, n_tiles_i8s, sample_i8, &chunks_s_used));
    // "i8_keep_select" (test-only): what select_i8_kernel wrote is copied aside before the bf16 collect pass overwrites the
    // answers of the uncertified queries; without the option nothing below allocates, copies or launches
    const bool keep = idx->i8_keep_select != 0;
    if (keep) {
        SQE_TRY(idx->i8keep_cos.ensure((size_t)B * p.k * 4));
        SQE_TRY(idx->i8keep_ids.ensure((size_t)B * p.k * 8));
        SQE_TRY(idx->i8keep_thr.ensure((size_t)plan.b_pad * 4));
        SQE_TRY(idx->i8keep_trace.ensure((size_t)B * 16));
    }
    idx->i8_kept = false;
    SQE_TRY(i8_scan_select(p, q8_pitch, keep ? idx->i8keep_trace.as<int>() : nullptr));
    if (keep) {
        SQE_HIP(hipMemcpyAsync(idx->i8keep_cos.p, p.cos_out, (size_t)B * p.k * 4, hipMemcpyDeviceToDevice, s));
        SQE_HIP(hipMemcpyAsync(idx->i8keep_ids.p, p.id_out, (size_t)B * p.k * 8, hipMemcpyDeviceToDevice, s));
        SQE_HIP(hipMemcpyAsync(idx->i8keep_thr.p, p.collect_thr, (size_t)plan.b_pad * 4, hipMemcpyDeviceToDevice, s));
        idx->i8_kept = true;
    }
    SQE_TRY(run_collect_fallback(p));
    {
        sqe_i8_launch_t& L = idx->i8_launch;           // what sqe_index_i8_last reports (the uncertified count is read there)
        L.rows = p.n_rows; L.tile_stride = idx->i8_tile_stride; L.dim = K; L.B = B; L.b_pad = plan.b_pad; L.k = p.k;
        L.tile_rows = SCAN_BM; L.q_pitch = q8_pitch; L.query_block = plan.bn; L.n_chunks = plan.n_chunks; L.list_cap = CAND_CAP; L.pool_cap = I8_OVF_CAP;
        L.sample_int8 = sample_i8 ? 1 : 0; L.sample_step = step8; L.sample_tiles = n_tiles_i8s;
        L.sample_chunks = chunks_s_used;
        L.sample_b_pad = b_pad_s; L.sample_m = m8; L.uncertified = -1;
    }
    SQE_HIP(hipMemcpyAsync(c->i8_last.p, idx->i8stats.p, 32, hipMemcpyDeviceToDevice, s));
    c->i8_valid.store(true);
    return SQE_OK;
}

// bf16 first pass: scan with the fused top-k filter, then select + fp32 rescore + certificate
// *info: what the scan launch ran with (untouched when the index is empty and nothing is launched)
int bf16_first_pass(const Pass& p, ScanLaunchInfo* info) {
    sqe_index* idx = p.idx;
    sqe_ctx* c = idx->ctx;
    const ScanPlan& plan = p.plan;
    hipStream_t s = p.s;
    if (p.n_rows > 0) {
        StageTimer t(c->prof, s, ST_SCAN);
        ScanArgs a = bf16_scan_args(p, idx->qb.as<bf16_t>());
        a.q_resid = idx->q_resid.as<float>(); a.db_resid_max = idx->resid_max.as<uint32_t>();   // the k-row bound's eps
        if (scan_counters_wanted()) SQE_TRY(arm_dbg(idx, s, &a.dbg_counters));
        a.info = info;
        SQE_TRY(launch_scan_bf16(plan, a, s));
    } else {
        SQE_HIP(hipMemsetAsync(idx->cand_cnt.p, 0, (size_t)plan.n_chunks * plan.b_pad * 4, s));
    }
    {
        StageTimer t(c->prof, s, ST_SELECT);
        SelectArgs sa;
        sa.cand = idx->cand.as<uint64_t>(); sa.cand_cnt = idx->cand_cnt.as<int>();
        sa.n_chunks = plan.n_chunks; sa.b_pad = plan.b_pad; sa.kp = p.kp;
        sa.master = idx->master; sa.qn = idx->qn.as<float>(); sa.K = idx->dim; sa.B = p.B; sa.k = p.k;
        sa.cos_out = p.cos_out; sa.id_out = p.id_out; sa.id_base = search_id_base(idx);
        sa.q_resid = p.certify ? idx->q_resid.as<float>() : nullptr;
        sa.db_resid_max = p.certify ? idx->resid_max.as<uint32_t>() : nullptr;
        sa.unc_count = p.unc_count; sa.collect_thr = p.collect_thr;
        sa.gmax = (p.n_rows > 0 && plan.gshift >= 0) ? idx->gmax.as<uint32_t>() : nullptr; sa.gshift = plan.gshift;
        SQE_TRY(launch_select_rescore(sa, s));
    }
    return SQE_OK;
}

// what sqe_stats reports of the last search; elem_bytes = bytes per stored element the first pass read (1 int8, 2 bf16)
void book_search(const Pass& p, int elem_bytes) {
    sqe_ctx* c = p.idx->ctx;
    const int64_t K = p.idx->dim;
    c->search_calls++;
    c->last_scan_rows.store(p.n_rows);
    c->last_scan_flops.store(2 * p.n_rows * K * p.B);
    c->last_scan_bytes.store(p.n_rows * K * elem_bytes + (int64_t)p.B * K * 4 + (int64_t)p.B * p.k * 12);
}

// The search pipeline on stream s (caller holds the index lock): query normalise -> bf16 scan with the fused
// top-k filter -> select + fp32 rescore + certificate -> collect pass for uncertified queries; where admit_i8 allows
// it the int8 first pass takes the place of the bf16 scan and select.
// The search over row POSITIONS; index_search_impl maps them to ids when the index has had deletes.
int search_positions(sqe_index* idx, const float* q_dev, int B, int k, int nprobe, float* cos_out_dev, int64_t* id_out_dev,
                     hipStream_t s, int pass_index) {
    sqe_ctx* c = idx->ctx;
    if (idx->ivf) {
        StageTimer t(c->prof, s, ST_SCAN);
        SQE_TRY(ivf_search(idx, idx->ivf, q_dev, B, k, nprobe > 0 ? nprobe : idx->nprobe, cos_out_dev, id_out_dev, s));
        c->search_calls++;
        return SQE_OK;
    }
    const int K = idx->dim;
    // More than four 256-query blocks would leave fewer than 64 DB chunks (one workgroup per CU), too few to
    // fill a row of the global-bound table: the filter would lose its cross-chunk threshold.  Larger batches
    // run as passes of 1024 queries, each at the full-batch rate.
    constexpr int MAX_PASS = 1024;
    if (B > MAX_PASS) {
        for (int off = 0; off < B; off += MAX_PASS) {
            const int m = std::min(MAX_PASS, B - off);
            SQE_TRY(search_positions(idx, q_dev + (size_t)off * K, m, k, nprobe, cos_out_dev + (size_t)off * k,
                                     id_out_dev + (size_t)off * k, s, off / MAX_PASS));
        }
        return SQE_OK;
    }
    Pass p{};
    p.idx = idx; p.s = s; p.n_rows = idx->n.load(); p.B = B; p.k = k; p.kp = auto_kp(idx, k);
    p.plan = make_scan_plan(p.n_rows, B, p.kp, c->cu_count, k);
    p.cos_out = cos_out_dev; p.id_out = id_out_dev; p.pass_index = pass_index;
    SQE_TRY(prepare_pass(p, q_dev));
    std::tie(p.step8, p.m8) = sample_plan(p.n_rows, idx->i8_sample_step, idx->i8_sample_m);
    bool use_i8 = false;
    SQE_TRY(admit_i8(p, &use_i8));
    if (use_i8) {
        idx->scan_launch.rows = 0;       // not the bf16 first pass
        SQE_TRY(i8_first_pass(p));
    } else {
        c->i8_valid.store(false);        // this search runs the bf16 first pass
        ScanLaunchInfo info;
        SQE_TRY(bf16_first_pass(p, &info));
        if (p.certify) SQE_TRY(run_collect_fallback(p));
        {
            sqe_scan_launch_t& L = idx->scan_launch;      // what sqe_index_scan_last reports (the uncertified count is read there)
            const ScanPlan& pl = p.plan;
            L.rows = p.n_rows; L.dim = K; L.B = B; L.k = k; L.kp = p.kp; L.bn = pl.bn; L.qblocks = pl.qblocks; L.b_pad = pl.b_pad;
            L.n_tiles = pl.n_tiles; L.n_chunks = pl.n_chunks; L.tiles_per_chunk = pl.tiles_per_chunk; L.ngroups = pl.ngroups;
            L.trig = info.trig; L.gshift = info.gshift; L.gshift_k = info.gshift_k; L.k_rows = info.k_rows;
            L.list_cap = CAND_CAP; L.exact_cap = EXACT_CAP;
            L.family = info.pingpong ? SQE_SCAN_FAMILY_PINGPONG : SQE_SCAN_FAMILY_STAGED; L.nst = info.nst; L.nstb = info.nstb;
            L.certified = p.certify ? 1 : 0; L.uncertified = -1;
        }
        SQE_TRY(report_scan_counters(p));
    }
    idx->last_B = B; idx->last_i8 = use_i8;       // what sqe_index_state_read may copy out
    book_search(p, use_i8 ? 1 : 2);
    return SQE_OK;
}

}  // namespace

int index_search_positions(sqe_index* idx, const float* q_dev, int B, int k, int nprobe, float* cos_out_dev, int64_t* id_out_dev,
                           hipStream_t s) {
    return search_positions(idx, q_dev, B, k, nprobe, cos_out_dev, id_out_dev, s, 0);
}

int index_search_impl(sqe_index* idx, const float* q_dev, int B, int k, int nprobe, float* cos_out_dev, int64_t* id_out_dev,
                      hipStream_t s, int pass_index) {
    SQE_TRY(search_positions(idx, q_dev, B, k, nprobe, cos_out_dev, id_out_dev, s, pass_index));
    // an index with deletes: positions -> ids (+ id_base) on the device, in stream order (compact.hip)
    return index_translate_ids(idx, id_out_dev, (int64_t)B * k, s);
}

}  // namespace sqe
