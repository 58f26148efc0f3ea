// ivf_select.hip -- the select kernels of the IVF search and their launchers (ivf_kernels.h), one workgroup per query each:
// the coarse-probe select behind ivf_coarse_topk (S5), the collect threshold from the sample strips, and the two final
// selects (over the strips, over a collect list), which re-score their kp best estimates in fp32 against the master and
// write the top-k.  All radix selects go through block_select.h but ivf_select_list_kernel's (the comment at the site).
// Called from ivf.hip only.
#include "block_select.h"
#include "ivf_kernels.h"

namespace sqe {

namespace {

// top-nprobe lists of a query from its dense coarse scores [nlist] (score desc, list id asc); one workgroup
// per query, scores staged in LDS, byte-wise radix select on (orderable score, ~id) keys
// The GEMM scores come from bf16 operands: the best nprobe + 8 by those scores are re-scored in fp32 (raw query
// row against the normalised fp32 centroid; dividing by the query norm does not change the order) and the
// best nprobe of them returned, so the list order is the exact fp32 one.
constexpr int PSEL_THREADS = 1024;      // (r04; 256 before: the re-score of the nprobe + 8 best centroids is a chain of row fetches per wave)
__global__ __launch_bounds__(PSEL_THREADS) void ivf_probe_select_kernel(const float* __restrict__ scores, int nlist, int nprobe,
                                                               const float* __restrict__ rows, const float* __restrict__ cent, int dim,
                                                               int64_t* __restrict__ probes, float* __restrict__ probes_cos) {
    extern __shared__ __attribute__((aligned(16))) float ssc[];      // [nlist]
    __shared__ int hist[256];
    __shared__ uint64_t top[MAX_KP];
    const int q = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < nlist; i += PSEL_THREADS) ssc[i] = scores[(size_t)q * nlist + i];
    __syncthreads();
    auto visit = each_key<PSEL_THREADS>([&](int i) { return make_key(ssc[i] + 0.0f, (uint32_t)i); }, nlist);
    const int nsel = min(min(nprobe + 8, MAX_KP), nlist);      // candidates kept for the fp32 re-score
    // (keys are unique, so the select stops early: r04c, three or four passes of the eight on scores that differ)
    const uint64_t T = nlist > nsel ? block_select_kth<PSEL_THREADS, uint64_t, true>(visit, nsel, hist) : 0ull;
    const int m = min(block_collect_top(visit, T, top), nsel);
    {
        const int lane = tid & 63, wave = tid >> 6;
        const float4* qv = reinterpret_cast<const float4*>(rows + (size_t)q * dim);
        const int nvec = dim >> 2;
        float qq = 0.f;
        for (int v4 = lane; v4 < nvec; v4 += 64) {
            const float4 b = qv[v4];
            qq = fmaf(b.x, b.x, qq); qq = fmaf(b.y, b.y, qq); qq = fmaf(b.z, b.z, qq); qq = fmaf(b.w, b.w, qq);
        }
        const float inv = 1.0f / (sqrtf(wave_sum(qq)) + 1e-9f);
        for (int e = wave; e < m; e += PSEL_THREADS / 64) {
            const uint32_t id = key_row(top[e]);
            const float4* cv = reinterpret_cast<const float4*>(cent + (size_t)id * dim);
            float s = 0.f;
            for (int v4 = lane; v4 < nvec; v4 += 64) {
                const float4 a = cv[v4], b = qv[v4];
                s = fmaf(a.x, b.x, s); s = fmaf(a.y, b.y, s); s = fmaf(a.z, b.z, s); s = fmaf(a.w, b.w, s);
            }
            s = wave_sum(s) * inv + 0.0f;
            if (lane == 0) top[e] = make_key(s, id);
        }
    }
    __syncthreads();
    block_rank_write<PSEL_THREADS>(top, m, nprobe, probes_cos + (size_t)q * nprobe, probes + (size_t)q * nprobe,
                                   [](uint32_t list) { return (int64_t)list; });
}

// Threshold of a query for the collect pass, from the sample strips (the first min(256, len) scores of each of its probed lists): the
// r-th largest sample score, r placed so that ~8 kp rows of the whole probed set are expected at or above it (r = 8 kp x sample
// fraction, plus three standard deviations of that count and 2), and the sample's own entries at or above it start the query's list.
// A probed set small enough to fit the list whole gets -inf.  One workgroup of 1,024 threads per query (r04c; 256 before: the sample
// came in as 32 dependent round trips, one strip after the other -- 36 us for a kernel that moves 32 KiB): 32 threads per strip, the
// eight loads of a thread issued together.
constexpr int THR_THREADS = 1024;
__global__ __launch_bounds__(THR_THREADS) void ivf_threshold_kernel(const int64_t* __restrict__ probes, const int64_t* __restrict__ offsets,
                                                            const int* __restrict__ order, const float* __restrict__ pair_scores,
                                                            int nprobe, int max_len, int kp, float* __restrict__ thr_out,
                                                            int* __restrict__ cnt, uint64_t* __restrict__ list) {
    __shared__ uint32_t samp[MAX_KP * 32];                   // up to 256 scores of each of up to 32 probed lists... (nprobe <= 32 here)
    __shared__ int s_len[32], s_pos[33];
    __shared__ int64_t s_off[32];
    __shared__ int hist[256];
    __shared__ int s_total, s_listed;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_listed = 0;
    if (tid < nprobe) {
        const int64_t L = probes[(size_t)q * nprobe + tid];
        const int64_t off = L >= 0 ? offsets[L] : 0;
        s_off[tid] = off;
        s_len[tid] = L >= 0 ? (int)(offsets[L + 1] - off) : 0;
    }
    __syncthreads();
    if (tid == 0) {
        int pos = 0, total = 0;
        for (int p = 0; p < nprobe; ++p) { s_pos[p] = pos; pos += min(s_len[p], LS_ROWS); total += s_len[p]; }
        s_pos[nprobe] = pos;
        s_total = total;
    }
    __syncthreads();
    const int S = s_pos[nprobe], total = s_total;
    {
        const int p = tid >> 5, sub = tid & 31;                // (nprobe <= 32: the host takes this mode only then)
        if (p < nprobe) {
            const int n = s_pos[p + 1] - s_pos[p];
            const float* strip = pair_scores + ((size_t)q * nprobe + p) * max_len;
            float v[LS_ROWS / 32];
#pragma unroll
            for (int j = 0; j < LS_ROWS / 32; ++j) v[j] = sub + 32 * j < n ? strip[sub + 32 * j] : 0.f;
#pragma unroll
            for (int j = 0; j < LS_ROWS / 32; ++j)
                if (sub + 32 * j < n) samp[s_pos[p] + sub + 32 * j] = v[j] == v[j] ? f32_orderable(v[j] + 0.0f) : 0u;      // (NaN rows never rank)
        }
    }
    __syncthreads();
    uint32_t thr = 0;                                          // orderable -inf: everything
    if (total > IVF_LIST_CAP / 4 && S > 0) {
        const float t = 8.0f * (float)kp * (float)S / (float)total;
        const int want = min(S, (int)(t + 3.0f * sqrtf(t) + 2.0f));
        // (the NaN placeholders are no keys: with fewer than `want` scores the threshold is 0, otherwise they lie below it)
        thr = block_select_kth<THR_THREADS, uint32_t, false>(each_key<THR_THREADS>([&](int i) { return samp[i]; }, S), want, hist);
    }
    // the sample's own entries at or above the threshold open the list
    {
        const int p = tid >> 5, sub = tid & 31;
        if (p < nprobe) {
            const int n = s_pos[p + 1] - s_pos[p];
            for (int i = sub; i < n; i += 32) {
                const uint32_t v32 = samp[s_pos[p] + i];
                if (v32 != 0u && v32 >= thr) {
                    const int slot = atomicAdd(&s_listed, 1);
                    if (slot < IVF_LIST_CAP) list[(size_t)q * IVF_LIST_CAP + slot] = make_key(f32_from_orderable(v32), (uint32_t)order[s_off[p] + i]);
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        cnt[q] = s_listed;
        cnt[gridDim.x + q] = total;                            // (ivf_select_list_kernel: a list shorter than min(kp, total) cannot answer)
        thr_out[q] = thr == 0u ? -INFINITY : f32_from_orderable(thr);
    }
}

// per query: the kp best scan scores over the strips of its probed lists, re-scored in fp32 against the
// master, then the top-k by (fp32 cosine desc, row id asc)
// 1,024 threads per query (r04; 256 before): the strip passes and the re-score are chains of dependent loads per wave -- one query
// alone took 83 us here, of a 196 us search (profiles/r04_configs/ivf_stream_ablation.log) -- sixteen waves shorten every chain fourfold.
constexpr int SEL_THREADS = 1024, SEL_WAVES = SEL_THREADS / 64;
// fp32 re-score of the kept rows top[0 .. m) against the master: out[e] = (exact cosine, row).  One wave per row; every thread of the
// block calls (SEL_WAVES waves); out may be top.
__device__ __forceinline__ void rescore_top(const uint64_t* top, uint64_t* out, int m, const float* __restrict__ master,
                                            const float* __restrict__ qrow, int K, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const float4* qv = reinterpret_cast<const float4*>(qrow);
    const int nvec = K >> 2;
    if (K == 1024 && m <= 3 * SEL_WAVES) {
        // the usual shape (kp = 40 rows of 4 KiB, sixteen waves): a wave's up to three rows are random rows of the master, each a full
        // memory round trip (and a TLB miss) -- all their loads are issued before the first sum, one round trip instead of three
        float4 a[3][4], b[4];
        uint32_t rows[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int e = wave + r * SEL_WAVES;
            rows[r] = e < m ? key_row(top[e]) : 0u;
            const float4* rv = reinterpret_cast<const float4*>(master + (size_t)rows[r] * K);
#pragma unroll
            for (int i = 0; i < 4; ++i) a[r][i] = e < m ? rv[lane + 64 * i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = qv[lane + 64 * i];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int e = wave + r * SEL_WAVES;
            float sc = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {          // (rescore_row's order: same bits)
                sc = fmaf(a[r][i].x, b[i].x, sc); sc = fmaf(a[r][i].y, b[i].y, sc);
                sc = fmaf(a[r][i].z, b[i].z, sc); sc = fmaf(a[r][i].w, b[i].w, sc);
            }
            sc = wave_sum(sc) + 0.0f;
            if (lane == 0 && e < m) out[e] = make_key(sc, rows[r]);
        }
        return;
    }
    for (int e = wave; e < m; e += SEL_WAVES) {
        const uint32_t row = key_row(top[e]);
        const float sc = rescore_row(reinterpret_cast<const float4*>(master + (size_t)row * K), qv, nvec, lane);
        if (lane == 0) out[e] = make_key(sc, row);
    }
}

__global__ __launch_bounds__(SEL_THREADS) void ivf_select_kernel(const int64_t* __restrict__ probes, const int64_t* __restrict__ offsets,
                                                         const int* __restrict__ order, const float* __restrict__ pair_scores,
                                                         int nprobe, int max_len, int k, int kp, int64_t id_base,
                                                         const float* __restrict__ master, const float* __restrict__ qn, int K,
                                                         float* __restrict__ cos_out, int64_t* __restrict__ id_out, const int* __restrict__ gate) {
    __shared__ int hist[256];
    __shared__ int s_ns, s_nc;                       // sample scores, collected keys of the fast path
    __shared__ uint64_t top[MAX_KP];
    if (gate && *gate == 0) return;                  // (the strip-mode fallback of a collect search: only if some query asked for it)
    const int q = blockIdx.x, tid = threadIdx.x;
    auto key_at = [&](int p, int i, int64_t off) {
        return make_key(pair_scores[((size_t)q * nprobe + p) * max_len + i], (uint32_t)order[off + i]);
    };
    // the query's probed lists into LDS once (r04: every pass below used to re-read probes / offsets list by list, a chain of
    // dependent loads per list; batch 1024: 476 us for the kernel)
    __shared__ int s_len[MAX_KP];
    __shared__ int64_t s_off[MAX_KP];
    __shared__ int s_total;
    if (tid == 0) s_total = 0;
    __syncthreads();
    for (int p = tid; p < nprobe; p += SEL_THREADS) {
        const int64_t L = probes[(size_t)q * nprobe + p];
        const int64_t off = L >= 0 ? offsets[L] : 0;
        const int len = L >= 0 ? (int)(offsets[L + 1] - off) : 0;
        s_off[p] = off;
        s_len[p] = len;
        if (len) atomicAdd(&s_total, len);
    }
    __syncthreads();
    const int total = s_total;                       // total number of probed rows
    const int wave4 = tid >> 6, lane64 = tid & 63;          // (wave4: one of SEL_WAVES)
    // ---- fast path: a threshold from a strided sample, ONE pass over the strips that collects every key
    // at or above it, exact top-kp among the few collected.  (The general path below walks the strips
    // eight times; it remains the fallback when the sample misjudges the tail.)  One wave per strip in both passes.
    constexpr int SAMPLE_CAP = 8704, COLLECT_CAP = 1024;
    __shared__ uint32_t sample[SAMPLE_CAP];
    __shared__ uint64_t coll[COLLECT_CAP];
    bool done = false;
    if (total > COLLECT_CAP) {
        const int stride = (total + 8191) / 8192;
        if (tid == 0) { s_ns = 0; s_nc = 0; }
        __syncthreads();
        for (int p = wave4; p < nprobe; p += SEL_WAVES) {
            const int len = s_len[p];
            const float* strip = pair_scores + ((size_t)q * nprobe + p) * max_len;
            // (r04c: four loads of a lane in flight; one at a time the strip came in as a chain of dependent round trips)
            for (int i0 = lane64 * stride + (p % stride); i0 < len; i0 += 4 * 64 * stride) {
                float sc[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + u * 64 * stride;
                    sc[u] = i < len ? strip[i] : __builtin_nanf("");
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (sc[u] != sc[u]) continue;
                    const int slot = atomicAdd(&s_ns, 1);
                    if (slot < SAMPLE_CAP) sample[slot] = f32_orderable(sc[u] + 0.0f);
                }
            }
        }
        __syncthreads();
        const int ns = min(s_ns, SAMPLE_CAP);
        // rank in the sample whose value is, with margin, below the kp-th best of the full set
        const float t = (float)kp / (float)stride;
        const int want = (int)(t + 4.0f * sqrtf(t) + 6.0f);
        auto sampled = each_key<SEL_THREADS>([&](int i) { return sample[i]; }, ns);
        const uint32_t thr = ns > want ? block_select_kth<SEL_THREADS, uint32_t, false>(sampled, want, hist) : 0u;
        for (int p = wave4; p < nprobe; p += SEL_WAVES) {
            const int len = s_len[p];
            const int64_t off = s_off[p];
            const float* strip = pair_scores + ((size_t)q * nprobe + p) * max_len;   // (16-byte aligned: max_len is a multiple of 4)
            for (int i0 = lane64 * 4; i0 < len; i0 += 4 * 256) {         // (four 16-byte loads of a lane in flight)
                f32x4 v4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + u * 256;
                    const f32x4 nan4 = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
                    v4[u] = i < len ? *reinterpret_cast<const f32x4*>(strip + i) : nan4;           // (strips are padded to 4 floats)
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + u * 256;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float sc = v4[u][e];
                        if (i + e < len && sc == sc && f32_orderable(sc + 0.0f) >= thr) {
                            const int slot = atomicAdd(&s_nc, 1);
                            if (slot < COLLECT_CAP) coll[slot] = make_key(sc, (uint32_t)(off + i + e));      // (position in the lists, for now)
                        }
                    }
                }
            }
        }
        __syncthreads();
        const int nc = s_nc;
        // positions -> row ids, all collected keys at once (r04c: looked up where a key was found, every hit of a wave was a dependent
        // round trip of its own)
        for (int i = tid; i < min(nc, COLLECT_CAP); i += SEL_THREADS) {
            const uint64_t kpos = coll[i];
            coll[i] = make_key(key_score(kpos), (uint32_t)order[key_row(kpos)]);
        }
        __syncthreads();
        if (nc >= kp && nc <= COLLECT_CAP) {
            for (int i = tid; i < nc; i += SEL_THREADS) {
                const uint64_t ki = coll[i];
                int rank = 0;
                for (int j = 0; j < nc; ++j) rank += coll[j] > ki ? 1 : 0;
                if (rank < kp) top[rank] = ki;
            }
            done = true;
        }
        __syncthreads();
    }

    int m = kp;                                       // (fast path: top[0 .. kp) is filled)
    if (!done) {
        // general path: eight passes over the strips, (probe, position) by (probe, position); NaN rows never rank
        auto visit = [&](auto f) {
            for (int p = 0; p < nprobe; ++p) {
                const int64_t off = s_off[p];
                const int len = s_len[p];
                for (int i = tid; i < len; i += SEL_THREADS) {
                    const uint64_t key = key_at(p, i, off);
                    const float sc = key_score(key);
                    if (sc == sc) f(key);
                }
            }
        };
        const uint64_t T = total > kp ? block_select_kth<SEL_THREADS, uint64_t, false>(visit, kp, hist) : 0ull;
        m = min(block_collect_top(visit, T, top), kp);
    }
    // fp32 re-score of the kept rows (one wave per row), then rank by the exact cosines
    rescore_top(top, top, m, master, qn + (size_t)q * K, K, tid);
    __syncthreads();
    block_rank_write<SEL_THREADS>(top, m, k, cos_out + (size_t)q * k, id_out + (size_t)q * k,
                                  [&](uint32_t row) { return (int64_t)row + id_base; });
}

// Collect mode: the query's list holds every (estimated score, row) at or above its threshold -- a few hundred to a few thousand keys.
// The kp best by estimate (radix select in LDS) are re-scored in fp32 against the master and ranked, as ivf_select_kernel does for the strips.  A
// list that overflowed, or holds fewer than kp keys although more rows were probed, cannot answer: the query raises the fallback flag
// and the strip-mode pass (gated launches behind this kernel) answers the whole batch.
__global__ __launch_bounds__(SEL_THREADS) void ivf_select_list_kernel(const int* __restrict__ cnt, const int* __restrict__ totals,
                                                                      const uint64_t* __restrict__ list, int k, int kp, int64_t id_base,
                                                                      const float* __restrict__ master, const float* __restrict__ qn, int K,
                                                                      float* __restrict__ cos_out, int64_t* __restrict__ id_out, int* __restrict__ fallback) {
    __shared__ uint64_t keys[IVF_LIST_CAP];
    __shared__ uint64_t top[MAX_KP];
    __shared__ int hist[256];
    __shared__ int scratch[4];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int n = cnt[q], total = totals[q];                  // (total: rows in the query's probed lists, from ivf_threshold_kernel)
    if (n > IVF_LIST_CAP || n < min(kp, total)) {
        if (tid == 0) atomicExch(fallback, 1);
        return;
    }
    for (int i = tid; i < n; i += SEL_THREADS) keys[i] = list[(size_t)q * IVF_LIST_CAP + i];
    if (tid == 0) scratch[2] = 0;
    __syncthreads();
    const int m = min(n, kp);
    // This site keeps its own select loop and collect pass: through block_select_kth and block_collect_top the kernel measured
    // 1.6 % slower and the cause was not found (profiles/select_shared/NOTES.md).
    // The kp best keys by byte-wise radix select (r04c; rank counting before: n^2 / 1,024 LDS reads per thread -- timing builds without
    // it: 49 -> 8 us for one query, 154 -> 47 us at batch 1024, profiles/r04_configs/ivf_select_list_ablation.log).  Keys are unique
    // (score | ~row), so the pass after which the located bin holds exactly the keys still wanted ends the search: three or four
    // passes of the eight on scores that differ.
    uint64_t T = 0;
    if (n > kp) {
        uint64_t prefix = 0;
        int remaining = kp;
        for (int byte = 7; byte >= 0; --byte) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const int shift = byte * 8;
            for (int i = tid; i < n; i += SEL_THREADS) {
                const uint64_t key = keys[i];
                if (byte == 7 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(int)((key >> shift) & 0xff)], 1);
            }
            __syncthreads();
            {
                int hb, hr, unused;
                hist_locate<false>(hist, remaining, hb, hr, unused);
                if (tid == 0) { scratch[0] = hb < 0 ? 0 : hb; scratch[1] = hr; scratch[3] = hb < 0 ? 0 : hist[hb]; }
            }
            __syncthreads();
            prefix |= ((uint64_t)scratch[0] << shift);
            remaining = scratch[1];
            const bool whole_bin = scratch[3] == remaining;   // every key of the bin is wanted: keys >= prefix (lower bytes 0) are the kp best
            __syncthreads();
            if (whole_bin) break;
        }
        T = prefix;
    }
    for (int i = tid; i < n; i += SEL_THREADS) {
        const uint64_t key = keys[i];
        if (key >= T) {
            const int slot = atomicAdd(&scratch[2], 1);
            if (slot < MAX_KP) top[slot] = key;
        }
    }
    __syncthreads();
    rescore_top(top, keys, m, master, qn + (size_t)q * K, K, tid);          // (keys[] is free: the kp best are in top[])
    __syncthreads();
    block_rank_write<SEL_THREADS>(keys, m, k, cos_out + (size_t)q * k, id_out + (size_t)q * k,
                                  [&](uint32_t row) { return (int64_t)row + id_base; });
}

}  // namespace

int launch_ivf_probe_select(const float* scores, int b, int nlist, int nprobe, const float* rows, const float* cent, int dim, int64_t* probes,
                            float* probes_cos, hipStream_t s) {
    SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(ivf_probe_select_kernel), 64 * 1024));     // (nlist * 4 <= 64 KiB: the dense gate)
    hipLaunchKernelGGL(ivf_probe_select_kernel, dim3(b), dim3(PSEL_THREADS), (size_t)nlist * 4, s, scores, nlist, nprobe, rows, cent, dim,
                       probes, probes_cos);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_ivf_threshold(const int64_t* probes, const int64_t* offsets, const int* order, const float* pair_scores, int B, int nprobe, int max_len,
                         int kp, float* thr, int* cnt, uint64_t* list, hipStream_t s) {
    hipLaunchKernelGGL(ivf_threshold_kernel, dim3(B), dim3(THR_THREADS), 0, s, probes, offsets, order, pair_scores, nprobe, max_len, kp, thr,
                       cnt, list);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_ivf_select(const int64_t* probes, const int64_t* offsets, const int* order, const float* pair_scores, int B, int nprobe, int max_len,
                      const IvfSelectOut& o, const int* gate, hipStream_t s) {
    hipLaunchKernelGGL(ivf_select_kernel, dim3(B), dim3(SEL_THREADS), 0, s, probes, offsets, order, pair_scores, nprobe, max_len, o.k, o.kp,
                       o.id_base, o.master, o.qn, o.dim, o.cos_out, o.id_out, gate);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_ivf_select_list(const int* cnt, const uint64_t* list, int B, const IvfSelectOut& o, int* fallback, hipStream_t s) {
    hipLaunchKernelGGL(ivf_select_list_kernel, dim3(B), dim3(SEL_THREADS), 0, s, cnt, cnt + B, list, o.k, o.kp, o.id_base, o.master, o.qn,
                       o.dim, o.cos_out, o.id_out, fallback);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

}  // namespace sqe
