// enc_attention.hip -- the encoder's attention (E3, head_dim = 64): flash-style per (sequence, head, block of query
// rows): S^T = K Q^T so the probabilities land in registers exactly as the B operand of the P V MFMA; V fragments by
// ds_read_b64_tr_b16; online softmax in fp32.  launch_attention picks the tiling from the sequence length.
#include <math.h>
#include <stdlib.h>

#include <type_traits>

#include "enc_device.h"

namespace sqe {

namespace {

// ------------------------------------------------------------------ attention (head_dim = 64)
// grid = B * heads * ceil(S / 64); 256 threads = 4 waves x 16 query rows.
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
// issue only: the caller waits once for a batch of these (lds_tr_wait8)
__device__ __forceinline__ u32x2 lds_tr_b64_issue(const char* addr) {
    u32x2 v;
    const uint32_t a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)addr;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=&v"(v) : "v"(a) : "memory");
    return v;
}
// the same read at a compile-time byte offset from a per-lane LDS address (the offset field of the DS instruction)
template <int OFF>
__device__ __forceinline__ u32x2 lds_tr_b64_issue_at(uint32_t lds_addr) {
    u32x2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=&v"(v) : "v"(lds_addr), "n"(OFF) : "memory");
    return v;
}
__device__ __forceinline__ void lds_tr_wait8(u32x2 (&x)[8]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])
                 :
                 : "memory");
}

// reductions over the four lane groups g of a query column c (lanes c, c + 16, c + 32, c + 48): two lane-swap
// instructions of gfx950 (v_permlane16_swap / v_permlane32_swap, VALU) instead of two trips through the LDS crossbar
__device__ __forceinline__ float xg_max(float v) {
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
    u32x2_t r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xg_sum(float v) {
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
    u32x2_t r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// NW waves x NQ blocks of 16 query rows per wave = NW * NQ * 16 query rows per workgroup: 64 for short sequences,
// 128 from 128 tokens on (8 waves x 1 block; from 256 tokens on 4 waves x 2 blocks).  A wave's NQ blocks share every K
// fragment and every transposed V fragment it reads from LDS, so LDS traffic per MFMA halves with NQ = 2.
//
// Per 64-key tile and query block: S^T[key][q] = K Q^T (8 MFMAs) leaves the scores of query c in lane (g, c);
// the softmax runs there in base 2 -- t = s * (log2 e / 8), p = exp2(t - m), one v_mul, one v_sub and one
// v_exp per score; keys are masked only in the last, partial tile -- and its probabilities are, as they stand
// in the accumulators, the B operand of O^T[d][q] += V^T P^T (8 MFMAs, A operand = the transposed V reads).
// With O transposed a lane holds output columns of ITS OWN query: the rescale by alpha and the final 1 / l
// need no cross-lane traffic, and a lane stores 4 consecutive output features at a time.
template <int NW, int NQ, int MINW = 1>
__global__ __launch_bounds__(NW * 64, MINW) void attention_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ lens,
                                                           bf16_t* __restrict__ ctx, int S, int H, int heads) {
    constexpr int QB = NW * NQ * 16;
    constexpr float SCALE_LOG2E = 0.125f * 1.4426950408889634f;        // 1 / sqrt(64) folded into the base-2 exponent
    __shared__ __attribute__((aligned(16))) char sKV[2][2 * 64 * ROWB];    // [buffer][K tile | V tile]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qblocks = (S + QB - 1) / QB;
    const int qb = blockIdx.x % qblocks;
    const int head = (blockIdx.x / qblocks) % heads;
    const int seq = blockIdx.x / (qblocks * heads);
    const int len = min(lens[seq], S);
    if (qb * QB >= len) return;                      // only padded query rows here
    const int g = lane >> 4, c = lane & 15;
    const size_t ld = (size_t)3 * H * 2;             // bytes per token row of qkv
    const char* base = reinterpret_cast<const char*>(qkv) + (size_t)seq * S * ld + (size_t)head * 64 * 2;

    // Q fragments of this wave's NQ x 16 query rows (lane (g, c) holds Q[q = c][d = kk*32 + g*8 .. +8))
    const int q_base = qb * QB + wave * (NQ * 16);
    bf16x8 qf[NQ][2];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        const int q_row = q_base + n * 16 + c;
        const int qr = q_row < S ? q_row : S - 1;
        const char* qp = base + (size_t)qr * ld;
        qf[n][0] = *reinterpret_cast<const bf16x8*>(qp + (0 * 32 + g * 8) * 2);
        qf[n][1] = *reinterpret_cast<const bf16x8*>(qp + (1 * 32 + g * 8) * 2);
    }
    float m[NQ], l[NQ];                              // running max (scaled, base-2 domain) / sum of query c
    f32x4 o[NQ][4];                                  // O^T: row d = dj*16 + g*4 + r, column = query c
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        m[n] = -INFINITY;
        l[n] = 0.f;
#pragma unroll
        for (int dj = 0; dj < 4; ++dj) o[n][dj] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // K/V tiles are double buffered: tile t + 1 is fetched while tile t is used (one barrier per tile)
    auto issue_kv = [&](int kv0, int buf) {
        // (the builtin form: hipcc knows these are loads; through inline asm it has to assume a store that still
        // reads its address registers and waits on vmcnt before it reuses them -- in the middle of the MFMAs)
        stage_rows<64, NW>(base + (size_t)kv0 * ld + (size_t)H * 2, ld, sKV[buf], wave, lane);                   // K part
        stage_rows<64, NW>(base + (size_t)kv0 * ld + (size_t)2 * H * 2, ld, sKV[buf] + 64 * ROWB, wave, lane);   // V part
    };
    // Per-lane LDS addresses, computed ONCE: every read of the loop is one of these plus a compile-time offset
    // (buffer, key block), so no address arithmetic is left in the loop.  The XOR swizzle of a tile row depends
    // on (row >> 1) & 7 only, which a step of 16 rows (K fragments) or 16 / 32 keys (V blocks) does not change.
    const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)&sKV[0][0];
    const int ksw = (c >> 1) & 7;
    const uint32_t kaddr0 = lds0 + c * ROWB + ((g ^ ksw) << 4);              // K fragment, d = g*8 .. (first 32 of 64)
    const uint32_t kaddr1 = lds0 + c * ROWB + (((4 + g) ^ ksw) << 4);        // d = 32 + g*8 ..
    uint32_t vaddr[4];                                                       // V^T fragment of feature block dj, key 4g + qq
    {
        const int qq = c >> 2, pp = c & 3, key0 = 4 * g + qq, vsw = (key0 >> 1) & 7;
#pragma unroll
        for (int dj = 0; dj < 4; ++dj)
            vaddr[dj] = lds0 + 64 * ROWB + key0 * ROWB + (((dj * 2 + (pp >> 1)) ^ vsw) << 4) + 8 * (pp & 1);
    }
    constexpr int BUFB = 2 * 64 * ROWB;              // bytes per K|V buffer

    // one 64-key tile out of buffer BUF (a compile-time constant: it selects the immediate offsets)
    auto tile = [&](int kv0, auto buf_tag) {
        constexpr int BUF = decltype(buf_tag)::value;
        // S^T[key][q] = sum_d K[key][d] Q[q][d]: every K fragment feeds all NQ query blocks
        f32x4 st[NQ][4];
#pragma unroll
        for (int kf = 0; kf < 4; ++kf) {
            const bf16x8 k0 = *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>((uintptr_t)(kaddr0 + BUF * BUFB + kf * 16 * ROWB));
            const bf16x8 k1 = *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>((uintptr_t)(kaddr1 + BUF * BUFB + kf * 16 * ROWB));
#pragma unroll
            for (int n = 0; n < NQ; ++n) {
                st[n][kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[n][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                st[n][kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[n][1], st[n][kf], 0, 0, 0);
            }
        }
        const bool partial = kv0 + 64 > len;         // wave-uniform: only the last tile of a sequence masks keys
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
            // scaled scores of query c (keys kf*16 + g*4 + r); the products are canonical numbers, so the maxima
            // need no NaN quieting and pair up into v_max3
            f32x4 t[4];
#pragma unroll
            for (int kf = 0; kf < 4; ++kf) t[kf] = st[n][kf] * SCALE_LOG2E;
            if (partial) {
                int lenx = len;
                asm volatile("; tail tile: mask keys >= len" : "+s"(lenx));   // opaque: nothing of this block is hoisted
#pragma unroll
                for (int kf = 0; kf < 4; ++kf)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kv0 + kf * 16 + g * 4 + r >= lenx) t[kf][r] = -INFINITY;
            }
            float mx = fmaxf(fmaxf(t[0][0], t[0][1]), t[0][2]);
            mx = fmaxf(fmaxf(mx, t[0][3]), t[1][0]);
            mx = fmaxf(fmaxf(mx, t[1][1]), t[1][2]);
            mx = fmaxf(fmaxf(mx, t[1][3]), t[2][0]);
            mx = fmaxf(fmaxf(mx, t[2][1]), t[2][2]);
            mx = fmaxf(fmaxf(mx, t[2][3]), t[3][0]);
            mx = fmaxf(fmaxf(mx, t[3][1]), t[3][2]);
            mx = xg_max(fmaxf(mx, t[3][3]));
            const float m_new = fmaxf(m[n], mx);     // finite: key kv0 < len is never masked
            const float alpha = __builtin_amdgcn_exp2f(m[n] - m_new);
            // p = exp2(s * c - m): one packed fma on the raw scores (masked ones come from t: they are -inf there)
            const f32x4 cv = {SCALE_LOG2E, SCALE_LOG2E, SCALE_LOG2E, SCALE_LOG2E};
            const f32x4 nm = {-m_new, -m_new, -m_new, -m_new};
            if (partial) {
                asm volatile("; tail tile: exponents from the masked scores" ::);
#pragma unroll
                for (int kf = 0; kf < 4; ++kf) t[kf] = t[kf] + nm;
            } else {
#pragma unroll
                for (int kf = 0; kf < 4; ++kf) t[kf] = __builtin_elementwise_fma(st[n][kf], cv, nm);
            }
#pragma unroll
            for (int kf = 0; kf < 4; ++kf) {
#pragma unroll
                for (int r = 0; r < 4; ++r) t[kf][r] = __builtin_amdgcn_exp2f(t[kf][r]);
                st[n][kf] = t[kf];
            }
            const f32x4 sv = (t[0] + t[1]) + (t[2] + t[3]);
            const float psum = xg_sum((sv[0] + sv[1]) + (sv[2] + sv[3]));
            l[n] = l[n] * alpha + psum;
            m[n] = m_new;
            // O^T columns are this lane's own query: rescale in place
#pragma unroll
            for (int dj = 0; dj < 4; ++dj) o[n][dj] *= alpha;
        }
        // O^T += V^T P^T : A operand = V by transposed LDS reads (k slot j of lane group g = key
        // 16*(2*kk2 + (j>>2)) + 4*g + (j&3), feature dj*16 + c), B operand = P straight from the S^T accumulators
        auto pv_half = [&](auto kk2_tag) {
            constexpr int KK2 = decltype(kk2_tag)::value;
            constexpr int LO = BUF * BUFB + 32 * KK2 * ROWB, HI = LO + 16 * ROWB;
            // the eight transposed reads of this half go out together and are waited for once
            u32x2 vt[8];
            vt[0] = lds_tr_b64_issue_at<LO>(vaddr[0]); vt[1] = lds_tr_b64_issue_at<HI>(vaddr[0]);
            vt[2] = lds_tr_b64_issue_at<LO>(vaddr[1]); vt[3] = lds_tr_b64_issue_at<HI>(vaddr[1]);
            vt[4] = lds_tr_b64_issue_at<LO>(vaddr[2]); vt[5] = lds_tr_b64_issue_at<HI>(vaddr[2]);
            vt[6] = lds_tr_b64_issue_at<LO>(vaddr[3]); vt[7] = lds_tr_b64_issue_at<HI>(vaddr[3]);
            bf16x8 pb[NQ];
#pragma unroll
            for (int n = 0; n < NQ; ++n) {
                typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
                const u32x4 pk = {pack_bf16x2(st[n][2 * KK2][0], st[n][2 * KK2][1]), pack_bf16x2(st[n][2 * KK2][2], st[n][2 * KK2][3]),
                                  pack_bf16x2(st[n][2 * KK2 + 1][0], st[n][2 * KK2 + 1][1]),
                                  pack_bf16x2(st[n][2 * KK2 + 1][2], st[n][2 * KK2 + 1][3])};
                pb[n] = __builtin_bit_cast(bf16x8, pk);
            }
            lds_tr_wait8(vt);
#pragma unroll
            for (int dj = 0; dj < 4; ++dj) {
                typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
                const u32x4 packed = {vt[2 * dj].x, vt[2 * dj].y, vt[2 * dj + 1].x, vt[2 * dj + 1].y};
                const bf16x8 va = __builtin_bit_cast(bf16x8, packed);
#pragma unroll
                for (int n = 0; n < NQ; ++n) o[n][dj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb[n], o[n][dj], 0, 0, 0);
            }
        };
        pv_half(std::integral_constant<int, 0>{});
        pv_half(std::integral_constant<int, 1>{});
    };
    auto tile_sync = [&]() {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");    // my pieces of this tile landed, my LDS reads are done
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();                                  // everyone's landed; everyone left the other buffer
        __builtin_amdgcn_sched_barrier(0);
    };
    issue_kv(0, 0);
    for (int kv0 = 0; kv0 < len; kv0 += 128) {       // two tiles per trip: the buffer index is a compile-time constant
        tile_sync();
        if (kv0 + 64 < len) issue_kv(kv0 + 64, 1);
        tile(kv0, std::integral_constant<int, 0>{});
        if (kv0 + 64 >= len) break;
        tile_sync();
        if (kv0 + 128 < len) issue_kv(kv0 + 128, 0);
        tile(kv0 + 64, std::integral_constant<int, 1>{});
    }
    // normalise and store: lane (g, c) holds O[q = c][d = dj*16 + g*4 + r], four consecutive features per dj
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        const int q = q_base + n * 16 + c;
        if (q < len) {
            const float inv = 1.0f / l[n];
            bf16_t* dst = ctx + ((size_t)seq * S + q) * H + head * 64 + g * 4;
#pragma unroll
            for (int dj = 0; dj < 4; ++dj) {
                uint2 w;
                w.x = pack_bf16x2(o[n][dj][0] * inv, o[n][dj][1] * inv);
                w.y = pack_bf16x2(o[n][dj][2] * inv, o[n][dj][3] * inv);
                *reinterpret_cast<uint2*>(dst + dj * 16) = w;
            }
        }
    }
}

// The tilings, first match wins: sequences of at least `min_s` tokens; `form` >= 0: only under SQE_ATT_FORM=form
// (knobs build, A/B of the forms the 256-token choice replaced).  A workgroup takes nw * nq * 16 query rows.
using AttentionKernel = void (*)(const bf16_t*, const int32_t*, bf16_t*, int, int, int);
struct AttentionForm { int min_s, form, nw, nq; AttentionKernel kern; };
const AttentionForm ATT_FORMS[] = {
    {256, 1, 8, 2, attention_kernel<8, 2, 4>},
    {256, 2, 8, 1, attention_kernel<8, 1>},
    {256, 3, 4, 1, attention_kernel<4, 1>},
    {256, -1, 4, 2, attention_kernel<4, 2, 3>},    // 4 waves x 2 blocks: 128 query rows per workgroup, three workgroups per CU
    {128, -1, 8, 1, attention_kernel<8, 1>},
    {0, -1, 4, 1, attention_kernel<4, 1>},
};

}  // namespace

int launch_attention(const bf16_t* qkv, const int32_t* lens, bf16_t* ctx, int B, int S, int H, int heads, int* nw, int* nq,
                     hipStream_t stream) {
    static const int att_form = [] { const char* e = knob_env("SQE_ATT_FORM"); return e ? atoi(e) : 0; }();   // knobs build: A/B
    const AttentionForm* f = ATT_FORMS;
    while (S < f->min_s || (f->form >= 0 && f->form != att_form)) ++f;       // the last row matches everything
    const int rows = f->nw * f->nq * 16;
    *nw = f->nw; *nq = f->nq;
    hipLaunchKernelGGL(f->kern, dim3(B * heads * ((S + rows - 1) / rows)), dim3(f->nw * 64), 0, stream, qkv, lens, ctx, S, H, heads);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

}  // namespace sqe
