// enc_device.h -- device-side helpers that more than one of the encoder's kernel files uses (enc_gemm.hip,
// enc_gemm_pp.hip, enc_rows.hip, enc_attention.hip): the tile image of a 64-wide bf16 K step and its staging, the
// GELU forms, and the epilogue the one-tile, ring and few-token GEMM kernels share.
#pragma once

#include "internal.h"
#include "encoder_kernels.h"

namespace sqe {

constexpr int ROWB = 128;   // bytes per tile row per 64-wide bf16 K step

// ------------------------------------------------------------------ staging helpers
template <int ROWS, int NW>
__device__ __forceinline__ void stage_rows(const char* gbase, size_t ld_bytes, char* lds, int wave, int lane) {
    constexpr int NINSTR = ROWS / 8;          // one 1-KiB wave-instruction per 8 rows
    constexpr int ITERS = (NINSTR + NW - 1) / NW;
    const int r_local = lane >> 3;
    const int cprime = lane & 7;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int g = it * NW + wave;
        if (NINSTR % NW == 0 || g < NINSTR) {
            const int r = g * 8 + r_local;
            const int c = cprime ^ ((r >> 1) & 7);
            const char* src = gbase + (size_t)r * ld_bytes + c * 16;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(lds + g * 1024), 16, 0, 0);
        }
    }
}
// same tile image, pieces issued through inline asm (invisible to hipcc's waitcnt insertion: the caller
// counts its own waits and may keep a tile in flight across LDS reads)
template <int ROWS, int NW>
__device__ __forceinline__ void stage_rows_asm(const char* gbase, size_t ld_bytes, char* lds, int wave, int lane) {
    constexpr int NINSTR = ROWS / 8;
    static_assert(NINSTR % NW == 0, "every wave issues the same number of pieces");
    const int r_local = lane >> 3;
    const int cprime = lane & 7;
#pragma unroll
    for (int it = 0; it < NINSTR / NW; ++it) {
        const int g = it * NW + wave;
        const int r = g * 8 + r_local;
        const int c = cprime ^ ((r >> 1) & 7);
        lds_dma16(gbase + (size_t)r * ld_bytes + c * 16, lds + g * 1024);
    }
}
__device__ __forceinline__ bf16x8 frag(const char* tile, int r, int c) {
    return *reinterpret_cast<const bf16x8*>(tile + r * ROWB + ((c ^ ((r >> 1) & 7)) << 4));
}
__device__ __forceinline__ float bf16_to_f32(bf16_t v) { return __uint_as_float((uint32_t)v << 16); }

// ------------------------------------------------------------------ GELU
// erf-GELU, 0.5 v (1 + erf(v / sqrt 2)), with erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, far below
// the bf16 rounding of the result): one v_rcp, one v_exp and a 5-term Horner chain instead of libm's
// branchy erff -- the GELU epilogue of the FFN-up GEMM was as long as its K loop.
__device__ __forceinline__ float gelu_erf(float v) {
    const float x = fabsf(v) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, x, 1.0f));
    float poly = fmaf(1.061405429f, t, -1.453152027f);
    poly = fmaf(poly, t, 1.421413741f);
    poly = fmaf(poly, t, -0.284496736f);
    poly = fmaf(poly, t, 0.254829592f);
    const float e = 1.0f - poly * t * __expf(-x * x);          // erf(|v| / sqrt 2)
    return 0.5f * v * (1.0f + copysignf(e, v));
}

// The same on two values at once: every multiply / fma of the chain is one packed fp32 instruction
// (v_pk_mul_f32 / v_pk_fma_f32), which halves the instruction count of the GELU epilogue -- the epilogue of the
// FFN-up GEMM is VALU-issue-bound (no MFMA runs beside it).
typedef __attribute__((ext_vector_type(2))) float f32x2;
__device__ __forceinline__ f32x2 gelu_erf2(f32x2 v) {
    const f32x2 x = {fabsf(v[0]) * 0.70710678118654752f, fabsf(v[1]) * 0.70710678118654752f};
    const f32x2 den = __builtin_elementwise_fma(f32x2{0.3275911f, 0.3275911f}, x, f32x2{1.0f, 1.0f});
    const f32x2 t = {__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])};
    f32x2 poly = __builtin_elementwise_fma(f32x2{1.061405429f, 1.061405429f}, t, f32x2{-1.453152027f, -1.453152027f});
    poly = __builtin_elementwise_fma(poly, t, f32x2{1.421413741f, 1.421413741f});
    poly = __builtin_elementwise_fma(poly, t, f32x2{-0.284496736f, -0.284496736f});
    poly = __builtin_elementwise_fma(poly, t, f32x2{0.254829592f, 0.254829592f});
    const f32x2 nx2 = x * x * -1.4426950408889634f;                  // exp(-x^2) = exp2(-x^2 log2 e)
    const f32x2 ex = {__builtin_amdgcn_exp2f(nx2[0]), __builtin_amdgcn_exp2f(nx2[1])};
    const f32x2 e = __builtin_elementwise_fma(poly * t, -ex, f32x2{1.0f, 1.0f});      // erf(|v| / sqrt 2)
    const f32x2 es = {copysignf(e[0], v[0]), copysignf(e[1], v[1])};
    return __builtin_elementwise_fma(es, v * 0.5f, v * 0.5f);          // 0.5 v (1 + erf)
}

// GELU for the large-batch GEMM epilogue, where it is the cost (128 values per lane, VALU-issue-bound: the erf form
// above is ~36 issue slots per pair of values, four of them transcendental): 0.5 x (1 + erf(x / sqrt 2)) =
// x (0.5 + h(x)), h odd; h(x) ~ x Q(x^2) with a degree-13 odd polynomial fitted on |x| <= 4 (weighted so that
// |x| |h error| is minimised), x clamped to [-4, 4] inside h, and the fit pinned so that this fp32 evaluation gives
// h(4) = 0.5 EXACTLY: beyond the clamp GELU is x or 0 exactly, however large |x| is.  12 issue slots per pair, no
// transcendental.  |GELU_poly - GELU_erf| <= 1.9e-4 absolute for every x (tools/gelu_fit.py makes the fit and prints
// the error of the fp32 evaluation); the output is rounded to bf16 (2^-9 relative) right after.
__device__ __forceinline__ f32x2 gelu_poly2(f32x2 v) {
    const f32x2 xc = {__builtin_amdgcn_fmed3f(v[0], -4.0f, 4.0f), __builtin_amdgcn_fmed3f(v[1], -4.0f, 4.0f)};
    const f32x2 t = xc * xc;
    f32x2 q = __builtin_elementwise_fma(f32x2{2.258820153144825e-08f, 2.258820153144825e-08f}, t, f32x2{-1.5888268762864755e-06f, -1.5888268762864755e-06f});
    q = __builtin_elementwise_fma(q, t, f32x2{4.776388232130557e-05f, 4.776388232130557e-05f});
    q = __builtin_elementwise_fma(q, t, f32x2{-0.000812187441624701f, -0.000812187441624701f});
    q = __builtin_elementwise_fma(q, t, f32x2{0.00876369047909975f, 0.00876369047909975f});
    q = __builtin_elementwise_fma(q, t, f32x2{-0.06455441564321518f, -0.06455441564321518f});
    q = __builtin_elementwise_fma(q, t, f32x2{0.39787042140960693f, 0.39787042140960693f});
    const f32x2 h = q * xc;
    return __builtin_elementwise_fma(v, h, v * 0.5f);
}

// ------------------------------------------------------------------ GEMM epilogue (one-tile, ring, few-token)
// A lane's four consecutive features n .. n + 3 of token t: acc + bias, then by EPI: + bf16 residual (split 0 only)
// and the fp32 partial sum of K slice `split` | plain fp32 | optional erf-GELU and bf16.  The caller keeps its loop,
// its `t < p.T` test and its rule for loading b4 (zeros where no bias is added).  gemm_persistent_kernel and
// gemm_pp_kernel are NOT callers: their epilogues are shaped by their schedules (stores under the next tile's DMA,
// packed GELU forms, bias in LDS) and stay with them.  (p by value, as the kernels take it: through a reference hipcc
// ordered the address arithmetic at the head of the few-token kernel differently.)
template <int EPI>
__device__ __forceinline__ void gemm_epilogue(f32x4 acc, float4 b4, int t, int n, int split, const GemmArgs p) {
    float v0 = acc[0] + b4.x, v1 = acc[1] + b4.y, v2 = acc[2] + b4.z, v3 = acc[3] + b4.w;
    const size_t o = (size_t)t * p.N + n;
    if (EPI == EPI_RESID) {
        if (split == 0) {
            const uint2 r2 = *reinterpret_cast<const uint2*>(p.resid + o);
            v0 += bf16_to_f32((bf16_t)(r2.x & 0xffff)); v1 += bf16_to_f32((bf16_t)(r2.x >> 16));
            v2 += bf16_to_f32((bf16_t)(r2.y & 0xffff)); v3 += bf16_to_f32((bf16_t)(r2.y >> 16));
        }
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.out) + (size_t)split * p.split_stride + o) =
            make_float4(v0, v1, v2, v3);
    } else if (EPI == EPI_F32) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.out) + o) = make_float4(v0, v1, v2, v3);
    } else {
        if (EPI == EPI_GELU) { v0 = gelu_erf(v0); v1 = gelu_erf(v1); v2 = gelu_erf(v2); v3 = gelu_erf(v3); }
        uint2 w2;
        w2.x = pack_bf16x2(v0, v1);
        w2.y = pack_bf16x2(v2, v3);
        *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(p.out) + o) = w2;
    }
}

}  // namespace sqe
