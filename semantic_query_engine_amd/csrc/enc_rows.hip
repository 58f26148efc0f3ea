// enc_rows.hip -- the encoder's row kernels, one wave per row (HBM stream): embedding + LayerNorm (E1), LayerNorm of
// the pre-LayerNorm sums, pooling LayerNorm of the CLS rows (E7), and the fp32 classification head (pooler, classifier).
#include <math.h>

#include "enc_device.h"

namespace sqe {

namespace {

// ------------------------------------------------------------------ LayerNorm family
// one wave per row; H % 4 == 0; two passes over registers-or-cache (row <= 16 KiB)
// row element i = sum over the nsplit split-K partial sums (stride floats apart); nsplit = 1: plain fp32 row;
// nsplit = 0: the row is bf16 (`row` then points at bf16 data: ln_row() does the addressing)
__device__ __forceinline__ float4 ln_load(const float* row, int i, int nsplit, size_t stride) {
    if (nsplit == 0) {
        const uint2 w = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16_t*>(row) + i);
        return make_float4(bf16_to_f32((bf16_t)(w.x & 0xffff)), bf16_to_f32((bf16_t)(w.x >> 16)),
                           bf16_to_f32((bf16_t)(w.y & 0xffff)), bf16_to_f32((bf16_t)(w.y >> 16)));
    }
    float4 v = *reinterpret_cast<const float4*>(row + i);
    if (nsplit == 1) return v;
    if (nsplit <= 4) {
        // (r04c) up to four partial sums, their loads issued together: a loop of `nsplit` trips is `nsplit` dependent round trips (the
        // LayerNorm of 16 tokens took 6.8 us, profiles/r04_configs/enc_1x16_forward_trace.txt).  A partial sum that does not exist is
        // read from partial sum 0 (a hit) and not added: no branch around the loads, the same additions in the same order.
        float4 w[3];
#pragma unroll
        for (int s = 1; s < 4; ++s) w[s - 1] = *reinterpret_cast<const float4*>(row + (size_t)(s < nsplit ? s : 0) * stride + i);
#pragma unroll
        for (int s = 1; s < 4; ++s)
            if (s < nsplit) { v.x += w[s - 1].x; v.y += w[s - 1].y; v.z += w[s - 1].z; v.w += w[s - 1].w; }
        return v;
    }
    for (int s = 1; s < nsplit; ++s) {
        const float4 w = *reinterpret_cast<const float4*>(row + (size_t)s * stride + i);
        v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
    return v;
}
// first element of row `r` of the pre-LayerNorm buffer in either form
__device__ __forceinline__ const float* ln_row(const float* in, size_t r, int H, int nsplit) {
    return nsplit == 0 ? reinterpret_cast<const float*>(reinterpret_cast<const bf16_t*>(in) + r * H) : in + r * H;
}

__device__ __forceinline__ void ln_stats(const float* row, int H, int lane, float& mean, float& rstd, float eps,
                                         int nsplit = 1, size_t stride = 0) {
    float s = 0.f;
    for (int i = lane * 4; i < H; i += 256) {
        const float4 v = ln_load(row, i, nsplit, stride);
        s += v.x + v.y + v.z + v.w;
    }
    mean = wave_sum(s) / (float)H;
    float q = 0.f;
    for (int i = lane * 4; i < H; i += 256) {
        const float4 v = ln_load(row, i, nsplit, stride);
        const float a = v.x - mean, b = v.y - mean, c = v.z - mean, d = v.w - mean;
        q += a * a + b * b + c * c + d * d;
    }
    rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + eps);
}

// Rows of at most 1024 elements (H % 256 == 0) are read ONCE into registers -- one memory round trip instead of
// three; sums run in the order ln_stats uses, so both forms give the same bits.
__device__ __forceinline__ bool ln_row_regs(const float* row, int H, int lane, float eps, int nsplit, size_t stride,
                                            float4 (&v)[4], float& mean, float& rstd) {
    const int nit = H >> 8;
    if ((H & 255) != 0 || nit > 4) return false;
#pragma unroll
    for (int it = 0; it < 4; ++it)
        if (it < nit) v[it] = ln_load(row, lane * 4 + it * 256, nsplit, stride);
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < 4; ++it)
        if (it < nit) s += v[it].x + v[it].y + v[it].z + v[it].w;
    mean = wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int it = 0; it < 4; ++it)
        if (it < nit) {
            const float a = v[it].x - mean, b = v[it].y - mean, c = v[it].z - mean, d = v[it].w - mean;
            q += a * a + b * b + c * c + d * d;
        }
    rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + eps);
    return true;
}

__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ in, const float* __restrict__ g,
                                                        const float* __restrict__ b, bf16_t* __restrict__ out,
                                                        int T, int H, float eps, int nsplit, size_t stride) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T) return;
    const float* x = ln_row(in, (size_t)row, H, nsplit);
    float mean, rstd;
    float4 vr[4];
    if (ln_row_regs(x, H, lane, eps, nsplit, stride, vr, mean, rstd)) {
#pragma unroll
        for (int it = 0; it < 4; ++it)
            if (it < (H >> 8)) {
                const int i = lane * 4 + it * 256;
                const float4 v = vr[it];
                const float4 gg = *reinterpret_cast<const float4*>(g + i);
                const float4 bb = *reinterpret_cast<const float4*>(b + i);
                uint2 w;
                w.x = pack_bf16x2((v.x - mean) * rstd * gg.x + bb.x, (v.y - mean) * rstd * gg.y + bb.y);
                w.y = pack_bf16x2((v.z - mean) * rstd * gg.z + bb.z, (v.w - mean) * rstd * gg.w + bb.w);
                *reinterpret_cast<uint2*>(out + (size_t)row * H + i) = w;
            }
        return;
    }
    ln_stats(x, H, lane, mean, rstd, eps, nsplit, stride);
    for (int i = lane * 4; i < H; i += 256) {
        const float4 v = ln_load(x, i, nsplit, stride);
        const float4 gg = *reinterpret_cast<const float4*>(g + i);
        const float4 bb = *reinterpret_cast<const float4*>(b + i);
        uint2 w;
        w.x = pack_bf16x2((v.x - mean) * rstd * gg.x + bb.x, (v.y - mean) * rstd * gg.y + bb.y);
        w.y = pack_bf16x2((v.z - mean) * rstd * gg.z + bb.z, (v.w - mean) * rstd * gg.w + bb.w);
        *reinterpret_cast<uint2*>(out + (size_t)row * H + i) = w;
    }
}

// E7: LayerNorm of the CLS row of every sequence, fp32 out [B, H]
__global__ __launch_bounds__(256) void pool_ln_kernel(const float* __restrict__ in, const float* __restrict__ g,
                                                      const float* __restrict__ b, float* __restrict__ out,
                                                      int B, int S, int H, float eps, int nsplit, size_t stride) {
    const int lane = threadIdx.x & 63;
    const int seq = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seq >= B) return;
    const float* x = ln_row(in, (size_t)seq * S, H, nsplit);
    float mean, rstd;
    float4 vr[4];
    if (ln_row_regs(x, H, lane, eps, nsplit, stride, vr, mean, rstd)) {
#pragma unroll
        for (int it = 0; it < 4; ++it)
            if (it < (H >> 8)) {
                const int i = lane * 4 + it * 256;
                const float4 v = vr[it];
                const float4 gg = *reinterpret_cast<const float4*>(g + i);
                const float4 bb = *reinterpret_cast<const float4*>(b + i);
                *reinterpret_cast<float4*>(out + (size_t)seq * H + i) =
                    make_float4((v.x - mean) * rstd * gg.x + bb.x, (v.y - mean) * rstd * gg.y + bb.y,
                                (v.z - mean) * rstd * gg.z + bb.z, (v.w - mean) * rstd * gg.w + bb.w);
            }
        return;
    }
    ln_stats(x, H, lane, mean, rstd, eps, nsplit, stride);
    for (int i = lane * 4; i < H; i += 256) {
        const float4 v = ln_load(x, i, nsplit, stride);
        const float4 gg = *reinterpret_cast<const float4*>(g + i);
        const float4 bb = *reinterpret_cast<const float4*>(b + i);
        *reinterpret_cast<float4*>(out + (size_t)seq * H + i) =
            make_float4((v.x - mean) * rstd * gg.x + bb.x, (v.y - mean) * rstd * gg.y + bb.y,
                        (v.z - mean) * rstd * gg.z + bb.z, (v.w - mean) * rstd * gg.w + bb.w);
    }
}

// E1: x = LN(word[id] + pos[s] + type[0]); the fp32 sum goes through `scratch` (one row per wave slot).
// SEGMENTS (pair scoring): type[types[row]] instead, clamped into [0, type_vocab); types == nullptr: row 0 everywhere.
template <bool SEGMENTS>
__global__ __launch_bounds__(256) void embed_ln_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ types,
                                                       const bf16_t* __restrict__ word,
                                                       const bf16_t* __restrict__ pos, const bf16_t* __restrict__ type,
                                                       const float* __restrict__ g, const float* __restrict__ b,
                                                       float* __restrict__ scratch, bf16_t* __restrict__ out,
                                                       int T, int S, int H, int vocab, int type_vocab, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T) return;
    int id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const int s = row % S;
    if (SEGMENTS && types) {
        int ty = types[row];
        ty = ty < 0 ? 0 : (ty >= type_vocab ? type_vocab - 1 : ty);
        type += (size_t)ty * H;
    }
    float* tmp = scratch + (size_t)row * H;
    for (int i = lane * 4; i < H; i += 256) {
        const uint2 w = *reinterpret_cast<const uint2*>(word + (size_t)id * H + i);
        const uint2 p = *reinterpret_cast<const uint2*>(pos + (size_t)s * H + i);
        const uint2 t = *reinterpret_cast<const uint2*>(type + i);
        float4 v;
        v.x = bf16_to_f32((bf16_t)(w.x & 0xffff)) + bf16_to_f32((bf16_t)(p.x & 0xffff)) + bf16_to_f32((bf16_t)(t.x & 0xffff));
        v.y = bf16_to_f32((bf16_t)(w.x >> 16)) + bf16_to_f32((bf16_t)(p.x >> 16)) + bf16_to_f32((bf16_t)(t.x >> 16));
        v.z = bf16_to_f32((bf16_t)(w.y & 0xffff)) + bf16_to_f32((bf16_t)(p.y & 0xffff)) + bf16_to_f32((bf16_t)(t.y & 0xffff));
        v.w = bf16_to_f32((bf16_t)(w.y >> 16)) + bf16_to_f32((bf16_t)(p.y >> 16)) + bf16_to_f32((bf16_t)(t.y >> 16));
        *reinterpret_cast<float4*>(tmp + i) = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    float mean, rstd;
    ln_stats(tmp, H, lane, mean, rstd, eps);
    for (int i = lane * 4; i < H; i += 256) {
        const float4 v = *reinterpret_cast<const float4*>(tmp + i);
        const float4 gg = *reinterpret_cast<const float4*>(g + i);
        const float4 bb = *reinterpret_cast<const float4*>(b + i);
        uint2 w;
        w.x = pack_bf16x2((v.x - mean) * rstd * gg.x + bb.x, (v.y - mean) * rstd * gg.y + bb.y);
        w.y = pack_bf16x2((v.z - mean) * rstd * gg.z + bb.z, (v.w - mean) * rstd * gg.w + bb.w);
        *reinterpret_cast<uint2*>(out + (size_t)row * H + i) = w;
    }
}

// ------------------------------------------------------------------ classification head (fp32)
// pooled[b][j] = tanh(b_p[j] + W_p[j] . cls[b]): one wave per output feature j, four to a workgroup.  REGS (H <= 1024): the
// wave keeps its row of W_p in registers (a float4 per lane and 256-column pass; H % 128 == 0, so the last pass may use
// lanes 0 .. 31 only) and walks the B CLS rows, which sit in L2: W_p comes from HBM once per call.  Wider models stream the
// row from cache per sequence.
template <bool REGS>
__global__ __launch_bounds__(256) void pooler_kernel(const float* __restrict__ cls, const float* __restrict__ W,
                                                     const float* __restrict__ bias, float* __restrict__ pooled, int B, int H) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= H) return;
    const float* wr = W + (size_t)j * H;
    float4 w[4];
    if (REGS) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int i = lane * 4 + it * 256;
            w[it] = i < H ? *reinterpret_cast<const float4*>(wr + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const float bj = bias[j];
    for (int b = 0; b < B; ++b) {
        const float* x = cls + (size_t)b * H;
        float s = 0.f;
        if (REGS) {
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int i = lane * 4 + it * 256;
                if (i < H) {
                    const float4 v = *reinterpret_cast<const float4*>(x + i);
                    s += w[it].x * v.x + w[it].y * v.y + w[it].z * v.z + w[it].w * v.w;
                }
            }
        } else {
            for (int i = lane * 4; i < H; i += 256) {
                const float4 u = *reinterpret_cast<const float4*>(wr + i);
                const float4 v = *reinterpret_cast<const float4*>(x + i);
                s += u.x * v.x + u.y * v.y + u.z * v.z + u.w * v.w;
            }
        }
        s = wave_sum(s);
        if (lane == 0) pooled[(size_t)b * H + j] = tanhf(bj + s);
    }
}

// logit[b][l] = b_c[l] + W_c[l] . pooled[b]: one wave per (b, l)
__global__ __launch_bounds__(256) void classifier_kernel(const float* __restrict__ pooled, const float* __restrict__ W,
                                                         const float* __restrict__ bias, float* __restrict__ logits,
                                                         int B, int H, int L) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= B * L) return;
    const int l = o % L;
    const float* x = pooled + (size_t)(o / L) * H;
    const float* wr = W + (size_t)l * H;
    float s = 0.f;
    for (int i = lane * 4; i < H; i += 256) {
        const float4 u = *reinterpret_cast<const float4*>(wr + i);
        const float4 v = *reinterpret_cast<const float4*>(x + i);
        s += u.x * v.x + u.y * v.y + u.z * v.z + u.w * v.w;
    }
    s = wave_sum(s);
    if (lane == 0) logits[o] = bias[l] + s;
}

}  // namespace

// ------------------------------------------------------------------ launchers: four rows (waves) to a workgroup
int launch_embed_ln(const int32_t* ids, const int32_t* types, const bf16_t* word, const bf16_t* pos, const bf16_t* type,
                    const float* g, const float* b, float* scratch, bf16_t* out, int T, int S, int H, int vocab,
                    int type_vocab, float eps, hipStream_t stream) {
    const auto kern = types ? embed_ln_kernel<true> : embed_ln_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((T + 3) / 4), dim3(256), 0, stream, ids, types, word, pos, type, g, b, scratch, out, T, S, H,
                       vocab, type_vocab, eps);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_layernorm(const float* in, const float* g, const float* b, bf16_t* out, int T, int H, float eps, int nsplit,
                     size_t stride, hipStream_t stream) {
    hipLaunchKernelGGL(layernorm_kernel, dim3((T + 3) / 4), dim3(256), 0, stream, in, g, b, out, T, H, eps, nsplit, stride);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_pool_ln(const float* in, const float* g, const float* b, float* out, int B, int S, int H, float eps, int nsplit,
                   size_t stride, hipStream_t stream) {
    hipLaunchKernelGGL(pool_ln_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, in, g, b, out, B, S, H, eps, nsplit, stride);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_pooler(const float* cls, const float* W, const float* bias, float* pooled, int B, int H, hipStream_t stream) {
    const auto kern = H <= 1024 ? pooler_kernel<true> : pooler_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(H / 4), dim3(256), 0, stream, cls, W, bias, pooled, B, H);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_classifier(const float* pooled, const float* W, const float* bias, float* logits, int B, int H, int L,
                      hipStream_t stream) {
    hipLaunchKernelGGL(classifier_kernel, dim3((B * L + 3) / 4), dim3(256), 0, stream, pooled, W, bias, logits, B, H, L);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

}  // namespace sqe
