// encoder_kernels.h -- host-callable launchers of the encoder's kernel files (enc_gemm.hip, enc_gemm_pp.hip,
// enc_rows.hip, enc_attention.hip).  This is all encoder.hip sees of them: it holds no device code, and the kernel
// files know nothing of sqe_encoder.  Every launcher enqueues on `stream` and returns SQE_OK or the error it set.
#pragma once

#include "common.h"

namespace sqe {

#pragma GCC visibility push(hidden)   // calls between the encoder's own files: the library exports none of these

// ------------------------------------------------------------------ GEMM (enc_gemm.hip, enc_gemm_pp.hip)
enum { EPI_BIAS = 0, EPI_GELU = 1, EPI_RESID = 2, EPI_F32 = 3 };   // EPI_F32: plain fp32 products, no bias (IVF coarse scores)

struct GemmArgs {
    const bf16_t* W;      // [N, K] row-major (torch Linear weight)
    const bf16_t* X;      // [T_pad, K]
    const float* bias;    // [N]
    const bf16_t* resid;  // [T_pad, N] (EPI_RESID)
    void* out;            // bf16 [T_pad, N] or fp32 [T_pad, N] (EPI_RESID)
    int N, K, T;          // T = valid token rows
    int n_tiles;
    int splits;           // split-K factor (ring kernel, EPI_RESID only): split s writes its partial sum to
    size_t split_stride;  //   out + s * split_stride floats; bias and residual are added by split 0
    int t_tiles;
    int xcd_patches;      // gemm_ring_kernel: XCD-aware tile walk (0: linear)
    int pp_stagger;       // gemm_pp_kernel: half of a group's waves read their operands before they issue their DMA pieces
    int pp_dbg;           // gemm_pp_kernel, knobs build, timing only: 2 = no stores (results wrong), 4 = phase stamps (STAMPS build)
};

// Y = X W^T + b with epilogue `epi` (EPI_BIAS, EPI_GELU or EPI_RESID): the routing rule of enc_gemm.hip picks the kernel.
// *splits_out = number of fp32 partial sums written (EPI_RESID), `split_stride` floats apart; 0 = the output is
// ONE bf16 row per token (the persistent kernels).  *plan = which kernel this call launched (sqe_encoder_state).
int launch_gemm(int epi, const GemmArgs& a, int t_pad, int cu_count, hipStream_t stream, size_t split_stride = 0,
                int* splits_out = nullptr, sqe_encoder_gemm_t* plan = nullptr);

// the ping-pong kernel of enc_gemm_pp.hip, for the routing rule alone: N % 256 == 0, t_pad % 256 == 0, N <= MAX_BIAS_N
namespace gpp {
constexpr int MAX_BIAS_N = 4096;                      // the bias vector sits in LDS behind the ring
}
int launch_gemm_pp(int epi, const GemmArgs& a, int t_pad, int cu_count, hipStream_t stream, int* splits_out = nullptr);

// ------------------------------------------------------------------ row kernels (enc_rows.hip)
// E1: x = LN(word[id] + pos[s] + type[types[row]]); types == nullptr: type row 0 everywhere.  `scratch`: T x H floats.
int launch_embed_ln(const int32_t* ids, const int32_t* types, const bf16_t* word, const bf16_t* pos, const bf16_t* type, const float* g,
                    const float* b, float* scratch, bf16_t* out, int T, int S, int H, int vocab, int type_vocab, float eps, hipStream_t stream);
// LayerNorm of T rows of the pre-LayerNorm buffer (nsplit partial sums `stride` floats apart; 0: one bf16 row) -> bf16
int launch_layernorm(const float* in, const float* g, const float* b, bf16_t* out, int T, int H, float eps, int nsplit, size_t stride, hipStream_t stream);
// E7: the same of the CLS row of each of B sequences of S rows -> fp32 [B, H]
int launch_pool_ln(const float* in, const float* g, const float* b, float* out, int B, int S, int H, float eps, int nsplit, size_t stride, hipStream_t stream);
// classification head: pooled = tanh(b_p + W_p cls) [B, H], logits = b_c + W_c pooled [B, L]
int launch_pooler(const float* cls, const float* W, const float* bias, float* pooled, int B, int H, hipStream_t stream);
int launch_classifier(const float* pooled, const float* W, const float* bias, float* logits, int B, int H, int L, hipStream_t stream);

// ------------------------------------------------------------------ attention (enc_attention.hip)
// ctx = softmax(Q K^T / 8) V per (sequence, head) of qkv [B * S, 3 H]; *nw, *nq = the tiling picked (waves per workgroup, 16-row query blocks per wave)
int launch_attention(const bf16_t* qkv, const int32_t* lens, bf16_t* ctx, int B, int S, int H, int heads, int* nw, int* nq, hipStream_t stream);

#pragma GCC visibility pop

}  // namespace sqe
