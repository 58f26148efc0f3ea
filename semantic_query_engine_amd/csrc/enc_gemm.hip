// enc_gemm.hip -- the encoder's GEMMs, Y = X W^T + b on v_mfma_f32_16x16x32_bf16 with both operands staged
// global -> LDS in full 128-B lines (XOR chunk swizzle on the source address and on the ds_read_b128 address), and
// the rule that routes a call to one of them:
//   gemm_skinny_kernel      at most 64 tokens: fragments straight from global memory, K split over the waves
//   gemm_ring_kernel        small batches: LDS ring with counted waits, tile picked from RING_MENU, optional split-K
//   gemm_pp_kernel          large batches, 256 x 256 tiles, ping-pong schedule (enc_gemm_pp.hip)
//   gemm_persistent_kernel  large batches, N > gpp::MAX_BIAS_N (and SQE_ENC_GEMM=0): two LDS stages
//   gemm_bf16_kernel        one tile per workgroup, double buffered (SQE_ENC_GEMM_V0=1 only)
// Epilogues: bias | bias + erf-GELU | bias + residual (fp32 out, feeds LayerNorm) | plain fp32 (IVF coarse scores).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "enc_device.h"

namespace sqe {

namespace {

// Block tile: (2*FM*16) output features x (4*FN*16) tokens, 8 waves as 2 (features) x 4 (tokens).
// MFMA A operand = W rows, B operand = X rows, so a lane holds 4 CONSECUTIVE features of one
// token per fragment: acc[i][j][r] = Y[t0 + j*16 + (lane&15)][n0 + i*16 + (lane>>4)*4 + r].
template <int FM, int FN, int EPI>
__global__ __launch_bounds__(512) void gemm_bf16_kernel(GemmArgs p) {
    constexpr int BNW = 2 * FM * 16, BT = 4 * FN * 16;
    constexpr int STAGE = (BNW + BT) * ROWB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int nt = blockIdx.x % p.n_tiles, tt = blockIdx.x / p.n_tiles;
    const int n0 = nt * BNW, t0 = tt * BT;
    const size_t ld = (size_t)p.K * 2;
    const char* wbase = reinterpret_cast<const char*>(p.W) + (size_t)n0 * ld;
    const char* xbase = reinterpret_cast<const char*>(p.X) + (size_t)t0 * ld;
    const int KS = p.K / 64;

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    stage_rows<BNW, 8>(wbase, ld, smem, wave, lane);
    stage_rows<BT, 8>(xbase, ld, smem + BNW * ROWB, wave, lane);
    __syncthreads();
    for (int ks = 0; ks < KS; ++ks) {
        const char* cur = smem + (ks & 1) * STAGE;
        if (ks + 1 < KS) {
            char* nxt = smem + ((ks + 1) & 1) * STAGE;
            stage_rows<BNW, 8>(wbase + (size_t)(ks + 1) * ROWB, ld, nxt, wave, lane);
            stage_rows<BT, 8>(xbase + (size_t)(ks + 1) * ROWB, ld, nxt + BNW * ROWB, wave, lane);
        }
        const char* tA = cur;
        const char* tB = cur + BNW * ROWB;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 a[FM], b[FN];
            const int c = kk * 4 + (lane >> 4);
#pragma unroll
            for (int i = 0; i < FM; ++i) a[i] = frag(tA, wm * (FM * 16) + i * 16 + (lane & 15), c);
#pragma unroll
            for (int j = 0; j < FN; ++j) b[j] = frag(tB, wn * (FN * 16) + j * 16 + (lane & 15), c);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // ---- epilogue
#pragma unroll
    for (int i = 0; i < FM; ++i) {
        const int n = n0 + wm * (FM * 16) + i * 16 + (lane >> 4) * 4;
        const float4 b4 = *reinterpret_cast<const float4*>(p.bias + n);
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            const int t = t0 + wn * (FN * 16) + j * 16 + (lane & 15);
            if (t >= p.T) continue;
            gemm_epilogue<EPI>(acc[i][j], b4, t, n, 0, p);       // (one slice: split_stride is 0)
        }
    }
}

template <int FM, int FN, int EPI>
int launch_gemm_cfg(const GemmArgs& a, int t_pad, hipStream_t stream) {
    constexpr int BNW = 2 * FM * 16, BT = 4 * FN * 16;
    constexpr int LDS = 2 * (BNW + BT) * ROWB;
    GemmArgs p = a;
    p.n_tiles = a.N / BNW;
    auto kern = gemm_bf16_kernel<FM, FN, EPI>;
    SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), LDS));
    hipLaunchKernelGGL(kern, dim3(p.n_tiles * (t_pad / BT)), dim3(512), LDS, stream, p);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

// Large-batch form: 256 x 256 tiles, PERSISTENT workgroups.  One workgroup per CU walks its tiles in a
// single flattened stream of K steps (two LDS stages; the first K step of the next tile is already in
// flight while the last one of this tile is computed), the epilogue's stores are fire-and-forget: they
// are issued after the next tile's first DMA pieces and the counted wait that ends the K step leaves
// them in flight.  Stores and DMA pieces go through inline asm so that hipcc inserts no vmcnt(0) of its
// own.  Consecutive tile ids share the token tile or the weight tile, so the 256 tiles in flight at any
// time reuse each other's operands in L2.
// Hazard audit (r03, DESIGN.md "asm stores"): the data of this store always comes out of v_cvt_pk_bf16_f32 -- a VALU
// write, which the hardware interlocks against a VMEM read of the same VGPR (no software wait states; the MFMA ->
// VALU distance in front of the pack is hipcc's, both instructions being visible to it) -- and a store of at most
// 8 bytes has read its data by the time the next instruction issues.  The 16-byte form does NOT have that second
// property (its data registers must not be written for two wait states AFTER it): r02 padded in front of it instead
// and got garbage; the large-batch epilogue's 16-byte stores are plain stores hipcc pads itself.
__device__ __forceinline__ void store_b64_asm(void* p, uint2 v) {
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
    u32x2 w;
    w.x = v.x; w.y = v.y;
    asm volatile("global_store_dwordx2 %0, %1, off" ::"v"(p), "v"(w) : "memory");
}

template <int EPI>
__global__ __launch_bounds__(512) void gemm_persistent_kernel(GemmArgs p) {
    constexpr int FM = 8, FN = 4;
    constexpr int BNW = 256, BT = 256;
    constexpr int STAGE = (BNW + BT) * ROWB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const size_t ld = (size_t)p.K * 2;
    const int KS = p.K / 64;
    const int tiles = p.n_tiles * p.t_tiles;
    // Tile walk.  Workgroups b and b + 8 share an XCD (and its 4 MiB L2): round r hands XCD x the patch
    // r * 8 + x of 4 weight tiles x 8 token tiles, one tile per workgroup, so the 32 tiles an XCD has in flight
    // read 12 operand tiles between them (a K slice of all of them is 384 KiB: it stays in that L2) instead of
    // the ~27 a strided walk touches.  Patches go weight-tile-group first, so the XCDs of one round share token
    // rows through the Infinity Cache.  Needs a full grid and n_tiles % 4 == 0; otherwise tile = b + r * grid.
    const int xcd = blockIdx.x & 7, lb = blockIdx.x >> 3;
    const bool patched = gridDim.x == 256 && (p.n_tiles & 3) == 0;
    const int NP = p.n_tiles >> 2, TP = (p.t_tiles + 7) >> 3;
    auto tile_at = [&](int r) -> int {             // linear id of this workgroup's r-th tile, < 0: none (and none later)
        if (!patched) {
            const int t = (int)blockIdx.x + r * (int)gridDim.x;
            return t < tiles ? t : -1;
        }
        const int pidx = r * 8 + xcd;
        if (pidx >= NP * TP) return -1;
        const int nt = (pidx % NP) * 4 + (lb & 3), tt = (pidx / NP) * 8 + (lb >> 2);
        return tt < p.t_tiles ? tt * p.n_tiles + nt : -1;
    };
    int my_tiles = 0;
    while (tile_at(my_tiles) >= 0) ++my_tiles;
    const int total = my_tiles * KS;
    if (total == 0) return;

    unsigned off[4];                       // per-lane source offsets of this wave's 4 pieces per operand
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (wave + 8 * i) * 8 + (lane >> 3);
        off[i] = (unsigned)(r * ld) + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
    }
    // issue cursor
    int i_round = 0, i_tile = tile_at(0), i_ks = 0;
    auto issue = [&](int s) {
        const int nt = i_tile % p.n_tiles, tt = i_tile / p.n_tiles;
        const char* ws = reinterpret_cast<const char*>(p.W) + (size_t)nt * BNW * ld + (size_t)i_ks * ROWB;
        const char* xs = reinterpret_cast<const char*>(p.X) + (size_t)tt * BT * ld + (size_t)i_ks * ROWB;
        char* buf = smem + (s & 1) * STAGE;
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma16(ws + off[i], buf + (wave + 8 * i) * 1024);
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma16(xs + off[i], buf + BNW * ROWB + (wave + 8 * i) * 1024);
        if (++i_ks == KS) { i_ks = 0; i_tile = tile_at(++i_round); }
    };

    f32x4 acc[FM][FN];
    issue(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    int round = 0, tile = tile_at(0), ks = 0;
    for (int s = 0; s < total; ++s) {
        const bool more = s + 1 < total;
        if (more) issue(s + 1);
        if (ks == 0) {
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const char* tA = smem + (s & 1) * STAGE;
        const char* tB = tA + BNW * ROWB;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 a[FM], b[FN];
            const int c = kk * 4 + (lane >> 4);
#pragma unroll
            for (int i = 0; i < FM; ++i) a[i] = frag(tA, wm * (FM * 16) + i * 16 + (lane & 15), c);
#pragma unroll
            for (int j = 0; j < FN; ++j) b[j] = frag(tB, wn * (FN * 16) + j * 16 + (lane & 15), c);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        bool stored = false;
        if (++ks == KS) {
            ks = 0;
            const int nt = tile % p.n_tiles, tt = tile / p.n_tiles;
            const int n0 = nt * BNW, t0 = tt * BT;
            // every load the epilogue needs is issued before its first store: a load hipcc can see makes it
            // wait for everything older, the stores included
            uint2 res[EPI == EPI_RESID ? FM : 1][EPI == EPI_RESID ? FN : 1];
            float4 bias4[FM];
#pragma unroll
            for (int i = 0; i < FM; ++i) {
                const int n = n0 + wm * (FM * 16) + i * 16 + (lane >> 4) * 4;
                bias4[i] = *reinterpret_cast<const float4*>(p.bias + n);
                if (EPI == EPI_RESID) {
#pragma unroll
                    for (int j = 0; j < FN; ++j) {
                        const int t = t0 + wn * (FN * 16) + j * 16 + (lane & 15);
                        res[EPI == EPI_RESID ? i : 0][EPI == EPI_RESID ? j : 0] =
                            *reinterpret_cast<const uint2*>(p.resid + (size_t)t * p.N + n);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < FM; ++i) {
                const int n = n0 + wm * (FM * 16) + i * 16 + (lane >> 4) * 4;
                const float4 b4 = bias4[i];
#pragma unroll
                for (int j = 0; j < FN; ++j) {
                    const int t = t0 + wn * (FN * 16) + j * 16 + (lane & 15);
                    // rows past T are padding of the activation buffers: written like the others (every
                    // wave then issues exactly FM * FN stores, which the counted wait below relies on)
                    float v0 = acc[i][j][0] + b4.x, v1 = acc[i][j][1] + b4.y, v2 = acc[i][j][2] + b4.z, v3 = acc[i][j][3] + b4.w;
                    const size_t o = (size_t)t * p.N + n;
                    if (EPI == EPI_RESID) {
                        const uint2 r2 = res[EPI == EPI_RESID ? i : 0][EPI == EPI_RESID ? j : 0];
                        v0 += bf16_to_f32((bf16_t)(r2.x & 0xffff)); v1 += bf16_to_f32((bf16_t)(r2.x >> 16));
                        v2 += bf16_to_f32((bf16_t)(r2.y & 0xffff)); v3 += bf16_to_f32((bf16_t)(r2.y >> 16));
                    } else if (EPI == EPI_GELU) {
                        const f32x2 g01 = gelu_erf2(f32x2{v0, v1}), g23 = gelu_erf2(f32x2{v2, v3});
                        v0 = g01[0]; v1 = g01[1]; v2 = g23[0]; v3 = g23[1];
                    }
                    // (the pre-LayerNorm sums of EPI_RESID leave as bf16 too: half the bytes written here and
                    // read by the LayerNorm kernel; the small-batch kernels keep fp32 split-K partial sums)
                    uint2 w2;
                    w2.x = pack_bf16x2(v0, v1);
                    w2.y = pack_bf16x2(v2, v3);
                    store_b64_asm(reinterpret_cast<bf16_t*>(p.out) + o, w2);
                }
            }
            tile = tile_at(++round);
            stored = true;
        }
        // next K step landed.  After an epilogue the FM * FN = 32 stores just issued are younger than its
        // DMA pieces and stay in flight.
        if (stored && more) asm volatile("s_waitcnt vmcnt(32) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int EPI>
int launch_gemm_persistent(const GemmArgs& a, int t_pad, int cu_count, hipStream_t stream, int* splits_out = nullptr) {
    constexpr int LDS = 2 * (256 + 256) * ROWB;
    GemmArgs p = a;
    p.n_tiles = a.N / 256;
    p.t_tiles = t_pad / 256;
    p.splits = 1; p.split_stride = 0;
    const int tiles = p.n_tiles * p.t_tiles;
    auto kern = gemm_persistent_kernel<EPI>;
    SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), LDS));
    hipLaunchKernelGGL(kern, dim3(std::min(tiles, cu_count)), dim3(512), LDS, stream, p);
    SQE_HIP(hipGetLastError());
    if (EPI == EPI_RESID && splits_out) *splits_out = 0;      // 0 partial sums: one bf16 row
    return SQE_OK;
}

// Small-batch form: LDS ring with counted waits (pieces issued through lds_dma16 so hipcc adds no vmcnt(0) of its own),
// optional split-K.  With a few hundred to a few thousand tokens a GEMM has about as many tiles as the chip has CUs:
// what decides its time is how many ROUNDS of tiles the grid needs and what one tile's K step costs, so the tile is
// picked per call from a menu (r03; r02 had 128 x 128 only: at 64 x 32 tokens the QKV GEMM made 384 tiles = two
// rounds, the second half empty, and ran at 0.46 PFLOP/s):
//     features x tokens   stage     ring   pieces per wave
//     (2 FM 16) x (4 FN 16)
//      64 x  64           16 KiB     4        2
//     128 x  64           24 KiB     4        3
//     192 x  64           32 KiB     4        4
//     256 x  64           40 KiB     3        5
//     128 x 128           32 KiB     4        4        (the r02 tile)
//     192 x 128           40 KiB     3        5
//     256 x 128           48 KiB     3        6
// ring_pick() takes the shape with the smallest  rounds x K steps x max(MFMA cycles, stage bytes / 28 B per cycle)
// (a CU takes in ~55 GB/s of L2-resident operands through LDS-DMA: MI355X_MICROARCH.md, indexed rows table).  The K
// loop of the two N = hidden GEMMs may also be cut into `splits` workgroups whose fp32 partial sums the LayerNorm
// kernels add up (deterministic, no atomics).
template <int EPI, int FM, int FN, int NST>
__global__ __launch_bounds__(512) void gemm_ring_kernel(GemmArgs p) {
    constexpr int BNW = 2 * FM * 16, BT = 4 * FN * 16;
    constexpr int STAGE = (BNW + BT) * ROWB;
    constexpr int PW = BNW / 8, PX = BT / 8;              // 1-KiB pieces (8 rows) of a stage: weights, then tokens
    constexpr int PIECES = (PW + PX) / 8;                 // per wave per stage
    static_assert((PW + PX) % 8 == 0, "every wave issues the same number of pieces");
    static_assert(NST * STAGE <= 160 * 1024, "LDS budget");
    constexpr int IN_FLIGHT = PIECES * (NST - 2);         // pieces the wait at the end of a K step leaves in flight
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int tiles = p.n_tiles * p.t_tiles;
    // Workgroups b and b + 8 share an XCD and its 4 MiB L2 (speed only).  When the tile grid cuts into 4 x 2 patches, XCD x
    // takes patch (x % 4, x / 4) -- a quarter of the weight tiles against half of the token tiles, all K slices of a tile
    // together -- so that what its 32 workgroups stream is a few MB that stay in its L2; a linear walk gives every XCD two
    // weight tiles against ALL tokens (at 64 x 32 tokens: 4.8 MB per XCD, served from the Infinity Cache at half the rate).
    int split, nt, tt;
    {
        const int G = gridDim.x;
        const int nq = p.n_tiles / 4, tq = p.t_tiles / 2;
        if (p.xcd_patches && (p.n_tiles & 3) == 0 && (p.t_tiles & 1) == 0 && (G & 7) == 0) {
            const int x = blockIdx.x & 7, j = blockIdx.x >> 3;          // j < nq * tq * splits
            const int per = nq * tq;
            split = j / per;
            const int jj = j - split * per;
            nt = (x & 3) * nq + jj % nq;
            tt = (x >> 2) * tq + jj / nq;
        } else {
            split = blockIdx.x / tiles;
            const int tile = blockIdx.x % tiles;
            nt = tile % p.n_tiles;
            tt = tile / p.n_tiles;
        }
    }
    const int n0 = nt * BNW, t0 = tt * BT;
    const size_t ld = (size_t)p.K * 2;
    const int KS = p.K / 64 / p.splits;
    const char* wbase = reinterpret_cast<const char*>(p.W) + (size_t)n0 * ld + (size_t)split * KS * ROWB;
    const char* xbase = reinterpret_cast<const char*>(p.X) + (size_t)t0 * ld + (size_t)split * KS * ROWB;

    // this wave's pieces: piece q = wave + 8 i of the stage; q < PW: weight rows 8 q .., else token rows 8 (q - PW) ..
    // (per-lane source: row 8 q' + (lane >> 3), 16-byte chunk (lane & 7) ^ swizzle(row))
    const char* src[PIECES];
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
        const int q = wave + 8 * i;
        const bool is_w = q < PW;
        const int r = (is_w ? q : q - PW) * 8 + (lane >> 3);
        src[i] = (is_w ? wbase : xbase) + (size_t)r * ld + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
    }
    auto issue = [&](int ks) {
        char* buf = smem + (ks % NST) * STAGE;
#pragma unroll
        for (int i = 0; i < PIECES; ++i) lds_dma16(src[i] + (size_t)ks * ROWB, buf + (wave + 8 * i) * 1024);
    };

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int s = 0; s < NST - 1 && s < KS; ++s) issue(s);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    for (int ks = 0; ks < KS; ++ks) {
        const bool more = ks + NST - 1 < KS;
        if (more) issue(ks + NST - 1);        // into the buffer K step ks - 1 used (all waves passed its barrier)
        const char* tA = smem + (ks % NST) * STAGE;
        const char* tB = tA + BNW * ROWB;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 a[FM], b[FN];
            const int c = kk * 4 + (lane >> 4);
#pragma unroll
            for (int i = 0; i < FM; ++i) a[i] = frag(tA, wm * (FM * 16) + i * 16 + (lane & 15), c);
#pragma unroll
            for (int j = 0; j < FN; ++j) b[j] = frag(tB, wn * (FN * 16) + j * 16 + (lane & 15), c);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        // K step ks + 1 landed; the younger stages stay in flight
        if (!more) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        else if (IN_FLIGHT == 4) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        else if (IN_FLIGHT == 5) asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)" ::: "memory");
        else if (IN_FLIGHT == 6) asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
        else if (IN_FLIGHT == 8) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        static_assert(IN_FLIGHT == 4 || IN_FLIGHT == 5 || IN_FLIGHT == 6 || IN_FLIGHT == 8, "a counted wait exists for this shape");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- epilogue (split-K partial sums for EPI_RESID: bias and residual are added by split 0)
#pragma unroll
    for (int i = 0; i < FM; ++i) {
        const int n = n0 + wm * (FM * 16) + i * 16 + (lane >> 4) * 4;
        float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (EPI != EPI_F32 && !(EPI == EPI_RESID && split != 0)) b4 = *reinterpret_cast<const float4*>(p.bias + n);
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            const int t = t0 + wn * (FN * 16) + j * 16 + (lane & 15);
            if (t >= p.T) continue;
            gemm_epilogue<EPI>(acc[i][j], b4, t, n, split, p);
        }
    }
}

struct RingShape { int fm, fn, nst; };
constexpr RingShape RING_MENU[7] = {{2, 1, 4}, {4, 1, 4}, {6, 1, 4}, {8, 1, 3}, {4, 2, 4}, {6, 2, 3}, {8, 2, 3}};

// estimated cycles of the whole GEMM with shape s and `splits` K slices (see the table above)
inline double ring_cost(const RingShape& s, int N, int K, int t_pad, int splits, int cu_count) {
    const int bnw = 2 * s.fm * 16, bt = 4 * s.fn * 16;
    if (N % bnw != 0 || t_pad % bt != 0) return 1e30;
    const long tiles = (long)(N / bnw) * (t_pad / bt) * splits;
    const long rounds = (tiles + cu_count - 1) / cu_count;
    const double mfma = s.fm * s.fn * 2 * 16.0;                       // cycles of one K step on a wave's SIMD
    const double mem = (bnw + bt) * 128.0 / 28.0;                     // LDS-DMA intake of a CU: ~28 B per cycle
    const double step = (mfma > mem ? mfma : mem) + 150.0;            // + barrier and issue
    const double fill = 2500.0 + (s.nst - 1) * 0.0;                   // first stages: one memory round trip
    return rounds * ((double)(K / 64 / splits) * step + fill + (splits > 1 ? 600.0 : 0.0));
}

template <int EPI, int FM, int FN, int NST>
int launch_gemm_ring_shape(const GemmArgs& p, int tiles, hipStream_t stream) {
    constexpr int LDS = NST * (2 * FM * 16 + 4 * FN * 16) * ROWB;
    auto kern = gemm_ring_kernel<EPI, FM, FN, NST>;
    SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), LDS));
    hipLaunchKernelGGL(kern, dim3(tiles * p.splits), dim3(512), LDS, stream, p);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

template <int EPI>
int launch_gemm_ring(const GemmArgs& a, int t_pad, int cu_count, size_t split_stride, int* splits_out, hipStream_t stream,
                     sqe_encoder_gemm_t* plan = nullptr) {
    GemmArgs p = a;
    // knobs build: SQE_ENC_RING=0 pins the r02 tile (128 x 128), A/B of the shape menu
    static const bool menu_on = [] { const char* e = knob_env("SQE_ENC_RING"); return !(e && e[0] == '0'); }();
    int best = 4, best_splits = 1;
    double best_cost = 1e30;
    const int ks = a.K / 64;
    for (int m = 0; m < 7; ++m) {
        if (!menu_on && m != 4) continue;
        for (int splits = 1; splits <= (EPI == EPI_RESID ? 4 : 1); splits *= 2) {
            if (splits > 1 && (ks % splits != 0 || ks / splits < 4)) continue;
            const double c = ring_cost(RING_MENU[m], a.N, a.K, t_pad, splits, cu_count);
            if (c < best_cost) { best_cost = c; best = m; best_splits = splits; }
        }
    }
    if (best_cost >= 1e30) return fail(SQE_ERR_INVALID, "encoder gemm: no ring tile fits N / padded token count");
    if (EPI == EPI_RESID) {
        // The two N = hidden GEMMs write fp32 partial sums that the LayerNorm kernel adds up: every extra K slice is
        // another T x N x 4 bytes written and read, which the cycle model above does not see.  Measured (tools/ring_tune.py,
        // whole encoder, 64 x 32 and 64 x 16 tokens, profiles/r03_configs/ring_tune_*.jsonl): out-proj (K = hidden) is
        // fastest on 64 x 64 tiles with NO split (3.03 -> 2.77 ms and 2.06 -> 1.92 ms against the model's 256 x 128 / 4
        // slices), FFN-down (K = 4 x hidden) on 128 x 128 / 2 slices from 2,048 tokens on and 128 x 64 / 2 slices below.
        // These rules cover 1,024-2,048 padded tokens (what was measured); elsewhere the model decides.
        if (t_pad >= 1024 && t_pad <= 2048 && a.N % 128 == 0) {
            if (a.K <= a.N) { best = 0; best_splits = 1; }
            else if (t_pad >= 2048) { best = 4; best_splits = ks % 2 == 0 && ks / 2 >= 4 ? 2 : 1; }
            else { best = 1; best_splits = ks % 2 == 0 && ks / 2 >= 4 ? 2 : 1; }
        }   // other token counts: the model's choice (1 x 128 tokens: 1.84 -> 1.28 ms against the r02 rule; 64 x 128: 7.63 -> 7.34)
    }
    {
        // knobs build, tuning runs (tools/ring_tune.sh): SQE_RING_FORCE_<EPI>_K<K>="menu index:splits" pins the choice for
        // the GEMMs of that epilogue and depth; SQE_RING_XCD=0 switches the XCD-aware tile walk off
        char name[64];
        snprintf(name, sizeof name, "SQE_RING_FORCE_%d_K%d", (int)EPI, a.K);
        const char* e = knob_env(name);
        int m = -1, sp = 1;
        if (e && sscanf(e, "%d:%d", &m, &sp) >= 1 && m >= 0 && m < 7 && ring_cost(RING_MENU[m], a.N, a.K, t_pad, 1, cu_count) < 1e30 &&
            (sp == 1 || (EPI == EPI_RESID && (sp == 2 || sp == 4) && ks % sp == 0))) {
            best = m;
            best_splits = sp;
        }
    }
    const RingShape sh = RING_MENU[best];
    p.n_tiles = a.N / (2 * sh.fm * 16);
    p.t_tiles = t_pad / (4 * sh.fn * 16);
    p.splits = best_splits;
    p.split_stride = split_stride;
    {
        static const bool xcd_off = [] { const char* e = knob_env("SQE_RING_XCD"); return e && e[0] == '0'; }();
        p.xcd_patches = xcd_off ? 0 : 1;
    }
    if (splits_out) *splits_out = best_splits;
    if (plan) *plan = {SQE_GEMM_RING, best, best_splits};
    const int tiles = p.n_tiles * p.t_tiles;
    switch (best) {
        case 0: return launch_gemm_ring_shape<EPI, 2, 1, 4>(p, tiles, stream);
        case 1: return launch_gemm_ring_shape<EPI, 4, 1, 4>(p, tiles, stream);
        case 2: return launch_gemm_ring_shape<EPI, 6, 1, 4>(p, tiles, stream);
        case 3: return launch_gemm_ring_shape<EPI, 8, 1, 3>(p, tiles, stream);
        case 4: return launch_gemm_ring_shape<EPI, 4, 2, 4>(p, tiles, stream);
        case 5: return launch_gemm_ring_shape<EPI, 6, 2, 3>(p, tiles, stream);
        default: return launch_gemm_ring_shape<EPI, 8, 2, 3>(p, tiles, stream);
    }
}

// A handful of tokens (T <= 64: one query, as the reference issues it): every GEMM of the layer is a few MB of
// weights against at most four 16-token groups, i.e. one memory round trip if the whole chip pulls on it at once,
// and the 128-row tiles above give it 8-32 workgroups.  Here a workgroup owns 16 output features: its 4 waves
// split K, each lane reads its MFMA fragments straight from global memory (W row n0 + (lane & 15), 16 B at
// k + 32 i + 8 (lane >> 4): 64 contiguous bytes per row per instruction; X rows the same way, L2-resident), no
// LDS staging, the four partial sums meet in LDS and wave j finishes token group j.  N / 16 workgroups (x the
// split-K factor for the two N = hidden GEMMs, whose partial sums the LayerNorm kernels already add).
template <int EPI>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(GemmArgs p) {
    __shared__ float4 red[4][4][64];          // [K-split wave][token group][lane]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int groups = p.N >> 4;
    const int split = blockIdx.x / groups;
    const int n0 = (blockIdx.x % groups) << 4;
    const int nt = (p.T + 15) >> 4;           // 16-token groups, <= 4
    const int kwave = p.K / p.splits / 4;     // K elements per wave, a multiple of 128
    const int kbeg = split * (p.K / p.splits) + wave * kwave;
    const int r = lane & 15, c = lane >> 4;
    const bf16_t* wrow = p.W + (size_t)(n0 + r) * p.K + kbeg + c * 8;
    const bf16_t* xrow = p.X + (size_t)r * p.K + kbeg + c * 8;
    const size_t xgroup = (size_t)16 * p.K;

    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // two 128-wide steps per pass, the loads of both issued before the first MFMA (kwave is 128 or 256 for the
    // BERT-large shapes: one pass, one memory round trip)
    for (int k = 0; k < kwave; k += 256) {
        bf16x8 a[2][4], b[2][4][4];
        const bool two = k + 128 < kwave;
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (h == 0 || two) {
#pragma unroll
                for (int i = 0; i < 4; ++i) a[h][i] = *reinterpret_cast<const bf16x8*>(wrow + k + h * 128 + i * 32);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nt) {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            b[h][j][i] = *reinterpret_cast<const bf16x8*>(xrow + j * xgroup + k + h * 128 + i * 32);
                    }
            }
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (h == 0 || two) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nt) {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[h][i], b[h][j][i], acc[j], 0, 0, 0);
                    }
            }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < nt) red[wave][j][lane] = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
    __syncthreads();
    if (wave >= nt) return;
    // wave j: token group j, partial sums added in wave order (deterministic)
    const int j = wave;
    float4 v = red[0][j][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const float4 u = red[w][j][lane];
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    const int t = j * 16 + r;
    if (t >= p.T) return;
    const int n = n0 + c * 4;
    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!(EPI == EPI_RESID && split != 0)) b4 = *reinterpret_cast<const float4*>(p.bias + n);
    gemm_epilogue<EPI>(f32x4{v.x, v.y, v.z, v.w}, b4, t, n, split, p);
}

template <int EPI>
int launch_gemm_skinny(const GemmArgs& a, int cu_count, size_t split_stride, int* splits_out, hipStream_t stream,
                       sqe_encoder_gemm_t* plan = nullptr) {
    GemmArgs p = a;
    int splits = 1;
    if (EPI == EPI_RESID)
        while (splits < 4 && a.K % (512 * splits * 2) == 0 && (a.N / 16) * splits * 2 <= cu_count) splits *= 2;
    p.splits = splits;
    p.split_stride = split_stride;
    if (splits_out) *splits_out = splits;
    if (plan) *plan = {SQE_GEMM_FEW_TOKEN, -1, splits};
    hipLaunchKernelGGL(gemm_skinny_kernel<EPI>, dim3((a.N / 16) * splits), dim3(256), 0, stream, p);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

// 256x256 tiles when there are enough tokens to fill the chip with them, the 128x128 ring kernel otherwise.
// *splits_out = number of fp32 partial sums written (EPI_RESID), `split_stride` floats apart; 0 = the output is
// ONE bf16 row per token (the persistent kernel).  *plan = which kernel this call launched (sqe_encoder_state).
template <int EPI>
int route_gemm(const GemmArgs& a, int t_pad, int cu_count, hipStream_t stream, size_t split_stride, int* splits_out,
               sqe_encoder_gemm_t* plan) {
    if (a.N % 128 != 0 || a.K % 64 != 0) return fail(SQE_ERR_INVALID, "encoder gemm: N % 128 or K % 64");
    if (splits_out) *splits_out = 1;
    if (EPI != EPI_F32 && a.T <= 64 && a.K % 512 == 0) {
        static const bool off = [] { const char* e = knob_env("SQE_ENC_SKINNY"); return e && e[0] == '0'; }();
        if (!off) return launch_gemm_skinny<EPI>(a, cu_count, split_stride, splits_out, stream, plan);
    }
    const bool big = a.N % 256 == 0 && t_pad % 256 == 0 && (int64_t)(a.N / 256) * (t_pad / 256) >= cu_count;
    if (big) {
        static const bool old_form = [] { const char* e = knob_env("SQE_ENC_GEMM_V0"); return e && e[0] == '1'; }();
        // the ping-pong kernel (r02: QKV 220 -> 207 us, out-proj + FFN-down 178 -> 172 us per call at 64 x 512 tokens,
        // FFN-up + GELU equal); SQE_ENC_GEMM=0 in a knobs build picks the two-stage persistent kernel it replaced
        static const int form = [] { const char* e = knob_env("SQE_ENC_GEMM"); return e ? atoi(e) : 1; }();
        if (!old_form && form == 1 && a.N <= gpp::MAX_BIAS_N) {
            if (plan) *plan = {SQE_GEMM_PING_PONG, -1, 1};
            return launch_gemm_pp(EPI, a, t_pad, cu_count, stream, splits_out);
        }
        if (!old_form) {
            if (plan) *plan = {SQE_GEMM_PERSISTENT, -1, 1};
            return launch_gemm_persistent<EPI>(a, t_pad, cu_count, stream, splits_out);
        }
        if (plan) *plan = {SQE_GEMM_ONE_TILE, -1, 1};
        GemmArgs p = a;
        p.splits = 1; p.split_stride = 0; p.t_tiles = 0;
        return launch_gemm_cfg<8, 4, EPI>(p, t_pad, stream);
    }
    return launch_gemm_ring<EPI>(a, t_pad, cu_count, split_stride, splits_out, stream, plan);
}

}  // namespace

int launch_gemm(int epi, const GemmArgs& a, int t_pad, int cu_count, hipStream_t stream, size_t split_stride, int* splits_out,
                sqe_encoder_gemm_t* plan) {
    switch (epi) {
        case EPI_BIAS: return route_gemm<EPI_BIAS>(a, t_pad, cu_count, stream, split_stride, splits_out, plan);
        case EPI_GELU: return route_gemm<EPI_GELU>(a, t_pad, cu_count, stream, split_stride, splits_out, plan);
        case EPI_RESID: return route_gemm<EPI_RESID>(a, t_pad, cu_count, stream, split_stride, splits_out, plan);
        default: return fail(SQE_ERR_INVALID, "encoder gemm: unknown epilogue");
    }
}

// scores[t][n] = <X[t], W[n]> in fp32 (bf16 operands, rows K elements apart): the IVF coarse quantiser
int launch_scores_gemm(const bf16_t* W, const bf16_t* X, float* out, int N, int K, int T, int t_pad, int cu_count, hipStream_t stream) {
    if (N % 128 != 0 || K % 64 != 0 || t_pad % 128 != 0 || T > t_pad) return fail(SQE_ERR_INVALID, "scores gemm: N % 128, K % 64, t_pad % 128");
    GemmArgs a;
    a.W = W; a.X = X; a.bias = nullptr; a.resid = nullptr; a.out = out; a.N = N; a.K = K; a.T = T; a.n_tiles = 0;
    return launch_gemm_ring<EPI_F32>(a, t_pad, cu_count, 0, nullptr, stream);
}

}  // namespace sqe
