// enc_gemm_pp.hip -- the encoder's large-batch GEMM, ping-pong schedule (namespace gpp, gemm_pp_kernel) and its
// launcher; the ablation builds (SQE_GPP_ABLATE, tools/build_gpp_ablate.sh) and the phase stamps (SQE_PHASE_STAMPS)
// compile this file alone.  The routing rule that picks it is in enc_gemm.hip.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "enc_device.h"

namespace sqe {

namespace {

// Large-batch form, ping-pong schedule (the flat scan's, scan_pp.hip, with an epilogue where the scan has its
// filter): 256 x 256 tiles, PERSISTENT workgroups, K in 32-wide half-steps through a 4-stage LDS ring, the two
// waves of a SIMD taking turns at the matrix pipe: while one computes a half-step (32 MFMAs on registers) the
// other does its memory work (4 LDS-DMA pieces, 12 ds_read_b128).
// Schedule (r04, shipped): ONE s_barrier per half-step (period T_j) instead of r02's one per phase -- the two groups no longer wait for
// each other in the middle of a period:
//     G0 (waves 0-3), T_j: compute j | [epilogue] issue pieces j + 3 | vmcnt: own pieces of j + 2 | read operands j + 1 | barrier
//     G1 (waves 4-7), T_j: [epilogue] issue pieces j + 3 | read operands j | compute j | vmcnt: own pieces of j + 2 | barrier
// Invariant, as in scan_i8.hip: a piece read in a period was retired by the wave that issued it before a barrier that precedes the
// read (every wave retires its pieces of x in T_{x-2}; x is read at the end of T_{x-1} and the head of T_x).  r03's form of this
// schedule had G0 retire its pieces of j + 1 at the head of T_j, behind the barrier -- sibling G0 waves read them unordered, the
// output of 64 x 512 tokens changed in a row or two between identical calls (7 of 30), and r03 shipped r02's schedule instead.  On
// the corrected schedule: 0 of 12 repeats at 64 x 512 tokens and 0 of 40 at 64 x 128 differ (tools/repeat_enc.py), 24.09-24.14 ->
// 23.70-23.74 ms for the encode of 64 x 512 tokens (profiles/r04_configs/enc_one_barrier_ab.log).  An epilogue always stands in
// FRONT of its period's pieces, so the plain vmcnt(4) behind them covers its stores (operations retire in issue order).
// Build 512 (tools/build_gpp_ablate.sh 512) keeps r02's schedule for A/B.
namespace gpp {
// Ablation builds of the ping-pong GEMM (tools/build_gpp_ablate.sh <bits>, timing only, results wrong): 8 = no DMA pieces,
// 16 = no operand reads, 32 = no epilogue, 64 = every tile reads the operands of tile 0 (always in L2), 128 = the pieces of a
// half-step read whole 128-B lines of 128 rows instead of 64-B halves of 256 rows (the same bytes per tile), 256 = a 5-stage
// ring (four half-steps in flight) over all 160 KiB, the bias vector read from inside it; 512 = r02's schedule, a barrier after
// every phase.  Compile-time, so
// that the shipped kernel's register allocation is the one measured (run-time switches made hipcc spill).
#ifndef SQE_GPP_ABLATE
#define SQE_GPP_ABLATE 0
#endif
using sqe::gpp::MAX_BIAS_N;                           // (encoder_kernels.h: the routing rule needs it too)
constexpr int GPP_ABLATE = SQE_GPP_ABLATE;
constexpr int HALF_K = 32, LINE_BYTES = 128, OPER_BYTES = 128 * LINE_BYTES, STAGE_BYTES = 2 * OPER_BYTES;
constexpr int NSTAGE = (GPP_ABLATE & 256) ? 5 : 4;   // (ablation 256: a 5-stage ring over ALL of the LDS, the bias vector inside it)
constexpr int AHEAD = NSTAGE - 1;                     // half-steps of DMA in flight
constexpr int RING_BYTES = NSTAGE * STAGE_BYTES;      // 128 KiB
constexpr int LDS_BYTES = (GPP_ABLATE & 256) ? RING_BYTES : RING_BYTES + MAX_BIAS_N * 4;
typedef bf16x8 AOps[8];
typedef bf16x8 BOps[4];
struct Cursor { int e, h; const char* a; const char* b; };
// DMA pieces through inline asm (common.h: lds_dma16), as in scan_pp.hip: hipcc does not see them and so never puts an
// s_waitcnt vmcnt(0) of its own in front of an LDS read; every wait for a piece is an explicit counted one.
__device__ __forceinline__ void glds16(const char* src, char* lds_wave_base) { lds_dma16(src, lds_wave_base); }
#define GPP_BARRIER()                          \
    do {                                       \
        __builtin_amdgcn_sched_barrier(0);     \
        __builtin_amdgcn_s_barrier();          \
        __builtin_amdgcn_sched_barrier(0);     \
    } while (0)
template <bool FIRST>
__device__ __forceinline__ void cmp_phase(f32x4 (&acc)[8][4], const AOps& a, const BOps& b) {
#pragma unroll
    for (int fm = 0; fm < 8; ++fm)
#pragma unroll
        for (int fn = 0; fn < 4; ++fn)
            acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[fm], b[fn], FIRST ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[fm][fn], 0, 0, 0);
}
}  // namespace gpp

// Phase timing of the ping-pong GEMM (make KNOBS=1 STAMPS=1, SQE_GEMM_DBG bit 4): core-clock sums of workgroup 0,
// waves 0 (group 0) and 4 (group 1): [0] tiles, [1] kernel, [2] epilogue, [3] memory phase after the epilogue,
// [4] barrier after it, [5] steady compute phases, [6] barriers after them, [7] steady phases counted
#ifdef SQE_PHASE_STAMPS
__device__ unsigned long long g_gemm_clk[2][8];
#define GPP_STAMP(var)                                 \
    do {                                               \
        __builtin_amdgcn_sched_barrier(0);             \
        var = __builtin_readcyclecounter();            \
        __builtin_amdgcn_sched_barrier(0);             \
    } while (0)
#define GPP_ACC(...) \
    do {             \
        __VA_ARGS__; \
    } while (0)
#else
#define GPP_STAMP(var) \
    do {               \
    } while (0)
#define GPP_ACC(...) \
    do {             \
    } while (0)
#endif

template <int EPI>
__global__ __launch_bounds__(512) void gemm_pp_kernel(GemmArgs p) {
    using namespace gpp;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* bias_lds = reinterpret_cast<float*>(smem + ((GPP_ABLATE & 256) ? 0 : RING_BYTES));
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int group = wave >> 2, wm = wave >> 2, wn = wave & 3;
    const size_t ld = (size_t)p.K * 2;
    const int HS = p.K / HALF_K;
    const int tiles = p.n_tiles * p.t_tiles;
    // tile walk: as gemm_persistent_kernel (XCD-aware 4 x 8 patches on a full grid)
    const int xcd = blockIdx.x & 7, lb = blockIdx.x >> 3;
    const bool patched = gridDim.x == 256 && (p.n_tiles & 3) == 0;
    const int NP = p.n_tiles >> 2, TP = (p.t_tiles + 7) >> 3;
    auto tile_at = [&](int r) -> int {
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
    const int J = my_tiles * HS;
    if (J == 0) return;

    // per-lane DMA source offsets (piece t covers LDS lines 8t .. 8t+7; line L holds the slices of tile rows L
    // and L + 128, chunk positions XOR-swizzled by (L >> 1) & 7) and operand read offsets: as scan_pp.hip
    unsigned off0, off1, offA0, offA1, rdA, rdB;
    {
        const int line = wave * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((line >> 1) & 7);
        const int row = line + 128 * (c >> 2);
        off0 = (unsigned)(row * ld) + (c & 3) * 16;
        off1 = off0 + (unsigned)(64 * ld);
        // Weight rows enter the tile PERMUTED inside each 128-row half: tile row p = i * 16 + g * 4 + r (fragment i,
        // lane group g, accumulator element r) holds feature (i >> 1) * 32 + g * 8 + (i & 1) * 4 + r, so that a lane's
        // fragments 2s and 2s + 1 are EIGHT consecutive features of its token: one 16-byte store, and the four lane
        // groups of a store cover 64 contiguous bytes of a token row (32-byte segments cost the epilogue ~300 cycles
        // per store instruction).  Only the source row of the DMA changes; the LDS image and the reads do not.
        auto wrow = [](int tr) {
            const int pr = tr & 127, i = pr >> 4, g = (pr >> 2) & 3, r = pr & 3;
            return (tr & 128) + (i >> 1) * 32 + g * 8 + (i & 1) * 4 + r;
        };
        offA0 = (unsigned)(wrow(row) * ld) + (c & 3) * 16;
        offA1 = (unsigned)(wrow(row + 64) * ld) + (c & 3) * 16;
        if (GPP_ABLATE & 128) {                       // whole 128-B lines: 8 lanes per row, 128 rows per half-step
            off0 = offA0 = (unsigned)(line * ld) + c * 16;
            off1 = offA1 = off0 + (unsigned)(64 * ld);
        }
        const int r = lane & 15, cq = lane >> 4, sw = (r >> 1) & 7;
        rdA = (unsigned)(r * LINE_BYTES + (((wm * 4 + cq) ^ sw) << 4));
        rdB = (unsigned)(((wn & 1) * 64 + r) * LINE_BYTES + ((((wn >> 1) * 4 + cq) ^ sw) << 4));
    }
    auto seat = [&](Cursor& c) {                      // operand tiles of entry c.e
        const int t = tile_at(c.e);
        int nt = t % p.n_tiles, tt = t / p.n_tiles;
        if (GPP_ABLATE & 64) nt = tt = 0;
        c.a = reinterpret_cast<const char*>(p.W) + (size_t)nt * 256 * ld;
        c.b = reinterpret_cast<const char*>(p.X) + (size_t)tt * 256 * ld;
    };
    auto advance = [&](Cursor& c) {
        if (++c.h == HS) {
            c.h = 0;
            if (++c.e < my_tiles) seat(c);
        }
    };
    auto issue = [&](const Cursor& c, int stage) {
        char* st = smem + stage * STAGE_BYTES;
        size_t koff = (size_t)c.h * (HALF_K * 2);
        if (GPP_ABLATE & 128) {                       // (rows 0-127 over all of K, then rows 128-255: the tile's bytes, each once)
            const size_t hh = (size_t)c.h * 128;
            koff = hh % ld + hh / ld * 128 * ld;
        }
        const char* as = c.a + koff;
        const char* bs = c.b + koff;
        glds16(as + offA0, st + wave * 1024);
        glds16(as + offA1, st + (wave + 8) * 1024);
        glds16(bs + off0, st + OPER_BYTES + wave * 1024);
        glds16(bs + off1, st + OPER_BYTES + (wave + 8) * 1024);
    };
    Cursor rd{0, 0, nullptr, nullptr}, dm{0, 0, nullptr, nullptr};
    seat(rd);
    seat(dm);
    int post_epi = 0;                                 // memory phases that still have this wave's epilogue stores in flight

    f32x4 acc[8][4];
    AOps a;
    BOps b;
    if (GPP_ABLATE & 16) {                            // (the MFMAs then compute on these)
        for (int i = 0; i < 8; ++i) a[i] = bf16x8{};
        for (int i = 0; i < 4; ++i) b[i] = bf16x8{};
    }
    // waves 0, 1 (4, 5) of a group issue their DMA pieces first and read their operands after, waves 2, 3 (6, 7) the
    // other way round: the address unit and the LDS then work side by side (scan_pp.hip: dma_and_reads)
    const bool reads_first = p.pp_stagger && ((wave >> 1) & 1);
    auto read_operands = [&](int j) {
        const char* st = smem + (NSTAGE == 4 ? (j & 3) : j % NSTAGE) * STAGE_BYTES;
#pragma unroll
        for (int fm = 0; fm < 8; ++fm) a[fm] = *reinterpret_cast<const bf16x8*>(st + rdA + fm * 2048);
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) b[fn] = *reinterpret_cast<const bf16x8*>(st + OPER_BYTES + rdB + fn * 2048);
    };
    auto mem_phase = [&](int j) {
        const bool more = j + AHEAD < J;
        const bool do_dma = more && !(GPP_ABLATE & 8);
        constexpr bool do_reads = !(GPP_ABLATE & 16);
        if (reads_first) {
            if (do_reads) read_operands(j);
            if (do_dma) issue(dm, NSTAGE == 4 ? ((j + 3) & 3) : (j + AHEAD) % NSTAGE);
        } else {
            if (do_dma) issue(dm, NSTAGE == 4 ? ((j + 3) & 3) : (j + AHEAD) % NSTAGE);
            if (do_reads) read_operands(j);
        }
        // retire the DMA of half-step j + 1; j + 2 and j + 3 stay in flight, and so do the 16 epilogue stores for
        // the two memory phases after an epilogue (they are younger than the half-step that has to land)
        if (!more) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        else if (post_epi > 0) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(16 + 4 * (AHEAD - 1)) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(4 * (AHEAD - 1)) : "memory");
        if (post_epi > 0) --post_epi;
        advance(rd);
        if (more) advance(dm);
    };
    auto epilogue = [&](int e) {
        if ((GPP_ABLATE & 32) && p.K > 0) return;         // (a run-time condition: the MFMAs stay)
        const int t = tile_at(e);
        const int nt = t % p.n_tiles, tt = t / p.n_tiles;
        const int n0 = nt * 256, t0 = tt * 256;
        // The loads an epilogue needs are issued before its first store (a load hipcc can see makes it wait for
        // everything older, the stores included).  EPI_RESID reads 64 VGPRs of residual per wave: it goes in two
        // halves of two fragment pairs, so that the kernel keeps its accumulators and the residual in registers.
        // A fragment pair (2s, 2s + 1) is eight consecutive features of the lane's token (see the row permutation
        // above): 16 stores of 16 bytes per wave.
        constexpr int HALVES = EPI == EPI_RESID ? 2 : 1;
        constexpr int SB = 4 / HALVES;                    // fragment pairs per half
#pragma unroll
        for (int half = 0; half < HALVES; ++half) {
            uint4 res[EPI == EPI_RESID ? SB : 1][EPI == EPI_RESID ? 4 : 1];
#pragma unroll
            for (int ss = 0; ss < SB; ++ss) {
                const int sp = half * SB + ss;
                const int n = n0 + wm * 128 + sp * 32 + (lane >> 4) * 8;
                if (EPI == EPI_RESID) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int tk = t0 + wn * 64 + j * 16 + (lane & 15);
                        res[EPI == EPI_RESID ? ss : 0][EPI == EPI_RESID ? j : 0] =
                            *reinterpret_cast<const uint4*>(p.resid + (size_t)tk * p.N + n);
                    }
                }
            }
            // bias from LDS (the whole vector was copied in at kernel start): no vector-memory load in the epilogue of the
            // bias / GELU kernels; all reads of a half up front, one LDS round trip (the operand registers are dead here)
            float4 ball[SB][2];
#pragma unroll
            for (int ss = 0; ss < SB; ++ss) {
                const int n = n0 + wm * 128 + (half * SB + ss) * 32 + (lane >> 4) * 8;
                ball[ss][0] = *reinterpret_cast<const float4*>(bias_lds + n);
                ball[ss][1] = *reinterpret_cast<const float4*>(bias_lds + n + 4);
            }
#pragma unroll
            for (int ss = 0; ss < SB; ++ss) {
                const int sp = half * SB + ss;
                const int n = n0 + wm * 128 + sp * 32 + (lane >> 4) * 8;
                const float4 bq[2] = {ball[ss][0], ball[ss][1]};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int tk = t0 + wn * 64 + j * 16 + (lane & 15);
                    const size_t o = (size_t)tk * p.N + n;
                    unsigned w[4];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {         // the two fragments of the pair
                        const int i = 2 * sp + q;
                        const float4 b4 = bq[q];
                        float v0 = acc[i][j][0] + b4.x, v1 = acc[i][j][1] + b4.y, v2 = acc[i][j][2] + b4.z, v3 = acc[i][j][3] + b4.w;
                        if (EPI == EPI_RESID) {
                            const uint4 r4 = res[EPI == EPI_RESID ? ss : 0][EPI == EPI_RESID ? j : 0];
                            const unsigned rx = q ? r4.z : r4.x, ry = q ? r4.w : r4.y;
                            v0 += bf16_to_f32((bf16_t)(rx & 0xffff)); v1 += bf16_to_f32((bf16_t)(rx >> 16));
                            v2 += bf16_to_f32((bf16_t)(ry & 0xffff)); v3 += bf16_to_f32((bf16_t)(ry >> 16));
                        } else if (EPI == EPI_GELU) {
                            const f32x2 g01 = gelu_poly2(f32x2{v0, v1}), g23 = gelu_poly2(f32x2{v2, v3});
                            v0 = g01[0]; v1 = g01[1]; v2 = g23[0]; v3 = g23[1];
                        }
                        w[2 * q] = pack_bf16x2(v0, v1);
                        w[2 * q + 1] = pack_bf16x2(v2, v3);
                    }
                    // a plain store: hipcc may see it (what it must not see are the DMA pieces).  The same 16-byte store
                    // through an asm block left garbage in the output in r02 -- with s_nop padding for the store-data
                    // hazard too; the 8-byte asm stores of the other GEMM kernels are fine -- cause not found, form not used.
                    if (!(p.pp_dbg & 2)) *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(p.out) + o) = uint4{w[0], w[1], w[2], w[3]};
                }
            }
        }
        post_epi = AHEAD - 1;
        __builtin_amdgcn_sched_barrier(0);
    };

    // ---- the bias vector into LDS (N <= MAX_BIAS_N: the launcher checks), then the prologue: half-steps 0, 1, 2
    if (!(GPP_ABLATE & 256))
        for (int i = tid * 4; i < p.N; i += 512 * 4) *reinterpret_cast<float4*>(bias_lds + i) = *reinterpret_cast<const float4*>(p.bias + i);
    for (int s = 0; s < AHEAD && s < J; ++s) {
        issue(dm, s);
        advance(dm);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the prologue's pieces (inline asm: the compiler does not wait for them)
    __syncthreads();                       // prologue landed

    int j = 0;
#ifdef SQE_PHASE_STAMPS
    unsigned long long k0 = 0, t0 = 0, t1 = 0, t2 = 0, t3 = 0, c0 = 0, c1 = 0, c2 = 0, clk[8] = {};
#endif
    GPP_STAMP(k0);
    static_assert(!(GPP_ABLATE & 256) || (GPP_ABLATE & 512), "the five-stage ring experiment runs on r02's schedule: build 768");
    if (!(GPP_ABLATE & 512)) {
        // SHIPPED (r04): one barrier per half-step (the schedule and its invariant: comment above the kernel, scan_i8.hip); build 512
        // keeps r02's loop, a barrier after every phase, below
        auto issue_next = [&](int jj) {
            if (jj + 3 < J && !(GPP_ABLATE & 8)) {
                issue(dm, (jj + 3) & 3);
                advance(dm);
            }
        };
        // at the end of T_jj: everything this wave has in flight but the four pieces of jj + 3 it issued LAST in this period
        // (vector-memory operations retire in issue order: epilogue stores and residual loads are older entries)
        auto wait_pieces = [&](int jj) {
            if (jj + 3 < J && !(GPP_ABLATE & 8)) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        };
        if (group == 0) {
            read_operands(0);
            for (int e = 0; e < my_tiles; ++e) {
                cmp_phase<true>(acc, a, b);
                issue_next(j);
                wait_pieces(j);
                if (j + 1 < J) read_operands(j + 1);
                GPP_BARRIER();
                ++j;
                for (int h = 1; h < HS - 1; ++h) {
                    // (stamps of this form: [3] memory part, [4] barrier, [5] compute part, per steady period)
                    GPP_STAMP(c0);
                    cmp_phase<false>(acc, a, b);
                    GPP_STAMP(c1);
                    issue_next(j);
                    wait_pieces(j);
                    if (j + 1 < J) read_operands(j + 1);
                    GPP_STAMP(c2);
                    GPP_BARRIER();
                    GPP_STAMP(t0);
                    GPP_ACC(clk[5] += c1 - c0; clk[3] += c2 - c1; clk[4] += t0 - c2; ++clk[7]; ++clk[0]);
                    ++j;
                }
                // last period of a tile: the epilogue goes in FRONT of the period's pieces, so that the plain vmcnt(4) covers its stores
                cmp_phase<false>(acc, a, b);
                epilogue(e);
                issue_next(j);
                wait_pieces(j);
                if (j + 1 < J) read_operands(j + 1);
                GPP_BARRIER();
                ++j;
            }
        } else {
            for (int e = 0; e < my_tiles; ++e) {
                if (e > 0) epilogue(e - 1);                  // beside G0's compute part; in front of this period's pieces
                issue_next(j);
                read_operands(j);
                cmp_phase<true>(acc, a, b);
                wait_pieces(j);
                GPP_BARRIER();
                ++j;
                for (int h = 1; h < HS; ++h) {
                    GPP_STAMP(c0);
                    issue_next(j);
                    read_operands(j);
                    GPP_STAMP(c1);
                    cmp_phase<false>(acc, a, b);
                    GPP_STAMP(c2);
                    wait_pieces(j);
                    GPP_BARRIER();
                    GPP_STAMP(t0);
                    GPP_ACC(clk[3] += c1 - c0; clk[5] += c2 - c1; clk[4] += t0 - c2; ++clk[7]; ++clk[0]);
                    ++j;
                }
            }
            epilogue(my_tiles - 1);
        }
    } else if (group == 0) {
        mem_phase(0);
        GPP_BARRIER();
        for (int e = 0; e < my_tiles; ++e) {
            cmp_phase<true>(acc, a, b);
            GPP_BARRIER();
            mem_phase(j + 1);
            GPP_BARRIER();
            ++j;
            for (int h = 1; h < HS - 1; ++h) {
                GPP_STAMP(c0);
                cmp_phase<false>(acc, a, b);
                GPP_STAMP(c1);
                GPP_BARRIER();
                GPP_STAMP(c2);
                GPP_ACC(clk[5] += c1 - c0; clk[6] += c2 - c1; ++clk[7]);
                mem_phase(j + 1);
                GPP_BARRIER();
                ++j;
            }
            cmp_phase<false>(acc, a, b);
            GPP_BARRIER();
            GPP_STAMP(t0);
            epilogue(e);
            GPP_STAMP(t1);
            if (j + 1 < J) mem_phase(j + 1);
            GPP_STAMP(t2);
            GPP_BARRIER();
            GPP_STAMP(t3);
            GPP_ACC(clk[2] += t1 - t0; clk[3] += t2 - t1; clk[4] += t3 - t2; ++clk[0]);
            ++j;
        }
    } else {
        GPP_BARRIER();
        for (int e = 0; e < my_tiles; ++e) {
            GPP_STAMP(t0);
            if (e > 0) epilogue(e - 1);
            GPP_STAMP(t1);
            mem_phase(j);
            GPP_STAMP(t2);
            GPP_BARRIER();
            GPP_STAMP(t3);
            GPP_ACC(if (e > 0) { clk[2] += t1 - t0; clk[3] += t2 - t1; clk[4] += t3 - t2; ++clk[0]; });
            cmp_phase<true>(acc, a, b);
            GPP_BARRIER();
            ++j;
            for (int h = 1; h < HS; ++h) {
                mem_phase(j);
                GPP_BARRIER();
                GPP_STAMP(c0);
                cmp_phase<false>(acc, a, b);
                GPP_STAMP(c1);
                GPP_BARRIER();
                GPP_STAMP(c2);
                GPP_ACC(clk[5] += c1 - c0; clk[6] += c2 - c1; ++clk[7]);
                ++j;
            }
        }
        epilogue(my_tiles - 1);
    }
#ifdef SQE_PHASE_STAMPS
    if ((p.pp_dbg & 4) && blockIdx.x == 0 && (wave == 0 || wave == 4) && lane == 0) {
        clk[1] = __builtin_readcyclecounter() - k0;
        for (int i = 0; i < 8; ++i) g_gemm_clk[wave >> 2][i] = clk[i];
    }
#endif
}

template <int EPI>
int launch_gemm_pp_epi(const GemmArgs& a, int t_pad, int cu_count, hipStream_t stream, int* splits_out) {
    GemmArgs p = a;
    p.n_tiles = a.N / 256;
    p.t_tiles = t_pad / 256;
    p.splits = 1; p.split_stride = 0;
    static const int stagger = [] { const char* e = knob_env("SQE_GEMM_STAGGER"); return e ? atoi(e) : 1; }();   // knobs build: A/B
    p.pp_stagger = stagger;
    static const int ppdbg = [] { const char* e = knob_env("SQE_GEMM_DBG"); return e ? atoi(e) : 0; }();
    p.pp_dbg = ppdbg;
    const int tiles = p.n_tiles * p.t_tiles;
    auto kern = gemm_pp_kernel<EPI>;
    SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), gpp::LDS_BYTES));
    hipLaunchKernelGGL(kern, dim3(std::min(tiles, cu_count)), dim3(512), gpp::LDS_BYTES, stream, p);
    SQE_HIP(hipGetLastError());
#ifdef SQE_PHASE_STAMPS
    if (p.pp_dbg & 4) {
        static int printed[3] = {0, 0, 0};
        if (printed[EPI]++ == 30) {                      // one launch well after warm-up, per epilogue kind
            unsigned long long h[2][8];
            SQE_HIP(hipStreamSynchronize(stream));
            SQE_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_gemm_clk), sizeof(h)));
            for (int g = 0; g < 2; ++g) {
                const double t = (double)std::max<unsigned long long>(h[g][0], 1), n = (double)std::max<unsigned long long>(h[g][7], 1);
                fprintf(stderr, "[sqe dbg] gemm_pp<%d> N=%d K=%d group %d: kernel %llu cycles, %llu tile epilogues: epilogue %.0f, memory phase after it %.0f, "
                                "barrier %.0f | steady compute phase %.0f + barrier %.0f (%llu phases)\n",
                        EPI, p.N, p.K, g, h[g][1], h[g][0], h[g][2] / t, h[g][3] / t, h[g][4] / t, h[g][5] / n, h[g][6] / n, h[g][7]);
            }
        }
    }
#endif
    if (EPI == EPI_RESID && splits_out) *splits_out = 0;      // 0 partial sums: one bf16 row
    return SQE_OK;
}

}  // namespace

int launch_gemm_pp(int epi, const GemmArgs& a, int t_pad, int cu_count, hipStream_t stream, int* splits_out) {
    switch (epi) {
        case EPI_BIAS: return launch_gemm_pp_epi<EPI_BIAS>(a, t_pad, cu_count, stream, splits_out);
        case EPI_GELU: return launch_gemm_pp_epi<EPI_GELU>(a, t_pad, cu_count, stream, splits_out);
        case EPI_RESID: return launch_gemm_pp_epi<EPI_RESID>(a, t_pad, cu_count, stream, splits_out);
        default: return fail(SQE_ERR_INVALID, "encoder gemm: unknown epilogue");
    }
}

}  // namespace sqe
