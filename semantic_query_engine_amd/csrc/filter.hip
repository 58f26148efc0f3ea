// filter.hip -- filtered k-NN search (sqe_index_search_filtered): the exact top-k over the live rows whose ids are on an
// allow-list.
//
// The scan kernels know nothing of filters.  A filtered search instead copies the allowed rows into a small internal FLAT
// index of its owner (the "sub-index", created lazily the way the IVF coarse quantiser is) and runs the unchanged bf16
// pipeline on it: scan, select, certificate, collect fallback.
//   1. ids -> positions: each id is resolved (position = id without an id map, a binary search of the map with one) and
//      marked in an n-bit bitmap with vector atomics, which drops repeats and sorts for free.  The bitmap is compacted into
//      an ascending position list (per-block popcount, exclusive scan, write) and its length M is read back once.
//   2. gather: the allowed rows are copied into the sub-index bit for bit, the fp32 master row and the stored bf16 row
//      as they are.  The sub-index inherits the owner's resid_max (a bound over every row is a bound over any subset).
//   3. search: the sub-index's positions are mapped through the position list to owner positions.  More than
//      `filter_gather_rows` allowed rows are searched chunk by chunk and merged on owner positions (ties: lowest id);
//      the owner's id map or id_base is applied once at the end.
// The call is split at the bitmap (filter_bitmap_ensure / filter_bitmap_mark before it, index_search_bitmap from the popcount on):
// a field predicate (fields.hip) fills or narrows the same map and runs the same second half.
// Nothing gathered survives the call, so adds, updates and deletes between calls are always seen.  The owner's own search
// buffers (int8 copy, candidate lists, fallback buffers, i8_last) are never touched.
#include <string.h>

#include <algorithm>
#include <vector>

#include "id_lists.h"
#include "internal.h"

namespace sqe {

struct FilterState {
    sqe_index* sub = nullptr;      // internal FLAT index of the gathered rows (runs under the owner's lock and stream)
    int64_t hwm = 0;               // rows [0, hwm) of the sub-index's bf16 copy may be nonzero
    DevBuf bits;                   // u32 [words]: the allow bitmap over owner positions
    DevBuf counts;                 // i32 [blocks] set bits per bitmap block | i64 [blocks] their exclusive scan | i64 total
    DevBuf pos;                    // i64 [min(n_allow, n)] ascending owner positions of the allowed rows
    DevBuf allow;                  // i64 [n_allow] the allow-list of the host entry points
    DevBuf work;                   // two [B, k] results (cos | ids) merged across chunks
};

namespace {

constexpr int WORDS_PER_BLOCK = 1024;            // 256 threads x one 16-B load of the bitmap: 32768 positions per block
constexpr int GATHER_ROWS_PER_WAVE = 4;

__global__ __launch_bounds__(256) void filter_mark_kernel(const int64_t* __restrict__ ids, int64_t m, const int64_t* __restrict__ map,
                                                          int64_t n, uint32_t* __restrict__ bits) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const int64_t p = resolve_id(map, n, ids[j]);
    if (p >= 0) atomicOr(bits + (p >> 5), 1u << (p & 31));
}

// sum over the 256 threads of a block; every thread gets the total.  red: 4 ints of LDS
__device__ __forceinline__ int block_sum(int v, int* red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ int popc4(uint4 w) { return __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w); }

__global__ __launch_bounds__(256) void filter_count_kernel(const uint4* __restrict__ bits, int* __restrict__ counts) {
    __shared__ int red[4];
    const int c = popc4(bits[(int64_t)blockIdx.x * 256 + threadIdx.x]);
    const int t = block_sum(c, red);
    if (threadIdx.x == 0) counts[blockIdx.x] = t;
}

// one workgroup: offs[b] = sum of counts[0, b), *total = sum of all
__global__ __launch_bounds__(256) void filter_scan_kernel(const int* __restrict__ counts, int64_t nb, int64_t* __restrict__ offs,
                                                          int64_t* __restrict__ total) {
    __shared__ int64_t sh[256];
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += 256) {
        const int64_t b = b0 + threadIdx.x;
        const int64_t v = b < nb ? counts[b] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {        // inclusive Hillis-Steele scan
            const int64_t add = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (b < nb) offs[b] = carry + sh[threadIdx.x] - v;
        carry += sh[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// the set bits of a block's 1024 words, in ascending order, to pos[offs[block] ..]
__global__ __launch_bounds__(256) void filter_write_kernel(const uint4* __restrict__ bits, const int64_t* __restrict__ offs,
                                                           int64_t* __restrict__ pos) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint4 w = bits[t];
    const int c = popc4(w);
    int incl = c;                                  // inclusive prefix within the wave
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int before = 0;
    for (int i = 0; i < wv; ++i) before += wsum[i];
    if (c == 0) return;
    int64_t o = offs[blockIdx.x] + before + incl - c;
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t x = ws[i];
        const int64_t base = (t * 4 + i) * 32;
        while (x) {
            const int b = __ffs(x) - 1;
            pos[o++] = base + b;
            x &= x - 1;
        }
    }
}

struct GatherArgs {
    const float* src_master;   // [n, dim] fp32 of the owner
    const char* src_scan;      // owner rows of src_pitch bytes (dim bf16 payload)
    float* dst_master;         // [m, dim] fp32 of the sub-index
    char* dst_scan;            // sub-index rows of dst_pitch bytes
    const int64_t* pos;        // [m] owner positions
    int64_t m;
    int dim, src_pitch, dst_pitch;
};

// R rows of one wave: U 16-B vectors per lane and row are loaded for all R rows before any of them is stored
template <typename V, int U, int R>
__device__ __forceinline__ void gather_rows(const char* src, int64_t src_stride, char* dst, int64_t dst_stride, const int64_t* p,
                                            int64_t d0, int rows, int nv, int lane) {
    for (int v0 = 0; v0 < nv; v0 += 64 * U) {
        V r[R][U];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const V* s = reinterpret_cast<const V*>(src + p[i] * src_stride);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int v = v0 + u * 64 + lane;
                r[i][u] = (i < rows && v < nv) ? s[v] : V{};
            }
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            V* d = reinterpret_cast<V*>(dst + (d0 + i) * dst_stride);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int v = v0 + u * 64 + lane;
                if (i < rows && v < nv) d[v] = r[i][u];
            }
        }
    }
}

// Row j of the sub-index = owner row pos[j]: its fp32 master row and its bf16 payload, bit for bit.  One wave per
// GATHER_ROWS_PER_WAVE consecutive rows; payloads are multiples of 128 B (dim % 64 == 0), moved as 16-B vectors.
__global__ __launch_bounds__(256) void filter_gather_kernel(GatherArgs a) {
    constexpr int R = GATHER_ROWS_PER_WAVE;
    const int lane = threadIdx.x & 63;
    const int64_t d0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
    if (d0 >= a.m) return;
    const int rows = (int)std::min<int64_t>(R, a.m - d0);
    int64_t p[R];
#pragma unroll
    for (int i = 0; i < R; ++i) p[i] = i < rows ? a.pos[d0 + i] : 0;
    gather_rows<float4, 2, R>(reinterpret_cast<const char*>(a.src_master), (int64_t)a.dim * 4, reinterpret_cast<char*>(a.dst_master),
                              (int64_t)a.dim * 4, p, d0, rows, a.dim >> 2, lane);
    gather_rows<int4, 2, R>(a.src_scan, a.src_pitch, a.dst_scan, a.dst_pitch, p, d0, rows, a.dim >> 3, lane);
}

// the sub-index holds at least `rows` rows (never more than the larger of `rows` and the cap's rounding); contents are not kept
int sub_reserve(sqe_index* sub, int64_t rows, int64_t limit, FilterState* f, hipStream_t s) {
    if (rows <= sub->cap) return SQE_OK;
    const int64_t want = std::min(limit, std::max(rows, sub->cap + sub->cap / 2));
    SQE_HIP(hipStreamSynchronize(s));                    // nothing may still read the old buffers
    if (sub->master) (void)hipFree(sub->master);
    if (sub->scan) (void)hipFree(sub->scan);
    sub->master = nullptr;
    sub->scan = nullptr;
    sub->cap = 0;
    sub->n.store(0);
    f->hwm = 0;
    return index_grow(sub, std::max(rows, want), s);     // zeroes the whole bf16 copy
}

// The scratch sub-index of the owner, created on first use, with the owner's options as they stand: what the plain search reads
// ("certify", "rescore_k", the residual maximum: a bound over every row is a bound over any subset) and the budgets of the
// searches within.hip runs on it.  It starts every call without keys.
int sub_prepare(sqe_index* idx, FilterState* f, hipStream_t s) {
    if (!f->sub) SQE_TRY(index_create_impl(idx->ctx, idx->dim, SQE_INDEX_FLAT, 0, true, &f->sub));
    sqe_index* sub = f->sub;
    sub->certify = idx->certify;
    sub->rescore_k = idx->rescore_k;
    sub->collapse_depth = idx->collapse_depth;
    sub->range_key_budget = idx->range_key_budget;
    sub->mmr_row_budget = idx->mmr_row_budget;
    sub->has_keys = false;
    SQE_TRY(sub->resid_max.ensure(16));
    SQE_HIP(hipMemcpyAsync(sub->resid_max.p, idx->resid_max.p, 16, hipMemcpyDeviceToDevice, s));
    return SQE_OK;
}

// owner rows pos[0, m) into sub rows [0, m), which are then all its rows; rows [m, hwm) of its bf16 copy read as zero again
int sub_gather(sqe_index* idx, FilterState* f, const int64_t* pos, int64_t m, hipStream_t s) {
    sqe_index* sub = f->sub;
    StageTimer t(idx->ctx->prof, s, ST_PREP);
    GatherArgs a;
    a.src_master = idx->master; a.src_scan = reinterpret_cast<const char*>(idx->scan);
    a.dst_master = sub->master; a.dst_scan = reinterpret_cast<char*>(sub->scan);
    a.pos = pos; a.m = m; a.dim = idx->dim; a.src_pitch = idx->pitch; a.dst_pitch = sub->pitch;
    const int64_t waves = (m + GATHER_ROWS_PER_WAVE - 1) / GATHER_ROWS_PER_WAVE;
    hipLaunchKernelGGL(filter_gather_kernel, dim3(grid_of(waves, 4)), dim3(256), 0, s, a);
    SQE_HIP(hipGetLastError());
    if (f->hwm > m)
        SQE_HIP(hipMemsetAsync(reinterpret_cast<char*>(sub->scan) + (size_t)m * sub->pitch, 0, (size_t)(f->hwm - m) * sub->pitch, s));
    f->hwm = m;
    sub->n.store(m);
    return SQE_OK;
}

FilterState* filter_state(sqe_index* idx) {
    if (!idx->filter) idx->filter = new (std::nothrow) FilterState;
    return idx->filter;
}

}  // namespace

void filter_destroy(FilterState* f) {
    if (!f) return;
    if (f->sub) sqe_index_destroy(f->sub);
    delete f;
}

// The allow bitmap of the index as it stands: u32 words, bit p & 31 of word p >> 5, zero-padded to whole blocks of 1,024 words
// and zero at or beyond n.  *words_out is its length; the count / scan buffers are sized with it.
int filter_bitmap_ensure(sqe_index* idx, FilterState** f_out, int64_t* words_out) {
    FilterState* f = filter_state(idx);
    if (!f) return fail(SQE_ERR_OOM, "sqe_index_search_filtered: host allocation failed");
    const int64_t words = round_up((idx->n.load() + 31) / 32, WORDS_PER_BLOCK), nb = words / WORDS_PER_BLOCK;
    SQE_TRY(f->bits.ensure((size_t)words * 4));
    SQE_TRY(f->counts.ensure((size_t)nb * 4 + (size_t)nb * 8 + 16));
    *f_out = f;
    *words_out = words;
    return SQE_OK;
}

uint32_t* filter_bitmap(FilterState* f) { return f->bits.as<uint32_t>(); }

// ---- 1a. ids -> their rows' bits: the map is cleared and every allowed live row marked
int filter_bitmap_mark(sqe_index* idx, FilterState* f, int64_t words, const int64_t* allow_dev, int64_t n_allow, hipStream_t s) {
    SQE_HIP(hipMemsetAsync(f->bits.p, 0, (size_t)words * 4, s));
    hipLaunchKernelGGL(filter_mark_kernel, dim3(grid_of(n_allow, 256)), dim3(256), 0, s, allow_dev, n_allow,
                       idx->has_map ? idx->idmap.as<int64_t>() : nullptr, idx->n.load(), f->bits.as<uint32_t>());
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int stage_allow_ids(FilterState* f, const int64_t* allow_host, int64_t n_allow, hipStream_t s, const int64_t** dev) {
    return stage_host_ids(f->allow, allow_host, n_allow, s, dev);
}

// the count / scan / write steps over any map of that layout: counts holds nb ints, then (8-byte aligned) nb offsets and the total
int launch_bitmap_count(const uint32_t* bits, int64_t nb, int* counts, int64_t* offs, int64_t* total, hipStream_t s) {
    if (nb <= 0) {
        SQE_HIP(hipMemsetAsync(total, 0, 8, s));
        return SQE_OK;
    }
    hipLaunchKernelGGL(filter_count_kernel, dim3((unsigned)nb), dim3(256), 0, s, reinterpret_cast<const uint4*>(bits), counts);
    hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(256), 0, s, counts, nb, offs, total);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_bitmap_write(const uint32_t* bits, int64_t nb, const int64_t* offs, int64_t* pos, hipStream_t s) {
    if (nb <= 0) return SQE_OK;
    hipLaunchKernelGGL(filter_write_kernel, dim3((unsigned)nb), dim3(256), 0, s, reinterpret_cast<const uint4*>(bits), offs, pos);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

// Caller holds the index lock; everything runs on stream s.  allow_dev: device ids [n_allow]; outputs [B, k] on the device.
int index_search_filtered_impl(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* allow_dev, int64_t n_allow,
                               float* cos_out_dev, int64_t* id_out_dev, hipStream_t s) {
    const int64_t n = idx->n.load();
    if (n == 0 || n_allow == 0) return launch_pad_hits(cos_out_dev, id_out_dev, nullptr, (int64_t)B * k, s);
    FilterState* f;
    int64_t words;
    SQE_TRY(filter_bitmap_ensure(idx, &f, &words));
    {
        StageTimer t(idx->ctx->prof, s, ST_PREP);
        SQE_TRY(filter_bitmap_mark(idx, f, words, allow_dev, n_allow, s));
    }
    return index_search_bitmap(idx, f, words, std::min(n_allow, n), q_dev, B, k, cos_out_dev, id_out_dev, s);
}

// The filtered search from its bitmap on (filled by filter_bitmap_mark, by the field match kernel, or by both): at most pos_cap
// bits are set.  Synchronises s once, for the number of allowed rows.
int index_search_bitmap(sqe_index* idx, FilterState* f, int64_t words, int64_t pos_cap, const float* q_dev, int B, int k,
                        float* cos_out_dev, int64_t* id_out_dev, hipStream_t s) {
    int64_t M = 0;
    SQE_TRY(index_bitmap_positions(idx, f, words, pos_cap, &M, s));
    return index_search_gathered(idx, f, M, q_dev, B, k, cos_out_dev, id_out_dev, s);
}

// Its first half: the map -> the ascending positions of its set bits and their number *M_out, read back (the one synchronisation).
int index_bitmap_positions(sqe_index* idx, FilterState* f, int64_t words, int64_t pos_cap, int64_t* M_out, hipStream_t s) {
    sqe_ctx* c = idx->ctx;
    const int64_t nb = words / WORDS_PER_BLOCK;
    SQE_TRY(f->pos.ensure((size_t)pos_cap * 8));
    int* counts = f->counts.as<int>();
    int64_t* offs = reinterpret_cast<int64_t*>(f->counts.as<char>() + round_up(nb * 4, 8));
    int64_t* total = offs + nb;
    int64_t* pos = f->pos.as<int64_t>();
    int64_t M = 0;
    {
        // ---- 1b. the map -> ascending owner positions
        StageTimer t(c->prof, s, ST_PREP);
        hipLaunchKernelGGL(filter_count_kernel, dim3((unsigned)nb), dim3(256), 0, s, f->bits.as<uint4>(), counts);
        hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(256), 0, s, counts, nb, offs, total);
        hipLaunchKernelGGL(filter_write_kernel, dim3((unsigned)nb), dim3(256), 0, s, f->bits.as<uint4>(), offs, pos);
        SQE_HIP(hipGetLastError());
        SQE_HIP(hipMemcpyAsync(&M, total, 8, hipMemcpyDeviceToHost, s));
    }
    SQE_HIP(hipStreamSynchronize(s));                    // the one read-back: M plans the chunks
    *M_out = M;
    return SQE_OK;
}

// Its second half: the M positions index_bitmap_positions left in the state are gathered, searched and mapped to ids.
int index_search_gathered(sqe_index* idx, FilterState* f, int64_t M, const float* q_dev, int B, int k, float* cos_out_dev,
                          int64_t* id_out_dev, hipStream_t s, bool as_positions) {
    const int64_t bk = (int64_t)B * k;
    int64_t* pos = f->pos.as<int64_t>();
    if (M == 0) return launch_pad_hits(cos_out_dev, id_out_dev, nullptr, bk, s);
    SQE_TRY(sub_prepare(idx, f, s));
    sqe_index* sub = f->sub;
    const int64_t chunk = std::min(M, idx->filter_gather_rows);
    const int64_t n_chunks = (M + chunk - 1) / chunk;
    SQE_TRY(sub_reserve(sub, chunk, idx->filter_gather_rows, f, s));
    float* cos2 = nullptr;
    int64_t* ids2 = nullptr;
    if (n_chunks > 1) {
        const int64_t cb = round_up(2 * bk * 4, 16);
        SQE_TRY(f->work.ensure((size_t)cb + (size_t)bk * 16));
        cos2 = f->work.as<float>();
        ids2 = reinterpret_cast<int64_t*>(f->work.as<char>() + cb);
    }
    for (int64_t ci = 0; ci < n_chunks; ++ci) {
        const int64_t c0 = ci * chunk, m = std::min(chunk, M - c0);
        // ---- 2. gather rows pos[c0, c0 + m) into sub rows [0, m)
        SQE_TRY(sub_gather(idx, f, pos + c0, m, s));
        // ---- 3. search the gathered rows; sub positions -> owner positions
        float* co = n_chunks == 1 ? cos_out_dev : cos2 + (ci == 0 ? 0 : bk);
        int64_t* io = n_chunks == 1 ? id_out_dev : ids2 + (ci == 0 ? 0 : bk);
        SQE_TRY(index_search_impl(sub, q_dev, B, k, 0, co, io, s));
        SQE_TRY(launch_translate_ids(io, bk, pos + c0, 0, s));
        if (ci > 0) {
            // ---- 4. running result (part 0) merged with this chunk's (part 1) on owner positions: ties to the lowest
            SQE_TRY(launch_merge_topk(cos2, ids2, 0, 2, B, k, cos_out_dev, id_out_dev, 1, 0, 0, s));
            if (ci + 1 < n_chunks) {
                SQE_HIP(hipMemcpyAsync(cos2, cos_out_dev, (size_t)bk * 4, hipMemcpyDeviceToDevice, s));
                SQE_HIP(hipMemcpyAsync(ids2, id_out_dev, (size_t)bk * 8, hipMemcpyDeviceToDevice, s));
            }
        }
    }
    // owner positions -> ids (+ id_base)
    return as_positions ? SQE_OK : index_positions_to_ids(idx, id_out_dev, bk, s);
}

// Rows pos[0, M) of the owner (M <= "filter_gather_rows": one chunk) copied into the scratch sub-index, which then holds exactly
// them, and with with_keys their group keys (has_keys follows the owner).  The sub-index inherits the owner's options as
// index_search_gathered sets them, and the budgets of the searches within.hip runs on it.  *pos_out: the positions, for the way back.
int filter_gather_sub(sqe_index* idx, FilterState* f, int64_t M, bool with_keys, sqe_index** sub_out, const int64_t** pos_out, hipStream_t s) {
    if (M <= 0 || M > idx->filter_gather_rows) return fail(SQE_ERR_STATE, "filter_gather_sub: the row set does not fit one chunk");
    SQE_TRY(sub_prepare(idx, f, s));
    sqe_index* sub = f->sub;
    SQE_TRY(sub_reserve(sub, M, idx->filter_gather_rows, f, s));
    const int64_t* pos = f->pos.as<int64_t>();
    SQE_TRY(sub_gather(idx, f, pos, M, s));
    if (with_keys && idx->has_keys) {
        if (sub->keys.bytes < (size_t)sub->cap * 8) {
            SQE_HIP(hipStreamSynchronize(s));                // nothing may still read the old column
            SQE_TRY(sub->keys.ensure((size_t)sub->cap * 8));
        }
        SQE_TRY(launch_keys_gather(idx->keys.as<int64_t>(), pos, sub->keys.as<int64_t>(), M, s));
        sub->has_keys = true;
    }
    *sub_out = sub;
    *pos_out = pos;
    return SQE_OK;
}

// the same with a host allow-list, staged in the index's own buffer (the call synchronises s before it returns to the host)
int index_search_filtered_host_ids(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* allow_host, int64_t n_allow,
                                   float* cos_out_dev, int64_t* id_out_dev, hipStream_t s) {
    FilterState* f = filter_state(idx);
    if (!f) return fail(SQE_ERR_OOM, "sqe_index_search_filtered: host allocation failed");
    const int64_t* allow_dev;
    SQE_TRY(stage_host_ids(f->allow, allow_host, n_allow, s, &allow_dev));
    SQE_TRY(index_search_filtered_impl(idx, q_dev, B, k, allow_dev, n_allow, cos_out_dev, id_out_dev, s));
    SQE_HIP(hipStreamSynchronize(s));                    // allow_host is not retained past return
    return SQE_OK;
}

}  // namespace sqe

// ================================================================ C ABI
using namespace sqe;

extern "C" {

static int filtered_args_ok(sqe_index* idx, const void* q, int B, int k, const void* allow, int64_t n_allow, const void* cos, const void* ids) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (B < 0 || k < 1 || k > MAX_KP) return fail(SQE_ERR_INVALID, "sqe_index_search_filtered: need B >= 0 and 1 <= k <= 256");
    if (B > 0 && (!q || !cos || !ids)) return fail(SQE_ERR_INVALID, "sqe_index_search_filtered: null buffer");
    if (n_allow < 0 || (n_allow > 0 && !allow)) return fail(SQE_ERR_INVALID, "sqe_index_search_filtered: bad allow-list");
    return SQE_OK;
}

int sqe_index_search_filtered(sqe_index* idx, const float* q_host, int B, int k, const int64_t* allow_ids_host, int64_t n_allow,
                              float* cos_out_host, int64_t* id_out_host) {
    SQE_TRY(filtered_args_ok(idx, q_host, B, k, allow_ids_host, n_allow, cos_out_host, id_out_host));
    if (B == 0) return SQE_OK;
    if (idx->group) return group_index_search(idx, q_host, B, k, 0, cos_out_host, id_out_host, false, allow_ids_host, n_allow);
    OpScope op(idx->ctx, idx->ord, true);
    const size_t qbytes = (size_t)B * idx->dim * 4, cb = (size_t)B * k * 4, ib = (size_t)B * k * 8;
    SQE_TRY(idx->stage_in.ensure(qbytes));
    SQE_TRY(idx->stage_out.ensure(round_up((int64_t)cb, 16) + ib));
    float* cos_dev = idx->stage_out.as<float>();
    int64_t* id_dev = reinterpret_cast<int64_t*>(idx->stage_out.as<char>() + round_up((int64_t)cb, 16));
    SQE_HIP(hipMemcpyAsync(idx->stage_in.p, q_host, qbytes, hipMemcpyHostToDevice, op.s));
    SQE_TRY(index_search_filtered_host_ids(idx, idx->stage_in.as<float>(), B, k, allow_ids_host, n_allow, cos_dev, id_dev, op.s));
    SQE_HIP(hipMemcpyAsync(cos_out_host, cos_dev, cb, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(id_out_host, id_dev, ib, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_search_filtered_device(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* allow_ids_dev, int64_t n_allow,
                                     float* cos_out_dev, int64_t* id_out_dev) {
    SQE_TRY(filtered_args_ok(idx, q_dev, B, k, allow_ids_dev, n_allow, cos_out_dev, id_out_dev));
    if (B == 0) return SQE_OK;
    if (idx->group) {
        std::vector<int64_t> allow;
        SQE_TRY(rowset_allow_to_host(idx, allow_ids_dev, n_allow, allow));
        return group_index_search(idx, q_dev, B, k, 0, cos_out_dev, id_out_dev, true, allow.data(), n_allow);
    }
    OpScope op(idx->ctx, idx->ord, false);
    return index_search_filtered_impl(idx, q_dev, B, k, allow_ids_dev, n_allow, cos_out_dev, id_out_dev, op.s);
}

}  // extern "C"
