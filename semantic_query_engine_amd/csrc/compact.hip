// compact.hip -- row deletion (sqe_index_delete): stable in-place compaction of an index and the id map it leaves.
//
// An index that never had a delete has no map: a row's id is its position, exactly as before.  The first delete creates
// `idmap` (int64 [cap], position -> local id, strictly increasing); from then on the live rows slide down over the deleted
// ones keeping their order, so what the scan / filter / select / certificate kernels see is exactly a fresh index built from
// the live rows in id order, and "ties to the lowest position" stays "ties to the lowest id".  Searches run on positions and
// translate_ids_kernel maps the returned positions to ids on the device (index_search_impl, once the search is done).
//
// The move.  dest(i) = i - (deleted positions below i) <= i, so with many workgroups in flight a row could be overwritten
// before its own mover has read it.  The rows from the first deleted position on are walked in blocks [b0, b1):
//   * staged block (fewer than b1 - b0 rows deleted below b0): one launch reads the block's live rows into a bounded staging
//     buffer, a second writes them to their destinations;
//   * direct block (at least b1 - b0 rows deleted below b0): dest(b1 - 1) < b0, so one launch moves the rows in place.
// Invariant: every destination of a block lies below b1, and every row below b0 has already been read (by an earlier launch
// on the same stream).  Writes of a block therefore only hit rows that are consumed, and peak extra HBM is the staging
// buffer, never a second copy of the index.
//
// dest(i) comes from a binary search of the sorted deleted positions (the host sorts them anyway to reject repeats), which is
// the prefix sum of the keep mask evaluated where it is needed: no [n] mask or destination array is materialised.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "id_lists.h"
#include "internal.h"

namespace sqe {

namespace {

constexpr size_t STAGE_BYTES = 128u << 20;      // staging buffer of the staged blocks

__global__ __launch_bounds__(256) void idmap_iota_kernel(int64_t* __restrict__ map, int64_t first_pos, int64_t first_id, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) map[first_pos + i] = first_id + i;
}

// pos_out[j] = position of ids[j] in the strictly increasing map[0, n), or -1
__global__ __launch_bounds__(256) void idmap_lookup_kernel(const int64_t* __restrict__ map, int64_t n, const int64_t* __restrict__ ids,
                                                           int64_t m, int64_t* __restrict__ pos_out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    pos_out[j] = resolve_id(map, n, ids[j]);
}

// id_out[j] = position >= 0 ? map[position] (the position itself with a null map) + id_base : -1
__global__ __launch_bounds__(256) void translate_ids_kernel(int64_t* __restrict__ ids, int64_t count, const int64_t* __restrict__ map,
                                                            int64_t id_base) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= count) return;
    const int64_t p = ids[j];
    ids[j] = p >= 0 ? (map ? map[p] : p) + id_base : -1;
}

// an empty result: (-inf, -1) and, with keys, SQE_KEY_NONE
__global__ __launch_bounds__(256) void pad_hits_kernel(float* __restrict__ cos, int64_t* __restrict__ ids, int64_t* __restrict__ keys,
                                                       int64_t count) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= count) return;
    cos[j] = -INFINITY;
    ids[j] = -1;
    if (keys) keys[j] = SQE_KEY_NONE;
}

enum { MOVE_TO_STAGE = 0, MOVE_FROM_STAGE = 1, MOVE_DIRECT = 2 };

struct MoveArgs {
    float* master;            // [cap, dim] fp32
    char* scan;               // [cap] rows of `pitch` bytes (dim bf16 payload)
    int64_t* map;             // [cap] ids
    int64_t* keys;            // [cap] group keys (collapse.hip); null: the index has none
    int* assign;              // IVF list of each row, rows [0, assign_n); null without IVF assignments
    int64_t assign_n;
    int dim, pitch;
    const int64_t* del;       // deleted positions, sorted
    int64_t m_del;
    int64_t b0, b1;           // the block
    char* stage;              // staging: row i of the block at (i - b0) * stage_pitch: master | scan payload | id | list | key
    int64_t stage_pitch;
    int mode;
};

// n vectors of one row by one wave: the loads of a round (U per lane, a whole row up to dim 2048) issue before its stores
template <typename V, int U>
__device__ __forceinline__ void copy_row(const V* __restrict__ src, V* __restrict__ dst, int n, int lane) {
    for (int v0 = 0; v0 < n; v0 += 64 * U) {
        V r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int v = v0 + u * 64 + lane;
            r[u] = v < n ? src[v] : V{};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int v = v0 + u * 64 + lane;
            if (v < n) dst[v] = r[u];
        }
    }
}

// One wave per row of the block.  The payloads are multiples of 256 B (dim % 64 == 0), moved as 16-B vectors.
__global__ __launch_bounds__(256) void compact_move_kernel(MoveArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t i = a.b0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.b1) return;
    bool hit;
    const int64_t below = del_rank(a.del, a.m_del, i, &hit);
    if (hit) return;                                   // a deleted row: nobody reads it again
    const int64_t d = i - below;
    const int nf = a.dim >> 2, ns = a.dim >> 3;        // float4 of the master row, int4 of the bf16 payload
    const int64_t sl = i - a.b0;
    const float4* mf;
    const int4* sf;
    int64_t id, key = 0;
    int lst = 0;
    const bool has_list = a.assign && i < a.assign_n;
    if (a.mode == MOVE_FROM_STAGE) {
        const char* st = a.stage + sl * a.stage_pitch;
        mf = reinterpret_cast<const float4*>(st);
        sf = reinterpret_cast<const int4*>(st + (size_t)a.dim * 4);
        id = *reinterpret_cast<const int64_t*>(st + (size_t)a.dim * 6);
        lst = *reinterpret_cast<const int*>(st + (size_t)a.dim * 6 + 8);
        if (a.keys) key = *reinterpret_cast<const int64_t*>(st + (size_t)a.dim * 6 + 16);
    } else {
        mf = reinterpret_cast<const float4*>(a.master + i * (int64_t)a.dim);
        sf = reinterpret_cast<const int4*>(a.scan + i * (int64_t)a.pitch);
        id = a.map[i];
        if (has_list) lst = a.assign[i];
        if (a.keys) key = a.keys[i];
    }
    float4* mt;
    int4* stt;
    if (a.mode == MOVE_TO_STAGE) {
        char* st = a.stage + sl * a.stage_pitch;
        mt = reinterpret_cast<float4*>(st);
        stt = reinterpret_cast<int4*>(st + (size_t)a.dim * 4);
        if (lane == 0) {
            *reinterpret_cast<int64_t*>(st + (size_t)a.dim * 6) = id;
            *reinterpret_cast<int*>(st + (size_t)a.dim * 6 + 8) = lst;
            if (a.keys) *reinterpret_cast<int64_t*>(st + (size_t)a.dim * 6 + 16) = key;
        }
    } else {
        mt = reinterpret_cast<float4*>(a.master + d * (int64_t)a.dim);
        stt = reinterpret_cast<int4*>(a.scan + d * (int64_t)a.pitch);
        if (lane == 0) {
            a.map[d] = id;
            if (has_list) a.assign[d] = lst;
            if (a.keys) a.keys[d] = key;
        }
    }
    copy_row<float4, 8>(mf, mt, nf, lane);
    copy_row<int4, 4>(sf, stt, ns, lane);
}

}  // namespace

// ================================================================ launchers
int launch_idmap_iota(int64_t* map, int64_t first_pos, int64_t first_id, int64_t n, hipStream_t s) {
    if (n <= 0) return SQE_OK;
    hipLaunchKernelGGL(idmap_iota_kernel, dim3(grid_of(n, 256)), dim3(256), 0, s, map, first_pos, first_id, n);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_idmap_lookup(const int64_t* map, int64_t n, const int64_t* ids, int64_t m, int64_t* pos_out, hipStream_t s) {
    if (m <= 0) return SQE_OK;
    hipLaunchKernelGGL(idmap_lookup_kernel, dim3(grid_of(m, 256)), dim3(256), 0, s, map, n, ids, m, pos_out);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_translate_ids(int64_t* ids, int64_t count, const int64_t* map, int64_t id_base, hipStream_t s) {
    if (count <= 0) return SQE_OK;
    hipLaunchKernelGGL(translate_ids_kernel, dim3(grid_of(count, 256)), dim3(256), 0, s, ids, count, map, id_base);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_pad_hits(float* cos, int64_t* ids, int64_t* keys, int64_t count, hipStream_t s) {
    if (count <= 0) return SQE_OK;
    hipLaunchKernelGGL(pad_hits_kernel, dim3(grid_of(count, 256)), dim3(256), 0, s, cos, ids, keys, count);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

// ================================================================ id lists: the host side of the calls that take them
int list_args_ok(const char* who, const char* ids_name, int min_list, sqe_index* idx, const void* q, int B, int k, const void* list_ids,
                 const int64_t* offsets, int n_lists, const int32_t* list_of_query, const void* cos, const void* ids) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (B < 0 || k < 1 || k > MAX_KP) return fail(SQE_ERR_INVALID, std::string(who) + "need B >= 0 and 1 <= k <= 256");
    if (n_lists < 0) return fail(SQE_ERR_INVALID, std::string(who) + "n_lists < 0");
    if (B > 0 && (!q || !cos || !ids || !list_of_query)) return fail(SQE_ERR_INVALID, std::string(who) + "null buffer");
    if (n_lists > 0) {
        if (!offsets) return fail(SQE_ERR_INVALID, std::string(who) + "null list_offsets");
        if (offsets[0] != 0) return fail(SQE_ERR_INVALID, std::string(who) + "list_offsets must start at 0");
        for (int f = 0; f < n_lists; ++f)
            if (offsets[f + 1] < offsets[f]) return fail(SQE_ERR_INVALID, std::string(who) + "list_offsets decrease");
        if (offsets[n_lists] > 0 && !list_ids) return fail(SQE_ERR_INVALID, std::string(who) + "null " + ids_name);
    }
    for (int b = 0; b < B; ++b)
        if (list_of_query[b] < min_list || list_of_query[b] >= n_lists)
            return fail(SQE_ERR_INVALID, std::string(who) + "list_of_query[" + std::to_string(b) + "] names no list");
    return SQE_OK;
}

int list_ids_to_host(sqe_ctx* ctx, const int64_t* ids_dev, const int64_t* offsets, int n_lists, std::vector<int64_t>& out) {
    const int64_t total = n_lists > 0 ? offsets[n_lists] : 0;
    out.resize((size_t)total);
    SQE_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream.load();
    if (total > 0) SQE_HIP(hipMemcpyAsync(out.data(), ids_dev, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));
    return SQE_OK;
}

int stage_host_ids(DevBuf& buf, const int64_t* host, int64_t count, hipStream_t s, const int64_t** dev) {
    *dev = nullptr;
    if (count <= 0) return SQE_OK;
    SQE_TRY(buf.ensure((size_t)count * 8));
    SQE_HIP(hipMemcpyAsync(buf.p, host, (size_t)count * 8, hipMemcpyHostToDevice, s));
    *dev = buf.as<int64_t>();
    return SQE_OK;
}

// ================================================================ index operations (caller holds the index lock; stream s)
int64_t search_id_base(const sqe_index* idx) { return idx->has_map ? 0 : idx->id_base; }

int index_translate_ids(sqe_index* idx, int64_t* id_dev, int64_t count, hipStream_t s) {
    if (!idx->has_map) return SQE_OK;
    return launch_translate_ids(id_dev, count, idx->idmap.as<int64_t>(), idx->id_base, s);
}

int index_positions_to_ids(sqe_index* idx, int64_t* id_dev, int64_t count, hipStream_t s) {
    if (!idx->has_map && idx->id_base == 0) return SQE_OK;
    return launch_translate_ids(id_dev, count, idx->has_map ? idx->idmap.as<int64_t>() : nullptr, idx->id_base, s);
}

int index_resolve_ids(sqe_index* idx, const int64_t* ids_host, int64_t m, std::vector<int64_t>& pos, hipStream_t s, const char* what) {
    const int64_t n = idx->n.load();
    pos.resize((size_t)m);
    if (!idx->has_map) {
        for (int64_t j = 0; j < m; ++j) {
            if (ids_host[j] < 0 || ids_host[j] >= n) return fail(SQE_ERR_INVALID, std::string(what) + ": id " + std::to_string(ids_host[j]) + " is not in the index");
            pos[(size_t)j] = ids_host[j];
        }
        return SQE_OK;
    }
    if (m == 0) return SQE_OK;
    DevBuf tmp;
    SQE_TRY(tmp.ensure((size_t)m * 16));
    int64_t* ids_dev = tmp.as<int64_t>();
    int64_t* pos_dev = ids_dev + m;
    SQE_HIP(hipMemcpyAsync(ids_dev, ids_host, (size_t)m * 8, hipMemcpyHostToDevice, s));
    SQE_TRY(launch_idmap_lookup(idx->idmap.as<int64_t>(), n, ids_dev, m, pos_dev, s));
    SQE_HIP(hipMemcpyAsync(pos.data(), pos_dev, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));
    for (int64_t j = 0; j < m; ++j)
        if (pos[(size_t)j] < 0) return fail(SQE_ERR_INVALID, std::string(what) + ": id " + std::to_string(ids_host[j]) + " is not in the index");
    return SQE_OK;
}

int index_ensure_map(sqe_index* idx, hipStream_t s) {
    if (idx->has_map) return SQE_OK;
    SQE_TRY(idx->idmap.ensure((size_t)std::max<int64_t>(idx->cap, 1) * 8));
    SQE_TRY(launch_idmap_iota(idx->idmap.as<int64_t>(), 0, 0, idx->n.load(), s));
    idx->has_map = true;
    return SQE_OK;
}

int index_ids_host(sqe_index* idx, std::vector<int64_t>& out, hipStream_t s) {
    const int64_t n = idx->n.load();
    out.resize((size_t)n);
    if (!idx->has_map) {
        for (int64_t i = 0; i < n; ++i) out[(size_t)i] = i;
        return SQE_OK;
    }
    if (n > 0) SQE_HIP(hipMemcpyAsync(out.data(), idx->idmap.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    SQE_HIP(hipStreamSynchronize(s));
    return SQE_OK;
}

int index_set_ids(sqe_index* idx, const int64_t* ids_host, int64_t next_id, hipStream_t s) {
    const int64_t n = idx->n.load();
    for (int64_t i = 0; i < n; ++i)
        if (ids_host[i] < 0 || ids_host[i] >= next_id || (i > 0 && ids_host[i] <= ids_host[i - 1]))
            return fail(SQE_ERR_IO, "sqe_index_load: the saved ids are not strictly increasing below next_id");
    SQE_TRY(idx->idmap.ensure((size_t)std::max<int64_t>(idx->cap, 1) * 8));
    if (n > 0) SQE_HIP(hipMemcpyAsync(idx->idmap.p, ids_host, (size_t)n * 8, hipMemcpyHostToDevice, s));
    SQE_HIP(hipStreamSynchronize(s));
    idx->has_map = true;
    idx->next_id.store(next_id);
    return SQE_OK;
}

// Remove the rows at `pos` (sorted ascending, distinct, all < n).
int index_delete_positions(sqe_index* idx, const std::vector<int64_t>& pos, hipStream_t s) {
    const int64_t m = (int64_t)pos.size();
    if (m == 0) return SQE_OK;
    const int64_t n_old = idx->n.load(), n_new = n_old - m, p0 = pos[0];
    const int dim = idx->dim, pitch = idx->pitch;
    SQE_TRY(index_ensure_map(idx, s));
    IvfState* ivf = idx->ivf;
    int* assign = nullptr;
    int64_t assign_n = 0;
    if (ivf) ivf_assignments(ivf, &assign, &assign_n);
    DevBuf del, stage;
    SQE_TRY(del.ensure((size_t)m * 8));
    SQE_HIP(hipMemcpyAsync(del.p, pos.data(), (size_t)m * 8, hipMemcpyHostToDevice, s));
    const int64_t stage_pitch = round_up((int64_t)dim * 6 + (idx->has_keys ? 24 : 12), 16);   // the key slot only where keys exist
    const int64_t w = std::max<int64_t>(256, (int64_t)(STAGE_BYTES / (size_t)stage_pitch));
    sqe_delete_last_t L{};                                // what sqe_index_delete_last reports: written as the loop launches
    L.n_old = n_old; L.n_new = n_new; L.first_pos = p0; L.block_rows = w;
    {
        StageTimer t(idx->ctx->prof, s, ST_ADD);
        MoveArgs a;
        a.master = idx->master; a.scan = reinterpret_cast<char*>(idx->scan); a.map = idx->idmap.as<int64_t>();
        a.keys = idx->has_keys ? idx->keys.as<int64_t>() : nullptr;
        a.assign = assign; a.assign_n = assign_n; a.dim = dim; a.pitch = pitch; a.del = del.as<int64_t>(); a.m_del = m;
        a.stage = nullptr; a.stage_pitch = stage_pitch;
        size_t k = 0;                                     // deleted positions below b0
        for (int64_t b0 = p0; b0 < n_old;) {
            while (k < pos.size() && pos[k] < b0) ++k;
            const int64_t shift = (int64_t)k;
            a.b0 = b0;
            if (shift >= w) {
                // direct: the block is no longer than the shift below it, so every destination lies below b0
                a.b1 = std::min(n_old, b0 + shift);
                a.mode = MOVE_DIRECT;
                hipLaunchKernelGGL(compact_move_kernel, dim3(grid_of(a.b1 - a.b0, 4)), dim3(256), 0, s, a);
                L.direct_blocks += 1; L.direct_rows += a.b1 - a.b0;
            } else {
                a.b1 = std::min(n_old, b0 + w);
                if (!stage.p) {
                    SQE_TRY(stage.ensure((size_t)std::min(w, n_old - p0) * stage_pitch));
                    a.stage = stage.as<char>();
                    L.stage_bytes = (int64_t)stage.bytes;
                }
                L.staged_blocks += 1; L.staged_rows += a.b1 - a.b0;
                a.mode = MOVE_TO_STAGE;
                hipLaunchKernelGGL(compact_move_kernel, dim3(grid_of(a.b1 - a.b0, 4)), dim3(256), 0, s, a);
                a.mode = MOVE_FROM_STAGE;
                hipLaunchKernelGGL(compact_move_kernel, dim3(grid_of(a.b1 - a.b0, 4)), dim3(256), 0, s, a);
            }
            SQE_HIP(hipGetLastError());
            b0 = a.b1;
        }
    }
    // the freed tail reads as zero again: the bf16 copy is "zero past n" (tile padding of the scan), the master likewise
    SQE_HIP(hipMemsetAsync(idx->scan + (size_t)n_new * (pitch / 2), 0, (size_t)m * pitch, s));
    SQE_HIP(hipMemsetAsync(idx->master + (size_t)n_new * dim, 0, (size_t)m * dim * 4, s));
    if (idx->has_keys) SQE_TRY(launch_fill_i64(idx->keys.as<int64_t>() + n_new, m, SQE_KEY_NONE, s));   // appended rows start without a key
    // int8 copy: not moved.  Rows from the tile of the first deleted position on are quantised again by the next int8 search
    // (whole tiles, rows past n written as zero vectors); the tiles that lie wholly past the new end are zeroed here.
    if (idx->i8db.p) {
        idx->i8_rows = std::min(idx->i8_rows, p0 / SCAN_BM * SCAN_BM);
        const int64_t t_lo = (n_new + SCAN_BM - 1) / SCAN_BM, t_hi = std::min((n_old + SCAN_BM - 1) / SCAN_BM, idx->i8_cap_tiles);
        if (t_hi > t_lo) {
            SQE_HIP(hipMemsetAsync(idx->i8db.as<char>() + (size_t)t_lo * idx->i8_tile_stride, 0, (size_t)(t_hi - t_lo) * idx->i8_tile_stride, s));
            SQE_HIP(hipMemsetAsync(idx->i8sxi.as<uint32_t>() + (size_t)t_lo * SCAN_BM, 0, (size_t)(t_hi - t_lo) * SCAN_BM * 4, s));
        }
    }
    // resid_max / i8resid_max are maxima over rows: they stay valid upper bounds and are left as they are
    if (ivf) {
        // live rows below the old n_assigned
        const int64_t below = assign_n - (int64_t)(std::lower_bound(pos.begin(), pos.end(), assign_n) - pos.begin());
        ivf_rows_deleted(ivf, below);
    }
    if (idx->fields) SQE_TRY(fields_rows_deleted(idx, del.as<int64_t>(), m, n_old, s));   // the field columns, each in a kernel of its own
    idx->n.store(n_new);
    idx->delete_last = L;
    SQE_HIP(hipStreamSynchronize(s));                     // the staging and position buffers die here
    return SQE_OK;
}

}  // namespace sqe

// ================================================================ C ABI
using namespace sqe;

extern "C" {

int sqe_index_delete(sqe_index* idx, const int64_t* ids_host, int64_t n) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (n < 0 || (n > 0 && !ids_host)) return fail(SQE_ERR_INVALID, "sqe_index_delete: bad arguments");
    if (n == 0) return SQE_OK;
    if (idx->group) return group_index_delete(idx, ids_host, n);
    OpScope op(idx->ctx, idx->ord, true);
    std::vector<int64_t> pos;
    SQE_TRY(index_resolve_ids(idx, ids_host, n, pos, op.s, "sqe_index_delete"));
    std::sort(pos.begin(), pos.end());
    if (std::adjacent_find(pos.begin(), pos.end()) != pos.end()) return fail(SQE_ERR_INVALID, "sqe_index_delete: an id repeats");
    return index_delete_positions(idx, pos, op.s);
}

int sqe_index_delete_last(sqe_index* idx, sqe_delete_last_t* out) {
    if (!idx || !out) return fail(SQE_ERR_INVALID, "sqe_index_delete_last: null argument");
    if (idx->group) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_delete_last: single-device indexes only");
    OpScope op(idx->ctx, idx->ord, true);
    if (idx->delete_last.n_old == 0) return fail(SQE_ERR_STATE, "sqe_index_delete_last: no row of this index was deleted yet");
    *out = idx->delete_last;
    return SQE_OK;
}

int sqe_index_ids(sqe_index* idx, int64_t* ids_out_host, int64_t cap) {
    if (!idx || (!ids_out_host && cap > 0)) return fail(SQE_ERR_INVALID, "sqe_index_ids: null argument");
    if (idx->group) return group_index_ids(idx, ids_out_host, cap);
    OpScope op(idx->ctx, idx->ord, true);
    std::vector<int64_t> ids;
    SQE_TRY(index_ids_host(idx, ids, op.s));
    if ((int64_t)ids.size() > cap) return fail(SQE_ERR_INVALID, "sqe_index_ids: cap is smaller than the live count");
    if (!ids.empty()) memcpy(ids_out_host, ids.data(), ids.size() * 8);
    return SQE_OK;
}

int sqe_index_next_id(const sqe_index* idx, int64_t* out) {
    if (!idx || !out) return fail(SQE_ERR_INVALID, "sqe_index_next_id: null argument");
    *out = idx->next_id.load();
    return SQE_OK;
}

}  // extern "C"
