// api.hip -- the C ABI of include/sqe.h: error text, context, life cycle and options of the flat vector index, the
// extern "C" entry points, persistence, cache scan and stats.  The search pipeline the search entry points run is in
// search.hip.  No C++ types or exceptions cross this boundary.  Locking and stream discipline: internal.h.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "internal.h"

namespace sqe {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

// Rows allocated for the index (never shrinks).  Runs on the operation's stream, which OpScope has ordered
// after every earlier operation of this index on any stream: once the copy on `s` has finished nothing
// can still read the old buffers.
int index_grow(sqe_index* idx, int64_t need_rows, hipStream_t s) {
    if (need_rows <= idx->cap) return SQE_OK;
    const int64_t n = idx->n.load();
    int64_t new_cap = std::max<int64_t>(need_rows, idx->cap + idx->cap / 2);
    new_cap = round_up(std::max<int64_t>(new_cap, 1024), SCAN_BM);
    const size_t row_f = (size_t)idx->dim * 4, row_b = (size_t)idx->pitch;
    float* nm = nullptr;
    bf16_t* ns = nullptr;
    hipError_t e = hipMalloc((void**)&nm, (size_t)new_cap * row_f);
    if (e != hipSuccess) return fail(SQE_ERR_OOM, std::string("index master alloc: ") + hipGetErrorString(e));
    e = hipMalloc((void**)&ns, (size_t)new_cap * row_b);
    if (e != hipSuccess) { (void)hipFree(nm); return fail(SQE_ERR_OOM, std::string("index scan-copy alloc: ") + hipGetErrorString(e)); }
    // rows past n of the scanned copy must read as zero (tile padding)
    SQE_HIP(hipMemsetAsync(ns, 0, (size_t)new_cap * row_b, s));
    if (n > 0) {
        SQE_HIP(hipMemcpyAsync(nm, idx->master, (size_t)n * row_f, hipMemcpyDeviceToDevice, s));
        SQE_HIP(hipMemcpyAsync(ns, idx->scan, (size_t)n * row_b, hipMemcpyDeviceToDevice, s));
    }
    DevBuf nmap;
    if (idx->has_map) {
        // the id map grows with the rows (position -> id of rows [0, n))
        SQE_TRY(nmap.ensure((size_t)new_cap * 8));
        if (n > 0) SQE_HIP(hipMemcpyAsync(nmap.p, idx->idmap.p, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    }
    DevBuf nkeys;
    if (idx->has_keys) {
        // so do the group keys (collapse.hip): rows [0, n) keep theirs, every other position reads SQE_KEY_NONE
        SQE_TRY(nkeys.ensure((size_t)new_cap * 8));
        SQE_TRY(launch_fill_i64(nkeys.as<int64_t>() + n, new_cap - n, SQE_KEY_NONE, s));
        if (n > 0) SQE_HIP(hipMemcpyAsync(nkeys.p, idx->keys.p, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    }
    if (idx->fields) SQE_TRY(fields_grow(idx, n, new_cap, s));      // the field columns (fields.hip) likewise
    SQE_HIP(hipStreamSynchronize(s));
    if (idx->has_map) {
        std::swap(nmap.p, idx->idmap.p);
        std::swap(nmap.bytes, idx->idmap.bytes);
    }
    if (idx->has_keys) {
        std::swap(nkeys.p, idx->keys.p);
        std::swap(nkeys.bytes, idx->keys.bytes);
    }
    if (idx->master) (void)hipFree(idx->master);
    if (idx->scan) (void)hipFree(idx->scan);
    idx->master = nm;
    idx->scan = ns;
    idx->cap = new_cap;
    return SQE_OK;
}

// append rows (normalise, or pass through bit for bit when `restore`: rows read back from a saved index)
int index_add_impl(sqe_index* idx, const float* x_dev, int64_t n, int64_t x_stride, bool restore, hipStream_t s) {
    if (n <= 0) return SQE_OK;
    const int64_t have = idx->n.load();
    if (have + n > 0xFFFFFFF0LL) return fail(SQE_ERR_INVALID, "sqe_index_add: more than 2^32 rows per shard");
    SQE_TRY(index_grow(idx, have + n, s));
    if (!idx->resid_max.p) {
        SQE_TRY(idx->resid_max.ensure(16));
        SQE_HIP(hipMemsetAsync(idx->resid_max.p, 0, 16, s));
    }
    {
        StageTimer t(idx->ctx->prof, s, ST_ADD);
        float* mdst = idx->master + (size_t)have * idx->dim;
        bf16_t* sdst = idx->scan + (size_t)have * (idx->pitch / 2);
        if (restore) SQE_TRY(launch_restore_rows(x_dev, n, idx->dim, x_stride, mdst, sdst, idx->pitch / 2, idx->resid_max.as<uint32_t>(), s));
        else SQE_TRY(launch_normalize_rows(x_dev, n, idx->dim, x_stride, mdst, sdst, idx->pitch / 2, nullptr, idx->resid_max.as<uint32_t>(), s));
    }
    // new rows get ids next_id ..: without a map that is their position
    if (idx->has_map) SQE_TRY(launch_idmap_iota(idx->idmap.as<int64_t>(), have, idx->next_id.load(), n, s));
    idx->next_id.fetch_add(n);
    idx->n.store(have + n);
    if (idx->ivf) SQE_TRY(ivf_rows_added(idx, idx->ivf, s));
    return SQE_OK;
}

int index_update_impl(sqe_index* idx, const int64_t* rows_dev, const float* x_dev, int64_t n, hipStream_t s) {
    if (n <= 0) return SQE_OK;
    SQE_TRY(launch_normalize_rows_scatter(x_dev, rows_dev, n, idx->dim, idx->master, idx->scan, idx->pitch / 2,
                                          idx->resid_max.as<uint32_t>(), s));
    if (idx->ivf) SQE_TRY(ivf_rows_updated(idx, idx->ivf, rows_dev, n, s));   // only the overwritten rows are re-assigned
    // the int8 copy follows (rows past i8_rows are quantised again by the next search; the residual maximum only grows)
    if (idx->i8db.p && idx->i8_cap_tiles == idx->cap / SCAN_BM)
        SQE_TRY(launch_quantize_rows_i8(idx->master, rows_dev, 0, n, idx->n.load(), idx->dim, idx->i8db.as<int8_t>(), idx->i8_tile_stride,
                                        idx->i8sxi.as<uint32_t>(), idx->i8resid_max.as<uint32_t>(), s));
    else idx->i8_rows = 0;
    idx->i8_dx_stale = true;      // the index grew since the copy was made: the next search rebuilds it from the master, whole
    return SQE_OK;
}

int index_create_impl(sqe_ctx* ctx, int dim, int kind, int nlist, bool internal, sqe_index** out) {
    *out = nullptr;
    if (dim <= 0 || dim % SCAN_BK != 0 || dim > 8192)
        return fail(SQE_ERR_INVALID, "sqe_index_create: dim must be a positive multiple of 64 (<= 8192)");
    if (kind != SQE_INDEX_FLAT && kind != SQE_INDEX_IVF_FLAT) return fail(SQE_ERR_INVALID, "sqe_index_create: unknown index kind");
    if (kind == SQE_INDEX_IVF_FLAT && (nlist < 1 || nlist > (1 << 20)))
        return fail(SQE_ERR_INVALID, "sqe_index_create: IVF needs 1 <= nlist <= 2^20");
    SQE_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<sqe_index> idx(new (std::nothrow) sqe_index);
    if (!idx) return fail(SQE_ERR_OOM, "sqe_index_create: host allocation failed");
    idx->ctx = ctx;
    idx->dim = dim;
    idx->kind = kind;
    idx->nlist = nlist;
    idx->internal = internal;
    // FLAT indexes take the int8 first pass wherever it applies (>= i8_min_rows rows, dim >= 256 and a multiple of 128,
    // k <= i8_sample_m, rows that quantise within i8_max_resid); everything else -- small indexes, IVF, the coarse quantiser's
    // own index -- runs the bf16 scan.  Both are exact (sqe.h: SQE_SCAN_*).
    idx->scan_mode = (kind == SQE_INDEX_FLAT && !internal) ? SQE_SCAN_INT8_RESCORE : SQE_SCAN_BF16_RESCORE;
    if (!internal) SQE_TRY(idx->ord.init());
    {
        // rows of the scanned copy are padded by one 128-B line by default: with a 2^n pitch every
        // row of a K slice would sit in the same memory channel
        const char* e = knob_env("SQE_ROW_PAD");
        const int pad = e ? atoi(e) : 128;
        idx->pitch = dim * 2 + (pad >= 0 && pad % 8 == 0 ? pad : 128);
    }
    if (kind == SQE_INDEX_IVF_FLAT) {
        int rc = ivf_create(idx.get(), &idx->ivf);
        if (rc == SQE_OK) ivf_coarse(idx->ivf)->certify = 0;   // probes are approximate by nature
        if (rc != SQE_OK) { ivf_destroy(idx->ivf); idx->ord.destroy(); return rc; }
    }
    *out = idx.release();
    return SQE_OK;
}

}  // namespace sqe

using namespace sqe;

// ================================================================ library / context
extern "C" {

int sqe_version(void) { return SQE_VERSION; }
const char* sqe_last_error(void) { return g_last_error.c_str(); }

static int ctx_init_device(sqe_ctx* c, int device) {
    int count = 0;
    SQE_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(SQE_ERR_INVALID, "sqe_create: no such HIP device");
    c->device = device;
    SQE_HIP(hipSetDevice(c->device));
    hipDeviceProp_t prop;
    SQE_HIP(hipGetDeviceProperties(&prop, c->device));
    c->cu_count = prop.multiProcessorCount;
    c->hbm_bytes = (int64_t)prop.totalGlobalMem;
    c->name = prop.name[0] ? prop.name : prop.gcnArchName;
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(SQE_ERR_UNSUPPORTED, std::string("libsqe is built for gfx950 only, device is ") + prop.gcnArchName);
    SQE_HIP(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream.store(c->own_stream);
    SQE_TRY(c->host.init());
    SQE_TRY(c->unc_last.ensure(16));
    SQE_HIP(hipMemsetAsync(c->unc_last.p, 0, 16, c->own_stream));
    SQE_TRY(c->i8_last.ensure(32));
    SQE_HIP(hipMemsetAsync(c->i8_last.p, 0, 32, c->own_stream));
    return SQE_OK;
}

int sqe_create_sharded(const int* device_ids, int n_shards, int exchange, sqe_ctx** out) {
    if (!out) return fail(SQE_ERR_INVALID, "sqe_create: out is null");
    *out = nullptr;
    if (n_shards < 1 || n_shards > 64 || !device_ids) return fail(SQE_ERR_INVALID, "sqe_create: need 1 <= n_dev <= 64 device ids");
    if (exchange < SQE_EXCHANGE_AUTO || exchange > SQE_EXCHANGE_COPY) return fail(SQE_ERR_INVALID, "sqe_create_sharded: unknown exchange mode");
    std::unique_ptr<sqe_ctx> c(new (std::nothrow) sqe_ctx);
    if (!c) return fail(SQE_ERR_OOM, "sqe_create: host allocation failed");
    int rc = ctx_init_device(c.get(), device_ids[0]);
    if (rc == SQE_OK) rc = group_create(c.get(), device_ids, n_shards, exchange);
    if (rc != SQE_OK) { sqe_destroy(c.release()); return rc; }
    *out = c.release();
    return SQE_OK;
}

int sqe_create(const int* device_ids, int n_dev, sqe_ctx** out) {
    if (!out) return fail(SQE_ERR_INVALID, "sqe_create: out is null");
    *out = nullptr;
    if (n_dev < 1 || !device_ids) return fail(SQE_ERR_INVALID, "sqe_create: need at least one device id");
    if (n_dev > 1) return sqe_create_sharded(device_ids, n_dev, SQE_EXCHANGE_AUTO, out);
    std::unique_ptr<sqe_ctx> c(new (std::nothrow) sqe_ctx);
    if (!c) return fail(SQE_ERR_OOM, "sqe_create: host allocation failed");
    int rc = ctx_init_device(c.get(), device_ids[0]);
    if (rc != SQE_OK) { sqe_destroy(c.release()); return rc; }
    *out = c.release();
    return SQE_OK;
}

void sqe_destroy(sqe_ctx* ctx) {
    if (!ctx) return;
    if (ctx->group) group_destroy(ctx);
    (void)hipSetDevice(ctx->device);
    // Wait for everything on the device rather than for ctx->stream: an installed caller-owned stream
    // (sqe_set_stream) may already be gone when the context is torn down.
    (void)hipDeviceSynchronize();
    ctx->prof.drain();
    ctx->host.destroy();
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int sqe_synchronize(sqe_ctx* ctx) {
    if (!ctx) return fail(SQE_ERR_INVALID, "null handle");
    SQE_HIP(hipSetDevice(ctx->device));
    SQE_HIP(hipStreamSynchronize(ctx->stream.load()));
    return SQE_OK;
}

void* sqe_stream(sqe_ctx* ctx) { return ctx ? (void*)ctx->stream.load() : nullptr; }

int sqe_set_stream(sqe_ctx* ctx, void* hip_stream) {
    if (!ctx) return fail(SQE_ERR_INVALID, "null handle");
    std::lock_guard<std::mutex> lk(ctx->mu);
    SQE_HIP(hipSetDevice(ctx->device));
    ctx->prof.drain();
    // the OLD stream is only synchronised when it is ours: a caller-owned one may be dead already; work
    // still queued there is ordered by the per-object events (OpScope) in any case
    if (!ctx->foreign.load()) SQE_HIP(hipStreamSynchronize(ctx->own_stream));
    ctx->stream.store(hip_stream ? (hipStream_t)hip_stream : ctx->own_stream);
    ctx->foreign.store(hip_stream != nullptr);
    return SQE_OK;
}

int sqe_device_info(sqe_ctx* ctx, char* name, int name_cap, int* cu_count, int64_t* hbm_bytes) {
    if (!ctx) return fail(SQE_ERR_INVALID, "null handle");
    if (name && name_cap > 0) {
        strncpy(name, ctx->name.c_str(), (size_t)name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (cu_count) *cu_count = ctx->cu_count;
    if (hbm_bytes) *hbm_bytes = ctx->hbm_bytes;
    return SQE_OK;
}

int sqe_group_info(sqe_ctx* ctx, int* n_shards, int* exchange, int* device_ids, int cap) {
    if (!ctx) return fail(SQE_ERR_INVALID, "null handle");
    if (!ctx->group) {
        if (n_shards) *n_shards = 1;
        if (exchange) *exchange = SQE_EXCHANGE_COPY;
        if (device_ids && cap > 0) device_ids[0] = ctx->device;
        return SQE_OK;
    }
    return group_describe(ctx, n_shards, exchange, device_ids, cap);
}

// ================================================================ index
int sqe_index_create(sqe_ctx* ctx, int dim, int kind, int nlist, sqe_index** out) {
    if (!ctx) return fail(SQE_ERR_INVALID, "null handle");
    if (!out) return fail(SQE_ERR_INVALID, "sqe_index_create: out is null");
    if (ctx->group) return group_index_create(ctx, dim, kind, nlist, out);
    return index_create_impl(ctx, dim, kind, nlist, false, out);
}

void sqe_index_destroy(sqe_index* idx) {
    if (!idx) return;
    if (idx->group) { group_index_destroy(idx); return; }
    (void)hipSetDevice(idx->ctx->device);
    {
        std::lock_guard<std::mutex> lk(idx->ord.mu);
        idx->ord.quiesce();                       // the last operation on this index, on whatever stream it ran
    }
    if (idx->ivf) { ivf_destroy(idx->ivf); idx->ivf = nullptr; }
    if (idx->filter) { filter_destroy(idx->filter); idx->filter = nullptr; }
    if (idx->filter_each) { filter_each_destroy(idx->filter_each); idx->filter_each = nullptr; }
    if (idx->range) { range_destroy(idx->range); idx->range = nullptr; }
    if (idx->collapse) { collapse_destroy(idx->collapse); idx->collapse = nullptr; }
    if (idx->exclude) { exclude_destroy(idx->exclude); idx->exclude = nullptr; }
    if (idx->mmr) { mmr_destroy(idx->mmr); idx->mmr = nullptr; }
    if (idx->fuse) { fuse_destroy(idx->fuse); idx->fuse = nullptr; }
    if (idx->fields) { fields_destroy(idx->fields); idx->fields = nullptr; }
    if (idx->agg) { aggregate_destroy(idx->agg); idx->agg = nullptr; }
    if (idx->sort) { sort_destroy(idx->sort); idx->sort = nullptr; }
    if (idx->where_mask) { where_mask_destroy(idx->where_mask); idx->where_mask = nullptr; }
    if (idx->master) (void)hipFree(idx->master);
    if (idx->scan) (void)hipFree(idx->scan);
    idx->ord.destroy();
    delete idx;                                   // DevBufs release in the destructor
}

int sqe_index_reserve(sqe_index* idx, int64_t rows) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (rows < 0) return fail(SQE_ERR_INVALID, "sqe_index_reserve: rows < 0");
    if (idx->group) return group_index_reserve(idx, rows);
    OpScope op(idx->ctx, idx->ord, true);
    return index_grow(idx, rows, op.s);
}

int sqe_index_add_device(sqe_index* idx, const float* x_dev, int64_t n) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (n < 0 || (n > 0 && !x_dev)) return fail(SQE_ERR_INVALID, "sqe_index_add: bad arguments");
    if (n == 0) return SQE_OK;
    if (idx->group) return group_index_add(idx, x_dev, n, true, false);
    OpScope op(idx->ctx, idx->ord, false);
    return index_add_impl(idx, x_dev, n, idx->dim, false, op.s);
}

int sqe_index_add(sqe_index* idx, const float* x_host, int64_t n) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (n < 0 || (n > 0 && !x_host)) return fail(SQE_ERR_INVALID, "sqe_index_add: bad arguments");
    if (n == 0) return SQE_OK;
    if (idx->group) return group_index_add(idx, x_host, n, false, false);
    OpScope op(idx->ctx, idx->ord, true);
    SQE_TRY(index_grow(idx, idx->n.load() + n, op.s));
    const int64_t rows_per_step = std::max<int64_t>(1, (64ll << 20) / ((int64_t)idx->dim * 4));
    SQE_TRY(idx->stage_in.ensure((size_t)std::min(rows_per_step, n) * idx->dim * 4));
    for (int64_t off = 0; off < n; off += rows_per_step) {
        const int64_t m = std::min(rows_per_step, n - off);
        SQE_HIP(hipMemcpyAsync(idx->stage_in.p, x_host + (size_t)off * idx->dim, (size_t)m * idx->dim * 4,
                               hipMemcpyHostToDevice, op.s));
        SQE_TRY(index_add_impl(idx, idx->stage_in.as<float>(), m, idx->dim, false, op.s));
    }
    SQE_HIP(hipStreamSynchronize(op.s));   // x_host is not retained past return
    return SQE_OK;
}

int sqe_index_update(sqe_index* idx, const int64_t* rows_host, const float* x_host, int64_t n) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (n < 0 || (n > 0 && (!rows_host || !x_host))) return fail(SQE_ERR_INVALID, "sqe_index_update: bad arguments");
    if (n == 0) return SQE_OK;
    if (idx->group) return group_index_update(idx, rows_host, x_host, n);
    OpScope op(idx->ctx, idx->ord, true);
    std::vector<int64_t> pos;                 // ids -> positions (the same numbers until the first delete)
    SQE_TRY(index_resolve_ids(idx, rows_host, n, pos, op.s, "sqe_index_update"));
    const size_t xb = (size_t)n * idx->dim * 4, rb = (size_t)n * 8;
    SQE_TRY(idx->stage_in.ensure(xb + rb));
    SQE_HIP(hipMemcpyAsync(idx->stage_in.p, x_host, xb, hipMemcpyHostToDevice, op.s));
    SQE_HIP(hipMemcpyAsync((char*)idx->stage_in.p + xb, pos.data(), rb, hipMemcpyHostToDevice, op.s));
    SQE_TRY(index_update_impl(idx, (const int64_t*)((char*)idx->stage_in.p + xb), idx->stage_in.as<float>(), n, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_count(const sqe_index* idx, int64_t* out) {
    if (!idx || !out) return fail(SQE_ERR_INVALID, "sqe_index_count: null argument");
    if (idx->group) return group_index_count(idx, out);
    *out = idx->n.load();
    return SQE_OK;
}

int sqe_index_get_rows(sqe_index* idx, const int64_t* rows_host, int64_t n, float* out_host) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (n < 0 || (n > 0 && (!rows_host || !out_host))) return fail(SQE_ERR_INVALID, "sqe_index_get_rows: bad arguments");
    if (idx->group) return group_index_get_rows(idx, rows_host, n, out_host);
    OpScope op(idx->ctx, idx->ord, true);
    std::vector<int64_t> pos;
    SQE_TRY(index_resolve_ids(idx, rows_host, n, pos, op.s, "sqe_index_get_rows"));
    for (int64_t i = 0; i < n;) {                          // one copy per run of consecutive positions
        int64_t j = i + 1;
        while (j < n && pos[(size_t)j] == pos[(size_t)j - 1] + 1) ++j;
        SQE_HIP(hipMemcpyAsync(out_host + (size_t)i * idx->dim, idx->master + (size_t)pos[(size_t)i] * idx->dim,
                               (size_t)(j - i) * idx->dim * 4, hipMemcpyDeviceToHost, op.s));
        i = j;
    }
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_set_option(sqe_index* idx, const char* key, double value) {
    if (!idx || !key) return fail(SQE_ERR_INVALID, "sqe_index_set_option: null argument");
    if (idx->group) return group_index_set_option(idx, key, value);
    std::lock_guard<std::mutex> lk(idx->ord.mu);
    const std::string k(key);
    if (k == "scan_mode") {
        if ((int)value != SQE_SCAN_BF16_RESCORE && (int)value != SQE_SCAN_INT8_RESCORE) return fail(SQE_ERR_INVALID, "scan_mode: unknown mode");
        if ((int)value == SQE_SCAN_INT8_RESCORE && idx->kind != SQE_INDEX_FLAT)
            return fail(SQE_ERR_INVALID, "scan_mode: the int8 first pass is for FLAT indexes");
        idx->scan_mode = (int)value;
    } else if (k == "i8_min_rows") {
        if (value < 0) return fail(SQE_ERR_INVALID, "i8_min_rows must be >= 0");
        idx->i8_min_rows = (int64_t)value;
    } else if (k == "i8_sample_step") {
        if (value < 1 || value > 4096) return fail(SQE_ERR_INVALID, "i8_sample_step must be in [1, 4096]");
        idx->i8_sample_step = (int)value;
    } else if (k == "i8_sample_int8") {
        idx->i8_sample_int8 = value != 0 ? 1 : 0;
    } else if (k == "i8_max_resid") {
        if (!(value > 0)) return fail(SQE_ERR_INVALID, "i8_max_resid must be > 0");
        idx->i8_max_resid = value;
    } else if (k == "i8_anchor_margin") {
        if (!(value >= 0) || value > 4) return fail(SQE_ERR_INVALID, "i8_anchor_margin must be in [0, 4]");
        idx->i8_anchor_margin = value;
    } else if (k == "i8_key_budget") {
        if (value < 0 || value > 1e9) return fail(SQE_ERR_INVALID, "i8_key_budget must be >= 0");
        idx->i8_key_budget = (int)value;
    } else if (k == "i8_keep_select") {
        idx->i8_keep_select = value != 0 ? 1 : 0;
    } else if (k == "i8_sample_m") {
        if (value < 1 || value > 64) return fail(SQE_ERR_INVALID, "i8_sample_m must be in [1, 64]");
        idx->i8_sample_m = (int)value;
    } else if (k == "rescore_k") {
        if (value < 0 || value > MAX_KP) return fail(SQE_ERR_INVALID, "rescore_k must be in [0, 256]");
        idx->rescore_k = (int)value;
    } else if (k == "nprobe") {
        idx->nprobe = (int)value;
    } else if (k == "certify") {
        idx->certify = value != 0.0;
    } else if (k == "id_base") {
        if (value < 0) return fail(SQE_ERR_INVALID, "id_base must be >= 0");
        idx->id_base = (int64_t)value;
    } else if (k == "filter_gather_rows") {
        if (value < 256 || value > 1e10) return fail(SQE_ERR_INVALID, "filter_gather_rows must be in [256, 1e10]");
        idx->filter_gather_rows = (int64_t)value;
    } else if (k == "filter_each_direct_rows") {
        if (value < 0 || value > (double)(1 << 30)) return fail(SQE_ERR_INVALID, "filter_each_direct_rows must be in [0, 2^30]");
        idx->filter_each_direct_rows = (int64_t)value;
    } else if (k == "filter_each_direct_queries") {
        if (value < 0 || value > (double)(1 << 30)) return fail(SQE_ERR_INVALID, "filter_each_direct_queries must be in [0, 2^30]");
        idx->filter_each_direct_queries = (int)value;
    } else if (k == "filter_each_key_budget") {
        if (value < (double)FILTER_EACH_MIN_KEY_BUDGET || value > 1e12) return fail(SQE_ERR_INVALID, "filter_each_key_budget must be in [4096, 1e12]");
        idx->filter_each_key_budget = (int64_t)value;
    } else if (k == "range_key_budget") {
        if (value < 4096 || value > 1e12) return fail(SQE_ERR_INVALID, "range_key_budget must be in [4096, 1e12]");
        idx->range_key_budget = (int64_t)value;
    } else if (k == "collapse_depth") {
        if (value < 0 || value > MAX_KP) return fail(SQE_ERR_INVALID, "collapse_depth must be in [0, 256]");
        idx->collapse_depth = (int)value;
    } else if (k == "exclude_depth") {
        if (value < 0 || value > MAX_KP) return fail(SQE_ERR_INVALID, "exclude_depth must be in [0, 256]");
        idx->exclude_depth = (int)value;
    } else if (k == "mmr_row_budget") {
        if (value < MMR_MAX_N || value > 1e9) return fail(SQE_ERR_INVALID, "mmr_row_budget must be in [256, 1e9]");
        idx->mmr_row_budget = (int64_t)value;
    } else if (k == "sort_fan_in") {
        if (value < 2 || value > SORT_MAX_FAN_IN) return fail(SQE_ERR_INVALID, "sort_fan_in must be in [2, 64]");
        idx->sort_fan_in = (int)value;
    } else if (k == "where_route") {
        if (value != 0 && value != 1 && value != 2) return fail(SQE_ERR_INVALID, "where_route must be 0 (auto), 1 (gather) or 2 (mask)");
        idx->where_route = (int)value;
    } else if (k == "where_mask_depth") {
        if (value < 0 || value > MAX_KP) return fail(SQE_ERR_INVALID, "where_mask_depth must be in [0, 256]");
        idx->where_mask_depth = (int)value;
    } else if (k == "within_route") {
        if (value != 0 && value != 2) return fail(SQE_ERR_INVALID, "within_route must be 0 (gather where the row set fits) or 2 (mask)");
        idx->within_route = (int)value;
    } else if (k == "where_mask_min_rows") {
        if (value < 0 || value > 1e12) return fail(SQE_ERR_INVALID, "where_mask_min_rows must be in [0, 1e12]");
        idx->where_mask_min_rows = (int64_t)value;
    } else {
        return fail(SQE_ERR_INVALID, "unknown option: " + k);
    }
    return SQE_OK;
}

// ---------------------------------------------------------------- search (the pipeline: search.hip)
static int search_args_ok(sqe_index* idx, const void* q, int B, int k, const void* cos, const void* ids) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (B < 0 || k < 1 || k > MAX_KP) return fail(SQE_ERR_INVALID, "sqe_index_search: need B >= 0 and 1 <= k <= 256");
    if (B > 0 && (!q || !cos || !ids)) return fail(SQE_ERR_INVALID, "sqe_index_search: null buffer");
    return SQE_OK;
}

int sqe_index_i8_last(sqe_index* idx, sqe_i8_launch_t* out) {
    if (!idx || !out) return fail(SQE_ERR_INVALID, "sqe_index_i8_last: null argument");
    if (idx->group || idx->ivf) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_i8_last: single-device FLAT indexes only");
    OpScope op(idx->ctx, idx->ord, true);
    if (idx->i8_launch.rows == 0) return fail(SQE_ERR_STATE, "sqe_index_i8_last: this index has not answered a search with the int8 first pass");
    int unc = 0;
    SQE_HIP(hipMemcpyAsync(&unc, idx->unc.p, 4, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    *out = idx->i8_launch;
    out->uncertified = unc;
    return SQE_OK;
}

int sqe_index_i8_read(sqe_index* idx, int what, int64_t offset, void* out_host, int64_t bytes) {
    if (!idx || (!out_host && bytes > 0)) return fail(SQE_ERR_INVALID, "sqe_index_i8_read: null argument");
    if (idx->group || idx->ivf) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_i8_read: single-device FLAT indexes only");
    OpScope op(idx->ctx, idx->ord, true);
    const sqe_i8_launch_t& L = idx->i8_launch;
    // the copy of the rows outlives the launch that read it: readable whenever it exists (an index that answers in bf16 because
    // its rows quantise badly has one too)
    const bool copy_only = what == SQE_I8_ROWS || what == SQE_I8_ROW_SCALES;
    if (L.rows == 0 && !(copy_only && idx->i8db.p && idx->i8_rows > 0))
        return fail(SQE_ERR_STATE, copy_only ? "sqe_index_i8_read: this index has no int8 copy of its rows"
                                             : "sqe_index_i8_read: this index has not answered a search with the int8 first pass");
    const int64_t tiles = L.rows ? (L.rows + L.tile_rows - 1) / L.tile_rows : (idx->i8_rows + SCAN_BM - 1) / SCAN_BM;
    const void* src = nullptr;
    int64_t size = 0;
    switch (what) {
        case SQE_I8_ROWS: src = idx->i8db.p; size = tiles * idx->i8_tile_stride; break;
        case SQE_I8_ROW_SCALES: src = idx->i8sxi.p; size = tiles * SCAN_BM * 4; break;
        case SQE_I8_QUERIES: src = idx->q8.p; size = (int64_t)L.b_pad * L.q_pitch; break;
        case SQE_I8_QUERIES_TILED: src = idx->q8t.p; size = ((int64_t)L.b_pad + 255) / 256 * 256 * L.dim; break;
        case SQE_I8_THRESHOLDS: src = idx->i8thr_int.p; size = (int64_t)L.b_pad * 4; break;
        case SQE_I8_LIST_COUNTS: src = idx->cand_cnt.p; size = (int64_t)L.n_chunks * L.b_pad * 4; break;
        case SQE_I8_LISTS: src = idx->cand.p; size = (int64_t)L.n_chunks * L.b_pad * L.list_cap * 8; break;
        case SQE_I8_POOL_COUNTS: src = idx->i8ovf_cnt.p; size = (int64_t)L.b_pad * 4; break;
        case SQE_I8_POOLS: src = idx->i8ovf.p; size = (int64_t)L.b_pad * L.pool_cap * 8; break;
        case SQE_I8_SAMPLE_BEST:
            if (!L.sample_int8) return fail(SQE_ERR_STATE, "sqe_index_i8_read: the threshold pass of the last search did not run in int8");
            src = idx->i8samp.p; size = (int64_t)L.sample_chunks * L.sample_b_pad * 16 * 8; break;
        case SQE_I8_THR_EFF: src = idx->i8thr_eff.p; size = (int64_t)L.b_pad * 4; break;
        case SQE_I8_SAMPLE_COS: src = idx->i8cos_s.p; size = (int64_t)L.B * L.sample_m * 4; break;
        case SQE_I8_SAMPLE_IDS: src = idx->i8ids_s.p; size = (int64_t)L.B * L.sample_m * 8; break;
        case SQE_I8_SELECT_COS: case SQE_I8_SELECT_IDS: case SQE_I8_SELECT_THR: case SQE_I8_SELECT_TRACE:
            if (!idx->i8_kept) return fail(SQE_ERR_STATE, "sqe_index_i8_read: the last int8 search ran without i8_keep_select");
            if (what == SQE_I8_SELECT_COS) { src = idx->i8keep_cos.p; size = (int64_t)L.B * L.k * 4; }
            else if (what == SQE_I8_SELECT_IDS) { src = idx->i8keep_ids.p; size = (int64_t)L.B * L.k * 8; }
            else if (what == SQE_I8_SELECT_THR) { src = idx->i8keep_thr.p; size = (int64_t)L.b_pad * 4; }
            else { src = idx->i8keep_trace.p; size = (int64_t)L.B * 4 * 4; }
            break;
        default: return fail(SQE_ERR_INVALID, "sqe_index_i8_read: unknown buffer");
    }
    if (offset < 0 || bytes < 0 || offset + bytes > size) return fail(SQE_ERR_INVALID, "sqe_index_i8_read: range outside the buffer");
    if (bytes == 0) return SQE_OK;
    SQE_HIP(hipMemcpyAsync(out_host, static_cast<const char*>(src) + offset, (size_t)bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_scan_last(sqe_index* idx, sqe_scan_launch_t* out) {
    if (!idx || !out) return fail(SQE_ERR_INVALID, "sqe_index_scan_last: null argument");
    if (idx->group || idx->ivf) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_scan_last: single-device FLAT indexes only");
    OpScope op(idx->ctx, idx->ord, true);
    if (idx->scan_launch.rows == 0) return fail(SQE_ERR_STATE, "sqe_index_scan_last: the last search of this index was not answered by the bf16 first pass");
    int unc = 0;
    if (idx->scan_launch.certified) {
        SQE_HIP(hipMemcpyAsync(&unc, idx->unc.p, 4, hipMemcpyDeviceToHost, op.s));
        SQE_HIP(hipStreamSynchronize(op.s));
    }
    *out = idx->scan_launch;
    out->uncertified = unc;
    return SQE_OK;
}

int sqe_index_scan_read(sqe_index* idx, int what, int64_t offset, void* out_host, int64_t bytes) {
    if (!idx || (!out_host && bytes > 0)) return fail(SQE_ERR_INVALID, "sqe_index_scan_read: null argument");
    if (idx->group || idx->ivf) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_scan_read: single-device FLAT indexes only");
    OpScope op(idx->ctx, idx->ord, true);
    const sqe_scan_launch_t& L = idx->scan_launch;
    if (L.rows == 0) return fail(SQE_ERR_STATE, "sqe_index_scan_read: the last search of this index was not answered by the bf16 first pass");
    if (what >= SQE_SCAN_COLLECT_THR && what <= SQE_SCAN_COLLECT_KEYS && !L.certified)
        return fail(SQE_ERR_STATE, "sqe_index_scan_read: the last search ran without the certificate");
    int unc = 0;
    if (what == SQE_SCAN_UNC_IDS || what == SQE_SCAN_COLLECT_KEYS) {      // their extent is the uncertified count
        SQE_HIP(hipMemcpyAsync(&unc, idx->unc.p, 4, hipMemcpyDeviceToHost, op.s));
        SQE_HIP(hipStreamSynchronize(op.s));
        if (unc < 0 || unc > L.B) return fail(SQE_ERR_STATE, "sqe_index_scan_read: uncertified count out of range");
    }
    const void* src = nullptr;
    int64_t size = 0;
    switch (what) {
        case SQE_SCAN_LISTS: src = idx->cand.p; size = (int64_t)L.n_chunks * L.b_pad * L.list_cap * 8; break;
        case SQE_SCAN_LIST_COUNTS: src = idx->cand_cnt.p; size = (int64_t)L.n_chunks * L.b_pad * 4; break;
        case SQE_SCAN_BOUNDS: src = idx->gmax.p; size = (int64_t)L.b_pad * L.ngroups * GMAX_COLS * 4; break;
        case SQE_SCAN_COLLECT_THR: src = idx->unc.as<char>() + 16; size = (int64_t)L.b_pad * 4; break;
        case SQE_SCAN_UNC_COUNT: src = idx->unc.p; size = 4; break;
        case SQE_SCAN_UNC_IDS: src = idx->unc_ids.p; size = (int64_t)unc * 4; break;
        case SQE_SCAN_COLLECT_COUNTS: src = idx->fb_cnt.p; size = (int64_t)L.B * 4; break;
        case SQE_SCAN_COLLECT_KEYS: src = idx->fb_keys.p; size = (int64_t)unc * L.exact_cap * 8; break;
        default: return fail(SQE_ERR_INVALID, "sqe_index_scan_read: unknown buffer");
    }
    if (offset < 0 || bytes < 0 || offset + bytes > size) return fail(SQE_ERR_INVALID, "sqe_index_scan_read: range outside the buffer");
    if (bytes == 0) return SQE_OK;
    SQE_HIP(hipMemcpyAsync(out_host, static_cast<const char*>(src) + offset, (size_t)bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_state(sqe_index* idx, sqe_index_state_t* out) {
    if (!idx || !out) return fail(SQE_ERR_INVALID, "sqe_index_state: null argument");
    if (idx->group || idx->ivf) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_state: single-device FLAT indexes only");
    OpScope op(idx->ctx, idx->ord, true);
    out->rows = idx->n.load();
    out->i8_rows = idx->i8db.p ? idx->i8_rows : 0;
    out->i8_tile_stride = idx->i8db.p ? idx->i8_tile_stride : 0;
    out->dim = idx->dim;
    out->scan_pitch = idx->pitch;
    out->last_B = idx->last_B;
    out->last_i8 = idx->last_i8 ? 1 : 0;
    return SQE_OK;
}

int sqe_index_state_read(sqe_index* idx, int what, int64_t offset, void* out_host, int64_t bytes) {
    if (!idx || (!out_host && bytes > 0)) return fail(SQE_ERR_INVALID, "sqe_index_state_read: null argument");
    if (idx->group || idx->ivf) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_state_read: single-device FLAT indexes only");
    OpScope op(idx->ctx, idx->ord, true);
    const void* src = nullptr;
    int64_t size = 0;
    const int64_t B = idx->last_B;
    switch (what) {
        case SQE_STATE_SCAN_BF16: src = idx->scan; size = round_up(idx->n.load(), SCAN_BM) * idx->pitch; break;
        case SQE_STATE_RESID_MAX: src = idx->resid_max.p; size = 4; break;
        case SQE_STATE_I8_RESID_MAX: src = idx->i8resid_max.p; size = 4; break;
        case SQE_STATE_QN: src = idx->qn.p; size = B * idx->dim * 4; break;
        case SQE_STATE_Q_RESID: src = idx->q_resid.p; size = B * 4; break;
        case SQE_STATE_Q8_RESID: src = idx->last_i8 ? idx->q8resid.p : nullptr; size = B * 4; break;
        case SQE_STATE_Q8_SCALES: src = idx->last_i8 ? idx->q8sqi.p : nullptr; size = B * 4; break;
        default: return fail(SQE_ERR_INVALID, "sqe_index_state_read: unknown buffer");
    }
    if (!src || size == 0) return fail(SQE_ERR_STATE, "sqe_index_state_read: the index does not hold that buffer yet");
    if (offset < 0 || bytes < 0 || offset + bytes > size) return fail(SQE_ERR_INVALID, "sqe_index_state_read: range outside the buffer");
    if (bytes == 0) return SQE_OK;
    SQE_HIP(hipMemcpyAsync(out_host, static_cast<const char*>(src) + offset, (size_t)bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_ivf_state(sqe_index* idx, sqe_ivf_state_t* out) {
    if (!idx || !out) return fail(SQE_ERR_INVALID, "sqe_index_ivf_state: null argument");
    if (idx->group || !idx->ivf) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_ivf_state: single-device IVF indexes only");
    OpScope op(idx->ctx, idx->ord, true);
    return ivf_state(idx, idx->ivf, out, op.s);
}

int sqe_index_ivf_state_read(sqe_index* idx, int what, int64_t offset, void* out_host, int64_t bytes) {
    if (!idx || (!out_host && bytes > 0)) return fail(SQE_ERR_INVALID, "sqe_index_ivf_state_read: null argument");
    if (idx->group || !idx->ivf) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_ivf_state_read: single-device IVF indexes only");
    OpScope op(idx->ctx, idx->ord, true);
    return ivf_state_read(idx, idx->ivf, what, offset, out_host, bytes, op.s);
}

int sqe_index_search_device(sqe_index* idx, const float* q_dev, int B, int k, int nprobe,
                            float* cos_out_dev, int64_t* id_out_dev) {
    SQE_TRY(search_args_ok(idx, q_dev, B, k, cos_out_dev, id_out_dev));
    if (B == 0) return SQE_OK;
    if (idx->group) return group_index_search(idx, q_dev, B, k, nprobe, cos_out_dev, id_out_dev, true);
    OpScope op(idx->ctx, idx->ord, false);
    return index_search_impl(idx, q_dev, B, k, nprobe, cos_out_dev, id_out_dev, op.s);
}

int sqe_index_search(sqe_index* idx, const float* q_host, int B, int k, int nprobe,
                     float* cos_out_host, int64_t* id_out_host) {
    SQE_TRY(search_args_ok(idx, q_host, B, k, cos_out_host, id_out_host));
    if (B == 0) return SQE_OK;
    if (idx->group) return group_index_search(idx, q_host, B, k, nprobe, cos_out_host, id_out_host, false);
    OpScope op(idx->ctx, idx->ord, true);
    const size_t qbytes = (size_t)B * idx->dim * 4, cb = (size_t)B * k * 4, ib = (size_t)B * k * 8;
    SQE_TRY(idx->stage_in.ensure(qbytes));
    SQE_TRY(idx->stage_out.ensure(round_up((int64_t)cb, 16) + ib));
    float* cos_dev = idx->stage_out.as<float>();
    int64_t* id_dev = reinterpret_cast<int64_t*>(idx->stage_out.as<char>() + round_up((int64_t)cb, 16));
    SQE_HIP(hipMemcpyAsync(idx->stage_in.p, q_host, qbytes, hipMemcpyHostToDevice, op.s));
    SQE_TRY(index_search_impl(idx, idx->stage_in.as<float>(), B, k, nprobe, cos_dev, id_dev, op.s));
    SQE_HIP(hipMemcpyAsync(cos_out_host, cos_dev, cb, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(id_out_host, id_dev, ib, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_train_device(sqe_index* idx, const float* x_dev, int64_t n, int iters, uint64_t seed) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (idx->group) {
        if (!x_dev || n <= 0) return fail(SQE_ERR_INVALID, "sqe_index_train: empty training set");
        return group_index_train(idx, x_dev, n, iters, seed, true);
    }
    if (!idx->ivf) return fail(SQE_ERR_STATE, "sqe_index_train: not an IVF index");
    if (!x_dev || n <= 0) return fail(SQE_ERR_INVALID, "sqe_index_train: empty training set");
    OpScope op(idx->ctx, idx->ord, false);
    return ivf_train(idx, idx->ivf, x_dev, n, iters, seed, op.s);
}

int sqe_index_train(sqe_index* idx, const float* x_host, int64_t n, int iters, uint64_t seed) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (idx->group) {
        if (!x_host || n <= 0) return fail(SQE_ERR_INVALID, "sqe_index_train: empty training set");
        return group_index_train(idx, x_host, n, iters, seed, false);
    }
    if (!idx->ivf) return fail(SQE_ERR_STATE, "sqe_index_train: not an IVF index");
    if (!x_host || n <= 0) return fail(SQE_ERR_INVALID, "sqe_index_train: empty training set");
    OpScope op(idx->ctx, idx->ord, true);
    DevBuf tmp;
    SQE_TRY(tmp.ensure((size_t)n * idx->dim * 4));
    SQE_HIP(hipMemcpyAsync(tmp.p, x_host, (size_t)n * idx->dim * 4, hipMemcpyHostToDevice, op.s));
    SQE_TRY(ivf_train(idx, idx->ivf, tmp.as<float>(), n, iters, seed, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_ivf_export(sqe_index* idx, float* centroids_host, int32_t* assign_host) {
    if (!idx) return fail(SQE_ERR_INVALID, "null index");
    if (idx->group) {
        if (!group_index_ivf_trained(idx)) return fail(SQE_ERR_STATE, "sqe_index_ivf_export: not a trained IVF index");
        return group_index_ivf_export(idx, centroids_host, assign_host);
    }
    if (!idx->ivf) return fail(SQE_ERR_STATE, "sqe_index_ivf_export: not an IVF index");
    OpScope op(idx->ctx, idx->ord, true);
    return ivf_export(idx, idx->ivf, centroids_host, assign_host, op.s);
}

// ---------------------------------------------------------------- persistence
// File: 64-byte header | master rows [n, dim] fp32 | (IVF, trained) centroids [nlist, dim] fp32 | assign [n] int32
//       | (version 2 only) next_id int64 | live ids [n] int64.
// Version 1 is an index whose ids are 0 .. n-1 (no row was ever deleted): byte for byte the file of before deletes existed.
// Version 2 is written when rows were deleted; rows and assignments are then in ascending id order, and a reader that only
// knows version 1 refuses the file rather than renumbering its rows.
// The bf16 scan copy, residuals and IVF lists are derived data and are rebuilt on load.  Rows are in GLOBAL row
// order whatever the number of devices the index was spread over, so a file written by an 8-device context
// loads on one device and the other way round.
namespace {
struct SaveHeader {
    char magic[8];          // "SQEIDX01"
    uint32_t version, dim, kind, nlist;
    int64_t n, id_base;
    uint32_t flags;         // bit 0: IVF centroids + assignments follow
    uint32_t certify;
    uint8_t pad[16];
};
static_assert(sizeof(SaveHeader) == 64, "header layout");
constexpr size_t IO_CHUNK = 64u << 20;

struct PinnedBuf {
    void* p = nullptr;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    int alloc(size_t bytes) {
        hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) return fail(SQE_ERR_OOM, std::string("pinned staging: ") + hipGetErrorString(e));
        return SQE_OK;
    }
};
struct FileCloser {
    FILE* f;
    ~FileCloser() { if (f) fclose(f); }
};

int write_device_range(FILE* f, const void* dev, size_t bytes, void* pinned, hipStream_t s) {
    for (size_t off = 0; off < bytes; off += IO_CHUNK) {
        const size_t m = std::min(IO_CHUNK, bytes - off);
        SQE_HIP(hipMemcpyAsync(pinned, (const char*)dev + off, m, hipMemcpyDeviceToHost, s));
        SQE_HIP(hipStreamSynchronize(s));
        if (fwrite(pinned, 1, m, f) != m) return fail(SQE_ERR_IO, "sqe_index_save: short write");
    }
    return SQE_OK;
}
}  // namespace

int sqe_index_save(sqe_index* idx, const char* path) {
    if (!idx || !path) return fail(SQE_ERR_INVALID, "sqe_index_save: null argument");
    FileCloser fc{fopen(path, "wb")};
    if (!fc.f) return fail(SQE_ERR_IO, std::string("sqe_index_save: cannot open ") + path);
    PinnedBuf pin;
    SQE_TRY(pin.alloc(IO_CHUNK));
    SaveHeader h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, "SQEIDX01", 8);
    h.version = 1; h.dim = (uint32_t)idx->dim; h.kind = (uint32_t)idx->kind; h.nlist = (uint32_t)idx->nlist;
    // the footer of a file with holes: next_id, then the live ids
    auto write_ids = [&](const std::vector<int64_t>& ids) -> int {
        const int64_t next = idx->next_id.load();
        if (fwrite(&next, 8, 1, fc.f) != 1) return fail(SQE_ERR_IO, "sqe_index_save: short write");
        if (!ids.empty() && fwrite(ids.data(), 8, ids.size(), fc.f) != ids.size()) return fail(SQE_ERR_IO, "sqe_index_save: short write");
        return SQE_OK;
    };
    if (idx->group) {
        SQE_TRY(group_index_count(idx, &h.n));
        const bool holes = idx->next_id.load() != h.n;
        if (holes) h.version = 2;
        const bool givf = group_index_ivf_trained(idx);
        h.id_base = idx->id_base; h.flags = givf ? 1u : 0u; h.certify = (uint32_t)idx->certify;
        if (fwrite(&h, 1, sizeof(h), fc.f) != sizeof(h)) return fail(SQE_ERR_IO, "sqe_index_save: short write");
        SQE_TRY(group_index_save_rows(idx, fc.f, pin.p, IO_CHUNK));
        if (givf) {
            // the same IVF section a single-device index writes: centroids, then the list of every row in global order
            std::vector<float> cent((size_t)idx->nlist * idx->dim);
            std::vector<int32_t> assign((size_t)std::max<int64_t>(h.n, 1));
            SQE_TRY(group_index_ivf_export(idx, cent.data(), assign.data()));
            if (fwrite(cent.data(), 4, cent.size(), fc.f) != cent.size()) return fail(SQE_ERR_IO, "sqe_index_save: short write");
            if (h.n > 0 && fwrite(assign.data(), 4, (size_t)h.n, fc.f) != (size_t)h.n)
                return fail(SQE_ERR_IO, "sqe_index_save: short write");
        }
        if (holes) {
            std::vector<int64_t> ids;
            SQE_TRY(group_index_ids_vec(idx, ids));
            SQE_TRY(write_ids(ids));
        }
        if (fflush(fc.f) != 0) return fail(SQE_ERR_IO, "sqe_index_save: flush failed");
        return SQE_OK;
    }
    OpScope op(idx->ctx, idx->ord, true);
    const bool ivf = idx->ivf && ivf_trained(idx->ivf);
    if (ivf) SQE_TRY(ivf_rows_added(idx, idx->ivf, op.s));
    const int64_t n = idx->n.load();
    const bool holes = idx->next_id.load() != n;
    if (holes) h.version = 2;
    h.n = n; h.id_base = idx->id_base; h.flags = ivf ? 1u : 0u; h.certify = (uint32_t)idx->certify;
    if (fwrite(&h, 1, sizeof(h), fc.f) != sizeof(h)) return fail(SQE_ERR_IO, "sqe_index_save: short write");
    SQE_HIP(hipStreamSynchronize(op.s));
    SQE_TRY(write_device_range(fc.f, idx->master, (size_t)n * idx->dim * 4, pin.p, op.s));
    if (ivf) {
        std::vector<float> cent((size_t)idx->nlist * idx->dim);
        std::vector<int32_t> assign((size_t)std::max<int64_t>(n, 1));
        SQE_TRY(ivf_export(idx, idx->ivf, cent.data(), assign.data(), op.s));
        if (fwrite(cent.data(), 4, cent.size(), fc.f) != cent.size()) return fail(SQE_ERR_IO, "sqe_index_save: short write");
        if (n > 0 && fwrite(assign.data(), 4, (size_t)n, fc.f) != (size_t)n)
            return fail(SQE_ERR_IO, "sqe_index_save: short write");
    }
    if (holes) {
        std::vector<int64_t> ids;
        SQE_TRY(index_ids_host(idx, ids, op.s));
        SQE_TRY(write_ids(ids));
    }
    if (fflush(fc.f) != 0) return fail(SQE_ERR_IO, "sqe_index_save: flush failed");
    return SQE_OK;
}

int sqe_index_load(sqe_ctx* ctx, const char* path, sqe_index** out) {
    if (!ctx || !path || !out) return fail(SQE_ERR_INVALID, "sqe_index_load: null argument");
    *out = nullptr;
    FileCloser fc{fopen(path, "rb")};
    if (!fc.f) return fail(SQE_ERR_IO, std::string("sqe_index_load: cannot open ") + path);
    SaveHeader h;
    if (fread(&h, 1, sizeof(h), fc.f) != sizeof(h) || memcmp(h.magic, "SQEIDX01", 8) != 0 || (h.version != 1 && h.version != 2))
        return fail(SQE_ERR_IO, "sqe_index_load: not a saved index (bad header)");
    if (h.n < 0 || h.dim == 0 || h.dim % 64 != 0) return fail(SQE_ERR_IO, "sqe_index_load: corrupt header");
    sqe_index* idx = nullptr;
    SQE_TRY(sqe_index_create(ctx, (int)h.dim, (int)h.kind, (int)h.nlist, &idx));
    struct Guard {
        sqe_index* i;
        ~Guard() { if (i) sqe_index_destroy(i); }
    } guard{idx};
    SQE_TRY(sqe_index_set_option(idx, "id_base", (double)h.id_base));
    SQE_TRY(sqe_index_set_option(idx, "certify", (double)h.certify));
    SQE_TRY(sqe_index_reserve(idx, h.n));
    PinnedBuf pin;
    SQE_TRY(pin.alloc(IO_CHUNK));
    const size_t row_bytes = (size_t)h.dim * 4;
    const int64_t rows_per_step = std::max<int64_t>(1, (int64_t)(IO_CHUNK / row_bytes));
    // version 2: next_id and the live ids behind the other sections
    int64_t next_id = h.n;
    std::vector<int64_t> ids;
    if (h.version == 2) {
        const long long footer = (long long)sizeof(h) + (long long)h.n * (long long)row_bytes +
                                 ((h.flags & 1u) ? (long long)h.nlist * (long long)row_bytes + (long long)h.n * 4 : 0);
        ids.resize((size_t)h.n);
        if (fseeko(fc.f, (off_t)footer, SEEK_SET) != 0 || fread(&next_id, 8, 1, fc.f) != 1 ||
            (h.n > 0 && fread(ids.data(), 8, (size_t)h.n, fc.f) != (size_t)h.n))
            return fail(SQE_ERR_IO, "sqe_index_load: file is truncated");
        if (next_id < h.n) return fail(SQE_ERR_IO, "sqe_index_load: corrupt id section");
        if (fseeko(fc.f, (off_t)sizeof(h), SEEK_SET) != 0) return fail(SQE_ERR_IO, "sqe_index_load: seek failed");
    }
    if (idx->group) {
        if (h.version == 2) {
            SQE_TRY(group_index_load_rows(idx, fc.f, h.n, ids.data(), next_id, pin.p, IO_CHUNK));
        } else {
            for (int64_t off = 0; off < h.n; off += rows_per_step) {
                const int64_t m = std::min(rows_per_step, h.n - off);
                if (fread(pin.p, row_bytes, (size_t)m, fc.f) != (size_t)m) return fail(SQE_ERR_IO, "sqe_index_load: file is truncated");
                SQE_TRY(group_index_add(idx, (const float*)pin.p, m, false, true));   // synchronises: the pinned buffer is reused
            }
        }
        if (h.flags & 1u) {
            if (idx->kind != SQE_INDEX_IVF_FLAT) return fail(SQE_ERR_IO, "sqe_index_load: IVF section in a flat index file");
            const size_t cb = (size_t)h.nlist * row_bytes, ab = (size_t)h.n * 4;
            std::vector<char> host(cb + ab);
            if (fread(host.data(), 1, cb + ab, fc.f) != cb + ab) return fail(SQE_ERR_IO, "sqe_index_load: file is truncated");
            SQE_TRY(group_index_ivf_restore(idx, (const float*)host.data(), (const int32_t*)(host.data() + cb), h.n,
                                            h.version == 2 ? ids.data() : nullptr));
        }
        guard.i = nullptr;
        *out = idx;
        return SQE_OK;
    }
    OpScope op(ctx, idx->ord, true);
    SQE_TRY(idx->stage_in.ensure((size_t)std::min<int64_t>(rows_per_step, std::max<int64_t>(h.n, 1)) * row_bytes));
    for (int64_t off = 0; off < h.n; off += rows_per_step) {
        const int64_t m = std::min(rows_per_step, h.n - off);
        if (fread(pin.p, row_bytes, (size_t)m, fc.f) != (size_t)m) return fail(SQE_ERR_IO, "sqe_index_load: file is truncated");
        SQE_HIP(hipMemcpyAsync(idx->stage_in.p, pin.p, (size_t)m * row_bytes, hipMemcpyHostToDevice, op.s));
        SQE_TRY(index_add_impl(idx, idx->stage_in.as<float>(), m, h.dim, true, op.s));
        SQE_HIP(hipStreamSynchronize(op.s));    // the pinned buffer is reused
    }
    if (h.flags & 1u) {
        if (!idx->ivf) return fail(SQE_ERR_IO, "sqe_index_load: IVF section in a flat index file");
        const size_t cb = (size_t)h.nlist * row_bytes, ab = (size_t)h.n * 4;
        std::vector<char> host(cb + ab);
        if (fread(host.data(), 1, cb + ab, fc.f) != cb + ab) return fail(SQE_ERR_IO, "sqe_index_load: file is truncated");
        DevBuf tmp;
        SQE_TRY(tmp.ensure(cb + std::max<size_t>(ab, 4)));
        SQE_HIP(hipMemcpyAsync(tmp.p, host.data(), cb + ab, hipMemcpyHostToDevice, op.s));
        SQE_TRY(ivf_restore(idx, idx->ivf, tmp.as<float>(), (const int32_t*)((char*)tmp.p + cb), h.n, op.s));
        SQE_HIP(hipStreamSynchronize(op.s));
    }
    if (h.version == 2) SQE_TRY(index_set_ids(idx, ids.data(), next_id, op.s));
    guard.i = nullptr;
    *out = idx;
    return SQE_OK;
}

int sqe_merge_topk_device(sqe_ctx* ctx, const float* cos_parts_dev, const int64_t* id_parts_dev,
                          int64_t part_stride_bytes, int P, int B, int k,
                          float* cos_out_dev, int64_t* id_out_dev) {
    if (!ctx) return fail(SQE_ERR_INVALID, "null handle");
    if (!cos_parts_dev || !id_parts_dev || !cos_out_dev || !id_out_dev)
        return fail(SQE_ERR_INVALID, "sqe_merge_topk: null buffer");
    if (part_stride_bytes < 0 || part_stride_bytes % 8 != 0) return fail(SQE_ERR_INVALID, "sqe_merge_topk: bad part stride");
    SQE_HIP(hipSetDevice(ctx->device));
    return launch_merge_topk(cos_parts_dev, id_parts_dev, part_stride_bytes, P, B, k, cos_out_dev, id_out_dev, 1, 0, 0,
                             ctx->stream.load());
}

// ================================================================ cache scan
// one-shot form: context-level host operation (its buffer and stream order belong to the context)
static int cosine_scan_host(sqe_ctx* ctx, const float* mat_host, int m, int dim, const float* q_host,
                            float* sims_out_host, float* best_sim, int32_t* best_idx) {
    if (m < 0 || dim <= 0 || dim % 4 != 0) return fail(SQE_ERR_INVALID, "cosine scan: bad m/dim");
    if (!q_host || (m > 0 && !mat_host)) return fail(SQE_ERR_INVALID, "cosine scan: null buffer");
    OpScope op(ctx, ctx->host, true);
    const size_t mb = (size_t)m * dim * 4, qb = (size_t)dim * 4, sb = round_up((int64_t)m * 4 + 4, 16);
    SQE_TRY(ctx->cache_tmp.ensure(mb + qb + sb + 16));
    char* base = ctx->cache_tmp.as<char>();
    float* d_mat = (float*)base;
    float* d_q = (float*)(base + mb);
    float* d_sims = (float*)(base + mb + qb);
    float* d_best = (float*)(base + mb + qb + sb);
    int32_t* d_idx = (int32_t*)(base + mb + qb + sb + 4);
    if (m > 0) SQE_HIP(hipMemcpyAsync(d_mat, mat_host, mb, hipMemcpyHostToDevice, op.s));
    SQE_HIP(hipMemcpyAsync(d_q, q_host, qb, hipMemcpyHostToDevice, op.s));
    {
        StageTimer t(ctx->prof, op.s, ST_CACHE);
        SQE_TRY(launch_cosine_scan(d_mat, nullptr, m, dim, d_q, d_sims, d_best, d_idx, op.s));
    }
    if (sims_out_host && m > 0)
        SQE_HIP(hipMemcpyAsync(sims_out_host, d_sims, (size_t)m * 4, hipMemcpyDeviceToHost, op.s));
    if (best_sim) SQE_HIP(hipMemcpyAsync(best_sim, d_best, 4, hipMemcpyDeviceToHost, op.s));
    if (best_idx) SQE_HIP(hipMemcpyAsync(best_idx, d_idx, 4, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_cosine_best(sqe_ctx* ctx, const float* mat_host, int m, int dim, const float* q_host,
                    float* best_sim, int32_t* best_idx) {
    if (!ctx) return fail(SQE_ERR_INVALID, "null handle");
    if (!best_sim || !best_idx) return fail(SQE_ERR_INVALID, "sqe_cosine_best: null output");
    return cosine_scan_host(ctx, mat_host, m, dim, q_host, nullptr, best_sim, best_idx);
}

int sqe_cosine_all(sqe_ctx* ctx, const float* mat_host, int m, int dim, const float* q_host,
                   float* sims_out_host) {
    if (!ctx) return fail(SQE_ERR_INVALID, "null handle");
    if (m > 0 && !sims_out_host) return fail(SQE_ERR_INVALID, "sqe_cosine_all: null output");
    float bs; int32_t bi;
    return cosine_scan_host(ctx, mat_host, m, dim, q_host, sims_out_host, &bs, &bi);
}

int sqe_cache_create(sqe_ctx* ctx, int capacity, int dim, sqe_cache** out) {
    if (!ctx) return fail(SQE_ERR_INVALID, "null handle");
    if (!out) return fail(SQE_ERR_INVALID, "sqe_cache_create: out is null");
    *out = nullptr;
    if (capacity <= 0 || dim <= 0 || dim % 4 != 0) return fail(SQE_ERR_INVALID, "sqe_cache_create: bad capacity/dim");
    SQE_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<sqe_cache> c(new (std::nothrow) sqe_cache);
    if (!c) return fail(SQE_ERR_OOM, "sqe_cache_create: host allocation failed");
    c->ctx = ctx; c->capacity = capacity; c->dim = dim;
    SQE_TRY(c->ord.init());
    int rc = c->mat.ensure((size_t)capacity * dim * 4);
    if (rc == SQE_OK) rc = c->work.ensure((size_t)dim * 4 + (size_t)capacity * 8 + 64);
    if (rc == SQE_OK) {
        OpScope op(ctx, c->ord, true);
        hipError_t e = hipMemsetAsync(c->mat.p, 0, (size_t)capacity * dim * 4, op.s);
        if (e != hipSuccess) rc = fail(SQE_ERR_HIP, std::string("cache memset: ") + hipGetErrorString(e));
    }
    if (rc != SQE_OK) { c->ord.destroy(); return rc; }
    *out = c.release();
    return SQE_OK;
}

void sqe_cache_destroy(sqe_cache* c) {
    if (!c) return;
    (void)hipSetDevice(c->ctx->device);
    {
        std::lock_guard<std::mutex> lk(c->ord.mu);
        c->ord.quiesce();
    }
    c->ord.destroy();
    delete c;
}

int sqe_cache_set_slot(sqe_cache* c, int slot, const float* vec_host) {
    if (!c) return fail(SQE_ERR_INVALID, "null cache");
    if (slot < 0 || slot >= c->capacity || !vec_host) return fail(SQE_ERR_INVALID, "sqe_cache_set_slot: bad slot");
    OpScope op(c->ctx, c->ord, true);
    SQE_HIP(hipMemcpyAsync(c->mat.as<float>() + (size_t)slot * c->dim, vec_host, (size_t)c->dim * 4,
                           hipMemcpyHostToDevice, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_cache_best(sqe_cache* c, const int32_t* order_host, int m, const float* q_host,
                   float* best_sim, int32_t* best_pos) {
    if (!c) return fail(SQE_ERR_INVALID, "null cache");
    if (m < 0 || m > c->capacity || !q_host || !best_sim || !best_pos || (m > 0 && !order_host))
        return fail(SQE_ERR_INVALID, "sqe_cache_best: bad arguments");
    for (int i = 0; i < m; ++i)
        if (order_host[i] < 0 || order_host[i] >= c->capacity) return fail(SQE_ERR_INVALID, "sqe_cache_best: slot out of range");
    sqe_ctx* ctx = c->ctx;
    OpScope op(ctx, c->ord, true);
    char* base = c->work.as<char>();
    float* d_q = (float*)base;
    float* d_sims = (float*)(base + (size_t)c->dim * 4);
    int32_t* d_order = (int32_t*)(base + (size_t)c->dim * 4 + (size_t)c->capacity * 4);
    float* d_best = (float*)(base + (size_t)c->dim * 4 + (size_t)c->capacity * 8);
    int32_t* d_idx = (int32_t*)(d_best + 1);
    SQE_HIP(hipMemcpyAsync(d_q, q_host, (size_t)c->dim * 4, hipMemcpyHostToDevice, op.s));
    if (m > 0) SQE_HIP(hipMemcpyAsync(d_order, order_host, (size_t)m * 4, hipMemcpyHostToDevice, op.s));
    {
        StageTimer t(ctx->prof, op.s, ST_CACHE);
        SQE_TRY(launch_cosine_scan(c->mat.as<float>(), d_order, m, c->dim, d_q, d_sims, d_best, d_idx, op.s));
    }
    SQE_HIP(hipMemcpyAsync(best_sim, d_best, 4, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(best_pos, d_idx, 4, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

// ================================================================ stats
int sqe_set_profiling(sqe_ctx* ctx, int on) {
    if (!ctx) return fail(SQE_ERR_INVALID, "null handle");
    ctx->prof.drain();
    ctx->prof.on.store(on != 0);
    return SQE_OK;
}

// one context's share of the statistics, ADDED to *out (timings, calls, uncertified queries of its last search)
static int stats_accumulate(sqe_ctx* ctx, sqe_stats_t* out) {
    SQE_HIP(hipSetDevice(ctx->device));
    ctx->prof.drain();
    {
        std::lock_guard<std::mutex> lk(ctx->prof.mu);
        out->scan_ms += ctx->prof.ms[ST_SCAN] + ctx->prof.ms[ST_COLLECT];   // collect-pass scans are scans
        out->prep_ms += ctx->prof.ms[ST_PREP];
        out->select_ms += ctx->prof.ms[ST_SELECT];
        out->add_ms += ctx->prof.ms[ST_ADD];
        out->encode_ms += ctx->prof.ms[ST_ENCODE];
        out->cache_ms += ctx->prof.ms[ST_CACHE];
        out->sample_ms += ctx->prof.ms[ST_SAMPLE];
        out->scan_calls += ctx->prof.calls[ST_SCAN];
    }
    if (ctx->i8_valid.load()) {
        unsigned long long v[4] = {0, 0, 0, 0};
        SQE_HIP(hipDeviceSynchronize());
        if (hipMemcpy(v, ctx->i8_last.p, 32, hipMemcpyDeviceToHost) == hipSuccess) {
            out->i8_collected += (int64_t)v[0]; out->i8_rescored += (int64_t)v[1]; out->i8_overflows += (int64_t)v[2];
        }
    }
    if (ctx->unc_valid.load()) {
        // the count was written on the stream of that search; a device-wide wait orders this read after it
        // whatever stream it was (stats are not on any hot path)
        int v = 0;
        SQE_HIP(hipDeviceSynchronize());
        if (hipMemcpy(&v, ctx->unc_last.p, 4, hipMemcpyDeviceToHost) == hipSuccess) out->uncertified += v;
    }
    return SQE_OK;
}

int sqe_stats(sqe_ctx* ctx, sqe_stats_t* out) {
    if (!ctx) return fail(SQE_ERR_INVALID, "null handle");
    if (!out) return fail(SQE_ERR_INVALID, "sqe_stats: out is null");
    memset(out, 0, sizeof(*out));
    SQE_TRY(stats_accumulate(ctx, out));
    // A multi-device context: the shards of its indexes belong to the member contexts, which is where their
    // searches book timings and uncertified counts (r02: the leader reported shard 0 only).  Timings add up over
    // the members (device time, not wall time: the shards run side by side), so does the uncertified count (a query
    // can fail its certificate on one shard and pass on another: the sum counts collect passes, not queries).
    if (ctx->group) {
        const int n = group_member_count(ctx);
        for (int p = 1; p < n; ++p) SQE_TRY(stats_accumulate(group_member(ctx, p), out));
        SQE_HIP(hipSetDevice(ctx->device));
        out->scan_rows = 0; out->scan_flops = 0; out->scan_bytes = 0;
        for (int p = 0; p < n; ++p) {
            sqe_ctx* m = group_member(ctx, p);
            out->scan_rows += m->last_scan_rows.load();
            out->scan_flops += m->last_scan_flops.load();
            out->scan_bytes += m->last_scan_bytes.load();
        }
        out->search_calls = ctx->search_calls.load();
        return SQE_OK;
    }
    out->search_calls = ctx->search_calls.load();
    out->scan_rows = ctx->last_scan_rows.load();
    out->scan_flops = ctx->last_scan_flops.load();
    out->scan_bytes = ctx->last_scan_bytes.load();
    return SQE_OK;
}

int sqe_collapse_swept(sqe_ctx* ctx, int64_t* out) {
    if (!ctx || !out) return fail(SQE_ERR_INVALID, "sqe_collapse_swept: null argument");
    int64_t v = 0;
    for (int p = 0; p < group_member_count(ctx); ++p) v += group_member(ctx, p)->collapse_swept.load();
    *out = v;
    return SQE_OK;
}

static void stats_reset_one(sqe_ctx* ctx) {
    ctx->prof.drain();
    std::lock_guard<std::mutex> lk(ctx->prof.mu);
    for (int i = 0; i < ST_COUNT; ++i) { ctx->prof.ms[i] = 0; ctx->prof.calls[i] = 0; }
    ctx->search_calls.store(0);
    ctx->i8_valid.store(false);      // the int8 counters describe the last int8 search SINCE the reset
}

int sqe_stats_reset(sqe_ctx* ctx) {
    if (!ctx) return fail(SQE_ERR_INVALID, "null handle");
    stats_reset_one(ctx);
    if (ctx->group) {
        for (int p = 1; p < group_member_count(ctx); ++p) {
            sqe_ctx* m = group_member(ctx, p);
            (void)hipSetDevice(m->device);
            stats_reset_one(m);
        }
        (void)hipSetDevice(ctx->device);
    }
    return SQE_OK;
}

}  // extern "C"
