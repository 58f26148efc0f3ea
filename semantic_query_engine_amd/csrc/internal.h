// internal.h -- the objects behind the opaque handles of include/sqe.h (shared by api.hip, search.hip, group.hip, ivf.hip (host side of the IVF layer),
// encoder.hip) and the locking / stream discipline every entry point follows.
//
// Threading model (the reference calls add_embeddings from a pool thread while search runs on the
// event loop, main.py:454-455 vs :499; ctypes drops the GIL):
//   * every object that owns device state (index, cache, encoder) has its OWN mutex and its OWN stream; there
//     is no context-wide lock, so an add on one index never blocks a search on another, the cache scan or the
//     encoder, and their kernels overlap on the device;
//   * host entry points (host pointers in, host pointers out) enqueue on the object's stream and synchronise
//     it before returning; "_device" entry points enqueue on the CONTEXT stream (sqe_stream / sqe_set_stream)
//     and do not synchronise -- that is the stream a caller orders its own work against;
//   * the operations of one object are serialised ACROSS streams by an event: an operation that runs on
//     another stream than the object's previous one first waits for that one's event (OpScope);
//   * a caller-owned stream installed with sqe_set_stream is used by every entry point of the context.
#pragma once

#include <atomic>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.h"

namespace sqe {

// ---------------------------------------------------------------- device buffer helper
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // grows (never shrinks); contents are NOT preserved
    int ensure(size_t need) {
        if (need <= bytes) return SQE_OK;
        release();
        hipError_t e = hipMalloc(&p, need);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(SQE_ERR_OOM, std::string("hipMalloc(") + std::to_string(need) + "): " + hipGetErrorString(e));
        }
        bytes = need;
        return SQE_OK;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// ---------------------------------------------------------------- profiling
enum Stage { ST_SCAN = 0, ST_PREP, ST_SELECT, ST_ADD, ST_ENCODE, ST_CACHE, ST_COLLECT, ST_SAMPLE, ST_COUNT };

// hipEvent pairs around the stages, on whatever stream the stage ran on; totals are read by sqe_stats.
struct Profiler {
    std::atomic<bool> on{false};
    std::mutex mu;
    struct Pending { int stage; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
    double ms[ST_COUNT] = {0};
    int64_t calls[ST_COUNT] = {0};

    hipEvent_t get() {                       // caller holds mu
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    void drain_locked() {
        for (auto& pd : pending) {
            float t = 0.f;
            if (hipEventSynchronize(pd.b) == hipSuccess && hipEventElapsedTime(&t, pd.a, pd.b) == hipSuccess) {
                ms[pd.stage] += t;
                calls[pd.stage]++;
            }
            pool.push_back(pd.a);
            pool.push_back(pd.b);
        }
        pending.clear();
    }
    void drain() {
        std::lock_guard<std::mutex> lk(mu);
        drain_locked();
    }
    ~Profiler() {
        for (auto& pd : pending) { (void)hipEventDestroy(pd.a); (void)hipEventDestroy(pd.b); }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
};

struct StageTimer {
    Profiler& pf; hipStream_t s; int stage; hipEvent_t a = nullptr;
    StageTimer(Profiler& p, hipStream_t st, int stg) : pf(p), s(st), stage(stg) {
        if (pf.on.load(std::memory_order_relaxed)) {
            std::lock_guard<std::mutex> lk(pf.mu);
            if (pf.pending.size() >= 2048) pf.drain_locked();
            a = pf.get();
            (void)hipEventRecord(a, s);
        }
    }
    ~StageTimer() {
        if (a) {
            std::lock_guard<std::mutex> lk(pf.mu);
            hipEvent_t b = pf.get();
            (void)hipEventRecord(b, s);
            pf.pending.push_back({stage, a, b});
        }
    }
};

// ---------------------------------------------------------------- per-object operation order
struct OpOrder {
    std::mutex mu;                 // one operation of the object at a time (host side)
    hipStream_t own = nullptr;     // the object's stream (host entry points)
    hipEvent_t ev = nullptr;       // recorded after every operation
    hipStream_t last = nullptr;    // stream of the previous operation
    bool armed = false;            // ev has been recorded at least once
    int init() {                   // current device = the object's device
        SQE_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
        SQE_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        return SQE_OK;
    }
    // wait (host) for the object's last operation, whatever stream it ran on -- never touches a stream handle,
    // so a caller-owned stream that has died since is no hazard
    void quiesce() {
        if (armed) (void)hipEventSynchronize(ev);
    }
    void destroy() {
        quiesce();
        if (ev) (void)hipEventDestroy(ev);
        if (own) (void)hipStreamDestroy(own);
        ev = nullptr; own = nullptr; armed = false;
    }
};

struct IvfState;
struct FilterState;  // filter.hip: the sub-index and buffers of filtered searches (created by the first one)
struct FieldState;   // fields.hip: the field columns and the buffers of the field predicates (created by the first sqe_index_set_field)
struct AggState;     // aggregate.hip: the tables and the route record of field aggregations (created by the first one)
struct WhereMaskState;   // where_mask.hip: the buffers of the mask route of sqe_index_search_where (created by the first call that takes it)
struct SortState;    // sort.hip: the candidate lists and the record of field sorts (created by the first one)
struct FilterEachState;  // filter_each.hip: the buffers of per-query filtered searches (created by the first one)
struct RangeState;   // range.hip: the buffers of radial searches (created by the first one)
struct CollapseState;   // collapse.hip: the buffers of collapsed searches (created by the first one)
struct ExcludeState;    // exclude.hip: the buffers of exclusion searches (created by the first one)
struct MmrState;     // mmr.hip: the buffers of MMR searches (created by the first one)
struct FuseState;    // fuse.hip: the buffers of fused multi-query searches (created by the first one)
constexpr int RANGE_MAX_HITS = 10000;   // max_hits limit of sqe_index_range_search (OpenSearch's k / window limit)
struct Group;        // group.hip: the member contexts / shards of a multi-device context
struct GroupIndex;

}  // namespace sqe

// ================================================================ objects
struct sqe_ctx {
    int device = 0;
    std::atomic<hipStream_t> stream{nullptr};   // stream of the "_device" entry points (own_stream unless sqe_set_stream)
    hipStream_t own_stream = nullptr;           // created by sqe_create
    std::atomic<bool> foreign{false};           // a caller-owned stream is installed: every entry point uses it
    std::mutex mu;                              // stream swaps and the one-shot cosine scan's buffer
    sqe::OpOrder host;                          // context-level host operations (one-shot cosine scan)
    int cu_count = 256;
    int64_t hbm_bytes = 0;
    std::string name;
    sqe::Profiler prof;
    std::atomic<int64_t> last_scan_rows{0}, last_scan_flops{0}, last_scan_bytes{0}, search_calls{0};
    sqe::DevBuf unc_last;    // 16 B owned by the context: uncertified-query count of the last certified search
                             //   (copied on the search's stream; never a pointer into an index's buffers)
    std::atomic<bool> unc_valid{false};
    sqe::DevBuf i8_last;     // 32 B: keys collected / rows re-scored / overflows / uncertified of the last int8 search
    std::atomic<bool> i8_valid{false};
    sqe::DevBuf cache_tmp;   // one-shot cosine scan: matrix + q + sims + best
    std::atomic<int64_t> collapse_swept{0};     // queries of the last collapsed search that the sweep (stage B) answered
    std::atomic<int64_t> exclude_swept{0};      // the same of the last exclusion search
    sqe::Group* group = nullptr;                // n_dev > 1: this context leads a device group (group.hip)
};

struct sqe_index {
    sqe_ctx* ctx = nullptr;
    sqe::OpOrder ord;
    int dim = 0;
    int kind = SQE_INDEX_FLAT;
    int nlist = 0;
    std::atomic<int64_t> n{0};
    int64_t cap = 0;               // rows allocated (multiple of 256)
    float* master = nullptr;       // [cap, dim] fp32 normalised
    sqe::bf16_t* scan = nullptr;   // [cap] rows of dim bf16 at `pitch` bytes, zero past n
    int pitch = 0;                 // bytes between rows of the scanned copy and of the bf16 query block
    int scan_mode = SQE_SCAN_BF16_RESCORE;
    int rescore_k = 0;             // 0 = automatic
    int nprobe = 0;
    int64_t id_base = 0;           // added to returned ids (row-sharded index)
    sqe::DevBuf qn;                // [B, dim] fp32 normalised queries
    sqe::DevBuf qb;                // [b_pad, dim] bf16 queries
    sqe::DevBuf cand;              // [n_chunks, b_pad, CAND_CAP] u64
    sqe::DevBuf cand_cnt;          // [n_chunks, b_pad] int
    sqe::DevBuf gmax;              // [b_pad, ngroups, 64] u32 chunk maxima (global bound table)
    sqe::DevBuf dbg;               // 8 x u64 debug counters (knobs build, SQE_DBG bit 32)
    sqe::DevBuf resid_max;         // u32 float bits: max over rows of || x_hat - bf16(x_hat) ||
    sqe::DevBuf q_resid;           // [B] the same per query
    sqe::DevBuf unc;               // int count (16 B) | float collect_thr[b_pad]
    sqe::DevBuf fb_keys, fb_cnt;   // exact-rescan collection buffers (by compact index)
    sqe::DevBuf unc_ids, thr_c, qb_c;   // uncertified queries compacted into a dense batch: ids, thresholds, bf16 rows
    sqe::DevBuf stage_in, stage_out;    // H2D / D2H staging of the host entry points
    int certify = 1;               // run the exactness certificate + fp32 rescan fallback
    // ---- int8 first pass (scan_mode == SQE_SCAN_INT8_RESCORE; quant.hip, scan_i8.hip, select_i8.hip)
    sqe::DevBuf i8db;              // tiled int8 copy: tile t (256 rows) at t * i8_tile_stride
    sqe::DevBuf i8sxi;             // [i8_cap_tiles * 256] u32 row scales
    sqe::DevBuf i8resid_max;       // u32 float bits: max over rows of || x_hat - sxi unit x8 ||
    int64_t i8_cap_tiles = 0, i8_tile_stride = 0;
    int64_t i8_rows = 0;           // rows [0, i8_rows) of the int8 copy are current (filled lazily by the first search after an add)
    sqe::DevBuf q8t;               // the quantised queries tiled in 256-query blocks (quant.hip): the ping-pong int8 kernels' operand
    sqe::DevBuf q8, q8sqi, q8resid, i8thr_int, i8thr_eff, i8cos_s, i8ids_s, i8stats, i8samp;   // per search
    int64_t i8_min_rows = 1000000; // below this many rows (or dim < 256, dim % 128 != 0, k > the sample's m) the bf16 scan answers (search.hip: admit_i8; any batch size)
    int i8_sample_step = 100;      // the threshold pass scans every i8_sample_step-th tile with the bf16 kernels ...
    int i8_sample_m = 20;          // ... and the collect threshold of a query is its m-th best true cosine there (~step x m = 2,000
                                   //   rows collected per query; r03 sweep, profiles/r03_search/i8_sample_sweep.log: a proof starts
                                   //   to fail when fewer than ~380 rows of a query are collected, i.e. when >= m sample rows beat
                                   //   the rank-380 score -- Poisson(3.8) >= 20: 1e-8 per query; any failure costs a 3 ms bf16 pass)
    float i8_dx = 0.f;             // host copy of the int8 residual maximum (refreshed when rows were quantised)
    bool i8_dx_stale = true;
    bool i8_oom_logged = false;    // the int8 copy did not fit: scan_mode fell back to BF16_RESCORE (search.hip: admit_i8)
    int i8_sample_int8 = 1;        // threshold pass: 1 = int8 sample scan + order statistic (r03c), 0 = bf16 scan + fp32 re-score of the sample
    double i8_max_resid = 0.02;    // rows that quantise worse than this (one element 40 x the others: 0.05 at dim 1024) would
                                   //   make every certificate fail: the index then answers with the bf16 scan
    sqe::DevBuf i8ovf, i8ovf_cnt;  // overflow pool of the collect scan: [b_pad, I8_OVF_CAP] keys, [b_pad] counts (kernels.h)
    double i8_anchor_margin = 0.25;// the collect threshold never lies above (best true cosine of the sample) - eps (1 + margin): select_i8.hip
    int i8_key_budget = 6144;      // where the sample predicts that the anchored threshold collects more keys than this, it is not used (0 = no limit)
    int i8_keep_select = 0;        // test-only ("i8_keep_select"): snapshot what select_i8_kernel wrote before the bf16 collect pass overwrites it
    bool i8_kept = false;          //   the last int8 search took that snapshot (sqe_index_i8_read: SQE_I8_SELECT_*)
    sqe::DevBuf i8keep_cos, i8keep_ids, i8keep_thr, i8keep_trace;   // [B, k] f32, [B, k] i64, [b_pad] f32, [B, 4] i32: allocated only with the option on
    sqe_i8_launch_t i8_launch{};   // the last int8 search (sqe_index_i8_last); rows == 0: none yet
    sqe_scan_launch_t scan_launch{};   // the last search pass when the bf16 first pass answered it (sqe_index_scan_last); rows == 0: it did not
    int last_B = 0;                // queries of the last search pass: extent of qn / q_resid / q8resid / q8sqi (sqe_index_state_read)
    bool last_i8 = false;          //   and whether it ran the int8 first pass
    sqe::IvfState* ivf = nullptr;  // kind == SQE_INDEX_IVF_FLAT
    bool internal = false;         // sub-index of another object (IVF coarse quantiser): runs under its owner's lock and stream
    sqe::GroupIndex* group = nullptr;   // index of a multi-device context: one shard per member device (group.hip)
    // ---- deletes (compact.hip).  Until the first delete a row's id is its position and there is no map.
    std::atomic<int64_t> next_id{0};    // rows ever appended: the id the next appended row gets (ids are never reused)
    bool has_map = false;               // idmap is valid: a row was deleted (or a file with holes was loaded)
    sqe::DevBuf idmap;                  // [cap] int64, position -> local id, strictly increasing over [0, n)
    sqe_delete_last_t delete_last{};    // the blocks the last delete walked (sqe_index_delete_last); n_old == 0: none yet
    // ---- filtered searches (filter.hip)
    sqe::FilterState* filter = nullptr; // null until the first filtered search
    int64_t filter_gather_rows = 1 << 20;   // allowed rows gathered (and searched) per chunk
    // ---- per-query filtered searches (filter_each.hip); the defaults: profiles/filter_each/NOTES.md
    sqe::FilterEachState* filter_each = nullptr;   // null until the first per-query filtered search
    int64_t filter_each_direct_rows = 1 << 14;     // a list of at most this many entries ...
    int filter_each_direct_queries = 32;           // ... that at most this many queries name is scored directly
    int64_t filter_each_key_budget = 1 << 24;      // keys (queries of a pass x their list's length) held at once
    // ---- radial searches (range.hip)
    sqe::RangeState* range = nullptr;   // null until the first radial search
    int64_t range_key_budget = 1 << 25; // collected keys held at once (queries per collect group = budget / 4096)
    // ---- group keys and collapsed searches (collapse.hip).  Until the first sqe_index_set_keys there is no key array.
    bool has_keys = false;              // keys is valid
    sqe::DevBuf keys;                   // [cap] int64, position -> group key, SQE_KEY_NONE for rows without one and past n
    sqe::CollapseState* collapse = nullptr;   // null until the first collapsed search
    int collapse_depth = 0;             // rows the first stage of a collapsed search fetches (0 = automatic)
    // ---- exclusion searches (exclude.hip)
    sqe::ExcludeState* exclude = nullptr;     // null until the first exclusion search
    int exclude_depth = 0;              // cap on the rows the first stage of an exclusion search fetches (0 = k + list length)
    // ---- MMR searches (mmr.hip)
    sqe::MmrState* mmr = nullptr;       // null until the first MMR search
    int64_t mmr_row_budget = 1 << 16;   // candidate rows (queries of a pass x depth n) whose Gram scratch and gathered parts are held at once
    // ---- fused multi-query searches (fuse.hip)
    sqe::FuseState* fuse = nullptr;     // null until the first fused search
    // ---- numeric fields and field predicates (fields.hip).  Until the first sqe_index_set_field there is no column.
    sqe::FieldState* fields = nullptr;  // null until the first set_field or field predicate
    sqe::AggState* agg = nullptr;       // field aggregations (aggregate.hip): null until the first one
    sqe::SortState* sort = nullptr;     // field sorts (sort.hip): null until the first one
    // ---- the routes of sqe_index_search_where (fields.hip: where_mask_plan; where_mask.hip)
    sqe::WhereMaskState* where_mask = nullptr;   // null until the first call that takes the mask route
    int where_route = 0;                // "where_route": 0 = the cost rule chooses, 1 = always gather, 2 = mask whenever the index is FLAT
    int where_mask_depth = 0;           // "where_mask_depth": rows the mask route's first stage fetches (0 = fieldpred.h: where_depth)
    int64_t where_mask_min_rows = 1000000;  // "where_mask_min_rows": fewer selected rows are always gathered under route 0 (profiles/where_mask/NOTES.md)
    sqe_where_last_t where_last{0, 0, 0, 0, 0, -1, 0};   // the last sqe_index_search_where (sqe_index_where_last); live < 0: none yet
    // ---- restricted radial, collapsed and MMR searches (within.hip)
    int within_route = 0;               // "within_route": 0 = gather iff the row set fits "filter_gather_rows", else mask; 2 = always mask
    sqe_within_last_t within_last{0, 0, 0, 0, 0, -1, 0};   // the last restricted search (sqe_index_within_last); live < 0: none yet
    int sort_fan_in = 64;               // candidate lists one merge workgroup of a field sort takes ("sort_fan_in", 2..64)
};

struct sqe_cache {
    sqe_ctx* ctx = nullptr;
    sqe::OpOrder ord;
    int capacity = 0, dim = 0;
    sqe::DevBuf mat;     // [capacity, dim] raw fp32
    sqe::DevBuf work;    // q [dim] | sims [capacity] | best_sim | best_idx | order [capacity]
};

namespace sqe {

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
inline unsigned grid_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }   // workgroups for n items

// ---- device groups: the byte layout of one shard's result part, from (B, k or m).  P parts lie one after the other in the
// leader's gather buffer, and the merged result of a host call has the layout of one part.  The merge kernels compute the
// same offsets on the device.
inline size_t round16(size_t v) { return (v + 15) / 16 * 16; }
struct PackedPart {      // ids [B, k] int64 | cos [B, k] fp32, the whole rounded to 16 B
    size_t id_off, cos_off, id_bytes, cos_bytes, total;
    static PackedPart of(int B, int k) {
        const size_t n = (size_t)B * k;
        return {0, n * 8, n * 8, n * 4, round16(n * 12)};
    }
};
struct RangePart {       // counts [B] int64 | cos [B, m] fp32 (16-B rounded) | ids [B, m] int64
    size_t count_off, cos_off, id_off, count_bytes, cos_bytes, id_bytes, total;
    static RangePart of(int B, int m) {
        const size_t n = (size_t)B * m, c = (size_t)B * 8, i = c + round16(n * 4);
        return {0, c, i, c, n * 4, n * 8, i + n * 8};
    }
};
struct CollapsePart {    // cos [B, k] fp32 (16-B rounded) | ids [B, k] int64 | keys [B, k] int64
    size_t cos_off, id_off, key_off, cos_bytes, id_bytes, total;      // keys take id_bytes
    static CollapsePart of(int B, int k) {
        const size_t n = (size_t)B * k, i = round16(n * 4);
        return {0, i, i + n * 8, n * 4, n * 8, i + n * 16};
    }
};

struct MmrPart {         // cos [B, n] fp32 (16-B rounded) | ids [B, n] int64 (16-B rounded) | rows [B, n, dim] fp32
    size_t cos_off, id_off, row_off, total;
    static MmrPart of(int B, int n, int dim) {
        const size_t m = (size_t)B * n, i = round16(m * 4), r = i + round16(m * 8);
        return {0, i, r, r + m * dim * 4};
    }
};
struct MmrOut {          // a host call's merged result: cos [B, k] fp32 (16-B rounded) | ids [B, k] int64 | mmr [B, k] fp32
    size_t cos_off, id_off, mmr_off, cos_bytes, id_bytes, total;
    static MmrOut of(int B, int k) {
        const size_t m = (size_t)B * k, i = round16(m * 4);
        return {0, i, i + m * 8, m * 4, m * 8, round16(i + m * 12)};
    }
};

struct FusedOut {        // a fused search's host result: fused [G, k] fp32 (16-B rounded) | ids [G, k] int64 | cos [G, k] fp32
    size_t fused_off, id_off, cos_off, f32_bytes, id_bytes, total;      // fused and cos take f32_bytes each
    static FusedOut of(int G, int k) {
        const size_t m = (size_t)G * k, i = round16(m * 4);
        return {0, i, i + m * 8, m * 4, m * 8, round16(i + m * 12)};
    }
};

// Scope of one operation on an object: device set, object locked, stream chosen and ordered after the
// object's previous operation; the destructor records the object's event on that stream.
struct OpScope {
    OpOrder& o;
    hipStream_t s;
    bool locked;
    OpScope(sqe_ctx* c, OpOrder& ord, bool host_call, bool lock = true) : o(ord), locked(lock) {
        (void)hipSetDevice(c->device);
        if (locked) o.mu.lock();
        s = (host_call && !c->foreign.load()) ? o.own : c->stream.load();
        if (o.armed && o.last != s) (void)hipStreamWaitEvent(s, o.ev, 0);
    }
    ~OpScope() {
        (void)hipEventRecord(o.ev, s);
        o.last = s;
        o.armed = true;
        if (locked) o.mu.unlock();
    }
    OpScope(const OpScope&) = delete;
    OpScope& operator=(const OpScope&) = delete;
};

// ---- internal forms of the index operations: no locking, explicit stream (api.hip; index_search_impl: search.hip)
int index_create_impl(sqe_ctx* ctx, int dim, int kind, int nlist, bool internal, sqe_index** out);
int index_grow(sqe_index* idx, int64_t need_rows, hipStream_t s);
// rows are [n] x dim floats, `x_stride` floats apart (>= dim; a strided view of a row-major block)
int index_add_impl(sqe_index* idx, const float* x_dev, int64_t n, int64_t x_stride, bool restore, hipStream_t s);
int index_update_impl(sqe_index* idx, const int64_t* rows_dev, const float* x_dev, int64_t n, hipStream_t s);
int index_search_impl(sqe_index* idx, const float* q_dev, int B, int k, int nprobe, float* cos_out_dev, int64_t* id_out_dev,
                      hipStream_t s, int pass_index = 0);

// ---- IVF layer (ivf.hip: host side; its kernels are in ivf_scan.hip, ivf_select.hip, ivf_build.hip); every call runs under the base index's lock, on stream s
int ivf_create(sqe_index* base, IvfState** out);
void ivf_destroy(IvfState* st);
int ivf_rows_added(sqe_index* base, IvfState* st, hipStream_t s);
int ivf_rows_updated(sqe_index* base, IvfState* st, const int64_t* rows_dev, int64_t n, hipStream_t s);
int ivf_train(sqe_index* base, IvfState* st, const float* x_dev, int64_t n, int iters, uint64_t seed, hipStream_t s);
int ivf_search(sqe_index* base, IvfState* st, const float* q_dev, int B, int k, int nprobe, float* cos_out, int64_t* id_out,
               hipStream_t s);
int ivf_export(sqe_index* base, IvfState* st, float* centroids_host, int32_t* assign_host, hipStream_t s);
// test-only read-back of the last search piece (sqe_index_ivf_state[_read]): one stream synchronisation, nothing allocated or launched
int ivf_state(sqe_index* base, IvfState* st, sqe_ivf_state_t* out, hipStream_t s);
int ivf_state_read(sqe_index* base, IvfState* st, int what, int64_t offset, void* out_host, int64_t bytes, hipStream_t s);
void ivf_invalidate(IvfState* st);
sqe_index* ivf_coarse(IvfState* st);
bool ivf_trained(IvfState* st);
int ivf_restore(sqe_index* base, IvfState* st, const float* centroids_dev, const int32_t* assign_dev, int64_t n, hipStream_t s);
void ivf_assignments(IvfState* st, int** assign, int64_t* n_assigned);     // (null, 0) before training
void ivf_rows_deleted(IvfState* st, int64_t n_assigned);                  // assign was compacted to n_assigned rows: lists rebuild lazily

// ---- deletes and the id map (compact.hip); caller holds the index lock, stream s
int64_t search_id_base(const sqe_index* idx);      // id_base the position-level search kernels add (0 once the index has a map)
int index_translate_ids(sqe_index* idx, int64_t* id_dev, int64_t count, hipStream_t s);   // positions -> ids (+ id_base) if mapped
// plain positions -> ids through the id map, if there is one, + id_base; launches nothing when neither applies
int index_positions_to_ids(sqe_index* idx, int64_t* id_dev, int64_t count, hipStream_t s);
// ids -> positions (host), SQE_ERR_INVALID naming `what` if an id is not live
int index_resolve_ids(sqe_index* idx, const int64_t* ids_host, int64_t m, std::vector<int64_t>& pos, hipStream_t s, const char* what);
int index_delete_positions(sqe_index* idx, const std::vector<int64_t>& pos_sorted, hipStream_t s);
int index_ids_host(sqe_index* idx, std::vector<int64_t>& out, hipStream_t s);
int index_set_ids(sqe_index* idx, const int64_t* ids_host, int64_t next_id, hipStream_t s);   // sqe_index_load of a file with holes
int launch_idmap_iota(int64_t* map, int64_t first_pos, int64_t first_id, int64_t n, hipStream_t s);
int launch_idmap_lookup(const int64_t* map, int64_t n, const int64_t* ids, int64_t m, int64_t* pos_out, hipStream_t s);
// ids[j] = position >= 0 ? (map ? map[position] : position) + id_base : -1
int launch_translate_ids(int64_t* ids, int64_t count, const int64_t* map, int64_t id_base, hipStream_t s);
// `count` empty hits: cos -inf, ids -1 and, unless null, keys SQE_KEY_NONE
int launch_pad_hits(float* cos, int64_t* ids, int64_t* keys, int64_t count, hipStream_t s);

// ---- id lists (compact.hip; their device side, resolve_id and the position sets, is id_lists.h): what the filtered, per-query
// filtered and exclusion searches share on the host.
// the argument checks of the entry points that take per-query id lists (who: "sqe_..: ", ids_name: the id array's name in the
// messages, min_list: the lowest list_of_query value allowed, -1 where a query may name no list)
int list_args_ok(const char* who, const char* ids_name, int min_list, sqe_index* idx, const void* q, int B, int k, const void* list_ids,
                 const int64_t* offsets, int n_lists, const int32_t* list_of_query, const void* cos, const void* ids);
// "_device" entry points of a device group route the lists on the host: the ids of all lists come over on the context stream
// (after the caller's work on it), which is synchronised
int list_ids_to_host(sqe_ctx* ctx, const int64_t* ids_dev, const int64_t* offsets, int n_lists, std::vector<int64_t>& out);
// host ids into buf (grown as needed) by one copy on s; *dev = the device copy, null for count 0.  `host` is read until s has
// passed the copy: the *_host_ids forms below synchronise s before they return
int stage_host_ids(DevBuf& buf, const int64_t* host, int64_t count, hipStream_t s, const int64_t** dev);

// ---- filtered searches (filter.hip); caller holds the index lock, stream s.  Both synchronise s once (the allowed-row count).
int index_search_filtered_impl(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* allow_dev, int64_t n_allow,
                               float* cos_out_dev, int64_t* id_out_dev, hipStream_t s);
int index_search_filtered_host_ids(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* allow_host, int64_t n_allow,
                                   float* cos_out_dev, int64_t* id_out_dev, hipStream_t s);
void filter_destroy(FilterState* f);
// The filtered search split at its bitmap (u32 words, bit p & 31 of word p >> 5, zero-padded to blocks of 1,024 words and zero at
// or beyond n): ensure sizes the map and the count buffers for the index as it stands, mark clears it and sets the rows of the
// allowed ids, index_search_bitmap runs everything from the count on (one synchronisation of s) over a map of at most pos_cap
// set bits.  stage_allow_ids: a host allow-list into the state's own buffer (the caller synchronises s before it returns).
// Besides the filtered search itself only rowset_map (rowset.hip) marks and stages.
int filter_bitmap_ensure(sqe_index* idx, FilterState** f_out, int64_t* words_out);
uint32_t* filter_bitmap(FilterState* f);
int filter_bitmap_mark(sqe_index* idx, FilterState* f, int64_t words, const int64_t* allow_dev, int64_t n_allow, hipStream_t s);
int stage_allow_ids(FilterState* f, const int64_t* allow_host, int64_t n_allow, hipStream_t s, const int64_t** dev);
int index_search_bitmap(sqe_index* idx, FilterState* f, int64_t words, int64_t pos_cap, const float* q_dev, int B, int k,
                        float* cos_out_dev, int64_t* id_out_dev, hipStream_t s);
// index_search_bitmap in its two halves, for a caller that chooses what to do once it knows the count (rowset_positions): the map ->
// the ascending positions in the state and *M_out, their number (the synchronisation); then the gather, search and id mapping
int index_bitmap_positions(sqe_index* idx, FilterState* f, int64_t words, int64_t pos_cap, int64_t* M_out, hipStream_t s);
// (as_positions: id_out gets plain row positions, -1 padded, as the callers that go on to read the rows want them)
int index_search_gathered(sqe_index* idx, FilterState* f, int64_t M, const float* q_dev, int B, int k, float* cos_out_dev,
                          int64_t* id_out_dev, hipStream_t s, bool as_positions = false);
// within.hip's gather route: rows pos[0, M) (one chunk) and, with_keys, their group keys into the scratch sub-index, which inherits
// the owner's options; *pos_out: the positions of index_bitmap_positions, sub position -> owner position
int filter_gather_sub(sqe_index* idx, FilterState* f, int64_t M, bool with_keys, sqe_index** sub_out, const int64_t** pos_out, hipStream_t s);
// the count / scan and write kernels of the filtered search over any map of that layout with nb blocks: counts [nb] ints,
// offs [nb] the blocks' exclusive scan, *total the set bits; pos gets the set positions ascending
int launch_bitmap_count(const uint32_t* bits, int64_t nb, int* counts, int64_t* offs, int64_t* total, hipStream_t s);
int launch_bitmap_write(const uint32_t* bits, int64_t nb, const int64_t* offs, int64_t* pos, hipStream_t s);

// ---- numeric fields and field predicates (fields.hip); caller holds the index lock, stream s.  The tables of FieldPreds are
// HOST memory, checked by the caller (fieldpred_check).
struct FieldPreds {
    const sqe_field_clause_t* clauses;
    const int64_t* offsets;        // [n_preds + 1]
    int n_preds;
    const int64_t* set_values;
    int64_t n_set;
};
// The row set of sqe_index_search_where, and how it travels inside the library to every call that takes one (search_where,
// aggregate_fields, sort_fields, the _where forms of radial, collapsed and MMR search): the live rows the predicate
// pr.offsets[0 .. 1] selects, intersected with an allow-list.  n_allow == -1: no list; 0: the empty list, which selects nothing;
// > 0: allow [n_allow] ids, LOCAL to the index or shard (a device group routes the caller's global ids first; ids that repeat
// or name no live row are fine).  allow_on_host: the list is host memory, staged by rowset_map and read until the caller's next
// synchronisation of the stream; else it is on the device.
struct RowSet {
    FieldPreds pr;
    const int64_t* allow;
    int64_t n_allow;
    bool allow_on_host;
};
// ---- the row set's checks and preparation (rowset.hip)
// the six row-set arguments of a C entry point `who` ("sqe_index_..."); one [2] receives the offsets of the one predicate
int rowset_args_ok(const char* who, const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                   const void* allow, int64_t n_allow, int64_t* one);
// a "_device" entry point on a device group plans the shards on the host: the device list (n_allow may be -1) comes over on the
// context stream (after the caller's work on it), which is synchronised
int rowset_allow_to_host(sqe_index* idx, const int64_t* allow_dev, int64_t n_allow, std::vector<int64_t>& out);
// The preparation; caller holds the index lock, n > 0 and n_allow != 0, stream s.  rowset_map: the filter's map for the index as it
// stands -- a host list staged, the list marked, the field match kernel written over the map or ANDed into the marks.  It
// synchronises nothing: a host list is read until the caller's next synchronisation of s, which every caller has on its error
// path too.  *f_out, *words_out: the filter state and the map's length, as filter_bitmap_ensure gives them; filter_bitmap(f) is
// the map.  rowset_positions: the ascending positions of the map's set bits into the filter state (index_search_gathered,
// filter_gather_sub read them there) and *M_out, their number: the one synchronisation of s.
int rowset_map(sqe_index* idx, const RowSet& set, FilterState** f_out, int64_t* words_out, hipStream_t s);
int rowset_positions(sqe_index* idx, const RowSet& set, FilterState* f, int64_t words, int64_t* M_out, hipStream_t s);
int fields_args_ok(const char* who, const FieldPreds& pr);
void fields_destroy(FieldState* f);
// index_grow: the columns follow to new_cap rows (rows [0, n) keep their values, every other position reads SQE_FIELD_NONE);
// synchronises s.  index_delete_positions: every column compacted by the sorted deleted positions del_dev [m]; synchronises s.
int fields_grow(sqe_index* idx, int64_t n, int64_t new_cap, hipStream_t s);
int fields_rows_deleted(sqe_index* idx, const int64_t* del_dev, int64_t m, int64_t n_old, hipStream_t s);
// values_host[j] to the row at pos[j] in column `field` (the last of a repeated position wins) / the values of those rows; both
// synchronise s
int index_set_field_at(sqe_index* idx, int field, const std::vector<int64_t>& pos, const int64_t* values_host, hipStream_t s);
int index_get_field_at(sqe_index* idx, int field, const std::vector<int64_t>& pos, int64_t* values_out_host, hipStream_t s);
void index_field_info(sqe_index* idx, int* n_fields, int64_t* bytes);
// counts [n_preds] and ids [n_preds, cap] on the device (ids as sqe_index_search returns them); synchronises nothing
int index_match_fields_impl(sqe_index* idx, const FieldPreds& pr, int64_t cap, int64_t* count_dev, int64_t* id_dev, hipStream_t s);
// the exact top-k over the rows of `set`.  One synchronisation of s, for the count; a host list synchronises s once more before
// the return.
int index_search_where_impl(sqe_index* idx, const float* q_dev, int B, int k, const RowSet& set, float* cos_out_dev, int64_t* id_out_dev,
                            hipStream_t s, bool as_positions = false);
// pred_of_query [B] on the host, checked by the caller.  One synchronisation of s for the counts, then what
// index_search_filtered_each_impl costs.
int index_search_where_each_impl(sqe_index* idx, const float* q_dev, int B, int k, const FieldPreds& pr, const int32_t* pred_of_query,
                                 float* cos_out_dev, int64_t* id_out_dev, hipStream_t s);
// the match kernel of the predicate pr.offsets[0 .. 1] over the index as it stands into a map of the filtered search's layout
// (filter_bitmap_ensure), written whole or, with and_into, ANDed into what filter_bitmap_mark left there; rowset_map's step
int fields_bitmap_eval(sqe_index* idx, const FieldPreds& pr, uint32_t* bits, bool and_into, hipStream_t s);
const int64_t* fields_column(const sqe_index* idx, int field);      // the device column of a slot by row position; null: never set

// ---- the mask route of sqe_index_search_where (where_mask.hip); caller holds the index lock, stream s.  bits: a map of the
// filtered search's layout over the index as it stands, read only; k <= d <= 256; FLAT indexes of at most 2^32 rows.  Outputs
// [B, k] on the device (ids as sqe_index_search returns them), *swept_out the queries the sweep answered.  Synchronises s once
// after the first stage and once per row range of the sweep.
int index_search_where_mask(sqe_index* idx, const uint32_t* bits, int d, const float* q_dev, int B, int k, float* cos_out_dev,
                            int64_t* id_out_dev, int64_t* swept_out, hipStream_t s, bool as_positions = false);
void where_mask_destroy(WhereMaskState* w);

// ---- restricted radial, collapsed and MMR searches (within.hip); caller holds the index lock, stream s.  Each is the unrestricted
// impl of its kind over the rows of `set` only, with the same outputs; each synchronises s once for the size of the set (MMR: as
// index_search_where_impl does) besides what its kind synchronises.
int index_range_search_within(sqe_index* idx, const float* q_dev, int B, const float* min_cos_dev, int m, const RowSet& set,
                              int64_t* count_dev, float* cos_dev, int64_t* id_dev, hipStream_t s);
int index_search_collapsed_within(sqe_index* idx, const float* q_dev, int B, int k, const RowSet& set, float* cos_dev, int64_t* id_dev,
                                  int64_t* key_dev, hipStream_t s);
int index_search_mmr_within(sqe_index* idx, const float* q_dev, int B, int k, int n, const float* lam_dev, const RowSet& set,
                            float* cos_dev, int64_t* id_dev, float* mmr_dev, hipStream_t s);

// ---- field aggregations (aggregate.hip)
void aggregate_destroy(AggState* a);
// A shard of a device group: the stats of every aggregation over the shard's own rows and ALL of its buckets on the host -- a
// histogram's counters from bucket `base` on in order (skipped: more than 16,384, which the group's histogram then has too), a
// TERMS aggregation's (value, count) pairs in no order.  set: the shard's row set, a host list if any.  More than
// AGG_GROUP_MAX_DISTINCT distinct values of a TERMS field: SQE_ERR_UNSUPPORTED.  Caller holds the shard's lock; synchronises s.
constexpr int64_t AGG_GROUP_MAX_DISTINCT = 65536;
// floor((v - offset) / interval) for interval >= 1, 0 <= offset < interval and v > INT64_MIN, without an intermediate that wraps
__host__ __device__ inline int64_t agg_bucket(int64_t v, int64_t interval, int64_t offset) {
    int64_t q = v / interval, r = v % interval;
    if (r < 0) {
        q -= 1;
        r += interval;
    }
    return r >= offset ? q : q - 1;
}
// the key of a bucket, bucket * interval + offset, in two's complement (it leaves int64 only where the lowest bucket starts below it)
__host__ __device__ inline int64_t agg_bucket_key(int64_t bucket, int64_t interval, int64_t offset) {
    return (int64_t)((uint64_t)bucket * (uint64_t)interval + (uint64_t)offset);
}
struct AggShardAgg {
    int64_t count = 0, min = INT64_MAX, max = INT64_MIN, sum_lo = 0, sum_hi = 0, base = 0;
    bool skipped = false;
    std::vector<int64_t> keys, counts;
};
struct AggShardResult {
    int64_t selected = 0;
    AggShardAgg agg[8];
};
int index_aggregate_shard(sqe_index* sh, const RowSet& set, const sqe_field_agg_t* aggs, int n_aggs, AggShardResult* out, hipStream_t s);

// ---- field sorts (sort.hip)
constexpr int SORT_MAX_FAN_IN = 64;     // x 256 rows = the 16,384 tuples one merge workgroup ranks
void sort_destroy(SortState* s);
// sqe_index_sort_fields over one index or one shard of a device group: the ids that go out, and that the cursor's after_id is
// compared with, are local id * id_mul + id_add (a single index: 1, id_base; shard p of P: P, p + the group's id_base).
// set: the row set, a host list if any.  Arguments validated by the caller; outputs on the host as sqe_index_sort_fields writes
// them.  Caller holds the index's lock; synchronises s once.
int index_sort_shard(sqe_index* sh, const RowSet& set, const sqe_field_sort_t* sort, int n_sort, int k, const int64_t* after_values,
                     int64_t after_id, int64_t id_mul, int64_t id_add, int64_t* total_out, int64_t* id_out, int64_t* value_out, hipStream_t s);

// ---- per-query filtered searches (filter_each.hip); caller holds the index lock and has validated the host arrays, stream s.
// offsets [n_lists + 1] and list_of_query [B] are host memory.  The direct route synchronises nothing; a list on the gathered
// route costs the one synchronisation of index_search_filtered_impl.  The host_ids form synchronises s before it returns.
constexpr int64_t FILTER_EACH_MIN_KEY_BUDGET = 4096;
int index_search_filtered_each_impl(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* allow_dev, const int64_t* offsets,
                                    int n_lists, const int32_t* list_of_query, float* cos_out_dev, int64_t* id_out_dev, hipStream_t s);
int index_search_filtered_each_host_ids(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* allow_host, const int64_t* offsets,
                                        int n_lists, const int32_t* list_of_query, float* cos_out_dev, int64_t* id_out_dev, hipStream_t s);
void filter_each_destroy(FilterEachState* f);
// rows of row_bytes (a multiple of 4): dst row j = src row idx[j], or with scatter dst row idx[j] = src row j
int launch_each_rows(const void* src, void* dst, const int* idx, int rows, int row_bytes, int scatter, hipStream_t s);

// ---- radial searches (range.hip); caller holds the index lock, stream s.  min_cos_dev holds no NaN (checked by the entry
// points).  Outputs on the device: counts [B], cos / ids [B, m] (ids as sqe_index_search returns them).
// bits (within.hip): a map of the filtered search's layout over the index as it stands; only rows whose bit is set count and are
// returned (null: every row).  walked_out (may be null): the queries whose candidates overflowed the buffer and took the walk.
int index_range_search_impl(sqe_index* idx, const float* q_dev, int B, const float* min_cos_dev, int m, int64_t* count_dev,
                            float* cos_dev, int64_t* id_dev, hipStream_t s, const uint32_t* bits = nullptr, int64_t* walked_out = nullptr);
void range_destroy(RangeState* r);
// device groups: P parts (RangePart, shard-local ids) -> the merged counts / cos / global ids
int launch_range_merge_parts(const char* parts, int P, int B, int m, int64_t id_base, int64_t* counts, float* cos, int64_t* ids,
                             hipStream_t s);

// ---- group keys and collapsed searches (collapse.hip); caller holds the index lock, stream s
int launch_fill_i64(int64_t* p, int64_t n, int64_t value, hipStream_t s);
int index_ensure_keys(sqe_index* idx, hipStream_t s);      // the key array, all SQE_KEY_NONE, if the index has none yet
// keys_host[j] to the row at pos[j] (the last of a repeated position wins) / the keys of the rows at pos[j]; both synchronise s
int index_set_keys_at(sqe_index* idx, const std::vector<int64_t>& pos, const int64_t* keys_host, hipStream_t s);
int index_get_keys_at(sqe_index* idx, const std::vector<int64_t>& pos, int64_t* keys_out_host, hipStream_t s);
// Outputs on the device: cos / ids / keys [B, k] (ids as sqe_index_search returns them).  Synchronises s once after the first
// stage and once per row range of the sweep.
// bits (within.hip): a map of the filtered search's layout over the index as it stands; the ranking walked is that of the rows
// whose bit is set (null: every row), and the first stage fetches `depth` rows (0: collapse_depth_of).
int index_search_collapsed_impl(sqe_index* idx, const float* q_dev, int B, int k, float* cos_dev, int64_t* id_dev, int64_t* key_dev,
                                hipStream_t s, const uint32_t* bits = nullptr, int depth = 0);
int collapse_depth_of(const sqe_index* idx, int k);      // rows the first stage fetches: "collapse_depth", automatic min(256, max(64, 4 k))
int launch_keys_gather(const int64_t* tab, const int64_t* pos, int64_t* out, int64_t m, hipStream_t s);   // out[j] = tab[pos[j]]
void collapse_destroy(CollapseState* c);
// the search over row POSITIONS (+ search_id_base) that index_search_impl translates to ids (search.hip)
int index_search_positions(sqe_index* idx, const float* q_dev, int B, int k, int nprobe, float* cos_out_dev, int64_t* id_out_dev,
                           hipStream_t s);
// device groups: P parts (CollapsePart, shard-local ids) -> the merged cos / global ids / keys
int launch_collapse_merge_parts(const char* parts, int P, int B, int k, int64_t id_base, float* cos, int64_t* ids, int64_t* keys,
                                hipStream_t s);

// ---- the sweep (sweep.hip): the walk over row ranges that radial, collapsed and exclusion search share; caller holds the index
// lock, stream s.  Every feature state embeds its own SweepBufs.
constexpr int SWEEP_MAX_PASS = 1024;    // queries normalised at once (larger batches run in passes, as search)
struct SweepBufs {
    DevBuf qn;         // [SWEEP_MAX_PASS, dim] fp32 normalised queries of the pass
    DevBuf qb;         // [SWEEP_MAX_PASS (+ 256: radial)] bf16 query rows of the pass at the index pitch
    DevBuf q_resid;    // [SWEEP_MAX_PASS]
    DevBuf qb_h;       // [G + 256] bf16 rows of the swept slots (the collect scan reads whole query blocks)
    DevBuf thr;        // [G] collect thresholds
    DevBuf kth;        // [G] k-th cosine of the running list (-inf: shorter than k); not radial
    DevBuf lcnt;       // [G] entries of the running list; not radial
    DevBuf keys;       // [G, EXACT_CAP] u64
    DevBuf key_cnt;    // [SWEEP_MAX_PASS] int, then the batch size (the collect scan reads it from the device)
    DevBuf qidx;       // slot -> query of its pass: [SWEEP_MAX_PASS] (radial), [passes * SWEEP_MAX_PASS] (sweep_flagged)
    DevBuf pass_cnt;   // [passes] slots of each pass (sweep_flagged)
    DevBuf dummy;      // candidate / bound pointers of the collect launch (COLLECT mode never reads or writes them)
    // everything but qidx's passes and pass_cnt, for B queries in groups of G slots; qb_h (and the radial qb) zeroed when they grow
    int ensure(sqe_index* idx, int B, int G, bool radial, hipStream_t s);
};
int sweep_slots_of(const sqe_index* idx);      // G: slots per sweep group = range_key_budget / EXACT_CAP, 1 to SWEEP_MAX_PASS
// the COLLECT-mode bf16 scan of G slots (bf16 rows qb_h, thresholds thr) over rows [r0, r1): keys [G, EXACT_CAP] relative to r0;
// key_cnt [SWEEP_MAX_PASS + 4]: the counts, then the batch size the scan reads from the device; dummy: 256 B the mode never touches
int launch_sweep_collect(sqe_index* idx, const bf16_t* qb_h, const float* thr, uint64_t* keys, int* key_cnt, void* dummy, int G, int64_t r0,
                         int64_t r1, hipStream_t s);
// the flagged queries (all of them with null flags) of every pass of SWEEP_MAX_PASS into dense slots
// qidx[pass * SWEEP_MAX_PASS + slot] = query of the pass, pass_cnt[pass] = their number
int launch_sweep_compact(const int* flags, int B, int* qidx, int* pass_cnt, hipStream_t s);
// The walk of the hs slots prepared in b (qb_h, thr, key_cnt) over all live rows, the first range L0 rows long: collect, read the
// counts back (one synchronisation of s per range), halve and collect again if a slot holds more than cap keys, else merge(r0)
// -- the feature's merge kernel over b.keys / b.key_cnt, rows relative to r0, under its StageTimer -- and double the range
// after one of at most cap / 4 keys.
using SweepMerge = std::function<int(int64_t r0)>;
int sweep_walk(sqe_index* idx, SweepBufs& b, int hs, int64_t L0, int cap, const SweepMerge& merge, hipStream_t s);
// Stage B of collapsed and exclusion search: compacts the flagged queries, reads their number per pass back (one synchronisation),
// stores the total in swept_out, then per pass normalises the queries and, per group of G slots, resets the slots (their rows of
// cos / pos / keys [B, k] to padding; keys may be null) and walks them from EXACT_CAP / 2 rows.  merge gets the pass's first
// query `off`, the group's slot -> query table and size, and the range's first row.
using SweepPassMerge = std::function<int(int off, const int* qidx, int hs, int64_t r0)>;
int sweep_flagged(sqe_index* idx, SweepBufs& b, const int* flags, const float* q_dev, int B, int k, float* cos, int64_t* pos, int64_t* keys,
                  std::atomic<int64_t>& swept_out, const SweepPassMerge& merge, hipStream_t s);

// ---- exclusion searches (exclude.hip); caller holds the index lock and has validated the host arrays, stream s.  deny ids of all
// lists on the device (local ids); offsets [n_lists + 1] and list_of_query [B] (-1: no list) on the host.  Synchronises s once
// after the first stage and once per row range of the sweep; the host_ids form stages the ids in the state's own buffer.
int index_search_excluding_impl(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* deny_dev, const int64_t* offsets,
                                int n_lists, const int32_t* list_of_query, float* cos_out_dev, int64_t* id_out_dev, hipStream_t s);
int index_search_excluding_host_ids(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* deny_host, const int64_t* offsets,
                                    int n_lists, const int32_t* list_of_query, float* cos_out_dev, int64_t* id_out_dev, hipStream_t s);
void exclude_destroy(ExcludeState* e);

// ---- MMR searches (mmr.hip); caller holds the index lock, stream s.  lam_dev [B] holds values in [0, 1] (checked by the
// entry points), 1 <= k <= n <= 256.  Outputs on the device: cos / ids / mmr [B, k] in selection order.  Nothing synchronises.
constexpr int MMR_MAX_N = 256;
int mmr_depth_of(int k, int n_cand);                     // n_cand == 0: automatic min(256, max(32, 4 k))
int mmr_pass_queries(int64_t row_budget, int n, int P);  // queries per pass: budget / (n P), at least 1
// set (may be null; within.hip): the candidates are the exact top-n of that row set, index_search_where_impl at depth n, which
// synchronises s per pass
int index_search_mmr_impl(sqe_index* idx, const float* q_dev, int B, int k, int n, const float* lam_dev, int nprobe, float* cos_dev,
                          int64_t* id_dev, float* mmr_dev, hipStream_t s, const RowSet* set = nullptr);
// device groups, on a shard: its top-n (cosines, shard-local ids, -1 padded) and the fp32 rows of those candidates
int index_mmr_candidates_impl(sqe_index* idx, const float* q_dev, int B, int n, int nprobe, float* cos_dev, int64_t* id_dev,
                              float* rows_dev, hipStream_t s, const RowSet* set = nullptr);
// device groups, on the leader: P parts (MmrPart) -> the global top-n, the Gram product over the gathered rows, the choice
int mmr_merge_parts(sqe_index* idx, const char* parts, int P, int B, int k, int n, const float* lam_dev, float* cos_dev,
                    int64_t* id_dev, float* mmr_dev, hipStream_t s);
void mmr_destroy(MmrState* m);

// ---- fused multi-query searches (fuse.hip); caller holds the index lock and has validated every argument (n is the resolved
// depth, Bs = offsets[G]), stream s.  offsets [G + 1] and weights [Bs] (null: all 1; RRF only) are host memory.  Outputs on the
// device: fused / ids / cos [G, k].  Nothing synchronises.
constexpr int FUSE_MAX_N = 256;          // depth of a list
constexpr int FUSE_MAX_LISTS = 32;       // sub-queries of a logical query
constexpr int FUSE_MAX_ENTRIES = 2048;   // sub-queries x depth of a logical query
int fuse_depth_of(int k, int n, int mode);               // n == 0: automatic, k (MAX) or min(256, max(32, 4 k)) (RRF)
int index_search_fused_impl(sqe_index* idx, const float* q_dev, int G, int Bs, const int64_t* offsets, int k, int n, int mode, int c,
                            const float* weights, int nprobe, float* fused_dev, int64_t* id_dev, float* cos_dev, hipStream_t s);
// the two halves a group leader uses: scratch for [Bs, n] hits, and the fuse kernel over hits that lie on this device
int fuse_hits(sqe_index* idx, int Bs, int n, float** cos, int64_t** ids);
// lx (hybrid search, RRF only): one more list per group, lx->score / lx->ids [G, lx->n] on this device; weights then holds
// Bs + G entries, the groups' lexical weights last, and lx->out [G, k] gets each row's lexical score (-inf: not in that list)
struct FuseLex {
    const float* score;
    const int64_t* ids;
    int n;
    float* out;
};
int fuse_lists(sqe_index* idx, const float* cos, const int64_t* ids, int G, int Bs, const int64_t* offsets, int k, int n, int mode, int c,
               const float* weights, float* fused_dev, int64_t* id_dev, float* cos_dev, hipStream_t s, const FuseLex* lx = nullptr);
// scratch for the [G, n] lists of the lexical side of a hybrid search
int fuse_lex_hits(sqe_index* idx, int G, int n, float** score, int64_t** ids);
void fuse_destroy(FuseState* f);

// ---- lexical index (lexical.hip)
sqe_ctx* lex_ctx(sqe_lex* lex);
// the checks of B lexical queries (offsets start at 0 and do not decrease, at most 64 occurrences each, terms in range)
int lex_query_check(const char* who, sqe_lex* lex, const int64_t* qoff, const int32_t* qterms, int B);
// sqe_lex_search_device on stream s for a caller that holds another object's lock: takes the lexical index's lock, orders s after
// the index's previous operation and records its event.  Arguments validated by the caller.
int lex_search_on_stream(sqe_lex* lex, const int64_t* qoff, const int32_t* qterms, int B, int k, float* score_dev, int64_t* id_dev,
                         hipStream_t s);

// ---- device groups (group.hip): n_dev > 1 contexts, one shard per member device
int group_create(sqe_ctx* leader, const int* device_ids, int n, int exchange);
void group_destroy(sqe_ctx* leader);
int group_index_create(sqe_ctx* leader, int dim, int kind, int nlist, sqe_index** out);
void group_index_destroy(sqe_index* idx);
int group_index_reserve(sqe_index* idx, int64_t rows);
int group_index_add(sqe_index* idx, const float* x, int64_t n, bool x_on_device, bool restore);
int group_index_update(sqe_index* idx, const int64_t* rows_host, const float* x_host, int64_t n);
int group_index_count(const sqe_index* idx, int64_t* out);
int group_index_get_rows(sqe_index* idx, const int64_t* rows_host, int64_t n, float* out_host);
int group_index_set_option(sqe_index* idx, const char* key, double value);
// allow_host / n_allow >= 0: the filtered search over the allowed GLOBAL ids (n_allow < 0: unfiltered)
int group_index_search(sqe_index* idx, const float* q, int B, int k, int nprobe, float* cos_out, int64_t* id_out, bool on_device,
                       const int64_t* allow_host = nullptr, int64_t n_allow = -1);
// per-query filtered search over GLOBAL ids; allow_host, offsets_host [n_lists + 1] and list_of_query_host [B] on the host in both forms
int group_index_search_filtered_each(sqe_index* idx, const float* q, int B, int k, const int64_t* allow_host, const int64_t* offsets_host,
                                     int n_lists, const int32_t* list_of_query_host, float* cos_out, int64_t* id_out, bool on_device);
// radial search; min_cos_host [B] on the host in both forms (the _device form reads it back first)
// exclusion search over GLOBAL deny ids; the three host arrays on the host in both forms
int group_index_search_excluding(sqe_index* idx, const float* q, int B, int k, const int64_t* deny_host, const int64_t* offsets_host,
                                 int n_lists, const int32_t* list_of_query_host, float* cos_out, int64_t* id_out, bool on_device);
// set (may be null: unrestricted) in these and the three below that take one: every shard restricts its own rows; the allow-list
// holds GLOBAL ids on the host
int group_index_range_search(sqe_index* idx, const float* q, int B, const float* min_cos_host, int m, int64_t* count_out, float* cos_out,
                             int64_t* id_out, bool on_device, const RowSet* set = nullptr);
int group_index_set_keys(sqe_index* idx, const int64_t* ids_host, const int64_t* keys_host, int64_t n);
int group_index_get_keys(sqe_index* idx, const int64_t* ids_host, int64_t n, int64_t* keys_out_host);
int group_index_search_collapsed(sqe_index* idx, const float* q, int B, int k, float* cos_out, int64_t* id_out, int64_t* key_out,
                                 bool on_device, const RowSet* set = nullptr);
// numeric fields: ids are routed as for the keys; a predicate names no id, so every shard evaluates it over its own rows
int group_index_set_field(sqe_index* idx, int field, const int64_t* ids_host, const int64_t* values_host, int64_t n);
int group_index_get_field(sqe_index* idx, int field, const int64_t* ids_host, int64_t n, int64_t* values_out_host);
int group_index_field_info(sqe_index* idx, int* n_fields, int64_t* bytes);
int group_index_match_fields(sqe_index* idx, const FieldPreds& pr, int64_t cap, int64_t* count_out, int64_t* id_out, bool on_device);
int group_index_search_where(sqe_index* idx, const float* q, int B, int k, const RowSet& set, float* cos_out, int64_t* id_out, bool on_device);
int group_index_search_where_each(sqe_index* idx, const float* q, int B, int k, const FieldPreds& pr, const int32_t* pred_of_query,
                                  float* cos_out, int64_t* id_out, bool on_device);
// field aggregations: every shard aggregates its own rows of `set` and the host merges exactly; arguments validated by the caller,
// outputs as sqe_index_aggregate_fields
int group_index_aggregate_fields(sqe_index* idx, const RowSet& set, const sqe_field_agg_t* aggs, int n_aggs, int64_t bucket_cap,
                                 int64_t* selected_out, sqe_field_agg_result_t* result_out, int64_t* key_out, int64_t* count_out);
// field sort: every shard sorts its own rows of `set` and returns its k best with global ids and its count; the host merges
// exactly; arguments validated by the caller, outputs as sqe_index_sort_fields
int group_index_sort_fields(sqe_index* idx, const RowSet& set, const sqe_field_sort_t* sort, int n_sort, int k, const int64_t* after_values,
                            int64_t after_id, int64_t* total_out, int64_t* id_out, int64_t* value_out);
// lam_host [B] on the host in both forms
int group_index_search_mmr(sqe_index* idx, const float* q, int B, int k, int n, const float* lam_host, int nprobe, float* cos_out,
                           int64_t* id_out, float* mmr_out, bool on_device, const RowSet* set = nullptr);
// offsets_host [G + 1] and weights_host [Bs] (or null) on the host in both forms; n is the resolved depth, Bs = offsets_host[G].
// hy (hybrid search, RRF): the lexical index -- it lives on the leader -- and the groups' lexical queries (host memory); its
// lists join the fuse kernel of the merge step, weights_host then holds Bs + G entries and hy->lex_out gets the lexical scores
struct GroupHybrid {
    sqe_lex* lex;
    const int64_t* qoff;
    const int32_t* qterms;
    float* lex_out;
};
int group_index_search_fused(sqe_index* idx, const float* q, int G, int Bs, const int64_t* offsets_host, int k, int n, int mode, int c,
                             const float* weights_host, int nprobe, float* fused_out, int64_t* id_out, float* cos_out, bool on_device,
                             const GroupHybrid* hy = nullptr);
int group_index_save_rows(sqe_index* idx, FILE* f, void* pinned, size_t pinned_bytes);
int group_index_delete(sqe_index* idx, const int64_t* ids_host, int64_t n);
int group_index_ids(sqe_index* idx, int64_t* ids_out, int64_t cap);
int group_index_ids_vec(sqe_index* idx, std::vector<int64_t>& out);         // live global ids (without id_base), ascending
// sqe_index_load of a file with holes: n rows in ascending id order, ids[n] global, routed by id
int group_index_load_rows(sqe_index* idx, FILE* f, int64_t n, const int64_t* ids, int64_t next_id, void* pinned, size_t pinned_bytes);
int group_index_train(sqe_index* idx, const float* x, int64_t n, int iters, uint64_t seed, bool x_on_device);
int group_index_ivf_export(sqe_index* idx, float* centroids_host, int32_t* assign_host);
bool group_index_ivf_trained(sqe_index* idx);
int group_index_ivf_restore(sqe_index* idx, const float* centroids_host, const int32_t* assign_host, int64_t n, const int64_t* ids = nullptr);
int group_describe(sqe_ctx* leader, int* n_shards, int* exchange, int* device_ids, int cap);
int group_member_count(const sqe_ctx* leader);          // shards of the context (1 without a group)
sqe_ctx* group_member(sqe_ctx* leader, int p);          // member context p (0 = the leader itself)

}  // namespace sqe
