// group.hip -- one host process driving several MI355X: the multi-device form of the context.
//
// The reference is ONE uvicorn process (main.py:738-739) that calls add_embeddings from a pool thread and search
// on the event loop; a drop-in OpenSearchIndexer therefore needs all the GPUs of the node behind one handle:
// sqe_create(device_ids, n_dev > 1) returns a context that leads a GROUP of member contexts, one per device,
// and every flat index created on it is sharded over them.
//
//   * Placement.  Global row g lives on shard g % P as its local row g / P (P = shards): appends stay balanced to
//     within one row whatever the call sizes, a row is located without a table, and an append of n rows is one
//     strided view per shard (host: hipMemcpy2DAsync, device: the normalise kernel reads every P-th row over xGMI).
//   * Search.  The query batch goes to every device (host -> each device, or leader -> peers by
//     hipMemcpyPeerAsync); each shard runs the whole single-device pipeline on its own stream; ONE exchange of
//     the packed [B, k] results (ids int64 | cosines fp32: 120 KB per shard at B = 1024, k = 10 -- latency-bound,
//     so a single step): RCCL ncclAllGather inside one ncclGroupStart/End over a communicator per device
//     (ncclCommInitAll -- single process, many devices), or peer copies to the leader where RCCL is not
//     available / the shards are logical shards of one device; then the merge kernel on the leader maps
//     shard-local ids to global ones (local * P + shard) and keeps the best k, ties to the lowest global id.
//     Top-k, filtered, radial and collapsed searches all run through group_search: a SearchKind names the part size, the
//     shard call and the merge; the five steps around them (query hand-over, delivery, fan-out, exchange, host tail) and
//     the per-shard buffers (GroupIndex::qbuf / gather / out) exist once.  Part layouts: internal.h.
//   * RCCL is loaded with dlopen at group creation (librccl.so.1): single-device users never map it, and a
//     process that already holds RCCL through torch shares that copy.
//
//   * Deletes.  Placement stays by id: global id g lives on shard g % P, whose id map (compact.hip) stores the local id
//     g / P.  A shard's search translates its positions to those local ids, so the merge above turns them into global
//     ids unchanged.  Adds route by the group's next_id; delete / update / get_rows / set_keys / get_keys route id g to
//     shard g % P (route_ids) and resolve every id on its shard before any shard writes (resolve_all).
//
// P logical shards may share one device (device_ids = {0, 0, 0}): the same code path, with the copy
// exchange -- that is how the one-GPU test box rehearses it.  IVF indexes are not sharded by this layer.
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <functional>
#include <memory>
#include <new>
#include <thread>

#include "fieldsort.h"
#include "internal.h"

namespace sqe {

namespace {

// ---- the handful of RCCL entry points, resolved at run time
typedef void* rccl_comm_t;
struct Rccl {
    void* lib = nullptr;
    int (*CommInitAll)(rccl_comm_t*, int, const int*) = nullptr;
    int (*CommDestroy)(rccl_comm_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, rccl_comm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool load() {
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (lib) break;
        }
        if (!lib) return false;
        CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
        AllGather = (decltype(AllGather))dlsym(lib, "ncclAllGather");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        return CommInitAll && CommDestroy && GroupStart && GroupEnd && AllGather;
    }
};
constexpr int RCCL_CHAR = 0;      // ncclInt8 / ncclChar

}  // namespace

// One enqueue thread per member beyond the leader (r03, r02 verdict item 8): a search enqueues ~15 launches, copies and
// events per shard; from ONE host thread that was 0.46 ms for 8 shards of 1.25 M rows -- a fifth of one shard's 2.3 ms step
// (profiles/r03_configs/group_host_cost.jsonl), and on P real GPUs the last shard would start that much late.  The
// calling thread keeps shard 0; worker p sets its device once and runs shard p's closure; errors come back with their text
// (sqe_last_error is thread-local).
struct ShardWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<int()> task;
    bool has_task = false, done = false, stop = false;
    int rc = SQE_OK;
    std::string err;
    int dev = 0;
    void loop() {
        (void)hipSetDevice(dev);
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return has_task || stop; });
            if (stop) return;
            std::function<int()> fn = std::move(task);
            has_task = false;
            lk.unlock();
            const int r = fn();
            std::string e = r == SQE_OK ? std::string() : std::string(sqe_last_error());
            lk.lock();
            rc = r;
            err = std::move(e);
            done = true;
            cv.notify_all();
        }
    }
    void post(std::function<int()> fn) {
        std::lock_guard<std::mutex> lk(mu);
        task = std::move(fn);
        has_task = true;
        done = false;
        cv.notify_all();
    }
    int wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done; });
        if (rc != SQE_OK) set_error(err);
        return rc;
    }
};

struct Group {
    int P = 0;
    std::vector<std::unique_ptr<ShardWorker>> workers;   // [P - 1]: worker p - 1 enqueues for member p
    std::vector<int> devs;
    std::vector<sqe_ctx*> members;        // members[0] is the leader itself
    std::vector<char> peer_ok;            // leader memory is directly addressable from member p
    int exchange = SQE_EXCHANGE_COPY;     // resolved mode
    Rccl rccl;
    std::vector<rccl_comm_t> comms;
    std::mutex coll_mu;                   // RCCL group calls of one process must not interleave
    std::mutex fan_mu;                    // the workers have ONE task slot each: a fan-out holds this from its first post() to its last
                                          // wait() (two indexes of one context searched from two threads share the workers; their
                                          // per-index locks do not exclude each other)
};

struct GroupIndex {
    std::vector<sqe_index*> shards;
    // per shard, on its device
    // qbuf: the shard's copy of the queries (and thresholds) of a search; gather: its result part (the leader's: all P parts);
    // every kind of search uses them, sized by its last ensure().  stage: rows on their way in (add, update, load, train)
    std::vector<std::unique_ptr<DevBuf>> qbuf, gather, stage;
    std::vector<hipEvent_t> ev;           // shard p's part is in the leader's gather buffer / its search is done
    hipEvent_t ev_q = nullptr;            // the leader's query batch is ready to be copied to the peers
    DevBuf out;                           // leader: the merged result of a host entry point, laid out as one part
};

namespace {

int64_t shard_rows_of(int64_t n_total, int P, int p) { return (n_total - p + P - 1) / P; }   // rows g < n_total with g % P == p

// scopes of one group operation: the group index lock, then every shard's OpScope (device p, its stream)
struct GroupScope {
    sqe_index* gi;
    std::vector<std::unique_ptr<OpScope>> ops;
    GroupScope(sqe_index* idx, bool host_call) : gi(idx) {
        gi->ord.mu.lock();
        Group* g = idx->ctx->group;
        for (int p = 0; p < g->P; ++p)
            ops.emplace_back(new OpScope(g->members[p], idx->group->shards[p]->ord, p == 0 ? host_call : true));
    }
    hipStream_t s(int p) const { return ops[p]->s; }
    ~GroupScope() {
        Group* g = gi->ctx->group;
        for (int p = g->P - 1; p >= 0; --p) {
            (void)hipSetDevice(g->devs[p]);
            ops[p].reset();
        }
        (void)hipSetDevice(g->devs[0]);
        gi->ord.mu.unlock();
    }
};

int sync_all(const GroupScope& sc, Group* g) {
    for (int p = 0; p < g->P; ++p) {
        SQE_HIP(hipSetDevice(g->devs[p]));
        SQE_HIP(hipStreamSynchronize(sc.s(p)));
    }
    SQE_HIP(hipSetDevice(g->devs[0]));
    return SQE_OK;
}

// Routing by id: global id g lives on shard g % P as its local id g / P.  Splits ids[n] into local[p]; with `which`,
// which[p][j] is the input index of local[p][j].  Ids outside [0, next_id) name no row.
typedef std::vector<std::vector<int64_t>> PerShard;
int route_ids(const sqe_index* idx, const int64_t* ids, int64_t n, const char* fn, PerShard& local, PerShard* which = nullptr) {
    const int P = idx->ctx->group->P;
    const int64_t total = idx->next_id.load();
    local.assign(P, {});
    if (which) which->assign(P, {});
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = ids[i];
        if (id < 0 || id >= total) return fail(SQE_ERR_INVALID, std::string(fn) + ": id " + std::to_string(id) + " is not in the index");
        local[id % P].push_back(id / P);
        if (which) (*which)[id % P].push_back(i);
    }
    return SQE_OK;
}

// The id lists of a search the same way: entries [offsets[f], offsets[f + 1]) of ids are list f, and every shard gets the same
// n_lists lists with its own offsets.  Unlike route_ids, an id outside [0, next_id) is no error here: it names no row and is
// silently dropped, as a deleted id is by the shard.
void route_lists(const sqe_index* idx, const int64_t* ids, const int64_t* offsets, int n_lists, PerShard& ids_local, PerShard& offs_local) {
    const int P = idx->ctx->group->P;
    const int64_t total = idx->next_id.load();
    ids_local.assign(P, {});
    offs_local.assign(P, {0});
    for (int f = 0; f < n_lists; ++f) {
        for (int64_t j = offsets[f]; j < offsets[f + 1]; ++j)
            if (ids[j] >= 0 && ids[j] < total) ids_local[ids[j] % P].push_back(ids[j] / P);
        for (int p = 0; p < P; ++p) offs_local[p].push_back((int64_t)ids_local[p].size());
    }
}

// local ids -> row positions, in place, on every shard: all of it is done (every id live) before the caller writes anything
int resolve_all(sqe_index* idx, const GroupScope& sc, PerShard& local, const char* fn) {
    Group* g = idx->ctx->group;
    for (int p = 0; p < g->P; ++p) {
        if (local[p].empty()) continue;
        SQE_HIP(hipSetDevice(g->devs[p]));
        std::vector<int64_t> pos;
        SQE_TRY(index_resolve_ids(idx->group->shards[p], local[p].data(), (int64_t)local[p].size(), pos, sc.s(p), fn));
        local[p].swap(pos);
    }
    return SQE_OK;
}

}  // namespace

// ================================================================ group lifetime
int group_create(sqe_ctx* leader, const int* device_ids, int n, int exchange) {
    if (n == 1 && exchange == SQE_EXCHANGE_AUTO) return SQE_OK;      // a plain single-device context
    int count = 0;
    SQE_HIP(hipGetDeviceCount(&count));
    std::unique_ptr<Group> g(new (std::nothrow) Group);
    if (!g) return fail(SQE_ERR_OOM, "sqe_create: host allocation failed");
    g->P = n;
    g->devs.assign(device_ids, device_ids + n);
    bool distinct = true;
    for (int i = 0; i < n; ++i) {
        if (device_ids[i] < 0 || device_ids[i] >= count) return fail(SQE_ERR_INVALID, "sqe_create: no such HIP device");
        for (int j = 0; j < i; ++j) distinct = distinct && device_ids[i] != device_ids[j];
    }
    g->members.push_back(leader);
    g->peer_ok.assign(n, 1);
    leader->group = g.get();       // from here on sqe_destroy(leader) releases the members
    Group* gp = g.release();
    for (int p = 1; p < n; ++p) {
        sqe_ctx* m = nullptr;
        const int one[1] = {device_ids[p]};
        SQE_TRY(sqe_create(one, 1, &m));
        gp->members.push_back(m);
        if (device_ids[p] != device_ids[0]) {
            int can = 0;
            (void)hipDeviceCanAccessPeer(&can, device_ids[p], device_ids[0]);
            bool ok = can != 0;
            if (ok) {
                SQE_HIP(hipSetDevice(device_ids[p]));
                hipError_t e = hipDeviceEnablePeerAccess(device_ids[0], 0);
                ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
                (void)hipGetLastError();
                SQE_HIP(hipSetDevice(device_ids[0]));
                e = hipDeviceEnablePeerAccess(device_ids[p], 0);
                ok = ok && (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled);
                (void)hipGetLastError();
            }
            gp->peer_ok[p] = ok ? 1 : 0;
        }
    }
    SQE_HIP(hipSetDevice(device_ids[0]));
    // exchange step: RCCL needs one communicator per DISTINCT device
    gp->exchange = SQE_EXCHANGE_COPY;
    if (exchange != SQE_EXCHANGE_COPY && distinct) {
        if (gp->rccl.load()) {
            gp->comms.assign(n, nullptr);
            const int rc = gp->rccl.CommInitAll(gp->comms.data(), n, gp->devs.data());
            if (rc == 0) gp->exchange = SQE_EXCHANGE_RCCL;
            else if (exchange == SQE_EXCHANGE_RCCL)
                return fail(SQE_ERR_HIP, std::string("ncclCommInitAll: ") + (gp->rccl.GetErrorString ? gp->rccl.GetErrorString(rc) : "failed"));
            else gp->comms.clear();
        } else if (exchange == SQE_EXCHANGE_RCCL) {
            return fail(SQE_ERR_UNSUPPORTED, "sqe_create_sharded: librccl.so.1 could not be loaded");
        }
        SQE_HIP(hipSetDevice(device_ids[0]));
    } else if (exchange == SQE_EXCHANGE_RCCL) {
        return fail(SQE_ERR_INVALID, "sqe_create_sharded: the RCCL exchange needs distinct devices (logical shards of one device use the copy exchange)");
    }
    for (int p = 1; p < n; ++p) {
        gp->workers.emplace_back(new ShardWorker);
        ShardWorker* w = gp->workers.back().get();
        w->dev = device_ids[p];
        w->th = std::thread([w] { w->loop(); });
    }
    return SQE_OK;
}

void group_destroy(sqe_ctx* leader) {
    Group* g = leader->group;
    if (!g) return;
    for (auto& w : g->workers) {
        {
            std::lock_guard<std::mutex> lk(w->mu);
            w->stop = true;
            w->cv.notify_all();
        }
        if (w->th.joinable()) w->th.join();
    }
    g->workers.clear();
    for (size_t p = 0; p < g->comms.size(); ++p)
        if (g->comms[p]) (void)g->rccl.CommDestroy(g->comms[p]);
    for (size_t p = 1; p < g->members.size(); ++p) sqe_destroy(g->members[p]);
    leader->group = nullptr;
    delete g;
}

int group_member_count(const sqe_ctx* leader) { return leader->group ? (int)leader->group->members.size() : 1; }
sqe_ctx* group_member(sqe_ctx* leader, int p) { return leader->group ? leader->group->members[p] : leader; }

int group_describe(sqe_ctx* leader, int* n_shards, int* exchange, int* device_ids, int cap) {
    Group* g = leader->group;
    if (n_shards) *n_shards = g->P;
    if (exchange) *exchange = g->exchange;
    for (int p = 0; device_ids && p < g->P && p < cap; ++p) device_ids[p] = g->devs[p];
    return SQE_OK;
}

// ================================================================ group index
int group_index_create(sqe_ctx* leader, int dim, int kind, int nlist, sqe_index** out) {
    *out = nullptr;
    Group* g = leader->group;
    if (kind != SQE_INDEX_FLAT && kind != SQE_INDEX_IVF_FLAT) return fail(SQE_ERR_INVALID, "sqe_index_create: unknown index kind");
    if (kind == SQE_INDEX_IVF_FLAT && (nlist < 1 || nlist > (1 << 20)))
        return fail(SQE_ERR_INVALID, "sqe_index_create: IVF needs 1 <= nlist <= 2^20");
    std::unique_ptr<sqe_index> idx(new (std::nothrow) sqe_index);
    std::unique_ptr<GroupIndex> gi(new (std::nothrow) GroupIndex);
    if (!idx || !gi) return fail(SQE_ERR_OOM, "sqe_index_create: host allocation failed");
    idx->ctx = leader;
    idx->dim = dim;
    idx->kind = kind;
    idx->nlist = kind == SQE_INDEX_IVF_FLAT ? nlist : 0;
    SQE_HIP(hipSetDevice(leader->device));
    SQE_TRY(idx->ord.init());
    SQE_HIP(hipEventCreateWithFlags(&gi->ev_q, hipEventDisableTiming));
    idx->group = gi.release();
    sqe_index* raw = idx.release();
    const int idx_nlist = raw->nlist;
    for (int p = 0; p < g->P; ++p) {
        sqe_index* sh = nullptr;
        // IVF: every shard is a complete IVF index over ITS rows with the same (replicated) centroids --
        // lists are sharded by the group's row ownership, the [B,k] exchange and the merge are the flat index's
        int rc = index_create_impl(g->members[p], dim, kind, idx_nlist, false, &sh);
        if (rc != SQE_OK) { group_index_destroy(raw); return rc; }
        raw->group->shards.push_back(sh);
        raw->group->qbuf.emplace_back(new DevBuf);
        raw->group->gather.emplace_back(new DevBuf);
        raw->group->stage.emplace_back(new DevBuf);
        hipEvent_t e = nullptr;
        (void)hipSetDevice(g->devs[p]);
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { group_index_destroy(raw); return fail(SQE_ERR_HIP, "hipEventCreate"); }
        raw->group->ev.push_back(e);
    }
    SQE_HIP(hipSetDevice(leader->device));
    raw->pitch = raw->group->shards[0]->pitch;
    *out = raw;
    return SQE_OK;
}

void group_index_destroy(sqe_index* idx) {
    if (!idx || !idx->group) return;
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    {
        std::lock_guard<std::mutex> lk(idx->ord.mu);
        for (size_t p = 0; p < gi->shards.size(); ++p) {
            (void)hipSetDevice(g->devs[p]);
            {
                std::lock_guard<std::mutex> lk2(gi->shards[p]->ord.mu);
                gi->shards[p]->ord.quiesce();
            }
            gi->qbuf[p].reset();
            gi->gather[p].reset();
            gi->stage[p].reset();
            if (p < gi->ev.size() && gi->ev[p]) (void)hipEventDestroy(gi->ev[p]);
            sqe_index_destroy(gi->shards[p]);
        }
        (void)hipSetDevice(g->devs[0]);
        if (gi->ev_q) (void)hipEventDestroy(gi->ev_q);
        gi->out.release();
        if (idx->mmr) { mmr_destroy(idx->mmr); idx->mmr = nullptr; }      // the leader's merge scratch
        if (idx->fuse) { fuse_destroy(idx->fuse); idx->fuse = nullptr; }  // the leader's merged hits and tables
    }
    idx->ord.destroy();
    delete gi;
    idx->group = nullptr;
    delete idx;
}

int group_index_reserve(sqe_index* idx, int64_t rows) {
    Group* g = idx->ctx->group;
    GroupScope sc(idx, true);
    for (int p = 0; p < g->P; ++p) {
        SQE_HIP(hipSetDevice(g->devs[p]));
        SQE_TRY(index_grow(idx->group->shards[p], shard_rows_of(rows, g->P, p), sc.s(p)));
    }
    return SQE_OK;
}

int group_index_count(const sqe_index* idx, int64_t* out) {
    int64_t n = 0;
    for (sqe_index* sh : idx->group->shards) n += sh->n.load();
    *out = n;
    return SQE_OK;
}

// Append n rows (ids next_id .. next_id + n - 1).  x: host block, or a device block on the LEADER device.
int group_index_add(sqe_index* idx, const float* x, int64_t n, bool x_on_device, bool restore) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P, dim = idx->dim;
    GroupScope sc(idx, !x_on_device);
    // placement is by id, not by the live count: global id total + i goes to shard (total + i) % P, where it gets the shard's
    // own next id (total + i) / P; shard p's first input row is i0 = (p - total) mod P
    const int64_t total = idx->next_id.load();
    if (x_on_device) {
        // the block is the caller's work on the leader's context stream (= sc.s(0)): the peers wait for it
        SQE_HIP(hipSetDevice(g->devs[0]));
        SQE_HIP(hipEventRecord(gi->ev_q, sc.s(0)));
    }
    for (int p = 0; p < P; ++p) {
        const int64_t i0 = ((p - total) % P + P) % P;
        const int64_t m = i0 < n ? (n - i0 + P - 1) / P : 0;
        if (m == 0) continue;
        sqe_index* sh = gi->shards[p];
        hipStream_t s = sc.s(p);
        SQE_HIP(hipSetDevice(g->devs[p]));
        if (x_on_device) {
            if (p > 0) SQE_HIP(hipStreamWaitEvent(s, gi->ev_q, 0));
            const float* src = x + i0 * dim;
            int64_t stride = (int64_t)P * dim;
            if (!g->peer_ok[p]) {
                // no direct access to the leader's memory: bring the block over, then take every P-th row locally
                SQE_TRY(gi->stage[p]->ensure((size_t)n * dim * 4));
                SQE_HIP(hipMemcpyPeerAsync(gi->stage[p]->p, g->devs[p], x, g->devs[0], (size_t)n * dim * 4, s));
                src = gi->stage[p]->as<float>() + i0 * dim;
            }
            SQE_TRY(index_add_impl(sh, src, m, stride, restore, s));
        } else {
            const int64_t rows_per_step = std::max<int64_t>(1, (64ll << 20) / ((int64_t)dim * 4));
            SQE_TRY(gi->stage[p]->ensure((size_t)std::min(rows_per_step, m) * dim * 4));
            for (int64_t off = 0; off < m; off += rows_per_step) {
                const int64_t mm = std::min(rows_per_step, m - off);
                SQE_HIP(hipMemcpy2DAsync(gi->stage[p]->p, (size_t)dim * 4, x + (i0 + off * P) * dim, (size_t)P * dim * 4,
                                         (size_t)dim * 4, (size_t)mm, hipMemcpyHostToDevice, s));
                SQE_TRY(index_add_impl(sh, gi->stage[p]->as<float>(), mm, dim, restore, s));
            }
        }
    }
    idx->next_id.fetch_add(n);
    if (!x_on_device) SQE_TRY(sync_all(sc, g));           // x is not retained past return
    else {
        // the caller may reuse its block once the leader's stream says so: order the peers' reads before that
        for (int p = 1; p < P; ++p) {
            SQE_HIP(hipSetDevice(g->devs[p]));
            SQE_HIP(hipEventRecord(gi->ev[p], sc.s(p)));
            SQE_HIP(hipSetDevice(g->devs[0]));
            SQE_HIP(hipStreamWaitEvent(sc.s(0), gi->ev[p], 0));
        }
    }
    return SQE_OK;
}

int group_index_update(sqe_index* idx, const int64_t* rows_host, const float* x_host, int64_t n) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P, dim = idx->dim;
    GroupScope sc(idx, true);
    PerShard local;
    SQE_TRY(route_ids(idx, rows_host, n, "sqe_index_update", local));
    std::vector<std::vector<float>> xs(P);
    for (int64_t i = 0; i < n; ++i) {
        std::vector<float>& dst = xs[rows_host[i] % P];
        dst.insert(dst.end(), x_host + i * dim, x_host + (i + 1) * dim);
    }
    SQE_TRY(resolve_all(idx, sc, local, "sqe_index_update"));
    for (int p = 0; p < P; ++p) {
        const int64_t m = (int64_t)local[p].size();
        if (m == 0) continue;
        SQE_HIP(hipSetDevice(g->devs[p]));
        hipStream_t s = sc.s(p);
        const size_t xb = (size_t)m * dim * 4, rb = (size_t)m * 8;
        SQE_TRY(gi->stage[p]->ensure(xb + rb));
        SQE_HIP(hipMemcpyAsync(gi->stage[p]->p, xs[p].data(), xb, hipMemcpyHostToDevice, s));
        SQE_HIP(hipMemcpyAsync((char*)gi->stage[p]->p + xb, local[p].data(), rb, hipMemcpyHostToDevice, s));
        SQE_TRY(index_update_impl(gi->shards[p], (const int64_t*)((char*)gi->stage[p]->p + xb), gi->stage[p]->as<float>(), m, s));
    }
    return sync_all(sc, g);
}

int group_index_get_rows(sqe_index* idx, const int64_t* rows_host, int64_t n, float* out_host) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P, dim = idx->dim;
    GroupScope sc(idx, true);
    PerShard pos, which;
    SQE_TRY(route_ids(idx, rows_host, n, "sqe_index_get_rows", pos, &which));
    SQE_TRY(resolve_all(idx, sc, pos, "sqe_index_get_rows"));
    for (int p = 0; p < P; ++p) {
        if (pos[p].empty()) continue;
        SQE_HIP(hipSetDevice(g->devs[p]));
        for (size_t j = 0; j < pos[p].size(); ++j)
            SQE_HIP(hipMemcpyAsync(out_host + (size_t)which[p][j] * dim, gi->shards[p]->master + (size_t)pos[p][j] * dim, (size_t)dim * 4,
                                   hipMemcpyDeviceToHost, sc.s(p)));
    }
    return sync_all(sc, g);
}

int group_index_set_option(sqe_index* idx, const char* key, double value) {
    const std::string k(key);
    if (k == "id_base") {
        if (value < 0) return fail(SQE_ERR_INVALID, "id_base must be >= 0");
        std::lock_guard<std::mutex> lk(idx->ord.mu);
        idx->id_base = (int64_t)value;           // applied by the merge; shards return local ids
        return SQE_OK;
    }
    for (sqe_index* sh : idx->group->shards) SQE_TRY(sqe_index_set_option(sh, key, value));
    if (k == "certify") idx->certify = value != 0.0;
    if (k == "mmr_row_budget") idx->mmr_row_budget = (int64_t)value;      // the pass size of the group (validated by the shards)
    return SQE_OK;
}

// ---------------------------------------------------------------- IVF on a device group
// Training runs ONCE, on the leader's shard (k-means over the sample), and the normalised centroids are then
// replicated: every other shard takes them bit for bit (ivf_restore) and assigns its own rows.  All shards therefore
// probe the same lists in the same order, a shard scans the rows it owns of every probed list, and the merged result is
// the IVF search over the global lists.  x: the training sample, host or LEADER-device memory.
int group_index_train(sqe_index* idx, const float* x, int64_t n, int iters, uint64_t seed, bool x_on_device) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P, dim = idx->dim, nlist = idx->nlist;
    if (idx->kind != SQE_INDEX_IVF_FLAT) return fail(SQE_ERR_STATE, "sqe_index_train: not an IVF index");
    GroupScope sc(idx, !x_on_device);        // a device block is the caller's work on the leader's context stream (= sc.s(0))
    SQE_HIP(hipSetDevice(g->devs[0]));
    sqe_index* lead = gi->shards[0];
    {
        DevBuf tmp;
        const float* xd = x;
        if (!x_on_device) {
            SQE_TRY(tmp.ensure((size_t)n * dim * 4));
            SQE_HIP(hipMemcpyAsync(tmp.p, x, (size_t)n * dim * 4, hipMemcpyHostToDevice, sc.s(0)));
            xd = tmp.as<float>();
        }
        SQE_TRY(ivf_train(lead, lead->ivf, xd, n, iters, seed, sc.s(0)));
        SQE_HIP(hipStreamSynchronize(sc.s(0)));
    }
    // replicate: leader -> host -> every member (16 MB at nlist 4096 x 1024; once per training)
    const size_t cb = (size_t)nlist * dim * 4;
    std::vector<float> cent(cb / 4);
    SQE_HIP(hipMemcpyAsync(cent.data(), ivf_coarse(lead->ivf)->master, cb, hipMemcpyDeviceToHost, sc.s(0)));
    SQE_HIP(hipStreamSynchronize(sc.s(0)));
    for (int p = 1; p < P; ++p) {
        SQE_HIP(hipSetDevice(g->devs[p]));
        sqe_index* sh = gi->shards[p];
        SQE_TRY(gi->stage[p]->ensure(cb));
        SQE_HIP(hipMemcpyAsync(gi->stage[p]->p, cent.data(), cb, hipMemcpyHostToDevice, sc.s(p)));
        SQE_TRY(ivf_restore(sh, sh->ivf, gi->stage[p]->as<float>(), nullptr, 0, sc.s(p)));   // no assignments yet ...
        SQE_TRY(ivf_rows_added(sh, sh->ivf, sc.s(p)));                                          // ... the shard makes its own
    }
    return sync_all(sc, g);
}

// centroids [nlist, dim] (the leader's = everyone's) and the list of every stored row in GLOBAL row order
int group_index_ivf_export(sqe_index* idx, float* centroids_host, int32_t* assign_host) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P;
    if (idx->kind != SQE_INDEX_IVF_FLAT) return fail(SQE_ERR_STATE, "sqe_index_ivf_export: not an IVF index");
    GroupScope sc(idx, true);
    std::vector<int32_t> part;
    std::vector<std::pair<int64_t, int32_t>> by_id;        // (global id, list) once rows were deleted
    bool holes = false;
    for (sqe_index* sh : gi->shards) holes = holes || sh->has_map;
    for (int p = 0; p < P; ++p) {
        SQE_HIP(hipSetDevice(g->devs[p]));
        sqe_index* sh = gi->shards[p];
        const int64_t m = sh->n.load();
        part.resize((size_t)std::max<int64_t>(m, 1));
        SQE_TRY(ivf_export(sh, sh->ivf, p == 0 ? centroids_host : nullptr, assign_host ? part.data() : nullptr, sc.s(p)));
        if (assign_host && !holes)
            for (int64_t i = 0; i < m; ++i) assign_host[i * P + p] = part[(size_t)i];      // local row i of shard p = global row i * P + p
        if (assign_host && holes) {
            std::vector<int64_t> ids;
            SQE_TRY(index_ids_host(sh, ids, sc.s(p)));
            for (int64_t i = 0; i < m; ++i) by_id.emplace_back(ids[(size_t)i] * P + p, part[(size_t)i]);
        }
    }
    if (holes) {
        std::sort(by_id.begin(), by_id.end());              // the live rows in ascending global id
        for (size_t i = 0; i < by_id.size(); ++i) assign_host[i] = by_id[i].second;
    }
    return SQE_OK;
}

bool group_index_ivf_trained(sqe_index* idx) {
    return idx->kind == SQE_INDEX_IVF_FLAT && idx->group->shards[0]->ivf && ivf_trained(idx->group->shards[0]->ivf);
}

// sqe_index_load: centroids and the per-row assignment in GLOBAL row order (host) -> every shard's share
// (ids: the global id of every row of the file, ascending, when it has holes; null: row i is id i)
int group_index_ivf_restore(sqe_index* idx, const float* centroids_host, const int32_t* assign_host, int64_t n, const int64_t* ids) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P, dim = idx->dim, nlist = idx->nlist;
    GroupScope sc(idx, true);
    const size_t cb = (size_t)nlist * dim * 4;
    std::vector<int32_t> part;
    for (int p = 0; p < P; ++p) {
        SQE_HIP(hipSetDevice(g->devs[p]));
        sqe_index* sh = gi->shards[p];
        const int64_t m = sh->n.load();
        part.clear();
        if (ids) {
            for (int64_t i = 0; i < n; ++i)
                if (ids[i] % P == p) part.push_back(assign_host[i]);
        } else {
            for (int64_t i = 0; i < shard_rows_of(n, P, p); ++i) part.push_back(assign_host[i * P + p]);
        }
        if (m != (int64_t)part.size()) return fail(SQE_ERR_STATE, "sqe_index_load: shard sizes do not match the file");
        part.resize((size_t)std::max<int64_t>(m, 1));
        SQE_TRY(gi->stage[p]->ensure(cb + (size_t)std::max<int64_t>(m, 1) * 4));
        SQE_HIP(hipMemcpyAsync(gi->stage[p]->p, centroids_host, cb, hipMemcpyHostToDevice, sc.s(p)));
        SQE_HIP(hipMemcpyAsync(gi->stage[p]->as<char>() + cb, part.data(), (size_t)m * 4, hipMemcpyHostToDevice, sc.s(p)));
        SQE_TRY(ivf_restore(sh, sh->ivf, gi->stage[p]->as<float>(), (const int32_t*)(gi->stage[p]->as<char>() + cb), m, sc.s(p)));
        SQE_HIP(hipStreamSynchronize(sc.s(p)));           // `part` is reused
    }
    return SQE_OK;
}

// ---------------------------------------------------------------- searches: one driver, three kinds
// What a kind of search contributes; group_search does everything else.  A part is one shard's answer over its own rows
// with shard-local ids (layouts: internal.h); the merged result of a host call has the layout of one part.
namespace {

struct SearchKind {
    size_t part = 0;                  // bytes of one part
    size_t out_bytes = 0;             // bytes of a host call's merged result where it is not laid out as a part (0: a part)
    const void* extra = nullptr;      // host input every shard needs besides the queries (the radial search's thresholds) ...
    size_t extra_bytes = 0;           // ... delivered behind the queries in the shard's qbuf, 16-byte aligned
    bool all_gather = false;          // the parts may meet by the RCCL all-gather where the group has it
    // run shard p from these queries (and its copy of `extra`) into this part, on the shard's stream
    std::function<int(int p, const float* q_dev, const void* extra_dev, char* part, hipStream_t s)> run;
    // merge the P parts on the leader into dst[i] (the caller's out[i].ptr, or where the host call's copy of it starts)
    std::function<int(const char* parts, void* const* dst, hipStream_t s)> merge;
    struct Out { void* ptr; size_t off, bytes; } out[4] = {};   // caller's outputs: offset in a part's layout, bytes to copy back
};

// step(p) for every shard: shard 0 on the calling thread, shard p on worker p.  The workers have one task slot each, so
// fan_mu is held from the first post() to the last wait(); every posted closure has run before the caller's frame goes away.
template <typename Step>
int fan_out(Group* g, Step&& step) {
    static const bool serial = [] { const char* e = knob_env("SQE_GROUP_SERIAL"); return e && e[0] == '1'; }();   // knobs build: the r02 form, for A/B
    const int P = g->P;
    int rc = SQE_OK;
    if (serial || g->workers.size() != (size_t)(P - 1)) {
        for (int p = 0; p < P && rc == SQE_OK; ++p) rc = step(p);
    } else {
        std::lock_guard<std::mutex> fan(g->fan_mu);
        for (int p = 1; p < P; ++p) g->workers[p - 1]->post([&step, p] { return step(p); });
        rc = step(0);
        for (int p = 1; p < P; ++p) {
            const int r = g->workers[p - 1]->wait();
            if (rc == SQE_OK) rc = r;
        }
    }
    SQE_HIP(hipSetDevice(g->devs[0]));
    return rc;
}

// q: [B, dim] raw queries, host or LEADER-device memory; the outputs of `kind` likewise.  Host callers return with
// everything synchronised; device callers get their results in order on the leader's context stream (= sc.s(0)).
int group_search(sqe_index* idx, const float* q, int B, bool on_device, const SearchKind& kind) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P;
    const size_t qbytes = (size_t)B * idx->dim * 4, xoff = round16(qbytes), part = kind.part;
    const bool rccl = kind.all_gather && g->exchange == SQE_EXCHANGE_RCCL;
    GroupScope sc(idx, !on_device);
    if (on_device) {                  // the queries are the caller's work on the leader's context stream: the peers wait for it
        SQE_HIP(hipSetDevice(g->devs[0]));
        SQE_HIP(hipEventRecord(gi->ev_q, sc.s(0)));
    }
    // ---- every shard: queries in, its part into its slot of the gather buffer
    auto shard_step = [&](int p) -> int {
        SQE_HIP(hipSetDevice(g->devs[p]));
        hipStream_t s = sc.s(p);
        // RCCL: every device holds the whole gather buffer (in-place all-gather); copy exchange: only the leader does
        const bool whole = rccl || p == 0;
        SQE_TRY(gi->gather[p]->ensure(whole ? part * P : part));
        const bool q_here = !on_device || p > 0;              // the shard reads its own copy of the queries
        if (q_here || kind.extra_bytes) SQE_TRY(gi->qbuf[p]->ensure(xoff + kind.extra_bytes));
        char* qb = gi->qbuf[p]->as<char>();
        if (!on_device) {
            SQE_HIP(hipMemcpyAsync(qb, q, qbytes, hipMemcpyHostToDevice, s));
        } else if (p > 0) {
            SQE_HIP(hipStreamWaitEvent(s, gi->ev_q, 0));
            SQE_HIP(hipMemcpyPeerAsync(qb, g->devs[p], q, g->devs[0], qbytes, s));
        }
        if (kind.extra_bytes) SQE_HIP(hipMemcpyAsync(qb + xoff, kind.extra, kind.extra_bytes, hipMemcpyHostToDevice, s));
        return kind.run(p, q_here ? reinterpret_cast<const float*>(qb) : q, kind.extra_bytes ? qb + xoff : nullptr,
                        gi->gather[p]->as<char>() + (whole ? part * p : 0), s);
    };
    SQE_TRY(fan_out(g, shard_step));
    // ---- ONE exchange step: part p into slot p of the leader's buffer.  The leader's wait for every ev[p] also orders the
    // peers' reads of a device caller's queries before the caller may reuse them.
    if (rccl) {
        std::lock_guard<std::mutex> lk(g->coll_mu);
        int rc = g->rccl.GroupStart();
        for (int p = 0; p < P && rc == 0; ++p) {
            char* buf = gi->gather[p]->as<char>();
            rc = g->rccl.AllGather(buf + part * p, buf, part, RCCL_CHAR, g->comms[p], sc.s(p));
        }
        const int rc2 = g->rccl.GroupEnd();
        if (rc != 0 || rc2 != 0)
            return fail(SQE_ERR_HIP, std::string("ncclAllGather: ") + (g->rccl.GetErrorString ? g->rccl.GetErrorString(rc ? rc : rc2) : "failed"));
    } else {
        for (int p = 1; p < P; ++p) {
            SQE_HIP(hipSetDevice(g->devs[p]));
            SQE_HIP(hipMemcpyPeerAsync(gi->gather[0]->as<char>() + part * p, g->devs[0], gi->gather[p]->p, g->devs[p], part, sc.s(p)));
            SQE_HIP(hipEventRecord(gi->ev[p], sc.s(p)));
        }
        SQE_HIP(hipSetDevice(g->devs[0]));
        for (int p = 1; p < P; ++p) SQE_HIP(hipStreamWaitEvent(sc.s(0), gi->ev[p], 0));
    }
    // ---- merge on the leader: into the caller's device memory, or into `out` and from there to the host
    SQE_HIP(hipSetDevice(g->devs[0]));
    hipStream_t s0 = sc.s(0);
    if (!on_device) SQE_TRY(gi->out.ensure(kind.out_bytes ? kind.out_bytes : part));
    void* dst[4];
    for (int i = 0; i < 4; ++i) dst[i] = on_device ? kind.out[i].ptr : gi->out.as<char>() + kind.out[i].off;
    SQE_TRY(kind.merge(gi->gather[0]->as<char>(), dst, s0));
    if (!on_device) {
        for (int i = 0; i < 4; ++i)
            if (kind.out[i].bytes) SQE_HIP(hipMemcpyAsync(kind.out[i].ptr, dst[i], kind.out[i].bytes, hipMemcpyDeviceToHost, s0));
        SQE_TRY(sync_all(sc, g));
    }
    return SQE_OK;
}

// A top-k search: run(shard, p, queries, cos, ids, stream) leaves shard p's local top-k (shard-local ids) in its packed part; the
// merge maps the ids to global ones (local * P + shard + id_base) and keeps the best k, ties to the lowest global id.
template <typename Run>
int group_topk_search(sqe_index* idx, const float* q, int B, int k, bool on_device, float* cos_out, int64_t* id_out, Run&& run) {
    const int P = idx->ctx->group->P;
    const PackedPart L = PackedPart::of(B, k);
    SearchKind kind;
    kind.part = L.total;
    kind.all_gather = true;
    kind.run = [&](int p, const float* qp, const void*, char* slot, hipStream_t s) -> int {
        return run(idx->group->shards[p], p, qp, reinterpret_cast<float*>(slot + L.cos_off), reinterpret_cast<int64_t*>(slot + L.id_off), s);
    };
    kind.merge = [&](const char* parts, void* const* dst, hipStream_t s) -> int {
        return launch_merge_topk(reinterpret_cast<const float*>(parts + L.cos_off), reinterpret_cast<const int64_t*>(parts + L.id_off),
                                 (int64_t)L.total, P, B, k, (float*)dst[0], (int64_t*)dst[1], P, 1, idx->id_base, s);
    };
    kind.out[0] = {cos_out, L.cos_off, L.cos_bytes};
    kind.out[1] = {id_out, L.id_off, L.id_bytes};
    return group_search(idx, q, B, on_device, kind);
}

}  // namespace

// Top-k, plain or filtered (n_allow >= 0: the allowed global ids are one list, routed to the shards as every list is).
int group_index_search(sqe_index* idx, const float* q, int B, int k, int nprobe, float* cos_out, int64_t* id_out, bool on_device,
                       const int64_t* allow_host, int64_t n_allow) {
    PerShard allow, offs;
    const int64_t one_list[2] = {0, n_allow};
    if (n_allow >= 0) route_lists(idx, allow_host, one_list, 1, allow, offs);
    return group_topk_search(idx, q, B, k, on_device, cos_out, id_out,
                             [&](sqe_index* sh, int p, const float* qp, float* cos, int64_t* ids, hipStream_t s) -> int {
                                 if (n_allow < 0) return index_search_impl(sh, qp, B, k, nprobe, cos, ids, s);
                                 return index_search_filtered_host_ids(sh, qp, B, k, allow[p].data(), (int64_t)allow[p].size(), cos, ids, s);
                             });
}

// Per-query filtered search (filter_each.hip does the work on every shard) over the routed lists.
int group_index_search_filtered_each(sqe_index* idx, const float* q, int B, int k, const int64_t* allow_host, const int64_t* offsets_host,
                                     int n_lists, const int32_t* list_of_query_host, float* cos_out, int64_t* id_out, bool on_device) {
    PerShard allow, offs;
    route_lists(idx, allow_host, offsets_host, n_lists, allow, offs);
    return group_topk_search(idx, q, B, k, on_device, cos_out, id_out,
                             [&](sqe_index* sh, int p, const float* qp, float* cos, int64_t* ids, hipStream_t s) -> int {
                                 return index_search_filtered_each_host_ids(sh, qp, B, k, allow[p].data(), offs[p].data(), n_lists,
                                                                            list_of_query_host, cos, ids, s);
                             });
}

// Exclusion search (exclude.hip does the work on every shard) over the routed deny-lists: every shard answers for its own rows,
// and the global answer is among the parts' rows.
int group_index_search_excluding(sqe_index* idx, const float* q, int B, int k, const int64_t* deny_host, const int64_t* offsets_host,
                                 int n_lists, const int32_t* list_of_query_host, float* cos_out, int64_t* id_out, bool on_device) {
    PerShard deny, offs;
    route_lists(idx, deny_host, offsets_host, n_lists, deny, offs);
    return group_topk_search(idx, q, B, k, on_device, cos_out, id_out,
                             [&](sqe_index* sh, int p, const float* qp, float* cos, int64_t* ids, hipStream_t s) -> int {
                                 return index_search_excluding_host_ids(sh, qp, B, k, deny[p].data(), offs[p].data(), n_lists,
                                                                        list_of_query_host, cos, ids, s);
                             });
}

// The row set (internal.h: RowSet) per shard, for the six group calls that take one: the predicate as it is -- it names no id, so
// every shard evaluates it over its own rows -- and the allow-list (global ids on the host) routed to local ids as one list.
namespace {
struct ShardSets {
    const RowSet* set;         // null: unrestricted
    PerShard allow, offs;
    ShardSets(const sqe_index* idx, const RowSet* st) : set(st) {
        const int64_t one_list[2] = {0, st ? st->n_allow : 0};
        if (st && st->n_allow >= 0) route_lists(idx, st->allow, one_list, 1, allow, offs);
    }
    RowSet of(int p) const {
        if (set->n_allow < 0) return RowSet{set->pr, nullptr, -1, false};
        return RowSet{set->pr, allow[p].data(), (int64_t)allow[p].size(), true};
    }
};
}  // namespace

// Radial search (range.hip does the work on every shard): every shard answers its own rows (counts, best m, shard-local
// ids); the merge sums the counts and ranks the entries in the union, ties to the lowest global id, id_base added.
int group_index_range_search(sqe_index* idx, const float* q, int B, const float* min_cos_host, int m, int64_t* count_out, float* cos_out,
                             int64_t* id_out, bool on_device, const RowSet* set) {
    GroupIndex* gi = idx->group;
    const int P = idx->ctx->group->P;
    const RangePart L = RangePart::of(B, m);
    ShardSets sets(idx, set);
    SearchKind kind;
    kind.part = L.total;
    kind.extra = min_cos_host;
    kind.extra_bytes = (size_t)B * 4;
    kind.run = [&](int p, const float* qp, const void* min_cos, char* slot, hipStream_t s) -> int {
        if (set)
            return index_range_search_within(gi->shards[p], qp, B, (const float*)min_cos, m, sets.of(p), reinterpret_cast<int64_t*>(slot + L.count_off),
                                             reinterpret_cast<float*>(slot + L.cos_off), reinterpret_cast<int64_t*>(slot + L.id_off), s);
        return index_range_search_impl(gi->shards[p], qp, B, (const float*)min_cos, m, reinterpret_cast<int64_t*>(slot + L.count_off),
                                       reinterpret_cast<float*>(slot + L.cos_off), reinterpret_cast<int64_t*>(slot + L.id_off), s);
    };
    kind.merge = [&](const char* parts, void* const* dst, hipStream_t s) -> int {
        return launch_range_merge_parts(parts, P, B, m, idx->id_base, (int64_t*)dst[0], (float*)dst[1], (int64_t*)dst[2], s);
    };
    kind.out[0] = {count_out, L.count_off, L.count_bytes};
    kind.out[1] = {cos_out, L.cos_off, L.cos_bytes};
    kind.out[2] = {id_out, L.id_off, L.id_bytes};
    return group_search(idx, q, B, on_device, kind);
}

// Collapsed search (collapse.hip does the work on every shard): every shard answers for its own rows [cos | shard-local
// ids | keys]; one wave per query walks the union of the parts keeping the best row of every key (a row without a key never
// merges).  Exact: a group among the global best k is among the best k of the shard that holds its best row.
int group_index_search_collapsed(sqe_index* idx, const float* q, int B, int k, float* cos_out, int64_t* id_out, int64_t* key_out,
                                 bool on_device, const RowSet* set) {
    GroupIndex* gi = idx->group;
    const int P = idx->ctx->group->P;
    const CollapsePart L = CollapsePart::of(B, k);
    ShardSets sets(idx, set);
    SearchKind kind;
    kind.part = L.total;
    kind.run = [&](int p, const float* qp, const void*, char* slot, hipStream_t s) -> int {
        if (set)
            return index_search_collapsed_within(gi->shards[p], qp, B, k, sets.of(p), reinterpret_cast<float*>(slot + L.cos_off),
                                                 reinterpret_cast<int64_t*>(slot + L.id_off), reinterpret_cast<int64_t*>(slot + L.key_off), s);
        return index_search_collapsed_impl(gi->shards[p], qp, B, k, reinterpret_cast<float*>(slot + L.cos_off),
                                           reinterpret_cast<int64_t*>(slot + L.id_off), reinterpret_cast<int64_t*>(slot + L.key_off), s);
    };
    kind.merge = [&](const char* parts, void* const* dst, hipStream_t s) -> int {
        return launch_collapse_merge_parts(parts, P, B, k, idx->id_base, (float*)dst[0], (int64_t*)dst[1], (int64_t*)dst[2], s);
    };
    kind.out[0] = {cos_out, L.cos_off, L.cos_bytes};
    kind.out[1] = {id_out, L.id_off, L.id_bytes};
    kind.out[2] = {key_out, L.key_off, L.id_bytes};
    return group_search(idx, q, B, on_device, kind);
}

// MMR search (mmr.hip does the work): every shard answers with its top-n (cosines, shard-local ids) AND the fp32 rows of those
// candidates; the leader merges the P lists into the global top-n (ties to the lowest global id), points the Gram kernel's
// index table at the rows inside the gathered parts and runs the same Gram and select kernels as a single device, so the
// answer is the single-device answer bit for bit.  A part holds n dim 4 bytes per query: "mmr_row_budget" bounds the rows
// the leader's gather buffer holds (queries per pass = budget / (n P)), and every pass is one group_search.
int group_index_search_mmr(sqe_index* idx, const float* q, int B, int k, int n, const float* lam_host, int nprobe, float* cos_out,
                           int64_t* id_out, float* mmr_out, bool on_device, const RowSet* set) {
    GroupIndex* gi = idx->group;
    const int P = idx->ctx->group->P, dim = idx->dim;
    ShardSets sets(idx, set);
    if (P > 64) return fail(SQE_ERR_UNSUPPORTED, "sqe_index_search_mmr: at most 64 shards (one lane of the merge wave per shard)");
    const int bp = mmr_pass_queries(idx->mmr_row_budget, n, P);
    for (int off = 0; off < B; off += bp) {
        const int bs = std::min(bp, B - off);
        const MmrPart L = MmrPart::of(bs, n, dim);
        const MmrOut O = MmrOut::of(bs, k);
        SearchKind kind;
        kind.part = L.total;
        kind.out_bytes = O.total;
        kind.extra = lam_host + off;
        kind.extra_bytes = (size_t)bs * 4;
        kind.run = [&](int p, const float* qp, const void*, char* slot, hipStream_t s) -> int {
            const RowSet sp = set ? sets.of(p) : RowSet{};
            return index_mmr_candidates_impl(gi->shards[p], qp, bs, n, nprobe, reinterpret_cast<float*>(slot + L.cos_off),
                                             reinterpret_cast<int64_t*>(slot + L.id_off), reinterpret_cast<float*>(slot + L.row_off), s,
                                             set ? &sp : nullptr);
        };
        kind.merge = [&](const char* parts, void* const* dst, hipStream_t s) -> int {
            // the leader's copy of the weights lies behind the queries in its qbuf (group_search: extra)
            const float* lam_dev = reinterpret_cast<const float*>(gi->qbuf[0]->as<char>() + round16((size_t)bs * dim * 4));
            return mmr_merge_parts(idx, parts, P, bs, k, n, lam_dev, (float*)dst[0], (int64_t*)dst[1], (float*)dst[2], s);
        };
        kind.out[0] = {cos_out + (size_t)off * k, O.cos_off, O.cos_bytes};
        kind.out[1] = {id_out + (size_t)off * k, O.id_off, O.id_bytes};
        kind.out[2] = {mmr_out + (size_t)off * k, O.mmr_off, O.cos_bytes};
        SQE_TRY(group_search(idx, q + (size_t)off * dim, bs, on_device, kind));
    }
    return SQE_OK;
}

// Fused multi-query search (fuse.hip does the work): stage 1 is the group's plain search of all Bs sub-queries at depth n, whose
// merge leaves the global top-n (ties to the lowest global id, id_base applied) in the leader's fuse scratch instead of the
// caller's memory; the fuse kernel then runs on the leader as on a single device.  No new exchange.
int group_index_search_fused(sqe_index* idx, const float* q, int G, int Bs, const int64_t* offsets_host, int k, int n, int mode, int c,
                             const float* weights_host, int nprobe, float* fused_out, int64_t* id_out, float* cos_out, bool on_device,
                             const GroupHybrid* hy) {
    GroupIndex* gi = idx->group;
    Group* g = idx->ctx->group;
    const int P = g->P;
    const FusedOut O = FusedOut::of(G, k);
    const size_t out_total = O.total + (hy ? O.f32_bytes : 0);      // hybrid: the lexical scores [G, k] behind the fused result
    // the fuse kernel on the leader over the merged vector lists (hc / hi at depth nv; none: nv = 0); hybrid: the lexical index
    // lives on the leader, its lists are searched there, on the same stream, at the depth n of the vector lists
    auto fuse_on_leader = [&](const float* hc, const int64_t* hi, int nv, void* const* dst, hipStream_t s) -> int {
        if (!hy) return fuse_lists(idx, hc, hi, G, Bs, offsets_host, k, nv, mode, c, weights_host, (float*)dst[0], (int64_t*)dst[1], (float*)dst[2], s);
        float* ls;
        int64_t* li;
        SQE_TRY(fuse_lex_hits(idx, G, n, &ls, &li));
        SQE_TRY(lex_search_on_stream(hy->lex, hy->qoff, hy->qterms, G, n, ls, li, s));
        const FuseLex lx{ls, li, n, (float*)dst[3]};
        return fuse_lists(idx, hc, hi, G, Bs, offsets_host, k, nv, mode, c, weights_host, (float*)dst[0], (int64_t*)dst[1], (float*)dst[2], s, &lx);
    };
    if (Bs == 0) {                           // only empty groups: no search, the kernel pads on the leader
        GroupScope sc(idx, !on_device);
        SQE_HIP(hipSetDevice(g->devs[0]));
        hipStream_t s0 = sc.s(0);
        if (on_device) {
            void* dst[4] = {fused_out, id_out, cos_out, hy ? hy->lex_out : nullptr};
            return fuse_on_leader(nullptr, nullptr, 0, dst, s0);
        }
        SQE_TRY(gi->out.ensure(out_total));
        char* o = gi->out.as<char>();
        void* dst[4] = {o + O.fused_off, o + O.id_off, o + O.cos_off, o + O.total};
        SQE_TRY(fuse_on_leader(nullptr, nullptr, 0, dst, s0));
        SQE_HIP(hipMemcpyAsync(fused_out, o + O.fused_off, O.f32_bytes, hipMemcpyDeviceToHost, s0));
        SQE_HIP(hipMemcpyAsync(id_out, o + O.id_off, O.id_bytes, hipMemcpyDeviceToHost, s0));
        SQE_HIP(hipMemcpyAsync(cos_out, o + O.cos_off, O.f32_bytes, hipMemcpyDeviceToHost, s0));
        if (hy) SQE_HIP(hipMemcpyAsync(hy->lex_out, o + O.total, O.f32_bytes, hipMemcpyDeviceToHost, s0));
        SQE_HIP(hipStreamSynchronize(s0));
        return SQE_OK;
    }
    const PackedPart L = PackedPart::of(Bs, n);
    SearchKind kind;
    kind.part = L.total;
    kind.out_bytes = out_total;
    kind.all_gather = true;
    kind.run = [&](int p, const float* qp, const void*, char* slot, hipStream_t s) -> int {
        return index_search_impl(gi->shards[p], qp, Bs, n, nprobe, reinterpret_cast<float*>(slot + L.cos_off),
                                 reinterpret_cast<int64_t*>(slot + L.id_off), s);
    };
    kind.merge = [&](const char* parts, void* const* dst, hipStream_t s) -> int {
        float* hc;
        int64_t* hi;
        SQE_TRY(fuse_hits(idx, Bs, n, &hc, &hi));
        SQE_TRY(launch_merge_topk(reinterpret_cast<const float*>(parts + L.cos_off), reinterpret_cast<const int64_t*>(parts + L.id_off),
                                  (int64_t)L.total, P, Bs, n, hc, hi, P, 1, idx->id_base, s));
        return fuse_on_leader(hc, hi, n, dst, s);
    };
    kind.out[0] = {fused_out, O.fused_off, O.f32_bytes};
    kind.out[1] = {id_out, O.id_off, O.id_bytes};
    kind.out[2] = {cos_out, O.cos_off, O.f32_bytes};
    if (hy) kind.out[3] = {hy->lex_out, O.total, O.f32_bytes};
    return group_search(idx, q, Bs, on_device, kind);
}

// ---------------------------------------------------------------- group keys: id g is row g / P of shard g % P
// Every id is resolved on its shard before any shard writes anything.
int group_index_set_keys(sqe_index* idx, const int64_t* ids_host, const int64_t* keys_host, int64_t n) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P;
    GroupScope sc(idx, true);
    PerShard pos, keys(P);
    SQE_TRY(route_ids(idx, ids_host, n, "sqe_index_set_keys", pos));
    for (int64_t i = 0; i < n; ++i) keys[ids_host[i] % P].push_back(keys_host[i]);
    SQE_TRY(resolve_all(idx, sc, pos, "sqe_index_set_keys"));
    for (int p = 0; p < P; ++p) {
        if (pos[p].empty()) continue;
        SQE_HIP(hipSetDevice(g->devs[p]));
        SQE_TRY(index_set_keys_at(gi->shards[p], pos[p], keys[p].data(), sc.s(p)));
    }
    return SQE_OK;
}

int group_index_get_keys(sqe_index* idx, const int64_t* ids_host, int64_t n, int64_t* keys_out_host) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P;
    GroupScope sc(idx, true);
    PerShard pos, which;
    SQE_TRY(route_ids(idx, ids_host, n, "sqe_index_get_keys", pos, &which));
    SQE_TRY(resolve_all(idx, sc, pos, "sqe_index_get_keys"));
    for (int p = 0; p < P; ++p) {
        if (pos[p].empty()) continue;
        SQE_HIP(hipSetDevice(g->devs[p]));
        std::vector<int64_t> got(pos[p].size());
        SQE_TRY(index_get_keys_at(gi->shards[p], pos[p], got.data(), sc.s(p)));
        for (size_t j = 0; j < got.size(); ++j) keys_out_host[which[p][j]] = got[j];
    }
    return SQE_OK;
}

// ---------------------------------------------------------------- numeric fields (fields.hip does the work on every shard)
// Values are routed as the keys are.  A predicate names no id: every shard evaluates it over its own rows.
int group_index_set_field(sqe_index* idx, int field, const int64_t* ids_host, const int64_t* values_host, int64_t n) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P;
    GroupScope sc(idx, true);
    PerShard pos, vals(P);
    SQE_TRY(route_ids(idx, ids_host, n, "sqe_index_set_field", pos));
    for (int64_t i = 0; i < n; ++i) vals[ids_host[i] % P].push_back(values_host[i]);
    SQE_TRY(resolve_all(idx, sc, pos, "sqe_index_set_field"));
    for (int p = 0; p < P; ++p) {
        if (pos[p].empty()) continue;
        SQE_HIP(hipSetDevice(g->devs[p]));
        SQE_TRY(index_set_field_at(gi->shards[p], field, pos[p], vals[p].data(), sc.s(p)));
    }
    return SQE_OK;
}

int group_index_get_field(sqe_index* idx, int field, const int64_t* ids_host, int64_t n, int64_t* values_out_host) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P;
    GroupScope sc(idx, true);
    PerShard pos, which;
    SQE_TRY(route_ids(idx, ids_host, n, "sqe_index_get_field", pos, &which));
    SQE_TRY(resolve_all(idx, sc, pos, "sqe_index_get_field"));
    for (int p = 0; p < P; ++p) {
        if (pos[p].empty()) continue;
        SQE_HIP(hipSetDevice(g->devs[p]));
        std::vector<int64_t> got(pos[p].size());
        SQE_TRY(index_get_field_at(gi->shards[p], field, pos[p], got.data(), sc.s(p)));
        for (size_t j = 0; j < got.size(); ++j) values_out_host[which[p][j]] = got[j];
    }
    return SQE_OK;
}

// the slots any shard holds a column of, and the bytes of all columns
int group_index_field_info(sqe_index* idx, int* n_fields, int64_t* bytes) {
    GroupScope sc(idx, true);
    *n_fields = 0;
    *bytes = 0;
    for (sqe_index* sh : idx->group->shards) {
        int nf = 0;
        int64_t b = 0;
        index_field_info(sh, &nf, &b);
        *n_fields = std::max(*n_fields, nf);
        *bytes += b;
    }
    return SQE_OK;
}

// Every shard's counts and lowest `cap` local ids come to the host, where the counts add up and the ids (local l of shard p =
// global l * P + p) merge; a device caller gets the result copied to the leader.
int group_index_match_fields(sqe_index* idx, const FieldPreds& pr, int64_t cap, int64_t* count_out, int64_t* id_out, bool on_device) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P, np = pr.n_preds;
    GroupScope sc(idx, !on_device);
    const size_t cb = (size_t)np * 8, ib = (size_t)np * cap * 8;
    std::vector<std::vector<int64_t>> got(P);
    for (int p = 0; p < P; ++p) {
        SQE_HIP(hipSetDevice(g->devs[p]));
        SQE_TRY(gi->gather[p]->ensure(cb + ib));
        int64_t* c_dev = gi->gather[p]->as<int64_t>();
        SQE_TRY(index_match_fields_impl(gi->shards[p], pr, cap, c_dev, c_dev + np, sc.s(p)));
        got[p].resize((size_t)np * (cap + 1));
        SQE_HIP(hipMemcpyAsync(got[p].data(), c_dev, cb + ib, hipMemcpyDeviceToHost, sc.s(p)));
    }
    SQE_TRY(sync_all(sc, g));
    std::vector<int64_t> counts((size_t)np, 0), ids((size_t)np * cap, -1), merged;
    for (int j = 0; j < np; ++j) {
        merged.clear();
        for (int p = 0; p < P; ++p) {
            counts[(size_t)j] += got[p][(size_t)j];
            const int64_t* l = got[p].data() + np + (size_t)j * cap;
            for (int64_t i = 0; i < cap && l[i] >= 0; ++i) merged.push_back(l[i] * P + p + idx->id_base);
        }
        std::sort(merged.begin(), merged.end());
        const size_t keep = std::min<size_t>(merged.size(), (size_t)cap);
        std::copy(merged.begin(), merged.begin() + (ptrdiff_t)keep, ids.begin() + (ptrdiff_t)((size_t)j * cap));
    }
    if (!on_device) {
        memcpy(count_out, counts.data(), cb);
        if (ib) memcpy(id_out, ids.data(), ib);
        return SQE_OK;
    }
    SQE_HIP(hipSetDevice(g->devs[0]));
    SQE_HIP(hipMemcpyAsync(count_out, counts.data(), cb, hipMemcpyHostToDevice, sc.s(0)));
    if (ib) SQE_HIP(hipMemcpyAsync(id_out, ids.data(), ib, hipMemcpyHostToDevice, sc.s(0)));
    SQE_HIP(hipStreamSynchronize(sc.s(0)));                 // the host copies die here
    return SQE_OK;
}

int group_index_search_where(sqe_index* idx, const float* q, int B, int k, const RowSet& set, float* cos_out, int64_t* id_out, bool on_device) {
    ShardSets sets(idx, &set);
    return group_topk_search(idx, q, B, k, on_device, cos_out, id_out,
                             [&](sqe_index* sh, int p, const float* qp, float* cos, int64_t* ids, hipStream_t s) -> int {
                                 return index_search_where_impl(sh, qp, B, k, sets.of(p), cos, ids, s);
                             });
}

int group_index_search_where_each(sqe_index* idx, const float* q, int B, int k, const FieldPreds& pr, const int32_t* pred_of_query,
                                  float* cos_out, int64_t* id_out, bool on_device) {
    return group_topk_search(idx, q, B, k, on_device, cos_out, id_out,
                             [&](sqe_index* sh, int, const float* qp, float* cos, int64_t* ids, hipStream_t s) -> int {
                                 return index_search_where_each_impl(sh, qp, B, k, pr, pred_of_query, cos, ids, s);
                             });
}

// Field aggregations (aggregate.hip does the work on every shard): a predicate names no id, so every shard aggregates its own
// rows of the set (ShardSets); all of a shard's buckets come to the host, where everything merges exactly --
// counts and the partial sums add, min / max fold, a histogram's counters are placed by their bucket, and a TERMS aggregation's
// (value, count) pairs add up per value and are ranked by (count desc, value asc).
int group_index_aggregate_fields(sqe_index* idx, const RowSet& set, const sqe_field_agg_t* aggs, int n_aggs, int64_t bucket_cap,
                                 int64_t* selected_out, sqe_field_agg_result_t* result_out, int64_t* key_out, int64_t* count_out) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P;
    ShardSets sets(idx, &set);
    GroupScope sc(idx, true);
    std::vector<AggShardResult> got((size_t)P);
    for (int p = 0; p < P; ++p) {
        SQE_HIP(hipSetDevice(g->devs[p]));
        SQE_TRY(index_aggregate_shard(gi->shards[p], sets.of(p), aggs, n_aggs, &got[(size_t)p], sc.s(p)));
    }
    SQE_HIP(hipSetDevice(g->devs[0]));
    // ---- the stats, and the histograms' extents from them: a refusal still leaves these valid
    const int64_t dcap = std::min<int64_t>(bucket_cap, 16384);
    std::vector<int64_t> kmin((size_t)n_aggs, 0);
    std::string too_many;
    int64_t selected = 0;
    for (int p = 0; p < P; ++p) selected += got[(size_t)p].selected;
    for (int j = 0; j < n_aggs; ++j) {
        sqe_field_agg_result_t r{0, INT64_MAX, SQE_FIELD_NONE, 0, 0, 0, 0};
        for (int p = 0; p < P; ++p) {
            const AggShardAgg& a = got[(size_t)p].agg[j];
            r.count += a.count;
            r.min = std::min(r.min, a.min);
            r.max = std::max(r.max, a.max);
            r.sum_lo += a.sum_lo;
            r.sum_hi += a.sum_hi;
        }
        if (aggs[j].kind == SQE_AGG_HISTOGRAM && r.count > 0) {
            kmin[(size_t)j] = agg_bucket(r.min, aggs[j].interval, aggs[j].offset);
            const uint64_t nb1 = (uint64_t)agg_bucket(r.max, aggs[j].interval, aggs[j].offset) - (uint64_t)kmin[(size_t)j];
            r.n_buckets = nb1 >= (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)nb1 + 1;
            if (r.n_buckets > dcap && too_many.empty())
                too_many = "sqe_index_aggregate_fields: too_many_buckets: the histogram of aggregation " + std::to_string(j) + " has " +
                           std::to_string(nb1 + 1) + " buckets (at most min(bucket_cap, 16384) = " + std::to_string(dcap) + ")";
        }
        result_out[j] = r;
    }
    *selected_out = selected;
    if (!too_many.empty()) return fail(SQE_ERR_INVALID, too_many);
    // ---- the buckets
    std::vector<std::pair<int64_t, int64_t>> merged;         // (value, count)
    for (int j = 0; j < n_aggs; ++j) {
        int64_t* kj = key_out + (size_t)j * bucket_cap;
        int64_t* cj = count_out + (size_t)j * bucket_cap;
        for (int64_t i = 0; i < bucket_cap; ++i) {
            kj[i] = SQE_FIELD_NONE;
            cj[i] = 0;
        }
        sqe_field_agg_result_t& r = result_out[j];
        if (r.count == 0 || aggs[j].kind == SQE_AGG_STATS) continue;
        if (aggs[j].kind == SQE_AGG_HISTOGRAM) {
            for (int64_t i = 0; i < r.n_buckets; ++i) kj[i] = agg_bucket_key(kmin[(size_t)j] + i, aggs[j].interval, aggs[j].offset);
            for (int p = 0; p < P; ++p) {
                const AggShardAgg& a = got[(size_t)p].agg[j];      // its buckets lie inside the group's: base >= kmin, none skipped
                for (size_t i = 0; i < a.counts.size(); ++i) cj[a.base - kmin[(size_t)j] + (int64_t)i] += a.counts[i];
            }
            continue;
        }
        merged.clear();
        for (int p = 0; p < P; ++p) {
            const AggShardAgg& a = got[(size_t)p].agg[j];
            for (size_t i = 0; i < a.keys.size(); ++i)
                merged.emplace_back(a.keys[i], a.counts[i]);
        }
        std::sort(merged.begin(), merged.end());
        size_t m = 0;
        for (size_t i = 0; i < merged.size(); ++i) {
            if (m > 0 && merged[m - 1].first == merged[i].first) merged[m - 1].second += merged[i].second;
            else merged[m++] = merged[i];
        }
        merged.resize(m);
        std::sort(merged.begin(), merged.end(), [](const std::pair<int64_t, int64_t>& a, const std::pair<int64_t, int64_t>& b) {
            return a.second != b.second ? a.second > b.second : a.first < b.first;
        });
        r.n_buckets = (int64_t)m;
        r.other = r.count;
        for (size_t i = 0; i < std::min<size_t>(m, (size_t)aggs[j].size); ++i) {
            kj[i] = merged[i].first;
            cj[i] = merged[i].second;
            r.other -= merged[i].second;
        }
    }
    return SQE_OK;
}

// Field sort (sort.hip does the work on every shard): every shard sorts its own rows of the set (ShardSets).  A shard maps its local ids to global ids on the device (local * P + p, + the group's id_base), so the
// cursor's after_id is compared in the caller's id space; its k best and its count come to the host, where the counts add up and
// fieldsort_merge takes the first k of the union: the group's first k are among its shards' first k each.
int group_index_sort_fields(sqe_index* idx, const RowSet& set, const sqe_field_sort_t* sort, int n_sort, int k, const int64_t* after_values,
                            int64_t after_id, int64_t* total_out, int64_t* id_out, int64_t* value_out) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P;
    ShardSets sets(idx, &set);
    GroupScope sc(idx, true);
    std::vector<std::vector<int64_t>> ids((size_t)P), values((size_t)P);
    int64_t total = 0;
    for (int p = 0; p < P; ++p) {
        SQE_HIP(hipSetDevice(g->devs[p]));
        int64_t t = 0;
        ids[(size_t)p].assign((size_t)k, -1);
        values[(size_t)p].assign((size_t)k * n_sort, SQE_FIELD_NONE);
        SQE_TRY(index_sort_shard(gi->shards[p], sets.of(p), sort, n_sort, k, after_values, after_id, P, p + idx->id_base, &t,
                                 ids[(size_t)p].data(), values[(size_t)p].data(), sc.s(p)));
        total += t;
        size_t m = 0;
        while (m < (size_t)k && ids[(size_t)p][m] >= 0) ++m;
        ids[(size_t)p].resize(m);
        values[(size_t)p].resize(m * (size_t)n_sort);
    }
    SQE_HIP(hipSetDevice(g->devs[0]));
    *total_out = total;
    fieldsort_merge(reinterpret_cast<const FieldSort*>(sort), n_sort, k, ids, values, id_out, value_out);
    return SQE_OK;
}

// ---------------------------------------------------------------- deletes (compact.hip does the work on every shard)
// live global ids of every shard (local l of shard p = global l * P + p), ascending; caller holds the scope
static int collect_ids(sqe_index* idx, const GroupScope& sc, std::vector<int64_t>& out, std::vector<std::vector<int64_t>>* per_shard) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P;
    out.clear();
    for (int p = 0; p < P; ++p) {
        SQE_HIP(hipSetDevice(g->devs[p]));
        std::vector<int64_t> ids;
        SQE_TRY(index_ids_host(gi->shards[p], ids, sc.s(p)));
        for (int64_t l : ids) out.push_back(l * P + p);
        if (per_shard) (*per_shard)[p].swap(ids);
    }
    std::sort(out.begin(), out.end());
    return SQE_OK;
}

// id g goes to shard g % P as its local id g / P.  Every id is resolved on its shard before any shard deletes anything.
int group_index_delete(sqe_index* idx, const int64_t* ids_host, int64_t n) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P;
    GroupScope sc(idx, true);
    std::vector<int64_t> sorted(ids_host, ids_host + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(SQE_ERR_INVALID, "sqe_index_delete: an id repeats");
    PerShard pos;
    SQE_TRY(route_ids(idx, sorted.data(), n, "sqe_index_delete", pos));
    SQE_TRY(resolve_all(idx, sc, pos, "sqe_index_delete"));
    for (int p = 0; p < P; ++p) {
        SQE_HIP(hipSetDevice(g->devs[p]));
        std::sort(pos[p].begin(), pos[p].end());
        SQE_TRY(index_delete_positions(gi->shards[p], pos[p], sc.s(p)));
    }
    return SQE_OK;
}

int group_index_ids_vec(sqe_index* idx, std::vector<int64_t>& out) {
    GroupScope sc(idx, true);
    return collect_ids(idx, sc, out, nullptr);
}

int group_index_ids(sqe_index* idx, int64_t* ids_out, int64_t cap) {
    std::vector<int64_t> ids;
    SQE_TRY(group_index_ids_vec(idx, ids));
    if ((int64_t)ids.size() > cap) return fail(SQE_ERR_INVALID, "sqe_index_ids: cap is smaller than the live count");
    if (!ids.empty()) memcpy(ids_out, ids.data(), ids.size() * 8);
    return SQE_OK;
}

// sqe_index_load of a file with holes: rows in ascending global id, each appended to shard id % P, then every shard's map
// set to the local ids id / P and the shard's next id to the ids of its residue class below next_id
int group_index_load_rows(sqe_index* idx, FILE* f, int64_t n, const int64_t* ids, int64_t next_id, void* pinned, size_t pinned_bytes) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P, dim = idx->dim;
    GroupScope sc(idx, true);
    const size_t row_bytes = (size_t)dim * 4;
    const int64_t step = std::max<int64_t>(1, (int64_t)(pinned_bytes / row_bytes));
    std::vector<std::vector<int64_t>> local(P);
    std::vector<float> part;
    for (int64_t off = 0; off < n; off += step) {
        const int64_t m = std::min(step, n - off);
        if (fread(pinned, row_bytes, (size_t)m, f) != (size_t)m) return fail(SQE_ERR_IO, "sqe_index_load: file is truncated");
        for (int p = 0; p < P; ++p) {
            part.clear();
            for (int64_t i = 0; i < m; ++i)
                if (ids[off + i] % P == p) {
                    const float* r = (const float*)pinned + (size_t)i * dim;
                    part.insert(part.end(), r, r + dim);
                    local[p].push_back(ids[off + i] / P);
                }
            const int64_t mp = (int64_t)(part.size() / dim);
            if (mp == 0) continue;
            SQE_HIP(hipSetDevice(g->devs[p]));
            SQE_TRY(index_grow(gi->shards[p], gi->shards[p]->n.load() + mp, sc.s(p)));
            SQE_TRY(gi->stage[p]->ensure(part.size() * 4));
            SQE_HIP(hipMemcpyAsync(gi->stage[p]->p, part.data(), part.size() * 4, hipMemcpyHostToDevice, sc.s(p)));
            SQE_TRY(index_add_impl(gi->shards[p], gi->stage[p]->as<float>(), mp, dim, true, sc.s(p)));
            SQE_HIP(hipStreamSynchronize(sc.s(p)));          // `part` is reused
        }
    }
    for (int p = 0; p < P; ++p) {
        SQE_HIP(hipSetDevice(g->devs[p]));
        SQE_TRY(index_set_ids(gi->shards[p], local[p].data(), shard_rows_of(next_id, P, p), sc.s(p)));
    }
    idx->next_id.store(next_id);
    return SQE_OK;
}

// rows in GLOBAL id order into f (sqe_index_save): chunk by chunk, every shard's part of the chunk
int group_index_save_rows(sqe_index* idx, FILE* f, void* pinned, size_t pinned_bytes) {
    Group* g = idx->ctx->group;
    GroupIndex* gi = idx->group;
    const int P = g->P, dim = idx->dim;
    GroupScope sc(idx, true);
    int64_t total = 0;
    for (sqe_index* sh : gi->shards) total += sh->n.load();
    const size_t row_bytes = (size_t)dim * 4;
    if (idx->next_id.load() != total) {
        // with holes a chunk of consecutive live ids is a run of consecutive positions on every shard (positions ascend with
        // ids): one copy per shard into its region of the pinned buffer, then the rows are put in id order on the host
        std::vector<int64_t> ids;
        SQE_TRY(collect_ids(idx, sc, ids, nullptr));
        const int64_t step = std::max<int64_t>(1, (int64_t)(pinned_bytes / row_bytes));
        std::vector<int64_t> cur(P, 0), cnt(P), base(P);
        std::vector<char> out;
        for (int64_t c0 = 0; c0 < total; c0 += step) {
            const int64_t c1 = std::min(total, c0 + step);
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int64_t i = c0; i < c1; ++i) cnt[ids[(size_t)i] % P]++;
            for (int p = 0, acc = 0; p < P; ++p) { base[p] = acc; acc += (int)cnt[p]; }
            for (int p = 0; p < P; ++p) {
                if (cnt[p] == 0) continue;
                SQE_HIP(hipSetDevice(g->devs[p]));
                SQE_HIP(hipMemcpyAsync((char*)pinned + (size_t)base[p] * row_bytes, gi->shards[p]->master + (size_t)cur[p] * dim,
                                       (size_t)cnt[p] * row_bytes, hipMemcpyDeviceToHost, sc.s(p)));
            }
            SQE_TRY(sync_all(sc, g));
            out.resize((size_t)(c1 - c0) * row_bytes);
            std::vector<int64_t> k(base);
            for (int64_t i = c0; i < c1; ++i) {
                const int p = (int)(ids[(size_t)i] % P);
                memcpy(out.data() + (size_t)(i - c0) * row_bytes, (char*)pinned + (size_t)k[p]++ * row_bytes, row_bytes);
            }
            for (int p = 0; p < P; ++p) cur[p] += cnt[p];
            if (fwrite(out.data(), 1, out.size(), f) != out.size()) return fail(SQE_ERR_IO, "sqe_index_save: short write");
        }
        return SQE_OK;
    }
    const int64_t step = std::max<int64_t>(P, (int64_t)(pinned_bytes / row_bytes) / P * P);   // a multiple of P rows
    for (int64_t g0 = 0; g0 < total; g0 += step) {
        const int64_t g1 = std::min(total, g0 + step);
        for (int p = 0; p < P; ++p) {
            // g0 is a multiple of P: shard p's rows of the chunk are global g0 + p, g0 + p + P, ...
            const int64_t first = g0 + p;
            if (first >= g1) continue;
            const int64_t cnt = (g1 - first + P - 1) / P;
            SQE_HIP(hipSetDevice(g->devs[p]));
            SQE_HIP(hipMemcpy2DAsync((char*)pinned + (size_t)p * row_bytes, (size_t)P * row_bytes,
                                     gi->shards[p]->master + (size_t)(first / P) * dim, row_bytes, row_bytes, (size_t)cnt,
                                     hipMemcpyDeviceToHost, sc.s(p)));
        }
        SQE_TRY(sync_all(sc, g));
        const size_t bytes = (size_t)(g1 - g0) * row_bytes;
        if (fwrite(pinned, 1, bytes, f) != bytes) return fail(SQE_ERR_IO, "sqe_index_save: short write");
    }
    return SQE_OK;
}

}  // namespace sqe
