// exclude.hip -- exclusion k-NN search (sqe_index_search_excluding): per query the exact top-k of the live rows whose ids are
// NOT on the query's deny-list.  Take the exact ranking of all live rows as sqe_index_search defines it (fp32 cosine
// descending, ties to the lowest id), remove the denied rows, return the first k.  The answer always lies within the
// exact top-(k + d) of the plain ranking, d the length of the list, so a short list costs a plain search plus a filter.
//
//   Deny tables: the ids of all lists are translated to row positions on the device (resolve_id: the id map's binary search,
//     or the identity without a map; ids that name no live row drop out) and inserted into one position set per list
//     (id_lists.h; exclude_insert_kernel: a repeated id collapses by itself).  All tables share one buffer of at most
//     4 x (entries + lists) words; they live for the call only.
//   Stage A (FLAT indexes): query b needs depth kd_b = min(256, k + len_b) ("exclude_depth", if set, caps it; a query
//     without a list needs k).  The queries of a pass form at most two classes -- kd_b <= "i8_sample_m" (the int8 first
//     pass of a large index stays on) and the rest -- so that a short list never pays for a long one's depth; each class is
//     gathered into contiguous scratch and searched by the unchanged certified search at the largest kd_b among it.
//     deny_drop_kernel<DenyTable> (deny_kernels.h; one wave per query) walks the hits 64 at a time, probes the query's table per lane, compacts the
//     survivors by ballot and prefix popcount and writes the first k into the caller's row.  A query with fewer than k
//     survivors although the index holds more rows than were fetched is flagged; with the automatic depth and
//     k + len_b <= 256 that cannot happen.
//   Stage B (the flagged queries; every query of an IVF index that names a list): sweep.hip's sweep (sweep_flagged: the
//     compaction of the flags, the one read-back of their number, the walk over row ranges), as collapsed search runs it,
//     with "denied" in place of "key already seen".  Per slot a running list of at most k (cosine, position) entries in the
//     caller's row and a threshold, its k-th cosine (-inf while shorter).  The keys a range collected at threshold - eps
//     are re-scored in fp32 by rescore_row (the chain of the search: same bits), the denied ones dropped by table
//     probe, and the rest merged with the running list by block_select.h's select (deny_merge_kernel<DenyTable>).  Dropping a row
//     below the k-th of k undenied rows never changes the answer, so ranges may come in any order and size.
//   Positions -> ids through the index's id map, then id_base.
// The owner's search state is left as plain searches of the class depths leave it.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "deny_kernels.h"
#include "internal.h"

namespace sqe {

constexpr int EX_MAX_PASS = SWEEP_MAX_PASS;

struct ExcludeState {
    DevBuf stage;      // host entry points: queries and results
    DevBuf hdeny;      // deny ids that came from the host
    DevBuf tab;        // the hash sets of all lists
    DevBuf meta;       // ExList [n_lists] | list_of_query [B]
    DevBuf cls;        // [passes, 2, EX_MAX_PASS] int: queries of the shallow / deep class of every pass
    DevBuf gq;         // [EX_MAX_PASS, dim] gathered raw queries of a class
    DevBuf hits;       // stage A of a class: cos [nq, kd] (16-B rounded) | positions [nq, kd]
    DevBuf flags;      // [B] int: the query is incomplete
    SweepBufs sw;      // stage B
};

namespace {

// entry e of the id array: its list by binary search of the entry offsets, its position, and -- if the id names a row of the
// index -- the position into the list's table
__global__ __launch_bounds__(256) void exclude_insert_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ map,
                                                             int64_t total, const ExList* __restrict__ lists, int n_lists, int64_t n_rows,
                                                             uint32_t* __restrict__ tab) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    int lo = 0, hi = n_lists - 1;               // the last list whose entry_off <= e (empty lists share an offset: take the last)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (lists[mid].entry_off <= e) lo = mid;
        else hi = mid - 1;
    }
    const ExList L = lists[lo];
    const int64_t p = resolve_id(map, n_rows, ids[e]);
    if (p >= 0) pos_set_insert(tab + L.tab_off, L.tab_mask, (uint32_t)p);
}

ExcludeState* exclude_state(sqe_index* idx) {
    if (!idx->exclude) idx->exclude = new (std::nothrow) ExcludeState;
    return idx->exclude;
}

// the tables of all lists, the list descriptors and list_of_query on the device (nothing is read back).  `host` is the image of
// st->meta; the caller keeps it until the stream is synchronised.
int build_tables(sqe_index* idx, ExcludeState* st, const int64_t* deny_dev, const int64_t* offsets, int n_lists, const int32_t* loq, int B,
                 std::vector<char>& host, hipStream_t s) {
    const int64_t n = idx->n.load();
    const int64_t total = n_lists > 0 ? offsets[n_lists] : 0;
    std::vector<ExList> lists((size_t)n_lists);
    int64_t n_tab = 0;
    for (int f = 0; f < n_lists; ++f) {
        const int64_t cap = pos_set_slots(offsets[f + 1] - offsets[f]);
        if (cap > POS_SET_MAX_SLOTS) return fail(SQE_ERR_INVALID, "sqe_index_search_excluding: a list of more than 2^31 entries");
        lists[(size_t)f] = {offsets[f], n_tab, (uint32_t)(cap - 1)};
        n_tab += cap;
    }
    const size_t lb = round16(lists.size() * sizeof(ExList));
    host.resize(lb + (size_t)B * 4);
    if (n_lists > 0) memcpy(host.data(), lists.data(), lists.size() * sizeof(ExList));
    memcpy(host.data() + lb, loq, (size_t)B * 4);
    SQE_TRY(st->meta.ensure(host.size()));
    SQE_TRY(st->tab.ensure((size_t)std::max<int64_t>(n_tab, 1) * 4));
    StageTimer t(idx->ctx->prof, s, ST_PREP);
    SQE_HIP(hipMemcpyAsync(st->meta.p, host.data(), host.size(), hipMemcpyHostToDevice, s));
    if (n_tab > 0) SQE_HIP(hipMemsetAsync(st->tab.p, 0xFF, (size_t)n_tab * 4, s));
    if (total > 0) {
        hipLaunchKernelGGL(exclude_insert_kernel, dim3(grid_of(total, 256)), dim3(256), 0, s, deny_dev,
                           idx->has_map ? idx->idmap.as<int64_t>() : nullptr, total, st->meta.as<ExList>(), n_lists, n, st->tab.as<uint32_t>());
        SQE_HIP(hipGetLastError());
    }
    return SQE_OK;
}

// Stage A for one class of a pass: `cls` (device) / nq queries of the pass at depth kd
int run_class(sqe_index* idx, ExcludeState* st, const float* q_pass, const int* cls, int nq, int kd, int k, const int32_t* loq_pass,
              const ExList* lists, float* cos_pass, int64_t* pos_pass, int* flags_pass, hipStream_t s) {
    const int K = idx->dim;
    const size_t cb = round16((size_t)nq * kd * 4);
    SQE_TRY(st->gq.ensure((size_t)nq * K * 4));
    SQE_TRY(st->hits.ensure(cb + (size_t)nq * kd * 8));
    SQE_TRY(launch_each_rows(q_pass, st->gq.p, cls, nq, K * 4, 0, s));      // the raw queries of the class
    float* hc = st->hits.as<float>();
    int64_t* hp = reinterpret_cast<int64_t*>(st->hits.as<char>() + cb);
    SQE_TRY(index_search_positions(idx, st->gq.as<float>(), nq, kd, 0, hc, hp, s));
    StageTimer t(idx->ctx->prof, s, ST_SELECT);
    DropArgs<DenyTable> a;
    a.hit_cos = hc; a.hit_pos = hp; a.kd = kd; a.k = k; a.cls = cls; a.deny = {loq_pass, lists, st->tab.as<uint32_t>()};
    a.id_sub = search_id_base(idx); a.n_rows = idx->n.load(); a.cos_out = cos_pass; a.pos_out = pos_pass; a.flags = flags_pass;
    hipLaunchKernelGGL(deny_drop_kernel<DenyTable>, dim3(nq), dim3(64), 0, s, a);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

// deny_merge_kernel over the keys a range collected for the hs slots qidx of the pass whose output rows are cos / pos
int launch_xmerge(sqe_index* idx, ExcludeState* st, const int* qidx, int hs, int64_t r0, int k, const int32_t* loq_pass, const ExList* lists,
                  float* cos, int64_t* pos, hipStream_t s) {
    SweepBufs& b = st->sw;
    StageTimer t(idx->ctx->prof, s, ST_SELECT);
    MergeArgs<DenyTable> a;
    a.master = idx->master; a.qn = b.qn.as<float>(); a.K = idx->dim; a.qidx = qidx;
    a.keys = b.keys.as<uint64_t>(); a.key_cnt = b.key_cnt.as<int>(); a.row_off = r0; a.k = k;
    a.deny = {loq_pass, lists, st->tab.as<uint32_t>()};
    a.q_resid = b.q_resid.as<float>(); a.resid_max = idx->resid_max.as<uint32_t>();
    a.thr = b.thr.as<float>(); a.kth = b.kth.as<float>(); a.lcnt = b.lcnt.as<int>();
    a.cos_out = cos; a.pos_out = pos;
    hipLaunchKernelGGL(deny_merge_kernel<DenyTable>, dim3(hs), dim3(DENY_MERGE_THREADS), 0, s, a);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

}  // namespace

void exclude_destroy(ExcludeState* e) { delete e; }

// Caller holds the index lock and has validated the host arrays; everything runs on stream s.
int index_search_excluding_impl(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* deny_dev, const int64_t* offsets,
                                int n_lists, const int32_t* list_of_query, float* cos_out_dev, int64_t* id_out_dev, hipStream_t s) {
    sqe_ctx* ctx = idx->ctx;
    const int64_t n = idx->n.load();
    const int K = idx->dim;
    if (B <= 0) return SQE_OK;
    ctx->exclude_swept.store(0);
    const int64_t bk = (int64_t)B * k;
    if (n == 0) return launch_pad_hits(cos_out_dev, id_out_dev, nullptr, bk, s);
    if (n > (int64_t)UINT32_MAX) return fail(SQE_ERR_INVALID, "sqe_index_search_excluding: more than 2^32 rows");
    ExcludeState* st = exclude_state(idx);
    if (!st) return fail(SQE_ERR_OOM, "sqe_index_search_excluding: host allocation failed");
    std::vector<char> meta_host;                 // the host images of the uploads live until the read-back below synchronises s
    SQE_TRY(build_tables(idx, st, deny_dev, offsets, n_lists, list_of_query, B, meta_host, s));
    const ExList* lists = st->meta.as<ExList>();
    const int32_t* loq_dev = reinterpret_cast<const int32_t*>(st->meta.as<char>() + round16((size_t)n_lists * sizeof(ExList)));
    const int passes = (B + EX_MAX_PASS - 1) / EX_MAX_PASS;
    SQE_TRY(st->flags.ensure((size_t)B * 4));
    SQE_TRY(st->cls.ensure((size_t)passes * 2 * EX_MAX_PASS * 4));
    // ---- stage A: the two classes of every pass of a FLAT index; on an IVF index only the queries without a list (the plain search)
    struct Class { int cnt = 0, depth = 0; };
    std::vector<Class> classes((size_t)passes * 2);
    std::vector<int> cls_host((size_t)passes * 2 * EX_MAX_PASS), flags_host;
    if (idx->ivf) flags_host.resize((size_t)B);
    const int cap = idx->exclude_depth > 0 ? std::max(idx->exclude_depth, k) : MAX_KP;
    for (int b = 0; b < B; ++b) {
        const int f = list_of_query[b];
        if (idx->ivf) {
            flags_host[(size_t)b] = f >= 0;
            if (f >= 0) continue;
        }
        const int64_t len = f < 0 ? 0 : offsets[f + 1] - offsets[f];
        const int kd = (int)std::min<int64_t>(cap, k + len);
        const size_t c = (size_t)(b / EX_MAX_PASS) * 2 + ((!idx->ivf && kd > idx->i8_sample_m) ? 1 : 0);
        cls_host[c * EX_MAX_PASS + classes[c].cnt++] = b % EX_MAX_PASS;
        classes[c].depth = std::max(classes[c].depth, kd);
    }
    SQE_HIP(hipMemcpyAsync(st->cls.p, cls_host.data(), cls_host.size() * 4, hipMemcpyHostToDevice, s));
    for (size_t c = 0; c < classes.size(); ++c) {
        if (classes[c].cnt == 0) continue;
        const int off = (int)(c / 2) * EX_MAX_PASS;
        SQE_TRY(run_class(idx, st, q_dev + (size_t)off * K, st->cls.as<int>() + c * EX_MAX_PASS, classes[c].cnt, classes[c].depth, k,
                          loq_dev + off, lists, cos_out_dev + (size_t)off * k, id_out_dev + (size_t)off * k,
                          idx->ivf ? nullptr : st->flags.as<int>() + off, s));
    }
    if (idx->ivf) SQE_HIP(hipMemcpyAsync(st->flags.p, flags_host.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    // ---- stage B: the sweep of the flagged queries
    SQE_TRY(sweep_flagged(idx, st->sw, st->flags.as<int>(), q_dev, B, k, cos_out_dev, id_out_dev, nullptr, ctx->exclude_swept,
                          [&](int off, const int* qidx, int hs, int64_t r0) {
                              return launch_xmerge(idx, st, qidx, hs, r0, k, loq_dev + off, lists, cos_out_dev + (size_t)off * k,
                                                   id_out_dev + (size_t)off * k, s);
                          },
                          s));
    // positions -> ids (+ id_base)
    return index_positions_to_ids(idx, id_out_dev, bk, s);
}

// the same with host ids, staged in the state's own buffer; synchronises s before it returns (deny_host is not retained)
int index_search_excluding_host_ids(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* deny_host, const int64_t* offsets,
                                    int n_lists, const int32_t* list_of_query, float* cos_out_dev, int64_t* id_out_dev, hipStream_t s) {
    ExcludeState* st = exclude_state(idx);
    if (!st) return fail(SQE_ERR_OOM, "sqe_index_search_excluding: host allocation failed");
    const int64_t* deny_dev;
    SQE_TRY(stage_host_ids(st->hdeny, deny_host, n_lists > 0 ? offsets[n_lists] : 0, s, &deny_dev));
    SQE_TRY(index_search_excluding_impl(idx, q_dev, B, k, deny_dev, offsets, n_lists, list_of_query, cos_out_dev, id_out_dev, s));
    SQE_HIP(hipStreamSynchronize(s));
    return SQE_OK;
}

}  // namespace sqe

// ================================================================ C ABI
using namespace sqe;

extern "C" {

static int excluding_args_ok(sqe_index* idx, const void* q, int B, int k, const void* deny, const int64_t* offsets, int n_lists,
                             const int32_t* list_of_query, const void* cos, const void* ids) {
    const char* who = "sqe_index_search_excluding: ";
    SQE_TRY(list_args_ok(who, "deny_ids", -1, idx, q, B, k, deny, offsets, n_lists, list_of_query, cos, ids));
    if (!idx->group && idx->n.load() > (int64_t)UINT32_MAX) return fail(SQE_ERR_INVALID, std::string(who) + "more than 2^32 rows");
    return SQE_OK;
}

int sqe_index_search_excluding(sqe_index* idx, const float* q_host, int B, int k, const int64_t* deny_ids_host,
                               const int64_t* list_offsets_host, int n_lists, const int32_t* list_of_query_host, float* cos_out_host,
                               int64_t* id_out_host) {
    SQE_TRY(excluding_args_ok(idx, q_host, B, k, deny_ids_host, list_offsets_host, n_lists, list_of_query_host, cos_out_host, id_out_host));
    if (B == 0) return SQE_OK;
    if (idx->group)
        return group_index_search_excluding(idx, q_host, B, k, deny_ids_host, list_offsets_host, n_lists, list_of_query_host, cos_out_host,
                                            id_out_host, false);
    OpScope op(idx->ctx, idx->ord, true);
    ExcludeState* st = exclude_state(idx);
    if (!st) return fail(SQE_ERR_OOM, "sqe_index_search_excluding: host allocation failed");
    const size_t qbytes = round16((size_t)B * idx->dim * 4), cb = (size_t)B * k * 4, ib = (size_t)B * k * 8;
    SQE_TRY(st->stage.ensure(qbytes + round16(cb) + ib));
    float* q_dev = st->stage.as<float>();
    float* cos_dev = reinterpret_cast<float*>(st->stage.as<char>() + qbytes);
    int64_t* id_dev = reinterpret_cast<int64_t*>(st->stage.as<char>() + qbytes + round16(cb));
    SQE_HIP(hipMemcpyAsync(q_dev, q_host, (size_t)B * idx->dim * 4, hipMemcpyHostToDevice, op.s));
    SQE_TRY(index_search_excluding_host_ids(idx, q_dev, B, k, deny_ids_host, list_offsets_host, n_lists, list_of_query_host, cos_dev, id_dev,
                                            op.s));
    SQE_HIP(hipMemcpyAsync(cos_out_host, cos_dev, cb, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(id_out_host, id_dev, ib, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

int sqe_index_search_excluding_device(sqe_index* idx, const float* q_dev, int B, int k, const int64_t* deny_ids_dev,
                                      const int64_t* list_offsets_host, int n_lists, const int32_t* list_of_query_host, float* cos_out_dev,
                                      int64_t* id_out_dev) {
    SQE_TRY(excluding_args_ok(idx, q_dev, B, k, deny_ids_dev, list_offsets_host, n_lists, list_of_query_host, cos_out_dev, id_out_dev));
    if (B == 0) return SQE_OK;
    if (idx->group) {
        std::vector<int64_t> deny;               // the shards' lists are routed on the host
        SQE_TRY(list_ids_to_host(idx->ctx, deny_ids_dev, list_offsets_host, n_lists, deny));
        return group_index_search_excluding(idx, q_dev, B, k, deny.data(), list_offsets_host, n_lists, list_of_query_host, cos_out_dev,
                                            id_out_dev, true);
    }
    OpScope op(idx->ctx, idx->ord, false);
    return index_search_excluding_impl(idx, q_dev, B, k, deny_ids_dev, list_offsets_host, n_lists, list_of_query_host, cos_out_dev,
                                       id_out_dev, op.s);
}

int sqe_exclude_swept(sqe_ctx* ctx, int64_t* out) {
    if (!ctx || !out) return fail(SQE_ERR_INVALID, "sqe_exclude_swept: null argument");
    int64_t v = 0;
    for (int p = 0; p < group_member_count(ctx); ++p) v += group_member(ctx, p)->exclude_swept.load();
    *out = v;
    return SQE_OK;
}

}  // extern "C"
