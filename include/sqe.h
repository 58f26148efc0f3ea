/* sqe.h -- C ABI of libsqe.so, the MI355X (gfx950) embedding + cosine k-NN + cosine-cache
 * engine that replaces the Ollama-embed / OpenSearch-HNSW / Redis-scan leg of the
 * reference's /ask pipeline (/root/reference/app/main.py:56-180, 250-373).
 *
 * The reference has no FFI of its own: its hot path is three network clients called by
 * plain Python names.  Each entry point below states which reference call it stands
 * behind; INTEGRATION.md shows the ctypes stub a maintainer adds on the reference side.
 *
 * Conventions
 *   - return 0 (SQE_OK) or a negative error code; sqe_last_error() gives thread-local text
 *   - the caller allocates every output buffer; the library owns all device memory
 *   - host inputs are copied before return and never retained
 *   - "_device" variants take device pointers, enqueue on the context stream and do not
 *     synchronise (sqe_synchronize does); they exist so a caller that already holds its
 *     data in HBM (bench.py, the encoder -> search hand-off, torch.distributed shards)
 *     pays no PCIe copy
 *   - every entry point is thread-safe: the reference calls add_embeddings from a
 *     thread-pool thread while search runs on the event-loop thread (main.py:454-455, 499).
 *     There is no context-wide lock: every index, cache and encoder has its own mutex and its
 *     own stream (host entry points run there and synchronise it before returning), so an add
 *     on one index never blocks a search on another, the cache scan or the encoder
 *   - multi-GPU, two forms: ONE host process driving several devices (sqe_create with
 *     n_dev > 1: what the reference's single uvicorn process needs, main.py:738-739), or one
 *     process per GPU over torch.distributed with single-device contexts (bench.py, sharded.py)
 *   - the library reads no environment variable
 */
#ifndef SQE_H
#define SQE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SQE_VERSION 100 /* 0.1.0 */

typedef struct sqe_ctx sqe_ctx;
typedef struct sqe_index sqe_index;
typedef struct sqe_cache sqe_cache;
typedef struct sqe_encoder sqe_encoder;
typedef struct sqe_tokenizer sqe_tokenizer;

enum {
    SQE_OK = 0,
    SQE_ERR_INVALID = -1,     /* bad argument */
    SQE_ERR_HIP = -2,         /* a HIP runtime call failed */
    SQE_ERR_OOM = -3,         /* device or host allocation failed */
    SQE_ERR_STATE = -4,       /* object not in a state that allows the call */
    SQE_ERR_UNSUPPORTED = -5, /* valid request this build does not implement */
    SQE_ERR_IO = -6           /* file could not be opened, read or written, or is not a saved index */
};

enum { SQE_INDEX_FLAT = 0, SQE_INDEX_IVF_FLAT = 1 };

/* How the stored rows are scanned.  Both return the exact fp32 top-k: cosines are fp32 re-scores from the fp32
 * master copy, and a per-query certificate (option "certify") proves that no row outside the re-scored set can
 * reach the k-th cosine -- the rounding of every scanned copy is measured and bounded -- with a bf16 collect pass
 * for the queries where the proof fails.
 *   BF16_RESCORE: bf16 MFMA scan with a fused top-k filter (every batch size, every index size; what IVF indexes and
 *                 every case outside the int8 conditions below run);
 *   INT8_RESCORE (default of FLAT indexes): int8 MFMA first pass at twice the bf16 rate over a per-row-scaled int8 copy (+1 byte per element):
 *                 a 2 % row sample fixes per-query thresholds, the int8 scan collects every row above them, the
 *                 collected rows are re-scored in fp32.  Used on FLAT indexes of >= "i8_min_rows" rows (default 1 M),
 *                 dim >= 256 and a multiple of 128, k <= "i8_sample_m" (20), rows that quantise within "i8_max_resid";
 *                 everything else runs the bf16 scan.  Suited to rows whose
 *                 elements are of similar magnitude (unit Gaussian-like embeddings): the int8 error bound is ~8 x the
 *                 bf16 one, and data on which it is too wide simply takes the bf16 pass.
 * (r02's header also listed an fp32 scan mode that was never built; it is gone.) */
enum { SQE_SCAN_BF16_RESCORE = 0, SQE_SCAN_INT8_RESCORE = 2 };

/* ---- library / context ---------------------------------------------------------- */
int sqe_version(void);
const char* sqe_last_error(void);

/* n_dev == 1: the context drives HIP device device_ids[0].
 * n_dev > 1: single process, many devices (the reference is one uvicorn process, main.py:738-739).  The
 * context leads one member context per device; flat indexes created on it are sharded row-wise (global row g
 * on shard g % n_dev), a search sends the query batch to every device, runs the per-shard top-k there and
 * exchanges the packed [B,k] results in ONE step -- RCCL all-gather over xGMI (ncclCommInitAll, one
 * communicator per device) or, where RCCL is unavailable, peer copies to device_ids[0] -- before the merge
 * on device_ids[0].  Device pointers of "_device" entry points are memory of device_ids[0].  Caches and
 * encoders live on device_ids[0] (replicas only).  IVF indexes shard the same way: sqe_index_train
 * runs k-means once on device_ids[0] and replicates the centroids, every device keeps the lists of the rows it owns,
 * all devices probe the same lists and the per-device top-k go through the same exchange + merge. */
int sqe_create(const int* device_ids, int n_dev, sqe_ctx** out);
/* General form: `exchange` picks the exchange step, and device ids may repeat (several logical shards on
 * one device -- how a one-GPU box rehearses the sharded path; those use the copy exchange).  A group of ONE
 * shard with SQE_EXCHANGE_RCCL runs the in-library RCCL leg on a single device. */
enum { SQE_EXCHANGE_AUTO = 0, SQE_EXCHANGE_RCCL = 1, SQE_EXCHANGE_COPY = 2 };
int sqe_create_sharded(const int* device_ids, int n_shards, int exchange, sqe_ctx** out);
/* Shards of the context (1 for a single-device context), the exchange in use and the device of each shard. */
int sqe_group_info(sqe_ctx* ctx, int* n_shards, int* exchange, int* device_ids, int cap);
void sqe_destroy(sqe_ctx* ctx);
int sqe_synchronize(sqe_ctx* ctx);
/* hipStream_t the "_device" entry points enqueue on (for event timing by the caller). */
void* sqe_stream(sqe_ctx* ctx);
/* Make the context enqueue on a caller-owned hipStream_t (e.g. torch's current stream, so
 * collectives and library kernels order without host synchronisation); NULL restores the
 * context's own stream.  The caller keeps the stream alive while it is set. */
int sqe_set_stream(sqe_ctx* ctx, void* hip_stream);
int sqe_device_info(sqe_ctx* ctx, char* name, int name_cap, int* cu_count, int64_t* hbm_bytes);

/* ---- vector index: stands behind OpenSearchIndexer (main.py:291-373) ------------- */
/* Index mapping of main.py:262-282: cosine similarity over `dim`-d vectors.  `kind`
 * selects exact brute force (FLAT) or IVF-flat with `nlist` lists. dim % 64 == 0. */
int sqe_index_create(sqe_ctx* ctx, int dim, int kind, int nlist, sqe_index** out);
void sqe_index_destroy(sqe_index* idx);
int sqe_index_reserve(sqe_index* idx, int64_t rows);

/* Ids.  Every appended row gets the next id: next_id .. next_id+n-1, where next_id counts the rows ever appended
 * (sqe_index_next_id).  Ids are never reused, so after a delete they are no longer 0 .. count-1; until the first
 * delete they are, exactly as before deletes existed.  Searches return ids (plus "id_base"); update, get_rows and
 * delete take ids local to this index (without id_base).  A group context keeps global id g on shard g % n_dev. */

/* add_embeddings (main.py:309-338): L2-normalises each row as x / (||x|| + 1e-9) in fp32
 * (main.py:315-316) and appends; rows get ids next_id .. next_id+n-1.  x is [n, dim] row-major. */
int sqe_index_add(sqe_index* idx, const float* x_host, int64_t n);
int sqe_index_add_device(sqe_index* idx, const float* x_dev, int64_t n);
/* Re-indexing an existing `_id` overwrites the document (OpenSearch "index" op,
 * main.py:321-325): replace the rows with the given ids in place.  A deleted or never-assigned id gives
 * SQE_ERR_INVALID and nothing is written. */
int sqe_index_update(sqe_index* idx, const int64_t* rows_host, const float* x_host, int64_t n);
/* Live rows.  has_any_data (main.py:300-307) is count > 0. */
int sqe_index_count(const sqe_index* idx, int64_t* out);
/* Normalised fp32 rows of the given ids as stored (`_source.embedding` of a hit, main.py:327-331).  A deleted or
 * never-assigned id gives SQE_ERR_INVALID. */
int sqe_index_get_rows(sqe_index* idx, const int64_t* rows_host, int64_t n, float* out_host);
/* OpenSearch "delete" / delete_by_query (the counterpart of the "index" op, main.py:321-325): the rows with these ids
 * leave the index.  Ids are local (without id_base), as for sqe_index_update.  Every id must be live, and no id may
 * repeat in the call; otherwise SQE_ERR_INVALID is returned and nothing is deleted.  Ids are never reused.  The live
 * rows are compacted in place keeping their order, so the index then searches exactly like one built from the live
 * rows in id order; the int8 copy of the moved rows is re-quantised by the next int8 search. */
int sqe_index_delete(sqe_index* idx, const int64_t* ids_host, int64_t n);
/* Live ids in ascending order (sqe_index_count of them); cap = room in ids_out. */
int sqe_index_ids(sqe_index* idx, int64_t* ids_out_host, int64_t cap);
/* The id the next appended row gets (= rows ever appended). */
int sqe_index_next_id(const sqe_index* idx, int64_t* out);

/* Options: "scan_mode" (SQE_SCAN_*; int8 tuning: "i8_min_rows", "i8_sample_step" = sample every n-th tile,
 * "i8_sample_m" = the threshold is the m-th best score of the sample, "i8_anchor_margin" (default 0.25): the threshold never
 * lies above (best true cosine of the sample) - eps * (1 + margin), which makes the int8 certificate hold by construction on rows
 * that crowd together, "i8_key_budget" (default 6144; 0 = no limit): where the sample predicts that the anchored threshold would collect more
 * keys than this, the m-th sample score alone stands, "i8_sample_int8" = 1 (default): the sample is scanned
 * in int8 too, 0: by the bf16 kernels with an fp32 re-score, "i8_keep_select" (0/1, default 0; TEST-ONLY: an int8 search
 * also copies what select_i8_kernel wrote aside before the bf16 collect pass runs -- sqe_index_i8_read: SQE_I8_SELECT_*; the answers
 * are the same bit for bit, and with 0 nothing is allocated, copied or launched for it), "i8_max_resid" = the largest int8 rounding residual
 * of a stored row, default 0.02, beyond which the index answers with the bf16 scan), "rescore_k" (candidates kept by the bf16 scan,
 * 0 = automatic), "nprobe" default for IVF, "id_base" (added to every returned row id:
 * the first global row of this shard in a row-sharded index), "certify" (default 1: prove
 * per query that no row outside the re-scored candidates can reach the k-th cosine -- the
 * bf16 rounding of every vector is bounded -- and re-scan the fp32 master for the queries
 * where that proof fails; 0 = skip both), "filter_gather_rows" (default 2^20, >= 256: allowed rows a filtered
 * search gathers and searches per chunk; more are searched chunk by chunk and merged), "filter_each_direct_rows",
 * "filter_each_direct_queries", "filter_each_key_budget" (sqe_index_search_filtered_each), "range_key_budget" (default 2^25,
 * >= 4096: collected keys a radial search or the sweep of a collapsed search holds at once, sqe_index_range_search),
 * "collapse_depth" (default 0 = automatic, else 1..256: rows the first stage of sqe_index_search_collapsed fetches),
 * "exclude_depth" (default 0 = k + the length of the query's deny-list, else 1..256: a cap on the rows the first stage of
 * sqe_index_search_excluding fetches),
 * "mmr_row_budget" (default 65536, >= 256: candidate rows -- queries of a pass x depth n -- whose Gram scratch and, on a device
 * group, gathered rows sqe_index_search_mmr holds at once; larger batches run in passes). */
int sqe_index_set_option(sqe_index* idx, const char* key, double value);

/* search (main.py:347-373): q is [B, dim] row-major raw query embeddings; each is
 * normalised as q / (||q|| + 1e-9) (main.py:353-354) and its cosine top-k returned best
 * first, ties to the lowest id.  cos_out [B,k] fp32 cosines, id_out [B,k] int64 row ids,
 * padded with (-inf, -1) when fewer than k rows qualify.  The reference searches row 0
 * only (main.py:355); B > 1 is the batched form of the same call.  nprobe is ignored for
 * FLAT (0 = index default for IVF).  1 <= k <= 256. */
int sqe_index_search(sqe_index* idx, const float* q_host, int B, int k, int nprobe,
                     float* cos_out_host, int64_t* id_out_host);
int sqe_index_search_device(sqe_index* idx, const float* q_dev, int B, int k, int nprobe,
                            float* cos_out_dev, int64_t* id_out_dev);

/* Filtered search: the exact fp32 cosine top-k over the live rows whose ids are in allow_ids[n_allow]; all B queries
 * share the list.  Output shape, order (best first, ties to the lowest id), (-inf, -1) padding and id_base are those of
 * sqe_index_search.  The ids are local ids as for sqe_index_delete (global ids on a device group).  The list may be in
 * any order and may repeat ids; ids that name no live row (deleted, never assigned, >= next_id, negative) are skipped,
 * and n_allow == 0 returns all padding.  FLAT and IVF indexes alike answer exactly over the allowed rows (no nprobe).
 * The allowed rows are copied into an internal scratch index of at most "filter_gather_rows" rows (option, default
 * 2^20) and searched there, chunk by chunk; an index that never gets a filtered search allocates nothing for it.
 * The _device form reads the number of allowed rows back to plan the scan: it synchronises the context stream once
 * (on a device group it first copies the list to the host). */
int sqe_index_search_filtered(sqe_index* idx, const float* q_host, int B, int k,
                              const int64_t* allow_ids_host, int64_t n_allow,
                              float* cos_out_host, int64_t* id_out_host);
int sqe_index_search_filtered_device(sqe_index* idx, const float* q_dev, int B, int k,
                                     const int64_t* allow_ids_dev, int64_t n_allow,
                                     float* cos_out_dev, int64_t* id_out_dev);

/* Per-query filtered search: query b is answered over its OWN allow-list.  List f is allow_ids[list_offsets[f] ..
 * list_offsets[f + 1]), query b is answered over list list_of_query[b]; any number of queries may name one list and a list
 * may be named by none.  list_offsets [n_lists + 1] and list_of_query [B] are HOST memory in both forms and are not retained
 * past return.  Row b of the output is the exact top-k of the live rows its list names, best first: ordered by the fp32 cosine
 * sqe_index_search returns for the row (same normalised query, same re-score chain), ties to the lowest id, (-inf, -1) padded.
 * Ids, repeats and ids that name no live row are treated as by sqe_index_search_filtered (a repeated id answers once; an
 * empty or all-dead list gives all padding); id_base is added.  A query's answer depends on the query, its list and the index
 * only: not on B, its place in the batch, the other lists, the route or the options below.
 * Two routes, chosen per list on the host.  A list of at most "filter_each_direct_rows" entries (option, default 16384;
 * 0 = none) that at most "filter_each_direct_queries" queries name (option, default 32; 0 = none) is scored DIRECTLY: every
 * listed row in fp32 against the master copy in place, then a per-query select -- no first pass, so the result is exact with
 * "certify" = 0 too, and the _device form reads nothing back and calls no stream synchronisation (its small planning tables
 * are copied from pageable host memory once per pass, which the runtime may complete before it returns).  Every other list is
 * GATHERED: the queries that name it are answered by one sqe_index_search_filtered over the list (one synchronisation per such
 * list; with "certify" = 0 as approximate as that search).  With "certify" = 1 both routes return the same bits, those of
 * sqe_index_search_filtered(q_b, 1, k, list).  The direct route holds one 8-byte key per (query, entry of its list):
 * "filter_each_key_budget" (option, default 2^24 keys, >= 4096) bounds the keys held at once, more run in passes.  An index
 * that never gets this call allocates nothing for it.  FLAT and IVF alike (no nprobe); on a device group the ids are global
 * and the _device form first copies the ids to the host.
 * SQE_ERR_INVALID, with nothing written: list_offsets not starting at 0 or decreasing, n_lists < 0, a list_of_query entry
 * outside [0, n_lists), k outside [1, 256], a null buffer that is needed.  B == 0 and an empty index are valid. */
int sqe_index_search_filtered_each(sqe_index* idx, const float* q_host, int B, int k,
                                   const int64_t* allow_ids_host, const int64_t* list_offsets_host, int n_lists,
                                   const int32_t* list_of_query_host, float* cos_out_host, int64_t* id_out_host);
int sqe_index_search_filtered_each_device(sqe_index* idx, const float* q_dev, int B, int k,
                                          const int64_t* allow_ids_dev, const int64_t* list_offsets_host, int n_lists,
                                          const int32_t* list_of_query_host, float* cos_out_dev, int64_t* id_out_dev);

/* Exclusion search: query b is answered over every live row EXCEPT those on its own deny-list (hits already shown on an earlier
 * page, the document being read, a must_not on an id).  List f is deny_ids[list_offsets[f] .. list_offsets[f + 1]), query b
 * names list list_of_query[b]; -1 means "no list": that row is bit for bit the row sqe_index_search returns.  Any number of
 * queries may name one list and a list may be named by none.  list_offsets [n_lists + 1] and list_of_query [B] are HOST memory
 * in both forms and are not retained past return.
 * Row b: take the exact ranking of all live rows as sqe_index_search defines it (fp32 cosine descending, ties to the lowest id;
 * the cosine is bit for bit the one sqe_index_search returns for the row), remove the rows whose id is on the list, return the
 * first k, padded with (-inf, -1).  Ids follow the rules of search (stable after deletes, id_base added, global on a device
 * group).  Deny ids are local ids as for sqe_index_delete (global ids on a device group); a list may be in any order and may
 * repeat ids; ids that name no live row (deleted, never assigned, >= next_id, negative) are skipped, and an empty list excludes
 * nothing.  Always exact with "certify" = 1, for FLAT and IVF indexes and device groups; an IVF index answers the queries that
 * name a list over every live row (no nprobe), as filtered, radial and collapsed search do.  A query's answer depends on the
 * query, its list and the index only: not on B, its place in the batch, the other lists or "exclude_depth".
 * How (csrc/exclude.hip): the deny ids become row positions on the device and go into one hash set of positions per list
 * (memory proportional to the number of entries; built without reading anything back; nothing is retained).  A FLAT index then
 * runs the certified search at depth min(256, k + list length) -- "exclude_depth" (option; 0 = that rule, else 1..256, raised
 * to k) caps it -- in at most two searches per 1024 queries, the queries whose depth is <= "i8_sample_m" (they keep the int8
 * first pass of a large index) and the rest, and drops the denied hits.  With "certify" = 0 that stage is as approximate as the
 * search it runs.  A query left with fewer than k hits although the index holds more rows than were fetched (k + list length
 * > 256, or a smaller "exclude_depth") -- and every query of an IVF index that names a list -- is answered by the sweep of
 * collapsed search with "denied" in place of "key already seen"; it holds at most "range_key_budget" collected keys.
 * sqe_exclude_swept reports the queries of the last call that the sweep answered.
 * Synchronisation: the _device form synchronises the context stream once after the first stage (the number of incomplete
 * queries comes back) and once per row range of the sweep; on a device group it first copies the ids to the host.  The owner's
 * search state is left as plain searches of those depths leave it.  Times are booked under prep_ms, scan_ms and select_ms.  An
 * index that never gets this call allocates nothing for it.
 * Measured (profiles/exclude/NOTES.md; one device, 10 M x 1024 FLAT, k = 10): 5 denied ids per query cost 0.06-0.11 ms over
 * the plain search of depth 15 (1.79 ms at B = 1, 9.17 ms at B = 1024), 14 x / 4.6 x less than the allow-list of everything
 * else; a forced sweep of 64 queries 6.9 ms; a stage at depth 256 for 64 queries (k + list length > 256) 33 ms, which is MORE
 * than that allow-list's 26 ms.  Device groups and IVF indexes were not measured.
 * SQE_ERR_INVALID, with nothing written: list_offsets not starting at 0 or decreasing, n_lists < 0, a list_of_query entry
 * outside [-1, n_lists), k outside [1, 256], a null buffer that is needed, more than 2^32 rows.  B == 0 and an empty index are
 * valid. */
int sqe_index_search_excluding(sqe_index* idx, const float* q_host, int B, int k,
                               const int64_t* deny_ids_host, const int64_t* list_offsets_host, int n_lists,
                               const int32_t* list_of_query_host, float* cos_out_host, int64_t* id_out_host);
int sqe_index_search_excluding_device(sqe_index* idx, const float* q_dev, int B, int k,
                                      const int64_t* deny_ids_dev, const int64_t* list_offsets_host, int n_lists,
                                      const int32_t* list_of_query_host, float* cos_out_dev, int64_t* id_out_dev);

/* Radial search: per query b, the live rows whose fp32 cosine is >= min_cos[b].
 * Queries are normalised as for sqe_index_search, and a row's cosine c is bit for bit the value sqe_index_search would
 * return for it (same normalised query, same fp32 re-score chain).  A row matches query b iff c >= min_cos[b].
 *   count_out [B] int64: the exact number of matches; it does not depend on max_hits.
 *   cos_out / id_out [B, max_hits]: the best min(count, max_hits) matches, best first, ties to the lowest id, padded with
 *   (-inf, -1).  Ids follow the rules of search: stable ids after deletes, id_base added, global ids on a device group.
 * 0 <= max_hits <= 10000; with max_hits == 0 only counts are produced and cos_out / id_out may be NULL.  Thresholds are per
 * query; a NaN threshold is SQE_ERR_INVALID, -inf matches every live row, +inf none.  B == 0 and an empty index are valid.
 * Always exact, whatever the data: a bf16 collect scan gathers every row whose scan score reaches min_cos - eps (the error
 * bound of the certificate) and the gathered rows are re-scored in fp32; "certify" and "rescore_k" do not apply.  FLAT and
 * IVF indexes alike are answered over every live row (no nprobe).  Batches above 1024 run in passes.
 * Memory: option "range_key_budget" (default 2^25, >= 4096) bounds the keys held at once: queries are collected in groups
 * of range_key_budget / 4096 (at most 1024), whatever the number of matches.  A query with more than 4096 candidates is
 * scanned again over row ranges sized from its count (halved when a range overflows, doubled when one comes in well under),
 * so a threshold that matches millions of rows stays exact and bounded, at the cost of one launch sequence and one
 * read-back per range (slow: see profiles/range/NOTES.md).  An index that never gets a radial search allocates nothing for it.
 * Synchronisation: the _device form reads the thresholds back once (NaN check), then synchronises the context stream once
 * per group of queries and once per row range of the queries that overflowed their buffer.  The owner's search state
 * (candidate lists, fallback buffers, int8 counters) is untouched.  Times are booked under scan_ms and select_ms. */
int sqe_index_range_search(sqe_index* idx, const float* q_host, int B, const float* min_cos_host,
                           int max_hits, int64_t* count_out_host, float* cos_out_host, int64_t* id_out_host);
int sqe_index_range_search_device(sqe_index* idx, const float* q_dev, int B, const float* min_cos_dev,
                                  int max_hits, int64_t* count_out_dev, float* cos_out_dev, int64_t* id_out_dev);

/* Group keys and collapsed search (OpenSearch `collapse` on a field, the group-by of other engines): per query the k best
 * GROUPS and each group's best row, so that the chunks of one document answer as one hit.
 * Every live row may carry an int64 key; a row without one (SQE_KEY_NONE) is a group by itself.  Take the exact ranking of all
 * live rows as sqe_index_search defines it (fp32 cosine descending, ties to the lowest id; the cosine is bit for bit the one
 * sqe_index_search returns for that row), walk it and keep the first row of every key: the first k rows kept are the answer,
 * in that order.  An index whose rows all lack keys returns exactly what sqe_index_search returns.
 *   sqe_index_set_keys: ids are local ids as for sqe_index_delete (global ids on a device group).  Every id must be live, else
 *     SQE_ERR_INVALID and nothing is written.  A repeated id: the last key wins.  SQE_KEY_NONE removes a key.  Keys stay with
 *     their rows through sqe_index_update, deletes and growth; appended rows start without a key.
 *   sqe_index_get_keys: the keys of the given live ids (SQE_KEY_NONE where none is set).
 *   Keys are NOT written by sqe_index_save: a loaded index has none, and its owner sets them again (the Python client re-derives
 *     them from its document store).  An index that never sets a key allocates nothing for them and saves the same file as before.
 *   sqe_index_search_collapsed: cos_out / id_out / key_out [B, k], padded with (-inf, -1, SQE_KEY_NONE) when the index holds fewer
 *     than k groups.  Ids follow the rules of search (stable after deletes, id_base added, global on a device group).
 *     1 <= k <= 256; B == 0 and an empty index are valid.  Always exact, on any data, for FLAT and IVF indexes and device groups;
 *     an IVF index is answered over every live row (no nprobe), as for filtered and radial search.
 * How: a FLAT index first runs the certified search at depth "collapse_depth" (option; 0 = automatic min(256, max(64, 4 k)),
 * else 1..256, raised to k; a depth <= "i8_sample_m" keeps the int8 first pass on large indexes) and folds its hits by key; with
 * "certify" = 0 that stage is as approximate as the search it runs.  A query that found fewer than k groups there -- and every
 * query of an IVF index -- is answered by a sweep over all live rows: bf16 collect scans of row ranges at the running k-th group
 * cosine - eps, fp32 re-score, best row per key (csrc/collapse.hip).  The sweep holds at most "range_key_budget" collected keys.
 * sqe_collapse_swept reports the queries of the last collapsed search that the sweep answered.
 * Synchronisation: the _device form synchronises the context stream once after the first stage (the number of incomplete
 * queries comes back) and once per row range of the sweep.  The owner's search state is left as a plain search of depth
 * collapse_depth leaves it.  Times are booked under scan_ms and select_ms. */
#define SQE_KEY_NONE INT64_MIN
int sqe_index_set_keys(sqe_index* idx, const int64_t* ids_host, const int64_t* keys_host, int64_t n);
int sqe_index_get_keys(sqe_index* idx, const int64_t* ids_host, int64_t n, int64_t* keys_out_host);
int sqe_index_search_collapsed(sqe_index* idx, const float* q_host, int B, int k,
                               float* cos_out_host, int64_t* id_out_host, int64_t* key_out_host);
int sqe_index_search_collapsed_device(sqe_index* idx, const float* q_dev, int B, int k,
                                      float* cos_out_dev, int64_t* id_out_dev, int64_t* key_out_dev);

/* Numeric fields and field predicates: per-row int64 columns on the device, and filters over them that never leave it
 * ("published in 2015 or later", "this user's chunks", "journal in this set").
 * Fields.  An index has SQE_MAX_FIELDS slots, 0..7.  A slot's column is an int64 per row, allocated by the first
 * sqe_index_set_field of the slot; a row without a value reads SQE_FIELD_NONE.  The rules are those of the group keys:
 *   sqe_index_set_field: ids as for sqe_index_delete (global ids on a device group).  Every id must be live and the slot in 0..7,
 *     else SQE_ERR_INVALID and nothing is written.  A repeated id: the last value wins.  SQE_FIELD_NONE removes a value.  Values
 *     stay with their rows through sqe_index_update, growth and deletes; appended rows start without a value.
 *   sqe_index_get_field: the values of the given live ids (SQE_FIELD_NONE where none is set, and for a slot never set).
 *   sqe_index_field_info: the slots that hold a column and the device bytes of all columns (0 and 0 before the first set_field).
 *   Fields are NOT written by sqe_index_save.  An index that never sets a field allocates nothing, runs the code it ran before
 *     and saves the same bytes.
 *   The device compares int64 only: what a float, a date or a string becomes is the caller's business (the Python layer maps
 *     doubles through an order-preserving image, dates to epoch milliseconds and keywords through a dictionary).
 * Predicates.  A clause tests one field of a row, v being the row's value in slot `field`:
 *   SQE_FOP_RANGE  holds iff the row has a value and lo <= v <= hi.  "Exists" is [INT64_MIN + 1, INT64_MAX]; lo > hi holds nowhere.
 *   SQE_FOP_IN     holds iff the row has a value and v is one of set_values[lo .. hi), a slice that must be strictly ascending.
 *   | SQE_FOP_NOT  negates the clause's result: a row WITHOUT a value passes a negated clause (OpenSearch `must_not`).
 *   A clause on a slot never set is valid and holds for no row (negated: for every row).
 * A predicate is the AND of 0..8 clauses; zero clauses select every live row.  Predicate j of a call owns the clauses
 * pred_offsets[j] .. pred_offsets[j + 1].  clauses, pred_offsets, set_values and pred_of_query are HOST memory in the _device forms
 * too, free to reuse once the call returns.
 * SQE_ERR_INVALID, with nothing written: more than 64 predicates or 4,096 set values in a call, more than 8 clauses in a
 * predicate, offsets that do not start at 0 or decrease, a slot outside 0..7, an unknown op, an IN slice outside [0, n_set] or not
 * strictly ascending, cap < 0, a pred_of_query entry outside [0, n_preds), and what the search calls refuse of B, k and buffers.
 *   sqe_index_match_fields: count_out [n_preds] int64 is the exact number of live rows each predicate selects, whatever cap is;
 *     id_out [n_preds, cap] holds the min(count, cap) lowest selected ids ascending, padded with -1.  With cap == 0 only the
 *     counts are produced and id_out may be NULL.  The _device form synchronises nothing (on a device group the shards' parts
 *     meet on the host, which synchronises them).
 *   sqe_index_search_where: the exact top-k over the live rows the predicate (clauses[0 .. n_clauses)) selects, as
 *     sqe_index_search_filtered answers over their ids, bit for bit.  n_allow >= 0 also restricts the rows to that id list (ids
 *     that name no live row are skipped; an empty list selects nothing); n_allow == -1: no list.  One synchronisation of the
 *     stream, for the number of selected rows M; then one of two routes, chosen per call (and per shard of a device group):
 *       gather  the selected rows are copied into a scratch index and searched there (sqe_index_search_filtered's second half):
 *               nothing else synchronises and the owner's search state is not touched.  Every IVF index, and
 *               sqe_index_search_filtered, _filtered_each and _where_each, always run it.
 *       mask    (FLAT indexes) the whole index is searched at one depth d for the call and the hits whose row the predicate
 *               refuses are dropped; a query left with fewer than k rows although d < the live rows is answered by a sweep over
 *               all rows (as sqe_index_search_excluding's), so the answer is the exact top-k of the selected rows whatever d is.
 *               d = sqe_where_depth(k, M, live): with f = M / live the smallest d in [k, 256] with P[Binomial(d, f) < k] <= 2^-10
 *               in double arithmetic (a pass of 1,024 queries whose selected rows fall independently of them expects at most one
 *               sweep), 0 if there is none or M < k.  One more synchronisation after the first stage and one per row range of a
 *               sweep; the owner's search state is left as a plain search of depth d leaves it (d <= "i8_sample_m" keeps the int8
 *               first pass of a large index, building its int8 copy if need be).  A predicate correlated with the queries costs
 *               sweeps, never a wrong answer.
 *     "where_route" (sqe_index_set_option; default 0): 1 = always gather; 2 = mask whenever the index is FLAT, at depth
 *     sqe_where_depth or 256 where that answers 0 -- with "certify" = 0 as approximate as the search it runs; 0 = mask only if
 *     the index is FLAT, "certify" is on (the answer's bits then never depend on the route), sqe_where_depth is not 0,
 *     M >= "where_mask_min_rows" (default 1,000,000) and a host-side cost rule on (live, M, B, k, d, int8 or bf16 first pass) expects
 *     the mask route to be cheaper (csrc/fieldpred.h; fitted at 10 M x 1024, profiles/where_mask/NOTES.md).
 *     "where_mask_depth" (default 0 = the rule, else 1..256, raised to k) sets d, like "exclude_depth".  A caller with a broad
 *     allow-list and no predicate passes zero clauses.
 *     sqe_index_where_last (test-only, as sqe_index_sort_last; single-device indexes only): of the last call the route
 *     (SQE_WHERE_ROUTE_NONE when nothing was selected), M, the live rows, d, whether the last pass of the first stage ran the
 *     int8 first pass, and the number of swept queries.
 *   sqe_index_search_where_each: query b over the rows of predicate pred_of_query[b], as sqe_index_search_filtered_each answers
 *     over their id lists, bit for bit.  All predicates are evaluated in one pass; the counts come back once (one
 *     synchronisation), then every list takes the direct or the gathered route of that call.
 * FLAT and IVF indexes are served alike (an IVF index over every selected row, no nprobe).  On a device group every shard
 * evaluates the predicate over its own rows and the group merges as for a plain search; only an allow-list is routed.
 * How (csrc/fields.hip): field_match_kernel -- one wave per 64 consecutive rows, one row per lane; the clauses sorted by slot, so
 * a column is read once per row (a coalesced 8-byte load) however many predicates name it; clause table and set values in LDS,
 * IN a binary search there; one bit per predicate and lane, one ballot per predicate, stored by lane 0 -- writes one bitmap per
 * predicate in the layout of the filtered search, whose count / scan / write / gather / search steps then run unchanged (after
 * filter_mark_kernel and ANDed into its map when there is an allow-list).  The mask route (csrc/where_mask.hip) reads the same map:
 * deny_drop_kernel, one wave per query, one bit test per lane, a ballot and a prefix popcount for a survivor's place;
 * deny_merge_kernel in the sweep (csrc/deny_kernels.h: both are exclusion search's kernels with the bit test as the denial).  Not served: OR inside a predicate, predicates in
 * exclusion, fused or hybrid search (radial, collapsed and MMR search take them through the _where calls further below).  Aggregations are served by sqe_index_aggregate_fields and sorting on fields by
 * sqe_index_sort_fields, both below; still out of scope for aggregations: sub-aggregations, float sums, and cardinality beyond
 * 65,536 per shard on a device group. */
#define SQE_FIELD_NONE INT64_MIN
#define SQE_MAX_FIELDS 8
typedef struct { int32_t field; int32_t op; int64_t lo, hi; } sqe_field_clause_t;
enum { SQE_FOP_RANGE = 0, SQE_FOP_IN = 1, SQE_FOP_NOT = 0x100 };
int sqe_index_set_field(sqe_index* idx, int field, const int64_t* ids_host, const int64_t* values_host, int64_t n);
int sqe_index_get_field(sqe_index* idx, int field, const int64_t* ids_host, int64_t n, int64_t* values_out_host);
int sqe_index_field_info(sqe_index* idx, int* n_fields_out, int64_t* device_bytes_out);
int sqe_index_match_fields(sqe_index* idx, const sqe_field_clause_t* clauses, const int64_t* pred_offsets, int n_preds,
                           const int64_t* set_values, int64_t n_set, int64_t cap, int64_t* count_out_host, int64_t* id_out_host);
int sqe_index_match_fields_device(sqe_index* idx, const sqe_field_clause_t* clauses, const int64_t* pred_offsets, int n_preds,
                                  const int64_t* set_values, int64_t n_set, int64_t cap, int64_t* count_out_dev, int64_t* id_out_dev);
int sqe_index_search_where(sqe_index* idx, const float* q_host, int B, int k, const sqe_field_clause_t* clauses, int n_clauses,
                           const int64_t* set_values, int64_t n_set, const int64_t* allow_ids_host, int64_t n_allow,
                           float* cos_out_host, int64_t* id_out_host);
int sqe_index_search_where_device(sqe_index* idx, const float* q_dev, int B, int k, const sqe_field_clause_t* clauses, int n_clauses,
                                  const int64_t* set_values, int64_t n_set, const int64_t* allow_ids_dev, int64_t n_allow,
                                  float* cos_out_dev, int64_t* id_out_dev);
enum { SQE_WHERE_ROUTE_NONE = 0, SQE_WHERE_ROUTE_GATHER = 1, SQE_WHERE_ROUTE_MASK = 2 };
typedef struct { int32_t route, depth, first_pass_i8, pad; int64_t selected, live, swept; } sqe_where_last_t;
int sqe_index_where_last(sqe_index* idx, sqe_where_last_t* out);
int sqe_where_depth(int k, int64_t selected, int64_t live);
int sqe_index_search_where_each(sqe_index* idx, const float* q_host, int B, int k, const sqe_field_clause_t* clauses,
                                const int64_t* pred_offsets, int n_preds, const int64_t* set_values, int64_t n_set,
                                const int32_t* pred_of_query_host, float* cos_out_host, int64_t* id_out_host);
int sqe_index_search_where_each_device(sqe_index* idx, const float* q_dev, int B, int k, const sqe_field_clause_t* clauses,
                                       const int64_t* pred_offsets, int n_preds, const int64_t* set_values, int64_t n_set,
                                       const int32_t* pred_of_query_host, float* cos_out_dev, int64_t* id_out_dev);

/* Radial, collapsed and MMR search within a row set.  Let S be the live rows that clauses[0 .. n_clauses) select, intersected
 * with the allow-list when n_allow >= 0 -- exactly the rows sqe_index_search_where searches (zero clauses with n_allow == -1:
 * every live row; ids that name no live row are skipped; n_allow == 0 selects nothing).  Then
 *   sqe_index_range_search_where      count_out[b] is the exact number of rows of S with fp32 cosine >= min_cos[b], and the best
 *                                     max_hits of them are returned;
 *   sqe_index_search_collapsed_where  walks the exact ranking of the rows of S, keeps the first row of every key, returns the first k;
 *   sqe_index_search_mmr_where        the candidates are the exact top-n of S (sqe_index_search_where at depth n; nprobe is accepted
 *                                     for symmetry and not used: the candidates of a restricted call are exact on every index kind),
 *                                     and the greedy choice runs among them.
 * Each call returns, bit for bit (ids, cosines, keys, counts, MMR scores), what the unrestricted call of its kind returns on a copy
 * of the index from which every row outside S was deleted.  Arguments: those of the unrestricted call, then the row-set arguments
 * of sqe_index_search_where; clauses, set_values and the host arrays of the unrestricted call are host memory in both forms, the
 * allow-list is host memory in the host form and device memory in the _device form.  Argument errors are those of the two calls
 * combined: SQE_ERR_INVALID, nothing written.  One synchronisation of the stream for the size M of S (MMR: per pass, inside its
 * sqe_index_search_where), besides what the kind synchronises.  M == 0: padded outputs and zero counts.  Two routes for radial and
 * collapsed search, chosen per call and per shard of a device group:
 *   gather  (M <= "filter_gather_rows", one chunk of the scratch index of the filtered search) the rows of S, and for collapsed
 *           search their keys, are copied into the scratch index, which inherits "certify", "rescore_k", "collapse_depth",
 *           "range_key_budget" and "mmr_row_budget"; the unchanged search of the kind runs there and its positions are mapped back.
 *           Nothing gathered survives the call.
 *   mask    (FLAT and IVF) the whole index is searched and the row's bit of the predicate's map is tested where a row is decided:
 *           in range_merge_kernel beside the threshold test (a denied row may fill a buffer and cost a walk over row ranges, never
 *           a count or an answer), in collapse_walk_kernel (a head whose bit is clear is passed over) and in collapse_merge_kernel
 *           before the per-key reduction.  Collapsed search on a FLAT index fetches d rows first: with kd the depth an unrestricted
 *           collapsed search takes ("collapse_depth"), d = sqe_where_depth(kd, M, live), or 256 where that answers 0; a query with
 *           fewer than k groups among them although d < live is swept.  An IVF index sweeps every query, as it does unrestricted.
 * "within_route" (sqe_index_set_option; default 0): 0 = gather iff M <= "filter_gather_rows", else mask -- a placeholder, not a
 * fitted rule; 2 = always mask.  MMR adds no route of its own: it takes the route of its sqe_index_search_where ("where_route").
 * On a device group every shard restricts its own rows (only the allow-list is routed) and the parts merge as for the
 * unrestricted calls.  sqe_index_within_last (test-only, single-device indexes only): of the last restricted call its kind
 * (1 radial, 2 collapsed, 3 MMR), route (SQE_WHERE_ROUTE_*; NONE when M == 0), depth (collapsed: rows the first stage fetched, 0 on
 * an IVF index; MMR: n; radial: 0), M, the live rows, and the swept queries (radial: the queries that took the walk).
 * Not served: restrictions under exclusion, fused and hybrid search, one predicate per query, a chunked gather route. */
int sqe_index_range_search_where(sqe_index* idx, const float* q_host, int B, const float* min_cos_host, int max_hits,
                                 const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                                 const int64_t* allow_ids_host, int64_t n_allow, int64_t* count_out_host, float* cos_out_host,
                                 int64_t* id_out_host);
int sqe_index_range_search_where_device(sqe_index* idx, const float* q_dev, int B, const float* min_cos_dev, int max_hits,
                                        const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                                        const int64_t* allow_ids_dev, int64_t n_allow, int64_t* count_out_dev, float* cos_out_dev,
                                        int64_t* id_out_dev);
int sqe_index_search_collapsed_where(sqe_index* idx, const float* q_host, int B, int k, const sqe_field_clause_t* clauses, int n_clauses,
                                     const int64_t* set_values, int64_t n_set, const int64_t* allow_ids_host, int64_t n_allow,
                                     float* cos_out_host, int64_t* id_out_host, int64_t* key_out_host);
int sqe_index_search_collapsed_where_device(sqe_index* idx, const float* q_dev, int B, int k, const sqe_field_clause_t* clauses,
                                            int n_clauses, const int64_t* set_values, int64_t n_set, const int64_t* allow_ids_dev,
                                            int64_t n_allow, float* cos_out_dev, int64_t* id_out_dev, int64_t* key_out_dev);
int sqe_index_search_mmr_where(sqe_index* idx, const float* q_host, int B, int k, int n_cand, const float* lambda_host, int nprobe,
                               const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                               const int64_t* allow_ids_host, int64_t n_allow, float* cos_out_host, int64_t* id_out_host,
                               float* mmr_out_host);
int sqe_index_search_mmr_where_device(sqe_index* idx, const float* q_dev, int B, int k, int n_cand, const float* lambda_host, int nprobe,
                                      const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                                      const int64_t* allow_ids_dev, int64_t n_allow, float* cos_out_dev, int64_t* id_out_dev,
                                      float* mmr_out_dev);
enum { SQE_WITHIN_RADIAL = 1, SQE_WITHIN_COLLAPSED = 2, SQE_WITHIN_MMR = 3 };
typedef struct { int32_t kind, route, depth, pad; int64_t selected, live, swept; } sqe_within_last_t;
int sqe_index_within_last(sqe_index* idx, sqe_within_last_t* out);

/* Field aggregations (OpenSearch `aggs` with "size": 0): stats, terms and histogram facets over the rows a predicate selects,
 * computed on the device from the columns -- no id and no value comes back, only the answer.  Integers throughout: every result
 * is defined exactly and does not depend on the batch, the order of the rows or the route taken.
 * The row set is exactly the one sqe_index_search_where searches: the live rows the predicate (0..8 clauses, AND) selects, also
 * restricted to the allow-list when n_allow >= 0 (ids that name no live row are skipped, an empty list selects nothing).
 * *selected_out is the size of that set.  Each of the n_aggs (1..8) aggregations names a field slot and runs over the selected rows
 * that HAVE a value in it; a slot never set therefore gives count = 0 everywhere.
 *   SQE_AGG_STATS      count = the number of such rows; min / max over them (count == 0: min = INT64_MAX, max = SQE_FIELD_NONE).  The
 *     exact sum is carried as two partial sums, which cannot wrap for fewer than 2^31 rows: sum_lo = the sum of each value's low
 *     32 bits taken unsigned, sum_hi = the sum of v >> 32 (arithmetic); the sum is sum_hi * 2^32 + sum_lo.  n_buckets = other = 0
 *     and no bucket is written.  TERMS and HISTOGRAM fill these five members too.
 *   SQE_AGG_TERMS      the buckets are the distinct values; the best `size` (1 <= size <= 256, size <= bucket_cap) go out ordered
 *     by count descending, ties to the lower value: key_out holds the value, count_out the count.  n_buckets = the exact number of
 *     distinct values, other = count - the returned counts.
 *   SQE_AGG_HISTOGRAM  interval >= 1, 0 <= offset < interval; the bucket of v is floor((v - offset) / interval), computed without
 *     wrap-around.  Every bucket from the lowest occupied to the highest occupied goes out ascending, the empty ones in between
 *     with count 0; key_out = bucket * interval + offset (two's complement: it can leave int64 only for the lowest bucket of values
 *     within `interval` of INT64_MIN).  n_buckets = kmax - kmin + 1 (0 without a value), other = 0.  More than
 *     min(bucket_cap, 16384) buckets: SQE_ERR_INVALID with a message that names the bucket count (OpenSearch's too_many_buckets);
 *     selected_out and result_out are then still written (the stats of every aggregation and the n_buckets of the histograms;
 *     n_buckets and other of a TERMS aggregation read 0) and no bucket is.
 * key_out / count_out are [n_aggs, bucket_cap] int64 on the host, row j for aggregation j; the places no bucket takes hold
 * (SQE_FIELD_NONE, 0), the whole row of a STATS aggregation too.  With bucket_cap == 0 both may be NULL.
 * SQE_ERR_INVALID, with nothing written: what sqe_index_search_where refuses of clauses and lists, n_aggs outside 1..8, an unknown
 * kind, a slot outside 0..7, a bad size, interval or offset, bucket_cap < 0, a null buffer.  An empty index answers zeros and padding.
 * FLAT and IVF indexes are served alike (the columns are by row position; no list is involved).
 * Device groups: every shard aggregates its own rows (only the allow-list is routed) and ALL of its buckets come to the host,
 * where STATS and HISTOGRAM merge exactly and TERMS adds the shards' counts per value and ranks by (count desc, value asc): the
 * answers are the single index's, bit for bit.  A shard returns the occupied slots of its table through a compaction of at most
 * 65,536 entries: a shard with more than 65,536 distinct values of a TERMS field makes the call answer SQE_ERR_UNSUPPORTED, with a
 * message that says so and nothing written.
 * On one device the call synchronises the index's stream twice: once for the stats, which choose the routes, once for
 * the buckets.
 * How (csrc/aggregate.hip): the bitmap of sqe_index_search_where, read and not changed; agg_stats_kernel (one pass, a lane per row,
 * every named column read once, wave and block reduction, one partial per block, folded by one block); then per TERMS / HISTOGRAM
 * aggregation a count pass -- dense (TERMS with max - min + 1 <= 16384, every HISTOGRAM): private LDS tables of u32 counters per
 * workgroup, added into one global table; hash (every other TERMS): an open-addressing table in HBM of the power of two >= 2 x count
 * and >= 1024 slots, 64-bit CAS on the key, linear probing -- and for TERMS a block radix select per 16,384 slots by (count desc,
 * value asc) plus a one-block merge.
 * sqe_index_aggregate_last (test-only, as sqe_index_delete_last): per aggregation of the last successful call the route taken,
 * the key span (max - min + 1, or the histogram's buckets; 0 on SQE_AGG_ROUTE_NONE), the table slots, the select blocks launched
 * and, of those, the blocks that held an occupied slot and so sent candidates to the merge (TERMS only).  Single-device indexes only. */
enum { SQE_AGG_STATS = 0, SQE_AGG_TERMS = 1, SQE_AGG_HISTOGRAM = 2 };
enum { SQE_AGG_ROUTE_NONE = 0, SQE_AGG_ROUTE_DENSE = 1, SQE_AGG_ROUTE_HASH = 2 };
typedef struct { int32_t kind, field; int32_t size, pad; int64_t interval, offset; } sqe_field_agg_t;
typedef struct { int64_t count, min, max, sum_lo, sum_hi, n_buckets, other; } sqe_field_agg_result_t;
typedef struct { int32_t route, select_blocks; int64_t span, slots; int32_t occupied_blocks, pad; } sqe_agg_route_t;
typedef struct { int32_t n_aggs, pad; sqe_agg_route_t agg[8]; } sqe_agg_last_t;
int sqe_index_aggregate_fields(sqe_index* idx, const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                               const int64_t* allow_ids_host, int64_t n_allow, const sqe_field_agg_t* aggs, int n_aggs, int64_t bucket_cap,
                               int64_t* selected_out, sqe_field_agg_result_t* result_out, int64_t* key_out, int64_t* count_out);
int sqe_index_aggregate_last(sqe_index* idx, sqe_agg_last_t* out);

/* Sorting on fields (OpenSearch `sort` with `search_after`): the first k rows, in the order of 1..4 field keys, of the rows a
 * predicate selects -- "the 10 newest chunks of this user", "this journal's papers by impact, page 3" -- computed on the device
 * from the columns.  Integers throughout: every result is defined exactly and compared bit for bit.
 * Row set.  Exactly the one sqe_index_search_where searches: the live rows the predicate (0..8 clauses, AND) selects, also
 * restricted to the allow-list when n_allow >= 0 (ids that name no live row are skipped, an empty list selects nothing).
 * *total_out is the size of that set, whatever the cursor is (OpenSearch hits.total).
 * Order.  Key j names a field slot, a direction (SQE_SORT_DESC, else ascending) and where the rows without a value go: last
 * by default (OpenSearch `_last`), first with SQE_SORT_MISSING_FIRST; neither placement depends on the direction.  As an image:
 * for a present value v (never INT64_MIN) let b = (uint64)v ^ 2^63, which lies in [1, 2^64 - 1];
 *                            u of a present value     u of a missing value
 *     asc,  missing last     b - 1                    2^64 - 1
 *     asc,  missing first    b                        0
 *     desc, missing last     ~b                       2^64 - 1
 *     desc, missing first    -b (mod 2^64)            0
 * and rows are ordered by the tuple (u_0, ..., u_{n_sort - 1}, id) ascending.  The id is the final tie-break, so the order is
 * total and no result depends on the batch, the route or the arrival order of waves.  A slot never set is valid: every row is
 * missing there, so that key ties everywhere.
 * Cursor (search_after).  after_values == NULL: no cursor.  Otherwise after_values [n_sort] holds raw field values, SQE_FIELD_NONE
 * for "missing", and after_id an id: only the rows whose tuple is strictly greater than the cursor's tuple qualify.  The cursor
 * need not name a live row, so paging survives deletes between pages.
 * Output.  id_out [k] holds the first min(k, qualifying) ids in order, padded with -1; value_out [k, n_sort] their raw values in
 * the sort slots, SQE_FIELD_NONE where missing and in the padding.  1 <= k <= 256.  All three outputs are host memory.
 * SQE_ERR_INVALID, with nothing written: what sqe_index_search_where refuses of clauses and lists, n_sort outside 1..4, a slot
 * outside 0..7, a slot named twice, unknown flag bits, k outside 1..256, a null output buffer.  An empty index, or n_allow == 0,
 * answers total = 0 and padding.
 * FLAT and IVF indexes are served alike (the columns are by row position; no list is involved).  One synchronisation of the
 * index's stream per call on one device.
 * Device groups: every shard sorts its own rows (only the allow-list is routed) and returns its k best with global ids and its
 * count; the leader merges them by the same tuple order and sums the counts: the single index's answer, bit for bit.
 * How (csrc/sort.hip): the bitmap of sqe_index_search_where, read and not changed.  sort_slab_kernel: one workgroup per slab of
 * 16,384 row positions, a wave per 64-row unit, a lane per row; zero bitmap words are skipped; a row is alive if its bit is set
 * and its tuple lies after the cursor; the set bits add into one 64-bit counter (the total) before the cursor test.  A slab with
 * more than k alive rows runs a lexicographic select: at level j the (still wanted)-th smallest u_j among the alive rows, by the
 * 64-bit block radix select over ~u_j (that select finds the largest keys and reads key 0 as "no key": ~u is 0 only for
 * u = 2^64 - 1, and its answer "fewer keys than wanted", 0, then complements to exactly that image); the rows below it win; the
 * rows equal to it win too if that is no more than what is wanted, else they are the alive set of level j + 1; after the last
 * key the lowest positions win -- ids ascend with positions.  sort_merge_kernel: one workgroup per group of up to "sort_fan_in"
 * (sqe_index_set_option, 2..64, default 64) candidate lists, the same select over tuples, level after level until one list is
 * left (10 M rows: 611 slabs -> 10 -> 1); the last level ranks its winners by counting with the full tuple comparison and
 * writes ids and raw values.
 * Not served: an order on keyword strings (the Python layer's dictionary codes are in order of first appearance), a score as a
 * sort key, sorting the hits of a k-NN search, more than 4 keys, windows beyond 256 rows (page with the cursor), fields in a
 * saved index.
 * sqe_index_sort_last (test-only, as sqe_index_aggregate_last): of the last successful call the slabs launched, the slabs that
 * held an alive row, the merge levels run, the fan-in used and the candidate tuples the slab pass wrote.  Single-device indexes only. */
enum { SQE_SORT_DESC = 1, SQE_SORT_MISSING_FIRST = 2 };
typedef struct { int32_t field; int32_t flags; } sqe_field_sort_t;
typedef struct { int32_t slabs, slabs_occupied, merge_levels, fan_in; int64_t candidates; } sqe_sort_last_t;
int sqe_index_sort_fields(sqe_index* idx, const sqe_field_clause_t* clauses, int n_clauses, const int64_t* set_values, int64_t n_set,
                          const int64_t* allow_ids_host, int64_t n_allow, const sqe_field_sort_t* sort, int n_sort, int k,
                          const int64_t* after_values, int64_t after_id,
                          int64_t* total_out, int64_t* id_out, int64_t* value_out);
int sqe_index_sort_last(sqe_index* idx, sqe_sort_last_t* out);

/* MMR search (maximal marginal relevance; OpenSearch `ext.mmr` on a k-NN query): a greedy, diversified choice of k rows among
 * the exact top-n, by what the vectors say.  For a query q, a depth n, k <= n and a weight lambda in [0, 1]:
 *   1. Candidates: exactly what sqe_index_search(q, k = n, nprobe) returns, in its order: cosines c_0 >= c_1 >= ..., ties to the
 *      lowest id.  "certify", "rescore_k", "scan_mode" and nprobe act on this stage as on a plain search; fewer than n live rows
 *      give fewer candidates.  On an IVF index they are therefore the IVF search's rows, approximate as that search is: it
 *      re-scores min(256, max(32, 4 n)) estimated rows, so at n = 256 nothing is left over for the estimates' error.
 *   2. Row similarity: s(i, j) = the fp32 dot product of the stored normalised fp32 rows of candidates i and j (a k-ordered
 *      fmaf chain; within 2e-6 of the float64 dot product of those rows).
 *   3. Greedy choice: S = {}, pen(i) = 0.  Step t = 0 .. k-1 picks the candidate i not in S with the largest
 *      obj(i) = lambda c_i - (1 - lambda) pen(i), evaluated in fp32 (two products, one subtraction, each rounded), ties to the
 *      lower rank; then i joins S and pen(j) = s(j, i) at t = 0, else max(pen(j), s(j, i)).  So the first pick is the best
 *      hit, lambda = 1 returns the plain top-k, and the first k' picks of a k-run are the k'-run (prefix-stable).
 *   4. Outputs [B, k] in selection order: cos_out = c_i, bit for bit the value sqe_index_search returns for that row; id_out
 *      under the id rules of search (stable after deletes, id_base added, global on a device group); mmr_out = obj(i) at the
 *      step that chose i; padded with (-inf, -1, -inf) where fewer than k candidates exist.
 *   5. A query's answer is a pure function of the query, the index and the options: it does not depend on B, on the query's
 *      place in the batch or on "mmr_row_budget", and a device group answers as a single device over the same rows.
 * lambda_host [B] is per query and is HOST memory in both forms: the _device form reads nothing back and does not synchronise
 * the stream.  A NaN or a value outside [0, 1] is SQE_ERR_INVALID and nothing is written.  1 <= k <= 256; n_cand == 0 means
 * automatic, min(256, max(32, 4 k)), else k <= n_cand <= 256.  B == 0 and an empty index are valid.
 * How (csrc/mmr.hip): the search at depth n into scratch, G = R R^T per query on the f32-input MFMA (rows read in place from
 * the fp32 master copy through an index table), then one wave per query runs the k steps.  Batches above
 * "mmr_row_budget" / n queries (option, default 65536 rows, so 256 queries at n = 256) run in passes; the scratch of a pass is
 * n (n + 5) 4 bytes per query, at most 64.3 MiB (at n = 256) at the default.  On a device group every shard returns its top-n with the rows
 * themselves, the leader merges them into the global top-n and runs the same two kernels over the gathered rows; a pass there
 * is budget / (n P) queries, so the leader's gather buffer holds at most budget x dim x 4 bytes.  An index that never gets an
 * MMR search allocates nothing for it.  Times are booked under scan_ms (the search) and select_ms (Gram and choice). */
int sqe_index_search_mmr(sqe_index* idx, const float* q_host, int B, int k, int n_cand, const float* lambda_host, int nprobe,
                         float* cos_out_host, int64_t* id_out_host, float* mmr_out_host);
int sqe_index_search_mmr_device(sqe_index* idx, const float* q_dev, int B, int k, int n_cand, const float* lambda_host, int nprobe,
                                float* cos_out_dev, int64_t* id_out_dev, float* mmr_out_dev);

/* Fused multi-query search (several vectors for one question -- the query and its rephrasings, the sentences of a long question --
 * and ONE ranked list back; OpenSearch `hybrid` over knn sub-queries): reciprocal rank fusion or the best cosine over the exact
 * top-n of every sub-query.  One call carries G logical queries.  Logical query g owns the sub-queries q[offsets[g] ..
 * offsets[g+1]) of the flat [Bs, dim] array q (Bs = offsets[G]); m_g is their number.  offsets [G+1] is HOST memory in both
 * forms, starts at 0 and does not decrease; m_g == 0 is valid and gives all padding.
 *   1. Lists: list j of a group is exactly what sqe_index_search(q_j, k = n, nprobe) returns, in its order.  Ranks are 1-based;
 *      (-inf, -1) padding entries are skipped.  "certify", "scan_mode", "rescore_k" and nprobe act on this stage as on a plain
 *      search (so on an IVF index the lists are the IVF search's, approximate as that search is).  1 <= k <= n <= 256; n == 0
 *      means automatic: k for SQE_FUSE_MAX, min(256, max(32, 4 k)) for SQE_FUSE_RRF.  0 <= m_g <= 32 and m_g * n <= 2048.
 *   2. SQE_FUSE_MAX: fused(x) = the largest cosine of row x over the lists that hold it, an fp32 value compared as a float
 *      (should both zeros occur, +0 is the one reported).  Because n >= k this is the exact top-k of max_j cos(q_j, x) over all
 *      live rows whenever stage 1 is exact.  weights must be NULL; rank_constant is not read.
 *      SQE_FUSE_RRF: fused_int(x) = sum over the lists j that hold x of T(w_j, r_j(x)), T(w, r) = llrint(ldexp((double)w /
 *      (double)(c + r), 40)): an IEEE double division, round half to even.  w_j is a per-sub-query fp32 weight in (0, 64]
 *      (weights [Bs], HOST memory in both forms; NULL = all 1), c = rank_constant, 1 <= c <= 10000.  The sum is an unsigned
 *      64-bit integer below 2^50, so it does not depend on the order of addition.  fused(x) = (float)((double)fused_int * 2^-40).
 *   3. Ranking: fused_int descending (RRF), fused descending (MAX), ties to the lowest id as returned (after id_base, global on a
 *      device group).
 *   4. Outputs [G, k]: fused_out = fused(x); id_out under the id rules of search; cos_out = the row's best cosine over the
 *      lists that hold it, bit for bit a value sqe_index_search returned; padded with (-inf, -1, -inf) where fewer than k
 *      distinct rows exist.
 *   5. A group's answer depends on its sub-queries, weights, the parameters and the index only: not on G, on its place in the
 *      batch or on the other groups.  Permuting a group's sub-queries together with their weights changes no bit.  m = 1 with
 *      SQE_FUSE_MAX is sqe_index_search(q, k) bit for bit; a sub-query repeated in SQE_FUSE_MAX changes nothing; a device group
 *      answers as a single device over the same rows.
 * SQE_ERR_INVALID, with nothing written: offsets that do not start at 0 or decrease, m_g > 32, m_g * n > 2048, k or n out of
 * range, weights given with SQE_FUSE_MAX, a NaN or out-of-range weight, rank_constant out of range (RRF), an unknown mode.
 * G == 0 and an empty index are valid.  The _device form reads nothing back and does not synchronise the stream.
 * How (csrc/fuse.hip): the search of all Bs sub-queries at depth n into scratch, then one workgroup per logical query: the
 * group's m n entries go into an open-addressing table in LDS keyed by the 64-bit id (64-bit compare-and-swap, integer add,
 * ordered-integer max: no floating-point accumulation order exists), a radix select finds the k-th score, the rows at or above
 * it are ranked by (score, id).  On a device group stage 1 is the group's plain search (global ids on the leader) and the same
 * kernel runs on the leader.  An index that never gets a fused search allocates nothing for it.  Times are booked under
 * scan_ms (the search) and select_ms (the fuse kernel). */
enum { SQE_FUSE_MAX = 0, SQE_FUSE_RRF = 1 };
int sqe_index_search_fused(sqe_index* idx, const float* q_host, int G, const int64_t* offsets_host, int k, int n, int mode,
                           int rank_constant, const float* weights_host, int nprobe, float* fused_out_host, int64_t* id_out_host,
                           float* cos_out_host);
int sqe_index_search_fused_device(sqe_index* idx, const float* q_dev, int G, const int64_t* offsets_host, int k, int n, int mode,
                                  int rank_constant, const float* weights_host, int nprobe, float* fused_out_dev,
                                  int64_t* id_out_dev, float* cos_out_dev);

/* IVF only: k-means (spherical, Lloyd) on a sample, then (re)assignment of stored rows. */
int sqe_index_train(sqe_index* idx, const float* x_host, int64_t n, int iters, uint64_t seed);
int sqe_index_train_device(sqe_index* idx, const float* x_dev, int64_t n, int iters, uint64_t seed);
/* IVF introspection: normalised centroids [nlist, dim] and the list of every live row [count], in ascending id
 * order (either pointer may be NULL). */
int sqe_index_ivf_export(sqe_index* idx, float* centroids_host, int32_t* assign_host);

/* INT8_RESCORE introspection (tests/test_i8_gpu.py: the bit-exact parity check of the int8 kernels' integer arithmetic -- the
 * set of keys one collect launch appended against {(acc * s, row) : acc * s >= thr} recomputed from the same int8 operands in
 * NumPy).  These buffers speak row POSITIONS (0 .. count-1, in ascending id order), not ids: after a delete the two
 * differ (sqe_index_ids maps one to the other).  sqe_index_i8_last describes the LAST search this index answered with the int8 first pass (SQE_ERR_STATE if
 * there was none); sqe_index_i8_read copies one of the device buffers that search read or wrote to the host, `bytes` bytes
 * from byte offset `offset`.  The buffers are overwritten by the next search.  Single-device FLAT indexes only.
 *   SQE_I8_ROWS        int8 copy of the rows, TILED: tile t (tile_rows rows) at t * tile_stride bytes; inside a tile the 64-element
 *                      slice h of row r at h * tile_rows * 64 + r * 64
 *   SQE_I8_ROW_SCALES  uint32 [tiles * tile_rows]: the integer scale of each row (one value per tile)
 *   SQE_I8_QUERIES     int8 [b_pad][q_pitch]: the quantised queries, row-major (rows >= B are zero)
 *   SQE_I8_THRESHOLDS  int32 [b_pad]: collect threshold of each query on acc * scale
 *   SQE_I8_LIST_COUNTS int32 [n_chunks][b_pad]: keys APPENDED to each (chunk, query) list (the first list_cap of them are in the
 *                      list, the rest went to the query's overflow pool)
 *   SQE_I8_LISTS       uint64 [n_chunks][b_pad][list_cap]: keys, (score ^ 0x80000000) << 32 | (0xFFFFFFFF - row), unordered
 *   SQE_I8_POOL_COUNTS int32 [b_pad]: keys that found their (chunk, query) list full and went to the query's overflow pool
 *   SQE_I8_POOLS       uint64 [b_pad][pool_cap]: those keys
 *   SQE_I8_SAMPLE_BEST int32 [sample_chunks][sample_b_pad][8 row lanes][2][2]: threshold pass, the two best (score, row) of each
 *                      lane stream (row lane l of a sampled tile: rows (l >> 2) * 128 + (l & 3) * 4 + 16 i + j, i < 8, j < 4)
 *   SQE_I8_QUERIES_TILED int8 [ceil(b_pad / 256)][dim / 64][256][64]: the same quantised queries in blocks of 256, the 64-element
 *                      slice h of query r of block qb at ((qb * dim / 64 + h) * 256 + r) * 64 (queries >= B are zero): the copy the
 *                      256-query kernels and the threshold pass read
 *   SQE_I8_THR_EFF     float [b_pad]: the estimated score (thr_int * S0^2 * sqi, rounded up) that every uncollected row stays below;
 *                      +inf for padding queries
 *   SQE_I8_SAMPLE_COS  float [B][sample_m]: threshold pass, fp32 cosines of the best sample rows, best first, ties to the lower row:
 *                      min(k, sample values) entries in the int8 form, up to sample_m in the bf16 form, then -inf.  An fp32 cosine here
 *                      and in every re-score is a 64-lane fmaf chain over the stored fp32 row and SQE_STATE_QN, within 2e-6 of the
 *                      exact product of the two
 *   SQE_I8_SAMPLE_IDS  int64 [B][sample_m]: their row positions, -1 for padding
 * Only after a search with the option "i8_keep_select" on (SQE_ERR_STATE otherwise), copied between select_i8_kernel and the bf16
 * collect pass:
 *   SQE_I8_SELECT_COS  float [B][k]   } what select_i8_kernel itself wrote as the answer (position + id_base; for a certified query
 *   SQE_I8_SELECT_IDS  int64 [B][k]   } this IS the answer)
 *   SQE_I8_SELECT_THR  float [b_pad]: collect_thr as it left it, +inf = certified (entries at or past B are never written)
 *   SQE_I8_SELECT_TRACE int32 [B][4]: keys gathered (capped at the 12288 the kernel holds), rows that got a bf16 estimate (capped at
 *                      4096), rows re-scored in fp32, flags: 1 = a list pool, the key buffer or the estimate buffer overflowed,
 *                      2 = answered from the sample (fewer than k rows reached the fp32 re-score), 4 = certified */
typedef struct sqe_i8_launch_t {
    int64_t rows;          /* rows scanned */
    int64_t tile_stride;   /* bytes between tiles of the int8 copy */
    int32_t dim, B, b_pad, k;
    int32_t tile_rows;     /* 256 */
    int32_t q_pitch;       /* bytes between quantised query rows */
    int32_t query_block;   /* queries per workgroup: 256 (ping-pong kernel, five-stage for one block), 128 or 64 (streaming or staged kernels: see `kernel`) */
    int32_t n_chunks;      /* row chunks of the collect launch: chunk c holds tiles [c * (T / n) + min(c, T % n), ...), T tiles dealt out evenly */
    int32_t list_cap;      /* slots per (chunk, query) list */
    int32_t sample_int8;   /* 1: the threshold pass ran in int8 (SQE_I8_SAMPLE_BEST is valid) */
    int32_t sample_step;   /* the threshold pass scanned tiles 0, step, 2 step, ... (whole tiles only) */
    int32_t sample_tiles, sample_chunks, sample_b_pad, sample_m;
    int32_t uncertified;   /* queries that went on to the bf16 collect pass (its launches write buffers of their own: the lists, counts and pools stay the int8 scan's) */
    int32_t pool_cap;      /* slots of a query's overflow pool */
    int32_t kernel;        /* SQE_I8_KERNEL_*: the kernel the collect launch ran, filled by the code that picked it */
} sqe_i8_launch_t;
/* scan_i8.hip: the ping-pong kernel (several 256-query blocks), its five-stage build (one block), the streaming kernels
 * <queries per workgroup, ring fragments> and the staged kernels of 64 / 128 queries */
enum { SQE_I8_KERNEL_PP = 1, SQE_I8_KERNEL_DEEP, SQE_I8_KERNEL_STREAM_64_32, SQE_I8_KERNEL_STREAM_64_16, SQE_I8_KERNEL_STREAM_128_16,
       SQE_I8_KERNEL_STAGED_64, SQE_I8_KERNEL_STAGED_128 };
enum { SQE_I8_ROWS = 0, SQE_I8_ROW_SCALES = 1, SQE_I8_QUERIES = 2, SQE_I8_THRESHOLDS = 3, SQE_I8_LIST_COUNTS = 4, SQE_I8_LISTS = 5,
       SQE_I8_SAMPLE_BEST = 6, SQE_I8_POOL_COUNTS = 7, SQE_I8_POOLS = 8, SQE_I8_QUERIES_TILED = 9, SQE_I8_THR_EFF = 10,
       SQE_I8_SAMPLE_COS = 11, SQE_I8_SAMPLE_IDS = 12, SQE_I8_SELECT_COS = 13, SQE_I8_SELECT_IDS = 14, SQE_I8_SELECT_THR = 15,
       SQE_I8_SELECT_TRACE = 16 };
int sqe_index_i8_last(sqe_index* idx, sqe_i8_launch_t* out);
int sqe_index_i8_read(sqe_index* idx, int what, int64_t offset, void* out_host, int64_t bytes);
/* SQE_I8_ROWS and SQE_I8_ROW_SCALES are readable whenever the int8 copy exists, also when no search was answered by the int8
 * first pass (an index whose rows exceed "i8_max_resid" builds the copy and answers in bf16): their extent is then
 * ceil(i8_rows / 256) tiles of i8_tile_stride bytes, both reported by sqe_index_state. */

/* bf16 first-pass introspection (tests/test_scan_stages_gpu.py: every candidate key, every column of the bound table and every
 * dropped row of ONE launch of the bf16 scan with the fused top-k filter -- csrc/scan.hip, scan_pp.hip, scan_common.h -- against a
 * float64 product of the library's own bf16 copies).  Test-only, with the rules of the int8 entries above: single-device FLAT
 * indexes only (SQE_ERR_UNSUPPORTED otherwise), row POSITIONS, one stream synchronisation per call, nothing allocated, no kernel
 * launched; a search only fills a host struct for it.  sqe_index_scan_last describes the LAST search pass (<= 1024 queries) of
 * this index when the bf16 first pass answered it (SQE_ERR_STATE when there was none, when the int8 first pass answered, or when
 * the index was empty); sqe_index_scan_read copies `bytes` bytes from byte offset `offset` of one buffer as that search left it.
 * The buffers are overwritten by the next search.  The scanned operands themselves are SQE_STATE_SCAN_BF16 and SQE_STATE_QN below
 * (the scan reads the bf16 rounding of the latter).
 *   SQE_SCAN_LISTS        uint64 [n_chunks][b_pad][list_cap]: the candidate lists, key = orderable(score) << 32 | (0xFFFFFFFF - row)
 *                         with orderable(f) = bits(f) ^ (bits(f) < 0 ? 0xFFFFFFFF : 0x80000000); unordered; chunk c holds tiles
 *                         [c * (T / n) + min(c, T % n), ...), the T = n_tiles tiles of 256 rows dealt out evenly
 *   SQE_SCAN_LIST_COUNTS  int32 [n_chunks][b_pad]: keys in each list (<= kp)
 *   SQE_SCAN_BOUNDS       uint32 [b_pad / 64][ngroups][64 columns][64 queries]: the bound table as the scan left it, orderable
 *                         scores, 0 = nothing published; chunk c folds its maxima into column c % 64 of its queries' slice
 *   SQE_SCAN_COLLECT_THR  float [b_pad]: the certificate's collect threshold of each query, +inf = certified (entries at or past B
 *                         are never written)                                                                    } only when
 *   SQE_SCAN_UNC_COUNT    int32 [1]: queries whose certificate failed                                           } `certified`
 *   SQE_SCAN_UNC_IDS      int32 [uncertified]: those queries, ascending; position = compact index               } (else
 *   SQE_SCAN_COLLECT_COUNTS int32 [B]: by compact index, rows the collect pass met at or above the threshold    } SQE_ERR_STATE)
 *   SQE_SCAN_COLLECT_KEYS uint64 [uncertified][exact_cap]: by compact index, the first exact_cap of those rows  }
 * The collect launches (scan.hip, COLLECT mode) write SQE_SCAN_COLLECT_KEYS / _COUNTS only: they never store to the lists, their
 * counts or the bound table, so the first three buffers are the first pass's whether or not a certificate failed.  The fp32
 * re-score that follows (exact.hip) REPLACES the score half of every collect key of a query with count <= exact_cap by the fp32
 * cosine of that row (master row x SQE_STATE_QN): after a search the keys name the rows the collect scan gathered, not its scores. */
typedef struct sqe_scan_launch_t {
    int64_t rows;            /* rows scanned */
    int32_t dim, B, k, kp;   /* kp: keys kept per (chunk, query) list */
    int32_t bn;              /* queries per workgroup: 256, 128 or 64 */
    int32_t qblocks, b_pad, n_tiles, n_chunks, tiles_per_chunk, ngroups;   /* the plan (kernels.h: ScanPlan) */
    int32_t trig;            /* a list is cut back to its best kp when it reaches this many keys */
    int32_t gshift;          /* as the kernel received it: log2 of the column group of the kp-row bound, < 0 = bound off */
    int32_t gshift_k;        /* the same for the k-row bound (lowered by 2 eps), < 0 = off */
    int32_t k_rows;          /* > 0: the k-row bound is the k_rows-th largest of the 16 quad maxima */
    int32_t list_cap;        /* slots per (chunk, query) list */
    int32_t exact_cap;       /* slots per uncertified query of the collect pass */
    int32_t family;          /* SQE_SCAN_FAMILY_*: the host branch that launched */
    int32_t nst, nstb;       /* staged family: ring depth of the row tiles / of the query tiles (0 for ping-pong) */
    int32_t certified;       /* 1: the certificate and the collect pass ran */
    int32_t uncertified;     /* queries that went on to the collect pass (0 without the certificate) */
} sqe_scan_launch_t;
enum { SQE_SCAN_FAMILY_PINGPONG = 0, SQE_SCAN_FAMILY_STAGED = 1 };
enum { SQE_SCAN_LISTS = 0, SQE_SCAN_LIST_COUNTS = 1, SQE_SCAN_BOUNDS = 2, SQE_SCAN_COLLECT_THR = 3, SQE_SCAN_UNC_COUNT = 4,
       SQE_SCAN_UNC_IDS = 5, SQE_SCAN_COLLECT_COUNTS = 6, SQE_SCAN_COLLECT_KEYS = 7 };
int sqe_index_scan_last(sqe_index* idx, sqe_scan_launch_t* out);
int sqe_index_scan_read(sqe_index* idx, int what, int64_t offset, void* out_host, int64_t bytes);

/* Scanned copies and measured residuals (tests/test_copies_gpu.py, tests/test_bound_gpu.py: the inputs of the exactness
 * certificate -- kernels.h: scan_eps -- against a float64 restatement).  Test-only introspection like the two entries above, with
 * the same rules: single-device FLAT indexes only, row POSITIONS (0 .. rows-1 in ascending id order; sqe_index_ids maps them to
 * ids), one stream synchronisation per call, nothing allocated.  sqe_index_state describes what can be read; sqe_index_state_read
 * copies `bytes` bytes from byte offset `offset` of one buffer to the host.
 *   SQE_STATE_SCAN_BF16     uint16 bf16 copy of the rows, row position r at r * scan_pitch bytes (dim values, then padding), for
 *                           positions 0 .. round_up(rows, 256) - 1: the rows past `rows` are zero
 *   SQE_STATE_RESID_MAX     float [1]: max over rows of || x - bf16(x) ||, as measured (it only grows: updates and deletes keep it)
 *   SQE_STATE_I8_RESID_MAX  float [1]: the same for the int8 copy, || x - sxi unit x8 || (SQE_ERR_STATE without an int8 copy)
 * Per-query buffers of the last sqe_index_search[_device] on this index (of its last pass of <= 1024 queries); filtered, radial
 * and collapsed searches keep their queries elsewhere.  SQE_ERR_STATE before the first search:
 *   SQE_STATE_QN            float [last_B][dim]: the normalised fp32 queries
 *   SQE_STATE_Q_RESID       float [last_B]: || q - bf16(q) || per query, as measured
 *   SQE_STATE_Q8_RESID      float [last_B]: || q - sqi unit q8 || per query   } only when that search ran the int8 first pass
 *   SQE_STATE_Q8_SCALES     uint32 [last_B]: the integer scale sqi of each query } (last_i8; else SQE_ERR_STATE); the quantised
 *                           queries themselves are SQE_I8_QUERIES */
typedef struct sqe_index_state_t {
    int64_t rows;            /* live rows */
    int64_t i8_rows;         /* rows [0, i8_rows) of the int8 copy are current (0: no copy, or all of it awaits the next int8 search) */
    int64_t i8_tile_stride;  /* bytes between 256-row tiles of the int8 copy (0: no copy) */
    int32_t dim;
    int32_t scan_pitch;      /* bytes between rows of the bf16 copy */
    int32_t last_B;          /* queries of the last search pass (0: none yet) */
    int32_t last_i8;         /* 1: that pass ran the int8 first pass */
} sqe_index_state_t;
enum { SQE_STATE_SCAN_BF16 = 0, SQE_STATE_RESID_MAX = 1, SQE_STATE_I8_RESID_MAX = 2, SQE_STATE_QN = 3, SQE_STATE_Q_RESID = 4,
       SQE_STATE_Q8_RESID = 5, SQE_STATE_Q8_SCALES = 6 };
int sqe_index_state(sqe_index* idx, sqe_index_state_t* out);
int sqe_index_state_read(sqe_index* idx, int what, int64_t offset, void* out_host, int64_t bytes);

/* The last delete (tests/test_delete_routes_gpu.py: every block route of the in-place compaction -- csrc/compact.hip -- and every
 * byte it moved, against a NumPy restatement of the block rule and of the moves).  Test-only, with the rules of the entries
 * above: nothing allocated, no kernel launched, the host loop that walks the blocks only fills a host struct as it launches.
 * sqe_index_delete walks the rows from the first deleted position in blocks [b0, b1): a block with fewer than block_rows deleted
 * rows below b0 is STAGED (block_rows rows at most, through the staging buffer, two launches), a block with at least that many
 * is DIRECT (as many rows as are deleted below b0, moved in place by one launch).  SQE_ERR_STATE before the first delete of this
 * index; single-device indexes only, FLAT or IVF (a device group: SQE_ERR_UNSUPPORTED). */
typedef struct sqe_delete_last_t {
    int64_t n_old, n_new;        /* live rows before and after */
    int64_t first_pos;           /* lowest deleted row POSITION: rows below it did not move */
    int64_t block_rows;          /* w = max(256, 128 MiB / stage_pitch), stage_pitch = round_up(6 dim + (keys ? 24 : 12), 16) */
    int64_t staged_blocks, direct_blocks;
    int64_t staged_rows, direct_rows;   /* rows spanned by the blocks of each kind (deleted rows inside them included) */
    int64_t stage_bytes;         /* bytes of the staging buffer that was allocated (0: no staged block) */
} sqe_delete_last_t;
int sqe_index_delete_last(sqe_index* idx, sqe_delete_last_t* out);

/* IVF search state (tests/test_ivf_stages_gpu.py: every list-scan route and every score strip against a float64 or bit-level
 * restatement).  Test-only introspection like sqe_index_state[_read], with the same rules: single-device IVF indexes only (a device
 * group: SQE_ERR_UNSUPPORTED), one stream synchronisation per call, nothing allocated, no kernel launched; SQE_ERR_STATE before the
 * first IVF search.  sqe_index_ivf_state describes the LAST piece of the last search (a search cut into sub-batches reports its
 * last piece and sub_batches > 1); the route fields are written by the host branches that launched, not derived from the shapes.
 * sqe_index_ivf_state_read copies `bytes` bytes from byte offset `offset` of one buffer, as that search left it (the next search,
 * add, update or delete overwrites or rebuilds them).  Row ids here are row POSITIONS (sqe_index_ids maps them to ids).
 *   SQE_IVF_PROBES        int64 [B][nprobe]: the probed lists of each query, best first
 *   SQE_IVF_PROBES_COS    float [B][nprobe]: their cosines
 *   SQE_IVF_STRIPS        float [B][nprobe][max_len]: the score strip of each (query, probe) pair; position p of a strip is row
 *                         order[offsets[L] + p] of the probed list L, positions at or past the list's length hold nothing
 *   SQE_IVF_ORDER         int32 [n_assigned]: rows grouped by list
 *   SQE_IVF_OFFSETS       int64 [nlist + 1]: start of each list in `order`
 *   SQE_IVF_TILE_OFF      int64 [nlist + 1]: 256-row tiles of the int8 copy in front of each list
 *   SQE_IVF_SCAN_BF16     uint16 [n_assigned] rows of dim bf16 at scan_pitch bytes: the bf16 scan copy
 *   SQE_IVF_ROWS_F32      float [n_assigned][dim]: the normalised fp32 rows
 *   SQE_IVF_I8_ROWS       int8, total_tiles tiles of i8_tile_stride bytes: the LIST-ORDERED int8 copy; every list starts on a tile,
 *                         the 64-byte K slice h of tile row r at h * 16 KiB + r * 64  } SQE_ERR_STATE unless list_kernel is an
 *   SQE_IVF_I8_ROW_SCALES uint32 [total_tiles * 256]: the integer scale of each row  } int8 one; so are the next two
 *   SQE_IVF_Q8            int8 [B] rows at q8_pitch = dim + 128 bytes: the quantised queries
 *   SQE_IVF_Q8_SCALES     uint32 [B]: their integer scales
 *   SQE_IVF_QN            float [B][dim]: the normalised fp32 queries
 *   SQE_IVF_QB            uint16 [B] rows of dim bf16 at scan_pitch bytes: the bf16 queries
 *   SQE_IVF_THRESHOLDS    float [B]: collect thresholds                               } SQE_ERR_STATE unless grid is
 *   SQE_IVF_COUNTS        int32 [2 B]: keys appended to each query's list, then the rows in its probed lists  } SQE_IVF_GRID_COLLECT
 *   SQE_IVF_KEY_LISTS     uint64 [B][list_cap]: keys (orderable score << 32 | 0xFFFFFFFF - row), unordered   } */
typedef struct sqe_ivf_state_t {
    int64_t n_assigned;      /* rows in the lists */
    int64_t total_tiles;     /* 256-row tiles of the int8 copy */
    int64_t i8_tile_stride;  /* bytes between them (0: no int8 copy) */
    int32_t B, nprobe, k, kp;   /* nprobe after clamping */
    int32_t max_len;         /* strip pitch in floats */
    int32_t nlist, dim;
    int32_t scan_pitch, q8_pitch;
    int32_t coarse;          /* SQE_IVF_COARSE_* */
    int32_t list_kernel;     /* SQE_IVF_KERNEL_* */
    int32_t grid;            /* SQE_IVF_GRID_* */
    int32_t split;           /* workgroups per (query, probe) pair: SQE_IVF_GRID_PAIR only, else 0 */
    int32_t queued;          /* bit mask SQE_IVF_QUEUED_*: launches that ran persistent workgroups on the unit queue */
    int32_t n_units1, n_units4, n_unitsS, n_unitsR;
    int32_t sub_batches;
    int32_t fallback;        /* the collect mode's fallback flag as the device holds it (0 outside that mode) */
    int32_t list_cap;        /* keys of a query's collect list */
    int32_t persistent;      /* workgroups of a queued launch (two per CU): a launch of more units than this takes the queue */
} sqe_ivf_state_t;
enum { SQE_IVF_COARSE_DENSE = 0, SQE_IVF_COARSE_FLAT = 1 };
enum { SQE_IVF_KERNEL_FP32 = 0, SQE_IVF_KERNEL_BF16_MFMA = 1, SQE_IVF_KERNEL_I8_STAGED = 2, SQE_IVF_KERNEL_I8_STREAM = 3 };
enum { SQE_IVF_GRID_LIST = 0, SQE_IVF_GRID_PAIR = 1, SQE_IVF_GRID_PAIR_GRID = 2, SQE_IVF_GRID_UNITS1 = 3, SQE_IVF_GRID_UNITS4 = 4,
       SQE_IVF_GRID_COLLECT = 5 };
enum { SQE_IVF_QUEUED_STRIPS = 1, SQE_IVF_QUEUED_SAMPLE = 2, SQE_IVF_QUEUED_COLLECT = 4, SQE_IVF_QUEUED_FALLBACK = 8 };
enum { SQE_IVF_PROBES = 0, SQE_IVF_PROBES_COS = 1, SQE_IVF_STRIPS = 2, SQE_IVF_ORDER = 3, SQE_IVF_OFFSETS = 4, SQE_IVF_TILE_OFF = 5,
       SQE_IVF_SCAN_BF16 = 6, SQE_IVF_ROWS_F32 = 7, SQE_IVF_I8_ROWS = 8, SQE_IVF_I8_ROW_SCALES = 9, SQE_IVF_Q8 = 10,
       SQE_IVF_Q8_SCALES = 11, SQE_IVF_QN = 12, SQE_IVF_QB = 13, SQE_IVF_THRESHOLDS = 14, SQE_IVF_COUNTS = 15, SQE_IVF_KEY_LISTS = 16 };
int sqe_index_ivf_state(sqe_index* idx, sqe_ivf_state_t* out);
int sqe_index_ivf_state_read(sqe_index* idx, int what, int64_t offset, void* out_host, int64_t bytes);

/* Persistence.  The reference keeps its vectors in the OpenSearch index across restarts and skips the
 * rebuild when `has_any_data()` is true (main.py:300-307, :422-424); here the index lives in HBM, so it
 * is written to / read from a local file: the normalised fp32 rows (plus IVF centroids and list
 * assignments) exactly as stored -- a loaded index returns bit-identical results.  The scanned bf16
 * copy and the IVF lists are rebuilt on load.  `sqe_index_load` creates the index.  An index that never had a
 * delete writes a version 1 file; one with deleted ids writes version 2, which adds next_id and the live ids
 * (readers that predate deletes refuse it). */
int sqe_index_save(sqe_index* idx, const char* path);
int sqe_index_load(sqe_ctx* ctx, const char* path, sqe_index** out);

/* Merge of per-shard results after the all-gather of a row-sharded index: part p holds
 * cos [B,k] fp32 at cos_parts_dev + p * part_stride_bytes and global ids [B,k] int64
 * (-1 padded) at id_parts_dev + p * part_stride_bytes (part_stride_bytes = 0: dense
 * [P,B,k] arrays).  out is [B,k], best first, ties to the lowest id.  Device pointers,
 * context stream. */
int sqe_merge_topk_device(sqe_ctx* ctx, const float* cos_parts_dev, const int64_t* id_parts_dev,
                          int64_t part_stride_bytes, int P, int B, int k,
                          float* cos_out_dev, int64_t* id_out_dev);

/* ---- lexical index: BM25 over the `text` field (OpenSearch `match`) ---------------- */
/* A document is an int64 id >= 0 and a bag of term ids in [0, n_terms); the caller's analyzer makes the term ids (the Python
 * client uses the WordPiece tokenizer without [CLS] / [SEP] / [PAD], the same function for documents and queries).
 * The score is defined in integers, so that every result can be compared bit for bit:
 *   tf(t, d)  occurrences of t in d, capped at 65535;   dl(d)  occurrences in d, before the cap
 *   N = live documents, L = the sum of dl over them, avgdl = (double)L / (double)N, df(t) = live documents that hold t
 *   idf(t)  = log(1.0 + ((double)(N - df) + 0.5) / ((double)df + 0.5))           libm log on the host
 *   norm(d) = k1 * ((1.0 - b) + b * ((double)dl / avgdl))                         every operation an IEEE double operation in
 *                                                                                 this order, nothing contracted into an FMA
 *   I(t, d) = max(1, llrint(ldexp(idf(t) * ((double)tf / ((double)tf + norm(d))), 16)))      for tf >= 1
 *   score_int(q, d) = the sum of I(t, d) over the term OCCURRENCES of the query that d holds: a repeated query term counts
 *             each time, a term with df = 0 adds nothing, a document that holds a query term is always a hit (I >= 1)
 *   score   = (float)((double)score_int * 2^-16)
 * This is the BM25 of Lucene 9 -- idf * tf / (tf + k1 * (1 - b + b * dl / avgdl)), WITHOUT the constant (k1 + 1) factor earlier
 * versions multiplied in -- and without Lucene's one-byte quantisation of the document length: dl enters exactly.
 * Bound: idf < log(2 N + 2) < 22.2 for N < 2^31 and tf / (tf + norm) <= 1, so I < 22.2 * 2^16 < 2^21; a query holds at most 64
 * term occurrences, so score_int < 2^27 fits a uint32.  sqe_lex_put refuses what would take N to 2^31, the searches refuse
 * longer queries.  Because scores are sums of integers no floating-point accumulation order exists: the answer cannot depend
 * on the batch size, the order of the postings or the chunking.
 * Ranking: score_int descending, ties to the lowest id.  Documents with score_int == 0 are not hits; unused places hold
 * (-inf, -1).
 *   sqe_lex_create: k1 in [0, 3] and b in [0, 1] are fixed at creation (OpenSearch's defaults: 1.2 and 0.75); 1 <= n_terms <=
 *     131072.  On a device group the index lives on the leader.
 *   sqe_lex_put: n documents, bag i = terms[offsets[i] .. offsets[i + 1]), in any order and with repeats.  The ids of one call
 *     are distinct; an id that is live has its bag replaced; an empty bag is a valid document that never scores (it counts in N).
 *   sqe_lex_delete: unknown ids are skipped.
 *   After any sequence of put and delete the index answers bit for bit like a fresh index of the live documents: the device
 *     index is rebuilt from the host's forward log by the first search after a mutation (every impact changes with N and avgdl
 *     anyway), and a search that finds it clean reads nothing back and does not synchronise.
 *   sqe_lex_search: query b = qterms[qoffsets[b] .. qoffsets[b + 1]), at most 64 occurrences, may be empty (all padding);
 *     qoffsets [B + 1] and qterms are HOST memory in both forms and are not retained.  score_out / id_out [B, k], 1 <= k <= 256.
 *     The _device form writes device memory on the context stream.  B == 0 and an empty index are valid.
 * SQE_ERR_INVALID, with nothing written or changed: a term outside [0, n_terms), a negative or repeated id, offsets that do not
 * start at 0 or decrease, more than 64 occurrences in a query, k outside [1, 256], k1 or b out of range or NaN, a null buffer
 * that is needed.
 * How (csrc/lexical.hip): rows are the live documents in id order, cut into chunks of chunk_rows; every chunk has its own CSR by
 * term over (row, impact) postings.  One workgroup per (chunk, query) adds the impacts of the query's runs into chunk_rows
 * uint32 accumulators in LDS and selects its best k; one workgroup per query merges the chunks.  Scoring is booked under scan_ms,
 * the merge under select_ms. */
typedef struct sqe_lex sqe_lex;
typedef struct sqe_lex_info_t {
    int64_t documents;       /* live documents */
    int64_t postings;        /* (row, impact) pairs of the device index as last built */
    int32_t n_terms;
    int32_t chunk_rows;      /* rows of a chunk (a compile-time power of two) */
    int32_t chunks;          /* of the device index as last built */
    int32_t rebuilds;        /* rebuilds so far: one per search that found the index changed */
    double avgdl;            /* of the last rebuild */
    double last_rebuild_ms;  /* host time of the last rebuild, upload and kernels included */
} sqe_lex_info_t;
int sqe_lex_create(sqe_ctx* ctx, int n_terms, double k1, double b, sqe_lex** out);
void sqe_lex_destroy(sqe_lex* lex);
int sqe_lex_put(sqe_lex* lex, const int64_t* ids_host, const int64_t* offsets_host, const int32_t* terms_host, int64_t n);
int sqe_lex_delete(sqe_lex* lex, const int64_t* ids_host, int64_t n);
int sqe_lex_count(const sqe_lex* lex, int64_t* out);
int sqe_lex_search(sqe_lex* lex, const int64_t* qoffsets_host, const int32_t* qterms_host, int B, int k,
                   float* score_out_host, int64_t* id_out_host);
int sqe_lex_search_device(sqe_lex* lex, const int64_t* qoffsets_host, const int32_t* qterms_host, int B, int k,
                          float* score_out_dev, int64_t* id_out_dev);
/* Boolean queries (OpenSearch `match` with `operator` / `minimum_should_match`, `bool` over `match` clauses) and match sets.
 * A query stays a list of at most 64 term occurrences; every occurrence carries a role, every query a number min_should:
 *   SQE_LEX_SHOULD    scores; optional (subject to min_should)
 *   SQE_LEX_MUST      scores; the document must hold the term
 *   SQE_LEX_FILTER    does not score; the document must hold the term
 *   SQE_LEX_MUST_NOT  does not score; the document must not hold the term
 * Occurrence j HOLDS in document d iff tf(t_j, d) >= 1; a term with df = 0 holds nowhere.  Document d MATCHES query b iff
 *   every MUST and FILTER occurrence holds, and
 *   no MUST_NOT occurrence holds, and
 *   the number of SHOULD occurrences that hold is at least m_b -- a repeated occurrence counts each time, as in the score --
 *     where m_b = min_should[b] if the query has a MUST or FILTER occurrence, else max(1, min_should[b]).
 * A query without a positive occurrence (empty, or MUST_NOT only) matches nothing.  min_should lies in [0, 64]; a value above
 * the number of SHOULD occurrences matches nothing.
 *   score_int(q, d) = the sum of I(t, d) over the SHOULD and MUST occurrences that hold; impacts, idf, norm and the 2^-16
 *     scaling are those above.  A match may have score_int == 0 (FILTER occurrences only): it is a hit with score 0.0f, ranked
 *     after every positive score.  Ranking: score_int descending, ties to the lowest id, padding (-inf, -1).
 *   sqe_lex_search_bool: the best k matches, 1 <= k <= 256.  qroles holds one uint8 per occurrence (beside qterms), min_should
 *     [B] int32, NULL = zeros; both are HOST memory in both forms.  With every role SQE_LEX_SHOULD and min_should NULL or zero
 *     the result is bit for bit that of sqe_lex_search.
 *   sqe_lex_match: the match SET.  count_out [B] int64 is the exact number of matches, whatever cap is; id_out [B, cap] int64
 *     holds the min(count, cap) lowest matching ids of each query in ascending order, padded with -1.  cap >= 0; with cap == 0
 *     only the counts are produced and id_out may be NULL.  The host form copies the counts and the ids back once.
 * SQE_ERR_INVALID, with nothing written: what sqe_lex_search refuses, a role above 3, min_should outside [0, 64], cap < 0.
 * B == 0 and an empty index are valid.  A call that finds the index clean reads nothing back and synchronises nothing in its
 * _device form.
 * How (csrc/lexical.hip): per (chunk, query) the match state is a bit per row in LDS -- a map per clause, filled by atomic ORs
 * and folded into the map of the rows alive; byte counters only for min_should >= 2 -- beside the impact accumulators; a
 * workgroup none of whose rows is alive leaves before scoring.  The match set is that map written out, an exclusive scan of the
 * chunks' popcounts per query and a ballot / popcount expansion to ids at each chunk's offset; no floating point is involved.
 * Scoring and the maps are booked under scan_ms, merge, scan and expansion under select_ms. */
enum { SQE_LEX_SHOULD = 0, SQE_LEX_MUST = 1, SQE_LEX_FILTER = 2, SQE_LEX_MUST_NOT = 3 };
int sqe_lex_search_bool(sqe_lex* lex, const int64_t* qoffsets_host, const int32_t* qterms_host, const uint8_t* qroles_host,
                        const int32_t* min_should_host, int B, int k, float* score_out_host, int64_t* id_out_host);
int sqe_lex_search_bool_device(sqe_lex* lex, const int64_t* qoffsets_host, const int32_t* qterms_host, const uint8_t* qroles_host,
                               const int32_t* min_should_host, int B, int k, float* score_out_dev, int64_t* id_out_dev);
int sqe_lex_match(sqe_lex* lex, const int64_t* qoffsets_host, const int32_t* qterms_host, const uint8_t* qroles_host,
                  const int32_t* min_should_host, int B, int64_t cap, int64_t* count_out_host, int64_t* id_out_host);
int sqe_lex_match_device(sqe_lex* lex, const int64_t* qoffsets_host, const int32_t* qterms_host, const uint8_t* qroles_host,
                         const int32_t* min_should_host, int B, int64_t cap, int64_t* count_out_dev, int64_t* id_out_dev);
/* Phrase queries (OpenSearch `match_phrase`, slop 0): documents that remember their order, queries made of clauses.
 *   sqe_lex_put_ordered: sqe_lex_put with the same arguments and the same refusals; the terms of document i are taken as its
 *     SEQUENCE seq_d[0 .. dl).  Its bag is the multiset of the sequence: every other entry point answers bit for bit as after
 *     sqe_lex_put of the same terms.  A document put with sqe_lex_put has no sequence and holds no phrase of two or more terms.
 *     Both kinds may live in one index; a put of either form replaces both the bag and the sequence.  The cost is four bytes
 *     per occurrence; an index that never saw an ordered put uploads and allocates nothing more than before.
 * Query b owns the CLAUSES qoffsets[b] .. qoffsets[b + 1]; clause c owns the occurrences qterms[coffsets[c] .. coffsets[c + 1]),
 * at least one; a query holds at most 64 occurrences in all.  croles holds one role per clause, min_should [B] or NULL as above;
 * all tables are HOST memory in both forms.
 *   pf(c, d)  for a clause t_0 .. t_{L-1} with L >= 2: the number of start positions p, 0 <= p <= dl(d) - L, with
 *             seq_d[p + j] == t_j for every j.  Overlapping occurrences each count (`a a` in `a a a`: pf = 2).  Capped at
 *             65535; 0 for a document without a sequence and for a phrase with a term of df = 0.  For L = 1, pf = tf(t_0, d).
 *   Clause c HOLDS in d iff pf(c, d) >= 1.  Document d MATCHES by the rules of sqe_lex_search_bool with "occurrence" read as
 *   "clause": m_b, "a repeated clause counts each time" and "no positive clause matches nothing" included.
 *   score_int(q, d) = the sum of I(c, d) over the SHOULD and MUST clauses that hold.  A clause of one term adds the stored
 *     I(t, d).  A clause of L >= 2 terms has idf(c) = idf(t_0) + idf(t_1) + ... added left to right as IEEE doubles and
 *     I(c, d) = max(1, llrint(ldexp(idf(c) * ((double)pf / ((double)pf + norm(d))), 16)))          every operation a double
 *     operation in this order, nothing contracted, norm(d) as above.  This is Lucene's phrase scoring: summed idf, phrase
 *     frequency in place of tf.
 * Bound: idf(c) < 22.2 L and the L of a query sum to at most 64, so score_int < 2^27 as before.  Ranking, padding, count_out, cap
 * and the -1 padding of the match set are those of sqe_lex_search_bool / sqe_lex_match, and with every clause of length 1 the two
 * calls return bit for bit what those return.
 * SQE_ERR_INVALID, with nothing written: what the boolean calls refuse, an empty clause, coffsets / qoffsets that do not start at
 * 0 or decrease, more than 64 occurrences in a query.
 * How (csrc/lexical.hip): a phrase is the AND of its terms' runs (one more bit map per row of the chunk, ANDed with the rows
 * still alive) followed by a check of the order: a wave per candidate row, its lanes over the start positions of the row's
 * sequence.  A scoring phrase adds its impact where it is verified; where the accumulators' space is taken by the byte counters
 * (min_should >= 2) it is verified once more over the rows alive at the end. */
int sqe_lex_put_ordered(sqe_lex* lex, const int64_t* ids_host, const int64_t* offsets_host, const int32_t* terms_host, int64_t n);
int sqe_lex_search_phrase(sqe_lex* lex, const int64_t* qoffsets_host, const int64_t* coffsets_host, const int32_t* qterms_host,
                          const uint8_t* croles_host, const int32_t* min_should_host, int B, int k, float* score_out_host,
                          int64_t* id_out_host);
int sqe_lex_search_phrase_device(sqe_lex* lex, const int64_t* qoffsets_host, const int64_t* coffsets_host, const int32_t* qterms_host,
                                 const uint8_t* croles_host, const int32_t* min_should_host, int B, int k, float* score_out_dev,
                                 int64_t* id_out_dev);
int sqe_lex_match_phrase(sqe_lex* lex, const int64_t* qoffsets_host, const int64_t* coffsets_host, const int32_t* qterms_host,
                         const uint8_t* croles_host, const int32_t* min_should_host, int B, int64_t cap, int64_t* count_out_host,
                         int64_t* id_out_host);
int sqe_lex_match_phrase_device(sqe_lex* lex, const int64_t* qoffsets_host, const int64_t* coffsets_host, const int32_t* qterms_host,
                                const uint8_t* croles_host, const int32_t* min_should_host, int B, int64_t cap, int64_t* count_out_dev,
                                int64_t* id_out_dev);
int sqe_lex_info(sqe_lex* lex, sqe_lex_info_t* out);
/* Test-only read-back of the device index as the last rebuild left it (tests/test_lexical_gpu.py), with the rules of
 * sqe_index_state_read: one stream synchronisation per call, nothing allocated, no kernel launched.  SQE_ERR_STATE while a
 * mutation awaits its rebuild (search first); an empty index holds nothing.  Rows are the live documents in ascending id order.
 *   SQE_LEX_DF        int32 [n_terms]
 *   SQE_LEX_IDF       double [n_terms] (0 where df = 0)
 *   SQE_LEX_IDS       int64 [documents]: row -> id
 *   SQE_LEX_DL        int64 [documents]
 *   SQE_LEX_TABLE     uint32 [chunks][n_terms + 1]: the run of term t in chunk c is postings [base_c + table[c][t], base_c +
 *                     table[c][t + 1]), base_c = the sum of table[c'][n_terms] over the chunks c' < c
 *   SQE_LEX_POSTINGS  uint32 [postings][2]: (row, impact); the order inside a run is unspecified
 *   SQE_LEX_SEQ_OFF   int64 [documents + 1]: where the row's sequence starts in SQE_LEX_SEQ (its length is the row's dl), -1
 *                     for a row without a sequence (an empty sequence has an offset and dl = 0); the last entry is the number
 *                     of words of SQE_LEX_SEQ.  Both hold nothing while no live document has a sequence.
 *   SQE_LEX_SEQ       int32: the live sequences one after the other in row order */
enum { SQE_LEX_DF = 0, SQE_LEX_IDF = 1, SQE_LEX_IDS = 2, SQE_LEX_DL = 3, SQE_LEX_TABLE = 4, SQE_LEX_POSTINGS = 5, SQE_LEX_SEQ_OFF = 6,
       SQE_LEX_SEQ = 7 };
int sqe_lex_state_read(sqe_lex* lex, int what, int64_t offset, void* out_host, int64_t bytes);

/* Hybrid search (OpenSearch `hybrid` over knn sub-queries and one `match`): reciprocal rank fusion of vector lists and one
 * lexical list.  Group g owns the vector sub-queries q[offsets[g] .. offsets[g + 1]), 0 <= m_g <= 31, and the lexical query
 * qterms[qoffsets[g] .. qoffsets[g + 1]), which may be empty: an empty query has no list.  The lists are sqe_index_search(q_j, n)
 * for each j and sqe_lex_search(terms, n) as one more list; (m_g + 1) * n <= 2048; n == 0 means automatic, min(256, max(32, 4 k)).
 * Fusion is exactly the SQE_FUSE_RRF arithmetic of sqe_index_search_fused: fused_int(x) = the sum of T(w_j, r_j(x)) over the
 * lists that hold x.  weights [Bs + G] (HOST memory, NULL = all 1): the Bs weights of the vector sub-queries first, then one
 * weight per group for its lexical list.  Ranking: fused_int descending, ties to the lowest id.
 * Outputs [G, k]: fused_out and id_out as for the fused search; cos_out = the row's best cosine over the vector lists that hold
 * it, -inf if none does; lex_out = its BM25 score as sqe_lex_search returned it, -inf if the lexical list does not hold it;
 * padded with (-inf, -1, -inf, -inf).  The lexical index's ids are the vector index's ids as a search returns them; keeping the
 * two in step is the caller's job, and an id known to one side only is still returned.  A group with no vector sub-query
 * returns the lexical list's ids in its order; with every lexical query empty the call returns bit for bit what
 * sqe_index_search_fused(SQE_FUSE_RRF) returns.  offsets, qoffsets, qterms and weights are HOST memory in both forms.
 * SQE_ERR_INVALID, with nothing written: what sqe_index_search_fused and sqe_lex_search refuse, m_g > 31, (m_g + 1) * n > 2048.
 * Both objects must belong to the same context.  The index lock is taken before the lexical index's. */
int sqe_index_search_hybrid(sqe_index* idx, sqe_lex* lex, const float* q_host, int G, const int64_t* offsets_host,
                            const int64_t* qoffsets_host, const int32_t* qterms_host, int k, int n, int rank_constant,
                            const float* weights_host, int nprobe, float* fused_out_host, int64_t* id_out_host,
                            float* cos_out_host, float* lex_out_host);
int sqe_index_search_hybrid_device(sqe_index* idx, sqe_lex* lex, const float* q_dev, int G, const int64_t* offsets_host,
                                   const int64_t* qoffsets_host, const int32_t* qterms_host, int k, int n, int rank_constant,
                                   const float* weights_host, int nprobe, float* fused_out_dev, int64_t* id_out_dev,
                                   float* cos_out_dev, float* lex_out_dev);

/* ---- semantic cache scan: stands behind the loop of lfu_cache_get (main.py:73-87) -- */
/* One-shot form: mat is [m, dim] raw (un-normalised) cached embeddings in list order
 * (index 0 = newest), q is [dim] raw.  cosine = dot / (||a|| * ||b||) in fp32 with the
 * zero-norm rule (main.py:59-64); returns the FIRST strict maximum starting from
 * (-1.0, -1) exactly as main.py:74-87 does (NaN never wins). */
int sqe_cosine_best(sqe_ctx* ctx, const float* mat_host, int m, int dim, const float* q_host,
                    float* best_sim, int32_t* best_idx);
/* All m cosines (the values cosine_similarity returns, main.py:59-64). */
int sqe_cosine_all(sqe_ctx* ctx, const float* mat_host, int m, int dim, const float* q_host,
                   float* sims_out_host);

/* Resident form: the cache matrix lives in HBM; the host keeps the LFU bookkeeping
 * (freq counters, JSON payloads) and tells the library which slot holds which list
 * position.  `order_host[i]` = slot of list position i (position 0 = newest). */
int sqe_cache_create(sqe_ctx* ctx, int capacity, int dim, sqe_cache** out);
void sqe_cache_destroy(sqe_cache* c);
int sqe_cache_set_slot(sqe_cache* c, int slot, const float* vec_host);
int sqe_cache_best(sqe_cache* c, const int32_t* order_host, int m, const float* q_host,
                   float* best_sim, int32_t* best_pos);

/* ---- encoder: stands behind ollama_embed_text (main.py:134-145) ------------------ */
typedef struct sqe_bert_cfg {
    int32_t vocab_size;  /* 30522 */
    int32_t hidden;      /* 1024 */
    int32_t layers;      /* 24 */
    int32_t heads;       /* 16 */
    int32_t inter;       /* 4096 */
    int32_t max_pos;     /* 512 */
    int32_t type_vocab;  /* 2 */
    float ln_eps;        /* 1e-12 */
} sqe_bert_cfg;

/* Tensors are fp32 host arrays named as in the HF BertModel state dict
 * ("embeddings.word_embeddings.weight", "encoder.layer.0.attention.self.query.weight"...);
 * they are converted to bf16 (matrices, embeddings) / fp32 (biases, LayerNorm) on load. */
int sqe_encoder_create(sqe_ctx* ctx, const sqe_bert_cfg* cfg, sqe_encoder** out);
void sqe_encoder_destroy(sqe_encoder* enc);
int sqe_encoder_load_tensor(sqe_encoder* enc, const char* name, const float* data_host,
                            const int64_t* shape, int ndim);
int sqe_encoder_finalize(sqe_encoder* enc);
/* Host-only BERT WordPiece (clean, CJK spacing, NFD + accent strip, lower-case, punctuation
 * split, greedy longest match with "##" continuations, [CLS] ... [SEP], truncation to max_len
 * ids): the tokenizer that ran inside Ollama for main.py:139-142.  Needs no GPU and no context.
 * vocab_utf8: one token per line, line number = id (a local vocab.txt; nothing is fetched). */
int sqe_tokenizer_create(const char* vocab_utf8, int64_t vocab_bytes, sqe_tokenizer** out);
void sqe_tokenizer_destroy(sqe_tokenizer* tok);
int sqe_tokenize(const sqe_tokenizer* tok, const char* text_utf8, int64_t text_bytes, int max_len,
                 int32_t* ids_out, int* len_out);
/* n texts -> ids_out [n, max_len] ([PAD] = 0 filled), lens_out [n]; multi-threaded for n >= 64. */
int sqe_tokenize_batch(const sqe_tokenizer* tok, const char* const* texts, const int64_t* text_bytes, int n,
                       int max_len, int32_t* ids_out, int32_t* lens_out);
/* Sentence pairs for a cross-encoder: row i of ids_out [n, max_len] is [CLS] A [SEP] B [SEP], types_out [n, max_len] is 0
 * over [CLS] A [SEP] and 1 over B [SEP]; past lens_out[i] both hold 0 ([PAD], type 0).  A is cut to its first max_a word
 * pieces (the rule sqe_tokenize applies with max_len = max_a + 2), B to the max_len - 3 - len(A) pieces that are left; an
 * empty B keeps its [SEP].  SQE_ERR_INVALID unless max_len >= 4 and 1 <= max_a <= max_len - 3.  Threads as
 * sqe_tokenize_batch (n >= 64, at most 16). */
int sqe_tokenize_pair_batch(const sqe_tokenizer* tok, const char* const* a_texts, const int64_t* a_bytes,
                            const char* const* b_texts, const int64_t* b_bytes, int n, int max_len, int max_a,
                            int32_t* ids_out, int32_t* types_out, int32_t* lens_out);
/* ids [B,S] int32 row-major (anything past lens[b] is ignored), lens [B];
 * out [B, hidden] fp32 = final-layer CLS row (no normalisation, as Ollama's
 * /api/embeddings output feeds main.py:315-316 and :59-64 un-normalised). */
int sqe_encode(sqe_encoder* enc, const int32_t* ids_host, const int32_t* lens_host, int B, int S,
               float* out_host);
int sqe_encode_device(sqe_encoder* enc, const int32_t* ids_dev, const int32_t* lens_dev, int B, int S,
                      float* out_dev);

/* Cross-encoder scoring (BertForSequenceClassification: BERT + pooler + linear classifier).  sqe_encoder_load_tensor also
 * takes "pooler.dense.weight" [hidden, hidden], "pooler.dense.bias" [hidden], "classifier.weight" [labels, hidden] and
 * "classifier.bias" [labels], 1 <= labels <= 8 (read from the shape of classifier.weight); all four stay fp32.
 * sqe_encoder_finalize accepts the encoder tensors alone or with all four; a partial head is SQE_ERR_STATE.
 * sqe_encoder_labels: labels, 0 without a head.
 * sqe_encode_pairs: the forward pass of sqe_encode with the type row types[b][s] (clamped into [0, type_vocab);
 * NULL: row 0 everywhere) in the embedding sum, then
 *   pooled[b][j] = tanh(b_p[j] + sum_i W_p[j][i] cls[b][i]),  logits[b][l] = b_c[l] + sum_j W_c[l][j] pooled[b][j]
 * on the LayerNorm'd CLS rows, all in fp32; logits_out [B, labels].  SQE_ERR_STATE on an encoder without a head; B == 0 is
 * valid.  The _device form takes device pointers and is stream-ordered like sqe_encode_device. */
int sqe_encoder_labels(sqe_encoder* enc, int* out);
int sqe_encode_pairs(sqe_encoder* enc, const int32_t* ids_host, const int32_t* types_host, const int32_t* lens_host,
                     int B, int S, float* logits_out_host);
int sqe_encode_pairs_device(sqe_encoder* enc, const int32_t* ids_dev, const int32_t* types_dev, const int32_t* lens_dev,
                            int B, int S, float* logits_out_dev);

/* Encoder workspace read-back (tests/test_encoder_stages_gpu.py: every stage of the last layer recomputed in float64 from
 * the input the GPU itself holds, oracle/bert.py: stage_*).  Test-only introspection like sqe_index_state[_read], with the
 * same rules: one stream synchronisation per call, nothing allocated, no kernel launched.  After an encode has returned the
 * workspace still holds what the LAST layer computed; sqe_encoder_state says which kernels the call that just returned ran
 * (whether it launched them itself, recorded them into a graph or replayed a graph recorded earlier) and what can be read,
 * sqe_encoder_state_read copies `bytes` bytes from byte offset `offset` of one buffer to the host.  SQE_ERR_STATE before the
 * first encode.  Rows are tokens, row = b * S + s; rows T .. t_pad + 63 exist (padding of the GEMM tiles and of the
 * attention kernel's key tiles) and hold nothing of meaning.
 *   SQE_ENC_X     bf16 [t_pad + 64][hidden]      input of the last layer (one layer: the embedding LayerNorm output)
 *   SQE_ENC_QKV   bf16 [t_pad + 64][3 hidden]    QKV projection: query, key, value features of a token side by side
 *   SQE_ENC_ATT   bf16 [t_pad + 64][hidden]      attention output; rows at positions >= lens[b] are never written
 *   SQE_ENC_X1    bf16 [t_pad + 64][hidden]      LayerNorm(x + att Wo^T + bo)
 *   SQE_ENC_HBUF  bf16 [t_pad + 64][inter]       GELU(x1 W1^T + b1)
 *   SQE_ENC_PRE   x1 + hbuf W2^T + b2 before the last LayerNorm: pre_slices >= 1: float [pre_slices][pre_stride] partial sums
 *                 over K slices, which the LayerNorm kernels add up; pre_slices == 0: bf16 [t_pad][hidden], one row per token
 *   SQE_ENC_OUT   float [B][hidden]              the pooled result as sqe_encode copied it out (SQE_ERR_STATE after
 *                                                sqe_encode_device, whose output buffer is the caller's)
 * After a scoring call (SQE_ERR_STATE after any other; SQE_ENC_OUT then gives SQE_ERR_STATE):
 *   SQE_ENC_CLS    float [B][hidden]             the LayerNorm'd CLS rows the head read
 *   SQE_ENC_POOLED float [B][hidden]             tanh(pooler)
 *   SQE_ENC_LOGITS float [B][labels]             as sqe_encode_pairs copied them out (SQE_ERR_STATE after the _device form) */
enum { SQE_ENC_X = 0, SQE_ENC_X1 = 1, SQE_ENC_QKV = 2, SQE_ENC_ATT = 3, SQE_ENC_HBUF = 4, SQE_ENC_PRE = 5, SQE_ENC_OUT = 6,
       SQE_ENC_CLS = 7, SQE_ENC_POOLED = 8, SQE_ENC_LOGITS = 9 };
enum { SQE_ENC_EAGER = 0, SQE_ENC_CAPTURED = 1, SQE_ENC_REPLAYED = 2 };
enum { SQE_GEMM_FEW_TOKEN = 0, SQE_GEMM_RING = 1, SQE_GEMM_PING_PONG = 2, SQE_GEMM_PERSISTENT = 3, SQE_GEMM_ONE_TILE = 4 };
enum { SQE_SITE_QKV = 0, SQE_SITE_OUT_PROJ = 1, SQE_SITE_FFN_UP = 2, SQE_SITE_FFN_DOWN = 3 };
typedef struct sqe_encoder_gemm_t {
    int32_t family;      /* SQE_GEMM_* */
    int32_t menu;        /* ring kernel: index into its tile menu (0 .. 6); -1 for every other family */
    int32_t slices;      /* K slices, each one workgroup's partial sum (1: K is not cut) */
} sqe_encoder_gemm_t;
typedef struct sqe_encoder_state_t {
    int32_t B, S, T, t_pad;
    int32_t mode;            /* SQE_ENC_EAGER, SQE_ENC_CAPTURED (recorded and launched once) or SQE_ENC_REPLAYED */
    int32_t att_nw, att_nq;  /* attention: waves per workgroup, 16-row query blocks per wave (16 nw nq query rows per workgroup) */
    int32_t pre_slices;      /* SQE_ENC_PRE: fp32 partial sums per element; 0: bf16 rows */
    int64_t pre_stride;      /* floats between the partial sums of SQE_ENC_PRE */
    sqe_encoder_gemm_t gemm[4];   /* by SQE_SITE_* */
} sqe_encoder_state_t;
int sqe_encoder_state(sqe_encoder* enc, sqe_encoder_state_t* out);
int sqe_encoder_state_read(sqe_encoder* enc, int what, int64_t offset, void* out_host, int64_t bytes);

/* ---- stats ----------------------------------------------------------------------- */
/* When profiling is on, every stage is bracketed by hipEvents on the context stream;
 * sqe_stats reads the accumulated totals (it synchronises the stream). */
typedef struct sqe_stats_t {
    double scan_ms;        /* bf16 scan kernels: the main launches plus the collect-pass scans of uncertified queries */
    double prep_ms;        /* query normalise + cast */
    double select_ms;      /* candidate merge + fp32 rescore + final top-k */
    double add_ms;         /* normalise + cast of added rows */
    double encode_ms;      /* encoder forward */
    double cache_ms;       /* cache scan */
    int64_t scan_calls;    /* main scan launches (the collect pass is not counted) */
    int64_t search_calls;
    int64_t scan_rows;     /* rows scanned by the last search */
    int64_t scan_flops;    /* 2 * rows * dim * B of the last search */
    int64_t scan_bytes;    /* algorithmic bytes of the last search */
    int64_t uncertified;   /* queries of the last search that needed the exact fp32 rescan */
    double sample_ms;      /* int8 mode: threshold pass (the int8 sample scan + order statistic, or with "i8_sample_int8" = 0 the bf16
                            * scan + fp32 re-score of the row sample); a stage of its own, not part of scan_ms */
    int64_t i8_collected;  /* int8 mode, last search: keys the collect scan appended (all queries) */
    int64_t i8_rescored;   /*   rows re-scored in fp32 */
    int64_t i8_overflows;  /*   queries whose lists or buffers overflowed (they took the bf16 pass) */
} sqe_stats_t;
int sqe_set_profiling(sqe_ctx* ctx, int on);
int sqe_stats(sqe_ctx* ctx, sqe_stats_t* out);
int sqe_stats_reset(sqe_ctx* ctx);
/* Queries of the context's last collapsed search that the sweep over all rows answered (as uncertified and i8_overflows
 * report their fallbacks; summed over the shards of a device group).  An entry of its own and not a field of sqe_stats_t:
 * that struct's size is part of the ABI (callers compiled against an earlier header pass 128 bytes). */
int sqe_collapse_swept(sqe_ctx* ctx, int64_t* out);
/* The same of the context's last exclusion search (sqe_index_search_excluding). */
int sqe_exclude_swept(sqe_ctx* ctx, int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* SQE_H */
