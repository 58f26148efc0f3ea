// lexical.hip -- BM25 lexical index (sqe_lex_*): a chunked inverted index of integer impacts on the device, one LDS accumulator
// per row of a chunk, the block radix select of block_select.h for the best k.
//
// Definition (include/sqe.h has the full text).  I(t, d) = max(1, llrint(2^16 idf(t) tf / (tf + norm(d)))) in IEEE double
// arithmetic, score_int(q, d) = the sum of I over the query's term occurrences, a uint32 below 2^27.  Ranking: score_int
// descending, ties to the lowest id.  Scores are sums of integers: no floating-point accumulation order exists, so the answer
// cannot depend on batch size, posting order or chunking.
//
//   Host: a forward log of canonical bags (lexbag.cpp: distinct terms ascending, capped tf, dl), one entry per put; a replaced
//     or deleted document's entry goes dead.  Nothing touches the device until a search finds the index dirty.
//     A document put with sqe_lex_put_ordered also has its sequence in a log of its own (log_seq); the rebuild uploads the
//     live sequences in row order (seq_off, seq) when there is one, for the phrase kernels at the end of this file.
//   Rebuild (lex_rebuild, on the first search after a mutation): the live documents ordered by id are the rows, so a tie on the
//     row is a tie on the id.  df, idf (libm log) and avgdl come from the host; the compacted forward arrays are uploaded and
//     four kernels build the index.  Rows are cut into chunks of LEX_CHUNK; every chunk has its own CSR by term, a table
//     [chunks, n_terms + 1] of uint32 offsets relative to the chunk's first posting, which is fwd_off[first row of the chunk]:
//       lex_impact_kernel   one wave per row: norm(d) once, then I(t, d) of each of its postings, contraction off
//       lex_count_kernel    one wave per row: table[chunk][term] += 1 (global atomics)
//       lex_scan_kernel     one workgroup per chunk: exclusive scan of its table row
//       lex_scatter_kernel  one wave per row: (row, impact) to the chunk's run of the term through an atomic cursor
//     The order inside a (chunk, term) run is whatever the atomics gave; integer adds make it harmless.
//   Search: lex_score_kernel, grid (chunk, query), 256 threads: LEX_CHUNK uint32 accumulators in LDS, one LDS integer atomic
//     add per posting of the query's terms, then the chunk's best k keys (score_int << 32 | 0xFFFFFFFF - row, 0 = no hit) into
//     the partial [B, chunks, k].  A workgroup whose runs are all empty writes k zeros and leaves before zeroing the
//     accumulators.  lex_merge_kernel<BIAS>, one workgroup per query: select over chunks x k partial keys, rank, row -> id,
//     write; BIAS is what the keys carry on top of score_int (0 here).
// The query tables are host memory in both forms, copied per call from a vector the object owns.  A search that finds the
// index clean reads nothing back and synchronises nothing.  Scoring is booked under scan_ms, the merge under select_ms.
//   Boolean queries (sqe_lex_search_bool) and match sets (sqe_lex_match) follow further down with a score kernel and a bits
//     kernel of their own, phrase queries (sqe_lex_search_phrase, sqe_lex_match_phrase) after them with a third pair, over the
//     sequences that sqe_lex_put_ordered keeps beside the bags.  Their keys carry score_int + 1 (lex_merge_kernel<1>).
//   What the three kinds share stands once.  Device: lex_block_exscan, lex_add_run, lex_no_hits and lex_chunk_topk (the tail
//     of the three score kernels), lex_merge_kernel, lex_store_alive.  The argument structs derive from each other,
//     LexSearchArgs <- LexBoolArgs <- LexPhraseArgs: the host fills one LexPhraseArgs and a kernel takes the part it declares.
//     lex_bool_alive and lex_phrase_alive, the key lambda of their score kernels and the impact expression of
//     lex_impact_kernel and lex_phrase_add are spelled out twice on purpose: shared, they compile to other code and
//     measurably slower kernels (profiles/lexrefactor/NOTES.md).
//   Host (at the end of the namespace): LexQuery is the view of a call's host tables; lex_check validates it, lex_upload
//     copies it to the device and fills the shared arguments; lex_topk_run and lex_match_run hold the launch logic, sub-batches
//     included, with the kernel and its LDS bytes as parameters; lex_topk and lex_match are the host and _device forms over
//     them.  An entry point is a LexQuery, an argument check under its own name and one call.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <unordered_map>
#include <vector>

#include "block_select.h"
#include "internal.h"
#include "lexbag.h"

#ifndef SQE_LEX_CHUNK
#define SQE_LEX_CHUNK 16384
#endif

namespace sqe {

constexpr int LEX_CHUNK = SQE_LEX_CHUNK;       // rows of a chunk: 64 KiB of accumulators (two workgroups per CU); 32768: 128 KiB (one)
constexpr int LEX_THREADS = 256;
constexpr int LEX_LDS = LEX_CHUNK * 4;
static_assert((LEX_CHUNK & (LEX_CHUNK - 1)) == 0 && LEX_CHUNK >= 256 && LEX_CHUNK <= 32768, "LEX_CHUNK: a power of two whose accumulators fit the LDS");

}  // namespace sqe

struct sqe_lex {
    sqe_ctx* ctx = nullptr;
    sqe::OpOrder ord;
    int n_terms = 0;
    double k1 = 1.2, b = 0.75;
    // ---- host forward log
    struct Doc { int64_t id, off, dl; int32_t distinct; bool live; int64_t seq_off; };      // seq_off < 0: a bag, no sequence
    std::vector<Doc> docs;
    std::vector<int32_t> log_term;          // canonical bags one after the other
    std::vector<uint16_t> log_tf;
    std::vector<int32_t> log_seq;           // the sequences of the ordered documents (dl words each), a log of their own
    std::unordered_map<int64_t, size_t> by_id;      // live id -> docs entry
    int64_t live = 0, live_postings = 0;
    int64_t live_ordered = 0, live_seq = 0; // live documents that have a sequence, and the words of their sequences
    bool dirty = false;
    // ---- what the last rebuild made
    int64_t rows = 0, postings = 0;
    int chunks = 0, rebuilds = 0;
    double avgdl = 0.0, last_rebuild_ms = 0.0;
    std::vector<int32_t> df;
    std::vector<double> idf;
    int64_t seq_words = 0;                  // of the device index: words of d_seq
    bool has_seq = false;                   // the last rebuild found an ordered document and uploaded d_seq_off / d_seq
    sqe::DevBuf d_seq_off, d_seq;           // [rows + 1] int64: where the row's sequence starts (its length is dl), -1: no sequence; the last: seq_words
    sqe::DevBuf d_df, d_idf, d_ids, d_dl, d_fwd_off, d_fwd_term, d_fwd_tf, d_fwd_imp, d_table, d_cursor, d_post;
    // ---- per search
    sqe::DevBuf q_tables, partial, stage;
    sqe::DevBuf match_bits, match_offs;     // sqe_lex_match: the chunks' match maps and their counts / offsets
    std::vector<char> q_host;               // what the last search copied its query tables from (see FuseState::tables_host)
};

namespace sqe {
namespace {

// norm(d) = k1 * ((1 - b) + b * (dl / avgdl)): every operation rounded on its own, in this order
__device__ __forceinline__ double lex_norm(double k1, double b, int64_t dl, double avgdl) {
    return __dmul_rn(k1, __dadd_rn(__dsub_rn(1.0, b), __dmul_rn(b, __ddiv_rn((double)dl, avgdl))));
}

// Exclusive scan of row[0 .. n) in place by one workgroup; the entries from `valid` on count as 0, so row[valid] gets the total,
// which is also returned to every thread.
template <typename T>
__device__ __forceinline__ T lex_block_exscan(T* row, int valid, int n) {
    __shared__ T part[LEX_THREADS];
    __shared__ T s_total;
    const int tid = threadIdx.x;
    const int per = (n + LEX_THREADS - 1) / LEX_THREADS;
    const int i0 = min(tid * per, n), i1 = min(i0 + per, n);
    T sum = 0;
    for (int i = i0; i < i1; ++i) sum += i < valid ? row[i] : (T)0;
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        T run = 0;
        for (int i = 0; i < LEX_THREADS; ++i) {
            const T v = part[i];
            part[i] = run;
            run += v;
        }
        s_total = run;
    }
    __syncthreads();
    T run = part[tid];
    for (int i = i0; i < i1; ++i) {
        const T v = i < valid ? row[i] : (T)0;
        row[i] = run;
        run += v;
    }
    return s_total;
}

// ---------------------------------------------------------------- rebuild kernels
// one wave per row; 4 rows per workgroup
__global__ __launch_bounds__(LEX_THREADS) void lex_impact_kernel(const int64_t* __restrict__ fwd_off, const int32_t* __restrict__ fwd_term,
                                                                 const uint16_t* __restrict__ fwd_tf, const int64_t* __restrict__ dl,
                                                                 const double* __restrict__ idf, double k1, double b, double avgdl,
                                                                 int64_t rows, uint32_t* __restrict__ fwd_imp) {
#pragma clang fp contract(off)
    const int64_t row = (int64_t)blockIdx.x * (LEX_THREADS / WAVE) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const double norm = lex_norm(k1, b, dl[row], avgdl);
    const int64_t p1 = fwd_off[row + 1];
    for (int64_t p = fwd_off[row] + lane; p < p1; p += WAVE) {
        const double tf = (double)fwd_tf[p];
        const double x = __dmul_rn(__dmul_rn(idf[fwd_term[p]], __ddiv_rn(tf, __dadd_rn(tf, norm))), 0x1p16);      // ldexp(., 16): exact
        const long long i = __double2ll_rn(x);                                                                     // llrint: half to even
        fwd_imp[p] = (uint32_t)(i < 1 ? 1 : i);
    }
}

__global__ __launch_bounds__(LEX_THREADS) void lex_count_kernel(const int64_t* __restrict__ fwd_off, const int32_t* __restrict__ fwd_term,
                                                                int64_t rows, int n_terms, uint32_t* __restrict__ table) {
    const int64_t row = (int64_t)blockIdx.x * (LEX_THREADS / WAVE) + (threadIdx.x >> 6);
    if (row >= rows) return;
    uint32_t* t = table + (size_t)(row / LEX_CHUNK) * (n_terms + 1);
    const int64_t p1 = fwd_off[row + 1];
    for (int64_t p = fwd_off[row] + (threadIdx.x & 63); p < p1; p += WAVE) atomicAdd(&t[fwd_term[p]], 1u);
}

// table row of one chunk: counts [n_terms] (+ one unused entry) -> exclusive offsets [n_terms + 1]
__global__ __launch_bounds__(LEX_THREADS) void lex_scan_kernel(uint32_t* __restrict__ table, int n_terms) {
    (void)lex_block_exscan(table + (size_t)blockIdx.x * (n_terms + 1), n_terms, n_terms + 1);
}

__global__ __launch_bounds__(LEX_THREADS) void lex_scatter_kernel(const int64_t* __restrict__ fwd_off, const int32_t* __restrict__ fwd_term,
                                                                  const uint32_t* __restrict__ fwd_imp, int64_t rows, int n_terms,
                                                                  const uint32_t* __restrict__ table, uint32_t* __restrict__ cursor,
                                                                  uint2* __restrict__ post) {
    const int64_t row = (int64_t)blockIdx.x * (LEX_THREADS / WAVE) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t chunk = row / LEX_CHUNK;
    const uint32_t* t = table + (size_t)chunk * (n_terms + 1);
    uint32_t* cur = cursor + (size_t)chunk * n_terms;
    const int64_t base = fwd_off[chunk * LEX_CHUNK];      // the chunk's first posting
    const int64_t p1 = fwd_off[row + 1];
    for (int64_t p = fwd_off[row] + (threadIdx.x & 63); p < p1; p += WAVE) {
        const int term = fwd_term[p];
        const uint32_t at = t[term] + atomicAdd(&cur[term], 1u);      // < t[term + 1]: the count pass saw the same postings
        post[base + at] = make_uint2((uint32_t)row, fwd_imp[p]);
    }
}

// ---------------------------------------------------------------- search kernels
struct LexSearchArgs {
    const int64_t* fwd_off;        // [rows + 1]
    const uint32_t* table;         // [chunks, n_terms + 1]
    const uint2* post;
    const int64_t* ids;            // [rows]
    const int64_t* qoff;           // [B + 1]
    const int32_t* qterms;
    uint64_t* partial;             // [B, chunks, k]
    int64_t rows;
    int n_terms, chunks, k;
    float* score_out;              // [B, k]
    int64_t* id_out;
};

// a workgroup that can have no hit: k zeros to its place in the partial
__device__ __forceinline__ void lex_no_hits(uint64_t* out, int k) {
    for (int i = threadIdx.x; i < k; i += LEX_THREADS) out[i] = 0;
}

// The chunk's keys key_of(0 .. LEX_CHUNK) at or above T, their k-th best, to out[0 .. k), zeros behind them.  Keys are unique
// (the row is part of them) and 0 where the row is no hit.  Every thread calls; s_n was zeroed before the last barrier.
// The callers make the block_select_kth call for T themselves: with that one line in here the three score kernels come out
// with other VGPR counts (27 -> 25, 61 -> 62, 62 -> 63).
template <typename KeyOf>
__device__ __forceinline__ void lex_chunk_topk(KeyOf key_of, uint64_t T, int k, uint64_t* out, int& s_n) {
    const int tid = threadIdx.x;
    for (int i = tid; i < LEX_CHUNK; i += LEX_THREADS) {
        const uint64_t key = key_of(i);
        if (key != 0 && key >= T) {
            const int at = atomicAdd(&s_n, 1);
            if (at < k) out[at] = key;             // always: unique keys, so at most k of them reach the k-th
        }
    }
    __syncthreads();
    for (int i = min(s_n, k) + tid; i < k; i += LEX_THREADS) out[i] = 0;
}

// acc[row] += impact over one run of postings; every thread calls, no barrier
__device__ __forceinline__ void lex_add_run(const uint2* post, uint32_t beg, uint32_t end, uint32_t* acc) {
    for (uint32_t p = beg + threadIdx.x; p < end; p += LEX_THREADS) {
        const uint2 v = post[p];
        atomicAdd(&acc[v.x & (LEX_CHUNK - 1)], v.y);
    }
}

__global__ __launch_bounds__(LEX_THREADS) void lex_score_kernel(LexSearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lex_acc[];      // [LEX_CHUNK]
    __shared__ int hist[256];
    __shared__ uint32_t s_beg[LEX_MAX_QUERY], s_end[LEX_MAX_QUERY];
    __shared__ int s_any, s_n;
    const int chunk = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    const int64_t q0 = a.qoff[q];
    const int nq = (int)(a.qoff[q + 1] - q0);      // <= LEX_MAX_QUERY (checked by the entry points)
    const uint32_t* t = a.table + (size_t)chunk * (a.n_terms + 1);
    uint64_t* out = a.partial + ((size_t)q * a.chunks + chunk) * a.k;
    if (tid == 0) { s_any = 0; s_n = 0; }
    __syncthreads();
    if (tid < nq) {
        const int term = a.qterms[q0 + tid];
        const uint32_t b0 = t[term], b1 = t[term + 1];
        s_beg[tid] = b0;
        s_end[tid] = b1;
        if (b1 > b0) s_any = 1;
    }
    __syncthreads();
    if (!s_any) return lex_no_hits(out, a.k);      // no posting of any query term in this chunk (also the empty query)
    for (int i = tid; i < LEX_CHUNK; i += LEX_THREADS) lex_acc[i] = 0;
    __syncthreads();
    const int64_t row0 = (int64_t)chunk * LEX_CHUNK;
    const uint2* post = a.post + a.fwd_off[row0];
    for (int j = 0; j < nq; ++j) {                 // a repeated term walks its run again: it counts each time
        const uint32_t e = s_end[j];               // read before s_beg[j], as the code has always done
        lex_add_run(post, s_beg[j], e, lex_acc);
    }
    __syncthreads();
    // 0 only where no posting arrived: every impact is >= 1
    const auto key_of = [&](int i) {
        const uint32_t sc = lex_acc[i];
        return sc ? ((uint64_t)sc << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)(row0 + i)) : (uint64_t)0;
    };
    const uint64_t T = block_select_kth<LEX_THREADS, uint64_t, true>(each_key<LEX_THREADS>(key_of, LEX_CHUNK), a.k, hist);
    lex_chunk_topk(key_of, T, a.k, out, s_n);
}

// One workgroup per query: the best k of its chunks x k partial keys, ranked, row -> id.  BIAS: what the keys carry on top of
// score_int (0: the plain search, 1: boolean and phrase searches).
template <uint32_t BIAS>
__global__ __launch_bounds__(LEX_THREADS) void lex_merge_kernel(LexSearchArgs a) {
    __shared__ int hist[256];
    __shared__ uint64_t top[MAX_KP];
    __shared__ int s_n;
    const int q = blockIdx.x, tid = threadIdx.x;
    const uint64_t* in = a.partial + (size_t)q * a.chunks * a.k;
    const int n = a.chunks * a.k;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const uint64_t T = block_select_kth<LEX_THREADS, uint64_t, true>(each_key<LEX_THREADS>([&](int i) { return in[i]; }, n), a.k, hist);
    for (int i = tid; i < n; i += LEX_THREADS) {
        const uint64_t key = in[i];
        if (key != 0 && key >= T) {
            const int at = atomicAdd(&s_n, 1);
            if (at < MAX_KP) top[at] = key;
        }
    }
    __syncthreads();
    const int m = min(s_n, a.k);
    float* so = a.score_out + (size_t)q * a.k;
    int64_t* io = a.id_out + (size_t)q * a.k;
    for (int i = tid; i < m; i += LEX_THREADS) {
        const uint64_t ki = top[i];
        int rank = 0;
        for (int j = 0; j < m; ++j) rank += top[j] > ki ? 1 : 0;
        so[rank] = (float)((double)((uint32_t)(ki >> 32) - BIAS) * 0x1p-16);
        io[rank] = a.ids[0xFFFFFFFFu - (uint32_t)ki];
    }
    for (int i = m + tid; i < a.k; i += LEX_THREADS) {
        so[i] = -INFINITY;
        io[i] = -1;
    }
}

// ---------------------------------------------------------------- rebuild
template <typename T>
int upload(DevBuf& buf, const std::vector<T>& v, hipStream_t s) {
    SQE_TRY(buf.ensure(std::max<size_t>(v.size() * sizeof(T), 16)));
    if (!v.empty()) SQE_HIP(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return SQE_OK;
}

// The live documents of the forward log as a fresh index.  Synchronises s (the host arrays it uploads from are its own).
int lex_rebuild(sqe_lex* L, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    const int T = L->n_terms;
    std::vector<const sqe_lex::Doc*> order;
    order.reserve((size_t)L->live);
    for (const auto& d : L->docs)
        if (d.live) order.push_back(&d);
    std::sort(order.begin(), order.end(), [](const sqe_lex::Doc* x, const sqe_lex::Doc* y) { return x->id < y->id; });
    const int64_t N = (int64_t)order.size();
    std::vector<int64_t> ids((size_t)N), dl((size_t)N), fwd_off((size_t)N + 1);
    std::vector<int32_t> fwd_term((size_t)L->live_postings);
    std::vector<uint16_t> fwd_tf((size_t)L->live_postings);
    L->df.assign((size_t)T, 0);
    // the live sequences in row order; an index without an ordered document builds, uploads and allocates none of this
    const bool has_seq = L->live_ordered > 0;
    std::vector<int64_t> seq_off(has_seq ? (size_t)N + 1 : 0);
    std::vector<int32_t> seq;
    seq.reserve(has_seq ? (size_t)L->live_seq : 0);
    int64_t P = 0, total_dl = 0;
    for (int64_t r = 0; r < N; ++r) {
        const sqe_lex::Doc& d = *order[(size_t)r];
        ids[(size_t)r] = d.id;
        dl[(size_t)r] = d.dl;
        total_dl += d.dl;
        if (has_seq) {
            seq_off[(size_t)r] = d.seq_off < 0 ? -1 : (int64_t)seq.size();
            if (d.seq_off >= 0) seq.insert(seq.end(), L->log_seq.begin() + d.seq_off, L->log_seq.begin() + d.seq_off + d.dl);
        }
        fwd_off[(size_t)r] = P;
        for (int32_t j = 0; j < d.distinct; ++j) {
            const int32_t term = L->log_term[(size_t)(d.off + j)];
            fwd_term[(size_t)P] = term;
            fwd_tf[(size_t)P] = L->log_tf[(size_t)(d.off + j)];
            L->df[(size_t)term]++;
            ++P;
        }
    }
    fwd_off[(size_t)N] = P;
    if (has_seq) seq_off[(size_t)N] = (int64_t)seq.size();
    L->avgdl = N > 0 ? (double)total_dl / (double)N : 0.0;
    L->idf.assign((size_t)T, 0.0);
    for (int t = 0; t < T; ++t) {
        const int32_t f = L->df[(size_t)t];
        if (f > 0) L->idf[(size_t)t] = log(1.0 + ((double)(N - f) + 0.5) / ((double)f + 0.5));
    }
    // the dead entries leave the log once they outweigh the live ones
    if (L->log_term.size() > 2 * (size_t)P + 1024 || L->log_seq.size() > 2 * seq.size() + 1024) {
        std::vector<sqe_lex::Doc> docs;
        docs.reserve((size_t)N);
        L->by_id.clear();
        for (int64_t r = 0; r < N; ++r) {
            sqe_lex::Doc d = *order[(size_t)r];
            d.off = fwd_off[(size_t)r];
            if (d.seq_off >= 0) d.seq_off = seq_off[(size_t)r];
            L->by_id[d.id] = docs.size();
            docs.push_back(d);
        }
        L->docs.swap(docs);
        L->log_term = fwd_term;
        L->log_tf = fwd_tf;
        L->log_seq = seq;
    }
    const int chunks = (int)((N + LEX_CHUNK - 1) / LEX_CHUNK);
    L->rows = N;
    L->postings = P;
    L->chunks = chunks;
    L->has_seq = has_seq;
    L->seq_words = (int64_t)seq.size();
    if (has_seq) {
        SQE_TRY(upload(L->d_seq_off, seq_off, s));
        SQE_TRY(upload(L->d_seq, seq, s));
    }
    if (N > 0) {
        SQE_TRY(upload(L->d_ids, ids, s));
        SQE_TRY(upload(L->d_dl, dl, s));
        SQE_TRY(upload(L->d_fwd_off, fwd_off, s));
        SQE_TRY(upload(L->d_fwd_term, fwd_term, s));
        SQE_TRY(upload(L->d_fwd_tf, fwd_tf, s));
        SQE_TRY(upload(L->d_df, L->df, s));
        SQE_TRY(upload(L->d_idf, L->idf, s));
        const size_t table_bytes = (size_t)chunks * (T + 1) * 4, cursor_bytes = (size_t)chunks * T * 4;
        SQE_TRY(L->d_fwd_imp.ensure(std::max<size_t>((size_t)P * 4, 16)));
        SQE_TRY(L->d_post.ensure(std::max<size_t>((size_t)P * 8, 16)));
        SQE_TRY(L->d_table.ensure(table_bytes));
        SQE_TRY(L->d_cursor.ensure(cursor_bytes));
        SQE_HIP(hipMemsetAsync(L->d_table.p, 0, table_bytes, s));
        SQE_HIP(hipMemsetAsync(L->d_cursor.p, 0, cursor_bytes, s));
        const unsigned g = grid_of(N, LEX_THREADS / WAVE);
        hipLaunchKernelGGL(lex_impact_kernel, dim3(g), dim3(LEX_THREADS), 0, s, L->d_fwd_off.as<int64_t>(), L->d_fwd_term.as<int32_t>(),
                           L->d_fwd_tf.as<uint16_t>(), L->d_dl.as<int64_t>(), L->d_idf.as<double>(), L->k1, L->b, L->avgdl, N,
                           L->d_fwd_imp.as<uint32_t>());
        hipLaunchKernelGGL(lex_count_kernel, dim3(g), dim3(LEX_THREADS), 0, s, L->d_fwd_off.as<int64_t>(), L->d_fwd_term.as<int32_t>(), N, T,
                           L->d_table.as<uint32_t>());
        hipLaunchKernelGGL(lex_scan_kernel, dim3(chunks), dim3(LEX_THREADS), 0, s, L->d_table.as<uint32_t>(), T);
        hipLaunchKernelGGL(lex_scatter_kernel, dim3(g), dim3(LEX_THREADS), 0, s, L->d_fwd_off.as<int64_t>(), L->d_fwd_term.as<int32_t>(),
                           L->d_fwd_imp.as<uint32_t>(), N, T, L->d_table.as<uint32_t>(), L->d_cursor.as<uint32_t>(), L->d_post.as<uint2>());
        SQE_HIP(hipGetLastError());
    }
    SQE_HIP(hipStreamSynchronize(s));
    L->dirty = false;
    L->rebuilds++;
    L->last_rebuild_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SQE_OK;
}

}  // namespace

sqe_ctx* lex_ctx(sqe_lex* L) { return L->ctx; }

int lex_query_check(const char* who, sqe_lex* L, const int64_t* qoff, const int32_t* qterms, int B) {
    if (B == 0) return SQE_OK;
    if (const char* why = lexbag_check(qoff, B, qterms, L->n_terms, LEX_MAX_QUERY)) return fail(SQE_ERR_INVALID, std::string(who) + ": " + why);
    return SQE_OK;
}

// ================================================================ boolean queries: sqe_lex_search_bool, sqe_lex_match
// Every occurrence carries a role and every query a min_should (include/sqe.h has the rules).  The match state of a chunk is
// one bit per row: LEX_WORDS words `alive`, and a second map `cur` that each clause fills with LDS atomic ORs before the
// thread that owns a word folds it into alive (required: &=, denied: &= ~).  Only min_should >= 2 needs a count per row: byte
// counters, one word-wide LDS atomic add of 1 << 8 * (row & 3) per posting -- a query has at most 64 occurrences, so a byte
// never carries into its neighbour.  The match state is complete before the first impact is added, so the scoring kernel
// keeps the counters in the accumulators' space and pays 4 KiB of LDS for the two maps, nothing else.
//   lex_bool_score_kernel   grid (chunk, query): match state, then the plain kernel's accumulation over the SHOULD and MUST
//     occurrences; key = (score_int + 1) << 32 | 0xFFFFFFFF - row for the rows alive (a FILTER-only match scores 0 and stays
//     a key), 0 for the others; same select and lex_chunk_topk, same partial; lex_merge_kernel<1> takes the + 1 off again.
//     Leaves before zeroing the accumulators when no row is alive.
//   lex_match_bits_kernel   grid (chunk, query): the chunk's alive map to global memory and its popcount
//   lex_match_scan_kernel   one workgroup per query: exclusive scan of the chunk counts, count_out, the -1 tail of id_out
//   lex_match_expand_kernel grid (chunk, query): ballot / popcount prefix per 64 rows, ids to the chunk's offset, up to cap
// No floating point anywhere but the score conversion of the merge.
namespace {

constexpr int LEX_WORDS = LEX_CHUNK / 32;             // words of a one-bit-per-row map of a chunk
constexpr int LEX_GROUPS = LEX_CHUNK / 64;            // 64-row groups of a chunk: one ballot each
constexpr int LEX_BOOL_LDS = LEX_LDS + 2 * LEX_WORDS * 4;                        // accumulators (before them the counters) | alive | cur
constexpr int LEX_MATCH_LDS = LEX_CHUNK + 2 * LEX_WORDS * 4;                     // byte counters | alive | cur
constexpr size_t LEX_MATCH_BITS_BYTES = (size_t)256 << 20;                       // the bit maps of one sub-batch of sqe_lex_match

struct LexBoolArgs : LexSearchArgs {      // partial, score_out and id_out: sqe_lex_search_bool only
    const uint8_t* qroles;         // one per occurrence
    const int32_t* min_should;     // [B]
    uint32_t* bits;                // [B, chunks, LEX_WORDS]           sqe_lex_match only, as what follows
    int64_t* offs;                 // [B, chunks + 1]: counts, then exclusive offsets and the total
    int64_t* count_out;            // [B]
    int64_t* match_out;            // [B, cap]
    int64_t cap;
};

struct LexBoolShared {
    uint32_t beg[LEX_MAX_QUERY], end[LEX_MAX_QUERY];
    uint8_t role[LEX_MAX_QUERY];
    int n_req, n_should, req_empty, should_runs, deny_runs, live;
};

__device__ __forceinline__ bool lex_scores(int role) { return role == SQE_LEX_SHOULD || role == SQE_LEX_MUST; }
__device__ __forceinline__ bool lex_requires(int role) { return role == SQE_LEX_MUST || role == SQE_LEX_FILTER; }

// cur = the rows of the runs of the occurrences that `pick` takes; every thread calls
template <typename Pick>
__device__ __forceinline__ void lex_mark_runs(const LexBoolShared& sh, int nq, const uint2* post, uint32_t* cur, Pick pick) {
    const int tid = threadIdx.x;
    for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) cur[w] = 0;
    __syncthreads();
    for (int j = 0; j < nq; ++j) {
        if (!pick(j)) continue;
        const uint32_t e = sh.end[j];
        for (uint32_t p = sh.beg[j] + tid; p < e; p += LEX_THREADS) {
            const uint32_t r = post[p].x & (LEX_CHUNK - 1);
            atomicOr(&cur[r >> 5], 1u << (r & 31));
        }
    }
    __syncthreads();
}

// The match state of chunk `chunk` for query q: alive[LEX_WORDS], one bit per row; cur[LEX_WORDS] and cnt[LEX_CHUNK / 4] are
// scratch.  Returns the number of rows alive, block-uniform; 0 may come before alive was written.  Thread t alone writes the
// words t, t + LEX_THREADS, ... of alive, so its folds need no barrier of their own.
// lazy_should: a caller that scores may leave "some SHOULD occurrence holds" of a query without MUST / FILTER and with
// m == 1 to its accumulators (every scoring occurrence is then a SHOULD one and every impact >= 1): need_pos says it did, and
// the count returned is then an upper bound.
__device__ __forceinline__ int lex_bool_alive(const LexBoolArgs& a, int chunk, int q, LexBoolShared& sh, uint32_t* alive, uint32_t* cur,
                                              uint32_t* cnt, bool lazy_should, bool& need_pos) {
    const int tid = threadIdx.x;
    const int64_t q0 = a.qoff[q];
    const int nq = (int)(a.qoff[q + 1] - q0);      // <= LEX_MAX_QUERY (checked by the entry points)
    const uint32_t* t = a.table + (size_t)chunk * (a.n_terms + 1);
    need_pos = false;
    if (tid == 0) sh.n_req = sh.n_should = sh.req_empty = sh.should_runs = sh.deny_runs = sh.live = 0;
    __syncthreads();
    if (tid < nq) {
        const int term = a.qterms[q0 + tid], role = a.qroles[q0 + tid];
        const uint32_t b0 = t[term], b1 = t[term + 1];
        sh.beg[tid] = b0;
        sh.end[tid] = b1;
        sh.role[tid] = (uint8_t)role;
        if (lex_requires(role)) {
            atomicAdd(&sh.n_req, 1);
            if (b1 == b0) sh.req_empty = 1;
        } else if (role == SQE_LEX_SHOULD) {
            atomicAdd(&sh.n_should, 1);
            if (b1 > b0) sh.should_runs = 1;
        } else if (b1 > b0) {
            sh.deny_runs = 1;
        }
    }
    __syncthreads();
    const int n_req = sh.n_req, n_should = sh.n_should;
    const int m = n_req ? a.min_should[q] : max(1, a.min_should[q]);
    // no positive occurrence; more wanted than there are; a required term without a posting here; no SHOULD posting where one is needed
    if (n_req + n_should == 0 || m > n_should || sh.req_empty || (m >= 1 && !sh.should_runs)) return 0;
    const int64_t row0 = (int64_t)chunk * LEX_CHUNK;
    const int nrows = (int)min((int64_t)LEX_CHUNK, a.rows - row0);
    const uint2* post = a.post + a.fwd_off[row0];
    for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) {
        const int lo = w * 32;
        alive[w] = nrows >= lo + 32 ? 0xFFFFFFFFu : nrows > lo ? (1u << (nrows - lo)) - 1u : 0u;
    }
    for (int j = 0; j < nq; ++j) {
        if (!lex_requires(sh.role[j])) continue;
        lex_mark_runs(sh, nq, post, cur, [&](int i) { return i == j; });
        for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) alive[w] &= cur[w];
    }
    if (m == 1 && n_req == 0 && lazy_should) {
        need_pos = true;
    } else if (m == 1) {
        lex_mark_runs(sh, nq, post, cur, [&](int i) { return sh.role[i] == SQE_LEX_SHOULD; });
        for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) alive[w] &= cur[w];
    } else if (m >= 2) {
        for (int i = tid; i < LEX_CHUNK / 4; i += LEX_THREADS) cnt[i] = 0;
        __syncthreads();
        for (int j = 0; j < nq; ++j) {
            if (sh.role[j] != SQE_LEX_SHOULD) continue;      // a repeated occurrence walks its run again: it counts each time
            const uint32_t e = sh.end[j];
            for (uint32_t p = sh.beg[j] + tid; p < e; p += LEX_THREADS) {
                const uint32_t r = post[p].x & (LEX_CHUNK - 1);
                atomicAdd(&cnt[r >> 2], 1u << (8 * (r & 3)));
            }
        }
        __syncthreads();
        for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) {
            uint32_t enough = 0;
            for (int i = 0; i < 8; ++i) {
                const uint32_t c = cnt[w * 8 + i];
                for (int b = 0; b < 4; ++b) enough |= (uint32_t)((int)((c >> (8 * b)) & 255u) >= m) << (i * 4 + b);
            }
            alive[w] &= enough;
        }
    }
    if (sh.deny_runs) {
        lex_mark_runs(sh, nq, post, cur, [&](int i) { return sh.role[i] == SQE_LEX_MUST_NOT; });
        for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) alive[w] &= ~cur[w];
    }
    int live = 0;
    for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) live += __popc(alive[w]);
    if (live) atomicAdd(&sh.live, live);
    __syncthreads();                               // also: alive is complete for every thread, cnt is free again
    return sh.live;
}

// the chunk's count to offs and, where a row is alive, its map to bits (lex_match_expand_kernel does not read the map of a
// chunk without one)
__device__ __forceinline__ void lex_store_alive(const LexBoolArgs& a, int chunk, int q, int live, const uint32_t* alive) {
    const int tid = threadIdx.x;
    if (tid == 0) a.offs[(size_t)q * (a.chunks + 1) + chunk] = live;
    if (live == 0) return;
    uint32_t* bits = a.bits + ((size_t)q * a.chunks + chunk) * LEX_WORDS;
    for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) bits[w] = alive[w];
}

__global__ __launch_bounds__(LEX_THREADS) void lex_bool_score_kernel(LexBoolArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lex_bool_lds[];      // [LEX_CHUNK] accumulators | alive | cur
    __shared__ LexBoolShared sh;
    __shared__ int hist[256];
    __shared__ int s_n;
    uint32_t* acc = lex_bool_lds;
    uint32_t* alive = lex_bool_lds + LEX_CHUNK;
    uint32_t* cur = alive + LEX_WORDS;
    const int chunk = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    uint64_t* out = a.partial + ((size_t)q * a.chunks + chunk) * a.k;
    if (tid == 0) s_n = 0;
    bool need_pos;
    if (lex_bool_alive(a, chunk, q, sh, alive, cur, acc, true, need_pos) == 0) return lex_no_hits(out, a.k);
    for (int i = tid; i < LEX_CHUNK; i += LEX_THREADS) acc[i] = 0;
    __syncthreads();
    const int nq = (int)(a.qoff[q + 1] - a.qoff[q]);
    const int64_t row0 = (int64_t)chunk * LEX_CHUNK;
    const uint2* post = a.post + a.fwd_off[row0];
    for (int j = 0; j < nq; ++j)
        if (lex_scores(sh.role[j])) lex_add_run(post, sh.beg[j], sh.end[j], acc);
    __syncthreads();
    // unique keys; score_int + 1 keeps a match that scores 0 apart from "no hit" (score_int < 2^27: no overflow)
    const auto key_of = [&](int i) {
        const uint32_t sc = acc[i];
        const bool hit = ((alive[i >> 5] >> (i & 31)) & 1u) && (sc || !need_pos);
        return hit ? ((uint64_t)(sc + 1u) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)(row0 + i)) : (uint64_t)0;
    };
    const uint64_t T = block_select_kth<LEX_THREADS, uint64_t, true>(each_key<LEX_THREADS>(key_of, LEX_CHUNK), a.k, hist);
    lex_chunk_topk(key_of, T, a.k, out, s_n);
}

__global__ __launch_bounds__(LEX_THREADS) void lex_match_bits_kernel(LexBoolArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lex_match_lds[];     // [LEX_CHUNK / 4] byte counters | alive | cur
    __shared__ LexBoolShared sh;
    uint32_t* cnt = lex_match_lds;
    uint32_t* alive = lex_match_lds + LEX_CHUNK / 4;
    uint32_t* cur = alive + LEX_WORDS;
    const int chunk = blockIdx.x, q = blockIdx.y;
    bool need_pos;
    lex_store_alive(a, chunk, q, lex_bool_alive(a, chunk, q, sh, alive, cur, cnt, false, need_pos), alive);
}

// offs row of one query: counts [chunks] (+ one unused entry) -> exclusive offsets [chunks + 1], the last one the total, which
// also goes to count_out; the places of id_out that no match will fill get -1.  chunks == 0 (an empty index) is valid.
__global__ __launch_bounds__(LEX_THREADS) void lex_match_scan_kernel(LexBoolArgs a) {
    const int q = blockIdx.x, tid = threadIdx.x;
    const int64_t total = lex_block_exscan(a.offs + (size_t)q * (a.chunks + 1), a.chunks, a.chunks + 1);
    if (tid == 0) a.count_out[q] = total;
    for (int64_t i = min(total, a.cap) + tid; i < a.cap; i += LEX_THREADS) a.match_out[(size_t)q * a.cap + i] = -1;
}

// Rows ascend with ids, so the matches of a chunk go to id_out in row order from the chunk's offset: per 64 rows one ballot,
// a lane's place is the popcount of the lanes below it after the matches of the groups before.
__global__ __launch_bounds__(LEX_THREADS) void lex_match_expand_kernel(LexBoolArgs a) {
    __shared__ uint32_t pref[LEX_GROUPS];
    const int chunk = blockIdx.x, q = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int64_t* o = a.offs + (size_t)q * (a.chunks + 1);
    const int64_t base = o[chunk];
    if (o[chunk + 1] == base || base >= a.cap) return;
    const uint32_t* bits = a.bits + ((size_t)q * a.chunks + chunk) * LEX_WORDS;
    for (int g = tid; g < LEX_GROUPS; g += LEX_THREADS) pref[g] = __popc(bits[2 * g]) + __popc(bits[2 * g + 1]);
    __syncthreads();
    if (tid < WAVE) {                              // exclusive scan of pref by one wave: PER consecutive groups per lane
        constexpr int PER = (LEX_GROUPS + WAVE - 1) / WAVE;
        uint32_t v[PER], sum = 0;
        for (int i = 0; i < PER; ++i) {
            const int g = tid * PER + i;
            v[i] = g < LEX_GROUPS ? pref[g] : 0u;
            sum += v[i];
        }
        uint32_t inc = sum;
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d);
            if (tid >= d) inc += up;
        }
        uint32_t run = inc - sum;
        for (int i = 0; i < PER; ++i) {
            const int g = tid * PER + i;
            if (g < LEX_GROUPS) pref[g] = run;
            run += v[i];
        }
    }
    __syncthreads();
    const int64_t row0 = (int64_t)chunk * LEX_CHUNK;
    int64_t* out = a.match_out + (size_t)q * a.cap;
    for (int g = tid >> 6; g < LEX_GROUPS; g += LEX_THREADS / WAVE) {
        const int64_t at = base + pref[g];
        if (at >= a.cap) break;                    // wave-uniform; the groups after it lie further still
        const bool hit = (bits[2 * g + (lane >> 5)] >> (lane & 31)) & 1u;
        const unsigned long long mask = __ballot(hit);
        const int64_t pos = at + __popcll(mask & ((1ull << lane) - 1ull));
        if (hit && pos < a.cap) out[pos] = a.ids[row0 + g * 64 + lane];      // a set bit is a row below rows
    }
}

// ================================================================ phrase queries: sqe_lex_search_phrase, sqe_lex_match_phrase
// A query is a list of CLAUSES, a clause a list of terms, the role belongs to the clause (include/sqe.h has the rules).  A clause
// of one term is an occurrence of the boolean kernels and is treated as there.  A clause of L >= 2 terms is a phrase:
//   candidates   cand = the AND of the runs of its terms (a map per term through tmp), ANDed with alive: only rows that can
//                still match are looked at.  A phrase with a term that has no posting in the chunk, and any phrase on an index
//                without sequences, is dead here.
//   verification a wave per candidate row, its lanes over the start positions p <= dl - L of the row's sequence: t_0 first, the
//                rest only on a hit; pf = the sum of the ballot popcounts.  The bound is dl - L, so no position is tried whose
//                tail would lie in the next row's sequence.
// Required one-term clauses go first, then the required phrases, the SHOULD clauses (a union map for m == 1, the byte counters
// for m >= 2) and the MUST_NOT clauses last, when alive is smallest.  A scoring phrase adds I(c, d) from pf where it is verified.
// With m < 2 that is the verification of the match state: the accumulators' space is free then (lex_phrase_alive).  With m >= 2
// it holds the byte counters, and the scoring kernel verifies the phrase a second time over the rows alive at the end, a
// subset of what the first verification saw; so it does for a SHOULD phrase that the match state never looked at.
//   lex_phrase_score_kernel  grid (chunk, query): lex_bool_score_kernel over clauses; same keys, same partial, same merge kernel
//   lex_phrase_bits_kernel   grid (chunk, query): lex_match_bits_kernel over clauses; the scan and expand kernels are reused
constexpr int LEX_PHRASE_LDS = LEX_LDS + 4 * LEX_WORDS * 4;                      // accumulators (before them the counters) | alive | cur | cand | tmp
constexpr int LEX_PHRASE_MATCH_LDS = LEX_CHUNK + 4 * LEX_WORDS * 4;              // byte counters | alive | cur | cand | tmp
static_assert(LEX_CHUNK > 16384 || LEX_PHRASE_LDS + 4096 <= 80 * 1024, "two phrase workgroups per CU");

struct LexPhraseArgs : LexBoolArgs {      // qoff: [B + 1] clause ranges; qterms: the occurrences; qroles: one per CLAUSE
    const int64_t* coff;           // [C + 1] occurrence ranges of the clauses
    const int64_t* seq_off;        // [rows + 1], -1: the row has no sequence; null: the index has none at all
    const int32_t* seq;
    const int64_t* dl;             // [rows]: the length of a row's sequence
    const double* idf;             // [n_terms]
    double k1, bm, avgdl;
};

struct LexPhraseShared {
    double cidf[LEX_MAX_QUERY];                            // per clause: idf(t_0) + idf(t_1) + ..., left to right
    uint32_t beg[LEX_MAX_QUERY], end[LEX_MAX_QUERY];       // per occurrence: the run of its term in this chunk
    int32_t term[LEX_MAX_QUERY];                           // per occurrence
    uint8_t first[LEX_MAX_QUERY + 1];                      // clause -> its first occurrence (of this query)
    uint8_t role[LEX_MAX_QUERY], dead[LEX_MAX_QUERY];      // per clause; dead: holds nowhere in this chunk
    uint8_t scored[LEX_MAX_QUERY];                         // per clause: a phrase that scored while the match state was made
    int n_req, n_should, req_empty, should_runs, deny_runs, live, n_cand, acc_ready;
};

// map |= the rows of one run; every thread calls, no barrier
__device__ __forceinline__ void lex_or_run(const uint2* post, uint32_t beg, uint32_t end, uint32_t* map) {
    for (uint32_t p = beg + threadIdx.x; p < end; p += LEX_THREADS) {
        const uint32_t r = post[p].x & (LEX_CHUNK - 1);
        atomicOr(&map[r >> 5], 1u << (r & 31));
    }
}

// cand = the rows alive that hold every term of phrase c; returns their number, block-uniform.  Every thread calls; thread t
// alone folds the words t, t + LEX_THREADS, ... of cand, as it does for alive.
__device__ __forceinline__ int lex_phrase_cand(LexPhraseShared& sh, int c, const uint2* post, const uint32_t* alive, uint32_t* cand, uint32_t* tmp) {
    const int tid = threadIdx.x, o0 = sh.first[c], o1 = sh.first[c + 1];
    for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) cand[w] = 0;
    if (tid == 0) sh.n_cand = 0;
    __syncthreads();
    lex_or_run(post, sh.beg[o0], sh.end[o0], cand);
    __syncthreads();
    for (int o = o0 + 1; o < o1; ++o) {
        for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) tmp[w] = 0;
        __syncthreads();
        lex_or_run(post, sh.beg[o], sh.end[o], tmp);
        __syncthreads();
        for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) cand[w] &= tmp[w];
    }
    int n = 0;
    for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) {
        const uint32_t v = cand[w] & alive[w];
        cand[w] = v;
        n += __popc(v);
    }
    if (n) atomicAdd(&sh.n_cand, n);
    __syncthreads();
    return sh.n_cand;
}

// pf(c, d) of every row of cand, a wave per row: hit(r, pf) is called by every lane of the wave that took row r (r relative to
// the chunk) where pf >= 1, pf capped at LEX_TF_CAP.  Every thread calls; ends with a barrier, so cand is free afterwards.
template <typename Hit>
__device__ __forceinline__ void lex_phrase_verify(const LexPhraseArgs& a, const LexPhraseShared& sh, int c, int64_t row0, const uint32_t* cand, Hit hit) {
    const int lane = threadIdx.x & 63, o0 = sh.first[c], len = sh.first[c + 1] - o0;
    const int32_t t0 = sh.term[o0];
    for (int w = threadIdx.x >> 6; w < LEX_WORDS; w += LEX_THREADS / WAVE) {
        uint32_t bits = __builtin_amdgcn_readfirstlane(cand[w]);
        if (!bits) continue;
        // lane i fetches where the sequence of the word's row i starts and how long it is: one round trip for the word's
        // candidates instead of one per row (a set bit is a row below rows)
        long long my_at = -1, my_dl = 0;
        if (lane < 32 && ((bits >> lane) & 1u)) {
            my_at = a.seq_off[row0 + w * 32 + lane];
            my_dl = a.dl[row0 + w * 32 + lane];
        }
        while (bits) {
            const int bit = __builtin_ctz(bits), r = w * 32 + bit;
            bits &= bits - 1;
            const int64_t at = __shfl(my_at, bit);
            if (at < 0) continue;                              // a bag: it holds no phrase
            const int64_t last = (int64_t)__shfl(my_dl, bit) - len;      // the last start position; past it the tail leaves the row's sequence
            const int32_t* sq = a.seq + at;
            int64_t pf = 0;
            for (int64_t p0 = 0; p0 <= last; p0 += 4 * WAVE) {          // four strides at once: their first words are loaded together
                int32_t first[4];
                for (int u = 0; u < 4; ++u) {
                    const int64_t p = p0 + u * WAVE + lane;
                    first[u] = p <= last ? sq[p] : -1;         // no term is negative
                }
                for (int u = 0; u < 4; ++u) {
                    const int64_t p = p0 + u * WAVE + lane;
                    bool ok = first[u] == t0;
                    if (ok)
                        for (int j = 1; j < len; ++j)
                            if (sq[p + j] != sh.term[o0 + j]) { ok = false; break; }
                    pf += __popcll(__ballot(ok));
                }
            }
            if (pf) hit(r, pf < LEX_TF_CAP ? (int)pf : LEX_TF_CAP);
        }
    }
    __syncthreads();
}

// I(c, d) of phrase clause c in row r (relative to the chunk) into its accumulator: lex_impact_kernel's expression with idf(c)
// and pf in place of idf(t) and tf.  One lane calls.
__device__ __forceinline__ void lex_phrase_add(const LexPhraseArgs& a, const LexPhraseShared& sh, int c, int64_t row0, int r, int pf, uint32_t* acc) {
#pragma clang fp contract(off)
    const double norm = lex_norm(a.k1, a.bm, a.dl[row0 + r], a.avgdl), f = (double)pf;
    const double x = __dmul_rn(__dmul_rn(sh.cidf[c], __ddiv_rn(f, __dadd_rn(f, norm))), 0x1p16);
    const long long i = __double2ll_rn(x);
    atomicAdd(&acc[r], (uint32_t)(i < 1 ? 1 : i));
}

#ifdef SQE_LEX_PHRASE_REVERIFY
constexpr bool LEX_PHRASE_EARLY = false;       // measurement build (make PHRASE_REVERIFY=1): every scoring phrase is verified twice
#else
constexpr bool LEX_PHRASE_EARLY = true;
#endif

// lex_bool_alive over clauses; cand and tmp are two more maps of LEX_WORDS words.
// acc (null: the caller does not score): with m < 2 no byte counter is needed, so the accumulators' space is free while the
// match state is made, and a scoring phrase that is verified here adds its impact at once instead of being verified again
// when scoring: acc is zeroed before the first such phrase (sh.acc_ready) and the clause is marked in sh.scored.  A row that
// dies afterwards keeps what it got; its key is 0 all the same.
__device__ __forceinline__ int lex_phrase_alive(const LexPhraseArgs& a, int chunk, int q, LexPhraseShared& sh, uint32_t* alive, uint32_t* cur,
                                                uint32_t* cand, uint32_t* tmp, uint32_t* cnt, uint32_t* acc, bool lazy_should, bool& need_pos) {
    const int tid = threadIdx.x;
    const int64_t c0 = a.qoff[q];
    const int nc = (int)(a.qoff[q + 1] - c0);    // <= LEX_MAX_QUERY: no clause is empty and the occurrences are at most that
    const int64_t o0 = a.coff[c0];
    const int nocc = (int)(a.coff[c0 + nc] - o0);    // <= LEX_MAX_QUERY (checked by the entry points)
    const uint32_t* t = a.table + (size_t)chunk * (a.n_terms + 1);
    need_pos = false;
    if (tid == 0) sh.n_req = sh.n_should = sh.req_empty = sh.should_runs = sh.deny_runs = sh.live = sh.acc_ready = 0;
    if (tid < LEX_MAX_QUERY) sh.scored[tid] = 0;
    if (tid <= nc) sh.first[tid] = (uint8_t)(a.coff[c0 + tid] - o0);
    if (tid < nocc) {
        const int term = a.qterms[o0 + tid];
        sh.term[tid] = term;
        sh.beg[tid] = t[term];
        sh.end[tid] = t[term + 1];
    }
    __syncthreads();
    if (tid < nc) {
        const int role = a.qroles[c0 + tid], f0 = sh.first[tid], f1 = sh.first[tid + 1];
        bool dead = f1 - f0 >= 2 && !a.seq_off;
        double idf = a.idf[sh.term[f0]];
        for (int o = f0; o < f1; ++o) {
            if (sh.end[o] == sh.beg[o]) dead = true;
            if (o > f0) idf = __dadd_rn(idf, a.idf[sh.term[o]]);
        }
        sh.cidf[tid] = idf;
        sh.role[tid] = (uint8_t)role;
        sh.dead[tid] = dead;
        if (lex_requires(role)) {
            atomicAdd(&sh.n_req, 1);
            if (dead) sh.req_empty = 1;
        } else if (role == SQE_LEX_SHOULD) {
            atomicAdd(&sh.n_should, 1);
            if (!dead) sh.should_runs = 1;
        } else if (!dead) {
            sh.deny_runs = 1;
        }
    }
    __syncthreads();
    const int n_req = sh.n_req, n_should = sh.n_should;
    const int m = n_req ? a.min_should[q] : max(1, a.min_should[q]);
    if (n_req + n_should == 0 || m > n_should || sh.req_empty || (m >= 1 && !sh.should_runs)) return 0;
    const int64_t row0 = (int64_t)chunk * LEX_CHUNK;
    const int nrows = (int)min((int64_t)LEX_CHUNK, a.rows - row0);
    const uint2* post = a.post + a.fwd_off[row0];
    const auto one = [&](int c) { return sh.first[c + 1] - sh.first[c] == 1; };
    const auto zero_cur = [&]() {
        for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) cur[w] = 0;
        __syncthreads();
    };
    const bool early = LEX_PHRASE_EARLY && acc != nullptr && m < 2;
    // cur |= the rows of cand in which phrase c occurs; a scoring phrase also scores there when the accumulators are free
    const auto phrase_to_cur = [&](int c) {
        const bool add = early && lex_scores(sh.role[c]);
        if (add) {                                     // (every thread has passed a barrier since sh.acc_ready was last written)
            if (!sh.acc_ready) {
                for (int i = tid; i < LEX_CHUNK; i += LEX_THREADS) acc[i] = 0;
                __syncthreads();
                if (tid == 0) sh.acc_ready = 1;
            }
            if (tid == 0) sh.scored[c] = 1;
        }
        lex_phrase_verify(a, sh, c, row0, cand, [&](int r, int pf) {
            if ((tid & 63) != 0) return;
            atomicOr(&cur[r >> 5], 1u << (r & 31));
            if (add) lex_phrase_add(a, sh, c, row0, r, pf, acc);
        });
    };
    for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) {
        const int lo = w * 32;
        alive[w] = nrows >= lo + 32 ? 0xFFFFFFFFu : nrows > lo ? (1u << (nrows - lo)) - 1u : 0u;
    }
    for (int c = 0; c < nc; ++c) {                   // the required terms first: they cost a run each
        if (!lex_requires(sh.role[c]) || !one(c)) continue;
        zero_cur();
        lex_or_run(post, sh.beg[sh.first[c]], sh.end[sh.first[c]], cur);
        __syncthreads();
        for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) alive[w] &= cur[w];
    }
    for (int c = 0; c < nc; ++c) {                   // then the required phrases, over the rows still alive
        if (!lex_requires(sh.role[c]) || one(c)) continue;
        if (lex_phrase_cand(sh, c, post, alive, cand, tmp) == 0) return 0;
        zero_cur();
        phrase_to_cur(c);
        for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) alive[w] &= cur[w];
    }
    if (m == 1 && n_req == 0 && lazy_should) {
        need_pos = true;
    } else if (m == 1) {
        zero_cur();
        for (int c = 0; c < nc; ++c)
            if (sh.role[c] == SQE_LEX_SHOULD && one(c)) lex_or_run(post, sh.beg[sh.first[c]], sh.end[sh.first[c]], cur);
        for (int c = 0; c < nc; ++c) {
            if (sh.role[c] != SQE_LEX_SHOULD || one(c) || sh.dead[c]) continue;
            if (lex_phrase_cand(sh, c, post, alive, cand, tmp)) phrase_to_cur(c);
        }
        __syncthreads();
        for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) alive[w] &= cur[w];
    } else if (m >= 2) {
        for (int i = tid; i < LEX_CHUNK / 4; i += LEX_THREADS) cnt[i] = 0;
        __syncthreads();
        for (int c = 0; c < nc; ++c) {               // a repeated clause counts each time
            if (sh.role[c] != SQE_LEX_SHOULD || sh.dead[c]) continue;
            if (one(c)) {
                const uint32_t e = sh.end[sh.first[c]];
                for (uint32_t p = sh.beg[sh.first[c]] + tid; p < e; p += LEX_THREADS) {
                    const uint32_t r = post[p].x & (LEX_CHUNK - 1);
                    atomicAdd(&cnt[r >> 2], 1u << (8 * (r & 3)));
                }
            } else if (lex_phrase_cand(sh, c, post, alive, cand, tmp)) {
                lex_phrase_verify(a, sh, c, row0, cand, [&](int r, int) {
                    if ((tid & 63) == 0) atomicAdd(&cnt[r >> 2], 1u << (8 * (r & 3)));
                });
            }
        }
        __syncthreads();
        for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) {
            uint32_t enough = 0;
            for (int i = 0; i < 8; ++i) {
                const uint32_t v = cnt[w * 8 + i];
                for (int b = 0; b < 4; ++b) enough |= (uint32_t)((int)((v >> (8 * b)) & 255u) >= m) << (i * 4 + b);
            }
            alive[w] &= enough;
        }
    }
    if (sh.deny_runs) {
        zero_cur();
        for (int c = 0; c < nc; ++c)
            if (sh.role[c] == SQE_LEX_MUST_NOT && one(c)) lex_or_run(post, sh.beg[sh.first[c]], sh.end[sh.first[c]], cur);
        for (int c = 0; c < nc; ++c) {
            if (sh.role[c] != SQE_LEX_MUST_NOT || one(c) || sh.dead[c]) continue;
            if (lex_phrase_cand(sh, c, post, alive, cand, tmp)) phrase_to_cur(c);
        }
        __syncthreads();
        for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) alive[w] &= ~cur[w];
    }
    int live = 0;
    for (int w = tid; w < LEX_WORDS; w += LEX_THREADS) live += __popc(alive[w]);
    if (live) atomicAdd(&sh.live, live);
    __syncthreads();                               // also: alive is complete for every thread, cnt is free again
    return sh.live;
}

__global__ __launch_bounds__(LEX_THREADS) void lex_phrase_score_kernel(LexPhraseArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) uint32_t lex_phrase_lds[];    // [LEX_CHUNK] accumulators | alive | cur | cand | tmp
    __shared__ LexPhraseShared sh;
    __shared__ int hist[256];
    __shared__ int s_n;
    uint32_t* acc = lex_phrase_lds;
    uint32_t* alive = lex_phrase_lds + LEX_CHUNK;
    uint32_t* cur = alive + LEX_WORDS;
    uint32_t* cand = cur + LEX_WORDS;
    uint32_t* tmp = cand + LEX_WORDS;
    const int chunk = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    uint64_t* out = a.partial + ((size_t)q * a.chunks + chunk) * a.k;
    if (tid == 0) s_n = 0;
    bool need_pos;
    if (lex_phrase_alive(a, chunk, q, sh, alive, cur, cand, tmp, acc, acc, true, need_pos) == 0) return lex_no_hits(out, a.k);
    if (!sh.acc_ready) {                               // no phrase has scored yet
        for (int i = tid; i < LEX_CHUNK; i += LEX_THREADS) acc[i] = 0;
        __syncthreads();
    }
    const int nc = (int)(a.qoff[q + 1] - a.qoff[q]);
    const int64_t row0 = (int64_t)chunk * LEX_CHUNK;
    const uint2* post = a.post + a.fwd_off[row0];
    for (int c = 0; c < nc; ++c) {
        if (!lex_scores(sh.role[c]) || sh.dead[c] || sh.scored[c]) continue;
        const int o = sh.first[c];
        if (sh.first[c + 1] - o == 1) {                // a term: its stored impacts
            lex_add_run(post, sh.beg[o], sh.end[o], acc);
        } else if (lex_phrase_cand(sh, c, post, alive, cand, tmp)) {
            lex_phrase_verify(a, sh, c, row0, cand, [&](int r, int pf) {
                if ((tid & 63) == 0) lex_phrase_add(a, sh, c, row0, r, pf, acc);
            });
        }
    }
    __syncthreads();
    const auto key_of = [&](int i) {
        const uint32_t sc = acc[i];
        const bool hit = ((alive[i >> 5] >> (i & 31)) & 1u) && (sc || !need_pos);
        return hit ? ((uint64_t)(sc + 1u) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)(row0 + i)) : (uint64_t)0;
    };
    const uint64_t T = block_select_kth<LEX_THREADS, uint64_t, true>(each_key<LEX_THREADS>(key_of, LEX_CHUNK), a.k, hist);
    lex_chunk_topk(key_of, T, a.k, out, s_n);
}

__global__ __launch_bounds__(LEX_THREADS) void lex_phrase_bits_kernel(LexPhraseArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lex_phrase_match_lds[];      // [LEX_CHUNK / 4] byte counters | alive | cur | cand | tmp
    __shared__ LexPhraseShared sh;
    uint32_t* cnt = lex_phrase_match_lds;
    uint32_t* alive = lex_phrase_match_lds + LEX_CHUNK / 4;
    uint32_t* cur = alive + LEX_WORDS;
    uint32_t* cand = cur + LEX_WORDS;
    uint32_t* tmp = cand + LEX_WORDS;
    const int chunk = blockIdx.x, q = blockIdx.y;
    bool need_pos;
    lex_store_alive(a, chunk, q, lex_phrase_alive(a, chunk, q, sh, alive, cur, cand, tmp, cnt, nullptr, false, need_pos), alive);
}

// ================================================================ host side of the searches and match sets
// The host tables of one call, whatever its kind.  A plain query has offsets and terms; a boolean one (with_roles) a role per
// occurrence and a min_should per query as well (null: zeros); a phrase one also coff, and its qoff ranges over clauses, coff
// over occurrences and roles over clauses.
struct LexQuery {
    const int64_t* qoff;           // [B + 1]
    const int64_t* coff;           // [qoff[B] + 1]; null: the queries are lists of occurrences
    const int32_t* terms;
    const uint8_t* roles;          // null for plain queries
    const int32_t* min_should;     // [B] or null
    int B;
    bool with_roles;               // a boolean or phrase call; roles may still be null where there is nothing to give a role to
};

// The tables of a call with B > 0, in the order the kinds have always been checked in: offsets and terms, then roles, then min_should.
int lex_check(const char* who, sqe_lex* L, const LexQuery& Q) {
    if (Q.coff) {
        if (const char* why = lexclause_check(Q.qoff, Q.B, Q.coff, Q.terms, L->n_terms, LEX_MAX_QUERY)) return fail(SQE_ERR_INVALID, std::string(who) + ": " + why);
    } else {
        SQE_TRY(lex_query_check(who, L, Q.qoff, Q.terms, Q.B));
    }
    if (!Q.with_roles) return SQE_OK;
    const int64_t n_roles = Q.qoff[Q.B];
    if (n_roles > 0 && !Q.roles) return fail(SQE_ERR_INVALID, std::string(who) + ": null roles");
    for (int64_t i = 0; i < n_roles; ++i)
        if (Q.roles[i] > SQE_LEX_MUST_NOT) return fail(SQE_ERR_INVALID, std::string(who) + ": a role must be one of SQE_LEX_SHOULD .. SQE_LEX_MUST_NOT");
    if (Q.min_should)
        for (int b = 0; b < Q.B; ++b)
            if (Q.min_should[b] < 0 || Q.min_should[b] > LEX_MAX_QUERY) return fail(SQE_ERR_INVALID, std::string(who) + ": min_should must be in [0, 64]");
    return SQE_OK;
}

int lex_topk_args_ok(const char* who, sqe_lex* L, const LexQuery& Q, int k, const void* score, const void* ids) {
    if (!L) return fail(SQE_ERR_INVALID, "null lexical index");
    if (Q.B < 0 || k < 1 || k > MAX_KP) return fail(SQE_ERR_INVALID, std::string(who) + ": need B >= 0 and 1 <= k <= 256");
    if (Q.B == 0) return SQE_OK;
    if (!score || !ids) return fail(SQE_ERR_INVALID, std::string(who) + ": null buffer");
    return lex_check(who, L, Q);
}

int lex_match_args_ok(const char* who, sqe_lex* L, const LexQuery& Q, int64_t cap, const void* count, const void* ids) {
    if (!L) return fail(SQE_ERR_INVALID, "null lexical index");
    if (Q.B < 0 || cap < 0) return fail(SQE_ERR_INVALID, std::string(who) + ": need B >= 0 and cap >= 0");
    if (Q.B == 0) return SQE_OK;
    if (!count || (cap > 0 && !ids)) return fail(SQE_ERR_INVALID, std::string(who) + ": null buffer");
    return lex_check(who, L, Q);
}

// The query tables to the device, one section after the other: offsets | clause offsets | terms | min_should (zeros for null) |
// roles, of which a call has those of its kind (a plain search: offsets | terms).  Fills what every kernel's arguments share: the
// index, the tables, and for phrases the sequences and the BM25 constants.
int lex_upload(sqe_lex* L, const LexQuery& Q, hipStream_t s, LexPhraseArgs& a) {
    const size_t n_roles = (size_t)Q.qoff[Q.B], n = Q.coff ? (size_t)Q.coff[n_roles] : n_roles;
    struct Section { const void* src; size_t bytes, at; };
    Section sec[5] = {{Q.qoff, (size_t)(Q.B + 1) * 8, 0}, {Q.coff, Q.coff ? (n_roles + 1) * 8 : 0, 0}, {Q.terms, n * 4, 0},
                      {Q.min_should, Q.with_roles ? (size_t)Q.B * 4 : 0, 0}, {Q.roles, Q.with_roles ? n_roles : 0, 0}};
    size_t total = 0;
    for (Section& x : sec) {
        x.at = total;
        total += x.bytes;
    }
    L->q_host.resize(total + 4);
    char* h = L->q_host.data();
    for (const Section& x : sec) {
        if (x.bytes && x.src) memcpy(h + x.at, x.src, x.bytes);
        else if (x.bytes) memset(h + x.at, 0, x.bytes);
    }
    SQE_TRY(L->q_tables.ensure(total + 16));
    SQE_HIP(hipMemcpyAsync(L->q_tables.p, h, total, hipMemcpyHostToDevice, s));
    const char* d = L->q_tables.as<char>();
    a.qoff = reinterpret_cast<const int64_t*>(d + sec[0].at); a.coff = reinterpret_cast<const int64_t*>(d + sec[1].at);
    a.qterms = reinterpret_cast<const int32_t*>(d + sec[2].at); a.min_should = reinterpret_cast<const int32_t*>(d + sec[3].at);
    a.qroles = reinterpret_cast<const uint8_t*>(d + sec[4].at);
    a.fwd_off = L->d_fwd_off.as<int64_t>(); a.table = L->d_table.as<uint32_t>(); a.post = L->d_post.as<uint2>(); a.ids = L->d_ids.as<int64_t>();
    a.rows = L->rows; a.n_terms = L->n_terms; a.chunks = L->chunks;
    a.seq_off = L->has_seq ? L->d_seq_off.as<int64_t>() : nullptr; a.seq = L->has_seq ? L->d_seq.as<int32_t>() : nullptr;
    a.dl = L->d_dl.as<int64_t>(); a.idf = L->d_idf.as<double>();
    a.k1 = L->k1; a.bm = L->b; a.avgdl = L->avgdl;
    return SQE_OK;
}

// The k best of each query to the device.  The caller holds the lock of L and has validated the arguments; everything runs on
// stream s.  score_kernel takes the arguments of its kind, LexSearchArgs or a struct derived from it, and lds bytes of dynamic
// LDS; merge_kernel is lex_merge_kernel with the bias of score_kernel's keys.
template <typename Args>
int lex_topk_run(sqe_lex* L, void (*score_kernel)(Args), int lds, void (*merge_kernel)(LexSearchArgs), const LexQuery& Q, int k, float* score_dev,
                 int64_t* id_dev, hipStream_t s) {
    const int B = Q.B;
    if (B <= 0) return SQE_OK;
    if (L->dirty) SQE_TRY(lex_rebuild(L, s));
    if (L->rows == 0) return launch_pad_hits(score_dev, id_dev, nullptr, (int64_t)B * k, s);
    LexPhraseArgs a = {};
    SQE_TRY(lex_upload(L, Q, s, a));
    SQE_TRY(L->partial.ensure((size_t)B * L->chunks * k * 8));
    a.partial = L->partial.as<uint64_t>(); a.k = k;
    SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(score_kernel), lds));
    for (int b0 = 0; b0 < B; b0 += 65535) {        // grid.y limit
        const int nb = std::min(65535, B - b0);
        LexPhraseArgs c = a;
        c.qoff = a.qoff + b0;
        if (Q.with_roles) c.min_should = a.min_should + b0;      // a plain search uploads none and its kernel has no such argument
        c.partial = a.partial + (size_t)b0 * L->chunks * k;
        c.score_out = score_dev + (size_t)b0 * k;
        c.id_out = id_dev + (size_t)b0 * k;
        {
            StageTimer t(L->ctx->prof, s, ST_SCAN);
            hipLaunchKernelGGL(score_kernel, dim3(L->chunks, nb), dim3(LEX_THREADS), lds, s, static_cast<const Args&>(c));
        }
        {
            StageTimer t(L->ctx->prof, s, ST_SELECT);
            hipLaunchKernelGGL(merge_kernel, dim3(nb), dim3(LEX_THREADS), 0, s, static_cast<const LexSearchArgs&>(c));
        }
    }
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

// The match set of each query to the device, in sub-batches whose bit maps fit LEX_MATCH_BITS_BYTES.  As lex_topk_run;
// bits_kernel is lex_match_bits_kernel or lex_phrase_bits_kernel.
template <typename Args>
int lex_match_run(sqe_lex* L, void (*bits_kernel)(Args), int lds, const LexQuery& Q, int64_t cap, int64_t* count_dev, int64_t* id_dev, hipStream_t s) {
    const int B = Q.B;
    if (B <= 0) return SQE_OK;
    if (L->dirty) SQE_TRY(lex_rebuild(L, s));
    LexPhraseArgs a = {};
    SQE_TRY(lex_upload(L, Q, s, a));
    const int chunks = L->rows ? L->chunks : 0;    // an empty index: the scan kernel alone writes zero counts and the padding
    a.chunks = chunks;
    a.cap = cap;
    const size_t map_bytes = (size_t)chunks * LEX_WORDS * 4;
    const int step = (int)std::min<size_t>(65535, std::max<size_t>(1, LEX_MATCH_BITS_BYTES / std::max<size_t>(map_bytes, 1)));      // grid.y limit too
    SQE_TRY(L->match_bits.ensure(std::max<size_t>((size_t)std::min(step, B) * map_bytes, 16)));
    SQE_TRY(L->match_offs.ensure((size_t)std::min(step, B) * (chunks + 1) * 8));
    a.bits = L->match_bits.as<uint32_t>(); a.offs = L->match_offs.as<int64_t>();
    if (chunks) SQE_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(bits_kernel), lds));
    for (int b0 = 0; b0 < B; b0 += step) {
        const int nb = std::min(step, B - b0);
        LexPhraseArgs c = a;
        c.qoff = a.qoff + b0;
        c.min_should = a.min_should + b0;
        c.count_out = count_dev + b0;
        c.match_out = id_dev ? id_dev + (size_t)b0 * cap : nullptr;
        if (chunks) {
            StageTimer t(L->ctx->prof, s, ST_SCAN);
            hipLaunchKernelGGL(bits_kernel, dim3(chunks, nb), dim3(LEX_THREADS), lds, s, static_cast<const Args&>(c));
        }
        {
            StageTimer t(L->ctx->prof, s, ST_SELECT);
            hipLaunchKernelGGL(lex_match_scan_kernel, dim3(nb), dim3(LEX_THREADS), 0, s, static_cast<const LexBoolArgs&>(c));
            if (chunks && cap > 0)
                hipLaunchKernelGGL(lex_match_expand_kernel, dim3(chunks, nb), dim3(LEX_THREADS), 0, s, static_cast<const LexBoolArgs&>(c));
        }
    }
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

// An entry point after its argument check.  The _device form (host_out false) runs on the context stream into the caller's
// device buffers; the host form runs into L->stage, copies the two outputs back and synchronises.
template <typename Args>
int lex_topk(sqe_lex* L, void (*score_kernel)(Args), int lds, void (*merge_kernel)(LexSearchArgs), const LexQuery& Q, int k, float* score_out,
             int64_t* id_out, bool host_out) {
    if (Q.B == 0) return SQE_OK;
    OpScope op(L->ctx, L->ord, host_out);
    if (!host_out) return lex_topk_run(L, score_kernel, lds, merge_kernel, Q, k, score_out, id_out, op.s);
    const size_t cnt = (size_t)Q.B * k, sb = round16(cnt * 4);
    SQE_TRY(L->stage.ensure(sb + cnt * 8));
    float* sc = L->stage.as<float>();
    int64_t* id = reinterpret_cast<int64_t*>(L->stage.as<char>() + sb);
    SQE_TRY(lex_topk_run(L, score_kernel, lds, merge_kernel, Q, k, sc, id, op.s));
    SQE_HIP(hipMemcpyAsync(score_out, sc, cnt * 4, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipMemcpyAsync(id_out, id, cnt * 8, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

template <typename Args>
int lex_match(sqe_lex* L, void (*bits_kernel)(Args), int lds, const LexQuery& Q, int64_t cap, int64_t* count_out, int64_t* id_out, bool host_out) {
    if (Q.B == 0) return SQE_OK;
    OpScope op(L->ctx, L->ord, host_out);
    if (!host_out) return lex_match_run(L, bits_kernel, lds, Q, cap, count_out, cap ? id_out : nullptr, op.s);
    const size_t cb = (size_t)Q.B * 8, ib = (size_t)Q.B * (size_t)cap * 8;
    SQE_TRY(L->stage.ensure(cb + ib));
    int64_t* cnt = L->stage.as<int64_t>();
    int64_t* id = cap ? cnt + Q.B : nullptr;
    SQE_TRY(lex_match_run(L, bits_kernel, lds, Q, cap, cnt, id, op.s));
    SQE_HIP(hipMemcpyAsync(count_out, cnt, cb, hipMemcpyDeviceToHost, op.s));
    if (ib) SQE_HIP(hipMemcpyAsync(id_out, id, ib, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

}  // namespace

int lex_search_on_stream(sqe_lex* L, const int64_t* qoff, const int32_t* qterms, int B, int k, float* score_dev, int64_t* id_dev, hipStream_t s) {
    std::lock_guard<std::mutex> lk(L->ord.mu);
    OpOrder& o = L->ord;
    if (o.armed && o.last != s) (void)hipStreamWaitEvent(s, o.ev, 0);
    const int rc = lex_topk_run(L, lex_score_kernel, LEX_LDS, lex_merge_kernel<0>, LexQuery{qoff, nullptr, qterms, nullptr, nullptr, B, false}, k, score_dev, id_dev, s);
    (void)hipEventRecord(o.ev, s);
    o.last = s;
    o.armed = true;
    return rc;
}

}  // namespace sqe

// ================================================================ C ABI
using namespace sqe;

extern "C" {

int sqe_lex_create(sqe_ctx* ctx, int n_terms, double k1, double b, sqe_lex** out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return fail(SQE_ERR_INVALID, "sqe_lex_create: null argument");
    if (n_terms < 1 || n_terms > LEX_MAX_TERMS) return fail(SQE_ERR_INVALID, "sqe_lex_create: n_terms must be in [1, 131072]");
    if (!(k1 >= 0.0 && k1 <= 3.0)) return fail(SQE_ERR_INVALID, "sqe_lex_create: k1 must be in [0, 3]");      // NaN fails both
    if (!(b >= 0.0 && b <= 1.0)) return fail(SQE_ERR_INVALID, "sqe_lex_create: b must be in [0, 1]");
    sqe_lex* L = new (std::nothrow) sqe_lex;
    if (!L) return fail(SQE_ERR_OOM, "sqe_lex_create: host allocation failed");
    L->ctx = ctx;
    L->n_terms = n_terms;
    L->k1 = k1;
    L->b = b;
    (void)hipSetDevice(ctx->device);
    const int rc = L->ord.init();
    if (rc != SQE_OK) {
        L->ord.destroy();
        delete L;
        return rc;
    }
    *out = L;
    return SQE_OK;
}

void sqe_lex_destroy(sqe_lex* L) {
    if (!L) return;
    (void)hipSetDevice(L->ctx->device);
    L->ord.destroy();
    delete L;
}

}  // extern "C"

namespace sqe {
namespace {

// a document leaves the live set (replaced or deleted); the caller holds the lock
void lex_retire(sqe_lex* L, sqe_lex::Doc& d) {
    d.live = false;
    L->live--;
    L->live_postings -= d.distinct;
    if (d.seq_off >= 0) {
        L->live_ordered--;
        L->live_seq -= d.dl;
    }
}

// sqe_lex_put and sqe_lex_put_ordered: the same checks, the same bag; the ordered form also logs the sequence
int lex_put(const char* who, sqe_lex* L, const int64_t* ids_host, const int64_t* offsets_host, const int32_t* terms_host, int64_t n, bool ordered) {
    if (!L) return fail(SQE_ERR_INVALID, "null lexical index");
    if (n == 0) return SQE_OK;
    if (const char* why = lexbag_check(offsets_host, n, terms_host, L->n_terms, 0)) return fail(SQE_ERR_INVALID, std::string(who) + ": " + why);
    if (const char* why = lexbag_check_ids(ids_host, n)) return fail(SQE_ERR_INVALID, std::string(who) + ": " + why);
    std::lock_guard<std::mutex> lk(L->ord.mu);
    // rows are uint32 and the score bound of the header needs N < 2^31
    if (L->live + n >= (int64_t)1 << 31) return fail(SQE_ERR_INVALID, std::string(who) + ": the index holds fewer than 2^31 documents");
    std::vector<int32_t> t;
    std::vector<uint16_t> tf;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t* terms = terms_host + offsets_host[i];
        const int64_t dl = offsets_host[i + 1] - offsets_host[i];
        int64_t seq_off = -1;
        if (ordered) seq_off = lexseq_append(terms, dl, t, tf, L->log_seq);
        else lexbag_canon(terms, dl, t, tf);
        auto it = L->by_id.find(ids_host[i]);
        if (it != L->by_id.end()) lex_retire(L, L->docs[it->second]);      // a live id: its bag and its sequence are replaced
        L->by_id[ids_host[i]] = L->docs.size();
        L->docs.push_back({ids_host[i], (int64_t)L->log_term.size(), dl, (int32_t)t.size(), true, seq_off});
        if (ordered) {
            L->live_ordered++;
            L->live_seq += dl;
        }
        L->log_term.insert(L->log_term.end(), t.begin(), t.end());
        L->log_tf.insert(L->log_tf.end(), tf.begin(), tf.end());
        L->live++;
        L->live_postings += (int64_t)t.size();
    }
    L->dirty = true;
    return SQE_OK;
}

}  // namespace
}  // namespace sqe

extern "C" {

int sqe_lex_put(sqe_lex* L, const int64_t* ids_host, const int64_t* offsets_host, const int32_t* terms_host, int64_t n) {
    return lex_put("sqe_lex_put", L, ids_host, offsets_host, terms_host, n, false);
}

int sqe_lex_put_ordered(sqe_lex* L, const int64_t* ids_host, const int64_t* offsets_host, const int32_t* terms_host, int64_t n) {
    return lex_put("sqe_lex_put_ordered", L, ids_host, offsets_host, terms_host, n, true);
}

int sqe_lex_delete(sqe_lex* L, const int64_t* ids_host, int64_t n) {
    if (!L) return fail(SQE_ERR_INVALID, "null lexical index");
    if (n < 0 || (n > 0 && !ids_host)) return fail(SQE_ERR_INVALID, "sqe_lex_delete: null ids or negative count");
    std::lock_guard<std::mutex> lk(L->ord.mu);
    for (int64_t i = 0; i < n; ++i) {
        auto it = L->by_id.find(ids_host[i]);
        if (it == L->by_id.end()) continue;      // unknown ids are skipped
        lex_retire(L, L->docs[it->second]);
        L->by_id.erase(it);
        L->dirty = true;
    }
    return SQE_OK;
}

int sqe_lex_count(const sqe_lex* L, int64_t* out) {
    if (!L || !out) return fail(SQE_ERR_INVALID, "sqe_lex_count: null argument");
    std::lock_guard<std::mutex> lk(const_cast<sqe_lex*>(L)->ord.mu);
    *out = L->live;
    return SQE_OK;
}

// The searches and match sets: a LexQuery over the caller's tables, the argument check under the entry point's own name, then
// the runner with the kernel of the query kind.
int sqe_lex_search(sqe_lex* L, const int64_t* qoffsets_host, const int32_t* qterms_host, int B, int k, float* score_out_host,
                   int64_t* id_out_host) {
    const LexQuery Q{qoffsets_host, nullptr, qterms_host, nullptr, nullptr, B, false};
    SQE_TRY(lex_topk_args_ok("sqe_lex_search", L, Q, k, score_out_host, id_out_host));
    return lex_topk(L, lex_score_kernel, LEX_LDS, lex_merge_kernel<0>, Q, k, score_out_host, id_out_host, true);
}

int sqe_lex_search_device(sqe_lex* L, const int64_t* qoffsets_host, const int32_t* qterms_host, int B, int k, float* score_out_dev,
                          int64_t* id_out_dev) {
    const LexQuery Q{qoffsets_host, nullptr, qterms_host, nullptr, nullptr, B, false};
    SQE_TRY(lex_topk_args_ok("sqe_lex_search_device", L, Q, k, score_out_dev, id_out_dev));
    return lex_topk(L, lex_score_kernel, LEX_LDS, lex_merge_kernel<0>, Q, k, score_out_dev, id_out_dev, false);
}

int sqe_lex_search_bool(sqe_lex* L, const int64_t* qoffsets_host, const int32_t* qterms_host, const uint8_t* qroles_host,
                        const int32_t* min_should_host, int B, int k, float* score_out_host, int64_t* id_out_host) {
    const LexQuery Q{qoffsets_host, nullptr, qterms_host, qroles_host, min_should_host, B, true};
    SQE_TRY(lex_topk_args_ok("sqe_lex_search_bool", L, Q, k, score_out_host, id_out_host));
    return lex_topk(L, lex_bool_score_kernel, LEX_BOOL_LDS, lex_merge_kernel<1>, Q, k, score_out_host, id_out_host, true);
}

int sqe_lex_search_bool_device(sqe_lex* L, const int64_t* qoffsets_host, const int32_t* qterms_host, const uint8_t* qroles_host,
                               const int32_t* min_should_host, int B, int k, float* score_out_dev, int64_t* id_out_dev) {
    const LexQuery Q{qoffsets_host, nullptr, qterms_host, qroles_host, min_should_host, B, true};
    SQE_TRY(lex_topk_args_ok("sqe_lex_search_bool_device", L, Q, k, score_out_dev, id_out_dev));
    return lex_topk(L, lex_bool_score_kernel, LEX_BOOL_LDS, lex_merge_kernel<1>, Q, k, score_out_dev, id_out_dev, false);
}

int sqe_lex_match(sqe_lex* L, const int64_t* qoffsets_host, const int32_t* qterms_host, const uint8_t* qroles_host,
                  const int32_t* min_should_host, int B, int64_t cap, int64_t* count_out_host, int64_t* id_out_host) {
    const LexQuery Q{qoffsets_host, nullptr, qterms_host, qroles_host, min_should_host, B, true};
    SQE_TRY(lex_match_args_ok("sqe_lex_match", L, Q, cap, count_out_host, id_out_host));
    return lex_match(L, lex_match_bits_kernel, LEX_MATCH_LDS, Q, cap, count_out_host, id_out_host, true);
}

int sqe_lex_match_device(sqe_lex* L, const int64_t* qoffsets_host, const int32_t* qterms_host, const uint8_t* qroles_host,
                         const int32_t* min_should_host, int B, int64_t cap, int64_t* count_out_dev, int64_t* id_out_dev) {
    const LexQuery Q{qoffsets_host, nullptr, qterms_host, qroles_host, min_should_host, B, true};
    SQE_TRY(lex_match_args_ok("sqe_lex_match_device", L, Q, cap, count_out_dev, id_out_dev));
    return lex_match(L, lex_match_bits_kernel, LEX_MATCH_LDS, Q, cap, count_out_dev, id_out_dev, false);
}

int sqe_lex_search_phrase(sqe_lex* L, const int64_t* qoffsets_host, const int64_t* coffsets_host, const int32_t* qterms_host,
                          const uint8_t* croles_host, const int32_t* min_should_host, int B, int k, float* score_out_host, int64_t* id_out_host) {
    const LexQuery Q{qoffsets_host, coffsets_host, qterms_host, croles_host, min_should_host, B, true};
    SQE_TRY(lex_topk_args_ok("sqe_lex_search_phrase", L, Q, k, score_out_host, id_out_host));
    return lex_topk(L, lex_phrase_score_kernel, LEX_PHRASE_LDS, lex_merge_kernel<1>, Q, k, score_out_host, id_out_host, true);
}

int sqe_lex_search_phrase_device(sqe_lex* L, const int64_t* qoffsets_host, const int64_t* coffsets_host, const int32_t* qterms_host,
                                 const uint8_t* croles_host, const int32_t* min_should_host, int B, int k, float* score_out_dev,
                                 int64_t* id_out_dev) {
    const LexQuery Q{qoffsets_host, coffsets_host, qterms_host, croles_host, min_should_host, B, true};
    SQE_TRY(lex_topk_args_ok("sqe_lex_search_phrase_device", L, Q, k, score_out_dev, id_out_dev));
    return lex_topk(L, lex_phrase_score_kernel, LEX_PHRASE_LDS, lex_merge_kernel<1>, Q, k, score_out_dev, id_out_dev, false);
}

int sqe_lex_match_phrase(sqe_lex* L, const int64_t* qoffsets_host, const int64_t* coffsets_host, const int32_t* qterms_host,
                         const uint8_t* croles_host, const int32_t* min_should_host, int B, int64_t cap, int64_t* count_out_host,
                         int64_t* id_out_host) {
    const LexQuery Q{qoffsets_host, coffsets_host, qterms_host, croles_host, min_should_host, B, true};
    SQE_TRY(lex_match_args_ok("sqe_lex_match_phrase", L, Q, cap, count_out_host, id_out_host));
    return lex_match(L, lex_phrase_bits_kernel, LEX_PHRASE_MATCH_LDS, Q, cap, count_out_host, id_out_host, true);
}

int sqe_lex_match_phrase_device(sqe_lex* L, const int64_t* qoffsets_host, const int64_t* coffsets_host, const int32_t* qterms_host,
                                const uint8_t* croles_host, const int32_t* min_should_host, int B, int64_t cap, int64_t* count_out_dev,
                                int64_t* id_out_dev) {
    const LexQuery Q{qoffsets_host, coffsets_host, qterms_host, croles_host, min_should_host, B, true};
    SQE_TRY(lex_match_args_ok("sqe_lex_match_phrase_device", L, Q, cap, count_out_dev, id_out_dev));
    return lex_match(L, lex_phrase_bits_kernel, LEX_PHRASE_MATCH_LDS, Q, cap, count_out_dev, id_out_dev, false);
}

int sqe_lex_info(sqe_lex* L, sqe_lex_info_t* out) {
    if (!L || !out) return fail(SQE_ERR_INVALID, "sqe_lex_info: null argument");
    std::lock_guard<std::mutex> lk(L->ord.mu);
    out->documents = L->live;
    out->postings = L->postings;
    out->n_terms = L->n_terms;
    out->chunk_rows = LEX_CHUNK;
    out->chunks = L->chunks;
    out->rebuilds = L->rebuilds;
    out->avgdl = L->avgdl;
    out->last_rebuild_ms = L->last_rebuild_ms;
    return SQE_OK;
}

int sqe_lex_state_read(sqe_lex* L, int what, int64_t offset, void* out_host, int64_t bytes) {
    if (!L || !out_host || offset < 0 || bytes < 0) return fail(SQE_ERR_INVALID, "sqe_lex_state_read: bad argument");
    OpScope op(L->ctx, L->ord, true);
    if (L->dirty) return fail(SQE_ERR_STATE, "sqe_lex_state_read: the index was changed since its last search");
    const DevBuf* buf = nullptr;
    int64_t extent = 0;
    switch (what) {
        case SQE_LEX_DF: buf = &L->d_df; extent = (int64_t)L->n_terms * 4; break;
        case SQE_LEX_IDF: buf = &L->d_idf; extent = (int64_t)L->n_terms * 8; break;
        case SQE_LEX_IDS: buf = &L->d_ids; extent = L->rows * 8; break;
        case SQE_LEX_DL: buf = &L->d_dl; extent = L->rows * 8; break;
        case SQE_LEX_TABLE: buf = &L->d_table; extent = (int64_t)L->chunks * (L->n_terms + 1) * 4; break;
        case SQE_LEX_POSTINGS: buf = &L->d_post; extent = L->postings * 8; break;
        case SQE_LEX_SEQ_OFF: buf = &L->d_seq_off; extent = L->has_seq ? (L->rows + 1) * 8 : 0; break;
        case SQE_LEX_SEQ: buf = &L->d_seq; extent = L->has_seq ? L->seq_words * 4 : 0; break;
        default: return fail(SQE_ERR_INVALID, "sqe_lex_state_read: unknown buffer");
    }
    if (L->rows == 0) extent = 0;              // an empty index holds nothing on the device
    if (offset + bytes > extent) return fail(SQE_ERR_INVALID, "sqe_lex_state_read: range past the end of the buffer");
    if (bytes == 0) return SQE_OK;
    SQE_HIP(hipMemcpyAsync(out_host, buf->as<char>() + offset, (size_t)bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

}  // extern "C"
