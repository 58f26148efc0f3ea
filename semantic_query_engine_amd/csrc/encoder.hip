// encoder.hip -- BERT encoder (mxbai-embed-large = BERT-large: 24 x {MHA 16x64, FFN 4096}, post-LN,
// erf-GELU, CLS pooling) behind sqe_encode*: stands where Ollama's /api/embeddings stood for
// ollama_embed_text (main.py:134-145).  bf16 weights and activations, fp32 MFMA accumulation,
// fp32 softmax / LayerNorm / residual sums.
//
// This file is the host side: the sqe_encoder object, tensor loading, the workspace, the hipGraph cache, the forward
// pass as a sequence of launches, and the sqe_* entry points.  It holds no device code; the kernels (gfx950, wave64)
// are reached through encoder_kernels.h alone:
//   enc_rows.hip        E1 embedding + LayerNorm, LayerNorm, E7 pooling LayerNorm, pooler and classifier
//   enc_gemm.hip        E2/E4/E5/E6 Y = X W^T + b: few-token, ring, persistent and one-tile kernels, the routing rule
//   enc_gemm_pp.hip     the large-batch ping-pong GEMM
//   enc_attention.hip   E3 flash-style attention
//   enc_device.h        what the kernel files share: tile staging, GELU forms, the common GEMM epilogue
//
// Token layout: padded [B, S] (row = b * S + s); keys at positions >= lens[b] are masked, padded
// query rows compute values nobody reads.  Activation buffers are padded to a multiple of the
// GEMM token tile.
#include <string.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include <stdlib.h>

#include "internal.h"
#include "encoder_kernels.h"

using namespace sqe;

namespace {

struct DevMem {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevMem() { if (p) (void)hipFree(p); }
    int alloc(size_t n) {
        if (n <= bytes) return SQE_OK;
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) return fail(SQE_ERR_OOM, std::string("encoder hipMalloc: ") + hipGetErrorString(e));
        bytes = n;
        return SQE_OK;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

bf16_t host_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((u >> 16) | 0x0040u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}

}  // namespace

struct sqe_layer {
    DevMem w_qkv, b_qkv, w_o, b_o, ln1_g, ln1_b, w_1, b_1, w_2, b_2, ln2_g, ln2_b;
};

struct sqe_encoder {
    sqe_ctx* ctx = nullptr;
    OpOrder ord;                     // own mutex + stream (internal.h): the encoder never blocks an index or the cache
    sqe_bert_cfg cfg;
    DevMem word, pos, type, emb_g, emb_b;
    DevMem pool_w, pool_b, cls_w, cls_b;   // classification head, fp32 (sqe_encode_pairs); labels == 0: none loaded
    int labels = 0, bias_labels = 0;
    std::vector<std::unique_ptr<sqe_layer>> layers;
    std::map<std::string, bool> loaded;
    bool finalized = false;
    // workspace
    DevMem x, x1, qkv, att, hbuf, pre, ids, lens, out;
    DevMem types, cls, pooled, logits;     // scoring: type ids and logits of the host form, CLS rows and pooler output [b_cap, H]
    int t_cap = 0, b_cap = 0;
    // Launch-bound regime (a query batch is ~170 short kernels): the forward pass of a given
    // (B, S, buffers) is captured once into a hipGraph and replayed.  A key is captured the second
    // time it is seen, so callers that pass fresh buffers every time just run eagerly.
    struct GraphEntry {
        int B = 0, S = 0;
        const void* ids = nullptr; const void* lens = nullptr; void* out = nullptr;
        const void* types = nullptr; bool head = false;   // a scoring call never replays an embedding call's graph
        int seen = 0;
        uint64_t last_use = 0;
        hipGraphExec_t exec = nullptr;
        sqe_encoder_state_t plan{};  // what the recorded launches are: a replay reports its own plan
    };
    std::vector<GraphEntry> graphs;
    uint64_t graph_clock = 0;
    bool use_graphs = true;
    // what the call that just returned ran (sqe_encoder_state; T == 0: no encode yet) and whether `out` holds its result
    sqe_encoder_state_t plan{};
    bool out_own = false;
    bool scored = false, logits_own = false;   // the last call ran the head / left its logits in `logits`
    void drop_graphs(bool head_only = false) {
        for (size_t i = graphs.size(); i-- > 0;)
            if (!head_only || graphs[i].head) {
                if (graphs[i].exec) (void)hipGraphExecDestroy(graphs[i].exec);
                graphs.erase(graphs.begin() + i);
            }
    }
    ~sqe_encoder() { drop_graphs(); }
};

namespace {

int upload(DevMem& dst, const float* src, size_t n, bool as_bf16, size_t offset_elems, size_t total_elems, hipStream_t st) {
    SQE_TRY(dst.alloc(total_elems * (as_bf16 ? 2 : 4)));
    if (as_bf16) {
        std::vector<bf16_t> tmp(n);
        for (size_t i = 0; i < n; ++i) tmp[i] = host_bf16(src[i]);
        SQE_HIP(hipMemcpyAsync(dst.as<bf16_t>() + offset_elems, tmp.data(), n * 2, hipMemcpyHostToDevice, st));
        SQE_HIP(hipStreamSynchronize(st));
    } else {
        SQE_HIP(hipMemcpyAsync(dst.as<float>() + offset_elems, src, n * 4, hipMemcpyHostToDevice, st));
        SQE_HIP(hipStreamSynchronize(st));
    }
    return SQE_OK;
}

}  // namespace

extern "C" {

int sqe_encoder_create(sqe_ctx* ctx, const sqe_bert_cfg* cfg, sqe_encoder** out) {
    if (!ctx || !cfg || !out) return fail(SQE_ERR_INVALID, "sqe_encoder_create: null argument");
    *out = nullptr;
    if (cfg->hidden % 128 != 0 || cfg->inter % 128 != 0 || cfg->heads <= 0 || cfg->hidden / cfg->heads != 64 ||
        cfg->layers <= 0 || cfg->max_pos <= 0 || cfg->vocab_size <= 0)
        return fail(SQE_ERR_INVALID, "sqe_encoder_create: need hidden % 128 == 0, inter % 128 == 0, head_dim == 64");
    std::unique_ptr<sqe_encoder> e(new (std::nothrow) sqe_encoder);
    if (!e) return fail(SQE_ERR_OOM, "sqe_encoder_create: host allocation failed");
    e->ctx = ctx;
    e->cfg = *cfg;
    SQE_HIP(hipSetDevice(ctx->device));
    SQE_TRY(e->ord.init());
    for (int l = 0; l < cfg->layers; ++l) e->layers.emplace_back(new sqe_layer);
    {
        const char* g = knob_env("SQE_ENC_GRAPH");          // SQE_ENC_GRAPH=0: always launch kernel by kernel
        e->use_graphs = !(g && g[0] == '0');
    }
    *out = e.release();
    return SQE_OK;
}

void sqe_encoder_destroy(sqe_encoder* enc) {
    if (!enc) return;
    (void)hipSetDevice(enc->ctx->device);
    {
        std::lock_guard<std::mutex> lk(enc->ord.mu);
        enc->ord.quiesce();
    }
    enc->ord.destroy();
    delete enc;
}

int sqe_encoder_load_tensor(sqe_encoder* enc, const char* name, const float* data_host, const int64_t* shape, int ndim) {
    if (!enc || !name || !data_host || !shape || ndim < 1 || ndim > 2) return fail(SQE_ERR_INVALID, "sqe_encoder_load_tensor: bad arguments");
    OpScope op(enc->ctx, enc->ord, true);
    hipStream_t st = op.s;
    const sqe_bert_cfg& c = enc->cfg;
    const size_t H = c.hidden, I = c.inter;
    const std::string n(name);
    size_t count = 1;
    for (int i = 0; i < ndim; ++i) count *= (size_t)shape[i];
    auto expect = [&](size_t want) -> int {
        if (count != want) return fail(SQE_ERR_INVALID, "sqe_encoder_load_tensor: wrong size for " + n);
        return SQE_OK;
    };
    int rc = SQE_OK;
    if (n == "embeddings.word_embeddings.weight") { SQE_TRY(expect((size_t)c.vocab_size * H)); rc = upload(enc->word, data_host, count, true, 0, count, st); }
    else if (n == "embeddings.position_embeddings.weight") { SQE_TRY(expect((size_t)c.max_pos * H)); rc = upload(enc->pos, data_host, count, true, 0, count, st); }
    else if (n == "embeddings.token_type_embeddings.weight") { SQE_TRY(expect((size_t)c.type_vocab * H)); rc = upload(enc->type, data_host, count, true, 0, count, st); }
    else if (n == "embeddings.LayerNorm.weight") { SQE_TRY(expect(H)); rc = upload(enc->emb_g, data_host, count, false, 0, count, st); }
    else if (n == "embeddings.LayerNorm.bias") { SQE_TRY(expect(H)); rc = upload(enc->emb_b, data_host, count, false, 0, count, st); }
    else if (n == "pooler.dense.weight") { SQE_TRY(expect(H * H)); rc = upload(enc->pool_w, data_host, count, false, 0, count, st); }
    else if (n == "pooler.dense.bias") { SQE_TRY(expect(H)); rc = upload(enc->pool_b, data_host, count, false, 0, count, st); }
    else if (n == "classifier.weight") {
        if (ndim != 2 || shape[1] != (int64_t)H || shape[0] < 1 || shape[0] > 8)
            return fail(SQE_ERR_INVALID, "sqe_encoder_load_tensor: classifier.weight must be [labels, hidden] with 1 <= labels <= 8");
        enc->drop_graphs();                               // a recorded head launch carries the label count
        rc = upload(enc->cls_w, data_host, count, false, 0, count, st);
        if (rc == SQE_OK) enc->labels = (int)shape[0];
    }
    else if (n == "classifier.bias") {
        if (count < 1 || count > 8) return fail(SQE_ERR_INVALID, "sqe_encoder_load_tensor: classifier.bias must hold 1 .. 8 labels");
        rc = upload(enc->cls_b, data_host, count, false, 0, count, st);
        if (rc == SQE_OK) enc->bias_labels = (int)count;
    }
    else if (n.rfind("encoder.layer.", 0) == 0) {
        const size_t dot = n.find('.', 14);
        if (dot == std::string::npos) return fail(SQE_ERR_INVALID, "unknown tensor " + n);
        const int l = atoi(n.substr(14, dot - 14).c_str());
        if (l < 0 || l >= c.layers) return fail(SQE_ERR_INVALID, "layer index out of range in " + n);
        sqe_layer& L = *enc->layers[l];
        const std::string s = n.substr(dot + 1);
        if (s == "attention.self.query.weight") { SQE_TRY(expect(H * H)); rc = upload(L.w_qkv, data_host, count, true, 0, 3 * H * H, st); }
        else if (s == "attention.self.key.weight") { SQE_TRY(expect(H * H)); rc = upload(L.w_qkv, data_host, count, true, H * H, 3 * H * H, st); }
        else if (s == "attention.self.value.weight") { SQE_TRY(expect(H * H)); rc = upload(L.w_qkv, data_host, count, true, 2 * H * H, 3 * H * H, st); }
        else if (s == "attention.self.query.bias") { SQE_TRY(expect(H)); rc = upload(L.b_qkv, data_host, count, false, 0, 3 * H, st); }
        else if (s == "attention.self.key.bias") { SQE_TRY(expect(H)); rc = upload(L.b_qkv, data_host, count, false, H, 3 * H, st); }
        else if (s == "attention.self.value.bias") { SQE_TRY(expect(H)); rc = upload(L.b_qkv, data_host, count, false, 2 * H, 3 * H, st); }
        else if (s == "attention.output.dense.weight") { SQE_TRY(expect(H * H)); rc = upload(L.w_o, data_host, count, true, 0, count, st); }
        else if (s == "attention.output.dense.bias") { SQE_TRY(expect(H)); rc = upload(L.b_o, data_host, count, false, 0, count, st); }
        else if (s == "attention.output.LayerNorm.weight") { SQE_TRY(expect(H)); rc = upload(L.ln1_g, data_host, count, false, 0, count, st); }
        else if (s == "attention.output.LayerNorm.bias") { SQE_TRY(expect(H)); rc = upload(L.ln1_b, data_host, count, false, 0, count, st); }
        else if (s == "intermediate.dense.weight") { SQE_TRY(expect(I * H)); rc = upload(L.w_1, data_host, count, true, 0, count, st); }
        else if (s == "intermediate.dense.bias") { SQE_TRY(expect(I)); rc = upload(L.b_1, data_host, count, false, 0, count, st); }
        else if (s == "output.dense.weight") { SQE_TRY(expect(H * I)); rc = upload(L.w_2, data_host, count, true, 0, count, st); }
        else if (s == "output.dense.bias") { SQE_TRY(expect(H)); rc = upload(L.b_2, data_host, count, false, 0, count, st); }
        else if (s == "output.LayerNorm.weight") { SQE_TRY(expect(H)); rc = upload(L.ln2_g, data_host, count, false, 0, count, st); }
        else if (s == "output.LayerNorm.bias") { SQE_TRY(expect(H)); rc = upload(L.ln2_b, data_host, count, false, 0, count, st); }
        else return fail(SQE_ERR_INVALID, "unknown tensor " + n);
    } else {
        return fail(SQE_ERR_INVALID, "unknown tensor " + n);
    }
    if (rc == SQE_OK) { enc->loaded[n] = true; enc->finalized = false; }
    return rc;
}

int sqe_encoder_finalize(sqe_encoder* enc) {
    if (!enc) return fail(SQE_ERR_INVALID, "null encoder");
    std::lock_guard<std::mutex> lk(enc->ord.mu);
    const size_t want = 5 + (size_t)enc->cfg.layers * 16;
    size_t head = 0;
    for (const char* n : {"pooler.dense.weight", "pooler.dense.bias", "classifier.weight", "classifier.bias"}) head += enc->loaded.count(n);
    if (enc->loaded.size() - head != want)
        return fail(SQE_ERR_STATE, "sqe_encoder_finalize: " + std::to_string(enc->loaded.size() - head) + " of " + std::to_string(want) + " tensors loaded");
    if (head != 0 && head != 4)
        return fail(SQE_ERR_STATE, "sqe_encoder_finalize: " + std::to_string(head) + " of the 4 head tensors loaded (pooler.dense.*, classifier.*)");
    if (head == 4 && enc->bias_labels != enc->labels)
        return fail(SQE_ERR_STATE, "sqe_encoder_finalize: classifier.bias does not match the labels of classifier.weight");
    enc->finalized = true;
    return SQE_OK;
}

// what a scoring call adds to the forward pass: per-token type rows in the embedding and the head after the pooling
// LayerNorm, whose CLS rows then go to enc->cls instead of the caller (logits == nullptr: an embedding call)
struct HeadCall { const int32_t* types = nullptr; float* logits = nullptr; };

static int encode_enqueue(sqe_encoder* enc, const int32_t* ids_dev, const int32_t* lens_dev, int B, int S, float* out_dev,
                          int t_pad, hipStream_t st, const HeadCall& hc);

// forward pass on stream st (caller holds the encoder's lock); a scoring call passes out_dev = the logits
static int encode_impl(sqe_encoder* enc, const int32_t* ids_dev, const int32_t* lens_dev, int B, int S, float* out_dev, hipStream_t st,
                       const int32_t* types_dev = nullptr, bool head = false) {
    if (!enc->finalized) return fail(SQE_ERR_STATE, "sqe_encode: encoder weights not finalized");
    if (head && enc->labels == 0) return fail(SQE_ERR_STATE, "sqe_encode_pairs: this encoder has no classification head");
    if (S > enc->cfg.max_pos) return fail(SQE_ERR_INVALID, "sqe_encode: need 1 <= S <= max_pos");
    StageTimer timer(enc->ctx->prof, st, ST_ENCODE);
    const sqe_bert_cfg& c = enc->cfg;
    const int H = c.hidden, I = c.inter;
    const int T = B * S;
    const int t_pad = (T + 255) / 256 * 256;
    enc->scored = false;                                  // set once the call is enqueued: a failed call leaves nothing to read
    enc->logits_own = false;
    if (head && B > enc->b_cap) {
        enc->drop_graphs(true);                           // recorded head launches point into the old cls / pooled rows
        enc->b_cap = 0;                                   // a failed alloc frees its buffer: neither holds rows until both do
        SQE_TRY(enc->cls.alloc((size_t)B * H * 4));
        SQE_TRY(enc->pooled.alloc((size_t)B * H * 4));
        enc->b_cap = B;
    }
    HeadCall hc;
    if (head) { hc.types = types_dev; hc.logits = out_dev; out_dev = enc->cls.as<float>(); enc->out_own = false; }
    // +64 rows: the attention kernel stages whole 64-key tiles, which may run past the last sequence
    if (t_pad > enc->t_cap) {
        enc->drop_graphs();                               // recorded launches point into the old workspace
        SQE_TRY(enc->x.alloc((size_t)(t_pad + 64) * H * 2));
        SQE_TRY(enc->x1.alloc((size_t)(t_pad + 64) * H * 2));
        SQE_TRY(enc->att.alloc((size_t)(t_pad + 64) * H * 2));
        SQE_TRY(enc->qkv.alloc((size_t)(t_pad + 64) * 3 * H * 2));
        SQE_TRY(enc->hbuf.alloc((size_t)(t_pad + 64) * I * 2));
        SQE_TRY(enc->pre.alloc((size_t)t_pad * H * 4 * 4));     // up to 4 split-K partial sums
        SQE_HIP(hipMemsetAsync(enc->x.p, 0, (size_t)(t_pad + 64) * H * 2, st));
        SQE_HIP(hipMemsetAsync(enc->x1.p, 0, (size_t)(t_pad + 64) * H * 2, st));
        SQE_HIP(hipMemsetAsync(enc->att.p, 0, (size_t)(t_pad + 64) * H * 2, st));
        SQE_HIP(hipMemsetAsync(enc->qkv.p, 0, (size_t)(t_pad + 64) * 3 * H * 2, st));
        SQE_HIP(hipMemsetAsync(enc->hbuf.p, 0, (size_t)(t_pad + 64) * I * 2, st));
        enc->t_cap = t_pad;
    }
    // ---- replay / capture (small batches only: above ~8k tokens the kernels are long enough)
    constexpr int GRAPH_MAX_TOKENS = 8192;
    constexpr size_t GRAPH_CACHE = 8;
    sqe_encoder::GraphEntry* ge = nullptr;
    if (enc->use_graphs && t_pad <= GRAPH_MAX_TOKENS) {
        for (auto& e : enc->graphs)
            if (e.B == B && e.S == S && e.ids == ids_dev && e.lens == lens_dev && e.out == (head ? hc.logits : out_dev) &&
                e.types == types_dev && e.head == head) ge = &e;   // replays on any stream
        if (!ge) {
            if (enc->graphs.size() >= GRAPH_CACHE) {              // evict the least recently used entry
                size_t victim = 0;
                for (size_t i = 1; i < enc->graphs.size(); ++i)
                    if (enc->graphs[i].last_use < enc->graphs[victim].last_use) victim = i;
                if (enc->graphs[victim].exec) (void)hipGraphExecDestroy(enc->graphs[victim].exec);
                enc->graphs.erase(enc->graphs.begin() + victim);
            }
            sqe_encoder::GraphEntry fresh;
            fresh.B = B; fresh.S = S; fresh.ids = ids_dev; fresh.lens = lens_dev; fresh.out = head ? hc.logits : out_dev;
            fresh.types = types_dev; fresh.head = head;
            enc->graphs.push_back(fresh);
            ge = &enc->graphs.back();
        }
        ge->last_use = ++enc->graph_clock;
        ++ge->seen;
        if (ge->exec) {
            SQE_HIP(hipGraphLaunch(ge->exec, st));
            enc->plan = ge->plan;
            enc->plan.mode = SQE_ENC_REPLAYED;
            enc->scored = head;
            return SQE_OK;
        }
    }
    const bool capture = ge && ge->seen >= 2;
    if (capture) SQE_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    enc->plan = sqe_encoder_state_t{};
    int rc = encode_enqueue(enc, ids_dev, lens_dev, B, S, out_dev, t_pad, st, hc);
    if (rc != SQE_OK) enc->plan.T = 0;
    if (capture) {
        hipGraph_t graph = nullptr;
        hipError_t e = hipStreamEndCapture(st, &graph);
        if (rc != SQE_OK) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc;
        }
        if (e != hipSuccess || !graph) return fail(SQE_ERR_HIP, std::string("encoder graph capture: ") + hipGetErrorString(e));
        e = hipGraphInstantiate(&ge->exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { ge->exec = nullptr; return fail(SQE_ERR_HIP, std::string("encoder graph instantiate: ") + hipGetErrorString(e)); }
        SQE_HIP(hipGraphLaunch(ge->exec, st));
        enc->plan.mode = SQE_ENC_CAPTURED;
        ge->plan = enc->plan;
    }
    if (rc == SQE_OK) enc->scored = head;
    return rc;
}

// the forward pass as a sequence of launches on `st` (run directly, or recorded by a stream capture)
static int encode_enqueue(sqe_encoder* enc, const int32_t* ids_dev, const int32_t* lens_dev, int B, int S, float* out_dev,
                          int t_pad, hipStream_t st, const HeadCall& hc) {
    const sqe_bert_cfg& c = enc->cfg;
    const int H = c.hidden, I = c.inter;
    const int T = B * S;
    const int cus = enc->ctx->cu_count;
    const size_t pstride = (size_t)t_pad * H;             // floats between split-K partial sums in `pre`
    sqe_encoder_state_t& plan = enc->plan;
    plan.B = B; plan.S = S; plan.T = T; plan.t_pad = t_pad; plan.mode = SQE_ENC_EAGER;
    SQE_TRY(launch_embed_ln(ids_dev, hc.types, enc->word.as<bf16_t>(), enc->pos.as<bf16_t>(), enc->type.as<bf16_t>(),
                            enc->emb_g.as<float>(), enc->emb_b.as<float>(), enc->pre.as<float>(), enc->x.as<bf16_t>(), T, S, H,
                            c.vocab_size, c.type_vocab, c.ln_eps, st));
    for (int l = 0; l < c.layers; ++l) {
        sqe_layer& L = *enc->layers[l];
        GemmArgs a;
        a.T = T; a.resid = nullptr; a.n_tiles = 0;
        // E2: QKV projection
        a.W = L.w_qkv.as<bf16_t>(); a.X = enc->x.as<bf16_t>(); a.bias = L.b_qkv.as<float>(); a.out = enc->qkv.p; a.N = 3 * H; a.K = H;
        SQE_TRY(launch_gemm(EPI_BIAS, a, t_pad, cus, st, 0, nullptr, &plan.gemm[SQE_SITE_QKV]));
        // E3: attention
        SQE_TRY(launch_attention(enc->qkv.as<bf16_t>(), lens_dev, enc->att.as<bf16_t>(), B, S, H, c.heads, &plan.att_nw, &plan.att_nq, st));
        // E4: output projection + residual, LayerNorm
        a.W = L.w_o.as<bf16_t>(); a.X = enc->att.as<bf16_t>(); a.bias = L.b_o.as<float>(); a.resid = enc->x.as<bf16_t>();
        a.out = enc->pre.p; a.N = H; a.K = H;
        int ns = 1;
        SQE_TRY(launch_gemm(EPI_RESID, a, t_pad, cus, st, pstride, &ns, &plan.gemm[SQE_SITE_OUT_PROJ]));
        SQE_TRY(launch_layernorm(enc->pre.as<float>(), L.ln1_g.as<float>(), L.ln1_b.as<float>(), enc->x1.as<bf16_t>(), T, H,
                                 c.ln_eps, ns, pstride, st));
        // E5: FFN up + GELU
        a.W = L.w_1.as<bf16_t>(); a.X = enc->x1.as<bf16_t>(); a.bias = L.b_1.as<float>(); a.resid = nullptr;
        a.out = enc->hbuf.p; a.N = I; a.K = H;
        SQE_TRY(launch_gemm(EPI_GELU, a, t_pad, cus, st, 0, nullptr, &plan.gemm[SQE_SITE_FFN_UP]));
        // E6: FFN down + residual, LayerNorm (the last layer's LayerNorm is done by the pooling kernel in fp32)
        a.W = L.w_2.as<bf16_t>(); a.X = enc->hbuf.as<bf16_t>(); a.bias = L.b_2.as<float>(); a.resid = enc->x1.as<bf16_t>();
        a.out = enc->pre.p; a.N = H; a.K = I;
        SQE_TRY(launch_gemm(EPI_RESID, a, t_pad, cus, st, pstride, &ns, &plan.gemm[SQE_SITE_FFN_DOWN]));
        plan.pre_slices = ns; plan.pre_stride = (int64_t)pstride;
        if (l + 1 < c.layers)
            SQE_TRY(launch_layernorm(enc->pre.as<float>(), L.ln2_g.as<float>(), L.ln2_b.as<float>(), enc->x.as<bf16_t>(), T, H,
                                     c.ln_eps, ns, pstride, st));
        else
            SQE_TRY(launch_pool_ln(enc->pre.as<float>(), L.ln2_g.as<float>(), L.ln2_b.as<float>(), out_dev, B, S, H, c.ln_eps, ns,
                                   pstride, st));
    }
    if (hc.logits) {                                      // out_dev is enc->cls here
        SQE_TRY(launch_pooler(out_dev, enc->pool_w.as<float>(), enc->pool_b.as<float>(), enc->pooled.as<float>(), B, H, st));
        SQE_TRY(launch_classifier(enc->pooled.as<float>(), enc->cls_w.as<float>(), enc->cls_b.as<float>(), hc.logits, B, H,
                                  enc->labels, st));
    }
    return SQE_OK;
}

int sqe_encode_device(sqe_encoder* enc, const int32_t* ids_dev, const int32_t* lens_dev, int B, int S, float* out_dev) {
    if (!enc) return fail(SQE_ERR_INVALID, "null encoder");
    if (B < 0 || S < 1) return fail(SQE_ERR_INVALID, "sqe_encode: need 1 <= S <= max_pos");
    if (B == 0) return SQE_OK;
    if (!ids_dev || !lens_dev || !out_dev) return fail(SQE_ERR_INVALID, "sqe_encode: null buffer");
    OpScope op(enc->ctx, enc->ord, false);
    enc->out_own = false;
    return encode_impl(enc, ids_dev, lens_dev, B, S, out_dev, op.s);
}

int sqe_encode(sqe_encoder* enc, const int32_t* ids_host, const int32_t* lens_host, int B, int S, float* out_host) {
    if (!enc) return fail(SQE_ERR_INVALID, "null encoder");
    if (B < 0 || S < 1) return fail(SQE_ERR_INVALID, "sqe_encode: bad shape");
    if (B == 0) return SQE_OK;
    if (!ids_host || !lens_host || !out_host) return fail(SQE_ERR_INVALID, "sqe_encode: null buffer");
    OpScope op(enc->ctx, enc->ord, true);
    hipStream_t st = op.s;
    SQE_TRY(enc->ids.alloc((size_t)B * S * 4));
    SQE_TRY(enc->lens.alloc((size_t)B * 4));
    SQE_TRY(enc->out.alloc((size_t)B * enc->cfg.hidden * 4));
    SQE_HIP(hipMemcpyAsync(enc->ids.p, ids_host, (size_t)B * S * 4, hipMemcpyHostToDevice, st));
    SQE_HIP(hipMemcpyAsync(enc->lens.p, lens_host, (size_t)B * 4, hipMemcpyHostToDevice, st));
    SQE_TRY(encode_impl(enc, enc->ids.as<int32_t>(), enc->lens.as<int32_t>(), B, S, enc->out.as<float>(), st));
    SQE_HIP(hipMemcpyAsync(out_host, enc->out.p, (size_t)B * enc->cfg.hidden * 4, hipMemcpyDeviceToHost, st));
    SQE_HIP(hipStreamSynchronize(st));
    enc->out_own = true;
    return SQE_OK;
}

int sqe_encoder_labels(sqe_encoder* enc, int* out) {
    if (!enc || !out) return fail(SQE_ERR_INVALID, "sqe_encoder_labels: null argument");
    std::lock_guard<std::mutex> lk(enc->ord.mu);
    *out = enc->finalized && enc->loaded.count("classifier.weight") ? enc->labels : 0;
    return SQE_OK;
}

int sqe_encode_pairs_device(sqe_encoder* enc, const int32_t* ids_dev, const int32_t* types_dev, const int32_t* lens_dev, int B, int S,
                            float* logits_out_dev) {
    if (!enc) return fail(SQE_ERR_INVALID, "null encoder");
    if (B < 0 || S < 1) return fail(SQE_ERR_INVALID, "sqe_encode_pairs: need 1 <= S <= max_pos");
    if (B > 0 && (!ids_dev || !lens_dev || !logits_out_dev)) return fail(SQE_ERR_INVALID, "sqe_encode_pairs: null buffer");
    OpScope op(enc->ctx, enc->ord, false);
    if (enc->labels == 0) return fail(SQE_ERR_STATE, "sqe_encode_pairs: this encoder has no classification head");
    if (B == 0) return SQE_OK;
    return encode_impl(enc, ids_dev, lens_dev, B, S, logits_out_dev, op.s, types_dev, true);
}

int sqe_encode_pairs(sqe_encoder* enc, const int32_t* ids_host, const int32_t* types_host, const int32_t* lens_host, int B, int S,
                     float* logits_out_host) {
    if (!enc) return fail(SQE_ERR_INVALID, "null encoder");
    if (B < 0 || S < 1) return fail(SQE_ERR_INVALID, "sqe_encode_pairs: bad shape");
    if (B > 0 && (!ids_host || !lens_host || !logits_out_host)) return fail(SQE_ERR_INVALID, "sqe_encode_pairs: null buffer");
    OpScope op(enc->ctx, enc->ord, true);
    if (enc->labels == 0) return fail(SQE_ERR_STATE, "sqe_encode_pairs: this encoder has no classification head");
    if (B == 0) return SQE_OK;
    hipStream_t st = op.s;
    const size_t nl = (size_t)B * enc->labels * 4;
    SQE_TRY(enc->ids.alloc((size_t)B * S * 4));
    SQE_TRY(enc->lens.alloc((size_t)B * 4));
    SQE_TRY(enc->logits.alloc(nl));
    SQE_HIP(hipMemcpyAsync(enc->ids.p, ids_host, (size_t)B * S * 4, hipMemcpyHostToDevice, st));
    SQE_HIP(hipMemcpyAsync(enc->lens.p, lens_host, (size_t)B * 4, hipMemcpyHostToDevice, st));
    if (types_host) {
        SQE_TRY(enc->types.alloc((size_t)B * S * 4));
        SQE_HIP(hipMemcpyAsync(enc->types.p, types_host, (size_t)B * S * 4, hipMemcpyHostToDevice, st));
    }
    SQE_TRY(encode_impl(enc, enc->ids.as<int32_t>(), enc->lens.as<int32_t>(), B, S, enc->logits.as<float>(), st,
                        types_host ? enc->types.as<int32_t>() : nullptr, true));
    SQE_HIP(hipMemcpyAsync(logits_out_host, enc->logits.p, nl, hipMemcpyDeviceToHost, st));
    SQE_HIP(hipStreamSynchronize(st));
    enc->logits_own = true;
    return SQE_OK;
}

int sqe_encoder_state(sqe_encoder* enc, sqe_encoder_state_t* out) {
    if (!enc || !out) return fail(SQE_ERR_INVALID, "sqe_encoder_state: null argument");
    OpScope op(enc->ctx, enc->ord, true);
    if (enc->plan.T == 0) return fail(SQE_ERR_STATE, "sqe_encoder_state: this encoder has not encoded anything yet");
    *out = enc->plan;
    return SQE_OK;
}

int sqe_encoder_state_read(sqe_encoder* enc, int what, int64_t offset, void* out_host, int64_t bytes) {
    if (!enc || (!out_host && bytes > 0)) return fail(SQE_ERR_INVALID, "sqe_encoder_state_read: null argument");
    OpScope op(enc->ctx, enc->ord, true);
    const sqe_encoder_state_t& P = enc->plan;
    if (P.T == 0) return fail(SQE_ERR_STATE, "sqe_encoder_state_read: this encoder has not encoded anything yet");
    const int64_t H = enc->cfg.hidden, I = enc->cfg.inter, rows = (int64_t)P.t_pad + 64;
    const DevMem* src = nullptr;
    int64_t size = 0;
    switch (what) {
        case SQE_ENC_X: src = &enc->x; size = rows * H * 2; break;
        case SQE_ENC_X1: src = &enc->x1; size = rows * H * 2; break;
        case SQE_ENC_QKV: src = &enc->qkv; size = rows * 3 * H * 2; break;
        case SQE_ENC_ATT: src = &enc->att; size = rows * H * 2; break;
        case SQE_ENC_HBUF: src = &enc->hbuf; size = rows * I * 2; break;
        case SQE_ENC_PRE: src = &enc->pre; size = P.pre_slices == 0 ? (int64_t)P.t_pad * H * 2 : P.pre_slices * P.pre_stride * 4; break;
        case SQE_ENC_OUT:
            if (!enc->out_own) return fail(SQE_ERR_STATE, "sqe_encoder_state_read: the last encode wrote to the caller's buffer");
            src = &enc->out; size = (int64_t)P.B * H * 4; break;
        case SQE_ENC_CLS: case SQE_ENC_POOLED: case SQE_ENC_LOGITS:
            if (!enc->scored) return fail(SQE_ERR_STATE, "sqe_encoder_state_read: the last call was not a scoring call");
            if (what == SQE_ENC_LOGITS && !enc->logits_own)
                return fail(SQE_ERR_STATE, "sqe_encoder_state_read: the last scoring call wrote its logits to the caller's buffer");
            src = what == SQE_ENC_CLS ? &enc->cls : what == SQE_ENC_POOLED ? &enc->pooled : &enc->logits;
            size = (int64_t)P.B * (what == SQE_ENC_LOGITS ? (int64_t)enc->labels : H) * 4; break;
        default: return fail(SQE_ERR_INVALID, "sqe_encoder_state_read: unknown buffer");
    }
    if (!src->p || (int64_t)src->bytes < size) return fail(SQE_ERR_STATE, "sqe_encoder_state_read: the encoder does not hold that buffer");
    if (offset < 0 || bytes < 0 || offset + bytes > size) return fail(SQE_ERR_INVALID, "sqe_encoder_state_read: range outside the buffer");
    if (bytes == 0) return SQE_OK;
    SQE_HIP(hipMemcpyAsync(out_host, static_cast<const char*>(src->p) + offset, (size_t)bytes, hipMemcpyDeviceToHost, op.s));
    SQE_HIP(hipStreamSynchronize(op.s));
    return SQE_OK;
}

}  // extern "C"
