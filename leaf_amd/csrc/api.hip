// C ABI (include/leaf_hip.h): handle + flat parameter layout + weight packing + encode_text +
// score_candidates.  Host orchestration only -- every device operation is a launch on the caller's stream.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "engine.h"

static thread_local char g_err[512] = "";

void leaf_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
int leaf_check(hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    leaf_set_error("%s: %s", what, hipGetErrorString(e));
    return 1;
}

extern "C" const char* leaf_last_error(void) { return g_err; }
extern "C" int leaf_version(void) { return 2; }

// ------------------------------------------------------------------ options (include/leaf_hip.h leaf_text_set_option)
namespace {
int norm_flag(const leaf_text*, int v) { return v ? 1 : 0; }
int norm_ln_fold(const leaf_text* h, int v) { return (v && h->cfg.width % 64 == 0) ? 1 : 0; }
struct Option {
    const char* name;
    int leaf_text::*member;
    const char* env;                        // environment variable holding the default of a new handle (NAME=0: off), or null
    int (*norm)(const leaf_text*, int);     // stored value of a requested one; null: not set through the table
};
const Option OPTIONS[] = {
    {"chunk", &leaf_text::chunk, nullptr, nullptr},                 // set: leaf_text_set_option itself (range check)
    {"last_layer_trim", &leaf_text::last_trim, "LEAF_LAST_TRIM", norm_flag},
    {"normalize_fare", &leaf_text::normalize_fare, nullptr, norm_flag},
    {"ln_fold", &leaf_text::ln_fold, "LEAF_LN_FOLD", norm_ln_fold},
    {"fuse_attn", &leaf_text::fuse_attn, "LEAF_FUSE_ATTN", norm_flag},
    {"compact_resid", &leaf_text::compact_resid, "LEAF_COMPACT_RESID", norm_flag},
    {"single_edit", &leaf_text::single_edit, nullptr, norm_flag},
    {"split_blocks", &leaf_text::split_blocks, nullptr, nullptr},   // get only: leaf_text_split_pack_masks sets it
};
const Option* find_option(const char* name) {
    for (const Option& o : OPTIONS)
        if (!strcmp(name, o.name)) return &o;
    return nullptr;
}
}  // namespace

extern "C" int leaf_text_create(const leaf_text_cfg* cfg, int fwd_dtype, leaf_text_t* out) {
    if (!cfg || !out) { leaf_set_error("null argument"); return 1; }
    const int d = cfg->width;
    if (cfg->layers < 1 || d < 128 || d % 128 || cfg->heads * 64 != d || cfg->embed_dim < 4 || cfg->embed_dim % 4 ||
        cfg->embed_dim > 2048 || d > 2048 || cfg->context_length < 1 || cfg->context_length > 96 ||
        cfg->vocab_size < 2 || (cfg->activation != 0 && cfg->activation != 1) ||
        (fwd_dtype != LEAF_DTYPE_BF16 && fwd_dtype != LEAF_DTYPE_FP16)) {
        leaf_set_error("unsupported text config (need width %% 128 == 0, head_dim 64, ctx <= 96, embed_dim %% 4 == 0)");
        return 1;
    }
    leaf_text* h = new leaf_text();
    h->cfg = *cfg;
    h->fwd_dtype = fwd_dtype;
    h->chunk = 4096;
    for (const Option& o : OPTIONS)      // on unless the environment says NAME=0
        if (o.env) { const char* e = getenv(o.env); h->*o.member = (e && e[0] == '0') ? 0 : 1; }
    {   // gradient path: fp16 + per-step power-of-two loss scale unless LEAF_GRAD_DTYPE=bf16
        const char* e = getenv("LEAF_GRAD_DTYPE");
        h->grad_dtype = (e && (e[0] == 'b' || e[0] == 'B')) ? LEAF_DTYPE_BF16 : LEAF_DTYPE_FP16;
    }
    const int L = cfg->layers, D = cfg->embed_dim;
    size_t off = 0;
    auto add = [&](const std::string& name, int64_t rows, int64_t cols) {
        TensorInfo t{name, off, rows, cols};
        off += t.numel();
        h->tensors.push_back(t);
        return t.offset;
    };
    h->layer.resize(L);
    // ---- weight-decay group (train_AT_text_only.py:323-331)
    h->tok_emb = add("token_embedding.weight", cfg->vocab_size, d);
    h->pos_emb = add("positional_embedding", cfg->context_length, d);
    h->text_proj = add("text_projection", d, D);
    for (int l = 0; l < L; ++l) {
        std::string p = "transformer.resblocks." + std::to_string(l) + ".";
        h->layer[l].qkv_w = add(p + "attn.in_proj_weight", 3 * d, d);
        h->layer[l].out_w = add(p + "attn.out_proj.weight", d, d);
        h->layer[l].fc_w = add(p + "mlp.c_fc.weight", 4 * d, d);
        h->layer[l].proj_w = add(p + "mlp.c_proj.weight", d, 4 * d);
    }
    h->n_decay = off;
    // ---- no-decay group
    for (int l = 0; l < L; ++l) {
        std::string p = "transformer.resblocks." + std::to_string(l) + ".";
        h->layer[l].ln1_w = add(p + "ln_1.weight", d, 0);
        h->layer[l].ln1_b = add(p + "ln_1.bias", d, 0);
        h->layer[l].qkv_b = add(p + "attn.in_proj_bias", 3 * d, 0);
        h->layer[l].out_b = add(p + "attn.out_proj.bias", d, 0);
        h->layer[l].ln2_w = add(p + "ln_2.weight", d, 0);
        h->layer[l].ln2_b = add(p + "ln_2.bias", d, 0);
        h->layer[l].fc_b = add(p + "mlp.c_fc.bias", 4 * d, 0);
        h->layer[l].proj_b = add(p + "mlp.c_proj.bias", d, 0);
    }
    h->lnf_w = add("ln_final.weight", d, 0);
    h->lnf_b = add("ln_final.bias", d, 0);
    h->n_params = off;
    *out = h;
    return 0;
}

extern "C" void leaf_text_destroy(leaf_text_t h) {
    if (!h) return;
    for (int i = 0; i < leaf_text::PLAN_RING; ++i) {
        if (h->plan_ev[i]) { (void)hipEventSynchronize(h->plan_ev[i]); (void)hipEventDestroy(h->plan_ev[i]); }
        if (h->plan_host[i]) (void)hipHostFree(h->plan_host[i]);
    }
    delete h;
}

extern "C" int leaf_text_set_option(leaf_text_t h, const char* name, int value) {
    if (!h || !name) { leaf_set_error("null argument"); return 1; }
    if (!strcmp(name, "chunk")) {
        if (value < 1) { leaf_set_error("bad chunk"); return 1; }
        h->chunk = value;
        return 0;
    }
    const Option* o = find_option(name);
    if (!o || !o->norm) { leaf_set_error("unknown option '%s'", name); return 1; }
    const int v = o->norm(h, value);
    if (o->member == &leaf_text::ln_fold && !v && h->split_blocks) { leaf_set_error("ln_fold = 0 with split blocks active: the split GEMMs are LN-folded (leaf_text_split_pack_masks(.., 0, ..) first)"); return 1; }
    h->*o->member = v;
    return 0;
}

extern "C" int leaf_text_get_option(leaf_text_t h, const char* name) {
    const Option* o = (h && name) ? find_option(name) : nullptr;
    return o ? h->*o->member : -1;
}

extern "C" size_t leaf_text_param_count(leaf_text_t h) { return h->n_params; }
extern "C" size_t leaf_text_decay_count(leaf_text_t h) { return h->n_decay; }
extern "C" int leaf_text_num_tensors(leaf_text_t h) { return (int)h->tensors.size(); }
extern "C" int leaf_text_param_info(leaf_text_t h, int index, char* name, size_t name_len, size_t* offset,
                                    int64_t* rows, int64_t* cols) {
    if (!h || index < 0 || index >= (int)h->tensors.size()) { leaf_set_error("tensor index out of range"); return 1; }
    const TensorInfo& t = h->tensors[index];
    if (name && name_len) { strncpy(name, t.name.c_str(), name_len - 1); name[name_len - 1] = 0; }
    if (offset) *offset = t.offset;
    if (rows) *rows = t.rows;
    if (cols) *cols = t.cols;
    return 0;
}

extern "C" size_t leaf_text_w16_bytes(leaf_text_t h) { return h->w16_total_bytes(); }

extern "C" size_t leaf_text_split_bytes(leaf_text_t h, int blocks) { return (h && blocks > 0) ? h->split_bytes(blocks) : 0; }

extern "C" int leaf_text_split_pack_masks(leaf_text_t h, const float* params, const int32_t* masks, int blocks, void* buf, leaf_stream_t s_) {
    if (!h) { leaf_set_error("null handle"); return 1; }
    if (blocks == 0) { h->split_blocks = 0; h->split_buf = nullptr; return 0; }
    if (blocks < 0 || blocks > h->cfg.layers - 1 || blocks > 64) { leaf_set_error("split blocks %d out of range 0..%d", blocks, h->cfg.layers - 1); return 1; }
    if (!params || !buf || !masks) { leaf_set_error("leaf_text_split_pack_masks: params / masks / buf is null"); return 1; }
    if (!h->ln_fold) { leaf_set_error("leaf_text_split_pack_masks: the split GEMMs exist in the LN-folded forward only (option ln_fold is 0)"); return 1; }
    for (int l = 0; l < blocks; ++l)
        if (masks[l] < 0 || masks[l] > 15) { leaf_set_error("split mask %d of block %d: bits 0..3 (QKV, out_proj, c_fc, c_proj)", masks[l], l); return 1; }
    hipStream_t s = (hipStream_t)s_;
    const int d = h->cfg.width, dt = h->fwd_dtype;
    h->split_blocks = blocks;
    h->split_buf = buf;
    for (int l = 0; l < 64; ++l) h->split_mask[l] = l < blocks ? masks[l] : 0;
    for (int l = 0; l < blocks; ++l) {      // only what the masks multiply
        const LayerOff& o = h->layer[l];
        if (h->split_qkv(l)) LEAF_TRY(leaf_launch_split_pack(params + o.qkv_w, params + o.ln1_w, (void*)h->split_qkv3(l), (float*)h->split_s_qkv(l), 3 * d, d, 1, dt, s));
        if (h->split_fc(l)) LEAF_TRY(leaf_launch_split_pack(params + o.fc_w, params + o.ln2_w, (void*)h->split_fc3(l), (float*)h->split_s_fc(l), 4 * d, d, 1, dt, s));
        if (h->split_out(l)) LEAF_TRY(leaf_launch_split_pack(params + o.out_w, nullptr, (void*)h->split_out2(l), nullptr, d, d, 2, dt, s));
        if (h->split_proj(l)) LEAF_TRY(leaf_launch_split_pack(params + o.proj_w, nullptr, (void*)h->split_proj_lo(l), nullptr, d, 4 * d, 0, dt, s));
    }
    return 0;
}

extern "C" int leaf_text_pack_weights(leaf_text_t h, const float* params, void* w16_fwd, void* w16_bwd,
                                      leaf_stream_t s_) {
    hipStream_t s = (hipStream_t)s_;
    const int d = h->cfg.width, L = h->cfg.layers;
    // The fp32 GEMM weights of all layers are one contiguous run (qkv, out, fc, proj per layer = 12 d^2 floats, the
    // layout of leaf_text_create) and the 16-bit packs use the same offsets: one cast launch for the forward copy, one
    // grouped transpose launch for the data-gradient copy (was 48 + 48 launches).
    const float* w32 = params + h->layer[0].qkv_w;
    for (int l = 0; l < L; ++l)
        if (h->layer[l].qkv_w != h->layer[0].qkv_w + (size_t)l * h->w16_layer_elems() ||
            h->layer[l].proj_w != h->layer[l].qkv_w + (size_t)8 * d * d) {
            leaf_set_error("unexpected parameter layout");
            return 1;
        }
    if (w16_fwd) {
        LEAF_TRY(leaf_launch_cast(w32, w16_fwd, h->w16_layer_elems() * L, h->fwd_dtype, s));
        // LN folding (lnfold.h): gamma-scaled QKV / c_fc weights + their s[n], c[n] vectors, all layers in one launch
        const LayerOff& o = h->layer[0];
        const size_t vstride = L > 1 ? h->layer[1].ln1_w - o.ln1_w : 0;
        for (int l = 1; l < L; ++l)
            if (h->layer[l].ln1_w != o.ln1_w + l * vstride || h->layer[l].fc_b != o.fc_b + l * vstride) { leaf_set_error("unexpected parameter layout"); return 1; }
        LEAF_TRY(leaf_launch_fold_pack(params + o.qkv_w, params + o.fc_w, h->w16_layer_elems(), params + o.ln1_w, params + o.ln1_b,
                                       params + o.qkv_b, params + o.ln2_w, params + o.ln2_b, params + o.fc_b, vstride,
                                       (uint16_t*)w16_fwd + h->w16_fold_qkv(0), (uint16_t*)w16_fwd + h->w16_fold_fc(0),
                                       (size_t)7 * d * d, const_cast<float*>(h->fold_aux(w16_fwd, 0)), (size_t)14 * d, d, L,
                                       h->fwd_dtype, s));
    }
    if (w16_bwd) LEAF_TRY(leaf_launch_pack_transpose(w32, w16_bwd, h->grad_dtype, d, L, s));
    return 0;
}

// ------------------------------------------------------------------ per-launch GEMM profiler (bench.py roofline)
namespace {
struct ProfRec { hipEvent_t a, b; int key, M, N, K; double flops, bytes; };
bool g_prof_on = false;
std::vector<ProfRec> g_prof;

// `launch` between two events on its stream, recorded under r
template <class Launch>
int prof_bracket(ProfRec r, hipStream_t s, Launch launch) {
    LEAF_TRY(hipEventCreate(&r.a));
    LEAF_TRY(hipEventCreate(&r.b));
    LEAF_TRY(hipEventRecord(r.a, s));
    const int rc = launch();
    LEAF_TRY(hipEventRecord(r.b, s));
    g_prof.push_back(r);
    return rc;
}
// stops recording, waits for the recorded events, hands every record and its milliseconds to `each` and drops them
template <class Each>
int prof_drain(Each each) {
    g_prof_on = false;
    for (auto& r : g_prof) {
        LEAF_TRY(hipEventSynchronize(r.b));
        float t = 0.f;
        LEAF_TRY(hipEventElapsedTime(&t, r.a, r.b));
        each(r, t);
    }
    for (auto& r : g_prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    g_prof.clear();
    return 0;
}
}  // namespace

int leaf_gemm(const GemmArgs& g, int dtype, int epi, hipStream_t s) {
    const bool fold = epi == EPI_LNFOLD_T || epi == EPI_LNFOLD_ACT_T, resid_ln = epi == EPI_RESID_LN || epi == EPI_RESID_LN8;
    if ((fold && (!g.ln_s || !g.rowstat || !g.bias)) || (resid_ln && (!g.x16 || !g.stat_out || g.N % 64 || g.stat_ld < g.M))) {
        leaf_set_error("gemm: LN-folding operands missing or misshapen (epilogue %d)", epi);
        return 1;
    }
    auto launch = [&] { return leaf_check(leaf_launch_gemm(g, dtype, epi, s), "gemm"); };
    if (!g_prof_on) return launch();
    const double M = g.M, N = g.N, K = g.K;
    ProfRec r;
    r.key = LEAF_PROF_KEY(leaf_gemm_family(g, epi), dtype, epi);
    r.M = g.M; r.N = g.N; r.K = g.K;
    r.flops = 2.0 * M * N * K;
    {   // algorithmic bytes of the launch: both operands once + the output (+ the fp32 read of a residual/accumulate)
        const bool resid = epi == EPI_RESID_F32 || epi == EPI_RESID_LN;
        const double out_b = (resid || epi == EPI_STORE_F32) ? 4.0 : 2.0;
        const double rmw = (resid || (epi == EPI_STORE_F32 && g.beta != 0.f)) ? 4.0 : 0.0;
        r.bytes = 2.0 * (M * K + N * K) + M * N * (out_b + rmw) + (epi == EPI_ACTGRAD_T ? 2.0 * g.M * g.N : 0.0) +
                  (epi == EPI_RESID_LN ? 2.0 * g.M * g.N + 8.0 * g.M * (g.N / 64) : 0.0) +              // 16-bit copy + statistics
                  ((epi == EPI_LNFOLD_T || epi == EPI_LNFOLD_ACT_T) ? 8.0 * g.M : 0.0);                  // (mean, rstd) per row
    }
    // 16 + 8-bit residual stream: 3 bytes read + 3 written per output element, statistics
    if (epi == EPI_RESID_LN8) r.bytes = 2.0 * (M * K + N * K) + 6.0 * M * N + 8.0 * g.M * (g.N / 64);
    return prof_bracket(r, s, launch);
}

// the fused QKV + attention launch, accounted like a GEMM launch (family 8, epilogue id of the LN-folded QKV GEMM): FLOPs = the
// projection's 2 M 3d K (the attention's own products are not counted), bytes = A + weights + attention output
int leaf_qkv_attn(const QkvAttnArgs& a, int dtype, hipStream_t s) {
    auto launch = [&] { return leaf_check(leaf_launch_qkv_attn(a, dtype, s), "qkv_attn"); };
    if (!g_prof_on) return launch();
    ProfRec r;
    r.key = LEAF_PROF_KEY(8, dtype, EPI_LNFOLD_T);
    r.M = a.M; r.N = 3 * a.d; r.K = a.K;
    r.flops = 2.0 * (double)a.M * (3.0 * a.d) * (double)a.K;
    r.bytes = 2.0 * ((double)a.M * a.K + 3.0 * a.d * a.K) + 2.0 * (double)(a.eot_pos ? a.n_seq : a.M) * a.d + 8.0 * a.M;
    return prof_bracket(r, s, launch);
}

extern "C" int leaf_prof_begin(void) {
    for (auto& r : g_prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    g_prof.clear();
    g_prof_on = true;
    return 0;
}

// Suspends (1) / resumes (0) the recording without dropping what has been recorded: a caller that times MANY steps takes the per-launch
// events on a sample of them only (each event pair costs the queue a completion barrier: round 4, 1.2 ms of a 50-ms step)
extern "C" int leaf_prof_pause(int paused) {
    g_prof_on = !paused;
    return 0;
}

// Stops recording, waits for the recorded events and sums them grouped by (key = LEAF_PROF_KEY: kernel_family*32 + dtype*16 +
// epilogue id, N, K) -- one line per GEMM SHAPE of each kernel, so that e.g. the two residual GEMMs (out_proj: N = K = d, HBM-bound;
// c_proj: K = 4d, MFMA-bound) are reported separately.  ms / flops / bytes (algorithmic operand + output bytes) per group; info[i] =
// {key (+ LEAF_PROF_BIG = 1024 for launches of >= 16,384 rows), N, K, launches}; rows[i] = sum of M over the launches.  Returns the number of groups in *n_out (<= max_groups).
extern "C" int leaf_prof_end_shapes(double* ms, double* flops, double* bytes, int64_t* rows, int32_t* info, int max_groups,
                                    int* n_out) {
    int n = 0;
    const int rc = prof_drain([&](const ProfRec& r, float t) {
        // launches of >= 16,384 rows (the scoring passes) and the small B-caption launches of the same kernel and shape are
        // reported apart: group key = key + LEAF_PROF_BIG for the big ones
        const int gkey = r.key + (r.M >= 16384 ? LEAF_PROF_BIG : 0);
        int i = 0;
        for (; i < n; ++i)
            if (info[4 * i] == gkey && info[4 * i + 1] == r.N && info[4 * i + 2] == r.K) break;
        if (i == n) {
            if (n == max_groups) return;
            info[4 * n] = gkey; info[4 * n + 1] = r.N; info[4 * n + 2] = r.K; info[4 * n + 3] = 0;
            ms[n] = 0; flops[n] = 0; bytes[n] = 0; rows[n] = 0;
            ++n;
        }
        ms[i] += t; flops[i] += r.flops; bytes[i] += r.bytes; rows[i] += r.M; info[4 * i + 3] += 1;
    });
    if (rc) return rc;
    if (n_out) *n_out = n;
    return 0;
}

extern "C" size_t leaf_text_workspace_bytes(leaf_text_t h, int n_seq, int mode) {
    if (!h || n_seq < 1) return 0;
    const int cs = n_seq < h->chunk ? n_seq : h->chunk;
    size_t b = fwd_chunk_bytes(h, cs) + 512;      // alignment slack of the buffer set and of the workspace base
    if (mode == 1) b += align_up((size_t)n_seq * h->cfg.embed_dim * 4, 256) + 256;
    if (mode == 2) return leaf_train_ws_bytes(h, n_seq);
    return b;
}

extern "C" int leaf_text_forward(leaf_text_t h, const float* params, const void* w16_fwd, const int32_t* tokens,
                                 const int32_t* seq_lens, const int32_t* cu_rows, int n_seq, float* out, int normalize,
                                 void* ws, size_t ws_bytes, leaf_stream_t s) {
    if (!h || !params || !w16_fwd || !tokens || !out || !ws || n_seq < 1) { leaf_set_error("null/invalid argument"); return 1; }
    Carver c(ws, ws_bytes);
    return forward_all(h, params, w16_fwd, tokens, seq_lens, cu_rows, n_seq, out, normalize, c, (hipStream_t)s);
}

// ------------------------------------------------------------------ per-token hidden states (include/leaf_hip.h, leaf_hidden_args)
// A plain pass with taps: the argument checks, then forward_all / precise_all.  Every refusal comes before the first HIP call.
extern "C" int leaf_text_forward_hidden(leaf_text_t h, const leaf_hidden_args* a) {
    if (!a || a->size != sizeof(*a)) { leaf_set_error("leaf_hidden_args: size %u, this library's is %zu", a ? a->size : 0u, sizeof(*a)); return 1; }
    if (!h) { leaf_set_error("forward_hidden: null handle"); return 1; }
    if (!a->params) { leaf_set_error("forward_hidden: params is null"); return 1; }
    if (!a->tokens) { leaf_set_error("forward_hidden: tokens is null"); return 1; }
    if (!a->ws) { leaf_set_error("forward_hidden: ws is null"); return 1; }
    if (a->n_seq < 1) { leaf_set_error("forward_hidden: n_seq %d", a->n_seq); return 1; }
    if (a->n_taps < 0 || (a->n_taps > 0 && !a->taps)) { leaf_set_error("forward_hidden: n_taps %d with taps %s", a->n_taps, a->taps ? "given" : "null"); return 1; }
    if (a->n_taps < 1 && !a->feat) { leaf_set_error("forward_hidden: n_taps < 1 and feat is null: the pass has no output"); return 1; }
    if (a->out_dtype != 0 && a->out_dtype != 1) { leaf_set_error("forward_hidden: out_dtype %d (0 fp32, 1 the handle's 16-bit type)", a->out_dtype); return 1; }
    if (a->precise && a->out_dtype) { leaf_set_error("forward_hidden: precise writes fp32 rows (out_dtype 0)"); return 1; }
    if (!a->precise && !a->w16_fwd) { leaf_set_error("forward_hidden: w16_fwd is null (only the precise pass does without it)"); return 1; }
    if ((a->seq_lens == nullptr) != (a->cu_rows == nullptr)) { leaf_set_error("forward_hidden: seq_lens (host) and cu_rows (device) go together"); return 1; }
    const int L = h->cfg.layers;
    for (int i = 0; i < a->n_taps; ++i) {
        const leaf_hidden_tap& t = a->taps[i];
        if (!t.out) { leaf_set_error("forward_hidden: taps[%d].out is null", i); return 1; }
        if (t.layer < 0 || t.layer > L) { leaf_set_error("forward_hidden: taps[%d].layer %d outside 0..%d", i, t.layer, L); return 1; }
        for (int j = 0; j < i; ++j)
            if (a->taps[j].layer == t.layer && !a->taps[j].final_ln == !t.final_ln) {
                leaf_set_error("forward_hidden: taps[%d] and taps[%d] are both (layer %d, final_ln %d)", j, i, t.layer, t.final_ln ? 1 : 0);
                return 1;
            }
    }
    if (a->n_taps > 0 && !leaf_hidden_rows_ok(h->cfg.width)) { leaf_set_error("forward_hidden: width %d (the row kernel takes width %% 4 == 0, <= 2048)", h->cfg.width); return 1; }
    const HiddenTaps taps{a->taps, a->n_taps, a->out_dtype};
    const HiddenTaps* tp = a->n_taps > 0 ? &taps : nullptr;
    hipStream_t s = (hipStream_t)a->stream;
    if (a->precise) return precise_all(h, a->params, a->tokens, a->seq_lens, a->cu_rows, a->n_seq, a->feat, a->normalize, a->ws, a->ws_bytes, s, tp);
    Carver c(a->ws, a->ws_bytes);
    return forward_all(h, a->params, a->w16_fwd, a->tokens, a->seq_lens, a->cu_rows, a->n_seq, a->feat, a->normalize, c, s, PrefixPlan(), tp);
}

// ------------------------------------------------------------------ scoring passes
namespace {
// argument checks of the class target (loss is required: best_idx is taken from it)
int cls_check(const float* class_feat, int C, const int32_t* labels, const float* loss, int rho) {
    if (!class_feat || !labels || !loss) { leaf_set_error("null/invalid argument"); return 1; }
    if (C < LEAF_CLS_MIN_CLASSES || C > LEAF_CLS_MAX_CLASSES) {
        leaf_set_error("%d classes: the classification score takes %d .. %d", C, LEAF_CLS_MIN_CLASSES, LEAF_CLS_MAX_CLASSES);
        return 1;
    }
    if (rho > LEAF_SCORE_MAX_RHO) { leaf_set_error("rho %d: one scoring launch takes %d candidates per caption", rho, LEAF_SCORE_MAX_RHO); return 1; }
    return 0;
}
}  // namespace

// ------------------------------------------------------------------ prefix reuse
extern "C" size_t leaf_text_kv_bytes(leaf_text_t h, int n_seq) {
    if (!h || n_seq < 1) return 0;
    return (size_t)h->cfg.layers * n_seq * h->cfg.context_length * 3 * h->cfg.width * 2;
}

extern "C" int leaf_text_forward_kv(leaf_text_t h, const float* params, const void* w16_fwd, const int32_t* tokens,
                                    const int32_t* seq_lens, const int32_t* cu_rows, int n_seq, float* out,
                                    int normalize, void* kv, size_t kv_bytes, void* ws, size_t ws_bytes, leaf_stream_t s) {
    if (!h || !params || !w16_fwd || !tokens || !kv || !ws || n_seq < 1) { leaf_set_error("null/invalid argument"); return 1; }
    if ((seq_lens == nullptr) != (cu_rows == nullptr)) { leaf_set_error("seq_lens (host) and cu_rows (device) go together"); return 1; }
    const int ctx = h->cfg.context_length;
    size_t rows = 0;
    int max_len = 0;
    for (int i = 0; i < n_seq; ++i) {
        const int L = seq_lens ? seq_lens[i] : ctx;
        rows += L;
        max_len = L > max_len ? L : max_len;
    }
    const size_t stride = rows * 3 * h->cfg.width;
    if (stride * 2 * h->cfg.layers > kv_bytes) { leaf_set_error("kv cache too small"); return 1; }
    if (rows > (size_t)h->chunk * ctx) { leaf_set_error("forward_kv needs the captions to fit one chunk (%zu rows)", rows); return 1; }
    Carver c(ws, ws_bytes);
    FwdBuf b = carve_fwd(h, c, (int)((rows + ctx - 1) / ctx));
    if (!c.ok()) { leaf_set_error("workspace too small: need %zu bytes, have %zu", c.off, c.cap); return 1; }
    KvPlan kvp;
    kvp.kv_write = (uint16_t*)kv;
    kvp.kv_stride = stride;
    RowMap map{cu_rows, 0, 0, ctx, nullptr, nullptr, 1};
    return forward_chunk(h, params, (const uint16_t*)w16_fwd, tokens, n_seq, (int)rows, map, out, normalize, b,
                         (hipStream_t)s, kvp, max_len);
}

// One scoring pass (include/leaf_hip.h, leaf_score_args): the fields say which rows it computes and what it compares the candidates
// with -- one anchor row per caption under one of the four objectives (leaf_launch_score), or a class matrix shared by all captions
// with a label per caption (leaf_launch_classify, classify.hip).  Every refusal comes before the first HIP call.
extern "C" int leaf_score_pass(leaf_text_t h, const leaf_score_args* a) {
    if (!a || a->size != sizeof(*a)) { leaf_set_error("leaf_score_args: size %u, this library's is %zu", a ? a->size : 0u, sizeof(*a)); return 1; }
    if (!h || !a->params || !a->w16_fwd || !a->tokens || !a->best_idx || !a->ws || a->B < 1 || a->rho < 1) {
        leaf_set_error("null/invalid argument");
        return 1;
    }
    if ((a->anchor != nullptr) == (a->class_feat != nullptr)) { leaf_set_error("score_pass: exactly one of anchor / class_feat"); return 1; }
    if (a->anchor && (a->objective < 0 || a->objective > 3)) { leaf_set_error("unknown objective %d", a->objective); return 1; }
    if (a->class_feat && cls_check(a->class_feat, a->C, a->labels, a->loss, a->rho)) return 1;
    const bool fused = a->kv_write != 0;
    if (!a->prefix && (a->kv || a->base_cu || fused)) { leaf_set_error("score_pass: kv / base_cu / kv_write without prefix"); return 1; }
    if (a->prefix && (!a->kv || !a->seq_lens || !a->cu_rows || (a->base_cu == nullptr) != fused)) {
        leaf_set_error("score_pass: a prefix pass needs seq_lens, cu_rows, kv and base_cu (the fused first stage: no base_cu)");
        return 1;
    }
    if (fused && a->class_feat) { leaf_set_error("score_pass: the fused first stage takes an anchor target only"); return 1; }
    // candidates grouped rho per caption; earlier positions are read from the cache ...
    PrefixPlan pp;
    int n_seq = a->B * a->rho;
    if (a->prefix) {
        pp.prefix_dev = a->prefix;
        pp.max_len = a->max_len;
        pp.group = a->rho;
        size_t base_rows = a->base_rows;
        if (fused) {
            // ... which this pass writes itself: sequences 0 .. B-1 are the captions (full rows, prefix 0), B .. B + B rho - 1 their
            // candidates; seq_lens / cu_rows / prefix cover all of them.  forward_all returns 2 (and an error text) when the rows do
            // not fit one chunk: the caller then runs leaf_text_forward_kv and a prefix pass
            base_rows = 0;
            for (int i = 0; i < a->B; ++i) base_rows += a->seq_lens[i];
            if (base_rows * 3 * h->cfg.width * 2 * h->cfg.layers > a->kv_bytes) { leaf_set_error("kv cache too small"); return 1; }
            n_seq += a->B;
            pp.base_cu_dev = a->cu_rows;          // the captions are the first sequences: their row offsets are the first B entries
            pp.group_off = a->B;
            pp.kv_copy = (uint16_t*)a->kv;
            pp.kv_self_rows = base_rows;
        } else {
            pp.base_cu_dev = a->base_cu;
            pp.kv = (const uint16_t*)a->kv;
        }
        pp.kv_stride = base_rows * 3 * h->cfg.width;
    }
    // features of the pass's n_seq sequences -> workspace, then the best of the rho candidates of each of the B captions: the candidates
    // are the LAST B * rho sequences of the pass (the fused first stage has its B captions in front of them)
    const int D = h->cfg.embed_dim, B = a->B, rho = a->rho;
    hipStream_t s = (hipStream_t)a->stream;
    Carver c(a->ws, a->ws_bytes);
    float* feat = (float*)c.take((size_t)n_seq * D * 4);
    const int normalize = (a->class_feat || a->objective == LEAF_OBJ_SIM || a->objective == LEAF_OBJ_DISSIM);
    const int rc = forward_all(h, a->params, a->w16_fwd, a->tokens, a->seq_lens, a->cu_rows, n_seq, feat, normalize, c, s, pp);
    if (rc) return rc;
    const float* cand = feat + (size_t)(n_seq - B * rho) * D;
    if (a->class_feat)
        LEAF_TRY(leaf_launch_classify(cand, a->class_feat, a->labels, B, rho, D, a->C, a->loss, a->pred, a->logits, a->best_idx, a->best_feat, s));
    else
        LEAF_TRY(leaf_launch_score(cand, a->anchor, B, rho, D, a->objective, a->best_idx, a->best_feat, a->loss, s));
    return 0;
}

// ------------------------------------------------------------------ single-kernel hooks for the parity tests
extern "C" int leaf_op_gemm_ld(int dtype, int epi, const void* A, int lda, const void* B, int ldb, void* C, int ldc,
                               const float* bias, void* aux, int M, int N, int K, int act, float beta, int aux_f16,
                               leaf_stream_t s) {
    GemmArgs g = gemm_dense(A, B, C, bias, M, N, K);
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.aux = aux; g.act = act; g.beta = beta; g.aux_f16 = aux_f16;
    return leaf_gemm(g, dtype, epi, (hipStream_t)s);
}
extern "C" int leaf_op_gemm(int dtype, int epi, const void* A, const void* B, void* C, const float* bias, void* aux,
                            int M, int N, int K, int act, float beta, int aux_f16, leaf_stream_t s) {
    return leaf_op_gemm_ld(dtype, epi, A, K, B, K, C, N, bias, aux, M, N, K, act, beta, aux_f16, s);
}
// C32 += [A | A] B^T + bias over K = 2 Ka with A stored once as [M, Ka] (GemmArgs::a_wrap: the half-stage ring kernel re-reads the A
// panel; fails for launches that kernel does not take) -- the out-projection of a split block; the parity tests hold it to the
// launch on a materialised [A | A]
extern "C" int leaf_op_gemm_awrap(int dtype, const void* A, const void* B, float* C, const float* bias, int M, int N, int Ka, leaf_stream_t s) {
    if (Ka % 64) { leaf_set_error("gemm_awrap: Ka %% 64"); return 1; }
    GemmArgs g = gemm_dense(A, B, C, bias, M, N, 2 * Ka);
    g.lda = Ka; g.a_wrap = Ka / 64;
    return leaf_gemm(g, dtype, EPI_RESID_F32, (hipStream_t)s);
}
// LN folding (lnfold.h): the producing residual GEMM (C32 += A B^T + bias, x16 = 16-bit(C32), stat[N/64][M] = (sum, M2)) ...
static int op_gemm_resid_ln(int dtype, int epi, const void* A, const void* B, void* C, const float* bias, void* x16, void* stat, int M,
                            int N, int K, leaf_stream_t s) {
    GemmArgs g = gemm_dense(A, B, C, bias, M, N, K);
    g.x16 = x16; g.ldx16 = N; g.stat_out = (float2*)stat; g.stat_ld = M;
    return leaf_gemm(g, dtype, epi, (hipStream_t)s);
}
extern "C" int leaf_op_gemm_resid_ln(int dtype, const void* A, const void* B, float* C, const float* bias, void* x16, void* stat,
                                     int M, int N, int K, leaf_stream_t s) {
    return op_gemm_resid_ln(dtype, EPI_RESID_LN, A, B, C, bias, x16, stat, M, N, K, s);
}
// the same on the 16 + 8-bit residual stream: (x16, lo8) <- encode(decode(x16, lo8) + A B^T + bias) in place, statistics as above
extern "C" int leaf_op_gemm_resid_ln8(int dtype, const void* A, const void* B, void* lo8, const float* bias, void* x16, void* stat,
                                      int M, int N, int K, leaf_stream_t s) {
    return op_gemm_resid_ln(dtype, EPI_RESID_LN8, A, B, lo8, bias, x16, stat, M, N, K, s);
}
extern "C" int leaf_op_resid_pack(int dtype, const float* x, void* x16, void* lo8, size_t n, leaf_stream_t s) {
    return leaf_check(leaf_launch_resid_pack(x, x16, lo8, n, dtype, (hipStream_t)s), "resid_pack");
}
extern "C" int leaf_op_resid_unpack(int dtype, const void* x16, const void* lo8, float* x, size_t n, leaf_stream_t s) {
    return leaf_check(leaf_launch_resid_unpack(x16, lo8, x, n, dtype, (hipStream_t)s), "resid_unpack");
}
// ... the merge of the partials into rowstat[M] = (mean, rstd), and the consuming GEMM: C16 = [act](rstd[m] (A Bp^T - mean[m] s[n]) + c[n]); act < 0: none
extern "C" int leaf_op_ln_finalize(const void* stat, int ld, int rows, int ngroups, float eps, void* rowstat, leaf_stream_t s) {
    return leaf_check(leaf_launch_ln_finalize((const float2*)stat, ld, rows, ngroups, eps, (float2*)rowstat, (hipStream_t)s), "ln_finalize");
}
extern "C" int leaf_op_gemm_lnfold(int dtype, int act, const void* A, const void* Bp, void* C16, const float* c_vec,
                                   const float* s_vec, const void* rowstat, int M, int N, int K, leaf_stream_t s) {
    GemmArgs g = gemm_dense(A, Bp, C16, c_vec, M, N, K);
    g.ln_s = s_vec; g.rowstat = (const float2*)rowstat; g.act = act < 0 ? 0 : act;
    return leaf_gemm(g, dtype, act < 0 ? EPI_LNFOLD_T : EPI_LNFOLD_ACT_T, (hipStream_t)s);
}
// The fused QKV + attention launch alone (tools/qkv_attn_bench.py): lens (host) = rows per sequence, cu / prefix / base_cu device
// arrays as in a prefix leaf_score_pass (prefix / base_cu / kv may be null: no cached prefix), tile_seq = device scratch
// [n_seq + 1].  Synchronous plan upload: a measuring / test hook, not a step of the pipeline.
extern "C" int leaf_op_qkv_attn(int dtype, const void* x16, const void* Wp, const float* c_vec, const float* s_vec, const void* rowstat,
                                void* out, const void* kv, const int32_t* lens, const int32_t* cu, const int32_t* prefix,
                                const int32_t* base_cu, const int32_t* eot_pos, int32_t* tile_seq, int n_seq, int rows, int group,
                                int ctx, int heads, int width, leaf_stream_t s) {
    if (!leaf_qkv_attn_eligible(width, heads, ctx, width, 0)) { leaf_set_error("qkv_attn: unsupported shape"); return 1; }
    std::vector<int32_t> plan(2 * ((size_t)n_seq + 2));
    const int n_tiles = leaf_qkv_attn_plan(lens, ctx, 0, n_seq, prefix != nullptr, group, 0, leaf_qkv_attn_tile_rows(), leaf_qkv_attn_ncap(ctx),
                                           plan.data());
    LEAF_TRY(hipMemcpy(tile_seq, plan.data(), (size_t)(n_tiles + 1) * 2 * sizeof(int32_t), hipMemcpyHostToDevice));
    const QkvAttnArgs qa = fill_qkv_attn_args(QkvOperands{x16, (const uint16_t*)Wp, s_vec, c_vec, width}, (const float2*)rowstat, out, kv, eot_pos,
                                              tile_seq, RowMap{cu, 0, 0, ctx, prefix, base_cu, group > 0 ? group : 1, 0}, rows, n_seq, n_tiles,
                                              heads, width, ctx);
    return leaf_check(leaf_launch_qkv_attn(qa, dtype, (hipStream_t)s), "qkv_attn");
}
// ---- diagnostic exports (include/leaf_hip_diag.h): only in the builds of `make variants` / `make stamps` ... under tools/diag/
#ifdef LEAF_DIAG_EXPORTS
extern "C" int leaf_debug_qkv_attn_plan(const int32_t* lens, int ctx, int s0, int n, int prefixed, int group, int group_off, int tile_rows,
                                        int ncap, int32_t* out) {
    return leaf_qkv_attn_plan(lens, ctx, s0, n, prefixed, group, group_off, tile_rows > 0 ? tile_rows : leaf_qkv_attn_tile_rows(),
                              ncap > 0 ? ncap : leaf_qkv_attn_ncap(ctx), out);
}
extern "C" int leaf_debug_gemm_stamps(void* buf) { leaf_gemm_set_stamps(buf); return 0; }
extern "C" int leaf_debug_gemm_min_tiles(int n) { leaf_gemm256h_set_min_tiles(n); return 0; }
extern "C" int leaf_debug_gemm_family(int M, int N, int K, int lda, int ldb, int ldc, int epi, int a_wrap) {
    GemmArgs g;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldx16 = N; g.a_wrap = a_wrap;
    return leaf_gemm_family(g, epi);
}
#endif
extern "C" int leaf_op_attention_fwd(const void* qkv, void* out, int n_seq, int ctx, int heads, int width, int dtype,
                                     leaf_stream_t s) {
    return leaf_check(leaf_launch_attention_fwd(qkv, nullptr, out, n_seq, RowMap{nullptr, 0, 0, ctx, nullptr, nullptr, 1}, heads, width, dtype,
                                                (hipStream_t)s), "attention_fwd");
}
// ... and in every row mode of the launcher (tests/test_gpu_attention_modes.py): no logic of its own, the launcher checks the arguments
extern "C" int leaf_op_attention_fwd_map(const void* qkv, const void* kv, void* out, const int32_t* cu, const int32_t* prefix,
                                         const int32_t* base_cu, const int32_t* eot_pos, int n_seq, int ctx, int group, int group_off,
                                         int max_len, int single_edit, int heads, int width, int dtype, leaf_stream_t s) {
    return leaf_check(leaf_launch_attention_fwd(qkv, kv, out, n_seq, RowMap{cu, 0, 0, ctx, prefix, base_cu, group > 0 ? group : 1, group_off},
                                                heads, width, dtype, (hipStream_t)s, eot_pos, max_len, single_edit), "attention_fwd_map");
}
extern "C" int leaf_op_layernorm(const float* x, const float* g, const float* b, float eps, void* out16, int rows,
                                 int width, int dtype, leaf_stream_t s) {
    return leaf_check(leaf_launch_layernorm(x, g, b, eps, out16, rows, width, dtype, (hipStream_t)s), "layernorm");
}
extern "C" int leaf_op_attention_bwd_t(const void* qkv, int qkv_dtype, const void* dout16, void* dqkv16, int g_dtype,
                                       int n_seq, int ctx, int heads, int width, leaf_stream_t s) {
    return leaf_check(leaf_launch_attention_bwd(qkv, qkv_dtype, dout16, dqkv16, g_dtype, n_seq,
                                                RowMap{nullptr, 0, 0, ctx, nullptr, nullptr, 1}, heads, width, (hipStream_t)s), "attention_bwd");
}
// ... and on packed rows (cu [n_seq + 1] on the device, NULL = dense): the RowMap of leaf_text_backward (tests/test_gpu_backward_rows.py)
extern "C" int leaf_op_attention_bwd_map(const void* qkv, int qkv_dtype, const void* dout16, void* dqkv16, int g_dtype,
                                         const int32_t* cu, int n_seq, int ctx, int heads, int width, leaf_stream_t s) {
    if (!qkv || !dout16 || !dqkv16 || n_seq < 1) { leaf_set_error("null/invalid argument"); return 1; }
    return leaf_check(leaf_launch_attention_bwd(qkv, qkv_dtype, dout16, dqkv16, g_dtype, n_seq,
                                                RowMap{cu, 0, 0, ctx, nullptr, nullptr, 1}, heads, width, (hipStream_t)s), "attention_bwd_map");
}
extern "C" int leaf_op_wgrad(const void* dY, const void* X, float* dW, float* db, int rows, int Nw, int Kw, int x_dtype,
                             int g_dtype, const float* alpha_dev, leaf_stream_t s) {
    if (!leaf_wgrad_tn_ok(Nw, Kw, Nw, Kw)) { leaf_set_error("wgrad needs Nw, Kw multiples of 128"); return 1; }
    WgradArgs wa{};
    wa.p[0] = WgradProb{(const uint16_t*)dY, (const uint16_t*)X, dW, db, Nw, Kw, Nw, Kw, 0, 0};
    wa.nprob = 1; wa.rows = rows; wa.alpha = alpha_dev;
    return leaf_check(leaf_launch_wgrad_group(wa, x_dtype, g_dtype, (hipStream_t)s), "wgrad_group");
}
extern "C" size_t leaf_op_layernorm_bwd_ws_bytes(int rows, int d) {
    return (size_t)leaf_ln_bwd_grid(rows, d) * 2 * d * sizeof(float);
}
extern "C" int leaf_op_layernorm_bwd(const float* dy, const float* x, const float* g, float eps, float* dx_inout, void* dx16,
                                     int g_dtype, const float* gscale, float* dg, float* db, int rows, int d, void* ws,
                                     size_t ws_bytes, leaf_stream_t s) {
    if (!dy || !x || !g || !dx_inout || !gscale || rows < 1 || (dg == nullptr) != (db == nullptr)) { leaf_set_error("layernorm_bwd: null/invalid argument"); return 1; }
    if (dg && (!ws || ws_bytes < leaf_op_layernorm_bwd_ws_bytes(rows, d))) { leaf_set_error("layernorm_bwd: workspace too small (need %zu bytes)", leaf_op_layernorm_bwd_ws_bytes(rows, d)); return 1; }
    LEAF_TRY(leaf_launch_layernorm_bwd(dy, x, g, eps, dx_inout, dx16, g_dtype == LEAF_F16 ? 1 : 0, dg ? (float*)ws : nullptr, rows, d, (hipStream_t)s));
    if (!dg) return 0;
    LnReduceArgs ra{};
    ra.part = (const float*)ws; ra.n = 1; ra.grid = leaf_ln_bwd_grid(rows, d); ra.d = d; ra.inv_s = gscale + 1;
    ra.dg[0] = dg; ra.db[0] = db;
    return leaf_check(leaf_launch_ln_param_reduce(ra, (hipStream_t)s), "ln_param_reduce");
}
// the classification score alone (classify.hip) on given feature rows: the kernel hook of tests/test_gpu_zeroshot.py
extern "C" int leaf_op_classify(const float* feat, const float* class_feat, const int32_t* labels, int B, int rho, int D, int C, float* loss,
                                int32_t* pred, float* logits, int32_t* best_idx, float* best_feat, leaf_stream_t s) {
    if (!feat || !best_idx || B < 1 || rho < 1 || D < 1) { leaf_set_error("null/invalid argument"); return 1; }
    if (cls_check(class_feat, C, labels, loss, rho)) return 1;
    return leaf_check(leaf_launch_classify(feat, class_feat, labels, B, rho, D, C, loss, pred, logits, best_idx, best_feat, (hipStream_t)s),
                      "classify");
}
extern "C" int leaf_op_project_rows(const float* xg, const float* g, const float* b, float eps, const float* proj,
                                    float* xn_scratch, float* out, int M, int d, int D, int normalize, leaf_stream_t s) {
    if (!leaf_project_rows_ok(d, D)) { leaf_set_error("project_rows needs D %% 128 == 0 and d %% 16 == 0"); return 1; }
    return leaf_check(leaf_launch_project_rows(xg, g, b, eps, proj, xn_scratch, out, M, d, D, normalize, (hipStream_t)s), "project_rows");
}
