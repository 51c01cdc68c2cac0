// C ABI, training half: forward with activation stash, TextFARE loss + backward into the flat gradient
// buffer, fused AdamW.  Host orchestration only; see include/leaf_hip.h for the contract.
#include "engine.h"

namespace {

struct Stash {
    float* xin;      // [(L+1)][rows,d]  layer inputs; xin[L] = final residual stream
    float* x1;       // [L][rows,d]      after the attention residual
    uint16_t* xn1;   // [L][rows,d]
    uint16_t* qkv;   // [L][rows,3d]
    uint16_t* ao;    // [L][rows,d]
    uint16_t* xn2;   // [L][rows,d]
    uint16_t* pre;   // [L][rows,4d]
    uint16_t* hh;    // [L][rows,4d]
    float* pooled;   // [n,d]
    int32_t* eot;    // [n]
    float* norms;    // [n]  ||features|| of the last training forward (--normalize_fare)
};

size_t total_rows(const leaf_text* h, const int32_t* lens, int n_seq) {
    if (!lens) return (size_t)n_seq * h->cfg.context_length;
    size_t r = 0;
    for (int i = 0; i < n_seq; ++i) r += lens[i];
    return r;
}

Stash carve_stash(const leaf_text* h, Carver& c, int n_seq, size_t rows) {
    const size_t d = h->cfg.width, L = h->cfg.layers;
    Stash s;
    s.xin = (float*)c.take((L + 1) * rows * d * 4);
    s.x1 = (float*)c.take(L * rows * d * 4);
    s.xn1 = (uint16_t*)c.take(L * rows * d * 2);
    s.qkv = (uint16_t*)c.take(L * rows * 3 * d * 2);
    s.ao = (uint16_t*)c.take(L * rows * d * 2);
    s.xn2 = (uint16_t*)c.take(L * rows * d * 2);
    s.pre = (uint16_t*)c.take(L * rows * 4 * d * 2);
    s.hh = (uint16_t*)c.take(L * rows * 4 * d * 2);
    s.pooled = (float*)c.take((size_t)n_seq * d * 4);
    s.eot = (int32_t*)c.take((size_t)n_seq * 4);
    s.norms = (float*)c.take((size_t)n_seq * 4);
    return s;
}

struct BwdBuf {
    float* dx;        // [rows,d]
    uint16_t* dx16;   // [rows,d] 16-bit gradient at the block output (dY of c_proj)
    uint16_t* dx16b;  // [rows,d] 16-bit gradient after the MLP branch (dY of out_proj)
    float* dxn;       // [rows,d]
    uint16_t* big16;  // [rows,4d] bf16
    uint16_t* dqkv;   // [rows,3d] bf16
    uint16_t* do16;   // [rows,d] bf16
    float* dout;      // [n,D]
    float* gscale;    // {S, 1/S}
    float* lnpart;    // [2 layers][leaf_ln_bwd_grid][2][d] per-workgroup partial sums of the LayerNorm parameter gradients
};

BwdBuf carve_bwd(const leaf_text* h, Carver& c, int n_seq, size_t rows) {
    const size_t d = h->cfg.width;
    BwdBuf b;
    b.dx = (float*)c.take(rows * d * 4);
    b.dx16 = (uint16_t*)c.take(rows * d * 2);
    b.dx16b = (uint16_t*)c.take(rows * d * 2);
    b.dxn = (float*)c.take(rows * d * 4 + (size_t)n_seq * 8);   // + {mu, rstd} per sequence (pool backward scratch)
    b.big16 = (uint16_t*)c.take(rows * 4 * d * 2);
    b.dqkv = (uint16_t*)c.take(rows * 3 * d * 2);
    b.do16 = (uint16_t*)c.take(rows * d * 2);
    b.dout = (float*)c.take((size_t)n_seq * h->cfg.embed_dim * 4);
    b.gscale = (float*)c.take(256 + (size_t)n_seq * 8);   // {S, 1/S} + per-caption loss partials
    b.lnpart = (float*)c.take((size_t)2 * h->cfg.layers * leaf_ln_bwd_grid((int)rows, (int)d) * 2 * d * 4);
    return b;
}

}  // namespace

size_t leaf_train_ws_bytes(const leaf_text* h, int n_seq) {
    Carver c(nullptr, 0);
    carve_bwd(h, c, n_seq, (size_t)n_seq * h->cfg.context_length);
    return align_up(c.off, 256) + 256;
}

extern "C" size_t leaf_text_stash_bytes(leaf_text_t h, int n_seq) {
    if (!h || n_seq < 1) return 0;
    Carver c(nullptr, 0);
    carve_stash(h, c, n_seq, (size_t)n_seq * h->cfg.context_length);
    return align_up(c.off, 256) + 256;
}

// Training forward (include/leaf_hip.h, leaf_train_fwd_args).  pool_last: pool at the last kept row of each sequence instead of the
// first maximum token id.  Every refusal comes before the first HIP call.
extern "C" int leaf_text_forward_train(leaf_text_t h, const leaf_train_fwd_args* a) {
    if (!a || a->size != sizeof(*a)) { leaf_set_error("leaf_train_fwd_args: size %u, this library's is %zu", a ? a->size : 0u, sizeof(*a)); return 1; }
    const float* P = a->params;
    const int32_t *tokens = a->tokens, *seq_lens = a->seq_lens, *cu_rows = a->cu_rows;
    const float* delta = a->delta;
    float* out = a->out;
    void* ws = a->ws;
    const size_t ws_bytes = a->ws_bytes;
    const int n_seq = a->n_seq;
    const bool pool_last = a->pool_last != 0;
    if (!h || !P || !a->w16_fwd || !tokens || !out || !a->stash || n_seq < 1) { leaf_set_error("null/invalid argument"); return 1; }
    hipStream_t s = (hipStream_t)a->stream;
    if ((seq_lens == nullptr) != (cu_rows == nullptr)) { leaf_set_error("seq_lens (host) and cu_rows (device) go together"); return 1; }
    if (pool_last && delta) { leaf_set_error("forward_train: pool_last takes no delta"); return 1; }
    if (pool_last && (!seq_lens || !ws || ws_bytes < (size_t)n_seq * h->cfg.width * 4)) {
        leaf_set_error("forward_train: pool_last needs explicit seq_lens / cu_rows and a workspace of n_seq x width floats");
        return 1;
    }
    const leaf_text_cfg& cf = h->cfg;
    const int rows = (int)total_rows(h, seq_lens, n_seq);
    Carver c(a->stash, a->stash_bytes);
    Stash st = carve_stash(h, c, n_seq, rows);
    if (!c.ok()) { leaf_set_error("stash too small: need %zu bytes, have %zu", c.off, c.cap); return 1; }
    const RowMap map{cu_rows, 0, 0, cf.context_length, nullptr, nullptr, 1};
    int max_len = 0;
    for (int i = 0; i < n_seq; ++i) { const int Ls = seq_lens ? seq_lens[i] : cf.context_length; max_len = Ls > max_len ? Ls : max_len; }
    const int d = cf.width, dt = h->fwd_dtype, L = cf.layers;
    const size_t rd = (size_t)rows * d;
    const uint16_t* W = (const uint16_t*)a->w16_fwd;
    LEAF_TRY(leaf_launch_embed_ln(tokens, P + h->tok_emb, P + h->pos_emb, P + h->layer[0].ln1_w, P + h->layer[0].ln1_b,
                                  cf.ln_eps, st.xin, st.xn1, rows, n_seq, map, d, cf.vocab_size, dt, s, delta));
    for (int l = 0; l < L; ++l) {
        const LayerOff& o = h->layer[l];
        float* xin = st.xin + l * rd; float* x1 = st.x1 + l * rd; float* xout = st.xin + (l + 1) * rd;
        uint16_t* xn1 = st.xn1 + l * rd; uint16_t* qkv = st.qkv + 3 * l * rd; uint16_t* ao = st.ao + l * rd;
        uint16_t* xn2 = st.xn2 + l * rd; uint16_t* pre = st.pre + 4 * l * rd; uint16_t* hh = st.hh + 4 * l * rd;
        if (l > 0) LEAF_TRY(leaf_launch_layernorm(xin, P + o.ln1_w, P + o.ln1_b, cf.ln_eps, xn1, rows, d, dt, s));
        if (leaf_gemm(gemm_dense(xn1, W + h->w16_qkv(l), qkv, P + o.qkv_b, rows, 3 * d, d), dt, EPI_STORE_T, s)) return 1;
        LEAF_TRY(leaf_launch_attention_fwd(qkv, nullptr, ao, n_seq, map, cf.heads, d, dt, s, nullptr, max_len));
        // out-of-place residual adds (aux = residual source): the stash keeps xin, x1 and xout
        GemmArgs g = gemm_dense(ao, W + h->w16_out(l), x1, P + o.out_b, rows, d, d);
        g.aux = xin;
        if (leaf_gemm(g, dt, EPI_RESID_F32, s)) return 1;
        LEAF_TRY(leaf_launch_layernorm(x1, P + o.ln2_w, P + o.ln2_b, cf.ln_eps, xn2, rows, d, dt, s));
        g = gemm_dense(xn2, W + h->w16_fc(l), hh, P + o.fc_b, rows, 4 * d, d);
        g.aux = pre; g.act = cf.activation;
        if (leaf_gemm(g, dt, EPI_ACT_T, s)) return 1;
        g = gemm_dense(hh, W + h->w16_proj(l), xout, P + o.proj_b, rows, d, 4 * d);
        g.aux = x1;
        if (leaf_gemm(g, dt, EPI_RESID_F32, s)) return 1;
    }
    if (leaf_project_rows_ok(d, cf.embed_dim) && ws && ws_bytes >= (size_t)n_seq * d * 4) {
        // pooled rows -> ws, ln_final -> st.pooled (the stash the backward reads), fp32 matrix-core projection -> out
        float* xg = (float*)ws;
        if (pool_last) LEAF_TRY(leaf_launch_last_positions(st.eot, n_seq, map, s));
        else LEAF_TRY(leaf_launch_eot_positions(tokens, st.eot, n_seq, map, s));
        LEAF_TRY(leaf_launch_gather_rows(st.xin + (size_t)L * rd, st.eot, xg, n_seq, map, d, s));
        LEAF_TRY(leaf_launch_project_rows(xg, P + h->lnf_w, P + h->lnf_b, cf.ln_eps, P + h->text_proj, st.pooled, out, n_seq, d,
                                          cf.embed_dim, 0, s));
    } else if (pool_last) {
        // the same pooled rows through the generic projection kernel, which then reads one row per sequence and leaves st.eot alone
        float* xg = (float*)ws;
        LEAF_TRY(leaf_launch_last_positions(st.eot, n_seq, map, s));
        LEAF_TRY(leaf_launch_gather_rows(st.xin + (size_t)L * rd, st.eot, xg, n_seq, map, d, s));
        LEAF_TRY(leaf_launch_pool_project(xg, tokens, P + h->lnf_w, P + h->lnf_b, cf.ln_eps, P + h->text_proj, out, st.pooled,
                                          nullptr, n_seq, map, d, cf.embed_dim, 0, s, 1));
    } else {
        LEAF_TRY(leaf_launch_pool_project(st.xin + (size_t)L * rd, tokens, P + h->lnf_w, P + h->lnf_b, cf.ln_eps,
                                          P + h->text_proj, out, st.pooled, st.eot, n_seq, map, d, cf.embed_dim, 0, s));
    }
    if (h->normalize_fare) LEAF_TRY(leaf_launch_normalize_rows(out, st.norms, n_seq, cf.embed_dim, s));   // utils_AT.py:319
    return 0;
}

// The backward through the stash (include/leaf_hip.h, leaf_backward_args) from the loss head a->head: TextFARE against an anchor (ref
// = anchor, scale = accum_scale, head_out = the loss, one float), the cosine head of text embedding inversion (ref = target, scale =
// loss_weight, head_out = cos [n_seq]) or a loss the caller computed itself (ref = dfeat = its d loss / d feat, scale = a factor on
// it).  One body for the parameter-gradient backward (G != null) and the input-gradient-only backward of the optional embedding-space
// PGD mode (G == null, d_embed != null: no weight / bias / LayerNorm / embedding-table gradients).  Every refusal comes before the
// first HIP call.
extern "C" int leaf_text_backward(leaf_text_t h, const leaf_backward_args* a) {
    if (!a || a->size != sizeof(*a)) { leaf_set_error("leaf_backward_args: size %u, this library's is %zu", a ? a->size : 0u, sizeof(*a)); return 1; }
    const float *P = a->params, *feat = a->feat;
    const int32_t *tokens = a->tokens, *seq_lens = a->seq_lens, *cu_rows = a->cu_rows;
    const int n_seq = a->n_seq, head = a->head;
    float *G = a->grads, *d_embed = a->d_embed;
    void* const* layer_events = a->layer_events;
    if (!h || !P || !a->w16_bwd || !tokens || !feat || !a->ref || !a->stash || (!G && !d_embed) || !a->ws || n_seq < 1) {
        leaf_set_error("null/invalid argument");
        return 1;
    }
    const bool outputs_ok = head == LEAF_HEAD_FARE     ? (G != nullptr) != (d_embed != nullptr) && (G || a->scale == 1.0f)
                          : head == LEAF_HEAD_COSINE   ? !G
                          : head == LEAF_HEAD_UPSTREAM;     // grads, d_embed or both
    if (!outputs_ok) {
        leaf_set_error("backward: head %d takes -- FARE: grads, or d_embed with scale 1; COSINE: d_embed only; UPSTREAM: either or both", head);
        return 1;
    }
    if (head == LEAF_HEAD_COSINE && h->normalize_fare) { leaf_set_error("backward: the cosine head needs option normalize_fare off"); return 1; }
    hipStream_t s = (hipStream_t)a->stream;
    if ((seq_lens == nullptr) != (cu_rows == nullptr)) { leaf_set_error("seq_lens (host) and cu_rows (device) go together"); return 1; }
    const leaf_text_cfg& cf = h->cfg;
    const int rows = (int)total_rows(h, seq_lens, n_seq);
    Carver cs((void*)a->stash, (size_t)-1);
    Stash st = carve_stash(h, cs, n_seq, rows);
    Carver cw(a->ws, a->ws_bytes);
    BwdBuf b = carve_bwd(h, cw, n_seq, rows);
    if (!cw.ok()) { leaf_set_error("workspace too small: need %zu bytes, have %zu", cw.off, cw.cap); return 1; }
    const RowMap map{cu_rows, 0, 0, cf.context_length, nullptr, nullptr, 1};
    const int d = cf.width, L = cf.layers, D = cf.embed_dim;
    const size_t rd = (size_t)rows * d;
    const int fk = h->fwd_dtype == LEAF_DTYPE_FP16 ? 1 : 0;  // source kind of stashed activations
    const int gk = h->grad_dtype == LEAF_DTYPE_FP16 ? 1 : 0;  // 16-bit kind of the gradient path (kind == LEAF_* dtype id)
    const float* inv_s = b.gscale + 1;
    const uint16_t* WT = (const uint16_t*)a->w16_bwd;

    if (head == LEAF_HEAD_COSINE)
        LEAF_TRY(leaf_launch_cos_loss(feat, a->ref, n_seq, D, a->scale, a->head_out, b.dout, b.gscale, gk == 1, s));
    else if (head == LEAF_HEAD_UPSTREAM)
        LEAF_TRY(leaf_launch_upstream_grad(a->ref, feat, n_seq, D, a->scale, b.dout, b.gscale, gk == 1, s,
                                           h->normalize_fare ? st.norms : nullptr, h->scaler));
    else
        LEAF_TRY(leaf_launch_fare_loss(feat, a->ref, n_seq, D, a->scale, a->head_out, b.dout, b.gscale, gk == 1, s,
                                       h->normalize_fare ? st.norms : nullptr, h->scaler));
    const bool sat_check = h->scaler && G && gk == 1;     // fp16 gradient path with a scaler attached (leaf_hip.h "gradient scaler")
    LEAF_TRY(hipMemsetAsync(b.dx, 0, rd * 4, s));
    LEAF_TRY(leaf_launch_pool_project_bwd(b.dout, st.pooled, st.xin + (size_t)L * rd, st.eot, P + h->lnf_w, P + h->lnf_b,
                                          cf.ln_eps, P + h->text_proj, b.dx, G ? G + h->text_proj : nullptr,
                                          G ? G + h->lnf_w : nullptr, G ? G + h->lnf_b : nullptr, b.gscale, n_seq, map, d, D,
                                          b.dxn /* free until the first dgrad */, s));
    LEAF_TRY(leaf_launch_cast16(b.dx, 2, b.dx16, gk, rd, s));

    const int ln_grid = leaf_ln_bwd_grid(rows, d);
    const size_t ln_stride = (size_t)ln_grid * 2 * d;      // floats per LayerNorm in b.lnpart
    for (int l = L - 1; l >= 0; --l) {
        const LayerOff& o = h->layer[l];
        const float* xin = st.xin + l * rd; const float* x1 = st.x1 + l * rd;
        const uint16_t* xn1 = st.xn1 + l * rd; const uint16_t* qkv = st.qkv + 3 * l * rd; const uint16_t* ao = st.ao + l * rd;
        const uint16_t* xn2 = st.xn2 + l * rd; const uint16_t* pre = st.pre + 4 * l * rd; const uint16_t* hh = st.hh + 4 * l * rd;
        // ---- MLP
        GemmArgs g = gemm_dense(b.dx16, WT + h->w16_proj(l), b.big16, nullptr, rows, 4 * d, d);
        g.aux = (void*)pre; g.aux_f16 = fk; g.act = cf.activation;
        if (leaf_gemm(g, gk, EPI_ACTGRAD_T, s)) return 1;
        if (leaf_gemm(gemm_dense(b.big16, WT + h->w16_fc(l), b.dxn, nullptr, rows, d, 4 * d), gk, EPI_STORE_F32, s)) return 1;
        LEAF_TRY(leaf_launch_layernorm_bwd(b.dxn, x1, P + o.ln2_w, cf.ln_eps, b.dx, b.dx16b, gk,
                                           G ? b.lnpart + (size_t)(2 * l + 1) * ln_stride : nullptr, rows, d, s));
        // ---- attention
        if (leaf_gemm(gemm_dense(b.dx16b, WT + h->w16_out(l), b.do16, nullptr, rows, d, d), gk, EPI_STORE_T, s)) return 1;
        LEAF_TRY(leaf_launch_attention_bwd(qkv, h->fwd_dtype, b.do16, b.dqkv, gk, n_seq, map, cf.heads, d, s));
        if (G) {
            // all four weight + bias gradients of the block in one launch (wgrad.hip); must run before ln1's backward
            // overwrites dx16, the dY of c_proj
            WgradArgs wa{};
            wa.p[0] = WgradProb{b.dx16, hh, G + o.proj_w, G + o.proj_b, d, 4 * d, d, 4 * d, 0, 0};
            wa.p[1] = WgradProb{b.big16, xn2, G + o.fc_w, G + o.fc_b, 4 * d, d, 4 * d, d, 0, 0};
            wa.p[2] = WgradProb{b.dx16b, ao, G + o.out_w, G + o.out_b, d, d, d, d, 0, 0};
            wa.p[3] = WgradProb{b.dqkv, xn1, G + o.qkv_w, G + o.qkv_b, 3 * d, d, 3 * d, d, 0, 0};
            wa.nprob = 4; wa.rows = rows; wa.alpha = inv_s;
            LEAF_TRY(leaf_launch_wgrad_group(wa, fk, gk, s));
        }
        if (sat_check) {
            // the five 16-bit gradient tensors of this block, before ln1's backward overwrites dx16
            const void* bufs[5] = {b.dx16, b.big16, b.dx16b, b.do16, b.dqkv};
            const size_t numel[5] = {rd, 4 * rd, rd, rd, 3 * rd};
            // poison target: the first element of the token-embedding gradient.  Everything that still touches it after this
            // launch only ADDS to it (the embedding scatter adds into it: NaN stays NaN), and it travels in the LAST bucket of the
            // data-parallel reduction (step.bucket_plan: offset 0, behind the last block's event), so no rank can ship a clean
            // element 0 before another rank's poison exists (tests/test_dp_gloo.py pins both facts)
            LEAF_TRY(leaf_launch_sat_check16(bufs, numel, 5, h->scaler, G + h->tok_emb, s));
        }
        if (leaf_gemm(gemm_dense(b.dqkv, WT + h->w16_qkv(l), b.dxn, nullptr, rows, d, 3 * d), gk, EPI_STORE_F32, s)) return 1;
        LEAF_TRY(leaf_launch_layernorm_bwd(b.dxn, xin, P + o.ln1_w, cf.ln_eps, b.dx, b.dx16, gk,
                                           G ? b.lnpart + (size_t)(2 * l) * ln_stride : nullptr, rows, d, s));
        // every gradient of block l is final here: the caller may start reducing this block's bucket (step.py)
        if (layer_events && layer_events[l]) LEAF_TRY(hipEventRecord((hipEvent_t)layer_events[l], s));
    }
    if (G) {
        // LayerNorm parameter gradients of all blocks: one reduction of the per-workgroup partials (LN_REDUCE_MAX per launch)
        for (int i0 = 0; i0 < 2 * L; i0 += LN_REDUCE_MAX) {
            LnReduceArgs ra{};
            ra.n = 2 * L - i0 < LN_REDUCE_MAX ? 2 * L - i0 : LN_REDUCE_MAX;
            ra.part = b.lnpart + (size_t)i0 * ln_stride; ra.grid = ln_grid; ra.d = d; ra.inv_s = inv_s;
            for (int i = 0; i < ra.n; ++i) {
                const LayerOff& o = h->layer[(i0 + i) >> 1];
                const bool second = (i0 + i) & 1;
                ra.dg[i] = G + (second ? o.ln2_w : o.ln1_w);
                ra.db[i] = G + (second ? o.ln2_b : o.ln1_b);
            }
            LEAF_TRY(leaf_launch_ln_param_reduce(ra, s));
        }
    }
    if (G) LEAF_TRY(leaf_launch_embed_bwd(b.dx, b.gscale, tokens, G + h->tok_emb, G + h->pos_emb, rows, n_seq, map, d, cf.vocab_size, s));
    if (d_embed) LEAF_TRY(leaf_launch_scale_copy(b.dx, inv_s, d_embed, rd, s));   // d loss / d (token embedding), un-scaled
    if (layer_events && layer_events[L]) LEAF_TRY(hipEventRecord((hipEvent_t)layer_events[L], s));
    return 0;
}

extern "C" int leaf_text_set_grad_scaler(leaf_text_t h, float* state) {
    if (!h) { leaf_set_error("null handle"); return 1; }
    if (state && h->tok_emb != 0) { leaf_set_error("gradient scaler: the poison element must be offset 0 of the flat buffer"); return 1; }
    h->scaler = state;
    return 0;
}

// the cosine head alone (kernel hook for the tests): dout [B, D], cos_out [B]; ws = 64 + 2 B floats
extern "C" int leaf_op_cosine_head(const float* feat, const float* target, int B, int D, float loss_weight, float* dout,
                                   float* cos_out, float* ws, leaf_stream_t s) {
    if (!feat || !target || !dout || !ws || B < 1 || D < 1) { leaf_set_error("null/invalid argument"); return 1; }
    return leaf_check(leaf_launch_cos_loss(feat, target, B, D, loss_weight, cos_out, dout, ws, 0, (hipStream_t)s), "cosine_head");
}

// ---- the launchers of leaf_text_backward one at a time, on the RowMap it builds (kernel hooks of tests/test_gpu_backward_rows.py): no
// logic of their own
extern "C" int leaf_op_pool_project_bwd(const float* dout, const float* pooled, const float* x, const int32_t* eot_idx, const float* g,
                                        float eps, const float* proj, float* dx, float* dproj, float* dg, float* db,
                                        const float* gscale, const int32_t* cu, int n_seq, int ctx, int d, int D, float* scratch,
                                        leaf_stream_t s) {
    if (!dout || !pooled || !x || !eot_idx || !g || !proj || !dx || !gscale || !scratch || n_seq < 1 || D < 1 ||
        (dg == nullptr) != (db == nullptr)) { leaf_set_error("null/invalid argument"); return 1; }
    return leaf_check(leaf_launch_pool_project_bwd(dout, pooled, x, eot_idx, g, nullptr, eps, proj, dx, dproj, dg, db, gscale, n_seq,
                                                   RowMap{cu, 0, 0, ctx, nullptr, nullptr, 1}, d, D, scratch, (hipStream_t)s),
                      "pool_project_bwd");
}

extern "C" int leaf_op_embed_bwd(const float* dx, const float* gscale, const int32_t* tokens, float* dtok, float* dpos,
                                 const int32_t* cu, int rows, int n_seq, int ctx, int d, int vocab, leaf_stream_t s) {
    if (!dx || !gscale || !tokens || !dtok || !dpos || rows < 1 || n_seq < 1 || ctx < 1 || d < 1 || vocab < 1) {
        leaf_set_error("null/invalid argument");
        return 1;
    }
    return leaf_check(leaf_launch_embed_bwd(dx, gscale, tokens, dtok, dpos, rows, n_seq, RowMap{cu, 0, 0, ctx, nullptr, nullptr, 1}, d,
                                            vocab, (hipStream_t)s), "embed_bwd");
}

// gscale_ws: 64 + 2 B floats, {S, 1/S} in front (as leaf_op_cosine_head); norms / scaler may be NULL
extern "C" int leaf_op_fare_loss(const float* feat, const float* anchor, const float* norms, const float* scaler, int B, int D,
                                 float scale, int use_scaling, float* loss, float* dout, float* gscale_ws, leaf_stream_t s) {
    if (!feat || !anchor || !gscale_ws || B < 1 || D < 1) { leaf_set_error("null/invalid argument"); return 1; }
    return leaf_check(leaf_launch_fare_loss(feat, anchor, B, D, scale, loss, dout, gscale_ws, use_scaling, (hipStream_t)s, norms, scaler),
                      "fare_loss");
}

// the upstream-gradient head alone (kernel hook for the tests): gscale_ws as leaf_op_fare_loss; feat / norms NULL = no normalisation
extern "C" int leaf_op_upstream_head(const float* dfeat, const float* feat, const float* norms, const float* scaler, int B, int D,
                                     float scale, int use_scaling, float* dout, float* gscale_ws, leaf_stream_t s) {
    if (!dfeat || !dout || !gscale_ws || B < 1 || D < 1 || (norms && !feat)) { leaf_set_error("upstream_head: null/invalid argument"); return 1; }
    if (D > 2048) { leaf_set_error("upstream_head: D = %d, at most 2048", D); return 1; }
    return leaf_check(leaf_launch_upstream_grad(dfeat, feat, B, D, scale, dout, gscale_ws, use_scaling, (hipStream_t)s, norms, scaler),
                      "upstream_head");
}

extern "C" int leaf_op_sat_check16(const void* const* bufs, const size_t* numel, int n, float* scaler, float* poison, leaf_stream_t s) {
    if (!bufs || !numel) { leaf_set_error("null/invalid argument"); return 1; }
    return leaf_check(leaf_launch_sat_check16(bufs, numel, n, scaler, poison, (hipStream_t)s), "sat_check16");
}

extern "C" int leaf_vocab_inv_norms(const float* table, int V, int d, float* inv_norm, leaf_stream_t s) {
    if (!table || !inv_norm || V < 1) { leaf_set_error("vocab_inv_norms: null/invalid argument"); return 1; }
    if (!leaf_nn_project_ok(d)) { leaf_set_error("vocab_inv_norms: d = %d must be a multiple of 4, at most 2048", d); return 1; }
    return leaf_check(leaf_launch_vocab_inv_norms(table, V, d, inv_norm, (hipStream_t)s), "vocab_inv_norms");
}

// sized for the lowest slab (16 table rows) so that it does not depend on d
extern "C" size_t leaf_nn_project_ws_bytes(int M, int V) {
    if (M < 1 || V < 1) return 0;
    return align_up((size_t)((V + 15) / 16) * (size_t)M * 8, 256);
}

extern "C" int leaf_nn_project(const float* q, int M, const float* table, const float* inv_norm, int V, int d, int32_t* ids,
                               float* cos, void* ws, size_t ws_bytes, leaf_stream_t s) {
    if (!q || !table || !inv_norm || !ids || !ws || M < 1 || V < 1) { leaf_set_error("nn_project: null/invalid argument"); return 1; }
    if (!leaf_nn_project_ok(d)) { leaf_set_error("nn_project: d = %d must be a multiple of 4, at most 2048", d); return 1; }
    const size_t need = (size_t)leaf_nn_project_slabs(V, d) * (size_t)M * 8;
    if (ws_bytes < need) { leaf_set_error("nn_project: workspace too small: need %zu bytes, have %zu", need, ws_bytes); return 1; }
    return leaf_check(leaf_launch_nn_project(q, M, table, inv_norm, V, d, ids, cos, ws, (hipStream_t)s), "nn_project");
}

extern "C" int leaf_pgd_step(float* delta, const float* grad, const int32_t* cu_rows, int n_seq, int ctx, int width,
                             float alpha, float eps, int norm, leaf_stream_t s_) {
    if (!delta || !grad || n_seq < 1 || ctx < 1 || (norm != 0 && norm != 2) || alpha < 0.f || eps < 0.f) {
        leaf_set_error("null/invalid argument (norm: 0 = linf, 2 = l2)");
        return 1;
    }
    const RowMap map{cu_rows, 0, 0, ctx, nullptr, nullptr, 1};
    return leaf_check(leaf_launch_pgd_step(delta, grad, n_seq, map, width, alpha, eps, norm == 2, (hipStream_t)s_), "pgd_step");
}

extern "C" int leaf_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n,
                               size_t n_decay, float lr, float beta1, float beta2, float eps, float wd, int step,
                               float grad_scale, leaf_stream_t s) {
    if (!params || !grads || !exp_avg || !exp_avg_sq) { leaf_set_error("null argument"); return 1; }
    return leaf_check(leaf_launch_adamw(params, grads, exp_avg, exp_avg_sq, n, n_decay, lr, beta1, beta2, eps, wd, step,
                                        grad_scale, (hipStream_t)s), "adamw");
}

extern "C" int leaf_clip_grads_inplace(float* grads, size_t n, float pre_scale, float max_norm, float* ws, leaf_stream_t s) {
    if (!grads || !ws || !(max_norm > 0.f) || !(pre_scale > 0.f)) { leaf_set_error("null/invalid argument"); return 1; }
    return leaf_check(leaf_launch_clip_inplace(grads, n, pre_scale, max_norm, ws, (hipStream_t)s), "clip_grads_inplace");
}

extern "C" int leaf_adamw_step_clip(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n,
                                    size_t n_decay, float lr, float beta1, float beta2, float eps, float wd, int step,
                                    float grad_scale, float max_norm, float* clip_ws, leaf_stream_t s) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !clip_ws || !(max_norm > 0.f)) { leaf_set_error("null/invalid argument"); return 1; }
    return leaf_check(leaf_launch_adamw(params, grads, exp_avg, exp_avg_sq, n, n_decay, lr, beta1, beta2, eps, wd, step,
                                        grad_scale, (hipStream_t)s, max_norm, clip_ws), "adamw_clip");
}
