// Driver of the forward-only passes (anchor encode, clean-caption K/V pass, scoring passes, fused first stage): one chunk of sequences
// through the layer stack (FwdPass), and the cut of a pass into chunks (forward_all).  Host orchestration only -- every device
// operation is a launch on the pass's stream.
#include "engine.h"

FwdBuf carve_fwd(const leaf_text* h, Carver& c, int cs) {
    const size_t rows = (size_t)cs * h->cfg.context_length, d = h->cfg.width;
    FwdBuf b;
    b.x = (float*)c.take(rows * d * 4);
    b.a = (uint16_t*)c.take(rows * d * 2);
    b.qkv = (uint16_t*)c.take(rows * 3 * d * 2);
    b.hh = (uint16_t*)c.take(rows * 4 * d * 2);
    b.eot = (int32_t*)c.take(rows * 4);   // one per sequence; a sequence has >= 1 row
    b.x16 = (uint16_t*)c.take(rows * d * 2);
    b.stat = (float2*)c.take(rows * (d / 64) * 8);
    b.rowstat = (float2*)c.take(rows * 8);
    b.tile_seq = (int32_t*)c.take((rows + 2) * 8);
    return b;
}

size_t fwd_chunk_bytes(const leaf_text* h, int cs) {
    Carver c(nullptr, 0);
    carve_fwd(h, c, cs);
    return align_up(c.off, 256);
}

QkvAttnArgs fill_qkv_attn_args(const QkvOperands& q, const float2* rowstat, void* out, const void* kv_base, const int32_t* eot_pos,
                               const int32_t* tile_seq, const RowMap& map, int M, int n_seq, int n_tiles, int heads, int d, int max_len) {
    QkvAttnArgs qa;
    qa.A = q.A; qa.B = q.B; qa.bias = q.bias; qa.ln_s = q.ln_s; qa.K = qa.lda = qa.ldb = q.K;
    qa.rowstat = rowstat; qa.out = out; qa.kv_base = kv_base; qa.eot_pos = eot_pos; qa.tile_seq = tile_seq;
    qa.map = map; qa.M = M; qa.n_seq = n_seq; qa.n_tiles = n_tiles; qa.heads = heads; qa.d = d; qa.kv_ld = 3 * d;
    leaf_qkv_attn_lds_plan(max_len, &qa.ncap, &qa.caprows);
    return qa;
}

namespace {

// Where a residual GEMM adds: `m` rows of the residual stream in the pass's format -- fp32 rows x, or the 16 + 8-bit pair (x16,
// remainder bytes x) -- with the 16-bit copy x16 and the statistics (row stride stat_ld in the chunk's statistics buffer) that a
// following LayerNorm-folded GEMM reads.  The full rows of the chunk, or the pooled rows of a trimmed last block.
struct Resid {
    void* x;
    uint16_t* x16;
    int m, stat_ld;
};

// pooled rows (one per sequence) in scratch: the residual rows in the stream's format, the MLP hidden rows hb [cs, 4d], and the fp32
// rows xg the final LayerNorm + projection read with their [cs, d] fp32 scratch xn
struct Pooled {
    Resid r;
    uint16_t* hb;
    float *xg, *xn;
};

struct FwdPass {
    const leaf_text* h;
    const float* P;          // fp32 parameters
    const uint16_t* W;       // 16-bit forward pack
    const int32_t* tokens;
    const int cs, rows;      // sequences and packed rows of the chunk
    const RowMap map;
    float* const out;        // [cs, D] features; null = K/V-only pass: the last block stops behind its q|k|v rows (a hidden pass
                             // without features: it stops behind the highest tapped block)
    const int normalize;
    const FwdBuf b;
    const hipStream_t s;
    const KvPlan kv;
    const int max_len;
    const HiddenTaps* const taps;   // hidden states for the caller (leaf_text_forward_hidden), or null
    const leaf_text_cfg& c;
    const int d, dt;
    // ---- modes, fixed for the pass
    const bool fold;       // option ln_fold: LayerNorm folded into the GEMM epilogues (lnfold.h), else LayerNorm kernels
    const bool splits;     // leaf_text_split_pack_masks: hi + lo operand splits for the masked GEMMs of the leading blocks (LN-folded only)
    const bool lo8;        // option compact_resid, LN-folded, width the fp32 projection takes: residual stream in 16 + 8 bits (b.x16, b.x)
    const bool edit;       // option single_edit on a packed LN-folded prefix pass with a cache to read: block 0 projects one row per sequence
    const bool trim_last;  // option last_layer_trim, rows not produced into a cache or handed to the caller: last block on the pooled rows only

    FwdPass(const leaf_text* h_, const float* P_, const uint16_t* W_, const int32_t* tokens_, int cs_, int rows_, const RowMap& map_,
            float* out_, int normalize_, const FwdBuf& b_, hipStream_t s_, const KvPlan& kv_, int max_len_, const HiddenTaps* taps_)
        : h(h_), P(P_), W(W_), tokens(tokens_), cs(cs_), rows(rows_), map(map_), out(out_), normalize(normalize_), b(b_), s(s_), kv(kv_),
          max_len(max_len_), taps(taps_), c(h_->cfg), d(c.width), dt(h_->fwd_dtype),
          fold(h->ln_fold != 0),
          splits(fold && h->split_buf && h->split_blocks > 0),
          lo8(fold && h->compact_resid && leaf_project_rows_ok(d, c.embed_dim)),
          edit(h->single_edit && fold && map.cu && map.prefix && map.base_cu && c.layers > 1 && !kv.kv_write &&
               (kv.kv_read || (kv.kv_copy && kv.kv_self_rows))),
          trim_last(h->last_trim && !kv.kv_write && !(taps && taps->top() == c.layers)) {}

    bool sq(int l) const { return splits && h->split_qkv(l); }   // block l's QKV product runs on [hi | lo | hi] rows over K = 3d
    Resid full() const { return Resid{b.x, b.x16, rows, rows}; }

    // ---- borrowed buffers: who lends, and why it is dead at that point
    // Single-edit block 0: the [cs, 3d] table of fresh q|k|v rows lives in the hidden buffer, which nothing touches before block 0's c_fc.
    uint16_t* fresh_rows() const { return b.hh; }
    // ... and the pooled-position buffer, unused before the last block, holds the row map cu = 0, 1, 2, .. of those fresh rows.
    int32_t* iota_cu() const { return b.eot; }
    // [hi | lo | hi] copy of the residual rows in front of a split QKV product: the hidden buffer (dead between a block's c_proj and the
    // next c_fc).  Single-edit block 0 keeps its table there and writes no q|k|v rows, so its copies go to the q|k|v buffer.
    uint16_t* split_copy_qkv(int l) const { return edit && l == 0 ? b.qkv : b.hh; }
    // The chunk's OWN q|k|v buffer is dead behind a block's attention (and never written at all by the fused launch, or when the rows
    // go straight into the caller's cache): the [hi | lo | hi] copy in front of a split c_fc and the [A | A] copy of a split
    // out-projection's operand live there.
    uint16_t* dead_qkv() const { return b.qkv; }
    // Pooled rows: behind the last block's attention and the gather, the q|k|v and hidden buffers (carved back to back, 14 d rows bytes)
    // are dead.  fp32 stream: xg [cs, d] fp32 | hb [cs, 4d] 16-bit = 12 d cs bytes; xn takes hb's place once c_proj has consumed it.
    // With folding the chunk's x16 / statistics buffers (dead after the last QKV product) take the pooled rows' copy and statistics.
    Pooled pooled_f32() const {
        Pooled p;
        p.xg = (float*)b.qkv;
        p.hb = (uint16_t*)((char*)b.qkv + align_up((size_t)cs * d * 4, 256));
        p.xn = (float*)p.hb;
        p.r = Resid{p.xg, b.x16, cs, cs};
        return p;
    }
    // 16 + 8-bit stream: the pooled rows stay in that format through the block (the same EPI_RESID_LN8 arithmetic as the untrimmed
    // pass: bit-identical), [x16 rows | remainder rows | hidden rows] = 11 d cs bytes; the fp32 rows the final LayerNorm + projection
    // read are decoded into the hidden rows' space once c_proj has consumed them.
    Pooled pooled_lo8() const {
        Pooled p;
        uint16_t* g16 = b.qkv;
        unsigned char* g8 = (unsigned char*)b.qkv + align_up((size_t)cs * d * 2, 256);
        p.hb = (uint16_t*)(g8 + align_up((size_t)cs * d, 256));
        p.xg = (float*)p.hb;
        p.xn = p.xg + (size_t)cs * d;
        p.r = Resid{g8, g16, cs, cs};
        return p;
    }

    int ln_finalize(int stat_ld, int m) const {
        return leaf_check(leaf_launch_ln_finalize(b.stat, stat_ld, m, d / 64, c.ln_eps, b.rowstat, s), "ln_finalize");
    }
    // [hi | lo | hi] copy of the rows of `r` for a three-pass GEMM (block 0's QKV operand comes out of the embedding kernel instead:
    // the exact fp32 sum is in its registers)
    int split_rows(const Resid& r, void* dst) const {
        return lo8 ? leaf_check(leaf_launch_split16_rows_lo8(r.x16, r.x, dst, r.m, d, dt, s), "split16_rows_lo8")
                   : leaf_check(leaf_launch_split16_rows((const float*)r.x, dst, r.m, d, dt, s), "split16_rows");
    }

    // ---- embedding: x = tok_emb + pos_emb, and what block 0's QKV product reads of it
    // Single-edit pass: the one row per sequence the caption does not have -- (token, position) at its prefix length -- through a
    // derived row map with one row per sequence, and its q|k|v row into the table.  The chunk's buffers serve as scratch: the
    // full-row embedding that follows overwrites them.
    int embed_fresh_rows() const {
        LEAF_TRY(leaf_launch_iota(iota_cu(), cs, s));
        const RowMap one{iota_cu(), 0, 0, map.ctx, map.prefix + map.s0, nullptr, 1, 0};
        LEAF_TRY(leaf_launch_embed_fold(tokens + (size_t)map.s0 * map.ctx, P + h->tok_emb, P + h->pos_emb, b.x, b.x16, b.stat, cs, cs, cs,
                                        one, d, c.vocab_size, dt, s, nullptr, lo8, sq(0) ? split_copy_qkv(0) : nullptr));
        if (ln_finalize(cs, cs)) return 1;
        return qkv_gemm(0, cs, fresh_rows());
    }
    int embed() const {
        if (!fold) {
            const LayerOff& o0 = h->layer[0];
            LEAF_TRY(leaf_launch_embed_ln(tokens, P + h->tok_emb, P + h->pos_emb, P + o0.ln1_w, P + o0.ln1_b, c.ln_eps, b.x, b.a, rows, cs,
                                          map, d, c.vocab_size, dt, s));
            return 0;
        }
        if (edit && embed_fresh_rows()) return 1;
        // (single-edit pass: nothing multiplies the [hi | lo | hi] copy of ALL rows -- 6 d bytes per row written and read once)
        LEAF_TRY(leaf_launch_embed_fold(tokens, P + h->tok_emb, P + h->pos_emb, b.x, b.x16, b.stat, rows, rows, cs, map, d, c.vocab_size,
                                        dt, s, nullptr, lo8, sq(0) && !edit ? split_copy_qkv(0) : nullptr));
        if (ln_finalize(rows, rows)) return 1;
        // ... except the captions' rows of a fused first stage (the first rows of the chunk), whose q|k|v GEMM into the cache wants it:
        // the same kernel over those rows alone (identical values for what it writes twice)
        if (edit && sq(0) && kv.kv_self_rows)
            LEAF_TRY(leaf_launch_embed_fold(tokens, P + h->tok_emb, P + h->pos_emb, b.x, b.x16, b.stat, rows, (int)kv.kv_self_rows,
                                            map.group_off, map, d, c.vocab_size, dt, s, nullptr, lo8, split_copy_qkv(0)));
        return 0;
    }

    // ---- QKV
    QkvOperands qkv_operands(int l) const {
        if (!fold) return QkvOperands{b.a, W + h->w16_qkv(l), nullptr, P + h->layer[l].qkv_b, d};
        if (sq(l)) return QkvOperands{split_copy_qkv(l), h->split_qkv3(l), h->split_s_qkv(l), h->fold_c_qkv(W, l), 3 * d};
        return QkvOperands{b.x16, W + h->w16_fold_qkv(l), h->fold_s_qkv(W, l), h->fold_c_qkv(W, l), d};
    }
    // columns [col0, 3d) of block l's q|k|v rows for the chunk's first m rows -> dst [m, 3d]
    int qkv_gemm(int l, int m, uint16_t* dst, int col0 = 0) const {
        const QkvOperands q = qkv_operands(l);
        GemmArgs g = gemm_dense(q.A, q.B + (size_t)col0 * q.K, dst + col0, q.bias + col0, m, 3 * d - col0, q.K);
        g.ldc = 3 * d;
        if (fold) { g.ln_s = q.ln_s + col0; g.rowstat = b.rowstat; }
        return leaf_gemm(g, dt, fold ? EPI_LNFOLD_T : EPI_STORE_T, s);
    }

    // ---- q|k|v and attention of block l -> b.a (attention output of all rows; pooled: of one row per sequence, positions in b.eot).
    // stop: K/V-only pass, last block -- nothing consumes the attention
    int attention_stage(int l, bool pooled, bool stop) const {
        // where this block's q|k|v rows go: the chunk's buffer, or straight into the caller's cache
        uint16_t* qkv = kv.kv_write ? kv.kv_write + (size_t)l * kv.kv_stride : b.qkv;
        const void* kvl = kv.kv_read ? kv.kv_read + (size_t)l * kv.kv_stride : nullptr;     // cached prefix K/V the attention reads
        if (sq(l) && l > 0 && split_rows(full(), split_copy_qkv(l))) return 1;
        if (edit && l == 0) {
            // single-edit lookup: every row but the fresh one comes out of layer 0 of the captions' cache.  Fused first stage: the
            // captions' WHOLE q|k|v rows go there first (their own attention reads its Q from there too)
            if (kv.kv_self_rows) {
                if (qkv_gemm(l, (int)kv.kv_self_rows, kv.kv_copy)) return 1;
                kvl = kv.kv_copy;
            }
            LEAF_TRY(leaf_launch_attention_fwd(fresh_rows(), kvl, b.a, cs, map, c.heads, d, dt, s, nullptr, max_len, 1));
            return 0;
        }
        // QKV GEMM -> attention in one launch (qkv_attn.hip): q|k|v stay on chip.  A split QKV block goes through it when it takes
        // K = 3d, else as QKV GEMM + attention kernel
        if (kv.attn_tiles > 0 && (!sq(l) || leaf_qkv_attn_eligible(d, c.heads, c.context_length, 3 * d, kv.attn_max_len))) {
            if (kv.kv_self_rows) {
                // fused first stage: the captions' rows -- which their candidates' attention reads as cached prefix and the second stage
                // reads again -- come from a small GEMM of their own straight into the cache (the same bits as from any other kernel).
                // Only the K and V thirds: nothing ever reads a caption's q rows from the cache (its own attention runs inside the
                // fused launch, from LDS) -- weight rows [d, 3d) into cache columns [d, 3d) of the [rows, 3d] layout
                uint16_t* dst = kv.kv_copy + (size_t)l * kv.kv_stride;
                if (qkv_gemm(l, (int)kv.kv_self_rows, dst, d)) return 1;
                kvl = dst;
            }
            if (stop) return 0;
            if (pooled) LEAF_TRY(leaf_launch_eot_positions(tokens, b.eot, cs, map, s));
            const QkvAttnArgs qa = fill_qkv_attn_args(qkv_operands(l), b.rowstat, b.a, kvl, pooled ? b.eot : nullptr, b.tile_seq, map, rows,
                                                      cs, kv.attn_tiles, c.heads, d, kv.attn_max_len);
            return leaf_qkv_attn(qa, dt, s);
        }
        if (qkv_gemm(l, rows, qkv)) return 1;
        if (kv.kv_self_rows) {     // fused first stage on two kernels: the captions' rows are read in place and copied to the cache
            kvl = qkv;
            LEAF_TRY(leaf_launch_copy_bytes(qkv, kv.kv_copy + (size_t)l * kv.kv_stride, (size_t)kv.kv_self_rows * 3 * d * 2, s));
        }
        if (stop) return 0;
        if (pooled) LEAF_TRY(leaf_launch_eot_positions(tokens, b.eot, cs, map, s));
        LEAF_TRY(leaf_launch_attention_fwd(qkv, kvl, b.a, cs, map, c.heads, d, dt, s, pooled ? b.eot : nullptr, max_len));
        return 0;
    }

    // ---- x += A W^T + bias on the rows of `r` (Wt = [d][K] 16-bit weights).  ln_next: a LayerNorm reads the result -- with folding the
    // GEMM also emits x16 / statistics and the tiny finalize launch turns the [group][row] partials into (mean, rstd) per row for the
    // consuming GEMM.  (The 16 + 8-bit stream has one epilogue: it emits them all the same, unread and not finalized.)
    // w_lo (split c_proj): A is a stored 16-bit tensor (exact as it is), so only the weights are split: x += A W_hi^T + bias, then
    // x += A W_lo^T in a second launch, which is the one whose x16 / statistics of the finished rows are read.
    // a_twice (split out-projection): Wt = [W_hi | W_lo] [d][2K] and x += [A | A] Wt^T + bias in ONE launch (the stream is
    // read-modify-written once).  The half-stage ring kernel re-reads A itself (GemmArgs::a_wrap); launches too small for it multiply a
    // duplicated copy of A -- the same operands in the same k order, so a row's bits do not depend on which of the two ran.
    int residual_add(const void* A, int K, const uint16_t* Wt, const float* bias, const Resid& r, bool ln_next,
                     const uint16_t* w_lo = nullptr, bool a_twice = false) const {
        const int epi = lo8 ? EPI_RESID_LN8 : (fold && ln_next) ? EPI_RESID_LN : EPI_RESID_F32;
        GemmArgs g = gemm_dense(A, Wt, r.x, bias, r.m, d, K);
        if (epi != EPI_RESID_F32) { g.x16 = r.x16; g.ldx16 = d; g.stat_out = b.stat; g.stat_ld = r.stat_ld; g.ln_eps = c.ln_eps; }
        if (w_lo) {
            if (leaf_gemm(g, dt, lo8 ? EPI_RESID_LN8 : EPI_RESID_F32, s)) return 1;
            g.B = w_lo; g.bias = nullptr;
        }
        if (a_twice) {
            g.K = g.ldb = 2 * K; g.a_wrap = K / 64;
            if (K % 64 || leaf_gemm_family(g, epi) != 4) {      // not the ring kernel's launch
                LEAF_TRY(leaf_launch_dup_cols16(A, dead_qkv(), r.m, K, s));
                g.A = dead_qkv(); g.lda = 2 * K; g.a_wrap = 0;
            }
        }
        if (leaf_gemm(g, dt, epi, s)) return 1;
        return epi != EPI_RESID_F32 && ln_next ? ln_finalize(r.stat_ld, r.m) : 0;
    }

    // c_fc: hid = act(LN2(rows of r) W^T + bias)
    int fc_gemm(int l, const Resid& r, uint16_t* hid) const {
        GemmArgs g = gemm_dense(b.a, W + h->w16_fc(l), hid, P + h->layer[l].fc_b, r.m, 4 * d, d);
        g.act = c.activation;
        if (!fold) return leaf_gemm(g, dt, EPI_ACT_T, s);
        g.A = r.x16; g.B = W + h->w16_fold_fc(l); g.bias = h->fold_c_fc(W, l); g.ln_s = h->fold_s_fc(W, l); g.rowstat = b.rowstat;
        if (splits && h->split_fc(l)) {
            if (split_rows(r, dead_qkv())) return 1;
            g.A = dead_qkv(); g.B = h->split_fc3(l); g.ln_s = h->split_s_fc(l); g.K = g.lda = g.ldb = 3 * d;
        }
        return leaf_gemm(g, dt, EPI_LNFOLD_ACT_T, s);
    }

    // ---- behind the attention (b.a): out_proj -> (LayerNorm kernel when not folded) -> c_fc -> c_proj on the rows of `r`
    int block_tail(int l, const Resid& r, uint16_t* hid, bool ln_after) const {
        const LayerOff& o = h->layer[l];
        const bool out2 = splits && h->split_out(l);
        if (residual_add(b.a, d, out2 ? h->split_out2(l) : W + h->w16_out(l), P + o.out_b, r, true, nullptr, out2)) return 1;
        if (!fold) LEAF_TRY(leaf_launch_layernorm((const float*)r.x, P + o.ln2_w, P + o.ln2_b, c.ln_eps, b.a, r.m, d, dt, s));
        if (fc_gemm(l, r, hid)) return 1;
        return residual_add(hid, 4 * d, W + h->w16_proj(l), P + o.proj_b, r, ln_after, splits && h->split_proj(l) ? h->split_proj_lo(l) : nullptr);
    }

    // ---- pooled rows (positions in b.eot) of the chunk's stream -> p: in the stream's format (a block tail follows), or decoded to fp32
    int gather_pooled(const Pooled& p, bool decode) const {
        if (!lo8) LEAF_TRY(leaf_launch_gather_rows(b.x, b.eot, p.xg, cs, map, d, s));
        else if (decode) LEAF_TRY(leaf_launch_gather_rows_lo8(b.x16, b.x, b.eot, p.xg, cs, map, d, dt, s));
        else LEAF_TRY(leaf_launch_gather_rows_pair(b.x16, b.x, b.eot, p.r.x16, (unsigned char*)p.r.x, cs, map, d, s));
        return 0;
    }
    // final LayerNorm + projection of fp32 rows x -- the pooled rows (xn = their scratch), or for the fall-back kernel also the chunk's
    // full rows, which it pools itself
    int project(const float* x, bool rows_are_pooled, float* xn) const {
        if (leaf_project_rows_ok(d, c.embed_dim))
            LEAF_TRY(leaf_launch_project_rows(x, P + h->lnf_w, P + h->lnf_b, c.ln_eps, P + h->text_proj, xn, out, cs, d, c.embed_dim, normalize, s));
        else
            LEAF_TRY(leaf_launch_pool_project(x, tokens, P + h->lnf_w, P + h->lnf_b, c.ln_eps, P + h->text_proj, out, nullptr, nullptr, cs,
                                              map, d, c.embed_dim, normalize, s, rows_are_pooled ? 1 : 0));
        return 0;
    }
    // Trimmed last block: only the pooled row (first maximum token id = EOT) of each sequence reaches the output, and every op behind
    // the attention is row-wise, so out-projection, LN2 and the MLP run on ONE row per sequence (bit-identical)
    int pooled_tail_and_project(int l) const {
        const Pooled p = lo8 ? pooled_lo8() : pooled_f32();
        if (gather_pooled(p, false)) return 1;
        if (block_tail(l, p.r, p.hb, false)) return 1;
        if (lo8) LEAF_TRY(leaf_launch_resid_unpack(p.r.x16, p.r.x, p.xg, (size_t)cs * d, dt, s));
        return project(p.xg, true, p.xn);
    }
    // Untrimmed: the same op sequence on the finished rows (bit-identical features): gather the pooled rows, LN, fp32 projection
    int pool_and_project() const {
        if (!leaf_project_rows_ok(d, c.embed_dim)) return project(b.x, false, nullptr);
        const Pooled p = pooled_f32();
        LEAF_TRY(leaf_launch_eot_positions(tokens, b.eot, cs, map, s));
        if (gather_pooled(p, true)) return 1;
        return project(p.xg, true, p.xn);
    }

    // ---- hidden states for the caller: the full rows of the stream as they stand behind `layer` blocks (HF's hidden_states index)
    // -> every tap of that index, the chunk's sequences at their place in the tap's [n_seq, ctx, d]
    int tap_rows(int layer) const {
        for (int i = 0; taps && i < taps->n; ++i) {
            const leaf_hidden_tap& t = taps->t[i];
            if (t.layer != layer) continue;
            char* dst = (char*)t.out + (size_t)map.s0 * c.context_length * d * (taps->out16 ? 2 : 4);
            LEAF_TRY(leaf_launch_hidden_rows(b.x, lo8 ? b.x16 : nullptr, P + h->lnf_w, P + h->lnf_b, c.ln_eps, t.final_ln, dst, taps->out16,
                                             cs, map, d, dt, s));
        }
        return 0;
    }

    int run() const {
        const bool kv_only = !out && !taps;                     // clean captions for the cache
        const int stop = !out && taps ? taps->top() : -1;       // hidden pass without features: nothing consumes the blocks behind
        if (embed()) return 1;
        if (tap_rows(0)) return 1;
        if (stop == 0) return 0;
        for (int l = 0; l < c.layers; ++l) {
            const LayerOff& o = h->layer[l];
            const bool last = l == c.layers - 1;
            if (l > 0 && !fold) LEAF_TRY(leaf_launch_layernorm(b.x, P + o.ln1_w, P + o.ln1_b, c.ln_eps, b.a, rows, d, dt, s));
            if (attention_stage(l, last && trim_last, last && kv_only)) return 1;
            if (last && kv_only) return 0;          // K/V-only pass: nothing consumes the rest
            if (last && trim_last) return pooled_tail_and_project(l);
            if (block_tail(l, full(), b.hh, !last)) return 1;      // (ln_final runs on the pooled rows)
            if (tap_rows(l + 1)) return 1;
            if (stop == l + 1) return 0;
        }
        return pool_and_project();
    }
};

// Fused QKV + attention for the big passes: cut the chunk's sequences [s0, s1) into M tiles of whole sequences on the host and send the
// cut points to tile_seq behind the work already queued on `s` (a pinned ring slot; its event keeps a slot from being rewritten early)
int plan_attn_tiles(leaf_text* h, const int32_t* lens, int s0, int s1, const PrefixPlan& pp, int max_len, int32_t* tile_seq, hipStream_t s,
                    KvPlan& kv) {
    const size_t need = 2 * ((size_t)(s1 - s0) + 2);
    if (h->plan_cap < need) {
        for (int i = 0; i < leaf_text::PLAN_RING; ++i) {
            if (h->plan_ev[i]) LEAF_TRY(hipEventSynchronize(h->plan_ev[i]));
            if (h->plan_host[i]) { LEAF_TRY(hipHostFree(h->plan_host[i])); h->plan_host[i] = nullptr; }
        }
        h->plan_cap = need * 2;
    }
    const int k = h->plan_next;
    h->plan_next = (k + 1) % leaf_text::PLAN_RING;
    if (!h->plan_host[k]) LEAF_TRY(hipHostMalloc((void**)&h->plan_host[k], h->plan_cap * sizeof(int32_t), hipHostMallocDefault));
    if (!h->plan_ev[k]) LEAF_TRY(hipEventCreateWithFlags(&h->plan_ev[k], hipEventDisableTiming));
    else LEAF_TRY(hipEventSynchronize(h->plan_ev[k]));
    kv.attn_tiles = leaf_qkv_attn_plan(lens ? lens + s0 : nullptr, h->cfg.context_length, s0, s1 - s0, pp.prefix_dev != nullptr, pp.group,
                                       pp.group_off, leaf_qkv_attn_tile_rows(), leaf_qkv_attn_ncap(max_len), h->plan_host[k]);
    kv.attn_max_len = max_len;
    LEAF_TRY(hipMemcpyAsync(tile_seq, h->plan_host[k], (size_t)(kv.attn_tiles + 1) * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    LEAF_TRY(hipEventRecord(h->plan_ev[k], s));
    return 0;
}

}  // namespace

int forward_chunk(const leaf_text* h, const float* P, const uint16_t* W, const int32_t* tokens, int cs, int rows, RowMap map,
                  float* out, int normalize, const FwdBuf& b, hipStream_t s, const KvPlan& kv, int max_len, const HiddenTaps* taps) {
    return FwdPass(h, P, W, tokens, cs, rows, map, out, normalize, b, s, kv, max_len, taps).run();
}

// Sequences are processed in chunks bounded by a ROW budget (chunk * ctx rows): with EOT-trimmed (packed) rows a
// chunk holds more sequences, so the GEMMs keep their M.  lens == nullptr -> dense (every sequence ctx rows).
int forward_all(leaf_text* h, const float* P, const void* W, const int32_t* tokens, const int32_t* lens, const int32_t* cu_dev,
                int n_seq, float* out, int normalize, Carver& c, hipStream_t s, const PrefixPlan& pp, const HiddenTaps* taps) {
    const int ctx = h->cfg.context_length;
    if ((lens == nullptr) != (cu_dev == nullptr)) { leaf_set_error("seq_lens (host) and cu_rows (device) go together"); return 1; }
    const size_t budget = (size_t)(n_seq < h->chunk ? n_seq : h->chunk) * ctx;
    size_t total = 0;
    int max_len = 0;
    for (int i = 0; i < n_seq; ++i) {
        const int L = lens ? lens[i] : ctx;
        if (L < 1 || L > ctx) { leaf_set_error("seq_lens[%d] = %d out of range 1..%d", i, L, ctx); return 1; }
        total += L;
        max_len = L > max_len ? L : max_len;
    }
    if (pp.prefix_dev) {   // computed rows are suffixes: the bound comes from the caller
        if (pp.max_len > 0 && pp.max_len < max_len) { leaf_set_error("max_len %d below a suffix length %d", pp.max_len, max_len); return 1; }
        max_len = pp.max_len > 0 && pp.max_len <= ctx ? pp.max_len : ctx;
    }
    const size_t nchunks = (total + budget - 1) / budget;
    if (pp.kv_self_rows && nchunks > 1) { leaf_set_error("fused pass: the captions and their candidates must fit one chunk (%zu rows > %zu)", total, budget); return 2; }
    const size_t target = (total + nchunks - 1) / nchunks;           // <= budget
    const FwdBuf buf = carve_fwd(h, c, (int)(budget / ctx));
    if (!c.ok()) { leaf_set_error("workspace too small: need %zu bytes, have %zu", c.off, c.cap); return 1; }
    int s0 = 0;
    size_t row0 = 0;
    while (s0 < n_seq) {
        int s1 = s0;
        size_t rows = 0;
        while (s1 < n_seq) {
            const int L = lens ? lens[s1] : ctx;
            if (rows + L > target && s1 > s0) break;
            if (rows + L > budget) break;
            rows += L;
            ++s1;
        }
        RowMap map{cu_dev, s0, (int)row0, ctx, pp.prefix_dev, pp.base_cu_dev, pp.group, pp.group_off};
        KvPlan kv;
        kv.kv_read = pp.kv;
        kv.kv_stride = pp.kv_stride;
        kv.kv_copy = pp.kv_copy;
        kv.kv_self_rows = pp.kv_self_rows;
        if (s1 == s0) { leaf_set_error("a sequence does not fit the row budget"); return 1; }
        if (h->fuse_attn && h->ln_fold && leaf_qkv_attn_eligible(h->cfg.width, h->cfg.heads, ctx, h->cfg.width, max_len) &&
            rows / 256 * (size_t)h->cfg.heads >= 256 &&      // at least a chip's worth of (256-row tile, head) items
            plan_attn_tiles(h, lens, s0, s1, pp, max_len, buf.tile_seq, s, kv))
            return 1;
        if (forward_chunk(h, P, (const uint16_t*)W, tokens, s1 - s0, (int)rows, map, out ? out + (size_t)s0 * h->cfg.embed_dim : nullptr,
                          normalize, buf, s, kv, max_len, taps))
            return 1;
        s0 = s1;
        row0 += rows;
    }
    return 0;
}
