// Host-side handle shared by api.hip (C ABI: handle, packing, scoring), forward.hip (forward-only pass driver) and api_train.hip
// (training step).
#pragma once
#include <string>
#include <vector>

#include "../../include/leaf_hip.h"
#include "kernels.h"

struct TensorInfo {
    std::string name;
    size_t offset;
    int64_t rows, cols;  // cols == 0 -> 1-D
    size_t numel() const { return (size_t)rows * (cols ? cols : 1); }
};

struct LayerOff {  // offsets (floats) into the flat parameter buffer
    size_t ln1_w, ln1_b, qkv_w, qkv_b, out_w, out_b, ln2_w, ln2_b, fc_w, fc_b, proj_w, proj_b;
};

struct leaf_text {
    leaf_text_cfg cfg;
    int fwd_dtype;
    int chunk;  // sequences per pass
    int last_trim;   // last transformer block: attention output / out-proj / MLP only for the pooled (EOT) row
    int grad_dtype;  // 16-bit type of the gradient path: LEAF_F16 (loss-scaled, default) or LEAF_BF16
    int normalize_fare = 0;   // --normalize_fare: the training forward returns F.normalize(features), the backward follows
    float* scaler = nullptr;  // gradient-scaler state (device, leaf_hip.h LEAF_SC_*) or null: no saturation check, no back-off
    // QKV GEMM -> attention as one launch in the big forward-only passes (qkv_attn.hip); option 'fuse_attn' / LEAF_FUSE_ATTN=0
    // restores the two kernels around the [rows, 3d] buffer.  The M-tile plan of a pass (first sequence of every tile) is cut on
    // the host and travels through a small ring of pinned buffers (an event per slot guards its re-use).
    int fuse_attn = 1;
    // Single-edit scoring passes (option 'single_edit', include/leaf_hip.h): the caller promises that every candidate of the pass is
    // its caption with ONE token replaced at position prefix[i].  Block 0's q|k|v row depends on (token, position) alone, so only
    // that one row per candidate is projected; every other row is read from layer 0 of the captions' cache (forward.hip: embed_fresh_rows, attention_stage).
    int single_edit = 0;
    static constexpr int PLAN_RING = 8;
    int32_t* plan_host[PLAN_RING] = {};
    hipEvent_t plan_ev[PLAN_RING] = {};
    size_t plan_cap = 0;      // ints per slot
    int plan_next = 0;
    std::vector<TensorInfo> tensors;
    std::vector<LayerOff> layer;
    size_t tok_emb, pos_emb, text_proj, lnf_w, lnf_b;
    size_t n_params, n_decay;
    // element offsets into the 16-bit weight pack, per layer: qkv, out, fc, proj (12 d^2 per layer)
    size_t w16_layer_elems() const { return (size_t)12 * cfg.width * cfg.width; }
    size_t w16_qkv(int l) const { return l * w16_layer_elems(); }
    size_t w16_out(int l) const { return w16_qkv(l) + (size_t)3 * cfg.width * cfg.width; }
    size_t w16_fc(int l) const { return w16_out(l) + (size_t)cfg.width * cfg.width; }
    size_t w16_proj(int l) const { return w16_fc(l) + (size_t)4 * cfg.width * cfg.width; }
    // ---- LN folding (lnfold.h), forward-only passes.  The 16-bit forward pack continues behind the standard copies with the
    // gamma-scaled QKV and c_fc weights of every layer (7 d^2 per layer), followed (256-B aligned) by the fp32 vectors
    // s_qkv[3d], c_qkv[3d], s_fc[4d], c_fc[4d] per layer.
    int ln_fold = 1;          // option 'ln_fold' / LEAF_LN_FOLD=0: separate LayerNorm kernels instead
    // Residual stream of the LN-folded forward-only passes in 16 + 8 bits (common.h resid_lo4): the 16-bit copy the next GEMM
    // multiplies anyway + a remainder byte per element (block-scaled e4m3, common.h resid_lo4) instead of an fp32 row beside that copy -- the out-projection moves 8 d bytes
    // per row instead of 12 d, c_proj 14 d instead of 18 d.  Option 'compact_resid' / LEAF_COMPACT_RESID=0: fp32 rows (also what the
    // split blocks of leaf_text_split_pack_masks and widths the fp32 matrix-core projection does not take run on).
    int compact_resid = 1;
    size_t w16_std_elems() const { return w16_layer_elems() * cfg.layers; }
    size_t w16_fold_qkv(int l) const { return w16_std_elems() + (size_t)l * 7 * cfg.width * cfg.width; }
    size_t w16_fold_fc(int l) const { return w16_fold_qkv(l) + (size_t)3 * cfg.width * cfg.width; }
    size_t w16_aux_byte_off() const { return ((w16_std_elems() + (size_t)cfg.layers * 7 * cfg.width * cfg.width) * 2 + 255) / 256 * 256; }
    size_t w16_total_bytes() const { return w16_aux_byte_off() + (size_t)cfg.layers * 14 * cfg.width * 4; }
    // fp32 aux vectors of layer l inside a forward pack at `w16`
    const float* fold_aux(const void* w16, int l) const { return (const float*)((const char*)w16 + w16_aux_byte_off()) + (size_t)l * 14 * cfg.width; }
    const float* fold_s_qkv(const void* w16, int l) const { return fold_aux(w16, l); }
    const float* fold_c_qkv(const void* w16, int l) const { return fold_aux(w16, l) + 3 * cfg.width; }
    const float* fold_s_fc(const void* w16, int l) const { return fold_aux(w16, l) + 6 * cfg.width; }
    const float* fold_c_fc(const void* w16, int l) const { return fold_aux(w16, l) + 10 * cfg.width; }
    // ---- optional higher-precision leading blocks (leaf_text_split_pack_masks): hi + lo operand splits for the four GEMMs of blocks
    // [0, split_blocks) of the forward-only passes.  Caller-owned buffer: per block 27 d^2 16-bit elements -- QKV' [3d][3d] and
    // c_fc' [4d][3d] as [hi | hi | lo] of the gamma-scaled weights, out_proj as [hi | lo] [d][2d] (ONE launch against [A | A]:
    // GemmArgs::a_wrap), the lo half of c_proj [d][4d] (a second launch) -- then (256-B aligned) per block the fp32 row sums
    // s_qkv[3d], s_fc[4d] of hi + lo.
    int split_blocks = 0;
    const void* split_buf = nullptr;
    // WHICH GEMMs of those blocks run on splits: one mask per block (leaf_text_split_pack_masks), bit 0 = QKV (both operands, three
    // passes), bit 1 = out_proj (weights, two passes), bit 2 = c_fc (both operands), bit 3 = c_proj (weights).
    // profiles/r06_precision_budget_sites.txt and the census price the choices.
    int split_mask[64] = {};
    bool split_on(int l) const { return split_buf && l < split_blocks && l < 64; }
    bool split_qkv(int l) const { return split_on(l) && (split_mask[l] & 1); }
    bool split_out(int l) const { return split_on(l) && (split_mask[l] & 2); }
    bool split_fc(int l) const { return split_on(l) && (split_mask[l] & 4); }
    bool split_proj(int l) const { return split_on(l) && (split_mask[l] & 8); }
    size_t split_block_elems() const { return (size_t)27 * cfg.width * cfg.width; }
    size_t split_aux_byte_off(int n) const { return ((size_t)n * split_block_elems() * 2 + 255) / 256 * 256; }
    size_t split_bytes(int n) const { return split_aux_byte_off(n) + (size_t)n * 7 * cfg.width * 4; }
    const uint16_t* split_qkv3(int l) const { return (const uint16_t*)split_buf + (size_t)l * split_block_elems(); }
    const uint16_t* split_fc3(int l) const { return split_qkv3(l) + (size_t)9 * cfg.width * cfg.width; }
    const uint16_t* split_out2(int l) const { return split_fc3(l) + (size_t)12 * cfg.width * cfg.width; }
    const uint16_t* split_proj_lo(int l) const { return split_out2(l) + (size_t)2 * cfg.width * cfg.width; }
    const float* split_s_qkv(int l) const { return (const float*)((const char*)split_buf + split_aux_byte_off(split_blocks)) + (size_t)l * 7 * cfg.width; }
    const float* split_s_fc(int l) const { return split_s_qkv(l) + 3 * cfg.width; }
};

size_t leaf_train_ws_bytes(const leaf_text* h, int n_seq);  // api_train.hip
// GEMM launch shared by the host files (api.hip): checks the operands of the LN epilogues (EPI_LNFOLD_* consume rowstat / ln_s /
// bias, EPI_RESID_LN* produce x16 / stat_out); when the profiler is armed (leaf_prof_begin) each launch is bracketed by HIP
// events on its own stream and accounted under its epilogue id.
int leaf_gemm(const GemmArgs& g, int dtype, int epi, hipStream_t s);
// C[M,N] (+)= A[M,K] B[N,K]^T + bias on densely stored operands; everything optional stays at GemmArgs' defaults
inline GemmArgs gemm_dense(const void* A, const void* B, void* C, const float* bias, int M, int N, int K) {
    GemmArgs g;
    g.A = A; g.B = B; g.C = C; g.bias = bias;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N;
    return g;
}
int leaf_qkv_attn(const QkvAttnArgs& a, int dtype, hipStream_t s);   // leaf_launch_qkv_attn + profiler accounting
void leaf_set_error(const char* fmt, ...);
int leaf_check(hipError_t e, const char* what);

#define LEAF_TRY(expr)                                   \
    do {                                                 \
        int _rc = leaf_check((expr), #expr);             \
        if (_rc) return _rc;                             \
    } while (0)

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// bump allocator over a caller-provided workspace
struct Carver {
    char* base;
    size_t off, cap;
    Carver(void* p, size_t bytes) : base((char*)p), off(0), cap(bytes) {}
    void* take(size_t bytes) {
        size_t o = align_up(off, 256);
        off = o + bytes;
        return base ? base + o : nullptr;
    }
    bool ok() const { return off <= cap; }
};

// ------------------------------------------------------------------ forward-only pass driver (forward.hip)
struct FwdBuf {    // workspace of one chunk
    float* x;      // [rows,d] fp32 residual stream (16 + 8-bit stream: the [rows,d] remainder bytes)
    uint16_t* a;   // [rows,d]   LN output / attention output (aliased)
    uint16_t* qkv; // [rows,3d]
    uint16_t* hh;  // [rows,4d]
    int32_t* eot;  // [seqs] pooled position per sequence (last-layer trimming)
    uint16_t* x16; // [rows,d]   LN folding: 16-bit copy of the residual stream (A operand of the QKV / c_fc GEMMs)
    float2* stat;  // [d/64][rows] LN folding: (sum, M2) per row and 64-column group
    float2* rowstat; // [rows]     LN folding: (mean, rstd) per row
    int32_t* tile_seq; // [seqs + 1][2] fused QKV + attention: (first sequence, first row) of every M tile (a sequence has >= 1 row)
};
FwdBuf carve_fwd(const leaf_text* h, Carver& c, int cs);   // cs sequences of context_length rows
size_t fwd_chunk_bytes(const leaf_text* h, int cs);        // what carve_fwd takes

// who produces and who reads the per-layer q|k|v cache of the clean captions (stride kv_stride elements per layer)
struct KvPlan {
    uint16_t* kv_write = nullptr;       // the rows of this (single) chunk are produced INTO the cache (leaf_text_forward_kv)
    const uint16_t* kv_read = nullptr;  // prefix mode: attention reads the prefix K/V of layer l from kv_read + l * kv_stride
    size_t kv_stride = 0;
    // fused pass (leaf_score_pass with kv_write): the clean captions are the FIRST kv_self_rows rows of this chunk; the
    // candidates' attention reads their K/V from the chunk's own rows, and every layer's caption rows also go to kv_copy
    uint16_t* kv_copy = nullptr;
    size_t kv_self_rows = 0;
    // fused QKV + attention launches (qkv_attn.hip): number of M tiles cut for this chunk (FwdBuf::tile_seq holds them); 0 = two kernels
    int attn_tiles = 0;
    int attn_max_len = 0;     // longest sequence (prefix + computed rows) the plan was cut for: sizes the caption images
};
// Hidden-state taps of a pass (leaf_text_forward_hidden): `layer` is HF's hidden_states index -- 0 = the embedding, l = the output of
// block l - 1 -- and every tap's rows go to its out[n_seq, ctx, width] (fp32, or the handle's 16-bit type with out16), the sequences
// of a chunk at their place in it
struct HiddenTaps {
    const leaf_hidden_tap* t;
    int n, out16;
    int top() const {     // highest tapped index: a pass without a feature output stops behind block top - 1
        int m = -1;
        for (int i = 0; i < n; ++i) m = t[i].layer > m ? t[i].layer : m;
        return m;
    }
};
// the layer stack on one chunk of `cs` sequences (`rows` = their packed row count); features -> out [cs, D], or out == null:
// K/V-only pass.  max_len: longest sequence (prefix + computed rows); 0 = context_length
// taps (may be null): hidden states for the caller; with them out == null means "no features": the pass stops behind the highest
// tapped block
int forward_chunk(const leaf_text* h, const float* P, const uint16_t* W, const int32_t* tokens, int cs, int rows, RowMap map,
                  float* out, int normalize, const FwdBuf& b, hipStream_t s, const KvPlan& kv, int max_len, const HiddenTaps* taps = nullptr);

struct PrefixPlan {   // prefix reuse: see RowMap in common.h
    const int32_t* prefix_dev = nullptr;
    const int32_t* base_cu_dev = nullptr;
    const uint16_t* kv = nullptr;
    size_t kv_stride = 0;
    int group = 1;
    int max_len = 0;   // upper bound of prefix + suffix length over the candidates (0 = context_length)
    int group_off = 0;          // fused pass: the first group_off sequences are the clean captions
    uint16_t* kv_copy = nullptr;
    size_t kv_self_rows = 0;
};
// all sequences of a pass, in chunks bounded by a row budget; carves one FwdBuf per stream from `c`
int forward_all(leaf_text* h, const float* P, const void* W, const int32_t* tokens, const int32_t* lens, const int32_t* cu_dev,
                int n_seq, float* out, int normalize, Carver& c, hipStream_t s, const PrefixPlan& pp = PrefixPlan(),
                const HiddenTaps* taps = nullptr);
// the fp32-grade pass (precise.hip) over all sequences; out may be null with taps
int precise_all(const leaf_text* h, const float* params, const int32_t* tokens, const int32_t* seq_lens, const int32_t* cu_rows, int n_seq,
                float* out, int normalize, void* ws, size_t ws_bytes, hipStream_t s, const HiddenTaps* taps = nullptr);

// operands of a block's QKV product C = A[M, K] B[3d, K]^T: the LN-folded form reads ln_s and bias = c, the plain one bias alone
struct QkvOperands {
    const void* A;
    const uint16_t* B;
    const float* ln_s;
    const float* bias;
    int K;
};
// arguments of the fused QKV + attention launch over `M` rows / `n_seq` sequences cut into `n_tiles` M tiles for `max_len`
QkvAttnArgs fill_qkv_attn_args(const QkvOperands& q, const float2* rowstat, void* out, const void* kv_base, const int32_t* eot_pos,
                               const int32_t* tile_seq, const RowMap& map, int M, int n_seq, int n_tiles, int heads, int d, int max_len);
