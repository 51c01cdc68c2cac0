/* libleaf_hip.so -- C ABI of the MI355X-native LEAF text hot path.
 *
 * The reference (LIONS-EPFL/LEAF) has no FFI: its seams are Python call signatures.
 * Each entry point below names the reference call site it replaces.  Conventions:
 *   - plain C symbols, `int` status (0 = ok), message via leaf_last_error(); no exceptions cross the ABI;
 *   - the library allocates NO caller-visible device memory: the caller (PyTorch) owns parameters,
 *     gradients, optimizer state, activations and workspace and passes raw device pointers + a hipStream_t;
 *   - every call is asynchronous on the given stream; a handle is host-only state, not thread-safe (it owns one small ring of
 *     PINNED HOST buffers for the tile plans of the fused QKV + attention launches, freed by leaf_text_destroy);
 *   - tokens are int32 [n_seq, ctx] row-major, pad id 0, EOT = row maximum (open_clip tokenizer.py:256-263).
 *
 * Parameter buffer: ONE flat fp32 array (leaf_text_param_count floats).  Tensors that receive weight
 * decay (train_AT_text_only.py:323-331: ndim >= 2 and no "bn"/"ln"/"bias"/"logit_scale" in the name) come
 * first (leaf_text_decay_count floats), the rest after; leaf_text_param_info enumerates
 * (open_clip state_dict key, offset, shape).  Gradients and AdamW moments use the same layout, so data
 * parallelism is a single flat all-reduce.
 */
#ifndef LEAF_HIP_H
#define LEAF_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct leaf_text_cfg {
    int32_t layers, width, heads, embed_dim; /* src/open_clip/model_configs/ViT-*.json text_cfg + embed_dim */
    int32_t context_length;                  /* 77 */
    int32_t vocab_size;                      /* 49408 */
    int32_t activation;                      /* 0 = nn.GELU (erf), 1 = QuickGELU (transformer.py:33-36) */
    float ln_eps;                            /* 1e-5 */
} leaf_text_cfg;

typedef struct leaf_text* leaf_text_t;
typedef void* leaf_stream_t; /* hipStream_t */

enum { LEAF_DTYPE_BF16 = 0, LEAF_DTYPE_FP16 = 1 };                               /* MFMA operand type */
enum { LEAF_OBJ_L2 = 0, LEAF_OBJ_NEGL2 = 1, LEAF_OBJ_DISSIM = 2, LEAF_OBJ_SIM = 3 }; /* utils_attacks.py:332-346 */

const char* leaf_last_error(void);
int leaf_version(void);

/* handle: replaces open_clip.factory.create_model's text tower construction (model.py:173-217) */
int leaf_text_create(const leaf_text_cfg* cfg, int fwd_dtype, leaf_text_t* out);
void leaf_text_destroy(leaf_text_t h);
/* options: "chunk" (sequences processed per pass through the layers, >= 1), "last_layer_trim" (0/1, default 1: the last block's attention output, out-projection and
 * MLP are computed for the pooled EOT row only -- exact, every op after attention is row-wise), "compact_resid" (0/1, default 1:
 * the residual stream of the LN-folded forward-only passes as the 16-bit copy + a remainder byte per element instead of an fp32
 * row beside that copy -- see leaf_op_gemm_resid_ln8 below; 0, or LEAF_COMPACT_RESID=0, keeps fp32 rows), "single_edit" (0/1, default 0: see "single-edit passes" below), and the A/B switches "ln_fold", "fuse_attn", "normalize_fare" */
int leaf_text_set_option(leaf_text_t h, const char* name, int value);
/* current value of an option of leaf_text_set_option (+ "split_blocks"); -1 = unknown name */
int leaf_text_get_option(leaf_text_t h, const char* name);

/* flat parameter layout */
size_t leaf_text_param_count(leaf_text_t h);
size_t leaf_text_decay_count(leaf_text_t h);
int leaf_text_num_tensors(leaf_text_t h);
int leaf_text_param_info(leaf_text_t h, int index, char* name, size_t name_len, size_t* offset, int64_t* rows,
                         int64_t* cols); /* cols = 0 for 1-D tensors */

/* 16-bit operand copies of the GEMM weights.  w16_fwd: [N,K] as stored, forward dtype.  w16_bwd (may be
 * NULL): transposed [K,N] copies for the data-gradient GEMMs in the gradient path's 16-bit type (fp16 with a
 * per-step power-of-two loss scale by default, bf16 unscaled with LEAF_GRAD_DTYPE=bf16).  Call after every optimizer step. */
size_t leaf_text_w16_bytes(leaf_text_t h);
int leaf_text_pack_weights(leaf_text_t h, const float* params, void* w16_fwd, void* w16_bwd, leaf_stream_t s);

/* Split blocks: higher-precision GEMMs in the leading transformer blocks of the forward-only passes (encode_text, score_candidates*,
 * forward_kv; the training forward is untouched -- the reference trains under fp16 autocast, utils_AT.py:317-319).  A split GEMM
 * multiplies hi + lo 16-bit splits (x_hi W_hi + x_lo W_hi + x_hi W_lo in the fp32 accumulator, over a longer K through the unchanged
 * GEMM kernels -- the fused QKV + attention launch included; stored q|k|v / attention / hidden rows stay 16-bit).  The embedding's
 * error is made early (profiles/r06_precision_budget_sites.txt).  leaf_text_split_pack_masks: one mask per block,
 * bit 0 = QKV (both operands), bit 1 = out_proj (weights), bit 2 = c_fc (both operands), bit 3 = c_proj (weights) -- leaf_amd's default
 * arithmetic is such a mask list (leaf_amd/model.py PRECISION_MODES; profiles/r06_row_error_census*.txt).  Works on both
 * residual-stream formats ("compact_resid").  `buf` (DEVICE, leaf_text_split_bytes(h, blocks) bytes, caller-owned, must outlive the calls that use it)
 * receives the split weight copies; call again after every optimizer step (as leaf_text_pack_weights).  blocks = 0 (buf ignored)
 * switches splits off.  0 <= blocks <= min(layers - 1, 64); needs option ln_fold = 1. */
size_t leaf_text_split_bytes(leaf_text_t h, int blocks);
int leaf_text_split_pack_masks(leaf_text_t h, const float* params, const int32_t* masks, int blocks, void* buf, leaf_stream_t s);

/* workspace sizes (bytes): mode 0 = forward, 1 = score_candidates, 2 = train backward */
size_t leaf_text_workspace_bytes(leaf_text_t h, int n_seq, int mode);
size_t leaf_text_stash_bytes(leaf_text_t h, int n_seq);

/* Exact work skipping ("EOT trimming"): the causal mask makes a sequence's pooled EOT state independent of every
 * position after EOT, so only the first len = eot_pos + 1 rows of each sequence need computing.  Entry points that
 * run the layer stack take an OPTIONAL pair: seq_lens (HOST int32 [n_seq], 1..ctx) and cu_rows (DEVICE int32
 * [n_seq+1], exclusive prefix sum of seq_lens).  Both NULL = dense (ctx rows per sequence).  Results are
 * bit-identical either way (tests/test_gpu_forward.py::test_packed_rows_are_bit_exact). */

/* CLIP.encode_text (src/open_clip/model.py:269-284): tokens [n_seq,ctx] -> out fp32 [n_seq,embed_dim] */
int leaf_text_forward(leaf_text_t h, const float* params, const void* w16_fwd, const int32_t* tokens,
                      const int32_t* seq_lens, const int32_t* cu_rows, int n_seq, float* out, int normalize, void* ws,
                      size_t ws_bytes, leaf_stream_t s);

/* The same function in fp32-grade arithmetic ("precise" mode, leaf_amd/csrc/precise.hip): fp32 stored intermediates, the fp32
 * MASTER weights (no 16-bit pack is read) and three MFMA passes of on-the-fly fp16 hi / lo splits per GEMM, fp32 LayerNorm /
 * softmax / activation.  For embeddings that leave the engine (export, eval_textfare.py:119-141) and, optionally, the frozen
 * model's anchor pass (utils_AT.py:296); B-caption sized work, about 8x the time per row of leaf_text_forward.  Same row-plan
 * arguments (seq_lens host / cu_rows device, both NULL = dense). */
size_t leaf_text_precise_workspace_bytes(leaf_text_t h, int n_seq);
int leaf_text_forward_precise(leaf_text_t h, const float* params, const int32_t* tokens, const int32_t* seq_lens,
                              const int32_t* cu_rows, int n_seq, float* out, int normalize, void* ws, size_t ws_bytes,
                              leaf_stream_t s);

/* Per-token hidden states of the text tower (the reference ships its encoders as HuggingFace CLIPTextModel(WithProjection) and
 * src/open_clip/transformer.py's text forward computes every row; eval_text_to_image.py:172-178 puts the tower into a diffusion
 * pipeline as text_encoder / text_encoder_2, which reads last_hidden_state, hidden_states[-2] and text_embeds; utils_attacks.py:49-59
 * reads pooler_output / text_embeds of the same call).  A plain pass that carries a list of TAPS: `layer` is HF's hidden_states index
 * -- 0 = token + positional embedding, l = the output of block l - 1, layers = the last block's output -- final_ln != 0 applies
 * ln_final to every row (last_hidden_state = {layers, 1}; SD 2.x / clip_skip: {layers - 1, 1}), and out (device) receives
 * [n_seq, ctx, width] rows in fp32 (out_dtype 0) or the handle's 16-bit type (1: the round-to-nearest conversion of the fp32 value).
 * Dense rows (seq_lens = cu_rows = NULL): all ctx rows of every sequence, which is what a pipeline that cross-attends to the padded
 * positions needs.  Packed rows: positions >= seq_lens[i] come back ZERO.  feat (may be NULL): the usual [n_seq, embed_dim] features
 * of the same pass, bit-identical to leaf_text_forward / _precise; without it the pass stops behind the highest tapped block.  A tap
 * at `layers` runs the last block on all rows (option last_layer_trim does not apply to that pass).  precise != 0: the fp32-grade
 * arithmetic of leaf_text_forward_precise (w16_fwd unused, out_dtype 0 only, ws of leaf_text_precise_workspace_bytes); else ws of
 * leaf_text_workspace_bytes(h, n_seq, 0).  The taps write straight to the caller's buffers.  The final LayerNorm of a tap is the
 * arithmetic of the pooled rows' LayerNorm (leaf_op_project_rows' xn_scratch) bit for bit.  `size` = sizeof(leaf_hidden_args),
 * checked; every refusal is reported before any HIP call and names the field. */
typedef struct leaf_hidden_tap { int32_t layer, final_ln; void* out; } leaf_hidden_tap;
typedef struct leaf_hidden_args {
    uint32_t size;
    const float* params; const void* w16_fwd;                                                    /* w16_fwd unused when precise */
    const int32_t *tokens, *seq_lens /* HOST */, *cu_rows; int32_t n_seq;
    const leaf_hidden_tap* taps /* HOST */; int32_t n_taps, out_dtype /* 0 fp32, 1 = the handle's 16-bit type */;
    float* feat; int32_t normalize;                    /* may be NULL: the usual [n_seq, embed_dim] features of the same pass */
    int32_t precise;
    void* ws; size_t ws_bytes; leaf_stream_t stream;
} leaf_hidden_args;
int leaf_text_forward_hidden(leaf_text_t h, const leaf_hidden_args* a);

/* One search stage of attack_text_leaf (utils_attacks.py:330-348 / 368-386,393): forward of the B*rho candidates in `tokens`, a loss
 * per candidate, the best of the rho candidates of each caption into best_idx [B] (int32) and its feature row into best_feat (fp32
 * [B,embed_dim], may be NULL); loss: fp32 [B,rho].  Every argument is a named field; `size` = sizeof(leaf_score_args), checked.
 * Exactly ONE target: `anchor` [B,embed_dim] with `objective` (LEAF_OBJ_*; first-index arg-max over rho, loss may be NULL), or
 * `class_feat` -- the classification score (leaf_amd/csrc/classify.hip; attack_text_charmer_classification, utils_attacks.py:582-643):
 * L2-normalised features against a class matrix shared by all captions.  class_feat [C, embed_dim] (fp32, device, unit rows: the
 * caller normalises), labels [B] (int32, device, each in [0, C): the caller checks, the engine cannot), LEAF_CLS_MIN_CLASSES <= C <=
 * LEAF_CLS_MAX_CLASSES (an error outside).
 *   logit[c] = <feat[b,r], class_feat[c]>;  loss[b,r] = max_{c != labels[b]} logit[c] - logit[labels[b]] (margin_loss_lm, :145-151;
 *   NaN when a logit is NaN);  pred[b,r] = first arg-max of logit over c (:630-631).
 * loss is REQUIRED with it (best_idx is taken from it); pred (int32 [B,rho]) and logits (fp32 [B*rho, C]) may be NULL.  best_idx[b] =
 * the first of loss[b,:] in the order of leaf_select_topk (NaN first, larger value, lower column).  A candidate's logits, loss and pred
 * do not depend on B, rho, its place in the launch or the grouping of captions into launches: each inner product is summed in one
 * fixed order.
 * The rows of the pass, by the fields (results are bit-identical in all three):
 *   prefix == NULL: all kept rows (seq_lens / cu_rows as in leaf_text_forward, both NULL = dense); kv, base_cu, kv_write NULL / 0.
 *   prefix != NULL, kv_write == 0: "prefix reuse" over the cache `kv` of leaf_text_forward_kv below; seq_lens / cu_rows (then the rows
 *     to COMPUTE per candidate and their prefix sum), base_cu, kv and base_rows are required.
 *   kv_write != 0: the fused first stage below: `kv` (kv_bytes) is written.  Anchor target only. */
#define LEAF_CLS_MIN_CLASSES 2
#define LEAF_CLS_MAX_CLASSES 1024
typedef struct leaf_score_args {
    uint32_t size;
    const float* params; const void* w16_fwd;                                                    /* weights */
    const int32_t *tokens, *seq_lens /* HOST */, *cu_rows;                                       /* rows */
    const int32_t *prefix, *base_cu; void* kv; size_t base_rows, kv_bytes; int32_t max_len, kv_write; /* prefix reuse */
    int32_t B, rho;
    const float* anchor; int32_t objective;                                                      /* anchor target */
    const float* class_feat; int32_t C; const int32_t* labels; int32_t* pred; float* logits;     /* class target */
    int32_t* best_idx; float *best_feat, *loss;                                                  /* outputs */
    void* ws; size_t ws_bytes; leaf_stream_t stream;
} leaf_score_args;
int leaf_score_pass(leaf_text_t h, const leaf_score_args* a);

/* Segmented top-n selection (leaf_amd/csrc/select.hip; Charmer's position pick and arg-max, leaf_amd/charmer.py): per row b of
 * loss [B, ld] (fp32, device) the min(n, count[b]) largest of columns [0, count[b]) in descending order -- ties -> lower column
 * first, NaN above every number (as torch.topk / torch.argmax) -- into idx / val [B, n]; unused slots: idx -1, val -inf.
 * accumulate != 0 (n == 1 only): merge into the running (val[b], idx[b]) instead, replacing it only on a STRICTLY greater value
 * (or when idx[b] < 0), column index reported as col_offset + j: a long row scored in column chunks keeps "first maximum wins".
 * No arithmetic touches a value: the result equals a stable descending sort bit for bit. */
int leaf_select_topk(const float* loss, int ld, const int32_t* count, int B, int n, int col_offset, int accumulate,
                     int32_t* idx, float* val, leaf_stream_t s);

/* Exact work skipping, part 2 ("prefix reuse"): a search candidate equals its clean caption at every
 * position before its first changed token, and under the causal mask those rows are identical at every layer.
 * leaf_text_forward_kv runs the clean captions once and keeps each layer's q|k|v rows in `kv` (leaf_text_kv_bytes);
 * leaf_score_pass with `prefix` (device, [B*rho]) then computes, for candidate i of caption i / rho, only positions
 * [prefix[i], prefix[i] + seq_lens[i]) and reads the K/V of earlier positions from the cache.  seq_lens = the suffix lengths (host),
 * cu_rows = their exclusive prefix sum (device), base_cu = packed row offsets of the captions inside the cache (device, [B+1]),
 * base_rows = total cached rows per layer, max_len = an upper bound of prefix[i] + seq_lens[i] over the candidates
 * (sizes the attention kernel's LDS; 0 = context_length).  Results are bit-identical to the pass without `prefix`. */
size_t leaf_text_kv_bytes(leaf_text_t h, int n_seq);
int leaf_text_forward_kv(leaf_text_t h, const float* params, const void* w16_fwd, const int32_t* tokens,
                         const int32_t* seq_lens, const int32_t* cu_rows, int n_seq, float* out /* may be NULL */,
                         int normalize, void* kv, size_t kv_bytes, void* ws, size_t ws_bytes, leaf_stream_t s);
/* leaf_text_forward_kv and the FIRST stage's prefix pass in one (leaf_score_pass with kv_write != 0; the clean-caption pass is a chain
 * of ~80 small launches; here its 3,200 rows ride in the candidates' launches): tokens [(B + B*rho), ctx] with the B captions FIRST,
 * seq_lens (host) = rows to compute per sequence (captions: their length; candidates: suffix length), cu_rows = exclusive
 * prefix sum (device, [B + B*rho + 1]), prefix (device; 0 for the captions); base_cu NULL (the captions' offsets are cu_rows' first).
 * `kv` receives the captions' per-layer q|k|v rows exactly as leaf_text_forward_kv writes them (later stages are prefix passes over
 * it).  Bit-identical results.  Returns 2 when the rows do not fit one chunk (use the two separate calls then). */

/* Exact work skipping, part 3 ("single-edit passes"; option "single_edit" of leaf_text_set_option, 0/1, default 0, set by the caller
 * for the passes it holds for).  Block 0's q|k|v row is LN1(E[token] + P[position]) W_qkv + b: it depends on the pair (token,
 * position) and on nothing else.  With the option set the caller PROMISES, for every candidate i of a prefix or fused
 * leaf_score_pass, that it is its caption with ONE token replaced at position prefix[i]: equal lengths, and every token BEHIND
 * prefix[i] equal to the caption's at the same position (in front of it: the promise prefix reuse makes already).  Of the rows a
 * candidate computes only row prefix[i] then has a pair its caption does not have; block 0 projects that one row per candidate (one
 * small GEMM) and its attention reads every other q|k|v row -- Q included -- from layer 0 of the captions' cache.  Every later
 * block is unchanged and the results are bit-identical.  The cache must hold the captions' Q rows of layer 0: leaf_text_forward_kv
 * writes them; the fused pass writes them only when it runs with the option set itself (without it the captions' Q rows never
 * leave the chip), so a cache from a fused pass WITHOUT the option must not be handed to a pass WITH it (leaf_amd/model.py keeps
 * that flag beside the cache and refuses).  The engine cannot check the promise (the tokens are on the device); a broken one gives
 * wrong scores.  Passes the mode does not take (ln_fold = 0, dense rows, no prefix map, a one-block tower) run as without the
 * option.  For token-level substitutions (leaf_amd/step.py, the benchmark's synthetic search); NOT for the character-level string
 * search (leaf_amd/attacks.py, charmer.py): a character edit re-tokenises the rest of the caption. */

/* Training forward (utils_AT.py:317-319) keeping activations in `stash` (leaf_text_stash_bytes) for the backward pass: tokens
 * [n_seq, ctx] -> out fp32 [n_seq, embed_dim]; `size` = sizeof(leaf_train_fwd_args), checked.
 * delta (may be NULL): the OPTIONAL embedding-space PGD mode (no reference path runs it on text, the pieces are
 * the reference's): forward of tokens whose embeddings carry an additive perturbation delta (fp32 [rows, width], packed like the
 * activations, resident in HBM across the inner iterations) - the embedding-input forward of src/pez/open_clip_pez/model.py:210-228
 * fused into the embedding gather + first LayerNorm.
 * pool_last != 0: text embedding inversion (PEZ: src/pez/optim_utils.py:26-55,139-232; leaf_amd/inversion.py).  The training forward
 * for an INVERTED PROMPT [SOT, ids, EOT]: a projected id may itself be 49407 or 49406, so the pooled row is not "the first maximum
 * token id" but the template's EOT slot (open_clip_pez/model.py:226 with the dummy ids of optim_utils.py:119-128), the LAST row of
 * the sequence: the pass pools at row seq_lens[i] - 1 and keeps all seq_lens[i] rows whatever the ids are; seq_lens / cu_rows are
 * REQUIRED, ws must hold n_seq x width floats, and delta must be NULL. */
typedef struct leaf_train_fwd_args {
    uint32_t size;
    const float* params; const void* w16_fwd;
    const int32_t *tokens, *seq_lens /* HOST */, *cu_rows; int32_t n_seq;
    const float* delta; int32_t pool_last;
    float* out; void* stash; size_t stash_bytes;
    void* ws; size_t ws_bytes; leaf_stream_t stream;
} leaf_train_fwd_args;
int leaf_text_forward_train(leaf_text_t h, const leaf_train_fwd_args* a);

/* Vocabulary projection (nn_project, optim_utils.py:26-55; leaf_amd/csrc/nnproj.hip): ids[m] = arg-max over v of
 * (q[m] . table[v]) * inv_norm[v], cos[m] (may be NULL) = that value / ||q[m]||.  q [M, d], table [V, d], inv_norm [V] (from
 * leaf_vocab_inv_norms: 1 / ||table[v]||, computed once while the weights are frozen), all fp32 on the device; any M >= 1, V >= 1,
 * d % 4 == 0, d <= 2048 (an error otherwise); ws: leaf_nn_project_ws_bytes(M, V) bytes.  Exact fp32 products on the matrix cores,
 * ONE summation order per (row, id): a row's ids / cos bits depend on neither M, its place in the launch nor the launch.  Order of
 * the arg-max: NaN first, larger value, lower id (as leaf_select_topk) -- identical table rows resolve to the lower id, a NaN
 * query row returns id 0.  The table is read from HBM once per call. */
int leaf_vocab_inv_norms(const float* table, int V, int d, float* inv_norm, leaf_stream_t s);
size_t leaf_nn_project_ws_bytes(int M, int V);
int leaf_nn_project(const float* q, int M, const float* table, const float* inv_norm, int V, int d, int32_t* ids,
                    float* cos /* may be NULL */, void* ws, size_t ws_bytes, leaf_stream_t s);

/* fused grad-sign / normalise - step - project on the resident perturbation, per sequence over its kept rows:
 * norm 0 (linf): delta <- clamp(delta + alpha sign(grad), -eps, eps)       (utils_attacks.py:693-694)
 * norm 2 (l2)  : delta <- renorm_2(delta + alpha grad / ||grad||_2, eps)   (src/robust_vlm/train/utils.py:96-114)
 * cu_rows: device prefix sums of the kept rows ([n_seq + 1]) or NULL for dense ctx rows per sequence. */
int leaf_pgd_step(float* delta, const float* grad, const int32_t* cu_rows, int n_seq, int ctx, int width, float alpha,
                  float eps, int norm, leaf_stream_t s);

/* The backward through the stash of the last training forward (feat fp32 [n_seq, embed_dim] = what it returned), from one of three
 * loss heads; `size` = sizeof(leaf_backward_args), checked.  grads (flat fp32, parameter layout): the parameter gradients are
 * ACCUMULATED (+=).  d_embed (fp32 [rows, width], packed like the activations): OVERWRITTEN with the un-scaled gradient with respect to
 * the token embeddings / delta, no parameter gradient touched when grads is NULL.  layer_events (may be NULL), for the overlap of the
 * data-parallel gradient reduction with the backward: L + 1 hipEvent_t (NULL entries skipped); [l] is recorded on
 * `stream` once every gradient of transformer block l is final in `grads` (blocks finish in the order L-1 .. 0), [L] after the last
 * kernel.  Every refusal below is reported before any HIP call.
 * LEAF_HEAD_FARE: TextFARE (utils_AT.py:321-337), ref = anchor: loss = mean_b sum_j (anchor - feat)^2 into head_out (one device
 *   float, unscaled); back-propagates loss * scale (= 1/accum_freq).  Exactly one of grads / d_embed; with d_embed (the backward of
 *   the continuous attack loop, utils_attacks.py:683-692) scale must be 1.
 * LEAF_HEAD_COSINE: text embedding inversion (optim_utils.py:191-196 with prompt_bs = batch_size = 1, for n_seq independent inversions
 *   at once), ref = target: loss_b = scale (1 - cos(feat_b, target_b)), the target normalised inside the head, fp32; d_embed = gradient
 *   of the SUM over b, so every sequence receives exactly the gradient of its own loss.  head_out = cos [n_seq] (may be NULL).
 *   d_embed only; option normalize_fare must be off.
 * LEAF_HEAD_UPSTREAM: ANY loss of the features that the caller computed, ref = dfeat = d loss / d feat (fp32 [n_seq, embed_dim],
 *   device); head_out unused.  Back-propagates scale * dfeat -- through F.normalize as well when option normalize_fare is on (feat is
 *   then the normalised rows; it is read for that product only).  grads, d_embed or both (one pass).  With a scaler state attached and
 *   grads given, the fp16 gradient path checks its 16-bit tensors for saturation and poisons gradient element 0, exactly as the
 *   TextFARE head does (GRADIENT SCALER below); a non-finite dfeat reaches the gradients as NaN and the guarded optimizer step skips.
 *   Every kernel behind the head is the one the other two heads run: fed their dout (kernel hooks leaf_op_fare_loss /
 *   leaf_op_cosine_head) and scale = 1, it writes their gradients bit for bit. */
enum { LEAF_HEAD_FARE = 0, LEAF_HEAD_COSINE = 1, LEAF_HEAD_UPSTREAM = 2 };
typedef struct leaf_backward_args {
    uint32_t size;
    const float* params; const void* w16_bwd;
    const int32_t *tokens, *seq_lens /* HOST */, *cu_rows; int32_t n_seq;
    const float* feat; int32_t head; const float* ref; float scale; float* head_out;             /* loss head */
    const void* stash; float *grads, *d_embed; void* const* layer_events;
    void* ws; size_t ws_bytes; leaf_stream_t stream;
} leaf_backward_args;
int leaf_text_backward(leaf_text_t h, const leaf_backward_args* a);

/* torch.optim.AdamW step over the flat buffers (train_AT_text_only.py:326-341): decoupled weight decay `wd`
 * on the first n_decay elements, 0 on the rest; step counts from 1; grads are multiplied by grad_scale first
 * (1/world_size after a sum all-reduce). */
int leaf_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, size_t n_decay,
                    float lr, float beta1, float beta2, float eps, float wd, int step, float grad_scale,
                    leaf_stream_t s);
/* GRADIENT SCALER (the reference trains under fp16 autocast with torch.cuda.amp.GradScaler: train_AT_text_only.py:347,
 * utils_AT.py:79-83,339-362).  The fp16 gradient path multiplies the loss gradient by a power of two S chosen on the device
 * each step (max|d loss / d feat| * S in [8, 16)) and its 16-bit conversions SATURATE at +-65504 instead of producing inf, so
 * an overflow would clip silently.  With a scaler state attached (leaf_text_set_grad_scaler) the backward checks every 16-bit
 * gradient tensor of every block for saturated / non-finite values; a hit poisons gradient element 0 with NaN (the first element
 * of the token-embedding gradient: every later writer only adds to it, and it is reduced with the last data-parallel bucket), so the guarded optimizer step below -- after the data-parallel all-reduce,
 * hence on every rank alike -- skips the step, and halves S for the following steps (state[LEAF_SC_BACKOFF] -= 1); after
 * state[LEAF_SC_INTERVAL] (default 2000, GradScaler's growth_interval) applied steps in a row the back-off is taken back by
 * one halving.  The state is the head of the clip_ws buffer of leaf_adamw_step_clip: device fp32 [LEAF_SC_WORDS + 2048],
 * zeroed once by the caller. */
enum {
    LEAF_SC_COEF = 0,      /* clip coefficient applied by the last guarded step, -1 = that step was skipped */
    LEAF_SC_NORM = 1,      /* total gradient norm seen by the last guarded step */
    LEAF_SC_SKIPPED = 2,   /* optimizer steps skipped so far (non-finite norm: overflow, saturation, NaN) */
    LEAF_SC_BACKOFF = 3,   /* <= 0: log2 of the persistent factor on the per-step loss scale */
    LEAF_SC_GOOD = 4,      /* applied steps since the scale last changed */
    LEAF_SC_SAT_FLAG = 5,  /* a 16-bit gradient tensor saturated during the current optimizer step */
    LEAF_SC_SAT_STEPS = 6, /* skipped steps that had the saturation flag up */
    LEAF_SC_INTERVAL = 7,  /* growth interval in applied steps (0 = 2000) */
    LEAF_SC_APPLIED = 8,   /* AdamW steps really taken = the `step` of the bias corrections (a skipped step does not count) */
    LEAF_SC_BC1 = 9, LEAF_SC_SQRT_BC2 = 10, /* bias corrections of the last applied step */
    LEAF_SC_WORDS = 16
};
/* attach (or detach with NULL) the scaler state used by leaf_text_backward of this handle */
int leaf_text_set_grad_scaler(leaf_text_t h, float* state);

/* the same step preceded by torch.nn.utils.clip_grad_norm_(parameters, max_norm, 2.0) (--grad-clip-norm,
 * utils_AT.py:348-357): total norm = grad_scale * ||grads||_2, gradients are multiplied by min(1, max_norm / (norm + 1e-6))
 * inside the AdamW kernel (grads themselves are left untouched).  clip_ws: fp32 device scratch [LEAF_SC_WORDS + 2048], zeroed
 * once by the caller (layout above).  NON-FINITE GUARD: when the norm is inf / NaN the whole step is skipped (parameters and
 * moments untouched, GradScaler.step semantics), clip_ws[LEAF_SC_COEF] = -1 and clip_ws[LEAF_SC_SKIPPED] counts the skipped
 * steps.  `step` counts ATTEMPTED steps from 1; the bias corrections use step - skipped (clip_ws[LEAF_SC_APPLIED]).
 * max_norm = +inf gives the guard without clipping. */
int leaf_adamw_step_clip(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, size_t n_decay,
                         float lr, float beta1, float beta2, float eps, float wd, int step, float grad_scale,
                         float max_norm, float* clip_ws, leaf_stream_t s);

/* torch.nn.utils.clip_grad_norm_ IN PLACE, for --grad-clip-norm together with --accum-freq > 1 (utils_AT.py:348-357 clips the
 * running gradient sum after every micro-batch's backward, not only before the step): grads <- grads * pre_scale *
 * min(1, max_norm / (pre_scale * ||grads||_2 + 1e-6)).  pre_scale folds a pending factor into the same pass (data parallel: the
 * replicated running sum is divided by the world size before the next micro-batch's local gradients are added and summed over
 * ranks); max_norm = +inf only applies pre_scale.  A non-finite norm leaves the gradients untouched (the step's guard skips).
 * ws: fp32 device scratch [2 + 2048]; ws[0] = the factor applied, ws[1] = the norm. */
int leaf_clip_grads_inplace(float* grads, size_t n, float pre_scale, float max_norm, float* ws, leaf_stream_t s);

/* ---- native host side of the search: CLIP BPE + single-edit mutation, multithreaded ----
 * leaf_tok_create takes the DECOMPRESSED text of bpe_simple_vocab_16e6.txt (src/open_clip/tokenizer.py:139-150).
 * Fast path = printable ASCII without '&'; other inputs are flagged in `fallback` (1 byte per text / per candidate)
 * and must be tokenised by the caller's reference-equivalent tokenizer.  lens[i] = EOT position + 1. */
typedef struct leaf_tok* leaf_tok_t;
int leaf_tok_create(const char* merges_text, size_t len, leaf_tok_t* out);
void leaf_tok_destroy(leaf_tok_t tk);
/* SimpleTokenizer.__call__ (tokenizer.py:226-265): texts -> int32 [n, ctx] */
int leaf_tok_encode_batch(leaf_tok_t tk, const char* const* texts, const int32_t* text_len, int n, int ctx,
                          int32_t* tokens, int32_t* lens, uint8_t* fallback, int n_threads);
/* generate_sentence(S, z, u, V, alternative=-1) (utils_attacks.py:169-213) for B sentences x rho (z, c = V[u]) pairs,
 * then tokenisation of every candidate: -> int32 [B*rho, ctx] */
int leaf_tok_mutate_encode(leaf_tok_t tk, const char* const* sentences, const int32_t* sent_len, int B, const int32_t* z,
                           const int32_t* c, int rho, int ctx, int32_t* tokens, int32_t* lens, uint8_t* fallback,
                           int n_threads);

/* --constrain (utils_attacks.py:110-143,321-325,360-364): valid[b * rho + r] = 1 iff candidate generate_sentence(S_b, z, c,
 * alternative = -1) holds STRICTLY FEWER distinct dictionary words than S_b.  The word set is built once (leaf_dict_create:
 * '\n'-separated words); only the whitespace-delimited window around the edit is re-tokenised.  tokenizer_kind 0 = the regex
 * tokenizer [A-Za-z0-9]+|[^\sA-Za-z0-9] (exact for all ASCII), 1 = nltk.word_tokenize: NLTKWordTokenizer's substitution pipeline
 * (nltk/tokenize/destructive.py, third-party: requirements.txt:14) restated window-locally, exact for ASCII text whose tokens
 * cannot depend on the Punkt sentence model -- a sentence / candidate in which a lone '.' ends a whitespace-delimited chunk
 * before the end of the text gets fallback = 1 from THIS entry point and is decided by the caller with the real nltk
 * (leaf_tok_constrain_ranges / leaf_tok_constrain_punkt below decide those natively too). */
typedef struct leaf_dict* leaf_dict_t;
int leaf_dict_create(const char* words, size_t len, leaf_dict_t* out);
void leaf_dict_destroy(leaf_dict_t d);
int leaf_tok_constrain(leaf_dict_t d, int tokenizer_kind, const char* const* sentences, const int32_t* sent_len, int B,
                       const int32_t* z, const int32_t* c, int rho, uint8_t* valid, uint8_t* fallback, int n_threads);
/* the same with the caller's SENTENCE SEGMENTATION (tokenizer_kind 1 only): nltk.word_tokenize tokenises sentence by sentence, and
 * where a sentence ends is decided by nltk's trained Punkt model, which is not restated.  ranges / ranges_off: for sentence b the
 * spans [ranges[2 i], ranges[2 i + 1]) , i in [ranges_off[b], ranges_off[b + 1]), as PunktSentenceTokenizer.span_tokenize returns them
 * for the lower-cased caption (none = handled as by leaf_tok_constrain).  A candidate is decided natively when its edit window lies
 * inside one span, holds no '.', '?' or '!' before or after the edit and does not directly follow a token that ends in one (Punkt
 * looks at the token carrying the period and the one after it); the others get fallback = 1. */
int leaf_tok_constrain_ranges(leaf_dict_t d, int tokenizer_kind, const char* const* sentences, const int32_t* sent_len, int B,
                              const int32_t* z, const int32_t* c, int rho, const int32_t* ranges, const int32_t* ranges_off,
                              uint8_t* valid, uint8_t* fallback, int n_threads);
/* nltk's Punkt sentence splitter restated (nltk/tokenize/punkt.py PunktSentenceTokenizer.span_tokenize, realign_boundaries = True;
 * third-party, requirements.txt:14): the algorithm is fixed, the trained model only fills four tables.  The tables as '\n'-separated
 * UTF-8 lines: abbreviation types; collocations "first\tsecond"; frequent sentence starters; orthographic contexts "type\tflags"
 * (PunktParameters.abbrev_types / collocations / sent_starters / ortho_context).  ASCII text without control characters only:
 * leaf_punkt_spans returns 2 for anything else.  spans: (start, end) pairs, at most cap_pairs (1 = overflow / bad arguments). */
typedef struct leaf_punkt* leaf_punkt_t;
int leaf_punkt_create(const char* abbrev, size_t abbrev_len, const char* colloc, size_t colloc_len, const char* starters,
                      size_t starters_len, const char* ortho, size_t ortho_len, leaf_punkt_t* out);
void leaf_punkt_destroy(leaf_punkt_t p);
/* strict = 1 (the default): a text in which one whitespace-delimited chunk holds two or more candidate break positions ("what?! yes",
 * "wow!!! nice") is declined (2): nltk 3.6.6 rewrote the scan for period contexts and the generations are only provably equal
 * elsewhere.  strict = 0 decides every text as nltk 3.6.5 does (the generation the golden vectors were made with). */
int leaf_punkt_set_strict(leaf_punkt_t p, int strict);
int leaf_punkt_spans(leaf_punkt_t p, const char* text, int len, int32_t* spans, int cap_pairs, int32_t* n_pairs);
/* leaf_tok_constrain for nltk.word_tokenize (tokenizer_kind 1) with the Punkt tables: the sentence spans of captions AND candidates
 * are computed natively, so only non-ASCII text / control characters get fallback = 1. */
int leaf_tok_constrain_punkt(leaf_dict_t d, leaf_punkt_t punkt, const char* const* sentences, const int32_t* sent_len, int B,
                             const int32_t* z, const int32_t* c, int rho, uint8_t* valid, uint8_t* fallback, int n_threads);
/* number of distinct dictionary words of ONE text (utils_attacks.py:135,139), for the strings leaf_tok_constrain* declines: with the
 * sentence spans of that text from the caller's Punkt (n_ranges pairs; 0 = the text must not depend on sentence boundaries) the count is
 * native too -- one Punkt call instead of a whole nltk.word_tokenize.  Returns 0; 2 = declined (non-ASCII, or spans missing). */
int leaf_tok_count_words(leaf_dict_t d, int tokenizer_kind, const char* text, int len, const int32_t* ranges, int n_ranges,
                         int32_t* count);
/* test / debug hook: the word tokens of `text` under tokenizer_kind (0 = the regex stand-in of leaf_amd/attacks.py, 1 =
 * nltk.word_tokenize restated: nltk/tokenize/destructive.py's substitution pipeline), '\n'-joined into out[0, cap).
 * Returns 0; 2 when the text is declined (kind 1: non-ASCII, or a lone '.' ends a chunk inside the text, where the result would
 * depend on nltk's trained Punkt sentence splitter); 1 on bad arguments. */
int leaf_tok_word_tokens(int tokenizer_kind, const char* text, int len, char* out, int cap, int* out_len);
/* dup_of[b * rho + r] = first r' <= r with tokens[b, r', :] == tokens[b, r, :] (SURVEY 8f-2 dedupe: src/open_clip/tokenizer.py:83-85,139
 * lower-cases and collapses whitespace, so distinct edits can tokenise identically; first index wins as in torch.argmax,
 * utils_attacks.py:348,386).  tokens int32 [B, rho, ctx] on the host. */
int leaf_tok_duplicate_map(const int32_t* tokens, int B, int rho, int ctx, int32_t* dup_of, int n_threads);

/* ---- per-launch GEMM timing (bench.py roofline): between begin/end every GEMM launch is bracketed by HIP events on
 * its stream; end_shapes() sums duration / algorithmic FLOPs / algorithmic bytes / launches per key = kernel_family*16 + operand_dtype*8 + epilogue id
 * (family 0 = gemm_nt_kernel, 4 = gemm_nt256_half_kernel, 6 = gemm_nt64_ring_kernel; keys < 128). */
int leaf_prof_begin(void);
int leaf_prof_pause(int paused);   /* suspend / resume the recording (per-launch events on a sample of the timed steps only) */
/* same records grouped by (key, N, K): info[4 i] = {key, N, K, launches}, rows[i] = sum of M; *n_out groups written */
int leaf_prof_end_shapes(double* ms, double* flops, double* bytes, int64_t* rows, int32_t* info, int max_groups, int* n_out);

/* ---- single-kernel hooks (used by the parity tests to check each HIP kernel against the oracle) ---- */
/* C[M,N] = epilogue(A[M,K] * B[N,K]^T): epi 0 store16(+bias), 1 act16(+bias, aux = pre-activation), 2 fp32 += ,
 * 3 fp32 = beta*C + acc, 4 store16(acc * act'(aux)).  A, B 16-bit of `dtype`, contiguous. */
int leaf_op_gemm(int dtype, int epi, const void* A, const void* B, void* C, const float* bias, void* aux, int M, int N,
                 int K, int act, float beta, int aux_f16, leaf_stream_t s);
/* same with explicit row strides (elements) */
int leaf_op_gemm_ld(int dtype, int epi, const void* A, int lda, const void* B, int ldb, void* C, int ldc, const float* bias,
                    void* aux, int M, int N, int K, int act, float beta, int aux_f16, leaf_stream_t s);
/* C32 += [A | A] B^T + bias: A [M, Ka] stored once and re-read along K = 2 Ka by the half-stage ring kernel (B [N, 2 Ka] = e.g. the
 * [hi | lo] split of a weight: the out-projection of a split block); an error for launches that kernel does not take */
int leaf_op_gemm_awrap(int dtype, const void* A, const void* B, float* C, const float* bias, int M, int N, int Ka, leaf_stream_t s);
/* LayerNorm folded into the GEMMs of the forward-only passes (leaf_amd/csrc/lnfold.h; replaces the LayerNorm launches between
 * the GEMMs of transformer.py:254-265).  Producer: C32[M,N] += A B^T + bias, x16 = 16-bit copy of the result, stat = float2
 * [N/64][M] (sum, M2 = sum (x - group mean)^2) of each row's 64-column groups.  Finalize: rowstat[m] = (mean, rstd) merged from
 * stat [ngroups][ld] (Chan).  Consumer: C16 = [act](rstd[m] (A Bp^T - mean[m] s[n]) + c[n]), Bp = 16-bit(gamma * W), s[n] =
 * sum_k Bp[n,k], c[n] = beta . W[n,:] + bias[n]; act: -1 none, 0 GELU, 1 QuickGELU. */
int leaf_op_gemm_resid_ln(int dtype, const void* A, const void* B, float* C, const float* bias, void* x16, void* stat, int M, int N,
                          int K, leaf_stream_t s);
/* The residual stream of the LN-folded forward-only passes in 16 + 8 bits (option 'compact_resid', default on): a residual value x is
 * held as x16 = 16-bit(x) -- the copy the next GEMM multiplies anyway -- and lo8 = the remainder x - x16 as an e4m3 byte, block-scaled (four consecutive values share
 * the power of two of their largest |x16|; v_cvt_scalef32_pk_fp8_f32 / _f32_fp8), i.e. to 2^-16 of that largest value (fp16) in 3 bytes instead of an fp32 row beside the 16-bit copy (6 bytes).  leaf_op_gemm_resid_ln8: the producer above
 * on that format, (x16, lo8) [M,N] updated IN PLACE, stat as above.  leaf_op_resid_pack / _unpack: the format itself, element-wise
 * (n % 4 == 0).  The reference's residual stream is fp32 (transformer.py:254-265); the difference is far inside the 16-bit operand
 * rounding of every GEMM (tests/test_gpu_kernels.py, test_compact_residual_*). */
int leaf_op_gemm_resid_ln8(int dtype, const void* A, const void* B, void* lo8, const float* bias, void* x16, void* stat, int M, int N,
                           int K, leaf_stream_t s);
int leaf_op_resid_pack(int dtype, const float* x, void* x16, void* lo8, size_t n, leaf_stream_t s);
int leaf_op_resid_unpack(int dtype, const void* x16, const void* lo8, float* x, size_t n, leaf_stream_t s);
int leaf_op_ln_finalize(const void* stat, int ld, int rows, int ngroups, float eps, void* rowstat, leaf_stream_t s);
int leaf_op_gemm_lnfold(int dtype, int act, const void* A, const void* Bp, void* C16, const float* c_vec, const float* s_vec,
                        const void* rowstat, int M, int N, int K, leaf_stream_t s);
/* LN-folded QKV projection + causal attention in ONE launch (leaf_amd/csrc/qkv_attn.hip; nn.MultiheadAttention's in_proj ->
 * softmax(q k^T / 8 + causal mask) v, src/open_clip/transformer.py:225,239-252): out[rows, width] (eot_pos: [n_seq, width]) from the
 * 16-bit residual copy x16 [rows, width], Wp = 16-bit(gamma * in_proj_weight) [3 width, width] with its c / s vectors and the rows'
 * (mean, rstd).  lens (HOST) = rows per sequence, cu (device) their exclusive prefix sum; prefix / base_cu / kv (device, or all
 * NULL) = cached-prefix mode as in leaf_score_pass with candidates grouped `group` per caption; tile_seq = device
 * scratch [2 (n_seq + 1)].  Kernel hook for tools/qkv_attn_bench.py; the scoring passes call the same launch internally. */
int leaf_op_qkv_attn(int dtype, const void* x16, const void* Wp, const float* c_vec, const float* s_vec, const void* rowstat,
                     void* out, const void* kv, const int32_t* lens, const int32_t* cu, const int32_t* prefix,
                     const int32_t* base_cu, const int32_t* eot_pos, int32_t* tile_seq, int n_seq, int rows, int group,
                     int ctx, int heads, int width, leaf_stream_t s);
/* the classification score of leaf_score_pass alone, on given feature rows feat [B*rho, D] (kernel hook for the tests) */
int leaf_op_classify(const float* feat, const float* class_feat, const int32_t* labels, int B, int rho, int D, int C, float* loss,
                     int32_t* pred, float* logits, int32_t* best_idx, float* best_feat, leaf_stream_t s);
/* the cosine head of leaf_text_backward (LEAF_HEAD_COSINE) alone (kernel hook for the tests): dout [B, D] = d (sum_b loss_b) / d feat, cos_out [B]
 * (may be NULL); ws: 64 + 2 B device floats */
int leaf_op_cosine_head(const float* feat, const float* target, int B, int D, float loss_weight, float* dout, float* cos_out,
                        float* ws, leaf_stream_t s);
int leaf_op_attention_fwd(const void* qkv, void* out, int n_seq, int ctx, int heads, int width, int dtype,
                          leaf_stream_t s);
/* the same launcher in every row mode (leaf_amd/csrc/attention.hip; RowMap in common.h).  All pointers are device pointers; kv, cu,
 * prefix, base_cu and eot_pos may each be NULL.  cu [n_seq + 1]: packed rows (NULL: dense, ctx rows per sequence); prefix [n_seq]
 * with kv [cache rows, 3 width] and base_cu [captions + 1]: positions < prefix[s] are read from the cache rows of caption
 * (s - group_off) / group, and only positions >= prefix[s] are computed and written; eot_pos [n_seq]: one query row per sequence,
 * written to out[sequence]; max_len: longest sequence of the launch (0: ctx), sizes the LDS image; single_edit: qkv is a
 * [n_seq, 3 width] table with the one fresh row of each sequence at position prefix[s], every other position (Q included) comes
 * from the cache, and sequences in front of group_off are captions read from the cache alone (an error without kv / prefix /
 * base_cu). */
int leaf_op_attention_fwd_map(const void* qkv, const void* kv, void* out, const int32_t* cu, const int32_t* prefix,
                              const int32_t* base_cu, const int32_t* eot_pos, int n_seq, int ctx, int group, int group_off,
                              int max_len, int single_edit, int heads, int width, int dtype, leaf_stream_t s);
int leaf_op_layernorm(const float* x, const float* g, const float* b, float eps, void* out16, int rows, int width,
                      int dtype, leaf_stream_t s);
/* attention backward; g_dtype (LEAF_DTYPE_*) is the gradient type of dout / dqkv */
int leaf_op_attention_bwd_t(const void* qkv, int qkv_dtype, const void* dout16, void* dqkv16, int g_dtype, int n_seq,
                            int ctx, int heads, int width, leaf_stream_t s);
/* the same on the row map of the training backward: cu [n_seq + 1] on the device = packed rows, NULL = dense (ctx rows per sequence) */
int leaf_op_attention_bwd_map(const void* qkv, int qkv_dtype, const void* dout16, void* dqkv16, int g_dtype, const int32_t* cu,
                              int n_seq, int ctx, int heads, int width, leaf_stream_t s);
/* The other launchers of the training backward one at a time, on the same row map (cu as above; all pointers device pointers).
 * pool_project_bwd: backward of text_projection + ln_final on the pooled rows.  dout [n_seq, D], pooled [n_seq, d] = LN_final of row
 * eot_idx[s] of sequence s of x [rows, d]; dx [rows, d]: ONLY the pooled rows are written, with S * d loss / d x (gscale = {S, 1/S});
 * dproj [d, D], dg [d], db [d] are added to, un-scaled, and may be NULL (all three: input gradient only); scratch: n_seq (d + 2) floats.
 * embed_bwd: dtok [vocab, d] += (1 / S) sum of the dx rows of each token id (ids clamped to 0 .. vocab - 1; tokens [n_seq, ctx], on
 * packed rows only the first len(s) slots of a sequence count), dpos [ctx, d] += (1 / S) sum over sequences; rows = rows of dx.
 * fare_loss: loss = mean_b ||feat_b - anchor_b||^2 * scale, dout = its gradient (through F.normalize when norms [B] = the norms of
 * the un-normalised features is given), gscale_ws [64 + 2 B]: {S, 1/S} in front, S = 1 without use_scaling, else the power of two
 * that brings max|dout| into [8, 16), times 2^scaler[LEAF_SC_BACKOFF] when scaler is given.  D <= 2048.
 * upstream_head: the head of leaf_text_backward alone: dout = scale * dfeat [B, D], through the VJP of F.normalize when feat [B, D] (the
 * normalised rows) and norms [B] are given (both NULL: none), dout = (g - feat (feat . g)) / max(norms, 1e-12) with g = scale * dfeat;
 * gscale_ws, use_scaling and scaler as fare_loss.  B >= 1, 1 <= D <= 2048 (an error otherwise, reported before any HIP call).
 * sat_check16: n <= 5 fp16 tensors (HOST arrays of device pointers / element counts; 16-byte aligned, numel % 8 == 0): any
 * |value| >= 65504 or non-finite raises scaler[LEAF_SC_SAT_FLAG] = 1 and stores NaN to *poison. */
int leaf_op_pool_project_bwd(const float* dout, const float* pooled, const float* x, const int32_t* eot_idx, const float* g, float eps,
                             const float* proj, float* dx, float* dproj, float* dg, float* db, const float* gscale, const int32_t* cu,
                             int n_seq, int ctx, int d, int D, float* scratch, leaf_stream_t s);
int leaf_op_embed_bwd(const float* dx, const float* gscale, const int32_t* tokens, float* dtok, float* dpos, const int32_t* cu,
                      int rows, int n_seq, int ctx, int d, int vocab, leaf_stream_t s);
int leaf_op_fare_loss(const float* feat, const float* anchor, const float* norms, const float* scaler, int B, int D, float scale,
                      int use_scaling, float* loss, float* dout, float* gscale_ws, leaf_stream_t s);
int leaf_op_upstream_head(const float* dfeat, const float* feat, const float* norms, const float* scaler, int B, int D, float scale,
                          int use_scaling, float* dout, float* gscale_ws, leaf_stream_t s);
int leaf_op_sat_check16(const void* const* bufs, const size_t* numel, int n, float* scaler, float* poison, leaf_stream_t s);
/* one problem of the grouped weight-gradient kernel: dW[Nw,Kw] += alpha dY^T X, db[Nw] += alpha colsum(dY)
 * (dY [rows,Nw] in g_dtype, X [rows,Kw] in x_dtype, alpha a device scalar or NULL = 1; Nw, Kw multiples of 128) */
int leaf_op_wgrad(const void* dY, const void* X, float* dW, float* db, int rows, int Nw, int Kw, int x_dtype,
                  int g_dtype, const float* alpha_dev, leaf_stream_t s);
/* LayerNorm backward of `rows` rows (autograd of F.layer_norm, src/open_clip/transformer.py:15-30): dx_inout[rows,d] +=
 * d LN / d x, dx16 (optional) = its 16-bit copy (g_dtype), dg[d] += sum_r dy * xhat / S, db[d] += sum_r dy / S with
 * gscale = {S, 1/S} on the device (the loss scale of the fp16 gradient path); dg = db = NULL: input gradient only.
 * ws: leaf_op_layernorm_bwd_ws_bytes(rows, d) bytes of device scratch for the per-workgroup partial sums (needed with dg) */
size_t leaf_op_layernorm_bwd_ws_bytes(int rows, int d);
int leaf_op_layernorm_bwd(const float* dy, const float* x, const float* g, float eps, float* dx_inout, void* dx16,
                          int g_dtype, const float* gscale, float* dg, float* db, int rows, int d, void* ws, size_t ws_bytes,
                          leaf_stream_t s);
/* out[M,D] = [normalize](LayerNorm(xg[M,d]; g, b) @ proj[d,D]) in fp32 on the matrix cores; xn_scratch = fp32 [M,d] */
int leaf_op_project_rows(const float* xg, const float* g, const float* b, float eps, const float* proj,
                         float* xn_scratch, float* out, int M, int d, int D, int normalize, leaf_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
