"""Per-token hidden states (leaf_text_forward_hidden / LeafCLIPText.encode_text_hidden) on the GPU.

Block 1 -- bit for bit, no tolerance: packed against dense rows, the tap rows against the pooled-row path of encode_text (the final
LayerNorm of a tap IS the arithmetic of leaf_op_project_rows' LayerNorm), all taps in one pass against one pass per tap, features
unchanged by taps, chunked passes, the 16-bit output against torch's conversion of the fp32 output.

Block 2 -- measured against an fp32 torch-CPU restatement of the tower that returns every layer (``ref_tower`` below; held to
oracle/torch_cpu_harness.TorchTextTower on its pooled row) and, on the tiny configs, against transformers' CLIPTextModel /
CLIPTextModelWithProjection loaded from write_hf_text_model's directory.  Metric: rel-L2 per row [of width]; every bound below is
2 x the worst row measured on the MI355X with the FIRST seed pair of its config (the figure beside it); the second seed pair, on
which nothing was tuned, must hold the same bound.

Shapes: tiny-test / tiny-test-quickgelu (d = 128, 2 layers: the fp32 residual stream, the fp32 projection does not take the width)
and ViT-L-14-quickgelu at random init (the 16 + 8-bit stream), n_seq = 3 with lengths {2, 77, 23} (EOT at position 1, in the last
slot, in between), padded once with 0 and once with the EOT id; n_seq = 5 under option chunk = 2 for the per-chunk output offset."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import text_oracle as O
from tests.util import ptr, row_rel_l2, stream

pytestmark = pytest.mark.gpu

SOT, EOT = 49406, 49407
LENS3, LENS5 = (2, 77, 23), (2, 77, 23, 40, 9)
CONFIGS = {"tiny-test": O.TextCfg(128, 2, 2, 64), "tiny-test-quickgelu": O.TextCfg(128, 2, 2, 64, quick_gelu=True),
           "ViT-L-14-quickgelu": O.CONFIGS["ViT-L-14-quickgelu"]}
SEEDS = {"tiny-test": (11, 21), "tiny-test-quickgelu": (12, 22), "ViT-L-14-quickgelu": (1, 2)}        # (measured on, held on)
NAMES = sorted(CONFIGS)


def make_tokens(lens, pad, seed):
    """[SOT, ids .., EOT] of the given lengths (ids below SOT: the EOT is the first maximum), every slot behind it = ``pad``"""
    rng = np.random.default_rng(seed)
    t = np.full((len(lens), 77), pad, np.int32)
    for row, L in zip(t, lens):
        row[:L] = rng.integers(1, SOT, L)
        row[0], row[L - 1] = SOT, EOT
    return t


_MODELS = {}


def model(name, seed, dtype="fp16"):
    """one engine model per (config, seed, operand type) for the whole module; a test that changes an option restores it"""
    from leaf_amd.model import create_model
    key = (name, seed, dtype)
    if key not in _MODELS:
        _MODELS[key] = create_model(name, device="cuda:0", seed=seed, dtype=dtype)
    return _MODELS[key]


def all_taps(L):
    """every hidden_states entry without ln_final, then ln_final of the last two: (layers, final_ln)"""
    return list(range(L + 1)) + [L, L - 1], [False] * (L + 1) + [True, True]


def states(m, tokens, **kw):
    layers, lns = all_taps(m.cfg.layers)
    return m.encode_text_hidden(tokens, layers=layers, final_ln=lns, **kw)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


# =============================================================================================== block 1: bit for bit
@pytest.mark.parametrize("pad", [0, EOT])
@pytest.mark.parametrize("name", NAMES)
def test_packed_and_dense_rows_agree_and_dropped_rows_are_zero(name, pad):
    m = model(name, SEEDS[name][0])
    t = make_tokens(LENS3, pad, seed=3)
    dense = states(m, t)                                      # the default: all 77 rows
    packed = states(m, t, seq_lens=None)                      # host ids: EOT trimming
    given = states(m, t, seq_lens=np.array(LENS3))            # ... and with the lengths from the caller
    device = states(m, torch.from_numpy(t).cuda(), seq_lens=None)      # device ids: lengths unknown on the host, dense
    for k, (d, p) in enumerate(zip(dense, packed)):
        assert d.shape == (3, 77, m.cfg.width) and d.dtype == torch.float32 and torch.isfinite(d).all()
        assert same(p, given[k]) and same(d, device[k])
        for i, L in enumerate(LENS3):
            assert torch.equal(d[i, :L], p[i, :L]), (k, i)
            assert not p[i, L:].any(), (k, i)
            assert d[i, :L].abs().sum(-1).min() > 0
        if pad == EOT:
            assert d[0, 76].any() and d[2, 76].any()          # the padded positions a pipeline cross-attends to
    if pad == EOT:      # the causal mask: rows in front of the EOT do not see what the pad slots hold
        other = states(m, make_tokens(LENS3, 0, seed=3))
        for d, o in zip(dense, other):
            for i, L in enumerate(LENS3):
                assert torch.equal(d[i, :L], o[i, :L])


def project_rows(m, xg):
    """leaf_op_project_rows on given fp32 rows with the model's ln_final / text_projection -> (xn_scratch, features)"""
    from leaf_amd import _lib
    M, d, D = xg.shape[0], m.cfg.width, m.cfg.embed_dim
    xn, out = torch.empty(M, d, device="cuda"), torch.empty(M, D, device="cuda")
    p = m.params
    _lib.check(_lib.lib().leaf_op_project_rows(ptr(xg), ptr(p["ln_final.weight"]), ptr(p["ln_final.bias"]), C.c_float(m.cfg.ln_eps),
                                               ptr(p["text_projection"]), ptr(xn), ptr(out), M, d, D, 0, stream()), "project_rows")
    return xn, out


@pytest.mark.parametrize("trim", [0, 1])
@pytest.mark.parametrize("mode", ["rowsafe", "fast", "precise"])
def test_vitl_tap_rows_are_the_rows_encode_text_pools(mode, trim):
    name = "ViT-L-14-quickgelu"
    m = model(name, SEEDS[name][0])
    precise = mode == "precise"
    t = make_tokens(LENS3, EOT, seed=4)
    eot = torch.tensor(LENS3, device="cuda") - 1
    rows = torch.arange(3, device="cuda")
    try:
        if not precise:
            m.set_precision(mode)
        m.set_option("last_layer_trim", trim)
        want = m.encode_text(t, precise=precise)
        L = m.cfg.layers
        (raw, normed), feat = m.encode_text_hidden(t, layers=(L, L), final_ln=(False, True), precise=precise, want_features=True)
        xn, out = project_rows(m, raw[rows, eot].contiguous())
        assert same(out, want)                                # the (layers, 0) EOT row IS the row the projection reads
        assert same(xn, normed[rows, eot])                    # ... and the tap's ln_final IS that call's LayerNorm
        assert same(feat, want)
    finally:
        m.set_precision("rowsafe")
        m.set_option("last_layer_trim", 1)


def test_vitl_pass_large_enough_for_the_fused_attention_launch():
    """96 sequences of 60 .. 77 rows: at >= 256 (256-row tile, head) items forward_all sends a chunk through the fused QKV + attention
    launch, which keeps q|k|v on chip -- the taps read the residual stream behind each block all the same"""
    name = "ViT-L-14-quickgelu"
    m = model(name, SEEDS[name][0])
    lens = [60 + (7 * i) % 18 for i in range(96)]
    t = make_tokens(lens, EOT, seed=8)
    L = m.cfg.layers
    eot = torch.tensor(lens, device="cuda") - 1
    rows = torch.arange(96, device="cuda")
    (mid, raw, normed), feat = m.encode_text_hidden(t, layers=(L - 1, L, L), final_ln=(False, False, True), want_features=True)
    assert same(feat, m.encode_text(torch.from_numpy(t).cuda()))            # the dense pass of the same shape
    xn, out = project_rows(m, raw[rows, eot].contiguous())
    assert same(out, feat) and same(xn, normed[rows, eot])
    packed = m.encode_text_hidden(t, layers=(L - 1, L, L), final_ln=(False, False, True), seq_lens=None)
    for d, p in zip((mid, raw, normed), packed):
        for i, n in enumerate(lens):
            assert torch.equal(d[i, :n], p[i, :n]) and not p[i, n:].any(), i


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_all_taps_in_one_pass_equal_one_pass_per_tap_and_change_no_feature_bit(name, precise):
    m = model(name, SEEDS[name][0])
    t = make_tokens(LENS3, EOT, seed=5)
    layers, lns = all_taps(m.cfg.layers)
    want = m.encode_text(t, precise=precise)
    together, feat = states(m, t, precise=precise, want_features=True)
    assert same(feat, want)
    assert same(m.encode_text_hidden(t, layers=(), want_features=True, precise=precise)[1], want)          # no tap at all
    for k, (l, ln) in enumerate(zip(layers, lns)):
        (alone,), f = m.encode_text_hidden(t, layers=(l,), final_ln=ln, precise=precise, want_features=True)      # l < layers: trimmed last block
        assert same(alone, together[k]), (l, ln)
        assert same(f, want), (l, ln)
        (stopped,) = m.encode_text_hidden(t, layers=(l,), final_ln=ln, precise=precise)                           # stops behind block l - 1
        assert same(stopped, together[k]), (l, ln)
    fn, = m.encode_text_hidden(t, layers=(-1,), precise=precise, want_features=True, normalize=True)[1:]
    assert same(fn, m.encode_text(t, normalize=True, precise=precise))


@pytest.mark.parametrize("name", ["tiny-test-quickgelu", "ViT-L-14-quickgelu"])
def test_chunked_pass_writes_every_chunk_at_its_place(name):
    m = model(name, SEEDS[name][0])
    t = make_tokens(LENS5, EOT, seed=6)
    whole, feat = states(m, t, want_features=True)
    whole_packed = states(m, t, seq_lens=None)
    try:
        m.set_option("chunk", 2)
        chunked, cfeat = states(m, t, want_features=True)                  # 2 + 2 + 1 sequences
        chunked_packed = states(m, t, seq_lens=None)                       # a row budget of 154: chunks of uneven sequence counts
    finally:
        m.set_option("chunk", 4096)
    assert same(cfeat, feat)
    for a, b, c, d in zip(whole, chunked, whole_packed, chunked_packed):
        assert same(a, b) and same(c, d)


@pytest.mark.parametrize("name,dtype", [("tiny-test", "fp16"), ("tiny-test", "bf16"), ("ViT-L-14-quickgelu", "fp16"), ("ViT-L-14-quickgelu", "bf16")])
def test_16_bit_output_is_the_rounded_fp32_output(name, dtype):
    m = model(name, SEEDS[name][0], dtype)
    half = torch.float16 if dtype == "fp16" else torch.bfloat16
    for kw in (dict(), dict(seq_lens=None)):
        t = make_tokens(LENS3, EOT, seed=7)
        wide = states(m, t, **kw)
        narrow = states(m, t, dtype=half, **kw)
        for w, n in zip(wide, narrow):
            assert n.dtype == half and same(w.to(half), n)
    with pytest.raises(ValueError):
        states(m, t, dtype=torch.float16 if dtype == "bf16" else torch.bfloat16)
    with pytest.raises(ValueError):
        states(m, t, dtype=half, precise=True)


def test_empty_batch_and_bad_arguments():
    m = model("tiny-test", SEEDS["tiny-test"][0])
    (e,), f = m.encode_text_hidden(np.zeros((0, 77), np.int32), want_features=True)
    assert e.shape == (0, 77, 128) and f.shape == (0, 64) and e.is_cuda
    from leaf_amd._lib import LeafHipError
    with pytest.raises(LeafHipError, match="are both"):
        m.encode_text_hidden(make_tokens(LENS3, 0, 1), layers=(-1, 2))


# =============================================================================================== block 2: against fp32
def ref_tower(w, cfg, tokens):
    """fp32 torch-CPU restatement of the text tower (src/open_clip/transformer.py text forward) that keeps every layer:
    (hidden_states: layers + 1 arrays [N, 77, d], ln_final of each of them, the projected pooled features)"""
    F = torch.nn.functional
    p = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()}
    tok = torch.from_numpy(np.asarray(tokens)).long()
    N, T = tok.shape
    d, H = cfg.width, cfg.heads
    mask = torch.full((T, T), float("-inf")).triu(1)
    x = p["token_embedding.weight"][tok] + p["positional_embedding"][:T]
    hs = [x]
    for i in range(cfg.layers):
        q = f"transformer.resblocks.{i}."
        xn = F.layer_norm(x, (d,), p[q + "ln_1.weight"], p[q + "ln_1.bias"], cfg.eps)
        qkv = F.linear(xn, p[q + "attn.in_proj_weight"], p[q + "attn.in_proj_bias"]).view(N, T, 3, H, d // H)
        qh, kh, vh = (qkv[:, :, j].transpose(1, 2) for j in range(3))
        att = torch.softmax(qh @ kh.transpose(-1, -2) / (d // H) ** 0.5 + mask, -1)
        x = x + F.linear((att @ vh).transpose(1, 2).reshape(N, T, d), p[q + "attn.out_proj.weight"], p[q + "attn.out_proj.bias"])
        xn = F.layer_norm(x, (d,), p[q + "ln_2.weight"], p[q + "ln_2.bias"], cfg.eps)
        h = F.linear(xn, p[q + "mlp.c_fc.weight"], p[q + "mlp.c_fc.bias"])
        h = h * torch.sigmoid(1.702 * h) if cfg.quick_gelu else F.gelu(h)
        x = x + F.linear(h, p[q + "mlp.c_proj.weight"], p[q + "mlp.c_proj.bias"])
        hs.append(x)
    ln = [F.layer_norm(v, (d,), p["ln_final.weight"], p["ln_final.bias"], cfg.eps) for v in hs]
    feat = ln[-1][torch.arange(N), tok.argmax(-1)] @ p["text_projection"]
    return [v.numpy() for v in hs], [v.numpy() for v in ln], feat.numpy()


_REFS = {}


def reference(name, seed):
    """(weights, tokens, hidden_states, their ln_final, features) of one (config, seed): the three sequences padded with 0 and the
    same three padded with the EOT id, computed once per module and left unchanged"""
    if (name, seed) not in _REFS:
        cfg = CONFIGS[name]
        w = O.init_weights(cfg, seed=seed)
        t = np.concatenate([make_tokens(LENS3, 0, seed=100 + seed), make_tokens(LENS3, EOT, seed=100 + seed)])
        _REFS[(name, seed)] = (w, t) + ref_tower(w, cfg, t)
    return _REFS[(name, seed)]


def worst_rows(name, seed, precise):
    """worst rel-L2 row per tap kind of encode_text_hidden (dense: all 6 x 77 rows, pad slots included) against ``reference``:
    embed = hidden_states[0]; blocks = hidden_states[1 .. layers]; final_ln = last_hidden_state; skip_ln = ln_final(hidden_states[-2])"""
    w, t, hs, ln, feat = reference(name, seed)
    m = model(name, seed)
    L = m.cfg.layers
    got, gfeat = states(m, t, precise=precise, want_features=True)
    got = [g.cpu().numpy() for g in got]
    r = {"embed": row_rel_l2(got[0], hs[0]).max(),
         "blocks": max(row_rel_l2(got[l], hs[l]).max() for l in range(1, L + 1)),
         "final_ln": row_rel_l2(got[L + 1], ln[L]).max(),
         "skip_ln": row_rel_l2(got[L + 2], ln[L - 1]).max(),
         "features": row_rel_l2(gfeat.cpu().numpy(), feat).max()}
    return {k: float(v) for k, v in r.items()}


# 2 x the worst row measured on the MI355X with SEEDS[name][0] (the literal is the measured figure; the rows of SEEDS[name][1], on which
# nothing was tuned, came out at 0.93 .. 1.18 of it).  "features": the pooled embedding of the same pass, for text_embeds against HF.
# The embedding of an fp32 stream is the exact fp32 sum, so its bound is 0; on the 16 + 8-bit stream it is the format's 2^-16.
# ViT-L's last_hidden_state rows (final_ln, 8.3e-4 worst) stay inside the project's 1e-3 feature gate.
BOUNDS = {
    ("tiny-test", False): {"embed": 0.0, "blocks": 2 * 9.096e-4, "final_ln": 2 * 9.151e-4, "skip_ln": 2 * 7.707e-4, "features": 2 * 7.763e-4},
    ("tiny-test-quickgelu", False): {"embed": 0.0, "blocks": 2 * 8.696e-4, "final_ln": 2 * 8.684e-4, "skip_ln": 2 * 7.939e-4, "features": 2 * 8.905e-4},
    ("ViT-L-14-quickgelu", False): {"embed": 2 * 5.893e-6, "blocks": 2 * 8.422e-4, "final_ln": 2 * 8.337e-4, "skip_ln": 2 * 8.374e-4, "features": 2 * 7.309e-4},
    ("tiny-test", True): {"embed": 0.0, "blocks": 2 * 1.035e-6, "final_ln": 2 * 9.493e-7, "skip_ln": 2 * 1.045e-6, "features": 2 * 7.407e-7},
    ("tiny-test-quickgelu", True): {"embed": 0.0, "blocks": 2 * 9.388e-7, "final_ln": 2 * 9.452e-7, "skip_ln": 2 * 8.944e-7, "features": 2 * 8.553e-7},
    ("ViT-L-14-quickgelu", True): {"embed": 0.0, "blocks": 2 * 1.034e-6, "final_ln": 2 * 1.030e-6, "skip_ln": 2 * 1.012e-6, "features": 2 * 1.124e-6},
}


@pytest.mark.parametrize("name", NAMES)
def test_reference_restatement_reproduces_the_torch_harness_on_its_pooled_row(name):
    from oracle.torch_cpu_harness import TorchTextTower
    for seed in SEEDS[name]:
        w, t, hs, ln, feat = reference(name, seed)
        with torch.no_grad():
            want = TorchTextTower(w, CONFIGS[name]).encode_text(torch.from_numpy(t).long()).numpy()
        r = row_rel_l2(feat, want).max()
        print(f"[hidden ref] {name} seed {seed}: pooled row vs TorchTextTower {r:.3e}")
        assert r < 2e-6            # fp32 reorder noise (softmax(q k^T) v against scaled_dot_product_attention)


@pytest.mark.parametrize("which", [0, 1], ids=["measured_seed", "second_seed"])
@pytest.mark.parametrize("precise", [False, True], ids=["fast_path", "precise"])
@pytest.mark.parametrize("name", NAMES)
def test_every_tap_against_the_fp32_reference(name, precise, which):
    seed = SEEDS[name][which]
    r = worst_rows(name, seed, precise)
    bounds = BOUNDS[(name, precise)]
    print(f"[hidden vs fp32] {name} seed {seed} precise {int(precise)}: " + "  ".join(f"{k} {v:.3e}" for k, v in r.items()))
    for k, b in bounds.items():
        assert r[k] <= b, (k, r[k], b)


@pytest.mark.parametrize("with_projection", [False, True])
@pytest.mark.parametrize("name", ["tiny-test", "tiny-test-quickgelu"])
def test_hf_clip_text_model_agrees_through_the_hf_encoder(name, with_projection, tmp_path):
    """transformers' CLIPTextModel(WithProjection), loaded from the directory write_hf_text_model writes, against LeafHFTextEncoder
    on EOT-padded ids.  HF is fp32 torch: it differs from ``ref_tower`` by reorder noise (asserted: 2e-5, the precise gate), so the
    engine is held to the bounds of the fp32 comparison plus that noise."""
    transformers = pytest.importorskip("transformers")
    from leaf_amd.checkpoint import write_hf_text_model
    from leaf_amd.hf_text import LeafHFTextEncoder
    seed = SEEDS[name][0]
    w, t, hs, ln, feat = reference(name, seed)
    t, hs, ln, feat = t[3:], [v[3:] for v in hs], [v[3:] for v in ln], feat[3:]
    m = model(name, seed)
    write_hf_text_model(str(tmp_path), m.state_dict(), m.cfg, with_projection=with_projection)
    cls = transformers.CLIPTextModelWithProjection if with_projection else transformers.CLIPTextModel
    hf = cls.from_pretrained(str(tmp_path)).eval()
    ids = torch.from_numpy(t).long()
    with torch.no_grad():
        want = hf(input_ids=ids, output_hidden_states=True)
    noise = 2e-5
    L = m.cfg.layers
    assert len(want.hidden_states) == L + 1
    for l in range(L + 1):
        assert row_rel_l2(want.hidden_states[l].numpy(), hs[l]).max() < noise
    assert row_rel_l2(want.last_hidden_state.numpy(), ln[L]).max() < noise
    for precise in (False, True):
        m.precise_encode = precise
        try:
            got = LeafHFTextEncoder(m, with_projection)(ids.cuda(), output_hidden_states=True)
        finally:
            m.precise_encode = False
        b = BOUNDS[(name, precise)]
        assert isinstance(got.hidden_states, tuple) and len(got.hidden_states) == L + 1
        fig = {"embed": row_rel_l2(got.hidden_states[0].cpu().numpy(), want.hidden_states[0].numpy()).max(),
               "blocks": max(row_rel_l2(got.hidden_states[l].cpu().numpy(), want.hidden_states[l].numpy()).max() for l in range(1, L + 1)),
               "final_ln": row_rel_l2(got.last_hidden_state.cpu().numpy(), want.last_hidden_state.numpy()).max()}
        pooled = (got.text_embeds, want.text_embeds) if with_projection else (got.pooler_output, want.pooler_output)
        fig["pooled"] = row_rel_l2(pooled[0].cpu().numpy(), pooled[1].numpy()).max()
        print(f"[hidden vs HF] {name} projection {int(with_projection)} precise {int(precise)}: " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()))
        for k in ("embed", "blocks", "final_ln"):
            assert fig[k] <= b[k] + noise, (k, fig[k])
        # pooler_output is a row of last_hidden_state; text_embeds the engine's feature row
        assert fig["pooled"] <= (b["features"] if with_projection else b["final_ln"]) + noise
        assert got[0] is (got.text_embeds if with_projection else got.last_hidden_state)


# =============================================================================================== encode_prompts.py
def test_encode_prompts_writes_what_the_model_computes(tmp_path):
    """the CLI end to end on the tiny tower: prompt_embeds are encode_text_hidden's rows of the EOT-padded ids, and with Charmer the
    perturbed captions, their embeddings and the clean/adversarial cosine come along"""
    import encode_prompts
    from leaf_amd.tokenizer import get_tokenizer
    prompts = ["a photo of a cat", "two dogs running on the beach", "a red car"]
    texts, out = tmp_path / "prompts.txt", tmp_path / "prompts.npz"
    texts.write_text("\n".join(prompts) + "\n")
    name, seed = "tiny-test-quickgelu", SEEDS["tiny-test-quickgelu"][0]
    encode_prompts.main(["--model", name, "--seed", str(seed), "--texts", str(texts), "--out", str(out), "--layer", "-2", "--no-final-ln",
                         "--batch-size", "2", "--attack-name", "charmer", "--k", "1", "--rho", "4"])
    z = np.load(out)
    ids = encode_prompts.pad_with_eot(get_tokenizer(name).encode_batch(prompts))
    assert np.array_equal(z["input_ids"], ids) and (ids[:, -1] == EOT).all() and list(z["captions"]) == prompts
    m = model(name, seed)
    (want,), feat = m.encode_text_hidden(ids, layers=(-2,), final_ln=False, want_features=True)
    assert z["prompt_embeds"].shape == (3, 77, 128) and np.array_equal(z["prompt_embeds"], want.cpu().numpy())
    assert np.array_equal(z["pooled_prompt_embeds"], feat.cpu().numpy())
    adv = list(z["perturbed_captions"])
    assert len(adv) == 3 and all(a != p for a, p in zip(adv, prompts))
    (want_adv,), feat_adv = m.encode_text_hidden(encode_prompts.pad_with_eot(get_tokenizer(name).encode_batch(adv)), layers=(-2,), final_ln=False,
                                                 want_features=True)
    assert np.array_equal(z["adv_prompt_embeds"], want_adv.cpu().numpy())
    cos = torch.nn.functional.cosine_similarity(feat, feat_adv).cpu().numpy()
    assert np.allclose(z["clean_adv_cosine"], cos, atol=1e-6) and (z["clean_adv_cosine"] < 1.0).all()
    assert int(z["layer"]) == -2 and int(z["final_ln"]) == 0
