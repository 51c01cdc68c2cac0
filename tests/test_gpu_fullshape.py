"""Parity at the shapes BASELINE.json names (configs[1]-[4]), not only on the tiny config:

* ViT-L: TextFARE loss + EVERY parameter gradient against the reference-generated fixture (tests/golden/vitl_grads_*.npz,
  torch.autograd on the reference's CLIP, utils_AT.py:317-337) and against the fp32 oracle tensor by tensor, then one AdamW step;
* ViT-L k=5 search (configs[2]): every one of the 10 scoring stages re-scored by the oracle, margin-aware arg-max;
* ViT-H with accum_freq=4 (configs[3], scripts/train_leaf_vith.sh:10-11): 4 micro-batch backwards == one 4x-batch backward,
  gradients against the oracle, one optimizer step per 4 micro-steps;
* ViT-bigG at B=256, rho=50 (configs[4]): workspace / K-V cache sizing and one real scoring stage through the
  size-independent properties dense == EOT-trimmed == prefix reuse;
* fp16 dynamic range: weights with planted massive activations (residual stream 1e3-1e4, c_fc pre-activations 1e2-1e3).
"""
import os

import numpy as np
import pytest

from oracle import text_oracle as O
from tests.util import TOL_ROW, rel_l2, row_rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _sample_index(numel, n_sample=257):
    """Same walk as tests/golden/make_golden_vitl_grads.py:sample_index."""
    n = min(n_sample, numel)
    stride = max(1, numel // n) | 1
    return (np.arange(n, dtype=np.int64) * stride * 7 + 3) % numel


def _grad(m, name):
    off, shape = m.layout[name]
    return m.grads[off: off + int(np.prod(shape))].view(shape)


# Per-tensor gradient rel-L2 against fp32 (16-bit MFMA operands, fp32 accumulation, fp32 residual/gradient streams, the
# reference's own amp regime).  The error grows with depth -- every block adds ~7 operand roundings to the data-gradient
# chain: measured on MI355X 3.5-4.0e-3 on the 2-layer config (bound 6e-3, tests/test_gpu_train.py), at ViT-L (12 layers)
# median 5.0e-3 / max 7.6e-3 (the biases and LayerNorm affine of blocks 0-1, the END of the chain), bound 1e-2.
_BF = os.environ.get("LEAF_GRAD_DTYPE", "").lower().startswith("b")
GRAD_TOL = 2e-2 if _BF else 1e-2


@pytest.mark.parametrize("tag,model", [("quickgelu", "ViT-L-14-quickgelu"), ("gelu", "ViT-L-14")])
def test_vitl_param_grads_vs_reference_fixture(torch_mod, golden_dir, tag, model):
    """P3/P4 at production shape: d=768, 12 layers, D=768 -- the project_rows + pooled-stash forward, the 256^2 / 64-row
    data-gradient GEMMs, the grouped TN weight gradients, ln_final / text_projection / embedding gradients."""
    from leaf_amd.model import create_model
    z = np.load(os.path.join(golden_dir, f"vitl_grads_{tag}.npz"))
    m = create_model(model, seed=1, trainable=True)
    toks = z["tokens"]
    anchor = torch_mod.from_numpy(z["anchor"]).cuda()
    feat = m.forward_train(toks)
    assert rel_l2(feat.cpu().numpy(), z["feat"]) < 1e-3 and row_rel_l2(feat.cpu().numpy(), z["feat"]).max() < TOL_ROW
    m.zero_grad()
    loss = float(m.backward(feat, anchor))
    assert abs(loss - float(z["loss"])) < 1e-3 * abs(float(z["loss"]))
    worst_n, worst_s = {}, {}
    names = [k[2:] for k in z.files if k.startswith("n:")]
    assert len(names) == len(m.layout) == 12 * m.cfg.layers + 5
    for k in names:
        g = _grad(m, k).reshape(-1)
        norm = float(torch_mod.linalg.vector_norm(g.double()))
        worst_n[k] = abs(norm / float(z["n:" + k]) - 1.0)
        idx = torch_mod.from_numpy(_sample_index(g.numel())).cuda()
        if k != "token_embedding.weight":       # the sampled rows of the embedding table are mostly untouched (zero) rows
            worst_s[k] = rel_l2(g[idx].cpu().numpy(), z["s:" + k])
    rows = z["tok_rows"].astype(np.int64)
    gt = _grad(m, "token_embedding.weight")
    worst_s["token_embedding.weight"] = rel_l2(gt[torch_mod.from_numpy(rows).cuda()].cpu().numpy(), z["g_tok_rows"].astype(np.float32))
    mask = torch_mod.ones(gt.shape[0], dtype=torch_mod.bool, device=gt.device)
    mask[torch_mod.from_numpy(rows).cuda()] = False
    assert float(gt[mask].abs().sum()) == 0.0, "embedding rows of unused token ids must get no gradient"
    print(f"{model}: loss {loss:.5f} (ref {float(z['loss']):.5f}); worst norm error {max(worst_n.values()):.2e} "
          f"({max(worst_n, key=worst_n.get)}), worst sampled rel-L2 {max(worst_s.values()):.2e} ({max(worst_s, key=worst_s.get)})")
    # norms: a random 6e-3 relative perturbation moves a norm by ~ its square; 2e-3 also catches a missing contribution.
    # samples: 257 elements per tensor, same statistics as the full-tensor rel-L2 (bound = the tiny-config bound)
    assert max(worst_n.values()) < 2e-3, {k: v for k, v in worst_n.items() if v >= 2e-3}
    bad = {k: v for k, v in worst_s.items() if v > GRAD_TOL}
    assert not bad, bad


def test_vitl_param_grads_and_adamw_vs_oracle(torch_mod):
    """All 149 tensors, full rel-L2 against the fp32 oracle backward (the oracle itself is pinned on these shapes by
    tests/test_oracle_golden.py::test_vitl_grad_fixture), then one fused AdamW step against the oracle's."""
    from leaf_amd.model import create_model
    cfg = O.CONFIGS["ViT-L-14-quickgelu"]
    w = O.init_weights(cfg, seed=1)
    m = create_model("ViT-L-14-quickgelu", seed=1, trainable=True)
    toks = O.synthetic_tokens(8, seed=33, min_len=4, max_len=50)
    rng = np.random.default_rng(9)
    f0 = O.encode_text(w, cfg, toks)
    anchor = (f0 + 0.6 * np.abs(f0).mean() * rng.standard_normal(f0.shape)).astype(np.float32)
    loss_o, feat_o, g_o = O.encode_text_backward(w, cfg, toks, anchor)
    feat = m.forward_train(toks)
    assert rel_l2(feat.cpu().numpy(), feat_o) < 1e-3
    m.zero_grad()
    loss = float(m.backward(feat, torch_mod.from_numpy(anchor).cuda()))
    assert abs(loss - loss_o) < 1e-3 * loss_o
    worst = {k: rel_l2(_grad(m, k).cpu().numpy(), g_o[k]) for k in m.layout}
    print("ViT-L all-tensor grad rel-L2: max", max(worst.values()), max(worst, key=worst.get),
          "median", float(np.median(list(worst.values()))))
    bad = {k: v for k, v in worst.items() if v > GRAD_TOL}
    assert not bad, bad
    # one fused AdamW step at full shape against the oracle's AdamW fed with the SAME (engine) gradients: step 1 of Adam is
    # -lr * g / (|g| + eps), i.e. sign-like, so feeding each side its own gradients would only count sign flips of ~0 elements
    keys = ("transformer.resblocks.5.mlp.c_fc.weight", "transformer.resblocks.0.ln_1.weight", "text_projection",
            "positional_embedding", "transformer.resblocks.11.attn.in_proj_bias", "ln_final.bias")
    sub_w = {k: m.params[k].cpu().numpy().copy() for k in keys}
    sub_g = {k: _grad(m, k).cpu().numpy().copy() for k in keys}
    mm = {k: np.zeros_like(v) for k, v in sub_w.items()}
    vv = {k: np.zeros_like(v) for k, v in sub_w.items()}
    O.adamw_step(sub_w, sub_g, mm, vv, 1, lr=1e-4, wd=1e-2, beta1=0.9, beta2=0.98, eps=1e-8)
    m.adamw_step(lr=1e-4, betas=(0.9, 0.98), eps=1e-8, weight_decay=1e-2)
    for k in keys:
        assert np.abs(m.params[k].cpu().numpy() - sub_w[k]).max() < 2e-6, k
        off, shape = m.layout[k]
        n = int(np.prod(shape))
        assert np.abs(m.exp_avg[off:off + n].cpu().numpy().reshape(shape) - mm[k]).max() <= 1e-6 * np.abs(mm[k]).max() + 1e-12
        assert np.abs(m.exp_avg_sq[off:off + n].cpu().numpy().reshape(shape) - vv[k]).max() <= 1e-5 * np.abs(vv[k]).max() + 1e-20


def test_vitl_k5_search_every_stage_rescored_by_oracle(torch_mod):
    """configs[2] (k=5): search_synthetic with prefix reuse on ViT-L; all 10 scoring calls (5 fused first stages, 5 second
    stages) are intercepted, their
    candidates re-scored by the fp32 oracle, and each arg-max must agree whenever the oracle's top-2 gap exceeds the
    measured loss error; stage inputs must chain (stage t+1 candidates derive from stage t's winner)."""
    from leaf_amd.model import LeafCLIPText, create_model, get_config
    from leaf_amd.step import StepConfig, search_synthetic
    name = "ViT-L-14-quickgelu"
    cfg = O.CONFIGS[name]
    w = O.init_weights(cfg, seed=1)
    m = create_model(name, seed=1)
    B, rho, k = 3, 12, 5
    base_np = O.synthetic_tokens(B, seed=5, min_len=6, max_len=24)
    lens = (base_np.argmax(-1) + 1).astype(np.int32)
    base = torch_mod.from_numpy(base_np.astype(np.int32)).cuda()
    anchor = m.encode_text(base_np)
    anchor_o = O.encode_text(w, cfg, base_np[:, :int(lens.max())])
    assert rel_l2(anchor.cpu().numpy(), anchor_o) < 1e-3
    calls = []
    real = m.score_candidates

    def spy(tokens, anchor_, rho_, objective="l2", **kw):
        kw.pop("want_loss", None)
        kw["want_features"] = True
        idx, feat, loss = real(tokens, anchor_, rho_, objective, want_loss=True, **kw)
        calls.append((tokens.detach().cpu().numpy().copy(), idx.cpu().numpy().copy(), loss.cpu().numpy().copy(),
                      feat.cpu().numpy().copy()))
        return idx, feat
    real_fused = m.score_candidates_fused

    def spy_fused(base_tokens, base_lens, tokens, anchor_, rho_, seq_lens, prefix_lens, objective="l2", **kw):
        # the first stage of every edit: the clean captions' K/V pass rides in the same launches (leaf_score_pass with kv_write)
        idx, feat, kv, loss = real_fused(base_tokens, base_lens, tokens, anchor_, rho_, seq_lens, prefix_lens, objective,
                                         want_features=True, want_loss=True)
        calls.append((tokens.detach().cpu().numpy().copy(), idx.cpu().numpy().copy(), loss.cpu().numpy().copy(),
                      feat.cpu().numpy().copy()))
        return idx, feat, kv
    # the second stage of every edit goes through the prepare / run pair (prepared before the host waits for the first stage's winners)
    real_prep, real_run = m.score_candidates_prepare, m.score_candidates_run

    def spy_prep(tokens, anchor_, rho_, objective="l2", want_features=True, want_loss=False, **kw):
        return real_prep(tokens, anchor_, rho_, objective, want_features=True, want_loss=True, **kw)

    def spy_run(plan, prefix_lens):
        idx, feat, loss = real_run(plan, prefix_lens)
        calls.append((plan.tokens.detach().cpu().numpy().copy(), idx.cpu().numpy().copy(), loss.cpu().numpy().copy(),
                      feat.cpu().numpy().copy()))
        return idx, feat
    m.score_candidates = spy
    m.score_candidates_fused = spy_fused
    m.score_candidates_prepare, m.score_candidates_run = spy_prep, spy_run
    adv = search_synthetic(m, anchor, base, StepConfig(rho=rho, k_adv=k), seed=3, base_lens=lens, prefix_reuse=True)
    m.score_candidates = real
    m.score_candidates_fused = real_fused
    m.score_candidates_prepare, m.score_candidates_run = real_prep, real_run
    assert len(calls) == 2 * k
    L = int(lens.max())
    cur = base_np.copy()
    for t, (toks, idx, loss, feat) in enumerate(calls):
        cand = toks.reshape(B, rho, 77)
        # every candidate differs from the current sentence in at most one position
        assert ((cand != cur[:, None, :]).sum(-1) <= 1).all()
        idx_o, best_o, loss_o = O.score_candidates(w, cfg, cand[:, :, :L], anchor_o)
        err = np.abs(loss - loss_o).max(-1)
        assert np.allclose(loss, loss_o, rtol=4e-3, atol=4e-3 * np.abs(loss_o).max()), (t, np.abs(loss - loss_o).max())
        srt = np.sort(loss_o, -1)
        gap = srt[:, -1] - srt[:, -2]
        for b in range(B):
            assert idx[b] == int(np.argmax(loss[b]))
            if gap[b] > 4 * err[b]:
                assert idx[b] == idx_o[b], (t, b)
            assert loss_o[b, idx[b]] >= loss_o[b, idx_o[b]] - 4 * err[b] - 1e-6
            assert rel_l2(feat[b], O.encode_text(w, cfg, cand[b, idx[b], :L][None])[0]) < TOL_ROW
        if t % 2 == 1:
            cur = cand[np.arange(B), idx]
    assert np.array_equal(adv.cpu().numpy(), cur), "the search must return the last stage's winners"
    # (no monotonicity claim over the k edits: an edit's candidates need not contain the unedited sentence, so the greedy
    # winner's distance to the anchor may drop from one edit to the next -- in the reference as here)


def test_vith_accum4_equals_one_4x_batch(torch_mod):
    """configs[3]: --accum-freq 4 (utils_AT.py:334-362: loss / accum_freq per micro-batch, one optimizer step per 4).
    The four accumulated micro-batch backwards must equal ONE backward of the 4x batch, and both the fp32 oracle."""
    from leaf_amd.model import LeafCLIPText, create_model, get_config
    from leaf_amd.step import StepConfig, train_step_tokens
    name = "ViT-H-14"
    cfg = O.CONFIGS[name]
    w = O.init_weights(cfg, seed=2)
    m = create_model(name, seed=2, trainable=True)
    toks = O.synthetic_tokens(8, seed=17, min_len=5, max_len=40)
    rng = np.random.default_rng(4)
    f0 = O.encode_text(w, cfg, toks)
    anchor = (f0 + 0.6 * np.abs(f0).mean() * rng.standard_normal(f0.shape)).astype(np.float32)
    ta = torch_mod.from_numpy(anchor).cuda()
    # one backward of the whole batch
    feat = m.forward_train(toks)
    assert rel_l2(feat.cpu().numpy(), f0) < 1e-3
    m.zero_grad()
    loss_full = float(m.backward(feat, ta))
    g_full = m.grads.clone()
    # four micro-batches of 2 with accum_scale 1/4
    m.zero_grad()
    losses = []
    for i in range(4):
        sl = slice(2 * i, 2 * i + 2)
        f = m.forward_train(toks[sl])
        losses.append(float(m.backward(f, ta[sl], accum_scale=0.25)))
    assert abs(np.mean(losses) - loss_full) < 1e-5 * loss_full
    worst = {}
    for k, (off, shape) in m.layout.items():
        n = int(np.prod(shape))
        worst[k] = rel_l2(m.grads[off:off + n].cpu().numpy(), g_full[off:off + n].cpu().numpy())
    print("ViT-H accum-4 vs one batch: worst per-tensor rel-L2", max(worst.values()), max(worst, key=worst.get))
    # different power-of-two loss scales / row packings per micro-batch: agreement to 16-bit operand noise, not bit-exact
    assert max(worst.values()) < GRAD_TOL
    loss_o, _, g_o = O.encode_text_backward(w, cfg, toks, anchor)
    assert abs(loss_full - loss_o) < 1e-3 * loss_o
    worst_o = {k: rel_l2(_grad(m, k).cpu().numpy(), g_o[k]) for k in m.layout}
    print("ViT-H accumulated grads vs oracle: max", max(worst_o.values()), max(worst_o, key=worst_o.get))
    bad = {k: v for k, v in worst_o.items() if v > 1.4 * GRAD_TOL}     # 24 layers deep
    assert not bad, bad
    # the token-id step API: 4 micro-steps -> exactly one optimizer step, weights change only then
    frozen = LeafCLIPText(get_config(name), device="cuda:0").copy_from(m)
    sc = StepConfig(rho=4, k_adv=2, lr=1e-4, wd=1e-4, accum_freq=4)
    base = torch_mod.from_numpy(toks[:2].astype(np.int32)).cuda()
    lens = (toks[:2].argmax(-1) + 1).astype(np.int32)
    p_before = m.flat.clone()
    m.opt_step = 0
    for mi in range(4):
        train_step_tokens(m, frozen, base, sc, seed=mi, micro_index=mi, base_lens=lens)
        if mi < 3:
            assert torch_mod.equal(m.flat, p_before), "no optimizer step before the last micro-batch"
    assert m.opt_step == 1 and not torch_mod.equal(m.flat, p_before)


def test_bigg_b256_sizing_and_scoring_stage_properties(torch_mod):
    """configs[4]: ViT-bigG-14 (d=1280, 32 layers), B=256, rho=50 -> 12,800 candidates per stage.  Sizing from the C ABI
    (everything resident in 288 GB), then ONE real stage at that size: dense == EOT-trimmed == prefix reuse bit for bit
    (losses, winners, winner features), and the winners' features against the fp32 oracle."""
    from leaf_amd.model import create_model
    name = "ViT-bigG-14"
    m = create_model(name, seed=2)
    lib = m._lib
    B, rho = 256, 50
    ws_score = lib.leaf_text_workspace_bytes(m._h, B * rho, 1)
    kv = lib.leaf_text_kv_bytes(m._h, B)
    stash = lib.leaf_text_stash_bytes(m._h, B)
    ws_train = lib.leaf_text_workspace_bytes(m._h, B, 2)
    resident = 4 * m.n_params * 4 + 2 * m.w16.numel() + ws_score + kv + stash + ws_train
    print(f"bigG B=256: params {m.n_params / 1e6:.1f} M; scoring workspace {ws_score / 2**30:.2f} GiB, K/V cache {kv / 2**30:.2f} GiB, "
          f"training stash {stash / 2**30:.2f} GiB, training workspace {ws_train / 2**30:.2f} GiB; resident total {resident / 2**30:.1f} GiB")
    assert resident < 0.5 * 288e9
    g = torch_mod.Generator().manual_seed(7)
    base = O.synthetic_tokens(B, seed=101, min_len=8, max_len=40)
    lens = (base.argmax(-1) + 1).astype(np.int32)
    rng = np.random.default_rng(8)
    pos = 1 + (rng.random((B, rho)) * (lens[:, None] - 2)).astype(np.int64)
    cand = np.repeat(base[:, None, :], rho, axis=1)
    cand[np.arange(B)[:, None], np.arange(rho)[None, :], pos] = rng.integers(1, 49406, size=(B, rho))
    cand[:, 0] = base                      # a no-op candidate per caption
    flat = cand.reshape(-1, 77)
    cand_lens = np.repeat(lens, rho)
    neq = cand != base[:, None, :]
    pl = neq.argmax(-1)
    pl[~neq.any(-1)] = 77
    anchor = m.encode_text(base) + 0.05
    tflat = torch_mod.from_numpy(flat.astype(np.int32)).cuda()
    m.trim_rows = False
    i_d, f_d, l_d = m.score_candidates(tflat, anchor, rho, "l2", want_loss=True)
    m.trim_rows = True
    i_t, f_t, l_t = m.score_candidates(tflat, anchor, rho, "l2", want_loss=True, seq_lens=cand_lens)
    kvc = m.encode_text_kv(base, seq_lens=lens)
    i_p, f_p, l_p = m.score_candidates(tflat, anchor, rho, "l2", want_loss=True, seq_lens=cand_lens, prefix_lens=pl.reshape(-1), kv=kvc)
    assert torch_mod.equal(l_d, l_t) and torch_mod.equal(i_d, i_t) and torch_mod.equal(f_d, f_t), "dense != EOT-trimmed"
    assert torch_mod.equal(l_t, l_p) and torch_mod.equal(i_t, i_p) and torch_mod.equal(f_t, f_p), "trimmed != prefix reuse"
    assert bool(torch_mod.isfinite(l_p).all())
    # the no-op candidate reproduces the clean caption's embedding exactly: loss = 0.05^2 * D
    assert np.allclose(l_p[:, 0].cpu().numpy(), 0.05 ** 2 * m.cfg.embed_dim, rtol=1e-3)
    # a few winners against the oracle
    cfg = O.CONFIGS[name]
    w = O.init_weights(cfg, seed=2)
    pick = [0, 100, 255]
    idx = i_p.cpu().numpy()
    want = O.encode_text(w, cfg, cand[pick, idx[pick]][:, :int(lens.max())])
    assert row_rel_l2(f_p.cpu().numpy()[pick], want).max() < TOL_ROW


def _plant_outliers(w, cfg, rng, kind):
    """Two planted-outlier models.
    'sot_sink': the pattern pretrained transformers show -- a MASSIVE activation at one token (here SOT: two residual
    channels at +2500 / -4000 from the embedding on, the 'attention sink'), one outlier DIMENSION shared by all tokens
    (~50x the typical magnitude), a few c_fc units with pre-activations of 1e2-1e3; LayerNorm gains of the massive channels
    attenuated as trained models learn to.  The embedding stays caption-dependent.
    'all_tokens': VERDICT r1's literal recipe -- c_proj / out_proj rows and biases scaled so that EVERY token's residual
    stream reaches ~5e3 in two channels, c_fc rows scaled for pre-activations of several hundred.  Here the common offset
    dominates the embedding (the caption-dependent part is a few % of its norm)."""
    d = cfg.width
    ch = [7, d // 2 + 3]
    if kind == "sot_sink":
        w["token_embedding.weight"][cfg.vocab_size - 2, ch] = np.array([2500.0, -4000.0], dtype=np.float32)
        w["positional_embedding"][:, 101] += 1.5
    else:
        for l in (0, 1):
            p = f"transformer.resblocks.{l}."
            w[p + "mlp.c_proj.weight"][ch] *= 400.0
            w[p + "mlp.c_proj.bias"][ch] += np.array([1500.0, -2500.0], dtype=np.float32)
            w[p + "attn.out_proj.weight"][ch[0]] *= 150.0
    for l in range(cfg.layers):
        p = f"transformer.resblocks.{l}."
        for ln in ("ln_1", "ln_2"):
            w[p + ln + ".weight"][ch] *= 0.05
        rows = rng.choice(4 * d, size=6, replace=False)
        w[p + "mlp.c_fc.weight"][rows] *= 40.0
        w[p + "mlp.c_fc.bias"][rows[:3]] += 60.0
        w[p + "mlp.c_fc.bias"][rows[3:]] += 300.0 if kind == "all_tokens" else 0.0
    w["ln_final.weight"][ch] *= 0.05
    return ch


@pytest.mark.parametrize("kind", ["sot_sink", "all_tokens"])
def test_fp16_range_with_planted_massive_activations(torch_mod, kind):
    """pretrained CLIP text towers carry residual-stream outliers; the engine stores LN outputs, QKV,
    attention outputs and MLP hidden activations in fp16 (conversions saturate at +-65504, never inf).  With planted
    outliers (magnitudes printed) the forward must stay finite, within 1e-3 rel-L2 of the fp32 oracle, pick the same
    candidates under the margin rule, and the training path must give finite gradients that match the oracle."""
    from leaf_amd.model import create_model
    name = "ViT-L-14-quickgelu"
    cfg = O.CONFIGS[name]
    w = O.init_weights(cfg, seed=1)
    _plant_outliers(w, cfg, np.random.default_rng(0), kind)
    B, rho = 6, 10
    base = O.synthetic_tokens(B, seed=61, min_len=6, max_len=30)
    L = int(base.argmax(-1).max()) + 1
    stash = []
    want = O.encode_text(w, cfg, base[:, :L], stash=stash)
    res_max = max(float(np.abs(s["x1"]).max()) for s in stash[:-1])
    pre_max = max(float(np.abs(s["pre"]).max()) for s in stash[:-1])
    pre_min_layer = min(float(np.abs(s["pre"]).max()) for s in stash[:-1])
    pd = np.linalg.norm(want[:, None] - want[None], axis=-1)[np.triu_indices(B, 1)]
    print(f"[{kind}] max |residual| {res_max:.3g}, max |c_fc pre-activation| {pre_max:.3g} (smallest per-layer max {pre_min_layer:.3g}), "
          f"||f|| {np.linalg.norm(want, axis=-1).mean():.3g}, caption-to-caption distance {pd.min():.3g}..{pd.max():.3g}")
    assert 1e3 <= res_max <= 2e4 and 1e2 <= pre_max <= 5e3 and pre_min_layer >= 50
    m = create_model(name, seed=1)
    m.load_state_dict(w)
    got_t = m.encode_text(base)
    assert bool(torch_mod.isfinite(got_t).all())
    got = got_t.cpu().numpy()
    r = row_rel_l2(got, want)
    # error relative to the caption-dependent component (what the search discriminates on)
    sig = rel_l2(got - got.mean(0), want - want.mean(0))
    print(f"[{kind}] rel-L2 global {rel_l2(got, want):.3e}, row max {r.max():.3e}; relative to the caption-dependent part {sig:.3e}")
    assert rel_l2(got, want) < 1e-3 and r.max() < TOL_ROW
    # fp16 operand-rounding emulation in the oracle (O.round_fp16) gives 1.0e-2 / 2.1e-2 here: a common offset costs
    # relative precision on the part that rides on it, in any 16-bit format (bf16: 8x more)
    assert sig < (3e-2 if kind == "sot_sink" else 8e-2)
    cand = O.synthetic_candidates(base, rho, seed=62)
    idx_o, _, loss_o = O.score_candidates(w, cfg, cand[:, :, :L], want)
    lens = np.repeat(base.argmax(-1) + 1, rho)
    neq = cand != base[:, None, :]
    kv = m.encode_text_kv(base)
    idx, feat, loss = m.score_candidates(cand.reshape(-1, 77), torch_mod.from_numpy(want).cuda(), rho, "l2", want_loss=True,
                                         seq_lens=lens, prefix_lens=neq.argmax(-1).reshape(-1), kv=kv)
    idx, loss = idx.cpu().numpy(), loss.cpu().numpy()
    assert np.isfinite(loss).all()
    err = np.abs(loss - loss_o).max(-1)
    srt = np.sort(loss_o, -1)
    agree = 0
    for b in range(B):
        if srt[b, -1] - srt[b, -2] > 4 * err[b]:
            assert idx[b] == idx_o[b]
        assert loss_o[b, idx[b]] >= loss_o[b, idx_o[b]] - 4 * err[b] - 1e-6
        agree += int(idx[b] == idx_o[b])
    print(f"[{kind}] arg-max agreement with the oracle {agree}/{B}")
    # training path on the same weights: finite gradients, loss and a spread of tensors against the oracle
    mt = create_model(name, seed=1, trainable=True)
    mt.load_state_dict(w)
    # anchor ~||f|| away from f (as every gradient fixture here): otherwise (f - anchor) is as small as the forward's own 3e-4 error
    anchor = (want + 0.5 * np.abs(want).mean() * np.random.default_rng(2).standard_normal(want.shape)).astype(np.float32)
    loss_ref, _, g_o = O.encode_text_backward(w, cfg, base[:, :L], anchor)
    f = mt.forward_train(base)
    mt.zero_grad()
    lt = float(mt.backward(f, torch_mod.from_numpy(anchor).cuda()))
    print(f"[{kind}] training loss {lt:.6g} (oracle {loss_ref:.6g})")
    assert bool(torch_mod.isfinite(mt.grads).all())
    keys = ("text_projection", "transformer.resblocks.11.mlp.c_fc.weight", "transformer.resblocks.0.attn.in_proj_weight",
            "transformer.resblocks.1.mlp.c_proj.weight", "transformer.resblocks.6.attn.out_proj.weight", "positional_embedding")
    worst = {k: rel_l2(_grad(mt, k).cpu().numpy(), g_o[k]) for k in keys}
    print(f"[{kind}] grads vs oracle:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert abs(lt - loss_ref) < 2e-3 * loss_ref
    assert max(worst.values()) < 2 * GRAD_TOL


@pytest.mark.parametrize("native", [False, True])
def test_config0_vitl_constrained_search_replays_reference_trace(torch_mod, golden_dir, native):
    """BASELINE.json configs[0] at its STATED size (VERDICT r4 missing-3): ViT-L, 8 captions, rho = 50, k = 1, --constrain.  The
    fixture is the reference's own ``attack_text`` run (utils_attacks.py:297-393; tests/golden/make_golden_vitl_attack.py):
    candidate strings, the reference's ``loss[B, rho]`` and arg-max of both stages, adversarial sentences, returned features.
    (1) the reference's candidates of each stage scored here: loss matrix within the k = 5 test's tolerance, arg-max under the
    margin rule, winners' features <= 1e-3 per row; (2) the search itself from the same numpy seed: same stage-1 candidates
    (RNG, mutation, constraint), same sentences unless a near-tie flipped -- then the pick must be within fp16 noise of the
    reference's best under the REFERENCE's loss."""
    import json
    from leaf_amd import attacks
    from leaf_amd.model import create_model
    from leaf_amd.tokenizer import SimpleTokenizer
    with open(os.path.join(golden_dir, "attack_vitl_k1_c1.json")) as f:
        t = json.load(f)
    with open(os.path.join(golden_dir, "mutation_kat.json")) as f:
        stub = json.load(f)["stub_words"]
    z = np.load(os.path.join(golden_dir, "attack_vitl_k1_c1.npz"))
    if native:
        from leaf_amd.native_text import NativeTokenizer
        tok = NativeTokenizer(n_threads=4)
    else:
        tok = SimpleTokenizer()
    m = create_model(t["model"], seed=t["weight_seed"])
    B, rho = len(t["sentences"]), t["rho"]
    assert (B, rho, t["k"], t["constrain"]) == (8, 50, 1, True)
    anchor = torch_mod.from_numpy(z["anchor"]).cuda()
    assert row_rel_l2(m.encode_text(tok.encode_batch(t["sentences"])).cpu().numpy(), z["anchor"]).max() < TOL_ROW
    # ---- (1) the reference's candidates, stage by stage
    for st in range(2):
        ids = np.asarray(tok.encode_batch(t["stage_candidates"][st]))
        assert ids.shape == (B * rho, 77)
        idx, feat, loss = m.score_candidates(ids, anchor, rho, "l2", want_loss=True)
        idx, feat, loss = idx.cpu().numpy(), feat.cpu().numpy(), loss.cpu().numpy()
        loss_r, pick_r = z["loss"][st], z["picks"][st]
        assert np.allclose(loss, loss_r, rtol=4e-3, atol=4e-3 * np.abs(loss_r).max()), (st, np.abs(loss - loss_r).max())
        err = np.abs(loss - loss_r).max(-1)
        srt = np.sort(loss_r, -1)
        gap = srt[:, -1] - srt[:, -2]
        for b in range(B):
            assert idx[b] == int(np.argmax(loss[b]))
            if gap[b] > 4 * err[b]:
                assert idx[b] == pick_r[b], (st, b)
            assert loss_r[b, idx[b]] >= loss_r[b, pick_r[b]] - 4 * err[b] - 1e-6
        # a caption whose candidates were ALL rejected (no dictionary word to lose): fifty copies of itself, first index wins
        for b in range(B):
            if t["candidates_equal_to_caption"][st * B + b] == rho:
                assert idx[b] == pick_r[b] == 0
        if st == 1:
            same = idx == pick_r
            assert same.sum() >= B - 1
            assert row_rel_l2(feat[same], z["feats"][same]).max() < TOL_ROW
    # ---- (2) the search itself
    attacks.set_dictionary(attacks.Dictionary(stub))
    try:
        got_trace, picks = [], []
        np.random.seed(t["seed"])
        feats, adv = attacks.attack_text_leaf(m, tok, list(t["sentences"]), anchor.clone(), objective="l2", n=rho, k=1,
                                              V=attacks.DEFAULT_V, constrain=True, return_trace=got_trace, return_picks=picks)
    finally:
        attacks.set_dictionary(None)
    ref = t["stage_candidates"]
    assert got_trace[0] == ref[0], "stage-1 candidates differ: RNG / mutation / constraint drift"
    if adv == t["adv"]:
        assert got_trace == ref
        assert [int(p) for p in picks[1]] == z["picks"][1].tolist()
        assert row_rel_l2(feats.cpu().numpy(), z["feats"]).max() < TOL_ROW
    else:
        s_div = next((i for i in range(2) if got_trace[i] != ref[i]), 2)
        assert s_div >= 1
        loss_r = z["loss"][s_div - 1]
        pick = loss_r[np.arange(B), np.asarray(picks[s_div - 1], dtype=int)]
        assert np.all(pick >= loss_r.max(-1) * (1 - 5e-3)), (s_div, pick, loss_r.max(-1))


def test_vitl_trained_like_spectrum_is_as_accurate_as_16_bit_operands_allow(torch_mod):
    """every embedding gate so far is on N(0, sigma) random init.  A tower with a TRAINED-LIKE weight structure
    (tests/util.py:trained_like_weights: power-law singular spectra, log-normal LayerNorm gains with outlier channels, non-zero
    biases, heavy-tailed token norms -- pretrained weights need the network) is less forgiving: the oracle's emulation of 16-bit
    operands with fp32 accumulation (what the MFMA path computes, up to summation order) is itself 1.1e-3 (median row) / 1.8e-3
    (worst of 12 rows) away from fp32 on it, and so is the emulation of the REFERENCE's own GPU arithmetic (TF32 operands, fp32
    stored intermediates: 1.2e-3 / 1.7e-3) -- north_star's 1e-3 is a statement about random-init towers.  The worst row is not a
    stable statistic here: some captions are ill-conditioned (making single sites EXACT in the emulation moves the worst row up as
    often as down, 1.5e-3 ... 2.4e-3; the GPU, a different summation order, measured 2.4e-3 with a median of 9.6e-4).  What is gated:
    the engine is as close to fp32 as its operand format allows (row median within 1.3x of the emulation's, worst row within 2x),
    stays finite, and the search still picks the oracle's candidates under the margin rule."""
    from leaf_amd.model import create_model
    from tests.util import trained_like_weights
    name = "ViT-L-14-quickgelu"
    cfg = O.CONFIGS[name]
    w = trained_like_weights(cfg, seed=0)
    B, rho = 12, 8
    base = O.synthetic_tokens(B, seed=71, min_len=4, max_len=40)
    L = int(base.argmax(-1).max()) + 1
    want = O.encode_text(w, cfg, base[:, :L])
    emu = O.encode_text(w, cfg, base[:, :L], rnd=O.RoundPolicy(O.round_fp16, lambda l, s, wh: s == "final"))
    r_emu = row_rel_l2(emu, want)
    m = create_model(name, seed=1)
    m.load_state_dict(w)
    got_t = m.encode_text(base)
    assert bool(torch_mod.isfinite(got_t).all())
    r = row_rel_l2(got_t.cpu().numpy(), want)
    print(f"[trained-like] GPU rows: max {r.max():.3e} median {np.median(r):.3e} | fp16-operand emulation: max {r_emu.max():.3e} "
          f"median {np.median(r_emu):.3e} | ||f|| {np.linalg.norm(want, axis=-1).mean():.3g}")
    assert r_emu.max() > 1.2e-3, "the emulation says this tower is no harder than random init: the generator changed"
    assert np.median(r) < 1.3 * np.median(r_emu) and r.max() < 2.0 * r_emu.max()
    assert r.max() < 4e-3
    cand = O.synthetic_candidates(base, rho, seed=72)
    idx_o, _, loss_o = O.score_candidates(w, cfg, cand[:, :, :L], want)
    idx, feat, loss = m.score_candidates(cand.reshape(-1, 77), torch_mod.from_numpy(want).cuda(), rho, "l2", want_loss=True)
    idx, loss = idx.cpu().numpy(), loss.cpu().numpy()
    err = np.abs(loss - loss_o).max(-1)
    srt = np.sort(loss_o, -1)
    for b in range(B):
        if srt[b, -1] - srt[b, -2] > 4 * err[b]:
            assert idx[b] == idx_o[b]
        assert loss_o[b, idx[b]] >= loss_o[b, idx_o[b]] - 4 * err[b] - 1e-6


def test_row_error_census_gate(torch_mod):
    """the per-row embedding gate on a LARGE sample instead of 8-24 rows.  2,040 ViT-L-quickgelu rows (40 synthetic
    captions + 50 single-edit candidates each, the benchmark model's weights) against the plain PyTorch CPU fp32 forward
    (oracle/torch_cpu_harness.py; the full census -- 12,928 rows of one configs[1] search and 2,000 rows per other tower -- is
    tests/row_error_census.py -> profiles/r06_row_error_census*.txt).  DEFAULT arithmetic ('rowsafe'): EVERY row within north_star's
    1e-3 with margin (census: max 8.7e-4 of 12,928).  'fast' (the rounds 1-5 arithmetic) is held to what the census supports: batch
    rel-L2 and P99 within 1e-3 (+2 %), i.e. about 1 % of its rows above 1e-3."""
    from leaf_amd.model import create_model
    from oracle import torch_cpu_harness as H
    name = "ViT-L-14-quickgelu"
    cfg = O.CONFIGS[name]
    w = O.init_weights(cfg, seed=1)
    base = O.synthetic_tokens(40, seed=1234)
    toks = np.concatenate([base, O.synthetic_candidates(base, 50, seed=1235).reshape(-1, 77)])
    L = int(toks.argmax(-1).max()) + 1
    torch_mod.set_num_threads(H.usable_cores())
    tower = H.TorchTextTower(w, cfg)
    with torch_mod.no_grad():
        ref = np.concatenate([tower.encode_text(torch_mod.from_numpy(toks[s:s + 120, :L].astype(np.int64))).numpy() for s in range(0, len(toks), 120)])
    m = create_model(name, seed=1)
    r = row_rel_l2(m.encode_text(toks).cpu().numpy(), ref)
    m.set_precision("fast")
    got_fast = m.encode_text(toks).cpu().numpy()
    rf = row_rel_l2(got_fast, ref)
    q = lambda a, p: float(np.quantile(a, p))
    print(f"[census gate] {len(toks)} rows  rowsafe: P50 {q(r, .5):.3e} P99 {q(r, .99):.3e} max {r.max():.3e} rows > 1e-3: {(r > 1e-3).sum()}   "
          f"fast: P50 {q(rf, .5):.3e} P99 {q(rf, .99):.3e} max {rf.max():.3e} rows > 1e-3: {(rf > 1e-3).sum()}")
    assert r.max() < TOL_ROW and q(r, .5) < 7.6e-4, "the default arithmetic must keep EVERY row of a large sample inside 1e-3"
    assert rel_l2(got_fast, ref) < 1e-3 and q(rf, .99) < 1.02e-3 and rf.max() < 1.25e-3
