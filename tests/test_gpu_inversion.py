"""Text embedding inversion (PEZ) on the GPU: the engine's pieces replay the REFERENCE's own trajectories teacher-forced -- every
step from the fixture's own state (tests/golden/tiny_pez.npz, written by tests/golden/make_golden_pez.py from
src/pez/optim_utils.py) -- then the ViT-L input gradient against the numpy oracle and ``invert_text`` end to end.

Free-running trajectories are NOT compared with the reference's: with lr 0.1 the projected ids change on almost every step, so a
16-bit forward legitimately takes another path after a few steps."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import text_oracle as O
from tests.util import ptr, rel_l2, stream

pytestmark = pytest.mark.gpu

SOT, EOT = 49406, 49407


def margin_bound(d):              # tests/test_gpu_nnproj.py, "MARGIN RULE"
    return 2.0 * d * 2.0 ** -23


@pytest.fixture(scope="module")
def env(golden_dir):
    import torch
    from leaf_amd.model import create_model
    assert torch.cuda.is_available()
    z = np.load(os.path.join(golden_dir, "tiny_pez.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    m = create_model("tiny-test-quickgelu", seed=12, trainable=True)
    cfg = O.TextCfg(128, 2, 2, 64, quick_gelu=True)
    w = O.init_weights(cfg, seed=12)
    return torch, m, z, meta, cfg, w


def _rows(ids_list):
    """token rows [SOT, ids, EOT, 0...] and lengths P + 2"""
    toks = np.zeros((len(ids_list), 77), np.int32)
    for i, ids in enumerate(ids_list):
        toks[i, 0], toks[i, 1:1 + len(ids)], toks[i, 1 + len(ids)] = SOT, ids, EOT
    return toks, np.array([len(i) + 2 for i in ids_list], np.int32)


def _prompt_rows(g, lens):
    """the gradient rows 1..P of every sequence out of the packed [rows, d] gradient"""
    cu = np.concatenate([[0], np.cumsum(lens)])
    return [g[cu[i] + 1: cu[i + 1] - 1] for i in range(len(lens))]


@pytest.fixture(scope="module")
def replay(env):
    """forward + cosine head + input gradient of all 4 x 30 recorded (ids, target) pairs in ONE batch: the sequences are independent"""
    torch, m, z, meta, cfg, w = env
    ids_list, targets, tag = [], [], []
    for c in range(4):
        for k in range(meta["iters"]):
            ids_list.append(z[f"c{c}_ids"][k])
            targets.append(z[f"c{c}_target"])
            tag.append((c, k))
    toks, lens = _rows(ids_list)
    feat = m.forward_train(toks, seq_lens=lens, pool_last=True)
    cos, g = m.cosine_input_grad(feat, torch.from_numpy(np.stack(targets)).cuda(), meta["loss_weight"])
    torch.cuda.synchronize()
    return toks, lens, tag, feat.cpu().numpy(), cos.cpu().numpy(), _prompt_rows(g.cpu().numpy(), lens)


def test_projection_reproduces_the_recorded_ids(env):
    torch, m, z, meta, cfg, w = env
    q = np.concatenate([z[f"c{c}_emb"][:-1].reshape(-1, 128) for c in range(4)])
    want = np.concatenate([z[f"c{c}_ids"].reshape(-1) for c in range(4)])
    ids, cosv = m.nn_project(torch.from_numpy(q).cuda())
    ids, cosv = ids.cpu().numpy(), cosv.cpu().numpy()
    t = w["token_embedding.weight"].astype(np.float64)
    q64 = q.astype(np.float64)
    ref = (q64 / np.linalg.norm(q64, axis=1, keepdims=True)) @ (t / np.linalg.norm(t, axis=1, keepdims=True)).T
    top2 = np.sort(np.partition(ref, -2, axis=1)[:, -2:], axis=1)
    clear = top2[:, 1] - top2[:, 0] > margin_bound(128)
    got = ref[np.arange(len(q)), ids]
    print(f"rows {len(q)}, decided by the margin {(~clear).sum()}, ids differing from the recording {(ids != want).sum()}, "
          f"max |cos - f64| {np.abs(cosv - got).max():.3e}")
    assert np.array_equal(ids[clear], want[clear])
    assert np.all(top2[~clear, 1] - got[~clear] <= margin_bound(128))
    assert (~clear).sum() <= 0.02 * len(q)
    assert np.abs(cosv - got).max() <= 128 * 2.0 ** -23


def test_forward_feature_on_recorded_ids(env, replay):
    """2e-3 rel-L2, what tests/test_gpu_pgd.py holds the tiny tower to.  The reference feature of a row whose prompt holds no SOT / EOT
    id is the oracle's encode_text (pinned to the reference by tests/test_oracle_golden.py); rows with one are covered by
    test_interior_eot_pools_at_the_last_row."""
    torch, m, z, meta, cfg, w = env
    toks, lens, tag, feat, cos, grads = replay
    plain = np.array([int(toks[i, 1:lens[i] - 1].max()) < SOT for i in range(len(lens))])
    assert plain.sum() >= 100
    want = O.encode_text(w, cfg, toks[plain].astype(np.int64))
    err = np.linalg.norm(feat[plain] - want, axis=1) / np.linalg.norm(want, axis=1)
    print(f"feature rel-L2 over {plain.sum()} rows: max {err.max():.3e}, batch {rel_l2(feat[plain], want):.3e}")
    assert rel_l2(feat[plain], want) < 2e-3


def test_cosine_on_recorded_ids(env, replay):
    torch, m, z, meta, cfg, w = env
    toks, lens, tag, feat, cos, grads = replay
    want = np.array([z[f"c{c}_cos"][k] for c, k in tag])
    print(f"max |cos - reference| {np.abs(cos - want).max():.3e}")
    assert np.abs(cos - want).max() < 4e-3


def test_gradient_on_recorded_ids(env, replay):
    """8e-3 rel-L2 per caption over its 30 recorded steps, the tolerance tests/test_gpu_pgd.py holds this backward chain to"""
    torch, m, z, meta, cfg, w = env
    toks, lens, tag, feat, cos, grads = replay
    for c in range(4):
        got = np.stack([grads[i] for i, (cc, k) in enumerate(tag) if cc == c])
        want = z[f"c{c}_grad"]
        step = [rel_l2(got[k], want[k]) for k in range(len(want))]
        print(f"caption {c} (P = {want.shape[1]}): gradient rel-L2 {rel_l2(got, want):.3e}, worst step {max(step):.3e}")
        assert rel_l2(got, want) < 8e-3


def test_adamw_update_from_the_recorded_gradient(env):
    """torch.optim.AdamW(lr 0.1, weight_decay 0.1) over the prompt rows, every step from the fixture's own embeddings and gradient,
    moments carried: the next recorded embeddings to 2e-6 (the bound of the AdamW-vs-oracle checks, tests/test_gpu_fullshape.py)"""
    torch, m, z, meta, cfg, w = env
    from leaf_amd import _lib
    lib = _lib.lib()
    worst = 0.0
    for c in range(4):
        emb, grad = z[f"c{c}_emb"], z[f"c{c}_grad"]
        m1 = torch.zeros(emb[0].shape, device="cuda")
        m2 = torch.zeros_like(m1)
        n = m1.numel()
        for k in range(meta["iters"]):
            p = torch.from_numpy(emb[k].copy()).cuda()
            g = torch.from_numpy(grad[k].copy()).cuda()
            _lib.check(lib.leaf_adamw_step(ptr(p), ptr(g), ptr(m1), ptr(m2), n, n, meta["lr"], 0.9, 0.999, 1e-8, meta["weight_decay"],
                                           k + 1, 1.0, stream()), "adamw")
            worst = max(worst, float(np.abs(p.cpu().numpy() - emb[k + 1]).max()))
    print(f"max |embedding after the step - reference| {worst:.3e}")
    assert worst < 2e-6


def test_interior_eot_pools_at_the_last_row(env):
    """id 49407 at an interior prompt position: the reference pools at the template's EOT slot.  Pooling at the first maximum id (the
    ordinary training forward) gives another feature, so this fails if pooling follows the ids."""
    torch, m, z, meta, cfg, w = env
    ids = z["interior_eot_ids"]
    toks, lens = _rows([ids])
    feat = m.forward_train(toks, seq_lens=lens, pool_last=True)
    cos, g = m.cosine_input_grad(feat, torch.from_numpy(z["interior_eot_target"][None]).cuda())
    f = feat.cpu().numpy()[0]
    got = _prompt_rows(g.cpu().numpy(), lens)[0]
    print(f"feature rel-L2 {rel_l2(f, z['interior_eot_feat']):.3e}, cos {float(cos[0]):.5f} vs {float(z['interior_eot_cos']):.5f}, "
          f"gradient rel-L2 {rel_l2(got, z['interior_eot_grad']):.3e}")
    assert rel_l2(f, z["interior_eot_feat"]) < 2e-3
    assert abs(float(cos[0]) - float(z["interior_eot_cos"])) < 4e-3
    assert rel_l2(got, z["interior_eot_grad"]) < 8e-3
    by_ids = m.forward_train(toks, seq_lens=lens).cpu().numpy()[0]
    assert rel_l2(by_ids, z["interior_eot_feat"]) > 5e-2
    # the entry needs the explicit lengths
    with pytest.raises(ValueError):
        m.forward_train(toks, pool_last=True)


@pytest.mark.parametrize("B,D,weight", [(5, 64, 1.0), (3, 768, 2.5), (2, 1280, 1.0)])
def test_cosine_head_alone_vs_float64(env, B, D, weight):
    torch = env[0]
    from leaf_amd import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(B * D)
    f = rng.standard_normal((B, D)).astype(np.float32)
    t = (0.6 * f + rng.standard_normal((B, D)) * 1.7).astype(np.float32)          # un-normalised target, cos ~ 0.3
    fd, td = torch.from_numpy(f).cuda(), torch.from_numpy(t).cuda()
    dout = torch.empty(B, D, device="cuda")
    cosv = torch.empty(B, device="cuda")
    ws = torch.zeros(64 + 2 * B, device="cuda")
    _lib.check(lib.leaf_op_cosine_head(ptr(fd), ptr(td), B, D, weight, ptr(dout), ptr(cosv), ptr(ws), stream()), "cosine_head")
    torch.cuda.synchronize()
    f64, t64 = f.astype(np.float64), t.astype(np.float64)
    nf, nt = np.linalg.norm(f64, axis=1, keepdims=True), np.linalg.norm(t64, axis=1, keepdims=True)
    c = (f64 * t64).sum(1, keepdims=True) / nf / nt
    want = -weight * (t64 / nf / nt - c * f64 / nf ** 2)                           # d [w (1 - cos)] / d f
    err = rel_l2(dout.cpu().numpy(), want)
    print(f"B {B} D {D}: upstream gradient rel-L2 {err:.3e} (bound {D * 2.0 ** -23:.3e}), cos error {np.abs(cosv.cpu().numpy() - c[:, 0]).max():.3e}")
    assert err <= D * 2.0 ** -23
    assert np.abs(cosv.cpu().numpy() - c[:, 0]).max() <= D * 2.0 ** -23


def test_large_tower_cosine_input_grad_vs_oracle(env):
    """ViT-L shapes, 4 captions.  The oracle's TextFARE backward with anchor_b = feat_b - (N / 2) g_b has the upstream gradient
    2 (feat - anchor) / N = g_b, the float64 gradient of the cosine loss: its d_embed is the reference.  8e-3 as
    tests/test_gpu_pgd.py::test_large_tower_input_grad_vs_oracle."""
    torch = env[0]
    from leaf_amd.model import create_model
    cfg = O.CONFIGS["ViT-L-14"]
    w = O.init_weights(cfg, seed=1)
    m = create_model("ViT-L-14", seed=1, trainable=True)
    toks = O.synthetic_tokens(4, seed=77, min_len=6, max_len=30)
    lens = (toks.argmax(-1) + 1).astype(np.int32)
    N = len(toks)
    rng = np.random.default_rng(4)
    feat_o = O.encode_text(w, cfg, toks).astype(np.float64)
    target = (feat_o + 0.5 * np.linalg.norm(feat_o, axis=1, keepdims=True) / np.sqrt(cfg.embed_dim)
              * rng.standard_normal(feat_o.shape)).astype(np.float32)
    t64 = target.astype(np.float64)
    nf, nt = np.linalg.norm(feat_o, axis=1, keepdims=True), np.linalg.norm(t64, axis=1, keepdims=True)
    c = (feat_o * t64).sum(1, keepdims=True) / nf / nt
    g_up = -(t64 / nf / nt - c * feat_o / nf ** 2)
    anchor = feat_o - (N / 2.0) * g_up
    _, _, g = O.encode_text_backward(w, cfg, toks, anchor, delta=np.zeros((N, 77, cfg.width), np.float32))
    feat = m.forward_train(toks, seq_lens=lens, pool_last=True)
    assert rel_l2(feat.cpu().numpy(), feat_o) < 1e-3
    cos, gd = m.cosine_input_grad(feat, torch.from_numpy(target).cuda())
    assert np.abs(cos.cpu().numpy() - c[:, 0]).max() < 4e-3
    keep = np.arange(77)[None, :] < lens[:, None]
    got = np.zeros((N, 77, cfg.width), np.float32)
    got[keep] = gd.cpu().numpy()
    err = rel_l2(got, g["d_embed"])
    print(f"ViT-L d_embed rel-L2 {err:.3e}, cos {cos.cpu().numpy()}")
    assert err < 8e-3


def test_table_norms_follow_the_weights(env):
    torch, m = env[0], env[1]
    x = m.params["token_embedding.weight"][[5, 77, 49407]].clone() * 3.0
    ids, cosv = m.nn_project(x)
    assert ids.tolist() == [5, 77, 49407] and m._vocab_inv is not None
    assert np.abs(cosv.cpu().numpy() - 1).max() < 128 * 2.0 ** -23
    m.load_state_dict(m.state_dict())
    assert m._vocab_inv is None
    assert m.nn_project(x)[0].tolist() == [5, 77, 49407]


CAPS = ["a photo of cat", "two people in the big park at sunset today", "cat"]


def test_invert_text_end_to_end(env):
    torch, m = env[0], env[1]
    from leaf_amd.inversion import invert_text
    from leaf_amd.tokenizer import SimpleTokenizer
    tok = SimpleTokenizer()
    a = invert_text(m, tok, captions=CAPS, iters=20, batch=3)
    b = invert_text(m, tok, captions=CAPS, iters=20, batch=3)
    assert [r["ids_rec"] for r in a] == [r["ids_rec"] for r in b] and [r["sim"] for r in a] == [r["sim"] for r in b]
    first = invert_text(m, tok, captions=CAPS, iters=1, batch=3)
    full = tok.encode_batch(CAPS)
    targets = m.encode_text(full, precise=True)
    for i, r in enumerate(a):
        assert set(r) >= {"original", "reconstructed", "ids_rec", "sim", "ids_orig"}
        assert r["original"] == CAPS[i] and r["ids_orig"] == full[i].tolist()
        assert len(r["ids_rec"]) == int((full[i] != 0).sum()) - 2
        assert r["reconstructed"] == tok.decode(r["ids_rec"])
        toks, _ = _rows([np.array(r["ids_rec"], np.int32)])
        f = m.encode_text(toks, precise=True)
        want = float(torch.nn.functional.cosine_similarity(f, targets[i:i + 1])[0])
        assert abs(r["sim"] - want) < 1e-6
        assert r["sim_loop"] >= first[i]["sim_loop"]    # the running best never falls behind the first iteration's cosine
    print("sim after 20 iterations:", [round(r["sim"], 4) for r in a], "loop:", [round(r["sim_loop"], 4) for r in a])


def test_first_iteration_of_a_batch_equals_each_caption_alone(env):
    torch, m = env[0], env[1]
    from leaf_amd.inversion import invert_text
    from leaf_amd.tokenizer import SimpleTokenizer
    tok = SimpleTokenizer()
    both = invert_text(m, tok, captions=CAPS, iters=1, batch=3)
    for i, cap in enumerate(CAPS):
        one = invert_text(m, tok, captions=[cap], iters=1)[0]
        assert one["ids_rec"] == both[i]["ids_rec"]
        assert abs(one["sim_loop"] - both[i]["sim_loop"]) < 4e-3 and abs(one["sim"] - both[i]["sim"]) < 4e-3
    # a bare target with an explicit prompt length, and a given start
    t = m.encode_text(tok.encode_batch(CAPS[:1]), precise=True)
    r = invert_text(m, tok, targets=t, prompt_len=4, iters=2, init_ids=[[320, 1125, 539, 2368]])[0]
    assert r["original"] is None and r["ids_orig"] is None and len(r["ids_rec"]) == 4
    with pytest.raises(ValueError):
        invert_text(m, tok, targets=t, iters=2)         # "match" needs captions
