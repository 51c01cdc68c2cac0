"""The float64 references of the training backward's kernels (tests/util.py: attn_bwd_seq_ref, ln_bwd_ref, pool_project_bwd_ref,
embed_bwd_ref, fare_ref), pinned on the CPU against torch float64 autograd of the plainly written operation and against np.add.at.
tests/test_gpu_backward_rows.py and test_layernorm_bwd hold the HIP kernels to these references."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import (BWD_LENS, attn_bwd_pack, attn_bwd_seq_ref, embed_bwd_ref, fare_ref, ln_bwd_ref, pool_project_bwd_ref, round16,
                        row_rel_l2)

REL = 1e-12


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / (np.abs(np.asarray(b)).max() + 1e-300))


@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("T", [1, 5, 33])
def test_attention_backward_reference_is_autograd_of_explicit_softmax_attention(T, H):
    rng = np.random.default_rng(10 * T + H)
    d = H * 64
    seq, do = rng.standard_normal((T, 3 * d)), rng.standard_normal((T, d))
    x = torch.tensor(seq, dtype=torch.float64, requires_grad=True)
    q, k, v = (x[:, i * d:(i + 1) * d].reshape(T, H, 64).transpose(0, 1) for i in range(3))
    mask = torch.full((T, T), float("-inf"), dtype=torch.float64).triu(1)
    out = (torch.softmax(q @ k.transpose(1, 2) / 8.0 + mask, -1) @ v).transpose(0, 1).reshape(T, d)
    out.backward(torch.tensor(do))
    got = attn_bwd_seq_ref(seq, do, H, "fp16", "fp16")
    assert _rel(got, x.grad.numpy()) <= REL
    if T == 1:
        assert not got[:, :2 * d].any() and np.array_equal(got[:, 2 * d:], do)       # P = 1: dq = dk = 0, dv = dO


def test_attention_backward_reference_converts_the_operands_once_when_the_types_differ():
    """ft != gt: P from the operands as given, every gradient product from q, k, v rounded to gt -- autograd of the same graph with
    the rounded copies wired in by hand (P detached from them)"""
    rng = np.random.default_rng(3)
    T, H = 17, 2
    d = H * 64
    seq, do = round16(rng.standard_normal((T, 3 * d)), "fp16"), round16(rng.standard_normal((T, d)), "bf16")
    got = attn_bwd_seq_ref(seq, do, H, "fp16", "bf16")
    # dv = P^T dO with the given operands' P; dq, dk through S = qg kg^T / 8 evaluated AT P (softmax Jacobian at the given P)
    for h in range(H):
        q, k, v = (seq[:, i * d + h * 64: i * d + (h + 1) * 64] for i in range(3))
        s = q @ k.T / 8.0 + np.triu(np.full((T, T), -np.inf), 1)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        g = do[:, h * 64:(h + 1) * 64]
        qg, kg, vg = round16(q, "bf16"), round16(k, "bf16"), round16(v, "bf16")
        dp = g @ vg.T
        ds = np.stack([(np.diag(p[i]) - np.outer(p[i], p[i])) @ dp[i] for i in range(T)]) / 8.0
        assert _rel(got[:, h * 64:(h + 1) * 64], ds @ kg) <= REL
        assert _rel(got[:, d + h * 64: d + (h + 1) * 64], ds.T @ qg) <= REL
        assert _rel(got[:, 2 * d + h * 64: 2 * d + (h + 1) * 64], p.T @ g) <= REL
    assert np.abs(got - attn_bwd_seq_ref(seq, do, H, "fp16", "fp16")).max() > 1e-4      # the conversion is not a no-op


@pytest.mark.parametrize("gt,whole", [("fp16", 2e-3), ("bf16", 1.2e-2)])
@pytest.mark.parametrize("ft", ["fp16", "bf16"])
@pytest.mark.parametrize("H", [1, 2])
def test_rounding_model_of_the_attention_backward_stays_inside_the_whole_matrix_tolerances(H, ft, gt, whole):
    """The GPU test's bound is 2 x the model's worst row / (row, 64-column slice) error on its own pack; that bound must not exceed
    the whole-matrix tolerances of test_attention_bwd_mfma (a condition on the inputs, checked here without a GPU)"""
    _, _, exact, model = attn_bwd_pack(5, BWD_LENS, H, ft, gt)
    assert (model != exact).any()
    for width in (3 * H * 64, 64):
        err = row_rel_l2(model.reshape(-1, width), exact.reshape(-1, width))
        assert 2.0 * err.max() <= whole, (width, err.max())
    # position 0 of every sequence: P = 1, dq is exactly zero in the model too
    cu = np.concatenate([[0], np.cumsum(BWD_LENS)])[:-1]
    assert not model[cu, :H * 64].any() and not exact[cu, :H * 64].any()


@pytest.mark.parametrize("n,d,D", [(1, 128, 64), (5, 128, 192), (33, 256, 128)])
def test_projection_and_final_layernorm_backward_reference_is_autograd(n, d, D):
    rng = np.random.default_rng(n + d)
    xe = rng.standard_normal((n, d)) * 2 + 0.3
    g, b = 1 + 0.1 * rng.standard_normal(d), 0.1 * rng.standard_normal(d)
    proj, dout = rng.standard_normal((d, D)) / np.sqrt(d), rng.standard_normal((n, D))
    eps = 1e-5
    tx, tg, tb, tp = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (xe, g, b, proj))
    pooled = F.layer_norm(tx, (d,), tg, tb, eps)
    (pooled @ tp).backward(torch.tensor(dout))
    r = pool_project_bwd_ref(dout, xe, g, b, eps, proj)
    assert _rel(r["pooled"], pooled.detach().numpy()) <= REL
    for key, t in (("dx", tx), ("dg", tg), ("db", tb), ("dproj", tp)):
        assert _rel(r[key], t.grad.numpy()) <= REL, key
    # the sums of absolute terms bound the sums themselves
    assert (np.abs(r["dproj"]) <= r["abs_dproj"] * (1 + 1e-12)).all() and (np.abs(r["dpooled"]) <= r["abs_dpooled"] * (1 + 1e-12)).all()
    assert (np.abs(r["db"]) <= r["abs_db"] * (1 + 1e-12)).all() and (np.abs(r["dg"]) <= r["abs_dg"] * (1 + 1e-12)).all()
    # the float32 evaluation is the same formula: it agrees to float32 accuracy and no better
    dx32, _ = ln_bwd_ref(r["dpooled"], xe, g, eps, np.float32)
    assert dx32.dtype == np.float32 and 0 < row_rel_l2(dx32, r["dx"]).max() < 1e-5


def test_layernorm_backward_reference_is_autograd():
    rng = np.random.default_rng(0)
    rows, d = 33, 128
    x, dy, g = rng.standard_normal((rows, d)) * 2 + 0.3, rng.standard_normal((rows, d)), 1 + 0.1 * rng.standard_normal(d)
    tx, tg = torch.tensor(x, requires_grad=True), torch.tensor(g, requires_grad=True)
    F.layer_norm(tx, (d,), tg, torch.zeros(d, dtype=torch.float64), 1e-5).backward(torch.tensor(dy))
    dx, xhat = ln_bwd_ref(dy, x, g, 1e-5)
    assert _rel(dx, tx.grad.numpy()) <= REL and _rel((dy * xhat).sum(0), tg.grad.numpy()) <= REL


def test_embedding_scatter_reference_is_add_at_over_the_kept_slots():
    rng = np.random.default_rng(1)
    ctx, vocab, d = 11, 9, 8
    lens = [1, 11, 4, 7, 11, 2]
    n = len(lens)
    tokens = rng.integers(-2, vocab + 3, size=(n, ctx)).astype(np.int32)       # out-of-range ids on both sides
    dx = rng.standard_normal((sum(lens), d))
    dtok, dpos, atok, apos, count = embed_bwd_ref(dx, tokens, lens, ctx, vocab)
    keep = np.arange(ctx)[None, :] < np.array(lens)[:, None]
    ids = np.clip(tokens, 0, vocab - 1)[keep]                                  # row-major over (sequence, position) = packed row order
    pos = np.broadcast_to(np.arange(ctx), (n, ctx))[keep]
    want_tok, want_pos = np.zeros((vocab, d)), np.zeros((ctx, d))
    np.add.at(want_tok, ids, dx)
    np.add.at(want_pos, pos, dx)
    assert _rel(dtok, want_tok) <= REL and _rel(dpos, want_pos) <= REL
    assert np.array_equal(count, np.bincount(ids, minlength=vocab))
    want_abs = np.zeros((vocab, d))
    np.add.at(want_abs, ids, np.abs(dx))
    assert _rel(atok, want_abs) <= REL and (np.abs(dpos) <= apos * (1 + 1e-12)).all()
    # dense rows: every slot counts
    dxd = rng.standard_normal((n * ctx, d))
    dtok_d, dpos_d, *_ = embed_bwd_ref(dxd, tokens, [ctx] * n, ctx, vocab)
    want_tok = np.zeros((vocab, d))
    np.add.at(want_tok, np.clip(tokens, 0, vocab - 1).reshape(-1), dxd)
    assert _rel(dtok_d, want_tok) <= REL and _rel(dpos_d, dxd.reshape(n, ctx, d).sum(0)) <= REL


@pytest.mark.parametrize("normalize", [False, True])
def test_fare_reference_is_autograd_of_the_mse_head(normalize):
    rng = np.random.default_rng(2)
    B, D, scale = 5, 48, 0.25
    f = rng.standard_normal((B, D)) * 1.7
    anchor = rng.standard_normal((B, D))
    tf = torch.tensor(f, requires_grad=True)
    feat = F.normalize(tf, dim=-1) if normalize else tf
    loss = F.mse_loss(torch.tensor(anchor), feat, reduction="none").sum(-1).mean()
    (loss * scale).backward()
    norms = np.linalg.norm(f, axis=-1) if normalize else None
    got_loss, dout, abs_loss, abs_dout = fare_ref(feat.detach().numpy(), anchor, scale, norms)
    want_loss = float(loss.detach())
    assert abs(got_loss - want_loss) <= REL * abs(want_loss) and abs_loss >= got_loss * (1 - 1e-12)
    assert _rel(dout, tf.grad.numpy()) <= REL
    assert (np.abs(dout) <= abs_dout * (1 + 1e-12)).all()
