"""Backward from any upstream gradient on the GPU: upstream_rows_kernel (leaf_amd/csrc/train.hip), leaf_text_backward,
``LeafCLIPText.backward_from`` / ``encode_text_train`` (leaf_amd/autograd.py) and the ``loss_fn`` seam of the reducer and trainer.

Bit identities are DERIVED, not measured: the new head multiplies the caller's gradient by ``scale`` and everything behind it is the
code the TextFARE and cosine backwards run, so fed the ``dout`` those heads wrote (their kernel hooks) and scale = 1.0f (an exact
product) it must reproduce their results bit for bit -- T1 (head), T2 (TextFARE backward), T3 (cosine input gradient), T4 (the autograd
seam makes exactly that call).  The one tolerance (T5) is the one tests/test_gpu_train.py::test_loss_and_grads_vs_golden holds the
fused path to on the same configuration and anchor: per-tensor rel-L2 <= 6e-3 (1.2e-2 under LEAF_GRAD_DTYPE=bf16), loss 2e-3.

Measured on an MI355X: see the docstring of test_weighted_textfare_through_autograd_vs_fp32.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import text_oracle as O
from tests.util import ptr, rel_l2, stream

pytestmark = pytest.mark.gpu
SOT, EOT = 49406, 49407
TINY_LENS = [2, 5, 77, 9, 16, 17, 33, 3]            # ragged, a length-2 caption (SOT, EOT) and a full row
VITL_LENS = [3, 11, 17, 32, 40]
PASS_LENS = [2, 5, 77]                               # the length set of tests/test_gpu_train_pass.py: shortest legal row, mid row, full context


@pytest.fixture(scope="module")
def env():
    import torch
    from leaf_amd import _lib
    assert torch.cuda.is_available()
    return _lib.lib(), torch, torch.device("cuda:0")


def _tokens(lens, seed):
    rng = np.random.default_rng(seed)
    toks = np.zeros((len(lens), 77), np.int32)
    for i, L in enumerate(lens):
        toks[i, 0], toks[i, 1:L - 1], toks[i, L - 1] = SOT, rng.integers(1, 49000, L - 2), EOT
    return toks


def _fare(env, feat, anchor, scale, norms=None, scaler=None, use_scaling=0):
    """leaf_op_fare_loss -> (dout [B, D], gscale {S, 1/S}, loss [1])"""
    lib, torch, dev = env
    from leaf_amd import _lib
    B, D = feat.shape
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    dout = torch.full((B, D), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.full((64 + 2 * B,), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(lib.leaf_op_fare_loss(ptr(feat), ptr(anchor), ptr(norms), ptr(scaler), B, D, float(scale), use_scaling, ptr(loss),
                                     ptr(dout), ptr(ws), stream()), "fare_loss")
    return dout, ws[:2].clone(), loss


def _upstream(env, dfeat, feat, norms, scale, scaler=None, use_scaling=0):
    """leaf_op_upstream_head -> (dout [B, D], gscale {S, 1/S}, row partials [B, 2])"""
    lib, torch, dev = env
    from leaf_amd import _lib
    B, D = dfeat.shape
    dout = torch.full((B, D), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.full((64 + 2 * B,), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(lib.leaf_op_upstream_head(ptr(dfeat), ptr(feat), ptr(norms), ptr(scaler), B, D, float(scale), use_scaling, ptr(dout),
                                         ptr(ws), stream()), "upstream_head")
    return dout, ws[:2].clone(), ws[64:].view(B, 2).clone()


# =============================================================================================== T1: the head against the fused head
@pytest.mark.parametrize("B", [1, 5, 300])
@pytest.mark.parametrize("D", [64, 768, 1280, 2048])
def test_upstream_head_equals_the_fused_head_bit_for_bit(env, D, B):
    lib, torch, dev = env
    rng = np.random.default_rng(7 * D + B)
    scale = 0.5
    raw = (rng.standard_normal((B, D)) * 1.7).astype(np.float32)
    norms = np.linalg.norm(raw.astype(np.float64), axis=-1).astype(np.float32)
    anchor = torch.from_numpy((rng.standard_normal((B, D)) / np.sqrt(D)).astype(np.float32)).to(dev)
    t_raw, t_norms = torch.from_numpy(raw).to(dev), torch.from_numpy(norms).to(dev)
    t_unit = torch.from_numpy((raw / norms[:, None]).astype(np.float32)).to(dev)
    for use_scaling, backoff in ((0, None), (1, None), (1, 0), (1, -2)):
        state = None
        if backoff is not None:
            host = np.zeros(16, np.float32)
            host[3] = backoff                            # LEAF_SC_BACKOFF
            state = torch.from_numpy(host).to(dev)
        label = f"D={D} B={B} scaling={use_scaling} backoff={backoff}"
        # no normalisation: fed the fused head's dout and scale = 1.0f, the head reproduces it
        want, gs_want, _ = _fare(env, t_raw, anchor, scale, None, state, use_scaling)
        got, gs_got, part = _upstream(env, want, None, None, 1.0, state, use_scaling)
        assert torch.equal(got, want) and torch.equal(gs_got, gs_want), label
        assert not part[:, 0].any(), label + ": the row loss of the upstream head is 0"
        assert torch.equal(part[:, 1], want.abs().amax(-1)), label
        # with norms: fed g = the gradient with respect to the NORMALISED features (the fused head without norms on them), it applies
        # the VJP of F.normalize with the fused head's reduction tree
        g, _, _ = _fare(env, t_unit, anchor, scale, None, state, use_scaling)
        want, gs_want, _ = _fare(env, t_unit, anchor, scale, t_norms, state, use_scaling)
        got, gs_got, _ = _upstream(env, g, t_unit, t_norms, 1.0, state, use_scaling)
        assert torch.equal(got, want) and torch.equal(gs_got, gs_want), label + " norms"
        if state is not None:
            assert np.array_equal(state.cpu().numpy(), host), "the head wrote to the scaler state"
    # a scale that is not 1: plain fp32 products
    got, gs, _ = _upstream(env, t_raw, None, None, 0.3, None, 0)
    assert torch.equal(got, t_raw * np.float32(0.3)) and gs.tolist() == [1.0, 1.0]


def test_upstream_head_refuses_more_than_2048_columns(env):
    lib, torch, dev = env
    z = torch.zeros(2, 2049, dtype=torch.float32, device=dev)
    ws = torch.zeros(64 + 4, dtype=torch.float32, device=dev)
    assert lib.leaf_op_upstream_head(ptr(z), None, None, None, 2, 2049, 1.0, 0, ptr(z.clone()), ptr(ws), stream()) != 0
    torch.cuda.synchronize()


# =============================================================================================== T2: the whole backward
@pytest.fixture(scope="module")
def models(env):
    from leaf_amd.model import create_model
    made = {}

    def get(name):
        if name not in made:
            made[name] = create_model(name, seed=5, trainable=True)
        return made[name]
    return get


def _anchor(env, m, toks, normalize, seed):
    """an anchor about ||f|| away from the features (as the golden fixtures: no cancellation in f - anchor)"""
    lib, torch, dev = env
    f = m.encode_text(toks)
    gen = torch.Generator(device=dev).manual_seed(seed)
    a = f + f.norm(dim=-1, keepdim=True) * torch.randn(f.shape, device=dev, generator=gen) / f.shape[1] ** 0.5
    return torch.nn.functional.normalize(a, dim=-1) if normalize else a


@pytest.mark.parametrize("accum", [1.0, 0.5])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("name,lens", [("tiny-test", TINY_LENS), ("tiny-test-quickgelu", TINY_LENS), ("ViT-L-14", VITL_LENS),
                                       ("tiny-test", PASS_LENS)])
def test_backward_from_equals_the_textfare_backward_bit_for_bit(env, models, name, lens, packed, normalize, accum):
    lib, torch, dev = env
    m = models(name)
    toks = _tokens(lens, seed=len(lens))
    anchor = _anchor(env, m, toks, normalize, seed=3)
    m.trim_rows = packed
    try:
        feat = m.forward_train(toks, normalize=normalize)
        rows = sum(lens) if packed else len(lens) * 77
        m.zero_grad()
        loss = m.backward(feat, anchor, accum_scale=accum)
        want = m.grads.clone()
        assert bool(torch.isfinite(loss)) and bool(want.any())
        # the gradient with respect to the features the forward RETURNED (normalised ones under normalize): the fused head without norms
        dout, _, _ = _fare(env, feat, anchor, accum)
        m.zero_grad()
        assert m.backward_from(feat, dout) is None
        assert torch.equal(m.grads, want), "parameter gradients"
        # input gradient only, against input_grad (which back-propagates the loss itself: scale 1)
        _, g_want = m.input_grad(feat, anchor)
        dout1, _, _ = _fare(env, feat, anchor, 1.0)
        g = m.backward_from(feat, dout1, param_grads=False, want_input_grad=True)
        assert tuple(g.shape) == (rows, m.cfg.width) and torch.equal(g, g_want), "input gradient"
        assert torch.equal(m.grads, want), "an input-gradient-only backward touched the parameter gradients"
        # the same through accum_scale instead of a pre-scaled gradient (powers of two: exact either way)
        m.zero_grad()
        m.backward_from(feat, dout1, accum_scale=accum)
        assert torch.equal(m.grads, want), "accum_scale"
        # both outputs in one pass == the two separate calls
        g_sep = m.backward_from(feat, dout, param_grads=False, want_input_grad=True)
        m.zero_grad()
        g_both = m.backward_from(feat, dout, want_input_grad=True)
        assert torch.equal(m.grads, want) and torch.equal(g_both, g_sep), "both outputs in one call"
        with pytest.raises(ValueError):
            m.backward_from(feat, dout, param_grads=False, want_input_grad=False)
        with pytest.raises(ValueError):
            m.backward_from(feat, dout[:-1])
    finally:
        m.trim_rows = True
        m.zero_grad()


# =============================================================================================== T3: against the cosine input gradient
def test_backward_from_equals_the_cosine_input_grad_bit_for_bit(env, models):
    lib, torch, dev = env
    from leaf_amd import _lib
    m = models("tiny-test")
    rng = np.random.default_rng(21)
    ids = [rng.integers(1, 49000, P) for P in (1, 4, 9, 15)]
    toks = np.zeros((4, 77), np.int32)
    for i, p in enumerate(ids):
        toks[i, 0], toks[i, 1:1 + len(p)], toks[i, 1 + len(p)] = SOT, p, EOT
    lens = np.array([len(p) + 2 for p in ids], np.int32)
    B, D, weight = 4, m.cfg.embed_dim, 1.7
    target = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(dev)
    feat = m.forward_train(toks, seq_lens=lens, pool_last=True)
    cos, g_want = m.cosine_input_grad(feat, target, weight)
    dout = torch.full((B, D), float("nan"), dtype=torch.float32, device=dev)
    cosv = torch.empty(B, dtype=torch.float32, device=dev)
    ws = torch.zeros(64 + 2 * B, dtype=torch.float32, device=dev)
    _lib.check(lib.leaf_op_cosine_head(ptr(feat), ptr(target), B, D, weight, ptr(dout), ptr(cosv), ptr(ws), stream()), "cosine_head")
    before = m.grads.clone()
    g = m.backward_from(feat, dout, param_grads=False, want_input_grad=True)
    assert torch.equal(cosv, cos) and bool(g_want.any())
    assert tuple(g.shape) == (int(lens.sum()), m.cfg.width) and torch.equal(g, g_want)
    assert torch.equal(m.grads, before)


# =============================================================================================== T4: the autograd seam
def _info_nce(torch, feat, matrix, scale=10.0):
    F = torch.nn.functional
    logits = scale * F.normalize(feat, dim=-1) @ F.normalize(matrix, dim=-1).T
    labels = torch.arange(feat.shape[0], device=feat.device)
    return 0.5 * (F.cross_entropy(logits, labels) + F.cross_entropy(logits.T, labels))


def test_autograd_seam_makes_exactly_the_backward_from_call(env, models):
    """A loss the engine has no head for (symmetric InfoNCE against a fixed matrix): loss.backward() through encode_text_train leaves
    in model.grads / delta.grad the bits that backward_from accumulates from torch.autograd.grad(loss, feat) on a detached copy."""
    lib, torch, dev = env
    m = models("tiny-test")
    toks = _tokens(TINY_LENS, seed=8)
    B, D = len(TINY_LENS), m.cfg.embed_dim
    matrix = torch.randn(B, D, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    delta = (1e-3 * torch.randn(sum(TINY_LENS), m.cfg.width, device=dev, generator=torch.Generator(device=dev).manual_seed(5)))
    delta.requires_grad_(True)
    m.zero_grad()
    feat = m.encode_text_train(toks, delta=delta)
    assert feat.grad_fn is not None and tuple(feat.shape) == (B, D)
    assert torch.equal(feat.detach(), m.forward_train(toks, delta=delta.detach()))          # same forward (and a fresh ticket ...)
    feat = m.encode_text_train(toks, delta=delta)                                           # ... so take the forward again
    loss = _info_nce(torch, feat, matrix)
    loss.backward(retain_graph=True)
    got, got_delta = m.grads.clone(), delta.grad.clone()
    assert bool(got.any()) and bool(got_delta.any())
    # the same call by hand, on the same stash
    f2 = feat.detach().clone().requires_grad_(True)
    dfeat, = torch.autograd.grad(_info_nce(torch, f2, matrix), f2)
    m.zero_grad()
    d_embed = m.backward_from(feat.detach(), dfeat, want_input_grad=True, ticket=m.stash_ticket)
    assert torch.equal(m.grads, got) and torch.equal(d_embed, got_delta)
    # retain_graph: a second backward while the ticket is current accumulates again.  delta.grad is autograd's sum of two equal
    # tensors (exact); the parameter buffer is added to by the kernels in their own order, held to the 1e-6 that
    # test_loss_and_grads_vs_golden holds a doubled backward to
    m.grads.copy_(got)
    loss.backward()
    assert torch.equal(delta.grad, 2 * got_delta)
    assert rel_l2(m.grads.cpu().numpy(), 2 * got.cpu().numpy()) < 1e-6
    # a stale ticket: another forward_train has overwritten the stash
    f1 = m.encode_text_train(toks)
    m.forward_train(toks)
    before = m.grads.clone()
    with pytest.raises(RuntimeError, match="stale"):
        f1.sum().backward()
    assert torch.equal(m.grads, before)
    with pytest.raises(RuntimeError, match="stale"):
        m.backward_from(feat.detach(), dfeat, ticket=m.stash_ticket - 1)
    with torch.no_grad():
        f = m.encode_text_train(toks)
    assert f.grad_fn is None and not f.requires_grad
    m.zero_grad()


# =============================================================================================== T5: a new loss against fp32
def test_weighted_textfare_through_autograd_vs_fp32(env, golden_dir):
    """mean_b w_b ||a_b - f_b||^2, w_b in [0.5, 1.5]: no kernel was written for it.  Reference: the same expression on the fp32 torch
    tower of oracle/torch_cpu_harness.py under CPU autograd (it reproduces the reference-generated gradients of this fixture).
    Bounds: those of test_loss_and_grads_vs_golden on this configuration and anchor.
    Measured on an MI355X (fp16 gradient path): worst tensor transformer.resblocks.1.ln_1.bias, rel-L2 3.5e-3 (bound 6e-3); loss
    relative error 1.3e-4 (bound 2e-3)."""
    lib, torch, dev = env
    from leaf_amd.model import create_model
    from oracle.torch_cpu_harness import TorchTextTower
    z = np.load(os.path.join(golden_dir, "tiny_gelu.npz"))
    toks, anchor = z["tokens"][:8], z["anchor"]
    w_np = np.random.default_rng(17).uniform(0.5, 1.5, 8).astype(np.float32)
    cfg = O.TextCfg(128, 2, 2, 64, quick_gelu=False)
    ref = TorchTextTower(O.init_weights(cfg, 11), cfg, requires_grad=True)
    a_cpu, w_cpu = torch.from_numpy(anchor), torch.from_numpy(w_np)
    loss_ref = (w_cpu * ((a_cpu - ref.encode_text(torch.from_numpy(toks.astype(np.int64)))) ** 2).sum(-1)).mean()
    loss_ref.backward()

    m = create_model("tiny-test", seed=11, trainable=True)
    m.zero_grad()
    feat = m.encode_text_train(toks)
    loss = (w_cpu.to(dev) * ((a_cpu.to(dev) - feat) ** 2).sum(-1)).mean()
    loss.backward()
    torch.cuda.synchronize()
    loss_err = abs(float(loss.detach()) - float(loss_ref.detach())) / abs(float(loss_ref.detach()))
    worst = {}
    batch_ids = np.unique(toks)
    for k, (off, shape) in m.layout.items():
        g = m.grads[off: off + int(np.prod(shape))].view(shape).cpu().numpy()
        want = ref.p[k].grad.numpy()
        if k == "token_embedding.weight":
            assert np.abs(np.delete(g, batch_ids, axis=0)).sum() == 0.0, "token-embedding rows outside the batch must be exactly zero"
            worst[k] = rel_l2(g[batch_ids], want[batch_ids])
        else:
            worst[k] = rel_l2(g, want)
    top = max(worst, key=worst.get)
    print(f"weighted TextFARE through autograd: worst tensor {top} rel-L2 {worst[top]:.3e}, loss rel err {loss_err:.3e}")
    tol = 1.2e-2 if os.environ.get("LEAF_GRAD_DTYPE", "").lower().startswith("b") else 6e-3
    assert loss_err < 2e-3
    bad = {k: v for k, v in worst.items() if v > tol}
    assert not bad, bad


# =============================================================================================== T6: non-finite upstream gradient
def test_non_finite_upstream_gradient_skips_the_step(env):
    lib, torch, dev = env
    from leaf_amd.model import create_model
    m = create_model("tiny-test-quickgelu", seed=12, trainable=True)
    toks = O.synthetic_tokens(6, seed=4)
    feat = m.forward_train(toks)
    dfeat = torch.randn(feat.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) * 0.1
    dfeat[2, 5] = float("nan")
    m.zero_grad()
    m.backward_from(feat, dfeat)
    p0, m0, v0 = m.flat.clone(), m.exp_avg.clone(), m.exp_avg_sq.clone()
    skipped = m.skipped_steps()
    norm = m.adamw_step(lr=1e-3, weight_decay=0.1)
    assert not bool(torch.isfinite(norm))
    assert m.skipped_steps() == skipped + 1
    assert torch.equal(m.flat, p0) and torch.equal(m.exp_avg, m0) and torch.equal(m.exp_avg_sq, v0)
    # the next finite step runs
    dfeat[2, 5] = 0.0
    m.zero_grad()
    m.backward_from(feat, dfeat)
    norm = m.adamw_step(lr=1e-3, weight_decay=0.1)
    assert bool(torch.isfinite(norm)) and m.skipped_steps() == skipped + 1 and not torch.equal(m.flat, p0)


# =============================================================================================== T7: reducer and trainer
def _mse(a, f):
    import torch.nn.functional as F
    return F.mse_loss(a, f, reduction="none").sum(-1).mean()


def test_reducer_loss_fn_with_block_events_forced_on(env, models, monkeypatch):
    """(a) One rank: the overlapped form (per-block events handed to the backward through the autograd seam, buckets reduced on the
    side stream -- a one-rank sum is the identity, so the collective is replaced by nothing) gives the gradients of the plain form
    bit for bit, and the backward records every event."""
    lib, torch, dev = env
    import torch.distributed as dist
    from leaf_amd import step
    m = models("tiny-test")
    red = step.GradReducer(m)
    toks = _tokens(TINY_LENS, seed=12)
    anchor = _anchor(env, m, toks, False, seed=6)
    m.zero_grad()
    loss_plain = red.backward(m.encode_text_train(toks), anchor, accum_scale=0.5, loss_fn=_mse)      # no process group: plain form
    want = m.grads.clone()
    assert red.events is None and bool(want.any())

    reduced = []
    monkeypatch.setattr(step, "_dp_active", lambda: True)
    monkeypatch.setattr(dist, "all_reduce", lambda t, op=None, group=None: reduced.append(int(t.numel())))
    red._setup()
    red.events = [torch.cuda.Event(enable_timing=True) for _ in range(m.cfg.layers + 1)]
    cur = torch.cuda.current_stream(dev)
    for e in red.events:
        e.record(cur)
    feat = m.encode_text_train(toks)                      # kernels between the events' first recording and t0
    m.zero_grad()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(cur)
    loss_events = red.backward(feat, anchor, accum_scale=0.5, last_micro=True, loss_fn=_mse)
    t1.record(cur)
    assert red._launched and sum(reduced) == m.n_params       # every bucket was handed to the collective, the ranges partition the buffer
    cur.wait_stream(red.comm)
    red._launched = False
    torch.cuda.synchronize()
    assert torch.equal(m.grads, want) and torch.equal(loss_events, loss_plain)
    assert loss_events.grad_fn is None
    # every event was recorded by THIS backward, in the order the blocks finish: t0 <= [L-1] <= ... <= [0] <= [L] <= t1
    order = [t0] + [red.events[l] for l in reversed(range(m.cfg.layers))] + [red.events[m.cfg.layers], t1]
    for a, b in zip(order[:-1], order[1:]):
        assert a.elapsed_time(b) >= 0.0
    m.zero_grad()


def _run_epoch(env, tmp_path, loss, batch, extra, dtype):
    """One epoch of train_one_epoch_text_only on tiny-test from seeded random weights, as the entry script sets it up; returns
    (flat, exp_avg, exp_avg_sq, the logged loss of every optimizer step)."""
    lib, torch, dev = env
    import random
    import string
    from leaf_amd.model import LeafCLIPText, create_model
    from leaf_amd.params import parse_args
    from leaf_amd.tokenizer import get_tokenizer
    from leaf_amd.train import LeafAdamW, get_text_data, make_scheduler, train_one_epoch_text_only
    caps = tmp_path / "caps.txt"
    words = "a photo of the small red car on wet street with two people near old house in sunny park at night dog cat".split()
    rng = random.Random(3)
    caps.write_text("\n".join(" ".join(rng.choice(words) for _ in range(rng.randint(3, 12))) for _ in range(32)) + "\n")
    args = parse_args(["--model", "tiny-test", "--dataset-type", "text", "--train-data", str(caps), "--batch-size", str(batch), "--lr", "1e-4",
                       "--wd", "1e-4", "--warmup", "2", "--rho", "6", "--k_adv", "1", "--seed", "2", "--epochs", "1", "--random-init",
                       "--workers", "0", "--log-every-n-steps", "1"] + extra)
    args.distributed, args.world_size, args.rank, args.local_rank, args.device = False, 1, 0, 0, "cuda:0"
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    random.seed(args.seed)
    V = [-1] + [ord(c) for c in string.ascii_lowercase + ' ' + string.ascii_uppercase + string.digits + string.punctuation]
    model = create_model("tiny-test", dtype=dtype, trainable=True, seed=args.seed)
    optimizer = LeafAdamW(model, lr=args.lr, betas=(args.beta1, args.beta2), eps=args.eps, weight_decay=args.wd)
    tokenizer = get_tokenizer(args.model)
    data = get_text_data(args, epoch=0)
    n_batches = data["train"].dataloader.num_batches
    scheduler = make_scheduler(args, optimizer, (n_batches // args.accum_freq) * args.epochs, n_batches)
    frozen = LeafCLIPText(model.cfg, dtype=dtype).copy_from(model)
    frozen.pack()
    model.pack()

    class Writer:
        losses = []

        def add_scalar(self, name, val, step):
            if name == "train/loss":
                self.losses.append(float(val))
    writer = Writer()
    writer.losses = []
    train_one_epoch_text_only(model, frozen, tokenizer, V, data, loss, 0, optimizer, None, scheduler, args, tb_writer=writer)
    torch.cuda.synchronize()
    return model.flat.clone(), model.exp_avg.clone(), model.exp_avg_sq.clone(), writer.losses, model.applied_steps()


def test_torch_mse_gradient_is_the_fused_heads_dout(env):
    """(b), first: at B = 8 every factor of torch's MSE gradient (2, 1 / B, accum_scale) is a power of two, so the callable's d loss /
    d feat is the fused head's dout bit for bit -- what makes the two trainer runs below comparable bit for bit."""
    lib, torch, dev = env
    for B, accum in ((8, 1.0), (4, 0.5)):
        gen = torch.Generator(device=dev).manual_seed(B)
        f = torch.randn(B, 64, device=dev, generator=gen).requires_grad_(True)
        a = torch.randn(B, 64, device=dev, generator=gen)
        loss = _mse(a, f)
        dfeat, = torch.autograd.grad(loss * accum, f)
        dout, _, loss_fused = _fare(env, f.detach(), a, accum)
        assert torch.equal(dfeat, dout), (B, accum)
        assert abs(float(loss.detach()) - float(loss_fused[0])) <= B * 64 * 2.0 ** -24 * abs(float(loss_fused[0]))


@pytest.mark.parametrize("batch,extra,grad_dtype", [
    (8, [], None),
    (4, ["--accum-freq", "2"], None),
    (8, ["--grad-clip-norm", "1.0"], None),
    (4, ["--accum-freq", "2", "--grad-clip-norm", "1.0", "--precision", "amp_bf16"], "bf16"),      # MicroClip: refuses --precision amp
], ids=["plain", "accum2", "clip", "microclip-bf16"])
def test_trainer_with_an_mse_callable_equals_the_fused_textfare_run(env, tmp_path, monkeypatch, batch, extra, grad_dtype):
    """(b) 4 optimizer steps from the same state, once with loss=None (the fused head) and once with the TextFARE expression as a
    PyTorch callable in the reference's argument order: weights and both AdamW moments bit-identical (see the test above), every
    logged loss within B D 2^-24 relative (fp32 summation order only)."""
    lib, torch, dev = env
    monkeypatch.chdir(tmp_path)
    if grad_dtype:
        monkeypatch.setenv("LEAF_GRAD_DTYPE", grad_dtype)
    dtype = "bf16" if "amp_bf16" in extra else "fp16"
    fused = _run_epoch(env, tmp_path, None, batch, extra, dtype)
    custom = _run_epoch(env, tmp_path, lambda a, f: _mse(a, f), batch, extra, dtype)
    assert fused[4] == custom[4] == 4 and len(fused[3]) == len(custom[3]) == 4
    for name, x, y in zip(("flat", "exp_avg", "exp_avg_sq"), fused[:3], custom[:3]):
        assert torch.equal(x, y), name
    assert bool(fused[1].any())
    bound = batch * 64 * 2.0 ** -24
    for lf, lc in zip(fused[3], custom[3]):
        assert np.isfinite(lf) and abs(lf - lc) <= bound * abs(lf), (fused[3], custom[3])
