"""The training-pass record of ``LeafCLIPText`` (``train_pass``) and the one marshaller behind its backward heads: a ``forward_train``
that raises leaves the committed pass, ``stash_ticket`` and the engine's ``normalize_fare`` option alone, a head called before any
forward names ``forward_train``, and the events entry of the TextFARE backward computes what the plain call computes.

tiny-test (width 128, 2 layers, embed 64), three captions of kept lengths 2, 5 and 77: the shortest legal row, a mid row and the
full context, so the packed row map is not the identity.  Every comparison is a bit identity: both sides run the same kernels on
the same arguments.  (``input_grad`` against ``backward_from`` on this length set is one more input of
tests/test_gpu_upstream_grad.py::test_backward_from_equals_the_textfare_backward_bit_for_bit.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SOT, EOT = 49406, 49407
LENS = np.array([2, 5, 77], np.int32)
OTHER_LENS = np.array([3, 4, 10], np.int32)


def _tokens(lens, seed):
    rng = np.random.default_rng(seed)
    toks = np.zeros((len(lens), 77), np.int32)
    for i, L in enumerate(lens):
        toks[i, 0], toks[i, 1:L - 1], toks[i, L - 1] = SOT, rng.integers(1, 49000, L - 2), EOT
    return toks


def _model():
    from leaf_amd.model import create_model
    return create_model("tiny-test", seed=5, trainable=True)


@pytest.fixture(scope="module")
def clean():
    """(tokens, anchor, feat, loss, grads) of forward_train + backward on a model that never saw a failed call; read-only"""
    import torch
    assert torch.cuda.is_available()
    m = _model()
    toks = _tokens(LENS, seed=1)
    anchor = torch.from_numpy(np.random.default_rng(2).standard_normal((len(LENS), m.cfg.embed_dim)).astype(np.float32)).to(m.device)
    feat = m.forward_train(toks, LENS)
    loss = m.backward(feat, anchor)
    assert bool(torch.isfinite(loss)) and bool(m.grads.any())
    return toks, anchor, feat.clone(), loss.clone(), m.grads.clone()


def _assert_backward_matches(torch, m, feat, clean):
    toks, anchor, feat_c, loss_c, grads_c = clean
    m.zero_grad()
    loss = m.backward(feat, anchor)
    assert torch.equal(feat, feat_c) and torch.equal(loss, loss_c) and torch.equal(m.grads, grads_c)


def test_failed_forward_leaves_the_pass_intact(clean):
    import torch
    m = _model()
    toks = clean[0]
    feat = m.forward_train(toks, LENS)
    ticket, kept = m.stash_ticket, m.train_pass
    delta = torch.zeros(int(OTHER_LENS.sum()), m.cfg.width, dtype=torch.float32, device=m.device)
    with pytest.raises(ValueError):
        m.forward_train(_tokens(OTHER_LENS, seed=3), seq_lens=OTHER_LENS, delta=delta, pool_last=True)
    with pytest.raises(ValueError):
        m.forward_train(toks, pool_last=True)
    assert m.stash_ticket == ticket and m.train_pass is kept
    _assert_backward_matches(torch, m, feat, clean)


def test_failed_normalized_forward_leaves_the_engine_option_alone(clean):
    import torch
    m = _model()
    toks = clean[0]
    feat = m.forward_train(toks, LENS)
    ticket = m.stash_ticket
    delta = torch.zeros(int(LENS.sum()), m.cfg.width, dtype=torch.float32, device=m.device)
    with pytest.raises(ValueError):
        m.forward_train(toks, seq_lens=LENS, delta=delta, normalize=True, pool_last=True)
    assert m._lib.leaf_text_get_option(m._h, b"normalize_fare") == 0 and m.stash_ticket == ticket
    _assert_backward_matches(torch, m, feat, clean)


class _NoCalls:
    """stands in for the C library: any entry a method reaches for is a launch the test forbids"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} reached before any forward_train")


def test_backward_heads_before_any_forward_name_forward_train():
    import torch
    m = _model()
    n, D, d = len(LENS), m.cfg.embed_dim, m.cfg.width
    feat = torch.zeros(n, D, dtype=torch.float32, device=m.device)
    rows = torch.zeros(int(LENS.sum()), d, dtype=torch.float32, device=m.device)
    torch.cuda.synchronize()
    lib, m._lib = m._lib, _NoCalls()
    try:
        for call in (lambda: m.backward(feat, feat), lambda: m.input_grad(feat, feat), lambda: m.cosine_input_grad(feat, feat),
                     lambda: m.backward_from(feat, feat), lambda: m.pgd_step(rows, rows, 0.1, 0.5)):
            with pytest.raises(RuntimeError, match="forward_train"):
                call()
    finally:
        m._lib = lib
    assert m.train_pass is None and m.stash_ticket == 0 and "stash" not in m._buf and not bool(m.grads.any())


def test_backward_with_block_events_equals_the_plain_backward(clean):
    import torch
    toks, anchor, feat_c, loss_c, grads_c = clean
    m = _model()
    feat = m.forward_train(toks, LENS)
    cur = torch.cuda.current_stream(m.device)
    events = [torch.cuda.Event() for _ in range(m.cfg.layers + 1)]
    for e in events:                   # an event's handle exists only once it has been recorded
        e.record(cur)
    loss = m.backward(feat, anchor, layer_events=events)
    assert torch.equal(loss, loss_c) and torch.equal(m.grads, grads_c)
    with pytest.raises(ValueError):
        m.backward(feat, anchor, layer_events=events[:-1])
    assert torch.equal(m.grads, grads_c), "a refused call touched the gradients"
