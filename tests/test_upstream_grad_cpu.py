"""CPU-only half of the backward from any upstream gradient: the argument checks of leaf_text_backward / leaf_op_upstream_head
(reported before any HIP call, so they run on a box without a GPU) and the wiring of leaf_amd/autograd.py against a stub model --
a torch-CPU linear map with the three names the module uses (forward_train, backward_from, stash_ticket).  The kernels and the real
model are held to their checks in tests/test_gpu_upstream_grad.py."""
import ctypes as C

import pytest
import torch


def test_text_backward_and_upstream_head_refuse_bad_arguments_before_any_hip_call():
    from leaf_amd import _lib
    l = _lib.lib()
    h = C.c_void_p()
    cfg = _lib.TextCfgC(2, 128, 2, 64, 77, 49408, 0, 1e-5)
    assert l.leaf_text_create(C.byref(cfg), 1, C.byref(h)) == 0
    fake = C.c_void_p(64)                      # never dereferenced on these paths
    n, ws_bytes = 2, 1 << 20

    def backward(dfeat, grads, d_embed, handle=h, n_seq=n, seq_lens=None):
        a = _lib.BackwardArgs(params=fake, w16_bwd=fake, tokens=fake, seq_lens=seq_lens, n_seq=n_seq, feat=fake, head=_lib.HEAD_UPSTREAM,
                              ref=dfeat, scale=1.0, stash=fake, grads=grads, d_embed=d_embed, ws=fake, ws_bytes=ws_bytes)
        return l.leaf_text_backward(handle, a)
    assert backward(None, fake, None) != 0 and b"null/invalid" in l.leaf_last_error()          # no upstream gradient
    assert backward(None, fake, fake) != 0 and b"null/invalid" in l.leaf_last_error()
    assert backward(fake, None, None) != 0 and b"null/invalid" in l.leaf_last_error()          # nothing to compute
    assert backward(fake, fake, None, handle=None) != 0
    assert backward(fake, fake, None, n_seq=0) != 0
    # seq_lens (host) without cu_rows (device): refused as in every other entry point
    lens = (C.c_int32 * 2)(3, 4)
    assert backward(fake, fake, None, seq_lens=C.addressof(lens)) != 0
    assert b"go together" in l.leaf_last_error()

    def head(dfeat, feat, norms, B, D, dout=fake, ws=fake):
        return l.leaf_op_upstream_head(dfeat, feat, norms, None, B, D, 1.0, 0, dout, ws, None)
    assert head(fake, None, None, 0, 64) != 0 and b"upstream_head" in l.leaf_last_error()      # B < 1
    assert head(fake, None, None, -3, 64) != 0
    assert head(fake, None, None, 4, 2049) != 0 and b"2048" in l.leaf_last_error()             # D > 2048
    assert head(fake, None, None, 4, 0) != 0
    assert head(None, None, None, 4, 64) != 0 and head(fake, None, None, 4, 64, dout=None) != 0
    assert head(fake, None, None, 4, 64, ws=None) != 0
    assert head(fake, None, fake, 4, 64) != 0                                                  # norms without the normalised features
    l.leaf_text_destroy(h)


class _StubModel:
    """feat = (emb[text] + delta) @ W on the CPU, with the engine's protocol: one stash, a ticket per forward, parameter gradients
    ACCUMULATED into the flat ``grads``, the input gradient returned."""

    def __init__(self, V=11, d=6, D=4, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.emb = torch.randn(V, d, generator=g)
        self.W = torch.randn(d, D, generator=g)
        self.grads = torch.zeros(d * D)
        self.stash_ticket = 0
        self.calls = []

    def forward_train(self, text, seq_lens=None, delta=None, normalize=False, pool_last=False):
        self.stash_ticket += 1
        self.calls.append(("forward_train", seq_lens, normalize, pool_last))
        self._x = self.emb[text] + (delta if delta is not None else 0.0)
        return self._x @ self.W

    def backward_from(self, feat, dfeat, accum_scale=1.0, param_grads=True, want_input_grad=False, layer_events=None, ticket=None):
        if ticket is not None and ticket != self.stash_ticket:
            raise RuntimeError("stale stash ticket")
        self.calls.append(("backward_from", param_grads, want_input_grad, layer_events, ticket))
        assert torch.equal(feat, self._x @ self.W)
        g = accum_scale * dfeat
        if param_grads:
            self.grads += (self._x.T @ g).reshape(-1)
        return g @ self.W.T if want_input_grad else None


def _loss(feat, target):
    return ((feat - target) ** 2).sum(-1).mean() + feat.tanh().sum()


def _reference(m, text, delta, target):
    """the same map under plain autograd: (loss, d loss / d W flat, d loss / d delta)"""
    W = m.W.clone().requires_grad_(True)
    dl = delta.clone().requires_grad_(True)
    loss = _loss((m.emb[text] + dl) @ W, target)
    gW, gd = torch.autograd.grad(loss, (W, dl))
    return loss.detach(), gW.reshape(-1), gd


def test_autograd_seam_on_a_stub_model():
    from leaf_amd.autograd import encode_text_train, layer_events
    m = _StubModel()
    text = torch.tensor([3, 1, 7, 7, 0])
    g = torch.Generator().manual_seed(1)
    target = torch.randn(5, 4, generator=g)
    delta = (0.1 * torch.randn(5, 6, generator=g)).requires_grad_(True)
    loss_ref, gW_ref, gd_ref = _reference(m, text, delta.detach(), target)

    feat = encode_text_train(m, text, seq_lens=[1] * 5, delta=delta, normalize=False, pool_last=False)
    assert feat.grad_fn is not None and feat.requires_grad
    assert m.calls[-1] == ("forward_train", [1] * 5, False, False)
    loss = _loss(feat, target)
    assert torch.equal(loss.detach(), loss_ref)
    loss.backward(retain_graph=True)
    assert m.calls[-1] == ("backward_from", True, True, None, 1)                  # the ticket taken in the forward, no events
    torch.testing.assert_close(m.grads, gW_ref, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(delta.grad, gd_ref, rtol=1e-6, atol=1e-6)
    # a second backward through the same graph while the ticket is current accumulates again: exactly twice the first
    once, once_d = m.grads.clone(), delta.grad.clone()
    events = [object()]
    with layer_events(m, events):
        loss.backward()
    assert m.calls[-1][3] is events                                               # ... and the block events reach backward_from
    assert torch.equal(m.grads, 2 * once) and torch.equal(delta.grad, 2 * once_d)
    with pytest.raises(RuntimeError):                                             # the graph is gone now (plain autograd behaviour)
        loss.backward()

    # without a delta that requires grad: parameter gradients only, no input gradient asked for
    m.grads.zero_()
    feat = encode_text_train(m, text, delta=delta.detach())
    assert feat.grad_fn is not None
    _loss(feat, target).backward()
    assert m.calls[-1][:3] == ("backward_from", True, False)
    torch.testing.assert_close(m.grads, gW_ref, rtol=1e-6, atol=1e-6)
    feat = encode_text_train(m, text)                                             # no delta at all
    assert feat.grad_fn is not None
    feat.sum().backward()
    assert m.calls[-1][:3] == ("backward_from", True, False)

    # a second forward before the backward: the stash holds the second forward's activations, the first backward must raise
    m.grads.zero_()
    f1 = encode_text_train(m, text, delta=delta)
    f2 = encode_text_train(m, text.flip(0))
    before = m.grads.clone()
    with pytest.raises(RuntimeError, match="stale"):
        _loss(f1, target).backward()
    assert torch.equal(m.grads, before)
    f2.sum().backward()                                                           # the pending one still works

    # no_grad: what forward_train returns, no graph
    with torch.no_grad():
        f = encode_text_train(m, text, delta=delta)
    assert f.grad_fn is None and not f.requires_grad
    assert torch.equal(f, (m.emb[text] + delta.detach()) @ m.W)


def test_reducer_seam_on_a_stub_model():
    """GradReducer._loss_backward: loss_fn(anchor, feat) in the reference's argument order, loss * accum_scale back-propagated, the
    detached loss returned."""
    from leaf_amd.autograd import encode_text_train
    from leaf_amd.step import GradReducer
    m = _StubModel(seed=3)
    text = torch.tensor([2, 9, 4, 4])
    anchor = torch.randn(4, 4, generator=torch.Generator().manual_seed(5))
    _, gW_ref, _ = _reference(m, text, torch.zeros(4, 6), anchor)
    red = GradReducer.__new__(GradReducer)
    red.model = m
    seen = []

    def loss_fn(a, f):
        seen.append((a, f))
        return _loss(f, a)
    feat = encode_text_train(m, text)
    loss = red._loss_backward(loss_fn, feat, anchor, 0.5)
    assert seen[0][0] is anchor and seen[0][1] is feat
    assert loss.grad_fn is None and torch.equal(loss, _loss(feat.detach(), anchor))
    torch.testing.assert_close(m.grads, 0.5 * gW_ref, rtol=1e-6, atol=1e-6)
