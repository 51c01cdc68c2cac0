"""The autograd seam of the text tower: ``forward_train`` as a ``torch.autograd.Function``, so that ANY PyTorch loss of the features
can be back-propagated through the engine (the reference's ``model.encode_text`` returns a tensor with a ``grad_fn``,
utils_AT.py:317-337).

    feat = encode_text_train(model, tokens)          # or model.encode_text_train(tokens)
    loss = my_loss(anchor, feat)                     # plain PyTorch
    loss.backward()                                  # -> model.backward_from(feat, d loss / d feat, ticket=...)

Where the gradients go: PARAMETER gradients are ACCUMULATED into ``model.grads``, the flat buffer that ``adamw_step`` / ``LeafAdamW``
consume -- not into ``.grad`` attributes (``model.zero_grad()`` clears them); the gradient of ``delta`` is returned to autograd when
``delta.requires_grad``.  A second backward through the same graph (``retain_graph=True``) accumulates again.

One differentiable forward may be pending per model: the engine keeps ONE activation stash, every ``forward_train`` overwrites it and
bumps ``model.stash_ticket``; the backward hands the ticket taken in its forward to ``backward_from``, which raises ``RuntimeError``
when it is stale.  No higher-order gradients, no gradient with respect to hidden states.

The module is duck-typed on the model: it calls ``forward_train``, ``backward_from`` and reads ``stash_ticket``, nothing else.
"""
from __future__ import annotations

import contextlib

import torch

# block events of the backward that is about to run, by id(model): set around ``loss.backward()`` by ``layer_events`` below (the
# backward runs on autograd's own thread, so this is a plain table, not a thread-local)
_EVENTS = {}


@contextlib.contextmanager
def layer_events(model, events):
    """Inside this block a backward through ``encode_text_train(model, ...)`` passes ``events`` (None: none) to ``backward_from`` as
    its ``layer_events`` -- the per-block completion events of the overlapped gradient reduction (leaf_amd/step.py)."""
    if events is None:
        yield
        return
    _EVENTS[id(model)] = events
    try:
        yield
    finally:
        _EVENTS.pop(id(model), None)


class _EncodeTextTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, graph, delta, model, text, seq_lens, normalize, pool_last):
        # ``graph``: a 0-d tensor that requires grad and receives none -- it gives the output a grad_fn when no ``delta`` does
        feat = model.forward_train(text, seq_lens=seq_lens, delta=delta, normalize=normalize, pool_last=pool_last)
        ctx.model, ctx.ticket = model, model.stash_ticket
        ctx.delta_shape = tuple(delta.shape) if delta is not None and ctx.needs_input_grad[1] else None
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(feat)
        return feat

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dfeat):
        if dfeat is None:
            return (None,) * 7
        model = ctx.model
        feat, = ctx.saved_tensors
        d_embed = model.backward_from(feat, dfeat, param_grads=True, want_input_grad=ctx.delta_shape is not None,
                                      layer_events=_EVENTS.get(id(model)), ticket=ctx.ticket)
        return (None, d_embed.view(ctx.delta_shape) if ctx.delta_shape is not None else None) + (None,) * 5


def encode_text_train(model, text, seq_lens=None, delta=None, normalize: bool = False, pool_last: bool = False) -> torch.Tensor:
    """``model.forward_train(text, seq_lens, delta, normalize, pool_last)`` with a ``grad_fn`` (module docstring).  Under
    ``torch.no_grad()`` it returns what ``forward_train`` returns."""
    if not torch.is_grad_enabled():
        return model.forward_train(text, seq_lens=seq_lens, delta=delta, normalize=normalize, pool_last=pool_last)
    graph = torch.zeros((), requires_grad=True)
    return _EncodeTextTrain.apply(graph, delta, model, text, seq_lens, normalize, pool_last)
