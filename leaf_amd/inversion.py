"""Text embedding inversion (PEZ) on the HIP engine: reconstruct a caption from its embedding alone.

A batched restatement of the reference's ``optimize_prompt_loop`` for text targets (src/pez/optim_utils.py:139-232, driven by
src/pez/run_coco.py:10-42).  The reference optimises ONE prompt at a time for 3,000 iterations; here many captions are inverted at
once, each with its own prompt, target and running best, and every inversion computes exactly what its own one-caption loop
computes: the projection, the forward, the cosine head and the optimizer are all row- or sequence-wise.

Per iteration, everything on the device:
  1. project every prompt row to its cosine-nearest token embedding           (nn_project :26-55  -> leaf_nn_project)
  2. forward of [SOT, ids, EOT], pooled at the template's EOT slot             (forward_text_embedding, open_clip_pez/model.py:210-246)
  3. loss_b = loss_weight (1 - cos(feat_b, target_b)) and its gradient with respect to the projected embeddings (:191-196)
  4. that gradient is handed to the CONTINUOUS prompt rows (:196) and
  5. AdamW steps them (:152,201; torch.optim.AdamW defaults, weight decay on every element)
  6. the best (cos, ids) so far is kept per inversion; a strictly greater cosine replaces it (:214)

Out of scope (an error): ``prompt_bs > 1``, image targets, ``avg_text`` pooling.  BLEU (compute_metrics.py:64) is left out.
"""
from __future__ import annotations

import logging
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .model import _ptr

SOT, EOT = 49406, 49407


# ------------------------------------------------------------------ metrics (src/pez/compute_metrics.py:8-27)
def token_accuracy(reconstructions_ids: Sequence[Sequence[int]], references_ids: Sequence[Sequence[int]]) -> float:
    """Share of the reference's tokens found anywhere in the reconstruction.  The reference's convention: zeros (padding) are
    dropped from both, and SOT / EOT -- the first and last id left -- from the reference ids (``ids_orig`` is a full token row,
    ``ids_rec`` the prompt alone); the two must then be equally long."""
    n_correct = n_total = 0
    for rec, ref in zip(reconstructions_ids, references_ids):
        rec = [int(r) for r in rec if r != 0]
        ref = [int(r) for r in ref if r != 0][1:-1]
        if len(rec) != len(ref):
            raise ValueError(f"token_accuracy: reconstruction of {len(rec)} ids against a reference of {len(ref)}")
        n_correct += sum(t in rec for t in ref)
        n_total += len(rec)
    return n_correct / n_total


def word_accuracy(reconstructions: Sequence[str], references: Sequence[str]) -> float:
    """Share of the reference's lower-cased whitespace words found in the reconstruction, over the reconstruction's word count."""
    n_correct = n_total = 0
    for rec, ref in zip(reconstructions, references):
        rec, ref = rec.lower().split(), ref.lower().split()
        n_correct += sum(t in rec for t in ref)
        n_total += len(rec)
    return n_correct / n_total


def initial_ids(prompt_len: int, seed: int, vocab_size: int = 49408) -> np.ndarray:
    """The reference's random start of one inversion: it seeds torch with ``seed`` before every caption (run_coco.py:25-28) and
    draws ``torch.randint(len(tokenizer.encoder), (1, prompt_len))`` on the CPU (optim_utils.py:113) -- from the WHOLE vocabulary,
    SOT and EOT included."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(vocab_size, (1, int(prompt_len)), generator=g).numpy().reshape(-1).astype(np.int32)


def _invert_batch(model, targets: torch.Tensor, plens: List[int], starts: List[np.ndarray], iters: int, lr: float, weight_decay: float,
                  loss_weight: float, print_step: Optional[int]):
    """(best ids per inversion [list of int32 arrays], best cosine of the loop [B]) for one batch of inversions"""
    dev, d, ctx = model.device, model.cfg.width, model.cfg.context_length
    B = len(plens)
    lens = np.asarray(plens, np.int32) + 2
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seg = np.repeat(np.arange(B), plens)                                  # inversion of every prompt row
    pos = np.concatenate([np.arange(p) for p in plens]) + 1               # its position in the sequence
    slot = torch.from_numpy(seg * ctx + pos).to(dev)                      # ... in the flat token matrix
    grow = torch.from_numpy(cu[seg] + pos).to(dev)                        # ... among the packed rows of the forward
    seg_t = torch.from_numpy(seg).to(dev)
    tokens = np.zeros((B, ctx), np.int32)
    tokens[:, 0] = SOT
    tokens[np.arange(B), lens - 1] = EOT
    tokens = torch.from_numpy(tokens).to(dev)
    table = model.params["token_embedding.weight"]
    start = torch.from_numpy(np.concatenate(starts).astype(np.int64)).to(dev)
    prompt = table.index_select(0, start).contiguous()                    # [sum P, d], the optimised embeddings (:116)
    m1, m2 = torch.zeros_like(prompt), torch.zeros_like(prompt)
    n = prompt.numel()
    best_cos = torch.full((B,), -1000.0 * loss_weight, dtype=torch.float32, device=dev)      # :154
    best_ids = torch.zeros(len(seg), dtype=torch.int32, device=dev)
    lib = _lib.lib()
    for it in range(iters):
        ids, _ = model.nn_project(prompt)
        tokens.view(-1).index_copy_(0, slot, ids)
        feat = model.forward_train(tokens, seq_lens=lens, pool_last=True)
        cos, g = model.cosine_input_grad(feat, targets, loss_weight)
        grad = g.index_select(0, grow)
        _lib.check(lib.leaf_adamw_step(_ptr(prompt), _ptr(grad), _ptr(m1), _ptr(m2), n, n, float(lr), 0.9, 0.999, 1e-8,
                                       float(weight_decay), it + 1, 1.0, model._stream()), "leaf_adamw_step")
        better = best_cos * loss_weight < cos * loss_weight               # :214
        best_cos = torch.where(better, cos, best_cos)
        best_ids = torch.where(better[seg_t], ids, best_ids)
        if print_step and (it % print_step == 0 or it == iters - 1):
            logging.info(f"step {it}: mean cosine {float(cos.mean()):.4f}, mean best {float(best_cos.mean()):.4f}")
    ids_host = best_ids.cpu().numpy()
    return [ids_host[cu[b] - 2 * b: cu[b] - 2 * b + plens[b]].copy() for b in range(B)], best_cos.cpu().numpy()


def invert_text(model, tokenizer, captions: Optional[Sequence[str]] = None, targets=None, prompt_len: Union[str, int] = "match",
                iters: int = 3000, lr: float = 0.1, weight_decay: float = 0.1, loss_weight: float = 1.0, seed: int = 0,
                init_ids=None, batch: int = 64, print_step: Optional[int] = None, prompt_bs: int = 1, target_images=None,
                avg_text: bool = False) -> List[dict]:
    """Invert one target embedding per entry: ``captions`` (targets = their ``encode_text(precise=True)`` embeddings) and / or
    ``targets`` [N, embed_dim] given directly.  ``prompt_len``: "match" (the caption's own token count, run_coco.py:17-21; needs
    captions) or an int.  ``init_ids``: one id array per inversion instead of the seeded random start.  Returns the reference's
    dict per inversion: ``original``, ``reconstructed``, ``ids_rec``, ``sim``, ``ids_orig`` (the caption's full token row, or None).
    ``sim`` is the cosine between the target and ``encode_text(precise=True)`` of [SOT, ids_rec, EOT] -- the fp32-grade forward,
    as eval_textfare's columns; it is the embedding a user of the reconstructed ids gets (pooled at their first EOT)."""
    if prompt_bs != 1:
        raise NotImplementedError("invert_text optimises one prompt per target (the reference's prompt_bs = 1); prompt_bs > 1 is out of scope")
    if target_images is not None:
        raise NotImplementedError("image targets need an image tower, which this project does not have: pass text captions or target embeddings")
    if avg_text:
        raise NotImplementedError("avg_text pooling is out of scope: the inversion pools at the template's EOT slot")
    if captions is None and targets is None:
        raise ValueError("give captions and / or targets")
    if iters < 1 or batch < 1:
        raise ValueError("iters >= 1 and batch >= 1")
    ctx = model.cfg.context_length
    N = len(captions) if captions is not None else len(targets)
    ids_orig = tokenizer.encode_batch(list(captions)) if captions is not None else None
    if targets is None:
        targets = model.encode_text(ids_orig, precise=True)
    targets = torch.as_tensor(targets, dtype=torch.float32).to(model.device).reshape(N, model.cfg.embed_dim).contiguous()
    if prompt_len == "match":
        if ids_orig is None:
            raise ValueError('prompt_len="match" needs captions; give an int with bare targets')
        plens = [int((row != 0).sum()) - 2 for row in ids_orig]
    else:
        plens = [int(prompt_len)] * N
    if min(plens) < 1 or max(plens) > ctx - 2:
        raise ValueError(f"prompt lengths must be in 1..{ctx - 2}, got {min(plens)}..{max(plens)}")
    if init_ids is not None:
        starts = [np.asarray(a, np.int32).reshape(-1) for a in init_ids]
        if len(starts) != N or any(len(a) != p for a, p in zip(starts, plens)):
            raise ValueError("init_ids: one array of prompt_len ids per inversion")
    else:
        starts = [initial_ids(p, seed, model.cfg.vocab_size) for p in plens]
    rec, loop_cos = [], []
    for i in range(0, N, batch):
        ids_b, cos_b = _invert_batch(model, targets[i:i + batch].contiguous(), plens[i:i + batch], starts[i:i + batch], iters, lr,
                                     weight_decay, loss_weight, print_step)
        rec += ids_b
        loop_cos += list(cos_b)
    rows = np.zeros((N, ctx), np.int32)
    for b, ids in enumerate(rec):
        rows[b, 0], rows[b, 1:1 + len(ids)], rows[b, 1 + len(ids)] = SOT, ids, EOT
    f = model.encode_text(rows, precise=True)
    sim = torch.nn.functional.cosine_similarity(f, targets, dim=-1).cpu().numpy()
    return [{"original": captions[b] if captions is not None else None, "reconstructed": tokenizer.decode(rec[b]),
             "ids_rec": [int(t) for t in rec[b]], "sim": float(sim[b]),
             "ids_orig": [int(t) for t in ids_orig[b]] if ids_orig is not None else None, "sim_loop": float(loop_cos[b])}
            for b in range(N)]


def summarize(results: Sequence[dict]) -> dict:
    """The three numbers compute_metrics.py prints (:54-62): mean cosine, word accuracy, token accuracy (captions required for the
    last two)."""
    out = {"cos-sim": float(np.mean([r["sim"] for r in results]))}
    if results and all(r["original"] is not None for r in results):
        out["word accuracy"] = word_accuracy([r["reconstructed"] for r in results], [r["original"] for r in results])
        out["token accuracy"] = token_accuracy([r["ids_rec"] for r in results], [r["ids_orig"] for r in results])
    return out
