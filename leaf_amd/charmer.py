"""Charmer and brute-force string attacks, batched over captions, on the HIP scoring path.

Restates the reference's deterministic attacks (utils_attacks.py):

* ``attack_text_charmer_inference``   utils_attacks.py:451-580 -- the original Charmer attack, the one the reference uses to
  MEASURE robustness (eval_textfare.py:129-130, eval_retrieval.py:78) and to train with under ``--use_charmer`` (utils_AT.py:297-304)
* ``attack_text_bruteforce``          utils_attacks.py:395-449 -- every position x every character (eval_textfare.py:131-132)
* ``attack_text_charmer_classification`` utils_attacks.py:582-643 -- Charmer with the margin loss over a class matrix and a stop
  per caption as soon as its prediction flips: the attack of the zero-shot text classification evaluation (eval_zero_shot_text.py)

Each edit of Charmer has two stages.  Stage 1 scores, for every position z in 0..2L of the expanded view (``generate_sentence``),
the insert / replace-with / delete-a-space edit and keeps the top-n positions; stage 2 scores every character of V at those positions
(in top-n order, then V order) and keeps the first arg-max.  The reference runs one sentence at a time; here the candidates of many
captions go into one launch: every caption's stage is padded to the longest one (R = max_b candidates per caption, the padding slots
hold the no-op edit -- one recomputed row under prefix reuse) so that the rectangular ``score_candidates`` path is reused unchanged,
and ``count[b]`` masks the padding out in the segmented selection kernel (``leaf_select_topk``, leaf_amd/csrc/select.hip).

Kept on purpose, as the reference does it: **the last candidate of every stage is never scored.**  The reference's chunk loop caps
``end`` at ``len(SS) - 1`` (utils_attacks.py:488, :543, :422), so stage 1 picks from positions 0..2L-1 only, the last (position,
V[-1]) pair of stage 2 is never a candidate, and brute force skips its last candidate.  ``count`` carries this.

Charmer draws no random numbers: a batched run gives exactly the adversarial sentences of the one-sentence loop (every row has
the same bits whichever launch computes it), whatever the grouping.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from .attacks import DEFAULT_V, _apply_edit, _stage_candidates, duplicate_map, first_difference, lend_duplicates

SCORE_MAX_COLUMNS = 8192        # candidates per caption and launch the score kernel takes (elementwise.hip: leaf_launch_score)


# ----------------------------------------------------------------------------- stage plans (host, no device)
def stage1_plan(sentences: Sequence[str]):
    """(z, c, count) of stage 1 (utils_attacks.py:470-477): column j of caption b is position j with a space
    (``generate_all_sentences(S, [' '], alternative=-1)``), count[b] = 2 L_b -- position 2 L_b, the last candidate, is not scored.
    Padding slots: the no-op edit (z = 0, c = -1)."""
    count = np.array([2 * len(S) for S in sentences], dtype=np.int32)
    R = max(1, int(count.max()) if len(sentences) else 1)
    cols = np.arange(R, dtype=np.int32)[None, :]
    real = cols < count[:, None]
    z = np.where(real, cols, 0).astype(np.int32)
    c = np.where(real, ord(' '), -1).astype(np.int32)
    return z, c, count


def stage2_plan(top: np.ndarray, m: np.ndarray, V: Sequence[int]):
    """(z, c, count) of stage 2 (utils_attacks.py:509-511): for caption b the first m[b] positions of ``top[b]`` (top-n order), for
    each of them all of V in order; count[b] = m[b] |V| - 1 (the last pair is not scored, :543)."""
    Varr = np.asarray(V, dtype=np.int32)
    nv = len(Varr)
    B = top.shape[0]
    m = np.asarray(m, dtype=np.int32)
    R = max(1, int(m.max()) * nv if B else 1)
    z = np.zeros((B, R), dtype=np.int32)
    c = np.full((B, R), -1, dtype=np.int32)
    for b in range(B):
        w = int(m[b]) * nv
        z[b, :w] = np.repeat(top[b, :m[b]].astype(np.int32), nv)
        c[b, :w] = np.tile(Varr, int(m[b]))
    count = np.maximum(m * nv - 1, 0).astype(np.int32)
    return z, c, count


def bruteforce_columns(L: int, nv: int) -> int:
    """candidates of brute force on a caption of L characters: every position of the expanded view x every character"""
    return (2 * L + 1) * nv


def bruteforce_plan(sentences: Sequence[str], V: Sequence[int], c0: int = 0, width: Optional[int] = None):
    """(z, c, count) of columns [c0, c0 + width) of brute force (utils_attacks.py:411): column j is position j // |V| with
    character V[j % |V|]; count[b] = the real columns of this window, where the whole list's last candidate is not scored (:422)."""
    Varr = np.asarray(V, dtype=np.int32)
    nv = len(Varr)
    total = np.array([bruteforce_columns(len(S), nv) - 1 for S in sentences], dtype=np.int32)      # scored candidates
    if width is None:
        width = max(1, int(total.max()) - c0 if len(sentences) else 1)
    count = np.clip(total - c0, 0, width).astype(np.int32)
    cols = c0 + np.arange(width, dtype=np.int32)[None, :]
    real = (cols - c0) < count[:, None]
    z = np.where(real, cols // nv, 0).astype(np.int32)
    c = np.where(real, Varr[cols % nv], -1).astype(np.int32)
    return z, c, count


def render_plan(sentences: Sequence[str], z: np.ndarray, c: np.ndarray, count: np.ndarray) -> List[List[str]]:
    """the scored candidate strings of a plan, per caption (after ``prepare_stage`` for --constrain)"""
    return [[_apply_edit(S, int(z[b, r]), int(c[b, r])) for r in range(int(count[b]))] for b, S in enumerate(sentences)]


def prepare_stage(tokenizer, sentences, z, c, constrain: bool):
    """Token ids / lengths of a padded plan.  With ``constrain`` an invalid candidate becomes the no-op edit, i.e. the sentence OF THE
    CURRENT EDIT (utils_attacks.py:479-482,532-537; brute force compares against the original, which is the same sentence for its
    single edit): ``z`` / ``c`` are rewritten in place (native ``constrain_mask`` or the Python rule, leaf_amd/attacks.py)."""
    return _stage_candidates(tokenizer, list(sentences), z, c, constrain, None)


# ----------------------------------------------------------------------------- device selection
def select_topk(loss, count, n: int, col_offset: int = 0, accumulate: bool = False, out=None):
    """``leaf_select_topk`` on fp32 CUDA ``loss`` [B, ld]: per row the min(n, count[b]) largest of columns [0, count[b]) in
    descending order (ties -> lower column, NaN first), unused slots idx -1 / val -inf.  ``count``: host int array or CUDA int32 [B].
    ``accumulate`` (n == 1): merge into ``out`` = (idx int32 [B, 1], val fp32 [B, 1]), first maximum of the whole list winning,
    column reported as col_offset + j.  Returns (idx, val)."""
    import torch
    from . import _lib
    B, ld = loss.shape
    loss = loss.contiguous()
    dev = loss.device
    if not isinstance(count, torch.Tensor):
        count = torch.from_numpy(np.ascontiguousarray(count, dtype=np.int32)).pin_memory().to(dev, non_blocking=True)
    count = count.to(device=dev, dtype=torch.int32).contiguous()
    if accumulate:
        if out is None:
            raise ValueError("accumulate needs out = (idx, val) from new_accumulator()")
        idx, val = out
    else:
        idx = torch.empty(B, n, dtype=torch.int32, device=dev)
        val = torch.empty(B, n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.lib().leaf_select_topk(loss.data_ptr() if B else None, ld, count.data_ptr() if B else None, B, n, col_offset,
                                           int(bool(accumulate)), idx.data_ptr() if B else None, val.data_ptr() if B else None,
                                           stream), "leaf_select_topk")
    return idx, val


def margin_scores(feat, class_features, labels, rho: int, want_logits: bool = False, want_features: bool = False):
    """``leaf_op_classify`` (leaf_amd/csrc/classify.hip) on given unit feature rows ``feat`` fp32 CUDA [B * rho, D]: the score of
    ``LeafCLIPText.score_candidates_cls`` without the forward.  ``class_features`` fp32 CUDA [C, D] unit rows, ``labels`` [B] host
    ints, checked here to lie in [0, C).  Returns (best_idx [B], best_feat [B, D] or None, loss [B, rho], pred [B, rho],
    logits [B * rho, C] or None)."""
    import torch
    from . import _lib
    feat = feat.contiguous()
    dev = feat.device
    cf = class_features.to(device=dev, dtype=torch.float32).contiguous()
    n_cls, D = int(cf.shape[0]), int(feat.shape[1])
    lab = np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int64)
    B = int(lab.size)
    if feat.shape[0] != B * rho or cf.shape[1] != D:
        raise ValueError(f"feat {tuple(feat.shape)} / class_features {tuple(cf.shape)} do not match B * rho = {B} * {rho}")
    if B and (lab.min() < 0 or lab.max() >= n_cls):
        raise ValueError(f"label outside [0, {n_cls}): {lab[(lab < 0) | (lab >= n_cls)][:4].tolist()}")
    lab_dev = torch.from_numpy(lab.astype(np.int32)).to(dev)
    idx = torch.empty(B, dtype=torch.int32, device=dev)
    best = torch.empty(B, D, dtype=torch.float32, device=dev) if want_features else None
    loss = torch.empty(B, rho, dtype=torch.float32, device=dev)
    pred = torch.empty(B, rho, dtype=torch.int32, device=dev)
    logits = torch.empty(B * rho, n_cls, dtype=torch.float32, device=dev) if want_logits else None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.lib().leaf_op_classify(feat.data_ptr(), cf.data_ptr(), lab_dev.data_ptr(), B, rho, D, n_cls, loss.data_ptr(),
                                           pred.data_ptr(), logits.data_ptr() if want_logits else None, idx.data_ptr(),
                                           best.data_ptr() if want_features else None, stream), "leaf_op_classify")
    return idx, best, loss, pred, logits


def new_accumulator(B: int, device):
    """(idx, val) = (-1, -inf) per row: the start of an ``accumulate`` chain"""
    import torch
    return (torch.full((B, 1), -1, dtype=torch.int32, device=device),
            torch.full((B, 1), float("-inf"), dtype=torch.float32, device=device))


# ----------------------------------------------------------------------------- scoring of one padded stage
class _Scorer:
    """Scores a padded [Bg, R] plan against the targets of its captions and returns (the COMPLETE loss matrix on the device, the
    predicted classes or None).  Under prefix reuse (EOT trimming on) only the positions from a candidate's first changed token on
    are computed, from the clean captions' K/V (``encode_text_kv``, once per edit); with ``dedupe`` a candidate whose id row repeats
    an earlier one of the same caption (the CLIP tokenizer lower-cases and collapses whitespace: 'a' / 'A', the -1 edit at every
    even position, a space next to a space) is not computed again: its slot gets the no-op edit and the first occurrence's loss is
    copied into it (leaf_amd/attacks.py: ``lend_duplicates``).  The target of a caption is its anchor row under ``objective``, or,
    with ``class_features`` (unit rows [C, D]), its label (host int) under the classification margin loss
    (``score_candidates_cls``): the predicted classes then come back with the losses, duplicates copying both."""

    def __init__(self, model, objective, dedupe, stats, class_features=None):
        self.model = model
        self.reuse = hasattr(model, "encode_text_kv") and getattr(model, "trim_rows", False)
        self.dedupe = dedupe and self.reuse
        self.stats = stats
        if class_features is None:
            self._score = lambda toks, target_g, R, **kw: (
                model.score_candidates(toks, target_g, R, objective, want_features=False, want_loss=True, **kw)[2], None)
        else:
            self._score = lambda toks, target_g, R, **kw: model.score_candidates_cls(toks, class_features, target_g, R, **kw)[2:4]

    def kv(self, base, slot):
        return self.model.encode_text_kv(base, slot=slot) if self.reuse else None

    def loss(self, toks, lens, base, kv, target_g, R, count):
        import torch
        Bg = len(target_g)
        pl = first_difference(toks, base, R) if self.reuse else None
        dup = duplicate_map(toks, Bg, R) if self.dedupe else None
        is_dup = None if dup is None else (dup != np.arange(R)[None, :])
        if self.stats is not None:
            real = np.arange(R)[None, :] < np.asarray(count)[:, None]
            self.stats["candidates"] = self.stats.get("candidates", 0) + int(real.sum())
            self.stats["duplicates"] = self.stats.get("duplicates", 0) + (int((is_dup & real).sum()) if is_dup is not None else 0)
            self.stats["full_rows"] = self.stats.get("full_rows", 0) + int(
                (lens if lens is not None else toks.reshape(Bg * R, -1).argmax(-1) + 1).reshape(Bg, R)[real].sum())
            rows0 = self.model.rows_scored
        lent = is_dup is not None and is_dup.any()
        if lent:
            toks, lens, pl = lend_duplicates(toks, lens, pl, base, dup)
        loss, pred = self._score(toks, target_g, R, seq_lens=lens, prefix_lens=pl, kv=kv)
        if lent:
            dup_dev = torch.from_numpy(dup).pin_memory().to(loss.device, non_blocking=True)
            loss = loss.gather(1, dup_dev)
            if pred is not None:
                pred = pred.gather(1, dup_dev)
        if self.stats is not None:
            self.stats["computed_rows"] = self.stats.get("computed_rows", 0) + (self.model.rows_scored - rows0)
        return loss, pred


def _to_host(t):
    """non-blocking copy into pinned host memory + an event; returns finish() -> numpy array"""
    import torch
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()

    def finish():
        ev.synchronize()
        return host.numpy()
    return finish


def _groups(idx: Sequence[int], pipeline: int, width_of, max_rows: int) -> List[List[int]]:
    """contiguous caption groups: ``pipeline`` of them at least, each with len(g) * max width <= max_rows (one caption at least)"""
    idx = list(idx)
    if not idx:
        return []
    pipeline = max(1, min(int(pipeline), len(idx)))
    bounds = np.linspace(0, len(idx), pipeline + 1).astype(int)
    out = []
    for p in range(pipeline):
        cur, wmax = [], 0
        for b in idx[bounds[p]:bounds[p + 1]]:
            w = max(wmax, width_of(b))
            if cur and (len(cur) + 1) * w > max_rows:
                out.append(cur)
                cur, w = [], width_of(b)
            cur.append(b)
            wmax = w
        if cur:
            out.append(cur)
    return out


def _prepare_anchor(anchor_features, objective):
    if objective not in ("l2", "negl2", "sim", "dissim"):
        raise ValueError(f"objective {objective!r}: one of l2, negl2, sim, dissim")
    if objective in ("dissim", "sim"):
        anchor_features /= anchor_features.norm(dim=-1, keepdim=True)     # in place, as the reference does
    return anchor_features


# ----------------------------------------------------------------------------- batched attacks
def _charmer_edits(scorer, tokenizer, sentences, target_of, n, k, V, constrain, pipeline, max_rows, after_edit, stop_idle,
                   return_trace, return_losses, return_picks, return_preds=None):
    """Up to ``k`` Charmer edits on the captions that are active (at first: the non-empty ones).  ``target_of(g)``: what
    ``scorer.loss`` compares the captions ``g`` (indices into the batch) with.  ``after_edit(sentences, picks)`` -> the captions of
    the next edit, ``picks[b]`` being the predicted class of caption b's pick (None from a scorer without classes; captions
    without a pick are absent); with ``stop_idle`` the loop ends when that set is empty.  Returns (sentences, edits received per
    caption)."""
    sentences = list(sentences)
    B = len(sentences)
    if pipeline is None:
        pipeline = 2 if (scorer.reuse and B >= 64) else 1
    nv = len(V)
    received = [0] * B
    active = [b for b, S in enumerate(sentences) if len(S) > 0]
    for _ in range(k):
        if stop_idle and not active:
            break
        groups = _groups(active, pipeline, lambda b: max(2 * len(sentences[b]), min(n, 2 * len(sentences[b])) * nv), max_rows)
        base_all = tokenizer.encode_batch(sentences) if scorer.reuse else None
        st1 = []
        for gi, g in enumerate(groups):
            sg = [sentences[b] for b in g]
            base = base_all[g] if scorer.reuse else None
            kv = scorer.kv(base, gi)          # the clean captions once per edit: their K/V serve both stages
            z, c, count = stage1_plan(sg)
            R = z.shape[1]
            if R > SCORE_MAX_COLUMNS:
                raise ValueError(f"a caption of {max(map(len, sg))} characters: stage 1 has {R} candidates, more than the "
                                 f"{SCORE_MAX_COLUMNS} per caption one scoring launch takes")
            toks, lens = prepare_stage(tokenizer, sg, z, c, constrain)
            target_g = target_of(g)
            loss, _ = scorer.loss(toks, lens, base, kv, target_g, R, count)
            idx, _ = select_topk(loss, count, n)
            st1.append((sg, base, kv, target_g, z, c, count, _to_host(idx), _to_host(loss) if return_losses is not None else None))
        st2 = []
        for sg, base, kv, target_g, z1, c1, count1, fin, fin_loss in st1:
            top = fin()
            m = np.minimum(n, count1)
            st1_out = (render_plan(sg, z1, c1, count1) if return_trace is not None else None,
                       [fin_loss()[i, :count1[i]] for i in range(len(sg))] if fin_loss is not None else None,
                       [top[i, :m[i]] for i in range(len(sg))])
            z, c, count = stage2_plan(top, m, V)
            R = z.shape[1]
            if R > SCORE_MAX_COLUMNS:
                raise ValueError(f"stage 2 has {R} = n |V| candidates per caption, more than the {SCORE_MAX_COLUMNS} one scoring "
                                 f"launch takes: lower n")
            toks, lens = prepare_stage(tokenizer, sg, z, c, constrain)
            loss, pred = scorer.loss(toks, lens, base, kv, target_g, R, count)
            idx, _ = select_topk(loss, count, 1)
            # the predicted class of the pick (a row without one: unused)
            fin_pred = _to_host(pred.gather(1, idx.clamp(min=0).long())) if pred is not None else None
            st2.append((sg, z, c, count, _to_host(idx), fin_pred, _to_host(loss) if return_losses is not None else None, st1_out))
        # hooks: one entry per stage, captions in input order (captions that sat out: empty entries)
        trace1, trace2 = ([[] for _ in range(B)] for _ in range(2))
        loss1, loss2 = ([np.zeros(0, np.float32) for _ in range(B)] for _ in range(2))
        pick1, pick2 = ([np.zeros(0, np.int64) for _ in range(B)] for _ in range(2))
        preds = [None] * B
        picks = {}
        for g, (sg, z, c, count, fin, fin_pred, fin_loss, st1_out) in zip(groups, st2):
            best = fin()[:, 0]
            bpred = fin_pred()[:, 0] if fin_pred is not None else None
            lh = fin_loss() if fin_loss is not None else None
            strings = render_plan(sg, z, c, count) if return_trace is not None else None
            for i, b in enumerate(g):
                j = int(best[i])
                if j >= 0:
                    sentences[b] = _apply_edit(sg[i], int(z[i, j]), int(c[i, j]))
                    received[b] += 1
                    picks[b] = preds[b] = int(bpred[i]) if bpred is not None else None
                if st1_out[0] is not None:
                    trace1[b], trace2[b] = st1_out[0][i], strings[i]
                if st1_out[1] is not None:
                    loss1[b], loss2[b] = st1_out[1][i], lh[i, :count[i]]
                pick1[b] = st1_out[2][i]
                pick2[b] = np.array([j] if j >= 0 else [], dtype=np.int64)
        if return_trace is not None:
            return_trace += [trace1, trace2]
        if return_losses is not None:
            return_losses += [loss1, loss2]
        if return_picks is not None:
            return_picks += [pick1, pick2]
        if return_preds is not None:
            return_preds.append(preds)
        active = after_edit(sentences, picks)
    return sentences, received


def attack_text_charmer(model, tokenizer, sentences, anchor_features, objective: str = "l2", n: int = 10, k: int = 1, V=DEFAULT_V,
                        constrain: bool = False, debug: bool = False, dedupe: bool = True, pipeline: Optional[int] = None,
                        max_rows: int = 65536, return_trace: Optional[list] = None, return_losses: Optional[list] = None,
                        return_picks: Optional[list] = None, stats: Optional[dict] = None):
    """Charmer (utils_attacks.py:451-580) on a batch of captions.  ``model``: a ``leaf_amd.model.LeafCLIPText``; ``anchor_features``
    fp32 CUDA [B, D] (normalised in place for sim / dissim, as the reference does).  Returns (adversarial sentences, dists) with
    dists[b] the reference's ``dist + 1``.

    An empty caption is returned unchanged (the reference raises on it: its stage-1 loss list is empty).  ``pipeline`` (default 2
    for B >= 64 under prefix reuse, else 1) and ``max_rows`` (candidate rows per launch) only decide the grouping of captions into
    launches: while the GPU scores one group the host builds the next group's candidates; results do not depend on it.
    Test / tool hooks: ``return_trace`` receives per stage the scored candidate strings per caption, ``return_losses`` the stage's
    loss rows (numpy, [count[b]] per caption), ``return_picks`` per stage the picked columns per caption, ``stats`` candidate / row
    counts (duplicates skipped, rows computed under prefix reuse)."""
    import torch
    anchor_features = _prepare_anchor(anchor_features, objective)

    def after_edit(sentences, picks):          # every non-empty caption takes every edit
        if debug and sentences:
            print(sentences[0])
        return [b for b, S in enumerate(sentences) if len(S) > 0]

    sentences, _ = _charmer_edits(_Scorer(model, objective, dedupe, stats), tokenizer, sentences,
                                  lambda g: anchor_features[torch.as_tensor(g, device=anchor_features.device)], n, k, V, constrain,
                                  pipeline, max_rows, after_edit, False, return_trace, return_losses, return_picks)
    return sentences, [max(k, 1)] * len(sentences)


def attack_text_charmer_classification_batched(model, tokenizer, sentences, class_features, labels, n: int = 10, k: int = 1, V=DEFAULT_V,
                                               dedupe: bool = True, pipeline: Optional[int] = None, max_rows: int = 65536,
                                               return_trace: Optional[list] = None, return_losses: Optional[list] = None,
                                               return_picks: Optional[list] = None, return_preds: Optional[list] = None,
                                               stats: Optional[dict] = None, scorer=None):
    """Charmer with the classification margin loss (attack_text_charmer_classification, utils_attacks.py:582-643) on a batch of
    captions.  ``class_features`` fp32 CUDA [C, D], unit rows -- the caller normalises them, nothing is normalised here --,
    ``labels`` [B] host ints in [0, C).  Each candidate's loss is max_{c != label} logit[c] - logit[label] over its cosine
    similarities to the classes (margin_loss_lm, :145-151), on the device (leaf_amd/csrc/classify.hip).  Stages, the never-scored
    last candidate of each stage and the selection are those of ``attack_text_charmer``.

    Early stop (:641): after an edit, caption b stops when the predicted class of its picked candidate differs from labels[b]; it
    leaves the active set and the later edits run on the remaining captions only.  A caption that is misclassified before the first
    edit still receives that edit, as in the reference.  Returns (adversarial sentences, dists) with dists[b] the number of edits
    caption b received (the reference's ``dist + 1``); an empty caption is returned unchanged with dist 0 (the reference raises).

    Stage 1 keeps min(n, count[b]) positions.  The reference's ``min(n, text_sims.shape[0])`` (:611) is the same number whenever the
    stage fits one of its 2,560-row chunks; for a longer sentence it takes the LAST chunk's row count, which is not reproduced.
    There is no ``constrain`` argument (the reference's attack has none).  No random numbers are drawn: grouping, pipelining and
    ``dedupe`` change no sentence, dist or loss bit.

    Hooks as in ``attack_text_charmer`` (two entries per edit; a caption that has stopped has empty entries); ``return_preds``
    receives per edit the predicted class of each caption's pick (None for a caption that did not take part).  ``scorer``: a test
    seam, an object with ``reuse`` / ``kv`` / ``loss`` like ``_Scorer`` in classification mode."""
    sentences = list(sentences)
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    if labels.size != len(sentences):
        raise ValueError(f"{labels.size} labels for {len(sentences)} sentences")
    if scorer is None:
        scorer = _Scorer(model, None, dedupe, stats, class_features=class_features)
    # a caption takes the next edit while its pick is still classified as its label; one without a pick leaves too
    return _charmer_edits(scorer, tokenizer, sentences, lambda g: labels[g], n, k, V, False, pipeline, max_rows,
                          lambda sentences, picks: [b for b, p in picks.items() if p == labels[b]], True,
                          return_trace, return_losses, return_picks, return_preds)


def attack_text_bruteforce_batched(model, tokenizer, sentences, anchor_features, objective: str = "l2", V=DEFAULT_V,
                                   constrain: bool = False, debug: bool = False, dedupe: bool = True, chunk_cols: int = 4096,
                                   max_rows: int = 65536, return_losses: Optional[list] = None, stats: Optional[dict] = None):
    """Brute force (utils_attacks.py:395-449) on a batch of captions: every position x every character of V, one edit, the first
    arg-max of the scored candidates (all but the last).  Captions go into launches in groups of at most ``max_rows`` candidate rows;
    a long caption is scored in column windows of ``chunk_cols`` merged by the selection kernel's ``accumulate`` mode ("first maximum
    wins" over the whole list).  Neither changes a result.  Returns (adversarial sentences, dists = 1).  ``return_losses``: the
    whole scored loss row per caption (numpy).  Objectives as Charmer's (the reference's brute force implements l2 and dissim)."""
    import torch
    sentences = list(sentences)
    B = len(sentences)
    anchor_features = _prepare_anchor(anchor_features, objective)
    scorer = _Scorer(model, objective, dedupe, stats)
    nv = len(V)
    chunk_cols = max(1, min(int(chunk_cols), SCORE_MAX_COLUMNS))
    total = [bruteforce_columns(len(S), nv) - 1 for S in sentences]
    groups = _groups(range(B), 1, lambda b: min(chunk_cols, max(total[b], 1)), max_rows)
    base_all = tokenizer.encode_batch(sentences) if scorer.reuse else None
    new = list(sentences)
    losses = [[] for _ in range(B)]
    pending = []
    for gi, g in enumerate(groups):
        sg = [sentences[b] for b in g]
        base = base_all[g] if scorer.reuse else None
        kv = scorer.kv(base, gi % 2)          # two cache slots: group g + 1's K/V pass may run while group g is still scored
        anchor_g = anchor_features[torch.as_tensor(g, device=anchor_features.device)]
        acc = new_accumulator(len(g), anchor_features.device)
        tmax = max(total[b] for b in g)
        plans, fins = [], []
        for c0 in range(0, max(tmax, 1), chunk_cols):
            width = min(chunk_cols, max(tmax - c0, 1))
            z, c, count = bruteforce_plan(sg, V, c0, width)
            toks, lens = prepare_stage(tokenizer, sg, z, c, constrain)
            loss, _ = scorer.loss(toks, lens, base, kv, anchor_g, width, count)
            select_topk(loss, count, 1, col_offset=c0, accumulate=True, out=acc)
            plans.append((c0, z, c, count))
            if return_losses is not None:
                fins.append(_to_host(loss))
        pending.append((g, sg, plans, _to_host(acc[0]), fins))
        if len(pending) == 2:          # keep at most two groups in flight (two K/V slots)
            _bruteforce_finish(pending.pop(0), new, losses, return_losses is not None)
    for p in pending:
        _bruteforce_finish(p, new, losses, return_losses is not None)
    if return_losses is not None:
        return_losses += [[np.concatenate(l) if l else np.zeros(0, np.float32) for l in losses]]
    if debug and B:
        print(new[0])
    return new, [1] * B


def _bruteforce_finish(p, new, losses, want_losses):
    g, sg, plans, fin, fins = p
    best = fin()[:, 0]
    for i, b in enumerate(g):
        j = int(best[i])
        if j < 0:
            continue
        for c0, z, c, count in plans:
            if c0 <= j < c0 + z.shape[1]:
                new[b] = _apply_edit(sg[i], int(z[i, j - c0]), int(c[i, j - c0]))
                break
    if want_losses:
        for (c0, z, c, count), f in zip(plans, fins):
            lh = f()
            for i, b in enumerate(g):
                losses[b].append(lh[i, :count[i]])


# ----------------------------------------------------------------------------- drop-in wrappers (reference signatures)
def _one(anchor_features):
    return anchor_features.reshape(1, -1)


def attack_text_charmer_inference(model, tokenizer, sentence, anchor_features, device=None, objective="l2", n=10, k=1, V=DEFAULT_V,
                                  constrain=False, debug=False, batch_size=20 * 128, model_2=None, model_2_anchor_features=None):
    """utils_attacks.py:451-580 with its signature and return (sentence, dist).  ``batch_size`` is accepted for compatibility and
    changes nothing (the reference's row chunking does not change its result either).  ``model_2`` (the dual-encoder SDXL path) is
    not supported.  An empty sentence is returned unchanged (the reference raises)."""
    if model_2 is not None or model_2_anchor_features is not None:
        raise NotImplementedError("model_2 (dual text encoder) is not supported by the batched Charmer attack")
    # a view of the caller's tensor: the in-place normalisation for sim / dissim reaches it, as in the reference
    adv, dists = attack_text_charmer(model, tokenizer, [sentence], _one(anchor_features), objective, n, k, V, constrain, debug)
    return adv[0], dists[0]


def attack_text_bruteforce(model, tokenizer, sentence, anchor_features, device=None, batch_size=20 * 128, objective="l2", k=1,
                           V=DEFAULT_V, constrain=False, debug=False):
    """utils_attacks.py:395-449 with its signature and return (sentence, 1).  ``k`` is ignored, as in the reference (one edit);
    ``batch_size`` changes nothing."""
    adv, dists = attack_text_bruteforce_batched(model, tokenizer, [sentence], _one(anchor_features), objective, V, constrain, debug)
    return adv[0], dists[0]


def attack_text_charmer_classification(model, tokenizer, sentence, image_features, label, device=None, n=10, k=1, V=DEFAULT_V, debug=False,
                                       batch_size=128 * 20):
    """utils_attacks.py:582-643 with its signature and return (sentence, dist).  ``image_features`` [C, D]: the class matrix, unit
    rows (the reference does not normalise it either).  ``batch_size`` is accepted for compatibility and changes nothing.  An empty
    sentence is returned unchanged with dist 0 (the reference raises)."""
    adv, dists = attack_text_charmer_classification_batched(model, tokenizer, [sentence], image_features.reshape(len(image_features), -1),
                                                            [int(label)], n, k, V)
    if debug:
        print(adv[0])
    return adv[0], dists[0]

