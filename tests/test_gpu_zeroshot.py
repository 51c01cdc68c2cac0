"""Classification Charmer on the MI355X (leaf_amd/csrc/classify.hip, leaf_amd/charmer.py, eval_zero_shot_text.py): the margin-loss
kernel against numpy; grouping, prefix reuse and duplicate skipping change no bit; the batched attack replays the reference's own
runs (tests/golden/zeroshot_trace.*) under the margin rule of tests/test_gpu_charmer.py; the drop-in and the CLI run end to end."""
import csv
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOSS_CAP = 4e-3      # derived, not measured -- see test_tiny_model_replays_the_reference


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def fx(golden_dir):
    with open(os.path.join(golden_dir, "zeroshot_trace.json")) as f:
        t = json.load(f)
    return t, np.load(os.path.join(golden_dir, "zeroshot_trace.npz"))


@pytest.fixture(scope="module")
def tiny(torch_mod):
    from leaf_amd.model import create_model
    return create_model("tiny-test-quickgelu", device="cuda:0", seed=12)


def _tok(native):
    if native:
        from leaf_amd.native_text import NativeTokenizer
        return NativeTokenizer(n_threads=4)
    from leaf_amd.tokenizer import SimpleTokenizer
    return SimpleTokenizer()


def _first_argmax(row):
    """first index in the order of leaf_select_topk: NaN first, then the larger value, then the lower index"""
    nan = np.nonzero(np.isnan(row))[0]
    return int(nan[0]) if len(nan) else int(np.argmax(row))


# ----------------------------------------------------------------------------- 1. the kernel against numpy
def _unit(rng, n, D):
    x = rng.standard_normal((n, D)).astype(np.float32)
    return x / np.linalg.norm(x, axis=-1, keepdims=True).astype(np.float32)


@pytest.mark.parametrize("D", [64, 768, 1280])
@pytest.mark.parametrize("C", [2, 3, 4, 17, 1000])
def test_margin_kernel_against_numpy(torch_mod, C, D):
    """Logits and loss within D 2^-23 absolute, the worst-case fp32 inner-product bound for unit vectors (|fl(x.y) - x.y| <= D u |x||y|
    with u = 2^-24, so a logit is within D 2^-24 and the loss, a difference of two logits, within D 2^-23): derived, not measured --
    the measured maximum is printed.  best_idx and pred EXACTLY the first arg-max of the kernel's own loss row / logits."""
    from leaf_amd.charmer import margin_scores
    rng = np.random.default_rng(1000 * C + D)
    bound = D * 2.0 ** -23
    worst = 0.0
    rhos = [1, 5, 67, 8192] if (C <= 4 and D <= 768) else [1, 5, 67, 300]      # ragged: 1, a non-multiple of the tile, the maximum
    for rho in rhos:
        B = 3 if rho < 8192 else 2
        cls = _unit(rng, C, D)
        feat = _unit(rng, B * rho, D)
        labels = np.array([0, C - 1, min(1, C - 1)][:B])
        if C >= 3:
            cls[2] = cls[0]                                      # an exact tie between two classes: the lower index is the prediction
        if rho >= 5:
            feat[3] = feat[1]                                    # an exact tie between two candidates: the lower column wins
            feat[rho + 2, 7] = np.nan                            # a NaN row in caption 1: its loss is NaN and it ranks first
        idx, best, loss, pred, logits = margin_scores(torch_mod.from_numpy(feat).cuda(), torch_mod.from_numpy(cls).cuda(), labels, rho,
                                                      want_logits=True, want_features=True)
        idx, best, loss, pred, logits = (x.cpu().numpy() for x in (idx, best, loss, pred, logits))
        assert C < 3 or not (pred == 2).any()                    # class 2 repeats class 0 bit for bit and never wins the tie
        ref = feat.astype(np.float64) @ cls.astype(np.float64).T
        ok = ~np.isnan(ref)
        assert np.array_equal(np.isnan(logits), ~ok)
        worst = max(worst, float(np.abs(logits[ok] - ref[ok]).max()))
        assert np.abs(logits[ok] - ref[ok]).max() <= bound, (C, D, rho)
        for b in range(B):
            r = ref[b * rho:(b + 1) * rho]
            others = np.delete(r, labels[b], axis=1)
            ref_loss = others.max(-1) - r[:, labels[b]]
            fin = ~np.isnan(ref_loss)
            assert np.array_equal(np.isnan(loss[b]), ~fin)
            worst = max(worst, float(np.abs(loss[b][fin] - ref_loss[fin]).max()))
            assert np.abs(loss[b][fin] - ref_loss[fin]).max() <= bound, (C, D, rho, b)
            # the kernel's own loss from its own logits: exactly max over the others - the label's
            own = logits[b * rho:(b + 1) * rho]
            own_loss = np.delete(own, labels[b], axis=1).max(-1) - own[:, labels[b]]
            assert np.array_equal(loss[b][fin].view(np.int32), own_loss[fin].view(np.int32))
            assert idx[b] == _first_argmax(loss[b]), (C, D, rho, b)
            assert np.array_equal(best[b].view(np.int32), feat[b * rho + idx[b]].view(np.int32))
            assert np.array_equal(pred[b], [_first_argmax(row) for row in own]), (C, D, rho, b)
        if rho >= 5:
            assert loss[0, 1].view(np.int32) == loss[0, 3].view(np.int32) and idx[1] == 2 and np.isnan(loss[1, 2])
    print(f"classify C={C} D={D}: max |error| of logits / loss {worst:.3e}, bound {bound:.3e}")


def test_margin_kernel_does_not_depend_on_the_launch(torch_mod):
    """a candidate's logits, loss and pred are the same bits alone (B = rho = 1), inside any tile, at any place of any launch"""
    from leaf_amd.charmer import margin_scores
    rng = np.random.default_rng(7)
    for C, D in ((4, 64), (17, 768), (3, 70)):                   # 70: the unvectorised path
        cls = torch_mod.from_numpy(_unit(rng, C, D)).cuda()
        feat = _unit(rng, 6 * 37, D)
        whole = [x.cpu().numpy() for x in margin_scores(torch_mod.from_numpy(feat).cuda(), cls, [1] * 6, 37, want_logits=True)[2:]]
        flat = [x.cpu().numpy() for x in margin_scores(torch_mod.from_numpy(feat).cuda(), cls, [1], 6 * 37, want_logits=True)[2:]]
        assert np.array_equal(whole[0].reshape(-1).view(np.int32), flat[0].reshape(-1).view(np.int32))
        assert np.array_equal(whole[1].reshape(-1), flat[1].reshape(-1)) and np.array_equal(whole[2].view(np.int32), flat[2].view(np.int32))
        for i in (0, 1, 36, 37, 110, 221):
            one = [x.cpu().numpy() for x in margin_scores(torch_mod.from_numpy(feat[i:i + 1].copy()).cuda(), cls, [1], 1, want_logits=True)[2:]]
            assert one[0].view(np.int32)[0, 0] == whole[0].reshape(-1).view(np.int32)[i]
            assert one[1][0, 0] == whole[1].reshape(-1)[i] and np.array_equal(one[2][0].view(np.int32), whole[2][i].view(np.int32))


def test_margin_kernel_errors(torch_mod, tiny):
    from leaf_amd._lib import LeafHipError
    from leaf_amd.charmer import margin_scores
    rng = np.random.default_rng(3)
    feat = torch_mod.from_numpy(_unit(rng, 4, 64)).cuda()
    for C in (1, 1025):
        with pytest.raises(LeafHipError):
            margin_scores(feat, torch_mod.from_numpy(_unit(rng, C, 64)).cuda(), [0], 4)
    cls = torch_mod.from_numpy(_unit(rng, 3, 64)).cuda()
    for bad in (3, -1):
        with pytest.raises(ValueError):
            margin_scores(feat, cls, [bad], 4)
    ids = _tok(False).encode_batch(["a cat", "a dog"])
    with pytest.raises(ValueError):
        tiny.score_candidates_cls(ids, cls, [3], 2)
    for C in (1, 1025):
        with pytest.raises(LeafHipError):
            tiny.score_candidates_cls(ids, torch_mod.from_numpy(_unit(rng, C, 64)).cuda(), [0], 2)


# ----------------------------------------------------------------------------- 2. grouping changes no bit
def _run(tiny, tok, S, classes, labels, **kw):
    from leaf_amd.charmer import attack_text_charmer_classification_batched
    losses, preds = [], []
    adv, dists = attack_text_charmer_classification_batched(tiny, tok, S, classes, labels, n=5, k=4, return_losses=losses,
                                                            return_preds=preds, **kw)
    return adv, dists, losses, preds


def _same_bits(la, lb):
    return len(la) == len(lb) and all(np.array_equal(np.asarray(x, np.float32).view(np.int32), np.asarray(y, np.float32).view(np.int32))
                                      for sa, sb in zip(la, lb) for x, y in zip(sa, sb))


def test_grouping_prefix_reuse_and_dedupe_change_no_bit(torch_mod, fx, tiny):
    t, z = fx
    tok = _tok(True)
    S = t["sentences"][:8]
    V = t["V"]
    classes = torch_mod.from_numpy(z["mean3/classes"]).cuda()
    labels = [0] * 8
    adv8, d8, l8, p8 = _run(tiny, tok, S, classes, labels, V=V)
    assert max(d8) >= 2                                                    # the multi-edit loop runs
    for kw in (dict(dedupe=False), dict(pipeline=3, max_rows=700), dict(pipeline=2)):
        adv, d, l, p = _run(tiny, tok, S, classes, labels, V=V, **kw)
        assert (adv, d, p) == (adv8, d8, p8), kw
        assert _same_bits(l8, l), kw
    trim = tiny.trim_rows
    try:
        tiny.trim_rows = False                                             # no prefix reuse: whole candidates, dense rows
        adv, d, l, p = _run(tiny, tok, S, classes, labels, V=V)
    finally:
        tiny.trim_rows = trim
    assert (adv, d, p) == (adv8, d8, p8) and _same_bits(l8, l)
    for i, s in enumerate(S):                                              # B = 1 calls against the one B = 8 call
        adv1, d1, l1, p1 = _run(tiny, tok, [s], classes, [0], V=V)
        assert adv1[0] == adv8[i] and d1[0] == d8[i]
        for st in range(2 * d1[0]):
            assert np.array_equal(l1[st][0].view(np.int32), l8[st][i].view(np.int32)), (i, st)
        assert [p[0] for p in p1] == [p[i] for p in p8[:d1[0]]]


# ----------------------------------------------------------------------------- 3. replay of the reference's runs
def _check_case(t, z, key, adv, dists, losses, picks, preds, trace):
    """The batched run of one case against the reference's.  Every scored candidate's loss is compared with the fixture's up to and
    including the first decision where the two runs diverge (stage 1 of the first edit always).  Equal sentences AND equal dists are
    the rule; at the first divergent decision the margin rule of tests/test_gpu_charmer.py::_check_against_reference holds: a
    stage-1 top-n set may differ only where the reference's gap at the n-th place is within 4x the measured error, a stage-2 pick must
    be within 4x of the reference's best, a stop decision may differ only where the reference's best loss is within the measured
    error of 0 (the loss is <= 0 exactly while the label still has the largest logit).  Returns the measured maximum error."""
    case = t["cases"][key]
    nv = len(t["V"])
    worst = 0.0
    for i, row in enumerate(case["rows"]):
        label = row["label"]
        err = 0.0
        for e in range(max(row["dist"], dists[i])):
            if e >= row["dist"] or e >= dists[i]:
                # one run stopped after edit e - 1 and the other did not: only at a best loss within the error of 0
                best_ref = float(z[f"{key}/{row['sentence']}/{2 * e - 1}"].max())
                assert abs(best_ref) <= err, (key, i, e, best_ref, err)
                break
            l1_ref, l2_ref = z[f"{key}/{row['sentence']}/{2 * e}"], z[f"{key}/{row['sentence']}/{2 * e + 1}"]
            l1 = losses[2 * e][i]
            assert l1.shape == l1_ref.shape                        # the reference never encodes its last candidate either
            err = max(err, float(np.abs(l1 - l1_ref).max()))
            assert err <= LOSS_CAP, (key, i, e, err)
            top_ref, top = row["stages"][2 * e]["top"], [int(p) for p in picks[2 * e][i]]
            if set(top) != set(top_ref):
                srt = np.sort(l1_ref)[::-1]
                m = len(top_ref)
                assert m < len(srt) and srt[m - 1] - srt[m] <= 4 * (err + 1e-6), (key, i, e, top, top_ref)
                break                                              # different stage-2 candidates from here on
            l2 = losses[2 * e + 1][i]
            ref_col = {(top_ref[j // nv], j % nv): j for j in range(len(l2_ref))}
            mine = {(top[j // nv], j % nv): j for j in range(len(l2))}
            both = [(mine[q], ref_col[q]) for q in mine if q in ref_col]
            err = max(err, float(max(abs(l2[a] - l2_ref[r]) for a, r in both)))
            assert err <= LOSS_CAP, (key, i, e, err)
            j = int(picks[2 * e + 1][i][0])
            jr = ref_col.get((top[j // nv], j % nv))
            if jr is None:
                break                                              # the pair the reference never scores (its tie order differs)
            assert l2_ref[jr] >= l2_ref.max() - 4 * (err + 1e-6), (key, i, e)
            if row["stages"][2 * e + 1]["argmax"] != jr:
                break                                              # a near-tie flipped: the runs edit different sentences from here on
            if preds[e][i] != row["stages"][2 * e + 1]["pred"]:
                # same pick, another prediction: the two largest logits are within the error of each other, so is the loss of 0
                assert abs(float(l2_ref[jr])) <= err, (key, i, e, float(l2_ref[jr]), err)
                break
        else:
            assert adv[i] == row["adv"] and dists[i] == row["dist"], (key, i, adv[i], row["adv"], dists[i], row["dist"])
        worst = max(worst, err)
    return worst


@pytest.mark.parametrize("native", [True, False])
def test_tiny_model_replays_the_reference(torch_mod, fx, tiny, native):
    """LOSS_CAP = 4e-3 absolute on every compared loss.  Derivation: the project's per-row gate is 1e-3 rel-L2 (smoke(),
    test_row_error_census_gate); normalising a row at most doubles its error (2e-3 on a unit row); the loss is a difference of two
    inner products with unit rows, each off by at most the row's error: 4e-3.  With the error capped there, the margin rule cannot
    excuse a divergence where the reference's gap exceeds 4 * 4e-3 = 1.6e-2."""
    from leaf_amd.charmer import attack_text_charmer_classification_batched
    t, z = fx
    tok = _tok(native)
    worst = 0.0
    for key, case in t["cases"].items():
        S = [t["sentences"][r["sentence"]] for r in case["rows"]]
        labels = [r["label"] for r in case["rows"]]
        classes = torch_mod.from_numpy(z[f"{key}/classes"]).cuda()
        losses, picks, preds, trace = [], [], [], []
        adv, dists = attack_text_charmer_classification_batched(tiny, tok, S, classes, labels, n=case["n"], k=case["k"], V=t["V"],
                                                                return_losses=losses, return_picks=picks, return_preds=preds,
                                                                return_trace=trace)
        err = _check_case(t, z, key, adv, dists, losses, picks, preds, trace)
        same = sum(a == r["adv"] and d == r["dist"] for a, d, r in zip(adv, dists, case["rows"]))
        print(f"zero-shot replay {key} native={native}: max |loss error| {err:.3e} (cap {LOSS_CAP:g}), {same}/{len(S)} runs identical, "
              f"dists {dists}")
        worst = max(worst, err)
        if key == "mean3":
            for i in t["strings_for"]:
                st = case["rows"][i]["stages"]
                assert trace[0][i] == st[0]["candidates"][:-1]           # the reference's candidates minus its last
                if [int(p) for p in picks[0][i]] == st[0]["top"]:
                    assert trace[1][i] == st[1]["candidates"][:-1]
        if key == "wrong_label":
            assert dists[0] >= 1 and adv[0] != S[0]                      # already misclassified: it still receives its first edit
    assert worst <= LOSS_CAP


# ----------------------------------------------------------------------------- 4. drop-in and CLI
def test_drop_in_equals_the_batched_run(torch_mod, fx, tiny):
    from leaf_amd.charmer import attack_text_charmer_classification, attack_text_charmer_classification_batched
    t, z = fx
    tok = _tok(True)
    S = t["sentences"][:5] + [""]
    classes = torch_mod.from_numpy(z["mean3/classes"]).cuda()
    adv, dists = attack_text_charmer_classification_batched(tiny, tok, S, classes, [0] * len(S), n=5, k=3, V=t["V"])
    assert adv[-1] == "" and dists[-1] == 0
    for i, s in enumerate(S):
        one, d = attack_text_charmer_classification(tiny, tok, s, classes, 0, None, n=5, k=3, V=t["V"], batch_size=7)
        assert (one, d) == (adv[i], dists[i])


def _read(path):
    with open(path) as f:
        return list(csv.DictReader(f))


def test_eval_cli_end_to_end(torch_mod, fx, tmp_path, monkeypatch):
    import eval_zero_shot_text as cli
    t, z = fx
    monkeypatch.chdir(tmp_path)
    texts = t["sentences"][:7]
    (tmp_path / "news.tsv").write_text("".join(f"{i % 3}\t{s}\n" for i, s in enumerate(texts)))
    (tmp_path / "classes.txt").write_text("a photo of a cat\nthe stock market\npeople in a park\n")
    np.save(tmp_path / "feats.npy", 3.0 * z["mean3/classes"])                       # not unit rows: normalised on load
    common = ["--model", "tiny-test-quickgelu", "--seed", "12", "--data", str(tmp_path / "news.tsv"), "--rho", "5", "--k", "3"]
    for target, suffix in ((["--class-names", str(tmp_path / "classes.txt")], "_text_only"),
                           (["--class-features", str(tmp_path / "feats.npy")], "")):
        rows = cli.main(common + target + ["--batch-size", "3", "--out-dir", "batched"])
        path = tmp_path / "batched" / f"tiny-test-quickgelu_news_k3_rho_5{suffix}.csv"
        assert path.exists(), list((tmp_path / "batched").iterdir())
        got = _read(path)
        assert list(got[0]) == cli.COLUMNS and len(got) == len(rows) == len(texts)
        assert [r["sentence"] for r in got] == texts and [int(r["original_label"]) for r in got] == [i % 3 for i in range(len(texts))]
        assert all(1 <= r["dist"] <= 3 for r in rows)
        cli.main(common + target + ["--per-sentence", "--out-dir", "per"])
        assert _read(tmp_path / "per" / path.name) == got
        fast = cli.main(common + target + ["--fast-columns", "--out-dir", "fast"])
        # in the arithmetic the attack scores in, the reported adversarial label left the true one exactly where the attack saw a flip
        assert [r["adv_label"] != r["original_label"] for r in fast] == [r["attack_flipped"] for r in fast]
        assert [r["adv_sentence"] for r in fast] == [r["adv_sentence"] for r in rows]
