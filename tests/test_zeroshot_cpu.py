"""Host side of the batched classification Charmer (leaf_amd/charmer.py, attack_text_charmer_classification_batched) and of
eval_zero_shot_text.py: the active set / early-stop bookkeeping against a fake scorer and a one-sentence restatement of the
reference's loop (utils_attacks.py:582-643), the margin loss restated in numpy against the reference's stored loss rows
(tests/golden/zeroshot_trace.*, tests/golden/make_golden_zeroshot.py), CLI argument handling and the construction of V.  CPU only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from leaf_amd import charmer
from leaf_amd.attacks import _apply_edit
from leaf_amd.tokenizer import SimpleTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = [-1] + [ord(ch) for ch in "abz XY9!"]
SENTENCES = ["a cat", "", "Hi.", "two dogs", "x", "the red car", "stocks fall", "ab"]


@pytest.fixture(scope="module")
def fx(golden_dir):
    with open(os.path.join(golden_dir, "zeroshot_trace.json")) as f:
        t = json.load(f)
    return t, np.load(os.path.join(golden_dir, "zeroshot_trace.npz"))


# ----------------------------------------------------------------------------- a fake score: a fixed function of the token row
def _fake(ids):
    """(loss, pred) per token row: a hash of the ids, so every run scores a given string the same way"""
    ids = np.asarray(ids, dtype=np.int64)
    h = (ids * (np.arange(ids.shape[-1]) + 1)).sum(-1)
    loss = ((h * 2654435761) % 10007).astype(np.float32) / np.float32(10007)
    pred = np.where(h % 4 == 0, 1, 0).astype(np.int32)          # the label is 0: about one pick in four flips
    return loss, pred


class FakeScorer:
    reuse = False

    def __init__(self):
        self.calls = []

    def kv(self, base, slot):
        return None

    def loss(self, toks, lens, base, kv, labels_g, R, count):
        import torch
        self.calls.append(len(labels_g))
        loss, pred = _fake(toks.reshape(len(labels_g), R, -1))
        return torch.from_numpy(loss), torch.from_numpy(pred)


def _cpu_select_topk(loss, count, n, col_offset=0, accumulate=False, out=None):
    """leaf_select_topk restated: NaN first, larger value, lower column; unused slots -1 / -inf"""
    import torch
    x = loss.numpy()
    idx = np.full((x.shape[0], n), -1, np.int32)
    val = np.full((x.shape[0], n), -np.inf, np.float32)
    for b in range(x.shape[0]):
        r = x[b, :count[b]]
        nan, num = np.nonzero(np.isnan(r))[0], np.nonzero(~np.isnan(r))[0]
        order = np.concatenate([nan, num[np.argsort(-r[num], kind="stable")]])[:n]
        idx[b, :len(order)], val[b, :len(order)] = order, r[order]
    return torch.from_numpy(idx), torch.from_numpy(val)


@pytest.fixture
def cpu_charmer(monkeypatch):
    monkeypatch.setattr(charmer, "select_topk", _cpu_select_topk)
    monkeypatch.setattr(charmer, "_to_host", lambda t: (lambda: t.numpy()))


def _reference_loop(tok, sentence, label, n, k):
    """utils_attacks.py:582-643 for one sentence with the fake score (first maximum wins, as the selection kernel)"""
    dist, trail = 0, []
    for dist in range(k):
        SS = [_apply_edit(sentence, z, ord(" ")) for z in range(2 * len(sentence) + 1)][:-1]      # the last one is never scored
        loss, _ = _fake(tok.encode_batch(SS))
        top = np.argsort(-loss, kind="stable")[:min(n, len(SS))]
        SS = [_apply_edit(sentence, int(z), c) for z in top for c in V][:-1]
        loss, pred = _fake(tok.encode_batch(SS))
        j = int(np.argmax(loss))
        sentence = SS[j]
        trail.append(int(pred[j]))
        if pred[j] != label:
            break
    return sentence, dist + 1, trail


def test_early_stop_active_set_and_groupings(cpu_charmer):
    tok = SimpleTokenizer()
    n, k = 3, 4
    labels = [0] * len(SENTENCES)
    ref = [(_reference_loop(tok, s, 0, n, k) if s else (s, 0, [])) for s in SENTENCES]
    want_dists = [r[1] for r in ref]
    assert max(want_dists) == k and min(d for d in want_dists if d) < k and len(set(want_dists)) >= 3      # the cases are all there
    runs = []
    for pipeline, max_rows in ((1, 65536), (3, 65536), (2, 40)):
        sc, preds, losses = FakeScorer(), [], []
        adv, dists = charmer.attack_text_charmer_classification_batched(None, tok, SENTENCES, None, labels, n=n, k=k, V=V, pipeline=pipeline,
                                                                        max_rows=max_rows, return_preds=preds, return_losses=losses,
                                                                        scorer=sc)
        assert adv == [r[0] for r in ref] and dists == want_dists
        assert adv[1] == "" and dists[1] == 0                                     # the empty caption: unchanged, no edit
        # a caption that has stopped is never scored again: edit e scores the captions with dist > e, in both stages
        assert sum(sc.calls) == 2 * sum(want_dists)
        assert len(preds) == max(want_dists)
        for e, p in enumerate(preds):
            for b, r in enumerate(ref):
                assert p[b] == (r[2][e] if e < len(r[2]) else None), (e, b)
        runs.append(losses)
    # grouping changes no loss bit
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        assert all(np.array_equal(x, y) for s0, s1 in zip(runs[0], other) for x, y in zip(s0, s1))


def test_one_sentence_calls_equal_the_batch_and_label_mismatch_still_edits(cpu_charmer):
    tok = SimpleTokenizer()
    adv, dists = charmer.attack_text_charmer_classification_batched(None, tok, SENTENCES, None, [0] * len(SENTENCES), n=3, k=4, V=V,
                                                                    scorer=FakeScorer())
    for b, s in enumerate(SENTENCES):
        one, d = charmer.attack_text_charmer_classification_batched(None, tok, [s], None, [0], n=3, k=4, V=V, scorer=FakeScorer())
        assert (one[0], d[0]) == (adv[b], dists[b])
    # a label the clean caption is not classified as (the fake never predicts 2): one edit, then it stops
    one, d = charmer.attack_text_charmer_classification_batched(None, tok, ["a cat"], None, [2], n=3, k=4, V=V, scorer=FakeScorer())
    assert d == [1] and one[0] != "a cat"
    with pytest.raises(ValueError):
        charmer.attack_text_charmer_classification_batched(None, tok, ["a", "b"], None, [0], scorer=FakeScorer())


def test_stage_counts_of_the_reference_runs(fx):
    """the reference's tokenizer sees every candidate, its encoder all but the last: count = n_candidates - 1 in both stages, of
    every edit of every case; a run ends on a flipped prediction or after k edits"""
    t, z = fx
    nv = len(t["V"])
    for key, case in t["cases"].items():
        for row in case["rows"]:
            S = t["sentences"][row["sentence"]]
            st = row["stages"]
            assert len(st) == 2 * row["dist"] and 1 <= row["dist"] <= case["k"]
            _, _, count = charmer.stage1_plan([S])
            assert count[0] == st[0]["n_candidates"] - 1 == z[f"{key}/{row['sentence']}/0"].shape[0]
            for e in range(row["dist"]):
                m = len(st[2 * e]["top"])
                _, _, count = charmer.stage2_plan(np.array([st[2 * e]["top"]]), np.array([m]), t["V"])
                assert count[0] == st[2 * e + 1]["n_candidates"] - 1 == m * nv - 1 == z[f"{key}/{row['sentence']}/{2 * e + 1}"].shape[0]
                flipped = st[2 * e + 1]["pred"] != row["label"]
                assert flipped == (e == row["dist"] - 1) or (e == case["k"] - 1 and not flipped)
    d = [r["dist"] for r in t["cases"]["mean3"]["rows"]]
    assert sum(x >= 2 for x in d) >= 3 and t["cases"]["mean3"]["k"] in d and 1 in d


def test_candidate_strings_of_the_reference_runs(fx):
    t, _ = fx
    case = t["cases"]["mean3"]
    for i in t["strings_for"]:
        row = case["rows"][i]
        S = t["sentences"][i]
        for e in range(row["dist"]):
            s1, s2 = row["stages"][2 * e], row["stages"][2 * e + 1]
            z, c, count = charmer.stage1_plan([S])
            assert charmer.render_plan([S], z, c, count)[0] == s1["candidates"][:-1]
            z, c, count = charmer.stage2_plan(np.array([s1["top"]]), np.array([len(s1["top"])]), t["V"])
            assert charmer.render_plan([S], z, c, count)[0] == s2["candidates"][:-1]
            S = s2["candidates"][s2["argmax"]]
        assert S == row["adv"]


def _margin_loss(feat, classes, label):
    """margin_loss_lm (utils_attacks.py:145-151) in numpy: max over the other classes - the label's logit"""
    logits = feat.astype(np.float32) @ classes.astype(np.float32).T
    others = np.delete(logits, label, axis=1)
    return others.max(-1) - logits[:, label], logits.argmax(-1)


def test_numpy_margin_loss_reproduces_the_stored_rows(fx):
    t, z = fx
    i = t["features_for"]
    row = t["cases"]["mean3"]["rows"][i]
    classes = z["mean3/classes"]
    assert np.allclose(np.linalg.norm(classes, axis=-1), 1.0, atol=1e-6)
    for st in (0, 1):
        feat = z[f"mean3/{i}/{st}/feat"]
        loss, pred = _margin_loss(feat, classes, row["label"])
        ref = z[f"mean3/{i}/{st}"]
        assert loss.shape == ref.shape
        # two 64-term fp32 inner products of unit vectors in another summation order: 2 * 64 * 2^-24 at the very most
        assert np.abs(loss - ref).max() <= 2 * 64 * 2.0 ** -24
    assert int(np.argmax(ref)) == row["stages"][1]["argmax"] and int(pred[np.argmax(ref)]) == row["stages"][1]["pred"]


# ----------------------------------------------------------------------------- CLI
def test_cli_arguments_vocab_and_paths(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "eval_zero_shot_text.py"), "--help"], capture_output=True, text=True,
                         cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    for flag in ("--data", "--class-names", "--class-features", "--vocab-from", "--k", "--rho", "--n-test", "--batch-size",
                 "--per-sentence", "--fast-columns", "--out-dir", "--checkpoint", "--random-init", "--seed"):
        assert flag in out.stdout, flag
    sys.path.insert(0, ROOT)
    import eval_zero_shot_text as cli
    data = tmp_path / "news.tsv"
    data.write_text("2\tStocks fall, oil up!\n\n0\tb a\n1\t  \n3\tZ9\ttab\n", encoding="utf-8")
    rows = cli.read_data(str(data))
    assert rows == [(2, "Stocks fall, oil up!"), (0, "b a"), (3, "Z9\ttab")]                  # empty texts skipped, later tabs kept
    assert cli.read_data(str(data), 2) == rows[:2]
    v = cli.build_vocab(str(data))
    assert v[0] == -1 and v[1:] == sorted(set(v[1:])) and all(isinstance(x, int) for x in v)
    assert set(v[1:]) == {ord(ch) for ch in "Stocks fall, oil up!b aZ9\ttab "}                # the labels' digits are not text
    assert ord("2") not in v and ord("0") not in v and ord("\n") not in v
    plain = tmp_path / "train.txt"
    plain.write_text("ba\nc 1\n", encoding="utf-8")
    assert cli.build_vocab(str(plain)) == [-1] + sorted(map(ord, "bac 1"))
    bad = tmp_path / "bad.tsv"
    bad.write_text("sports\ttext\n")
    with pytest.raises(SystemExit):
        cli.read_data(str(bad))
    base = ["--data", str(data), "--model", "tiny-test-quickgelu"]
    for extra in ([], ["--class-names", "a", "--class-features", "b"], ["--class-names", "a", "--rho", "0"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + extra)
    with pytest.raises(SystemExit):
        cli.parse_args(["--data", str(data), "--class-names", "a"])                          # ViT-L default without a checkpoint
    a = cli.parse_args(["--data", "/d/agnews_test.tsv", "--class-names", "c.txt", "--checkpoint", "/ck/run/epoch_latest.pt", "--k", "2",
                        "--rho", "20"])
    assert cli.result_path(a) == os.path.join("results_zero_shot_text", "epoch_latest_agnews_test_k2_rho_20_text_only.csv")
    a = cli.parse_args(base + ["--class-features", "f.npy", "--out-dir", "o"])
    assert cli.result_path(a) == os.path.join("o", "tiny-test-quickgelu_news_k1_rho_20.csv")
    assert cli.COLUMNS == ["sentence", "original_label", "predicted_label", "adv_sentence", "adv_label"]
