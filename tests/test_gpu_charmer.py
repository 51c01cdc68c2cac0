"""Batched Charmer / brute force on the MI355X (leaf_amd/charmer.py, leaf_amd/csrc/select.hip): the segmented selection kernel is
exact; the attacks reproduce the reference's own runs (tests/golden/charmer_trace.json) up to the margin rule of
tests/test_gpu_forward.py; batching, pipelining and column chunking change nothing; the CLI entry points run end to end."""
import csv
import json
import os

import numpy as np
import pytest

from oracle import text_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def fx(golden_dir):
    with open(os.path.join(golden_dir, "charmer_trace.json")) as f:
        t = json.load(f)
    return t, np.load(os.path.join(golden_dir, "charmer_trace.npz"))


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


# ----------------------------------------------------------------------------- 1. the selection kernel
def _ref_topk(row, cnt, n):
    """stable descending order, NaN first, ties -> lower column"""
    r = row[:cnt]
    nan = np.nonzero(np.isnan(r))[0]
    num = np.nonzero(~np.isnan(r))[0]
    order = np.concatenate([nan, num[np.argsort(-r[num], kind="stable")]])[:n]
    idx = np.full(n, -1, np.int32)
    val = np.full(n, -np.inf, np.float32)
    idx[:len(order)] = order
    val[:len(order)] = r[order]
    return idx, val


def _losses(rng, B, ld):
    x = rng.standard_normal((B, ld)).astype(np.float32)
    x[:, ::7] = np.round(x[:, ::7])                      # planted exact ties (many equal values per row)
    x[rng.random((B, ld)) < 0.01] = np.nan
    x[rng.random((B, ld)) < 0.01] = -np.inf
    x[rng.random((B, ld)) < 0.01] = -0.0
    if B > 1:
        x[1, :] = 0.5                                    # a row of one value
    return x


@pytest.mark.parametrize("ld", [1, 37, 961, 40000])
def test_select_topk_is_a_stable_sort(torch_mod, ld):
    from leaf_amd.charmer import select_topk
    rng = np.random.default_rng(ld)
    B = 9
    x = _losses(rng, B, ld)
    count = np.array([ld, 0, ld // 2, 1, ld, max(ld - 1, 0), 3, ld, ld], np.int32)[:B].clip(0, ld)
    count[1] = ld if ld > 1 else 0                        # the constant row: every column ties
    for n in (1, 5, 50):
        idx, val = select_topk(torch_mod.from_numpy(x).cuda(), count, n)
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        for b in range(B):
            ri, rv = _ref_topk(x[b], count[b], n)
            assert np.array_equal(idx[b], ri), (ld, n, b, idx[b][:8], ri[:8])
            assert np.array_equal(val[b].view(np.int32), rv.view(np.int32)), (ld, n, b)      # bit for bit (NaN, -0.0 included)


def test_select_topk_accumulate_over_column_chunks(torch_mod):
    from leaf_amd.charmer import new_accumulator, select_topk
    rng = np.random.default_rng(3)
    B, ld = 6, 3001
    x = _losses(rng, B, ld)
    x[2, np.isnan(x[2])] = 0.0                           # (rows 0, 1, 5 keep their NaNs: a NaN ranks above every number)
    x[2, 1000:1010] = 50.0                               # the same maximum in two chunks: the first one wins
    x[2, 2500] = 50.0
    x[3, :] = -np.inf
    count = np.array([ld, ld - 1, ld, ld, 0, 1700], np.int32)
    whole, _ = select_topk(torch_mod.from_numpy(x).cuda(), count, 1)
    acc = new_accumulator(B, "cuda:0")
    for c0 in (0, 1000, 2000):
        w = min(1000, ld - c0)
        part = np.ascontiguousarray(x[:, c0:c0 + w])
        select_topk(torch_mod.from_numpy(part).cuda(), np.clip(count - c0, 0, w), 1, col_offset=c0, accumulate=True, out=acc)
    got = acc[0].cpu().numpy()[:, 0]
    ref = np.array([_ref_topk(x[b], count[b], 1)[0][0] for b in range(B)])
    assert np.array_equal(got, ref) and np.array_equal(whole.cpu().numpy()[:, 0], ref)
    assert got[2] == 1000 and got[3] == 0 and got[4] == -1


# ----------------------------------------------------------------------------- 2./4. tiny model vs the reference's runs
def _check_against_reference(t, z, key, adv, losses, picks, V):
    """``adv`` / per-stage ``losses`` / ``picks`` of a batched run vs the reference's run of the same case.  Equal sentences are the
    rule; where they differ, the margin rule holds at the first divergent decision: a stage-1 top-n set may differ only where the
    reference's gap at the n-th place is within the measured loss error (exact ties: torch.topk orders them arbitrarily, the
    kernel by column), and a stage-2 pick must be as good as the reference's best within that error."""
    case = t["cases"][key]
    n, nv = case["n"], len(V)
    differ = 0
    for i, row in enumerate(case["rows"]):
        if adv[i] == row["adv"]:
            continue
        differ += 1
        for e in range(case["k"]):
            l1_ref, l2_ref = z[f"{key}/{i}/{2 * e}"], z[f"{key}/{i}/{2 * e + 1}"]
            l1 = losses[2 * e][i]
            assert l1.shape == l1_ref.shape                   # the reference never encodes its last candidate either
            err = float(np.abs(l1 - l1_ref).max()) + 1e-6
            top_ref = row["stages"][2 * e]["top"]
            top = [int(p) for p in picks[2 * e][i]]
            if set(top) != set(top_ref):
                srt = np.sort(l1_ref)[::-1]
                m = len(top_ref)
                assert m < len(srt) and srt[m - 1] - srt[m] <= 4 * err, (key, i, e, top, top_ref)
                break                                          # different stage-2 candidates from here on
            # same positions (maybe in another tie order): match the columns by (position, character)
            l2 = losses[2 * e + 1][i]
            ref_col = {(top_ref[j // nv], j % nv): j for j in range(len(l2_ref))}
            mine = {(top[j // nv], j % nv): j for j in range(len(l2))}
            both = [(mine[q], ref_col[q]) for q in mine if q in ref_col]
            err2 = max(err, float(max(abs(l2[a] - l2_ref[r]) for a, r in both)) + 1e-6)
            j = int(picks[2 * e + 1][i][0])
            jr = ref_col.get((top[j // nv], j % nv))
            if jr is None:
                break                                          # the pair the reference never scores (its tie order differs)
            assert l2_ref[jr] >= l2_ref.max() - 4 * err2, (key, i, e)
            if row["stages"][2 * e + 1]["argmax"] != jr:
                break                                          # a near-tie flipped: the runs edit different sentences from here on
    return differ


@pytest.mark.parametrize("key,native", [("k1_n5", True), ("k2_n10", True), ("k1_n5_c", True), ("k1_n5_c", False)])
def test_tiny_model_replays_the_reference(torch_mod, fx, tiny, key, native):
    from leaf_amd import attacks
    from leaf_amd.charmer import attack_text_charmer
    t, z = fx
    case = t["cases"][key]
    attacks.set_dictionary(attacks.Dictionary(t["stub_words"]))
    try:
        losses, picks, trace = [], [], []
        adv, dists = attack_text_charmer(tiny, _tok(native), t["sentences"], torch_mod.from_numpy(z["anchors"]).cuda(), "l2",
                                         case["n"], case["k"], t["V"], case["constrain"], return_losses=losses,
                                         return_picks=picks, return_trace=trace)
    finally:
        attacks.set_dictionary(None)
    assert dists == [case["k"]] * len(adv)
    _check_against_reference(t, z, key, adv, losses, picks, t["V"])
    # where the sentence and the top positions agree, the scored candidates are the reference's strings
    for i in t["strings_for"]:
        st = case["rows"][i]["stages"]
        assert trace[0][i] == st[0]["candidates"][:-1]
        if [int(p) for p in picks[0][i]] == st[0]["top"]:
            assert trace[1][i] == st[1]["candidates"][:-1]


def test_bruteforce_replays_the_reference(torch_mod, fx, tiny):
    from leaf_amd.charmer import attack_text_bruteforce, attack_text_bruteforce_batched
    t, z = fx
    br = t["brute"]
    losses = []
    adv, dists = attack_text_bruteforce_batched(tiny, _tok(True), br["sentences"], torch_mod.from_numpy(z["brute_anchors"]).cuda(),
                                                "l2", t["V"], return_losses=losses)
    assert dists == [1] * len(adv)
    for i, row in enumerate(br["rows"]):
        l_ref, l = z[f"brute/{i}"], losses[0][i]
        assert l.shape == l_ref.shape
        err = float(np.abs(l - l_ref).max()) + 1e-6
        j = int(np.argmax(l))
        if adv[i] != row["adv"]:
            assert l_ref[j] >= l_ref.max() - 4 * err, (i, adv[i], row["adv"])
        one, d = attack_text_bruteforce(tiny, _tok(False), br["sentences"][i], torch_mod.from_numpy(z["brute_anchors"][i]).cuda(), None,
                                        objective="l2", V=t["V"])
        assert one == adv[i] and d == 1


# ----------------------------------------------------------------------------- 3. batching changes nothing
def test_batching_pipelining_and_chunking_change_nothing(torch_mod, fx, tiny):
    from leaf_amd.charmer import attack_text_bruteforce_batched, attack_text_charmer, attack_text_charmer_inference
    t, z = fx
    tok = _tok(True)
    S = t["sentences"]
    A = z["anchors"]
    l8, p8 = [], []
    adv8, _ = attack_text_charmer(tiny, tok, S, torch_mod.from_numpy(A).cuda(), "l2", 10, 2, t["V"], return_losses=l8)
    for pipeline, max_rows in ((2, 65536), (3, 700)):
        lp = []
        advp, _ = attack_text_charmer(tiny, tok, S, torch_mod.from_numpy(A).cuda(), "l2", 10, 2, t["V"], pipeline=pipeline,
                                      max_rows=max_rows, return_losses=lp)
        assert advp == adv8
        assert all(np.array_equal(a, b) for st8, stp in zip(l8, lp) for a, b in zip(st8, stp))
    for i, s in enumerate(S):
        l1 = []
        adv1, _ = attack_text_charmer(tiny, tok, [s], torch_mod.from_numpy(A[i:i + 1]).cuda(), "l2", 10, 2, t["V"], return_losses=l1)
        assert adv1[0] == adv8[i]
        for st in range(4):
            assert np.array_equal(l1[st][0], l8[st][i]), (i, st)
        one, d = attack_text_charmer_inference(tiny, tok, s, torch_mod.from_numpy(A[i]).cuda(), None, n=10, k=2, V=t["V"],
                                               batch_size=7)
        assert one == adv8[i] and d == 2
    # brute force: column windows of 257 (accumulate) vs one window, a ragged batch vs one caption at a time
    bs = ["a cat", "Hi.", "the red car", "x"]
    ab = torch_mod.from_numpy(np.concatenate([z["brute_anchors"], A[:1]])).cuda()
    lw, lc = [], []
    whole, _ = attack_text_bruteforce_batched(tiny, tok, bs, ab.clone(), "l2", t["V"], return_losses=lw)
    chunked, _ = attack_text_bruteforce_batched(tiny, tok, bs, ab.clone(), "l2", t["V"], chunk_cols=257, max_rows=600, return_losses=lc)
    assert whole == chunked
    assert all(np.array_equal(a, b) for a, b in zip(lw[0], lc[0]))
    for i, s in enumerate(bs):
        one, _ = attack_text_bruteforce_batched(tiny, tok, [s], ab[i:i + 1].clone(), "l2", t["V"], chunk_cols=300)
        assert one[0] == whole[i]


def test_objectives_and_empty_caption(torch_mod, fx, tiny):
    from leaf_amd.charmer import attack_text_charmer
    t, z = fx
    S = ["", "a photo of a cat", "Hi."]
    A = np.concatenate([z["anchors"][:1], z["anchors"][:2]])
    for obj in ("l2", "negl2", "sim", "dissim"):
        a = torch_mod.from_numpy(A.copy()).cuda()
        adv, dists = attack_text_charmer(tiny, _tok(True), S, a, obj, 5, 1, t["V"])
        assert adv[0] == "" and dists == [1, 1, 1] and all(isinstance(s, str) for s in adv)
        if obj in ("sim", "dissim"):
            assert np.allclose(a.norm(dim=-1).cpu().numpy(), 1.0, atol=1e-6)            # normalised in place, as the reference does
        with pytest.raises(NotImplementedError):
            from leaf_amd.charmer import attack_text_charmer_inference
            attack_text_charmer_inference(tiny, _tok(True), "a cat", a[1], None, model_2=object())


# ----------------------------------------------------------------------------- 5. ViT-L at full shape
def test_vitl_full_shape_margin_rule(torch_mod):
    from leaf_amd.charmer import attack_text_charmer
    from leaf_amd.model import create_model
    cfg = O.TextCfg(768, 12, 12, 768)
    w = O.init_weights(cfg, seed=1)
    m = create_model("ViT-L-14", device="cuda:0", seed=1)
    tok = _tok(True)
    S = ["A man rides a red bicycle down a busy city street.", "Two dogs play with a ball on the beach",
         "Stocks rally as oil prices fall", "a bowl of soup, bread and a glass of wine"]
    anchor = m.encode_text(tok.encode_batch(S))
    losses, picks, trace = [], [], []
    adv, _ = attack_text_charmer(m, tok, S, anchor.clone(), "l2", 10, 1, return_losses=losses, return_picks=picks, return_trace=trace)
    A = anchor.cpu().numpy()

    def oracle_loss(strings, b):
        ids = tok.encode_batch(strings)
        uniq, inv = np.unique(ids, axis=0, return_inverse=True)
        L = int(uniq.argmax(-1).max()) + 1                      # causal: positions after the longest EOT change nothing pooled
        f = np.concatenate([O.encode_text(w, cfg, uniq[s:s + 256, :L]) for s in range(0, len(uniq), 256)])
        return ((f - A[b]) ** 2).sum(-1)[inv.reshape(-1)]

    for b in range(len(S)):
        o1 = oracle_loss(trace[0][b], b)
        err = float(np.abs(losses[0][b] - o1).max()) + 1e-6
        srt = np.sort(o1)[::-1]
        top = [int(p) for p in picks[0][b]]
        ref_top = set(np.argsort(-o1, kind="stable")[:10].tolist())
        if srt[9] - srt[10] > 4 * err:
            assert set(top) == ref_top, (b, top, sorted(ref_top))
        assert o1[top].min() >= srt[9] - 4 * err
        o2 = oracle_loss(trace[1][b], b)
        err2 = float(np.abs(losses[1][b] - o2).max()) + 1e-6
        j = int(picks[1][b][0])
        assert o2[j] >= o2.max() - 4 * err2, (b, o2[j], o2.max(), err2)
        assert adv[b] == trace[1][b][j]


# ----------------------------------------------------------------------------- 6. CLI end to end
def _read(path):
    with open(path) as f:
        return list(csv.DictReader(f))


@pytest.mark.parametrize("attack", ["charmer", "bruteforce"])
def test_eval_cli_charmer_and_bruteforce(torch_mod, tmp_path, monkeypatch, attack):
    import eval_textfare
    monkeypatch.chdir(tmp_path)
    caps = "a photo of a cat\nHi.\nthe red car\nx\n" if attack == "bruteforce" else \
        "a photo of a cat\nthe red car on the street\ntwo people in the park\nx\nStocks rally as oil prices fall\n"
    (tmp_path / "caps.txt").write_text(caps)
    common = ["--model", "tiny-test-quickgelu", "--robust-seed", "13", "--texts", str(tmp_path / "caps.txt"), "--rho", "5", "--k", "1",
              "--attack-name", attack]
    rows = eval_textfare.main(common + ["--batch-size", "3", "--out-dir", "batched"])
    path = tmp_path / "batched" / f"tiny-test-quickgelu_caps_{attack}_k1_rho_5.csv"
    assert path.exists(), list((tmp_path / "batched").iterdir())
    got = _read(path)
    assert list(got[0]) == ["sentence", "adv_sentence", "textfare_clean", "textfare_adv"] and len(got) == len(rows)
    assert all(float(r["textfare_adv"]) >= 0 for r in got)
    per = eval_textfare.main(common[:-2] + ["--attack_name", attack, "--per-sentence", "--out-dir", "per"])
    assert [(r["sentence"], r["adv_sentence"]) for r in per] == [(r["sentence"], r["adv_sentence"]) for r in rows]
    assert np.allclose([r["textfare_adv"] for r in per], [r["textfare_adv"] for r in rows], rtol=1e-6, atol=1e-9)


def test_train_cli_use_charmer(torch_mod, tmp_path, monkeypatch):
    import train_AT_text_only as cli
    from leaf_amd.charmer import attack_text_charmer
    from leaf_amd.model import create_model
    from leaf_amd.tokenizer import get_tokenizer
    monkeypatch.chdir(tmp_path)
    dump = tmp_path / "dump"
    dump.mkdir()
    monkeypatch.setenv("LEAF_DEBUG_DUMP_ADV", str(dump))
    args = ["--model", "tiny-test-quickgelu", "--dataset-type", "synthetic", "--train-num-samples", "16", "--batch-size", "8",
            "--lr", "1e-4", "--wd", "1e-4", "--warmup", "2", "--rho", "5", "--k_adv", "1", "--seed", "3", "--epochs", "1",
            "--custom_out_folder", "c_", "--logs", str(tmp_path / "logs"), "--name", "runc", "--use_charmer"]
    assert cli.main(args) == 0
    times = (tmp_path / "times_True.csv").read_text().split()
    assert times[0] == "0" and len(times) == 3 and all(float(x) > 0 for x in times[1:])
    out = tmp_path / "results" / "c_text_only_k1_rho5_seed3"
    rows = open(out / "results.csv").read().strip().splitlines()
    hdr, vals = rows[0].split(","), rows[1].split(",")
    assert np.isfinite(float(vals[hdr.index("loss")]))
    # the first batch's adversarial texts are Charmer's on that batch against the frozen (initial) model's anchors
    pairs = [l.split("\t") for l in (dump / "adv_epoch0_rank0.txt").read_text().splitlines()]
    texts, adv = [p[0] for p in pairs], [p[1] for p in pairs]
    m = create_model("tiny-test-quickgelu", device="cuda:0", seed=3)        # the trainer's random init: --seed
    tok = get_tokenizer("tiny-test-quickgelu")
    anchor = m.encode_text(tok.encode_batch(texts))
    again, _ = attack_text_charmer(m, tok, texts, anchor, "l2", 5, 1)
    assert again == adv

