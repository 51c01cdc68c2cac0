"""Host side of the batched Charmer / brute-force attacks (leaf_amd/charmer.py) against the reference's own candidate lists
(tests/golden/charmer_trace.json, tests/golden/make_golden_charmer.py): the padded stage plans (z, c, count), rendered through
``_apply_edit``, give the scored candidates string for string -- the dropped last candidate of every stage, 2 L < n, the padding of a
ragged batch and the --constrain replacement included.  CPU only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from leaf_amd import attacks, charmer
from leaf_amd.tokenizer import SimpleTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def trace(golden_dir):
    with open(os.path.join(golden_dir, "charmer_trace.json")) as f:
        return json.load(f)


def _tokenizers():
    toks = [SimpleTokenizer()]
    try:
        from leaf_amd.native_text import NativeTokenizer
        toks.append(NativeTokenizer(n_threads=4))
    except Exception:        # the native host library is built by __graft_entry__.build(); the Python tokenizer covers the rule
        pass
    return toks


def _edits(trace, key, i):
    """per edit: (sentence attacked, stage-1 entry, stage-2 entry) of fixture sentence i, for the sentences with strings"""
    st = trace["cases"][key]["rows"][i]["stages"]
    S = trace["sentences"][i]
    out = []
    for e in range(len(st) // 2):
        out.append((S, st[2 * e], st[2 * e + 1]))
        S = st[2 * e + 1]["candidates"][st[2 * e + 1]["argmax"]]
    return out


@pytest.mark.parametrize("key", ["k1_n5", "k2_n10", "k1_n5_c"])
def test_stage_plans_render_the_reference_candidates(trace, key):
    case = trace["cases"][key]
    V, n = trace["V"], case["n"]
    attacks.set_dictionary(attacks.Dictionary(trace["stub_words"]))
    try:
        for tok in _tokenizers():
            for i in trace["strings_for"]:
                for S, s1, s2 in _edits(trace, key, i):
                    # a ragged batch: the sentence next to a longer one, so its row is padded
                    batch = [S, S + " and a much longer neighbour caption"]
                    z, c, count = charmer.stage1_plan(batch)
                    assert count[0] == 2 * len(S) == s1["n_candidates"] - 1          # the last position is never scored
                    assert z.shape[1] == count.max() and (c[0, count[0]:] == -1).all()
                    charmer.prepare_stage(tok, batch, z, c, case["constrain"])
                    assert charmer.render_plan(batch, z, c, count)[0] == s1["candidates"][:-1]
                    top = np.array([s1["top"], s1["top"][:1] * len(s1["top"])])
                    m = np.array([len(s1["top"]), 1])
                    assert m[0] == min(n, 2 * len(S))                                  # 2 L < n: every position is kept
                    z, c, count = charmer.stage2_plan(top, m, V)
                    assert count[0] == s2["n_candidates"] - 1 and count[1] == len(V) - 1
                    charmer.prepare_stage(tok, batch, z, c, case["constrain"])
                    assert charmer.render_plan(batch, z, c, count)[0] == s2["candidates"][:-1]
    finally:
        attacks.set_dictionary(None)


def test_stage_counts_of_every_sentence(trace):
    V = trace["V"]
    for key, case in trace["cases"].items():
        for S, row in zip(trace["sentences"], case["rows"]):
            s1, s2 = row["stages"][0], row["stages"][1]
            _, _, count = charmer.stage1_plan([S])
            assert count[0] == s1["n_candidates"] - 1
            _, _, count = charmer.stage2_plan(np.array([s1["top"]]), np.array([len(s1["top"])]), V)
            assert count[0] == s2["n_candidates"] - 1 == len(s1["top"]) * len(V) - 1
            assert row["dist"] == case["k"]


def test_bruteforce_plan_and_column_windows(trace):
    V = trace["V"]
    br = trace["brute"]
    for S, row in zip(br["sentences"], br["rows"]):
        z, c, count = charmer.bruteforce_plan([S], V)
        assert count[0] == row["n_scored"] == (2 * len(S) + 1) * len(V) - 1
        whole = charmer.render_plan([S], z, c, count)[0]
        if row["candidates"] is not None:
            assert whole == row["candidates"]
        # windows of 257 columns over a ragged batch concatenate to the whole list
        batch = [S, "x"]
        got = []
        for c0 in range(0, count[0], 257):
            zw, cw, cnt = charmer.bruteforce_plan(batch, V, c0, 257)
            got += charmer.render_plan(batch, zw, cw, cnt)[0]
        assert got == whole


def test_empty_and_padding_rows_are_no_ops():
    z, c, count = charmer.stage1_plan(["", "ab"])
    assert list(count) == [0, 4]
    assert charmer.render_plan(["", "ab"], z, c, np.array([z.shape[1]] * 2))[0] == [""] * z.shape[1]


def test_eval_cli_attack_name_and_default_output_path(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "eval_textfare.py"), "--help"], capture_output=True, text=True,
                         cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "--attack-name" in out.stdout and "charmer" in out.stdout and "bruteforce" in out.stdout
    sys.path.insert(0, ROOT)
    import argparse
    import eval_textfare
    base = dict(model="ViT-L-14-quickgelu", clean="/ck/clean.bin", robust="/ck/run/epoch_latest.pt", texts="/d/captions.txt", k=1,
                rho=50, constrain=False, out_dir="results_textfare")
    a = argparse.Namespace(attack_name="leaf", **base)
    assert eval_textfare.result_path(a) == os.path.join("results_textfare", "epoch_latest_captions_leaf_k1_rho_50.csv")
    a = argparse.Namespace(attack_name="charmer", **dict(base, constrain=True, rho=5))
    assert eval_textfare.result_path(a) == os.path.join("results_textfare", "epoch_latest_captions_charmer_k1_rho_5_constrained.csv")
