"""Host side of text embedding inversion (leaf_amd/inversion.py, invert_text.py) and the reference fixture tests/golden/tiny_pez.npz
(tests/golden/make_golden_pez.py), without a GPU."""
import json
import os

import numpy as np
import pytest

from oracle import text_oracle as O


def margin_bound(d):              # tests/test_gpu_nnproj.py, "MARGIN RULE"
    return 2.0 * d * 2.0 ** -23


@pytest.fixture(scope="module")
def pez(golden_dir):
    z = np.load(os.path.join(golden_dir, "tiny_pez.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return z, meta


def test_token_accuracy_follows_the_reference_convention():
    from leaf_amd.inversion import token_accuracy
    ref = [49406, 320, 1125, 539, 2368, 49407] + [0] * 71           # a full token row: SOT, 4 ids, EOT, padding
    assert token_accuracy([[320, 1125, 539, 2368]], [ref]) == 1.0
    assert token_accuracy([[2368, 320, 7, 7]], [ref]) == 0.5        # order does not matter, membership does
    assert token_accuracy([[7, 7, 7, 7]], [ref]) == 0.0
    # zeros are dropped from the reconstruction too; SOT / EOT of the reference never count
    assert token_accuracy([[320, 1125, 539, 2368, 0, 0]], [ref]) == 1.0
    assert token_accuracy([[49406, 49407, 7, 7]], [ref]) == 0.0
    # pooled over captions: (4 + 1) / (4 + 2)
    ref2 = [49406, 5, 6, 49407] + [0] * 73
    assert token_accuracy([[320, 1125, 539, 2368], [6, 9]], [ref, ref2]) == pytest.approx(5 / 6)
    with pytest.raises(ValueError):
        token_accuracy([[320, 1125]], [ref])                        # the reference asserts equal lengths


def test_word_accuracy_follows_the_reference_convention():
    from leaf_amd.inversion import word_accuracy
    assert word_accuracy(["a photo of a cat"], ["A Photo of a Cat"]) == 1.0
    assert word_accuracy(["cat cat dog"], ["a cat"]) == pytest.approx(1 / 3)       # reference words found / reconstruction length
    assert word_accuracy(["x y", "the red car"], ["a b", "the car"]) == pytest.approx(2 / 5)


def test_initial_ids_are_the_reference_draw(pez):
    from leaf_amd.inversion import initial_ids
    z, meta = pez
    for c in range(len(meta["captions"])):
        P = z[f"c{c}_ids"].shape[1]
        assert np.array_equal(initial_ids(P, meta["seed"]), z[f"c{c}_init_ids"])


def test_out_of_scope_modes_raise():
    from leaf_amd.inversion import invert_text
    for kw in (dict(prompt_bs=2), dict(target_images=[object()]), dict(avg_text=True)):
        with pytest.raises(NotImplementedError):
            invert_text(None, None, captions=["a cat"], **kw)
    with pytest.raises(ValueError):
        invert_text(None, None)


def test_cli_arguments_and_config(tmp_path):
    import invert_text as cli
    caps = tmp_path / "caps.txt"
    caps.write_text("a photo of a cat\n  two dogs \nthird\n")
    a = cli.parse_args(["--model", "tiny-test-quickgelu", "--captions", str(caps), "--n-samples", "2", "--iter", "7", "--batch", "3"])
    assert (a.n_samples, a.iter, a.batch, a.checkpoint) == (2, 7, 3, None)
    assert cli.read_captions(str(caps), a.n_samples) == ["a photo of a cat", "two dogs"]
    with pytest.raises(SystemExit):
        cli.parse_args(["--model", "ViT-L-14", "--captions", str(caps)])            # no checkpoint and no --random-init
    cli.parse_args(["--model", "ViT-L-14", "--captions", str(caps), "--random-init"])
    cfg = cli.load_config(None)
    assert cfg == cli.CONFIG_DEFAULTS and cfg["prompt_len"] == "match" and cfg["iter"] == 3000
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps({"seed": 3, "prompt_len": 8, "lr": 0.05, "weight_decay": 0.2, "loss_weight": 2.0, "print_step": 100}))
    cfg = cli.load_config(str(p), iters=11)
    assert (cfg["seed"], cfg["prompt_len"], cfg["lr"], cfg["weight_decay"], cfg["loss_weight"], cfg["print_step"], cfg["iter"]) == \
        (3, 8, 0.05, 0.2, 2.0, 100, 11)
    for bad in ({"prompt_bs": 4}, {"learning_rate": 1.0}, {"batch_size": 2}, {"iter": 0}):
        p.write_text(json.dumps(bad))
        with pytest.raises(SystemExit):
            cli.load_config(str(p))
    assert cli.result_path(a, cfg).endswith("results-2smpls-11iters-tiny-test-quickgelu.json")
    a.out = "x/y.json"
    assert cli.result_path(a, cfg) == "x/y.json"


def test_fixture_is_self_consistent(pez):
    """Every step's recorded ids are the float64 cosine arg-max of its recorded embeddings over the token table, outside the margin;
    the embeddings start at the table rows of the initial ids; the returned dict is the best step of the recorded cosines."""
    z, meta = pez
    cfg = O.TextCfg(128, 2, 2, 64, quick_gelu=True)
    table = O.init_weights(cfg, seed=12)["token_embedding.weight"].astype(np.float64)
    tn = table / np.linalg.norm(table, axis=1, keepdims=True)
    assert meta["iters"] == 30 and [z[f"c{c}_ids"].shape[1] for c in range(4)] == [1, 4, 9, 15]
    rows = inside = 0
    for c, res in enumerate(meta["results"]):
        emb, ids, cosv = z[f"c{c}_emb"], z[f"c{c}_ids"], z[f"c{c}_cos"]
        T, P = ids.shape
        assert emb.shape == (T + 1, P, 128) and z[f"c{c}_grad"].shape == (T, P, 128)
        assert np.array_equal(emb[0], table[z[f"c{c}_init_ids"]].astype(np.float32))
        q = emb[:T].reshape(T * P, 128).astype(np.float64)
        ref = (q / np.linalg.norm(q, axis=1, keepdims=True)) @ tn.T
        top2 = np.sort(np.partition(ref, -2, axis=1)[:, -2:], axis=1)
        clear = top2[:, 1] - top2[:, 0] > margin_bound(128)
        got = ref[np.arange(T * P), ids.reshape(-1)]
        assert np.array_equal(ids.reshape(-1)[clear], ref.argmax(1)[clear])
        assert np.all(top2[~clear, 1] - got[~clear] <= margin_bound(128))
        rows += T * P
        inside += int((~clear).sum())
        best = int(np.argmax(cosv))                      # the first strictly greatest cosine (optim_utils.py:214)
        assert res["ids_rec"] == ids[best].tolist() and abs(res["sim"] - cosv[best]) < 1e-6
        assert res["ids_orig"] == z[f"c{c}_tokens"].tolist() and res["original"] == meta["captions"][c]
    assert inside <= 0.02 * rows
    e = z["interior_eot_ids"]
    assert 49407 in e[:-1].tolist() and z["interior_eot_grad"].shape == (len(e), 128) and z["interior_eot_feat"].shape == (64,)
