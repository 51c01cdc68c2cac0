#!/usr/bin/env python3
"""Fixture for the batched classification Charmer (leaf_amd/charmer.py, attack_text_charmer_classification_batched): the
reference's own ``attack_text_charmer_classification`` (utils_attacks.py:582-643), one sentence per call, on the tiny quickgelu
model of weight seed 12 (the model of charmer_trace.json), CPU, fp32.

Runs only where make_golden.py runs (it needs the reference checkout; the stub recipe of make_golden.py, the spies of
make_golden_charmer.py).
Here the tokenizer sees the WHOLE candidate list of a stage and ``encode_text`` all of it but the last (:600, :622).  The stage
losses are recomputed from the spied features with the reference's own ``margin_loss_lm``, the top-n positions with its own
``torch.topk`` call, the predictions with its softmax / argmax.  Stored (inputs and outputs only):

* zeroshot_trace.json: sentences, V, per case the labels, k, n and per sentence the adversarial sentence, dist and per stage the
  number of candidates, the top-n positions / the arg-max and the prediction at it; the full candidate strings of the
  ``strings_for`` sentences of the first case
* zeroshot_trace.npz: the class matrix per case ("<case>/classes"), the stage losses ("<case>/<sentence>/<stage>") and, for one
  short sentence, the spied features of its first edit ("<case>/<sentence>/<stage>/feat")

With class features from encoded class captions, or random ones, the tiny random model flips on the first edit every time; the
first case therefore takes the normalised mean of the clean sentence features as class 0 (and two random unit rows), which the
attack needs several edits to leave.  The generator asserts that the reference's runs exercise the multi-edit loop.

    python tests/golden/make_golden_zeroshot.py
"""
import json
import os
import sys

import numpy as np
import torch
import transformers  # noqa: F401  (before torchvision is stubbed)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REPO, STUB_WORDS, TINY, V_DEFAULT, install_stubs, load_np_state  # noqa: E402
from make_golden_charmer import SENTENCES as CHARMER_SENTENCES  # noqa: E402

SENTENCES = CHARMER_SENTENCES + ["a bowl of soup, bread and a glass of wine on the table",
                                 "Two dogs play with a ball on the beach while a man watches them"]
STRINGS_FOR = (1, 3)                 # full candidate strings for these sentences, first case only
FEATURES_FOR = 6                     # "x": the spied features of its first edit (2 + 191 rows)
CLASS_CAPTIONS = ["a photo of a cat", "the stock market", "people in a park", "a red car"]
K, N = 4, 5


def main():
    install_stubs()
    import open_clip
    from open_clip.model import CLIP
    import utils_attacks
    sys.path.insert(0, REPO)
    from oracle import text_oracle as O

    torch.set_num_threads(8)
    tokenizer = open_clip.get_tokenizer("ViT-L-14")
    cfg = O.TextCfg(128, 2, 2, 64, quick_gelu=True)
    model = CLIP(**TINY, quick_gelu=True).float().eval()
    load_np_state(model, O.init_weights(cfg, seed=12))
    cands, feats = [], []

    class SpyTok:
        def __call__(self, texts, context_length=None):
            cands.append(list(texts) if not isinstance(texts, str) else [texts])
            return tokenizer(texts, context_length)

    encode = model.encode_text

    def spy_encode(tokens, normalize=False):
        f = encode(tokens, normalize=normalize)
        feats.append(f.detach().clone())
        return f
    model.encode_text = spy_encode

    with torch.no_grad():
        clean = encode(tokenizer(SENTENCES), normalize=True).detach()
        text4 = encode(tokenizer(CLASS_CAPTIONS), normalize=True).detach()
    g = torch.Generator().manual_seed(8)      # a seed under which the reference's dists cover 1, 2, 3 and k (asserted below)
    rnd = torch.randn(2, clean.shape[1], generator=g)
    mean3 = torch.cat([clean.mean(0, keepdim=True), rnd], 0)
    mean3 = mean3 / mean3.norm(dim=-1, keepdim=True)
    pred3 = (clean @ mean3.T).argmax(-1).tolist()
    pred4 = (clean @ text4.T).argmax(-1).tolist()
    assert pred3 == [0] * len(SENTENCES), pred3
    # (case, class matrix, sentence indices, labels)
    cases = [("mean3", mean3, list(range(len(SENTENCES))), [0] * len(SENTENCES)),
             ("wrong_label", mean3, [0], [1]),                  # the label is not the clean prediction: one edit all the same
             ("text4", text4, list(range(len(SENTENCES))), pred4)]

    out = {"sentences": SENTENCES, "stub_words": STUB_WORDS, "V": V_DEFAULT, "model": "tiny-test-quickgelu", "weight_seed": 12,
           "strings_for": list(STRINGS_FOR), "features_for": FEATURES_FOR, "class_captions": CLASS_CAPTIONS, "cases": {}}
    arrays = {}
    for key, classes, which, labels in cases:
        rows = []
        for i, label in zip(which, labels):
            del cands[:], feats[:]
            with torch.no_grad():
                adv, dist = utils_attacks.attack_text_charmer_classification(model, SpyTok(), SENTENCES[i], classes.clone(), label, "cpu",
                                                                             n=N, k=K, V=V_DEFAULT)
            assert len(cands) == 2 * dist and len(feats) == 2 * dist, (key, i, dist, len(cands), len(feats))
            stages = []
            for st, (cl, f) in enumerate(zip(cands, feats)):
                assert f.shape[0] == len(cl) - 1                             # the last candidate is never encoded (:600, :622)
                sims = f @ classes.T                                         # :605 / :627
                loss = utils_attacks.margin_loss_lm(sims, label)             # what the criterion computes per row (:161)
                arrays[f"{key}/{i}/{st}"] = loss.numpy().astype(np.float32)
                e = dict(n_candidates=len(cl))
                if st % 2 == 0:
                    e["top"] = torch.topk(loss, min(N, sims.shape[0]), dim=0).indices.tolist()          # :611
                else:
                    e["argmax"] = int(torch.argmax(loss).item())                                        # :639
                    e["pred"] = int(sims.softmax(dim=-1).argmax(dim=-1)[e["argmax"]].item())            # :630-631, :641
                if key == "mean3" and i in STRINGS_FOR:
                    e["candidates"] = cl
                if key == "mean3" and i == FEATURES_FOR and st < 2:
                    arrays[f"{key}/{i}/{st}/feat"] = f.numpy().astype(np.float32)
                stages.append(e)
            assert (stages[-1]["pred"] != label) or dist == K
            rows.append(dict(sentence=i, label=label, adv=adv, dist=dist, stages=stages))
        arrays[f"{key}/classes"] = classes.numpy().astype(np.float32)
        out["cases"][key] = dict(k=K, n=N, rows=rows)
        print(key, [r["dist"] for r in rows])

    d = [r["dist"] for r in out["cases"]["mean3"]["rows"]]
    assert sum(x >= 2 for x in d) >= 3 and K in d and 1 in d, d      # the multi-edit loop, the k-th edit and an early stop all occur
    w = out["cases"]["wrong_label"]["rows"][0]
    assert w["label"] != pred3[0] and w["dist"] >= 1 and w["adv"] != SENTENCES[0]

    with open(os.path.join(HERE, "zeroshot_trace.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    np.savez_compressed(os.path.join(HERE, "zeroshot_trace.npz"), **arrays)
    print("zero-shot fixtures written to", HERE)


if __name__ == "__main__":
    main()
