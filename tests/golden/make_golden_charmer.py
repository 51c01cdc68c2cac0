#!/usr/bin/env python3
"""Fixture for the batched Charmer / brute-force attacks (leaf_amd/charmer.py): the reference's own
``attack_text_charmer_inference`` (utils_attacks.py:451-580) and ``attack_text_bruteforce`` (:395-449), one sentence per call, on
the tiny quickgelu model of weight seed 12 (the model of attack_trace.json), CPU, fp32.

Runs only in the build container (needs /root/reference; same stub recipe as make_golden.py).  A spying tokenizer records every
stage's candidate list and a wrapped ``encode_text`` every stage's features; the stage losses are recomputed from them with the
reference's own expression and the top-n positions with its own ``torch.topk`` call.  Stored (inputs and outputs only):

* charmer_trace.json: per case and sentence the adversarial sentence, per stage the number of candidates and the top-n positions;
  the full candidate strings for two sentences per case (``strings_for``)
* charmer_trace.npz: the anchors per case and the stage losses ("<case>/<sentence>/<stage>")

    python tests/golden/make_golden_charmer.py
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

SENTENCES = ["a photo of a cat", "A Photo of a DOG on the table!", "two  people in the park", "Hi.",
             "the red car at sunset, with a hat", "I'm sure it's 42 degrees", "x", "Stocks rally as oil prices fall"]
STRINGS_FOR = (1, 3)                 # full candidate strings for these sentences (capitals + punctuation; 2 L < n)
CASES = [("k1_n5", dict(k=1, n=5, constrain=False)),
         ("k2_n10", dict(k=2, n=10, constrain=False)),
         ("k1_n5_c", dict(k=1, n=5, constrain=True))]
BRUTE = ["a cat", "Hi.", "x y"]


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

    out = {"sentences": SENTENCES, "stub_words": STUB_WORDS, "V": V_DEFAULT, "model": "tiny-test-quickgelu", "weight_seed": 12,
           "strings_for": list(STRINGS_FOR), "cases": {}}
    arrays = {}
    with torch.no_grad():
        anchors = encode(tokenizer(SENTENCES)).detach()
    for key, cs in CASES:
        rows = []
        for i, s in enumerate(SENTENCES):
            del cands[:], feats[:]
            anchor = anchors[i:i + 1].clone()
            with torch.no_grad():
                adv, dist = utils_attacks.attack_text_charmer_inference(model, SpyTok(), s, anchor, "cpu", objective="l2", n=cs["n"],
                                                                        k=cs["k"], V=V_DEFAULT, constrain=cs["constrain"])
            assert len(cands) == 2 * cs["k"], (key, s, len(cands))
            # one encode_text call per stage (every stage has fewer candidates than the reference's 2,560-row chunks)
            assert len(feats) == 2 * cs["k"]
            stages = []
            for st, (cl, f) in enumerate(zip(cands, feats)):
                loss = ((f - anchor) ** 2).sum(dim=-1)                      # utils_attacks.py:497 / :552, same expression
                arrays[f"{key}/{i}/{st}"] = loss.numpy().astype(np.float32)
                e = dict(n_candidates=len(cl))
                if st % 2 == 0:
                    e["top"] = torch.topk(loss, min(cs["n"], loss.shape[0]), dim=0).indices.tolist()    # :506
                else:
                    e["argmax"] = int(torch.argmax(loss).item())                                        # :574
                if i in STRINGS_FOR:
                    e["candidates"] = cl
                stages.append(e)
            rows.append(dict(adv=adv, dist=dist, stages=stages))
        out["cases"][key] = dict(cs, rows=rows)
    arrays["anchors"] = anchors.numpy().astype(np.float32)

    rows = []
    with torch.no_grad():
        banchors = encode(tokenizer(BRUTE)).detach()
    for i, s in enumerate(BRUTE):
        del cands[:], feats[:]
        anchor = banchors[i:i + 1].clone()
        with torch.no_grad():
            adv, dist = utils_attacks.attack_text_bruteforce(model, SpyTok(), s, anchor, "cpu", objective="l2", V=V_DEFAULT)
        f = torch.cat(feats, 0)
        loss = ((f - anchor) ** 2).sum(dim=-1)                              # utils_attacks.py:430
        arrays[f"brute/{i}"] = loss.numpy().astype(np.float32)
        scored = [x for cl in cands for x in cl]                            # the tokenizer sees the scored chunks only (:422-427)
        rows.append(dict(adv=adv, dist=dist, n_scored=len(scored), argmax=int(torch.argmax(loss).item()),
                         candidates=scored if i == 0 else None))
    arrays["brute_anchors"] = banchors.numpy().astype(np.float32)
    out["brute"] = dict(sentences=BRUTE, rows=rows)

    with open(os.path.join(HERE, "charmer_trace.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    np.savez_compressed(os.path.join(HERE, "charmer_trace.npz"), **arrays)
    print("charmer fixtures written to", HERE)


if __name__ == "__main__":
    main()
