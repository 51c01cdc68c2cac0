#!/usr/bin/env python3
"""Golden fixture for text embedding inversion (PEZ), produced by the REFERENCE's own code: ``optimize_prompt_loop`` /
``nn_project`` (src/pez/optim_utils.py:26-55,139-232) on ``open_clip_pez.model.CLIP`` (src/pez/open_clip_pez/model.py:210-246),
tiny quickgelu tower with oracle.init_weights(seed=12), CPU, fp32.

The loop runs UNCHANGED; its per-iteration state is recorded from outside by wrapping ``nn_project`` (prompt embeddings before the
step, projected ids), ``torch.autograd.grad`` (loss -> cosine, gradient) and ``torch.randint`` (the initial ids).  The embeddings
after step k are the embeddings before step k + 1, so ``<name>_emb`` holds iters + 1 states.  ``sentence_transformers`` is absent
here: its three functions the loop imports are stubbed with plain torch (third-party, not reference code).

Case ``interior_eot``: a direct call of ``forward_text_embedding(..., return_feature=True)`` on a prompt with id 49407 planted at an
interior position, its feature, and the gradient of 1 - cos(feature, target) with respect to the prompt embeddings.

Runs only in the build container.   python tests/golden/make_golden_pez.py  ->  tests/golden/tiny_pez.npz
"""
import argparse
import importlib.machinery
import json
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (stubs, TINY config, weight loading)

CAPTIONS = ["cat", "a photo of cat", "two people in the big park at sunset today",          # P = 1, 4, 9, 15
            "a man with a red hat and a dog on the table in the park"]
ITERS, LR, WD, SEED, LOSS_WEIGHT = 30, 0.1, 0.1, 0, 1.0


def stub_third_party():
    st = types.ModuleType("sentence_transformers")
    st.__spec__ = importlib.machinery.ModuleSpec("sentence_transformers", None)
    util = types.ModuleType("sentence_transformers.util")
    util.normalize_embeddings = lambda e: torch.nn.functional.normalize(e, p=2, dim=1)
    util.dot_score = lambda a, b: a @ b.t()

    def semantic_search(queries, corpus, query_chunk_size=100, corpus_chunk_size=500000, top_k=10, score_function=None):
        scores = (score_function or util.dot_score)(queries, corpus)
        val, idx = torch.topk(scores, min(top_k, scores.shape[1]), dim=1, largest=True, sorted=True)
        return [[{"corpus_id": int(i), "score": float(v)} for v, i in zip(vr, ir)] for vr, ir in zip(val, idx)]
    util.semantic_search = semantic_search
    st.util = util
    sys.modules.update({"sentence_transformers": st, "sentence_transformers.util": util})
    for name in ("requests",):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = MagicMock()


def main():
    MG.install_stubs()
    stub_third_party()
    sys.path.insert(0, os.path.join(MG.REF, "src", "pez"))
    import open_clip_pez
    from open_clip_pez.model import CLIP
    import optim_utils as OU
    from oracle import text_oracle as O

    torch.set_num_threads(8)
    cfg = O.TextCfg(128, 2, 2, 64, quick_gelu=True)
    w = O.init_weights(cfg, seed=12)
    model = CLIP(**MG.TINY, quick_gelu=True).float().eval()
    MG.load_np_state(model, w)
    for p in model.parameters():
        p.requires_grad = False
    tokenizer = open_clip_pez.tokenizer._tokenizer

    rec = {}
    orig_nn, orig_grad, orig_randint = OU.nn_project, torch.autograd.grad, torch.randint

    def nn_project(curr_embeds, embedding_layer, print_hits=False):
        rec["emb"].append(curr_embeds.detach().numpy()[0].copy())
        rec["live"] = curr_embeds
        out = orig_nn(curr_embeds, embedding_layer, print_hits=print_hits)
        rec["ids"].append(out[1].numpy()[0].astype(np.int32))
        return out

    def grad(loss, inputs, *a, **k):
        g = orig_grad(loss, inputs, *a, **k)
        rec["cos"].append(1.0 - float(loss.item()) / LOSS_WEIGHT)
        rec["grad"].append(g[0].detach().numpy()[0].copy())
        return g

    def randint(*a, **k):
        out = orig_randint(*a, **k)
        rec.setdefault("init", out.numpy().reshape(-1).astype(np.int32))
        return out

    out, meta = {}, {"captions": CAPTIONS, "iters": ITERS, "lr": LR, "weight_decay": WD, "seed": SEED, "loss_weight": LOSS_WEIGHT,
                     "results": []}
    targets = []
    OU.nn_project, torch.autograd.grad, torch.randint = nn_project, grad, randint
    try:
        for c, text in enumerate(CAPTIONS):
            ids = open_clip_pez.tokenize([text])
            P = int((ids != 0).sum()) - 2                  # run_coco.py:17-21 (prompt_len "match")
            args = argparse.Namespace(iter=ITERS, lr=LR, weight_decay=WD, print_step=None, batch_size=1, prompt_bs=1, prompt_len=P,
                                      loss_weight=LOSS_WEIGHT, seed=SEED)
            import random
            random.seed(SEED); np.random.seed(SEED); torch.manual_seed(SEED)       # run_coco.py:25-28
            rec.clear()
            rec.update(emb=[], ids=[], cos=[], grad=[])
            with torch.no_grad():
                target = model.encode_text(ids)                                   # get_target_feature, optim_utils.py:103-104
            res = OU.optimize_prompt_loop(model, tokenizer, model.token_embedding, target, args, "cpu")
            rec["emb"].append(rec["live"].detach().numpy()[0].copy())              # after the last step
            assert len(rec["ids"]) == ITERS and len(rec["grad"]) == ITERS and len(rec["emb"]) == ITERS + 1
            out[f"c{c}_emb"] = np.stack(rec["emb"]).astype(np.float32)             # [iters + 1, P, d]
            out[f"c{c}_ids"] = np.stack(rec["ids"])                                # [iters, P]
            out[f"c{c}_cos"] = np.asarray(rec["cos"], np.float64)
            out[f"c{c}_grad"] = np.stack(rec["grad"]).astype(np.float32)           # [iters, P, d]
            out[f"c{c}_init_ids"] = rec["init"]
            out[f"c{c}_target"] = target.numpy()[0]
            out[f"c{c}_tokens"] = ids.numpy()[0].astype(np.int32)
            targets.append(target)
            meta["results"].append({"original": text, "reconstructed": res["reconstructed"], "ids_rec": [int(i) for i in res["ids_rec"]],
                                    "sim": float(res["sim"]), "ids_orig": [int(i) for i in ids[0].tolist()]})
    finally:
        OU.nn_project, torch.autograd.grad, torch.randint = orig_nn, orig_grad, orig_randint

    # interior EOT: the pooled row is the template's EOT slot (dummy ids), not the first 49407 among the prompt's ids
    pids = np.array([320, 49407, 1125, 49406, 2368], dtype=np.int64)
    P = len(pids)
    dummy = torch.tensor([[49406] + [-1] * P + [49407] + [0] * (77 - P - 2)])
    tmp = dummy.clone()
    tmp[tmp == -1] = 0
    with torch.no_grad():
        padded = model.token_embedding(tmp).detach().clone()
    emb = model.token_embedding(torch.from_numpy(pids)).detach().clone().requires_grad_(True)
    padded[dummy == -1] = emb
    feat = model.forward_text_embedding(padded, dummy, None, return_feature=True)
    t = targets[2]
    cos = (feat / feat.norm(dim=1, keepdim=True)) @ (t / t.norm(dim=1, keepdim=True)).t()
    (g,) = torch.autograd.grad(1 - cos.mean(), [emb])
    out["interior_eot_ids"] = pids.astype(np.int32)
    out["interior_eot_feat"] = feat.detach().numpy()[0]
    out["interior_eot_target"] = t.numpy()[0]
    out["interior_eot_cos"] = np.float64(cos.item())
    out["interior_eot_grad"] = g.numpy().copy()
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "tiny_pez.npz")
    np.savez_compressed(path, **out)
    print("written tiny_pez.npz", os.path.getsize(path), "bytes;", [(r["original"], round(r["sim"], 4)) for r in meta["results"]])


if __name__ == "__main__":
    main()
