#!/usr/bin/env python3
"""Throughput of the batched Charmer attack (leaf_amd/charmer.py) against the reference's loop shape (one sentence per call):
ViT-L random init, synthetic captions (leaf_amd.train._SYN_WORDS), k in {1, 2}, n in {10, 20}.  Prints per setting the sentences/s
of both, the scored candidate rows/s of the batched run, and the fraction of work removed by duplicate skipping (candidate rows)
and by prefix reuse (token rows of the remaining candidates).  Informational: nothing is gated on it.

    python tools/charmer_bench.py [--batch 64] [--model ViT-L-14] [--loop-sentences 8] [--classes 4]
"""
import argparse
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from leaf_amd import configure_runtime  # noqa: E402

configure_runtime()
import torch  # noqa: E402

from leaf_amd.charmer import attack_text_charmer, attack_text_charmer_classification_batched  # noqa: E402
from leaf_amd.model import create_model  # noqa: E402
from leaf_amd.native_text import NativeTokenizer  # noqa: E402
from leaf_amd.train import _SYN_WORDS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="ViT-L-14")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--loop-sentences", type=int, default=8, help="sentences timed in the one-per-call loop (same captions, a prefix)")
ap.add_argument("--ks", default="1,2")
ap.add_argument("--ns", default="10,20")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--classes", type=int, default=0, help="> 0: the classification attack (margin loss, early stop) against this many "
                "random unit class rows, labels = the clean predictions, instead of the l2 attack")
a = ap.parse_args()

rng = random.Random(a.seed)
caps = [" ".join(rng.choice(_SYN_WORDS) for _ in range(rng.randint(3, 14))) for _ in range(a.batch)]
m = create_model(a.model, device="cuda:0", seed=1)
tok = NativeTokenizer()
anchor = m.encode_text(tok.encode_batch(caps))
if a.classes:
    classes = torch.nn.functional.normalize(torch.randn(a.classes, anchor.shape[1], generator=torch.Generator().manual_seed(a.seed)), dim=-1).cuda()
    labels = (torch.nn.functional.normalize(anchor, dim=-1) @ classes.T).argmax(-1).tolist()


def attack(idx, n, k, stats=None):
    sub = [caps[i] for i in idx]
    if a.classes:
        return attack_text_charmer_classification_batched(m, tok, sub, classes, [labels[i] for i in idx], n, k, stats=stats)
    return attack_text_charmer(m, tok, sub, anchor[idx].clone(), "l2", n, k, stats=stats)


attack(list(range(4)), 10, 1)        # warm-up: workspaces, K/V slots, kernels
torch.cuda.synchronize()
print(f"{a.model}: B = {a.batch} synthetic captions, mean {sum(map(len, caps)) / len(caps):.1f} characters")
for k in map(int, a.ks.split(",")):
    for n in map(int, a.ns.split(",")):
        stats = {}
        t0 = time.time()
        adv, _ = attack(list(range(a.batch)), n, k, stats)
        torch.cuda.synchronize()
        tb = time.time() - t0
        nl = min(a.loop_sentences, a.batch)
        t0 = time.time()
        for i in range(nl):
            one, _ = attack([i], n, k)
            assert one[0] == adv[i], "batched and per-sentence runs differ"
        torch.cuda.synchronize()
        tl = max(time.time() - t0, 1e-9)
        nl = max(nl, 1e-9)            # --loop-sentences 0: the batched run alone (profiling)
        cand, dup = stats["candidates"], stats["duplicates"]
        print(f"k={k} n={n:2d}: batched {a.batch / tb:8.1f} sentences/s ({tb * 1e3:7.1f} ms)   per-sentence loop {nl / tl:7.1f} "
              f"sentences/s   x{(a.batch / tb) / (nl / tl):5.1f}   scored candidates {cand / tb:,.0f}/s   duplicates skipped "
              f"{dup / max(cand, 1):.1%} of candidates   token rows computed {stats['computed_rows']:,} of {stats['full_rows']:,} "
              f"({1 - stats['computed_rows'] / max(stats['full_rows'], 1):.1%} removed by prefix reuse + dedupe)", flush=True)
