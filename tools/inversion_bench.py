#!/usr/bin/env python3
"""Throughput of text embedding inversion (leaf_amd/inversion.py) and of its projection kernel (leaf_amd/csrc/nnproj.hip).
Informational: nothing is gated on it.

  loop      ViT-L random init, --batch synthetic captions: iterations/s of the batched loop (every caption advances one step per
            iteration) against the one-caption loop, the reference's shape (src/pez/run_coco.py: one caption after the other).
  project   leaf_nn_project at M in {16, 256, 1024} query rows against torch.mm + argmax on the same device and the same fp32 table
            (normalised once, outside the timed region, as the kernel's inverse norms are): time, fraction of the 155 TFLOP/s fp32
            matrix peak, and the table bytes a call must read (V d 4: the vocabulary is stationary, read once per call).

The projection kernel's share of a loop iteration comes from a kernel trace of its own:
    rocprofv3 --kernel-trace --stats -- python tools/inversion_bench.py --mode loop --iters 20 --loop-captions 0

    python tools/inversion_bench.py [--mode loop|project|both] [--batch 64] [--iters 50] [--model ViT-L-14]
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

from leaf_amd.inversion import invert_text  # noqa: E402
from leaf_amd.model import create_model  # noqa: E402
from leaf_amd.tokenizer import SimpleTokenizer  # noqa: E402
from leaf_amd.train import _SYN_WORDS  # noqa: E402

PEAK_F32_MATRIX = 155e12        # measured fp32 MFMA rate of the MI355X

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="ViT-L-14")
ap.add_argument("--mode", default="both", choices=["loop", "project", "both"])
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--loop-captions", type=int, default=4, help="captions timed one at a time (a prefix of the batch); 0 = batched run only")
ap.add_argument("--rows", default="16,256,1024")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()

m = create_model(a.model, device="cuda:0", seed=1)
tok = SimpleTokenizer()
V, d = m.cfg.vocab_size, m.cfg.width


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


if a.mode in ("loop", "both"):
    rng = random.Random(a.seed)
    caps = [" ".join(rng.choice(_SYN_WORDS) for _ in range(rng.randint(3, 14))) for _ in range(a.batch)]
    invert_text(m, tok, captions=caps[:2], iters=2)                  # warm-up: workspaces, stash, kernels
    torch.cuda.synchronize()
    t0 = time.time()
    res = invert_text(m, tok, captions=caps, iters=a.iters, batch=a.batch)
    torch.cuda.synchronize()
    tb = time.time() - t0
    rows = sum(len(r["ids_rec"]) for r in res)
    line = (f"{a.model} loop: {a.batch} captions ({rows} prompt rows), {a.iters} iterations: batched {a.iters / tb:7.1f} iterations/s "
            f"({tb / a.iters * 1e3:6.2f} ms each, {a.batch * a.iters / tb:8.1f} caption-steps/s)")
    nl = min(a.loop_captions, a.batch)
    if nl:
        t0 = time.time()
        for i in range(nl):
            invert_text(m, tok, captions=[caps[i]], iters=a.iters)
        torch.cuda.synchronize()
        tl = time.time() - t0
        line += (f"   one caption at a time {nl * a.iters / tl:7.1f} caption-steps/s ({tl / nl / a.iters * 1e3:6.2f} ms per step)"
                 f"   x{(a.batch * a.iters / tb) / (nl * a.iters / tl):5.1f}")
    print(line, flush=True)

if a.mode in ("project", "both"):
    table = m.params["token_embedding.weight"]
    tn = torch.nn.functional.normalize(table, dim=1)                 # the baseline's normalised table, built once
    print(f"{a.model} projection: V = {V}, d = {d}, table {V * d * 4 / 1e6:.1f} MB read per call")
    for M in map(int, a.rows.split(",")):
        g = torch.Generator().manual_seed(M)
        q = (table[torch.randint(V, (M,), generator=g).cuda()] + 0.01 * torch.randn(M, d, generator=g).cuda()).contiguous()
        m.nn_project(q)
        t_k = timed(lambda: m.nn_project(q), a.reps)
        t_b = timed(lambda: torch.mm(q, tn.T).argmax(1), a.reps)
        same = float((m.nn_project(q)[0].long() == torch.mm(q, tn.T).argmax(1)).float().mean())
        fl = 2.0 * M * V * d
        print(f"  M = {M:5d}: leaf_nn_project {t_k * 1e6:8.1f} us ({fl / t_k / 1e12:6.1f} TFLOP/s, {fl / t_k / PEAK_F32_MATRIX:6.1%} of the "
              f"fp32 matrix peak, table at {V * d * 4 / t_k / 1e12:5.2f} TB/s)   torch.mm + argmax {t_b * 1e6:8.1f} us "
              f"({fl / t_b / 1e12:6.1f} TFLOP/s)   kernel / baseline time {t_k / t_b:5.2f}   same ids {same:.1%}", flush=True)
