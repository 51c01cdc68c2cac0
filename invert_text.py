#!/usr/bin/env python3
"""Text embedding inversion (PEZ) of a text encoder: reconstruct captions from their embeddings alone.

Equivalent of the reference's ``src/pez/run_coco.py`` followed by ``src/pez/compute_metrics.py``: every caption of ``--captions``
(one per line, the first ``--n-samples``) is embedded, a prompt of the caption's own token count is optimised for ``--iter``
iterations to reproduce that embedding (leaf_amd/inversion.py), and the reconstructions are written as JSON
``{"config", "results", "metrics"}`` -- ``results`` holds the reference's dict per caption (original, reconstructed, ids_rec, sim,
ids_orig), ``metrics`` the mean cosine, word accuracy and token accuracy (BLEU is left out).  ``--config`` is a JSON file with the
reference's keys (coco_config.json: seed, prompt_len, lr, weight_decay, loss_weight, print_step; iter, prompt_bs, batch_size are
read too); command-line flags win over it.  Differences: everything is local (``--checkpoint`` is an OpenCLIP / HF file), and
``--batch`` captions are inverted at once instead of one after the other -- every caption still gets its own prompt, target and
the reference's per-caption seeded start.

    python invert_text.py --model ViT-L-14-quickgelu --checkpoint /path/epoch_latest.pt --captions coco_captions.txt \
        --n-samples 100 --iter 3000 --out results_inversions/robust.json
"""
import argparse
import json
import os

from leaf_amd import configure_runtime

configure_runtime()   # HIP_FORCE_DEV_KERNARG=1, before torch loads the HIP runtime (leaf_amd/__init__.py says why)

CONFIG_DEFAULTS = {"seed": 0, "prompt_len": "match", "lr": 0.1, "weight_decay": 0.1, "loss_weight": 1.0, "print_step": None,
                   "iter": 3000, "prompt_bs": 1, "batch_size": 1}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14-quickgelu")
    ap.add_argument("--checkpoint", default=None, help="checkpoint of the inverted text encoder (OpenCLIP .pt / .bin or HF safetensors)")
    ap.add_argument("--random-init", action="store_true", help="allow --checkpoint to be omitted (seeded random weights)")
    ap.add_argument("--captions", required=True, help="text file, one caption per line")
    ap.add_argument("--n-samples", type=int, default=100, help="number of captions to invert (the first ones of the file)")
    ap.add_argument("--iter", type=int, default=None, help="optimisation steps per caption (default: the config's, else 3000)")
    ap.add_argument("--config", default=None, help="JSON with the reference's keys: seed, prompt_len, lr, weight_decay, loss_weight, print_step")
    ap.add_argument("--batch", type=int, default=64, help="captions inverted at once")
    ap.add_argument("--out", default=None, help="result file (default: results_inversions/results-<n>smpls-<iter>iters-<name>.json)")
    a = ap.parse_args(argv)
    if not a.checkpoint and not a.random_init and not a.model.startswith("tiny-test"):
        ap.error("--checkpoint is empty: pass the checkpoint, or --random-init to invert seeded random weights on purpose")
    if a.n_samples < 1 or a.batch < 1:
        ap.error("--n-samples >= 1 and --batch >= 1")
    return a


def load_config(path, iters=None) -> dict:
    """The reference's config keys over their defaults; unknown keys are an error (a typo would silently run the default)."""
    cfg = dict(CONFIG_DEFAULTS)
    if path:
        with open(path, encoding="utf-8") as f:
            given = json.load(f)
        unknown = sorted(set(given) - set(cfg))
        if unknown:
            raise SystemExit(f"{path}: unknown config keys {unknown}; known: {sorted(cfg)}")
        cfg.update(given)
    if iters is not None:
        cfg["iter"] = iters
    if cfg["prompt_len"] != "match":
        cfg["prompt_len"] = int(cfg["prompt_len"])
    if int(cfg["prompt_bs"]) != 1:
        raise SystemExit("prompt_bs > 1 is out of scope: one prompt is optimised per caption")
    if cfg["batch_size"] not in (1, None):
        raise SystemExit("batch_size (targets sampled per step) must be 1: every inversion has one target")
    if int(cfg["iter"]) < 1:
        raise SystemExit("iter >= 1")
    return cfg


def read_captions(path: str, n: int):
    with open(path, encoding="utf-8") as f:
        out = [l.strip() for l in f.readlines()[:n]]            # run_coco.py:109-110,126
    if not out or any(not c for c in out):
        raise SystemExit(f"{path}: an empty caption among the first {n} lines")
    return out


def result_path(a, cfg) -> str:
    name = os.path.basename((a.checkpoint or a.model).rstrip("/")).split(".")[0]
    return a.out or os.path.join("results_inversions", f"results-{a.n_samples}smpls-{cfg['iter']}iters-{name}.json")


def main(argv=None):
    a = parse_args(argv)
    cfg = load_config(a.config, a.iter)
    captions = read_captions(a.captions, a.n_samples)
    from leaf_amd.inversion import invert_text, summarize
    from leaf_amd.model import create_model
    from leaf_amd.tokenizer import get_tokenizer
    model = create_model(a.model, pretrained=a.checkpoint, seed=1)
    results = invert_text(model, get_tokenizer(a.model), captions=captions, prompt_len=cfg["prompt_len"], iters=int(cfg["iter"]),
                          lr=float(cfg["lr"]), weight_decay=float(cfg["weight_decay"]), loss_weight=float(cfg["loss_weight"]),
                          seed=int(cfg["seed"]), batch=a.batch, print_step=cfg["print_step"])
    metrics = summarize(results)
    out = {"config": dict(cfg, model=a.model, checkpoint=a.checkpoint, n_samples=len(captions), batch=a.batch),
           "results": results, "metrics": metrics}
    path = result_path(a, cfg)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=2)
    print(f"inverted {len(results)} captions, {cfg['iter']} iterations: cos-sim {metrics['cos-sim']:.4f}, word accuracy "
          f"{100 * metrics['word accuracy']:.2f}, token accuracy {100 * metrics['token accuracy']:.2f} -> {path}")
    return out


if __name__ == "__main__":
    main()
