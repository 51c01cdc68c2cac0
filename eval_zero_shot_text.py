#!/usr/bin/env python3
"""Zero-shot text classification of a text encoder, clean and under Charmer with the classification margin loss.

Equivalent of the reference's ``eval_zero_shot_text.py:99-132``: every sentence is classified by the cosine similarity of its
embedding to one feature row per class, attacked with ``attack_text_charmer_classification`` (n = rho positions, at most k edits,
stopping as soon as the prediction leaves the label), and classified again.  Results go to
``results_zero_shot_text/<name>_<data>_k{k}_rho_{rho}[_text_only].csv`` with the reference's five columns, and one summary line
gives clean and adversarial accuracy.  Differences: everything is local.  ``--data`` is a text file with one example per line,
``label<TAB>text`` (the reference downloads AG-News, SST-2, ...); the class matrix is either the encoded ``--class-names`` (one
class caption per line, class c on line c: the reference's ``--label_encoder text``, file suffix ``_text_only``) or a ``[C, D]``
array ``--class-features FILE.npy``, normalised on load -- the reference's default ``--label_encoder image`` takes its class
features from an image tower, which this project does not have, so they come in as a file.  The character set V is ``[-1]`` + the
SORTED code points of ``--vocab-from`` (default: the texts of ``--data``); the reference takes the characters of the training split
in set order (utils_AT.py:30-43), and since V's order breaks ties between equal losses it is fixed here.  Sentences are attacked in
batches of ``--batch-size`` (``--per-sentence``: one at a time, the reference's loop); the attack draws no random numbers and both
give the same file.  The attack scores in the engine's default arithmetic; the reported labels come from the fp32-grade forward
unless ``--fast-columns`` is given (the convention of eval_textfare.py).

    python eval_zero_shot_text.py --model ViT-L-14-quickgelu --checkpoint /path/epoch_latest.pt --data agnews_test.tsv \
        --class-names agnews_classes.txt --vocab-from agnews_train.tsv --k 1 --rho 20 --n-test 100
"""
import argparse
import csv
import os

from leaf_amd import configure_runtime

configure_runtime()   # HIP_FORCE_DEV_KERNARG=1, before torch loads the HIP runtime (leaf_amd/__init__.py says why)
import numpy as np

COLUMNS = ["sentence", "original_label", "predicted_label", "adv_sentence", "adv_label"]


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14-quickgelu")
    ap.add_argument("--checkpoint", default=None, help="checkpoint of the evaluated text encoder")
    ap.add_argument("--random-init", action="store_true", help="allow --checkpoint to be omitted (seeded random weights)")
    ap.add_argument("--seed", type=int, default=1, help="seed of the random-init model (--random-init / tiny-test only)")
    ap.add_argument("--data", required=True, help="one example per line: label<TAB>text, label an integer class index")
    ap.add_argument("--class-names", default=None, help="one class caption per line; their normalised embeddings are the class matrix")
    ap.add_argument("--class-features", default=None, help=".npy file [C, D] with one feature row per class (normalised on load)")
    ap.add_argument("--vocab-from", default=None, help="file whose characters form V (default: --data)")
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--rho", type=int, default=20, help="Charmer's n: positions kept by stage 1")
    ap.add_argument("--n-test", type=int, default=100)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--per-sentence", action="store_true", help="one sentence per attack call, the reference's loop (same results, B = 1 launches)")
    ap.add_argument("--fast-columns", action="store_true",
                    help="compute the reported labels from the 16-bit forward the attack scores with instead of the fp32-grade one")
    ap.add_argument("--out-dir", default="results_zero_shot_text")
    a = ap.parse_args(argv)
    if (a.class_names is None) == (a.class_features is None):
        ap.error("give exactly one of --class-names and --class-features")
    if not a.checkpoint and not a.random_init and not a.model.startswith("tiny-test"):
        ap.error("--checkpoint is empty: pass the checkpoint, or --random-init to evaluate seeded random weights on purpose")
    if a.k < 0 or a.rho < 1 or a.batch_size < 1:
        ap.error("--k >= 0, --rho >= 1 and --batch-size >= 1")
    return a


def _text_of(line: str) -> str:
    """the text of a ``label<TAB>text`` line; a line without an integer label in front is text as a whole"""
    head, tab, rest = line.partition("\t")
    return rest if tab and head.strip().lstrip("-").isdigit() else line


def read_data(path: str, n_test=None):
    """[(label, text)] of a ``label<TAB>text`` file; empty lines and empty texts are skipped"""
    out = []
    with open(path, encoding="utf-8") as f:
        for ln, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            head, tab, text = line.partition("\t")
            try:
                label = int(head)
            except ValueError:
                label = None
            if not tab or label is None:
                raise SystemExit(f"{path}:{ln}: expected label<TAB>text with an integer label")
            if text.strip():
                out.append((label, text.strip()))
            if n_test is not None and len(out) == n_test:
                break
    return out


def build_vocab(path: str):
    """V = [-1] + the sorted code points of the file's texts (line ends excluded)"""
    chars = set()
    with open(path, encoding="utf-8") as f:
        for line in f:
            chars.update(_text_of(line.rstrip("\r\n")))
    return [-1] + sorted(ord(ch) for ch in chars)


def result_path(a) -> str:
    """<out-dir>/<name>_<data>_k{k}_rho_{rho}[_text_only].csv (the reference's name, eval_zero_shot_text.py:100-104)"""
    name = os.path.basename((a.checkpoint or a.model).rstrip("/")).split(".")[0]
    return os.path.join(a.out_dir, f"{name}_{os.path.basename(a.data).split('.')[0]}_k{a.k}_rho_{a.rho}" +
                        ("_text_only" if a.class_names else "") + ".csv")


def main(argv=None):
    """Returns the CSV's rows with two more keys: ``dist`` (edits received) and ``attack_flipped`` (the attack's own last prediction
    differs from the label)."""
    a = parse_args(argv)
    import torch

    from leaf_amd.charmer import attack_text_charmer_classification_batched
    from leaf_amd.model import create_model
    from leaf_amd.tokenizer import get_tokenizer
    data = read_data(a.data, a.n_test)
    V = build_vocab(a.vocab_from or a.data)
    model = create_model(a.model, pretrained=a.checkpoint, seed=a.seed)
    tok = get_tokenizer(a.model)
    precise = not a.fast_columns
    if a.class_names:
        with open(a.class_names, encoding="utf-8") as f:
            names = [l.strip() for l in f if l.strip()]
        classes = model.encode_text(tok.encode_batch(names), normalize=True)          # the arithmetic the attack scores in
        classes_rep = model.encode_text(tok.encode_batch(names), normalize=True, precise=True) if precise else classes
    else:
        arr = np.load(a.class_features).astype(np.float32)
        if arr.ndim != 2 or arr.shape[1] != model.cfg.embed_dim:
            raise SystemExit(f"{a.class_features}: expected [C, {model.cfg.embed_dim}], got {arr.shape}")
        classes = torch.from_numpy(arr / np.linalg.norm(arr, axis=-1, keepdims=True)).to(model.device)
        classes_rep = classes
    n_cls = classes.shape[0]
    bad = [lab for lab, _ in data if not 0 <= lab < n_cls]
    if bad:
        raise SystemExit(f"{a.data}: label {bad[0]} outside the {n_cls} classes")

    def predict(ids, labels):
        if precise:
            f = model.encode_text(ids, normalize=True, precise=True)
            return (f @ classes_rep.T).argmax(-1).cpu().numpy()
        # the scoring pass itself, one candidate per caption: the bits the attack saw
        return model.score_candidates_cls(ids, classes, labels, 1)[3][:, 0].cpu().numpy()

    os.makedirs(a.out_dir, exist_ok=True)
    path = result_path(a)
    bs = 1 if a.per_sentence else a.batch_size
    rows = []
    for i in range(0, len(data), bs):
        labels = [lab for lab, _ in data[i:i + bs]]
        batch = [s for _, s in data[i:i + bs]]
        preds = []
        adv, dists = attack_text_charmer_classification_batched(model, tok, batch, classes, labels, n=a.rho, k=a.k, V=V, return_preds=preds)
        last = [next((p[b] for p in reversed(preds) if p[b] is not None), None) for b in range(len(batch))]
        p_clean = predict(tok.encode_batch(batch), labels)
        p_adv = predict(tok.encode_batch(adv), labels)
        rows += [dict(sentence=s, original_label=lab, predicted_label=int(pc), adv_sentence=t, adv_label=int(pa), dist=d,
                      attack_flipped=(lp is not None and lp != lab))
                 for s, lab, pc, t, pa, d, lp in zip(batch, labels, p_clean, adv, p_adv, dists, last)]
        with open(path, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=COLUMNS, extrasaction="ignore")
            w.writeheader()
            w.writerows(rows)
    n = max(len(rows), 1)
    acc = sum(r["predicted_label"] == r["original_label"] for r in rows) / n
    acc_adv = sum(r["adv_label"] == r["original_label"] for r in rows) / n
    print(f"charmer classification k={a.k} rho={a.rho}: accuracy clean {acc:.4f} adv {acc_adv:.4f}  ({len(rows)} sentences, "
          f"{n_cls} classes) -> {path}")
    return rows


if __name__ == "__main__":
    main()
