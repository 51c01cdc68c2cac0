#!/usr/bin/env python3
"""Per-token prompt embeddings of a text encoder for a diffusion pipeline that runs elsewhere: the text half of the reference's
``eval_text_to_image.py``.

The reference puts the fine-tuned tower into a Stable Diffusion pipeline as ``pipeline.text_encoder`` (eval_text_to_image.py:172-178);
the pipeline reads per-token states, not the pooled embedding.  This tool writes them to an ``.npz`` that the pipeline takes as
``prompt_embeds`` / ``pooled_prompt_embeds`` (as ``eval_zero_shot_text.py --class-features`` takes image-side arrays from elsewhere):

    prompt_embeds         [N, 77, width]   hidden state ``--layer`` (HF ``hidden_states`` index, negative from the end), through ln_final
                                           unless ``--no-final-ln``.  SD 1.x: ``--layer -1``; SDXL: ``--layer -2 --no-final-ln``;
                                           SD 2.x / clip_skip: ``--layer -2``
    pooled_prompt_embeds  [N, embed_dim]   the projected features of the same pass (SDXL's ``text_embeds``)
    input_ids             [N, 77]          the ids that were encoded (``--pad eot``: HF's padding with the EOT id, the default;
                                           ``--pad zero``: open_clip's)

With ``--attack-name charmer --k K --rho N`` (the batched Charmer ``eval_textfare.py`` calls; anchor = the clean feature, objective
``--adv-objective``) it also writes ``perturbed_captions``, their ``adv_prompt_embeds`` / ``adv_pooled_prompt_embeds`` and
``clean_adv_cosine`` -- the ``caps_corr_model_text_encoder`` column of eval_text_to_image.py:201-226.  Image generation and the
CLIP-score columns stay outside the engine.

    python encode_prompts.py --model ViT-L-14-quickgelu --checkpoint /path/epoch_latest.pt --texts captions.txt --out prompts.npz
"""
import argparse

from leaf_amd import configure_runtime

configure_runtime()   # HIP_FORCE_DEV_KERNARG=1, before torch loads the HIP runtime (leaf_amd/__init__.py says why)
import string

import numpy as np


def pad_with_eot(ids: np.ndarray) -> np.ndarray:
    """open_clip's rows (pad id 0) -> HF's (every slot behind the EOT holds the EOT id); the first maximum stays where it was"""
    ids = ids.copy()
    eot = ids.argmax(-1)
    for row, e in zip(ids, eot):
        row[e + 1:] = row[e]
    return ids


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="ViT-L-14-quickgelu")
    ap.add_argument("--checkpoint", default=None, help="checkpoint of the text encoder (OpenCLIP .bin/.pt or HF directory)")
    ap.add_argument("--random-init", action="store_true", help="allow --checkpoint to be omitted (seeded random weights)")
    ap.add_argument("--seed", type=int, default=1, help="seed of the random-init model")
    ap.add_argument("--texts", required=True, help="one prompt per line")
    ap.add_argument("--n-test", type=int, default=None, help="only the first N prompts")
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--layer", type=int, default=-1, help="HF hidden_states index: 0 = embedding .. layers = last block; negative from the end")
    ap.add_argument("--final-ln", dest="final_ln", action="store_true", default=True, help="apply ln_final to every row (default)")
    ap.add_argument("--no-final-ln", dest="final_ln", action="store_false")
    ap.add_argument("--precise", action="store_true", help="the fp32-grade forward (precise.hip) instead of the 16-bit one")
    ap.add_argument("--pad", choices=["eot", "zero"], default="eot", help="ids behind the EOT: the EOT id (HF, default) or 0 (open_clip)")
    ap.add_argument("--out", required=True, help="FILE.npz")
    ap.add_argument("--attack-name", "--attack_name", dest="attack_name", choices=["none", "charmer"], default="none")
    ap.add_argument("--k", type=int, default=None, help="Charmer: edits per prompt")
    ap.add_argument("--rho", type=int, default=None, help="Charmer: positions per edit")
    ap.add_argument("--adv-objective", "--adv_objective", dest="adv_objective", choices=["l2", "negl2", "sim", "dissim"], default="l2")
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    from leaf_amd.model import get_config
    if not a.out.endswith(".npz"):
        ap.error("--out must name an .npz file")
    if a.attack_name == "none" and (a.k is not None or a.rho is not None):
        ap.error("--k / --rho belong to --attack-name charmer")
    if a.attack_name == "charmer" and (a.k is None or a.rho is None or a.k < 1 or a.rho < 1):
        ap.error("--attack-name charmer needs --k >= 1 and --rho >= 1")
    if a.batch_size < 1:
        ap.error("--batch-size must be >= 1")
    try:
        layers = get_config(a.model).layers
    except KeyError as e:
        ap.error(str(e.args[0]))
    if not -(layers + 1) <= a.layer <= layers:
        ap.error(f"--layer {a.layer}: hidden_states of {a.model} has {layers + 1} entries (0 .. {layers}, or -{layers + 1} .. -1)")
    if not a.checkpoint and not a.random_init and not a.model.startswith("tiny-test"):
        ap.error("--checkpoint is empty: pass the encoder's checkpoint, or --random-init to encode with seeded random weights on purpose")

    from leaf_amd.charmer import attack_text_charmer
    from leaf_amd.model import create_model
    from leaf_amd.tokenizer import get_tokenizer
    model = create_model(a.model, pretrained=a.checkpoint, seed=a.seed)
    tok = get_tokenizer(a.model)
    with open(a.texts) as f:
        prompts = [l.strip() for l in f if l.strip()][:a.n_test]
    V = [-1] + [ord(c) for c in string.ascii_lowercase + ' ' + string.ascii_uppercase + string.digits + string.punctuation]

    def encode(texts):
        ids = tok.encode_batch(texts)
        if a.pad == "eot":
            ids = pad_with_eot(ids)
        (states,), feat = model.encode_text_hidden(ids, layers=(a.layer,), final_ln=a.final_ln, precise=a.precise, want_features=True)
        return ids, states.cpu().numpy(), feat

    out = {k: [] for k in ("input_ids", "prompt_embeds", "pooled_prompt_embeds")}
    adv_out = {k: [] for k in ("perturbed_captions", "adv_prompt_embeds", "adv_pooled_prompt_embeds", "clean_adv_cosine")}
    for i in range(0, len(prompts), a.batch_size):
        batch = prompts[i:i + a.batch_size]
        ids, states, feat = encode(batch)
        out["input_ids"].append(ids)
        out["prompt_embeds"].append(states)
        out["pooled_prompt_embeds"].append(feat.cpu().numpy())
        if a.attack_name == "charmer":
            # the attack's anchor is the clean feature in the arithmetic the candidates are scored in (eval_text_to_image.py:207,219)
            adv, _ = attack_text_charmer(model, tok, batch, model.encode_text(tok.encode_batch(batch)), objective=a.adv_objective, n=a.rho, k=a.k, V=V)
            _, adv_states, adv_feat = encode(adv)
            cos = (feat * adv_feat).sum(-1) / (feat.norm(dim=-1) * adv_feat.norm(dim=-1))       # eval_text_to_image.py:222
            adv_out["perturbed_captions"] += list(adv)
            adv_out["adv_prompt_embeds"].append(adv_states)
            adv_out["adv_pooled_prompt_embeds"].append(adv_feat.cpu().numpy())
            adv_out["clean_adv_cosine"].append(cos.cpu().numpy())
    cfg = model.cfg
    empty = {"input_ids": (0, cfg.context_length), "prompt_embeds": (0, cfg.context_length, cfg.width), "pooled_prompt_embeds": (0, cfg.embed_dim)}
    arrays = {k: np.concatenate(v) if v else np.zeros(empty[k], np.int32 if k == "input_ids" else np.float32) for k, v in out.items()}
    arrays["captions"] = np.array(prompts, dtype=str)
    if a.attack_name == "charmer" and prompts:
        arrays["perturbed_captions"] = np.array(adv_out["perturbed_captions"], dtype=str)
        for k in ("adv_prompt_embeds", "adv_pooled_prompt_embeds", "clean_adv_cosine"):
            arrays[k] = np.concatenate(adv_out[k])
    arrays["layer"] = np.int32(a.layer)
    arrays["final_ln"] = np.int32(a.final_ln)
    np.savez(a.out, **arrays)
    msg = f"{len(prompts)} prompts, hidden_states[{a.layer}]{' + ln_final' if a.final_ln else ''}{' (precise)' if a.precise else ''} -> {a.out}"
    if "clean_adv_cosine" in arrays:
        msg += f"; charmer k={a.k} rho={a.rho}: mean clean/adversarial cosine {float(arrays['clean_adv_cosine'].mean()):.4f}"
    print(msg)
    return arrays


if __name__ == "__main__":
    main()
