"""Text tower of CLIP on the HIP engine, behind the reference's ``model.encode_text`` seam.

``LeafCLIPText`` owns ONE flat fp32 parameter tensor on the GPU (layout defined by libleaf_hip, decay
group first) plus 16-bit MFMA operand copies, and exposes

* ``encode_text(text, normalize=False)``   -- src/open_clip/model.py:269-284
* ``score_candidates(tokens, anchor, rho, objective)`` -- one stage of utils_attacks.py:297-393
* ``encode_text_hidden(text, layers, final_ln)``     -- per-token hidden states in HF's ``hidden_states`` index (leaf_amd/hf_text.py)
* ``forward_train`` / ``backward`` / ``adamw_step``    -- utils_AT.py:317-362
* ``encode_text_train`` / ``backward_from``            -- the same forward under autograd: any PyTorch loss of the features
* ``state_dict`` / ``load_state_dict`` with OpenCLIP keys and HF ``CLIPTextModel`` keys
  (conversion/convert_2.py:37-99 key map).

PyTorch is used for device memory and streams only; every computation is a call into the C ABI.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib


@dataclass(frozen=True)
class TextConfig:
    width: int = 768
    heads: int = 12
    layers: int = 12
    embed_dim: int = 768
    context_length: int = 77
    vocab_size: int = 49408
    quick_gelu: bool = False
    ln_eps: float = 1e-5


# src/open_clip/model_configs/ViT-{L,H,g,bigG}-14.json (text_cfg + embed_dim); the hf-hub ids are the ones the
# reference's launch scripts pass as --model (scripts/train_leaf_vit*.sh)
MODEL_CONFIGS: Dict[str, TextConfig] = {
    "ViT-L-14": TextConfig(768, 12, 12, 768),
    "ViT-L-14-quickgelu": TextConfig(768, 12, 12, 768, quick_gelu=True),
    "ViT-H-14": TextConfig(1024, 16, 24, 1024),
    "ViT-g-14": TextConfig(1024, 16, 24, 1024),
    "ViT-bigG-14": TextConfig(1280, 20, 32, 1280),
    "tiny-test": TextConfig(128, 2, 2, 64),
    "tiny-test-quickgelu": TextConfig(128, 2, 2, 64, quick_gelu=True),
}
_HUB_ALIASES = {
    "hf-hub:chs20/fare2-clip": "ViT-L-14-quickgelu",
    "hf-hub:chs20/tecoa2-clip": "ViT-L-14-quickgelu",
    "hf-hub:laion/CLIP-ViT-H-14-laion2B-s32B-b79K": "ViT-H-14",
    "hf-hub:laion/CLIP-ViT-g-14-laion2B-s12B-b42K": "ViT-g-14",
    "hf-hub:laion/CLIP-ViT-bigG-14-laion2B-39B-b160k": "ViT-bigG-14",
}


def get_config(name: str) -> TextConfig:
    name = _HUB_ALIASES.get(name, name)
    if name not in MODEL_CONFIGS:
        raise KeyError(f"unknown text tower '{name}'; known: {sorted(MODEL_CONFIGS)}")
    return MODEL_CONFIGS[name]


_DTYPES = {"bf16": 0, "fp16": 1}
# arithmetic of the forward-only passes: split masks per leading block (LeafCLIPText.set_split_masks: bit 0 QKV, 1 out_proj weights,
# 2 c_fc, 3 c_proj weights)
PRECISION_MODES = {"rowsafe": (3, 2, 2, 2), "fast": ()}
PRECISION_DEFAULT = "rowsafe"
_OBJ = {"l2": 0, "negl2": 1, "dissim": 2, "sim": 3}


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _host_lens(tokens) -> np.ndarray:
    """kept length per token row, EOT position + 1 (EOT is the largest id); device-resident tokens are copied to the host"""
    arr = tokens if isinstance(tokens, np.ndarray) else tokens.cpu().numpy()
    return arr.reshape(-1, arr.shape[-1]).argmax(-1) + 1


def _lens_cu(lens):
    """(lens int32 [n], cu int32 [n + 1]: cu[i] = rows in front of sequence i) of host lengths, both contiguous"""
    lens = np.ascontiguousarray(np.asarray(lens).reshape(-1), dtype=np.int32)
    cu = np.zeros(lens.size + 1, dtype=np.int32)
    np.cumsum(lens, out=cu[1:])
    return lens, cu


class _RowPlan:
    """Row layout of one pass.  EOT trimming: the host ``lens`` (int32 [n], kept rows per sequence) and, once ``place``d, the device
    ``cu`` (int32 [n + 1], rows in front of each sequence); the dense layout: neither.  The plan owns both arrays, so the C arguments
    ``lens_ptr`` / ``cu_ptr`` stay valid for as long as it is alive."""

    def __init__(self, lens=None):
        self.lens, self._cu_host = _lens_cu(lens) if lens is not None else (None, None)
        self.cu = None

    def place(self, device):
        """``cu`` on the device (pinned + non_blocking: a pageable H2D copy would make the host wait for all queued GPU work)"""
        if self.lens is not None:
            self.cu = torch.from_numpy(self._cu_host).pin_memory().to(device, non_blocking=True)
        return self

    @property
    def lens_ptr(self):
        return C.c_void_p(self.lens.ctypes.data if self.lens is not None else 0)

    @property
    def cu_ptr(self):
        return _ptr(self.cu)

    def rows(self, n: int, ctx: int) -> int:
        return int(self.lens.sum()) if self.lens is not None else n * ctx


@dataclass(frozen=True)
class _TrainPass:
    """What a successful ``forward_train`` leaves for the backward heads: the stash holds the activations of exactly this pass."""
    tokens: torch.Tensor      # int32 [n, ctx] on the device
    plan: _RowPlan
    n: int
    rows: int                 # packed rows: the leading dimension of ``delta`` and of every d_embed
    normalize: bool
    pool_last: bool
    ticket: int               # ``stash_ticket`` of this pass


@dataclass(frozen=True, slots=True)
class _KvCache:
    """The clean captions' per-layer q|k|v rows in one of the model's cache buffers, as ``encode_text_kv`` or ``score_candidates_fused``
    left them.  A later writer of the same slot rewrites those bytes: the cache is then stale, and a pass over it is refused."""
    buf: torch.Tensor         # the slot's byte buffer
    base_cu: torch.Tensor     # int32 [n + 1] on the device: rows in front of each caption
    base_rows: int
    lens: np.ndarray          # host int32 [n]: rows per caption
    n: int
    arith: tuple              # ``arithmetic_tag()`` of the pass that wrote the rows
    q0: bool                  # layer 0 holds the captions' Q rows too: what a single_edit pass reads
    tokens: torch.Tensor      # int32 [n, ctx] on the device
    slot: int
    ticket: int               # ``kv_tickets[slot]`` of the pass that wrote the rows


class _ScoreTarget:
    """What a scoring pass compares its candidates with: one anchor row per caption under an objective, or (``class_feat`` given) a
    class matrix shared by all captions with a label per caption and the wanted extra outputs.  ``bind`` writes it into the C
    arguments of a pass (the target fields of ``leaf_score_args``, include/leaf_hip.h)."""

    def __init__(self, anchor=None, objective="l2", class_feat=None, labels=None, want_pred=False, want_logits=False):
        self.anchor, self.obj = anchor, _OBJ[objective]
        self.class_feat, self.labels, self.want_pred, self.want_logits = class_feat, labels, want_pred, want_logits
        self.B = int((anchor if class_feat is None else labels).shape[0])

    def bind(self, a: _lib.ScoreArgs, rho: int, embed_dim: int, want_features: bool, want_loss: bool):
        """Sets the shape, target and output fields of ``a`` for one pass over B * rho candidates, with fresh output buffers.  Returns
        (those buffers, which must outlive the call; what the scoring call returns)."""
        B, dev = self.B, (self.anchor if self.class_feat is None else self.class_feat).device
        idx = torch.empty(B, dtype=torch.int32, device=dev)
        feat = torch.empty(B, embed_dim, dtype=torch.float32, device=dev) if want_features else None
        a.B, a.rho, a.best_idx, a.best_feat = B, rho, _ptr(idx), _ptr(feat)
        if self.class_feat is None:
            loss = torch.empty(B, rho, dtype=torch.float32, device=dev) if want_loss else None
            a.anchor, a.objective, a.loss = _ptr(self.anchor), self.obj, _ptr(loss)
            return (idx, feat, loss), ((idx, feat, loss) if want_loss else (idx, feat))
        n_cls = int(self.class_feat.shape[0])
        loss = torch.empty(B, rho, dtype=torch.float32, device=dev)          # always: the pass takes best_idx from it
        pred = torch.empty(B, rho, dtype=torch.int32, device=dev) if self.want_pred else None
        logits = torch.empty(B * rho, n_cls, dtype=torch.float32, device=dev) if self.want_logits else None
        a.class_feat, a.C, a.labels, a.loss, a.pred, a.logits = _ptr(self.class_feat), n_cls, _ptr(self.labels), _ptr(loss), _ptr(pred), _ptr(logits)
        return (idx, feat, loss, pred, logits), (idx, feat, (loss if want_loss else None), pred, logits)


@dataclass(slots=True)
class _ScorePlan:
    """What ``score_candidates_prepare`` hands to ``score_candidates_run``: everything of a prefix-reuse pass but the prefix lengths.
    ``args`` holds addresses only: the plan keeps alive every buffer behind them (``tokens``, ``cache``, ``target``, ``keep``; the
    weights are the model's)."""
    full: np.ndarray          # host int32 [n]: the candidates' full lengths
    limit: np.ndarray         # ``_prefix_limit`` of them
    host: torch.Tensor        # pinned int32 [cu (n + 1) | prefix (n)], staged for one host-to-device copy
    tokens: torch.Tensor      # the candidates, int32 [n, ctx] on the device
    rho: int
    cache: _KvCache
    single_edit: bool
    target: _ScoreTarget
    keep: tuple               # the pass's workspace and output buffers
    ret: tuple                # what the scoring call returns
    args: _lib.ScoreArgs      # the C arguments, all but seq_lens / cu_rows / prefix / stream


def _prefix_limit(full, base_lens, rho: int) -> np.ndarray:
    """int32 [n]: the longest prefix candidate ``i`` (``full[i]`` rows) may take from the cache of caption ``i // rho`` -- its own EOT
    row is always computed, and no more rows are read than the caption's cache holds"""
    return np.minimum(np.asarray(full, dtype=np.int32) - 1, np.repeat(np.asarray(base_lens, dtype=np.int32), rho))


def _clamp_prefix(prefix_lens, limit, out) -> np.ndarray:
    """``prefix_lens`` clamped to ``limit`` (``_prefix_limit``) into the int32 array ``out``"""
    return np.minimum(np.asarray(prefix_lens).reshape(-1), limit, out=out, casting="unsafe")


def _check_equal_lengths(full, base_lens, rho: int) -> None:
    """the length half of the ``single_edit`` promise: candidate ``i`` is as long as caption ``i // rho``"""
    full, want = np.asarray(full).reshape(-1), np.repeat(np.asarray(base_lens).reshape(-1), rho)
    if (full != want).any():
        i = int((full != want).argmax())
        raise ValueError(f"single_edit: candidate {i} has length {int(full[i])}, its caption {int(want[i])}")


def verify_single_edit(cand_tokens, cand_lens, prefix, base_tokens, base_lens, rho: int) -> None:
    """The promise of a ``single_edit`` scoring pass, checked on the tokens (``LEAF_VERIFY_SINGLE_EDIT=1``; tests and debugging: the
    comparison needs the tokens on the host): candidate ``i`` belongs to caption ``i // rho``, has the caption's length, and differs
    from it at position ``prefix[i]`` at most -- every kept position in front of it AND behind it carries the caption's token.
    Raises ``ValueError`` naming the first offender.  Arrays or tensors; works without a GPU."""
    def host(x):
        return np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)
    cand, base = host(cand_tokens), host(base_tokens)
    cand = cand.reshape(-1, cand.shape[-1])
    base = base.reshape(-1, base.shape[-1])
    n, ctx = cand.shape
    if n != base.shape[0] * rho:
        raise ValueError(f"single_edit: {n} candidates for {base.shape[0]} captions x rho = {rho}")
    cl = host(cand_lens).reshape(-1).astype(np.int64)
    pfx = host(prefix).reshape(-1).astype(np.int64)
    _check_equal_lengths(cl, host(base_lens), rho)
    pos = np.arange(ctx)[None, :]
    differs = (cand != np.repeat(base, rho, axis=0)) & (pos < cl[:, None]) & (pos != pfx[:, None])
    bad = np.nonzero(differs.any(-1))[0]
    if bad.size:
        i = int(bad[0])
        j = int(differs[i].argmax())
        raise ValueError(f"single_edit: candidate {i} differs from its caption at position {j}, not only at its prefix length {int(pfx[i])}")


class LeafCLIPText:
    """Text tower on the HIP engine.  Not an ``nn.Module``: parameters live in ``self.flat`` (fp32, CUDA);
    ``self.params[name]`` are views into it with the OpenCLIP names."""

    def __init__(self, cfg: TextConfig, device="cuda:0", dtype: str = None, chunk: int = None, trainable: bool = False):
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.LeafHipError("LeafCLIPText needs a CUDA(HIP) device; there is no CPU path")
        dtype = dtype or os.environ.get("LEAF_DTYPE", "fp16")
        self.dtype_name = dtype
        self._lib = _lib.lib()
        c = _lib.TextCfgC(cfg.layers, cfg.width, cfg.heads, cfg.embed_dim, cfg.context_length, cfg.vocab_size,
                          1 if cfg.quick_gelu else 0, cfg.ln_eps)
        h = C.c_void_p()
        _lib.check(self._lib.leaf_text_create(C.byref(c), _DTYPES[dtype], C.byref(h)), "leaf_text_create")
        self._h = h
        self.set_option("chunk", chunk or int(os.environ.get("LEAF_CHUNK", "4096")))   # sequences-worth of rows per pass (x 77 rows)
        self.n_params = self._lib.leaf_text_param_count(h)
        self.n_decay = self._lib.leaf_text_decay_count(h)
        with torch.cuda.device(self.device):
            self.flat = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
            self.w16 = torch.empty(self._lib.leaf_text_w16_bytes(h), dtype=torch.uint8, device=self.device)
        self.layout: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        self.params: Dict[str, torch.Tensor] = {}
        name = C.create_string_buffer(128)
        off, rows, cols = C.c_size_t(), C.c_int64(), C.c_int64()
        for i in range(self._lib.leaf_text_num_tensors(h)):
            _lib.check(self._lib.leaf_text_param_info(h, i, name, 128, C.byref(off), C.byref(rows), C.byref(cols)), "param_info")
            shape = (rows.value, cols.value) if cols.value else (rows.value,)
            self.layout[name.value.decode()] = (off.value, shape)
            self.params[name.value.decode()] = self.flat[off.value: off.value + int(np.prod(shape))].view(shape)
        self.logit_scale = torch.tensor(math.log(1 / 0.07), device=self.device)  # carried for checkpoints only
        # tensors of a loaded checkpoint outside the text tower (visual.*, ...): kept on the host and written back by
        # state_dict(), so that epoch_latest.pt stays a FULL CLIP state_dict the reference's --resume / converters can load
        self.extra_state: Dict[str, torch.Tensor] = {}
        self._buf: Dict[object, torch.Tensor] = {}      # device byte buffers that grow on demand (_grow): workspaces, K/V slots, stash
        self._packed = False
        # exact work skipping: compute only rows up to EOT (include/leaf_hip.h, "EOT trimming"); LEAF_PACK=0 disables
        self.trim_rows = os.environ.get("LEAF_PACK", "1") != "0"
        self.training = False
        self.precise_encode = False   # encode_text's default for ``precise``
        self._vocab_inv = None        # nn_project's inverse row norms of the token table, per weight version
        self.split_masks = ()
        self._split_buf = None
        # training state (allocated by enable_training)
        self.grads = self.exp_avg = self.exp_avg_sq = self.w16_bwd = self._clip_ws = self._clipi_ws = None
        self._scaler_attached = False
        self.opt_step = 0
        self.stash_ticket = 0     # bumped by every successful forward_train: names the forward whose activations the stash holds
        self.train_pass: Optional[_TrainPass] = None      # that forward (None: the stash holds nothing a backward may read)
        self.kv_tickets: Dict[int, int] = {}      # per K/V cache slot: bumped by every pass that has rewritten the slot (_kv_cache)
        self.rows_scored = 0      # packed rows handed to the scoring passes so far (host-side count; bench.py reports it per rank)
        if trainable:
            self.enable_training()
        # default arithmetic of the forward-only passes: LEAF_PRECISION=rowsafe (default) | fast
        mode = os.environ.get("LEAF_PRECISION", PRECISION_DEFAULT)
        if mode not in PRECISION_MODES:
            raise ValueError(f"LEAF_PRECISION={mode}: one of {sorted(PRECISION_MODES)}")
        if PRECISION_MODES[mode] and self._lib.leaf_text_get_option(self._h, b"ln_fold"):
            self.set_precision(mode)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.leaf_text_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_option(self, name: str, value: int):
        """Engine switches (leaf_text_set_option): 'chunk', 'last_layer_trim', 'normalize_fare' (training forward / backward on normalised features),
        'compact_resid' (1 default: the residual stream of the forward-only passes as the 16-bit copy + an 8-bit remainder per
        element instead of fp32 rows; 0 = fp32 rows), 'single_edit' (set per pass by the ``single_edit=`` argument of the scoring calls)."""
        if name == "ln_fold" and not value and self.split_masks:
            self.set_split_masks(())          # the split GEMMs exist in the LN-folded forward only: switching folding off switches them off
        _lib.check(self._lib.leaf_text_set_option(self._h, name.encode(), int(value)), "leaf_text_set_option")
        return self

    def _single_edit_call(self, on: bool, fn, promise):
        """``fn()`` with the engine's per-pass ``single_edit`` option set for its duration.  ``promise``: the arguments of
        ``verify_single_edit``, checked first under ``LEAF_VERIFY_SINGLE_EDIT=1``."""
        if not on:
            return fn()
        if os.environ.get("LEAF_VERIFY_SINGLE_EDIT") == "1":
            verify_single_edit(*promise)
        self.set_option("single_edit", 1)
        try:
            return fn()
        finally:
            self.set_option("single_edit", 0)

    # ------------------------------------------------------------------ nn.Module look-alikes
    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        self.training = mode
        return self

    def named_parameters(self):
        return list(self.params.items())

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _grow(self, key, need: int) -> torch.Tensor:
        """the device byte buffer ``key``, allocated anew when it holds fewer than ``need`` bytes (the old one is dropped first)"""
        buf = self._buf.get(key)
        if buf is None or buf.numel() < need:
            buf = self._buf[key] = None
            with torch.cuda.device(self.device):
                buf = self._buf[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return buf

    def _workspace(self, mode: int, n_seq: int) -> torch.Tensor:
        return self._grow(("ws", mode), self._lib.leaf_text_workspace_bytes(self._h, n_seq, mode))

    def _kv_buffer(self, slot: int, rows: int) -> torch.Tensor:
        """cache buffer ``slot`` for the per-layer 16-bit q|k|v rows of ``rows`` caption rows"""
        return self._grow(("kv", slot), max(rows * 3 * self.cfg.width * 2 * self.cfg.layers, 1))

    # ------------------------------------------------------------------ weights
    def init_random(self, seed: int = 1):
        """Same generator and distributions as oracle.text_oracle.init_weights (numpy PCG64), restated here so
        the product does not import the oracle: transformer.py:731-752 std's, perturbed LN affine / biases."""
        cfg = self.cfg
        rng = np.random.default_rng(seed)
        d, L, D = cfg.width, cfg.layers, cfg.embed_dim
        n = lambda shape, std: (rng.standard_normal(shape, dtype=np.float32) * np.float32(std)).astype(np.float32)
        sd = {"token_embedding.weight": n((cfg.vocab_size, d), 0.02), "positional_embedding": n((cfg.context_length, d), 0.01)}
        proj_std, attn_std, fc_std = (d ** -0.5) * ((2 * L) ** -0.5), d ** -0.5, (2 * d) ** -0.5
        for i in range(L):
            p = f"transformer.resblocks.{i}."
            sd[p + "ln_1.weight"] = (1.0 + n((d,), 0.05)).astype(np.float32)
            sd[p + "ln_1.bias"] = n((d,), 0.02)
            sd[p + "attn.in_proj_weight"] = n((3 * d, d), attn_std)
            sd[p + "attn.in_proj_bias"] = n((3 * d,), 0.02)
            sd[p + "attn.out_proj.weight"] = n((d, d), proj_std)
            sd[p + "attn.out_proj.bias"] = n((d,), 0.02)
            sd[p + "ln_2.weight"] = (1.0 + n((d,), 0.05)).astype(np.float32)
            sd[p + "ln_2.bias"] = n((d,), 0.02)
            sd[p + "mlp.c_fc.weight"] = n((4 * d, d), fc_std)
            sd[p + "mlp.c_fc.bias"] = n((4 * d,), 0.02)
            sd[p + "mlp.c_proj.weight"] = n((d, 4 * d), proj_std)
            sd[p + "mlp.c_proj.bias"] = n((d,), 0.02)
        sd["ln_final.weight"] = (1.0 + n((d,), 0.05)).astype(np.float32)
        sd["ln_final.bias"] = n((d,), 0.02)
        sd["text_projection"] = n((d, D), d ** -0.5)
        self.load_state_dict(sd)
        return self

    def load_state_dict(self, sd, strict: bool = True):
        """OpenCLIP text-tower keys (a full CLIP state_dict is accepted: visual.* is ignored, 'module.' stripped,
        factory.py:138-139) or HF CLIPTextModel / CLIPModel keys (conversion/convert_to_openclip.py:78-121)."""
        from .checkpoint import non_text_tensors, to_openclip_text_keys
        extra = non_text_tensors(sd)
        if extra:
            self.extra_state = extra
        sd = to_openclip_text_keys(sd, self.cfg)
        missing = [k for k in self.params if k not in sd]
        if missing and strict:
            raise KeyError(f"missing text-tower keys: {missing[:5]}{'...' if len(missing) > 5 else ''}")
        for k, p in self.params.items():
            if k in sd:
                v = sd[k]
                v = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
                if tuple(v.shape) != tuple(p.shape):
                    raise ValueError(f"{k}: shape {tuple(v.shape)} != {tuple(p.shape)}")
                p.copy_(v.to(device=self.device, dtype=torch.float32))
        if "logit_scale" in sd:
            self.logit_scale = torch.as_tensor(sd["logit_scale"], dtype=torch.float32).to(self.device)
        self._packed = False
        self._vocab_inv = None
        return self

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """OpenCLIP keys: the text tower (device tensors), ``logit_scale`` and every non-text tensor of the checkpoint this
        model was loaded from (``visual.*`` etc., host tensors) -- a full CLIP ``state_dict`` when it started from one."""
        out = {k: v.detach().clone() for k, v in self.params.items()}
        out["logit_scale"] = self.logit_scale.detach().clone()
        out.update(self.extra_state)
        return out

    def set_split_masks(self, masks):
        """Higher-precision GEMMs in the leading blocks of the forward-only passes (include/leaf_hip.h, leaf_text_split_pack_masks):
        ``masks[l]`` says which GEMMs of block l multiply hi + lo 16-bit splits (more MFMA passes through the unchanged kernels):
        bit 0 = QKV (both operands), 1 = out_proj (weights), 2 = c_fc (both operands), 3 = c_proj (weights).  ``PRECISION_MODES``
        names the lists that matter: 'rowsafe' (the DEFAULT: every one of the census's 12,928 ViT-L search rows within 1e-3 of the
        fp32 reference, profiles/r06_row_error_census*.txt) and 'fast' (no split: rounds 1-5, batch 8.7e-4, 1.1 % of the rows above
        1e-3).  ``pack()`` refreshes the split weight copies after every optimizer step."""
        masks = [int(x) for x in masks]
        while masks and masks[-1] == 0:
            masks.pop()
        if len(masks) > self.cfg.layers - 1 or any(x < 0 or x > 15 for x in masks):
            raise ValueError(f"split masks {masks}: at most {self.cfg.layers - 1} blocks, values 0..15")
        self.split_masks = tuple(masks)
        self._split_buf = None
        if masks:
            with torch.cuda.device(self.device):
                self._split_buf = torch.empty(self._lib.leaf_text_split_bytes(self._h, len(masks)), dtype=torch.uint8, device=self.device)
        self._split_pack()
        return self

    def set_split_blocks(self, blocks: int):
        """All four GEMMs of the first ``blocks`` blocks on splits (rounds 4-5's escape hatch; 0 = none): ``set_split_masks([15] * blocks)``."""
        blocks = int(blocks)
        if blocks < 0 or blocks > self.cfg.layers - 1:
            raise ValueError(f"split blocks {blocks} out of range 0..{self.cfg.layers - 1}")
        return self.set_split_masks([15] * blocks)

    @property
    def split_blocks(self) -> int:
        return len(self.split_masks)

    def set_precision(self, mode: str):
        """'rowsafe' (default) | 'fast' (no split GEMMs: the round-5 arithmetic) -- see ``set_split_masks``."""
        if mode not in PRECISION_MODES:
            raise ValueError(f"precision mode '{mode}': one of {sorted(PRECISION_MODES)}")
        return self.set_split_masks(PRECISION_MODES[mode][:self.cfg.layers - 1])

    def precision_name(self) -> str:
        for k, v in PRECISION_MODES.items():
            vv = list(v[:self.cfg.layers - 1])
            while vv and vv[-1] == 0:
                vv.pop()
            if tuple(vv) == tuple(self.split_masks):
                return k
        return "masks" + "-".join(str(x) for x in self.split_masks)

    def arithmetic_tag(self):
        """What a K/V cache depends on besides the weights: a cache built under one setting must not be consumed under another
        (the bit-exact prefix reuse would silently break): (compact_resid, split masks, ln_fold)."""
        return (int(self._lib.leaf_text_get_option(self._h, b"compact_resid")), tuple(self.split_masks),
                int(self._lib.leaf_text_get_option(self._h, b"ln_fold")))

    def _split_pack(self):
        masks = self.split_masks
        arr = (C.c_int32 * max(len(masks), 1))(*masks)
        _lib.check(self._lib.leaf_text_split_pack_masks(self._h, _ptr(self.flat), arr, len(masks), _ptr(self._split_buf),
                                                        self._stream()), "leaf_text_split_pack_masks")

    def copy_from(self, other: "LeafCLIPText"):
        """Weights AND arithmetic of ``other`` (split blocks / policy, residual-stream format): a frozen copy must embed like its source."""
        self.flat.copy_(other.flat)
        if tuple(other.split_masks) != tuple(self.split_masks):
            self.set_split_masks(other.split_masks)
        self.set_option("compact_resid", other.arithmetic_tag()[0])
        self.logit_scale = other.logit_scale.clone()
        self.extra_state = dict(other.extra_state)
        self._packed = False
        self._vocab_inv = None
        return self

    def _weights(self):
        """the C arguments (fp32 masters, 16-bit operand copies) of a pass, the copies packed first when they are out of date"""
        if not self._packed:
            self.pack()
        return _ptr(self.flat), _ptr(self.w16)

    def pack(self):
        """fp32 masters -> 16-bit MFMA operand copies (forward dtype; + transposed bf16 when training)."""
        _lib.check(self._lib.leaf_text_pack_weights(self._h, _ptr(self.flat), _ptr(self.w16), _ptr(self.w16_bwd),
                                                    self._stream()), "leaf_text_pack_weights")
        if self.split_masks:
            self._split_pack()
        self._packed = True

    # ------------------------------------------------------------------ inference
    def _tokens(self, text) -> torch.Tensor:
        if isinstance(text, np.ndarray):
            text = torch.from_numpy(text)
        t = text.to(device=self.device, dtype=torch.int32, non_blocking=True).contiguous()
        if t.dim() != 2 or t.shape[1] != self.cfg.context_length:
            raise ValueError(f"tokens must be [N,{self.cfg.context_length}], got {tuple(t.shape)}")
        return t

    def _row_plan(self, text, seq_lens, place: bool = True) -> _RowPlan:
        """The row layout of a pass over ``text``: EOT trimming with lengths from the caller (host array) or, for host-resident tokens,
        from argmax(tokens) + 1; the dense layout when trimming is off or the tokens live on the device (lengths unknown on the
        host).  ``place=False`` leaves the device copy of ``cu`` to the caller (``_RowPlan.place``)."""
        host = isinstance(text, np.ndarray) or (isinstance(text, torch.Tensor) and text.device.type == "cpu")
        if self.trim_rows and seq_lens is None and host:
            seq_lens = _host_lens(text)
        plan = _RowPlan(seq_lens if self.trim_rows else None)
        return plan.place(self.device) if place else plan

    def encode_text(self, text, normalize: bool = False, seq_lens=None, precise: Optional[bool] = None) -> torch.Tensor:
        """``precise`` (default: the model's ``precise_encode`` attribute, False): the fp32-grade forward of precise.hip -- fp32 stored
        intermediates, fp32 master weights through three MFMA passes of fp16 hi / lo splits -- for embeddings that leave the engine
        (export, eval_textfare) or the frozen model's anchors; ~1e-6 of the fp32 reference per row instead of ~9e-4, about 8x the
        time per row.  The search's scoring passes always run the 16-bit arithmetic."""
        if len(text) == 0:      # an empty batch encodes to an empty [0, embed_dim] tensor, as the torch module's (model.py:269-284)
            return torch.empty(0, self.cfg.embed_dim, dtype=torch.float32, device=self.device)
        if precise is None:
            precise = self.precise_encode
        plan = self._row_plan(text, seq_lens)
        t = self._tokens(text)
        n = t.shape[0]
        out = torch.empty(n, self.cfg.embed_dim, dtype=torch.float32, device=self.device)
        if precise:     # the fp32 masters alone, a workspace of its own
            entry, weights = "leaf_text_forward_precise", (_ptr(self.flat),)
            ws = self._grow(("ws", "precise"), self._lib.leaf_text_precise_workspace_bytes(self._h, n))
        else:
            entry, weights = "leaf_text_forward", self._weights()
            ws = self._workspace(0, n)
        _lib.check(getattr(self._lib, entry)(self._h, *weights, _ptr(t), plan.lens_ptr, plan.cu_ptr, n, _ptr(out), int(bool(normalize)),
                                             _ptr(ws), ws.numel(), self._stream()), entry)
        return out

    def hidden_taps(self, layers=(-1,), final_ln=True):
        """[(layer, final_ln)] of ``encode_text_hidden``'s arguments, ``layer`` in HF's ``hidden_states`` index 0..cfg.layers: negative
        indices count from the end of that tuple (-1 = cfg.layers, -2 = cfg.layers - 1); ``final_ln`` a bool or one per layer."""
        layers = [int(l) for l in layers]
        lns = [bool(final_ln)] * len(layers) if isinstance(final_ln, (bool, int)) else [bool(x) for x in final_ln]
        if len(lns) != len(layers):
            raise ValueError(f"final_ln: {len(lns)} values for {len(layers)} layers")
        n = self.cfg.layers + 1
        if any(l < -n or l >= n for l in layers):
            raise ValueError(f"layers {layers}: hidden_states has {n} entries (0 = embedding .. {n - 1} = last block)")
        return [(l + n if l < 0 else l, ln) for l, ln in zip(layers, lns)]

    def encode_text_hidden(self, text, layers=(-1,), final_ln=True, seq_lens="dense", precise: Optional[bool] = None,
                           dtype: torch.dtype = torch.float32, want_features: bool = False, normalize: bool = False):
        """Per-token hidden states (include/leaf_hip.h, leaf_text_forward_hidden): a list with one ``[N, ctx, width]`` tensor per
        entry of ``layers``, in HF ``CLIPTextModel``'s ``hidden_states`` index (0 = token + positional embedding, l = output of block
        l - 1; negative indices from the end: -1 = the last block, -2 = the one before).  ``final_ln`` (a bool, or one per layer)
        applies ``ln_final`` to every row: ``last_hidden_state`` is ``layers=(-1,), final_ln=True`` (SD 1.x), SDXL's
        ``hidden_states[-2]`` is ``layers=(-2,), final_ln=False``, SD 2.x / clip_skip is ``(-2,)`` with ``final_ln=True``.
        ``dtype``: ``torch.float32`` or the model's 16-bit type (the rounded fp32 value).  ``want_features``: also return the
        ``[N, embed_dim]`` features of the same pass (``encode_text``'s bits): ``(states, features)``.

        ROWS.  ``seq_lens="dense"`` (the default) computes all ctx rows of every sequence, whatever the tokens' device: a diffusion
        pipeline cross-attends to the padded positions too (HF pads with the EOT id), so the rows behind the EOT are part of the
        result.  EOT trimming is OPT-IN here, unlike in ``encode_text``: ``seq_lens=None`` (lengths from host-resident tokens, as
        ``encode_text``; device-resident tokens still run dense) or an array of lengths runs packed rows, and every row at a position
        >= the sequence's length comes back ZERO.  Rows in front of the EOT are bit-identical either way.
        ``precise``: as ``encode_text`` (fp32 states only)."""
        taps = self.hidden_taps(layers, final_ln)
        if precise is None:
            precise = self.precise_encode
        half = torch.float16 if self.dtype_name == "fp16" else torch.bfloat16
        if dtype not in (torch.float32, half):
            raise ValueError(f"dtype {dtype}: torch.float32 or the model's 16-bit type {half}")
        if precise and dtype != torch.float32:
            raise ValueError("precise=True returns fp32 states")
        cfg = self.cfg
        n = len(text)
        with torch.cuda.device(self.device):
            outs = [torch.empty(n, cfg.context_length, cfg.width, dtype=dtype, device=self.device) for _ in taps]
            feat = torch.empty(n, cfg.embed_dim, dtype=torch.float32, device=self.device) if want_features else None
        if n == 0:
            return (outs, feat) if want_features else outs
        plan = _RowPlan() if isinstance(seq_lens, str) and seq_lens == "dense" else self._row_plan(text, seq_lens)
        t = self._tokens(text)
        arr = (_lib.HiddenTap * max(len(taps), 1))(*[_lib.HiddenTap(l, int(ln), o.data_ptr()) for (l, ln), o in zip(taps, outs)])
        if precise:
            params, w16 = _ptr(self.flat), None
            ws = self._grow(("ws", "precise"), self._lib.leaf_text_precise_workspace_bytes(self._h, n))
        else:
            params, w16 = self._weights()
            ws = self._workspace(0, n)
        a = _lib.HiddenArgs(params=params, w16_fwd=w16, tokens=_ptr(t), seq_lens=plan.lens_ptr, cu_rows=plan.cu_ptr, n_seq=n,
                            taps=C.addressof(arr), n_taps=len(taps), out_dtype=int(dtype != torch.float32), feat=_ptr(feat),
                            normalize=int(bool(normalize)), precise=int(bool(precise)), ws=_ptr(ws), ws_bytes=ws.numel(), stream=self._stream())
        _lib.check(self._lib.leaf_text_forward_hidden(self._h, a), "leaf_text_forward_hidden")
        return (outs, feat) if want_features else outs

    def encode_text_kv(self, text, seq_lens=None, want_features: bool = False, slot: int = 0):
        """Forward of the clean captions that keeps every layer's q|k|v rows for prefix reuse by the search
        (include/leaf_hip.h, "prefix reuse").  Returns the cache, a ``_KvCache`` (and the features when asked).  ``slot``: which of the
        model's cache buffers to fill -- caches of different slots can be alive at the same time (the string search pipelines
        groups of captions, leaf_amd/attacks.py); filling a slot makes every earlier cache of that slot stale."""
        plan = _RowPlan(_host_lens(text) if seq_lens is None else seq_lens).place(self.device)
        t = self._tokens(text)
        n = t.shape[0]
        rows = plan.rows(n, self.cfg.context_length)
        kvbuf = self._kv_buffer(slot, rows)
        out = torch.empty(n, self.cfg.embed_dim, dtype=torch.float32, device=self.device) if want_features else None
        ws = self._workspace(0, n)
        _lib.check(self._lib.leaf_text_forward_kv(self._h, *self._weights(), _ptr(t), plan.lens_ptr, plan.cu_ptr, n,
                                                  _ptr(out), 0, _ptr(kvbuf), kvbuf.numel(), _ptr(ws), ws.numel(), self._stream()),
                   "leaf_text_forward_kv")
        # q0: layer 0 holds the captions' Q rows too (this pass writes whole q|k|v rows) -- what a single_edit pass reads
        cache = self._kv_cache(kvbuf, plan.cu, rows, plan.lens, True, t, slot)
        return (cache, out) if want_features else cache

    def _kv_cache(self, buf, base_cu, base_rows: int, lens, q0: bool, tokens, slot: int) -> _KvCache:
        """The record of the rows that a C call, which has returned success, wrote into cache buffer ``slot``: the slot's ticket moves
        on, so every earlier cache of the slot is stale from here."""
        self.kv_tickets[slot] = ticket = self.kv_tickets.get(slot, 0) + 1
        return _KvCache(buf, base_cu, base_rows, lens, int(tokens.shape[0]), self.arithmetic_tag(), q0, tokens, slot, ticket)

    def _check_cache(self, cache: _KvCache, B: int, rho: int, full, single_edit: bool) -> None:
        """Refuses a pass of B * rho candidates (lengths ``full``) over ``cache`` unless it holds the rows of B captions, written under
        the arithmetic the model runs now and not rewritten since."""
        if cache.n != B or full.size != B * rho:
            raise ValueError("candidate rows / kv cache do not match B*rho")
        if cache.arith != self.arithmetic_tag():
            raise ValueError(f"K/V cache built under arithmetic {cache.arith} (compact_resid, split masks, ln_fold), "
                             f"the model now runs {self.arithmetic_tag()}: rebuild the cache (encode_text_kv)")
        if cache.ticket != self.kv_tickets.get(cache.slot):
            raise RuntimeError(f"stale K/V cache: ticket {cache.ticket} of slot {cache.slot} (current {self.kv_tickets.get(cache.slot)}): the "
                               "slot was rewritten since; rebuild the cache (encode_text_kv / score_candidates_fused)")
        if single_edit:
            # the pass reads the captions' Q rows of layer 0 and, behind the edit, as many cache rows as the candidate is long
            if not cache.q0:
                raise ValueError("single_edit pass on a K/V cache without the captions' layer-0 Q rows (written by a fused first stage "
                                 "that did not run with single_edit): rebuild it with encode_text_kv or score_candidates_fused(single_edit=True)")
            _check_equal_lengths(full, cache.lens, rho)

    def score_candidates(self, tokens, anchor: torch.Tensor, rho: int, objective: str = "l2", want_features=True,
                         want_loss=False, seq_lens=None, prefix_lens=None, kv=None, single_edit: bool = False):
        """tokens [B*rho, ctx] (or [B,rho,ctx]); anchor [B,D] fp32 CUDA.  Returns (best_idx int32[B],
        best_feat [B,D] or None) (+ loss [B,rho] when want_loss).

        ``prefix_lens`` (host int array [B*rho], number of leading positions equal to the clean caption) together
        with ``kv`` (from ``encode_text_kv`` of the clean captions) enables prefix reuse: only positions from the
        first changed token on are recomputed.  ``seq_lens`` must then be the candidates' full lengths.

        ``single_edit`` (with prefix reuse only; off by default): the caller promises that every candidate is its caption with ONE
        token replaced, at position ``prefix_lens[i]`` -- equal lengths, equal tokens behind that position.  Block 0 then projects
        one q|k|v row per candidate instead of all of its rows (include/leaf_hip.h, "single-edit passes"); same bits.  Meant for
        token-level substitutions (``leaf_amd.step.search_synthetic``); NOT for the string search of ``leaf_amd.attacks`` /
        ``charmer``, where a character edit re-tokenises the rest of the caption.  ``LEAF_VERIFY_SINGLE_EDIT=1`` checks the promise
        against the tokens (a device-to-host copy)."""
        return self._score(self._anchor_target(anchor, objective), tokens, rho, want_features, want_loss, seq_lens, prefix_lens, kv, single_edit)

    def _anchor_target(self, anchor, objective):
        return _ScoreTarget(anchor.to(device=self.device, dtype=torch.float32).contiguous(), objective)

    def _score(self, target, tokens, rho, want_features, want_loss, seq_lens, prefix_lens, kv, single_edit=False):
        """one scoring pass against ``target``: prefix reuse when the caller gives prefix lengths and a cache, else all kept rows"""
        if prefix_lens is not None and kv is not None and self.trim_rows:
            return self.score_candidates_run(self._prepare(target, tokens, rho, want_features, want_loss, seq_lens, kv, single_edit), prefix_lens)
        return self._score_dense(target, tokens, rho, want_features, want_loss, seq_lens)

    def _candidates(self, tokens, B: int, rho: int = 1) -> torch.Tensor:
        """the rho candidates of each of B captions ([B * rho, ctx] or [B, rho, ctx]; rho = 1: the captions themselves) on the device,
        as int32 [B * rho, ctx]"""
        t = self._tokens(tokens.reshape(-1, tokens.shape[-1]))
        if t.shape[0] != B * rho:
            raise ValueError(f"{t.shape[0]} token rows != B*rho = {B}*{rho}")
        return t

    def _score_args(self, target, t, rho, want_features, want_loss, **mode):
        """(the C arguments of a scoring pass over the candidates ``t`` against ``target``: the fields that every pass sets and
        ``mode``, those of its row mode; the workspace and output buffers behind them, to be kept until the call has returned; what
        the pass returns)"""
        ws = self._workspace(1, t.shape[0])
        params, w16 = self._weights()
        a = _lib.ScoreArgs(params=params, w16_fwd=w16, tokens=_ptr(t), ws=_ptr(ws), ws_bytes=ws.numel(), **mode)
        outs, ret = target.bind(a, rho, self.cfg.embed_dim, want_features, want_loss)
        return a, (ws, *outs), ret

    def _score_pass(self, a: _lib.ScoreArgs) -> int:
        """the C call of a scoring pass on the current stream; returns 2 when the rows of a fused first stage do not fit one chunk"""
        a.stream = self._stream()
        rc = self._lib.leaf_score_pass(self._h, a)
        return rc if rc == 2 and a.kv_write else _lib.check(rc, "leaf_score_pass")

    def _score_dense(self, target, tokens, rho, want_features, want_loss, seq_lens):
        """one pass over all kept rows of the B * rho candidates, scored against ``target``"""
        plan = self._row_plan(tokens, seq_lens)
        t = self._candidates(tokens, target.B, rho)
        a, keep, ret = self._score_args(target, t, rho, want_features, want_loss, seq_lens=plan.lens_ptr, cu_rows=plan.cu_ptr)
        self.rows_scored += plan.rows(t.shape[0], self.cfg.context_length)
        self._score_pass(a)
        return ret

    def score_candidates_prepare(self, tokens, anchor, rho, objective="l2", want_features=True, want_loss=False, seq_lens=None, kv=None,
                                 single_edit: bool = False) -> _ScorePlan:
        """Everything of a prefix-reuse ``score_candidates`` call that does NOT depend on the prefix lengths: the check of the cache,
        token / anchor placement, output buffers, the length limits, a pinned staging buffer for the row plan, the C arguments
        known by now.  The search calls this BEFORE it waits for the previous stage's winners and
        ``score_candidates_run(plan, prefix_lens)`` right after them: the device idles at that boundary for as long as the host needs
        between the two (round 4, tools/stage_hole_probe.py: 270 -> 94 us at ViT-L B = 128, 181 -> 123 us at ViT-H B = 32)."""
        return self._prepare(self._anchor_target(anchor, objective), tokens, rho, want_features, want_loss, seq_lens, kv, single_edit)

    def _prepare(self, target, tokens, rho, want_features, want_loss, seq_lens, kv: _KvCache, single_edit) -> _ScorePlan:
        full = np.ascontiguousarray(np.asarray(_host_lens(tokens) if seq_lens is None else seq_lens).reshape(-1), dtype=np.int32)
        self._check_cache(kv, target.B, rho, full, single_edit)
        host = torch.zeros(2 * full.size + 1, dtype=torch.int32, pin_memory=True)      # [cu (n + 1), cu[0] = 0 | prefix (n)]
        t = self._candidates(tokens, target.B, rho)
        a, keep, ret = self._score_args(target, t, rho, want_features, want_loss, base_cu=_ptr(kv.base_cu), kv=_ptr(kv.buf),
                                        base_rows=kv.base_rows, max_len=int(full.max()))
        return _ScorePlan(full, _prefix_limit(full, kv.lens, rho), host, t, rho, kv, bool(single_edit), target, keep, ret, a)

    def score_candidates_run(self, plan: _ScorePlan, prefix_lens):
        """The prefix-dependent rest of ``score_candidates_prepare``: row plan (suffix rows per candidate, their running sum), one
        host-to-device copy, the launches.  Returns what ``score_candidates`` (``score_candidates_cls``) returns."""
        full, n, cache = plan.full, plan.full.size, plan.cache
        hv = plan.host.numpy()
        pfx = _clamp_prefix(prefix_lens, plan.limit, hv[n + 1:])
        suf = full - pfx                                                       # rows to compute per candidate (int32, contiguous)
        np.cumsum(suf, out=hv[1:n + 1])
        dev = plan.host.to(self.device, non_blocking=True)
        self.rows_scored += int(hv[n])
        a = plan.args
        a.seq_lens, a.cu_rows, a.prefix = suf.ctypes.data, dev.data_ptr(), dev.data_ptr() + 4 * (n + 1)      # dev: [cu (n + 1) | prefix (n)]
        self._single_edit_call(plan.single_edit, lambda: self._score_pass(a), (plan.tokens, full, pfx, cache.tokens, cache.lens, plan.rho))
        return plan.ret

    # ------------------------------------------------------------------ classification scoring (classify.hip)
    def _cls_target(self, class_features, labels, want_pred, want_logits):
        """the class matrix and labels of a ``score_candidates_cls`` call on the device, checked on the host: embed_dim columns, every
        label in [0, C) (the kernel cannot report a bad label; the engine itself refuses a class count outside 2 .. 1,024)"""
        cf = class_features.to(device=self.device, dtype=torch.float32).contiguous()
        if cf.dim() != 2 or cf.shape[1] != self.cfg.embed_dim:
            raise ValueError(f"class_features must be [C, {self.cfg.embed_dim}], got {tuple(cf.shape)}")
        n_cls = int(cf.shape[0])
        lab = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        lab = np.ascontiguousarray(lab.reshape(-1), dtype=np.int64)
        if lab.size and (lab.min() < 0 or lab.max() >= n_cls):
            raise ValueError(f"label outside [0, {n_cls}): {lab[(lab < 0) | (lab >= n_cls)][:4].tolist()}")
        lab_dev = torch.from_numpy(lab.astype(np.int32)).pin_memory().to(self.device, non_blocking=True)
        return _ScoreTarget(class_feat=cf, labels=lab_dev, want_pred=want_pred, want_logits=want_logits)

    def score_candidates_cls(self, tokens, class_features: torch.Tensor, labels, rho: int, want_features=False, want_loss=True,
                             want_pred=True, want_logits=False, seq_lens=None, prefix_lens=None, kv=None):
        """The pass of ``score_candidates`` scored against a class matrix shared by all captions (leaf_score_pass with a class target,
        leaf_amd/csrc/classify.hip; the objective of the reference's attack_text_charmer_classification): the candidates' features are
        L2-normalised, ``class_features`` [C, D] are unit rows (the caller normalises), ``labels`` [B] (host array or tensor) the true
        classes.  loss[b, r] = max_{c != labels[b]} logit[c] - logit[labels[b]], pred[b, r] = first arg-max of the logits.
        Returns (best_idx int32 [B], best_feat [B, D] or None, loss [B, rho] or None, pred int32 [B, rho] or None,
        logits [B * rho, C] or None).  ``prefix_lens`` / ``kv``: prefix reuse as in ``score_candidates``; same bits."""
        return self._score(self._cls_target(class_features, labels, want_pred, want_logits), tokens, rho, want_features, want_loss,
                           seq_lens, prefix_lens, kv)

    def score_candidates_fused(self, base_tokens, base_lens, tokens, anchor: torch.Tensor, rho: int, seq_lens, prefix_lens,
                               objective: str = "l2", want_features: bool = False, want_loss: bool = False, single_edit: bool = False):
        """``encode_text_kv(base_tokens)`` and the first stage's ``score_candidates(..., prefix_lens, kv)`` in ONE pass
        (leaf_score_pass with kv_write: the B clean captions ride in the launches of their B*rho candidates).
        Returns (best_idx, best_feat or None, kv cache for the later stages[, loss [B, rho] when want_loss]), or None when
        the rows do not fit one chunk (the caller then uses the two separate calls).  Bit-identical to the separate calls.
        The pass fills cache slot 0, the one ``encode_text_kv`` fills by default: earlier caches of that slot are stale once it succeeds.
        ``single_edit``: as in ``score_candidates``; the cache it returns then holds the captions' layer-0 Q rows, which the later
        single_edit stages read (a cache of a pass without it does not, and such a stage refuses it)."""
        target = self._anchor_target(anchor, objective)
        B = target.B
        blens = np.ascontiguousarray(np.asarray(base_lens).reshape(-1), dtype=np.int32)
        full = np.asarray(seq_lens).reshape(-1).astype(np.int32)
        if single_edit:
            _check_equal_lengths(full, blens, rho)
        pfx = _clamp_prefix(prefix_lens, _prefix_limit(full, blens, rho), np.empty(full.size, dtype=np.int32))
        lens, cu = _lens_cu(np.concatenate([blens, full - pfx]))                             # rows to compute per sequence
        # [cu (B + n + 1) | prefix (B + n): the captions' own is 0]
        dev = torch.from_numpy(np.concatenate([cu, np.zeros(B, dtype=np.int32), pfx])).pin_memory().to(self.device, non_blocking=True)
        bt, ct = self._candidates(base_tokens, B), self._candidates(tokens, B, rho)
        t = torch.cat([bt, ct], 0)
        kvbuf = self._kv_buffer(0, int(cu[B]))
        a, keep, ret = self._score_args(target, t, rho, want_features, want_loss, seq_lens=lens.ctypes.data, cu_rows=dev.data_ptr(),
                                        prefix=dev.data_ptr() + 4 * (lens.size + 1), max_len=max(int(full.max()), int(blens.max())),
                                        kv=_ptr(kvbuf), kv_bytes=kvbuf.numel(), kv_write=1)
        if self._single_edit_call(single_edit, lambda: self._score_pass(a), (ct, full, pfx, bt, blens, rho)) == 2:
            return None
        self.rows_scored += int(cu[-1])
        # q0: without single_edit the fused launch keeps the captions' Q rows on chip, layer 0 of the cache holds K and V only
        return (*ret[:2], self._kv_cache(kvbuf, dev[:B + 1], int(cu[B]), blens, bool(single_edit), bt, 0), *ret[2:])

    # ------------------------------------------------------------------ training
    def enable_training(self):
        if self.grads is None:
            with torch.cuda.device(self.device):
                self.grads = torch.zeros_like(self.flat)
                self.exp_avg = torch.zeros_like(self.flat)
                self.exp_avg_sq = torch.zeros_like(self.flat)
                self.w16_bwd = torch.empty_like(self.w16)
                # gradient-scaler state + scratch of the guarded optimizer step (include/leaf_hip.h "gradient scaler"): attached to
                # the handle, so the fp16 backward checks its 16-bit gradient tensors for saturation (LEAF_GRAD_SCALER=0 detaches)
                self._clip_ws = torch.zeros(_lib.SC_WORDS + 2048, dtype=torch.float32, device=self.device)
                self._clipi_ws = torch.zeros(2 + 2048, dtype=torch.float32, device=self.device)     # scratch of clip_grads_
            self._scaler_attached = os.environ.get("LEAF_GRAD_SCALER", "1") != "0"
            if self._scaler_attached:
                _lib.check(self._lib.leaf_text_set_grad_scaler(self._h, _ptr(self._clip_ws)), "leaf_text_set_grad_scaler")
            self._packed = False
        return self

    def zero_grad(self):
        self.grads.zero_()

    def forward_train(self, text, seq_lens=None, delta: Optional[torch.Tensor] = None, normalize: bool = False,
                      pool_last: bool = False) -> torch.Tensor:
        """Training-mode forward that keeps the activation stash.  ``pool_last`` (text embedding inversion, leaf_amd/inversion.py):
        pool at row ``seq_lens[i] - 1`` and keep all ``seq_lens[i]`` rows whatever the ids are -- an inverted prompt may hold
        EOT / SOT ids anywhere (include/leaf_hip.h, leaf_train_fwd_args); needs ``seq_lens``, excludes ``delta``.  ``delta`` (optional embedding-space PGD mode, SURVEY 8a
        row a12): fp32 CUDA tensor [rows, width] in the PACKED row layout of this call (``rows_of(seq_lens)`` rows; dense
        [N * ctx, width] when rows are not trimmed), added to the token embeddings.  ``normalize`` = --normalize_fare
        (utils_AT.py:319): returns F.normalize(features); the following ``backward`` differentiates through it."""
        # everything that can refuse the call comes before the first change of the model's training state
        plan = self._row_plan(text, seq_lens, place=False)
        rows = plan.rows(len(text), self.cfg.context_length)
        if pool_last and (delta is not None or seq_lens is None or plan.lens is None):
            raise ValueError("pool_last needs explicit seq_lens (and row trimming on) and takes no delta")
        if delta is not None and (delta.dtype != torch.float32 or not delta.is_contiguous() or delta.numel() != rows * self.cfg.width):
            raise ValueError(f"delta must be contiguous fp32 with {rows} x {self.cfg.width} elements")
        self.enable_training()
        plan.place(self.device)
        t = self._tokens(text)
        n = t.shape[0]
        self.train_pass = None      # from here on the stash no longer holds the previous pass
        stash = self._grow("stash", self._lib.leaf_text_stash_bytes(self._h, n))
        out = torch.empty(n, self.cfg.embed_dim, dtype=torch.float32, device=self.device)
        ws = self._workspace(2, n)
        if self._lib.leaf_text_get_option(self._h, b"normalize_fare") != int(bool(normalize)):
            self.set_option("normalize_fare", int(bool(normalize)))
        params, w16 = self._weights()
        a = _lib.TrainFwdArgs(params=params, w16_fwd=w16, tokens=_ptr(t), seq_lens=plan.lens_ptr, cu_rows=plan.cu_ptr, n_seq=n,
                              delta=_ptr(delta), pool_last=int(bool(pool_last)), out=_ptr(out), stash=_ptr(stash),
                              stash_bytes=stash.numel(), ws=_ptr(ws), ws_bytes=ws.numel(), stream=self._stream())
        _lib.check(self._lib.leaf_text_forward_train(self._h, a), "leaf_text_forward_train")
        self.stash_ticket += 1
        self.train_pass = _TrainPass(t, plan, n, rows, bool(normalize), bool(pool_last), self.stash_ticket)
        return out

    def _last_pass(self, who: str, ticket: Optional[int] = None) -> _TrainPass:
        """the pass whose activations the stash holds, for ``who``; ``ticket`` (optional): the ``stash_ticket`` it must carry"""
        p = self.train_pass
        if p is None:
            raise RuntimeError(f"{who}: the stash holds no training pass; run forward_train first")
        if ticket is not None and ticket != p.ticket:
            raise RuntimeError(f"{who}: stale stash ticket {ticket} (current {p.ticket}): another forward_train has "
                               "overwritten the activations of this forward; one differentiable forward may be pending per model")
        return p

    def _backward_call(self, p: _TrainPass, head: int, feat: torch.Tensor, ref: torch.Tensor, scale: float = 1.0, head_out=None,
                       grads=None, d_embed: bool = False, layer_events=None):
        """The backward through the stash of pass ``p`` from loss head ``head`` (``_lib.HEAD_*``; ``ref`` / ``scale`` / ``head_out``
        as in include/leaf_hip.h, leaf_backward_args).  ``grads``: the flat buffer the parameter gradients are added to, or None;
        ``d_embed``: also return the gradient of the token embeddings, fp32 [rows, width] packed, allocated here (else None);
        ``layer_events``: the caller's block events or None."""
        g = torch.empty(p.rows, self.cfg.width, dtype=torch.float32, device=self.device) if d_embed else None
        events = None
        if layer_events is not None:
            if len(layer_events) != self.cfg.layers + 1:
                raise ValueError(f"layer_events must hold {self.cfg.layers + 1} events")
            events = (C.c_void_p * len(layer_events))(*[C.c_void_p(e.cuda_event) for e in layer_events])
        ws = self._workspace(2, p.n)
        a = _lib.BackwardArgs(params=_ptr(self.flat), w16_bwd=_ptr(self.w16_bwd), tokens=_ptr(p.tokens), seq_lens=p.plan.lens_ptr,
                              cu_rows=p.plan.cu_ptr, n_seq=p.n, feat=_ptr(feat), head=head, ref=_ptr(ref), scale=float(scale),
                              head_out=_ptr(head_out), stash=_ptr(self._buf["stash"]), grads=_ptr(grads), d_embed=_ptr(g),
                              layer_events=C.addressof(events) if events is not None else None, ws=_ptr(ws), ws_bytes=ws.numel(),
                              stream=self._stream())
        _lib.check(self._lib.leaf_text_backward(self._h, a), "leaf_text_backward")
        return g

    def input_grad(self, feat: torch.Tensor, anchor: torch.Tensor):
        """TextFARE loss of (anchor, feat) and its gradient with respect to the token embeddings (= the gradient of
        ``delta``) through the stash of the last ``forward_train``: (loss 0-d, d_embed fp32 [rows, width] packed).
        No parameter gradient is touched (the inner step of the optional embedding-space PGD mode)."""
        p = self._last_pass("input_grad")
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        anchor = anchor.to(device=self.device, dtype=torch.float32).contiguous()
        return loss, self._backward_call(p, _lib.HEAD_FARE, feat.contiguous(), anchor, head_out=loss, d_embed=True)

    def cosine_input_grad(self, feat: torch.Tensor, target: torch.Tensor, loss_weight: float = 1.0):
        """Cosine head of text embedding inversion on the stash of the last ``forward_train``: per sequence b the loss
        ``loss_weight (1 - cos(feat_b, target_b))`` and the gradient of the SUM over b with respect to the token embeddings, so
        every sequence gets the gradient of its own loss (src/pez/optim_utils.py:191-196 for one prompt and one target).
        Returns (cos fp32 [n], d_embed fp32 [rows, width] packed)."""
        p = self._last_pass("cosine_input_grad")
        target = target.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(target.shape) != (p.n, self.cfg.embed_dim) or tuple(feat.shape) != (p.n, self.cfg.embed_dim):
            raise ValueError(f"feat and target must be [{p.n}, {self.cfg.embed_dim}]")
        cos = torch.empty(p.n, dtype=torch.float32, device=self.device)
        return cos, self._backward_call(p, _lib.HEAD_COSINE, feat.contiguous(), target, loss_weight, head_out=cos, d_embed=True)

    def nn_project(self, embeds: torch.Tensor):
        """PEZ's projection step (nn_project, src/pez/optim_utils.py:26-55): for every row of ``embeds`` [M, width] the id of the
        cosine-nearest row of the token-embedding table and that cosine, on the device: (ids int32 [M], cos fp32 [M]).  The
        table's inverse row norms are computed once per weight version (``load_state_dict`` / ``adamw_step`` / ``copy_from``
        drop them)."""
        d, V = self.cfg.width, self.cfg.vocab_size
        if embeds.device != self.device or embeds.dtype != torch.float32 or embeds.dim() != 2 or embeds.shape[1] != d:
            raise ValueError(f"embeds must be fp32 [M, {d}] on {self.device}")
        q = embeds.contiguous()
        M = q.shape[0]
        table = self.params["token_embedding.weight"]
        if self._vocab_inv is None:
            inv = torch.empty(V, dtype=torch.float32, device=self.device)
            _lib.check(self._lib.leaf_vocab_inv_norms(_ptr(table), V, d, _ptr(inv), self._stream()), "leaf_vocab_inv_norms")
            self._vocab_inv = inv
        ids = torch.empty(M, dtype=torch.int32, device=self.device)
        cos = torch.empty(M, dtype=torch.float32, device=self.device)
        ws = self._grow(("ws", "nnproj"), self._lib.leaf_nn_project_ws_bytes(M, V))
        _lib.check(self._lib.leaf_nn_project(_ptr(q), M, _ptr(table), _ptr(self._vocab_inv), V, d, _ptr(ids), _ptr(cos), _ptr(ws),
                                             ws.numel(), self._stream()), "leaf_nn_project")
        return ids, cos

    def pgd_step(self, delta: torch.Tensor, grad: torch.Tensor, alpha: float, eps: float, norm: str = "linf"):
        """In-place fused update of the resident perturbation for the rows of the last ``forward_train``:
        'linf': clamp(delta + alpha sign(grad), -eps, eps); 'l2': per-sequence normalised step + L2-ball projection."""
        p = self._last_pass("pgd_step")
        _lib.check(self._lib.leaf_pgd_step(_ptr(delta), _ptr(grad), p.plan.cu_ptr, p.n, self.cfg.context_length, self.cfg.width,
                                           float(alpha), float(eps), {"linf": 0, "l2": 2}[norm], self._stream()), "leaf_pgd_step")
        return delta

    def backward(self, feat: torch.Tensor, anchor: torch.Tensor, accum_scale: float = 1.0, layer_events=None) -> torch.Tensor:
        """TextFARE loss of (anchor, feat) + backward through the stash of the last ``forward_train``.
        Accumulates into ``self.grads``; returns the (unscaled) loss as a 0-d CUDA tensor.
        ``layer_events``: optional list of cfg.layers + 1 ``torch.cuda.Event`` (already created, i.e. recorded once): event l
        is recorded when every gradient of block l is final, the last one when everything is (gradient-bucket overlap)."""
        p = self._last_pass("backward")
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        anchor = anchor.to(device=self.device, dtype=torch.float32).contiguous()
        self._backward_call(p, _lib.HEAD_FARE, feat.contiguous(), anchor, accum_scale, head_out=loss, grads=self.grads, layer_events=layer_events)
        return loss

    def backward_from(self, feat: torch.Tensor, dfeat: torch.Tensor, accum_scale: float = 1.0, param_grads: bool = True,
                      want_input_grad: bool = False, layer_events=None, ticket: Optional[int] = None):
        """Backward from ANY upstream gradient through the stash of the last ``forward_train`` (LEAF_HEAD_UPSTREAM): ``dfeat``
        [n, embed_dim] = d loss / d ``feat`` of a loss the caller computed; ``accum_scale * dfeat`` is back-propagated, through
        F.normalize as well when that forward ran with ``normalize=True``.  ``param_grads``: ACCUMULATE the parameter gradients into
        ``self.grads`` (as ``backward``); ``want_input_grad``: also return the gradient with respect to the token embeddings
        (= ``delta``), fp32 [rows, width] in the packed row layout of ``input_grad``.  Returns that tensor, or None when it was not
        asked for.  ``layer_events``: as in ``backward``.  ``ticket``: the value of ``self.stash_ticket`` right after the forward
        this gradient belongs to; when another ``forward_train`` has run since, the stash holds ITS activations and this raises
        ``RuntimeError`` instead of differentiating through them."""
        p = self._last_pass("backward_from", ticket)
        if not param_grads and not want_input_grad:
            raise ValueError("backward_from: nothing to compute (param_grads and want_input_grad are both off)")
        if tuple(feat.shape) != (p.n, self.cfg.embed_dim) or tuple(dfeat.shape) != (p.n, self.cfg.embed_dim):
            raise ValueError(f"feat and dfeat must be [{p.n}, {self.cfg.embed_dim}]")
        feat = feat.detach().to(device=self.device, dtype=torch.float32).contiguous()
        dfeat = dfeat.detach().to(device=self.device, dtype=torch.float32).contiguous()
        return self._backward_call(p, _lib.HEAD_UPSTREAM, feat, dfeat, accum_scale, grads=self.grads if param_grads else None,
                                   d_embed=want_input_grad, layer_events=layer_events)

    def encode_text_train(self, text, seq_lens=None, delta: Optional[torch.Tensor] = None, normalize: bool = False,
                          pool_last: bool = False) -> torch.Tensor:
        """``forward_train`` under autograd (leaf_amd/autograd.py): the returned features carry a ``grad_fn``, and ``backward()`` of any
        PyTorch loss of them runs the engine's backward (``backward_from``).  Parameter gradients are ACCUMULATED into ``self.grads``,
        the flat buffer that ``adamw_step`` / ``LeafAdamW`` consume -- NOT into ``.grad`` attributes; ``delta.grad`` is filled when
        ``delta.requires_grad``.  One differentiable forward may be pending per model (a later ``forward_train`` makes the backward of
        an earlier one raise).  Under ``torch.no_grad()`` this is ``forward_train``."""
        from .autograd import encode_text_train
        return encode_text_train(self, text, seq_lens=seq_lens, delta=delta, normalize=normalize, pool_last=pool_last)

    def clip_grads_(self, max_norm: Optional[float], pre_scale: float = 1.0) -> torch.Tensor:
        """``torch.nn.utils.clip_grad_norm_`` on the accumulated gradient buffer, in place (utils_AT.py:348-357 with
        --accum-freq > 1: the running sum is clipped after every micro-batch's backward).  ``pre_scale`` is applied in the same
        pass; ``max_norm=None`` only applies it.  Returns the 0-d norm tensor (of pre_scale * grads, before clipping)."""
        _lib.check(self._lib.leaf_clip_grads_inplace(_ptr(self.grads), self.n_params, float(pre_scale),
                                                     float(max_norm) if max_norm is not None else float("inf"),
                                                     _ptr(self._clipi_ws), self._stream()), "leaf_clip_grads_inplace")
        return self._clipi_ws[1]

    def adamw_step(self, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                   grad_scale: float = 1.0, max_norm: Optional[float] = None, guard: bool = True):
        """Fused AdamW over the flat buffers.  ``max_norm`` (--grad-clip-norm, utils_AT.py:348-357): clip the global L2
        norm of grad_scale * grads first (torch.nn.utils.clip_grad_norm_ semantics).  ``guard`` (default): one extra read of
        the gradients computes their global norm and SKIPS the whole step when it is inf / NaN (what GradScaler.step does in
        the reference's fp16 regime).  The 16-bit conversions of the gradient path saturate instead of producing inf; the backward
        therefore checks its 16-bit gradient tensors and poisons the gradient with a NaN when one saturated, so this guard skips
        that step too -- on every rank, the NaN travels through the all-reduce -- and the persistent loss-scale back-off halves
        (GradScaler.update; ``loss_scale_backoff()``).  ``opt_step`` counts ATTEMPTED steps; the bias corrections use the steps
        really applied (kept on the device: a skipped step does not advance them, as torch's per-parameter ``step``).
        Returns the 0-d total-norm tensor when clipping or guarding, else None; ``skipped_steps()`` counts skipped steps."""
        self.opt_step += 1
        self._vocab_inv = None      # nn_project's table norms belong to the weights before this step
        # with the gradient scaler attached a saturated backward has poisoned the gradient with a NaN that only the guard stops
        guard = guard or self._scaler_attached
        if max_norm is not None or guard:
            _lib.check(self._lib.leaf_adamw_step_clip(_ptr(self.flat), _ptr(self.grads), _ptr(self.exp_avg),
                                                      _ptr(self.exp_avg_sq), self.n_params, self.n_decay, float(lr),
                                                      float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                                      self.opt_step, float(grad_scale),
                                                      float(max_norm) if max_norm is not None else float("inf"),
                                                      _ptr(self._clip_ws), self._stream()), "leaf_adamw_step_clip")
            self._packed = False
            return self._clip_ws[_lib.SC_NORM]
        _lib.check(self._lib.leaf_adamw_step(_ptr(self.flat), _ptr(self.grads), _ptr(self.exp_avg),
                                             _ptr(self.exp_avg_sq), self.n_params, self.n_decay, float(lr),
                                             float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                             self.opt_step, float(grad_scale), self._stream()), "leaf_adamw_step")
        self._packed = False
        return None

    def skipped_steps(self) -> int:
        """Optimizer steps skipped by the non-finite guard so far (synchronises: call it where the loop already does)."""
        ws = self._clip_ws
        return int(ws[_lib.SC_SKIPPED].item()) if ws is not None else 0

    def applied_steps(self) -> int:
        """AdamW steps really taken = attempted - skipped: the ``step`` of the bias corrections and of a checkpoint (synchronises)."""
        return self.opt_step - self.skipped_steps()

    def set_applied_steps(self, step: int):
        """After loading optimizer state: ``step`` applied steps so far, none skipped."""
        self.opt_step = int(step)
        ws = self._clip_ws
        if ws is not None:
            ws[_lib.SC_SKIPPED] = 0.0
            ws[_lib.SC_APPLIED] = float(step)

    def grad_scaler_state(self) -> dict:
        """GradScaler-style bookkeeping of the fp16 gradient path (synchronises): the persistent loss-scale factor 2^backoff,
        steps skipped in all / because a 16-bit gradient tensor saturated."""
        ws = self._clip_ws
        if ws is None:
            return {"loss_scale_factor": 1.0, "skipped": 0, "skipped_saturated": 0}
        h = ws[:_lib.SC_WORDS].cpu()
        return {"loss_scale_factor": float(2.0 ** float(h[_lib.SC_BACKOFF])), "skipped": int(h[_lib.SC_SKIPPED]),
                "skipped_saturated": int(h[_lib.SC_SAT_STEPS]), "good_steps": int(h[_lib.SC_GOOD])}

def create_model(name: str, device="cuda:0", dtype: str = None, pretrained: Optional[str] = None,
                 trainable: bool = False, seed: int = 1) -> LeafCLIPText:
    """open_clip.create_model equivalent for the text tower: random init (seeded) or a local checkpoint
    (OpenCLIP .bin/.pt or HF safetensors / directory).  ``hf-hub:`` ids map to their architecture; weights must be
    given as a local path (there is no network on the build or GPU boxes).  An ``open_clip_config.json`` next to the
    checkpoint (the hub layout, src/open_clip/factory.py:200-207) defines the architecture when present."""
    cfg = None
    if pretrained:
        import dataclasses
        import logging
        from .checkpoint import read_open_clip_config
        cfg = read_open_clip_config(pretrained)
        try:
            named = get_config(name)
        except (KeyError, ValueError):
            named = None              # an unknown name is fine when the json defines the architecture
        if cfg is not None and named is not None:
            # the name (or --force-quick-gelu's '-quickgelu' suffix) can only ADD QuickGELU: hub configs of the OpenAI-lineage
            # towers omit the flag and rely on the model name (src/open_clip/factory.py:219-222)
            if named.quick_gelu and not cfg.quick_gelu:
                cfg = dataclasses.replace(cfg, quick_gelu=True)
            shape = lambda c: (c.width, c.heads, c.layers, c.embed_dim, c.context_length, c.vocab_size)
            if shape(cfg) != shape(named):
                if not name.startswith("hf-hub:"):
                    raise ValueError(f"open_clip_config.json next to '{pretrained}' describes a text tower (width, heads, layers, embed_dim, "
                                     f"ctx, vocab) = {shape(cfg)}, but --model {name} is {shape(named)}: remove the stray json or name the "
                                     "model the checkpoint belongs to")
                logging.info(f"architecture taken from the open_clip_config.json next to '{pretrained}': {shape(cfg)}")
            else:
                logging.info(f"open_clip_config.json next to '{pretrained}' agrees with --model {name}"
                             + (" (QuickGELU from the model name)" if named.quick_gelu else ""))
    m = LeafCLIPText(cfg or get_config(name), device=device, dtype=dtype, trainable=trainable)
    if pretrained:
        from .checkpoint import load_checkpoint_file
        m.load_state_dict(load_checkpoint_file(pretrained))
    else:
        m.init_random(seed)
    return m
