"""CPU-only half of the per-token hidden states (include/leaf_hip.h, leaf_text_forward_hidden): the ctypes mirror of leaf_hidden_args /
leaf_hidden_tap against the header, every refusal of the entry (each reported before any HIP call, so they run without a GPU),
the wiring of leaf_amd/hf_text.py against a stub model with the three names it uses (encode_text_hidden, encode_text, cfg), and the
argument handling of encode_prompts.py.  The kernel and the passes are held to their checks in tests/test_gpu_hidden.py.

One refusal of the entry cannot be provoked through a valid handle: "a width the kernel does not take" (width % 4, width <= 2048) --
leaf_text_create itself refuses every such width (width % 128, <= 2048), which the last test pins."""
import ctypes as C
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from leaf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "size_t": C.c_size_t, "float": C.c_float, "leaf_stream_t": C.c_void_p}
FAKE = 64                   # a non-null address that no refused call dereferences


def header_fields(name):
    """[(field, ctypes type)] of ``typedef struct name { ... } name;`` in the header: every pointer is a c_void_p"""
    hdr = open(os.path.join(ROOT, "include", "leaf_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base, rest = re.match(r"(?:const\s+)?(\w+)\s*(.*)$", decl, re.S).groups()
        for d in rest.split(","):
            fields.append((re.search(r"(\w+)\s*$", d).group(1), C.c_void_p if "*" in d else SCALARS[base]))
    return fields


def test_ctypes_structs_equal_the_header():
    want = header_fields("leaf_hidden_args")
    assert want[0] == ("size", C.c_uint32)
    assert list(_lib.HiddenArgs._fields_) == want
    assert _lib.HiddenArgs().size == C.sizeof(_lib.HiddenArgs)
    assert list(_lib.HiddenTap._fields_) == header_fields("leaf_hidden_tap")
    assert C.sizeof(_lib.HiddenTap) == 16
    assert _lib._SIGS["leaf_text_forward_hidden"] == (C.c_int, [C.c_void_p, C.POINTER(_lib.HiddenArgs)])


@pytest.fixture(scope="module")
def vitl():
    l = _lib.lib()
    h = C.c_void_p()
    cfg = _lib.TextCfgC(12, 768, 12, 768, 77, 49408, 1, 1e-5)
    assert l.leaf_text_create(C.byref(cfg), 1, C.byref(h)) == 0
    yield l, h
    l.leaf_text_destroy(h)


LENS = (C.c_int32 * 2)(5, 5)


def taps(*rows):
    return (_lib.HiddenTap * max(len(rows), 1))(*[_lib.HiddenTap(*r) for r in rows])


def hidden_args(tap_rows=((12, 1, FAKE),), **change):
    """last_hidden_state of 2 dense sequences; ``tap_rows`` / ``change`` make it a call the entry refuses.  Returns (args, the tap
    array, which must outlive the call)"""
    arr = taps(*tap_rows)
    fields = dict(params=FAKE, w16_fwd=FAKE, tokens=FAKE, n_seq=2, taps=C.addressof(arr), n_taps=len(tap_rows), ws=FAKE, ws_bytes=1 << 20)
    fields.update(change)
    return _lib.HiddenArgs(**fields), arr


def refused(l, rc, message):
    assert rc != 0 and message in l.leaf_last_error(), (rc, l.leaf_last_error())


@pytest.mark.parametrize("tap_rows,change,message", [
    (((12, 1, FAKE),), dict(params=None), b"params"),
    (((12, 1, FAKE),), dict(tokens=None), b"tokens"),
    (((12, 1, FAKE),), dict(ws=None), b"ws"),
    (((12, 1, FAKE),), dict(w16_fwd=None), b"w16_fwd"),                           # only the precise pass does without the pack
    (((12, 1, FAKE),), dict(n_seq=0), b"n_seq"),
    ((), dict(), b"n_taps"),                                                     # neither taps nor features
    ((), dict(n_taps=-1, feat=FAKE), b"n_taps"),
    (((12, 1, FAKE),), dict(taps=None), b"n_taps"),                              # a count without the array
    (((12, 1, None),), dict(), b"taps[0].out"),
    (((0, 0, FAKE), (3, 1, None)), dict(), b"taps[1].out"),
    (((13, 0, FAKE),), dict(), b"taps[0].layer 13 outside 0..12"),
    (((0, 0, FAKE), (-1, 0, FAKE)), dict(), b"taps[1].layer -1 outside 0..12"),
    (((11, 0, FAKE), (12, 1, FAKE), (11, 0, FAKE)), dict(), b"taps[0] and taps[2] are both (layer 11, final_ln 0)"),
    (((12, 1, FAKE), (12, 2, FAKE)), dict(), b"are both (layer 12, final_ln 1)"),   # any non-zero final_ln is "on"
    (((12, 1, FAKE),), dict(seq_lens=C.addressof(LENS)), b"go together"),
    (((12, 1, FAKE),), dict(cu_rows=FAKE), b"go together"),
    (((12, 1, FAKE),), dict(out_dtype=2), b"out_dtype 2"),
    (((12, 1, FAKE),), dict(out_dtype=-1), b"out_dtype -1"),
    (((12, 1, FAKE),), dict(precise=1, out_dtype=1), b"precise writes fp32"),
])
def test_forward_hidden_refusals(vitl, tap_rows, change, message):
    l, h = vitl
    a, keep = hidden_args(tap_rows, **change)
    refused(l, l.leaf_text_forward_hidden(h, a), message)
    assert b"forward_hidden" in l.leaf_last_error()
    del keep


def test_forward_hidden_refuses_a_null_handle_null_arguments_and_another_size(vitl):
    l, h = vitl
    a, keep = hidden_args()
    refused(l, l.leaf_text_forward_hidden(None, a), b"null handle")
    refused(l, l.leaf_text_forward_hidden(h, None), b"leaf_hidden_args")
    for off in (-4, 4):
        a, keep = hidden_args()
        a.size += off
        refused(l, l.leaf_text_forward_hidden(h, a), b"leaf_hidden_args")


def test_no_handle_has_a_width_the_row_kernel_refuses():
    l = _lib.lib()
    for width in (130, 132, 2176):
        h = C.c_void_p()
        cfg = _lib.TextCfgC(2, width, width // 64, 128, 77, 49408, 1, 1e-5)
        assert l.leaf_text_create(C.byref(cfg), 1, C.byref(h)) != 0 and not h.value


# ---------------------------------------------------------------- leaf_amd/hf_text.py against a stub
class _StubModel:
    """hidden state l of row (i, p) = ids[i, p] + 1000 l (+ 0.5 behind ln_final); features = 2 x the EOT row's id"""

    def __init__(self, layers=3, width=4, embed_dim=2, ctx=6):
        self.cfg = SimpleNamespace(layers=layers, width=width, embed_dim=embed_dim, context_length=ctx, vocab_size=50, quick_gelu=True)
        self.calls = []

    def encode_text_hidden(self, text, layers=(-1,), final_ln=True, seq_lens="dense", precise=None, dtype=torch.float32,
                           want_features=False, normalize=False):
        self.calls.append(dict(layers=list(layers), final_ln=list(final_ln), seq_lens=seq_lens, want_features=want_features))
        ids = torch.as_tensor(text).float()
        out = [(ids + 1000.0 * l + (0.5 if ln else 0.0))[..., None].expand(-1, -1, self.cfg.width).clone() for l, ln in zip(layers, final_ln)]
        feat = 2.0 * ids.max(-1).values[:, None].expand(-1, self.cfg.embed_dim)
        return (out, feat) if want_features else out

    def encode_text(self, text, normalize=False):
        self.calls.append(("encode_text", normalize))
        return torch.full((len(text), self.cfg.embed_dim), 7.0)


IDS = torch.tensor([[48, 3, 49, 0, 0, 0], [48, 5, 6, 7, 49, 49], [48, 49, 49, 49, 49, 49]])      # EOT = 49 at 2, 4 (then padded with it), 1


def test_hf_encoder_plain_output_names_tuple_access_and_pooling_row():
    from leaf_amd.hf_text import LeafHFTextEncoder
    m = _StubModel()
    enc = LeafHFTextEncoder(m)
    out = enc(IDS)
    assert m.calls == [dict(layers=[3], final_ln=[True], seq_lens="dense", want_features=False)]      # last_hidden_state alone, all rows
    assert out.last_hidden_state.shape == (3, 6, 4) and out.hidden_states is None and out.text_embeds is None
    assert torch.equal(out.last_hidden_state[..., 0], IDS.float() + 3000.5)
    # the row at the FIRST maximum id, of last_hidden_state
    assert torch.equal(out.pooler_output, out.last_hidden_state[torch.arange(3), torch.tensor([2, 4, 1])])
    assert out[0] is out.last_hidden_state and out[1] is out.pooler_output
    a, b = out
    assert a is out.last_hidden_state and b is out.pooler_output


def test_hf_encoder_hidden_states_follow_hf_indexing():
    from leaf_amd.hf_text import LeafHFTextEncoder
    m = _StubModel()
    out = LeafHFTextEncoder(m)(IDS, output_hidden_states=True, position_ids=None, output_attentions=None)
    assert m.calls[0]["layers"] == [0, 1, 2, 3, 3] and m.calls[0]["final_ln"] == [False, False, False, False, True]
    assert isinstance(out.hidden_states, tuple) and len(out.hidden_states) == m.cfg.layers + 1
    for l, hs in enumerate(out.hidden_states):
        assert torch.equal(hs[..., 0], IDS.float() + 1000.0 * l)                                   # no ln_final on any of them
    assert torch.equal(out.hidden_states[-2][..., 0], IDS.float() + 2000.0)                        # SDXL's layer
    assert torch.equal(out.last_hidden_state[..., 0], IDS.float() + 3000.5)
    assert out[2] is out.hidden_states


def test_hf_encoder_with_projection_returns_the_features_of_the_same_pass():
    from leaf_amd.hf_text import LeafHFTextEncoder
    m = _StubModel()
    enc = LeafHFTextEncoder(m, with_projection=True)
    out = enc(IDS, output_hidden_states=True)
    assert len(m.calls) == 1 and m.calls[0]["want_features"] is True
    assert torch.equal(out.text_embeds, torch.full((3, 2), 98.0)) and out.pooler_output is None
    assert out[0] is out.text_embeds and out[1] is out.last_hidden_state and out[2] is out.hidden_states      # CLIPTextModelOutput's order
    assert torch.equal(enc.encode_text(IDS, normalize=True), torch.full((3, 2), 7.0)) and m.calls[-1] == ("encode_text", True)


def test_hf_encoder_attributes_and_refusals():
    from leaf_amd.hf_text import LeafHFTextEncoder
    m = _StubModel()
    enc = LeafHFTextEncoder(m)
    c = enc.config
    assert (c.hidden_size, c.projection_dim, c.num_hidden_layers, c.max_position_embeddings) == (4, 2, 3, 6)
    assert enc.dtype == torch.float32 and enc.device == torch.device("cpu")
    with pytest.raises(ValueError, match="attention_mask"):
        enc(IDS, attention_mask=torch.ones_like(IDS))
    with pytest.raises(TypeError, match="position_ids"):
        enc(IDS, position_ids=torch.arange(6))
    assert m.calls == []


# ---------------------------------------------------------------- negative layers (LeafCLIPText.hidden_taps needs no device)
def test_negative_layers_count_from_the_end_of_hidden_states():
    from leaf_amd.model import LeafCLIPText
    m = SimpleNamespace(cfg=SimpleNamespace(layers=12))
    taps_of = lambda *a, **k: LeafCLIPText.hidden_taps(m, *a, **k)
    assert taps_of() == [(12, True)]
    assert taps_of((-1, -2, 0, 12, -13), final_ln=(True, False, False, True, False)) == [(12, True), (11, False), (0, False), (12, True), (0, False)]
    assert taps_of((-2,), final_ln=False) == [(11, False)]
    for bad in ((13,), (-14,)):
        with pytest.raises(ValueError, match="hidden_states has 13 entries"):
            taps_of(bad)
    with pytest.raises(ValueError, match="final_ln"):
        taps_of((1, 2), final_ln=(True,))


# ---------------------------------------------------------------- encode_prompts.py
def _cli(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "encode_prompts.py"), *argv], capture_output=True, text=True, cwd=ROOT)


def test_encode_prompts_help_names_its_arguments():
    r = _cli("--help")
    assert r.returncode == 0
    for word in ("--model", "--checkpoint", "--texts", "--layer", "--final-ln", "--no-final-ln", "--precise", "--pad", "{eot,zero}", "--out",
                 "--attack-name", "--k", "--rho", "--adv-objective", "prompt_embeds", "pooled_prompt_embeds"):
        assert word in r.stdout, word


@pytest.mark.parametrize("argv,message", [
    (["--out", "x.npz"], "--texts"),                                                                # required
    (["--texts", "t.txt"], "--out"),
    (["--texts", "t.txt", "--out", "x.npy"], ".npz"),
    (["--texts", "t.txt", "--out", "x.npz", "--pad", "space"], "--pad"),
    (["--texts", "t.txt", "--out", "x.npz", "--model", "tiny-test", "--layer", "3"], "--layer 3"),   # 2 blocks: 0..2
    (["--texts", "t.txt", "--out", "x.npz", "--model", "tiny-test", "--layer", "-4"], "--layer -4"),
    (["--texts", "t.txt", "--out", "x.npz", "--model", "no-such-tower"], "unknown text tower"),
    (["--texts", "t.txt", "--out", "x.npz", "--model", "tiny-test", "--k", "2"], "--attack-name charmer"),
    (["--texts", "t.txt", "--out", "x.npz", "--model", "tiny-test", "--attack-name", "charmer", "--k", "1"], "--rho"),
    (["--texts", "t.txt", "--out", "x.npz", "--model", "tiny-test", "--attack-name", "leaf"], "--attack-name"),
    (["--texts", "t.txt", "--out", "x.npz"], "--checkpoint is empty"),                              # ViT-L without weights
])
def test_encode_prompts_argument_errors(argv, message, capsys):
    import encode_prompts
    with pytest.raises(SystemExit) as e:
        encode_prompts.main(argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_pad_with_eot_keeps_the_first_maximum():
    import numpy as np
    from encode_prompts import pad_with_eot
    ids = np.array([[48, 3, 49, 0, 0, 0], [48, 5, 6, 7, 8, 49]], np.int32)
    got = pad_with_eot(ids)
    assert got.tolist() == [[48, 3, 49, 49, 49, 49], [48, 5, 6, 7, 8, 49]] and ids[0, 3] == 0
    assert (got.argmax(-1) == ids.argmax(-1)).all()
