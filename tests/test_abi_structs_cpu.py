"""CPU-only: the three argument structs of the C ABI (include/leaf_hip.h: leaf_score_args, leaf_train_fwd_args, leaf_backward_args).
Their ctypes mirrors in leaf_amd/_lib.py are held to the header field by field, and every combination of fields that an entry refuses
is refused before its first HIP call: each row checks the message of the argument check itself, on a box without a GPU."""
import ctypes as C
import os
import re

import pytest

from leaf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"leaf_score_args": _lib.ScoreArgs, "leaf_train_fwd_args": _lib.TrainFwdArgs, "leaf_backward_args": _lib.BackwardArgs}
ENTRIES = {"leaf_score_args": "leaf_score_pass", "leaf_train_fwd_args": "leaf_text_forward_train", "leaf_backward_args": "leaf_text_backward"}
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


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_ctypes_struct_equals_the_header(name):
    want = header_fields(name)
    assert want[0] == ("size", C.c_uint32)
    assert list(STRUCTS[name]._fields_) == want
    assert STRUCTS[name]().size == C.sizeof(STRUCTS[name])
    assert _lib._SIGS[ENTRIES[name]] == (C.c_int, [C.c_void_p, C.POINTER(STRUCTS[name])])


@pytest.fixture(scope="module")
def vitl():
    l = _lib.lib()
    h = C.c_void_p()
    cfg = _lib.TextCfgC(12, 768, 12, 768, 77, 49408, 1, 1e-5)
    assert l.leaf_text_create(C.byref(cfg), 1, C.byref(h)) == 0
    yield l, h
    l.leaf_text_destroy(h)


def refused(l, rc, message):
    assert rc != 0 and rc != 2 and message in l.leaf_last_error(), (rc, l.leaf_last_error())


LENS = (C.c_int32 * 8)(*[5] * 8)


def score_args(**change):
    """a dense pass of 2 x 3 candidates against an anchor; ``change`` makes it one the entry refuses"""
    fields = dict(params=FAKE, w16_fwd=FAKE, tokens=FAKE, B=2, rho=3, anchor=FAKE, objective=0, best_idx=FAKE, ws=FAKE, ws_bytes=1 << 20)
    fields.update(change)
    return _lib.ScoreArgs(**fields)


PREFIX = dict(prefix=FAKE, kv=FAKE, seq_lens=C.addressof(LENS), cu_rows=FAKE, base_cu=FAKE, base_rows=10)
CLASSES = dict(anchor=None, class_feat=FAKE, C=10, labels=FAKE, loss=FAKE)


@pytest.mark.parametrize("change,message", [
    (dict(anchor=None), b"exactly one of anchor / class_feat"),                                       # neither target
    (dict(class_feat=FAKE, C=10, labels=FAKE, loss=FAKE), b"exactly one of anchor / class_feat"),     # both
    (dict(kv=FAKE), b"without prefix"),                                                               # dense with kv
    (dict(base_cu=FAKE), b"without prefix"),
    (dict(kv_write=1), b"without prefix"),
    (dict(PREFIX, base_cu=None), b"a prefix pass needs"),                                             # prefix without base_cu
    (dict(PREFIX, kv=None), b"a prefix pass needs"),
    (dict(PREFIX, seq_lens=None), b"a prefix pass needs"),
    (dict(PREFIX, cu_rows=None), b"a prefix pass needs"),
    (dict(PREFIX, kv_write=1), b"a prefix pass needs"),                                               # fused: base_cu is cu_rows' head
    (dict(PREFIX, **CLASSES, base_cu=None, kv_write=1, kv_bytes=1 << 30), b"anchor target only"),     # fused with class_feat
    (dict(CLASSES, C=1), b"classes"),                                                                 # LEAF_CLS_MIN_CLASSES - 1
    (dict(CLASSES, C=1025), b"classes"),                                                              # LEAF_CLS_MAX_CLASSES + 1
    (dict(CLASSES, loss=None), b"null/invalid"),                                                      # a class target without loss
    (dict(CLASSES, labels=None), b"null/invalid"),
    (dict(CLASSES, rho=1 << 20), b"candidates per caption"),                                          # rho > LEAF_SCORE_MAX_RHO
    (dict(objective=4), b"unknown objective 4"),
    (dict(objective=-1), b"unknown objective"),
    (dict(B=0), b"null/invalid"),
    (dict(rho=0), b"null/invalid"),
    (dict(best_idx=None), b"null/invalid"),
])
def test_score_pass_refusals(vitl, change, message):
    l, h = vitl
    refused(l, l.leaf_score_pass(h, score_args(**change)), message)


def test_score_pass_refuses_a_null_handle_and_null_arguments(vitl):
    l, h = vitl
    refused(l, l.leaf_score_pass(None, score_args()), b"null/invalid")
    refused(l, l.leaf_score_pass(h, None), b"leaf_score_args")


def backward_args(**change):
    """the upstream head into the parameter gradients over 2 dense sequences; ``change`` makes it a call the entry refuses"""
    fields = dict(params=FAKE, w16_bwd=FAKE, tokens=FAKE, n_seq=2, feat=FAKE, head=_lib.HEAD_UPSTREAM, ref=FAKE, scale=1.0, stash=FAKE,
                  grads=FAKE, ws=FAKE, ws_bytes=1 << 20)
    fields.update(change)
    return _lib.BackwardArgs(**fields)


@pytest.mark.parametrize("change,message", [
    (dict(head=_lib.HEAD_FARE, d_embed=FAKE), b"head 0 takes"),                                       # FARE with both outputs
    (dict(head=_lib.HEAD_FARE, grads=None), b"null/invalid"),                                         # ... with neither
    (dict(head=_lib.HEAD_FARE, grads=None, d_embed=FAKE, scale=0.5), b"head 0 takes"),                # ... d_embed and scale != 1
    (dict(head=_lib.HEAD_COSINE), b"head 1 takes"),                                                   # COSINE with grads
    (dict(head=_lib.HEAD_COSINE, d_embed=FAKE), b"head 1 takes"),                                     # ... with both
    (dict(grads=None), b"null/invalid"),                                                              # UPSTREAM with neither output
    (dict(ref=None), b"null/invalid"),
    (dict(head=_lib.HEAD_FARE, ref=None), b"null/invalid"),
    (dict(seq_lens=C.addressof(LENS)), b"go together"),                                               # seq_lens without cu_rows
    (dict(cu_rows=FAKE), b"go together"),
    (dict(head=3), b"head 3 takes"),
    (dict(head=-1), b"head -1 takes"),
    (dict(n_seq=0), b"null/invalid"),
])
def test_text_backward_refusals(vitl, change, message):
    l, h = vitl
    refused(l, l.leaf_text_backward(h, backward_args(**change)), message)


def test_cosine_head_refuses_normalize_fare(vitl):
    l, h = vitl
    cosine = backward_args(head=_lib.HEAD_COSINE, grads=None, d_embed=FAKE)
    assert l.leaf_text_set_option(h, b"normalize_fare", 1) == 0
    try:
        refused(l, l.leaf_text_backward(h, cosine), b"normalize_fare off")
    finally:
        assert l.leaf_text_set_option(h, b"normalize_fare", 0) == 0
    refused(l, l.leaf_text_backward(None, cosine), b"null/invalid")


def train_fwd_args(**change):
    fields = dict(params=FAKE, w16_fwd=FAKE, tokens=FAKE, n_seq=2, out=FAKE, stash=FAKE, stash_bytes=1 << 20, ws=FAKE, ws_bytes=1 << 20)
    fields.update(change)
    return _lib.TrainFwdArgs(**fields)


@pytest.mark.parametrize("change,message", [
    (dict(pool_last=1, delta=FAKE, seq_lens=C.addressof(LENS), cu_rows=FAKE), b"pool_last takes no delta"),
    (dict(pool_last=1), b"pool_last needs explicit seq_lens"),                                        # pool_last without seq_lens
    (dict(pool_last=1, seq_lens=C.addressof(LENS), cu_rows=FAKE, ws=None), b"pool_last needs explicit seq_lens"),
    (dict(pool_last=1, seq_lens=C.addressof(LENS), cu_rows=FAKE, ws_bytes=2 * 768 * 4 - 1), b"workspace of n_seq x width floats"),
    (dict(seq_lens=C.addressof(LENS)), b"go together"),
    (dict(out=None), b"null/invalid"),
    (dict(n_seq=0), b"null/invalid"),
])
def test_forward_train_refusals(vitl, change, message):
    l, h = vitl
    refused(l, l.leaf_text_forward_train(h, train_fwd_args(**change)), message)


@pytest.mark.parametrize("name,make", [("leaf_score_args", score_args), ("leaf_train_fwd_args", train_fwd_args),
                                       ("leaf_backward_args", backward_args)])
@pytest.mark.parametrize("off", [-4, 4])
def test_entries_refuse_a_struct_of_another_size(vitl, name, make, off):
    l, h = vitl
    a = make()
    a.size += off
    refused(l, getattr(l, ENTRIES[name])(h, a), name.encode())


def test_chunk_option_keeps_its_range_check(vitl):
    l, h = vitl
    before = l.leaf_text_get_option(h, b"chunk")
    refused(l, l.leaf_text_set_option(h, b"chunk", 0), b"bad chunk")
    assert l.leaf_text_get_option(h, b"chunk") == before
    assert l.leaf_text_set_option(h, b"chunk", 64) == 0 and l.leaf_text_get_option(h, b"chunk") == 64
    assert l.leaf_text_set_option(h, b"chunk", before) == 0
