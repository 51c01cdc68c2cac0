"""Single-edit scoring passes (include/leaf_hip.h "single-edit passes"; ``single_edit=True`` of LeafCLIPText.score_candidates*): block 0
projects ONE q|k|v row per candidate and reads every other row from layer 0 of the captions' cache.  Exact work skipping: winners,
losses and features are bit-identical to the same calls without the option and to full recomputation without prefix reuse.

Reference op: nn.MultiheadAttention inside ResidualAttentionBlock (src/open_clip/transformer.py:225,239-252); the candidates are the
single-token substitutions of SURVEY.md section 8d."""
import numpy as np
import pytest

from oracle import text_oracle as O
from tests.util import launch_families

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _model(name, seed, dtype="fp16", precision=None):
    from leaf_amd.model import create_model
    m = create_model(name, device="cuda:0", dtype=dtype, seed=seed)
    if precision is not None:
        m.set_precision(precision)
    return m


def _eq(torch_mod, a, b, what):
    for x, y, name in zip(a, b, ("winners", "features", "losses")):
        assert (x is None) == (y is None), f"{what}: {name}"
        if x is None:
            continue
        if not torch_mod.equal(x, y):
            d = (x.float() - y.float()).abs()
            raise AssertionError(f"{what}: {name} differ in {int((x != y).sum())} of {x.numel()} elements, max |diff| {float(d.max()):.3e}")


def _substitutions(base, rho, seed, pin=None):
    """[B, rho, ctx] single-token substitutions + their positions [B, rho]; the first candidates of every caption are the corner
    cases: position 1, the last position before EOT, and a drawn id equal to the caption's (no change at all).  ``pin`` (int [B])
    puts every candidate of a caption at one position (the search's second stage)."""
    rng = np.random.default_rng(seed)
    B = base.shape[0]
    eot = base.argmax(-1)
    cand = np.repeat(base[:, None, :], rho, axis=1).copy()
    pos = np.zeros((B, rho), dtype=np.int64)
    for b in range(B):
        for r in range(rho):
            p = int(pin[b]) if pin is not None else int(rng.integers(1, eot[b]))
            if pin is None and r == 0:
                p = 1
            if pin is None and r == 1:
                p = int(eot[b]) - 1
            pos[b, r] = p
            cand[b, r, p] = int(base[b, p]) if r == 2 else int(rng.integers(1, 49405))
    return cand, pos


def _two_stages(m, base, anchor, rho, seed, single_edit):
    """The search's two stages as leaf_amd.step.search_synthetic issues them: fused first stage (captions ride along, cache out),
    prepare / run second stage on that cache."""
    bl = base.argmax(-1) + 1
    lens = np.repeat(bl, rho)
    c1, p1 = _substitutions(base, rho, seed)
    got = m.score_candidates_fused(base, bl, c1.reshape(-1, 77), anchor, rho, lens, p1.reshape(-1), want_features=True, want_loss=True,
                                   single_edit=single_edit)
    assert got is not None
    i1, f1, cache, l1 = got
    win = p1[np.arange(base.shape[0]), i1.cpu().numpy()]
    c2, p2 = _substitutions(base, rho, seed + 1, pin=win)
    plan = m.score_candidates_prepare(c2.reshape(-1, 77), anchor, rho, "l2", want_features=True, want_loss=True, seq_lens=lens, kv=cache,
                                      single_edit=single_edit)
    i2, f2, l2 = m.score_candidates_run(plan, p2.reshape(-1))
    out = [x.clone() for x in (i1, f1, l1, i2, f2, l2)]
    full1 = m.score_candidates(c1.reshape(-1, 77), anchor, rho, "l2", want_loss=True, seq_lens=lens)
    full2 = m.score_candidates(c2.reshape(-1, 77), anchor, rho, "l2", want_loss=True, seq_lens=lens)
    return out, full1, full2


@pytest.mark.parametrize("model,dtype,precision,B,rho,min_len,max_len", [
    ("ViT-L-14-quickgelu", "fp16", "rowsafe", 40, 50, 1, 40),      # big passes: the fused launch runs blocks 1 .. layers - 1
    ("ViT-L-14-quickgelu", "fp16", "fast", 40, 50, 1, 40),
    ("ViT-L-14-quickgelu", "fp16", "rowsafe", 5, 7, 1, 12),        # small passes: GEMM + attention kernel in every block
    ("ViT-H-14", "bf16", None, 12, 13, 1, 60),
    ("tiny-test", "fp16", None, 6, 7, 1, 30),
])
def test_single_edit_is_bit_identical(torch_mod, monkeypatch, model, dtype, precision, B, rho, min_len, max_len):
    monkeypatch.setenv("LEAF_VERIFY_SINGLE_EDIT", "1")
    m = _model(model, 3, dtype, precision)
    base = O.synthetic_tokens(B, seed=31, min_len=min_len, max_len=max_len)
    base[0, :] = 0
    base[0, :3] = (49406, 1234, 49407)            # a one-token caption: SOT, token, EOT
    anchor = m.encode_text(base) + 0.2
    on, full1, full2 = _two_stages(m, base, anchor, rho, 41, True)
    off, _, _ = _two_stages(m, base, anchor, rho, 41, False)
    _eq(torch_mod, on[:3], off[:3], "first stage, single_edit on / off")
    _eq(torch_mod, on[3:], off[3:], "second stage, single_edit on / off")
    _eq(torch_mod, on[:3], full1, "first stage against full recomputation")
    _eq(torch_mod, on[3:], full2, "second stage against full recomputation")


def test_single_edit_pass_above_16384_rows(torch_mod):
    """A large second-stage pass, above 16,384 suffix rows: its 1,600 sequences fit one row-budget chunk, and every GEMM of it is a
    launch of more than 128 tiles of 256^2.  With the option and without it, the pass equals the full recomputation bit for bit."""
    m = _model("ViT-L-14-quickgelu", 4)
    B, rho = 32, 50
    base = O.synthetic_tokens(B, seed=33, min_len=30, max_len=60)
    bl = base.argmax(-1) + 1
    lens = np.repeat(bl, rho)
    cand, pos = _substitutions(base, rho, 43, pin=np.full(B, 2))
    assert int((lens - pos.reshape(-1)).sum()) > 16384
    anchor = m.encode_text(base) + 0.1
    kv = m.encode_text_kv(base)
    flat = cand.reshape(-1, 77)
    full = m.score_candidates(flat, anchor, rho, "l2", want_loss=True, seq_lens=lens)
    res = {}
    for se in (False, True):
        res[se] = [x.clone() for x in m.score_candidates(flat, anchor, rho, "l2", want_loss=True, seq_lens=lens,
                                                         prefix_lens=pos.reshape(-1), kv=kv, single_edit=se)]
    _eq(torch_mod, res[True], res[False], "single_edit on / off")
    for se, r in res.items():
        _eq(torch_mod, r, full, f"single_edit = {se} against full recomputation")


@pytest.mark.parametrize("precision", ["rowsafe", "fast"])
def test_single_edit_replaces_the_fused_launch_of_block_0(torch_mod, precision):
    """With the option on a scoring stage issues layers - 1 fused QKV + attention launches (profiler family 8) and none over the
    split K = 3d; with it off, layers (block 0 of the default arithmetic over K = 3d)."""
    m = _model("ViT-L-14-quickgelu", 1, precision=precision)
    B, rho = 32, 50
    d, L = m.cfg.width, m.cfg.layers
    base = O.synthetic_tokens(B, seed=95, min_len=8, max_len=40)
    bl = base.argmax(-1) + 1
    lens = np.repeat(bl, rho)
    cand, pos = _substitutions(base, rho, 96)
    flat = cand.reshape(-1, 77)
    anchor = m.encode_text(base)
    kv = m.encode_text_kv(base)

    def stage2(se):
        return lambda: m.score_candidates(flat, anchor, rho, "l2", seq_lens=lens, prefix_lens=pos.reshape(-1), kv=kv, single_edit=se)

    def stage1(se):
        return lambda: m.score_candidates_fused(base, bl, flat, anchor, rho, lens, pos.reshape(-1), single_edit=se)

    for stage in (stage2, stage1):      # stage 2 first: the fused first stage rewrites the slot that ``kv`` names
        off = launch_families(stage(False))
        on = launch_families(stage(True))
        fused = lambda f: sum(c for (fam, e, N, K), c in f.items() if fam == 8 and N == 3 * d)
        fused_k3 = lambda f: sum(c for (fam, e, N, K), c in f.items() if fam == 8 and N == 3 * d and K == 3 * d)
        assert fused(off) == L, off
        assert fused_k3(off) == (1 if precision == "rowsafe" else 0), off
        assert fused(on) == L - 1 and fused_k3(on) == 0, on


def test_single_edit_refuses_a_cache_without_layer_0_q(torch_mod):
    m = _model("ViT-L-14-quickgelu", 2)
    B, rho = 6, 9
    base = O.synthetic_tokens(B, seed=51, min_len=4, max_len=20)
    bl = base.argmax(-1) + 1
    lens = np.repeat(bl, rho)
    cand, pos = _substitutions(base, rho, 52)
    flat = cand.reshape(-1, 77)
    anchor = m.encode_text(base)
    _, _, cache = m.score_candidates_fused(base, bl, flat, anchor, rho, lens, pos.reshape(-1))         # option off: K and V only
    with pytest.raises(ValueError, match="layer-0 Q"):
        m.score_candidates(flat, anchor, rho, "l2", seq_lens=lens, prefix_lens=pos.reshape(-1), kv=cache, single_edit=True)
    m.score_candidates(flat, anchor, rho, "l2", seq_lens=lens, prefix_lens=pos.reshape(-1), kv=cache)   # ... which serves a plain pass
    assert m._lib.leaf_text_get_option(m._h, b"single_edit") == 0
    _, _, cache = m.score_candidates_fused(base, bl, flat, anchor, rho, lens, pos.reshape(-1), single_edit=True)
    m.score_candidates(flat, anchor, rho, "l2", seq_lens=lens, prefix_lens=pos.reshape(-1), kv=cache, single_edit=True)
    assert m._lib.leaf_text_get_option(m._h, b"single_edit") == 0          # the option is per pass


def test_single_edit_verification_catches_a_second_edit(torch_mod, monkeypatch):
    monkeypatch.setenv("LEAF_VERIFY_SINGLE_EDIT", "1")
    m = _model("tiny-test", 2)
    B, rho = 4, 5
    base = O.synthetic_tokens(B, seed=61, min_len=6, max_len=20)
    bl = base.argmax(-1) + 1
    lens = np.repeat(bl, rho)
    cand, pos = _substitutions(base, rho, 62)
    cand[1, 3, int(pos[1, 3]) + 1 if pos[1, 3] + 1 < bl[1] - 1 else 1] += 1     # a second changed token
    anchor = m.encode_text(base)
    kv = m.encode_text_kv(base)
    with pytest.raises(ValueError, match="differs from its caption"):
        m.score_candidates(cand.reshape(-1, 77), anchor, rho, "l2", seq_lens=lens, prefix_lens=pos.reshape(-1), kv=kv, single_edit=True)
