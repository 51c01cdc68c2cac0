"""Every row mode of the three forward attention kernel bodies against a float64 reference of the operation, at kernel scale:
attn_fwd_kernel and attn_edit_kernel (leaf_amd/csrc/attention.hip, through leaf_op_attention_fwd_map) and the fused QKV +
attention launch (qkv_attn.hip, through leaf_op_qkv_attn) -- packed rows, cached prefix, eot pooling, single-edit lookup, every
LDS image size (MAXT 2..6), the three work-item orders of the fused launch (hsplit 1, 2, 4) with one-tile and remainder tile
counts, the 256-sequence tile, the caption-count cut of the tile plan, the four- and five-K-tile loops.

Per case two things are asserted.
(a) float64, per row and per (row, head) 64-column slice: row_rel_l2 against the reference (tests/util.py: attn_assemble ->
    attn_seq_ref -> attn_slice; nn.MultiheadAttention of the assembled sequence).  The bound comes from the reference alone: twice
    the worst error, on the case's own inputs, of the ROUNDING MODEL -- the same float64 computation with P rounded to the operand
    type before P V and the output rounded to it, the two roundings the kernels are documented to make.  The factor 2 covers fp32
    accumulation order, v_exp / v_rcp at 1 ulp of fp32 and the rare 1-ulp flips of a q|k|v element of the fused launch.  No bound
    may exceed the whole-matrix thresholds of test_attention_fwd (2e-3 fp16, 1.2e-2 bf16).
(b) bits, between the paths that promise them (attention.hip "same body, same bits", qkv_attn.hip "a row has the same bits as from
    the stand-alone GEMM"): prefix-mode rows, edit-mode rows, the eot row, a plain packed launch on the fully assembled sequences,
    the old dense hook, and the fused launch against leaf_op_gemm_lnfold -> leaf_op_attention_fwd_map.

Every output is allocated between guard rows and prefilled with a NaN payload no kernel produces; after each launch every row the
mode must write is written, every other row and every guard row is untouched.

Worst "kernel error / rounding-model error" (worst row or slice of the kernel over worst row or slice of the model, per case;
1.0 = the kernel is exactly as good as its documented roundings, the bound is 2.0) measured on an MI355X:
                              fp16 row   fp16 slice   bf16 row   bf16 slice
    attn_fwd_kernel             1.000       1.000       1.002       1.002
    attn_edit_kernel            1.000       1.000       1.000       1.000
    fused QKV + attention       1.201       1.671       1.022       1.000
The two attention.hip kernels read given q|k|v rows and are as good as the model; the fused launch forms q|k|v itself, with fp32
accumulation where the reference rounds a float64 product: its worst cases (fp16, width 320 packed rows: slice 9.4e-4 against the
model's 5.6e-4; width 256 prefixed rows: row 5.3e-4 against 4.4e-4) are rows with a flipped last bit of a q|k|v element.  Every
bit-identity of (b) held in every case.
"""
import ctypes as C

import numpy as np
import pytest

from tests.util import attn_assemble, attn_seq_ref, attn_slice, lnfold_rows_ref, ptr, round16, row_rel_l2, stream

pytestmark = pytest.mark.gpu
DT = {"bf16": 0, "fp16": 1}
WHOLE = {"fp16": 2e-3, "bf16": 1.2e-2}      # test_attention_fwd's whole-matrix thresholds: no per-row bound may exceed them
SENT = 0x7FFD                               # a NaN payload (canonical NaNs are 0x7E00 / 0x7FC0; the kernels' packs saturate, never NaN)
GUARD = 4                                   # guard rows in front of and behind every output
LENS = [1, 2, 15, 16, 17, 31, 33, 48, 49, 64, 65, 77]
CAPS = [5, 20, 33, 64, 77]
GROUP = 7
TILE_ROWS, NCAP = 256, 3                    # the fused launch's M tile and caption images per tile (kernels.h)


@pytest.fixture(scope="module")
def env():
    import torch
    from leaf_amd import _lib
    assert torch.cuda.is_available()
    return _lib.lib(), torch, torch.device("cuda:0")


def _t16(torch, dtype):
    return torch.float16 if dtype == "fp16" else torch.bfloat16


def _dev16(env, x, dtype):
    """values already rounded to the operand type -> device tensor of that type (exact)"""
    _, torch, dev = env
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev).to(_t16(torch, dtype)).contiguous()


def _dev32(env, x, np_type):
    _, torch, dev = env
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, np_type)).to(dev)


def _qkv_rows(rng, n, d, dtype):
    x = rng.standard_normal((n, 3 * d)).astype(np.float32)
    x[:, :d] *= 2.0      # sharper softmax
    return round16(x, dtype)


class _Out:
    """[rows, d] output between guard rows, everything prefilled with the sentinel"""

    def __init__(self, env, dtype, rows, d):
        _, torch, dev = env
        self.rows, self.d = rows, d
        self.raw = torch.full(((rows + 2 * GUARD) * d,), SENT, dtype=torch.int16, device=dev)
        self.t = self.raw[GUARD * d: (GUARD + rows) * d].view(_t16(torch, dtype)).view(rows, d)

    def written(self, nw):
        """rows [0, nw) written in full, rows [nw, rows) and the guards untouched -> (tensor, float64 numpy) of the written rows"""
        raw = self.raw.cpu().numpy().reshape(-1, self.d)
        assert (raw[:GUARD] == SENT).all(), "guard rows in front of the output were written"
        assert (raw[GUARD + self.rows:] == SENT).all(), "guard rows behind the output were written"
        assert (raw[GUARD + nw: GUARD + self.rows] == SENT).all(), "rows this mode must not write were written"
        holes = np.argwhere(raw[GUARD: GUARD + nw] == SENT)
        assert holes.size == 0, f"{len(holes)} elements not written, first (row, column) {holes[:3].tolist()}"
        t = self.t[:nw].clone()
        return t, t.float().cpu().numpy().astype(np.float64)


def _launch_map(env, dtype, qkv, kv, heads, n_seq, ctx, n_written, cu=None, prefix=None, base_cu=None, eot=None, group=1, group_off=0,
                max_len=0, edit=0, spare_rows=3):
    lib, torch, dev = env
    from leaf_amd import _lib
    d = heads * 64
    out = _Out(env, dtype, n_written + spare_rows, d)
    i32 = [_dev32(env, v, np.int32) for v in (cu, prefix, base_cu, eot)]
    _lib.check(lib.leaf_op_attention_fwd_map(ptr(qkv), ptr(kv), ptr(out.t), ptr(i32[0]), ptr(i32[1]), ptr(i32[2]), ptr(i32[3]), n_seq, ctx,
                                             group, group_off, max_len, edit, heads, d, DT[dtype], stream()), "attention_fwd_map")
    torch.cuda.synchronize()
    return out.written(n_written)


def _check_a(label, dtype, heads, got, want, model):
    """(a): every row and every (row, head) slice of the kernel within twice the rounding model's worst on this case"""
    assert got.shape == want.shape == model.shape
    assert np.isfinite(got).all()
    d = heads * 64
    for tag, width in (("row", d), ("slice", 64)):
        w = want.reshape(-1, width)
        e_model = row_rel_l2(model.reshape(-1, width), w)
        e_kernel = row_rel_l2(got.reshape(-1, width), w)
        bound = 2.0 * e_model.max()
        print(f"ATTN_MODES {label} {dtype} {tag}: kernel {e_kernel.max():.3e} model {e_model.max():.3e} "
              f"ratio {e_kernel.max() / max(e_model.max(), 1e-300):.3f} ({len(w)} {tag}s)")
        assert bound <= WHOLE[dtype], f"{label} {tag}: the model's bound {bound:.3e} exceeds the whole-matrix threshold"
        worst = int(e_kernel.argmax())
        assert e_kernel.max() <= bound, f"{label} {tag} {worst} ({worst * width // d}, head {worst * width % d // 64}): " \
                                        f"{e_kernel.max():.3e} > 2 x model {e_model.max():.3e}"


def _eot_choice(prefix, tot):
    """pooled positions: first computed row, last row, the tile boundary (15, 16), a position that is not the last -- in turn"""
    eot = []
    for s, (p, t) in enumerate(zip(prefix, tot)):
        p, t = int(p), int(t)
        want = (p, t - 1, 15, 16, p + (t - 1 - p) // 2)[s % 5]
        eot.append(min(max(want, p), t - 1))
    return np.array(eot, np.int32)


def _cu(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


# =============================================================================================== attn_fwd_kernel: packed rows
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("longest", [16, 32, 48, 64, 80, 96])
def test_packed_mixed_lengths(env, dtype, longest):
    """Mixed lengths in one launch, max_len = the launch's true maximum: MAXT 2 (16, 32), 3, 4, 5, 6 each with shorter sequences
    (zeroed V rows behind their end) beside the longest one; eot rows without a prefix."""
    H = 3
    d = H * 64
    rng = np.random.default_rng(longest)
    ctx = 96 if longest == 96 else 77
    lens = [L for L in LENS + ([80, 96] if longest == 96 else []) if L <= longest]
    lens = [lens[i] for i in rng.permutation(len(lens))]
    n, rows = len(lens), sum(lens)
    own = _qkv_rows(rng, rows, d, dtype)
    seqs = attn_assemble(own, None, lens)
    exact = [attn_seq_ref(q, H) for q in seqs]
    model = [attn_seq_ref(q, H, dtype) for q in seqs]
    t = _dev16(env, own, dtype)
    got_t, got = _launch_map(env, dtype, t, None, H, n, ctx, rows, cu=_cu(lens), max_len=max(lens))
    _check_a(f"fwd packed<={longest}", dtype, H, got, attn_slice(exact), attn_slice(model))
    if longest == 80:       # the image sized by ctx instead: the same instantiation, the same bits
        again, _ = _launch_map(env, dtype, t, None, H, n, ctx, rows, cu=_cu(lens), max_len=0)
        assert env[1].equal(got_t, again)
    eot = _eot_choice(np.zeros(n, np.int32), lens)
    pool_t, pool = _launch_map(env, dtype, t, None, H, n, ctx, n, cu=_cu(lens), eot=eot, max_len=max(lens), spare_rows=rows)
    _check_a(f"fwd packed<={longest} eot", dtype, H, pool, attn_slice(exact, None, eot), attn_slice(model, None, eot))
    starts = _cu(lens)[:-1]
    assert env[1].equal(pool_t, got_t[env[1].from_numpy((starts + eot).astype(np.int64)).to(got_t.device)]), "eot row != the full launch's row"


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("L", [16, 48, 64, 77, 96])
def test_dense_hook_agrees_with_the_row_map_hook(env, dtype, L):
    """All lengths agree: the old dense hook, dense rows and packed rows through the new hook give the same bits"""
    lib, torch, dev = env
    from leaf_amd import _lib
    H, n = 3, 5
    d = H * 64
    rng = np.random.default_rng(1000 + L)
    own = _qkv_rows(rng, n * L, d, dtype)
    t = _dev16(env, own, dtype)
    old = _Out(env, dtype, n * L, d)
    _lib.check(lib.leaf_op_attention_fwd(ptr(t), ptr(old.t), n, L, H, d, DT[dtype], stream()), "attention_fwd")
    torch.cuda.synchronize()
    old_t, old_np = old.written(n * L)
    seqs = attn_assemble(own, None, [L] * n)
    _check_a(f"fwd dense L={L}", dtype, H, old_np, attn_slice([attn_seq_ref(q, H) for q in seqs]),
             attn_slice([attn_seq_ref(q, H, dtype) for q in seqs]))
    dense_t, _ = _launch_map(env, dtype, t, None, H, n, L, n * L)
    packed_t, _ = _launch_map(env, dtype, t, None, H, n, L, n * L, cu=_cu([L] * n), max_len=L)
    assert torch.equal(old_t, dense_t) and torch.equal(old_t, packed_t)


# =============================================================================================== cached prefix and single edit
def _captions(longest):
    caps = [L for L in CAPS + [90] if L <= longest]
    return caps, (96 if longest > 77 else 77)


def _prefixes(L):
    return [min(max(p, 0), L - 1) for p in (0, 1, 15, 16, 17, L - 2, L - 1)]


def _prefix_problem(rng, caps, ctx, d, dtype, group_off, edit):
    """Captions packed in the cache, GROUP candidates each with the prefixes of _prefixes; group_off > 0: the captions themselves in front.
    Row modes: the candidates' own rows are independent of the cache and their total lengths vary around the caption's.  Edit: a
    candidate is its caption with ONE fresh row (the table; NaN for the captions in front), one candidate per caption cut short."""
    base_cu = _cu(caps)
    cache = _qkv_rows(rng, int(base_cu[-1]), d, dtype)
    prefix, tot = [0] * group_off, list(caps[:group_off])
    for L in caps:
        for j, p in enumerate(_prefixes(L)):
            t = L - 1 if (edit and j == 2) else L if edit else L + (j % 3) - 1
            prefix.append(p)
            tot.append(min(max(t, p + 1), ctx, max(caps)))
    prefix, tot = np.array(prefix, np.int32), np.array(tot, np.int32)
    lens = tot - prefix
    if edit:
        own = _qkv_rows(rng, len(tot), d, dtype)
        own[:group_off] = np.nan
    else:
        own = _qkv_rows(rng, int(lens.sum()), d, dtype)
    seqs = attn_assemble(own, cache, lens, prefix, base_cu, GROUP, group_off, edit)
    return base_cu, cache, prefix, tot, lens, own, seqs


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("longest", [20, 33, 64, 77, 90])
@pytest.mark.parametrize("front", [False, True])
def test_cached_prefix(env, dtype, longest, front):
    """K/V of positions < prefix from the captions' cache (prefixes 0, 1, 15, 16, 17, len - 2, len - 1: not multiples of 16, later
    query tiles, the one-row sequence behind the longest prefix), group_off = 0 and the captions in front of the candidates; with
    and without eot_pos; the rows equal those of a plain packed launch on the assembled sequences.  MAXT 2, 3, 4, 5, 6."""
    torch = env[1]
    H = 2
    d = H * 64
    caps, ctx = _captions(longest)
    rng = np.random.default_rng(2000 + longest + front)
    group_off = len(caps) if front else 0
    base_cu, cache, prefix, tot, lens, own, seqs = _prefix_problem(rng, caps, ctx, d, dtype, group_off, False)
    n, rows = len(tot), int(lens.sum())
    exact = [attn_seq_ref(q, H) for q in seqs]
    model = [attn_seq_ref(q, H, dtype) for q in seqs]
    t, kv = _dev16(env, own, dtype), _dev16(env, cache, dtype)
    kw = dict(cu=_cu(lens), prefix=prefix, base_cu=base_cu, group=GROUP, group_off=group_off, max_len=int(tot.max()))
    label = f"fwd prefix<={longest} off={group_off}"
    got_t, got = _launch_map(env, dtype, t, kv, H, n, ctx, rows, **kw)
    _check_a(label, dtype, H, got, attn_slice(exact, prefix), attn_slice(model, prefix))
    eot = _eot_choice(prefix, tot)
    pool_t, pool = _launch_map(env, dtype, t, kv, H, n, ctx, n, eot=eot, spare_rows=rows, **kw)
    _check_a(label + " eot", dtype, H, pool, attn_slice(exact, prefix, eot), attn_slice(model, prefix, eot))
    # (b) a plain packed launch on the fully assembled sequences
    full = _dev16(env, np.concatenate(seqs), dtype)
    full_t, _ = _launch_map(env, dtype, full, None, H, n, ctx, int(tot.sum()), cu=_cu(tot), max_len=int(tot.max()))
    starts = _cu(tot)[:-1]
    keep = np.concatenate([np.arange(s + p, s + L) for s, p, L in zip(starts, prefix, tot)])
    idx = lambda a: torch.from_numpy(np.asarray(a, np.int64)).to(full_t.device)
    assert torch.equal(got_t, full_t[idx(keep)]), "prefix-mode rows != rows of the assembled sequences"
    assert torch.equal(pool_t, full_t[idx(starts + eot)]), "eot rows != rows of the assembled sequences"


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("longest", [20, 33, 64, 77, 90])
@pytest.mark.parametrize("front", [False, True])
def test_single_edit(env, dtype, longest, front):
    """attn_edit_kernel: one fresh row per candidate at position prefix[s]; every other position, before and behind it and Q included,
    from the cache; the captions in front of group_off from the cache alone (their table rows are NaN); with and without eot_pos.
    The same sequences in prefix mode and as plain packed rows give the same bits."""
    torch = env[1]
    H = 2
    d = H * 64
    caps, ctx = _captions(longest)
    rng = np.random.default_rng(3000 + longest + front)
    group_off = len(caps) if front else 0
    base_cu, cache, prefix, tot, lens, table, seqs = _prefix_problem(rng, caps, ctx, d, dtype, group_off, True)
    n, rows = len(tot), int(lens.sum())
    exact = [attn_seq_ref(q, H) for q in seqs]
    model = [attn_seq_ref(q, H, dtype) for q in seqs]
    t, kv = _dev16(env, table, dtype), _dev16(env, cache, dtype)
    kw = dict(cu=_cu(lens), prefix=prefix, base_cu=base_cu, group=GROUP, group_off=group_off, max_len=int(tot.max()))
    label = f"edit<={longest} off={group_off}"
    got_t, got = _launch_map(env, dtype, t, kv, H, n, ctx, rows, edit=1, **kw)
    _check_a(label, dtype, H, got, attn_slice(exact, prefix), attn_slice(model, prefix))
    eot = _eot_choice(prefix, tot)
    pool_t, pool = _launch_map(env, dtype, t, kv, H, n, ctx, n, eot=eot, edit=1, spare_rows=rows, **kw)
    _check_a(label + " eot", dtype, H, pool, attn_slice(exact, prefix, eot), attn_slice(model, prefix, eot))
    # (b) the same sequences in prefix mode (own rows = their positions >= prefix) ...
    suffix = _dev16(env, np.concatenate([q[p:] for q, p in zip(seqs, prefix)]), dtype)
    pre_t, _ = _launch_map(env, dtype, suffix, kv, H, n, ctx, rows, **kw)
    assert torch.equal(got_t, pre_t), "edit-mode rows != prefix-mode rows"
    # ... and as plain packed rows
    full = _dev16(env, np.concatenate(seqs), dtype)
    full_t, _ = _launch_map(env, dtype, full, None, H, n, ctx, int(tot.sum()), cu=_cu(tot), max_len=int(tot.max()))
    starts = _cu(tot)[:-1]
    keep = np.concatenate([np.arange(s + p, s + L) for s, p, L in zip(starts, prefix, tot)])
    idx = lambda a: torch.from_numpy(np.asarray(a, np.int64)).to(full_t.device)
    assert torch.equal(got_t, full_t[idx(keep)]), "edit-mode rows != rows of the assembled sequences"
    assert torch.equal(pool_t, full_t[idx(starts + eot)]), "eot rows != rows of the assembled sequences"


def test_single_edit_needs_a_cache(env):
    lib, torch, dev = env
    t = torch.zeros(4, 3 * 128, dtype=torch.float16, device=dev)
    out = torch.zeros(4, 128, dtype=torch.float16, device=dev)
    assert lib.leaf_op_attention_fwd_map(ptr(t), None, ptr(out), None, None, None, None, 4, 1, 1, 0, 0, 1, 2, 128, 1, stream()) != 0


# =============================================================================================== the fused QKV + attention launch
def _plan(lens, caption_of):
    """The greedy tile cut of qkv_attn.hip restated: whole sequences, <= TILE_ROWS rows, prefixed sequences of <= NCAP consecutive
    captions -> (first sequence of every tile, why each cut was made)"""
    first, why, rows, cap0 = [0], [], 0, -1
    for i, L in enumerate(lens):
        cap = -1 if caption_of is None else int(caption_of[i])
        by_rows = rows + L > TILE_ROWS
        by_caps = cap >= 0 and cap0 >= 0 and cap - cap0 >= NCAP
        if i > first[-1] and (by_rows or by_caps):
            first.append(i)
            why.append("rows" if by_rows else "captions")
            rows, cap0 = 0, -1
        rows += L
        if cap >= 0 and cap0 < 0:
            cap0 = cap
    return first, why


def _fused_row_map(rng, kind, d, dtype, n_dense=0):
    """-> lens, prefix, base_cu, cache of a row map of the fused launch (ctx = 77)"""
    if kind == "dense":
        return [77] * n_dense, None, None, None
    if kind == "packed":
        return [LENS[i] for i in rng.permutation(len(LENS))], None, None, None
    if kind == "ones":       # one tile of exactly 256 one-row sequences; a second tile of longer ones keeps the case's bound above zero
        return [1] * 256 + [33, 16, 77, 2], None, None, None
    assert kind == "prefix"
    base_cu = _cu(CAPS)
    cache = _qkv_rows(rng, int(base_cu[-1]), d, dtype)
    prefix, tot = [], []
    for L in CAPS:
        for j, p in enumerate(_prefixes(L)):
            prefix.append(p)
            tot.append(min(max(L + (j % 3) - 1, p + 1), 77))
    prefix = np.array(prefix, np.int32)
    return list(np.array(tot) - prefix), prefix, base_cu, cache


FUSED = [  # width, heads, hsplit of the launcher's rule, row map, dense sequences, tiles
    (256, 4, 1, "dense", 7, 3), (256, 4, 1, "packed", 0, 2), (256, 4, 1, "ones", 0, 2), (256, 4, 1, "prefix", 0, None),
    (320, 5, 1, "dense", 7, 3), (320, 5, 1, "packed", 0, 2), (320, 5, 1, "ones", 0, 2), (320, 5, 1, "prefix", 0, None),
    (640, 10, 2, "dense", 2, 1), (640, 10, 2, "dense", 13, 5), (640, 10, 2, "packed", 0, 2), (640, 10, 2, "prefix", 0, None),
    (1024, 16, 4, "dense", 2, 1), (1024, 16, 4, "dense", 7, 3), (1024, 16, 4, "ones", 0, 2), (1024, 16, 4, "prefix", 0, None),
]


def _fused_problem(dtype, width, H, hsplit, kind, n_dense, tiles):
    """The CPU side of a fused case: row map, operands, the assembled sequences"""
    d = width
    rng = np.random.default_rng(width + 7 * n_dense + len(kind))
    lens, prefix, base_cu, cache = _fused_row_map(rng, kind, d, dtype, n_dense)
    n, rows = len(lens), int(sum(lens))
    # the launcher's hsplit rule and the tile plan, restated: the case runs what its name says
    hs = 1
    for cand in (1, 2, 4):
        if H % cand:
            break
        hs = cand
        if (H // cand) * 192 * width * 2 <= 2 << 20:
            break
    assert hs == hsplit
    first, why = _plan(lens, None if prefix is None else np.arange(n) // GROUP)
    if tiles is not None:
        assert len(first) == tiles
    if hsplit > 1 and kind == "dense" and tiles > 1:
        assert tiles % (8 // hsplit) != 0
    if kind == "ones":
        assert first[:2] == [0, 256]
    if kind == "prefix":
        assert "captions" in why, "the plan must cut on the caption count before it cuts on rows"
    # operands: x16 rows with a mean, gamma-scaled weights (q rows x 2: sharper softmax), s and c as leaf_hip.h defines them
    x = round16(rng.standard_normal((rows, width)) * 1.5 + 0.3, dtype)
    wp = rng.standard_normal((3 * width, width)) / np.sqrt(width)
    wp[:width] *= 2.0
    wp = round16(wp, dtype)
    s_vec = wp.sum(-1).astype(np.float32)
    c_vec = (0.1 * rng.standard_normal(3 * width)).astype(np.float32)
    mean = x.mean(-1).astype(np.float32)
    rstd = (1.0 / np.sqrt(x.var(-1) + 1e-5)).astype(np.float32)
    own = lnfold_rows_ref(x, wp, s_vec, c_vec, mean, rstd, dtype)
    seqs = attn_assemble(own, cache, lens, prefix, base_cu, GROUP)
    return lens, prefix, base_cu, cache, x, wp, s_vec, c_vec, mean, rstd, seqs


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("width,H,hsplit,kind,n_dense,tiles", FUSED)
def test_fused_qkv_attention(env, dtype, width, H, hsplit, kind, n_dense, tiles):
    """qkv_attn.hip in every row map: K = 256 and 320 (four and five K tiles), hsplit 1, 2, 4 with one tile and with a tile count that
    leaves a remainder over 8 / hsplit, a tile of 256 one-row sequences, the caption-count cut, eot on packed and prefixed rows.
    (a) against the float64 LN-folded projection + attention; (b) the same bits as leaf_op_gemm_lnfold -> leaf_op_attention_fwd_map."""
    lib, torch, dev = env
    from leaf_amd import _lib
    d, ctx = width, 77
    lens, prefix, base_cu, cache, x, wp, s_vec, c_vec, mean, rstd, seqs = _fused_problem(dtype, width, H, hsplit, kind, n_dense, tiles)
    n, rows = len(lens), int(sum(lens))
    exact = [attn_seq_ref(q, H) for q in seqs]
    model = [attn_seq_ref(q, H, dtype) for q in seqs]
    pfx = prefix if prefix is not None else np.zeros(n, np.int32)
    tot = pfx + np.array(lens, np.int32)

    x_t, w_t = _dev16(env, x, dtype), _dev16(env, wp, dtype)
    c_t, s_t = _dev32(env, c_vec, np.float32), _dev32(env, s_vec, np.float32)
    rowstat = _dev32(env, np.stack([mean, rstd], 1), np.float32)
    kv = None if cache is None else _dev16(env, cache, dtype)
    cu_t, pfx_t, bcu_t = (_dev32(env, v, np.int32) for v in (_cu(lens), prefix, base_cu))
    lens_h = np.ascontiguousarray(lens, np.int32)
    tile_seq = torch.zeros(2 * (n + 2), dtype=torch.int32, device=dev)

    def fused(eot):
        nw = n if eot is not None else rows
        out = _Out(env, dtype, nw + (rows if eot is not None else 3), d)
        eot_t = _dev32(env, eot, np.int32)
        _lib.check(lib.leaf_op_qkv_attn(DT[dtype], ptr(x_t), ptr(w_t), ptr(c_t), ptr(s_t), ptr(rowstat), ptr(out.t), ptr(kv),
                                        C.c_void_p(lens_h.ctypes.data), ptr(cu_t), ptr(pfx_t), ptr(bcu_t), ptr(eot_t),
                                        ptr(tile_seq), n, rows, GROUP if prefix is not None else 1, ctx, H, width, stream()), "qkv_attn")
        torch.cuda.synchronize()
        return out.written(nw)

    # the chain the fused launch replaces: LN-folded QKV GEMM -> attention kernel on the same row map
    # (the stand-alone GEMMs take N % 128 == 0: width 320 runs with zero weight rows behind its 960, which no column in front sees)
    n_pad = (3 * d + 127) // 128 * 128
    pad = lambda t: torch.cat([t, torch.zeros(n_pad - 3 * d, *t.shape[1:], dtype=t.dtype, device=dev)]).contiguous()
    qkv = torch.zeros(rows, n_pad, dtype=_t16(torch, dtype), device=dev)
    w_p, c_p, s_p = pad(w_t), pad(c_t), pad(s_t)
    _lib.check(lib.leaf_op_gemm_lnfold(DT[dtype], -1, ptr(x_t), ptr(w_p), ptr(qkv), ptr(c_p), ptr(s_p), ptr(rowstat), rows, n_pad, width,
                                       stream()), "gemm_lnfold")
    torch.cuda.synchronize()
    qkv = qkv[:, :3 * d].contiguous()
    kw = dict(cu=_cu(lens), prefix=prefix, base_cu=base_cu, group=GROUP if prefix is not None else 1)
    label = f"fused {width}x{H} {kind}{n_dense or ''}"
    for eot in (None,) + ((_eot_choice(pfx, tot),) if kind in ("packed", "prefix") else ()):
        got_t, got = fused(eot)
        _check_a(label + (" eot" if eot is not None else ""), dtype, H, got, attn_slice(exact, pfx, eot), attn_slice(model, pfx, eot))
        chain_t, _ = _launch_map(env, dtype, qkv, kv, H, n, ctx, got.shape[0], eot=eot, **kw)
        assert torch.equal(got_t, chain_t), "fused launch != LN-folded GEMM -> attention kernel"
