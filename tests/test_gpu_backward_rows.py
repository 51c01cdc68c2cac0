"""The kernels of the training backward on the packed row map that leaf_text_backward (leaf_amd/csrc/api_train.hip) builds, each alone
through its hook and against a float64 reference of the operation (tests/util.py, pinned by tests/test_backward_ref_cpu.py):
attn_bwd_mfma_kernel (attention_bwd.hip), the projection + ln_final backward, the embedding scatter, the TextFARE loss head and the
fp16 saturation check (train.hip).  test_layernorm_bwd (tests/test_gpu_kernels.py) holds ln_bwd_kernel to the same rules.

Bounds come from the references alone.
  * 16-bit outputs (attention backward): per row (width 3d) and per (row, 64-column slice) -- dq, dk, dv of each head apart -- the
    relative L2 error against float64 is at most 2 x the worst such error, on the same pack, of the ROUNDING MODEL: the float64
    computation with the kernel's three documented roundings to the gradient type (P before P^T dO, dS before its two products, the
    output).  The factor 2 covers fp32 accumulation order and v_exp / v_rcp.  The bound itself may not exceed the whole-matrix
    tolerances of test_attention_bwd_mfma (2e-3 fp16 gradients, 1.2e-2 bf16).
  * fp32 sums of n terms (dproj, dg, db, dtok, dpos, the loss, dout): |got - want| <= 2 (n + 2) 2^-24 sum|terms| per element, the
    sum of absolute terms evaluated in float64 (n counts every accumulation of the chain behind the element).
  * fp32 LayerNorm-backward rows: no row's relative error exceeds 4 x the worst row error of the same formula in numpy float32.
Every output that is only partly written starts from a sentinel bit pattern (or random values for accumulators) between guard rows.

Worst "kernel error / model error" measured on an MI355X (worst row or slice of the kernel over the model's; the bound is 2.0,
for the LayerNorm rows 4.0):
    attn_bwd_mfma_kernel, all four (forward, gradient) pairs, H = 1, 2, 12, ctx 77 / 96: row 1.000, slice 1.000 (the worst rows are
        those whose error is the output rounding alone, which kernel and model make alike; with dO x 2^10 the worst slice is 0.834 ..
        1.000); worst bounds in use 2 x 6.5e-4 (fp16 gradients) and 2 x 4.7e-3 (bf16)
    pool_ln_bwd_kernel rows (bound 4.0): 1.02
    worst error / derived accumulation bound (1.0 = the bound): dproj 0.245, dg 0.001, db 0.001, dtok 0.204, dpos 0.151, loss 0.007,
        dout 0.372
Every bit-identity held in every case.

Mutations (values only, each built apart and never kept) and the assertion that caught them:
    mask `kidx >= qv` in attn_bwd_mfma_kernel: the per-row bound of test_attention_bwd_on_packed_rows (error 1.0 on row 0)
    tok_bwd_kernel's `hit` without the kept-slot test: the dtok bound of test_embed_bwd[9-128-False] (an id whose first slot lies
        behind a sequence's end loses its rows)
    proj_wgrad_kernel without the reset of `acc` per 1,024-column pass: the dproj bound of test_pool_project_bwd[260-128-1280]
    ln_bwd_kernel zeroing `mine` inside the row loop: the dg / db check of test_layernorm_bwd at the shapes past the grid cap
    `inv = 1 / sum` for padded query rows in attn_bwd_mfma_kernel: caught by NOTHING, and cannot be: the Q and dO images in LDS are
        zero behind the sequence's last row, so a padded query row's P and dS meet zero operands in dK^T += Q^T dS and dV^T += dO^T P,
        and its dq is never stored.  The two guards are redundant by design; all 20 attention cases give the same bits either way.
"""
import ctypes as C

import numpy as np
import pytest

from tests.util import (BWD_LENS, attn_bwd_pack, embed_bwd_ref, fare_ref, pool_project_bwd_ref, ptr, row_rel_l2, stream)

pytestmark = pytest.mark.gpu
DT = {"bf16": 0, "fp16": 1}
WHOLE = {"fp16": 2e-3, "bf16": 1.2e-2}      # test_attention_bwd_mfma's whole-matrix tolerances, by gradient type
SENT16 = 0x7FFD                             # a 16-bit NaN payload no kernel produces (the packs saturate, never NaN)
SENT32 = 0x7FC0BEEF                         # ... and an fp32 one
GUARD = 16
U = 2.0 ** -24                              # unit roundoff of fp32
PAIRS = [("fp16", "fp16"), ("fp16", "bf16"), ("bf16", "fp16"), ("bf16", "bf16")]
SUB77 = [L for L in BWD_LENS if L <= 77]


@pytest.fixture(scope="module")
def env():
    import torch
    from leaf_amd import _lib
    assert torch.cuda.is_available()
    return _lib.lib(), torch, torch.device("cuda:0")


def _t16(torch, dtype):
    return torch.float16 if dtype == "fp16" else torch.bfloat16


def _dev16(env, x, dtype):
    """values already rounded to the 16-bit type -> device tensor of that type (exact)"""
    _, torch, dev = env
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev).to(_t16(torch, dtype)).contiguous()


def _dev(env, x, np_type=np.float32):
    _, torch, dev = env
    return torch.from_numpy(np.ascontiguousarray(x, np_type)).to(dev)


def _cu(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _acc_ok(label, got, want, n_terms, abs_terms):
    """the derived bound of an fp32 accumulation: |got - want| <= 2 (n + 2) 2^-24 sum|terms|, per element"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), label
    bound = 2.0 * (np.asarray(n_terms, np.float64) + 2.0) * U * np.asarray(abs_terms, np.float64)
    err = np.abs(got - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"BWD_ROWS {label}: worst error / derived bound {ratio:.3f}")
    worst = np.unravel_index(int((err - bound).argmax()), err.shape)
    assert (err <= bound).all(), f"{label}: element {worst}: |{got[worst]} - {want[worst]}| = {err[worst]:.3e} > {np.broadcast_to(bound, err.shape)[worst]:.3e}"


def _rows_ok(label, got, want, model, factor, widths, cap=None):
    """every row (and slice) of the kernel within `factor` x the model's worst on the same inputs"""
    assert got.shape == want.shape == model.shape
    assert np.isfinite(got).all(), label
    for width in widths:
        w = want.reshape(-1, width)
        e_model, e_kernel = row_rel_l2(model.reshape(-1, width), w), row_rel_l2(got.reshape(-1, width), w)
        bound = factor * e_model.max()
        print(f"BWD_ROWS {label} width {width}: kernel {e_kernel.max():.3e} model {e_model.max():.3e} "
              f"ratio {e_kernel.max() / max(e_model.max(), 1e-300):.3f} ({len(w)} rows)")
        if cap is not None:
            assert bound <= cap, f"{label} width {width}: the model's bound {bound:.3e} exceeds the whole-matrix tolerance {cap}"
        worst = int(e_kernel.argmax())
        assert e_kernel.max() <= bound, f"{label} width {width}: row/slice {worst}: {e_kernel.max():.3e} > {factor} x model {e_model.max():.3e}"


# =============================================================================================== (a) attention backward
def _attn_launch(env, ft, gt, qkv_t, do_t, H, lens, ctx, dense=False):
    """one launch into a sentinel-filled [rows, 3d] buffer between guard rows -> the written rows (device tensor); guards checked"""
    lib, torch, dev = env
    from leaf_amd import _lib
    d, rows, n = H * 64, int(sum(lens)), len(lens)
    raw = torch.full(((rows + 2 * GUARD) * 3 * d,), SENT16, dtype=torch.int16, device=dev)
    out = raw[GUARD * 3 * d: (GUARD + rows) * 3 * d].view(_t16(torch, gt)).view(rows, 3 * d)
    if dense:
        assert all(L == ctx for L in lens)
        _lib.check(lib.leaf_op_attention_bwd_t(ptr(qkv_t), DT[ft], ptr(do_t), ptr(out), DT[gt], n, ctx, H, d, stream()), "attention_bwd_t")
    else:
        cu = _dev(env, _cu(lens), np.int32)
        _lib.check(lib.leaf_op_attention_bwd_map(ptr(qkv_t), DT[ft], ptr(do_t), ptr(out), DT[gt], ptr(cu), n, ctx, H, d, stream()),
                   "attention_bwd_map")
    torch.cuda.synchronize()
    bits = raw.cpu().numpy().reshape(-1, 3 * d)
    assert (bits[:GUARD] == SENT16).all(), "guard rows in front of the output were written"
    assert (bits[GUARD + rows:] == SENT16).all(), "guard rows behind the last packed row were written"
    holes = np.argwhere(bits[GUARD: GUARD + rows] == SENT16)
    assert holes.size == 0, f"{len(holes)} elements not written, first (row, column) {holes[:3].tolist()}"
    return out.clone()


@pytest.mark.parametrize("ft,gt", PAIRS)
@pytest.mark.parametrize("H,lens,ctx", [(1, BWD_LENS, 96), (2, BWD_LENS, 96), (1, SUB77, 77), (2, SUB77, 77), (12, [1, 17, 77], 77)],
                         ids=["H1-ctx96", "H2-ctx96", "H1-ctx77", "H2-ctx77", "H12-ctx77"])
def test_attention_bwd_on_packed_rows(env, H, lens, ctx, ft, gt):
    """Mixed lengths in one launch: every tile count 1..6, each 16-row boundary - 1, + 0, + 1, L = 1 and L = 2; all four
    (forward, gradient) type pairs.  Bit-identities: the kernel owns one wave per (sequence, head) and loops on the sequence's own tile
    count, so a sequence's rows cannot depend on its neighbours, on ctx, or on dense / packed addressing."""
    _, torch, _ = env
    d = H * 64
    qkv, do, exact, model = attn_bwd_pack(5, lens, H, ft, gt)
    tq, tdo = _dev16(env, qkv, ft), _dev16(env, do, gt)
    got_t = _attn_launch(env, ft, gt, tq, tdo, H, lens, ctx)
    got = got_t.float().cpu().numpy().astype(np.float64)
    label = f"attn_bwd ({ft},{gt}) H={H} ctx={ctx}"
    _rows_ok(label, got, exact, model, 2.0, (3 * d, 64), cap=WHOLE[gt])
    cu = _cu(lens)
    # position 0 attends to itself alone: P = 1 and dP - rowsum(P o dP) = dp - fma(1, dp, 0) is zero in the kernel's own arithmetic
    assert not got[cu[:-1], :d].any(), "dq of a sequence's position 0 is not exactly zero"
    # a sequence launched alone, the dense hook at L = ctx, another ctx
    for s, L in enumerate(lens):
        a, b = int(cu[s]), int(cu[s + 1])
        alone = _attn_launch(env, ft, gt, tq[a:b], tdo[a:b], H, [L], ctx)
        assert torch.equal(alone.view(torch.int16), got_t[a:b].view(torch.int16)), f"sequence {s} (L = {L}) differs from its launch alone"
        if L == ctx:
            dense = _attn_launch(env, ft, gt, tq[a:b], tdo[a:b], H, [L], ctx, dense=True)
            assert torch.equal(dense.view(torch.int16), alone.view(torch.int16)), f"L = ctx = {L}: the dense hook gives other bits"
    assert ctx in lens
    if ctx == 77:
        wide = _attn_launch(env, ft, gt, tq, tdo, H, lens, 96)
        assert torch.equal(wide.view(torch.int16), got_t.view(torch.int16)), "the same pack under ctx = 96 gives other bits"
    if gt == "fp16":
        # the loss scale: dO x 2^10 (exact in fp16) gives 2^10 x the unscaled gradient, within the same bound
        up = _attn_launch(env, ft, gt, tq, _dev16(env, do * 1024.0, gt), H, lens, ctx)
        up = up.float().cpu().numpy().astype(np.float64) / 1024.0
        _rows_ok(label + " dO x 2^10", up, exact, model, 2.0, (3 * d, 64), cap=WHOLE[gt])
        assert not up[cu[:-1], :d].any()


# =============================================================================================== (c) projection + ln_final backward
def _sent32(env, n):
    _, torch, dev = env
    return torch.full((n,), SENT32, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("n_seq,d,D", [(7, 128, 128), (13, 768, 768), (260, 128, 1280), (3, 2048, 1024), (9, 1280, 1280)])
def test_pool_project_bwd(env, n_seq, d, D):
    """text_projection + ln_final backward on the pooled rows of a packed map (proj_wgrad_kernel, dpooled_kernel, pool_ln_bwd_kernel,
    pool_ln_wgrad_kernel): 7 = the tail loop of the 8-caption unroll alone, 13 = body + tail, 260 x 1280 = the second 256-caption
    window and the second 1,024-column pass of proj_wgrad_kernel, 2048 = 8 float4 chunks per lane; the pooled position is 0, the last
    row or an interior row of its sequence."""
    lib, torch, dev = env
    from leaf_amd import _lib
    rng = np.random.default_rng(n_seq + d + D)
    ctx, eps, S = 77, 1e-5, 8.0
    lens = np.concatenate([[1, 77, 40], rng.integers(1, 78, size=n_seq)])[:n_seq].astype(np.int64)
    cu = _cu(lens)
    rows = int(cu[-1])
    eot = np.array([(0, L - 1, L // 2)[s % 3] for s, L in enumerate(lens)], np.int32)
    assert (eot == 0).any() and (eot == lens - 1).any() and ((eot > 0) & (eot < lens - 1)).any()
    x = (rng.standard_normal((rows, d)) * 2 + 0.3).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d)).astype(np.float32)
    proj = (rng.standard_normal((d, D)) / np.sqrt(d)).astype(np.float32)
    dout = rng.standard_normal((n_seq, D)).astype(np.float32)
    dproj0, dg0, db0 = (rng.standard_normal(s).astype(np.float32) for s in ((d, D), d, d))
    pool_rows = cu[:-1] + eot
    xe = x[pool_rows]
    ref = pool_project_bwd_ref(dout, xe, g, b, eps, proj)
    model = pool_project_bwd_ref(dout, xe, g, b, eps, proj, dtype=np.float32)
    pooled = ref["pooled"].astype(np.float32)          # what the forward stashes: fp32 LN_final of the pooled rows
    dout64, pooled64 = dout.astype(np.float64), pooled.astype(np.float64)

    t = {k: _dev(env, v) for k, v in dict(dout=dout, pooled=pooled, x=x, g=g, proj=proj, dproj=dproj0, dg=dg0, db=db0).items()}
    t_eot, t_cu = _dev(env, eot, np.int32), _dev(env, cu, np.int32)
    gs = _dev(env, np.array([S, 1.0 / S], np.float32))
    scratch = torch.zeros(n_seq * (d + 2), dtype=torch.float32, device=dev)

    def launch(with_params):
        raw = _sent32(env, (rows + 2 * GUARD) * d)
        dx = raw[GUARD * d: (GUARD + rows) * d]
        p = [ptr(t[k]) if with_params else None for k in ("dproj", "dg", "db")]
        _lib.check(lib.leaf_op_pool_project_bwd(ptr(t["dout"]), ptr(t["pooled"]), ptr(t["x"]), ptr(t_eot), ptr(t["g"]), eps, ptr(t["proj"]),
                                                ptr(dx), p[0], p[1], p[2], ptr(gs), ptr(t_cu), n_seq, ctx, d, D, ptr(scratch), stream()),
                   "pool_project_bwd")
        torch.cuda.synchronize()
        return raw.cpu().numpy().reshape(rows + 2 * GUARD, d)

    bits = launch(True)
    sent = np.int32(SENT32)
    other = np.ones(rows + 2 * GUARD, bool)
    other[GUARD + pool_rows] = False
    assert (bits[other] == sent).all(), "a row of dx that is not a pooled row (or a guard row) was written"
    got_dx = bits[GUARD + pool_rows].view(np.float32).astype(np.float64) / S
    label = f"pool_project_bwd n={n_seq} d={d} D={D}"
    _rows_ok(label + " dx", got_dx, ref["dx"], model["dx"].astype(np.float64), 4.0, (d,))
    _acc_ok(label + " dproj", t["dproj"].cpu().numpy(), dproj0 + pooled64.T @ dout64, n_seq + 1,
            np.abs(dproj0) + np.abs(pooled64).T @ np.abs(dout64))
    _acc_ok(label + " dg", t["dg"].cpu().numpy(), dg0 + ref["dg"], n_seq + D + d + 1, np.abs(dg0) + ref["abs_dg"])
    _acc_ok(label + " db", t["db"].cpu().numpy(), db0 + ref["db"], n_seq + D + 1, np.abs(db0) + ref["abs_db"])
    # input gradient only: the same dx bits, the parameter gradients untouched
    keep = {k: t[k].clone() for k in ("dproj", "dg", "db")}
    again = launch(False)
    assert np.array_equal(again, bits), "dx depends on whether the parameter gradients are asked for"
    assert all(torch.equal(keep[k], t[k]) for k in keep)


# =============================================================================================== (d) embedding backward
HEAVY, FAR, GHOST = 3, 5, 7     # ids with > 256 kept rows / two rows > 256 slots apart / slots behind the sequences' ends only


def _embed_lens(n_seq):
    if n_seq == 3:
        return [77, 30, 1]
    if n_seq == 9:
        return [77, 1, 40, 16, 77, 5, 33, 64, 2]
    return [77, 60, 77, 1, 45, 77, 16, 70, 77, 33, 77, 2, 64, 77, 50, 77, 17, 77, 31, 77, 65, 48, 77, 15][:n_seq]


def _embed_tokens(rng, lens, ctx, vocab):
    """ordinary ids in [16, vocab - 16), then the special ones on kept slots (GHOST: only behind the ends)"""
    n = len(lens)
    tok = rng.integers(16, vocab - 16, size=(n, ctx)).astype(np.int32)
    kept = [(s, p) for s in range(n) for p in range(lens[s])]
    for s in range(n):
        tok[s, lens[s]::2] = GHOST
    special = {}
    far = [i for i, (s, p) in enumerate(kept) if s * ctx + p > 256 + 8]
    if far:
        special[0], special[far[0]] = FAR, FAR          # kept[0] is slot 0
    for i, v in ((1, -3), (len(kept) // 2, -3), (2, vocab + 5), (len(kept) - 1, vocab + 5)):
        special.setdefault(i, v)
    for i in range(len(kept)):
        if i % 3 == 1:
            special.setdefault(i, HEAVY)
    for i, v in special.items():
        tok[kept[i]] = v
    return tok


@pytest.mark.parametrize("n_seq,d,dense", [(9, 128, False), (24, 1280, False), (3, 768, False), (24, 1280, True)])
def test_embed_bwd(env, n_seq, d, dense):
    """tok_bwd_kernel (first-row owner, 256-slot windows, kept slots only) and pos_bwd_kernel (8-sequence unroll + tail) against the
    float64 scatter.  Packed rows: slots behind a sequence's end do not count; dense rows (cu NULL): every slot counts."""
    lib, torch, dev = env
    from leaf_amd import _lib
    rng = np.random.default_rng(n_seq + d)
    ctx, vocab, S = 77, 512, 8.0
    true_lens = _embed_lens(n_seq)
    tok = _embed_tokens(rng, true_lens, ctx, vocab)
    lens = [ctx] * n_seq if dense else true_lens
    rows = int(sum(lens))
    dx = (S * rng.standard_normal((rows, d))).astype(np.float32)
    dtok0, dpos0 = rng.standard_normal((vocab, d)).astype(np.float32), rng.standard_normal((ctx, d)).astype(np.float32)
    sum_tok, sum_pos, abs_tok, abs_pos, count = embed_bwd_ref(dx, tok, lens, ctx, vocab)
    # the token layout holds what the test is about
    if n_seq == 24:
        assert count[HEAVY] > 256
    if n_seq >= 9:
        slots = np.flatnonzero((tok == FAR).reshape(-1))
        assert count[FAR] == 2 and slots[1] - slots[0] > 256
    assert (tok == GHOST).any() and (count[GHOST] == 0) == (not dense)
    assert count[0] == 2 and count[vocab - 1] == 2 and (tok == -3).sum() == 2 and (tok == vocab + 5).sum() == 2     # tok_clamp's rows
    assert (count[16: vocab - 16] == 1).any() and (count[16: vocab - 16] == 0).any()

    t_dx, t_tok = _dev(env, dx), _dev(env, tok, np.int32)
    t_cu = None if dense else _dev(env, _cu(lens), np.int32)
    gs = _dev(env, np.array([S, 1.0 / S], np.float32))

    def launch():
        dtok, dpos = _dev(env, dtok0), _dev(env, dpos0)
        _lib.check(lib.leaf_op_embed_bwd(ptr(t_dx), ptr(gs), ptr(t_tok), ptr(dtok), ptr(dpos), ptr(t_cu), rows, n_seq, ctx, d, vocab,
                                         stream()), "embed_bwd")
        torch.cuda.synchronize()
        return dtok.cpu().numpy(), dpos.cpu().numpy()

    dtok, dpos = launch()
    label = f"embed_bwd n={n_seq} d={d} {'dense' if dense else 'packed'}"
    _acc_ok(label + " dtok", dtok, dtok0 + sum_tok / S, count[:, None] + 1, np.abs(dtok0) + abs_tok / S)
    _acc_ok(label + " dpos", dpos, dpos0 + sum_pos / S, n_seq + 1, np.abs(dpos0) + abs_pos / S)
    absent = count == 0
    assert absent.any() and np.array_equal(dtok[absent].view(np.int32), dtok0[absent].view(np.int32)), "the dtok row of an absent id changed"
    dtok2, dpos2 = launch()
    assert np.array_equal(dtok.view(np.int32), dtok2.view(np.int32)) and np.array_equal(dpos.view(np.int32), dpos2.view(np.int32))


def test_embed_bwd_leaves_positions_behind_the_longest_sequence(env):
    """no sequence of the pack reaches position 40: dpos rows 40.. keep their bits"""
    lib, torch, dev = env
    from leaf_amd import _lib
    rng = np.random.default_rng(40)
    ctx, vocab, d, S = 77, 512, 128, 8.0
    lens = [40, 1, 17, 33, 40, 2, 16, 39, 5, 21, 8]           # one unrolled group of eight sequences + a tail of three
    tok = rng.integers(0, vocab, size=(len(lens), ctx)).astype(np.int32)
    rows = sum(lens)
    dx = (S * rng.standard_normal((rows, d))).astype(np.float32)
    dtok0, dpos0 = rng.standard_normal((vocab, d)).astype(np.float32), rng.standard_normal((ctx, d)).astype(np.float32)
    sum_tok, sum_pos, abs_tok, abs_pos, count = embed_bwd_ref(dx, tok, lens, ctx, vocab)
    dtok, dpos = _dev(env, dtok0), _dev(env, dpos0)
    gs = _dev(env, np.array([S, 1.0 / S], np.float32))
    t_dx, t_tok, t_cu = _dev(env, dx), _dev(env, tok, np.int32), _dev(env, _cu(lens), np.int32)
    _lib.check(lib.leaf_op_embed_bwd(ptr(t_dx), ptr(gs), ptr(t_tok), ptr(dtok), ptr(dpos), ptr(t_cu), rows, len(lens), ctx, d, vocab,
                                     stream()), "embed_bwd")
    torch.cuda.synchronize()
    dtok, dpos = dtok.cpu().numpy(), dpos.cpu().numpy()
    assert np.array_equal(dpos[40:].view(np.int32), dpos0[40:].view(np.int32)), "a position no sequence reaches changed"
    _acc_ok("embed_bwd short pack dpos", dpos, dpos0 + sum_pos / S, len(lens) + 1, np.abs(dpos0) + abs_pos / S)
    _acc_ok("embed_bwd short pack dtok", dtok, dtok0 + sum_tok / S, count[:, None] + 1, np.abs(dtok0) + abs_tok / S)
    assert np.array_equal(dtok[count == 0].view(np.int32), dtok0[count == 0].view(np.int32))


def test_forward_embedding_reads_the_rows_the_scatter_writes_for_out_of_range_ids(env):
    """tok_clamp (train.hip) sends ids < 0 to row 0 and ids >= vocab to row vocab - 1 (test_embed_bwd checks the scatter lands there);
    the forward embedding kernel (elementwise.hip) must read the same rows: a training forward of the tiny tower on ids -3 and
    vocab + 5 gives the bits of the forward on 0 and vocab - 1, and other bits than on their neighbours 1 and vocab - 2."""
    _, torch, _ = env
    from leaf_amd.model import create_model
    m = create_model("tiny-test-quickgelu", device="cuda:0", seed=12, trainable=True)
    V, ctx = m.cfg.vocab_size, m.cfg.context_length
    rng = np.random.default_rng(0)
    lens = np.array([9, 1, 30, 77], np.int32)
    base = rng.integers(16, V - 16, size=(len(lens), ctx)).astype(np.int32)

    def feats(lo, hi):
        tok = base.copy()
        tok[0, 2], tok[1, 0], tok[2, 29], tok[3, 40] = lo, hi, lo, hi
        return m.forward_train(tok, seq_lens=lens, pool_last=True).clone()

    out, clamped, neighbours = feats(-3, V + 5), feats(0, V - 1), feats(1, V - 2)
    assert torch.isfinite(out).all()
    assert torch.equal(out, clamped)
    assert not torch.equal(out[0], neighbours[0]) and not torch.equal(out[1], neighbours[1])


# =============================================================================================== (e) FARE loss head
@pytest.mark.parametrize("B", [1, 5, 300])
@pytest.mark.parametrize("D", [64, 768, 1000, 2048])
def test_fare_loss_head(env, D, B):
    """fare_rows_kernel + fare_reduce_kernel alone: loss, dout and the loss-scale choice; with and without --normalize_fare's norms,
    with and without scaling, scaler back-off absent, 0 and -3"""
    lib, torch, dev = env
    from leaf_amd import _lib
    rng = np.random.default_rng(D + B)
    scale = 0.5
    raw = (rng.standard_normal((B, D)) * 1.7).astype(np.float32)
    norms = np.linalg.norm(raw.astype(np.float64), axis=-1).astype(np.float32)
    anchor = (rng.standard_normal((B, D)) / np.sqrt(D)).astype(np.float32)
    t_anchor = _dev(env, anchor)
    for with_norms in (False, True):
        feat = (raw / norms[:, None]).astype(np.float32) if with_norms else raw
        loss_ref, dout_ref, abs_loss, abs_dout = fare_ref(feat, anchor, scale, norms if with_norms else None)
        amax = float(np.abs(dout_ref).max())
        t_feat, t_norms = _dev(env, feat), _dev(env, norms) if with_norms else None
        for use_scaling, backoff in ((0, None), (0, -3), (1, None), (1, 0), (1, -3)):
            state = np.zeros(16, np.float32)
            if backoff is not None:
                state[3] = backoff                       # LEAF_SC_BACKOFF
            t_state = _dev(env, state) if backoff is not None else None
            loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
            dout = torch.full((B, D), float("nan"), dtype=torch.float32, device=dev)
            ws = torch.full((64 + 2 * B,), float("nan"), dtype=torch.float32, device=dev)
            _lib.check(lib.leaf_op_fare_loss(ptr(t_feat), ptr(t_anchor), ptr(t_norms), ptr(t_state), B, D, scale, use_scaling, ptr(loss),
                                             ptr(dout), ptr(ws), stream()), "fare_loss")
            torch.cuda.synchronize()
            label = f"fare_loss D={D} B={B} norms={int(with_norms)} scaling={use_scaling} backoff={backoff}"
            _acc_ok(label + " loss", loss.cpu().numpy()[0], loss_ref, D + B, abs_loss)
            _acc_ok(label + " dout", dout.cpu().numpy(), dout_ref, (D + 4) if with_norms else 1, abs_dout)
            Sg, inv = (float(v) for v in ws[:2].cpu().numpy().astype(np.float64))
            if not use_scaling:
                assert Sg == 1.0 and inv == 1.0, label
            else:
                mant, _ = np.frexp(Sg)
                assert mant == 0.5 and Sg > 0, f"{label}: S = {Sg} is not a power of two"
                assert 8.0 <= Sg * 2.0 ** (-(backoff or 0)) * amax < 16.0, f"{label}: S = {Sg}, max|dout| = {amax}"
                assert inv == 1.0 / Sg, label
            if backoff is not None:
                assert np.array_equal(t_state.cpu().numpy(), state), "the loss head wrote to the scaler state"
    # feat == anchor: an all-zero gradient has no scale to choose
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    dout = torch.full((B, D), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.full((64 + 2 * B,), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(lib.leaf_op_fare_loss(ptr(t_anchor), ptr(t_anchor), None, None, B, D, scale, 1, ptr(loss), ptr(dout), ptr(ws), stream()),
               "fare_loss")
    torch.cuda.synchronize()
    assert float(loss[0]) == 0.0 and not dout.cpu().numpy().any() and ws[:2].cpu().tolist() == [1.0, 1.0]


def test_fare_loss_head_refuses_more_than_2048_columns(env):
    lib, torch, dev = env
    B, D = 2, 2049
    z = torch.zeros(B, D, dtype=torch.float32, device=dev)
    ws = torch.zeros(64 + 2 * B, dtype=torch.float32, device=dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    dout = z.clone()
    assert lib.leaf_op_fare_loss(ptr(z), ptr(z), None, None, B, D, 1.0, 0, ptr(loss), ptr(dout), ptr(ws), stream()) != 0
    torch.cuda.synchronize()


# =============================================================================================== (f) saturation check
SAT_NUMEL = [8, 64, 4096, 8, (1 << 22) + 8]         # the last one is more than one pass of the capped grid
SAT_BITS = [0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00]  # +-65504 (the saturated conversions), +-inf, NaN


@pytest.fixture(scope="module")
def sat_bufs(env):
    _, torch, dev = env
    g = torch.Generator(device="cpu").manual_seed(6)
    return [torch.randn(n, generator=g).to(torch.float16).to(dev).contiguous() for n in SAT_NUMEL]


def _sat_launch(env, bufs, numel=None):
    """-> (return code, flag raised, poison is NaN); every other word of the scaler state must keep its value"""
    lib, torch, dev = env
    state0 = np.arange(16, dtype=np.float32) + 100.0
    state0[5] = 0.0                                  # LEAF_SC_SAT_FLAG
    state, poison = _dev(env, state0), _dev(env, np.array([1.5, 2.5], np.float32))
    arr = (C.c_void_p * 5)(*[b.data_ptr() for b in bufs])
    num = (C.c_size_t * 5)(*(numel or [b.numel() for b in bufs]))
    rc = lib.leaf_op_sat_check16(arr, num, 5, ptr(state), ptr(poison), stream())
    torch.cuda.synchronize()
    st, po = state.cpu().numpy(), poison.cpu().numpy()
    assert np.array_equal(np.delete(st, 5), np.delete(state0, 5)) and po[1] == 2.5
    assert st[5] in (0.0, 1.0) and (np.isnan(po[0]) or po[0] == 1.5)
    assert (st[5] == 1.0) == bool(np.isnan(po[0])), "flag and poison disagree"
    return rc, bool(st[5] == 1.0)


def test_sat_check_leaves_clean_gradients_alone(env, sat_bufs):
    _, torch, _ = env
    assert _sat_launch(env, sat_bufs) == (0, False)
    # 65472, the largest fp16 below the saturation value, at both ends of every tensor, either sign
    saved = [(b[0].clone(), b[-1].clone()) for b in sat_bufs]
    for i, b in enumerate(sat_bufs):
        b.view(torch.int16)[0] = 0x7BFE
        b.view(torch.int16)[-1] = 0xFBFE - (1 << 16)
    try:
        assert _sat_launch(env, sat_bufs) == (0, False)
    finally:
        for b, (first, last) in zip(sat_bufs, saved):
            b[0], b[-1] = first, last


@pytest.mark.parametrize("which", range(5))
def test_sat_check_finds_one_value_anywhere(env, sat_bufs, which):
    """one saturated / non-finite value at the first or the last element of one tensor raises flag and poison: 4 launches per tensor,
    20 in all, every bit pattern of SAT_BITS at four places"""
    _, torch, _ = env
    b = sat_bufs[which].view(torch.int16)
    for k, at in enumerate((0, -1, 0, -1)):
        bits = SAT_BITS[(4 * which + k) % 5]
        saved = b[at].clone()
        b[at] = bits - (1 << 16) if bits >= (1 << 15) else bits
        try:
            assert _sat_launch(env, sat_bufs) == (0, True), f"0x{bits:04X} at element {at} of tensor {which} not found"
        finally:
            b[at] = saved
    assert _sat_launch(env, sat_bufs) == (0, False)


def test_sat_check_refuses_what_it_cannot_read_in_16_byte_chunks(env, sat_bufs):
    rc, raised = _sat_launch(env, [sat_bufs[0], sat_bufs[1][1:9], *sat_bufs[2:]])       # a pointer that is not 16-byte aligned
    assert rc != 0 and not raised
    rc, raised = _sat_launch(env, sat_bufs, numel=[8, 60, 4096, 8, (1 << 22) + 8])       # an element count that is no multiple of 8
    assert rc != 0 and not raised
