"""The vocabulary projection kernel of text embedding inversion (leaf_amd/csrc/nnproj.hip; nn_project, src/pez/optim_utils.py:26-55)
alone, through the C ABI, against a float64 product on the CPU.

MARGIN RULE (also used by tests/test_gpu_inversion.py and tests/test_inversion_cpu.py).  An fp32 inner product of d terms is within
d 2^-23 of the exact one relative to sum |a_i b_i| <= ||a|| ||b||, i.e. within d 2^-23 in units of the cosine; two
operands (the product and the table row's norm) double it: BOUND = 2 d 2^-23.  ``ids`` must equal the float64 arg-max wherever the
float64 gap between the best and the runner-up cosine exceeds BOUND; elsewhere the returned id's float64 cosine must be within BOUND
of the maximum, and at most 2 % of the rows of a case may be decided that way.  ``cos`` must be within d 2^-23 of float64."""
import ctypes as C

import numpy as np
import pytest

from tests.util import ptr, stream

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1000, 128), (17, 1000, 128), (65, 4097, 768), (65, 49408, 768), (33, 1031, 1280)]


def margin_bound(d):
    return 2.0 * d * 2.0 ** -23


def cos64(q, table):
    q, t = np.asarray(q, np.float64), np.asarray(table, np.float64)
    return (q @ t.T) / np.linalg.norm(q, axis=1)[:, None] / np.linalg.norm(t, axis=1)[None, :]


def check_margin_rule(ids, cosv, ref, d, what=""):
    """ids [M], cosv [M] (or None) against the float64 cosine matrix ref [M, V]; returns the number of rows decided by the margin"""
    M = ref.shape[0]
    order = np.argsort(-ref, axis=1, kind="stable")[:, :2]
    best = ref[np.arange(M), order[:, 0]]
    gap = best - ref[np.arange(M), order[:, 1]] if ref.shape[1] > 1 else np.full(M, np.inf)
    clear = gap > margin_bound(d)
    got = ref[np.arange(M), ids]
    print(f"{what}: rows {M}, decided by the margin {int((~clear).sum())}, min gap {gap.min():.3e}, "
          f"max (best - got) {float((best - got).max()):.3e}" +
          (f", max |cos - f64| {float(np.abs(cosv - got).max()):.3e}" if cosv is not None else ""))
    assert np.array_equal(ids[clear], order[clear, 0]), f"{what}: wrong nearest neighbour outside the margin"
    assert np.all(best[~clear] - got[~clear] <= margin_bound(d)), f"{what}: id inside the margin is not within the bound of the maximum"
    assert (~clear).sum() <= 0.02 * M, f"{what}: {(~clear).sum()} of {M} rows decided by the margin"
    if cosv is not None:
        assert np.abs(cosv - got).max() <= d * 2.0 ** -23, f"{what}: cos differs from float64"
    return int((~clear).sum())


class Projector:
    def __init__(self):
        import torch
        from leaf_amd import _lib
        assert torch.cuda.is_available()
        self.torch, self._lib, self.lib = torch, _lib, _lib.lib()

    def inv_norms(self, table):
        V, d = table.shape
        inv = self.torch.empty(V, dtype=self.torch.float32, device="cuda")
        self._lib.check(self.lib.leaf_vocab_inv_norms(ptr(table), V, d, ptr(inv), stream()), "leaf_vocab_inv_norms")
        return inv

    def project(self, q, table, inv, want_cos=True):
        torch = self.torch
        M, d = q.shape
        V = table.shape[0]
        ids = torch.full((M,), -7, dtype=torch.int32, device="cuda")
        cosv = torch.full((M,), -7.0, dtype=torch.float32, device="cuda") if want_cos else None
        nb = self.lib.leaf_nn_project_ws_bytes(M, V)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        self._lib.check(self.lib.leaf_nn_project(ptr(q), M, ptr(table), ptr(inv), V, d, ptr(ids), ptr(cosv), ptr(ws), nb, stream()),
                        "leaf_nn_project")
        torch.cuda.synchronize()
        return ids.cpu().numpy(), (cosv.cpu().numpy() if want_cos else None)


@pytest.fixture(scope="module")
def proj():
    return Projector()


def _case(M, V, d, seed):
    """table [V, d] ~ N(0, 1); queries = table rows + 0.3 sigma noise, winners planted at id 0, id V - 1 and in the last partial tile"""
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((V, d)).astype(np.float32)
    last_tile = V - 1 - (((V - 1) % 16) // 2)                    # inside the vocabulary's last 16-row tile, not its last row
    planted = [0, V - 1, last_tile]
    win = np.array((planted + list(rng.integers(0, V, size=max(M - 3, 0))))[:M])
    q = (table[win] + 0.3 * rng.standard_normal((M, d))).astype(np.float32)
    return table, q, win, planted


@pytest.mark.parametrize("M,V,d", SHAPES)
def test_nearest_row_vs_float64(proj, M, V, d):
    torch = proj.torch
    table, q, win, planted = _case(max(M, 3), V, d, seed=M * 1000 + d)
    tt = torch.from_numpy(table).cuda()
    inv = proj.inv_norms(tt)
    inv64 = 1.0 / np.linalg.norm(table.astype(np.float64), axis=1)
    assert np.abs(inv.cpu().numpy() / inv64 - 1).max() < 4 * 2.0 ** -23
    ref = cos64(q, table)
    assert np.array_equal(ref.argmax(1), win)                    # the planted rows do win in float64
    if M == 1:                                                   # one row per launch: each planted winner in turn
        for r in range(3):
            ids, cosv = proj.project(torch.from_numpy(q[r:r + 1]).cuda(), tt, inv)
            assert ids[0] == planted[r]
            check_margin_rule(ids, cosv, ref[r:r + 1], d, f"M=1 V={V} d={d} winner {planted[r]}")
        return
    ids, cosv = proj.project(torch.from_numpy(q).cuda(), tt, inv)
    check_margin_rule(ids, cosv, ref, d, f"M={M} V={V} d={d}")
    assert list(ids[:3]) == planted
    ids2, none = proj.project(torch.from_numpy(q).cuda(), tt, inv, want_cos=False)      # cos may be NULL
    assert none is None and np.array_equal(ids2, ids)


def test_identical_table_rows_resolve_to_the_lower_id(proj):
    torch = proj.torch
    V, d = 4097, 768
    rng = np.random.default_rng(5)
    table = rng.standard_normal((V, d)).astype(np.float32)
    pairs = [(100, 101), (5, V - 3), (33, 2050), (V - 2, V - 1)]          # same tile, far slabs, ..., the last partial tile
    for lo, hi in pairs:
        table[hi] = table[lo]
    q = np.stack([table[lo] + 0.3 * rng.standard_normal(d).astype(np.float32) for lo, _ in pairs]).astype(np.float32)
    tt = torch.from_numpy(table).cuda()
    ids, _ = proj.project(torch.from_numpy(q).cuda(), tt, proj.inv_norms(tt))
    assert list(ids) == [lo for lo, _ in pairs]


def test_nan_query_returns_id_zero(proj):
    torch = proj.torch
    table, q, win, _ = _case(17, 1000, 128, seed=9)
    q[4, 7] = np.nan
    q[16, :] = np.nan
    tt = torch.from_numpy(table).cuda()
    ids, cosv = proj.project(torch.from_numpy(q).cuda(), tt, proj.inv_norms(tt))
    assert ids[4] == 0 and ids[16] == 0 and np.isnan(cosv[4]) and np.isnan(cosv[16])
    keep = [i for i in range(17) if i not in (4, 16)]
    assert np.array_equal(ids[keep], win[keep])


def test_a_row_gets_the_same_bits_in_any_launch(proj):
    """alone, inside M = 65, and at another slot of another batch: identical ids and cos bits"""
    torch = proj.torch
    for V, d in ((4097, 768), (1031, 1280), (1000, 128)):
        table, q, _, _ = _case(65, V, d, seed=V + d)
        tt = torch.from_numpy(table).cuda()
        inv = proj.inv_norms(tt)
        ids, cosv = proj.project(torch.from_numpy(q).cuda(), tt, inv)
        for r in (0, 3, 40, 64):
            i1, c1 = proj.project(torch.from_numpy(q[r:r + 1]).cuda(), tt, inv)
            assert i1[0] == ids[r] and c1.view(np.uint32)[0] == cosv.view(np.uint32)[r]
        perm = np.roll(np.arange(65), 23)[:37]                                # other slots, other M, other tiles
        i2, c2 = proj.project(torch.from_numpy(q[perm]).cuda(), tt, inv)
        assert np.array_equal(i2, ids[perm]) and np.array_equal(c2.view(np.uint32), cosv.view(np.uint32)[perm])


def test_bad_shapes_are_errors_not_launches(proj):
    torch, lib = proj.torch, proj.lib
    V, M = 1000, 17
    table = torch.zeros(V, 132, device="cuda")
    q = torch.zeros(M, 132, device="cuda")
    inv = torch.ones(V, device="cuda")
    ids = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    nb = lib.leaf_nn_project_ws_bytes(M, V)
    assert nb >= M * ((V + 15) // 16) * 8
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    assert lib.leaf_nn_project(ptr(q), M, ptr(table), ptr(inv), V, 130, ptr(ids), C.c_void_p(0), ptr(ws), nb, stream()) != 0
    assert b"130" in lib.leaf_last_error()
    assert lib.leaf_vocab_inv_norms(ptr(table), V, 130, ptr(inv), stream()) != 0
    assert lib.leaf_nn_project(ptr(q), M, ptr(table), ptr(inv), V, 2052, ptr(ids), C.c_void_p(0), ptr(ws), nb, stream()) != 0
    assert lib.leaf_nn_project(ptr(q), M, ptr(table), ptr(inv), V, 132, ptr(ids), C.c_void_p(0), ptr(ws), 64, stream()) != 0
    assert b"workspace too small" in lib.leaf_last_error()
    assert lib.leaf_nn_project(ptr(q), 0, ptr(table), ptr(inv), V, 132, ptr(ids), C.c_void_p(0), ptr(ws), nb, stream()) != 0
    torch.cuda.synchronize()
    assert bool((ids == -7).all())                                             # nothing ran
