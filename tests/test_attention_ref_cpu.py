"""The float64 reference of the attention kernels' row modes (tests/util.py), pinned on the CPU: assembling a sequence from its
own rows and its caption's cache rows (prefix / single-edit) and slicing the rows a launch writes (positions >= prefix, or the
eot row) must give exactly what the dense reference gives on the fully assembled sequences."""
import numpy as np

from tests.test_gpu_kernels import _attention_ref
from tests.util import attn_assemble, attn_seq_ref, attn_slice

H, D = 2, 128
CAPS = [5, 20, 33]
GROUP = 3


def _problem():
    rng = np.random.default_rng(3)
    base_cu = np.concatenate([[0], np.cumsum(CAPS)]).astype(np.int32)
    cache = rng.standard_normal((int(base_cu[-1]), 3 * D))
    prefix = np.array([min(p, L - 1) for L in CAPS for p in (0, 4, L - 1)], np.int32)
    fresh = rng.standard_normal((prefix.size, 3 * D))          # one row per candidate: its position prefix[s]
    # by hand, position by position: candidate s of caption c is the caption with row prefix[s] replaced
    full = []
    for s, p in enumerate(prefix):
        c = s // GROUP
        full.append(np.stack([fresh[s] if pos == p else cache[base_cu[c] + pos] for pos in range(CAPS[c])]))
    return base_cu, cache, prefix, fresh, full


def test_assembled_row_modes_equal_the_dense_reference():
    base_cu, cache, prefix, fresh, full = _problem()
    n = prefix.size
    tot = np.array([f.shape[0] for f in full])
    dense = [attn_seq_ref(f, H) for f in full]
    eot = np.array([min(max(p, e), t - 1) for p, t, e in zip(prefix, tot, [0, 4, 15, 16, 3, 19, 1, 32, 32])], np.int32)
    # plain packed rows
    plain = attn_assemble(np.concatenate(full), None, tot)
    # cached prefix: the own rows are the positions >= prefix
    suffix = np.concatenate([f[p:] for f, p in zip(full, prefix)])
    pre = attn_assemble(suffix, cache, tot - prefix, prefix, base_cu, GROUP)
    # single edit, and with the captions themselves in front (NaN in their table rows: never read)
    ed = attn_assemble(fresh, cache, tot - prefix, prefix, base_cu, GROUP, 0, edit=True)
    k = len(CAPS)
    table = np.concatenate([np.full((k, 3 * D), np.nan), fresh])
    ed_off = attn_assemble(table, cache, np.concatenate([CAPS, tot - prefix]), np.concatenate([np.zeros(k, np.int32), prefix]), base_cu,
                           GROUP, k, edit=True)
    for i in range(k):
        assert np.array_equal(ed_off[i], cache[base_cu[i]: base_cu[i + 1]])
    for seqs in (plain, pre, ed, ed_off[k:]):
        assert len(seqs) == n
        for a, b in zip(seqs, full):
            assert np.array_equal(a, b)
        outs = [attn_seq_ref(a, H) for a in seqs]
        assert np.array_equal(attn_slice(outs), np.concatenate(dense))
        assert np.array_equal(attn_slice(outs, prefix), np.concatenate([o[p:] for o, p in zip(dense, prefix)]))
        assert np.array_equal(attn_slice(outs, prefix, eot), np.stack([o[e] for o, e in zip(dense, eot)]))
    # in front of group_off without the edit mode: own rows only, whatever the cache holds
    own = np.concatenate([np.concatenate(full[:2]), suffix])
    mixed = attn_assemble(own, cache, np.concatenate([tot[:2], tot - prefix]), np.concatenate([[0, 0], prefix]), base_cu, GROUP, 2)
    assert all(np.array_equal(a, b) for a, b in zip(mixed, full[:2] + full))


def test_sequence_reference_is_the_dense_tests_reference():
    """... and per sequence it is the batched reference test_attention_fwd has always used (same operation, another evaluation order)"""
    rng = np.random.default_rng(4)
    n, L = 3, 33
    qkv = rng.standard_normal((n * L, 3 * D))
    want = _attention_ref(qkv, n, L, H)[0]
    got = attn_slice([attn_seq_ref(qkv[i * L:(i + 1) * L], H) for i in range(n)])
    assert np.abs(got - want).max() < 1e-13
    # the rounding model differs from it by the two roundings only: no more than their sum, P (<= 1, 11 / 8 significant bits) against
    # |v| rows and one output rounding
    for dtype, ulp in (("fp16", 2.0 ** -11), ("bf16", 2.0 ** -8)):
        m = attn_slice([attn_seq_ref(qkv[i * L:(i + 1) * L], H, dtype) for i in range(n)])
        assert 0 < np.abs(m - want).max() <= ulp * (np.abs(qkv[:, 2 * D:]).max() * 2 + np.abs(want).max())
