"""The host arithmetic of a prefix-reuse scoring pass (leaf_amd.model._prefix_limit, _clamp_prefix, _check_equal_lengths): how many leading
rows of a candidate come out of its caption's K/V cache.  The rule -- the candidate's EOT row is always computed, and no more rows are
read than the caption's cache holds -- lives in these helpers only; score_candidates_prepare / _run and score_candidates_fused use
them.  Runs without a GPU."""
import numpy as np
import pytest

CTX = 77


def _loop(prefix, full, base_lens, rho):
    """the rule, one candidate at a time in Python integers"""
    out = []
    for i, p in enumerate(prefix):
        p = min(int(p), int(full[i]) - 1)              # keep the EOT row
        p = min(p, int(base_lens[i // rho]))           # rows the caption really has
        out.append(p)
    return out


def _case(rng, rho):
    """captions of 2 .. 77 rows; candidates as long as their caption or a few rows off (a character edit re-tokenises); prefixes at
    0, 1, len - 1, len, 77 (the no-op edit: no differing position), above the caption's length, and anywhere"""
    B = int(rng.integers(1, 5))
    base_lens = rng.integers(2, CTX + 1, B)
    cap = np.repeat(base_lens, rho)
    full = np.clip(cap + rng.integers(-3, 4, B * rho) * (rng.random(B * rho) < 0.6), 2, CTX)
    special = np.stack([np.zeros_like(full), np.ones_like(full), full - 1, full, np.full_like(full, CTX), cap + rng.integers(1, 9, B * rho),
                        rng.integers(0, CTX + 1, B * rho)])
    prefix = special[rng.integers(0, len(special), B * rho), np.arange(B * rho)]
    return base_lens, full, prefix


@pytest.mark.parametrize("rho", [1, 3])
def test_prefix_clamp_equals_the_per_candidate_loop(rho):
    from leaf_amd.model import _clamp_prefix, _prefix_limit
    rng = np.random.default_rng(100 + rho)
    seen = set()
    for _ in range(300):
        base_lens, full, prefix = _case(rng, rho)
        want = _loop(prefix, full, base_lens, rho)
        for lens_t, pfx_t in ((np.int64, np.int64), (np.int32, np.int32), (np.int32, np.int64)):      # the callers' integer types
            limit = _prefix_limit(full.astype(lens_t), base_lens.astype(lens_t), rho)
            assert limit.dtype == np.int32 and limit.shape == full.shape
            out = np.full(full.size, -7, dtype=np.int32)
            got = _clamp_prefix(prefix.astype(pfx_t), limit, out)
            assert got is out and got.dtype == np.int32
            assert got.tolist() == want
            assert (got >= 0).all() and (got <= full - 1).all()
        cap = np.repeat(base_lens, rho)
        seen |= {"other length"} if (full != cap).any() else set()
        seen |= {name for name, hit in (("0", prefix == 0), ("1", prefix == 1), ("len - 1", prefix == full - 1), ("len", prefix == full),
                                        ("77", prefix == CTX), ("above the caption", prefix > cap)) if hit.any()}
    assert seen == {"other length", "0", "1", "len - 1", "len", "77", "above the caption"}


def test_prefix_clamp_takes_a_prefix_matrix():
    """the callers hand over [B, rho] position matrices as well as flat arrays"""
    from leaf_amd.model import _clamp_prefix, _prefix_limit
    base_lens, full = np.array([5, 9]), np.array([5, 5, 5, 9, 9, 9])
    prefix = np.array([[0, 4, 77], [9, 8, 3]])
    out = np.empty(6, dtype=np.int32)
    assert _clamp_prefix(prefix, _prefix_limit(full, base_lens, 3), out).tolist() == [0, 4, 4, 8, 8, 3]


def test_equal_lengths_check_names_the_first_offender():
    from leaf_amd.model import _check_equal_lengths
    base_lens = np.array([6, 12, 77], dtype=np.int32)
    for rho in (1, 3):
        full = np.repeat(base_lens, rho)
        _check_equal_lengths(full, base_lens, rho)
        _check_equal_lengths(full.astype(np.int64), base_lens, rho)
        bad = full.copy()
        bad[rho] += 1               # the first candidate of caption 1 ...
        bad[-1] -= 2                # ... and a later one
        with pytest.raises(ValueError, match=f"candidate {rho} has length 13, its caption 12"):
            _check_equal_lengths(bad, base_lens, rho)
