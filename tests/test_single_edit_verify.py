"""The token-level check behind LEAF_VERIFY_SINGLE_EDIT=1 (leaf_amd.model.verify_single_edit): a ``single_edit`` scoring pass promises
that every candidate is its caption with ONE token replaced at its prefix length.  Runs without a GPU."""
import numpy as np
import pytest

from oracle import text_oracle as O


def _case(B=3, rho=4, seed=5):
    base = O.synthetic_tokens(B, seed=seed, min_len=6, max_len=20)
    lens = base.argmax(-1) + 1
    rng = np.random.default_rng(seed)
    cand = np.repeat(base[:, None, :], rho, axis=1)
    pos = np.zeros((B, rho), dtype=np.int64)
    for b in range(B):
        for r in range(rho):
            pos[b, r] = int(rng.integers(1, lens[b] - 1))
            cand[b, r, pos[b, r]] = int(rng.integers(1, 49000))
    return base, lens, cand, pos


def test_accepts_substitutions_and_unchanged_candidates():
    from leaf_amd.model import verify_single_edit
    base, lens, cand, pos = _case()
    rho = cand.shape[1]
    cand[0, 0] = base[0]                         # the drawn id equals the caption's: no change at all
    cand[1, 1] = base[1]
    cand[1, 1, 1] = 9                            # edit at position 1
    pos[1, 1] = 1
    cand[2, 2] = base[2]
    cand[2, 2, lens[2] - 2] = 11                 # last position before EOT
    pos[2, 2] = lens[2] - 2
    verify_single_edit(cand.reshape(-1, 77), np.repeat(lens, rho), pos.reshape(-1), base, lens, rho)
    import torch                                 # tensors as well as arrays
    verify_single_edit(torch.from_numpy(cand.reshape(-1, 77)), np.repeat(lens, rho), torch.from_numpy(pos.reshape(-1)),
                       torch.from_numpy(base), lens, rho)


def test_rejects_a_second_changed_token_behind_the_prefix():
    from leaf_amd.model import verify_single_edit
    base, lens, cand, pos = _case()
    rho = cand.shape[1]
    b, r = 1, 2
    p = int(pos[b, r])
    behind = p + 1 if p + 1 < lens[b] - 1 else p - 1
    if behind < p:                               # keep the changed token BEHIND the declared prefix
        pos[b, r] = behind
        behind = p
    cand[b, r, behind] = int(cand[b, r, behind]) % 40000 + 7
    with pytest.raises(ValueError, match="differs from its caption at position"):
        verify_single_edit(cand.reshape(-1, 77), np.repeat(lens, rho), pos.reshape(-1), base, lens, rho)


def test_rejects_a_changed_token_in_front_of_the_prefix():
    from leaf_amd.model import verify_single_edit
    base, lens, cand, pos = _case()
    rho = cand.shape[1]
    cand[0, 1] = base[0]
    cand[0, 1, 1] = int(base[0, 1]) % 40000 + 3
    cand[0, 1, 3] = int(base[0, 3]) % 40000 + 3
    pos[0, 1] = 3
    with pytest.raises(ValueError, match="position 1"):
        verify_single_edit(cand.reshape(-1, 77), np.repeat(lens, rho), pos.reshape(-1), base, lens, rho)


def test_rejects_a_different_length():
    from leaf_amd.model import verify_single_edit
    base, lens, cand, pos = _case()
    rho = cand.shape[1]
    cl = np.repeat(lens, rho)
    b, r = 2, 0
    eot = int(lens[b] - 1)
    cand[b, r, eot + 1] = cand[b, r, eot]        # one token longer: EOT moves by one
    cand[b, r, eot] = 17
    cl[b * rho + r] += 1
    with pytest.raises(ValueError, match="length"):
        verify_single_edit(cand.reshape(-1, 77), cl, pos.reshape(-1), base, lens, rho)


def test_rejects_a_candidate_count_that_is_not_b_times_rho():
    from leaf_amd.model import verify_single_edit
    base, lens, cand, pos = _case()
    rho = cand.shape[1]
    with pytest.raises(ValueError, match="candidates for"):
        verify_single_edit(cand.reshape(-1, 77)[:-1], np.repeat(lens, rho)[:-1], pos.reshape(-1)[:-1], base, lens, rho)
