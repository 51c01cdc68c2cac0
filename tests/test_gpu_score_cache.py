"""The K/V cache record of the scoring passes (leaf_amd.model._KvCache): a cache names a buffer slot of the model, and a later
``encode_text_kv`` / ``score_candidates_fused`` on that slot rewrites its rows.  A pass over such a stale cache is refused, as is one
under another arithmetic (``arithmetic_tag``, ``ln_fold`` included); a refused or declined call leaves the model's counters alone; the
prefix clamp of the fused pass and of the prepare / run pair is one rule, so the two agree bit for bit where it bites."""
import numpy as np
import pytest

from oracle import text_oracle as O

pytestmark = pytest.mark.gpu

B, RHO = 4, 5


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def tiny(torch_mod):
    from leaf_amd.model import create_model
    return create_model("tiny-test-quickgelu", device="cuda:0", seed=3)


@pytest.fixture(scope="module")
def vitl(torch_mod):
    from leaf_amd.model import create_model
    return create_model("ViT-L-14-quickgelu", device="cuda:0", seed=3)


def _case(seed):
    """B captions of 5 .. 40 rows, RHO single-token candidates each (the first one of every caption: no change at all), their lengths
    and first differing positions (77: none)"""
    base = O.synthetic_tokens(B, seed=seed, min_len=3, max_len=38)
    cand = O.synthetic_candidates(base, RHO, seed=seed + 1)
    cand[:, 0] = base
    neq = cand != base[:, None, :]
    pl = neq.argmax(-1)
    pl[~neq.any(-1)] = 77
    return base, cand.reshape(-1, 77), np.repeat(base.argmax(-1) + 1, RHO), pl.reshape(-1)


def _score(m, case, kv, anchor, prefix=None):
    base, flat, lens, pl = case
    out = m.score_candidates(flat, anchor, RHO, "l2", want_loss=True, seq_lens=lens, prefix_lens=pl if prefix is None else prefix, kv=kv)
    return [x.clone() for x in out]


def _eq(torch_mod, a, b, what):
    assert len(a) == len(b)
    for x, y, name in zip(a, b, ("winners", "features", "losses", "predictions", "logits")):
        assert torch_mod.equal(x, y), f"{what}: {name}"


def test_a_cache_is_stale_once_its_slot_is_rewritten(torch_mod, vitl):
    m = vitl
    one, a, b = _case(11), _case(21), _case(31)
    anchor = m.encode_text(one[0]) + 0.1
    kv_one = m.encode_text_kv(one[0], slot=1)
    before = _score(m, one, kv_one, anchor)
    kv_a = m.encode_text_kv(a[0])
    kv_b = m.encode_text_kv(b[0])
    assert (kv_a.slot, kv_b.slot, kv_one.slot) == (0, 0, 1) and kv_b.ticket == kv_a.ticket + 1
    with pytest.raises(RuntimeError, match="encode_text_kv"):
        _score(m, a, kv_a, anchor)
    _eq(torch_mod, _score(m, b, kv_b, anchor), [x.clone() for x in m.score_candidates(b[1], anchor, RHO, "l2", want_loss=True, seq_lens=b[2])],
        "the live cache of slot 0 against full recomputation")
    _eq(torch_mod, _score(m, one, kv_one, anchor), before, "slot 1 after two rewrites of slot 0")


def test_a_fused_pass_stales_the_cache_of_slot_0_and_leaves_a_live_one(torch_mod, vitl):
    m = vitl
    case = base, flat, lens, pl = _case(41)
    anchor = m.encode_text(base) + 0.1
    kv = m.encode_text_kv(base)
    want1 = _score(m, case, kv, anchor)
    got = m.score_candidates_fused(base, base.argmax(-1) + 1, flat, anchor, RHO, lens, pl, want_features=True, want_loss=True)
    assert got is not None
    i, f, cache, l = got
    _eq(torch_mod, [i, f, l], want1, "fused first stage against encode_text_kv + score_candidates")
    with pytest.raises(RuntimeError, match="score_candidates_fused"):
        _score(m, case, kv, anchor)
    assert cache.slot == 0 and cache.ticket == kv.ticket + 1 == m.kv_tickets[0]
    # a later stage (the candidates edited at a pinned position) out of the fused pass's cache, and out of a fresh encode_text_kv
    cand2 = O.synthetic_candidates(base, RHO, seed=43, fixed_pos=np.full(B, 2))
    later = base, cand2.reshape(-1, 77), lens, np.full(B * RHO, 2)
    from_fused = _score(m, later, cache, anchor)
    _eq(torch_mod, from_fused, _score(m, later, m.encode_text_kv(base), anchor), "later stage: fused pass's cache against encode_text_kv's")


def test_a_refused_prepare_and_a_declined_fused_pass_leave_the_counters_alone(torch_mod, tiny):
    m = tiny
    case = base, flat, lens, pl = _case(61)
    anchor = m.encode_text(base) + 0.1
    stale = m.encode_text_kv(base)
    kv = m.encode_text_kv(base)
    rows, tickets = m.rows_scored, dict(m.kv_tickets)
    with pytest.raises(ValueError, match="B\\*rho"):                       # one candidate short
        m.score_candidates_prepare(flat[:-1], anchor, RHO, seq_lens=lens[:-1], kv=kv)
    with pytest.raises(ValueError, match="B\\*rho"):                       # a cache of other captions' count
        m.score_candidates_prepare(flat[RHO:], anchor[1:], RHO, seq_lens=lens[RHO:], kv=kv)
    with pytest.raises(RuntimeError, match="stale"):
        m.score_candidates_prepare(flat, anchor, RHO, seq_lens=lens, kv=stale)
    masks = m.split_masks
    m.set_split_masks(())                                                  # foreign arithmetic: the cache was built on split GEMMs
    try:
        assert masks and m.arithmetic_tag() != kv.arith
        with pytest.raises(ValueError, match="K/V cache built under arithmetic"):
            m.score_candidates_prepare(flat, anchor, RHO, seq_lens=lens, kv=kv)
    finally:
        m.set_split_masks(masks)
    assert m.rows_scored == rows and m.kv_tickets == tickets
    # a fused pass whose rows do not fit one chunk declines: slot 0 keeps its ticket, and its cache stays readable
    chunk = m._lib.leaf_text_get_option(m._h, b"chunk")
    m.set_option("chunk", 1)
    try:
        assert m.score_candidates_fused(base, base.argmax(-1) + 1, flat, anchor, RHO, lens, pl) is None
    finally:
        m.set_option("chunk", chunk)
    assert m.rows_scored == rows and m.kv_tickets == tickets
    got = _score(m, case, kv, anchor)
    assert m.rows_scored > rows and m.kv_tickets == tickets
    _eq(torch_mod, got, [x.clone() for x in m.score_candidates(flat, anchor, RHO, "l2", want_loss=True, seq_lens=lens)], "the following valid call")


def test_ln_fold_is_part_of_a_cache_s_arithmetic(torch_mod, vitl):
    m = vitl
    case = _case(71)
    m.set_precision("fast")            # ln_fold = 0 drops the split masks: start without them, so that the tag differs in ln_fold alone
    try:
        anchor = m.encode_text(case[0]) + 0.1
        kv = m.encode_text_kv(case[0])
        want = _score(m, case, kv, anchor)
        m.set_option("ln_fold", 0)
        try:
            assert m.arithmetic_tag()[:2] == kv.arith[:2] and m.arithmetic_tag() != kv.arith
            with pytest.raises(ValueError, match="K/V cache built under arithmetic"):
                _score(m, case, kv, anchor)
        finally:
            m.set_option("ln_fold", 1)
        _eq(torch_mod, _score(m, case, kv, anchor), want, "the old cache after ln_fold is back on")
    finally:
        m.set_precision("rowsafe")


def test_fused_and_separate_passes_clamp_the_prefix_alike(torch_mod, vitl):
    """prefixes that need the clamp: 77 on candidates equal to their caption, and values above the caption's length"""
    m = vitl
    base, flat, lens, pl = _case(81)
    bl = base.argmax(-1) + 1
    cand = flat.reshape(B, RHO, 77).copy()
    cand[:, 1] = base                                  # a second unchanged candidate per caption ...
    pl = pl.reshape(B, RHO).copy()
    pl[:, 1] = bl + np.arange(1, B + 1)                # ... declared with a prefix above the caption's length
    assert (pl[:, 0] == 77).all() and (pl[:, 1] > bl).all()
    case = base, cand.reshape(-1, 77), lens, pl.reshape(-1)
    anchor = m.encode_text(base) + 0.1
    separate = _score(m, case, m.encode_text_kv(base), anchor)
    i, f, cache, l = m.score_candidates_fused(base, bl, case[1], anchor, RHO, lens, case[3], want_features=True, want_loss=True)
    _eq(torch_mod, [i, f, l], separate, "fused pass against encode_text_kv + score_candidates")
    _eq(torch_mod, _score(m, case, cache, anchor), separate, "the fused pass's cache")
    _eq(torch_mod, separate, [x.clone() for x in m.score_candidates(case[1], anchor, RHO, "l2", want_loss=True, seq_lens=lens)], "full recomputation")


def test_class_scoring_with_and_without_prefix_reuse_agree(torch_mod, vitl):
    m = vitl
    base, flat, lens, pl = _case(91)
    cf = torch_mod.nn.functional.normalize(torch_mod.randn(3, m.cfg.embed_dim, generator=torch_mod.Generator().manual_seed(5)), dim=-1).cuda()
    labels = np.array([0, 2, 1, 2])
    kw = dict(want_features=True, want_loss=True, want_pred=True, want_logits=True, seq_lens=lens)
    plain = [x.clone() for x in m.score_candidates_cls(flat, cf, labels, RHO, **kw)]
    reuse = [x.clone() for x in m.score_candidates_cls(flat, cf, labels, RHO, prefix_lens=pl, kv=m.encode_text_kv(base), **kw)]
    assert plain[4].shape == (B * RHO, 3)
    _eq(torch_mod, reuse, plain, "score_candidates_cls, prefix reuse against full recomputation")
