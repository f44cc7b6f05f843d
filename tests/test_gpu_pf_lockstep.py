"""Partition function: the lockstep batch (ccj_pf_batch_*, PfLockstepBatch, pf_many(lockstep=K)) fills K
sequences with one set of level launches.

Everything is held against tests/golden/pf_golden.json (the reference's own part_func.cc): a member
of a batch must give what a fresh context gives, bit for bit, whatever its neighbours are.
"""
import json
import os
import random
import struct

import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden", "pf_golden.json")

with open(GOLD) as _f:
    CASES = json.load(_f)["cases"]
BY_NAME = {c["name"]: c for c in CASES}
GROUPS = sorted({(c["params"], c["dangles"]) for c in CASES})
D2 = ("default", 2)


def _group(g):
    return [c for c in CASES if (c["params"], c["dangles"]) == g]


def _by_len(g, lengths):
    by_n = {len(c["seq"]): c for c in _group(g)}
    return [by_n[n] for n in lengths]


def _wbits(ws):
    return ["%016x" % struct.unpack("<Q", struct.pack("<d", w))[0] for w in ws]


def _check(pf, case):
    """What test_gpu_pf_contexts.py::_fold_and_check checks of a context, on a filled member."""
    import ccj_amd
    assert pf.refused is None, (case["name"], pf.refused)
    e = pf.energy
    assert repr(e) == repr(float(case["energy"])) or (e != e and case["energy"] == "nan"), case["name"]
    assert _wbits(pf.W()) == case["wbits"], case["name"]
    h = pf.hashes()
    bad = {k: (h[k], v) for k, v in {**case["h2"], **case["h4"]}.items() if h[k] != v}
    assert not bad, (case["name"], bad)
    assert pf.exp_hashes() == case["exp"]
    if "srand" in case:
        pf.srand(case["srand"])
        try:
            got = pf.sample(5)
            assert "sample_exit" not in case
            assert got == case["samples"]
        except ccj_amd.SampleExit as ex:
            assert ex.structures == case["samples"]
            assert ex.stdout == case["sample_exit"]


def _bind_fill_check(batch, cases):
    batch.bind([c["seq"] for c in cases])
    assert batch.count == len(cases) == len(batch.members)
    import ccj_amd
    assert ccj_amd.lib().ccj_pf_batch_count(batch._h) == len(cases)
    for pf, c in zip(batch.members, cases):
        assert pf.n == len(c["seq"]) == ccj_amd.lib().ccj_pf_n(pf._h) and pf.seq == c["seq"]
    batch.fill()
    for pf, c in zip(batch.members, cases):
        _check(pf, c)


# ---- 1. mixed lengths, idle levels --------------------------------------------------------------
@pytest.mark.gpu
def test_mixed_lengths_and_idle_levels():
    import ccj_amd
    first = _by_len(D2, (60, 3, 44, 8, 30, 23, 1))
    second = _by_len(D2, (4, 5, 6, 2, 37))
    batch = ccj_amd.PfLockstepBatch(64, 8, dangle=2, params="default")
    try:
        assert (batch.size, batch.capacity, batch.count) == (8, 64, 0)
        assert all(pf.capacity == 64 for pf in batch._all)
        _bind_fill_check(batch, first)       # 7 bound, 1 idle; the longest first, n = 3 and 1 between long ones
        _bind_fill_check(batch, second)      # fewer members, the first levels, a shorter longest
        _bind_fill_check(batch, first[::-1])
    finally:
        batch.close()


# ---- 2. same geometry, different sequences ------------------------------------------------------
@pytest.mark.gpu
def test_same_geometry_different_sequences():
    import ccj_amd
    g = ("DirksPierce09", 2)
    cases = [c for c in _group(g) if len(c["seq"]) == 32]
    assert sorted(c["name"] for c in cases) == sorted(
        ["hexa_DirksPierce09", "tetra_DirksPierce09", "samp_tetra_s1", "samp_tetra_s7", "samp_tetra_s12345"])
    # a member index lost anywhere makes two members agree: these two must not
    assert BY_NAME["hexa_DirksPierce09"]["h4"]["PK"] != BY_NAME["tetra_DirksPierce09"]["h4"]["PK"]
    batch = ccj_amd.PfLockstepBatch(32, 5, dangle=2, params="DirksPierce09")
    try:
        _bind_fill_check(batch, cases)
    finally:
        batch.close()


# ---- 3. every group -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS, ids=["%s-d%d" % g for g in GROUPS])
def test_every_group_in_lockstep_runs(g):
    import ccj_amd
    cases = [c for c in _group(g) if len(c["seq"]) <= 60]
    assert len(cases) >= 5
    batch = ccj_amd.PfLockstepBatch(60, 8, dangle=g[1], params=g[0])
    try:
        done = 0
        for run in ccj_amd.plan_lockstep([len(c["seq"]) for c in cases], 8):
            _bind_fill_check(batch, [cases[x] for x in run])
            done += len(run)
        assert done == len(cases)
    finally:
        batch.close()


@pytest.mark.gpu
def test_long_level_range_with_idle_members():
    import ccj_amd
    cases = [BY_NAME[k] for k in ("big80_default", "big60_default", "edge1")]
    batch = ccj_amd.PfLockstepBatch(80, 3, dangle=2, params="default")
    try:
        _bind_fill_check(batch, cases)
    finally:
        batch.close()


# ---- 4. a refused member ------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_refused_member_leaves_the_others(monkeypatch):
    """With the exactness bound lowered to 2^10 (CCJ_PF_RANGE_LOG2) big60_default ends in
    CCJ_E_PF_RANGE; edge3 (n = 3: every P is 0) cannot."""
    import ccj_amd
    from ccj_amd import CCJ_E_STATE, CCJError
    cases = [BY_NAME[k] for k in ("r16_default_d2", "big60_default", "r12_default_d2", "edge3")]
    batch = ccj_amd.PfLockstepBatch(60, 4, dangle=2, params="default")
    try:
        batch.bind([c["seq"] for c in cases])
        monkeypatch.setenv("CCJ_PF_RANGE_LOG2", "10")
        batch.fill()
        monkeypatch.delenv("CCJ_PF_RANGE_LOG2")
        big = batch.members[1]
        assert big.energy is None and big.refused is not None and big.refused.code == 10
        assert "2^53" in big.refused.msg
        with pytest.raises(CCJError) as e:
            big.W()
        assert e.value.code == CCJ_E_STATE
        for k in (0, 2, 3):
            _check(batch.members[k], cases[k])
        _bind_fill_check(batch, cases)  # the bound back at 2^53: all four fold
    finally:
        batch.close()


# ---- 5. misuse ----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_misuse():
    import ccj_amd
    from ccj_amd import CCJ_E_ARG, CCJ_E_STATE, CCJError
    cases = _by_len(D2, (25, 4, 20))
    batch = ccj_amd.PfLockstepBatch(30, 3, dangle=2, params="default")
    try:
        _bind_fill_check(batch, cases)
        good = cases[0]["seq"]
        for bad in ([good, "A" * 31], [good[:10] + "X" + good[11:], good], [], [good] * 4, [good, ""]):
            with pytest.raises(CCJError) as e:
                batch.bind(bad)
            assert e.value.code == CCJ_E_ARG, bad
            assert batch.count == 3 and [pf.seq for pf in batch.members] == [c["seq"] for c in cases]
            batch.fill()  # the previous binding still fills to its goldens
            for pf, c in zip(batch.members, cases):
                _check(pf, c)
        pf = batch.members[0]
        for call in (lambda: pf.rebind(good), lambda: pf.reset(good), pf.ccj_pf, lambda: pf.set_timing(True)):
            with pytest.raises(CCJError) as e:
                call()
            assert e.value.code == CCJ_E_STATE
        assert pf.n == 25 and pf.seq == good
        for p, c in zip(batch.members, cases):  # the refused calls left the fill in place
            _check(p, c)
        batch.bind([c["seq"] for c in cases])
        for call in (pf.W, pf.hashes, lambda: pf.sample(1), lambda: pf.get2("V")):
            with pytest.raises(CCJError) as e:
                call()
            assert e.value.code == CCJ_E_STATE
        batch.fill()
        for p, c in zip(batch.members, cases):
            _check(p, c)
    finally:
        batch.close()
    for args in ((10, 0), (0, 2)):
        with pytest.raises(CCJError) as e:
            ccj_amd.PfLockstepBatch(*args)
        assert e.value.code == CCJ_E_ARG


# ---- 6. one set of launches ---------------------------------------------------------------------
def _planned_launches(batch):
    """The zeroing launch, then per level every family of pf_level_plan some member has work in."""
    import ccj_amd
    lengths = [pf.n for pf in batch.members]
    total = 1
    for t in range(-3, max(lengths) - 2):
        plan = ccj_amd.pf_level_plan(lengths, t, batch.item_counts(t + 2))
        total += sum(1 for k in ccj_amd.PF_PLAN_KERNELS if plan[k][0][0] > 0)
    return total


@pytest.mark.gpu
def test_one_set_of_launches_for_the_batch():
    import ccj_amd
    big = BY_NAME["big60_default"]
    others = _by_len(D2, (44, 37, 30, 23, 8, 3))
    batch = ccj_amd.PfLockstepBatch(60, 7, dangle=2, params="default")
    try:
        _bind_fill_check(batch, [big])
        alone = batch.launches()
        assert alone == _planned_launches(batch)
        # n = 60: spans 0..59 (k_pf_diag), P pushes of levels 0..56, levels 0..57, and k_pf_iloop
        # wherever the level has items (none below level 4: a window needs a >= 2 and b >= 2 at least)
        items = [batch.item_counts(t)[0] for t in range(58)]
        assert items[:4] == [0, 0, 0, 0]
        assert alone == 1 + 60 + 57 + 58 + sum(1 for x in items if x > 0)
        _bind_fill_check(batch, [big] + others)
        assert batch.launches() == _planned_launches(batch) == alone
        assert alone < 2 * (alone - 1)  # one context needs alone - 1 launches (and three memsets) for n = 60
        assert batch.fill_ms() > 0
    finally:
        batch.close()


# ---- 7. pf_many(lockstep=K) ---------------------------------------------------------------------
def _shuffled27():
    cs = _group(D2)
    assert len(cs) == 27
    random.Random(2027).shuffle(cs)
    return cs


@pytest.mark.gpu
@pytest.mark.parametrize("k", [4, 8])
def test_pf_many_lockstep_records_in_input_order(k):
    import ccj_amd
    cs = _shuffled27()
    recs = ccj_amd.pf_many([c["seq"] for c in cs], 2, "default", lockstep=k)
    assert len(recs) == 27
    for c, (seq, e, wn) in zip(cs, recs):
        assert seq == c["seq"]
        assert repr(e) == repr(float(c["energy"])), c["name"]
        assert _wbits([wn])[0] == c["wbits"][-1], c["name"]
    assert ccj_amd.pf_many([], lockstep=8) == []
