"""The launch geometry of the partition function's fill, single and batched (pf_level_plan over
ccj_pf_level_plan): no GPU.

With level t the fill's graph enqueues k_pf_iloop(t+2), k_pf_level(t), k_pf_ppush(t) and
k_pf_diag(t+3); t = -3, -2, -1 are the launches ahead of level 0.  A batch launches each of them once
for all members: the member index is a grid dimension of its own and every other extent is the
maximum over the members.  For one member the plan must be the launch a single context has always
made: _level / _ppush / _diag / _iloop below restate the grids of the ccjk_pf_* wrappers as they
stood before the plan existed, and SINGLE pins their values for n = 4, 5, 6 and 30.
"""
import pytest

import ccj_amd
from ccj_amd import PF_PLAN_KERNELS, CCJError, pf_level_plan

NONE = (0, 0, 0)
UNKNOWN = (-1, -1, -1)
PP_S, HS_LEN = 8, 32  # k_pf_ppush: spans per wave, h steps per item


def _level(n, t):  # ccjk_pf_level: 256 cells of one a-block per workgroup, t+1 a-blocks
    if t < 0 or t > n - 3:
        return NONE
    m = n - t - 2
    M = m * (m + 1) // 2
    return ((M + 255) // 256, t + 1, 1) if M > 0 else NONE


def _ppush(n, lev):  # ccjk_pf_ppush: parts A and B, 4 items per workgroup
    nmax = min(lev, n - 4 - lev) + 1
    if lev < 0 or nmax <= 0:
        return NONE
    ngrp = (n - lev - 3 + 63) // 64
    nch = (nmax + PP_S - 1) // PP_S
    npairs = sum((min((c + 1) * PP_S, nmax) + HS_LEN - 1) // HS_LEN for c in range(nch))
    return (2 * ((npairs * ngrp * (lev + 1) + 3) // 4), 1, 1)


def _diag(n, s):  # ccjk_pf_diag: a wave per interval of span s
    return (n - s, 1, 1) if s >= 0 and n - s > 0 else NONE


def _iloop(n, t, nitems):  # ccjk_pf_iloop: a wave per item, 4 per workgroup
    if t < 0 or t > n - 3 or nitems == 0:
        return NONE
    return UNKNOWN if nitems is None else ((nitems + 3) // 4, 1, 1)


def _alone(n, t, nitems):
    return {"k_pf_iloop": _iloop(n, t + 2, nitems), "k_pf_level": _level(n, t), "k_pf_ppush": _ppush(n, t),
            "k_pf_diag": _diag(n, t + 3)}


def _items(n, t):
    """Some item count for level t of a length-n member (the real one depends on the sequence)."""
    return (7 * n + 3 * t) % 23 if 0 <= t <= n - 3 else 0


# t: (k_pf_level(t), k_pf_ppush(t), k_pf_diag(t+3)) as the single-context wrappers launch them
SINGLE = {
    4: {
        -3: ((0, 0, 0), (0, 0, 0), (4, 1, 1)),
        -2: ((0, 0, 0), (0, 0, 0), (3, 1, 1)),
        -1: ((0, 0, 0), (0, 0, 0), (2, 1, 1)),
        0: ((1, 1, 1), (2, 1, 1), (1, 1, 1)),
        1: ((1, 2, 1), (0, 0, 0), (0, 0, 0)),
    },
    5: {
        -3: ((0, 0, 0), (0, 0, 0), (5, 1, 1)),
        -2: ((0, 0, 0), (0, 0, 0), (4, 1, 1)),
        -1: ((0, 0, 0), (0, 0, 0), (3, 1, 1)),
        0: ((1, 1, 1), (2, 1, 1), (2, 1, 1)),
        1: ((1, 2, 1), (2, 1, 1), (1, 1, 1)),
        2: ((1, 3, 1), (0, 0, 0), (0, 0, 0)),
    },
    6: {
        -3: ((0, 0, 0), (0, 0, 0), (6, 1, 1)),
        -2: ((0, 0, 0), (0, 0, 0), (5, 1, 1)),
        -1: ((0, 0, 0), (0, 0, 0), (4, 1, 1)),
        0: ((1, 1, 1), (2, 1, 1), (3, 1, 1)),
        1: ((1, 2, 1), (2, 1, 1), (2, 1, 1)),
        2: ((1, 3, 1), (2, 1, 1), (1, 1, 1)),
        3: ((1, 4, 1), (0, 0, 0), (0, 0, 0)),
    },
    30: {
        -3: ((0, 0, 0), (0, 0, 0), (30, 1, 1)),
        -2: ((0, 0, 0), (0, 0, 0), (29, 1, 1)),
        -1: ((0, 0, 0), (0, 0, 0), (28, 1, 1)),
        0: ((2, 1, 1), (2, 1, 1), (27, 1, 1)),
        1: ((2, 2, 1), (2, 1, 1), (26, 1, 1)),
        2: ((2, 3, 1), (2, 1, 1), (25, 1, 1)),
        3: ((2, 4, 1), (2, 1, 1), (24, 1, 1)),
        4: ((2, 5, 1), (4, 1, 1), (23, 1, 1)),
        5: ((2, 6, 1), (4, 1, 1), (22, 1, 1)),
        6: ((1, 7, 1), (4, 1, 1), (21, 1, 1)),
        7: ((1, 8, 1), (4, 1, 1), (20, 1, 1)),
        8: ((1, 9, 1), (10, 1, 1), (19, 1, 1)),
        9: ((1, 10, 1), (10, 1, 1), (18, 1, 1)),
        10: ((1, 11, 1), (12, 1, 1), (17, 1, 1)),
        11: ((1, 12, 1), (12, 1, 1), (16, 1, 1)),
        12: ((1, 13, 1), (14, 1, 1), (15, 1, 1)),
        13: ((1, 14, 1), (14, 1, 1), (14, 1, 1)),
        14: ((1, 15, 1), (16, 1, 1), (13, 1, 1)),
        15: ((1, 16, 1), (16, 1, 1), (12, 1, 1)),
        16: ((1, 17, 1), (18, 1, 1), (11, 1, 1)),
        17: ((1, 18, 1), (18, 1, 1), (10, 1, 1)),
        18: ((1, 19, 1), (20, 1, 1), (9, 1, 1)),
        19: ((1, 20, 1), (10, 1, 1), (8, 1, 1)),
        20: ((1, 21, 1), (12, 1, 1), (7, 1, 1)),
        21: ((1, 22, 1), (12, 1, 1), (6, 1, 1)),
        22: ((1, 23, 1), (12, 1, 1), (5, 1, 1)),
        23: ((1, 24, 1), (12, 1, 1), (4, 1, 1)),
        24: ((1, 25, 1), (14, 1, 1), (3, 1, 1)),
        25: ((1, 26, 1), (14, 1, 1), (2, 1, 1)),
        26: ((1, 27, 1), (14, 1, 1), (1, 1, 1)),
        27: ((1, 28, 1), (0, 0, 0), (0, 0, 0)),
    },
}


@pytest.mark.parametrize("n", sorted(SINGLE))
def test_pinned_single_context_grids(n):
    assert sorted(SINGLE[n]) == list(range(-3, n - 2))
    for t, (lev, pp, dg) in SINGLE[n].items():
        assert (_level(n, t), _ppush(n, t), _diag(n, t + 3)) == (lev, pp, dg), (n, t)
        plan = pf_level_plan([n], t, [5])
        assert plan["k_pf_level"] == (lev, (lev,)), (n, t)
        assert plan["k_pf_ppush"] == (pp, (pp,)), (n, t)
        assert plan["k_pf_diag"] == (dg, (dg,)), (n, t)
        il = (2, 1, 1) if 0 <= t + 2 <= n - 3 else NONE  # 5 items: two workgroups of 4 waves
        assert plan["k_pf_iloop"] == (il, (il,)), (n, t)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 8, 30, 60])
def test_one_member_is_the_single_context_launch(n):
    for t in range(-3, n - 2):
        for nitems in (None, 0, 1, 4, 5, _items(n, t + 2)):
            want = _alone(n, t, nitems)
            plan = pf_level_plan([n], t, None if nitems is None else [nitems])
            assert sorted(plan) == sorted(PF_PLAN_KERNELS)
            for k in PF_PLAN_KERNELS:
                assert plan[k] == (want[k], (want[k],)), (n, t, nitems, k)


LENGTHS = (60, 3, 44, 8, 30, 23, 1)


def _joint(lengths, t, items):
    plan = pf_level_plan(lengths, t, items)
    alone = [_alone(n, t, None if items is None else items[k]) for k, n in enumerate(lengths)]
    for name in PF_PLAN_KERNELS:
        grid, per = plan[name]
        assert per == tuple(a[name] for a in alone), (t, name)
        if any(g == UNKNOWN for g in per):
            assert name == "k_pf_iloop" and grid == UNKNOWN
            continue
        live = [g for g in per if g != NONE]
        if not live:
            assert grid == NONE, (t, name)
            continue
        mdim = 2 if name == "k_pf_level" else 1  # the member dimension: z for k_pf_level, y otherwise
        assert grid[mdim] == len(lengths) == 7, (t, name)
        for d in range(3):
            if d != mdim:
                assert grid[d] == max(g[d] for g in live), (t, name, d)
    return plan


def test_batched_grids_are_the_members_maxima():
    seen_idle = 0
    for t in range(-3, max(LENGTHS) - 2):
        items = [_items(n, t + 2) for n in LENGTHS]
        plan = _joint(LENGTHS, t, items)
        _joint(LENGTHS, t, None)
        for k, n in enumerate(LENGTHS):  # a member without the level or span has extent 0
            if t > n - 3:
                assert plan["k_pf_level"][1][k] == NONE and plan["k_pf_ppush"][1][k] == NONE
                seen_idle += 1
            if t + 2 > n - 3:
                assert plan["k_pf_iloop"][1][k] == NONE
            if t + 3 > n - 1:
                assert plan["k_pf_diag"][1][k] == NONE
    assert seen_idle > 100
    # the longest member alone decides the last levels
    assert pf_level_plan(LENGTHS, 57)["k_pf_level"] == ((1, 58, 7), ((1, 58, 1),) + (NONE,) * 6)


def test_plan_of_a_permutation_is_the_permutation_of_the_plan():
    perm = (4, 6, 0, 2, 5, 1, 3)
    lengths = tuple(LENGTHS[p] for p in perm)
    for t in range(-3, max(LENGTHS) - 2):
        items = [_items(n, t + 2) for n in LENGTHS]
        a = pf_level_plan(LENGTHS, t, items)
        b = pf_level_plan(lengths, t, [items[p] for p in perm])
        for name in PF_PLAN_KERNELS:
            assert b[name][0] == a[name][0], (t, name)
            assert b[name][1] == tuple(a[name][1][p] for p in perm), (t, name)


@pytest.mark.parametrize("lengths, t, items", [
    ((30, 0, 8), 0, None),        # a length < 1
    ((30, -4), 0, None),
    ((), 0, None),                # count < 1
    ((30, 8), 28, None),          # beyond the longest member's last level (27)
    ((8, 30), 28, None),
    ((1,), -1, None),             # n = 1 has the launches of t = -3 and -2 only
    ((30,), -4, None),
    ((30, 8), 0, (3, -1)),        # a negative item count
    ((30, 1024), 0, None),
])
def test_bad_arguments(lengths, t, items):
    with pytest.raises(CCJError) as e:
        pf_level_plan(lengths, t, items)
    assert e.value.code == ccj_amd.CCJ_E_ARG


def test_item_counts_must_match_the_members():
    with pytest.raises(CCJError):
        pf_level_plan((30, 8), 0, (3,))
    assert pf_level_plan((30,), 27)["k_pf_level"][0] == (1, 28, 1)
