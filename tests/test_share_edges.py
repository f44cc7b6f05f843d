"""Split-point sharing in the gap columns whose other gap is short, on the CPU.

A leader's term for follower r at split point s reads a W operand of span s+r-1, which level t
has only for s <= a+b-r.  Where the other gap is below r the leader leaves its top r-b (r-a) split
points out of that follower's partial and the follower scans them itself.  Everything here comes
from the library's own role function through ccj_share_roles (include/ccj.h: the function
level4d_body and the leader lists call): no test restates it.

1. every cell's split points are covered exactly once by its leader's partial and its own scans;
2. every point a leader reduces for a follower has its W operand at that level;
3. columns that shared before (both gaps >= 3) have the roles and counts of CCJ_SHARE_EDGES=0;
4. at n = 200 under the default target the leader launch shrinks as modelled and no sharing level
   loses its leader launch.
"""
import functools

import pytest

from ccj_amd import DEFAULT_SPLIT_TARGET, level_layout, share_roles

R = 4
NS = (20, 64, 168, 200)
TARGETS = (0, DEFAULT_SPLIT_TARGET)  # 0: what the option's -1 resolves to (never split: every level shares)


@functools.lru_cache(maxsize=None)
def roles(n, target, edges):
    """{(t, a): ShareRoles} for every a-block of every level"""
    return {(t, a): share_roles(n, t, a, target, edges) for t in range(n - 2) for a in range(t + 1)}


def sides(n, target, edges):
    """(t, a, side, len, oth, SideRole, leader's (t, a)) for both sides of every block"""
    rr = roles(n, target, edges)
    for (t, a), x in rr.items():
        b = t - a
        yield t, a, 0, a, b, x.a_side, (t - a % R, a - a % R)  # i / j side: leader in block a - r
        yield t, a, 1, b, a, x.b_side, (t - b % R, a)          # k / l side: leader in the same block


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("n", NS)
def test_split_points_are_covered_exactly_once(n, target):
    rr = roles(n, target, True)
    g_lo, g_hi = rr[0, 0].g_lo, rr[0, 0].g_hi
    if target == 0:
        assert (g_lo, g_hi) == (0, n - 2)
    seen_cut = set()
    for t, a, side, ln, oth, s, lead in sides(n, target, True):
        cover = [0] * (ln + 1)
        assert 0 <= s.top and 0 <= s.low and s.low + s.top <= ln
        for p in list(range(1, s.low + 1)) + list(range(ln - s.top + 1, ln + 1)):
            cover[p] += 1
        r = ln % R
        if not g_lo <= t < g_hi:
            assert s.role == 0 and not rr[t, a].sharing
        elif r == 0:
            assert s.role == 1
        elif t - r < g_lo:
            assert s.role == 0  # its leader would lie below g_lo: it scans everything itself
        else:
            assert s.role == 2 and s.low == r
        if s.role == 2:
            L = rr[lead].b_side if side else rr[lead].a_side
            assert L.role == 1 and L.low == ln - r
            cut = L.cuts[r - 1]
            seen_cut.add((r, oth, cut))
            for p in range(1, ln - r - cut + 1):  # the leader's unmasked range, in the follower's numbering
                cover[p + r] += 1
        else:
            assert (s.low, s.top) == (ln, 0)
        assert cover[1:] == [1] * ln, (n, target, t, a, side, s)
    if g_hi > g_lo:  # every short-gap cut occurs, and no column that shared before has one
        assert {(r, o, c) for r, o, c in seen_cut if c} == {(r, o, r - o) for r in (1, 2, 3) for o in range(r)}


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("n", NS)
def test_leader_reduces_only_available_operands(n, target):
    for t, a, side, ln, oth, s, _ in sides(n, target, True):
        if s.role != 1:
            assert s.cuts == (0, 0, 0)
            continue
        for r in (1, 2, 3):
            cut = s.cuts[r - 1]
            assert 0 <= cut <= 3
            # W(i-r, i+s-1) / W(j-s+1, j+r) (k, l alike) has span s+r-1; k_diag2d(t-1) is the last before level t
            assert all(p + r - 1 <= t - 1 for p in range(1, ln - cut + 1)), (n, target, t, a, side, r)
            # and the cut is no larger than that asks for
            assert cut == 0 or (ln - cut + 1) + r - 1 > t - 1


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("n", NS)
def test_columns_that_shared_before_are_untouched(n, target):
    on, off = roles(n, target, True), roles(n, target, False)
    for (t, a), x in on.items():
        y = off[t, a]
        assert (x.sharing, x.g_lo, x.g_hi) == (y.sharing, y.g_lo, y.g_hi)
        b = t - a
        if min(a, b) >= R - 1:
            assert x == y, (n, target, t, a)
        for s, oth in ((y.a_side, b), (y.b_side, a)):  # off: a short other gap scans in full
            if oth < R - 1:
                assert (s.role, s.top, s.cuts) == (0, 0, (0, 0, 0))
        for s in (x.a_side, x.b_side):
            if s.top:
                assert s.role == 2 and min(a, b) < R - 1


def _lead_launch(n, target, edges):
    """blocks, cells and cell-steps of k_level4d_lead summed over the sharing levels"""
    blocks = cells = steps = 0
    for (t, a), x in roles(n, target, edges).items():
        if x.in_lead:
            M = level_layout(n, t, 1)[1]
            blocks += 1
            cells += M
            steps += M * (x.a_side.low + x.a_side.top + x.b_side.low + x.b_side.top)
    return blocks, cells, steps


def test_leader_launch_shrinks_at_n200():
    n, target = 200, DEFAULT_SPLIT_TARGET
    on, off = roles(n, target, True), roles(n, target, False)
    g_lo, g_hi = on[0, 0].g_lo, on[0, 0].g_hi
    assert (g_lo, g_hi) == (17, n - 2)
    for t in range(g_lo, g_hi):  # lead_split is 0 only for an empty list: a block with a % 4 == 0 always stays
        assert any(on[t, a].in_lead for a in range(t + 1)), t
        assert all(on[t, a].in_lead for a in range(0, t + 1, R))
        # three of every four short-gap a-blocks leave the leader launch where they have a leader
        for a in range(max(0, t - 2), t + 1):
            assert off[t, a].in_lead
            assert on[t, a].in_lead == (a % R == 0 or (t - a) % R == 0 or t - a % R < g_lo or t - (t - a) % R < g_lo)
    b_on, c_on, s_on = _lead_launch(n, target, True)
    b_off, c_off, s_off = _lead_launch(n, target, False)
    assert b_on < b_off and c_on < c_off and s_on < s_off
    # the model of the change: 31.4 M -> 28.5 M cells, 1.62 G -> 1.35 G cell-steps
    assert (round(c_off / 1e6, 1), round(c_on / 1e6, 1)) == (31.4, 28.5)
    assert (round(s_off / 1e9, 2), round(s_on / 1e9, 2)) == (1.62, 1.35)
