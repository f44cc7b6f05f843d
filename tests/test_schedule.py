"""The level schedule on the CPU: which launch regime each level of the chain k_level4d ->
k_level4d_lead runs in, read from the library's own schedule function
(include/ccj.h ccj_level_schedule: the function create_impl and the two launchers call).

The regime is decided by n and the split target alone, so a tuning constant can move whole
regimes out of the suite's reach without any test noticing.  These tests pin what the rows of
tests/schedule_rows.py reach (tests/test_gpu_schedule.py runs those rows on the GPU and asserts
the same through the context getter) and what the default target reaches at the sizes the rest of
the suite folds; a change of the heuristic or its default then fails here.
"""
import pytest

from ccj_amd import DEFAULT_SPLIT_TARGET, CCJError, level_schedule
from tests.oracle_lib import HASH_NAMES, OracleFold, blob, first_difference, golden
from tests.schedule_rows import (ALL_REGIMES, ALL_REGIME_TARGET, BOUNDARY_TARGET, SHARDED, flips, nlev, regimes,
                                 schedule, share_range, signature)

FIXTURE_NS = sorted({len(c["seq"]) for c in golden("hashes.json") if len(c["seq"]) >= 51})
# the smallest n whose default schedule shares at all (DEFAULT_SPLIT_TARGET = 9216)
FIRST_SHARING_N = 159


def test_fixture_sizes_are_the_ones_the_rows_cover():
    assert FIXTURE_NS == [52, 54, 55]
    assert set(FIXTURE_NS) <= set(ALL_REGIME_TARGET) and set(BOUNDARY_TARGET) == set(FIXTURE_NS)
    assert {n for n, _, _ in SHARDED} == set(FIXTURE_NS)


@pytest.mark.parametrize("n,target", sorted(ALL_REGIME_TARGET.items()))
def test_all_regime_rows_reach_every_regime(n, target):
    """World 1: plain splits 2, 4, 8 below the sharing range, lead splits 2, 4, 8 inside it, and a
    sharing range that starts above level 0 (so the leaderless followers exist)."""
    assert regimes(n, target) == ALL_REGIMES
    g_lo, g_hi = share_range(n, target)
    assert 0 < g_lo < g_hi == nlev(n)
    # the smallest multiple of 8 that does: the next one down misses a regime or the boundary
    assert target % 8 == 0
    assert not (regimes(n, target - 8) >= ALL_REGIMES and share_range(n, target - 8)[0] > 0)


def test_no_all_regime_target_below_n51():
    """The fixtures with n >= 51 are the smallest shapes at which every regime can go wrong."""
    for n in range(8, 51):
        for target in range(8, 1200, 8):
            assert not (regimes(n, target) >= ALL_REGIMES and share_range(n, target)[0] > 0), (n, target)


@pytest.mark.parametrize("row", sorted(SHARDED), ids=lambda r: "n%d-t%d-w%d" % r)
def test_sharded_rows_reach_the_stated_union(row):
    n, target, world = row
    assert target == ALL_REGIME_TARGET[n]
    got = regimes(n, target, world)
    assert got == SHARDED[row]
    assert (1, 8) in got and (8, 0) in got and (1, 4) in got
    # the range itself does not depend on the world or the rank
    for r in range(world):
        s = level_schedule(n, 0, world, r, target)
        assert (s.g_lo, s.g_hi) == share_range(n, target)
    # lead split 8 on at least one rank, and every rank leads somewhere
    per_rank = [{s.lead_split for s in schedule(n, target, world, r)} for r in range(world)]
    assert any(8 in p for p in per_rank) and all(p - {0} for p in per_rank)


def test_boundary_rows_cover_every_class():
    """g_lo mod 4 decides which followers of levels g_lo .. g_lo+2 have no leader: all four classes
    per fixture size, each on a schedule that shares with g_lo > 0."""
    for n, rows in BOUNDARY_TARGET.items():
        assert sorted(rows) == [0, 1, 2, 3]
        for cls, target in rows.items():
            g_lo, g_hi = share_range(n, target)
            assert 0 < g_lo < g_hi == nlev(n) and g_lo % 4 == cls and target % 8 == 0, (n, cls, target)
            assert {(1, 2), (1, 4)} <= regimes(n, target)
    # n = 55: every class under an all-regime target
    assert all(regimes(55, t) == ALL_REGIMES for t in BOUNDARY_TARGET[55].values())
    # and the all-regime rows alone already take all four values
    assert {share_range(n, t)[0] % 4 for n, t in ALL_REGIME_TARGET.items() if n in FIXTURE_NS} | \
           {share_range(55, t)[0] % 4 for t in BOUNDARY_TARGET[55].values()} == {0, 1, 2, 3}


def test_threshold_targets_at_n55():
    """The targets test_gpu_schedule.py runs on either side of: between the first all-regime target
    and the target at which n = 55 stops sharing, every change of g_lo or of a level's lead split."""
    lo, hi = ALL_REGIME_TARGET[55], 400
    fl = flips(55, lo - 1, hi)
    assert fl == [352, 360, 364, 368, 376, 384, 390, 392, 396, 400]
    g = [share_range(55, t)[0] for t in fl]
    assert g == [11, 12, 14, 14, 14, 14, 17, 17, 19, 0]
    assert share_range(55, 400) == (0, 0) and share_range(55, 399) == (19, 53)
    for t in fl:
        assert signature(55, t) != signature(55, t - 1)


def test_default_schedule_coverage():
    """Under the default target nothing below n = 159 shares, so the n = 100 / 150 fixtures and every
    small-n test run k_level4d's split loops only; the n >= 200 fixtures and n = 400 share with all
    three lead splits.  A change of the default that moves this trips here."""
    assert DEFAULT_SPLIT_TARGET == 9216
    first = next(n for n in range(3, 400) if share_range(n)[1] > 0)
    assert first == FIRST_SHARING_N
    assert all(share_range(n) == (0, 0) for n in range(1, FIRST_SHARING_N))
    large = sorted({c["n"] for c in golden("hashes_large.json")})
    assert large == [100, 150, 200, 220, 230]
    n400 = {c["n"] for c in golden("hashes_n400.json")}
    assert n400 == {400}
    for n in large + [400]:
        got = regimes(n, DEFAULT_SPLIT_TARGET)
        if n < FIRST_SHARING_N:
            assert share_range(n) == (0, 0) and got <= {(2, 0), (4, 0), (8, 0)}, n
        else:
            g_lo, g_hi = share_range(n)
            assert 0 < g_lo < g_hi == nlev(n), n
            assert {(1, 2), (1, 4), (1, 8)} <= got, n
    # the size test_gpu_share.py adds to reach the default sharing schedule
    assert regimes(168, DEFAULT_SPLIT_TARGET) == ALL_REGIMES and share_range(168)[0] > 0
    # 90 and 140 (test_sharing_on_off_identical) do not share by default: default == share off there
    for n in (90, 140):
        assert schedule(n, DEFAULT_SPLIT_TARGET) == schedule(n, DEFAULT_SPLIT_TARGET, share=False)


@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("n,target", sorted(ALL_REGIME_TARGET.items()) + [(30, 200), (100, 9216), (168, 9216), (200, 9216), (40, 0)])
def test_schedule_is_consistent(n, target, world):
    g_lo, g_hi = share_range(n, target)
    assert (g_lo, g_hi) == (0, 0) or (0 <= g_lo < g_hi == nlev(n))
    for r in range(world):
        sch = schedule(n, target, world, r)
        assert len(sch) == nlev(n)
        for t, s in enumerate(sch):
            assert (s.g_lo, s.g_hi) == (g_lo, g_hi)
            assert s.sharing == (g_lo <= t < g_hi)
            assert s.split in (0, 1, 2, 4, 8) and s.lead_split in (0, 2, 4, 8)
            if world == 1:
                assert s.split >= 1
            if s.sharing:
                assert s.split in (0, 1)               # the plain launch never splits where leaders run
                assert s.lead_split == 0 or s.lead_split >= 2
                if world == 1:
                    assert s.lead_split >= 2           # every unsharded sharing level has a leader block
            else:
                assert s.lead_split == 0
                if target > 0 and world == 1 and g_hi > g_lo:
                    assert s.split > 1                 # plain split is 1 exactly on the sharing levels
            if s.split == 0:
                assert s.lead_split == 0
    # a level without cells
    z = level_schedule(n, nlev(n), world, 0, target)
    assert (z.sharing, z.split, z.lead_split, z.g_lo, z.g_hi) == (False, 0, 0, g_lo, g_hi)


@pytest.mark.parametrize("n", [12, 55, 100, 200])
def test_share_off_and_target_zero_degenerate(n):
    """Sharing off: no range, no leader launch, the plain split as the heuristic gives it.  Target 0
    (the option's -1): nothing ever splits, so with sharing on every level shares at lead split 2."""
    for target in (0, 352, DEFAULT_SPLIT_TARGET):
        off = schedule(n, target, share=False)
        on = schedule(n, target)
        for t, (a, b) in enumerate(zip(off, on)):
            assert (a.sharing, a.lead_split, a.g_lo, a.g_hi) == (False, 0, 0, 0)
            assert a.split >= 1 and (a.split == b.split or b.sharing)
            if b.sharing:
                # the leaders split the narrow late levels as the plain launch would have
                assert b.lead_split == max(2, a.split)
    z = schedule(n, 0)
    assert share_range(n, 0) == (0, nlev(n))
    assert all(s.regime == (1, 2) and s.sharing for s in z)
    assert all(s.regime == (1, 0) for s in schedule(n, 0, share=False))


def test_bad_arguments():
    for args in [(0, 0, 1, 0, 352), (55, -1, 1, 0, 352), (55, 0, 0, 0, 352), (55, 0, 2, 2, 352), (55, 0, 1, 0, -1)]:
        with pytest.raises(CCJError):
            level_schedule(*args)


def test_first_difference_reports_the_first_cell_in_level_order():
    """The failure-localisation helper (tests/oracle_lib.py) on two CPU folds that differ (Turner04
    against DirksPierce09 tables): it must name a cell whose values differ, and no 4-D cell of an earlier level
    or an earlier position of that level may differ."""
    seq = "GGGAAACCCGGGAAACCCAAGGCC"
    a, b = OracleFold(seq, blob("Turner04"), 2, 0), OracleFold(seq, blob("DirksPierce09"), 2, 0)
    try:
        ha, hb = a.hashes(), b.hashes()
        bad = [k for k in ha if ha[k] != hb[k]]
        assert bad
        name = next(k for k in bad if k in HASH_NAMES[:22])
        d = first_difference(a.get4, b.get4, len(seq), [name])
        assert d is not None and d["matrix"] == name
        i, j, k, l = d["cell"]
        x = HASH_NAMES.index(name)
        assert d["got"] == a.get4(x, i, j, k, l) != b.get4(x, i, j, k, l) == d["want"]
        assert d["t"] == (j - i) + (l - k) and d["a"] == j - i
        # every cell the walk visits before it agrees
        n = len(seq)
        for t in range(d["t"] + 1):
            for aa in range(t + 1):
                for ii in range(1, n + 1):
                    jj = ii + aa
                    for kk in range(jj + 2, n + 1):
                        ll = kk + t - aa
                        if ll > n or (t, aa, ii, kk) >= (d["t"], d["a"], i, k):
                            continue
                        assert a.get4(x, ii, jj, kk, ll) == b.get4(x, ii, jj, kk, ll)
    finally:
        a.close()
        b.close()
