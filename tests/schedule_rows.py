"""The (n, split_target, world) rows at which the small-n GPU tests reach every launch regime of
the level chain — TEST INFRASTRUCTURE ONLY.

tests/test_schedule.py pins, on the CPU and through the library's own schedule function
(include/ccj.h ccj_level_schedule), what each row reaches; tests/test_gpu_schedule.py runs them
and asserts the same through the context getter.  Nothing here restates the heuristic: every
schedule value comes from ccj_amd.level_schedule.

A regime is (k_level4d's split, k_level4d_lead's split): (1, s) on a sharing level whose leader
launch runs s = 2, 4 or 8 waves per chunk, (p, 0) on a level that does not share and splits p ways,
(1, 0) on a sharing level where the rank launches no leader block and (0, 0) where the rank owns
no block at all (band-sharded early levels).
"""
from ccj_amd import DEFAULT_SPLIT_TARGET, level_schedule

ALL_REGIMES = frozenset({(1, 2), (1, 4), (1, 8), (2, 0), (4, 0), (8, 0)})

# n -> a split_target under which the unsharded fold reaches all six regimes with g_lo > 0: the
# smallest multiple of 8 that does (found by sweeping the target in steps of 8 with the helper;
# test_schedule.py checks both claims).  52, 54 and 55 are the n >= 51 reference fixtures of
# tests/golden/hashes.json; 57 .. 64 are the fresh oracle cases.
ALL_REGIME_TARGET = {52: 328, 54: 344, 55: 352,
                     57: 368, 58: 376, 59: 384, 60: 392, 61: 400, 62: 408, 63: 416, 64: 424}

# n -> {g_lo mod 4: target}: one sharing schedule with g_lo > 0 per class of the leaderless
# boundary (followers on g_lo .. g_lo+2 whose leader would lie below g_lo).  Where an all-regime
# target of that n has the class it is used (n = 55 has all four); the others share with lead
# splits 2 and 4 only.
BOUNDARY_TARGET = {52: {0: 336, 1: 272, 2: 328, 3: 304},
                   54: {0: 368, 1: 344, 2: 376, 3: 264},
                   55: {0: 360, 1: 392, 2: 368, 3: 352}}

# (n, target, world) -> the union over ranks of the regimes the band-sharded fold reaches.  A rank
# owns only the blocks with (a / 4) % world == rank, so it splits further than the whole level
# would: plain split 2 is gone from world 3 on, lead split 2 at world 4 (at n = 52 already at world
# 3), and (0, 0) appears on the early levels where a rank owns no block.  Lead split 8 stays on
# every row.
_W2 = ALL_REGIMES | {(0, 0)}
_W3 = _W2 - {(2, 0)}
_W4 = _W3 - {(1, 2)}
SHARDED = {(52, 328, 2): _W2, (54, 344, 2): _W2, (55, 352, 2): _W2,
           (52, 328, 3): _W4, (54, 344, 3): _W3, (55, 352, 3): _W3,
           (52, 328, 4): _W4, (54, 344, 4): _W4, (55, 352, 4): _W4}


def nlev(n):
    return max(n - 2, 0)


def schedule(n, target, world=1, rank=0, share=True):
    """[LevelSchedule of level t for t in 0 .. n-3]"""
    return [level_schedule(n, t, world, rank, target, share) for t in range(nlev(n))]


def regimes(n, target, world=1, share=True):
    """Union over ranks and levels of (plain split, lead split)."""
    return {s.regime for r in range(world) for s in schedule(n, target, world, r, share)}


def share_range(n, target=DEFAULT_SPLIT_TARGET, share=True):
    s = level_schedule(n, 0, 1, 0, target, share)
    return s.g_lo, s.g_hi


def signature(n, target):
    """What a target decides at this n for the unsharded fold: g_lo and every level's lead split."""
    return share_range(n, target)[0], tuple(s.lead_split for s in schedule(n, target))


def flips(n, lo, hi):
    """Targets in (lo, hi] at which g_lo or some level's lead split differs from target - 1."""
    out, prev = [], signature(n, lo)
    for tg in range(lo + 1, hi + 1):
        cur = signature(n, tg)
        if cur != prev:
            out.append(tg)
        prev = cur
    return out
