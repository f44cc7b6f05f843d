"""The lockstep batch's host side without a GPU: the batched level launch's plan
(ccj_batch_level_plan, the function the launch itself uses) against the members' own geometry, and
fold_many's planner (sorting by length, cutting into runs, restoring the input order).
"""
import random

import pytest

from ccj_amd import (DEFAULT_SPLIT_TARGET, CCJError, batch_level_plan, level_layout, plan_lockstep, shard_blocks)
from tests.lockstep_rows import LENGTHS, TARGET_SPLITS, levels, splits

SPLIT_RED = 10  # ints per lane a split wave hands over (ccj_kernels.hip); LDS = chunks * (split-1) * 10 * 64 * 4


def _geometry(n, t):
    """(a-blocks, 64-cell chunks per a-block) of level t of an unsharded fold of length n."""
    if n - t - 2 <= 0:
        return 0, 0
    nblk = len(shard_blocks(n, t, 1, 0))
    _, M = level_layout(n, t, 1)
    return nblk, (M + 63) // 64


@pytest.mark.parametrize("target", sorted(TARGET_SPLITS))
def test_plan_covers_every_members_waves_exactly(target):
    for t in range(levels(LENGTHS) + 2):
        p = batch_level_plan(LENGTHS, t, target)
        geo = [_geometry(n, t) for n in LENGTHS]
        total = sum(nblk * wpa for nblk, wpa in geo)
        if total == 0:  # past the longest member's last level
            assert tuple(p) == (0, 0, 0, 0, tuple((0, 0) for _ in LENGTHS))
            continue
        assert p.split in (1, 2, 4, 8)
        assert p.threads == (256 if p.split <= 4 else 64 * p.split)
        cpb = p.threads // 64 // p.split  # chunks per block
        assert cpb * p.split * 64 == p.threads
        assert p.lds == (cpb * (p.split - 1) * SPLIT_RED * 64 * 4 if p.split > 1 else 0)
        for n, (blocks, wpa), (nblk, want_wpa) in zip(LENGTHS, p.members, geo):
            waves = nblk * want_wpa
            if t >= n - 2:
                assert (blocks, wpa) == (0, 0) and waves == 0
                continue
            assert wpa == want_wpa and nblk == t + 1
            # the member's blocks hold its waves and not one block more
            assert (blocks - 1) * cpb < waves <= blocks * cpb
        assert p.grid_x == max(b for b, _ in p.members) > 0


@pytest.mark.parametrize("target,want", sorted(TARGET_SPLITS.items()))
def test_targets_reach_the_splits_the_gpu_test_folds_under(target, want):
    assert max(LENGTHS) <= 54
    assert splits(LENGTHS, target) == want


def test_every_split_is_reached():
    assert set().union(*(splits(LENGTHS, tg) for tg in TARGET_SPLITS)) == {1, 2, 4, 8}
    assert splits(LENGTHS, DEFAULT_SPLIT_TARGET) == {8}


def test_one_split_for_all_members_comes_from_the_total():
    """The split follows the launch's total wave count: members that alone would split further share
    the launch's one split, and a batch of K equal members splits like one member under target / K."""
    for t in (0, 10, 30):
        one = batch_level_plan([40], t, 512)
        four = batch_level_plan([40] * 4, t, 4 * 512)
        assert one.split == four.split and four.members == one.members * 4 and four.grid_x == one.grid_x


def test_plan_rejects_bad_arguments():
    for args in (([], 0, 512), ([0], 0, 512), ([1024], 0, 512), ([10], -1, 512), ([10], 0, -1)):
        with pytest.raises(CCJError):
            batch_level_plan(*args)


@pytest.mark.parametrize("k", [1, 2, 4, 7, 64])
def test_planner_runs_cover_the_input_once_in_length_order(k):
    r = random.Random(11)
    lengths = [r.randint(8, 48) for _ in range(24)]
    runs = plan_lockstep(lengths, k)
    assert all(1 <= len(run) <= k for run in runs)
    flat = [x for run in runs for x in run]
    assert sorted(flat) == list(range(len(lengths)))
    assert [lengths[x] for x in flat] == sorted(lengths)
    # restoring the order: writing each run's results back by index gives the input order
    out = [None] * len(lengths)
    for run in runs:
        for x in run:
            out[x] = lengths[x]
    assert out == lengths


def test_planner_single_sequence_and_k1():
    assert plan_lockstep([17], 4) == [[0]]
    assert plan_lockstep([5, 3, 9], 1) == [[1], [0], [2]]
    assert plan_lockstep([], 4) == []
    assert plan_lockstep([5, 5, 5], 2) == [[0, 1], [2]]  # ties keep the input order
