"""Lockstep batch (-m gpu): many sequences folded in one set of level launches (ccj_batch_*,
LockstepBatch, fold_many(lockstep=K), python -m ccj_amd.batch --lockstep K).

Every member of every fold is held against the reference's own run of its sequence
(tests/golden/hashes.json: all 31 hashes and the MFE; tests/golden/e2e.json: its last stdout line, or
its exit code and stderr).  The batches put members without any 4-D level (n <= 4) beside the longest,
are bound again to fewer and to other sequences (a stale argument row, descriptor or sentinel shows
there), fold under every split of the batched level launch, and are misused.
"""
import os
import random
import subprocess
import sys

import pytest

from tests.lockstep_rows import LENGTHS, TARGET_SPLITS, option, splits
from tests.oracle_lib import ROOT, golden
from tests.test_gpu_schedule import _check_reference, _result

pytestmark = pytest.mark.gpu

HASHES = golden("hashes.json")
E2E = golden("e2e.json")


def _group(params, dangles):
    return sorted((c for c in HASHES if (c["params"], c["dangles"], c["noGU"]) == (params, dangles, 0)),
                  key=lambda c: len(c["seq"]))


A = _group("Turner04", 2)
B = _group("DirksPierce09", 2)
D1 = _group("Turner04", 1)


def _batch(cases, capacity, members=None, **kw):
    from ccj_amd import LockstepBatch
    c = cases[0]
    return LockstepBatch(capacity, len(cases) if members is None else members, c["dangles"], params=c["params"],
                         noGU=bool(c["noGU"]), **kw)


def _fold_and_check(batch, cases):
    batch.bind([c["seq"] for c in cases])
    assert batch.count == len(cases) == len(batch.members)
    batch.fold()
    for wf, case in zip(batch.members, cases):
        assert (wf.n, wf.seq) == (len(case["seq"]), case["seq"])
        _check_reference(wf, case)


def test_fixture_groups_are_the_ones_the_batches_were_made_for():
    assert [len(c["seq"]) for c in A] == [1, 2, 3, 4, 9, 10, 12, 20, 22, 24, 24, 30, 30, 31, 32, 32, 33, 35, 42, 50, 54]
    assert [len(c["seq"]) for c in B] == [10, 14, 19, 25, 30, 32, 34, 39, 39, 40, 44, 50, 54]
    assert [len(c["seq"]) for c in D1] == [17, 32, 32, 37, 38, 47, 52, 55]


@pytest.mark.parametrize("cases", [A, B], ids=["Turner04-d2", "DirksPierce09-d2"])
def test_full_fixture_group_in_one_batch_and_rebound(cases):
    """The whole group as one batch of capacity 54; then the same batch bound to its short half only
    (the other members idle), then to its long half."""
    half = len(cases) // 2
    batch = _batch(cases, 54)
    try:
        assert batch.size == len(cases) and batch.count == 0
        _fold_and_check(batch, cases)
        _fold_and_check(batch, cases[:half])
        assert batch.count == half < batch.size
        _fold_and_check(batch, cases[half:])
        # longest first: every member's layout changes again
        _fold_and_check(batch, cases[::-1])
    finally:
        batch.close()


def test_reference_exits_do_not_disturb_the_other_members():
    batch = _batch(D1, 55)
    try:
        _fold_and_check(batch, D1)
        kinds = [(wf.n, _result(wf)[0]) for wf in batch.members]
        assert [n for n, k in kinds if k == "exit"] == [32, 47]
        assert sum(k == "ok" for _, k in kinds) == 6
        for wf in batch.members:
            assert (wf.exit is not None) == (wf.structure is None)
        exits = [wf.exit for wf in batch.members if wf.exit is not None]
        assert len(exits) == 2 and all("P_PR" in ex.msg for ex in exits)
    finally:
        batch.close()


@pytest.mark.parametrize("target", sorted(TARGET_SPLITS))
def test_every_split_regime(target):
    """One fold of the LENGTHS batch under each target of the CPU test; between them the four targets
    run the batched level launch with split 1, 2, 4 and 8."""
    by_n = {len(c["seq"]): c for c in A}
    cases = [by_n[n] for n in LENGTHS]
    assert splits(LENGTHS, target) == TARGET_SPLITS[target]
    batch = _batch(cases, 54, split_target=option(target))
    try:
        assert batch.members == [] and batch._all[0].schedule_options() == (target, False)
        _fold_and_check(batch, cases)
    finally:
        batch.close()


def test_the_targets_reach_every_split():
    assert set().union(*TARGET_SPLITS.values()) == {1, 2, 4, 8}


def test_degenerate_batches():
    by_n = {len(c["seq"]): c for c in A}
    one = _batch([by_n[33]], 33)
    try:
        _fold_and_check(one, [by_n[33]])
    finally:
        one.close()
    four = _batch([by_n[35]] * 4, 40)
    try:
        _fold_and_check(four, [by_n[35]] * 4)
        got = [(_result(wf), wf.hashes()) for wf in four.members]
        assert got[0] == got[1] == got[2] == got[3]
    finally:
        four.close()


def test_misuse_leaves_the_previous_binding_usable():
    from ccj_amd import CCJ_E_ARG, CCJ_E_STATE, CCJError, LockstepBatch
    by_n = {len(c["seq"]): c for c in A}
    cases = [by_n[35], by_n[12], by_n[3]]
    batch = _batch(cases, 42, members=3)

    def still_folds():
        assert [wf.seq for wf in batch.members] == [c["seq"] for c in cases]
        batch.fold()
        for wf, case in zip(batch.members, cases):
            _check_reference(wf, case)

    try:
        _fold_and_check(batch, cases)
        for bad in ([by_n[50]["seq"], by_n[12]["seq"]],            # longer than the capacity
                    [by_n[12]["seq"], "ACGUX" * 4],                 # a character outside ACGUT
                    [by_n[12]["seq"]] * 4,                          # count > members
                    []):                                            # count < 1
            with pytest.raises(CCJError) as e:
                batch.bind(bad)
            assert e.value.code == CCJ_E_ARG
            still_folds()
        wf = batch.members[0]
        for call in (lambda: wf.rebind(by_n[20]["seq"]), lambda: wf.reset(by_n[35]["seq"]), wf.fill, wf.fill_device,
                     wf.fill_async):
            with pytest.raises(CCJError) as e:
                call()
            assert e.value.code == CCJ_E_STATE
            still_folds()
        batch.fold_async()
        with pytest.raises(CCJError) as e:
            batch.bind([by_n[20]["seq"]])  # a fold is in flight
        assert e.value.code == CCJ_E_STATE
        batch.wait()
        for wf, case in zip(batch.members, cases):
            _check_reference(wf, case)
    finally:
        batch.close()
    for kw in (dict(shard_world=2), dict(host_traceback=True), dict(overlap_d2h=True), dict(share_splits=1)):
        with pytest.raises(CCJError) as e:
            LockstepBatch(20, 2, 2, params="Turner04", **kw)
        assert e.value.code == CCJ_E_ARG


def _random_seqs():
    r = random.Random(2024)
    return ["".join(r.choice("ACGU") for _ in range(r.randint(8, 48))) for _ in range(24)]


def test_fold_many_lockstep_equals_fold_many():
    from ccj_amd import fold_many
    seqs = _random_seqs()
    assert len(seqs) == 24 and min(map(len, seqs)) >= 8 and max(map(len, seqs)) <= 48
    want = fold_many(seqs, 2, params="Turner04")
    got = fold_many(seqs, 2, params="Turner04", lockstep=4)
    assert [r[0] for r in got] == seqs
    assert got == want


def test_batch_module_lockstep_prints_the_same_bytes(tmp_path):
    cases = [c for c in E2E if (c["params"], c["dangles"], c["noGU"]) == ("Turner04", 1, 0)]
    random.Random(7).shuffle(cases)
    f = tmp_path / "seqs.txt"
    # the file tests/test_gpu_rebind.py builds for its command-line case
    f.write_text("".join((c["seq"].lower().replace("u", "t") if k % 2 else c["seq"]) + "\n" for k, c in enumerate(cases)))
    runs = []
    for extra in ([], ["--lockstep", "4"]):
        runs.append(subprocess.run([sys.executable, "-m", "ccj_amd.batch", "-d", "1", "-P", "Turner04", *extra, str(f)],
                                   cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120))
    plain, lock = runs
    assert len(cases) == 10 and plain.returncode == 1
    assert (lock.stdout, lock.stderr, lock.returncode) == (plain.stdout, plain.stderr, plain.returncode)
    assert lock.stdout == "".join(c["stdout"] for c in cases)
