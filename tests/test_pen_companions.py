"""CPU tests of tests/pen_companions.py: the conditions under which tests/test_gpu_pen_contexts.py means
something, for exactly the folds it runs.

  * the selection is the one the GPU file's batches were made for;
  * every kept (case, sequence) lies inside the int16 domain (OracleFold.low_stores() == 0; DESIGN.md
    §1): outside it the engine is not held to the restatement;
  * on each case's own sequence the restatement, which is the companions' expectation, reproduces the
    reference's 31 hashes and W(n);
  * the multiloop folds at n <= 34 are dense in the twelve table-carried matrices, the state a stale or
    mis-indexed table entry would show in;
  * the cap on dropped companions.
"""
import pytest

from tests.pen_companions import (CASES, COMPANIONS, DROPPED, MIN_DENSE, MLOOP_CASES, OWN, PAIR_CASES, SAME_LENGTH,
                                  SPLIT_CASE, STP_CASES, case_id, companions, restated, sequences)

FOLDS = [(c, name) for c in CASES for name in sequences(c)]


def _fold_id(f):
    return f"{case_id(f[0])}-{f[1]}"


def test_selection():
    assert len(MLOOP_CASES) == 22 and all(c["pen"][10] < 0 for c in MLOOP_CASES)
    assert sorted(len(c["seq"]) for c in STP_CASES) == [48, 52, 53]
    assert sorted(tuple(c["pen"][12:]) for c in STP_CASES) == [(1.2, 0.4), (2.67, 7.4), (4.0, 0.74)]
    a, b = PAIR_CASES
    assert a["pen"] == b["pen"] and a["seq"] != b["seq"] and len(a["seq"]) == len(b["seq"]) == 49
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids) == 27
    assert sum(c["rc"] == 1 for c in MLOOP_CASES) == 8


def test_companion_rule():
    s = "GGGAAACUUCGGUCCCAAGGA"
    got = companions(s)
    assert tuple(got) == COMPANIONS
    assert [len(got[k]) for k in COMPANIONS] == [18, 14, 19, 14, 21, 21]
    assert got["head3"] == "GGGAAACUUCGGUCCCAA" and got["head7"] == "GGGAAACUUCGGUC"
    assert got["tail2"] == "GAAACUUCGGUCCCAAGGA" and got["mid"] == "AAACUUCGGUCCCA"
    assert got["reverse"] == s[::-1] and sorted(got["shuffle"]) == sorted(s) and got["shuffle"] not in (s, s[::-1])
    assert companions(s) == got  # the shuffle is seeded by the length alone


def test_dropped_companions_stay_within_the_cap():
    """A companion is dropped only for lying outside the domain (the int16 range, or a traceback the
    reference itself does not finish), and at most one per case: each case keeps one companion of its
    own length and two shorter ones of different lengths."""
    assert set(DROPPED) <= {case_id(c) for c in CASES} and sum(len(v) for v in DROPPED.values()) == 1
    for c in CASES:
        kept = [k for k in sequences(c) if k != OWN]
        assert len(kept) >= 5 and set(kept) <= set(COMPANIONS)
        seqs = sequences(c)
        assert any(k in SAME_LENGTH for k in kept)
        assert len({len(seqs[k]) for k in kept if len(seqs[k]) < len(c["seq"])}) >= 2
        assert len(set(seqs.values())) == len(seqs)  # seven different folds


def test_split_case_reaches_every_split_of_the_batched_launch():
    """Asked of ccj_batch_level_plan, the function the launch itself uses, for the seven lengths the GPU
    test folds under each target."""
    from tests.lockstep_rows import TARGET_SPLITS, splits
    lengths = [len(s) for s in sequences(SPLIT_CASE).values()]
    assert len(lengths) == 7 and 57 <= max(lengths) <= 59
    got = {target: splits(lengths, target) for target in TARGET_SPLITS}
    print(got)
    assert set().union(*got.values()) == {1, 2, 4, 8}


@pytest.mark.parametrize("fold", FOLDS, ids=_fold_id)
def test_fold_lies_inside_the_int16_domain(fold):
    assert restated(*fold)["low_stores"] == 0


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_restatement_reproduces_the_fixture(case):
    r = restated(case, OWN)
    bad = [k for k in case["hashes"] if r["hashes"][k] != case["hashes"][k]]
    assert len(case["hashes"]) == 31 and not bad, f"matrices differ from the reference: {bad}"
    assert r["mfe"] == case["mfe"]


@pytest.mark.parametrize("fold", [f for f in FOLDS if f[0] in MLOOP_CASES and len(f[0]["seq"]) <= 34], ids=_fold_id)
def test_multiloop_folds_are_dense_in_the_table_carried_matrices(fold):
    """The smallest count the restatement shows over these folds is 3576 (n = 11); the bound only keeps
    the GPU tests from going silent."""
    assert restated(*fold)["dense"] >= MIN_DENSE
