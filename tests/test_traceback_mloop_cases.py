"""CPU tests of tests/golden/traceback_mloop_cases.json (oracle/gen_traceback_mloop_cases.py): folds
with a strongly negative bp, under which the reference's own traceback enters the multiloop-family
nodes (P_P{L,R,M,O}mloop / ...00 / ...01 / ...10, P_WB, P_WBP and the multiloop sub-case of P_PL /
P_PR / P_PM / P_PO) that tests/golden/traceback_cases.json lists as unreached.

  * the C restatement, given each case's penalties, reproduces the reference's 31 hashes and W(n);
  * the domain: no 4-D store of any case lies below -32768 (OracleFold.low_stores() == 0; below that
    the reference's int16 store wraps and the engine does not follow), and a control
    fold outside the domain shows that the counter counts;
  * the invariants the engine's 2-D tables and closed forms rest on hold under these penalties: the
    closed forms of ccj_pmpo2d.h (the header's own host code) and the two-index property of the PL /
    PR families, zero differences on every case;
  * the fixture's own conditions.
"""
import ctypes

import pytest

from tests.mloop2d_cases import FAMILY_L, FAMILY_R, rseq, valid_cells
from tests.oracle_lib import HASH_NAMES, OracleFold, blob, golden
from tests.schedule_rows import ALL_REGIME_TARGET
from tests.test_pmpo_closed_invariant import SIX as CLOSED_SIX
from tests.test_pmpo_closed_invariant import _closed

DOC = golden("traceback_mloop_cases.json")
CASES = DOC["cases"]
TWELVE = FAMILY_L + FAMILY_R + CLOSED_SIX  # the IN_TAB and IN_CF matrices (ccj_engine.h carrier)
# every one of the twelve holds more values below 32767 than this in every case; the smallest count
# the restatement shows is 2275 (PLmloop10 at n = 18; test_tables_and_closed_forms_hold prints them)
MIN_FINITE = 1000

LABELS = [f"P_P{f}mloop{s}" for f in "LRMO" for s in ("", "00", "01", "10")] + ["P_WB", "P_WBP"]
# the multiloop sub-case (best_row 2) of P_PL / P_PR / P_PM / P_PO, by reference line (pseudo_loop.cc)
MLOOP_SUB_CASES = ["P_PL@1051", "P_PR@1116", "P_PM@1188", "P_PO@1248"]
# a fold outside the domain: ap = bp = -12500 at n = 24 (PL = PLmloop + ap + 2 bp falls below -32768)
CONTROL = (rseq(4201, 24, "GGCCAU"), "Turner04", 2,
           (-138, 1007, 1500, 246, 6, 96, 339, 3, 2, -12500, -12500, 12, 0.89, 0.74))

_folds = {}


def case_id(c):
    return f"n{len(c['seq'])}-{c['params']}-d{c['dangles']}-bp{c['pen'][10]}-{c['seq'][:6]}{len(c['entered'])}"


def _fold(case):
    """One restatement fold per case, shared by the tests of this file and never changed."""
    key = case_id(case)
    if key not in _folds:
        _folds[key] = OracleFold(case["seq"], blob(case["params"]), case["dangles"], case["noGU"], pen=case["pen"])
    return _folds[key]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_oracle_with_penalties_matches_reference(case):
    o = _fold(case)
    got = o.hashes()
    assert list(case["hashes"]) == HASH_NAMES
    bad = [k for k in case["hashes"] if got[k] != case["hashes"][k]]
    assert not bad, f"matrices differ from the reference: {bad}"
    assert o.W(o.n) == case["mfe"]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_case_lies_inside_the_int16_domain(case):
    assert _fold(case).low_stores() == 0


def test_counter_counts_outside_the_domain():
    """The control fold stores values below -32768; the level-parallel fill counts the same number
    (the counter is per fold and updated atomically) and computes the same matrices."""
    seq, params, d, pen = CONTROL
    a = OracleFold(seq, blob(params), d, 0, pen=pen)
    b = OracleFold(seq, blob(params), d, 0, pen=pen, threads=4)
    c = OracleFold(seq, blob(params), d, 0)  # default penalties: a counter of its own, at 0
    try:
        print(f"control: {a.low_stores()} stores below -32768 (sequential), {b.low_stores()} (level-parallel)")
        assert a.low_stores() > 0
        assert a.low_stores() == b.low_stores()
        assert a.hashes() == b.hashes()
        assert c.low_stores() == 0
    finally:
        a.close()
        b.close()
        c.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_tables_and_closed_forms_hold(case):
    o = _fold(case)
    n = o.n
    cells = list(valid_cells(n))
    finite = {}
    # PL / PR families: functions of (i, j) / (k, l) alone (tests/test_mloop2d_invariant.py)
    for names, key in ((FAMILY_L, lambda c: c[:2]), (FAMILY_R, lambda c: c[2:])):
        for nm in names:
            x = HASH_NAMES.index(nm)
            first, diffs, fin = {}, 0, 0
            for c in cells:
                v = o.get4(x, *c)
                fin += v < 32767
                diffs += first.setdefault(key(c), v) != v
            finite[nm] = fin
            assert diffs == 0, f"{nm}: {diffs} of {len(cells)} cells differ from the first cell of their 2-D key"
    # PM / PO families: the closed forms (tests/test_pmpo_closed_invariant.py)
    wbp = (ctypes.c_int * ((n + 1) * (n + 1)))()
    for i in range(1, n + 1):
        for j in range(i, n + 1):
            wbp[i * (n + 1) + j] = o.get2(1, i, j)
    got = _closed(n, wbp, case["pen"][10], case["pen"][11], len(cells))
    for m, nm in enumerate(CLOSED_SIX):
        x = HASH_NAMES.index(nm)
        diffs, fin, first = 0, 0, None
        for c, cell in enumerate(cells):
            want = o.get4(x, *cell)
            g = got[m * len(cells) + c]
            fin += want < 32767
            if g != want:
                diffs += 1
                first = first or (cell, g, want)
        finite[nm] = fin
        assert diffs == 0, f"{nm}: {diffs} of {len(cells)} cells differ, first (cell, closed form, oracle) = {first}"
    print(f"{case_id(case)}: {len(cells)} cells, 0 differences, below 32767: {finite}")
    for nm in TWELVE:
        assert finite[nm] > MIN_FINITE, f"{nm}: only {finite[nm]} values below 32767 (the check would be vacuous)"


def test_fixture_conditions():
    entered = set()
    for c in CASES:
        entered |= set(c["entered"])
    unreached = {u["id"]: u["reason"] for u in DOC["unreached"]}
    assert len(unreached) == len(DOC["unreached"])
    # every multiloop-family node is pinned by a reference run
    missing = [i for i in LABELS + MLOOP_SUB_CASES if i not in entered]
    assert not missing, missing
    assert DOC["mloop_sub_cases"] == MLOOP_SUB_CASES
    # the static parse: entered or unreached, never both
    ids = DOC["ids"]
    assert set(LABELS + MLOOP_SUB_CASES) <= set(ids) and len(set(ids)) == len(ids)
    assert all("mloop" in i or i.startswith("P_WB") or i in MLOOP_SUB_CASES for i in ids)
    family = {i for i in entered | set(unreached) if "mloop" in i or i.startswith("P_WB")} | set(MLOOP_SUB_CASES)
    assert family == set(ids), sorted(family ^ set(ids))
    assert set(unreached) <= set(ids)
    assert not entered & set(unreached), sorted(entered & set(unreached))
    # P_POmloop10's second sub-case is reached by the search, but only where the reference's stores wrap
    assert unreached["P_POmloop10@2812"].startswith("entered only by folds outside the int16 range")
    for i, why in unreached.items():
        assert "@" in i, i  # sub-cases only: every label is entered
        assert why.startswith("entered only by folds outside the int16 range") or "search budget exhausted" in why, (i, why)
    rcs = {c["rc"] for c in CASES}
    assert 0 in rcs and rcs - {0}, rcs
    default = DOC["pen_default"]
    assert default == [-138, 1007, 1500, 246, 6, 96, 339, 3, 2, 341, 56, 12, 0.89, 0.74]
    for c in CASES:
        assert set(c) >= {"seq", "params", "dangles", "noGU", "pen", "rc", "stdout", "stderr", "hashes", "mfe",
                          "entered", "source"}
        assert c["entered"], c["source"]
        assert len(c["pen"]) == 14 and c["pen"][10] < 0, c["source"]
    ns = sorted(len(c["seq"]) for c in CASES)
    assert ns[-1] <= 64
    assert sum(1 for n in ns if n <= 34) * 2 > len(ns), "most cases are at n <= 34"
    # the launch-regime band
    band = [c for c in CASES if len(c["seq"]) in ALL_REGIME_TARGET and any("mloop" in i for i in c["entered"])]
    fams = {i.split("@")[0][2:4] for c in band for i in c["entered"] if "mloop" in i.split("@")[0]}
    assert len(band) >= 2 and len(fams) >= 2, (len(band), fams)
