"""The edge of the domain of bit-identity, on the CPU (no GPU).

tests/golden/range_cases.json (tools/gen_range_cases.py) holds folds whose penalties pen_in / pen_out
differ by one unit of one penalty: under pen_in no 4-D value lies below -32768 before it is stored
(OracleFold.low_stores() == 0), under pen_out at least one does.  Here the restatement re-derives both
counts, and the host form of the closed-form range check (ccj_pmpo2d_low, ccj_amd/csrc/ccj_pmpo2d.h)
is held against a cell-by-cell minimum and against the restatement's stored values.
"""
import ctypes
import os

import pytest

from tests.mloop2d_cases import valid_cells
from tests.oracle_lib import HASH_NAMES, ROOT, OracleFold, blob, golden

LIB = os.path.join(ROOT, "ccj_amd", "lib", "libccj_hip.so")
SIX = ("PMmloop00", "PMmloop01", "PMmloop10", "POmloop00", "POmloop01", "POmloop10")
DOC = golden("range_cases.json")
CASES = DOC["cases"]
SHORT = [c for c in CASES if len(c["seq"]) <= 30]
LONG = [c for c in CASES if len(c["seq"]) > 30]

_folds = {}


def _fold(case, which):
    """One restatement fold per (case, pen_in / pen_out), shared and never changed."""
    key = (case["name"], which)
    if key not in _folds:
        seq = case["seq"]
        _folds[key] = OracleFold(seq, blob(case["params"]), case["dangles"], 0, threads=0 if len(seq) > 40 else None,
                                 pen=case[which])
    return _folds[key]


def _wbp(o, n):
    wbp = (ctypes.c_int * ((n + 1) * (n + 1)))()
    for i in range(1, n + 1):
        for j in range(i, n + 1):
            wbp[i * (n + 1) + j] = o.get2(1, i, j)
    return wbp


def _lib():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    L = ctypes.CDLL(LIB)
    ip = ctypes.POINTER(ctypes.c_int)
    L.ccj_pmpo2d_low.argtypes = [ctypes.c_int, ip, ctypes.c_int, ctypes.c_int, ip]
    L.ccj_pmpo2d_low_brute.argtypes = [ctypes.c_int, ip, ctypes.c_int, ctypes.c_int, ctypes.c_int, ip]
    return L


def _low(case, which, brute=None):
    """ccj_pmpo2d_low of the fold (brute: None, or valid_only of ccj_pmpo2d_low_brute)."""
    o = _fold(case, which)
    n = len(case["seq"])
    out = (ctypes.c_int * 6)()
    bp, cp = case[which][10], case[which][11]
    if brute is None:
        assert _lib().ccj_pmpo2d_low(n, _wbp(o, n), bp, cp, out) == 0
    else:
        assert _lib().ccj_pmpo2d_low_brute(n, _wbp(o, n), bp, cp, brute, out) == 0
    return list(out)


def test_fixture_covers_what_it_must():
    assert 12 <= len(CASES) <= 16 and len(LONG) == 1 and 57 <= len(LONG[0]["seq"]) <= 59
    assert LONG[0]["split_target"] > 0
    assert {c["params"] for c in CASES} >= {"Turner04", "DirksPierce09"}
    assert {c["dangles"] for c in CASES} == {0, 1, 2}
    assert {c["field"] for c in CASES} & {"cp", "PSM"}
    lowest_class = [min(c["lowest"], key=lambda k: c["lowest"][k][0]) for c in CASES]
    assert sum(k in ("IN_D4", "IN_REC") for k in lowest_class) >= 2
    only_tab_cf = [c for c in CASES if c["wrapped"] and all(m in HASH_NAMES[10:22] for m in c["wrapped"])]
    assert len(only_tab_cf) >= 2
    for c in CASES:
        d = [k for k in range(14) if c["pen_in"][k] != c["pen_out"][k]]
        assert len(d) == 1 and abs(c["pen_in"][d[0]] - c["pen_out"][d[0]]) == 1, c["name"]
        assert c["low_in"] == 0 < c["low_out"]
    found = DOC["closed_form_first_search"]["found"]
    for nm in found:  # a fold whose only wrapped stores are closed-form ones
        c = next(c for c in CASES if c["name"] == nm)
        assert all(m in SIX for m in c["wrapped"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_pen_in_is_inside_and_pen_out_is_outside(case):
    assert _fold(case, "pen_in").low_stores() == 0
    assert _fold(case, "pen_out").low_stores() == case["low_out"] > 0


@pytest.mark.parametrize("case", SHORT, ids=lambda c: c["name"])
def test_low_equals_the_cell_by_cell_minimum(case):
    """The O(n^2) reduction against the minimum of the formulas' inner expressions over valid_cells(n)
    (which also holds the branch list against pmpo2d_eval at every valid cell)."""
    for which in ("pen_in", "pen_out"):
        assert _low(case, which) == _low(case, which, brute=1), which


@pytest.mark.parametrize("case", SHORT, ids=lambda c: c["name"])
def test_low_equals_the_lowest_stored_value_inside_the_domain(case):
    """At pen_in nothing wraps, so wherever a closed-form matrix holds a value below 32767 its lowest
    stored value is the lowest pre-clamp value."""
    o = _fold(case, "pen_in")
    n = len(case["seq"])
    got = _low(case, "pen_in")
    cells = list(valid_cells(n))
    checked = 0
    for m, nm in enumerate(SIX):
        x = HASH_NAMES.index(nm)
        want = min(o.get4(x, *c) for c in cells)
        if want < 32767:
            assert got[m] == want, (nm, got[m], want)
            checked += 1
        else:
            assert got[m] >= 32767, (nm, got[m])
    assert checked >= 1


def test_intervals_of_no_valid_cell_stay_out():
    """(i, j = n) has no k and (k < 3, l) has no i: the constrained minimum ignores them, and on at least
    one case the minimum over all interval pairs is strictly lower, so the two can be told apart."""
    strictly = 0
    for case in SHORT:
        con, unc = _low(case, "pen_in"), _low(case, "pen_in", brute=0)
        assert all(u <= c for u, c in zip(unc, con)), case["name"]
        strictly += any(u < c for u, c in zip(unc, con))
        assert con == _low(case, "pen_in", brute=1)
    assert strictly >= 1


def test_low_decides_the_closed_form_site():
    """Across pen_in / pen_out: some closed form below -32768 exactly where the restatement's wrapped
    stores include a closed-form matrix."""
    for case in SHORT:
        assert min(_low(case, "pen_in")) >= -32768, case["name"]
        cf_wraps = any(m in SIX for m in case["wrapped"])
        assert (min(_low(case, "pen_out")) < -32768) == cf_wraps, (case["name"], _low(case, "pen_out"), case["wrapped"])
