"""CPU tests of tests/golden/traceback_cases.json (oracle/gen_traceback_cases.py): folds chosen so
that the reference's own traceback (pseudo_loop::backtrack, W_final::backtrack) enters every case
and sub-branch a search could reach, several of them with non-default pseudoknot penalties.

  * the C restatement of the fill, given each case's penalties, reproduces the reference's 31
    matrix hashes and W(n): this pins OracleFold(..., pen=...) against `ref_driver hash --pen`;
  * the fixture itself is complete: every traceback label of ccj_backtrack.h and every listed
    W_final sub-case is either entered by some case or in `unreached` with its reason.
"""
import os
import re

import pytest

from tests.oracle_lib import ROOT, OracleFold, blob, golden

DOC = golden("traceback_cases.json")
CASES = DOC["cases"]


def case_id(c):
    pen = "pen" if c["pen"] else "def"
    return f"n{len(c['seq'])}-{c['params']}-d{c['dangles']}-g{c['noGU']}-{pen}-{c['seq'][:6]}{len(c['entered'])}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_oracle_with_penalties_matches_reference(case):
    n = len(case["seq"])
    # the level-parallel restatement above n = 64 (seconds instead of a minute at n = 100)
    o = OracleFold(case["seq"], blob(case["params"]), case["dangles"], case["noGU"], pen=case["pen"],
                   threads=None if n <= 64 else 0)
    try:
        got = o.hashes()
        assert len(case["hashes"]) == 31
        bad = [k for k in case["hashes"] if got[k] != case["hashes"][k]]
        assert not bad, f"matrices differ from the reference: {bad}"
        assert o.W(n) == case["mfe"]
    finally:
        o.close()


def p_labels():
    """The case labels of pseudo_loop::backtrack as the engine names them: bt_case_name's, plus the
    two PfromM helper nodes (constants of ccj_backtrack.h without an exit message of their own)."""
    with open(os.path.join(ROOT, "ccj_amd", "csrc", "ccj_backtrack.h")) as f:
        src = f.read()
    names = set(re.findall(r'case (P_\w+): return "\1";', src))
    for extra in ("P_PfromMprime", "P_PfromMdoubleprime"):
        assert re.search(r"\b%s = '" % extra, src)
        names.add(extra)
    return names


# W_final::backtrack: nodes and sub-cases by reference line (W_final.cc)
W_FINAL = (["LOOP", "FREE", "M_WM", "M_WMv", "M_WMp"]
           + ["LOOP@%d" % k for k in (233, 308, 312, 316, 321, 326, 329, 332, 335)]  # INTER exit, multiloop 1-8
           + ["FREE@%d" % k for k in (485, 488, 494, 500, 506, 514, 520, 526, 532)]   # sub-cases 0-8
           + ["M_WM@%d" % k for k in (582, 583, 584, 588, 592)]
           + ["M_WMv@%d" % k for k in (638, 639, 640, 641, 642)]
           + ["M_WMp@662"])


def test_fixture_covers_every_label_or_says_why_not():
    entered = set()
    for c in CASES:
        entered |= set(c["entered"])
    unreached = {u["id"]: u["reason"] for u in DOC["unreached"]}
    assert len(unreached) == len(DOC["unreached"])
    labels = p_labels()
    assert len(labels) == 36
    required = labels | set(W_FINAL)
    union = entered | set(unreached)
    assert required <= union, sorted(required - union)
    # nothing else: every further id is a sub-branch LABEL@line of a known label
    known = labels | {"LOOP", "FREE", "M_WM", "M_WMv", "M_WMp"}
    stray = [i for i in union if i.split("@")[0] not in known or ("@" in i and not i.split("@")[1].isdigit())]
    assert not stray, stray
    assert not entered & set(unreached), sorted(entered & set(unreached))
    for i, why in unreached.items():
        assert len(why) > 40, (i, why)
        if "search budget exhausted" in why:
            assert DOC["search"]["searched_beyond_corpus"] >= 2000
    # what the corpus and the probes of the issue reached stays pinned
    for must in ("P_WPP", "P_PfromM", "P_PM", "P_PL", "P_PO", "P_P", "P_PK", "P_PR", "P_WP",
                 "P_PfromL", "P_PfromR", "P_PfromO", "P_PLiloop", "P_PRiloop", "P_PMiloop", "P_POiloop",
                 "LOOP", "FREE", "M_WM", "M_WMv"):
        assert must in entered, must


def test_fixture_conditions():
    default = DOC["pen_default"]
    assert default == [-138, 1007, 1500, 246, 6, 96, 339, 3, 2, 341, 56, 12, 0.89, 0.74]
    pens = [c["pen"] for c in CASES if c["pen"] is not None]
    assert all(len(p) == 14 and p != default for p in pens)
    assert len(pens) >= 6
    assert sum(1 for p in pens if p[12:] != default[12:]) >= 2, "e_stP / e_intP overrides"
    # sane range: each magnitude within 10x of its default, same sign
    for p in pens:
        for v, d in zip(p, default):
            assert v * d > 0 and abs(d) / 10 - 1e-9 <= abs(v) <= abs(d) * 10 + 1e-9, (p, v, d)
    ns = sorted(len(c["seq"]) for c in CASES)
    assert ns[-1] <= 100
    assert sum(1 for n in ns if n <= 64) * 2 > len(ns), "most cases are at n <= 64"
    for c in CASES:
        assert set(c) >= {"seq", "params", "dangles", "noGU", "pen", "rc", "stdout", "stderr", "hashes", "mfe",
                          "entered", "source"}
        assert c["entered"], c["source"]
