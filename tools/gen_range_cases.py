"""Generate tests/golden/range_cases.json: folds at the edge of the domain of bit-identity.

    python tools/gen_range_cases.py [-o tests/golden/range_cases.json]

CPU only, the C restatement only (tests/oracle_lib.py OracleFold).  A fold lies inside the domain iff
no 4-D value is below -32768 before it is stored, i.e. OracleFold.low_stores() == 0.  For every case
below, one penalty is bisected between a value inside and a value outside until two adjacent integers
remain: pen_in (low_stores 0) and pen_out (low_stores > 0).  Recorded per case:
  seq, params, dangles, field (the bisected penalty), pen_in, pen_out (14 values, ccj_pk_penalties order),
  low_in (0), low_out, split_target (0 = the default; TARGETS below),
  lowest: per carrier class (IN_D4 / IN_REC / IN_TAB / IN_CF) the lowest stored value at pen_in with its
          matrix and cell (found by walking get4 over the valid cells),
  wrapped: matrix -> [count, first cell] of the cells that pen_in stores within 100 of -32768 and
           pen_out stores within 100 of +32767 (the wrapped stores themselves, not what reads them),
  inside_prefixes: lengths m < n whose prefix seq[:m] stays inside the domain under pen_out
           (companions for a lockstep batch with the same penalties).
The header records the bounded search for a fold whose first wrap is in a closed-form matrix (PM / PO
multiloop families) while the PL / PR tables stay inside.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.mloop2d_cases import rseq, valid_cells  # noqa: E402
from tests.oracle_lib import HASH_NAMES, OracleFold, blob  # noqa: E402

PEN_DEFAULT = (-138, 1007, 1500, 246, 6, 96, 339, 3, 2, 341, 56, 12, 0.89, 0.74)
FIELDS = ("PS", "PSM", "PSP", "PB", "PUP", "PPS", "a", "b", "c", "ap", "bp", "cp", "e_stP", "e_intP")
CLASSES = {
    "IN_D4": ("PK", "PL", "PR", "PM", "PO", "PfromM"),
    "IN_REC": ("PfromL", "PfromR", "PfromMprime", "PfromO"),
    "IN_TAB": ("PLmloop00", "PLmloop01", "PLmloop10", "PRmloop00", "PRmloop01", "PRmloop10"),
    "IN_CF": ("PMmloop00", "PMmloop01", "PMmloop10", "POmloop00", "POmloop01", "POmloop10"),
}
# split targets other than the default (0): the long case folds under its all-regime target
# (tests/schedule_rows.py ALL_REGIME_TARGET[58]), so that leaders and ring partials are on the path; so
# does one short case, whose target makes every level a sharing level.  Its PUP is strongly negative:
# unpaired bases then lower a split term, the lowest PfromL values are sums over long unpaired heads,
# and the part of such a minimum that a follower takes from its leader's partial is itself below
# -32768 (at pen_out: the a-side partial of PfromL(1,22,24,30), a = 21, a follower of the leader a = 20).
TARGETS = {"n58_T04_d2_bp": 376, "n30_T04_d2_pupneg_bp": 8}

# (name, sequence, parameter set, dangles, fixed penalties, bisected field, value inside, value outside)
CASES = [
    ("n20_T04_d2_bp", "AGGCGAGCUCCGCGGACACG", "Turner04", 2, {}, "bp", -1000, -33000),
    ("n20_T04_d2_apneg_bp", "AGGCGAGCUCCGCGGACACG", "Turner04", 2, {"ap": -10000, "cp": -10}, "bp", -1000, -33000),
    ("n24_DP09_d1_bp", "AAGGUAUGCGGGGGUAAGCGGGCC", "DirksPierce09", 1, {}, "bp", -1000, -33000),
    ("n30_T04_d0_apneg_bp", "GCGCCCGGCGCGCGCCCGGCCGGGGGGCGG", "Turner04", 0, {"ap": -10000, "cp": -10}, "bp", -1000, -33000),
    ("n20_T04_d2_appos_bp", "AGGCGAGCUCCGCGGACACG", "Turner04", 2, {"ap": 30000}, "bp", -1000, -33000),
    ("n24_DP09_d1_appos_bp", "AAGGUAUGCGGGGGUAAGCGGGCC", "DirksPierce09", 1, {"ap": 30000}, "bp", -1000, -33000),
    ("n58_T04_d2_bp", "AGCCUUAAUAUCACGGCCAUGAUAUCGAAUGAGUGACUGGGACUAUUGUCAGCGAAGU", "Turner04", 2, {}, "bp", -1000, -33000),
    ("n26_DP09_d0_apneg_bp", rseq(7126, 26, "GCGCAU"), "DirksPierce09", 0, {"ap": -10000, "cp": -10}, "bp", -1000, -33000),
    ("n28_T04_d1_bp", rseq(7128, 28, "GGCCAU"), "Turner04", 1, {}, "bp", -1000, -33000),
    ("n24_T04_d1_cp", "AAGGUAUGCGGGGGUAAGCGGGCC", "Turner04", 1, {"bp": -6000}, "cp", 0, -6000),
    ("n22_DP09_d2_psm", rseq(7122, 22, "GCGCAU"), "DirksPierce09", 2, {"bp": -3000}, "PSM", 0, -33000),
    ("n27_DP09_d0_appos_bp", rseq(7127, 27, "GCGCAU"), "DirksPierce09", 0, {"ap": 30000}, "bp", -1000, -33000),
    ("n25_T04_d2_cpneg_cp", rseq(7125, 25, "GCGCAU"), "Turner04", 2, {"ap": 30000, "bp": -4000}, "cp", 0, -6000),
    # e_intP < 0 turns the interior loops' energies negative: the lowest PL / PR / PM values then come from
    # the interior-loop minima themselves (k_iloop), not from a stack or a multiloop term
    ("n29_T04_d0_eintneg_bp", rseq(7129, 29, "GGCCAU"), "Turner04", 0, {"e_intP": -0.74}, "bp", -500, -33000),
    ("n30_T04_d2_pupneg_bp", rseq(7130, 30, "GGCCAU"), "Turner04", 2, {"PUP": -300}, "bp", 56, -33000),
]
# bounded search for a closed-form-first fold: negative cp with both intervals long, ap large so that PL / PR / PM
# stay high, the bisection on cp or bp
CF_SEARCH = [
    ("cf_n24_cp", "AAGGUAUGCGGGGGUAAGCGGGCC", "Turner04", 2, {"ap": 30000, "bp": -2000}, "cp", 0, -8000),
    ("cf_n26_cp", rseq(7226, 26, "ACGU"), "DirksPierce09", 1, {"ap": 30000, "bp": -1000}, "cp", 0, -8000),
    ("cf_n22_cp", rseq(7222, 22, "GCAU"), "Turner04", 0, {"ap": 30000, "bp": 56}, "cp", 0, -12000),
    ("cf_n28_bp", rseq(7228, 28, "GCGCAU"), "Turner04", 2, {"ap": 30000, "cp": -600}, "bp", 56, -33000),
]


def pen_of(fixed, field, value):
    p = list(PEN_DEFAULT)
    for k, v in fixed.items():
        p[FIELDS.index(k)] = v
    p[FIELDS.index(field)] = value
    return p


def fold(seq, params, dangles, pen):
    return OracleFold(seq, blob(params), dangles, 0, threads=0 if len(seq) > 40 else None, pen=pen)


def low(seq, params, dangles, pen):
    o = fold(seq, params, dangles, pen)
    try:
        return o.low_stores()
    finally:
        o.close()


def bisect(seq, params, dangles, fixed, field, inside, outside):
    assert low(seq, params, dangles, pen_of(fixed, field, inside)) == 0, (field, inside, "is not inside")
    assert low(seq, params, dangles, pen_of(fixed, field, outside)) > 0, (field, outside, "is not outside")
    while abs(inside - outside) > 1:
        mid = (inside + outside) // 2
        if low(seq, params, dangles, pen_of(fixed, field, mid)) == 0:
            inside = mid
        else:
            outside = mid
    return inside, outside


def describe(name, seq, params, dangles, fixed, field, inside, outside):
    n = len(seq)
    v_in, v_out = bisect(seq, params, dangles, fixed, field, inside, outside)
    pen_in, pen_out = pen_of(fixed, field, v_in), pen_of(fixed, field, v_out)
    oi, oo = fold(seq, params, dangles, pen_in), fold(seq, params, dangles, pen_out)
    try:
        low_in, low_out = oi.low_stores(), oo.low_stores()
        assert low_in == 0 and low_out > 0
        lowest = {c: None for c in CLASSES}
        wrapped = {}
        cls_of = {HASH_NAMES.index(m): c for c, ms in CLASSES.items() for m in ms}
        for cell in valid_cells(n):
            for x in range(22):
                v = oi.get4(x, *cell)
                c = cls_of[x]
                if lowest[c] is None or v < lowest[c][0]:
                    lowest[c] = [v, HASH_NAMES[x], list(cell)]
                if v <= -32768 + 100 and oo.get4(x, *cell) >= 32767 - 100:
                    w = wrapped.setdefault(HASH_NAMES[x], [0, list(cell)])
                    w[0] += 1
    finally:
        oi.close()
        oo.close()
    inside_prefixes = [m for m in range(n - 1, max(n - 9, 7), -1) if low(seq[:m], params, dangles, pen_out) == 0]
    rec = {"name": name, "seq": seq, "params": params, "dangles": dangles, "field": field, "pen_in": pen_in,
           "pen_out": pen_out, "low_in": low_in, "low_out": low_out, "split_target": TARGETS.get(name, 0),
           "lowest": lowest, "wrapped": wrapped, "inside_prefixes": inside_prefixes}
    print(name, field, v_in, v_out, "low_out", low_out, {c: v[:2] for c, v in lowest.items()}, wrapped, inside_prefixes,
          flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "tests", "golden", "range_cases.json"))
    a = ap.parse_args()
    cases = [describe(*c) for c in CASES]
    tried, found = [], []
    for c in CF_SEARCH:
        r = describe(*c)
        first_cf = bool(r["wrapped"]) and all(m in CLASSES["IN_CF"] for m in r["wrapped"])
        tried.append({"name": r["name"], "field": r["field"], "pen_out": r["pen_out"], "wrapped": sorted(r["wrapped"]),
                      "closed_form_first": first_cf})
        if first_cf:
            found.append(r)
    cases += found[:1]
    doc = {"comment": "Folds at the edge of the domain of bit-identity; written by tools/gen_range_cases.py (see its "
                      "docstring for the fields).  pen_in / pen_out differ by one unit of `field`.",
           "closed_form_first_search": {"tried": tried, "found": [r["name"] for r in found[:1]],
                                        "note": "a fold counts when every wrapped store at pen_out is in a PM / PO "
                                                "multiloop matrix (none in the PL / PR tables or a d4 / record matrix)"},
           "cases": cases}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
