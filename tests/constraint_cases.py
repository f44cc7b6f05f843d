"""Shared by the constrained-folding tests (CPU and GPU): the committed fixtures
(tests/golden/constraint_cases.json, written by tools/gen_constraint_cases.py), their constraints as
ccj_amd.Constraint objects, and small helpers on structures.  No tests here."""
import ccj_amd
from tests.oracle_lib import golden

OPEN, CLOSE = "([{<", ")]}>"
_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = golden("constraint_cases.json")
    return _cases


def case_id(c):
    return "n%d_%s_d%d%s_%s" % (len(c["seq"]), c["params"], c["dangles"], "_noGU" if c["noGU"] else "", c["kind"])


def constraint_of(c):
    return ccj_amd.Constraint(c["unpaired"], [tuple(p) for p in c["forbid"]],
                              None if c["allow_only"] is None else [tuple(p) for p in c["allow_only"]])


def pairs_of(structure):
    """{(i, j)} of a dot-bracket string, 1-based, i < j."""
    stacks, out = {k: [] for k in range(len(OPEN))}, set()
    for p, ch in enumerate(structure, 1):
        if ch in OPEN:
            stacks[OPEN.index(ch)].append(p)
        elif ch in CLOSE:
            out.add((stacks[CLOSE.index(ch)].pop(), p))
    return out


def gu_pairs(seq):
    """Every G-U position pair of the sequence."""
    n = len(seq)
    return [(i, j) for i in range(1, n + 1) for j in range(i + 1, n + 1) if {seq[i - 1], seq[j - 1]} == {"G", "U"}]


def pseudoknotted_e2e(nmax):
    """The folds of e2e.json whose reference structure has a pseudoknot, n <= nmax:
    (case, structure, energy text)."""
    out = []
    for c in golden("e2e.json"):
        lines = c["stdout"].splitlines()
        if c["rc"] != 0 or not lines or len(c["seq"]) > nmax:
            continue
        st, en = lines[-1].split()
        if any(ch in st for ch in "[{<"):
            out.append((c, st, en))
    return out
