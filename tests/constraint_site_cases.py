"""Shared by the constraint-site tests (CPU and GPU): the committed fixtures
(tests/golden/constraint_site_cases.json, written by tools/gen_constraint_site_cases.py).  Every
case is a constrained fold with the 31 hashes and W(n) of the masked restatement, and names in
`pins` the sites (tests/masked_oracle.py SITES) whose omission changes it.  No tests here."""
from tests.oracle_lib import golden

_file = None


def site_file():
    global _file
    if _file is None:
        _file = golden("constraint_site_cases.json")
    return _file


def cases():
    return site_file()["cases"]


UNOBSERVED = site_file()["unobserved"]
OBSERVED = [s for s in site_file()["sites"] if s not in UNOBSERVED]


def case_id(c):
    return "n%d_%s_d%d_%s_%d" % (len(c["seq"]), c["params"], c["dangles"], c["kind"], cases().index(c))


def one_case_per_site():
    """The first case of every observed site (a case may stand for several)."""
    out = []
    for s in OBSERVED:
        c = next(c for c in cases() if s in c["pins"])
        if c not in out:
            out.append(c)
    return out
