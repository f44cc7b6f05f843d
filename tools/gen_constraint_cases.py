"""Write tests/golden/constraint_cases.json: constrained folds with the hashes of the masked
restatement (tests/masked_oracle.py).  CPU only, a few seconds:

    python tools/gen_constraint_cases.py

Every case takes a pseudoknotted fold of tests/golden/e2e.json (sequence, parameter set, dangles,
noGU and the reference's MFE structure) and puts one constraint on it, derived from that structure by
the rules below, so the file can be regenerated bit for bit.  Each case carries the constraint, the
31 hashes and W(n) of the masked restatement, and is asserted to have low_stores() == 0 (inside the
domain of bit-identity).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.masked_oracle import MaskedFold  # noqa: E402
from tests.oracle_lib import blob, golden  # noqa: E402

OPEN, CLOSE = "([{<", ")]}>"


def pairs_of(structure):
    """[(i, j, bracket kind)] of a dot-bracket string, 1-based, sorted by i."""
    stacks, out = {k: [] for k in range(len(OPEN))}, []
    for p, ch in enumerate(structure, 1):
        if ch in OPEN:
            stacks[OPEN.index(ch)].append(p)
        elif ch in CLOSE:
            k = CLOSE.index(ch)
            out.append((stacks[k].pop(), p, k))
    return sorted(out)


def helices(structure):
    """Maximal runs (i, j), (i+1, j-1), ... of one bracket kind, each a list of pairs."""
    prs = pairs_of(structure)
    have = {(i, j): k for i, j, k in prs}
    out = []
    for i, j, k in prs:
        if have.get((i - 1, j + 1)) == k:
            continue
        h = []
        while have.get((i, j)) == k:
            h.append((i, j))
            i, j = i + 1, j - 1
        out.append((k, h))
    return out


def longest(structure, kind):
    hs = [h for k, h in helices(structure) if (k > 0) == (kind == "pk")]
    return max(hs, key=len)


def unpaired_string(n, positions):
    return "".join("x" if p in positions else "." for p in range(1, n + 1))


# kind -> constraint of a fold with MFE structure st
def make(kind, n, st):
    if kind == "x_in_helix":          # the 5' base of the middle pair of the longest nested helix
        h = longest(st, "nested")
        return dict(unpaired=unpaired_string(n, {h[len(h) // 2][0]}))
    if kind == "x_in_pk_helix":       # the 3' base of the middle pair of the longest pseudoknot helix
        h = longest(st, "pk")
        return dict(unpaired=unpaired_string(n, {h[len(h) // 2][1]}))
    if kind == "forbid_mid_pair":     # the middle pair of the longest nested helix
        h = longest(st, "nested")
        return dict(forbid=[list(h[len(h) // 2])])
    if kind == "forbid_mid_pk_pair":
        h = longest(st, "pk")
        return dict(forbid=[list(h[len(h) // 2])])
    if kind == "forbid_pk_helix":     # every pair of the longest pseudoknot helix
        return dict(forbid=[list(p) for p in longest(st, "pk")])
    if kind == "allow_only_mfe":
        return dict(allow_only=[[i, j] for i, j, _ in pairs_of(st)])
    if kind == "mix":                 # x in the nested helix and one pseudoknot pair forbidden
        h, g = longest(st, "nested"), longest(st, "pk")
        return dict(unpaired=unpaired_string(n, {h[0][0], h[-1][1]}), forbid=[list(g[len(g) // 2])])
    if kind == "x_everywhere":
        return dict(unpaired="x" * n)
    raise ValueError(kind)


# (sequence, params, dangles, noGU) of the e2e fold, constraint kind
CASES = [
    ("GCGGAUUUAGCUCAGUUGGGAGAGCGCCAGAC", "Turner04", 2, 0, "x_in_helix"),
    ("UCCCGUCAUACCAUACCGUGAUGAAUAAUGC", "Turner04", 0, 0, "forbid_mid_pair"),
    ("GCGGAUUUAGCUCAGUUGGGAGAGCGCCAGAC", "Turner04", 1, 0, "forbid_pk_helix"),
    ("ACUAUAGUGGUCGAGGUAUGGAGAGCAGUGCGUU", "DirksPierce09", 0, 0, "allow_only_mfe"),
    ("CGGUGGUAACCUUGAGCCUC", "DirksPierce03", 1, 0, "mix"),
    ("ACCAACGUUCUGAAGGCUGAUGCAUG", "DirksPierce03", 0, 0, "x_everywhere"),
    ("GCGGATTTAGCTCAGTTGGGAGAGCGCCAGAC", "DNA_Mathews2004", 2, 1, "forbid_pk_helix"),
    ("GCAACGAUGACAUACAUCGCUAGUCGACGC", "Turner04", 2, 0, "x_in_pk_helix"),
    ("CUGCUAAGGUCGCUUCAGAUACUUACCGUGCUCAGG", "Turner04", 0, 0, "forbid_mid_pk_pair"),
    ("GGGGGGAAGGGGGGGGAACCCCCCACCCCCCCC", "DirksPierce09", 1, 0, "mix"),
    ("CGCAAGUCCUGCCAGAUCACACGGCGUGUGUUAUC", "DirksPierce03", 0, 0, "allow_only_mfe"),
    ("ACUUAGAACUUGAAGGGCGGUCCUGACUGC", "CaoChen09", 1, 1, "forbid_pk_helix"),
    ("GGCUGGGGGCCAGUAGGUGCUCUUCCCGUU", "Turner04", 2, 0, "mix"),
]


def generate():
    e2e = golden("e2e.json")
    out = []
    for seq, params, dangles, noGU, kind in CASES:
        ref = next(c for c in e2e if c["seq"] == seq and c["params"] == params and c["dangles"] == dangles
                   and int(bool(c["noGU"])) == noGU and c["rc"] == 0)
        st = ref["stdout"].splitlines()[-1].split()[0]
        n = len(seq)
        assert len(st) == n and any(ch in st for ch in "[{<"), (seq, st)
        cons = dict(unpaired=None, forbid=[], allow_only=None)
        cons.update(make(kind, n, st))
        m = MaskedFold(seq, blob(params), dangles, noGU, **cons)
        try:
            assert m.low_stores() == 0, (seq, kind, m.low_stores())
            out.append(dict(seq=seq, params=params, dangles=dangles, noGU=noGU, kind=kind, mfe_structure=st, **cons,
                            hashes=m.hashes(), Wn=m.W(n)))
        finally:
            m.close()
    return out


if __name__ == "__main__":
    cases = generate()
    path = os.path.join(ROOT, "tests", "golden", "constraint_cases.json")
    with open(path, "w") as f:
        json.dump(cases, f, indent=1)
        f.write("\n")
    for c in cases:
        print(len(c["seq"]), c["params"], c["dangles"], c["noGU"], c["kind"], c["Wn"])
