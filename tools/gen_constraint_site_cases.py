"""Write tests/golden/constraint_site_cases.json: for every reader of the pair table in the fill
(the sites of tests/masked_oracle.py), small constrained folds that notice when that one reader
ignores the constraint.  CPU only, seeded, regenerated bit for bit:

    python tools/gen_constraint_site_cases.py                # the fixtures (about a minute)
    python tools/gen_constraint_site_cases.py --unobserved N # N folds per unobserved site, counts on stdout

A candidate is a constrained fold; a site notices it when its omission variant (the masked
restatement with that one reader left on the bare table) gives other matrices than the full mask.
Candidates come, in this order, from the pseudoknotted folds of tests/golden/e2e.json under the
constraint kinds of tools/gen_constraint_cases.py, from seeded random folds (n 12-30, smallest
first), and from directed constructions (a multiloop-closing or otherwise stored pair forbidden, `x`
beside a stem end).  The search for a site ends once it has a candidate that changes W(n) itself and
two that differ in parameter set or constraint kind and reach beyond WM/WMv, or a hundred of any sort (the
sites whose omission only revalues the V left at a forbidden pair rarely move W(n)); it keeps, per site,
the two best: W(n) changed, then a difference beyond WM/WMv, then a case already kept, then small n.

The sites in UNOBSERVED get no fixture.  That is a condition of the recurrences (the argument stands
beside each name and in DESIGN.md §1), not a measurement; --unobserved runs the search that found
nothing (profiles/constraint_sites.txt).

The file ends with the folds of TRACEBACK, which pin no site but the traceback's own check.

Every case also carries W(n) of the strict variant (no V stored at a forbidden pair), asserted
equal to the masked W(n): no structure of these folds can hold a forbidden pair.
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_constraint_cases as base  # noqa: E402
from tests.masked_oracle import (MAY_BE_UNOBSERVED, SITES, MaskedFold, OmittedFold, StrictFold,  # noqa: E402
                                 build_variants, fold_case as fold)
from tests.oracle_lib import HASH_NAMES, blob, golden  # noqa: E402

SEED = 20261021
N_RANDOM = 300
PER_SITE = 2
MAX_HITS = 100
PARAMS = ["Turner04", "DirksPierce09", "DNA_Mathews2004", "CaoChen09"]
E2E_KINDS = ["x_in_helix", "x_in_pk_helix", "forbid_mid_pair", "forbid_mid_pk_pair", "forbid_pk_helix", "mix"]

_OUTER = ("get_P%siloop is called only under `if (ptype(o, %s) > 0)` of compute_cell, a masked reader of the same "
          "pair: where the mask decides, the call is not reached")
_INNER = ("the candidate adds get4(%s, d, dp, ..) of a masked (d, dp), which the guard `ptype > 0` of the %s store never "
          "lets be written: it reads as 32767, and the memoised loop energy of a masked inner pair (type 0: no stack, "
          "no 1x1, 2x1 or 2x2 entry) is never negative, so the sum is stored as 32767, the value an unwritten cell holds")
_EXT = ("the term adds V of a masked pair, which holds a value only through an interior-loop or multiloop branch with "
        "pair type 0: the inner structure plus a closing cost that is positive at these lengths (Turner04 needs ten "
        "branches for a multiloop to cost less than nothing), while W can take the same inner stems as exterior stems "
        "at no such cost; the term never wins the minimum, whatever pair type its exterior-stem energy is given")
UNOBSERVED = {
    "get_PLiloop.ij": _OUTER % ("L", "i, j"),
    "get_PRiloop.kl": _OUTER % ("R", "k, l"),
    "get_PMiloop.jk": _OUTER % ("M", "j, k"),
    "get_POiloop.il": _OUTER % ("O", "i, l"),
    "get_PLiloop.ddp": _INNER % ("PL", "PL"),
    "get_PRiloop.ddp": _INNER % ("PR", "PR"),
    "get_PMiloop.ddp": _INNER % ("PM", "PM"),
    "get_POiloop.ddp": _INNER % ("PO", "PO"),
    "get_PfromMdoubleprime.il": "dead: its only caller (PfromMprime) passes k = d < l, so `i == j && k == l` never holds",
    "E_ext_Stem.ij": _EXT,
    "E_ext_Stem.i1j": _EXT,
    "E_ext_Stem.ij1": _EXT,
    "E_ext_Stem.i1j1": _EXT,
}
assert set(UNOBSERVED) <= MAY_BE_UNOBSERVED
# Folds for the traceback's own constraint check (ccj_backtrack.hip DevStore::pr).  The traceback
# reads matrices that carry the constraint already, so no site's omission stands for that check; an
# engine build without it was searched on the GPU (random and directed candidates as below) for folds
# whose device structure differs from the host's, and these are four of the eight found among 4,043:
# the unchecked traceback pairs a forbidden position at an interior-loop node.  They pin no site.
TRACEBACK = [
    ("GUCCCCCGCCAUGCGGGGCGC", "DirksPierce09", 2, "....x................", []),
    ("GAGCUGCGGGCACCCUUGUCCGGCC", "CaoChen09", 1, "....x....................", []),
    ("GGGCUGUGUCGGCUGACCGCGGCGA", "DirksPierce09", 1, "......x..................", [(5, 20), (7, 11), (7, 19), (12, 15), (15, 23)]),
    ("GGCGGCCCUACUGGGAGUGGGCGGCCGGC", "DirksPierce09", 0, "........................x....", []),
]
OBSERVED = [s for s in SITES if s not in UNOBSERVED]


def _case(seq, params, dangles, noGU, kind, unpaired=None, forbid=(), allow_only=None):
    return dict(seq=seq, params=params, dangles=dangles, noGU=noGU, kind=kind, unpaired=unpaired,
                forbid=[list(p) for p in forbid], allow_only=allow_only)


def from_e2e():
    seen = set()
    todo = sorted((len(c["seq"]), c["seq"], c["params"], c["dangles"], int(bool(c["noGU"])), c["stdout"].splitlines()[-1].split()[0])
                  for c in golden("e2e.json")
                  if c["rc"] == 0 and len(c["seq"]) <= 30 and any(ch in c["stdout"].splitlines()[-1].split()[0] for ch in "[{<"))
    for n, seq, params, dangles, noGU, st in todo:
        if (seq, params, dangles, noGU) in seen:
            continue
        seen.add((seq, params, dangles, noGU))
        for kind in E2E_KINDS:
            try:
                cons = base.make(kind, n, st)
            except ValueError:  # no helix of that sort in this structure
                continue
            yield _case(seq, params, dangles, noGU, "e2e_" + kind, **cons)


def random_case(rng, kind="random"):
    n = rng.randint(12, 30)
    seq = "".join(rng.choice("GGCCAU") for _ in range(n))
    dangles = rng.choice([1, 1, 0, 2])
    params = rng.choice(PARAMS)
    if params.startswith("DNA"):
        seq = seq.replace("U", "T")
    forbid = sorted({tuple(sorted(rng.sample(range(1, n + 1), 2))) for _ in range(rng.randint(1, 6))})
    unpaired = "".join("x" if rng.random() < 0.08 else "." for _ in range(n))
    return _case(seq, params, dangles, 0, kind, unpaired if "x" in unpaired else None, forbid)


def from_random(count=N_RANDOM, seed=SEED):
    rng = random.Random(seed)
    return sorted((random_case(rng) for _ in range(count)), key=lambda c: len(c["seq"]))


def stored_pairs(c):
    """(i, j, how V(i, j) was won) of every pair with V < 0 in the unconstrained fold."""
    n = len(c["seq"])
    m = MaskedFold(c["seq"], blob(c["params"]), c["dangles"], c["noGU"])
    try:
        return [(i, j, chr(m.get2(4, i, j))) for i in range(1, n + 1) for j in range(i + 4, n + 1) if m.get2(3, i, j) < 0]
    finally:
        m.close()


def from_directed(count, seed=SEED + 1):
    """Helix-rich random sequences whose unconstrained fold shows where a constraint bites: every
    multiloop-closed pair forbidden at once; one stored pair forbidden; `x` on the base before or
    after a stored pair, so that (i+1, j), (i, j-1), (i+1, j-1) of the enclosing positions is forbidden
    while the pair itself stands."""
    rng = random.Random(seed)
    done = 0
    while done < count:
        c = random_case(rng)
        n = len(c["seq"])
        c.update(unpaired=None, forbid=[])
        prs = stored_pairs(c)
        if not prs:
            continue
        closed = [(i, j) for i, j, t in prs if t == "M"]
        i, j, _ = prs[rng.randrange(len(prs))]
        out = [dict(c, kind="directed_forbid_stored_pair", forbid=[[i, j]])]
        if closed:
            out.append(dict(c, kind="directed_forbid_mloop_closers", forbid=[list(p) for p in closed]))
            a, b = closed[rng.randrange(len(closed))]
            out.append(dict(c, kind="directed_forbid_mloop_closer", forbid=[[a, b]]))
        for p in {i - 1, j + 1} & set(range(1, n + 1)):
            out.append(dict(c, kind="directed_x_beside_stem", unpaired="".join("x" if q == p else "." for q in range(1, n + 1))))
        for x in out[:count - done]:
            done += 1
            yield x


def search(sites, candidates, per_site=PER_SITE, max_hits=MAX_HITS):
    """(hits, compared): hits[site] = [(candidate index, case, full fold, differing matrices, omitted
    W(n))], compared[site] = the candidates whose full-mask fold was held against that site's omission.
    A site leaves the search once it holds a hit that changes W(n) and per_site hits that differ in
    params or kind and reach beyond WM/WMv, or max_hits hits of any sort.  A candidate outside the
    domain of bit-identity (low stores) is compared with nothing."""
    hits = {s: [] for s in sites}
    compared = {s: 0 for s in sites}
    want = set(sites)

    def done(hs):
        good = [h for h in hs if h[4] != h[2][1] or not set(h[3]) <= {"WM", "WMv"}]
        return (any(h[4] != h[2][1] for h in hs) and len({(h[1]["params"], h[1]["kind"]) for h in good}) >= per_site) \
            or len(hs) >= max_hits

    for x, c in enumerate(candidates):
        if not want:
            break
        full = fold(MaskedFold, c)
        if full[2] != 0:
            continue
        for s in sorted(want, key=SITES.index):
            h, w, low = fold(OmittedFold, c, s)
            compared[s] += 1
            bad = [k for k in HASH_NAMES if h[k] != full[0][k]]
            if bad:
                hits[s].append((x, c, full, bad, w))
                if done(hits[s]):
                    want.discard(s)
    return hits, compared


def choose(hits, per_site=PER_SITE):
    """{candidate index: (case, full fold, {site: (matrices, omitted W(n))})}"""
    kept = {}
    for s in [s for s in SITES if s in hits]:
        taken = []
        for _ in range(per_site):
            pool = [h for h in hits[s] if h[0] not in [t[0] for t in taken]]
            other = [h for h in pool if all((h[1]["params"], h[1]["kind"]) != (t[1]["params"], t[1]["kind"]) for t in taken)]
            pool = other or pool
            if not pool:
                break
            taken.append(min(pool, key=lambda h: (h[4] == h[2][1], set(h[3]) <= {"WM", "WMv"}, h[0] not in kept,
                                                  len(h[1]["seq"]), h[0])))
            x, c, full, bad, w = taken[-1]
            kept.setdefault(x, (c, full, {}))[2][s] = (bad, w)
    return kept


def candidates():
    yield from from_e2e()
    yield from from_random()
    yield from from_directed(300)


def generate():
    build_variants(OBSERVED, strict=True)
    kept = choose(search(OBSERVED, candidates())[0])
    cases = []
    for x in sorted(kept):
        c, (hashes, Wn, low), pins = kept[x]
        _, strict_Wn, _ = fold(StrictFold, c)
        assert low == 0
        assert strict_Wn == Wn, ("a forbidden pair lowers W(n)", c, Wn, strict_Wn)
        cases.append(dict(c, pins={s: dict(differs=bad, Wn=w) for s, (bad, w) in pins.items()},
                          hashes=hashes, Wn=Wn, low_stores=low, strict_Wn=strict_Wn))
    for seq, params, dangles, unpaired, forbid in TRACEBACK:
        c = _case(seq, params, dangles, 0, "traceback_x" if not forbid else "traceback_mix", unpaired, forbid)
        hashes, Wn, low = fold(MaskedFold, c)
        _, strict_Wn, _ = fold(StrictFold, c)
        assert low == 0 and strict_Wn == Wn and Wn < 0, (c, Wn, strict_Wn, low)
        cases.append(dict(c, pins={}, hashes=hashes, Wn=Wn, low_stores=low, strict_Wn=strict_Wn))
    return dict(sites=SITES, unobserved=UNOBSERVED, cases=cases)


def _count(args):
    """One share of the --unobserved search: per site, the folds compared and those it noticed."""
    sites, kind, count, seed = args
    rng = random.Random(seed)
    cands = from_directed(count, seed) if kind == "directed" else (random_case(rng) for _ in range(count))
    hits, compared = search(sites, cands, per_site=10 ** 9, max_hits=10 ** 9)
    return kind, compared, {s: len(h) for s, h in hits.items()}


def search_unobserved(total, procs=8):
    import multiprocessing
    sites = sorted(UNOBSERVED, key=SITES.index)
    build_variants(sites)
    share = -(-total // (2 * procs))
    jobs = [(sites, kind, share, SEED + 100 + 2 * p + (kind == "directed")) for p in range(procs) for kind in ("random", "directed")]
    with multiprocessing.get_context("fork").Pool(procs) as pool:
        out = pool.map(_count, jobs, chunksize=1)
    print("search for a fold that an unobserved site notices (n 12-30, seeds %d..%d); folds compared" % (SEED + 100, SEED + 99 + 2 * procs))
    print("%-26s %8s %8s %8s" % ("site", "random", "directed", "noticed"))
    for s in sites:
        r = sum(n[s] for k, n, _ in out if k == "random")
        d = sum(n[s] for k, n, _ in out if k == "directed")
        print("%-26s %8d %8d %8d" % (s, r, d, sum(h[s] for _, _, h in out)))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--unobserved":
        search_unobserved(int(sys.argv[2]))
        sys.exit(0)
    out = generate()
    with open(os.path.join(ROOT, "tests", "golden", "constraint_site_cases.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for c in out["cases"]:
        print(len(c["seq"]), c["params"], c["dangles"], c["kind"], c["Wn"],
              {s: (p["Wn"], p["differs"][:4]) for s, p in c["pins"].items()})
    for s in OBSERVED:
        print(s, sum(s in c["pins"] for c in out["cases"]))
