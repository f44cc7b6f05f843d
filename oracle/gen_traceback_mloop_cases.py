#!/usr/bin/env python3
"""oracle/gen_traceback_mloop_cases.py — TEST INFRASTRUCTURE: tests/golden/traceback_mloop_cases.json.

The sibling of oracle/gen_traceback_cases.py for the traceback nodes that one never reached: the 16
P_P{L,R,M,O}mloop / ...mloop00 / ...mloop01 / ...mloop10 cases of pseudo_loop::backtrack, P_WB and
P_WBP (which only those nodes push) and the multiloop sub-case of P_PL / P_PR / P_PM / P_PO.  The
families' seed is 32767 + bp, so they become the minimum of PL / PR / PM / PO only when bp is
strongly negative: a sign change that the other generator's penalty range (same sign, within 10x)
excludes.  It does not touch traceback_cases.json.

    make -C oracle ref cov oracle && python3 oracle/gen_traceback_mloop_cases.py

reproduces the committed fixture byte for byte (everything is seeded; the number of jobs changes
nothing).

  1. candidates: random folds with bp in -33000 .. -5000 (two of three in -12500 .. -5000, where folds
     inside the int16 range are found), half of them with ap, cp, PSM and PPS varied
     too (ap -16500 .. -100, cp -100 .. 12, PSM / PPS negative); n 18 .. 34, five alphabets, Turner04 /
     DirksPierce09, dangles 0 / 1 / 2.  A second band at n = 57 .. 64 (the keys of
     tests/schedule_rows.ALL_REGIME_TARGET from 57 on: there a fold can be run in every launch regime of
     the level chain) with bp in -6000 .. -3000;
  2. each runs through the coverage build of the reference (gen_traceback_cases.run_candidate); one the
     reference ends with a signal, or that hits the time limit, is dropped;
  3. each is folded by the C restatement with the same penalties, and dropped unless
     OracleFold.low_stores() == 0: below -32768 the reference's int16 store (matrices.hh:188-191)
     wraps, the engine does not follow, and a difference there would mean nothing;
  4. a greedy set cover over executed lines of the two backtrack functions, over the admitted
     candidates only (ties: the shorter sequence, then the earlier candidate); then band folds are
     added until two of them are kept that enter multiloop-family labels of two families;
  5. the kept folds are re-run through the plain reference driver (fold and hash) and written out;
  6. `unreached`: every multiloop-family id of the static parse that no admitted candidate enters, with
     its reason (entered only by candidates outside the int16 range, or by none at all).

Only recorded data is written; no gcov output is kept (the work directory is removed).
"""
import argparse
import concurrent.futures as cf
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import gen_traceback_cases as G  # noqa: E402
from tests.oracle_lib import HASH_NAMES, OracleFold, blob  # noqa: E402

OUT = os.path.join(G.GOLDEN, "traceback_mloop_cases.json")
IX = {k: x for x, k in enumerate(G.PEN_NAMES)}
FAMILIES = ("PL", "PR", "PM", "PO")
BAND_N = list(range(57, 65))
OUT_OF_RANGE = "entered only by folds outside the int16 range"


def family_of(i):
    """'PL' / 'PR' / 'PM' / 'PO' for an id of that family's four multiloop labels, else None."""
    base = i.split("@")[0]
    return base[2:4] if base.startswith("P_P") and "mloop" in base else None


def family_ids():
    """The multiloop-family ids of the static parse: every label and sub-branch whose label holds
    `mloop` or begins with P_WB, and the sub-case of P_PL / P_PR / P_PM / P_PO that pushes P_P?mloop."""
    first, last, labels, subs = G.STRUCT["pseudo_loop.cc"]
    with open(os.path.join(G.REFSRC, "pseudo_loop.cc")) as f:
        src = f.read().split("\n")
    ids = [i for i in list(labels) + list(subs) if "mloop" in i.split("@")[0] or i.startswith("P_WB")]
    parents = []
    for fam in FAMILIES:
        own = sorted((k, i) for i, k in subs.items() if i.split("@")[0] == "P_" + fam)
        hit = [i for x, (k, i) in enumerate(own)
               if any(f"P_{fam}mloop)" in s for s in src[k - 1:(own[x + 1][0] if x + 1 < len(own) else labels["P_" + fam][1]) - 1])]
        assert len(hit) == 1, (fam, hit)
        parents += hit
    return ids + parents, parents


def candidates(n_small, n_band):
    c = []
    r = random.Random(20261020)

    def add(seq, params, dangles, pen, source):
        c.append({"seq": seq, "params": params, "dangles": dangles, "noGU": 0, "pen": pen, "source": source})

    for k in range(n_small):
        pen = list(G.PEN_DEFAULT)
        # beyond about -12500 nearly every fold leaves the int16 range: two of three stay above it
        pen[IX["bp"]] = -r.randint(5000, 12500 if k % 3 else 33000)
        what = "bp"
        if k % 2:
            pen[IX["ap"]] = -r.randint(100, 16500)
            pen[IX["cp"]] = r.choice([-100, -30, -10, -3, 2, 12])
            what += " ap cp"
            if k % 4 == 3:
                pen[IX["PSM"]] = -r.choice([100, 200, 1000])
                pen[IX["PPS"]] = -r.choice([10, 30, 96])
                what += " PSM PPS"
        alpha = G.ALPHABETS[k % 5]
        add(G.rseq(r, r.randint(18, 34), alpha), ("Turner04", "DirksPierce09")[(k // 5) % 2], r.choice([0, 1, 2]), pen,
            f"mloop #{k}: alphabet {alpha}, changed {what}")
    for k in range(n_band):
        pen = list(G.PEN_DEFAULT)
        pen[IX["bp"]] = -r.randint(3000, 6000)
        alpha = G.ALPHABETS[k % 5]
        add(G.rseq(r, BAND_N[k % len(BAND_N)], alpha), ("Turner04", "DirksPierce09")[(k // 5) % 2], r.choice([0, 1, 2]), pen,
            f"mloop band #{k}: alphabet {alpha}, changed bp")
    return c


def low_stores(c):
    o = OracleFold(c["seq"], blob(c["params"]), c["dangles"], c["noGU"], pen=c["pen"])
    try:
        return o.low_stores()
    finally:
        o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--small", type=int, default=720)
    ap.add_argument("--band", type=int, default=48)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    for p in (G.COVDRV, G.DRV):
        if not os.path.exists(p):
            sys.exit(f"{p} missing: make -C oracle ref cov oracle")
    cands = candidates(a.small, a.band)
    ids, parents = family_ids()
    work = tempfile.mkdtemp(prefix="ccj_tbmloop_")
    results = [None] * len(cands)
    try:
        with cf.ThreadPoolExecutor(a.jobs) as ex:
            for idx, res in ex.map(G.run_candidate, [(k, c, work, a.timeout) for k, c in enumerate(cands)]):
                results[idx] = res
            low = list(ex.map(low_stores, cands))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    timed_out = [k for k, r in enumerate(results) if r is None]
    killed = [k for k, r in enumerate(results) if r is not None and r["rc"] < 0]
    ran = [k for k, r in enumerate(results) if r is not None and r["rc"] >= 0 and r["lines"]]
    outside = [k for k in ran if low[k] != 0]
    live = [k for k in ran if low[k] == 0]
    ent = {k: G.entered_ids(results[k]) for k in ran}

    def lineset(k):
        return {(f, ln) for f in G.FUNCS for ln in results[k]["lines"].get(f, [])}

    covered, keep = set(), []
    sets = {k: lineset(k) for k in live}
    while True:
        best, gain = None, 0
        for k in live:
            g = len(sets[k] - covered)
            if g > gain or (g == gain and g > 0 and best is not None and len(cands[k]["seq"]) < len(cands[best]["seq"])):
                best, gain = k, g
        if best is None or gain == 0:
            break
        keep.append(best)
        covered |= sets[best]

    # the launch-regime band: two kept folds with n in BAND_N, labels of two families between them
    def fams(k):
        return {family_of(i) for i in ent[k]} - {None}

    def band_state():
        kept = [k for k in keep if len(cands[k]["seq"]) in BAND_N and fams(k)]
        return len(kept), set().union(*[fams(k) for k in kept]) if kept else set()

    band = sorted((k for k in live if len(cands[k]["seq"]) in BAND_N and fams(k)),
                  key=lambda k: (-len(fams(k)), -len(sets[k]), k))
    while True:
        cnt, have = band_state()
        if cnt >= 2 and len(have) >= 2:
            break
        more = [k for k in band if k not in keep]
        assert more, "no admitted band fold left"
        keep.append(max(more, key=lambda k: (len(fams(k) - have), -band.index(k))))
    keep.sort()

    entered = set()
    cases = []
    for k in keep:
        c = cands[k]
        f_ = subprocess.run(G.driver_cmd(G.DRV, "fold", c), capture_output=True, text=True, timeout=a.timeout)
        h_ = subprocess.run(G.driver_cmd(G.DRV, "hash", c), capture_output=True, text=True, timeout=a.timeout)
        assert h_.returncode == 0, (c, h_.stderr)
        assert f_.returncode == results[k]["rc"], (c, f_.returncode, results[k]["rc"])
        h, mfe = G.parse_hashes(h_.stdout)
        assert list(h) == HASH_NAMES
        entered |= set(ent[k])
        cases.append({"seq": c["seq"], "params": c["params"], "dangles": c["dangles"], "noGU": c["noGU"],
                      "pen": c["pen"], "rc": f_.returncode, "stdout": f_.stdout, "stderr": f_.stderr,
                      "hashes": h, "mfe": mfe, "entered": ent[k], "source": c["source"]})
    in_range = set().union(*[set(ent[k]) for k in live])
    assert in_range == entered, sorted(in_range - entered)  # the cover is over lines, ids follow

    n_out = {i: sum(1 for k in outside if i in ent[k]) for i in ids}
    unreached = []
    for i in ids:
        if i in entered:
            continue
        if n_out[i]:
            why = (f"{OUT_OF_RANGE}: {n_out[i]} of the {len(outside)} candidates with 4-D stores below -32768, none "
                   f"of the {len(live)} without")
        else:
            why = f"search budget exhausted: zero hits in {len(ran)} candidate folds, inside or outside the int16 range"
        unreached.append({"id": i, "reason": why})

    doc = {"pen_order": G.PEN_NAMES, "pen_default": G.PEN_DEFAULT,
           "search": {"candidates": len(cands), "small": a.small, "band": a.band, "band_n": BAND_N,
                      "dropped_at_time_limit": len(timed_out), "dropped_killed_by_signal": len(killed),
                      "dropped_outside_int16_range": len(outside), "admitted": len(live),
                      "admitted_entering_family_labels": sum(1 for k in live if fams(k))},
           "ids": ids, "mloop_sub_cases": parents, "cases": cases, "unreached": unreached}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(json.dumps({"search": doc["search"], "cases": len(cases), "n": [len(c["seq"]) for c in cases],
                      "rc": [c["rc"] for c in cases], "unreached": unreached}, indent=1))


if __name__ == "__main__":
    main()
