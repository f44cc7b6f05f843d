#!/usr/bin/env python3
"""oracle/gen_traceback_cases.py — TEST INFRASTRUCTURE: tests/golden/traceback_cases.json.

Searches for a small set of folds that drives the reference's own traceback
(pseudo_loop::backtrack in pseudo_loop.cc, W_final::backtrack in W_final.cc) through as many of
its cases and sub-branches as possible, and records what the reference answers for them.

  1. every candidate fold runs through the coverage-instrumented driver (make -C oracle cov ->
     oracle/_ref/cov/ref_driver) with its own GCOV_PREFIX directory, so its counters are its own;
  2. gcov gives the executed lines of the two backtrack functions; from them: which `case` labels
     of the outer switch were entered, and which sub-branches (the `case N:` labels of the inner
     best_row switches and the "NOT GOOD RESTR INTER" exit), each named LABEL@<reference line>;
  3. a greedy set cover over executed lines keeps the folds whose union covers the most (ties: the
     shorter sequence, then the earlier candidate);
  4. the kept folds are re-run through the plain reference driver (fold and hash) and written out.

Candidates, in this order: the e2e.json corpus (so everything it reaches stays pinned), the n=100
fold of e2e_large.json and the device-vs-host seeds of tests/test_gpu_parity.py up to n=90, random
sequences (n 30-70, six parameter sets, dangles 0/1/2, with and
without noGU, five alphabets), hand-designed sequences, and penalty overrides (each magnitude at
most 10x its default, same sign), last the designed shapes again with pseudoknots made cheap inside
multiloops.  A candidate whose reference run hits the time limit is dropped.
Everything is seeded: two runs give the same file.

Only recorded data is written; no gcov output is kept (the work directory is removed).
"""
import argparse
import concurrent.futures as cf
import json
import os
import random
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFSRC = os.environ.get("REFSRC", "/root/reference/src")
COVDIR = os.path.join(ROOT, "oracle", "_ref", "cov")
COVDRV = os.path.join(COVDIR, "ref_driver")
DRV = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
BLOBDIR = os.path.join(ROOT, "ccj_amd", "params")
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "traceback_cases.json")

PEN_NAMES = ["PS", "PSM", "PSP", "PB", "PUP", "PPS", "a", "b", "c", "ap", "bp", "cp", "e_stP", "e_intP"]
PEN_DEFAULT = [-138, 1007, 1500, 246, 6, 96, 339, 3, 2, 341, 56, 12, 0.89, 0.74]
PARAMS = ["Turner04", "DirksPierce09", "DirksPierce03", "CaoChen06", "CaoChen09", "DNA_Mathews2004"]
ALPHABETS = ["ACGU", "GGCCAU", "GC", "GCU", "GGGCCCAU"]
FUNCS = {"pseudo_loop.cc": "void pseudo_loop::backtrack(", "W_final.cc": "void W_final::backtrack("}


# ---- static structure of the two backtrack functions -------------------------------------------
def parse_function(fname):
    """-> (first, last, labels {name: (from, to)}, subs {id: label line}) for the backtrack
    function of a reference source file: outer `case` labels, inner `case` labels (sub-branches)."""
    with open(os.path.join(REFSRC, fname)) as f:
        src = f.read().split("\n")
    first = next(k for k, s in enumerate(src, 1) if s.startswith(FUNCS[fname]))
    last = next(k for k in range(first + 1, len(src) + 1) if src[k - 1].startswith("}"))
    cases = []  # (line, indent, name)
    for k in range(first, last + 1):
        m = re.match(r"^(\s*)case\s+(\w+)\s*:", src[k - 1])
        if m:
            cases.append((k, len(m.group(1).expandtabs(4)), m.group(2)))
    outer_indent = min(c[1] for c in cases)
    # pseudo_loop.cc indents two of its outer labels (P_PfromMprime, P_PfromMdoubleprime) deeper
    is_outer = lambda c: c[1] == outer_indent or (fname == "pseudo_loop.cc" and c[2].startswith("P_"))
    outer = [c for c in cases if is_outer(c)]
    labels, subs = {}, {}
    for x, (k, _, name) in enumerate(outer):
        end = outer[x + 1][0] - 1 if x + 1 < len(outer) else last
        labels[name] = (k, end)
    if fname == "W_final.cc":  # the P_* labels there only forward to pseudo_loop::backtrack
        labels = {k: v for k, v in labels.items() if not k.startswith("P_")}
    for (k, ind, name) in cases:
        if is_outer((k, ind, name)):
            continue
        own = [n for n, (a, b) in labels.items() if a <= k <= b]
        if own:
            subs[f"{own[0]}@{k}"] = k
    for k in range(first, last + 1):
        if "NOT GOOD RESTR INTER" in src[k - 1]:
            own = [n for n, (a, b) in labels.items() if a <= k <= b]
            subs[f"{own[0]}@{k}"] = k
    return first, last, labels, subs


STRUCT = {f: parse_function(f) for f in FUNCS}


def all_ids():
    ids = []
    for f in FUNCS:
        _, _, labels, subs = STRUCT[f]
        ids += list(labels) + list(subs)
    return ids


# ---- one candidate through the coverage build ---------------------------------------------------
def pen_arg(pen):
    return ",".join(repr(v) for v in pen)


def driver_cmd(drv, mode, c):
    cmd = [drv, mode, "--blob", os.path.join(BLOBDIR, c["params"] + ".ccjp"), "-d", str(c["dangles"])]
    if c["noGU"]:
        cmd.append("--noGU")
    if c["pen"] is not None:
        cmd += ["--pen", pen_arg(c["pen"])]
    return cmd + [c["seq"]]


def gcov_lines(objdir, stem, fname):
    """{line: count} of the reference source fname from <objdir>/<stem>.gcda."""
    shutil.copy(os.path.join(COVDIR, "obj", stem + ".gcno"), objdir)
    r = subprocess.run(["gcov", "-t", stem + ".gcda"], cwd=objdir, capture_output=True, text=True)
    lines, on = {}, False
    for s in r.stdout.split("\n"):
        p = s.split(":", 2)
        if len(p) < 3:
            continue
        cnt, ln = p[0].strip(), p[1].strip()
        if ln == "0":
            if p[2].startswith("Source:"):
                on = p[2].endswith("/" + fname)
            continue
        if on and cnt != "-" and ln.isdigit():
            v = 0 if cnt.startswith(("#", "=")) else int(cnt.rstrip("*"))
            lines[int(ln)] = max(lines.get(int(ln), 0), v)
    return lines


def run_candidate(args):
    idx, c, work, timeout = args
    pre = os.path.join(work, f"c{idx}")
    env = dict(os.environ, GCOV_PREFIX=pre)
    try:
        r = subprocess.run(driver_cmd(COVDRV, "fold", c), capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        shutil.rmtree(pre, ignore_errors=True)
        return idx, None
    objdir = None
    for d, _, files in os.walk(pre):
        if "pseudo_loop.gcda" in files:
            objdir = d
    res = {"rc": r.returncode, "lines": {}, "exec": {}}
    if objdir:  # an abort (assert) leaves no counters: such a fold covers nothing
        for fname, stem in (("pseudo_loop.cc", "pseudo_loop"), ("W_final.cc", "W_final")):
            first, last, _, _ = STRUCT[fname]
            ln = gcov_lines(objdir, stem, fname)
            res["lines"][fname] = sorted(k for k, v in ln.items() if first <= k <= last and v > 0)
            res["exec"][fname] = sorted(k for k in ln if first <= k <= last)
    shutil.rmtree(pre, ignore_errors=True)
    return idx, res


def entered_ids(res):
    out = []
    for fname in FUNCS:
        _, last, labels, subs = STRUCT[fname]
        hit = set(res["lines"].get(fname, []))
        ex = res["exec"].get(fname, [])
        for name, (a, b) in labels.items():
            if any(a <= k <= b for k in hit):
                out.append(name)
        for sid, k in subs.items():
            nxt = next((e for e in ex if e >= k), None)  # a label itself carries no counter
            if nxt is not None and nxt in hit:
                out.append(sid)
    return out


# ---- candidates -----------------------------------------------------------------------------
def rseq(r, n, alphabet):
    return "".join(r.choice(alphabet) for _ in range(n))


def rand_n(r):
    """n in 30..70, most of them below 52 (the reference's cost grows like n^6)."""
    return r.randint(30, 51) if r.random() < 0.75 else r.randint(52, 70)


def helix(r, k):
    a = rseq(r, k, "GC")
    return a, "".join({"G": "C", "C": "G"}[c] for c in reversed(a))


def designed(r):
    """Hand-designed shapes: multiloops closed by a helix (LOOP multiloop sub-cases, M_WM / M_WMv),
    H-type pseudoknots, a pseudoknot nested inside a multiloop (M_WMp), kissing hairpins."""
    out = []
    for rep in range(40):
        h = [helix(r, r.randint(3, 6)) for _ in range(5)]
        u = lambda a, b: rseq(r, r.randint(a, b), "A" if rep % 2 else "AU")
        # three-way junction closed by h0
        out.append(h[0][0] + u(0, 2) + h[1][0] + u(3, 5) + h[1][1] + u(0, 2) + h[2][0] + u(3, 5) + h[2][1] + u(0, 2) + h[0][1])
        # H-type pseudoknot
        out.append(u(0, 2) + h[0][0] + u(1, 3) + h[1][0] + u(1, 3) + h[0][1] + u(2, 5) + h[1][1] + u(0, 2))
        # pseudoknot nested inside a multiloop closed by h2, beside a hairpin h3
        pk = h[0][0] + u(1, 2) + h[1][0] + u(1, 2) + h[0][1] + u(2, 4) + h[1][1]
        out.append(h[2][0] + u(0, 2) + pk + u(0, 2) + h[3][0] + u(3, 4) + h[3][1] + u(0, 2) + h[2][1])
        # kissing hairpins (three interleaved helices)
        out.append(h[0][0] + u(1, 2) + h[1][0] + u(1, 2) + h[0][1] + u(1, 2) + h[2][0] + u(1, 2) + h[1][1] + u(1, 2) + h[2][1])
        # a nested helix inside one arm of a pseudoknot (WP / WPP and WB)
        out.append(h[0][0] + u(0, 1) + h[3][0] + u(3, 4) + h[3][1] + u(0, 1) + h[1][0] + u(1, 2) + h[0][1] + u(1, 3) + h[1][1])
        # a helix that closes nothing but a pseudoknot (LOOP multiloop sub-cases 5-8, M_WMp)
        out.append(h[2][0] + u(0, 3) + pk + u(0, 3) + h[2][1])
    return [s for s in out if 12 <= len(s) <= 70]



def rand_pen(r):
    """Penalty overrides in a sane range: |value| <= 10x the default, same sign; a few named recipes
    (pseudoknots cheap inside multiloops / pseudoloops, band multiloops cheap, scaled e_stP / e_intP)."""
    p = list(PEN_DEFAULT)
    ix = {k: x for x, k in enumerate(PEN_NAMES)}
    kind = r.randrange(8)
    if kind == 0:
        p[ix["PSM"]] = r.choice([101, 150, 300])
    elif kind == 1:
        p[ix["PSP"]] = r.choice([150, 300])
        p[ix["PPS"]] = r.choice([10, 30])
    elif kind == 2:
        p[ix["ap"]], p[ix["bp"]], p[ix["cp"]] = r.choice([35, 100]), r.choice([6, 20]), r.choice([2, 6])
    elif kind == 3:
        p[ix["e_stP"]] = r.choice([0.5, 1.0, 1.5, 2.0, 4.0])
    elif kind == 4:
        p[ix["e_intP"]] = r.choice([0.3, 1.0, 1.5, 3.0])
    elif kind == 5:
        p[ix["e_stP"]], p[ix["e_intP"]] = r.choice([0.6, 1.2, 2.5]), r.choice([0.4, 1.1, 2.2])
        p[ix["PB"]] = r.choice([25, 100, 500])
    elif kind == 6:
        p[ix["PS"]] = r.choice([-1380, -600, -14])
        p[ix["PUP"]], p[ix["PB"]] = r.choice([1, 20, 60]), r.choice([25, 600])
    else:
        for x, d in enumerate(PEN_DEFAULT):
            f = r.choice([0.1, 0.3, 1, 1, 1, 3, 10])
            p[x] = round(d * f, 3) if isinstance(d, float) else int(round(d * f)) or (1 if d > 0 else -1)
    return p


def candidates(n_random, n_pen):
    c = []

    def add(seq, params, dangles, noGU, pen, source):
        c.append({"seq": seq, "params": params, "dangles": dangles, "noGU": int(noGU), "pen": pen, "source": source})

    with open(os.path.join(GOLDEN, "e2e.json")) as f:
        for k, e in enumerate(json.load(f)):
            add(e["seq"], e["params"], e["dangles"], e["noGU"], None, f"corpus: e2e.json #{k}")
    with open(os.path.join(GOLDEN, "e2e_large.json")) as f:
        for k, e in enumerate(json.load(f)):
            if len(e["seq"]) <= 100:
                add(e["seq"], e["params"], e["dangles"], e["noGU"], None, f"corpus: e2e_large.json #{k}")
    # the random device-vs-host folds of tests/test_gpu_parity.py (n <= 90)
    for seed in range(12):
        r = random.Random(7000 + seed)
        n = r.choice([24, 40, 64, 90, 130])
        alpha = r.choice(["ACGU", "GGCCAU", "GCAU"])
        rs = random.Random(9000 + seed)
        s = "".join(rs.choice(alpha) for _ in range(n))
        p = r.choice(["Turner04", "DirksPierce09", "DirksPierce03", "CaoChen09", "Matthews04"])
        d, g = r.choice([0, 1, 2]), r.random() < 0.25
        if n <= 90:
            add(s, p, d, g, None, f"corpus: device-vs-host seed {seed}")
    n_corpus = len(c)
    r = random.Random(20240611)
    for k in range(n_random):
        p = PARAMS[k % 6]
        alpha = ALPHABETS[(k // 6) % 5]
        if p == "DNA_Mathews2004":
            alpha, noGU = alpha.replace("U", "T"), 1  # CCJ.cc:88-90: DNA implies noGU
        else:
            noGU = int(r.random() < 0.3)
        add(rseq(r, rand_n(r), alpha), p, r.choice([0, 1, 2]), noGU, None, f"random #{k}: alphabet {alpha}")
    for k, s in enumerate(designed(r)):
        add(s, PARAMS[k % 5], r.choice([0, 1, 2]), 0, None, f"designed #{k}")
    des = designed(random.Random(77))
    for k in range(n_pen):
        pen = rand_pen(r)
        if k % 4 == 0:
            s = des[(k // 4) % len(des)]
        else:
            s = rseq(r, r.randint(30, 56), ALPHABETS[k % 5])
        add(s, PARAMS[k % 5], r.choice([0, 1, 2]), int(r.random() < 0.2), pen, f"penalty override #{k}")
    # pseudoknots made cheap inside multiloops (a lower PSM, and b with it), every dangle model: the
    # WMp terms of the multiloop, M_WM and M_WMp nodes of W_final::backtrack
    des = designed(random.Random(78))
    ix = {k: x for x, k in enumerate(PEN_NAMES)}
    for k, s in enumerate(des):
        pen = list(PEN_DEFAULT)
        pen[ix["PSM"]] = [101, 200, 400][k % 3]
        if k % 2:
            pen[ix["PS"]] = -600
        for d in (0, 1, 2):
            add(s, PARAMS[(k // 3) % 5], d, 0, pen, f"pseudoknot in multiloop #{k} d{d}")
    return c, n_corpus


# ---- main -----------------------------------------------------------------------------------
def parse_hashes(stdout):
    h, mfe = {}, None
    for line in stdout.splitlines():
        p = line.split()
        if p and p[0] == "HASH":
            h[p[1]] = p[2]
        elif p and p[0] == "MFE":
            mfe = int(p[1])
    return h, mfe


UNREACHED_REASONS_FILE = os.path.join(ROOT, "oracle", "traceback_unreached.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--random", type=int, default=1260)
    ap.add_argument("--pen", type=int, default=800)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--max-n", type=int, default=100, help="drop longer candidates (quick trial runs)")
    a = ap.parse_args()
    for p in (COVDRV, DRV):
        if not os.path.exists(p):
            sys.exit(f"{p} missing: make -C oracle ref cov")
    cands, n_corpus = candidates(a.random, a.pen)
    n_corpus = sum(1 for c in cands[:n_corpus] if len(c["seq"]) <= a.max_n)
    cands = [c for c in cands if len(c["seq"]) <= a.max_n]
    work = tempfile.mkdtemp(prefix="ccj_tbcov_")
    results = [None] * len(cands)
    try:
        with cf.ThreadPoolExecutor(a.jobs) as ex:
            done = 0
            for idx, res in ex.map(run_candidate, [(k, c, work, a.timeout) for k, c in enumerate(cands)]):
                results[idx] = res
                done += 1
                if done % 100 == 0:
                    print(f"{done}/{len(cands)} candidates", file=sys.stderr, flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    dropped = [k for k, r in enumerate(results) if r is None]
    live = [k for k, r in enumerate(results) if r is not None and r["lines"]]

    def lineset(k):
        return {(f, ln) for f in FUNCS for ln in results[k]["lines"].get(f, [])}

    # greedy set cover over executed lines of the two backtrack functions
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
    # the fixture must carry non-default penalties: at least 6 such folds, 2 of them changing
    # e_stP / e_intP, whatever the cover needed (the largest remaining tracebacks of each kind)
    def is_est(k):
        p = cands[k]["pen"]
        return p is not None and (p[12] != PEN_DEFAULT[12] or p[13] != PEN_DEFAULT[13])
    pen_live = [k for k in live if cands[k]["pen"] is not None and results[k]["rc"] == 0]
    by_size = sorted(pen_live, key=lambda k: (-len(sets[k]), k))
    for want, pred in ((3, is_est), (8, lambda k: True)):
        for k in by_size:
            if sum(1 for q in keep if cands[q]["pen"] is not None and pred(q)) >= want:
                break
            if k not in keep and pred(k):
                keep.append(k)
    keep.sort()

    all_entered = set()
    cases = []
    for k in keep:
        c = cands[k]
        f_ = subprocess.run(driver_cmd(DRV, "fold", c), capture_output=True, text=True, timeout=a.timeout)
        h_ = subprocess.run(driver_cmd(DRV, "hash", c), capture_output=True, text=True, timeout=a.timeout)
        assert h_.returncode == 0, (c, h_.stderr)
        assert f_.returncode == results[k]["rc"], (c, f_.returncode, results[k]["rc"])
        h, mfe = parse_hashes(h_.stdout)
        ent = entered_ids(results[k])
        all_entered |= set(ent)
        cases.append({"seq": c["seq"], "params": c["params"], "dangles": c["dangles"], "noGU": c["noGU"],
                      "pen": c["pen"], "rc": f_.returncode, "stdout": f_.stdout, "stderr": f_.stderr,
                      "hashes": h, "mfe": mfe, "entered": ent, "source": c["source"]})
    # what any candidate reached must be in the fixture (the cover is over lines, ids follow)
    reached_any = set()
    for k in live:
        reached_any |= set(entered_ids(results[k]))
    assert reached_any == all_entered, sorted(reached_any - all_entered)

    searched = len(cands) - n_corpus - len(dropped)
    with open(UNREACHED_REASONS_FILE) as f:
        reasons = json.load(f)
    budget = (f"search budget exhausted: zero hits in {searched} candidate folds beyond the corpus "
              f"({a.random} random, n 30-70, six parameter sets, dangles 0/1/2, five alphabets, with and without "
              f"noGU; {a.pen} penalty overrides within 10x of the defaults; the rest hand-designed shapes, with "
              f"default and with lowered PSM)")
    unreached = []
    for i in all_ids():
        if i in all_entered:
            continue
        base = i.split("@")[0]
        if i in reasons:
            why = reasons[i]
        elif "@" in i and base not in all_entered and base in reasons:
            why = f"sub-branch of {base}, which is never entered: " + reasons[base]
        else:
            why = budget
        unreached.append({"id": i, "reason": why})

    stats = {}
    for fname in FUNCS:
        execl = set()
        for k in live:
            execl |= set(results[k]["exec"].get(fname, []))
        corpus = set()
        for k in live:
            if k < n_corpus:
                corpus |= set(results[k]["lines"].get(fname, []))
        fixture = {ln for (f, ln) in covered if f == fname}
        for k in keep:
            fixture |= set(results[k]["lines"].get(fname, []))
        stats[fname] = {"function": FUNCS[fname].split()[1].rstrip("("), "lines": len(execl),
                        "corpus": len(corpus), "corpus_and_fixture": len(corpus | fixture), "fixture": len(fixture)}
    doc = {"pen_order": PEN_NAMES, "pen_default": PEN_DEFAULT,
           "search": {"candidates": len(cands), "corpus": n_corpus, "dropped_at_time_limit": len(dropped),
                      "searched_beyond_corpus": searched},
           "coverage": stats, "cases": cases, "unreached": unreached}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(json.dumps({"cases": len(cases), "pen_cases": sum(1 for c in cases if c["pen"]), "unreached": len(unreached),
                      "coverage": stats, "dropped": len(dropped)}, indent=1))


if __name__ == "__main__":
    main()
