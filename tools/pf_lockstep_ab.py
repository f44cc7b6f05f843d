"""Partition function: the lockstep batch against one capacity context on the parent commit's
library, alternating, on one GPU.

    python tools/pf_lockstep_ab.py [--reps 3] [--ks 4,8,16] [--parent parent] [--out FILE]   the driver
    python tools/pf_lockstep_ab.py --child rebind | lockstep --k K                            one mode, one process

--parent NAME: the A side runs on ccj_amd/lib/libccj_hip_NAME.so, a build of the parent commit
(CCJ_LIB_VARIANT, as tools/pf_contexts_ab.py's A side); the B side on this tree's library.

The workload is the MFE batch's own (tools/lockstep_ab.py): 64 random ACGU sequences, lengths uniform in
20 .. 120, long and short alternating, Turner04 d2; every process is warmed by three folds.  Per
repetition the driver runs, in alternation and in one fresh process per mode, pf_many(seqs) on the parent
(rebind + fill per sequence) and pf_many(seqs, lockstep=K) for each K.  A process reports, as JSON lines,
ms per sequence of
  * the 64-sequence set through pf_many (context or batch created inside the call), and
  * equal-length sequences at n = 30, 60, 120: rebind + fill of one context that exists already (parent),
    against bind + fill of an existing batch of K members (lockstep; median / min of 8),
timed by the host clock around calls that end in a device synchronise.  A lockstep process also runs the
set without lockstep (untimed) and reports same_results.  Then bench.py --pf (n = 200, the single
sequence) runs on the parent and on this tree, alternating.  The driver ends with one line per K: whether
the batch was ahead of the parent in every repetition, and with the bench pairs.
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED, NSEQ, LO, HI = 20240, 64, 20, 120
FIXED = (30, 60, 120)


def workload():
    r = random.Random(SEED)
    seqs = sorted(("".join(r.choice("ACGU") for _ in range(r.randint(LO, HI))) for _ in range(NSEQ)), key=len)
    out = []
    while seqs:  # long and short alternating
        out.append(seqs.pop())
        if seqs:
            out.append(seqs.pop(0))
    return out


def equal_length(n, k):
    r = random.Random(SEED + n)
    return ["".join(r.choice("ACGU") for _ in range(n)) for _ in range(k)]


def _plain(recs):
    return [(s, repr(e), repr(w)) for s, e, w in recs]


def child(mode, k):
    import torch
    from ccj_amd import W_final_pf, pf_many
    kw = {} if mode == "rebind" else dict(lockstep=k)
    tag = dict(mode=mode, k=k, lib=os.environ.get("CCJ_LIB_VARIANT", "") or "tree")

    def emit(**d):
        print(json.dumps({**tag, **d}), flush=True)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    seqs = workload()
    pf_many(seqs[:3], 2, params="Turner04", **kw)  # warm-up: three folds
    ms, recs = timed(lambda: pf_many(seqs, 2, params="Turner04", **kw))
    d = dict(config="pf_many_64", ms_per_seq=ms / len(seqs), nseq=len(seqs), ok=sum(r[1] is not None for r in recs))
    if mode == "lockstep":
        d["same_results"] = _plain(recs) == _plain(pf_many(seqs, 2, params="Turner04"))
    emit(**d)
    for n in FIXED:
        eq, other = equal_length(n, k), equal_length(n, k)[::-1]
        if mode == "rebind":
            pf = W_final_pf(eq[0], params="Turner04", capacity=n)
            try:
                pf.ccj_pf()
                ts = []
                for s in (other + eq)[:8]:
                    def one():
                        pf.rebind(s)
                        pf.ccj_pf()
                    ts.append(timed(one)[0])
                emit(config="rebind_fill_at_n", n=n, nseq=1, ms_per_seq_median=statistics.median(ts), ms_per_seq_min=min(ts),
                     fill_ms=pf.fill_ms())
            finally:
                pf.close()
            continue
        from ccj_amd import PfLockstepBatch
        b = PfLockstepBatch(n, k, 2, params="Turner04")
        try:
            ts, fills = [], []
            for rep in range(9):  # the first is the batch's warm-up
                def one():
                    b.bind(eq if rep % 2 else other)
                    b.fill()
                ts.append(timed(one)[0] / k)
                fills.append(b.fill_ms())
            emit(config="bind_fill_at_n", n=n, nseq=k, ms_per_seq_median=statistics.median(ts[1:]), ms_per_seq_min=min(ts[1:]),
                 fill_ms_median=statistics.median(fills[1:]), fill_ms_per_level=statistics.median(fills[1:]) / max(n - 2, 1),
                 launches=b.launches())
        finally:
            b.close()


def drive(reps, ks, parent, out, bench_steps):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if out:  # every line as it comes: a run cut short keeps what it measured
            with open(out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def run(cmd, variant):
        env = dict(os.environ)
        env.pop("CCJ_LIB_VARIANT", None)
        if variant:
            env["CCJ_LIB_VARIANT"] = variant
        return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)

    say(f"# PF lockstep A/B: {NSEQ} random ACGU sequences, lengths uniform in {LO}..{HI}, long and short alternating, seed {SEED},")
    say(f"# Turner04 d2; A = pf_many(seqs) on libccj_hip_{parent}.so (the parent commit), B = pf_many(seqs, lockstep=K) on this")
    say("# tree; one fresh process per mode, alternating, each warmed by three folds; host clock around calls that end in a")
    say("# device synchronise; ms per sequence.")
    modes = [("rebind", 1, parent)] + [("lockstep", k, "") for k in ks]
    got = {}
    for rep in range(1, reps + 1):
        for mode, k, variant in modes:
            p = run([sys.executable, os.path.abspath(__file__), "--child", mode, "--k", str(8 if mode == "rebind" else k)], variant)
            if p.returncode != 0:
                say(f"rep {rep} FAIL {mode} k={k}: {p.stderr[-400:]}")
                return 1
            for ln in p.stdout.splitlines():
                if ln.startswith("{"):
                    say(f"rep {rep} {ln}")
                    d = json.loads(ln)
                    if d["config"] == "pf_many_64":
                        got.setdefault((mode, k), []).append(d)
    base = [d["ms_per_seq"] for d in got[("rebind", 1)]]
    say(f"# parent pf_many: {' '.join('%.2f' % v for v in base)} ms per sequence (spread {min(base):.2f} .. {max(base):.2f})")
    for k in ks:
        v = [d["ms_per_seq"] for d in got[("lockstep", k)]]
        same = all(d.get("same_results") for d in got[("lockstep", k)])
        ahead = all(x < y for x, y in zip(v, base))
        say(f"# lockstep={k}: {' '.join('%.2f' % x for x in v)} ms per sequence; ahead of the parent in every pair: {ahead}; "
            f"same_results: {same}")
    # the single sequence: bench.py --pf at n = 200, parent against this tree, alternating pairs
    say(f"# bench.py --pf --gpus 1 --n 200 --steps {bench_steps} --warmup 1: parent / tree, alternating")
    vals = {parent: [], "tree": []}
    for rep in range(1, reps + 1):
        for name, variant in ((parent, parent), ("tree", "")):
            p = run([sys.executable, os.path.join(ROOT, "bench.py"), "--pf", "--gpus", "1", "--n", "200", "--steps", str(bench_steps),
                     "--warmup", "1"], variant)
            ln = next((x for x in reversed(p.stdout.splitlines()) if x.startswith("{")), None)
            if p.returncode != 0 or ln is None:
                say(f"bench rep {rep} FAIL {name}: {p.stderr[-400:]}")
                return 1
            d = json.loads(ln)
            vals[name].append(d["value"])
            say(f"bench rep {rep} lib={name} {ln}")
    a, b = vals[parent], vals["tree"]
    say(f"# bench --pf value: parent {' '.join('%.4g' % x for x in a)} (spread {min(a):.4g} .. {max(a):.4g}); "
        f"tree {' '.join('%.4g' % x for x in b)}; tree inside the parent's spread: {all(min(a) <= x <= max(a) for x in b)}")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["rebind", "lockstep"])
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ks", default="4,8,16")
    ap.add_argument("--parent", default="parent")
    ap.add_argument("--bench-steps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.k)
    else:
        sys.exit(drive(a.reps, [int(x) for x in a.ks.split(",")], a.parent, a.out, a.bench_steps))
