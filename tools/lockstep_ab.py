"""Lockstep batch against the capacity-context pipeline, alternating, on one GPU.

    python tools/lockstep_ab.py [--reps 3] [--ks 4,8,16] [--out FILE]      the driver
    python tools/lockstep_ab.py --child contexts2 | lockstep --k K         one mode, one process

The workload is the README's mixed-length batch (profiles/rebind_ab.txt): 64 random ACGU sequences,
lengths uniform in 20 .. 120, long and short alternating, Turner04 d2; every process is warmed by three
folds.  Per repetition the driver runs, in alternation and in one fresh process per mode,
fold_many(contexts=2) (the path of the parent commit, untouched) and fold_many(lockstep=K) for each K.
A process reports, as JSON lines, ms per sequence of
  * the 64-sequence batch through fold_many (contexts and batches created inside the call), and
  * K equal-length sequences at n = 30, 60, 120: fold_many again, and for lockstep also one bind + fold
    of a batch that exists already (median / min of 8), the counterpart of rebind_ab.txt's
    a_rebind_fold_at_n,
timed by the host clock around calls that end in a device synchronise.  A lockstep process also folds
the batch without lockstep (untimed) and reports same_results.  The driver ends with one line per K:
whether lockstep was ahead of contexts=2 in every repetition.
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


def child(mode, k):
    import torch
    from ccj_amd import LockstepBatch, fold_many
    kw = dict(contexts=2) if mode == "contexts2" else dict(lockstep=k)
    tag = dict(mode=mode, k=k)

    def emit(**d):
        print(json.dumps({**tag, **d}), flush=True)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    seqs = workload()
    fold_many(seqs[:3], 2, params="Turner04", **kw)  # warm-up: three folds
    ms, recs = timed(lambda: fold_many(seqs, 2, params="Turner04", **kw))
    d = dict(config="fold_many_64", ms_per_seq=ms / len(seqs), nseq=len(seqs),
             ok=sum(r[4] == 0 for r in recs), exits=sum(r[4] != 0 for r in recs))
    if mode == "lockstep":
        d["same_results"] = recs == fold_many(seqs, 2, params="Turner04", contexts=2)
    emit(**d)
    for n in FIXED:
        eq = equal_length(n, k if mode == "lockstep" else 16)
        ts = [timed(lambda: fold_many(eq, 2, params="Turner04", **kw))[0] / len(eq) for _ in range(3)]
        emit(config="fold_many_equal", n=n, nseq=len(eq), ms_per_seq_median=statistics.median(ts), ms_per_seq_min=min(ts))
        if mode != "lockstep":
            continue
        b = LockstepBatch(n, k, 2, params="Turner04")
        try:
            other = equal_length(n, k)[::-1]
            ts, fills = [], []
            for rep in range(9):  # the first is the batch's warm-up
                def one():
                    b.bind(eq if rep % 2 else other)
                    b.fold()
                ts.append(timed(one)[0] / k)
                fills.append(b.fill_ms())
            emit(config="bind_fold_at_n", n=n, nseq=k, ms_per_seq_median=statistics.median(ts[1:]), ms_per_seq_min=min(ts[1:]),
                 fill_ms_median=statistics.median(fills[1:]), fill_ms_per_level=statistics.median(fills[1:]) / max(n - 2, 1))
        finally:
            b.close()


def drive(reps, ks, out):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# lockstep A/B: {NSEQ} random ACGU sequences, lengths uniform in {LO}..{HI}, long and short alternating, seed {SEED},")
    say("# Turner04 d2; one fresh process per mode, alternating, each warmed by three folds; host clock around calls that end")
    say("# in a device synchronise; ms per sequence.")
    modes = [("contexts2", 2)] + [("lockstep", k) for k in ks]
    got = {}
    for rep in range(1, reps + 1):
        for mode, k in modes:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--k", str(k)], cwd=ROOT,
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                say(f"rep {rep} FAIL {mode} k={k}: {p.stderr[-400:]}")
                return 1
            for ln in p.stdout.splitlines():
                if ln.startswith("{"):
                    say(f"rep {rep} {ln}")
                    d = json.loads(ln)
                    if d["config"] == "fold_many_64":
                        got.setdefault((mode, k), []).append(d)
    base = [d["ms_per_seq"] for d in got[("contexts2", 2)]]
    say(f"# contexts=2: {' '.join('%.2f' % v for v in base)} ms per sequence (spread {min(base):.2f} .. {max(base):.2f})")
    for k in ks:
        v = [d["ms_per_seq"] for d in got[("lockstep", k)]]
        same = all(d.get("same_results") for d in got[("lockstep", k)])
        ahead = all(x < y for x, y in zip(v, base))
        say(f"# lockstep={k}: {' '.join('%.2f' % x for x in v)} ms per sequence; ahead of contexts=2 in every pair: {ahead}; "
            f"same_results: {same}")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["contexts2", "lockstep"])
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ks", default="4,8,16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.k)
    else:
        sys.exit(drive(a.reps, [int(x) for x in a.ks.split(",")], a.out))
