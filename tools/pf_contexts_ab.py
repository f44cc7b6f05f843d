"""What a partition-function fold of a NEW sequence costs, per sequence (wall clock, ms).

    python tools/pf_contexts_ab.py MODE N [N ...] [--k K] [--params Turner04]

MODE  create : W_final_pf(seq) + ccj_pf() + close() for each sequence — the only way before
               capacity contexts (also runs on a library built from an older tree: CCJ_LIB_VARIANT)
      rebind : one capacity-N context, rebind(seq) + ccj_pf() for each sequence
      setup  : one capacity-N context, rebind(seq) alone (CCJ_PF_HOST_SETUP=1: the host builder)
K distinct random sequences per length (seed 5 + their index; default 4), after one untimed warm-up
sequence; prints one line per length with the median and the min.  For A/B runs see tools/gpu_ab.sh
(MODE=pfctx).
"""
import argparse
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ccj_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["create", "rebind", "setup"])
ap.add_argument("n", type=int, nargs="+")
ap.add_argument("--k", type=int, default=4)
ap.add_argument("--params", default="Turner04")
a = ap.parse_args()


def seqs(n, k):
    out = []
    for x in range(k):
        r = random.Random(5 + 1000 * x)
        out.append("".join(r.choice("ACGU") for _ in range(n)))
    return out


for n in a.n:
    ss = seqs(n, a.k + 1)
    ms, extra = [], ""
    if a.mode == "create":
        for x, s in enumerate(ss):
            t0 = time.perf_counter()
            pf = ccj_amd.W_final_pf(s, params=a.params)
            e = pf.ccj_pf()
            pf.close()
            if x:
                ms.append(1e3 * (time.perf_counter() - t0))
    else:
        t0 = time.perf_counter()
        pf = ccj_amd.W_final_pf(ss[0], params=a.params, capacity=n)
        e = pf.ccj_pf()
        kt_ms, kt_b = pf.keytab_info()
        extra = " context %.1f ms keytab %.1f ms %d B" % (1e3 * (time.perf_counter() - t0), kt_ms, kt_b)
        for s in ss[1:]:
            t0 = time.perf_counter()
            pf.rebind(s)
            if a.mode == "rebind":
                e = pf.ccj_pf()
            ms.append(1e3 * (time.perf_counter() - t0))
        pf.close()
    print("pfctx %-6s n=%-4d ms/seq median %.2f min %.2f (k=%d)%s energy %r" %
          (a.mode, n, statistics.median(ms), min(ms), len(ms), extra, e), flush=True)
