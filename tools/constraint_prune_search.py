"""Bounded search for a constrained fold whose pruned interior-loop lists give other matrices than the
masked restatement ("Under a constraint").  CPU only, about a minute:

    python tools/constraint_prune_search.py [--folds 60] [--seed 7]

Each fold is a random sequence over GGCCAU of length 22..30, Turner04 or DirksPierce09, dangles 0 / 1 / 2,
with about 10 % of its positions `x` and 1 to 12 random forbidden pairs.  Its PL, PR and PM are restated
cell by cell from the kept entries of ccj_il_prune_host_constrained and compared with the masked
restatement (the check of tests/test_constraint_oracle.py, which runs it on the committed fixtures).
Prints the first fold that differs (exit code 1), or how many folds and dropped entries it covered.
"""
import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ccj_amd  # noqa: E402
from tests.oracle_lib import blob  # noqa: E402
from tests.test_constraint_oracle import test_pruned_lists_under_a_mask_restate_the_masked_fill as restate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--folds", type=int, default=60)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    r = random.Random(a.seed)
    done = dropped = 0
    for _ in range(a.folds):
        n = r.randint(22, 30)
        seq = "".join(r.choice("GGCCAU") for _ in range(n))
        params, dangles = r.choice(["Turner04", "DirksPierce09"]), r.choice([0, 1, 2])
        unpaired = "".join("x" if r.random() < 0.1 else "." for _ in range(n))
        forbid = []
        for _ in range(r.randint(1, 12)):
            i = r.randint(1, n - 4)
            forbid.append([i, r.randint(i + 4, n)])
        c = dict(seq=seq, params=params, dangles=dangles, noGU=0, unpaired=unpaired, forbid=forbid, allow_only=None, kind="search")
        try:
            restate(c)
        except AssertionError as e:
            print("FOUND", c, e)
            return 1
        k = ccj_amd.il_prune_host(seq, blob(params), dangles, False, windows=False,
                                  constraint=ccj_amd.Constraint(unpaired, [tuple(p) for p in forbid]))["counts"]
        dropped += k[1] - k[0] + k[3] - k[2]
        done += 1
    print(f"searched {done} folds, {dropped} dropped entries: every restated cell equals the masked restatement")
    return 0


if __name__ == "__main__":
    sys.exit(main())
