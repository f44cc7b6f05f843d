"""Shared by tests/test_il_prune.py (CPU) and tests/test_gpu_il_prune.py: the folds, and the
interior-loop candidate lists of a fold as the host form of the pruning rule reports them
(ccj_amd.il_prune_host, ccj_amd/csrc/ccj_ilprune.h).  No tests here."""
import random

import numpy as np

import ccj_amd
from tests.oracle_lib import blob, golden

U = ccj_amd.IL_U
NEAR, FAR = 1, 2  # ccj_ilprune.h IL_NEAR / IL_FAR: status = 1 | 2 * bits
E_INT_NEG = (-138, 1007, 1500, 246, 6, 96, 339, 3, 2, 341, 56, 12, 0.89, -0.74)
PEN_OTHER = (-120, 900, 1400, 200, 9, 80, 300, 5, 4, 300, 70, 20, 0.83, 0.62)  # every penalty off its default
PAIRS = {"AU", "UA", "GC", "CG", "GU", "UG"}


def rseq(seed, n, letters="ACGU"):
    r = random.Random(seed)
    return "".join(r.choice(letters) for _ in range(n))


def range_case(name):
    return next(c for c in golden("range_cases.json")["cases"] if c["name"] == name)


RANGE = range_case("n30_T04_d0_apneg_bp")
# name -> (sequence, parameter set, dangles, penalties or None)
CPU_FOLDS = {
    "T04_n34": (rseq(21, 34), "Turner04", 2, None),
    "DP09_n32_gc": (rseq(22, 32, "GGGCCCAU"), "DirksPierce09", 2, None),
    "T04_n30_eintneg": (rseq(23, 30), "Turner04", 2, E_INT_NEG),
    "range_pen_in": (RANGE["seq"], RANGE["params"], RANGE["dangles"], tuple(RANGE["pen_in"])),
}

_lists = {}


def lists(seq, params, dangles=2, pen=None, noGU=False):
    """il_prune_host of a fold, computed once and never changed."""
    key = (seq, params, dangles, pen, noGU)
    if key not in _lists:
        _lists[key] = ccj_amd.il_prune_host(seq, blob(params), dangles, noGU, pen)
    return _lists[key]


def can_pair(seq, i, j):
    """pair type > 0 of the 1-based positions, as the fill's pt plane has it (no distance rule)."""
    return seq[i - 1] + seq[j - 1] in PAIRS


def window(seq, kind, p, q):
    """The (u1, u2) of the full list of pair (p, q), from the sequence alone (build_il_body's window)."""
    n, w = len(seq), q - p
    out = []
    for u1 in range(U):
        for u2 in range(U):
            if kind == 0:
                d, dp = p + 1 + u1, q - 1 - u2
                ok = u1 <= min(w, 30) - 2 and u2 <= min(w - u1 - 6, 28) and can_pair(seq, d, dp)
            else:
                d, dp = p - 1 - u1, q + 1 + u2
                ok = d >= 1 and dp <= n and can_pair(seq, d, dp)
            if ok:
                out.append((u1, u2))
    return out


def entries(L, kind):
    """(w, p, u1, u2) of every list entry, as an array of rows."""
    return np.argwhere(L["st_ilm" if kind else "st_il"] != 0)
