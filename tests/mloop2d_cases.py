"""Inputs shared by tests/test_mloop2d_invariant.py and tests/test_gpu_mloop2d.py.

The engine keeps the PL and PR multiloop families (PLmloop00/01/10, PRmloop00/01/10) as 2-D tables
(ccj_amd/csrc/ccj_mloop2d.h).  Under the reference's default penalties these families are mostly
32767 at small n (the same-cell seed is 32767 + bp with bp > 0), so the cases include one penalty
set with negative PSM, PPS, ap, bp and cp, under which they, and the PM / PO families and PL / PR
that read them, hold many finite values.
"""
import random

# ccj_pk_penalties in struct order: PS PSM PSP PB PUP PPS a b c ap bp cp e_stP e_intP
# (h_globals.hh:7-25 defaults: -138 1007 1500 246 6 96 339 3 2 341 56 12 0.89 0.74)
NEG_PEN = (-138, -200, 1500, 246, 6, -30, 339, 3, 2, -100, -40, -3, 0.89, 0.74)

FAMILY_L = ("PLmloop00", "PLmloop01", "PLmloop10")  # functions of (i, j)
FAMILY_R = ("PRmloop00", "PRmloop01", "PRmloop10")  # functions of (k, l)


def rseq(seed, n, alphabet):
    r = random.Random(seed)
    return "".join(r.choice(alphabet) for _ in range(n))


# (sequence, parameter set, dangles, pen): two parameter sets, dangles 0 / 1 / 2, a GC-rich alphabet
CPU_CASES = [
    (rseq(4101, 36, "ACGU"), "Turner04", 2, None),
    (rseq(4102, 40, "GC"), "DirksPierce09", 1, None),
    (rseq(4103, 44, "GCGCAU"), "Turner04", 0, None),
    (rseq(4104, 48, "ACGU"), "DirksPierce09", 2, None),
    (rseq(4105, 42, "GCGCAU"), "Turner04", 2, NEG_PEN),
    (rseq(4106, 38, "ACGU"), "DirksPierce09", 1, NEG_PEN),
]


def valid_cells(n):
    """Every (i, j, k, l) with 1 <= i <= j < k-1, k <= l <= n, (i, j) ascending, then (k, l)."""
    for i in range(1, n + 1):
        for j in range(i, n + 1):
            for k in range(j + 2, n + 1):
                for l in range(k, n + 1):
                    yield i, j, k, l
