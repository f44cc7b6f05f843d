"""Folds under non-default pseudoknot penalties for the reset, rebind and lockstep paths, shared by
tests/test_pen_companions.py (CPU) and tests/test_gpu_pen_contexts.py — TEST INFRASTRUCTURE ONLY.

A case is one reference-pinned fold of tests/golden/traceback_mloop_cases.json (strongly negative bp:
the twelve table-carried matrices are dense and the traceback enters the multiloop-family nodes) or
of tests/golden/traceback_cases.json (an e_stP / e_intP override, or the one fixture group with two
sequences under one penalty set).  Each case's sequence s has six companions, derived from s alone:
four shorter ones of different lengths, whose planes lie inside those of s, and two of its own length
with the same base composition.  A fold is one (case, sequence): what it must give is the fixture's
own record for s, and for a companion the C restatement's hashes and W(n) under the case's penalties.
"""
import random

from tests.mloop2d_cases import FAMILY_L, FAMILY_R, valid_cells
from tests.oracle_lib import HASH_NAMES, OracleFold, blob, golden

MLOOP_CASES = golden("traceback_mloop_cases.json")["cases"]
_TB = golden("traceback_cases.json")["cases"]
STP_CASES = [c for c in _TB if c["pen"] is not None and tuple(c["pen"][12:]) != (0.89, 0.74)]
PAIR_CASES = [c for c in _TB if (c["params"], c["dangles"], len(c["seq"])) == ("CaoChen06", 1, 49)]
CASES = MLOOP_CASES + STP_CASES + PAIR_CASES
SMALLEST = sorted(MLOOP_CASES, key=lambda c: len(c["seq"]))[:2]  # stable: ties keep the fixture's order
# its seven lengths reach every split of the batched level launch under the targets of
# tests/lockstep_rows.py (tests/test_pen_companions.py asks ccj_batch_level_plan)
SPLIT_CASE = next(c for c in MLOOP_CASES if 57 <= len(c["seq"]) <= 59)

OWN = "own"  # the fixture's sequence itself
COMPANIONS = ("head3", "head7", "tail2", "mid", "reverse", "shuffle")
SAME_LENGTH = ("reverse", "shuffle")
# companions left out because their fold lies outside the domain in which the reference defines a
# result, by case id.  None for the int16 range (tests/test_pen_companions.py holds every
# kept fold to low_stores() == 0).  One because the reference's own traceback does not end on it: its
# run of this sequence under these penalties recurses until it is killed by SIGSEGV, and the engine's
# walk, in a fresh context too, stops at its step limit ("traceback did not end within 4194304 steps",
# seconds on the device).  The fixture generators drop such folds too (oracle/gen_traceback_mloop_cases.py).
# tests/test_pen_companions.py holds this map to its cap.
DROPPED = {"n21-DirksPierce09-d0-bp-8084-st0.89-CGGUUG22": ("reverse",)}

TWELVE = FAMILY_L + FAMILY_R + tuple(f"P{f}mloop{s}" for f in "MO" for s in ("00", "01", "10"))
MIN_DENSE = 1000  # of the twelve matrices' valid cells below 32767, per multiloop fold at n <= 34

_restated = {}


def case_id(c):
    return f"n{len(c['seq'])}-{c['params']}-d{c['dangles']}-bp{c['pen'][10]}-st{c['pen'][12]}-{c['seq'][:6]}{len(c['entered'])}"


def companions(s):
    """The six companion sequences of s, by name."""
    n = len(s)
    return {"head3": s[:n - 3], "head7": s[:n - 7], "tail2": s[2:], "mid": s[3:n - 4], "reverse": s[::-1],
            "shuffle": "".join(random.Random(n).sample(s, n))}


def sequences(case):
    """name -> sequence: the case's own and the companions it keeps, own first."""
    out = {OWN: case["seq"]}
    out.update((k, v) for k, v in companions(case["seq"]).items() if k not in DROPPED.get(case_id(case), ()))
    return out


def oracle(case, seq):
    """A restatement fold of seq under the case's parameters and penalties (the caller closes it); the
    level-parallel restatement above n = 40, which computes the same matrices and the same counter
    (tests/test_traceback_mloop_cases.py test_counter_counts_outside_the_domain)."""
    return OracleFold(seq, blob(case["params"]), case["dangles"], case["noGU"], pen=case["pen"],
                      threads=None if len(seq) <= 40 else 4)


def dense_cells(o, limit):
    """Valid cells of the twelve table-carried matrices below 32767 in the restatement fold o, counted
    up to `limit`."""
    xs = [HASH_NAMES.index(nm) for nm in TWELVE]
    count = 0
    for c in valid_cells(o.n):
        for x in xs:
            count += o.get4(x, *c) < 32767
        if count >= limit:
            break
    return count


def restated(case, name):
    """The restatement's fold of (case, name): {"hashes" (31), "mfe" (W(n)), "low_stores", "dense"
    (dense_cells up to MIN_DENSE at n <= 34, else None)}.  Computed once per process, never changed."""
    key = (case_id(case), name)
    if key not in _restated:
        o = oracle(case, sequences(case)[name])
        try:
            _restated[key] = {"hashes": o.hashes(), "mfe": o.W(o.n), "low_stores": o.low_stores(),
                              "dense": dense_cells(o, MIN_DENSE) if o.n <= 34 else None}
        finally:
            o.close()
    return _restated[key]


def expected(case, name):
    """What the fold (case, name) must give: {"seq", "hashes" (31), "mfe" (W(n)), "output"}.  For the
    case's own sequence these are the reference's own record, output = its (rc, stdout, stderr); for a
    companion the restatement's hashes and W(n), output = None."""
    seq = sequences(case)[name]
    if name == OWN:
        return {"seq": seq, "hashes": case["hashes"], "mfe": case["mfe"],
                "output": (case["rc"], case["stdout"], case["stderr"])}
    r = restated(case, name)
    return {"seq": seq, "hashes": r["hashes"], "mfe": r["mfe"], "output": None}
