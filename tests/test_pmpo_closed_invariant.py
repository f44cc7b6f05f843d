"""The closed forms of the PM and PO multiloop families (ccj_amd/csrc/ccj_pmpo2d.h), on the CPU (no GPU).

PMmloop00/01/10 and POmloop00/01/10 are const + f(i,j) + g(k,l), or the minimum of two such sums,
through the reference's clamp at 32767: nine 2-D tables computed from WBP alone.  The
header's own host code (ccj_pmpo2d_closed in the engine library, which loads without a GPU) computes
the tables from the restatement's raw WBP and evaluates all six matrices at every valid cell; each must
equal OracleFold.get4: zero differences.

Inputs: the six CPU_CASES, and two folds whose bp and cp have opposite signs (neither mix is in
CPU_CASES).  Every case with a changed penalty set must hold more than 1000 values below 32767 in each
of the six matrices, and so must at least one default-penalty case, or the comparison would be of
constants.
"""
import ctypes
import os

import pytest

from tests.mloop2d_cases import CPU_CASES, NEG_PEN, rseq, valid_cells
from tests.oracle_lib import HASH_NAMES, ROOT, OracleFold, blob

LIB = os.path.join(ROOT, "ccj_amd", "lib", "libccj_hip.so")
SIX = ("PMmloop00", "PMmloop01", "PMmloop10", "POmloop00", "POmloop01", "POmloop10")


def _pen(bp, cp):
    p = list(NEG_PEN)
    p[10], p[11] = bp, cp
    return tuple(p)


# ccj_pk_penalties: ... ap bp cp ...; the other negative entries of NEG_PEN keep WBP finite
MIX_BP_NEG = _pen(-40, 12)  # bp < 0 < cp
MIX_CP_NEG = _pen(56, -3)   # cp < 0 < bp
CASES = CPU_CASES + [
    (rseq(4107, 40, "GCGCAU"), "Turner04", 2, MIX_BP_NEG),
    (rseq(4108, 40, "GCGCAU"), "DirksPierce09", 1, MIX_CP_NEG),
]

_finite = {}  # case id -> {matrix: values below 32767}


def _id(c):
    pen = c[3]
    tag = "def" if pen is None else "neg" if pen == NEG_PEN else "bpneg" if pen == MIX_BP_NEG else "cpneg"
    return f"n{len(c[0])}-{c[1]}-d{c[2]}-{tag}"


def _closed(n, wbp, bp, cp, cells):
    L = ctypes.CDLL(LIB)
    L.ccj_pmpo2d_closed.restype = ctypes.c_longlong
    L.ccj_pmpo2d_closed.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(ctypes.c_int16), ctypes.c_longlong]
    out = (ctypes.c_int16 * (6 * cells))()
    assert L.ccj_pmpo2d_closed(n, wbp, bp, cp, out, cells) == cells
    return out


def test_cases_cover_the_sign_mixes():
    assert len(CASES) == len(CPU_CASES) + 2 == 8
    assert MIX_BP_NEG[10] < 0 < MIX_BP_NEG[11] and MIX_CP_NEG[11] < 0 < MIX_CP_NEG[10]
    signs = {(c[3][10] < 0, c[3][11] < 0) for c in CASES if c[3] is not None}
    assert signs == {(True, True), (True, False), (False, True)}


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_closed_forms_equal_the_restatement(case):
    seq, params, dangles, pen = case
    n = len(seq)
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    o = OracleFold(seq, blob(params), dangles, 0, pen=pen)
    try:
        wbp = (ctypes.c_int * ((n + 1) * (n + 1)))()
        for i in range(1, n + 1):
            for j in range(i, n + 1):
                wbp[i * (n + 1) + j] = o.get2(1, i, j)
        bp, cp = (56, 12) if pen is None else (pen[10], pen[11])  # h_globals.hh defaults
        cells = list(valid_cells(n))
        got = _closed(n, wbp, bp, cp, len(cells))
        fin = _finite.setdefault(_id(case), {})
        for m, nm in enumerate(SIX):
            x = HASH_NAMES.index(nm)
            diffs, finite, first = 0, 0, None
            for c, cell in enumerate(cells):
                want = o.get4(x, *cell)
                g = got[m * len(cells) + c]
                finite += want < 32767
                if g != want:
                    diffs += 1
                    first = first or (cell, g, want)
            fin[nm] = finite
            print(f"{_id(case)} {nm}: {len(cells)} cells, {finite} below 32767, {diffs} differences")
            assert diffs == 0, f"{nm}: {diffs} of {len(cells)} cells differ, first (cell, closed form, oracle) = {first}"
            if pen is not None:
                assert finite > 1000, f"{nm}: only {finite} values below 32767 (the check would be vacuous)"
    finally:
        o.close()


def test_a_default_penalty_case_is_not_vacuous():
    """Runs after the parametrised test (file order): at least one default-penalty case held more than
    1000 values below 32767 in every one of the six matrices."""
    defs = [_id(c) for c in CASES if c[3] is None]
    missing = [d for d in defs if d not in _finite]
    if missing:  # run alone: fold the default cases now
        for c in CASES:
            if c[3] is None:
                test_closed_forms_equal_the_restatement(c)
    assert any(all(_finite[d].get(nm, 0) > 1000 for nm in SIX) for d in defs), {d: _finite[d] for d in defs}
