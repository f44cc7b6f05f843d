"""The invariant the 2-D multiloop tables rest on, on the CPU restatement alone (no GPU).

PLmloop00 / PLmloop01 / PLmloop10 (i,j,k,l) depend on (i,j) only and PRmloop00 / PRmloop01 /
PRmloop10 on (k,l) only (ccj_amd/csrc/ccj_mloop2d.h): compute_PLmloop00
(pseudo_loop.cc:445-463) seeds with PL.get of the cell being computed, always 32767, and every
other term of :445-542 stays inside the family at the same (k,l) / (i,j).  Every valid cell of the
six matrices must equal the first cell with the same (i,j) / (k,l): zero differences.  The fold
with negative penalties must hold more than 1000 values below 32767 in each of the six, or the
comparison would be of constants.
"""
import pytest

from tests.mloop2d_cases import CPU_CASES, FAMILY_L, FAMILY_R, NEG_PEN, valid_cells
from tests.oracle_lib import HASH_NAMES, OracleFold, blob


def _id(c):
    return f"n{len(c[0])}-{c[1]}-d{c[2]}-{'neg' if c[3] else 'def'}"


def test_cases_cover_what_the_invariant_is_claimed_for():
    assert 4 <= len(CPU_CASES) <= 6 and all(30 <= len(c[0]) <= 48 for c in CPU_CASES)
    assert len({c[1] for c in CPU_CASES}) >= 2 and {c[2] for c in CPU_CASES} == {0, 1, 2}
    assert any(set(c[0]) <= set("GC") for c in CPU_CASES)
    assert any(c[3] == NEG_PEN for c in CPU_CASES)
    PSM, PPS, ap, bp, cp = NEG_PEN[1], NEG_PEN[5], NEG_PEN[9], NEG_PEN[10], NEG_PEN[11]
    assert max(PSM, PPS, ap, bp, cp) < 0


@pytest.mark.parametrize("case", CPU_CASES, ids=_id)
def test_families_depend_on_two_indices_only(case):
    seq, params, dangles, pen = case
    n = len(seq)
    o = OracleFold(seq, blob(params), dangles, 0, pen=pen)
    try:
        for names, key in ((FAMILY_L, lambda i, j, k, l: (i, j)), (FAMILY_R, lambda i, j, k, l: (k, l))):
            for nm in names:
                x = HASH_NAMES.index(nm)
                first, diffs, finite, cells = {}, 0, 0, 0
                for i, j, k, l in valid_cells(n):
                    v = o.get4(x, i, j, k, l)
                    cells += 1
                    finite += v < 32767
                    diffs += first.setdefault(key(i, j, k, l), v) != v
                print(f"{_id(case)} {nm}: {cells} cells, {finite} below 32767, {diffs} differences")
                assert diffs == 0, f"{nm}: {diffs} of {cells} cells differ from the first cell of their 2-D key"
                if pen is not None:
                    assert finite > 1000, f"{nm}: only {finite} values below 32767 (the check would be vacuous)"
    finally:
        o.close()
