// ccj_mloop2d.h — the PL and PR multiloop families as 2-D tables.
//
// PLmloop00 / 01 / 10 (i,j,k,l) depend on (i,j) only and PRmloop00 / 01 / 10 on (k,l) only:
// compute_PLmloop00 (pseudo_loop.cc:445-463) seeds with PL.get of the cell itself, which is not
// computed yet (always 32767 + bp), and every other term of :445-493 is a 2-D WB /
// WBP value plus a family value of a sub-interval of [i,j] at the same (k,l), a valid cell.  By
// induction on j-i no term sees k or l; the PR family (:495-542) is the mirror image in (k,l).
// So the fill keeps six span-major tables, F00/F01/F10 [j-i][i] and G00/G01/G10 [l-k][k], of the
// stored int16 values (Matrix4D::set clamps at 32767; a minimum >= INF/2 is never stored and reads
// back as the initial 32767), computed per span by k_diag2d.
//
// The recurrences are written once here, for host and device: one split step, then the end of a cell.
#pragma once
#include "ccj_energy.h"

namespace ccj {

// the six table-carried matrices (ccj_engine.h carrier: IN_TAB)
constexpr unsigned TAB_MASK = (1u << PLmloop00) | (1u << PLmloop01) | (1u << PLmloop10) | (1u << PRmloop00) |
                              (1u << PRmloop01) | (1u << PRmloop10);
// table of matrix x: 0..2 = F00 F01 F10 (indexed by (i,j)), 3..5 = G00 G01 G10 (indexed by (k,l))
CCJ_HD constexpr int tab_index(int x) { return x - PLmloop00; }
static_assert(tab_index(PLmloop00) == 0 && tab_index(PLmloop10) == 2 && tab_index(PRmloop00) == 3 &&
              tab_index(PRmloop10) == 5, "the six families are consecutive in Mat4");

struct Mloop2dAcc {
    int m00, m01, m10;
};

// the running minima before the first split step: PLmloop00 / PRmloop00 start from the same-cell
// seed PL.get / PR.get (32767, never set yet) + beta2P = bp (:448, :498), the others from INF
CCJ_HD Mloop2dAcc mloop2d_begin(int bp) { return {INTERN_INF + bp, INF, INF}; }

// get_WB (pseudo_loop.cc:647-653) of an interval of len bases from its WBP
CCJ_HD int mloop2d_wb(int wbp, int len, int cp) { return imin(cp * len, wbp); }

// Split step s (1 <= s <= w, w the interval's span) of interval (p, q = p+w); d is the reference's
// split point.
//   head = WBP(p, p+s-1)    (d = p+s:   get_WB(p,d-1)  / WBP.get(p,d-1))
//   tail = WBP(q-s+1, q)    (d = q-s:   get_WB(d+1,q)  / WBP.get(d+1,q))
//   x00r = X00(p+s, q), x00l = X00(p, q-s), x10l = X10(p, q-s)   (stored values of shorter spans)
// left = the PL family; the PR family has no X10(p,d) + WB(d+1,q) term (:529-542).
CCJ_HD void mloop2d_step(Mloop2dAcc &A, bool left, int s, int w, int cp, int head, int tail, int x00r, int x00l, int x10l) {
    const int wb_head = mloop2d_wb(head, s, cp), wb_tail = mloop2d_wb(tail, s, cp);
    A.m00 = imin(A.m00, imin(wb_head + x00r, x00l + wb_tail));  // :449-458 / :499-508
    A.m01 = imin(A.m01, x00l + tail);                           // :468-471 / :520-523
    A.m10 = imin(A.m10, head + x00r);                           // :481-483 / :534-537
    if (left && s < w) A.m10 = imin(A.m10, x10l + wb_tail);     // :484-486 (d < j)
}

// PR family only: the neighbour terms PRmloop01(i,j,k,l-1) + cp (:519) and PRmloop10(i,j,k+1,l) + cp
// (:533), both of span w-1 (INF when w = 0: the getter of an invalid cell)
CCJ_HD void mloop2d_right_seed(Mloop2dAcc &A, int w, int cp, int g01_prev, int g10_next) {
    if (w < 1) return;
    A.m01 = imin(A.m01, g01_prev + cp);
    A.m10 = imin(A.m10, g10_next + cp);
}

// the stored value: set only if < INF/2, clamped at 32767 (Matrix4D::set); else the initial 32767
CCJ_HD int mloop2d_store(int v) { return v >= INTERN_INF ? INTERN_INF : v; }

}  // namespace ccj
