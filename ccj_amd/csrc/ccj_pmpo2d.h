// ccj_pmpo2d.h — the PM and PO multiloop families in closed form from 2-D tables.
//
// compute_PMmloop00 (pseudo_loop.cc:544-560) and compute_POmloop00 (:595-612) seed with PM.get /
// PO.get of the cell being computed, which is not set yet: always 32767 + bp.  Every
// other term of :544-644 is a family value of a smaller cell plus a 2-D WB / WBP value, and each term
// moves (i,j) or (k,l), never both.  So every value of PMmloop00/01/10 and POmloop00/01/10 is a
// shortest path whose steps have separable costs, through a store that clamps at 32767 (Matrix4D::set;
// a minimum >= INF/2 is never stored and reads back as the initial 32767): const + f(i,j) + g(k,l), or
// the minimum of two such sums, one of which restarts from a clamped cell.
//
// Notation: cl(x) = min(32767, x); WBPr the raw WBP (INF + 1 when unset); WB(p,q) = 0 if p > q, else
// min(cp (q-p+1), WBPr(p,q)) (get_WB, :647-653); s = cl(32767 + bp).  An empty min is INF.  Nine
// int32 span-major tables of an interval (p, q), p <= q (the same recurrence serves an (i,j) and a
// (k,l) interval, so the (k,l) tables B and Bo of the derivation are Ao and A):
//   A (p,q) = min(0, min_{d=p..q-1}   A(p,d) + WB(d+1,q))
//   Ao(p,q) = min(0, min_{d=p+1..q}   WB(p,d-1) + Ao(d,q))
//   Up(p,q) = min(U(p,q), Up(p,q-1) + cp),  U(p,q) = min_{d=p+1..q} WBPr(p,d-1) + A(d,q)
//   Uo(p,q) =                                         min_{d=p+1..q} WBPr(p,d-1) + Ao(d,q)
//   Y (p,q) = min(X(p,q), Y(p+1,q) + cp),   X(p,q) = min_{d=p..q-1} Ao(p,d) + WBPr(d+1,q)
//   Xo(p,q) =                                         min_{d=p..q-1} A(p,d) + WBPr(d+1,q)
//   Z (p,q) = min(Ao(p,q), min_{d=p+1..q-1} Z(p,d)  + WB(d+1,q))
//   Zo(p,q) = min(A(p,q),  min_{d=p+1..q-1} Zo(p,d) + WB(d+1,q))
//   Cl(p,q) = min(0,       min_{d=p+1..q-1} Cl(p,d) + WB(d+1,q))
// and the stored values of cell (i,j,k,l):
//   PMmloop00 = cl(s + A(i,j) + Ao(k,l))
//   PMmloop01 = cl(min(32767 + min(0, cp (l-k)),           s + A(i,j) + Y(k,l)))
//   PMmloop10 = cl(min(32767 + min(0, cp (j-i)) + Cl(k,l), s + Up(i,j) + Z(k,l)))
//   POmloop00 = cl(s + Ao(i,j) + A(k,l))
//   POmloop01 = cl(s + Ao(i,j) + Xo(k,l))
//   POmloop10 = cl(min(32767 + Cl(k,l),                    s + Uo(i,j) + Zo(k,l)))
// A span-w entry needs WBP of spans <= w-1 and table entries of spans < w: k_diag2d(w) computes it.
// The INF entries must survive the sums, hence int32 (finite entries stay below INF/2 like a stored WBP).
//
// The recurrences are written once here, for host and device: one split step, the end of a span, and
// the six evaluators.
#pragma once
#include "ccj_energy.h"

namespace ccj {

// the six closed-form matrices (ccj_engine.h carrier: IN_CF)
constexpr unsigned CF_MASK = (1u << PMmloop00) | (1u << PMmloop01) | (1u << PMmloop10) | (1u << POmloop00) |
                             (1u << POmloop01) | (1u << POmloop10);
enum CfTab { CF_A = 0, CF_AO, CF_UP, CF_UO, CF_Y, CF_XO, CF_Z, CF_ZO, CF_CL, NCF };

struct Pmpo2dAcc {
    int a, ao, u, uo, x, xo, z, zo, cl;
};
CCJ_HD Pmpo2dAcc pmpo2d_begin() { return {INF, INF, INF, INF, INF, INF, INF, INF, INF}; }

// Split step s (1 <= s <= w) of interval (p, q = p+w):
//   head = WBPr(p, p+s-1), tail = WBPr(q-s+1, q)
//   aL aoL zL zoL clL = A Ao Z Zo Cl (p, q-s)   (d = q-s: the left part, then WB / WBPr(d+1, q))
//   aR aoR            = A Ao (p+s, q)           (d = p+s: WB / WBPr(p, d-1), then the right part)
CCJ_HD void pmpo2d_step(Pmpo2dAcc &R, int s, int w, int cp, int head, int tail, int aL, int aoL, int zL, int zoL, int clL,
                        int aR, int aoR) {
    const int wb_head = imin(cp * s, head), wb_tail = imin(cp * s, tail);
    R.a = imin(R.a, aL + wb_tail);
    R.ao = imin(R.ao, wb_head + aoR);
    R.u = imin(R.u, head + aR);
    R.uo = imin(R.uo, head + aoR);
    R.x = imin(R.x, aoL + tail);
    R.xo = imin(R.xo, aL + tail);
    if (s < w) {  // d > p
        R.z = imin(R.z, zL + wb_tail);
        R.zo = imin(R.zo, zoL + wb_tail);
        R.cl = imin(R.cl, clL + wb_tail);
    }
}

// the span's entries from the reduced steps; up_prev = Up(p, q-1), y_next = Y(p+1, q) (span w-1; unused when w = 0)
CCJ_HD void pmpo2d_end(const Pmpo2dAcc &R, int w, int cp, int up_prev, int y_next, int *out) {
    out[CF_A] = imin(0, R.a);
    out[CF_AO] = imin(0, R.ao);
    out[CF_UP] = w >= 1 ? imin(R.u, up_prev + cp) : R.u;
    out[CF_UO] = R.uo;
    out[CF_Y] = w >= 1 ? imin(R.x, y_next + cp) : R.x;
    out[CF_XO] = R.xo;
    out[CF_Z] = imin(out[CF_AO], R.z);
    out[CF_ZO] = imin(out[CF_A], R.zo);
    out[CF_CL] = imin(0, R.cl);
}

CCJ_HD int pmpo2d_cl(int v) { return imin(INTERN_INF, v); }
CCJ_HD int pmpo2d_seed(int bp) { return pmpo2d_cl(INTERN_INF + bp); }

// the six stored values from table entries; ij = entries of (i,j), kl = entries of (k,l)
CCJ_HD int pmpo2d_PMmloop00(int s, int a_ij, int ao_kl) { return pmpo2d_cl(s + a_ij + ao_kl); }
CCJ_HD int pmpo2d_PMmloop01(int s, int cp, int b, int a_ij, int y_kl) {
    return pmpo2d_cl(imin(INTERN_INF + imin(0, cp * b), s + a_ij + y_kl));
}
CCJ_HD int pmpo2d_PMmloop10(int s, int cp, int a, int up_ij, int z_kl, int cl_kl) {
    return pmpo2d_cl(imin(INTERN_INF + imin(0, cp * a) + cl_kl, s + up_ij + z_kl));
}
CCJ_HD int pmpo2d_POmloop00(int s, int ao_ij, int a_kl) { return pmpo2d_cl(s + ao_ij + a_kl); }
CCJ_HD int pmpo2d_POmloop01(int s, int ao_ij, int xo_kl) { return pmpo2d_cl(s + ao_ij + xo_kl); }
CCJ_HD int pmpo2d_POmloop10(int s, int uo_ij, int zo_kl, int cl_kl) {
    return pmpo2d_cl(imin(INTERN_INF + cl_kl, s + uo_ij + zo_kl));
}

// matrix x (one of CF_MASK) at cell (i,j,k,l); tab(f, p, q) = entry (p,q) of table f
template <class TAB>
CCJ_HD int pmpo2d_eval(int x, int bp, int cp, const TAB &tab, int i, int j, int k, int l) {
    const int s = pmpo2d_seed(bp);
    switch (x) {
        case PMmloop00: return pmpo2d_PMmloop00(s, tab(CF_A, i, j), tab(CF_AO, k, l));
        case PMmloop01: return pmpo2d_PMmloop01(s, cp, l - k, tab(CF_A, i, j), tab(CF_Y, k, l));
        case PMmloop10: return pmpo2d_PMmloop10(s, cp, j - i, tab(CF_UP, i, j), tab(CF_Z, k, l), tab(CF_CL, k, l));
        case POmloop00: return pmpo2d_POmloop00(s, tab(CF_AO, i, j), tab(CF_A, k, l));
        case POmloop01: return pmpo2d_POmloop01(s, tab(CF_AO, i, j), tab(CF_XO, k, l));
        default: return pmpo2d_POmloop10(s, tab(CF_UO, i, j), tab(CF_ZO, k, l), tab(CF_CL, k, l));
    }
}

// ---- the lowest pre-clamp value of the six matrices over the valid cells (site CF) ----
// Wherever the inner expression F of cl(F) above is below 32767 it is the value Matrix4D::set is
// handed, so "some valid cell of matrix x is stored from a value below -32768" is min F < -32768 over
// the valid cells 1 <= i <= j, j+2 <= k <= l <= n.  F is the minimum of one or two branches
// const + f(i,j) + g(k,l); a branch's minimum under k >= j+2 is
//   const + min_{k=3..n} ( min_{j<=k-2} min_{i<=j} f(i,j)  +  min_{l>=k} g(k,l) ).
// An interval that belongs to no valid cell ((i,j) with j > n-2, (k,l) with k < 3) never enters.
// The branches are listed once here; the host reduction below and k_cf_low walk the same list.
constexpr int CF_NBR = 9;                              // branches of the six formulas
constexpr int CF_ZERO = NCF, CF_CPSPAN = NCF + 1;      // term kinds beside the tables: 0, min(0, cp * span)
constexpr int CF_NKIND = NCF + 2;
// branch br: the matrix it belongs to (0..5 = PMmloop00/01/10, POmloop00/01/10), whether its constant
// is the seed s (else the restart 32767), and the kinds of its (i,j) and (k,l) terms
CCJ_HD void pmpo2d_branch(int br, int &mat6, bool &seeded, int &f, int &g) {
    switch (br) {
        case 0: mat6 = 0; seeded = true; f = CF_A; g = CF_AO; break;
        case 1: mat6 = 1; seeded = false; f = CF_ZERO; g = CF_CPSPAN; break;
        case 2: mat6 = 1; seeded = true; f = CF_A; g = CF_Y; break;
        case 3: mat6 = 2; seeded = false; f = CF_CPSPAN; g = CF_CL; break;
        case 4: mat6 = 2; seeded = true; f = CF_UP; g = CF_Z; break;
        case 5: mat6 = 3; seeded = true; f = CF_AO; g = CF_A; break;
        case 6: mat6 = 4; seeded = true; f = CF_AO; g = CF_XO; break;
        case 7: mat6 = 5; seeded = false; f = CF_ZERO; g = CF_CL; break;
        default: mat6 = 5; seeded = true; f = CF_UO; g = CF_ZO; break;
    }
}
CCJ_HD int pmpo2d_branch_const(bool seeded, int bp) { return seeded ? pmpo2d_seed(bp) : INTERN_INF; }
// a term of kind `kind` at interval (p,q) from its table entry (unused for the two table-free kinds)
CCJ_HD int pmpo2d_term(int kind, int cp, int span, int entry) {
    return kind == CF_ZERO ? 0 : kind == CF_CPSPAN ? imin(0, cp * span) : entry;
}

// F of matrix mat6 at one cell from the branch list: pmpo2d_eval's value before its outer cl()
template <class TAB>
CCJ_HD int pmpo2d_inner(int mat6, int bp, int cp, const TAB &tab, int i, int j, int k, int l) {
    int v = 3 * INF;
    for (int br = 0; br < CF_NBR; ++br) {
        int m, f, g;
        bool seeded;
        pmpo2d_branch(br, m, seeded, f, g);
        if (m != mat6) continue;
        v = imin(v, pmpo2d_branch_const(seeded, bp) + pmpo2d_term(f, cp, j - i, f < NCF ? tab(f, i, j) : 0) +
                        pmpo2d_term(g, cp, l - k, g < NCF ? tab(g, k, l) : 0));
    }
    return v;
}

// Host: out6[x] = the minimum of F over the valid cells (INF when there is none, n < 3), by the
// reduction above: O(n^2) table reads per branch.  tab(f, p, q) as for pmpo2d_eval.
template <class TAB>
inline void pmpo2d_low_host(int n, int bp, int cp, const TAB &tab, int out6[6]) {
    for (int x = 0; x < 6; ++x) out6[x] = INF;
    if (n < 3) return;
    int *pre = new int[n + 1];
    for (int br = 0; br < CF_NBR; ++br) {
        int mat6, f, g;
        bool seeded;
        pmpo2d_branch(br, mat6, seeded, f, g);
        pre[0] = INF;
        for (int j = 1; j <= n - 2; ++j) {
            int fm = INF;
            for (int i = 1; i <= j; ++i) fm = imin(fm, pmpo2d_term(f, cp, j - i, f < NCF ? tab(f, i, j) : 0));
            pre[j] = imin(pre[j - 1], fm);
        }
        int best = 3 * INF;
        for (int k = 3; k <= n; ++k) {
            int gm = INF;
            for (int l = k; l <= n; ++l) gm = imin(gm, pmpo2d_term(g, cp, l - k, g < NCF ? tab(g, k, l) : 0));
            best = imin(best, pre[k - 2] + gm);
        }
        out6[mat6] = imin(out6[mat6], pmpo2d_branch_const(seeded, bp) + best);
    }
    delete[] pre;
}

// Host: all nine tables of a sequence from its raw WBP, wbp[(q-p)*rs + p] for 1 <= p <= q <= n (rs >= n+2),
// into tabs[f*N + (q-p)*rs + p].  The device fill computes the same entries span by span (k_diag2d).
inline void pmpo2d_host_tables(int n, int rs, int cp, const int *wbp, int *tabs, long long N) {
    for (int w = 0; w < n; ++w)
        for (int p = 1; p + w <= n; ++p) {
            const int q = p + w;
            Pmpo2dAcc R = pmpo2d_begin();
            for (int s = 1; s <= w; ++s) {
                const int o = (w - s) * rs + p;  // span w-s: (p, q-s) at o, (p+s, q) at o+s
                pmpo2d_step(R, s, w, cp, wbp[(s - 1) * rs + p], wbp[(s - 1) * rs + q - s + 1], tabs[CF_A * N + o],
                            tabs[CF_AO * N + o], tabs[CF_Z * N + o], tabs[CF_ZO * N + o], tabs[CF_CL * N + o],
                            tabs[CF_A * N + o + s], tabs[CF_AO * N + o + s]);
            }
            int out[NCF];
            const int o1 = (w - 1) * rs + p;
            pmpo2d_end(R, w, cp, w >= 1 ? tabs[CF_UP * N + o1] : 0, w >= 1 ? tabs[CF_Y * N + o1 + 1] : 0, out);
            for (int f = 0; f < NCF; ++f) tabs[f * N + w * rs + p] = out[f];
        }
}

}  // namespace ccj
