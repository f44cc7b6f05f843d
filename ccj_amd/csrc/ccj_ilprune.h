// ccj_ilprune.h — interior-loop candidates dominated through a stacked pair.
//
// A candidate of an interior-loop list may be dropped when the fill takes the same inner value by a
// route that costs no more: through an intermediate pair (x,y) that lies strictly between the list's
// own pair and the candidate's pair, can pair under the binding (pt: a pair a constraint forbids cannot),
// and is stacked on one of the two.  With PL as the
// example (closing pair (i,j), candidate (d,dp), u1 = d-i-1 >= 1, u2 = j-dp-1 >= 1; every store clamps
// at 32767 and nowhere else, cl):
//   E  = e_intP(i,d,dp,j)                    the candidate's own energy,
//   E1 = the best energy with which the fill takes PL(x,y,k,l) into PL(i,j,k,l),
//   E2 = the same for (d,dp) into (x,y).
// (d,dp) is a term of get_PLiloop(x,y,k,l), so PL(x,y,k,l) <= cl(PL(d,dp,k,l) + E2), and with
// E1 + E2 <= E the term PL(x,y,k,l) + E1 is not above PL(d,dp,k,l) + E whether or not the clamp bit.
// That term is the stack or the u1 = u2 = 0 loop of the level kernel, or a list entry with a smaller
// u1, which is kept or dominated in turn: the minimum of the cell does not change, ties included.  No
// sign of an energy is used.  PR reads the same lists; PM is the mirror image (its pair (j,k) lies
// inside, the candidates (d,dp) outside), and its per-cell bounds d > i, dp < l hold for (x,y) whenever
// they hold for (d,dp).
//
// Two intermediates are tried, each stacked on one end so that one of E1, E2 is a (0,0) term the level
// kernel evaluates itself (level4d_body: min(est, ie) of the outer of the two stacked pairs):
//   near: (x,y) stacked on the list's own pair      — E1 = that (0,0) term, E2 = one more E_IntLoop;
//   far : (x,y) stacked on the candidate's pair     — E2 = that (0,0) term, E1 = the window's own
//         entry (u1-1, u2-1).
// The window conditions of the list (build_il_body) imply the level kernel's conditions for each
// (0,0) term used (spans > TURN+2 for PL / PR; a, b >= 2 for PM).
//
// Written once for host and device.  TB is any table view with the members n, rs, S, S1, pt, pair
// (8x8, row-major), rtype, prm, lx, e_intP, est, ie (ccj_engine.h DevTables; IlHostTables below).
#pragma once
#include <cmath>
#include <cstdint>
#include "ccj_energy.h"

namespace ccj {

constexpr int IL_NEAR = 1, IL_FAR = 2;  // il_dominated: which intermediate dominates the candidate

// lrint(e_intP * E_IntLoop) of the loop closed by (p,q) around (p+1+u1, q-1-u2), not narrowed
// (pseudo_loop.cc:822-826, 836-840); INTERN_INF where the reference skips the candidate (a pair that
// cannot pair) or the loop has no room
template <class TB>
CCJ_HD int il_eint_raw(const TB &T, int u1, int u2, int p, int q) {
    const int d = p + u1 + 1, dp = q - u2 - 1;
    if (dp - d < 1) return INTERN_INF;
    // the binding's relation (the pt plane), not the 8x8 table: under a constraint a forbidden pair is
    // no pair, so a witness through one is no witness (1 <= p < q <= n and p < d < dp < q here)
    const int t1 = T.pt[(q - p) * T.rs + p];
    const int t2 = T.pt[(dp - d) * T.rs + d];
    if (t1 <= 0 || t2 <= 0) return INTERN_INF;
    const int e = E_IntLoop(T.prm, T.lx, u1, u2, t1, T.rtype[t2], T.S1[p + 1], T.S1[q - 1], T.S1[d - 1], T.S1[dp + 1]);
    return (int)rint(T.e_intP * (double)e);
}
CCJ_HD bool il_e_in_range(int v) { return v >= -32768 && v < INTERN_INF; }

// One candidate (u1,u2) of the window of pair (p,q): kind 0 = the list il (the pair closes the loop
// around (p+1+u1, q-1-u2); get_PLiloop / get_PRiloop, pseudo_loop.cc:694-700, 729-735), kind 1 = ilm
// (an outer pair (p-1-u1, q+1+u2) encloses it; get_PMiloop :762-768 without its per-cell bounds).
// True if the candidate is in the list; e is then its energy (il_eint_raw).
template <class TB>
CCJ_HD bool il_window(const TB &T, int kind, int p, int q, int u1, int u2, int &e) {
    const int w = q - p, rs = T.rs;
    if (kind == 0) {
        const int d = p + 1 + u1, dp = q - 1 - u2;
        if (!(u1 <= imin(w, MAXLOOP) - 2 && u2 <= imin(w - u1 - 6, MAXLOOP - 2) && T.pt[(dp - d) * rs + d] > 0)) return false;
        e = il_eint_raw(T, u1, u2, p, q);
    } else {
        const int d = p - 1 - u1, dp = q + 1 + u2;
        if (!(d >= 1 && dp <= T.n && T.pt[(dp - d) * rs + d] > 0)) return false;
        e = il_eint_raw(T, u1, u2, d, dp);
    }
    return true;
}

// the level kernel's (0,0) terms on the pair stacked inside (x,y): min(est, ie) of (x,y)
template <class TB>
CCJ_HD int il_stack00(const TB &T, int x, int y) {
    const int o = (y - x) * T.rs + x;
    return imin((int)T.est[o], (int)T.ie[o]);
}

// Is candidate (u1,u2), in the list of pair (p,q) with energy E, dominated?  Returns IL_NEAR | IL_FAR
// bits (0: keep).  v00 / e00: the window's (0,0) entry; vprev / eprev: its (u1-1, u2-1) entry (the
// same entry when u1 = u2 = 1).  Entries with an energy outside int16 (the fold fails with
// CCJ_E_PARAMS on them) never serve as a witness, and the extra E_IntLoop of the near intermediate
// raises no error of its own: out of range, it is no witness.
template <class TB>
CCJ_HD int il_dominated(const TB &T, int kind, int p, int q, int u1, int u2, int E, bool v00, int e00, bool vprev, int eprev) {
    if (u1 < 1 || u2 < 1 || !il_e_in_range(E)) return 0;
    // the candidate's pair, and the outer pair of each stacked couple
    const int d = kind ? p - 1 - u1 : p + 1 + u1, dp = kind ? q + 1 + u2 : q - 1 - u2;
    const int sN = kind ? il_stack00(T, p - 1, q + 1) : il_stack00(T, p, q);  // own pair <-> (0,0) entry
    const int sF = kind ? il_stack00(T, d, dp) : il_stack00(T, d - 1, dp + 1);  // candidate <-> (u1-1,u2-1) entry
    const bool one = u1 == 1 && u2 == 1;
    int bits = 0;
    if (vprev && il_e_in_range(eprev)) {
        const int E1 = one ? sN : eprev;
        if (E1 + sF <= E) bits |= IL_FAR;
    }
    if (v00 && il_e_in_range(e00)) {
        int E2 = sF;
        if (!one) {
            if (bits) return bits;  // already dropped: spare the evaluation
            // the loop between the (0,0) entry's pair and the candidate's pair: (u1-1, u2-1) unpaired
            E2 = kind ? il_eint_raw(T, u1 - 1, u2 - 1, d, dp) : il_eint_raw(T, u1 - 1, u2 - 1, p + 1, q - 1);
            if (!il_e_in_range(E2)) return bits;
        }
        if (sN + E2 <= E) bits |= IL_NEAR;
    }
    return bits;
}

// host view of one sequence's tables (ccj_il_prune_host)
struct IlHostTables {
    int n, rs;
    const short *S, *S1;
    const int8_t *pt, *pair, *rtype;
    const ccj_energy_params *prm;
    const int *lx;
    double e_intP;
    const int16_t *est, *ie;
};

}  // namespace ccj
