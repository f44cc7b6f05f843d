// ccj_traceback.h — the traceback's node logic, written once for both executors.
//
// The reference's traceback is W_final::backtrack (W_final.cc:175-719) plus pseudo_loop::backtrack
// (pseudo_loop.cc:861-2820): nodes popped from a LIFO stack, each case an argmin with strict `<`
// (first minimum in loop order) followed by pushes and pair writes.  This header restates it, quirks
// included, in three layers, all plain C++ (CCJ_HD, no HIP include):
//
//   View<Store>      the reference getters (V, WM, WMv, WMp, P, WBP, WPP, WB, WP, the 4-D get with
//                    get_uc's assert, can_pair, compute_int, e_stP, e_intP) over a storage adaptor;
//   E_ext_Stem       W_final.cc:118-173, used by W (device k_w_terms, host compute_W) and by FREE;
//   Traceback<Exec>  one node: the dispatch, LOOP / FREE / M_WM / M_WMv / M_WMp, the P_* switch and
//                    the get_P?iloop / get_P?mloop values it needs.
//
// Every argmin is scan(count, f, bv, bx): f(c) is the value of candidate c, candidates numbered in
// the reference's loop order (BIG: no candidate at c), (bv, bx) the first minimum and its position.
// Loops the reference runs one after another are scanned one after another, each result compared
// strictly with the running minimum, so ties resolve as in the sequential code.
//
// A Store supplies (ccj_backtrack.hip DevStore over device memory, ccj_host.cc HostStore over the
// host mirror): n, S, S1, W; pr(i, j), rt(type), prm(), lx(), pen(), dangles(), est(), eint();
// raw2(which, i, j), Vtype(i, j), raw4(x, i, j, k, l) of a cell inside the matrix, pk(i, l).
// An Exec supplies: H (a View), st (the BtOut record), scan, scan2, push, setpair, pairup.  The
// device executor evaluates a scan's candidates across the lanes of a workgroup and reduces
// (value, position) lexicographically; the host executor walks them in order.  Neither holds any
// case of the algorithm.
#pragma once
#include <math.h>

#include "ccj_backtrack.h"
#include "ccj_energy.h"

namespace ccj {

constexpr int BIG = 0x7fffffff;  // "no candidate" in a scan

// 2-D arrays of the fill, in the order the engine stores them back to back
enum { A2_V = 0, A2_WM, A2_WMV, A2_WMP, A2_P, A2_WBP, A2_WPP, A2_WB, A2_WP, A2_N };

struct Int2 { int x, y; };  // what a scan2 candidate returns

template <class Store>
struct View : Store {
    mutable int bad = 0;  // Matrix4D::get_uc assert (matrices.hh:167) hit; the driver reads it after the node
    using Store::n;
    using Store::S1;
    using Store::pr;
    using Store::raw2;

    // s_energy_matrix.hh:37-43
    CCJ_HD int V(int i, int j) const { return i >= j ? INF : raw2(A2_V, i, j); }
    CCJ_HD int WM(int i, int j) const { return i >= j ? INF : raw2(A2_WM, i, j); }
    CCJ_HD int WMv(int i, int j) const { return i >= j ? INF : raw2(A2_WMV, i, j); }
    CCJ_HD int WMp(int i, int j) const { return i >= j ? INF : raw2(A2_WMP, i, j); }
    // TriangleMatrix::get (matrices.hh:38-41)
    CCJ_HD int Pg(int i, int j) const { return i > j ? INF : raw2(A2_P, i, j); }
    CCJ_HD int WBPg(int i, int j) const { return i > j ? INF : raw2(A2_WBP, i, j); }
    CCJ_HD int WPPg(int i, int j) const { return i > j ? INF : raw2(A2_WPP, i, j); }
    // pseudo_loop.cc:647-661
    CCJ_HD int WB(int i, int j) const {
        if (i <= 0 || j <= 0 || i > n || j > n) return INF;
        if (i > j) return 0;
        return imin(this->pen().cp * (j - i + 1), WBPg(i, j));
    }
    CCJ_HD int WP(int i, int j) const {
        if (i <= 0 || j <= 0 || i > n || j > n) return INF;
        if (i > j) return 0;
        return imin(this->pen().PUP * (j - i + 1), WPPg(i, j));
    }
    // Matrix4D::get (matrices.hh:177-182).  get_uc's assert is live in the reference build, so an
    // in-order but out-of-range cell aborts there: here it raises `bad` and reads nothing.
    CCJ_HD int g4(int x, int i, int j, int k, int l) const {
        if (!(i <= j && j < k - 1 && k <= l)) return INF;
        if (i <= 0 || l > n) {
            bad = 1;
            return INF;
        }
        return this->raw4(x, i, j, k, l);
    }
    CCJ_HD bool can_pair(int i, int j) const { return (j - i > TURN) && pr(i, j) > 0; }  // pseudo_loop.hh:131-135
    // pseudo_loop.cc:822-840 (lrint there; rint rounds the same, half to even, in the default mode)
    CCJ_HD int compute_int(int i, int j, int k, int l) const {
        return E_IntLoop(this->prm(), this->lx(), k - i - 1, j - l - 1, pr(i, j), this->rt(pr(k, l)), S1[i + 1], S1[j - 1],
                         S1[k - 1], S1[l + 1]);
    }
    CCJ_HD int e_stP(int i, int j) const {
        if (i + 1 == j - 1) return INF;
        return (int)rint(this->est() * (double)compute_int(i, j, i + 1, j - 1));
    }
    CCJ_HD int e_intP(int i, int ip, int jp, int j) const { return (int)rint(this->eint() * (double)compute_int(i, j, ip, jp)); }
};

// W_final.cc:118-173
template <class Store>
CCJ_HD int E_ext_Stem(const View<Store> &H, int vij, int vi1j, int vij1, int vi1j1, int i, int j) {
    const short *S = H.S;
    const int n = H.n, dangles = H.dangles();
    int e = INF, en;
    int tt = H.pr(i, j);
    en = vij;
    if (en != INF) {
        if (dangles == 2) en += E_ExtLoop(H.prm(), tt, i > 1 ? S[i - 1] : -1, j < n ? S[j + 1] : -1);
        else en += E_ExtLoop(H.prm(), tt, -1, -1);
        e = imin(e, en);
    }
    if (dangles == 1) {
        tt = H.pr(i + 1, j);
        en = (j - i - 1 > TURN) ? vi1j : INF;
        if (en != INF) en += E_ExtLoop(H.prm(), tt, S[i], -1);
        e = imin(e, en);
        tt = H.pr(i, j - 1);
        en = (j - 1 - i > TURN) ? vij1 : INF;
        if (en != INF) en += E_ExtLoop(H.prm(), tt, -1, S[j]);
        e = imin(e, en);
        tt = H.pr(i + 1, j - 1);
        en = (j - 1 - i - 1 > TURN) ? vi1j1 : INF;
        if (en != INF) en += E_ExtLoop(H.prm(), tt, S[i], S[j]);
        e = imin(e, en);
    }
    return e;
}

template <class Exec>
struct Traceback {
    Exec &x;
    decltype(Exec::H) H;  // const View<Store> &
    // the interior-loop argmin a P_PL / PR / PM / PO node computed with its get_P?iloop value, for
    // the P_P?iloop node it pushes (popped next); type 0: none
    struct IlCache { int type, i, j, k, l, bv, bx; };
    mutable IlCache ilc{0, 0, 0, 0, 0, 0, 0};

    CCJ_HD explicit Traceback(Exec &e) : x(e), H(e.H) {}

    CCJ_HD bool il_cached(int type, int i, int j, int k, int l, int &bv, int &bx) const {
        const bool hit = ilc.type == type && ilc.i == i && ilc.j == j && ilc.k == k && ilc.l == l;
        if (hit) {
            bv = ilc.bv;
            bx = ilc.bx;
        }
        ilc.type = 0;
        return hit;
    }

    CCJ_HD void push2(int i, int j, int type) { x.push(i, j, 0, 0, type); }
    // pseudo_loop::insert_node(i, j, k, l, type): fields i, j(=l of the region), k(=j), l(=k)
    CCJ_HD void push4(int i, int j, int k, int l, int type) { x.push(i, j, k, l, type); }
    CCJ_HD void pairup(int p, int q, int type) { x.pairup(p, q, type); }
    CCJ_HD void die(int prefix, int node) {
        x.st.status = BT_DIE;
        x.st.prefix = prefix;
        x.st.node = node;
    }
    CCJ_HD bool in_range4(int i, int j, int k, int l) const {
        const int n = H.n;
        return !(i <= 0 || j <= 0 || k <= 0 || l <= 0 || i > n || j > n || k > n || l > n);
    }
    CCJ_HD static bool order4(int i, int j, int k, int l) { return i <= j && j < k - 1 && k <= l; }

    // get_P?iloop (pseudo_loop.cc:682-808): the value takes pairable inner pairs only (.y); the
    // argmin its P_P?iloop node takes next over the same candidates has no can_pair filter (.x)
    CCJ_HD int get_PLiloop(int i, int j, int k, int l) const {
        if (!order4(i, j, k, l) || !H.can_pair(i, j)) return INF;
        int mn = INF;
        if (i + TURN + 2 < j) mn = H.g4(PL, i + 1, j - 1, k, l) + H.e_stP(i, j);
        const int nd = imin(j, i + MAXLOOP) - (i + 1);
        int fm, bv, bx;
        x.scan2(imax(nd, 0) * 32, [&](int c) {
            const int d = i + 1 + (c >> 5), dp = j - 1 - (c & 31);
            if (dp <= imax(d + TURN, j - MAXLOOP)) return Int2{BIG, BIG};
            const int v = H.e_intP(i, d, dp, j) + H.g4(PL, d, dp, k, l);
            return Int2{v, H.can_pair(d, dp) ? v : BIG};
        }, fm, bv, bx);
        ilc = IlCache{P_PLiloop, i, j, k, l, bv, bx};
        return imin(mn, fm);
    }
    CCJ_HD int get_PRiloop(int i, int j, int k, int l) const {
        if (!order4(i, j, k, l) || !H.can_pair(k, l)) return INF;
        int mn = INF;
        if (k + TURN + 2 < l) mn = H.g4(PR, i, j, k + 1, l - 1) + H.e_stP(k, l);
        const int nd = imin(l, k + MAXLOOP) - (k + 1);
        int fm, bv, bx;
        x.scan2(imax(nd, 0) * 32, [&](int c) {
            const int d = k + 1 + (c >> 5), dp = l - 1 - (c & 31);
            if (dp <= imax(d + TURN, l - MAXLOOP)) return Int2{BIG, BIG};
            const int v = H.e_intP(k, d, dp, l) + H.g4(PR, i, j, d, dp);
            return Int2{v, H.can_pair(d, dp) ? v : BIG};
        }, fm, bv, bx);
        ilc = IlCache{P_PRiloop, i, j, k, l, bv, bx};
        return imin(mn, fm);
    }
    CCJ_HD int get_PMiloop(int i, int j, int k, int l) const {
        if (!order4(i, j, k, l) || !H.can_pair(j, k)) return INF;
        int mn = INF;
        if (i < j && k < l) mn = H.g4(PM, i, j - 1, k + 1, l) + H.e_stP(j - 1, k + 1);
        const int nd = (j - 1) - imax(i, j - MAXLOOP);
        const int min_dp = imin(l, k + MAXLOOP);
        int fm, bv, bx;
        x.scan2(imax(nd, 0) * 32, [&](int c) {
            const int d = j - 1 - (c >> 5), dp = k + 1 + (c & 31);
            if (dp >= min_dp) return Int2{BIG, BIG};
            const int v = H.e_intP(d, j, k, dp) + H.g4(PM, i, d, dp, l);
            return Int2{v, H.can_pair(d, dp) ? v : BIG};
        }, fm, bv, bx);
        ilc = IlCache{P_PMiloop, i, j, k, l, bv, bx};
        return imin(mn, fm);
    }
    CCJ_HD int get_POiloop(int i, int j, int k, int l) const {
        if (!order4(i, j, k, l) || !H.can_pair(i, l)) return INF;
        int mn = INF;
        if (i < j && k < l) mn = H.g4(PO, i + 1, j, k, l - 1) + H.e_stP(i, l);
        const int nd = imin(j, i + MAXLOOP) - (i + 1);
        const int min_dp = imax(l - MAXLOOP, k);
        int fm, bv, bx;
        x.scan2(imax(nd, 0) * 32, [&](int c) {
            const int d = i + 1 + (c >> 5), dp = l - 1 - (c & 31);
            if (dp <= min_dp) return Int2{BIG, BIG};
            const int v = H.e_intP(i, d, dp, l) + H.g4(PO, d, j, dp, k);
            return Int2{v, H.can_pair(d, dp) ? v : BIG};
        }, fm, bv, bx);
        ilc = IlCache{P_POiloop, i, j, k, l, bv, bx};
        return imin(mn, fm);
    }
    // get_P?mloop (pseudo_loop.cc:705-820): validity of the outer cell, then min of the two
    CCJ_HD int get_PXmloop(int m10, int m01, int i2, int j2, int k2, int l2, int i, int j, int k, int l) const {
        if (!order4(i, j, k, l)) return INF;
        const int b1 = H.g4(m10, i2, j2, k2, l2) + H.pen().ap + H.pen().bp;
        const int b2 = H.g4(m01, i2, j2, k2, l2) + H.pen().ap + H.pen().bp;
        return imin(b1, b2);
    }

    // one node (W_final::backtrack W_final.cc:175-719)
    CCJ_HD void node(const Interval &cur) {
        switch (cur.type) {
            case LOOP: bt_loop(cur); break;
            case FREE: bt_free(cur); break;
            case M_WM: bt_wm(cur); break;
            case M_WMv: bt_wmv(cur); break;
            case M_WMp: bt_wmp(cur); break;
            case P_PK: case P_PL: case P_PR: case P_PM: case P_PO: case P_PfromL: case P_PfromR: case P_PfromM:
            case P_PfromO: case P_PLiloop: case P_PLiloop5: case P_PLmloop: case P_PLmloop00: case P_PLmloop01:
            case P_PLmloop10: case P_PRiloop: case P_PRiloop5: case P_PRmloop: case P_PRmloop00: case P_PRmloop01:
            case P_PRmloop10: case P_PMiloop: case P_PMiloop5: case P_PMmloop: case P_PMmloop00: case P_PMmloop01:
            case P_PMmloop10: case P_POiloop: case P_POiloop5: case P_POmloop: case P_POmloop00: case P_POmloop01:
            case P_POmloop10: case P_WB: case P_WBP: case P_WP: case P_WPP: case P_P:
                pl(cur);
                break;
            default:
                ++x.st.n_snbh;  // "Should not be here!" (A-B1: P_PfromMprime / P_PfromMdoubleprime)
        }
    }

    CCJ_HD void bt_loop(const Interval &cur) {
        const int i = cur.i, j = cur.j;
        if (i >= j) return;
        const int type = H.Vtype(i, j);
        x.setpair(i, j);
        if (type == T_HAIRP) {
            pairup(i, j, T_HAIRP);
        } else if (type == T_INTER) {
            pairup(i, j, T_INTER);
            // W_final.cc:198-226: k ascending, l descending, first strict minimum
            const int max_ip = imin(j - TURN - 2, i + MAXLOOP + 1);
            int bv, bx;
            x.scan(imax(max_ip - i, 0) * 32, [&](int c) {
                const int k = i + 1 + (c >> 5), l = j - 1 - (c & 31);
                const int min_l = imax(k + TURN + 1 + MAXLOOP + 2, k + j - i) - MAXLOOP - 2;
                if (l < min_l) return BIG;
                // s_energy_matrix::compute_int (:309-313): E_IntLoop + V(k,l)
                return E_IntLoop(H.prm(), H.lx(), k - i - 1, j - l - 1, H.pr(i, j), H.rt(H.pr(k, l)), H.S1[i + 1], H.S1[j - 1],
                                 H.S1[k - 1], H.S1[l + 1]) + H.V(k, l);
            }, bv, bx);
            int best_ip = j, best_jp = i;
            if (bv < INF) {
                best_ip = i + 1 + (bx >> 5);
                best_jp = j - 1 - (bx & 31);
            }
            if (best_ip < best_jp) push2(best_ip, best_jp, LOOP);
            else {
                x.st.status = BT_INTER;
                x.st.args[0] = i;
                x.st.args[1] = j;
                x.st.args[2] = best_ip;
                x.st.args[3] = best_jp;
            }
        } else if (type == T_MULTI) {
            pairup(i, j, T_MULTI);
            const short *S = H.S;
            const ccj_energy_params *P = H.prm();
            const int tt = H.pr(j, i);
            // W_final.cc:228-300: per k (ascending) rows 1..8 in order
            int bv, bx;
            x.scan(imax(j - 1 - i, 0) * 8, [&](int c) {
                const int k = i + 1 + (c >> 3), row = (c & 7) + 1;
                switch (row) {
                    case 1: return H.WM(i + 1, k - 1) + imin(H.WMv(k, j - 1), H.WMp(k, j - 1)) + E_MLstem(P, tt, -1, -1) + P->MLclosing;
                    case 2: return H.WM(i + 2, k - 1) + imin(H.WMv(k, j - 1), H.WMp(k, j - 1)) + E_MLstem(P, tt, -1, S[i + 1]) +
                                   P->MLclosing + P->MLbase;
                    case 3: return H.WM(i + 1, k - 1) + imin(H.WMv(k, j - 2), H.WMp(k, j - 2)) + E_MLstem(P, tt, S[j - 1], -1) +
                                   P->MLclosing + P->MLbase;
                    case 4: return H.WM(i + 2, k - 1) + imin(H.WMv(k, j - 2), H.WMp(k, j - 2)) + E_MLstem(P, tt, S[j - 1], S[i + 1]) +
                                   P->MLclosing + 2 * P->MLbase;
                    case 5: return (k - i - 1) * P->MLbase + H.WMp(k, j - 1) + E_MLstem(P, tt, -1, -1) + P->MLclosing;
                    case 6:  // the reference re-tests the previous tmp when the guard fails: no new candidate
                        if ((k - (i + 1) - 1) < 0) return BIG;
                        return (k - (i + 1) - 1) * P->MLbase + H.WMp(k, j - 1) + E_MLstem(P, tt, -1, S[i + 1]) + P->MLclosing + P->MLbase;
                    case 7: return (k - i - 1) * P->MLbase + H.WMp(k, j - 2) + E_MLstem(P, tt, S[j - 1], -1) + P->MLclosing + P->MLbase;
                    default:
                        if ((k - (i + 1) - 1) < 0) return BIG;
                        return (k - (i + 1) - 1) * P->MLbase + H.WMp(k, j - 2) + E_MLstem(P, tt, S[j - 1], S[i + 1]) + P->MLclosing +
                               2 * P->MLbase;
                }
            }, bv, bx);
            if (bv < INF) {
                const int best_k = i + 1 + (bx >> 3), best_row = (bx & 7) + 1;
                switch (best_row) {
                    case 1: push2(i + 1, best_k - 1, M_WM); push2(best_k, j - 1, M_WM); break;
                    case 2: push2(i + 2, best_k - 1, M_WM); push2(best_k, j - 1, M_WM); break;
                    case 3: push2(i + 1, best_k - 1, M_WM); push2(best_k, j - 2, M_WM); break;
                    case 4: push2(i + 2, best_k - 1, M_WM); push2(best_k, j - 2, M_WM); break;
                    case 5: push2(best_k, j - 1, M_WM); break;
                    case 6: push2(best_k, j - 1, M_WM); break;
                    case 7: push2(best_k, j - 2, M_WM); break;
                    case 8: push2(best_k, j - 2, M_WM); break;
                }
            }
        }
    }

    CCJ_HD void bt_free(const Interval &cur) {
        const int j = cur.j, n = H.n;
        if (j == 1) return;
        const short *S = H.S;
        const int dangles = H.dangles();
        const int *W = H.W;
        int mn = INF, best_row = -1, best_i = -1;
        if (W[j - 1] < mn) {
            mn = W[j - 1];
            best_row = 0;
        }
        // W_final.cc:316-360: i ascending, rows 1..4
        int bv, bx;
        x.scan((j - 1) * 4, [&](int c) {
            const int i = 1 + (c >> 2), row = (c & 3) + 1;
            const int acc = (i > 1) ? W[i - 1] : 0;
            if (row == 1) {
                const int eij = H.V(i, j);
                if (eij >= INF) return BIG;
                if (dangles == 2) return eij + E_ExtLoop(H.prm(), H.pr(i, j), i > 1 ? S[i - 1] : -1, j < n ? S[j + 1] : -1) + acc;
                return eij + E_ExtLoop(H.prm(), H.pr(i, j), -1, -1) + acc;
            }
            if (dangles != 1) return BIG;
            if (row == 2) {
                const int eij = H.V(i + 1, j);
                return eij < INF ? eij + E_ExtLoop(H.prm(), H.pr(i + 1, j), S[i], -1) + acc : BIG;
            }
            if (row == 3) {
                const int eij = H.V(i, j - 1);
                return eij < INF ? eij + E_ExtLoop(H.prm(), H.pr(i, j - 1), -1, S[j]) + acc : BIG;
            }
            const int eij = H.V(i + 1, j - 1);
            return eij < INF ? eij + E_ExtLoop(H.prm(), H.pr(i + 1, j - 1), S[i], S[j]) + acc : BIG;
        }, bv, bx);
        if (bv < mn) {
            mn = bv;
            best_i = 1 + (bx >> 2);
            best_row = (bx & 3) + 1;
        }
        // W_final.cc:362-395: P rows 5..8
        x.scan((j - 1) * 4, [&](int c) {
            const int i = 1 + (c >> 2), row = (c & 3) + 5;
            const int acc = (i - 1 > 0) ? W[i - 1] : 0;
            int eij;
            if (row == 5) eij = H.Pg(i, j);
            else if (dangles != 1) return BIG;
            else if (row == 6) eij = H.Pg(i + 1, j);
            else if (row == 7) eij = H.Pg(i, j - 1);
            else eij = H.Pg(i + 1, j - 1);
            return eij < INF ? eij + H.pen().PS + acc : BIG;
        }, bv, bx);
        if (bv < mn) {
            mn = bv;
            best_i = 1 + (bx >> 2);
            best_row = (bx & 3) + 5;
        }
        switch (best_row) {
            case 0: push2(1, j - 1, FREE); break;
            case 1: push2(best_i, j, LOOP); if (best_i - 1 > 1) push2(1, best_i - 1, FREE); break;
            case 2: push2(best_i + 1, j, LOOP); if (best_i >= 1) push2(1, best_i, FREE); break;
            case 3: push2(best_i, j - 1, LOOP); if (best_i - 1 > 1) push2(1, best_i - 1, FREE); break;
            case 4: push2(best_i + 1, j - 1, LOOP); if (best_i >= 1) push2(1, best_i, FREE); break;
            case 5: push2(best_i, j, P_P); if (best_i - 1 > 1) push2(1, best_i - 1, FREE); break;
            case 6: push2(best_i + 1, j, P_P); if (best_i >= 1) push2(1, best_i, FREE); break;
            case 7: push2(best_i, j - 1, P_P); if (best_i - 1 > 1) push2(1, best_i - 1, FREE); break;
            case 8: push2(best_i + 1, j - 1, P_P); if (best_i >= 1) push2(1, best_i, FREE); break;
        }
    }

    CCJ_HD void bt_wm(const Interval &cur) {
        const int i = cur.i, j = cur.j;
        const int MLb = H.prm()->MLbase;
        int mn = H.WM(i, j - 1) + MLb;
        int best_k = j, best_row = 5;
        // W_final.cc:408-440: k ascending, rows 1..4
        int bv, bx;
        x.scan(imax(j - TURN - i, 0) * 4, [&](int c) {
            const int k = i + (c >> 2), row = (c & 3) + 1;
            switch (row) {
                case 1: return (k - i) * MLb + H.WMv(k, j);
                case 2: return (k - i) * MLb + H.WMp(k, j);
                case 3: return H.WM(i, k - 1) + H.WMv(k, j);
                default: return H.WM(i, k - 1) + H.WMp(k, j);
            }
        }, bv, bx);
        if (bv < mn) {
            best_k = i + (bx >> 2);
            best_row = (bx & 3) + 1;
        }
        switch (best_row) {
            case 1: push2(best_k, j, M_WMv); break;
            case 2: push2(best_k, j, M_WMp); break;
            case 3: push2(i, best_k - 1, M_WM); push2(best_k, j, M_WMv); break;
            case 4: push2(i, best_k - 1, M_WM); push2(best_k + 1, j, M_WMp); break;  // A-B3
            case 5: push2(i, j - 1, M_WM); break;
        }
    }

    CCJ_HD void bt_wmv(const Interval &cur) {
        const int i = cur.i, j = cur.j, n = H.n;
        const short *S = H.S;
        const ccj_energy_params *P = H.prm();
        const int si = S[i], sj = S[j];
        const int si1 = (i > 1) ? S[i - 1] : -1;
        const int sj1 = (j < n) ? S[j + 1] : -1;
        int tt = H.pr(i, j);
        int mn = H.V(i, j) + ((H.dangles() == 2) ? E_MLstem(P, tt, si1, sj1) : E_MLstem(P, tt, -1, -1));
        int best_row = 1;
        if (H.dangles() == 1) {
            tt = H.pr(i + 1, j);
            int tmp = H.V(i + 1, j) + E_MLstem(P, tt, si, -1) + P->MLbase;
            if (tmp < mn) { mn = tmp; best_row = 2; }
            tt = H.pr(i, j - 1);
            tmp = H.V(i, j - 1) + E_MLstem(P, tt, -1, sj) + P->MLbase;
            if (tmp < mn) { mn = tmp; best_row = 3; }
            tt = H.pr(i + 1, j - 1);
            tmp = H.V(i + 1, j - 1) + E_MLstem(P, tt, si, sj) + 2 * P->MLbase;
            if (tmp < mn) { mn = tmp; best_row = 4; }
        }
        const int tmp = H.WMv(i, j - 1) + P->MLbase;
        if (tmp < mn) { mn = tmp; best_row = 5; }
        switch (best_row) {
            case 1: push2(i, j, LOOP); break;
            case 2: push2(i + 1, j, LOOP); break;
            case 3: push2(i, j - 1, LOOP); break;
            case 4: push2(i + 1, j - 1, LOOP); break;
            case 5: push2(i, j - 1, M_WMv); break;
        }
    }

    CCJ_HD void bt_wmp(const Interval &cur) {
        const int i = cur.i, j = cur.j;
        const int mn = H.Pg(i, j) + H.pen().PSM + H.pen().b;
        const int tmp = H.WMp(i, j - 1) + H.prm()->MLbase;
        if (tmp < mn) push2(i, j - 1, M_WMp);  // case 1 is commented out in the reference (A-B2)
    }

    // pseudo_loop::backtrack, pseudo_loop.cc:861-2820
    CCJ_HD void pl(const Interval &cur) {
        const auto &pe = H.pen();
        const int PB = pe.PB, bp = pe.bp, cp = pe.cp, ap = pe.ap, n = H.n;
        const int i = cur.i, l = cur.j, j = cur.k, k = cur.l;
        int bv, bx;
        switch (cur.type) {
            case P_P: {
                if (i >= l) return die(1, P_P);
                // first (j,d,k) in the reference loop order whose PK(i,j,d+1,k)+PK(j+1,d,k+1,l) is P(i,l)
                // (pseudo_loop.cc:867-896): k_pterm keeps it with the minimum (Pk)
                int best_d = 0, best_j = 0, best_k = 0;
                const int target = H.Pg(i, l);
                if (l - i >= 3 && target < INF / 2) {
                    const unsigned sig = (unsigned)(l - i), kk = H.pk(i, l);
                    best_j = i + (int)(kk / (sig * sig));
                    best_d = i + (int)((kk / sig) % sig);
                    best_k = i + (int)(kk % sig);
                }
                push4(i, best_k, best_j, best_d + 1, P_PK);
                push4(best_j + 1, l, best_d, best_k + 1, P_PK);
            } break;

            case P_PK: {
                if (!order4(i, j, k, l)) return die(2, P_PK);
                if (!in_range4(i, j, k, l)) return die(4, P_PK);
                int mn = INF, best_row = -1, best_d = -1;
                x.scan(imax(j - i - 1, 0), [&](int c) { const int d = i + 1 + c; return H.g4(PK, i, d, k, l) + H.WP(d + 1, j); }, bv, bx);
                if (bv < mn) { mn = bv; best_row = 1; best_d = i + 1 + bx; }
                x.scan(imax(l - k - 1, 0), [&](int c) { const int d = k + 1 + c; return H.g4(PK, i, j, d, l) + H.WP(k, d - 1); }, bv, bx);
                if (bv < mn) { mn = bv; best_row = 2; best_d = k + 1 + bx; }
                int tmp = H.g4(PL, i, j, k, l) + PB; if (tmp < mn) { mn = tmp; best_row = 3; best_d = -1; }
                tmp = H.g4(PM, i, j, k, l) + PB; if (tmp < mn) { mn = tmp; best_row = 4; best_d = -1; }
                tmp = H.g4(PR, i, j, k, l) + PB; if (tmp < mn) { mn = tmp; best_row = 5; best_d = -1; }
                tmp = H.g4(PO, i, j, k, l) + PB; if (tmp < mn) { mn = tmp; best_row = 6; best_d = -1; }
                switch (best_row) {
                    case 1: if (best_d > -1) { push4(i, l, best_d, k, P_PK); push2(best_d + 1, j, P_WP); } break;
                    case 2: if (best_d > -1) { push4(i, l, j, best_d, P_PK); push2(k, best_d - 1, P_WP); } break;
                    case 3: push4(i, l, j, k, P_PL); break;
                    case 4: push4(i, l, j, k, P_PM); break;
                    case 5: push4(i, l, j, k, P_PR); break;
                    case 6: push4(i, l, j, k, P_PO); break;
                }
            } break;

            case P_PL: {
                if (!order4(i, j, k, l)) return die(2, P_PL);
                if (!in_range4(i, j, k, l)) return die(4, P_PL);
                int mn = INF, tmp, best_row = -1;
                if (H.pr(i, j) > 0) {
                    tmp = get_PLiloop(i, j, k, l); if (tmp < mn) { mn = tmp; best_row = 1; }
                    tmp = get_PXmloop(PLmloop10, PLmloop01, i + 1, j - 1, k, l, i, j, k, l) + bp; if (tmp < mn) { mn = tmp; best_row = 2; }
                    if (j >= i + TURN + 1) { tmp = H.g4(PfromL, i + 1, j - 1, k, l); if (tmp < mn) { mn = tmp; best_row = 3; } }
                }
                switch (best_row) {
                    case 1: push4(i, l, j, k, P_PLiloop); break;
                    case 2: push4(i, l, j, k, P_PLmloop); break;
                    case 3: push4(i + 1, l, j - 1, k, P_PfromL); pairup(i, j, P_PL); break;
                }
            } break;

            case P_PR: {
                if (!order4(i, j, k, l)) return die(3, P_PR);
                if (i < 0 || j < 0 || k < 0 || l < 0 || i >= n || j >= n || k >= n || l >= n) return die(4, P_PR);  // A-B5
                int mn = INF, tmp, best_row = -1;
                if (H.pr(k, l) > 0) {
                    tmp = get_PRiloop(i, j, k, l); if (tmp < mn) { mn = tmp; best_row = 1; }
                    tmp = get_PXmloop(PRmloop10, PRmloop01, i, j, k + 1, l - 1, i, j, k, l) + bp; if (tmp < mn) { mn = tmp; best_row = 2; }
                    if (l >= k + TURN + 1) { tmp = H.g4(PfromR, i, j, k + 1, l - 1); if (tmp < mn) { mn = tmp; best_row = 3; } }
                }
                switch (best_row) {
                    case 1: push4(i, l, j, k, P_PRiloop); break;
                    case 2: push4(i, l, j, k, P_PRmloop); break;
                    case 3: push4(i, l - 1, j, k + 1, P_PfromR); pairup(k, l, P_PR); break;
                }
            } break;

            case P_PM: {
                if (!order4(i, j, k, l)) return die(2, P_PM);
                if (!in_range4(i, j, k, l)) return die(4, P_PM);
                if (i == j && k == l) { pairup(j, k, P_PM); return; }
                int mn = INF, tmp, best_row = -1;
                if (H.pr(j, k) > 0) {
                    tmp = get_PMiloop(i, j, k, l); if (tmp < mn) { mn = tmp; best_row = 1; }
                    tmp = get_PXmloop(PMmloop10, PMmloop01, i, j - 1, k + 1, l, i, j, k, l) + bp; if (tmp < mn) { mn = tmp; best_row = 2; }
                    if (k >= j + TURN - 1) { tmp = H.g4(PfromM, i, j - 1, k + 1, l); if (tmp < mn) { mn = tmp; best_row = 3; } }
                }
                switch (best_row) {
                    case 1: push4(i, l, j, k, P_PMiloop); break;
                    case 2: push4(i, l, j, k, P_PMmloop); break;
                    case 3: push4(i, l, j - 1, k + 1, P_PfromM); pairup(j, k, P_PM); break;
                }
            } break;

            case P_PO: {
                if (!order4(i, j, k, l)) return die(2, P_PO);
                if (!in_range4(i, j, k, l)) return die(4, P_PO);
                int mn = INF, tmp, best_row = -1;
                if (H.pr(i, l) > 0) {
                    tmp = get_POiloop(i, j, k, l); if (tmp < mn) { mn = tmp; best_row = 1; }
                    tmp = get_PXmloop(POmloop10, POmloop01, i + 1, j, k, l - 1, i, j, k, l) + bp; if (tmp < mn) { mn = tmp; best_row = 2; }
                    if (l >= i + TURN + 1) { tmp = H.g4(PfromO, i + 1, j, k, l - 1); if (tmp < mn) { mn = tmp; best_row = 3; } }
                }
                switch (best_row) {
                    case 1: push4(i, l, j, k, P_POiloop); break;
                    case 2: push4(i, l, j, k, P_POmloop); break;
                    case 3: push4(i + 1, l - 1, j, k, P_PfromO); pairup(i, l, P_PO); break;
                }
            } break;

            case P_PfromL: {
                if (!order4(i, j, k, l)) return die(0, P_PfromL);
                if (!in_range4(i, j, k, l)) return die(0, P_PfromL);
                if (i == j && k == l) return;
                int mn = INF, tmp, best_row = -1, best_d = -1;
                x.scan(imax(j - i - 1, 0) * 2, [&](int c) {
                    const int d = i + 1 + (c >> 1);
                    return (c & 1) ? H.g4(PfromL, i, d, k, l) + H.WP(d + 1, j) : H.g4(PfromL, d, j, k, l) + H.WP(i, d - 1);
                }, bv, bx);
                if (bv < mn) { mn = bv; best_row = (bx & 1) + 1; best_d = i + 1 + (bx >> 1); }
                tmp = H.g4(PR, i, j, k, l) + PB; if (tmp < mn) { mn = tmp; best_row = 3; best_d = -1; }
                tmp = H.g4(PM, i, j, k, l) + PB; if (tmp < mn) { mn = tmp; best_row = 4; best_d = -1; }
                tmp = H.g4(PO, i, j, k, l) + PB; if (tmp < mn) { mn = tmp; best_row = 5; best_d = -1; }
                switch (best_row) {
                    case 1: if (best_d > -1) { push4(best_d, l, j, k, P_PfromL); push2(i, best_d - 1, P_WP); } break;
                    case 2: if (best_d > -1) { push4(i, l, best_d, k, P_PfromL); push2(best_d + 1, j, P_WP); } break;
                    case 3: push4(i, l, j, k, P_PR); break;
                    case 4: push4(i, l, j, k, P_PM); break;
                    case 5: push4(i, l, j, k, P_PO); break;
                }
            } break;

            case P_PfromR: {
                if (!order4(i, j, k, l)) return die(0, P_PfromR);
                if (!in_range4(i, j, k, l)) return die(5, P_PfromR);
                if (i == j && k == l) return;
                int mn = INF, tmp, best_row = -1, best_d = -1;
                x.scan(imax(l - k - 1, 0) * 2, [&](int c) {
                    const int d = k + 1 + (c >> 1);
                    return (c & 1) ? H.g4(PfromR, i, j, k, d) + H.WP(d + 1, l) : H.g4(PfromR, i, j, d, l) + H.WP(k, d - 1);
                }, bv, bx);
                if (bv < mn) { mn = bv; best_row = (bx & 1) + 1; best_d = k + 1 + (bx >> 1); }
                tmp = H.g4(PM, i, j, k, l) + PB; if (tmp < mn) { mn = tmp; best_row = 3; best_d = -1; }
                tmp = H.g4(PO, i, j, k, l) + PB; if (tmp < mn) { mn = tmp; best_row = 4; best_d = -1; }
                switch (best_row) {
                    case 1: if (best_d > -1) { push4(i, l, j, best_d, P_PfromR); push2(k, best_d - 1, P_WP); } break;
                    case 2: if (best_d > -1) { push4(i, best_d, j, k, P_PfromR); push2(best_d + 1, l, P_WP); } break;
                    case 3: push4(i, l, j, k, P_PM); break;
                    case 4: push4(i, l, j, k, P_PO); break;
                }
            } break;

            case P_PfromM: {
                if (!order4(i, j, k, l)) return die(0, P_PfromM);
                if (!in_range4(i, j, k, l)) return die(0, P_PfromM);
                if (i == j && k == l) return;
                x.scan(imax(j - i - 1, 0), [&](int c) { const int d = i + 1 + c; return H.g4(PfromMprime, i, d, k, l) + H.WP(d + 1, j); }, bv, bx);
                if (bv < INF) {
                    const int best_d = i + 1 + bx;
                    push4(i, l, best_d, k, P_PfromMprime);
                    push2(best_d + 1, j, P_WP);
                }
            } break;

            case P_PfromO: {
                if (!order4(i, j, k, l)) return die(2, P_PfromO);
                if (!in_range4(i, j, k, l)) return die(5, P_PfromO);
                if (i == j && k == l) return;
                int mn = INF, tmp, best_row = -1, best_d = -1;
                x.scan(imax(j - i - 1, 0), [&](int c) { const int d = i + 1 + c; return H.g4(PfromO, d, j, k, l) + H.WP(i, d - 1); }, bv, bx);
                if (bv < mn) { mn = bv; best_row = 1; best_d = i + 1 + bx; }
                x.scan(imax(l - k - 1, 0), [&](int c) { const int d = k + 1 + c; return H.g4(PfromO, i, j, k, d) + H.WP(d + 1, l); }, bv, bx);
                if (bv < mn) { mn = bv; best_row = 2; best_d = k + 1 + bx; }
                tmp = H.g4(PL, i, j, k, l) + PB; if (tmp < mn) { mn = tmp; best_row = 3; best_d = -1; }
                tmp = H.g4(PR, i, j, k, l) + PB; if (tmp < mn) { mn = tmp; best_row = 4; best_d = -1; }
                switch (best_row) {
                    case 1: if (best_d > -1) { push4(best_d, l, j, k, P_PfromO); push2(i, best_d - 1, P_WP); } break;
                    case 2: if (best_d > -1) { push4(i, best_d, j, k, P_PfromO); push2(best_d + 1, l, P_WP); } break;
                    case 3: push4(i, l, j, k, P_PL); break;
                    case 4: push4(i, l, j, k, P_PR); break;
                }
            } break;

            case P_WB: {
                if (i <= 0 || l <= 0 || i > n || l > n) return die(4, P_WB);
                if (i > l) return;
                int mn = INF, best_row = -1;
                int tmp = H.WBPg(i, l); if (tmp < mn) { mn = tmp; best_row = 1; }
                tmp = cp * (l - i + 1); if (tmp < mn) { mn = tmp; best_row = 2; }
                if (best_row == 1) push2(i, l, P_WBP);
            } break;

            case P_WBP: {
                if (i > l) return die(1, P_WBP);
                if (i <= 0 || l <= 0 || i > n || l > n) return die(4, P_WBP);
                int mn = INF, best_row = -1, best_d = -1;
                x.scan((l - i) * 2, [&](int c) {
                    const int d = i + (c >> 1);
                    return (c & 1) ? H.WB(i, d - 1) + H.Pg(d, l) + pe.PSM + pe.PPS : H.WB(i, d - 1) + H.V(d, l) + bp + pe.PPS;
                }, bv, bx);
                if (bv < mn) { mn = bv; best_row = (bx & 1) + 1; best_d = i + (bx >> 1); }
                const int tmp = H.WBPg(i, l - 1) + cp;
                if (tmp < mn) { mn = tmp; best_row = 3; }
                switch (best_row) {
                    case 1: push2(i, best_d - 1, P_WB); push2(best_d, l, LOOP); break;
                    case 2: push2(i, best_d - 1, P_WB); push2(best_d, l, P_P); break;
                    case 3: push2(i, l - 1, P_WBP); break;
                }
            } break;

            case P_WP: {
                if (i <= 0 || l <= 0 || i > n || l > n) return die(4, P_WP);
                if (i > l) return;
                int mn = INF, best_row = -1;
                int tmp = H.WPPg(i, l); if (tmp < mn) { mn = tmp; best_row = 1; }
                tmp = pe.PUP * (l - i + 1); if (tmp < mn) { mn = tmp; best_row = 2; }
                if (best_row == 1) push2(i, l, P_WPP);
            } break;

            case P_WPP: {
                if (i > l) return die(1, P_WPP);
                if (i <= 0 || l <= 0 || i > n || l > n) return die(4, P_WPP);
                int mn = INF, best_row = -1, best_d = -1;
                x.scan((l - i) * 2, [&](int c) {
                    const int d = i + (c >> 1);
                    return (c & 1) ? H.WP(i, d - 1) + H.Pg(d, l) + pe.PSP + pe.PPS : H.WP(i, d - 1) + H.V(d, l) + 0 + pe.PPS;
                }, bv, bx);
                if (bv < mn) { mn = bv; best_row = (bx & 1) + 1; best_d = i + (bx >> 1); }
                const int tmp = H.WPPg(i, l - 1) + pe.PUP;
                if (tmp < mn) { mn = tmp; best_row = 3; }
                switch (best_row) {
                    case 1: push2(i, best_d - 1, P_WP); push2(best_d, l, LOOP); break;
                    case 2: push2(i, best_d - 1, P_WP); push2(best_d, l, P_P); break;
                    case 3: push2(i, l - 1, P_WPP); break;
                }
            } break;

            case P_PLiloop: {
                if (!(i < j && j < k - 1 && k < l)) return die(2, P_PLiloop);
                if (!in_range4(i, j, k, l)) return die(6, P_PLiloop);
                pairup(i, j, P_PLiloop);
                int mn = INF, best_row = -1, best_d = -1, best_dp = -1;
                if (H.pr(i, j) > 0) {
                    const int tmp = H.g4(PL, i + 1, j - 1, k, l) + H.e_stP(i, j);  // no i+TURN+2<j test here
                    if (tmp < mn) { mn = tmp; best_row = 1; }
                    const int nd = imin(j, i + MAXLOOP) - (i + 1);
                    if (!il_cached(P_PLiloop, i, j, k, l, bv, bx))
                        x.scan(imax(nd, 0) * 32, [&](int c) {  // d ascending, dp descending; no can_pair filter
                            const int d = i + 1 + (c >> 5), dp = j - 1 - (c & 31);
                            if (dp <= imax(d + TURN, j - MAXLOOP)) return BIG;
                            return H.e_intP(i, d, dp, j) + H.g4(PL, d, dp, k, l);
                        }, bv, bx);
                    if (bv < mn) { mn = bv; best_d = i + 1 + (bx >> 5); best_dp = j - 1 - (bx & 31); best_row = 2; }
                }
                switch (best_row) {
                    case 1: push4(i + 1, l, j - 1, k, P_PL); break;
                    case 2: push4(best_d, l, best_dp, k, P_PL); break;
                }
            } break;

            case P_PLmloop: {
                if (!order4(i, j, k, l)) return die(2, P_PLmloop);
                if (!in_range4(i, j, k, l)) return die(4, P_PLmloop);
                pairup(i, j, P_PLmloop);
                const int br1 = H.g4(PLmloop10, i + 1, j - 1, k, l) + ap + bp;
                const int br2 = H.g4(PLmloop01, i + 1, j - 1, k, l) + ap + bp;
                if (br1 < br2) push4(i + 1, l, j - 1, k, P_PLmloop10);
                else push4(i + 1, l, j - 1, k, P_PLmloop01);
            } break;

            case P_PLmloop00: {
                if (!order4(i, j, k, l)) return die(2, P_PLmloop00);
                if (!in_range4(i, j, k, l)) return die(4, P_PLmloop00);
                const int mn = H.g4(PL, i, j, k, l) + bp;
                x.scan((j - i + 1) * 2, [&](int c) {  // d ascending; row 2 (d > i) then row 3 (d < j)
                    const int d = i + (c >> 1);
                    if (!(c & 1)) return d > i ? H.WB(i, d - 1) + H.g4(PLmloop00, d, j, k, l) : BIG;
                    return d < j ? H.g4(PLmloop00, i, d, k, l) + H.WB(d + 1, j) : BIG;
                }, bv, bx);
                if (bv < mn) {
                    const int best_d = i + (bx >> 1);
                    if (!(bx & 1)) { push4(best_d, l, j, k, P_PLmloop00); push2(i, best_d - 1, P_WB); }
                    else { push4(i, l, best_d, k, P_PLmloop00); push2(best_d + 1, j, P_WB); }
                } else {
                    push4(i, l, j, k, P_PL);
                }
            } break;

            case P_PLmloop01: {
                if (!order4(i, j, k, l)) return die(2, P_PLmloop01);
                if (!in_range4(i, j, k, l)) return die(4, P_PLmloop01);
                x.scan(j - i, [&](int c) { const int d = i + c; return H.g4(PLmloop00, i, d, k, l) + H.WBPg(d + 1, j); }, bv, bx);
                const int best_d = bv < INF ? i + bx : -1;
                push4(i, l, best_d, k, P_PLmloop00);
                push2(best_d + 1, j, P_WBP);
            } break;

            case P_PLmloop10: {
                if (!order4(i, j, k, l)) return die(2, P_PLmloop10);
                if (!in_range4(i, j, k, l)) return die(4, P_PLmloop10);
                x.scan((j - i) * 2, [&](int c) {  // d = i+1..j; row 1, then row 2 if d < j
                    const int d = i + 1 + (c >> 1);
                    if (!(c & 1)) return H.WBPg(i, d - 1) + H.g4(PLmloop00, d, j, k, l);
                    return d < j ? H.g4(PLmloop10, i, d, k, l) + H.WB(d + 1, j) : BIG;
                }, bv, bx);
                if (bv < INF) {
                    const int best_d = i + 1 + (bx >> 1);
                    if (!(bx & 1)) { push2(i, best_d - 1, P_WBP); push4(best_d, l, j, k, P_PLmloop00); }
                    else { push4(i, l, best_d, k, P_PLmloop10); push2(best_d + 1, j, P_WB); }
                }
            } break;

            case P_PRiloop: {
                if (!order4(i, j, k, l)) return die(2, P_PRiloop);
                if (!in_range4(i, j, k, l)) return die(4, P_PRiloop);
                pairup(k, l, P_PRiloop);
                int mn = INF, best_row = -1, best_d = -1, best_dp = -1;
                if (H.pr(k, l) > 0) {
                    const int tmp = H.g4(PR, i, j, k + 1, l - 1) + H.e_stP(k, l);
                    if (tmp < mn) { mn = tmp; best_row = 1; }
                    const int nd = imin(l, k + MAXLOOP) - (k + 1);
                    if (!il_cached(P_PRiloop, i, j, k, l, bv, bx))
                        x.scan(imax(nd, 0) * 32, [&](int c) {
                            const int d = k + 1 + (c >> 5), dp = l - 1 - (c & 31);
                            if (dp <= imax(d + TURN, l - MAXLOOP)) return BIG;
                            return H.e_intP(k, d, dp, l) + H.g4(PR, i, j, d, dp);
                        }, bv, bx);
                    if (bv < mn) { mn = bv; best_d = k + 1 + (bx >> 5); best_dp = l - 1 - (bx & 31); best_row = 2; }
                }
                switch (best_row) {
                    case 1: push4(i, l - 1, j, k + 1, P_PR); break;
                    case 2: push4(i, best_dp, j, best_d, P_PR); break;
                }
            } break;

            case P_PRmloop: {
                if (!order4(i, j, k, l)) return die(2, P_PRmloop);
                if (!in_range4(i, j, k, l)) return die(4, P_PRmloop);
                pairup(k, l, P_PRmloop);
                const int br1 = H.g4(PRmloop10, i, j, k + 1, l - 1) + ap + bp;
                const int br2 = H.g4(PRmloop01, i, j, k + 1, l - 1) + ap + bp;
                if (br1 < br2) push4(i, l - 1, j, k + 1, P_PRmloop10);
                else push4(i, l - 1, j, k + 1, P_PRmloop01);
            } break;

            case P_PRmloop00: {
                if (!order4(i, j, k, l)) return die(2, P_PRmloop00);
                if (!in_range4(i, j, k, l)) return die(4, P_PRmloop00);
                const int mn = H.g4(PR, i, j, k, l) + bp;
                x.scan((l - k + 1) * 2, [&](int c) {
                    const int d = k + (c >> 1);
                    if (!(c & 1)) return d > k ? H.WB(k, d - 1) + H.g4(PRmloop00, i, j, d, l) : BIG;
                    return d < l ? H.g4(PRmloop00, i, j, k, d) + H.WB(d + 1, l) : BIG;
                }, bv, bx);
                if (bv < mn) {  // A-B4: (i,j,k,l) argument order
                    const int best_d = k + (bx >> 1);
                    if (!(bx & 1)) { push4(i, j, best_d, l, P_PRmloop00); push2(k, best_d - 1, P_WB); }
                    else { push4(i, j, k, best_d, P_PRmloop00); push2(best_d + 1, l, P_WB); }
                } else {
                    push4(i, j, k, l, P_PR);
                }
            } break;

            case P_PRmloop01: {
                if (!order4(i, j, k, l)) return die(2, P_PRmloop01);
                if (!in_range4(i, j, k, l)) return die(4, P_PRmloop01);
                const int mn = H.g4(PRmloop01, i, j, k, l - 1) + cp;
                x.scan(l - k, [&](int c) { const int d = k + c; return H.g4(PRmloop00, i, j, k, d) + H.WBPg(d + 1, l); }, bv, bx);
                if (bv < mn) {
                    const int best_d = k + bx;
                    push2(best_d + 1, l, P_WBP);
                    push4(i, best_d, j, k, P_PRmloop00);
                } else {
                    push4(i, l - 1, j, k, P_PRmloop01);
                }
            } break;

            case P_PRmloop10: {
                if (!order4(i, j, k, l)) return die(2, P_PRmloop10);
                if (!in_range4(i, j, k, l)) return die(4, P_PRmloop10);
                const int mn = H.g4(PRmloop10, i, j, k + 1, l) + cp;
                x.scan(l - k, [&](int c) { const int d = k + 1 + c; return H.WBPg(k, d - 1) + H.g4(PRmloop00, i, j, d, l); }, bv, bx);
                if (bv < mn) {
                    const int best_d = k + 1 + bx;
                    push2(k, best_d - 1, P_WBP);
                    push4(i, l, j, best_d, P_PRmloop00);
                } else {
                    push4(i, l, j, k + 1, P_PRmloop10);
                }
            } break;

            case P_PMiloop: {
                if (!order4(i, j, k, l)) return die(2, P_PMiloop);
                if (!in_range4(i, j, k, l)) return die(4, P_PMiloop);
                pairup(j, k, P_PMiloop);
                int mn = INF, best_d = -1, best_dp = -1, best_row = -1;
                if (H.pr(j, k) > 0) {
                    const int tmp = H.g4(PM, i, j - 1, k + 1, l) + H.e_stP(j - 1, k + 1);
                    if (tmp < mn) { mn = tmp; best_row = 1; }
                    const int nd = (j - 1) - imax(i, j - MAXLOOP);
                    const int min_dp = imin(l, k + MAXLOOP);
                    if (!il_cached(P_PMiloop, i, j, k, l, bv, bx))
                        x.scan(imax(nd, 0) * 32, [&](int c) {  // d descending, dp ascending
                            const int d = j - 1 - (c >> 5), dp = k + 1 + (c & 31);
                            if (dp >= min_dp) return BIG;
                            return H.e_intP(d, j, k, dp) + H.g4(PM, i, d, dp, l);
                        }, bv, bx);
                    if (bv < mn) { mn = bv; best_d = j - 1 - (bx >> 5); best_dp = k + 1 + (bx & 31); best_row = 2; }
                }
                switch (best_row) {
                    case 1: push4(i, l, j - 1, k + 1, P_PM); break;
                    case 2: push4(i, l, best_d, best_dp, P_PM); break;
                }
            } break;

            case P_PMmloop: {
                if (!order4(i, j, k, l)) return die(2, P_PMmloop);
                if (!in_range4(i, j, k, l)) return die(4, P_PMmloop);
                pairup(j, k, P_PMmloop);
                const int br1 = H.g4(PMmloop10, i, j - 1, k + 1, l) + ap + bp;
                const int br2 = H.g4(PMmloop01, i, j - 1, k + 1, l) + ap + bp;
                if (br1 < br2) push4(i, l, j - 1, k + 1, P_PMmloop10);
                else push4(i, l, j - 1, k + 1, P_PMmloop01);
            } break;

            case P_PMmloop00: {
                if (!order4(i, j, k, l)) return die(2, P_PMmloop00);
                if (!in_range4(i, j, k, l)) return die(4, P_PMmloop00);
                pairup(j, k, P_PMmloop);
                int mn = H.g4(PM, i, j, k, l) + bp, best_row = 1, best_d = -1;
                x.scan(j - i, [&](int c) { const int d = i + c; return H.WB(d + 1, j) + H.g4(PMmloop00, i, d, k, l); }, bv, bx);
                if (bv < mn) { mn = bv; best_row = 2; best_d = i + bx; }
                x.scan(l - k, [&](int c) { const int d = k + 1 + c; return H.g4(PMmloop00, i, j, d, l) + H.WB(k, d - 1); }, bv, bx);
                if (bv < mn) { mn = bv; best_row = 3; best_d = k + 1 + bx; }
                switch (best_row) {
                    case 1: push4(i, l, j, k, P_PM); break;
                    case 2: push4(i, l, best_d, k, P_PMmloop00); push2(best_d + 1, j, P_WB); break;
                    case 3: push4(i, l, j, best_d, P_PMmloop00); push2(k, best_d - 1, P_WB); break;
                }
            } break;

            case P_PMmloop01: {
                if (!order4(i, j, k, l)) return die(2, P_PMmloop01);
                if (!in_range4(i, j, k, l)) return die(4, P_PMmloop01);
                const int mn = H.g4(PMmloop01, i, j, k + 1, l) + cp;
                x.scan(l - k, [&](int c) { const int d = k + 1 + c; return H.g4(PMmloop00, i, j, d, l) + H.WBPg(k, d - 1); }, bv, bx);
                if (bv < mn) {
                    const int best_d = k + 1 + bx;
                    push4(i, l, j, best_d, P_PMmloop00);
                    push2(k, best_d - 1, P_WBP);
                } else {
                    push4(i, l, j, k + 1, P_PMmloop01);
                }
            } break;

            case P_PMmloop10: {
                if (!order4(i, j, k, l)) return die(2, P_PMmloop10);
                if (!in_range4(i, j, k, l)) return die(4, P_PMmloop10);
                const int mn = H.g4(PMmloop10, i, j - 1, k, l) + cp;
                x.scan(imax(j - i - 1, 0), [&](int c) { const int d = i + 1 + c; return H.WBPg(d, j) + H.g4(PMmloop00, i, d - 1, k, l); }, bv, bx);
                if (bv < mn) {
                    const int best_d = i + 1 + bx;
                    push4(i, l, best_d - 1, k, P_PMmloop00);
                    push2(best_d, j, P_WBP);
                } else {
                    push4(i, l, j - 1, k, P_PMmloop10);
                }
            } break;

            case P_POiloop: {
                if (!in_range4(i, j, k, l)) return die(4, P_POiloop);
                if (!order4(i, j, k, l)) return die(2, P_POiloop);
                pairup(i, l, P_POiloop);
                int mn = INF, best_d = -1, best_dp = -1, best_row = -1;
                if (H.pr(i, l) > 0) {
                    const int tmp = H.g4(PO, i + 1, j, k, l - 1) + H.e_stP(i, l);
                    if (tmp < mn) { mn = tmp; best_row = 1; }
                    const int nd = imin(j, i + MAXLOOP) - (i + 1);
                    const int min_dp = imax(l - MAXLOOP, k);
                    if (!il_cached(P_POiloop, i, j, k, l, bv, bx))
                        x.scan(imax(nd, 0) * 32, [&](int c) {  // reads PO(d,j,dp,k) with dp > k: always INF (A-Q5)
                            const int d = i + 1 + (c >> 5), dp = l - 1 - (c & 31);
                            if (dp <= min_dp) return BIG;
                            return H.e_intP(i, d, dp, l) + H.g4(PO, d, j, dp, k);
                        }, bv, bx);
                    if (bv < mn) { mn = bv; best_row = 2; best_d = i + 1 + (bx >> 5); best_dp = l - 1 - (bx & 31); }
                }
                switch (best_row) {
                    case 1: push4(i + 1, l - 1, j, k, P_PO); break;
                    case 2: push4(best_d, k, j, best_dp, P_PO); break;
                }
            } break;

            case P_POmloop: {
                if (!order4(i, j, k, l)) return die(2, P_POmloop);
                if (!in_range4(i, j, k, l)) return die(4, P_POmloop);
                pairup(i, l, P_POmloop);
                const int br1 = H.g4(POmloop10, i + 1, j, k, l - 1) + ap + bp;
                const int br2 = H.g4(POmloop01, i + 1, j, k, l - 1) + ap + bp;
                if (br1 < br2) push4(i + 1, l - 1, j, k, P_POmloop10);
                else push4(i + 1, l - 1, j, k, P_POmloop01);
            } break;

            case P_POmloop00: {
                if (!order4(i, j, k, l)) return die(2, P_POmloop00);
                if (!in_range4(i, j, k, l)) return die(4, P_POmloop00);
                int mn = H.g4(PO, i, j, k, l) + bp, best_row = 1, best_d = -1;
                x.scan(j - i, [&](int c) { const int d = i + 1 + c; return H.WB(i, d - 1) + H.g4(POmloop00, d, j, k, l); }, bv, bx);
                if (bv < mn) { mn = bv; best_row = 2; best_d = i + 1 + bx; }
                x.scan(l - k, [&](int c) { const int d = k + c; return H.g4(POmloop00, i, j, k, d) + H.WB(d + 1, l); }, bv, bx);
                if (bv < mn) { mn = bv; best_row = 3; best_d = k + bx; }
                switch (best_row) {
                    case 1: push4(i, l, j, k, P_PO); break;
                    case 2: push4(best_d, l, j, k, P_POmloop00); push2(i, best_d - 1, P_WBP); break;  // sic
                    case 3: push4(i, best_d, j, k, P_POmloop00); push2(best_d + 1, l, P_WB); break;
                }
            } break;

            case P_POmloop01: {
                if (!order4(i, j, k, l)) return die(2, P_POmloop01);
                if (!in_range4(i, j, k, l)) return die(4, P_POmloop01);
                x.scan(l - k, [&](int c) { const int d = k + c; return H.g4(POmloop00, i, j, k, d) + H.WBPg(d + 1, l); }, bv, bx);
                const int best_d = bv < INF ? k + bx : -1;
                push4(i, best_d, j, k, P_POmloop00);
                push2(best_d + 1, l, P_WBP);
            } break;

            case P_POmloop10: {
                if (!order4(i, j, k, l)) return die(2, P_POmloop10);
                if (!in_range4(i, j, k, l)) return die(4, P_POmloop10);
                int mn = INF, best_row = -1, best_d = -1;
                x.scan(j - i, [&](int c) { const int d = i + 1 + c; return H.WBPg(i, d - 1) + H.g4(POmloop00, d, j, k, l); }, bv, bx);
                if (bv < mn) { mn = bv; best_row = 1; best_d = i + 1 + bx; }
                x.scan(imax(l - k - 1, 0), [&](int c) { const int d = k + 1 + c; return H.g4(POmloop10, i, j, k, d) + H.WB(d + 1, l); }, bv, bx);
                if (bv < mn) { mn = bv; best_row = 2; best_d = k + 1 + bx; }
                switch (best_row) {
                    case 1: push4(best_d, l, j, k, P_POmloop00); push2(i, best_d - 1, P_WBP); break;
                    case 2: push4(i, best_d, j, k, P_POmloop10); push2(best_d + 1, l, P_WB); break;
                }
            } break;

            default:
                break;  // P_PLiloop5 etc.: no case in pseudo_loop::backtrack
        }
    }
};

}  // namespace ccj
