// ccj_pf_setup.h — per-sequence tables of the partition function as gathers.
//
// get_e_intP(i, j, k, l) = pow(exp_E_IntLoop(u1, u2, type, type2, si1, sj1, sp1, sq1), e_intP)
// (part_func.cc:886-891) depends on the sequence only through two pair types and four neighbour
// bases.  For A/C/G/U the pair type follows from its bases (1..6), so a weight that survives the
// mask (both pairs can pair) is one of at most 29 * 29 * 96 * 96 values: the key table, built once
// per context on the host with libm (ccj_pf.cc build_keytab) from the context's parameters,
// penalties and noGU.  The same holds for get_e_stP (:877-884): pow(expstack[type][type2], e_stP),
// 64 values (types 0..7, so also exact where a pair cannot pair).  The kernels of ccj_pf.hip and
// the host's keyed builder only gather through the functions below, so no pow is ever evaluated on
// the device and every weight is the host's double.
#pragma once
#include <stdint.h>

#include "ccj_pf_engine.h"

namespace ccj {

constexpr int PF_KEY_STEM = 96;  // (pair type 1..6, two neighbour bases 1..4)
constexpr long long PF_KEYS = (long long)PF_IEW * PF_IEW * PF_KEY_STEM * PF_KEY_STEM;

// Key of exp_E_IntLoop's arguments; type, type2 in 1..6, the four bases in 1..4, u1, u2 < PF_IEW.
CCJ_HD long long pf_ie_key(int u1, int u2, int type, int si1, int sj1, int type2, int sp1, int sq1) {
    const int k1 = (type - 1) * 16 + (si1 - 1) * 4 + (sj1 - 1), k2 = (type2 - 1) * 16 + (sp1 - 1) * 4 + (sq1 - 1);
    return ((long long)(u1 * PF_IEW + u2) * PF_KEY_STEM + k1) * PF_KEY_STEM + k2;
}

struct PfSeqView {
    int n, rs;
    const short *S;        // S == S1 on 1..n (encode_sequence)
    const int8_t *pair;    // 8x8
    const int8_t *rtype;   // 8
    const double *ietab;   // PF_KEYS doubles (pf_ie_key)
    const double *esttab;  // 64 doubles [type][type2]
    CCJ_HD int ptype(int i, int j) const { return pair[S[i] * 8 + S[j]]; }
};

// get_e_intP(i, j, k, l) for i < k < l < j inside 1..n with both pairs able to pair; false (a
// masked-out term) when one of them cannot.
CCJ_HD bool pf_ie_gather(const PfSeqView &v, int i, int j, int k, int l, double &w) {
    const int type = v.ptype(i, j), t2 = v.ptype(k, l);
    if (type <= 0 || t2 <= 0) return false;
    w = v.ietab[pf_ie_key(k - i - 1, j - l - 1, type, v.S[i + 1], v.S[j - 1], v.rtype[t2], v.S[k - 1], v.S[l + 1])];
    return true;
}

// Window entry (u1, u2) of the pair (p, p+w) as the closing pair (ieO / mO): the mask bit, and the
// weight when it is set.  The stack case u1 == u2 == 0 is 0 in get_e_intP.
CCJ_HD bool pf_ie_outer(const PfSeqView &v, int w, int p, int u1, int u2, double &wt) {
    const int q = p + w, ip = p + 1 + u1, jp = q - 1 - u2;
    if (p < 1 || q > v.n || ip >= jp || (u1 == 0 && u2 == 0)) return false;
    return pf_ie_gather(v, p, q, ip, jp, wt) && wt != 0.0;
}
// ... as the inner pair (ieI / mI) of the loop closed by (p-1-u1, p+w+1+u2)
CCJ_HD bool pf_ie_inner(const PfSeqView &v, int w, int p, int u1, int u2, double &wt) {
    const int d = p - 1 - u1, dp = p + w + 1 + u2;
    if (p < 1 || d < 1 || dp > v.n || (u1 == 0 && u2 == 0)) return false;
    return pf_ie_gather(v, d, dp, p, p + w, wt) && wt != 0.0;
}

// get_e_stP(p, p+w) as create builds it: 0 for w == 0, w == 2 and outside the triangle
CCJ_HD double pf_est_gather(const PfSeqView &v, int w, int p) {
    if (w < 1 || w == 2 || p < 1 || p + w > v.n) return 0.0;
    return v.esttab[v.ptype(p, p + w) * 8 + v.rtype[v.ptype(p + 1, p + w - 1)]];
}

// k_pf_iloop work items of level t (ccj_items.h's encoding, unsharded, 64-lane chunks): rows
// x < nPL + nPR as item_row's, then the PM rows, which start at h = 0 here (get_PMiloop has no
// hairpin bound on (j, k), part_func.cc:804-824): x - nPL - nPR = h * n + (j - 1).
CCJ_HD int pf_item_nrows(int n, int t) {
    const int m = n - t - 2;
    return 2 * imax(0, t - 5) * m + m * n;
}
template <class PT>
CCJ_HD int pf_item_row(const PT &pt, int n, int t, int x, uint32_t &it0) {
    const int m = n - t - 2, na = imax(0, t - 5);
    if (x < na * m) {
        const int a = 6 + x / m, i = 1 + x % m;
        it0 = (0u << 30) | ((uint32_t)a << 20) | ((uint32_t)i << 10);
        return pt(i, i + a) > 0 ? (m - i) / 64 + 1 : 0;
    }
    x -= na * m;
    if (x < na * m) {
        const int a = x / m, q = x % m, k = q + a + 3, b = t - a;
        it0 = (1u << 30) | ((uint32_t)a << 20) | ((uint32_t)q << 10);
        return pt(k, k + b) > 0 ? q / 64 + 1 : 0;
    }
    x -= na * m;
    const int h = x / n, j = 1 + x % n, k = j + h + 2;
    if (k > n) return 0;
    const int alo = imax(2, t - (n - k)), ahi = imin(t - 2, j - 1);
    if (alo > ahi || pt(j, k) <= 0) return 0;
    it0 = (2u << 30) | ((uint32_t)h << 20) | ((uint32_t)j << 10);
    return (ahi - alo) / 64 + 1;
}

// setup launches (ccj_pf.hip); v's pointers are device pointers
struct PfSetupDev {
    PfSeqView v;
    int8_t *pt;
    double *est, *ieO, *ieI;
    uint32_t *mO, *mI;
};

}  // namespace ccj

extern "C" {
int ccjk_pf_setup_tables(const ccj::PfSetupDev *T, void *stream);
// pass 0: counts[t * KI_SPLIT + s]; pass 1: items written from offs[t * KI_SPLIT + s]
int ccjk_pf_items(const ccj::PfSetupDev *T, long long *counts, const long long *offs, uint32_t *items, int pass, void *stream);
}
