// ccj_pmpo2d.cc — host entry points of the closed forms in ccj_pmpo2d.h (no GPU): the six PM / PO
// multiloop matrices of every valid cell from a raw WBP alone (tests/test_pmpo_closed_invariant.py
// holds them against the C restatement cell by cell), and their lowest pre-clamp values over the
// valid cells (the fill's range check; tests/test_range_cases.py).
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "ccj_pmpo2d.h"

using namespace ccj;

// wbp: raw WBP, row-major [(n+1) x (n+1)], entry i*(n+1)+j for 1 <= i <= j <= n.  out: for each of
// PMmloop00/01/10, POmloop00/01/10 (in that order) `cells` values, cell order i, j >= i, k >= j+2,
// l >= k ascending (l fastest).  Returns the number of cells per matrix, or -1.
extern "C" long long ccj_pmpo2d_closed(int n, const int *wbp, int bp, int cp, int16_t *out, long long cells) {
    if (n < 1 || !wbp) return -1;
    const int rs = n + 2;
    const long long N = (long long)(n + 1) * rs;
    std::vector<int> w2((size_t)N, INF + 1), tabs((size_t)(NCF * N), 0);
    for (int i = 1; i <= n; ++i)
        for (int j = i; j <= n; ++j) w2[(size_t)(j - i) * rs + i] = wbp[(size_t)i * (n + 1) + j];
    pmpo2d_host_tables(n, rs, cp, w2.data(), tabs.data(), N);
    const int *tp = tabs.data();
    auto tab = [=](int f, int p, int q) { return tp[f * N + (long long)(q - p) * rs + p]; };
    const int mats[6] = {PMmloop00, PMmloop01, PMmloop10, POmloop00, POmloop01, POmloop10};
    long long c = 0;
    for (int i = 1; i <= n; ++i)
        for (int j = i; j <= n; ++j)
            for (int k = j + 2; k <= n; ++k)
                for (int l = k; l <= n; ++l, ++c) {
                    if (!out) continue;
                    if (c >= cells) return -1;
                    for (int x = 0; x < 6; ++x) out[x * cells + c] = (int16_t)pmpo2d_eval(mats[x], bp, cp, tab, i, j, k, l);
                }
    return c;
}

// The lowest pre-clamp value of each of PMmloop00/01/10, POmloop00/01/10 (in that order) over the valid
// cells, from the same raw WBP (pmpo2d_low_host): below -32768 means the reference's int16 store of
// that matrix wraps somewhere (site CF).  INF where n has no valid cell.  Returns 0, or -1.
extern "C" int ccj_pmpo2d_low(int n, const int *wbp, int bp, int cp, int *out6) {
    if (n < 1 || !wbp || !out6) return -1;
    const int rs = n + 2;
    const long long N = (long long)(n + 1) * rs;
    std::vector<int> w2((size_t)N, INF + 1), tabs((size_t)(NCF * N), 0);
    for (int i = 1; i <= n; ++i)
        for (int j = i; j <= n; ++j) w2[(size_t)(j - i) * rs + i] = wbp[(size_t)i * (n + 1) + j];
    pmpo2d_host_tables(n, rs, cp, w2.data(), tabs.data(), N);
    const int *tp = tabs.data();
    pmpo2d_low_host(n, bp, cp, [=](int f, int p, int q) { return tp[f * N + (long long)(q - p) * rs + p]; }, out6);
    return 0;
}

// The same six minima cell by cell (tests): the minimum of pmpo2d_inner over the valid cells, O(n^4),
// or with valid_only = 0 over every pair of intervals 1 <= i <= j <= n, 1 <= k <= l <= n, whether or
// not they form a cell.  Returns 0; -1 on bad arguments; -2 if, at some valid cell, pmpo2d_inner
// clamped at 32767 is not pmpo2d_eval (the branch list would not be the formulas).
extern "C" int ccj_pmpo2d_low_brute(int n, const int *wbp, int bp, int cp, int valid_only, int *out6) {
    if (n < 1 || !wbp || !out6) return -1;
    const int rs = n + 2;
    const long long N = (long long)(n + 1) * rs;
    std::vector<int> w2((size_t)N, INF + 1), tabs((size_t)(NCF * N), 0);
    for (int i = 1; i <= n; ++i)
        for (int j = i; j <= n; ++j) w2[(size_t)(j - i) * rs + i] = wbp[(size_t)i * (n + 1) + j];
    pmpo2d_host_tables(n, rs, cp, w2.data(), tabs.data(), N);
    const int *tp = tabs.data();
    auto tab = [=](int f, int p, int q) { return tp[f * N + (long long)(q - p) * rs + p]; };
    const int mats[6] = {PMmloop00, PMmloop01, PMmloop10, POmloop00, POmloop01, POmloop10};
    for (int x = 0; x < 6; ++x) out6[x] = INF;
    for (int i = 1; i <= n; ++i)
        for (int j = i; j <= n; ++j)
            for (int k = valid_only ? j + 2 : 1; k <= n; ++k)
                for (int l = k; l <= n; ++l)
                    for (int x = 0; x < 6; ++x) {
                        const int v = pmpo2d_inner(x, bp, cp, tab, i, j, k, l);
                        if (k >= j + 2 && pmpo2d_cl(v) != pmpo2d_eval(mats[x], bp, cp, tab, i, j, k, l)) return -2;
                        out6[x] = imin(out6[x], v);
                    }
    return 0;
}
