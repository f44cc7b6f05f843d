// ccj_pmpo2d.cc — host entry point of the closed forms in ccj_pmpo2d.h (no GPU): the six PM / PO
// multiloop matrices of every valid cell from a raw WBP alone.  tests/test_pmpo_closed_invariant.py
// holds them against the C restatement cell by cell.
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
