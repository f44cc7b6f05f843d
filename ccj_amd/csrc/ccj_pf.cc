// ccj_pf.cc — host side of the CCJ partition function (include/ccj_pf.h).
//
// Builds the Boltzmann tables the way the reference's W_final_pf constructor gets them
// (part_func.cc:31-93: scale_pf_parameters() -> get_scaled_exp_params, params.c:558-738;
// rescale_pk_globals :127-146; exp_params_rescale :97-125), the per-sequence weight tables
// (HairpinE :214-220 with the special-hairpin strstr cases, get_e_stP / get_e_intP :877-891, which
// call pow()), drives the level-synchronous fill of ccj_pf.hip, then runs W (:163-172) and the
// stochastic traceback (stoch_backtrack.cc:36-326) on the host over the 2-D matrices.
// A context serves many sequences (ccj_pf_create_cap / ccj_pf_rebind / ccj_pf_reset): the pow()
// values are tabulated once per context by their arguments (ccj_pf_setup.h) and the per-sequence
// tables are gathered from them by kernels; CCJ_PF_HOST_SETUP=1 keeps the direct host builder.
// A lockstep batch (ccj_pf_batch_*) fills K such contexts with one event graph: one launch per level
// or span for all of them (the k_pf_*_many entries of ccj_pf.hip).
//
// Everything here is evaluated as written, without floating-point contraction, with the host
// libm — the same exp/log/pow/sin the reference links — so the device only ever multiplies and
// adds table values and the results are bit-identical to part_func.cc (-ffp-contract=off).
//
// Raw INF entries.  get_scaled_exp_params reads the raw 37 C tables, in which some dangles /
// multiloop and exterior mismatches are INF (SMOOTH turns INF into a weight of 1).  The
// ccj_energy_params blob holds the MFE tables, where those entries are clamped to 0
// (params.c:487-512), so the raw tables come separately (ccj_pf_raw, the .pfraw files).  Without
// them the pair type 0 rows are taken as INF — true for every parameter file the reference ships;
// its other raw-INF entries (the 'N' column, pair type 7) are unreachable for A/C/G/U sequences.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/ccj_pf.h"
#include "ccj_pf_energy.h"
#include "ccj_pf_engine.h"
#include "ccj_items.h"
#include "ccj_pf_setup.h"

using namespace ccj;

namespace {

constexpr double K0 = 273.15, GASCONST = 1.98717;  // params/constants.h:13-15

const int BP_PAIR_PF[8][8] = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 5, 0, 0, 5}, {0, 0, 0, 1, 0, 0, 0, 0},
                              {0, 0, 2, 0, 3, 0, 0, 0}, {0, 6, 0, 4, 0, 0, 0, 6}, {0, 0, 0, 0, 0, 0, 2, 0},
                              {0, 0, 0, 0, 0, 1, 0, 0}, {0, 6, 0, 0, 5, 0, 0, 0}};  // pair_mat.h:20-29

uint64_t fnv_init() { return 1469598103934665603ull; }
void fnv_bytes(uint64_t &h, const void *p, size_t n) {
    const unsigned char *c = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i) {
        h ^= c[i];
        h *= 1099511628211ull;
    }
}
template <class T>
uint64_t fnv_arr(const T *p, size_t cnt) {
    uint64_t h = fnv_init();
    fnv_bytes(h, p, cnt * sizeof(T));
    return h;
}

// RESCALE_BF (params.c:66-72) at 37 C: RESCALE_dG is the identity (dT == 1.0) and pf_smooth == 1
// makes TRUNC_MAYBE the identity.
double bf(double kT, int dG) { return exp(-(double)dG * 10. / kT); }
// RESCALE_BF_SMOOTH (params.c:39-45, 74-82), SCALE == 10
double bf_smooth(double kT, int dG) {
    const double X = -(double)dG;
    double s;
    if (X / 10 < -1.2283697) s = 0;
    else if (X / 10 > 0.8660254) s = X;
    else s = 10 * 0.38490018 * (sin(X / 10 - 0.34242663) + 1) * (sin(X / 10 - 0.34242663) + 1);
    return exp(s * 10. / kT);
}

void build_exp(const ccj_energy_params &p, const ccj_pf_raw *raw, const ccj_pk_penalties &k, PfExp &E) {
    memset(&E, 0, sizeof E);
    const double kT = 1. * (37. + K0) * GASCONST;  // betaScale * (temperature + K0) * GASCONST
    E.kT = kT;
    E.pf_scale = 1.;  // exp_params_rescale forces 1 (part_func.cc:107)
    E.lxc = p.lxc * 1.0;
    E.TermAU = bf(kT, p.TerminalAU);
    E.MLbase = bf(kT, p.MLbase);
    E.MLclosing = bf(kT, p.MLclosing);
    for (int i = 0; i < 31; ++i) E.hairpin[i] = bf(kT, p.hairpin[i]);
    double internal[31];
    for (int i = 0; i <= 30; ++i) {
        E.bulge[i] = bf(kT, p.bulge[i]);
        internal[i] = bf(kT, p.internal_loop[i]);
    }
    internal[2] = exp(-80 * 10. / kT);  // james_rule (params.c:609-610)
    for (int j = 0; j <= 30; ++j) {
        const double GT = (double)p.ninio2;
        E.ninio[j] = exp(-(p.max_ninio < j * GT ? (double)p.max_ninio : j * GT) * 10. / kT);
    }
    const int ntetra = (int)strnlen(p.Tetraloops, sizeof p.Tetraloops);
    for (int i = 0; i * 7 < ntetra && i < 40; ++i) E.tetra[i] = bf(kT, p.Tetraloop_E[i]);
    const int ntri = (int)strnlen(p.Triloops, sizeof p.Triloops);
    for (int i = 0; i * 5 < ntri && i < 40; ++i) E.tri[i] = bf(kT, p.Triloop_E[i]);
    const int nhex = (int)strnlen(p.Hexaloops, sizeof p.Hexaloops);
    for (int i = 0; i * 9 < nhex && i < 40; ++i) E.hex[i] = bf(kT, p.Hexaloop_E[i]);
    for (int i = 0; i < 8; ++i) E.MLintern[i] = bf(kT, p.MLintern[1]);  // one ML_intern37 for every type
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 5; ++j) {
            E.dangle5[i][j] = bf_smooth(kT, raw ? raw->dangle5[i][j] : i == 0 ? CCJ_INF : p.dangle5[i][j]);
            E.dangle3[i][j] = bf_smooth(kT, raw ? raw->dangle3[i][j] : i == 0 ? CCJ_INF : p.dangle3[i][j]);
        }
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j) E.stack[i][j] = bf(kT, p.stack[i][j]);
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 5; ++j)
            for (int q = 0; q < 5; ++q) {
                E.mismatchI[i][j][q] = bf(kT, p.mismatchI[i][j][q]);
                E.mismatch1nI[i][j][q] = bf(kT, p.mismatch1nI[i][j][q]);
                E.mismatchH[i][j][q] = bf(kT, p.mismatchH[i][j][q]);
                E.mismatch23I[i][j][q] = bf(kT, p.mismatch23I[i][j][q]);
                E.mismatchM[i][j][q] = bf_smooth(kT, raw ? raw->mismatchM[i][j][q] : i == 0 ? CCJ_INF : p.mismatchM[i][j][q]);
                E.mismatchExt[i][j][q] =
                    bf_smooth(kT, raw ? raw->mismatchExt[i][j][q] : i == 0 ? CCJ_INF : p.mismatchExt[i][j][q]);
            }
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j)
            for (int a = 0; a < 5; ++a)
                for (int b = 0; b < 5; ++b) {
                    E.int11[i][j][a][b] = bf(kT, p.int11[i][j][a][b]);
                    for (int c = 0; c < 5; ++c) {
                        E.int21[i][j][a][b][c] = bf(kT, p.int21[i][j][a][b][c]);
                        for (int d = 0; d < 5; ++d) E.int22[i][j][a][b][c][d] = bf(kT, p.int22[i][j][a][b][c][d]);
                    }
                }
    // expinternal[0..30] and the 26 doubles that follow it in vrna_exp_param_t (basic.h:127-128)
    for (int i = 0; i <= 30; ++i) E.internal57[i] = internal[i];
    for (int i = 31; i < 57; ++i) E.internal57[i] = (&E.mismatchExt[0][0][0])[i - 31];
    // rescale_pk_globals: RESCALE_BF(x, 3x, TT, kT) == exp(-x*10/kT) at 37 C
    E.PS = bf(kT, k.PS);
    E.PSM = bf(kT, k.PSM);
    E.PSP = bf(kT, k.PSP);
    E.PB = bf(kT, k.PB);
    E.PUP = bf(kT, k.PUP);
    E.PPS = bf(kT, k.PPS);
    E.a = bf(kT, k.a);
    E.b = bf(kT, k.b);
    E.c = bf(kT, k.c);
    E.ap = bf(kT, k.ap);
    E.bp = bf(kT, k.bp);
    E.cp = bf(kT, k.cp);
}

const char *const kExpNames =
    "expstack exphairpin expbulge expinternal expninio expmismatchI expmismatch1nI expmismatch23I expmismatchH "
    "expmismatchM expmismatchExt expdangle5 expdangle3 expint11 expint21 expint22 expMLintern scalars exptetra exptri "
    "exphex pk";
constexpr int kNExp = 22;

}  // namespace

struct ccj_pf_ctx {
    // a lockstep batch's member (ccj_pf_batch): st is the batch's stream and the model's device tables
    // (d_E, d_pair, d_rtype, d_mlb, d_cpp, d_pup, d_ietab, d_esttab) are the batch's, all borrowed; it
    // has no streams, events or timing of its own, and only the batch binds, fills and frees it
    ccj_pf_batch *batch = nullptr;
    int n = 0, rs = 0, dangles = 2, device = 0;
    int cap = 0;     // capacity N: every buffer holds any length 1..N (ccj_pf_create_cap)
    int noGU = 0;
    std::string seq;
    ccj_energy_params prm{};
    ccj_pk_penalties pen{};
    int pair[8][8]{};
    int rtype[8]{};
    std::vector<short> S, S1;
    PfExp E{};
    std::vector<double> mlb, cpp, pup;  // powers up to the capacity
    std::vector<PfLvl> lv;
    long long cells = 0;  // cells of one 4-D matrix
    long long offx = 0, offm = 0;  // bound extents of d_cx / d_pmx (ints)
    // key tables (ccj_pf_setup.h): built once per context, gathered by every sequence setup
    double *d_ietab = nullptr, *d_esttab = nullptr;
    double esttab[64]{};
    double keytab_ms = 0;
    long long *d_icount = nullptr, *d_ioff = nullptr;  // k_pf_items: items per (level, split), first item
    long long items_cap = 0;                           // d_items holds this many
    // pinned staging of the asynchronous uploads / the item counts; reused only after the wait of
    // the setup that filled it (setup_seq)
    short *h_S = nullptr;       // S then S1, cap+2 each
    double *h_hp = nullptr;     // [w][p] HairpinE of the bound sequence
    PfLvl *h_lv = nullptr;
    long long *h_icount = nullptr, *h_ioff = nullptr;
    // device
    PfExp *d_E = nullptr;
    short *d_S = nullptr, *d_S1 = nullptr;
    int8_t *d_pt = nullptr, *d_pair = nullptr, *d_rtype = nullptr;
    double *d_hp = nullptr, *d_est = nullptr, *d_ieO = nullptr, *d_ieI = nullptr, *d_mlb = nullptr, *d_cpp = nullptr, *d_pup = nullptr;
    double *d_2d = nullptr;  // CCJ_PF_NMAT2 planes of (n+1)*rs
    long long *d_Pacc = nullptr;
    unsigned long long *d_Pabs = nullptr;
    int *d_d4 = nullptr;
    int *d_prec = nullptr;  // split-loop operand records (PfDev::r1 .. r4)
    int *d_cx = nullptr, *d_pmx = nullptr;  // k_pf_iloop's copies of PL / PR and PM (ccj_pf_engine.h)
    double *d_R = nullptr;                  // k_pf_iloop's sums of one level, 3 planes of max C_t
    uint32_t *d_items = nullptr, *d_mO = nullptr, *d_mI = nullptr;
    std::vector<long long> ifirst;          // k_pf_iloop items of level t: [ifirst[t], ifirst[t+1])
    bool setup_pending = false;             // between setup_seq_a and setup_seq_b
    std::vector<uint32_t> h_items, h_mO, h_mI;  // host copies (ccj_pf_work_model)
    PfLvl *d_ld = nullptr;
    hipStream_t st = nullptr;     // levels (k_pf_level), the memsets, the result copies
    hipStream_t st_il = nullptr;  // k_pf_iloop(t): after level t-2
    hipStream_t st_d = nullptr;   // k_pf_ppush(s-3) (P of span s), k_pf_diag(s): after level s-3
    std::vector<hipEvent_t> ev_lev, ev_il, ev_dg;  // level t done, iloop t done, span s done
    hipEvent_t ev_start = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    PfDev D{};
    // results
    bool filled = false;
    std::vector<double> h2d;  // host copies of the 2-D planes
    std::vector<double> W;
    double energy = 0;
    float fill_ms = 0;
    // per-kernel-family timing (ccj_pf_set_timing): an event pair around every launch
    bool timing = false;
    std::vector<hipEvent_t> tev;
    std::vector<int> tfam;      // family of launch q: 0 k_pf_iloop, 1 k_pf_level, 2 P terms (k_pf_ppush / k_pf_pterm), 3 k_pf_diag
    double kms[4] = {0, 0, 0, 0};
    std::string msg;
    // vrna_urn() of the reference build: rand() / RAND_MAX (utils.c:262-271, no HAVE_ERAND48), on
    // this context's own glibc random_r state (a fresh one behaves like a process that never
    // called srand, i.e. srand(1))
    struct random_data rnd {};
    char rnd_state[128]{};

    size_t plane() const { return (size_t)(n + 1) * rs; }
    double g2(int m, int i, int j) const { return i > j ? 0.0 : h2d[(size_t)m * plane() + (size_t)(j - i) * rs + i]; }
    int ptype(int i, int j) const { return pair[S[i]][S[j]]; }
};

// A lockstep batch: `model` holds what the members share (the model's host and device tables, the
// main stream) and the one fill graph (its streams and events, sized for the capacity); it is never
// bound to a sequence.  mem[k] are capacity contexts that borrow from it (ccj_pf_ctx::batch).
struct ccj_pf_batch {
    ccj_pf_ctx model;
    std::vector<ccj_pf_ctx *> mem;
    int count = 0, nmax = 0;      // bound members; the longest of them
    std::vector<int> n;           // their lengths
    std::vector<int> rc;          // each member's outcome of the last fill
    PfDev *d_D = nullptr, *h_D = nullptr;          // the bound members' PfDev (device; pinned staging)
    long long *d_if = nullptr, *h_if = nullptr;    // k_pf_iloop_many's table: row k = member k's ifirst[]
    int stride = 0;                                // its row length (capacity + 1)
    int launches = 0;
    std::string msg;
};

// The allocations of ccj_pf_create for a sequence of length n, in bytes: device (every hipMalloc
// of create_impl; the work items, sequence-dependent, by their count when every pair can pair) and host (the two get_e_intP window tables, built before they are uploaded).
// The items' upper bound of ccj_pf_footprint alone.  It grows with n (a longer sequence adds rows
// to every level and levels on top), so the bound at the capacity covers every shorter length.
static unsigned long long pf_items_bound(int n) {
    unsigned long long rows = 0;
    for (int t = 0; t <= n - 3; ++t) {
        const int mi = n - t - 2;
        for (int i = 1; i <= mi; ++i) rows += (unsigned long long)std::max(0, t - 5) * ((mi - i) / 64 + 1);
        for (int q = 0; q < mi; ++q) rows += (unsigned long long)std::max(0, t - 5) * (q / 64 + 1);
        for (int h = 0; h <= mi - 1; ++h)
            for (int j = 1; j + h + 2 <= n; ++j) {
                const int k = j + h + 2, alo = std::max(2, t - (n - k)), ahi = std::min(t - 2, j - 1);
                if (alo <= ahi) rows += (unsigned long long)((ahi - alo) / 64 + 1);
            }
    }
    return rows;
}

extern "C" void ccj_pf_footprint(int n, unsigned long long *device_bytes, unsigned long long *host_bytes) {
    if (n < 1) n = 1;
    const unsigned long long rs = (unsigned long long)n + 2, plane = (unsigned long long)(n + 1) * rs;
    const unsigned long long ie = 2ull * (PF_IEW * PF_IEW * plane + PF_ILW) * sizeof(double);  // ieO + ieI (+ tail pad)
    unsigned long long d4 = 0, cx = 0, pmx = 0, maxC = 1, rows = 0;
    for (int t = 0; t <= n - 3; ++t) {
        const unsigned long long m = (unsigned long long)(n - t - 2), C = (unsigned long long)(t + 1) * (m * (m + 1) / 2);
        d4 += (unsigned long long)PF_NMAT4 * C;
        cx += 2 * C;
        pmx += m * (unsigned long long)n * (t + 1);
        maxC = std::max(maxC, C);
        // work items: create_impl's enumeration with every pair able to pair (its upper bound), one item
        // per 64-lane chunk of each PL / PR / PM row
        const int mi = (int)m;
        for (int i = 1; i <= mi; ++i) rows += (unsigned long long)std::max(0, t - 5) * ((mi - i) / 64 + 1);  // PL, a in [6, t]
        for (int q = 0; q < mi; ++q) rows += (unsigned long long)std::max(0, t - 5) * (q / 64 + 1);         // PR, a in [0, t-6]
        for (int h = 0; h <= mi - 1; ++h)                                                                   // PM
            for (int j = 1; j + h + 2 <= n; ++j) {
                const int k = j + h + 2, alo = std::max(2, t - (n - k)), ahi = std::min(t - 2, j - 1);
                if (alo <= ahi) rows += (unsigned long long)((ahi - alo) / 64 + 1);
            }
    }
    unsigned long long dev = ie + (d4 + cx + pmx + (unsigned long long)PF_RECS * (d4 / PF_NMAT4)) * sizeof(int) +
                             2ull * 3 * maxC * sizeof(double);  // d4, copies, split-loop records, R
    dev += (unsigned long long)CCJ_PF_NMAT2 * plane * sizeof(double) + 2 * plane * sizeof(long long);  // 2-D, Pacc, Pabs
    dev += 3 * plane * sizeof(double) + plane + 2ull * plane * PF_IEW * sizeof(uint32_t);             // hp, est, cp; pt; mO, mI
    dev += rows * sizeof(uint32_t) + sizeof(PfExp) + (1u << 20);                                      // items; small tables
    dev += (unsigned long long)PF_KEYS * sizeof(double);                                              // interior-loop key table
    if (device_bytes) *device_bytes = dev;
    if (host_bytes) *host_bytes = ie;
}

namespace {

int pf_err(ccj_pf_ctx *c, int code, const char *what, hipError_t e = hipSuccess) {
    if (c) c->msg = e == hipSuccess ? std::string(what) : std::string(what) + ": " + hipGetErrorString(e);
    return code;
}
#define PFCHK(c, x)                                                   \
    do {                                                              \
        const hipError_t e_ = (x);                                    \
        if (e_ != hipSuccess) return pf_err((c), CCJ_E_HIP, #x, e_);  \
    } while (0)

// exp_E_Hairpin (loops/hairpin.h:231-291) * scale[j-i+1] for HairpinE(i, j) (part_func.cc:214-220)
double hairpin_pf(const ccj_pf_ctx &c, int i, int j) {
    const int type = c.ptype(i, j);
    if (type == 0) return 0;
    const PfExp &P = c.E;
    const int u = j - i - 1;
    double q;
    if (u <= 30) q = P.hairpin[u];
    else q = P.hairpin[30] * exp(-(P.lxc * log(u / 30.)) * 10. / P.kT);
    if (u < 3) return q * 1.0;
    const char *str = c.seq.c_str() + (i - 1);
    if (c.prm.special_hp) {
        if (u == 4) {
            char tl[7] = {0};
            memcpy(tl, str, 6);
            if (const char *ts = strstr(c.prm.Tetraloops, tl)) {
                if (type != 7) return P.tetra[(ts - c.prm.Tetraloops) / 7] * 1.0;
                q *= P.tetra[(ts - c.prm.Tetraloops) / 7];
            }
        } else if (u == 6) {
            char tl[9] = {0};
            memcpy(tl, str, 8);
            if (const char *ts = strstr(c.prm.Hexaloops, tl)) return P.hex[(ts - c.prm.Hexaloops) / 9] * 1.0;
        } else if (u == 3) {
            char tl[6] = {0};
            memcpy(tl, str, 5);
            if (const char *ts = strstr(c.prm.Triloops, tl)) return P.tri[(ts - c.prm.Triloops) / 6] * 1.0;
            return (type > 2 ? q * P.TermAU : q) * 1.0;
        }
    }
    q *= P.mismatchH[type][c.S1[i + 1]][c.S1[j - 1]];
    return q * 1.0;
}

// compute_int (part_func.cc:872-875)
double compute_int_pf(const ccj_pf_ctx &c, int i, int j, int k, int l) {
    return exp_E_IntLoop_pf(c.E, k - i - 1, j - l - 1, c.ptype(i, j), c.rtype[c.ptype(k, l)], c.S1[i + 1], c.S1[j - 1],
                            c.S1[k - 1], c.S1[l + 1]);
}

double ext_pf(const ccj_pf_ctx &c, int i, int j) {  // exp_Extloop :180-190
    const int tt = c.ptype(i, j);
    if (c.dangles == 1 || c.dangles == 2) return exp_E_ExtLoop_pf(c.E, tt, i > 1 ? c.S[i - 1] : -1, j < c.n ? c.S[j + 1] : -1);
    return exp_E_ExtLoop_pf(c.E, tt, -1, -1);
}
double mlstem_pf(const ccj_pf_ctx &c, int i, int j) {  // exp_MLstem :192-201
    const int tt = c.ptype(i, j);
    if (c.dangles == 1 || c.dangles == 2) return exp_E_MLstem_pf(c.E, tt, i > 1 ? c.S[i - 1] : -1, j < c.n ? c.S[j + 1] : -1);
    return exp_E_MLstem_pf(c.E, tt, -1, -1);
}
double mbloop_pf(const ccj_pf_ctx &c, int i, int j) {  // exp_Mbloop :203-212
    const int tt = c.pair[c.S[j]][c.S[i]];
    if (c.dangles == 1 || c.dangles == 2) return exp_E_MLstem_pf(c.E, tt, j < c.n ? c.S[j - 1] : -1, i > 1 ? c.S[i + 1] : -1);
    return exp_E_MLstem_pf(c.E, tt, -1, -1);
}

void run_threads(int total, int nthr, const std::function<void(int, int)> &f) {
    std::vector<std::thread> th;
    const int per = (total + nthr - 1) / nthr;
    for (int t = 0; t < nthr; ++t) {
        const int lo = t * per, hi = std::min(total, lo + per);
        if (lo < hi) th.emplace_back(f, lo, hi);
    }
    for (auto &x : th) x.join();
}

void free_dev(ccj_pf_ctx *c) {
    void *model[] = {c->d_E, c->d_pair, c->d_rtype, c->d_mlb, c->d_cpp, c->d_pup, c->d_ietab, c->d_esttab};
    void *ptrs[] = {c->d_S, c->d_S1, c->d_pt, c->d_hp, c->d_est, c->d_ieO, c->d_ieI, c->d_2d, c->d_Pacc, c->d_Pabs,
                    c->d_d4, c->d_cx, c->d_pmx, c->d_prec, c->d_R, c->d_items, c->d_mO, c->d_mI, c->d_ld, c->d_icount,
                    c->d_ioff};
    if (!c->batch)
        for (void *p : model)
            if (p) hipFree(p);
    for (void *p : ptrs)
        if (p) hipFree(p);
    void *pinned[] = {c->h_S, c->h_hp, c->h_lv, c->h_icount, c->h_ioff};
    for (void *p : pinned)
        if (p) hipHostFree(p);
    if (c->e0) hipEventDestroy(c->e0);
    if (c->e1) hipEventDestroy(c->e1);
    for (hipEvent_t e : c->tev) hipEventDestroy(e);
    c->tev.clear();
    for (auto *v : {&c->ev_lev, &c->ev_il, &c->ev_dg}) {
        for (hipEvent_t e : *v)
            if (e) hipEventDestroy(e);
        v->clear();
    }
    if (c->ev_start) hipEventDestroy(c->ev_start);
    if (c->st_il) hipStreamDestroy(c->st_il);
    if (c->st_d) hipStreamDestroy(c->st_d);
    if (c->st && !c->batch) hipStreamDestroy(c->st);
}

// Algorithmic bytes of one fill per kernel family (ccj_pf_work_model): the operands each kernel's
// recurrences read from and write to HBM-resident arrays, counted from the same enumerations the
// kernels run (the small 2-D tables and weight windows, which stay in cache, are not charged).
//   k_pf_iloop: 4 B per active lane per window term it loads (masked), 4 B stack operand, 8 B R store
//   k_pf_level: 4 B per 4-D operand load of the 21 recurrences (split loops, seeds, P blocks as
//               evaluated for this sequence's pairs), 8 B per R read, 21 x 4 B stores + 4 B per copy
//   P terms (k_pf_ppush / k_pf_pterm): 2 x 4 B per PK product, the pull form's operands;  k_pf_diag: 8 B per 2-D operand of the span's sums
struct PfWork {
    double iloop = 0, level = 0, pterm = 0, diag = 0;
};

PfWork pf_work_model(const ccj_pf_ctx &c) {
    const int n = c.n, rs = c.rs;
    PfWork w;
    if (n < 3) return w;
    auto low = [](int u) { return u < 0 ? 0u : (2u << u) - 1u; };
    const int nthr = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<double> il(n, 0.0), lv(n, 0.0);
    run_threads(n - 2, nthr, [&](int t0, int t1) {
        for (int t = t0; t < t1; ++t) {
            const int m = n - t - 2;
            double b_il = 0;
            for (long long q = c.ifirst[t]; q < c.ifirst[t + 1]; ++q) {
                const uint32_t it = c.h_items[q];
                const int role = (int)(it >> 30), f1 = (int)((it >> 20) & 1023), f2 = (int)((it >> 10) & 1023),
                          ch = (int)(it & 1023);
                if (role < 2) {
                    const int a = f1, b = t - a;
                    const int lanes = role == 0 ? std::min(64, m - f2 + 1 - ch * 64) : std::min(64, f2 + 1 - ch * 64);
                    const int w0 = role == 0 ? a : b, p0 = role == 0 ? f2 : f2 + a + 3;
                    const uint32_t *mw = c.h_mO.data() + ((size_t)w0 * rs + p0) * PF_IEW;
                    long long terms = 0;
                    for (int u1 = 0; u1 <= std::min(w0, MAXLOOP) - 2; ++u1)
                        terms += __builtin_popcount(mw[u1] & low(std::min(w0 - u1 - 6, PF_IEW - 1)));
                    b_il += (double)lanes * (12.0 + 4.0 * terms);
                } else {
                    const int h = f1, j = f2, k = j + h + 2;
                    const int alo = std::max(2, t - (n - k)), ahi = std::min(t - 2, j - 1);
                    const int a0 = alo + ch * 64, a1 = std::min(ahi, a0 + 63);
                    const uint32_t *mw = c.h_mI.data() + ((size_t)(h + 2) * rs + j) * PF_IEW;
                    double lt = 0;
                    for (int u1 = 0; u1 <= std::min(a1 - 2, PF_IEW - 1); ++u1) {
                        uint32_t mk = mw[u1] & low(std::min(std::min(t - a0 - 2, PF_IEW - 1), t - 4 - u1));
                        while (mk) {
                            const int u2 = __builtin_ctz(mk);
                            mk &= mk - 1;
                            lt += std::max(0, std::min(a1, t - 2 - u2) - std::max(a0, u1 + 2) + 1);
                        }
                    }
                    b_il += 12.0 * (a1 - a0 + 1) + 4.0 * lt;
                }
            }
            il[t] = b_il;
            double b_lv = 0;
            for (int a = 0; a <= t; ++a) {
                const int b = t - a;
                const double split = (a >= 1 ? 11.0 * a - 6 : 0) + (b >= 1 ? 11.0 * b - 6 : 0) + 4.0 * (b >= 1) + (a >= 1);
                for (int h = 0; h < m; ++h)
                    for (int i = 1; i + h <= m; ++i) {
                        const int j = i + a, k = j + h + 2, l = k + b;
                        double r4 = split, by = 21.0 * 4;
                        if (c.ptype(i, j) > 0) {
                            const bool in = a >= 2;
                            by += (a >= 6 ? 8 : 0) + 4;  // R or the stack operand; the copy store
                            r4 += (a < 6 && in ? 1 : 0) + (in ? 2 : 0) + (in && j >= i + TURN + 1 ? 1 : 0);
                        }
                        if (c.ptype(k, l) > 0) {
                            const bool in = b >= 2;
                            by += (b >= 6 ? 8 : 0) + 4;
                            r4 += (b < 6 && in ? 1 : 0) + (in ? 2 : 0) + (in && l >= k + TURN + 1 ? 1 : 0);
                        }
                        const bool in11 = a >= 1 && b >= 1;
                        if (c.ptype(j, k) > 0) {
                            const bool rr = a >= 2 && b >= 2;
                            by += (rr ? 8 : 0) + 4;
                            r4 += (!rr && in11 ? 1 : 0) + (in11 ? 2 : 0) + (in11 && k >= j + TURN - 1 ? 1 : 0);
                        }
                        if (c.ptype(i, l) > 0) r4 += in11 ? 3 + (l >= i + TURN + 1 ? 1 : 0) : 0;
                        b_lv += 4.0 * r4 + by;
                    }
            }
            lv[t] = b_lv;
        }
    });
    for (int t = 0; t < n; ++t) {
        w.iloop += il[t];
        w.level += lv[t];
    }
    for (int s = 3; s <= n - 1; ++s)  // C(s,3) (j, d, k) triples per i, two 4-B operands each
        w.pterm += 8.0 * (n - s) * ((double)s * (s - 1) * (s - 2) / 6.0);
    for (int s = 0; s <= n - 1; ++s)
        for (int i = 1; i + s <= n; ++i) {
            const int j = i + s;
            double ops = 0;
            for (int k = i + 1; k <= std::min(j - TURN - 2, i + MAXLOOP + 1); ++k)
                ops += std::max(0, j - (std::max(k + TURN + 1 + MAXLOOP + 2, k + j - i) - MAXLOOP - 2));
            ops += 3.0 * std::max(0, j - TURN - 1 - i) * 2 + 2.0 * s * 3 * 2 + 4.0 * std::max(0, j - TURN - i) * 3;
            w.diag += 8.0 * ops;
        }
    return w;
}

// ---------------------------------------------------------------------------------------------
// Context set-up in three parts: the model (parameters, penalties, key tables) and
// the allocation for a capacity, once per context; binding a length; the per-sequence tables.
// ---------------------------------------------------------------------------------------------

// The model of a problem: everything of a context that does not depend on the sequence.  No GPU.
int init_model(const ccj_problem *prob, const ccj_pf_raw *raw, ccj_pf_ctx *c) {
    if (!prob || !prob->params) return pf_err(c, CCJ_E_ARG, "null problem");
    if (prob->params->magic != CCJ_PARAMS_MAGIC || prob->params->size_bytes != sizeof(ccj_energy_params))
        return pf_err(c, CCJ_E_ARG, "bad parameter blob");
    if (raw && (raw->magic != CCJ_PF_RAW_MAGIC || raw->size_bytes != sizeof(ccj_pf_raw)))
        return pf_err(c, CCJ_E_ARG, "bad ccj_pf_raw table");
    c->dangles = prob->dangles;
    c->noGU = prob->noGU ? 1 : 0;
    c->prm = *prob->params;
    const ccj_pk_penalties defp = CCJ_PK_PENALTIES_DEFAULT;
    c->pen = prob->pen ? *prob->pen : defp;
    // make_pair_matrix (pair_mat.h:81-183)
    const int base_rtype[8] = {0, 2, 1, 4, 3, 6, 5, 7};
    memcpy(c->rtype, base_rtype, sizeof base_rtype);
    for (int x = 0; x < 8; ++x)
        for (int y = 0; y < 8; ++y) c->pair[x][y] = BP_PAIR_PF[x][y];
    if (prob->noGU) c->pair[3][4] = c->pair[4][3] = 0;
    for (int x = 0; x < 8; ++x)
        for (int y = 0; y < 8; ++y) c->rtype[c->pair[x][y]] = c->pair[y][x];
    build_exp(c->prm, raw, c->pen, c->E);
    return CCJ_OK;
}

// A sequence a context of capacity cap can take: 1..cap of A/C/G/U/T.  Checked before the context
// is touched.
int check_seq(ccj_pf_ctx *c, const char *seq, int cap) {
    if (!seq) return pf_err(c, CCJ_E_ARG, "null sequence");
    const size_t n = strlen(seq);
    if (n < 1) return pf_err(c, CCJ_E_ARG, "empty sequence");
    if (n > 1023) return pf_err(c, CCJ_E_ARG, "sequence longer than 1023");
    if (cap > 0 && n > (size_t)cap) return pf_err(c, CCJ_E_ARG, "sequence longer than the context's capacity");
    for (const char *p = seq; *p; ++p)
        if (!(*p == 'A' || *p == 'C' || *p == 'G' || *p == 'U' || *p == 'T'))
            return pf_err(c, CCJ_E_ARG, "sequence must be A/C/G/U/T");
    return CCJ_OK;
}

// encode_sequence (pair_mat.h:81-183)
void set_seq_host(ccj_pf_ctx *c, const char *seq) {
    c->seq = seq;
    c->n = (int)c->seq.size();
    c->rs = c->n + 2;
    const int n = c->n;
    c->S.assign(n + 2, 0);
    c->S1.assign(n + 2, 0);
    for (int i = 1; i <= n; ++i) c->S[i] = c->S1[i] = (short)encode_base(c->seq[i - 1]);
    c->S[n + 1] = c->S[1];
    c->S[0] = (short)n;
    c->S1[n + 1] = c->S1[1];
    c->S1[0] = c->S1[n];
}

// exp_params_rescale (part_func.cc:97-125), pf_scale == 1 so every scale[] is 1: entry i does not
// depend on the length, so the tables of the capacity serve every binding
void build_powers(ccj_pf_ctx *c, int N) {
    c->mlb.assign(N + 2, 0);
    c->cpp.assign(N + 2, 0);
    c->pup.assign(N + 2, 0);
    c->mlb[0] = 1;
    c->mlb[1] = c->E.MLbase / 1.;
    c->cpp[0] = 1;
    c->cpp[1] = c->E.cp / 1.;
    c->pup[0] = 1;
    c->pup[1] = c->E.PUP / 1.;
    for (int i = 2; i <= N; ++i) {
        c->mlb[i] = pow(c->E.MLbase, (double)i) * 1.;
        c->cpp[i] = pow(c->E.cp, (double)i) * 1.;
        c->pup[i] = pow(c->E.PUP, (double)i) * 1.;
    }
}

// The key tables of ccj_pf_setup.h for sequences up to length N: get_e_intP / get_e_stP with the
// host's pow, one entry per key.  A loop with u1 + u2 > N - 4 fits no such sequence
// (p+1+u1 < q-1-u2 <= N-1), so those keys stay 0 and are never gathered.
void build_keytab(const ccj_pf_ctx &c, int N, std::vector<double> &ietab, double *esttab) {
    ietab.assign((size_t)PF_KEYS, 0.0);
    const int nthr = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    run_threads(PF_IEW * PF_IEW, nthr, [&](int s0, int s1) {
        for (int s = s0; s < s1; ++s) {
            const int u1 = s / PF_IEW, u2 = s % PF_IEW;
            if ((u1 == 0 && u2 == 0) || u1 + u2 > N - 4) continue;  // get_e_intP's stack case is 0
            for (int type = 1; type <= 6; ++type)
                for (int si1 = 1; si1 <= 4; ++si1)
                    for (int sj1 = 1; sj1 <= 4; ++sj1)
                        for (int type2 = 1; type2 <= 6; ++type2)
                            for (int sp1 = 1; sp1 <= 4; ++sp1)
                                for (int sq1 = 1; sq1 <= 4; ++sq1)
                                    ietab[(size_t)pf_ie_key(u1, u2, type, si1, sj1, type2, sp1, sq1)] =
                                        pow(exp_E_IntLoop_pf(c.E, u1, u2, type, type2, si1, sj1, sp1, sq1), c.pen.e_intP);
        }
    });
    for (int type = 0; type < 8; ++type)
        for (int type2 = 0; type2 < 8; ++type2)
            esttab[type * 8 + type2] = pow(exp_E_IntLoop_pf(c.E, 0, 0, type, type2, 0, 0, 0, 0), c.pen.e_stP);
}

// The per-sequence tables on the host.
struct PfHostTabs {
    std::vector<int8_t> pt;
    std::vector<double> est, ieO, ieI;  // ieO / ieI compacted, with the PF_ILW tail
    std::vector<uint32_t> mO, mI, items;
    std::vector<long long> ifirst;
};

// k_pf_iloop reads the weights of a window row only at the row's mask bits, in ascending order:
// store them compacted (k-th set bit -> slot k), so that a round's weights are one scalar load;
// PF_ILW zero doubles of tail padding cover the last row's round-wide reads
void compact_rows(std::vector<double> &v, const std::vector<uint32_t> &mk) {
    for (size_t r = 0; r < mk.size(); ++r) {
        double *row = v.data() + r * PF_IEW;
        int k = 0;
        for (int u2 = 0; u2 < PF_IEW; ++u2)
            if (mk[r] >> u2 & 1u) row[k++] = row[u2];
        for (; k < PF_IEW; ++k) row[k] = 0.0;
    }
    v.resize(v.size() + PF_ILW, 0.0);
}

// HairpinE of every interval, [w][p] (plane doubles)
void build_hp(const ccj_pf_ctx &c, double *hp) {
    const int n = c.n, rs = c.rs;
    memset(hp, 0, c.plane() * sizeof(double));
    for (int w = 0; w <= n - 1; ++w)
        for (int p = 1; p + w <= n; ++p) hp[(size_t)w * rs + p] = hairpin_pf(c, p, p + w);
}

// The direct builder: one pow per entry (CCJ_PF_HOST_SETUP=1; the yardstick of the key tables).
void host_tables(const ccj_pf_ctx &cx, PfHostTabs &T) {
    const ccj_pf_ctx *c = &cx;
    const int n = c->n, rs = c->rs;
    const size_t plane = c->plane();
    T.pt.assign(plane, 0);
    T.est.assign(plane, 0);
    for (int w = 0; w <= n - 1; ++w)
        for (int p = 1; p + w <= n; ++p) {
            const size_t ix = (size_t)w * rs + p;
            T.pt[ix] = (int8_t)c->ptype(p, p + w);
            // get_e_stP (part_func.cc:877-884); w == 0 is never read with a nonzero factor
            if (w >= 1 && w != 2) T.est[ix] = pow(compute_int_pf(*c, p, p + w, p + 1, p + w - 1), c->pen.e_stP);
        }
    // ieO / ieI: get_e_intP by outer / inner pair, each pair's 29 x 29 window contiguous
    constexpr int W2 = PF_IEW * PF_IEW;
    const size_t ie_n = (size_t)W2 * plane;
    std::vector<double> &ie = T.ieO, &ieI = T.ieI;
    ie.assign(ie_n, 0.0);
    ieI.assign(ie_n, 0.0);
    {
        const int nthr = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        run_threads(n, nthr, [&](int w0, int w1) {
            for (int w = w0; w < w1; ++w)
                for (int p = 1; p + w <= n; ++p) {
                    const int q = p + w;
                    for (int u1 = 0; u1 < PF_IEW; ++u1)
                        for (int u2 = 0; u2 < PF_IEW; ++u2) {
                            const int ip = p + 1 + u1, jp = q - 1 - u2;
                            if (ip >= jp || (u1 == 0 && u2 == 0)) continue;  // get_e_intP's stack case is 0
                            ie[((size_t)w * rs + p) * W2 + u1 * PF_IEW + u2] =
                                pow(compute_int_pf(*c, p, q, ip, jp), c->pen.e_intP);
                        }
                }
        });
        // ieI[g][j][u1][u2] = ieO[g+2+u1+u2][j-1-u1][u1][u2] (closing (j-1-u1, j+g+1+u2))
        run_threads(n, nthr, [&](int g0, int g1) {
            for (int g = g0; g < g1; ++g)
                for (int j = 1; j + g <= n; ++j)
                    for (int u1 = 0; u1 < PF_IEW; ++u1)
                        for (int u2 = 0; u2 < PF_IEW; ++u2) {
                            const int p = j - 1 - u1, w = g + 2 + u1 + u2;
                            if (p < 1 || p + w > n) continue;
                            ieI[((size_t)g * rs + j) * W2 + u1 * PF_IEW + u2] = ie[((size_t)w * rs + p) * W2 + u1 * PF_IEW + u2];
                        }
        });
    }
    // window masks: a term adds nothing when its weight is 0.0 or the pair of the 4-D value it reads
    // cannot pair (that value is 0): mO over (p+1+u1, p+w-1-u2), mI over (j-1-u1, j+g+1+u2)
    std::vector<uint32_t> &mO = T.mO, &mI = T.mI;
    mO.assign(plane * PF_IEW, 0u);
    mI.assign(plane * PF_IEW, 0u);
    for (int w = 0; w <= n - 1; ++w)
        for (int p = 1; p + w <= n; ++p)
            for (int u1 = 0; u1 < PF_IEW; ++u1) {
                const size_t r = ((size_t)w * rs + p) * PF_IEW + u1;
                for (int u2 = 0; u2 < PF_IEW; ++u2) {
                    const size_t e = ((size_t)w * rs + p) * W2 + u1 * PF_IEW + u2;
                    {   // outer (p, p+w)
                        const int ip = p + 1 + u1, jp = p + w - 1 - u2;
                        if (ip < jp && ie[e] != 0.0 && c->ptype(ip, jp) > 0) mO[r] |= 1u << u2;
                    }
                    {   // inner (p, p+w) = (j, j+g)
                        const int d = p - 1 - u1, dp = p + w + 1 + u2;
                        if (d >= 1 && dp <= n && ieI[e] != 0.0 && c->ptype(d, dp) > 0) mI[r] |= 1u << u2;
                    }
                }
            }
    compact_rows(ie, mO);
    compact_rows(ieI, mI);
    // k_pf_iloop work items: the cells of each pairing closing pair in 64-lane chunks, encoded as
    // ccj_items.h's (unsharded).  PL and PR rows are the MFE engine's; PM rows here start at h = 0,
    // since get_PMiloop has no hairpin bound on (j, k) (part_func.cc:804-824)
    std::vector<uint32_t> &items = T.items;
    items.clear();
    T.ifirst.assign(std::max(n - 1, 2), 0);
    struct PT {
        const int8_t *p;
        int rs;
        int operator()(int i, int j) const { return p[(size_t)(j - i) * rs + i]; }
    } ptf{T.pt.data(), rs};
    for (int t = 0; t <= n - 3; ++t) {
        T.ifirst[t] = (long long)items.size();
        const ItemRows R = item_rows(n, t, 1, 0);
        for (int x = 0; x < R.nPL + R.nPR; ++x) {
            uint32_t it0 = 0;
            const int cnt = item_row(ptf, n, t, R, x, 1, 0, it0);
            for (int q = 0; q < cnt; ++q) items.push_back(it0 | (uint32_t)q);
        }
        for (int h = 0; h <= R.m - 1; ++h)  // PM: pair (j, k = j+h+2), lanes a in [alo, ahi]
            for (int j = 1; j + h + 2 <= n; ++j) {
                const int k = j + h + 2, alo = std::max(2, t - (n - k)), ahi = std::min(t - 2, j - 1);
                if (alo > ahi || ptf(j, k) <= 0) continue;
                const uint32_t it0 = (2u << 30) | ((uint32_t)h << 20) | ((uint32_t)j << 10);
                for (int q = 0; q <= (ahi - alo) / 64; ++q) items.push_back(it0 | (uint32_t)q);
            }
    }
    T.ifirst[std::max(n - 2, 1)] = (long long)items.size();
}

// The same tables through the key tables and the gathers of ccj_pf_setup.h, as the setup kernels
// form them (row by row: mask, then the set bits' weights in ascending order).  Rows of intervals
// that cannot pair are zero here, which the fill never reads (k_pf_iloop has no item for them).
void keyed_tables(const ccj_pf_ctx &c, const double *ietab, const double *esttab, PfHostTabs &T) {
    const int n = c.n, rs = c.rs;
    const size_t plane = c.plane();
    int8_t pair8[64], rt8[8];
    for (int x = 0; x < 8; ++x) {
        rt8[x] = (int8_t)c.rtype[x];
        for (int y = 0; y < 8; ++y) pair8[x * 8 + y] = (int8_t)c.pair[x][y];
    }
    const PfSeqView v{n, rs, c.S.data(), pair8, rt8, ietab, esttab};
    constexpr int W2 = PF_IEW * PF_IEW;
    T.pt.assign(plane, 0);
    T.est.assign(plane, 0);
    T.ieO.assign(W2 * plane + PF_ILW, 0.0);
    T.ieI.assign(W2 * plane + PF_ILW, 0.0);
    T.mO.assign(plane * PF_IEW, 0u);
    T.mI.assign(plane * PF_IEW, 0u);
    for (int w = 0; w <= n - 1; ++w)
        for (int p = 1; p + w <= n; ++p) {
            const size_t ix = (size_t)w * rs + p;
            T.pt[ix] = (int8_t)v.ptype(p, p + w);
            T.est[ix] = pf_est_gather(v, w, p);
            for (int u1 = 0; u1 < PF_IEW; ++u1) {
                const size_t r = ix * PF_IEW + u1;
                int kO = 0, kI = 0;
                for (int u2 = 0; u2 < PF_IEW; ++u2) {
                    double wt;
                    if (pf_ie_outer(v, w, p, u1, u2, wt)) {
                        T.mO[r] |= 1u << u2;
                        T.ieO[r * PF_IEW + kO++] = wt;
                    }
                    if (pf_ie_inner(v, w, p, u1, u2, wt)) {
                        T.mI[r] |= 1u << u2;
                        T.ieI[r * PF_IEW + kI++] = wt;
                    }
                }
            }
        }
}

// FNV hashes of the setup tables: est whole; per interval whose pair can pair, in [w][p] order,
// the 29 mask words and the 29 x 29 compacted weights of ieO / mO and of ieI / mI.
void setup_table_hashes(const ccj_pf_ctx &c, const int8_t *pt, const double *est, const double *ieO, const double *ieI,
                        const uint32_t *mO, const uint32_t *mI, uint64_t *out5) {
    const int n = c.n, rs = c.rs;
    constexpr int W2 = PF_IEW * PF_IEW;
    out5[0] = fnv_arr(est, c.plane());
    uint64_t h[4] = {fnv_init(), fnv_init(), fnv_init(), fnv_init()};
    for (int w = 0; w <= n - 1; ++w)
        for (int p = 1; p + w <= n; ++p) {
            const size_t ix = (size_t)w * rs + p;
            if (pt[ix] <= 0) continue;
            fnv_bytes(h[0], ieO + ix * W2, W2 * sizeof(double));
            fnv_bytes(h[1], ieI + ix * W2, W2 * sizeof(double));
            fnv_bytes(h[2], mO + ix * PF_IEW, PF_IEW * sizeof(uint32_t));
            fnv_bytes(h[3], mI + ix * PF_IEW, PF_IEW * sizeof(uint32_t));
        }
    for (int q = 0; q < 4; ++q) out5[1 + q] = h[q];
}

// Level layout of a length (ccj_pf_engine.h).  Fails where k_pf_ppush's offsets would not fit.
struct PfLayout {
    std::vector<PfLvl> lv;
    long long cells = 0, off = 0, offx = 0, offm = 0, maxC = 1;
};
bool make_layout(int n, PfLayout &Y) {
    Y = PfLayout{};
    Y.lv.assign(std::max(n - 2, 1), PfLvl{0, 0, 0, 0, 0, 0, 0});
    for (int t = 0; t <= n - 3; ++t) {
        const long long m = n - t - 2, M = m * (m + 1) / 2;
        Y.lv[t] = PfLvl{Y.off, (t + 1) * M, (int)M, 0, Y.offx, Y.offm, Y.cells};
        Y.off += (long long)PF_NMAT4 * (t + 1) * M;
        Y.offx += 2 * (t + 1) * M;
        Y.offm += m * n * (t + 1);
        Y.maxC = std::max(Y.maxC, (t + 1) * M);
        Y.cells += (t + 1) * M;
    }
    // k_pf_ppush addresses the PK rows of PF_PP_S consecutive levels as 32-bit byte offsets from the
    // lowest one's PK start (one buffer resource per wave): that span must stay below 4 GB
    for (int t = 0; t <= n - 3; ++t) {
        const int tt = std::min(t + PF_PP_S - 1, n - 3);
        const long long lo = Y.lv[t].lb + PF_PK * Y.lv[t].C, hi = Y.lv[tt].lb + PF_PK * Y.lv[tt].C + Y.lv[tt].C;
        if (4 * (hi - lo) >= (1LL << 32)) return false;
    }
    return true;
}
const char *const kPpushMsg = "n too large: the PK rows of 8 levels exceed 4 GB (k_pf_ppush offsets)";

// The streams and events of one fill graph for lengths up to N (a context's, or a batch's).
struct PfGraph {
    hipStream_t *st, *st_il, *st_d;
    std::vector<hipEvent_t> *ev_lev, *ev_il, *ev_dg;
    hipEvent_t *ev_start, *e0, *e1;
};
hipError_t make_graph(const PfGraph &g, int N) {
    hipError_t e;
    for (hipStream_t *s : {g.st, g.st_il, g.st_d})
        if ((e = hipStreamCreateWithFlags(s, hipStreamNonBlocking)) != hipSuccess) return e;
    if ((e = hipEventCreateWithFlags(g.ev_start, hipEventDisableTiming)) != hipSuccess) return e;
    for (auto *v : {g.ev_lev, g.ev_il, g.ev_dg}) {
        v->assign(N + 1, nullptr);
        for (hipEvent_t &x : *v)
            if ((e = hipEventCreateWithFlags(&x, hipEventDisableTiming)) != hipSuccess) return e;
    }
    if ((e = hipEventCreate(g.e0)) != hipSuccess) return e;
    return hipEventCreate(g.e1);
}

// Once per context, or once per lockstep batch: the fill graph and the model's device tables
// (Boltzmann tables, powers, key tables) for lengths up to N.
int alloc_model(ccj_pf_ctx *c, int N, int device) {
    c->cap = N;
    c->device = device;
    PFCHK(c, hipSetDevice(device));
    PFCHK(c, make_graph(PfGraph{&c->st, &c->st_il, &c->st_d, &c->ev_lev, &c->ev_il, &c->ev_dg, &c->ev_start, &c->e0, &c->e1}, N));
    auto up = [&](void **d, const void *h, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(d, bytes ? bytes : 8);
        if (e != hipSuccess) return e;
        return bytes ? hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    int8_t pair8[64], rt8[8];
    for (int x = 0; x < 8; ++x) {
        rt8[x] = (int8_t)c->rtype[x];
        for (int y = 0; y < 8; ++y) pair8[x * 8 + y] = (int8_t)c->pair[x][y];
    }
    PFCHK(c, up((void **)&c->d_E, &c->E, sizeof(PfExp)));
    PFCHK(c, up((void **)&c->d_pair, pair8, 64));
    PFCHK(c, up((void **)&c->d_rtype, rt8, 8));
    PFCHK(c, up((void **)&c->d_mlb, c->mlb.data(), c->mlb.size() * sizeof(double)));
    PFCHK(c, up((void **)&c->d_cpp, c->cpp.data(), c->cpp.size() * sizeof(double)));
    PFCHK(c, up((void **)&c->d_pup, c->pup.data(), c->pup.size() * sizeof(double)));
    std::vector<double> ietab;
    const auto t0 = std::chrono::steady_clock::now();
    build_keytab(*c, N, ietab, c->esttab);
    c->keytab_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    PFCHK(c, up((void **)&c->d_ietab, ietab.data(), ietab.size() * sizeof(double)));
    PFCHK(c, up((void **)&c->d_esttab, c->esttab, sizeof c->esttab));
    return CCJ_OK;
}

// Allocation for a capacity N: every buffer, event and pinned staging area at its maximum over the
// lengths 1..N.  Each size grows with the length, so the layout of N gives the maxima.
// share: a batch's model context, which owns the model's device tables and the stream: c (a member,
// c->batch set) borrows them and gets no fill graph of its own.
int alloc_cap(ccj_pf_ctx *c, int N, int device, const PfLayout &Y, const ccj_pf_ctx *share = nullptr) {
    const size_t plane = (size_t)(N + 1) * (N + 2);
    constexpr int W2 = PF_IEW * PF_IEW;
    if (share) {
        c->cap = N;
        c->device = device;
        c->st = share->st;
        c->d_E = share->d_E;
        c->d_pair = share->d_pair;
        c->d_rtype = share->d_rtype;
        c->d_mlb = share->d_mlb;
        c->d_cpp = share->d_cpp;
        c->d_pup = share->d_pup;
        c->d_ietab = share->d_ietab;
        c->d_esttab = share->d_esttab;
        memcpy(c->esttab, share->esttab, sizeof c->esttab);
        c->keytab_ms = share->keytab_ms;
        PFCHK(c, hipSetDevice(device));
    } else {
        const int rc = alloc_model(c, N, device);
        if (rc != CCJ_OK) return rc;
    }
    // per sequence
    PFCHK(c, hipMalloc((void **)&c->d_S, (size_t)(N + 2) * sizeof(short)));
    PFCHK(c, hipMalloc((void **)&c->d_S1, (size_t)(N + 2) * sizeof(short)));
    PFCHK(c, hipMalloc((void **)&c->d_pt, plane));
    PFCHK(c, hipMalloc((void **)&c->d_hp, plane * sizeof(double)));
    PFCHK(c, hipMalloc((void **)&c->d_est, plane * sizeof(double)));
    PFCHK(c, hipMalloc((void **)&c->d_ieO, (W2 * plane + PF_ILW) * sizeof(double)));
    PFCHK(c, hipMalloc((void **)&c->d_ieI, (W2 * plane + PF_ILW) * sizeof(double)));
    PFCHK(c, hipMalloc((void **)&c->d_mO, plane * PF_IEW * sizeof(uint32_t)));
    PFCHK(c, hipMalloc((void **)&c->d_mI, plane * PF_IEW * sizeof(uint32_t)));
    c->items_cap = (long long)pf_items_bound(N);
    PFCHK(c, hipMalloc((void **)&c->d_items, (size_t)std::max(c->items_cap, 2LL) * sizeof(uint32_t)));
    const size_t nsp = (size_t)std::max(N - 2, 1) * KI_SPLIT;
    PFCHK(c, hipMalloc((void **)&c->d_icount, nsp * sizeof(long long)));
    PFCHK(c, hipMalloc((void **)&c->d_ioff, nsp * sizeof(long long)));
    PFCHK(c, hipMalloc((void **)&c->d_ld, Y.lv.size() * sizeof(PfLvl)));
    // per fill
    PFCHK(c, hipMalloc((void **)&c->d_2d, (size_t)CCJ_PF_NMAT2 * plane * sizeof(double)));
    PFCHK(c, hipMalloc((void **)&c->d_Pacc, plane * sizeof(long long)));
    PFCHK(c, hipMalloc((void **)&c->d_Pabs, plane * sizeof(unsigned long long)));
    PFCHK(c, hipMalloc((void **)&c->d_d4, (size_t)std::max(Y.off, 1LL) * sizeof(int)));
    PFCHK(c, hipMalloc((void **)&c->d_prec, (size_t)PF_RECS * std::max(Y.cells, 1LL) * sizeof(int)));
    PFCHK(c, hipMalloc((void **)&c->d_cx, (size_t)std::max(Y.offx, 1LL) * sizeof(int)));
    PFCHK(c, hipMalloc((void **)&c->d_pmx, (size_t)std::max(Y.offm, 1LL) * sizeof(int)));
    PFCHK(c, hipMalloc((void **)&c->d_R, (size_t)2 * 3 * Y.maxC * sizeof(double)));
    // pinned staging
    PFCHK(c, hipHostMalloc((void **)&c->h_S, (size_t)2 * (N + 2) * sizeof(short)));
    PFCHK(c, hipHostMalloc((void **)&c->h_hp, plane * sizeof(double)));
    PFCHK(c, hipHostMalloc((void **)&c->h_lv, Y.lv.size() * sizeof(PfLvl)));
    PFCHK(c, hipHostMalloc((void **)&c->h_icount, nsp * sizeof(long long)));
    PFCHK(c, hipHostMalloc((void **)&c->h_ioff, nsp * sizeof(long long)));

    PfDev &D = c->D;
    D.dangles = c->dangles;
    D.ap_int = c->pen.ap;
    D.E = c->d_E;
    D.S = c->d_S;
    D.S1 = c->d_S1;
    D.pt = c->d_pt;
    D.pair = c->d_pair;
    D.rtype = c->d_rtype;
    D.hp = c->d_hp;
    D.est = c->d_est;
    D.ieO = c->d_ieO;
    D.ieI = c->d_ieI;
    D.mO = c->d_mO;
    D.mI = c->d_mI;
    D.mlb = c->d_mlb;
    D.cpp = c->d_cpp;
    D.pup = c->d_pup;
    D.Pacc = c->d_Pacc;
    D.Pabs = c->d_Pabs;
    D.d4 = c->d_d4;
    D.cx = c->d_cx;
    D.pmx = c->d_pmx;
    D.items = c->d_items;
    D.R = c->d_R;
    D.ld = c->d_ld;
    return CCJ_OK;
}

// Bind the length of c->seq (set_seq_host): the row stride and the plane bases inside d_2d, the
// level descriptors with the record bases, Rst.  Allocates nothing; at n == capacity every offset
// is what a context created for that length has.
int bind_len(ccj_pf_ctx *c, const PfLayout &Y) {
    const int n = c->n;
    const size_t plane = c->plane();
    c->lv = Y.lv;
    c->cells = Y.cells;
    c->offx = Y.offx;
    c->offm = Y.offm;
    memcpy(c->h_lv, c->lv.data(), c->lv.size() * sizeof(PfLvl));
    PFCHK(c, hipMemcpyAsync(c->d_ld, c->h_lv, c->lv.size() * sizeof(PfLvl), hipMemcpyHostToDevice, c->st));
    PfDev &D = c->D;
    D.n = n;
    D.rs = c->rs;
    D.Rst = 3 * Y.maxC;
    double *pl[CCJ_PF_NMAT2];
    for (int m = 0; m < CCJ_PF_NMAT2; ++m) pl[m] = c->d_2d + (size_t)m * plane;
    D.V = pl[CCJ_PF_V];
    D.VM = pl[CCJ_PF_VM];
    D.WM = pl[CCJ_PF_WM];
    D.WMv = pl[CCJ_PF_WMv];
    D.WMp = pl[CCJ_PF_WMp];
    D.WBP = pl[CCJ_PF_WBP];
    D.WPP = pl[CCJ_PF_WPP];
    D.P = pl[CCJ_PF_P];
    D.r1 = c->d_prec;
    D.r2 = D.r1 + (size_t)PF_REC1 * c->cells;
    D.r3 = D.r2 + (size_t)PF_REC2 * c->cells;
    D.r4 = D.r3 + (size_t)PF_REC3 * c->cells;
    return CCJ_OK;
}

bool host_setup() {
    const char *e = getenv("CCJ_PF_HOST_SETUP");
    return e && atoi(e) != 0;
}

PfSetupDev setup_dev(const ccj_pf_ctx *c) {
    PfSetupDev T;
    T.v = PfSeqView{c->n, c->rs, c->d_S, c->d_pair, c->d_rtype, c->d_ietab, c->d_esttab};
    T.pt = c->d_pt;
    T.est = c->d_est;
    T.ieO = c->d_ieO;
    T.ieI = c->d_ieI;
    T.mO = c->d_mO;
    T.mI = c->d_mI;
    return T;
}

// The per-sequence state of the bound sequence, on the context's stream: S / S1 and hp (host,
// through pinned staging), the copies zeroed, then pt, est, ieO / ieI, mO / mI and the work items
// by the setup kernels (ccj_pf.hip).  One wait: the item counts, whose prefix the host forms.
// CCJ_PF_HOST_SETUP=1: the tables of host_tables() instead, uploaded with blocking copies.
// In two halves around that wait, so that a lockstep batch waits once for all its members:
// setup_seq_a enqueues everything up to the copy of the item counts, setup_seq_b (after the
// stream has been synchronized) forms their prefix and enqueues the items pass.
int setup_seq_a(ccj_pf_ctx *c) {
    const int n = c->n, N2 = c->cap + 2;
    const size_t plane = c->plane();
    constexpr int W2 = PF_IEW * PF_IEW;
    c->filled = false;
    c->h_items.clear();
    c->h_mO.clear();
    c->h_mI.clear();
    PFCHK(c, hipSetDevice(c->device));
    memcpy(c->h_S, c->S.data(), (size_t)(n + 2) * sizeof(short));
    memcpy(c->h_S + N2, c->S1.data(), (size_t)(n + 2) * sizeof(short));
    PFCHK(c, hipMemcpyAsync(c->d_S, c->h_S, (size_t)(n + 2) * sizeof(short), hipMemcpyHostToDevice, c->st));
    PFCHK(c, hipMemcpyAsync(c->d_S1, c->h_S + N2, (size_t)(n + 2) * sizeof(short), hipMemcpyHostToDevice, c->st));
    // The copies of PL / PR / PM are written only where the pair can pair and read as 0 elsewhere;
    // which pairs can pair changes with the sequence: zero the bound extent (DESIGN.md §10 audit)
    PFCHK(c, hipMemsetAsync(c->d_cx, 0, (size_t)std::max(c->offx, 1LL) * sizeof(int), c->st));
    PFCHK(c, hipMemsetAsync(c->d_pmx, 0, (size_t)std::max(c->offm, 1LL) * sizeof(int), c->st));
    c->ifirst.assign(std::max(n - 1, 2), 0);
    c->setup_pending = false;
    if (host_setup()) {
        build_hp(*c, c->h_hp);
        PFCHK(c, hipMemcpyAsync(c->d_hp, c->h_hp, plane * sizeof(double), hipMemcpyHostToDevice, c->st));
        PfHostTabs T;
        host_tables(*c, T);
        if ((long long)T.items.size() > c->items_cap) return pf_err(c, CCJ_E_STATE, "work items exceed their bound");
        PFCHK(c, hipStreamSynchronize(c->st));
        PFCHK(c, hipMemcpy(c->d_pt, T.pt.data(), T.pt.size(), hipMemcpyHostToDevice));
        PFCHK(c, hipMemcpy(c->d_est, T.est.data(), T.est.size() * sizeof(double), hipMemcpyHostToDevice));
        PFCHK(c, hipMemcpy(c->d_ieO, T.ieO.data(), T.ieO.size() * sizeof(double), hipMemcpyHostToDevice));
        PFCHK(c, hipMemcpy(c->d_ieI, T.ieI.data(), T.ieI.size() * sizeof(double), hipMemcpyHostToDevice));
        PFCHK(c, hipMemcpy(c->d_mO, T.mO.data(), T.mO.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        PFCHK(c, hipMemcpy(c->d_mI, T.mI.data(), T.mI.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (!T.items.empty())
            PFCHK(c, hipMemcpy(c->d_items, T.items.data(), T.items.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        c->ifirst = T.ifirst;
        return CCJ_OK;
    }
    const PfSetupDev T = setup_dev(c);
    PFCHK(c, (hipError_t)ccjk_pf_setup_tables(&T, c->st));
    PFCHK(c, hipMemsetAsync(c->d_ieO + W2 * plane, 0, PF_ILW * sizeof(double), c->st));
    PFCHK(c, hipMemsetAsync(c->d_ieI + W2 * plane, 0, PF_ILW * sizeof(double), c->st));
    const int nl = std::max(n - 2, 0);
    const size_t nsp = (size_t)nl * KI_SPLIT;
    if (nsp) {
        PFCHK(c, (hipError_t)ccjk_pf_items(&T, c->d_icount, nullptr, nullptr, 0, c->st));
        PFCHK(c, hipMemcpyAsync(c->h_icount, c->d_icount, nsp * sizeof(long long), hipMemcpyDeviceToHost, c->st));
    }
    // hp: the special-hairpin strstr cases stay on the host; built while the kernels run
    build_hp(*c, c->h_hp);
    PFCHK(c, hipMemcpyAsync(c->d_hp, c->h_hp, plane * sizeof(double), hipMemcpyHostToDevice, c->st));
    c->setup_pending = true;
    return CCJ_OK;
}

int setup_seq_b(ccj_pf_ctx *c) {
    if (!c->setup_pending) return CCJ_OK;  // the host builder left nothing to do
    c->setup_pending = false;
    const int n = c->n, nl = std::max(n - 2, 0);
    const size_t nsp = (size_t)nl * KI_SPLIT;
    const PfSetupDev T = setup_dev(c);
    long long o = 0;
    for (int t = 0; t < nl; ++t) {
        c->ifirst[t] = o;
        for (int s = 0; s < KI_SPLIT; ++s) {
            c->h_ioff[(size_t)t * KI_SPLIT + s] = o;
            o += c->h_icount[(size_t)t * KI_SPLIT + s];
        }
    }
    c->ifirst[std::max(n - 2, 1)] = o;
    if (o > c->items_cap) return pf_err(c, CCJ_E_STATE, "work items exceed their bound");
    if (nsp) {
        PFCHK(c, hipMemcpyAsync(c->d_ioff, c->h_ioff, nsp * sizeof(long long), hipMemcpyHostToDevice, c->st));
        PFCHK(c, (hipError_t)ccjk_pf_items(&T, nullptr, c->d_ioff, c->d_items, 1, c->st));
    }
    return CCJ_OK;
}

int setup_seq(ccj_pf_ctx *c) {
    int rc = setup_seq_a(c);
    if (rc != CCJ_OK || !c->setup_pending) return rc;
    PFCHK(c, hipStreamSynchronize(c->st));  // the one wait of a reset: the item counts
    return setup_seq_b(c);
}

// Rebind an open context to seq (any length up to the capacity; the bound length = a reset).
int rebind_impl(ccj_pf_ctx *c, const char *seq) {
    const int rc = check_seq(c, seq, c->cap);
    if (rc != CCJ_OK) return rc;
    PfLayout Y;
    if (!make_layout((int)strlen(seq), Y)) return pf_err(c, CCJ_E_ARG, kPpushMsg);
    set_seq_host(c, seq);
    PFCHK(c, hipSetDevice(c->device));
    const int rb = bind_len(c, Y);
    return rb != CCJ_OK ? rb : setup_seq(c);
}

int create_impl(const ccj_problem *prob, const ccj_pf_raw *raw, int device, int N, ccj_pf_ctx *c) {
    // N > 0: a capacity context, bound to prob->seq when it has one, else to poly-A of length N
    if (!prob) return pf_err(c, CCJ_E_ARG, "null problem");
    std::string seq = prob->seq ? prob->seq : "";
    if (N <= 0) N = (int)seq.size();
    else if (seq.empty()) seq.assign((size_t)std::min(N, 1023), 'A');
    if (N > 1023) return pf_err(c, CCJ_E_ARG, "sequence longer than 1023");
    int rc = check_seq(c, seq.c_str(), N);
    if (rc == CCJ_OK) rc = init_model(prob, raw, c);
    if (rc != CCJ_OK) return rc;
    {
        // Size check before any table is built (ccj_pf_footprint: the allocations below, summed).
        // Past what the GPU (or, for the host builder, the host) can hold, fail with CCJ_E_OOM up
        // front.  CCJ_PF_DEVMEM_LIMIT (bytes) stands in for the device's free memory (tests pin the
        // accept/reject boundary with it).
        unsigned long long dev_b = 0, host_b = 0;
        ccj_pf_footprint(N, &dev_b, &host_b);
        size_t dfree = 0, dtotal = 0;
        char msg[200];
        const char *lim = getenv("CCJ_PF_DEVMEM_LIMIT");
        if (lim && *lim) dfree = (size_t)strtoull(lim, nullptr, 10);
        else if (hipSetDevice(device) != hipSuccess || hipMemGetInfo(&dfree, &dtotal) != hipSuccess) dfree = SIZE_MAX;
        if ((double)dev_b > (double)dfree) {
            snprintf(msg, sizeof msg, "n=%d needs ~%.1f GB of device memory, %.1f GB free", N, dev_b / 1e9, dfree / 1e9);
            return pf_err(c, CCJ_E_OOM, msg);
        }
        // MemAvailable counts reclaimable page cache (sysconf(_SC_AVPHYS_PAGES) does not)
        unsigned long long avail_kb = 0;
        if (host_setup())
            if (FILE *f = fopen("/proc/meminfo", "r")) {
                char line[256];
                while (fgets(line, sizeof line, f))
                    if (sscanf(line, "MemAvailable: %llu kB", &avail_kb) == 1) break;
                fclose(f);
            }
        if (avail_kb > 0 && (double)host_b > (double)avail_kb * 1024.0) {
            snprintf(msg, sizeof msg, "n=%d needs ~%.1f GB of host memory for the interior-loop tables", N, host_b / 1e9);
            return pf_err(c, CCJ_E_OOM, msg);
        }
    }
    PfLayout YN, Y;
    if (!make_layout(N, YN) || !make_layout((int)seq.size(), Y)) return pf_err(c, CCJ_E_ARG, kPpushMsg);
    build_powers(c, N);
    rc = alloc_cap(c, N, device, YN);
    if (rc != CCJ_OK) return rc;
    set_seq_host(c, seq.c_str());
    rc = bind_len(c, Y);
    return rc != CCJ_OK ? rc : setup_seq(c);
}

// The host's end of a fill, over the copies of the 2-D planes (c->h2d) and of Pabs: the exactness
// check, W and the energy.  CCJ_E_PF_RANGE leaves the context without a fill.
int finish_fill(ccj_pf_ctx *c, const unsigned long long *pabs) {
    const int n = c->n;
    // the exact int64 P sums equal the reference's serial double sums only while every partial sum
    // is an exactly representable integer: guaranteed by sum |term| < 2^53 (part_func.cc:383-393)
    // CCJ_PF_RANGE_LOG2 lowers the 2^53 bound (tests only: reaches this exit with short sequences)
    unsigned long long range_lim = 1ull << 53;
    if (const char *e = getenv("CCJ_PF_RANGE_LOG2")) {
        const int l2 = atoi(e);
        if (l2 >= 1 && l2 <= 53) range_lim = 1ull << l2;
    }
    for (int w = 0; w < n; ++w)
        for (int p = 1; p + w <= n; ++p)
            if (pabs[(size_t)w * c->rs + p] >= range_lim) {
                char msg[160];
                snprintf(msg, sizeof msg, "P(%d,%d): sum of |terms| >= 2^53, the reference's double sum may round", p, p + w);
                return pf_err(c, CCJ_E_PF_RANGE, msg);
            }
    // W (part_func.cc:163-172)
    c->W.assign(n + 1, 1.0);  // W.resize(n+1, scale[1])
    for (int j = TURN + 1; j <= n; ++j) {
        double s = 0;
        s += c->W[j - 1] * 1.0;
        for (int k = 1; k <= j - TURN - 1; ++k) {
            const double acc = (k > 1) ? c->W[k - 1] : 1;
            s += acc * c->g2(CCJ_PF_V, k, j) * ext_pf(*c, k, j);
            s += acc * c->g2(CCJ_PF_P, k, j) * c->E.PS;
        }
        c->W[j] = s;
    }
    // to_Energy (part_func.cc:148-150)
    c->energy = (-log(c->W[n]) - n * log(c->E.pf_scale)) * c->E.kT / 1000.0;
    c->filled = true;
    return CCJ_OK;
}

int fill_impl(ccj_pf_ctx *c) {
    const int n = c->n;
    const size_t plane = c->plane();
    c->filled = false;  // a failed re-fill must not leave the previous fill's tables looking valid
    PFCHK(c, hipSetDevice(c->device));
    PFCHK(c, hipMemsetAsync(c->d_2d, 0, (size_t)CCJ_PF_NMAT2 * plane * sizeof(double), c->st));
    PFCHK(c, hipMemsetAsync(c->d_Pacc, 0, plane * sizeof(long long), c->st));
    PFCHK(c, hipMemsetAsync(c->d_Pabs, 0, plane * sizeof(unsigned long long), c->st));
    PFCHK(c, hipEventRecord(c->e0, c->st));
    // level t needs the 2-D spans <= t-1; span s needs P(s), i.e. the levels <= s-3
    // timed launches: an event pair from the context's pool around each (ccj_pf_set_timing)
    c->tfam.clear();
    auto launch = [&](int fam, hipStream_t s, auto &&go) -> hipError_t {
        const size_t q = c->tfam.size();
        if (c->timing) {
            while (c->tev.size() < 2 * q + 2) {
                hipEvent_t e;
                const hipError_t r = hipEventCreate(&e);
                if (r != hipSuccess) return r;
                c->tev.push_back(e);
            }
            c->tfam.push_back(fam);
            const hipError_t r = hipEventRecord(c->tev[2 * q], s);
            if (r != hipSuccess) return r;
        }
        const hipError_t e = (hipError_t)go();
        if (e != hipSuccess || !c->timing) return e;
        return hipEventRecord(c->tev[2 * q + 1], s);
    };
    // Three streams: level t needs k_pf_iloop(t) and the spans <= t-1; k_pf_iloop(t)
    // reads the copies of levels <= t-2 and refills the R buffer level t-2 read; P(s) needs the
    // levels <= s-3 and span s the spans < s.  So iloop(t) and the span s = t+1 (with its P terms)
    // run beside level t-1, off the level chain.  Every event is recorded before a wait on it is
    // enqueued (host order below).
    const int nl = n - 2;  // levels 0 .. n-3
    // P(s): pushed by level (k_pf_ppush(s-3) completes it, after every earlier push on this stream),
    // or pulled per span (k_pf_pterm, CCJ_PF_PULL=1)
    const bool pull = getenv("CCJ_PF_PULL") && atoi(getenv("CCJ_PF_PULL")) != 0;
    auto span = [&](int s) -> hipError_t {
        hipError_t e = launch(2, c->st_d, [&] {
            return pull ? ccjk_pf_pterm(&c->D, s, c->st_d) : s >= 3 ? ccjk_pf_ppush(&c->D, s - 3, c->st_d) : 0;
        });
        if (e == hipSuccess) e = launch(3, c->st_d, [&] { return ccjk_pf_diag(&c->D, s, c->st_d); });
        return e != hipSuccess ? e : hipEventRecord(c->ev_dg[s], c->st_d);
    };
    auto iloop = [&](int t) -> hipError_t {
        const long long f = c->ifirst[t];
        const hipError_t e = launch(0, c->st_il, [&] { return ccjk_pf_iloop(&c->D, t, f, (int)(c->ifirst[t + 1] - f), c->st_il); });
        return e != hipSuccess ? e : hipEventRecord(c->ev_il[t], c->st_il);
    };
    PFCHK(c, hipEventRecord(c->ev_start, c->st));
    PFCHK(c, hipStreamWaitEvent(c->st_d, c->ev_start, 0));
    PFCHK(c, hipStreamWaitEvent(c->st_il, c->ev_start, 0));
    for (int s = 0; s <= std::min(2, n - 1); ++s) PFCHK(c, span(s));   // no P terms below span 3
    for (int t = 0; t <= std::min(1, nl - 1); ++t) PFCHK(c, iloop(t));
    for (int t = 0; t < nl; ++t) {
        PFCHK(c, hipStreamWaitEvent(c->st, c->ev_il[t], 0));
        if (t >= 1) PFCHK(c, hipStreamWaitEvent(c->st, c->ev_dg[t - 1], 0));
        PFCHK(c, launch(1, c->st, [&] { return ccjk_pf_level(&c->D, c->lv.data(), t, c->st); }));
        PFCHK(c, hipEventRecord(c->ev_lev[t], c->st));
        if (t + 2 < nl) {
            PFCHK(c, hipStreamWaitEvent(c->st_il, c->ev_lev[t], 0));
            PFCHK(c, iloop(t + 2));
        }
        if (t + 3 <= n - 1) {
            PFCHK(c, hipStreamWaitEvent(c->st_d, c->ev_lev[t], 0));
            PFCHK(c, span(t + 3));
        }
    }
    PFCHK(c, hipStreamWaitEvent(c->st, c->ev_dg[n - 1], 0));
    PFCHK(c, hipEventRecord(c->e1, c->st));
    c->h2d.assign((size_t)CCJ_PF_NMAT2 * plane, 0.0);
    PFCHK(c, hipMemcpyAsync(c->h2d.data(), c->d_2d, c->h2d.size() * sizeof(double), hipMemcpyDeviceToHost, c->st));
    std::vector<unsigned long long> pabs(plane, 0);
    PFCHK(c, hipMemcpyAsync(pabs.data(), c->d_Pabs, plane * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->st));
    PFCHK(c, hipStreamSynchronize(c->st));
    float fill_ms = 0;
    double kms[4] = {0, 0, 0, 0};
    PFCHK(c, hipEventElapsedTime(&fill_ms, c->e0, c->e1));
    for (size_t q = 0; q < c->tfam.size(); ++q) {
        float ms = 0;
        PFCHK(c, hipEventElapsedTime(&ms, c->tev[2 * q], c->tev[2 * q + 1]));
        kms[c->tfam[q]] += ms;
    }
    const int rc = finish_fill(c, pabs.data());
    if (rc != CCJ_OK) return rc;
    c->fill_ms = fill_ms;
    memcpy(c->kms, kms, sizeof kms);
    return CCJ_OK;
}

// ---------------------------------------------------------------------------------------------
// Lockstep batch (include/ccj_pf.h): K capacity contexts filled by one event graph.
// ---------------------------------------------------------------------------------------------
thread_local std::string g_batch_create_msg;

int batch_err(ccj_pf_batch *b, int code, const std::string &what, hipError_t e = hipSuccess) {
    b->msg = e == hipSuccess ? what : what + ": " + hipGetErrorString(e);
    return code;
}
#define PBCHK(b, x)                                                      \
    do {                                                                 \
        const hipError_t e_ = (x);                                       \
        if (e_ != hipSuccess) return batch_err((b), CCJ_E_HIP, #x, e_);  \
    } while (0)

void batch_free(ccj_pf_batch *b) {
    hipSetDevice(b->model.device);
    for (ccj_pf_ctx *c : b->mem) {
        free_dev(c);
        delete c;
    }
    b->mem.clear();
    if (b->d_D) hipFree(b->d_D);
    if (b->d_if) hipFree(b->d_if);
    if (b->h_D) hipHostFree(b->h_D);
    if (b->h_if) hipHostFree(b->h_if);
    free_dev(&b->model);
}

int batch_create_impl(const ccj_problem *prob, const ccj_pf_raw *raw, int device, int N, int K, ccj_pf_batch *b) {
    if (N > 1023) return batch_err(b, CCJ_E_ARG, "capacity above 1023");
    ccj_pf_ctx *m = &b->model;
    int rc = init_model(prob, raw, m);
    if (rc != CCJ_OK) return batch_err(b, rc, m->msg);
    PfLayout YN;
    if (!make_layout(N, YN)) return batch_err(b, CCJ_E_ARG, kPpushMsg);
    {   // the members' allocations and the shared tables against the free memory, before any of them
        unsigned long long dev_b = 0;
        ccj_pf_footprint(N, &dev_b, nullptr);
        const double need = (double)K * (double)dev_b + (double)PF_KEYS * sizeof(double) + sizeof(PfExp);
        size_t dfree = 0, dtotal = 0;
        const char *lim = getenv("CCJ_PF_DEVMEM_LIMIT");
        if (lim && *lim) dfree = (size_t)strtoull(lim, nullptr, 10);
        else if (hipSetDevice(device) != hipSuccess || hipMemGetInfo(&dfree, &dtotal) != hipSuccess) dfree = SIZE_MAX;
        if (need > (double)dfree) {
            char msg[200];
            snprintf(msg, sizeof msg, "%d members of capacity %d need ~%.1f GB of device memory, %.1f GB free", K, N, need / 1e9,
                     dfree / 1e9);
            return batch_err(b, CCJ_E_OOM, msg);
        }
    }
    build_powers(m, N);
    rc = alloc_model(m, N, device);
    if (rc != CCJ_OK) return batch_err(b, rc, m->msg);
    const std::string polyA((size_t)N, 'A');
    PfLayout Y1;
    make_layout(1, Y1);
    for (int k = 0; k < K; ++k) {
        ccj_pf_ctx *c = new ccj_pf_ctx();
        b->mem.push_back(c);
        c->batch = b;
        initstate_r(1, c->rnd_state, sizeof c->rnd_state, &c->rnd);
        // the model on the host: a member evaluates hairpins, W and samples with its own copy
        c->dangles = m->dangles;
        c->noGU = m->noGU;
        c->prm = m->prm;
        c->pen = m->pen;
        memcpy(c->pair, m->pair, sizeof c->pair);
        memcpy(c->rtype, m->rtype, sizeof c->rtype);
        c->E = m->E;
        c->mlb = m->mlb;
        c->cpp = m->cpp;
        c->pup = m->pup;
        rc = alloc_cap(c, N, device, YN, m);
        if (rc != CCJ_OK) return batch_err(b, rc, c->msg);
        // until the first bind a member stands at length 1, without a fill
        set_seq_host(c, "A");
        rc = bind_len(c, Y1);
        if (rc == CCJ_OK) rc = setup_seq(c);
        if (rc != CCJ_OK) return batch_err(b, rc, c->msg);
    }
    b->stride = N + 1;
    PBCHK(b, hipMalloc((void **)&b->d_D, (size_t)K * sizeof(PfDev)));
    PBCHK(b, hipMalloc((void **)&b->d_if, (size_t)K * b->stride * sizeof(long long)));
    PBCHK(b, hipHostMalloc((void **)&b->h_D, (size_t)K * sizeof(PfDev)));
    PBCHK(b, hipHostMalloc((void **)&b->h_if, (size_t)K * b->stride * sizeof(long long)));
    PBCHK(b, hipStreamSynchronize(m->st));
    return CCJ_OK;
}

int batch_bind_impl(ccj_pf_batch *b, const char *const *seqs, int count) {
    const int K = (int)b->mem.size(), N = b->model.cap;
    if (!seqs || count < 1 || count > K) return batch_err(b, CCJ_E_ARG, "ccj_pf_batch_bind: count must be 1..members");
    // every argument before any member is touched
    std::vector<PfLayout> Y((size_t)count);
    for (int k = 0; k < count; ++k) {
        const int rc = check_seq(&b->model, seqs[k], N);
        if (rc != CCJ_OK) return batch_err(b, rc, "member " + std::to_string(k) + ": " + b->model.msg);
        if (!make_layout((int)strlen(seqs[k]), Y[k])) return batch_err(b, CCJ_E_ARG, kPpushMsg);
    }
    hipStream_t st = b->model.st;
    PBCHK(b, hipSetDevice(b->model.device));
    b->count = 0;  // a failure below leaves the batch unbound
    for (ccj_pf_ctx *c : b->mem) c->filled = false;
    b->rc.assign(K, CCJ_E_STATE);
    for (int k = 0; k < count; ++k) {
        ccj_pf_ctx *c = b->mem[k];
        set_seq_host(c, seqs[k]);
        int rc = bind_len(c, Y[k]);
        if (rc == CCJ_OK) rc = setup_seq_a(c);
        if (rc != CCJ_OK) return batch_err(b, rc, c->msg);
    }
    PBCHK(b, hipStreamSynchronize(st));  // the one wait of a bind: every member's item counts
    memset(b->h_if, 0, (size_t)K * b->stride * sizeof(long long));
    b->n.assign(count, 0);
    b->nmax = 0;
    for (int k = 0; k < count; ++k) {
        ccj_pf_ctx *c = b->mem[k];
        const int rc = setup_seq_b(c);
        if (rc != CCJ_OK) return batch_err(b, rc, c->msg);
        b->n[k] = c->n;
        b->nmax = std::max(b->nmax, c->n);
        b->h_D[k] = c->D;
        // row k: ifirst[0 .. n-2] (the total behind the last level), the total again up to the row's end
        long long *row = b->h_if + (size_t)k * b->stride;
        const int last = std::max(c->n - 2, 0);
        for (int t = 0; t < b->stride; ++t) row[t] = c->n >= 3 ? c->ifirst[std::min(t, last)] : 0;
    }
    PBCHK(b, hipMemcpyAsync(b->d_D, b->h_D, (size_t)count * sizeof(PfDev), hipMemcpyHostToDevice, st));
    PBCHK(b, hipMemcpyAsync(b->d_if, b->h_if, (size_t)K * b->stride * sizeof(long long), hipMemcpyHostToDevice, st));
    b->count = count;
    return CCJ_OK;
}

int batch_items(const ccj_pf_batch *b, int k, int t) {
    const ccj_pf_ctx *c = b->mem[k];
    return t >= 0 && t <= c->n - 3 ? (int)(c->ifirst[t + 1] - c->ifirst[t]) : 0;
}

int batch_fill_impl(ccj_pf_batch *b) {
    if (b->count < 1) return batch_err(b, CCJ_E_STATE, "ccj_pf_batch_fill: no sequences bound");
    ccj_pf_ctx *g = &b->model;  // the batch's graph: its streams and events
    const int count = b->count, n = b->nmax;
    const int *ns = b->n.data();
    for (int k = 0; k < count; ++k) b->mem[k]->filled = false;
    b->rc.assign(b->mem.size(), CCJ_E_STATE);
    b->launches = 0;
    PBCHK(b, hipSetDevice(g->device));
    // every kernel launch of the fill goes through here
    auto launch = [&](auto &&go) -> hipError_t {
        int launched = 0;
        const hipError_t e = (hipError_t)go(&launched);
        b->launches += launched;
        return e;
    };
    PBCHK(b, launch([&](int *l) { *l = 1; return ccjk_pf_zero_many(b->d_D, n, count, g->st); }));
    PBCHK(b, hipEventRecord(g->e0, g->st));
    // fill_impl's graph for the longest member n: level t after k_pf_iloop(t) and the spans <= t-1;
    // k_pf_iloop(t+2) and the span t+3 (its P pushes first) after level t.  A shorter member's
    // levels and spans carry the same indices, so the same edges order them.
    const int nl = n - 2;
    std::vector<int> items((size_t)count);
    auto span = [&](int s) -> hipError_t {
        hipError_t e = hipSuccess;
        if (s >= 3) e = launch([&](int *l) { return ccjk_pf_ppush_many(b->d_D, ns, count, s - 3, g->st_d, l); });
        if (e == hipSuccess) e = launch([&](int *l) { return ccjk_pf_diag_many(b->d_D, ns, count, s, g->st_d, l); });
        return e != hipSuccess ? e : hipEventRecord(g->ev_dg[s], g->st_d);
    };
    auto iloop = [&](int t) -> hipError_t {
        for (int k = 0; k < count; ++k) items[k] = batch_items(b, k, t);
        const hipError_t e = launch([&](int *l) {
            return ccjk_pf_iloop_many(b->d_D, ns, items.data(), count, b->d_if, b->stride, t, g->st_il, l);
        });
        return e != hipSuccess ? e : hipEventRecord(g->ev_il[t], g->st_il);
    };
    PBCHK(b, hipEventRecord(g->ev_start, g->st));
    PBCHK(b, hipStreamWaitEvent(g->st_d, g->ev_start, 0));
    PBCHK(b, hipStreamWaitEvent(g->st_il, g->ev_start, 0));
    for (int s = 0; s <= std::min(2, n - 1); ++s) PBCHK(b, span(s));
    for (int t = 0; t <= std::min(1, nl - 1); ++t) PBCHK(b, iloop(t));
    for (int t = 0; t < nl; ++t) {
        PBCHK(b, hipStreamWaitEvent(g->st, g->ev_il[t], 0));
        if (t >= 1) PBCHK(b, hipStreamWaitEvent(g->st, g->ev_dg[t - 1], 0));
        PBCHK(b, launch([&](int *l) { return ccjk_pf_level_many(b->d_D, ns, count, t, g->st, l); }));
        PBCHK(b, hipEventRecord(g->ev_lev[t], g->st));
        if (t + 2 < nl) {
            PBCHK(b, hipStreamWaitEvent(g->st_il, g->ev_lev[t], 0));
            PBCHK(b, iloop(t + 2));
        }
        if (t + 3 <= n - 1) {
            PBCHK(b, hipStreamWaitEvent(g->st_d, g->ev_lev[t], 0));
            PBCHK(b, span(t + 3));
        }
    }
    PBCHK(b, hipStreamWaitEvent(g->st, g->ev_dg[n - 1], 0));
    PBCHK(b, hipEventRecord(g->e1, g->st));
    std::vector<std::vector<unsigned long long>> pabs((size_t)count);
    for (int k = 0; k < count; ++k) {
        ccj_pf_ctx *c = b->mem[k];
        const size_t plane = c->plane();
        c->h2d.assign((size_t)CCJ_PF_NMAT2 * plane, 0.0);
        pabs[k].assign(plane, 0);
        PBCHK(b, hipMemcpyAsync(c->h2d.data(), c->d_2d, c->h2d.size() * sizeof(double), hipMemcpyDeviceToHost, g->st));
        PBCHK(b, hipMemcpyAsync(pabs[k].data(), c->d_Pabs, plane * sizeof(unsigned long long), hipMemcpyDeviceToHost, g->st));
    }
    PBCHK(b, hipStreamSynchronize(g->st));
    PBCHK(b, hipEventElapsedTime(&g->fill_ms, g->e0, g->e1));
    for (int k = 0; k < count; ++k) {
        ccj_pf_ctx *c = b->mem[k];
        c->fill_ms = g->fill_ms;
        b->rc[k] = finish_fill(c, pabs[k].data());  // CCJ_E_PF_RANGE: this member alone holds no fill
    }
    return CCJ_OK;
}

// ---------------------------------------------------------------------------------------------
// Stochastic traceback (stoch_backtrack.cc).  Each failure path of the reference prints a line and
// calls exit(0); here it is reported as CCJ_E_PF_SAMPLE with that line in ccj_pf_last_message.
// ---------------------------------------------------------------------------------------------
struct Sampler {
    ccj_pf_ctx &c;
    std::string &st;
    bool failed = false;

    double urn() {  // vrna_urn (utils.c:262-271) without HAVE_ERAND48
        int32_t r = 0;
        random_r(&c.rnd, &r);
        return ((double)r) / RAND_MAX;
    }
    double V(int i, int j) const { return c.g2(CCJ_PF_V, i, j); }
    double VM(int i, int j) const { return c.g2(CCJ_PF_VM, i, j); }
    double WM(int i, int j) const { return c.g2(CCJ_PF_WM, i, j); }
    double WMv(int i, int j) const { return c.g2(CCJ_PF_WMv, i, j); }
    double WMp(int i, int j) const { return c.g2(CCJ_PF_WMp, i, j); }
    double P(int i, int j) const { return c.g2(CCJ_PF_P, i, j); }
    void fail(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        c.msg = buf;
        failed = true;
    }

    // boustrophedon (stoch_backtrack.cc:17-34)
    static std::vector<int> bous(int start, int end) {
        std::vector<int> s;
        if (end >= start) {
            s.push_back(end - start + 1);
            for (int pos = 1; pos <= end - start + 1; ++pos) {
                const int count = pos - 1, adv = count / 2;
                s.push_back(start + (end - start) * (count % 2) + adv - (2 * (count % 2)) * adv);
            }
        }
        return s;
    }

    void W_(int start, int end) {  // :36-85
        if (failed) return;
        int j = end, m;
        double W_temp = 0;
        const std::vector<double> &W = c.W;
        if (end > start) {
            for (; j > start; --j) {
                W_temp = W[j - 1] * 1.0;
                const double r = urn() * W[j];
                if (r > W_temp) break;
            }
            if (j <= start + TURN) return;
            const double r = urn() * (W[j] - W_temp);
            const std::vector<int> is = bous(start, j - 1);
            const int bn = (int)is.size();
            double qt = 0;
            int k = start;
            bool pk = false;
            for (m = 1; m < bn; ++m) {
                k = is[m];
                const double acc = (k > 1) ? W[k - 1] : 1;
                double Wkl = acc * V(k, j) * ext_pf(c, k, j);
                qt += Wkl;
                if (qt > r) break;
                Wkl = acc * P(k, j) * c.E.PS;
                qt += Wkl;
                if (qt > r) {
                    pk = true;
                    break;
                }
            }
            if (k + start > j) {
                fail("backtracking failed in ext loop at %d and %d with W[j] = %f, qt:%f < r:%f\n", start, end, W[j], qt, r);
                return;
            }
            W_(start, k - 1);
            if (failed) return;
            if (!pk) V_(k, j);
            // else Sample_P (:323-326) is empty
        }
    }

    void V_(int i, int j) {  // :87-141
        if (failed) return;
        int k = i, l = j;
        st[i - 1] = '(';
        st[j - 1] = ')';
        const double qbr = V(i, j);
        const double r = urn() * qbr;
        double qbt1 = 0, V_temp = hairpin_pf(c, i, j);
        qbt1 += V_temp;
        if (qbt1 >= r) return;
        const int max_k = std::min(j - TURN - 2, i + MAXLOOP + 1);
        // stoch_backtrack.cc:112,119 read `pair` of ViennaRNA/pair_mat.h, a static array every
        // translation unit owns; only part_func.cc's copy is filled (make_pair_matrix in the
        // constructor), so here every pair type is 0 and rtype[0] is 0.
        const int tc = 0, t2 = 0;
        for (k = i + 1; k <= max_k; k++) {
            const int min_l = std::max(k + TURN + 1 + MAXLOOP + 2, k + j - i) - MAXLOOP - 2;
            for (l = j - 1; l >= min_l; --l) {
                const int u1 = k - i - 1, u2 = j - l - 1;
                V_temp = V(k, l) * exp_E_IntLoop_pf(c.E, u1, u2, tc, t2, c.S1[i + 1], c.S1[j - 1], c.S1[k - 1], c.S1[l + 1]);
                V_temp *= 1.0;
                qbt1 += V_temp;
                if (qbt1 >= r) break;
            }
            if (qbt1 >= r) break;
        }
        if (qbt1 >= r) {
            V_(k, l);
            return;
        }
        V_temp = VM(i, j);
        qbt1 += V_temp;
        if (qbt1 < r) {
            fail("Backtracking failed for pair (%d,%d)\n", i, j);
            return;
        }
        VM_(i, j);
    }

    void VM_(int i, int j) {  // :143-192
        if (failed) return;
        int k;
        double qt = 0;
        if ((i + 1) + 2 * TURN + 2 >= (j - 1)) {
            fail("backtracking impossible for VM[%d, %d]\n", i, j);
            return;
        }
        double V_temp;
        const double VM_inside = VM(i, j) / 1.0;
        const double r = urn() * VM_inside;
        bool unpaired = false, pk = false;
        const double mb = mbloop_pf(c, i, j), mc = c.E.MLclosing;
        for (k = i + 1; k <= j - TURN - 1; ++k) {
            V_temp = WM(i + 1, k - 1) * WMv(k, j - 1) * mb * mc;
            qt += V_temp;
            if (qt > r) break;
            V_temp = (WM(i + 1, k - 1) * WMp(k, j - 1) * mb * mc);
            qt += V_temp;
            if (qt > r) {
                pk = true;
                break;
            }
            V_temp = (c.mlb[k - i - 1] * WMp(k, j - 1) * mb * mc);
            qt += V_temp;
            if (qt > r) {
                unpaired = true;
                pk = true;
                break;
            }
        }
        if (k > j - TURN) {
            fail("backtracking failed for VM at i=%d and j =%d\n", i, j);
            return;
        }
        if (!unpaired) WM_(i + 1, k - 1);
        if (failed) return;
        if (!pk) WMv_(k, j - 1);
        else WMp_(k, j - 1);
    }

    void WM_(int i, int j) {  // :193-272
        if (failed) return;
        int k;
        double qt = 0, qbt1 = 0, qbt2 = 0, V_temp = 0;
        bool unpaired = false, pk = false;
        if (i + TURN >= j) {
            fail("backtracking impossible for WM[%u, %u]\n", (unsigned)i, (unsigned)j);
            return;
        }
        for (; j > i + TURN; --j) {
            const double r = urn() * (WM(i, j));
            V_temp = WM(i, j - 1) * c.mlb[1];
            qt = V_temp;
            if (r > qt) break;
        }
        if (i + TURN == j) {
            fail("backtracking failed for WM\n");
            return;
        }
        qt = 0.;
        const double qm_rem = WM(i, j) - V_temp;
        const double r = urn() * qm_rem;
        for (k = i; k < j - TURN; ++k) {
            qbt1 = V(k, j) * mlstem_pf(c, k, j);
            qbt2 = P(k, j) * c.E.PSM * c.E.b;
            V_temp = c.mlb[k - i] * qbt1;
            qt += V_temp;
            if (qt >= r) {
                unpaired = true;
                break;
            }
            V_temp = c.mlb[k - i] * qbt2;
            qt += V_temp;
            if (qt >= r) {
                unpaired = true;
                pk = true;
                break;
            }
            V_temp = WM(i, k - 1) * qbt1;
            qt += V_temp;
            if (qt >= r) break;
            V_temp = WM(i, k - 1) * qbt2;
            qt += V_temp;
            if (qt >= r) {
                pk = true;
                break;
            }
        }
        if (k > j - TURN || qt < r) {
            fail("backtracking failed for WM at i=%d and j =%d with k=%d, qt=%f and r =%f and qt<r=%d\n", i, j, k, qt, r,
                 qt < r);
            return;
        }
        if (!unpaired) WM_(i, k - 1);
        if (failed) return;
        if (!pk) V_(k, j);
    }

    void WMv_(int i, int j) {  // :273-296
        if (failed) return;
        double qt = 0, V_temp = 0;
        (void)qt;
        for (; j > i + TURN; --j) {
            const double r = urn() * WMv(i, j);
            V_temp = WMv(i, j - 1) * c.mlb[1];
            qt = V_temp;
            if (r > qt) break;
        }
        if (i + TURN == j) {
            fail("backtracking failed for WMV\n");
            return;
        }
        V_(i, j);
    }

    void WMp_(int i, int j) {  // :298-321
        if (failed) return;
        double qt = 0, V_temp = 0;
        (void)qt;
        for (; j > i + TURN; --j) {
            const double r = urn() * WMp(i, j);
            V_temp = WMp(i, j - 1) * c.mlb[1];
            qt = V_temp;
            if (r > qt) break;
        }
        if (i + TURN == j) {
            fail("backtracking failed for WMP\n");
            return;
        }
        // Sample_P(i, j) is empty (:323-326)
    }
};

int exp_hashes(const PfExp &P, const ccj_energy_params &prm, uint64_t *out);

}  // namespace

extern "C" {

static int create_any(const ccj_problem *prob, const ccj_pf_raw *raw, int device, int N, ccj_pf_ctx **out) {
    if (!out) return CCJ_E_ARG;
    *out = nullptr;
    ccj_pf_ctx *c = new (std::nothrow) ccj_pf_ctx();
    if (!c) return CCJ_E_OOM;
    initstate_r(1, c->rnd_state, sizeof c->rnd_state, &c->rnd);
    int rc;
    try {
        rc = create_impl(prob, raw, device, N, c);
    } catch (const std::bad_alloc &) {  // host tables: no exception crosses the C ABI
        rc = pf_err(c, CCJ_E_OOM, "host allocation failed");
    }
    if (rc != CCJ_OK) {
        fprintf(stderr, "ccj_pf_create: %s\n", c->msg.c_str());
        free_dev(c);
        delete c;
        return rc;
    }
    *out = c;
    return CCJ_OK;
}

int ccj_pf_create(const ccj_problem *prob, const ccj_pf_raw *raw, int device, ccj_pf_ctx **out) {
    if (!prob || !prob->seq) return CCJ_E_ARG;
    return create_any(prob, raw, device, 0, out);
}

int ccj_pf_create_cap(const ccj_problem *prob, const ccj_pf_raw *raw, int device, int capacity, ccj_pf_ctx **out) {
    if (capacity < 1) return CCJ_E_ARG;
    return create_any(prob, raw, device, capacity, out);
}

static const char *const kMemberMsg = "the context is a lockstep batch's member: the batch binds and fills it";

int ccj_pf_rebind(ccj_pf_ctx *c, const char *seq) {
    if (!c) return CCJ_E_ARG;
    if (c->batch) return pf_err(c, CCJ_E_STATE, kMemberMsg);
    try {
        return rebind_impl(c, seq);
    } catch (const std::bad_alloc &) {
        return pf_err(c, CCJ_E_OOM, "host allocation failed");
    }
}

int ccj_pf_reset(ccj_pf_ctx *c, const char *seq) {
    if (!c) return CCJ_E_ARG;
    if (c->batch) return pf_err(c, CCJ_E_STATE, kMemberMsg);
    if (!seq || strlen(seq) != (size_t)c->n) return pf_err(c, CCJ_E_ARG, "ccj_pf_reset: the sequence must have the bound length");
    return ccj_pf_rebind(c, seq);
}

int ccj_pf_capacity(const ccj_pf_ctx *c) { return c ? c->cap : 0; }
int ccj_pf_n(const ccj_pf_ctx *c) { return c ? c->n : 0; }

int ccj_pf_keytab_info(const ccj_pf_ctx *c, double *build_ms, unsigned long long *bytes) {
    if (!c) return CCJ_E_ARG;
    if (build_ms) *build_ms = c->keytab_ms;
    if (bytes) *bytes = (unsigned long long)PF_KEYS * sizeof(double) + sizeof c->esttab;
    return CCJ_OK;
}

// pt, est, hp, items (with ifirst), then per pairing interval ieO, ieI, mO, mI: 8 hashes of the
// bound sequence's setup tables as they stand on the device.
int ccj_pf_setup_hashes(ccj_pf_ctx *c, uint64_t *out, int cap) {
    if (!c || !out || cap < 8) return CCJ_E_ARG;
    const size_t plane = c->plane();
    constexpr size_t W2 = PF_IEW * PF_IEW;
    try {
        std::vector<int8_t> pt(plane);
        std::vector<double> est(plane), hp(plane), ieO(W2 * plane), ieI(W2 * plane);
        std::vector<uint32_t> mO(plane * PF_IEW), mI(plane * PF_IEW);
        const long long ni = c->ifirst[std::max(c->n - 2, 1)];
        std::vector<uint32_t> items((size_t)std::max(ni, 1LL), 0u);
        PFCHK(c, hipSetDevice(c->device));
        PFCHK(c, hipStreamSynchronize(c->st));
        PFCHK(c, hipMemcpy(pt.data(), c->d_pt, plane, hipMemcpyDeviceToHost));
        PFCHK(c, hipMemcpy(est.data(), c->d_est, plane * sizeof(double), hipMemcpyDeviceToHost));
        PFCHK(c, hipMemcpy(hp.data(), c->d_hp, plane * sizeof(double), hipMemcpyDeviceToHost));
        PFCHK(c, hipMemcpy(ieO.data(), c->d_ieO, ieO.size() * sizeof(double), hipMemcpyDeviceToHost));
        PFCHK(c, hipMemcpy(ieI.data(), c->d_ieI, ieI.size() * sizeof(double), hipMemcpyDeviceToHost));
        PFCHK(c, hipMemcpy(mO.data(), c->d_mO, mO.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        PFCHK(c, hipMemcpy(mI.data(), c->d_mI, mI.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (ni > 0) PFCHK(c, hipMemcpy(items.data(), c->d_items, (size_t)ni * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint64_t h5[5];
        setup_table_hashes(*c, pt.data(), est.data(), ieO.data(), ieI.data(), mO.data(), mI.data(), h5);
        out[0] = fnv_arr(pt.data(), plane);
        out[1] = h5[0];
        out[2] = fnv_arr(hp.data(), plane);
        uint64_t hi = fnv_init();
        fnv_bytes(hi, c->ifirst.data(), c->ifirst.size() * sizeof(long long));
        fnv_bytes(hi, items.data(), (size_t)ni * sizeof(uint32_t));
        out[3] = hi;
        for (int q = 0; q < 4; ++q) out[4 + q] = h5[1 + q];
    } catch (const std::bad_alloc &) {
        return pf_err(c, CCJ_E_OOM, "host allocation failed");
    }
    return CCJ_OK;
}

// Host only (no GPU): the hashes of setup_table_hashes (est, ieO, ieI, mO, mI) of a problem, built
// with one pow per entry (direct) and through the key tables and the shared gathers (keyed).
int ccj_pf_setup_host_hashes(const ccj_problem *prob, const ccj_pf_raw *raw, uint64_t *direct5, uint64_t *keyed5) {
    if (!prob || !prob->seq || !direct5 || !keyed5) return CCJ_E_ARG;
    try {
        ccj_pf_ctx c;
        int rc = check_seq(&c, prob->seq, 0);
        if (rc == CCJ_OK) rc = init_model(prob, raw, &c);
        if (rc != CCJ_OK) return rc;
        set_seq_host(&c, prob->seq);
        {
            PfHostTabs T;
            host_tables(c, T);
            setup_table_hashes(c, T.pt.data(), T.est.data(), T.ieO.data(), T.ieI.data(), T.mO.data(), T.mI.data(), direct5);
        }
        std::vector<double> ietab;
        double esttab[64];
        build_keytab(c, c.n, ietab, esttab);
        PfHostTabs T;
        keyed_tables(c, ietab.data(), esttab, T);
        setup_table_hashes(c, T.pt.data(), T.est.data(), T.ieO.data(), T.ieI.data(), T.mO.data(), T.mI.data(), keyed5);
    } catch (const std::bad_alloc &) {
        return CCJ_E_OOM;
    }
    return CCJ_OK;
}

void ccj_pf_destroy(ccj_pf_ctx *c) {
    if (!c || c->batch) return;  // a batch's member is freed by ccj_pf_batch_destroy
    hipSetDevice(c->device);
    free_dev(c);
    delete c;
}

int ccj_pf_batch_create(const ccj_problem *prob, const ccj_pf_raw *raw, int device, int capacity, int members,
                        ccj_pf_batch **out) {
    if (!out) return CCJ_E_ARG;
    *out = nullptr;
    if (!prob || capacity < 1 || members < 1) {
        g_batch_create_msg = "ccj_pf_batch_create: needs a problem, capacity >= 1 and members >= 1";
        return CCJ_E_ARG;
    }
    ccj_pf_batch *b = new (std::nothrow) ccj_pf_batch();
    if (!b) return CCJ_E_OOM;
    b->model.device = device;
    int rc;
    try {
        rc = batch_create_impl(prob, raw, device, capacity, members, b);
    } catch (const std::bad_alloc &) {
        rc = batch_err(b, CCJ_E_OOM, "host allocation failed");
    }
    if (rc != CCJ_OK) {
        g_batch_create_msg = b->msg;
        batch_free(b);
        delete b;
        return rc;
    }
    *out = b;
    return CCJ_OK;
}

int ccj_pf_batch_bind(ccj_pf_batch *b, const char *const *seqs, int count) {
    if (!b) return CCJ_E_ARG;
    try {
        return batch_bind_impl(b, seqs, count);
    } catch (const std::bad_alloc &) {
        return batch_err(b, CCJ_E_OOM, "host allocation failed");
    }
}

int ccj_pf_batch_fill(ccj_pf_batch *b) {
    if (!b) return CCJ_E_ARG;
    try {
        return batch_fill_impl(b);
    } catch (const std::bad_alloc &) {
        return batch_err(b, CCJ_E_OOM, "host allocation failed");
    }
}

int ccj_pf_batch_result(ccj_pf_batch *b, int k, double *energy) {
    if (!b || k < 0 || k >= b->count) return CCJ_E_ARG;
    if (b->rc[k] == CCJ_OK && energy) *energy = b->mem[k]->energy;
    return b->rc[k];
}

ccj_pf_ctx *ccj_pf_batch_member(ccj_pf_batch *b, int k) { return b && k >= 0 && k < (int)b->mem.size() ? b->mem[k] : nullptr; }
int ccj_pf_batch_members(const ccj_pf_batch *b) { return b ? (int)b->mem.size() : 0; }
int ccj_pf_batch_count(const ccj_pf_batch *b) { return b ? b->count : 0; }
double ccj_pf_batch_fill_ms(const ccj_pf_batch *b) { return b ? (double)b->model.fill_ms : 0.0; }
int ccj_pf_batch_launches(const ccj_pf_batch *b) { return b ? b->launches : 0; }

int ccj_pf_batch_item_counts(const ccj_pf_batch *b, int t, int *out) {
    if (!b || !out) return CCJ_E_ARG;
    for (int k = 0; k < b->count; ++k) out[k] = batch_items(b, k, t);
    return CCJ_OK;
}

const char *ccj_pf_batch_last_error(const ccj_pf_batch *b) { return b ? b->msg.c_str() : g_batch_create_msg.c_str(); }

void ccj_pf_batch_destroy(ccj_pf_batch *b) {
    if (!b) return;
    batch_free(b);
    delete b;
}

int ccj_pf_fill(ccj_pf_ctx *c, double *energy) {
    if (!c) return CCJ_E_ARG;
    if (c->batch) return pf_err(c, CCJ_E_STATE, kMemberMsg);
    const int rc = fill_impl(c);
    if (rc != CCJ_OK) return rc;
    if (energy) *energy = c->energy;
    return CCJ_OK;
}

int ccj_pf_W(ccj_pf_ctx *c, double *W) {
    if (!c || !W) return CCJ_E_ARG;
    if (!c->filled) return CCJ_E_STATE;
    memcpy(W, c->W.data(), c->W.size() * sizeof(double));
    return CCJ_OK;
}

int ccj_pf_get2(ccj_pf_ctx *c, int which, double *out) {
    if (!c || !out || which < 0 || which >= CCJ_PF_NMAT2) return CCJ_E_ARG;
    if (!c->filled) return CCJ_E_STATE;
    size_t q = 0;
    for (int i = 1; i <= c->n; ++i)
        for (int j = i; j <= c->n; ++j) out[q++] = c->g2(which, i, j);
    return CCJ_OK;
}

int ccj_pf_get4(ccj_pf_ctx *c, int x, int i, int j, int k, int l, int *out) {
    if (!c || !out || x < 0 || x >= CCJ_PF_NMAT4) return CCJ_E_ARG;
    if (!c->filled) return CCJ_E_STATE;
    if (!(i <= j && j < k - 1 && k <= l)) {  // Matrix4DPF::get (matrices.hh:258-263)
        *out = 0;
        return CCJ_OK;
    }
    if (i <= 0 || l > c->n) return CCJ_E_ARG;  // the reference's get_uc assert
    const int a = j - i, b = l - k, t = a + b, h = k - j - 2, m = c->n - t - 2;
    const PfLvl &L = c->lv[t];
    const long long off = L.lb + (long long)x * L.C + (long long)a * L.M + h * m - ((h * (h - 1)) >> 1) + i - 1;
    PFCHK(c, hipSetDevice(c->device));
    PFCHK(c, hipMemcpy(out, c->d_d4 + off, sizeof(int), hipMemcpyDeviceToHost));
    return CCJ_OK;
}

int ccj_pf_hashes(ccj_pf_ctx *c, uint64_t *h4, uint64_t *h2) {
    if (!c) return CCJ_E_ARG;
    if (!c->filled) return CCJ_E_STATE;
    const int n = c->n;
    if (h2) {
        for (int m = 0; m < CCJ_PF_NMAT2; ++m) {
            uint64_t h = fnv_init();
            for (int i = 1; i <= n; ++i)
                for (int j = i; j <= n; ++j) {
                    const double v = c->g2(m, i, j);
                    fnv_bytes(h, &v, 8);
                }
            h2[m] = h;
        }
    }
    if (h4) {
        // canonical (i, j, k) rows of l, gathered on the GPU
        std::vector<long long> rows;
        long long q = 0;
        for (int i = 1; i <= n; ++i)
            for (int j = i; j <= n; ++j)
                for (int k = j + 2; k <= n; ++k) {
                    rows.push_back(q);
                    rows.push_back(((long long)i << 40) | ((long long)j << 20) | k);
                    q += n - k + 1;
                }
        const int nrows = (int)(rows.size() / 2);
        long long *d_rows = nullptr;
        int *d_out = nullptr;
        PFCHK(c, hipSetDevice(c->device));
        PFCHK(c, hipMalloc((void **)&d_rows, std::max<size_t>(rows.size(), 1) * sizeof(long long)));
        hipError_t e = hipMalloc((void **)&d_out, std::max<long long>(q, 1) * sizeof(int));
        if (e != hipSuccess) {
            hipFree(d_rows);
            return pf_err(c, CCJ_E_OOM, "hash buffer", e);
        }
        std::vector<int> hbuf((size_t)std::max<long long>(q, 1));
        int rc = CCJ_OK;
        if ((e = hipMemcpy(d_rows, rows.data(), rows.size() * sizeof(long long), hipMemcpyHostToDevice)) != hipSuccess)
            rc = pf_err(c, CCJ_E_HIP, "hash rows", e);
        for (int x = 0; x < CCJ_PF_NMAT4 && rc == CCJ_OK; ++x) {
            if ((e = (hipError_t)ccjk_pf_canon(&c->D, x, d_rows, nrows, d_out, c->st)) != hipSuccess ||
                (e = hipMemcpyAsync(hbuf.data(), d_out, q * sizeof(int), hipMemcpyDeviceToHost, c->st)) != hipSuccess ||
                (e = hipStreamSynchronize(c->st)) != hipSuccess) {
                rc = pf_err(c, CCJ_E_HIP, "hash gather", e);
                break;
            }
            h4[x] = fnv_arr(hbuf.data(), (size_t)q);
        }
        hipFree(d_rows);
        hipFree(d_out);
        if (rc != CCJ_OK) return rc;
    }
    return CCJ_OK;
}

const char *ccj_pf_exp_names(void) { return kExpNames; }

int ccj_pf_exp_hashes(ccj_pf_ctx *c, uint64_t *out, int cap) {
    if (!c || !out || cap < kNExp) return CCJ_E_ARG;
    return exp_hashes(c->E, c->prm, out);
}

int ccj_pf_exp_hashes_params(const ccj_energy_params *prm, const ccj_pf_raw *raw, const ccj_pk_penalties *pen,
                             uint64_t *out, int cap) {
    if (!prm || !out || cap < kNExp || prm->magic != CCJ_PARAMS_MAGIC) return CCJ_E_ARG;
    if (raw && (raw->magic != CCJ_PF_RAW_MAGIC || raw->size_bytes != sizeof(ccj_pf_raw))) return CCJ_E_ARG;
    const ccj_pk_penalties defp = CCJ_PK_PENALTIES_DEFAULT;
    PfExp *E = new PfExp;
    build_exp(*prm, raw, pen ? *pen : defp, *E);
    const int q = exp_hashes(*E, *prm, out);
    delete E;
    return q;
}

}  // extern "C"

namespace {

int exp_hashes(const PfExp &P, const ccj_energy_params &prm, uint64_t *out) {
    int q = 0;
    out[q++] = fnv_arr(&P.stack[0][0], 64);
    out[q++] = fnv_arr(P.hairpin, 31);
    out[q++] = fnv_arr(P.bulge, 31);
    out[q++] = fnv_arr(P.internal57, 31);
    out[q++] = fnv_arr(P.ninio, 31);
    out[q++] = fnv_arr(&P.mismatchI[0][0][0], 200);
    out[q++] = fnv_arr(&P.mismatch1nI[0][0][0], 200);
    out[q++] = fnv_arr(&P.mismatch23I[0][0][0], 200);
    out[q++] = fnv_arr(&P.mismatchH[0][0][0], 200);
    out[q++] = fnv_arr(&P.mismatchM[0][0][0], 200);
    out[q++] = fnv_arr(&P.mismatchExt[0][0][0], 200);
    out[q++] = fnv_arr(&P.dangle5[0][0], 40);
    out[q++] = fnv_arr(&P.dangle3[0][0], 40);
    out[q++] = fnv_arr(&P.int11[0][0][0][0], 64 * 25);
    out[q++] = fnv_arr(&P.int21[0][0][0][0][0], 64 * 125);
    out[q++] = fnv_arr(&P.int22[0][0][0][0][0][0], 64 * 625);
    out[q++] = fnv_arr(P.MLintern, 8);
    const double sc[] = {P.TermAU, P.MLbase, P.MLclosing, P.kT, P.lxc, P.pf_scale};
    out[q++] = fnv_arr(sc, 6);
    out[q++] = fnv_arr(P.tetra, strnlen(prm.Tetraloops, sizeof prm.Tetraloops) / 7);
    out[q++] = fnv_arr(P.tri, strnlen(prm.Triloops, sizeof prm.Triloops) / 6);
    out[q++] = fnv_arr(P.hex, strnlen(prm.Hexaloops, sizeof prm.Hexaloops) / 9);
    const double pk[] = {P.PS, P.PSM, P.PSP, P.PB, P.PUP, P.PPS, P.a, P.b, P.c, P.ap, P.bp, P.cp};
    out[q++] = fnv_arr(pk, 12);
    return q;
}

}  // namespace

extern "C" {

int ccj_pf_srand(ccj_pf_ctx *c, unsigned int seed) {
    if (!c) return CCJ_E_ARG;
    return srandom_r(seed, &c->rnd) == 0 ? CCJ_OK : CCJ_E_ARG;
}

int ccj_pf_sample(ccj_pf_ctx *c, int nsamples, char *structures, int *done) {
    if (!c || nsamples < 0 || (nsamples > 0 && !structures)) return CCJ_E_ARG;
    if (done) *done = 0;
    if (!c->filled) return CCJ_E_STATE;
    const int n = c->n;
    for (int s = 0; s < nsamples; ++s) {
        std::string st(n, '.');
        Sampler S{*c, st};
        S.W_(1, n);
        if (S.failed) return CCJ_E_PF_SAMPLE;
        memcpy(structures + (size_t)s * (n + 1), st.c_str(), n + 1);
        if (done) *done = s + 1;
    }
    return CCJ_OK;
}

const char *ccj_pf_last_message(ccj_pf_ctx *c) { return c ? c->msg.c_str() : ""; }

int ccj_pf_timing(ccj_pf_ctx *c, float *fill_ms) {
    if (!c || !fill_ms) return CCJ_E_ARG;
    *fill_ms = c->fill_ms;
    return CCJ_OK;
}

int ccj_pf_set_timing(ccj_pf_ctx *c, int on) {
    if (!c) return CCJ_E_ARG;
    if (c->batch) return pf_err(c, CCJ_E_STATE, kMemberMsg);  // a batch's launches are not per member
    c->timing = on != 0;
    return CCJ_OK;
}

int ccj_pf_kernel_ms(ccj_pf_ctx *c, double *ms4) {
    if (!c || !ms4) return CCJ_E_ARG;
    for (int k = 0; k < 4; ++k) ms4[k] = c->kms[k];
    return CCJ_OK;
}

int ccj_pf_work_model(ccj_pf_ctx *c, double *bytes4) {
    if (!c || !bytes4) return CCJ_E_ARG;
    if (c->h_mO.empty()) {  // the items and masks live on the device: fetched on demand, kept until the next setup
        const size_t nm = c->plane() * PF_IEW;
        const long long ni = c->ifirst[std::max(c->n - 2, 1)];
        c->h_items.assign((size_t)std::max(ni, 1LL), 0u);
        c->h_mO.assign(nm, 0u);
        c->h_mI.assign(nm, 0u);
        PFCHK(c, hipSetDevice(c->device));
        PFCHK(c, hipStreamSynchronize(c->st));
        if (ni > 0) PFCHK(c, hipMemcpy(c->h_items.data(), c->d_items, (size_t)ni * sizeof(uint32_t), hipMemcpyDeviceToHost));
        PFCHK(c, hipMemcpy(c->h_mO.data(), c->d_mO, nm * sizeof(uint32_t), hipMemcpyDeviceToHost));
        PFCHK(c, hipMemcpy(c->h_mI.data(), c->d_mI, nm * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    const PfWork w = pf_work_model(*c);
    bytes4[0] = w.iloop;
    bytes4[1] = w.level;
    bytes4[2] = w.pterm;
    bytes4[3] = w.diag;
    return CCJ_OK;
}

}  // extern "C"
