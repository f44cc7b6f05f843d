// ccj_host.cc — host side of libccj_hip.so: context + HBM allocation, sequence tables,
// level-by-level kernel schedule on a HIP stream, overlapped D2H of finished levels into a
// pinned host mirror, the way out of a traceback (exit record to the reference's messages and
// return code) and the bracket emission.
//
// The traceback's node logic is ccj_traceback.h, restated from the reference so the output is
// bit-identical, including its quirks.  It runs on the GPU
// (ccj_backtrack.hip); with ccj_options::host_traceback the same logic runs here through a small
// host executor over the mirror (HostStore, HostExec).  This file restates:
//   W_final::ccj (exterior W + driver)   reference src/W_final.cc:58-105
//   W_final::fill_structure               reference src/W_final.cc:764-819
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <memory>
#include <stack>
#include <string>
#include <thread>
#include <vector>

#include "ccj.h"
#include "ccj_energy.h"
#include "ccj_engine.h"
#include "ccj_backtrack.h"
#include "ccj_traceback.h"
#include "ccj_items.h"
#include "ccj_ilprune.h"

using namespace ccj;

namespace {

const int BP_PAIR[8][8] = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 5, 0, 0, 5}, {0, 0, 0, 1, 0, 0, 0, 0},
                           {0, 0, 2, 0, 3, 0, 0, 0}, {0, 6, 0, 4, 0, 0, 0, 6}, {0, 0, 0, 0, 0, 0, 2, 0},
                           {0, 0, 0, 0, 0, 1, 0, 0}, {0, 6, 0, 0, 5, 0, 0, 0}};

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t count = 0;
};

}  // namespace

// In-process stand-in for the RCCL communicator (tests): world contexts, one host
// thread each, exchange through device-to-device copies with a host barrier around every level.
struct ccj_group {
    int world = 1;
    std::vector<ccj_ctx *> members;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    long gen = 0;
    bool broken = false;
    int busy = 0;  // members between taking the peers' send pointers and finishing their copies
    // the union of the members' range sites (fill_finish): fold k gathers in range_acc[k & 1]
    int range_acc[2] = {0, 0};
    // false when a member gave up (error or 120 s without the others)
    bool barrier() {
        std::unique_lock<std::mutex> lk(mu);
        if (broken) return false;
        const long g = gen;
        if (++arrived == world) {
            arrived = 0;
            ++gen;
            cv.notify_all();
            return true;
        }
        if (!cv.wait_for(lk, std::chrono::seconds(120), [&] { return gen != g || broken; }) || broken) {
            broken = true;
            cv.notify_all();
            return false;
        }
        return true;
    }
};

// timing events per level (timing mode 2): [0,1] k_diag2d, [2,3] k_iloop, [4,5] the level, [6] the
// edge exchange's start (band-sharded), [7,8] k_ppush, [9,10] the bulk exchange (band-sharded, st_x)
constexpr int TEV_PER = 11;

// What a fill's graph orders itself with: the side streams, the per-level events and
// the fill's start / setup / end.  A context that is no batch member owns one, a lockstep batch owns
// one for all its members.  The level stream stays with its owner (a context also sets up on it).
struct FillSync {
    hipStream_t st_p = nullptr, st_il = nullptr;
    std::vector<hipEvent_t> il_done, dg_done;  // k_iloop(t) / k_diag2d(sigma) finished
    std::vector<hipEvent_t> lev_done;
    std::vector<hipEvent_t> p_done;            // P(sigma) reduced
    hipEvent_t ev_start = nullptr, ev_pre = nullptr, ev_end = nullptr;
};

// Band-sharded exchange: what only a context with world > 1 that does not simulate
// has (ccj_ctx::exchanges); nothing in it exists for any other context.
struct Exchange {
    hipStream_t st_d = nullptr;          // k_diag2d, each span partitioned by rank
    hipStream_t st_x = nullptr;          // the bulk part of each level's exchange
    std::vector<hipEvent_t> bulk_done;   // level t complete on this rank (bulk part unpacked)
    std::vector<hipEvent_t> pp_done;     // this rank's P-term push of span sigma done (before the exchange)
    // in-process group: this rank's bulk slice packed / the peers' bulk slices copied (reused every level;
    // the group's barriers order each record before the peers' waits on it)
    hipEvent_t ev_bpacked = nullptr, ev_bcopied = nullptr;
    // per part (XCH_EDGE, XCH_BULK): own slice, world slices
    int16_t *d_send[2] = {nullptr, nullptr}, *d_recv[2] = {nullptr, nullptr};
    std::vector<int> xnmax[2];           // per level: the largest rank's block count of the part (slice = 22 x nmax x M + tail)
    ccj_group *lgroup = nullptr;         // in-process exchange between contexts (tests), else RCCL
    ncclComm_t comm = nullptr;           // the edge all-gathers (level stream)
    ncclComm_t comm_b = nullptr;         // the bulk all-gathers (st_x), split from comm: one communicator per stream
};

struct ccj_ctx {
    // problem
    int n = 0;
    std::string seq;
    int dangles = 2;
    int noGU = 0;
    ccj_energy_params prm{};
    Penalties pen{};
    double e_stP = 0.89, e_intP = 0.74;
    int pair[8][8]{};
    int rtype[8]{};
    std::vector<short> S, S1;
    std::vector<int> lx;
    int rs = 0;
    int device = 0;
    bool overlap = true;
    int world = 1, rank = 0, simulate = 0;  // band sharding
    bool host_tb = false;                   // W + traceback on the host over the mirror (else on the GPU)
    int split_target = 9216;                // k_level4d split heuristic (0: never split)
    bool share = true;                      // split-point sharing
    int share_edges = 1;                    // ... also in the columns with a short other gap (CCJ_SHARE_EDGES)
    // fill timing (ccj_set_timing, CCJ_LEVEL_TIMING): 0 = fill only; 1 = + level durations from the
    // lev_done events the fill records anyway (no extra packets); 2 = + a marker pair around every
    // kernel family launch (k_diag2d, k_iloop, the level span).  The markers of mode 2 are barrier
    // packets on the streams and cost ~3 ms per n=200 fill, so the default is 1.
    int level_timing = 1;
    bool exchanges() const { return world > 1 && !simulate; }  // band-sharded with an exchange

    // layout
    std::vector<LevelDesc> lv_host;     // device pointers
    std::vector<int64_t> lv_off;        // element offset of each level in d4 (nm4 slots per level)
    std::vector<int64_t> lv_offh;       // element offset of each level in the host mirror (NMAT4 slots)
    int64_t ncell = 0;                  // cells of the 4-D state per matrix, C(n+1, 4)
    int64_t total4 = 0;                 // elements of d4: nm4 * ncell
    bool full4 = false;                 // a full context: d4 has all 22 slots per level (DevTables::full4)
    int nm4 = NMAT_D4;                  // matrix slots per level in d4 (NMAT4 when full4; ccj_engine.h mslot)
    int nlev = 0;                       // levels with cells (0..n-3)
    // capacity (ccj_create_cap): the allocations hold any binding of 1 <= n <= ncap; cap_ext = their
    // element counts (ccj_layout_extents, as_capacity = 1)
    int ncap = 0;
    std::vector<long long> cap_ext;
    void *h_bind = nullptr;             // pinned staging of the leader lists (bind_layout)
    hipEvent_t ev_bind = nullptr;       // their upload has read the staging

    // device
    int16_t *d4 = nullptr;
    int16_t *d_ie = nullptr, *d_est = nullptr;
    int *d_hp = nullptr, *d_lx = nullptr, *d_err = nullptr;
    int8_t *d_pt = nullptr, *d_pair = nullptr, *d_rtype = nullptr;
    short *d_S = nullptr, *d_S1 = nullptr;
    ccj_energy_params *d_prm = nullptr;
    LevelDesc *d_lv = nullptr;
    long long *d_lb = nullptr;
    LvlDev *d_ld = nullptr;
    int16_t *d4x = nullptr, *pmx = nullptr;  // interior-loop copies of PL/PR and PM (IT_PAD into the allocations)
    int16_t *d4x_alloc = nullptr, *pmx_alloc = nullptr;
    rec_t *d_rec = nullptr;                  // loop records RA (8 bytes)
    rk_t *d_rk = nullptr;                    // loop records RK (8 bytes)
    rl_t *d_rl = nullptr;                    // loop records RL (4 bytes)
    int *d_cf = nullptr;                     // the nine PM / PO closed-form tables [w][p] (ccj_pmpo2d.h)
    int16_t *d_tab = nullptr;                // the six PL / PR multiloop tables [w][p] (ccj_mloop2d.h)
    uint2 *d_acc = nullptr;                  // partial-record ring (split-point sharing)
    int16_t *d_lord = nullptr;               // long-scan a-blocks per sharing level, longest first
    int *d_lord_off = nullptr;
    std::vector<int> lord_off;
    int2 *d_wbw = nullptr;                   // (WBP, WP) pairs [w][p]
    long long nrec = 0;
    long long nx = 0, npm = 0, xpad = 0, xspan = 0;
    LvlX *d_ldx = nullptr;
    uint2 *d_il = nullptr, *d_ilm = nullptr;
    int16_t *d_dummy = nullptr;
    uint32_t *d_items = nullptr;          // k_iloop work items, all levels back to back
    size_t items_cap = 0;
    long long *d_icount = nullptr, *d_ioff = nullptr;  // k_items: items per (t, r), first item
    long long *h_ioff = nullptr;          // pinned staging of it_off
    long long *h_icount = nullptr;        // pinned landing of the k_items counts (so the copy is asynchronous)
    void *h_stage = nullptr;              // pinned staging of the sequence tables
    hipEvent_t ev_stage = nullptr;        // the uploads from the staging (and h_ioff) are done
    std::vector<long long> it_off;        // first item of (level t, shard r) at t*world + r
    uint32_t *d_ilseg = nullptr, *d_ilmseg = nullptr;
    int *d2i = nullptr;       // 9 int 2-D arrays back to back: V WM WMv WMp P WBP WPP WB WP
    unsigned long long *d_pk = nullptr;  // P with its first split (k_pterm), [w][p]
    int *d_W = nullptr, *d_fpair = nullptr;  // device traceback outputs
    int *d_wterm = nullptr;                  // W's (k, j) terms [j][k] (ccjk_compute_W scratch)
    int8_t *d_ftype = nullptr;
    BtOut *d_btout = nullptr;
    std::vector<unsigned long long> h_pk;
    int8_t *d_vt = nullptr;
    hipStream_t st = nullptr, st_copy = nullptr;
    FillSync fs;   // none for a lockstep batch's member: the batch's runs its fill
    Exchange xch;  // exchanges() only
    std::vector<double> lev_ms_v, diag_ms_v, il_ms_v, xch_ms_v, xbulk_ms_v, pp_ms_v;
    std::vector<hipEvent_t> tev;  // timing events (TEV_PER per level): 2 per k_level4d, k_iloop, k_diag2d and k_ppush launch
    DevTables T{};

    // host mirror
    int16_t *h4 = nullptr;
    std::vector<int> h2i;     // same 9 arrays
    std::vector<int8_t> hvt;
    std::vector<int> hpt_h;   // pair type table [w][p] host copy (int): the binding's pair relation
    // the binding's constraint (include/ccj.h): fmask[i*(n+1)+j] = 1 for (i,j) in F, symmetric; empty:
    // none.  seq_setup folds it into pt / hpt_h, the one source of the relation for every reader
    std::vector<uint8_t> fmask;
    long long fcount = 0;     // ccj_constraint_count
    // pair[S[i]][S[j]] as the binding sees it, for any positions the reference may index
    int pair_at(int i, int j) const {
        if (i >= 1 && i <= j && j <= n) return hpt_h[(size_t)(j - i) * rs + i];
        if (j >= 1 && j < i && i <= n) return rtype[hpt_h[(size_t)(i - j) * rs + j]];
        return pair[S[i]][S[j]];  // a position outside the sequence (S[0], S[n+1]): the table itself
    }
    bool filled = false, mirrored = false, mirrored2d = false;
    bool pending = false;                 // a fill is enqueued and not yet finished (fill_finish)
    // the last fill's range sites (CCJ_RANGE_*) and whether they refuse its result
    // (CCJ_E_RANGE; not with CCJ_ALLOW_OUT_OF_RANGE=1)
    int range_flags = 0;
    bool range_refused = false;
    long range_gen = 0;                   // fills finished in an in-process group (ccj_group::range_acc)
    bool res_pending = false;             // W + traceback enqueued (result_enqueue), not yet read
    // a member of a lockstep batch (ccj_batch_create): the batch binds and folds it, its own rebind /
    // reset / fill calls are refused, and ccj_batch_wait leaves its traceback's outputs in the pinned
    // result buffers (res_ready), from where ccj_result reports them
    struct ccj_batch *batch = nullptr;
    bool member = false;  // set before create_impl: no fill streams or per-level events of its own (the batch has them)
    bool res_ready = false;
    hipEvent_t ev_res = nullptr;          // device traceback results copied to the pinned buffers
    int *hr_W = nullptr, *hr_fp = nullptr;  // pinned: W, f[].pair, f[].type, the exit record
    int8_t *hr_ft = nullptr;
    BtOut *hr_bo = nullptr;
    std::vector<int> W;

    double fill_ms = 0, level_ms = 0, diag_ms = 0, pre_ms = 0, il_ms = 0, pp_ms = 0;
    double sync_ms = 0, w_ms = 0, bt_ms = 0;  // host side of the last fold
    int bt_steps = 0;
    std::string err;

    // ---- host accessors (reference getter semantics) ----
    size_t a2(int i, int j) const { return (size_t)(j - i) * rs + i; }
    int hV(int i, int j) const { return h2i[0 * plane() + a2(i, j)]; }
    int plane() const { return (n + 1) * rs; }
    int raw2(int which, int i, int j) const { return h2i[(size_t)which * plane() + a2(i, j)]; }
};

namespace {

int set_err(ccj_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    c->err = buf;
    return code;
}

#define HIPCHK(ctx, x)                                                                                   \
    do {                                                                                                 \
        hipError_t e_ = (x);                                                                             \
        if (e_ != hipSuccess) return set_err((ctx), CCJ_E_HIP, "%s: %s", #x, hipGetErrorString(e_));     \
    } while (0)
// inside a function that returns the hipError_t itself (the caller reports it: HIPCHK, BHIP)
#define HIPTRY(x)                                  \
    do {                                           \
        const hipError_t e_ = (hipError_t)(x);     \
        if (e_ != hipSuccess) return e_;           \
    } while (0)

// The cross-stream events only order work on one device, so they are recorded without the default
// system-scope fence (hipEventDisableSystemFence: fill -0.65 ms at n=200).  ev_start /
// ev_pre / ev_end, which the host waits on or times, keep it.  timed_levels: lev_done can be timed
// (a context's level durations, timing mode 1; recording them untimed measured the same).
constexpr unsigned EV_ORDER_TIMED = (unsigned)hipEventDisableSystemFence, EV_ORDER = hipEventDisableTiming | EV_ORDER_TIMED;
hipError_t fill_sync_create(FillSync &f, size_t nev, bool timed_levels) {
    HIPTRY(hipStreamCreateWithFlags(&f.st_p, hipStreamNonBlocking));
    HIPTRY(hipStreamCreateWithFlags(&f.st_il, hipStreamNonBlocking));
    for (auto *v : {&f.il_done, &f.dg_done, &f.lev_done, &f.p_done}) {
        v->assign(nev, nullptr);
        for (auto &e : *v) HIPTRY(hipEventCreateWithFlags(&e, timed_levels && v == &f.lev_done ? EV_ORDER_TIMED : EV_ORDER));
    }
    for (hipEvent_t *e : {&f.ev_start, &f.ev_pre, &f.ev_end}) HIPTRY(hipEventCreate(e));
    return hipSuccess;
}

// after the owner has synchronised the streams
void fill_sync_destroy(FillSync &f) {
    for (auto *v : {&f.il_done, &f.dg_done, &f.lev_done, &f.p_done})
        for (hipEvent_t e : *v)
            if (e) hipEventDestroy(e);
    for (hipEvent_t e : {f.ev_start, f.ev_pre, f.ev_end})
        if (e) hipEventDestroy(e);
    for (hipStream_t q : {f.st_p, f.st_il})
        if (q) hipStreamDestroy(q);
}

// --------------------------------------------------------------------------------------------
// host energy helpers
// --------------------------------------------------------------------------------------------
int E_Hairpin_host(const ccj_energy_params *P, const int *lx, int size, int type, int si1, int sj1,
                   const char *string) {
    // reference ViennaRNA/loops/hairpin.h:148-200
    int energy;
    if (size <= 30) energy = P->hairpin[size];
    else energy = P->hairpin[30] + lx[size];
    if (size < 3) return energy;
    if (string && P->special_hp) {
        if (size == 4) {
            char tl[7] = {0};
            memcpy(tl, string, 6);
            if (const char *ts = strstr(P->Tetraloops, tl)) return P->Tetraloop_E[(ts - P->Tetraloops) / 7];
        } else if (size == 6) {
            char tl[9] = {0};
            memcpy(tl, string, 8);
            if (const char *ts = strstr(P->Hexaloops, tl)) return P->Hexaloop_E[(ts - P->Hexaloops) / 9];
        } else if (size == 3) {
            char tl[6] = {0};
            memcpy(tl, string, 5);
            if (const char *ts = strstr(P->Triloops, tl)) return P->Triloop_E[(ts - P->Triloops) / 6];
            return energy + (type > 2 ? P->TerminalAU : 0);
        }
    }
    energy += P->mismatchH[type][si1][sj1];
    return energy;
}

// --------------------------------------------------------------------------------------------
// Host executor of the traceback (ccj_traceback.h): the host mirror as its Store, scans as
// sequential loops.  A test-only option (ccj_options::host_traceback); the device executor is
// ccj_backtrack.hip.
// --------------------------------------------------------------------------------------------
struct HostStore {
    const ccj_ctx *c;
    int n;
    const short *S, *S1;
    const int *W;

    explicit HostStore(const ccj_ctx *cc) : c(cc), n(cc->n), S(cc->S.data()), S1(cc->S1.data()), W(cc->W.data()) {}
    int pr(int i, int j) const { return c->pair_at(i, j); }
    int rt(int type) const { return c->rtype[type]; }
    const ccj_energy_params *prm() const { return &c->prm; }
    const int *lx() const { return c->lx.data(); }
    const Penalties &pen() const { return c->pen; }
    int dangles() const { return c->dangles; }
    double est() const { return c->e_stP; }
    double eint() const { return c->e_intP; }
    int raw2(int which, int i, int j) const { return c->raw2(which, i, j); }
    int Vtype(int i, int j) const { return c->hvt[c->a2(i, j)]; }
    int raw4(int x, int i, int j, int k, int l) const {
        const int t = (j - i) + (l - k);
        return (int)c->h4[c->lv_offh[t] + cell_offset_host(c->lv_host[t], x, j - i, k - j - 2, i)];
    }
    unsigned pk(int i, int l) const { return (unsigned)(c->h_pk[c->a2(i, l)] & 0xffffffffull); }
};
using MirrorView = View<HostStore>;

// W (W_final.cc:68-79)
void compute_W(ccj_ctx *c) {
    const int n = c->n;
    c->W.assign(n + 1, 0);
    const MirrorView H{HostStore(c)};
    std::vector<int> &W = c->W;
    for (int j = TURN + 1; j <= n; j++) {
        int m1 = W[j - 1], m2 = INF, m3 = INF;
        for (int k = 1; k <= j - TURN - 1; ++k) {
            const int acc = (k > 1) ? W[k - 1] : 0;
            m2 = std::min(m2, acc + E_ext_Stem(H, H.V(k, j), H.V(k + 1, j), H.V(k, j - 1), H.V(k + 1, j - 1), k, j));
            m3 = std::min(m3, acc + std::min({H.Pg(k, j), H.Pg(k + 1, j), H.Pg(k, j - 1), H.Pg(k + 1, j - 1)}) + c->pen.PS);
        }
        W[j] = std::min({m1, m2, m3});
    }
}

struct HostExec {
    const MirrorView &H;
    std::vector<Interval> stk;  // LIFO; back() is the top (reference insert_node pushes on the head)
    std::vector<int> f_pair;    // h_struct.hh:9-19
    std::vector<int8_t> f_type;
    BtOut st{};

    // first strict minimum over candidates [0, count) in order
    template <class F>
    void scan(int count, F f, int &bv, int &bx) {
        bv = bx = BIG;
        for (int c = 0; c < count; ++c) {
            const int t = f(c);
            if (t < bv) {
                bv = t;
                bx = c;
            }
        }
    }
    template <class F>
    void scan2(int count, F f, int &fmin, int &bv, int &bx) {
        fmin = BIG;
        scan(count, [&](int c) {
            const Int2 t = f(c);
            fmin = std::min(fmin, t.y);
            return t.x;
        }, bv, bx);
    }
    void push(int i, int j, int k, int l, int type) { stk.push_back(Interval{i, j, k, l, type}); }
    void setpair(int p, int q) {
        f_pair[p] = q;
        f_pair[q] = p;
    }
    void pairup(int p, int q, int type) {
        setpair(p, q);
        f_type[p] = f_type[q] = (int8_t)type;
    }
};

// W_final.cc:84-99: the driver loop, ended like the device's (k_backtrack)
BtOut host_backtrack(const ccj_ctx *c, std::vector<int> &f_pair) {
    const MirrorView H{HostStore(c)};
    HostExec X{H, {}, std::vector<int>(c->n + 1, -1), std::vector<int8_t>(c->n + 1, (int8_t)T_NONE)};
    Traceback<HostExec> B(X);
    X.push(1, c->n, 0, 0, FREE);
    while (!X.stk.empty() && X.st.status == BT_OK) {
        if (X.st.steps >= BT_MAX_STEPS) {
            X.st.status = BT_STEPS;
            break;
        }
        const Interval cur = X.stk.back();
        X.stk.pop_back();
        ++X.st.steps;
        B.node(cur);
        if (H.bad) X.st.status = BT_ASSERT;
    }
    f_pair.swap(X.f_pair);
    return X.st;
}

int bt_stack_cap(int n) { return std::min(4 * n + 64, 3000); }  // device node stack entries

// The one way out of a traceback, device or host: the BtOut record as the reference's stdout lines
// (appended to out), its stderr text (c->err) and the return code.
int bt_exit(ccj_ctx *c, const BtOut &bo, std::string &out) {
    for (int x = 0; x < bo.n_snbh; ++x) out += "Should not be here!\n";
    switch (bo.status) {
        case BT_OK: return CCJ_OK;
        case BT_DIE:
            c->err = std::string(bt_prefix(bo.prefix)) + "This should not have happened!, " + bt_case_name(bo.node) + "\n";
            return CCJ_E_BACKTRACK;
        case BT_INTER: {
            char buf[160];
            snprintf(buf, sizeof buf, "NOT GOOD RESTR INTER, i=%d, j=%d, best_ip=%d, best_jp=%d\n", bo.args[0], bo.args[1],
                     bo.args[2], bo.args[3]);
            c->err = buf;
            return CCJ_E_INTER_EXIT;
        }
        case BT_ASSERT:
            c->err = "CCJ: matrices.hh:167: Assertion `!(i<=0 || l> n_)' failed.\n";
            return CCJ_E_BACKTRACK;
        case BT_STEPS:
            return set_err(c, CCJ_E_HIP, "%s traceback did not end within %d steps", c->host_tb ? "host" : "device", BT_MAX_STEPS);
        default:
            return set_err(c, CCJ_E_HIP, "device traceback stack overflow (capacity %d)", bt_stack_cap(c->n));
    }
}

// W_final::fill_structure, W_final.cc:764-819: brackets from the pair list f[1..n] into
// structure[1..n].  False when more than 4 bands cross (the reference pops an empty std::stack).
bool fill_structure(int n, const int *f_pair, std::string &structure) {
    struct Brack { char open, close; };
    struct Band { char open, close; int outer_start, outer_end, inner_start, inner_end; };
    std::stack<Brack> st;
    st.push({'<', '>'});
    st.push({'{', '}'});
    st.push({'[', ']'});
    st.push({'(', ')'});
    std::list<Band> bands;
    bands.push_back({'|', '|', 0, 0, 0, 0});
    structure.assign(n + 1, '.');
    for (int i = 1; i <= n; i++) {
        const int j = f_pair[i];
        if (j == -1) {
            structure[i] = '.';
        } else if (i < j) {
            bool inband = false;
            for (auto it = bands.begin(); it != bands.end(); ++it) {
                if (i > it->inner_start && j < it->inner_end) {
                    it->inner_start = i;
                    it->inner_end = j;
                    structure[i] = it->open;
                    structure[j] = it->close;
                    inband = true;
                    break;
                }
            }
            if (!inband) {
                if (st.empty()) return false;
                Brack e = st.top();
                st.pop();
                bands.push_back({e.open, e.close, i, j, i, j});
                structure[i] = e.open;
                structure[j] = e.close;
            }
        } else {
            for (auto it = bands.begin(); it != bands.end(); ++it) {
                if (i == it->outer_end) {
                    st.push({it->open, it->close});
                    break;
                }
            }
        }
    }
    return true;
}

// bt_exit, then the brackets: what both executors' results go through
int bt_finish(ccj_ctx *c, const BtOut &bo, const int *f_pair, std::string &structure, std::string &out) {
    if (const int rc = bt_exit(c, bo, out)) return rc;
    if (fill_structure(c->n, f_pair, structure)) return CCJ_OK;
    c->err = "CCJ: fill_structure: more than 4 crossing bands (reference pops an empty std::stack)\n";
    return CCJ_E_BACKTRACK;
}

uint64_t fnv(uint64_t h, const void *p, size_t nb) {
    const unsigned char *c = (const unsigned char *)p;
    for (size_t x = 0; x < nb; ++x) { h ^= c[x]; h *= 1099511628211ull; }
    return h;
}

}  // namespace

// ============================================================================================
// C ABI
// ============================================================================================
extern "C" uint64_t ccj_num_cells(int n) {
    if (n < 3) return 0;
    const uint64_t m = (uint64_t)n + 1;
    return m * (m - 1) * (m - 2) * (m - 3) / 24;
}

static thread_local std::string g_create_err;


// One part of a level's exchange through the in-process group: every member pulls each member's
// packed slice of the part into its own receive buffer (same device) on stream q, between two
// barriers, so no slice is overwritten by the part's next pack before every member has read it.
static int local_allgather(ccj_ctx *c, int part, size_t slice, hipStream_t q) {
    ccj_group *g = c->xch.lgroup;
    HIPCHK(c, hipStreamSynchronize(q));  // own slice packed
    if (!g->barrier()) return set_err(c, CCJ_E_STATE, "local exchange: a group member failed");
    // take the peers' send buffers under the lock and hold the group busy until the copies are
    // done: ccj_destroy of a peer waits for busy == 0 before it frees anything
    std::vector<const int16_t *> src(g->world, nullptr);
    {
        std::lock_guard<std::mutex> lk(g->mu);
        for (int r = 0; r < g->world; ++r) {
            if (!g->members[r]) {
                g->broken = true;  // every other member's next barrier fails instead of waiting
                g->cv.notify_all();
                return set_err(c, CCJ_E_STATE, "local exchange: rank %d has no context", r);
            }
            src[r] = g->members[r]->xch.d_send[part];
        }
        ++g->busy;
    }
    hipError_t e = hipSuccess;
    for (int r = 0; r < g->world && e == hipSuccess; ++r)
        e = hipMemcpyAsync(c->xch.d_recv[part] + (size_t)r * slice, src[r], slice * sizeof(int16_t), hipMemcpyDeviceToDevice, q);
    const hipError_t e2 = hipStreamSynchronize(q);
    {
        std::lock_guard<std::mutex> lk(g->mu);
        --g->busy;
        g->cv.notify_all();
    }
    HIPCHK(c, e);
    HIPCHK(c, e2);
    if (!g->barrier()) return set_err(c, CCJ_E_STATE, "local exchange: a group member failed");
    return CCJ_OK;
}

// The bulk part of a level's exchange through the in-process group, without blocking the host: after
// one barrier (every member has recorded its ev_bpacked for this level), each member's bulk slice is
// copied on this member's side stream behind that member's ev_bpacked, and ev_bcopied marks the copies
// (a member's next bulk pack waits for every member's ev_bcopied, bulk_start).  The level chain keeps
// running meanwhile; only the edge part (local_allgather) synchronises the host with the level.
static int local_bulk_gather(ccj_ctx *c, size_t slice) {
    ccj_group *g = c->xch.lgroup;
    if (!g->barrier()) return set_err(c, CCJ_E_STATE, "local exchange: a group member failed");
    std::lock_guard<std::mutex> lk(g->mu);
    for (int r = 0; r < g->world; ++r) {
        const ccj_ctx *p = g->members[r];
        if (!p) {
            g->broken = true;
            g->cv.notify_all();
            return set_err(c, CCJ_E_STATE, "local exchange: rank %d has no context", r);
        }
        HIPCHK(c, hipStreamWaitEvent(c->xch.st_x, p->xch.ev_bpacked, 0));
        HIPCHK(c, hipMemcpyAsync(c->xch.d_recv[XCH_BULK] + (size_t)r * slice, p->xch.d_send[XCH_BULK], slice * sizeof(int16_t),
                                 hipMemcpyDeviceToDevice, c->xch.st_x));
    }
    HIPCHK(c, hipEventRecord(c->xch.ev_bcopied, c->xch.st_x));
    return CCJ_OK;
}
// before this member's next bulk pack overwrites its send slice: every member's copies of it are done
static int local_bulk_wait_copied(ccj_ctx *c) {
    ccj_group *g = c->xch.lgroup;
    std::lock_guard<std::mutex> lk(g->mu);
    for (int r = 0; r < g->world; ++r)
        if (const ccj_ctx *p = g->members[r]) HIPCHK(c, hipStreamWaitEvent(c->xch.st_x, p->xch.ev_bcopied, 0));
    return CCJ_OK;
}

// element counts of the n-dependent buffers (layout_extents below; ccj_layout_extents)
enum LayoutExtent {
    LX_D4, LX_REC, LX_RK, LX_RL, LX_ACC, LX_D4X, LX_PMX, LX_LORD, LX_LORD_OFF, LX_PLANE, LX_IL, LX_ILSEG,
    LX_LEVELS, LX_LXTAB, LX_EVENTS, LX_ICOUNT, LX_PPUSH_SPAN, LX_ILOOP_SPAN, LX_N
};
static const char *const LX_NAMES =
    "d4 rec rk rl acc d4x pmx lord lord_off plane il ilseg levels lx events icount ppush_span iloop_span";
constexpr long long X_EDGE = 256;  // sentinel elements on either side of the interior-loop copies

// Everything that depends on the sequence itself (not only on n): the encoding, the pair-type,
// hairpin and e_stP tables, and the k_iloop work items.  ccj_create runs it once, ccj_reset and
// ccj_rebind for each new sequence (the allocations are reused; a rebind to another length lays
// the buffers out anew first, bind_layout).
static int seq_setup(ccj_ctx *c) {
    ccj_ctx *cp = c;
    const int n = c->n;
    const bool trace = getenv("CCJ_TRACE_SETUP") != nullptr;
    auto tp0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "seq_setup %-10s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - tp0).count());
        tp0 = now;
    };
    const size_t plane = (size_t)(n + 1) * c->rs;
    // pair_mat.h:159-183 encode_sequence
    c->S.assign(n + 2, 0);
    c->S1.assign(n + 2, 0);
    for (int i = 1; i <= n; ++i) c->S[i] = c->S1[i] = (short)encode_base(c->seq[i - 1]);
    c->S[n + 1] = c->S[1];
    c->S[0] = (short)n;
    c->S1[n + 1] = c->S1[1];
    c->S1[0] = c->S1[n];
    // ---- host-side sequence tables: pair types, hairpins, e_stP
    std::vector<int8_t> pt(plane, 0);
    std::vector<int> hp(plane, INF);
    std::vector<int16_t> est(plane, (int16_t)INTERN_INF);
    c->hpt_h.assign(plane, 0);
    c->fcount = 0;
    for (int w = 0; w < n; ++w)
        for (int p = 1; p + w <= n; ++p) {
            const size_t x = (size_t)w * c->rs + p;
            int tc = c->pair[c->S[p]][c->S[p + w]];
            if (!c->fmask.empty() && c->fmask[(size_t)p * (n + 1) + p + w]) {  // (p, p+w) in F
                c->fcount += tc > 0;
                tc = 0;
            }
            pt[x] = (int8_t)tc;
            c->hpt_h[x] = tc;
        }
    // the device traceback consults pt only where the constraint changed the relation at all
    c->T.cons = c->fcount > 0 ? 1 : 0;
    // the energy tables, built on the host while the GPU counts the work items (below)
    const char *tab_err = nullptr;
    auto energy_tables = [&]() {
        for (int w = 0; w < n; ++w)
            for (int p = 1; p + w <= n; ++p) {
                const int q = p + w;
                const size_t x = (size_t)w * c->rs + p;
                const int tc = pt[x];
                // HairpinE, s_energy_matrix.cc:275-282
                hp[x] = (tc == 0) ? INF
                                  : E_Hairpin_host(&c->prm, c->lx.data(), w - 1, tc, c->S1[p + 1], c->S1[q - 1],
                                                   c->seq.c_str() + p - 1);
                // get_e_stP, pseudo_loop.cc:828-834 (saturated, see k_precompute_ie)
                if (q - p >= 2 && p + 1 != q - 1) {
                    const int t2 = pt[(size_t)(w - 2) * c->rs + p + 1];
                    const int e = E_IntLoop(&c->prm, c->lx.data(), 0, 0, tc, c->rtype[t2], c->S1[p + 1], c->S1[q - 1],
                                            c->S1[p], c->S1[q]);
                    const long v = lrint(c->e_stP * e);
                    if (v < -32768) { tab_err = "e_stP below int16 range"; return; }
                    if (tc > 0 && t2 > 0 && v >= INTERN_INF) { tab_err = "e_stP of a canonical stack >= 32767"; return; }
                    est[x] = (int16_t)(v >= INTERN_INF ? INTERN_INF : v);
                }
            }
    };
    lap("pair types");
    // the sequence tables go up asynchronously on st from pinned staging (a reset never blocks on
    // work another context has running on the GPU); the fill's launches follow on st
    if (!c->h_stage) {  // sized for the capacity, like every allocation (create_impl)
        const size_t stage_bytes = (size_t)c->cap_ext[LX_PLANE] * (1 + sizeof(int) + sizeof(int16_t)) +
                                   2 * (size_t)(c->ncap + 2) * sizeof(short);
        HIPCHK(cp, hipHostMalloc(&c->h_stage, stage_bytes, hipHostMallocDefault));
        HIPCHK(cp, hipEventCreateWithFlags(&c->ev_stage, hipEventDisableTiming));
    } else {
        HIPCHK(cp, hipEventSynchronize(c->ev_stage));  // the previous uploads have read the staging
    }
    char *stg = (char *)c->h_stage;
    auto up = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        memcpy(stg, src, bytes);
        const hipError_t e = hipMemcpyAsync(dst, stg, bytes, hipMemcpyHostToDevice, c->st);
        stg += bytes;
        return e;
    };
    HIPCHK(cp, up(c->d_pt, pt.data(), plane));
    // ---- k_iloop work items (one per wave), counted per (level, shard), then written by k_items
    // on the GPU at the prefix offsets.  By default the count pass runs on the GPU too (k_items
    // pass 0 on st) and the host WAITS for it (hipStreamSynchronize): the offsets are needed on
    // the host to size the k_iloop launches, so ccj_reset blocks until the context's stream has
    // run it.  CCJ_HOST_COUNT=1 counts on host threads instead (the same enumeration, ccj_items.h;
    // slower, ~1.3 ms at n=200, but no device round trip).
    if (n > 1023) return set_err(cp, CCJ_E_ARG, "sequence longer than 1023 (k_iloop item encoding)");
    {
        const int G = c->world;
        const int nb = n * G;
        const int rs = c->rs;
        struct HostPT {
            const int8_t *pt;
            int rs;
            int operator()(int i, int j) const { return pt[(size_t)(j - i) * rs + i]; }
        } hpt{pt.data(), rs};
        std::vector<long long> cnt((size_t)nb, 0), cnt2((size_t)nb * KI_SPLIT, 0);  // per (t, r) / per split
        // default: counted on the GPU by k_items (KI_SPLIT workgroups per level, then one round
        // trip); CCJ_HOST_COUNT=1: on host threads (slower, but no device round trip, so a reset
        // never waits behind another context's fill on a shared hardware queue)
        static const bool host_count = getenv("CCJ_HOST_COUNT") && atoi(getenv("CCJ_HOST_COUNT")) != 0;
        if (!host_count) {
            HIPCHK(cp, (hipError_t)ccjk_items(&c->T, G, c->rank, c->simulate, c->d_icount, nullptr, nullptr, 0, c->st));
            if (!c->h_icount) HIPCHK(cp, hipHostMalloc(&c->h_icount, (size_t)c->cap_ext[LX_ICOUNT] * sizeof(long long), hipHostMallocDefault));
            HIPCHK(cp, hipMemcpyAsync(c->h_icount, c->d_icount, cnt2.size() * sizeof(long long), hipMemcpyDeviceToHost, c->st));
            energy_tables();
            lap("tables");
            HIPCHK(cp, hipStreamSynchronize(c->st));
            memcpy(cnt2.data(), c->h_icount, cnt2.size() * sizeof(long long));
        } else {
            energy_tables();
            lap("tables");
        }
        if (tab_err) return set_err(cp, CCJ_E_PARAMS, "%s", tab_err);
        std::atomic<int> next{0};
        static const bool check = getenv("CCJ_CHECK_ITEMS") && atoi(getenv("CCJ_CHECK_ITEMS")) != 0;
        std::atomic<bool> bad{false};
        auto worker = [&]() {
            for (int b; (b = next.fetch_add(1)) < nb;) {
                const int t = b / G, r = b % G;
                if (!(c->simulate || r == c->rank) || t < 4 || t >= c->nlev) continue;
                const long long hc = count_level_items(pt.data(), rs, n, t, G, r, IL_CW);
                long long gpu = 0;
                for (int s = 0; s < KI_SPLIT; ++s) gpu += cnt2[(size_t)b * KI_SPLIT + s];
                if (!host_count && hc != gpu) bad = true;  // check mode: host and GPU counts agree
                if (host_count || check) {  // the generic enumeration per split (host mode sizes the splits with it)
                    const ItemRows R = item_rows(n, t, G, r);
                    long long sum = 0;
                    uint32_t it0;
                    for (int s = 0; s < KI_SPLIT; ++s) {
                        int lo, hi;
                        ki_split_rows(R.nPL + R.nPR + R.nPM, s, lo, hi);
                        long long cs = 0;
                        for (int x = lo; x < hi; ++x) cs += item_row(hpt, n, t, R, x, G, r, it0, IL_CW);
                        if (host_count) cnt2[(size_t)b * KI_SPLIT + s] = cs;
                        else if (cs != cnt2[(size_t)b * KI_SPLIT + s]) bad = true;
                        sum += cs;
                    }
                    if (sum != hc) bad = true;
                }
            }
        };
        if (host_count || check) {
            const int nth = std::max(1, std::min<int>(8, (int)std::thread::hardware_concurrency()));
            std::vector<std::thread> pool;
            for (int x = 1; x < nth; ++x) pool.emplace_back(worker);
            worker();
            for (auto &th : pool) th.join();
        }
        if (bad) return set_err(cp, CCJ_E_STATE, "k_iloop item count pass disagrees with the enumeration");
        for (int b = 0; b < nb; ++b)
            for (int s = 0; s < KI_SPLIT; ++s) cnt[b] += cnt2[(size_t)b * KI_SPLIT + s];
        c->it_off.assign((size_t)nb + 1, 0);
        for (int x = 0; x < nb; ++x) c->it_off[x + 1] = c->it_off[x] + cnt[x];
        const size_t total = (size_t)c->it_off[nb];
        lap("count");
        if (total > c->items_cap || !c->d_items) {  // ccj_reset: grow only
            if (c->d_items) HIPCHK(cp, hipFree(c->d_items));
            c->d_items = nullptr;
            c->items_cap = std::max<size_t>(total, 1);
            HIPCHK(cp, hipMalloc(&c->d_items, c->items_cap * sizeof(uint32_t)));
        }
        c->T.items = c->d_items;
        // the first item of every split, through pinned staging so the upload is asynchronous on st
        // (the fill's first launches follow it)
        const size_t nsp = (size_t)nb * KI_SPLIT;
        if (!c->h_ioff) HIPCHK(cp, hipHostMalloc(&c->h_ioff, (size_t)c->cap_ext[LX_ICOUNT] * sizeof(long long), hipHostMallocDefault));
        for (int b = 0; b < nb; ++b) {
            long long o = c->it_off[b];
            for (int s = 0; s < KI_SPLIT; ++s) {
                c->h_ioff[(size_t)b * KI_SPLIT + s] = o;
                o += cnt2[(size_t)b * KI_SPLIT + s];
            }
        }
        HIPCHK(cp, hipMemcpyAsync(c->d_ioff, c->h_ioff, nsp * sizeof(long long), hipMemcpyHostToDevice, c->st));
        HIPCHK(cp, (hipError_t)ccjk_items(&c->T, G, c->rank, c->simulate, c->d_icount, c->d_ioff, c->d_items, 1, c->st));
    }
    HIPCHK(cp, up(c->d_hp, hp.data(), plane * sizeof(int)));
    HIPCHK(cp, up(c->d_est, est.data(), plane * sizeof(int16_t)));
    HIPCHK(cp, up(c->d_S, c->S.data(), (n + 2) * sizeof(short)));
    HIPCHK(cp, up(c->d_S1, c->S1.data(), (n + 2) * sizeof(short)));
    HIPCHK(cp, hipEventRecord(c->ev_stage, c->st));
    lap("upload");
    c->filled = c->mirrored = c->mirrored2d = false;
    c->range_flags = 0;  // a new binding: the last fold's refusal does not stick
    c->range_refused = false;
    return CCJ_OK;
}

// CCJ_SHARE_EDGES=0 (read where a schedule is resolved: a context's creation, the context-free
// schedule and layout exports) keeps the columns with a short other gap out of split-point sharing
// (ccj_engine.h share_role): the A side of an A/B run.  The host lists and the kernels both follow
// the context's value (DevTables::share_edges).
static int share_edges_env() {
    const char *e = getenv("CCJ_SHARE_EDGES");
    return !(e && atoi(e) == 0);
}

// --------------------------------------------------------------------------------------------
// The layout of one sequence length: every quantity the device buffers' sizes and offsets derive
// from n (with the d4 slot count and the split target).  create_impl sizes every allocation from
// the extents of its capacity (layout_extents, exported as ccj_layout_extents); bind_layout lays a
// length n <= capacity out inside them.
// --------------------------------------------------------------------------------------------
struct Layout {
    int n = 0, nlev = 0, g_lo = 0, g_hi = 0;
    int64_t total4 = 0, ncell = 0;      // elements of d4, cells per matrix
    long long nx = 0, npm = 0, xpad = 0, xspan = 0, ppspan = 0, accC = 0, nlord = 0;
    std::vector<LevelDesc> lv;          // base unset
    std::vector<int64_t> off, offh;     // level offsets in d4 / in the host mirror
    std::vector<LvlX> ldx;
};

static void layout_build(int n, int nm4, int split_target, bool share, int edges, Layout &L) {
    const int nent = std::max(n, 1);
    L = Layout{};
    L.n = n;
    L.lv.assign(nent, LevelDesc{nullptr, 0, 0, 0, 0});
    L.off.assign(nent, 0);
    L.offh.assign(nent, 0);
    L.ldx.assign(nent, LvlX{0, 0});
    int64_t off = 0, cells = 0;
    for (int t = 0; t < n; ++t) {
        const int m = n - t - 2;
        LevelDesc D{nullptr, 0, 0, m > 0 ? m : 0, 0};
        if (m > 0) {
            long long C = 0;
            ccj_level_layout(n, t, 1, &C, &D.M);
            D.C = (int)C;
            L.nlev = t + 1;
        }
        L.off[t] = off;
        L.offh[t] = (int64_t)NMAT4 * cells;
        L.lv[t] = D;
        off += (int64_t)nm4 * D.C;
        cells += D.C;
    }
    L.total4 = off;
    L.ncell = cells;
    // k_ppush addresses the PK rows of PPUSH_S consecutive levels as 32-bit byte offsets from the
    // lowest one's start (one buffer resource per wave): that span must stay below 4 GB
    for (int t = 0; t < L.nlev; ++t) {
        const int tt = std::min(t + PPUSH_S - 1, L.nlev - 1);
        L.ppspan = std::max<long long>(L.ppspan, 2 * (L.off[tt] + (long long)L.lv[tt].C - L.off[t]));
    }
    // interior-loop copies (ccj_engine.h): PLx+PRx mirror the level sizes, PMx is padded per (h, j).
    // In front of every level: xpad sentinel elements of 32767, the null target of k_iloop's
    // waves (a wave addresses its source levels as 32-bit offsets from the pad of the lowest)
    L.xpad = n + 256;
    long long ox = 0, op = 0;
    for (int t = 0; t < L.nlev; ++t) {
        ox += L.xpad;
        op += L.xpad;
        L.ldx[t] = LvlX{ox, op};
        ox += 2LL * L.lv[t].C;
        op += (long long)L.lv[t].m * n * (t + 1);
        const int tlo = std::max(0, t - (2 * MAXLOOP - 2));  // a wave of level t + 3 .. t + 58 reads down to tlo
        L.xspan = std::max({L.xspan, 2 * (ox - (L.ldx[tlo].lbx - L.xpad)), 2 * (op - (L.ldx[tlo].pmb - L.xpad))});
    }
    L.nx = ox;
    L.npm = op;
    // split-point sharing: the level range it covers (every level of it runs unsplit, so each leader
    // and its followers run one cell per lane; sched_share_range, ccj_engine.h), the partial-record
    // ring's slot size and the a-blocks k_level4d_lead runs (whatever the world: each block has one owner)
    sched_share_range(n, split_target, share, L.g_lo, L.g_hi);
    for (int t = L.g_lo; t < L.g_hi; ++t) {
        L.accC = std::max<long long>(L.accC, L.lv[t].C);
        for (int a = 0; a <= t; ++a) L.nlord += sched_lead_block(t, a, L.g_lo, edges, nullptr);
    }
}

static void layout_extents_of(const Layout &L, int G, long long *e) {
    const long long n = L.n, plane = (n + 1) * (n + 2);
    const bool sharing = L.g_hi > L.g_lo;
    e[LX_D4] = L.total4;
    e[LX_REC] = e[LX_RK] = e[LX_RL] = L.ncell;
    e[LX_ACC] = sharing ? (long long)SHARE_SLOTS * SHARE_NACC * L.accC : 0;
    e[LX_D4X] = L.nx + 2 * X_EDGE;
    e[LX_PMX] = L.npm + 2 * X_EDGE;
    e[LX_LORD] = L.nlord;
    e[LX_LORD_OFF] = sharing ? n * G + 1 : 0;
    e[LX_PLANE] = plane;
    e[LX_IL] = plane * IL_CAP;
    e[LX_ILSEG] = plane * IL_SEG;
    e[LX_LEVELS] = std::max<long long>(n, 1);
    e[LX_LXTAB] = 2 * n + 128;
    e[LX_EVENTS] = n + 1;
    e[LX_ICOUNT] = n * G * KI_SPLIT;
    e[LX_PPUSH_SPAN] = L.ppspan;
    e[LX_ILOOP_SPAN] = L.xspan;
}

// what a binding of n uses, or (as_capacity) what a context for every length 1 .. n allocates: the
// entrywise maximum over those lengths (the sharing range, and with it the leader list and the
// ring, moves with n and the split target, so those are not monotone in n)
static std::vector<long long> layout_extents(int n, int G, int nm4, int split_target, bool share, int edges, bool as_capacity) {
    std::vector<long long> e(LX_N, 0), x(LX_N, 0);
    Layout L;
    for (int q = as_capacity ? 1 : n; q <= n; ++q) {
        layout_build(q, nm4, split_target, share, edges, L);
        layout_extents_of(L, G, x.data());
        for (int k = 0; k < LX_N; ++k) e[k] = std::max(e[k], x[k]);
    }
    return e;
}

extern "C" const char *ccj_layout_extent_names(void) { return LX_NAMES; }

extern "C" int ccj_layout_extents(int n, int split_target, int share, int full4, int as_capacity, long long *out, int cap) {
    if (n < 1 || n > 1023 || split_target < 0 || (cap > 0 && !out)) return -CCJ_E_ARG;
    if (cap >= LX_N) {
        const std::vector<long long> e = layout_extents(n, 1, full4 ? NMAT4 : NMAT_D4, split_target, share != 0, share_edges_env(), as_capacity != 0);
        std::copy(e.begin(), e.end(), out);
    }
    return LX_N;
}

static int span_check(ccj_ctx *c, const long long *e, int n) {
    if (e[LX_PPUSH_SPAN] >= (1LL << 32))
        return set_err(c, CCJ_E_ARG, "n=%d: the PK rows of %d levels exceed 4 GB (k_ppush offsets)", n, PPUSH_S);
    if (e[LX_ILOOP_SPAN] >= (1LL << 32) - 4096)
        return set_err(c, CCJ_E_ARG, "n=%d: the interior-loop copies of 56 levels exceed 4 GB (k_iloop offsets)", n);
    return CCJ_OK;
}

// Bind the context to sequence length n <= its capacity: the host's level tables, the DevTables
// fields and, on the context's stream, the device state that depends on n alone (k_bind_layout:
// the level descriptors and the sentinels of the interior-loop copies; the leader lists, which
// need the host's cost sort, through pinned staging).  No allocation, no blocking copy and no wait
// on the stream: like seq_setup, a rebind never waits behind another context's fill.
static int bind_layout(ccj_ctx *c, int n) {
    if (n < 1 || n > c->ncap) return set_err(c, CCJ_E_ARG, "length %d outside the context's capacity 1..%d", n, c->ncap);
    const int G = c->world;
    Layout L;
    layout_build(n, c->nm4, c->split_target, c->share, c->share_edges, L);
    if ((uint64_t)L.ncell != (uint64_t)ccj_num_cells(n)) return set_err(c, CCJ_E_ARG, "layout size mismatch");
    long long e[LX_N];
    layout_extents_of(L, G, e);
    if (const int rc = span_check(c, e, n)) return rc;
    for (int k = 0; k < LX_N; ++k)
        if (e[k] > c->cap_ext[k]) return set_err(c, CCJ_E_ARG, "n=%d: layout extent %d exceeds the capacity's", n, k);
    const bool sharing = L.g_hi > L.g_lo;
    const bool relayout = n != c->n;
    // the a-blocks k_level4d_lead runs on each sharing level (a leader or a full scan on either
    // side; the roles of level4d_body), ordered by scan cost, longest first, so the longest
    // waves do not start last.  A leader step costs about 2.5 plain steps.  One list per
    // (level t, rank r) at t*world + r: the rank's own blocks (ccj_engine.h shard_owner).
    c->lord_off.clear();
    if (sharing) {
        HIPCHK(c, hipEventSynchronize(c->ev_bind));  // the previous upload has read the staging
        int *h_off = (int *)c->h_bind;
        int16_t *h_lord = (int16_t *)(h_off + c->cap_ext[LX_LORD_OFF]);
        c->lord_off.assign((size_t)n * G + 1, 0);
        std::vector<std::pair<double, int>> blk;
        int cnt = 0;
        for (int tr = 0; tr < n * G; ++tr) {
            const int t = tr / G, r = tr % G;
            c->lord_off[tr] = cnt;
            if (t < L.g_lo || t >= L.g_hi) continue;
            blk.clear();
            for (int a = 0; a <= t; ++a) {
                double cost = 0;
                if (shard_owner(a, G) != r || !sched_lead_block(t, a, L.g_lo, c->share_edges, &cost)) continue;
                blk.push_back({cost, a});
            }
            std::stable_sort(blk.begin(), blk.end(), [](const auto &x, const auto &y) { return x.first > y.first; });
            if (cnt + (long long)blk.size() > L.nlord) return set_err(c, CCJ_E_STATE, "leader list longer than its extent");
            for (auto &b : blk) h_lord[cnt++] = (int16_t)b.second;
        }
        c->lord_off[(size_t)n * G] = cnt;
        std::copy(c->lord_off.begin(), c->lord_off.end(), h_off);
        if (cnt > 0) HIPCHK(c, hipMemcpyAsync(c->d_lord, h_lord, (size_t)cnt * sizeof(int16_t), hipMemcpyHostToDevice, c->st));
        HIPCHK(c, hipMemcpyAsync(c->d_lord_off, h_off, c->lord_off.size() * sizeof(int), hipMemcpyHostToDevice, c->st));
        HIPCHK(c, hipEventRecord(c->ev_bind, c->st));
    }
    c->n = n;
    c->rs = n + 2;
    c->nlev = L.nlev;
    c->lv_host.swap(L.lv);
    c->lv_off.swap(L.off);
    c->lv_offh.swap(L.offh);
    c->total4 = L.total4;
    c->ncell = L.ncell;
    c->nrec = L.ncell;
    c->nx = L.nx;
    c->npm = L.npm;
    c->xpad = L.xpad;
    c->xspan = L.xspan;
    for (int t = 0; t < n; ++t) c->lv_host[t].base = c->d4 ? c->d4 + c->lv_off[t] : nullptr;
    const size_t plane = (size_t)(n + 1) * c->rs;
    c->h2i.assign(A2_N * plane, 0);
    c->hvt.assign(plane, 0);

    DevTables &T = c->T;
    T.n = n;
    T.nlev = c->nlev;
    T.rs = c->rs;
    T.V = c->d2i + A2_V * plane;
    T.WM = c->d2i + A2_WM * plane;
    T.WMv = c->d2i + A2_WMV * plane;
    T.WMp = c->d2i + A2_WMP * plane;
    T.P = c->d2i + A2_P * plane;
    T.WBP = c->d2i + A2_WBP * plane;
    T.WPP = c->d2i + A2_WPP * plane;
    T.WB = c->d2i + A2_WB * plane;
    T.WP = c->d2i + A2_WP * plane;
    T.tabN = (long long)plane;
    T.nrec = c->nrec;
    T.nx = c->nx;
    T.npm = c->npm;
    T.xpad = c->xpad;
    T.xspan = c->xspan;
    T.g_lo = L.g_lo;
    T.g_hi = L.g_hi;
    T.share_edges = c->share_edges;
    T.acc = sharing ? c->d_acc : nullptr;
    T.lord = sharing ? c->d_lord : nullptr;
    T.lord_off = sharing ? c->d_lord_off : nullptr;
    T.lord_off_h = c->lord_off.empty() ? nullptr : c->lord_off.data();
    T.accC = L.accC;
    // a changed layout moves every level of the interior-loop copies: 32767 again over the bound
    // extent, never over the capacity's
    const bool fill = relayout;
    HIPCHK(c, (hipError_t)ccjk_bind_layout(&T, (int)c->lv_host.size(), c->nm4, c->d_lv, c->d_lb, c->d_ld, c->d_ldx, c->d4x_alloc,
                                           fill ? e[LX_D4X] : 0, c->pmx_alloc, fill ? e[LX_PMX] : 0, c->st));
    return CCJ_OK;
}

// The fill's own side streams and per-level events of a context (a lockstep batch's members have
// none: the batch's streams and events run their fills).
static int create_fill_sync(ccj_ctx *c, size_t nev) {
    HIPCHK(c, hipStreamCreateWithFlags(&c->st_copy, hipStreamNonBlocking));
    HIPCHK(c, fill_sync_create(c->fs, nev, true));
    if (c->exchanges()) {
        Exchange &x = c->xch;
        HIPCHK(c, hipStreamCreateWithFlags(&x.st_d, hipStreamNonBlocking));
        HIPCHK(c, hipStreamCreateWithFlags(&x.st_x, hipStreamNonBlocking));
        for (auto *v : {&x.pp_done, &x.bulk_done}) {
            v->assign(nev, nullptr);
            for (auto &e : *v) HIPCHK(c, hipEventCreateWithFlags(&e, EV_ORDER));
        }
        HIPCHK(c, hipEventCreateWithFlags(&x.ev_bpacked, EV_ORDER));
        HIPCHK(c, hipEventCreateWithFlags(&x.ev_bcopied, EV_ORDER));
    }
    c->tev.resize(TEV_PER * nev);
    for (auto &e : c->tev) HIPCHK(c, hipEventCreate(&e));
    return CCJ_OK;
}

static int create_impl(const ccj_problem *prob, const ccj_options *opts, int nmax, std::unique_ptr<ccj_ctx> &c, ccj_ctx **out) {
    c->seq = prob->seq;
    const int n = (int)c->seq.size();
    c->dangles = prob->dangles;
    c->noGU = prob->noGU ? 1 : 0;
    c->device = opts ? opts->device : 0;
    c->overlap = opts ? (opts->overlap_d2h != 0) : true;
    c->world = (opts && opts->shard_world > 1) ? opts->shard_world : 1;
    c->rank = (opts && c->world > 1) ? opts->shard_rank : 0;
    c->simulate = (opts && c->world > 1) ? (opts->shard_simulate != 0) : 0;
    c->host_tb = opts ? (opts->host_traceback != 0) : false;
    {
        const char *e = getenv("CCJ_SPLIT_TARGET");
        c->split_target = e ? atoi(e) : 9216;
        if (opts && opts->split_target) c->split_target = opts->split_target < 0 ? 0 : opts->split_target;
        const char *lt = getenv("CCJ_LEVEL_TIMING");
        if (lt) c->level_timing = std::max(0, std::min(2, atoi(lt)));
        const char *g = getenv("CCJ_SHARE_SPLITS");
        c->share = !(g && atoi(g) < 0) && !(opts && opts->share_splits < 0);
        c->share_edges = share_edges_env();
    }
    if (c->rank < 0 || c->rank >= c->world) return CCJ_E_ARG;
    memcpy(&c->prm, prob->params, sizeof(ccj_energy_params));
    if (c->prm.magic != CCJ_PARAMS_MAGIC || c->prm.size_bytes != sizeof(ccj_energy_params))
        return CCJ_E_ARG;
    ccj_pk_penalties pk = CCJ_PK_PENALTIES_DEFAULT;
    if (prob->pen) pk = *prob->pen;
    c->pen = Penalties{pk.PS, pk.PSM, pk.PSP, pk.PB, pk.PUP, pk.PPS, pk.a, pk.b, pk.c, pk.ap, pk.bp, pk.cp};
    c->e_stP = pk.e_stP;
    c->e_intP = pk.e_intP;
    if (n < 1) return CCJ_E_ARG;
    if (nmax < n) return set_err(c.get(), CCJ_E_ARG, "ccj_create_cap: sequence of length %d exceeds the capacity %d", n, nmax);
    for (char ch : c->seq)
        if (!(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'U' || ch == 'T')) return CCJ_E_ARG;
    if (nmax > 1023) return set_err(c.get(), CCJ_E_ARG, "sequence longer than 1023 (k_iloop item encoding)");
    if (c->world > 1 && nmax != n)
        return set_err(c.get(), CCJ_E_ARG, "ccj_create_cap: a band-sharded context holds one length (capacity %d, sequence %d)",
                       nmax, n);
    c->ncap = nmax;

    // pair_mat.h:81-155 make_pair_matrix + 159-183 encode_sequence
    const int base_rtype[8] = {0, 2, 1, 4, 3, 6, 5, 7};
    memcpy(c->rtype, base_rtype, sizeof base_rtype);
    for (int x = 0; x < 8; ++x)
        for (int y = 0; y < 8; ++y) c->pair[x][y] = BP_PAIR[x][y];
    if (c->noGU) c->pair[3][4] = c->pair[4][3] = 0;
    for (int x = 0; x < 8; ++x)
        for (int y = 0; y < 8; ++y) c->rtype[c->pair[x][y]] = c->pair[y][x];

    // d4 has the NMAT_D4 slots per level the fill writes, or all 22 (a full context)
    // where the band-sharded exchange packs them or a host mirror streams them during the fill
    // (ccj_engine.h carrier); CCJ_D4_FULL=1 makes any context full (A/B timing).  The host mirror
    // always has 22
    c->full4 = c->exchanges() || c->overlap || (getenv("CCJ_D4_FULL") && atoi(getenv("CCJ_D4_FULL")) != 0);
    c->nm4 = c->full4 ? NMAT4 : NMAT_D4;
    // every allocation below is sized from the capacity's extents and nothing else
    c->cap_ext = layout_extents(nmax, c->world, c->nm4, c->split_target, c->share, c->share_edges, true);
    const std::vector<long long> &X = c->cap_ext;
    if (const int rc = span_check(c.get(), X.data(), nmax)) return rc;
    // (int)(lxc*log(x/30.)) with the host libm, as ViennaRNA computes it
    c->lx.assign((size_t)X[LX_LXTAB], 0);
    for (size_t x = 31; x < c->lx.size(); ++x) c->lx[x] = (int)(c->prm.lxc * log((double)x / 30.));

    ccj_ctx *cp = c.get();
    HIPCHK(cp, hipSetDevice(c->device));
    HIPCHK(cp, hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    const size_t plane = (size_t)X[LX_PLANE];
    if (!c->member) {
        if (const int rc = create_fill_sync(cp, (size_t)X[LX_EVENTS])) return rc;
    }
    if (X[LX_D4] > 0 && hipMalloc(&c->d4, (size_t)X[LX_D4] * sizeof(int16_t)) != hipSuccess)
        return set_err(cp, CCJ_E_OOM, "device allocation of %.2f GB for 4-D matrices failed", X[LX_D4] * 2e-9);
    // loop records: one RA (8 bytes), RK (8) and RL (4) record per cell, each its own array (ccj_engine.h)
    if (X[LX_REC] > 0 && (hipMalloc(&c->d_rec, (size_t)X[LX_REC] * sizeof(rec_t)) != hipSuccess ||
                          hipMalloc(&c->d_rk, (size_t)X[LX_RK] * sizeof(rk_t)) != hipSuccess ||
                          hipMalloc(&c->d_rl, (size_t)X[LX_RL] * sizeof(rl_t)) != hipSuccess))
        return set_err(cp, CCJ_E_OOM, "device allocation of %.2f GB for loop records failed", X[LX_REC] * (REC_BYTES * 1e-9));
    // split-point sharing (where some length up to the capacity shares): the leader lists with
    // their pinned staging, and the partial-record ring
    if (X[LX_LORD_OFF] > 0) {
        HIPCHK(cp, hipMalloc(&c->d_lord, std::max<size_t>((size_t)X[LX_LORD], 1) * sizeof(int16_t)));
        HIPCHK(cp, hipMalloc(&c->d_lord_off, (size_t)X[LX_LORD_OFF] * sizeof(int)));
        if (hipMalloc(&c->d_acc, (size_t)X[LX_ACC] * sizeof(uint2)) != hipSuccess)
            return set_err(cp, CCJ_E_OOM, "device allocation of %.2f GB for split-sharing records failed", X[LX_ACC] * 8e-9);
        HIPCHK(cp, hipHostMalloc(&c->h_bind, (size_t)X[LX_LORD_OFF] * sizeof(int) + (size_t)X[LX_LORD] * sizeof(int16_t),
                                 hipHostMallocDefault));
        HIPCHK(cp, hipEventCreateWithFlags(&c->ev_bind, hipEventDisableTiming));
    }
    HIPCHK(cp, hipMalloc(&c->d_ie, plane * sizeof(int16_t)));  // the u1 = u2 = 0 plane (k_build_il evaluates the rest)
    HIPCHK(cp, hipMalloc(&c->d_est, plane * sizeof(int16_t)));
    HIPCHK(cp, hipMalloc(&c->d_hp, plane * sizeof(int)));
    HIPCHK(cp, hipMalloc(&c->d_pt, plane));
    HIPCHK(cp, hipMalloc(&c->d_pair, 64));
    HIPCHK(cp, hipMalloc(&c->d_rtype, 8));
    HIPCHK(cp, hipMalloc(&c->d_lx, c->lx.size() * sizeof(int)));
    HIPCHK(cp, hipMalloc(&c->d_err, 2 * sizeof(int)));  // the error word; [1]: the sharded range word (exchange_enqueue)
    HIPCHK(cp, hipMalloc(&c->d_S, (nmax + 2) * sizeof(short)));
    HIPCHK(cp, hipMalloc(&c->d_S1, (nmax + 2) * sizeof(short)));
    HIPCHK(cp, hipMalloc(&c->d_prm, sizeof(ccj_energy_params)));
    const size_t nent = (size_t)X[LX_LEVELS];
    HIPCHK(cp, hipMalloc(&c->d_lv, nent * sizeof(LevelDesc)));
    HIPCHK(cp, hipMalloc(&c->d_lb, nent * sizeof(long long)));
    HIPCHK(cp, hipMalloc(&c->d_ld, nent * sizeof(LvlDev)));
    {
        // interior-loop copies: X_EDGE pad elements on both sides; bind_layout (k_bind_layout) sets the
        // bound extent to 32767 (the pads stay so: no level writes them)
        if (hipMalloc(&c->d4x_alloc, (size_t)X[LX_D4X] * sizeof(int16_t)) != hipSuccess ||
            hipMalloc(&c->pmx_alloc, (size_t)X[LX_PMX] * sizeof(int16_t)) != hipSuccess)
            return set_err(cp, CCJ_E_OOM, "device allocation of %.2f GB for interior-loop copies failed",
                           (X[LX_D4X] + X[LX_PMX]) * 2e-9);
        c->d4x = c->d4x_alloc + X_EDGE;
        c->pmx = c->pmx_alloc + X_EDGE;
        HIPCHK(cp, hipMalloc(&c->d_ldx, nent * sizeof(LvlX)));
        std::vector<int16_t> dummy((size_t)nmax + 64, (int16_t)INTERN_INF);
        HIPCHK(cp, hipMalloc(&c->d_dummy, dummy.size() * sizeof(int16_t)));
        HIPCHK(cp, hipMemcpy(c->d_dummy, dummy.data(), dummy.size() * sizeof(int16_t), hipMemcpyHostToDevice));
        {  // the k_iloop work items' candidate lists (k_build_il)
            HIPCHK(cp, hipMalloc(&c->d_il, (size_t)X[LX_IL] * sizeof(uint2)));
            HIPCHK(cp, hipMalloc(&c->d_ilm, (size_t)X[LX_IL] * sizeof(uint2)));
            HIPCHK(cp, hipMalloc(&c->d_ilseg, (size_t)X[LX_ILSEG] * sizeof(uint32_t)));
            HIPCHK(cp, hipMalloc(&c->d_ilmseg, (size_t)X[LX_ILSEG] * sizeof(uint32_t)));
            HIPCHK(cp, hipMemset(c->d_ilseg, 0, (size_t)X[LX_ILSEG] * sizeof(uint32_t)));
            HIPCHK(cp, hipMemset(c->d_ilmseg, 0, (size_t)X[LX_ILSEG] * sizeof(uint32_t)));
        }
    }
    HIPCHK(cp, hipMalloc(&c->d2i, A2_N * plane * sizeof(int)));
    HIPCHK(cp, hipMalloc(&c->d_wbw, plane * sizeof(int2)));
    HIPCHK(cp, hipMalloc(&c->d_tab, 6 * plane * sizeof(int16_t)));  // k_init2d resets them with every fill
    HIPCHK(cp, hipMalloc(&c->d_cf, NCF * plane * sizeof(int)));     // and these
    HIPCHK(cp, hipMalloc(&c->d_pk, plane * sizeof(unsigned long long)));
    HIPCHK(cp, hipMalloc(&c->d_W, (nmax + 1) * sizeof(int)));
    HIPCHK(cp, hipMalloc(&c->d_wterm, plane * sizeof(int)));
    HIPCHK(cp, hipMalloc(&c->d_fpair, (nmax + 1) * sizeof(int)));
    HIPCHK(cp, hipMalloc(&c->d_ftype, (nmax + 1)));
    HIPCHK(cp, hipMalloc(&c->d_btout, sizeof(BtOut)));
    HIPCHK(cp, hipMalloc(&c->d_vt, plane));
    // the pinned host mirror is only needed by the host traceback and the getters: allocate it up
    // front when the fill streams into it, else on first use (ccj_sync_host); sized for the capacity
    if (c->overlap && X[LX_REC] > 0 &&
        hipHostMalloc(&c->h4, (size_t)NMAT4 * X[LX_REC] * sizeof(int16_t), hipHostMallocDefault) != hipSuccess)
        return set_err(cp, CCJ_E_OOM, "pinned host allocation of %.2f GB failed", NMAT4 * X[LX_REC] * 2e-9);

    int8_t pair8[64], rt8[8];
    for (int x = 0; x < 8; ++x) {
        rt8[x] = (int8_t)c->rtype[x];
        for (int y = 0; y < 8; ++y) pair8[x * 8 + y] = (int8_t)c->pair[x][y];
    }
    HIPCHK(cp, hipMemcpy(c->d_pair, pair8, 64, hipMemcpyHostToDevice));
    HIPCHK(cp, hipMemcpy(c->d_rtype, rt8, 8, hipMemcpyHostToDevice));
    HIPCHK(cp, hipMemcpy(c->d_lx, c->lx.data(), c->lx.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(cp, hipMemcpy(c->d_prm, &c->prm, sizeof(ccj_energy_params), hipMemcpyHostToDevice));

    // what no binding moves; bind_layout sets the rest
    DevTables &T = c->T;
    T.dangles = c->dangles;
    T.pen = c->pen;
    T.e_stP = c->e_stP;
    T.e_intP = c->e_intP;
    T.prm = c->d_prm;
    T.lx = c->d_lx;
    T.S = c->d_S;
    T.S1 = c->d_S1;
    T.pt = c->d_pt;
    T.pair = c->d_pair;
    T.rtype = c->d_rtype;
    T.hp = c->d_hp;
    T.est = c->d_est;
    T.ie = c->d_ie;
    T.Pk = c->d_pk;
    T.WBW = c->d_wbw;
    T.Vt = c->d_vt;
    T.lv = c->d_lv;
    T.d4 = c->d4;
    T.lb = c->d_lb;
    T.ld = c->d_ld;
    T.d4x = c->d4x;
    T.rec = c->d_rec;
    T.rk = c->d_rk;
    T.rl = c->d_rl;
    T.cf = c->d_cf;
    T.tab = c->d_tab;
    T.pmx = c->pmx;
    T.ldx = c->d_ldx;
    T.il = c->d_il;
    T.ilm = c->d_ilm;
    T.dummy = c->d_dummy;
    T.items = c->d_items;
    T.full4 = c->full4 ? 1 : 0;
    T.ilseg = c->d_ilseg;
    T.ilmseg = c->d_ilmseg;
    T.err = c->d_err;
    T.split_target = c->split_target;
    {
        const int G = c->world;
        HIPCHK(cp, hipMalloc(&c->d_icount, (size_t)X[LX_ICOUNT] * sizeof(long long)));
        HIPCHK(cp, hipMalloc(&c->d_ioff, (size_t)X[LX_ICOUNT] * sizeof(long long)));
        if (nmax > n) {
            // a capacity context allocates its k_iloop work items once, for the most any sequence up
            // to the capacity can have: every row of every level (ccj_items.h item_rows, which grow
            // with n) in its most chunks
            size_t bound = 1;
            for (int t = 4; t < nmax - 2; ++t) {
                const ItemRows R = item_rows(nmax, t, 1, 0);
                bound += (size_t)(R.nPL + R.nPR + R.nPM) * (nmax / IL_CW + 1);
            }
            c->items_cap = bound;
            HIPCHK(cp, hipMalloc(&c->d_items, c->items_cap * sizeof(uint32_t)));
        }
        if (c->exchanges()) {
            // exchange slices, per part: 22 matrices x the largest rank's blocks of the
            // part x M, then the part's tail (a band-sharded context holds one length: nmax == n)
            for (int part = 0; part < 2; ++part) {
                c->xch.xnmax[part].assign(n, 0);
                size_t slice = 0;
                for (int t = 0; t + 2 < n; ++t) {
                    const int nm = xch_nmax(t, G, part), m = n - t - 2;
                    c->xch.xnmax[part][t] = nm;
                    slice = std::max(slice, (size_t)xch_slice(n, nm, m * (m + 1) / 2, part));
                }
                if (hipMalloc(&c->xch.d_send[part], std::max<size_t>(slice, 1) * sizeof(int16_t)) != hipSuccess ||
                    hipMalloc(&c->xch.d_recv[part], std::max<size_t>(slice * G, 1) * sizeof(int16_t)) != hipSuccess)
                    return set_err(cp, CCJ_E_OOM, "device allocation of the exchange buffers (%.2f GB) failed",
                                   slice * (G + 1) * 2e-9);
            }
        }
    }
    c->n = 0;  // no binding yet: bind_layout sets the sentinels of its layout
    if (const int rc = bind_layout(cp, n)) return rc;
    if (const int rc = seq_setup(cp)) return rc;
    *out = c.release();
    return CCJ_OK;
}

extern "C" int ccj_create_cap(const ccj_problem *prob, const ccj_options *opts, int nmax, ccj_ctx **out) {
    if (!out) return CCJ_E_ARG;
    *out = nullptr;
    g_create_err.clear();
    if (!prob || !prob->seq || !prob->params) {
        g_create_err = "null problem / sequence / params";
        return CCJ_E_ARG;
    }
    std::unique_ptr<ccj_ctx> c(new ccj_ctx());
    const int rc = create_impl(prob, opts, nmax, c, out);
    if (rc != CCJ_OK) {
        g_create_err = c ? c->err : std::string("ccj_create failed");
        if (g_create_err.empty()) g_create_err = "invalid problem (sequence alphabet, length or parameter blob)";
        if (c) ccj_destroy(c.release());
    }
    return rc;
}

extern "C" int ccj_create(const ccj_problem *prob, const ccj_options *opts, ccj_ctx **out) {
    return ccj_create_cap(prob, opts, prob && prob->seq ? (int)strlen(prob->seq) : 0, out);
}

// The set F of a constraint for a sequence of length n (include/ccj.h) as a symmetric byte mask,
// mask[i*(n+1)+j]; cons == NULL leaves it empty (no constraint).  false: a bad constraint, named in why.
static bool constraint_mask(const ccj_constraint *cons, int n, std::vector<uint8_t> &mask, std::string &why) {
    mask.clear();
    if (!cons) return true;
    const size_t N = (size_t)n + 1;
    auto bad_pairs = [&](const int *v, int cnt, const char *name) {
        if (cnt < 0 || (cnt > 0 && !v)) {
            why = std::string(name) + ": bad count or missing list";
            return true;
        }
        for (int k = 0; k < cnt; ++k) {
            const int i = v[2 * k], j = v[2 * k + 1];
            if (i < 1 || j > n || i >= j) {
                why = std::string(name) + " pair " + std::to_string(k) + " (" + std::to_string(i) + ", " + std::to_string(j) +
                      ") is not 1 <= i < j <= " + std::to_string(n);
                return true;
            }
        }
        return false;
    };
    if (bad_pairs(cons->forbid, cons->n_forbid, "forbid") || bad_pairs(cons->allow_only, cons->allow_only ? cons->n_allow : 0, "allow_only"))
        return false;
    if (cons->unpaired) {
        if (strlen(cons->unpaired) != (size_t)n) {
            why = "unpaired string of length " + std::to_string(strlen(cons->unpaired)) + ", sequence of " + std::to_string(n);
            return false;
        }
        for (const char *q = cons->unpaired; *q; ++q)
            if (*q != '.' && *q != 'x') {
                why = "unpaired string has a character other than '.' and 'x'";
                return false;
            }
    }
    mask.assign(N * N, 0);
    auto set = [&](int i, int j, uint8_t v) { mask[i * N + j] = mask[j * N + i] = v; };
    if (cons->allow_only) {
        for (int i = 1; i <= n; ++i)
            for (int j = i + 1; j <= n; ++j) set(i, j, 1);
        for (int k = 0; k < cons->n_allow; ++k) set(cons->allow_only[2 * k], cons->allow_only[2 * k + 1], 0);
    }
    if (cons->unpaired)
        for (int p = 1; p <= n; ++p)
            if (cons->unpaired[p - 1] == 'x')
                for (int q = 1; q <= n; ++q)
                    if (q != p) set(p, q, 1);
    for (int k = 0; k < cons->n_forbid; ++k) set(cons->forbid[2 * k], cons->forbid[2 * k + 1], 1);
    return true;
}

// ccj_reset (same_length) and ccj_rebind: `what` names the call in the messages.  mask: the binding's
// constraint from constraint_mask (checked by the caller), or NULL for none; it is taken over.
static int rebind_impl(ccj_ctx *c, const char *seq, bool same_length, const char *what, bool from_batch = false,
                       std::vector<uint8_t> *mask = nullptr) {
    if (!c || !seq) return CCJ_E_ARG;
    if (c->batch && !from_batch) return set_err(c, CCJ_E_STATE, "%s: the context is a member of a lockstep batch", what);
    const std::string s(seq);
    const int len = (int)s.size();
    if (same_length && len != c->n)
        return set_err(c, CCJ_E_ARG, "%s: length %zu differs from the context's n=%d", what, s.size(), c->n);
    if (len < 1 || len > c->ncap)
        return set_err(c, CCJ_E_ARG, "%s: length %zu outside the context's capacity 1..%d", what, s.size(), c->ncap);
    for (char ch : s)
        if (!(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'U' || ch == 'T'))
            return set_err(c, CCJ_E_ARG, "%s: invalid character in sequence", what);
    if (c->world > 1 && len != c->n)
        return set_err(c, CCJ_E_ARG, "%s: a band-sharded context holds one length (n=%d)", what, c->n);
    if (c->pending || c->res_pending) return set_err(c, CCJ_E_STATE, "%s: a fold is in flight (ccj_wait first)", what);
    HIPCHK(c, hipSetDevice(c->device));
    // no fold is in flight (checked above): ccj_wait / ccj_fill returned only after the fill and
    // the traceback completed, so the streams are idle.  Only the optional host-mirror copies can
    // still run.  (A hipStreamSynchronize here would enqueue a marker that can wait behind another
    // context's fill on a shared hardware queue.)
    if (c->overlap && c->h4) HIPCHK(c, hipStreamSynchronize(c->st_copy));
    if (len != c->n) {
        if (const int rc = bind_layout(c, len)) return rc;
    }
    c->seq = s;
    if (mask) c->fmask.swap(*mask);
    else c->fmask.clear();
    c->W.clear();
    c->res_ready = false;
    return seq_setup(c);
}

static int rebind_constrained(ccj_ctx *c, const char *seq, const ccj_constraint *cons, bool same_length, const char *what) {
    if (!c || !seq) return CCJ_E_ARG;
    std::vector<uint8_t> mask;
    std::string why;
    // the constraint is checked against the new sequence's length before anything moves; a length the
    // context refuses is reported by rebind_impl's own checks
    const size_t len = strlen(seq);
    const bool len_ok = len >= 1 && len <= (size_t)c->ncap && !(same_length && (int)len != c->n) && !(c->world > 1 && (int)len != c->n);
    if (len_ok && !constraint_mask(cons, (int)len, mask, why))
        return set_err(c, CCJ_E_ARG, "%s: bad constraint: %s", what, why.c_str());
    return rebind_impl(c, seq, same_length, what, false, cons ? &mask : nullptr);
}

extern "C" int ccj_reset(ccj_ctx *c, const char *seq) { return rebind_impl(c, seq, true, "ccj_reset"); }
extern "C" int ccj_rebind(ccj_ctx *c, const char *seq) { return rebind_impl(c, seq, false, "ccj_rebind"); }
extern "C" int ccj_reset_constrained(ccj_ctx *c, const char *seq, const ccj_constraint *cons) {
    return rebind_constrained(c, seq, cons, true, "ccj_reset_constrained");
}
extern "C" int ccj_rebind_constrained(ccj_ctx *c, const char *seq, const ccj_constraint *cons) {
    return rebind_constrained(c, seq, cons, false, "ccj_rebind_constrained");
}
extern "C" long long ccj_constraint_count(const ccj_ctx *c) { return c ? c->fcount : 0; }
extern "C" int ccj_capacity(const ccj_ctx *c) { return c ? c->ncap : 0; }


// The joined level graph of a fill, written once: every wait and record of the
// four-stream wavefront over `steps` spans of which the first `nlev` are 4-D levels.
//   st_il: k_iloop(t)   needs 4-D levels <= t-3 (lev_done[t-3]; the dt = 2 term is in k_level4d);
//          k_diag2d(t-1) follows it on the same stream, behind P(t-1) (p_done), so that level t
//          waits on one event that covers both (fill -0.25 ms at n=200 in 3/3 alternating runs)
//   st   : k_level4d(t) needs level t-1 (stream order), k_iloop(t), k_diag2d(t-1)
//   st_p : k_ppush(t)   needs level t (lev_done[t]); it completes P(t+3)
// so k_diag2d(t) and k_iloop(t+1) overlap k_level4d(t).  Every event is recorded (enqueued) before
// a stream waits on it.  What is launched is the launcher's affair (CtxLaunch, BatchLaunch):
// L.pre(q), L.iloop(s, q), L.diag(sg, q), L.level(s, q), L.ppush(s, q) and L.behind_span(sg, q),
// which follows span sg on its stream, in front of dg_done[sg].  It serves the unsharded fill, the
// shard_simulate fill and the lockstep batch; the fill with an exchange has other edges
// (exchange_enqueue).  The caller joins: the fill ends behind dg_done[steps-1].
template <class Launch>
static hipError_t enqueue_level_dag(const FillSync &f, hipStream_t st, int steps, int nlev, const Launch &L) {
    HIPTRY(L.pre(st));
    HIPTRY(hipEventRecord(f.ev_pre, st));
    HIPTRY(hipStreamWaitEvent(f.st_il, f.ev_pre, 0));
    HIPTRY(hipStreamWaitEvent(f.st_p, f.ev_pre, 0));
    auto diag = [&](int sg) -> hipError_t {
        if (sg >= 3) HIPTRY(hipStreamWaitEvent(f.st_il, f.p_done[sg], 0));
        HIPTRY(L.diag(sg, f.st_il));
        HIPTRY(L.behind_span(sg, f.st_il));
        return hipEventRecord(f.dg_done[sg], f.st_il);
    };
    for (int s = 0; s < steps; ++s) {
        if (s >= nlev) {  // the spans past the last level; the first of them still owes span nlev-1
            if (s == nlev && s >= 1) HIPTRY(diag(s - 1));
            HIPTRY(diag(s));
            continue;
        }
        if (s >= 3) HIPTRY(hipStreamWaitEvent(f.st_il, f.lev_done[s - 3], 0));
        HIPTRY(L.iloop(s, f.st_il));
        if (s >= 1) HIPTRY(diag(s - 1));
        HIPTRY(hipEventRecord(f.il_done[s], f.st_il));
        HIPTRY(hipStreamWaitEvent(st, f.il_done[s], 0));
        HIPTRY(L.level(s, st));
        HIPTRY(hipEventRecord(f.lev_done[s], st));
        if (s + 3 < steps) {  // P(s+3) only needs PK levels <= s
            HIPTRY(hipStreamWaitEvent(f.st_p, f.lev_done[s], 0));
            HIPTRY(L.ppush(s, f.st_p));
            HIPTRY(hipEventRecord(f.p_done[s + 3], f.st_p));
        }
    }
    return hipSuccess;
}

// A context's launches: ccjk_* for each rank the context launches for, and in timing mode 2 the
// markers tev[0..5, 7, 8] around them (TEV_PER).  Both of a context's graphs launch through it.
struct CtxLaunch {
    const ccj_ctx *c;
    hipError_t mark(int s, int x, hipStream_t q) const {
        return c->level_timing == 2 ? hipEventRecord(c->tev[TEV_PER * (size_t)s + x], q) : hipSuccess;
    }
    // every rank's launch in simulation, else this rank's (the only one when unsharded)
    template <class F>
    hipError_t ranks(F launch) const {
        for (int r = 0; r < c->world; ++r)
            if (c->simulate || r == c->rank) HIPTRY(launch(r));
        return hipSuccess;
    }
    hipError_t pre(hipStream_t q) const {
        HIPTRY(ccjk_init2d(&c->T, q));
        HIPTRY(ccjk_precompute_ie(&c->T, q));
        return (hipError_t)ccjk_build_il(&c->T, q);
    }
    hipError_t iloop(int s, hipStream_t q) const {
        HIPTRY(mark(s, 2, q));
        HIPTRY(ranks([&](int r) {
            const size_t tr = (size_t)s * c->world + r;
            return ccjk_iloop(&c->T, s, c->it_off[tr], (int)(c->it_off[tr + 1] - c->it_off[tr]), c->world, r, q);
        }));
        return mark(s, 3, q);
    }
    // span sg, its intervals partitioned over G ranks (G = 1: every interval)
    hipError_t diag(int sg, int G, hipStream_t q) const {
        HIPTRY(mark(sg, 0, q));
        if (G == 1) HIPTRY(ccjk_diag2d(&c->T, sg, 1, 0, q));
        else HIPTRY(ranks([&](int r) { return ccjk_diag2d(&c->T, sg, G, r, q); }));
        return mark(sg, 1, q);
    }
    hipError_t diag(int sg, hipStream_t q) const { return diag(sg, c->world, q); }
    // behind span n-3, the longest a valid cell's (i,j) or (k,l) can have: the range check of the six
    // closed-form matrices (site CF; every rank holds the whole tables).  The two spans
    // that follow on this stream are ordered behind it, so the fill's end (dg_done[n-1]) covers it,
    // and it runs beside the last level.
    hipError_t behind_span(int sg, hipStream_t q) const { return sg == c->n - 3 ? (hipError_t)ccjk_cf_low(&c->T, q) : hipSuccess; }
    // the level: its plain launch, then (sharing levels) the leaders on the same stream, no
    // cross-stream hop between the two launches or between levels
    hipError_t level(int s, hipStream_t q) const {
        HIPTRY(mark(s, 4, q));
        HIPTRY(level_launches(s, q));
        return mark(s, 5, q);
    }
    hipError_t level_launches(int s, hipStream_t q) const {
        HIPTRY(ranks([&](int r) { return ccjk_level4d(&c->T, s, c->world, r, 1, q); }));
        return ranks([&](int r) { return ccjk_level4d_lead(&c->T, s, c->world, r, q); });
    }
    // The P terms that complete P(s+3): every term whose operands' highest level is s (k_ppush,
    // DESIGN.md §4).  Band-sharded, each rank pushes its share (outer index r, r+G, ...; every share
    // in simulation) and the spans are min-combined in the exchange of level s+1.
    hipError_t ppush(int s, hipStream_t q) const {
        HIPTRY(mark(s, 7, q));
        HIPTRY(ranks([&](int r) { return ccjk_ppush(&c->T, s, c->world, r, q); }));
        return mark(s, 8, q);
    }
};

// A full context's d4 has the host mirror's layout except that the fill leaves the IN_TAB and IN_CF
// slots (the last twelve) of every level unwritten: write level t's from the tables, in front of a
// copy to the mirror.
static int expand_tab_slots(const ccj_ctx *c, int t, hipStream_t s) {
    constexpr int first = NMAT_D4 + NMAT_REC;
    return ccjk_expand(&c->T, t, first, c->d4 + c->lv_off[t] + (size_t)first * c->lv_host[t].C, s);
}

// The level graph of the band-sharded fill with an exchange (in-process group or
// RCCL).  Its edges differ from the joined graph's: each span is partitioned by rank and runs on
// st_d, the level-s edge exchange on the level stream carries span s and the partials of P(s+1), and
// the bulk exchange runs one level behind on st_x.
//   st_d : k_diag2d(s)  needs P(s) (p_done) and span s-1 from the other ranks (lev_done[s-1])
//   st_il: k_iloop(t)   needs levels <= t-3 complete on this rank (bulk_done[t-3])
//   st   : k_level4d(t) needs level t-1 (stream order), k_iloop(t), k_diag2d(t-1), and the other
//                       ranks' blocks of level t-2 (bulk_done[t-2]); then the edge exchange
//   st_p : k_ppush(t)   needs level t complete (bulk_done[t]); records pp_done[t+3], and the edge
//                       exchange that combines the ranks' partials records p_done
//   st_x : the bulk exchange of level t, behind lev_done[t]; records bulk_done[t]
// Timing mode 2 adds the markers 6 (the edge exchange's start) and 9, 10 (the bulk exchange).
static int exchange_enqueue(ccj_ctx *c) {
    const int n = c->n, G = c->world, nlev = c->nlev;
    const FillSync &f = c->fs;
    Exchange &x = c->xch;
    const CtxLaunch L{c};
    hipStream_t st = c->st;
    HIPCHK(c, L.pre(st));
    HIPCHK(c, hipEventRecord(f.ev_pre, st));
    HIPCHK(c, hipStreamWaitEvent(x.st_d, f.ev_pre, 0));
    HIPCHK(c, hipStreamWaitEvent(f.st_il, f.ev_pre, 0));
    HIPCHK(c, hipStreamWaitEvent(f.st_p, f.ev_pre, 0));
    // Exchange of level s, part `part` (ccj_engine.h XCH_EDGE / XCH_BULK): pack the rank's blocks of the
    // part (+ the part's tail), gather, unpack.  The edge part runs on the level stream; the bulk part on
    // st_x, split into its start (wait, pack; over RCCL also gather and unpack) and, for the in-process
    // group, its finish one level later (the host-side gather), so that the host thread does not block
    // on it before the next level is enqueued.
    auto part_slice = [&](int s, int part) { return (size_t)xch_slice(n, x.xnmax[part][s], c->lv_host[s].M, part); };
    auto gather = [&](int part, size_t slice, hipStream_t q, const char *what, int s) -> int {
        if (x.lgroup) return local_allgather(c, part, slice, q);
        ncclComm_t cm = part == XCH_EDGE ? x.comm : x.comm_b;
        if (!cm) return set_err(c, CCJ_E_STATE, "sharded context without ccj_comm_init");
        if (ncclAllGather(x.d_send[part], x.d_recv[part], slice * sizeof(int16_t), ncclInt8, cm, q) != ncclSuccess)
            return set_err(c, CCJ_E_COMM, "ncclAllGather (%s) failed at level %d", what, s);
        return CCJ_OK;
    };
    auto bulk_unpack = [&](int s) -> int {
        HIPCHK(c, (hipError_t)ccjk_unpack(&c->T, s, G, c->rank, XCH_BULK, x.xnmax[XCH_BULK][s], x.d_recv[XCH_BULK],
                                          part_slice(s, XCH_BULK), x.st_x));
        HIPCHK(c, L.mark(s, 10, x.st_x));
        HIPCHK(c, hipEventRecord(x.bulk_done[s], x.st_x));
        return CCJ_OK;
    };
    auto bulk_start = [&](int s) -> int {
        HIPCHK(c, hipStreamWaitEvent(x.st_x, f.lev_done[s], 0));
        if (x.lgroup) {
            if (const int rc = local_bulk_wait_copied(c)) return rc;
        }
        HIPCHK(c, L.mark(s, 9, x.st_x));
        HIPCHK(c, (hipError_t)ccjk_pack(&c->T, s, G, c->rank, XCH_BULK, x.xnmax[XCH_BULK][s], x.d_send[XCH_BULK], x.st_x));
        if (x.lgroup) {  // gathered and unpacked when the next level is enqueued (bulk_finish)
            HIPCHK(c, hipEventRecord(x.ev_bpacked, x.st_x));
            return CCJ_OK;
        }
        if (const int rc = gather(XCH_BULK, part_slice(s, XCH_BULK), x.st_x, "bulk", s)) return rc;
        return bulk_unpack(s);
    };
    // the in-process group's bulk gather of level s, then what waits for level s to be complete on
    // this rank: its share of the P terms of P(s+3), combined in the edge exchange of level s+2
    auto bulk_finish = [&](int s) -> int {
        if (x.lgroup) {
            if (const int rc = local_bulk_gather(c, part_slice(s, XCH_BULK))) return rc;
            if (const int rc = bulk_unpack(s)) return rc;
        }
        if (s + 3 < n) {
            HIPCHK(c, hipStreamWaitEvent(f.st_p, x.bulk_done[s], 0));
            HIPCHK(c, L.ppush(s, f.st_p));
            HIPCHK(c, hipEventRecord(x.pp_done[s + 3], f.st_p));
        }
        return CCJ_OK;
    };
    for (int s = 0; s < n; ++s) {
        // span s: this rank's intervals (the exchange of level s brings the rest); past the last
        // level no exchange is left, so every rank computes every interval
        if (s >= 3) HIPCHK(c, hipStreamWaitEvent(x.st_d, f.p_done[s], 0));
        // span s-1 is complete on this rank only after the level-(s-1) edge exchange, which carries it
        if (s >= 1 && s - 1 < nlev) HIPCHK(c, hipStreamWaitEvent(x.st_d, f.lev_done[s - 1], 0));
        HIPCHK(c, L.diag(s, s < nlev ? G : 1, x.st_d));
        HIPCHK(c, L.behind_span(s, x.st_d));
        HIPCHK(c, hipEventRecord(f.dg_done[s], x.st_d));
        if (s >= nlev) {
            if (s > nlev) continue;
            if (s >= 1) {  // the last level's bulk part
                if (const int rc = bulk_finish(s - 1)) return rc;
            }
            if (n - 1 >= 3) {
                // the partials of P(n-1) (pushed after level n-4): no level n-2 carries them, so they
                // travel alone, as a slice of one P tail in the edge buffers
                const int sig = n - 1;
                const size_t pslice = (size_t)xch_ptail(n);
                HIPCHK(c, hipStreamWaitEvent(st, x.pp_done[sig], 0));
                HIPCHK(c, (hipError_t)ccjk_ptail_pack(&c->T, sig, x.d_send[XCH_EDGE], st));
                if (const int rc = gather(XCH_EDGE, pslice, st, "P tail", s)) return rc;
                HIPCHK(c, (hipError_t)ccjk_ptail_unpack(&c->T, sig, x.d_recv[XCH_EDGE], pslice, 0, G, st));
                HIPCHK(c, hipEventRecord(f.p_done[sig], st));
            }
            continue;
        }
        // k_iloop(s) reads levels <= s-3 (complete: their bulk parts unpacked)
        if (s >= 3) HIPCHK(c, hipStreamWaitEvent(f.st_il, x.bulk_done[s - 3], 0));
        HIPCHK(c, L.iloop(s, f.st_il));
        HIPCHK(c, hipEventRecord(f.il_done[s], f.st_il));
        HIPCHK(c, hipStreamWaitEvent(st, f.il_done[s], 0));
        if (s >= 1) HIPCHK(c, hipStreamWaitEvent(st, f.dg_done[s - 1], 0));
        // level s reads the other ranks' blocks of level s-2 from its bulk part (the edge part of
        // level s-1 arrived on this stream; older levels precede s-2 on st_x)
        if (s >= 2) HIPCHK(c, hipStreamWaitEvent(st, x.bulk_done[s - 2], 0));
        HIPCHK(c, L.mark(s, 4, st));
        HIPCHK(c, L.level_launches(s, st));
        // the previous level's bulk part (in-process: its gather), the P terms it completes
        if (s >= 1) {
            if (const int rc = bulk_finish(s - 1)) return rc;
        }
        HIPCHK(c, L.mark(s, 6, st));  // timing mode 2: the edge exchange's share of the level span
        // edge part: the rank's blocks a % 4 == 3 (all 22 matrices), its partials of P(s+1)
        // (pushed after level s-2, so a level of slack) and its intervals of span s
        const size_t slice = part_slice(s, XCH_EDGE), body = (size_t)xch_body(x.xnmax[XCH_EDGE][s], c->lv_host[s].M);
        const size_t dt_off = body + (size_t)xch_ptail(n);
        const int sig = s + 1;
        const bool ptail = sig >= 3 && sig <= n - 2;
        if (ptail) {
            HIPCHK(c, hipStreamWaitEvent(st, x.pp_done[sig], 0));
            HIPCHK(c, (hipError_t)ccjk_ptail_pack(&c->T, sig, x.d_send[XCH_EDGE] + body, st));
        }
        HIPCHK(c, hipStreamWaitEvent(st, f.dg_done[s], 0));
        HIPCHK(c, (hipError_t)ccjk_dtail_pack(&c->T, s, G, c->rank, x.d_send[XCH_EDGE] + dt_off, st));
        HIPCHK(c, (hipError_t)ccjk_pack(&c->T, s, G, c->rank, XCH_EDGE, x.xnmax[XCH_EDGE][s], x.d_send[XCH_EDGE], st));
        if (const int rc = gather(XCH_EDGE, slice, st, "edge", s)) return rc;
        HIPCHK(c, (hipError_t)ccjk_unpack(&c->T, s, G, c->rank, XCH_EDGE, x.xnmax[XCH_EDGE][s], x.d_recv[XCH_EDGE], slice, st));
        HIPCHK(c, (hipError_t)ccjk_dtail_unpack(&c->T, s, x.d_recv[XCH_EDGE], slice, dt_off, G, c->rank, st));
        if (ptail) {
            HIPCHK(c, (hipError_t)ccjk_ptail_unpack(&c->T, sig, x.d_recv[XCH_EDGE], slice, body, G, st));
            HIPCHK(c, hipEventRecord(f.p_done[sig], st));  // P(sig) final on every rank
        }
        HIPCHK(c, L.mark(s, 5, st));
        HIPCHK(c, hipEventRecord(f.lev_done[s], st));
        if (const int rc = bulk_start(s)) return rc;
    }
    // over RCCL a rank sees the LEVEL / ILOOP / PARTIAL sites of its own blocks only, so after the
    // last level the ranks sum one 4-byte word of per-site counts on the level stream's communicator
    // and every rank ends with the union (the in-process group: fill_finish)
    if (!x.lgroup) {
        if (!x.comm) return set_err(c, CCJ_E_STATE, "sharded context without ccj_comm_init");
        unsigned *word = (unsigned *)(c->d_err + 1);
        HIPCHK(c, (hipError_t)ccjk_range_spread(&c->T, word, st));
        if (ncclAllReduce(word, word, 1, ncclUint32, ncclSum, x.comm, st) != ncclSuccess)
            return set_err(c, CCJ_E_COMM, "ncclAllReduce (range sites) failed");
        HIPCHK(c, (hipError_t)ccjk_range_merge(&c->T, word, st));
    }
    // the fill's end also covers every rank's part of the last level
    if (nlev >= 1) HIPCHK(c, hipStreamWaitEvent(st, x.bulk_done[nlev - 1], 0));
    return CCJ_OK;
}

// Enqueue the whole fill on the context's streams; it ends with ev_end on st, after which every
// stream's work of the fill is complete (st waits for the last span, which waits for the last P,
// and every level waited for its k_iloop / leader launches).
static int fill_enqueue(ccj_ctx *c, const ccj_ctx *after = nullptr) {
    if (!c) return CCJ_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int n = c->n;
    const FillSync &f = c->fs;
    hipStream_t st = c->st;
    // pipelining (ccj_fill_async_after): start when the other context's last enqueued fill has
    // ended (its ev_end; its W + traceback may still run beside this fill)
    if (after && after != c && after->fs.ev_end) HIPCHK(c, hipStreamWaitEvent(st, after->fs.ev_end, 0));
    const auto enq0 = std::chrono::steady_clock::now();
    c->filled = c->mirrored = c->mirrored2d = false;
    c->range_flags = 0;
    c->range_refused = false;
    HIPCHK(c, hipMemsetAsync(c->d_err, 0, sizeof(int), st));
    HIPCHK(c, hipEventRecord(f.ev_start, st));
    if (c->exchanges()) {
        if (const int rc = exchange_enqueue(c)) return rc;
    } else {
        HIPCHK(c, enqueue_level_dag(f, st, n, c->nlev, CtxLaunch{c}));
    }
    if (getenv("CCJ_TRACE_ENQUEUE"))
        fprintf(stderr, "ccj_fill_device: enqueue %.2f ms\n",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - enq0).count());
    if (c->overlap && c->h4) {
        // stream each finished level to the pinned host mirror while later levels run.  Its six
        // table-carried slots are written first, from table spans <= s (k_diag2d(s)); enqueued here
        // because every event st_copy waits on must have been recorded.  Level s is complete on this
        // rank at its lev_done or, with an exchange, when its bulk part is unpacked (lev_done[s] then
        // only covers the rank's own cells and the other ranks' edge blocks)
        const std::vector<hipEvent_t> &complete = c->exchanges() ? c->xch.bulk_done : f.lev_done;
        for (int s = 0; s < c->nlev; ++s) {
            HIPCHK(c, hipStreamWaitEvent(c->st_copy, complete[s], 0));
            HIPCHK(c, hipStreamWaitEvent(c->st_copy, f.dg_done[s], 0));
            HIPCHK(c, (hipError_t)expand_tab_slots(c, s, c->st_copy));
            const size_t bytes = (size_t)NMAT4 * c->lv_host[s].C * sizeof(int16_t);
            HIPCHK(c, hipMemcpyAsync(c->h4 + c->lv_offh[s], c->d4 + c->lv_off[s], bytes, hipMemcpyDeviceToHost, c->st_copy));
        }
    }
    // join: the fill ends when the last level and the last span are done
    HIPCHK(c, hipStreamWaitEvent(st, f.dg_done[n - 1], 0));
    HIPCHK(c, hipEventRecord(f.ev_end, st));
    c->pending = true;
    return CCJ_OK;
}

// Wait for the fill's end event.  A band-sharded fill over RCCL cannot finish if a peer rank died
// or hangs (its all-gathers never complete): the wait polls the communicator's asynchronous error
// state and a deadline (CCJ_COMM_TIMEOUT_S, default 300 s) and, on either, aborts the communicator
// (ncclCommAbort makes the pending collectives return) and fails with CCJ_E_COMM instead of hanging.
static int wait_fill_end(ccj_ctx *c) {
    if (!c->xch.comm) {
        HIPCHK(c, hipEventSynchronize(c->fs.ev_end));
        return CCJ_OK;
    }
    static const double limit_s = [] {
        const char *e = getenv("CCJ_COMM_TIMEOUT_S");
        return e && atof(e) > 0 ? atof(e) : 300.0;
    }();
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipEventQuery(c->fs.ev_end);
        if (q == hipSuccess) return CCJ_OK;
        if (q != hipErrorNotReady) return set_err(c, CCJ_E_HIP, "fill: %s", hipGetErrorString(q));
        ncclResult_t ae = ncclSuccess, ae2 = ncclSuccess;
        ncclResult_t qr = ncclCommGetAsyncError(c->xch.comm, &ae);
        if (qr == ncclSuccess && ae == ncclSuccess && c->xch.comm_b) {  // the bulk communicator too
            qr = ncclCommGetAsyncError(c->xch.comm_b, &ae2);
            ae = ae2;
        }
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (qr != ncclSuccess || ae != ncclSuccess || el > limit_s) {
            if (c->xch.comm_b) ncclCommAbort(c->xch.comm_b);
            ncclCommAbort(c->xch.comm);
            c->xch.comm = c->xch.comm_b = nullptr;
            if (qr != ncclSuccess || ae != ncclSuccess)
                return set_err(c, CCJ_E_COMM, "band-sharded exchange failed: %s",
                               ncclGetErrorString(qr != ncclSuccess ? qr : ae));
            return set_err(c, CCJ_E_COMM, "band-sharded exchange made no progress for %.0f s (a peer rank failed?)", limit_s);
        }
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}

// CCJ_ALLOW_OUT_OF_RANGE=1 (read at call time): a fold outside the domain completes under the engine's
// clamp-only semantics instead of being refused
static bool allow_out_of_range() {
    const char *e = getenv("CCJ_ALLOW_OUT_OF_RANGE");
    return e && atoi(e) != 0;
}

// A finished fill's range sites (CCJ_RANGE_* bits): recorded, and unless allowed they refuse the result.
static int range_verdict(ccj_ctx *c, int rflags) {
    c->range_flags = rflags;
    c->range_refused = rflags != 0 && !allow_out_of_range();
    if (!c->range_refused) return CCJ_OK;
    static const char *const site[5] = {"LEVEL", "ILOOP", "PARTIAL", "TAB", "CF"};
    std::string names;
    for (int x = 0; x < 5; ++x)
        if (rflags >> x & 1) names += std::string(names.empty() ? "" : " ") + site[x];
    return set_err(c, CCJ_E_RANGE,
                   "a 4-D value lies below -32768 (sites: %s; flags %d): the reference's int16 store wraps there, so no "
                   "reference-identical result exists for this fold (CCJ_ALLOW_OUT_OF_RANGE=1 folds it clamp-only)",
                   names.c_str(), rflags);
}
static int range_refusal(ccj_ctx *c) { return range_verdict(c, c->range_flags); }

// Wait for an enqueued fill, check the device error word and read its timings.
static int fill_finish(ccj_ctx *c) {
    if (!c || !c->pending) return c ? set_err(c, CCJ_E_STATE, "no fill in flight") : CCJ_E_ARG;
    c->pending = false;
    HIPCHK(c, hipSetDevice(c->device));
    const int n = c->n;
    if (const int rc = wait_fill_end(c)) return rc;
    int herr = 0;
    HIPCHK(c, hipMemcpy(&herr, c->d_err, sizeof(int), hipMemcpyDeviceToHost));
    if (herr & 1) return set_err(c, CCJ_E_PARAMS, "e_intP table value outside int16 range (flags %d)", herr);
    if (herr & ~ERR_RANGE_MASK) return set_err(c, CCJ_E_HIP, "device bounds check failed (flags %d)", herr);
    int rflags = (herr & ERR_RANGE_MASK) >> ERR_RANGE_SHIFT;
    if (c->xch.lgroup) {
        // in-process group: a rank saw the sites of its own blocks; every rank reports the union
        ccj_group *g = c->xch.lgroup;
        const int slot = (int)(c->range_gen++ & 1);
        {
            std::lock_guard<std::mutex> lk(g->mu);
            g->range_acc[slot] |= rflags;
        }
        if (!g->barrier()) return set_err(c, CCJ_E_STATE, "local exchange: a group member failed");
        {
            std::lock_guard<std::mutex> lk(g->mu);
            rflags = g->range_acc[slot];
        }
        if (!g->barrier()) return set_err(c, CCJ_E_STATE, "local exchange: a group member failed");
        {
            std::lock_guard<std::mutex> lk(g->mu);
            g->range_acc[slot] = 0;  // every member, before its next fill's barrier: clean two fills on
        }
    }
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->fs.ev_start, c->fs.ev_end));
    c->fill_ms = ms;
    HIPCHK(c, hipEventElapsedTime(&ms, c->fs.ev_start, c->fs.ev_pre));
    c->pre_ms = ms;
    double lsum = 0, dsum = 0, isum = 0;
    c->lev_ms_v.assign(n, 0.0);
    c->diag_ms_v.assign(n, 0.0);
    c->il_ms_v.assign(n, 0.0);
    c->xch_ms_v.assign(n, 0.0);
    c->xbulk_ms_v.assign(n, 0.0);
    c->pp_ms_v.assign(n, 0.0);
    double psum = 0;
    if (c->level_timing == 1) {
        // level s = from the end of level s-1 (ev_pre for s = 0) to its lev_done on st: the waits for
        // k_iloop(s) / k_diag2d(s-1), the plain launch and the leaders
        for (int s = 0; s < c->nlev && s < n; ++s) {
            HIPCHK(c, hipEventElapsedTime(&ms, s == 0 ? c->fs.ev_pre : c->fs.lev_done[s - 1], c->fs.lev_done[s]));
            lsum += ms;
            c->lev_ms_v[s] = ms;
        }
    }
    for (int s = 0; s < n && c->level_timing == 2; ++s) {
        const hipEvent_t *ev = &c->tev[TEV_PER * (size_t)s];
        HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
        dsum += ms;
        c->diag_ms_v[s] = ms;
        if (s < c->nlev) {
            HIPCHK(c, hipEventElapsedTime(&ms, ev[2], ev[3]));
            isum += ms;
            c->il_ms_v[s] = ms;
            // the level's span: from its first launch to its last (exchange included when sharded)
            HIPCHK(c, hipEventElapsedTime(&ms, ev[4], ev[5]));
            lsum += ms;
            c->lev_ms_v[s] = ms;
            if (s + 3 < n) {  // k_ppush(s) on st_p
                HIPCHK(c, hipEventElapsedTime(&ms, ev[7], ev[8]));
                psum += ms;
                c->pp_ms_v[s] = ms;
            }
            if (c->exchanges()) {
                // the edge part on the level stream: waits for span s, packs, all-gather, unpacks
                HIPCHK(c, hipEventElapsedTime(&ms, ev[6], ev[5]));
                c->xch_ms_v[s] = ms;
                // the bulk part on st_x: from its start (after the level) to its unpack
                HIPCHK(c, hipEventElapsedTime(&ms, ev[9], ev[10]));
                c->xbulk_ms_v[s] = ms;
            }
        }
    }
    c->level_ms = lsum;
    c->diag_ms = dsum;
    c->il_ms = isum;
    c->pp_ms = psum;
    c->filled = true;  // the clamp-only matrices stay readable (getters, ccj_hashes, ccj_sync_host)
    return range_verdict(c, rflags);
}

extern "C" int ccj_fill_device(ccj_ctx *c) {
    if (!c) return CCJ_E_ARG;
    if (c->pending || c->res_pending) return set_err(c, CCJ_E_STATE, "ccj_fill_device: a fold is in flight (ccj_wait first)");
    if (c->batch) return set_err(c, CCJ_E_STATE, "ccj_fill_device: the context is a member of a lockstep batch");
    if (const int rc = fill_enqueue(c)) return rc;
    return fill_finish(c);
}

extern "C" int ccj_sync_host(ccj_ctx *c) {
    if (!c || !c->filled) return CCJ_E_STATE;
    const auto t0 = std::chrono::steady_clock::now();
    struct Rec {
        ccj_ctx *c;
        std::chrono::steady_clock::time_point t0;
        ~Rec() { c->sync_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    } rec{c, t0};
    HIPCHK(c, hipSetDevice(c->device));
    const size_t plane = (size_t)(c->n + 1) * c->rs;
    if (c->overlap && c->h4) {
        HIPCHK(c, hipStreamSynchronize(c->st_copy));
    } else if (c->total4 > 0) {
        const size_t hbytes = (size_t)NMAT4 * c->ncell * sizeof(int16_t);
        const size_t cap_bytes = (size_t)NMAT4 * c->cap_ext[LX_REC] * sizeof(int16_t);  // once, for the capacity
        if (!c->h4 && hipHostMalloc(&c->h4, cap_bytes, hipHostMallocDefault) != hipSuccess)
            return set_err(c, CCJ_E_OOM, "pinned host allocation of %.2f GB failed", cap_bytes * 1e-9);
        if (c->full4) {  // d4 has the mirror's layout
            for (int t = 0; t < c->nlev; ++t) HIPCHK(c, (hipError_t)expand_tab_slots(c, t, c->st));
            HIPCHK(c, hipStreamSynchronize(c->st));
            HIPCHK(c, hipMemcpy(c->h4, c->d4, hbytes, hipMemcpyDeviceToHost));
        } else {  // per level: the NMAT_D4 slots of d4, then the other matrices written out into a scratch
            constexpr int nexp = NMAT4 - NMAT_D4;
            size_t cmax = 0;
            for (int t = 0; t < c->nlev; ++t) cmax = std::max(cmax, (size_t)c->lv_host[t].C);
            int16_t *scr = nullptr;
            if (hipMalloc(&scr, (size_t)nexp * cmax * sizeof(int16_t)) != hipSuccess)
                return set_err(c, CCJ_E_OOM, "ccj_sync_host: device scratch of %.2f GB", nexp * cmax * 2e-9);
            int rc = CCJ_OK;
            for (int t = 0; t < c->nlev && rc == CCJ_OK; ++t) {
                const size_t C = (size_t)c->lv_host[t].C;
                if (ccjk_expand(&c->T, t, NMAT_D4, scr, c->st) != 0 || hipStreamSynchronize(c->st) != hipSuccess ||
                    hipMemcpy(c->h4 + c->lv_offh[t], c->d4 + c->lv_off[t], (size_t)NMAT_D4 * C * sizeof(int16_t),
                              hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(c->h4 + c->lv_offh[t] + (size_t)NMAT_D4 * C, scr, (size_t)nexp * C * sizeof(int16_t),
                              hipMemcpyDeviceToHost) != hipSuccess)
                    rc = set_err(c, CCJ_E_HIP, "ccj_sync_host: mirror copy of level %d failed", t);
            }
            hipFree(scr);
            if (rc != CCJ_OK) return rc;
        }
    }
    HIPCHK(c, hipMemcpy(c->h2i.data(), c->d2i, A2_N * plane * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(c->hvt.data(), c->d_vt, plane, hipMemcpyDeviceToHost));
    c->h_pk.resize(plane);
    HIPCHK(c, hipMemcpy(c->h_pk.data(), c->d_pk, plane * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    c->mirrored = true;
    return CCJ_OK;
}

extern "C" int ccj_fill(ccj_ctx *c) {
    if (c && (c->pending || c->res_pending)) return set_err(c, CCJ_E_STATE, "ccj_fill: a fold is in flight (ccj_wait first)");
    int rc = ccj_fill_device(c);
    if (rc) return rc;
    // the device traceback needs no host mirror; getters make it on demand (ccj_sync_host)
    return c->host_tb ? ccj_sync_host(c) : CCJ_OK;
}

namespace {
int ensure_mirror(const ccj_ctx *cc) {
    ccj_ctx *c = const_cast<ccj_ctx *>(cc);
    return c->mirrored ? CCJ_OK : ccj_sync_host(c);
}

// only the 2-D arrays (no 4-D copy): what ccj_get2 needs
int ensure_mirror_2d(const ccj_ctx *cc) {
    ccj_ctx *c = const_cast<ccj_ctx *>(cc);
    if (c->mirrored || c->mirrored2d) return CCJ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t plane = (size_t)(c->n + 1) * c->rs;
    HIPCHK(c, hipMemcpy(c->h2i.data(), c->d2i, A2_N * plane * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(c->hvt.data(), c->d_vt, plane, hipMemcpyDeviceToHost));
    c->mirrored2d = true;
    return CCJ_OK;
}

// W + traceback on the GPU (ccj_backtrack.hip); brackets on the host
// W + traceback on the GPU (ccj_backtrack.hip), enqueued on st behind the fill; the outputs land in
// pinned host buffers, ev_res marks them complete
int result_enqueue(ccj_ctx *c) {
    const int n = c->n;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->hr_W) {
        HIPCHK(c, hipHostMalloc(&c->hr_W, (c->ncap + 1) * sizeof(int), hipHostMallocDefault));
        HIPCHK(c, hipHostMalloc(&c->hr_fp, (c->ncap + 1) * sizeof(int), hipHostMallocDefault));
        HIPCHK(c, hipHostMalloc(&c->hr_ft, c->ncap + 1, hipHostMallocDefault));
        HIPCHK(c, hipHostMalloc(&c->hr_bo, sizeof(BtOut), hipHostMallocDefault));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_res, hipEventDisableTiming));
    }
    HIPCHK(c, (hipError_t)ccjk_compute_W(&c->T, c->d_W, c->d_wterm, c->st));
    HIPCHK(c, (hipError_t)ccjk_backtrack(&c->T, c->d_W, c->d_fpair, c->d_ftype, c->d_btout, bt_stack_cap(n), c->st));
    HIPCHK(c, hipMemcpyAsync(c->hr_W, c->d_W, (n + 1) * sizeof(int), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(c->hr_fp, c->d_fpair, (n + 1) * sizeof(int), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(c->hr_ft, c->d_ftype, n + 1, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(c->hr_bo, c->d_btout, sizeof(BtOut), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipEventRecord(c->ev_res, c->st));
    c->res_pending = true;
    return CCJ_OK;
}

// wait for result_enqueue's outputs; the reference's exits, then brackets on the host
int result_finish(ccj_ctx *c, std::string &structure, std::string &out, std::chrono::steady_clock::time_point t0) {
    const int n = c->n;
    if (!c->res_pending) return set_err(c, CCJ_E_STATE, "no traceback in flight");
    c->res_pending = false;
    HIPCHK(c, hipEventSynchronize(c->ev_res));
    const BtOut bo = *c->hr_bo;
    c->W.assign(c->hr_W, c->hr_W + n + 1);
    c->w_ms = 0;
    c->bt_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->bt_steps = bo.steps;
    return bt_finish(c, bo, c->hr_fp, structure, out);
}

int device_result(ccj_ctx *c, std::string &structure, std::string &out) {
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = result_enqueue(c)) return rc;
    return result_finish(c, structure, out, t0);
}

// the reference's outputs of W_final::ccj() (W_final.cc:79-104) into the caller's buffers
int emit_result(ccj_ctx *c, int rc, const std::string &st, const std::string &out, char *structure, double *energy_kcal,
                char *msgs, int msgs_cap) {
    if (msgs && msgs_cap > 0) {
        const size_t nb = std::min((size_t)msgs_cap - 1, out.size());
        memcpy(msgs, out.data(), nb);
        msgs[nb] = 0;
    }
    if (rc != CCJ_OK) return rc;
    if (energy_kcal) *energy_kcal = c->W[c->n] / 100.0;
    if (structure) {
        memcpy(structure, st.data() + 1, c->n);
        structure[c->n] = 0;
    }
    return CCJ_OK;
}
}  // namespace

extern "C" int ccj_result(ccj_ctx *c, char *structure, double *energy_kcal, char *msgs, int msgs_cap) {
    if (!c) return CCJ_E_ARG;
    if (!c->filled) return set_err(c, CCJ_E_STATE, "ccj_result before ccj_fill");
    if (c->range_refused) return range_refusal(c);  // no structure, no energy
    std::string st, out;
    int rc = CCJ_OK;
    if (c->res_ready) {  // a batch member: its traceback ran with the batch's (ccj_batch_wait)
        rc = bt_finish(c, *c->hr_bo, c->hr_fp, st, out);
    } else if (!c->host_tb) {
        rc = device_result(c, st, out);
    } else {
        if (int e = ensure_mirror(c)) return e;
        const auto t0 = std::chrono::steady_clock::now();
        compute_W(c);
        const auto t1 = std::chrono::steady_clock::now();
        c->w_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        std::vector<int> f_pair;
        const BtOut bo = host_backtrack(c, f_pair);
        c->bt_steps = bo.steps;
        rc = bt_finish(c, bo, f_pair.data(), st, out);
        c->bt_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    }
    return emit_result(c, rc, st, out, structure, energy_kcal, msgs, msgs_cap);
}

extern "C" int ccj_fill_async_after(ccj_ctx *c, const ccj_ctx *after) {
    if (!c) return CCJ_E_ARG;
    if (c->pending || c->res_pending) return set_err(c, CCJ_E_STATE, "ccj_fill_async: a fold is already in flight");
    if (c->batch) return set_err(c, CCJ_E_STATE, "ccj_fill_async: the context is a member of a lockstep batch");
    if (after && after->device != c->device) return set_err(c, CCJ_E_ARG, "ccj_fill_async_after: contexts on different devices");
    if (const int rc = fill_enqueue(c, after)) return rc;
    // the device traceback follows the fill on the same stream; the host traceback needs the mirror
    return c->host_tb ? CCJ_OK : result_enqueue(c);
}

extern "C" int ccj_fill_async(ccj_ctx *c) { return ccj_fill_async_after(c, nullptr); }

extern "C" int ccj_wait(ccj_ctx *c, char *structure, double *energy_kcal, char *msgs, int msgs_cap) {
    if (!c) return CCJ_E_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = fill_finish(c)) {
        // a refused fold's traceback is already enqueued (over the clamp-only matrices): let it end
        if (rc == CCJ_E_RANGE && c->res_pending) hipEventSynchronize(c->ev_res);
        c->res_pending = false;
        return rc;
    }
    if (c->host_tb) {
        if (const int rc = ccj_sync_host(c)) return rc;
        return ccj_result(c, structure, energy_kcal, msgs, msgs_cap);
    }
    std::string st, out;
    const int rc = result_finish(c, st, out, t0);
    return emit_result(c, rc, st, out, structure, energy_kcal, msgs, msgs_cap);
}

extern "C" int ccj_get4(const ccj_ctx *c, int mat, int i, int j, int k, int l) {
    if (!c || !c->filled || ensure_mirror(c) || mat < 0 || mat >= NMAT4) return INF;
    if (!(i <= j && j < k - 1 && k <= l)) return INF;
    if (i < 1 || l > c->n) return INF;
    const int t = (j - i) + (l - k);
    return (int)c->h4[c->lv_offh[t] + cell_offset_host(c->lv_host[t], mat, j - i, k - j - 2, i)];
}

extern "C" int ccj_get2(const ccj_ctx *c, int mat, int i, int j) {
    if (!c || !c->filled || ensure_mirror_2d(c) || i < 1 || j > c->n || i > j) return INF;
    switch (mat) {
        case CCJ_M2_P: return c->raw2(A2_P, i, j);
        case CCJ_M2_WBP: return c->raw2(A2_WBP, i, j);
        case CCJ_M2_WPP: return c->raw2(A2_WPP, i, j);
        case CCJ_M2_V: return c->raw2(A2_V, i, j);
        case CCJ_M2_VTYPE: return c->hvt[c->a2(i, j)];
        case CCJ_M2_WM: return c->raw2(A2_WM, i, j);
        case CCJ_M2_WMV: return c->raw2(A2_WMV, i, j);
        case CCJ_M2_WMP: return c->raw2(A2_WMP, i, j);
    }
    return INF;
}

extern "C" int ccj_getW(const ccj_ctx *c, int j) {
    if (!c || j < 0 || j >= (int)c->W.size()) return INF;
    return c->W[j];
}

extern "C" int ccj_hashes(const ccj_ctx *cc, uint64_t *out) {
    if (!cc || !cc->filled || !out) return CCJ_E_STATE;
    ccj_ctx *c = const_cast<ccj_ctx *>(cc);
    const int n = c->n;
    const uint64_t H0 = 1469598103934665603ull;
    // 4-D: each matrix is rewritten in canonical (i,j,k,l) order on the GPU (k_canon), copied back,
    // and FNV-hashed on host threads (one chain per matrix)
    const size_t cells = (size_t)ccj_num_cells(n);
    if (cells > 0) {
        HIPCHK(c, hipSetDevice(c->device));
        std::vector<long long> offij((size_t)(n + 1) * (n + 1), 0);
        long long pos = 0;
        for (int i = 1; i <= n; ++i)
            for (int j = i; j <= n; ++j) {
                offij[(size_t)i * (n + 1) + j] = pos;
                for (int k = j + 2; k <= n; ++k) pos += n - k + 1;
            }
        long long *d_off = nullptr;
        int16_t *d_canon = nullptr;
        HIPCHK(c, hipMalloc(&d_off, offij.size() * sizeof(long long)));
        if (hipMalloc(&d_canon, cells * sizeof(int16_t)) != hipSuccess) {
            hipFree(d_off);
            return set_err(c, CCJ_E_OOM, "ccj_hashes: device scratch of %.2f GB", cells * 2e-9);
        }
        HIPCHK(c, hipMemcpy(d_off, offij.data(), offij.size() * sizeof(long long), hipMemcpyHostToDevice));
        std::vector<std::vector<int16_t>> host(NMAT4);
        std::vector<std::thread> th;
        int rc = CCJ_OK;
        for (int m = 0; m < NMAT4 && rc == CCJ_OK; ++m) {
            host[m].resize(cells);
            if (ccjk_canon(&c->T, m, d_off, d_canon, c->st) != 0 ||
                hipMemcpyAsync(host[m].data(), d_canon, cells * sizeof(int16_t), hipMemcpyDeviceToHost, c->st) != hipSuccess ||
                hipStreamSynchronize(c->st) != hipSuccess) {
                rc = set_err(c, CCJ_E_HIP, "ccj_hashes: canonical copy of matrix %d failed", m);
                break;
            }
            th.emplace_back([&host, out, m, H0] {
                out[m] = fnv(H0, host[m].data(), host[m].size() * sizeof(int16_t));
                std::vector<int16_t>().swap(host[m]);
            });
        }
        for (auto &x : th) x.join();
        hipFree(d_off);
        hipFree(d_canon);
        if (rc != CCJ_OK) return rc;
        if (ensure_mirror_2d(c)) return CCJ_E_STATE;
    } else {
        if (ensure_mirror(c)) return CCJ_E_STATE;
        for (int m = 0; m < NMAT4; ++m) {
            uint64_t h = H0;
            for (int i = 1; i <= n; ++i)
                for (int j = i; j <= n; ++j)
                    for (int k = j + 2; k <= n; ++k)
                        for (int l = k; l <= n; ++l) {
                            const int16_t v = (int16_t)ccj_get4(c, m, i, j, k, l);
                            h = fnv(h, &v, 2);
                        }
            out[m] = h;
        }
    }
    for (int m = 0; m < CCJ_NMAT2; ++m) {
        uint64_t h = H0;
        for (int i = 1; i <= n; ++i)
            for (int j = i; j <= n; ++j) {
                const int32_t v = ccj_get2(c, m, i, j);
                h = fnv(h, &v, 4);
            }
        out[NMAT4 + m] = h;
    }
    uint64_t h = H0;
    for (size_t j = 0; j < c->W.size(); ++j) {
        const int32_t v = c->W[j];
        h = fnv(h, &v, 4);
    }
    out[NMAT4 + CCJ_NMAT2] = h;
    return CCJ_OK;
}

extern "C" int ccj_last_timing(const ccj_ctx *c, double *fill_ms, double *kernel_ms3) {
    if (!c) return CCJ_E_ARG;
    if (fill_ms) *fill_ms = c->fill_ms;
    if (kernel_ms3) {
        kernel_ms3[0] = c->level_ms;
        kernel_ms3[1] = c->diag_ms;
        kernel_ms3[2] = c->pre_ms;
    }
    return CCJ_OK;
}


// Algorithmic work model: R4 = sum over cells of 14a + 16b (the linear split-point
// reads of pseudo_loop.cc:181-644) + can_pair-filtered interior-loop candidates and stack terms
// (get_P{L,R,M}iloop :682-773; PO's interior branch reads nothing, A-Q5) ; each read is one int16.
// Writes are 22 int16 per cell.  The 2-D kernel's P recurrence (:166-179) reads 2 int16 per term.
// pr(p, q), 1 <= p < q <= n: the binding's pair type
template <class PR>
static int work_model(int n, PR pr, double *out) {
    auto can = [&](int p, int q) { return (q - p > TURN) && pr(p, q) > 0; };
    // PL/PR window count for outer (p, p+w): u1 <= min(w,30)-2, u2 <= min(w-u1-6, 28)
    std::vector<int> cntW((size_t)(n + 1) * (n + 2), 0);
    for (int w = 0; w < n; ++w)
        for (int p = 1; p + w <= n; ++p) {
            const int q = p + w;
            int cnt = 0;
            for (int u1 = 0; u1 <= std::min(w, MAXLOOP) - 2; ++u1)
                for (int u2 = 0; u2 <= std::min(w - u1 - 6, MAXLOOP - 2); ++u2)
                    cnt += can(p + u1 + 1, q - u2 - 1);
            cntW[(size_t)w * (n + 2) + p] = cnt;
        }
    double reads = 0, cells = 0, ilreads = 0;
    std::vector<int> cum(IE_U * IE_U);
    for (int j = 1; j <= n; ++j)
        for (int g = 2; j + g <= n; ++g) {
            const int k = j + g;
            const bool pm_ok = pr(j, k) > 0 && g > TURN;
            if (pm_ok)
                for (int u1 = 0; u1 < IE_U; ++u1)
                    for (int u2 = 0; u2 < IE_U; ++u2) {
                        const int d = j - 1 - u1, dp = k + 1 + u2;
                        int v = (d >= 1 && dp <= n) ? (int)can(d, dp) : 0;
                        if (u1) v += cum[(u1 - 1) * IE_U + u2];
                        if (u2) v += cum[u1 * IE_U + u2 - 1];
                        if (u1 && u2) v -= cum[(u1 - 1) * IE_U + u2 - 1];
                        cum[u1 * IE_U + u2] = v;
                    }
            for (int a = 0; a < j; ++a) {
                const int i = j - a;
                const bool pl = pr(i, j) > 0 && a > TURN;
                const double rl = pl ? (double)((a > TURN + 2) + cntW[(size_t)a * (n + 2) + i]) : 0.0;
                const double il_l = pl ? (double)cntW[(size_t)a * (n + 2) + i] : 0.0;
                for (int b = 0; k + b <= n; ++b) {
                    const int l = k + b;
                    double r = 14.0 * a + 16.0 * b + rl;
                    double il = il_l;
                    if (b > TURN && pr(k, l) > 0) {
                        r += (b > TURN + 2) + cntW[(size_t)b * (n + 2) + k];
                        il += cntW[(size_t)b * (n + 2) + k];
                    }
                    if (pm_ok) {
                        r += (a >= 1 && b >= 1);
                        if (a >= 2 && b >= 2) {
                            const int cm = cum[std::min(a - 2, IE_U - 1) * IE_U + std::min(b - 2, IE_U - 1)];
                            r += cm;
                            il += cm;
                        }
                    }
                    ilreads += il;
                    if (a >= 1 && b >= 1 && l - i > TURN && pr(i, l) > 0) r += 1;
                    reads += r;
                }
                cells += (double)(n - k + 1);
            }
        }
    double pterms = 0;
    for (int s = 3; s < n; ++s) pterms += (double)(n - s) * ((double)s * (s - 1) * (s - 2) / 6.0);
    out[0] = 2.0 * reads + 44.0 * cells;  // bytes, 4-D level kernels
    out[1] = 4.0 * pterms;                 // bytes, P terms of the 2-D kernels
    out[2] = reads;                        // R4 (4-D part)
    out[3] = cells;
    out[4] = ilreads;                      // interior-loop candidate reads (k_iloop)
    return CCJ_OK;
}

extern "C" int ccj_work_model(const ccj_ctx *c, double *out) {
    if (!c || !out) return CCJ_E_ARG;
    double w[5];
    const int rc = work_model(c->n, [c](int p, int q) { return c->pair_at(p, q); }, w);
    for (int x = 0; x < 4; ++x) out[x] = w[x];
    return rc;
}

extern "C" int ccj_work_split(const ccj_ctx *c, double *out2) {
    if (!c || !out2) return CCJ_E_ARG;
    double w[5];
    const int rc = work_model(c->n, [c](int p, int q) { return c->pair_at(p, q); }, w);
    out2[0] = 2.0 * w[4];                    // k_iloop: candidate reads
    out2[1] = w[0] - out2[0];                // k_level4d: everything else (incl. 44 B of stores per cell)
    return rc;
}

extern "C" int ccj_work_model_seq_constrained(const char *seq, int noGU, const ccj_constraint *cons, double *out) {
    if (!seq || !out) return CCJ_E_ARG;
    const int n = (int)strlen(seq);
    std::vector<uint8_t> mask;
    std::string why;
    if (!constraint_mask(cons, n, mask, why)) return CCJ_E_ARG;
    int pairt[8][8];
    for (int x = 0; x < 8; ++x)
        for (int y = 0; y < 8; ++y) pairt[x][y] = BP_PAIR[x][y];
    if (noGU) pairt[3][4] = pairt[4][3] = 0;
    std::vector<short> S(n + 2, 0);
    for (int i = 1; i <= n; ++i) S[i] = (short)encode_base(seq[i - 1]);
    double w[5];
    const int rc = work_model(
        n, [&](int p, int q) { return !mask.empty() && mask[(size_t)p * (n + 1) + q] ? 0 : pairt[S[p]][S[q]]; }, w);
    for (int x = 0; x < 4; ++x) out[x] = w[x];
    return rc;
}
extern "C" int ccj_work_model_seq(const char *seq, int noGU, double *out) { return ccj_work_model_seq_constrained(seq, noGU, nullptr, out); }

// Kept and full entry counts of the last fill's candidate lists (k_build_il; seg[IL_SEG-1] and
// seg[0] of every pair that can pair): out4 = il kept, il full, ilm kept, ilm full.
extern "C" int ccj_il_counts(ccj_ctx *c, long long *out4) {
    if (!c || !out4) return CCJ_E_ARG;
    if (!c->filled) return set_err(c, CCJ_E_STATE, "ccj_il_counts before a fill");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t plane = (size_t)(c->n + 1) * c->rs;
    std::vector<uint32_t> seg(plane * IL_SEG);
    for (int kind = 0; kind < 2; ++kind) {
        HIPCHK(c, hipMemcpy(seg.data(), kind ? c->d_ilmseg : c->d_ilseg, seg.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        long long kept = 0, full = 0;
        for (int w = 0; w < c->n; ++w)
            for (int p = 1; p + w <= c->n; ++p) {
                const size_t x = (size_t)w * c->rs + p;
                if (c->hpt_h[x] <= 0) continue;  // no list is built for a pair that cannot pair
                kept += seg[x * IL_SEG + IL_SEG - 1];
                full += seg[x * IL_SEG];
            }
        out4[2 * kind] = kept;
        out4[2 * kind + 1] = full;
    }
    return CCJ_OK;
}

// The pruning rule of the candidate lists on the host, no GPU (ccj_ilprune.h: the functions
// k_build_il runs).  Planes are [w][p] with row stride n+2, (n+1)(n+2) elements; windows are
// [plane][IE_U][IE_U] = [..][u1][u2].  Any output may be NULL.
//   counts4: il kept, il full, ilm kept, ilm full over the pairs that can pair (as ccj_il_counts)
//   e_il / e_ilm: the window energies (0 outside the list)
//   st_il / st_ilm: 0 = not in the list, 1 = kept, 1 | 2 * (IL_NEAR | IL_FAR bits) = dropped
//   est, ie: the two planes the rule reads
extern "C" int ccj_il_prune_host_constrained(const ccj_problem *prob, const ccj_constraint *cons, long long *counts4, int16_t *e_il,
                                             int16_t *e_ilm, uint8_t *st_il, uint8_t *st_ilm, int16_t *est_out, int16_t *ie_out) {
    if (!prob || !prob->seq || !prob->params) return CCJ_E_ARG;
    const int n = (int)strlen(prob->seq), rs = n + 2;
    std::vector<uint8_t> mask;
    std::string why;
    if (!constraint_mask(cons, n, mask, why)) return CCJ_E_ARG;
    if (n < 1 || prob->params->magic != CCJ_PARAMS_MAGIC || prob->params->size_bytes != sizeof(ccj_energy_params)) return CCJ_E_ARG;
    ccj_pk_penalties pk = CCJ_PK_PENALTIES_DEFAULT;
    if (prob->pen) pk = *prob->pen;
    int8_t pair[64], rtype[8] = {0, 2, 1, 4, 3, 6, 5, 7};
    for (int x = 0; x < 8; ++x)
        for (int y = 0; y < 8; ++y) pair[x * 8 + y] = (int8_t)BP_PAIR[x][y];
    if (prob->noGU) pair[3 * 8 + 4] = pair[4 * 8 + 3] = 0;
    for (int x = 0; x < 8; ++x)
        for (int y = 0; y < 8; ++y) rtype[pair[x * 8 + y]] = pair[y * 8 + x];
    std::vector<short> S(n + 2, 0), S1(n + 2, 0);
    for (int i = 1; i <= n; ++i) S[i] = S1[i] = (short)encode_base(prob->seq[i - 1]);
    S[n + 1] = S[1], S[0] = (short)n, S1[n + 1] = S1[1], S1[0] = S1[n];
    std::vector<int> lx((size_t)2 * n + 64, 0);
    for (size_t x = 31; x < lx.size(); ++x) lx[x] = (int)(prob->params->lxc * log((double)x / 30.));
    const size_t plane = (size_t)(n + 1) * rs;
    std::vector<int8_t> pt(plane, 0);
    std::vector<int16_t> est(plane, (int16_t)INTERN_INF), ie(plane, (int16_t)INTERN_INF);
    const IlHostTables T{n, rs, S.data(), S1.data(), pt.data(), pair, rtype, prob->params, lx.data(), pk.e_intP, est.data(), ie.data()};
    bool bad = false;
    for (int w = 0; w < n; ++w)  // the binding's relation first: est and ie read the inner pair's type from it
        for (int p = 1; p + w <= n; ++p)
            pt[(size_t)w * rs + p] = !mask.empty() && mask[(size_t)p * (n + 1) + p + w] ? 0 : pair[S[p] * 8 + S[p + w]];
    for (int w = 0; w < n; ++w)
        for (int p = 1; p + w <= n; ++p) {
            const int q = p + w;
            const size_t x = (size_t)w * rs + p;
            if (q - p >= 2 && p + 1 != q - 1) {  // get_e_stP as seq_setup saturates it
                const int t2 = pt[(size_t)(w - 2) * rs + p + 1];
                const long v = lrint(pk.e_stP * E_IntLoop(prob->params, lx.data(), 0, 0, pt[x], rtype[t2], S1[p + 1], S1[q - 1], S1[p], S1[q]));
                if (v < -32768 || (pt[x] > 0 && t2 > 0 && v >= INTERN_INF)) bad = true;
                est[x] = (int16_t)(v >= INTERN_INF ? INTERN_INF : v);
            }
            const int v = il_eint_raw(T, 0, 0, p, q);  // k_precompute_ie
            if (v != INTERN_INF && !il_e_in_range(v)) bad = true;
            ie[x] = (int16_t)v;
        }
    if (bad) return CCJ_E_PARAMS;
    long long cnt[4] = {0, 0, 0, 0};
    int es[IE_U][IE_U];
    bool in[IE_U][IE_U];
    for (int kind = 0; kind < 2; ++kind) {
        int16_t *eo = kind ? e_ilm : e_il;
        uint8_t *so = kind ? st_ilm : st_il;
        if (eo) memset(eo, 0, plane * IE_U * IE_U * sizeof(int16_t));
        if (so) memset(so, 0, plane * IE_U * IE_U);
        for (int w = 0; w < n; ++w)
            for (int p = 1; p + w <= n; ++p) {
                const size_t x = (size_t)w * rs + p;
                if (pt[x] <= 0) continue;
                const int q = p + w;
                for (int u1 = 0; u1 < IE_U; ++u1)
                    for (int u2 = 0; u2 < IE_U; ++u2) {
                        es[u1][u2] = 0;
                        in[u1][u2] = il_window(T, kind, p, q, u1, u2, es[u1][u2]);
                        if (in[u1][u2] && !il_e_in_range(es[u1][u2])) return CCJ_E_PARAMS;
                    }
                for (int u1 = 0; u1 < IE_U; ++u1)
                    for (int u2 = 0; u2 < IE_U; ++u2) {
                        if (!in[u1][u2]) continue;
                        const int dom = (u1 && u2) ? il_dominated(T, kind, p, q, u1, u2, es[u1][u2], in[0][0], es[0][0],
                                                                  in[u1 - 1][u2 - 1], es[u1 - 1][u2 - 1])
                                                   : 0;
                        cnt[2 * kind] += dom == 0;
                        cnt[2 * kind + 1] += 1;
                        const size_t o = (x * IE_U + u1) * IE_U + u2;
                        if (eo) eo[o] = (int16_t)es[u1][u2];
                        if (so) so[o] = (uint8_t)(1 | 2 * dom);
                    }
            }
    }
    if (counts4) memcpy(counts4, cnt, sizeof cnt);
    if (est_out) memcpy(est_out, est.data(), plane * sizeof(int16_t));
    if (ie_out) memcpy(ie_out, ie.data(), plane * sizeof(int16_t));
    return CCJ_OK;
}

extern "C" int ccj_il_prune_host(const ccj_problem *prob, long long *counts4, int16_t *e_il, int16_t *e_ilm, uint8_t *st_il,
                                 uint8_t *st_ilm, int16_t *est_out, int16_t *ie_out) {
    return ccj_il_prune_host_constrained(prob, nullptr, counts4, e_il, e_ilm, st_il, st_ilm, est_out, ie_out);
}

extern "C" int ccj_host_timing(const ccj_ctx *c, double *out3) {
    if (!c || !out3) return CCJ_E_ARG;
    out3[0] = c->sync_ms;
    out3[1] = c->w_ms;
    out3[2] = c->bt_ms;
    return CCJ_OK;
}

extern "C" int ccj_level_times(const ccj_ctx *c, double *level_ms, double *diag_ms, int cap) {
    if (!c) return CCJ_E_ARG;
    for (int t = 0; t < cap && t < (int)c->lev_ms_v.size(); ++t) {
        if (level_ms) level_ms[t] = c->lev_ms_v[t];
        if (diag_ms) diag_ms[t] = c->diag_ms_v[t];
    }
    return CCJ_OK;
}

extern "C" int ccj_iloop_times(const ccj_ctx *c, double *iloop_ms, int cap) {
    if (!c || !iloop_ms) return CCJ_E_ARG;
    for (int t = 0; t < cap && t < (int)c->il_ms_v.size(); ++t) iloop_ms[t] = c->il_ms_v[t];
    return CCJ_OK;
}

extern "C" int ccj_exchange_times(const ccj_ctx *c, double *edge_ms, double *bulk_ms, int cap) {
    if (!c || (!edge_ms && !bulk_ms)) return CCJ_E_ARG;
    for (int t = 0; t < cap && t < (int)c->xch_ms_v.size(); ++t) {
        if (edge_ms) edge_ms[t] = c->xch_ms_v[t];
        if (bulk_ms) bulk_ms[t] = c->xbulk_ms_v[t];
    }
    return CCJ_OK;
}

extern "C" double ccj_iloop_ms(const ccj_ctx *c) { return c ? c->il_ms : 0.0; }
extern "C" double ccj_ppush_ms(const ccj_ctx *c) { return c ? c->pp_ms : 0.0; }
extern "C" int ccj_ppush_times(const ccj_ctx *c, double *ppush_ms, int cap) {
    if (!c || !ppush_ms) return CCJ_E_ARG;
    for (int t = 0; t < cap && t < (int)c->pp_ms_v.size(); ++t) ppush_ms[t] = c->pp_ms_v[t];
    return CCJ_OK;
}

extern "C" int ccj_set_timing(ccj_ctx *c, int mode) {
    if (!c || mode < 0 || mode > 2) return CCJ_E_ARG;
    c->level_timing = mode;
    return CCJ_OK;
}

extern "C" int ccj_shard_blocks(int n, int t, int world, int rank, int *a_out, int cap) {
    if (world < 1 || rank < 0 || rank >= world || t < 0 || (cap > 0 && !a_out)) return -CCJ_E_ARG;
    (void)n;
    const int cnt = shard_count(t, world, rank);
    for (int o = 0; o < cnt && o < cap; ++o) a_out[o] = shard_a(o, world, rank);
    return cnt;
}

// The launch regime of level t for one rank (ccj_engine.h level_sched: what create_impl,
// ccjk_level4d and ccjk_level4d_lead use), without a context ...
extern "C" int ccj_level_schedule(int n, int t, int world, int rank, int split_target, int share, int *out5) {
    if (!out5 || n < 1 || world < 1 || rank < 0 || rank >= world || t < 0 || split_target < 0) return CCJ_E_ARG;
    int g_lo, g_hi;
    sched_share_range(n, split_target, share != 0, g_lo, g_hi);
    const LevelSched s = level_sched(n, t, world, rank, split_target, g_lo, g_hi, -1, share_edges_env());
    out5[0] = s.sharing, out5[1] = s.split, out5[2] = s.lead_split, out5[3] = g_lo, out5[4] = g_hi;
    return CCJ_OK;
}

// ... and of a live context: the range it created its lists for, the leader list it launches from
extern "C" int ccj_ctx_level_schedule(const ccj_ctx *c, int t, int rank, int *out7) {
    if (!c || !out7 || t < 0) return CCJ_E_ARG;
    if (rank < 0) rank = c->rank;
    if (rank >= c->world || (!c->simulate && rank != c->rank)) return CCJ_E_ARG;
    const int G = c->world, g_lo = c->T.g_lo, g_hi = c->T.g_hi;
    int lead_nblk = 0;
    if (t >= g_lo && t < g_hi)
        lead_nblk = c->lord_off.empty() ? shard_count(t, G, rank) : c->lord_off[(size_t)t * G + rank + 1] - c->lord_off[(size_t)t * G + rank];
    const LevelSched s = level_sched(c->n, t, G, rank, c->split_target, g_lo, g_hi, lead_nblk);
    out7[0] = s.sharing, out7[1] = s.split, out7[2] = s.lead_split, out7[3] = g_lo, out7[4] = g_hi;
    out7[5] = c->split_target, out7[6] = c->share ? 1 : 0;
    return CCJ_OK;
}

// The sharing roles of a-block a of level t (ccj_engine.h share_role: what level4d_body and the
// leader lists use), without a context or a GPU.  Per side (a-loop at 0, b-loop at 6): role, the
// split points the cell scans itself (low, top) and, for a leader, the cut of follower r = 1 .. 3;
// then whether k_level4d_lead runs the block, whether level t shares, g_lo, g_hi.
extern "C" int ccj_share_roles(int n, int t, int a, int split_target, int edges, int *out16) {
    if (!out16 || n < 1 || t < 0 || a < 0 || a > t || n - t - 2 <= 0 || split_target < 0) return CCJ_E_ARG;
    int g_lo, g_hi;
    sched_share_range(n, split_target, true, g_lo, g_hi);
    const bool grp = t >= g_lo && t < g_hi;
    const int len[2] = {a, t - a};
    for (int s = 0; s < 2; ++s) {
        const ShareRole R = share_role(grp, edges != 0, len[s], len[1 - s], g_lo);
        int *o = out16 + 6 * s;
        o[0] = R.role, o[1] = R.low, o[2] = R.top;
        for (int r = 1; r <= 3; ++r) o[2 + r] = R.role == 1 && r < SHARE_R ? share_cut(r, len[1 - s]) : 0;
    }
    out16[12] = grp && sched_lead_block(t, a, g_lo, edges != 0, nullptr);
    out16[13] = grp, out16[14] = g_lo, out16[15] = g_hi;
    return CCJ_OK;
}

extern "C" int ccj_level_layout(int n, int t, int world, long long *C, int *M) {
    if (!C || !M || world < 1 || t < 0) return CCJ_E_ARG;
    const int m = n - t - 2;
    *M = m > 0 ? m * (m + 1) / 2 : 0;
    *C = (long long)(t + 1) * *M;  // unpadded for every world (the exchange packs slices)
    return CCJ_OK;
}

// The exchange geometry k_pack / k_unpack use (ccj_engine.h xch_*), per part (0 = edge, 1 = bulk),
// for tests and integrators: {nmax, tail offset (= padded body), slice elements}.
extern "C" int ccj_exchange_layout(int n, int t, int world, int part, long long *out3) {
    if (!out3 || world < 1 || t < 0 || n < 4 || t > n - 3 || (part != XCH_EDGE && part != XCH_BULK)) return CCJ_E_ARG;
    const int m = n - t - 2, M = m * (m + 1) / 2, nmax = xch_nmax(t, world, part);
    out3[0] = nmax;
    out3[1] = xch_body(nmax, M);                // the part's tail (edge: P(t+1) partials, then span t; bulk: none)
    out3[2] = xch_slice(n, nmax, M, part);      // slice elements
    return CCJ_OK;
}

// which == 0 (pack, rank `rank`): out[k] for every body element k of the rank's slice of the part =
//   the level element (x * C + a * M + c) k_pack copies there, -1 for padding;
// which == 1 (unpack at rank `rank`): out[e] for every level element e = x * C + a * M + c = the
//   position in the part's gathered buffer (owner * slice + body position) k_unpack reads it from, -1
//   for the rank's own cells and the other part's.
// Returns the number of entries (cap: the room in out), or -CCJ_E_ARG.
extern "C" long long ccj_exchange_index(int n, int t, int world, int rank, int part, int which, long long *out, long long cap) {
    if (world < 1 || rank < 0 || rank >= world || t < 0 || n < 4 || t > n - 3 || (which != 0 && which != 1) ||
        (part != XCH_EDGE && part != XCH_BULK))
        return -CCJ_E_ARG;
    const int m = n - t - 2, M = m * (m + 1) / 2, nmax = xch_nmax(t, world, part);
    const long long C = (long long)(t + 1) * M, slice = xch_slice(n, nmax, M, part);
    const long long cnt = which == 0 ? (long long)NMAT4 * nmax * M : (long long)NMAT4 * C;
    if (cap < cnt || !out) return cnt;
    if (which == 0) {
        for (long long k = 0; k < cnt; ++k) out[k] = -1;
        const int np = xch_pcount(t, world, rank, part);
        for (int x = 0; x < NMAT4; ++x)
            for (int k = 0; k < np; ++k)
                for (int c = 0; c < M; ++c)
                    out[xch_pos(x, k, c, nmax, M)] = x * C + (long long)shard_a(xch_own(k, part), world, rank) * M + c;
    } else {
        for (int x = 0; x < NMAT4; ++x)
            for (int a = 0; a <= t; ++a) {
                int ro, pa, k;
                xch_src(a, world, ro, pa, k);
                for (int c = 0; c < M; ++c)
                    out[x * C + (long long)a * M + c] = (ro == rank || pa != part) ? -1 : ro * slice + xch_pos(x, k, c, nmax, M);
            }
    }
    return cnt;
}

extern "C" int ccj_comm_unique_id(char *id_out) {
    if (!id_out) return CCJ_E_ARG;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return CCJ_E_HIP;
    static_assert(sizeof(id) == CCJ_COMM_ID_BYTES, "RCCL unique id size");
    memcpy(id_out, &id, sizeof id);
    return CCJ_OK;
}

extern "C" int ccj_comm_init(ccj_ctx *c, const char *id_in) {
    if (!c || !id_in) return CCJ_E_ARG;
    if (c->world == 1 || c->simulate) return CCJ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    ncclUniqueId id;
    memcpy(&id, id_in, sizeof id);
    if (c->xch.comm_b) ncclCommDestroy(c->xch.comm_b);
    if (c->xch.comm) ncclCommDestroy(c->xch.comm);
    c->xch.comm = c->xch.comm_b = nullptr;
    const ncclResult_t r = ncclCommInitRank(&c->xch.comm, c->world, id, c->rank);
    if (r != ncclSuccess) return set_err(c, CCJ_E_HIP, "ncclCommInitRank: %s", ncclGetErrorString(r));
    // the bulk all-gathers run on their own stream: their own communicator (same ranks, same order), so
    // the two streams' collectives never queue behind each other inside one communicator
    const ncclResult_t r2 = ncclCommSplit(c->xch.comm, 0, c->rank, &c->xch.comm_b, nullptr);
    if (r2 != ncclSuccess) return set_err(c, CCJ_E_HIP, "ncclCommSplit: %s", ncclGetErrorString(r2));
    return CCJ_OK;
}

extern "C" int ccj_group_create(int world, ccj_group **out) {
    if (!out || world < 1) return CCJ_E_ARG;
    *out = new ccj_group();
    (*out)->world = world;
    (*out)->members.assign(world, nullptr);
    return CCJ_OK;
}

extern "C" void ccj_group_destroy(ccj_group *g) { delete g; }

extern "C" int ccj_comm_init_local(ccj_ctx *c, ccj_group *g) {
    if (!c || !g || g->world != c->world || c->world < 2 || c->simulate) return CCJ_E_ARG;
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->members[c->rank] && g->members[c->rank] != c)
        return set_err(c, CCJ_E_STATE, "ccj_comm_init_local: rank %d of the group is already taken", c->rank);
    g->members[c->rank] = c;
    c->xch.lgroup = g;
    return CCJ_OK;
}

extern "C" int ccj_n(const ccj_ctx *c) { return c ? c->n : 0; }
extern "C" const char *ccj_last_error(const ccj_ctx *c) { return c ? c->err.c_str() : g_create_err.c_str(); }
extern "C" int ccj_range_flags(const ccj_ctx *c) { return c ? c->range_flags : 0; }

extern "C" void ccj_destroy(ccj_ctx *c) {
    if (!c || c->batch) return;  // a batch member is borrowed: ccj_batch_destroy frees it
    bool leak_send = false;
    if (c->xch.lgroup) {  // leave the in-process group: no member may copy from this context's buffers
        ccj_group *g = c->xch.lgroup;
        std::unique_lock<std::mutex> lk(g->mu);
        if (g->members[c->rank] == c) {  // registered (a failed ccj_comm_init_local never was)
            g->members[c->rank] = nullptr;
            g->broken = true;  // the exchange cannot complete without this rank
            g->cv.notify_all();
        }
        // peers still copying from d_send; bounded like the group's barriers (a peer stuck in a
        // GPU call must not hang this destroy): on timeout d_send is leaked instead of freed
        if (!g->cv.wait_for(lk, std::chrono::seconds(120), [&] { return g->busy == 0; })) {
            fprintf(stderr, "ccj_destroy: a group member is still copying after 120 s; leaking its source buffer\n");
            leak_send = true;
        }
        // the peers' asynchronous bulk copies (local_bulk_gather) from this member's send slice
        for (ccj_ctx *p : g->members)
            if (p && p->xch.st_x) hipStreamSynchronize(p->xch.st_x);
        c->xch.lgroup = nullptr;
    }
    hipSetDevice(c->device);
    Exchange &x = c->xch;
    for (hipStream_t q : {c->st, c->st_copy, c->fs.st_p, c->fs.st_il, x.st_d, x.st_x})
        if (q) hipStreamSynchronize(q);
    for (void *p : {(void *)c->d4, (void *)c->d_ie, (void *)c->d_est, (void *)c->d_hp, (void *)c->d_pt, (void *)c->d_pair,
                    (void *)c->d_rtype, (void *)c->d_lx, (void *)c->d_err, (void *)c->d_S, (void *)c->d_S1, (void *)c->d_prm,
                    (void *)c->d_lv, (void *)c->d_lb, (void *)c->d_ld, (void *)c->d4x_alloc, (void *)c->d_icount,
                    (void *)c->d_ioff, (void *)c->d_rec, (void *)c->d_rk, (void *)c->d_rl, (void *)c->d_cf, (void *)c->d_acc,
                    (void *)c->d_wterm, (void *)c->d_lord, (void *)c->d_lord_off, (void *)c->d_wbw, (void *)c->d_tab,
                    (void *)c->pmx_alloc, (void *)c->d_ldx, (void *)c->d_il, (void *)c->d_ilm, (void *)c->d_dummy,
                    (void *)c->d_items, (void *)c->d_ilseg, (void *)c->d_ilmseg, (void *)c->d2i, (void *)c->d_pk, (void *)c->d_W,
                    (void *)c->d_fpair, (void *)c->d_ftype, (void *)c->d_btout, (void *)c->d_vt})
        hipFree(p);
    for (int part = 0; part < 2; ++part) {
        if (!leak_send) hipFree(x.d_send[part]);
        hipFree(x.d_recv[part]);
    }
    if (c->h_stage) hipHostFree(c->h_stage);
    if (c->h_bind) hipHostFree(c->h_bind);
    if (c->ev_bind) hipEventDestroy(c->ev_bind);
    if (c->h_ioff) hipHostFree(c->h_ioff);
    if (c->h_icount) hipHostFree(c->h_icount);
    if (c->ev_stage) hipEventDestroy(c->ev_stage);
    if (c->hr_W) hipHostFree(c->hr_W);
    if (c->hr_fp) hipHostFree(c->hr_fp);
    if (c->hr_ft) hipHostFree(c->hr_ft);
    if (c->hr_bo) hipHostFree(c->hr_bo);
    if (c->ev_res) hipEventDestroy(c->ev_res);
    if (c->h4) hipHostFree(c->h4);
    for (auto *v : {&x.pp_done, &x.bulk_done, &c->tev})
        for (hipEvent_t e : *v)
            if (e) hipEventDestroy(e);
    for (hipEvent_t e : {x.ev_bpacked, x.ev_bcopied})
        if (e) hipEventDestroy(e);
    if (x.comm_b) ncclCommDestroy(x.comm_b);
    if (x.comm) ncclCommDestroy(x.comm);
    fill_sync_destroy(c->fs);
    for (hipStream_t q : {x.st_d, x.st_x, c->st, c->st_copy})
        if (q) hipStreamDestroy(q);
    delete c;
}

// ============================================================================================
// Lockstep batch (include/ccj.h): K capacity contexts whose fills run as ONE
// wavefront over the steps s = 0 .. max(n_k)-1.  Every kernel of a step is launched once for all
// bound members (ccj_engine.h k_*_many), so the per-level chain of launches and events, which is
// what a short fold costs, is paid once per batch.  The graph is enqueue_level_dag, on the batch's
// own streams and events (by step), with BatchLaunch's launches.  Members never share split points
// (created with sharing off: g_lo = g_hi = 0, no leader launch).
// ============================================================================================
struct ccj_batch {
    int device = 0, ncap = 0, K = 0;
    int count = 0;            // bound members: 0 .. count-1 (the others idle)
    int nb = 0;               // the longest bound length: steps of a fold
    int split_target = 0;
    std::vector<ccj_ctx *> m;
    std::vector<int> n;       // bound lengths
    hipStream_t st = nullptr;
    FillSync fs;
    hipEvent_t ev_res = nullptr, ev_args = nullptr;
    // per member: tables, result pointers; per (step, member): launch arguments; device + pinned staging
    DevTables *d_tabs = nullptr, *h_tabs = nullptr;
    BatchRes *d_res = nullptr, *h_res = nullptr;
    LevelArgs *d_args = nullptr, *h_args = nullptr;
    // contiguous results, K x (ncap + 1) (BtOut, err: K), so a fold ends in one copy per array
    int *d_W = nullptr, *d_fp = nullptr, *d_err = nullptr, *h_W = nullptr, *h_fp = nullptr, *h_err = nullptr;
    int8_t *d_ft = nullptr, *h_ft = nullptr;
    BtOut *d_bo = nullptr, *h_bo = nullptr;
    bool pending = false;
    double fill_ms = 0;
    std::string err;
    size_t stride() const { return (size_t)ncap + 1; }
};

static thread_local std::string g_batch_err;

static int batch_err(ccj_batch *b, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_batch_err = buf;
    if (b) b->err = buf;
    return code;
}
#define BHIP(b, x)                                                                                  \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) return batch_err((b), CCJ_E_HIP, "%s: %s", #x, hipGetErrorString(e_)); \
    } while (0)

// A batch's launches for enqueue_level_dag: one k_*_many per family over the cnt bound members, with
// the step's rows of launch arguments (device, and the pinned staging they were uploaded from).
struct BatchLaunch {
    const ccj_batch *b;
    int cnt, nb;
    const LevelArgs *row(int s) const { return b->d_args + (size_t)s * b->K; }
    const LevelArgs *hrow(int s) const { return b->h_args + (size_t)s * b->K; }
    hipError_t pre(hipStream_t q) const { return (hipError_t)ccjk_pre_many(b->d_tabs, cnt, nb, q); }
    hipError_t iloop(int s, hipStream_t q) const { return (hipError_t)ccjk_iloop_many(b->d_tabs, row(s), hrow(s), cnt, s, q); }
    hipError_t diag(int sg, hipStream_t q) const { return (hipError_t)ccjk_diag2d_many(b->d_tabs, row(sg), hrow(sg), cnt, sg, q); }
    // behind the last span: every member's closed-form range check (site CF)
    hipError_t behind_span(int sg, hipStream_t q) const {
        return sg == nb - 1 ? (hipError_t)ccjk_cf_low_many(b->d_tabs, cnt, nb, q) : hipSuccess;
    }
    hipError_t level(int s, hipStream_t q) const {
        return (hipError_t)ccjk_level4d_many(b->d_tabs, row(s), b->n.data(), cnt, s, b->split_target, q);
    }
    hipError_t ppush(int s, hipStream_t q) const { return (hipError_t)ccjk_ppush_many(b->d_tabs, row(s), hrow(s), cnt, s, q); }
};

extern "C" void ccj_batch_destroy(ccj_batch *b) {
    if (!b) return;
    hipSetDevice(b->device);
    for (hipStream_t q : {b->st, b->fs.st_p, b->fs.st_il})
        if (q) hipStreamSynchronize(q);
    for (ccj_ctx *c : b->m) {
        if (!c) continue;
        // what points into the batch's buffers is the batch's to free
        c->d_W = c->d_fpair = c->d_err = nullptr;
        c->d_ftype = nullptr;
        c->d_btout = nullptr;
        c->hr_W = c->hr_fp = nullptr;
        c->hr_ft = nullptr;
        c->hr_bo = nullptr;
        c->batch = nullptr;
        ccj_destroy(c);
    }
    hipFree(b->d_tabs);
    hipFree(b->d_res);
    hipFree(b->d_args);
    hipFree(b->d_W);
    hipFree(b->d_fp);
    hipFree(b->d_ft);
    hipFree(b->d_bo);
    hipFree(b->d_err);
    for (void *p : {(void *)b->h_tabs, (void *)b->h_res, (void *)b->h_args, (void *)b->h_W, (void *)b->h_fp, (void *)b->h_ft,
                    (void *)b->h_bo, (void *)b->h_err})
        if (p) hipHostFree(p);
    for (hipEvent_t e : {b->ev_res, b->ev_args})
        if (e) hipEventDestroy(e);
    fill_sync_destroy(b->fs);
    if (b->st) hipStreamDestroy(b->st);
    delete b;
}

static int batch_create_impl(const ccj_problem *p, const ccj_options *o, int nmax, int members, ccj_batch *b) {
    b->device = o ? o->device : 0;
    b->ncap = nmax;
    b->K = members;
    BHIP(b, hipSetDevice(b->device));
    // members: lean d4, device traceback, sharing off, each bound to p->seq (or a placeholder) until
    // the first ccj_batch_bind
    ccj_options mo{};
    if (o) mo = *o;
    mo.overlap_d2h = 0;
    mo.share_splits = -1;
    ccj_problem mp = *p;
    if (!mp.seq) mp.seq = "A";
    b->m.assign(members, nullptr);
    for (int k = 0; k < members; ++k) {
        std::unique_ptr<ccj_ctx> c(new ccj_ctx());
        c->member = true;
        if (const int rc = create_impl(&mp, &mo, nmax, c, &b->m[k])) {
            const std::string why = c && !c->err.empty() ? c->err : std::string("invalid problem (sequence alphabet, length or parameter blob)");
            if (c) ccj_destroy(c.release());
            return batch_err(b, rc, "member %d: %s", k, why.c_str());
        }
        if (b->m[k]->full4) return batch_err(b, CCJ_E_ARG, "a lockstep batch needs lean members (CCJ_D4_FULL is set)");
    }
    b->split_target = b->m[0]->split_target;
    BHIP(b, hipStreamCreateWithFlags(&b->st, hipStreamNonBlocking));
    BHIP(b, fill_sync_create(b->fs, (size_t)nmax + 1, false));
    BHIP(b, hipEventCreateWithFlags(&b->ev_res, hipEventDisableTiming));
    BHIP(b, hipEventCreateWithFlags(&b->ev_args, hipEventDisableTiming));
    const size_t K = (size_t)members, st = b->stride(), nargs = (size_t)nmax * K;
    BHIP(b, hipMalloc(&b->d_tabs, K * sizeof(DevTables)));
    BHIP(b, hipMalloc(&b->d_res, K * sizeof(BatchRes)));
    BHIP(b, hipMalloc(&b->d_args, nargs * sizeof(LevelArgs)));
    BHIP(b, hipMalloc(&b->d_W, K * st * sizeof(int)));
    BHIP(b, hipMalloc(&b->d_fp, K * st * sizeof(int)));
    BHIP(b, hipMalloc(&b->d_ft, K * st));
    BHIP(b, hipMalloc(&b->d_bo, K * sizeof(BtOut)));
    BHIP(b, hipMalloc(&b->d_err, K * sizeof(int)));
    BHIP(b, hipHostMalloc(&b->h_tabs, K * sizeof(DevTables), hipHostMallocDefault));
    BHIP(b, hipHostMalloc(&b->h_res, K * sizeof(BatchRes), hipHostMallocDefault));
    BHIP(b, hipHostMalloc(&b->h_args, nargs * sizeof(LevelArgs), hipHostMallocDefault));
    BHIP(b, hipHostMalloc(&b->h_W, K * st * sizeof(int), hipHostMallocDefault));
    BHIP(b, hipHostMalloc(&b->h_fp, K * st * sizeof(int), hipHostMallocDefault));
    BHIP(b, hipHostMalloc(&b->h_ft, K * st, hipHostMallocDefault));
    BHIP(b, hipHostMalloc(&b->h_bo, K * sizeof(BtOut), hipHostMallocDefault));
    BHIP(b, hipHostMalloc(&b->h_err, K * sizeof(int), hipHostMallocDefault));
    BHIP(b, hipMemset(b->d_err, 0, K * sizeof(int)));
    // the members' result arrays and error words become slices of the batch's
    for (int k = 0; k < members; ++k) {
        ccj_ctx *c = b->m[k];
        BHIP(b, hipStreamSynchronize(c->st));  // its creation's setup used d_err
        hipFree(c->d_W);
        hipFree(c->d_fpair);
        hipFree(c->d_ftype);
        hipFree(c->d_btout);
        hipFree(c->d_err);
        c->d_W = b->d_W + k * st;
        c->d_fpair = b->d_fp + k * st;
        c->d_ftype = b->d_ft + k * st;
        c->d_btout = b->d_bo + k;
        c->d_err = c->T.err = b->d_err + k;
        c->hr_W = b->h_W + k * st;
        c->hr_fp = b->h_fp + k * st;
        c->hr_ft = b->h_ft + k * st;
        c->hr_bo = b->h_bo + k;
        c->batch = b;
    }
    return CCJ_OK;
}

extern "C" int ccj_batch_create(const ccj_problem *p, const ccj_options *o, int nmax, int members, ccj_batch **out) {
    if (!out) return CCJ_E_ARG;
    *out = nullptr;
    if (!p || !p->params || nmax < 1 || members < 1) return batch_err(nullptr, CCJ_E_ARG, "ccj_batch_create: bad arguments");
    if (o && (o->shard_world > 1 || o->host_traceback || o->overlap_d2h || o->share_splits > 0))
        return batch_err(nullptr, CCJ_E_ARG, "ccj_batch_create: no band sharding, host traceback, host mirror stream or sharing");
    ccj_batch *b = new ccj_batch();
    const int rc = batch_create_impl(p, o, nmax, members, b);
    if (rc != CCJ_OK) {
        const std::string keep = g_batch_err;
        ccj_batch_destroy(b);
        g_batch_err = keep;
        return rc;
    }
    *out = b;
    return CCJ_OK;
}

extern "C" const char *ccj_batch_last_error(const ccj_batch *b) { return b ? b->err.c_str() : g_batch_err.c_str(); }
extern "C" int ccj_batch_members(const ccj_batch *b) { return b ? b->K : 0; }
extern "C" int ccj_batch_count(const ccj_batch *b) { return b ? b->count : 0; }
extern "C" ccj_ctx *ccj_batch_member(ccj_batch *b, int k) { return b && k >= 0 && k < b->K ? b->m[k] : nullptr; }

static int batch_bind_impl(ccj_batch *b, const char *const *seqs, const ccj_constraint *const *cons, int count) {
    if (!b || !seqs) return CCJ_E_ARG;
    if (b->pending) return batch_err(b, CCJ_E_STATE, "ccj_batch_bind: a fold is in flight (ccj_batch_wait first)");
    if (count < 1 || count > b->K) return batch_err(b, CCJ_E_ARG, "ccj_batch_bind: count %d outside 1..%d", count, b->K);
    // every sequence is checked before any member moves: a refused bind leaves the previous binding
    for (int k = 0; k < count; ++k) {
        const size_t len = seqs[k] ? strlen(seqs[k]) : 0;
        if (len < 1 || len > (size_t)b->ncap)
            return batch_err(b, CCJ_E_ARG, "ccj_batch_bind: sequence %d has length %zu outside 1..%d", k, len, b->ncap);
        for (const char *q = seqs[k]; *q; ++q)
            if (!(*q == 'A' || *q == 'C' || *q == 'G' || *q == 'U' || *q == 'T'))
                return batch_err(b, CCJ_E_ARG, "ccj_batch_bind: invalid character in sequence %d", k);
    }
    // ... and every constraint
    std::vector<std::vector<uint8_t>> masks(count);
    for (int k = 0; k < count && cons; ++k) {
        std::string why;
        if (!constraint_mask(cons[k], (int)strlen(seqs[k]), masks[k], why))
            return batch_err(b, CCJ_E_ARG, "ccj_batch_bind: bad constraint of sequence %d: %s", k, why.c_str());
    }
    BHIP(b, hipSetDevice(b->device));
    const int prev = b->count;
    b->count = 0;  // unbound until every member is
    for (int k = 0; k < count; ++k)
        if (const int rc = rebind_impl(b->m[k], seqs[k], false, "ccj_batch_bind", true, cons && cons[k] ? &masks[k] : nullptr))
            return batch_err(b, rc, "member %d: %s", k, b->m[k]->err.c_str());
    for (int k = count; k < prev; ++k) b->m[k]->filled = b->m[k]->res_ready = false;  // idle now
    // tables, result pointers and every step's launch arguments, through pinned staging
    BHIP(b, hipEventSynchronize(b->ev_args));  // the previous upload has read the staging
    b->n.assign(count, 0);
    b->nb = 0;
    for (int k = 0; k < count; ++k) {
        ccj_ctx *c = b->m[k];
        b->n[k] = c->n;
        b->nb = std::max(b->nb, c->n);
        b->h_tabs[k] = c->T;
        b->h_res[k] = BatchRes{c->d_W, c->d_wterm, c->d_fpair, c->d_ftype, c->d_btout, bt_stack_cap(c->n), 0};
    }
    const size_t K = (size_t)b->K;
    for (int s = 0; s < b->nb; ++s)
        for (int k = 0; k < count; ++k) {
            const ccj_ctx *c = b->m[k];
            const bool lev = s < c->nlev && (size_t)s + 1 < c->it_off.size();
            ccjk_batch_args(c->n, s, lev ? c->it_off[s] : 0, lev ? (int)(c->it_off[s + 1] - c->it_off[s]) : 0, &b->h_args[s * K + k]);
        }
    BHIP(b, hipMemcpyAsync(b->d_tabs, b->h_tabs, count * sizeof(DevTables), hipMemcpyHostToDevice, b->st));
    BHIP(b, hipMemcpyAsync(b->d_res, b->h_res, count * sizeof(BatchRes), hipMemcpyHostToDevice, b->st));
    BHIP(b, hipMemcpyAsync(b->d_args, b->h_args, (size_t)b->nb * K * sizeof(LevelArgs), hipMemcpyHostToDevice, b->st));
    BHIP(b, hipEventRecord(b->ev_args, b->st));
    // the members' own setup (layout kernel, sequence tables, work items) runs on their streams
    for (int k = 0; k < count; ++k) BHIP(b, hipStreamWaitEvent(b->st, b->m[k]->ev_stage, 0));
    b->count = count;
    return CCJ_OK;
}

extern "C" int ccj_batch_bind(ccj_batch *b, const char *const *seqs, int count) { return batch_bind_impl(b, seqs, nullptr, count); }
extern "C" int ccj_batch_bind_constrained(ccj_batch *b, const char *const *seqs, const ccj_constraint *const *cons, int count) {
    return batch_bind_impl(b, seqs, cons, count);
}

extern "C" int ccj_batch_fold_async(ccj_batch *b) {
    if (!b) return CCJ_E_ARG;
    if (b->pending) return batch_err(b, CCJ_E_STATE, "ccj_batch_fold_async: a fold is already in flight");
    if (b->count < 1) return batch_err(b, CCJ_E_STATE, "ccj_batch_fold_async: no binding (ccj_batch_bind first)");
    BHIP(b, hipSetDevice(b->device));
    const int cnt = b->count, nb = b->nb, nlev = nb > 2 ? nb - 2 : 0;
    hipStream_t st = b->st;
    for (int k = 0; k < cnt; ++k) {
        ccj_ctx *c = b->m[k];
        c->filled = c->mirrored = c->mirrored2d = c->res_ready = false;
    }
    BHIP(b, hipMemsetAsync(b->d_err, 0, cnt * sizeof(int), st));
    BHIP(b, hipEventRecord(b->fs.ev_start, st));
    BHIP(b, enqueue_level_dag(b->fs, st, nb, nlev, BatchLaunch{b, cnt, nb}));
    BHIP(b, hipStreamWaitEvent(st, b->fs.dg_done[nb - 1], 0));
    BHIP(b, hipEventRecord(b->fs.ev_end, st));
    // W and the traceback, one workgroup per member, then one copy per result array
    int capmax = 0;
    for (int k = 0; k < cnt; ++k) capmax = std::max(capmax, bt_stack_cap(b->n[k]));
    BHIP(b, (hipError_t)ccjk_compute_W_many(b->d_tabs, b->d_res, cnt, nb, st));
    BHIP(b, (hipError_t)ccjk_backtrack_many(b->d_tabs, b->d_res, cnt, nb, nlev, capmax, st));
    const size_t ne = (size_t)cnt * b->stride();
    BHIP(b, hipMemcpyAsync(b->h_W, b->d_W, ne * sizeof(int), hipMemcpyDeviceToHost, st));
    BHIP(b, hipMemcpyAsync(b->h_fp, b->d_fp, ne * sizeof(int), hipMemcpyDeviceToHost, st));
    BHIP(b, hipMemcpyAsync(b->h_ft, b->d_ft, ne, hipMemcpyDeviceToHost, st));
    BHIP(b, hipMemcpyAsync(b->h_bo, b->d_bo, cnt * sizeof(BtOut), hipMemcpyDeviceToHost, st));
    BHIP(b, hipMemcpyAsync(b->h_err, b->d_err, cnt * sizeof(int), hipMemcpyDeviceToHost, st));
    BHIP(b, hipEventRecord(b->ev_res, st));
    b->pending = true;
    return CCJ_OK;
}

extern "C" int ccj_batch_wait(ccj_batch *b) {
    if (!b) return CCJ_E_ARG;
    if (!b->pending) return batch_err(b, CCJ_E_STATE, "ccj_batch_wait: no fold in flight");
    b->pending = false;
    BHIP(b, hipSetDevice(b->device));
    BHIP(b, hipEventSynchronize(b->ev_res));
    float ms = 0;
    BHIP(b, hipEventElapsedTime(&ms, b->fs.ev_start, b->fs.ev_end));
    b->fill_ms = ms;
    int rc = CCJ_OK;
    for (int k = 0; k < b->count; ++k) {
        ccj_ctx *c = b->m[k];
        const int herr = b->h_err[k];
        c->range_flags = 0;
        c->range_refused = false;
        if (herr & ~ERR_RANGE_MASK) {
            const int e = (herr & 1) ? set_err(c, CCJ_E_PARAMS, "e_intP table value outside int16 range (flags %d)", herr)
                                     : set_err(c, CCJ_E_HIP, "device bounds check failed (flags %d)", herr);
            if (rc == CCJ_OK) rc = batch_err(b, e, "member %d: %s", k, c->err.c_str());
            continue;
        }
        c->fill_ms = ms;
        c->W.assign(c->hr_W, c->hr_W + c->n + 1);
        c->bt_steps = c->hr_bo->steps;
        c->filled = true;
        c->res_ready = true;
        // a member outside the domain is its own affair, like a reference backtrack exit: the batch is
        // fine, its ccj_result returns CCJ_E_RANGE
        range_verdict(c, (herr & ERR_RANGE_MASK) >> ERR_RANGE_SHIFT);
    }
    return rc;
}

extern "C" double ccj_batch_fill_ms(const ccj_batch *b) { return b ? b->fill_ms : 0.0; }

extern "C" int ccj_batch_level_plan(const int *n, int count, int t, int split_target, int *out) {
    if (!n || !out || count < 1 || t < 0 || split_target < 0) return CCJ_E_ARG;
    for (int k = 0; k < count; ++k)
        if (n[k] < 1 || n[k] > 1023) return CCJ_E_ARG;
    std::vector<int> blocks(count), wpa(count);
    const BatchLevelPlan P = ccjk_batch_level_plan(n, count, t, split_target, blocks.data(), wpa.data());
    out[0] = P.split, out[1] = P.threads, out[2] = P.lds, out[3] = P.gridx;
    for (int k = 0; k < count; ++k) out[4 + 2 * k] = blocks[k], out[5 + 2 * k] = wpa[k];
    return CCJ_OK;
}
