// ccj_backtrack.hip — exterior W and the whole traceback on the GPU.
//
// The reference runs W (W_final.cc:68-79) and the traceback (W_final::backtrack :175-719,
// pseudo_loop::backtrack pseudo_loop.cc:861-2820) on the host over the filled matrices.  Doing it
// here removes the 2.9 GB device-to-host copy of the 4-D matrices (n=200) from every fold: only
// W, the pair list f[] and an exit record come back, and fill_structure (W_final.cc:764-819)
// stays on the host.
//
// The node logic (every case of the two backtrack functions) is ccj_traceback.h, shared with the
// host executor of ccj_host.cc.  This file holds the device executor only: the storage adaptor
// over device memory, the parallel scans, the LDS node stack and the driver loop.  One workgroup
// (CCJ_BT_WAVES waves, default 8) does the traceback.  Nodes are popped from the LDS stack in the
// reference's LIFO order; a scan's candidates are evaluated by the lanes, each a strided subset,
// and a lexicographic (value, position) reduction picks the first minimum, i.e. the reference's
// strict `<` in loop order (see DevExec::scan for how short and long scans are spread).
#include <hip/hip_runtime.h>

#include "ccj_backtrack.h"
#include "ccj_energy.h"
#include "ccj_engine.h"
#include "ccj_traceback.h"

using namespace ccj;

namespace {

// the filled matrices and small tables in device memory (the Store of ccj_traceback.h)
struct DevStore {
    const DevTables &T;
    int n, rs;
    const int *W;
    // the small tables every candidate reads (k_backtrack: copies in LDS; else T's)
    const short *S, *S1;
    const int8_t *pair, *rtype;
    const LvlDev *ld;

    // pair[S[i]][S[j]] of the binding's relation.  The table lookup behind the LDS copies is all an
    // unconstrained binding does (T.cons = 0, uniform); under a constraint a pair type is then checked
    // against the pt plane, which holds 0 at the constraint's pairs (either order of i, j; a position
    // outside 1..n is the reference's own S[0] / S[n+1] lookup and stays with the table)
    __device__ __forceinline__ int pr(int i, int j) const {
        int t = pair[S[i] * 8 + S[j]];
        if (T.cons && t > 0) {
            const int lo = imin(i, j), hi = imax(i, j);
            if (lo >= 1 && hi <= n && T.pt[(hi - lo) * rs + lo] == 0) t = 0;
        }
        return t;
    }
    __device__ __forceinline__ int rt(int type) const { return rtype[type]; }
    __device__ __forceinline__ const ccj_energy_params *prm() const { return T.prm; }
    __device__ __forceinline__ const int *lx() const { return T.lx; }
    __device__ __forceinline__ const Penalties &pen() const { return T.pen; }
    __device__ __forceinline__ int dangles() const { return T.dangles; }
    __device__ __forceinline__ double est() const { return T.e_stP; }
    __device__ __forceinline__ double eint() const { return T.e_intP; }
    __device__ __forceinline__ int raw2(int which, int i, int j) const {
        const int *A = which == A2_V ? T.V : which == A2_WM ? T.WM : which == A2_WMV ? T.WMv : which == A2_WMP ? T.WMp
                     : which == A2_P ? T.P : which == A2_WBP ? T.WBP : T.WPP;
        return A[(j - i) * rs + i];
    }
    __device__ __forceinline__ int Vtype(int i, int j) const { return T.Vt[(j - i) * rs + i]; }
    __device__ __forceinline__ int raw4(int x, int i, int j, int k, int l) const {
        const int t = (j - i) + (l - k), m = n - t - 2, h = k - j - 2, a = j - i;
        const LvlDev L = ld[t];
        return mat4_get(T, x, L, (long long)a * L.M + h * m - ((h * (h - 1)) >> 1) + i - 1, i, j, k, l);
    }
    // the P_P split key k_pterm keeps with the minimum (T.Pk)
    __device__ __forceinline__ unsigned pk(int i, int l) const { return (unsigned)(T.Pk[(l - i) * rs + i] & 0xffffffffull); }
};
using DV = View<DevStore>;

__device__ __forceinline__ int lane_id() { return (int)threadIdx.x; }

__device__ __forceinline__ void wreduce(int &v, int &x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int v2 = __shfl_xor(v, o), x2 = __shfl_xor(x, o);
        if (v2 < v || (v2 == v && x2 < x)) {
            v = v2;
            x = x2;
        }
    }
}

// The traceback workgroup has BT_MAXW waves at most.  Every wave walks the same nodes in lockstep
// (all control flow is uniform: it depends only on scan results, which every lane holds).  A scan
// of at most REPL_MAX candidates is evaluated by every wave redundantly (lane x: x, x+64, ...) and
// reduced inside the wave — no barrier; a longer one is spread over the whole workgroup (thread t:
// t, t+blockDim, ...) and the waves' partial minima meet in LDS.  Either way every lane ends with
// the lexicographic (value, position) minimum, i.e. the reference's first strict minimum.
constexpr int BT_MAXW = 16;
constexpr int BT_WAVES_DEFAULT = 8;
constexpr int REPL_MAX = 64;

__device__ __forceinline__ void block_reduce(int &v, int &x) {
    __shared__ int rv[BT_MAXW], rx[BT_MAXW];
    const int w = (int)(threadIdx.x >> 6), nw = (int)(blockDim.x >> 6);
    if ((threadIdx.x & 63) == 0) {
        rv[w] = v;
        rx[w] = x;
    }
    __syncthreads();
    for (int q = 0; q < nw; ++q) {
        const int v2 = rv[q], x2 = rx[q];
        if (v2 < v || (v2 == v && x2 < x)) {
            v = v2;
            x = x2;
        }
    }
    __syncthreads();  // rv/rx are reused by the next scan
}

// The device executor of ccj_traceback.h: scans over the workgroup, the LDS node stack, and pair
// writes by lane 0 (every lane holds the same uniform state otherwise).
struct DevExec {
    const DV &H;
    Interval *stk;
    int cap, sp;
    int *f_pair;
    int8_t *f_type;
    BtOut st;  // uniform

    // first minimum (value, position) over candidate positions [0, count) in loop order
    template <class F>
    __device__ __forceinline__ void scan(int count, F f, int &bv, int &bx) {
        int v = BIG, x = BIG;
        const bool spread = count > REPL_MAX && blockDim.x > 64;
        const int c0 = spread ? (int)threadIdx.x : (int)(threadIdx.x & 63), dc = spread ? (int)blockDim.x : 64;
        for (int c = c0; c < count; c += dc) {
            const int t = f(c);
            if (t < v) {
                v = t;
                x = c;
            }
        }
        wreduce(v, x);
        if (spread) block_reduce(v, x);
        bv = v;
        bx = x;
    }

    // One pass over candidates that yields both the first minimum (value, position) of f(c).x and
    // the minimum of f(c).y (the get_P?iloop hand-over of ccj_traceback.h)
    template <class F>
    __device__ __forceinline__ void scan2(int count, F f, int &fmin, int &bv, int &bx) {
        int v = BIG, x = BIG, fm = BIG, z = 0;
        const bool spread = count > REPL_MAX && blockDim.x > 64;
        const int c0 = spread ? (int)threadIdx.x : (int)(threadIdx.x & 63), dc = spread ? (int)blockDim.x : 64;
        for (int c = c0; c < count; c += dc) {
            const Int2 t = f(c);
            if (t.x < v) {
                v = t.x;
                x = c;
            }
            fm = imin(fm, t.y);
        }
        wreduce(v, x);
        wreduce(fm, z);
        if (spread) {
            block_reduce(v, x);
            block_reduce(fm, z);
        }
        fmin = fm;
        bv = v;
        bx = x;
    }

    __device__ __forceinline__ void push(int i, int j, int k, int l, int type) {
        if (sp >= cap) {
            st.status = BT_OVERFLOW;
            return;
        }
        if (lane_id() == 0) stk[sp] = Interval{i, j, k, l, type};
        ++sp;
    }
    __device__ __forceinline__ void setpair(int p, int q) {
        if (lane_id() == 0) {
            f_pair[p] = q;
            f_pair[q] = p;
        }
    }
    __device__ __forceinline__ void pairup(int p, int q, int type) {
        if (lane_id() == 0) {
            f_pair[p] = q;
            f_pair[q] = p;
            f_type[p] = (int8_t)type;
            f_type[q] = (int8_t)type;
        }
    }
};

// W_final.cc:68-79.  W[j] = min(W[j-1], min_k W[k-1] + S(k,j)) with
//   S(k,j) = min(E_ext_Stem(V(k..j) ...), min(P(k,j), P(k+1,j), P(k,j-1), P(k+1,j-1)) + PS),
// since the reference's two terms share the W[k-1] addend.  k_w_terms evaluates every S(k,j) in
// parallel; k_compute_W then runs the recurrence in one wave, j ascending, k over the lanes.
__device__ __forceinline__ void w_terms_body(const DevTables &T, int *S) {
    const int n = T.n;
    DV H{{T, n, T.rs, nullptr, T.S, T.S1, T.pair, T.rtype, T.ld}};
    const int j = blockIdx.y + TURN + 1;
    const int k = blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (j > n || k > j - TURN - 1) return;
    const int e2 = E_ext_Stem(H, H.V(k, j), H.V(k + 1, j), H.V(k, j - 1), H.V(k + 1, j - 1), k, j);
    const int e3 = imin(imin(H.Pg(k, j), H.Pg(k + 1, j)), imin(H.Pg(k, j - 1), H.Pg(k + 1, j - 1))) + T.pen.PS;
    S[(size_t)j * T.rs + k] = imin(e2, e3);
}
__global__ __launch_bounds__(256) void k_w_terms(DevTables T, int *S) { w_terms_body(T, S); }
// Lockstep batch (ccj_engine.h): one launch for every member, the member's tables and result
// pointers (BatchRes) read at a wave-uniform address; k_w_terms uses y, so the member is z.
__global__ __launch_bounds__(256) void k_w_terms_many(const DevTables *__restrict__ tabs, const BatchRes *__restrict__ res) {
    w_terms_body(tabs[blockIdx.z], res[blockIdx.z].S);
}

// The recurrence with W held in registers: W[x] lives in lane x % 64, slot x / 64 (Q slots cover
// 0..n), so a step is a register pass plus a wave reduction — no LDS, no barrier — and the S row
// of step j+1 is loaded while step j reduces, which hides the load latency behind the chain.
template <int Q>
__device__ __forceinline__ void compute_W_reg_body(const DevTables &T, const int *S, int *Wout) {
    const int n = T.n, lane = (int)threadIdx.x;
    int w[Q], s_cur[Q], s_nxt[Q];
    // S(k, j) for k = lane + 64q + 1, which adds to W[k-1] = w[q]; k runs 1 .. j-TURN-1
    auto load = [&](int j, int *s) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int k = lane + 64 * q + 1;
            s[q] = (j <= n && k <= j - TURN - 1) ? S[(size_t)j * T.rs + k] : BIG;
        }
    };
#pragma unroll
    for (int q = 0; q < Q; ++q) w[q] = 0;
    load(TURN + 1, s_cur);
    int wprev = 0;
    for (int j = TURN + 1; j <= n; ++j) {
        load(j + 1, s_nxt);
        int m = INF;
#pragma unroll
        for (int q = 0; q < Q; ++q)
            if (s_cur[q] != BIG) m = imin(m, w[q] + s_cur[q]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = imin(m, __shfl_xor(m, o));
        wprev = imin(wprev, m);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            if (lane + 64 * q == j) w[q] = wprev;
            s_cur[q] = s_nxt[q];
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q)
        if (lane + 64 * q <= n) Wout[lane + 64 * q] = w[q];
}
template <int Q>
__global__ __launch_bounds__(64) void k_compute_W_reg(DevTables T, const int *S, int *Wout) {
    compute_W_reg_body<Q>(T, S, Wout);
}
// one workgroup per member; Q covers the longest member (slots past a member's n stay unused)
template <int Q>
__global__ __launch_bounds__(64) void k_compute_W_reg_many(const DevTables *__restrict__ tabs, const BatchRes *__restrict__ res) {
    compute_W_reg_body<Q>(tabs[blockIdx.x], res[blockIdx.x].S, res[blockIdx.x].W);
}

__device__ __forceinline__ void compute_W_body(const DevTables &T, const int *S, int *Wout) {
    extern __shared__ int Ws[];
    const int n = T.n;
    for (int j = lane_id(); j <= n; j += 64) Ws[j] = 0;
    __syncthreads();
    for (int j = TURN + 1; j <= n; ++j) {
        const int *Sj = S + (size_t)j * T.rs;
        int m = INF;
        for (int k = 1 + lane_id(); k <= j - TURN - 1; k += 64) m = imin(m, ((k > 1) ? Ws[k - 1] : 0) + Sj[k]);
        int x = 0;
        wreduce(m, x);
        if (lane_id() == 0) Ws[j] = imin(Ws[j - 1], m);
        __syncthreads();
    }
    for (int j = lane_id(); j <= n; j += 64) Wout[j] = Ws[j];
}
__global__ __launch_bounds__(64) void k_compute_W(DevTables T, const int *S, int *Wout) { compute_W_body(T, S, Wout); }
__global__ __launch_bounds__(64) void k_compute_W_many(const DevTables *__restrict__ tabs, const BatchRes *__restrict__ res) {
    compute_W_body(tabs[blockIdx.x], res[blockIdx.x].S, res[blockIdx.x].W);
}


// one workgroup of 1..BT_MAXW waves; LDS: the node stack (cap entries)
__device__ __forceinline__ void backtrack_body(const DevTables &T, const int *W, int *f_pair, int8_t *f_type, BtOut *out, int cap,
                                               int lds_ld) {
    extern __shared__ Interval stk[];
    const int n = T.n;
    // LDS copies of the small tables behind every candidate's first loads (sequence, pair types,
    // level descriptors), placed after the node stack; the descriptors only when they fit (lds_ld)
    short *sS = (short *)(stk + cap), *sS1 = sS + (n + 2);
    int8_t *sPair = (int8_t *)(sS1 + (n + 2)), *sRt = sPair + 64;
    LvlDev *sLd = (LvlDev *)(((unsigned long long)(sRt + 8) + 15) & ~15ull);
    for (int x = (int)threadIdx.x; x < n + 2; x += (int)blockDim.x) {
        sS[x] = T.S[x];
        sS1[x] = T.S1[x];
    }
    for (int x = (int)threadIdx.x; x < 72; x += (int)blockDim.x) {
        if (x < 64) sPair[x] = T.pair[x];
        else sRt[x - 64] = T.rtype[x - 64];
    }
    if (lds_ld)
        for (int x = (int)threadIdx.x; x < T.nlev; x += (int)blockDim.x) sLd[x] = T.ld[x];
    DV H{{T, n, T.rs, W, sS, sS1, sPair, sRt, lds_ld ? sLd : T.ld}};
    for (int x = (int)threadIdx.x; x <= n; x += (int)blockDim.x) {
        f_pair[x] = -1;
        f_type[x] = (int8_t)T_NONE;
    }
    __syncthreads();  // the pair list is cleared before lane 0 starts writing pairs
    DevExec X{H, stk, cap, 0, f_pair, f_type, BtOut{}};
    Traceback<DevExec> B(X);
    X.push(1, n, 0, 0, FREE);  // W_final.cc:84-99
    __syncthreads();
    while (X.sp > 0 && X.st.status == BT_OK) {
        if (X.st.steps >= BT_MAX_STEPS) {  // uniform: every lane counts the same steps
            X.st.status = BT_STEPS;
            break;
        }
        const Interval cur = stk[X.sp - 1];
        __syncthreads();  // every lane has read the top before lane 0 overwrites it
        --X.sp;
        ++X.st.steps;
        B.node(cur);
        // a get_uc assert on any lane of any wave; the barrier also publishes lane 0's pushes
        if (__syncthreads_or(H.bad)) X.st.status = BT_ASSERT;
    }
    if (lane_id() == 0) *out = X.st;
}
__global__ __launch_bounds__(64 * BT_MAXW) void k_backtrack(DevTables T, const int *W, int *f_pair, int8_t *f_type, BtOut *out, int cap,
                                                            int lds_ld) {
    backtrack_body(T, W, f_pair, f_type, out, cap, lds_ld);
}
// one workgroup per member: its own stack capacity, inside LDS sized for the largest member
__global__ __launch_bounds__(64 * BT_MAXW) void k_backtrack_many(const DevTables *__restrict__ tabs, const BatchRes *__restrict__ res,
                                                                 int lds_ld) {
    const BatchRes &R = res[blockIdx.x];
    backtrack_body(tabs[blockIdx.x], R.W, R.f_pair, R.f_type, R.out, R.cap, lds_ld);
}

}  // namespace

extern "C" int ccjk_compute_W(const void *Tv, int *W, int *S, void *stream) {
    const DevTables *T = (const DevTables *)Tv;
    const int n = T->n;
    if (n > TURN) {
        hipLaunchKernelGGL(k_w_terms, dim3((unsigned)((n + 255) / 256), (unsigned)(n - TURN)), dim3(256), 0,
                           (hipStream_t)stream, *T, S);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    const hipStream_t s = (hipStream_t)stream;
    switch ((n + 64) / 64) {  // slots for W[0..n]
        case 1: hipLaunchKernelGGL(k_compute_W_reg<1>, dim3(1), dim3(64), 0, s, *T, S, W); break;
        case 2: hipLaunchKernelGGL(k_compute_W_reg<2>, dim3(1), dim3(64), 0, s, *T, S, W); break;
        case 3: hipLaunchKernelGGL(k_compute_W_reg<3>, dim3(1), dim3(64), 0, s, *T, S, W); break;
        case 4: hipLaunchKernelGGL(k_compute_W_reg<4>, dim3(1), dim3(64), 0, s, *T, S, W); break;
        case 5: hipLaunchKernelGGL(k_compute_W_reg<5>, dim3(1), dim3(64), 0, s, *T, S, W); break;
        case 6: hipLaunchKernelGGL(k_compute_W_reg<6>, dim3(1), dim3(64), 0, s, *T, S, W); break;
        case 7: hipLaunchKernelGGL(k_compute_W_reg<7>, dim3(1), dim3(64), 0, s, *T, S, W); break;
        case 8: hipLaunchKernelGGL(k_compute_W_reg<8>, dim3(1), dim3(64), 0, s, *T, S, W); break;
        default: hipLaunchKernelGGL(k_compute_W, dim3(1), dim3(64), (n + 1) * sizeof(int), s, *T, S, W);
    }
    return (int)hipGetLastError();
}

static int bt_waves() {
    static const int waves = [] {
        const char *e = getenv("CCJ_BT_WAVES");
        const int w = e ? atoi(e) : BT_WAVES_DEFAULT;
        return w < 1 ? 1 : (w > BT_MAXW ? BT_MAXW : w);
    }();
    return waves;
}

extern "C" int ccjk_backtrack(const void *Tv, const int *W, int *f_pair, int8_t *f_type, BtOut *out, int stack_cap,
                              void *stream) {
    const DevTables *T = (const DevTables *)Tv;
    const int waves = bt_waves();
    // dynamic LDS: the node stack, then the small tables (k_backtrack); the level descriptors too
    // while the whole stays within 64 KB
    const size_t base = (size_t)stack_cap * sizeof(Interval) + 4 * ((size_t)T->n + 2) + 72 + 16;
    const size_t with_ld = base + (size_t)T->nlev * sizeof(LvlDev);
    const int lds_ld = with_ld <= 65536 ? 1 : 0;
    hipLaunchKernelGGL(k_backtrack, dim3(1), dim3(64 * waves), lds_ld ? with_ld : base, (hipStream_t)stream, *T, W, f_pair,
                       f_type, out, stack_cap, lds_ld);
    return (int)hipGetLastError();
}

// Lockstep batch: W and the traceback of `count` members, one workgroup each (nmax / nlevmax / capmax:
// the largest member's length, level count and stack capacity; they size the uniform LDS).
extern "C" int ccjk_compute_W_many(const void *tabs_v, const BatchRes *res, int count, int nmax, void *stream) {
    const DevTables *tabs = (const DevTables *)tabs_v;
    const hipStream_t s = (hipStream_t)stream;
    if (count <= 0) return 0;
    if (nmax > TURN) {
        hipLaunchKernelGGL(k_w_terms_many, dim3((unsigned)((nmax + 255) / 256), (unsigned)(nmax - TURN), (unsigned)count), dim3(256), 0,
                           s, tabs, res);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    const dim3 g((unsigned)count), b(64);
    switch ((nmax + 64) / 64) {  // slots for W[0..nmax]
        case 1: hipLaunchKernelGGL(k_compute_W_reg_many<1>, g, b, 0, s, tabs, res); break;
        case 2: hipLaunchKernelGGL(k_compute_W_reg_many<2>, g, b, 0, s, tabs, res); break;
        case 3: hipLaunchKernelGGL(k_compute_W_reg_many<3>, g, b, 0, s, tabs, res); break;
        case 4: hipLaunchKernelGGL(k_compute_W_reg_many<4>, g, b, 0, s, tabs, res); break;
        case 5: hipLaunchKernelGGL(k_compute_W_reg_many<5>, g, b, 0, s, tabs, res); break;
        case 6: hipLaunchKernelGGL(k_compute_W_reg_many<6>, g, b, 0, s, tabs, res); break;
        case 7: hipLaunchKernelGGL(k_compute_W_reg_many<7>, g, b, 0, s, tabs, res); break;
        case 8: hipLaunchKernelGGL(k_compute_W_reg_many<8>, g, b, 0, s, tabs, res); break;
        default: hipLaunchKernelGGL(k_compute_W_many, g, b, (nmax + 1) * sizeof(int), s, tabs, res);
    }
    return (int)hipGetLastError();
}

extern "C" int ccjk_backtrack_many(const void *tabs_v, const BatchRes *res, int count, int nmax, int nlevmax, int capmax,
                                   void *stream) {
    if (count <= 0) return 0;
    const size_t base = (size_t)capmax * sizeof(Interval) + 4 * ((size_t)nmax + 2) + 72 + 16;
    const size_t with_ld = base + (size_t)nlevmax * sizeof(LvlDev);
    const int lds_ld = with_ld <= 65536 ? 1 : 0;
    hipLaunchKernelGGL(k_backtrack_many, dim3((unsigned)count), dim3(64 * bt_waves()), lds_ld ? with_ld : base, (hipStream_t)stream,
                       (const DevTables *)tabs_v, res, lds_ld);
    return (int)hipGetLastError();
}
