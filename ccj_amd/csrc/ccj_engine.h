// ccj_engine.h — internal data layout shared by the HIP kernels and the host engine.
//
// HBM layout:
//   * 4-D gap matrices: level-major.  A cell (i,j,k,l) has a = j-i, g = k-j (>= 2), b = l-k,
//     level t = a+b, h = g-2.  Level t holds (t+1) blocks (one per a) of M_t = m_t(m_t+1)/2 cells,
//     m_t = n-t-2, each block a triangle of rows h = 0..m_t-1 of length m_t-h, i fastest.
//     Within a level the matrix slots (mslot below: 6 in a lean context, all 22 in a full one) are
//     stored one after another (SoA), so one level is one contiguous span:
//     elem(x,t,a,h,i) = LB_t + mslot(x)*C_t + a*M_t + G_t(h) + (i-1),
//     G_t(h) = h*m_t - h(h-1)/2, C_t = (t+1)*M_t.
//     Every dependency of a level-t cell lies in levels < t, and lanes of one
//     wave (same t, a) read shifted neighbours whose offsets differ by a lane-uniform amount,
//     so reads and writes are coalesced along i.
//   * 2-D interval arrays: span-major [w][p] (w = j-i, p = i), row stride n+2, so a wave
//     reading (i, i+w) for consecutive i touches consecutive words.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "ccj_energy.h"  // Mat4, Penalties
#include "ccj_mloop2d.h"  // the six table-carried matrices
#include "ccj_pmpo2d.h"   // the six closed-form matrices
#include "ccj_params.h"

namespace ccj {

// Every 4-D matrix has exactly one carrier, the place the fill writes it to and every reader takes it
// from:
//   IN_D4  (6): its slot of d4.  The level kernel stores it and later levels read it there.
//   IN_REC (4): the loop records (RA / RK / RL below; rec_get).  A full context (DevTables::full4:
//               band-sharded over an exchange, which packs them from d4, or a host mirror streamed
//               during the fill) stores them in d4 as well and reads them there.
//   IN_TAB (6): the 2-D tables of the PL / PR multiloop families (ccj_mloop2d.h; tab_get).  The fill
//               never writes their d4 slots.
//   IN_CF  (6): the PM / PO multiloop families, evaluated in closed form from nine 2-D tables
//               (ccj_pmpo2d.h; cf_get).  The fill never computes them for a cell's own sake and
//               never writes their d4 slots.
enum Carrier { IN_D4 = 0, IN_REC = 1, IN_TAB = 2, IN_CF = 3 };
constexpr unsigned REC_MASK = (1u << PfromL) | (1u << PfromR) | (1u << PfromMprime) | (1u << PfromO);
constexpr unsigned D4_MASK = ((1u << NMAT4) - 1u) & ~(REC_MASK | TAB_MASK | CF_MASK);
static_assert((REC_MASK & TAB_MASK) == 0 && (REC_MASK & CF_MASK) == 0 && (TAB_MASK & CF_MASK) == 0, "one carrier per matrix");
__host__ __device__ constexpr Carrier carrier(int x) {
    return (TAB_MASK >> x) & 1u ? IN_TAB : (CF_MASK >> x) & 1u ? IN_CF : (REC_MASK >> x) & 1u ? IN_REC : IN_D4;
}
constexpr int NMAT_D4 = __builtin_popcount(D4_MASK), NMAT_REC = __builtin_popcount(REC_MASK), NMAT_TAB = __builtin_popcount(TAB_MASK),
              NMAT_CF = __builtin_popcount(CF_MASK);
// Storage slot of matrix x inside a level of d4 and of the host mirror: the IN_D4 matrices in enum
// order, then IN_REC, then IN_TAB, then IN_CF (the two classes the fill never writes come last, so one
// ccjk_expand from slot NMAT_D4 + NMAT_REC covers both).  d4 holds slots [0, NMAT_D4) per level, or all
// 22 in a full context; the host mirror always holds 22 (ccjk_expand writes out what d4 lacks).
// Matrix-major "level element" indices of the exchange API (x*C + a*M + c) are by matrix, not by slot.
__host__ __device__ constexpr int mslot(int x) {
    const Carrier c = carrier(x);
    const unsigned cls = c == IN_D4 ? D4_MASK : c == IN_REC ? REC_MASK : c == IN_TAB ? TAB_MASK : CF_MASK;
    const int first = c == IN_D4 ? 0 : c == IN_REC ? NMAT_D4 : c == IN_TAB ? NMAT_D4 + NMAT_REC : NMAT_D4 + NMAT_REC + NMAT_TAB;
    return first + __builtin_popcount(cls & ((1u << x) - 1u));
}
static_assert(NMAT_D4 == 6 && NMAT_REC == 4 && NMAT_TAB == 6 && NMAT_CF == 6 && NMAT_D4 + NMAT_REC + NMAT_TAB + NMAT_CF == NMAT4,
              "the partition");
static_assert(carrier(PK) == IN_D4 && mslot(PK) == 0 && mslot(PO) == 4 && carrier(PfromM) == IN_D4 && mslot(PfromM) == NMAT_D4 - 1,
              "d4 slots");
static_assert(carrier(PfromL) == IN_REC && mslot(PfromL) == NMAT_D4 && carrier(PfromO) == IN_REC &&
                  mslot(PfromO) == NMAT_D4 + NMAT_REC - 1,
              "record-carried slots");
static_assert(carrier(PLmloop00) == IN_TAB && mslot(PLmloop00) == NMAT_D4 + NMAT_REC && carrier(PRmloop10) == IN_TAB &&
                  mslot(PRmloop10) == NMAT_D4 + NMAT_REC + NMAT_TAB - 1,
              "table-carried slots");
static_assert(carrier(PMmloop00) == IN_CF && mslot(PMmloop00) == NMAT4 - NMAT_CF && carrier(POmloop10) == IN_CF &&
                  mslot(POmloop10) == NMAT4 - 1,
              "closed-form slots");

// The device error word (DevTables::err).  Bits 1 .. 512 are the parameter and bounds checks; the
// bits from ERR_RANGE_SHIFT on are the range sites: a 4-D value below -32768 was about
// to be narrowed to int16, where the reference's store wraps.  (err >> ERR_RANGE_SHIFT) & 31 is what
// ccj_range_flags reports (include/ccj.h CCJ_RANGE_*).
constexpr int ERR_RANGE_SHIFT = 10;
constexpr int ERR_RANGE_LEVEL = 1 << ERR_RANGE_SHIFT, ERR_RANGE_ILOOP = 2 << ERR_RANGE_SHIFT,
              ERR_RANGE_PARTIAL = 4 << ERR_RANGE_SHIFT, ERR_RANGE_TAB = 8 << ERR_RANGE_SHIFT, ERR_RANGE_CF = 16 << ERR_RANGE_SHIFT;
constexpr int ERR_RANGE_MASK = 31 << ERR_RANGE_SHIFT;
constexpr int LOW16 = -32768;  // the lowest value an int16 store keeps

constexpr int IE_U = 29;  // u1,u2 in [0,28] for pseudoknot interior loops (pseudo_loop.cc:694-806)
#ifndef CCJ_ILB
#define CCJ_ILB 8
#endif
constexpr int IL_B = CCJ_ILB;  // interior-loop candidates per load batch (k_iloop)
constexpr int IL_CAP = (IE_U * IE_U + IL_B + 7) / 8 * 8;  // candidate-list capacity per pair (+ IL_B null tail)
constexpr int IL_SEG = 64;   // per pair: seg[dt] = first list entry of source-level distance dt

// k_ppush: spans per wave, i.e. consecutive partner levels a wave reads through one buffer resource
constexpr int PPUSH_S = 8;

struct LevelDesc {
    int16_t *base;  // first element of level t (matrix 0)
    int C;          // cells per matrix in this level
    int M;          // cells per a-block
    int m;          // n - t - 2 (rows per a-block)
    int pad;
};

struct LvlDev {     // per-level descriptor read by the level kernel (one s_load_dwordx8)
    long long lb;  // element offset of level t in the 4-D storage
    long long lr;  // record offset of level t in each of the three loop-record arrays (cells of the levels below)
    int C;         // cells per matrix in level t = (t+1)*M
    int M;         // cells per a-block = m(m+1)/2, m = n-t-2
    int pad[2];
};

// AoS loop records: the operands the fused split-point loops of k_level4d read at
// one neighbour cell, int16 fields packed in one record, so each neighbour costs one dwordx2 (dword)
// load instead of 2-4 int16 loads.  Three record types, each its own array indexed like a matrix
// (ld[t].lr + a*M + G(h) + i-1): 20 bytes per cell
//   RA (a-loop, both sides; T.rec, 8 B): PfromL PfromO | PfromMprime PK
//   RK (b-loop, k side;     T.rk,  8 B): PfromR min(PL,PR) | PK -
//   RL (b-loop, l side;     T.rl,  4 B): PfromR PfromO
// Values are the stored (clamped) int16 matrix values.  (The multiloop families are not in the records:
// PL / PR are 2-D tables, ccj_mloop2d.h; PM / PO closed forms of 2-D tables, ccj_pmpo2d.h.)
typedef uint2 rec_t;     // RA
typedef uint2 rk_t;      // RK
typedef unsigned rl_t;   // RL
static_assert(sizeof(rec_t) == 8 && sizeof(rk_t) == 8 && sizeof(rl_t) == 4, "record sizes");
constexpr int REC_BYTES = (int)(sizeof(rec_t) + sizeof(rk_t) + sizeof(rl_t));  // per cell

// Split-point sharing (k_level4d).  The cells of one gap column — same (j,k,l)
// for the i-side split, (i,k,l) j-side, (i,j,l) k-side, (i,j,k) l-side — sit on consecutive levels
// and read the same neighbours over the same split range, shifted by one split point per level.
// A leader cell (a % SHARE_R == 0 for the a-loop, b % SHARE_R == 0 for the b-loop) scans its whole
// range once and also reduces it for the next SHARE_R-1 cells of each of its columns; those
// followers scan only the split points the leader did not see and take the rest from a partial
// record.  Partial records live in a ring of SHARE_R level slots (the level t' cells' records are
// written at levels t'-SHARE_R+1 .. t'-1 and read at t'), SHARE_NACC 8-byte slots per cell, of which
// a record uses its first 4 / 8 / 8 / 4 bytes:
//   AI (i side, 4 B): PfromL PfromO
//   AJ (j side, 8 B): PfromL PfromMprime | PK -
//   AK (k side, 8 B): PfromR PfromM'' | PK -
//   AL (l side, 4 B): PfromR PfromO
// Values are min-clamped at 32767 like a store (clamp commutes with min).  The leader's W(i-r, .) / W(., j+r) operands are read
// from the span-major WP plane (span s-1+r, coalesced along the lanes).
#ifndef CCJ_SHARE_R
#define CCJ_SHARE_R 4
#endif
constexpr int SHARE_R = CCJ_SHARE_R;
constexpr int SHARE_NACC = 4;
// ring slots (one per target level): the leader launch of level t reads slot t (its follower
// sides) and writes slots t+1 .. t+SHARE_R-1, after level t's plain launch on the same stream
constexpr int SHARE_SLOTS = SHARE_R;
enum AccRec { AI = 0, AJ = 1, AK = 2, AL = 3 };

// The sharing role of one side of a cell, written once for level4d_body, the host's leader lists
// and ccj_share_roles.  len is the side's own gap (a for the a-loop, b for the b-loop), oth the
// other gap, t = len + oth the level, grp whether level t shares.
//   role 0: the cell scans its whole range 1..len;  1: leader, scans 1..len for itself and its
//   followers;  2: follower r = len % SHARE_R of the leader at level t-r, gap len-r.
// The cell itself scans the split points 1..low and len-top+1..len.  A leader's term for follower r
// at split point s reads a W operand of span s+r-1, which k_diag2d has finished before level t only
// for s <= len+oth-r: the leader leaves the top share_cut(r, oth) = max(0, r-oth) split points out of
// that follower's partial (the points 1..len-cut are in it), and the follower scans them itself at
// its own level, where they are its top min(cut, len-r) points.  (The cut cannot be one smaller
// because the last point is masked anyway: for cut = 2 the point below the last is not available
// either.)  edges = 0 keeps the rule this replaced: a column whose other gap is below SHARE_R-1
// does not share at all (CCJ_SHARE_EDGES=0, A/B runs).  A follower whose leader would lie below
// g_lo has none and scans in full.
struct ShareRole {
    int role, low, top;
};
__host__ __device__ __forceinline__ int share_cut(int r, int oth) { return r > oth ? r - oth : 0; }
__host__ __device__ __forceinline__ ShareRole share_role(bool grp, int edges, int len, int oth, int g_lo) {
    const int r = len % SHARE_R;
    if (!grp || (!edges && oth < SHARE_R - 1)) return ShareRole{0, len, 0};
    if (r == 0) return ShareRole{1, len, 0};
    if (len + oth - r < g_lo) return ShareRole{0, len, 0};
    const int cut = share_cut(r, oth);
    return ShareRole{2, r, cut < len - r ? cut : len - r};
}

// Band sharding: a-block a of every level belongs to rank (a / SHARD_GRP) % world,
// the same rank on every level, so a split-sharing leader (a % SHARE_R == 0) and its followers
// (a+1 .. a+SHARE_R-1, later levels) always live on one rank.  A rank's blocks are numbered by
// their "own index" o = 0, 1, ...: a = shard_a(o) ascending.  world = 1: a = o.
constexpr int SHARD_GRP = SHARE_R;
__host__ __device__ __forceinline__ int shard_owner(int a, int G) { return (a / SHARD_GRP) % G; }
__host__ __device__ __forceinline__ int shard_a(int o, int G, int r) {
    return ((o / SHARD_GRP) * G + r) * SHARD_GRP + o % SHARD_GRP;
}
// number of a in [0, x] owned by rank r (x >= -1)
__host__ __device__ __forceinline__ int shard_count(int x, int G, int r) {
    const int nb = x + 1, qf = nb / SHARD_GRP, rem = nb % SHARD_GRP;
    const int full = qf / G + (qf % G > r ? 1 : 0);
    return full * SHARD_GRP + (qf % G == r ? rem : 0);
}
// own index of the first a >= x owned by rank r
__host__ __device__ __forceinline__ int shard_ceil(int x, int G, int r) {
    if (x < 0) x = 0;
    int q = x / SHARD_GRP, off = x % SHARD_GRP;
    if (q % G != r) {
        q += ((r - q % G) + G) % G;
        off = 0;
    }
    return (q / G) * SHARD_GRP + off;
}

// The band-sharded exchange of level t has two parts, each ONE all-gather of equal
// slices:
//   part XCH_EDGE: the rank's blocks with a % SHARD_GRP == SHARD_GRP-1 (own index o % SHARD_GRP ==
//     SHARD_GRP-1): of level t, another rank's level t+1 reads only these (its group's first block a
//     reads block a-1 at split step 1, pseudo_loop.cc:357-362); then the tail: the P tail (XCH_PTAIL:
//     this rank's partials of P(t+1), pushed after level t-2) and the span tail (XCH_DTAIL: span t,
//     which level t+1 reads).  Gathered on the level stream: the critical path.
//   part XCH_BULK: the rank's other blocks (read from level t+2 on, and by k_iloop(t+3) / k_ppush(t)),
//     no tail.  Gathered on a side stream while level t+1 runs.
// The partials of P(n-1) (pushed after level n-4; no level n-2 carries them) travel alone after the
// last level, as a slice of one P tail.
// A part's slice: body [matrix x][part index k][cell c] of nmax blocks per matrix (nmax = the largest
// rank's block count of that part at t), padded to 8 bytes, then the part's tail.  k_pack / k_unpack /
// k_?tail_* and the host's buffer sizing use these; ccj_exchange_layout / ccj_exchange_index export
// them (tests).
constexpr int XCH_EDGE = 0, XCH_BULK = 1;
constexpr int XCH_DT_N = 10;  // span tail planes: V, Vt, P, WBP, WB, WPP, WP, WMv, WMp, WM
__host__ __device__ __forceinline__ long long xch_body(int nmax, int M) { return ((long long)22 * nmax * M + 3) & ~3LL; }
__host__ __device__ __forceinline__ long long xch_ptail(int n) { return 4LL * (n + 1); }
__host__ __device__ __forceinline__ long long xch_dtail(int n) { return 2LL * XCH_DT_N * (n + 1); }
__host__ __device__ __forceinline__ long long xch_tail(int n, int part) { return part == XCH_EDGE ? xch_ptail(n) + xch_dtail(n) : 0; }
__host__ __device__ __forceinline__ long long xch_slice(int n, int nmax, int M, int part) { return xch_body(nmax, M) + xch_tail(n, part); }
// part of own index o, its index inside the part, and back
__host__ __device__ __forceinline__ int xch_part(int o) { return o % SHARD_GRP == SHARD_GRP - 1 ? XCH_EDGE : XCH_BULK; }
__host__ __device__ __forceinline__ int xch_pidx(int o) {
    return xch_part(o) == XCH_EDGE ? o / SHARD_GRP : (o / SHARD_GRP) * (SHARD_GRP - 1) + o % SHARD_GRP;
}
__host__ __device__ __forceinline__ int xch_own(int k, int part) {
    return part == XCH_EDGE ? k * SHARD_GRP + SHARD_GRP - 1 : (k / (SHARD_GRP - 1)) * SHARD_GRP + k % (SHARD_GRP - 1);
}
// rank r's blocks of the part at level t (own indices 0 .. shard_count(t)-1)
__host__ __device__ __forceinline__ int xch_pcount(int t, int G, int r, int part) {
    const int own = shard_count(t, G, r);
    return part == XCH_EDGE ? own / SHARD_GRP : own - own / SHARD_GRP;
}
// body position of matrix x, part index k, cell c
__host__ __device__ __forceinline__ long long xch_pos(int x, int k, int c, int nmax, int M) {
    return ((long long)x * nmax + k) * M + c;
}
// where block a's cells arrive: its owner's slice of the block's part, at the block's part index
__host__ __device__ __forceinline__ void xch_src(int a, int G, int &owner, int &part, int &k) {
    owner = shard_owner(a, G);
    const int o = shard_count(a - 1, G, owner);
    part = xch_part(o);
    k = xch_pidx(o);
}
// the largest rank's block count of the part at level t
__host__ __device__ __forceinline__ int xch_nmax(int t, int G, int part) {
    int nm = 0;
    for (int r = 0; r < G; ++r) nm = xch_pcount(t, G, r, part) > nm ? xch_pcount(t, G, r, part) : nm;
    return nm;
}

struct LvlX {        // per-level bases of the interior-loop copies
    long long lbx;  // element offset of level t in d4x: PLx (C_t elements) then PRx (C_t)
    long long pmb;  // element offset of level t in pmx: m_t * n * (t+1) elements
};

struct DevTables {
    int n;
    int nlev;                      // levels that hold cells (t <= n-3)
    int rs;                        // 2-D row stride (n+2)
    int dangles;
    Penalties pen;
    double e_stP, e_intP;
    const ccj_energy_params *prm;  // device copy of the blob
    const int *lx;                 // (int)(lxc*log(x/30.)), x in [0, 2n+64)
    const short *S, *S1;           // encoded sequence, n+2
    const int8_t *pt;              // [w][p] pair type pair[S[p]][S[p+w]], 0 where a constraint forbids (p, p+w): the binding's relation
    const int8_t *pair;            // 8x8 pair table (after noGU)
    const int8_t *rtype;           // 8
    const int *hp;                 // [w][p] HairpinE (s_energy_matrix.cc:275-282), INF if type 0
    const int16_t *est;            // [w][p] e_stP, saturated at 32767
    int16_t *ie;                   // [w][p] e_intP of the u1 = u2 = 0 interior loop (k_precompute_ie), 32767 where skipped
    int *V; int8_t *Vt; int *WM, *WMv, *WMp, *P, *WBP, *WPP, *WB, *WP;  // [w][p]
    int2 *WBW;                     // [w][p] (WBP, WP) in one word pair (k_diag2d's table workgroups read .x)
    unsigned long long *Pk;        // [w][p] (P + 2^31) << 32 | first (j,d,k) split of the minimum (k_pterm)
    const LevelDesc *lv;           // per level t
    int16_t *d4;                   // 4-D storage base
    const long long *lb;           // element offset of level t in d4
    const LvlDev *ld;             // per-level descriptors
    rec_t *rec;                    // RA loop records: level t at ld[t].lr
    long long nrec;                // records allocated per array (debug bounds checks)
    rk_t *rk;                      // RK records, indexed like rec
    rl_t *rl;                      // RL records, indexed like rec
    // the PL / PR multiloop families (ccj_mloop2d.h): six int16 tables [w][p], row stride rs, one
    // after another (tab_index) tabN elements apart; span w is written by k_diag2d(w)
    int16_t *tab;
    long long tabN;
    // the PM / PO multiloop families (ccj_pmpo2d.h): NCF int32 tables [w][p] (CfTab), tabN elements
    // apart; span w is written by k_diag2d(w)
    int *cf;
    // interior-loop copies of PL / PR / PM, laid out so that the lanes of one k_iloop wave share
    // the loop's closing pair:
    //   PLx(t,a,h,i) = lbx + a*M + G(i-1) + h               (h fastest: fixed (i,j), lanes k)
    //   PRx(t,a,h,i) = lbx + C + a*M + q(q+1)/2 + i-1       (q = i+h-1: fixed (k,l), lanes i)
    //   PMx(t,a,h,i) = pmb + (h*n + j-1)*(t+1) + a          (j = i+a: fixed (j,k), lanes a)
    int16_t *d4x, *pmx;
    long long nx, npm;             // elements of d4x / pmx (debug bounds checks)
    const LvlX *ldx;
    // interior-loop candidate lists (k_build_il): per pair [w][p], the (u1,u2) whose inner pair can
    // pair, ordered by dt = 2+u1+u2 then u1; entry .x = dt << 21 | u1 << 16 | (uint16)energy,
    // .y = 2*u1*dt (the address cross term); IL_B null entries (dt 63) follow the last one.  Entries
    // dominated through a stacked pair are left out (ccj_ilprune.h; CCJ_IL_PRUNE=0 keeps them)
    uint2 *il, *ilm;               // il: pair (p,p+w) closes the loop (PL, PR); ilm: pair encloses (PM)
    int16_t *dummy;                // n+64 values 32767: target of the null entries
    const uint32_t *items;         // k_iloop work items (role << 30 | f1 << 20 | f2 << 10 | chunk)
    int full4;                     // 1: a full context, d4 has all 22 slots per level (mslot); 0: the NMAT_D4 first
    uint32_t *ilseg, *ilmseg;      // [pair][IL_SEG]; word 0 (no dt < 2 exists): the entry count before pruning
    int *err;                      // device error word
    // split-point sharing (above): levels [g_lo, g_hi) share; partial-record ring of SHARE_R
    // slots x SHARE_NACC x accC
    int split_target;              // k_level4d: narrow levels split loops so ~this many waves run (0: never)
    long long xpad;                // 32767 sentinel elements in front of every level's PLx/PRx and PMx (k_iloop's null target)
    long long xspan;               // bytes k_iloop may address from a wave's buffer base (debug check)
    int g_lo, g_hi;
    int share_edges;               // 1: columns with a short other gap share too (share_role; CCJ_SHARE_EDGES=0: 0)
    int cons;                      // 1: the binding carries a constraint (pt holds 0 at its pairs; the traceback's pr)
    // k_level4d_lead walks only the long-scan a-blocks of a sharing level, longest scan first:
    // rank r's list lord[lord_off[t*G+r] .. lord_off[t*G+r+1]) (device), lord_off_h = the same
    // offsets on the host
    const int16_t *lord;
    const int *lord_off;
    const int *lord_off_h;
    uint2 *acc;
    long long accC;
};

__device__ __forceinline__ int rlo16(unsigned w) { return (int)(int16_t)(w & 0xffffu); }
__device__ __forceinline__ int rhi16(unsigned w) { return (int)(int16_t)(w >> 16); }
// an IN_REC matrix from the records of the cell at in-level offset cell (a*M + G(h) + i-1)
__device__ __forceinline__ int rec_get(const DevTables &T, int x, const LvlDev &L, long long cell) {
    if (x == PfromR) return rlo16(T.rl[L.lr + cell]);  // RL: fR|fO
    const rec_t r = T.rec[L.lr + cell];  // RA: fL|fO, fMp|K
    switch (x) {
        case PfromL: return rlo16(r.x);
        case PfromO: return rhi16(r.x);
        default: return rlo16(r.y);  // PfromMprime
    }
}
// an IN_TAB matrix at cell (i,j,k,l)
__device__ __forceinline__ int tab_get(const DevTables &T, int x, int i, int j, int k, int l) {
    const int ti = tab_index(x);
    const int w = ti < 3 ? j - i : l - k, p = ti < 3 ? i : k;
    return (int)T.tab[(long long)ti * T.tabN + w * T.rs + p];
}

// an IN_CF matrix at cell (i,j,k,l): the closed form over the nine tables
struct CfTabs {
    const int *cf;
    long long N;
    int rs;
    __device__ __forceinline__ int operator()(int f, int p, int q) const { return cf[(long long)f * N + (q - p) * rs + p]; }
};
__device__ __forceinline__ int cf_get(const DevTables &T, int x, int i, int j, int k, int l) {
    return pmpo2d_eval(x, T.pen.bp, T.pen.cp, CfTabs{T.cf, T.tabN, T.rs}, i, j, k, l);
}

// The one read of matrix x at cell (i,j,k,l) of level L outside the fill's own hot loops (hashes,
// traceback, host mirror): by carrier; cell = a*M + G(h) + i-1.
__device__ __forceinline__ int mat4_get(const DevTables &T, int x, const LvlDev &L, long long cell, int i, int j, int k, int l) {
    if (carrier(x) == IN_TAB) return tab_get(T, x, i, j, k, l);
    if (carrier(x) == IN_CF) return cf_get(T, x, i, j, k, l);
    if (carrier(x) == IN_REC && !T.full4) return rec_get(T, x, L, cell);
    return (int)T.d4[L.lb + (long long)mslot(x) * L.C + cell];
}

// Row h of in-block cell c (0 <= c < m(m+1)/2) of a level with m rows: the largest h with
// G(h) = h*m - h(h-1)/2 <= c.  Gh = G(h), so the cell's i is c - Gh + 1.
__device__ __forceinline__ int cell_row(int c, int m, int &Gh) {
    const float tm = 2.0f * m + 1.0f;
    int h = (int)((tm - sqrtf(tm * tm - 8.0f * (float)c)) * 0.5f);
    h = imax(0, imin(h, m - 1));
    while (h > 0 && h * m - ((h * (h - 1)) >> 1) > c) --h;
    while (h + 1 < m && (h + 1) * m - (((h + 1) * h) >> 1) <= c) ++h;
    Gh = h * m - ((h * (h - 1)) >> 1);
    return h;
}

// element offset of cell (a,h,i) of matrix x inside level t of the host mirror (relative to lv_offh[t])
inline int64_t cell_offset_host(const LevelDesc &L, int x, int a, int h, int i) {
    return (int64_t)mslot(x) * L.C + (int64_t)a * L.M + (int64_t)h * L.m - (int64_t)h * (h - 1) / 2 + (i - 1);
}

// ---- the level schedule: which launch regime level t runs in (host only) ----
// create_impl, ccjk_level4d and ccjk_level4d_lead all take it from here; ccj_level_schedule /
// ccj_ctx_level_schedule (include/ccj.h) export it.

// narrow levels: split each chunk's a/b loops over up to 8 waves so ~split_target waves run at once
// the split that brings `waves` one-wave chunks to about split_target waves (also what a lockstep
// batch's level launch takes for the waves of all its members, below)
inline int sched_split_of(long waves, int split_target) {
    int split = 1;
    while (split_target > 0 && split < 8 && waves * split * 2 <= split_target) split *= 2;
    return split;
}
inline int sched_level_split(int n, int t, int nblk, int split_target) {
    const int m = n - t - 2;
    if (m <= 0 || nblk <= 0) return 1;
    return sched_split_of((long)nblk * ((m * (m + 1) / 2 + 63) / 64), split_target);
}

// The sharing range [g_lo, g_hi): from the first level that runs unsplit (by the whole level's
// block count, whatever the world) to the last level; empty (0, 0) with sharing off or when every
// level splits.  The narrow early levels keep their split loops (short scans); on the narrow late
// levels k_level4d_lead splits the long scans like the level heuristic would.  (Sharing on the
// unsplit middle levels only measured 0.6 ms slower at n=200.)
inline void sched_share_range(int n, int split_target, bool share, int &g_lo, int &g_hi) {
    g_lo = g_hi = 0;
    if (!share) return;
    const int nlev = n > 2 ? n - 2 : 0;
    for (int t = 0; t < nlev; ++t)
        if (sched_level_split(n, t, t + 1, split_target) == 1) {
            g_lo = t;
            g_hi = nlev;
            return;
        }
}

// Does k_level4d_lead run a-block a of sharing level t (a leader or a full scan on either side;
// the roles of level4d_body, share_role)?  cost: the split steps its cells scan themselves, a leader
// step at about 2.5 plain steps, a follower its low and top points.
inline bool sched_lead_block(int t, int a, int g_lo, int edges, double *cost) {
    const int b = t - a;
    const ShareRole ar = share_role(true, edges, a, b, g_lo), br = share_role(true, edges, b, a, g_lo);
    if (ar.role == 2 && br.role == 2) return false;
    if (cost) *cost = (ar.role == 1 ? 2.5 : 1.0) * (ar.low + ar.top) + (br.role == 1 ? 2.5 : 1.0) * (br.low + br.top);
    return true;
}

// rank r's blocks of level t that k_level4d_lead runs (the length of its lord list)
inline int sched_lead_count(int t, int G, int r, int g_lo, int g_hi, int edges) {
    if (t < g_lo || t >= g_hi) return 0;
    int cnt = 0;
    for (int a = 0; a <= t; ++a) cnt += shard_owner(a, G) == r && sched_lead_block(t, a, g_lo, edges, nullptr);
    return cnt;
}

struct LevelSched {
    int sharing;     // 1: t in [g_lo, g_hi)
    int split;       // k_level4d's split for rank r's blocks (1 on the sharing levels; 0: no launch)
    int lead_split;  // k_level4d_lead's waves per chunk (0: rank r launches no leader block)
};

// lead_nblk: the length of rank r's lord list at t (< 0: count it, under the edge rule `edges`)
inline LevelSched level_sched(int n, int t, int G, int r, int split_target, int g_lo, int g_hi, int lead_nblk, int edges = 1) {
    LevelSched s{0, 0, 0};
    if (n - t - 2 <= 0 || t < 0) return s;
    s.sharing = t >= g_lo && t < g_hi;
    const int own = shard_count(t, G, r);
    // on the sharing levels the plain launch only has follower cells (short scans): never split
    if (own > 0) s.split = s.sharing ? 1 : sched_level_split(n, t, own, split_target);
    if (!s.sharing) return s;
    if (lead_nblk < 0) lead_nblk = sched_lead_count(t, G, r, g_lo, g_hi, edges);
    if (lead_nblk <= 0) return s;
    // each leader chunk's scans are split over lead_split waves of one workgroup (the barriers
    // inside the leader scans need every wave of the workgroup on the same chunk)
    constexpr int lsplit = 2;  // 1 / 3 / 4 measured +1.1 / +6.5 / +9.4 ms
    // narrow late levels: as many split waves as the plain heuristic would give the rank's blocks
    const int sp = sched_level_split(n, t, own, split_target);
    s.lead_split = sp > lsplit ? sp : lsplit;
    return s;
}

// ---- lockstep batch: K contexts ("members") whose fills advance through the steps
// s = 0 .. max(n_k)-1 together, every kernel of a step launched once for all of them with the member
// index as a grid dimension of its own.  The batched entry points (k_*_many) read tabs[member] and
// the member's own launch arguments of step s from device arrays at wave-uniform addresses and call
// the same bodies as the single-context entry points, so blockIdx.x stays the member's own block
// index.  Members never share split points (g_lo = g_hi = 0 in every member's tables, no leader
// launch): under the default target nothing below n = 159 shares anyway.
struct LevelArgs {         // one member at step s: level t = s, span sigma = s
    long long il_first;    // k_iloop: first work item and item count (0: none)
    int il_nitems;
    int lv_wavesPerA;      // k_level4d: 64-cell chunks per a-block, a-blocks (0: the member has no level s)
    int lv_nblk;
    int pp_ngrp, pp_npairs, pp_blocksA, pp_nout;  // k_ppush(s) (pp_blocksA = 0: none)
    int dg_nb, dg_blocks;  // k_diag2d(s): interval workgroups, + the table workgroups (0: no span s)
    int pad;
};
static_assert(sizeof(LevelArgs) == 48, "LevelArgs");

// One batched k_level4d launch: block size and dynamic LDS are uniform, so it has ONE split for all
// members, taken from the launch's total wave count against the same target as sched_level_split
// (any split is bit-exact: min is order-independent).
struct BatchLevelPlan {
    int split, threads, lds, gridx;
};

}  // namespace ccj

// Kernel launchers (ccj_kernels.hip); all return a hipError_t as int.
extern "C" {
// lockstep batch: one member's arguments of step s (everything that follows from n alone, plus its
// k_iloop items), the level launch's plan (blocks / wpa: per member, may be NULL), and the launches.
// rows: the step's LevelArgs on the device and the same on the host (for the grid extents).
void ccjk_batch_args(int n, int s, long long il_first, int il_nitems, ccj::LevelArgs *out);
ccj::BatchLevelPlan ccjk_batch_level_plan(const int *n, int count, int t, int split_target, int *blocks, int *wpa);
int ccjk_pre_many(const ccj::DevTables *tabs, int count, int nmax, void *stream);  // k_init2d, k_precompute_ie, k_build_il
int ccjk_iloop_many(const ccj::DevTables *tabs, const ccj::LevelArgs *row, const ccj::LevelArgs *hrow, int count, int t, void *stream);
int ccjk_diag2d_many(const ccj::DevTables *tabs, const ccj::LevelArgs *row, const ccj::LevelArgs *hrow, int count, int sigma,
                     void *stream);
int ccjk_level4d_many(const ccj::DevTables *tabs, const ccj::LevelArgs *row, const int *n, int count, int t, int split_target,
                      void *stream);  // n: the members' lengths (host); launches from ccjk_batch_level_plan
int ccjk_ppush_many(const ccj::DevTables *tabs, const ccj::LevelArgs *row, const ccj::LevelArgs *hrow, int count, int lev,
                    void *stream);
int ccjk_init2d(const ccj::DevTables *T, void *stream);
int ccjk_precompute_ie(const ccj::DevTables *T, void *stream);
int ccjk_build_il(const ccj::DevTables *T, void *stream);
int ccjk_iloop(const ccj::DevTables *T, int t, long long first_item, int nitems, int G, int rank, void *stream);
int ccjk_diag2d(const ccj::DevTables *T, int sigma, int G, int rank, void *stream);
// the range check of the six closed-form matrices (site CF), after the last k_diag2d on its stream:
// one workgroup per context / member; nmax = the longest member
int ccjk_cf_low(const ccj::DevTables *T, void *stream);
int ccjk_cf_low_many(const ccj::DevTables *tabs, int count, int nmax, void *stream);
// band-sharded over RCCL: the ranks' LEVEL / ILOOP / PARTIAL bits as one summed 4-byte word (spread:
// err -> *word, a count field per site; merge: every non-zero field of *word back into err)
int ccjk_range_spread(const ccj::DevTables *T, unsigned *word, void *stream);
int ccjk_range_merge(const ccj::DevTables *T, const unsigned *word, void *stream);
int ccjk_dtail_pack(const ccj::DevTables *T, int sigma, int G, int rank, int16_t *tail, void *stream);
int ccjk_dtail_unpack(const ccj::DevTables *T, int sigma, const int16_t *recv, size_t slice, size_t off, int G, int rank,
                      void *stream);
int ccjk_level4d(const ccj::DevTables *T, int t, int G, int rank, int copies, void *stream);
int ccjk_level_split(int n, int t, int nblk, int split_target);
int ccjk_level4d_lead(const ccj::DevTables *T, int t, int G, int rank, void *stream);
int ccjk_pack(const ccj::DevTables *T, int t, int G, int r, int part, int nmax, int16_t *send, void *stream);
int ccjk_unpack(const ccj::DevTables *T, int t, int G, int r, int part, int nmax, const int16_t *recv, size_t rstride, void *stream);
int ccjk_pterm(const ccj::DevTables *T, int sigma, void *stream);
int ccjk_ppush(const ccj::DevTables *T, int lev, int G, int rank, void *stream);
int ccjk_ptail_pack(const ccj::DevTables *T, int sigma, int16_t *tail, void *stream);
int ccjk_ptail_unpack(const ccj::DevTables *T, int sigma, const int16_t *recv, size_t slice, size_t off, int G, void *stream);
int ccjk_items(const ccj::DevTables *T, int G, int rank, int simulate, long long *counts, const long long *offs,
               uint32_t *items, int pass, void *stream);
int ccjk_canon(const ccj::DevTables *T, int x, const long long *offij, int16_t *out, void *stream);
int ccjk_expand(const ccj::DevTables *T, int t, int first_slot, int16_t *out, void *stream);
// The n-dependent device state of a binding (k_bind_layout): the nent = max(n, 1) level descriptors
// (lv, lb, ld, ldx) from T->n, T->d4, T->xpad and nm4, and 32767 over x_cnt elements from x_fill and
// pm_cnt from pm_fill (16-byte aligned; 0: no fill).
int ccjk_bind_layout(const ccj::DevTables *T, int nent, int nm4, ccj::LevelDesc *lv, long long *lb, ccj::LvlDev *ld,
                     ccj::LvlX *ldx, int16_t *x_fill, long long x_cnt, int16_t *pm_fill, long long pm_cnt, void *stream);
}
