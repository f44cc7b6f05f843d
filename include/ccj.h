/*
 * ccj.h — C ABI of libccj_hip.so, the MI355X-native CCJ pseudoknot MFE engine.
 *
 * Drop-in boundary.  The reference has no FFI; its seam is the fill loop of
 * W_final::ccj() (reference src/W_final.cc:60-67), which calls, per interval (i,l),
 *   s_energy_matrix::compute_energy / compute_WMv_WMp / compute_energy_WM  (s_energy_matrix.cc:206-358)
 *   pseudo_loop::compute_energies                                            (pseudo_loop.cc:69-132)
 * and afterwards W (W_final.cc:68-79), backtrack (W_final.cc:84-104, pseudo_loop.cc:861-2820)
 * and bracket emission (W_final.cc:764-819).  This ABI replaces that whole body: one
 * ccj_fill() runs every recurrence on the GPU; ccj_result() runs W + backtrack + emission on
 * the GPU by default (k_compute_W / k_backtrack over the device matrices), or, with
 * ccj_options.host_traceback = 1, on the host against a host mirror; the getters keep the
 * reference's semantics either way.
 *
 * Plain C types only (no torch / HIP types).  All positions are 1-based like the reference.
 * Not re-entrant per context; independent contexts may run on separate host threads.
 */
#ifndef CCJ_H
#define CCJ_H

#include <stdint.h>
#include "ccj_params.h"

#ifdef __cplusplus
extern "C" {
#endif

/* error codes (SURVEY.md §8b "Errors") */
#define CCJ_OK           0
#define CCJ_E_ARG        1   /* bad argument (sequence, n, parameter blob) */
#define CCJ_E_OOM        2   /* host or device allocation failed */
#define CCJ_E_HIP        3   /* HIP runtime error */
#define CCJ_E_PARAMS     4   /* parameter set outside what the int16 tables can represent */
#define CCJ_E_BACKTRACK  5   /* reference backtrack would exit(EXIT_FAILURE); message in ccj_last_error() */
#define CCJ_E_STATE      6   /* call out of order (e.g. ccj_result before ccj_fill) */
#define CCJ_E_INTER_EXIT 7   /* reference "NOT GOOD RESTR INTER" path: it prints and exit(0) */
#define CCJ_E_COMM       9   /* band-sharded exchange failed: an RCCL error on the communicator, or no
                                progress within CCJ_COMM_TIMEOUT_S seconds (default 300; a peer rank
                                died or hung); the communicator is aborted and the context must be
                                destroyed */
#define CCJ_E_RANGE     11   /* the fold leaves the domain in which a reference-identical result exists:
                                some 4-D value lies below -32768 before it is stored, where the
                                reference's int16 assignment (matrices.hh:188-191) wraps.  The fill
                                detects it exactly and ccj_fill / ccj_fill_device /
                                ccj_wait / ccj_result return this code and report no structure or
                                energy; ccj_range_flags names the detection sites.  The context stays
                                usable (ccj_reset, ccj_rebind), and the getters, ccj_hashes and
                                ccj_sync_host still serve the clamp-only matrices the fill computed.
                                With CCJ_ALLOW_OUT_OF_RANGE=1 in the environment (read at call time)
                                the fold completes under those clamp-only semantics instead, and
                                ccj_range_flags still reports. */

/* Where the last fill of the context saw a 4-D value below -32768 (0: the fold lies inside the
 * domain and the result is the reference's, bit for bit).  One bit per kind of place where the
 * engine narrows to int16 or stands in for a per-cell store:
 *   LEVEL   the ten values a level-kernel cell stores
 *   ILOOP   an interior-loop minimum of PL / PR / PM handed to the level kernel as int16
 *   PARTIAL a leader's partial minimum packed as int16 for a follower cell
 *   TAB     an entry of the six PL / PR multiloop tables that belongs to a valid cell
 *   CF      a PM / PO multiloop closed form at a valid cell
 * A band-sharded rank reports the union over all ranks. */
#define CCJ_RANGE_LEVEL   1
#define CCJ_RANGE_ILOOP   2
#define CCJ_RANGE_PARTIAL 4
#define CCJ_RANGE_TAB     8
#define CCJ_RANGE_CF      16

/* 4-D gap matrices, reference pseudo_loop.hh:62-108 / allocation order pseudo_loop.cc:37-62 */
enum ccj_mat4 {
    CCJ_PK = 0, CCJ_PL, CCJ_PR, CCJ_PM, CCJ_PO,
    CCJ_PfromL, CCJ_PfromR, CCJ_PfromM, CCJ_PfromMprime, CCJ_PfromO,
    CCJ_PLmloop00, CCJ_PLmloop01, CCJ_PLmloop10,
    CCJ_PRmloop00, CCJ_PRmloop01, CCJ_PRmloop10,
    CCJ_PMmloop00, CCJ_PMmloop01, CCJ_PMmloop10,
    CCJ_POmloop00, CCJ_POmloop01, CCJ_POmloop10,
    CCJ_NMAT4
};

/* 2-D interval matrices (raw stored value for 1 <= i <= j <= n) */
enum ccj_mat2 {
    CCJ_M2_P = 0, CCJ_M2_WBP, CCJ_M2_WPP, CCJ_M2_V, CCJ_M2_VTYPE, CCJ_M2_WM, CCJ_M2_WMV, CCJ_M2_WMP,
    CCJ_NMAT2
};

typedef struct ccj_problem {
    const char *seq;                 /* upper-case A/C/G/U/T, length n (validated by caller like CCJ.cc:23-36) */
    int dangles;                     /* -d, reference W_final.cc:25 */
    int noGU;                        /* --noGU global, reference pair_mat.h:94-95 */
    const ccj_energy_params *params; /* scaled 37 C tables (include/ccj_params.h) */
    const ccj_pk_penalties *pen;     /* NULL -> reference h_globals.hh defaults */
} ccj_problem;

typedef struct ccj_ctx ccj_ctx;

/* Engine options for ccj_create.  device = HIP device ordinal. */
typedef struct ccj_options {
    int device;
    int overlap_d2h;     /* 1: stream finished levels to the host mirror while later levels compute */
    /* Band sharding of one sequence over shard_world processes (one per GPU):
     * this process computes the a-blocks ccj_shard_blocks() gives it and each level is all-gathered
     * over RCCL (ccj_comm_init, or ccj_comm_init_local, before the first fill).  0 or 1 = unsharded. */
    int shard_world;
    int shard_rank;
    int shard_simulate;  /* 1: run every shard's launches in this one context, no exchange (tests) */
    /* 0 (default): W and the traceback run on the GPU (no host copy of the 4-D matrices; getters
     * copy them on first use).  1: the same traceback logic run on the host over the mirror (tests). */
    int host_traceback;
    /* Level-kernel tuning (0 = default for both).
     * split_target: narrow levels split each cell's split-point loops over up to 8 waves so
     *   about this many waves run at once (default 9216); < 0 never splits.  It also places the
     *   sharing range: from the first level that runs unsplit to the last.  Under the default
     *   no level runs unsplit below n = 159, so smaller folds share nothing; small targets
     *   reproduce every regime at small n (ccj_level_schedule below; tests/test_schedule.py).
     * share_splits: split-point sharing between the cells of one gap column: a
     *   leader cell scans its whole split range once for itself and the next CCJ_SHARE_R-1 cells of
     *   its column; < 0 turns it off (every cell scans its own range). */
    int split_target;
    int share_splits;
} ccj_options;

/* Create a context for one sequence: copies the problem, allocates device + pinned host
 * storage (22 x C(n+1,4) int16 + 2-D tables).  Replaces W_final::W_final + space_allocation
 * (reference W_final.cc:20-56).  opts may be NULL. */
int  ccj_create(const ccj_problem *prob, const ccj_options *opts, ccj_ctx **out);

/* Rebind a context to another sequence of the same length n (same tables, dangles, noGU,
 * options): rebuilds only the sequence tables and the interior-loop work lists and reuses every
 * allocation, so a batch of equal-length sequences pays ccj_create's multi-GB allocation once.
 * The reference has no equivalent (each fold constructs a new W_final, W_final.cc:20-56).
 * Blocking: the interior-loop work-list count pass runs on the context's stream and the call
 * waits for it (the host sizes the fill's launches from the counts), so it returns only after
 * the work already queued on that stream; with CCJ_HOST_COUNT=1 the count runs on host threads.
 * CCJ_E_ARG if the length differs or the sequence has characters other than ACGUT; CCJ_E_STATE
 * while a fold is in flight. */
int  ccj_reset(ccj_ctx *ctx, const char *seq);

/* One context for sequences of any length 1 .. nmax (a mixed-length batch without an allocation per
 * sequence or a context per length): ccj_create_cap sizes every buffer for the capacity nmax and binds
 * prob->seq (1 <= length <= nmax, else CCJ_E_ARG); ccj_create(p, o, out) is ccj_create_cap(p, o,
 * strlen(p->seq), out), and at length == capacity every offset, descriptor and launch is the same.
 * ccj_rebind binds another sequence of any length up to the capacity; with the bound length it is
 * ccj_reset.  A rebind allocates nothing and copies nothing synchronously: the level descriptors and
 * the sentinels of the new layout are written by a kernel on the context's stream (k_bind_layout), the
 * leader lists and sequence tables go up from pinned staging, and the call waits only where ccj_reset
 * does (the work-item counts).  CCJ_E_ARG for a longer sequence or a character outside ACGUT,
 * CCJ_E_STATE while a fold is in flight; a refused rebind leaves the previous binding usable.
 * ccj_n is the bound length, ccj_capacity the capacity.  ccj_reset still refuses another length.
 * A band-sharded context (shard_world > 1, simulated or not) holds one length: ccj_create_cap with
 * nmax != length and a rebind to another length are refused with CCJ_E_ARG. */
int  ccj_create_cap(const ccj_problem *prob, const ccj_options *opts, int nmax, ccj_ctx **out);
int  ccj_rebind(ccj_ctx *ctx, const char *seq);
int  ccj_capacity(const ccj_ctx *ctx);

/* ---- constrained folding: forbidden pairs and unpaired positions ----
 * A constraint belongs to one binding of a sequence of length n.  It defines a symmetric set F of
 * position pairs (i, j), 1 <= i < j <= n:
 *   allow_only (non-NULL): F starts as the complement of the listed pairs (NULL: empty);
 *   unpaired: NULL, or a string of length n over '.' and 'x'; 'x' at position p adds (p, q) for every q;
 *   forbid: adds its pairs.
 * Pair lists hold 1-based positions, pair k = (list[2k], list[2k+1]) with list[2k] < list[2k+1].
 * A constrained fold is the reference's fill, W, traceback and emission with one change: every lookup
 * pair[S[i]][S[j]] at positions (i, j) gives 0 where (i, j) is in F.  The energy functions, penalties,
 * noGU, the int16 store and the CCJ_E_RANGE domain stay; a pair that could not pair anyway changes
 * nothing; an empty F is the unconstrained fold, and F = every G-U position pair with noGU = 0 is the
 * reference's --noGU run.  Pairs cannot be forced, and the partition function (ccj_pf.h) takes no
 * constraint.
 *   ccj_reset_constrained / ccj_rebind_constrained: ccj_reset / ccj_rebind with the constraint `cons`
 *     (NULL: none).  A constrained fold from the start is ccj_create_cap + ccj_rebind_constrained.
 *   ccj_batch_bind_constrained: ccj_batch_bind where member k folds seqs[k] under cons[k]; cons, or any
 *     of its entries, may be NULL.
 *   The plain ccj_reset, ccj_rebind and ccj_batch_bind bind without a constraint, so a context never
 *   carries a stale one.
 * A bad constraint (an unpaired string of another length or with another character, a pair with
 * i >= j or a position outside 1..n, a negative count, a forbid count without its list) is refused with
 * CCJ_E_ARG before the context or any batch member is touched: the previous binding still folds.
 *   ccj_constraint_count: |F| over the pairs (i, j) whose bases could pair under the binding's table
 *     (after noGU), whatever their distance; 0 for an unconstrained binding and for NULL.
 * Band-sharded contexts: every rank must be given the same constraint (over RCCL this is the caller's
 * duty and unverified, like the rest of that path). */
typedef struct ccj_constraint {
    const char *unpaired;   /* NULL, or length n over '.' / 'x' */
    const int *forbid;      /* 2 * n_forbid positions */
    int n_forbid;
    const int *allow_only;  /* NULL: no allow-only list; else 2 * n_allow positions (n_allow may be 0) */
    int n_allow;
} ccj_constraint;
int  ccj_reset_constrained(ccj_ctx *ctx, const char *seq, const ccj_constraint *cons);
int  ccj_rebind_constrained(ccj_ctx *ctx, const char *seq, const ccj_constraint *cons);
long long ccj_constraint_count(const ccj_ctx *ctx);
/* Element counts of every device buffer whose size depends on n (host helper, no GPU), in the order
 * of ccj_layout_extent_names() (space separated):
 *   d4 (int16; 6 per cell, 22 with full4), rec, rk, rl (one 8 / 8 / 4-byte record per cell), acc
 *   (the partial-record ring, 8-byte slots), d4x, pmx (the interior-loop copies with their pads, int16),
 *   lord, lord_off (the leader list, int16, and its offsets, int), plane (one 2-D plane, (n+1)(n+2)),
 *   il, ilseg (candidate-list entries, segment-table words), levels (descriptors), lx (the lx table),
 *   events (per-level events of each kind), icount (per-level count / offset words),
 *   ppush_span, iloop_span (bytes a k_ppush / k_iloop wave addresses from one base; must stay < 4 GB).
 * as_capacity = 0: what a binding of n uses; 1: what a context of capacity n allocates, the maximum
 * over every length up to n (equal wherever an extent grows with n; the sharing range, and with it
 * acc, lord and lord_off, moves with n and the target).  split_target: the resolved target (0 = never
 * split); share: 0 = sharing off; full4: d4 holds all 22 slots.  For an unsharded context.
 * Returns the entry count and fills out when cap >= it; < 0: bad arguments. */
int  ccj_layout_extents(int n, int split_target, int share, int full4, int as_capacity, long long *out, int cap);
const char *ccj_layout_extent_names(void);

/* Run the whole DP fill on the GPU (replaces W_final.cc:60-67).  With host_traceback = 1 it
 * also makes the host mirror valid (ccj_sync_host is implied); by default the matrices stay on
 * the device and the getters copy them on first use. */
int  ccj_fill(ccj_ctx *ctx);

/* Device-only fill, no host mirror (for timing the kernels alone).  CCJ_E_STATE while a fold
 * is in flight (ccj_fill_async without ccj_wait). */
int  ccj_fill_device(ccj_ctx *ctx);
/* Copy the device matrices to the host mirror. */
int  ccj_sync_host(ccj_ctx *ctx);

/* W (W_final.cc:68-79), backtrack and bracket emission: on the GPU by default (k_compute_W,
 * k_backtrack; results copied back), on the host mirror with host_traceback = 1.  Both are
 * bit-identical to the reference.
 * structure: buffer of n+1 chars (NUL-terminated on return); *energy_kcal = W[n]/100.0;
 * stdout_msgs: optional buffer receiving the reference's stdout side messages
 * ("Should not be here!\n" lines, W_final.cc:715), NUL-terminated, may be NULL. */
int  ccj_result(ccj_ctx *ctx, char *structure, double *energy_kcal, char *stdout_msgs, int msgs_cap);

/* Asynchronous fold, for pipelining a batch over contexts: ccj_fill_async enqueues the fill and
 * (device traceback) W + traceback on the context's streams and returns at once; ccj_wait blocks
 * until they are done and returns exactly what ccj_fill + ccj_result would.  While one context's
 * traceback (one wave) runs, another context's fill can use the rest of the GPU.  One fold in
 * flight per context; ccj_reset / ccj_fill refuse with CCJ_E_STATE until ccj_wait. */
int  ccj_fill_async(ccj_ctx *ctx);
/* The same, but the fill starts only when `after`'s last enqueued fill has ended (not its W +
 * traceback): two contexts on one device then alternate fills back to back while each fold's
 * traceback runs beside the next fill.  after == NULL: ccj_fill_async. */
int  ccj_fill_async_after(ccj_ctx *ctx, const ccj_ctx *after);
int  ccj_wait(ccj_ctx *ctx, char *structure, double *energy_kcal, char *stdout_msgs, int msgs_cap);

/* ---- lockstep batch: many short sequences in one set of level launches ----
 * A short fold costs its chain of per-level launches and events, not its cells.  A lockstep batch is
 * `members` capacity contexts with one set of parameters, dangles, noGU, penalties and options whose
 * fills run as ONE wavefront over the levels: every kernel of a level is launched once for all bound
 * members, with the member index as a grid dimension, so the chain is paid once per batch.  Members
 * shorter than the longest idle through the late levels (batch sequences of similar length).  The
 * kernels' arithmetic is the single context's: every result is bit-identical.
 *   ccj_batch_create: p->seq may be NULL.  CCJ_E_ARG with shard_world > 1, host_traceback,
 *     overlap_d2h or share_splits > 0 (members never share split points; under the default target
 *     nothing below n = 159 shares anyway).
 *   ccj_batch_bind: member k folds seqs[k], 1 <= count <= members, each of length 1 .. nmax; the
 *     other members idle.  CCJ_E_ARG (sequence too long, character outside ACGUT, bad count) leaves
 *     the previous binding usable; CCJ_E_STATE while a fold is in flight.
 *   ccj_batch_fold_async / ccj_batch_wait: enqueue the fill, W and the traceback of every bound
 *     member / wait for them and check every member's error word.  Afterwards each bound member is in
 *     the state ccj_wait leaves (filled, result available): ccj_result, the getters, ccj_hashes,
 *     ccj_sync_host and ccj_n work on it; a member whose traceback ends in a reference exit reports it
 *     from ccj_result and does not disturb the others.  Likewise a member whose fold leaves the domain
 *     (CCJ_E_RANGE above): ccj_batch_wait returns CCJ_OK, that member's ccj_result CCJ_E_RANGE.
 *   ccj_batch_member: borrowed (ccj_destroy ignores it); its own ccj_rebind, ccj_reset and ccj_fill*
 *     return CCJ_E_STATE while it belongs to the batch.
 *   ccj_batch_level_plan (host helper, no GPU): the batched k_level4d launch of level t for members of
 *     lengths n[0 .. count) under the resolved split_target (0 = never split), from the one function
 *     the launch itself uses: out[0..3] = {split (1, 2, 4, 8; 0: no member has level t), block threads,
 *     dynamic LDS bytes, grid x}, then per member {workgroups, 64-cell chunks per a-block}; out holds
 *     4 + 2 * count ints.  One split serves all members: it comes from the launch's total wave count
 *     against the same target as ccj_level_schedule's. */
typedef struct ccj_batch ccj_batch;
int  ccj_batch_create(const ccj_problem *p, const ccj_options *o, int nmax, int members, ccj_batch **out);
int  ccj_batch_bind(ccj_batch *b, const char *const *seqs, int count);
/* member k folds seqs[k] under cons[k] (constrained folding above; cons or cons[k] may be NULL) */
int  ccj_batch_bind_constrained(ccj_batch *b, const char *const *seqs, const ccj_constraint *const *cons, int count);
int  ccj_batch_fold_async(ccj_batch *b);
int  ccj_batch_wait(ccj_batch *b);
ccj_ctx *ccj_batch_member(ccj_batch *b, int k);
int  ccj_batch_members(const ccj_batch *b);
int  ccj_batch_count(const ccj_batch *b);              /* bound members */
double ccj_batch_fill_ms(const ccj_batch *b);          /* the last fold's fill, first launch to last span (ms) */
const char *ccj_batch_last_error(const ccj_batch *b);  /* b == NULL: the last failed ccj_batch_create */
int  ccj_batch_level_plan(const int *n, int count, int t, int split_target, int *out);
void ccj_batch_destroy(ccj_batch *b);

/* Reference getter semantics (matrices.hh:177-182: INF outside i<=j<k-1<=l-1). */
int  ccj_get4(const ccj_ctx *ctx, int mat, int i, int j, int k, int l);
/* Raw 2-D value for 1 <= i <= j <= n (ccj_mat2). */
int  ccj_get2(const ccj_ctx *ctx, int mat, int i, int j);
/* W[j], 0 <= j <= n (valid after ccj_result). */
int  ccj_getW(const ccj_ctx *ctx, int j);
/* FNV-1a 64 hashes in canonical order: 22 4-D matrices, 8 2-D (ccj_mat2), W. out[31]. */
int  ccj_hashes(const ccj_ctx *ctx, uint64_t *out);

/* Timing of the last ccj_fill_device (ms, HIP events on the streams the kernels run on) and of
 * its kernel families: kernel_ms[0] = k_level4d, [1] = k_diag2d, [2] = precompute. */
int  ccj_last_timing(const ccj_ctx *ctx, double *fill_ms, double *kernel_ms3);
/* Sum of the k_iloop (interior-loop pass) times of the last fill (ms). */
double ccj_iloop_ms(const ccj_ctx *ctx);
/* summed k_ppush (P terms) launch times of the last fill in timing mode 2 (ms) */
double ccj_ppush_ms(const ccj_ctx *ctx);
/* Host side of the last fold (ms): out3[0] = wait for the host mirror (D2H tail), [1] = W, [2] = backtrack. */
int  ccj_host_timing(const ccj_ctx *ctx, double *out3);
/* Per-level kernel times of the last fill (ms): level_ms[t] (k_level4d, level t), diag_ms[s]
 * (k_diag2d, span s); ccj_iloop_times: iloop_ms[t] (k_iloop, level t). */
int  ccj_level_times(const ccj_ctx *ctx, double *level_ms, double *diag_ms, int cap);
/* Band-sharded contexts in timing mode 2, per level (0 elsewhere; either pointer may be NULL):
 * edge_ms[t] = the edge part's share of the level span on the level stream (from the end of the
 * level's launches to the end of its unpack: the waits for the P and span tails, pack, all-gather,
 * unpack); bulk_ms[t] = the bulk part on its side stream (from the level's end: pack, all-gather,
 * unpack), which overlaps the next level. */
int  ccj_exchange_times(const ccj_ctx *ctx, double *edge_ms, double *bulk_ms, int cap);
int  ccj_iloop_times(const ccj_ctx *ctx, double *iloop_ms, int cap);
/* ccj_ppush_times: ppush_ms[t] (k_ppush after level t), timing mode 2 */
int  ccj_ppush_times(const ccj_ctx *ctx, double *ppush_ms, int cap);
/* What the next fills time (HIP events): 0 = the fill only; 1 (default) = + per-level durations
 * (level_ms, from events the fill records anyway); 2 = + k_diag2d / k_iloop times and level spans
 * from extra marker events around every launch (they slow the fill down by a few percent). */
int  ccj_set_timing(ccj_ctx *ctx, int mode);

/* ---- band sharding (one sequence over several GPUs) ---- */
#define CCJ_COMM_ID_BYTES 128
/* A fresh RCCL unique id (call on one rank, broadcast the bytes to the others). */
int  ccj_comm_unique_id(char *id_out);
/* Join the sharded context to the RCCL communicator of shard_world ranks. */
int  ccj_comm_init(ccj_ctx *ctx, const char *id);
/* The a-blocks of level t that rank computes (host helper, no GPU): writes up to cap of them to
 * a_out, ascending, and returns how many there are (< 0: bad arguments).  Block a belongs to rank
 * (a / 4) % world on every level. */
int  ccj_shard_blocks(int n, int t, int world, int rank, int *a_out, int cap);
/* Per-matrix element count C_t of level t and the a-block size M_t (the same for every world). */
int  ccj_level_layout(int n, int t, int world, long long *C, int *M);
/* The launch regime of level t for one rank (host helper, no GPU), from the one
 * schedule function the launches themselves use.  split_target: the resolved target (0 = never
 * split, what ccj_options.split_target < 0 resolves to); share: 0 = sharing off.
 * out5 = {sharing (1: t in [g_lo, g_hi)),
 *         k_level4d's split for the rank's blocks: 1, 2, 4 or 8 (0: the rank has no block at t),
 *         k_level4d_lead's waves per chunk: 2, 4 or 8 (0: the rank launches no leader block at t),
 *         g_lo, g_hi}.
 * Levels [g_lo, g_hi) share (0, 0: none); followers on g_lo .. g_lo+2 whose leader would lie
 * below g_lo scan their full range in the leader launch.  CCJ_E_ARG on bad arguments; a level
 * without cells (t > n-3) gives zeros with the range. */
int  ccj_level_schedule(int n, int t, int world, int rank, int split_target, int share, int *out5);
/* The same for a live context, with the target and share flag it resolved from its options and
 * the environment (CCJ_SPLIT_TARGET, CCJ_SHARE_SPLITS) and the leader lists it launches from:
 * out7 = the five values above, then {resolved split_target, share (0/1)}.  rank < 0: the
 * context's own rank; another rank only in a shard_simulate context. */
int  ccj_ctx_level_schedule(const ccj_ctx *ctx, int t, int rank, int *out7);
/* The split-point-sharing roles of a-block a (0 .. t) of level t (host helper, no GPU),
 * from the one role function the level kernels and the leader lists use.  split_target as above;
 * edges: 1 = columns whose other gap is below 3 share too (the default), 0 = they scan in full
 * (what CCJ_SHARE_EDGES=0 makes a context do).  out16 = the a-loop's side, then the b-loop's, each
 *   {role (0 full scan, 1 leader, 2 follower), low, top (the cell scans split points 1 .. low and
 *    len-top+1 .. len of its range 1 .. len itself), cut of follower r = 1, 2, 3 (a leader leaves its
 *    top `cut` split points out of that follower's partial; 0 for other roles)},
 * then {1: k_level4d_lead runs the block, 1: level t shares, g_lo, g_hi}. */
int  ccj_share_roles(int n, int t, int a, int split_target, int edges, int *out16);
/* The level-t exchange is two all-gathers: part 0 ("edge") = each rank's blocks
 * a % 4 == 3, the only cells of level t another rank's level t+1 reads, then its P(t+1) partials
 * (4(n+1) elements) and span t (20(n+1) elements), on the level stream; part 1 ("bulk") = the other
 * blocks, no tail, on a side stream that overlaps level t+1.  (P(n-1)'s partials travel alone after
 * the last level.)  ccj_exchange_layout (host helper, no GPU; the geometry k_pack / k_unpack use), in
 * int16 elements: out3 = {nmax (the largest rank's block count of the part), tail offset, slice size}.
 * The body is [matrix][part index][cell] of nmax blocks per matrix. */
int  ccj_exchange_layout(int n, int t, int world, int part, long long *out3);
/* which = 0: for each body element of rank's slice of the part, the level element (x*C + a*M + c:
 * matrix-major by matrix index x of ccj_mat4; d4 keeps matrix x at its storage slot) packed there
 * (-1: padding); which = 1: for each level element, its position in the part's
 * gathered buffer (owner * slice + body position) as rank unpacks it (-1: rank's own cell or the other
 * part's).  Returns the entry count; fills out only when cap >= that count.  < 0: bad arguments. */
long long ccj_exchange_index(int n, int t, int world, int rank, int part, int which, long long *out, long long cap);
/* In-process exchange group (tests, and several ranks sharing one device): shard_world contexts,
 * each driven by its own host thread, join one group instead of an RCCL communicator. */
typedef struct ccj_group ccj_group;
int  ccj_group_create(int world, ccj_group **out);
void ccj_group_destroy(ccj_group *g);
int  ccj_comm_init_local(ccj_ctx *ctx, ccj_group *g);

/* Algorithmic work model of this sequence:
 * out[0] = bytes moved by the 4-D level kernels (2 B per int16 operand read + 44 B of writes per cell),
 * out[1] = bytes of the P terms in the 2-D kernels, out[2] = R4 (4-D operand reads), out[3] = cells. */
int  ccj_work_model(const ccj_ctx *ctx, double *out4);
/* Split of out[0] by kernel: out2[0] = bytes of k_iloop (interior-loop candidate reads),
 * out2[1] = bytes of k_level4d (split-point, stack and t-2 reads + 44 B of stores per cell). */
int  ccj_work_split(const ccj_ctx *ctx, double *out2);
/* Same model for a bare sequence (no GPU, no context). */
int  ccj_work_model_seq(const char *seq, int noGU, double *out4);

int  ccj_n(const ccj_ctx *ctx);
const char *ccj_last_error(const ccj_ctx *ctx);
/* The CCJ_RANGE_* bits of the context's last fill (above); 0 inside the domain, before any fill and
 * for a NULL context.  A lockstep batch's member reports its own fold's. */
int  ccj_range_flags(const ccj_ctx *ctx);
void ccj_destroy(ccj_ctx *ctx);

/* Number of 4-D DP cells (unit of work): C(n+1,4). */
uint64_t ccj_num_cells(int n);

/* The closed forms of the PM / PO multiloop families on the host, no GPU: from the
 * raw WBP of a sequence (row-major (n+1) x (n+1), entry i*(n+1)+j, 1 <= i <= j <= n) and bp, cp, the
 * stored values of PMmloop00/01/10 and POmloop00/01/10 (in that order, `cells` values each) of every
 * valid cell in the order i, j >= i, k >= j+2, l >= k (l fastest).  Returns the cells per matrix
 * (out may be NULL to count), or -1. */
long long ccj_pmpo2d_closed(int n, const int *wbp, int bp, int cp, int16_t *out, long long cells);
/* From the same inputs, out6[x] = the lowest value of matrix x (the same order) over the valid cells
 * before the store's clamp at 32767 (INF when n has no valid cell): the fold's CCJ_RANGE_CF bit is
 * "some out6[x] < -32768".  O(n^2) per formula branch, not O(n^4).  Returns 0, or -1. */
int  ccj_pmpo2d_low(int n, const int *wbp, int bp, int cp, int *out6);
/* The same minima cell by cell, O(n^4) (tests): over the valid cells, or with valid_only = 0 over every
 * pair of intervals (i,j), (k,l) whether or not they form a cell.  -2: the formulas' branch list
 * disagrees with ccj_pmpo2d_closed's evaluator at some valid cell. */
int  ccj_pmpo2d_low_brute(int n, const int *wbp, int bp, int cp, int valid_only, int *out6);

/* Interior-loop candidate lists: the list builder drops the candidates that are
 * dominated through a stacked pair, which changes no stored value.  CCJ_IL_PRUNE=0 in the
 * environment (read when a fill is enqueued) keeps the full lists.
 * ccj_il_counts: after a fill, out4 = kept and full entry counts of the context's il lists (PL, PR),
 * then of its ilm lists (PM), over the pairs that can pair.
 * ccj_il_prune_host: the same rule on the host, no GPU, for prob's sequence, parameters and penalties.
 * Planes are [w][p] = w*(n+2)+p over (n+1)(n+2) elements; windows are plane x 29 x 29, [u1][u2].
 * counts4 as ccj_il_counts; e_il / e_ilm: each list entry's e_intP energy; st_il / st_ilm: 0 = not in
 * the list, 1 = kept, 3 / 5 / 7 = dropped (through the pair stacked on the list's own pair / on the
 * candidate's pair / either); est, ie: the e_stP plane and the e_intP plane of the loop without
 * unpaired bases.  Any output may be NULL. */
int  ccj_il_counts(ccj_ctx *ctx, long long *out4);
int  ccj_il_prune_host(const ccj_problem *prob, long long *counts4, int16_t *e_il, int16_t *e_ilm, uint8_t *st_il,
                       uint8_t *st_ilm, int16_t *est, int16_t *ie);
/* The same under a constraint (NULL: none; CCJ_E_ARG for a bad one): every pair the rule uses, the
 * intermediate stacked pair of a witness included, is one that can pair under the binding. */
int  ccj_il_prune_host_constrained(const ccj_problem *prob, const ccj_constraint *cons, long long *counts4, int16_t *e_il,
                                   int16_t *e_ilm, uint8_t *st_il, uint8_t *st_ilm, int16_t *est, int16_t *ie);
/* ccj_work_model_seq under a constraint (NULL: none; CCJ_E_ARG for a bad one). */
int  ccj_work_model_seq_constrained(const char *seq, int noGU, const ccj_constraint *cons, double *out4);

#ifdef __cplusplus
}
#endif

#endif /* CCJ_H */
