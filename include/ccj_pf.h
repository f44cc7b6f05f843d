/*
 * ccj_pf.h — C ABI of the CCJ partition function in libccj_hip.so.
 *
 * Replaces the reference's W_final_pf (src/part_func.hh:28-194): the constructor
 * (part_func.cc:31-93, Boltzmann tables of scale_pf_parameters() + rescale_pk_globals
 * :127-146 + exp_params_rescale :97-125), the fill ccj_pf() (part_func.cc:152-178: every
 * compute_* of :222-699 over the same 2-D / 4-D matrices) and the stochastic traceback
 * Sample_W/V/VM/WM/WMv/WMp (stoch_backtrack.cc:36-326).  The reference never compiles these
 * files into its binary (CMakeLists.txt:23,25) and never calls them (CCJ.cc:51-56,105); this ABI
 * is what a maintainer would bind to switch that path on.
 *
 * Semantics are the reference's as written, evaluated in IEEE double without contraction (the
 * oracle builds part_func.cc with -ffp-contract=off): every 4-D matrix stores the x86 int
 * truncation of its double sum (Matrix4DPF::set takes an int, matrices.hh:265-267, and get
 * returns int, :251-263), the P term multiplies those ints in 32-bit int arithmetic
 * (part_func.cc:388), expinternal[] is read past its 31 entries for pseudoknot interior loops
 * longer than 30 (part_func.cc:874 -> internal.h:645), and the recurrences keep the reference's
 * typos (POmloop00's '=' :673, PMmloop01 / POmloop10's '+' :645,695, get_WB/get_WP's '+'
 * :706,714).  DESIGN.md §10 lists them.
 *
 * Plain C types only.  Positions are 1-based like the reference.
 */
#ifndef CCJ_PF_H
#define CCJ_PF_H

#include <stdint.h>
#include "ccj.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CCJ_E_PF_SAMPLE 8 /* a Sample_* "backtracking failed" path: the reference prints and exit(0)s */
#define CCJ_E_PF_RANGE 10 /* ccj_pf_fill: some P(i,l) has sum |terms| >= 2^53, so the reference's serial
                             double sum of its int products (part_func.cc:383-393) could round
                             differently from the exact sum the GPU forms; no result is reported.
                             Only reachable for long sequences (never below n = 296). */

/* 4-D matrices of W_final_pf (part_func.hh:86-113), in canonical-hash order */
enum ccj_pf_mat4 {
    CCJ_PF_PK = 0, CCJ_PF_PL, CCJ_PF_PR, CCJ_PF_PM, CCJ_PF_PO,
    CCJ_PF_PfromL, CCJ_PF_PfromR, CCJ_PF_PfromM, CCJ_PF_PfromO,
    CCJ_PF_PLmloop00, CCJ_PF_PLmloop01, CCJ_PF_PLmloop10,
    CCJ_PF_PRmloop00, CCJ_PF_PRmloop01, CCJ_PF_PRmloop10,
    CCJ_PF_PMmloop00, CCJ_PF_PMmloop01, CCJ_PF_PMmloop10,
    CCJ_PF_POmloop00, CCJ_PF_POmloop01, CCJ_PF_POmloop10,
    CCJ_PF_NMAT4
};

/* 2-D matrices (TriangleMatrix_PF, part_func.hh:62,76-84) */
enum ccj_pf_mat2 {
    CCJ_PF_V = 0, CCJ_PF_VM, CCJ_PF_WM, CCJ_PF_WMv, CCJ_PF_WMp, CCJ_PF_WBP, CCJ_PF_WPP, CCJ_PF_P,
    CCJ_PF_NMAT2
};

typedef struct ccj_pf_ctx ccj_pf_ctx;

/* The raw 37 C tables the Boltzmann weights of the dangles and the multiloop / exterior
 * mismatches come from (ViennaRNA dangle5_37, dangle3_37, mismatchM37, mismatchExt37).  The MFE
 * blob holds them clamped to <= 0 (params.c:487-512), which loses their INF entries, while
 * get_scaled_exp_params smooths the raw values (SMOOTH(-INF) -> weight 1).  ccj_amd/params/<set>.pfraw
 * holds them for the bundled sets. */
#define CCJ_PF_RAW_MAGIC 0x52434343u /* "CCCR" */
typedef struct ccj_pf_raw {
    uint32_t magic;
    uint32_t size_bytes; /* sizeof(ccj_pf_raw) */
    int32_t dangle5[8][5];
    int32_t dangle3[8][5];
    int32_t mismatchM[8][5][5];
    int32_t mismatchExt[8][5][5];
} ccj_pf_raw;

/* W_final_pf(seq, MFE_structure, MFE_energy, dangle, num_samples, PSplot) minus the arguments the
 * reference ignores (MFE_structure and PSplot are stored only; MFE_energy only feeds a pf_scale
 * that exp_params_rescale then forces to 1, part_func.cc:101-107).  prob->params are the 37 C
 * tables; raw = their unclamped dangle / mismatch tables (NULL: the blob's values with the pair
 * type 0 rows taken as INF, which every shipped set has).  device = HIP ordinal. */
int ccj_pf_create(const ccj_problem *prob, const ccj_pf_raw *raw, int device, ccj_pf_ctx **out);
void ccj_pf_destroy(ccj_pf_ctx *ctx);
/* The device bytes ccj_pf_create allocates for a sequence of length n (its up-front size check
 * compares them with the device's free memory), and the host bytes of the two window tables the
 * host builder (CCJ_PF_HOST_SETUP=1) forms before it uploads them. */
void ccj_pf_footprint(int n, unsigned long long *device_bytes, unsigned long long *host_bytes);

/* One context, many sequences — the semantics of ccj_create_cap / ccj_rebind / ccj_reset (ccj.h,
 * DESIGN.md §3.1) for the partition function.
 *
 * ccj_pf_create_cap allocates every buffer, event and pinned staging area for the largest demand
 * over the lengths 1..capacity and builds the context's key tables (once: the interior-loop and
 * stack weights by their arguments, host libm).  prob->seq (length <= capacity) is
 * bound at once; NULL binds poly-A of the capacity.  ccj_pf_create(prob) is
 * ccj_pf_create_cap(prob, strlen(prob->seq)): at n == capacity every offset and launch is that of
 * a context created for n.
 *
 * ccj_pf_rebind binds another sequence of any length 1..capacity: it recomputes the row stride, the
 * plane bases, the level descriptors and record bases, and rebuilds the per-sequence tables with
 * kernels on the context's stream (pt, est, the weight windows and masks, the k_pf_iloop items;
 * hp on the host, uploaded from pinned staging) with one wait (the item counts).  It allocates
 * nothing.  ccj_pf_reset is ccj_pf_rebind for a sequence of the bound length (another length is
 * CCJ_E_ARG).  A sequence longer than the capacity or with a character outside A/C/G/U/T is refused
 * with CCJ_E_ARG before the context is touched: the previous binding stays usable.  After either
 * call the context holds no fill (ccj_pf_W, ccj_pf_hashes, ccj_pf_sample ... return CCJ_E_STATE)
 * until ccj_pf_fill.  The parameters, dangles, penalties, noGU and the ccj_pf_srand state belong to
 * the context and stay.  A fill that ends in CCJ_E_PF_RANGE leaves the context able to take the
 * next sequence.  CCJ_PF_HOST_SETUP=1 (read at each call) builds the tables on the host with one
 * pow per entry instead, as before — the yardstick of the key tables. */
int ccj_pf_create_cap(const ccj_problem *prob, const ccj_pf_raw *raw, int device, int capacity, ccj_pf_ctx **out);
int ccj_pf_rebind(ccj_pf_ctx *ctx, const char *seq);
int ccj_pf_reset(ccj_pf_ctx *ctx, const char *seq);
int ccj_pf_capacity(const ccj_pf_ctx *ctx);
int ccj_pf_n(const ccj_pf_ctx *ctx); /* the bound length */
/* The one-time key-table build of this context: host milliseconds and device bytes. */
int ccj_pf_keytab_info(const ccj_pf_ctx *ctx, double *build_ms, unsigned long long *bytes);
/* FNV-1a of the bound sequence's setup tables as they stand on the device (cap >= 8): pt, est, hp,
 * the work items with their per-level firsts, then over the intervals whose pair can pair the
 * compacted 29 x 29 weights of ieO and ieI and the 29 mask words of mO and mI. */
int ccj_pf_setup_hashes(ccj_pf_ctx *ctx, uint64_t *out, int cap);
/* No GPU: the hashes (est, ieO, ieI, mO, mI as above) of a problem's tables built with one pow per
 * entry (direct5) and through the key tables and the gather functions the kernels share (keyed5). */
int ccj_pf_setup_host_hashes(const ccj_problem *prob, const ccj_pf_raw *raw, uint64_t *direct5, uint64_t *keyed5);

/* Lockstep batch — the partition function's ccj_batch (ccj.h): `members`
 * capacity contexts for the lengths 1..capacity whose fills run in ONE set of level launches, so a
 * set of short sequences pays the launch chain of its longest member once.
 *
 * ccj_pf_batch_create builds the Boltzmann tables and the key tables once and shares them among the
 * members (prob->seq may be NULL).  Its up-front size check compares members x
 * ccj_pf_footprint(capacity) plus the shared tables with the device's free memory (CCJ_E_OOM with a
 * message, before anything is allocated); members < 1 or capacity < 1 is CCJ_E_ARG.
 *
 * ccj_pf_batch_bind gives member k the sequence seqs[k] (1 <= count <= members, each of length
 * 1..capacity over A/C/G/U/T); the other members idle.  A bad argument is CCJ_E_ARG before any
 * member is touched: the previous binding stays usable.  The per-sequence setup is ccj_pf_rebind's,
 * enqueued for all members on the batch's stream with one host wait (the item counts of all
 * members).  After bind no member holds a fill.
 *
 * ccj_pf_batch_fill zeroes every member's sums in one launch, enqueues ccj_pf_fill's event graph once,
 * sized for the longest bound member, with each kernel launched once per level or span for all
 * members (k_pf_*_many; always the pushed P terms, CCJ_PF_PULL is not read), then per member copies
 * the 2-D planes back, runs the exactness check (CCJ_PF_RANGE_LOG2 as in ccj_pf_fill) and forms W and
 * the energy on the host.  A member whose check fails holds no fill: ccj_pf_batch_result gives
 * CCJ_E_PF_RANGE for it (ccj_pf_last_message on the member has the text); the other members are
 * untouched and the call still returns CCJ_OK.  A HIP error fails the whole call.
 *
 * ccj_pf_batch_member is borrowed: after a fill it is in the state ccj_pf_fill leaves, so ccj_pf_W,
 * _get2, _get4, _hashes, _exp_hashes, _setup_hashes, _srand, _sample, _n, _capacity and _work_model
 * work on it; its own ccj_pf_rebind, _reset, _fill and _set_timing return CCJ_E_STATE, and
 * ccj_pf_destroy ignores it.  ccj_pf_batch_launches: the kernel launches the last fill enqueued (the
 * zeroing launch and every k_pf_*_many launch of the graph); ccj_pf_batch_item_counts: each bound
 * member's k_pf_iloop items of level t (0 where it has no such level), what ccj_pf_level_plan_items
 * takes.  ccj_pf_batch_last_error(NULL): the message of the last failed create. */
typedef struct ccj_pf_batch ccj_pf_batch;
int ccj_pf_batch_create(const ccj_problem *prob, const ccj_pf_raw *raw, int device, int capacity, int members,
                        ccj_pf_batch **out);
int ccj_pf_batch_bind(ccj_pf_batch *b, const char *const *seqs, int count);
int ccj_pf_batch_fill(ccj_pf_batch *b);
int ccj_pf_batch_result(ccj_pf_batch *b, int k, double *energy);
ccj_pf_ctx *ccj_pf_batch_member(ccj_pf_batch *b, int k);
int ccj_pf_batch_members(const ccj_pf_batch *b);
int ccj_pf_batch_count(const ccj_pf_batch *b);
double ccj_pf_batch_fill_ms(const ccj_pf_batch *b);
int ccj_pf_batch_launches(const ccj_pf_batch *b);
int ccj_pf_batch_item_counts(const ccj_pf_batch *b, int t, int *out);
const char *ccj_pf_batch_last_error(const ccj_pf_batch *b);
void ccj_pf_batch_destroy(ccj_pf_batch *b);

/* The launch geometry of a fill, host only (no GPU).  With level t the fill's graph enqueues four
 * launches: k_pf_iloop(t+2), k_pf_level(t), k_pf_ppush(t), k_pf_diag(t+3); t = -3, -2, -1 are the
 * launches ahead of level 0 (the spans 0..2 and the iloops of levels 0 and 1), so t runs from -3 to
 * the longest member's last level max(n) - 3 (anything else, a length outside 1..1023 or count < 1
 * is CCJ_E_ARG).  For members of lengths n[count], out receives 12 + 12 * count ints: the grid
 * (x, y, z) of each of the four launches in that order, then per member the four grids that member
 * would launch alone.  {0,0,0} = no launch.  In a joint grid the member dimension (z for
 * k_pf_level, y for the others) is count and every other extent is the maximum over the members;
 * for count == 1 it is the single context's launch.  k_pf_iloop's extent depends on the sequence:
 * ccj_pf_level_plan_items takes each member's item count of level t+2 (ccj_pf_batch_item_counts);
 * without them (ccj_pf_level_plan) that family is reported as {-1,-1,-1} wherever the level exists. */
int ccj_pf_level_plan(const int *n, int count, int t, int *out);
int ccj_pf_level_plan_items(const int *n, const int *nitems, int count, int t, int *out);

/* ccj_pf(): the whole fill on the GPU, then W on the host.  *energy = to_Energy(W[n], n)
 * (part_func.cc:148-150,173). */
int ccj_pf_fill(ccj_pf_ctx *ctx, double *energy);

/* W[0..n] (n+1 doubles) after ccj_pf_fill. */
int ccj_pf_W(ccj_pf_ctx *ctx, double *W);

/* One 2-D matrix, canonical order i = 1..n, j = i..n (n(n+1)/2 doubles). */
int ccj_pf_get2(ccj_pf_ctx *ctx, int which, double *out);

/* One 4-D value with Matrix4DPF::get semantics (matrices.hh:258-263): 0 outside i <= j < k-1, k <= l. */
int ccj_pf_get4(ccj_pf_ctx *ctx, int which, int i, int j, int k, int l, int *out);

/* FNV-1a of every matrix in canonical order: h4[CCJ_PF_NMAT4] over the int32 values of the 4-D
 * matrices (i <= j < k-1, k <= l), h2[CCJ_PF_NMAT2] over the IEEE bits of the 2-D matrices. */
int ccj_pf_hashes(ccj_pf_ctx *ctx, uint64_t *h4, uint64_t *h2);

/* Hashes of the Boltzmann tables (names and order: ccj_pf_exp_names), for pinning against the
 * reference's scale_pf_parameters(). */
int ccj_pf_exp_hashes(ccj_pf_ctx *ctx, uint64_t *out, int cap);
const char *ccj_pf_exp_names(void); /* space-separated */
/* The same tables for a parameter blob without a context (no GPU needed). */
int ccj_pf_exp_hashes_params(const ccj_energy_params *params, const ccj_pf_raw *raw, const ccj_pk_penalties *pen,
                             uint64_t *out, int cap);

/* Stochastic traceback: nsamples times Sample_W(1, n) (stoch_backtrack.cc:36-85).  vrna_urn() of
 * the reference build is rand()/RAND_MAX (utils.c:262-271; its CMake defines no HAVE_ERAND48);
 * each context draws from its own glibc random_r state, which starts like a process that never
 * called srand() and is reseeded by ccj_pf_srand (= srand(seed)).  structures receives nsamples
 * NUL-terminated strings of n characters at stride n+1.  On a reference failure path (it prints
 * a line and calls exit(0)) that line is returned by ccj_pf_last_message() and the call returns
 * CCJ_E_PF_SAMPLE with *done = the samples completed before it. */
int ccj_pf_srand(ccj_pf_ctx *ctx, unsigned int seed);
int ccj_pf_sample(ccj_pf_ctx *ctx, int nsamples, char *structures, int *done);
const char *ccj_pf_last_message(ccj_pf_ctx *ctx);

/* Fill timing of the last ccj_pf_fill (ms, HIP events). */
int ccj_pf_timing(ccj_pf_ctx *ctx, float *fill_ms);
/* on != 0: the following fills record an event pair around every kernel launch (measurement only;
 * it adds the event cost to fill_ms).  ccj_pf_kernel_ms then gives the summed launch durations of
 * the last fill per family: [0] k_pf_iloop, [1] k_pf_level, [2] the P terms (k_pf_ppush; k_pf_pterm
 * with CCJ_PF_PULL=1), [3] k_pf_diag (0 when timing was off). */
int ccj_pf_set_timing(ccj_pf_ctx *ctx, int on);
int ccj_pf_kernel_ms(ccj_pf_ctx *ctx, double *ms4);
/* Algorithmic HBM bytes of one fill per kernel family (same order): the operands the
 * recurrences read and write, counted over this sequence's work items.  Host-side; the items and
 * masks are fetched from the device on the first call after a setup. */
int ccj_pf_work_model(ccj_pf_ctx *ctx, double *bytes4);

#ifdef __cplusplus
}
#endif

#endif /* CCJ_PF_H */
