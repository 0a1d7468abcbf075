/*
 * nyskoop.h -- C-ABI of libnyskoop.so: MI355X (gfx950) Nystrom-Koopman regression hot path.
 *
 * The reference (LCSL/nys-koop-lqr) has no FFI: its boundary is the Python class surface of
 * regressors.py.  Each entry point below names the reference interface it replaces (file:line into
 * /root/reference).  INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - All matrices are row-major float64 with an explicit leading dimension (in elements), so strided views
 *     such as X[:, :d] of an n x (d+p) array are passed without copying (regressors.py:52,142).
 *   - Every data pointer may be a HOST pointer or a DEVICE (HIP) pointer; the library detects which
 *     (hipPointerGetAttributes).  Host buffers are staged through HBM by the library; device buffers are used
 *     in place.  All buffers are caller-owned; the library never retains a caller pointer after return.
 *   - Return value: NK_OK (0) or a negative NK_ERR_* code; nk_last_error() gives a thread-local message.
 *     No exceptions or aborts cross the ABI.
 *   - One nk_ctx per (thread, device).  Calls on distinct contexts are re-entrant; a context is not
 *     thread-safe.  A context owns its HIP streams (nk_stream() returns the main one) and a grow-only HBM workspace.
 *   - There is NO CPU fallback: without a usable HIP device nk_create fails with NK_ERR_NO_DEVICE.
 */
#ifndef NYSKOOP_H
#define NYSKOOP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NK_ABI_VERSION 2

enum {
  NK_OK = 0,
  NK_ERR_BAD_ARG = -1,        /* NULL / negative size / lengthscale-dimension mismatch (sklearn ValueError) */
  NK_ERR_HIP = -2,            /* a HIP runtime call failed */
  NK_ERR_NOT_SPD = -3,        /* Cholesky met a non-positive pivot and strict mode is on (nk_set_strict_spd); by
                                 default the solve falls back to gelsd's rank-truncated minimum-norm solution */
  NK_ERR_OOM = -4,            /* HBM allocation failed */
  NK_ERR_NO_CONVERGENCE = -5, /* matrix square-root iteration did not converge */
  NK_ERR_NO_DEVICE = -6       /* no gfx950 device visible */
};

/* kernel families: regressors.py:15-22 (RBF, anisotropic), :24-26 (Matern nu=2.5), :28-30 (DotProduct), :225-233 (thin-plate
 * spline r^2 log(sqrt(r^2)), exactly 0 at r = 0; no length scale: n_lengthscale and lengthscale are ignored).  The spline
 * family is for nk_kernel_matrix and the spline fit (nk_spline_fit); the Nystrom entry points reject it. */
enum { NK_KERNEL_RBF = 0, NK_KERNEL_MATERN52 = 1, NK_KERNEL_LINEAR = 2, NK_KERNEL_TPS = 3 };

typedef struct nk_kernel_desc {
  int32_t type;              /* NK_KERNEL_* */
  int32_t d;                 /* state dimension the kernel acts on */
  int32_t n_lengthscale;     /* 1 (isotropic) or d (anisotropic); ignored for LINEAR and TPS */
  int32_t reserved;
  const double* lengthscale; /* HOST pointer, n_lengthscale entries */
  double sigma0;             /* LINEAR only: k(x,y) = x.y + sigma0^2 */
} nk_kernel_desc;

/* per-fit diagnostics, all times in milliseconds measured with HIP events on the context's stream */
typedef struct nk_fit_stats {
  double ms_total;     /* whole nk_nystrom_fit call, device side (main stream, first to last event) */
  double ms_upload;    /* host->HBM staging and K(Z,Z) (0 when inputs are device pointers) */
  double ms_kmat;      /* the two n x m kernel blocks (of the first pass when the rows are processed in passes) */
  double ms_gram;      /* the fused Gram launch (+ kernel blocks and Gram launches of later passes) */
  double ms_sqrt;      /* matrix square root of K_mm on the side stream; OVERLAPS the factorisation chain */
  double ms_solve;     /* operator products after the two streams join (the factorisations and substitutions run
                          between ms_gram and this stage, concurrently with ms_sqrt) */
  double ms_gram_kernel_avg; /* average duration of one fused Gram launch (HIP events around the kernel) */
  int32_t gram_kernel_launches;
  int32_t sqrt_iters;
  double sqrt_residual;      /* ||X^T X - I||_F / sqrt(m) at the last convergence check (< 1e-7; the returned
                                square root is one quadratically convergent step beyond that iterate) */
  double gram_flops;         /* algorithmic flop of the Gram contractions actually issued */
  double kmat_pairs;         /* number of (row,row,dim) triples evaluated by the kernel-matrix builds */
  /* numerical rank used for the two regularised systems (regressors.py:155,165): m+p and m when the Cholesky
   * factorisations succeeded (full rank), otherwise the number of singular values kept by the pseudo-inverse path -- what
   * scipy.linalg.lstsq (gelsd) reports as `rank` */
  int32_t rank_inner;
  int32_t rank_inner_rec;
  /* smallest / largest Cholesky pivot of the two regularised systems (0 when the factorisation failed); below the
   * threshold of nk_set_refine (off by default) the solve is refined with doubled-precision residuals while the corrections contract;
   * `refined` = steps applied to inner + 16 x steps applied to inner_rec (0 = none); refine_ratio_* = |first correction| /
   * |solution| (an estimate of cond x backward error of the factor; the first step is applied when it is <= 1/4) */
  double pivot_ratio_inner;
  double pivot_ratio_inner_rec;
  int32_t refined;
  int32_t reserved_;
  double refine_ratio_inner;
  double refine_ratio_inner_rec;
} nk_fit_stats;

typedef struct nk_ctx nk_ctx;
typedef struct nk_model nk_model;

/* ---- library / context ------------------------------------------------------------------------------ */
int nk_version(void);
const char* nk_last_error(void);
int nk_device_count(void);
int nk_create(int device, nk_ctx** out);
int nk_destroy(nk_ctx* ctx);
int nk_synchronize(nk_ctx* ctx);
/* the hipStream_t all work of this context is launched on (for event timing by the caller) */
void* nk_stream(nk_ctx* ctx);
/* how nk_nystrom_fit builds the two n x m kernel blocks: 0 = automatic (Gram form |a|^2+|b|^2-2ab on the MFMA engine
 * when d >= 32, direct differences otherwise), 1 = always direct differences like scipy cdist (regressors.py:141-142
 * -> sklearn -> cdist).  K(Z,Z), lift queries and nk_kernel_matrix always use direct differences (nk_kernel_matrix of
 * NK_KERNEL_TPS excepted).  nk_spline_fit builds its two blocks the same way.
 * Also settable with the environment variable NYSKOOP_KMAT=direct before nk_create. */
int nk_set_kmat_mode(nk_ctx* ctx, int mode);
/* Rank-deficient regularised systems.  scipy.linalg.lstsq (regressors.py:155,165; LAPACK gelsd, rcond = eps) silently
 * returns the minimum-norm solution with singular values <= eps * sigma_max dropped.  By default (strict = 0) the library
 * does the same -- a one-sided Jacobi SVD on the device with the same cut-off -- whenever its Cholesky factorisation meets
 * a non-positive pivot or an isolated cluster of rounding-level pivots (<= 8 order eps d_max, separated from the other pivots
 * by a factor 1000: an exact null space), i.e. a matrix that is singular to working precision.  (A system whose Cholesky succeeds with healthy pivots is solved at full rank even if its singular values
 * reach below eps * sigma_max: there gelsd's rank decision is taken inside its own rounding noise and no two solvers
 * agree on it -- DESIGN.md section 3.)  strict = 1 turns the fallback into NK_ERR_NOT_SPD (also: environment variable
 * NYSKOOP_STRICT_SPD=1 before nk_create; the variable takes 0, 1 or 2 and nk_create refuses any other value).  strict = 2 is the lstsq-shaped mode: BOTH regularised systems of every fit go
 * through the SVD and are cut at eps * sigma_max exactly as gelsd cuts -- 10-50 x slower for small fits and, on the
 * ill-conditioned candidates it was asked for, no closer to the reference than the default (profiles/r03_cloth_units.txt);
 * kept for callers who want lstsq's rank rule whatever it costs. */
int nk_set_strict_spd(nk_ctx* ctx, int strict);
/* Optional refinement of the two regularised solves of a fit (regressors.py:155,165).  The blocked Cholesky solve is
 * backward stable (every product with an inverted diagonal block takes a correction step from the data); a system whose
 * smallest / largest pivot is below `pivot_ratio` can in addition be refined `steps` times with residuals accumulated in
 * doubled precision, which returns the system's own solution to working precision whatever its condition (as long as
 * cond x eps < 1/4: a step is applied only while the corrections contract).  pivot_ratio = 0 (default; also the
 * environment variable NYSKOOP_REFINE_PIVOT before nk_create) = never.  nk_fit_stats.refined / refine_ratio_* report it. */
int nk_set_refine(nk_ctx* ctx, double pivot_ratio, int32_t steps);
/* Arithmetic of the two O(n m d) kernel blocks and the O(n m^2) Gram contractions of nk_nystrom_fit / nk_nystrom_gram
 * (regressors.py:141-142,151,153,162,164).  NK_DTYPE_F64 (default): fp64 end to end, the only mode that meets the 1e-6
 * operator bar.  NK_DTYPE_F32 (the stress configuration of BASELINE.json: n = 1e6, m = 8000, d = 1024, "fp32"): rows and
 * kernel values are rounded to fp32 and multiplied on the fp32 matrix pipe (twice the fp64 rate, half the bytes); the
 * Gram accumulators are kept in fp64 (fp32 partial sums never run over more than 32 rows) and everything m x m --
 * regularised solves, square root, operators, lift, predict, rollouts -- stays fp64.  Needs d >= 32 and shared input /
 * output landmarks; contexts of a lock-step group ignore it. */
#define NK_DTYPE_F64 0
#define NK_DTYPE_F32 1
int nk_set_compute_dtype(nk_ctx* ctx, int dtype);
/* Stream ordering for DEVICE-pointer arguments: work already queued on `producer_stream` (a hipStream_t; NULL = the
 * legacy default stream) is ordered before everything this context launches afterwards -- an event recorded on the
 * producer stream that all of the context's streams wait for; the host does not block.  Call it before handing the
 * library a device buffer that another stream is still writing (a torch tensor that is the output of a pending
 * all-reduce, for example): the context's streams are non-blocking and do not synchronise with any other stream
 * implicitly.  Results are complete when a call returns (every entry point synchronises its streams before returning
 * unless documented otherwise), so no ordering is needed in the other direction. */
int nk_wait_stream(nk_ctx* ctx, void* producer_stream);
/* ---- lock-step groups: batched execution of many SMALL fits (the (candidate, fold) units of the hyper-parameter sweep,
 * benchmark_lqr_cloth.py:39-66; multi-seed sweeps :168-203).  One small fit is a chain of a few hundred launch-bound
 * kernels that leaves the chip idle; a group runs `size` of them in lock step.  nk_group_create returns `size` member
 * contexts; each is driven by its own host thread through the ordinary entry points (nk_nystrom_fit, nk_spline_fit,
 * nk_score_neg_rmse, ...).  Inside the library a member's launches are recorded, and whenever members wait for the
 * device the recorded sequences are merged -- equal launches become one launch with blockIdx.z = member -- and issued
 * on one shared stream.  Results are bit-identical to an ordinary context (same kernels, same arguments).
 * nk_group_enter / nk_group_leave bracket a unit of work of one member: members inside a unit wait for one another at
 * their synchronisation points; a member outside a unit never blocks the others (its calls still work, unbatched).
 * Enter all members that take part in a round before any of them starts (any thread may call nk_group_enter).
 * Destroy the members with nk_destroy; the group goes with its last member.
 * nk_group_stats: {flushes, merged launches, single launches, member-launches covered by merged launches}. */
int nk_group_create(int device, int size, nk_ctx** members);
/* ---- the hyper-parameter sweep as ONE call: replaces the fit/predict/score loop GridSearchCV runs over (candidate, fold)
 *   units (benchmark_lqr_cloth.py:52-65 and the classic / hjb twins; sklearn: clone -> fit(X_train, Y_train) ->
 *   'neg_root_mean_squared_error' on the held-out fold).  Unit u fits on all rows of X, Y except [test_begin, test_end)
 *   with the landmarks Y[landmark_rows[0..m)] (rows of the DATA SET, i.e. after mapping training-row indices past the
 *   fold) and scores the held-out rows.  `members`: the contexts of ONE lock-step group (nk_group_create); the units are
 *   run n_members at a time, one host thread per member inside the library, their kernel launches merged.
 *   X: n x (d+p), Y: n x d (host or device).  scores[u] = the unit's score; status[u] = NK_OK or the error code of a
 *   unit whose fit failed (its score is NaN, like GridSearchCV's error_score=nan). ------------------------------------ */
typedef struct nk_cv_unit {
  const nk_kernel_desc* kernel;
  double gamma;
  double jitter;
  int32_t m;
  int32_t reserved;
  int64_t test_begin, test_end;
  const int64_t* landmark_rows; /* m row indices into Y */
} nk_cv_unit;
int nk_cv_grid(nk_ctx* const* members, int32_t n_members, const double* X, int64_t ldx, const double* Y, int64_t ldy,
               int64_t n, int32_t d, int32_t p, const nk_cv_unit* units, int32_t n_units, double* scores, int32_t* status);
/* The same sweep for the thin-plate-spline estimator (nk_spline_fit; benchmark_lqr_classic.py:55-60: GridSearchCV over
 * KoopmanSplineRegressor).  Unit u fits on all rows but [test_begin, test_end) with its own centres and scores the held-out
 * rows.  The centres are VALUES (m x d rows, dense, host memory), not row indices: the reference draws them from the state
 * bounds (regressors.py:189-193) or from columns of the training states (:195-197), and the first kind are rows of nothing.
 * Checked before any unit runs: pointers, sizes, folds; a unit's gamma is checked by its own fit (status[u] =
 * NK_ERR_BAD_ARG, scores[u] = NaN).  Two phases as in nk_cv_grid: the units whose system takes the pseudo-inverse (pivot
 * ratio inside the window described at nk_spline_fit) stop there in the first phase and are run together in the second,
 * where their Jacobi sweeps can merge (by construction, as in nk_cv_grid; the gain of the second phase has not been
 * measured for spline units).  The scores do not depend on the schedule, and are the bits of nk_spline_fit +
 * nk_score_neg_rmse on an ordinary context. */
typedef struct nk_spline_cv_unit {
  double gamma;
  int32_t m;
  int32_t reserved;
  int64_t test_begin, test_end;
  const double* centers; /* HOST pointer, m x d rows, dense */
} nk_spline_cv_unit;
int nk_spline_cv_grid(nk_ctx* const* members, int32_t n_members, const double* X, int64_t ldx, const double* Y,
                      int64_t ldy, int64_t n, int32_t d, int32_t p, const nk_spline_cv_unit* units, int32_t n_units,
                      double* scores, int32_t* status);
/* ---- the multi-seed system-identification sweep as ONE call: replaces the loops of benchmark_lqr_classic.py:211-255 and
 *   benchmark_lqr_cloth.py:163-211 (for each seed and each m: draw, fit, validate_dyn_sys on the test trajectories).  Unit u
 *   fits on the rows `row_ranges` of the shared data set X, Y -- a Nystrom fit with the landmarks Y[landmark_rows[0..m)]
 *   when `kernel` is set, a thin-plate-spline fit with `centers` (m x d VALUES, host memory) when it is NULL -- and scores
 *   the test trajectories trajs[traj[0..n_traj)] with nk_rollout_err.  One call may hold units of both estimators.
 *   trajs: n_trajs x T x d, U: n_trajs x T x p (row T-1 never read), host or device; uploaded once, like the data set.
 *   err_abs / err_rel (either may be NULL): flat, unit-major -- unit u starts at the sum of n_traj over the units before it.
 *   status[u] = NK_OK or the unit's error code (all its entries are NaN then).  Checked before any unit runs: pointers,
 *   sizes, m <= 4096, landmark rows, row ranges and trajectory indices; a unit's gamma is checked by its own fit.  Two
 *   phases as in nk_cv_grid / nk_spline_cv_grid (units that take the rank-truncating / pseudo-inverse branch run together
 *   afterwards).  The results do not depend on the schedule: they are the bits of nk_nystrom_fit / nk_spline_fit +
 *   nk_rollout_err on an ordinary context. */
typedef struct nk_sysid_unit {
  const nk_kernel_desc* kernel;   /* NULL: a spline unit (nk_spline_fit), `centers` used; else nk_nystrom_fit */
  double gamma, jitter;
  int32_t m, n_ranges;
  const int64_t* row_ranges;      /* training rows of the shared data set, as in nk_nystrom_fit; NULL = all */
  const int64_t* landmark_rows;   /* Nystrom: m rows of Y */
  const double* centers;          /* spline: HOST, m x d dense */
  const int32_t* traj;            /* indices into the call's test trajectories */
  int32_t n_traj, reserved;
} nk_sysid_unit;
int nk_sysid_grid(nk_ctx* const* members, int32_t n_members, const double* X, int64_t ldx, const double* Y, int64_t ldy,
                  int64_t n, int32_t d, int32_t p, const double* trajs, const double* U, int32_t n_trajs, int32_t T,
                  const nk_sysid_unit* units, int32_t n_units, double* err_abs, double* err_rel, int32_t* status);
int nk_group_enter(nk_ctx* member);
int nk_group_leave(nk_ctx* member);
int nk_group_stats(nk_ctx* member, uint64_t* out4);
/* Process-wide counters of the slow paths that are otherwise silent (they cost time, never correctness):
 *   out[0] single-launch lifted recursions (nk_rollout / nk_closed_loop*, 128 < m <= 2048) that gave up waiting for a
 *          workgroup that was not resident and were repeated with one launch per step (5-10x slower);
 *   out[1] single-launch Jacobi sweeps (rank-truncating branch of the fit inside a lock-step group) that gave up the
 *          same way and finished with one launch per round;
 *   out[2] fits whose regularised system(s) took the rank-truncating branch (regressors.py:155,165: lstsq / gelsd);
 *   out[3] fits that repeated the matrix square root with the factorisation-free iteration;
 *   out[4] fits whose regularised solves were refined with doubled-precision residuals (nk_set_refine).
 * Three more slots say which implementation of the augmented blocked Cholesky ran (diagnostics, not slow paths as such):
 *   out[5] tile-dataflow Cholesky launches that gave up waiting (the caller re-ran the launch-per-step chain);
 *   out[6] tile-dataflow Cholesky launches issued (every call whose systems all have m >= 256, on an ordinary context);
 *   out[7] launch-per-step chains that ran with look-ahead (NYSKOOP_CHOL_LOOKAHEAD=1, >= 4 blocks, main stream, no group).
 * n = number of entries the caller provides (<= 8 are written). */
int nk_runtime_counters(uint64_t* out, int32_t n);
/* Releases everything the library still holds on every device -- live contexts (their streams, events and workspaces),
 * live models, the model-buffer pool and page-locked host blocks -- after waiting for pending work.  Handles that were
 * live become invalid; destroying them afterwards is a harmless no-op, so language bindings may call this from an
 * exit hook that runs BEFORE the HIP runtime's own static destructors and keep their finalisers.  Idempotent. */
int nk_shutdown(void);

/* page-locked host memory for result arrays (device->host copies into it run at the PCIe rate and skip first-touch
 * page faults); nk_host_free(NULL) is a no-op. */
void* nk_host_alloc(uint64_t bytes);
void nk_host_free(void* ptr);

/* ---- kernel matrix: replaces `kern.kernel(A, B)` (regressors.py:22,26,30 -> sklearn RBF/Matern/DotProduct
 *      __call__): out[i][j] = k(A[i,:], B[j,:]),  A: nA x d, B: nB x d, out: nA x nB.  Direct differences, except for
 *      NK_KERNEL_TPS, which follows nk_set_kmat_mode like the kernel blocks of nk_spline_fit (Gram form at d >= 32 in
 *      the automatic mode: r^2 carries a cancellation error of about eps (|a|^2 + |b|^2) after centring on the mean of
 *      B, so coincident points give values of that order times |log r^2| instead of exact zeros). ------------------ */
int nk_kernel_matrix(nk_ctx* ctx, const nk_kernel_desc* kd,
                     const double* A, int64_t lda, int64_t nA,
                     const double* B, int64_t ldb, int64_t nB,
                     double* out, int64_t ldo);

/* ---- landmark selection (beyond the reference, which draws landmarks uniformly at random, regressors.py:129-132): m
 *   steps of partial pivoted Cholesky of K(Y, Y) over the CANDIDATE rows -- all n rows, or the rows of row_ranges
 *   concatenated in the order given, as the fits gather them ([begin,end) pairs as in nk_nystrom_fit; empty ranges are
 *   dropped; n_c = number of candidates).  Y: n x d, host or device.  The state is the residual diagonal
 *   dg_i = k(y_i, y_i) and a factor F (n_c x m, a dedicated HBM allocation of 8 n_c m bytes that is released before the
 *   call returns, never part of the context's workspace; NK_ERR_OOM when it does not fit).  Step j = 0 .. m-1:
 *     pick    NK_LANDMARK_GREEDY: the candidate with the largest dg; equal values go to the LOWEST candidate position
 *             (ties are real: far-apart points leave many residuals at exactly 1).  NK_LANDMARK_RPCHOLESKY: with
 *             T = sum dg, the smallest position whose inclusive prefix sum of dg exceeds u[j] * T (a position with
 *             dg == 0 is never picked; should rounding let no prefix exceed it, the last position with dg > 0).
 *     record  out_resid[j] = dg[piv] and out_trace[j] = T (the sum of dg before the step).
 *     stop    if dg[piv] <= tol * dg0max (dg0max = the largest initial diagonal entry) or dg[piv] <= 0 the selection ends
 *             with *m_selected = j: the residual at which a landmark is picked is the squared Cholesky pivot of K_mm at
 *             that landmark, so tol > 0 stops before K_mm becomes singular to working precision.
 *     column  c_i = k(y_i, y_piv) - sum_{l<j} F[i,l] F[piv,l], F[i,j] = c_i / sqrt(dg[piv]),
 *             dg_i = max(dg_i - F[i,j]^2, 0), dg[piv] = 0 exactly.
 *   Summation orders, all fixed by the inputs alone (no atomics; the result does not depend on the launch geometry):
 *   kernel values from direct differences (dot products for LINEAR) of the pre-scaled coordinates, accumulated over
 *   k in four partial sums (k mod 4) combined as (a0 + a1) + (a2 + a3); the sum over l < j likewise in four partial sums
 *   (l mod 4) in increasing l; T and the prefix sums: blocks of 256 consecutive candidate positions are summed by a halving
 *   tree (entry t + entry t + s for s = 128, 64, .. 1), the block sums are added in index order, and inside the block
 *   that holds the pick dg is added in index order on top of the prefix before that block.
 *   Kernel families: RBF (isotropic or anisotropic), MATERN52, LINEAR.  NK_KERNEL_TPS is rejected: the thin-plate spline
 *   is not positive semi-definite (its diagonal is 0), so it has no Cholesky factor.
 *   The selection is nested: the rows for m are the first m rows for any larger m (same u prefix, same tol).
 *   out_rows (HOST, m): rows of Y in pick order, -1 from entry *m_selected on.  out_resid (HOST, m, may be NULL): entry
 *   *m_selected, if there is one, is the residual that fired the stop rule, later entries are 0.  out_trace (HOST, m + 1,
 *   may be NULL): entry *m_selected is the trace left, tr(K - K_nm K_mm^-1 K_mn) over the candidates; later entries are 0.
 *   u: HOST, m numbers in [0, 1), read for NK_LANDMARK_RPCHOLESKY only (may be NULL for GREEDY).
 *   Everything is checked before anything is queued: 1 <= m <= min(n_c, 4096), d <= 2048, tol finite and >= 0, the rule,
 *   u, the kernel family and its dimension, the ranges inside [0, n]; a failed check is NK_ERR_BAD_ARG and no output is
 *   written.  All 2m + 1 launches are queued without a host round trip and one copy brings the results back.  Ordinary
 *   contexts only (not lock-step members). ------------------------------------------------------------------------- */
#define NK_LANDMARK_GREEDY 0
#define NK_LANDMARK_RPCHOLESKY 1
int nk_select_landmarks(nk_ctx* ctx, const nk_kernel_desc* kd, const double* Y, int64_t ldy, int64_t n, int32_t d,
                        const int64_t* row_ranges, int32_t n_ranges, int32_t rule, const double* u, int32_t m, double tol,
                        int64_t* out_rows, double* out_resid, double* out_trace, int32_t* m_selected);

/* ---- fit: replaces KoopmanNystromRegressor.fit given landmarks (regressors.py:136-169).
 *   X: n x (d+p) rows [state | input] (the array the reference's fit(X, Y) receives), Y: n x d.
 *   row_ranges: optional 2*n_ranges int64 [begin,end) pairs selecting the training rows (K-fold training
 *     sets are two contiguous ranges, benchmark_lqr_cloth.py:52-65); NULL = all n rows.
 *   Zin / Zout: m x d landmark rows (nystrom_centers_input/_output transposed; regressors.py:129-134);
 *     Zin may be NULL or equal to Zout (the reference's default, :133-134).
 *   gamma, jitter: regressors.py:127,120.   The fitted operators live in *model (device resident). ------ */
int nk_nystrom_fit(nk_ctx* ctx, const nk_kernel_desc* kd,
                   const double* X, int64_t ldx, const double* Y, int64_t ldy,
                   int64_t n, int32_t d, int32_t p,
                   const int64_t* row_ranges, int32_t n_ranges,
                   const double* Zin, int64_t ldzi, const double* Zout, int64_t ldzo, int32_t m,
                   double gamma, double jitter,
                   nk_model** model, nk_fit_stats* stats);

/* ---- the same fit split at its one exchange point, for SAMPLE-SHARDED fits over several GPUs: every
 *   rank holds all landmarks and a slice of the rows, accumulates the four Gram blocks of its rows with nk_nystrom_gram
 *   (regressors.py:151,153,162,164 without the regularisers), the packed accumulators are summed over the ranks (one
 *   all-reduce of nk_gram_doubles(m,d,p) doubles: 102 MB at m=2000, d=384), and nk_nystrom_solve finishes the fit from the
 *   sum (n_total = number of rows over all ranks, regressors.py:127).  gram: host or device memory; layout
 *   [G1 (m+p)x(m+p) ; G2 m x (m+p)] row-major, then at the next even offset [G3 m x m ; G4 d x m].
 *   nk_nystrom_gram followed by nk_nystrom_solve on one rank equals nk_nystrom_fit. ----------------------------------- */
int nk_gram_doubles(int32_t m, int32_t d, int32_t p, int64_t* count);
int nk_nystrom_gram(nk_ctx* ctx, const nk_kernel_desc* kd,
                    const double* X, int64_t ldx, const double* Y, int64_t ldy,
                    int64_t n, int32_t d, int32_t p,
                    const int64_t* row_ranges, int32_t n_ranges,
                    const double* Zin, int64_t ldzi, const double* Zout, int64_t ldzo, int32_t m,
                    double* gram, nk_fit_stats* stats);
int nk_nystrom_solve(nk_ctx* ctx, const nk_kernel_desc* kd,
                     const double* Zin, int64_t ldzi, const double* Zout, int64_t ldzo, int32_t m, int32_t d, int32_t p,
                     const double* gram, int64_t n_total, double gamma, double jitter,
                     nk_model** model, nk_fit_stats* stats);

/* rebuild a device model from host copies (un-pickling a regressor, benchmark_lqr_cloth.py:266-267 /
 * closed_loop_lqr_control.m:158-161); recomputes K_mm^{-1/2} from the landmarks once. A,B,C,W may be NULL. */
int nk_model_create(nk_ctx* ctx, const nk_kernel_desc* kd, const double* Zout, int64_t ldz,
                    int32_t m, int32_t d, int32_t p, double jitter,
                    const double* A, const double* B, const double* C, const double* W,
                    nk_model** model);
int nk_model_destroy(nk_model* model);

/* ---- thin-plate-spline EDMD: replaces KoopmanSplineRegressor.fit given its centres (regressors.py:199-221, the Korda-Mezic
 *   baseline).  X: n x (d+p) rows [state | input], Y: n x d, row_ranges as in nk_nystrom_fit; centers: m x d rows (the
 *   reference's `centers`, d x m, transposed).  With Phi_x = TPS(X_state, centres), Phi_y = TPS(Y, centres) (n x m blocks)
 *   and P = [Phi_x U]^T [Phi_x U] + gamma n_train I:  M_ls = [Phi_y^T ; X_state^T] [Phi_x U] pinv(P),  A = M_ls[:m, :m],
 *   B = M_ls[:m, m:], C = M_ls[m:, :m], W = C [A B].  pinv follows scipy.linalg.pinv (singular values <= (m+p) eps
 *   sigma_max dropped); systems whose Cholesky pivots show they cannot come near that cut-off are solved by the blocked
 *   Cholesky instead.  stats->rank_inner = singular values kept (m+p on the Cholesky path), rank_inner_rec = 0,
 *   pivot_ratio_inner = smallest / largest Cholesky pivot whenever the factorisation succeeded, also when the ratio then
 *   sent the system to the pseudo-inverse (0 when it failed or, with strict_spd = 2, was not run).  fp64 only: the compute dtype of
 *   nk_set_compute_dtype is ignored (the fit runs in fp64).  strict_spd (nk_set_strict_spd): 1 = a non-positive pivot
 *   is NK_ERR_NOT_SPD, 2 = always the pseudo-inverse.  Members of a lock-step group may call it (same bits as on an
 *   ordinary context; stats may be NULL, the ms_* fields are 0 there; nk_spline_cv_grid is the sweep).  The model is a spline
 *   model: its lift is the raw block TPS(x, centres) (no K_mm^{-1/2}); nk_lift, nk_predict, nk_score_neg_rmse,
 *   nk_rollout, nk_closed_loop(_batch), nk_model_get ('S' / 'I': NK_ERR_BAD_ARG) and nk_model_get_ops accept it. */
int nk_spline_fit(nk_ctx* ctx, const double* X, int64_t ldx, const double* Y, int64_t ldy, int64_t n, int32_t d, int32_t p,
                  const int64_t* row_ranges, int32_t n_ranges, const double* centers, int64_t ldc, int32_t m, double gamma,
                  nk_model** model, nk_fit_stats* stats);
/* rebuild a spline model from host copies (un-pickling); A, B, C, W as in nk_model_create (W may be NULL). */
int nk_spline_model_create(nk_ctx* ctx, const double* centers, int64_t ldc, int32_t m, int32_t d, int32_t p,
                           const double* A, const double* B, const double* C, const double* W, nk_model** model);

/* which: 'A' m x m, 'B' m x p, 'C' d x m, 'W' d x (m+p), 'S' m x m (K_mm^{1/2}), 'I' m x m (K_mm^{-1/2}),
 *        'Z' m x d landmarks.   regressors.py:158-159,166,169. */
int nk_model_get(nk_ctx* ctx, const nk_model* model, char which, double* out, int64_t ldo);
int nk_model_dims(const nk_model* model, int32_t* m, int32_t* d, int32_t* p);
/* all fitted operators in one call: G = [A B] (m x (m+p), the layout of regressors.py:157-159), C and W, copied
 * concurrently on the context's streams (two DMA engines) when the outputs are host buffers.  Any of the three output
 * pointers may be NULL. */
int nk_model_get_ops(nk_ctx* ctx, const nk_model* model, double* G, int64_t ldg, double* C, int64_t ldc, double* W,
                     int64_t ldw);
/* the same without waiting: returns once the copies are queued on the context's copy stream, so that they overlap with
 * whatever the caller launches next (page-locked destination buffers, see nk_host_alloc, are needed for a true
 * overlap).  The destinations must not be read before nk_model_wait(model) has returned; nk_model_destroy waits by
 * itself.  One fetch per model is in flight at a time. */
int nk_model_get_ops_async(nk_ctx* ctx, nk_model* model, double* G, int64_t ldg, double* C, int64_t ldc, double* W,
                           int64_t ldw);
int nk_model_wait(nk_model* model);

/* ---- lift: replaces KoopmanNystromRegressor.lift (regressors.py:171-178) with K_mm^{-1/2} cached.
 *   Xq: nq x d query rows; out: nq x m (row i = phi(x_i); the reference returns the transpose, m x nq). ---- */
int nk_lift(nk_ctx* ctx, const nk_model* model, const double* Xq, int64_t ldx, int64_t nq,
            double* out, int64_t ldo);

/* ---- predict: replaces KoopmanRegressor.predict (regressors.py:48-55). Xaug: nq x (d+p); out: nq x d. -- */
int nk_predict(nk_ctx* ctx, const nk_model* model, const double* Xaug, int64_t ldx, int64_t nq,
               double* out, int64_t ldo);

/* ---- CV score: sklearn scorer 'neg_root_mean_squared_error' on a held-out block
 *      (benchmark_lqr_cloth.py:55): -(mean over columns of sqrt(mean over rows of (Y - predict(X))^2)). ---- */
int nk_score_neg_rmse(nk_ctx* ctx, const nk_model* model, const double* Xaug, int64_t ldx,
                      const double* Ytrue, int64_t ldy, int64_t nq, double* score);

/* ---- open-loop rollout: replaces the loop of validate_dyn_sys (benchmark_lqr_cloth.py:23-32) for a batch
 *   of trajectories.  x0: batch x d initial states; U: batch x T x p controls (row t of trajectory b at
 *   U + (b*T + t)*p); out_x: batch x T x d with out_x[b][0] = C lift(x0_b), out_x[b][t+1] = C(A z_t + B u_t);
 *   out_z (optional, may be NULL): batch x T x m lifted states. ------------------------------------------ */
int nk_rollout(nk_ctx* ctx, const nk_model* model, const double* x0, int64_t ldx0,
               const double* U, int32_t T, int32_t batch, double* out_x, double* out_z);

/* ---- open-loop validation error: validate_dyn_sys (benchmark_lqr_cloth.py:18-36, _classic.py:23-41) for `batch` trajectories,
 *   reduced on the device: the simulated trajectory C z_t is never written, two sums per trajectory come back.
 *   x0 = row 0 of each true trajectory.  traj: batch x T x d, U: batch x T x p (row T-1 never read), host or device.
 *   err_abs[b] = sqrt(sse / (d T)), err_rel[b] = 100 sqrt(sse) / sqrt(ssim) with sse = sum (x_true - C z)^2 and
 *   ssim = sum (C z)^2 over the T x d entries; either output (HOST arrays of `batch` doubles) may be NULL.  Same staging and
 *   recursion as nk_rollout (the lifted states are the same bits); the sums are taken in a fixed order, so a trajectory's
 *   result does not depend on `batch`.  Nystrom and spline models, m <= 4096, batch <= 65535; ordinary contexts and
 *   lock-step group members. */
int nk_rollout_err(nk_ctx* ctx, const nk_model* model, const double* traj, const double* U, int32_t T, int32_t batch,
                   double* err_abs, double* err_rel);

/* ---- closed loop in lifted space: replaces the loop of lqr_control (benchmark_lqr_cloth.py:79-84).
 *   K: p x m gain; phi0, phi_ref: m-vectors; out_x: steps x d visited states C phi_t; out_u: steps x p. ---- */
int nk_closed_loop(nk_ctx* ctx, const nk_model* model, const double* K, const double* phi0,
                   const double* phi_ref, int32_t steps, double* out_x, double* out_u);
/* the same for `batch` independent loops that share the gain: phi0, phi_ref: batch x m; out_x: batch x steps x d;
 * out_u: batch x steps x p (multi-seed / multi-reference sweeps of benchmark_lqr_cloth.py:212-270). */
int nk_closed_loop_batch(nk_ctx* ctx, const nk_model* model, const double* K, const double* phi0,
                         const double* phi_ref, int32_t steps, int32_t batch, double* out_x, double* out_u);
/* ---- closed loop around the TRUE plant: replaces the loop of lqr_control in benchmark_lqr_hjb.py:73-97 and
 *   benchmark_lqr_classic.py:67-89 for the reference's three plants (dynamical_systems.py), which the library restates
 *   as closed-form maps: one Runge-Kutta step of length Ts in the reference's order of operations, with its k4 evaluated
 *   at x + k1 Ts, in plain IEEE arithmetic (the host and the device build of a plant give the same bits).
 *   NK_PLANT_DUFFING: d = 2, f = (x2, -0.5 x2 - x1 (4 x1^2 - 1) + 0.5 u); NK_PLANT_DOUBLE_INTEGRATOR: d = 2, f = (x2, u);
 *   NK_PLANT_HJB: d = 1, f = -x^3 + u.  Every plant has one input.
 *   nk_plant_step: x_next = plant(x, u) on the HOST (x, x_next: d doubles, u: one double; no context, no GPU needed).
 *   nk_plant_loop: `batch` independent loops u_t = K (phi(x_ref) - phi(x_t)), x_{t+1} = plant(x_t, u_t) for t < steps in
 *   ONE launch, one workgroup per loop, phi = the model's lift.  K: 1 x m gain; x0, x_ref: batch x d (dense);
 *   out_x: batch x (steps + 1) x d visited states, row 0 = x0; out_u: batch x steps x 1 controls.  Host or device
 *   pointers.  The gain is folded into the lift once per call (w = K_mm^{-1/2} K^T, u_t = sum_j w_j (k(z_j, x_ref) -
 *   k(z_j, x_t))), so u_t agrees with K times the difference of two nk_lift results to rounding, not bit for bit; a
 *   loop's results do not depend on `batch`.  Needs a Nystrom model with an RBF, Matern-5/2 or linear kernel or a
 *   spline model, p = 1, d = the plant's state dimension and m <= 4096 (NK_ERR_BAD_ARG otherwise); fitted operators
 *   are not needed.  Not available to lock-step group members. */
#define NK_PLANT_DUFFING 0
#define NK_PLANT_DOUBLE_INTEGRATOR 1
#define NK_PLANT_HJB 2
int nk_plant_step(int plant, double Ts, const double* x, const double* u, double* x_next);
int nk_plant_loop(nk_ctx* ctx, const nk_model* model, int plant, double Ts, const double* K, const double* x0,
                  const double* x_ref, int32_t steps, int32_t batch, double* out_x, double* out_u);
/* ---- the multi-model form of nk_plant_loop, scored on the device: the control branch of the sweeps of
 *   benchmark_lqr_classic.py:256-299 and benchmark_lqr_hjb.py:265-333 (per seed and m: fit, gain, closed loop, replay and
 *   cost, control RMSE) in ONE call after the fits.  Every unit has its own model, gain, initial state and reference;
 *   the units of a call share the plant, Ts and steps and may differ in everything else (model kind, kernel family, m).
 *   Unit u runs exactly the loop of nk_plant_loop(model, K, x0, x_ref, batch = 1): its states and controls have the same
 *   bits, whatever else the call holds and in whatever order.
 *   u_opt: n_uopt x steps reference controls (host or device, dense; NULL with n_uopt = 0); unit.uopt = the row a unit is
 *   scored against, or -1.  out_x: n_units x (steps + 1) x d, out_u: n_units x steps (host or device); EITHER MAY BE NULL
 *   and is then never written on the device either.  scores: HOST, n_units x 4, may be NULL:
 *     scores[u] = {sse_u, ss_opt, J, u_absmax},
 *     sse_u = sum_t (u_t - u_opt[t])^2 and ss_opt = sum_t u_opt[t]^2, summed in step order (both 0 when uopt < 0);
 *     J = the cost of open_loop_control (benchmark_lqr_hjb.py:99-107): J = sum_k x0_k^2, then per step
 *         J = (J + sum_k x_{t+1,k}^2) + u_t^2, plain IEEE operations in this order (squares rounded, sums over k in index
 *         order): a host loop over the returned x, u gives the same bits;
 *     u_absmax = max_t |u_t|, NaN from the first NaN control on: a diverged unit shows without its trajectory.
 *   Everything is checked before anything is launched; a bad unit is NK_ERR_BAD_ARG with its index in nk_last_error().
 *   Per unit the conditions of nk_plant_loop hold (p = 1, d = the plant's, m <= 4096, kernel family).  K, x0, x_ref and
 *   scores are host memory.  Not all of out_x, out_u, scores may be NULL.  Ordinary contexts only (not lock-step
 *   members).  A model is not tied to the context that fitted it: models fitted by lock-step members (or by any other
 *   context) on the same device are accepted as they are.
 *   Device side: one record per unit in a table staged with one copy, blockIdx.x selects the record; one launch per class
 *   of (kernel family, landmarks per lane, waves per workgroup). */
typedef struct nk_plant_unit {
  const nk_model* model; /* Nystrom (RBF / Matern-5/2 / linear) or spline model, p = 1, d = the plant's, m <= 4096 */
  const double* K;       /* HOST, 1 x m gain */
  const double* x0;      /* HOST, d */
  const double* x_ref;   /* HOST, d */
  int32_t uopt;          /* row of u_opt this unit is scored against, or -1 */
  int32_t reserved;
} nk_plant_unit;
int nk_plant_loop_multi(nk_ctx* ctx, int plant, double Ts, int32_t steps, const nk_plant_unit* units, int32_t n_units,
                        const double* u_opt, int32_t n_uopt, double* out_x, double* out_u, double* scores);
/* ---- the same loops around a plant the CALLER describes: a polynomial vector field as a table of monomials, up to four
 *   states and four inputs, under one Runge-Kutta step of length Ts.
 *     f_row(x, u) = sum over the row's terms of coef * prod_k x_k^ex[k] * prod_j u_j^eu[j]
 *   The order of operations is part of the interface; the host build, the device build and the Python class
 *   PolynomialSystem give the same bits (plain IEEE operations, no fused multiply-add):
 *     term:  v = coef; for k = 0 .. d-1: v = v * x_k, ex[k] times; then for j = 0 .. p-1: v = v * u_j, eu[j] times;
 *     row:   f[row] starts at 0.0 and receives f[row] = f[row] + v in table order;
 *     step:  k2 = f(x + k1 Ts / 2.0), k3 = f(x + k2 Ts / 2.0), x + (Ts / 6.0) (((k1 + 2.0 k2) + 2.0 k3) + k4) with
 *            k4 = f(x + k3 Ts) (k4_at_k1 = 0: classical RK4) or f(x + k1 Ts) (k4_at_k1 = 1: the reference's variant, with
 *            which NK_PLANT_DUFFING, _DOUBLE_INTEGRATOR and _HJB can be written as tables).
 *   A description is checked by every entry point before anything is queued; NK_ERR_BAD_ARG with the field or the term
 *   index in the message for: d or p outside 1..4, n_terms outside 1..32, a row outside 0..d-1, an exponent set for
 *   k >= d or j >= p, a term of degree above 5, a non-finite coef, a non-finite or non-positive Ts, k4_at_k1 not 0 or 1.
 *   The step function: x_next = plant(x, u) on the HOST (x, x_next: d doubles, u: p doubles; no context, no GPU needed).
 *   The loop: the contract of nk_plant_loop with K: p x m, out_u: batch x steps x p; the model's d and p must equal the
 *   plant's.  u_j = sum_l W[l][j] (k(z_l, x_ref) - k(z_l, x_t)) with W = K_mm^{-1/2} K^T folded once per call.
 *   The multi form: the contract of nk_plant_loop_multi with nk_plant_unit.K: p x m, u_opt: n_uopt x steps x p, and the
 *   sums of the scores extended over the inputs in index order:
 *     sse_u = sum_t sum_j (u_tj - uopt_tj)^2,  ss_opt = sum_t sum_j uopt_tj^2  (both in (t, j) order),
 *     J = sum_k x0_k^2, then per step J = (J + sx) + su with sx = sum_k x_{t+1,k}^2 and su = sum_j u_tj^2 (rounded
 *     squares, index order),  u_absmax over t and j, NaN from the first NaN control on.
 *   Limit on m per class of (states, inputs) -- the landmarks, their reference values and p weights each stay in the
 *   registers of one workgroup of 16 waves:  d = 1, 2: m <= 4096 for p = 1, 2 and m <= 2048 for p = 3, 4;
 *   d = 3, 4: m <= 2048 for p = 1, 2 and m <= 1024 for p = 3, 4.  Beyond its class limit a call is NK_ERR_BAD_ARG. */
#define NK_POLY_MAX_D 4
#define NK_POLY_MAX_P 4
#define NK_POLY_MAX_TERMS 32
#define NK_POLY_MAX_DEGREE 5 /* sum of a term's exponents */
typedef struct nk_poly_term {
  int32_t row;   /* the state whose derivative the term belongs to */
  uint8_t ex[4]; /* exponents of the states */
  uint8_t eu[4]; /* exponents of the inputs */
  double coef;
} nk_poly_term;
typedef struct nk_poly_plant {
  int32_t d, p, n_terms, k4_at_k1;
  double Ts;
  nk_poly_term terms[NK_POLY_MAX_TERMS];
} nk_poly_plant;
int nk_poly_plant_step(const nk_poly_plant* plant, const double* x, const double* u, double* x_next);
int nk_poly_plant_loop(nk_ctx* ctx, const nk_model* model, const nk_poly_plant* plant, const double* K, const double* x0,
                       const double* x_ref, int32_t steps, int32_t batch, double* out_x, double* out_u);
int nk_poly_plant_loop_multi(nk_ctx* ctx, const nk_poly_plant* plant, int32_t steps, const nk_plant_unit* units,
                             int32_t n_units, const double* u_opt, int32_t n_uopt, double* out_x, double* out_u,
                             double* scores);
/* ---- the multi-model form of the lifted closed loop, scored on the device: the control branch of the cloth sweep
 *   (benchmark_lqr_cloth.py:213-270: per seed and estimator fit, gain, lqr_control) in ONE call after the fits and gains.
 *   Every unit has its own model, gain, lifted initial state and lifted reference; the units of a call share `steps` and
 *   `c` and may differ in everything else (model kind, m, p, d).  Unit u runs the loop of benchmark_lqr_cloth.py:79-84 in
 *   the reference's order of operations, for t = 0 .. steps-1:
 *     u_t = K (phi_ref - phi_t),   x_t = C phi_t,   phi_{t+1} = A phi_t + B u_t
 *   (not the (A - B K) form of nk_closed_loop_batch: the results agree with it to rounding, not bit for bit).
 *   Outputs, each dense with the units back to back (unit u owns the rows of its own width after those of the units before
 *   it; with equal shapes these are plain 3-D arrays), host or device memory, EACH MAY BE NULL and is then never written on
 *   the device either:
 *     out_x:    n_units x steps x d        x_t
 *     out_u:    n_units x steps x p        u_t
 *     out_ucum: n_units x (steps + 1) x p  the cumulative input sequence of benchmark_lqr_cloth.py:76-81: row 0 = u_init,
 *               row t+1 = row t + u_t, one rounded addition per entry in step order (u_s[:, -1] + u_op, not u0 + cumsum)
 *     out_err:  n_units x steps            e_t = sqrt(sum_k (x_{t,k} - target_k)^2 / d)  (plot_reg_error_cloth.py:24)
 *   scores: HOST, n_units x 4, may be NULL:  scores[u] = {J, err_final, u_sumsq, u_absmax},
 *     J = sum_t (c sum_k (x_{t,k} - target_k)^2 + sum_j u_{t,j}^2),  err_final = e_{steps-1},
 *     u_sumsq = sum_t sum_j u_{t,j}^2,  u_absmax = max_{t,j} |u_{t,j}|, NaN from the first NaN control on.
 *     All sums are taken in an order fixed by (m, p, d, steps).
 *   Not all five outputs may be NULL.  Everything is checked before anything is queued; a bad unit is NK_ERR_BAD_ARG with
 *   its index in nk_last_error(), and no output is written.  Per unit: a Nystrom or spline model WITH fitted operators on
 *   the context's device, 1 <= m <= 128, 1 <= p <= 8, d >= 1; K, phi0, phi_ref, target, u_init are HOST memory.  steps >= 1,
 *   c finite and non-negative.  Ordinary contexts only (not lock-step members); models need not belong to ctx (models
 *   fitted by lock-step members are accepted).
 *   Device side: one 1024-thread workgroup owns one unit from its first to its last step ([A B] in registers, phi_t and u_t in
 *   LDS, then x_t = C phi_t from the stored phi_t by the same workgroup); blockIdx.x selects a record of a table staged with
 *   one copy, all gains, lifted states, targets and seeds are staged with one more, and the whole call is one launch.  A
 *   unit's outputs depend on that unit alone: the same bits whatever else the call holds, in whatever order. */
typedef struct nk_loop_unit {
  const nk_model* model;   /* Nystrom or spline model WITH fitted operators; 1 <= m <= 128, 1 <= p <= 8, d >= 1 */
  const double* K;         /* HOST, p x m, dense */
  const double* phi0;      /* HOST, m: lifted initial state   (nk_lift of x0)    */
  const double* phi_ref;   /* HOST, m: lifted reference state (nk_lift of x_ref) */
  const double* target;    /* HOST, d: the state the loop is scored against (callers pass x_ref); NULL only if out_err and scores are NULL */
  const double* u_init;    /* HOST, p: seed of the cumulative input sequence (benchmark_lqr_cloth.py:78); NULL = zeros */
} nk_loop_unit;
int nk_closed_loop_multi(nk_ctx* ctx, int32_t steps, double c, const nk_loop_unit* units, int32_t n_units,
                         double* out_x, double* out_u, double* out_ucum, double* out_err, double* scores);
/* ---- the gains of the sweep: K = dlqr(A, B, Q, R) (benchmark_lqr_hjb.py:293,356, benchmark_lqr_classic.py:288,
 *   benchmark_lqr_cloth.py:262: control.dlqr) for MANY independent problems in one call.  P solves the discrete algebraic
 *   Riccati equation A'PA - P - A'PB (R + B'PB)^-1 B'PA + Q = 0 by the structure-preserving doubling iteration
 *     A_0 = A, G_0 = B R^-1 B', H_0 = Q;  W = I + G H,  [X_A | X_G] = W^-1 [A_k | G],
 *     A+ = A_k X_A,  G+ = sym(G + A_k X_G A_k'),  H+ = H + sym(A_k' H X_A),
 *   stopped when |H+ - H|_1 <= tol |H+|_1 or after max_iter steps (the reference values are tol = 1e-13, max_iter = 40);
 *   P = H and K = (R + B'PB)^-1 B'PA.  One workgroup owns one problem from start to finish (products on the fp64 matrix
 *   pipe, LU with partial row pivoting for W), so a problem's results do not depend on what else the call holds or in
 *   which order.  Limits: 1 <= m <= 256, 1 <= p <= 8.  Per problem the device workspace is 7 M^2 doubles, M = m rounded up
 *   to 16; the library issues launches in chunks so that the workspace of one launch stays under NK_DARE_WS_CAP_BYTES.
 *   out_status[u]: 0 = converged; 1 = max_iter reached; 2 = non-finite values, a zero or non-finite pivot of W, or R /
 *   R + B'PB not positive definite.  For a status other than 0 the problem's out_K and out_P are NaN; the other problems of
 *   the call are not affected.  out_iters[u] (may be NULL) = steps taken.
 *   Everything is checked before anything is queued; a bad problem is NK_ERR_BAD_ARG with its index in nk_last_error(),
 *   and no output is written.  All operands and results are HOST memory (staged with one copy per array kind).  Ordinary
 *   contexts only (not lock-step members). */
#define NK_DARE_WS_CAP_BYTES (1ll << 30)
typedef struct nk_dare_problem {
  int32_t m, p;
  const double* A; int64_t lda;  /* m x m */
  const double* B; int64_t ldb;  /* m x p */
  const double* Q; int64_t ldq;  /* m x m, symmetric positive semi-definite */
  const double* R; int64_t ldr;  /* p x p, symmetric positive definite */
  double* out_K;                 /* p x m, dense */
  double* out_P;                 /* m x m, dense; NULL skips the copy */
  double* out_delta;             /* the last relative step |H+ - H|_1 / |H+|_1 (NaN if no step was taken); may be NULL */
} nk_dare_problem;
int nk_dare_batch(nk_ctx* ctx, const nk_dare_problem* problems, int32_t n, double tol, int32_t max_iter,
                  int32_t* out_status, int32_t* out_iters);
/* The sweep's entry: the gains of n fitted models, K_u = dlqr(A_u, B_u, c sym(C_u'C_u), R), read from the models' device
 * allocations; the cost is formed on the device by the solver's own product and only the gains travel back.
 * R: HOST, p x p dense (then every model has p inputs), or NULL for the identity.  out_K: HOST, the gains back to back
 * (model u: p_u x m_u, dense).  Status, limits and checks as in nk_dare_batch.  Models need not belong to ctx: only the
 * device must match (models fitted by lock-step members are accepted); the call itself is for ordinary contexts.
 * nk_model_lqr_cost returns the cost matrix c sym(C'C) (m x m) exactly as the solver forms it, so that nk_dare_batch fed
 * nk_model_get's operators and this matrix reproduces nk_model_lqr_gain_batch bit for bit. */
int nk_model_lqr_gain_batch(nk_ctx* ctx, const nk_model* const* models, int32_t n, double c, const double* R_or_NULL,
                            double tol, int32_t max_iter, double* out_K, int32_t* out_status, int32_t* out_iters);
int nk_model_lqr_cost(nk_ctx* ctx, const nk_model* model, double c, double* Q, int64_t ldq);
/* ---- ONE problem past the batched solver's limits: the same doubling steps, stopping rule, status codes and NaN outputs as
 *   nk_dare_batch, run as a chain of ordinary launches on the context's stream: every m x m product on the fp64 GEMM engine,
 *   W = I + G H solved by a blocked LU with partial row pivoting (column blocks of 64; panel, row exchanges, row block and
 *   trailing update are separate launches).  No kernel waits for another workgroup, and the results are the same bits from
 *   call to call.  The host synchronises once per doubling step to read the status and the two norms of the stopping test.
 *   Limits: 1 <= m <= NK_DARE_LARGE_MAX_M, 1 <= p <= NK_DARE_LARGE_MAX_P.  Workspace: about 9 M^2 doubles (M = m rounded up
 *   to 16; 1.2 GB at m = 4096), a dedicated device allocation made for the call and freed before it returns; when it is
 *   refused the call returns NK_ERR_OOM and writes nothing.
 *   A, B, Q, R and out_K (p x m, dense), out_P (m x m, dense; may be NULL) are HOST or DEVICE memory, each on its own.
 *   out_delta (may be NULL): the last relative step; out_iters may be NULL.  Everything is checked before anything is
 *   queued or allocated: a bad argument is NK_ERR_BAD_ARG and no output is touched.  Ordinary contexts only. */
#define NK_DARE_LARGE_MAX_M 10240
#define NK_DARE_LARGE_MAX_P 32
int nk_dare_large(nk_ctx* ctx, int32_t m, int32_t p, const double* A, int64_t lda, const double* B, int64_t ldb,
                  const double* Q, int64_t ldq, const double* R, int64_t ldr, double tol, int32_t max_iter, double* out_K,
                  double* out_P, double* out_delta, int32_t* out_status, int32_t* out_iters);
/* The gain of one fitted model, K = dlqr(A, B, c sym(C'C), R), by the solver of nk_dare_large whatever m is: [A B] and C are
 * read from the model's device allocation, the cost is formed on the device (fp64 GEMM engine).  R: p x p dense, host or
 * device, or NULL for the identity.  out_K: p x m dense, host or device.  out_iters may be NULL. */
int nk_model_lqr_gain(nk_ctx* ctx, const nk_model* model, double c, const double* R_or_NULL, double tol, int32_t max_iter,
                      double* out_K, int32_t* out_status, int32_t* out_iters);
/* Diagnostics: host wall clock of the calling thread's last nk_dare_large / nk_model_lqr_gain in milliseconds,
 * out[0] = the solver in all, and -- only when NYSKOOP_DARE_TIMING is set in the environment, which synchronises the stream
 * around every phase -- out[1] = the LU launches, out[2] = the products and elementwise kernels of the steps, out[3] = the
 * per-step synchronisation; out[4] = steps taken. */
int nk_dare_large_times(double out[5]);
/* ---- Constrained Koopman MPC around a polynomial plant in ONE launch: box and rate limits on the inputs.
 *   Per step, with e = phi(x_t) - phi(x_ref) and the decision vector U = (u_0, ..., u_{N-1}) of nv = N p entries:
 *       minimise 1/2 U'HU + (F e)'U   subject to   lo <= U <= hi,   dlo <= u_k - u_{k-1} <= dhi  (k = 0 .. N-1),
 *   u_{-1} = the control applied at the previous step (u_init, or zeros, at t = 0), and the first p entries are applied.  H
 *   (nv x nv) and F (nv x m) are the condensed problem of the lifted model (lqr.mpc_condense in Python).  Bounds of +-inf are
 *   allowed and make a constraint inactive.
 *   THE ITERATION IS PART OF THE INTERFACE (lqr.mpc_admm_step / lqr.mpc_solve are its NumPy statement).  Constraint rows
 *   A_c = [I; D], D the block first difference, (D U)_k = u_k - u_{k-1} with (D U)_0 = u_0; the first p rate bounds are shifted
 *   by u_{-1}.  M = (H + rho (I + D'D))^-1 and H^-1 are formed once per call on the host (Cholesky).  With g = F e:
 *       U_unc = -H^-1 g;   s = A_c U_unc;   z = clip(s);   lambda = 0;   r = max |s - z|;   k = 0
 *       while k < iters and not (r <= tol and (k == 0 or tol > 0)):
 *           w = z - lambda;   U = M (rho (w_1 + D'w_2) - g);   s = A_c U;   z = clip(s + lambda);   lambda += s - z
 *           r = max |s - z|;   k += 1
 *       v = the first p entries of z;   u_t = clip(clip(v, lo, hi), u_{-1} + dlo, u_{-1} + dhi)
 *   The rate clip comes last, so a returned control never violates a rate limit whatever iters is, and never a bound either
 *   when u_{-1} lies within the bounds and dlo <= 0 <= dhi; at convergence both clips change nothing.  When U_unc is feasible
 *   r = 0 at k = 0: no iteration runs and u_t is the LQR control to rounding (the first p rows of H^-1 F are the Riccati gain
 *   when the terminal cost is the Riccati solution).  tol = 0 runs all iterations unless the start is feasible.
 *   iters = 0 is the SATURATED LQR: v = -K e = K (phi(x_ref) - phi(x_t)) from the gain K and the two clips above; H and F
 *   are not read.  For one input under a symmetric box alone and the Riccati terminal cost this IS the first move of the QP
 *   (measured: equal to 1e-15 of the bound at every step), so a bounds-only single-input user should take this mode.
 *   out_info (may be NULL): batch x steps x 2 = {iterations run, final max |s - z|} (iters = 0: zeros).
 *   NaN: a step whose gradient F e (a NaN state) or whose shifted rate bound u_{-1} + dlo / dhi (a NaN seed, inf - inf) holds a
 *   NaN ends as the NumPy statement ends it, whose clips hand a NaN on: every entry of u_t is NaN, out_info = {iters, NaN}
 *   (iters = 0: the entries of u_t whose own v or bounds are NaN, out_info zeros).  The device loop and nk_mpc_qp_host decide such a
 *   step before the iteration (their clips are fmin / fmax, which would return a bound); no other step is affected.
 *   Device side (nk_mpc_loop.hip): one workgroup per trajectory, ceil(m / 64) waves, the whole loop inside it.  F is folded
 *   into the lift once per call, W = S^-1 F' (m x nv; spline models: F'), and lives in LDS; g = W'(k(Z, x_t) - k(Z, x_ref)),
 *   the difference taken landmark by landmark before the product.  Lane i of the first wave owns decision variable i: its row
 *   of M stays in registers, the iterate is broadcast with v_readlane, D and D' are shifts by p lanes; the plant step
 *   follows in the same wave and the new state reaches the others through LDS.  Every summation order is fixed by (m, nv, p)
 *   alone: a trajectory has the same bits alone or in any batch.
 *   Limits: nv <= NK_MPC_MAX_NV, p <= 4, d <= 4, m <= 512 (eight waves: the largest workgroup whose lanes keep a row of M
 *   in registers without scratch) and 8 (m nv + 64 ceil(m / 64) + 16) <= 160 KB of LDS: m <= 512 up to nv = 38, 314 at
 *   nv = 64 (nk_mpc_loop_max_m).  Beyond: NK_ERR_BAD_ARG before anything is queued, as for every malformed field (H not
 *   symmetric positive definite, lo > hi, dlo > dhi, rho not finite and positive, iters < 0, tol negative, sizes) with the
 *   field named in nk_last_error(); no output is touched.  The arrays of the description are HOST memory; x0 (batch x d),
 *   x_ref (batch x d), u_init (batch x p, may be NULL), out_x (batch x (steps + 1) x d), out_u (batch x steps x p) and
 *   out_info are host or device memory.  Ordinary contexts only.
 *   nk_mpc_qp_host: ONE solve of the same iteration in the host build, no context and no GPU: e (m), u_prev (p, NULL =
 *   zeros); out_u (p) the control, out_z (nv, may be NULL; not written when iters = 0) the first nv entries of z, out_info
 *   (2, may be NULL). */
#define NK_MPC_MAX_NV 64
typedef struct nk_mpc_desc {
  int32_t N, p;       /* horizon and inputs; nv = N p */
  int32_t m;          /* lifted dimension: F is nv x m, K is p x m */
  int32_t iters;      /* >= 0; 0 = the saturated LQR */
  const double* H;    /* nv x nv dense, symmetric positive definite (iters > 0) */
  const double* F;    /* nv x m dense (iters > 0) */
  const double* lo;   /* nv, or NULL = -inf */
  const double* hi;   /* nv, or NULL = +inf */
  const double* dlo;  /* nv, or NULL = -inf */
  const double* dhi;  /* nv, or NULL = +inf */
  const double* K;    /* p x m dense (iters = 0) */
  double rho, tol;    /* rho finite > 0; tol finite >= 0 */
} nk_mpc_desc;
int nk_mpc_loop(nk_ctx* ctx, const nk_model* model, const nk_poly_plant* plant, const nk_mpc_desc* desc, const double* x0,
                const double* x_ref, const double* u_init_or_NULL, int32_t steps, int32_t batch, double* out_x, double* out_u,
                double* out_info_or_NULL);
int nk_mpc_qp_host(const nk_mpc_desc* desc, const double* e, const double* u_prev_or_NULL, double* out_u, double* out_z,
                   double* out_info);
int nk_mpc_loop_max_m(int32_t nv);  /* the limit on m for nv decision variables (0: nv out of range) */
/* ---- Limits on PREDICTED STATES in the constrained MPC loop, hard or soft: ny output rows beside an unchanged nk_mpc_desc.
 *   Per step, with e = phi(x_t) - phi(x_ref) and U as for nk_mpc_loop:
 *       minimise 1/2 U'HU + (F e)'U + (w_y / 2) dist^2(G U + T e, [ylo', yhi'])
 *       subject to lo <= U <= hi,  dlo <= u_k - u_{k-1} <= dhi
 *   w_y = y_weight = +inf makes the output rows hard constraints; a finite w_y > 0 penalises the squared violation -- that QP
 *   is always feasible, which a plant pushed outside its limits needs.  A hard problem whose first predicted state is out of
 *   reach does not converge; w_y far above rho (1e3 rho) converges very slowly.
 *   G (ny x nv) and T (ny x m) are the condensed prediction of selected state components over the steps k = 1 .. Ny <= N in
 *   the error coordinates of the cost (lqr.mpc_condense_outputs): row (k, c) of T is C_c A^k, block (k, j) of G is
 *   C_c A^(k-1-j) B for j < k, else 0.  ycomp[r] names the state component of row r, or -1 for a row without a reference
 *   shift (NULL: every row -1).  ylo, yhi are ABSOLUTE state bounds: b = ylo_r - x_ref[ycomp_r] is one rounded subtraction
 *   per trajectory, done once, and the bound of a step is b - t_r with t = T e; likewise for yhi.
 *   THE ITERATION IS PART OF THE INTERFACE, in the folded form the device runs (lqr.mpc_out_solve is its NumPy statement,
 *   csrc/nk_mpc_out.h the host build).  A_c = [I; D; G]; nt = nv + ny.  Formed once per call on the host:
 *       M = (H + rho (I + D'D + G'G))^-1 by Cholesky;   Kb = [[M, M G'], [G M, G M G']] (nt x nt) by plain products from M,
 *       symmetrised;   S0 = [H^-1; G H^-1] (nt x nv);   theta = rho / (rho + w_y), 0 for w_y = inf.
 *       prox: box and rate rows clip;  output rows  c = clip(v);  z = c + theta (v - c).
 *   With g = F e, rows ordered (box, rate, output) and s_K the nt entries (s_1, s_3):
 *       s_K = -(S0 g);   s = (s_K[:nv], D s_K[:nv], s_K[nv:]);   z = prox(s);   lambda = 0;   r = max |s - z|;   k = 0
 *       while k < iters and not (r <= tol and (k == 0 or tol > 0)):
 *           w = z - lambda;   q = [rho (w_1 + D'w_2) - g ; rho w_3];   s_K = Kb q, and s from it as above
 *           z = prox(s + lambda);   lambda += s - z;   r = max |s - z|;   k += 1
 *       v = the first p entries of z_1;   u_t = clip(clip(v, lo, hi), u_{-1} + dlo, u_{-1} + dhi)
 *   Output bounds all inactive at the start give r = 0 at k = 0 (when the input limits are inactive too): no iteration, and
 *   z_1 = U_unc.  A finite w_y leaves r > 0 at a start outside the output bounds.
 *   NaN: the rule of nk_mpc_loop, extended to t = T e and to the shifted output bounds: such a step has NaN controls and
 *   out_info = {iters, NaN}, and affects no other step or trajectory.
 *   Device side (nk_mpc_loop.hip): the loop of nk_mpc_loop on nt lanes of the first wave.  W = S^-1 [F; T]' (m x nt;
 *   spline models: [F; T]') lives in LDS; lane i < nv receives g_i and lane nv + r receives t_r from the same pass.  Lane i
 *   keeps row i of Kb in registers (classes 16 / 32 / 64 over nt), one iteration is one pass of FMAs over q broadcast with
 *   v_readlane; S0 is read once per step, transposed so that lanes read consecutive words; output lanes hold their shifted
 *   bounds where input lanes hold lo / hi and take no part in the shifts of D.  Every summation order is fixed by
 *   (m, nv, ny, p) alone: a trajectory has the same bits alone or in any batch.
 *   Limits: iters >= 1 (iters = 0, the saturated LQR, is nk_mpc_loop's), nv + ny <= 64, m <= nk_mpc_loop_max_m(nv + ny), p <= 4,
 *   d <= 4.  Everything is validated before anything is queued or written, with the field named in nk_last_error(): every
 *   rule of nk_mpc_desc, ny outside 1 .. 64 - nv, ylo > yhi, ycomp outside -1 .. d - 1, y_weight not positive or NaN, G or T
 *   NULL or not finite, M not positive definite.  The arrays of both descriptions are HOST memory; everything else as for
 *   nk_mpc_loop.  Ordinary contexts only.
 *   nk_mpc_out_qp_host: ONE solve of the same iteration in the host build, no context and no GPU: e (m), x_ref (the reference
 *   state, read at ycomp; NULL = no shift; ycomp is checked against -1 .. 3), u_prev (p, NULL = zeros); out_u (p), out_z
 *   (nt = nv + ny, may be NULL: z_1 then z_3), out_info (2, may be NULL). */
typedef struct nk_mpc_out {
  int32_t ny, reserved;  /* output rows, 1 .. 64 - nv */
  const double* G;       /* ny x nv dense */
  const double* T;       /* ny x m dense */
  const double* ylo;     /* ny absolute lower bounds, or NULL = -inf */
  const double* yhi;     /* ny absolute upper bounds, or NULL = +inf */
  const int32_t* ycomp;  /* ny state components, -1 = no reference shift; NULL = all -1 */
  double y_weight;       /* > 0; +inf = hard rows */
} nk_mpc_out;
int nk_mpc_out_loop(nk_ctx* ctx, const nk_model* model, const nk_poly_plant* plant, const nk_mpc_desc* desc,
                    const nk_mpc_out* out, const double* x0, const double* x_ref, const double* u_init_or_NULL, int32_t steps,
                    int32_t batch, double* out_x, double* out_u, double* out_info_or_NULL);
int nk_mpc_out_qp_host(const nk_mpc_desc* desc, const nk_mpc_out* out, const double* e, const double* x_ref_or_NULL,
                       const double* u_prev_or_NULL, double* out_u, double* out_z, double* out_info);
/* ---- the multi-model form of the constrained MPC loop, scored on the device: the seeds x m table of the control experiments
 *   under actuator limits in ONE call after the fits and controllers.  The units of a call share the plant and `steps` and
 *   may differ in everything else: model kind, kernel family, m, horizon, iters (0, the saturated LQR, included), rho, tol,
 *   limits, x0, x_ref, u_init.  UNIT u IS BIT FOR BIT nk_mpc_loop(model, plant, desc, x0, x_ref, u_init, steps, batch = 1) in
 *   out_x, out_u and out_info, whatever else the call holds and in whatever order: M, H^-1 and the bounds come from the same
 *   host preparation, and the fold W = S^-1 F' (iters = 0: S^-1 K') is the same product on operands laid out as the single
 *   call lays them out.
 *   Outputs, host or device memory, EACH MAY BE NULL and is then never written on the device either:
 *     out_x:    n_units x (steps + 1) x d   (row 0 = x0)
 *     out_u:    n_units x steps x p
 *     out_info: n_units x steps x 2         {iterations run, final max |s - z|}
 *   scores: HOST, n_units x NK_MPC_N_SCORES, may be NULL.  The four outputs must not all be NULL.
 *   u_opt: n_uopt x steps x p reference controls (host or device), unit u is scored against row units[u].uopt (-1: none, and
 *   then sse_u = ss_opt = 0), as in nk_poly_plant_loop_multi.
 *     scores[u] = {sse_u, ss_opt, J, u_absmax, iters_sum, r_max, n_at_limit, n_iterated}
 *   The first four are those of nk_poly_plant_loop_multi: the same order of operations, rounded squares, no contraction.
 *     iters_sum  = sum over t of the iterations run (out_info[t][0]), in step order;
 *     r_max      = max over t of the final max |s - z| (out_info[t][1]), NaN from the first NaN on (the rule of u_absmax);
 *     n_at_limit = the number of (t, j) at which the applied u_tj equals one of its four bounds of that step: lo_j, hi_j,
 *                  fl(u_{t-1,j} + dlo_j), fl(u_{t-1,j} + dhi_j) (u_{-1} = u_init or zeros).  A clip returns the bound itself,
 *                  so this is exact; a (t, j) at two bounds at once counts once;
 *     n_iterated = the number of steps with at least one iteration.
 *   A host loop over the returned out_x, out_u, out_info and the bounds gives the same bits for all eight
 *   (harness.mpc_scores in Python).  A unit started at a NaN x0 has NaN controls (the NaN rule of nk_mpc_loop), so its
 *   u_absmax, J and r_max are NaN, iters_sum = steps * iters and n_at_limit = 0; the other units are not affected.
 *   Everything is checked before anything is queued or written; a bad unit is NK_ERR_BAD_ARG with its index and the field in
 *   nk_last_error().  Per unit every check of nk_mpc_loop applies (the description and its host arrays, d / p / m agreement,
 *   kernel family, m <= nk_mpc_loop_max_m(nv), LDS), and: uopt in -1 .. n_uopt - 1, reserved == 0, x0 / x_ref / u_init host
 *   memory; n_units >= 1, steps >= 1.  Ordinary contexts only (not lock-step members); models need not belong to ctx, the
 *   same device suffices.
 *   Device side (nk_mpc_loop.hip): the loop body of nk_mpc_loop reading a per-unit record; blockIdx.x selects a record of a
 *   table staged with one copy, all constants, F / K, states and seeds are staged with one more.  One launch per class of
 *   (kernel family, padded states, nv padded to 16 / 32 / 64, ceil(m / 64) waves); no kernel waits for another workgroup.
 *   The scores are accumulated by one lane in step order. */
typedef struct nk_mpc_unit {
  const nk_model* model;    /* as for nk_mpc_loop: Nystrom (RBF / Matern-5/2 / linear) or spline model, d and p = the plant's */
  const nk_mpc_desc* desc;  /* HOST, its arrays HOST; desc->m == model->m, desc->p == plant->p; units may share one */
  const double* x0;         /* HOST, d */
  const double* x_ref;      /* HOST, d */
  const double* u_init;     /* HOST, p, or NULL = zeros */
  int32_t uopt;             /* row of u_opt this unit is scored against, or -1 */
  int32_t reserved;         /* must be 0 */
} nk_mpc_unit;
#define NK_MPC_N_SCORES 8
int nk_mpc_loop_multi(nk_ctx* ctx, const nk_poly_plant* plant, int32_t steps, const nk_mpc_unit* units, int32_t n_units,
                      const double* u_opt, int32_t n_uopt, double* out_x, double* out_u, double* out_info, double* scores);
/* ---- the multi-model form of the loop with limits on predicted states, scored on the device: the seeds x m table under a
 *   state limit in ONE call, with and without the limit side by side.  `units` is the unit table of nk_mpc_loop_multi,
 *   unchanged; outs[u] (HOST, its arrays HOST) is the output description of unit u, outs[u] == NULL marks a unit without rows,
 *   and outs itself may be NULL (no unit has rows).
 *   WITH ROWS, UNIT u IS BIT FOR BIT nk_mpc_out_loop(model, plant, desc, outs[u], x0, x_ref, u_init, steps, batch = 1) in out_x,
 *   out_u and out_info; WITHOUT ROWS IT IS BIT FOR BIT nk_mpc_loop(...), and with it its entry of nk_mpc_loop_multi.  Both hold
 *   whatever else the call holds and in whatever order, and one call may mix both kinds: Kb, S0, M, H^-1 and the bounds come
 *   from the host preparation of the single calls, and the fold W = S^-1 [F; T]' (W = S^-1 F', S^-1 K') is the same product on
 *   operands laid out as the single call lays them out.  Units that share (model, desc, outs[u]) share every prepared piece.
 *   A unit with outs[u] != NULL and desc->iters == 0 is NK_ERR_BAD_ARG naming the unit, as nk_mpc_out_loop refuses it (the
 *   saturated LQR has no rows: pass outs[u] = NULL).
 *   Outputs as for nk_mpc_loop_multi: each may be NULL, not all four; scores: HOST, n_units x NK_MPC_OUT_N_SCORES.
 *     scores[u] = {sse_u, ss_opt, J, u_absmax, iters_sum, r_max, n_at_limit, n_iterated, y_viol_max, n_y_viol}
 *   The first eight keep the definitions of nk_mpc_loop_multi (n_at_limit counts input bounds only).
 *     y_viol_max = max over the steps t = 0 .. steps - 1 and the output rows r with ycomp[r] >= 0 of
 *                  max(fl(ylo_r - x_{t+1}[c]), fl(x_{t+1}[c] - yhi_r), 0), c = ycomp[r]: each difference is one rounded
 *                  subtraction on the ABSOLUTE bounds and the REALISED next state -- for the tiled bounds that solve_mpc builds,
 *                  the largest excursion of the plant past its state limits.  0 when nothing is violated.  The NaN rule of
 *                  u_absmax: a step with a NaN difference has a NaN maximum, which enters once and stays;
 *     n_y_viol   = the number of steps at which that per-step maximum is > 0 (a NaN step does not count).
 *   A unit without rows has 0 and 0 in both.  A host loop over the returned out_x and the bounds gives the same bits
 *   (harness.mpc_out_scores in Python).  A unit started at a NaN x0 has NaN u_absmax, J, r_max and y_viol_max (the latter when
 *   a row has a component); the other units are not affected.
 *   Everything is checked before anything is queued or written, with the unit index and the field in nk_last_error(): every
 *   check of nk_mpc_loop_multi, and per unit with rows every check of nk_mpc_out_loop (the rules of nk_mpc_out, m <=
 *   nk_mpc_loop_max_m(nv + ny), LDS, outs[u] and its arrays host memory).  Ordinary contexts only.
 *   Device side (nk_mpc_loop.hip): the loop body of nk_mpc_out_loop on a per-unit record, one launch per class of (kernel
 *   family, padded states, nv + ny padded to 16 / 32 / 64, ceil(m / 64) waves); the units without rows run the launches of
 *   nk_mpc_loop_multi.  One staging copy, one table copy per kind, one synchronisation; no kernel waits for another workgroup.
 *   An output lane keeps its absolute bounds and forms its violation from the new state; one butterfly per step gives the
 *   maximum, lane 0 of the first wave folds it in step order. */
#define NK_MPC_OUT_N_SCORES 10
int nk_mpc_out_loop_multi(nk_ctx* ctx, const nk_poly_plant* plant, int32_t steps, const nk_mpc_unit* units,
                          const nk_mpc_out* const* outs, int32_t n_units, const double* u_opt, int32_t n_uopt, double* out_x,
                          double* out_u, double* out_info, double* scores);
/* ---- the controllers of the MPC sweeps, built on the device for MANY independent units in one call: the Riccati solution,
 *   a Newton polish, the condensed problem (H, F) of the loops above and the output rows (G, T) of nk_mpc_out.
 *   Per unit, with nv = N p:
 *   Riccati stage (skipped when P is given): (K, P) by the doubling iteration of nk_dare_batch (m <= 256: ONE launch of that
 *     solver over all such units of a group) or of nk_dare_large (256 < m <= 512: one unit after the other), with tol and
 *     max_iter; the same code, so with newton_steps = 0 K and P are bit for bit what those calls return.
 *   Newton stage (newton_steps Hewer steps; skipped when P is given), each step a correction of the current P
 *   (lqr.dare_newton_smith in Python is the NumPy statement):
 *       Ac = A - B K,  Y = sym((Ac'P Ac - P) + (Q + (K'R) K));
 *       repeat  D = sym(Ac' Y Ac),  Y += D,  stop when |D|_1 <= newton_tol |Y|_1,  else Ac = Ac Ac   (at most newton_max_iter times)
 *       P += Y,  K = (R + sym(B'PB))^-1 B'PA  (Cholesky).
 *     P + Y solves the step's Lyapunov equation X = Ac'X Ac + Q + K'RK; the Smith iteration carries the correction alone, so
 *     its rounding is relative to the correction and not to P.
 *     With P given (symmetric: B'PA is formed as (P B)'A), K = (R + sym(B'PB))^-1 B'PA from that P.
 *   Condensing (lqr.mpc_condense_blocked in Python is the NumPy statement; the result is that of lqr.mpc_condense):
 *       G_0 = B, G_k = A G_{k-1};  QG = Q [G_0 .. G_{N-1}],  PG = P [G_0 .. G_{N-1}];  W = 0 (m x nv)
 *       for l = N .. 0:  W = A' W;  block column j of W += (PG if l == N else QG) block l-1-j, for every j < min(l, N);
 *                        for l >= 1: block row l-1 of H, columns 0 .. l-1, = 2 B' W
 *       F = 2 W';  H is mirrored from its lower triangle (entry by entry) and its diagonal blocks get + 2 sym(R):
 *     H is returned bitwise symmetric.
 *   Output rows (nc > 0; lqr.mpc_condense_outputs): R_0 = C_rows, R_k = R_{k-1} A; row block k of T = R_k, block (k, j) of G =
 *     R_{k-1-j} B for j < k and exactly 0 otherwise, k = 1 .. Ny.
 *   One workgroup owns one unit from start to finish; the products run on the fp64 matrix pipe in orders fixed by (m, p, N,
 *   nc, Ny) alone, so a unit's results do not depend on what else the call holds or in which order.
 *   out_status[u]: 0 = success; 1 = the doubling iteration reached max_iter; 2 = non-finite values, a singular pivot, or R /
 *   R + B'PB not positive definite; 3 = the Smith iteration reached newton_max_iter.  A unit with a status other than 0 has
 *   NaN in all its outputs; the other units of the call are not affected.  out_iters (may be NULL): n x 2, {doubling steps,
 *   Smith squarings over all Newton steps}.
 *   Limits: 1 <= m <= 512, 1 <= p <= 4, N >= 1, N p <= NK_MPC_MAX_NV, 0 <= nc <= 4, 1 <= Ny <= N when nc > 0,
 *   0 <= newton_steps <= 4, 1 <= max_iter, newton_max_iter <= 1000.  Device workspace per unit: about 6 M^2 + 5 M NVP doubles
 *   (M, NVP = m, nv rounded up to 16), plus 7 M^2 in the Riccati stage for m <= 256; the library works in groups whose
 *   workspace stays under NK_DARE_WS_CAP_BYTES.
 *   nk_mpc_build_batch: every operand and result is HOST memory (staged with one copy in and one copy out per group); the
 *   operands have leading dimensions, the results are dense.  Everything is checked before anything is queued or allocated: a
 *   bad field is NK_ERR_BAD_ARG with the problem index and the field's name in nk_last_error(), and no output is touched.
 *   Ordinary contexts only (not lock-step members). */
typedef struct nk_mpc_build_problem {
  int32_t m, p, N;
  int32_t nc, Ny;                     /* output rows: nc rows of C_rows over the steps 1 .. Ny; nc = 0: none (Ny is ignored) */
  int32_t reserved;
  const double* A; int64_t lda;       /* m x m */
  const double* B; int64_t ldb;       /* m x p */
  const double* Q; int64_t ldq;       /* m x m, symmetric positive semi-definite */
  const double* R; int64_t ldr;       /* p x p, symmetric positive definite */
  const double* P; int64_t ldp;       /* m x m SYMMETRIC terminal cost, or NULL: the Riccati solution of (A, B, Q, R) */
  const double* C_rows; int64_t ldc;  /* nc x m; may be NULL when nc = 0 */
  double* out_H;                      /* nv x nv */
  double* out_F;                      /* nv x m */
  double* out_K;                      /* p x m */
  double* out_P;                      /* m x m: the terminal cost used; NULL skips the copy */
  double* out_G;                      /* Ny nc x nv; may be NULL when nc = 0 */
  double* out_T;                      /* Ny nc x m; may be NULL when nc = 0 */
} nk_mpc_build_problem;
int nk_mpc_build_batch(nk_ctx* ctx, const nk_mpc_build_problem* problems, int32_t n, double tol, int32_t max_iter,
                       int32_t newton_steps, double newton_tol, int32_t newton_max_iter, int32_t* out_status,
                       int32_t* out_iters);
/* The sweep's entry: the controllers of n fitted models.  [A B] and C are read from the models' device allocations,
 * Q = c sym(C'C) is formed on the device exactly as nk_model_lqr_cost forms it, R: HOST, p x p dense (then every model has p
 * inputs), or NULL for the identity.  specs[u] (HOST): the horizon N and the output rows, row r = row comps[r] of C (a state
 * component, 0 <= comps[r] < d), r < nc, over the steps 1 .. Ny.  outs[u] (HOST, its arrays HOST and dense): H, F, K, and G, T
 * when nc > 0; only these travel back.  Stages, status, limits and checks as in nk_mpc_build_batch (the Riccati stage always
 * runs).  Models need not belong to ctx: only the device must match (models fitted by lock-step members are accepted); the
 * call itself is for ordinary contexts. */
typedef struct nk_mpc_build_spec {
  int32_t N, nc;
  int32_t comps[4];
  int32_t Ny, reserved;
} nk_mpc_build_spec;
typedef struct nk_mpc_build_out {
  double *H, *F, *K, *G, *T;
} nk_mpc_build_out;
int nk_model_mpc_build_batch(nk_ctx* ctx, const nk_model* const* models, int32_t n, double c, const double* R_or_NULL,
                             const nk_mpc_build_spec* specs, double tol, int32_t max_iter, int32_t newton_steps,
                             double newton_tol, int32_t newton_max_iter, const nk_mpc_build_out* outs, int32_t* out_status,
                             int32_t* out_iters);
/* Diagnostics: device time of the calling thread's last nk_mpc_build_batch / nk_model_mpc_build_batch in milliseconds, by
 * events on the context's stream, summed over the call's groups: out[0] = the Riccati stage (the staging of its table
 * included; 0 when every P was given), out[1] = the build launch, out[2] = the number of groups. */
int nk_mpc_build_times(double out[3]);
/* ---- rollout of explicit operators without a model (any estimator that exposes A, B, C: the exact-kernel comparator of
 *   benchmark_lqr_hjb.py:334-381, un-pickled gains): z0: batch x m lifted initial states; A: m x m, B: m x p, C: d x m
 *   (row-major, host or device); U, out_x, out_z as in nk_rollout. --------------------------------------------------- */
int nk_linear_rollout(nk_ctx* ctx, const double* A, const double* B, const double* C, int32_t m, int32_t d, int32_t p,
                      const double* z0, const double* U, int32_t T, int32_t batch, double* out_x, double* out_z);

/* ---- building blocks exported for parity tests and reuse (device or host pointers) --------------------- */
/* C[M x N] (fp64) = A^T B with fp32 operands stored K x M / K x N (the fp32 engine of nk_set_compute_dtype as a building
 * block: fp32 products, fp32 partial sums over at most 32 rows, fp64 beyond).  M, N >= 4, K > 0.  Host operands need only
 * lda >= M, ldb >= N, ldc >= N: they are packed for the engine, and only the M x N block of a host C is written.  A DEVICE A
 * or B is read in place and must be 16-byte aligned with a leading dimension that is a multiple of 4 and covers the columns
 * rounded up to one (the pad columns are read, never used); a device C needs ldc >= N only.  A device operand that breaks
 * this is NK_ERR_BAD_ARG before anything is copied or written. */
int nk_gemm_f32(nk_ctx* ctx, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B, int64_t ldb,
                double* C, int64_t ldc);
/* C[M x N] = alpha * op(A) op(B) + beta * C;  transA: A is stored K x M;  transB: B is stored N x K. */
int nk_gemm(nk_ctx* ctx, int transA, int transB, int64_t M, int64_t N, int64_t K, double alpha,
            const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
/* S = P^{1/2}, Sinv = P^{-1/2} for symmetric positive definite P (m x m); regressors.py:140,163,175. */
int nk_sqrtm_spd(nk_ctx* ctx, const double* P, int64_t ldp, int32_t m, double* S, double* Sinv,
                 int32_t* iters, double* residual);
/* X = P^{-1} R for symmetric positive definite P (m x m), R: m x nrhs; regressors.py:155,165.  A numerically singular P
 * gets lstsq's minimum-norm solution (see nk_set_strict_spd). */
int nk_solve_spd(nk_ctx* ctx, const double* P, int64_t ldp, int32_t m, const double* R, int64_t ldr,
                 int32_t nrhs, double* X, int64_t ldxo);

/* ---- diagnostics ---------------------------------------------------------------------------------------- */
/* Runs `reps` fused Gram launches (the dominant kernel of nk_nystrom_fit) on a synthetic n x (2m+p) feature matrix and
 * n x d targets resident in HBM; returns the average kernel time (HIP events on the context's stream) and the
 * algorithmic flop of one launch.  For rocprofv3 --pmc runs that should not pay for a whole fit. */
int nk_bench_gram(nk_ctx* ctx, int64_t n, int32_t m, int32_t p, int32_t d, int32_t reps, double* ms_avg, double* flop);

/* The augmented blocked Cholesky that every fit runs, on matrices of the caller's own (tests/test_gpu_chol_accuracy.py).
 * nsys = 1 or 2 systems [P_q (m_q x m_q, symmetric, leading dimension ldp_q >= m_q); R_q (extra_q x m_q, dense)], all host
 * arrays, are staged as the fits lay them out (the extra rows below the matrix, leading dimension ldp_q), factorised and
 * solved in one paired call (tile-dataflow launch where every m_q >= 256 and NYSKOOP_CHOL_FLOW is not 0, the launch-per-step
 * chain otherwise), and come back as
 *   L_q (m_q x m_q, dense): the lower factor, P = L L^T.  Only the lower triangle is the factor: tiles of 64 x 64 that lie
 *       strictly above the block diagonal are never written and return the input, and the strict upper triangle INSIDE a
 *       diagonal tile holds leftovers of the in-tile elimination (no meaning, and not the same on the two code paths);
 *   X_q (extra_q x m_q, dense) = R_q P_q^-1;
 *   failed[q]: 0 = factorised; k > 0 = the first non-positive pivot was met at row k - 1, i.e. LAPACK potrf's `info`
 *       (L and X are then meaningless from that row on); -1 = all pivots positive but an isolated cluster of them at the
 *       rounding level (an exact null space; L and X are still returned); NK_CHOL_FLOW_GIVEUP = the dataflow launch
 *       stopped waiting (set for every system of the call; the fits re-run the chain then, this function does not);
 *   piv_ratio[q]: smallest / largest pivot (0 when failed[q] is positive or the give-up word).
 * No recovery or fallback of any kind happens here. */
#define NK_CHOL_FLOW_GIVEUP (-0x40000000)
int nk_chol_aug(nk_ctx* ctx, int32_t nsys, const double* const* P, const int64_t* ldp, const int32_t* m,
                const double* const* R, const int32_t* extra, double* const* L, double* const* X, int32_t* failed,
                double* piv_ratio);

#ifdef __cplusplus
}
#endif
#endif /* NYSKOOP_H */
