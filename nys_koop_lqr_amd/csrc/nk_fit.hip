// The two fits behind the C ABI: the Nystrom fit (nk_nystrom_fit / nk_nystrom_gram / nk_nystrom_solve: struct NystromFit,
// a sequence of named stages called by NystromFit::run) and the thin-plate-spline fit (nk_spline_fit), with the row selection,
// pass planning and fp64 kernel blocks they share.
#include "nk_common.h"
#include "nk_chol.h"
#include "nk_tn.h"
#include "nk_api_internal.h"

#include <cmath>
#include <cstring>
#include <cstdlib>
#include <algorithm>
#include <initializer_list>

using namespace nk;

// Packed Gram accumulator of a fit (nk_nystrom_gram / nk_nystrom_solve): [G1 (m+p)x(m+p) ; G2 m x (m+p)] row-major with
// leading dimension m+p, then (at an even offset) [G3 m x m ; G4 d x m] with leading dimension m.
static inline size_t gram_block1(int m, int p) { return (((size_t)(2 * m + p) * (m + p)) + 1) & ~(size_t)1; }
static inline size_t gram_doubles(int m, int d, int p) { return gram_block1(m, p) + (size_t)(m + d) * m; }

// ---- row and pass plumbing shared by the two fits --------------------------------------------------------------------

// The training rows as [begin, end) pairs in `rng` (the whole of [0, n) without row ranges; empty ranges dropped).
static int select_rows(const char* who, const int64_t* row_ranges, int32_t n_ranges, int64_t n, std::vector<int64_t>* rng,
                       int64_t* n_eff) {
  if (row_ranges && n_ranges > 0) {
    for (int i = 0; i < n_ranges; ++i) {
      const int64_t b = row_ranges[2 * i], e = row_ranges[2 * i + 1];
      NK_REQUIRE(0 <= b && b <= e && e <= n, "%s: row range %d = [%lld,%lld) outside [0,%lld)", who, i, (long long)b,
                 (long long)e, (long long)n);
      if (e > b) { rng->push_back(b); rng->push_back(e); }
    }
  } else {
    rng->push_back(0); rng->push_back(n);
  }
  *n_eff = 0;
  for (size_t i = 0; i < rng->size(); i += 2) *n_eff += (*rng)[i + 1] - (*rng)[i];
  NK_REQUIRE(*n_eff > 0, "%s: no training rows selected", who);
  return NK_OK;
}

// several row ranges (a K-fold training set is two) of at most 256 MB: gather the rows into contiguous scratch once, so
// that everything downstream sees ONE piece of n_eff rows whatever the split point -- the kernel blocks and the fused Gram
// launch then have the same shape for every fold (which is also what lets the units of a sweep share launches,
// nk_lockstep.h)
static int gather_ranges(nk_ctx* ctx, int d, int p, int64_t n_eff, std::vector<int64_t>* rng, MatIn* x, MatIn* y) {
  if (!(rng->size() > 2 && (double)n_eff * (2.0 * d + p) * 8.0 <= 256e6)) return NK_OK;
  const int64_t ldxg = (d + p + 1) & ~(int64_t)1, ldyg = (d + 1) & ~(int64_t)1;
  double *xg = nullptr, *yg = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)n_eff * ldxg, &xg));
  NK_TRY(arena_alloc_t(ctx, (size_t)n_eff * ldyg, &yg));
  int64_t o = 0;
  for (size_t i = 0; i < rng->size(); i += 2) {
    const int64_t b = (*rng)[i], len = (*rng)[i + 1] - (*rng)[i];
    NK_TRY(launch_copy2d(ctx, x->ptr + b * x->ld, x->ld, xg + o * ldxg, ldxg, len, d + p));
    NK_TRY(launch_copy2d(ctx, y->ptr + b * y->ld, y->ld, yg + o * ldyg, ldyg, len, d));
    o += len;
  }
  x->ptr = xg; x->ld = ldxg; y->ptr = yg; y->ld = ldyg;
  rng->assign({(int64_t)0, n_eff});
  return NK_OK;
}

// rows of the feature matrix (leading dimension ldf) per pass under the workspace budget NYSKOOP_F_BUDGET_GB (read per fit)
static int64_t pass_rows_for(int64_t ldf, double bytes_per_elem) {
  const char* b = getenv("NYSKOOP_F_BUDGET_GB");
  const double budget = (b ? atof(b) : 48.0) * 1073741824.0;
  int64_t pass_rows = (int64_t)(budget / ((double)ldf * bytes_per_elem));
  if (pass_rows < 1024) pass_rows = 1024;
  return pass_rows & ~(int64_t)1023;  // whole k-steps per pass (the assembly k loops take K ranges of full steps only)
}

struct Piece { int64_t b, len; };
// the selected rows cut into passes of at most pass_rows rows, each a list of contiguous pieces
static std::vector<std::vector<Piece>> plan_passes(const std::vector<int64_t>& rng, int64_t pass_rows) {
  std::vector<std::vector<Piece>> passes(1);
  int64_t used = 0;
  for (size_t i = 0; i < rng.size(); i += 2) {
    int64_t b = rng[i];
    const int64_t e = rng[i + 1];
    while (b < e) {
      if (used == pass_rows) { passes.emplace_back(); used = 0; }
      const int64_t len = std::min(e - b, pass_rows - used);
      passes.back().push_back(Piece{b, len});
      used += len;
      b += len;
    }
  }
  return passes;
}

// The fp64 kernel blocks of a fit: feature rows F = [k(x, Z_in) | U | (pad) | k(y, Z_out)] (leading dimension ldf, the second
// block at column off_out), either in Gram form on the MFMA engine (rows and landmarks centred on `center`, scaled by 1/l,
// transposed: Rt / sqr are scratch for one piece of rows, Zt* / sqz* the prepared landmarks) or by direct differences from
// the raw landmarks.
struct KernelBlocks {
  int ktype = 0;
  double sigma0 = 0.0;
  int d = 0, p = 0, m = 0;
  const double* winv = nullptr;
  bool gram_form = false;
  MatIn zi, zo;
  double *center = nullptr, *Rt = nullptr, *sqr = nullptr, *Zto = nullptr, *sqzo = nullptr, *Zti = nullptr, *sqzi = nullptr;
  int64_t ldt = 0, ldzt = 0;
  int64_t ldf = 0, off_out = 0;
  // the inputs U of a piece into their columns
  int copy_inputs(nk_ctx* ctx, const double* xs, int64_t ldx, int64_t len, double* Fo) const {
    if (p > 0) NK_TRY(launch_copy2d(ctx, xs + d, ldx, Fo + m, ldf, len, p));
    return NK_OK;
  }
  // one piece of `len` rows (xs, ys) into the feature rows at Fo
  // (a piece of ONE row -- a one-row fit, or the one-row tail of the last pass -- is below the two rows the engine's
  // operand contract asks for: direct differences for that piece)
  int piece(nk_ctx* ctx, const double* xs, int64_t ldx, const double* ys, int64_t ldy, int64_t len, double* Fo) const {
    if (gram_form && len >= 2) {
      NK_TRY(prep_rows(ctx, xs, ldx, len, d, winv, center, Rt, ldt, sqr));
      NK_TRY(launch_kmat_gram(ctx, ktype, Rt, ldt, sqr, len, Zti, ldzt, sqzi, m, d, sigma0, Fo, ldf));
      NK_TRY(prep_rows(ctx, ys, ldy, len, d, winv, center, Rt, ldt, sqr));
      NK_TRY(launch_kmat_gram(ctx, ktype, Rt, ldt, sqr, len, Zto, ldzt, sqzo, m, d, sigma0, Fo + off_out, ldf));
    } else {
      NK_TRY(launch_kmat(ctx, ktype, xs, ldx, len, zi.ptr, zi.ld, m, d, winv, sigma0, Fo, ldf));
      NK_TRY(launch_kmat(ctx, ktype, ys, ldy, len, zo.ptr, zo.ld, m, d, winv, sigma0, Fo + off_out, ldf));
    }
    return copy_inputs(ctx, xs, ldx, len, Fo);
  }
};

// the part of nk_fit_stats both fits fill the same way: upload, kernel blocks, Gram stage, the Gram kernel's own time
static void fill_gram_stats(nk_ctx* ctx, nk_fit_stats* stats, bool staged, bool gram_deferred, float ms_gram_kernel,
                            int gram_launches) {
  memset(stats, 0, sizeof(*stats));
  stats->ms_upload = staged ? ev_ms(ctx, EV_FIT_BEGIN, EV_STAGED) : 0.0;
  stats->ms_kmat = ev_ms(ctx, EV_STAGED, EV_KMAT_DONE);
  stats->ms_gram = ev_ms(ctx, EV_KMAT_DONE, EV_GRAM_DONE);
  if (gram_deferred) ms_gram_kernel = ev_ms(ctx, EV_GEMM_T0, EV_GEMM_T1);
  stats->ms_gram_kernel_avg = gram_launches ? ms_gram_kernel / gram_launches : 0.0;
  stats->gram_kernel_launches = gram_launches;
}

// on an early (error) return: drain the streams the fit used before the model buffers go back to the pool.  (Each fit
// names its own streams: in a lock-step group every synchronisation is a barrier, nk_lockstep.h.)
struct FitGuard {
  nk_model* m = nullptr;
  hipStream_t s[5] = {};
  int ns = 0;
  void arm(nk_model* mdl, std::initializer_list<hipStream_t> streams) {
    m = mdl;
    for (hipStream_t q : streams) s[ns++] = q;
  }
  ~FitGuard() {
    if (m) {
      for (int i = 0; i < ns; ++i) (void)hipStreamSynchronize(s[i]);
      nk_model_destroy(m);
    }
  }
};

// ---- the Nystrom fit -------------------------------------------------------------------------------------------------

enum { FIT_FULL = 0, FIT_GRAM = 1, FIT_SOLVE = 2 };

// State of one fit (one of the three entry points: FIT_FULL = nk_nystrom_fit, FIT_GRAM = accumulate the Gram blocks of the given
// rows into gram_io and stop, FIT_SOLVE = start from the accumulated Gram blocks in gram_io, n = total row count).  run()
// calls the stages in the order in which the work is queued.
struct NystromFit {
  // the call's arguments
  nk_ctx* ctx; const nk_kernel_desc* kd;
  const double* X; int64_t ldx; const double* Y; int64_t ldy; int64_t n; int32_t d, p;
  const int64_t* row_ranges; int32_t n_ranges;
  const double* Zin; int64_t ldzi; const double* Zout; int64_t ldzo; int32_t m;
  double gamma, jitter; nk_model** model; nk_fit_stats* stats; int mode; double* gram_io;
  // rows, sizes, the model, the staged matrices
  HostTrace tr;
  std::vector<int64_t> rng;
  int64_t n_eff = 0;
  bool same_centers = false;
  int mp = 0;
  double gamma_n = 0.0;
  nk_model* mdl = nullptr;
  FitGuard guard;
  MatIn x, y, zi, zo;
  int host_passes = 1;
  // landmark matrices, Gram accumulators and their counters
  double *Kmm = nullptr, *Kj = nullptr, *Kj_in = nullptr, *Kxo = nullptr;
  bool landmarks_aside = false, sqrt_early = false;
  double *G1 = nullptr, *G2 = nullptr, *G3 = nullptr, *G4 = nullptr;
  int64_t ldd = 0;
  float ms_gram_kernel = 0.f;
  int gram_launches = 0;
  bool gram_deferred = false, timed = false;
  // feature matrix and passes
  bool f32 = false, overlap_prep = false, multi_pass = false, pipelined = false;
  KernelBlocks kb;
  std::vector<std::vector<Piece>> passes;
  int64_t f_rows = 0, maxlen = 0, ldt32 = 0, ldzt32 = 0, ldy32 = 0;
  double *F = nullptr, *Rt2 = nullptr, *sqr2 = nullptr;
  float *F32 = nullptr, *Rt32 = nullptr, *sq32 = nullptr, *Zt32 = nullptr, *sqz32 = nullptr, *Y32 = nullptr;
  // square root
  SqrtPlan splan;
  int it = 0;
  double resid = 0.0;
  double *Sinvt = nullptr, *T1t = nullptr, *X1 = nullptr;
  // the two regularised systems
  double *Gsave = nullptr, *V1 = nullptr, *Wc = nullptr, *Ct = nullptr;
  CholSys sys[2];
  int chol_failed[2] = {0, 0}, rank_sys[2] = {0, 0}, refined[2] = {0, 0};
  double piv_ratio[2] = {1.0, 1.0}, refine_ratio[2] = {0.0, 0.0};
  bool redo_products = false;

  int run();
  int validate(), stage_rows(), stage_landmarks(), landmark_matrices(), alloc_gram(), load_gram(), prepare_features(), run_passes();
  int upload_pass(size_t ip), pass_f32(size_t ip), pass_f64(size_t ip), blocks_overlapped(const Piece& pc, double* Fo);
  int return_gram();
  bool sqrt_factor_early() const;
  int fence_sqrt_factor(size_t ip);
  int queue_sqrt_prep(), assemble_and_factor(), queue_sqrt_side(), sqrt_products(), operator_products();
  int settle_factorisations(), refine(), settle_sqrt();
  void read_refinement(), write_stats();
};

int NystromFit::validate() {
  NK_TRY(check_ctx(ctx));
  tr.mark("check_ctx/arena_reset");
  NK_REQUIRE(kd && Zout, "nk_nystrom_fit: null argument");
  NK_REQUIRE(mode == FIT_SOLVE || (X && Y), "nk_nystrom_fit: null data pointer");
  NK_REQUIRE(mode == FIT_GRAM || model != nullptr, "nk_nystrom_fit: null model pointer");
  NK_REQUIRE(mode == FIT_FULL || gram_io != nullptr, "nk_nystrom_gram/solve: null accumulator");
  NK_REQUIRE(n > 0 && d > 0 && p >= 0 && m > 0, "nk_nystrom_fit: sizes must be positive (n=%lld d=%d p=%d m=%d)",
             (long long)n, d, p, m);
  NK_REQUIRE(mode == FIT_SOLVE || (ldx >= d + p && ldy >= d), "nk_nystrom_fit: leading dimension too small");
  NK_REQUIRE(ldzo >= d, "nk_nystrom_fit: leading dimension too small");
  NK_REQUIRE(std::isfinite(gamma) && std::isfinite(jitter), "nk_nystrom_fit: gamma/jitter not finite");
  NK_REQUIRE(kd->type != NK_KERNEL_TPS, "nk_nystrom_fit: the thin-plate spline has no Nystrom fit (nk_spline_fit)");
  if (model) *model = nullptr;
  NK_TRY(select_rows("nk_nystrom_fit", row_ranges, n_ranges, n, &rng, &n_eff));
  same_centers = (Zin == nullptr) || (Zin == Zout && ldzi == ldzo);
  mp = m + p;
  gamma_n = gamma * (double)n_eff;  // regressors.py:127

  NK_TRY(model_alloc(ctx, m, d, p, &mdl));
  guard.arm(mdl, {ctx->stream_main, ctx->stream_side, ctx->stream_prep, ctx->stream_la[0], ctx->stream_la[1]});
  mdl->ktype = kd->type; mdl->sigma0 = kd->sigma0; mdl->jitter = jitter;
  tr.mark("validate + model_alloc");
  return NK_OK;
}

// the data rows: uploaded here, or space for the pipelined upload; several row ranges gathered
int NystromFit::stage_rows() {
  // Large HOST arrays (how the reference's fit(X, Y) is called: 620 MB at the headline shape, ~11 ms of PCIe): the rows
  // are uploaded in `host_passes` blocks on the side stream, block k + 1 while the kernel blocks and the Gram launch of
  // block k run (the contraction is accumulated over passes anyway, below).  Only the first block's upload is exposed.
  const char* e = getenv("NYSKOOP_HOST_PASSES");
  const int want = e ? atoi(e) : 6;  // measured at the headline shape: 3 -> 47.5, 4 -> 47.2, 6 -> 46.2, 8 -> 46.6 ms per fit
  if (want > 1 && rng.size() == 2 && !ctx_recording(ctx) && (double)n_eff * (2.0 * d + p) * 8.0 >= 64e6 &&
      !is_device_ptr(X) && !is_device_ptr(Y))
    host_passes = want > 8 ? 8 : want;
  if (host_passes > 1) {
    x.ld = (d + p + 1) & ~(int64_t)1;
    y.ld = (d + 1) & ~(int64_t)1;
    double *xd = nullptr, *yd = nullptr;
    NK_TRY(arena_alloc_t(ctx, (size_t)n * x.ld, &xd));
    NK_TRY(arena_alloc_t(ctx, (size_t)n * y.ld, &yd));
    x.ptr = xd; y.ptr = yd; x.staged = y.staged = true;
  } else {
    NK_TRY(stage_in(ctx, X, ldx, n, d + p, &x));
    NK_TRY(stage_in(ctx, Y, ldy, n, d, &y));
  }
  return gather_ranges(ctx, d, p, n_eff, &rng, &x, &y);
}

int NystromFit::stage_landmarks() {
  NK_TRY(stage_in(ctx, Zout, ldzo, m, d, &zo));
  if (same_centers) zi = zo; else NK_TRY(stage_in(ctx, Zin, ldzi, m, d, &zi));
  NK_TRY(launch_copy2d(ctx, zo.ptr, zo.ld, mdl->Z, d, m, d));
  NK_HIP(hipEventRecord(ctx->ev[EV_STAGED], ctx->stream));
  tr.mark("staging issued");
  return NK_OK;
}

// ---- landmark kernels (regressors.py:139,143,144) -----------------------------------------------------------------
int NystromFit::landmark_matrices() {
  NK_TRY(arena_alloc_t(ctx, (size_t)m * m, &Kmm));
  NK_TRY(arena_alloc_t(ctx, (size_t)m * m, &Kj));
  if (same_centers) {
    Kj_in = Kj;
    Kxo = Kmm;
  } else {
    NK_TRY(arena_alloc_t(ctx, (size_t)m * m, &Kj_in));
    NK_TRY(arena_alloc_t(ctx, (size_t)m * m, &Kxo));
  }
  // Nothing on the main stream needs the landmark matrices before the fused Gram launch has ended (the regularisers of
  // the two systems; the square root's preparation follows them on the preparation stream), and at the headline shape
  // K_mm is 160 us on 16 workgroups: for large fits they are built on the preparation stream, beside the row preparation
  // and the kernel blocks instead of in front of them (EV_LANDMARKS: ready; the main stream waits for it where it
  // assembles the systems).
  {
    const char* la = getenv("NYSKOOP_LANDMARKS_ASIDE");  // 0: on the main stream, in front of the kernel blocks (read per fit: A/B runs)
    landmarks_aside = mode == FIT_FULL && n_eff >= 20000 && m >= 1024 && !ctx_recording(ctx) && !(la && la[0] == '0');
  }
  hipStream_t s0 = ctx->stream;
  if (landmarks_aside) {
    NK_HIP(hipEventRecord(ctx->ev[EV_FORK], ctx->stream));  // the staged landmarks / lengthscales are ready
    ctx->stream = ctx->stream_prep;
    NK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev[EV_FORK], 0));
  }
  int rc_l = launch_kmat(ctx, kd->type, zo.ptr, zo.ld, m, zo.ptr, zo.ld, m, d, mdl->winv, kd->sigma0, Kmm, m);
  if (rc_l == NK_OK) rc_l = launch_copy2d(ctx, Kmm, m, Kj, m, m, m);
  if (rc_l == NK_OK) rc_l = launch_add_diag(ctx, Kj, m, m, jitter);
  if (rc_l == NK_OK && !same_centers) {
    rc_l = launch_kmat(ctx, kd->type, zi.ptr, zi.ld, m, zi.ptr, zi.ld, m, d, mdl->winv, kd->sigma0, Kj_in, m);
    if (rc_l == NK_OK) rc_l = launch_add_diag(ctx, Kj_in, m, m, jitter);
    if (rc_l == NK_OK) rc_l = launch_kmat(ctx, kd->type, zi.ptr, zi.ld, m, zo.ptr, zo.ld, m, d, mdl->winv, kd->sigma0, Kxo, m);
  }
  const hipError_t he = rc_l == NK_OK ? hipEventRecord(ctx->ev[EV_LANDMARKS], ctx->stream) : hipSuccess;  // the landmark matrices are ready
  ctx->stream = s0;
  NK_TRY(rc_l);
  NK_HIP(he);
  return NK_OK;
}

// Gram accumulators (regressors.py:151,153,162,164), one packed block (see gram_doubles):
//   G1 = Phi_in^T Phi_in (symmetric), G2 = Phi_out^T Phi_in (= cross), G3 = Phi_out^T Phi_out (symmetric),
//   G4 = Y^T Phi_out (= left_rec).  G2 sits directly below G1 and G4 below G3: the right-hand sides of the two
//   regularised systems ride along the blocked factorisations as extra rows (cholesky_aug_pair_async).
int NystromFit::alloc_gram() {
  ldd = d + (d & 1);
  NK_TRY(arena_alloc_t(ctx, gram_doubles(m, d, p), &G1));
  G2 = G1 + (size_t)mp * mp;
  G3 = G1 + gram_block1(m, p);
  G4 = G3 + (size_t)m * m;
  timed = stats != nullptr;
  return NK_OK;
}

// FIT_SOLVE: the accumulated Gram blocks come from the caller (host or device memory)
int NystromFit::load_gram() {
  NK_HIP(hipMemcpyAsync(G1, gram_io, gram_doubles(m, d, p) * sizeof(double),
                        is_device_ptr(gram_io) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  NK_HIP(hipEventRecord(ctx->ev[EV_KMAT_DONE], ctx->stream));
  return NK_OK;
}

// ---- feature matrix F = [K_nm_in | U | (pad) | K_nm_out], sample-major (regressors.py:141-142,147), built and
//      contracted in PASSES of at most `pass_rows` rows so that the workspace stays bounded for very large n (the
//      Gram accumulators are updated with beta = 1 from the second pass on); C4 (3.2 GB) is a single pass.
// fp32 engine (nk_set_compute_dtype): the feature matrix, the prepared rows and Y as the operand of G4 are fp32; the
// Gram accumulators come back fp64 (nk_gemm_tn_f32.hip)
int NystromFit::prepare_features() {
  f32 = ctx->compute_f32 != 0 && ctx->kmat_mode == 0 && d >= 32 && !ctx_recording(ctx) && m >= 4 && d >= 4;
  kb.off_out = f32 ? ((mp + 3) & ~3) : ((mp + 1) & ~1);
  kb.ldf = f32 ? ((kb.off_out + m + 3) & ~(int64_t)3) : ((kb.off_out + m + 1) & ~(int64_t)1);
  const int64_t ldf = kb.ldf;
  int64_t pass_rows = pass_rows_for(ldf, f32 ? 4.0 : 8.0);
  if (host_passes > 1) {  // pipelined upload: at least `host_passes` passes (more if the workspace budget says so)
    const int64_t per = ((n_eff + host_passes - 1) / host_passes + 1023) & ~(int64_t)1023;
    if (per < pass_rows) pass_rows = per;
  }
  passes = plan_passes(rng, pass_rows);
  f_rows = passes.size() > 1 ? pass_rows : n_eff;
  NK_TRY(arena_alloc_t(ctx, f32 ? ((size_t)f_rows * ldf + 1) / 2 + 64 : (size_t)f_rows * ldf + 64, &F));
  kb.ktype = kd->type; kb.sigma0 = kd->sigma0; kb.d = d; kb.p = p; kb.m = m; kb.winv = mdl->winv; kb.zi = zi; kb.zo = zo;
  kb.gram_form = ctx->kmat_mode == 0 && d >= 32 && m >= 2;  // (one landmark is below the engine's two operand columns)
  // Gram-form kernel blocks (MFMA engine): rows centred on the landmark mean, scaled by 1/l, transposed
  for (auto& ps : passes) for (auto& pc : ps) maxlen = std::max(maxlen, pc.len);
  kb.ldt = (maxlen + 1) & ~(int64_t)1;
  kb.ldzt = (m + 1) & ~1;
  overlap_prep = kb.gram_form && passes.size() == 1 && passes[0].size() == 1 && maxlen >= 2;
  if (kb.gram_form) {
    NK_TRY(arena_alloc_t(ctx, (size_t)d, &kb.center));
    if (!f32) {
      NK_TRY(arena_alloc_t(ctx, (size_t)d * kb.ldt, &kb.Rt));
      NK_TRY(arena_alloc_t(ctx, (size_t)maxlen, &kb.sqr));
    }
    if (overlap_prep && !f32) {
      NK_TRY(arena_alloc_t(ctx, (size_t)d * kb.ldt, &Rt2));
      NK_TRY(arena_alloc_t(ctx, (size_t)maxlen, &sqr2));
    }
    NK_TRY(arena_alloc_t(ctx, (size_t)d * kb.ldzt, &kb.Zto));
    NK_TRY(arena_alloc_t(ctx, (size_t)m, &kb.sqzo));
    if (kd->type == NK_KERNEL_LINEAR) NK_TRY(launch_fill(ctx, kb.center, d, 1, d, 0.0));  // x.y is not shift invariant
    else NK_TRY(launch_colmean(ctx, zo.ptr, zo.ld, m, d, kb.center));
    NK_TRY(prep_rows(ctx, zo.ptr, zo.ld, m, d, mdl->winv, kb.center, kb.Zto, kb.ldzt, kb.sqzo));
    if (same_centers) {
      kb.Zti = kb.Zto; kb.sqzi = kb.sqzo;
    } else {
      NK_TRY(arena_alloc_t(ctx, (size_t)d * kb.ldzt, &kb.Zti));
      NK_TRY(arena_alloc_t(ctx, (size_t)m, &kb.sqzi));
      NK_TRY(prep_rows(ctx, zi.ptr, zi.ld, m, d, mdl->winv, kb.center, kb.Zti, kb.ldzt, kb.sqzi));
    }
  }
  F32 = reinterpret_cast<float*>(F);
  ldt32 = (maxlen + 3) & ~(int64_t)3; ldzt32 = (m + 3) & ~3; ldy32 = (d + 3) & ~3;
  if (f32) {
    NK_REQUIRE(same_centers, "fp32 engine: separate input landmarks are not supported");
    double* tmp = nullptr;
    NK_TRY(arena_alloc_t(ctx, ((size_t)d * ldt32 + 1) / 2 + 2, &tmp)); Rt32 = reinterpret_cast<float*>(tmp);
    NK_TRY(arena_alloc_t(ctx, ((size_t)maxlen + 1) / 2 + 2, &tmp)); sq32 = reinterpret_cast<float*>(tmp);
    NK_TRY(arena_alloc_t(ctx, ((size_t)d * ldzt32 + 1) / 2 + 2, &tmp)); Zt32 = reinterpret_cast<float*>(tmp);
    NK_TRY(arena_alloc_t(ctx, ((size_t)m + 1) / 2 + 2, &tmp)); sqz32 = reinterpret_cast<float*>(tmp);
    NK_TRY(arena_alloc_t(ctx, ((size_t)f_rows * ldy32 + 1) / 2 + 2, &tmp)); Y32 = reinterpret_cast<float*>(tmp);
    NK_TRY(prep_rows_f32(ctx, zo.ptr, zo.ld, m, d, mdl->winv, kb.center, Zt32, ldzt32, sqz32));
  }
  multi_pass = passes.size() > 1;
  pipelined = host_passes > 1;
  return NK_OK;
}

// upload of the rows of pass ip from the caller's host arrays, on the side stream (the call blocks the HOST while the
// runtime moves pageable memory through its bounce buffers; the device works on the previous pass meanwhile)
int NystromFit::upload_pass(size_t ip) {
  for (const Piece& pc : passes[ip]) {
    NK_HIP(hipMemcpy2DAsync(const_cast<double*>(x.ptr) + pc.b * x.ld, (size_t)x.ld * 8, X + pc.b * ldx, (size_t)ldx * 8,
                            (size_t)(d + p) * 8, (size_t)pc.len, hipMemcpyHostToDevice, ctx->stream_side));
    NK_HIP(hipMemcpy2DAsync(const_cast<double*>(y.ptr) + pc.b * y.ld, (size_t)y.ld * 8, Y + pc.b * ldy, (size_t)ldy * 8,
                            (size_t)d * 8, (size_t)pc.len, hipMemcpyHostToDevice, ctx->stream_side));
  }
  NK_HIP(hipEventRecord(ctx->ev_up[ip & 7], ctx->stream_side));
  return NK_OK;
}

// kernel blocks and Gram contraction pass by pass; with a pipelined upload the rows of pass ip + 1 travel meanwhile
int NystromFit::run_passes() {
  if (pipelined) {
    NK_HIP(hipEventRecord(ctx->ev[EV_FORK], ctx->stream));  // the side stream starts after whatever the main stream has queued
    NK_HIP(hipStreamWaitEvent(ctx->stream_side, ctx->ev[EV_FORK], 0));
    NK_TRY(upload_pass(0));
  }
  for (size_t ip = 0; ip < passes.size(); ++ip) {
    if (pipelined) NK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_up[ip & 7], 0));
    NK_TRY(f32 ? pass_f32(ip) : pass_f64(ip));
    if (pipelined && ip + 1 < passes.size()) NK_TRY(upload_pass(ip + 1));
  }
  return NK_OK;
}

// -- fp32 engine: kernel blocks, then ONE fused Gram launch with fp64 results
int NystromFit::pass_f32(size_t ip) {
  const std::vector<Piece>& ps = passes[ip];
  const double beta = ip == 0 ? 0.0 : 1.0;
  const int64_t ldf = kb.ldf, off_out = kb.off_out;
  int64_t o32 = 0;
  for (const Piece& pc : ps) {
    const double* xs = x.ptr + pc.b * x.ld;
    const double* ys = y.ptr + pc.b * y.ld;
    NK_TRY(prep_rows_f32(ctx, xs, x.ld, pc.len, d, mdl->winv, kb.center, Rt32, ldt32, sq32));
    NK_TRY(launch_kmat_gram_f32(ctx, kd->type, Rt32, ldt32, sq32, pc.len, Zt32, ldzt32, sqz32, m, d, kd->sigma0,
                                F32 + o32 * ldf, ldf));
    NK_TRY(prep_rows_f32(ctx, ys, y.ld, pc.len, d, mdl->winv, kb.center, Rt32, ldt32, sq32));
    NK_TRY(launch_kmat_gram_f32(ctx, kd->type, Rt32, ldt32, sq32, pc.len, Zt32, ldzt32, sqz32, m, d, kd->sigma0,
                                F32 + o32 * ldf + off_out, ldf));
    if (p > 0) NK_TRY(launch_cvt_f64_f32(ctx, xs + d, x.ld, F32 + o32 * ldf + m, ldf, pc.len, p));
    NK_TRY(launch_cvt_f64_f32(ctx, ys, y.ld, Y32 + o32 * ldy32, ldy32, pc.len, d));
    o32 += pc.len;
  }
  if (ip == 0) {
    NK_HIP(hipEventRecord(ctx->ev[EV_KMAT_DONE], ctx->stream));
    tr.mark("kmat issued");
  }
  NK_TRY(fence_sqrt_factor(ip));
  TnProblemF pf[4];
  pf[0].A = F32; pf[0].B = F32; pf[0].lda = pf[0].ldb = ldf; pf[0].M = pf[0].N = mp; pf[0].C = G1; pf[0].ldc = mp;
  pf[0].tri = TRI_UPPER_MIRROR;
  pf[1].A = F32 + off_out; pf[1].B = F32; pf[1].lda = pf[1].ldb = ldf; pf[1].M = m; pf[1].N = mp; pf[1].C = G2; pf[1].ldc = mp;
  pf[2].A = F32 + off_out; pf[2].B = F32 + off_out; pf[2].lda = pf[2].ldb = ldf; pf[2].M = pf[2].N = m; pf[2].C = G3;
  pf[2].ldc = m; pf[2].tri = TRI_UPPER_MIRROR;
  pf[3].A = Y32; pf[3].lda = ldy32; pf[3].M = d; pf[3].N = m; pf[3].C = G4; pf[3].ldc = m; pf[3].B = F32 + off_out;
  pf[3].ldb = ldf;
  for (int q = 0; q < 4; ++q) pf[q].beta = beta;
  float ms1 = 0.f;
  NK_TRY(launch_gemm_tn_f32_multi(ctx, pf, 4, o32, 0, timed ? &ms1 : nullptr, multi_pass));
  if (multi_pass) ms_gram_kernel += ms1; else gram_deferred = timed;
  gram_launches += 1;
  return NK_OK;
}

// Gram-form kernel blocks of a fit that is a single piece: the (HBM-bound) preparation of the Y rows runs on the side
// stream beside the (MFMA-bound) kernel block of the X rows, into its own scratch
int NystromFit::blocks_overlapped(const Piece& pc, double* Fo) {
  const double* xs = x.ptr + pc.b * x.ld;
  const double* ys = y.ptr + pc.b * y.ld;
  NK_HIP(hipEventRecord(ctx->ev[EV_FORK], ctx->stream));  // landmarks, centre and the staged data are ready
  {
    SideScope side(ctx);
    NK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev[EV_FORK], 0));
    NK_TRY(prep_rows(ctx, ys, y.ld, pc.len, d, mdl->winv, kb.center, Rt2, kb.ldt, sqr2));
    NK_HIP(hipEventRecord(ctx->ev[EV_YPREP_DONE], ctx->stream));
  }
  NK_TRY(prep_rows(ctx, xs, x.ld, pc.len, d, mdl->winv, kb.center, kb.Rt, kb.ldt, kb.sqr));
  NK_TRY(launch_kmat_gram(ctx, kd->type, kb.Rt, kb.ldt, kb.sqr, pc.len, kb.Zti, kb.ldzt, kb.sqzi, m, d, kd->sigma0, Fo, kb.ldf));
  NK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev[EV_YPREP_DONE], 0));
  NK_TRY(launch_kmat_gram(ctx, kd->type, Rt2, kb.ldt, sqr2, pc.len, kb.Zto, kb.ldzt, kb.sqzo, m, d, kd->sigma0,
                          Fo + kb.off_out, kb.ldf));
  return kb.copy_inputs(ctx, xs, x.ld, pc.len, Fo);
}

// fp64: kernel blocks of the pass, then its contraction
int NystromFit::pass_f64(size_t ip) {
  const std::vector<Piece>& ps = passes[ip];
  const double beta = ip == 0 ? 0.0 : 1.0;
  const int64_t ldf = kb.ldf, off_out = kb.off_out;
  // -- kernel blocks of this pass
  int64_t o = 0;
  for (const Piece& pc : ps) {
    if (overlap_prep) NK_TRY(blocks_overlapped(pc, F + o * ldf));
    else NK_TRY(kb.piece(ctx, x.ptr + pc.b * x.ld, x.ld, y.ptr + pc.b * y.ld, y.ld, pc.len, F + o * ldf));
    o += pc.len;
  }
  const int64_t rows = o;
  if (ip == 0) {
    NK_HIP(hipEventRecord(ctx->ev[EV_KMAT_DONE], ctx->stream));
    tr.mark("kmat issued");
  }
  // -- contraction of this pass: ONE fused launch when the operands meet the LDS-DMA alignment contract
  NK_TRY(fence_sqrt_factor(ip));
  TnProblem pr[4];
  pr[0].A = F; pr[0].B = F; pr[0].lda = pr[0].ldb = ldf; pr[0].M = pr[0].N = mp; pr[0].C = G1; pr[0].ldc = mp;
  pr[0].tri = TRI_UPPER_MIRROR;
  pr[1].A = F + off_out; pr[1].B = F; pr[1].lda = pr[1].ldb = ldf; pr[1].M = m; pr[1].N = mp; pr[1].C = G2;
  pr[1].ldc = mp;
  pr[2].A = F + off_out; pr[2].B = F + off_out; pr[2].lda = pr[2].ldb = ldf; pr[2].M = pr[2].N = m; pr[2].C = G3;
  pr[2].ldc = m; pr[2].tri = TRI_UPPER_MIRROR;
  pr[3].A = y.ptr + ps[0].b * y.ld; pr[3].lda = y.ld; pr[3].M = d; pr[3].N = m; pr[3].C = G4; pr[3].ldc = m;
  pr[3].B = F + off_out; pr[3].ldb = ldf;
  for (int q = 0; q < 4; ++q) pr[q].beta = beta;
  const bool single = ps.size() == 1;
  const bool fast = tn_fast_ok(pr[0]) && tn_fast_ok(pr[1]) && tn_fast_ok(pr[2]);
  const bool fast_y = fast && tn_fast_ok(pr[3]);
  bool y_done = false;
  if (fast) {
    const int np = (single && fast_y) ? 4 : 3;
    float ms1 = 0.f;
    // (pipelined uploads: no per-launch timing, it would make the host wait for the launch before the next upload)
    NK_TRY(launch_gemm_tn_multi(ctx, pr, np, rows, 0, (timed && !pipelined) ? &ms1 : nullptr, multi_pass));
    if (multi_pass) ms_gram_kernel += ms1; else gram_deferred = timed;
    gram_launches += 1;
    y_done = np == 4;
  } else {  // m = 1, below the contract's two columns: generic engine.  (An odd m + p does not come here: F is padded to
            // even columns, off_out and ldf are even, so its operands meet the contract; only ldc = m + p is odd.)
    GemmOpts sym;
    sym.tri = TRI_UPPER_MIRROR;
    float t3[3] = {0.f, 0.f, 0.f};
    NK_TRY(launch_gemm(ctx, true, false, mp, mp, rows, 1.0, F, ldf, F, ldf, beta, G1, mp, sym, timed ? &t3[0] : nullptr));
    NK_TRY(launch_gemm(ctx, true, false, m, mp, rows, 1.0, F + off_out, ldf, F, ldf, beta, G2, mp, GemmOpts(),
                       timed ? &t3[1] : nullptr));
    NK_TRY(launch_gemm(ctx, true, false, m, m, rows, 1.0, F + off_out, ldf, F + off_out, ldf, beta, G3, m, sym,
                       timed ? &t3[2] : nullptr));
    ms_gram_kernel += t3[0] + t3[1] + t3[2];
    gram_launches += 3;
  }
  if (!y_done) {
    int64_t oo = 0;
    bool first = true;
    for (const Piece& pc : ps) {
      NK_TRY(launch_gemm(ctx, true, false, d, m, pc.len, 1.0, y.ptr + pc.b * y.ld, y.ld, F + oo * ldf + off_out, ldf,
                         (first && ip == 0) ? 0.0 : 1.0, G4, m));
      oo += pc.len;
      first = false;
    }
  }
  return NK_OK;
}

// FIT_GRAM: hand the accumulated blocks to the caller and stop (the model only carried the kernel parameters)
int NystromFit::return_gram() {
  NK_HIP(hipMemcpyAsync(gram_io, G1, gram_doubles(m, d, p) * sizeof(double),
                        is_device_ptr(gram_io) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  if (stats) {
    fill_gram_stats(ctx, stats, x.staged || y.staged, gram_deferred, ms_gram_kernel, gram_launches);
    stats->ms_total = ev_ms(ctx, EV_FIT_BEGIN, EV_GRAM_DONE);
  }
  if (ctx->arena.chunks.size() > 1 || ctx->arena_side.chunks.size() > 1) NK_TRY(arena_reset(ctx));
  return NK_OK;  // the guard returns the model buffers to the pool
}

// ---- the matrix square root S = (K_mm + jitter I)^{1/2}, S^-1 (regressors.py:140,163) runs beside the main stream's work in
//      two parts, queue_sqrt_prep and queue_sqrt_side: the latency-bound preparation (preparation stream) and the GEMM-bound
//      iteration with the products that depend on S only (side stream).  The iteration runs behind the fused Gram launch,
//      beside the factorisation of the regularised systems; where the preparation runs is queue_sqrt_prep's schedule.
//      (Round 3 also measured the whole square root queued BEFORE the Gram launch, beside the kernel blocks, with the Gram
//      launch waiting for it: 44.5 against 42.9 ms per fit -- the factorisation was a chain of ~100 small kernels then, each
//      waiting for a workgroup slot of the long-running kernel blocks; the square root took 13 ms there instead of 9, and
//      what the tail gained (the factorisation chain alone: 4.2 ms) the wait gave back.  Only the preparation, now one
//      dataflow launch, goes there.)

// products that depend on the square root only (current stream)
int NystromFit::sqrt_products() {
  NK_TRY(launch_transpose(ctx, mdl->Sinv, m, Sinvt, m, m, m));
  if (same_centers) {
    // K_xo = K_mm = S^2 - jitter I, hence K_xo S^-1 = S - jitter S^-1: no product (and a smaller rounding error than
    // the product, whose terms are ||K|| ||S^-1|| large)
    NK_TRY(launch_copy2d(ctx, mdl->S, m, T1t, m, m, m));
    NK_TRY(launch_axpby2d(ctx, -jitter, mdl->Sinv, m, 1.0, T1t, m, m, m));
  } else {
    NK_TRY(launch_transpose(ctx, Kxo, m, X1, m, m, m));
    NK_TRY(launch_gemm(ctx, true, false, m, m, m, 1.0, X1, m, mdl->Sinv, m, 0.0, T1t, m));
  }
  return NK_OK;
}

// Schedule of the preparation (queue_sqrt_prep) in a large fit whose factorisations are dataflow launches: true = queued as
// soon as the landmark matrices are, beside the kernel blocks, and fenced from the fused Gram launch (fence_sqrt_factor);
// false = queued behind the Gram launch, where NYSKOOP_PREP_PAUSE (read per fit: A/B runs) says what it waits for.
bool NystromFit::sqrt_factor_early() const {
  if (mode != FIT_FULL || n_eff < 20000 || m < 1024 || ctx_recording(ctx)) return false;
  if (ctx->chol_flow_off || !chol_flow_enabled()) return false;  // launch-per-step chain: the fractional pause below
  const char* e = getenv("NYSKOOP_PREP_PAUSE");
  return !(e && e[0]);
}

// The first fused Gram launch of a fit waits for the early-queued preparation (EV_SQRT_PREPARED, recorded behind
// tri_scale_both).  The factorisation is done by then and the wait is free; were it ever slow to become resident, the
// Gram launch starts late by the rest of that launch instead of sharing its first round of workgroups with it.
int NystromFit::fence_sqrt_factor(size_t ip) {
  if (sqrt_early && ip == 0) NK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev[EV_SQRT_PREPARED], 0));
  return NK_OK;
}

// Cholesky factor of K_mm + jitter and its inverse, the latency-bound half of the square root, on the preparation stream
int NystromFit::queue_sqrt_prep() {
  SideScope prep(ctx, ctx->stream_prep);
  NK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev[EV_LANDMARKS], 0));
  // kernel matrices are positive semi-definite: the jitter bounds the smallest eigenvalue of K_mm + jitter I from
  // below, which lets the iteration be queued before this factorisation has run (SqrtPlan::lambda_min_hint)
  splan.lambda_min_hint = jitter > 0.0 ? jitter : 0.0;
  // The factorisation must not run beside the fused Gram launch: that launch fills the chip in exact rounds of 3-ms
  // workgroups, and a Gram workgroup whose slot the factorisation holds at a round boundary finds the next free slot a
  // whole round later (measured with the launch-per-step chain: the launch takes 26.5-27.0 ms inside the fit against 25.0
  // alone).  It needs the landmarks only, so as ONE dataflow launch it runs beside the kernel blocks, queued ahead of
  // their 12 512 workgroups, and the Gram launch is fenced from it.  The square-root iteration then starts when the Gram
  // launch ends instead of 2 ms later, and the tail is 0.9 ms shorter.  What the kernel blocks pay decides the width: a
  // workgroup of the launch takes one of the two slots of their engine on its CU, and the engine's lone workgroup there
  // does not make up for it (its exp epilogue, it seems, no longer hides behind the other's MFMA).  Headline fit, same
  // process, alternating, 5 x 12 fits, fit less Gram stage (ms): behind the Gram 14.0-14.1; here with 128 workgroups 14.0-14.2
  // (kernel blocks 5.75 -> 6.65: nothing gained); 96: 13.7-13.9; 64: 13.6-13.75 (kernel blocks 6.2); 48: 13.6-13.7; 32:
  // the launch (6.3-6.9 ms) outlasts the kernel blocks and the Gram starts 0.5 ms late.  So a quarter of the CUs where
  // the kernel blocks last as long as such a launch -- 5.7-6.0 ms beside them at m = 2000, growing as m^3, against 5.8 ms
  // of kernel blocks at n = 1e5, d = 384, growing as n m d: n d >= 9 m^2 --, half of them (2.2 ms) otherwise.  bench.py,
  // 5 interleaved runs against the build before: 39.98-40.51 against 40.60-40.92 ms per fit (median -0.54 ms).
  // NYSKOOP_PREP_PAUSE unset: that schedule.  Set, with dataflow factorisations: queued behind the Gram launch; 0 (any
  // value below 1) waits for the Gram's end -- the schedule before this one --, 1 does not wait.  On the launch-per-step
  // chain (NYSKOOP_CHOL_FLOW=0) it is queued behind the Gram launch and the value is the fraction of the block steps to
  // run BEFORE the wait, beside the kernel blocks (1 = never wait; default 0).  Measured on one box with that chain, ms
  // per fit: 1 -> 44.1, 0.75 -> 44.1, 0.5 -> 43.2, 0.25 -> 43.2, 0 -> 42.9 (kernel blocks 6.9 -> 6.3, Gram 26.7 -> 25.5).
  if (!sqrt_early && mode == FIT_FULL && n_eff >= 20000 && m >= 1024) {
    const char* e = getenv("NYSKOOP_PREP_PAUSE");
    const double frac = e ? atof(e) : 0.0;
    const int nb = (m + CHOL_NB - 1) / CHOL_NB;
    if (frac < 1.0) {
      splan.pause_event = ctx->ev_fork;  // recorded behind the last Gram launch
      splan.pause_step = std::max(0, std::min(nb - 1, (int)(frac * nb)));
    }
  }
  const bool narrow = sqrt_early && (double)n_eff * d >= 9.0 * (double)m * m;
  FlowWidth width(ctx, narrow ? std::max(1, ctx->num_cu / 4) : 0);
  NK_TRY(sqrtm_prepare(ctx, Kj, m, m, &splan));
  NK_HIP(hipEventRecord(ctx->ev[EV_SQRT_PREPARED], ctx->stream));
  return NK_OK;
}

// ---- the two regularised systems (regressors.py:151,162) are assembled, factorised AND solved on the main stream
//      without waiting for the square root: with inner and inner_rec symmetric,
//        [A B] = S^-1 (cross inner^-1) blkdiag(K_xo S^-1, I)            cross = G2     (regressors.py:152-156)
//        C     = (left_rec inner_rec^-1) S                               left_rec = G4  (regressors.py:163-166)
//      so the right-hand sides are cross^T (m columns) and left_rec^T (only d columns instead of the reference's m).
int NystromFit::assemble_and_factor() {
  if (landmarks_aside) NK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev[EV_LANDMARKS], 0));  // (long done: built beside the kernel blocks)
  NK_TRY(launch_axpby2d(ctx, gamma_n, Kj_in, m, 1.0, G1, mp, m, m));               // inner = G1 + gamma_n*blkdiag(K, I)
  if (p > 0) NK_TRY(launch_add_diag(ctx, G1 + (int64_t)m * mp + m, mp, p, gamma_n));
  NK_TRY(launch_axpby2d(ctx, gamma_n, Kj, m, 1.0, G3, m, m, m));                   // inner_rec = gamma_n K + G3
  // The factorisations below work in place.  A copy of the assembled systems and their right-hand sides (one device
  // copy of the packed block: 0.1 % of a fit) is what the rank-truncating fallback starts from if a pivot turns out
  // non-positive (regressors.py:155,165: lstsq / gelsd semantics).
  NK_TRY(arena_alloc_t(ctx, gram_doubles(m, d, p), &Gsave));
  NK_HIP(hipMemcpyAsync(Gsave, G1, gram_doubles(m, d, p) * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  double *Linv = nullptr, *Linv2 = nullptr, *pivlog = nullptr;
  const int nblk = (mp + CHOL_NB - 1) / CHOL_NB;
  NK_TRY(arena_alloc_t(ctx, (size_t)nblk * CHOL_WS, &Linv));
  NK_TRY(arena_alloc_t(ctx, (size_t)nblk * CHOL_WS, &Linv2));
  NK_TRY(arena_alloc_t(ctx, (size_t)m * m, &V1));
  // (the square root's outputs S^-T, K_xo S^-1 and a scratch live in the main arena: the operator products read them)
  NK_TRY(arena_alloc_t(ctx, (size_t)m * m, &Sinvt));
  NK_TRY(arena_alloc_t(ctx, (size_t)m * m, &T1t));
  NK_TRY(arena_alloc_t(ctx, (size_t)m * m, &X1));
  NK_TRY(arena_alloc_t(ctx, (size_t)m * ldd, &Wc));
  NK_TRY(arena_alloc_t(ctx, (size_t)m * ldd, &Ct));
  NK_TRY(arena_alloc_t(ctx, (size_t)mp + m + 4, &pivlog));
  sys[0].P = G1; sys[0].ldp = mp; sys[0].m = mp; sys[0].Linv = Linv; sys[0].extra = m;   // [inner; cross]
  sys[1].P = G3; sys[1].ldp = m; sys[1].m = m; sys[1].Linv = Linv2; sys[1].extra = d;    // [inner_rec; left_rec]
  sys[0].pivlog = pivlog; sys[1].pivlog = pivlog + mp + (mp & 1);
  // both systems advance in lock step (paired launches); the per-block kernels are latency bound and leave the chip
  // mostly idle ...
  // (With the square root prepared ahead of the Gram launch, the iteration runs beside this factorisation from its first
  // step on, and each of its workgroups costs the iteration's GEMMs a slot: same measurement as in queue_sqrt_prep, fit less
  // Gram stage with 256 / 192 / 128 / 96 / 80 / 64 workgroups here: 14.1 / 13.9 / 13.7 / 13.5 / 13.65 / 14.05 ms.)
  FlowWidth width(ctx, sqrt_early ? std::max(1, 3 * ctx->num_cu / 8) : 0);
  NK_TRY(cholesky_aug_pair_async(ctx, sys, 2));  // G2 <- cross inner^-1 (m x mp) ; G4 <- left_rec inner_rec^-1 (d x m)
  // (tried: holding the GEMM-bound iteration back until this latency-bound chain is done -- 43.3 against 42.7 ms per fit;
  // with look-ahead in both chains 43.7 / 47.5: the overlap of the two, slow as each becomes, is still the best schedule)
  tr.mark("cholesky + solves issued");
  return NK_OK;
}

// the GEMM-bound iteration, then S^-T and K_xo S^-1, on the side stream
int NystromFit::queue_sqrt_side() {
  SideScope side(ctx);
  NK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_fork, 0));  // starts when the Gram launch is done
  NK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev[EV_SQRT_PREPARED], 0));
  NK_HIP(hipEventRecord(ctx->ev[EV_SQRT_BEGIN], ctx->stream));
  NK_TRY(sqrtm_finish(ctx, &splan, mdl->S, mdl->Sinv));
  NK_HIP(hipEventRecord(ctx->ev[EV_SQRT_END], ctx->stream));
  // still on the side stream (the factorisation chain is usually not finished yet): S^-T and K_xo S^-1
  NK_TRY(sqrt_products());
  NK_HIP(hipEventRecord(ctx->ev_join, ctx->stream));
  return NK_OK;
}

// ---- operator products; every product is P^T Q with P stored contraction-major (fast TN engine) -----------------------
//   [A B] = S^-1 (cross inner^-1) blkdiag(K_xo S^-1, I)   with  cross inner^-1 = [V1^T | V2^T] in G2
//   (T1t holds K_xo S^-1, computed on the side stream)
int NystromFit::operator_products() {
  NK_TRY(launch_transpose(ctx, G2, mp, V1, m, m, m));                                         // V1 (m x m)
  NK_TRY(launch_gemm(ctx, true, false, m, m, m, 1.0, V1, m, T1t, m, 0.0, X1, m));             // X1 = V1^T (K_xo S^-1)
  NK_TRY(launch_gemm(ctx, true, false, m, m, m, 1.0, Sinvt, m, X1, m, 0.0, mdl->A, mp));      // A = S^-1 X1
  if (p > 0) NK_TRY(launch_gemm(ctx, true, false, m, p, m, 1.0, Sinvt, m, G2 + m, mp, 0.0, mdl->B, mp));  // B = S^-1 V2^T
  //   C = (left_rec inner_rec^-1) S : C^T = S^T Wc with Wc = G4^T
  NK_TRY(launch_transpose(ctx, G4, m, Wc, ldd, d, m));
  NK_TRY(launch_gemm(ctx, true, false, m, d, m, 1.0, mdl->S, m, Wc, ldd, 0.0, Ct, ldd));      // C^T = S^T Wc
  NK_TRY(launch_transpose(ctx, Ct, ldd, mdl->C, m, m, d));
  NK_TRY(launch_gemm(ctx, true, false, d, mp, m, 1.0, Ct, ldd, mdl->A, mp, 0.0, mdl->W, mp));  // W = C G (:167)
  return NK_OK;
}

// verdict of the two factorisations: the give-up re-run of the dataflow launch, the strict modes, the rank-truncating fallback
int NystromFit::settle_factorisations() {
  NK_TRY(cholesky_fail_flags(ctx, sys, 2, chol_failed, piv_ratio));  // synchronises the main stream (which has joined the side stream)
  tr.mark("final sync");
  bool chol_rerun = false;
  if (chol_failed[0] == CHOL_FLOW_GIVEUP || chol_failed[1] == CHOL_FLOW_GIVEUP) {
    // the dataflow factorisation gave up waiting: both systems once more from the saved copy, on the launch-per-step chain
    ChainOnly chain(ctx);
    NK_HIP(hipMemcpyAsync(G1, Gsave, gram_doubles(m, d, p) * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    NK_TRY(cholesky_aug_pair_async(ctx, sys, 2));
    NK_TRY(cholesky_fail_flags(ctx, sys, 2, chol_failed, piv_ratio));
    chol_rerun = true;
  }
  rank_sys[0] = mp; rank_sys[1] = m;
  redo_products = chol_rerun;
  if (ctx->strict_spd == 2) chol_failed[0] = chol_failed[1] = -1;  // lstsq-shaped: always the SVD with gelsd's cut-off
  if (chol_failed[0] || chol_failed[1]) {
    if (ctx->strict_spd == 1) {  // NK_ERR_NOT_SPD
      set_error("Cholesky: system %d is numerically rank deficient (non-positive or rounding-level pivot; the reference's "
                "lstsq truncates here) and strict mode is on", chol_failed[0] ? 0 : 1);
      return NK_ERR_NOT_SPD;
    }
    // numerically rank-deficient system(s): lstsq's (gelsd's) minimum-norm solution, singular values <= eps * sigma_max
    // dropped (nk_pinv.hip)
    const double rcond = 2.220446049250313e-16;
    for (int q = 0; q < 2; ++q) {
      if (!chol_failed[q]) continue;
      PinvInfo pi;
      if (q == 0)  // cross inner^+  ->  G2
        NK_TRY(pinv_right_divide(ctx, Gsave, mp, mp, Gsave + (size_t)mp * mp, mp, m, G2, mp, rcond, &pi));
      else         // left_rec inner_rec^+  ->  G4
        NK_TRY(pinv_right_divide(ctx, Gsave + gram_block1(m, p), m, m, Gsave + gram_block1(m, p) + (size_t)m * m, m, d, G4,
                                 m, rcond, &pi));
      if (!pi.converged) {
        set_error("rank-revealing fallback: Jacobi SVD of system %d did not converge in %d sweeps", q, pi.sweeps);
        return NK_ERR_NO_CONVERGENCE;
      }
      rank_sys[q] = pi.rank;
    }
    // (tried in round 3: solving the systems whose pivots decay gradually through the rounding level -- no spectral gap,
    // the gamma = 1e-7 candidates of the cloth grid -- by a minimally shifted Cholesky instead of the SVD.  4 x faster grid
    // (0.29 s), but a shift of 4 m eps ||P|| is 2000 x gelsd's eps sigma_max cut-off: 15 of the 405 units moved 1.5e-2 .. 0.37
    // away from the reference's score, against <= 1e-2 with the SVD.  Dropped.)
    count_event(CNT_RANK_TRUNCATED);
    redo_products = true;
  }
  return NK_OK;
}

// ---- optional refinement of ill-conditioned systems (nk_set_refine / NYSKOOP_REFINE_PIVOT; off by default).  Each step
//      forms the residual R - X inner from the SAVED system in doubled precision (launch_resid_dd: a plain fp64 residual
//      is all rounding error and makes things worse) and solves for the correction with the same factor; a step is
//      applied only while the corrections contract (decided on the device).  The solution then is the system's own to
//      working precision -- what is left against the reference is the reference's rounding (gelsd) and the Gram
//      products' summation order.  With the backward-stable blocked solve (chol_panel_kernel) this buys little: config 2
//      A 1.5e-4 -> 1.15e-4 from the reference whose own row-order spread is 1.0e-4; it costs 10 flop per term on the
//      vector ALU (0.15 s on the 405-unit cloth grid), hence opt-in.
int NystromFit::refine() {
  const double refine_below = ctx->refine_pivot;
  const int refine_steps = ctx->refine_steps;
  double* refine_state = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)8, &refine_state));
  for (int q = 0; q < 2 && refine_steps > 0; ++q) {
    if (chol_failed[q] || !(piv_ratio[q] > 0.0) || piv_ratio[q] >= refine_below) continue;
    const int mq = sys[q].m, nr = sys[q].extra;                       // system size, number of right-hand sides (rows)
    const size_t off = q == 0 ? 0 : gram_block1(m, p);
    const double* Pq = Gsave + off;                                   // saved system (symmetric)
    const double* Rq = Gsave + off + (size_t)mq * mq;                 // saved right-hand-side rows (nr x mq)
    double* Xq = G1 + off + (size_t)mq * mq;                          // solution rows (nr x mq) = R P^-1
    const ArenaMark mk = arena_mark(ctx);
    double *Res = nullptr, *ResT = nullptr, *partial = nullptr;
    const int64_t ldt_ = nr + (nr & 1);
    NK_TRY(arena_alloc_t(ctx, (size_t)nr * mq, &Res));
    NK_TRY(arena_alloc_t(ctx, (size_t)mq * ldt_, &ResT));
    NK_TRY(arena_alloc_t(ctx, (size_t)2 * refine_partial_blocks(), &partial));
    CholSys cs = sys[q];
    cs.R = ResT; cs.ldr = ldt_; cs.nrhs = nr;
    for (int step = 0; step < refine_steps; ++step) {
      NK_TRY(launch_resid_dd(ctx, Xq, mq, Pq, mq, Rq, mq, Res, mq, nr, mq));                    // Res = R - X P
      NK_TRY(launch_transpose(ctx, Res, mq, ResT, ldt_, nr, mq));                               // columns for the solve
      NK_TRY(cholesky_solve_pair(ctx, &cs, 1));                                                 // P dX^T = Res^T
      NK_TRY(launch_transpose(ctx, ResT, ldt_, Res, mq, mq, nr));
      // X += dX while the corrections contract (a numerically singular system that happened to factor is left alone)
      NK_TRY(launch_refine_apply(ctx, Res, mq, Xq, mq, nr, mq, step, refine_state + 4 * q, partial));
    }
    NK_HIP(hipMemcpyAsync(ctx->h_scalars + HS_REFINE + 4 * q, refine_state + 4 * q, 4 * sizeof(double), hipMemcpyDeviceToHost,
                          ctx->stream));
    arena_release(ctx, mk);
    refined[q] = -1;  // verdict in h_scalars[HS_REFINE + 4 q ..] after the synchronisation that follows (read_refinement)
    redo_products = true;
  }
  return NK_OK;
}

// verdict of the square root (the iteration was queued without host round trips) and its two retry branches
int NystromFit::settle_sqrt() {
  const int vr = sqrtm_verdict(ctx, &splan, &it, &resid);
  if (vr == NK_SQRT_RETRY && splan.flow_gave_up) {
    // the dataflow factorisation of K_mm gave up waiting: the square root once more with the launch-per-step chain,
    // then everything that depends on it
    // (in the same early-queued form, i.e. with the same eigenvalue bound and scaling schedule: the synchronous form would
    // converge to the same square root along other iterates, and the recovered fit would differ from an undisturbed one
    // in its last bits)
    ChainOnly chain(ctx);
    SqrtPlan again;
    again.lambda_min_hint = splan.lambda_min_hint;
    NK_TRY(sqrtm_prepare(ctx, Kj, m, m, &again));
    NK_TRY(sqrtm_finish(ctx, &again, mdl->S, mdl->Sinv));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    const int vr2 = sqrtm_verdict(ctx, &again, &it, &resid);
    if (vr2 == NK_SQRT_RETRY) {  // the chain's verdict: not positive definite to working precision
      count_event(CNT_SQRT_RETRY);
      NK_TRY(sqrtm_spd_coupled(ctx, Kj, m, m, mdl->S, mdl->Sinv, &it, &resid));
    } else {
      NK_TRY(vr2);
    }
    NK_TRY(sqrt_products());
    redo_products = true;
  } else if (vr == NK_SQRT_RETRY) {
    count_event(CNT_SQRT_RETRY);
    // K_mm + jitter I is not positive definite to working precision (or the eigenvalue bound did not hold): the
    // coupled iteration needs no factorisation; then everything that depends on the square root once more
    NK_TRY(sqrtm_spd_coupled(ctx, Kj, m, m, mdl->S, mdl->Sinv, &it, &resid));
    NK_TRY(sqrt_products());
    redo_products = true;
  } else {
    NK_TRY(vr);
  }
  return NK_OK;
}

// what the refinement steps left in the host mirror (the stream has been synchronised since they were queued)
void NystromFit::read_refinement() {
  for (int q = 0; q < 2; ++q)
    if (refined[q] < 0) {
      refined[q] = (int)ctx->h_scalars[HS_REFINE + 4 * q + 2];  // steps accepted by the contraction guard
      refine_ratio[q] = ctx->h_scalars[HS_REFINE + 4 * q + 3];
    }
  if (refined[0] > 0 || refined[1] > 0) count_event(CNT_REFINED);
}

void NystromFit::write_stats() {
  fill_gram_stats(ctx, stats, x.staged || y.staged, gram_deferred, ms_gram_kernel, gram_launches);
  stats->ms_total = ev_ms(ctx, EV_FIT_BEGIN, EV_FIT_END);
  stats->ms_sqrt = ev_ms(ctx, EV_SQRT_BEGIN, EV_SQRT_END);  // on the side stream, overlapping the kernel-block and Gram stages
  stats->ms_solve = ev_ms(ctx, EV_SOLVE_BEGIN, EV_FIT_END);
  stats->sqrt_iters = it;
  stats->sqrt_residual = resid;
  const double ne = (double)n_eff;
  const double t128 = 128.0;
  auto tiles = [&](double v) { return std::ceil(v / t128); };
  const double tmp_ = tiles(mp), tm_ = tiles(m);
  // flop actually issued by the three big tile sets (upper-triangular tile sets for the symmetric Grams)
  stats->gram_flops = 2.0 * ne * t128 * t128 * (tmp_ * (tmp_ + 1) / 2 + tm_ * tmp_ + tm_ * (tm_ + 1) / 2) +
                      2.0 * ne * (double)d * m;
  stats->kmat_pairs = 2.0 * ne * m * d + (same_centers ? 1.0 : 3.0) * (double)m * m * d;
  stats->rank_inner = rank_sys[0];
  stats->rank_inner_rec = rank_sys[1];
  stats->pivot_ratio_inner = piv_ratio[0];
  stats->pivot_ratio_inner_rec = piv_ratio[1];
  stats->refined = refined[0] + 16 * refined[1];
  stats->refine_ratio_inner = refine_ratio[0];
  stats->refine_ratio_inner_rec = refine_ratio[1];
}


// The schedule of a fit: the order of the calls below is the order in which the work is queued.
int NystromFit::run() {
  NK_TRY(validate());
  NK_HIP(hipEventRecord(ctx->ev[EV_FIT_BEGIN], ctx->stream));
  NK_TRY(make_winv(ctx, kd, d, mdl->winv));
  if (mode != FIT_SOLVE) NK_TRY(stage_rows());
  NK_TRY(stage_landmarks());
  if (mode != FIT_GRAM) NK_TRY(landmark_matrices());
  sqrt_early = sqrt_factor_early();
  if (sqrt_early) NK_TRY(queue_sqrt_prep());  // preparation stream, beside the kernel blocks
  NK_TRY(alloc_gram());
  if (mode == FIT_SOLVE) {
    NK_TRY(load_gram());
  } else {
    NK_TRY(prepare_features());
    NK_TRY(run_passes());
  }
  NK_HIP(hipEventRecord(ctx->ev[EV_GRAM_DONE], ctx->stream));
  if (mode == FIT_GRAM) return return_gram();

  NK_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));  // the square-root iteration starts when the Gram launch is done
  tr.mark("gram issued");
  if (!sqrt_early) NK_TRY(queue_sqrt_prep());  // preparation stream
  NK_TRY(assemble_and_factor());  // main stream
  NK_TRY(queue_sqrt_side());      // side stream
  NK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
  NK_HIP(hipEventRecord(ctx->ev[EV_SOLVE_BEGIN], ctx->stream));
  tr.mark("side stream joined (queued)");
  // (the verdict of the factorisations is read at the end of the call: a blocking check here would leave the GPU idle
  // while the host wakes up and queues the products; on a failed factorisation they compute on garbage, harmlessly)
  NK_TRY(operator_products());
  NK_HIP(hipEventRecord(ctx->ev[EV_FIT_END], ctx->stream));
  tr.mark("solve issued");

  NK_TRY(settle_factorisations());  // first host synchronisation of the fit
  NK_TRY(refine());
  NK_TRY(settle_sqrt());
  if (redo_products) {
    NK_TRY(operator_products());
    NK_HIP(hipStreamSynchronize(ctx->stream));
  }
  read_refinement();
  mdl->has_ops = true;
  if (stats) write_stats();
  tr.mark("stats");
  if (ctx->arena.chunks.size() > 1 || ctx->arena_side.chunks.size() > 1) NK_TRY(arena_reset(ctx));  // coalesce now (everything is synchronised), not in the next call
  guard.m = nullptr;
  *model = mdl;
  return NK_OK;
}

extern "C" {

int nk_nystrom_fit(nk_ctx* ctx, const nk_kernel_desc* kd, const double* X, int64_t ldx, const double* Y, int64_t ldy,
                   int64_t n, int32_t d, int32_t p, const int64_t* row_ranges, int32_t n_ranges, const double* Zin,
                   int64_t ldzi, const double* Zout, int64_t ldzo, int32_t m, double gamma, double jitter,
                   nk_model** model, nk_fit_stats* stats) {
  NK_REQUIRE(model != nullptr, "nk_nystrom_fit: null argument");
  NystromFit f{ctx, kd, X, ldx, Y, ldy, n, d, p, row_ranges, n_ranges, Zin, ldzi, Zout, ldzo, m, gamma, jitter, model, stats,
               FIT_FULL, nullptr};
  return f.run();
}

int nk_gram_doubles(int32_t m, int32_t d, int32_t p, int64_t* count) {
  NK_REQUIRE(count && m > 0 && d > 0 && p >= 0, "nk_gram_doubles: bad argument");
  *count = (int64_t)gram_doubles(m, d, p);
  return NK_OK;
}

int nk_nystrom_gram(nk_ctx* ctx, const nk_kernel_desc* kd, const double* X, int64_t ldx, const double* Y, int64_t ldy,
                    int64_t n, int32_t d, int32_t p, const int64_t* row_ranges, int32_t n_ranges, const double* Zin,
                    int64_t ldzi, const double* Zout, int64_t ldzo, int32_t m, double* gram, nk_fit_stats* stats) {
  NystromFit f{ctx, kd, X, ldx, Y, ldy, n, d, p, row_ranges, n_ranges, Zin, ldzi, Zout, ldzo, m, 0.0, 0.0, nullptr, stats,
               FIT_GRAM, gram};
  return f.run();
}

int nk_nystrom_solve(nk_ctx* ctx, const nk_kernel_desc* kd, const double* Zin, int64_t ldzi, const double* Zout,
                     int64_t ldzo, int32_t m, int32_t d, int32_t p, const double* gram, int64_t n_total, double gamma,
                     double jitter, nk_model** model, nk_fit_stats* stats) {
  NK_REQUIRE(model != nullptr, "nk_nystrom_solve: null argument");
  NystromFit f{ctx, kd, nullptr, 0, nullptr, 0, n_total, d, p, nullptr, 0, Zin, ldzi, Zout, ldzo, m, gamma, jitter, model, stats,
               FIT_SOLVE, const_cast<double*>(gram)};
  return f.run();
}

// ---- thin-plate-spline EDMD fit (regressors.py:199-221), fp64 on every path ------------------------------------------
// Feature matrix F = [Phi_x | U | (pad) | Phi_y] in the layout of the Nystrom fit (Phi_x = TPS(X_state, centres),
// Phi_y = TPS(Y, centres)), built and contracted in passes of at most `pass_rows` rows; ONE fused Gram launch per pass
// computes the three products that share the rows:
//   cov = [Phi_x U]^T [Phi_x U]  ((m+p) x (m+p)),  top = Phi_y^T [Phi_x U]  (m x (m+p)),  bot = X_state^T [Phi_x U]  (d x (m+p))
// stored one below the other (leading dimension m+p), so that [top; bot] rides along the blocked Cholesky of
// P = cov + gamma n I as the extra rows of the augmented factorisation and comes out as M_ls = [top; bot] P^-1
// (P is symmetric).  Systems whose condition could reach scipy.linalg.pinv's cut-off (m+p) eps sigma_max take the
// Jacobi pseudo-inverse with that cut-off instead (see SPLINE_SVD_WINDOW).
//
// Which path: the Cholesky pivots d_k (Schur-complement diagonals) of an SPD matrix satisfy sigma_min <= d_k <= sigma_max,
// so min d / max d >= sigma_min / sigma_max: a pivot ratio at or below the cut-off (m+p) eps means pinv certainly
// truncates, but a ratio above it does not prove the opposite.  Measured with the reference's systems (f15 fixtures:
// cloth n = 3030, d = 192, p = 6, m = 10..500, gamma = 1e-7..1e-5; Duffing m = 10..200) the pivot ratio exceeds
// sigma_min / sigma_max by a factor 3 (m = 10) to 172 (m = 500), growing about linearly with m.  The safety window
// therefore scales with the system: every system whose pivot ratio is below 2 (m+p) x (m+p) eps takes the SVD path
// (at m = 500: a window of 1012 against the measured 172).  The Cholesky result is used only above it.
static constexpr double SPLINE_SVD_WINDOW_PER_ROW = 2.0;

int nk_spline_fit(nk_ctx* ctx, const double* X, int64_t ldx, const double* Y, int64_t ldy, int64_t n, int32_t d, int32_t p,
                  const int64_t* row_ranges, int32_t n_ranges, const double* centers, int64_t ldc, int32_t m, double gamma,
                  nk_model** model, nk_fit_stats* stats) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(X && Y && centers && model, "nk_spline_fit: null argument");
  NK_REQUIRE(n > 0 && d > 0 && p >= 0 && m > 0, "nk_spline_fit: sizes must be positive (n=%lld d=%d p=%d m=%d)",
             (long long)n, d, p, m);
  NK_REQUIRE(ldx >= d + p && ldy >= d && ldc >= d, "nk_spline_fit: leading dimension too small");
  NK_REQUIRE(std::isfinite(gamma), "nk_spline_fit: gamma not finite");
  *model = nullptr;
  std::vector<int64_t> rng;
  int64_t n_eff = 0;
  NK_TRY(select_rows("nk_spline_fit", row_ranges, n_ranges, n, &rng, &n_eff));
  // (nk_set_compute_dtype(F32) is ignored here: the spline systems reach cond 1e13, the fit is fp64 only)
  const int mp = m + p;
  const double gamma_n = gamma * (double)n_eff;  // regressors.py:204

  nk_model* mdl = nullptr;
  NK_TRY(model_alloc(ctx, m, d, p, &mdl, NK_MODEL_SPLINE));
  FitGuard guard;
  guard.arm(mdl, {ctx->stream_main, ctx->stream_side});
  mdl->ktype = NK_KERNEL_TPS; mdl->sigma0 = 0.0; mdl->jitter = 0.0;
  NK_HIP(hipEventRecord(ctx->ev[EV_FIT_BEGIN], ctx->stream));
  NK_TRY(launch_fill(ctx, mdl->winv, d, 1, d, 1.0));  // no length scale
  MatIn x, y, zc;
  NK_TRY(stage_in(ctx, X, ldx, n, d + p, &x));
  NK_TRY(stage_in(ctx, Y, ldy, n, d, &y));
  NK_TRY(gather_ranges(ctx, d, p, n_eff, &rng, &x, &y));  // K-fold training set: one contiguous piece
  NK_TRY(stage_in(ctx, centers, ldc, m, d, &zc));
  NK_TRY(launch_copy2d(ctx, zc.ptr, zc.ld, mdl->Z, d, m, d));
  NK_HIP(hipEventRecord(ctx->ev[EV_STAGED], ctx->stream));

  // Gram accumulators [cov ; top ; bot], (m+p+m+d) x (m+p)
  double* G = nullptr;
  const size_t gdoubles = (size_t)(mp + m + d) * mp;
  NK_TRY(arena_alloc_t(ctx, gdoubles, &G));
  double* Gtop = G + (size_t)mp * mp;
  double* Gbot = Gtop + (size_t)m * mp;
  const int64_t off_out = (mp + 1) & ~1;
  const int64_t ldf = (off_out + m + 1) & ~(int64_t)1;
  const int64_t pass_rows = pass_rows_for(ldf, 8.0);
  const std::vector<std::vector<Piece>> passes = plan_passes(rng, pass_rows);
  const bool multi_pass = passes.size() > 1;
  const int64_t f_rows = multi_pass ? pass_rows : n_eff;
  double* F = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)f_rows * ldf + 64, &F));
  // Gram-form kernel blocks (nk_set_kmat_mode: automatic at d >= 32) or direct differences
  KernelBlocks kb;
  kb.ktype = NK_KERNEL_TPS; kb.sigma0 = 0.0; kb.d = d; kb.p = p; kb.m = m; kb.winv = mdl->winv; kb.zi = kb.zo = zc;
  kb.ldf = ldf; kb.off_out = off_out;
  kb.gram_form = ctx->kmat_mode == 0 && d >= 32 && m >= 2;  // (one landmark is below the engine's two operand columns)
  int64_t maxlen = 0;
  for (auto& ps : passes) for (auto& pc : ps) maxlen = std::max(maxlen, pc.len);
  kb.ldt = (maxlen + 1) & ~(int64_t)1;
  kb.ldzt = (m + 1) & ~1;
  if (kb.gram_form) {
    NK_TRY(arena_alloc_t(ctx, (size_t)d, &kb.center));
    NK_TRY(arena_alloc_t(ctx, (size_t)d * kb.ldt, &kb.Rt));
    NK_TRY(arena_alloc_t(ctx, (size_t)maxlen, &kb.sqr));
    NK_TRY(arena_alloc_t(ctx, (size_t)d * kb.ldzt, &kb.Zto));
    NK_TRY(arena_alloc_t(ctx, (size_t)m, &kb.sqzo));
    NK_TRY(launch_colmean(ctx, zc.ptr, zc.ld, m, d, kb.center));  // distances are shift invariant: centred rows cancel less
    NK_TRY(prep_rows(ctx, zc.ptr, zc.ld, m, d, mdl->winv, kb.center, kb.Zto, kb.ldzt, kb.sqzo));
    kb.Zti = kb.Zto; kb.sqzi = kb.sqzo;
  }
  float ms_gram_kernel = 0.f;
  int gram_launches = 0;
  bool gram_deferred = false;
  const bool timed = stats != nullptr;
  for (size_t ip = 0; ip < passes.size(); ++ip) {
    const std::vector<Piece>& ps = passes[ip];
    const double beta = ip == 0 ? 0.0 : 1.0;
    int64_t o = 0;
    for (const Piece& pc : ps) {
      NK_TRY(kb.piece(ctx, x.ptr + pc.b * x.ld, x.ld, y.ptr + pc.b * y.ld, y.ld, pc.len, F + o * ldf));
      o += pc.len;
    }
    const int64_t rows = o;
    if (ip == 0) NK_HIP(hipEventRecord(ctx->ev[EV_KMAT_DONE], ctx->stream));
    TnProblem pr[3];
    pr[0].A = F; pr[0].B = F; pr[0].lda = pr[0].ldb = ldf; pr[0].M = pr[0].N = mp; pr[0].C = G; pr[0].ldc = mp;
    pr[0].tri = TRI_UPPER_MIRROR;
    pr[1].A = F + off_out; pr[1].B = F; pr[1].lda = pr[1].ldb = ldf; pr[1].M = m; pr[1].N = mp; pr[1].C = Gtop;
    pr[1].ldc = mp;
    pr[2].A = x.ptr + ps[0].b * x.ld; pr[2].lda = x.ld; pr[2].M = d; pr[2].N = mp; pr[2].C = Gbot; pr[2].ldc = mp;
    pr[2].B = F; pr[2].ldb = ldf;
    for (int q = 0; q < 3; ++q) pr[q].beta = beta;
    const bool fast = tn_fast_ok(pr[0]) && tn_fast_ok(pr[1]);
    const bool fast_x = fast && ps.size() == 1 && tn_fast_ok(pr[2]);
    if (fast) {
      float ms1 = 0.f;
      NK_TRY(launch_gemm_tn_multi(ctx, pr, fast_x ? 3 : 2, rows, 0, timed ? &ms1 : nullptr, multi_pass));
      if (multi_pass) ms_gram_kernel += ms1; else gram_deferred = timed;
      gram_launches += 1;
    } else {  // operands outside the alignment contract of the fused engine: generic engine
      GemmOpts sym;
      sym.tri = TRI_UPPER_MIRROR;
      NK_TRY(launch_gemm(ctx, true, false, mp, mp, rows, 1.0, F, ldf, F, ldf, beta, G, mp, sym));
      NK_TRY(launch_gemm(ctx, true, false, m, mp, rows, 1.0, F + off_out, ldf, F, ldf, beta, Gtop, mp));
      gram_launches += 2;
    }
    if (!fast_x) {  // bot = X_state^T [Phi_x U], piece by piece
      int64_t oo = 0;
      for (const Piece& pc : ps) {
        NK_TRY(launch_gemm(ctx, true, false, d, mp, pc.len, 1.0, x.ptr + pc.b * x.ld, x.ld, F + oo * ldf, ldf,
                           (oo == 0 && ip == 0) ? 0.0 : 1.0, Gbot, mp));
        oo += pc.len;
      }
    }
  }
  NK_HIP(hipEventRecord(ctx->ev[EV_GRAM_DONE], ctx->stream));

  // ---- M_ls = [top; bot] pinv(P), P = cov + gamma n I (regressors.py:213-214)
  NK_TRY(launch_add_diag(ctx, G, mp, mp, gamma_n));
  double* Gsave = nullptr;  // the assembled system for the pseudo-inverse path (the factorisation works in place)
  NK_TRY(arena_alloc_t(ctx, gdoubles, &Gsave));
  NK_HIP(hipMemcpyAsync(Gsave, G, gdoubles * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  double *Linv = nullptr, *pivlog = nullptr;
  const int nblk = (mp + CHOL_NB - 1) / CHOL_NB;
  NK_TRY(arena_alloc_t(ctx, (size_t)nblk * CHOL_WS, &Linv));
  NK_TRY(arena_alloc_t(ctx, (size_t)mp + 4, &pivlog));
  CholSys sys;
  sys.P = G; sys.ldp = mp; sys.m = mp; sys.Linv = Linv; sys.extra = m + d; sys.pivlog = pivlog;  // [P; top; bot]
  int failed = -1;
  double piv_ratio = 0.0;
  if (ctx->strict_spd != 2) {  // (strict = 2: the SVD whatever the pivots)
    NK_TRY(cholesky_aug_pair_async(ctx, &sys, 1));
    NK_TRY(cholesky_fail_flags(ctx, &sys, 1, &failed, &piv_ratio));  // synchronises
    if (failed == CHOL_FLOW_GIVEUP) {
      ChainOnly chain(ctx);
      NK_HIP(hipMemcpyAsync(G, Gsave, gdoubles * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      NK_TRY(cholesky_aug_pair_async(ctx, &sys, 1));
      NK_TRY(cholesky_fail_flags(ctx, &sys, 1, &failed, &piv_ratio));
    }
  }
  const double eps = 2.220446049250313e-16;
  const double rcond = (double)mp * eps;  // scipy.linalg.pinv: atol = 0, rtol = max(M, N) eps
  int rank = mp;
  const bool use_svd = failed != 0 || !(piv_ratio > SPLINE_SVD_WINDOW_PER_ROW * (double)mp * rcond);
  if (use_svd) {
    if (failed != 0 && ctx->strict_spd == 1) {
      set_error("nk_spline_fit: Cholesky met a non-positive pivot and strict mode is on");
      return NK_ERR_NOT_SPD;
    }
    if (ctx->spline_defer_svd) {  // first phase of nk_spline_cv_grid: the unit is run again beside the others of its kind
      set_error("nk_spline_fit: the system takes the pseudo-inverse (deferred to the second phase of the sweep)");
      return NK_ERR_NOT_SPD;
    }
    PinvInfo pi;
    NK_TRY(pinv_right_divide(ctx, Gsave, mp, mp, Gsave + (size_t)mp * mp, mp, m + d, Gtop, mp, rcond, &pi));
    if (!pi.converged) {
      set_error("nk_spline_fit: Jacobi SVD did not converge in %d sweeps", pi.sweeps);
      return NK_ERR_NO_CONVERGENCE;
    }
    rank = pi.rank;
    if (rank < mp) count_event(CNT_RANK_TRUNCATED);
  }
  // ---- operators: A | B = M_ls[:m, :], C = M_ls[m:, :m], W = C [A B] (regressors.py:215-219)
  NK_HIP(hipEventRecord(ctx->ev[EV_SOLVE_BEGIN], ctx->stream));
  NK_TRY(launch_copy2d(ctx, Gtop, mp, mdl->A, mp, m, mp));
  NK_TRY(launch_copy2d(ctx, Gbot, mp, mdl->C, m, d, m));
  NK_TRY(launch_gemm(ctx, false, false, d, mp, m, 1.0, mdl->C, m, mdl->A, mp, 0.0, mdl->W, mp));
  NK_HIP(hipEventRecord(ctx->ev[EV_FIT_END], ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  mdl->has_ops = true;
  if (stats) {
    fill_gram_stats(ctx, stats, x.staged || y.staged, gram_deferred, ms_gram_kernel, gram_launches);
    stats->ms_total = ev_ms(ctx, EV_FIT_BEGIN, EV_FIT_END);
    stats->ms_solve = ev_ms(ctx, EV_GRAM_DONE, EV_FIT_END);
    const double ne = (double)n_eff;
    stats->gram_flops = 2.0 * ne * (double)mp * (double)(mp + m + d);
    stats->kmat_pairs = 2.0 * ne * m * d;
    stats->rank_inner = rank;
    stats->rank_inner_rec = 0;
    stats->pivot_ratio_inner = failed == 0 ? piv_ratio : 0.0;
  }
  if (ctx->arena.chunks.size() > 1 || ctx->arena_side.chunks.size() > 1) NK_TRY(arena_reset(ctx));
  guard.m = nullptr;
  *model = mdl;
  return NK_OK;
}

}  // extern "C"
