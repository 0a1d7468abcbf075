// Compute entry points of the C ABI that need nothing of the runtime's registry (nk_api.hip): kernel matrix, landmark
// selection, lift / predict / score and the small linear-algebra calls.
#include "nk_common.h"
#include "nk_chol.h"
#include "nk_tn.h"
#include "nk_api_internal.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>

namespace nk {

int lift_device(nk_ctx* ctx, const nk_model* mdl, const double* Xq, int64_t ldx, int64_t nq, double* out,
                       int64_t ldo) {
  const int m = mdl->m;
  if (mdl->kind == NK_MODEL_SPLINE)  // regressors.py:225-233
    return launch_kmat(ctx, mdl->ktype, Xq, ldx, nq, mdl->Z, mdl->d, m, mdl->d, mdl->winv, mdl->sigma0, out, ldo);
  const int64_t chunk = 32768;
  const ArenaMark mk = arena_mark(ctx);
  double* Kq = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)(nq < chunk ? nq : chunk) * m, &Kq));
  for (int64_t r0 = 0; r0 < nq; r0 += chunk) {
    const int64_t len = nq - r0 < chunk ? nq - r0 : chunk;
    NK_TRY(launch_kmat(ctx, mdl->ktype, Xq + r0 * ldx, ldx, len, mdl->Z, mdl->d, m, mdl->d, mdl->winv, mdl->sigma0, Kq,
                       m));
    NK_TRY(launch_gemm(ctx, false, false, len, m, m, 1.0, Kq, m, mdl->Sinv, m, 0.0, out + r0 * ldo, ldo));
  }
  arena_release(ctx, mk);
  return NK_OK;
}

int predict_device(nk_ctx* ctx, const nk_model* mdl, const double* Xaug, int64_t ldx, int64_t nq, double* out,
                          int64_t ldo) {
  const int m = mdl->m, d = mdl->d, p = mdl->p;
  const int64_t chunk = 32768;
  const ArenaMark mk = arena_mark(ctx);
  double* phi = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)(nq < chunk ? nq : chunk) * m, &phi));
  for (int64_t r0 = 0; r0 < nq; r0 += chunk) {
    const int64_t len = nq - r0 < chunk ? nq - r0 : chunk;
    NK_TRY(lift_device(ctx, mdl, Xaug + r0 * ldx, ldx, len, phi, m));
    NK_TRY(launch_gemm(ctx, false, true, len, d, m, 1.0, phi, m, mdl->W, m + p, 0.0, out + r0 * ldo, ldo));
    if (p > 0)
      NK_TRY(launch_gemm(ctx, false, true, len, d, p, 1.0, Xaug + r0 * ldx + d, ldx, mdl->W + m, m + p, 1.0,
                         out + r0 * ldo, ldo));
  }
  arena_release(ctx, mk);
  return NK_OK;
}

}  // namespace nk

using namespace nk;

extern "C" {

int nk_kernel_matrix(nk_ctx* ctx, const nk_kernel_desc* kd, const double* A, int64_t lda, int64_t nA, const double* B,
                     int64_t ldb, int64_t nB, double* out, int64_t ldo) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(kd && A && B && out, "nk_kernel_matrix: null argument");
  NK_REQUIRE(nA >= 0 && nB >= 0 && kd->d > 0, "nk_kernel_matrix: negative size");
  NK_REQUIRE(lda >= kd->d && ldb >= kd->d && ldo >= nB, "nk_kernel_matrix: leading dimension too small");
  if (nA == 0 || nB == 0) return NK_OK;
  const int d = kd->d;
  double* winv = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)d, &winv));
  NK_TRY(make_winv(ctx, kd, d, winv));
  MatIn a, b;
  NK_TRY(stage_in(ctx, A, lda, nA, d, &a));
  NK_TRY(stage_in(ctx, B, ldb, nB, d, &b));
  MatOut o;
  NK_TRY(stage_out(ctx, out, ldo, nA, nB, &o));
  if (kd->type == NK_KERNEL_TPS && ctx->kmat_mode == 0 && d >= 32 && nA >= 2 && nB >= 2) {
    // the thin-plate spline follows nk_set_kmat_mode, so that the Gram-form blocks of nk_spline_fit can be inspected:
    // rows centred on the mean of B, |a|^2 + |b|^2 - 2 a.b on the MFMA engine
    const int64_t lta = (nA + 1) & ~(int64_t)1, ltb = (nB + 1) & ~(int64_t)1;
    double *center = nullptr, *At = nullptr, *sqa = nullptr, *Bt = nullptr, *sqb = nullptr;
    NK_TRY(arena_alloc_t(ctx, (size_t)d, &center));
    NK_TRY(arena_alloc_t(ctx, (size_t)d * lta, &At));
    NK_TRY(arena_alloc_t(ctx, (size_t)nA, &sqa));
    NK_TRY(arena_alloc_t(ctx, (size_t)d * ltb, &Bt));
    NK_TRY(arena_alloc_t(ctx, (size_t)nB, &sqb));
    NK_TRY(launch_colmean(ctx, b.ptr, b.ld, (int)nB, d, center));
    NK_TRY(prep_rows(ctx, a.ptr, a.ld, nA, d, winv, center, At, lta, sqa));
    NK_TRY(prep_rows(ctx, b.ptr, b.ld, nB, d, winv, center, Bt, ltb, sqb));
    NK_TRY(launch_kmat_gram(ctx, NK_KERNEL_TPS, At, lta, sqa, nA, Bt, ltb, sqb, nB, d, 0.0, o.dev, o.ld));
  } else {
    NK_TRY(launch_kmat(ctx, kd->type, a.ptr, a.ld, nA, b.ptr, b.ld, nB, d, winv, kd->sigma0, o.dev, o.ld));
  }
  NK_TRY(finish_out(ctx, o));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  return NK_OK;
}

int nk_select_landmarks(nk_ctx* ctx, const nk_kernel_desc* kd, const double* Y, int64_t ldy, int64_t n, int32_t d,
                        const int64_t* row_ranges, int32_t n_ranges, int32_t rule, const double* u, int32_t m, double tol,
                        int64_t* out_rows, double* out_resid, double* out_trace, int32_t* m_selected) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(!ctx_recording(ctx), "nk_select_landmarks: not available to the members of a lock-step group");
  NK_REQUIRE(kd && Y && out_rows && m_selected, "nk_select_landmarks: null argument");
  NK_REQUIRE(n >= 1 && d >= 1 && ldy >= d, "nk_select_landmarks: bad sizes (n = %lld, d = %d, ldy = %lld)", (long long)n, d,
             (long long)ldy);
  NK_REQUIRE(d <= LANDMARKS_MAX_D, "nk_select_landmarks: d = %d is beyond the column kernel's range (%d)", d, LANDMARKS_MAX_D);
  NK_REQUIRE(kd->type != NK_KERNEL_TPS,
             "nk_select_landmarks: the thin-plate spline is not positive semi-definite and has no Cholesky factor");
  NK_REQUIRE(kd->type == NK_KERNEL_RBF || kd->type == NK_KERNEL_MATERN52 || kd->type == NK_KERNEL_LINEAR,
             "nk_select_landmarks: unknown kernel type %d", kd->type);
  NK_REQUIRE(rule == NK_LANDMARK_GREEDY || rule == NK_LANDMARK_RPCHOLESKY, "nk_select_landmarks: unknown rule %d", rule);
  NK_REQUIRE(std::isfinite(tol) && tol >= 0.0, "nk_select_landmarks: tol must be finite and non-negative");
  NK_REQUIRE(n_ranges >= 0 && (n_ranges == 0 || row_ranges != nullptr), "nk_select_landmarks: bad row ranges");
  std::vector<int64_t> rng;  // the candidates as [begin, end) pairs, in the order given
  int64_t nc = 0;
  if (n_ranges > 0) {
    for (int i = 0; i < n_ranges; ++i) {
      const int64_t b = row_ranges[2 * i], e = row_ranges[2 * i + 1];
      NK_REQUIRE(0 <= b && b <= e && e <= n, "nk_select_landmarks: row range %d = [%lld,%lld) outside [0,%lld)", i, (long long)b,
                 (long long)e, (long long)n);
      if (e > b) { rng.push_back(b); rng.push_back(e); nc += e - b; }
    }
  } else {
    rng.push_back(0); rng.push_back(n); nc = n;
  }
  NK_REQUIRE(m >= 1 && m <= LANDMARKS_MAX_M && m <= nc, "nk_select_landmarks: m = %d must lie in 1 .. min(%lld candidates, %d)",
             m, (long long)nc, LANDMARKS_MAX_M);
  if (rule == NK_LANDMARK_RPCHOLESKY) {
    NK_REQUIRE(u != nullptr, "nk_select_landmarks: the RPCholesky rule needs m uniforms in u");
    for (int j = 0; j < m; ++j) NK_REQUIRE(u[j] >= 0.0 && u[j] < 1.0, "nk_select_landmarks: u[%d] = %g is outside [0, 1)", j, u[j]);
  }
  NK_REQUIRE(!is_device_ptr(out_rows) && !is_device_ptr(out_resid) && !is_device_ptr(out_trace) && !is_device_ptr(u),
             "nk_select_landmarks: u and the outputs must be host memory");
  double* winv = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)d, &winv));
  NK_TRY(make_winv(ctx, kd, d, winv));  // (checks the descriptor's dimension and length scales before its one copy)
  CallStage st(ctx);
  MatIn y;
  st.in(&y, Y, ldy, n, d);
  NK_TRY(st.commit());
  NK_TRY(st.resident(&y, d));  // every workgroup of the preparation reads it: HBM, not the page-locked block
  std::vector<int64_t> pos;
  std::vector<double> resid, trace;
  int count = 0;
  NK_TRY(select_landmarks_device(ctx, kd->type, y.ptr, y.ld, rng, nc, d, winv, kd->sigma0, rule, u, m, tol, &pos, &resid, &trace,
                                 &count));
  // candidate positions -> rows of Y
  for (int j = 0; j < m; ++j) {
    int64_t row = -1;
    if (j < count) {
      int64_t p = pos[j];
      for (size_t r = 0; r < rng.size(); r += 2) {
        const int64_t len = rng[r + 1] - rng[r];
        if (p < len) { row = rng[r] + p; break; }
        p -= len;
      }
    }
    out_rows[j] = row;
  }
  if (out_resid) std::copy(resid.begin(), resid.end(), out_resid);
  if (out_trace) std::copy(trace.begin(), trace.end(), out_trace);
  *m_selected = count;
  return NK_OK;
}

int nk_lift(nk_ctx* ctx, const nk_model* mdl, const double* Xq, int64_t ldx, int64_t nq, double* out, int64_t ldo) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(mdl && Xq && out, "nk_lift: null argument");
  NK_REQUIRE(nq >= 0 && ldx >= mdl->d && ldo >= mdl->m, "nk_lift: bad sizes");
  if (nq == 0) return NK_OK;
  // a few states (one per tick of a controller that closes the loop on a plant, benchmark_lqr_hjb.py:73-97) go through the
  // page-locked block: no hipMemcpy of pageable memory (whose completion wait alone costs 30-100 us, depending on how
  // the runtime decides to wait)
  CallStage st(ctx);
  MatIn x;
  MatOut o;
  st.in(&x, Xq, ldx, nq, mdl->d);
  st.out(&o, out, ldo, nq, mdl->m);
  NK_TRY(st.commit());
  NK_TRY(st.resident(&x, mdl->d));  // every wave of the kernel-matrix kernel reads its state row
  NK_TRY(lift_device(ctx, mdl, x.ptr, x.ld, nq, o.dev, o.ld));
  NK_TRY(st.queue_outputs());
  NK_HIP(hipStreamSynchronize(ctx->stream));
  st.deliver();
  return NK_OK;
}

int nk_predict(nk_ctx* ctx, const nk_model* mdl, const double* Xaug, int64_t ldx, int64_t nq, double* out,
               int64_t ldo) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(mdl && Xaug && out, "nk_predict: null argument");
  NK_REQUIRE(mdl->has_ops, "nk_predict: model holds no fitted operators");
  NK_REQUIRE(nq >= 0 && ldx >= mdl->d + mdl->p && ldo >= mdl->d, "nk_predict: bad sizes");
  if (nq == 0) return NK_OK;
  const int64_t dp = mdl->d + mdl->p;
  CallStage st(ctx);  // see nk_lift
  MatIn x;
  MatOut o;
  st.in(&x, Xaug, ldx, nq, dp);
  st.out(&o, out, ldo, nq, mdl->d);
  NK_TRY(st.commit());
  NK_TRY(st.resident(&x, dp + (dp & 1)));
  NK_TRY(predict_device(ctx, mdl, x.ptr, x.ld, nq, o.dev, o.ld));
  NK_TRY(st.queue_outputs());
  NK_HIP(hipStreamSynchronize(ctx->stream));
  st.deliver();
  return NK_OK;
}

int nk_score_neg_rmse(nk_ctx* ctx, const nk_model* mdl, const double* Xaug, int64_t ldx, const double* Ytrue,
                      int64_t ldy, int64_t nq, double* score) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(mdl && Xaug && Ytrue && score, "nk_score_neg_rmse: null argument");
  NK_REQUIRE(mdl->has_ops, "nk_score_neg_rmse: model holds no fitted operators");
  NK_REQUIRE(nq > 0 && ldx >= mdl->d + mdl->p && ldy >= mdl->d, "nk_score_neg_rmse: bad sizes");
  const int d = mdl->d;
  MatIn x, y;
  NK_TRY(stage_in(ctx, Xaug, ldx, nq, d + mdl->p, &x));
  NK_TRY(stage_in(ctx, Ytrue, ldy, nq, d, &y));
  double *P = nullptr, *colsum = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)nq * d, &P));
  NK_TRY(arena_alloc_t(ctx, (size_t)d, &colsum));
  NK_TRY(predict_device(ctx, mdl, x.ptr, x.ld, nq, P, d));
  NK_TRY(launch_colsum_sqdiff(ctx, P, d, y.ptr, y.ld, nq, d, colsum));
  std::vector<double> h((size_t)d);
  NK_HIP(hipMemcpyAsync(h.data(), colsum, sizeof(double) * d, hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  double s = 0.0;
  for (int j = 0; j < d; ++j) s += std::sqrt(h[j] / (double)nq);
  *score = -s / d;
  return NK_OK;
}

int nk_gemm(nk_ctx* ctx, int transA, int transB, int64_t M, int64_t N, int64_t K, double alpha, const double* A,
            int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(A && B && C && M >= 0 && N >= 0 && K >= 0, "nk_gemm: bad argument");
  if (M == 0 || N == 0) return NK_OK;
  MatIn a, b;
  NK_TRY(stage_in(ctx, A, lda, transA ? K : M, transA ? M : K, &a));
  NK_TRY(stage_in(ctx, B, ldb, transB ? N : K, transB ? K : N, &b));
  MatOut c;
  NK_TRY(stage_out(ctx, C, ldc, M, N, &c));
  if (c.host && beta != 0.0)
    NK_HIP(hipMemcpy2DAsync(c.dev, (size_t)c.ld * 8, C, (size_t)ldc * 8, (size_t)N * 8, (size_t)M, hipMemcpyHostToDevice,
                            ctx->stream));
  NK_TRY(launch_gemm(ctx, transA != 0, transB != 0, M, N, K, alpha, a.ptr, a.ld, b.ptr, b.ld, beta, c.dev, c.ld));
  NK_TRY(finish_out(ctx, c));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  return NK_OK;
}

// An fp32 operand of nk_gemm_f32 (rows x cols): a device pointer in place, a host array packed into a 16-byte aligned arena
// block whose leading dimension is cols rounded up to a multiple of 4 (the engine's contract; stage_in for floats).
static int stage_in_f32(nk_ctx* ctx, const float* p, int64_t ld, int64_t rows, int64_t cols, const float** out, int64_t* ld_out) {
  if (is_device_ptr(p)) {
    *out = p;
    *ld_out = ld;
    return NK_OK;
  }
  const int64_t ldd = (cols + 3) & ~(int64_t)3;
  float* d = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)rows * ldd, &d));
  NK_HIP(hipMemcpy2DAsync(d, (size_t)ldd * 4, p, (size_t)ld * 4, (size_t)cols * 4, (size_t)rows, hipMemcpyHostToDevice,
                          ctx->stream));
  *out = d;
  *ld_out = ldd;
  return NK_OK;
}

static int gemm_f32_staged(nk_ctx* ctx, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B,
                           int64_t ldb, double* Cm, int64_t ldc) {
  TnProblemF pf;
  pf.M = (int)M; pf.N = (int)N;
  NK_TRY(stage_in_f32(ctx, A, lda, K, M, &pf.A, &pf.lda));
  NK_TRY(stage_in_f32(ctx, B, ldb, K, N, &pf.B, &pf.ldb));
  MatOut c;
  NK_TRY(stage_out(ctx, Cm, ldc, M, N, &c));
  pf.C = c.dev; pf.ldc = c.ld;
  NK_TRY(launch_gemm_tn_f32_multi(ctx, &pf, 1, K, 0, nullptr, true));
  NK_TRY(finish_out(ctx, c));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  return NK_OK;
}

int nk_gemm_f32(nk_ctx* ctx, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B, int64_t ldb,
                double* Cm, int64_t ldc) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(A && B && Cm && M >= 4 && N >= 4 && K > 0 && M < (1 << 30) && N < (1 << 30) && lda >= M && ldb >= N && ldc >= N,
             "nk_gemm_f32: bad argument (M, N >= 4, K > 0, lda >= M, ldb >= N, ldc >= N)");
  // the engine's operand contract binds the operands it reads in place; host operands are packed to it.  Checked before
  // anything is allocated or copied.
  const bool a_dev = is_device_ptr(A), b_dev = is_device_ptr(B);
  NK_REQUIRE(!a_dev || (aligned16(A) && lda % 4 == 0 && lda >= ((M + 3) & ~(int64_t)3)),
             "nk_gemm_f32: a device A must be 16-byte aligned with lda a multiple of 4 that covers M rounded up to one");
  NK_REQUIRE(!b_dev || (aligned16(B) && ldb % 4 == 0 && ldb >= ((N + 3) & ~(int64_t)3)),
             "nk_gemm_f32: a device B must be 16-byte aligned with ldb a multiple of 4 that covers N rounded up to one");
  const ArenaMark mk = arena_mark(ctx);
  const int rc = gemm_f32_staged(ctx, M, N, K, A, lda, B, ldb, Cm, ldc);
  arena_release(ctx, mk);
  return rc;
}

int nk_sqrtm_spd(nk_ctx* ctx, const double* P, int64_t ldp, int32_t m, double* S, double* Sinv, int32_t* iters,
                 double* residual) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(P && S && Sinv && m > 0 && ldp >= m, "nk_sqrtm_spd: bad argument");
  MatIn p;
  NK_TRY(stage_in(ctx, P, ldp, m, m, &p));
  double *s = nullptr, *si = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)m * m, &s));
  NK_TRY(arena_alloc_t(ctx, (size_t)m * m, &si));
  int it = 0;
  double r = 0.0;
  NK_TRY(sqrtm_spd(ctx, p.ptr, p.ld, m, s, si, &it, &r));
  if (iters) *iters = it;
  if (residual) *residual = r;
  const hipMemcpyKind k1 = is_device_ptr(S) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const hipMemcpyKind k2 = is_device_ptr(Sinv) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  NK_HIP(hipMemcpyAsync(S, s, sizeof(double) * m * m, k1, ctx->stream));
  NK_HIP(hipMemcpyAsync(Sinv, si, sizeof(double) * m * m, k2, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  return NK_OK;
}

int nk_solve_spd(nk_ctx* ctx, const double* P, int64_t ldp, int32_t m, const double* R, int64_t ldr, int32_t nrhs,
                 double* X, int64_t ldxo) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(P && R && X && m > 0 && nrhs > 0 && ldp >= m && ldr >= nrhs && ldxo >= nrhs, "nk_solve_spd: bad argument");
  MatIn p, r;
  NK_TRY(stage_in(ctx, P, ldp, m, m, &p));
  NK_TRY(stage_in(ctx, R, ldr, m, nrhs, &r));
  double *L = nullptr, *Linv = nullptr, *W = nullptr;
  const int nblk = (m + CHOL_NB - 1) / CHOL_NB;
  const int64_t ldw = nrhs + (nrhs & 1);
  NK_TRY(arena_alloc_t(ctx, (size_t)m * m, &L));
  NK_TRY(arena_alloc_t(ctx, (size_t)nblk * CHOL_WS, &Linv));
  NK_TRY(arena_alloc_t(ctx, (size_t)m * ldw, &W));
  NK_TRY(launch_copy2d(ctx, p.ptr, p.ld, L, m, m, m));
  NK_TRY(launch_copy2d(ctx, r.ptr, r.ld, W, ldw, m, nrhs));
  double* pivlog = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)m, &pivlog));
  CholSys csys;
  csys.P = L; csys.ldp = m; csys.m = m; csys.Linv = Linv; csys.pivlog = pivlog;
  int rc_chol = cholesky_lower_pair(ctx, &csys, 1);
  if (getenv("NYSKOOP_FORCE_PINV")) rc_chol = NK_ERR_NOT_SPD;  // testing hook: always take the SVD path
  if (rc_chol == NK_ERR_NOT_SPD && ctx->strict_spd != 1) {
    // numerically singular: X = P^+ R with gelsd's cut-off, i.e. X^T = R^T P^+ (P symmetric)
    double *Rt = nullptr, *Xt = nullptr;
    NK_TRY(arena_alloc_t(ctx, (size_t)nrhs * m, &Rt));
    NK_TRY(arena_alloc_t(ctx, (size_t)nrhs * m, &Xt));
    NK_TRY(launch_transpose(ctx, r.ptr, r.ld, Rt, m, m, nrhs));
    PinvInfo pi;
    const double rcond_use = getenv("NYSKOOP_PINV_RCOND") ? atof(getenv("NYSKOOP_PINV_RCOND")) : 2.220446049250313e-16;
    NK_TRY(pinv_right_divide(ctx, p.ptr, p.ld, m, Rt, m, nrhs, Xt, m, rcond_use, &pi));
    if (getenv("NYSKOOP_PINV_TRACE"))
      fprintf(stderr, "[nk pinv] rank %d of %d, sigma_max %.3e, smallest kept %.3e, smallest %.3e, %d sweeps\n", pi.rank, m,
              pi.sigma_max, pi.sigma_min_kept, pi.sigma_min, pi.sweeps);
    if (!pi.converged) {
      set_error("nk_solve_spd: Jacobi SVD of the singular system did not converge in %d sweeps", pi.sweeps);
      return NK_ERR_NO_CONVERGENCE;
    }
    NK_TRY(launch_transpose(ctx, Xt, m, W, ldw, nrhs, m));
  } else {
    NK_TRY(rc_chol);
    NK_TRY(cholesky_solve(ctx, L, m, m, Linv, W, ldw, nrhs));
  }
  NK_HIP(hipMemcpy2DAsync(X, (size_t)ldxo * 8, W, (size_t)ldw * 8, (size_t)nrhs * 8, (size_t)m,
                          is_device_ptr(X) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  return NK_OK;
}

__global__ void nk_fill_pattern_kernel(double* p, int64_t n, unsigned seed) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long x = (unsigned long long)i * 6364136223846793005ULL + seed * 1442695040888963407ULL + 1;
    x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ULL; x ^= x >> 32;
    p[i] = (double)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5;  // uniform [-0.5, 0.5), full mantissa
  }
}

int nk_bench_gram(nk_ctx* ctx, int64_t n, int32_t m, int32_t p, int32_t d, int32_t reps, double* ms_avg, double* flop) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(n > 0 && m > 0 && p >= 0 && d > 0 && reps > 0 && ms_avg, "nk_bench_gram: bad argument");
  const int mp = m + p;
  const int64_t off_out = (mp + 1) & ~1;
  const int64_t ldf = (off_out + m + 1) & ~(int64_t)1;
  const int64_t ldd = d + (d & 1);
  double *F = nullptr, *Y = nullptr, *G1 = nullptr, *G2t = nullptr, *G3 = nullptr, *G4t = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)n * ldf + 64, &F));
  NK_TRY(arena_alloc_t(ctx, (size_t)n * ldd, &Y));
  NK_TRY(arena_alloc_t(ctx, (size_t)mp * mp, &G1));
  NK_TRY(arena_alloc_t(ctx, (size_t)mp * m, &G2t));
  NK_TRY(arena_alloc_t(ctx, (size_t)m * m, &G3));
  NK_TRY(arena_alloc_t(ctx, (size_t)m * ldd, &G4t));
  hipLaunchKernelGGL(nk_fill_pattern_kernel, dim3(4096), dim3(256), 0, ctx->stream, F, n * ldf, 1u);
  hipLaunchKernelGGL(nk_fill_pattern_kernel, dim3(4096), dim3(256), 0, ctx->stream, Y, n * ldd, 2u);
  NK_HIP(hipGetLastError());
  TnProblem pr[4];
  pr[0].A = F; pr[0].B = F; pr[0].lda = pr[0].ldb = ldf; pr[0].M = pr[0].N = mp; pr[0].C = G1; pr[0].ldc = mp;
  pr[0].tri = TRI_UPPER_MIRROR;
  pr[1].A = F; pr[1].B = F + off_out; pr[1].lda = pr[1].ldb = ldf; pr[1].M = mp; pr[1].N = m; pr[1].C = G2t; pr[1].ldc = m;
  pr[2].A = F + off_out; pr[2].B = F + off_out; pr[2].lda = pr[2].ldb = ldf; pr[2].M = pr[2].N = m; pr[2].C = G3;
  pr[2].ldc = m; pr[2].tri = TRI_UPPER_MIRROR;
  pr[3].A = F + off_out; pr[3].lda = ldf; pr[3].M = m; pr[3].N = d; pr[3].C = G4t; pr[3].ldc = ldd; pr[3].B = Y;
  pr[3].ldb = ldd;
  for (int q = 0; q < 4; ++q) NK_REQUIRE(tn_fast_ok(pr[q]), "nk_bench_gram: shape violates the alignment contract");
  double total = 0.0;
  for (int r = 0; r < reps + 1; ++r) {
    float ms = 0.f;
    NK_TRY(launch_gemm_tn_multi(ctx, pr, 4, n, 0, &ms));
    if (r > 0) total += ms;
  }
  NK_HIP(hipStreamSynchronize(ctx->stream));
  *ms_avg = total / reps;
  if (flop) *flop = ((double)mp * (mp + 1) + 2.0 * m * mp + (double)m * (m + 1) + 2.0 * d * m) * (double)n;
  return NK_OK;
}

int nk_chol_aug(nk_ctx* ctx, int32_t nsys, const double* const* P, const int64_t* ldp, const int32_t* m, const double* const* R,
                const int32_t* extra, double* const* L, double* const* X, int32_t* failed, double* piv_ratio) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(nsys >= 1 && nsys <= 2 && P && ldp && m && R && extra && L && X && failed && piv_ratio, "nk_chol_aug: bad argument");
  for (int q = 0; q < nsys; ++q)
    NK_REQUIRE(P[q] && R[q] && L[q] && X[q] && m[q] > 0 && extra[q] > 0 && ldp[q] >= m[q] && !is_device_ptr(P[q]) &&
                   !is_device_ptr(R[q]) && !is_device_ptr(L[q]) && !is_device_ptr(X[q]),
               "nk_chol_aug: system %d: host arrays with m > 0, extra > 0, ld >= m", q);
  // each system as the fits lay it out: the extra rows directly below the matrix, one leading dimension (the caller's)
  CholSys sys[2];
  for (int q = 0; q < nsys; ++q) {
    const int mq = m[q], eq = extra[q];
    const int64_t ld = ldp[q];
    const int nblk = (mq + CHOL_NB - 1) / CHOL_NB;
    double *W = nullptr, *Linv = nullptr, *pivlog = nullptr;
    NK_TRY(arena_alloc_t(ctx, (size_t)(mq + eq) * ld, &W));
    NK_TRY(arena_alloc_t(ctx, (size_t)nblk * CHOL_WS, &Linv));
    NK_TRY(arena_alloc_t(ctx, (size_t)mq + 4, &pivlog));
    if (ld > mq) NK_HIP(hipMemsetAsync(W, 0, (size_t)(mq + eq) * ld * sizeof(double), ctx->stream));
    NK_HIP(hipMemcpy2DAsync(W, (size_t)ld * 8, P[q], (size_t)ld * 8, (size_t)mq * 8, (size_t)mq, hipMemcpyHostToDevice,
                            ctx->stream));
    NK_HIP(hipMemcpy2DAsync(W + (size_t)mq * ld, (size_t)ld * 8, R[q], (size_t)mq * 8, (size_t)mq * 8, (size_t)eq,
                            hipMemcpyHostToDevice, ctx->stream));
    sys[q].P = W; sys[q].ldp = ld; sys[q].m = mq; sys[q].extra = eq; sys[q].Linv = Linv; sys[q].pivlog = pivlog;
  }
  NK_TRY(cholesky_aug_pair_async(ctx, sys, nsys));
  int fl[2] = {0, 0};
  double pr[2] = {0.0, 0.0};
  NK_TRY(cholesky_fail_flags(ctx, sys, nsys, fl, pr));  // synchronises; a CHOL_FLOW_GIVEUP word goes out as it is
  for (int q = 0; q < nsys; ++q) {
    const int mq = m[q], eq = extra[q];
    const int64_t ld = ldp[q];
    failed[q] = fl[q];
    piv_ratio[q] = pr[q];
    NK_HIP(hipMemcpy2DAsync(L[q], (size_t)mq * 8, sys[q].P, (size_t)ld * 8, (size_t)mq * 8, (size_t)mq, hipMemcpyDeviceToHost,
                            ctx->stream));
    NK_HIP(hipMemcpy2DAsync(X[q], (size_t)mq * 8, sys[q].P + (size_t)mq * ld, (size_t)ld * 8, (size_t)mq * 8, (size_t)eq,
                            hipMemcpyDeviceToHost, ctx->stream));
  }
  NK_HIP(hipStreamSynchronize(ctx->stream));
  return NK_OK;
}

}  // extern "C"
