// The TN engines' interface: the fp64 engine (nk_gemm_tn.hip) and the fp32 one (nk_gemm_tn_f32.hip) as their callers see
// them, and what the two share: the 128 x 128 tile walk and the deterministic split-K reduce (partial tiles are fp64 in
// both engines).  Tile size, problems per launch and the launch plan are in nk_gemm_plan.h.
#pragma once
#include "nk_common.h"

namespace nk {

constexpr int RPARTS = 8;  // workgroups per tile in the reduce kernel

// ---- fast TN multi-problem GEMM (LDS-DMA staged), see nk_gemm_tn.hip -------------------------------------------
// C_p[M_p x N_p] = alpha_p * A_p^T B_p + beta_p * C_p for up to 4 problems that share the contraction length K:
// A_p stored K x M_p (lda), B_p stored K x N_p (ldb).  One launch covers every 128x128 tile of every problem.
enum { KTRIM_NONE = 0, KTRIM_B_UPPER = 1 /* B (K x N) upper triangular */, KTRIM_A_LOWER = 2 /* A (K x M) lower triangular */ };
struct TnProblem {
  const double* A = nullptr;
  const double* B = nullptr;
  double* C = nullptr;
  int64_t lda = 0, ldb = 0, ldc = 0;
  int M = 0, N = 0;
  int tri = TRI_FULL;  // TRI_UPPER_MIRROR for symmetric products (A == B)
  int ktrim = 0;       // KTRIM_B_UPPER / KTRIM_A_LOWER: a triangular operand, the k range where it is zero is skipped
  double alpha = 1.0, beta = 0.0;
  double* Ct = nullptr;  // optional: also store the transpose, Ct[col][row] = C[row][col] (N x M, leading dim ldct)
  int64_t ldct = 0;
  const double* A_even = nullptr;  // operand selection (TnSkip::select): alternatives of A / B for an even step count
  const double* B_even = nullptr;
  double* Caff = nullptr;  // optional second output Caff = aff_a * C + aff_c * I (same leading dimension as C)
  double aff_a = 0.0, aff_c = 0.0;
};
// Device-side control of a launch, so that an iteration with a data-dependent length can be queued in full without host
// round trips.  state: the launch returns at once when state[0] != 0 && state[0] <= step (state[0] = number of steps after
// which the iteration converged, written on the device).  select: the parity of select[0] picks A/B (odd) or
// A_even/B_even (even) -- the buffer of a ping-pong iteration that holds the final iterate.
struct TnSkip {
  const double* state = nullptr;
  int step = 0;
  const double* select = nullptr;
  // single symmetric product C: the reduce kernel also leaves per-workgroup partial sums of (C - I)^2 here (at least
  // 8 * tiles entries); *resid_count receives how many
  double* resid_partials = nullptr;
  int* resid_count = nullptr;
};
// alignment / leading-dimension requirements of the LDS-DMA path
inline bool tn_fast_ok(const TnProblem& p) { return plan_operands_ok(p.A, p.B, p.lda, p.ldb, p.M, p.N, 2); }
// fp32 engine (nk_gemm_tn_f32.hip): operands fp32 contraction-major, results fp64
struct TnProblemF {
  const float* A = nullptr;
  const float* B = nullptr;
  double* C = nullptr;
  int64_t lda = 0, ldb = 0, ldc = 0;
  int M = 0, N = 0;
  int tri = TRI_FULL;
  double beta = 0.0;
};
inline bool tnf_fast_ok(const TnProblemF& p) { return plan_operands_ok(p.A, p.B, p.lda, p.ldb, p.M, p.N, 4); }
int launch_gemm_tn_f32_multi(nk_ctx* ctx, const TnProblemF* probs, int nprob, int64_t K, int splitk /*0=auto*/,
                             float* ms_kernel = nullptr, bool sync_timing = true);
int prep_rows_f32(nk_ctx* ctx, const double* X, int64_t ldx, int64_t rows, int d, const double* winv, const double* center,
                  float* Xt, int64_t ldt, float* sq);
int launch_cvt_f64_f32(nk_ctx* ctx, const double* src, int64_t lds_, float* dst, int64_t ldd, int64_t rows, int cols);
int launch_kmat_gram_f32(nk_ctx* ctx, int ktype, const float* At, int64_t ldat, const float* sqa, int64_t nA, const float* Bt,
                         int64_t ldbt, const float* sqb, int64_t nB, int d, double sigma0, float* out, int64_t ldo);
int launch_gemm_tn_multi(nk_ctx* ctx, const TnProblem* probs, int nprob, int64_t K, int splitk /*0=auto*/,
                         float* ms_kernel = nullptr, bool sync_timing = true, const TnSkip* skip = nullptr);
int launch_transpose(nk_ctx* ctx, const double* src, int64_t lds, double* dst, int64_t ldd, int rows, int cols);
// Gram-form kernel matrix on the MFMA engine (nk_gemm_tn.hip): prep_rows centres/scales/transposes rows to
// contraction-major and returns their squared norms; launch_kmat_gram evaluates k() in the GEMM epilogue
int launch_colmean(nk_ctx* ctx, const double* Z, int64_t ldz, int rows, int d, double* mean);
int prep_rows(nk_ctx* ctx, const double* X, int64_t ldx, int64_t rows, int d, const double* winv, const double* center,
              double* Xt, int64_t ldt, double* sq);
int launch_kmat_gram(nk_ctx* ctx, int ktype, const double* At, int64_t ldat, const double* sqa, int64_t nA,
                     const double* Bt, int64_t ldbt, const double* sqb, int64_t nB, int d, double sigma0, double* out,
                     int64_t ldo);

// tile (tm, tn) of index t within a problem.  Full problems whose tile grid is a multiple of 8 x 8 are walked in 8 x 8
// super-blocks: workgroups are dispatched in index order, so the ~64 tiles an XCD holds at a time then stream 8 + 8
// operand panels instead of 4 + 16, and more of the panel traffic is shared through that XCD's L2.
__device__ __forceinline__ void tn_tile_coords(int t, int tri, int tiles_n, int M, int& tm, int& tn) {
  if (tri == TRI_FULL) {
    const int tiles_m = (M + TBM - 1) / TBM;
    if ((tiles_m & 7) == 0 && (tiles_n & 7) == 0) {
      const int sb = t >> 6, w = t & 63;
      const int sbn = tiles_n >> 3;
      const int sbr = sb / sbn, sbc = sb - sbr * sbn;
      tm = sbr * 8 + (w >> 3);
      tn = sbc * 8 + (w & 7);
    } else {
      tm = t / tiles_n;
      tn = t - tm * tiles_n;
    }
  } else if ((tiles_n & 7) == 0) {
    // upper triangle in 8 x 8 super-blocks (I <= J, row-major over the super-blocks): 36 tiles in a diagonal super-block
    // (its own upper triangle, row-major), 64 in the others
    const int S = tiles_n >> 3;
    int I = 0, J = 0, rem = t;
    for (;;) {
      const int cnt = (I == J) ? 36 : 64;
      if (rem < cnt) break;
      rem -= cnt;
      if (++J == S) { ++I; J = I; }
    }
    int r, c;
    if (I == J) {
      r = 0;
      while (rem >= 8 - r) {
        rem -= 8 - r;
        ++r;
      }
      c = r + rem;
    } else {
      r = rem >> 3;
      c = rem & 7;
    }
    tm = I * 8 + r;
    tn = J * 8 + c;
  } else {  // upper triangle, row-major enumeration
    int row = 0, rem = t;
    while (rem >= tiles_n - row) {
      rem -= tiles_n - row;
      ++row;
    }
    tm = row;
    tn = row + rem;
  }
}

struct TnRed {
  double* C;
  double* Ct;
  double* Caff;  // see TnDev
  double aff_a, aff_c;
  int64_t ldc, ldct;
  int M, N, tiles_n, tri, tile_begin;
  double alpha, beta;
};
struct TnRedParams {
  TnRed p[TN_MAXP];
  int nprob, splitk;
  const double* slab;
  const double* skip_state;  // see TnParams
  int skip_step;
  // optional (single symmetric problem): every workgroup leaves sum (C - I)^2 over its band in resid_partials[block]
  // (mirrored tiles counted twice), for a convergence check of ||C - I||_F without a separate pass over C
  double* resid_partials;
};

int launch_tn_reduce(nk_ctx* ctx, const TnRedParams& R, int ntiles);  // sums the K slices of a slab in a fixed order
int tn_ensure_zero_page(nk_ctx* ctx);

}  // namespace nk
