// Landmark selection on the device (nk_select_landmarks): partial pivoted Cholesky of K(Y, Y) over the candidate rows, the
// pivot of every step chosen greedily (largest residual diagonal entry) or at random in proportion to the residual
// diagonal (RPCholesky).  DESIGN.md section 5i.
//
// State in HBM: the candidates' pre-scaled coordinates, coordinate-major (Yt[k][i]: a thread per candidate row reads
// coalesced); the residual diagonal dg[n_c]; the factor F, column-major n_c x m (F[i + l * ldf]); per-workgroup partials
// (sum of dg, largest dg and its lowest position); the pivot's row of F and its coordinates, gathered once per step into
// contiguous buffers; a result block (LmState, positions, residuals, traces).
//
// A step is two launches, queued for all m steps without a host round trip:
//   lm_pick_kernel   (one workgroup)        finishes the pick from the partials, records residual and trace, applies the stop
//                                           rule, gathers the pivot's row of F and its coordinates;
//   lm_column_kernel (a thread per row)     the new column of F, the residual update, the partials of the next pick.
// Once the done flag is set every queued launch returns at once.  A closing pick launch (j == m) records the trace left.
//
// Orders (the result is a function of the inputs alone: no atomics, nothing depends on the launch geometry but LM_ROWS):
//   kernel value      squared distance / dot product over k in four accumulators (k mod 4), combined (a0 + a1) + (a2 + a3);
//   column sum        sum_{l<j} F[i,l] F[piv,l] over l in four accumulators (l mod 4), combined the same way;
//   sum of dg         inside a workgroup of LM_ROWS rows the halving tree of lm_block_partials; over workgroups thread 0
//                     adds the partial sums in index order; inside the chosen workgroup thread 0 adds dg in index order;
//   ties              the larger dg wins, equal values go to the LOWER position (an associative rule: any tree).
#include "nk_common.h"

#include <climits>
#include <cstring>

namespace nk {
namespace {

constexpr int LM_ROWS = 256;    // candidate rows per workgroup = threads per workgroup
constexpr int LM_CHUNK = 1024;  // partial sums the pick kernel stages in LDS per pass

struct LmState {
  long long piv;  // candidate position of the current pivot
  double dpiv;    // its residual dg[piv] when it was picked
  double dg0max;  // largest entry of the initial diagonal
  int done;       // the stop rule fired: every later launch returns at once
  int count;      // m_selected
};

// candidate rows [0, rows) of Y, scaled by winv, to coordinate-major: Yt[k * ldt + r]
__global__ void __launch_bounds__(256) lm_prep_kernel(const double* __restrict__ Y, int64_t ldy, int64_t rows, int d,
                                                      const double* __restrict__ winv, double* __restrict__ Yt, int64_t ldt) {
  __shared__ double tile[32][33];
  const int64_t r0 = (int64_t)blockIdx.x * 32;
  const int k0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int q = ty; q < 32; q += 8) {
    const int64_t r = r0 + q;
    const int k = k0 + tx;
    tile[q][tx] = (r < rows && k < d) ? Y[r * ldy + k] * winv[k] : 0.0;
  }
  __syncthreads();
  for (int q = ty; q < 32; q += 8) {
    const int k = k0 + q;
    const int64_t r = r0 + tx;
    if (k < d && r < rows) Yt[(int64_t)k * ldt + r] = tile[tx][q];
  }
}

__device__ __forceinline__ double lm_sum4(double a0, double a1, double a2, double a3) { return (a0 + a1) + (a2 + a3); }

// a workgroup's sum of v, largest v and the lowest position that holds it (rows past n_c: valid = false)
__device__ __forceinline__ void lm_block_partials(double v, bool valid, long long i, double* __restrict__ psum,
                                                  double* __restrict__ pmax, long long* __restrict__ ppos) {
  __shared__ double s_sum[LM_ROWS];
  __shared__ double s_max[LM_ROWS];
  __shared__ long long s_pos[LM_ROWS];
  const int t = threadIdx.x;
  s_sum[t] = valid ? v : 0.0;
  s_max[t] = valid ? v : -1.0;
  s_pos[t] = valid ? i : LLONG_MAX;
  __syncthreads();
  for (int s = LM_ROWS / 2; s > 0; s >>= 1) {
    if (t < s) {
      s_sum[t] += s_sum[t + s];
      const double a = s_max[t], b = s_max[t + s];
      if (b > a || (b == a && s_pos[t + s] < s_pos[t])) {
        s_max[t] = b;
        s_pos[t] = s_pos[t + s];
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    psum[blockIdx.x] = s_sum[0];
    pmax[blockIdx.x] = s_max[0];
    ppos[blockIdx.x] = s_pos[0];
  }
}

// dg[i] = k(y_i, y_i): 1 for RBF and Matern, |y_i|^2 + sigma0^2 for the linear kernel; and the partials of the first pick
__global__ void __launch_bounds__(LM_ROWS) lm_init_kernel(int ktype, const double* __restrict__ Yt, int64_t ldt, int64_t nc,
                                                          int d, double sigma0sq, double* __restrict__ dg,
                                                          double* __restrict__ psum, double* __restrict__ pmax,
                                                          long long* __restrict__ ppos) {
  const int64_t i = (int64_t)blockIdx.x * LM_ROWS + threadIdx.x;
  const bool valid = i < nc;
  double v = 0.0;
  if (valid) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (ktype == NK_KERNEL_LINEAR) {
      for (int k = 0; k < d; ++k) {
        const double y = Yt[(int64_t)k * ldt + i];
        a[k & 3] = __builtin_fma(y, y, a[k & 3]);
      }
    }
    v = chain_kfun(ktype, lm_sum4(a[0], a[1], a[2], a[3]), sigma0sq);
    dg[i] = v;
  }
  lm_block_partials(v, valid, i, psum, pmax, ppos);
}

// step j: F[:, j], the residual update and the partials of pick j + 1.  Dynamic LDS: j + d doubles.
__global__ void __launch_bounds__(LM_ROWS) lm_column_kernel(int ktype, const double* __restrict__ Yt, int64_t ldt, int64_t nc,
                                                            int d, double sigma0sq, int j, double* __restrict__ F, int64_t ldf,
                                                            double* __restrict__ dg, const LmState* __restrict__ st,
                                                            const double* __restrict__ prow, const double* __restrict__ ypiv,
                                                            double* __restrict__ psum, double* __restrict__ pmax,
                                                            long long* __restrict__ ppos) {
  extern __shared__ double lm_lds[];
  if (st->done) return;
  double* fp = lm_lds;      // F[piv, 0..j)
  double* yp = lm_lds + j;  // y_piv
  const int t = threadIdx.x;
  for (int l = t; l < j; l += LM_ROWS) fp[l] = prow[l];
  for (int k = t; k < d; k += LM_ROWS) yp[k] = ypiv[k];
  __syncthreads();
  const long long piv = st->piv;
  const double dpiv = st->dpiv;
  const int64_t i = (int64_t)blockIdx.x * LM_ROWS + t;
  const bool valid = i < nc;
  double v = 0.0;
  if (valid) {
    const double* yi = Yt + i;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const int d4 = d & ~3;
    if (ktype == NK_KERNEL_LINEAR) {
      for (int k = 0; k < d4; k += 4) {
        a0 = __builtin_fma(yi[(int64_t)k * ldt], yp[k], a0);
        a1 = __builtin_fma(yi[(int64_t)(k + 1) * ldt], yp[k + 1], a1);
        a2 = __builtin_fma(yi[(int64_t)(k + 2) * ldt], yp[k + 2], a2);
        a3 = __builtin_fma(yi[(int64_t)(k + 3) * ldt], yp[k + 3], a3);
      }
      if (d4 < d) a0 = __builtin_fma(yi[(int64_t)d4 * ldt], yp[d4], a0);
      if (d4 + 1 < d) a1 = __builtin_fma(yi[(int64_t)(d4 + 1) * ldt], yp[d4 + 1], a1);
      if (d4 + 2 < d) a2 = __builtin_fma(yi[(int64_t)(d4 + 2) * ldt], yp[d4 + 2], a2);
    } else {
      for (int k = 0; k < d4; k += 4) {
        const double e0 = yi[(int64_t)k * ldt] - yp[k], e1 = yi[(int64_t)(k + 1) * ldt] - yp[k + 1];
        const double e2 = yi[(int64_t)(k + 2) * ldt] - yp[k + 2], e3 = yi[(int64_t)(k + 3) * ldt] - yp[k + 3];
        a0 = __builtin_fma(e0, e0, a0);
        a1 = __builtin_fma(e1, e1, a1);
        a2 = __builtin_fma(e2, e2, a2);
        a3 = __builtin_fma(e3, e3, a3);
      }
      if (d4 < d) { const double e = yi[(int64_t)d4 * ldt] - yp[d4]; a0 = __builtin_fma(e, e, a0); }
      if (d4 + 1 < d) { const double e = yi[(int64_t)(d4 + 1) * ldt] - yp[d4 + 1]; a1 = __builtin_fma(e, e, a1); }
      if (d4 + 2 < d) { const double e = yi[(int64_t)(d4 + 2) * ldt] - yp[d4 + 2]; a2 = __builtin_fma(e, e, a2); }
    }
    const double kv = chain_kfun(ktype, lm_sum4(a0, a1, a2, a3), sigma0sq);
    const double* fi = F + i;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const int j4 = j & ~3;
#pragma unroll 2
    for (int l = 0; l < j4; l += 4) {
      s0 = __builtin_fma(fi[(int64_t)l * ldf], fp[l], s0);
      s1 = __builtin_fma(fi[(int64_t)(l + 1) * ldf], fp[l + 1], s1);
      s2 = __builtin_fma(fi[(int64_t)(l + 2) * ldf], fp[l + 2], s2);
      s3 = __builtin_fma(fi[(int64_t)(l + 3) * ldf], fp[l + 3], s3);
    }
    if (j4 < j) s0 = __builtin_fma(fi[(int64_t)j4 * ldf], fp[j4], s0);
    if (j4 + 1 < j) s1 = __builtin_fma(fi[(int64_t)(j4 + 1) * ldf], fp[j4 + 1], s1);
    if (j4 + 2 < j) s2 = __builtin_fma(fi[(int64_t)(j4 + 2) * ldf], fp[j4 + 2], s2);
    const double c = kv - lm_sum4(s0, s1, s2, s3);
    const double f = c / sqrt(dpiv);
    v = fmax(dg[i] - f * f, 0.0);
    if (i == piv) v = 0.0;
    F[i + (int64_t)j * ldf] = f;
    dg[i] = v;
  }
  lm_block_partials(v, valid, i, psum, pmax, ppos);
}

// pick j from the partials of the launch before; j == m: the closing launch (trace left, count)
__global__ void __launch_bounds__(LM_ROWS) lm_pick_kernel(int rule, int j, int m, int64_t nc, int nwg, const double* __restrict__ u,
                                                          double tol, const double* __restrict__ dg,
                                                          const double* __restrict__ psum, const double* __restrict__ pmax,
                                                          const long long* __restrict__ ppos, const double* __restrict__ F,
                                                          int64_t ldf, const double* __restrict__ Yt, int64_t ldt, int d,
                                                          LmState* __restrict__ st, long long* __restrict__ out_pos,
                                                          double* __restrict__ out_resid, double* __restrict__ out_trace,
                                                          double* __restrict__ prow, double* __restrict__ ypiv) {
  __shared__ double sh[LM_CHUNK];
  __shared__ double s_max[LM_ROWS];
  __shared__ long long s_pos[LM_ROWS];
  __shared__ long long s_piv;
  __shared__ double s_before;
  __shared__ int s_w, s_stop;
  if (st->done) return;
  const int t = threadIdx.x;
  // T = sum of dg: the workgroups' partial sums added in index order by thread 0
  double T = 0.0;
  for (int base = 0; base < nwg; base += LM_CHUNK) {
    const int cnt = min(LM_CHUNK, nwg - base);
    for (int q = t; q < cnt; q += LM_ROWS) sh[q] = psum[base + q];
    __syncthreads();
    if (t == 0)
      for (int q = 0; q < cnt; ++q) T += sh[q];
    __syncthreads();
  }
  if (j == m) {
    if (t == 0) {
      out_trace[m] = T;
      st->count = m;
    }
    return;
  }
  // the largest residual and the lowest position that holds it (greedy pick; first step: dg0max of the stop rule)
  double gmax = 0.0;
  long long gpos = 0;
  if (rule == NK_LANDMARK_GREEDY || j == 0) {
    double bv = -1.0;
    long long bp = LLONG_MAX;
    for (int w = t; w < nwg; w += LM_ROWS) {
      const double v = pmax[w];
      const long long p = ppos[w];
      if (v > bv || (v == bv && p < bp)) { bv = v; bp = p; }
    }
    s_max[t] = bv;
    s_pos[t] = bp;
    __syncthreads();
    for (int s = LM_ROWS / 2; s > 0; s >>= 1) {
      if (t < s) {
        const double a = s_max[t], b = s_max[t + s];
        if (b > a || (b == a && s_pos[t + s] < s_pos[t])) { s_max[t] = b; s_pos[t] = s_pos[t + s]; }
      }
      __syncthreads();
    }
    gmax = s_max[0];
    gpos = s_pos[0];
  }
  long long piv = gpos;
  double dpiv = gmax;
  if (rule == NK_LANDMARK_RPCHOLESKY) {
    // the first workgroup whose inclusive prefix (index order) exceeds u T; when rounding lets none exceed it, the last
    // workgroup with a positive sum
    const double target = u[j] * T;
    double run = 0.0;  // thread 0: prefix before the workgroup under test
    double last_before = 0.0;
    int last_w = -1;
    if (t == 0) s_w = -1;
    __syncthreads();
    for (int base = 0; base < nwg; base += LM_CHUNK) {
      const int cnt = min(LM_CHUNK, nwg - base);
      for (int q = t; q < cnt; q += LM_ROWS) sh[q] = psum[base + q];
      __syncthreads();
      if (t == 0) {
        for (int q = 0; q < cnt; ++q) {
          const double ps = sh[q];
          if (!(ps > 0.0)) continue;
          last_w = base + q;
          last_before = run;
          const double nxt = run + ps;
          if (nxt > target) { s_w = base + q; s_before = run; break; }
          run = nxt;
        }
      }
      __syncthreads();
      if (s_w >= 0) break;
    }
    if (t == 0 && s_w < 0) { s_w = last_w; s_before = last_before; }
    __syncthreads();
    const int w = s_w;
    __syncthreads();
    if (w < 0) {  // no positive residual is left
      piv = 0;
      dpiv = 0.0;
    } else {
      // inside the workgroup: dg in index order on top of the prefix before it; entries with dg == 0 cannot be hit
      const int64_t i = (int64_t)w * LM_ROWS + t;
      sh[t] = i < nc ? dg[i] : 0.0;
      __syncthreads();
      if (t == 0) {
        double r2 = s_before;
        int pick = -1, last = 0;
        for (int q = 0; q < LM_ROWS; ++q) {
          const double g = sh[q];
          if (!(g > 0.0)) continue;
          last = q;
          const double nxt = r2 + g;
          if (nxt > target) { pick = q; break; }
          r2 = nxt;
        }
        if (pick < 0) pick = last;
        s_piv = (long long)w * LM_ROWS + pick;
        s_before = sh[pick];
      }
      __syncthreads();
      piv = s_piv;
      dpiv = s_before;
    }
  }
  if (t == 0) {
    const double dg0max = j == 0 ? gmax : st->dg0max;
    if (j == 0) st->dg0max = gmax;
    out_resid[j] = dpiv;
    out_trace[j] = T;
    const int stop = !(dpiv > 0.0) || !(dpiv > tol * dg0max);
    if (stop) {
      st->done = 1;
      st->count = j;
    } else {
      st->piv = piv;
      st->dpiv = dpiv;
      out_pos[j] = piv;
    }
    s_stop = stop;
  }
  __syncthreads();
  if (s_stop) return;
  // the pivot's row of F and its coordinates, contiguous for the column launch
  for (int l = t; l < j; l += LM_ROWS) prow[l] = F[piv + (int64_t)l * ldf];
  for (int k = t; k < d; k += LM_ROWS) ypiv[k] = Yt[(int64_t)k * ldt + piv];
}

}  // namespace

int select_landmarks_device(nk_ctx* ctx, int ktype, const double* Y, int64_t ldy, const std::vector<int64_t>& rng, int64_t nc,
                            int d, const double* winv, double sigma0, int rule, const double* u_host, int m, double tol,
                            std::vector<int64_t>* positions, std::vector<double>* resid, std::vector<double>* trace,
                            int* m_selected) {
  const int nwg = (int)((nc + LM_ROWS - 1) / LM_ROWS);
  const int64_t ldt = nc, ldf = nc;
  double *Yt = nullptr, *dg = nullptr, *psum = nullptr, *pmax = nullptr, *prow = nullptr, *ypiv = nullptr, *du = nullptr;
  long long* ppos = nullptr;
  char* res = nullptr;
  // result block: LmState | positions (m) | residuals (m) | traces (m + 1)
  const size_t res_bytes = sizeof(LmState) + (size_t)(3 * m + 1) * 8;
  NK_TRY(arena_alloc_t(ctx, (size_t)d * ldt, &Yt));
  NK_TRY(arena_alloc_t(ctx, (size_t)nc, &dg));
  NK_TRY(arena_alloc_t(ctx, (size_t)nwg, &psum));
  NK_TRY(arena_alloc_t(ctx, (size_t)nwg, &pmax));
  NK_TRY(arena_alloc_t(ctx, (size_t)nwg, &ppos));
  NK_TRY(arena_alloc_t(ctx, (size_t)m, &prow));
  NK_TRY(arena_alloc_t(ctx, (size_t)d, &ypiv));
  NK_TRY(arena_alloc_t(ctx, (size_t)m, &du));
  NK_TRY(arena_alloc_t(ctx, res_bytes, &res));
  // the factor: a dedicated allocation, released before the call returns (the context's workspace only grows)
  struct Factor {
    double* p = nullptr;
    ~Factor() { if (p) (void)hipFree(p); }
  } fac;
  {
    const size_t bytes = (size_t)ldf * m * 8;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&fac.p), bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      fac.p = nullptr;
      set_error("nk_select_landmarks: the %lld x %d factor (%zu bytes) does not fit: %s", (long long)nc, m, bytes,
                hipGetErrorString(e));
      return NK_ERR_OOM;
    }
  }
  LmState* st = reinterpret_cast<LmState*>(res);
  long long* d_pos = reinterpret_cast<long long*>(res + sizeof(LmState));
  double* d_resid = reinterpret_cast<double*>(d_pos + m);
  double* d_trace = d_resid + m;
  NK_HIP(hipMemsetAsync(res, 0, res_bytes, ctx->stream));
  if (rule == NK_LANDMARK_RPCHOLESKY) NK_HIP(hipMemcpyAsync(du, u_host, (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream));
  int64_t o = 0;
  for (size_t r = 0; r < rng.size(); r += 2) {
    const int64_t b = rng[r], len = rng[r + 1] - rng[r];
    hipLaunchKernelGGL(lm_prep_kernel, dim3((unsigned)((len + 31) / 32), (unsigned)((d + 31) / 32)), dim3(256), 0, ctx->stream,
                       Y + b * ldy, ldy, len, d, winv, Yt + o, ldt);
    o += len;
  }
  const double s0sq = sigma0 * sigma0;
  hipLaunchKernelGGL(lm_init_kernel, dim3(nwg), dim3(LM_ROWS), 0, ctx->stream, ktype, (const double*)Yt, ldt, nc, d, s0sq, dg,
                     psum, pmax, ppos);
  for (int j = 0; j <= m; ++j) {
    hipLaunchKernelGGL(lm_pick_kernel, dim3(1), dim3(LM_ROWS), 0, ctx->stream, rule, j, m, nc, nwg, (const double*)du, tol,
                       (const double*)dg, (const double*)psum, (const double*)pmax, (const long long*)ppos,
                       (const double*)fac.p, ldf, (const double*)Yt, ldt, d, st, d_pos, d_resid, d_trace, prow, ypiv);
    if (j == m) break;
    hipLaunchKernelGGL(lm_column_kernel, dim3(nwg), dim3(LM_ROWS), (size_t)(j + d) * 8, ctx->stream, ktype, (const double*)Yt,
                       ldt, nc, d, s0sq, j, fac.p, ldf, dg, (const LmState*)st, (const double*)prow, (const double*)ypiv, psum,
                       pmax, ppos);
  }
  NK_HIP(hipGetLastError());
  std::vector<char> h(res_bytes);
  NK_HIP(hipMemcpyAsync(h.data(), res, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  LmState hs;
  memcpy(&hs, h.data(), sizeof(LmState));
  const long long* hp = reinterpret_cast<const long long*>(h.data() + sizeof(LmState));
  const double* hr = reinterpret_cast<const double*>(hp + m);
  *m_selected = hs.count;
  positions->assign(hp, hp + hs.count);
  resid->assign(hr, hr + m);
  trace->assign(hr + m, hr + 2 * m + 1);
  return NK_OK;
}

}  // namespace nk
