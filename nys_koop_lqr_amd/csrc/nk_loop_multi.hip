// The lifted closed loop of lqr_control (benchmark_lqr_cloth.py:79-84) for MANY models in ONE launch, scored on the device:
// the control branch of the cloth sweep (benchmark_lqr_cloth.py:213-270: seeds x {Nystrom, splines}, each with its own
// operators and gain).  One 1024-thread workgroup owns one unit from its first to its last step; blockIdx.x selects the
// unit's record in a table staged with one copy.  Nothing crosses workgroups, so a unit's results depend on that unit alone.
//
// The recursion, in the reference's order of operations: for t < steps
//     u_t = K (phi_ref - phi_t),    x_t = C phi_t,    phi_{t+1} = A phi_t + B u_t.
// A and B live in registers with the tiling of lifted_chain_kernel (nk_rollout.hip): thread (quad = tid / 32, part = tid % 32)
// keeps A[4 quad + r][part + 32 j] (r < 4, j < 4) and, for part < p, B[4 quad + r][part]; phi_t and u_t live in LDS.  A step
// has two halves with one LDS-only barrier each: (a) wave j < p forms u_{t,j} from its row of K (two entries per lane, in
// registers) by a DPP reduction while every wave accumulates its rows of A phi_t; (b) the products with u_t are added, the
// four partial sums per lane are reduced across the 32 parts without LDS (reduce_4rows_32parts) and phi_{t+1} is written.
// The last wave keeps the books beside them: the cumulative inputs (lane j: s_j <- s_j + u_{t,j}, one rounded addition per
// step), sum_j u_{t,j}^2 and the largest |u|.  phi_t goes to the unit's scratch with stores that nothing in the loop waits for.
//
// The states, afterwards and by the same workgroup: C (d x m; 154 KB at d = 192, m = 100) does not fit LDS beside the rest,
// but a slab of 256 rows is 32 entries per thread: thread (rq = tid / 32, part) keeps C[d0 + 8 rq + r][part + 32 j] in
// registers and walks the stored phi_t sixteen steps at a time (staged in LDS).  x_t is stored, (x_t - target)^2 goes through LDS
// and wave w sums step w of the block over the slab's rows in a fixed order.  At the end the per-step terms are summed
// in a fixed order by the last wave.  Every summation order depends on (m, p, d, steps) alone.
// Every loop is bounded by steps, m, p or d; every store is an ordinary vector store.
#include "nk_common.h"

namespace nk {

constexpr int LOOP_THREADS = 1024;
constexpr int LOOP_TB = 16;    // steps per staged block of the projection (= waves per workgroup)
constexpr int LOOP_DT = 256;   // rows of C per slab (8 per 32-lane group)

__global__ void __launch_bounds__(LOOP_THREADS) loop_multi_kernel(const LoopMultiUnit* __restrict__ table, int steps, double c) {
  __shared__ __attribute__((aligned(16))) double zu[2][LOOP_MULTI_MAX_M];   // phi_t, phi_{t+1}: zero beyond m
  __shared__ double us[2][LOOP_MULTI_MAX_P];                                // u_t (parity of the step): zero beyond p
  __shared__ __attribute__((aligned(16))) double phiS[LOOP_TB][LOOP_MULTI_MAX_M];
  __shared__ double sqS[LOOP_TB][LOOP_DT];
  const LoopMultiUnit U = table[blockIdx.x];
  const int m = U.m, p = U.p, d = U.d;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = tid & 31, row0 = (tid >> 5) * 4;
  // after reduce_4rows_32parts lane l holds the total of value 2 * bit4(l) + bit3(l); the lanes with l % 8 == 0 store
  const int rsel = 2 * ((lane >> 4) & 1) + ((lane >> 3) & 1);
  const int myrow = row0 + rsel;
  const bool store_lane = (lane & 7) == 0;
  const bool writer = store_lane && myrow < m;
  const bool wave_active = row0 - (lane >> 5) * 4 < m;  // wave-uniform: the first row of the wave exists
  if (tid < LOOP_MULTI_MAX_M) {
    zu[0][tid] = tid < m ? U.phi0[tid] : 0.0;
    zu[1][tid] = 0.0;
  }
  if (tid < 2 * LOOP_MULTI_MAX_P) (&us[0][0])[tid] = 0.0;
  double g[4][4], gb[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool have = row0 + r < m;
    const double* grow = U.G + (int64_t)(have ? row0 + r : 0) * U.ldg;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = part + 32 * j;
      g[r][j] = (have && k < m) ? grow[k] : 0.0;
    }
    gb[r] = (have && part < p) ? grow[m + part] : 0.0;
  }
  // wave j < p: row j of K and phi_ref, two entries per lane
  double k0 = 0.0, k1 = 0.0, r0 = 0.0, r1 = 0.0;
  if (wave < p) {
    if (lane < m) { k0 = U.K[(int64_t)wave * m + lane]; r0 = U.phi_ref[lane]; }
    if (lane + 64 < m) { k1 = U.K[(int64_t)wave * m + lane + 64]; r1 = U.phi_ref[lane + 64]; }
  }
  // the last wave keeps the books: lane j < p the running input sum s_j, lane 0 the scores of the controls
  const bool books = wave == LOOP_THREADS / 64 - 1;
  double s_cum = 0.0, usum = 0.0, umax = 0.0;
  if (books && lane < p) {
    s_cum = U.u_init[lane];
    if (U.out_ucum) U.out_ucum[lane] = s_cum;
  }
  __syncthreads();
  for (int t = 0; t < steps; ++t) {
    double* cur = zu[t & 1];
    double* nxt = zu[(t + 1) & 1];
    double* ub = us[t & 1];
    // (a) u_t = K (phi_ref - phi_t) beside the rows of A phi_t
    if (wave < p) {  // wave-uniform
      const double pu = fma(k1, r1 - cur[lane + 64], k0 * (r0 - cur[lane]));
      const double u = wave_sum64_dpp(pu);
      if (lane == 0) ub[wave] = u;
    }
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (wave_active) {
      double v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = cur[part + 32 * j];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = fma(g[r][j], v[j], a[r]);
    }
    if (tid < m) U.Phi[(int64_t)t * m + tid] = cur[tid];
    // LDS-only barrier: the global stores need not have retired, nothing reads them back before the loop has ended
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    // (b) phi_{t+1} = A phi_t + B u_t
    {
      const double uv = ub[part & (LOOP_MULTI_MAX_P - 1)];  // (gb is zero for part >= p)
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = fma(gb[r], uv, a[r]);
    }
    const double z = reduce_4rows_32parts(a[0], a[1], a[2], a[3], lane);
    if (writer) nxt[myrow] = z;
    if (books) {
#pragma clang fp contract(off)
      if (lane < p) {
        const double uj = ub[lane];
        if (U.out_u) U.out_u[(int64_t)t * U.ldu + lane] = uj;
        s_cum = s_cum + uj;
        if (U.out_ucum) U.out_ucum[(int64_t)(t + 1) * U.ldc + lane] = s_cum;
      }
      if (lane == 0) {
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < LOOP_MULTI_MAX_P; ++j) {
          if (j < p) {
            const double uj = ub[j];
            const double sq = uj * uj;
            q = j == 0 ? sq : q + sq;
            const double au = fabs(uj);
            umax = (au > umax || au != au) ? au : umax;  // a NaN enters once and stays: no later comparison is true
          }
        }
        usum = usum + q;
        U.usq[t] = q;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  const bool want_states = U.out_x != nullptr || U.out_err != nullptr || U.score != nullptr;  // uniform over the workgroup
  if (!want_states) return;
  __syncthreads();  // the stores of phi_t and of the per-step sums have retired: this workgroup reads them back
  const bool scored = U.target != nullptr;
  const int rq = tid >> 5;
  for (int d0 = 0; d0 < d; d0 += LOOP_DT) {
    double cc[8][4];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int row = d0 + rq * 8 + r;
      const double* crow = U.C + (int64_t)(row < d ? row : 0) * m;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = part + 32 * j;
        cc[r][j] = (row < d && k < m) ? crow[k] : 0.0;
      }
    }
    // the two rows this lane ends up with (one per reduction), and their targets
    const int loc0 = rq * 8 + rsel, loc1 = loc0 + 4;
    const int xr0 = d0 + loc0, xr1 = d0 + loc1;
    const double tg0 = (scored && store_lane && xr0 < d) ? U.target[xr0] : 0.0;
    const double tg1 = (scored && store_lane && xr1 < d) ? U.target[xr1] : 0.0;
    for (int t0 = 0; t0 < steps; t0 += LOOP_TB) {
      const int nb = min(LOOP_TB, steps - t0);
      for (int e = tid; e < nb * LOOP_MULTI_MAX_M; e += LOOP_THREADS) {
        const int ts = e >> 7, k = e & (LOOP_MULTI_MAX_M - 1);
        phiS[ts][k] = k < m ? U.Phi[(int64_t)(t0 + ts) * m + k] : 0.0;
      }
      __syncthreads();
      for (int ts = 0; ts < nb; ++ts) {
        double v[4], a[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = phiS[ts][part + 32 * j];
#pragma unroll
        for (int r = 0; r < 8; ++r) a[r] = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 8; ++r) a[r] = fma(cc[r][j], v[j], a[r]);
        const double x0 = reduce_4rows_32parts(a[0], a[1], a[2], a[3], lane);
        const double x1 = reduce_4rows_32parts(a[4], a[5], a[6], a[7], lane);
        if (store_lane) {
#pragma clang fp contract(off)
          double q0 = 0.0, q1 = 0.0;
          if (xr0 < d) {
            if (U.out_x) U.out_x[(int64_t)(t0 + ts) * U.ldx + xr0] = x0;
            const double df = x0 - tg0;
            q0 = df * df;
          }
          if (xr1 < d) {
            if (U.out_x) U.out_x[(int64_t)(t0 + ts) * U.ldx + xr1] = x1;
            const double df = x1 - tg1;
            q1 = df * df;
          }
          sqS[ts][loc0] = q0;
          sqS[ts][loc1] = q1;
        }
      }
      __syncthreads();
      if (wave < nb) {  // wave w: step t0 + w, the slab's rows in a fixed order
#pragma clang fp contract(off)
        double s = sqS[wave][lane];
#pragma unroll
        for (int q = 1; q < LOOP_DT / 64; ++q) s = s + sqS[wave][lane + 64 * q];
        s = wave_sum64_dpp(s);
        if (lane == 0) U.sse[t0 + wave] = d0 == 0 ? s : U.sse[t0 + wave] + s;
      }
      // (the next block's staging writes phiS only, and every wave has left sqS before it reaches the barrier behind it)
    }
  }
  __syncthreads();  // the per-step sums of squares are complete
  if (!scored) return;
  const double dd = (double)d;
  if (U.out_err)
    for (int t = tid; t < steps; t += LOOP_THREADS) U.out_err[t] = sqrt(U.sse[t] / dd);
  if (books && U.score) {
#pragma clang fp contract(off)
    double J = 0.0;
    for (int t = lane; t < steps; t += 64) {  // lane l: steps l, l + 64, ... in order; then the lanes by the DPP tree
      const double cx = c * U.sse[t];
      J = J + (cx + U.usq[t]);
    }
    J = wave_sum64_dpp(J);
    if (lane == 0) {
      U.score[0] = J;
      U.score[1] = sqrt(U.sse[steps - 1] / dd);
      U.score[2] = usum;
      U.score[3] = umax;
    }
  }
}

int launch_closed_loop_multi(nk_ctx* ctx, const LoopMultiUnit* units, int n_units, int steps, double c) {
  NK_REQUIRE(n_units >= 1 && steps >= 1, "closed_loop_multi: bad sizes");
  for (int u = 0; u < n_units; ++u)
    NK_REQUIRE(units[u].m >= 1 && units[u].m <= LOOP_MULTI_MAX_M && units[u].p >= 1 && units[u].p <= LOOP_MULTI_MAX_P &&
                   units[u].d >= 1,
               "closed_loop_multi: unit %d: bad sizes", u);
  LoopMultiUnit* table = nullptr;
  NK_TRY(arena_alloc_t(ctx, (size_t)n_units, &table));
  NK_HIP(hipMemcpyAsync(table, units, sizeof(LoopMultiUnit) * (size_t)n_units, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(loop_multi_kernel, dim3(n_units), dim3(LOOP_THREADS), 0, ctx->stream,
                     static_cast<const LoopMultiUnit*>(table), steps, c);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

}  // namespace nk
