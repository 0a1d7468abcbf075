// The one-call sweeps behind the C ABI: nk_cv_grid, nk_spline_cv_grid, nk_sysid_grid (lock-step groups, nk_lockstep.h).
#include "nk_common.h"
#include "nk_api_internal.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <cstdlib>
#include <algorithm>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

using namespace nk;

// ---- the one-call sweeps (nk_cv_grid, nk_spline_cv_grid): data set staged once, one host thread per member, rounds of
// n_members units behind a barrier, two phases.  The estimator enters through two callbacks only.
struct CvData {  // what a unit sees: the data set in HBM, a host copy of Y (only if asked for), the sizes
  const double *Xd = nullptr, *Yd = nullptr, *Yh = nullptr;
  int64_t ldxd = 0, ldyd = 0, ldyh = 0, n = 0;
  int32_t d = 0, p = 0;
};
// fit_score(member, unit, data, scratch, &score): fit + score of one unit on a member that is inside its unit of work.
// Phases: 1 = stop at a system that needs the rank-truncating branch (NK_ERR_NOT_SPD: the unit is run again in phase 2),
// 2 = take the branch, 0 = back to what the caller had set.  strict_phases: the members' strict mode follows the phases
// (1 = strict: the factorisation reports a rank-deficient system and the unit stops there, 2 = the fallback);
// set_phase(member, phase), may be empty: what else the estimator switches.
// A unit may produce several numbers (the trajectories of a system-identification unit): fit_score writes up to `max_vals`
// of them and store(unit, rc, vals) files them -- or NaN when rc != NK_OK -- with the unit's status.
using CvFitScore = std::function<int(nk_ctx*, int, const CvData&, std::vector<double>&, double*)>;
using CvSetPhase = std::function<void(nk_ctx*, int)>;
using CvStore = std::function<void(int, int, const double*)>;
static int cv_grid_run(const char* what, nk_ctx* const* members, int32_t n_members, const double* X, int64_t ldx,
                       const double* Y, int64_t ldy, int64_t n, int32_t d, int32_t p, int32_t n_units, bool want_host_y,
                       const CvFitScore& fit_score, bool strict_phases, const CvSetPhase& set_phase, const CvStore& store,
                       int max_vals) {
  if (n_units == 0) return NK_OK;
  nk_ctx* lead = members[0];
  NK_HIP(hipSetDevice(lead->device));
  // the data set lives in HBM once for all units
  const double *Xd = X, *Yd = Y;
  int64_t ldxd = ldx, ldyd = ldy;
  double *Xown = nullptr, *Yown = nullptr;
  struct Free { double*& a; double*& b; ~Free() { if (a) (void)hipFree(a); if (b) (void)hipFree(b); } } freer{Xown, Yown};
  if (!is_device_ptr(X)) {
    ldxd = d + p + ((d + p) & 1);
    NK_HIP(hipMalloc(reinterpret_cast<void**>(&Xown), (size_t)n * ldxd * 8));
    NK_HIP(hipMemcpy2D(Xown, (size_t)ldxd * 8, X, (size_t)ldx * 8, (size_t)(d + p) * 8, (size_t)n, hipMemcpyHostToDevice));
    Xd = Xown;
  }
  if (!is_device_ptr(Y)) {
    ldyd = d + (d & 1);
    NK_HIP(hipMalloc(reinterpret_cast<void**>(&Yown), (size_t)n * ldyd * 8));
    NK_HIP(hipMemcpy2D(Yown, (size_t)ldyd * 8, Y, (size_t)ldy * 8, (size_t)d * 8, (size_t)n, hipMemcpyHostToDevice));
    Yd = Yown;
  }
  // landmark rows are gathered on the host from a host copy of Y (one download if Y came as a device pointer)
  std::vector<double> Yhost;
  const double* Yh = Y;
  int64_t ldyh = ldy;
  if (is_device_ptr(Y)) {
    Yh = nullptr;
    if (want_host_y) {
      Yhost.resize((size_t)n * d);
      NK_HIP(hipMemcpy2D(Yhost.data(), (size_t)d * 8, Y, (size_t)ldy * 8, (size_t)d * 8, (size_t)n, hipMemcpyDeviceToHost));
      Yh = Yhost.data();
      ldyh = d;
    }
  }
  CvData data;
  data.Xd = Xd; data.Yd = Yd; data.Yh = Yh; data.ldxd = ldxd; data.ldyd = ldyd; data.ldyh = ldyh; data.n = n; data.d = d;
  data.p = p;
  const int B = n_members;
  // one host thread per member; rounds of B units; everybody is inside its unit before anybody starts (round barrier)
  struct Round {
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    void wait(int parties) {
      std::unique_lock<std::mutex> lk(mu);
      const uint64_t g = gen;
      if (++arrived == parties) { arrived = 0; ++gen; lk.unlock(); cv.notify_all(); return; }
      cv.wait(lk, [&] { return gen != g; });
    }
  };
  // Two phases.  A unit whose regularised system is numerically rank deficient takes gelsd's branch: a Jacobi SVD of ~1e4
  // launches (0.2 s at m = 500) during which the other members of its round have nothing to merge with and wait at the
  // next barrier -- a 405-unit cloth grid with 30 such units spent 2 of its 2.4 s that way.  So the first phase runs every
  // unit in strict mode (the factorisation reports the condition and the unit stops there), and the units that reported
  // it are run again TOGETHER in a second phase with the fallback enabled: their Jacobi sweeps merge into shared launches.
  // Same kernels on the same data in both orders: the scores do not depend on the schedule.
  bool all_lenient = true;
  for (int k = 0; k < B; ++k) all_lenient = all_lenient && members[k]->strict_spd == 0;
  std::mutex deferred_mu;
  std::vector<int> deferred;
  auto run_units = [&](const std::vector<int>& list, bool defer_rank_deficient) {
    Round round;
    const int count = (int)list.size();
    const int n_rounds = (count + B - 1) / B;
    auto worker = [&](int k) {
      nk_ctx* ctx = members[k];
      std::vector<double> Z, vals((size_t)max_vals);
      for (int r = 0; r < n_rounds; ++r) {
        const int slot = r * B + k;
        const bool mine = slot < count;
        if (mine) (void)group_enter(ctx);
        round.wait(B);
        if (mine) {
          const int u = list[(size_t)slot];
          std::fill(vals.begin(), vals.end(), std::nan(""));
          int rc = fit_score(ctx, u, data, Z, vals.data());
          tl_ctx = ctx;
          const int rc_leave = group_leave(ctx);  // flushes what the unit recorded after its last synchronisation
          if (rc == NK_OK) rc = rc_leave;
          if (rc == NK_ERR_NOT_SPD && defer_rank_deficient) {
            std::lock_guard<std::mutex> lk(deferred_mu);
            deferred.push_back(u);
          } else {
            store(u, rc, vals.data());
          }
        }
        round.wait(B);
      }
      tl_ctx = nullptr;
    };
    std::vector<std::thread> threads;
    threads.reserve((size_t)B);
    for (int k = 0; k < B; ++k) threads.emplace_back(worker, k);
    for (auto& t : threads) t.join();
  };
  std::vector<int> all((size_t)n_units);
  for (int u = 0; u < n_units; ++u) all[(size_t)u] = u;
  if (!all_lenient) {  // the caller wants the error (strict contexts): one phase, nothing to defer
    run_units(all, false);
    return NK_OK;
  }
  std::vector<int> saved_strict((size_t)B);
  for (int k = 0; k < B; ++k) saved_strict[(size_t)k] = members[k]->strict_spd;
  auto enter_phase = [&](int phase) {
    for (int k = 0; k < B; ++k) {
      if (strict_phases) members[k]->strict_spd = phase == 1 ? 1 : (phase == 2 ? 0 : saved_strict[(size_t)k]);
      if (set_phase) set_phase(members[k], phase);
    }
  };
  const bool cv_trace = getenv("NYSKOOP_CV_TRACE") != nullptr;
  const auto t_start = std::chrono::steady_clock::now();
  enter_phase(1);
  run_units(all, true);
  enter_phase(0);
  const auto t_mid = std::chrono::steady_clock::now();
  if (!deferred.empty()) {
    std::sort(deferred.begin(), deferred.end());
    enter_phase(2);
    run_units(deferred, false);
    enter_phase(0);
  }
  if (cv_trace)
    fprintf(stderr, "[nyskoop] %s: %d units in %.3f s, %zu rank-deficient units again in %.3f s (%d members)\n", what, n_units,
            std::chrono::duration<double>(t_mid - t_start).count(), deferred.size(),
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t_mid).count(), B);
  return NK_OK;
}

// ---- what the sweeps' entry points share
// a unit's test fold [begin, end) inside the n rows
static int check_test_fold(const char* who, int u, int64_t begin, int64_t end, int64_t n) {
  NK_REQUIRE(0 <= begin && begin < end && end <= n, "%s: unit %d: bad test fold", who, u);
  return NK_OK;
}
// a unit's landmarks: rows of the host copy of Y, gathered densely (m x d)
static void gather_landmarks(const CvData& dt, const int64_t* rows, int m, int d, std::vector<double>& Z) {
  Z.resize((size_t)m * d);
  for (int j = 0; j < m; ++j) memcpy(&Z[(size_t)j * d], dt.Yh + rows[j] * dt.ldyh, (size_t)d * 8);
}
// phase 1 stops a spline unit where nk_spline_fit would enter the pseudo-inverse, the other phases let it go on
static void spline_defer_phase(nk_ctx* ctx, int phase) { ctx->spline_defer_svd = phase == 1; }
// one score per unit, NaN for a unit that failed, with the unit's status
static CvStore scalar_store(double* scores, int32_t* status) {
  return [=](int u, int rc, const double* v) {
    scores[u] = rc == NK_OK ? v[0] : std::nan("");
    if (status) status[u] = rc;
  };
}

extern "C" {

int nk_cv_grid(nk_ctx* const* members, int32_t n_members, const double* X, int64_t ldx, const double* Y, int64_t ldy,
               int64_t n, int32_t d, int32_t p, const nk_cv_unit* units, int32_t n_units, double* scores, int32_t* status) {
  NK_REQUIRE(members && n_members >= 1 && X && Y && units && scores, "nk_cv_grid: null argument");
  NK_REQUIRE(n > 0 && d > 0 && p >= 0 && n_units >= 0 && ldx >= d + p && ldy >= d, "nk_cv_grid: bad sizes");
  for (int k = 0; k < n_members; ++k) NK_REQUIRE(members[k] != nullptr, "nk_cv_grid: null member context");
  for (int u = 0; u < n_units; ++u) {
    const nk_cv_unit& cu = units[u];
    NK_REQUIRE(cu.kernel && cu.landmark_rows && cu.m > 0, "nk_cv_grid: unit %d: null kernel / landmarks", u);
    NK_TRY(check_test_fold("nk_cv_grid", u, cu.test_begin, cu.test_end, n));
    for (int j = 0; j < cu.m; ++j)
      NK_REQUIRE(cu.landmark_rows[j] >= 0 && cu.landmark_rows[j] < n, "nk_cv_grid: unit %d: landmark row out of range", u);
  }
  auto fit_score = [&](nk_ctx* ctx, int u, const CvData& dt, std::vector<double>& Z, double* sc) -> int {
    const nk_cv_unit& cu = units[u];
    gather_landmarks(dt, cu.landmark_rows, cu.m, d, Z);
    const int64_t rr[4] = {0, cu.test_begin, cu.test_end, n};
    nk_model* mdl = nullptr;
    int rc = nk_nystrom_fit(ctx, cu.kernel, dt.Xd, dt.ldxd, dt.Yd, dt.ldyd, n, d, p, rr, 2, nullptr, 0, Z.data(), d, cu.m,
                            cu.gamma, cu.jitter, &mdl, nullptr);
    if (rc == NK_OK)
      rc = nk_score_neg_rmse(ctx, mdl, dt.Xd + cu.test_begin * dt.ldxd, dt.ldxd, dt.Yd + cu.test_begin * dt.ldyd, dt.ldyd,
                             cu.test_end - cu.test_begin, sc);
    if (mdl) nk_model_destroy(mdl);
    return rc;
  };
  return cv_grid_run("cv_grid", members, n_members, X, ldx, Y, ldy, n, d, p, n_units, true, fit_score, true, nullptr,
                     scalar_store(scores, status), 1);
}

// The spline sweep (regressors.py:181-221 under GridSearchCV, benchmark_lqr_classic.py:55-60): same rounds, same two phases.
// Phase 1 stops a unit at the point where nk_spline_fit would enter the pseudo-inverse (pivot ratio inside the SVD window or a
// failed factorisation); phase 2 runs those units together.
int nk_spline_cv_grid(nk_ctx* const* members, int32_t n_members, const double* X, int64_t ldx, const double* Y, int64_t ldy,
                      int64_t n, int32_t d, int32_t p, const nk_spline_cv_unit* units, int32_t n_units, double* scores,
                      int32_t* status) {
  NK_REQUIRE(members && n_members >= 1 && X && Y && units && scores, "nk_spline_cv_grid: null argument");
  NK_REQUIRE(n > 0 && d > 0 && p >= 0 && n_units >= 0 && ldx >= d + p && ldy >= d, "nk_spline_cv_grid: bad sizes");
  for (int k = 0; k < n_members; ++k) NK_REQUIRE(members[k] != nullptr, "nk_spline_cv_grid: null member context");
  for (int u = 0; u < n_units; ++u) {
    const nk_spline_cv_unit& cu = units[u];
    NK_REQUIRE(cu.centers && cu.m > 0, "nk_spline_cv_grid: unit %d: null centres / m <= 0", u);
    NK_REQUIRE(!is_device_ptr(cu.centers), "nk_spline_cv_grid: unit %d: centres must be a host pointer", u);
    NK_TRY(check_test_fold("nk_spline_cv_grid", u, cu.test_begin, cu.test_end, n));
  }
  auto fit_score = [&](nk_ctx* ctx, int u, const CvData& dt, std::vector<double>&, double* sc) -> int {
    const nk_spline_cv_unit& cu = units[u];
    const int64_t rr[4] = {0, cu.test_begin, cu.test_end, n};
    nk_model* mdl = nullptr;
    int rc = nk_spline_fit(ctx, dt.Xd, dt.ldxd, dt.Yd, dt.ldyd, n, d, p, rr, 2, cu.centers, d, cu.m, cu.gamma, &mdl, nullptr);
    if (rc == NK_OK)
      rc = nk_score_neg_rmse(ctx, mdl, dt.Xd + cu.test_begin * dt.ldxd, dt.ldxd, dt.Yd + cu.test_begin * dt.ldyd, dt.ldyd,
                             cu.test_end - cu.test_begin, sc);
    if (mdl) nk_model_destroy(mdl);
    return rc;
  };
  return cv_grid_run("spline_cv_grid", members, n_members, X, ldx, Y, ldy, n, d, p, n_units, false, fit_score, false,
                     spline_defer_phase, scalar_store(scores, status), 1);
}

// The multi-seed system-identification sweep (benchmark_lqr_classic.py:211-255, benchmark_lqr_cloth.py:163-211) as one call:
// unit = one fit (either estimator) on some rows of the shared data set + the open-loop error of its test trajectories,
// reduced on the device.  Same rounds and the same two phases as the hyper-parameter sweeps; the test trajectories and
// their controls live in HBM once, like the data set.
int nk_sysid_grid(nk_ctx* const* members, int32_t n_members, const double* X, int64_t ldx, const double* Y, int64_t ldy,
                  int64_t n, int32_t d, int32_t p, const double* trajs, const double* U, int32_t n_trajs, int32_t T,
                  const nk_sysid_unit* units, int32_t n_units, double* err_abs, double* err_rel, int32_t* status) {
  NK_REQUIRE(members && n_members >= 1 && X && Y && trajs && units, "nk_sysid_grid: null argument");
  NK_REQUIRE(n > 0 && d > 0 && p >= 0 && n_units >= 0 && ldx >= d + p && ldy >= d, "nk_sysid_grid: bad sizes");
  NK_REQUIRE(n_trajs >= 1 && T >= 1 && (p == 0 || T == 1 || U != nullptr), "nk_sysid_grid: bad trajectories / controls missing");
  for (int k = 0; k < n_members; ++k) NK_REQUIRE(members[k] != nullptr, "nk_sysid_grid: null member context");
  std::vector<int64_t> offs((size_t)n_units + 1, 0);
  int max_traj = 1;
  bool any_nystrom = false;
  for (int u = 0; u < n_units; ++u) {
    const nk_sysid_unit& su = units[u];
    NK_REQUIRE(su.m > 0 && su.m <= 4096, "nk_sysid_grid: unit %d: m = %d outside 1..4096", u, su.m);
    if (su.kernel) {
      any_nystrom = true;
      NK_REQUIRE(su.landmark_rows != nullptr, "nk_sysid_grid: unit %d: null landmark rows", u);
      for (int j = 0; j < su.m; ++j)
        NK_REQUIRE(su.landmark_rows[j] >= 0 && su.landmark_rows[j] < n, "nk_sysid_grid: unit %d: landmark row out of range", u);
    } else {
      NK_REQUIRE(su.centers != nullptr, "nk_sysid_grid: unit %d: neither a kernel nor centres", u);
      NK_REQUIRE(!is_device_ptr(su.centers), "nk_sysid_grid: unit %d: centres must be a host pointer", u);
    }
    NK_REQUIRE(su.n_ranges >= 0 && (su.n_ranges == 0 || su.row_ranges != nullptr), "nk_sysid_grid: unit %d: bad row ranges", u);
    for (int i = 0; su.row_ranges && i < su.n_ranges; ++i)
      NK_REQUIRE(0 <= su.row_ranges[2 * i] && su.row_ranges[2 * i] <= su.row_ranges[2 * i + 1] && su.row_ranges[2 * i + 1] <= n,
                 "nk_sysid_grid: unit %d: row range %d outside [0,%lld)", u, i, (long long)n);
    NK_REQUIRE(su.traj != nullptr && su.n_traj >= 1 && su.n_traj <= 65535, "nk_sysid_grid: unit %d: no test trajectories", u);
    for (int i = 0; i < su.n_traj; ++i)
      NK_REQUIRE(su.traj[i] >= 0 && su.traj[i] < n_trajs, "nk_sysid_grid: unit %d: trajectory index out of range", u);
    offs[(size_t)u + 1] = offs[(size_t)u] + su.n_traj;
    max_traj = std::max(max_traj, (int)su.n_traj);
  }
  if (n_units == 0) return NK_OK;
  NK_HIP(hipSetDevice(members[0]->device));
  // the test trajectories and their controls: in HBM once for all units (copied on the caller's thread before any member
  // thread exists: no current context, so the two copies and their wait are issued, not recorded)
  tl_ctx = nullptr;
  const bool have_u = p > 0 && T > 1;
  const int64_t td = (int64_t)T * d, tp = (int64_t)T * p;
  const double *Td = trajs, *Ud = have_u ? U : nullptr;
  double *Town = nullptr, *Uown = nullptr;
  struct Free { double*& a; double*& b; ~Free() { if (a) (void)hipFree(a); if (b) (void)hipFree(b); } } freer{Town, Uown};
  if (!is_device_ptr(trajs)) {
    NK_HIP(hipMalloc(reinterpret_cast<void**>(&Town), (size_t)n_trajs * td * 8));
    NK_HIP(hipMemcpyAsync(Town, trajs, (size_t)n_trajs * td * 8, hipMemcpyHostToDevice, members[0]->stream_main));
    Td = Town;
  }
  if (have_u && !is_device_ptr(U)) {
    NK_HIP(hipMalloc(reinterpret_cast<void**>(&Uown), (size_t)n_trajs * tp * 8));
    NK_HIP(hipMemcpyAsync(Uown, U, (size_t)n_trajs * tp * 8, hipMemcpyHostToDevice, members[0]->stream_main));
    Ud = Uown;
  }
  NK_HIP(hipStreamSynchronize(members[0]->stream_main));
  auto fit_score = [&](nk_ctx* ctx, int u, const CvData& dt, std::vector<double>& Z, double* out) -> int {
    const nk_sysid_unit& su = units[u];
    nk_model* mdl = nullptr;
    int rc;
    if (su.kernel) {
      gather_landmarks(dt, su.landmark_rows, su.m, d, Z);
      rc = nk_nystrom_fit(ctx, su.kernel, dt.Xd, dt.ldxd, dt.Yd, dt.ldyd, n, d, p, su.row_ranges, su.n_ranges, nullptr, 0,
                          Z.data(), d, su.m, su.gamma, su.jitter, &mdl, nullptr);
    } else {
      rc = nk_spline_fit(ctx, dt.Xd, dt.ldxd, dt.Yd, dt.ldyd, n, d, p, su.row_ranges, su.n_ranges, su.centers, d, su.m,
                         su.gamma, &mdl, nullptr);
    }
    if (rc == NK_OK) rc = check_ctx(ctx);
    if (rc == NK_OK) {
      // the unit's trajectories as one batch: in place when their indices are consecutive, gathered into the arena otherwise
      bool consecutive = true;
      for (int i = 1; i < su.n_traj; ++i) consecutive = consecutive && su.traj[i] == su.traj[0] + i;
      const double *tq = Td + (int64_t)su.traj[0] * td, *uq = have_u ? Ud + (int64_t)su.traj[0] * tp : nullptr;
      if (!consecutive) {
        double *tg = nullptr, *ug = nullptr;
        rc = arena_alloc_t(ctx, (size_t)su.n_traj * td, &tg);
        if (rc == NK_OK && have_u) rc = arena_alloc_t(ctx, (size_t)su.n_traj * tp, &ug);
        for (int i = 0; rc == NK_OK && i < su.n_traj; ++i) {
          rc = launch_copy2d(ctx, Td + (int64_t)su.traj[i] * td, td, tg + (int64_t)i * td, td, 1, td);
          if (rc == NK_OK && have_u) rc = launch_copy2d(ctx, Ud + (int64_t)su.traj[i] * tp, tp, ug + (int64_t)i * tp, tp, 1, tp);
        }
        tq = tg; uq = ug;
      }
      if (rc == NK_OK) rc = rollout_err_run(ctx, mdl, tq, uq, T, su.n_traj, out, out + max_traj);
    }
    if (mdl) nk_model_destroy(mdl);
    return rc;
  };
  // phase 1: both estimators stop where they would enter the rank-truncating branch, phase 2: they take it
  auto store = [&](int u, int rc, const double* v) {
    const nk_sysid_unit& su = units[u];
    for (int i = 0; i < su.n_traj; ++i) {
      if (err_abs) err_abs[offs[(size_t)u] + i] = rc == NK_OK ? v[i] : std::nan("");
      if (err_rel) err_rel[offs[(size_t)u] + i] = rc == NK_OK ? v[max_traj + i] : std::nan("");
    }
    if (status) status[u] = rc;
  };
  return cv_grid_run("sysid_grid", members, n_members, X, ldx, Y, ldy, n, d, p, n_units, any_nystrom, fit_score, true,
                     spline_defer_phase, store, 2 * max_traj);
}

}  // extern "C"
