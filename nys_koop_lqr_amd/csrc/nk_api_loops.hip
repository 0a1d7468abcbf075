// Closed loops that run as one launch behind the C ABI: the plant loops (nk_plant_step, nk_plant_loop, nk_plant_loop_multi and
// their forms for a polynomial plant the caller describes, nk_poly_plant_*; nk_plant_loop.hip), the constrained MPC loop
// (nk_mpc_loop, nk_mpc_loop_multi, nk_mpc_qp_host; nk_mpc_loop.hip, nk_mpc.h), its form with limits on predicted states
// (nk_mpc_out_loop, nk_mpc_out_qp_host; nk_mpc_loop.hip, nk_mpc_out.h) and the lifted loop of many models
// (nk_closed_loop_multi; nk_loop_multi.hip).  The unit-table calls
// check every unit, lay its host operands out in one staging block (nk_unit_pack.h), move it with one copy, build the
// table of device records, launch, and bring the results back behind one synchronisation.
#include "nk_common.h"
#include "nk_api_internal.h"
#include "nk_plant.h"
#include "nk_poly_plant.h"
#include "nk_mpc.h"
#include "nk_mpc_out.h"

#include <cmath>
#include <limits>
#include <map>
#include <string>
#include <tuple>
#include <vector>

using namespace nk;

// One model against a plant, for both plant-loop entries.  unit < 0: the single-model call (no "unit %d: " in the text).
static int check_plant_model(nk_ctx* ctx, const char* who, int unit, const nk_model* mdl, int plant) {
  auto at = [unit] { return unit >= 0 ? "unit " + std::to_string(unit) + ": " : std::string(); };  // (a failed check only)
  NK_REQUIRE(mdl->device == ctx->device, "%s: %sthe model lives on device %d, the context on %d", who, at().c_str(),
             mdl->device, ctx->device);
  NK_REQUIRE(mdl->p == 1, "%s: %sthe plants have one input, the model has %d", who, at().c_str(), mdl->p);
  NK_REQUIRE(mdl->d == plant_dim(plant), "%s: %sthe %s has %d states, the model has %d", who, at().c_str(),
             plant_name(plant), plant_dim(plant), mdl->d);
  NK_REQUIRE(mdl->m >= 1 && mdl->m <= plant_loop_max_m(), "%s: %sm = %d landmarks, at most %d fit one workgroup", who,
             at().c_str(), mdl->m, plant_loop_max_m());
  NK_REQUIRE(mdl->kind == NK_MODEL_SPLINE
                 ? mdl->ktype == NK_KERNEL_TPS
                 : (mdl->ktype == NK_KERNEL_RBF || mdl->ktype == NK_KERNEL_MATERN52 || mdl->ktype == NK_KERNEL_LINEAR),
             "%s: %skernel type %d is not supported for this model", who, at().c_str(), mdl->ktype);
  return NK_OK;
}

// The plant description of the polynomial-plant entries: the one validation of nk_poly_plant.h, its message behind `who`.
static int check_poly_plant(const char* who, const nk_poly_plant* plant) {
  char msg[160];
  NK_REQUIRE(poly_plant_check(plant, msg, sizeof msg), "%s: %s", who, msg);
  return NK_OK;
}

// One model against a (validated) polynomial plant, for both polynomial-plant loops; unit as in check_plant_model.
static int check_poly_model(nk_ctx* ctx, const char* who, int unit, const nk_model* mdl, const nk_poly_plant& pl) {
  auto at = [unit] { return unit >= 0 ? "unit " + std::to_string(unit) + ": " : std::string(); };  // (a failed check only)
  NK_REQUIRE(mdl->device == ctx->device, "%s: %sthe model lives on device %d, the context on %d", who, at().c_str(),
             mdl->device, ctx->device);
  NK_REQUIRE(mdl->p == pl.p, "%s: %sthe plant has %d inputs, the model has %d", who, at().c_str(), pl.p, mdl->p);
  NK_REQUIRE(mdl->d == pl.d, "%s: %sthe plant has %d states, the model has %d", who, at().c_str(), pl.d, mdl->d);
  const int max_m = poly_loop_max_m(pl.d, pl.p);
  NK_REQUIRE(mdl->m >= 1 && mdl->m <= max_m, "%s: %sm = %d landmarks, at most %d fit one workgroup with %d states and %d inputs",
             who, at().c_str(), mdl->m, max_m, pl.d, pl.p);
  NK_REQUIRE(mdl->kind == NK_MODEL_SPLINE
                 ? mdl->ktype == NK_KERNEL_TPS
                 : (mdl->ktype == NK_KERNEL_RBF || mdl->ktype == NK_KERNEL_MATERN52 || mdl->ktype == NK_KERNEL_LINEAR),
             "%s: %skernel type %d is not supported for this model", who, at().c_str(), mdl->ktype);
  return NK_OK;
}

// One model and description against a (validated) polynomial plant, for both MPC loops; unit as in check_plant_model.
// *nv_out: the decision variables the loop runs on (the saturated LQR: the p entries of one move).
static int check_mpc_model(nk_ctx* ctx, const char* who, int unit, const nk_model* mdl, const nk_poly_plant& pl,
                           const nk_mpc_desc* desc, int* nv_out) {
  auto at = [unit] { return unit >= 0 ? "unit " + std::to_string(unit) + ": " : std::string(); };  // (a failed check only)
  char msg[200];
  NK_REQUIRE(desc != nullptr, "%s: %sthe description is null", who, at().c_str());
  // the validation reads the arrays of the description on the host: a device pointer is rejected before it is followed
  NK_REQUIRE(!is_device_ptr(desc->H) && !is_device_ptr(desc->F) && !is_device_ptr(desc->K) && !is_device_ptr(desc->lo) &&
                 !is_device_ptr(desc->hi) && !is_device_ptr(desc->dlo) && !is_device_ptr(desc->dhi),
             "%s: %sthe arrays of the description (H, F, K, lo, hi, dlo, dhi) must be host memory", who, at().c_str());
  NK_REQUIRE(mpc_desc_check(desc, msg, sizeof msg), "%s: %s%s", who, at().c_str(), msg);
  NK_REQUIRE(desc->p == pl.p, "%s: %sthe plant has %d inputs, the description has p = %d", who, at().c_str(), pl.p, desc->p);
  NK_REQUIRE(mdl->device == ctx->device, "%s: %sthe model lives on device %d, the context on %d", who, at().c_str(),
             mdl->device, ctx->device);
  NK_REQUIRE(mdl->p == pl.p, "%s: %sthe plant has %d inputs, the model has %d", who, at().c_str(), pl.p, mdl->p);
  NK_REQUIRE(mdl->d == pl.d, "%s: %sthe plant has %d states, the model has %d", who, at().c_str(), pl.d, mdl->d);
  NK_REQUIRE(desc->m == mdl->m, "%s: %sthe description is for m = %d, the model has %d landmarks", who, at().c_str(), desc->m,
             mdl->m);
  const int m = mdl->m, p = mdl->p;
  const int nv = desc->iters == 0 ? p : desc->N * p;  // the saturated LQR runs the loop on the p entries of one move
  NK_REQUIRE(m <= mpc_loop_max_m(nv), "%s: %sm = %d landmarks, at most %d fit one workgroup with nv = %d variables", who,
             at().c_str(), m, mpc_loop_max_m(nv), nv);
  NK_REQUIRE(mdl->kind == NK_MODEL_SPLINE
                 ? mdl->ktype == NK_KERNEL_TPS
                 : (mdl->ktype == NK_KERNEL_RBF || mdl->ktype == NK_KERNEL_MATERN52 || mdl->ktype == NK_KERNEL_LINEAR),
             "%s: %skernel type %d is not supported for this model", who, at().c_str(), mdl->ktype);
  NK_TRY(mpc_loop_check_lds(ctx, m, nv));  // the device's LDS per workgroup against what this (m, nv) needs
  *nv_out = nv;
  return NK_OK;
}

// The constants of one checked description on the host, [M | H^-1 | lo hi dlo dhi] (2 nn + 4 nv doubles, nn = nv^2, or 0
// for the saturated LQR): mpc_prepare and mpc_bound, the same for the single call and for a unit of the multi form.
static int mpc_constants(const char* who, int unit, const nk_mpc_desc& desc, int nv, std::vector<double>* out) {
  const bool cheap = desc.iters == 0;
  const size_t nn = cheap ? 0 : (size_t)nv * nv;
  std::vector<double>& blk = *out;
  blk.assign(2 * nn + 4 * (size_t)nv, 0.0);
  char msg[200];
  if (!cheap && !mpc_prepare(desc, blk.data() + nn, blk.data(), msg, sizeof msg)) {
    if (unit >= 0) set_error("%s: unit %d: %s", who, unit, msg);
    else set_error("%s: %s", who, msg);
    return NK_ERR_BAD_ARG;
  }
  const double inf = std::numeric_limits<double>::infinity();
  double* bnd = blk.data() + 2 * nn;
  for (int i = 0; i < nv; ++i) {
    bnd[i] = mpc_bound(desc.lo, i, -inf);
    bnd[nv + i] = mpc_bound(desc.hi, i, inf);
    bnd[2 * nv + i] = mpc_bound(desc.dlo, i, -inf);
    bnd[3 * nv + i] = mpc_bound(desc.dhi, i, inf);
  }
  return NK_OK;
}

// The output description of one (checked) model and description, for nk_mpc_out_loop and a unit with rows of
// nk_mpc_out_loop_multi; unit as in check_plant_model.  nv: what check_mpc_model gave.
static int check_mpc_out(nk_ctx* ctx, const char* who, int unit, const nk_model* mdl, const nk_mpc_desc* desc,
                         const nk_mpc_out* out, int nv) {
  auto at = [unit] { return unit >= 0 ? "unit " + std::to_string(unit) + ": " : std::string(); };  // (a failed check only)
  NK_REQUIRE(out != nullptr, "%s: %sthe output description is null", who, at().c_str());
  NK_REQUIRE(!is_device_ptr(out), "%s: %sthe output description must be host memory", who, at().c_str());
  NK_REQUIRE(!is_device_ptr(out->G) && !is_device_ptr(out->T) && !is_device_ptr(out->ylo) && !is_device_ptr(out->yhi) &&
                 !is_device_ptr(out->ycomp),
             "%s: %sthe arrays of the output description (G, T, ylo, yhi, ycomp) must be host memory", who, at().c_str());
  char msg[200];
  NK_REQUIRE(mpc_out_check(desc, out, mdl->d, msg, sizeof msg), "%s: %s%s", who, at().c_str(), msg);
  const int m = mdl->m, nt = nv + out->ny;
  NK_REQUIRE(m <= mpc_loop_max_m(nt), "%s: %sm = %d landmarks, at most %d fit one workgroup with nv + ny = %d lanes", who,
             at().c_str(), m, mpc_loop_max_m(nt), nt);
  NK_TRY(mpc_loop_check_lds(ctx, m, nt));
  return NK_OK;
}

// The constants of one checked pair of descriptions on the host, [Kb | S0' | lo hi dlo dhi ycomp] (nt^2 + nv nt + 5 nt
// doubles), and [F; T] (nt x m): mpc_out_prepare and the bounds, the same for the single call and for a unit of the multi
// form.
static int mpc_out_constants(const char* who, int unit, const nk_mpc_desc& desc, const nk_mpc_out& out, int nv,
                             std::vector<double>* consts, std::vector<double>* ft) {
  const int ny = out.ny, nt = nv + ny, m = desc.m;
  const size_t nkb = (size_t)nt * nt, ns0 = (size_t)nv * nt;
  std::vector<double>& blk = *consts;
  blk.assign(nkb + ns0 + 5 * (size_t)nt, 0.0);
  char msg[200];
  if (!mpc_out_prepare(desc, out, blk.data(), blk.data() + nkb, msg, sizeof msg)) {
    if (unit >= 0) set_error("%s: unit %d: %s", who, unit, msg);
    else set_error("%s: %s", who, msg);
    return NK_ERR_BAD_ARG;
  }
  const double inf = std::numeric_limits<double>::infinity();
  double* bnd = blk.data() + nkb + ns0;
  for (int i = 0; i < nt; ++i) {
    const bool in = i < nv;
    bnd[i] = in ? mpc_bound(desc.lo, i, -inf) : mpc_bound(out.ylo, i - nv, -inf);
    bnd[nt + i] = in ? mpc_bound(desc.hi, i, inf) : mpc_bound(out.yhi, i - nv, inf);
    bnd[2 * nt + i] = in ? mpc_bound(desc.dlo, i, -inf) : -inf;
    bnd[3 * nt + i] = in ? mpc_bound(desc.dhi, i, inf) : inf;
    bnd[4 * nt + i] = in ? -1.0 : (double)mpc_out_ycomp(&out, i - nv);
  }
  ft->resize((size_t)nt * m);
  std::copy(desc.F, desc.F + (size_t)nv * m, ft->begin());
  std::copy(out.T, out.T + (size_t)ny * m, ft->begin() + (size_t)nv * m);
  return NK_OK;
}

extern "C" {

int nk_plant_step(int plant, double Ts, const double* x, const double* u, double* x_next) {
  NK_REQUIRE(plant_dim(plant) > 0, "nk_plant_step: unknown plant %d", plant);
  NK_REQUIRE(x && u && x_next, "nk_plant_step: null argument");
  plant_step_host(plant, Ts, x, u[0], x_next);
  return NK_OK;
}

int nk_plant_loop(nk_ctx* ctx, const nk_model* mdl, int plant, double Ts, const double* K, const double* x0,
                  const double* x_ref, int32_t steps, int32_t batch, double* out_x, double* out_u) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(!ctx_recording(ctx), "nk_plant_loop: not available to the members of a lock-step group");
  NK_REQUIRE(mdl && K && x0 && x_ref && out_x && out_u, "nk_plant_loop: null argument");
  NK_REQUIRE(plant_dim(plant) > 0, "nk_plant_loop: unknown plant %d", plant);
  NK_TRY(check_plant_model(ctx, "nk_plant_loop", -1, mdl, plant));
  NK_REQUIRE(steps >= 1 && batch >= 1, "nk_plant_loop: steps = %d and batch = %d must be positive", steps, batch);
  NK_REQUIRE(std::isfinite(Ts), "nk_plant_loop: Ts is not finite");
  const int m = mdl->m, d = mdl->d;
  MatIn k, xi, xr;
  MatOut ox, ou;
  NK_TRY(stage_in(ctx, K, m, 1, m, &k));
  NK_TRY(stage_in(ctx, x0, d, batch, d, &xi));
  NK_TRY(stage_in(ctx, x_ref, d, batch, d, &xr));
  NK_TRY(stage_out(ctx, out_x, d, (int64_t)batch * (steps + 1), d, &ox));
  NK_TRY(stage_out(ctx, out_u, 1, (int64_t)batch * steps, 1, &ou));
  // u = K phi = K (k S^-1)^T = (S^-1 K^T) . k: the product nk_lift forms, contracted with the gain first
  const double* w = k.ptr;
  if (mdl->kind != NK_MODEL_SPLINE) {
    double* wf = nullptr;
    NK_TRY(arena_alloc_t(ctx, (size_t)m + 2, &wf));
    NK_TRY(launch_gemm(ctx, false, true, m, 1, m, 1.0, mdl->Sinv, m, k.ptr, k.ld, 0.0, wf, 1));
    w = wf;
  }
  NK_TRY(launch_plant_loop(ctx, mdl, plant, Ts, w, xi.ptr, xi.ld, xr.ptr, xr.ld, steps, batch, ox.dev, ox.ld, ou.dev,
                           ou.ld));
  NK_TRY(finish_out(ctx, ox));
  NK_TRY(finish_out(ctx, ou));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  return NK_OK;
}

int nk_plant_loop_multi(nk_ctx* ctx, int plant, double Ts, int32_t steps, const nk_plant_unit* units, int32_t n_units,
                        const double* u_opt, int32_t n_uopt, double* out_x, double* out_u, double* scores) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(!ctx_recording(ctx), "nk_plant_loop_multi: not available to the members of a lock-step group");
  NK_REQUIRE(plant_dim(plant) > 0, "nk_plant_loop_multi: unknown plant %d", plant);
  NK_REQUIRE(units != nullptr && n_units >= 1, "nk_plant_loop_multi: n_units = %d units at %p: at least one is needed",
             n_units, (const void*)units);
  NK_REQUIRE(steps >= 1, "nk_plant_loop_multi: steps = %d must be positive", steps);
  NK_REQUIRE(std::isfinite(Ts), "nk_plant_loop_multi: Ts is not finite");
  NK_REQUIRE(out_x || out_u || scores, "nk_plant_loop_multi: out_x, out_u and scores are all null: nothing to return");
  NK_REQUIRE(n_uopt >= 0 && (n_uopt == 0 || u_opt != nullptr), "nk_plant_loop_multi: n_uopt = %d rows of a null u_opt",
             n_uopt);
  NK_REQUIRE(!is_device_ptr(scores), "nk_plant_loop_multi: scores must be host memory");
  const int d = plant_dim(plant);
  // every unit is checked before anything is queued; its gain, initial state and reference are laid out on the way
  UnitPack in, folds;
  std::vector<PlantUnitOffsets> off((size_t)n_units);
  for (int u = 0; u < n_units; ++u) {
    const nk_plant_unit& un = units[u];
    NK_REQUIRE(un.model && un.K && un.x0 && un.x_ref, "nk_plant_loop_multi: unit %d: null argument", u);
    NK_TRY(check_plant_model(ctx, "nk_plant_loop_multi", u, un.model, plant));
    NK_REQUIRE(un.uopt >= -1 && un.uopt < n_uopt, "nk_plant_loop_multi: unit %d: uopt = %d, u_opt has %d rows", u, un.uopt,
               n_uopt);
    NK_REQUIRE(!is_device_ptr(un.K) && !is_device_ptr(un.x0) && !is_device_ptr(un.x_ref),
               "nk_plant_loop_multi: unit %d: K, x0 and x_ref must be host memory", u);
    off[u] = pack_plant_unit(in, folds, un.K, un.x0, un.x_ref, (size_t)un.model->m, (size_t)d,
                             un.model->kind != NK_MODEL_SPLINE);
  }
  double *d_in = nullptr, *d_w = nullptr, *d_sc = nullptr;
  NK_TRY(stage_pack(ctx, in, &d_in));
  if (folds.doubles()) NK_TRY(arena_alloc_t(ctx, folds.doubles(), &d_w));
  if (scores) NK_TRY(arena_alloc_t(ctx, (size_t)n_units * 4, &d_sc));
  MatIn uo;
  MatOut ox, ou;
  if (n_uopt > 0) NK_TRY(stage_in(ctx, u_opt, steps, n_uopt, steps, &uo));
  if (out_x) NK_TRY(stage_out(ctx, out_x, d, (int64_t)n_units * (steps + 1), d, &ox));
  if (out_u) NK_TRY(stage_out(ctx, out_u, 1, (int64_t)n_units * steps, 1, &ou));
  std::vector<PlantLoopUnit> recs((size_t)n_units);
  std::vector<int> ktypes((size_t)n_units);
  for (int u = 0; u < n_units; ++u) {
    const nk_plant_unit& un = units[u];
    const nk_model* mdl = un.model;
    const int m = mdl->m;
    // u = K phi = K (k S^-1)^T = (S^-1 K^T) . k, the fold of nk_plant_loop by the same call on the same operands (the gain
    // row has its leading dimension there); the folds of all units are queued back to back, nothing waits between them
    const double* w = d_in + off[u].K;
    if (mdl->kind != NK_MODEL_SPLINE) {
      double* wf = d_w + off[u].w;
      NK_TRY(launch_gemm(ctx, false, true, m, 1, m, 1.0, mdl->Sinv, m, w, (int64_t)gain_row_reserve((size_t)m), 0.0, wf,
                         1));
      w = wf;
    }
    PlantLoopUnit& r = recs[u];
    r.Z = mdl->Z; r.winv = mdl->winv; r.w = w; r.x0 = d_in + off[u].x0; r.xref = d_in + off[u].x_ref;
    r.out_x = out_x ? ox.dev + (int64_t)u * (steps + 1) * ox.ld : nullptr; r.ldx = out_x ? ox.ld : 0;
    r.out_u = out_u ? ou.dev + (int64_t)u * steps * ou.ld : nullptr; r.ldu = out_u ? ou.ld : 0;
    r.u_opt = un.uopt >= 0 ? uo.ptr + (int64_t)un.uopt * uo.ld : nullptr;
    r.score = scores ? d_sc + 4 * (size_t)u : nullptr;
    r.sigma0sq = mdl->sigma0 * mdl->sigma0; r.m = m; r.reserved = 0;
    ktypes[u] = mdl->ktype;
  }
  NK_TRY(launch_plant_loop_multi(ctx, plant, Ts, steps, recs.data(), ktypes.data(), n_units));
  if (out_x) NK_TRY(finish_out(ctx, ox));
  if (out_u) NK_TRY(finish_out(ctx, ou));
  if (scores) NK_HIP(hipMemcpyAsync(scores, d_sc, (size_t)n_units * 32, hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));  // (the staging block and recs are read by the copies queued above)
  return NK_OK;
}

int nk_poly_plant_step(const nk_poly_plant* plant, const double* x, const double* u, double* x_next) {
  NK_TRY(check_poly_plant("nk_poly_plant_step", plant));
  NK_REQUIRE(x && u && x_next, "nk_poly_plant_step: null argument");
  poly_plant_step_host(*plant, x, u, x_next);
  return NK_OK;
}

int nk_poly_plant_loop(nk_ctx* ctx, const nk_model* mdl, const nk_poly_plant* plant, const double* K, const double* x0,
                       const double* x_ref, int32_t steps, int32_t batch, double* out_x, double* out_u) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(!ctx_recording(ctx), "nk_poly_plant_loop: not available to the members of a lock-step group");
  NK_REQUIRE(mdl && K && x0 && x_ref && out_x && out_u, "nk_poly_plant_loop: null argument");
  NK_TRY(check_poly_plant("nk_poly_plant_loop", plant));
  NK_TRY(check_poly_model(ctx, "nk_poly_plant_loop", -1, mdl, *plant));
  NK_REQUIRE(steps >= 1 && batch >= 1, "nk_poly_plant_loop: steps = %d and batch = %d must be positive", steps, batch);
  const int m = mdl->m, d = mdl->d, p = mdl->p;
  MatIn k, xi, xr;
  MatOut ox, ou;
  NK_TRY(stage_in(ctx, K, m, p, m, &k));
  NK_TRY(stage_in(ctx, x0, d, batch, d, &xi));
  NK_TRY(stage_in(ctx, x_ref, d, batch, d, &xr));
  NK_TRY(stage_out(ctx, out_x, d, (int64_t)batch * (steps + 1), d, &ox));
  NK_TRY(stage_out(ctx, out_u, p, (int64_t)batch * steps, p, &ou));
  // u = K phi = K (k S^-1)^T = (S^-1 K^T)^T k: W = S^-1 K^T (m x p) by ONE product; a spline model lifts with the raw
  // block, W = K^T is the gain read with its strides exchanged
  const double* w = k.ptr;
  int64_t w_ls = 1, w_js = k.ld;
  if (mdl->kind != NK_MODEL_SPLINE) {
    double* wf = nullptr;
    NK_TRY(arena_alloc_t(ctx, (size_t)m * p + 2, &wf));
    NK_TRY(launch_gemm(ctx, false, true, m, p, m, 1.0, mdl->Sinv, m, k.ptr, k.ld, 0.0, wf, p));
    w = wf;
    w_ls = p;
    w_js = 1;
  }
  NK_TRY(launch_poly_loop(ctx, mdl, *plant, w, w_ls, w_js, xi.ptr, xi.ld, xr.ptr, xr.ld, steps, batch, ox.dev, ox.ld, ou.dev,
                          ou.ld));
  NK_TRY(finish_out(ctx, ox));
  NK_TRY(finish_out(ctx, ou));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  return NK_OK;
}

int nk_poly_plant_loop_multi(nk_ctx* ctx, const nk_poly_plant* plant, int32_t steps, const nk_plant_unit* units,
                             int32_t n_units, const double* u_opt, int32_t n_uopt, double* out_x, double* out_u,
                             double* scores) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(!ctx_recording(ctx), "nk_poly_plant_loop_multi: not available to the members of a lock-step group");
  NK_TRY(check_poly_plant("nk_poly_plant_loop_multi", plant));
  NK_REQUIRE(units != nullptr && n_units >= 1, "nk_poly_plant_loop_multi: n_units = %d units at %p: at least one is needed",
             n_units, (const void*)units);
  NK_REQUIRE(steps >= 1, "nk_poly_plant_loop_multi: steps = %d must be positive", steps);
  NK_REQUIRE(out_x || out_u || scores, "nk_poly_plant_loop_multi: out_x, out_u and scores are all null: nothing to return");
  NK_REQUIRE(n_uopt >= 0 && (n_uopt == 0 || u_opt != nullptr), "nk_poly_plant_loop_multi: n_uopt = %d rows of a null u_opt",
             n_uopt);
  NK_REQUIRE(!is_device_ptr(scores), "nk_poly_plant_loop_multi: scores must be host memory");
  const int d = plant->d, p = plant->p;
  // every unit is checked before anything is queued; its gain, initial state and reference are laid out on the way
  UnitPack in, folds;
  std::vector<PolyUnitOffsets> off((size_t)n_units);
  for (int u = 0; u < n_units; ++u) {
    const nk_plant_unit& un = units[u];
    NK_REQUIRE(un.model && un.K && un.x0 && un.x_ref, "nk_poly_plant_loop_multi: unit %d: null argument", u);
    NK_TRY(check_poly_model(ctx, "nk_poly_plant_loop_multi", u, un.model, *plant));
    NK_REQUIRE(un.uopt >= -1 && un.uopt < n_uopt, "nk_poly_plant_loop_multi: unit %d: uopt = %d, u_opt has %d rows", u,
               un.uopt, n_uopt);
    NK_REQUIRE(!is_device_ptr(un.K) && !is_device_ptr(un.x0) && !is_device_ptr(un.x_ref),
               "nk_poly_plant_loop_multi: unit %d: K, x0 and x_ref must be host memory", u);
    off[u] = pack_poly_unit(in, folds, un.K, un.x0, un.x_ref, (size_t)un.model->m, (size_t)d, (size_t)p,
                            un.model->kind != NK_MODEL_SPLINE);
  }
  double *d_in = nullptr, *d_w = nullptr, *d_sc = nullptr;
  NK_TRY(stage_pack(ctx, in, &d_in));
  if (folds.doubles()) NK_TRY(arena_alloc_t(ctx, folds.doubles(), &d_w));
  if (scores) NK_TRY(arena_alloc_t(ctx, (size_t)n_units * 4, &d_sc));
  MatIn uo;
  MatOut ox, ou;
  const int64_t sp = (int64_t)steps * p;
  if (n_uopt > 0) NK_TRY(stage_in(ctx, u_opt, sp, n_uopt, sp, &uo));
  if (out_x) NK_TRY(stage_out(ctx, out_x, d, (int64_t)n_units * (steps + 1), d, &ox));
  if (out_u) NK_TRY(stage_out(ctx, out_u, p, (int64_t)n_units * steps, p, &ou));
  std::vector<PolyLoopUnit> recs((size_t)n_units);
  std::vector<int> ktypes((size_t)n_units);
  for (int u = 0; u < n_units; ++u) {
    const nk_plant_unit& un = units[u];
    const nk_model* mdl = un.model;
    const int m = mdl->m;
    // the fold of nk_poly_plant_loop by the same call on the same operands (the gain rows have their leading dimension
    // there); the folds of all units are queued back to back, nothing waits between them
    const int64_t ldk = (int64_t)gain_row_reserve((size_t)m);
    PolyLoopUnit& r = recs[u];
    r.w = d_in + off[u].K; r.w_ls = 1; r.w_js = ldk;
    if (mdl->kind != NK_MODEL_SPLINE) {
      double* wf = d_w + off[u].w;
      NK_TRY(launch_gemm(ctx, false, true, m, p, m, 1.0, mdl->Sinv, m, d_in + off[u].K, ldk, 0.0, wf, p));
      r.w = wf; r.w_ls = p; r.w_js = 1;
    }
    r.Z = mdl->Z; r.winv = mdl->winv; r.x0 = d_in + off[u].x0; r.xref = d_in + off[u].x_ref;
    r.out_x = out_x ? ox.dev + (int64_t)u * (steps + 1) * ox.ld : nullptr; r.ldx = out_x ? ox.ld : 0;
    r.out_u = out_u ? ou.dev + (int64_t)u * steps * ou.ld : nullptr; r.ldu = out_u ? ou.ld : 0;
    r.u_opt = un.uopt >= 0 ? uo.ptr + (int64_t)un.uopt * uo.ld : nullptr;
    r.score = scores ? d_sc + 4 * (size_t)u : nullptr;
    r.sigma0sq = mdl->sigma0 * mdl->sigma0; r.m = m; r.reserved = 0;
    ktypes[u] = mdl->ktype;
  }
  NK_TRY(launch_poly_loop_multi(ctx, *plant, steps, recs.data(), ktypes.data(), n_units));
  if (out_x) NK_TRY(finish_out(ctx, ox));
  if (out_u) NK_TRY(finish_out(ctx, ou));
  if (scores) NK_HIP(hipMemcpyAsync(scores, d_sc, (size_t)n_units * 32, hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));  // (the staging block and recs are read by the copies queued above)
  return NK_OK;
}

int nk_mpc_loop_max_m(int32_t nv) { return mpc_loop_max_m(nv); }

int nk_mpc_qp_host(const nk_mpc_desc* desc, const double* e, const double* u_prev, double* out_u, double* out_z,
                   double* out_info) {
  char msg[200];
  NK_REQUIRE(mpc_qp_host(desc, e, u_prev, out_u, out_z, out_info, msg, sizeof msg) == 0, "nk_mpc_qp_host: %s", msg);
  return NK_OK;
}

int nk_mpc_loop(nk_ctx* ctx, const nk_model* mdl, const nk_poly_plant* plant, const nk_mpc_desc* desc, const double* x0,
                const double* x_ref, const double* u_init, int32_t steps, int32_t batch, double* out_x, double* out_u,
                double* out_info) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(!ctx_recording(ctx), "nk_mpc_loop: not available to the members of a lock-step group");
  NK_REQUIRE(mdl && x0 && x_ref && out_x && out_u, "nk_mpc_loop: null argument");
  NK_TRY(check_poly_plant("nk_mpc_loop", plant));
  int nv = 0;
  NK_TRY(check_mpc_model(ctx, "nk_mpc_loop", -1, mdl, *plant, desc, &nv));
  const int m = mdl->m, d = mdl->d, p = mdl->p;
  const bool cheap = desc->iters == 0;
  NK_REQUIRE(steps >= 1 && batch >= 1, "nk_mpc_loop: steps = %d and batch = %d must be positive", steps, batch);
  // the constants of the call on the host: [M | H^-1 | lo hi dlo dhi]
  const size_t nn = cheap ? 0 : (size_t)nv * nv;
  std::vector<double> blk;
  NK_TRY(mpc_constants("nk_mpc_loop", -1, *desc, nv, &blk));
  // ---- everything is checked: stage and queue
  const double* G = cheap ? desc->K : desc->F;  // nv x m, host
  MatIn cst, gm, xi, xr, ui;
  MatOut ox, ou, oi;
  NK_TRY(stage_in(ctx, blk.data(), (int64_t)blk.size(), 1, (int64_t)blk.size(), &cst));
  NK_TRY(stage_in(ctx, x0, d, batch, d, &xi));
  NK_TRY(stage_in(ctx, x_ref, d, batch, d, &xr));
  if (u_init) NK_TRY(stage_in(ctx, u_init, p, batch, p, &ui));
  NK_TRY(stage_out(ctx, out_x, d, (int64_t)batch * (steps + 1), d, &ox));
  NK_TRY(stage_out(ctx, out_u, p, (int64_t)batch * steps, p, &ou));
  if (out_info) NK_TRY(stage_out(ctx, out_info, 2, (int64_t)batch * steps, 2, &oi));
  // g = F e = F (k S^-1)^T = (S^-1 F^T)^T k: W = S^-1 F^T (m x nv) by ONE product; a spline model lifts with the raw block,
  // W = F^T
  const double* w = nullptr;
  std::vector<double> Gt;
  if (mdl->kind != NK_MODEL_SPLINE) {
    double* wf = nullptr;
    NK_TRY(stage_in(ctx, G, m, nv, m, &gm));
    NK_TRY(arena_alloc_t(ctx, (size_t)m * nv + 2, &wf));
    NK_TRY(launch_gemm(ctx, false, true, m, nv, m, 1.0, mdl->Sinv, m, gm.ptr, gm.ld, 0.0, wf, nv));
    w = wf;
  } else {
    Gt.resize((size_t)m * nv);
    for (int l = 0; l < m; ++l)
      for (int i = 0; i < nv; ++i) Gt[(size_t)l * nv + i] = G[(size_t)i * m + l];
    NK_TRY(stage_in(ctx, Gt.data(), (int64_t)Gt.size(), 1, (int64_t)Gt.size(), &gm));
    w = gm.ptr;
  }
  NK_TRY(launch_mpc_loop(ctx, mdl, *plant, nv, desc->iters, desc->rho, desc->tol, w, cst.ptr, cst.ptr + nn, cst.ptr + 2 * nn,
                         xi.ptr, xi.ld, xr.ptr, xr.ld, u_init ? ui.ptr : nullptr, u_init ? ui.ld : 0, steps, batch, ox.dev,
                         ox.ld, ou.dev, ou.ld, out_info ? oi.dev : nullptr));
  NK_TRY(finish_out(ctx, ox));
  NK_TRY(finish_out(ctx, ou));
  if (out_info) NK_TRY(finish_out(ctx, oi));
  NK_HIP(hipStreamSynchronize(ctx->stream));  // (blk and Gt are read by the copies queued above)
  return NK_OK;
}

int nk_mpc_out_qp_host(const nk_mpc_desc* desc, const nk_mpc_out* out, const double* e, const double* x_ref,
                       const double* u_prev, double* out_u, double* out_z, double* out_info) {
  char msg[200];
  NK_REQUIRE(mpc_out_qp_host(desc, out, e, x_ref, u_prev, out_u, out_z, out_info, msg, sizeof msg) == 0,
             "nk_mpc_out_qp_host: %s", msg);
  return NK_OK;
}

int nk_mpc_out_loop(nk_ctx* ctx, const nk_model* mdl, const nk_poly_plant* plant, const nk_mpc_desc* desc,
                    const nk_mpc_out* out, const double* x0, const double* x_ref, const double* u_init, int32_t steps,
                    int32_t batch, double* out_x, double* out_u, double* out_info) {
  const char* who = "nk_mpc_out_loop";
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(!ctx_recording(ctx), "%s: not available to the members of a lock-step group", who);
  NK_REQUIRE(mdl && x0 && x_ref && out_x && out_u, "%s: null argument", who);
  NK_TRY(check_poly_plant(who, plant));
  int nv = 0;
  NK_TRY(check_mpc_model(ctx, who, -1, mdl, *plant, desc, &nv));
  NK_TRY(check_mpc_out(ctx, who, -1, mdl, desc, out, nv));
  const int m = mdl->m, d = mdl->d, p = mdl->p;
  const int ny = out->ny, nt = nv + ny;
  NK_REQUIRE(steps >= 1 && batch >= 1, "%s: steps = %d and batch = %d must be positive", who, steps, batch);
  // the constants of the call on the host: [Kb | S0' | lo hi dlo dhi ycomp], and [F; T] (nt x m)
  const size_t nkb = (size_t)nt * nt, ns0 = (size_t)nv * nt;
  std::vector<double> blk, FT;
  NK_TRY(mpc_out_constants(who, -1, *desc, *out, nv, &blk, &FT));
  // ---- everything is checked: stage and queue
  MatIn cst, gm, xi, xr, ui;
  MatOut ox, ou, oi;
  NK_TRY(stage_in(ctx, blk.data(), (int64_t)blk.size(), 1, (int64_t)blk.size(), &cst));
  NK_TRY(stage_in(ctx, x0, d, batch, d, &xi));
  NK_TRY(stage_in(ctx, x_ref, d, batch, d, &xr));
  if (u_init) NK_TRY(stage_in(ctx, u_init, p, batch, p, &ui));
  NK_TRY(stage_out(ctx, out_x, d, (int64_t)batch * (steps + 1), d, &ox));
  NK_TRY(stage_out(ctx, out_u, p, (int64_t)batch * steps, p, &ou));
  if (out_info) NK_TRY(stage_out(ctx, out_info, 2, (int64_t)batch * steps, 2, &oi));
  // W = S^-1 [F; T]' (m x nt) by ONE product, as nk_mpc_loop folds F; a spline model lifts with the raw block, W = [F; T]'
  const double* w = nullptr;
  std::vector<double> Gt;
  if (mdl->kind != NK_MODEL_SPLINE) {
    double* wf = nullptr;
    NK_TRY(stage_in(ctx, FT.data(), m, nt, m, &gm));
    NK_TRY(arena_alloc_t(ctx, (size_t)m * nt + 2, &wf));
    NK_TRY(launch_gemm(ctx, false, true, m, nt, m, 1.0, mdl->Sinv, m, gm.ptr, gm.ld, 0.0, wf, nt));
    w = wf;
  } else {
    Gt.resize((size_t)m * nt);
    for (int l = 0; l < m; ++l)
      for (int i = 0; i < nt; ++i) Gt[(size_t)l * nt + i] = FT[(size_t)i * m + l];
    NK_TRY(stage_in(ctx, Gt.data(), (int64_t)Gt.size(), 1, (int64_t)Gt.size(), &gm));
    w = gm.ptr;
  }
  NK_TRY(launch_mpc_out_loop(ctx, mdl, *plant, nv, ny, desc->iters, desc->rho, desc->tol, mpc_out_theta(desc->rho, out->y_weight),
                             w, cst.ptr, cst.ptr + nkb, cst.ptr + nkb + ns0, xi.ptr, xi.ld, xr.ptr, xr.ld,
                             u_init ? ui.ptr : nullptr, u_init ? ui.ld : 0, steps, batch, ox.dev, ox.ld, ou.dev, ou.ld,
                             out_info ? oi.dev : nullptr));
  NK_TRY(finish_out(ctx, ox));
  NK_TRY(finish_out(ctx, ou));
  if (out_info) NK_TRY(finish_out(ctx, oi));
  NK_HIP(hipStreamSynchronize(ctx->stream));  // (blk, FT and Gt are read by the copies queued above)
  return NK_OK;
}

}  // extern "C"

// The body of nk_mpc_loop_multi (outs = nullptr, n_scores = NK_MPC_N_SCORES) and of nk_mpc_out_loop_multi (n_scores =
// NK_MPC_OUT_N_SCORES): the units without rows are prepared and launched as nk_mpc_loop_multi always did (their score row is
// n_scores wide), the units with rows (outs[u] != nullptr) get the preparation of nk_mpc_out_loop and run in
// launch_mpc_out_loop_multi.  One staging copy and one synchronisation for both kinds.
static int mpc_multi_run(const char* who, nk_ctx* ctx, const nk_poly_plant* plant, int32_t steps, const nk_mpc_unit* units,
                         const nk_mpc_out* const* outs, int32_t n_units, const double* u_opt, int32_t n_uopt, double* out_x,
                         double* out_u, double* out_info, double* scores, int n_scores) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(!ctx_recording(ctx), "%s: not available to the members of a lock-step group", who);
  NK_TRY(check_poly_plant(who, plant));
  NK_REQUIRE(units != nullptr && n_units >= 1, "%s: n_units = %d units at %p: at least one is needed", who, n_units,
             (const void*)units);
  NK_REQUIRE(steps >= 1, "%s: steps = %d must be positive", who, steps);
  NK_REQUIRE(out_x || out_u || out_info || scores, "%s: out_x, out_u, out_info and scores are all null: nothing to return", who);
  NK_REQUIRE(n_uopt >= 0 && (n_uopt == 0 || u_opt != nullptr), "%s: n_uopt = %d rows of a null u_opt", who, n_uopt);
  NK_REQUIRE(!is_device_ptr(scores), "%s: scores must be host memory", who);
  NK_REQUIRE(!is_device_ptr(outs), "%s: outs must be host memory", who);
  const int d = plant->d, p = plant->p;
  // every unit is checked before anything is queued; its constants (mpc_prepare / mpc_out_prepare: the Cholesky inverses of
  // the single calls), its F or K or [F; T], initial state, reference and seed are laid out on the way
  UnitPack in, folds;
  std::vector<MpcUnitOffsets> off((size_t)n_units);
  std::vector<MpcOutUnitOffsets> ooff((size_t)n_units);
  std::vector<std::vector<double>> consts((size_t)n_units), gts((size_t)n_units), fts((size_t)n_units);
  std::vector<int> nvs((size_t)n_units), first((size_t)n_units);
  // (model, description, output description) -> the first unit that holds them
  std::map<std::tuple<const void*, const void*, const void*>, int> prepared;
  int n_rows = 0;
  for (int u = 0; u < n_units; ++u) {
    const nk_mpc_unit& un = units[u];
    const nk_mpc_out* out = outs ? outs[u] : nullptr;
    NK_REQUIRE(un.model && un.desc && un.x0 && un.x_ref, "%s: unit %d: null argument (model, desc, x0, x_ref)", who, u);
    NK_REQUIRE(un.reserved == 0, "%s: unit %d: reserved = %d must be 0", who, u, un.reserved);
    NK_REQUIRE(!is_device_ptr(un.desc), "%s: unit %d: the description must be host memory", who, u);
    NK_TRY(check_mpc_model(ctx, who, u, un.model, *plant, un.desc, &nvs[u]));
    if (out) NK_TRY(check_mpc_out(ctx, who, u, un.model, un.desc, out, nvs[u]));
    NK_REQUIRE(un.uopt >= -1 && un.uopt < n_uopt, "%s: unit %d: uopt = %d, u_opt has %d rows", who, u, un.uopt, n_uopt);
    NK_REQUIRE(!is_device_ptr(un.x0) && !is_device_ptr(un.x_ref) && !is_device_ptr(un.u_init),
               "%s: unit %d: x0, x_ref and u_init must be host memory", who, u);
    n_rows += out != nullptr;
    // units that share model and descriptions share the prepared pieces of the first of them: the same constants, bounds, W
    first[u] = prepared.emplace(std::make_tuple((const void*)un.model, (const void*)un.desc, (const void*)out), u).first->second;
    if (first[u] != u) {
      if (out) {
        ooff[u] = ooff[first[u]];
        pack_mpc_out_unit_state(in, ooff[u], un.x0, un.x_ref, un.u_init, (size_t)d, (size_t)p);
      } else {
        off[u] = off[first[u]];
        pack_mpc_unit_state(in, off[u], un.x0, un.x_ref, un.u_init, (size_t)d, (size_t)p);
      }
      continue;
    }
    if (out) {
      NK_TRY(mpc_out_constants(who, u, *un.desc, *out, nvs[u], &consts[u], &fts[u]));
      const nk_model* mdl = un.model;
      const int m = mdl->m, nt = nvs[u] + out->ny;
      const bool fold = mdl->kind != NK_MODEL_SPLINE;
      const double* FT = fts[u].data();
      if (!fold) {  // a spline model lifts with the raw block: W = [F; T]', formed here as the single call forms it
        gts[u].resize((size_t)m * nt);
        for (int l = 0; l < m; ++l)
          for (int i = 0; i < nt; ++i) gts[u][(size_t)l * nt + i] = FT[(size_t)i * m + l];
        FT = gts[u].data();
      }
      ooff[u] = pack_mpc_out_unit(in, folds, consts[u].data(), FT, un.x0, un.x_ref, un.u_init, (size_t)m, (size_t)nvs[u],
                                  (size_t)out->ny, (size_t)d, (size_t)p, fold);
      continue;
    }
    NK_TRY(mpc_constants(who, u, *un.desc, nvs[u], &consts[u]));
    const nk_model* mdl = un.model;
    const int m = mdl->m, nv = nvs[u];
    const bool cheap = un.desc->iters == 0, fold = mdl->kind != NK_MODEL_SPLINE;
    const double* G = cheap ? un.desc->K : un.desc->F;  // nv x m, host
    if (!fold) {  // a spline model lifts with the raw block: W = G', formed here as the single call forms it
      gts[u].resize((size_t)m * nv);
      for (int l = 0; l < m; ++l)
        for (int i = 0; i < nv; ++i) gts[u][(size_t)l * nv + i] = G[(size_t)i * m + l];
      G = gts[u].data();
    }
    off[u] = pack_mpc_unit(in, folds, consts[u].data(), G, un.x0, un.x_ref, un.u_init, (size_t)m, (size_t)nv, (size_t)d,
                           (size_t)p, !cheap, fold);
  }
  double *d_in = nullptr, *d_w = nullptr, *d_sc = nullptr;
  NK_TRY(stage_pack(ctx, in, &d_in));
  if (folds.doubles()) NK_TRY(arena_alloc_t(ctx, folds.doubles(), &d_w));
  if (scores) {
    NK_TRY(arena_alloc_t(ctx, (size_t)n_units * n_scores, &d_sc));
    // a unit without rows writes its first NK_MPC_N_SCORES scores: the two behind them read 0
    if (n_scores > NK_MPC_N_SCORES && n_rows < n_units)
      NK_HIP(hipMemsetAsync(d_sc, 0, sizeof(double) * (size_t)n_units * n_scores, ctx->stream));
  }
  MatIn uo;
  MatOut ox, ou, oi;
  const int64_t sp = (int64_t)steps * p;
  if (n_uopt > 0) NK_TRY(stage_in(ctx, u_opt, sp, n_uopt, sp, &uo));
  if (out_x) NK_TRY(stage_out(ctx, out_x, d, (int64_t)n_units * (steps + 1), d, &ox));
  if (out_u) NK_TRY(stage_out(ctx, out_u, p, (int64_t)n_units * steps, p, &ou));
  if (out_info) NK_TRY(stage_out(ctx, out_info, 2, (int64_t)n_units * steps, 2, &oi));
  // the records of the two kinds, each in unit order: a kind is launched only when it has units
  std::vector<MpcLoopUnit> recs, orecs;
  std::vector<int> ktypes, oktypes;
  recs.reserve((size_t)(n_units - n_rows)); ktypes.reserve((size_t)(n_units - n_rows));
  orecs.reserve((size_t)n_rows); oktypes.reserve((size_t)n_rows);
  for (int u = 0; u < n_units; ++u) {
    const nk_mpc_unit& un = units[u];
    const nk_mpc_out* out = outs ? outs[u] : nullptr;
    const nk_model* mdl = un.model;
    const int m = mdl->m, nv = nvs[u], ny = out ? out->ny : 0, nt = nv + ny;
    // where the unit's pieces lie: with rows [F; T], Kb, S0'; without them F or K, M, H^-1.  (Only the offsets of the unit's
    // own kind were filled above; the other record is all zeros and is named in the untaken branches alone.)
    const MpcUnitOffsets& o = off[u];
    const MpcOutUnitOffsets& oo = ooff[u];
    const size_t at_G = out ? oo.FT : o.G, at_w = out ? oo.w : o.w, at_Kb = out ? oo.Kb : o.M, at_S0t = out ? oo.S0t : o.Hinv,
                 at_bnd = out ? oo.bnd : o.bnd, at_x0 = out ? oo.x0 : o.x0, at_xref = out ? oo.x_ref : o.x_ref,
                 at_uinit = out ? oo.u_init : o.u_init;
    MpcLoopUnit r;
    // the fold of the single call by the same call on the same operands (the rows of F, K or [F; T] have their leading
    // dimension there); the folds of all units are queued back to back, nothing waits between them
    r.w = d_in + at_G;
    if (mdl->kind != NK_MODEL_SPLINE) {
      double* wf = d_w + at_w;
      if (first[u] == u)
        NK_TRY(launch_gemm(ctx, false, true, m, nt, m, 1.0, mdl->Sinv, m, d_in + at_G, (int64_t)gain_row_reserve((size_t)m), 0.0,
                           wf, nt));
      r.w = wf;
    }
    r.Z = mdl->Z; r.winv = mdl->winv;
    r.Kb = d_in + at_Kb; r.S0t = d_in + at_S0t; r.bnd = d_in + at_bnd;
    r.x0 = d_in + at_x0; r.xref = d_in + at_xref; r.uinit = un.u_init ? d_in + at_uinit : nullptr;
    r.out_x = out_x ? ox.dev + (int64_t)u * (steps + 1) * ox.ld : nullptr; r.ldx = out_x ? ox.ld : 0;
    r.out_u = out_u ? ou.dev + (int64_t)u * steps * ou.ld : nullptr; r.ldu = out_u ? ou.ld : 0;
    r.out_info = out_info ? oi.dev + (int64_t)u * steps * oi.ld : nullptr;
    r.u_opt = un.uopt >= 0 ? uo.ptr + (int64_t)un.uopt * uo.ld : nullptr;
    r.score = scores ? d_sc + (size_t)n_scores * u : nullptr;
    r.sigma0sq = mdl->sigma0 * mdl->sigma0; r.rho = un.desc->rho; r.tol = un.desc->tol;
    r.theta = out ? mpc_out_theta(un.desc->rho, out->y_weight) : 0.0;
    r.m = m; r.nv = nv; r.ny = ny; r.iters = un.desc->iters;
    (out ? orecs : recs).push_back(r);
    (out ? oktypes : ktypes).push_back(mdl->ktype);
  }
  if (!recs.empty()) NK_TRY(launch_mpc_loop_multi(ctx, *plant, steps, recs.data(), ktypes.data(), (int)recs.size()));
  if (!orecs.empty()) NK_TRY(launch_mpc_out_loop_multi(ctx, *plant, steps, orecs.data(), oktypes.data(), (int)orecs.size()));
  if (out_x) NK_TRY(finish_out(ctx, ox));
  if (out_u) NK_TRY(finish_out(ctx, ou));
  if (out_info) NK_TRY(finish_out(ctx, oi));
  if (scores)
    NK_HIP(hipMemcpyAsync(scores, d_sc, sizeof(double) * (size_t)n_scores * (size_t)n_units, hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));  // (the staging block and the records are read by the copies queued above)
  return NK_OK;
}

extern "C" {

int nk_mpc_loop_multi(nk_ctx* ctx, const nk_poly_plant* plant, int32_t steps, const nk_mpc_unit* units, int32_t n_units,
                      const double* u_opt, int32_t n_uopt, double* out_x, double* out_u, double* out_info, double* scores) {
  return mpc_multi_run("nk_mpc_loop_multi", ctx, plant, steps, units, nullptr, n_units, u_opt, n_uopt, out_x, out_u, out_info,
                       scores, NK_MPC_N_SCORES);
}

int nk_mpc_out_loop_multi(nk_ctx* ctx, const nk_poly_plant* plant, int32_t steps, const nk_mpc_unit* units,
                          const nk_mpc_out* const* outs, int32_t n_units, const double* u_opt, int32_t n_uopt, double* out_x,
                          double* out_u, double* out_info, double* scores) {
  return mpc_multi_run("nk_mpc_out_loop_multi", ctx, plant, steps, units, outs, n_units, u_opt, n_uopt, out_x, out_u, out_info,
                       scores, NK_MPC_OUT_N_SCORES);
}

// every unit of nk_closed_loop_multi is checked before anything is queued
static int check_loop_unit(nk_ctx* ctx, int u, const nk_loop_unit& un, bool scored) {
  const nk_model* mdl = un.model;
  NK_REQUIRE(mdl != nullptr, "nk_closed_loop_multi: unit %d: the model is null", u);
  NK_REQUIRE(mdl->p >= 1 && mdl->p <= LOOP_MULTI_MAX_P, "nk_closed_loop_multi: unit %d: p = %d inputs must lie in 1 .. %d", u,
             mdl->p, LOOP_MULTI_MAX_P);
  NK_REQUIRE(mdl->m >= 1 && mdl->m <= LOOP_MULTI_MAX_M,
             "nk_closed_loop_multi: unit %d: m = %d must lie in 1 .. %d (larger models: nk_closed_loop)", u, mdl->m,
             LOOP_MULTI_MAX_M);
  NK_REQUIRE(mdl->d >= 1, "nk_closed_loop_multi: unit %d: d = %d", u, mdl->d);
  NK_REQUIRE(mdl->has_ops, "nk_closed_loop_multi: unit %d: the model holds no fitted operators", u);
  NK_REQUIRE(mdl->device == ctx->device, "nk_closed_loop_multi: unit %d: the model lives on device %d, the context on %d", u,
             mdl->device, ctx->device);
  NK_REQUIRE(un.K && un.phi0 && un.phi_ref, "nk_closed_loop_multi: unit %d: null argument (K, phi0, phi_ref)", u);
  NK_REQUIRE(un.target != nullptr || !scored,
             "nk_closed_loop_multi: unit %d: target is null, but out_err or scores are requested", u);
  NK_REQUIRE(!is_device_ptr(un.K) && !is_device_ptr(un.phi0) && !is_device_ptr(un.phi_ref) && !is_device_ptr(un.target) &&
                 !is_device_ptr(un.u_init),
             "nk_closed_loop_multi: unit %d: K, phi0, phi_ref, target and u_init must be host memory", u);
  return NK_OK;
}

int nk_closed_loop_multi(nk_ctx* ctx, int32_t steps, double c, const nk_loop_unit* units, int32_t n_units, double* out_x,
                         double* out_u, double* out_ucum, double* out_err, double* scores) {
  NK_TRY(check_ctx(ctx));
  NK_REQUIRE(!ctx_recording(ctx), "nk_closed_loop_multi: not available to the members of a lock-step group");
  NK_REQUIRE(units != nullptr && n_units >= 1, "nk_closed_loop_multi: n_units = %d units at %p: at least one is needed",
             n_units, (const void*)units);
  NK_REQUIRE(steps >= 1, "nk_closed_loop_multi: steps = %d must be positive", steps);
  NK_REQUIRE(std::isfinite(c) && c >= 0.0, "nk_closed_loop_multi: c must be finite and non-negative");
  NK_REQUIRE(out_x || out_u || out_ucum || out_err || scores,
             "nk_closed_loop_multi: out_x, out_u, out_ucum, out_err and scores are all null: nothing to return");
  NK_REQUIRE(!is_device_ptr(scores), "nk_closed_loop_multi: scores must be host memory");
  // the staging block (gains, lifted states, targets, seeds), the workspace and the dense, unit-major output offsets are
  // laid out while the units are checked
  UnitPack in, ws;
  std::vector<LoopUnitOffsets> off((size_t)n_units);
  std::vector<size_t> x_off((size_t)n_units), u_off((size_t)n_units), uc_off((size_t)n_units);
  size_t x_doubles = 0, u_doubles = 0, uc_doubles = 0;
  for (int u = 0; u < n_units; ++u) {
    const nk_loop_unit& un = units[u];
    NK_TRY(check_loop_unit(ctx, u, un, out_err != nullptr || scores != nullptr));
    const size_t m = (size_t)un.model->m, p = (size_t)un.model->p, d = (size_t)un.model->d;
    off[u] = pack_loop_unit(in, ws, un.K, un.phi0, un.phi_ref, un.target, un.u_init, m, p, d, (size_t)steps);
    x_off[u] = x_doubles;
    x_doubles += (size_t)steps * d;
    u_off[u] = u_doubles;
    u_doubles += (size_t)steps * p;
    uc_off[u] = uc_doubles;
    uc_doubles += ((size_t)steps + 1) * p;
  }
  double *d_in = nullptr, *d_ws = nullptr, *d_sc = nullptr;
  NK_TRY(stage_pack(ctx, in, &d_in));
  NK_TRY(arena_alloc_t(ctx, ws.doubles(), &d_ws));
  if (scores) NK_TRY(arena_alloc_t(ctx, (size_t)n_units * 4, &d_sc));
  // a dense output: the caller's device memory as it is, or an arena block that one copy brings back
  struct Out { double* host; double* dev; size_t doubles; };
  Out outs[4] = {{out_x, nullptr, x_doubles}, {out_u, nullptr, u_doubles}, {out_ucum, nullptr, uc_doubles},
                 {out_err, nullptr, (size_t)n_units * steps}};
  for (Out& o : outs) {
    if (!o.host) continue;
    if (is_device_ptr(o.host)) { o.dev = o.host; o.host = nullptr; }
    else NK_TRY(arena_alloc_t(ctx, o.doubles, &o.dev));
  }
  std::vector<LoopMultiUnit> recs((size_t)n_units);
  for (int u = 0; u < n_units; ++u) {
    const nk_model* mdl = units[u].model;
    const LoopUnitOffsets& o = off[u];
    LoopMultiUnit& r = recs[u];
    r = LoopMultiUnit{};
    r.G = mdl->A; r.ldg = mdl->m + mdl->p; r.C = mdl->C;
    r.K = d_in + o.K; r.phi0 = d_in + o.phi0; r.phi_ref = d_in + o.phi_ref;
    r.target = units[u].target ? d_in + o.target : nullptr;
    r.u_init = d_in + o.u_init;
    r.Phi = d_ws + o.Phi; r.usq = d_ws + o.usq; r.sse = d_ws + o.sse;
    r.out_x = outs[0].dev ? outs[0].dev + x_off[u] : nullptr; r.ldx = mdl->d;
    r.out_u = outs[1].dev ? outs[1].dev + u_off[u] : nullptr; r.ldu = mdl->p;
    r.out_ucum = outs[2].dev ? outs[2].dev + uc_off[u] : nullptr; r.ldc = mdl->p;
    r.out_err = outs[3].dev ? outs[3].dev + (size_t)u * steps : nullptr;
    r.score = scores ? d_sc + 4 * (size_t)u : nullptr;
    r.m = mdl->m; r.p = mdl->p; r.d = mdl->d;
  }
  NK_TRY(launch_closed_loop_multi(ctx, recs.data(), n_units, steps, c));
  for (const Out& o : outs)
    if (o.host) NK_HIP(hipMemcpyAsync(o.host, o.dev, o.doubles * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (scores) NK_HIP(hipMemcpyAsync(scores, d_sc, (size_t)n_units * 32, hipMemcpyDeviceToHost, ctx->stream));
  NK_HIP(hipStreamSynchronize(ctx->stream));  // (the staging block and recs are read by the copies queued above)
  return NK_OK;
}

}  // extern "C"
