"""Host-side mirror of the reference's estimator surface (regressors.py:32-55, 114-178): same constructor, same
public attributes, same fit / lift / predict shapes and error behaviour, so that the reference's drivers
(GridSearchCV, validate_dyn_sys, lqr_control, pickling) run unchanged -- with the arithmetic done by the HIP
kernels of libnyskoop.so through ctypes.  The DARE (control.dlqr in the reference) stays on the host by default;
solve_lqr(device=True) runs it on the device (the batched solver up to m = 256, the launch-chain solver beyond).
"""
import ctypes as C
import time

import os

import numpy as np
from sklearn.base import BaseEstimator

from . import _lib
from .dynamical_systems import PolynomialSystem
from .lqr import dlqr


def _lqr_gain_batch(regs, c, R=None, tol=1e-13, max_iter=40):
    """(Ks, status, iterations) of the device Riccati solvers for fitted regressors, in the callers' order.  The models
    within the batched solver's limits (m <= 256, p <= 8) go through nk_model_lqr_gain_batch together (one device call,
    chunked by the library; a model's result does not depend on what else the call holds); every other model goes through
    nk_model_lqr_gain, the launch-chain solver, one call each.  A module-level seam: tests without a GPU replace it."""
    ctx = _lib.get_context()
    handles = [r._ensure_model() for r in regs]
    dims = [(int(r._landmark_shape()[1]), int(r.n_inputs)) for r in regs]
    small = [u for u, (m, p) in enumerate(dims) if m <= DARE_BATCH_MAX_M and p <= DARE_BATCH_MAX_P]
    if len(small) == len(regs):
        return ctx.model_lqr_gain_batch(handles, c, R, tol=tol, max_iter=max_iter, dims=dims)
    Ks = [None] * len(regs)
    status = np.full(len(regs), -1, dtype=np.int32)
    iters = np.zeros(len(regs), dtype=np.int32)
    if small:
        Kb, sb, ib = ctx.model_lqr_gain_batch([handles[u] for u in small], c, R, tol=tol, max_iter=max_iter,
                                              dims=[dims[u] for u in small])
        for k, u in enumerate(small):
            Ks[u], status[u], iters[u] = Kb[k], sb[k], ib[k]
    for u, (m, p) in enumerate(dims):
        if Ks[u] is None:
            Ks[u], status[u], iters[u] = ctx.model_lqr_gain(handles[u], m, p, c, R, tol=tol, max_iter=max_iter)
    return Ks, status, iters


DARE_BATCH_MAX_M, DARE_BATCH_MAX_P = 256, 8  # limits of nk_dare_batch (include/nyskoop.h)
MPC_BUILD_MAX_ROWS = 4  # output rows per step of nk_model_mpc_build_batch (include/nyskoop.h)


def _mpc_build_batch(regs, c, R, specs, **solver):
    """(units, status, iterations) of nk_model_mpc_build_batch for fitted regressors in ONE device call: specs[u] = (N, comps,
    Ny); units[u] = dict(H, F, K, G, T).  A module-level seam: tests without a GPU replace it."""
    ctx = _lib.get_context()
    handles = [r._ensure_model() for r in regs]
    dims = [(int(r._landmark_shape()[1]), int(r.n_inputs)) for r in regs]
    return ctx.model_mpc_build_batch(handles, dims, c, R, specs, **solver)


def _mpc_controller_batch(regs, c, controller):
    """The controllers of fitted regressors for the checked `controller` dict of harness.lqr_sweep, built by ONE device call
    (reg.solve_mpc(..., device=True) for all of them at once).  Returns (controllers, status): a unit whose limits solve_mpc
    refuses has None and status -1 and is not part of the call; a unit with a non-zero build status has None."""
    n = len(regs)
    limits = [None] * n
    for i, reg in enumerate(regs):
        try:
            limits[i] = _mpc_limits(reg, controller["horizon"], controller["u_min"], controller["u_max"], controller["du_min"],
                                        controller["du_max"], controller.get("x_min"), controller.get("x_max"),
                                        controller.get("y_horizon"), device=True)
        except ValueError:
            pass
    live = [i for i in range(n) if limits[i] is not None]
    ctrls, status = [None] * n, np.full(n, -1, dtype=np.int32)
    if live:
        units, st, _ = _mpc_build_batch([regs[i] for i in live], c, None,
                                        [(controller["horizon"], limits[i]["comps"], limits[i]["Ny"]) for i in live])
        for k, i in enumerate(live):
            status[i] = int(st[k])
            if status[i] == 0:
                try:
                    ctrls[i] = _mpc_controller(units[k], limits[i], controller["horizon"], controller["rho"],
                                               controller.get("y_weight", np.inf))
                except (ValueError, np.linalg.LinAlgError):
                    pass
    return ctrls, status


def _mpc_limits(reg, horizon, u_min, u_max, du_min, du_max, x_min, x_max, y_horizon, device=False):
    """The checked limits of reg.solve_mpc: dict(lo, hi, dlo, dhi (nv entries each), xlo, xhi (d entries), comps (the state
    components with a finite bound), Ny).  Raises ValueError as solve_mpc does."""
    from . import lqr
    p = int(reg.n_inputs)
    lo, hi, dlo, dhi = lqr.mpc_bounds(int(horizon) * p, u_min, u_max, du_min, du_max)
    if np.any(lo > hi) or np.any(dlo > dhi):
        raise ValueError("u_min <= u_max and du_min <= du_max are required")
    lim = dict(lo=lo, hi=hi, dlo=dlo, dhi=dhi, xlo=None, xhi=None, comps=np.zeros(0, dtype=np.int64), Ny=None)
    if x_min is None and x_max is None:
        return lim
    d = int(reg._landmark_shape()[0]) if device else np.shape(reg.C)[0]

    def full(a, missing):
        if a is None:
            return np.full(d, missing)
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        if a.size not in (1, d):
            raise ValueError(f"a state bound of {a.size} entries, the model has {d} states")
        return np.ascontiguousarray(np.broadcast_to(a, (d,)))
    xlo, xhi = full(x_min, -np.inf), full(x_max, np.inf)
    if np.any(np.isnan(xlo)) or np.any(np.isnan(xhi)) or np.any(xlo > xhi):
        raise ValueError("x_min <= x_max is required")
    comps = np.flatnonzero(np.isfinite(xlo) | np.isfinite(xhi))
    if comps.size:
        Ny = int(horizon) if y_horizon is None else int(y_horizon)
        if device and comps.size > MPC_BUILD_MAX_ROWS:
            raise ValueError(f"{comps.size} state components have a finite bound: the device build takes at most "
                             f"{MPC_BUILD_MAX_ROWS} output rows per step")
        if device and not 1 <= Ny <= int(horizon):
            raise ValueError("the horizons must satisfy 1 <= Ny <= N")
        lim.update(xlo=xlo, xhi=xhi, comps=comps, Ny=Ny)
    return lim


def _mpc_controller(built, lim, horizon, rho, y_weight):
    """The lqr.MPCController / MPCOutputController of built matrices (H, F, K and G, T with rows) and checked limits."""
    from . import lqr
    H, F, K = built["H"], built["F"], built["K"]
    rho = lqr.mpc_default_rho(H) if rho is None else rho
    if lim["comps"].size == 0:
        return lqr.MPCController(H, F, lim["lo"], lim["hi"], lim["dlo"], lim["dhi"], K, rho, horizon)
    comps, Ny = lim["comps"], lim["Ny"]
    return lqr.MPCOutputController(H, F, lim["lo"], lim["hi"], lim["dlo"], lim["dhi"], K, rho, horizon, built["G"], built["T"],
                                   np.tile(lim["xlo"][comps], Ny), np.tile(lim["xhi"][comps], Ny), np.tile(comps, Ny), y_weight)


def _is_device_tensor(x):
    return hasattr(x, "data_ptr") and hasattr(x, "stride")


def linear_rollout(A, B, C, z0, controls, return_lifted=False):
    """Open-loop recursion z_{t+1} = A z_t + B u_t, x_t = C z_t on the device for explicit operators (nk_linear_rollout).

    z0: (m,) / (m, 1) with controls (p, T) -> simulated (d, T) [and lifted (m, T)]; column 0 is C z0 and the last control
    column is not used, exactly like the loop of validate_dyn_sys (benchmark_lqr_cloth.py:23-32).
    z0: (batch, m) with controls (batch, T, p) -> (batch, T, d) [and (batch, T, m)]."""
    ctx = _lib.get_context()
    A = np.ascontiguousarray(A, dtype=np.float64)
    C_ = np.ascontiguousarray(C, dtype=np.float64)
    m, d = A.shape[0], C_.shape[0]
    B = np.asarray(B, dtype=np.float64)
    B = np.ascontiguousarray(B.reshape(m, B.size // m))
    p = B.shape[1]
    if A.shape != (m, m) or C_.shape != (d, m):
        raise ValueError(f"operator shapes {A.shape}, {B.shape}, {C_.shape} do not fit together")
    controls = np.asarray(controls, dtype=np.float64)
    single = controls.ndim == 2
    if single:
        z0b = np.ascontiguousarray(np.asarray(z0, dtype=np.float64).reshape(1, m))
        U = np.ascontiguousarray(controls.T).reshape(1, controls.shape[1], p)
    else:
        z0b = np.ascontiguousarray(np.asarray(z0, dtype=np.float64).reshape(-1, m))
        U = np.ascontiguousarray(controls)
    batch, T = U.shape[0], U.shape[1]
    if U.shape != (batch, T, p) or z0b.shape[0] != batch:
        raise ValueError(f"controls have shape {U.shape}, expected {(z0b.shape[0], T, p)}")
    out_x = np.empty((batch, T, d))
    out_z = np.empty((batch, T, m)) if return_lifted else None
    _lib.check(ctx.lib.nk_linear_rollout(ctx.handle, A.ctypes.data, B.ctypes.data if p else None, C_.ctypes.data, m, d, p,
                                         z0b.ctypes.data, U.ctypes.data if p else None, T, batch, out_x.ctypes.data,
                                         None if out_z is None else out_z.ctypes.data))
    if single:
        return (out_x[0].T, out_z[0].T) if return_lifted else out_x[0].T
    return (out_x, out_z) if return_lifted else out_x


def open_loop_pack(trajs, controls, d, p):
    """Test trajectories (k, d, T) and controls (k, p, T or T-1) in the layout of nk_rollout_err / nk_sysid_grid: returns
    (k, T, d) and (k, T, p) contiguous arrays (the control row T-1 is never read and is zero when absent; None when p = 0
    or T = 1).  A single (d, T) trajectory with (p, .) controls is a batch of one.  Needs no GPU."""
    tr = np.asarray(trajs, dtype=np.float64)
    if tr.ndim == 2:
        tr = tr[None]
        controls = None if controls is None else np.asarray(controls, dtype=np.float64)[None]
    if tr.ndim != 3 or tr.shape[1] != d:
        raise ValueError(f"trajectories must be (k, {d}, T), got {tr.shape}")
    k, _, T = tr.shape
    out = np.ascontiguousarray(np.transpose(tr, (0, 2, 1)))
    if p == 0 or T == 1:
        return out, None
    ctrl = np.asarray(controls, dtype=np.float64)
    if ctrl.ndim != 3 or ctrl.shape[0] != k or ctrl.shape[1] != p or ctrl.shape[2] < T - 1:
        raise ValueError(f"controls have shape {ctrl.shape}, expected ({k}, {p}, >= {T - 1})")
    U = np.zeros((k, T, p))
    U[:, : min(T, ctrl.shape[2]), :] = np.transpose(ctrl[:, :, :T], (0, 2, 1))
    return out, U


class KoopmanRegressor(BaseEstimator):
    """regressors.py:32-55."""

    def __init__(self, n_inputs, gamma, m=None):
        self.gamma = gamma
        self.m = m
        self.A = None
        self.B = None
        self.C = None
        self.weights = None
        self.n_inputs = n_inputs

    def lift(self, X):
        raise NotImplementedError

    def fit(self, X, Y):
        raise NotImplementedError

    def rollout(self, x0, controls, return_lifted=False):
        """Open-loop forecast of validate_dyn_sys (benchmark_lqr_cloth.py:23-32; benchmark_lqr_hjb.py:23-44) for any
        estimator that provides `lift`, `A`, `B`, `C`: x0 (d,) with controls (p, T) -> simulated (d, T)."""
        z0 = self.lift(np.asarray(x0, dtype=np.float64).reshape(-1, 1))
        return linear_rollout(self.A, self.B, self.C, z0, controls, return_lifted)

    def predict(self, X_aug):
        """regressors.py:48-55 for a subclass that only provides `lift` and `weights`: the product W [phi; u] runs
        on the device through nk_gemm."""
        n_states = X_aug.shape[1] - self.n_inputs
        X = np.asarray(X_aug).T
        phi_X = np.ascontiguousarray(np.vstack((self.lift(X[:n_states, :]), X[n_states:, :])))
        W = np.ascontiguousarray(self.weights, dtype=np.float64)
        ctx = _lib.get_context()
        out = np.empty((W.shape[0], phi_X.shape[1]))
        _lib.check(ctx.lib.nk_gemm(ctx.handle, 0, 0, W.shape[0], phi_X.shape[1], W.shape[1], 1.0, W.ctypes.data,
                                   W.shape[1], phi_X.ctypes.data, phi_X.shape[1], 0.0, out.ctypes.data, out.shape[1]))
        return out.T


def _fetched(name):
    """Operator attribute of a fitted Nystrom regressor: `fit` queues the device->host copies and returns; the first
    access waits for them (nk_model_wait), so a sweep that fits the next candidate right away overlaps the copies of
    one fit with the kernels of the next.  Assigning an operator bumps a version counter that is part of the key of the
    cached device model, so predict / rollout never run on stale device copies; an IN-PLACE edit (`reg.A[0, 0] = 1`)
    cannot be seen -- follow it with `reg.A = reg.A` (or `reg.invalidate_device_model()`)."""
    key = "_" + name

    def get(self):
        self._wait_fetch()
        return self.__dict__.get(key)

    def set_(self, value):
        self._wait_fetch()
        self.__dict__[key] = value
        self.__dict__["_ops_version"] = self.__dict__.get("_ops_version", 0) + 1

    return property(get, set_)


_PLANT_MESSAGE = ("plant must be one of the package's dynamical systems (plant_id) or a PolynomialSystem, with its step length "
                  "Ts set")


def _check_plant(plant):
    """(plant_id, Ts, whether it is a PolynomialSystem) of a plant the single-launch loops take; ValueError otherwise."""
    plant_id, Ts = getattr(plant, "plant_id", None), getattr(plant, "Ts", None)
    poly = isinstance(plant, PolynomialSystem)
    if (plant_id is None and not poly) or Ts is None:
        raise ValueError(_PLANT_MESSAGE)
    return plant_id, Ts, poly


def _as_polynomial_plant(plant):
    """A PolynomialSystem as it is; a built-in plant as its table (the reference's RK4 variant)."""
    if isinstance(plant, PolynomialSystem):
        return plant
    plant_id, Ts, _ = _check_plant(plant)
    make = {_lib.NK_PLANT_DUFFING: PolynomialSystem.duffing, _lib.NK_PLANT_DOUBLE_INTEGRATOR: PolynomialSystem.double_integrator,
            _lib.NK_PLANT_HJB: PolynomialSystem.hjb}.get(plant_id)
    if make is None:
        raise ValueError(_PLANT_MESSAGE)
    return make(float(Ts))


def _single_or_batch(x0, x_ref, d, u_init=None, p=None):
    """(single, xb (batch, d), xr (batch, d), ui (batch, p) or None) of the states a plant loop is called with.  single: x0 is
    a vector or a (d, 1) column, as the reference's drivers pass states (with d = 1 a (1, 1) array is that column); else x0
    is (batch, d).  x_ref: one state for all loops or (batch, d); u_init: p entries for all loops or (batch, p)."""
    x0 = np.asarray(x0, dtype=np.float64)
    x_ref = np.asarray(x_ref, dtype=np.float64)
    single = x0.ndim < 2 or x0.shape == (d, 1)
    if x0.size % d:
        raise ValueError(f"initial states have shape {x0.shape}, the model has {d} states")
    xb = np.ascontiguousarray(x0.reshape(1, d) if single else x0.reshape(-1, d))
    batch = xb.shape[0]
    if x_ref.size not in (d, batch * d):
        raise ValueError(f"reference has shape {x_ref.shape}, expected one state of dimension {d} or {(batch, d)}")
    xr = np.ascontiguousarray(np.broadcast_to(x_ref.reshape(-1, d), (batch, d)))
    ui = None
    if u_init is not None:
        u_init = np.asarray(u_init, dtype=np.float64)
        if u_init.size not in (p, batch * p):
            raise ValueError(f"u_init has shape {u_init.shape}, expected {p} entries or {(batch, p)}")
        ui = np.ascontiguousarray(np.broadcast_to(u_init.reshape(-1, p), (batch, p)))
    return single, xb, xr, ui


class _DeviceModelRegressor(KoopmanRegressor):
    """What the estimators with a device model (nk_model) share: the asynchronous operator fetch, pickling through host
    copies, the model's lifetime, and lift / predict / rollout / closed loops on it.  An estimator names the attribute that
    holds its landmarks (`_landmarks_attr`, d x m), creates its model from host copies (`_create_model`) and fits."""

    A = _fetched("A")
    B = _fetched("B")
    C = _fetched("C")
    weights = _fetched("weights")
    _landmarks_attr = None
    _no_landmarks = "regressor has no landmarks: call fit first"

    def __init__(self, n_inputs, gamma, m):
        self._fetching = False
        super().__init__(n_inputs, gamma, m)
        self._model = None
        self._model_key = None
        self._stats = None
        self._ops_version = 0

    # ------------------------------------------------------------------------------------------------ plumbing
    def invalidate_device_model(self):
        """Forget the device copy of landmarks and operators (rebuilt from the host attributes at the next use)."""
        self._wait_fetch()
        self._drop_model()

    def _wait_fetch(self):
        if self.__dict__.get("_fetching"):
            self.__dict__["_fetching"] = False
            if self.__dict__.get("_fetch_lazy"):  # fit(..., fetch=False): copy the operators now, on first use
                self.__dict__["_fetch_lazy"] = False
                ctx = _lib.get_context()
                G, Cm, Wm = self.__dict__["_A"].base, self.__dict__["_C"], self.__dict__["_weights"]
                _lib.check(ctx.lib.nk_model_get_ops(ctx.handle, self._model, G.ctypes.data, G.shape[1], Cm.ctypes.data,
                                                    Cm.shape[1], Wm.ctypes.data, Wm.shape[1]))
            else:
                _lib.check(_lib.load_library().nk_model_wait(self._model))

    def __getstate__(self):
        self._wait_fetch()
        state = dict(self.__dict__)
        state["_fetch_lazy"] = False
        state["_model"] = None  # device handles never travel (benchmark_lqr_cloth.py:266-267 pickles regressors)
        state["_model_key"] = None
        return state

    def __setstate__(self, state):
        for name in ("A", "B", "C", "weights"):  # states written before the operators became properties
            if name in state:
                state["_" + name] = state.pop(name)
        self.__dict__.update(state)
        self.__dict__["_fetching"] = False
        self.__dict__.setdefault("_model", None)
        self.__dict__.setdefault("_model_key", None)
        self.__dict__.setdefault("_stats", None)
        self.__dict__.setdefault("_ops_version", 0)

    def __del__(self):
        try:
            self._drop_model()
        except Exception:
            pass

    def _drop_model(self):
        if getattr(self, "_model", None):
            self.__dict__["_fetching"] = False  # nk_model_destroy waits for a pending fetch itself
            _lib.load_library().nk_model_destroy(self._model)
            self._model = None
            self._model_key = None

    def _create_model(self, ctx, Z, p, pa, pb, pc, pw):
        """Handle of a new device model with landmarks Z (m x d) and the operators behind the four pointers (or None)."""
        raise NotImplementedError

    def _ensure_model(self):
        """Device model for lift / predict / rollout; rebuilt from host copies after un-pickling or when a caller
        replaced the landmarks / operators by hand."""
        landmarks = self._landmarks()
        if landmarks is None:
            raise RuntimeError(self._no_landmarks)
        key = self._ops_key()
        if self._model is not None and self._model_key == key:
            return self._model
        self._wait_fetch()
        self._drop_model()
        ctx = _lib.get_context()
        Z = np.ascontiguousarray(np.asarray(landmarks, dtype=np.float64).T)  # m x d
        m, d = Z.shape
        p = int(self.n_inputs)
        keep = []

        def ptr(a, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != shape:
                raise ValueError(f"operator has shape {a.shape}, expected {shape}")
            keep.append(a)
            return a.ctypes.data

        h = self._create_model(ctx, Z, p, ptr(self.A, (m, m)), ptr(self.B, (m, p)), ptr(self.C, (d, m)),
                               ptr(self.weights, (d, m + p)))
        self._model, self._model_key = h, key
        return h

    @staticmethod
    def _ranges(row_ranges):
        if row_ranges is None:
            return None, 0, None
        flat = np.ascontiguousarray(np.asarray(row_ranges, dtype=np.int64).reshape(-1))
        return flat.ctypes.data_as(C.POINTER(C.c_int64)), flat.size // 2, flat

    def _adopt(self, ctx, h, stats, m, d, p, t_host, fetch=True):
        """Take over a freshly fitted device model: queue the copies of the operators into page-locked arrays
        (fetch=False: leave them on the device until an attribute is read -- sweeps that only score never pay the copy)."""
        t_host2 = time.perf_counter()
        self._model = h
        self._stats = stats.as_dict()
        if fetch:
            G = _lib.pinned_empty((m, m + p))  # page-locked: the device->host copies run at the PCIe rate
            Cm = _lib.pinned_empty((d, m))
            Wm = _lib.pinned_empty((d, m + p))
        else:
            G, Cm, Wm = np.empty((m, m + p)), np.empty((d, m)), np.empty((d, m + p))
        t_host2b = time.perf_counter()
        self.__dict__.update(_A=G[:, :m], _B=G[:, m:], _C=Cm, _weights=Wm)  # A, B: views of G_ls (regressors.py:158-159)
        if fetch:
            _lib.check(ctx.lib.nk_model_get_ops_async(ctx.handle, h, G.ctypes.data, m + p, Cm.ctypes.data, m,
                                                      Wm.ctypes.data, m + p))
        self.__dict__["_fetch_lazy"] = not fetch
        self._fetching = True
        t_host3 = time.perf_counter()
        self._stats.update(host_ms_drop=(t_host[1] - t_host[0]) * 1e3, host_ms_call=(t_host2 - t_host[1]) * 1e3,
                           host_ms_fetch=(t_host3 - t_host2) * 1e3, host_ms_pinned=(t_host2b - t_host2) * 1e3)
        self._model_key = self._ops_key()

    def _landmarks(self):
        return getattr(self, self._landmarks_attr)

    def _landmark_shape(self):
        """(d, m) of the landmarks the device model lifts with."""
        return np.asarray(self._landmarks()).shape

    def _ops_key(self):
        # landmarks are a plain attribute (the reference's callers assign them): identity + shape; operators: the
        # version counter bumped by every assignment (ids alone could be reused by a new array after a free)
        z = self._landmarks()
        return (id(z), None if z is None else np.shape(z), self.__dict__.get("_ops_version", 0))

    # ------------------------------------------------------------------------------------------------ lift / predict
    def lift(self, X):
        """regressors.py:171-178: X is d x n_q (not augmented); returns phi, m x n_q."""
        ctx = _lib.get_context()
        h = self._ensure_model()
        Xq = _lib.Mat(X.t() if _is_device_tensor(X) else np.asarray(X, dtype=np.float64).T)
        nq = Xq.shape[0]
        m = self._landmark_shape()[1]
        out = np.empty((nq, m))
        ctx.wait_for(X)
        _lib.check(ctx.lib.nk_lift(ctx.handle, h, Xq.ptr, Xq.ld, nq, out.ctypes.data, m))
        return out.T

    def predict(self, X_aug):
        """regressors.py:48-55: X_aug is n_q x (d+p); returns n_q x d."""
        ctx = _lib.get_context()
        h = self._ensure_model()
        Xm = _lib.Mat(X_aug)
        d = self._landmark_shape()[0]
        if Xm.shape[1] != d + int(self.n_inputs):
            raise ValueError(f"X_aug has {Xm.shape[1]} columns, expected {d + int(self.n_inputs)}")
        out = np.empty((Xm.shape[0], d))
        ctx.wait_for(X_aug)
        _lib.check(ctx.lib.nk_predict(ctx.handle, h, Xm.ptr, Xm.ld, Xm.shape[0], out.ctypes.data, d))
        return out

    def score_neg_rmse(self, X_aug, Y):
        """sklearn's 'neg_root_mean_squared_error' of predict(X_aug) against Y, reduced on the device
        (benchmark_lqr_cloth.py:55)."""
        ctx = _lib.get_context()
        h = self._ensure_model()
        Xm, Ym = _lib.Mat(X_aug), _lib.Mat(Y)
        d = self._landmark_shape()[0]
        if Xm.shape[1] != d + int(self.n_inputs):
            raise ValueError(f"X_aug has {Xm.shape[1]} columns, expected {d + int(self.n_inputs)}")
        if Ym.shape != (Xm.shape[0], d):
            raise ValueError(f"Y has shape {Ym.shape}, expected {(Xm.shape[0], d)}")
        if Xm.shape[0] == 0:
            raise ValueError("score_neg_rmse needs at least one row")
        s = C.c_double()
        ctx.wait_for(X_aug, Y)
        _lib.check(ctx.lib.nk_score_neg_rmse(ctx.handle, h, Xm.ptr, Xm.ld, Ym.ptr, Ym.ld, Xm.shape[0], C.byref(s)))
        return s.value

    # ------------------------------------------------------------------------------------------------ callers' loops
    def rollout(self, x0, controls, return_lifted=False):
        """Open-loop forecast of validate_dyn_sys (benchmark_lqr_cloth.py:23-32).

        x0: (d,) / (d,1) with controls (p, T)  -> simulated (d, T) [and lifted (m, T)];
        x0: (batch, d) with controls (batch, T, p) -> (batch, T, d) [and (batch, T, m)]."""
        ctx = _lib.get_context()
        h = self._ensure_model()
        d, m = self._landmark_shape()
        p = int(self.n_inputs)
        controls = np.asarray(controls, dtype=np.float64)
        single = controls.ndim == 2
        if single:
            x0b = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(1, d))
            U = np.ascontiguousarray(controls.T).reshape(1, controls.shape[1], p)
        else:
            x0b = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(-1, d))
            U = np.ascontiguousarray(controls)
        batch, T = U.shape[0], U.shape[1]
        out_x = np.empty((batch, T, d))
        out_z = np.empty((batch, T, m)) if return_lifted else None
        _lib.check(ctx.lib.nk_rollout(ctx.handle, h, x0b.ctypes.data, d, U.ctypes.data, T, batch, out_x.ctypes.data,
                                      None if out_z is None else out_z.ctypes.data))
        if single:
            return (out_x[0].T, out_z[0].T) if return_lifted else out_x[0].T
        return (out_x, out_z) if return_lifted else out_x

    def open_loop_errors(self, trajs, controls, relative=False):
        """validate_dyn_sys (benchmark_lqr_cloth.py:18-36; relative=True: the %-form of benchmark_lqr_classic.py:39) for k
        test trajectories in one device call that returns k numbers (nk_rollout_err): the forecast is rolled out from each
        trajectory's first state and compared with it on the device -- the simulated trajectories are never formed.
        trajs: (k, d, T) (or one (d, T)); controls: (k, p, T) or (k, p, T-1) (or (p, .)).  Returns (k,) errors."""
        ctx = _lib.get_context()
        h = self._ensure_model()
        d, m = self._landmark_shape()
        p = int(self.n_inputs)
        tr, U = open_loop_pack(trajs, controls, d, p)
        k, T = tr.shape[0], tr.shape[1]
        out = np.empty(k)
        ptr = out.ctypes.data_as(C.POINTER(C.c_double))
        rc = ctx.lib.nk_rollout_err(ctx.handle, h, tr.ctypes.data, None if U is None else U.ctypes.data, T, k,
                                    None if relative else ptr, ptr if relative else None)
        _lib.check_mapped(rc)
        return out

    def closed_loop(self, K, phi0, phi_ref, num_steps):
        """Lifted closed loop of lqr_control (benchmark_lqr_cloth.py:79-84).

        phi0, phi_ref: (m,) / (m, 1)  -> (visited (d, steps), u_ops (p, steps));
        phi0, phi_ref: (batch, m)     -> (visited (batch, steps, d), u_ops (batch, steps, p)): independent loops that share
        the gain (several initial states / references in one call)."""
        ctx = _lib.get_context()
        h = self._ensure_model()
        d, m = self._landmark_shape()
        p = int(self.n_inputs)
        K = np.ascontiguousarray(K, dtype=np.float64)
        if K.shape != (p, m):
            raise ValueError(f"gain has shape {K.shape}, expected {(p, m)}")
        phi0 = np.asarray(phi0, dtype=np.float64)
        phi_ref = np.asarray(phi_ref, dtype=np.float64)
        single = phi0.ndim < 2 or phi0.shape[1] == 1  # a vector or the (m, 1) column that `lift` returns
        if single:
            f0 = np.ascontiguousarray(phi0.reshape(1, m))
            fr = np.ascontiguousarray(phi_ref.reshape(1, m))
        else:
            f0 = np.ascontiguousarray(phi0.reshape(-1, m))
            fr = np.ascontiguousarray(np.broadcast_to(phi_ref.reshape(-1, m), f0.shape))
        ox, ou = ctx.closed_loop_batch(h, K, f0, fr, num_steps, d)
        return (ox[0].T, ou[0].T) if single else (ox, ou)

    def closed_loop_plant(self, K, x0, x_ref, num_steps, plant):
        """LQR closed loop around the TRUE plant (lqr_control of benchmark_lqr_hjb.py:73-97 / benchmark_lqr_classic.py:67-89):
        u_t = K (phi(x_ref) - phi(x_t)), x_{t+1} = plant(x_t, u_t), all `num_steps` steps in one device launch
        (nk_plant_loop).  `plant`: one of dynamical_systems.DuffingOscillator / DoubleIntegrator / HJB (its `plant_id` and
        `Ts` are used), whose state dimension is the model's; one input.  Or a dynamical_systems.PolynomialSystem
        (nk_poly_plant_loop): up to four states and four inputs, the model's; K is (p, m) and u below has p rows / columns.

        x0: (d,) / (d, 1)  -> (states (d, num_steps + 1) with x0 first, u (1, num_steps)); a (1, 1) array with d = 1 is this case;
        x0: (batch, d)     -> (states (batch, num_steps + 1, d), u (batch, num_steps, 1)): independent loops that share the
        gain; x_ref: one state for all of them or (batch, d).  A loop's results do not depend on the batch it runs in."""
        ctx = _lib.get_context()
        h = self._ensure_model()
        d, m = self._landmark_shape()
        p = int(self.n_inputs)
        plant_id, Ts, poly = _check_plant(plant)
        K = np.ascontiguousarray(K, dtype=np.float64)
        if K.shape != (p, m):
            raise ValueError(f"gain has shape {K.shape}, expected {(p, m)}")
        single, xb, xr, _ = _single_or_batch(x0, x_ref, d)
        if poly:
            ox, ou = ctx.poly_plant_loop(h, plant.descriptor(), K, xb, xr, int(num_steps))
        else:
            ox, ou = ctx.plant_loop(h, plant_id, Ts, K, xb, xr, int(num_steps))
        return (ox[0].T, ou[0].T) if single else (ox, ou)

    def solve_mpc(self, horizon, c=1.0, R=None, u_min=None, u_max=None, du_min=None, du_max=None, Q=None, rho=None,
                  x_min=None, x_max=None, y_horizon=None, y_weight=np.inf, device=False):
        """The constrained Koopman MPC of this model: lqr.MPCController with the condensed QP of
        sum_{k<N} (e_k'Q e_k + u_k'R u_k) + e_N'P e_N over the horizon N (lqr.mpc_condense on the host; Q = c sym(C'C), R = I
        by default; P and the gain K from lqr.dlqr, refined by two Newton steps (lqr.dare_refine) so that the first move of the
        unconstrained QP is K to rounding -- K differs from solve_lqr's by the residual scipy leaves, 1e-6 .. 1e-11 relative),
        the box u_min <= u_k <= u_max and the rate limits
        du_min <= u_k - u_{k-1} <= du_max (scalars, p entries or N p entries; None = no limit), and the ADMM step
        rho = sqrt(lambda_min(H) lambda_max(H)) unless given.  N p <= 64 for the device loop (closed_loop_plant_mpc).

        x_min / x_max (scalars or d entries; +-inf or None for a free component) limit the PREDICTED states C e_k + x_ref over
        the steps k = 1 .. y_horizon (default N): every component with a finite bound gets one output row per step
        (lqr.mpc_condense_outputs) and the result is an lqr.MPCOutputController.  y_weight = np.inf makes the rows hard
        constraints; a finite y_weight > 0 penalises the squared violation with that weight (always feasible: a plant pushed
        outside its limits needs this; weights far above rho, 1e3 rho say, converge very slowly).  The rows of a sampled plant
        are small beside the identity rows of the inputs, so the output rows want a rho far above the default (300 x the
        default reached a hard velocity limit within 2 % in 100 iterations on the Duffing models; with the default the
        controls did not move).  N p + rows <= 64 for the device loop.  Without these arguments the result is what it always was.

        device=True: the same controller built by ONE nk_model_mpc_build_batch call (csrc/nk_mpc_build.hip): Q = c sym(C'C)
        formed on the device from the model's own operators (so Q must be None), P and K by the doubling Riccati solver and one
        Newton step (lqr.dare_newton_smith), H, F (lqr.mpc_condense_blocked) and G, T on the device; rho, the bounds and the row
        bookkeeping stay on the host.  m <= 512, p <= 4, at most 4 bounded state components.  Raises np.linalg.LinAlgError
        when the build reports a non-zero status, as lqr.dlqr_device does."""
        from . import lqr
        p = int(self.n_inputs)
        if device:
            if Q is not None:
                raise ValueError("solve_mpc(device=True) forms Q = c sym(C'C) on the device: pass c, not Q")
            lim = _mpc_limits(self, horizon, u_min, u_max, du_min, du_max, x_min, x_max, y_horizon, device=True)
            units, status, _ = _mpc_build_batch([self], c, R, [(int(horizon), lim["comps"], lim["Ny"])])
            if int(status[0]) != 0:
                raise np.linalg.LinAlgError(f"device controller build failed with status {int(status[0])} (1: the doubling "
                                            "iteration reached max_iter, 2: non-finite values or a matrix that is not positive "
                                            "definite, 3: the Smith iteration reached its cap)")
            return _mpc_controller(units[0], lim, horizon, rho, y_weight)
        if Q is None:
            Q = c * self.C.T @ self.C
            Q = (Q + Q.T) / 2
        if R is None:
            R = np.eye(p)
        A, B = np.asarray(self.A, dtype=np.float64), np.asarray(self.B, dtype=np.float64)
        K, P = lqr.dare_refine(A, B, Q, R, dlqr(A, B, Q, R)[0])
        H, F = lqr.mpc_condense(A, B, Q, R, P, horizon)
        lim = _mpc_limits(self, horizon, u_min, u_max, du_min, du_max, x_min, x_max, y_horizon)
        built = dict(H=H, F=F, K=K)
        if lim["comps"].size:
            built["G"], built["T"] = lqr.mpc_condense_outputs(A, B, np.asarray(self.C, dtype=np.float64)[lim["comps"]], horizon,
                                                              lim["Ny"])
        return _mpc_controller(built, lim, horizon, rho, y_weight)

    def closed_loop_plant_mpc(self, controller, x0, x_ref, num_steps, plant, iters=50, tol=0.0, u_init=None,
                              return_info=False):
        """Constrained MPC closed loop around the TRUE plant, all `num_steps` steps in one device launch (nk_mpc_loop): per
        step the QP of `controller` (solve_mpc) at e = phi(x_t) - phi(x_ref) by `iters` ADMM iterations (stopped early when
        max |s - z| <= tol; tol = 0 runs all of them), the first move applied, x_{t+1} = plant(x_t, u_t).  A returned control
        never violates a rate limit, nor a bound when u_init lies within the bounds and du_min <= 0 <= du_max, whatever
        `iters` is.  When the limits are inactive the loop is the LQR loop of closed_loop_plant to rounding.

        iters = 0 is the SATURATED LQR, u_t = clip(clip(K (phi(x_ref) - phi(x_t)), u_min, u_max), u_{t-1} + du_min,
        u_{t-1} + du_max), at about twice the LQR step of closed_loop_plant (measured: 3.3 against 1.7 us per step at
        m = 20).  A single-input user with bounds alone should take this mode: with one
        input, a symmetric box and the Riccati terminal cost the first move of the QP EQUALS the clipped LQR control
        (measured on the Duffing models, Matern-5/2, m = 40 and 200, c = 1 .. 1e4, horizons 5 .. 64: equal to 1e-15 of the
        bound at every one of 300 steps), so the QP pays for itself only with rate limits or several inputs.

        `plant`: a PolynomialSystem, or one of the built-in plants, which runs as its table (PolynomialSystem.duffing / .hjb /
        .double_integrator: the reference's RK4 variant).  Shapes and single / batch conventions of closed_loop_plant; u_init
        (p,) or (batch, p), zeros by default, is the control applied before the first step.  return_info=True adds info
        (steps, 2) / (batch, steps, 2) = {iterations run, final max |s - z|} per step.
        Limits: N p <= 64, p <= 4, d <= 4, m <= 512 and 8 (m N p + 64 ceil(m / 64) + 16) bytes <= 160 KB."""
        ctx = _lib.get_context()
        h = self._ensure_model()
        d, m = self._landmark_shape()
        p = int(self.n_inputs)
        plant = _as_polynomial_plant(plant)
        if controller.K.shape != (p, m) or controller.F.shape[1] != m:
            raise ValueError(f"the controller is for a model with K of shape {controller.K.shape}, expected {(p, m)}")
        single, xb, xr, ui = _single_or_batch(x0, x_ref, d, u_init, p)
        ds, keep = _lib.mpc_desc(controller, iters, tol)
        out = None
        if hasattr(controller, "ycomp") and int(iters) != 0:  # an lqr.MPCOutputController (iters = 0: the saturated LQR)
            out, keep_out = _lib.mpc_out(controller)
            keep.append(keep_out)
        ox, ou, oi = ctx.mpc_loop(h, plant.descriptor(), ds, xb, xr, int(num_steps), ui, return_info, out)
        del keep
        if single:
            return (ox[0].T, ou[0].T, oi[0]) if return_info else (ox[0].T, ou[0].T)
        return (ox, ou, oi) if return_info else (ox, ou)

    def solve_lqr(self, Q=None, R=None, c=0.0075, device=False):
        """Host DARE, standing in for control.dlqr(A, B, Q, R) (benchmark_lqr_cloth.py:238-240,262): by default
        Q = c * C^T C symmetrised and R = I.  Returns the gain K (p x m).
        device=True: the device solvers with this one model (Q = c sym(C'C) formed on the device from the model's own
        operators, so Q must be None): the batched solver for m <= 256, p <= 8 (nk_model_lqr_gain_batch), the
        launch-chain solver beyond (nk_model_lqr_gain; m <= 10240, p <= 32); raises np.linalg.LinAlgError when the
        iteration does not converge or breaks down, as scipy does."""
        if device:
            if Q is not None:
                raise ValueError("solve_lqr(device=True) forms Q = c sym(C'C) on the device: pass c, not Q")
            Ks, status, _ = _lqr_gain_batch([self], c, R)
            if int(status[0]) != 0:
                raise np.linalg.LinAlgError(f"device Riccati solve failed with status {int(status[0])} "
                                            "(1: max_iter reached, 2: non-finite values or a singular pivot)")
            return Ks[0]
        if Q is None:
            Q = c * self.C.T @ self.C
            Q = (Q + Q.T) / 2
        if R is None:
            R = np.eye(int(self.n_inputs))
        K, _ = dlqr(self.A, self.B, Q, R)
        return K

    @property
    def fit_stats_(self):
        return self._stats


class KoopmanNystromRegressor(_DeviceModelRegressor):
    """regressors.py:114-178, MI355X-native.

    Differences a caller can observe (all additive): `lift`/`predict` reuse K_mm^{-1/2} computed at fit time instead
    of re-running sqrtm per call (regressors.py:174-175); `fit` accepts `row_ranges` (training rows of a K-fold split
    without copying) and device-resident inputs; `rollout`, `score_neg_rmse`, `closed_loop` and `solve_lqr` expose
    the callers' inner loops (benchmark_lqr_cloth.py:18-36, 52-57, 69-104, 238-263) as single calls.
    """

    # Arithmetic of the O(n m d) kernel blocks and O(n m^2) Gram contractions of `fit` and `gram_partial`: "f64" (the only
    # mode that meets the 1e-6 operator bar) or "f32" (BASELINE.json's stress configuration; include/nyskoop.h, nk_set_compute_dtype).  An
    # attribute, not a constructor argument: the constructor mirrors the reference's (sklearn clone / get_params), and a
    # clone starts from the default.
    compute_dtype = "f64"
    # How `fit` chooses landmarks when none are set: "uniform" (the reference's draw, regressors.py:129-132), or "greedy" /
    # "rpcholesky": pivoted-Cholesky selection on the device over the fit's training rows (landmarks.select_landmarks),
    # stopped early by landmark_tol (the fit then has fewer than m landmarks).  Attributes like compute_dtype: not
    # constructor arguments, and a clone starts from the defaults.
    landmark_rule = "uniform"
    landmark_tol = 0.0
    _landmarks_attr = "nystrom_centers_output"

    def __init__(self, n_inputs, kernel=None, gamma=None, m=None):
        super().__init__(n_inputs, gamma, m)
        self.kernel = kernel
        self.nystrom_centers_input = None
        self.nystrom_centers_output = None
        self.jitter = 1e-6

    def _create_model(self, ctx, Z, p, pa, pb, pc, pw):
        m, d = Z.shape
        kd, keep = self.kernel.kernel.desc(d)
        h = C.c_void_p()
        rc = ctx.lib.nk_model_create(ctx.handle, C.byref(kd), Z.ctypes.data, d, m, d, p, float(self.jitter),
                                     pa, pb, pc, pw, C.byref(h))
        _lib.check_mapped(rc)
        return h

    # ------------------------------------------------------------------------------------------------ fit
    def _prepare(self, n, d, Y=None, row_ranges=None):
        """Landmarks (regressors.py:129-134) and kernel descriptor for a fit on d-dimensional states."""
        if self.nystrom_centers_output is None:  # regressors.py:129-132: global legacy NumPy RNG, n = #samples
            if Y is None:
                raise RuntimeError("landmarks must be set before a fit from Gram blocks")
            if self.landmark_rule != "uniform":
                from .landmarks import select_landmarks
                idx = select_landmarks(Y, self.kernel, self.m, rule=self.landmark_rule, row_ranges=row_ranges,
                                       tol=self.landmark_tol)
            else:
                idx = np.random.choice(np.arange(0, n), size=self.m, replace=False)
            if _is_device_tensor(Y):
                rows = Y[idx.tolist()]
                self.nystrom_centers_output = np.ascontiguousarray(rows.cpu().numpy().T)
            else:
                self.nystrom_centers_output = np.asarray(Y).T[:, idx]
        if self.nystrom_centers_input is None:  # regressors.py:133-134
            self.nystrom_centers_input = self.nystrom_centers_output
        Zo = np.ascontiguousarray(np.asarray(self.nystrom_centers_output, dtype=np.float64).T)
        if Zo.shape[1] != d:
            raise ValueError(f"landmarks have dimension {Zo.shape[1]}, data has {d}")
        same = self.nystrom_centers_input is self.nystrom_centers_output
        Zi = Zo if same else np.ascontiguousarray(np.asarray(self.nystrom_centers_input, dtype=np.float64).T)
        kd, keep = self.kernel.kernel.desc(d)
        return Zo, Zi, same, kd, keep

    def fit(self, X, Y, row_ranges=None, fetch=True):
        """regressors.py:122-169.  X: n x (d+p) rows [state | input], Y: n x d (NumPy arrays, or float64 device
        tensors already resident in HBM).  Returns None, like the reference."""
        ctx = _lib.get_context()
        Xm, Ym = _lib.Mat(X), _lib.Mat(Y)
        n, d = Ym.shape
        p = int(self.n_inputs)
        if Xm.shape != (n, d + p):
            raise ValueError(f"X has shape {Xm.shape}, expected {(n, d + p)}")
        Zo, Zi, same, kd, keep = self._prepare(n, d, Y, row_ranges)
        m = Zo.shape[0]
        rr, n_rr, keep_rr = self._ranges(row_ranges)
        stats = _lib.FitStats()
        h = C.c_void_p()
        t_host0 = time.perf_counter()
        self._drop_model()
        t_host1 = time.perf_counter()
        ctx.wait_for(X, Y)  # device tensors: whatever torch still has queued for them comes first
        ctx.set_compute_dtype(self.compute_dtype)
        try:
            rc = ctx.lib.nk_nystrom_fit(ctx.handle, C.byref(kd), Xm.ptr, Xm.ld, Ym.ptr, Ym.ld, n, d, p, rr, n_rr,
                                        None if same else Zi.ctypes.data, d, Zo.ctypes.data, d, m,
                                        float(self.gamma), float(self.jitter), C.byref(h), C.byref(stats))
        finally:
            if self.compute_dtype != "f64":
                ctx.set_compute_dtype("f64")
        _lib.check_mapped(rc)
        self._adopt(ctx, h, stats, m, d, p, (t_host0, t_host1), fetch)

    # ------------------------------------------------------------------------- sample-sharded fit
    def gram_size(self, d):
        """Number of float64 entries of the packed Gram accumulator for d-dimensional states."""
        m = np.asarray(self.nystrom_centers_output).shape[1] if self.nystrom_centers_output is not None else int(self.m)
        cnt = C.c_int64()
        _lib.check(_lib.load_library().nk_gram_doubles(m, d, int(self.n_inputs), C.byref(cnt)))
        return int(cnt.value)

    def gram_partial(self, X, Y, row_ranges=None, out=None):
        """The four Gram blocks of regressors.py:151,153,162,164 (without the regularisers) over the given rows only,
        packed into one flat float64 buffer `out` (a NumPy array, or a 1-D device tensor which is then filled in
        place without leaving the GPU).  Landmarks must be set: every shard of a sharded fit uses the same ones."""
        ctx = _lib.get_context()
        Xm, Ym = _lib.Mat(X), _lib.Mat(Y)
        n, d = Ym.shape
        p = int(self.n_inputs)
        if Xm.shape != (n, d + p):
            raise ValueError(f"X has shape {Xm.shape}, expected {(n, d + p)}")
        if self.nystrom_centers_output is None:
            raise RuntimeError("landmarks must be set before gram_partial (all shards share them)")
        Zo, Zi, same, kd, keep = self._prepare(n, d)
        m = Zo.shape[0]
        cnt = self.gram_size(d)
        if out is None:
            out = np.empty(cnt)
        if _is_device_tensor(out):
            if out.dim() != 1 or out.numel() != cnt or not out.is_contiguous() or "float64" not in str(out.dtype):
                raise ValueError(f"out must be a contiguous float64 tensor with {cnt} entries")
            optr = out.data_ptr()
        else:
            if out.shape != (cnt,) or out.dtype != np.float64 or not out.flags.c_contiguous:
                raise ValueError(f"out must be a contiguous float64 array with {cnt} entries")
            optr = out.ctypes.data
        rr, n_rr, keep_rr = self._ranges(row_ranges)
        stats = _lib.FitStats()
        ctx.wait_for(X, Y, out)
        ctx.set_compute_dtype(self.compute_dtype)  # as in `fit`: the shards of a sharded fit use the engine the attribute names
        try:
            rc = ctx.lib.nk_nystrom_gram(ctx.handle, C.byref(kd), Xm.ptr, Xm.ld, Ym.ptr, Ym.ld, n, d, p, rr, n_rr,
                                         None if same else Zi.ctypes.data, d, Zo.ctypes.data, d, m, optr, C.byref(stats))
        finally:
            if self.compute_dtype != "f64":
                ctx.set_compute_dtype("f64")
        _lib.check_mapped(rc)
        self._gram_stats = stats.as_dict()
        return out

    def fit_from_gram(self, gram, n_total, d):
        """Finish the fit from accumulated Gram blocks (the sum of gram_partial over all shards); n_total = number of
        training rows over all shards (the `n` of regressors.py:127)."""
        ctx = _lib.get_context()
        p = int(self.n_inputs)
        Zo, Zi, same, kd, keep = self._prepare(n_total, d)
        m = Zo.shape[0]
        cnt = self.gram_size(d)
        if _is_device_tensor(gram):
            if gram.numel() != cnt or not gram.is_contiguous() or "float64" not in str(gram.dtype):
                raise ValueError(f"gram must be a contiguous float64 tensor with {cnt} entries")
            gptr = gram.data_ptr()
        else:
            gram = np.ascontiguousarray(gram, dtype=np.float64).reshape(-1)
            if gram.size != cnt:
                raise ValueError(f"gram must have {cnt} entries")
            gptr = gram.ctypes.data
        stats = _lib.FitStats()
        h = C.c_void_p()
        t_host0 = time.perf_counter()
        self._drop_model()
        t_host1 = time.perf_counter()
        ctx.wait_for(gram)  # e.g. the output of an all-reduce still running on torch's (RCCL's) stream
        rc = ctx.lib.nk_nystrom_solve(ctx.handle, C.byref(kd), None if same else Zi.ctypes.data, d, Zo.ctypes.data, d, m,
                                      d, p, gptr, int(n_total), float(self.gamma), float(self.jitter), C.byref(h),
                                      C.byref(stats))
        _lib.check_mapped(rc)
        self._adopt(ctx, h, stats, m, d, p, (t_host0, t_host1))


class KoopmanKernelRegressor(KoopmanRegressor):
    """regressors.py:58-111: the exact (non-Nystrom) kernel estimator, lifted dimension N = #samples.  Used by the
    reference only as the accuracy comparator of benchmark_lqr_hjb.py:334-381 (N ~ 4000).  Composed on the host from
    the library's device building blocks (nk_kernel_matrix, nk_sqrtm_spd, nk_solve_spd, nk_gemm): every O(N^2 d) and
    O(N^3) step runs on the GPU; the reference's pinv(sqrtm(K)) is the inverse square root the Newton-Schulz
    iteration returns directly.
    """

    def __init__(self, n_inputs, kernel=None, gamma=None):
        super().__init__(n_inputs, gamma)
        self.kernel = kernel
        self.training_inputs = None
        self.training_outputs = None
        self.jitter = 1e-6

    @staticmethod
    def _gemm(ctx, A, B):
        A = np.ascontiguousarray(A, dtype=np.float64)
        B = np.ascontiguousarray(B, dtype=np.float64)
        out = np.empty((A.shape[0], B.shape[1]))
        _lib.check(ctx.lib.nk_gemm(ctx.handle, 0, 0, A.shape[0], B.shape[1], A.shape[1], 1.0, A.ctypes.data, A.shape[1],
                                   B.ctypes.data, B.shape[1], 0.0, out.ctypes.data, out.shape[1]))
        return out

    @staticmethod
    def _solve_spd(ctx, P, R):
        P = np.ascontiguousarray(P, dtype=np.float64)
        R = np.ascontiguousarray(R, dtype=np.float64)
        X = np.empty_like(R)
        rc = ctx.lib.nk_solve_spd(ctx.handle, P.ctypes.data, P.shape[1], P.shape[0], R.ctypes.data, R.shape[1],
                                  R.shape[1], X.ctypes.data, X.shape[1])
        if rc == -3:
            raise np.linalg.LinAlgError(ctx.lib.nk_last_error().decode())
        _lib.check(rc)
        return X

    # ---- device-resident composition: every N x N intermediate lives in HBM (torch tensors as the allocator), only the
    #      attributes the reference exposes are copied to the host, once, at the end.  At config 2's N = 1e4 an N x N matrix
    #      is 800 MB: the host-composed version below moves sixteen of them over PCIe.
    @staticmethod
    def _dgemm(ctx, A, B, out, tA=0, tB=0, beta=0.0):
        a, b, o = _lib.Mat(A), _lib.Mat(B), _lib.Mat(out)
        M, K = (a.shape[1], a.shape[0]) if tA else a.shape
        N = b.shape[0] if tB else b.shape[1]
        ctx.wait_for(A, B, out)
        _lib.check(ctx.lib.nk_gemm(ctx.handle, int(tA), int(tB), M, N, K, 1.0, a.ptr, a.ld, b.ptr, b.ld, float(beta), o.ptr, o.ld))
        return out

    @staticmethod
    def _dsolve(ctx, P, R, out):
        pm, rm, om = _lib.Mat(P), _lib.Mat(R), _lib.Mat(out)
        ctx.wait_for(P, R, out)
        rc = ctx.lib.nk_solve_spd(ctx.handle, pm.ptr, pm.ld, pm.shape[0], rm.ptr, rm.ld, rm.shape[1], om.ptr, om.ld)
        if rc == -3:
            raise np.linalg.LinAlgError(ctx.lib.nk_last_error().decode())
        _lib.check(rc)
        return out

    def _fit_device(self, ctx, torch, Xs, Us, Ys, N, gamma_n):
        dev = torch.device("cuda", ctx.device)
        f64 = torch.float64
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        new = lambda r, c: torch.empty((r, c), dtype=f64, device=dev)
        k = self.kernel.kernel
        p = Us.shape[1]
        Xs_d, Ys_d = up(Xs), up(Ys)
        Us_d = up(Us) if p > 0 else None
        K_ins = k(Xs_d, Xs_d, out=new(N, N))  # :82-84
        if p > 0:
            self._dgemm(ctx, Us_d, Us_d, K_ins, tB=1, beta=1.0)
        K_ins.diagonal().add_(gamma_n)
        Kout = k(Ys_d, Ys_d, out=new(N, N))  # :85
        Kout.diagonal().add_(self.jitter)
        S, Sinv = new(N, N), new(N, N)
        it, res = C.c_int32(), C.c_double()
        ctx.wait_for(Kout)
        _lib.check(ctx.lib.nk_sqrtm_spd(ctx.handle, Kout.data_ptr(), N, N, S.data_ptr(), Sinv.data_ptr(), C.byref(it),
                                        C.byref(res)))  # :87-88 (sqrtm, pinv)
        Kxy = k(Xs_d, Ys_d, out=new(N, N))  # :90
        right = new(N, N + p)  # :91-92: [(Sinv Kxy^T)^T | U]
        self._dgemm(ctx, Kxy, Sinv, right[:, :N], tB=1)
        if p > 0:
            right[:, N:] = Us_d
        del Kxy
        sol = self._dsolve(ctx, K_ins, right, new(N, N + p))
        del right, K_ins
        G_ls = self._dgemm(ctx, S, sol, new(N, N + p))  # :93
        del sol
        Phi = self._dgemm(ctx, Kout, Sinv, new(N, N), tA=1, tB=1)  # :98 Phi = (Sinv Kout)^T
        PPt = self._dgemm(ctx, Phi, Phi, new(N, N), tB=1)
        PPt.diagonal().add_(gamma_n)
        sol2 = self._dsolve(ctx, PPt, Phi, new(N, N))
        del PPt, Phi
        Yt_d = up(self.training_outputs)  # d x N
        Cd = self._dgemm(ctx, Yt_d, sol2, new(Yt_d.shape[0], N))  # :99
        del sol2
        Wd = self._dgemm(ctx, Cd, G_ls, new(Cd.shape[0], N + p))  # :100-102
        torch.cuda.synchronize(dev)
        G_host = G_ls.cpu().numpy()
        self.A = G_host[:, :N]
        self.B = G_host[:, N:]
        self.C = Cd.cpu().numpy()
        self.weights = Wd.cpu().numpy()
        self.Kout = Kout.cpu().numpy()
        self.Kout_sqrt_inv = Sinv.cpu().numpy()
        # lift() multiplies from HBM; solve_lqr(device=True) reads the operators there
        self._dev_cache = dict(Sinv=Sinv, Ys=Ys_d, G_ls=G_ls, Cd=Cd, device=ctx.device)

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_dev_cache", None)  # device tensors never travel
        return state

    def fit(self, X, Y):
        ctx = _lib.get_context()
        X = np.asarray(X, dtype=np.float64).T  # (d+p) x N, as regressors.py:67-68
        Y = np.asarray(Y, dtype=np.float64).T
        n_states = X.shape[0] - self.n_inputs
        N = X.shape[1]
        gamma_n = self.gamma * N
        if self.training_inputs is None:
            self.training_inputs = X
        if self.training_outputs is None:
            self.training_outputs = Y
        k = self.kernel.kernel
        Xs = np.ascontiguousarray(self.training_inputs[:n_states, :].T)
        Us = np.ascontiguousarray(self.training_inputs[n_states:, :].T)  # N x p
        Ys = np.ascontiguousarray(self.training_outputs.T)
        self.__dict__.pop("_dev_cache", None)
        torch = _lib.torch_if_cuda()
        if torch is not None and os.environ.get("NYSKOOP_EXACT_HOST", "0") != "1":
            return self._fit_device(ctx, torch, Xs, Us, Ys, N, gamma_n)
        K_ins = k(Xs, Xs) + self._gemm(ctx, Us, Us.T) + gamma_n * np.eye(N)  # :82-84
        Kout = k(Ys, Ys) + self.jitter * np.eye(N)  # :85
        self.Kout = Kout
        S, Sinv = np.empty((N, N)), np.empty((N, N))
        it, res = C.c_int32(), C.c_double()
        _lib.check(ctx.lib.nk_sqrtm_spd(ctx.handle, Kout.ctypes.data, N, N, S.ctypes.data, Sinv.ctypes.data,
                                        C.byref(it), C.byref(res)))  # :87-88 (sqrtm, pinv)
        self.Kout_sqrt_inv = Sinv
        Kins_x_outs = k(Xs, Ys)  # :90
        right_state = self._gemm(ctx, Sinv, Kins_x_outs.T).T  # :91
        right = np.hstack((right_state, Us))  # :92
        G_ls = self._gemm(ctx, S, self._solve_spd(ctx, K_ins, right))  # :93
        self.A = G_ls[:, :N]
        self.B = G_ls[:, N:]
        # :98-99 -- Phi = (S^-1 Kout)^T; C = Y (Phi Phi^T + gamma_n I)^-1 Phi
        Phi = self._gemm(ctx, Sinv, Kout).T
        PPt = self._gemm(ctx, Phi, Phi.T) + gamma_n * np.eye(N)
        self.C = self._gemm(ctx, self.training_outputs, self._solve_spd(ctx, PPt, Phi))
        self.weights = self._gemm(ctx, self.C, G_ls)  # :100-102

    def lift(self, X):
        """regressors.py:104-111."""
        ctx = _lib.get_context()
        Xq = np.ascontiguousarray(np.asarray(X, dtype=np.float64).T)
        cache = self.__dict__.get("_dev_cache")
        if cache is not None and cache["device"] == ctx.device:
            import torch
            Sinv, Ys_d = cache["Sinv"], cache["Ys"]
            Xq_d = torch.from_numpy(Xq).to(Ys_d.device)
            Kt = self.kernel.kernel(Ys_d, Xq_d, out=torch.empty((Ys_d.shape[0], Xq.shape[0]), dtype=torch.float64, device=Ys_d.device))
            out = self._dgemm(ctx, Sinv, Kt, torch.empty_like(Kt))
            return out.cpu().numpy()
        Kout_test = self.kernel.kernel(np.ascontiguousarray(self.training_outputs.T), Xq)
        return self._gemm(ctx, self.Kout_sqrt_inv, Kout_test)

    def solve_lqr(self, Q=None, R=None, c=1.0, device=False):
        """The gain of the exact model (benchmark_lqr_hjb.py:356: control.dlqr on the N x N operators): by default
        Q = c * C^T C symmetrised and R = I.  Returns K (p x N).  On the host it is lqr.dlqr (scipy); device=True runs
        the launch-chain Riccati solver (nk_dare_large) on the operators, read from HBM where the fit left them there
        (nothing N x N crosses PCIe again) and from the host attributes after a host-composed fit or un-pickling.
        Raises np.linalg.LinAlgError when the device iteration does not converge or breaks down."""
        p = int(self.n_inputs)
        if not device:
            if Q is None:
                S = self.C.T @ self.C
                Q = c * ((S + S.T) / 2)
            if R is None:
                R = np.eye(p)
            K, _ = dlqr(self.A, self.B, Q, R)
            return K
        ctx = _lib.get_context()
        N = self.A.shape[0]
        if R is None:
            R = np.eye(p)
        cache = self.__dict__.get("_dev_cache")
        if cache is not None and cache["device"] == ctx.device and "G_ls" in cache:
            import torch
            G_ls, Cd = cache["G_ls"], cache["Cd"]
            A_op, B_op = G_ls[:, :N], G_ls[:, N:]
            if Q is None:
                Qd = self._dgemm(ctx, Cd, Cd, torch.empty((N, N), dtype=torch.float64, device=G_ls.device), tA=1)
                Q = (Qd + Qd.T).mul_(0.5 * c)
            torch.cuda.synchronize(G_ls.device)
        else:
            A_op, B_op = np.asarray(self.A), np.asarray(self.B).reshape(N, p)
            if Q is None:
                S = self.C.T @ self.C
                Q = c * ((S + S.T) / 2)
        K, _, status, _, _ = ctx.dare_large(A_op, B_op, Q, R, want_P=False)
        if status != 0:
            raise np.linalg.LinAlgError(f"device Riccati solve failed with status {status} "
                                        "(1: max_iter reached, 2: non-finite values or a singular pivot)")
        return K


class KoopmanSplineRegressor(_DeviceModelRegressor):
    """regressors.py:181-233 (the Korda-Mezic thin-plate-spline baseline), MI355X-native: the two n x m spline blocks, the
    three Gram products, the regularised pseudo-inverse and the operator products run on the device (nk_spline_fit).

    Same constructor, attributes (`centers` d x m, A, B, C, weights) and random draws as the reference: the centres come
    from NumPy's global legacy RNG the first time `lift` needs them (in `fit`: from the training states) and are reused
    by every later fit.  Additive, as for the Nystrom class: `fit` accepts `row_ranges` and device tensors; `rollout`,
    `score_neg_rmse`, `closed_loop` and `solve_lqr` run the callers' loops on the device.  The device-model plumbing
    (asynchronous operator fetch, pickling through host copies, lift / predict / rollout / closed loop) is the base
    class's, shared with the Nystrom estimator."""

    _landmarks_attr = "centers"
    _no_landmarks = "regressor has no centres: call fit (or lift) first"

    def __init__(self, n_inputs, state_bounds_params=None, m=None, gamma=None):
        super().__init__(n_inputs, gamma, m)
        self.state_bounds_params = state_bounds_params
        self.centers = None

    def compute_centers(self, X):
        """regressors.py:187-197, draw for draw: X is d x n (the array `lift` sees first)."""
        if self.state_bounds_params is not None:
            length = np.sqrt(np.random.uniform(0, self.state_bounds_params[0], size=(1, self.m)))
            angle = np.pi * np.random.uniform(0, self.state_bounds_params[1], size=(1, self.m))
            return np.vstack((length * np.cos(angle), length * np.sin(angle)))
        centers_indices = np.random.choice(np.arange(0, X.shape[1]), size=self.m, replace=False)
        if _is_device_tensor(X):
            return np.ascontiguousarray(X[:, centers_indices.tolist()].cpu().numpy())
        return np.asarray(X)[:, centers_indices]

    def _create_model(self, ctx, Z, p, pa, pb, pc, pw):
        m, d = Z.shape  # (an unfitted regressor gets a model that can only lift)
        h = C.c_void_p()
        rc = ctx.lib.nk_spline_model_create(ctx.handle, Z.ctypes.data, d, m, d, p, pa, pb, pc, pw, C.byref(h))
        _lib.check_mapped(rc)
        return h

    def fit(self, X, Y, row_ranges=None, fetch=True):
        """regressors.py:199-221.  X: n x (d+p) rows [state | input], Y: n x d (NumPy arrays or float64 device tensors).
        row_ranges: [begin, end) row pairs of the training rows (default: all).  Returns None, like the reference."""
        ctx = _lib.get_context()
        Xm, Ym = _lib.Mat(X), _lib.Mat(Y)
        n, d = Ym.shape
        p = int(self.n_inputs)
        if Xm.shape != (n, d + p):
            raise ValueError(f"X has shape {Xm.shape}, expected {(n, d + p)}")
        rr, n_rr, keep_rr = self._ranges(row_ranges)
        if self.centers is None:  # regressors.py:207 -> lift(X[:n_states, :]) of the training states
            rows = None if keep_rr is None else np.concatenate(
                [np.arange(b, e) for b, e in keep_rr.reshape(-1, 2) if e > b])
            if _is_device_tensor(X):
                states = X[:, :d] if rows is None else X[rows.tolist(), :d]
                self.centers = self.compute_centers(states.t())
            else:
                states = np.asarray(X)[:, :d] if rows is None else np.asarray(X)[rows, :d]
                self.centers = self.compute_centers(states.T)
        Z = np.ascontiguousarray(np.asarray(self.centers, dtype=np.float64).T)
        if Z.shape[1] != d:
            raise ValueError(f"centres have dimension {Z.shape[1]}, data has {d}")
        m = Z.shape[0]
        stats = _lib.FitStats()
        h = C.c_void_p()
        t_host0 = time.perf_counter()
        self._drop_model()
        t_host1 = time.perf_counter()
        ctx.wait_for(X, Y)
        rc = ctx.lib.nk_spline_fit(ctx.handle, Xm.ptr, Xm.ld, Ym.ptr, Ym.ld, n, d, p, rr, n_rr, Z.ctypes.data, d, m,
                                   float(self.gamma), C.byref(h), C.byref(stats))
        _lib.check_mapped(rc)
        self._adopt(ctx, h, stats, m, d, p, (t_host0, t_host1), fetch)

    def lift(self, X):
        """regressors.py:223-233: X is d x n_q (not augmented); returns phi, m x n_q.  Draws the centres from X when
        there are none yet, as the reference does."""
        if self.centers is None:
            self.centers = self.compute_centers(X)
        return super().lift(X)
