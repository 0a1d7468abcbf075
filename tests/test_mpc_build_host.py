"""CPU: the host side of the device controller build -- the NumPy statements of what the device computes
(lqr.mpc_condense_blocked, lqr.lyap_smith, lqr.dare_newton_smith) against the existing host path, scipy and the np.longdouble
evaluation of tests/mpc_build_reference.py, the two new entry points in the header, the library and the bindings, and the
bookkeeping of harness.lqr_sweep(controller=dict(..., build="device")) with stubs standing in for the fits, the device build
and the device loop."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.linalg

import dare_reference as dr
import mpc_build_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


# ---- the NumPy statements ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,p,N", mr.HOST_SHAPES, ids=str)
def test_blocked_condensing_equals_the_column_form_and_the_extended_evaluation(m, p, N):
    from nys_koop_lqr_amd import lqr
    A, B, Q, R, P, _ = mr.condense_problem(m, p, N, 0)
    Hb, Fb = lqr.mpc_condense_blocked(A, B, Q, R, P, N)
    Hc, Fc = lqr.mpc_condense(A, B, Q, R, P, N)
    H_ld, F_ld = mr.condense_blocked_ld(A, B, Q, R, P, N)
    assert Hb.shape == (N * p, N * p) and Fb.shape == (N * p, m) and np.array_equal(Hb, Hb.T)
    # both float64 forms against the extended one: a sum of at most (N + 1) m + m products per entry, each with a relative
    # rounding of eps, stays far below 64 eps of the largest entry on these operators (measured: <= 2e-15)
    for name, got, ref in (("H blocked", Hb, H_ld), ("F blocked", Fb, F_ld), ("H columns", Hc, H_ld), ("F columns", Fc, F_ld)):
        assert mr.err(got, ref) <= 64 * EPS, (name, mr.err(got, ref))
    assert mr.err(Hb, Hc) <= 64 * EPS and mr.err(Fb, Fc) <= 64 * EPS
    with pytest.raises(ValueError, match="at least 1"):
        lqr.mpc_condense_blocked(A, B, Q, R, P, 0)


def test_extended_output_rows_bound_the_numpy_statement():
    from nys_koop_lqr_amd import lqr
    for m, p, N, nc, Ny in ((5, 1, 1, 1, 1), (17, 3, 5, 2, 3), (65, 2, 8, 1, 8)):
        A, B, _, _, _, Cr = mr.condense_problem(m, p, N, nc)
        G, T = lqr.mpc_condense_outputs(A, B, Cr, N, Ny)
        G_ld, T_ld = mr.condense_outputs_ld(A, B, Cr, N, Ny)
        assert mr.err(G, G_ld) <= 64 * EPS and mr.err(T, T_ld) <= 64 * EPS


@pytest.mark.parametrize("m,rho", [(1, 0.5), (5, 0.9), (17, 0.99), (64, 0.993)])
def test_lyap_smith_against_scipy(m, rho):
    from nys_koop_lqr_amd import lqr
    rng = np.random.default_rng(m)
    Ac = rng.standard_normal((m, m))
    Ac *= rho / np.abs(np.linalg.eigvals(Ac)).max()
    X0 = rng.standard_normal((m, m))
    X0 = X0 @ X0.T
    X, it, status = lqr.lyap_smith(Ac, X0)
    ref = scipy.linalg.solve_discrete_lyapunov(Ac.T, X0)

    def resid(Y):
        return np.linalg.norm(Ac.T @ Y @ Ac - Y + X0) / np.linalg.norm(Y)

    assert status == 0 and 1 <= it <= 60 and np.array_equal(X, X.T)
    # the residual of the iteration is held against scipy's own, with the rounding of evaluating it as the floor
    assert resid(X) <= max(10 * resid(ref), 64 * m * EPS), (resid(X), resid(ref))
    assert lqr.lyap_smith(Ac, X0, max_iter=1)[2] == 3
    assert lqr.lyap_smith(1.5 * np.eye(2), np.eye(2), max_iter=2000)[2] == 2  # diverges to inf: non-finite
    assert lqr.lyap_smith(np.zeros((3, 3)), np.eye(3))[1:] == (1, 0)


@pytest.mark.parametrize("name,c", dr.HOST_CASES, ids=lambda v: str(v))
def test_newton_smith_is_no_worse_than_dare_refine(name, c):
    """One correction step from the doubling iteration's (K, P), what the device runs, against the host path (scipy and two
    steps of dare_refine): the Riccati residual is not larger, on every fixture and both cost weights.  Measured: 1.8e-16 ..
    1.0e-15 against 2.0e-16 .. 1.8e-14.  (The same step as a full solve from P = 0 does not hold this bar on the fixtures with
    a closed-loop radius above 0.9995: f12_m48 2.8e-13, f15_m48 9.3e-14, f15_m200 6.0e-14, f12_m200 5.1e-15, f1_illcond
    4.0e-15 .. 4.8e-15 against 2.0e-15 .. 3.9e-15 of dare_refine -- the rounding of the squarings is relative to what the Smith
    iteration carries, which is why the step is stated as a correction.)"""
    from nys_koop_lqr_amd import lqr
    A, B, Q, R = dr.fixture_problem(name, c)
    P0, K0, _, st = lqr.dare_doubling(A, B, Q, R)
    assert st == 0
    K, P, it, status = lqr.dare_newton_smith(A, B, Q, R, K0, steps=1, P=P0)
    assert status == 0 and it >= 1
    Kr, Pr = lqr.dare_refine(A, B, Q, R, lqr.dlqr(A, B, Q, R)[0])
    r, r_ref = dr.residual(A, B, Q, P, K), dr.residual(A, B, Q, Pr, Kr)
    assert r <= r_ref, (name, c, r, r_ref)


def test_newton_smith_from_zero_is_the_full_lyapunov_solve():
    """P = None: the first step solves X = Ac'X Ac + Q + K'RK itself (the correction of zero)."""
    from nys_koop_lqr_amd import lqr
    A, B, Q, R = dr.random_problem(17, 3, 1.1, seed=17)
    K0 = lqr.dare_doubling(A, B, Q, R)[1]
    K, P, it, status = lqr.dare_newton_smith(A, B, Q, R, K0, steps=1)
    Ac = A - B @ K0
    X = scipy.linalg.solve_discrete_lyapunov(Ac.T, Q + K0.T @ R @ K0)
    assert status == 0 and np.linalg.norm(P - X) <= 64 * 17 * EPS * np.linalg.norm(X) / (1 - np.abs(np.linalg.eigvals(Ac)).max())


def test_newton_smith_reports_its_failures():
    from nys_koop_lqr_amd import lqr
    A, B, Q, R = dr.random_problem(5, 1, 1.1, seed=5)
    K0 = lqr.dare_doubling(A, B, Q, R)[1]
    K, P, it, status = lqr.dare_newton_smith(A, B, Q, R, K0, max_iter=1)
    assert status == 3 and it == 1 and np.all(np.isnan(K)) and np.all(np.isnan(P))
    K, P, it, status = lqr.dare_newton_smith(A, B, Q, R, np.zeros_like(K0), max_iter=2000)  # A itself is unstable
    assert status == 2 and np.all(np.isnan(K))
    K, P, it, status = lqr.dare_newton_smith(A, B, Q, R, K0, steps=0)
    assert status == 0 and it == 0 and P is None and np.array_equal(K, K0)
    P0 = lqr.dare_doubling(A, B, Q, R)[0]
    assert lqr.dare_newton_smith(A, B, Q, R, K0, steps=0, P=P0)[1] is P0


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_the_build_entries_are_declared_exported_and_mirrored():
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from nys_koop_lqr_amd import _lib
    lib = _lib.load_library()
    header = open(os.path.join(ROOT, "include", "nyskoop.h")).read()
    declared = set(re.findall(r"\b(nk_[a-z_0-9]+)\s*\(", header))
    for name in ("nk_mpc_build_batch", "nk_model_mpc_build_batch"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    for struct, cls in (("nk_mpc_build_problem", _lib.MpcBuildProblem), ("nk_mpc_build_spec", _lib.MpcBuildSpec),
                        ("nk_mpc_build_out", _lib.MpcBuildOut)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f for decl in body.split(";") for f in re.findall(r"\*?\s*(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
        assert [f[0] for f in cls._fields_] == fields, (struct, fields)
    assert C.sizeof(_lib.MpcBuildProblem) == 24 + 6 * 16 + 6 * 8 and C.sizeof(_lib.MpcBuildSpec) == 32
    assert C.sizeof(_lib.MpcBuildOut) == 40
    assert len(_lib.SIGNATURES["nk_mpc_build_batch"][1]) == 10 and len(_lib.SIGNATURES["nk_model_mpc_build_batch"][1]) == 14


# ---- the sweep's bookkeeping ------------------------------------------------------------------------------------------------
def _stubs(fail_status=None):
    """Stand-ins: a 'fit' tagged with its unit, a device 'build' that returns a controller tagged like its regressor (a
    non-zero status for the chosen unit) and records what it was handed, and an MPC 'loop' that scores a unit by its tag."""
    calls = []

    def fit_fn(X, Y, n_inputs, params, unit, estimator):
        if unit["si"] == 2 and unit["k"] == 1:
            return None  # a failed fit: not part of the build call
        tag = 10.0 * unit["si"] + unit["k"] + 1.0

        def solve_mpc(*a, **kw):
            raise AssertionError("build='device' must not call reg.solve_mpc")

        return SimpleNamespace(A=np.full((2, 2), tag), B=np.ones((2, 1)), C=np.ones((1, 2)), tag=tag, solve_mpc=solve_mpc)

    def build_fn(regs, c, controller):
        calls.append(("build", [r.tag for r in regs], c, dict(controller)))
        status = np.array([fail_status[1] if fail_status and r.tag == fail_status[0] else 0 for r in regs], dtype=np.int32)
        return [SimpleNamespace(tag=r.tag) if st == 0 else None for r, st in zip(regs, status)], status

    def loop_fn(regs, ctls, x0, x_ref, num_steps, plant, iters=50, tol=0.0, u_opt=None, return_trajectories=False):
        calls.append(("mpc", [r.tag for r in regs]))
        tags = np.array([r.tag for r in regs])
        assert [c.tag for c in ctls] == list(tags)
        return dict(sse_u=tags, ss_opt=4.0 * tags, J=tags + 0.5, u_absmax=-tags, iters_sum=2.0 * tags, r_max=0.25 * tags,
                    n_at_limit=3.0 * tags, n_iterated=tags - 1.0)

    return fit_fn, build_fn, loop_fn, calls


ARGS = (np.zeros((50, 3)), np.zeros((50, 2)), 1, dict(kernel=None, gamma=1e-6), [4, 6], [0, 1, 2], None, np.zeros(2), np.zeros(2), 5)
BOX = dict(horizon=8, u_min=-0.5, u_max=0.5, du_max=0.1, iters=30, tol=1e-6, build="device")


def test_build_device_is_one_call_over_the_fitted_units():
    from nys_koop_lqr_amd import harness
    assert harness.CONTROLLER_KEYS[-5] == "build" and harness.lqr_controller_spec(dict(horizon=4))["build"] == "host"
    fit_fn, build_fn, loop_fn, calls = _stubs()
    full = harness.lqr_sweep(*ARGS, c=2.0, fit_fn=fit_fn, loop_fn=loop_fn, controller=BOX, controller_batch_fn=build_fn)
    assert [c[0] for c in calls] == ["build", "mpc"]
    kind, tags, c, spec = calls[0]
    assert tags == [1.0, 11.0, 21.0, 2.0, 12.0] and c == 2.0  # exactly the fitted units, in plan order
    assert spec["horizon"] == 8 and spec["build"] == "device" and spec["u_max"] == 0.5 and spec["rho"] is None
    assert calls[1][1] == tags
    assert sorted(full["timing"]) == ["fit_s", "gain_cpu_s", "gain_wait_s", "loop_s", "total_s"]
    assert full["timing"]["gain_cpu_s"] == 0.0 and full["timing"]["gain_wait_s"] >= 0.0
    assert np.isnan(full["J"][2, 1]) and np.sum(np.isnan(full["J"])) == 1
    # a non-zero status: a NaN row, not run, the others as in the full run
    for st in (1, 2, 3):
        fit_fn, build_fn, loop_fn, calls = _stubs(fail_status=(11.0, st))
        part = harness.lqr_sweep(*ARGS, c=2.0, fit_fn=fit_fn, loop_fn=loop_fn, controller=BOX, controller_batch_fn=build_fn)
        assert calls[1] == ("mpc", [1.0, 21.0, 2.0, 12.0])
        hole = np.zeros((3, 2), dtype=bool)
        hole[1, 0] = hole[2, 1] = True
        for name in harness.MPC_SCORE_NAMES + ("rmse_control",):
            assert np.all(np.isnan(part[name][hole])) and np.array_equal(part[name][~hole], full[name][~hole]), name
        assert sorted(part["timing"]) == sorted(full["timing"])


def test_build_values_and_the_device_gain_are_checked():
    from nys_koop_lqr_amd import dist, harness
    fit_fn, build_fn, loop_fn, calls = _stubs()
    with pytest.raises(ValueError, match="'gpu'"):
        harness.lqr_sweep(*ARGS, fit_fn=fit_fn, loop_fn=loop_fn, controller=dict(BOX, build="gpu"), controller_batch_fn=build_fn)
    with pytest.raises(ValueError, match="host Riccati"):
        harness.lqr_sweep(*ARGS, fit_fn=fit_fn, loop_fn=loop_fn, controller=BOX, gain="device", controller_batch_fn=build_fn)
    with pytest.raises(ValueError, match="host Riccati"):
        harness.lqr_sweep(*ARGS, fit_fn=fit_fn, loop_fn=loop_fn, controller=dict(BOX, build="host"), gain="device")
    assert calls == []
    sh = dist.sharded_lqr_sweep(*ARGS, c=2.0, fit_fn=fit_fn, loop_fn=loop_fn, controller=BOX, controller_batch_fn=build_fn)
    plain = harness.lqr_sweep(*ARGS, c=2.0, fit_fn=fit_fn, loop_fn=loop_fn, controller=BOX, controller_batch_fn=build_fn)
    assert [c[0] for c in calls] == ["build", "mpc", "build", "mpc"] and calls[0][1] == calls[2][1]
    for name in harness.MPC_SCORE_NAMES + ("rmse_control",):
        assert np.array_equal(sh[name], plain[name], equal_nan=True), name


def test_the_default_build_batch_drops_units_whose_limits_are_refused(monkeypatch):
    """regressors._mpc_controller_batch with the device call replaced: a unit whose limits solve_mpc refuses is not part of
    the call and has no controller; the others get what reg.solve_mpc(device=True) would assemble."""
    from nys_koop_lqr_amd import lqr, regressors
    seen = []

    def fake_build(regs, c, R, specs, **solver):
        seen.append(([r.tag for r in regs], c, R, [(N, list(comps), Ny) for N, comps, Ny in specs]))
        units = []
        for r, (N, comps, Ny) in zip(regs, specs):
            H = np.eye(N) * (2.0 + r.tag)
            u = dict(H=H, F=np.ones((N, 3)), K=np.ones((1, 3)), G=None, T=None)
            if len(comps):
                u["G"], u["T"] = np.ones((Ny * len(comps), N)), np.ones((Ny * len(comps), 3))
            units.append(u)
        return units, np.array([0, 2][:len(regs)] + [0] * max(len(regs) - 2, 0), dtype=np.int32), None

    monkeypatch.setattr(regressors, "_mpc_build_batch", fake_build)
    regs = [SimpleNamespace(tag=float(i), n_inputs=1, _landmark_shape=lambda d=d: (d, 3)) for i, d in enumerate((2, 2, 2, 6))]
    spec = dict(horizon=4, u_min=-1.0, u_max=1.0, du_min=None, du_max=None, rho=None, x_min=None, x_max=0.5, y_horizon=2,
                y_weight=7.0)
    ctrls, status = regressors._mpc_controller_batch(regs, 1.5, spec)
    assert seen == [([0.0, 1.0, 2.0], 1.5, None, [(4, [0, 1], 2)] * 3)]  # six bounded components: refused, not in the call
    assert list(status) == [0, 2, 0, -1] and ctrls[1] is None and ctrls[3] is None
    for i in (0, 2):
        ctl = ctrls[i]
        assert isinstance(ctl, lqr.MPCOutputController) and ctl.rho == 2.0 + i and ctl.y_weight == 7.0
        assert np.array_equal(ctl.ycomp, [0, 1, 0, 1]) and np.array_equal(ctl.yhi, np.full(4, 0.5)) and np.all(ctl.ylo == -np.inf)
        assert np.array_equal(ctl.hi, np.ones(4)) and np.all(ctl.dlo == -np.inf)
