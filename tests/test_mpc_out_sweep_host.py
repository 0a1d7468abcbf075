"""CPU: the host side of the one-call MPC sweep under state limits -- the C-ABI declares and exports nk_mpc_out_loop_multi,
harness.mpc_out_scores states the two new scores on hand-made arrays, the controller dict of harness.lqr_sweep knows the
state-limit keys, and the bookkeeping of lqr_run_units / lqr_sweep carries ten scores with stubs standing in for the fits,
the controllers and the device loop."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from nys_koop_lqr_amd import _lib
    return _lib.load_library()


def test_mpc_out_multi_declared_exported_and_mirrored(lib):
    from nys_koop_lqr_amd import _lib, harness
    header = open(os.path.join(ROOT, "include", "nyskoop.h")).read()
    declared = set(re.findall(r"\b(nk_[a-z_0-9]+)\s*\(", header))
    assert "nk_mpc_out_loop_multi" in declared and "nk_mpc_out_loop_multi" in _lib.SIGNATURES
    assert hasattr(lib, "nk_mpc_out_loop_multi")
    assert re.search(r"#define\s+NK_MPC_OUT_N_SCORES\s+10\b", header)
    assert _lib.MPC_OUT_N_SCORES == 10 == len(harness.MPC_OUT_SCORE_NAMES)
    assert harness.MPC_OUT_SCORE_NAMES == harness.MPC_SCORE_NAMES + ("y_viol_max", "n_y_viol")
    assert re.search(r"#define\s+NK_ABI_VERSION\s+2\b", header) and lib.nk_version() == 2  # symbols added, nothing changed
    # the prototype: ctx, plant, steps, units, outs, n_units, u_opt, n_uopt, out_x, out_u, out_info, scores
    proto = re.search(r"int nk_mpc_out_loop_multi\((.*?)\);", header, re.S).group(1)
    names = [re.findall(r"(\w+)$", a.strip())[0] for a in proto.split(",")]
    assert names == ["ctx", "plant", "steps", "units", "outs", "n_units", "u_opt", "n_uopt", "out_x", "out_u", "out_info", "scores"]
    res, args = _lib.SIGNATURES["nk_mpc_out_loop_multi"]
    assert res is C.c_int and len(args) == 12 and args[3] is C.POINTER(_lib.MpcUnit) and args[2] is C.c_int32
    assert args[4] is C.POINTER(C.POINTER(_lib.MpcOut)) and args[5] is C.c_int32
    # the multi form without rows and the single calls keep their prototypes
    assert len(_lib.SIGNATURES["nk_mpc_loop_multi"][1]) == 11 and len(_lib.SIGNATURES["nk_mpc_out_loop"][1]) == 13


def _ctl(ylo, yhi, ycomp, p=1):
    inf = np.full(p, INF)
    return SimpleNamespace(lo=-inf, hi=inf, dlo=-inf, dhi=inf, ylo=np.array(ylo, dtype=np.float64),
                           yhi=np.array(yhi, dtype=np.float64), ycomp=np.array(ycomp, dtype=np.int32))


def test_mpc_out_scores_on_hand_made_arrays():
    """Two states, four steps.  Row 0 bounds x_2 in [-0.5, 0.25], row 1 bounds x_1 in [-inf, 0.75], row 2 has ycomp = -1 and
    bounds nothing could meet: ignored.  x0 itself is outside and does not count: the steps score x_{t+1}."""
    from nys_koop_lqr_amd import harness
    ctl = _ctl([-0.5, -INF, 5.0], [0.25, 0.75, -5.0], [1, 0, -1])
    #             x0    t=0    t=1     t=2   t=3
    xs = np.array([[9.0, 0.5, 0.875, 0.75, 0.0],      # x_1: above 0.75 by 0.125 after t = 1
                   [9.0, 0.0, -0.75, 0.375, 0.25]])   # x_2: below -0.5 by 0.25 after t = 1, above 0.25 by 0.125 after t = 2
    us, info = np.zeros((1, 4)), np.zeros((4, 2))
    sc = harness.mpc_out_scores(xs, us, info, ctl)
    assert sc["y_viol_max"] == 0.25 and sc["n_y_viol"] == 2.0
    base = harness.mpc_scores(xs, us, info, ctl)
    assert all(sc[k] == base[k] for k in harness.MPC_SCORE_NAMES) and set(sc) == set(base) | {"y_viol_max", "n_y_viol"}
    assert list(sc)[-2:] == ["y_viol_max", "n_y_viol"]
    # each sign alone
    assert harness.mpc_out_scores(xs, us, info, _ctl([-0.5], [INF], [1]))["y_viol_max"] == 0.25
    up = harness.mpc_out_scores(xs, us, info, _ctl([-INF], [0.25], [1]))
    assert up["y_viol_max"] == 0.125 and up["n_y_viol"] == 1.0
    # nothing violated: exactly 0 and 0; a bound met exactly is no violation
    none = harness.mpc_out_scores(xs, us, info, _ctl([-0.75], [0.375], [1]))
    assert none["y_viol_max"] == 0.0 and none["n_y_viol"] == 0.0
    # only rows without a component, and a controller without rows at all
    for c in (_ctl([5.0], [-5.0], [-1]), SimpleNamespace(lo=ctl.lo, hi=ctl.hi, dlo=ctl.dlo, dhi=ctl.dhi)):
        z = harness.mpc_out_scores(xs, us, info, c)
        assert z["y_viol_max"] == 0.0 and z["n_y_viol"] == 0.0
    # one rounded subtraction on the absolute bound: 0.1 + 0.2 - 0.3 is 2^-54 in double
    tiny = harness.mpc_out_scores(np.array([[0.0, 0.1 + 0.2]]), np.zeros((1, 1)), np.zeros((1, 2)), _ctl([-INF], [0.3], [0]))
    assert tiny["y_viol_max"] == (0.1 + 0.2) - 0.3 > 0 and tiny["n_y_viol"] == 1.0


def test_mpc_out_scores_nan_rule():
    """A NaN state enters y_viol_max once and stays, whatever follows, and its step is not counted; inf - inf of an infinite
    state at an infinite bound is such a NaN too; controls (states, p) are accepted as mpc_scores accepts them."""
    from nys_koop_lqr_amd import harness
    ctl = _ctl([-0.5], [0.25], [1])
    xs = np.array([[0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.5, np.nan, 9.0, 0.0]])
    sc = harness.mpc_out_scores(xs, np.zeros((4, 1)), np.zeros((4, 2)), ctl)
    assert np.isnan(sc["y_viol_max"]) and sc["n_y_viol"] == 2.0  # t = 0 (0.25 above) and t = 2 (8.75 above)
    xs2 = np.array([[0.0, 0.0, 0.0], [0.0, np.inf, 0.0]])
    sc2 = harness.mpc_out_scores(xs2, np.zeros((1, 2)), np.zeros((2, 2)), _ctl([-0.5], [INF], [1]))
    assert np.isnan(sc2["y_viol_max"]) and sc2["n_y_viol"] == 0.0
    # a NaN in a component no row names changes nothing
    xs3 = np.array([[0.0, np.nan, 0.0], [0.0, 0.5, 0.0]])
    sc3 = harness.mpc_out_scores(xs3, np.zeros((1, 2)), np.zeros((2, 2)), ctl)
    assert sc3["y_viol_max"] == 0.25 and sc3["n_y_viol"] == 1.0


def test_controller_spec_knows_the_state_limits():
    from nys_koop_lqr_amd import harness
    assert harness.CONTROLLER_KEYS[-4:] == ("x_min", "x_max", "y_horizon", "y_weight")
    spec = harness.lqr_controller_spec(dict(horizon=8, x_max=[INF, 0.5], y_weight=40.0))
    assert spec["x_min"] is None and spec["x_max"] == [INF, 0.5] and spec["y_horizon"] is None and spec["y_weight"] == 40.0
    assert spec["iters"] == 50 and spec["rho"] is None
    assert harness.lqr_controller_spec(dict(horizon=8))["y_weight"] == INF
    assert harness.lqr_controller_has_rows(spec)
    assert not harness.lqr_controller_has_rows(harness.lqr_controller_spec(dict(horizon=8, u_max=1.0)))
    assert not harness.lqr_controller_has_rows(harness.lqr_controller_spec(dict(horizon=8, x_max=[INF, INF])))
    assert not harness.lqr_controller_has_rows(harness.lqr_controller_spec(dict(horizon=8, x_max=0.5, iters=0)))
    assert not harness.lqr_controller_has_rows(None)
    with pytest.raises(ValueError, match="x_limit"):
        harness.lqr_controller_spec(dict(horizon=8, x_limit=0.5))


def _stubs(fail=None):
    """Stand-ins: a 'fit' whose solve_mpc returns a controller tagged with its unit and the arguments it was built from
    (raising for the chosen unit), and an MPC 'loop' that returns ten scores per unit."""
    calls = []

    def fit_fn(X, Y, n_inputs, params, unit, estimator):
        tag = 10.0 * unit["si"] + unit["k"] + 1.0

        def solve_mpc(horizon, c=1.0, **kw):
            if fail is not None and (unit["si"], unit["k"]) == fail:
                raise np.linalg.LinAlgError("no stabilising solution")
            return SimpleNamespace(tag=tag, horizon=horizon, c=c, kw=kw)

        return SimpleNamespace(A=np.full((2, 2), tag), B=np.ones((2, 1)), C=np.ones((1, 2)), tag=tag, solve_mpc=solve_mpc)

    def loop_fn(regs, ctls, x0, x_ref, num_steps, plant, iters=50, tol=0.0, u_opt=None, return_trajectories=False):
        calls.append(([r.tag for r in regs], [c.kw for c in ctls], iters, tol))
        tags = np.array([r.tag for r in regs])
        out = dict(sse_u=tags, ss_opt=4.0 * tags, J=tags + 0.5, u_absmax=-tags, iters_sum=2.0 * tags, r_max=0.25 * tags,
                   n_at_limit=3.0 * tags, n_iterated=tags - 1.0, y_viol_max=0.125 * tags, n_y_viol=tags + 2.0)
        if return_trajectories:
            out["states"] = np.tile(tags[:, None, None], (1, num_steps + 1, 2))
            out["controls"] = np.tile(tags[:, None, None], (1, num_steps, 1))
        return out

    return fit_fn, loop_fn, calls


ARGS = (np.zeros((50, 3)), np.zeros((50, 2)), 1, dict(kernel=None, gamma=1e-6), [4, 6], [0, 1, 2], None, np.zeros(2), np.zeros(2), 5)
LIMITED = dict(horizon=8, u_min=-2.0, u_max=2.0, x_min=[-INF, -0.5], x_max=[INF, 0.5], y_horizon=4, y_weight=40.0, rho=7.0,
               iters=30, tol=1e-6)


def test_sweep_under_state_limits_carries_ten_scores_and_nan_fills_dead_units():
    from nys_koop_lqr_amd import harness
    fit_fn, loop_fn, calls = _stubs()
    full = harness.lqr_sweep(*ARGS, c=2.0, fit_fn=fit_fn, loop_fn=loop_fn, return_trajectories=True, controller=LIMITED)
    assert len(calls) == 1  # ONE loop call, every unit, in plan (m-major) order
    tags_seen, kws, iters, tol = calls[0]
    assert tags_seen == [1.0, 11.0, 21.0, 2.0, 12.0, 22.0] and (iters, tol) == (30, 1e-6)
    want = dict(u_min=-2.0, u_max=2.0, du_min=None, du_max=None, rho=7.0, x_min=[-INF, -0.5], x_max=[INF, 0.5], y_horizon=4,
                y_weight=40.0)
    assert all(kw == want for kw in kws)  # the state limits reach reg.solve_mpc
    tags = np.array([[1.0, 2.0], [11.0, 12.0], [21.0, 22.0]])
    assert np.array_equal(full["y_viol_max"], 0.125 * tags) and np.array_equal(full["n_y_viol"], tags + 2.0)
    assert np.array_equal(full["J"], tags + 0.5) and np.array_equal(full["n_iterated"], tags - 1.0)
    assert np.array_equal(full["rmse_control"], np.full((3, 2), 50.0))
    assert full["states"].shape == (3, 2, 6, 2) and full["controls"].shape == (3, 2, 5, 1)
    fit_fn, loop_fn, calls = _stubs(fail=(1, 1))
    part = harness.lqr_sweep(*ARGS, c=2.0, fit_fn=fit_fn, loop_fn=loop_fn, return_trajectories=True, controller=LIMITED)
    assert [c[0] for c in calls] == [[1.0, 11.0, 21.0, 2.0, 22.0]]  # the unit without a controller is not submitted
    hole = np.zeros((3, 2), dtype=bool)
    hole[1, 1] = True
    for name in harness.MPC_OUT_SCORE_NAMES + ("rmse_control",):
        assert np.all(np.isnan(part[name][hole])) and np.array_equal(part[name][~hole], full[name][~hole]), name
    assert np.all(np.isnan(part["states"][1, 1])) and np.all(np.isnan(part["controls"][1, 1]))


def test_run_units_and_result_by_width():
    """lqr_run_units returns (n_units, 10) under state limits and (n_units, 8) without them from the same stand-ins (which
    offer ten); lqr_result names the tables by the width it is given; every controller failing gives all-NaN tables of all ten."""
    from nys_koop_lqr_amd import harness
    fit_fn, loop_fn, calls = _stubs()
    units = harness.lqr_plan(*ARGS[:6], "nystrom")
    sc10 = harness.lqr_run_units(*ARGS[:4], units, *ARGS[6:], fit_fn=fit_fn, loop_fn=loop_fn, controller=LIMITED)[0]
    sc8 = harness.lqr_run_units(*ARGS[:4], units, *ARGS[6:], fit_fn=fit_fn, loop_fn=loop_fn,
                                controller=dict(horizon=8, u_max=2.0))[0]
    assert sc10.shape == (6, 10) and sc8.shape == (6, 8) and np.array_equal(sc10[:, :8], sc8)
    assert "x_min" not in calls[1][1][0]  # without state limits solve_mpc is called as it always was
    r10, r8 = harness.lqr_result(units, sc10, None, None, 3, 2), harness.lqr_result(units, sc8, None, None, 3, 2)
    assert "y_viol_max" in r10 and "n_y_viol" in r10 and "y_viol_max" not in r8 and "n_iterated" in r8

    def broken(*a):
        reg = fit_fn(*a)
        reg.solve_mpc = lambda *b, **kw: (_ for _ in ()).throw(ValueError("x_min <= x_max"))
        return reg

    calls.clear()
    none = harness.lqr_sweep(*ARGS, fit_fn=broken, loop_fn=loop_fn, controller=LIMITED)
    assert calls == [] and all(np.all(np.isnan(none[name])) for name in harness.MPC_OUT_SCORE_NAMES)
