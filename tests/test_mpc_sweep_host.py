"""CPU: the host side of the one-call MPC control sweep -- the C-ABI declares and exports nk_mpc_loop_multi and its unit
struct, harness.mpc_scores states the eight scores of the call on hand-made arrays, and the bookkeeping of
harness.lqr_sweep(controller=...) and dist.sharded_lqr_sweep(controller=...) holds with stubs standing in for the fits, the
controllers and the device loop."""
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


def test_mpc_multi_declared_exported_and_mirrored(lib):
    from nys_koop_lqr_amd import _lib, harness
    header = open(os.path.join(ROOT, "include", "nyskoop.h")).read()
    declared = set(re.findall(r"\b(nk_[a-z_0-9]+)\s*\(", header))
    assert "nk_mpc_loop_multi" in declared and "nk_mpc_loop_multi" in _lib.SIGNATURES
    assert hasattr(lib, "nk_mpc_loop_multi")
    assert re.search(r"#define\s+NK_MPC_N_SCORES\s+8\b", header) and _lib.MPC_N_SCORES == 8 == len(harness.MPC_SCORE_NAMES)
    assert re.search(r"#define\s+NK_ABI_VERSION\s+2\b", header) and lib.nk_version() == 2  # symbols added, nothing changed
    # the documented layout of nk_mpc_unit on an LP64 target: five pointers, then two int32 -- 48 bytes, no padding
    body = re.search(r"typedef struct nk_mpc_unit \{(.*?)\} nk_mpc_unit;", header, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["model", "desc", "x0", "x_ref", "u_init", "uopt", "reserved"]
    assert [f[0] for f in _lib.MpcUnit._fields_] == fields
    assert C.sizeof(_lib.MpcUnit) == 48
    assert [getattr(_lib.MpcUnit, f).offset for f in fields] == [0, 8, 16, 24, 32, 40, 44]
    assert [getattr(_lib.MpcUnit, f).size for f in fields] == [8, 8, 8, 8, 8, 4, 4]
    # the prototype: ctx, plant, steps, units, n_units, u_opt, n_uopt, out_x, out_u, out_info, scores
    res, args = _lib.SIGNATURES["nk_mpc_loop_multi"]
    assert res is C.c_int and len(args) == 11 and args[3] is C.POINTER(_lib.MpcUnit) and args[2] is C.c_int32
    assert harness.MPC_SCORE_NAMES[:4] == harness.SCORE_NAMES


def _bounds(lo, hi, dlo, dhi):
    return SimpleNamespace(lo=np.array(lo, dtype=np.float64), hi=np.array(hi, dtype=np.float64),
                           dlo=np.array(dlo, dtype=np.float64), dhi=np.array(dhi, dtype=np.float64))


def test_mpc_scores_on_hand_made_arrays():
    """One input, horizon 2 (the bounds carry nv = 2 entries, the first p = 1 are the applied move's): each of the four bounds
    hit once, a step inside all of them, then a NaN control and an absent u_opt."""
    from nys_koop_lqr_amd import harness
    ctl = _bounds([-1.0, -9.0], [2.0, 9.0], [-0.25, -9.0], [0.5, 9.0])
    u_init = np.array([0.125])
    # t = 0: u = 0.625 = 0.125 + 0.5 (dhi);  t = 1: u = 0.375 = 0.625 - 0.25 (dlo);  t = 2: u = 0.5 (inside everything)
    us = np.array([[0.625, 0.375, 0.5]])
    xs = np.array([[1.0, 0.5, 0.25, 0.125], [0.0, 1.0, 2.0, 3.0]])
    info = np.array([[3.0, 0.5], [0.0, 0.0], [2.0, 0.75]])
    u_opt = np.array([0.5, 0.5, 0.25])
    sc = harness.mpc_scores(xs, us, info, ctl, u_opt, u_init)
    base = harness.control_scores(xs, us, u_opt)
    for name in harness.SCORE_NAMES + ("rmse_control",):
        assert sc[name] == base[name], name
    assert sc["sse_u"] == (0.125 * 0.125 + 0.125 * 0.125) + 0.25 * 0.25 and sc["ss_opt"] == (0.25 + 0.25) + 0.0625
    assert sc["iters_sum"] == 5.0 and sc["r_max"] == 0.75 and sc["n_at_limit"] == 2.0 and sc["n_iterated"] == 2.0
    # the box: hi, then lo (rates wide open), then nothing
    box = _bounds([-1.0, -9.0], [2.0, 9.0], [-INF, -INF], [INF, INF])
    us2 = np.array([[2.0, -1.0, 0.0]])
    sc2 = harness.mpc_scores(xs, us2, info, box)
    assert sc2["n_at_limit"] == 2.0 and sc2["sse_u"] == 0.0 and sc2["ss_opt"] == 0.0 and np.isnan(sc2["rmse_control"])
    # all four bounds once in one walk: dhi, hi, dlo, lo, and a free step; (steps, p) controls are accepted as well
    four = _bounds([-0.5], [1.0], [-1.25], [0.75])
    us4 = np.array([[0.75, 1.0, -0.25, -0.5, 0.0]])  # 0 + 0.75 | hi | 1.0 - 1.25 | lo | inside
    xs4 = np.zeros((1, 6))
    info4 = np.zeros((5, 2))
    sc4 = harness.mpc_scores(xs4, us4, info4, four)
    assert sc4["n_at_limit"] == 4.0 and sc4["n_iterated"] == 0.0 and sc4["iters_sum"] == 0.0 and sc4["r_max"] == 0.0
    tr = harness.mpc_scores(xs4, us4.T, info4, four)
    assert all(tr[name] == sc4[name] for name in harness.MPC_SCORE_NAMES)
    # two inputs: a (t, j) at two bounds at once counts once; the counts run over both inputs
    two = _bounds([-1.0, -2.0, 0, 0], [1.0, 2.0, 0, 0], [-1.0, -INF, 0, 0], [1.0, INF, 0, 0])
    usb = np.array([[1.0, 0.5], [2.0, -2.0]])  # t = 0: input 0 at hi AND at 0 + dhi, input 1 at hi; t = 1: input 1 at lo
    scb = harness.mpc_scores(np.zeros((2, 3)), usb, np.zeros((2, 2)), two)
    assert scb["n_at_limit"] == 3.0
    # a NaN control: u_absmax is NaN whatever follows, and it equals no bound; a NaN residual stays
    bad = us4.copy()
    bad[0, 1] = np.nan
    info_bad = info4.copy()
    info_bad[2, 1] = np.nan
    info_bad[3, 1] = 5.0
    scn = harness.mpc_scores(xs4, bad, info_bad, four)
    assert np.isnan(scn["u_absmax"]) and np.isnan(scn["r_max"])
    assert scn["n_at_limit"] == 2.0  # dhi at t = 0 and lo at t = 3; t = 2 follows a NaN: its rate bounds are NaN


def _stubs(fail=None):
    """Stand-ins: a 'fit' whose solve_mpc returns a controller tagged with its unit (raising for the chosen unit), an MPC 'loop'
    that scores a unit by its tag and records what it was handed, and an LQR 'loop' with today's signature."""
    calls = []

    def fit_fn(X, Y, n_inputs, params, unit, estimator):
        tag = 10.0 * unit["si"] + unit["k"] + 1.0

        def solve_mpc(horizon, c=1.0, u_min=None, u_max=None, du_min=None, du_max=None, rho=None):
            if fail is not None and (unit["si"], unit["k"]) == fail:
                raise np.linalg.LinAlgError("no stabilising solution")
            return SimpleNamespace(tag=tag, spec=(horizon, c, u_min, u_max, du_min, du_max, rho))

        return SimpleNamespace(A=np.full((2, 2), tag), B=np.ones((2, 1)), C=np.ones((1, 2)), tag=tag, solve_mpc=solve_mpc)

    def mpc_loop_fn(regs, ctls, x0, x_ref, num_steps, plant, iters=50, tol=0.0, u_opt=None, return_trajectories=False):
        calls.append(("mpc", [r.tag for r in regs], [c.spec for c in ctls], iters, tol))
        tags = np.array([r.tag for r in regs])
        assert [c.tag for c in ctls] == list(tags)
        out = dict(sse_u=tags, ss_opt=4.0 * tags, J=tags + 0.5, u_absmax=-tags, iters_sum=2.0 * tags, r_max=0.25 * tags,
                   n_at_limit=3.0 * tags, n_iterated=tags - 1.0)
        if return_trajectories:
            out["states"] = np.tile(tags[:, None, None], (1, num_steps + 1, 2))
            out["controls"] = np.tile(tags[:, None, None], (1, num_steps, 1))
        return out

    def lqr_loop_fn(regs, gains, x0, x_ref, num_steps, plant, u_opt=None, return_trajectories=False):
        calls.append(("lqr", [r.tag for r in regs]))
        tags = np.array([r.tag for r in regs])
        return dict(sse_u=tags, ss_opt=4.0 * tags, J=tags + 0.5, u_absmax=-tags)

    return fit_fn, mpc_loop_fn, lqr_loop_fn, calls


ARGS = (np.zeros((50, 3)), np.zeros((50, 2)), 1, dict(kernel=None, gamma=1e-6), [4, 6], [0, 1, 2], None, np.zeros(2), np.zeros(2), 5)
BOX = dict(horizon=8, u_min=-0.5, u_max=0.5, du_max=0.1, iters=30, tol=1e-6)
NEW = ("iters_sum", "r_max", "n_at_limit", "n_iterated")


def test_a_failing_controller_is_nan_and_is_not_run():
    from nys_koop_lqr_amd import harness
    fit_fn, loop_fn, _, calls = _stubs()
    full = harness.lqr_sweep(*ARGS, c=2.0, fit_fn=fit_fn, loop_fn=loop_fn, return_trajectories=True, controller=BOX)
    assert len(calls) == 1  # ONE loop call, every unit, in plan (m-major) order, iters and tol handed on
    kind, tags_seen, specs, iters, tol = calls[0]
    assert kind == "mpc" and tags_seen == [1.0, 11.0, 21.0, 2.0, 12.0, 22.0] and (iters, tol) == (30, 1e-6)
    assert all(s == (8, 2.0, -0.5, 0.5, None, 0.1, None) for s in specs)  # reg.solve_mpc(horizon, c=c, limits, rho)
    tags = np.array([[1.0, 2.0], [11.0, 12.0], [21.0, 22.0]])
    assert np.array_equal(full["J"], tags + 0.5) and np.array_equal(full["iters_sum"], 2.0 * tags)
    assert np.array_equal(full["r_max"], 0.25 * tags) and np.array_equal(full["n_at_limit"], 3.0 * tags)
    assert np.array_equal(full["n_iterated"], tags - 1.0) and np.array_equal(full["rmse_control"], np.full((3, 2), 50.0))
    assert full["states"].shape == (3, 2, 6, 2) and full["controls"].shape == (3, 2, 5, 1)
    fit_fn, loop_fn, _, calls = _stubs(fail=(1, 1))
    part = harness.lqr_sweep(*ARGS, c=2.0, fit_fn=fit_fn, loop_fn=loop_fn, return_trajectories=True, controller=BOX)
    assert [c[1] for c in calls] == [[1.0, 11.0, 21.0, 2.0, 22.0]]  # the unit without a controller is not submitted
    hole = np.zeros((3, 2), dtype=bool)
    hole[1, 1] = True
    for name in harness.MPC_SCORE_NAMES + ("rmse_control",):
        assert np.all(np.isnan(part[name][hole])) and np.array_equal(part[name][~hole], full[name][~hole]), name
    assert np.all(np.isnan(part["states"][1, 1])) and np.all(np.isnan(part["controls"][1, 1]))
    # every controller fails: no loop call at all, all-NaN tables of all eight names
    fit_fn, loop_fn, _, calls = _stubs()

    def broken(*a):
        reg = fit_fn(*a)
        reg.solve_mpc = lambda *b, **kw: (_ for _ in ()).throw(ValueError("u_min <= u_max"))
        return reg

    none = harness.lqr_sweep(*ARGS, fit_fn=broken, loop_fn=loop_fn, controller=BOX)
    assert calls == [] and all(np.all(np.isnan(none[name])) for name in harness.MPC_SCORE_NAMES) and "states" not in none


def test_controller_with_device_gain_raises_and_bad_keys_are_named():
    from nys_koop_lqr_amd import dist, harness
    fit_fn, loop_fn, _, calls = _stubs()
    with pytest.raises(ValueError, match="host Riccati"):
        harness.lqr_sweep(*ARGS, fit_fn=fit_fn, loop_fn=loop_fn, controller=BOX, gain="device")
    with pytest.raises(ValueError, match="host Riccati"):
        dist.sharded_lqr_sweep(*ARGS, fit_fn=fit_fn, loop_fn=loop_fn, controller=BOX, gain="device")
    with pytest.raises(ValueError, match="horizon"):
        harness.lqr_sweep(*ARGS, fit_fn=fit_fn, loop_fn=loop_fn, controller=dict(u_max=1.0))
    with pytest.raises(ValueError, match="umax"):
        harness.lqr_sweep(*ARGS, fit_fn=fit_fn, loop_fn=loop_fn, controller=dict(horizon=4, umax=1.0))
    assert calls == []


def test_controller_none_calls_loop_fn_with_todays_arguments():
    """controller=None: the stand-in with today's signature (no iters, no tol) is called as before, four score tables."""
    from nys_koop_lqr_amd import harness
    fit_fn, _, lqr_loop, calls = _stubs()
    res = harness.lqr_sweep(*ARGS, gain_fn=lambda A, B, C: np.full((1, 2), A[0, 0]), fit_fn=fit_fn, loop_fn=lqr_loop,
                            controller=None)
    assert calls == [("lqr", [1.0, 11.0, 21.0, 2.0, 12.0, 22.0])]
    assert all(name in res for name in harness.SCORE_NAMES) and not any(name in res for name in NEW)


def test_sharded_sweep_in_a_world_of_one_equals_the_plain_sweep():
    from nys_koop_lqr_amd import dist, harness
    fit_fn, loop_fn, _, calls = _stubs(fail=(2, 0))
    plain = harness.lqr_sweep(*ARGS, fit_fn=fit_fn, loop_fn=loop_fn, controller=BOX)
    sh = dist.sharded_lqr_sweep(*ARGS, fit_fn=fit_fn, loop_fn=loop_fn, controller=BOX)
    assert len(calls) == 2 and calls[0] == calls[1]
    for name in harness.MPC_SCORE_NAMES + ("rmse_control",):
        assert np.array_equal(sh[name], plain[name], equal_nan=True), name
    assert np.isnan(plain["J"][2, 0]) and np.sum(np.isnan(plain["J"])) == 1


def test_nan_step_of_the_host_qp_is_the_numpy_statement(lib):
    """nk_mpc_qp_host at a NaN lifted error and at a NaN previous control against lqr.MPCController.control (np.minimum /
    np.maximum hand a NaN on): NaN control, all iterations counted, NaN residual; iters = 0: NaN control, zeros in info; a
    finite step beside them keeps the values of the NumPy statement."""
    from nys_koop_lqr_amd import _lib, lqr
    rng = np.random.default_rng(0)
    nv, m = 4, 6
    G = rng.standard_normal((nv, nv))
    H = np.eye(nv) + G @ G.T
    lo, hi, dlo, dhi = lqr.mpc_bounds(nv, -1.0, 1.0, -0.1, 0.1)
    ctl = lqr.MPCController(H, rng.standard_normal((nv, m)), lo, hi, dlo, dhi, rng.standard_normal((1, m)), lqr.mpc_default_rho(H), nv)

    def host(e, u_prev, iters, tol=0.0):
        ds, keep = _lib.mpc_desc(ctl, iters, tol)
        e, u_prev = np.ascontiguousarray(e, dtype=np.float64), np.ascontiguousarray(u_prev, dtype=np.float64)
        u, z, info = np.full(1, 7.0), np.full(nv, 7.0), np.full(2, 7.0)
        _lib.check(lib.nk_mpc_qp_host(C.byref(ds), e.ctypes.data, u_prev.ctypes.data, u.ctypes.data, z.ctypes.data,
                                      info.ctypes.data))
        return u, info

    bad = np.ones(m)
    bad[2] = np.nan
    for e, up, iters, tol in ((bad, [0.0], 7, 0.0), (bad, [0.0], 7, 1e-3), (bad, [0.0], 0, 0.0), (np.ones(m), [np.nan], 7, 0.0),
                              (np.ones(m), [np.nan], 0, 0.0), (np.ones(m), [0.05], 7, 0.0), (np.ones(m), [0.05], 0, 0.0)):
        u, info = host(e, up, iters, tol)
        u_ref, info_ref = ctl.control(np.asarray(e), np.asarray(up, dtype=np.float64), iters, tol)
        assert np.array_equal(np.isnan(u), np.isnan(u_ref)) and info[0] == info_ref[0], (up, iters, u, u_ref, info, info_ref)
        assert np.isnan(info[1]) == np.isnan(info_ref[1])
        if not np.any(np.isnan(u_ref)):
            assert np.allclose(u, u_ref, rtol=1e-12, atol=0) and abs(info[1] - info_ref[1]) <= 1e-12
    assert np.isnan(host(bad, [0.0], 7)[0][0]) and np.isnan(host(np.ones(m), [np.nan], 0)[0][0])
