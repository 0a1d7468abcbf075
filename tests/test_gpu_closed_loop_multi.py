"""GPU: the multi-model lifted closed loop scored on the device (nk_closed_loop_multi, harness.closed_loop_multi,
harness.cloth_lqr_sweep): every unit against the host loop in the reference's order of operations, the reference's recorded
cloth run (f10), the cumulative inputs and the scores recomputed from the returned trajectories, bit-identity of a unit
whatever else its call holds, NULL outputs, the argument checks, and the sweep on the committed cloth rows against the plain
loop it replaces.  Models are rebuilt from host copies; only the sweep fits on the device."""
import ctypes as C

import numpy as np
import pytest

from conftest import relf

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NODES = [168, 169, 170, 189, 190, 191]
# (m, p, d, steps, kind): one row / one lane, odd sizes, two u-rows, the cloth shape, the limits m = 128 and p = 8, a spline
SHAPES = [(1, 1, 1, 1, "nystrom"), (5, 1, 2, 2, "nystrom"), (33, 2, 6, 12, "nystrom"), (100, 6, 192, 60, "f10"),
          (128, 8, 3, 7, "nystrom"), (20, 1, 2, 30, "spline")]


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


def _regressor(nk, kind, m, p, d, rng):
    if kind == "spline":
        reg = nk.KoopmanSplineRegressor(p, m=m, gamma=1e-6)
        reg.centers = rng.standard_normal((d, m))
    else:
        reg = nk.KoopmanNystromRegressor(p, kernel=nk.KernelWrapper(np.ones(d)), gamma=1e-6, m=m)
        reg.nystrom_centers_output = rng.standard_normal((d, m))
    return reg


def _random_unit(nk, rng, m, p, d, kind="nystrom", a_scale=0.9, k_scale=0.2):
    """Random stable operators: A = 0.9 x a random orthogonal matrix; B and K scaled by 1 / sqrt(m), so that ||B K|| stays
    near 0.3 x 0.2 x (1 + sqrt(p / m))^2 < 0.1 and the closed loop A - B K is a contraction too."""
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    reg = _regressor(nk, kind, m, p, d, rng)
    u = dict(reg=reg, A=a_scale * Q, B=0.3 * rng.standard_normal((m, p)) / np.sqrt(m), C=rng.standard_normal((d, m)),
             K=k_scale * rng.standard_normal((p, m)) / np.sqrt(m), phi0=rng.standard_normal(m), phi_ref=rng.standard_normal(m),
             target=rng.standard_normal(d), u_init=rng.standard_normal(p), dims=(m, p, d))
    reg.A, reg.B, reg.C = u["A"], u["B"], u["C"]
    return u


def _f10_unit(nk, golden):
    g = golden("f10_lqr_control.npz")
    t = golden("cloth_trajs_all.npz")
    states = t["states_e10"] / 1e10
    Y = np.hstack([states[i][:, 1:] for i in range(10, 40)]).T
    reg = nk.KoopmanNystromRegressor(6, kernel=nk.ThreeDimensionalKernel(*g["ls"], 192), gamma=float(g["gamma"]), m=100)
    reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, g["idx"]])
    reg.A, reg.B, reg.C = g["A"], g["B"], g["C"]
    init, ref = g["initial_state"], g["reference_lqr"]
    phi = reg.lift(np.hstack((init, ref)))
    return dict(reg=reg, A=g["A"], B=g["B"], C=g["C"], K=g["K"], phi0=np.ascontiguousarray(phi[:, 0]),
                phi_ref=np.ascontiguousarray(phi[:, 1]), target=ref.reshape(-1), u_init=init.reshape(-1)[NODES],
                dims=(100, 6, 192), init=init, golden=g)


def _run(nk, units, steps, c=0.0075, **want):
    """One Context.closed_loop_multi call over `units`: dict of scores, err and the per-unit trajectory lists."""
    want = dict(dict(want_x=True, want_u=True, want_ucum=True, want_err=True, want_scores=True), **want)
    sc, err, ox, ou, oc = nk.get_context().closed_loop_multi(
        steps, c, [u["reg"]._ensure_model() for u in units], [u["dims"] for u in units], [u["K"] for u in units],
        [u["phi0"] for u in units], [u["phi_ref"] for u in units], [u["target"] for u in units],
        [u["u_init"] for u in units], **want)
    return dict(scores=sc, err=err, x=ox, u=ou, ucum=oc)


@pytest.fixture(scope="module")
def cases(nk, golden):
    """The six shapes, each run ALONE at its own step count with every output, and the host loop on the same operands."""
    from oracle import nk_oracle as O
    rng = np.random.default_rng(2024)
    out = []
    for (m, p, d, steps, kind) in SHAPES:
        u = _f10_unit(nk, golden) if kind == "f10" else _random_unit(nk, rng, m, p, d, kind)
        u["steps"] = steps
        u["res"] = _run(nk, [u], steps)
        u["host_x"], u["host_u"] = O.lqr_closed_loop_lifted(u["A"], u["B"], u["C"], u["K"], u["phi0"], u["phi_ref"], steps)
        out.append(u)
    return out


def _movement(u):
    """The host loop's own relF change when K is multiplied entrywise by 1 + 1e-15 xi (worst of 3 seeded draws)."""
    from oracle import nk_oracle as O
    rng = np.random.default_rng(7)
    mx = mu = 0.0
    for _ in range(3):
        K2 = u["K"] * (1.0 + 1e-15 * rng.standard_normal(u["K"].shape))
        x2, u2 = O.lqr_closed_loop_lifted(u["A"], u["B"], u["C"], K2, u["phi0"], u["phi_ref"], u["steps"])
        mx, mu = max(mx, relf(x2, u["host_x"])), max(mu, relf(u2, u["host_u"]))
    return mx, mu


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=[f"m{s[0]}-p{s[1]}-d{s[2]}-T{s[3]}-{s[4]}" for s in SHAPES])
def test_against_the_host_loop(cases, k):
    """out_x, out_u against oracle.lqr_closed_loop_lifted on the same A, B, C, K, phi0, phi_ref.  Bar:
    relF <= max(10 x movement, 1e-10), movement = what a 1e-15 relative perturbation of K does to the host loop itself."""
    u = cases[k]
    m, p, d = u["dims"]
    x, us = u["res"]["x"][0], u["res"]["u"][0]
    assert x.shape == (u["steps"], d) and us.shape == (u["steps"], p)
    mx, mu = _movement(u)
    ex, eu = relf(x.T, u["host_x"]), relf(us.T, u["host_u"])
    print(f"\n[{SHAPES[k]}] relF states {ex:.2e} (movement {mx:.2e}), controls {eu:.2e} (movement {mu:.2e})")
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(us))
    assert ex <= max(10.0 * mx, 1e-10) and eu <= max(10.0 * mu, 1e-10)


def test_f10_golden(cases):
    """The reference's operators, gain, initial_state, reference_lqr and u_init = initial_state[control_nodes]: the assembled
    x_s, y_s, z_s, final_us against the reference's recorded run, relF < 1e-8 (the bar of test_lqr_control_cloth_full)."""
    from nys_koop_lqr_amd import harness
    u = cases[3]
    g = u["golden"]
    got = harness.cloth_control_layout(u["init"], u["res"]["x"][0], u["res"]["ucum"][0])
    for arr, key in zip(got, ("x_s", "y_s", "z_s", "final_us")):
        e = relf(arr, g[key])
        print(f"\n[f10] {key}: relF {e:.2e}")
        assert arr.shape == g[key].shape and e < 1e-8, key


def test_cumulative_inputs_are_the_running_sum(nk, cases):
    """out_ucum is, bit for bit, s_0 = u_init, s_{t+1} = s_t + u_t over the returned out_u; also with u_init = NULL."""
    for u in cases:
        us, cum = u["res"]["u"][0], u["res"]["ucum"][0]
        s = np.array(u["u_init"], dtype=np.float64)
        assert cum.shape == (u["steps"] + 1, u["dims"][1]) and np.array_equal(cum[0], s)
        for t in range(u["steps"]):
            s = s + us[t]
            assert np.array_equal(cum[t + 1], s), (u["dims"], t)
    u = dict(cases[2], u_init=None)
    r = _run(nk, [u], u["steps"])
    assert np.array_equal(r["u"][0], cases[2]["res"]["u"][0]) and np.all(r["ucum"][0][0] == 0.0)
    s = np.zeros(u["dims"][1])
    for t in range(u["steps"]):
        s = s + r["u"][0][t]
        assert np.array_equal(r["ucum"][0][t + 1], s)


def test_scores_and_errors(cases):
    """Recomputed in NumPy from the returned out_x, out_u and the target.  All sums are of non-negative terms, so a sum in
    any fixed order is within n eps of the exact one: relative difference <= 4 (d + p + steps) eps for J, u_sumsq,
    err_final and every e_t; u_absmax exactly."""
    c = 0.0075
    for u in cases:
        m, p, d = u["dims"]
        x, us, sc, err = u["res"]["x"][0], u["res"]["u"][0], u["res"]["scores"][0], u["res"]["err"][0]
        sse = np.sum((x - u["target"]) ** 2, axis=1)
        usq = np.sum(us ** 2, axis=1)
        want = dict(J=np.sum(c * sse + usq), err_final=np.sqrt(sse[-1] / d), u_sumsq=np.sum(usq))
        bound = 4 * (d + p + u["steps"]) * EPS
        print(f"\n[{u['dims']}] device {sc.tolist()} numpy {want} u_absmax {np.max(np.abs(us))!r}")
        for k, name in enumerate(("J", "err_final", "u_sumsq")):
            assert abs(sc[k] - want[name]) <= bound * abs(want[name]), (u["dims"], name)
        e = np.sqrt(sse / d)
        assert err.shape == (u["steps"],) and np.all(np.abs(err - e) <= bound * e), u["dims"]
        assert sc[3] == np.max(np.abs(us)) and sc[1] == err[-1]


def _same(a, b, i, j):
    for key in ("x", "u", "ucum"):
        if not np.array_equal(a[key][i], b[key][j], equal_nan=True):
            return False
    return np.array_equal(a["err"][i], b["err"][j], equal_nan=True) and np.array_equal(a["scores"][i], b["scores"][j],
                                                                                       equal_nan=True)


def test_composition(nk, cases):
    """Six units mixing the shapes in one call: the same bits for each unit with the order reversed and alone in its call."""
    steps = 12
    fwd = _run(nk, cases, steps)
    rev = _run(nk, cases[::-1], steps)
    n = len(cases)
    for i, u in enumerate(cases):
        assert fwd["x"][i].shape == (steps, u["dims"][2]) and np.all(np.isfinite(fwd["scores"][i]))
        assert _same(fwd, rev, i, n - 1 - i), i
        assert _same(fwd, _run(nk, [u], steps), i, 0), i
    assert not np.array_equal(fwd["scores"][0], fwd["scores"][1])  # the units differ: equality above is not vacuous
    # a prefix of a longer run: the run at the unit's own step count starts with the same states
    assert np.array_equal(fwd["x"][3], cases[3]["res"]["x"][0][:steps])


def test_a_diverging_unit_does_not_disturb_the_others(nk, cases):
    """A = 1.5 I under a gain that does not stabilise it, 400 steps: the loop overflows, u_absmax is not finite, and the
    healthy units of the same call keep the bits they have without it."""
    from oracle import nk_oracle as O
    rng = np.random.default_rng(99)
    bad = _random_unit(nk, rng, 33, 2, 6, k_scale=500.0)
    bad["A"] = 1.5 * np.eye(33)
    bad["reg"].A = bad["A"]
    steps = 400
    with np.errstate(all="ignore"):
        hx, hu = O.lqr_closed_loop_lifted(bad["A"], bad["B"], bad["C"], bad["K"], bad["phi0"], bad["phi_ref"], steps)
    assert not np.all(np.isfinite(hu))  # the host loop diverges too
    mixed = _run(nk, [cases[2], bad, cases[5], cases[3]], steps)
    healthy = _run(nk, [cases[2], cases[5], cases[3]], steps)
    print(f"\nscores of the diverging unit: {mixed['scores'][1].tolist()}")
    assert not np.isfinite(mixed["scores"][1, 3])
    for i, j in ((0, 0), (2, 1), (3, 2)):
        assert _same(mixed, healthy, i, j) and np.all(np.isfinite(mixed["scores"][i])), i
    assert _same(mixed, _run(nk, [bad], steps), 1, 0)


def _table(units, keep, target=True):
    from nys_koop_lqr_amd import _lib
    arr = (_lib.LoopUnit * len(units))()
    for i, u in enumerate(units):
        vec = [np.ascontiguousarray(u[k], dtype=np.float64) for k in ("K", "phi0", "phi_ref", "target", "u_init")]
        keep.extend(vec)
        arr[i].model = u["reg"]._ensure_model().value
        arr[i].K, arr[i].phi0, arr[i].phi_ref = (v.ctypes.data for v in vec[:3])
        arr[i].target = vec[3].ctypes.data if target else None
        arr[i].u_init = vec[4].ctypes.data
    return arr


def test_null_outputs_and_canaries(nk, cases):
    """A scores-only call equals the scores of the full call; every combination with one output missing leaves the others
    unchanged; and a canary region behind each passed host buffer stays intact."""
    ctx = nk.get_context()
    units = [cases[2], cases[5], cases[4]]
    steps, n, tail = 9, 3, 64
    full = _run(nk, units, steps)
    only = _run(nk, units, steps, want_x=False, want_u=False, want_ucum=False, want_err=False)
    assert only["x"] is None and only["u"] is None and only["ucum"] is None and only["err"] is None
    assert np.array_equal(only["scores"], full["scores"])
    no_sc = _run(nk, units, steps, want_scores=False, want_x=False)
    assert no_sc["scores"] is None and np.array_equal(no_sc["err"], full["err"])
    assert all(np.array_equal(a, b) for a, b in zip(no_sc["ucum"], full["ucum"]))
    sizes = dict(x=sum(steps * u["dims"][2] for u in units), u=sum(steps * u["dims"][1] for u in units),
                 ucum=sum((steps + 1) * u["dims"][1] for u in units), err=n * steps, scores=4 * n)
    bufs = {k: np.full(sz + tail, -7.25) for k, sz in sizes.items()}
    keep = []
    rc = ctx.lib.nk_closed_loop_multi(ctx.handle, steps, 0.0075, _table(units, keep), n,
                                      *[bufs[k].ctypes.data for k in ("x", "u", "ucum", "err", "scores")])
    assert rc == 0, ctx.lib.nk_last_error()
    for k, sz in sizes.items():
        assert np.all(bufs[k][sz:] == -7.25), k
        assert not np.any(bufs[k][:sz] == -7.25), k
    assert np.array_equal(bufs["x"][:sizes["x"]], np.concatenate([a.reshape(-1) for a in full["x"]]))
    assert np.array_equal(bufs["scores"][:4 * n].reshape(n, 4), full["scores"])


def test_argument_checks(nk, cases):
    """Each bad call returns NK_ERR_BAD_ARG, names the unit where there is one, and writes nothing."""
    from nys_koop_lqr_amd import _lib
    ctx = nk.get_context()
    lib = ctx.lib
    rng = np.random.default_rng(3)
    good = [cases[1], cases[2]]
    steps = 5
    big = _random_unit(nk, rng, 129, 1, 2)  # m = 129, with operators
    wide = dict(_random_unit(nk, rng, 4, 1, 2), dims=(4, 9, 2))  # p = 9 and no operators: refused by its size first
    wide["reg"] = _regressor(nk, "nystrom", 4, 9, 2, rng)
    wide["K"], wide["u_init"] = np.zeros((9, 4)), np.zeros(9)
    bare = _random_unit(nk, rng, 5, 1, 2)  # landmarks, no operators
    bare["reg"] = _regressor(nk, "nystrom", 5, 1, 2, rng)
    outs = [np.full(4096, 7.0) for _ in range(5)]
    keep = []

    def call(handle, units, n=None, steps=steps, c=0.0075, outs=outs, target=True):
        ptrs = [None if o is None else o.ctypes.data for o in outs]
        rc = lib.nk_closed_loop_multi(handle, steps, c, _table(units, keep, target), len(units) if n is None else n, *ptrs)
        return rc, lib.nk_last_error()

    rc, msg = call(ctx.handle, [good[0], big])
    assert rc == -1 and b"unit 1" in msg and b"m = 129" in msg, (rc, msg)
    rc, msg = call(ctx.handle, [wide, good[0]])
    assert rc == -1 and b"unit 0" in msg and b"p = 9" in msg, (rc, msg)
    rc, msg = call(ctx.handle, [good[0], good[1], bare])
    assert rc == -1 and b"unit 2" in msg and b"operators" in msg, (rc, msg)
    rc, msg = call(ctx.handle, good, steps=0)
    assert rc == -1 and b"steps" in msg, (rc, msg)
    rc, msg = call(ctx.handle, good, c=-1.0)
    assert rc == -1 and b"c must be" in msg, (rc, msg)
    rc, msg = call(ctx.handle, good, c=float("nan"))
    assert rc == -1 and b"c must be" in msg, (rc, msg)
    rc, msg = call(ctx.handle, good, outs=[None] * 5)
    assert rc == -1 and b"null" in msg, (rc, msg)
    rc, msg = call(ctx.handle, good, target=False)
    assert rc == -1 and b"unit 0" in msg and b"target" in msg, (rc, msg)
    rc, msg = call(ctx.handle, good, n=0)
    assert rc == -1 and b"n_units" in msg, (rc, msg)
    assert all(np.all(o == 7.0) for o in outs)  # nothing was written by any refused call
    rc, msg = call(ctx.handle, good, outs=outs[:3] + [None, None], target=False)  # without scores no target is needed ...
    assert rc == 0, (rc, msg)
    assert np.array_equal(outs[0][:steps * 2], _run(nk, [good[0]], steps)["x"][0].reshape(-1))
    assert np.all(outs[3] == 7.0) and np.all(outs[4] == 7.0)
    for o in outs:
        o[:] = 7.0
    handles = (C.c_void_p * 2)()
    _lib.check(lib.nk_group_create(ctx.device, 2, handles))
    members = [_lib.Context(ctx.device, C.c_void_p(handles[i])) for i in range(2)]
    try:
        rc, msg = call(members[0].handle, good)  # ... and a lock-step member is refused
        assert rc == -1 and b"lock-step" in msg, (rc, msg)
    finally:
        for mem in members:
            mem.close()
    assert all(np.all(o == 7.0) for o in outs)
    # the Python layer turns the code into ValueError, and the call still works afterwards
    with pytest.raises(ValueError, match="unit 1"):
        _run(nk, [good[0], big], steps)
    assert np.all(np.isfinite(_run(nk, good, steps)["scores"]))


def test_harness_paths(nk, cases):
    """harness.closed_loop_multi lifts with reg.lift and defaults the target to x_ref; a model with m > 128 takes the
    single-model call and is scored on the host by the same formulas (held to the device's bars against each other)."""
    from nys_koop_lqr_amd import harness
    rng = np.random.default_rng(17)
    small, large = _random_unit(nk, rng, 40, 2, 6), _random_unit(nk, rng, 150, 2, 6)
    x0, xr = rng.standard_normal(6), rng.standard_normal(6)
    steps = 10
    res = harness.closed_loop_multi([small["reg"], large["reg"]], [small["K"], large["K"]], x0, xr, steps,
                                    return_trajectories=True)
    assert res["path"] == ["device", "single"] and res["states"].shape == (2, steps, 6)
    assert res["cum_controls"].shape == (2, steps + 1, 2) and np.all(res["cum_controls"][:, 0] == 0.0)
    for i, u in enumerate((small, large)):
        phi = u["reg"].lift(np.stack((x0, xr), axis=1))
        sc = harness.closed_loop_scores(res["states"][i], res["controls"][i], xr)
        bound = 4 * (6 + 2 + steps) * EPS
        for name in ("J", "err_final", "u_sumsq"):
            assert abs(res[name][i] - sc[name]) <= bound * abs(sc[name]), (i, name)
        assert res["u_absmax"][i] == sc["u_absmax"] and np.all(np.abs(res["err"][i] - sc["err"]) <= bound * sc["err"])
        xs, us = u["reg"].closed_loop(u["K"], phi[:, 0], phi[:, 1], steps)  # the (A - B K) form: to rounding
        assert relf(res["states"][i].T, xs) < 1e-9 and relf(res["controls"][i].T, us) < 1e-8
    assert np.array_equal(res["states"][1].T, large["reg"].closed_loop(large["K"], *large["reg"].lift(
        np.stack((x0, xr), axis=1)).T, steps)[0])


@pytest.fixture(scope="module")
def cloth(golden):
    g = golden("f10_lqr_control.npz")
    t = golden("cloth_trajs_all.npz")
    states = t["states_e10"] / 1e10
    X = np.ascontiguousarray(np.hstack([np.vstack((states[i][:, :-1], t["inputs"][i][:, :-1])) for i in range(10, 40)]).T)
    Y = np.ascontiguousarray(np.hstack([states[i][:, 1:] for i in range(10, 40)]).T)
    return dict(X=X, Y=Y, g=g, x0=g["initial_state"].reshape(-1), x_ref=g["reference_lqr"].reshape(-1))


def test_sweep_on_the_cloth_rows(nk, cloth):
    """cloth_lqr_sweep on trajectories 10..39 (f10's kernel, gamma and m = 100), seeds 0..2, both estimators, batch 0 and 4:
    per unit, states and controls equal, bit for bit, closed_loop_multi on a plain reg.fit + solve_lqr of the same unit.
    With gain="device" the scores are finite and J is within 1e-6 relative of the gain="host" run (the device solver is held
    to 10 x scipy's own movement elsewhere, and the closed loop is a contraction: rho(A - BK) = 0.9976 on f10)."""
    from nys_koop_lqr_amd import harness
    g, X, Y, x0, x_ref = cloth["g"], cloth["X"], cloth["Y"], cloth["x0"], cloth["x_ref"]
    params = dict(nystrom=dict(kernel=nk.ThreeDimensionalKernel(*g["ls"], 192), gamma=float(g["gamma"])),
                  spline=dict(gamma=float(g["gamma"])))
    seeds, names = [0, 1, 2], ("nystrom", "spline")
    _, units = harness.cloth_lqr_plan(X, Y, 6, params, 100, seeds, names)
    assert np.array_equal(units[0]["marks"], g["idx"])  # seed 0: the landmark draw the reference's run recorded
    plain = []
    for u in units:
        reg = harness.lqr_fit_unit(X, Y, 6, u["params"], u, u["estimator"])
        K = reg.solve_lqr(c=0.0075)
        plain.append(harness.closed_loop_multi([reg], [K], x0, x_ref, 60, u_inits=[x0[NODES]], return_trajectories=True))
    runs = {}
    for batch in (0, 4):
        runs[batch] = r = harness.cloth_lqr_sweep(X, Y, 6, params, 100, seeds, x0, x_ref, estimator=names, batch=batch,
                                                  return_trajectories=True)
        assert r["J"].shape == (2, 3) and r["err"].shape == (2, 3, 60) and r["x_s"].shape == (2, 3, 64, 61)
        print(f"\n[batch {batch}] J {r['J'].tolist()} err_final {r['err_final'].tolist()} timing {r['timing']}")
        for u, pl in zip(units, plain):
            at = (u["ei"], u["si"])
            assert np.all(np.isfinite(pl["states"][0])) and np.isfinite(pl["J"][0])
            assert np.array_equal(r["states"][at], pl["states"][0]), (batch, at)
            assert np.array_equal(r["controls"][at], pl["controls"][0]), (batch, at)
            assert np.array_equal(r["final_us"][at], pl["cum_controls"][0].T[[0, 3, 1, 4, 2, 5]]), (batch, at)
            for name in harness.LOOP_SCORE_NAMES:
                assert r[name][at] == pl[name][0], (batch, at, name)
    dev = harness.cloth_lqr_sweep(X, Y, 6, params, 100, seeds, x0, x_ref, estimator=names, batch=4, gain="device")
    rel = np.abs(dev["J"] - runs[4]["J"]) / runs[4]["J"]
    print(f"\n[gain=device] J {dev['J'].tolist()}; relative to gain=host {rel.tolist()}")
    for name in harness.LOOP_SCORE_NAMES:
        assert np.all(np.isfinite(dev[name])), name
    assert np.all(rel <= 1e-6)
