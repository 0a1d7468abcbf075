"""GPU: the controller build on the device (nk_mpc_build_batch, nk_model_mpc_build_batch; csrc/nk_mpc_build.hip, one workgroup
per unit) at the smallest shapes at which padding, tiling and the recursions can go wrong: the condensing alone against the
np.longdouble evaluation of its statement (tests/mpc_build_reference.py), bit-for-bit independence of what else a call holds,
the Riccati and Newton stages under the bars of tests/dare_reference.py, the status codes, the refusals with guard bands, the
model entry behind reg.solve_mpc(device=True) and the sweep with build="device"."""
import ctypes as C

import numpy as np
import pytest

import dare_reference as dr
import mpc_build_reference as mr

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


def _bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _condense(nk, cases, order=None):
    """The cases (mr.condense_case dicts) in one call with P given; returns the per-case dicts of outputs in `cases` order."""
    order = list(range(len(cases))) if order is None else list(order)
    cs = [cases[i] for i in order]
    res = nk.lqr.mpc_build_batch([c["A"] for c in cs], [c["B"] for c in cs], [c["Q"] for c in cs], [c["R"] for c in cs],
                                 [c["N"] for c in cs], Ps=[c["P"] for c in cs], C_rows=[c["C_rows"] for c in cs],
                                 Nys=[c["Ny"] or None for c in cs])
    assert np.all(res["status"] == 0), res["status"]
    out = [None] * len(cases)
    for k, i in enumerate(order):
        out[i] = {key: res[key][k] for key in ("H", "F", "K", "P", "G", "T")}
    return out


@pytest.fixture(scope="module")
def cases():
    return [mr.condense_case(*sh) for sh in mr.GPU_SHAPES]


@pytest.fixture(scope="module")
def together(nk, cases):
    return _condense(nk, cases)


# ---- 1. condensing alone -------------------------------------------------------------------------------------------------
def _check_condensed(case, got, shape):
    m, p, N, nc, Ny = shape
    for key in ("H", "F", "K") + (("G", "T") if nc else ()):
        e, b = mr.err(got[key], case[key + "_ld"]), mr.bar(case["own"][key])
        print(f"{shape} {key}: err {e:.3e} own {case['own'][key]:.3e} bar {b:.3e}")
        assert e <= b, (shape, key, e, b)
    assert _bits(got["H"], got["H"].T)
    assert _bits(got["P"], case["P"])
    if nc:
        for k in range(1, Ny + 1):
            blk = got["G"][(k - 1) * nc:k * nc, k * p:]
            assert _bits(blk, np.zeros_like(blk)), (shape, k)
    else:
        assert got["G"] is None and got["T"] is None


@pytest.mark.parametrize("idx", range(len(mr.GPU_SHAPES)), ids=[str(s) for s in mr.GPU_SHAPES])
def test_condensing_alone_meets_the_extended_evaluation(nk, cases, idx):
    _check_condensed(cases[idx], _condense(nk, [cases[idx]])[0], mr.GPU_SHAPES[idx])


def test_condensing_in_one_call_meets_the_extended_evaluation(cases, together):
    for case, got, shape in zip(cases, together, mr.GPU_SHAPES):
        _check_condensed(case, got, shape)


# ---- 2. independence -----------------------------------------------------------------------------------------------------
def test_a_unit_does_not_depend_on_the_call_it_is_in(nk, cases, together):
    n = len(cases)
    runs = [_condense(nk, cases, order=range(n - 1, -1, -1))]
    half = n // 2
    a, b = _condense(nk, cases[:half]), _condense(nk, cases[half:])
    runs.append(a + b)
    runs.append([_condense(nk, [c])[0] for c in cases])
    for run in runs:
        for i in range(n):
            for key in ("H", "F", "K", "P", "G", "T"):
                assert _bits(run[i][key], together[i][key]), (mr.GPU_SHAPES[i], key)


# ---- 3. Riccati + Newton ---------------------------------------------------------------------------------------------------
RICCATI = [("r5", 5, 1, 8), ("r17", 17, 3, 5), ("r33", 33, 1, 8), ("f3", 50, 1, 16), ("f8", 200, 1, 8), ("f12_m200", 200, 1, 8),
           ("r256", 256, 4, 4), ("r257", 257, 1, 6)]


@pytest.fixture(scope="module")
def riccati_problems():
    out = {}
    for label, m, p, N in RICCATI:
        if label.startswith("r"):
            A, B, Q, R = dr.random_problem(m, p, 1.1, seed=m)
            ref = dr.reference(A, B, Q, R, seed=m)
        else:
            A, B, Q, R = dr.fixture_problem(label)
            ref = dr.fixture_reference(label)
        assert A.shape == (m, m) and B.shape == (m, p)
        out[label] = dict(A=A, B=B, Q=Q, R=R, N=N, ref=ref)
    return out


def _first_move_gap(H, F, K, p):
    return float(np.linalg.norm(np.linalg.solve(H, F)[:p] - K) / np.linalg.norm(K))


def _build(nk, probs, **kw):
    return nk.lqr.mpc_build_batch([q["A"] for q in probs], [q["B"] for q in probs], [q["Q"] for q in probs],
                                  [q["R"] for q in probs], [q["N"] for q in probs], **kw)


def test_riccati_and_newton_meet_the_scipy_bars(nk, riccati_problems):
    labels = [r[0] for r in RICCATI]
    probs = [riccati_problems[k] for k in labels]
    res = _build(nk, probs)
    assert np.all(res["status"] == 0), res["status"]
    for i, (label, m, p, N) in enumerate(RICCATI):
        q = probs[i]
        K, P, H, F = res["K"][i], res["P"][i], res["H"][i], res["F"][i]
        rbar, kbar = dr.bars(q["ref"], m)
        r, dk = dr.residual(q["A"], q["B"], q["Q"], P, K), dr.relk(K, q["ref"]["K"])
        Kh, Ph = nk.lqr.dare_refine(q["A"], q["B"], q["Q"], q["R"], nk.lqr.dlqr(q["A"], q["B"], q["Q"], q["R"])[0])
        Hh, Fh = nk.lqr.mpc_condense(q["A"], q["B"], q["Q"], q["R"], Ph, N)
        gap, gap_host = _first_move_gap(H, F, K, p), _first_move_gap(Hh, Fh, Kh, p)
        gbar = max(10 * gap_host, 64 * m * EPS)
        print(f"{label}: residual {r:.3e} (bar {rbar:.3e})  gain {dk:.3e} (bar {kbar:.3e})  first move {gap:.3e} "
              f"(host {gap_host:.3e}, bar {gbar:.3e})  iters {res['iters'][i]}")
        assert r <= rbar, (label, r, rbar)
        assert dk <= kbar, (label, dk, kbar)
        assert gap <= gbar, (label, gap, gbar)
        assert res["iters"][i][0] >= 1 and res["iters"][i][1] >= 1


def test_without_newton_steps_the_gain_is_the_riccati_solvers(nk, riccati_problems):
    ctx = nk.get_context()
    small = [riccati_problems[k] for k, m, _, _ in RICCATI if m <= 256]
    res = _build(nk, small, newton_steps=0)
    Ks, Ps, st, it, _ = ctx.dare_batch([q["A"] for q in small], [q["B"] for q in small], [q["Q"] for q in small],
                                       [q["R"] for q in small])
    assert np.all(res["status"] == 0) and np.all(st == 0)
    for i in range(len(small)):
        assert _bits(res["K"][i], Ks[i]) and _bits(res["P"][i], Ps[i])
        assert res["iters"][i][0] == it[i] and res["iters"][i][1] == 0
    q = riccati_problems["r257"]
    res = _build(nk, [q], newton_steps=0)
    K, P, st, _, _ = ctx.dare_large(q["A"], q["B"], q["Q"], q["R"])
    assert res["status"][0] == 0 and st == 0
    assert _bits(res["K"][0], K) and _bits(res["P"][0], P)


# ---- 4. status -------------------------------------------------------------------------------------------------------------
def _all_nan(res, i):
    return all(np.all(np.isnan(res[key][i])) for key in ("H", "F", "K", "P"))


def _zero_a_problem(m, p, N):
    """A = 0: the doubling and the Smith iteration both stop at their first step, whatever the caps are."""
    A, B, Q, R = dr.random_problem(m, p, 0.5, seed=70 + m)
    return dict(A=np.zeros_like(A), B=B, Q=Q, R=R, N=N)


@pytest.mark.parametrize("what,status", [("R", 2), ("max_iter", 1), ("newton_max_iter", 3)])
def test_a_failing_unit_has_its_status_and_leaves_its_neighbours_alone(nk, riccati_problems, what, status):
    # the caps hold for every unit of a call: the neighbours are problems that converge within a cap of one
    probs = [_zero_a_problem(5, 1, 3), dict(riccati_problems["f3"]), _zero_a_problem(33, 2, 4)]
    alone = [_build(nk, [q]) for q in probs]
    assert all(r["status"][0] == 0 for r in alone)
    kw = {}
    if what == "R":
        probs[1]["R"] = -np.eye(1)
    else:
        kw = {what: 1}
    res = _build(nk, probs, **kw)
    assert list(res["status"]) == [0, status, 0], res["status"]
    assert _all_nan(res, 1)
    for i in (0, 2):
        for key in ("H", "F", "K", "P"):
            assert not np.any(np.isnan(res[key][i]))
            assert _bits(res[key][i], alone[i][key][0]), (what, i, key)


# ---- 5. bad arguments and guard bands --------------------------------------------------------------------------------------
CANARY = -7.25e77


def _guarded(a, ld=None, pad=5):
    """(buffer, pointer to the first entry, leading dimension): the matrix inside a buffer of canaries, rows `ld` apart."""
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    r, c = a.shape
    ld = c if ld is None else ld
    buf = np.full(pad + r * ld + pad, CANARY)
    view = buf[pad:pad + r * ld].reshape(r, ld)
    view[:, :c] = a
    return buf, buf.ctypes.data + 8 * pad, ld


def _canaries_intact(buf, r, c, ld, pad=5):
    body = buf[pad:pad + r * ld].reshape(r, ld)
    return np.all(buf[:pad] == CANARY) and np.all(buf[pad + r * ld:] == CANARY) and np.all(body[:, c:] == CANARY)


def _raw_call(nk, case, shape, extra_ld=0, **override):
    """One problem through the C entry with every operand and output inside guard bands.  Returns (rc, message, outputs
    dict of arrays, all canaries intact, outputs untouched)."""
    from nys_koop_lqr_amd import _lib
    ctx = nk.get_context()
    m, p, N, nc, Ny = shape
    nv, ny = N * p, nc * Ny
    ops = dict(A=(case["A"], m + extra_ld), B=(case["B"], p + extra_ld), Q=(case["Q"], m + extra_ld),
               R=(case["R"], p + extra_ld), P=(case["P"], m + extra_ld))
    if nc:
        ops["C_rows"] = (case["C_rows"], m + extra_ld)
    g = {k: _guarded(a, ld) for k, (a, ld) in ops.items()}
    outs = dict(out_H=(nv, nv), out_F=(nv, m), out_K=(p, m), out_P=(m, m))
    if nc:
        outs.update(out_G=(ny, nv), out_T=(ny, m))
    o = {k: _guarded(np.full(s, CANARY)) for k, s in outs.items()}
    pr = _lib.MpcBuildProblem()
    pr.m, pr.p, pr.N, pr.nc, pr.Ny = m, p, N, nc, Ny
    for k, ldname in (("A", "lda"), ("B", "ldb"), ("Q", "ldq"), ("R", "ldr"), ("P", "ldp"), ("C_rows", "ldc")):
        if k in g:
            setattr(pr, k, g[k][1])
            setattr(pr, ldname, g[k][2])
    for k in o:
        setattr(pr, k, o[k][1])
    for k, v in override.items():
        setattr(pr, k, v)
    status, iters = (C.c_int32 * 1)(-1), (C.c_int32 * 2)(-1, -1)
    rc = ctx.lib.nk_mpc_build_batch(ctx.handle, C.byref(pr), 1, 1e-13, 40, 1, 1e-15, 60, status, iters)
    msg = ctx.lib.nk_last_error().decode()
    intact = all(_canaries_intact(g[k][0], *np.atleast_2d(ops[k][0]).shape, g[k][2]) for k in g)
    intact = intact and all(np.all(o[k][0][:5] == CANARY) and np.all(o[k][0][-5:] == CANARY) for k in o)
    untouched = all(np.all(o[k][0] == CANARY) for k in o) and status[0] == -1
    arrays = {k[4:]: o[k][0][5:-5].reshape(outs[k]).copy() for k in o}
    return rc, msg, arrays, intact, untouched


def test_bad_arguments_are_refused_with_the_field_named_and_nothing_written(nk, cases):
    import torch
    shape = mr.GPU_SHAPES[1]  # (5, 1, 1, 1, 1)
    case = cases[1]
    dev = torch.zeros(5 * 5, dtype=torch.float64, device="cuda")
    bad = [(dict(N=65), "nv = N p = 65"), (dict(N=0), "N = 0"), (dict(Ny=2), "Ny = 2"), (dict(m=513), "m = 513"),
           (dict(A=dev.data_ptr()), "A must be host"), (dict(Q=None), "Q is null"), (dict(out_F=None), "out_F is null")]
    for override, needle in bad:
        rc, msg, _, intact, untouched = _raw_call(nk, case, shape, **override)
        assert rc == -1, (override, rc)
        assert "problem 0" in msg, msg
        assert needle in msg, (override, msg)
        assert intact and untouched, override


def test_leading_dimensions_do_not_change_the_results_and_guard_bands_hold(nk, cases, together):
    for idx in (3, 5):
        rc, msg, arrays, intact, _ = _raw_call(nk, cases[idx], mr.GPU_SHAPES[idx], extra_ld=3)
        assert rc == 0, msg
        assert intact
        for key in ("H", "F", "K", "P", "G", "T"):
            assert _bits(arrays[key], together[idx][key]), (idx, key)


# ---- 6. models ---------------------------------------------------------------------------------------------------------------
LIMITS = dict(u_min=-0.1, u_max=0.1, du_min=-0.01, du_max=0.01)
ROWS = dict(x_max=[1.5, 0.8], y_horizon=4)
PARTS = ("H", "F", "K", "G", "T")


@pytest.fixture(scope="module")
def duffing_models(nk):
    """Duffing fits at m = 20 and 40, Nystrom (Matern-5/2) and thin-plate spline: [(label, regressor)]."""
    from nys_koop_lqr_amd import harness
    plant = nk.PolynomialSystem.duffing(0.01)
    X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))
    out = []
    for estimator, params in (("nystrom", dict(kernel=nk.KernelWrapper([1.0, 1.0]), gamma=1e-6)),
                              ("spline", dict(gamma=1e-3, state_bounds_params=(1.0, 2.0)))):
        for u in harness.lqr_plan(X, Y, 1, params, (20, 40), (0,), estimator):
            out.append((f"{estimator}-{u['m']}", harness.lqr_fit_unit(X, Y, 1, params, u, estimator)))
    return out


def _host_controller(reg, A, B):
    from types import SimpleNamespace
    twin = SimpleNamespace(A=A, B=B, C=np.asarray(reg.C, dtype=np.float64), n_inputs=1)
    return type(reg).solve_mpc(twin, 8, c=1.0, **LIMITS, **ROWS)


def _chain_controller(nk, reg):
    """The NumPy statements of the device stages, in their order."""
    lqr = nk.lqr
    A, B, C = (np.asarray(a, dtype=np.float64) for a in (reg.A, reg.B, reg.C))
    Q, R = mr.sym(C.T @ C), np.eye(1)
    P0, K0, _, st = lqr.dare_doubling(A, B, Q, R)
    K, P, _, st2 = lqr.dare_newton_smith(A, B, Q, R, K0, steps=1, P=P0)
    assert st == 0 and st2 == 0
    H, F = lqr.mpc_condense_blocked(A, B, Q, R, P, 8)
    G, T = lqr.mpc_condense_outputs(A, B, C[[0, 1]], 8, 4)
    return dict(H=H, F=F, K=K, G=G, T=T, rho=lqr.mpc_default_rho(H))


def test_device_built_controllers_of_fitted_models_meet_the_host_path(nk, duffing_models):
    from nys_koop_lqr_amd import regressors
    singles = []
    for label, reg in duffing_models:
        A, B = np.asarray(reg.A, dtype=np.float64), np.asarray(reg.B, dtype=np.float64)
        host = _host_controller(reg, A, B)
        dev = reg.solve_mpc(8, c=1.0, device=True, **LIMITS, **ROWS)
        singles.append(dev)
        chain = _chain_controller(nk, reg)
        rng = np.random.default_rng(2000 + A.shape[0])
        moved = {k: 0.0 for k in PARTS + ("rho",)}
        for _ in range(3):
            pert = _host_controller(reg, A * (1.0 + 1e-15 * rng.standard_normal(A.shape)),
                                    B * (1.0 + 1e-15 * rng.standard_normal(B.shape)))
            for k in PARTS:
                moved[k] = max(moved[k], mr.err(getattr(pert, k), getattr(host, k)))
            moved["rho"] = max(moved["rho"], abs(pert.rho - host.rho) / host.rho)
        for k in PARTS + ("rho",):
            if k == "rho":
                e, dist = abs(dev.rho - host.rho) / host.rho, abs(chain["rho"] - host.rho) / host.rho
            else:
                e, dist = mr.err(getattr(dev, k), getattr(host, k)), mr.err(chain[k], getattr(host, k))
            bar = max(10.0 * moved[k], dist)
            print(f"{label} {k}: device vs host {e:.3e}; host moves {moved[k]:.3e}, statements vs host {dist:.3e}, bar {bar:.3e}")
            assert e <= bar, (label, k, e, bar)
        for k in ("lo", "hi", "dlo", "dhi", "ylo", "yhi", "ycomp"):
            assert np.array_equal(getattr(dev, k), getattr(host, k)), (label, k)
        assert type(dev) is type(host) and dev.horizon == host.horizon and dev.y_weight == host.y_weight
        assert _bits(dev.H, dev.H.T)
    # all of them in ONE call: every unit bit for bit its own call
    spec = dict(horizon=8, rho=None, x_min=None, y_weight=np.inf, **LIMITS, **ROWS)
    ctrls, status = regressors._mpc_controller_batch([reg for _, reg in duffing_models], 1.0, spec)
    assert np.all(status == 0)
    for got, alone, (label, _) in zip(ctrls, singles, duffing_models):
        for k in PARTS:
            assert _bits(getattr(got, k), getattr(alone, k)), (label, k)
        assert got.rho == alone.rho
    # without rows the plain controller comes back, and a failing build raises as dlqr_device does
    reg = duffing_models[0][1]
    plain = reg.solve_mpc(8, c=1.0, device=True, **LIMITS)
    assert type(plain) is nk.lqr.MPCController and _bits(plain.H, singles[0].H) and _bits(plain.K, singles[0].K)
    with pytest.raises(np.linalg.LinAlgError, match="status 2"):
        reg.solve_mpc(8, c=1.0, R=-np.eye(1), device=True)
    with pytest.raises(ValueError, match="pass c, not Q"):
        reg.solve_mpc(8, Q=np.eye(20), device=True)


# ---- 7. sweep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [False, True], ids=["inputs", "x_max"])
def test_sweep_with_device_built_controllers(nk, rows):
    from nys_koop_lqr_amd import harness
    plant = nk.PolynomialSystem.duffing(0.01)
    X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))
    params = dict(kernel=nk.KernelWrapper([1.0, 1.0]), gamma=1e-6)
    ms, seeds, steps = (20, 40), (0, 1), 50
    x0, ref = np.array([-0.5, 0.0]), np.zeros(2)
    extra = dict(x_max=[np.inf, 0.8]) if rows else {}
    box = dict(horizon=8, iters=20, **LIMITS, **extra)
    dev = harness.lqr_sweep(X, Y, 1, params, ms, seeds, plant, x0, ref, steps, batch=4, workers=2, return_trajectories=True,
                            controller=dict(box, build="device"))
    host = harness.lqr_sweep(X, Y, 1, params, ms, seeds, plant, x0, ref, steps, batch=4, workers=2,
                             controller=dict(box, build="host"))
    assert sorted(dev["timing"]) == sorted(host["timing"]) == ["fit_s", "gain_cpu_s", "gain_wait_s", "loop_s", "total_s"]
    assert dev["timing"]["gain_cpu_s"] == 0.0 and dev["timing"]["gain_wait_s"] > 0.0
    assert ("y_viol_max" in dev) == rows
    for u in harness.lqr_plan(X, Y, 1, params, ms, seeds, "nystrom"):
        si, k = u["si"], u["k"]
        reg = harness.lqr_fit_unit(X, Y, 1, params, u, "nystrom")
        ctl = reg.solve_mpc(8, c=1.0, device=True, **LIMITS, **extra)
        s, c = reg.closed_loop_plant_mpc(ctl, x0, ref, steps, plant, iters=20)
        assert np.array_equal(dev["states"][si, k], s.T) and np.array_equal(dev["controls"][si, k], c.T), (si, k)
        for name in ("J", "u_absmax"):
            e = abs(dev[name][si, k] - host[name][si, k]) / abs(host[name][si, k])
            print(f"[seed {si}, m = {u['m']}] {name}: build='device' vs build='host' {e:.2e}")
            assert e <= 1e-6, (name, si, k, e)
