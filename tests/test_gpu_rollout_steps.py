"""GPU: the lifted recursion z_{t+1} = A z_t + B u_t (+ bias) step by step, on every route and size class.

Every entry of every step of the lifted states and of x = C z (and of u, sse, ssim where they exist) is held against the
extended-precision reference of tests/rollout_reference.py under its derived entry-wise bar; no tolerance is chosen.  The
operators are designed (|| |A| ||_inf <= 1, a cyclic shift keeps the state alive and makes a transposed or shifted operator
visible), so late steps weigh as much as early ones.  Every case asserts the route the library's plan (csrc/nk_chain_plan.h,
mirrored in rollout_reference.py and held equal to it by tests/test_rollout_reference_host.py) gives for the device's compute
unit count, and prints its worst err / bar.

1. recursion through nk_linear_rollout: the register chain (m <= 128, m + p <= 160; one, two and 1024-capped control blocks),
   the multi-workgroup chain in all nine <KPT, NT> instantiations (padding slots, a chunked call, no give-up), the
   matrix-vector step (batches 1 / 8 / 9 / 16, bits of a trajectory do not depend on the batch) and the GEMM per step;
2. the lifted closed loop on all four routes, distinct and shared references;
3. the lift inside the chain kernel: four kernel families, d from 1 to 192, m = 1 / 5 / 128, and a spline model;
4. the fused open-loop score at tiles of 8, 7 and 2 steps with a partial last tile.

Worst err / bar on an MI355X (256 compute units; profiles/rollout_steps.log; 129 passed, none skipped, the give-up counter
moved only under the hook): recursion CHAIN 0.31 (m = 1, where a bar is a few units in the last place; 0.094 across the control
blocks), MW 0.027, STEP 0.022, GEMM 0.052; closed loop 0.15 (x and u; phi is not returned); lift 0.16 on z_0 and 0.044 against
nk_lift under the sum of both bars; score 0.021 (sse) and 1.8e-4 (ssim) of the bound."""
import numpy as np
import pytest

import rollout_reference as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason=R.LONGDOUBLE_SKIP)]
HOOK = "NYSKOOP_CHAIN_MW_TEST_GIVEUP"


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


@pytest.fixture(scope="module")
def num_cu(nk):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def giveups():
    from nys_koop_lqr_amd import _lib
    return _lib.runtime_counters()["chain_giveups"]


def report(section, name, **ratios):
    print(f"\n[rollout-steps] {section} {name}: " + " ".join(f"{k} {v:.3e}" for k, v in ratios.items()))


def check(tag, got, ref, bar):
    r, at = R.worst(got, ref, bar)
    assert r <= 1.0, f"{tag}: err / bar = {r:.3e} at (trajectory, step, entry) {at}"
    return r


# ---------------------------------------------------------------------------------------------------------------------
# 1. recursion
# ---------------------------------------------------------------------------------------------------------------------
_BATCH_MAX = {}
for _c in R.RECURSION_CASES:
    _k = (_c.m, _c.p)
    _BATCH_MAX[_k] = max(_BATCH_MAX.get(_k, (0, 0))[0], _c.T), max(_BATCH_MAX.get(_k, (0, 0))[1], _c.batch)


def run_recursion(nk, num_cu, c, monkeypatch=None):
    """One call of nk_linear_rollout for case c; returns (worst Z ratio, worst x ratio, Z)."""
    q = R.recursion_problem(c.m, c.p, *_BATCH_MAX[(c.m, c.p)])
    first, repeat = R.case_plans(c, num_cu)
    if c.hook:
        assert first.route == R.MW and repeat.route == c.route, (c.name, first, repeat)
        monkeypatch.setenv(HOOK, "1")
    else:
        assert R.claimed_plan_matches(c, first), (c.name, first)
    before = giveups()
    x, Z = nk.linear_rollout(q["A"], q["B"], q["C"], q["z0"][:c.batch], q["U"][:c.batch, :c.T], return_lifted=True)
    moved = giveups() - before
    if c.hook:
        monkeypatch.delenv(HOOK)
    assert Z.shape == (c.batch, c.T, c.m) and x.shape == (c.batch, c.T, R.D_OUT)
    assert np.array_equal(Z[:, 0], q["z0"][:c.batch])
    rz = check(c.name + " Z", Z, q["Z"][:c.batch, :c.T], q["bar"][:c.batch, :c.T])
    rx = check(c.name + " x", x, q["x"][:c.batch, :c.T], q["bar_x"][:c.batch, :c.T])
    if c.hook:
        assert moved == 1, (c.name, moved)
    elif moved:  # the answer above is the repeat's and has passed; the route under test was not the one that produced it
        pytest.skip(f"{c.name}: the multi-workgroup recursion gave up ({moved} give-up(s)): the stepwise repeat was checked")
    return rz, rx, Z


@pytest.mark.parametrize("m,p", R.CHAIN_SHAPES, ids=lambda v: None)
def test_register_chain(nk, num_cu, m, p):
    worst = 0.0
    for c in R.CHAIN_CASES:
        if (c.m, c.p) == (m, p):
            rz, rx, Z = run_recursion(nk, num_cu, c)
            worst = max(worst, rz, rx)
            if c.batch > 1:  # a trajectory of a batch has the bits it has alone
                q = R.recursion_problem(m, p, *_BATCH_MAX[(m, p)])
                _, Z1 = nk.linear_rollout(q["A"], q["B"], q["C"], q["z0"][2:3], q["U"][2:3, :c.T], return_lifted=True)
                assert np.array_equal(Z1[0], Z[2]), c.name
    report("recursion CHAIN", f"m{m}-p{p} (T 1/2/3/40, batch 1/3)", worst=worst)


@pytest.mark.parametrize("c", R.BLOCK_CASES, ids=R._name)
def test_register_chain_control_blocks(nk, num_cu, c):
    plan, _ = R.case_plans(c, num_cu)
    assert plan.blocks == 2 and plan.tb == {238: 236, 240: 236, 1030: 1024}[c.T]
    rz, rx, _ = run_recursion(nk, num_cu, c)
    report("recursion CHAIN", c.name, Z=rz, x=rx)


@pytest.mark.parametrize("c", R.MW_CASES, ids=R._name)
def test_multi_workgroup_chain(nk, num_cu, c):
    rz, rx, _ = run_recursion(nk, num_cu, c)
    report("recursion MW", c.name, Z=rz, x=rx)


@pytest.mark.parametrize("c", R.STEP_CASES + R.GEMM_CASES, ids=R._name)
def test_one_launch_per_step(nk, num_cu, c, monkeypatch):
    rz, rx, Z = run_recursion(nk, num_cu, c, monkeypatch)
    if c.route == R.STEP and c.batch > 1:  # a batch gives each trajectory the bits it gets alone
        q = R.recursion_problem(c.m, c.p, *_BATCH_MAX[(c.m, c.p)])
        for b in (0, c.batch - 1):
            if c.hook:
                monkeypatch.setenv(HOOK, "1")
            _, Z1 = nk.linear_rollout(q["A"], q["B"], q["C"], q["z0"][b:b + 1], q["U"][b:b + 1, :c.T], return_lifted=True)
            if c.hook:
                monkeypatch.delenv(HOOK)
            assert R.chain_plan(c.m, c.p, 0, c.T, 1, num_cu, mw_allowed=not c.hook).route == R.STEP
            assert np.array_equal(Z1[0], Z[b]), (c.name, b)
    report(f"recursion {c.route}", c.name, Z=rz, x=rx)


# ---------------------------------------------------------------------------------------------------------------------
# models with designed operators
# ---------------------------------------------------------------------------------------------------------------------
def rbf(nk, ls):
    """A wrapper like ThreeDimensionalKernel around an RBF with the given length scale(s)."""
    import types
    from nys_koop_lqr_amd import _lib
    return types.SimpleNamespace(kernel=nk.kernels.DeviceKernel(_lib.NK_KERNEL_RBF, ls))


def designed_model(nk, kernel, Zl, p, A, B, C, seed=0):
    """A Nystrom model with landmarks Zl (m x d): a small fit, then the designed operators are assigned."""
    m, d = Zl.shape
    rng = np.random.default_rng([m, d, p, seed])
    n = m + 40
    S = Zl[rng.integers(m, size=n)] + 0.1 * rng.standard_normal((n, d))
    Uin = rng.standard_normal((n, p))
    Y = 0.9 * S + 0.05 * rng.standard_normal((n, d))
    reg = nk.KoopmanNystromRegressor(p, kernel=kernel, gamma=1e-4, m=m)
    reg.nystrom_centers_output = np.ascontiguousarray(Zl.T)
    reg.fit(np.hstack([S, Uin]), Y)
    reg.A, reg.B, reg.C = A, B, C
    return reg


def model_sinv(reg):
    from nys_koop_lqr_amd import _lib
    ctx = _lib.get_context()
    m = reg._landmark_shape()[1]
    Si = np.empty((m, m))
    _lib.check(ctx.lib.nk_model_get(ctx.handle, reg._ensure_model(), b"I", Si.ctypes.data, m))
    return Si


# ---------------------------------------------------------------------------------------------------------------------
# 2. closed loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_models(nk):
    cache = {}

    def get(m):
        if m not in cache:
            A, B, C = R.design(m, R.LOOP_P, R.LOOP_D, row=0.8, brow=0.2)
            Zl = R.lattice_landmarks(m, R.LOOP_D)
            cache[m] = (designed_model(nk, rbf(nk, R.LATTICE_LS), Zl, R.LOOP_P, A, B, C), A, B, C, R.gain(m, R.LOOP_P))
        return cache[m]
    return get


@pytest.mark.parametrize("c", R.LOOP_CASES, ids=R._name)
def test_closed_loop(nk, num_cu, loop_models, monkeypatch, c):
    reg, A, B, C, K = loop_models(c.m)
    first = R.chain_plan(c.m, 0, 0, c.steps, c.batch, num_cu, per_trajectory_bias=True)
    last = R.chain_plan(c.m, 0, 0, c.steps, c.batch, num_cu, per_trajectory_bias=True, mw_allowed=False) if c.hook else first
    assert last.route == c.route and (not c.hook or first.route == R.MW), (c, first, last)
    phi0, _ = R.inputs(c.m, 0, c.steps, c.batch, seed=1)
    refs, _ = R.inputs(c.m, 0, c.steps, c.batch, seed=2)
    worst = {}
    for tag, ref in (("distinct", refs), ("shared", refs[:1])):
        want = R.closed_loop_ld(A, B, C, K, phi0, ref, c.steps)
        if c.hook:
            monkeypatch.setenv(HOOK, "1")
        before = giveups()
        xs, us = reg.closed_loop(K, phi0, ref, c.steps)
        moved = giveups() - before
        if c.hook:
            monkeypatch.delenv(HOOK)
        assert xs.shape == (c.batch, c.steps, R.LOOP_D) and us.shape == (c.batch, c.steps, R.LOOP_P)
        worst[f"x-{tag}"] = check(f"{c.name} {tag} x", xs, want["x"], want["bar_x"])
        worst[f"u-{tag}"] = check(f"{c.name} {tag} u", us, want["u"], want["bar_u"])
        if c.hook:
            assert moved == 1, (c.name, moved)
        elif moved:
            pytest.skip(f"{c.name}: the multi-workgroup recursion gave up ({moved}): the stepwise repeat was checked")
    report("closed loop", c.name, **worst)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the lift inside the chain kernel
# ---------------------------------------------------------------------------------------------------------------------
def lift_kernel(nk, tag, d):
    family, aniso = R.LIFT_FAMILIES[tag]
    fam, par = R.G.kernel_spec(family, d, aniso)
    if fam == R.LINEAR:
        return fam, par, nk.LinearKernelWrapper(par)
    if fam == R.MATERN:
        return fam, par, nk.KernelWrapper(np.asarray(par))
    return fam, par, rbf(nk, np.asarray(par))


@pytest.mark.parametrize("tag", sorted(R.LIFT_FAMILIES))
@pytest.mark.parametrize("d", R.LIFT_D)
def test_lift_in_the_chain_kernel(nk, num_cu, tag, d):
    worst = dict(z0=0.0, Z=0.0, x=0.0, api=0.0)
    for m in R.LIFT_M:
        fam, par, kern = lift_kernel(nk, tag, d)
        rng = np.random.default_rng([d, m, len(tag)])
        Zl = rng.standard_normal((m, d))
        # one state next to a landmark (cancellation in the differences), the others anywhere
        x0 = np.vstack([Zl[:1] + 0.05 * rng.standard_normal((1, d)), rng.standard_normal((R.LIFT_BATCH - 1, d))])
        A, B, _ = R.design(m, R.LIFT_P, R.D_OUT)
        C = rng.standard_normal((d, m)) / np.sqrt(m)
        reg = designed_model(nk, kern, Zl, R.LIFT_P, A, B, C)
        Sinv = model_sinv(reg)
        want = R.lift_ld(x0, Zl, par, fam, Sinv, center=np.zeros(d) if fam == R.LINEAR else Zl.mean(axis=0))
        api = reg.lift(x0.T).T
        for T in R.LIFT_T:
            plan = R.chain_plan(m, R.LIFT_P, d, T, R.LIFT_BATCH, num_cu)
            assert plan.route == R.CHAIN and plan.lift_in_kernel, (m, d, T, plan)
            _, U = R.inputs(m, R.LIFT_P, T, R.LIFT_BATCH)
            x, Z = reg.rollout(x0, U, return_lifted=True)
            name = f"lift {tag} d{d} m{m} T{T}"
            worst["z0"] = max(worst["z0"], check(name + " z0", Z[:, 0], want["z0"], want["bar"]))
            worst["api"] = max(worst["api"], check(name + " against nk_lift", Z[:, 0], api, want["bar"] + want["bar_api"]))
            Zr, bar = R.recursion_ld(A, B, want["z0"], U, b0=want["bar"])
            xr, bar_x = R.output_ld(C, Zr, bar)
            worst["Z"] = max(worst["Z"], check(name + " Z", Z, Zr, bar))
            worst["x"] = max(worst["x"], check(name + " x", x, xr, bar_x))
    report("lift", f"{tag} d{d} (m 1/5/128, T 1/5)", **worst)


def test_spline_model_lifts_outside_the_chain_kernel(nk, num_cu):
    """A spline model at m = 100: nk_lift's code writes z_0 into row 0 of the trajectory and the chain kernel reads it there."""
    m, d, p, T, batch = 100, 2, 1, 20, 3
    rng = np.random.default_rng(5)
    cen = rng.uniform(-1.0, 1.0, (m, d))
    n = 300
    S = rng.uniform(-1.0, 1.0, (n, d))
    Uin = rng.standard_normal((n, p))
    reg = nk.KoopmanSplineRegressor(p, m=m, gamma=1e-6)
    reg.centers = np.ascontiguousarray(cen.T)
    reg.fit(np.hstack([S, Uin]), 0.9 * S + 0.1 * Uin)
    A, B, _ = R.design(m, p, d)
    C = rng.standard_normal((d, m)) / np.sqrt(m)
    reg.A, reg.B, reg.C = A, B, C
    plan = R.chain_plan(m, p, 0, T, batch, num_cu)  # (no kernel lift for a spline model: d_lift = 0)
    assert plan.route == R.CHAIN and not plan.lift_in_kernel
    x0 = rng.uniform(-1.0, 1.0, (batch, d))
    _, U = R.inputs(m, p, T, batch)
    x, Z = reg.rollout(x0, U, return_lifted=True)
    assert np.array_equal(Z[:, 0], reg.lift(x0.T).T)
    Zr, bar = R.recursion_ld(A, B, Z[:, 0], U)
    xr, bar_x = R.output_ld(C, Zr, bar)
    report("lift", "spline m100 d2 T20", Z=check("spline Z", Z, Zr, bar), x=check("spline x", x, xr, bar_x))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the fused score
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", sorted(R.SCORE_M))
@pytest.mark.parametrize("d", R.SCORE_D)
def test_fused_score_tiles(nk, num_cu, monkeypatch, m, d):
    """The score walks the matrix-vector steps (batch invariant) and reduces x_true - C z in tiles of 8, 7 or 2 steps; T = 11
    leaves a partial last tile.  The lifted states it is compared with come from the same steps: a rollout that is made to
    repeat stepwise, 16 trajectories at a time."""
    T, p, k = R.SCORE_T, R.SCORE_P, max(R.SCORE_BATCH)
    assert R.traj_err_tile(m) == R.SCORE_M[m] and T % R.SCORE_M[m] != 0
    A, B, _ = R.design(m, p, R.D_OUT)
    rng = np.random.default_rng([m, d, 3])
    C = rng.standard_normal((d, m)) / np.sqrt(m)
    Zl = R.lattice_landmarks(m, d)
    reg = designed_model(nk, rbf(nk, R.LATTICE_LS), Zl, p, A, B, C)
    trajs = rng.standard_normal((k, d, T)) * 0.5
    trajs[:, :, 0] = Zl[rng.integers(m, size=k)] + 0.1 * rng.standard_normal((k, d))
    ctrls = rng.standard_normal((k, p, T - 1))
    from nys_koop_lqr_amd.regressors import open_loop_pack
    tr, U = open_loop_pack(trajs, ctrls, d, p)
    monkeypatch.setenv(HOOK, "1")
    Z = np.concatenate([reg.rollout(np.ascontiguousarray(tr[b:b + 16, 0, :]), U[b:b + 16], return_lifted=True)[1]
                        for b in range(0, k, 16)])
    monkeypatch.delenv(HOOK)
    sse, ssim, b_sse, b_ssim = R.score_reference(Z, C, tr)
    assert np.all(sse > 0) and np.all(ssim > 0)
    got = {}
    for nb in R.SCORE_BATCH:
        plan = R.chain_plan(m, p, 0, T, nb, num_cu, batch_invariant=True)
        assert plan.route == R.STEP, plan
        got[nb] = (reg.open_loop_errors(trajs[:nb], ctrls[:nb]), reg.open_loop_errors(trajs[:nb], ctrls[:nb], relative=True))
        assert np.all(np.isfinite(got[nb][0])) and np.all(np.isfinite(got[nb][1]))
    sse_dev, ssim_dev = R.score_sums(got[k][0], got[k][1], d, T)
    r_sse, r_ssim = np.abs(sse_dev - sse) / b_sse, np.abs(ssim_dev - ssim) / b_ssim
    report("score", f"m{m} d{d} T{T} tile{R.SCORE_M[m]}", sse=float(r_sse.max()), ssim=float(r_ssim.max()))
    assert np.all(r_sse <= 1.0), r_sse
    assert np.all(r_ssim <= 1.0), r_ssim
    assert got[1][0][0] == got[k][0][0] and got[1][1][0] == got[k][1][0]  # trajectory 0 does not feel the batch
