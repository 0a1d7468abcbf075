"""GPU: the one-call multi-seed system-identification sweep (nk_sysid_grid) and its device-side score (nk_rollout_err).

1. the fused score against the unfused formula on the same lifted states, inside a bound derived from the arithmetic;
2. one call equals the plain loop bit for bit (Nystrom, spline, a mixed call, a failing unit);
3. parity with the reference through the bars the fixtures carry, no unit left out;
4. the cloth protocol (per-seed shuffle, training set as row ranges of one data set, the discarded second draw);
5. the lock-step counters show merged launches."""
import numpy as np
import pytest

from rollout_reference import score_reference, score_sums

pytestmark = pytest.mark.gpu
NK_ERR_BAD_ARG = -1


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


# ---------------------------------------------------------------------------------------------------------------
# 1. fused score vs the unfused formula
# ---------------------------------------------------------------------------------------------------------------
def synthetic(nk, m, seed=0):
    """A small controlled system with d = 7 states (more rows of C than the error kernel has waves, and an odd count),
    p = 2 inputs and T = 37 steps (not a multiple of the kernel's 8-step tiles)."""
    rng = np.random.default_rng(seed)
    n, d, p, T, k = 900, 7, 2, 37, 17
    S = rng.standard_normal((n, d))
    U = rng.standard_normal((n, p))
    Y = np.tanh(S @ (rng.standard_normal((d, d)) * 0.9 / np.sqrt(d))) + U @ (rng.standard_normal((p, d)) * 0.1)
    X = np.hstack([S, U])
    idx = rng.choice(n, m, replace=False)
    trajs = rng.standard_normal((k, d, T)) * 0.5
    ctrls = rng.standard_normal((k, p, T - 1))

    def make():
        reg = nk.KoopmanNystromRegressor(p, kernel=nk.ThreeDimensionalKernel(3.0, 3.0, 3.0, d), gamma=1e-4, m=m)
        reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, idx])
        reg.fit(X, Y)
        return reg
    return make, trajs, ctrls


def duffing_spline(nk, golden, m=48):
    g12, f = golden("f12_duffing_full.npz"), golden("f15_spline_duffing.npz")
    X, Y = np.ascontiguousarray(g12["X"]), np.ascontiguousarray(g12["Y"])
    k = list(f["ms"]).index(m)
    o = int(np.sum(f["ms"][:k]))
    trajs = np.stack([g12[f"traj_{i % 8}"] * (1.0 + 0.01 * (i // 8)) for i in range(17)])
    ctrls = np.stack([g12[f"ctrl_{i % 8}"] for i in range(17)])

    def make():
        reg = nk.KoopmanSplineRegressor(1, state_bounds_params=f["bounds"], m=m, gamma=float(f["gamma"]))
        reg.centers = np.ascontiguousarray(f["centers_0"][:, o:o + m])
        reg.fit(X, Y)
        return reg
    return make, trajs, ctrls


def measure(reg, trajs, ctrls):
    """Lifted states of the plain rollout, C, and the fused errors for batches of 1, 3 and 17 -- all on the calling
    thread's context."""
    from nys_koop_lqr_amd.regressors import open_loop_pack
    d, p = trajs.shape[1], ctrls.shape[1]
    tr, U = open_loop_pack(trajs, ctrls, d, p)
    # (16 at a time: beyond that a stepwise rollout advances the batch with a GEMM per step, the score never does)
    Z = np.concatenate([reg.rollout(np.ascontiguousarray(tr[b:b + 16, 0, :]), U[b:b + 16], return_lifted=True)[1]
                        for b in range(0, tr.shape[0], 16)])
    out = dict(Z=Z, C=np.array(reg.C))
    for nb in (1, 3, 17):
        out[f"abs{nb}"] = reg.open_loop_errors(trajs[:nb], ctrls[:nb])
        out[f"rel{nb}"] = reg.open_loop_errors(trajs[:nb], ctrls[:nb], relative=True)
    return out


def check_fused(tag, got, trajs):
    """|d sse| <= 2 sqrt(sse) |e| + |e|^2 + gamma_{dT} sse with e = gamma_{m+2} (|C| |z|) entry by entry: the device forms
    each entry of C z as a sum of m products (any order: at most m + 2 roundings on a path with the final subtraction),
    squares and adds dT of them (any order: at most dT roundings on a path).  Same for ssim with sqrt(ssim).  The device
    hands back sqrt(sse / dT) and 100 sqrt(sse) / sqrt(ssim): recovering the two sums from them costs a square root, a
    division, a square and a product each (gamma_8 on sse; ssim is recovered from both numbers: gamma_16).  The host side
    of the comparison is evaluated in extended precision from the same lifted states, so it adds nothing.  The bound itself
    is rollout_reference.score_reference (shared with test_gpu_rollout_steps.py)."""
    Z, C = got["Z"], got["C"]
    k, T, m = Z.shape
    d = C.shape[0]
    sse, ssim, bound_sse, bound_ssim = score_reference(Z, C, np.transpose(trajs, (0, 2, 1)))
    assert np.all(np.isfinite(got["abs17"])) and np.all(np.isfinite(got["rel17"]))
    sse_dev, ssim_dev = score_sums(got["abs17"], got["rel17"], d, T)
    r_sse, r_ssim = np.abs(sse_dev - sse) / bound_sse, np.abs(ssim_dev - ssim) / bound_ssim
    print(f"\n[{tag}] m = {m}, d = {d}, T = {T}: |d sse| / bound max {float(r_sse.max()):.3e}, |d ssim| / bound max "
          f"{float(r_ssim.max()):.3e}; rel. deviation of sse max {float((np.abs(sse_dev - sse) / sse).max()):.2e}")
    assert np.all(r_sse <= 1.0), r_sse
    assert np.all(r_ssim <= 1.0), r_ssim
    # and the formulas of validate_dyn_sys themselves, loosely (they are the same quantities)
    np.testing.assert_allclose(got["abs17"], np.sqrt(np.asarray(sse / (d * T), dtype=np.float64)), rtol=1e-9)
    np.testing.assert_allclose(got["rel17"], 100 * np.sqrt(np.asarray(sse / ssim, dtype=np.float64)), rtol=1e-9)
    # trajectory b does not feel the batch
    for key in ("abs", "rel"):
        assert got[f"{key}1"][0] == got[f"{key}3"][0] == got[f"{key}17"][0], key
        assert np.array_equal(got[f"{key}3"], got[f"{key}17"][:3]), key


def test_fused_score_single_launch_recursion(nk):
    make, trajs, ctrls = synthetic(nk, 48)
    check_fused("nystrom m=48", measure(make(), trajs, ctrls), trajs)


def test_fused_score_spline_model(nk, golden):
    make, trajs, ctrls = duffing_spline(nk, golden)
    check_fused("spline m=48", measure(make(), trajs, ctrls), trajs)


def test_fused_score_stepwise_recursion_and_member_context(nk):
    """m = 200: beyond the single-launch chain the score walks the matrix-vector steps -- the recursion a lock-step member
    runs -- so the lifted states it is compared with are those of a rollout on a member context (fit, rollout and score
    inside one unit of a one-member group).  An ordinary context must return the member's bits."""
    from nys_koop_lqr_amd import _lib
    make, trajs, ctrls = synthetic(nk, 200)
    pool = _lib.lockstep_pool(1, index=7)
    member = pool.run_round(lambda _: measure(make(), trajs, ctrls), [0])[0]
    check_fused("nystrom m=200 (member)", member, trajs)
    reg = make()
    for nb in (1, 3, 17):
        assert np.array_equal(reg.open_loop_errors(trajs[:nb], ctrls[:nb]), member[f"abs{nb}"]), nb
        assert np.array_equal(reg.open_loop_errors(trajs[:nb], ctrls[:nb], relative=True), member[f"rel{nb}"]), nb
    # against the host formula on the ordinary context's own rollout (other recursion kernel: rounding-level agreement)
    from nys_koop_lqr_amd import harness
    want = harness.validate_dyn_sys_all(reg, trajs, ctrls)
    np.testing.assert_allclose(member["abs17"], want, rtol=1e-9)


# ---------------------------------------------------------------------------------------------------------------
# 2 + 3 + 5. Duffing at the reference's shape: one call = the loop, parity bars, group counters
# ---------------------------------------------------------------------------------------------------------------
def duffing_args(nk, golden, estimator):
    g = golden("f12_duffing_full.npz")
    X, Y = np.ascontiguousarray(g["X"]), np.ascontiguousarray(g["Y"])
    if estimator == "nystrom":
        seeds = [int(s) for s in g["seeds"]]
        params = dict(kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"]))
        src, ms, centers = g, g["ms"], None
    else:
        f = golden("f15_spline_duffing.npz")
        seeds = [int(s) for s in f["seeds"]][:3]
        params = dict(gamma=float(f["gamma"]), state_bounds_params=f["bounds"])
        src, ms = f, f["ms"]
        offs = np.concatenate(([0], np.cumsum(ms)))
        centers = {(s, 0, k): f[f"centers_{s}"][:, offs[k]:offs[k + 1]] for s in seeds for k in range(len(ms))}
    trajs = np.stack([src[f"traj_{s}"] for s in seeds])
    ctrls = np.stack([src[f"ctrl_{s}"] for s in seeds])
    return dict(X=X, Y=Y, n_inputs=1, params=params, ms=ms, seeds=seeds, trajs=trajs, controls=ctrls,
                test_index=[[i] for i in range(len(seeds))], estimator=estimator, relative=True, centers=centers)


@pytest.fixture(scope="module")
def duffing_tables(nk, golden):
    from nys_koop_lqr_amd import harness, _lib
    out = {}
    for est in ("nystrom", "spline"):
        a = duffing_args(nk, golden, est)
        out[est, 0] = harness.sysid_sweep(batch=0, **a)
        before = _lib.lockstep_pool(3).stats()
        out[est, 3] = harness.sysid_sweep(batch=3, **a)
        after = _lib.lockstep_pool(3).stats()
        out[est, "stats"] = {k: after[k] - before[k] for k in after}
        out[est, 8] = harness.sysid_sweep(batch=8, **a)
    return out


@pytest.mark.parametrize("estimator", ["nystrom", "spline"])
def test_duffing_one_call_equals_the_loop(duffing_tables, estimator):
    t0, t3, t8 = (duffing_tables[estimator, b] for b in (0, 3, 8))
    assert t0.shape == (3, 1, 20) and np.all(np.isfinite(t0))
    assert np.array_equal(t3, t0)
    assert np.array_equal(t8, t0)


def test_duffing_nystrom_sweep_parity_with_reference(duffing_tables, golden):
    """Fit by fit inside max(10 spread, 10 roworder, 3 envelope, 1e-8): formula and constants of the project's existing
    Duffing replay; no unit is left out."""
    g, e12 = golden("f12_duffing_full.npz"), golden("f12b_duffing_envelope.npz")
    K_BAR, K_ENV, FLOOR = 10.0, 3.0, 1e-8
    ref, refp = g["ref_rmse"], g["ref_rmse_perturbed"]
    spread = np.abs(refp - ref) / ref
    envelope, roworder = e12["envelope"], e12["roworder"]
    got = duffing_tables["nystrom", 3][:, 0, :]
    worst, over = 0.0, []
    for si in range(3):
        for k in range(20):
            err = abs(got[si, k] - ref[si, k]) / ref[si, k]
            bar = max(K_BAR * spread[si, k], K_BAR * roworder[si, k], K_ENV * envelope[si, k], FLOOR)
            worst = max(worst, err / bar)
            if err > bar:
                over.append((si, k, got[si, k], ref[si, k], err, bar))
    print(f"\nduffing sweep in one call: worst err / bar = {worst:.3f}")
    assert not over, over


def test_duffing_spline_sweep_parity_with_reference(duffing_tables, golden):
    f = golden("f15_spline_duffing.npz")
    got = duffing_tables["spline", 3][:, 0, :]
    ref, bar = f["ref_rmse"][:3], f["bar_rmse"][:3]
    rel = np.abs(got - ref) / ref
    print(f"\nspline duffing sweep in one call: worst err / bar = {(rel / bar).max():.3f}")
    assert np.all(rel <= bar), np.argwhere(rel > bar)


def test_group_counters_show_merged_launches(duffing_tables):
    for est in ("nystrom", "spline"):
        st = duffing_tables[est, "stats"]
        print(f"\n[{est}] lock-step counters of the 60-unit call, 3 members: {st}")
        assert st["merged_launches"] > 0 and st["member_launches_merged"] >= 2 * st["merged_launches"]


def test_mixed_call_and_failing_unit(nk, golden):
    """Nystrom and spline units in one nk_sysid_grid call, with one unit whose gamma is not a number: that unit is NaN with
    NK_ERR_BAD_ARG, every other entry carries the bits of the plain loop."""
    from nys_koop_lqr_amd import harness, _lib
    from nys_koop_lqr_amd.regressors import open_loop_pack
    an, asp = duffing_args(nk, golden, "nystrom"), duffing_args(nk, golden, "spline")
    plan_n = harness.sysid_plan(an["X"], an["Y"], 1, an["params"], an["ms"], an["seeds"], an["test_index"])
    plan_s = harness.sysid_plan(asp["X"], asp["Y"], 1, asp["params"], asp["ms"], asp["seeds"], asp["test_index"],
                                estimator="spline", centers=asp["centers"])
    pick_n = [u for u in plan_n if u["k"] in (0, 7, 19) and u["si"] < 2]
    pick_s = [u for u in plan_s if u["k"] in (0, 7, 12) and u["si"] < 2]
    tr, U = open_loop_pack(an["trajs"], an["controls"], 2, 1)
    np.testing.assert_array_equal(an["trajs"], asp["trajs"])  # seeds 0..2: the same test trajectories in both fixtures
    tn = harness.sysid_grid_units(an["params"], pick_n, "nystrom")
    ts = harness.sysid_grid_units(asp["params"], pick_s, "spline")
    units, kinds = [], []
    for a, b in zip(tn, ts):
        units += [a, b]
        kinds += ["nystrom", "spline"]
    bad = list(tn[1])
    bad[1] = float("nan")
    units.insert(3, tuple(bad))
    kinds.insert(3, "bad")
    # unit 0 scores two trajectories, to exercise the prefix-sum layout and the gather of non-consecutive trajectories
    u0 = list(units[0])
    u0[6] = [2, 0]
    units[0] = tuple(u0)
    ea, er, status, offs = _lib.lockstep_pool(4).sysid_grid(an["X"], an["Y"], 1, tr, U, units)
    assert offs.tolist() == [0, 2] + list(range(3, len(units) + 2))
    picks = iter(zip(pick_n, pick_s))
    flat = []
    for a, b in picks:
        flat += [("nystrom", a), ("spline", b)]
    flat.insert(3, ("bad", None))
    for i, (kind, u) in enumerate(flat):
        lo = int(offs[i])
        if kind == "bad":
            assert status[i] == NK_ERR_BAD_ARG and np.isnan(ea[lo]) and np.isnan(er[lo])
            continue
        assert status[i] == 0, (i, status[i])
        par = an["params"] if kind == "nystrom" else asp["params"]
        trajs_u = [2, 0] if i == 0 else [u["traj"]]
        for j, t in enumerate(trajs_u):
            uu = dict(u, traj=t)
            assert ea[lo + j] == harness.sysid_unit_error(an["X"], an["Y"], 1, par, uu, tr, U, kind, False), (i, j)
            assert er[lo + j] == harness.sysid_unit_error(an["X"], an["Y"], 1, par, uu, tr, U, kind, True), (i, j)


# ---------------------------------------------------------------------------------------------------------------
# 4. cloth: seed 0 of the reference's validation loop in one call
# ---------------------------------------------------------------------------------------------------------------
def test_cloth_seed0_in_one_call(nk, golden):
    """Seed 0 of benchmark_lqr_cloth.py:168-203 with RBF l = 10, gamma = 1e-7: the trajectory shuffle, 10 test
    trajectories x 20 values of m, one landmark draw per fit plus the discarded second draw (the code version that wrote
    the shipped CSV drew the input centres separately).  The data set holds all 40 trajectories once; a seed trains on 30
    row ranges of it, in the shuffle's order.  Rows 0-2 against the shipped values under the bars of the existing
    replay, and bit for bit against the plain loop; rows 3-9 have no per-entry bar in the fixtures: printed only."""
    from nys_koop_lqr_amd import harness
    g = golden("f10_lqr_control.npz")
    t = golden("cloth_trajs_all.npz")
    states = t["states_e10"] / 1e10
    trajs = np.stack([states[i] for i in range(10, 50)])
    ctrls = np.stack([t["inputs"][i] for i in range(10, 50)])
    T = trajs.shape[2]
    ms = np.logspace(1.0, 2.6, num=20, dtype=int)
    shipped = g["all_rmses"]
    Xa, Ya = harness.create_data_matrices(list(trajs), list(ctrls), range(40))
    X, Y = np.ascontiguousarray(Xa.T), np.ascontiguousarray(Ya.T)
    params = dict(kernel=nk.ThreeDimensionalKernel(10, 10, 10, 192), gamma=1e-7)

    def protocol():
        rs = np.random.RandomState(0)
        order = np.arange(40)
        rs.shuffle(order)
        train, test = order[:30], order[30:]
        ranges = [(int(i) * (T - 1), (int(i) + 1) * (T - 1)) for i in train]
        return rs, ranges, [int(i) for i in test]

    rs, ranges, test = protocol()
    # the training matrix the fit gathers from the ranges is the reference's own, row for row
    Xr, Yr = harness.create_data_matrices(list(trajs), list(ctrls), [r[0] // (T - 1) for r in ranges])
    np.testing.assert_array_equal(Y[harness.train_row_map(ranges, Y.shape[0])], Yr.T)
    full = harness.sysid_sweep(X, Y, 6, params, ms, [0], trajs, ctrls, {0: test}, train_ranges={0: ranges}, extra_draws=1,
                               batch=8, streams={0: rs})
    assert full.shape == (1, 10, 20)
    assert np.all(np.isfinite(full)), np.argwhere(~np.isfinite(full))  # (a failed unit would be NaN: status != 0)
    rs, ranges, test = protocol()
    loop = harness.sysid_sweep(X, Y, 6, params, ms, [0], trajs, ctrls, {0: test[:3]}, train_ranges={0: ranges},
                               extra_draws=1, batch=0, streams={0: rs})
    rows = full[0, :3]
    assert np.array_equal(rows, loop[0])
    rel = np.abs(rows - shipped[:3]) / shipped[:3]
    print("\n[cloth seed 0, one call] relative error of the open-loop RMSE vs the shipped CSV, rows 0-2: median %.1e, "
          "max %.1e; by m: %s" % (np.median(rel), rel.max(), np.array2string(rel.max(axis=0), precision=1)))
    rest = np.abs(full[0, 3:] - shipped[3:10]) / shipped[3:10]
    print("[cloth seed 0, one call] rows 3-9 (not asserted): median %.1e, max %.1e; by m: %s"
          % (np.median(rest), rest.max(), np.array2string(rest.max(axis=0), precision=1)))
    assert np.median(rel) < 1e-3 and rel.max() < 5e-2
    assert rel[:, :8].max() < 1e-4  # m <= 38: well conditioned


def test_cloth_units_report_status_zero(nk, golden):
    """The statuses themselves, straight from the library call, for one test trajectory of the cloth seed (20 units)."""
    from nys_koop_lqr_amd import harness, _lib
    from nys_koop_lqr_amd.regressors import open_loop_pack
    t = golden("cloth_trajs_all.npz")
    states = t["states_e10"] / 1e10
    trajs = np.stack([states[i] for i in range(10, 50)])
    ctrls = np.stack([t["inputs"][i] for i in range(10, 50)])
    T = trajs.shape[2]
    ms = np.logspace(1.0, 2.6, num=20, dtype=int)
    Xa, Ya = harness.create_data_matrices(list(trajs), list(ctrls), range(40))
    X, Y = np.ascontiguousarray(Xa.T), np.ascontiguousarray(Ya.T)
    params = dict(kernel=nk.ThreeDimensionalKernel(10, 10, 10, 192), gamma=1e-7)
    rs = np.random.RandomState(0)
    order = np.arange(40)
    rs.shuffle(order)
    ranges = [(int(i) * (T - 1), (int(i) + 1) * (T - 1)) for i in order[:30]]
    units = harness.sysid_plan(X, Y, 6, params, ms, [0], {0: [int(i) for i in order[30:]]}, {0: ranges}, extra_draws=1,
                               streams={0: rs})
    assert len(units) == 200
    tr, U = open_loop_pack(trajs, ctrls, 192, 6)
    ea, er, status, offs = _lib.lockstep_pool(8).sysid_grid(X, Y, 6, tr, U, harness.sysid_grid_units(params, units))
    assert np.all(status == 0), status
    assert np.all(np.isfinite(ea)) and np.all(np.isfinite(er)) and offs[-1] == 200
