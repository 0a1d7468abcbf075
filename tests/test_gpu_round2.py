"""GPU parity tests added in round 2: the rank-truncating fallback of the regularised solves (gelsd semantics,
regressors.py:155,165), sweep robustness, the single-launch lifted recursion (rollout / closed loop, batched), rollouts of
explicit operators, the full lqr_control of benchmark_lqr_cloth.py:69-104, stream ordering for device-tensor inputs and
deterministic teardown.  All calls go through the C-ABI (ctypes)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import relf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


@pytest.fixture(scope="module")
def O():
    from oracle import nk_oracle
    return nk_oracle


def _solve_spd(nk, P, R):
    from nys_koop_lqr_amd.regressors import KoopmanKernelRegressor
    return KoopmanKernelRegressor._solve_spd(nk.get_context(), P, R)


# ---------------------------------------------------------------------------------------------------------------
# rank-revealing fallback
# ---------------------------------------------------------------------------------------------------------------
def test_solve_spd_singular_gives_min_norm_solution(nk, O, golden):
    """A singular PSD system (rank 40 of 64, P = B B^T): the Cholesky meets a non-positive or rounding-level pivot and
    the library returns lstsq's minimum-norm solution with singular values <= eps * s_max dropped (Jacobi SVD on the
    device).  The golden records that gelsd itself kept 41 singular values here (its computed 41st lands just above the
    cut-off) and returns garbage along that direction -- so the checker is the oracle's SVD restatement with the cut-off
    inside the gap.  Whether the rounding-level null singular values of THIS matrix (formed in floating point) fall below
    eps * s_max is decided by the matrix, not by the solver; for this fixture they do."""
    g = golden("f9_rank_deficient.npz")
    P, R = g["spd_P"], g["spd_R"]
    Xo, rank = O.truncated_solve(P, R, rcond=1e-10)  # cut-off inside the gap: the well-defined answer
    assert rank == 40 and int(g["spd_rank"]) == 41
    X = _solve_spd(nk, P, R)
    assert relf(X, Xo) < 1e-9
    assert relf(P @ X, P @ Xo) < 1e-10  # the projection of R on range(P) is reproduced
    ctx = nk.get_context()
    ctx.set_strict_spd(True)
    try:
        with pytest.raises(np.linalg.LinAlgError):
            _solve_spd(nk, P, R)
    finally:
        ctx.set_strict_spd(False)
    # a well-conditioned system still takes the Cholesky path and matches a direct solve
    rng = np.random.default_rng(0)
    B = rng.standard_normal((64, 80))
    P2 = B @ B.T + 1e-3 * np.eye(64)
    assert relf(_solve_spd(nk, P2, R), np.linalg.solve(P2, R)) < 1e-10


@pytest.mark.parametrize("m", [7, 64, 130, 257])
def test_pinv_fallback_shapes(nk, O, m):
    """Odd / even sizes (the round-robin pairing has a dummy player for odd m), ranks 1, m/3, 3m/4, EXACTLY singular
    input: B has small integer entries, so P = B B^T is formed without rounding and has exact rank.  The rounding-level
    singular values the decomposition leaves for the null space ((1..50) eps s_max) form an isolated cluster and are
    dropped as a whole (nk_pinv.hip); the checker is the minimum-norm solution with the cut-off anywhere inside the gap.
    (Rank m - 1 with a nearly square random B is left out: there the leading (m-1) x (m-1) block is itself ill-conditioned
    and an UNPIVOTED Cholesky's last pivot carries an error of cond^2 eps, far above the rounding level the detection
    looks for -- the documented limit of triggering the fallback from Cholesky pivots.)"""
    rng = np.random.default_rng(m)
    for rank in sorted({1, max(1, m // 3), max(1, (3 * m) // 4)}):
        B = rng.integers(-3, 4, size=(m, rank)).astype(np.float64)
        while np.linalg.matrix_rank(B) < rank:
            B = rng.integers(-3, 4, size=(m, rank)).astype(np.float64)
        P = B @ B.T
        R = rng.standard_normal((m, 3))
        Xo, rk = O.truncated_solve(P, R, rcond=1e-10)
        assert rk == rank
        assert relf(_solve_spd(nk, P, R), Xo) < 1e-8, (m, rank)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_rank_deficient_fit_matches_reference(nk, O, golden, tag):
    """Duplicated landmarks + tiny gamma (tests/golden/make_golden_configs.py f9): both regularised systems have an exact
    null space next to a well-conditioned rest; the reference's gelsd truncates it.  A, B do not depend on how the null
    directions are treated (1e-8); C does at the 1e-6 level -- LAPACK's own SVD with gelsd's rule sits 1.7e-6 from
    gelsd's C, an untruncated Cholesky 8e-5 -- so C, W and predictions are held to 1e-5."""
    g = golden("f9_rank_deficient.npz")
    X, Y, idx = g["X"], g["Y"], g["idx"]
    d, p, m = Y.shape[1], int(g["p"]), int(g["m"])
    ls = float(g["ls"])
    reg = nk.KoopmanNystromRegressor(p, kernel=nk.ThreeDimensionalKernel(ls, ls, ls, d), gamma=float(g[f"{tag}_gamma"]), m=m)
    reg.nystrom_centers_output = Y.T[:, idx]
    reg.fit(X, Y)
    st = reg.fit_stats_
    assert relf(reg.A, g[f"{tag}_A"]) < 1e-8 and relf(reg.B, g[f"{tag}_B"]) < 1e-8
    assert relf(reg.C, g[f"{tag}_C"]) < 1e-5 and relf(reg.weights, g[f"{tag}_W"]) < 1e-5
    q = g["q"]
    assert relf(reg.predict(X[q]), g[f"{tag}_predict"]) < 1e-5
    assert relf(reg.lift(X[q, :d].T), g[f"{tag}_lift"]) < 1e-8
    # the numerical ranks the library reports are lstsq's `rank`: full, or full minus the 8 duplicated landmarks (gelsd's
    # own SVD kept one of the eight rounding-level singular values: its ranks are 92 / 89 for tag a)
    assert st["rank_inner"] in (m + p, m + p - 8)
    assert st["rank_inner_rec"] in (m, m - 8)
    if tag == "a":  # gamma = 1e-13: gamma n jitter = 6e-17, the null-space pivots are pure rounding noise
        assert st["rank_inner_rec"] == m - 8 and st["rank_inner"] == m + p - 8


def test_sweep_survives_a_failing_candidate(nk, golden):
    """GridSearchCV's error_score=nan behaviour: in strict mode the rank-deficient candidate raises inside its unit, scores
    NaN and ranks last; the sweep completes and picks the best finite candidate.  By default (no strict mode) the same
    sweep has no NaN at all."""
    from nys_koop_lqr_amd import harness
    g = golden("f9_rank_deficient.npz")
    X, Y, idx = g["X"], g["Y"], g["idx"]
    d, p, m = Y.shape[1], int(g["p"]), int(g["m"])
    kern = nk.ThreeDimensionalKernel(3.0, 3.0, 3.0, d)
    cands = [dict(kernel=kern, gamma=1e-13, m=m), dict(kernel=kern, gamma=1e-4, m=m)]
    folds = harness.kfold_slices(X.shape[0], 5)
    centers = {}
    for c in range(2):
        for f, (lo, hi) in enumerate(folds):
            n_train = X.shape[0] - (hi - lo)
            base = np.random.RandomState(100 + f).choice(n_train, m - 8, replace=False)
            centers[(c, f)] = np.concatenate([base, base[:8]])  # duplicated landmarks in every fold
    res = harness.grid_search_cv(X, Y, p, cands, centers=centers)
    assert np.all(np.isfinite(res["split_scores"])) and res["best_index"] in (0, 1)
    ctx = nk.get_context()
    ctx.set_strict_spd(True)
    try:
        strict = harness.grid_search_cv(X, Y, p, cands, centers=centers)
        with pytest.raises(np.linalg.LinAlgError):
            harness.grid_search_cv(X, Y, p, cands[:1], centers=centers, error_score="raise")
    finally:
        ctx.set_strict_spd(False)
    assert np.isnan(strict["split_scores"][0]).any() and np.all(np.isfinite(strict["split_scores"][1]))
    assert np.isnan(strict["mean_test_score"][0]) and strict["best_index"] == 1
    assert np.allclose(strict["split_scores"][1], res["split_scores"][1], rtol=0, atol=0)


# ---------------------------------------------------------------------------------------------------------------
# single-launch lifted recursion: rollout / closed loop, batched; explicit operators
# ---------------------------------------------------------------------------------------------------------------
def _fitted(nk, O, n=500, d=12, p=2, m=48, seed=3, ls=4.0, gamma=1e-4):
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((n, d))
    U = rng.standard_normal((n, p))
    Y = np.tanh(S @ (rng.standard_normal((d, d)) * 0.8 / np.sqrt(d))) + U @ (rng.standard_normal((p, d)) * 0.1)
    X = np.hstack([S, U])
    idx = rng.choice(n, m, replace=False)
    reg = nk.KoopmanNystromRegressor(p, kernel=nk.ThreeDimensionalKernel(ls, ls, ls, d), gamma=gamma, m=m)
    reg.nystrom_centers_output = Y.T[:, idx]
    reg.fit(X, Y)
    ref = O.KoopmanNystromOracle(p, kernel=O.ThreeDimensionalKernel(ls, ls, ls, d), gamma=gamma, m=m)
    ref.nystrom_centers_output = Y.T[:, idx]
    ref.fit(X, Y)
    return reg, ref, X, Y, rng


@pytest.mark.parametrize("m,p", [(48, 2), (100, 6), (128, 6), (129, 3), (200, 1), (33, 0), (300, 2), (520, 6), (1100, 2)])
def test_rollout_single_launch_and_stepwise_paths(nk, O, m, p):
    """m <= 128: the whole recursion (and the lift) in one launch with [A | B] resident in the registers of one workgroup;
    larger m: one launch as well, [A | B] spread over ceil(m / 16) workgroups that exchange the state through memory
    (lifted_chain_mw_kernel).  Both against the oracle's loop on the SAME operators (so that only the recursion is under
    test), single and batched, with and without the lifted trajectory."""
    reg, ref, X, Y, rng = _fitted(nk, O, n=max(4 * m, 300), d=9, p=p, m=m, seed=m + p)
    d = Y.shape[1]
    T = 40
    Useq = rng.standard_normal((p, T))
    sim, Z = reg.rollout(X[3, :d], Useq, return_lifted=True)
    z0 = reg.lift(X[3, :d].reshape(-1, 1))
    B = reg.B if p > 0 else np.zeros((m, 0))
    so, Zo = O.rollout(reg.A, B, reg.C, z0, Useq)
    assert sim.shape == (d, T) and Z.shape == (m, T)
    assert relf(Z, Zo) < 1e-11 and relf(sim, so) < 1e-11
    batch = 5
    Ub = rng.standard_normal((batch, T, p))
    xb = X[10:10 + batch, :d]
    out, outz = reg.rollout(xb, Ub, return_lifted=True)
    for b in range(batch):
        sb = reg.rollout(xb[b], Ub[b].T)
        assert np.array_equal(out[b].T, sb)  # trajectories of a batch do not influence each other: same bits
    so, _ = O.rollout(reg.A, B, reg.C, reg.lift(xb[4].reshape(-1, 1)), Ub[4].T)
    assert relf(out[4].T, so) < 1e-11
    # explicit operators, no model (nk_linear_rollout)
    lin = nk.linear_rollout(reg.A, B, reg.C, z0, Useq)
    assert relf(lin, sim) < 1e-12
    linb = nk.linear_rollout(reg.A, B, reg.C, outz[:, 0, :], Ub)
    assert relf(linb, out) < 1e-12
    # T = 1: only the lifted initial state
    one = reg.rollout(X[3, :d], Useq[:, :1])
    assert relf(one, reg.C @ z0) < 1e-12
    if m in (129, 200):
        # 70 trajectories are 18 groups of four: more than the 16 groups that are chunked unconditionally, so the multi-workgroup
        # recursion takes them only where 18 x ceil(m / 16) workgroups are resident at once (on 256 compute units they are: one
        # launch), and one GEMM per step advances them elsewhere (csrc/nk_chain_plan.h).  The GEMM per step itself is held
        # entry by entry in test_gpu_rollout_steps.py::test_one_launch_per_step[gemm-*], which asserts its route.
        nb = 70
        Ubig = rng.standard_normal((nb, 12, p))
        big = reg.rollout(X[:nb, :d], Ubig)
        for b in (0, 33, 69):
            so, _ = O.rollout(reg.A, B, reg.C, reg.lift(X[b, :d].reshape(-1, 1)), Ubig[b].T)
            assert relf(big[b].T, so) < 1e-11


def test_rollout_multi_workgroup_recursion_repeats_stepwise_when_it_gives_up(nk, O, monkeypatch):
    """m > 128: if a wave of the single-launch recursion gives up waiting for its neighbours (oversubscribed device) the
    call repeats the recursion with one launch per step.  The hook makes the library take that branch."""
    reg, ref, X, Y, rng = _fitted(nk, O, n=900, d=9, p=3, m=200, seed=21)
    d, T = Y.shape[1], 25
    Ub = rng.standard_normal((3, T, 3))
    first = reg.rollout(X[:3, :d], Ub)
    monkeypatch.setenv("NYSKOOP_CHAIN_MW_TEST_GIVEUP", "1")
    again = reg.rollout(X[:3, :d], Ub)
    K = reg.solve_lqr(c=0.5)
    f0 = reg.lift(X[:2, :d].T).T
    xs_step, us_step = reg.closed_loop(K, f0, f0[::-1].copy(), 15)
    monkeypatch.delenv("NYSKOOP_CHAIN_MW_TEST_GIVEUP")
    xs, us = reg.closed_loop(K, f0, f0[::-1].copy(), 15)
    assert relf(again, first) < 1e-12 and relf(xs_step, xs) < 1e-12 and relf(us_step, us) < 1e-11
    so, _ = O.rollout(reg.A, reg.B, reg.C, reg.lift(X[1, :d].reshape(-1, 1)), Ub[1].T)
    assert relf(again[1].T, so) < 1e-11


def test_rollout_vs_reference_golden_through_single_launch(nk, golden):
    """The reference's own forecast (tests/golden f1 well-conditioned, m = 32 -> LDS-resident path)."""
    g = golden("f1_cloth_rbf_wellcond.npz")
    ls = g["ls"]
    reg = nk.KoopmanNystromRegressor(6, kernel=nk.ThreeDimensionalKernel(*ls, 192), gamma=float(g["gamma"]), m=32)
    reg.nystrom_centers_output = g["Y"].T[:, g["idx"]]
    reg.fit(g["X"], g["Y"])
    sim = reg.rollout(g["test_traj"][:, 0], g["test_u"][:, :g["test_traj"].shape[1]])
    assert relf(sim, g["rollout"]) < 1e-6


def test_closed_loop_batch(nk, O):
    reg, ref, X, Y, rng = _fitted(nk, O, n=400, d=12, p=2, m=64, seed=11)
    d = Y.shape[1]
    K = reg.solve_lqr(c=0.5)
    x0s, refs = X[:6, :d], X[20:26, :d]
    phi0 = reg.lift(x0s.T).T
    phir = reg.lift(refs.T).T
    xs, us = reg.closed_loop(K, phi0, phir, 30)
    assert xs.shape == (6, 30, d) and us.shape == (6, 30, 2)
    for b in range(6):
        xo, uo = O.lqr_closed_loop_lifted(reg.A, reg.B, reg.C, K, phi0[b], phir[b], 30)
        assert relf(xs[b].T, xo) < 1e-9 and relf(us[b].T, uo) < 1e-8
        x1, u1 = reg.closed_loop(K, phi0[b], phir[b], 30)
        assert np.array_equal(x1, xs[b].T) and np.array_equal(u1, us[b].T)
    # one shared reference broadcast over the batch
    xs2, _ = reg.closed_loop(K, phi0, phir[:1], 30)
    assert np.array_equal(xs2[0], xs[0])
    # m > 128: the multi-workgroup recursion with a bias per trajectory (the stepwise paths of the closed loop, which this
    # call only reaches after a give-up, are run in test_gpu_rollout_steps.py::test_closed_loop[loop-step-*, loop-gemm-*])
    reg2, _, X2, Y2, _ = _fitted(nk, O, n=600, d=6, p=2, m=150, seed=12)
    K2 = reg2.solve_lqr(c=0.5)
    f0 = reg2.lift(X2[:3, :6].T).T
    fr = reg2.lift(X2[5:8, :6].T).T
    xs3, us3 = reg2.closed_loop(K2, f0, fr, 12)
    for b in range(3):
        xo, uo = O.lqr_closed_loop_lifted(reg2.A, reg2.B, reg2.C, K2, f0[b], fr[b], 12)
        assert relf(xs3[b].T, xo) < 1e-9 and relf(us3[b].T, uo) < 1e-8


def test_lqr_control_cloth_full(nk, O, golden):
    """benchmark_lqr_cloth.py:69-104 end to end against the reference estimator's own outputs (f10): cumulative inputs
    seeded from the control nodes, per-axis split, simulator row order."""
    from nys_koop_lqr_amd import harness
    g = golden("f10_lqr_control.npz")
    t = golden("cloth_trajs_all.npz")
    states = t["states_e10"] / 1e10
    X = np.hstack([np.vstack((states[i][:, :-1], t["inputs"][i][:, :-1])) for i in range(10, 40)]).T
    Y = np.hstack([states[i][:, 1:] for i in range(10, 40)]).T
    reg = nk.KoopmanNystromRegressor(6, kernel=nk.ThreeDimensionalKernel(*g["ls"], 192), gamma=float(g["gamma"]), m=100)
    reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, g["idx"]])
    reg.fit(np.ascontiguousarray(X), np.ascontiguousarray(Y))
    assert relf(reg.A, g["A"]) < 1e-6 and relf(reg.C, g["C"]) < 1e-6
    # the loop itself on the reference's operators and gain
    reg.A, reg.B, reg.C = g["A"], g["B"], g["C"]
    init, ref_state = g["initial_state"], g["reference_lqr"]
    x_s, y_s, z_s, final_us = harness.lqr_control(60, ref_state, init, reg, g["K"])
    for got, key in ((x_s, "x_s"), (y_s, "y_s"), (z_s, "z_s"), (final_us, "final_us")):
        assert got.shape == g[key].shape
        assert relf(got, g[key]) < 1e-8, key
    xo = O.lqr_control_cloth(g["A"], g["B"], g["C"], g["K"], reg.lift(init), reg.lift(ref_state), init, 60)
    assert relf(final_us, xo[3]) < 1e-9
    # whole chain with the library's own operators and host DARE
    reg.fit(np.ascontiguousarray(X), np.ascontiguousarray(Y))
    K = reg.solve_lqr(c=0.0075)
    assert relf(K, g["K"]) < 1e-5
    out = harness.lqr_control(60, ref_state, init, reg, K)
    assert relf(out[3], g["final_us"]) < 1e-5 and relf(out[2], g["z_s"]) < 1e-6


def test_open_loop_rmse_matches_shipped_csv(nk, golden):
    """H1 pin on the reference authors' own numbers: all_rmses_nystrom_cloth_swing_angle.csv (20 rows x 20 values of m),
    produced by the loop of benchmark_lqr_cloth.py:163-211 with RBF l = 10, gamma = 1e-7 (the hyper-parameters of the
    shipped regressors).  Replaying seed 0 -- the trajectory shuffle, then one landmark draw per fit from the global
    legacy RNG PLUS one discarded draw of the same size (the code version that wrote the CSV drew the input centres
    separately) -- reproduces the shipped entries to 8 digits with the faithful oracle
    (tests/test_oracle_golden.py::test_shipped_cloth_rmse_rows).  Here the HIP path replays the first three rows = 60 fits;
    large m is ill-conditioned (cond ~ 1e13), where the reference's gelsd noise shows in the third digit."""
    import random
    from nys_koop_lqr_amd import harness
    g = golden("f10_lqr_control.npz")
    t = golden("cloth_trajs_all.npz")
    states = t["states_e10"] / 1e10
    trajs = [states[i] for i in range(10, 50)]
    ctrls = [t["inputs"][i] for i in range(10, 50)]
    ms = np.logspace(1.0, 2.6, num=20, dtype=int)
    shipped = g["all_rmses"]
    assert shipped.shape == (20, 20)
    np.random.seed(0)
    random.seed(0)
    order = np.arange(40)
    np.random.shuffle(order)
    train, test = order[:30], order[30:]
    Xc, Yc = harness.create_data_matrices(trajs, ctrls, train)
    X, Y = np.ascontiguousarray(Xc.T), np.ascontiguousarray(Yc.T)
    rows = []
    for i in test[:3]:
        row = []
        for m in ms:
            reg = nk.KoopmanNystromRegressor(6, kernel=nk.ThreeDimensionalKernel(10, 10, 10, 192), gamma=1e-7, m=int(m))
            reg.fit(X, Y)  # landmarks from the global legacy RNG, like the reference
            np.random.choice(np.arange(0, X.shape[0]), size=int(m), replace=False)  # the discarded second draw
            row.append(harness.validate_dyn_sys(reg, trajs[i], ctrls[i]))
        rows.append(row)
    rows = np.array(rows)
    rel = np.abs(rows - shipped[:3]) / shipped[:3]
    print("\n[H1 shipped CSV] relative error of the open-loop RMSE, rows 0-2: median %.1e, max %.1e; by m: %s"
          % (np.median(rel), rel.max(), np.array2string(rel.max(axis=0), precision=1)))
    assert np.median(rel) < 1e-3 and rel.max() < 5e-2
    assert rel[:, :8].max() < 1e-4  # m <= 38: well conditioned


# ---------------------------------------------------------------------------------------------------------------
# plumbing: stream ordering for device tensors, versioned device model, deterministic teardown
# ---------------------------------------------------------------------------------------------------------------
def test_device_tensor_inputs_are_ordered_after_torch_work(nk, O):
    """A device tensor handed to the library while torch still has work queued for it: nk_wait_stream orders the library's
    non-blocking streams behind torch's current stream (the all-reduce -> fit_from_gram hand-off)."""
    import torch
    reg, ref, X, Y, rng = _fitted(nk, O, n=3000, d=24, p=2, m=64, seed=5)
    d = Y.shape[1]
    Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    cnt = reg.gram_size(d)
    acc = torch.zeros(cnt, dtype=torch.float64, device="cuda")
    parts = []
    for lo, hi in ((0, 1000), (1000, 3000)):
        part = torch.empty(cnt, dtype=torch.float64, device="cuda")
        reg.gram_partial(Xd[lo:hi], Yd[lo:hi], out=part)
        parts.append(part)
    big = torch.randn(4096, 4096, device="cuda")
    for _ in range(20):  # keep torch's stream busy so that the adds below are still pending at the hand-off
        big = big @ big
        big = big / big.norm()
    for part in parts:
        acc += part
    reg2 = nk.KoopmanNystromRegressor(2, kernel=reg.kernel, gamma=reg.gamma, m=64)
    reg2.nystrom_centers_output = reg.nystrom_centers_output
    reg2.fit_from_gram(acc, 3000, d)
    assert relf(reg2.A, reg.A) < 1e-9 and relf(reg2.C, reg.C) < 1e-9
    # scaling the inputs on torch's stream right before the fit must be seen by the fit
    Xs = Xd.clone()
    Ys = Yd.clone()
    for _ in range(10):
        big = big @ big
        big = big / big.norm()
    Xs.mul_(1.0)
    Ys.mul_(1.0)
    reg3 = nk.KoopmanNystromRegressor(2, kernel=reg.kernel, gamma=reg.gamma, m=64)
    reg3.nystrom_centers_output = reg.nystrom_centers_output
    reg3.fit(Xs, Ys)
    assert relf(reg3.A, reg.A) < 1e-10


def test_assigning_operators_rebuilds_device_model(nk, O):
    reg, ref, X, Y, rng = _fitted(nk, O, n=300, d=6, p=1, m=24, seed=8)
    d = Y.shape[1]
    Useq = rng.standard_normal((1, 10))
    a = reg.rollout(X[0, :d], Useq)
    reg.A = reg.A * 0.5  # assignment: the device copy must follow
    b = reg.rollout(X[0, :d], Useq)
    z0 = reg.lift(X[0, :d].reshape(-1, 1))
    so, _ = O.rollout(reg.A, reg.B, reg.C, z0, Useq)
    assert relf(b, so) < 1e-11 and relf(a, so) > 1e-3
    with pytest.raises(ValueError):
        reg.score_neg_rmse(X[:10], Y[:9])
    with pytest.raises(ValueError):
        reg.score_neg_rmse(X[:10, :d], Y[:10])


def test_clean_exit_with_live_objects():
    """Teardown order: a process that exits with live contexts, models, pinned result arrays, a pending asynchronous
    fetch and worker threads must exit cleanly (atexit -> nk_shutdown before the HIP runtime's static destructors);
    explicit shutdown followed by finalisers is harmless too."""
    code = r'''
import numpy as np, sys
sys.path.insert(0, %r)
import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import harness, _lib
rng = np.random.default_rng(0)
X = rng.standard_normal((400, 8)); Y = np.tanh(X[:, :6])
regs = []
for i in range(3):
    r = nk.KoopmanNystromRegressor(2, kernel=nk.ThreeDimensionalKernel(2., 2., 2., 6), gamma=1e-4, m=32)
    r.nystrom_centers_output = Y.T[:, :32]
    r.fit(X, Y)          # leaves an asynchronous fetch pending
    regs.append(r)
cands = [dict(kernel=nk.ThreeDimensionalKernel(2., 2., 2., 6), gamma=g, m=16) for g in (1e-4, 1e-3)]
np.random.seed(0)
res = harness.grid_search_cv(X, Y, 2, cands, workers=3)
a = np.array(regs[0].A)   # a copy: the page-locked result arrays go away with nk_shutdown
if len(sys.argv) > 1:
    nk.shutdown(); nk.shutdown()
    del regs
print("OK", float(a[0, 0]) == float(a[0, 0]))
''' % ROOT
    for extra in ([], ["explicit"]):
        out = subprocess.run([sys.executable, "-c", code] + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (out.returncode, out.stdout[-500:], out.stderr[-2000:])
        assert "OK" in out.stdout


# ---------------------------------------------------------------------------------------------------------------
# lock-step batching of small fits (nk_group_*, nk_cv_grid)
# ---------------------------------------------------------------------------------------------------------------
def _cv_problem(nk, n=505, d=24, p=2, m=64, ncand=6, seed=4):
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((n, d))
    U = rng.standard_normal((n, p))
    Y = np.tanh(S @ (rng.standard_normal((d, d)) * 0.8 / np.sqrt(d))) + U @ (rng.standard_normal((p, d)) * 0.1)
    X = np.hstack([S, U])
    ls = (2.0, 4.0, 8.0)
    cands = [dict(kernel=nk.ThreeDimensionalKernel(l, l, l, d), gamma=g, m=m) for l in ls for g in (1e-5, 1e-3)][:ncand]
    folds = [(0, 101), (101, 202), (202, 303), (303, 404), (404, 505)]
    centers = {(c, f): np.random.RandomState(31 * c + f).choice(n - 101, m, replace=False) for c in range(len(cands))
               for f in range(5)}
    return X, Y, p, cands, centers


@pytest.mark.parametrize("batch,groups", [(4, 1), (16, 1), (7, 2), (40, 1)])
def test_lockstep_batched_sweep_is_bit_identical(nk, batch, groups):
    """The batched sweep (members of a lock-step group, launches merged into blockIdx.z-batched twins) computes exactly
    the bits of the one-unit-at-a-time sweep: same kernels, same arguments.  d = 24 takes the direct-difference kernel
    blocks; folds 1-3 have two row ranges (gathered), folds 0 and 4 one; the candidates need different numbers of
    square-root iterations (alignment points)."""
    from nys_koop_lqr_amd import harness, _lib
    X, Y, p, cands, centers = _cv_problem(nk)
    base = harness.grid_search_cv(X, Y, p, cands, centers=centers)
    res = harness.grid_search_cv(X, Y, p, cands, centers=centers, batch=batch, batch_groups=groups)
    assert np.array_equal(res["split_scores"], base["split_scores"])
    assert res["best_index"] == base["best_index"]
    st = _lib.lockstep_pool(batch).stats()
    assert st["merged_launches"] > 0 and st["member_launches_merged"] > st["merged_launches"]


def test_lockstep_gram_form_blocks_and_failing_unit(nk):
    """d >= 32: Gram-form kernel blocks on the MFMA engine inside a batch; one candidate (duplicated landmarks, tiny gamma)
    takes the SVD fallback inside its unit while the others go on -- its kernels have no twin and run one member at a time."""
    from nys_koop_lqr_amd import harness
    X, Y, p, cands, centers = _cv_problem(nk, d=48, m=96, ncand=4, seed=9)
    cands[1] = dict(kernel=cands[1]["kernel"], gamma=1e-13, m=96)
    for f in range(5):
        base_idx = centers[(1, f)][:88]
        centers[(1, f)] = np.concatenate([base_idx, base_idx[:8]])
    one = harness.grid_search_cv(X, Y, p, cands, centers=centers)
    res = harness.grid_search_cv(X, Y, p, cands, centers=centers, batch=10)
    assert np.all(np.isfinite(one["split_scores"]))
    assert np.array_equal(res["split_scores"], one["split_scores"])


def test_lockstep_pool_runs_ordinary_api_calls(nk, O):
    """Members of a group driven through the ordinary estimator API from their own threads (fit, lift, predict, rollout,
    operator fetch): every call works inside and outside a unit of work and equals the ungrouped result."""
    from nys_koop_lqr_amd import _lib
    reg0, ref, X, Y, rng = _fitted(nk, O, n=400, d=10, p=2, m=40, seed=21)
    d = Y.shape[1]
    Useq = rng.standard_normal((2, 12))
    want = (np.array(reg0.A), reg0.predict(X[:20]), reg0.rollout(X[0, :d], Useq))

    def unit(k):
        reg = nk.KoopmanNystromRegressor(2, kernel=reg0.kernel, gamma=reg0.gamma, m=40)
        reg.nystrom_centers_output = reg0.nystrom_centers_output
        reg.fit(X, Y)
        return np.array(reg.A), reg.predict(X[:20]), reg.rollout(X[0, :d], Useq)

    pool = _lib.lockstep_pool(5, index=7)
    for got in pool.map(unit, range(8)):  # a full round of 5 and a partial round of 3
        for a, b in zip(got, want):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("family", [0, 1, 2])
@pytest.mark.parametrize("d", [2, 21, 192])
def test_kernel_matrix_bits_do_not_depend_on_the_shape(nk, family, d):
    """The three kernel-matrix kernels (tiled, flat streaming for d <= 8, one thread per entry for a handful of entries --
    the lift of ONE state inside a control loop) do the same operations per entry in the same order: a row of a big call
    and the same row computed alone have the same bits."""
    rng = np.random.default_rng(100 * family + d)
    A = rng.standard_normal((700, d)); B = rng.standard_normal((150, d))
    ls = rng.uniform(0.5, 3.0, size=d) * np.sqrt(d)
    k = nk.kernels.DeviceKernel(family, ls) if family < 2 else nk.LinearKernelWrapper(0.7).kernel
    big = k(A, B)                      # 105 000 entries: tiled (or flat at d = 2)
    for rows in (slice(0, 1), slice(3, 8), slice(650, 700)):
        assert np.array_equal(k(A[rows], B), big[rows])   # <= 7500 entries: one thread per entry
    assert np.array_equal(k(A[:40], B[:7]), big[:40, :7])


def test_exact_kernel_regressor_device_and_host_compositions_agree(nk, monkeypatch):
    """KoopmanKernelRegressor.fit keeps its N x N intermediates in HBM (torch tensors as the allocator); the host-composed
    version (NYSKOOP_EXACT_HOST=1, also the path without torch) runs the same library calls on host arrays."""
    import pickle
    rng = np.random.default_rng(5)
    N = 350
    x = rng.uniform(-1, 1, (N, 2)); u = rng.uniform(-1, 1, (N, 1))
    y = x + 0.05 * np.tanh(x @ rng.standard_normal((2, 2))) + 0.05 * u
    X = np.hstack([x, u])
    dev = nk.KoopmanKernelRegressor(1, kernel=nk.KernelWrapper([0.7, 0.7]), gamma=1e-6)
    dev.fit(X, y)
    assert "_dev_cache" in dev.__dict__  # the device path ran
    monkeypatch.setenv("NYSKOOP_EXACT_HOST", "1")
    host = nk.KoopmanKernelRegressor(1, kernel=nk.KernelWrapper([0.7, 0.7]), gamma=1e-6)
    host.fit(X, y)
    assert "_dev_cache" not in host.__dict__
    Xq = X[:40]
    assert relf(dev.predict(Xq), host.predict(Xq)) < 1e-9
    assert relf(dev.lift(x[:9].T), host.lift(x[:9].T)) < 1e-10
    assert relf(dev.weights, host.weights) < 1e-7 and relf(dev.C, host.C) < 1e-7
    back = pickle.loads(pickle.dumps(dev))  # device tensors do not travel; the copy lifts from its host arrays
    assert "_dev_cache" not in back.__dict__
    assert relf(back.predict(Xq), dev.predict(Xq)) < 1e-10


@pytest.mark.parametrize("m", [64, 200])
def test_validate_dyn_sys_all_trajectories_in_one_call(nk, O, m):
    """The loop over test trajectories (benchmark_lqr_cloth.py:171-176) as one batched rollout: same numbers."""
    from nys_koop_lqr_amd import harness
    reg, ref, X, Y, rng = _fitted(nk, O, n=4 * m + 200, d=9, p=2, m=m, seed=40 + m)
    k, T = 7, 30
    trajs = rng.standard_normal((k, 9, T)); ctrl = rng.standard_normal((k, 2, T - 1))
    for relative in (False, True):
        one_by_one = np.array([harness.validate_dyn_sys(reg, trajs[i], ctrl[i], relative) for i in range(k)])
        together = harness.validate_dyn_sys_all(reg, trajs, ctrl, relative)
        assert together.shape == (k,) and np.allclose(together, one_by_one, rtol=1e-12, atol=0)


@pytest.mark.parametrize("m,block", [(130, "1"), (130, "0"), (600, "1"), (1100, "1")])
def test_rank_deficient_solve_through_every_jacobi_kernel(nk, O, monkeypatch, m, block):
    """The minimum-norm solution of an exactly rank-deficient PSD system through the block Jacobi with 8 / 4 / 2 rows per
    block (m <= 512 / 1024 / 2048) and through the scalar rounds (NYSKOOP_PINV_BLOCK=0), against the oracle's truncated
    SVD solve with the cut-off inside the spectral gap."""
    rng = np.random.default_rng(m)
    r = m - 37
    Bm = rng.standard_normal((m, r)) / np.sqrt(r)
    P = Bm @ Bm.T
    R = rng.standard_normal((m, 3))
    monkeypatch.setenv("NYSKOOP_PINV_BLOCK", block)
    X = _solve_spd(nk, P, R)
    Xo, rank = O.truncated_solve(P, R, rcond=1e-10)
    assert rank == r
    assert relf(X, Xo) < 1e-8 and relf(P @ X, P @ Xo) < 1e-8
