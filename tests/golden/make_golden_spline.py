#!/usr/bin/env python3
"""Thin-plate-spline EDMD (the reference's KoopmanSplineRegressor, regressors.py:181-233): golden vectors produced by
RUNNING THE REFERENCE in the build container.  Only DATA is written.

    python tests/golden/make_golden_spline.py

The inputs are not duplicated: the Duffing data set is X, Y of f12_duffing_full.npz, the cloth trajectories are those of
cloth_trajs_all.npz.

  f15_spline_duffing.npz   benchmark_lqr_classic.py:211-255 with kapprox = 'splines': gamma = 1e-6,
      state_bounds_params = [1.0, 2], for seeds 0, 1, 2 and 199: np.random.seed(seed) -> test trajectory,
      np.random.seed(seed) -> 20 sequential fits with m = around(logspace(1, 2.3, 20)), centres drawn by the reference
      (disc branch of compute_centers) -> relative-% RMSE of validate_dyn_sys.  Stored: the centres of all 80 fits, the
      test trajectories, the reference's RMSEs, the rows of the authors' duffing/all_rmses_splines_double_dataset.csv,
      and A, B, C of seed 0 at m = 10, 48, 200.
  f15_spline_cloth.npz     the seed-0 split of benchmark_lqr_cloth.py:168-193 (30 training trajectories, n = 3030,
      d = 192, p = 6); fits with the centres drawn by the reference (data branch) at gamma = 1e-5 for m = 10, 12, 14
      (the first three m of the driver's schedule, drawn in sequence after the shuffle) and m = 500, and at gamma = 1e-7
      for m = 398 and 500 (the cases where scipy.linalg.pinv truncates).  Stored per case: centre indices into the
      training rows, predict() on the first 16 rows of the first test trajectory, the cloth validate_dyn_sys RMSE on it,
      the rank pinv keeps, and seeded operator probes (A PA, C PC, B).
  f15_spline_tps.npz       thin-plate-spline kernel matrices r^2 log(sqrt(r^2)) (regressors.py:229-233) at d = 2 and
      d = 192, both with coincident pairs (exact zeros).

The reference's own spread is recorded for every case: (a) the inputs perturbed by one part in 1e15 with the same
centres, (b) pinv computed through scipy.linalg.svd(lapack_driver='gesvd') instead of gesdd.  The bars of the GPU tests
are a fixed multiple of that spread with a floor, computed here once (BAR_FACTOR, BAR_FLOOR_*).
"""
import os
import random
import sys
from multiprocessing import Pool

os.environ.setdefault("OMP_NUM_THREADS", "2")  # four worker processes on the fits
import numpy as np  # noqa: E402
import scipy.linalg  # noqa: E402

REF = os.environ.get("NK_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, OUT)

import regressors as R  # noqa: E402  (the reference)
from make_golden_duffing import duffing_plant, load_dataset, simulate_true_system, validate_dyn_sys  # noqa: E402

GAMMA_DUF = 1e-6
BOUNDS = np.array([1.0, 2])
SEEDS = [0, 1, 2, 199]
BAR_FACTOR = 100.0
BAR_FLOOR_RMSE = 1e-9      # relative, on RMSEs
BAR_FLOOR_OPS = 1e-9       # relative Frobenius, on operators / predictions
EPS = np.finfo(float).eps

_orig_pinv = scipy.linalg.pinv


def pinv_gesvd(a):
    """scipy.linalg.pinv's rule (atol = 0, rtol = max(M, N) eps) on singular values from gesvd."""
    u, s, vh = scipy.linalg.svd(a, full_matrices=False, lapack_driver="gesvd")
    cut = max(a.shape) * EPS * s.max()
    keep = s > cut
    return (vh[keep].T / s[keep]) @ u[:, keep].T


class Gesvd:
    def __enter__(self):
        R.scipy.linalg.pinv = pinv_gesvd

    def __exit__(self, *exc):
        R.scipy.linalg.pinv = _orig_pinv


def fit_with(centers, m, gamma, X, Y, bounds):
    reg = R.KoopmanSplineRegressor(X.shape[1] - Y.shape[1], state_bounds_params=bounds, m=m, gamma=gamma)
    reg.centers = centers
    reg.fit(X, Y)
    return reg


def system_stats(reg, X, Y):
    """rank scipy.linalg.pinv keeps (regressors.py:214) and the Cholesky pivots of P = cov + gamma n I."""
    n_states = Y.shape[1]
    phi = np.vstack((reg.lift(X[:, :n_states].T), X[:, n_states:].T))
    P = phi @ phi.T + reg.gamma * X.shape[0] * np.eye(phi.shape[0])
    s = np.linalg.svd(P, compute_uv=False)
    rank = int(np.sum(s > max(P.shape) * EPS * s.max()))
    L = np.linalg.cholesky(P)
    piv = np.diag(L) ** 2
    return rank, float(s.min() / s.max()), float(piv.min() / piv.max())


def relf(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def duffing_seed(seed):
    X, Y = load_dataset()
    Xs, Ys = X.T.copy(), Y.T.copy()
    prng = np.random.default_rng(1000 + seed)
    Xp = Xs * (1 + 1e-15 * prng.standard_normal(Xs.shape))
    ds = duffing_plant()
    ms = np.around(np.logspace(1, 2.3, num=20)).astype(int)
    np.random.seed(seed); random.seed(seed)
    traj, ctrl = simulate_true_system(ds, 2)
    np.random.seed(seed); random.seed(seed)
    res = dict(traj=traj, ctrl=ctrl, centers=[], rmse=[], rmse_pert=[], rmse_gesvd=[], ops={}, ops_spread=[], stats=[])
    for m in ms:
        reg = R.KoopmanSplineRegressor(1, state_bounds_params=BOUNDS, m=int(m), gamma=GAMMA_DUF)
        reg.fit(Xs, Ys)
        r0, _ = validate_dyn_sys(reg, traj, ctrl)
        c = reg.centers.copy()
        rp = fit_with(c, int(m), GAMMA_DUF, Xp, Ys, BOUNDS)
        r1, _ = validate_dyn_sys(rp, traj, ctrl)
        with Gesvd():
            rg = fit_with(c, int(m), GAMMA_DUF, Xs, Ys, BOUNDS)
        r2, _ = validate_dyn_sys(rg, traj, ctrl)
        res["centers"].append(c)
        res["rmse"].append(r0); res["rmse_pert"].append(r1); res["rmse_gesvd"].append(r2)
        res["ops_spread"].append(max(max(relf(o.A, reg.A), relf(o.B, reg.B), relf(o.C, reg.C)) for o in (rp, rg)))
        if seed == 0 and int(m) in (10, 48, 200):
            res["ops"][int(m)] = (reg.A, reg.B, reg.C)
        if int(m) in (10, 200):
            res["stats"].append((int(m),) + system_stats(reg, Xs, Ys))
        print(f"duffing seed {seed} m {m}: rmse {r0:.6g} spread {abs(r1 - r0) / r0:.2e} {abs(r2 - r0) / r0:.2e}",
              flush=True)
    return seed, res


def f15_duffing(pool):
    ms = np.around(np.logspace(1, 2.3, num=20)).astype(int)
    shipped = np.loadtxt(f"{REF}/duffing/all_rmses_splines_double_dataset.csv")
    out = dict(ms=ms, gamma=GAMMA_DUF, bounds=BOUNDS, seeds=np.array(SEEDS), bar_factor=BAR_FACTOR)
    rm, spread, ospread = np.zeros((4, 20)), np.zeros((4, 20)), np.zeros((4, 20))
    stats = []
    for seed, res in pool.map(duffing_seed, SEEDS):
        si = SEEDS.index(seed)
        out[f"traj_{seed}"], out[f"ctrl_{seed}"] = res["traj"], res["ctrl"]
        out[f"centers_{seed}"] = np.concatenate(res["centers"], axis=1)  # 2 x sum(ms), fit k = columns of block k
        rm[si] = res["rmse"]
        r = np.array(res["rmse"])
        spread[si] = np.maximum(np.abs(np.array(res["rmse_pert"]) - r), np.abs(np.array(res["rmse_gesvd"]) - r)) / r
        ospread[si] = res["ops_spread"]
        for m, (A, B, C) in res["ops"].items():
            out[f"A_{m}"], out[f"B_{m}"], out[f"C_{m}"] = A, B, C
        stats += [(seed,) + s for s in res["stats"]]
    out["ref_rmse"] = rm
    out["shipped_rows"] = shipped[SEEDS]
    out["spread_rmse"] = spread
    out["spread_ops"] = ospread
    out["bar_rmse"] = np.maximum(BAR_FACTOR * spread, BAR_FLOOR_RMSE)
    # operators of seed 0: the spread of those fits
    out["bar_ops"] = np.maximum(BAR_FACTOR * ospread[0], BAR_FLOOR_OPS)
    # (seed, m, rank kept by pinv, sigma_min / sigma_max, smallest / largest Cholesky pivot)
    out["system_stats"] = np.array(stats)
    np.savez_compressed(f"{OUT}/f15_spline_duffing.npz", **out)
    print("shipped vs reference, max relative per seed:", np.max(np.abs(rm - out["shipped_rows"]) / out["shipped_rows"], axis=1))


def cloth_split():
    """benchmark_lqr_cloth.py:138-193 for seed 0: trajectories 10..49, shuffled; 30 train, 10 test."""
    g = np.load(f"{OUT}/cloth_trajs_all.npz")
    states = g["states_e10"] / 1e10
    inputs = g["inputs"]
    all_t = list(range(10, 50))
    np.random.seed(0); random.seed(0)
    idx = np.arange(0, 40)
    np.random.shuffle(idx)
    train, test = [all_t[i] for i in idx[:30]], [all_t[i] for i in idx[30:]]
    X = np.hstack([np.vstack((states[i][:, :-1], inputs[i][:, :-1])) for i in train]).T.copy()
    Y = np.hstack([states[i][:, 1:] for i in train]).T.copy()
    return np.array(train), np.array(test), X, Y, states, inputs


def cloth_rmse(reg, traj, ctrl):
    """benchmark_lqr_cloth.py:18-36."""
    x = reg.lift(traj[:, 0].reshape([-1, 1]))
    sim = reg.C @ x
    for i in range(traj.shape[1] - 1):
        x = reg.A @ x + reg.B @ ctrl[:, i].reshape([-1, 1])
        sim = np.hstack((sim, reg.C @ x))
    return float(np.sqrt(np.mean(np.square(traj - sim))))


CLOTH_CASES = [(1e-5, 10), (1e-5, 12), (1e-5, 14), (1e-5, 500), (1e-7, 398), (1e-7, 500)]


def cloth_case(k):
    gamma, m = CLOTH_CASES[k]
    train, test, X, Y, states, inputs = cloth_split()
    n = X.shape[0]
    # centres: the first three are drawn in sequence right after the shuffle (the driver's loop over ms); the others
    # after np.random.seed(0) + shuffle again (one fit each)
    draws = []
    orig = np.random.choice

    def spy(*a, **kw):
        o = orig(*a, **kw)
        draws.append(np.array(o))
        return o
    np.random.choice = spy
    try:
        if k < 3:
            for gm in CLOTH_CASES[:k + 1]:
                reg = R.KoopmanSplineRegressor(6, m=gm[1], gamma=gm[0])
                reg.fit(X, Y)
        else:
            reg = R.KoopmanSplineRegressor(6, m=m, gamma=gamma)
            reg.fit(X, Y)
    finally:
        np.random.choice = orig
    cidx = draws[-1]
    assert np.array_equal(reg.centers, X[:, :192].T[:, cidx])
    traj, ctrl = states[test[0]], inputs[test[0]]
    Xq = np.vstack((traj[:, :-1], ctrl[:, :-1])).T[:16]
    prng = np.random.default_rng(77 + k)
    Xp = X * (1 + 1e-15 * prng.standard_normal(X.shape))
    rp = fit_with(reg.centers, m, gamma, Xp, Y, None)
    with Gesvd():
        rg = fit_with(reg.centers, m, gamma, X, Y, None)
    PA = np.random.default_rng(5).standard_normal((m, 4))
    PC = np.random.default_rng(6).standard_normal((m, 4))
    out = dict(centers_idx=cidx, predict=reg.predict(Xq), rmse=cloth_rmse(reg, traj, ctrl), A_probe=reg.A @ PA,
               C_probe=reg.C @ PC, B=reg.B)
    sp = {}
    for tag, o in (("pert", rp), ("gesvd", rg)):
        sp[f"predict_{tag}"] = relf(o.predict(Xq), out["predict"])
        sp[f"rmse_{tag}"] = abs(cloth_rmse(o, traj, ctrl) - out["rmse"]) / out["rmse"]
        sp[f"A_{tag}"] = relf(o.A @ PA, out["A_probe"])
        sp[f"C_{tag}"] = relf(o.C @ PC, out["C_probe"])
        sp[f"B_{tag}"] = relf(o.B, out["B"])
    out["rank"], out["sv_ratio"], out["piv_ratio"] = system_stats(reg, X, Y)
    print(f"cloth gamma {gamma} m {m}: rank {out['rank']}/{m + 6} sv_ratio {out['sv_ratio']:.3e} "
          f"piv_ratio {out['piv_ratio']:.3e} spread {sp}", flush=True)
    return k, out, sp


def f15_cloth(pool):
    train, test, X, Y, _, _ = cloth_split()
    out = dict(train=train, test=test, gammas=np.array([c[0] for c in CLOTH_CASES]), ms=np.array([c[1] for c in CLOTH_CASES]),
               probe_seeds=np.array([5, 6]), bar_factor=BAR_FACTOR, n_predict=16)
    for k, o, sp in pool.map(cloth_case, range(len(CLOTH_CASES))):
        for key, v in o.items():
            out[f"c{k}_{key}"] = v
        for what in ("predict", "rmse", "A", "C", "B"):
            spread = max(sp[f"{what}_pert"], sp[f"{what}_gesvd"])
            out[f"c{k}_spread_{what}"] = spread
            out[f"c{k}_bar_{what}"] = max(BAR_FACTOR * spread, BAR_FLOOR_RMSE if what == "rmse" else BAR_FLOOR_OPS)
    np.savez_compressed(f"{OUT}/f15_spline_cloth.npz", **out)


def tps_ref(A, Bc):
    """regressors.py:225-233 verbatim: rows of the result = centres (columns of Bc), columns = points (columns of A)."""
    reg = R.KoopmanSplineRegressor(0, m=Bc.shape[1], gamma=1.0)
    reg.centers = Bc
    with np.errstate(divide="ignore", invalid="ignore"):
        return reg.lift(A)


def f15_tps():
    rng = np.random.default_rng(15)
    out = {}
    a2 = rng.uniform(-1.2, 1.2, size=(2, 70))
    c2 = np.hstack((a2[:, 3:13], rng.uniform(-1, 1, size=(2, 30))))  # 10 coincident pairs
    out["d2_points"], out["d2_centers"], out["d2_K"] = a2.T.copy(), c2.T.copy(), tps_ref(a2, c2).T.copy()
    _, _, X, _, _, _ = cloth_split()
    a192 = X[:300:7, :192].T
    c192 = np.hstack((a192[:, 5:15], X[1000:1800:40, :192].T))  # 10 coincident pairs
    out["d192_points"], out["d192_centers"], out["d192_K"] = a192.T.copy(), c192.T.copy(), tps_ref(a192, c192).T.copy()
    for k in ("d2", "d192"):
        assert np.sum(out[f"{k}_K"] == 0.0) >= 10
    np.savez_compressed(f"{OUT}/f15_spline_tps.npz", **out)


if __name__ == "__main__":
    f15_tps()
    with Pool(4) as pool:
        f15_cloth(pool)
        f15_duffing(pool)
