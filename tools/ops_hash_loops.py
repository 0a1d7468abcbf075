#!/usr/bin/env python3
"""SHA-256 of what the single-launch closed loops return (library given by NYSKOOP_LIB): nk_plant_loop, nk_poly_plant_loop,
nk_mpc_loop, nk_mpc_out_loop and their multi forms, on models rebuilt from host copies, 30 steps each.  States, controls,
info and scores are hashed separately; two builds that compute the same bits print the same lines.  tools/ops_hash.py runs
these cases after its own; run this file for the loops alone.

Sizes: the plant loops at m = 40, 64 | 65 (one | four landmarks per lane), 256 | 257 (one | two waves) and 300 around the
Duffing and HJB plants, every kernel family at m = 65; the polynomial loops at (d, p) = (2, 1), (2, 2), (4, 4), m = 20, 64 | 65
and 200, batch 3; the MPC loops at nv = 8, 24, 40 (lane classes 16 / 32 / 64), m = 20, 64 | 65 and 200, iters = 0 and 25, tight and
loose limits, a NaN initial state, with and without a seed control; the loops with output rows at ny = 2, hard and soft, nt = 10
and 26, with a NaN unit, a unit without rows, and the multi call once more with scores alone."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import _lib

STEPS = 30
h = lambda *a: hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in a)).hexdigest()[:16]
fin = lambda *a: int(sum(np.isfinite(x).sum() for x in a))


def rebuilt(family, m, p, d, seed):
    """Random stable operators on random landmarks: A = 0.9 x orthogonal, B and C of order one."""
    r = np.random.default_rng(seed)
    if family == "tps":
        reg = nk.KoopmanSplineRegressor(p, m=m, gamma=1e-6)
        reg.centers = r.standard_normal((d, m))
    else:
        kern = {"matern": lambda: nk.KernelWrapper(np.ones(d)), "rbf": lambda: nk.ThreeDimensionalKernel(0.7, 0.7, 0.7, d),
                "linear": lambda: nk.LinearKernelWrapper(1.0)}[family]()
        reg = nk.KoopmanNystromRegressor(p, kernel=kern, gamma=1e-6, m=m)
        reg.nystrom_centers_output = r.standard_normal((d, m))
    Q, _ = np.linalg.qr(r.standard_normal((m, m)))
    reg.A, reg.B, reg.C = 0.9 * Q, 0.3 * r.standard_normal((m, p)) / np.sqrt(m), r.standard_normal((d, m))
    return reg, r


def plant_loops(ctx):
    for name, plant, d in (("duffing", nk.DuffingOscillator(Ts=0.01), 2), ("hjb", nk.HJB(Ts=0.01), 1)):
        cases = [("matern", m) for m in (40, 64, 65, 256, 257, 300)]
        if d == 2:
            cases += [(fam, 65) for fam in ("rbf", "linear", "tps")]
        units = [rebuilt(fam, m, 1, d, 100 + 7 * m + len(fam)) for fam, m in cases]
        gains = [0.1 * r.standard_normal((1, m)) for (reg, r), (_, m) in zip(units, cases)]
        x0s = [0.5 * r.uniform(-1.0, 1.0, (3, d)) for reg, r in units]
        ref = 0.1 * np.ones(d)
        for (fam, m), (reg, _), K, x0 in zip(cases, units, gains, x0s):
            ox, ou = reg.closed_loop_plant(K, x0, ref, STEPS, plant)
            print("plant_loop", name, fam, m, "batch 3: states", h(ox), "controls", h(ou), "finite", fin(ox, ou), flush=True)
        u_opt = np.stack([np.linspace(-1.0, 1.0, STEPS), np.cos(np.arange(STEPS))])
        rows = [(-1, 0, 1)[k % 3] for k in range(len(units))]
        sc, ox, ou = ctx.plant_loop_multi(plant.plant_id, plant.Ts, STEPS, [reg._ensure_model() for reg, _ in units], gains,
                                          np.stack([x[0] for x in x0s]), np.tile(ref, (len(units), 1)), u_opt=u_opt, uopt_rows=rows,
                                          want_x=True, want_u=True)
        print("plant_loop_multi", name, len(units), "units: states", h(ox), "controls", h(ou), "scores", h(sc), "finite",
              fin(ox, ou, sc), flush=True)
        sc2, _, _ = ctx.plant_loop_multi(plant.plant_id, plant.Ts, STEPS, [reg._ensure_model() for reg, _ in units][::-1], gains[::-1],
                                         np.stack([x[0] for x in x0s])[::-1], np.tile(ref, (len(units), 1)), u_opt=u_opt,
                                         uopt_rows=rows[::-1])
        print("plant_loop_multi", name, "reversed, scores alone:", h(sc2), "same", bool(np.array_equal(sc2[::-1], sc, equal_nan=True)),
              flush=True)


POLY = {
    (2, 1): [(0, 1.0, (0, 1), (0,)), (1, -1.0, (1, 0), (0,)), (1, -0.5, (0, 1), (0,)), (1, -1.0, (3, 0), (0,)), (1, 1.0, (0, 0), (1,))],
    (2, 2): [(0, 1.0, (0, 1), (0, 0)), (0, 0.5, (0, 0), (0, 1)), (1, -1.0, (1, 0), (0, 0)), (1, -0.5, (0, 1), (0, 0)),
             (1, -1.0, (3, 0), (0, 0)), (1, 1.0, (0, 0), (1, 0)), (1, 0.1, (1, 0), (0, 1))],
    (4, 4): [(0, 1.0, (0, 1, 0, 0), ()), (0, 0.3, (), (0, 0, 1, 0)), (1, -1.0, (1, 0, 0, 0), ()), (1, -0.5, (0, 1, 0, 0), ()),
             (1, -1.0, (3, 0, 0, 0), ()), (1, 0.2, (0, 0, 1, 0), ()), (1, 1.0, (), (1, 0, 0, 0)), (2, 1.0, (0, 0, 0, 1), ()),
             (2, 0.3, (), (0, 0, 0, 1)), (3, -1.0, (0, 0, 1, 0), ()), (3, -0.5, (0, 0, 0, 1), ()), (3, -1.0, (0, 0, 2, 1), ()),
             (3, 0.2, (1, 0, 0, 0), ()), (3, 1.0, (), (0, 1, 0, 0)), (3, 0.1, (0, 1, 0, 0), (0, 0, 1, 1))],
}


def poly_loops(ctx):
    for (d, p), terms in POLY.items():
        plant = nk.PolynomialSystem(d, p, terms, 0.01)
        ms = (20, 64, 65, 200)
        fams = ("matern", "rbf", "matern", "tps")
        units = [rebuilt(fam, m, p, d, 200 + 5 * m + 10 * d + p) for fam, m in zip(fams, ms)]
        gains = [0.1 * r.standard_normal((p, m)) for (reg, r), m in zip(units, ms)]
        x0s = [0.5 * r.uniform(-1.0, 1.0, (3, d)) for reg, r in units]
        ref = 0.1 * np.ones(d)
        for fam, m, (reg, _), K, x0 in zip(fams, ms, units, gains, x0s):
            ox, ou = reg.closed_loop_plant(K, x0, ref, STEPS, plant)
            print("poly_plant_loop", (d, p), fam, m, "batch 3: states", h(ox), "controls", h(ou), "finite", fin(ox, ou), flush=True)
        u_opt = np.random.default_rng(d + p).standard_normal((2, STEPS, p))
        sc, ox, ou = ctx.poly_plant_loop_multi(plant.descriptor(), STEPS, [reg._ensure_model() for reg, _ in units], gains,
                                               np.stack([x[1] for x in x0s]), np.tile(ref, (4, 1)), u_opt=u_opt,
                                               uopt_rows=[0, 1, -1, 0], want_x=True, want_u=True)
        print("poly_plant_loop_multi", (d, p), "m", ms, ": states", h(ox), "controls", h(ou), "scores", h(sc), "finite",
              fin(ox, ou, sc), flush=True)


def mpc_loops(ctx):
    plant = nk.PolynomialSystem.duffing(0.01)
    ms, Ns = (20, 64, 65, 200), (8, 24, 40)
    fams = ("matern", "rbf", "matern", "tps")
    regs = {m: rebuilt(fam, m, 1, 2, 300 + m)[0] for fam, m in zip(fams, ms)}
    limits = {"loose": dict(u_min=-2.0, u_max=2.0, du_min=-0.5, du_max=0.5), "tight": dict(u_min=-0.05, u_max=0.05, du_min=-0.01, du_max=0.01)}
    ctl = {(m, N, lim): regs[m].solve_mpc(N, c=1.0, **kw) for m in ms for N in Ns for lim, kw in limits.items() if lim == "loose" or N == 24}
    assert sorted({c.nv for c in ctl.values()}) == [8, 24, 40]
    x0 = np.array([[-0.5, 0.0], [0.3, -0.2], [float("nan"), 0.1]])
    ref = np.array([0.5, 0.0])
    units = []  # (m, N, limits, iters, x0, u_init)
    for m in ms:
        for N in Ns:
            for lim in (("loose", "tight") if N == 24 else ("loose",)):
                for iters in ((0, 25) if N == 8 else (25,)):
                    ui = np.array([0.02]) if (m + N + iters) % 2 else None
                    ox, ou, oi = regs[m].closed_loop_plant_mpc(ctl[(m, N, lim)], x0, ref, STEPS, plant, iters=iters, u_init=ui, return_info=True)
                    print("mpc_loop m", m, "nv", N, lim, "iters", iters, "seed", ui is not None, "batch 3 (one NaN): states", h(ox),
                          "controls", h(ou), "info", h(oi), "finite", fin(ox, ou, oi), "iterations", float(np.nansum(oi[:, :, 0])),
                          flush=True)
                    units += [(m, N, lim, iters, x0[k], ui) for k in ((0, 2) if lim == "tight" and N == 24 else (1,))]
    pairs = [_lib.mpc_desc(ctl[(m, N, lim)], iters, 1e-9 if k % 5 == 0 else 0.0) for k, (m, N, lim, iters, _, _) in enumerate(units)]
    u_opt = np.random.default_rng(9).standard_normal((2, STEPS, 1))
    rows = [(0, -1, 1)[k % 3] for k in range(len(units))]
    args = (plant.descriptor(), STEPS, [regs[u[0]]._ensure_model() for u in units], [ds for ds, _ in pairs], np.stack([u[4] for u in units]),
            np.tile(ref, (len(units), 1)))
    sc, ox, ou, oi = ctx.mpc_loop_multi(*args, u_inits=[u[5] for u in units], u_opt=u_opt, uopt_rows=rows, want_x=True, want_u=True,
                                        want_info=True)
    print("mpc_loop_multi", len(units), "units: states", h(ox), "controls", h(ou), "info", h(oi), "scores", h(sc), "finite",
          fin(ox, ou, oi, sc), "at a limit", float(np.nansum(sc[:, 6])), flush=True)
    sc2 = ctx.mpc_loop_multi(*args, u_inits=[u[5] for u in units], u_opt=u_opt, uopt_rows=rows)[0]
    print("mpc_loop_multi scores alone:", h(sc2), "same", bool(np.array_equal(sc, sc2, equal_nan=True)), flush=True)
    del pairs


def mpc_out_loops(ctx):
    plant = nk.PolynomialSystem.duffing(0.01)
    regs = {m: rebuilt("matern", m, 1, 2, 400 + m)[0] for m in (20, 65)}
    ctl = {}
    for m, reg in regs.items():
        for N in (8, 24):
            rho = 300.0 * reg.solve_mpc(N, c=1.0).rho
            kw = dict(c=1.0, u_min=-2.0, u_max=2.0, rho=rho, x_min=[-np.inf, -0.3], x_max=[np.inf, 0.3], y_horizon=2)
            ctl[(m, N, "hard")] = reg.solve_mpc(N, **kw)
            ctl[(m, N, "soft")] = reg.solve_mpc(N, y_weight=10.0 * rho, **kw)
            ctl[(m, N, "none")] = reg.solve_mpc(N, c=1.0, u_min=-2.0, u_max=2.0, rho=rho)
    assert all(c.ny == 2 for k, c in ctl.items() if k[2] != "none") and sorted({c.nv for c in ctl.values()}) == [8, 24]
    x0 = np.array([[-0.5, 0.0], [0.3, -0.5], [0.2, float("nan")]])
    ref = np.array([0.5, 0.0])
    units = []  # (m, controller, x0, u_init)
    for (m, N, kind), c in ctl.items():
        if kind == "none":
            units.append((m, c, x0[0], None))
            continue
        ui = np.array([-0.1]) if N == 24 else None
        ox, ou, oi = regs[m].closed_loop_plant_mpc(c, x0, ref, STEPS, plant, iters=25, u_init=ui, return_info=True)
        print("mpc_out_loop m", m, "nv", N, "ny 2", kind, "seed", ui is not None, "batch 3 (one NaN): states", h(ox), "controls", h(ou),
              "info", h(oi), "finite", fin(ox, ou, oi), flush=True)
        units += [(m, c, x0[k], ui) for k in ((1, 2) if (m, N) == (65, 8) else (1,))]
    pairs = [_lib.mpc_desc(c, 25, 0.0) for _, c, _, _ in units]
    opairs = [_lib.mpc_out(c) if hasattr(c, "ycomp") else (None, None) for _, c, _, _ in units]
    u_opt = np.random.default_rng(10).standard_normal((2, STEPS, 1))
    rows = [(1, 0, -1)[k % 3] for k in range(len(units))]
    args = (plant.descriptor(), STEPS, [regs[u[0]]._ensure_model() for u in units], [ds for ds, _ in pairs], np.stack([u[2] for u in units]),
            np.tile(ref, (len(units), 1)))
    kw = dict(u_inits=[u[3] for u in units], u_opt=u_opt, uopt_rows=rows, outs=[o for o, _ in opairs])
    sc, ox, ou, oi = ctx.mpc_loop_multi(*args, want_x=True, want_u=True, want_info=True, **kw)
    print("mpc_out_loop_multi", len(units), "units: states", h(ox), "controls", h(ou), "info", h(oi), "scores", h(sc), "finite",
          fin(ox, ou, oi, sc), "steps past a limit", float(np.nansum(sc[:, 9])), flush=True)
    sc2 = ctx.mpc_loop_multi(*args, **kw)[0]
    print("mpc_out_loop_multi scores alone:", h(sc2), "same", bool(np.array_equal(sc, sc2, equal_nan=True)), flush=True)
    del pairs, opairs


def main():
    ctx = nk.get_context()
    plant_loops(ctx)
    poly_loops(ctx)
    mpc_loops(ctx)
    mpc_out_loops(ctx)


if __name__ == "__main__":
    main()
