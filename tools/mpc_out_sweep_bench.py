"""The MPC sweep under state limits in one call (harness.mpc_loop_multi -> nk_mpc_out_loop_multi) against what it replaces, in
one process.  The protocol of tools/mpc_sweep_bench.py.

    python tools/mpc_out_sweep_bench.py [--out profiles/mpc_out_sweep_bench.json] [--steps 1000] [--units 200] [--reps 5]

Setup: `units` units of the Duffing table (Matern-5/2 [1, 1], samples of tests/golden/f12_duffing_full.npz) dealt evenly
over m = 20 and 200 and over three controllers per model: N = 8 with 8 soft rows (the velocity limit |x_2| <= 0.3 over 8
steps, y_weight = 10 rho; nt = 16), N = 32 with 32 hard rows (x_1 <= 0.55 and the velocity limit over 16 steps; nt = 64),
and N = 8 with input limits alone (a unit WITHOUT rows in the same call); Q = C'C, |u| <= 2, rho = 300 x the default,
iters = 25, tol = 0; initial states on a circle of radius 0.5, to (0.5, 0); `steps` steps.
  (a) one mpc_loop_multi call, the ten scores only;
  (b) the same call with states, controls and info returned;
  (c) the single closed_loop_plant_mpc calls, one per unit, plus harness.mpc_out_scores on the host: what the call replaces;
  (d) per configuration with rows: closed_loop_plant_mpc with batch = units on the one model (nk_mpc_out_loop: the same kernel
      body without the table and without the scores) against one mpc_loop_multi call of `units` units of that configuration,
      scores only: the price of the indirection and of the scoring per step.
Every figure is WALL time (time.perf_counter) around calls that end in a synchronise, warm, median of `reps`, the variants
alternating within a repetition; the smallest and largest of the rounds are kept beside the median."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nys_koop_lqr_amd as nk  # noqa: E402
from nys_koop_lqr_amd import harness  # noqa: E402


def alternate(fns, reps):
    """(median, min, max) wall seconds of every callable of `fns` (a dict): one warm-up each, then `reps` rounds over all"""
    for fn in fns.values():
        fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_out_sweep_bench.json"))
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--units", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    nk.get_context()
    g = np.load(os.path.join(ROOT, "tests", "golden", "f12_duffing_full.npz"))
    X, Y = g["X"], g["Y"]
    plant = nk.PolynomialSystem.duffing(0.01)
    ref, umax, iters = np.array([0.5, 0.0]), 2.0, 25
    ang = 2 * np.pi * np.arange(args.units) / args.units
    x0s = 0.5 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    configs = []
    for m in (20, 200):
        reg = nk.KoopmanNystromRegressor(1, kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"]), m=m)
        reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, np.random.default_rng(100 + m).choice(X.shape[0], m, False)])
        reg.fit(X, Y)
        for N, rows in ((8, "soft8"), (32, "hard32"), (8, "none")):
            rho = 300.0 * reg.solve_mpc(N, c=1.0).rho
            kw = dict(c=1.0, u_min=-umax, u_max=umax, rho=rho)
            if rows == "soft8":
                ctl = reg.solve_mpc(N, x_min=[-np.inf, -0.3], x_max=[np.inf, 0.3], y_weight=10.0 * rho, **kw)
            elif rows == "hard32":
                ctl = reg.solve_mpc(N, x_min=[-np.inf, -0.3], x_max=[0.55, 0.3], y_horizon=16, **kw)
            else:
                ctl = reg.solve_mpc(N, **kw)
            configs.append(dict(m=m, N=N, rows=rows, nt=ctl.nv + getattr(ctl, "ny", 0), reg=reg, ctl=ctl))
    mix = [configs[u % len(configs)] for u in range(args.units)]
    regs, ctls = [c["reg"] for c in mix], [c["ctl"] for c in mix]

    def multi(traj):
        return harness.mpc_loop_multi(regs, ctls, x0s, ref, args.steps, plant, iters=iters, return_trajectories=traj,
                                      return_info=traj)

    def singles():
        out = []
        for c, x0 in zip(mix, x0s):
            s, u, i = c["reg"].closed_loop_plant_mpc(c["ctl"], x0, ref, args.steps, plant, iters=iters, return_info=True)
            out.append(harness.mpc_out_scores(s, u, i, c["ctl"]))
        return out

    t = alternate(dict(a=lambda: multi(False), b=lambda: multi(True), c=singles), args.reps)
    sc, host = multi(False), singles()
    same = all(sc[name][u] == host[u][name] or (sc[name][u] != sc[name][u] and host[u][name] != host[u][name])
               for u in range(args.units) for name in harness.MPC_OUT_SCORE_NAMES)
    a, b, c = t["a"][0], t["b"][0], t["c"][0]
    mixed = dict(units=args.units, steps=args.steps, iters=iters, a_scores_only_s=a, b_with_trajectories_s=b,
                 c_single_calls_and_host_scores_s=c, c_over_a=c / a, c_over_b=c / b,
                 a_min_max_s=t["a"][1:], b_min_max_s=t["b"][1:], c_min_max_s=t["c"][1:],
                 a_us_per_unit_step=a * 1e6 / (args.units * args.steps), scores_equal_host_bit_for_bit=bool(same),
                 iterations_per_step=float(np.sum(sc["iters_sum"])) / (args.units * args.steps),
                 units_with_violation=int(np.sum(sc["n_y_viol"] > 0)), y_viol_max=float(np.nanmax(sc["y_viol_max"])))
    print(json.dumps(mixed), flush=True)
    rows = []
    for c in configs:
        if c["rows"] == "none":
            continue
        one = dict(
            multi=lambda c=c: harness.mpc_loop_multi([c["reg"]] * args.units, [c["ctl"]] * args.units, x0s, ref, args.steps, plant,
                                                     iters=iters),
            batch=lambda c=c: c["reg"].closed_loop_plant_mpc(c["ctl"], x0s, ref, args.steps, plant, iters=iters))
        tt = alternate(one, args.reps)
        mu, ba = tt["multi"], tt["batch"]
        row = dict(m=c["m"], N=c["N"], rows=c["rows"], nt=c["nt"], iters=iters, units=args.units, steps=args.steps,
                   multi_scores_only_s=mu[0], batch_single_call_s=ba[0], multi_min_max_s=mu[1:], batch_min_max_s=ba[1:],
                   multi_us_per_step=mu[0] * 1e6 / args.steps, batch_us_per_step=ba[0] * 1e6 / args.steps,
                   multi_over_batch=mu[0] / ba[0], multi_over_batch_spread=[mu[1] / ba[2], mu[2] / ba[1]])
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(what="Koopman MPC sweep under state limits around the Duffing table: ONE nk_mpc_out_loop_multi call over all units "
                    "(two thirds with output rows, one third without), scored on the device, vs one nk_mpc_out_loop / nk_mpc_loop "
                    "call per unit with host scoring, and vs nk_mpc_out_loop with batch = units on one model (the same body "
                    "without the unit table and the scores)",
               timing="wall time (perf_counter) around synchronous calls; warm; median of reps, the variants alternating",
               reps=args.reps, mixed=mixed, per_configuration=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
