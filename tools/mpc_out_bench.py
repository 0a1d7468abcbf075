"""Constrained Koopman MPC loop with limits on predicted states (reg.closed_loop_plant_mpc with an lqr.MPCOutputController ->
nk_mpc_out_loop) against nk_mpc_loop at the same padded lane class, in the same process, and against the host loop
(harness.mpc_control_plant) on the same steps.

    python tools/mpc_out_bench.py [--out profiles/mpc_out_bench.json] [--steps 1000] [--reps 5]

The question: does an iteration of nk_mpc_out_loop cost what an iteration of nk_mpc_loop costs at equal class?  Per class
nt = 16 / 32 / 64 the Duffing table (Matern-5/2 [1, 1], m = 40, samples of tests/golden/f12_duffing_full.npz), from (-0.5, 0)
to (0.5, 0), |u| <= 2, Q = C'C:
    out:  N = nt / 2 with nt / 2 soft rows (the velocity limit |x_2| <= 0.3 over nt / 2 steps, y_weight = 10 rho)
    in:   N = nt (nv = nt), the same box and a rate limit of 5 % of it per step
Each loop runs at iters = 25 and 100 with tol = 0; the rounds of the four calls are interleaved, the figures are the median
(and the minimum) of `reps` WALL times (time.perf_counter) around one synchronous call after one warm-up call of each shape.
us_per_iteration = (t(100) - t(25)) / (iterations run at 100 - iterations run at 25), the iterations as the device reported
them; us_per_step at 100 iterations beside it.  The host loop runs `host_steps` of the same trajectory once."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_out_bench.json"))
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--host-steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    nk.get_context()
    g = np.load(os.path.join(ROOT, "tests", "golden", "f12_duffing_full.npz"))
    X, Y = g["X"], g["Y"]
    plant = nk.PolynomialSystem.duffing(0.01)
    x0, ref, m, umax = np.array([-0.5, 0.0]), np.array([0.5, 0.0]), 40, 2.0
    reg = nk.KoopmanNystromRegressor(1, kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"]), m=m)
    reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, np.random.default_rng(100 + m).choice(X.shape[0], m, False)])
    reg.fit(X, Y)
    rows = []
    for nt in (16, 32, 64):
        rho = 300.0 * reg.solve_mpc(nt // 2, c=1.0).rho
        ctl_out = reg.solve_mpc(nt // 2, c=1.0, u_min=-umax, u_max=umax, rho=rho, x_min=[-np.inf, -0.3], x_max=[np.inf, 0.3],
                                y_weight=10.0 * rho)
        ctl_in = reg.solve_mpc(nt, c=1.0, u_min=-umax, u_max=umax, du_min=-0.05 * umax, du_max=0.05 * umax)
        assert ctl_out.nv + ctl_out.ny == nt and ctl_in.nv == nt
        calls = {(name, it): (lambda c=c, it=it: reg.closed_loop_plant_mpc(c, x0, ref, args.steps, plant, iters=it, return_info=True))
                 for name, c in (("out", ctl_out), ("in", ctl_in)) for it in (25, 100)}
        ran = {k: float(fn()[2][:, 0].sum()) for k, fn in calls.items()}  # (the warm-up call of each shape)
        ts = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                ts[k].append(time.perf_counter() - t0)
        row = dict(nt=nt, m=m, steps=args.steps, reps=args.reps)
        for name in ("out", "in"):
            for stat, f in (("median", statistics.median), ("min", min)):
                t25, t100 = f(ts[(name, 25)]), f(ts[(name, 100)])
                row[f"{name}_us_per_step_100_{stat}"] = t100 * 1e6 / args.steps
                row[f"{name}_us_per_iteration_{stat}"] = (t100 - t25) * 1e6 / (ran[(name, 100)] - ran[(name, 25)])
            row[f"{name}_iterations_per_step_100"] = ran[(name, 100)] / args.steps
        row["iteration_ratio_out_over_in_median"] = row["out_us_per_iteration_median"] / row["in_us_per_iteration_median"]
        t0 = time.perf_counter()
        harness.mpc_control_plant(args.host_steps, ref, x0, reg, ctl_out, plant.update_SOM, iters=100)
        row["host_loop_us_per_step_100"] = (time.perf_counter() - t0) * 1e6 / args.host_steps
        row["host_steps"] = args.host_steps
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(what="nk_mpc_out_loop (nv = ny = nt / 2) vs nk_mpc_loop (nv = nt) at the same lane class on the Duffing table, m = 40, "
                    "and the host loop harness.mpc_control_plant with the output controller",
               timing="wall time (perf_counter) around one synchronous call; interleaved rounds, median and minimum of reps after "
                      "one warm-up call per shape; per iteration from the difference of the 100- and 25-iteration loops",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
