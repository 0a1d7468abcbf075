"""Constrained Koopman MPC closed loop: the single device launch (reg.closed_loop_plant_mpc -> nk_mpc_loop) against the host
loop it replaces (harness.mpc_control_plant: one nk_lift call and one NumPy ADMM solve per step) and against the LQR step of
nk_poly_plant_loop on the same model, in the same process.

    python tools/mpc_loop_bench.py [--out profiles/mpc_loop_bench.json] [--steps 1000] [--reps 5]

Cases: the Duffing table (Matern-5/2 [1, 1], samples of tests/golden/f12_duffing_full.npz) at m = 20 and 200, Q = 100 C'C,
horizons N = 8 and 32, |u| <= 0.3 |K e_0| with rates of 5 % of that per step, iters = 0 (the saturated LQR), 25 and 100, tol = 0,
from (-0.5, 0) to the origin.  The host loop and the device loop run the SAME `steps` steps of the same trajectory, so both
meet the same mix of steps with active limits and steps whose unconstrained move is feasible (no iteration runs there;
`iterations_per_step` is the mean the device reported, `host_iterations_per_step` the host's).  Every figure is WALL time
(time.perf_counter) around one synchronous call, median of `reps` after one warm-up call of the same shape.
Per (m, N) the two rows with iterations give two equations  t(iters) = t(0) + steps * start + iterations_run * per_iteration:
`qp_start_us_per_step` is what the QP path costs per step over the saturated mode before any iteration (the gradient with nv
columns and U_unc = -H^-1 g, on every step) and `us_per_iteration` what one ADMM iteration costs."""
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


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_loop_bench.json"))
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    nk.get_context()
    g = np.load(os.path.join(ROOT, "tests", "golden", "f12_duffing_full.npz"))
    X, Y = g["X"], g["Y"]
    plant = nk.PolynomialSystem.duffing(0.01)
    x0, ref = np.array([-0.5, 0.0]), np.zeros(2)
    rows = []
    for m in (20, 200):
        reg = nk.KoopmanNystromRegressor(1, kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"]), m=m)
        reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, np.random.default_rng(100 + m).choice(X.shape[0], m, False)])
        reg.fit(X, Y)
        K = reg.solve_lqr(c=1e2)
        e0 = (reg.lift(x0.reshape(-1, 1)) - reg.lift(ref.reshape(-1, 1))).reshape(-1)
        b = 0.3 * float(np.max(np.abs(K @ e0)))
        lqr_s = timed(lambda: reg.closed_loop_plant(K, x0, ref, args.steps, plant), args.reps)
        for N in (8, 32):
            ctl = reg.solve_mpc(N, c=1e2, u_min=-b, u_max=b, du_min=-0.05 * b, du_max=0.05 * b)
            t, ran, group = {}, {}, []
            for iters in (0, 25, 100):
                dev = lambda: reg.closed_loop_plant_mpc(ctl, x0, ref, args.steps, plant, iters=iters, return_info=True)  # noqa: E731
                host = lambda: harness.mpc_control_plant(args.steps, ref, x0, reg, ctl, plant.update_SOM, iters=iters)  # noqa: E731
                d_s, h_s = timed(dev, args.reps), timed(host, max(3, args.reps // 2))
                t[iters], ran[iters] = d_s, float(dev()[2][:, 0].sum())
                d_us, h_us = d_s * 1e6 / args.steps, h_s * 1e6 / args.steps
                group.append(dict(m=m, N=N, nv=N, iters=iters, steps=args.steps, cond_H=float(np.linalg.cond(ctl.H)), rho=ctl.rho,
                                  device_us_per_step=d_us, host_loop_us_per_step=h_us, speedup=h_us / d_us,
                                  lqr_step_us=lqr_s * 1e6 / args.steps, ratio_to_lqr_step=d_s / lqr_s,
                                  iterations_per_step=ran[iters] / args.steps,
                                  host_iterations_per_step=float(host()[2][:, 0].sum()) / args.steps))
            per_it = (t[100] - t[25]) / (ran[100] - ran[25]) if ran[100] > ran[25] else None
            start = None if per_it is None else (t[25] - t[0] - ran[25] * per_it) / args.steps
            for row in group:
                row["us_per_iteration"] = None if per_it is None else per_it * 1e6
                row["qp_start_us_per_step"] = None if start is None else start * 1e6
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = dict(what="constrained Koopman MPC closed loop around the Duffing table: one device launch (nk_mpc_loop) vs the host loop "
                    "(harness.mpc_control_plant: one nk_lift and one NumPy ADMM solve per step) and vs the LQR step of "
                    "nk_poly_plant_loop on the same model",
               timing="wall time (perf_counter) around one synchronous call; median of reps after one warm-up call",
               reps=args.reps, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
