"""The MPC control sweep in one call (harness.mpc_loop_multi -> nk_mpc_loop_multi) against what it replaces, in one process.

    python tools/mpc_sweep_bench.py [--out profiles/mpc_sweep_bench.json] [--steps 1000] [--units 200] [--reps 5]

Setup: `units` units of the Duffing table (Matern-5/2 [1, 1], samples of tests/golden/f12_duffing_full.npz) dealt evenly
over m = 20 and 200, horizons N = 8 and 32 and iters = 0 (the saturated LQR) and 25; Q = 100 C'C, |u| <= 0.3 |K e_0| with rates of
5 % of that per step, tol = 0; initial states on a circle of radius 0.5, to the origin; `steps` steps.
  (a) one mpc_loop_multi call, scores only;
  (b) the same call with states, controls and info returned;
  (c) the single closed_loop_plant_mpc calls, one per unit, plus harness.mpc_scores on the host: what the call replaces;
  (d) per (m, N, iters): closed_loop_plant_mpc with batch = units on the one model (the same kernel body without the table and
      without the scores) against one mpc_loop_multi call of `units` units of that configuration, scores only: the price of
      the indirection and of the scoring per step.
Every figure is WALL time (time.perf_counter) around calls that end in a synchronise, warm, median of `reps`, the variants
alternating within a repetition."""
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
    """median wall seconds of every callable of `fns` (a dict), one warm-up each, then `reps` rounds over all of them"""
    for fn in fns.values():
        fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    return {k: statistics.median(v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_sweep_bench.json"))
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--units", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    nk.get_context()
    g = np.load(os.path.join(ROOT, "tests", "golden", "f12_duffing_full.npz"))
    X, Y = g["X"], g["Y"]
    plant = nk.PolynomialSystem.duffing(0.01)
    ref = np.zeros(2)
    ang = 2 * np.pi * np.arange(args.units) / args.units
    x0s = 0.5 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    configs = []
    for m in (20, 200):
        reg = nk.KoopmanNystromRegressor(1, kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"]), m=m)
        reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, np.random.default_rng(100 + m).choice(X.shape[0], m, False)])
        reg.fit(X, Y)
        K = reg.solve_lqr(c=1e2)
        e0 = (reg.lift(np.array([[-0.5], [0.0]])) - reg.lift(ref.reshape(-1, 1))).reshape(-1)
        b = 0.3 * float(np.max(np.abs(K @ e0)))
        for N in (8, 32):
            ctl = reg.solve_mpc(N, c=1e2, u_min=-b, u_max=b, du_min=-0.05 * b, du_max=0.05 * b)
            configs += [dict(m=m, N=N, iters=it, reg=reg, ctl=ctl) for it in (0, 25)]
    mix = [configs[u % len(configs)] for u in range(args.units)]
    regs, ctls, its = [c["reg"] for c in mix], [c["ctl"] for c in mix], [c["iters"] for c in mix]

    def multi(traj):
        return harness.mpc_loop_multi(regs, ctls, x0s, ref, args.steps, plant, iters=its, return_trajectories=traj,
                                      return_info=traj)

    def singles():
        out = []
        for c, x0 in zip(mix, x0s):
            s, u, i = c["reg"].closed_loop_plant_mpc(c["ctl"], x0, ref, args.steps, plant, iters=c["iters"], return_info=True)
            out.append(harness.mpc_scores(s, u, i, c["ctl"]))
        return out

    t = alternate(dict(a=lambda: multi(False), b=lambda: multi(True), c=singles), args.reps)
    sc, host = multi(False), singles()
    same = all(sc[name][u] == host[u][name] or (sc[name][u] != sc[name][u] and host[u][name] != host[u][name])
               for u in range(args.units) for name in harness.MPC_SCORE_NAMES)
    mixed = dict(units=args.units, steps=args.steps, a_scores_only_s=t["a"], b_with_trajectories_s=t["b"],
                 c_single_calls_and_host_scores_s=t["c"], c_over_a=t["c"] / t["a"], c_over_b=t["c"] / t["b"],
                 a_us_per_unit_step=t["a"] * 1e6 / (args.units * args.steps), scores_equal_host_bit_for_bit=bool(same),
                 iterations_per_step=float(np.sum(sc["iters_sum"])) / (args.units * args.steps))
    print(json.dumps(mixed), flush=True)
    rows = []
    for c in configs:
        one = dict(
            multi=lambda c=c: harness.mpc_loop_multi([c["reg"]] * args.units, [c["ctl"]] * args.units, x0s, ref, args.steps, plant,
                                                     iters=c["iters"]),
            batch=lambda c=c: c["reg"].closed_loop_plant_mpc(c["ctl"], x0s, ref, args.steps, plant, iters=c["iters"]))
        tt = alternate(one, args.reps)
        row = dict(m=c["m"], N=c["N"], iters=c["iters"], units=args.units, steps=args.steps, multi_scores_only_s=tt["multi"],
                   batch_single_call_s=tt["batch"], multi_us_per_step=tt["multi"] * 1e6 / args.steps,
                   batch_us_per_step=tt["batch"] * 1e6 / args.steps, multi_over_batch=tt["multi"] / tt["batch"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(what="constrained Koopman MPC sweep around the Duffing table: ONE nk_mpc_loop_multi call over all units, scored on "
                    "the device, vs one nk_mpc_loop call per unit with host scoring, and vs nk_mpc_loop with batch = units on one "
                    "model (the same body without the unit table and the scores)",
               timing="wall time (perf_counter) around synchronous calls; warm; median of reps, the variants alternating",
               reps=args.reps, mixed=mixed, per_configuration=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
