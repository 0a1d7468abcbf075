"""The control branch of the cloth driver (benchmark_lqr_cloth.py:213-270), timed.

    python tools/cloth_lqr_sweep_bench.py [--out profiles/cloth_lqr_sweep_bench.json] [--units 100] [--seeds 10] [--reps 5]

(a) Loop cost: ONE nk_closed_loop_multi call over `units` fitted models (m = 100, p = 6, d = 192, 60 steps) with their own
    Riccati gains -- scores only, and with the trajectories copied back -- against the `units` reg.closed_loop calls
    (nk_closed_loop) it replaces, on the same models, gains and lifted states.
(b) Whole sweep: harness.cloth_lqr_sweep over `seeds` seeds x {Nystrom, splines} against the plain loop fit -> solve_lqr ->
    harness.lqr_control over the same draws, wall time split into fit / gain / loop.
Everything runs in one process.  Every figure is WALL time (time.perf_counter) around synchronous calls, the median of
`reps` timings after one warm-up of the same shape."""
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

STEPS, M, C_COST = 60, 100, 0.0075
NODES = [168, 169, 170, 189, 190, 191]


def median_of(fn, reps):
    fn()  # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0, r))
    return statistics.median(t for t, _ in out), out[-1][1]


def cloth():
    golden = os.path.join(ROOT, "tests", "golden")
    t = np.load(os.path.join(golden, "cloth_trajs_all.npz"))
    g = np.load(os.path.join(golden, "f10_lqr_control.npz"))
    states, inputs = t["states_e10"] / 1e10, t["inputs"]
    X = np.ascontiguousarray(np.hstack([np.vstack((states[i][:, :-1], inputs[i][:, :-1])) for i in range(10, 40)]).T)
    Y = np.ascontiguousarray(np.hstack([states[i][:, 1:] for i in range(10, 40)]).T)
    params = dict(nystrom=dict(kernel=nk.ThreeDimensionalKernel(*g["ls"], 192), gamma=float(g["gamma"])),
                  spline=dict(gamma=float(g["gamma"])))
    return dict(X=X, Y=Y, params=params, x0=g["initial_state"].reshape(-1), x_ref=g["reference_lqr"].reshape(-1))


def loop_cost(s, n_units, reps):
    names, units = harness.cloth_lqr_plan(s["X"], s["Y"], 6, s["params"], M, list(range(n_units // 2)), ("nystrom", "spline"))
    both = np.stack((s["x0"], s["x_ref"]), axis=1)
    regs, gains, lifts, _ = harness.lqr_fit_and_gain(s["X"], s["Y"], 6, None, units, c=C_COST, batch=32, workers=8,
                                                     after_fit=lambda reg, u: reg.lift(both))
    live = [i for i in range(len(units)) if gains[i] is not None]
    regs, gains = [regs[i] for i in live], [gains[i] for i in live]
    lifts = [(np.ascontiguousarray(lifts[i][:, 0]), np.ascontiguousarray(lifts[i][:, 1])) for i in live]
    n = len(regs)
    targets, u_inits = [s["x_ref"]] * n, [s["x0"][NODES]] * n
    args = (regs, gains, lifts, targets, STEPS, C_COST, u_inits)
    t_scores, res = median_of(lambda: harness.closed_loop_multi_lifted(*args), reps)
    t_traj, full = median_of(lambda: harness.closed_loop_multi_lifted(*args, return_trajectories=True), reps)
    t_single, alone = median_of(lambda: [r.closed_loop(K, f[0], f[1], STEPS) for r, K, f in zip(regs, gains, lifts)], reps)
    worst = max(float(np.linalg.norm(full["states"][i].T - alone[i][0]) / np.linalg.norm(alone[i][0])) for i in range(n))
    return dict(units=n, m=M, p=6, d=192, steps=STEPS, multi_scores_only_ms=t_scores * 1e3,
                multi_with_trajectories_ms=t_traj * 1e3, single_calls_ms=t_single * 1e3,
                single_call_ms_each=t_single * 1e3 / n, speedup_scores_only=t_single / t_scores,
                speedup_with_trajectories=t_single / t_traj, scores_only_faster_than_single_calls=bool(t_scores < t_single),
                worst_relF_states_vs_single=worst,
                scores_same_bits=bool(all(np.array_equal(res[k], full[k], equal_nan=True) for k in harness.LOOP_SCORE_NAMES)),
                diverged_units=int(np.sum(~np.isfinite(res["u_absmax"]))))


def plain_sweep(s, seeds):
    """fit -> solve_lqr -> harness.lqr_control, one unit after the other; returns the stage times."""
    _, units = harness.cloth_lqr_plan(s["X"], s["Y"], 6, s["params"], M, seeds, ("nystrom", "spline"))
    t_fit = t_gain = t_loop = 0.0
    for u in units:
        t0 = time.perf_counter()
        reg = harness.lqr_fit_unit(s["X"], s["Y"], 6, u["params"], u, u["estimator"])
        if reg is None:
            continue
        A = reg.A  # waits for the operators
        t1 = time.perf_counter()
        try:
            K = reg.solve_lqr(c=C_COST)
        except Exception:  # noqa: BLE001 -- no stabilising solution: the unit is NaN in the sweep, skipped here
            continue
        t2 = time.perf_counter()
        x_s, y_s, z_s, us = harness.lqr_control(STEPS, s["x_ref"], s["x0"], reg, K)
        np.sqrt(np.mean(np.square(np.stack((x_s, y_s, z_s), axis=1).reshape(192, -1)[:, 1:] - s["x_ref"][:, None]), axis=0))
        t3 = time.perf_counter()
        t_fit, t_gain, t_loop = t_fit + t1 - t0, t_gain + t2 - t1, t_loop + t3 - t2
        del A
    return dict(fit_s=t_fit, gain_s=t_gain, loop_s=t_loop)


def sweep_split(s, n_seeds, reps, gain):
    seeds = list(range(n_seeds))
    t_sweep, res = median_of(lambda: harness.cloth_lqr_sweep(s["X"], s["Y"], 6, s["params"], M, seeds, s["x0"], s["x_ref"], STEPS,
                                                             estimator=("nystrom", "spline"), gain=gain, batch=32, workers=8),
                             reps)
    t_plain, split = median_of(lambda: plain_sweep(s, seeds), reps)
    tm = res["timing"]
    return dict(seeds=n_seeds, units=2 * n_seeds, gain=gain, sweep_s=t_sweep, sweep_fit_s=tm["fit_s"],
                sweep_gain_wait_s=tm["gain_wait_s"], sweep_gain_cpu_s=tm["gain_cpu_s"], sweep_loop_s=tm["loop_s"],
                plain_s=t_plain, plain_fit_s=split["fit_s"], plain_gain_s=split["gain_s"], plain_loop_s=split["loop_s"],
                speedup=t_plain / t_sweep, failed_units=int(np.sum(np.isnan(res["J"]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloth_lqr_sweep_bench.json"))
    ap.add_argument("--units", type=int, default=100)
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    nk.get_context()
    s = cloth()
    out = dict(what="cloth LQR sweep: one nk_closed_loop_multi call / harness.cloth_lqr_sweep against the loops of single calls",
               timing="wall time (perf_counter) around synchronous calls, same process; median of reps after one warm-up",
               reps=args.reps, loop_cost=[], sweep_split=[])
    row = loop_cost(s, args.units, args.reps)
    out["loop_cost"].append(row)
    print(json.dumps(row), flush=True)
    for gain in ("host", "device"):
        row = sweep_split(s, args.seeds, args.reps, gain)
        out["sweep_split"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
