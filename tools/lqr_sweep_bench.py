"""The control sweep of the one-input drivers (benchmark_lqr_classic.py:256-299, benchmark_lqr_hjb.py:265-333), timed.

    python tools/lqr_sweep_bench.py [--out profiles/lqr_sweep_bench.json] [--units 200] [--steps 2000] [--reps 5]

(a) Loop cost: ONE nk_plant_loop_multi call over `units` fitted models with their own Riccati gains -- scores only, and
    with the trajectories copied back -- against `units` closed_loop_plant calls (nk_plant_loop) on the same models and gains.
    Shapes: Duffing m = 20 (f12 data) and HJB m = 100 (f8 data), `steps` steps.
(b) Whole-sweep stage split: harness.lqr_sweep against the plain loop fit -> solve_lqr -> closed_loop_plant -> NumPy scores
    over the same draws, wall time split into fit, gain (the host Riccati solve) and loop.  In the sweep the gains are solved
    in worker threads while later rounds fit: `gain_wait_s` is the wall time the sweep still waits for gains after the last
    fit, `gain_cpu_s` the host seconds summed over the solves.  Shapes: Duffing m = 20, HJB m = 100 and HJB m = 200.
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


def median_of(fn, reps):
    fn()  # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0, r))
    return statistics.median(t for t, _ in out), out[-1][1]


def shape(name):
    golden = os.path.join(ROOT, "tests", "golden")
    if name == "hjb":
        g = np.load(os.path.join(golden, "f8_hjb_config2.npz"))
        return dict(X=np.ascontiguousarray(g["X"]), Y=np.ascontiguousarray(g["Y"]), plant=nk.HJB(Ts=0.01),
                    params=dict(kernel=nk.KernelWrapper([float(g["ls"])]), gamma=float(g["gamma"])), x0=np.array([0.9]),
                    ref=np.zeros(1))
    g = np.load(os.path.join(golden, "f12_duffing_full.npz"))
    return dict(X=np.ascontiguousarray(g["X"]), Y=np.ascontiguousarray(g["Y"]), plant=nk.DuffingOscillator(Ts=0.01),
                params=dict(kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"])), x0=np.array([-0.5, 0.0]), ref=np.zeros(2))


def loop_cost(name, m, n_units, steps, reps):
    s = shape(name)
    units = harness.lqr_plan(s["X"], s["Y"], 1, s["params"], [m], list(range(n_units)))
    pool = nk._lib.lockstep_pool(32)
    regs = pool.map(lambda u: harness.lqr_fit_unit(s["X"], s["Y"], 1, s["params"], u), units)
    gain = harness.lqr_default_gain(1.0)

    def solve(r):
        try:
            return None if r is None else gain(np.asarray(r.A), np.asarray(r.B), np.asarray(r.C))
        except Exception:  # noqa: BLE001 -- a unit without a gain is left out of all three timings
            return None

    gains = list(nk._lib.worker_pool(8).map(solve, regs))
    regs, gains = [r for r, K in zip(regs, gains) if K is not None], [K for K in gains if K is not None]
    n_units = len(regs)
    u_opt = harness.hjb_optimal_control(s["x0"], steps, s["plant"])[0] if name == "hjb" else None
    args = (regs, gains, s["x0"], s["ref"], steps, s["plant"])
    t_scores, res = median_of(lambda: harness.plant_loop_multi(*args, u_opt=u_opt), reps)
    t_traj, full = median_of(lambda: harness.plant_loop_multi(*args, u_opt=u_opt, return_trajectories=True), reps)
    t_single, alone = median_of(lambda: [r.closed_loop_plant(K, s["x0"], s["ref"], steps, s["plant"]) for r, K in zip(regs, gains)],
                                reps)
    same = all(np.array_equal(full["controls"][i], alone[i][1][0]) for i in range(n_units))
    return dict(plant=name, m=m, units=n_units, steps=steps, multi_scores_only_ms=t_scores * 1e3,
                multi_with_trajectories_ms=t_traj * 1e3, single_calls_ms=t_single * 1e3,
                single_call_ms_each=t_single * 1e3 / n_units, speedup_scores_only=t_single / t_scores,
                speedup_with_trajectories=t_single / t_traj, controls_bit_identical=bool(same),
                scores_same_bits=bool(all(np.array_equal(res[k], full[k], equal_nan=True) for k in harness.SCORE_NAMES)),
                diverged_units=int(np.sum(~np.isfinite(res["u_absmax"]))))


def plain_sweep(s, m, seeds, steps, u_opt):
    """fit -> solve_lqr -> closed_loop_plant -> NumPy scores, one unit after the other; returns the stage times."""
    units = harness.lqr_plan(s["X"], s["Y"], 1, s["params"], [m], seeds)
    t_fit = t_gain = t_loop = t_score = 0.0
    J = []
    for u in units:
        t0 = time.perf_counter()
        reg = harness.lqr_fit_unit(s["X"], s["Y"], 1, s["params"], u)
        if reg is None:
            continue
        A = reg.A  # waits for the operators
        t1 = time.perf_counter()
        try:
            K = reg.solve_lqr(c=1.0)
        except Exception:  # noqa: BLE001 -- no stabilising solution: the unit is NaN in the sweep, skipped here
            continue
        t2 = time.perf_counter()
        states, us = reg.closed_loop_plant(K, s["x0"], s["ref"], steps, s["plant"])
        t3 = time.perf_counter()
        J.append(float(np.sum(np.square(states)) + np.sum(np.square(us))))
        if u_opt is not None:
            harness.control_rmse_percent(us, u_opt)
        np.max(np.abs(us))
        t4 = time.perf_counter()
        t_fit, t_gain, t_loop, t_score = t_fit + t1 - t0, t_gain + t2 - t1, t_loop + t3 - t2, t_score + t4 - t3
        del A
    return dict(fit_s=t_fit, gain_s=t_gain, loop_s=t_loop, score_s=t_score)


def sweep_split(name, m, n_seeds, steps, reps):
    s = shape(name)
    seeds = list(range(n_seeds))
    u_opt = harness.hjb_optimal_control(s["x0"], steps, s["plant"])[0] if name == "hjb" else None
    t_sweep, res = median_of(lambda: harness.lqr_sweep(s["X"], s["Y"], 1, s["params"], [m], seeds, s["plant"], s["x0"], s["ref"],
                                                       steps, u_opt=u_opt, batch=32, workers=8), reps)
    t_plain, split = median_of(lambda: plain_sweep(s, m, seeds, steps, u_opt), reps)
    tm = res["timing"]
    return dict(plant=name, m=m, seeds=n_seeds, steps=steps, sweep_s=t_sweep, sweep_fit_s=tm["fit_s"],
                sweep_gain_wait_s=tm["gain_wait_s"], sweep_gain_cpu_s=tm["gain_cpu_s"], sweep_loop_s=tm["loop_s"],
                plain_s=t_plain, plain_fit_s=split["fit_s"], plain_gain_s=split["gain_s"], plain_loop_s=split["loop_s"],
                plain_score_s=split["score_s"], plain_gain_share=split["gain_s"] / t_plain, speedup=t_plain / t_sweep,
                failed_units=int(np.sum(np.isnan(res["J"]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lqr_sweep_bench.json"))
    ap.add_argument("--units", type=int, default=200)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep-seeds", type=int, nargs=3, default=[200, 48, 16], metavar=("DUFFING20", "HJB100", "HJB200"),
                    help="seeds of the three whole-sweep shapes (the host Riccati solve at m = 200 takes most of a unit)")
    args = ap.parse_args()
    nk.get_context()
    out = dict(what="LQR control sweep: one nk_plant_loop_multi call / harness.lqr_sweep against the loops of single calls",
               timing="wall time (perf_counter) around synchronous calls, same process; median of reps after one warm-up",
               reps=args.reps, loop_cost=[], sweep_split=[])
    for name, m in (("duffing", 20), ("hjb", 100)):
        row = loop_cost(name, m, args.units, args.steps, args.reps)
        out["loop_cost"].append(row)
        print(json.dumps(row), flush=True)
    for (name, m), n_seeds in zip((("duffing", 20), ("hjb", 100), ("hjb", 200)), args.sweep_seeds):
        row = sweep_split(name, m, n_seeds, args.steps, args.reps)
        out["sweep_split"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
