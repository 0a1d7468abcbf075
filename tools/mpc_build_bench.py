"""The controllers of an MPC sweep built on the device in one call (regressors._mpc_build_batch ->
nk_model_mpc_build_batch) against what it replaces, in one process.

    python tools/mpc_build_bench.py [--out profiles/mpc_build_bench.json] [--units 200] [--reps 5] [--steps 1000]

Setup: the Duffing data of tools/mpc_sweep_bench.py (Matern-5/2 [1, 1], samples of tests/golden/f12_duffing_full.npz), but
every unit with its OWN fit: `units` units dealt evenly over m = 20 and 200 (landmarks drawn per unit) and the horizons N = 8
and 32; Q = 100 C'C, |u| <= 0.3, rates of 5 % of that per step.
  (a) reg.solve_mpc per unit on 4 host threads (scipy's Riccati solve, two Lyapunov solves, the Python loops of
      lqr.mpc_condense): what harness.lqr_sweep(controller=...) does today;
  (b) the same on 16 host threads;
  (c) ONE device build call over all units (nk_model_mpc_build_batch takes the horizon per unit), the bounds and rho on the
      host as reg.solve_mpc(device=True) forms them;
  (d) the mpc_loop_multi call that follows (iters = 25, `steps` steps), for scale.
Every figure is WALL time (time.perf_counter) around calls that end in a synchronise, warm, median of `reps`, the variants
alternating within a repetition.  Also recorded: the device time of the Riccati launch and of the build launch of (c), by
device events (nk_mpc_build_times), and the largest H / F / K difference between (a) and (c), max |X_c - X_a| / max |X_a|."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nys_koop_lqr_amd as nk  # noqa: E402
from nys_koop_lqr_amd import harness, regressors  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_build_bench.json"))
    ap.add_argument("--units", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000)
    args = ap.parse_args()
    ctx = nk.get_context()
    g = np.load(os.path.join(ROOT, "tests", "golden", "f12_duffing_full.npz"))
    X, Y = g["X"], g["Y"]
    plant = nk.PolynomialSystem.duffing(0.01)
    ref = np.zeros(2)
    c, b = 1e2, 0.3
    limits = dict(u_min=-b, u_max=b, du_min=-0.05 * b, du_max=0.05 * b)
    units = []
    t0 = time.perf_counter()
    for u in range(args.units):
        m, N = (20, 200)[u % 2], (8, 32)[(u // 2) % 2]
        reg = nk.KoopmanNystromRegressor(1, kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"]), m=m)
        reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, np.random.default_rng(1000 + u).choice(X.shape[0], m, False)])
        reg.fit(X, Y)
        units.append(dict(m=m, N=N, reg=reg))
    print(json.dumps(dict(fits=args.units, fit_s=time.perf_counter() - t0)), flush=True)

    def host(workers):
        with ThreadPoolExecutor(workers) as pool:
            return list(pool.map(lambda u: u["reg"].solve_mpc(u["N"], c=c, **limits), units))

    times = dict(ms_riccati=0.0, ms_build=0.0)
    regs = [u["reg"] for u in units]

    def device():
        """what reg.solve_mpc(device=True) does, for all units at once: the checked limits, ONE build call, the controllers"""
        lims = [regressors._mpc_limits(u["reg"], u["N"], limits["u_min"], limits["u_max"], limits["du_min"], limits["du_max"],
                                       None, None, None, device=True) for u in units]
        built, status, _ = regressors._mpc_build_batch(regs, c, None, [(u["N"], lim["comps"], lim["Ny"])
                                                                       for u, lim in zip(units, lims)])
        assert np.all(status == 0), status
        times.update(ctx.mpc_build_times())
        return [regressors._mpc_controller(bu, lim, u["N"], None, np.inf) for bu, lim, u in zip(built, lims, units)]

    ang = 2 * np.pi * np.arange(args.units) / args.units
    x0s = 0.5 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    built = device()

    def loop():
        return harness.mpc_loop_multi(regs, built, x0s, ref, args.steps, plant, iters=25)

    fns = dict(a=lambda: host(4), b=lambda: host(16), c=device, d=loop)
    ts = {k: [] for k in fns}
    for rep in range(-1, args.reps):  # rep -1: the warm-up round
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if rep >= 0:
                ts[k].append(dt)
            print(json.dumps(dict(rep=rep, variant=k, s=dt)), flush=True)
    med = {k: statistics.median(v) for k, v in ts.items()}
    ctl_a, ctl_c = host(4), device()
    diff = {k: max(float(np.max(np.abs(getattr(cc, k) - getattr(ca, k))) / np.max(np.abs(getattr(ca, k))))
                   for ca, cc in zip(ctl_a, ctl_c)) for k in ("H", "F", "K")}
    out = dict(what="the controllers of an MPC sweep over the Duffing table, every unit with its own fit: reg.solve_mpc per unit "
                    "on host threads vs ONE nk_model_mpc_build_batch call",
               timing="wall time (perf_counter) around synchronous calls; warm; median of reps, the variants alternating",
               units=args.units, reps=args.reps, ms=[20, 200], horizons=[8, 32], c=c,
               a_host_4_threads_s=med["a"], b_host_16_threads_s=med["b"], c_device_build_s=med["c"],
               d_mpc_loop_multi_s=med["d"], loop_steps=args.steps, a_over_c=med["a"] / med["c"], b_over_c=med["b"] / med["c"],
               c_device_ms_riccati_launches=times["ms_riccati"], c_device_ms_build_launches=times["ms_build"],
               max_relative_difference_a_vs_c=diff, all_samples_s=ts,
               cpu_threads_blas=os.environ.get("OMP_NUM_THREADS"))
    print(json.dumps({k: v for k, v in out.items() if k != "all_samples_s"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
