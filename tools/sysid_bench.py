#!/usr/bin/env python
"""Throughput of the multi-seed system-identification sweep: harness.sysid_sweep with batch in {0, 8, 32} against the
path it replaces -- the loop of reg.fit + harness.validate_dyn_sys (one launch-bound fit, one scored rollout with the
trajectory copied to the host, per unit) -- on the two shapes of the reference's experiments:

  duffing: benchmark_lqr_classic.py:211-255, n = 69 900, Matern-5/2, 20 values of m per seed.  The reference runs 200
           seeds; the fixtures hold the data set and test trajectories of seeds 0..7, so the sweep is measured on
           --duffing-seeds of them (default 8 = 160 units; landmarks drawn by the sweep's own per-seed streams).
  cloth:   benchmark_lqr_cloth.py:163-211, one seed = 10 test trajectories x 20 values of m = 200 units, d = 192.

Per configuration: one warm-up run, then --reps timed runs (wall clock around the whole call, which ends with the
device idle: every library call synchronises before it returns); units per second = units / median.  Writes
profiles/sysid_sweep_bench.json.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def duffing_problem(nk, n_seeds):
    g = dict(np.load(os.path.join(GOLDEN, "f12_duffing_full.npz")))
    seeds = list(range(n_seeds))
    return dict(X=np.ascontiguousarray(g["X"]), Y=np.ascontiguousarray(g["Y"]), n_inputs=1,
                params=dict(kernel=nk.KernelWrapper([1, 1]), gamma=float(g["gamma"])), ms=g["ms"], seeds=seeds,
                trajs=np.stack([g[f"traj_{s}"] for s in seeds]), controls=np.stack([g[f"ctrl_{s}"] for s in seeds]),
                test_index=[[i] for i in range(n_seeds)], relative=True)


def cloth_problem(nk):
    from nys_koop_lqr_amd import harness
    t = dict(np.load(os.path.join(GOLDEN, "cloth_trajs_all.npz")))
    states = t["states_e10"] / 1e10
    trajs = np.stack([states[i] for i in range(10, 50)])
    ctrls = np.stack([t["inputs"][i] for i in range(10, 50)])
    T = trajs.shape[2]
    Xa, Ya = harness.create_data_matrices(list(trajs), list(ctrls), range(40))
    order = np.arange(40)
    np.random.RandomState(0).shuffle(order)
    ranges = [(int(i) * (T - 1), (int(i) + 1) * (T - 1)) for i in order[:30]]
    return dict(X=np.ascontiguousarray(Xa.T), Y=np.ascontiguousarray(Ya.T), n_inputs=6,
                params=dict(kernel=nk.ThreeDimensionalKernel(10, 10, 10, 192), gamma=1e-7),
                ms=np.logspace(1.0, 2.6, num=20, dtype=int), seeds=[0], trajs=trajs, controls=ctrls,
                test_index={0: [int(i) for i in order[30:]]}, train_ranges={0: ranges}, extra_draws=1)


def baseline_loop(nk, prob):
    """The path the sweep replaces: fit on a copy of the seed's training rows, then harness.validate_dyn_sys."""
    from nys_koop_lqr_amd import harness
    plan_args = {k: prob[k] for k in ("X", "Y", "n_inputs", "params", "ms", "seeds", "test_index")}
    units = harness.sysid_plan(train_ranges=prob.get("train_ranges"), extra_draws=prob.get("extra_draws", 0), **plan_args)
    X, Y = prob["X"], prob["Y"]
    sets = {}
    out = []
    for u in units:
        if u["si"] not in sets:
            rows = harness.train_row_map(u["ranges"], Y.shape[0])
            sets[u["si"]] = (X, Y) if u["ranges"] is None else (np.ascontiguousarray(X[rows]), np.ascontiguousarray(Y[rows]))
        Xs, Ys = sets[u["si"]]
        reg = nk.KoopmanNystromRegressor(prob["n_inputs"], **dict(prob["params"], m=u["m"]))
        reg.nystrom_centers_output = np.ascontiguousarray(Y[u["marks"]].T)
        reg.fit(Xs, Ys)
        out.append(harness.validate_dyn_sys(reg, prob["trajs"][u["traj"]], prob["controls"][u["traj"]],
                                            relative=prob.get("relative", False)))
    return np.array(out), len(units)


def timed(fn, reps):
    fn()  # warm-up: workspaces, lock-step pools, code objects
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return times


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--duffing-seeds", type=int, default=8)
    ap.add_argument("--batches", type=int, nargs="*", default=[0, 8, 32])
    ap.add_argument("--shapes", nargs="*", default=["duffing", "cloth"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sysid_sweep_bench.json"))
    args = ap.parse_args()
    import nys_koop_lqr_amd as nk
    from nys_koop_lqr_amd import harness
    nk.get_context()
    result = dict(reps=args.reps, timing="wall clock around the whole call after one warm-up run; median of reps",
                  shapes={})
    for shape in args.shapes:
        prob = duffing_problem(nk, args.duffing_seeds) if shape == "duffing" else cloth_problem(nk)
        _, n_units = baseline_loop(nk, prob)
        entry = dict(units=n_units, n=int(prob["X"].shape[0]), d=int(prob["Y"].shape[1]), configs={})
        t = timed(lambda: baseline_loop(nk, prob), args.reps)
        entry["configs"]["baseline_fit_validate_loop"] = dict(seconds=t, units_per_s=n_units / float(np.median(t)))
        print(f"[{shape}] baseline loop: {n_units / np.median(t):.1f} units/s", flush=True)
        for b in args.batches:
            t = timed(lambda: harness.sysid_sweep(batch=b, **prob), args.reps)
            entry["configs"][f"sysid_sweep_batch{b}"] = dict(seconds=t, units_per_s=n_units / float(np.median(t)))
            print(f"[{shape}] sysid_sweep batch={b}: {n_units / np.median(t):.1f} units/s", flush=True)
        result["shapes"][shape] = entry
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({s: {c: round(v["units_per_s"], 1) for c, v in e["configs"].items()}
                      for s, e in result["shapes"].items()}))


if __name__ == "__main__":
    main()
