"""Plant-in-the-loop LQR closed loop: the single device launch (KoopmanNystromRegressor.closed_loop_plant -> nk_plant_loop)
against the host loop it replaces (harness.lqr_control_plant: one nk_lift call per step), in the same process.

    python tools/plant_loop_bench.py [--out profiles/plant_loop_bench.json] [--steps 2000] [--reps 9] [--warmup 2]

Cases: HJB (d = 1, Matern-5/2, landmarks and samples of tests/golden/f8_hjb_config2.npz) at m = 100, 200 and the Duffing
oscillator (d = 2, Matern-5/2 [1, 1], samples of tests/golden/f12_duffing_full.npz) at m = 20, 200; `steps` steps each;
device call also at batch = 16 and 200.  Every figure is WALL time (time.perf_counter) around one synchronous call -- both
calls return only after their device work has completed and the results are in host memory -- median of `reps` after
`warmup` calls of the same shape.  The model is built once per case (outside the timed calls), the gain is K = 2 C[0]."""
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


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def make_case(name, m):
    golden = os.path.join(ROOT, "tests", "golden")
    rng = np.random.default_rng(100 + m)
    if name == "hjb":
        g = np.load(os.path.join(golden, "f8_hjb_config2.npz"))
        X, Y = g["X"], g["Y"]
        kern, gamma, plant = nk.KernelWrapper([float(g["ls"])]), float(g["gamma"]), nk.HJB(Ts=0.01)
        x0, lo, hi = np.array([0.9]), -0.9, 0.9
    else:
        g = np.load(os.path.join(golden, "f12_duffing_full.npz"))
        X, Y = g["X"], g["Y"]
        kern, gamma, plant = nk.KernelWrapper([1, 1]), float(g["gamma"]), nk.DuffingOscillator(Ts=0.01)
        x0, lo, hi = np.array([-0.5, 0.0]), -0.9, 0.9
    reg = nk.KoopmanNystromRegressor(1, kernel=kern, gamma=gamma, m=m)
    reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, rng.choice(X.shape[0], m, replace=False)])
    reg.fit(X, Y)
    K = 2.0 * np.asarray(reg.C)[0:1, :]
    return reg, K, plant, x0, rng.uniform(lo, hi, size=(200, x0.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_loop_bench.json"))
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    nk.get_context()
    rows = []
    for name, m in (("hjb", 100), ("hjb", 200), ("duffing", 20), ("duffing", 200)):
        reg, K, plant, x0, X0 = make_case(name, m)
        ref = np.zeros_like(x0)
        dev = lambda: reg.closed_loop_plant(K, x0, ref, args.steps, plant)  # noqa: E731
        host = lambda: harness.lqr_control_plant(args.steps, ref, x0, reg, K, plant.update_SOM)  # noqa: E731
        d_med, d_min, d_max = timed(dev, args.reps, args.warmup)
        h_med, h_min, h_max = timed(host, args.reps, args.warmup)
        xs_h, us_h = host()
        st_d, us_d = dev()
        row = dict(plant=name, m=m, steps=args.steps, device_ms=d_med, device_ms_min=d_min, device_ms_max=d_max,
                   device_us_per_step=d_med * 1e3 / args.steps, host_loop_ms=h_med, host_loop_ms_min=h_min,
                   host_loop_ms_max=h_max, host_loop_us_per_step=h_med * 1e3 / args.steps, speedup=h_med / d_med,
                   controls_rel_diff=float(np.linalg.norm(us_d - us_h) / np.linalg.norm(us_h)))
        for batch in (16, 200):
            fb = lambda: reg.closed_loop_plant(K, X0[:batch], ref, args.steps, plant)  # noqa: E731
            b_med, _, _ = timed(fb, args.reps, args.warmup)
            row[f"device_batch{batch}_ms"] = b_med
            row[f"device_batch{batch}_ms_per_trajectory"] = b_med / batch
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(what="plant-in-the-loop LQR closed loop: one device launch (nk_plant_loop) vs the host loop "
                    "(harness.lqr_control_plant, one nk_lift per step)",
               timing="wall time (perf_counter) around one synchronous call; median of reps after warmup calls",
               reps=args.reps, warmup=args.warmup, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
