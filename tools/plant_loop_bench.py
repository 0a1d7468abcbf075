"""Plant-in-the-loop LQR closed loop: the single device launch (KoopmanNystromRegressor.closed_loop_plant -> nk_plant_loop)
against the host loop it replaces (harness.lqr_control_plant: one nk_lift call per step), in the same process.

    python tools/plant_loop_bench.py [--out profiles/plant_loop_bench.json] [--steps 2000] [--reps 9] [--warmup 2]

Cases: HJB (d = 1, Matern-5/2, landmarks and samples of tests/golden/f8_hjb_config2.npz) at m = 100, 200 and the Duffing
oscillator (d = 2, Matern-5/2 [1, 1], samples of tests/golden/f12_duffing_full.npz) at m = 20, 200; `steps` steps each;
device call also at batch = 16 and 200.  After them the polynomial-plant loop (PolynomialSystem -> nk_poly_plant_loop), in the
same process: the Duffing TABLE on the models of the two Duffing rows (`ratio_to_builtin` = its time over the built-in
kernel's on the same model and gain) and the coupled oscillators (d = 4, p = 2, 2000 snapshot pairs of the plant itself,
Matern-5/2 [1, 1, 1, 1], gain from solve_lqr) at m = 200, each with its own host loop.  Every figure is WALL time (time.perf_counter) around one synchronous call -- both
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


# x1' = x2, x2' = -x1 - 0.5 x2 - x1^3 + 0.2 x3 + u1, x3' = x4, x4' = -x3 - 0.5 x4 - x3^2 x4 + 0.2 x1 + u2
COUPLED = [(0, 1.0, (0, 1, 0, 0), (0, 0)), (1, -1.0, (1, 0, 0, 0), (0, 0)), (1, -0.5, (0, 1, 0, 0), (0, 0)),
           (1, -1.0, (3, 0, 0, 0), (0, 0)), (1, 0.2, (0, 0, 1, 0), (0, 0)), (1, 1.0, (0, 0, 0, 0), (1, 0)),
           (2, 1.0, (0, 0, 0, 1), (0, 0)), (3, -1.0, (0, 0, 1, 0), (0, 0)), (3, -0.5, (0, 0, 0, 1), (0, 0)),
           (3, -1.0, (0, 0, 2, 1), (0, 0)), (3, 0.2, (1, 0, 0, 0), (0, 0)), (3, 1.0, (0, 0, 0, 0), (0, 1))]


def make_coupled_case(m):
    plant = nk.PolynomialSystem(4, 2, COUPLED, 0.01)
    X, Y = harness.plant_snapshots(plant, 2000, np.random.default_rng(7))
    reg = nk.KoopmanNystromRegressor(2, kernel=nk.KernelWrapper([1.0] * 4), gamma=1e-6, m=m)
    reg.nystrom_centers_output = np.ascontiguousarray(Y.T[:, np.random.default_rng(1).choice(2000, m, False)])
    reg.fit(X, Y)
    return reg, np.ascontiguousarray(reg.solve_lqr(c=1.0)), plant, 0.5 * np.ones(4)


def poly_row(name, reg, K, plant, x0, m, args, builtin_ms=None):
    ref = np.zeros_like(x0)
    dev = lambda: reg.closed_loop_plant(K, x0, ref, args.steps, plant)  # noqa: E731
    host = lambda: harness.lqr_control_plant(args.steps, ref, x0, reg, K, plant.update_SOM)  # noqa: E731
    d_med, d_min, d_max = timed(dev, args.reps, args.warmup)
    h_med, h_min, h_max = timed(host, max(3, args.reps // 3), 1)  # (the Python plant step makes this loop slow)
    _, us_h = host()
    _, us_d = dev()
    row = dict(plant=name, m=m, d=plant.n_states, p=plant.n_inputs, terms=len(plant.terms), steps=args.steps,
               device_ms=d_med, device_ms_min=d_min, device_ms_max=d_max, device_us_per_step=d_med * 1e3 / args.steps,
               host_loop_ms=h_med, host_loop_ms_min=h_min, host_loop_ms_max=h_max,
               host_loop_us_per_step=h_med * 1e3 / args.steps, speedup=h_med / d_med,
               controls_rel_diff=float(np.linalg.norm(us_d - us_h) / np.linalg.norm(us_h)))
    if builtin_ms is not None:
        row["builtin_device_ms"] = builtin_ms
        row["ratio_to_builtin"] = d_med / builtin_ms
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_loop_bench.json"))
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    nk.get_context()
    rows, poly_rows = [], []
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
        if name == "duffing":  # the same model and gain around the Duffing table
            prow = poly_row("duffing_table", reg, K, nk.PolynomialSystem.duffing(0.01), x0, m, args, builtin_ms=d_med)
            poly_rows.append(prow)
    reg, K, plant, x0 = make_coupled_case(200)
    poly_rows.append(poly_row("coupled_oscillators", reg, K, plant, x0, 200, args))
    for prow in poly_rows:
        rows.append(prow)
        print(json.dumps(prow), flush=True)
    out = dict(what="plant-in-the-loop LQR closed loop: one device launch (nk_plant_loop; nk_poly_plant_loop for the rows with "
                    "`terms`) vs the host loop (harness.lqr_control_plant, one nk_lift per step)",
               timing="wall time (perf_counter) around one synchronous call; median of reps after warmup calls",
               reps=args.reps, warmup=args.warmup, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
