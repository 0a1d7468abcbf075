"""Landmark selection on the device (nk_select_landmarks), timed.

    python tools/landmark_bench.py [--out profiles/landmark_bench.json] [--reps 5]

Two shapes: the Duffing data set of tests/golden (n = 69 900, d = 2, Matern-5/2, m = 200) and a synthetic cloth-sized one
(n = 100 000, d = 384, anisotropic RBF with length scales cycling (10, 10, 10), m = 2000), both pick rules.  Y is a device
tensor, so no staging copy is inside the timed call.  Every time is WALL time (time.perf_counter) around the call, which
ends synchronised (its one result copy), in one process: the median of `reps` timings after one warm-up of the same shape.
Next to each time: the factor traffic the algorithm needs, 8 n m^2 / 2 bytes (step j reads j columns of n doubles), over
the time -- a whole-call rate, launch gaps and the kernel-column passes (8 n d m bytes, listed apart) included, so it is
a lower bound of what the column kernel sustains -- beside the 5.14 TB/s the project's write-bound kernel-matrix kernel reaches."""
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

FILL_TBPS = 5.14  # the write-bound kernel-matrix kernel with the linear epilogue (5.1-5.3 TB/s)


def time_case(label, Y, kernel, m, rule, reps):
    n, d = int(Y.shape[0]), int(Y.shape[1])
    u = np.random.RandomState(0).uniform(size=m)
    nk.select_landmarks(Y, kernel, m, rule=rule, u=u)  # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rows, info = nk.select_landmarks(Y, kernel, m, rule=rule, u=u, return_info=True)
        times.append(time.perf_counter() - t0)
    t = statistics.median(times)
    factor_bytes = 8.0 * n * m * m / 2
    return dict(case=label, n=n, d=d, m=m, rule=rule, m_selected=int(len(rows)), call_s=t, call_s_min=min(times),
                call_s_max=max(times), ms_per_step=1e3 * t / m, factor_bytes=factor_bytes, kernel_column_bytes=8.0 * n * d * m,
                factor_tbps=factor_bytes / t / 1e12, fill_kernel_tbps=FILL_TBPS, share_of_fill_rate=factor_bytes / t / 1e12 / FILL_TBPS,
                trace_start=float(info["trace"][0]), trace_left=float(info["trace"][-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landmark_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    import torch
    nk.get_context()
    g = np.load(os.path.join(ROOT, "tests", "golden", "f12_duffing_full.npz"))
    cases = [("duffing", torch.from_numpy(np.ascontiguousarray(g["Y"])).to("cuda"), nk.KernelWrapper([1, 1]), 200)]
    if not args.skip_large:
        gen = torch.Generator(device="cuda").manual_seed(0)
        Yl = torch.rand((100000, 384), dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        cases.append(("synthetic-d384", Yl, nk.ThreeDimensionalKernel(10, 10, 10, 384), 2000))
    torch.cuda.synchronize()
    out = dict(what="nk_select_landmarks: partial pivoted Cholesky of K(Y, Y) on the device, two launches per step",
               timing="wall time (perf_counter) around the synchronous call, Y resident on the device, same process; "
                      "median of reps after one warm-up",
               reps=args.reps, rows=[])
    for label, Y, kernel, m in cases:
        for rule in ("greedy", "rpcholesky"):
            row = time_case(label, Y, kernel, m, rule, args.reps)
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
