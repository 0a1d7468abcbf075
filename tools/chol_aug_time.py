#!/usr/bin/env python3
"""Timed loop of nk_chol_aug on the launch-per-step chain: the (200, 1, 2) pair of the Duffing sweeps (orders 201 and 200 with
200 and 2 right-hand sides) and one system of order 200 with 203 right-hand sides, the matrices of tests/chol_reference.py.
Each call stages its operands from the host, queues the chain and waits for the verdict, so a figure is the latency of one
whole call; the library is the one NYSKOOP_LIB names.  Prints one line per case: median and fastest of `--repeats` windows of
`--calls` calls each, in microseconds per call, and a hash of the results (equal between two builds that compute the same
bits)."""
import argparse, hashlib, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import nys_koop_lqr_amd as nk
import chol_reference as cr

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=30)
args = ap.parse_args()

ctx = nk.get_context()
CASES = {
    "pair (200, 1, 2)": [(np.array(cr.matrix(f, m, s)), np.array(cr.rhs(e, m, s)), m)
                         for f, m, s, e in cr.small_pair_systems(200, 1, 2, "rbf", "rbf")],
    "single m = 200": [(np.array(cr.matrix("rbf", 200, 200)), np.array(cr.rhs(203, 200, 200)), 200)],
}
for name, systems in CASES.items():
    for _ in range(args.warmup):
        out = cr.chol_aug(ctx, systems)
    assert all(failed == 0 for _, _, failed, _ in out), name
    windows = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            cr.chol_aug(ctx, systems)  # (returns after the verdict: the device is idle again)
        windows.append((time.perf_counter() - t0) / args.calls * 1e6)
    digest = hashlib.sha256(b"".join(np.tril(L).tobytes() + X.tobytes() for L, X, _, _ in out)).hexdigest()[:16]
    print(f"chol_aug {name}: median {statistics.median(windows):.1f} us/call, fastest {min(windows):.1f} us/call "
          f"({args.repeats} x {args.calls} calls)  bits {digest}", flush=True)
