"""The launch-chain device Riccati solver (nk_dare_large), timed and checked against the host.

    python tools/dare_large_bench.py [--out profiles/dare_large_bench.json] [--sizes 300 500 1000 2000 4000]
                                     [--rhos 0.9 1.1] [--scipy-max-m 1000] [--movement-max-m 4000] [--exact-n 4000]

Per size m: tests/dare_reference.random_problem(m, 6, rho, seed = m) for every rho, and at the end the exact-kernel HJB model
(KoopmanKernelRegressor on the first `exact-n` samples of the f8 fixture, Q = C'C, R = 1; --exact-n 0 skips it).  Recorded:
  device_s        wall time of Context.dare_large with host operands (staging included), the second of two calls;
  split           a third call with NYSKOOP_DARE_TIMING=1, which synchronises the stream around every phase: milliseconds in
                  the LU launches (panel, exchanges, row block, trailing and backward updates), in the products and
                  elementwise kernels of the steps, and in the per-step synchronisation (that call's total is recorded too:
                  the phase synchronisations cost time of their own);
  mirror_s        lqr.dare_doubling (LAPACK getrf + dgemm) on the host, with as many BLAS threads as the environment gives
                  (recorded as host_threads);
  scipy_s         lqr.dlqr where m <= scipy-max-m;
  steps, residual, |K - K_mirror| / |K_mirror| and, where m <= movement-max-m, the same over the mirror's movement under
  1e-15 perturbations (three more mirror solves: tests/dare_large_reference.mirror_reference).
Everything runs in one process; wall time is time.perf_counter around calls that end synchronised."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dare_reference as dr  # noqa: E402
import dare_large_reference as dl  # noqa: E402
import nys_koop_lqr_amd as nk  # noqa: E402
from nys_koop_lqr_amd import lqr  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def measure(tag, A, B, Q, R, seed, args, dev_ops=None):
    ctx = nk.get_context()
    m, p = B.shape
    ops = dev_ops if dev_ops is not None else (A, B, Q, R)
    ctx.dare_large(*ops)  # warm-up: code objects, workspace of the staging copies
    t_dev, (K, P, status, iters, delta) = timed(lambda: ctx.dare_large(*ops))
    os.environ["NYSKOOP_DARE_TIMING"] = "1"
    try:
        ctx.dare_large(*ops, want_P=False)
        split = ctx.dare_large_times()
    finally:
        del os.environ["NYSKOOP_DARE_TIMING"]
    row = dict(case=tag, m=m, p=p, status=status, steps=iters, last_step=delta, device_s=t_dev,
               operands="device" if dev_ops is not None else "host", split_ms=split)
    t_mir, (Pm, Km, itm, stm) = timed(lambda: lqr.dare_doubling(A, B, Q, R))
    row.update(mirror_s=t_mir, mirror_steps=itm, mirror_status=stm, speedup_vs_mirror=t_mir / t_dev)
    if status == 0:
        row["residual"] = dr.residual(A, B, Q, P, K)
        if stm == 0:
            row["residual_mirror"] = dr.residual(A, B, Q, Pm, Km)
            row["gain_vs_mirror"] = dr.relk(K, Km)
    if stm == 0 and m <= args.movement_max_m:
        ref = dl.mirror_reference(A, B, Q, R, seed=seed)
        row["mirror_movement"] = ref["movement"]
        if status == 0:
            row["gain_vs_mirror_in_movements"] = dr.relk(K, Km) / ref["movement"]
    if m <= args.scipy_max_m:
        try:
            t_sp, (Ks, Ps) = timed(lambda: lqr.dlqr(A, B, Q, R))
            row.update(scipy_s=t_sp, residual_scipy=dr.residual(A, B, Q, Ps, Ks))
            if status == 0:
                row["gain_vs_scipy"] = dr.relk(K, Ks)
        except Exception as e:  # noqa: BLE001 -- scipy refuses some of the ill-conditioned pencils
            row["scipy_error"] = str(e)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dare_large_bench.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[300, 500, 1000, 2000, 4000])
    ap.add_argument("--rhos", type=float, nargs="*", default=[0.9, 1.1])
    ap.add_argument("--scipy-max-m", type=int, default=1000)
    ap.add_argument("--movement-max-m", type=int, default=4000)
    ap.add_argument("--exact-n", type=int, default=4000)
    args = ap.parse_args()
    nk.get_context()
    threads = os.environ.get("OMP_NUM_THREADS") or os.environ.get("OPENBLAS_NUM_THREADS") or str(os.cpu_count())
    out = dict(what="launch-chain device Riccati solver (nk_dare_large) against lqr.dare_doubling and scipy on the host",
               timing="wall time (perf_counter) around synchronous calls, same process; device: second of two calls",
               host_threads=threads, rows=[])

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for m in args.sizes:
        for rho in args.rhos:
            A, B, Q, R = dr.random_problem(m, 6, rho, seed=m)
            out["rows"].append(measure(f"random m={m} rho={rho}", A, B, Q, R, m, args))
            save()
    if args.exact_n > 0:
        g = np.load(os.path.join(ROOT, "tests", "golden", "f8_hjb_config2.npz"))
        N = args.exact_n
        reg = nk.KoopmanKernelRegressor(1, kernel=nk.KernelWrapper([float(g["ls"])]), gamma=float(g["gamma"]))
        t_fit, _ = timed(lambda: reg.fit(np.ascontiguousarray(g["X"][:N]), np.ascontiguousarray(g["Y"][:N])))
        t_gain, K = timed(lambda: reg.solve_lqr(c=1.0, device=True))  # operators read from HBM
        A, B, Cm = np.array(reg.A), np.array(reg.B).reshape(N, 1), np.array(reg.C)
        row = measure(f"exact HJB N={N}", A, B, dr.sym(Cm.T @ Cm), np.eye(1), 0, args)
        row.update(fit_s=t_fit, solve_lqr_device_first_call_s=t_gain,
                   spectral_radius=float(np.abs(np.linalg.eigvals(A)).max()) if N <= 2000 else None)
        out["rows"].append(row)
    save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
