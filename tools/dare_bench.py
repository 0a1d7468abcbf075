"""The batched device Riccati solver (nk_dare_batch / nk_model_lqr_gain_batch), timed and checked.

    python tools/dare_bench.py [--out profiles/dare_bench.json] [--problems 200] [--reps 5] [--threads 16]

(a) Solver cost: `problems` problems built from the fixture operators at m = 20 (f12 control runs), 100 (f10) and 200 (f8,
    f12, f15; Q = sym(C'C), R = I; each copy's A perturbed by a seeded 1e-6 relative so that no two are equal) -- ONE
    nk_dare_batch call against lqr.dlqr (scipy) in a pool of `threads` host threads.
(b) Accuracy per shape of tests/test_gpu_dare.py: residual and gain distance as multiples of the bars of
    tests/dare_reference.py (scipy's own residual and movement).
(c) Sweep split: harness.lqr_sweep with gain="host" and gain="device", wall time split into fit_s, gain_wait_s, loop_s;
    shapes Duffing m = 20, HJB m = 100 and HJB m = 200 as in tools/lqr_sweep_bench.py.
Everything runs in one process.  Every figure is WALL time (time.perf_counter) around calls that end synchronised, the
median of `reps` timings after one warm-up of the same shape."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dare_reference as dr  # noqa: E402
import nys_koop_lqr_amd as nk  # noqa: E402
from nys_koop_lqr_amd import harness, lqr  # noqa: E402
from lqr_sweep_bench import shape  # noqa: E402


def median_of(fn, reps):
    fn()  # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0, r))
    return statistics.median(t for t, _ in out), out[-1][1]


def fixture_set(m):
    if m == 20:
        g = np.load(os.path.join(ROOT, "tests", "golden", "f12_duffing_full.npz"))
        return [(np.array(g[f"lqr_A_{s}"]), np.array(g[f"lqr_B_{s}"]).reshape(20, -1), np.array(g[f"lqr_C_{s}"])) for s in range(3)]
    names = {100: ["f10"], 200: ["f8", "f12_m200", "f15_m200"]}[m]
    out = []
    for name in names:
        fname, ka, kb, kc = dr.FIXTURE_OPS[name]
        g = np.load(os.path.join(ROOT, "tests", "golden", fname))
        out.append((np.array(g[ka]), np.array(g[kb]).reshape(m, -1), np.array(g[kc])))
    return out


def solver_cost(m, n, reps, threads):
    base = fixture_set(m)
    rng = np.random.default_rng(m)
    As, Bs, Qs, Rs = [], [], [], []
    for i in range(n):
        A, B, C = base[i % len(base)]
        As.append(A * (1.0 + 1e-6 * rng.standard_normal(A.shape)))
        Bs.append(B)
        Qs.append(dr.sym(C.T @ C))
        Rs.append(np.eye(B.shape[1]))
    ctx = nk.get_context()
    t_dev, dev = median_of(lambda: ctx.dare_batch(As, Bs, Qs, Rs, want_P=False), reps)
    pool = ThreadPoolExecutor(threads)

    def host_one(i):
        try:
            return lqr.dlqr(As[i], Bs[i], Qs[i], Rs[i])[0]
        except Exception:  # noqa: BLE001
            return None

    t_host, host = median_of(lambda: list(pool.map(host_one, range(n))), reps)
    pool.shutdown()
    Ks, _, status, iters, _ = dev
    dist = [dr.relk(K, Kh) for K, Kh, s in zip(Ks, host, status) if s == 0 and Kh is not None]
    return dict(m=m, p=int(Bs[0].shape[1]), problems=n, device_batch_s=t_dev, host_pool_s=t_host, host_threads=threads,
                speedup=t_host / t_dev, device_ms_per_problem=t_dev * 1e3 / n, status_nonzero=int(np.sum(status != 0)),
                host_failed=int(sum(K is None for K in host)), iterations_min=int(iters.min()), iterations_max=int(iters.max()),
                max_rel_gain_distance_to_scipy=float(max(dist)) if dist else None)


def accuracy():
    ctx = nk.get_context()
    rows = []
    cases = [("r%d" % m, m, p) for m, p in ((1, 1), (5, 1), (16, 1), (17, 6), (33, 1), (256, 8))]
    cases += [("f3", 50, 1), ("f10", 100, 6), ("f8", 200, 1), ("f12_m200", 200, 1)]
    for label, m, p in cases:
        if label.startswith("r"):
            A, B, Q, R = dr.random_problem(m, p, 1.1, seed=m)
            ref = dr.reference(A, B, Q, R, seed=m)
        else:
            A, B, Q, R = dr.fixture_problem(label)
            ref = dr.fixture_reference(label)
        Ks, Ps, st, it, _ = ctx.dare_batch([A], [B], [Q], [R])
        Km = lqr.dare_doubling(A, B, Q, R)[1]
        r_bar, k_bar = dr.bars(ref, m)
        rows.append(dict(case=label, m=m, p=p, status=int(st[0]), iterations=int(it[0]),
                         residual=dr.residual(A, B, Q, Ps[0], Ks[0]), residual_scipy=ref["r"], residual_bar=r_bar,
                         gain_vs_scipy_in_movements=dr.relk(Ks[0], ref["K"]) / ref["movement"],
                         gain_vs_mirror_in_movements=dr.relk(Ks[0], Km) / ref["movement"], scipy_movement=ref["movement"],
                         bar_in_movements=dr.MULTIPLIER))
    return rows


def sweep_split(name, m, n_seeds, steps, reps):
    s = shape(name)
    seeds = list(range(n_seeds))
    u_opt = harness.hjb_optimal_control(s["x0"], steps, s["plant"])[0] if name == "hjb" else None
    row = dict(plant=name, m=m, seeds=n_seeds, steps=steps)
    for gain in ("host", "device"):
        t, res = median_of(lambda: harness.lqr_sweep(s["X"], s["Y"], 1, s["params"], [m], seeds, s["plant"], s["x0"], s["ref"], steps,
                                                     u_opt=u_opt, batch=32, workers=8, gain=gain), reps)
        tm = res["timing"]
        row[gain] = dict(sweep_s=t, fit_s=tm["fit_s"], gain_wait_s=tm["gain_wait_s"], gain_cpu_s=tm["gain_cpu_s"],
                         loop_s=tm["loop_s"], failed_units=int(np.sum(np.isnan(res["J"]))))
    row["speedup"] = row["host"]["sweep_s"] / row["device"]["sweep_s"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dare_bench.json"))
    ap.add_argument("--problems", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--sweep-seeds", type=int, nargs=3, default=[200, 48, 16], metavar=("DUFFING20", "HJB100", "HJB200"))
    ap.add_argument("--skip-sweeps", action="store_true")
    args = ap.parse_args()
    nk.get_context()
    out = dict(what="batched device Riccati solver (nk_dare_batch, one workgroup per problem) against scipy in a host thread pool",
               timing="wall time (perf_counter) around synchronous calls, same process; median of reps after one warm-up",
               reps=args.reps, solver_cost=[], accuracy=[], sweep_split=[])
    for m in (20, 100, 200):
        row = solver_cost(m, args.problems, args.reps, args.threads)
        out["solver_cost"].append(row)
        print(json.dumps(row), flush=True)
    out["accuracy"] = accuracy()
    for row in out["accuracy"]:
        print(json.dumps(row), flush=True)
    if not args.skip_sweeps:
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
