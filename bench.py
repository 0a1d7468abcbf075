#!/usr/bin/env python3
"""Headline benchmark: Nystrom-Koopman fits/sec (K_nm build + A,B,C solve) at N=1e5, m=2000, d=384 (+p=6), fp64.

    python bench.py --gpus 1 --steps 5 --warmup 1 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is one complete fit (everything regressors.py:136-169 does given landmarks) over the C4 synthetic workload
of BASELINE.md section 3, with X, Y already resident in HBM (uploaded with torch before the timed region; the C-ABI
receives device pointers).  With N > 1 every rank owns a full replica of the dataset and fits a different
(lengthscale, gamma) candidate of the CV grid per step -- independent units, no data-path collective -- and the ranks
all-gather one diagnostic scalar per fit at the end (RCCL); value = total fits / max-over-ranks time ("weak" scaling).

Rank 0 prints ONE JSON line carrying `roofline` (dominant kernel: the fp64-MFMA Gram GEMM, timed live with HIP events
on the library's stream, from the timed fits themselves).  A plain run does only that: set-up, warm-up, the timed steps,
the outputs (`--dump-outputs`) and the line.  With `--full`, at N=1, the line also carries `cpu_baseline` (the
NumPy/SciPy oracle in reference-faithful mode: by default on the full workload, one warm-up + two timed fits, about two
minutes; `--cpu-baseline sample` is the quick extrapolated form) with `parity_full_size`, `value_host_inputs` (host
arrays in, host arrays out) and `cv_sweep` (the cloth-shaped hyper-parameter sweep).

`--dump-outputs DIR` writes what a caller of the timed path receives from its last step -- the operators A, B, C and the
weights W of the last timed fit, float64, 45 MB at the default shape -- as DIR/<name>.npy.  The inputs are seeded, so two
builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

METRIC = "Nyström-Koopman fits/sec (K_nm build + A,B,C solve), N=1e5 m=2000 d=384"
MFMA_F64_PEAK_TFLOPS = 78.6  # MI355X fp64 matrix peak (spec); measured 77.7 with tools/microbench_f64_v2.hip
CV_GRID = [(l, g) for l in (10.0, 20.0, 40.0) for g in (1e-7, 1e-6, 1e-5, 1e-4, 1e-3)]


def make_c4(n, d, p, m, seed=1234):
    """S~N(0,1), U~N(0,1), Y = tanh(S Wt) + U Bt, landmarks from the legacy RNG seed 0."""
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((n, d))
    U = rng.standard_normal((n, p))
    Wt = rng.standard_normal((d, d)) * 0.9 / np.sqrt(d)
    Bt = rng.standard_normal((p, d)) * 0.1
    Y = np.tanh(S @ Wt) + U @ Bt
    X = np.hstack([S, U])
    np.random.seed(0)
    idx = np.random.choice(np.arange(n), size=m, replace=False)
    return X, Y, idx


def gram_flops_syrk(n, m, p, d):
    """Algorithmic flop of the fused Gram launch with the symmetry of the two SYRKs exploited
    (the 2.07e12-per-fit figure minus the distance flops): (m+p)(m+p+1)n + 2m(m+p)n + m(m+1)n + 2dmn."""
    mp = m + p
    return mp * (mp + 1) * n + 2.0 * m * mp * n + m * (m + 1) * n + 2.0 * d * m * n


def _oracle_fit(O, X, Y, Z, ls, gamma, p, faithful=True):
    n, d = Y.shape
    reg = O.KoopmanNystromOracle(p, kernel=O.ThreeDimensionalKernel(ls, ls, ls, d), gamma=gamma, m=Z.shape[0],
                                 faithful=faithful)
    reg.nystrom_centers_output = Z.T
    t0 = time.perf_counter()
    reg.fit(X, Y)
    return time.perf_counter() - t0, reg


def _blas_threads():
    try:
        from threadpoolctl import threadpool_info
        return sorted({int(i.get("num_threads", 0)) for i in threadpool_info() if i.get("user_api") == "blas"})
    except Exception:
        return []


def cpu_baseline_full(X, Y, idx, ls, gamma, p, threads, timed=2, budget_s=240.0):
    """SURVEY 8(d) protocol: the reference-faithful oracle (cdist + exp, sqrtm x2, solve(her), lstsq x2) on the FULL
    workload, one warm-up (a fit on a 10 % row sample with all landmarks: pages in SciPy / BLAS and spins up the thread
    pool) and `timed` full-size fits; value = 1 / median.  The warm-up also predicts the cost of a full fit: on a host
    where `timed` fits would not fit into `budget_s` seconds, fewer are run (at least one), and if even one would not
    fit, the labelled sample extrapolation is reported instead -- the default run must finish within minutes anywhere."""
    from oracle import nk_oracle as O
    from threadpoolctl import threadpool_limits
    n, d = Y.shape
    Z = Y[idx]
    rows = max(n // 10, len(idx))
    with threadpool_limits(limits=threads):
        blas = _blas_threads()
        warm, wreg = _oracle_fit(O, X[:rows], Y[:rows], Z, ls, gamma, p)
        tw = wreg.timings
        predicted = tw["fixed"] + (tw["kernel_n"] + tw["gram_n"]) * (n / rows)
        if predicted > budget_s:
            return None, None
        timed = max(1, min(timed, int(budget_s // predicted)))
        walls, stages = [], None
        for _ in range(timed):
            w, reg = _oracle_fit(O, X, Y, Z, ls, gamma, p)
            walls.append(w)
            stages = reg.timings
        # the de-pessimised CPU form (eigh square root once + Cholesky solves), from the 10 % sample, n-proportional stages
        # scaled: reported so that the speed-up is not inflated by the reference's avoidable O(m^3) work
        _, freg = _oracle_fit(O, X[:rows], Y[:rows], Z, ls, gamma, p, faithful=False)
        tf = freg.timings
        fast = tf["fixed"] + (tf["kernel_n"] + tf["gram_n"]) * (n / rows)
    med = float(np.median(walls))
    return dict(value=1.0 / med, unit="fits/s", cores=threads, kind="port", protocol="full-size",
                seconds_per_fit=walls, spread_rel=float((max(walls) - min(walls)) / med),
                os_cpu_count=os.cpu_count(), blas_threads=blas, fast_mode_value_extrapolated=1.0 / fast,
                sample=(f"oracle in reference-faithful mode (cdist+exp, sqrtm x2, solve(her), lstsq x2) on the full workload "
                        f"n={n} m={len(idx)} d={d}: warm-up on a 10% row sample ({warm:.1f} s), then {timed} timed full-size "
                        f"fit(s) {['%.1f' % w for w in walls]} s (last: {stages['kernel_n']:.1f} s kernel builds + "
                        f"{stages['gram_n']:.1f} s Gram + {stages['fixed']:.1f} s O(m^3)); cdist/exp are single-threaded; "
                        f"fast_mode_value_extrapolated = the same algebra with eigh square root + Cholesky, from the 10% sample")), reg


def cpu_baseline_sample(X, Y, idx, ls, gamma, p, sample_rows, threads):
    """Fallback (--cpu-baseline sample): faithful oracle on the first `sample_rows` rows with all landmarks; the stages
    that scale with n (kernel builds, Gram products) are extrapolated linearly, the O(m^3) stages taken as measured."""
    from oracle import nk_oracle as O
    from threadpoolctl import threadpool_limits
    n, d = Y.shape
    Z = Y[idx]
    with threadpool_limits(limits=threads):
        wall, reg = _oracle_fit(O, X[:sample_rows], Y[:sample_rows], Z, ls, gamma, p)
        _, fast = _oracle_fit(O, X[:sample_rows], Y[:sample_rows], Z, ls, gamma, p, faithful=False)
    tm, tf = reg.timings, fast.timings
    full = tm["fixed"] + (tm["kernel_n"] + tm["gram_n"]) * (n / sample_rows)
    full_fast = tf["fixed"] + (tf["kernel_n"] + tf["gram_n"]) * (n / sample_rows)
    return dict(value=1.0 / full, unit="fits/s", cores=threads, kind="port", protocol="extrapolated-sample",
                os_cpu_count=os.cpu_count(), blas_threads=_blas_threads(), fast_mode_value=1.0 / full_fast,
                sample=(f"EXTRAPOLATED: faithful oracle on the first {sample_rows} of {n} rows with all {len(idx)} landmarks: "
                        f"{wall:.1f} s wall = {tm['kernel_n']:.1f} s kernel builds + {tm['gram_n']:.1f} s Gram (both scaled "
                        f"x{n / sample_rows:.0f}) + {tm['fixed']:.1f} s O(m^3) stages (unscaled) => {full:.0f} s per full fit"))


def cv_sweep_rate(nk, workers=4):
    """Secondary figure: the hyper-parameter sweep of benchmark_lqr_cloth.py:39-66 at its real shape (n = 1010 rows in 5
    folds, m = 500 landmarks, d = 192, p = 6; synthetic cloth-shaped rows) -- (candidate, fold) units per second."""
    from nys_koop_lqr_amd import harness
    rng = np.random.default_rng(7)
    n, d, p, m = 1010, 192, 6, 500
    S = rng.standard_normal((n, d)) * 0.3
    U = rng.standard_normal((n, p)) * 0.05
    Y = np.tanh(S @ (rng.standard_normal((d, d)) * 0.9 / np.sqrt(d))) + U @ (rng.standard_normal((p, d)) * 0.1)
    X = np.hstack([S, U])
    cands = [dict(kernel=nk.ThreeDimensionalKernel(l, l, l, d), gamma=g, m=m) for l in (3.0, 6.0, 12.0)
             for g in (1e-6, 1e-5, 1e-4)]
    centers = {(c, f): np.random.RandomState(17 * c + f).choice(808, m, replace=False) for c in range(9) for f in range(5)}
    cands = cands * 9  # 81 candidates x 5 folds = 405 units, the size of the reference's grid (benchmark_lqr_cloth.py:46-57)
    centers = {(c, f): np.random.RandomState(17 * c + f).choice(808, m, replace=False) for c in range(len(cands))
               for f in range(5)}
    nu = len(cands) * 5
    one = harness.grid_search_cv(X, Y, p, cands[:9], centers=centers)  # one unit at a time (also the bit-identity reference)
    t0 = time.perf_counter()
    harness.grid_search_cv(X, Y, p, cands[:9], centers=centers)
    dt1 = time.perf_counter() - t0
    # ONE pool shape (2 groups x 32 units), the MEDIAN of five timed sweeps after a warm-up of every group member
    batch, groups = 32, 2
    harness.grid_search_cv(X, Y, p, cands, centers=centers, batch=batch, batch_groups=groups)
    dts = []
    for _ in range(5):
        t0 = time.perf_counter()
        res = harness.grid_search_cv(X, Y, p, cands, centers=centers, batch=batch, batch_groups=groups)
        dts.append(time.perf_counter() - t0)
    dt = float(np.median(dts))
    out = dict(units_per_s=nu / dt, units=nu, seconds=dt, seconds_min_max=[min(dts), max(dts)],
               mode="lock-step batched: %d groups x %d units (nk_cv_grid); median of 5 sweeps" % (groups, batch),
               units_per_s_unbatched=45 / dt1, shape="n=1010 (808 train / 202 test) m=500 d=192 p=6",
               data="synthetic cloth-shaped rows, 9 distinct well-conditioned candidates x 9 (no unit takes the rank-truncating branch)",
               bit_identical_to_unbatched=bool(np.array_equal(one["split_scores"], res["split_scores"][:9])),
               finite=bool(np.all(np.isfinite(res["split_scores"]))))
    real = real_cloth_grid_rate(nk, batch, groups)
    if real is not None:
        out.update(real)
    return out


def real_cloth_grid_rate(nk, batch, groups):
    """The REAL grid of benchmark_lqr_cloth.py:39-66: the reference's ten validation trajectories (n = 1010), 27 kernels x 3
    gammas x 5 folds = 405 units, landmarks replayed from the seed in GridSearchCV's order -- inputs from the committed
    fixtures (tests/golden/cloth_trajs_all.npz, f7_cloth_cv_full.npz).  Includes the ill-conditioned candidates whose
    systems take the rank-truncating branch of lstsq (regressors.py:155,165), which the synthetic rows above never do."""
    from nys_koop_lqr_amd import harness
    gdir = os.path.join(ROOT, "tests", "golden")
    try:
        g = np.load(os.path.join(gdir, "f7_cloth_cv_full.npz"))
        t = np.load(os.path.join(gdir, "cloth_trajs_all.npz"))
    except OSError:
        return None
    st = t["states_e10"] / 1e10
    X = np.ascontiguousarray(np.hstack([np.vstack((st[i][:, :-1], t["inputs"][i][:, :-1])) for i in range(10)]).T)
    Y = np.ascontiguousarray(np.hstack([st[i][:, 1:] for i in range(10)]).T)
    cands = [dict(kernel=nk.ThreeDimensionalKernel(*g["ls_grid"][int(g["order_kernel"][c])], 192),
                  gamma=float(g["order_gamma"][c]), m=int(g["m"])) for c in range(len(g["order_gamma"]))]
    dts, res = [], None
    for rep in range(4):
        np.random.seed(int(g["seed"]))
        t0 = time.perf_counter()
        res = harness.grid_search_cv(X, Y, 6, cands, n_splits=5, batch=batch, batch_groups=groups)
        if rep > 0:
            dts.append(time.perf_counter() - t0)
    dt = float(np.median(dts))
    rel = np.abs(res["split_scores"] - g["split_scores"]) / np.abs(g["split_scores"])
    return dict(real_grid_units_per_s=405 / dt, real_grid_seconds=dt, real_grid_seconds_min_max=[min(dts), max(dts)],
                real_grid_best_index_matches_reference=bool(res["best_index"] == int(np.argmax(g["mean_test_score"]))),
                real_grid_max_rel_score_error=float(rel.max()),
                real_grid_note="reference inputs and GridSearchCV landmark draws (fixtures f0 / f7); median of 3 sweeps after one warm-up")


def dump_outputs(path, reg):
    """What the timed path hands its caller, from the regressor of the last timed step: DIR/{A,B,C,W}.npy in float64."""
    os.makedirs(path, exist_ok=True)
    arrays = {"A": reg.A, "B": reg.B, "C": reg.C, "W": reg.weights}
    total = sum(np.asarray(a).size * 8 for a in arrays.values())
    assert total <= 64 << 20, f"outputs of {total / 2**20:.1f} MiB exceed the 64 MiB dump limit"
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=2000)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--p", type=int, default=6)
    ap.add_argument("--full", action="store_true",
                    help="also measure the secondary figures (at N=1: CPU baseline with full-size parity, host-input rate, "
                         "CV sweeps); a plain run measures the headline fits only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the operators of the last timed fit (A, B, C, W) as DIR/<name>.npy")
    ap.add_argument("--cpu-baseline", choices=["full", "sample", "none"], default="full",
                    help="the CPU leg of --full.  full: faithful oracle on the full workload, warm-up + 2 timed fits (~2 min); "
                         "sample: one fit on --cpu-sample-rows rows, extrapolated (labelled as such); none: skip")
    ap.add_argument("--cpu-sample-rows", type=int, default=10000)
    ap.add_argument("--cpu-threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--sweep", action="store_true",
                    help="walk a 15-candidate (lengthscale, gamma) grid instead: step s on rank r fits candidate (r + N s) mod 15 (the "
                         "units of a sharded CV sweep; their cost differs by the square-root iteration count).  Default at "
                         "every N: each unit is the headline fit (l=20, gamma=1e-6), so a 1 -> N curve times the same work per GPU")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the host-input and CV-sweep secondary figures")
    ap.add_argument("--concurrency", type=int, default=1,
                    help="host threads issuing independent fits concurrently on each GPU (each with its own context and "
                         "streams); 1 = one fit at a time (the default, and the setting the roofline figure refers to)")
    args = ap.parse_args()

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # NYSKOOP_BENCH_BACKEND=gloo rehearses the multi-rank path on a box with fewer GPUs than ranks (ranks share
    # devices round-robin, collectives on CPU tensors); the real runs use RCCL ("nccl"), one rank per GPU.
    backend = os.environ.get("NYSKOOP_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    dev_index = local_rank if backend == "nccl" else local_rank % max(ndev, 1)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(dev_index)
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend=backend)
    assert args.gpus == world, f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run"
    dev = torch.device("cuda", dev_index)
    cdev = dev if backend == "nccl" else torch.device("cpu")  # where collective payloads live
    torch.cuda.set_device(dev)
    local_rank = dev_index

    import nys_koop_lqr_amd as nk
    from nys_koop_lqr_amd import _lib
    os.environ["NYSKOOP_DEVICE"] = str(local_rank)
    ctx = nk.get_context(local_rank)

    n, m, d, p = args.n, args.m, args.d, args.p
    X, Y, idx = make_c4(n, d, p, m)
    Xd = torch.from_numpy(X).to(dev)  # resident in HBM before the timed region
    Yd = torch.from_numpy(Y).to(dev)
    Z = np.ascontiguousarray(Y[idx])
    torch.cuda.synchronize()

    sweep = args.sweep  # default at every N: each unit is the headline fit, so that the per-GPU work of the N-rank run IS the N = 1 line's

    def one_fit(step):
        ls, gamma = CV_GRID[(rank + world * step) % len(CV_GRID)] if sweep else (20.0, 1e-6)
        reg = nk.KoopmanNystromRegressor(p, kernel=nk.ThreeDimensionalKernel(ls, ls, ls, d), gamma=gamma, m=m)
        reg.nystrom_centers_output = Z.T
        reg.fit(Xd, Yd)  # device pointers: no PCIe traffic for X, Y inside the timed region
        return reg

    conc = max(1, args.concurrency)
    if conc > 1:
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=conc)
        list(pool.map(lambda w: [one_fit(w) for _ in range(max(args.warmup, 1))], range(conc)))  # per-thread warm-up
    last = None
    for w in range(args.warmup):
        last = one_fit(w)  # same object lifetime as in the timed loop: the pinned-buffer pool reaches its steady state
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    # as `timeit` does: no cyclic garbage collection inside the timed region (a full CPython collection walks the ~1e6
    # objects NumPy / SciPy / torch keep alive and takes 45-75 ms here, tools/gc_probe.py -- more than one fit)
    import gc
    gc.collect()
    gc.disable()
    t0 = time.perf_counter()
    stats = []
    if conc > 1:
        regs = list(pool.map(one_fit, range(args.steps)))  # exactly K fits, issued by `conc` threads
        stats = [r.fit_stats_ for r in regs]
        last = regs[-1]
    else:
        for s in range(args.steps):
            last = one_fit(s)
            stats.append(last.fit_stats_)
    ctx.synchronize()
    torch.cuda.synchronize()
    diag = torch.tensor([st["sqrt_residual"] for st in stats], dtype=torch.float64, device=cdev)
    if world > 1:
        gathered = [torch.empty_like(diag) for _ in range(world)]
        dist.all_gather(gathered, diag)  # per-fit scalars only: the one collective of the sweep
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    gc.enable()
    t = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, last)

    if rank == 0:
        ms_step = elapsed / args.steps * 1e3
        value = world * args.steps / elapsed
        avg = lambda k: float(np.mean([st[k] for st in stats]))
        launches = max(int(stats[-1]["gram_kernel_launches"]), 1)
        flops_per_launch = gram_flops_syrk(n, m, p, d) / launches  # one fused launch when operands are aligned
        achieved = flops_per_launch / (avg("ms_gram_kernel_avg") * 1e-3) / 1e12
        traffic = None
        tfile = os.path.join(ROOT, "profiles", "gram_traffic.json")
        if os.path.exists(tfile):
            try:
                tj = json.load(open(tfile))
                if tj.get("n") == n and tj.get("m") == m and tj.get("d") == d:
                    traffic = tj.get("hbm_bytes_per_launch")
            except Exception:
                traffic = None
        out = {
            "metric": METRIC, "value": value, "unit": "fits/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms_step, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": "C4 synthetic cloth-sized (BASELINE.md s3): n=%d m=%d d=%d p=%d, isotropic RBF "
                                   "%s jitter=1e-6" % (n, m, d, p, "l=20 gamma=1e-6" if not sweep else
                                                       "CV-grid candidates l in {10,20,40} x gamma in {1e-7..1e-3}, candidate "
                                                       "(rank + world*step) mod 15 per step"),
                       "n": n, "m": m, "d": d, "p": p, "inputs": "HBM-resident (device pointers through the C-ABI)",
                       "outputs": "A,B,C,W copied to page-locked host arrays by asynchronous DMA that overlaps the next fit; all copies complete inside the timed region",
                       "parallelism": "1 process/GPU, independent fits per rank (the units of a sharded sweep; no data-path collective), RCCL all-gather of per-fit scalars",
                       "concurrent_fits_per_gpu": conc,
                       "timed_region": "CPython's cyclic GC disabled inside the timed region, as timeit does (a full collection "
                                       "walks ~1e6 live NumPy / SciPy / torch objects: 45-75 ms, more than one fit)"},
            "stages_ms": {k: avg(k) for k in ("ms_total", "ms_kmat", "ms_gram", "ms_sqrt", "ms_solve", "host_ms_drop",
                                              "host_ms_call", "host_ms_fetch", "host_ms_pinned")},
            "sqrt_iters": int(stats[-1]["sqrt_iters"]),
            "roofline": {"bound": "mfma", "kernel": "nk::gram_fused_f64_kernel (fused Gram / cross-Gram launch over n; engine nk_gemm_tn.hip)",
                         "achieved": achieved, "peak": MFMA_F64_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / MFMA_F64_PEAK_TFLOPS, "traffic": traffic,
                         "flops_per_launch": flops_per_launch, "avg_launch_ms": avg("ms_gram_kernel_avg"),
                         "launches_per_fit": launches,
                         "note": "algorithmic flop with SYRK symmetry exploited: (m+p)(m+p+1)n + 2m(m+p)n + m(m+1)n + 2dmn "
                                 "in one fused launch; the split-K reduce kernel is excluded from the launch time"},
        }
        if world == 1 and args.full and not args.no_extras:
            # fits/s as the reference's fit(X, Y) is called: X, Y host NumPy arrays in, operators landed in host arrays
            # (the 620 MB upload from pageable memory is inside; never the headline `value`)
            def host_fit():
                reg = nk.KoopmanNystromRegressor(p, kernel=nk.ThreeDimensionalKernel(20.0, 20.0, 20.0, d), gamma=1e-6, m=m)
                reg.nystrom_centers_output = Z.T
                reg.fit(X, Y)
                return reg.A, reg.B, reg.C, reg.weights
            host_fit()
            t1 = time.perf_counter()
            for _ in range(3):
                host_fit()
            out["value_host_inputs"] = 3 / (time.perf_counter() - t1)
            out["cv_sweep"] = cv_sweep_rate(nk)
        mode = "none" if args.no_cpu_baseline or not args.full else args.cpu_baseline
        if world == 1 and mode != "none":
            base, oracle_fit = None, None
            if mode == "full":
                base, oracle_fit = cpu_baseline_full(X, Y, idx, 20.0, 1e-6, p, args.cpu_threads)
            if base is None:
                base = cpu_baseline_sample(X, Y, idx, 20.0, 1e-6, p, min(args.cpu_sample_rows, n), args.cpu_threads)
            out["cpu_baseline"] = base
            out["gpu_over_cpu"] = value / base["value"]
            if oracle_fit is not None and not sweep:
                # the timed CPU leg IS the reference-faithful oracle on the full workload with the same landmarks and
                # hyper-parameters: relative Frobenius distance of the GPU operators of the last timed fit from it
                rel = lambda a, b: float(np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b))
                fc = oracle_fit.predict(X[:256])
                out["parity_full_size"] = dict(A=rel(last.A, oracle_fit.A), B=rel(last.B, oracle_fit.B),
                                               C=rel(last.C, oracle_fit.C), W=rel(last.weights, oracle_fit.weights),
                                               predict=rel(last.predict(X[:256]), fc),
                                               against="oracle, reference-faithful mode, full n (the cpu_baseline fit)")
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
