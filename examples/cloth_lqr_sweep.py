#!/usr/bin/env python3
"""The control branch of the reference's benchmark_lqr_cloth.py (:213-270) as ONE call, on the reference's own data from the
committed fixtures: for every seed and both estimators (Nystrom, thin-plate splines) fit at m = 100 on trajectories 10..39 ->
K = dlqr(A, B, 0.0075 C'C, I) -> 60 steps of the lifted closed loop from the first state of trajectory 10 towards the recorded
swing-up reference, all loops in one device launch and scored there.  Needs an MI355X (the library has no CPU path):

    python3 examples/cloth_lqr_sweep.py [--seeds 10] [--gain device]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import harness

ap = argparse.ArgumentParser()
ap.add_argument("--seeds", type=int, default=10, help="the reference runs 50")
ap.add_argument("--gain", choices=("host", "device"), default="host")
args = ap.parse_args()

G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
t = np.load(os.path.join(G, "cloth_trajs_all.npz"))
f10 = np.load(os.path.join(G, "f10_lqr_control.npz"))
states, inputs = t["states_e10"] / 1e10, t["inputs"]          # 50 trajectories: (192 x T), (6 x T)
X = np.ascontiguousarray(np.hstack([np.vstack((states[i][:, :-1], inputs[i][:, :-1])) for i in range(10, 40)]).T)
Y = np.ascontiguousarray(np.hstack([states[i][:, 1:] for i in range(10, 40)]).T)
x0 = states[10][:, 0]                                          # all_trajs[0] after the validation split (:154-156, :237)
x_ref = f10["reference_lqr"].reshape(-1)                       # the reference state the authors' run wrote (:241-261)

params = dict(nystrom=dict(kernel=nk.ThreeDimensionalKernel(*f10["ls"], 192), gamma=float(f10["gamma"])),
              spline=dict(gamma=float(f10["gamma"])))
res = harness.cloth_lqr_sweep(X, Y, 6, params, 100, list(range(args.seeds)), x0, x_ref, num_steps=60,
                              estimator=("nystrom", "spline"), gain=args.gain, return_trajectories=True)
tm = res["timing"]
print(f"{2 * args.seeds} units (seeds x estimators): fits {tm['fit_s']:.3f} s, gains ({args.gain}) {tm['gain_wait_s']:.3f} s after the "
      f"fits, ONE closed-loop call {1e3 * tm['loop_s']:.2f} ms")
start = np.sqrt(np.mean(np.square(x0 - x_ref)))
for ei, name in enumerate(res["estimators"]):
    J, e = res["J"][ei], res["err_final"][ei]
    print(f"{name:8s} distance to the reference (RMSE per state) {start:.4f} -> median {np.nanmedian(e):.4f} "
          f"[{np.nanmin(e):.4f}, {np.nanmax(e):.4f}]; cost J median {np.nanmedian(J):.4f}; largest control "
          f"{np.nanmax(res['u_absmax'][ei]):.4f}; failed units {int(np.sum(np.isnan(J)))}")
print(f"error over time, Nystrom, median over the seeds (plot_reg_error_cloth.py:24): "
      f"{np.round(np.nanmedian(res['err'][0], axis=0)[::10], 4).tolist()} (every 10th step)")
print(f"simulator inputs of seed 0: x_s {res['x_s'][0, 0].shape}, final_us {res['final_us'][0, 0].shape}, K_sim {res['K_sim'][0, 0].shape}")
