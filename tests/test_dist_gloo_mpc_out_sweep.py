"""CPU, world_size 2, gloo: dist.sharded_lqr_sweep(controller=dict(..., x_max=...)) deals the units round-robin, every rank
builds the state-limited controllers of its share and runs ONE MPC loop call, the all-gather carries TEN scores per unit
(harness.MPC_OUT_SCORE_NAMES), and every rank ends with the tables of the plain sweep.  Fits, controllers and the device loop
are stand-ins (no GPU is present here)."""
import json
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STUBS = textwrap.dedent("""
    from types import SimpleNamespace
    import numpy as np

    ARGS = (np.zeros((50, 3)), np.zeros((50, 2)), 1, dict(kernel=None, gamma=1e-6), [4, 6, 8], [0, 1, 2], None, np.zeros(2),
            np.zeros(2), 5)
    BOX = dict(horizon=8, u_min=-0.5, u_max=0.5, x_min=[-np.inf, -0.5], x_max=[np.inf, 0.5], y_weight=40.0, rho=7.0, iters=30)
    FAIL = (1, 2)
    calls = []

    def fit_fn(X, Y, n_inputs, params, unit, estimator):
        tag = 10.0 * unit["si"] + unit["k"] + 1.0

        def solve_mpc(horizon, c=1.0, **limits):
            if (unit["si"], unit["k"]) == FAIL:
                raise np.linalg.LinAlgError("no stabilising solution")
            assert limits["x_max"] == [np.inf, 0.5] and limits["y_weight"] == 40.0 and limits["rho"] == 7.0
            return SimpleNamespace(tag=tag)

        return SimpleNamespace(A=np.eye(2), B=np.ones((2, 1)), C=np.ones((1, 2)), tag=tag, solve_mpc=solve_mpc)

    def loop_fn(regs, ctls, x0, x_ref, num_steps, plant, iters=50, tol=0.0, u_opt=None, return_trajectories=False):
        tags = np.array([r.tag for r in regs])
        calls.append(list(tags))
        assert [c.tag for c in ctls] == list(tags) and iters == 30
        return dict(sse_u=tags, ss_opt=4.0 * tags, J=tags + 0.5, u_absmax=-tags, iters_sum=2.0 * tags, r_max=0.25 * tags,
                    n_at_limit=3.0 * tags, n_iterated=tags - 1.0, y_viol_max=0.125 * tags, n_y_viol=tags + 2.0)
""")

WORKER = textwrap.dedent("""
    import os, sys, json
    import numpy as np
    sys.path.insert(0, {root!r})
    sys.path.insert(0, {out!r})
    from nys_koop_lqr_amd import dist as nkd, harness
    import mpc_out_sweep_stubs as S
    rank, world = nkd.init_process_group("gloo")
    res = nkd.sharded_lqr_sweep(*S.ARGS, fit_fn=S.fit_fn, loop_fn=S.loop_fn, controller=S.BOX)
    np.savez(os.path.join({out!r}, f"tables_{{rank}}.npz"), **{{k: res[k] for k in harness.MPC_OUT_SCORE_NAMES + ("rmse_control",)}})
    # one write per rank, newline included: the ranks share the pipe, and print() hands the text and its newline over apart
    sys.stdout.write(json.dumps(dict(rank=rank, world=world, calls=S.calls)) + "\\n")
    sys.stdout.flush()
""")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_sharded_mpc_out_sweep_world2_gloo(tmp_path):
    (tmp_path / "mpc_out_sweep_stubs.py").write_text(STUBS)
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, out=str(tmp_path)))
    env = dict(os.environ, OMP_NUM_THREADS="2", OPENBLAS_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    reports = sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")), key=lambda d: d["rank"])
    assert [d["world"] for d in reports] == [2, 2]
    # ONE loop call per rank over its share: units 0, 2, 4, 6, 8 and 1, 3, 5, 7 of the m-major plan, the failed one left out
    plan_tags = [10.0 * si + k + 1.0 for k in range(3) for si in range(3)]
    fail_tag = 10.0 * 1 + 2 + 1.0
    assert reports[0]["calls"] == [[t for t in plan_tags[0::2] if t != fail_tag]]
    assert reports[1]["calls"] == [[t for t in plan_tags[1::2] if t != fail_tag]]
    a, b = np.load(tmp_path / "tables_0.npz"), np.load(tmp_path / "tables_1.npz")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, str(tmp_path))
    from nys_koop_lqr_amd import harness
    import mpc_out_sweep_stubs as S
    plain = harness.lqr_sweep(*S.ARGS, fit_fn=S.fit_fn, loop_fn=S.loop_fn, controller=S.BOX)
    for name in harness.MPC_OUT_SCORE_NAMES + ("rmse_control",):
        assert a[name].shape == (3, 3) and np.array_equal(a[name], b[name], equal_nan=True), name
        assert np.array_equal(a[name], plain[name], equal_nan=True), name
    assert np.isnan(a["J"][1, 2]) and np.sum(np.isnan(a["J"])) == 1
    tags = np.array([[10.0 * si + k + 1.0 for k in range(3)] for si in range(3)])
    ok = ~np.isnan(a["J"])
    assert np.array_equal(a["y_viol_max"][ok], 0.125 * tags[ok]) and np.array_equal(a["n_y_viol"][ok], tags[ok] + 2.0)
