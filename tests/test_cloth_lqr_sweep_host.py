"""CPU: the host side of the one-call cloth LQR sweep -- the C-ABI declares nk_closed_loop_multi and its unit struct and
_lib.LoopUnit mirrors it, harness.cloth_lqr_sweep plans with lqr_plan's per-seed draws and keeps its books around failing
fits and gains (stubs stand in for the fits, the device gains and the device loop), the x_s / y_s / z_s / final_us assembly
is the reference's lqr_control layout, and the sharded sweep at world size 2 assembles the one-rank table."""
import ctypes as C
import os
import re
import socket
import subprocess
import sys
import textwrap
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from nys_koop_lqr_amd import _lib
    return _lib.load_library()


def test_loop_unit_mirrors_the_header(lib):
    from nys_koop_lqr_amd import _lib
    header = open(os.path.join(ROOT, "include", "nyskoop.h")).read()
    assert "nk_closed_loop_multi" in _lib.SIGNATURES and hasattr(lib, "nk_closed_loop_multi")
    assert re.search(r"#define\s+NK_ABI_VERSION\s+2\b", header) and lib.nk_version() == 2  # a symbol added, nothing changed
    # nk_loop_unit on an LP64 target: six pointers, 48 bytes, no padding
    body = re.search(r"typedef struct nk_loop_unit \{(.*?)\} nk_loop_unit;", header, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["model", "K", "phi0", "phi_ref", "target", "u_init"]
    assert [f[0] for f in _lib.LoopUnit._fields_] == fields
    assert C.sizeof(_lib.LoopUnit) == 48
    assert [getattr(_lib.LoopUnit, f).offset for f in fields] == [0, 8, 16, 24, 32, 40]
    assert all(getattr(_lib.LoopUnit, f).size == 8 for f in fields)
    # the prototype: ctx, steps, c, units, n_units, out_x, out_u, out_ucum, out_err, scores
    proto = re.search(r"int nk_closed_loop_multi\((.*?)\);", header, re.S).group(1)
    assert len(proto.split(",")) == 10
    res, args = _lib.SIGNATURES["nk_closed_loop_multi"]
    assert res is C.c_int and len(args) == 10 and args[1] is C.c_int32 and args[2] is C.c_double
    assert args[3] is C.POINTER(_lib.LoopUnit)


M, P, D, STEPS = 5, 6, 192, 4


def _stubs(fail_fit=(), fail_gain=()):
    """Stand-ins for the device, tagged by the unit: a 'fit' whose regressor lifts to its tag, a device gain call that
    reports a non-zero status for chosen tags, a 'loop' that scores a unit by its tag and records what it was handed."""
    calls = []

    def tag_of(unit):
        return 100.0 * unit["ei"] + unit["si"] + 1.0

    def fit_fn(X, Y, n_inputs, params, unit, estimator):
        tag = tag_of(unit)
        if tag in fail_fit:
            return None
        assert estimator == unit["estimator"] and params is unit["params"]
        return SimpleNamespace(tag=tag, marks=unit["marks"], lift=lambda S, tag=tag: np.full((M, S.shape[1]), tag) + S[:1])

    def gain_batch_fn(regs, c):
        assert c == 0.0075
        return ([np.full((P, M), r.tag) for r in regs], [1 if r.tag in fail_gain else 0 for r in regs], [3] * len(regs))

    def loop_fn(regs, gains, lifts, targets, num_steps, c, u_inits, return_trajectories):
        tags = np.array([r.tag for r in regs])
        calls.append(tags.tolist())
        for K, (f0, fr), t, tg, ui in zip(gains, lifts, tags, targets, u_inits):
            assert np.all(K == t) and f0.shape == (M,) and np.all(f0 == t + 1.0) and np.all(fr == t + 2.0)
            assert tg.shape == (D,) and tg[0] == 2.0 and np.array_equal(ui, np.ones(P))  # x0[control_nodes]
        out = dict(J=tags, err_final=2.0 * tags, u_sumsq=3.0 * tags, u_absmax=-tags,
                   err=np.tile(tags[:, None], (1, num_steps)))
        if return_trajectories:
            out["states"] = np.tile(tags[:, None, None], (1, num_steps, D)) + np.arange(D)
            out["cum_controls"] = np.tile(tags[:, None, None], (1, num_steps + 1, P)) + np.arange(P)
        return out

    return fit_fn, gain_batch_fn, loop_fn, calls


def test_sweep_bookkeeping_with_stand_ins():
    import nys_koop_lqr_amd as nk
    from nys_koop_lqr_amd import harness
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((40, D + P)), rng.standard_normal((40, D))
    params = dict(kernel=nk.ThreeDimensionalKernel(1, 1, 1, D), gamma=1e-6)
    seeds = [3, 0, 7]
    x0, x_ref = np.ones(D), np.full(D, 2.0)
    args = (X, Y, P, params, M, seeds, x0, x_ref, STEPS)
    # plan order and landmark draws are lqr_plan's
    names, units = harness.cloth_lqr_plan(X, Y, P, params, M, seeds)
    ref = harness.lqr_plan(X, Y, P, params, [M], seeds)
    assert names == ["nystrom"] and [u["si"] for u in units] == [0, 1, 2] == [u["si"] for u in ref]
    for u, r, s in zip(units, ref, seeds):
        assert np.array_equal(u["marks"], r["marks"]) and u["m"] == M and u["estimator"] == "nystrom"
        assert np.array_equal(u["marks"], np.random.RandomState(s).choice(np.arange(0, 40), size=M, replace=False))
    fit_fn, gb, loop_fn, calls = _stubs()
    full = harness.cloth_lqr_sweep(*args, gain="device", fit_fn=fit_fn, loop_fn=loop_fn, gain_batch_fn=gb,
                                   return_trajectories=True)
    assert calls == [[1.0, 2.0, 3.0]]  # ONE loop call, every unit, in plan order
    tags = np.array([1.0, 2.0, 3.0])
    for name, want in (("J", tags), ("err_final", 2 * tags), ("u_sumsq", 3 * tags), ("u_absmax", -tags)):
        assert full[name].shape == (len(seeds),) and np.array_equal(full[name], want), name
    assert full["err"].shape == (3, STEPS) and np.array_equal(full["err"][:, 0], tags)
    assert set(full["timing"]) >= {"fit_s", "gain_wait_s", "loop_s", "gain_cpu_s", "total_s"}
    assert [np.array_equal(a["marks"], b["marks"]) for a, b in zip(full["units"], units)] == [True] * 3
    assert full["x_s"].shape == full["y_s"].shape == full["z_s"].shape == (3, D // 3, STEPS + 1)
    assert full["final_us"].shape == (3, P, STEPS + 1) and full["K_sim"].shape == (3, P, M)
    assert np.all(full["x_s"][:, :, 0] == 1.0) and np.array_equal(full["y_s"][1, :, 1], 2.0 + np.arange(1, D, 3))
    assert np.array_equal(full["final_us"][2, :, 0], 3.0 + np.array([0, 3, 1, 4, 2, 5]))
    # a unit whose fit fails and one whose gain fails: NaN, and not submitted
    fit_fn, gb, loop_fn, calls = _stubs(fail_fit=(1.0,), fail_gain=(3.0,))
    part = harness.cloth_lqr_sweep(*args, gain="device", fit_fn=fit_fn, loop_fn=loop_fn, gain_batch_fn=gb,
                                   return_trajectories=True)
    assert calls == [[2.0]]
    for name in harness.LOOP_SCORE_NAMES:
        assert np.all(np.isnan(part[name][[0, 2]])) and part[name][1] == full[name][1], name
    assert np.all(np.isnan(part["err"][[0, 2]])) and np.all(np.isnan(part["x_s"][[0, 2]])) and np.all(np.isnan(part["K"][0]))
    assert np.array_equal(part["z_s"][1], full["z_s"][1]) and np.array_equal(part["final_us"][1], full["final_us"][1])
    # nothing survives: no loop call at all
    fit_fn, gb, loop_fn, calls = _stubs(fail_fit=(1.0, 2.0, 3.0))
    none = harness.cloth_lqr_sweep(*args, gain="device", fit_fn=fit_fn, loop_fn=loop_fn, gain_batch_fn=gb)
    assert calls == [] and np.all(np.isnan(none["J"])) and "x_s" not in none
    # both estimators: a leading estimator axis, still ONE loop call; the spline units draw from the same per-seed streams
    fit_fn, gb, loop_fn, calls = _stubs()
    both = harness.cloth_lqr_sweep(X, Y, P, dict(nystrom=params, spline=dict(gamma=1e-6)), M, seeds, x0, x_ref, STEPS,
                                   estimator=("nystrom", "spline"), gain="device", fit_fn=fit_fn, loop_fn=loop_fn,
                                   gain_batch_fn=gb)
    assert calls == [[1.0, 2.0, 3.0, 101.0, 102.0, 103.0]] and both["J"].shape == (2, 3)
    assert np.array_equal(both["J"], [[1.0, 2.0, 3.0], [101.0, 102.0, 103.0]])
    sp = [u for u in both["units"] if u["estimator"] == "spline"]
    want = harness.spline_centers_draw(dict(m=M), X[:, :D], rng=np.random.RandomState(seeds[0]))
    assert sp[0]["marks"].shape == (D, M) and np.array_equal(sp[0]["marks"], want)
    # the host gain path: regressor.solve_lqr's arithmetic on the fitted operators; an operator set without a stabilising
    # solution is a NaN unit
    Aop = 0.5 * np.eye(M)
    Bop, Cop = rng.standard_normal((M, P)), rng.standard_normal((D, M))
    seen = []

    def fit_ops(X, Y, n_inputs, par, unit, est):
        bad = unit["si"] == 1
        return SimpleNamespace(A=np.full((M, M), np.nan) if bad else Aop, B=Bop, C=Cop, lift=lambda S: np.zeros((M, 2)))

    def loop_ops(regs, gains, lifts, targets, num_steps, c, u_inits, rt):
        seen.extend(gains)
        z = np.zeros(len(regs))
        return dict(J=z, err_final=z, u_sumsq=z, u_absmax=z, err=np.zeros((len(regs), num_steps)))

    host = harness.cloth_lqr_sweep(*args, fit_fn=fit_ops, loop_fn=loop_ops)
    assert len(seen) == 2 and np.isnan(host["J"][1]) and np.all(host["J"][[0, 2]] == 0.0)
    assert np.array_equal(seen[0], harness.lqr_default_gain(0.0075)(Aop, Bop, Cop))


def test_layout_is_the_reference_lqr_control():
    """cloth_control_layout on the states of the oracle's lifted loop and the running input sum against
    oracle.lqr_control_cloth (benchmark_lqr_cloth.py:69-104) on random operators: the same operations, so equal."""
    from nys_koop_lqr_amd import harness
    from oracle import nk_oracle as O
    rng = np.random.default_rng(4)
    m, steps = 9, 7
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    A, B, Cm = 0.9 * Q, 0.3 * rng.standard_normal((m, P)), rng.standard_normal((D, m))
    K = 0.2 * rng.standard_normal((P, m))
    phi0, phi_ref, x0 = rng.standard_normal(m), rng.standard_normal(m), rng.standard_normal(D)
    xs, us = O.lqr_closed_loop_lifted(A, B, Cm, K, phi0, phi_ref, steps)
    nodes = [168, 169, 170, 189, 190, 191]
    sc = harness.closed_loop_scores(xs.T, us.T, np.zeros(D), u_init=x0[nodes])
    got = harness.cloth_control_layout(x0, xs.T, sc["cum_controls"])
    want = O.lqr_control_cloth(A, B, Cm, K, phi0, phi_ref, x0, steps)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)
    # and the scores are the documented formulas
    tgt = rng.standard_normal(D)
    sc = harness.closed_loop_scores(xs.T, us.T, tgt, c=0.3)
    sse = np.sum((xs.T - tgt) ** 2, axis=1)
    assert np.allclose(sc["err"], np.sqrt(sse / D), rtol=1e-14) and sc["err_final"] == sc["err"][-1]
    assert np.isclose(sc["J"], 0.3 * sse.sum() + np.sum(us ** 2), rtol=1e-13)
    assert np.isclose(sc["u_sumsq"], np.sum(us ** 2), rtol=1e-13) and sc["u_absmax"] == np.max(np.abs(us))
    bad = us.T.copy()
    bad[2, 1] = np.nan
    assert np.isnan(harness.closed_loop_scores(xs.T, bad, tgt)["u_absmax"])


WORKER = textwrap.dedent("""
    import os, sys, json
    import numpy as np
    sys.path.insert(0, {root!r})
    sys.path.insert(0, os.path.join({root!r}, "tests"))
    from nys_koop_lqr_amd import dist as nkd
    from test_cloth_lqr_sweep_host import sharded_case
    rank, world = nkd.init_process_group("gloo")
    res = sharded_case(nkd)
    np.save(os.path.join({out!r}, f"scores_{{rank}}.npy"), np.stack([res[k] for k in ("J", "err_final", "u_sumsq", "u_absmax")]))
    print(json.dumps(dict(rank=rank, world=world)))
""")


def sharded_case(nkd):
    """Five seeds x two estimators through dist.sharded_cloth_lqr_sweep with the stand-ins; one fit and one gain fail."""
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((40, D + P)), rng.standard_normal((40, D))
    fit_fn, gb, loop_fn, _ = _stubs(fail_fit=(2.0,), fail_gain=(104.0,))
    return nkd.sharded_cloth_lqr_sweep(X, Y, P, dict(nystrom=dict(kernel=None, gamma=1e-6), spline=dict(gamma=1e-6)), M,
                                       [0, 1, 2, 3, 4], np.ones(D), np.full(D, 2.0), STEPS, estimator=("nystrom", "spline"),
                                       gain="device", fit_fn=fit_fn, loop_fn=loop_fn, gain_batch_fn=gb)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_sharded_sweep_world2_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, out=str(tmp_path)))
    env = dict(os.environ, OMP_NUM_THREADS="2", OPENBLAS_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    s0, s1 = np.load(tmp_path / "scores_0.npy"), np.load(tmp_path / "scores_1.npy")
    from nys_koop_lqr_amd import dist as nkd
    one = sharded_case(nkd)
    want = np.stack([one[k] for k in ("J", "err_final", "u_sumsq", "u_absmax")])
    assert want.shape == (4, 2, 5) and np.array_equal(s0, s1, equal_nan=True) and np.array_equal(s0, want, equal_nan=True)
    hole = np.zeros((2, 5), dtype=bool)
    hole[0, 1] = hole[1, 3] = True
    assert np.all(np.isnan(want[:, hole])) and np.all(np.isfinite(want[:, ~hole]))
    assert np.array_equal(want[0][~hole], [1.0, 3.0, 4.0, 5.0, 101.0, 102.0, 103.0, 105.0])
