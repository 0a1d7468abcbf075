#!/usr/bin/env python3
"""Host time of the Python bindings alone: the median over --calls calls of each packing method of _lib.Context and of
closed_loop_plant / closed_loop_plant_mpc, with a stand-in library whose entry points return at once.  Needs no GPU and no
libnyskoop.so.  The table calls pack 200 units (m = 20, p = 1, 100 steps, scores alone); the single-call loops run batch 1,
where the bindings are the largest share of a call.  Prints one JSON line, microseconds per call."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import _lib


class NoLib:
    """Every nk_* entry point: return NK_OK, touch nothing."""

    def __getattr__(self, name):
        if not name.startswith("nk_"):
            raise AttributeError(name)
        fn = lambda *a: 0
        setattr(self, name, fn)
        return fn


class Reg(nk.KoopmanNystromRegressor):
    def __init__(self, p, d, m):
        super().__init__(p)
        self._shape = (d, m)

    def _ensure_model(self):
        return 0x1000

    def _landmark_shape(self):
        return self._shape


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--units", type=int, default=200)
    args = ap.parse_args()
    n, m, p, d, steps = args.units, 20, 1, 2, 100
    rng = np.random.default_rng(0)
    ctx = _lib.Context.__new__(_lib.Context)
    ctx.handle, ctx.lib, ctx.device = C.c_void_p(7), NoLib(), 0
    _lib.get_context = lambda device=None: ctx
    _lib.load_library = lambda: ctx.lib  # (a PolynomialSystem has the library check its table)
    models = [0x1000 + 16 * i for i in range(n)]
    gains = [rng.standard_normal((p, m)) for _ in range(n)]
    x0s, x_refs = rng.standard_normal((n, d)), rng.standard_normal((n, d))
    u_opt = rng.standard_normal(steps)
    plant = nk.PolynomialSystem.duffing(0.01)
    desc = plant.descriptor()
    ctl = SimpleNamespace(H=np.eye(10), F=rng.standard_normal((10, m)), K=gains[0], lo=np.full(10, -1.0), hi=np.full(10, 1.0),
                          dlo=np.full(10, -np.inf), dhi=np.full(10, np.inf), rho=1.0, horizon=10)
    ds, keep = _lib.mpc_desc(ctl, 50, 0.0)
    dims3 = [(m, p, d)] * n
    dims2 = [(m, p)] * n
    phis = [rng.standard_normal(m) for _ in range(n)]
    targets = [rng.standard_normal(d) for _ in range(n)]
    As = [rng.standard_normal((m, m)) for _ in range(n)]
    Bs = [rng.standard_normal((m, p)) for _ in range(n)]
    Qs, Rs = [np.eye(m)] * n, [np.eye(p)] * n
    specs = [(10, [], None)] * n
    reg = Reg(p, d, m)
    duffing = nk.DuffingOscillator(Ts=0.01)
    x0, x_ref = x0s[0], x_refs[0]
    cases = {
        "plant_loop_multi": lambda: ctx.plant_loop_multi(0, 0.01, steps, models, gains, x0s, x_refs, u_opt),
        "poly_plant_loop_multi": lambda: ctx.poly_plant_loop_multi(desc, steps, models, gains, x0s, x_refs, u_opt),
        "mpc_loop_multi": lambda: ctx.mpc_loop_multi(desc, steps, models, [ds] * n, x0s, x_refs, None, u_opt),
        "closed_loop_multi": lambda: ctx.closed_loop_multi(steps, 0.0075, models, dims3, gains, phis, phis, targets, None, False,
                                                           False, False, False),
        "dare_batch": lambda: ctx.dare_batch(As, Bs, Qs, Rs),
        "model_lqr_gain_batch": lambda: ctx.model_lqr_gain_batch(models, 1.0, None, dims=dims2),
        "mpc_build_batch": lambda: ctx.mpc_build_batch(As, Bs, Qs, Rs, [10] * n),
        "model_mpc_build_batch": lambda: ctx.model_mpc_build_batch(models, dims2, 1.0, None, specs),
        "model_lqr_gain": lambda: ctx.model_lqr_gain(models[0], m, p, 1.0),
        "closed_loop_plant": lambda: reg.closed_loop_plant(gains[0], x0, x_ref, steps, duffing),
        "closed_loop_plant_mpc": lambda: reg.closed_loop_plant_mpc(ctl, x0, x_ref, steps, plant),
    }
    out = {}
    for name, fn in cases.items():
        for _ in range(10):
            fn()
        ts = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        out[name] = round(1e6 * statistics.median(ts), 1)
    del keep
    print(json.dumps(dict(calls=args.calls, units=n, median_us=out)))


if __name__ == "__main__":
    main()
