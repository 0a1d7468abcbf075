"""The plant-loop control law's reference, bars and class mirrors without a GPU (tests/plant_loop_reference.py).

1. the float64 emulation of the device's summation order, run as a closed loop around the library's host plants
   (nk_plant_step, nk_poly_plant_step) with distinct and with one shared reference, stays under the bar at every step of every
   case tests/test_gpu_plant_loop_steps.py runs; the worst err / bar is printed per section, and beside it the ratio against a
   bar that takes gram_reference.kblock_bar_direct alone for the kernel values (the module docstring says why that rule does
   not bound this arithmetic);
2. every planted fault exceeds the bar at some (trajectory, step), on 100 % of the (case, fault) pairs where the fault can
   occur: a landmark dropped (the last, the first of the second wave, the first of the second per-lane slot), two entries of w
   exchanged, a wave's word missing, a wave's word of step t - 2, kref of the next landmark, the next column of W, the inverse
   length scale left off one coordinate, x and x_ref exchanged;
3. every landmark of every case is visible: dropping it moves some control by more than twice its bar (the two runs of a case
   together) -- the GPU test runs the same states and inherits the condition;
4. the class mirrors agree with the documented limits, with nk_mpc_loop_max_m and with the constants in the sources.

S^-1 is a float64 eigendecomposition here; the GPU test reads the model's own."""
import os
import re

import numpy as np
import pytest

import plant_loop_reference as P
from test_gpu_poly_plant_loop import LIMITS
from test_poly_plant_host import make_plant

pytestmark = pytest.mark.skipif(not P.HAVE_LONGDOUBLE, reason=P.LONGDOUBLE_SKIP)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nys_koop_lqr_amd", "csrc")


@pytest.fixture(scope="module")
def nk():
    import __graft_entry__ as g
    g.build()
    import nys_koop_lqr_amd as nk
    return nk


def plant_of(nk, c):
    """The plant object of a case: the built-in plants in section A, polynomial tables elsewhere."""
    if c.section == "A":
        return {"duffing": nk.DuffingOscillator, "double_integrator": nk.DoubleIntegrator, "hjb": nk.HJB}[c.plant](Ts=P.TS)
    if c.plant in ("duffing", "hjb"):
        return getattr(nk.PolynomialSystem, c.plant)(P.TS)
    if c.plant == "P23":
        return nk.PolynomialSystem(P.P23[0], P.P23[1], P.P23[2], P.TS)
    return make_plant(c.plant, Ts=P.TS)


def closed_loop(c, q, plant, xref):
    """(X (B, STEPS + 1, d), U (B, STEPS, p)): the emulation's controls, the library's host plant step."""
    B = q["x0"].shape[0]
    X = np.empty((B, P.STEPS + 1, c.d))
    U = np.empty((B, P.STEPS, c.p))
    X[:, 0] = q["x0"]
    for t in range(P.STEPS):
        U[:, t] = P.emulate(q["spec"], q["w64"], X[:, t:t + 1], xref, q["lpt"], q["waves"], mpc=c.section == "D")[:, 0]
        for b in range(B):
            X[b, t + 1] = plant.step_library(X[b, t], U[b, t])
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(U)), P.name(c)
    return X, U


@pytest.fixture(scope="module")
def runs(nk):
    """runs(c) -> (problem, [(tag, xref, X, U, reference)] for the distinct and the shared references), computed once."""
    cache = {}

    def get(c):
        if c not in cache:
            q = P.problem(c, P.host_sinv(c.fam, c.d, c.m))
            plant = plant_of(nk, c)
            out = []
            for tag, xref in (("distinct", q["xref"]), ("shared", q["xref"][:1])):
                X, U = closed_loop(c, q, plant, xref)
                out.append((tag, xref, X, U, P.control_reference(q["spec"], q["w"], q["F"], X[:, :-1], xref, q["c"])))
            cache[c] = (q, out)
        return cache[c]
    return get


SECTIONS = {"A": P.A_CASES, "B": P.B_CASES, "D": P.D_CASES}


@pytest.mark.parametrize("section", sorted(SECTIONS))
def test_emulation_meets_the_bar(runs, section):
    worst, worst_direct, at = 0.0, 0.0, None
    for c in SECTIONS[section]:
        q, out = runs(c)
        assert (q["lpt"], q["waves"], q["c"]) == P.case_class(c)
        for tag, _, _, U, ref in out:
            r, where = P.worst(U, ref["u"], ref["bar"])
            assert r <= 1.0, f"{P.name(c)} {tag}: err / bar = {r:.3e} at (trajectory, step, input) {where}"
            if r > worst:
                worst, at = r, (P.name(c), tag) + where
            worst_direct = max(worst_direct, P.worst(U, ref["u"], ref["bar_direct"])[0])
    print(f"\n[plant-loop-steps host] section {section}: {len(SECTIONS[section])} cases, emulation worst err / bar "
          f"{worst:.3e} at {at}; against the direct kernel bar alone {worst_direct:.3e}")


def test_every_planted_fault_exceeds_the_bar(runs):
    table = {f: [0, 0, np.inf] for f in P.FAULTS}
    missed = []
    for c in P.ALL_CASES:
        q, out = runs(c)
        _, xref, X, _, ref = out[0]
        for f in P.FAULTS:
            if not P.fault_applies(f, q["spec"], c.p, q["lpt"], q["waves"], mpc=c.section == "D"):
                continue
            u = P.emulate(q["spec"], q["w64"], X[:, :-1], xref, q["lpt"], q["waves"], fault=f, mpc=c.section == "D")
            r, _ = P.worst(u, ref["u"], ref["bar"])
            table[f][0] += 1
            table[f][1] += r > 1.0
            table[f][2] = min(table[f][2], r)
            if not r > 1.0:
                missed.append((P.name(c), f, r))
    print("\n[plant-loop-steps host] fault: caught / applicable (cases), smallest worst err / bar")
    for f, (n, hit, lo) in table.items():
        print(f"  {f:18s} {hit:3d} / {n:3d}   {lo:.3e}")
    assert not missed, missed
    assert all(n > 0 for n, _, _ in table.values())


def test_every_landmark_is_visible(runs):
    total, seen, worst = 0, 0, np.inf
    hidden = []
    for c in P.ALL_CASES:
        _, out = runs(c)
        share = np.maximum.reduce([np.max(ref["share"], axis=(0, 1)) for *_, ref in out])
        total += share.size
        seen += int(np.sum(share > 2.0))
        worst = min(worst, float(share.min()))
        if not np.all(share > 2.0):
            hidden.append((P.name(c), int(np.sum(share <= 2.0)), float(share.min())))
    print(f"\n[plant-loop-steps host] landmark visibility: {seen} of {total} landmarks ({100.0 * seen / total:.1f} %) move some "
          f"control by more than twice its bar; the least visible one by {worst:.3e} bars")
    assert not hidden, hidden


def test_class_mirrors(nk):
    from nys_koop_lqr_amd import _lib
    for (d, p), limit in LIMITS.items():
        assert P.poly_loop_max_m(d, p) == limit
    assert [P.poly_loop_max_m(d, p) for d, p in ((2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (4, 2), (4, 3), (4, 4))] == \
        [4096, 4096, 2048, 2048, 2048, 2048, 1024, 1024]
    assert P.poly_loop_max_m(5, 1) == 0 and P.poly_loop_max_m(1, 5) == 0
    lib = _lib.load_library()
    for nv in (0, 1, 2, 3, 4, 16, 17, 32, 33, 39, 40, 41, 64, 65):
        assert lib.nk_mpc_loop_max_m(nv) == P.mpc_loop_max_m(nv), nv
    assert P.plant_loop_class(4096) == (4, 16) and P.PLANT_LOOP_MAX_M == 4096
    for m, want in P.LADDER_CLASS.items():
        assert P.plant_loop_class(m) == want
    assert {P.LADDER_CLASS[m][1] for m in P.LADDER} == {1, 2, 5, 16}
    assert P.poly_loop_class(257, 4, 4) == (1, 5) and P.poly_loop_class(129, 2, 3) == (2, 2) and P.poly_loop_class(64, 2, 1) == (1, 1)
    assert P.mpc_class(129, 4) == (16, 3) and P.mpc_class(512, 64) == (64, 8)
    # the constants in the sources
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("nk_plant_loop.hip", "nk_poly_lanes.h", "nk_mpc.h", "nk_loop_lanes.h")}
    assert re.search(r"constexpr int PLANT_LOOP_LPT = (\d+);", text["nk_plant_loop.hip"]).group(1) == str(P.PLANT_LOOP_LPT)
    assert re.search(r"constexpr int PLANT_LOOP_MAX_WAVES = (\d+);", text["nk_poly_lanes.h"]).group(1) == str(P.PLANT_LOOP_MAX_WAVES)
    assert "return D == 2 ? (P <= 2 ? 4 : 2) : (P <= 2 ? 2 : 1);" in text["nk_plant_loop.hip"]
    assert "constexpr int poly_pad_p(int p) { return p == 3 ? 4 : p; }" in text["nk_plant_loop.hip"]
    assert "constexpr int poly_pad_d(int d) { return d <= 2 ? 2 : 4; }" in text["nk_poly_lanes.h"]
    assert re.search(r"constexpr int MPC_MAX_WAVES = (\d+);", text["nk_mpc.h"]).group(1) == str(P.MPC_MAX_WAVES)
    assert "constexpr int MPC_LDS_DOUBLES = 160 * 1024 / 8;" in text["nk_mpc.h"]
    assert "if (nv <= 16) go(kt, dd, std::integral_constant<int, 16>{});" in text["nk_loop_lanes.h"]
    # every compiled (D, P) class of the polynomial loops is reached by section B, the padded ones included
    assert {(P.poly_pad_d(c.d), P.poly_pad_p(c.p)) for c in P.B_CASES} == {(D, Pp) for D in (2, 4) for Pp in (1, 2, 4)}
    assert {c.d for c in P.B_CASES} >= {1, 3} and 3 in {c.p for c in P.B_CASES}
    for c in P.B_CASES:
        assert c.m <= P.poly_loop_max_m(c.d, c.p)
    assert {(c.plant, c.m) for c in P.A_CASES if c.plant == "double_integrator"}
