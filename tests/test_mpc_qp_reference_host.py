"""The MPC loop's QP reference, bars and planted faults without a GPU (tests/mpc_qp_reference.py).

On trajectories advanced with the library's host plant step (nk_poly_plant_step) under the float64 emulation's controls:
1. the emulation stays under the bar on every run of every case tests/test_gpu_mpc_qp_steps.py runs (controls and residual,
   entry by entry), with the reference's iteration count on every step that is not ambiguous;
2. every planted fault exceeds the bar by a factor 2 or more on every (case, run) where fault_applies says it can occur;
3. every lane moves some control by more than twice its bar through the M (Kb) product, and every landmark through g;
4. at most 2 % of a case's steps are ambiguous, and every step of the active regime has r_0 above 1e3 times its bar;
5. the inactive regime returns info = (0, 0) exactly;
6. the bounds dKb, dS0 hold against the float64 mirror of mpc_spd_inverse and of the mpc_out_prepare products;
7. the class mirrors and the cited source lines are what the reference's docstring says.
The bar's growth over the iterations is printed.  S^-1 is a float64 eigendecomposition here; the GPU test reads the model's own."""
import os

import numpy as np
import pytest

import mpc_qp_reference as Q
import plant_loop_reference as P
from test_plant_loop_reference_host import plant_of as _plant_of

pytestmark = pytest.mark.skipif(not Q.HAVE_LONGDOUBLE, reason=Q.LONGDOUBLE_SKIP)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nys_koop_lqr_amd", "csrc")
FAULT_RUNS = ("it3", "it30", "early", "lo_only", "no_rate", "no_box")


@pytest.fixture(scope="module")
def nk():
    import __graft_entry__ as g
    g.build()
    import nys_koop_lqr_amd as nk
    return nk


def plant_of(nk, c):
    """The polynomial plant of a case (plant_loop_reference's table)."""
    return _plant_of(nk, c._replace(section="poly"))


def closed_loop(q, run, plant):
    """(X (B, STEPS + 1, d), U (B, STEPS, p), info (B, STEPS, 2)): the emulation's controls, the library's host plant step."""
    c = q.c
    X, U, I = np.empty((Q.BATCH, Q.STEPS + 1, c.d)), np.empty((Q.BATCH, Q.STEPS, c.p)), np.empty((Q.BATCH, Q.STEPS, 2))
    X[:, 0] = q.x0
    up = q.u_init
    for t in range(Q.STEPS):
        U[:, t], I[:, t] = Q.emulate_step(q, run, X[:, t], up)
        up = U[:, t]
        for b in range(Q.BATCH):
            X[b, t + 1] = plant.step_library(X[b, t], U[b, t])
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(U)), (Q.name(c), run.tag)
    return X, U, I


@pytest.fixture(scope="module")
def runs(nk):
    """runs(c) -> (problem, {run: (X, U, info, reference)}), computed once."""
    cache = {}

    def get(c):
        if c not in cache:
            q = Q.problem(c, P.host_sinv(c.fam, c.d, c.m))
            plant = plant_of(nk, c)
            out = {}
            for run in Q.runs_of(c):
                X, U, I = closed_loop(q, run, plant)
                out[run] = (X, U, I, Q.reference(q, run, X, U))
            cache[c] = (q, out)
        return cache[c]
    return get


SECTIONS = {"A": Q.A_CASES, "B": Q.B_CASES}


@pytest.mark.parametrize("section", sorted(SECTIONS))
def test_emulation_meets_the_bar(runs, section):
    worst, at, n_amb, n_steps, growth = 0.0, None, 0, 0, {}
    for c in SECTIONS[section]:
        q, out = runs(c)
        case_amb = 0
        for run, (X, U, I, ref) in out.items():
            cmp_ = Q.compare(ref, U, I)
            label = f"{Q.name(c)} {run.tag}"
            assert cmp_["u"] <= 1.0, f"{label}: control err / bar = {cmp_['u']:.3e} at (trajectory, step, input) {cmp_['at_u']}"
            assert cmp_["r"] <= 1.0, f"{label}: residual err / bar = {cmp_['r']:.3e} at (trajectory, step) {cmp_['at_r']}"
            assert cmp_["same_it"], f"{label}: iteration counts differ on an unambiguous step"
            assert cmp_["n_amb"] <= Q.AMBIGUITY_CAP * U.shape[0] * U.shape[1], (label, cmp_["n_amb"])
            case_amb += cmp_["n_amb"]
            if run.regime == "active":
                assert float(np.min(ref["margin"])) > 1e3, (label, "r_0 / bar", float(np.min(ref["margin"])))
                if run.tol == 0.0:
                    assert np.all(I[..., 0] == run.iters), label
            else:
                assert np.all(I == 0.0) and np.all(ref["it"] == 0) and np.all(ref["r"] == 0), label
            if max(cmp_["u"], cmp_["r"]) > worst:
                worst, at = max(cmp_["u"], cmp_["r"]), label
            if run.tag == "it30" and ref["growth"]:
                g = ref["growth"]
                growth[P.mpc_class(c.m, c.p * c.N + c.ny)[0]] = max(growth.get(P.mpc_class(c.m, c.p * c.N + c.ny)[0], 0.0), g[-1] / g[0])
        n_amb += case_amb
        n_steps += len(out) * Q.BATCH * Q.STEPS
    print(f"\n[mpc-qp-steps host] section {section}: {len(SECTIONS[section])} cases, emulation worst err / bar {worst:.3e} at "
          f"{at}; ambiguous steps {n_amb} of {n_steps}; control bar after iteration 30 over the bar after iteration 1, "
          f"largest per NP class: " + ", ".join(f"{k}: {v:.2f}" for k, v in sorted(growth.items())))


def test_every_planted_fault_exceeds_the_bar(runs):
    table = {f: [0, 0, np.inf] for f in Q.FAULTS}
    missed = []
    for c in Q.ALL_CASES:
        q, out = runs(c)
        for run, (X, U, I, ref) in out.items():
            if run.tag not in FAULT_RUNS:
                continue
            for f in Q.FAULTS:
                if not Q.fault_applies(f, c, run):
                    continue
                em = Q.emulate(q, run, X, U, fault=f)
                cmp_ = Q.compare(ref, em["u"], np.stack([em["it"].astype(np.float64), em["r"]], axis=-1))
                r = np.inf if not cmp_["same_it"] else max(cmp_["u"], cmp_["r"])
                table[f][0] += 1
                table[f][1] += r >= 2.0
                table[f][2] = min(table[f][2], r)
                if not r >= 2.0:
                    missed.append((Q.name(c), run.tag, f, r))
    print("\n[mpc-qp-steps host] fault: caught / applicable (case, run) pairs, smallest worst err / bar")
    for f, (n, hit, lo) in table.items():
        print(f"  {f:18s} {hit:3d} / {n:3d}   {lo:.3e}")
    assert not missed, missed
    assert all(n > 0 for f, (n, _, _) in table.items() if f != "dn_wrap")


def test_every_lane_and_landmark_is_visible(runs):
    lanes, worst_lane, worst_lm, hidden = 0, np.inf, np.inf, []
    for c in Q.ALL_CASES:
        _, out = runs(c)
        vis = np.maximum.reduce([ref["vis"] for *_, ref in out.values()])
        share = np.maximum.reduce([np.max(ref["share"], axis=(0, 1)) for *_, ref in out.values()])
        lanes += vis.size
        worst_lane, worst_lm = min(worst_lane, float(vis.min())), min(worst_lm, float(share.min()))
        if not (np.all(vis > 2.0) and np.all(share > 2.0)):
            hidden.append((Q.name(c), int(np.sum(vis <= 2.0)), int(np.sum(share <= 2.0))))
    print(f"\n[mpc-qp-steps host] visibility: {lanes} lanes, the least visible one moves a control by {worst_lane:.3e} bars; the "
          f"least visible landmark moves a gradient row by {worst_lm:.3e} bars")
    assert not hidden, hidden


def test_prepare_bounds_hold_for_the_float64_mirror():
    worst = 0.0
    for c in Q.ALL_CASES:
        H, G = Q._design(c, Q.DESIGN_DRAW.get(Q.name(c), 0))[:2]
        for rho in (Q.default_rho(H), Q.small_rho(H, G)):
            ld, f64 = Q.matrices_ld(H, G, rho, c.p), Q.matrices64(H, G, rho, c.p)
            for a, b, bar in ((f64.Kb, ld.Kb, ld.dKb), (f64.S0, ld.S0, ld.dS0)):
                r = P.worst(a, b, bar)[0]
                assert r <= 1.0, (Q.name(c), rho, r)
                worst = max(worst, r)
    print(f"\n[mpc-qp-steps host] float64 mirror of mpc_spd_inverse / mpc_out_prepare against dKb, dS0: worst ratio {worst:.3e}")


def test_class_mirrors_and_cited_lines(nk):
    from nys_koop_lqr_amd import _lib
    lib = _lib.load_library()
    for nt, want in ((1, 16), (15, 16), (16, 16), (17, 32), (31, 32), (32, 32), (33, 64), (63, 64), (64, 64)):
        assert P.mpc_class(65, nt) == (want, 2)
    for nt in range(0, 66):
        assert lib.nk_mpc_loop_max_m(nt) == P.mpc_loop_max_m(nt), nt
    assert P.mpc_loop_max_m(16) == 512 and P.mpc_loop_max_m(64) == 314
    assert {P.mpc_class(c.m, c.p * c.N + c.ny)[0] for c in Q.A_CASES} == {16, 32, 64}
    assert {P.mpc_class(c.m, c.p * c.N + c.ny)[0] for c in Q.B_CASES} == {16, 32, 64}
    assert {P.poly_pad_d(c.d) for c in Q.A_CASES} == {2, 4} and {c.d for c in Q.A_CASES} == {1, 2, 3, 4}
    assert {c.fam for c in Q.A_CASES} == {"rbf", "matern", "linear", "spline"}
    for c in Q.ALL_CASES:
        assert c.m <= P.mpc_loop_max_m(c.p * c.N + c.ny)
    src = {f: open(os.path.join(CSRC, f)).read().split("\n") for f in ("nk_mpc_loop.hip", "nk_mpc.h", "nk_mpc_out.h")}

    def has(f, first, last, text):
        assert any(text in ln for ln in src[f][first - 1:last]), (f, first, last, text)

    has("nk_mpc_loop.hip", 171, 173, "a = fma(hc[j * nt], lane_bcast(gt, j), a)")
    has("nk_mpc_loop.hip", 149, 153, "const double ds = lane >= p ? s - shifted : s;")
    has("nk_mpc_loop.hip", 154, 159, "theta != 0.0 ? c1 + theta * (v - c1) : c1")
    has("nk_mpc_loop.hip", 181, 196, "const double dt = lane + p < nv ? w2 - w2n : w2;")
    has("nk_mpc_loop.hip", 181, 196, "const double rhs = Q.rho * ((z1 - l1) + dt) - g;")
    has("nk_mpc_loop.hip", 181, 196, "for (int j = 0; j < NP; ++j) U = fma(Krow[j], lane_bcast(rhs, j), U);")
    has("nk_mpc_loop.hip", 181, 196, "l1 = l1 + (s1 - z1);")
    has("nk_mpc_loop.hip", 127, 203, "const double uc = clipd(clipd(z1, lo, hi), dlo, dhi);")
    has("nk_mpc.h", 77, 106, "inline bool mpc_spd_inverse(const double* A, int n, double* inv)")
    has("nk_mpc.h", 113, 120, "A[i * nv + i] += ds.rho * (i + p < nv ? 3.0 : 2.0);")
    has("nk_mpc.h", 143, 215, "inline void mpc_qp(")
    has("nk_mpc_out.h", 53, 66, "A[i * nv + j] += ds.rho * s;")
    has("nk_mpc_out.h", 69, 101, "Kb[i * nt + nv + r] = Kb[(nv + r) * nt + i] = (MG[(size_t)i * ny + r] + gm) / 2;")
    has("nk_mpc_out.h", 105, 105, "rho / (rho + y_weight)")
    has("nk_mpc_out.h", 123, 207, "inline void mpc_out_qp(")
