"""GPU: the QP iteration of the MPC loops step by step, on every lane class.

Every control and every info pair {iterations, final max |s - z|} the device returns is recomputed in longdouble from the
state x_t and the control u_{t-1} the device stored (tests/mpc_qp_reference.py: gradient rows folded in longdouble from the
model's own K_mm^-1/2, H^-1, M, Kb, S0 inverted in longdouble from the H, G, rho passed, the iteration in the interface's order)
and held entry by entry under the bar propagated there; no tolerance is chosen, and nothing of the library stands on the
reference side.  8 steps, 16 starts spread over the state box, non-zero u_init for half of them.  All calls go through
reg.closed_loop_plant_mpc(..., return_info=True) and harness.mpc_loop_multi.

A. no output rows, m = 65: nv = 1, 2, 3, 4, 15, 16 (p = 1 and 4), 17, 31, 32, 33, 63, 64 (p = 1, 2, 4) -- the edges of the
   register classes NP = 16, 32, 64 -- in three regimes (active: box at 0.3 and rates at 0.1 of the median start |H^-1 g|,
   tol = 0; inactive; early stop at the reference's median r of iteration 5), the ladder iters = 1, 2, 3 at the default rho
   and 30 at the designed rho, one-sided limits at one shape per class; then m = 1, 63, 64, 128, 129 and nk_mpc_loop_max_m(nv)
   at nv = 16 (p = 1) and nv = 64 (p = 4), and RBF, linear and spline models at nv = 17 (Matern everywhere else); d = 1, 2, 3, 4.
B. output rows (nv, ny) = (1, 1), (12, 4), (13, 4), (28, 4), (30, 3), (48, 16), (63, 1), (1, 63), hard and soft, at m = 65 (all
   regimes) and at nk_mpc_loop_max_m(nv + ny).
C. the multi forms: per plant, the units of A in one nk_mpc_loop_multi call and those of B in one nk_mpc_out_loop_multi call,
   in a shuffled order: states, controls and info are the bits of the single calls, and without trajectory outputs the scores
   are the bits of the storing call.
Per run: u_t and info[t, 1] under their bars, info[t, 0] equal on every unambiguous step (at most 2 % are ambiguous),
x_{t+1} = nk_poly_plant_step(x_t, u_t) and row 0 = x0 bit for bit, every control inside the rate limits as the loop forms
them and inside the box unless pinned to a rate limit outside it, one trajectory alone has the bits it has in the batch, every
lane and every landmark visible on the device's own trajectories.

Worst err / bar on an MI355X (profiles/mpc_qp_steps.log; 73 passed in 10.4 s, none skipped; the bars were fixed by the host test
before the first device run and none was changed): A 1.3e-3 / 5.3e-4 / 4.0e-4 at NP 16 / 32 / 64 with iterations (the early-stop
runs) and 2.5e-3 on an inactive run, where the bar is the start's alone; B 4.7e-4 / 3.5e-4 / 5.3e-4 and 1.2e-3; 4.8e-8 and 7.2e-6
at eight waves; C bit for bit.  Iteration counts equal everywhere, no ambiguous step.  The ratios are small because the gradient
bar is a worst-case sum over the landmarks; what the bar still resolves is measured by the host test: the weakest planted fault
exceeds it by 232 bars (S0 read untransposed at nv = 12, ny = 4, 30 iterations; every other fault by 1.2e4 or more), the least
visible lane moves a control by 2.9e5 bars (host and device), the least visible landmark a gradient row by 5.5e6 bars, and the
control's bar grows over 30 iterations at the designed rho by a factor of 131 at most.  No defect was found."""
import numpy as np
import pytest

import mpc_qp_reference as Q
import plant_loop_reference as P
from test_gpu_plant_loop_steps import models, nk  # noqa: F401  (fixtures)
from test_mpc_qp_reference_host import plant_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not Q.HAVE_LONGDOUBLE, reason=Q.LONGDOUBLE_SKIP)]


@pytest.fixture(scope="module")
def problems(models):  # noqa: F811
    """problems(c) -> (regressor, designed problem around the model's own S^-1), computed once."""
    cache = {}

    def get(c):
        if c not in cache:
            reg, Sinv = models(c.fam, c.d, c.m, c.p)
            cache[c] = (reg, Q.problem(c, Sinv))
        return cache[c]
    return get


def call(reg, q, run, plant, b=None):
    """The device loop of a run: the whole batch, or trajectory b alone."""
    sel = (lambda a: a) if b is None else (lambda a: a[b])
    return reg.closed_loop_plant_mpc(Q.controller(q, run), sel(q.x0), sel(q.xref), Q.STEPS, plant, iters=run.iters,
                                     tol=Q.run_tol(q, run), u_init=sel(q.u_init), return_info=True)


def check_limits(q, ctl, U, label):
    """Inside the rate limits as the loop forms them (u_prev + dlo in float64); inside the box, or on a rate limit beyond it."""
    p = q.c.p
    up = Q.uprev_of(q, U)
    dlo, dhi = up + ctl.dlo[:p], up + ctl.dhi[:p]
    assert np.all((U >= dlo) & (U <= dhi)), label
    assert np.all(((U >= ctl.lo[:p]) & (U <= ctl.hi[:p])) | (U == dlo) | (U == dhi)), label


def check_case(nk, problems, c):  # noqa: F811
    reg, q = problems(c)
    plant = plant_of(nk, c)
    nt = c.p * c.N + c.ny
    np_class, waves = P.mpc_class(c.m, nt)
    vis, share, ratios = None, None, {}
    for run in Q.runs_of(c):
        label = f"{Q.name(c)} {run.tag}"
        ctl = Q.controller(q, run)
        S, U, I = call(reg, q, run, plant)
        assert S.shape == (Q.BATCH, Q.STEPS + 1, c.d) and U.shape == (Q.BATCH, Q.STEPS, c.p) and I.shape == (Q.BATCH, Q.STEPS, 2)
        assert np.all(np.isfinite(S)) and np.all(np.isfinite(U)) and np.all(np.isfinite(I)), label
        assert np.array_equal(S[:, 0], q.x0), label
        for b in range(Q.BATCH):  # the plant step and the stores: bit for bit
            for t in range(Q.STEPS):
                want = plant.step_library(S[b, t], U[b, t])
                assert np.array_equal(S[b, t + 1], want), (label, b, t, S[b, t + 1], want)
        check_limits(q, ctl, U, label)
        S1, U1, I1 = call(reg, q, run, plant, b=5)  # a trajectory has the same bits alone and in the batch
        assert np.array_equal(S1.T, S[5]) and np.array_equal(U1.T, U[5]) and np.array_equal(I1, I[5]), label
        ref = Q.reference(q, run, S, U)
        cmp_ = Q.compare(ref, U, I)
        g = ref["growth"]
        print(f"\n[mpc-qp-steps] {label}: class NP {np_class} waves {waves}; control err / bar {cmp_['u']:.3e} at (trajectory, "
              f"step, input) {cmp_['at_u']}; residual err / bar {cmp_['r']:.3e} at {cmp_['at_r']}; iterations "
              f"{int(I[..., 0].min())} .. {int(I[..., 0].max())}; ambiguous steps {cmp_['n_amb']}; bar growth "
              + (f"{g[-1] / g[0]:.1f} over {len(g)} iterations" if g else "-"))
        assert cmp_["u"] <= 1.0, f"{label}: control err / bar = {cmp_['u']:.3e} at (trajectory, step, input) {cmp_['at_u']}"
        assert cmp_["r"] <= 1.0, f"{label}: residual err / bar = {cmp_['r']:.3e} at (trajectory, step) {cmp_['at_r']}"
        assert cmp_["same_it"], f"{label}: iteration counts differ on an unambiguous step"
        assert cmp_["n_amb"] <= Q.AMBIGUITY_CAP * Q.BATCH * Q.STEPS, (label, cmp_["n_amb"])
        if run.regime == "active":
            assert float(np.min(ref["margin"])) > 1e3, (label, "r_0 / bar", float(np.min(ref["margin"])))
            if run.tol == 0.0:
                assert np.all(I[..., 0] == run.iters), label
        else:
            assert np.all(I == 0.0), label
        ratios[run.tag] = max(cmp_["u"], cmp_["r"])
        vis = ref["vis"] if vis is None else np.maximum(vis, ref["vis"])
        mine = np.max(ref["share"], axis=(0, 1))
        share = mine if share is None else np.maximum(share, mine)
    print(f"[mpc-qp-steps] {Q.name(c)}: least visible lane {vis.min():.3e} bars, least visible landmark {share.min():.3e} bars")
    assert np.all(vis > 2.0), (Q.name(c), "lanes hidden behind the bar", int(np.sum(vis <= 2.0)))
    assert np.all(share > 2.0), (Q.name(c), "landmarks hidden behind the bar", int(np.sum(share <= 2.0)))
    return ratios


# ---------------------------------------------------------------------------------------------------------------------
# A. no output rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", Q.A_CASES, ids=Q.name)
def test_input_lanes(nk, problems, c):  # noqa: F811
    from nys_koop_lqr_amd import _lib
    assert c.m <= _lib.load_library().nk_mpc_loop_max_m(c.p * c.N)
    check_case(nk, problems, c)


# ---------------------------------------------------------------------------------------------------------------------
# B. output rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", Q.B_CASES, ids=Q.name)
def test_output_rows(nk, problems, c):  # noqa: F811
    from nys_koop_lqr_amd import _lib
    assert c.m <= _lib.load_library().nk_mpc_loop_max_m(c.p * c.N + c.ny)
    check_case(nk, problems, c)


# ---------------------------------------------------------------------------------------------------------------------
# C. the multi forms
# ---------------------------------------------------------------------------------------------------------------------
RUN3 = Q.Run("it3", "active", "all", "default", 3, 0.0)
RUN30 = Q.Run("it30", "active", "all", "small", 30, 0.0)


def _check_multi(nk, problems, cases, seed, score_names):  # noqa: F811
    from nys_koop_lqr_amd import harness
    units = []
    for k, c in enumerate(cases):
        reg, q = problems(c)
        units.append((c, reg, q, RUN30 if k % 3 == 2 else RUN3, (3 + 5 * k) % Q.BATCH))
    units = [units[i] for i in np.random.default_rng(seed).permutation(len(units))]
    plant = plant_of(nk, cases[0])
    alone = [call(reg, q, run, plant, b=b) for _, reg, q, run, b in units]
    args = ([u[1] for u in units], [Q.controller(u[2], u[3]) for u in units], np.stack([u[2].x0[u[4]] for u in units]),
            np.stack([u[2].xref[u[4]] for u in units]), Q.STEPS, plant)
    kw = dict(iters=[u[3].iters for u in units], tol=0.0, u_inits=np.stack([u[2].u_init[u[4]] for u in units]))
    out = harness.mpc_loop_multi(*args, **kw, return_trajectories=True, return_info=True)
    for i, (S1, U1, I1) in enumerate(alone):
        label = (i, Q.name(units[i][0]), units[i][3].tag)
        assert np.array_equal(out["states"][i], S1.T) and np.array_equal(out["controls"][i], U1.T), label
        assert np.array_equal(out["info"][i], I1), label
    bare = harness.mpc_loop_multi(*args, **kw)
    assert "states" not in bare and "info" not in bare
    for nm in score_names:
        assert np.all(np.isfinite(out[nm])) and np.array_equal(bare[nm], out[nm]), nm
    assert np.array_equal(out["iters_sum"], [u[3].iters * Q.STEPS for u in units])
    return len(units), {P.mpc_class(u[0].m, u[0].p * u[0].N + u[0].ny) for u in units}


# the classes (NP, waves) a plant group must meet, written out where the group spans several
WANT_CLASSES = {("A", "duffing"): {(16, 1), (16, 2), (16, 3), (16, 8), (32, 2), (64, 2)},
                ("A", "P4b"): {(16, 2), (64, 1), (64, 2), (64, 3), (64, 5)},
                ("B", "duffing"): {(16, 2), (16, 8), (32, 2), (32, 8), (64, 2), (64, 5)},
                ("B", "P4b"): {(64, 2), (64, 5)}}


def _plants(cases):
    return sorted({c.plant for c in cases})


@pytest.mark.parametrize("plant", _plants(Q.A_CASES))
def test_multi_form_input_lanes(nk, problems, plant):  # noqa: F811
    from nys_koop_lqr_amd import harness
    cases = [c for c in Q.A_CASES if c.plant == plant]
    n, classes = _check_multi(nk, problems, cases, 47, harness.MPC_SCORE_NAMES)
    assert classes == WANT_CLASSES.get(("A", plant), classes), sorted(classes)
    print(f"\n[mpc-qp-steps] C nk_mpc_loop_multi {plant}: {n} units, classes (NP, waves) {sorted(classes)}: the bits of the single "
          "calls; scores without trajectories: the same bits")


@pytest.mark.parametrize("plant", _plants(Q.B_CASES))
def test_multi_form_output_rows(nk, problems, plant):  # noqa: F811
    from nys_koop_lqr_amd import harness
    cases = [c for c in Q.B_CASES if c.plant == plant]
    n, classes = _check_multi(nk, problems, cases, 53, harness.MPC_OUT_SCORE_NAMES)
    assert classes == WANT_CLASSES.get(("B", plant), classes), sorted(classes)
    print(f"\n[mpc-qp-steps] C nk_mpc_out_loop_multi {plant}: {n} units, classes (NP, waves) {sorted(classes)}: the bits of the "
          "single calls; scores without trajectories: the same bits")
