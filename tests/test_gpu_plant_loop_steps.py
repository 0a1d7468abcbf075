"""GPU: the control law of the plant-in-the-loop family step by step, on every workgroup class.

Every control the device returns is recomputed in longdouble from the state the device returned for that step
(tests/plant_loop_reference.py: u_ref = sum_l w_l (k(z_l, x_ref) - k(z_l, x_t)), w folded in longdouble from the model's own
K_mm^-1/2) and held entry by entry under the bar derived there; no tolerance is chosen, and nothing of the library stands on
the reference side.  32 steps, so that both parity buffers of the wave words are reused many times; 16 starts spread over the
state box, so that every landmark of every case moves some control by more than twice its bar
(tests/test_plant_loop_reference_host.py asserts that on the emulation's states; it is asserted again here on the device's).
Every case asserts the class the mirror of the sources predicts and prints it with its worst err / bar.

A. nk_plant_loop around the three built-in plants, the double integrator included: the ladder m = 1, 63, 64, 65, 255, 256, 257,
   1025, 4095, 4096 (one landmark per lane / four; one, two, five and sixteen waves; a partly filled last wave) on Duffing x
   Matern and HJB x RBF, every other (plant, family) pair at m = 64, 65, 257, the spline model also at 4096; distinct
   references and one shared reference (the C ABI takes one reference per trajectory; the binding repeats a shared one).  Per
   step: u_t under the bar, x_{t+1} = nk_plant_step(x_t, u_t) bit for bit, row 0 = x0 bit for bit, and a trajectory has the
   same bits alone and in the batch.
B. nk_poly_plant_loop: every compiled (D, P) class, the padded ones included (d = 1, d = 3, p = 3), at m = 64, 65, 64 lpt,
   64 lpt + 1 and the class limit; every input column, the same assertions, states replayed with nk_poly_plant_step.
C. the multi-model forms: all Duffing units of section A in one nk_plant_loop_multi call and all P2 units of section B in one
   nk_poly_plant_loop_multi call, in a shuffled order: states and controls are the bits of the single calls, and with
   out_x = out_u = NULL the scores are the bits of the call that stores the trajectories.
D. the lift and gradient pass of nk_mpc_loop with iters = 0 and no limits (W = S^-1 K', v = -g), m = 1, 64, 65, 128, 129 and
   nk_mpc_loop_max_m(p) for p = 1, 2, 4, against the same reference with the reduction term of mpc_w_pass.

Worst err / bar on an MI355X (profiles/plant_loop_steps.log; 110 passed in 13 s, none skipped; the bars were fixed before the
first device run and none was changed): A 0.20 at m = 1 (a bar is a few units in the last place), 0.012 at two waves, 2.9e-5 at
five, 2.6e-3 at sixteen (spline; 9.8e-6 for the Nystrom models); B 0.023 / 0.018 / 4.2e-3 at one / two / sixteen waves; D 0.22 at
m = 1, 2.6e-4 at eight waves; C bit for bit.  The ratios fall with m because the bars are worst-case sums over the landmarks;
every landmark still moves some control by more than twice its bar (the least visible one by 367 bars).  No defect was found."""
import types

import numpy as np
import pytest

import plant_loop_reference as P
from test_gpu_rollout_steps import model_sinv
from test_plant_loop_reference_host import plant_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not P.HAVE_LONGDOUBLE, reason=P.LONGDOUBLE_SKIP)]


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


@pytest.fixture(scope="module")
def models(nk):
    """models(fam, d, m, p) -> (regressor, S^-1 read back from its model or None for a spline), built once."""
    from nys_koop_lqr_amd import _lib
    cache = {}

    def get(fam, d, m, p):
        if (fam, d, m, p) not in cache:
            s = P.model_spec(fam, d, m)
            Zt = np.ascontiguousarray(s.Z.T)
            if s.family == P.SPLINE:
                reg = nk.KoopmanSplineRegressor(p, m=m, gamma=1e-6)
                reg.centers = Zt
                Sinv = None
            else:
                if s.family == P.LINEAR:
                    kern = nk.LinearKernelWrapper(s.par)
                elif s.family == P.MATERN:
                    kern = nk.KernelWrapper(np.asarray(s.par))
                else:
                    kern = types.SimpleNamespace(kernel=nk.kernels.DeviceKernel(_lib.NK_KERNEL_RBF, np.asarray(s.par)))
                reg = nk.KoopmanNystromRegressor(p, kernel=kern, gamma=1e-6, m=m)
                reg.nystrom_centers_output = Zt
                reg.jitter = s.jitter
                Sinv = model_sinv(reg)
                assert np.all(np.isfinite(Sinv))
            cache[(fam, d, m, p)] = (reg, Sinv)
        return cache[(fam, d, m, p)]
    return get


@pytest.fixture(scope="module")
def problems(models):
    """problems(c) -> (regressor, designed problem around the model's own S^-1), the longdouble fold computed once."""
    cache = {}

    def get(c):
        if c not in cache:
            reg, Sinv = models(c.fam, c.d, c.m, c.p)
            cache[c] = (reg, P.problem(c, Sinv))
        return cache[c]
    return get


def controller(K):
    """What closed_loop_plant_mpc reads of a controller, for iters = 0 without limits: the gain; H and F are not used."""
    p, m = K.shape
    inf = np.full(p, np.inf)
    return types.SimpleNamespace(K=K, F=np.zeros((p, m)), H=np.eye(p), horizon=1, lo=-inf, hi=inf, dlo=-inf, dhi=inf, rho=1.0)


def run_loop(c, reg, q, plant, x0, xref):
    if c.section == "D":
        return reg.closed_loop_plant_mpc(controller(q["K"]), x0, xref, P.STEPS, plant, iters=0)
    return reg.closed_loop_plant(q["K"], x0, xref, P.STEPS, plant)


def check_case(nk, problems, c, want_class=None):
    reg, q = problems(c)
    lpt, waves, cc = P.case_class(c)
    if want_class is not None:
        assert (lpt, waves) == want_class, (P.name(c), lpt, waves)
    assert (q["lpt"], q["waves"], q["c"]) == (lpt, waves, cc)
    plant = plant_of(nk, c)
    ratios, share = {}, None
    for tag, xref in (("distinct", q["xref"]), ("shared", q["xref"][0])):
        S, U = run_loop(c, reg, q, plant, q["x0"], xref)
        assert S.shape == (P.BATCH, P.STEPS + 1, c.d) and U.shape == (P.BATCH, P.STEPS, c.p)
        assert np.all(np.isfinite(S)) and np.all(np.isfinite(U)), (P.name(c), tag)
        assert np.array_equal(S[:, 0], q["x0"]), (P.name(c), tag)
        ref = P.control_reference(q["spec"], q["w"], q["F"], S[:, :-1], np.atleast_2d(xref), cc)
        r, at = P.worst(U, ref["u"], ref["bar"])
        ratios[tag] = r
        mine = np.max(ref["share"], axis=(0, 1))
        share = mine if share is None else np.maximum(share, mine)
        for b in range(P.BATCH):  # the plant step and the stores: bit for bit
            for t in range(P.STEPS):
                want = plant.step_library(S[b, t], U[b, t])
                assert np.array_equal(S[b, t + 1], want), (P.name(c), tag, b, t, S[b, t + 1], want)
        b = 5  # a trajectory has the same bits alone and in the batch
        S1, U1 = run_loop(c, reg, q, plant, q["x0"][b], xref if tag == "shared" else xref[b])
        assert np.array_equal(S1.T, S[b]) and np.array_equal(U1.T, U[b]), (P.name(c), tag)
        print(f"\n[plant-loop-steps] {c.section} {P.name(c)} {tag}: class lpt {lpt} waves {waves} c {cc}; worst err / bar "
              f"{r:.3e} at (trajectory, step, input) {at}")
        assert r <= 1.0, f"{P.name(c)} {tag}: err / bar = {r:.3e} at (trajectory, step, input) {at}"
    assert np.all(share > 2.0), (P.name(c), "landmarks hidden behind the bar", int(np.sum(share <= 2.0)))
    return ratios


# ---------------------------------------------------------------------------------------------------------------------
# A. built-in plants
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.A_CASES, ids=P.name)
def test_built_in_plants(nk, problems, c):
    ladder = (c.plant, c.fam) in P.LADDER_PAIRS
    check_case(nk, problems, c, P.LADDER_CLASS[c.m] if ladder else {64: (1, 1), 65: (4, 1), 257: (4, 2), 4096: (4, 16)}[c.m])


# ---------------------------------------------------------------------------------------------------------------------
# B. polynomial plants
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.B_CASES, ids=P.name)
def test_polynomial_plants(nk, problems, c):
    lpt = P.poly_lpt(P.poly_pad_d(c.d), P.poly_pad_p(c.p))
    want = (1, 1) if c.m <= 64 else (lpt, -(-c.m // (64 * lpt)))
    if c.m == P.poly_loop_max_m(c.d, c.p):
        assert want == (lpt, 16)
    check_case(nk, problems, c, want)


# ---------------------------------------------------------------------------------------------------------------------
# C. the multi-model forms
# ---------------------------------------------------------------------------------------------------------------------
def _multi(nk, problems, cases, per_case, seed):
    """(units in a shuffled order as (case, regressor, problem, trajectory), their single calls)."""
    units = []
    for c in cases:
        reg, q = problems(c)
        units += [(c, reg, q, (3 + 5 * k) % P.BATCH) for k in range(per_case)]
    order = np.random.default_rng(seed).permutation(len(units))
    units = [units[i] for i in order]
    plant = plant_of(nk, cases[0])
    alone = [u[1].closed_loop_plant(u[2]["K"], u[2]["x0"][u[3]], u[2]["xref"][u[3]], P.STEPS, plant) for u in units]
    return units, plant, alone


def _check_multi(call, units, alone, p):
    args = ([u[1]._ensure_model() for u in units], [u[2]["K"] for u in units], np.stack([u[2]["x0"][u[3]] for u in units]),
            np.stack([u[2]["xref"][u[3]] for u in units]))
    sc, ox, ou = call(*args, want_x=True, want_u=True)
    n = len(units)
    assert ox.shape[:2] == (n, P.STEPS + 1) and sc.shape == (n, 4) and np.all(np.isfinite(sc))
    ou = ou.reshape(n, P.STEPS, p)
    for i, (S1, U1) in enumerate(alone):
        assert np.array_equal(ox[i], S1.T) and np.array_equal(ou[i], U1.T), (i, P.name(units[i][0]))
    sc2, ox2, ou2 = call(*args)
    assert ox2 is None and ou2 is None and np.array_equal(sc2, sc)
    return n, sorted({P.case_class(u[0])[:2] for u in units})


def test_multi_form_built_in(nk, problems):
    cases = [c for c in P.A_CASES if c.plant == "duffing"]
    units, plant, alone = _multi(nk, problems, cases, 1, 41)
    ctx = nk.get_context()
    n, classes = _check_multi(lambda *a, **kw: ctx.plant_loop_multi(plant.plant_id, plant.Ts, P.STEPS, *a, **kw), units, alone, 1)
    assert {(1, 1), (4, 1), (4, 2), (4, 5), (4, 16)} <= set(classes)
    print(f"\n[plant-loop-steps] C nk_plant_loop_multi: {n} units, classes (lpt, waves) {classes}: the bits of the single calls; "
          "scores without trajectories: the same bits")


def test_multi_form_polynomial(nk, problems):
    cases = [c for c in P.B_CASES if c.plant == "P2"]
    units, plant, alone = _multi(nk, problems, cases, 2, 43)
    ctx = nk.get_context()
    n, classes = _check_multi(lambda *a, **kw: ctx.poly_plant_loop_multi(plant.descriptor(), P.STEPS, *a, **kw), units, alone, 2)
    assert {(1, 1), (4, 1), (4, 2), (4, 16)} <= set(classes)
    print(f"\n[plant-loop-steps] C nk_poly_plant_loop_multi: {n} units, classes (lpt, waves) {classes}: the bits of the single "
          "calls; scores without trajectories: the same bits")


# ---------------------------------------------------------------------------------------------------------------------
# D. the lift and gradient pass of the MPC loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.D_CASES, ids=P.name)
def test_mpc_lift_and_gradient_pass(nk, problems, c):
    from nys_koop_lqr_amd import _lib
    assert c.m <= _lib.load_library().nk_mpc_loop_max_m(c.p)
    check_case(nk, problems, c, (1, -(-c.m // 64)))
