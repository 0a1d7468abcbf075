"""The matrix square root (nk_sqrtm_spd, and the S / S^-1 of a Nystrom fit) on every route against an extended-precision
reference (tests/sqrtm_reference.py): the host-checked polar iteration on the generic engine (m < 128 or odd m, m = 1025
included) and on the LDS-DMA engine (even m, 128 .. 1022), the queued iteration (even m >= 1024), the early-queued form of a
fit, and the coupled Newton-Schulz fallback through NYSKOOP_SQRT_FORCE_COUPLED=1.

Measures (longdouble): resid ||S S - P||_F / ||P||_F, whiten ||S^-1 P S^-1 - I||_F / sqrt(m), inv ||S S^-1 - I||_F / sqrt(m),
asym ||S - S^T||_F / ||S||_F and, where the full longdouble reference exists (m <= 400), fwd_S, fwd_Sinv, max_S, max_Sinv.  At
m >= 1024 resid / whiten / inv are formed in fp64 BLAS over the whole matrix and resid / inv in longdouble on a fixed row set.

Two bars, kept apart:
  cap  -- derived: fwd_S <= m eps sqrt(kappa_2(P)), fwd_Sinv <= m eps kappa_2(P).  test_sqrtm_reference_host.py holds the
          comparison solver to half of it on the CPU first.
  bar  -- from the reference alone: 2 x the worst value of the same algorithm in fp64 NumPy (numpy_polar / numpy_coupled) over
          the matrix and 4 seeded symmetric permutations of it, then floored at eps (forward, asym) or m eps (residuals).

Thresholds looked at for the scaling test (P 4^k): `c > 0`, the pivot test `d_kk > 0`, the stop at a residual of 1e-7 of
M = X^T X and the schedule's 0.5 / 1 +- 1e-9 are all taken on quantities that do not change with the scale of P (M_0 = P / c,
sqrt(sumsq) / c, trace / c, 0.5 / (c ||L^-1||_F^2)), and a scaling by 4^k is exact in every product.  One is not relative:
the verdict whether a diagonal block's inverse needs the correction step compares ||L_jj||_F ||L_jj^-1||_F, taken over the
64 x 64 tile WITH the identity that pads a short last block, against CHOL_FIX_KAPPA.  The padding can only raise the
figure (the correction runs where it is not needed, never the reverse), so it is intended; at m = 258 (a last block of 2
rows) the scaled runs therefore need not give the unscaled bits and are held to the bars, at m = 1024 (no padding) the
bits are asserted.

Measured on one MI355X (profiles/sqrtm_accuracy.log).  Step counts: the device's equal numpy_polar's / numpy_coupled's in every
case (5 .. 32; queued 22 / 8 / 29, so both parity buffers are taken; early form 23 where nk_sqrtm_spd on the same matrix
takes 22).  Device value / NumPy value, device value / bar:
  host-checked, both engines (14 cases)  resid 0.20 .. 1.01   whiten 0.74 .. 1.21   inv 0.60 .. 1.11   fwd_S 0.24 .. 1.11
                                         fwd_Sinv 0.76 .. 1.19   max_S 0.22 .. 1.84   max_Sinv 0.33 .. 1.11; at most 0.57 of a bar
  queued (3 cases)                       resid 1.26 .. 1.43   whiten 0.71 .. 1.02   inv 0.70 .. 1.01   asym 1.28 .. 1.50; at most
                                         0.74 of a bar (asym), 0.36 otherwise
  early-queued / synchronous fit         0.66 .. 1.52 (resid_rows of the early form; its bar is the m eps floor), at most 0.40 of a bar
  asymmetric input                       0.73 .. 2.55 (max_Sinv), at most 0.82 of a bar
No forward error is above 2e-4 of its cap.  Scaling by 4^+-20 returns the unscaled bits at m = 1024 and not at m = 258, as
derived above.  The coupled iteration was the finding: before M was averaged with its transpose in sqrtm_spd_coupled (its
128 x 128 diagonal tiles were symmetric only up to rounding while Z <- T Z is issued as T^T Z) the device stood at up to
7.7 x NumPy on whiten, 3.9 x on asym and 3.6 x on fwd_S at (258, rbf) and was over a bar in three of the four cases;
numpy_coupled with that defect planted gives the same figures to 10 %.  numpy_coupled symmetrises M as the device now does."""
import ctypes as C
import os

import numpy as np
import pytest

import sqrtm_reference as sr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not sr.HAVE_LONGDOUBLE, reason=sr.LONGDOUBLE_SKIP)]

HOOK = "NYSKOOP_SQRT_FORCE_COUPLED"


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    return nk


@pytest.fixture(scope="module")
def ctx(nk):
    return nk.get_context()


def _log(line):
    print(line)
    path = os.environ.get("NYSKOOP_SQRTM_ACC_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _grade(tag, P, S, Sinv, vals, bars, caps, ref=None, rows=None, only=None):
    """one log line per measure, then every measure under its bar and under its cap"""
    assert np.isfinite(S).all() and np.isfinite(Sinv).all(), f"{tag}: NaN / inf in the output"
    got = sr.measures(S, Sinv, P, ref) if rows is None else sr.measures_large(S, Sinv, P, rows)
    names = [k for k in got if only is None or k in only]
    for k in names:
        ref_vals = [v[k] for v in vals]
        cap = f"{caps[k]:.3e}" if k in caps else "-"
        _log(f"{tag} {k}: gpu {got[k]:.3e} numpy {ref_vals[0]:.3e} (perms {min(ref_vals):.3e}..{max(ref_vals):.3e}) "
             f"bar {bars[k]:.3e} cap {cap}")
    over = {k: (got[k], bars[k]) for k in names if not got[k] <= bars[k]}
    over_cap = {k: (got[k], caps[k]) for k in names if k in caps and not got[k] <= caps[k]}
    assert not over and not over_cap, (tag, "over bar", over, "over cap", over_cap)
    return got


def _run_case(ctx, m, family, ld, route):
    seed = sr.seed_of(m)
    c = sr.case(family, m, seed, route)
    S, Sinv, iters, resid = sr.sqrtm(ctx, c.P, ld)
    tag = f"{route} m={m} ld={ld} {family}"
    _log(f"{tag} iters: gpu {iters} numpy {c.steps[0]} (perms {min(c.steps)}..{max(c.steps)}) residual {resid:.3e}")
    assert resid < 1e-7
    # a residual at the 1e-7 threshold may flip one step; a wrong scale coefficient moves the count by more
    assert abs(iters - c.steps[0]) <= 1, (iters, c.steps)
    _grade(tag, c.P, S, Sinv, c.vals, c.bars, c.caps, c.ref, c.rows)
    return iters


@pytest.mark.parametrize("m,family,ld", sr.GENERIC)
def test_generic_engine_host_checked(ctx, m, family, ld):
    _run_case(ctx, m, family, ld, "host")


@pytest.mark.parametrize("m,family,ld", sr.LDS_DMA)
def test_lds_dma_engine_host_checked(ctx, m, family, ld):
    _run_case(ctx, m, family, ld, "host")


QUEUED_ITERS = {}


@pytest.mark.parametrize("m,family,ld", sr.QUEUED)
def test_queued(ctx, m, family, ld):
    QUEUED_ITERS[m] = _run_case(ctx, m, family, ld, "queued")


def test_queued_cases_took_both_parities(ctx):
    """The converged iterate lives in Xa after an odd and in Xb after an even number of steps, and the device picks: rbf 1024
    (22 steps) and random 1026 (8) end in Xb, graded 1152 (29) in Xa."""
    for m, family, ld in sr.QUEUED:
        if m not in QUEUED_ITERS:  # run alone: the cases' own test did not come first
            QUEUED_ITERS[m] = sr.sqrtm(ctx, sr.matrix(family, m, m), ld)[2]
    assert {it % 2 for it in QUEUED_ITERS.values()} == {0, 1}, QUEUED_ITERS


@pytest.mark.parametrize("m,family,ld", sr.LARGE_ODD)
def test_large_odd_size_is_host_checked_on_the_generic_engine(ctx, m, family, ld):
    _run_case(ctx, m, family, ld, "host")


# ---------------------------------------------------------------------------------------------------------------------
# the coupled iteration
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,family", sr.COUPLED)
def test_coupled_route(ctx, monkeypatch, m, family):
    """kappa_2 <= 1e6 here: the coupled iteration is not expected to converge at 1e10."""
    c = sr.case(family, m, m, "coupled")
    polar = sr.sqrtm(ctx, c.P)
    monkeypatch.setenv(HOOK, "1")
    S, Sinv, iters, resid = sr.sqrtm(ctx, c.P)
    monkeypatch.delenv(HOOK)
    again = sr.sqrtm(ctx, c.P)
    tag = f"coupled m={m} {family}"
    differs = not np.array_equal(S, polar[0])
    _log(f"{tag} iters: gpu {iters} numpy {c.steps[0]} (perms {min(c.steps)}..{max(c.steps)}) residual {resid:.3e}; "
         f"polar iters {polar[2]}, S bits differ from the polar run: {differs}")
    assert iters != polar[2] or differs  # the route was taken
    assert abs(iters - c.steps[0]) <= 1, (iters, c.steps)
    # the last looked-at residual: below 5e-14, or one quadratic step after a residual below 1e-7
    assert resid < 1e-7
    _grade(tag, c.P, S, Sinv, c.vals, c.bars, c.caps, c.ref)
    # unset again, the polar bits return
    assert again[2] == polar[2] and np.array_equal(again[0], polar[0]) and np.array_equal(again[1], polar[1])


def test_hook_values_other_than_one_change_nothing(ctx, monkeypatch):
    P = sr.matrix("rbf", 130, 130)
    polar = sr.sqrtm(ctx, P)
    for value in ("0", "", "2"):
        monkeypatch.setenv(HOOK, value)
        out = sr.sqrtm(ctx, P)
        assert out[2] == polar[2] and np.array_equal(out[0], polar[0]) and np.array_equal(out[1], polar[1]), value


# ---------------------------------------------------------------------------------------------------------------------
# the square root inside a fit
# ---------------------------------------------------------------------------------------------------------------------
FIT = dict(d=6, p=1, n=1280, ls=2.0, jitter=1e-6)


def _fit_case(nk, m, route, keep=None):
    X, Y, Z = sr.fit_data(m, FIT["d"], FIT["p"], FIT["n"], seed=m)
    c0 = sr.counters()
    S, Sinv, stats, P = sr.fit_sqrt(nk, Z, FIT["ls"], FIT["jitter"], X, Y, p=FIT["p"])
    c1 = sr.counters()
    assert c1[sr.CNT_SQRT_RETRY] == c0[sr.CNT_SQRT_RETRY] and c1[sr.CNT_CHOL_FLOW_GIVEUP] == c0[sr.CNT_CHOL_FLOW_GIVEUP]
    rows = sr.row_set(m, m)
    solver = (lambda A: sr.numpy_polar(A, "early", jitter=FIT["jitter"])) if route == "early" else sr.SOLVERS[route]
    vals, steps = sr.solver_values(P, solver, None, m, rows, keep)
    return S, Sinv, stats, P, rows, vals, steps


def test_early_queued_form_of_a_fit(nk):
    """m = 1024 with lambda_min_hint = jitter: the iteration is queued from the jitter bound before the factorisation's
    verdict.  Residual measures only: the fit's own K_mm may differ from nk_kernel_matrix's in the last bit, to which forward
    errors are sensitive (by kappa_2) and residuals are not.  The step count tells the early schedule from the ordinary
    queued one: on this matrix numpy_polar takes 23 steps from the jitter bound and 22 from 1 / ||L^-1||_F^2, and the fit
    has to take the former's."""
    m = 1024
    S, Sinv, stats, P, rows, vals, steps = _fit_case(nk, m, "early")
    tag = f"early m={m} fit"
    queued_steps = sr.numpy_polar(P, "queued").steps
    direct = sr.sqrtm(nk.get_context(), P)  # the queued route, scheduled from 1 / ||L^-1||_F^2 instead of the jitter
    _log(f"{tag} iters: gpu {stats['sqrt_iters']} numpy {steps[0]} (perms {min(steps)}..{max(steps)}) "
         f"residual {stats['sqrt_residual']:.3e}; queued schedule on the same matrix: gpu {direct[2]} numpy {queued_steps}")
    assert stats["sqrt_residual"] < 1e-7
    assert queued_steps != steps[0], "the matrix does not tell the two schedules apart: choose another"
    assert stats["sqrt_iters"] == steps[0] and direct[2] == queued_steps, (stats["sqrt_iters"], steps, direct[2], queued_steps)
    _grade(tag, P, S, Sinv, vals, sr.bars_from(vals, m), {}, None, rows, only=("resid", "whiten", "inv", "resid_rows", "inv_rows"))


def test_synchronous_form_of_a_fit_meets_the_direct_call(nk, ctx):
    """m = 1022, the largest even size below the queued iteration: the fit's S and nk_sqrtm_spd(P) are two runs of the
    host-checked route on matrices that agree to the last bit or so (the fit's own K_mm against nk_kernel_matrix's: equal
    bits cannot be shown from the code).  Their distance is held to twice the worst distance of numpy_polar's permuted runs
    from its unpermuted one (sqrtm_reference.distance_bars), and both to that case's bars."""
    m = 1022
    kept = []
    S, Sinv, stats, P, rows, vals, steps = _fit_case(nk, m, "host", kept)
    bars = sr.bars_from(vals, m)
    bar_S, bar_Sinv = sr.distance_bars(kept)
    D, Dinv, iters, resid = sr.sqrtm(ctx, P)
    dist_S = float(np.linalg.norm(S - D) / np.linalg.norm(D))
    dist_Sinv = float(np.linalg.norm(Sinv - Dinv) / np.linalg.norm(Dinv))
    _log(f"sync m={m} fit iters: fit {stats['sqrt_iters']} direct {iters} numpy {steps[0]}; "
         f"||S_fit - S_direct||_F / ||S_direct||_F {dist_S:.3e} bar {bar_S:.3e}; for S^-1 {dist_Sinv:.3e} bar {bar_Sinv:.3e}")
    assert abs(stats["sqrt_iters"] - steps[0]) <= 1 and abs(iters - steps[0]) <= 1
    assert dist_S <= bar_S and dist_Sinv <= bar_Sinv, (dist_S, bar_S, dist_Sinv, bar_Sinv)
    _grade(f"sync m={m} fit", P, S, Sinv, vals, bars, {}, None, rows)
    _grade(f"sync m={m} direct", P, D, Dinv, vals, bars, {}, None, rows)


# ---------------------------------------------------------------------------------------------------------------------
# scaling, asymmetry, device operands, refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,route,same_bits", [(258, "host", False), (1024, "queued", True)])
def test_scaling_by_powers_of_four(ctx, m, route, same_bits):
    """P 4^k gives S 2^k and S^-1 2^-k within the unscaled case's bars; see the module docstring for the thresholds."""
    c = sr.case("rbf", m, m, route)
    base = sr.sqrtm(ctx, c.P)
    for k in (-20, 20):
        S, Sinv, iters, resid = sr.sqrtm(ctx, c.P * 4.0 ** k)
        S, Sinv = S * 2.0 ** -k, Sinv * 2.0 ** k  # exact
        equal = np.array_equal(S, base[0]) and np.array_equal(Sinv, base[1])
        _log(f"scaled m={m} k={k}: iters {iters} (unscaled {base[2]}), the unscaled bits: {equal}")
        assert abs(iters - base[2]) <= 1
        _grade(f"scaled m={m} k={k}", c.P, S, Sinv, c.vals, c.bars, c.caps, c.ref, c.rows)
        if same_bits:
            assert iters == base[2] and equal


def test_slightly_asymmetric_input(ctx):
    """P + E, E strictly upper triangular with |E_ij| <= 4 eps |P_ij|: the first M averages P and P^T, so the result is graded
    as a square root of P + E / 2 + E^T / 2."""
    m = 258
    P = sr.matrix("rbf", m, m)
    rng = np.random.default_rng(99)
    E = np.triu(rng.uniform(-4.0, 4.0, (m, m)) * sr.EPS * P, 1)
    assert np.abs(E).max() > 0 and (np.abs(E) <= 4 * sr.EPS * np.abs(P)).all()
    Psym = P + E / 2 + E.T / 2
    assert np.array_equal(Psym, Psym.T)
    ref = sr.sqrt_ld(Psym)
    vals, steps = sr.solver_values(Psym, sr.SOLVERS["host"], ref, m)
    S, Sinv, iters, resid = sr.sqrtm(ctx, P + E)
    assert abs(iters - steps[0]) <= 1 and resid < 1e-7
    _grade(f"asymmetric m={m}", Psym, S, Sinv, vals, sr.bars_from(vals, m), sr.caps(m, sr.kappa2(Psym)), ref)


def test_device_resident_operands(ctx):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch does not see the device")
    m = 258
    P = sr.matrix("rbf", m, m)
    host = sr.sqrtm(ctx, P)
    dev = torch.device("cuda", ctx.device)
    Pd = torch.from_numpy(np.array(P)).to(dev)
    Sd = torch.full((m, m), float("nan"), dtype=torch.float64, device=dev)
    Sid = torch.full((m, m), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    it, res = C.c_int32(-1), C.c_double(np.nan)
    rc = ctx.lib.nk_sqrtm_spd(ctx.handle, Pd.data_ptr(), m, m, Sd.data_ptr(), Sid.data_ptr(), C.byref(it), C.byref(res))
    torch.cuda.synchronize(dev)
    assert rc == 0 and it.value == host[2] and res.value == host[3]
    assert np.array_equal(Sd.cpu().numpy(), host[0]) and np.array_equal(Sid.cpu().numpy(), host[1])


def test_clean_refusals(ctx):
    """m = 192 (below the size that takes the dataflow launch): -I and a NaN entry are refused with a message, the context
    stays usable, and bad shapes are bad arguments."""
    m = 192
    P = sr.matrix("random", m, m)
    good = sr.sqrtm(ctx, P)
    with_nan = np.array(P)
    with_nan[17, 40] = with_nan[40, 17] = np.nan
    for name, bad in (("-I", -np.eye(m)), ("NaN entry", with_nan)):
        rc = sr.sqrtm_raw(ctx, bad)[0]
        msg = ctx.lib.nk_last_error()
        _log(f"refusal m={m} {name}: rc {rc} message {msg!r}")
        assert rc in (sr.NK_ERR_NOT_SPD, sr.NK_ERR_NO_CONVERGENCE) and msg
        again = sr.sqrtm(ctx, P)
        assert again[2] == good[2] and np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
    assert sr.sqrtm_raw(ctx, P, ld=m - 1)[0] == sr.NK_ERR_BAD_ARG
    assert sr.sqrtm_raw(ctx, P, m=0)[0] == sr.NK_ERR_BAD_ARG
