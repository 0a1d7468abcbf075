"""tests/sqrtm_reference.py without a GPU: the longdouble square root is held to its own residuals, to a closed form and to a
second, independent build of itself; the Python ports of the step schedule are compared number for number with the printout of
csrc/nk_sqrt_schedule.h (the stand-alone program of test_sqrt_schedule_host.py); the comparison solvers are held to the derived
caps with the factor-of-two room the GPU test's bar gives; and four errors of the kind the device code could make are planted
in numpy_polar's output, each of which has to put a measure over its bar.

Which measure catches which planted error (random family, m = 258, kappa_2 = 31):
  the iterate one step before the converged one ......... every residual and forward measure (1e-9 .. 1e-8 against 1e-14 .. 1e-13)
  a 128 x 128 tile of Q^T X_0 contracted one index short . resid, inv, asym, fwd_S, max_S (1e-2); S^-1 is not touched
  a 64 x 64 tile of Q used untransposed .................. every measure (1e-1)
  one entry of S^-1 off by 64 eps max|S^-1| .............. max_Sinv alone (1.5e-14 against a bar of 1.1e-14): every norm-wise
      measure averages one entry away.  On the rbf and graded families (kappa_2 = 1e6, 1e10) the iteration's own forward error
      of S^-1 is 1e-12 / 4e-8, and an error of 64 eps lies below it for every measure: that error is planted where it can show."""
import math
import subprocess

import numpy as np
import pytest

import sqrtm_reference as sr
from test_sqrt_schedule_host import LAM_MINS, cases, schedule_program, schedules, spectrum  # noqa: F401

pytestmark = pytest.mark.skipif(not sr.HAVE_LONGDOUBLE, reason=sr.LONGDOUBLE_SKIP)

RESIDUALS = ("resid", "whiten", "inv")
S_ONLY = ("resid", "asym", "fwd_S", "max_S")


# ---------------------------------------------------------------------------------------------------------------------
# the longdouble reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [130, 257])
@pytest.mark.parametrize("family", ["random", "rbf", "graded"])
def test_reference_is_a_thousand_times_better_than_any_solver(family, m):
    """Residuals of the reference, and its distance from a second build that starts from another eigenbasis (the matrix
    permuted), against the smallest value any comparison solver reaches.  scipy.linalg.sqrtm returns no inverse: it is a
    comparison for the measures of S."""
    P = sr.matrix(family, m, m)
    ref = sr.reference(family, m, m)
    perm = np.random.default_rng(m).permutation(m)
    inv_perm = np.argsort(perm)
    again = sr.permuted(sr.sqrt_ld(np.ascontiguousarray(P[perm][:, perm])), inv_perm)
    own = sr.measures(ref[0], ref[1], P, again)
    solvers = {"host": sr.numpy_polar(P, "host"), "queued": sr.numpy_polar(P, "queued"), "eigh": sr.eigh_sqrt(P),
               "scipy": sr.scipy_sqrt(P)}
    try:
        solvers["coupled"] = sr.numpy_coupled(P)
    except RuntimeError:
        pass
    vals = {name: sr.measures(o.S, o.Sinv, P, ref) for name, o in solvers.items()}
    assert own["resid"] < 1e-17, own
    for name in RESIDUALS + sr.FORWARD:
        best = min(v[name] for s, v in vals.items() if s != "scipy" or name in S_ONLY)
        print(f"{family} {m} {name}: reference {own[name]:.2e}, best solver {best:.2e}, ratio {best / max(own[name], 1e-300):.0f}")
        assert own[name] * 1000.0 <= best, (name, own[name], best)


def test_reference_on_a_closed_form():
    """P = B B for an integer symmetric positive definite B: P is exact in fp64 and its square root is B."""
    B = np.array([[9, 1, 0, 2, 0, 1], [1, 8, 1, 0, 2, 0], [0, 1, 7, 1, 0, 2], [2, 0, 1, 6, 1, 0], [0, 2, 0, 1, 5, 1],
                  [1, 0, 2, 0, 1, 4]], dtype=np.float64)
    assert np.array_equal(B, B.T) and np.linalg.eigvalsh(B).min() > 1.0
    P = B @ B
    S, Si = sr.sqrt_ld(P)
    assert float(np.abs(S - B.astype(sr.LD)).max()) < 1e-17 * 9
    assert float(np.abs(Si @ B.astype(sr.LD) - np.eye(6)).max()) < 1e-17
    own = sr.measures(S, Si, P, (B.astype(sr.LD), Si))
    for o in (sr.numpy_polar(P), sr.numpy_coupled(P), sr.eigh_sqrt(P), sr.scipy_sqrt(P)):
        v = sr.measures(o.S, o.Sinv, P, (S, Si))
        assert v["fwd_S"] < 64 * sr.EPS and v["fwd_Sinv"] < 64 * sr.EPS, v
    assert max(own["resid"], own["whiten"], own["inv"], own["fwd_S"]) < 1e-18, own


# ---------------------------------------------------------------------------------------------------------------------
# the ports of csrc/nk_sqrt_schedule.h
# ---------------------------------------------------------------------------------------------------------------------
def test_schedule_port_equals_the_header_number_for_number(schedules):
    assert len(schedules) == 96
    for (_, a, lower), (kmax, s2, check) in schedules.items():
        mine = sr.ns_queued_schedule(a, lower)
        assert mine[0] == kmax and mine[2] == check, (a, lower, mine[0], kmax)
        assert mine[1] == s2, (a, lower)  # floats read back from hexadecimal: equal means the same bits


def _program(schedule_program, mode, text):
    res = subprocess.run([schedule_program.exe, mode], input=text, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-3000:])
    return res.stdout.splitlines()


def test_interval_estimate_port_equals_the_header(schedule_program):
    """ns_interval_estimate on that test's spectra and on inputs that reach each of its guards"""
    inputs = []
    for lam_min in LAM_MINS:
        lam = spectrum(lam_min)
        inputs.append((math.sqrt(float(np.sum(lam * lam))), float(np.sum(lam)), lam.size))
    inputs += [(1.0, 1.0, 1), (0.0, 0.0, 5), (0.5, 40.0, 3), (float("nan"), float("nan"), 3), (0.3, 0.2, 7), (2.5, 3.0, 2)]
    lines = _program(schedule_program, "estimate", "".join(f"{f!r} {t!r} {m}\n" for f, t, m in inputs))
    assert len(lines) == len(inputs)
    for (f, t, m), line in zip(inputs, lines):
        assert sr.ns_interval_estimate(f, t, m) == float.fromhex(line), (f, t, m)


def test_host_recurrence_port_equals_the_header(schedule_program):
    """ns_scale / ns_advance as the host-checked route calls them, with the upper end b carried from step to step"""
    starts = sorted({a for _, a, _ in cases()})
    lines = _program(schedule_program, "host", "".join(f"{a!r} 60\n" for a in starts))
    assert len(lines) == len(starts)
    for a0, line in zip(starts, lines):
        a, b = a0, 1.0
        for k, tok in enumerate(line.split()):
            s2 = sr.ns_scale(a, b)
            assert s2 == float.fromhex(tok), (a0, k)
            a, b = sr.ns_advance(s2, a, b)


# ---------------------------------------------------------------------------------------------------------------------
# the comparison solvers against the caps
# ---------------------------------------------------------------------------------------------------------------------
def _rel(A, B):
    return float(np.linalg.norm(A - B) / np.linalg.norm(B))


FULL = [(m, f) for m, f, _ in sr.GENERIC + sr.LDS_DMA if m <= sr.FULL_REFERENCE_MAX_M]


@pytest.mark.parametrize("m,family", FULL)
def test_numpy_polar_is_under_half_the_caps(m, family):
    """Every GPU case that has the full reference: fwd_S <= m eps sqrt(kappa_2) / 2 and fwd_Sinv <= m eps kappa_2 / 2 for both
    step schedules, and the same distance from the eigh and the scipy square roots."""
    seed = sr.seed_of(m)
    P, ref = sr.matrix(family, m, seed), sr.reference(family, m, seed)
    caps = sr.caps(m, sr.kappa2(P))
    e, s = sr.eigh_sqrt(P), sr.scipy_sqrt(P)
    for route in ("host", "queued") if m >= 128 else ("host",):  # (below 128 there is no LDS-DMA engine to queue on)
        o = sr.numpy_polar(P, route)
        v = sr.measures(o.S, o.Sinv, P, ref)
        print(f"{family} {m} {route}: steps {o.steps} fwd_S {v['fwd_S']:.2e} (cap {caps['fwd_S']:.2e}) "
              f"fwd_Sinv {v['fwd_Sinv']:.2e} (cap {caps['fwd_Sinv']:.2e})")
        assert o.resid < 1e-7 and 1 <= o.steps < 60
        assert v["fwd_S"] <= caps["fwd_S"] / 2 and v["fwd_Sinv"] <= caps["fwd_Sinv"] / 2, (v, caps)
        assert _rel(o.S, e.S) <= caps["fwd_S"] and _rel(o.S, s.S) <= caps["fwd_S"]
        assert _rel(o.Sinv, e.Sinv) <= caps["fwd_Sinv"] and _rel(o.Sinv, s.Sinv) <= caps["fwd_Sinv"]


@pytest.mark.parametrize("m,family", sr.COUPLED)
def test_numpy_coupled_is_under_half_the_caps(m, family):
    P, ref = sr.matrix(family, m, m), sr.reference(family, m, m)
    caps = sr.caps(m, sr.kappa2(P))
    o, e, s = sr.numpy_coupled(P), sr.eigh_sqrt(P), sr.scipy_sqrt(P)
    v = sr.measures(o.S, o.Sinv, P, ref)
    print(f"{family} {m} coupled: steps {o.steps} fwd_S {v['fwd_S']:.2e} (cap {caps['fwd_S']:.2e}) "
          f"fwd_Sinv {v['fwd_Sinv']:.2e} (cap {caps['fwd_Sinv']:.2e})")
    assert v["fwd_S"] <= caps["fwd_S"] / 2 and v["fwd_Sinv"] <= caps["fwd_Sinv"] / 2, (v, caps)
    assert _rel(o.S, e.S) <= caps["fwd_S"] and _rel(o.S, s.S) <= caps["fwd_S"]
    assert _rel(o.Sinv, e.Sinv) <= caps["fwd_Sinv"] and _rel(o.Sinv, s.Sinv) <= caps["fwd_Sinv"]


def test_early_schedule_converges_like_the_queued_one():
    """the early form's bound (0.9 jitter / c) is a lower bound like the other: same square root within the caps"""
    P = sr.matrix("rbf", 258, 258)
    caps = sr.caps(258, sr.kappa2(P))
    q, e = sr.numpy_polar(P, "queued"), sr.numpy_polar(P, "early", jitter=1e-6)
    assert abs(q.steps - e.steps) <= 3
    assert _rel(e.S, q.S) <= caps["fwd_S"] and _rel(e.Sinv, q.Sinv) <= caps["fwd_Sinv"]


# ---------------------------------------------------------------------------------------------------------------------
# planted errors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    c = sr.case("random", 258, 258, "host")
    return c, sr.numpy_polar(c.P, "host")


def _over(c, S, Sinv):
    v = sr.measures(S, Sinv, c.P, c.ref)
    over = {k: v[k] for k in v if v[k] > c.bars[k]}
    print({k: f"{v[k]:.2e} / {c.bars[k]:.2e}" for k in v})
    return over


def test_unplanted_output_is_under_every_bar(planted):
    c, o = planted
    assert not _over(c, o.S, o.Sinv)


def test_planted_previous_iterate(planted):
    """the wrong parity buffer of the queued route: X_{j-1} in place of X_j"""
    c, o = planted
    over = _over(c, math.sqrt(o.c) * (o.Q_prev.T @ o.X0), o.Linv.T @ o.Q_prev)
    assert {"resid", "whiten", "inv", "fwd_S", "fwd_Sinv"} <= set(over)


def test_planted_short_contraction(planted):
    """tile (0, 1) of S = sqrt(c) Q^T X_0: X_0 is upper triangular, so the contraction is trimmed to k < 256; cut at k < 255"""
    c, o = planted
    S = o.S.copy()
    S[0:128, 128:256] = math.sqrt(o.c) * (o.Q[:255, 0:128].T @ o.X0[:255, 128:256])
    over = _over(c, S, o.Sinv)
    assert {"resid", "inv", "asym", "fwd_S", "max_S"} <= set(over)


def test_planted_untransposed_tile(planted):
    c, o = planted
    Q = o.Q.copy()
    Q[64:128, 128:192] = o.Q[64:128, 128:192].T
    over = _over(c, math.sqrt(o.c) * (Q.T @ o.X0), o.Linv.T @ Q)
    assert set(over) == set(c.bars)


@pytest.mark.parametrize("i,j", [(5, 200), (100, 100)])
def test_planted_single_entry_of_the_inverse(planted, i, j):
    c, o = planted
    Sinv = o.Sinv.copy()
    Sinv[i, j] += 64 * sr.EPS * np.abs(Sinv).max()
    over = _over(c, o.S, Sinv)
    assert "max_Sinv" in over
