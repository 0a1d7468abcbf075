"""CPU checks of tests/fit_tail_reference.py, the reference tests/test_gpu_fit_tail.py grades the tail of a Nystrom fit with:
the longdouble tail agrees with the oracle's fit and is consistent with itself, every planted fault of the comparison solver
stands at least 100 x above the bar of the block it touches on every shape it applies to, the packed layout round-trips at an
odd and an even first block, the refinement's systems have the conditioning the GPU test asks for, and a NumPy emulation of the
refinement meets the refined operators' bar (so the bar is one fp64 code can meet)."""
import numpy as np
import pytest

import fit_tail_reference as T
import gram_reference as R
from chol_reference import LD, LD_EPS
from sqrtm_reference import _fro, _mm

pytestmark = pytest.mark.skipif(not T.HAVE_LONGDOUBLE, reason=T.LONGDOUBLE_SKIP)

FAULT_FACTOR = 100.0


def _bar_of(block, bar, p):
    # the last column of W is an input column when there are inputs, a state column otherwise
    return bar[("W_input" if p else "W_state") if block == "W_last" else block]


@pytest.mark.parametrize("name", T.DEFAULT_CASES)
def test_every_fault_stands_100_bars_above_its_block(name):
    c, v, key = T.CASES[name], T.inputs(name), T.variant(name)
    S, Si = T.sqrt_f64(name)
    ref, bar = T.reference(key), T.bars(key)
    applicable = T.faults_of(c)
    assert len(applicable) >= 6 and set(applicable) <= set(T.FAULTS)
    seen = {}
    for fault in applicable:
        got = T.tail_f64(v.G, v.K_mm, v.K_in, v.K_xo, c.n, c.gamma, c.jitter, S, Si, not c.sep, fault=fault)
        block = T.FAULTS[fault]
        seen[fault] = T.distances(got, ref, extra=("W_last",))[block] / _bar_of(block, bar, c.p)
    print(f"fit-tail: {name}: faults / bar: " + ", ".join(f"{k} {x:.3g}" for k, x in seen.items()))
    assert min(seen.values()) >= FAULT_FACTOR, seen
    # and the comparison solver without a fault is inside the bar it defines, and inside the derived cap
    clean = T.tail_f64(v.G, v.K_mm, v.K_in, v.K_xo, c.n, c.gamma, c.jitter, S, Si, not c.sep)
    dist, cap = T.distances(clean, ref), T.caps(key)
    assert all(dist[b] <= bar[b] / T.MARGIN for b in dist), (dist, bar)
    assert all(dist[b] <= cap[b] for b in dist), (dist, cap)


def test_every_fault_applies_somewhere():
    assert {f for name in T.DEFAULT_CASES for f in T.faults_of(T.CASES[name])} == set(T.FAULTS)


@pytest.mark.parametrize("name", T.DEFAULT_CASES)
def test_tail_ld_is_consistent_with_itself(name):
    """V inner - G2, Y inner_rec - G4 and S S - K_j at the longdouble level (own square root: sqrt_ld)."""
    c, v = T.CASES[name], T.inputs(name)
    t = T.tail_ld(v.G, v.K_mm, v.K_in, v.K_xo, c.n, c.gamma, c.jitter)
    G2, G4 = v.G["G2"].astype(LD), v.G["G4"].astype(LD)
    # a residual formed in longdouble resolves (order of the system) x LD_EPS of |X| |P|
    r1 = float(_fro(_mm(t.V, t.inner) - G2) / (_fro(t.V) * _fro(t.inner)))
    r2 = float(_fro(_mm(t.Y, t.inner_rec) - G4) / (_fro(t.Y) * _fro(t.inner_rec)))
    Kj = (v.K_mm + c.jitter * np.eye(c.m)).astype(LD)  # the fp64 sum: the matrix whose root is taken, on the device as here
    r3 = float(_fro(_mm(t.S, t.S) - Kj) / _fro(Kj))
    r4 = float(_fro(_mm(t.S, t.Sinv) - np.eye(c.m, dtype=LD)) / np.sqrt(c.m))
    print(f"fit-tail: {name}: longdouble residuals / LD_EPS: V {r1 / LD_EPS:.2f}, Y {r2 / LD_EPS:.2f}, S S {r3 / LD_EPS:.2f}, "
          f"S S^-1 {r4 / LD_EPS:.2f}")
    assert r1 <= (c.m + c.p) * LD_EPS and r2 <= c.m * LD_EPS and r3 <= c.m * LD_EPS
    assert r4 <= c.m * LD_EPS * float(_fro(t.S) * _fro(t.Sinv)) / c.m
    assert np.array_equal(t.W, _mm(t.C, np.hstack([t.A, t.B])))


def test_tail_ld_agrees_with_the_oracle_fit():
    """The oracle's fit (fp64 NumPy / LAPACK, its Cholesky form) from the rows themselves, against tail_ld from the longdouble
    accumulators: separate, anisotropic landmarks, so the orientation of K_xo and the second landmark pair are part of it.
    Tolerance: the oracle's own, 1e-6 relative Frobenius (test_fit_variants_vs_oracle)."""
    from oracle import nk_oracle as O
    name = "n2100_d7_m65_p6_aniso_sep"
    c, v = T.CASES[name], T.inputs(name)
    ls = np.asarray(v.kernel[1])
    ref = O.KoopmanNystromOracle(c.p, kernel=O._K(lambda A, B: O.rbf_kernel(A, B, ls)), gamma=c.gamma, m=c.m, faithful=False)
    ref.jitter = c.jitter
    ref.nystrom_centers_output = np.ascontiguousarray(v.Zout.T)
    ref.nystrom_centers_input = np.ascontiguousarray(v.Zin.T)
    ref.fit(v.X, v.Y)
    t = T.tail_ld(v.G, v.K_mm, v.K_in, v.K_xo, c.n, c.gamma, c.jitter)
    rel = lambda a, b: float(np.linalg.norm(a - b.astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))
    errs = dict(A=rel(ref.A, t.A), B=rel(ref.B, t.B), C=rel(ref.C, t.C), W=rel(ref.weights, t.W))
    print("fit-tail: oracle fit against tail_ld:", {k: f"{x:.2e}" for k, x in errs.items()})
    assert max(errs.values()) < 1e-6, errs


def test_relabelling_is_exact_on_the_reference():
    """tail_ld of the relabelled problem is the relabelled tail_ld (measured() relies on it), up to the longdouble solves."""
    name = "n400_d3_m64_p1_matern"
    c, v = T.CASES[name], T.inputs(name)
    S, Si = T.sqrt_f64(name)
    ref = T.reference(T.variant(name))
    pi, po = T._perms(v, 1)
    Gp, Kmm, Kin, Kxo = T.relabel(v, v.G, pi, po)
    again = T.tail_ld(Gp, Kmm, Kin, Kxo, c.n, c.gamma, c.jitter, S[po][:, po], Si[po][:, po])
    dist = T.distances(again, T.relabelled(ref, po))
    bar = T.bars(T.variant(name))
    assert all(dist[b] < 1e-3 * bar[b] for b in dist), (dist, bar)


@pytest.mark.parametrize("m,d,p", [(64, 3, 1), (5, 1, 0), (33, 5, 2), (65, 7, 6)])
def test_packed_layout_round_trips(m, d, p):
    """(2m + p)(m + p) odd: the second block starts one double later, at the even offset (64, 3, 1 and 5, 1, 0); even: directly
    behind the first (33, 5, 2 and 65, 7, 6)."""
    rng = np.random.default_rng(m)
    G = dict(G1=rng.standard_normal((m + p, m + p)), G2=rng.standard_normal((m, m + p)), G3=rng.standard_normal((m, m)),
             G4=rng.standard_normal((d, m)))
    flat = R.pack(G["G1"], G["G2"], G["G3"], G["G4"], fill=np.nan)
    first = (2 * m + p) * (m + p)
    assert R.gram_block1(m, p) == first + first % 2 and flat.shape == (R.gram_block1(m, p) + (m + d) * m,)
    assert np.isnan(flat).sum() == first % 2 and (first % 2 == 0 or np.isnan(flat[first]))
    back = R.unpack(flat, m, d, p)
    assert all(np.array_equal(back[k], G[k]) for k in G)


@pytest.mark.parametrize("name", T.REFINE_CASES)
def test_refinement_systems_and_the_refined_bar(name):
    """cond(inner) and cond(inner_rec) are in the range the GPU test asks for; the fp64 emulation of the refinement takes both steps on both systems,
    meets the refined operators' bar and ends nearer the reference than the unrefined comparison solver."""
    c, v, key = T.CASES[name], T.inputs(name), T.variant(name)
    lo, hi = T.REFINE_COND
    k_inner, k_rec = T.conds(key)
    assert lo <= k_inner <= hi and lo <= k_rec <= hi, (k_inner, k_rec)
    S, Si = T.sqrt_f64(name)
    ref = T.reference(key)
    got, accepted, ratio0 = T.refine_emulate(key)
    bar = T.bars(key, converged_solves=True)
    r = T.ratios(got, ref, bar)
    plain = T.distances(T.tail_f64(v.G, v.K_mm, v.K_in, v.K_xo, c.n, c.gamma, c.jitter, S, Si, not c.sep), ref)
    refined = T.distances(got, ref)
    print(f"fit-tail: {name}: cond {k_inner:.2e} / {k_rec:.2e}, emulated refinement err / bar "
          + ", ".join(f"{b} {x:.3f}" for b, x in r.items()) + f", accepted {accepted}, |dX0| / |X| {ratio0}")
    assert accepted == [2, 2] and all(0.0 < x < 0.25 for x in ratio0)
    assert max(r.values()) <= 1.0, r
    assert all(refined[b] <= plain[b] for b in plain), (refined, plain)
    # what the reference itself is known to stays under the comparison solver's own distance (a quarter of the bar)
    res = T.resolution(key)
    print(f"fit-tail: {name}: reference's own spread / bar " + ", ".join(f"{b} {res[b] / bar[b]:.4f}" for b in res))
    assert all(res[b] <= bar[b] / T.MARGIN for b in res), (res, bar)


def test_the_small_refinement_case_is_well_conditioned():
    assert max(T.conds(T.variant(T.REFINE_SMALL))) < 1e5
