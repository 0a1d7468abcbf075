"""CPU checks of tests/gram_reference.py, the reference and bars of tests/test_gpu_gram_entries.py: the longdouble kernels
against the oracle's, the packed layout, the identity-input extraction, every bar against a plain NumPy emulation of what the
device does (worst ratios printed), and mutation checks -- each defect a Gram launch could have exceeds the bar on every
shape the GPU tests use, so a bar that holds on the GPU means something."""
import ctypes as C

import numpy as np
import pytest

import gram_reference as R
from gram_reference import LD, LINEAR, MATERN, RBF, U32, U64

pytestmark = pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason=R.LONGDOUBLE_SKIP)


def _ulps(got, ref):
    return float(np.max(np.abs(got - ref) / np.spacing(np.abs(ref))))


# ------------------------------------------------------------------------------------------------- kernel_ld vs the oracle
@pytest.mark.parametrize("family", [RBF, MATERN, LINEAR])
@pytest.mark.parametrize("aniso", [False, True])
def test_kernel_ld_rounds_to_the_oracle(family, aniso):
    """Within 4 ulp of oracle.nk_oracle (scipy cdist in fp64).  The oracle's own error grows with d r^2 (RBF) and with the
    cancellation of a dot product (linear), so the points are few-dimensional, close and (linear) positive: there the oracle is
    good to a few ulp and a wrong formula, scaling or sigma0 in kernel_ld shows at once."""
    from oracle import nk_oracle as O
    rng = np.random.default_rng(5)
    d = 3
    A, B = rng.uniform(0.1, 1.0, (40, d)), rng.uniform(0.1, 1.0, (23, d))
    B[3] = A[7]  # a coincident point
    ls = np.array([0.8, 1.7, 2.9]) if aniso else np.array([1.3])
    if family == LINEAR:
        got, r2 = R.kernel_ld(A, B, 0.7, LINEAR)
        ref = O.linear_kernel(A, B, 0.7)
        assert r2[7, 3] == 0
    else:
        got, r2 = R.kernel_ld(A, B, ls, family)
        ref = (O.rbf_kernel if family == RBF else O.matern52_kernel)(A, B, ls)
        assert r2[7, 3] == 0 and got[7, 3] == 1
    assert got.dtype == LD and r2.dtype == LD
    worst = _ulps(got.astype(np.float64), ref)
    print(f"kernel_ld {family} aniso={aniso}: {worst:.2f} ulp from the oracle")
    assert worst <= 4.0


# ---------------------------------------------------------------------------------------------------------- packed layout
@pytest.fixture(scope="module")
def lib_gram_doubles():
    """nk_gram_doubles of the built library where it loads (no GPU needed), else None."""
    try:
        from nys_koop_lqr_amd import _lib
        lib = _lib.load_library()
    except Exception:  # noqa: BLE001  (not built on this machine: the formula of the header stands alone)
        return None

    def f(m, d, p):
        cnt = C.c_int64()
        _lib.check(lib.nk_gram_doubles(m, d, p, C.byref(cnt)))
        return int(cnt.value)
    return f


@pytest.mark.parametrize("m,d,p", [(4, 3, 0), (5, 3, 0), (5, 3, 1), (4, 7, 1), (130, 40, 2), (130, 40, 3), (3, 2, 3)])
def test_pack_unpack_round_trip_and_length(lib_gram_doubles, m, d, p):
    """[G1 ; G2] with leading dimension m + p, then [G3 ; G4] with leading dimension m at the next even offset
    (include/nyskoop.h); odd and even (2m + p)(m + p) both occur in the list."""
    rng = np.random.default_rng(m + 10 * d + 100 * p)
    mp = m + p
    G = dict(G1=rng.standard_normal((mp, mp)), G2=rng.standard_normal((m, mp)), G3=rng.standard_normal((m, m)),
             G4=rng.standard_normal((d, m)))
    flat = R.pack(G["G1"], G["G2"], G["G3"], G["G4"], fill=np.nan)
    first = (2 * m + p) * mp
    assert flat.shape == (first + (first & 1) + (m + d) * m,) == (R.gram_doubles(m, d, p),)
    if lib_gram_doubles is not None:
        assert lib_gram_doubles(m, d, p) == flat.size
    assert int(np.isnan(flat).sum()) == (first & 1)  # the one padding entry of an odd first block, nothing else
    back = R.unpack(flat, m, d, p)
    assert all(np.array_equal(back[k], G[k]) for k in G)
    # where the header puts them
    assert flat[0] == G["G1"][0, 0] and flat[mp * mp] == G["G2"][0, 0] and flat[mp + 1] == G["G1"][1, 1]
    assert flat[R.gram_block1(m, p)] == G["G3"][0, 0] and flat[R.gram_block1(m, p) + m * m] == G["G4"][0, 0]
    assert R.gram_block1(m, p) % 2 == 0
    with pytest.raises(AssertionError):
        R.unpack(flat[:-1], m, d, p)


def test_odd_and_even_first_blocks_are_both_tested():
    sizes = [((2 * m + p) * (m + p)) & 1 for m, d, p in [(4, 3, 0), (5, 3, 1), (3, 2, 3), (130, 40, 3)]]
    assert 0 in sizes and 1 in sizes


# ------------------------------------------------------------------------------- gram_ld vs the restatement of test_dist_gloo
def test_gram_ld_agrees_with_the_oracle_restatement():
    """gram_partial as the stub of test_dist_gloo.py restates it with the oracle's kernel (fp64 NumPy), against gram_ld:
    within the contraction bar plus the propagated bar of direct-difference kernel blocks."""
    from oracle import nk_oracle as O
    q = R.problem(600, 12, 24, 3)
    ls = q.par[0]
    kern = O.ThreeDimensionalKernel(ls, ls, ls, q.d)
    m, p, d = q.m, q.p, q.d
    phi_in = np.hstack([kern.kernel(q.X[:, :d], q.Zout), q.X[:, d:]])
    phi_out = kern.kernel(q.Y, q.Zout)
    out = np.zeros(R.gram_doubles(m, d, p))
    b1 = (((2 * m + p) * (m + p)) + 1) & ~1
    out[: (2 * m + p) * (m + p)] = np.vstack([phi_in.T @ phi_in, phi_out.T @ phi_in]).ravel()
    out[b1:] = np.vstack([phi_out.T @ phi_out, q.Y.T @ phi_out]).ravel()
    got = R.unpack(out, m, d, p)
    G, S = R.gram_ld(q.X, q.Y, q.Zin, q.Zout, p, q.kernel)
    fi, U, fo = R.features_ld(q.X, q.Y, q.Zin, q.Zout, p, q.kernel)
    E = R.propagated_bar(*R.kblock_bars(q, "direct"), fi, U, fo, q.Y)
    for k in G:
        r = R.worst_ratio(got[k], G[k], R.contraction_bar(q.n, S[k]) + E[k])
        print(f"oracle restatement {k}: worst err/bar {r:.3f}")
        assert r <= 1.0, (k, r)
    # row ranges: the rows concatenated
    rr = ((0, 100), (150, 150), (400, 600))
    G2, _ = R.gram_ld(q.X, q.Y, q.Zin, q.Zout, p, q.kernel, row_ranges=rr)
    rows = np.r_[0:100, 400:600]
    G3, _ = R.gram_ld(q.X[rows], q.Y[rows], q.Zin, q.Zout, p, q.kernel)
    assert all(np.array_equal(G2[k], G3[k]) for k in G2)


# ------------------------------------------------------------------------------------------------ identity-input extraction
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("n,m", R.A_SHAPES)
def test_identity_inputs_return_the_kernel_block_bit_for_bit(n, m, f32):
    """[Phi | I]^T [Phi | I] has Phi below its leading m x m block: sums with one non-zero term, exact whatever the order."""
    q = R.problem(n, 40, m, n, RBF, False, False, True, 0)
    phi = R.kblock_emulate(q.X[:, :40], q.Zout, q.center, q.par, RBF, np.float32 if f32 else np.float64).astype(np.float64)
    F = np.hstack([phi, q.X[:, 40:]])
    G1 = R.contraction_emulate(F, F, f32=f32)
    assert np.array_equal(G1[m:, :m], phi) and np.array_equal(G1[:m, m:], phi.T)
    assert np.array_equal(G1[m:, m:], np.eye(n))


# ------------------------------------------------------------------------------------------- the bars hold for the emulations
@pytest.mark.parametrize("d", [33, 40, 64])
@pytest.mark.parametrize("kind", ["rbf", "rbf_aniso", "matern", "linear", "rbf_sep"])
def test_kernel_block_bar_holds_for_the_gram_form_in_numpy(kind, d):
    family = {"rbf": RBF, "rbf_aniso": RBF, "matern": MATERN, "linear": LINEAR, "rbf_sep": RBF}[kind]
    q = R.problem(300, d, 130, 300, family, kind == "rbf_aniso", kind == "rbf_sep", True, 0)
    for name, A, Z in (("in", q.X[:, :d], q.Zin), ("out", q.Y, q.Zout)):
        k, r2 = R.kernel_ld(A, Z, q.par, family)
        r = R.worst_ratio(R.kblock_emulate(A, Z, q.center, q.par, family), k,
                          R.kblock_bar_gram_form(A, Z, q.center, q.par, family))
        print(f"gram form fp64 {kind} d={d} {name}: worst err/bar {r:.3f}")
        assert r <= 1.0
        if family != LINEAR and (name == "out" or q.sep):
            assert (r2 == 0).any()  # coincident points are in the data


@pytest.mark.parametrize("d", [40, 64])
@pytest.mark.parametrize("family", [RBF, MATERN])
def test_fp32_kernel_block_emulation_ratio(family, d):
    """The float32 emulation against the fp32 bar: this ratio x 4 is what the device is allowed (f32_kblock_allowance).  It may
    exceed 1: the bar's 8 u |k| does not know the error of a float32 exp, which is why the ratio is measured here."""
    q = R.problem(300, d, 130, 300, family, False, False, True, 0)
    allowed, r = R.f32_kblock_allowance(q.Y, q.Zout, q.center, q.par, family)
    print(f"gram form fp32 emulation {family} d={d}: worst err/bar {r:.3f}, device allowance {allowed:.3f}")
    assert 0.0 < r < 8.0 and allowed == 4.0 * r


def test_direct_bar_holds_for_direct_differences_in_numpy():
    from oracle import nk_oracle as O
    q = R.problem(300, 40, 130, 300, MATERN, False, False, True, 0)
    k, _ = R.kernel_ld(q.Y, q.Zout, q.par, MATERN)
    r = R.worst_ratio(O.matern52_kernel(q.Y, q.Zout, q.par), k, R.kblock_bar_direct(q.Y, q.Zout, q.par, MATERN))
    print(f"direct differences (cdist) matern d=40: worst err/bar {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("f32", [False, True])
def test_contraction_bar_holds_for_numpy(f32):
    key = R.B_CASES["fused_p2"]["key"]
    q = R.problem(*key)
    fi, U, fo = (np.asarray(v, dtype=np.float64) for v in R.problem_features(*key))
    if f32:  # the fp32 engine's kernel blocks are fp32 values: that rounding belongs to the kernel-block bar, not to this one
        fi, fo = fi.astype(np.float32).astype(np.float64), fo.astype(np.float32).astype(np.float64)
    Fin = np.hstack([fi, U])
    G, S = R.gram_from_features(fi.astype(LD), U.astype(LD), fo.astype(LD), q.Y)
    got = dict(G1=R.contraction_emulate(Fin, Fin, f32), G2=R.contraction_emulate(fo, Fin, f32),
               G3=R.contraction_emulate(fo, fo, f32), G4=R.contraction_emulate(q.Y, fo, f32))
    for k in G:
        bar = R.contraction_bar(q.n, S[k], U32 if f32 else 0.0, R.F32_FLUSH_ROWS if f32 else 0)
        r = R.worst_ratio(got[k], G[k], bar)
        print(f"contraction {'fp32' if f32 else 'fp64'} {k}: worst err/bar {r:.4f}")
        assert r <= 1.0
    assert R.contraction_bar(2100, 1.0) < 2.4e-13  # the figure the module's docstring quotes


# ------------------------------------------------------------------------------------------------------------- mutations
def _gram64(Fin, fo, Y):
    return dict(G1=Fin.T @ Fin, G2=fo.T @ Fin, G3=fo.T @ fo, G4=Y.T @ fo)


def _mutants(Fin, fo, Y):
    """name -> Gram blocks (fp64 NumPy) with one defect a launch could have."""
    n, mp = Fin.shape
    m, d = fo.shape[1], Y.shape[1]
    good = _gram64(Fin, fo, Y)
    r = n // 2
    keep = np.r_[0:r, r + 1:n]
    out = {"dropped row": _gram64(Fin[keep], fo[keep], Y[keep])}
    twice = np.r_[0:n, r]
    out["row counted twice"] = _gram64(Fin[twice], fo[twice], Y[twice])
    # one 128 x 128 tile left at its previous contents: zeros (beta = 0), or what the earlier passes left (beta = 1: the last
    # 52 rows are missing from it); the last tile of each block, which is an edge tile wherever there is one
    for name, prev in (("stale tile (zeros)", None), ("stale tile (previous passes)", n - min(52, n))):
        old = _gram64(Fin[:prev], fo[:prev], Y[:prev]) if prev is not None else {k: np.zeros_like(v) for k, v in good.items()}
        for blk in ("G1", "G2", "G3", "G4"):
            g = {k: v.copy() for k, v in good.items()}
            i0, j0 = ((g[blk].shape[0] - 1) // R.TILE) * R.TILE, ((g[blk].shape[1] - 1) // R.TILE) * R.TILE
            g[blk][i0:i0 + R.TILE, j0:j0 + R.TILE] = old[blk][i0:i0 + R.TILE, j0:j0 + R.TILE]
            out[f"{name} of {blk}"] = g
    for blk in ("G1", "G3"):  # TRI_UPPER_MIRROR without the mirror: the strict lower triangle keeps its zeros
        g = {k: v.copy() for k, v in good.items()}
        g[blk] = np.triu(g[blk])
        out[f"un-mirrored lower triangle of {blk}"] = g
    # G4 = Y^T Phi_out with Y read at the wrong leading dimension (d + 1 instead of d, or d instead of the even d + 1)
    g = {k: v.copy() for k, v in good.items()}
    flat = np.concatenate([Y.ravel(), np.zeros(n + d + 1)])
    Yw = np.lib.stride_tricks.as_strided(flat, shape=(n, d), strides=(8 * (d + 1), 8)).copy()
    g["G4"] = Yw.T @ fo
    out["G4 with the wrong leading dimension of Y"] = g
    return good, out


@pytest.mark.parametrize("shape", R.all_shapes(), ids=lambda s: "n{}_d{}_m{}_p{}_{}{}{}".format(
    *s[0][:5], "_sep" if s[0][6] else "", "_ranges" if s[1] else ""))
def test_mutations_exceed_the_bar(shape):
    """Every defect moves at least one entry of the block it hits by more than twice the bar away from the fp64 NumPy Gram,
    which itself sits within a hundredth of the bar of the longdouble reference (test_contraction_bar_holds_for_numpy): so it
    exceeds the bar against the reference.  The bar is the widest a GPU case of this shape uses: the fp32 engine's where the
    shape has an fp32 case, with the propagated kernel-block bar."""
    key, rr = shape
    q = R.problem(*key)
    rows = R.select_rows(q.n, rr)
    fi, U, fo = (np.asarray(v, dtype=np.float64)[rows] for v in R.problem_features(*key))
    Y = q.Y[rows]
    Fin = np.hstack([fi, U])
    n = len(rows)
    has_f32 = q.d >= 32 and not q.sep  # Section A and B run such shapes on the fp32 engine too
    E_in, E_out = R.kblock_bars_f32(q) if has_f32 else R.kblock_bars(q, "gram", U64)
    E = R.propagated_bar(E_in[rows], E_out[rows], fi, U, fo, Y)
    good, mutants = _mutants(Fin, fo, Y)
    S = dict(G1=np.abs(Fin).T @ np.abs(Fin), G2=np.abs(fo).T @ np.abs(Fin), G3=np.abs(fo).T @ np.abs(fo),
             G4=np.abs(Y).T @ np.abs(fo))
    bar = {k: R.contraction_bar(n, S[k], U32 if has_f32 else 0.0, R.F32_FLUSH_ROWS if has_f32 else 0) + E[k] for k in S}
    for name, g in mutants.items():
        hit = [k for k in good if not np.array_equal(g[k], good[k])]
        if n == 1 and ("previous passes" in name or "leading dimension" in name):
            continue  # (one row: "the earlier passes" hold nothing, and a single row reads the same at any leading dimension)
        if q.m == 1 and name == "un-mirrored lower triangle of G3":
            continue  # (a 1 x 1 block has no lower triangle)
        assert hit, name
        for k in hit:
            r = R.worst_ratio(g[k], good[k], bar[k])
            assert r > 2.0, (name, k, r)
        if name in ("dropped row", "row counted twice"):
            assert set(hit) == {"G1", "G2", "G3", "G4"}
