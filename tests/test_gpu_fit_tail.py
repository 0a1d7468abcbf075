"""The tail of a Nystrom fit as nk_nystrom_solve composes it, from GIVEN Gram accumulators to the operators A, B, C, W, block by
block against the longdouble reference of tests/fit_tail_reference.py: the two regularisers of assemble_and_factor, the
even-offset rule of the packed layout, the shortcut K_xo S^-1 = S - jitter S^-1 (shared landmarks) and the real product
(separate ones), the padded transposes, operator_products, the second pass through the products behind the SVD branch and
behind a refinement, and the refinement's own kernels on edge tiles in both directions.  Reference, comparison solver and
device start from the same fp64 accumulator (gram_ld rounded once, handed to fit_from_gram), so the Gram stage is no part of
what is measured; the reference takes the device's own S and S^-1, so the square root (tests/test_gpu_sqrtm.py) is not either.

Every block -- A, B, C, the last row of C, W's state columns, W's input columns -- has its own bar: max(m eps, 4 x the worst
distance of the float64 NumPy tail from the longdouble one over the problem and four relabellings of its landmarks, each in
three equally valid fp64 assemblies of the systems) + the worst movement of the NumPy tail when the landmark kernel matrices move by
+- kblock_bar_direct + (shared landmarks) ||S^2 - K_j|| ||S^-1|| / ||S|| of the device's S.  The caps (first-order
composition of cond x order x eps per solve and gamma_m per product) are printed beside them.  The host test
(test_fit_tail_reference_host.py) shows that each of eleven planted faults -- n_total + 1, a jitter left out of K_in or of the
shortcut, no regulariser on the p x p block, V1 transposed, B one column early, a zero last row of C or last column of W,
G3 / G4 from the unpadded offset, K_in in inner_rec, K_xo transposed -- stands 4e5 .. 6e14 bars above the block it touches.

The refined operators are held to the same kind of bar with the NumPy tail's own fp64 systems solved in longdouble and rounded
(what a converged refinement returns).  On the two ill-conditioned systems (cond(inner) / cond(inner_rec) 5.1e10 / 6.1e10 and
6.8e9 / 1.7e10) every block of the refined operators is no farther from tail_ld than the unrefined one, and no farther from the
fp64 system's own solution either: what the rounding of the assembled fp64 system leaves between any fp64 run and tail_ld
(cond-fold, the same for both runs) does not enter the second comparison, so a correction that is partly wrong shows there
even where the unrefined solve already sits at that floor.  It does for the d = 7 right-hand sides of inner_rec at m = 65:
over fifteen systems of that shape with both condition numbers in 1e9 .. 1e11 the refined C is 0.98 .. 1.08 x nearer tail_ld
than the unrefined one (the m = 130 system: 3.9 x); the system used is one where every block is strictly nearer.
Of the well-conditioned smallest case it is asked that the refinement moves no block by more than its bar.  Its first
correction is at rounding level and certainly within |X| / 4, so step 0 is accepted; whether step 1 is depends on whether one
rounding-level correction is at most half of another, which neither the gate's rule nor the host emulation (first corrections
5e-15, the device's 5e-14) pins down: 1 or 2 accepted steps per system, the recorded run has 2 / 2.

Each check prints its worst err / bar as a "fit-tail: ..." line (pytest -s); profiles/README.md records one MI355X run.

Measured there (worst err / bar over the blocks, every one under 1 and none between bar and cap; profiles/fit_tail.log):
  default route, the seven shapes     0.036 (50, 1, 5, 0)  0.074 (400, 3, 64, 1)  0.098 (400, 5, 33, 2)  0.148 (2100, 7, 65, 6)
                                      0.092 (300, 50, 20, 2)  0.140 (900, 40, 130, 3)  0.073 (900, 4, 257, 2); bars 6e-15 .. 8e-12,
                                      caps 3e-12 .. 1e-4; S and S^-1 at most 0.58 of sqrtm_reference's bars (whiten, m = 33)
  dataflow launch against the chain   the same bits at m = 257 (2 dataflow launches, then 0)
  SVD route                           0.114 (m = 5)  0.953 (m = 20, d = 50, linear: W's input columns 1.7e-14 from the reference
                                      under a bar of 1.8e-14, gelsd's own 4.5e-15; the other blocks 0.40 .. 0.79)  0.540 (m = 33)
                                      0.307 (m = 64)  0.388 (m = 130); rank counter + 1, full ranks
  n_total and n_total + 1             0.098 / 0.093 and 0.074 / 0.043 against their own references; 2.3e8 .. 5e10 bars apart
  refinement, cond 1e9 .. 1e11        unrefined 0.055 and 0.184, refined 0.232 and 0.250 of the refined bar; both steps taken
                                      on both systems, |dX0| / |X| 1e-8 .. 6e-8; unrefined / refined distance from tail_ld:
                                      m = 130 3.9 .. 10.8; m = 65 A 90, B 84, W 1.61 and 1.30, C 1.044, last row of C 1.054; from
                                      the fp64 system's own solution: m = 130 80 .. 2200; m = 65 A 100, B 99, W 18.5 and 7.4,
                                      C 2.66, last row of C 8.46
  refinement, (50, 1, 5, 0)           refined 0.016; moved by 0.038 of a bar; 2 / 2 steps accepted
  device tensor, NaN padding double, lock-step member, NYSKOOP_STRICT_SPD=2 in a child process: the same bits"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fit_tail_reference as T
import sqrtm_reference as sr
from chol_reference import counters

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not T.HAVE_LONGDOUBLE, reason=T.LONGDOUBLE_SKIP)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CNT_RANK_TRUNCATED, CNT_REFINED, CNT_CHOL_FLOW_GIVEUP, CNT_CHOL_FLOW = 2, 4, 5, 6
OPS = ("A", "B", "C", "W", "S", "Sinv")


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()  # fails loudly without a gfx950 device / built library
    return nk


@pytest.fixture(scope="module")
def ctx(nk):
    return nk.get_context()


def _log(line):
    print("fit-tail: " + line)
    path = os.environ.get("NYSKOOP_FIT_TAIL_LOG")
    if path:
        with open(path, "a") as f:
            f.write("fit-tail: " + line + "\n")


# ---------------------------------------------------------------------------------------------------------------------
# the device call
# ---------------------------------------------------------------------------------------------------------------------
def _regressor(nk, v, gamma):
    import types
    from nys_koop_lqr_amd import _lib
    family, par = v.kernel
    code = {T.RBF: _lib.NK_KERNEL_RBF, T.MATERN: _lib.NK_KERNEL_MATERN52, T.LINEAR: _lib.NK_KERNEL_LINEAR}[family]
    kern = nk.kernels.DeviceKernel(code, None, par) if family == T.LINEAR else nk.kernels.DeviceKernel(code, np.asarray(par))
    reg = nk.KoopmanNystromRegressor(v.p, kernel=types.SimpleNamespace(kernel=kern), gamma=gamma, m=v.m)
    reg.jitter = v.case.jitter
    reg.nystrom_centers_output = np.ascontiguousarray(v.Zout.T)
    if v.sep:
        reg.nystrom_centers_input = np.ascontiguousarray(v.Zin.T)
    return reg


def _solve(nk, key, gram=None):
    """fit_from_gram of key = T.variant(...) on the calling thread's context: the operators, S and S^-1 as the model keeps
    them, the fit's statistics.  gram: the accumulator to hand over (default: a fresh copy of the case's packed fp64 array)."""
    import ctypes as C
    import types
    from nys_koop_lqr_amd import _lib
    name, gamma, n_total = key
    v = T.inputs(name)
    reg = _regressor(nk, v, gamma)
    reg.fit_from_gram(np.array(v.packed) if gram is None else gram, n_total, v.d)
    ctx = _lib.get_context()
    S, Si = np.full((v.m, v.m), np.nan), np.full((v.m, v.m), np.nan)
    _lib.check(ctx.lib.nk_model_get(ctx.handle, reg._model, b"S", S.ctypes.data, v.m))
    _lib.check(ctx.lib.nk_model_get(ctx.handle, reg._model, b"I", Si.ctypes.data, v.m))
    out = types.SimpleNamespace(A=np.array(reg.A), B=np.array(reg.B), C=np.array(reg.C), W=np.array(reg.weights), S=S, Sinv=Si,
                                stats=dict(reg.fit_stats_), reg=reg)
    assert out.A.shape == (v.m, v.m) and out.B.shape == (v.m, v.p) and out.C.shape == (v.d, v.m) and out.W.shape == (v.d, v.m + v.p)
    assert all(np.isfinite(getattr(out, k)).all() for k in OPS), name
    return out


_DEFAULT = {}


def _default_run(nk, key):
    """the default route's result of `key`, computed once a module (several checks compare with its bits)"""
    if key not in _DEFAULT:
        _DEFAULT[key] = _solve(nk, key)
    return _DEFAULT[key]


def _same_bits(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in OPS)


_REFERENCES = {}


def _reference(key, got):
    """tail_ld of `key` with the device's S and S^-1 (cached on their bits: two routes with the same bits share it)"""
    k = (key, got.S.tobytes(), got.Sinv.tobytes())
    if k not in _REFERENCES:
        _REFERENCES[k] = T.reference(key, got.S, got.Sinv)
    return _REFERENCES[k]


def _grade(tag, key, got, lstsq=False, converged_solves=False):
    """every block of the operators under its bar; the log line holds err / bar, the bar and the cap of every block"""
    ref = _reference(key, got)
    bar = T.bars(key, got.S, got.Sinv, lstsq=lstsq, converged_solves=converged_solves)
    cap = T.caps(key)
    dist = T.distances(got, ref)
    r = {b: dist[b] / bar[b] for b in dist}
    _log(f"{tag}: err / bar " + ", ".join(f"{b} {x:.3f}" for b, x in r.items()) + " | bar "
         + ", ".join(f"{b} {bar[b]:.2e}" for b in r) + " | cap " + ", ".join(f"{b} {cap[b]:.2e}" for b in r))
    over = {b: (dist[b], bar[b]) for b in r if not dist[b] <= bar[b]}
    assert not over, (tag, "over bar", over)
    return dist, bar


def _device_kj(nk, got, v):
    """K_mm + jitter I from nk_kernel_matrix, which builds these kernels by direct differences in either mode of
    nk_set_kmat_mode, as the fit builds its landmark matrices (fit_sqrt's way: the same kernel code, equal to the fit's own
    matrix to the last bit or so)"""
    K = np.array(got.reg.kernel.kernel(v.Zout, v.Zout))
    assert np.all(np.abs(K - v.K_mm) <= v.E_mm + T.EPS * np.abs(v.K_mm)), float(np.abs(K - v.K_mm).max())
    return K + v.case.jitter * np.eye(v.m)


def _full_rank(key, st):
    v = T.inputs(key[0])
    assert st["rank_inner"] == v.m + v.p and st["rank_inner_rec"] == v.m, st
    assert 0.0 < st["pivot_ratio_inner"] <= 1.0 and 0.0 < st["pivot_ratio_inner_rec"] <= 1.0, st


# ---------------------------------------------------------------------------------------------------------------------
# 1.  the default route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.DEFAULT_CASES)
def test_default_route_block_by_block(nk, name):
    key = T.variant(name)
    v = T.inputs(name)
    c0 = counters()
    got = _default_run(nk, key)
    c1 = counters()
    assert c1[CNT_RANK_TRUNCATED] == c0[CNT_RANK_TRUNCATED] and c1[CNT_REFINED] == c0[CNT_REFINED], (c0, c1)
    assert c1[CNT_CHOL_FLOW_GIVEUP] == c0[CNT_CHOL_FLOW_GIVEUP], (c0, c1)
    _full_rank(key, got.stats)
    assert got.stats["refined"] == 0 and got.stats["refine_ratio_inner"] == 0.0 and got.stats["refine_ratio_inner_rec"] == 0.0
    _grade(f"default {name}", key, got)
    # S and S^-1 themselves, at sqrtm_reference's bars for the host-checked route (residual measures, as for the fits of
    # test_gpu_sqrtm.py: the forward errors are sensitive by kappa_2 to a last-bit difference of K_mm, these are not)
    P = _device_kj(nk, got, v)
    vals, _ = sr.solver_values(P, sr.SOLVERS["host"], None, v.m)
    sbar = sr.bars_from(vals, v.m)
    sgot = sr.measures(got.S, got.Sinv, P)
    _log(f"default {name} square root: measure / bar " + ", ".join(f"{k} {sgot[k] / sbar[k]:.3f}" for k in sgot))
    assert all(sgot[k] <= sbar[k] for k in sgot), (sgot, sbar)
    assert got.stats["sqrt_residual"] < 1e-7


def test_dataflow_and_chain_factorisations_give_the_same_bits(nk, monkeypatch):
    """m = 257, m + p = 259: both systems (and K_mm) are over the threshold of the dataflow launch; NYSKOOP_CHOL_FLOW=0 sends
    the same accumulator through the launch-per-step chain.  The counters say which route ran."""
    key = T.variant(T.FLOW_CASE)
    monkeypatch.delenv("NYSKOOP_CHOL_FLOW", raising=False)
    c0 = counters()
    flow = _solve(nk, key)
    c1 = counters()
    monkeypatch.setenv("NYSKOOP_CHOL_FLOW", "0")
    chain = _solve(nk, key)
    c2 = counters()
    _log(f"flow / chain {T.FLOW_CASE}: dataflow launches {c1[CNT_CHOL_FLOW] - c0[CNT_CHOL_FLOW]} then "
         f"{c2[CNT_CHOL_FLOW] - c1[CNT_CHOL_FLOW]}, give-ups {c2[CNT_CHOL_FLOW_GIVEUP] - c0[CNT_CHOL_FLOW_GIVEUP]}")
    assert c1[CNT_CHOL_FLOW] >= c0[CNT_CHOL_FLOW] + 2  # the pair of systems, and the factor of K_mm + jitter I
    assert c2[CNT_CHOL_FLOW] == c1[CNT_CHOL_FLOW] and c2[CNT_CHOL_FLOW_GIVEUP] == c0[CNT_CHOL_FLOW_GIVEUP]
    assert _same_bits(flow, chain)
    assert _same_bits(flow, _default_run(nk, key))
    _grade(f"chain {T.FLOW_CASE}", key, chain)


# ---------------------------------------------------------------------------------------------------------------------
# 2.  the SVD route: both systems through the pseudo-inverse, the products queued a second time
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.SVD_CASES)
def test_svd_route_block_by_block(nk, ctx, name):
    key = T.variant(name)
    base = _default_run(nk, key)
    c0 = counters()
    ctx.set_strict_spd(2)
    try:
        got = _solve(nk, key)
    finally:
        ctx.set_strict_spd(0)
    c1 = counters()
    assert c1[CNT_RANK_TRUNCATED] == c0[CNT_RANK_TRUNCATED] + 1, (c0, c1)
    _full_rank(key, got.stats)  # well conditioned: gelsd's cut-off drops nothing
    assert got.stats["refined"] == 0
    assert np.array_equal(got.S, base.S) and np.array_equal(got.Sinv, base.Sinv)
    assert not np.array_equal(got.A, base.A) and not np.array_equal(got.C, base.C)  # the other solver did run
    _grade(f"svd {name}", key, got, lstsq=True)
    again = _solve(nk, key)  # and the mode is off again
    assert _same_bits(again, base)


# ---------------------------------------------------------------------------------------------------------------------
# 3.  n_total is the caller's: one accumulator, two row counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n400_d5_m33_p2_rbf", "n400_d3_m64_p1_matern"])
def test_n_total_and_n_total_plus_one_each_meet_their_own_reference(nk, name):
    key = T.variant(name)
    key1 = T.variant(name, n_total=T.CASES[name].n + 1)
    got, got1 = _default_run(nk, key), _solve(nk, key1)
    assert np.array_equal(got.S, got1.S) and np.array_equal(got.Sinv, got1.Sinv)  # the square root does not see n_total
    _, bar = _grade(f"n_total {name}", key, got)
    _grade(f"n_total + 1 {name}", key1, got1)
    apart = T.distances(got1, _reference(key, got))
    _log(f"n_total + 1 {name}: distance from the n_total reference / bar " + ", ".join(f"{b} {apart[b] / bar[b]:.3g}" for b in apart))
    assert all(apart[b] >= 100.0 * bar[b] for b in apart), (apart, bar)


# ---------------------------------------------------------------------------------------------------------------------
# 4.  the opt-in refinement
# ---------------------------------------------------------------------------------------------------------------------
def _refined_run(nk, ctx, key):
    c0 = counters()
    ctx.set_refine(1.0, 2)
    try:
        got = _solve(nk, key)
    finally:
        ctx.set_refine(0.0, 2)
    return got, counters()[CNT_REFINED] - c0[CNT_REFINED]


def _accepted(st):
    return st["refined"] % 16, st["refined"] // 16


@pytest.mark.parametrize("name", T.REFINE_CASES)
def test_refinement_of_ill_conditioned_systems(nk, ctx, name):
    """(nr, mq) = (65, 71) and (7, 65), (130, 133) and (40, 130): resid_dd_kernel's 64 x 64 tiles with edges in both
    directions and mq % 16 != 0, the padded transposes around the correction solve, refine_norms_partial / refine_gate /
    guarded_add, then the products a second time."""
    key = T.variant(name)
    plain = _default_run(nk, key)
    _full_rank(key, plain.stats)
    assert plain.stats["refined"] == 0
    d_plain, _ = _grade(f"unrefined {name}", key, plain)
    got, counted = _refined_run(nk, ctx, key)
    st = got.stats
    a0, a1 = _accepted(st)
    _log(f"refined {name}: accepted steps {a0} / {a1}, |dX0| / |X| {st['refine_ratio_inner']:.3e} / {st['refine_ratio_inner_rec']:.3e}, "
         f"pivot ratios {st['pivot_ratio_inner']:.3e} / {st['pivot_ratio_inner_rec']:.3e}")
    _full_rank(key, st)
    # cond x (the factor's backward error) is 1e-7 .. 1e-5 here: the first correction is far inside |X| / 4 and the second
    # far inside half the first, so both steps are taken on both systems (the host test's emulation takes them too)
    assert (a0, a1) == (2, 2) and counted == 1, (st, counted)
    assert 0.0 < st["refine_ratio_inner"] < 0.25 and 0.0 < st["refine_ratio_inner_rec"] < 0.25, st
    assert np.array_equal(got.S, plain.S) and np.array_equal(got.Sinv, plain.Sinv)
    d_ref, _ = _grade(f"refined {name}", key, got, converged_solves=True)
    _log(f"refined {name}: unrefined / refined distance " + ", ".join(f"{b} {d_plain[b] / d_ref[b]:.4f}" for b in d_ref))
    assert all(d_ref[b] <= d_plain[b] for b in d_ref), (d_ref, d_plain)
    # and nearer the fp64 system's own solution (the NumPy tail with its systems solved in longdouble, in each way of assembling
    # them): what the rounding of the assembled system leaves between either run and tail_ld does not enter here, so this is
    # where a correction that is partly wrong on a tile shape shows
    v = T.inputs(name)
    for how in range(T.ASSEMBLIES):
        own = T.tail_f64(v.G, v.K_mm, v.K_in, v.K_xo, key[2], key[1], v.case.jitter, got.S, got.Sinv, not v.sep, solves="ld",
                         assembly=how)
        o_plain, o_ref = T.distances(plain, own), T.distances(got, own)
        _log(f"refined {name}: unrefined / refined distance from the fp64 system's own solution (assembly {how}) "
             + ", ".join(f"{b} {o_plain[b] / o_ref[b]:.2f}" for b in o_ref))
        assert all(o_ref[b] <= o_plain[b] for b in o_ref), (how, o_ref, o_plain)
    again = _solve(nk, key)  # switched off again: the unrefined bits
    assert again.stats["refined"] == 0 and _same_bits(again, plain)


def test_refinement_leaves_a_well_conditioned_fit_where_it_is(nk, ctx):
    """(nr, mq) = (5, 5) and (1, 5): one partial tile, a single row.  Both systems are refined (the threshold 1.0 is above any
    pivot ratio), the corrections are at rounding level, and no block moves by more than its bar."""
    name = T.REFINE_SMALL
    key = T.variant(name)
    plain = _default_run(nk, key)
    got, counted = _refined_run(nk, ctx, key)
    st = got.stats
    a0, a1 = _accepted(st)
    _log(f"refined {name}: accepted steps {a0} / {a1}, |dX0| / |X| {st['refine_ratio_inner']:.3e} / {st['refine_ratio_inner_rec']:.3e}")
    # the first correction is accepted (rounding level against |X| / 4); the second is as small as the first and may or may not halve it
    assert 1 <= a0 <= 2 and 1 <= a1 <= 2 and counted == 1, (st, counted)
    assert 0.0 < st["refine_ratio_inner"] < 0.25 and 0.0 < st["refine_ratio_inner_rec"] < 0.25, st
    _, bar = _grade(f"refined {name}", key, got, converged_solves=True)
    moved = T.distances(got, plain)
    _log(f"refined {name}: moved / bar " + ", ".join(f"{b} {moved[b] / bar[b]:.3f}" for b in moved))
    assert all(moved[b] <= bar[b] for b in moved), (moved, bar)


# ---------------------------------------------------------------------------------------------------------------------
# 5.  a device-resident accumulator: the same bits, and the caller's tensor untouched
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n400_d3_m64_p1_matern", "n400_d5_m33_p2_rbf"])
def test_device_resident_accumulator_gives_the_bits_and_stays_unchanged(nk, name):
    """The tail assembles and factors in place: it must do so on its own copy.  (64, 1): the padded offset of G3 / G4."""
    import torch
    key = T.variant(name)
    v = T.inputs(name)
    acc = torch.from_numpy(np.array(v.packed)).to("cuda")
    keep = acc.clone()
    torch.cuda.synchronize()
    got = _solve(nk, key, gram=acc)
    torch.cuda.synchronize()
    assert torch.equal(acc, keep) and np.array_equal(acc.cpu().numpy(), v.packed)
    assert _same_bits(got, _default_run(nk, key))


def test_padding_double_of_the_packed_layout_is_never_read(nk):
    """(2m + p)(m + p) odd: the double between the two blocks belongs to nobody; NaN there changes nothing."""
    name = "n400_d3_m64_p1_matern"
    v = T.inputs(name)
    first = (2 * v.m + v.p) * (v.m + v.p)
    assert first % 2 == 1
    gram = np.array(v.packed)
    gram[first] = np.nan
    assert _same_bits(_solve(nk, T.variant(name), gram=gram), _default_run(nk, T.variant(name)))


# ---------------------------------------------------------------------------------------------------------------------
# 6.  a lock-step group member
# ---------------------------------------------------------------------------------------------------------------------
def test_lockstep_member_gives_the_ordinary_contexts_bits(nk):
    from nys_koop_lqr_amd import _lib
    key = T.variant(T.LOCKSTEP_CASE)
    base = _default_run(nk, key)
    pool = _lib.lockstep_pool(2, index=12)

    def unit(k):
        out = _solve(nk, k)
        out.reg = None  # (the model belongs to the member's context: dropped inside the round)
        return out

    members = pool.run_round(unit, [key, key])
    assert all(_same_bits(mres, base) for mres in members)
    assert all(mres.stats["rank_inner"] == base.stats["rank_inner"] and mres.stats["refined"] == 0 for mres in members)


# ---------------------------------------------------------------------------------------------------------------------
# 7.  NYSKOOP_STRICT_SPD
# ---------------------------------------------------------------------------------------------------------------------
CHILD = """
import json, os, sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import fit_tail_reference as T
import test_gpu_fit_tail as G
from chol_reference import counters
import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import _lib
key = T.variant({name!r})
c0 = counters()
got = G._solve(nk, key)
c1 = counters()
refused = []
for bad in ("3", "-1", "1x", "two"):
    os.environ["NYSKOOP_STRICT_SPD"] = bad
    try:
        _lib.Context(0)
        refused.append(False)
    except Exception as e:
        refused.append("NYSKOOP_STRICT_SPD" in str(e))
np.save({out!r}, np.hstack([got.A, got.B]))
print(json.dumps(dict(truncated=c1[2] - c0[2], rank_inner=got.stats["rank_inner"], rank_inner_rec=got.stats["rank_inner_rec"],
                      refused=refused)))
"""


def test_strict_spd_2_from_the_environment_takes_the_svd_route(nk, ctx, tmp_path):
    """NYSKOOP_STRICT_SPD=2 before nk_create is nk_set_strict_spd(ctx, 2): a well-conditioned fit_from_gram in a fresh process
    reports the SVD route through the rank-truncation counter and returns the bits of the setter's route here; values other
    than 0, 1, 2 are refused, as the setter refuses them."""
    name = T.LOCKSTEP_CASE
    out = str(tmp_path / "ab.npy")
    script = tmp_path / "child.py"
    script.write_text(CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), name=name, out=out))
    env = dict(os.environ, NYSKOOP_STRICT_SPD="2")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rep = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    v = T.inputs(name)
    assert rep["truncated"] == 1 and rep["rank_inner"] == v.m + v.p and rep["rank_inner_rec"] == v.m, rep
    assert rep["refused"] == [True, True, True, True], rep
    ctx.set_strict_spd(2)
    try:
        here = _solve(nk, T.variant(name))
    finally:
        ctx.set_strict_spd(0)
    assert np.array_equal(np.load(out), np.hstack([here.A, here.B]))
