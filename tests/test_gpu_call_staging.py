"""The two staging transports of the latency-bound C-ABI calls (CallStage, nk_api_internal.h): operands that together fit
4 MiB and are all host memory travel through the page-locked block with tight leading dimensions, everything else
through the arena (DMA, even leading dimensions; device pointers in place with the caller's).  Every case crosses that
switch, or the host / device / strided forms of one operand, with the smallest shapes that do."""
import numpy as np
import pytest

from conftest import relf
from test_gpu_round2 import _fitted

pytestmark = pytest.mark.gpu
LIMIT = 4 << 20


@pytest.fixture(scope="module")
def nk():
    import nys_koop_lqr_amd as nk
    nk.get_context()
    return nk


@pytest.fixture(scope="module")
def O():
    from oracle import nk_oracle
    return nk_oracle


@pytest.fixture(scope="module")
def small_model(nk, O):
    """d = 9, p = 2, m = 48 (single-launch chain with its own lift)."""
    return _fitted(nk, O, n=300, d=9, p=2, m=48, seed=50)


def test_lift_and_predict_host_strided_and_device_operands(nk, O, small_model):
    """8 queries as a small host array (page-locked), a host view with ld > cols (page-locked, repacked tight), a float64
    device tensor and a device tensor with a row stride (arena transport, used in place): each against the oracle, and
    predict on the host array and on the device tensor with equal bits."""
    torch = pytest.importorskip("torch")
    reg, ref, X, Y, rng = small_model
    d, dp = 9, 11
    wide = np.ascontiguousarray(rng.standard_normal((8, 15)))
    wide[:, :dp] = X[40:48]
    xa = np.ascontiguousarray(wide[:, :dp])
    wd = torch.from_numpy(wide).to(torch.device("cuda", 0))
    xd = wd[:, :dp].contiguous()
    assert wd[:, :d].stride(0) == 15 and xd.stride(0) == dp
    lift_ref, pred_ref = ref.lift(xa[:, :d].T), ref.predict(xa)
    lifts = dict(host=reg.lift(xa[:, :d].T), host_strided=reg.lift(wide[:, :d].T),
                 device=reg.lift(xd[:, :d].contiguous().t()), device_strided=reg.lift(wd[:, :d].t()))
    preds = dict(host=reg.predict(xa), host_strided=reg.predict(wide[:, :dp]), device=reg.predict(xd),
                 device_strided=reg.predict(wd[:, :dp]))
    for name in lifts:
        el, ep = relf(lifts[name], lift_ref), relf(preds[name], pred_ref)
        print(f"{name}: lift {el:.3e} predict {ep:.3e}")
        assert lifts[name].shape == (48, 8) and preds[name].shape == (8, d)
        assert el < 1e-7 and ep < 1e-7, name
    assert np.array_equal(preds["host"], preds["device"])


def test_lift_above_the_limit(nk, O):
    """2100 queries at m = 256, d = 2: the lifted block alone is 4.3 MB, so the call stages through the arena; its first
    and last 8 rows against the oracle, like the same rows lifted 8 at a time through the page-locked block (the product
    with K_mm^{-1/2} over 2100 rows and over 8 does not give the same bits, so each side is held to the oracle)."""
    reg, ref, X, Y, rng = _fitted(nk, O, n=1024, d=2, p=1, m=256, seed=51, ls=0.3)
    xq = rng.standard_normal((2100, 2))
    assert 2100 * 256 * 8 > LIMIT
    big = reg.lift(xq.T)
    assert big.shape == (256, 2100)
    for rows in (slice(0, 8), slice(2092, 2100)):
        few, want = reg.lift(xq[rows].T), ref.lift(xq[rows].T)
        print(f"rows {rows}: arena {relf(big[:, rows], want):.3e} page-locked {relf(few, want):.3e}")
        assert relf(big[:, rows], want) < 1e-7 and relf(few, want) < 1e-7


def test_rollout_with_lifted_trajectory_above_the_limit(nk, O):
    """batch 8, T = 520, m = 128, p = 6 (single-launch chain): the lifted trajectories are 4.26 MB (arena transport); each
    of the eight single rollouts fits the page-locked block.  The output product x = C z is a GEMM over batch * T rows with
    an even leading dimension in one case and over T rows with a tight one in the other, and its bits differ between the
    two, so each transport is held to the oracle's loop on the same operators; the lifted trajectories have equal bits."""
    reg, ref, X, Y, rng = _fitted(nk, O, n=512, d=9, p=6, m=128, seed=52)
    d, T, batch = 9, 520, 8
    assert batch * T * 128 * 8 > LIMIT > T * (128 + d + 6) * 8 + 4096
    Ub = 0.1 * rng.standard_normal((batch, T, 6))
    xb = X[10:10 + batch, :d]
    out, outz = reg.rollout(xb, Ub, return_lifted=True)
    assert out.shape == (batch, T, d) and outz.shape == (batch, T, 128)
    for b in range(batch):
        sb, zb = reg.rollout(xb[b], Ub[b].T, return_lifted=True)
        so, Zo = O.rollout(reg.A, reg.B, reg.C, reg.lift(xb[b].reshape(-1, 1)), Ub[b].T)
        errs = relf(out[b].T, so), relf(outz[b].T, Zo), relf(sb, so), relf(zb, Zo)
        print(f"trajectory {b}: arena x {errs[0]:.3e} z {errs[1]:.3e} | page-locked x {errs[2]:.3e} z {errs[3]:.3e}")
        assert max(errs) < 1e-11, (b, errs)
        assert np.array_equal(outz[b].T, zb), b  # the recursion is one kernel per trajectory on either transport


def test_open_loop_errors_above_the_limit(nk, O, small_model):
    """64 trajectories of T = 1024, d = 9: 4.7 MB of true trajectories (arena transport); the first four alone fit the
    page-locked block.  The error mode's bits do not depend on the batch."""
    reg, ref, X, Y, rng = small_model
    k, T = 64, 1024
    assert k * T * 9 * 8 > LIMIT > 4 * T * (9 + 2) * 8 + 4096
    trajs = rng.standard_normal((k, 9, T))
    ctrls = 0.1 * rng.standard_normal((k, 2, T))
    for relative in (False, True):
        every = reg.open_loop_errors(trajs, ctrls, relative=relative)
        four = reg.open_loop_errors(trajs[:4], ctrls[:4], relative=relative)
        assert every.shape == (k,) and np.isfinite(every).all()
        assert np.array_equal(every[:4], four)


def test_closed_loop_above_the_limit(nk, O):
    """batch 64, 800 steps, m = 64, d = 9, p = 2: 4.5 MB of states and controls (arena transport); trajectories 0 and 63
    also as single calls (page-locked).  States and controls come out of GEMMs over all rows of the call, whose bits differ
    between 51200 rows and 800, so each transport is held to the oracle's loop."""
    reg, ref, X, Y, rng = _fitted(nk, O, n=400, d=9, p=2, m=64, seed=53)
    d, steps, batch = 9, 800, 64
    assert batch * steps * (d + 2) * 8 > LIMIT
    K = reg.solve_lqr(c=0.5)
    phi0 = reg.lift(X[:batch, :d].T).T
    phir = reg.lift(X[100:100 + batch, :d].T).T
    xs, us = reg.closed_loop(K, phi0, phir, steps)
    assert xs.shape == (batch, steps, d) and us.shape == (batch, steps, 2)
    for b in (0, 63):
        x1, u1 = reg.closed_loop(K, phi0[b], phir[b], steps)
        xo, uo = O.lqr_closed_loop_lifted(reg.A, reg.B, reg.C, K, phi0[b], phir[b], steps)
        print(f"trajectory {b}: arena states {relf(xs[b].T, xo):.3e} controls {relf(us[b].T, uo):.3e} | "
              f"page-locked states {relf(x1, xo):.3e} controls {relf(u1, uo):.3e}")
        assert relf(xs[b].T, xo) < 1e-9 and relf(us[b].T, uo) < 1e-8
        assert relf(x1, xo) < 1e-9 and relf(u1, uo) < 1e-8


def test_give_up_retry_queues_the_arena_outputs_twice(nk, O, monkeypatch):
    """m = 200, p = 3, batch 3, T = 2400 with the lifted trajectory (11.5 MB: arena transport, multi-workgroup recursion).
    With the hook the recursion `gives up`, so the call repeats it stepwise and queues its device-to-host copies a
    second time: same results as the undisturbed call.  The hook reports a give-up after a first attempt that was in
    fact valid and whose copies have already reached the caller's arrays, so this case exercises the second queueing but
    could not tell a repeat that forgot its copies from one that made them."""
    from nys_koop_lqr_amd import _lib
    reg, ref, X, Y, rng = _fitted(nk, O, n=900, d=9, p=3, m=200, seed=21)
    d, T = 9, 2400
    assert 3 * T * 200 * 8 > LIMIT
    Ub = 0.1 * rng.standard_normal((3, T, 3))
    first, firstz = reg.rollout(X[:3, :d], Ub, return_lifted=True)
    before = _lib.runtime_counters()["chain_giveups"]
    monkeypatch.setenv("NYSKOOP_CHAIN_MW_TEST_GIVEUP", "1")
    again, againz = reg.rollout(X[:3, :d], Ub, return_lifted=True)
    monkeypatch.delenv("NYSKOOP_CHAIN_MW_TEST_GIVEUP")
    assert _lib.runtime_counters()["chain_giveups"] == before + 1
    assert np.isfinite(first).all() and np.isfinite(firstz).all()
    print(f"repeat against first: states {relf(again, first):.3e} lifted {relf(againz, firstz):.3e}")
    assert relf(again, first) < 1e-12 and relf(againz, firstz) < 1e-12
    so, _ = O.rollout(reg.A, reg.B, reg.C, reg.lift(X[1, :d].reshape(-1, 1)), Ub[1].T)
    assert relf(again[1].T, so) < 1e-11
