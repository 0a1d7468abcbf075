"""KoopmanSplineRegressor without a GPU: the estimator surface of the reference's thin-plate-spline class
(regressors.py:181-233), its random draws of the centres, and the absence of any CPU fallback."""
import inspect
import pickle

import numpy as np
import pytest
from sklearn.base import clone

import nys_koop_lqr_amd as nk
from nys_koop_lqr_amd import _lib


def cloth_training_states(golden):
    """States of the seed-0 training split of f15_spline_cloth.npz, d x n as the reference's lift sees them."""
    g = golden("f15_spline_cloth.npz")
    t = golden("cloth_trajs_all.npz")
    states = t["states_e10"] / 1e10
    return np.hstack([states[i][:, :-1] for i in g["train"]]), g


def test_import_and_signature():
    assert "KoopmanSplineRegressor" in nk.__all__
    assert issubclass(nk.KoopmanSplineRegressor, nk.KoopmanRegressor)
    sig = inspect.signature(nk.KoopmanSplineRegressor.__init__)
    assert list(sig.parameters) == ["self", "n_inputs", "state_bounds_params", "m", "gamma"]
    assert [sig.parameters[k].default for k in ("state_bounds_params", "m", "gamma")] == [None, None, None]
    reg = nk.KoopmanSplineRegressor(6)
    assert reg.centers is None and reg.A is None and reg.B is None and reg.C is None and reg.weights is None


def test_get_params_clone_pickle_unfitted():
    reg = nk.KoopmanSplineRegressor(1, state_bounds_params=np.array([1.0, 2]), m=20, gamma=1e-6)
    params = reg.get_params()
    assert set(params) == {"n_inputs", "state_bounds_params", "m", "gamma"}
    assert params["m"] == 20 and params["gamma"] == 1e-6 and params["n_inputs"] == 1
    c = clone(reg)
    assert type(c) is nk.KoopmanSplineRegressor and c.m == 20 and c.centers is None
    np.testing.assert_array_equal(c.state_bounds_params, [1.0, 2.0])
    r2 = pickle.loads(pickle.dumps(reg))
    assert r2.get_params()["m"] == 20 and r2.centers is None and r2.A is None
    reg.set_params(m=30)
    assert reg.m == 30


def test_disc_centres_match_the_reference(golden):
    """benchmark_lqr_classic.py:223-242: np.random.seed(seed), then 20 sequential fits that each draw their centres."""
    g = golden("f15_spline_duffing.npz")
    for seed in g["seeds"]:
        np.random.seed(int(seed))
        cols = g[f"centers_{int(seed)}"]
        o = 0
        for m in g["ms"]:
            reg = nk.KoopmanSplineRegressor(1, state_bounds_params=g["bounds"], m=int(m), gamma=float(g["gamma"]))
            c = reg.compute_centers(None)
            assert c.shape == (2, m)
            np.testing.assert_array_equal(c, cols[:, o:o + m])
            o += int(m)


def test_data_centres_match_the_reference(golden):
    """benchmark_lqr_cloth.py:168-199: after np.random.seed(0) and the shuffle of the split, the fits of m = 10, 12, 14 draw
    their centres from the training states in sequence."""
    S, g = cloth_training_states(golden)
    np.random.seed(0)
    np.random.shuffle(np.arange(0, 40))
    for k in range(3):
        reg = nk.KoopmanSplineRegressor(6, m=int(g["ms"][k]), gamma=float(g["gammas"][k]))
        c = reg.compute_centers(S)
        np.testing.assert_array_equal(c, S[:, g[f"c{k}_centers_idx"]])


def test_fit_without_gpu_raises(monkeypatch):
    """No CPU fallback: without a device the fit fails with NyskoopError."""
    try:
        count = _lib.load_library().nk_device_count()
    except _lib.NyskoopError:
        count = 0
    if count > 0:
        pytest.skip("a device is visible: tests/test_gpu_spline.py covers the fit")
    reg = nk.KoopmanSplineRegressor(1, state_bounds_params=np.array([1.0, 2]), m=10, gamma=1e-6)
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((100, 3)), rng.standard_normal((100, 2))
    with pytest.raises(nk.NyskoopError):
        reg.fit(X, Y)
    assert reg.A is None and reg.weights is None


def test_abi_declares_the_spline_entry_points():
    for name in ("nk_spline_fit", "nk_spline_model_create"):
        assert name in _lib.SIGNATURES
    assert _lib.NK_KERNEL_TPS == 3
