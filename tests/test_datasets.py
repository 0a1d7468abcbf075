"""CPU: the data-format readers against files written in the reference's layout, and against the reference's own
files (their first lines / columns, copied unchanged into tests/golden/reference_csv/ by tests/golden/make_golden_csv.py)
and the committed golden arrays read from the whole files."""
import os
import shutil

import numpy as np

from nys_koop_lqr_amd import datasets, harness

REF_CSV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_csv")


def test_cloth_and_duffing_layouts(tmp_path):
    rng = np.random.default_rng(0)
    for i in range(3):
        np.savetxt(tmp_path / f"state_samples_cloth_swing_{i}.csv", rng.standard_normal((7, 192)), delimiter=",")
        np.savetxt(tmp_path / f"input_samples_cloth_swing_{i}.csv", rng.standard_normal((7, 9)), delimiter=",")
    trajs, ctrls = datasets.load_cloth_experiment(str(tmp_path), n_trajs=3)
    assert [t.shape for t in trajs] == [(192, 7)] * 3 and [c.shape for c in ctrls] == [(6, 7)] * 3
    (vt, vc), (tt, tc) = datasets.cloth_splits(trajs, ctrls, n_val_trajs=1)
    assert len(vt) == 1 and len(tt) == 2
    X, Y = harness.create_data_matrices(tt, tc, range(2))
    assert X.shape == (198, 12) and Y.shape == (192, 12) and np.array_equal(Y[:, 0], tt[0][:, 1])
    for name, shape in (("x_forced", (2, 5)), ("x_unforced", (2, 4)), ("y_forced", (2, 5)), ("y_unforced", (2, 4))):
        np.savetxt(tmp_path / f"duffing_{name}.csv", rng.standard_normal(shape), delimiter=",")
    np.savetxt(tmp_path / "duffing_u_forced.csv", rng.standard_normal(5), delimiter=",")
    X, Y = datasets.load_duffing(str(tmp_path))
    assert X.shape == (3, 9) and Y.shape == (2, 9) and np.all(X[2, 5:] == 0)
    ref = datasets.cloth_reference_state(trajs[0][:, 0])
    assert ref.shape == (192, 1) and np.array_equal(ref[0::3], trajs[0][0::3, :1])  # x coordinates unchanged


def test_readers_on_the_reference_files(golden, tmp_path):
    # the first 2 time steps of the reference's cloth trajectories 10 and 11, as trajectories 0 and 1 of an experiment
    for j, i in enumerate((10, 11)):
        for kind in ("state", "input"):
            shutil.copyfile(os.path.join(REF_CSV, f"{kind}_samples_cloth_swing_{i}.csv"),
                            tmp_path / f"{kind}_samples_cloth_swing_{j}.csv")
    trajs, ctrls = datasets.load_cloth_experiment(str(tmp_path), n_trajs=2)
    g = golden("f6_cloth_known_gain.npz")  # trajectories 10..39 as the reference's scripts slice them
    for j in range(2):
        assert trajs[j].shape == (192, 2) and ctrls[j].shape == (6, 2)
        assert np.array_equal(trajs[j], g["trajs"][j][:, :2]) and np.array_equal(ctrls[j], g["inputs"][j][:, :2])
    # the Duffing CSVs cut after their first 20 (forced) / 30 (unforced) columns; f12 holds the whole files assembled
    X, Y = datasets.load_duffing(REF_CSV)
    f12 = golden("f12_duffing_full.npz")
    assert f12["X"].shape == (69900, 3) and f12["Y"].shape == (69900, 2)
    cols = np.r_[0:20, 20000:20030]  # 20 000 forced columns, then the unforced ones
    assert X.shape == (3, 50) and Y.shape == (2, 50)
    assert np.array_equal(X, f12["X"][cols].T) and np.array_equal(Y, f12["Y"][cols].T)


def test_cloth_reference_state_matches_shipped_csv(golden):
    """datasets.cloth_reference_state (benchmark_lqr_cloth.py:241-255) against the reference's shipped
    8x8_cloth_swing_xyz/sim_results/nystrom/data/reference_lqr.csv (kept in the f10 golden; 5-digit CSV)."""
    from nys_koop_lqr_amd import datasets
    g = golden("f10_lqr_control.npz")
    got = datasets.cloth_reference_state(g["initial_state"])
    assert got.shape == g["reference_lqr"].shape
    assert np.max(np.abs(got - g["reference_lqr"])) < 5e-6
