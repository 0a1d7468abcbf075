#!/usr/bin/env python3
"""Copy the first lines / columns of a few of the reference's data files into tests/golden/reference_csv/ so that the
readers of nys_koop_lqr_amd/datasets.py are tested on the reference's own files without a reference checkout.

    python tests/golden/make_golden_csv.py        # needs a reference checkout at $NK_REFERENCE

What is written (data only, no source text):
  * cloth: state_samples_cloth_swing_{10,11}.csv and input_samples_cloth_swing_{10,11}.csv, their first CLOTH_ROWS
    lines (time steps; trajectories 0 and 1 of f6_cloth_known_gain.npz);
  * duffing: duffing_{x,y}_{forced,unforced}.csv and duffing_u_forced.csv, every line cut after its first
    DUFFING_COLS[kind] comma-separated fields (the whole files are 20 000 forced and 49 900 unforced columns, assembled
    in f12_duffing_full.npz).
Lines and fields are copied unchanged.
"""
import os

REF = os.environ.get("NK_REFERENCE", "")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_csv")
CLOTH_TRAJS = (10, 11)
CLOTH_ROWS = 2
DUFFING_COLS = {"forced": 20, "unforced": 30}


def main():
    if not os.path.isdir(REF):
        raise SystemExit("set NK_REFERENCE to a checkout of the reference")
    os.makedirs(OUT, exist_ok=True)
    for i in CLOTH_TRAJS:
        for kind in ("state", "input"):
            name = f"{kind}_samples_cloth_swing_{i}.csv"
            with open(os.path.join(REF, "8x8_cloth_swing_xyz", name), newline="") as f:
                lines = f.readlines()[:CLOTH_ROWS]
            with open(os.path.join(OUT, name), "w", newline="") as f:
                f.writelines(lines)
    for name in ("x_forced", "u_forced", "y_forced", "x_unforced", "y_unforced"):
        cols = DUFFING_COLS[name.split("_")[1]]
        with open(os.path.join(REF, "duffing", f"duffing_{name}.csv")) as f:
            lines = [",".join(line.rstrip("\n").split(",")[:cols]) + "\n" for line in f]
        with open(os.path.join(OUT, f"duffing_{name}.csv"), "w") as f:
            f.writelines(lines)
    for name in sorted(os.listdir(OUT)):
        print(name, os.path.getsize(os.path.join(OUT, name)), "B")


if __name__ == "__main__":
    main()
