"""Regenerate tests/golden/setup.npz — runs in the survey container only.

One 4x4 deck (nst 2000, one step) with a different medium in each of the 16
zones is run through the reference driver (oracle/_ref/c2d_refdrv, built by
__graft_entry__.build()); f_nt and Pnt of setup's gam_min + P_nontherm are
taken from in_000.bin, which the driver writes and closes before any
transport, so the dump is valid even where a later phase of the reference
dislikes a medium (the driver's exit status is not checked; the file's size
is).  A second 1x2 deck with T_const = 0 and two steps holds the two mixed
media; its fpin_001.bin gives the gmin that gam_min adjusted.

The media reach every branch of gam_min / P_nontherm (see MEDIA below).
Only arrays are stored: inputs, f_nt, Pnt, gmin.

    python tests/golden/make_setup_golden.py
"""
from __future__ import annotations

import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import refcase  # noqa: E402
from compton2d_amd import abi  # noqa: E402

#        tea      amxwl          gmin    gmax   p_nth
MEDIA = (
    ("100.0", "0.0", "100.0", "1.0E+05", "2.3"),          # 0  the inputm.dat medium
    ("100.0", "0.0", "1.005", "1.0E+04", "2.5"),          # 1  gmin < 1.01: clamped
    ("100.0", "0.0", "10.0", "1.0E+04", "1.0"),           # 2  p_nth = 1: p_1 nudged in gam_min only
    ("100.0", "0.0", "10.0", "1.0E+04", "2.0"),           # 3  p_nth = 2: p_2 nudged
    ("100.0", "0.0", "2.0", "50.0", "2.2"),               # 4  gmax so small that g/gmax >= 100 in the tail
    ("100.0", "0.0", "100.0", "1.0E+09", "2.3"),          # 5  gmax above the grid's last gamma
    ("50.0", "1.0", "10.0", "1.0E+04", "2.3"),            # 6  amxwl = 1
    ("50.0", "0.999999995", "10.0", "1.0E+04", "2.3"),    # 7  between 0.99999999d0 and the REAL 0.99999999
    ("100.0", "5.0E-05", "10.0", "1.0E+04", "2.3"),       # 8  below 1e-4
    ("100.0", "2.0E-04", "10.0", "1.0E+04", "2.3"),       # 9  above 1e-4
    ("200.0", "0.5", "20.0", "1.0E+04", "2.3"),           # 10 mixed, tea >= 1
    ("50.0", "0.9", "5.0", "1.0E+03", "3.0"),             # 11 mixed, tea >= 1
    ("0.5", "0.5", "10.0", "1.0E+04", "2.3"),             # 12 mixed, tea < 1
    ("5.0", "0.5", "10.0", "1.0E+04", "2.3"),             # 13 cold: the Maxwellian reaches y >= 100
    ("600.0", "1.0", "10.0", "1.0E+04", "2.3"),           # 14 thermal, Theta > 0.2 (McDonald)
    ("300.0", "0.3", "50.0", "1.0E+05", "1.8"),           # 15 mixed, Theta > 0.2
)
MIXED = (10, 11)
KEYS = ("tea", "amxwl", "gmin", "gmax", "p_nth")


def zone_file(path: Path, m) -> None:
    """An input_JJ_KK.dat with the medium's five values as written in MEDIA
    (the reader's e14.7 field takes any decimal that fits its 14 columns)."""
    tea, amxwl, gmin, gmax, p_nth = m
    rows = (("tea", tea), ("tna", "100.0"), ("n_e", "80.0"), ("ep_switch", "0"), ("B_field", "0.13"),
            ("amxwl", amxwl), ("gmin", gmin), ("gmax", gmax), ("p_nth", p_nth), ("q_turb", "1.666667"),
            ("turb_lev", "1.0E-20"))
    for _, v in rows:
        assert len(v) <= 14
    path.write_text("".join(nm.ljust(80) + v + "\n" for nm, v in rows))


def run(case: Path, nsteps: int) -> None:
    import resource

    def big_stack():
        resource.setrlimit(resource.RLIMIT_STACK, (resource.RLIM_INFINITY, resource.RLIM_INFINITY))
    try:
        subprocess.run([str(refcase.REFDRV), str(nsteps), "1", "0"], cwd=str(case), timeout=900,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, preexec_fn=big_stack)
    except subprocess.TimeoutExpired:
        pass


def main() -> None:
    out = {k: np.array([float(m[i]) for m in MEDIA]) for i, k in enumerate(KEYS)}
    with tempfile.TemporaryDirectory() as td:
        case = Path(td) / "setup16"
        refcase.write_input_deck(case, dict(nz=4, nr=4, nst=2000))
        for z, m in enumerate(MEDIA):
            zone_file(case / "input" / ("input_%02d_%02d.dat" % (z // 4 + 1, z % 4 + 1)), m)
        run(case, 1)
        cfg = refcase.read_config(case)
        nb = (case / "in_000.bin").stat().st_size
        d = refcase.read_step_in(case, 0, cfg)          # raises if the file is short
        print("in_000.bin: %d bytes" % nb)
        out["f_nt"] = d["f_nt"].reshape(16, abi.NUM_NT)
        out["Pnt"] = d["Pnt"].reshape(16, abi.NUM_NT)
        out["gnt"] = cfg["gnt"]

        case2 = Path(td) / "setup_mixed"
        refcase.write_input_deck(case2, dict(nz=1, nr=2, nst=2000, T_const=0))
        for k, z in enumerate(MIXED):
            zone_file(case2 / "input" / ("input_01_%02d.dat" % (k + 1)), MEDIA[z])
        run(case2, 2)
        if refcase.has_fp(case2, 1):
            cfg2 = refcase.read_config(case2)
            fp = refcase.read_fp_in(case2, 1, cfg2)
            out["mixed_zones"] = np.array(MIXED)
            out["mixed_gmin"] = fp["gmin"].reshape(-1)
            out["mixed_f_nt"] = fp["f_nt"].reshape(len(MIXED), abi.NUM_NT)
            print("fpin_001.bin: gmin", out["mixed_gmin"])
        else:
            print("the reference did not reach fpin_001.bin: no gmin stored")
    np.savez_compressed(ROOT / "tests" / "golden" / "setup.npz", **out)
    print("wrote tests/golden/setup.npz")


if __name__ == "__main__":
    main()
