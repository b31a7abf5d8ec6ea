"""Run directories with several boundary time windows — TEST INFRASTRUCTURE.

`refcase.write_input_deck` writes one window.  `write_deck` writes any number
(src/reader.f:169-283: ntime, then per window t0, t1 and per ring tbbu, a name
line, tbbl, a name line), in the same fixed columns: label in 1-80, value from
column 81.  `ec_case` is the deck of tests/test_deck_ec.py and
tests/test_gpu_deck_ec.py: the 2x2 grid and geometry of the golden case
ec_lower with the inputm.dat medium, Gamma = 25, nst = 3000, FP on, and
`disk/blackbody_G25_4spectra.in` on both lower rings during window 1 only.
"""
from __future__ import annotations

from pathlib import Path

from compton2d_amd import synth
from refcase import BASE_CASE

SEED_FILE = "blackbody_G25_4spectra.in"
EC_CONST = dict(R_blr=2.0e38, fr_blr=0.2, R_ir=0.7e19, fr_ir=0.4, R_disk=2.0e17, d_jet=0.25e17)
CASE = dict(BASE_CASE, nz=2, nr=2, nst=3000, T_const=0, g_bulk=25.0, split1=10, split2=10, split3=3,
            spl3_trg=10, **EC_CONST)
DT = synth.mc_dt(CASE["zmax"], CASE["rmax"], CASE["nz"], CASE["nr"], CASE["mcdt"], CASE["g_bulk"])


def deck_float(v: float) -> float:
    """A value as it comes back from its e14.7 field."""
    return float("%.7E" % v)


def _line(label: str, value) -> str:
    v = "%.7E" % value if isinstance(value, float) else str(value)
    return label[:80].ljust(80) + v + "\n"


def window(t0, t1, tbbu=0.0, tbbl=0.0, file_u="none.in", file_l="none.in", nr=2) -> dict:
    ring = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * nr
    return dict(t0=float(t0), t1=float(t1), tbbu=[float(x) for x in ring(tbbu)],
                tbbl=[float(x) for x in ring(tbbl)], file_u=ring(file_u), file_l=ring(file_l))


def ec_windows(t0=0.0, t1_last=1.0e30, tbbl=-1.0, file_l=SEED_FILE) -> list:
    """Window 1 [t0 gate, ends at 2.25 dt] with the EC lower rings, window 2 without sources."""
    return [window(t0, 2.25 * DT, tbbl=tbbl, file_l=file_l), window(0.0, t1_last)]


def write_deck(run_dir, windows, **over) -> dict:
    """Write input/input.dat and the zone files of CASE (+ over); returns the case."""
    c = dict(CASE, **over)
    d = Path(run_dir)
    (d / "input").mkdir(parents=True, exist_ok=True)
    L = [_line("nz", c["nz"]), _line("nr", c["nr"]), _line("z(nz)", float(c["zmax"])),
         _line("rmin", float(c["rmin"])), _line("r(nr)", float(c["rmax"])), _line("star_switch", 0),
         _line("tstop", float(c["tstop"])), _line("mcdt", float(c["mcdt"])),
         _line("ntime", len(windows))]
    for t, w in enumerate(windows):
        L += [_line("t0(%d)" % (t + 1), w["t0"]), _line("t1(%d)" % (t + 1), w["t1"])]
        for k in range(c["nr"]):
            L += [_line("tbbu", w["tbbu"][k]), _line("u_fname", w["file_u"][k]),
                  _line("tbbl", w["tbbl"][k]), _line("l_fname", w["file_l"][k])]
    L += [_line("spec_switch", c["spec_switch"]), _line("nphreg", len(c["regions"]))]
    for lo, hi, nb in c["regions"]:
        L += [_line("Ephmin", float(lo)), _line("Ephmax", float(hi)), _line("nphbins", nb)]
    L += [_line("nmu", c["nmu"]), _line("nph_lc", len(c["lc"]))]
    for lo, hi in c["lc"]:
        L += [_line("Elcmin", float(lo)), _line("Elcmax", float(hi))]
    for nm in ("output/spb.dat", "output/phb.dat", "output/lcb_01.dat", "evb.dat", "output/temp_b.dat"):
        L.append(_line("file", nm))
    for nm in ("nst", "rseed", "rand_switch", "cr_sent"):
        L.append(_line(nm, c[nm]))
    L += [_line("upper_sent", 0), _line("dh_sentinel", 0)]
    for nm in ("pair_switch", "T_const", "cf_sentinel"):
        L.append(_line(nm, c[nm]))
    for nm in ("r_flare", "z_flare", "t_flare", "sigma_r", "sigma_z", "sigma_t", "flare_amp", "r_esc",
               "r_acc"):
        L.append(_line(nm, float(c[nm])))
    for nm in ("inj_switch", "inj_dis", "g2var_switch", "pick_sw"):
        L.append(_line(nm, int(c[nm])))
    for nm in ("inj_g1", "inj_g2", "inj_p", "inj_t", "inj_L", "pick_rate", "inj_gg", "inj_sigma", "g_bulk",
               "R_blr", "fr_blr", "R_ir", "fr_ir", "R_disk", "d_jet"):
        L.append(_line(nm, float(c[nm])))
    for nm in ("split1", "split2", "split3", "spl3_trg"):
        L.append(_line(nm, c[nm]))
    (d / "input" / "input.dat").write_text("".join(L))
    zone = "".join([_line(nm, float(c[nm])) for nm in ("tea", "tna", "n_e")] + [_line("ep_switch", 0)] +
                   [_line(nm, float(c[key])) for nm, key in (("B_field", "B"), ("amxwl", "amxwl"), ("gmin", "gmin"),
                                                           ("gmax", "gmax"), ("p_nth", "p_nth"),
                                                           ("q_turb", "q_turb"), ("turb_lev", "turb_lev"))])
    for j in range(1, c["nz"] + 1):
        for k in range(1, c["nr"] + 1):
            (d / "input" / ("input_%02d_%02d.dat" % (j, k))).write_text(zone)
    return c
