"""Input decks of the reference, and coupled workloads started from them.

`read_deck` parses a run directory's `input/input.dat` and every
`input/input_JJ_KK.dat` (fixed columns: label in 1-80, value from column 81;
field order of src/reader.f:157-657) into the keys of `synth.C3_DECK`, the
zone medium as [nz, nr] arrays.  It is the inverse of the test helper
`refcase.write_input_deck`.

`deck_workload` builds a `synth.CoupledWorkload` from such a deck (or a dict
like `synth.C3_DECK`, whose medium scalars stand for every zone).  Unlike
`synth.c3_workload`, which starts every zone from the one medium shipped in
data/medium_inputm.npz, the initial electron spectra and the IC-loss table
come from the run-setup calls (csrc/setup.hip): gam_min + P_nontherm per zone
and IC_loss, on the GPU or on the host.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

from . import abi, engine, synth

MEDIUM_KEYS = ("tea", "tna", "n_e", "B", "amxwl", "gmin", "gmax", "p_nth", "q_turb", "turb_lev")
SETUPS = ("device", "host-det", "host-libm")


_NUMBER = re.compile(r"[+-]?(\d+\.?\d*|\.\d+)(e[+-]?\d+)?")


class _Lines:
    """The values of a deck file in order: whatever starts at column 81."""

    def __init__(self, path: Path):
        self.path = path
        self.rows = [ln.rstrip("\n") for ln in Path(path).read_text().splitlines() if ln.strip()]
        self.i = 0

    def _field(self, width: int) -> str:
        if self.i >= len(self.rows):
            raise ValueError("%s: ends after %d values" % (self.path, self.i))
        f = self.rows[self.i][80:80 + width].strip()
        self.i += 1
        if not f:
            raise ValueError("%s: no value from column 81 in line %d" % (self.path, self.i))
        return f

    def int(self) -> int:
        return int(self._field(10))

    def float(self) -> float:
        """An e14.7 field: the 14 columns from column 81, d or e exponents.  A
        longer number is cut there as the reference's reader cuts it
        (inputm.dat's `0.00000000000e+0` loses its exponent)."""
        f = self._field(14).lower().replace("d", "e")
        m = _NUMBER.match(f)
        if not m:
            raise ValueError("%s: line %d: not a number: %r" % (self.path, self.i, f))
        return float(m.group(0))

    def str(self) -> str:
        return self._field(30)


def read_deck(run_dir) -> dict:
    """The deck of `run_dir` (input/input.dat + input/input_JJ_KK.dat)."""
    d = Path(run_dir)
    L = _Lines(d / "input" / "input.dat")
    k = {}
    k["nz"], k["nr"] = L.int(), L.int()
    nz, nr = k["nz"], k["nr"]
    k["zmax"], k["rmin"], k["rmax"] = L.float(), L.float(), L.float()
    if L.int() != 0:
        raise ValueError("read_deck: star_switch != 0 is not supported")
    k["tstop"], k["mcdt"] = L.float(), L.float()
    if L.int() != 1:
        raise ValueError("read_deck: ntime != 1 is not supported")
    k["t0"], k["t1"] = L.float(), L.float()
    tbbu, tbbl, names = [], [], []
    for _ in range(nr):
        tbbu.append(L.float())
        names.append(L.str())
        tbbl.append(L.float())
        names.append(L.str())
    # one value when every ring has the same, else the list (refcase.write_input_deck takes both)
    k["tbbu"] = tbbu[0] if len(set(tbbu)) == 1 else tbbu
    k["tbbl"] = tbbl[0] if len(set(tbbl)) == 1 else tbbl
    k["spec_file"] = names[0]
    k["spec_switch"] = L.int()
    k["regions"] = tuple((L.float(), L.float(), L.int()) for _ in range(L.int()))
    k["nmu"] = L.int()
    k["lc"] = tuple((L.float(), L.float()) for _ in range(L.int()))
    for _ in range(5):          # spectrum, photon, light-curve, event and temperature file names
        L.str()
    k["nst"], k["rseed"], k["rand_switch"], k["cr_sent"] = L.int(), L.int(), L.int(), L.int()
    L.int()                     # upper_sent
    L.int()                     # dh_sentinel
    k["pair_switch"], k["T_const"], k["cf_sentinel"] = L.int(), L.int(), L.int()
    for nm in ("r_flare", "z_flare", "t_flare", "sigma_r", "sigma_z", "sigma_t", "flare_amp",
               "r_esc", "r_acc"):
        k[nm] = L.float()
    for nm in ("inj_switch", "inj_dis", "g2var_switch", "pick_sw"):
        k[nm] = L.int()
    for nm in ("inj_g1", "inj_g2", "inj_p", "inj_t", "inj_L", "pick_rate", "inj_gg", "inj_sigma",
               "g_bulk"):
        k[nm] = L.float()
    for _ in range(6):          # R_blr, fr_blr, R_ir, fr_ir, R_disk, d_jet
        L.float()
    for nm in ("split1", "split2", "split3", "spl3_trg"):
        k[nm] = L.int()
    for nm in MEDIUM_KEYS:
        k[nm] = np.zeros((nz, nr))
    k["ep_switch"] = np.zeros((nz, nr), dtype=np.int32)
    for j in range(nz):
        for kk in range(nr):
            Z = _Lines(d / "input" / ("input_%02d_%02d.dat" % (j + 1, kk + 1)))
            for nm in ("tea", "tna", "n_e"):
                k[nm][j, kk] = Z.float()
            k["ep_switch"][j, kk] = Z.int()
            for nm in ("B", "amxwl", "gmin", "gmax", "p_nth", "q_turb", "turb_lev"):
                k[nm][j, kk] = Z.float()
    return k


def _zones(deck: dict, key: str) -> np.ndarray:
    return np.ascontiguousarray(np.broadcast_to(np.asarray(deck[key], dtype=np.float64),
                                                (deck["nz"], deck["nr"])))


def deck_workload(deck: dict, sources: int, setup: str = "device",
                  comtot_mode: int = abi.COMTOT_TABLE, rank: int = 0, world: int = 1, device: int = 0,
                  seed: int = 0x5EEDC2D, census_capacity: int | None = None,
                  event_capacity: int | None = None) -> synth.CoupledWorkload:
    """A T_const = 0 workload of `deck` with `sources` volume packets per step
    (nst = 2*sources, src/imcgen2d.f:448).  setup: "device" (the setup
    kernels on GPU `device`), "host-det" (their host twin, the same bits) or
    "host-libm" (the host with the C library's log/exp/pow, the reference's
    bits)."""
    if setup not in SETUPS:
        raise ValueError("deck_workload: setup must be one of %s" % (SETUPS,))
    if deck["nmu"] != 1:
        raise ValueError("deck_workload: one angular bin only (nmu = %d)" % deck["nmu"])
    if np.any(np.asarray(deck["tbbu"]) != 0.0) or np.any(np.asarray(deck["tbbl"]) != 0.0):
        raise ValueError("deck_workload: boundary sources (tbbu / tbbl != 0) are not driven")
    nz, nr = deck["nz"], deck["nr"]
    med = {k: _zones(deck, k) for k in MEDIUM_KEYS}
    gnt, E_field, E_ph = abi.setup_grids()
    ins = [med[k] for k in ("tea", "amxwl", "gmin", "gmax", "p_nth")]
    if setup == "device":
        el = engine.setup_electrons(*ins, device=device)
        F_IC = engine.ic_loss(gnt, E_field, device=device)
    else:
        el = abi.setup_electrons_host(*ins, libm=setup == "host-libm")
        F_IC = abi.ic_loss_host(gnt, E_field, libm=setup == "host-libm")

    z, r, vol, zs = synth.zone_geometry(nz, nr, deck["zmax"], deck["rmin"], deck["rmax"])
    dt = synth.mc_dt(deck["zmax"], deck["rmax"], nz, nr, deck["mcdt"], deck["g_bulk"])
    lc = np.array(deck["lc"])
    per_gpu = int(np.ceil(sources / world))
    grid = abi.GridConfig(
        nz=nz, nr=nr, rmin=deck["rmin"], zmin=0.0, z=z, r=r, E_ph=E_ph, E_field=E_field, gnt=gnt,
        hu=synth.photon_grid(deck["regions"]), Elcmin=lc[:, 0], Elcmax=lc[:, 1], mu=np.array([1.0]),
        split1=deck["split1"], split2=deck["split2"], split3=deck["split3"], spl3_trg=deck["spl3_trg"],
        spec_switch=deck["spec_switch"], cr_sent=deck["cr_sent"], pair_switch=deck["pair_switch"],
        comtot_mode=comtot_mode, device=device, seed=seed, rank=rank, world=world,
        census_capacity=census_capacity or max(1 << 20, 8 * per_gpu),
        event_capacity=event_capacity or max(1 << 20, 2 * per_gpu),
        queue_capacity=1 << 20)
    cells = (nz, nr)
    # gmin is the one gam_min adjusted, as the reference's gmin(j,k) after setup
    state0 = dict(f_nt=el["f_nt"].reshape(cells + (abi.NUM_NT,)), Pnt=el["Pnt"].reshape(cells + (abi.NUM_NT,)),
                  tea=med["tea"].copy(), n_e=med["n_e"].copy(), gmin=el["gmin"].reshape(cells),
                  gmax=med["gmax"].copy(), amxwl=med["amxwl"].copy(), p_nth=med["p_nth"].copy())
    fixed = dict(tna=med["tna"].copy(), B_field=med["B"].copy(), f_pair=np.zeros(cells),
                 turb_lev=med["turb_lev"].copy(), vol=vol, zsurf=zs)
    fp_const = abi.FpConstants(F_IC=F_IC, pair_switch=int(deck["pair_switch"]),
                               **{k: deck[k] for k in synth.FP_CONST_KEYS})
    desc = ("deck: %dx%d (z,r) grid, %d volume packets/step, FP on, run setup %s, splits %s"
            % (nz, nr, sources, setup,
               "/".join(str(deck[k]) for k in ("split1", "split2", "split3", "spl3_trg"))))
    return synth.CoupledWorkload(grid, deck, 2 * int(sources), dt, state0, fixed, fp_const, desc)
