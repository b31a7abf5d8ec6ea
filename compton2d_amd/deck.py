"""Input decks of the reference, and coupled workloads started from them.

`read_deck` parses a run directory's `input/input.dat` and every
`input/input_JJ_KK.dat` (fixed columns: label in 1-80, value from column 81;
field order of src/reader.f:157-657) into the keys of `synth.C3_DECK`, the
zone medium as [nz, nr] arrays.  It is the inverse of the test helper
`refcase.write_input_deck`.  A deck has `ntime` boundary time windows
(src/reader.f:169-283): `windows` lists them (t0, t1 and per ring tbbu, tbbl
and the two file names), the scalar keys t0, t1, tbbu, tbbl and spec_file
describe window 1.  The external-Compton constants R_blr, fr_blr, R_ir, fr_ir,
R_disk and d_jet (src/reader.f:581-586) come back under those names, and
`run_dir` is the directory that was read.

`deck_workload` builds a `synth.CoupledWorkload` from such a deck (or a dict
like `synth.C3_DECK`, whose medium scalars stand for every zone and whose
scalar boundary keys mean one window).  A ring with tbbu < 0 or tbbl < 0 in
any window is an external-Compton ring: `deck_boundary` builds one
`surface.file_sp` table per distinct seed file and hangs the windows, tables
and per-ring table indices on the workload as `boundary`
(`surface.Boundary`; None for a deck without such rings), from which
`coupled.CoupledRun` takes every step's surface sources.  Planck rings
(tbb > 0), star_switch and nmu > 1 are refused.  Unlike
`synth.c3_workload`, which starts every zone from the one medium shipped in
data/medium_inputm.npz, the initial electron spectra and the IC-loss table
come from the run-setup calls (csrc/setup.hip): gam_min + P_nontherm per zone
and IC_loss, on the GPU or on the host.

A deck says nothing about the size of the census: the reference stops at
ucens records a rank (src/imctrk2d.f:573-577).  A long deck run on a card it
would fill passes `coupled.CoupledRun` a `popcontrol.CensusControl`
(`census_control=`), which bounds the census with the weight-window roulette.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

from . import abi, engine, surface, synth

MEDIUM_KEYS = ("tea", "tna", "n_e", "B", "amxwl", "gmin", "gmax", "p_nth", "q_turb", "turb_lev")
EC_KEYS = ("R_blr", "fr_blr", "R_ir", "fr_ir", "R_disk", "d_jet")
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
    k = {"run_dir": str(d)}
    k["nz"], k["nr"] = L.int(), L.int()
    nz, nr = k["nz"], k["nr"]
    k["zmax"], k["rmin"], k["rmax"] = L.float(), L.float(), L.float()
    if L.int() != 0:
        raise ValueError("read_deck: star_switch != 0 is not supported")
    k["tstop"], k["mcdt"] = L.float(), L.float()
    ntime = L.int()
    if ntime < 1:
        raise ValueError("read_deck: ntime = %d: at least one boundary time window" % ntime)
    # per window t0, t1 and per ring tbbu, a name line, tbbl, a name line; the
    # name line is always there, the reference keeps it only for tbb < 0
    # (src/reader.f:222-247)
    k["windows"] = []
    for _ in range(ntime):
        w = dict(t0=L.float(), t1=L.float(), tbbu=[], tbbl=[], file_u=[], file_l=[])
        for _ in range(nr):
            w["tbbu"].append(L.float())
            w["file_u"].append(L.str())
            w["tbbl"].append(L.float())
            w["file_l"].append(L.str())
        k["windows"].append(w)
    # the scalar keys describe window 1
    w = k["windows"][0]
    k["t0"], k["t1"] = w["t0"], w["t1"]
    tbbu, tbbl = w["tbbu"], w["tbbl"]
    # one value when every ring has the same, else the list (refcase.write_input_deck takes both)
    k["tbbu"] = tbbu[0] if len(set(tbbu)) == 1 else list(tbbu)
    k["tbbl"] = tbbl[0] if len(set(tbbl)) == 1 else list(tbbl)
    k["spec_file"] = w["file_u"][0]
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
    for nm in EC_KEYS:          # src/reader.f:581-586
        k[nm] = L.float()
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


def deck_windows(deck: dict) -> list:
    """The boundary time windows of a deck; a dict without `windows` (such as
    synth.C3_DECK) means one window built from its scalar keys."""
    if "windows" in deck:
        return deck["windows"]
    nr = deck["nr"]
    ring = lambda v: [float(x) for x in np.broadcast_to(np.asarray(v, dtype=np.float64), (nr,))]
    name = deck.get("spec_file", "")
    return [dict(t0=deck["t0"], t1=deck["t1"], tbbu=ring(deck["tbbu"]), tbbl=ring(deck["tbbl"]),
                 file_u=[name] * nr, file_l=[name] * nr)]


SEED_COLUMNS = ("E", "L_disk", "F_blr", "F_ir")
TABLE_COLUMNS = ("E_file", "a1", "I_file", "F_file", "P_file")


def seed_columns(name: str, run_dir=None) -> np.ndarray:
    """The seed file a deck names: run_dir/<name>, run_dir/input/<name>, then
    the shipped data/ec_seed_spectra.npz by the name's stem."""
    name = name.strip()
    if run_dir is not None:
        for p in (Path(run_dir) / name, Path(run_dir) / "input" / name):
            if p.is_file():
                return surface.read_seed_columns(p)
    try:
        return surface.seed_spectrum(Path(name).stem)
    except KeyError:
        raise ValueError("deck_workload: seed file '%s' is neither in the run directory (%s) nor "
                         "among the shipped seed spectra" % (name, run_dir)) from None


def seed_table(name: str, cols: np.ndarray, ec: surface.EcConstants):
    """file_sp of one seed file; a non-finite entry of the file or of the
    table is an error (hazard H9: the reference's disk/blackbody.in holds a
    NaN column, and its run hangs on the NaN table)."""
    for i, col in enumerate(SEED_COLUMNS):
        if not np.isfinite(cols[:, i]).all():
            raise ValueError("deck_workload: seed file '%s': non-finite entry in column %d (%s)"
                             % (name, i + 1, col))
    try:
        tab, int_file = surface.file_sp(cols, ec)
    except (ValueError, ZeroDivisionError, OverflowError) as e:
        raise ValueError("deck_workload: seed file '%s': %s" % (name, e)) from None
    for col in TABLE_COLUMNS:
        if not np.isfinite(getattr(tab, col)).all():
            raise ValueError("deck_workload: seed file '%s': non-finite entry in table column %s"
                             % (name, col))
    if not np.isfinite(int_file):
        raise ValueError("deck_workload: seed file '%s': non-finite integral" % name)
    return tab, int_file


def deck_boundary(deck: dict, r: np.ndarray):
    """The surface.Boundary of a deck, or None when no ring has a source.  A
    ring with tbbu < 0 or tbbl < 0 in any window is an external-Compton ring:
    its packets draw from the file the deck names.  A Planck ring (tbb > 0) is
    refused: the reference gives it energy but no packets
    (src/imcgen2d.f:436-437), so driving the deck would silently drop it."""
    nz, nr = deck["nz"], deck["nr"]
    windows = deck_windows(deck)
    tbbu = np.array([w["tbbu"] for w in windows], dtype=np.float64).reshape(len(windows), nr)
    tbbl = np.array([w["tbbl"] for w in windows], dtype=np.float64).reshape(len(windows), nr)
    if np.any(tbbu > 0.0) or np.any(tbbl > 0.0):
        raise ValueError("deck_workload: blackbody boundary rings (tbbu / tbbl > 0) are not driven")
    if not (np.any(tbbu < 0.0) or np.any(tbbl < 0.0)):
        return None
    defaults = surface.EcConstants()
    ec = surface.EcConstants(g_bulk=deck["g_bulk"],
                             **{k: deck.get(k, getattr(defaults, k)) for k in EC_KEYS})
    files, tables, ints = [], [], []
    spec = {}
    for side, tbb in (("file_u", tbbu), ("file_l", tbbl)):
        spec[side] = np.full(tbb.shape, -1, np.int32)
        for t, w in enumerate(windows):
            for k in range(nr):
                if tbb[t, k] < 0.0:
                    name = w[side][k].strip()
                    if name not in files:
                        tab, int_file = seed_table(name, seed_columns(name, deck.get("run_dir")), ec)
                        files.append(name)
                        tables.append(tab)
                        ints.append(int_file)
                    spec[side][t, k] = files.index(name)
    return surface.Boundary(nz=nz, r=np.array(r, dtype=np.float64), rmin=float(deck["rmin"]),
                            t0=np.array([w["t0"] for w in windows], dtype=np.float64),
                            t1=np.array([w["t1"] for w in windows], dtype=np.float64),
                            tbbu=tbbu, tbbl=tbbl, spec_u=spec["file_u"], spec_l=spec["file_l"],
                            files=files, tables=tables, int_file=ints)


def deck_workload(deck: dict, sources: int, setup: str = "device",
                  comtot_mode: int = abi.COMTOT_TABLE, rank: int = 0, world: int = 1, device: int = 0,
                  seed: int = 0x5EEDC2D, census_capacity: int | None = None,
                  event_capacity: int | None = None) -> synth.CoupledWorkload:
    """A T_const = 0 workload of `deck` with `sources` volume packets per step
    (nst = 2*sources, src/imcgen2d.f:448).  setup: "device" (the setup
    kernels on GPU `device`), "host-det" (their host twin, the same bits) or
    "host-libm" (the host with the C library's log/exp/pow, the reference's
    bits).  A deck with external-Compton rings gives the workload its
    `boundary` (deck_boundary); ValueError for a Planck ring, nmu != 1, a seed
    file that is not found or a seed table with a non-finite entry."""
    if setup not in SETUPS:
        raise ValueError("deck_workload: setup must be one of %s" % (SETUPS,))
    if deck["nmu"] != 1:
        raise ValueError("deck_workload: one angular bin only (nmu = %d)" % deck["nmu"])
    nz, nr = deck["nz"], deck["nr"]
    z, r, vol, zs = synth.zone_geometry(nz, nr, deck["zmax"], deck["rmin"], deck["rmax"])
    boundary = deck_boundary(deck, r)
    med = {k: _zones(deck, k) for k in MEDIUM_KEYS}
    gnt, E_field, E_ph = abi.setup_grids()
    ins = [med[k] for k in ("tea", "amxwl", "gmin", "gmax", "p_nth")]
    if setup == "device":
        el = engine.setup_electrons(*ins, device=device)
        F_IC = engine.ic_loss(gnt, E_field, device=device)
    else:
        el = abi.setup_electrons_host(*ins, libm=setup == "host-libm")
        F_IC = abi.ic_loss_host(gnt, E_field, libm=setup == "host-libm")

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
    if boundary is not None:
        desc += ", EC rings from %s in %d window(s)" % (", ".join(boundary.files), len(boundary.t1))
    return synth.CoupledWorkload(grid, deck, 2 * int(sources), dt, state0, fixed, fp_const, desc,
                                 boundary=boundary)
