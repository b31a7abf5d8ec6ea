"""Run setup on the host (csrc/setup_host.h through c2d_setup_grids,
c2d_ic_loss_host, c2d_setup_electrons_host) against the reference's dumps,
and compton2d_amd.deck.read_deck.

* F_IC, libm flavour: bit for bit tests/golden/fp_fic.npz (the reference's
  IC_loss on the standard grids), negative cancellation entries included.
* F_IC, det flavour (c2d_log, what the GPU runs): differs only through log's
  last ulp; max relative difference <= 1e-9, Thomson-branch entries equal.
* grids: bit-equal to data/medium_inputm.npz and synth.field_grid().
* electrons, libm flavour: f_nt, Pnt bit for bit tests/golden/setup.npz on all
  16 media (glibc's pow matches flang's here: no residue), gmin of the mixed
  media equal to the reference's fpin_001.bin.  p_nth = 1 gives NaN in the
  reference (0/0 in P_nontherm) and here: the NaN positions must agree.
* electrons, det flavour: max relative difference measured 5.4e-15 on this
  CPU, pinned at 6e-15.
"""
import math
import shutil
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

import refcase
from compton2d_amd import abi, deck, engine, synth

GOLD = Path(__file__).resolve().parent / "golden"
IN_KEYS = ("tea", "amxwl", "gmin", "gmax", "p_nth")


def bits_equal(a, b):
    """Equal bit for bit; a NaN equals a NaN (x86 and gfx950 give 0/0 different signs)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    nan = np.isnan(a)
    return (a.shape == b.shape and np.array_equal(nan, np.isnan(b))
            and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


@pytest.fixture(scope="module")
def grids():
    return abi.setup_grids()


@pytest.fixture(scope="module")
def fic(grids):
    """(golden, libm, det) F_IC on the standard grids; the two host tables at once."""
    gnt, E_field, _ = grids
    with ThreadPoolExecutor(2) as ex:
        a = ex.submit(abi.ic_loss_host, gnt, E_field, True)
        b = ex.submit(abi.ic_loss_host, gnt, E_field, False)
        libm, det = a.result(), b.result()
    with np.load(GOLD / "fp_fic.npz", allow_pickle=False) as z:
        gold = z["F_IC"].copy()
    return gold, libm, det


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD / "setup.npz", allow_pickle=False) as z:
        return {k: z[k].copy() for k in z.files}


def test_grids_bitwise(grids):
    gnt, E_field, E_ph = grids
    with np.load(synth.DATA, allow_pickle=False) as med:
        assert bits_equal(gnt, med["gnt"])
        assert bits_equal(E_ph, med["E_ph"])
    assert bits_equal(E_field, synth.field_grid())
    # any pointer may be null
    lib = engine.load_library()
    g2 = np.zeros(abi.NUM_NT)
    assert lib.c2d_setup_grids(g2.ctypes.data_as(abi.PD), None, None) == 0
    assert bits_equal(g2, gnt)


def test_ic_loss_libm_is_the_reference_bit_for_bit(fic):
    g, libm, _ = fic
    assert (g < 0).sum() == 15430          # cancellation garbage, reproduced, not repaired
    assert np.array_equal(libm.view(np.uint64), g.view(np.uint64))


def test_ic_loss_det_differs_through_log_only(fic, grids):
    g, _, det = fic
    gnt, E_field, _ = grids
    thomson = (1.0 + gnt)[:, None] * (1.957e-3 * E_field)[None, :] < 1.0e-2
    assert (~thomson).sum() == 50854
    assert np.array_equal(det[thomson].view(np.uint64), g[thomson].view(np.uint64))
    rel = np.abs(det - g) / np.abs(g)
    print("det vs golden: %d entries differ, max rel %.3e" % ((det != g).sum(), rel.max()))
    assert rel.max() <= 1e-9


def test_ic_loss_host_strides_and_small_grids(grids):
    gnt, E_field, _ = grids
    rows, cols = gnt[[0, 120]], E_field[150:250:7]
    a = abi.ic_loss_host(rows, cols, True)
    f = abi.ic_loss_host(rows, cols, True, fortran=True)
    assert f.flags.f_contiguous and np.array_equal(a, f)
    one = abi.ic_loss_host(rows[:1], cols[:1], True)
    assert one.shape == (1, 1) and one[0, 0] == a[0, 0]


def _ic_host(gnt, n_el, E_field, n_ph, out=True, libm=1):
    lib = engine.load_library()
    F = np.zeros((max(n_el, 1), max(n_ph, 1)))
    p = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(abi.PD)
    return lib.c2d_ic_loss_host(p(gnt), n_el, p(E_field), n_ph, F.ctypes.data_as(abi.PD) if out else None,
                                max(n_ph, 1), 1, libm)


def test_ic_loss_host_argument_errors():
    g, e = np.array([1.0, 2.0]), np.array([1.0, 2.0, 3.0])
    assert _ic_host(g, 2, e, 3) == 0
    assert _ic_host(None, 2, e, 3) == abi.C2D_E_ARG
    assert _ic_host(g, 2, None, 3) == abi.C2D_E_ARG
    assert _ic_host(g, 2, e, 3, out=False) == abi.C2D_E_ARG
    assert _ic_host(g, 0, e, 3) == abi.C2D_E_ARG
    assert _ic_host(g, 2, e, 0) == abi.C2D_E_ARG
    assert _ic_host(np.ones(201), 201, e, 3) == abi.C2D_E_ARG
    assert _ic_host(g, 2, np.ones(401), 401) == abi.C2D_E_ARG
    assert _ic_host(np.array([1.0, 0.0]), 2, e, 3) == abi.C2D_E_ARG
    assert _ic_host(g, 2, np.array([1.0, -2.0, 3.0]), 3) == abi.C2D_E_ARG
    assert _ic_host(np.array([1.0, math.nan]), 2, e, 3) == abi.C2D_E_NONFINITE
    assert _ic_host(g, 2, np.array([1.0, math.inf, 3.0]), 3) == abi.C2D_E_NONFINITE


def test_electrons_libm_is_the_reference_bit_for_bit(gold):
    o = abi.setup_electrons_host(*[gold[k] for k in IN_KEYS], libm=True)
    assert bits_equal(gold["gnt"], abi.setup_grids()[0])
    for z in range(16):
        for k in ("f_nt", "Pnt"):
            assert bits_equal(o[k][z], gold[k][z]), (z, k)
    assert np.isnan(gold["f_nt"][2]).all()             # p_nth = 1: 0/0 in P_nontherm
    assert not np.isnan(np.delete(gold["f_nt"], 2, axis=0)).any()
    with np.load(synth.DATA, allow_pickle=False) as med:
        assert bits_equal(o["f_nt"][0], med["f_nt"]) and bits_equal(o["Pnt"][0], med["Pnt"])
    # gam_min's gmin where it is adjusted: the two mixed media, from the reference's fpin_001.bin
    assert bits_equal(o["gmin"][gold["mixed_zones"]], gold["mixed_gmin"])
    # ... and by hand elsewhere
    assert o["gmin"][0] == 100.0 and o["gmin"][1] == 1.01
    assert o["gmin"][6] == 1.0 + 1.0e2 * (50.0 / 511.0) and o["N_nth"][6] == 1.0e-20
    assert o["N_nth"][7] == 1.0e-20                     # 0.999999995 > 0.99999999d0: thermal in gam_min
    assert gold["f_nt"][7][150] > 0.0                   # ... but < the REAL 0.99999999: a power law in P_nontherm
    assert o["gmin"][12] == 10.0                        # tea < 1: not divided by 1.01


def test_electrons_det_within_measured_bound(gold):
    o = abi.setup_electrons_host(*[gold[k] for k in IN_KEYS], libm=False)
    l = abi.setup_electrons_host(*[gold[k] for k in IN_KEYS], libm=True)
    worst = 0.0
    for k in ("f_nt", "Pnt"):
        ok = ~np.isnan(gold[k])
        assert np.array_equal(np.isnan(o[k]), ~ok)
        nz = ok & (gold[k] != 0.0)
        assert np.array_equal(o[k][ok & ~nz], gold[k][ok & ~nz])
        worst = max(worst, float(np.max(np.abs(o[k][nz] - gold[k][nz]) / np.abs(gold[k][nz]))))
    print("det vs golden: max rel %.3e" % worst)
    assert worst <= 6e-15
    assert bits_equal(o["gmin"], l["gmin"])             # divisions and comparisons only
    for k in ("N_nth", "gbar_nth"):
        np.testing.assert_allclose(o[k], l[k], rtol=1e-12)


def _el_host(n, arrs, outs=True, null_in=None):
    lib = engine.load_library()
    ins = [np.ascontiguousarray(a, np.float64) for a in arrs]
    m = max(int(n), 1)
    out = [np.zeros(m), np.zeros(m), np.zeros(m), np.zeros((m, abi.NUM_NT)), np.zeros((m, abi.NUM_NT))]
    pi = [None if null_in == i else a.ctypes.data_as(abi.PD) for i, a in enumerate(ins)]
    po = [a.ctypes.data_as(abi.PD) if outs else None for a in out]
    return lib.c2d_setup_electrons_host(n, *pi, *po, 1)


def test_electrons_host_argument_errors():
    ok = [np.array([100.0]), np.array([0.0]), np.array([100.0]), np.array([1e5]), np.array([2.3])]
    assert _el_host(1, ok) == 0
    assert _el_host(0, ok) == abi.C2D_E_ARG
    assert _el_host(99 * 99 + 1, ok) == abi.C2D_E_ARG
    assert _el_host(1, ok, outs=False) == abi.C2D_E_ARG
    assert _el_host(1, ok, null_in=3) == abi.C2D_E_ARG
    for i in (0, 2, 3):                                  # tea, gmin, gmax must be positive
        bad = [a.copy() for a in ok]
        bad[i][0] = 0.0
        assert _el_host(1, bad) == abi.C2D_E_ARG
    for i in range(5):
        bad = [a.copy() for a in ok]
        bad[i][0] = math.nan
        assert _el_host(1, bad) == abi.C2D_E_NONFINITE


def _per_zone_deck(tmp_path):
    case = dict(nz=3, nr=2, nst=4000, T_const=0, pair_switch=1, tstop=2.0e6)
    refcase.write_input_deck(tmp_path, case)
    rng = np.random.default_rng(5)
    med = {}
    for k, (lo, hi) in dict(tea=(1.0, 500.0), tna=(1.0, 500.0), n_e=(1.0, 1e3), B=(0.01, 1.0), amxwl=(0.0, 1.0),
                            gmin=(1.0, 100.0), gmax=(1e3, 1e6), p_nth=(1.5, 3.5), q_turb=(1.0, 2.0),
                            turb_lev=(1e-20, 1e-3)).items():
        med[k] = np.array([float("%.7E" % v) for v in rng.uniform(lo, hi, 6)]).reshape(3, 2)
    for j in range(3):
        for k in range(2):
            rows = [("tea", med["tea"][j, k]), ("tna", med["tna"][j, k]), ("n_e", med["n_e"][j, k]),
                    ("ep_switch", 0), ("B_field", med["B"][j, k]), ("amxwl", med["amxwl"][j, k]),
                    ("gmin", med["gmin"][j, k]), ("gmax", med["gmax"][j, k]), ("p_nth", med["p_nth"][j, k]),
                    ("q_turb", med["q_turb"][j, k]), ("turb_lev", med["turb_lev"][j, k])]
            (tmp_path / "input" / ("input_%02d_%02d.dat" % (j + 1, k + 1))).write_text(
                "".join(refcase._line(nm, float(v) if nm != "ep_switch" else v) for nm, v in rows))
    return case, med


def test_read_deck_round_trips_a_written_deck(tmp_path):
    case, med = _per_zone_deck(tmp_path)
    d = deck.read_deck(tmp_path)
    want = dict(refcase.BASE_CASE)
    want.update(case)
    for k in synth.C3_DECK:
        if k in deck.MEDIUM_KEYS:
            assert d[k].shape == (3, 2) and np.array_equal(d[k], med[k]), k
        elif k in want:
            assert d[k] == want[k], k
    assert set(synth.C3_DECK) <= set(d)
    assert d["ep_switch"].shape == (3, 2) and not d["ep_switch"].any()


def test_read_deck_parses_the_reference_c3_deck(tmp_path):
    src = refcase.REFERENCE / "src_20121026"
    if not (src / "input.dat").exists():
        pytest.skip("the reference's decks are not on this machine")
    (tmp_path / "input").mkdir()
    shutil.copy(src / "input.dat", tmp_path / "input" / "input.dat")
    for j in range(30):
        for k in range(9):
            shutil.copy(src / "inputm.dat", tmp_path / "input" / ("input_%02d_%02d.dat" % (j + 1, k + 1)))
    d = deck.read_deck(tmp_path)
    # synth.C3_DECK's documented deviations from the deck: splits, rand_switch (nst is the deck's)
    deviations = dict(split1=1000, split2=1000, split3=300, spl3_trg=10, rand_switch=2, nst=800000)
    for k, v in synth.C3_DECK.items():
        if k in deck.MEDIUM_KEYS:
            assert d[k].shape == (30, 9) and np.all(d[k] == v), k
        else:
            assert d[k] == deviations.get(k, v), k


def test_deck_workload_rejects_what_the_coupled_run_does_not_drive():
    with pytest.raises(ValueError):
        deck.deck_workload(dict(synth.C3_DECK, nmu=2), 1000, setup="host-libm")
    with pytest.raises(ValueError):
        deck.deck_workload(dict(synth.C3_DECK, tbbu=1.0), 1000, setup="host-libm")
    with pytest.raises(ValueError):
        deck.deck_workload(dict(synth.C3_DECK, tbbl=[0.0] * 8 + [2.0]), 1000, setup="host-libm")
    with pytest.raises(ValueError):
        deck.deck_workload(synth.C3_DECK, 1000, setup="gpu")


@pytest.mark.parametrize("medium", [(300.0, 0.3, 50.0, 1.0e5, 1.8), (5.0, 0.5, 10.0, 1.0e4, 2.3)])
def test_header_as_c99_under_host_sanitizers(tmp_path, grids, medium):
    """csrc/setup_host.h compiled as C99 by gcc into a program of its own, with
    ASan + UBSan: the same bits as the library's (hipcc) build of the header,
    in both flavours."""
    import subprocess
    from fmt_cases import GCC_FLAGS
    src = Path(__file__).resolve().parent / "c" / "setup_main.c"
    exe = tmp_path / "setup_main"
    subprocess.run(["gcc", "-O1", "-g", "-ffp-contract=off"] + GCC_FLAGS +
                   ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=undefined", "-o", str(exe), str(src), "-lm"], check=True)
    p = subprocess.run([str(exe)] + [repr(v) for v in medium], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array([int(x, 16) for x in p.stdout.split()], dtype=np.uint64).view(np.float64)
    gnt, E_field, _ = grids
    want = []
    for libm in (True, False):
        want.append(abi.ic_loss_host(gnt[[0, 120, 199]], E_field[150:390:30], libm).reshape(-1))
        o = abi.setup_electrons_host(*[[v] for v in medium], libm=libm)
        want += [o["gmin"], o["N_nth"], o["gbar_nth"], o["f_nt"][0], o["Pnt"][0]]
    assert bits_equal(got, np.concatenate(want))
