"""Decks with external-Compton boundary rings and several time windows, on the
host: read_deck (windows, file names, the EC constants of src/reader.f:581-586),
deck_workload (which rings it drives, where it finds the seed files) and
surface.step_surfaces, the per-step surface fields of the coupled run, against
a hand composition of the pinned pieces (time_window, ring_budget, file_sp,
apply_bias) and against the budgets the reference itself dumped for the golden
case ec_lower."""
import dataclasses

import numpy as np
import pytest

import ec_deck as D
import refcase
from compton2d_amd import abi, deck, surface as S, synth
from golden_io import GoldenCase

SURFACE_FIELDS = ("nsurfi", "nsurfo", "ewsurfi", "ewsurfo", "nsurfu", "nsurfl", "ewsurfu", "ewsurfl",
                  "tbbi", "tbbo", "tbbu", "tbbl")
NST = D.CASE["nst"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_fields(got: abi.StepInputs, want: abi.StepInputs, what):
    for k in SURFACE_FIELDS + ("nsv", "ewsv"):
        g, w = np.asarray(getattr(got, k)), np.asarray(getattr(want, k))
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        np.testing.assert_array_equal(bits(g), bits(w), err_msg="%s %s" % (what, k))
    assert len(got.spectra) == len(want.spectra)
    for a, b in zip(got.spectra, want.spectra):
        for col in ("E_file", "a1", "I_file", "F_file", "P_file"):
            np.testing.assert_array_equal(bits(getattr(a, col)), bits(getattr(b, col)), err_msg=col)


# ------------------------------------------------------------------ 1. read_deck
def test_read_deck_returns_the_windows_and_the_ec_constants(tmp_path):
    wins = [D.window(0.0, 2.25 * D.DT, tbbu=[0.0, -2.0], tbbl=-1.0, file_u=["a.in", "upper.in"],
                     file_l=[D.SEED_FILE, "other.in"]),
            D.window(3.0e5, 1.0e30, tbbl=[-1.0, 0.0], file_l=["late.in", "unused.in"])]
    D.write_deck(tmp_path, wins)
    d = deck.read_deck(tmp_path)
    assert len(d["windows"]) == 2
    for got, w in zip(d["windows"], wins):
        assert set(got) == {"t0", "t1", "tbbu", "tbbl", "file_u", "file_l"}
        assert got["t0"] == D.deck_float(w["t0"]) and got["t1"] == D.deck_float(w["t1"])
        assert list(got["tbbu"]) == w["tbbu"] and list(got["tbbl"]) == w["tbbl"]
        assert list(got["file_u"]) == w["file_u"] and list(got["file_l"]) == w["file_l"]
    for k, v in D.EC_CONST.items():
        assert d[k] == v, k
    assert d["run_dir"] == str(tmp_path)
    # the scalar keys describe window 1
    assert d["t0"] == 0.0 and d["t1"] == D.deck_float(2.25 * D.DT)
    assert d["tbbu"] == [0.0, -2.0] and d["tbbl"] == -1.0 and d["spec_file"] == "a.in"
    assert d["nst"] == NST and d["g_bulk"] == 25.0 and d["T_const"] == 0


def test_read_deck_of_one_window_keeps_its_keys(tmp_path):
    case = dict(nz=3, nr=2, nst=4000, T_const=0, tbbl=[0.0, -1.0], t0=1.0, t1=5.0e5)
    refcase.write_input_deck(tmp_path, case)
    d = deck.read_deck(tmp_path)
    want = dict(refcase.BASE_CASE, **case)
    for k in synth.C3_DECK:
        if k in deck.MEDIUM_KEYS:
            assert d[k].shape == (3, 2) and np.all(d[k] == want[k]), k
        else:
            assert d[k] == want[k], k
    assert set(synth.C3_DECK) <= set(d)
    (w,) = d["windows"]
    assert (w["t0"], w["t1"], w["tbbu"], w["tbbl"]) == (1.0, 5.0e5, [0.0, 0.0], [0.0, -1.0])
    assert w["file_u"] == w["file_l"] == [want["spec_file"]] * 2


def test_read_deck_still_rejects_a_star(tmp_path):
    D.write_deck(tmp_path, D.ec_windows())
    p = tmp_path / "input" / "input.dat"
    rows = p.read_text().splitlines(True)
    assert rows[5].startswith("star_switch")
    rows[5] = D._line("star_switch", 1)
    p.write_text("".join(rows))
    with pytest.raises(ValueError, match="star_switch"):
        deck.read_deck(tmp_path)


# -------------------------------------------------------------- 2. deck_workload
def ec_workload(tmp_path, windows=None, **over):
    D.write_deck(tmp_path, D.ec_windows() if windows is None else windows, **over)
    d = deck.read_deck(tmp_path)
    return d, deck.deck_workload(d, d["nst"] // 2, setup="host-libm")


def ec_boundary(run_dir):
    """The boundary alone: what deck_workload builds before the (slow, host) run setup."""
    d = deck.read_deck(run_dir)
    _, r, _, _ = synth.zone_geometry(d["nz"], d["nr"], d["zmax"], d["rmin"], d["rmax"])
    return deck.deck_boundary(d, r)


def test_deck_workload_accepts_ec_rings(tmp_path):
    d, wl = ec_workload(tmp_path)
    b = wl.boundary
    assert wl.nst == NST and wl.dt == D.DT and b is not None
    assert b.files == [D.SEED_FILE] and len(b.tables) == 1 and b.nz == 2
    np.testing.assert_array_equal(b.spec_l, [[0, 0], [-1, -1]])
    np.testing.assert_array_equal(b.spec_u, [[-1, -1], [-1, -1]])
    np.testing.assert_array_equal(b.tbbl, [[-1.0, -1.0], [0.0, 0.0]])
    np.testing.assert_array_equal(b.t1, [D.deck_float(2.25 * D.DT), 1.0e30])
    np.testing.assert_array_equal(b.r, wl.grid.r)
    tab, int_file = S.file_sp(S.seed_spectrum("blackbody_G25_4spectra"), S.EcConstants(g_bulk=25.0, **D.EC_CONST))
    assert b.int_file == [int_file]
    np.testing.assert_array_equal(bits(b.tables[0].P_file), bits(tab.P_file))
    # a deck without boundary sources has no boundary, as before
    assert deck.deck_boundary(synth.C3_DECK, np.linspace(1.0, 9.0, 9)) is None
    assert synth.c3_workload(sources=100).boundary is None


def test_deck_workload_rejects_what_is_not_driven(tmp_path):
    for name, wins, over in (("planck", [D.window(0.0, 1e30, tbbl=[-1.0, 2.0], file_l=D.SEED_FILE)], {}),
                             ("planck2", D.ec_windows()[:1] + [D.window(0.0, 1e30, tbbu=0.5)], {}),
                             ("nmu", D.ec_windows(), dict(nmu=2)),
                             ("missing", D.ec_windows(file_l="no_such_seed.in"), {})):
        with pytest.raises(ValueError):
            ec_workload(tmp_path / name, wins, **over)
    with pytest.raises(ValueError, match="no_such_seed.in"):
        deck.deck_workload(dict(synth.C3_DECK, tbbl=-1.0, spec_file="no_such_seed.in"), 100, setup="host-libm")


def test_seed_files_are_found_in_the_run_directory_first(tmp_path):
    cols = S.seed_spectrum("blackbody_20110929")
    text = "".join(" ".join("%.17E" % v for v in row) + "\n" for row in cols)
    for sub in ("", "input"):
        d = tmp_path / ("in_" + sub)
        D.write_deck(d, D.ec_windows(file_l="own.in"))
        (d / sub / "own.in").write_text(text)
        want, _ = S.file_sp(cols, S.EcConstants(g_bulk=25.0, **D.EC_CONST))
        np.testing.assert_array_equal(bits(ec_boundary(d).tables[0].F_file), bits(want.F_file))
    # the run directory's file wins over the shipped one of the same name
    d = tmp_path / "shadow"
    D.write_deck(d, D.ec_windows())
    (d / D.SEED_FILE).write_text(text)
    np.testing.assert_array_equal(bits(ec_boundary(d).tables[0].F_file), bits(want.F_file))


def test_a_non_finite_seed_table_is_refused(tmp_path):
    """Hazard H9: the reference's disk/blackbody.in holds a NaN in its third column."""
    cols = S.seed_spectrum("blackbody_20110929")
    rows = [" ".join("%.17E" % v for v in row) for row in cols]
    rows[3] = " ".join(rows[3].split()[:2] + ["NaN"] + rows[3].split()[3:])
    D.write_deck(tmp_path, D.ec_windows(file_l="nan.in"))
    (tmp_path / "nan.in").write_text("\n".join(rows) + "\n")
    with pytest.raises(ValueError, match=r"nan\.in.*column 3 \(F_blr\)"):
        deck.deck_workload(deck.read_deck(tmp_path), NST // 2, setup="host-libm")


# -------------------------------------------------------------- 3. step_surfaces
def hand_step(base, windows, n, nsv, ec):
    """Step n of the deck composed by hand from the pinned pieces."""
    tab, int_file = S.file_sp(S.seed_spectrum("blackbody_G25_4spectra"), ec)
    r, rmin = np.asarray(base_grid().r, float), 0.0
    t1 = [D.deck_float(w["t1"]) for w in windows]
    t0 = [D.deck_float(w["t0"]) for w in windows]
    ncycle, t = n, max(n - 1, 0) * D.DT
    w = S.time_window(ncycle, t, D.DT, t1)
    zr, izr = np.zeros(2), np.zeros(2, np.int32)
    if w < len(windows):
        ec_on = t + 0.5 * D.DT >= t0[w]
        tbbl = np.array(windows[w]["tbbl"])
        ns, ew, _ = S.ring_budget(r, rmin, NST, D.DT, tbbl, ec_on, int_file)
        spec_l = np.where(tbbl < 0.0, 0, -1).astype(np.int32)
    else:
        ec_on, tbbl, ns, ew, spec_l = False, zr, izr, zr, np.full(2, -1, np.int32)
    si = dataclasses.replace(base, ncycle=ncycle, time=t, dt=D.DT, nsv=nsv.copy(), nsurfi=izr, nsurfo=izr,
                             ewsurfi=zr, ewsurfo=zr, nsurfu=izr, ewsurfu=zr, nsurfl=ns, ewsurfl=ew, tbbi=zr,
                             tbbo=zr, tbbu=zr, tbbl=tbbl, spectra=[tab], spec_l=spec_l,
                             spec_u=np.full(2, -1, np.int32))
    fb = S.apply_bias(NST, si)
    return si, w, ec_on, fb


def base_grid():
    return GoldenCase("ec_lower").grid()


def surfaces_step(base, b, n, nsv):
    ncycle, t = n, max(n - 1, 0) * D.DT
    f, w, ec_on = S.step_surfaces(b, b.r, b.rmin, NST, ncycle, t, D.DT)
    si = dataclasses.replace(base, ncycle=ncycle, time=t, dt=D.DT, nsv=nsv.copy(), **f)
    return si, w, ec_on, S.apply_bias(NST, si)


@pytest.mark.parametrize("variant", ["deck", "late gate", "windows run out"])
@pytest.mark.parametrize("volume", [NST // 2, 40 * NST])
def test_step_surfaces_equals_the_hand_composition(tmp_path, variant, volume):
    """volume: the step's volume packets; 40 nst of them make the 10 nst cap bite."""
    wins = dict(deck=D.ec_windows(), **{"late gate": D.ec_windows(t0=0.75 * D.DT),
                                        "windows run out": D.ec_windows(t1_last=3.25 * D.DT)})[variant]
    D.write_deck(tmp_path, wins)
    b = ec_boundary(tmp_path)
    np.testing.assert_array_equal(b.r, base_grid().r)       # the grid of ec_lower
    base = GoldenCase("ec_lower").step_inputs(0)
    nsv = np.array([[volume // 4] * 2] * 2, np.int32)
    ec = S.EcConstants(g_bulk=25.0, **D.EC_CONST)
    seen = []
    for n in range(5):
        got, w, ec_on, fb = surfaces_step(base, b, n, nsv)
        want, w_h, ec_h, fb_h = hand_step(base, wins, n, nsv, ec)
        assert (w, ec_on, fb) == (w_h, ec_h, fb_h)
        same_fields(got, want, "step %d" % n)
        for k in ("spec_u", "spec_l"):
            np.testing.assert_array_equal(getattr(got, k), getattr(want, k))
        np.testing.assert_array_equal(got.spec_i, -1)
        np.testing.assert_array_equal(got.spec_o, -1)
        assert (fb < 1.0) == (volume > 10 * NST)
        seen.append((w, bool(ec_on), int(got.nsurfl.sum()) > 0))
    windows, gates, sources = zip(*seen)
    if variant == "deck":
        assert list(windows) == [0, 0, 0, 1, 1]
        assert list(gates) == [True] * 5 and list(sources) == [True] * 3 + [False] * 2
    elif variant == "late gate":
        # t + dt/2 = 0.5 dt at ncycle 0 and 1: the gate is closed and the rings
        # emit the blackbody energy of |tbb| = 1 (ring_budget's ec_on=False branch)
        assert list(windows) == [0, 0, 0, 1, 1] and list(gates)[:3] == [False, False, True]
        closed, _, _, _ = surfaces_step(base, b, 1, nsv * 0)
        A = S.ring_areas(b.r, 0.0)
        np.testing.assert_array_equal(closed.ewsurfl, D.DT * A * S.SIGMA_SB * 1.0 / closed.nsurfl)
        assert list(sources) == [True] * 3 + [False] * 2
    else:
        assert list(windows) == [0, 0, 0, 1, 2] and list(sources) == [True] * 3 + [False] * 2
        last, w, ec_on, _ = surfaces_step(base, b, 4, nsv)
        assert w == 2 and ec_on is False
        for k in SURFACE_FIELDS:
            assert not np.any(getattr(last, k)), k


# --------------------------------------------------- 4. the reference's own dump
def test_step_surfaces_reproduces_the_reference_budgets():
    """ec_lower: tbbl = -1 on both rings with disk/blackbody_20110929.in, one
    window, Gamma = 33; nsurfl / ewsurfl as imcgen2d left them in COMMON."""
    gc = GoldenCase("ec_lower")
    case = dict(refcase.BASE_CASE, **gc.meta["case"])
    b = deck.deck_boundary(case, gc.a["cfg_r"])
    assert b.files == ["blackbody_20110929.in"]
    for n in range(gc.nsteps):
        st, si = gc.meta["step%d" % n], gc.step_inputs(n)
        f, w, ec_on = S.step_surfaces(b, gc.a["cfg_r"], gc.meta["rmin"], case["nst"], st["ncycle"],
                                      st["time"], st["dt"])
        assert w == 0 and ec_on
        assert si.nsurfl.sum() > 0
        for k in ("nsurfl", "ewsurfl", "nsurfu", "ewsurfu", "tbbl", "tbbu"):
            np.testing.assert_array_equal(bits(f[k]), bits(np.asarray(getattr(si, k))), err_msg="step %d %s" % (n, k))
        np.testing.assert_array_equal(bits(f["spectra"][0].P_file), bits(gc.out(n, "P_file")[:len(f["spectra"][0].P_file)]))
