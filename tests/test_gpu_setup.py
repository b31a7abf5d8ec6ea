"""Run setup on the GPU (csrc/setup.hip: c2d_icloss_kernel, c2d_esetup_kernel)
against its host twin (the det flavour of csrc/setup_host.h), the reference's
tables, and through compton2d_amd.deck.deck_workload into a coupled run.

Device and det host run the same arithmetic with contraction off, so they are
compared through uint64 views: cancellation garbage and negative entries
count.  (A NaN counts as equal to a NaN: 0/0 has the sign bit set on x86-64
and clear on gfx950.)
"""
import math
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

from compton2d_amd import abi, deck, engine, synth
from compton2d_amd.coupled import CoupledRun
from compton2d_amd.engine import Engine
from test_setup_host import IN_KEYS, bits_equal

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def grids():
    return abi.setup_grids()


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD / "setup.npz", allow_pickle=False) as z:
        return {k: z[k].copy() for k in z.files}


@pytest.fixture(scope="module")
def full_device(grids):
    """The standard 200 x 400 table on the device, once."""
    gnt, E_field, _ = grids
    return engine.ic_loss(gnt, E_field)


def thomson_mask(gnt, E_field):
    return (1.0 + gnt)[:, None] * (1.957e-3 * E_field)[None, :] < 1.0e-2


def straddle_grid():
    """gamma*epsilon on both sides of 1e-2 within a few ulp."""
    gnt = np.array([0.2, 9.0, 3.0e4])
    E = []
    for g in 1.0 + gnt:
        e0 = 1.0e-2 / (g * 1.957e-3)
        for _ in range(4):
            e0 = np.nextafter(e0, 0.0)
        for _ in range(9):
            E.append(e0)
            e0 = np.nextafter(e0, np.inf)
    return gnt, np.array(E)


def small_grids(grids):
    gnt, E_field, _ = grids
    yield "1x1 series", gnt[100:101], E_field[300:301]
    yield "1x1 product", gnt[:1], E_field[:1]
    yield "3x70", gnt[[0, 120, 199]], E_field[100:380:4]
    yield "5x130", gnt[[0, 57, 120, 180, 199]], E_field[10::3]
    yield "all product", gnt[0:60:20], E_field[::5] * 1.0e-12
    yield "all series", np.array([1.0e3, 1.0e5]), np.logspace(-1.0, 4.0, 20)
    yield ("straddle",) + straddle_grid()


def test_ic_loss_small_grids_device_equals_det_host(grids):
    gnt, E_field, _ = grids
    assert E_field[10::3].size == 130
    seen = set()
    for name, g, e in small_grids(grids):
        d = engine.ic_loss(g, e)
        h = abi.ic_loss_host(g, e, libm=False)
        assert d.shape == (g.size, e.size)
        assert np.array_equal(d.view(np.uint64), h.view(np.uint64)), name
        m = thomson_mask(g, e)
        seen.add((name, bool(m.any()), bool((~m).any())))
    assert ("all product", True, False) in seen and ("all series", False, True) in seen
    assert ("straddle", True, True) in seen and ("5x130", True, True) in seen
    assert ("3x70", True, True) in seen


def test_ic_loss_terms_past_the_factor_table(grids, monkeypatch):
    """With the ((n-1)/n)^2 table cut to 100 terms nearly every series runs
    past it (the longest has 77 970 terms): the factors computed in place
    must give the table's bits."""
    gnt, E_field, _ = grids
    g, e = gnt[[0, 120, 199]], E_field[100:380:4]
    full = engine.ic_loss(g, e)
    monkeypatch.setenv("C2D_ICLOSS_TAB_N", "100")
    cut = engine.ic_loss(g, e)
    monkeypatch.delenv("C2D_ICLOSS_TAB_N")
    assert np.array_equal(cut.view(np.uint64), full.view(np.uint64))
    assert np.array_equal(cut.view(np.uint64), abi.ic_loss_host(g, e, libm=False).view(np.uint64))


def test_ic_loss_full_table(full_device, grids):
    gnt, E_field, _ = grids
    with np.load(GOLD / "fp_fic.npz", allow_pickle=False) as z:
        g = z["F_IC"].copy()
    d = full_device
    rel = np.abs(d - g) / np.abs(g)
    print("device vs the reference's F_IC: %d entries differ, max rel %.3e" % ((d != g).sum(), rel.max()))
    assert rel.max() <= 1e-9
    m = thomson_mask(gnt, E_field)
    assert np.array_equal(d[m].view(np.uint64), g[m].view(np.uint64))
    rows = [0, 57, 199]
    h = abi.ic_loss_host(gnt[rows], E_field, libm=False)
    assert np.array_equal(d[rows].view(np.uint64), h.view(np.uint64))


def test_ic_loss_fortran_layout(grids):
    gnt, E_field, _ = grids
    g, e = gnt[[0, 57, 120, 180, 199]], E_field[10::3]
    c = engine.ic_loss(g, e)
    f = engine.ic_loss(g, e, fortran=True)           # F_IC(n_el, n_ph): s_i = 1, s_ph = n_el
    assert f.flags.f_contiguous and f.strides == (8, 8 * g.size)
    assert np.array_equal(np.ascontiguousarray(f).view(np.uint64), c.view(np.uint64))


def test_ic_loss_reports_kernel_time(grids):
    gnt, E_field, _ = grids
    ms = []
    engine.ic_loss(gnt[[0, 199]], E_field[::8], kernel_ms=ms)
    assert len(ms) == 1 and ms[0] > 0.0


@pytest.mark.parametrize("n", [1, 16, 65])
def test_electrons_device_equals_det_host(gold, n):
    idx = np.arange(n) % 16
    ins = [gold[k][idx] for k in IN_KEYS]
    d = engine.setup_electrons(*ins)
    h = abi.setup_electrons_host(*ins, libm=False)
    for k in abi.SETUP_ELECTRON_OUT:
        assert d[k].shape == h[k].shape
        for z in range(n):
            assert bits_equal(d[k][z], h[k][z]), (k, z, int(idx[z]))
    assert np.isnan(d["f_nt"][idx == 2]).all() and not np.isnan(d["f_nt"][idx != 2]).any()
    ok = idx != 2
    worst = np.max(np.abs(d["f_nt"][ok] - gold["f_nt"][idx[ok]]) / np.maximum(gold["f_nt"][idx[ok]], 1e-300))
    print("device f_nt vs the reference: max rel %.3e" % worst)
    assert worst <= 6e-15                               # the det flavour's bound (tests/test_setup_host.py)


def _p(a):
    return None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(abi.PD)


def _ic(gnt, n_el, E_field, n_ph, out=True):
    lib = engine.load_library()
    F = np.full((max(n_el, 1), max(n_ph, 1)), -7.0)
    rc = lib.c2d_ic_loss(0, _p(gnt), n_el, _p(E_field), n_ph, F.ctypes.data_as(abi.PD) if out else None,
                         max(n_ph, 1), 1)
    assert (F == -7.0).all() or rc == 0                 # a refused call writes nothing
    return rc


def test_ic_loss_argument_errors():
    g, e = np.array([1.0, 2.0]), np.array([1.0, 2.0, 3.0])
    assert _ic(g, 2, e, 3) == 0
    assert _ic(None, 2, e, 3) == abi.C2D_E_ARG
    assert _ic(g, 2, None, 3) == abi.C2D_E_ARG
    assert _ic(g, 2, e, 3, out=False) == abi.C2D_E_ARG
    assert _ic(g, 0, e, 3) == abi.C2D_E_ARG
    assert _ic(g, 2, e, 0) == abi.C2D_E_ARG
    assert _ic(np.ones(201), 201, e, 3) == abi.C2D_E_ARG
    assert _ic(g, 2, np.ones(401), 401) == abi.C2D_E_ARG
    assert _ic(np.array([1.0, 0.0]), 2, e, 3) == abi.C2D_E_ARG
    assert _ic(g, 2, np.array([1.0, -2.0, 3.0]), 3) == abi.C2D_E_ARG
    assert _ic(np.array([1.0, math.nan]), 2, e, 3) == abi.C2D_E_NONFINITE
    assert _ic(g, 2, np.array([1.0, math.inf, 3.0]), 3) == abi.C2D_E_NONFINITE


def _el(n, arrs, outs=True, null_in=None):
    lib = engine.load_library()
    ins = [np.ascontiguousarray(a, np.float64) for a in arrs]
    m = max(int(n), 1)
    out = [np.zeros(m), np.zeros(m), np.zeros(m), np.zeros((m, abi.NUM_NT)), np.zeros((m, abi.NUM_NT))]
    pi = [None if null_in == i else a.ctypes.data_as(abi.PD) for i, a in enumerate(ins)]
    po = [a.ctypes.data_as(abi.PD) if outs else None for a in out]
    rc = lib.c2d_setup_electrons(0, n, *pi, *po)
    assert rc == 0 or not any(a.any() for a in out)       # a refused call writes nothing
    return rc


def test_electrons_argument_errors():
    ok = [np.array([100.0]), np.array([0.0]), np.array([100.0]), np.array([1e5]), np.array([2.3])]
    assert _el(1, ok) == 0
    assert _el(0, ok) == abi.C2D_E_ARG
    assert _el(99 * 99 + 1, ok) == abi.C2D_E_ARG
    assert _el(1, ok, outs=False) == abi.C2D_E_ARG
    assert _el(1, ok, null_in=0) == abi.C2D_E_ARG
    for i in (0, 2, 3):
        bad = [a.copy() for a in ok]
        bad[i][0] = -1.0
        assert _el(1, bad) == abi.C2D_E_ARG
    for i in range(5):
        bad = [a.copy() for a in ok]
        bad[i][0] = math.inf
        assert _el(1, bad) == abi.C2D_E_NONFINITE


SOURCES = 20_000


@pytest.fixture(scope="module")
def host_workloads():
    """deck_workload of the C3 deck with both host setups (their IC-loss
    tables take one core ~10 s each: built side by side, once)."""
    with ThreadPoolExecutor(2) as ex:
        a = ex.submit(deck.deck_workload, synth.C3_DECK, SOURCES, "host-libm", abi.COMTOT_EXACT)
        b = ex.submit(deck.deck_workload, synth.C3_DECK, SOURCES, "host-det", abi.COMTOT_EXACT)
        return a.result(), b.result()


def run3(wl):
    eng = Engine(wl.grid)
    run = CoupledRun(eng, wl, fp_mode=abi.FP_EXACT)
    rows = [dict(run.step()) for _ in range(3)]
    f, p = run.electrons()
    t = {k: np.array(v, copy=True) for k, v in eng.tallies().items()}
    st = {k: np.array(v, copy=True) for k, v in run.state.items()}
    eng.close()
    return rows, f, p, t, st


def test_deck_workload_host_libm_is_c3_workload(host_workloads):
    """The C3 deck through deck_workload(setup="host-libm") starts from the
    same bits as synth.c3_workload (the reference's own P_nontherm and
    IC_loss dumps), so three steps of the exact build follow the same packet
    histories: equal counters, tallies and electrons up to the order of the
    atomic tally sums (1e-16 a step, carried through FP_calc's sub-steps;
    the bounds are those of the device-resident / host-loop comparison in
    tests/test_gpu_c3.py)."""
    wl, _ = host_workloads
    ref = synth.c3_workload(sources=SOURCES, comtot_mode=abi.COMTOT_EXACT)
    for k in ref.state0:
        assert bits_equal(wl.state0[k], ref.state0[k]), k
    for k in ref.fixed:
        assert bits_equal(wl.fixed[k], ref.fixed[k]), k
    assert bits_equal(wl.fp_const.F_IC, ref.fp_const.F_IC)
    for k in ("E_ph", "E_field", "gnt", "hu", "z", "r"):
        assert bits_equal(getattr(wl.grid, k), getattr(ref.grid, k)), k
    assert wl.dt == ref.dt and wl.nst == ref.nst
    ra, fa, pa, ta, sa = run3(wl)
    rb, fb, pb, tb, sb = run3(ref)
    for a, b in zip(ra, rb):
        assert a["volume_packets"] == b["volume_packets"] and a["sources"] == b["sources"]
        assert abs(a["packet_steps"] - b["packet_steps"]) <= 1e-3 * b["packet_steps"]
        assert a["aborted"] == 0 and b["aborted"] == 0
    np.testing.assert_allclose(fa, fb, rtol=1e-6, atol=1e-12 * np.max(np.abs(fb)))
    np.testing.assert_allclose(pa, pb, rtol=1e-6, atol=1e-12)
    np.testing.assert_array_equal(sa["tea"], sb["tea"])
    for k in ("ecens", "edep"):
        np.testing.assert_allclose(ta[k], tb[k], rtol=1e-6, atol=1e-9 * np.max(np.abs(tb[k])))


def test_deck_workload_device_setup(host_workloads, full_device):
    _, det = host_workloads
    wl = deck.deck_workload(synth.C3_DECK, SOURCES, setup="device", comtot_mode=abi.COMTOT_EXACT)
    for k in det.state0:
        assert bits_equal(wl.state0[k], det.state0[k]), k
    assert np.array_equal(wl.fp_const.F_IC.view(np.uint64), det.fp_const.F_IC.view(np.uint64))
    assert np.array_equal(wl.fp_const.F_IC.view(np.uint64), full_device.view(np.uint64))
    rows, f, p, t, st = run3(wl)
    assert rows[-1]["aborted"] == 0
    assert np.isfinite(f).all() and np.isfinite(p).all()
    assert all(np.isfinite(v).all() for v in st.values())
    ref_rows = run3(synth.c3_workload(sources=SOURCES, comtot_mode=abi.COMTOT_EXACT))[0]
    for name, rr in (("device setup", rows), ("c3_workload", ref_rows)):
        print(name, "mean_Te", [r["mean_Te"] for r in rr], "escapes", [r["escapes"] for r in rr])
