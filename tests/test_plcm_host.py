"""The library's host-side plcm code (compton2d_amd/csrc/plcm_host.h: the
dialogue parser and the file writer behind c2d_obs_set_add_plcm /
c2d_obs_set_write) on the CPU, compiled with gcc as C99 into a small harness
(tests/c/plcm_wrap.c): its names, scalars and bin edges equal
compton2d_amd/observer.py's parse_plcm_deck bit for bit, and its files equal
observer.write_lc byte for byte, on the reference's own decks
(tests/golden/obs.npz) and on edge cases of the dialogue (defaults, a
digit-only input series, n_mu above plcm's 10, more than 7 regions, a linear
multi-bin region, defaulted lower mu edges, too many channels)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from compton2d_amd import observer

HERE = Path(__file__).resolve().parent
G = np.load(HERE / "golden" / "obs.npz", allow_pickle=False)
PD = C.POINTER(C.c_double)


class Deck(C.Structure):
    _fields_ = [("infile", C.c_char * 64), ("names", (C.c_char * 64) * 10),
                ("gam_bulk", C.c_double), ("rmax", C.c_double), ("dt", C.c_double),
                ("t_offset", C.c_double), ("t_max", C.c_double),
                ("n_t", C.c_int), ("n_mu", C.c_int), ("n_e", C.c_int),
                ("t0", C.c_double * 1024), ("t1", C.c_double * 1024),
                ("mu0", C.c_double * 10), ("mu1", C.c_double * 10),
                ("E0", C.c_double * 20), ("E1", C.c_double * 20)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("plcm") / "libplcm_wrap.so"
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Werror",
                    "-fPIC", "-shared", "-o", str(so), str(HERE / "c" / "plcm_wrap.c"), "-lm"], check=True)
    L = C.CDLL(str(so))
    assert L.lw_sizeof() == C.sizeof(Deck)
    L.lw_parse.argtypes = [C.c_char_p, C.POINTER(Deck)]
    L.lw_write.argtypes = [C.c_char_p, C.POINTER(Deck), PD, PD, PD, C.c_int]
    return L


DECKS = {k[5:]: str(G[k]) for k in G.files if k.startswith("deck_") and str(G["tool_" + k[5:]]) == "plcm"}
DECKS.update({
    "defaults": "",
    # input series by its digits, default output names, two angular bins
    "digits": "7\n15\n1e17\n\n2\n\n0.9\n0.95\n\n\n0.99\n5e2\n1e3\n4e4\n2\n1e-2\n1\n2\n0\n\n\n\n\n",
    # 12 angular bins asked for: plcm keeps 10; lower edges defaulted (the bin before's upper edge)
    "many_mu": "p002_evc.dat\n20\n\nwide\n12\n" + "".join("\n\n%.5f\n" % (0.9995 + 0.00005 * k) for k in range(10))
               + "1e3\n2e3\n9e4\n1\n1\n1e4\n3\n0\n",
    # 9 regions, all defaulted: the last two take E_lower = E_upper of the one before
    "nine_regions": "p001_evb.dat\n33\n1e16\nlc_r.dat\n1\n\n0.5\n1\n7e2\n0\n3e4\n9\n" + "\n" * 36,
    # a linear region of 4 bins after a log one of 3
    "linear": "p001_evb.dat\n10\n2e16\nlin\n2\nlin_a\n0.99\n0.999\nlin_b.txt\n\n1\n2e3\n-1e4\n5e4\n2\n"
              "1e-3\n1\n3\n0\n1e2\n1e6\n4\n1\n",
})
assert len(DECKS) == 7


def _parse(lib, text):
    d = Deck()
    rc = lib.lw_parse(text.encode(), C.byref(d))
    return rc, d


def _arr(a):
    return np.ascontiguousarray(a, np.float64)


def _write(lib, d, directory, F, F2, cnt, factor):
    F, F2, cnt = _arr(F), _arr(F2), _arr(cnt)
    rc = lib.lw_write(str(directory).encode(), C.byref(d), F.ctypes.data_as(PD), F2.ctypes.data_as(PD),
                      cnt.ctypes.data_as(PD), factor)
    assert rc == 0


@pytest.mark.parametrize("name", sorted(DECKS))
def test_plcm_dialogue_equals_observer(lib, name):
    rc, d = _parse(lib, DECKS[name])
    assert rc == 0
    b = observer.parse_plcm_deck(DECKS[name])
    assert d.infile.decode() == b.infile
    assert [d.names[k].value.decode() for k in range(d.n_mu)] == b.outfiles
    assert (d.gam_bulk, d.rmax, d.dt, d.t_offset, d.t_max) == (b.gam_bulk, b.rmax, b.dt, b.t_offset, b.t_end)
    assert (d.t_offset, d.t_max - d.t_offset) == (b.t_start, b.t_stop)
    assert (d.n_t, d.n_mu, d.n_e) == (b.n_t, b.n_mu, b.n_e)
    for f, ref in (("t0", b.t0), ("t1", b.t1), ("mu0", b.mu0), ("mu1", b.mu1), ("E0", b.E0), ("E1", b.E1)):
        got = np.ctypeslib.as_array(getattr(d, f))[:len(ref)]
        assert np.array_equal(got, ref), f
    if name == "many_mu":
        assert d.n_mu == 10 and d.mu0[3] == d.mu1[2]
    if name == "nine_regions":
        assert d.n_e == 9 and d.E0[8] == d.E1[7] == 1e10


@pytest.mark.parametrize("name", sorted(DECKS))
def test_plcm_files_equal_observer(lib, name, tmp_path):
    rc, d = _parse(lib, DECKS[name])
    b = observer.parse_plcm_deck(DECKS[name])
    rng = np.random.default_rng(11)
    shape = (b.n_t, b.n_mu, b.n_e)
    cnt = np.floor(rng.random(shape) * 40) * (rng.random(shape) < 0.7)
    cnt[rng.random(shape) < 0.15] = 1.0
    F = rng.lognormal(30, 5, shape) * (cnt > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        F2 = np.where(cnt > 0, F * F / cnt, 0.0) * (1.0 + rng.random(shape))
    F2[cnt == 1] = (F * F)[cnt == 1]
    shave = (rng.random(shape) < 0.05) & (cnt > 1)      # rounding below <ew>^2: sqrt of a negative, "-nan"
    F2[shave] = (F * F / np.where(cnt > 0, cnt, 1.0))[shave] * (1 - 1e-15)
    rows = int(np.argmax(b.t1 > b.t_stop)) + 1          # the rows the files print
    assert (cnt[:rows] == 0).any() and (cnt[:rows] == 1).any() and shave[:rows].any()
    (tmp_path / "c").mkdir()
    (tmp_path / "p").mkdir()
    _write(lib, d, tmp_path / "c", F, F2, cnt, 2)
    with np.errstate(all="ignore"):
        written = observer.write_lc(tmp_path / "p", b, observer.Histogram(F, F2, cnt), 2)
    assert len(written) == 1 + 2 * b.n_mu
    assert sorted(p.name for p in (tmp_path / "c").iterdir()) == sorted(p.name for p in written)
    for p in written:
        assert (tmp_path / "c" / p.name).read_bytes() == p.read_bytes(), p.name


@pytest.mark.parametrize("name,nfiles", [("lc_mrk421", 3), ("lc_wide", 7)])
def test_plcm_files_equal_reference_plcm_output(lib, name, nfiles, tmp_path):
    """The reference plcm's own files for its own events (obs.npz), written by
    the library's writer from the oracle's sums of those events."""
    import oracle_lib as OL
    deck = str(G["deck_" + name])
    rc, d = _parse(lib, deck)
    assert rc == 0
    b = observer.parse_plcm_deck(deck)
    F, F2, cnt = OL.obs_bin(b, G["events"], "ref")
    _write(lib, d, tmp_path, F, F2, cnt, 1)
    files = list(G["files_" + name])
    assert len(files) == nfiles and sorted(p.name for p in tmp_path.iterdir()) == sorted(files)
    for f in files:
        assert (tmp_path / f).read_text() == str(G["out_%s__%s" % (name, f)]), f


def test_plcm_too_many_channels(lib):
    rc, _ = _parse(lib, "p001_evb.dat\n33\n1e16\nx\n1\n\n\n\n7e2\n0\n7e4\n2\n1e-3\n1\n10\n0\n1\n1e3\n11\n0\n")
    assert rc == -1
    rc, _ = _parse(lib, "p001_evb.dat\n33\n1e16\nx\n1\n\n\n\n7e2\n0\n7e4\n2\n1e-3\n1\n10\n0\n1\n1e3\n10\n0\n")
    assert rc == 0
