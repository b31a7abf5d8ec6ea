"""Event files read back by the library (c2d_events_read,
c2d_obs_accumulate_file, c2d_obs_set_accumulate_file; csrc/c2d_scan.h,
evparse.hip): the parser on the device equals the host harness of
tests/test_scan_host.py bit for bit, statuses included, also with every field
forced through the multi-limb path; files the library wrote come back as
float() of each written field at every edge of the kernel (workgroups of 256
records, 16-byte staging, chunk boundaries) and must have been parsed by the
kernel (canonical == n, host_parsed == 0); binning a file equals binning the
events Python reads from it; free-format, CRLF, split records and NaN fall
back to the host parser from the first such record on and equal
observer.read_events; a bad token is C2D_E_IO with its byte offset after the
records before it were delivered.

Observer sums are accumulated with device atomics in an unspecified order
(tests/test_gpu_observe.py): counts are compared exactly, the ew sums to rtol
1e-12."""
from pathlib import Path

import numpy as np
import pytest
import torch

import fmt_cases as FC
import scan_cases as SC
from compton2d_amd import abi, observer
from compton2d_amd.engine import C2DError, Engine, device_scan_e14_7, obs_engine
from golden_io import GoldenCase

pytestmark = pytest.mark.gpu

NS = (0, 1, 15, 16, 17, 255, 256, 257, 4099)
DIRECTED_X = np.array([v for v, _ in FC.DIRECTED])
DIRECTED_S = [s for _, s in FC.DIRECTED]
G = np.load(Path(__file__).resolve().parent / "golden" / "obs.npz", allow_pickle=False)


def directed_events(n, shift=0):
    """n events cycling through the directed values; float() of each field flang
    would write of them (what a correct reader returns), as uint64 [n, 7]."""
    idx = (np.arange(7 * n) + shift) % len(DIRECTED_X)
    want = SC.expected_bits(DIRECTED_S)[idx].reshape(n, 7)
    return DIRECTED_X[idx].reshape(n, 7), want


def bits(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float64).view(np.uint64).reshape(-1, 7)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("scan")


@pytest.fixture(scope="module")
def host(work):
    return SC.HostScan(work)


@pytest.fixture(scope="module")
def eng():
    e = obs_engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def stepped(tmp_path_factory):
    """The golden case stepped as in tests/test_gpu_event_text.py, its last
    step's events, the file the library writes of them and what Python reads
    from that file."""
    gc = GoldenCase("ssc_tau")
    e = Engine(gc.grid(comtot_mode=abi.COMTOT_EXACT))
    for n in range(gc.nsteps):
        e.transport_step(gc.step_inputs(n))
    ev = e.events()
    p = tmp_path_factory.mktemp("own") / "p001_evb.dat"
    assert e.events_write(p) == len(ev) > 0
    yield e, ev, p, observer.read_events(p)
    e.close()


def test_selftest_field_set_equals_the_host_harness(host, work, monkeypatch):
    fields = SC.field_set(work) + tuple(SC.NOT_CANONICAL)
    text = SC.to_bytes(fields)
    want, st, slow = host.scan(text, fill=0.0)
    assert slow > 100 and set(np.unique(st)) == {-1, 0, 1}
    got, gst = device_scan_e14_7(text)
    assert np.array_equal(gst, st.astype(np.int32))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(fields[i], hex(got[i]), hex(want[i])) for i in bad[:5]]
    ok = st >= 0
    assert np.array_equal(got[ok], SC.expected_bits([f for f, k in zip(fields, ok) if k]))
    # every field through the multi-limb path on the device
    sub = fields[::7] + tuple(SC.HAND) + tuple(f for f, _, _ in SC.constructed_ties()) + tuple(SC.NOT_CANONICAL)
    text = SC.to_bytes(sub)
    want, st, slow = host.scan(text, exact=True, fill=0.0)
    assert slow > len(sub) // 2
    monkeypatch.setenv("C2D_SCAN_SELFTEST_EXACT", "1")
    got, gst = device_scan_e14_7(text)
    assert np.array_equal(gst, st.astype(np.int32)) and np.array_equal(got, want)
    assert np.array_equal(got, host.scan(text, fill=0.0)[0])


def expected_chunks(n, chunk):
    return -(-n // chunk) if n else 0


@pytest.fixture(scope="module")
def written(eng, tmp_path_factory):
    """The files the library writes of the directed events, once for all chunk sizes."""
    d = tmp_path_factory.mktemp("rt")
    out = {}
    for n in NS:
        for shift in (0, 3):
            ev, want = directed_events(n, shift)
            p = d / ("e%d_%d.dat" % (n, shift))
            eng.events_write_from(ev, p)
            assert p.stat().st_size == 105 * n
            out[n, shift] = (p, want)
    return out


@pytest.mark.parametrize("chunk", [None, 1, 16, 17, 1000])
def test_round_trip_at_the_kernels_edges(eng, written, monkeypatch, chunk):
    if chunk is not None:
        monkeypatch.setenv("C2D_EVTEXT_CHUNK", str(chunk))
    for (n, shift), (p, want) in written.items():
        if chunk == 1 and n > 257:
            continue
        for device in (False, True):
            got = eng.events_read(p, device=device)
            assert (got.is_cuda if device else isinstance(got, np.ndarray)) and tuple(got.shape) == (n, 7)
            assert np.array_equal(bits(got), want), (n, shift, device)
            t = eng.last_events_read()
            assert t["host_parsed"] == 0 and t["canonical"] == n, t
            assert t["chunks"] == expected_chunks(n, chunk or (1 << 20)), t


@pytest.mark.parametrize("chunk", [None, 17])
def test_capacity_below_the_record_count(eng, written, monkeypatch, chunk):
    """cap < n: the first cap records, nothing beyond them, and the whole count."""
    if chunk is not None:
        monkeypatch.setenv("C2D_EVTEXT_CHUNK", str(chunk))
    for n, cap in ((17, 1), (257, 256), (4099, 4083), (4099, 30)):
        if chunk is not None and n > 257:
            continue
        p, want = written[n, 3]
        out = np.full((cap + 1, 7), 7.0)
        assert eng.events_read_into(p, out[:cap]) == n
        assert np.array_equal(bits(out[:cap]), want[:cap]) and np.all(out[cap] == 7.0)
        dev = torch.full((cap + 1, 7), 7.0, dtype=torch.float64, device="cuda")
        assert eng.events_read_into(p, dev[:cap]) == n
        assert np.array_equal(bits(dev[:cap]), want[:cap]) and bool((dev[cap] == 7.0).all())
        assert eng.events_read_into(p, np.zeros((0, 7))) == n          # only counts
        assert eng.last_events_read()["canonical"] == n


def test_ties_in_a_file_take_the_exact_path_on_the_device(eng, tmp_path):
    ties = [f for f, _, _ in SC.constructed_ties()]
    fl = (ties * 7)[:7 * (len(ties) - 1)]
    p = tmp_path / "ties.dat"
    p.write_bytes("".join(" ".join(fl[7 * i:7 * i + 7]) + "\n" for i in range(len(fl) // 7)).encode())
    got = eng.events_read(p)
    assert np.array_equal(bits(got), SC.expected_bits(fl).reshape(-1, 7))
    t = eng.last_events_read()
    assert t["exact_fields"] == len(fl) and t["canonical"] == len(fl) // 7 and t["host_parsed"] == 0


def test_own_events_binned_from_the_file(stepped):
    e, ev, p, ev_py = stepped
    assert len(ev_py) == len(ev)
    wide = observer.sed_binning(33., 7.5e15, 20, -1e12, 1e12, -1.0, 1.0,
                                ((1e-12, 1e2, 30, False), (1e2, 1e15, 30, False)))
    e.obs_begin(wide)
    e.obs_accumulate(ev_py)
    want = e.obs_result()[:3]
    e.obs_begin(wide)
    assert e.obs_accumulate_file(p) == len(ev)
    got = e.obs_result()[:3]
    t = e.last_events_read()
    assert t["canonical"] == len(ev) and t["host_parsed"] == 0 and t["chunks"] == 1
    assert want[2].sum() > 0
    np.testing.assert_array_equal(got[2], want[2])
    for k in (0, 1):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(e.events(), ev)
    np.testing.assert_array_equal(bits(e.events_read(p)), bits(ev_py))
    single = e.obs_result()[:3]

    def members():
        e.obs_set_clear()
        return [e.obs_set_add_pspt(str(G["deck_sed_wide"])), e.obs_set_add_plcm(str(G["deck_lc_wide"])),
                e.obs_set_add(wide)]
    ids = members()
    e.obs_set_accumulate(ev_py)
    want = [e.obs_set_result(i) for i in ids]
    ids = members()
    assert e.obs_set_accumulate_file(p) == len(ev)
    got = [e.obs_set_result(i) for i in ids]
    assert want[2][2].sum() > 0
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g[2], w[2])
        for k in (0, 1):
            np.testing.assert_allclose(g[k], w[k], rtol=1e-12, atol=0)
    # the single observer and the event buffer are as they were
    for g, w in zip(e.obs_result()[:3], single):
        np.testing.assert_array_equal(g, w)
    np.testing.assert_array_equal(e.events(), ev)
    assert e.last_event_count() == len(ev)
    e.obs_set_clear()


def fallback_text():
    e_form = [f for f in DIRECTED_S if f[10] == "E"]         # float() does not take the E-less form
    lines = [" ".join(e_form[i % len(e_form)] for i in range(7 * r + 3, 7 * r + 10)) + "\n" for r in range(500)]
    mid = ["1.5 2 3e0 4 5 6 7\n",
           lines[300].rstrip("\n") + "\r\n",
           " 0.1000000E+01  0.2000000E+01\n 0.3000000E+01 4 5\n6 7\n",
           lines[301][:15] + "           NaN" + lines[301][29:]]
    return "".join(lines[:300] + mid + lines[300:] + ["1 2 3\n"]), 300, 4 + 200


def nan_equal(a, b):
    a, b = bits(a), bits(b)
    fa, fb = a.view(np.float64), b.view(np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(fa) & np.isnan(fb))))


@pytest.mark.parametrize("chunk", [None, 64, 300])
def test_fallback_to_the_host_parser(eng, tmp_path, monkeypatch, chunk):
    if chunk is not None:
        monkeypatch.setenv("C2D_EVTEXT_CHUNK", str(chunk))
    text, n_canon, n_host = fallback_text()
    p = tmp_path / "mixed.dat"
    p.write_bytes(text.encode())
    want = observer.read_events(p)
    assert len(want) == n_canon + n_host and np.isnan(want).sum() == 1
    for device in (False, True):
        got = eng.events_read(p, device=device)
        assert nan_equal(got, want)
        t = eng.last_events_read()
        assert t["canonical"] == n_canon and t["host_parsed"] == n_host, t
    # binned like the events Python reads (the NaN as pspt's comparisons bin it)
    b = observer.sed_binning(33., 7.5e15, 20, -1e12, 1e12, -1.0, 1.0, ((1e-12, 1e2, 30, False), (1e2, 1e15, 30, False)))
    eng.obs_begin(b)
    eng.obs_accumulate(want)
    ref = eng.obs_result()[:3]
    eng.obs_begin(b)
    assert eng.obs_accumulate_file(p) == len(want)
    res = eng.obs_result()[:3]
    np.testing.assert_array_equal(res[2], ref[2])
    # only the final newline missing: everything parses, the last record on the host
    ev, bits_want = directed_events(257, 0)
    q = tmp_path / "nonl.dat"
    eng.events_write_from(ev, q)
    q.write_bytes(q.read_bytes()[:-1])
    assert q.stat().st_size == 105 * 257 - 1
    got = eng.events_read(q)
    assert np.array_equal(bits(got), bits_want)
    t = eng.last_events_read()
    assert t["canonical"] == 256 and t["host_parsed"] == 1


def test_errors(eng, tmp_path):
    with pytest.raises(C2DError, match="C2D_E_IO"):
        eng.events_read(tmp_path / "missing.dat")
    lib = eng.lib
    assert lib.c2d_events_read(eng.ctx, None, None, 0, 0, None) == -1      # C2D_E_ARG
    # a token that is no number in record 40: the 39 before it are delivered and binned
    ev, want = directed_events(100, 0)
    p = tmp_path / "bad.dat"
    eng.events_write_from(ev, p)
    raw = bytearray(p.read_bytes())
    off = 105 * 39 + 15 * 2
    raw[off:off + 14] = b"           abc"
    p.write_bytes(bytes(raw))
    b = observer.sed_binning(33., 7.5e15, 20, -1e12, 1e12, -1.0, 1.0, ((1e-12, 1e2, 30, False), (1e2, 1e15, 30, False)))
    eng.obs_begin(b)
    eng.obs_accumulate(want.view(np.float64)[:39])
    ref = eng.obs_result()[:3]
    eng.obs_begin(b)
    with pytest.raises(C2DError, match="C2D_E_IO.*'abc' at byte offset %d " % (off + 11)) as ei:
        eng.obs_accumulate_file(p)
    assert ei.value.records == 39
    res = eng.obs_result()[:3]
    np.testing.assert_array_equal(res[2], ref[2])
    np.testing.assert_allclose(res[0], ref[0], rtol=1e-12, atol=0)
    out = np.full((100, 7), 7.0)
    with pytest.raises(C2DError, match="byte offset %d " % (off + 11)) as ei:
        eng.events_read_into(p, out)
    assert ei.value.records == 39
    assert np.array_equal(bits(out[:39]), want[:39]) and np.all(out[39:] == 7.0)
    t = eng.last_events_read()
    assert t["canonical"] == 39 and t["host_parsed"] == 0
    eng.obs_set_clear()
    eng.obs_set_add(b)
    with pytest.raises(C2DError, match="C2D_E_IO") as ei:
        eng.obs_set_accumulate_file(p)
    assert ei.value.records == 39 and eng.obs_set_result(0)[2].sum() == ref[2].sum()
    # state rules of the _device siblings
    eng.obs_set_clear()
    with pytest.raises(C2DError, match="C2D_E_STATE"):
        eng.obs_set_accumulate_file(p)
    fresh = obs_engine(0)
    try:
        with pytest.raises(C2DError, match="C2D_E_STATE"):
            fresh.obs_accumulate_file(p)
    finally:
        fresh.close()
    # an empty file
    z = tmp_path / "empty.dat"
    z.write_bytes(b"")
    assert eng.events_read(z).shape == (0, 7) and tuple(eng.events_read(z, device=True).shape) == (0, 7)
    eng.obs_begin(b)
    assert eng.obs_accumulate_file(z) == 0 and eng.obs_result()[2].sum() == 0
    assert eng.last_events_read()["chunks"] == 0


def test_read_events_with_an_engine_reads_e_less_fields(eng, tmp_path):
    """The three-digit-exponent form, which observer.read_events without an
    engine cannot take, is read as the number that was written."""
    ev = np.tile(np.array([[1e3, 1e-120, 1e100, 1e15, 1e15, 0.5, 1.0]]), (5, 1))
    p = tmp_path / "p001_evb.dat"
    eng.events_write_from(ev, p)
    assert b"-119" in p.read_bytes()
    with pytest.raises(ValueError):
        observer.read_events(p)
    got = observer.read_events(p, engine=eng)
    assert np.array_equal(got, ev)
