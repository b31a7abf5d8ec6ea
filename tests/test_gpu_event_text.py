"""The escape-event file written by the library (c2d_events_write*,
compton2d_amd/csrc/evtext.hip): the text is formatted on the GPU by
csrc/c2d_fmt.h and must be, byte for byte, what the host build of the same
header gives (tests/c/fmt_wrap.c, pinned to flang and glibc in
tests/test_fmt_host.py) and what observer.write_events writes in Python.

Events of the caller are built from the directed cases of the formatter, 18
values cycling over 7 fields, so exact ties, carries and three-digit exponents
land on every field position and on every chunk and workgroup edge; the event
counts straddle 16 (the store vector), 256 (the workgroup) and the chunk knob
C2D_EVTEXT_CHUNK.  The error cases pass arguments the library rejects on the
host or counts in a scan kernel; none makes the device fault.

The observer sums compared around a write are accumulated with device atomics
in an unspecified order (tests/test_gpu_observe.py): counts are compared
exactly, the ew sums to rtol 1e-12."""
import numpy as np
import pytest
import torch

import fmt_cases as FC
from compton2d_amd import abi, observer
from compton2d_amd.engine import C2DError, Engine, device_fmt_e14_7, obs_engine
from golden_io import GoldenCase

pytestmark = pytest.mark.gpu

NS = (0, 1, 15, 16, 17, 255, 256, 257, 4099)
DIRECTED_X = np.array([v for v, _ in FC.DIRECTED])
DIRECTED_S = [s for _, s in FC.DIRECTED]


def directed_events(n, shift=0):
    """n events cycling through the directed values, and the file flang would write."""
    idx = (np.arange(7 * n) + shift) % len(DIRECTED_X)
    ev = DIRECTED_X[idx].reshape(n, 7)
    text = "".join(" ".join(DIRECTED_S[i] for i in row) + "\n" for row in idx.reshape(n, 7))
    return ev, text.encode()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return FC.HostFmt(tmp_path_factory.mktemp("fmt"))


@pytest.fixture(scope="module")
def eng():
    e = obs_engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def stepped():
    """The golden case of tests/test_gpu_edge.py up to its last step (the first
    lets nothing escape), that step's events (a few thousand, in a few of the
    buffer's shards) and the file Python writes of them."""
    gc = GoldenCase("ssc_tau")
    e = Engine(gc.grid(comtot_mode=abi.COMTOT_EXACT))
    for n in range(gc.nsteps):
        e.transport_step(gc.step_inputs(n))
    ev = e.events()
    assert len(ev) == e.last_event_count() > 0
    yield e, ev
    e.close()


@pytest.fixture(scope="module")
def stepped_text(stepped, tmp_path_factory):
    p = tmp_path_factory.mktemp("evpy") / "p001_evb.dat"
    observer.write_events(p, stepped[1])
    return p.read_bytes()


def test_selftest_whole_stress_set_equals_the_host_function(host):
    x = FC.stress_set()
    assert x.size > 2700000
    want, st, slow, bad = host.format(x)
    assert bad == 0 and slow > 1000
    got = device_fmt_e14_7(x)
    diff = np.nonzero(np.any(got != want, axis=1))[0]
    assert diff.size == 0, [(x[i], bytes(got[i]), bytes(want[i])) for i in diff[:5]]
    np.testing.assert_array_equal(device_fmt_e14_7(DIRECTED_X).tobytes().decode(), "".join(DIRECTED_S))


def test_selftest_multilimb_path_on_the_device(host, monkeypatch):
    """The events hardly ever reach the multi-limb path (ties and round values
    are decided by the exact integer test before it): with the selftest's knob
    every ambiguous value goes through it, and the bytes stay the same."""
    x = np.concatenate([FC.decimal_ties(), DIRECTED_X, [1e16, 1e7, 1e22], FC.carry_cases(), FC.powers_of_ten()])
    want, st, slow, _ = host.format(x, multilimb=True)
    assert slow > 3000 and set(np.unique(st)) == {0, 2}
    monkeypatch.setenv("C2D_FMT_SELFTEST_MULTILIMB", "1")
    np.testing.assert_array_equal(device_fmt_e14_7(x), want)
    np.testing.assert_array_equal(host.format(x)[0], want)


def test_selftest_nonfinite_is_an_error():
    with pytest.raises(C2DError, match="C2D_E_NONFINITE"):
        device_fmt_e14_7(np.array([1.0, np.nan, 2.0]))


def test_own_events_equal_the_python_writer(stepped, stepped_text, tmp_path):
    e, ev = stepped
    p = tmp_path / "p001_evb.dat"
    assert e.events_write(p) == len(ev)
    assert p.read_bytes() == stepped_text
    assert len(stepped_text) == 105 * len(ev)
    np.testing.assert_array_equal(e.events(), ev)


@pytest.mark.parametrize("chunk", [1, 16, 17, 1000])
def test_own_events_across_chunk_boundaries(stepped, stepped_text, tmp_path, monkeypatch, chunk):
    e, ev = stepped
    monkeypatch.setenv("C2D_EVTEXT_CHUNK", str(chunk))
    if chunk == 1 and len(ev) > 4000:   # one launch and copy per event: keep the test short
        ev3 = ev[:3000]
        p = tmp_path / "few.dat"
        e.events_write_from(torch.from_numpy(ev3).cuda(), p)
        assert p.read_bytes() == stepped_text[:105 * 3000]
        assert e.last_events_write()["chunks"] == 3000
        return
    p = tmp_path / "p001_evb.dat"
    assert e.events_write(p) == len(ev)
    assert p.read_bytes() == stepped_text
    assert e.last_events_write()["chunks"] == -(-len(ev) // chunk)


def test_append_concatenates_and_plain_write_truncates(stepped, stepped_text, tmp_path):
    e, ev = stepped
    p = tmp_path / "p001_evb.dat"
    assert e.events_write(p, append=True) == len(ev)      # append creates the file
    assert e.events_write(p, append=True) == len(ev)
    assert p.read_bytes() == stepped_text + stepped_text
    assert e.events_write(p) == len(ev)
    assert p.read_bytes() == stepped_text


def test_write_leaves_events_and_observer_pass_alone(stepped, tmp_path):
    e, ev = stepped
    b = observer.sed_binning(33., 7.5e15, 20, -1e12, 1e12, -1.0, 1.0,
                             ((1e-12, 1e2, 30, False), (1e2, 1e15, 30, False)))
    res = []
    for write in (True, False):
        e.obs_begin(b)
        e.obs_accumulate(None)            # asynchronous: the write must let it finish, not disturb it
        if write:
            e.events_write(tmp_path / "between.dat")
        res.append(e.obs_result()[:3])
        np.testing.assert_array_equal(e.events(), ev)
    np.testing.assert_array_equal(res[0][2], res[1][2])
    assert res[0][2].sum() > 0
    for k in (0, 1):
        np.testing.assert_allclose(res[0][k], res[1][k], rtol=1e-12, atol=0)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("n", NS)
def test_supplied_events(eng, tmp_path, where, n):
    ev, want = directed_events(n, shift=n)
    arg = torch.from_numpy(ev).cuda() if where == "device" else ev
    p = tmp_path / "ev.dat"
    eng.events_write_from(arg, p)
    assert p.read_bytes() == want
    if n:
        eng.events_write_from(arg, p, append=True)
        assert p.read_bytes() == want + want
        assert eng.last_events_write()["ambiguous"] > 0     # the ties left the fast path on the device


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("chunk", [17, 1000])
def test_supplied_events_across_chunks(eng, tmp_path, monkeypatch, where, chunk):
    monkeypatch.setenv("C2D_EVTEXT_CHUNK", str(chunk))
    ev, want = directed_events(4099, shift=3)
    p = tmp_path / "ev.dat"
    eng.events_write_from(torch.from_numpy(ev).cuda() if where == "device" else ev, p)
    assert p.read_bytes() == want
    assert eng.last_events_write()["chunks"] == -(-4099 // chunk)


def test_golden_events_round_trip(eng, tmp_path):
    ev = FC.golden_events()
    p, q, r = tmp_path / "lib.dat", tmp_path / "py.dat", tmp_path / "obs.dat"
    eng.events_write_from(ev, p)
    observer.write_events(q, ev)
    assert p.read_bytes() == q.read_bytes()
    np.testing.assert_array_equal(observer.read_events(p), ev)
    observer.write_events(r, torch.from_numpy(ev).cuda(), engine=eng)     # the observer's own door to it
    assert r.read_bytes() == q.read_bytes()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("append", [False, True])
def test_nonfinite_event_fails_and_leaves_the_file(eng, tmp_path, where, append):
    ev, _ = directed_events(4099)
    ev = ev.copy()
    ev[4000, 4] = np.nan
    ev[4050, 1] = np.inf
    p = tmp_path / "keep.dat"
    p.write_bytes(b"what was here before\n")
    with pytest.raises(C2DError, match=r"C2D_E_NONFINITE.*record 4001 .*field 5") as ei:
        eng.events_write_from(torch.from_numpy(ev).cuda() if where == "device" else ev, p, append=append)
    assert ei.value.code == abi.C2D_E_NONFINITE
    assert p.read_bytes() == b"what was here before\n"
    fresh = tmp_path / "never.dat"
    with pytest.raises(C2DError, match="C2D_E_NONFINITE"):
        eng.events_write_from(ev, fresh, append=append)
    assert not fresh.exists()


def test_io_and_argument_errors(eng, stepped, tmp_path):
    e, ev = stepped
    ev1, _ = directed_events(3)
    for call in (lambda p: eng.events_write_from(ev1, p), lambda p: e.events_write(p),
                 lambda p: eng.events_write_from(ev1[:0], p)):
        with pytest.raises(C2DError, match="C2D_E_IO") as ei:
            call(tmp_path / "no_such_directory" / "ev.dat")
        assert ei.value.code == -10 and "no_such_directory" in str(ei.value)
    with pytest.raises(C2DError, match="C2D_E_STATE"):
        eng.events_write(tmp_path / "x.dat")                 # this context has not run a step
    assert not (tmp_path / "x.dat").exists()
    lib = eng.lib
    assert lib.c2d_events_write_from(eng.ctx, None, 5, 0, b"x", 0) == -1      # C2D_E_ARG
    assert lib.c2d_events_write_from(eng.ctx, ev1.ctypes.data, -1, 0, b"x", 0) == -1
    assert lib.c2d_events_write_from(eng.ctx, ev1.ctypes.data, 3, 0, None, 0) == -1
    assert lib.c2d_events_write(e.ctx, None, 0, None) == -1
    assert lib.c2d_events_write(None, b"x", 0, None) == -1


def test_no_events(eng, tmp_path):
    p = tmp_path / "empty.dat"
    p.write_bytes(b"old\n")
    eng.events_write_from(np.zeros((0, 7)), p, append=True)
    assert p.read_bytes() == b"old\n"                        # n == 0, append: untouched
    eng.events_write_from(np.zeros((0, 7)), p)
    assert p.read_bytes() == b""                             # n == 0: an empty file
    q = tmp_path / "absent.dat"
    eng.events_write_from(torch.zeros((0, 7), dtype=torch.float64, device="cuda"), q, append=True)
    assert not q.exists()
