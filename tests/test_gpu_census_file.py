"""Census record files written and read by the library (c2d_census_write*,
c2d_census_read*; csrc/censtext.hip, c2d_censfmt.h): the bytes of the
reference's own write_cens and the values of its read_cens
(tests/golden/census_fmt.npz); directed doubles and integers at every edge of
the kernels (4 records = the 16-byte period, workgroups of 256 records, chunk
boundaries); the context's census, all four kinds (exact / tabulated comtot x
double-buffered / in place), byte for byte what save_census writes, and read
back bit for bit what load_census stores; the host parser behind the first
record that is not canonical; the errors.

census_io.fortran_e14_7 writes -0.0 without its sign; AMD flang, and so the
library, keep it (fmt_cases.DIRECTED[1], tests/test_fmt_host.py).  Where
bytes are compared with census_io.write_census, the sign column of a
negative zero is the one byte taken from flang instead (python_text)."""
import ctypes as C
import re
import shutil

import numpy as np
import pytest
import torch

import fmt_cases as FC
import scan_cases as SC
from compton2d_amd import abi, census_io
from compton2d_amd.engine import C2DError, Engine, obs_engine
from golden_io import GOLDEN, GoldenCase

pytestmark = pytest.mark.gpu

NS = (0, 1, 3, 4, 5, 255, 256, 257, 4099)
CHUNKS = (None, 1, 4, 5, 17, 1000)
DIRECTED_X = np.array([v for v, _ in FC.DIRECTED])
DIRECTED_S = [s for _, s in FC.DIRECTED]
INTS = np.array([0, 1, 9, 10, 99, 255, 99999], np.int32)
KINDS = [(m, i) for m in (abi.COMTOT_EXACT, abi.COMTOT_TABLE) for i in (0, 1)]
SMALL_PHI = np.array([0.0, 5.0e-11, 1.0e-10, 1.0e-6, 1.0, 3.0, 3.1415926536, 4.0, 6.0])


def set_chunk(monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("C2D_CENSTEXT_CHUNK", raising=False)
    else:
        monkeypatch.setenv("C2D_CENSTEXT_CHUNK", str(chunk))


def flang_zero_sign(text: bytes, d6) -> bytes:
    """census_io's bytes, a negative zero with flang's sign (module docstring)."""
    t = bytearray(text)
    d6 = np.asarray(d6, np.float64).reshape(-1, 6)
    for r, f in zip(*np.nonzero((d6 == 0) & np.signbit(d6))):
        assert t[116 * r + 14 * f] == ord(" ")
        t[116 * r + 14 * f] = ord("-")
    return bytes(t)


def python_text(d6, i5, keys, path) -> bytes:
    census_io.write_census(path, d6, i5, keys)
    return flang_zero_sign(path.read_bytes(), d6)


def directed_records(n, seed=0):
    """n records cycling through the directed doubles and the integers, random 64-bit keys."""
    d6 = DIRECTED_X[np.arange(6 * n) % len(DIRECTED_X)].reshape(n, 6)
    i5 = INTS[(np.arange(5 * n) + seed) % len(INTS)].reshape(n, 5)
    keys = np.random.default_rng(100 + n).integers(0, 2 ** 64, n, dtype=np.uint64)
    return d6, i5, keys


def keys_of(path):
    return np.fromfile(str(path) + census_io.KEY_SUFFIX, "<u8")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def packed(e):
    """The raw 8-word records of an engine's census."""
    n = e.census_count()
    raw = torch.zeros(max(n, 1) * abi.CENSUS_REC_WORDS, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()      # torch's fill runs on its own stream, the pack on the context's
    e.census_pack(0, n, raw.data_ptr())
    return raw.view(-1, abi.CENSUS_REC_WORDS)[:n].cpu().numpy().view(np.uint64)


def sort_rows(a):
    return a[np.lexsort(a.T[::-1])] if len(a) else a


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("censfile")


@pytest.fixture(scope="module")
def host(work):
    return SC.HostScan(work)


@pytest.fixture(scope="module")
def eng():
    e = obs_engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fmt():
    return dict(np.load(GOLDEN / "census_fmt.npz", allow_pickle=False))


@pytest.fixture(scope="module")
def directed(work, host):
    """Per n: the records, the text Python writes of them and strtod of each of its fields."""
    out = {}
    for n in NS:
        d6, i5, keys = directed_records(n)
        text = python_text(d6, i5, keys, work / ("py%d.txt" % n))
        assert len(text) == 116 * n
        fields = [text[116 * r + 14 * f:116 * r + 14 * f + 14].decode() for r in range(n) for f in range(6)]
        assert fields == [DIRECTED_S[i % len(DIRECTED_S)] for i in range(6 * n)]      # flang's own bytes
        want, st, _ = host.scan(fields) if n else (np.zeros(0, np.uint64), np.zeros(0, np.int8), 0)
        assert np.all(st >= 0)
        out[n] = (d6, i5, keys, text, want.reshape(n, 6))
    return out


_STEPPED = {}


def stepped(name, mode, inplace, work):
    """Step 0 of a golden case on one kind of context; the census save_census writes of it."""
    k = (name, mode, inplace)
    if k not in _STEPPED:
        gc = GoldenCase(name)
        e = Engine(gc.grid(comtot_mode=mode, census_inplace=inplace))
        e.transport_step(gc.step_inputs(0))
        p = work / ("save_%s_%d_%d.dat" % k)
        n = e.save_census(p)
        assert n == e.census_count() > 300
        _STEPPED[k] = (gc, e, p, flang_zero_sign(p.read_bytes(), e.census()[0]), keys_of(p))
    return _STEPPED[k]


@pytest.fixture(scope="module", autouse=True)
def close_stepped():
    yield
    for _, e, _, _, _ in _STEPPED.values():
        e.close()
    _STEPPED.clear()


# ---- 1, 2: the reference's own bytes and its own read-back ---------------------------------
@pytest.mark.parametrize("chunk", [None, 1, 17])
def test_write_from_equals_reference_write_cens(eng, fmt, tmp_path, monkeypatch, chunk):
    set_chunk(monkeypatch, chunk)
    d, i6 = fmt["d"], fmt["i6"]
    keys = i6[:, 5].astype(np.uint64)
    p = tmp_path / "c.txt"
    eng.write_census_records(d, i6[:, :5], keys, p)
    assert p.read_bytes() == bytes(fmt["text"])
    assert re.search(rb"\d[+-]\d\d\d", p.read_bytes())      # E-less three-digit exponents among them
    assert np.array_equal(keys_of(p), keys)
    t = eng.last_census_file()
    assert t["chunks"] == -(-len(keys) // (chunk or (1 << 20))) and t["convert_ms"] == 0.0


@pytest.mark.parametrize("chunk", [None, 1, 17])
def test_read_records_equals_reference_read_cens(eng, fmt, tmp_path, monkeypatch, chunk):
    set_chunk(monkeypatch, chunk)
    p = tmp_path / "ref.txt"
    p.write_bytes(bytes(fmt["text"]))              # a file written by the reference: no .keys
    d6, i5, keys = eng.parse_census_file(p)
    n = len(fmt["read_d"])
    assert np.array_equal(bits(d6), bits(fmt["read_d"]))
    assert np.array_equal(i5, fmt["read_i"][:, :5])
    assert keys.tolist() == [census_io.derive_key(int(fmt["read_i"][r, 5]), r) for r in range(n)]
    t = eng.last_census_file()
    assert t["device_records"] == n and t["host_records"] == 0, t
    mine = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(3)
    mine.astype("<u8").tofile(str(p) + census_io.KEY_SUFFIX)
    d6, i5, keys = eng.parse_census_file(p)
    assert np.array_equal(keys, mine) and np.array_equal(bits(d6), bits(fmt["read_d"]))
    # count only
    m = C.c_int64()
    assert eng.lib.c2d_census_read_records(eng.ctx, str(p).encode(), None, None, None, 0, C.byref(m)) == 0
    assert m.value == n


# ---- 3: directed values at the kernels' edges ------------------------------------------------
@pytest.mark.parametrize("chunk", CHUNKS)
def test_directed_values_at_the_kernels_edges(eng, directed, tmp_path, monkeypatch, chunk):
    set_chunk(monkeypatch, chunk)
    for n, (d6, i5, keys, text, want) in directed.items():
        if chunk is not None and chunk < 17 and n > 257:
            continue                  # thousands of chunks take seconds; 4099 straddles the larger chunks
        p = tmp_path / ("d%d.txt" % n)
        eng.write_census_records(d6, i5, keys, p)
        assert p.read_bytes() == text, n
        assert np.array_equal(keys_of(p), keys)
        assert eng.last_census_file()["chunks"] == (-(-n // (chunk or (1 << 20))) if n else 0)
        g6, g5, gk = eng.parse_census_file(p)
        assert g6.shape == (n, 6) and g5.shape == (n, 5) and gk.shape == (n,)
        assert np.array_equal(bits(g6), want), n
        assert np.array_equal(g5, i5) and np.array_equal(gk, keys)
        t = eng.last_census_file()
        assert t["device_records"] == n and t["host_records"] == 0, (n, t)
        # without the .keys file: derived from the seed column and the record index
        (tmp_path / ("d%d.txt.keys" % n)).unlink()
        gk = eng.parse_census_file(p)[2]
        assert gk.tolist() == [census_io.derive_key(int(keys[r] % np.uint64(100000)), r) for r in range(n)]


def test_integers_that_overflow_i5(eng, tmp_path):
    d6, i5, keys = directed_records(300)
    i5 = i5.copy()
    i5[7, 2] = 100000
    i5[270, 4] = -10000
    i5[271, 0] = -9999
    p = tmp_path / "o.txt"
    eng.write_census_records(d6, i5, keys, p)
    text = p.read_bytes()
    assert text == python_text(d6, i5, keys, tmp_path / "py.txt")
    assert text[116 * 7 + 85 + 10:116 * 7 + 85 + 15] == b"*****" and text.count(b"*****") == 2
    assert text[116 * 271 + 85:116 * 271 + 90] == b"-9999"
    with pytest.raises(C2DError) as e:
        eng.parse_census_file(p)
    assert e.value.code == abi.C2D_E_IO and "byte offset %d" % (116 * 7 + 85 + 10) in str(e.value)
    assert e.value.records == 7


# ---- 4: the context's census, all four kinds -------------------------------------------------
@pytest.mark.parametrize("mode,inplace", KINDS)
@pytest.mark.parametrize("name", ["ssc_tau", "c3_mrk421"])
def test_write_census_file_equals_save_census(work, tmp_path, monkeypatch, name, mode, inplace):
    gc, e, p, text, keys = stepped(name, mode, inplace, work)
    n = len(keys)
    before = e.census()
    for chunk in (None, 1000, 17):
        set_chunk(monkeypatch, chunk)
        q = tmp_path / ("w%s.dat" % chunk)
        assert e.write_census_file(q) == n
        assert q.read_bytes() == text, chunk
        assert np.array_equal(keys_of(q), keys)
        t = e.last_census_file()
        assert t["chunks"] == -(-n // (chunk or (1 << 20))) and t["kernel_ms"] > 0 and t["convert_ms"] > 0
    assert e.census_count() == n
    for a, b in zip(before, e.census()):
        assert np.array_equal(a, b)


# ---- 5: read into a context, bit for bit -----------------------------------------------------
@pytest.mark.parametrize("mode,inplace", KINDS)
@pytest.mark.parametrize("name", ["ssc_tau", "c3_mrk421"])
def test_read_census_file_equals_load_census(work, tmp_path, monkeypatch, name, mode, inplace):
    gc, e, p, text, keys = stepped(name, mode, inplace, work)
    n = len(keys)
    b = Engine(gc.grid(comtot_mode=mode, census_inplace=inplace))
    c = Engine(gc.grid(comtot_mode=mode, census_inplace=inplace))
    assert c.load_census(p) == n
    want = packed(c)
    for chunk in (None, 1000, 17):
        set_chunk(monkeypatch, chunk)
        assert b.read_census_file(p) == n == b.census_count()
        assert np.array_equal(packed(b), want), chunk
        t = b.last_census_file()
        assert t["device_records"] == n and t["host_records"] == 0 and t["convert_ms"] > 0, t
    set_chunk(monkeypatch, None)
    # azimuths at the quadrant switch's edges (tests/test_gpu_census_restart.py)
    m = len(SMALL_PHI)
    d6, i5, k = (a[:m].copy() for a in c.census())
    d6[:, 3] = SMALL_PHI
    q = tmp_path / "phi.dat"
    census_io.write_census(q, d6, i5, k)
    assert b.read_census_file(q) == m and c.load_census(q) == m
    pb, pc = packed(b), packed(c)
    assert np.array_equal(pb, pc)
    if mode == abi.COMTOT_TABLE:
        esw = (pb[:, 6] >> np.uint64(32 + 24)) & np.uint64(1)
        assert esw.tolist() == [1, 1, 0, 0, 0, 0, 1, 1, 1]       # 0.3141593E+01 > pi and pb[0, 3] == bits(np.array([1.0]))[0]
    if mode == abi.COMTOT_EXACT:
        # one further step from either census: the same histories
        assert b.read_census_file(p) == n and c.load_census(p) == n
        si = gc.step_inputs(1)
        b.transport_step(si)
        c.transport_step(si)
        assert np.array_equal(b.tallies()["counters"], c.tallies()["counters"])
        rb, rc = packed(b), packed(c)
        assert len(rb) > 0 and np.array_equal(sort_rows(rb), sort_rows(rc))
        assert np.array_equal(sort_rows(bits(b.events())), sort_rows(bits(c.events())))
    b.close()
    c.close()


# ---- 6: the host parser behind the first record that is not canonical -----------------------
def crlf(rec):
    return rec.replace(b"\n", b"\r\n")


def blank_line_before(rec):
    return b"\n" + rec


def d_exponents(rec):
    assert b"E" in rec[:14]
    return rec[:84].replace(b"E", b"D") + rec[84:]


@pytest.mark.parametrize("chunk", [None, 64, 300])
def test_host_parser_takes_over_at_the_first_record_that_is_not_canonical(work, tmp_path, monkeypatch, chunk):
    gc, e, p, text, keys = stepped("ssc_tau", abi.COMTOT_EXACT, 0, work)
    n = len(keys)
    set_chunk(monkeypatch, chunk)
    want = e.parse_census_file(p)
    recs = [text[116 * r:116 * r + 116] for r in range(n)]
    cases = []
    for k in (3, 296):                     # in the first workgroup, in a later one
        for change in (crlf, blank_line_before, d_exponents):
            cases.append((k, b"".join(recs[:k]) + b"".join(change(r) for r in recs[k:])))
    cases.append((n - 1, text[:-1]))        # the last newline dropped: a tail shorter than a record
    for with_keys in (True, False):
        if not with_keys:
            want = want[0], want[1], np.array([census_io.derive_key(int(s % np.uint64(100000)), r)
                                               for r, s in enumerate(keys)], np.uint64)
        for j, (k, changed) in enumerate(cases):
            q = tmp_path / ("m%d_%d.dat" % (j, with_keys))
            q.write_bytes(changed)
            if with_keys:
                shutil.copy(str(p) + census_io.KEY_SUFFIX, str(q) + census_io.KEY_SUFFIX)
            got = e.parse_census_file(q)
            for a, b in zip(got, want):
                assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (j, k)
            t = e.last_census_file()
            assert t["device_records"] == k and t["host_records"] == n - k, (j, k, t)
    # the same into a context
    b = Engine(gc.grid(comtot_mode=abi.COMTOT_EXACT))
    assert b.read_census_file(p) == n
    ref = packed(b)
    q = tmp_path / "m0_1.dat"
    assert b.read_census_file(q) == n
    assert np.array_equal(packed(b), ref)
    t = b.last_census_file()
    assert t["device_records"] == 3 and t["host_records"] == n - 3
    b.close()


# ---- 7: errors ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_write_nonfinite_leaves_both_files_as_they_were(eng, tmp_path, bad):
    d6, i5, keys = directed_records(600)
    p = tmp_path / "c.txt"
    eng.write_census_records(d6[:5], i5[:5], keys[:5], p)
    old = p.read_bytes(), keys_of(p).tobytes()
    d6 = d6.copy()
    d6[300, 4] = bad
    d6[411, 0] = bad
    with pytest.raises(C2DError) as e:
        eng.write_census_records(d6, i5, keys, p)
    assert e.value.code == abi.C2D_E_NONFINITE and "record 301 " in str(e.value) and "field 5" in str(e.value)
    assert (p.read_bytes(), keys_of(p).tobytes()) == old


def test_write_errors(eng, work, tmp_path):
    d6, i5, keys = directed_records(5)
    with pytest.raises(C2DError) as e:
        eng.write_census_records(d6, i5, keys, tmp_path / "no_such_dir" / "c.txt")
    assert e.value.code == abi.C2D_E_IO
    with pytest.raises(C2DError) as e:
        eng.write_census_file(tmp_path / "no_such_dir" / "c.txt")
    assert e.value.code == abi.C2D_E_IO
    path = str(tmp_path / "c.txt").encode()
    lib = eng.lib
    assert lib.c2d_census_write_from(eng.ctx, None, None, None, 3, path) == abi.C2D_E_ARG
    assert lib.c2d_census_write_from(eng.ctx, d6.ctypes.data, i5.ctypes.data, keys.ctypes.data, 5, None) == abi.C2D_E_ARG
    assert lib.c2d_census_write_from(eng.ctx, d6.ctypes.data, i5.ctypes.data, keys.ctypes.data, -1, path) == abi.C2D_E_ARG
    assert lib.c2d_census_write(eng.ctx, None, None) == abi.C2D_E_ARG
    assert lib.c2d_census_write(None, path, None) == abi.C2D_E_ARG
    assert lib.c2d_census_read(eng.ctx, None, None) == abi.C2D_E_ARG
    assert lib.c2d_census_read_records(eng.ctx, path, None, None, None, 4, C.byref(C.c_int64())) == abi.C2D_E_ARG
    # an empty census: two empty files
    assert eng.census_count() == 0 and eng.write_census_file(tmp_path / "e.txt") == 0
    assert (tmp_path / "e.txt").read_bytes() == b"" and (tmp_path / "e.txt.keys").read_bytes() == b""


def test_write_of_a_lost_census_is_a_state_error(work, tmp_path):
    """The census lost as in tests/test_gpu_census_restart.py
    test_chunked_census_lost_after_failed_step; a file read restores it."""
    gc, e, p, text, keys = stepped("ssc_tau", abi.COMTOT_EXACT, 1, work)
    b = Engine(gc.grid(comtot_mode=abi.COMTOT_EXACT, census_inplace=1, queue_capacity=1))
    assert b.read_census_file(p) == len(keys)
    with pytest.raises(C2DError) as err:
        b.transport_step(gc.step_inputs(1))
    assert err.value.code == -5 and b.census_count() == 0
    q = tmp_path / "lost.dat"
    q.write_bytes(b"as it was")
    with pytest.raises(C2DError) as err:
        b.write_census_file(q)
    assert err.value.code == abi.C2D_E_STATE and q.read_bytes() == b"as it was"
    assert b.read_census_file(p) == len(keys) == b.census_count()
    assert b.write_census_file(q) == len(keys) and q.read_bytes() == text
    b.close()


def test_read_errors(work, tmp_path, fmt):
    gc, e, p, text, keys = stepped("ssc_tau", abi.COMTOT_EXACT, 0, work)
    n = len(keys)
    b = Engine(gc.grid(comtot_mode=abi.COMTOT_EXACT, census_capacity=n))
    assert b.read_census_file(p) == n
    ref = packed(b)

    def intact():
        return b.census_count() == n and np.array_equal(packed(b), ref)

    def raises(code, path, call=None):
        with pytest.raises(C2DError) as err:
            (call or b.read_census_file)(path)
        assert err.value.code == code, str(err.value)
        return str(err.value)

    raises(abi.C2D_E_IO, tmp_path / "missing.dat")
    raises(abi.C2D_E_IO, tmp_path / "missing.dat", b.parse_census_file)
    assert intact()
    # more records than the capacity: decided from the size, the census stays
    q = tmp_path / "big.dat"
    q.write_bytes(text + text[:116])
    raises(abi.C2D_E_CENSUS_OVERFLOW, q)
    assert intact()
    assert len(b.parse_census_file(q)[2]) == n + 1          # parsing alone knows no capacity
    # a garbage field, in a record the kernel takes and in one the host parser takes
    base = 116 * 280
    q = tmp_path / "garbage.dat"
    q.write_bytes(text[:base + 28] + b"   garbage    " + text[base + 42:])
    assert "byte offset %d" % (base + 28) in raises(abi.C2D_E_IO, q, b.parse_census_file)
    q.write_bytes(text[:base + 95] + b"12x45" + text[base + 100:])
    assert "byte offset %d" % (base + 95) in raises(abi.C2D_E_IO, q, b.parse_census_file)
    # an odd number of lines
    q = tmp_path / "odd.dat"
    q.write_bytes(text[:-31])
    assert "byte offset %d" % (116 * (n - 1)) in raises(abi.C2D_E_IO, q, b.parse_census_file)
    # a .keys file of the wrong size
    for size in (8 * n - 8, 8 * n + 8, 8 * n - 3):
        q = tmp_path / ("keys%d.dat" % size)
        q.write_bytes(text)
        (tmp_path / ("keys%d.dat.keys" % size)).write_bytes((keys.tobytes() + bytes(8))[:size])
        raises(abi.C2D_E_IO, q, b.parse_census_file)
    assert intact()
    # a record off the grid: C2D_E_ARG, and the census is lost until the next read
    d6, i5, k = b.parse_census_file(p)
    i5 = i5.copy()
    i5[290, 3] = gc.nz + 1
    q = tmp_path / "range.dat"
    b.write_census_records(d6, i5, k, q)
    assert "record 290 " in raises(abi.C2D_E_ARG, q)
    assert b.census_count() == 0
    raises(abi.C2D_E_STATE, None, lambda _: b.census())
    raises(abi.C2D_E_STATE, tmp_path / "w.dat", b.write_census_file)
    assert b.read_census_file(p) == n and intact()
    # an empty file: an empty census
    q = tmp_path / "empty.dat"
    q.write_bytes(b"")
    assert b.read_census_file(q) == 0 and b.census_count() == 0 and len(b.census()[2]) == 0
    d6, i5, k = b.parse_census_file(q)
    assert d6.shape == (0, 6) and i5.shape == (0, 5) and k.shape == (0,)
    b.close()
