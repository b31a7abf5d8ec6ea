"""The integer line of a census record and the whole 116-byte record
(compton2d_amd/csrc/c2d_censfmt.h) on the CPU, compiled with gcc as C99 into
a small harness (tests/c/cens_wrap.c): I5 equals census_io.fortran_i5 over
-10000..100000, asterisks included, and parses back; the derived key equals
census_io.derive_key; the records of the fixture equal the reference's own
write_cens bytes (tests/golden/census_fmt.npz) and census_io.write_census.
The same harness runs as a stand-alone program under
-fsanitize=address,undefined."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fmt_cases as FC
from compton2d_amd import census_io as CI
from golden_io import GOLDEN

WRAP = FC.HERE / "c" / "cens_wrap.c"


class HostCens:
    """tests/c/cens_wrap.c built with gcc as C99 into `directory`."""

    def __init__(self, directory):
        so = directory / "libcens_wrap.so"
        subprocess.run(["gcc", "-O2"] + FC.GCC_FLAGS + ["-fPIC", "-shared", "-o", str(so), str(WRAP)], check=True)
        L = self.lib = C.CDLL(str(so))
        L.cw_i5.argtypes = [C.c_void_p, C.c_int64, C.c_char_p]
        L.cw_scan_i5.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.cw_derive_key.restype = C.c_uint64
        L.cw_derive_key.argtypes = [C.c_int64, C.c_int64]
        L.cw_records.restype = C.c_int64
        L.cw_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p]

    def i5(self, v):
        v = np.ascontiguousarray(v, np.int64)
        out = C.create_string_buffer(5 * v.size)
        self.lib.cw_i5(v.ctypes.data, v.size, out)
        return out.raw

    def scan_i5(self, text, fill=123456):
        n = len(text) // 5
        out, st = np.full(n, fill, np.int32), np.zeros(n, np.int8)
        self.lib.cw_scan_i5(text, n, out.ctypes.data, st.ctypes.data)
        return out, st

    def records(self, d6, i5, keys):
        d6 = np.ascontiguousarray(d6, np.float64)
        i5 = np.ascontiguousarray(i5, np.int32)
        keys = np.ascontiguousarray(keys, np.uint64)
        out = C.create_string_buffer(116 * keys.size)
        bad = self.lib.cw_records(d6.ctypes.data, i5.ctypes.data, keys.ctypes.data, keys.size, out)
        return out.raw, bad


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return HostCens(tmp_path_factory.mktemp("cens"))


def test_i5_equals_fortran_i5_over_its_range_and_beyond(host):
    v = np.arange(-10000, 100001)
    got = host.i5(v).decode()
    want = "".join(CI.fortran_i5(int(x)) for x in v)
    assert got == want
    assert got[:5] == "*****" and got[5:10] == "-9999" and got[-10:-5] == "99999" and got[-5:] == "*****"
    far = np.array([-2 ** 31, 2 ** 31 - 1, -2 ** 62, 2 ** 62])
    assert host.i5(far) == b"*" * 20
    back, st = host.scan_i5(got.encode())
    assert list(st[[0, -1]]) == [-1, -1] and back[0] == back[-1] == 123456     # asterisks: nothing written
    assert np.all(st[1:-1] == 0) and np.array_equal(back[1:-1], v[1:-1])


def test_i5_parser_takes_only_the_canonical_field(host):
    bad = ["     ", "1    ", " 1 2 ", "+   1", "   +1", "  - 1", "    -", "1-   ", "  1a ", "\t   1", "****1", "0x1  ",
           "   1\n", "--  1"]
    _, st = host.scan_i5("".join(bad).encode())
    assert np.all(st == -1), [b for b, s in zip(bad, st) if s != -1]
    good = {"    0": 0, "   -0": 0, "00012": 12, "-0012": -12, "99999": 99999, "-9999": -9999}
    got, st = host.scan_i5("".join(good).encode())
    assert np.all(st == 0) and list(got) == list(good.values())


def test_derived_key_equals_census_io(host):
    rng = np.random.default_rng(3)
    for seed, index in [(0, 0), (99999, 0), (1, 2 ** 40), (-5, 7)] + [
            (int(s), int(i)) for s, i in zip(rng.integers(0, 100000, 200), rng.integers(0, 2 ** 33, 200))]:
        assert host.lib.cw_derive_key(seed, index) == CI.derive_key(seed, index), (seed, index)


def test_records_equal_the_reference_and_the_python_writer(host, tmp_path):
    fmt = np.load(GOLDEN / "census_fmt.npz", allow_pickle=False)
    d, i6 = fmt["d"], fmt["i6"]
    keys = i6[:, 5].astype(np.uint64)
    text, bad = host.records(d, i6[:, :5], keys)
    assert bad == 0 and text == bytes(fmt["text"]) and len(text) == 116 * len(keys)
    # full 64-bit keys (the sixth integer is key mod 100000), directed doubles, integers at the I5 edges
    n = 64
    rng = np.random.default_rng(5)
    x = np.array([v for v, _ in FC.DIRECTED])
    d6 = x[np.arange(6 * n) % len(x)].reshape(n, 6)
    i5 = np.array([0, 1, 9, 10, 99, 255, 99999, 100000, -1, -9999, -10000], np.int32)[
        np.arange(5 * n) % 11].reshape(n, 5)
    keys = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    text, bad = host.records(d6, i5, keys)
    assert bad == 0 and b"*****" in text
    # the doubles are flang's own bytes of the directed values ...
    s = [t for _, t in FC.DIRECTED]
    for r in range(n):
        assert text[116 * r:116 * r + 84].decode() == "".join(s[(6 * r + f) % len(s)] for f in range(6)), r
    # ... and census_io's, which writes -0.0 without its sign (flang keeps it: FC.DIRECTED[1])
    CI.write_census(tmp_path / "c.txt", d6, i5, keys)
    want = bytearray((tmp_path / "c.txt").read_bytes())
    for r, f in zip(*np.nonzero((d6 == 0) & np.signbit(d6))):
        assert want[116 * r + 14 * f] == ord(" ")
        want[116 * r + 14 * f] = ord("-")
    assert text == bytes(want)


def test_nonfinite_record_is_reported(host):
    d6 = np.ones((3, 6))
    d6[1, 4] = np.nan
    d6[2, 0] = -np.inf
    _, bad = host.records(d6, np.zeros((3, 5), np.int32), np.zeros(3, np.uint64))
    assert bad == 2


def test_entry_points_are_declared_in_every_layer():
    """The five calls in the C header, the Fortran module (compiled by
    tests/test_fortran_binding.py) and the ctypes bindings; Engine has the methods."""
    root = FC.HERE.parent
    names = ("c2d_census_write", "c2d_census_write_from", "c2d_census_read", "c2d_census_read_records",
             "c2d_last_census_file_ms")
    header = (root / "include" / "compton2d.h").read_text()
    module = (root / "include" / "compton2d_mod.f90").read_text()
    engine = (root / "compton2d_amd" / "engine.py").read_text()
    for nm in names:
        assert "int  %s(c2d_ctx* ctx" % nm in header, nm
        assert "bind(C, name='%s')" % nm in module and "end function %s\n" % nm in module, nm
        assert "lib.%s.argtypes" % nm in engine, nm
    from compton2d_amd.engine import Engine
    for m in ("write_census_file", "read_census_file", "parse_census_file", "write_census_records",
              "last_census_file", "save_census", "load_census"):
        assert callable(getattr(Engine, m))


def test_standalone_program_under_host_sanitizers(tmp_path):
    """Host C only: the harness with its own main, built with ASan + UBSan and run as a program."""
    exe = tmp_path / "cens_main"
    subprocess.run(["gcc", "-O1", "-g"] + FC.GCC_FLAGS + ["-fsanitize=address,undefined", "-static-libasan",
                    "-static-libubsan", "-fno-sanitize-recover=undefined", "-DCENS_WRAP_MAIN", "-o", str(exe),
                    str(WRAP)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failures" in p.stdout
