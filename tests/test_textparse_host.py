"""The host parsers of the event and census text files
(compton2d_amd/csrc/c2d_textparse.hpp: what the device parsers hand over) on
the CPU, compiled with g++ into a small harness (tests/c/textparse_wrap.cpp):
events equal observer.read_events and census records census_io.read_census bit
for bit on what Python reads, the forms Python does not read give the values
written out here, and the error cases give C2D_E_IO with the records before
them delivered.  The same harness runs as a stand-alone program over the same
files under -fsanitize=address,undefined."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fmt_cases as FC
from compton2d_amd import census_io as CI
from compton2d_amd import observer

WRAP = FC.HERE / "c" / "textparse_wrap.cpp"
GXX_FLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Werror"]
C2D_E_IO = -10
CAP = 4096


class HostParse:
    """tests/c/textparse_wrap.cpp built with g++ into `directory`."""

    def __init__(self, directory):
        so = directory / "libtextparse_wrap.so"
        subprocess.run(["g++", "-O2"] + GXX_FLAGS + ["-fPIC", "-shared", "-o", str(so), str(WRAP)], check=True)
        L = self.lib = C.CDLL(str(so))
        tail = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_char_p, C.c_int64]
        L.tw_events.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64] + tail
        L.tw_census.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + tail

    def events(self, path, chunk=1000, off=0):
        """(code, events [n, 7], the parser's count, delivery sizes, message)"""
        ev = np.zeros((CAP, 7))
        n, sizes, ns = C.c_int64(), np.zeros(64, np.int64), C.c_int32()
        err = C.create_string_buffer(768)
        rc = self.lib.tw_events(str(path).encode(), off, chunk, ev.ctypes.data, CAP, C.byref(n), sizes.ctypes.data, 64,
                                C.byref(ns), err, 768)
        return rc, ev[:n.value].copy(), n.value, list(sizes[:ns.value]), err.value.decode()

    def census(self, path, chunk=1000, base=0):
        """(code, d6, i5, keys, records delivered, delivery sizes, message)"""
        d6, i5, keys = np.zeros((CAP, 6)), np.zeros((CAP, 5), np.int32), np.zeros(CAP, np.uint64)
        n, sizes, ns = C.c_int64(), np.zeros(64, np.int64), C.c_int32()
        err = C.create_string_buffer(768)
        rc = self.lib.tw_census(str(path).encode(), base, chunk, d6.ctypes.data, i5.ctypes.data, keys.ctypes.data, CAP,
                                C.byref(n), sizes.ctypes.data, 64, C.byref(ns), err, 768)
        m = n.value - base
        return rc, d6[:m].copy(), i5[:m].copy(), keys[:m].copy(), m, list(sizes[:ns.value]), err.value.decode()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return HostParse(tmp_path_factory.mktemp("textparse"))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ---------------------------------------------------------------- the inputs
def event_values(n=10, seed=17):
    """n records: the directed values with a two-digit exponent, then random ones of either sign."""
    rng = np.random.default_rng(seed)
    x = [v for v, s in FC.DIRECTED if "E" in s]
    x += list(rng.standard_normal(7 * n - len(x)) * 10.0 ** rng.integers(-90, 90, 7 * n - len(x)))
    return np.array(x[:7 * n]).reshape(n, 7)


def tokens(ev):
    return [CI.fortran_e14_7(v).strip() for v in np.ravel(ev)]


def canonical_events(ev):
    return "".join(" ".join(CI.fortran_e14_7(v) for v in r) + "\n" for r in ev)


def event_files(d):
    """{name: path} of event files that Python reads, each with the 10 records of event_values()."""
    ev = event_values()
    t = tokens(ev)
    text = canonical_events(ev)
    seps = ["\t", "   ", " \t ", "\n", "  \n\t"]
    free = ["1.5", "-2e-3", "7", "+3.25E2", "1e-320", "-0.5E+00", ".25"]
    cases = {
        "canonical": text,
        "tabs_blanks": "".join(tok + seps[i % len(seps)] for i, tok in enumerate(t)),
        "broken_lines": "".join(tok + ("\n" if i % 3 == 2 else " ") for i, tok in enumerate(t)) + "\n",
        "crlf": text.replace("\n", "\r\n"),
        "no_final_newline": text[:-1],
        "free_form": text + " ".join(free) + "\n" + " ".join(free[::-1]),
        "empty": "",
    }
    for k in range(1, 7):
        cases["trailing_%d" % k] = text + " ".join(t[:k]) + "\n"
    paths = {}
    for name, s in cases.items():
        paths[name] = d / ("ev_%s.dat" % name)
        paths[name].write_bytes(s.encode())
    return paths


def census_values(n=7, seed=23):
    rng = np.random.default_rng(seed)
    d6 = rng.standard_normal((n, 6)) * 10.0 ** rng.integers(-90, 90, (n, 6))
    d6[0, :3] = [0.0, 1.0, -1234567.5]
    i5 = rng.integers(0, 256, (n, 5)).astype(np.int32)
    i5[1] = [0, 255, -9999, 99999, 7]
    keys = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    return d6, i5, keys


def census_files(d):
    """{name: path} of census files that read_census reads; every one has its .keys except `no_keys`."""
    d6, i5, keys = census_values()
    src = d / "cens_canonical.txt"
    CI.write_census(src, d6, i5, keys)
    text = src.read_text()
    lines = text.splitlines()
    big = d6.copy()
    big[:, 0] = [1e100, 1e-150, 4.9e-324, -1e100, 1.797693e308, -2.5e-200, 1e150]
    CI.write_census(d / "cens_eless.txt", big, i5, keys)
    assert "+101" in (d / "cens_eless.txt").read_text() and "-323" in (d / "cens_eless.txt").read_text()
    cases = {
        "crlf": text.replace("\n", "\r\n"),
        "blank_lines": "\n  \n" + "".join(s + ("\n\n" if i % 3 == 0 else "\n \t\n" if i % 3 == 1 else "\n")
                                           for i, s in enumerate(lines)),
        "lower_e": text.replace("E", "e"),
        "no_final_newline": text[:-1],
        "no_keys": text,
    }
    paths = {"canonical": src, "eless": d / "cens_eless.txt"}
    for name, s in cases.items():
        paths[name] = d / ("cens_%s.txt" % name)
        paths[name].write_bytes(s.encode())
        if name != "no_keys":
            keys.astype("<u8").tofile(str(paths[name]) + CI.KEY_SUFFIX)
    return paths


BAD_EVENTS = {   # name: (text after five canonical records, records delivered)
    "long_token": ("1 2 3 4 5 6 7\n" + "9" * 70 + " 1 2 3 4 5 6\n", 6),
    "not_a_number": ("1 2 3 abc 5 6 7\n1 2 3 4 5 6 7\n", 5),
}


def bad_event_files(d):
    head = canonical_events(event_values()[:5])   # the first five records of the canonical file
    paths = {}
    for name, (tail, _) in BAD_EVENTS.items():
        paths[name] = d / ("ev_bad_%s.dat" % name)
        paths[name].write_text(head + tail)
    return paths


def bad_census_files(d):
    d6, i5, keys = census_values()
    src = d / "cens_bad_src.txt"
    CI.write_census(src, d6, i5, keys)
    lines = src.read_text().splitlines()
    cases = {
        "odd_lines": lines[:-1],
        "asterisks": lines[:3] + ["*****" + lines[3][5:]] + lines[4:],
        "not_a_number": lines[:4] + [lines[4][:14] + " 0.12x4567E+01" + lines[4][28:]] + lines[5:],
        "short_keys": lines,
    }
    paths = {}
    for name, ls in cases.items():
        paths[name] = d / ("cens_bad_%s.txt" % name)
        paths[name].write_text("".join(s + "\n" for s in ls))
        keys[:len(keys) - (name == "short_keys")].astype("<u8").tofile(str(paths[name]) + CI.KEY_SUFFIX)
    return paths


# --------------------------------------------------------------------- events
def test_events_equal_read_events_bit_for_bit(host, tmp_path):
    want_n = {"empty": 0, "free_form": 12}
    for name, path in event_files(tmp_path).items():
        want = observer.read_events(path)
        rc, got, n, sizes, err = host.events(path)
        assert rc == 0, (name, err)
        assert n == len(want) == want_n.get(name, 10), name
        assert np.array_equal(bits(got), bits(want)), name
        assert sizes == ([n] if n else []), name


def test_events_three_digit_exponents_without_the_letter(host, tmp_path):
    """float() does not take these; the values are those that fortran_e14_7 printed the fields from."""
    want = [1e100, -0.1234567e-101, 4.9e-324, 0.1797693e309, -0.2225074e-307, 0.9999999e-100, 1.0]
    text = [" 0.1000000+101", "-0.1234567-101", " 0.4940656-323", " 0.1797693+309", "-0.2225074-307", " 0.9999999-100",
            " 0.1000000E+01"]
    assert [CI.fortran_e14_7(v) for v in want] == text
    path = tmp_path / "eless.dat"
    path.write_text(" ".join(text) + "\n" + "\t".join(s.strip() for s in text) + "\n")
    rc, got, n, _, err = host.events(path)
    assert rc == 0 and n == 2, err
    assert np.array_equal(bits(got), bits([want, want]))


def test_events_error_cases_deliver_the_records_before(host, tmp_path):
    head = observer.read_events(event_files(tmp_path)["canonical"])[:5]
    for name, path in bad_event_files(tmp_path).items():
        want_n = BAD_EVENTS[name][1]
        rc, got, n, sizes, err = host.events(path)
        assert rc == C2D_E_IO and err, name
        assert n == want_n == len(got) and sum(sizes) == n, name
        assert np.array_equal(bits(got[:5]), bits(head)), name


def test_events_in_several_deliveries(host, tmp_path):
    path = event_files(tmp_path)["canonical"]
    want = observer.read_events(path)
    for chunk, sizes_want in ((1, [1] * 10), (3, [3, 3, 3, 1]), (1000, [10])):
        rc, got, n, sizes, err = host.events(path, chunk=chunk)
        assert rc == 0 and n == 10 and sizes == sizes_want, (chunk, sizes, err)
        assert np.array_equal(bits(got), bits(want)), chunk
    # from a byte offset, as the device parser hands over: the records from the fourth on
    rc, got, n, _, err = host.events(path, off=3 * 105)
    assert rc == 0 and n == 7 and np.array_equal(bits(got), bits(want[3:])), err


# --------------------------------------------------------------------- census
def test_census_equals_read_census_bit_for_bit(host, tmp_path):
    for name, path in census_files(tmp_path).items():
        d6, i5, keys = CI.read_census(path)
        rc, g6, g5, gk, n, sizes, err = host.census(path)
        assert rc == 0, (name, err)
        assert n == len(keys) == 7 and sizes == [7], name
        assert np.array_equal(bits(g6), bits(d6)) and np.array_equal(g5, i5) and np.array_equal(gk, keys), name
        if name != "no_keys":
            assert np.array_equal(keys, census_values()[2]), name
    # derived keys count records from the `delivered` base; deliveries of two records
    path = census_files(tmp_path)["no_keys"]
    _, i5, keys = CI.read_census(path)
    seed = census_values()[2] % np.uint64(100000)
    assert [int(k) for k in keys] == [CI.derive_key(int(s), r) for r, s in enumerate(seed)]
    rc, _, g5, gk, n, sizes, err = host.census(path, chunk=2, base=1000)
    assert rc == 0 and n == 7 and sizes == [2, 2, 2, 1], err
    assert np.array_equal(g5, i5)
    assert [int(k) for k in gk] == [CI.derive_key(int(s), 1000 + r) for r, s in enumerate(seed)]


def test_census_d_exponents(host, tmp_path):
    """read_census inserts an E before the sign of a field without one and so spoils these."""
    path = tmp_path / "d.txt"
    path.write_text(" 0.1000000D+01-0.2500000d-02 0.1234567D+05 0.5000000d+00 0.1000000D+21 0.3000000d-10\n"
                    "    1    2    3    4    5    6\n")
    rc, d6, i5, keys, n, _, err = host.census(path)
    assert rc == 0 and n == 1, err
    assert np.array_equal(bits(d6[0]), bits([1.0, -0.0025, 12345.67, 0.5, 1e20, 3e-11]))
    assert list(i5[0]) == [1, 2, 3, 4, 5] and int(keys[0]) == CI.derive_key(6, 0)


def test_census_error_cases(host, tmp_path):
    for name, path in bad_census_files(tmp_path).items():
        rc, _, _, _, n, _, err = host.census(path)
        assert rc == C2D_E_IO and err, name
        assert n == 0, name            # one delivery would have held them all


# ----------------------------------------------------------------- sanitizers
def test_standalone_program_under_host_sanitizers(tmp_path):
    """Host C++ only: the harness with its own main, built with ASan + UBSan and run as a program over
    every file of the tests above; the codes and record counts it must find are the ones found here."""
    exe = tmp_path / "textparse_main"
    subprocess.run(["g++", "-O0"] + GXX_FLAGS + ["-fsanitize=address,undefined", "-static-libasan",
                    "-static-libubsan", "-fno-sanitize-recover=undefined", "-DTEXTPARSE_WRAP_MAIN", "-o", str(exe),
                    str(WRAP)], check=True)
    rows = []
    for path in event_files(tmp_path).values():
        for chunk in (1, 3, 1000):
            rows.append(("E", chunk, 0, 0, len(observer.read_events(path)), path))
    for name, path in bad_event_files(tmp_path).items():
        rows.append(("E", 1000, 0, C2D_E_IO, BAD_EVENTS[name][1], path))
    for name, path in census_files(tmp_path).items():
        for chunk, base in ((1, 0), (2, 1000 * (name == "no_keys")), (1000, 0)):
            rows.append(("C", chunk, base, 0, 7, path))
    for path in bad_census_files(tmp_path).values():
        rows.append(("C", 1000, 0, C2D_E_IO, 0, path))
    lst = tmp_path / "files.lst"
    lst.write_text("".join("%s %d %d %d %d %s\n" % r for r in rows))
    p = subprocess.run([str(exe), str(lst)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "%d files, 0 failures" % len(rows) in p.stdout
