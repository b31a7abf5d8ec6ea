"""Inputs of the E14.7 field parser's tests (compton2d_amd/csrc/c2d_scan.h),
shared by tests/test_scan_host.py and tests/test_gpu_event_read.py: the field
set, Python's value of a field, and the gcc build of tests/c/scan_wrap.c."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

import fmt_cases as FC

WRAP = FC.HERE / "c" / "scan_wrap.c"


def e_form(field: str) -> str:
    """The field with its exponent letter: what float() and strtod read."""
    tail = field[10:]
    return field[:10].strip() + (tail if tail[0] == "E" else "E" + tail)


def expected_bits(fields) -> np.ndarray:
    """Python's correctly rounded float() of every field, as uint64."""
    return np.array([float(e_form(f)) for f in fields], np.float64).view(np.uint64)


def field(sign: str, digits: str, x: int) -> str:
    assert len(digits) == 7 and sign in " -"
    return "%s0.%s%s" % (sign, digits, "E%+03d" % x if abs(x) < 100 else "%+04d" % x)


def constructed_ties(per_k=40, seed=17):
    """Exact decimal-to-binary ties: odd m < 10^7 with m 5^k in [2^53, 2^54), so
    that m 10^k lies halfway between two doubles (k = 13..23), as (field, m, k)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(13, 24):
        lo, hi = -(-2 ** 53 // 5 ** k), min(10 ** 7, -(-2 ** 54 // 5 ** k))
        ms = {lo | 1, hi - 1 if hi % 2 == 0 else hi - 2} | {int(v) | 1 for v in rng.integers(lo, hi, per_k)}
        for m in sorted(ms):
            if not (m % 2 == 1 and m < 10 ** 7 and 2 ** 53 <= m * 5 ** k < 2 ** 54):
                continue
            d = len(str(m))
            out.append((field(" -"[m % 3 == 0], str(m).ljust(7, "0"), d + k), m, k))
    assert any(f == " 0.7378699E+20" or f == "-0.7378699E+20" for f, _, _ in out)
    return out


def tie_neighbours(ties):
    """One unit in the 7th digit either side of each tie."""
    out = []
    for f, _, _ in ties:
        d = int(f[3:10])
        for dd in (d - 1, d + 1):
            if 0 < dd < 10 ** 7:
                out.append(f[:3] + "%07d" % dd + f[10:])
    return out


HAND = [
    " 0.0000000E+00", "-0.0000000E+00", " 0.0000000+999", "-0.0000000-999", " 0.0000000E-42",
    # leading zeros among the digits
    " 0.0000001E+00", "-0.0012345E-05", " 0.0999999E+17", " 0.0000001-300", " 0.0000001-310", " 0.0000001-316",
    " 0.0000001-317", " 0.0000049-318", " 0.0000001+315", " 0.0000001+316", " 0.0000017+315", " 0.0000018+315",
    " 0.0100000E+02", " 0.0000123+012",
    # the E-less form at both ends
    " 0.4940656-323", " 0.2225074-307", " 0.1797693+309", " 0.9999999+309", "-0.4940656-323", "-0.1797693+309",
    " 0.2470328-323", " 0.2470329-323", " 0.7410984-323", " 0.7410985-323", " 0.1797694+309", " 0.2225073-307",
    " 0.2225075-307", " 0.9999999-999", " 0.9999999+999", " 0.1000000-330", " 0.1000000+310", " 0.1234567+100",
    " 0.1234567-100", " 0.1234567+007", " 0.9999999-322", " 0.1000000-322",
]

NOT_CANONICAL = [
    "\t0.1234567E+01",        # a tab as pad
    "0.1234567E+01 ",         # 13 bytes left-justified
    " 1.2345678E+01",
    " 0.12a4567E+01",         # a letter among the digits
    "           NaN",
    " 0.1234567E 01",         # no sign in the exponent
    " 0.1234567E+1 ", " 0.1234567e+01", "  .1234567E+01", "+0.1234567E+01", " 0,1234567E+01", " 0.1234567+1E2",
    " 0.1234567D+01", "      Infinity", " 0.1234567E+0\n", "\n0.1234567E+01", " 0.123456:E+01", " 0.123456/E+01",
]


def to_bytes(fields) -> bytes:
    b = "".join(fields).encode("latin-1")
    assert len(b) == 14 * len(fields)
    return b


@functools.lru_cache(maxsize=None)
def field_set(directory):
    """The fields of both tests, unique, as a tuple of 14-character strings."""
    host = FC.HostFmt(directory)
    x = np.concatenate([FC.stress_set()[::4], [v for v, _ in FC.DIRECTED], FC.powers_of_ten(), FC.carry_cases(),
                        FC.golden_events().ravel()])
    x = x[np.isfinite(x)]
    raw = host.format(x)[0].tobytes().decode()
    written = {raw[14 * i:14 * i + 14] for i in range(x.size)}
    ties = constructed_ties()
    hand = [f for f, _, _ in ties] + tie_neighbours(ties) + HAND
    return tuple(sorted(written | set(hand)))


def random_fields(n=200000, seed=23):
    """Random 7-digit fields with exponents in -30..30."""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 10 ** 7, n)
    x = rng.integers(-30, 31, n)
    s = rng.integers(0, 2, n)
    return [field(" -"[int(k)], "%07d" % int(a), int(b)) for a, b, k in zip(d, x, s)]


class HostScan:
    """tests/c/scan_wrap.c built with gcc as C99 into `directory`."""

    def __init__(self, directory):
        so = Path(directory) / "libscan_wrap.so"
        subprocess.run(["gcc", "-O2"] + FC.GCC_FLAGS + ["-fPIC", "-shared", "-o", str(so), str(WRAP)], check=True)
        L = self.lib = C.CDLL(str(so))
        L.sw_scan.restype = C.c_int64
        L.sw_scan.argtypes = [C.c_char_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_int8), C.c_int]

    def scan(self, fields, exact=False, fill=12345.0):
        """(bits uint64 [n], status int8 [n], how many took the exact path)."""
        text = fields if isinstance(fields, bytes) else to_bytes(fields)
        n = len(text) // 14
        out = np.full(n, fill, np.float64)
        st = np.zeros(n, np.int8)
        slow = self.lib.sw_scan(text, n, out.ctypes.data_as(C.POINTER(C.c_double)),
                                st.ctypes.data_as(C.POINTER(C.c_int8)), int(exact))
        return out.view(np.uint64), st, slow
