"""Inputs of the E14.7 formatter's tests (compton2d_amd/csrc/c2d_fmt.h): the
directed cases with AMD flang's output, the stress set of
tests/test_fmt_host.py (shared with tests/test_gpu_event_text.py) and the
gcc build of the host harness tests/c/fmt_wrap.c."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
WRAP = HERE / "c" / "fmt_wrap.c"
GCC_FLAGS = ["-std=c99", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Werror"]

# value, flang's E14.7 of it
DIRECTED = [
    (0.0, " 0.0000000E+00"), (-0.0, "-0.0000000E+00"), (1e100, " 0.1000000+101"),
    (1e-100, " 0.1000000E-99"), (1e20, " 0.1000000E+21"), (0.99999995, " 0.9999999E+00"),
    (1234567.5, " 0.1234568E+07"), (1234566.5, " 0.1234566E+07"), (-1234566.5, "-0.1234566E+07"),
    (4.9e-324, " 0.4940656-323"), (1.7976931348623157e308, " 0.1797693+309"),
    (2.2250738585072014e-308, " 0.2225074-307"), (-3.1415926536, "-0.3141593E+01"),
    (9.9999995e-100, " 0.9999999E-99"), (0.12345675, " 0.1234568E+00"), (99999995.0, " 0.1000000E+09"),
    (99999985.0, " 0.9999998E+08"), (9.9999995e22, " 0.1000000E+24"),
]
assert len(DIRECTED) == 18


def with_neighbours(x):
    x = np.asarray(x, np.float64)
    return np.concatenate([x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)])


def powers_of_ten():
    return with_neighbours([float("1e%d" % k) for k in range(-323, 309)])


def near_half(per_decade=300, seed=7):
    """The doubles nearest to d.dddddd5 x 10^k, every decade, random 7-digit prefixes."""
    rng = np.random.default_rng(seed)
    v = []
    for k in range(-323, 309):
        for p in rng.integers(1000000, 10000000, per_decade):
            x = float("%d5e%d" % (p, k - 7))
            if 0.0 < x < np.inf:
                v.append(x)
    return with_neighbours(v)


def decimal_ties(n_j=400, seed=11):
    """Exact 7-digit ties (j + 1/2) 10^p that a double holds: (2j + 1) 5^p 2^(p-1)
    for p >= 0 while (2j + 1) 5^p < 2^53, and p < 0 where 5^-p divides 2j + 1."""
    rng = np.random.default_rng(seed)
    js = np.concatenate([rng.integers(1000000, 10000000, n_j), [1000000, 9999999, 1234566, 1234567]])
    v = []
    for j in (int(j) for j in js):
        for p in range(0, 16):
            if (2 * j + 1) * 5 ** p < 2 ** 53:
                v.append(float((2 * j + 1) * 5 ** p) * 2.0 ** (p - 1))
        for p in range(1, 11):
            if (2 * j + 1) % 5 ** p == 0:
                v.append(float((2 * j + 1) // 5 ** p) * 2.0 ** (-p - 1))
    v = np.array(v)
    return np.concatenate([v, -v[::7]])


def binary_half_steps(n_j=100, seed=13):
    """(j + 1/2) 2^s for a sample of j in [1e6, 1e7) of both parities and every
    s that keeps it an exact finite double (2j + 1 has 25 bits at most)."""
    rng = np.random.default_rng(seed)
    j = rng.integers(1000000, 10000000, n_j)
    j[::2] |= 1
    j[1::2] &= ~1
    s = np.arange(-1073, 1000)
    return np.ldexp((2.0 * j + 1.0)[:, None], (s - 1)[None, :]).ravel()


def carry_cases():
    v = []
    for k in range(0, 40):
        n = 99999995 * 10 ** k
        if float(n) == n:
            v.append(float(n))
    assert len(v) >= 8
    return np.array(v)


def extremes():
    return np.array([4.9e-324, 2.225073858507201e-308, 2.2250738585072014e-308, 1.7976931348623157e308])


def golden_events():
    return np.load(HERE / "golden" / "obs.npz", allow_pickle=False)["events"]


def random_bits(n=2000000, seed=20260):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2 ** 64, n + n // 256, dtype=np.uint64)
    u = u[((u >> np.uint64(52)) & np.uint64(0x7ff)) != np.uint64(0x7ff)][:n]
    assert len(u) == n
    return u.view(np.float64)


@functools.lru_cache(maxsize=None)
def stress_set():
    """Every input of the comparison with census_io.fortran_e14_7 (about 2.8e6 values)."""
    x = np.concatenate([powers_of_ten(), near_half(), decimal_ties(), binary_half_steps(), carry_cases(),
                        extremes(), golden_events().ravel(), random_bits()])
    x = np.ascontiguousarray(x[np.isfinite(x)])
    x.setflags(write=False)
    return x


class HostFmt:
    """tests/c/fmt_wrap.c built with gcc as C99 into `directory`."""

    def __init__(self, directory):
        so = Path(directory) / "libfmt_wrap.so"
        subprocess.run(["gcc", "-O2"] + GCC_FLAGS + ["-fPIC", "-shared", "-o", str(so), str(WRAP)], check=True)
        L = self.lib = C.CDLL(str(so))
        PD = C.POINTER(C.c_double)
        L.fw_format.restype = C.c_int64
        L.fw_format.argtypes = [PD, C.c_int64, C.c_char_p, C.POINTER(C.c_int8), C.POINTER(C.c_int64)]
        L.fw_format_multilimb.restype = C.c_int64
        L.fw_format_multilimb.argtypes = L.fw_format.argtypes
        L.fw_exact.argtypes = [C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.fw_format_glibc.argtypes = [PD, C.c_int64, C.c_char_p]

    def format(self, x, fill=b"?", multilimb=False):
        """(bytes [n, 14], status [n], count off the fast path, non-finite count);
        multilimb: every ambiguous value decided by the multi-limb path."""
        x = np.ascontiguousarray(x, np.float64).ravel()
        out = C.create_string_buffer(fill * (14 * x.size), 14 * x.size)
        st = np.zeros(x.size, np.int8)
        bad = C.c_int64()
        slow = (self.lib.fw_format_multilimb if multilimb else self.lib.fw_format)(x.ctypes.data_as(C.POINTER(C.c_double)), x.size, out,
                                  st.ctypes.data_as(C.POINTER(C.c_int8)), C.byref(bad))
        return np.frombuffer(out.raw, np.uint8).reshape(-1, 14), st, slow, bad.value

    def strings(self, x):
        return [bytes(r).decode() for r in self.format(x)[0]]

    def exact(self, m, e, q):
        D, r = C.c_uint32(), C.c_int()
        self.lib.fw_exact(m, e, q, C.byref(D), C.byref(r))
        return D.value, r.value
