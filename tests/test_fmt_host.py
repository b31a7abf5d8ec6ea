"""The E14.7 formatter of the escape-event file (compton2d_amd/csrc/c2d_fmt.h)
on the CPU, compiled with gcc as C99 into a small harness
(tests/c/fmt_wrap.c): its 14 bytes equal AMD flang's on the directed cases,
literally, and census_io.fortran_e14_7's (glibc's %.6e re-laid) on powers of
ten, near-half values of every decade, exact ties, carries into the next
decade, the ends of the double range, the golden escape events and 2e6 random
bit patterns.  Exact ties must take the exact (multi-limb) path, which is
also checked against Python's integers directly; non-finite input is an error
that writes nothing.  The same harness runs as a stand-alone program under
-fsanitize=address,undefined."""
import math
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fmt_cases as FC
from compton2d_amd.census_io import fortran_e14_7


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return FC.HostFmt(tmp_path_factory.mktemp("fmt"))


def test_directed_cases_equal_flang(host):
    x = np.array([v for v, _ in FC.DIRECTED])
    assert host.strings(x) == [s for _, s in FC.DIRECTED]


def test_exponent_estimate_is_floor_log10_or_one_less():
    """The header starts from k = floor(E2 * 78913 / 2^18), E2 = floor(log2 x):
    it is floor(E2 log10(2)), hence floor(log10 x) or one less."""
    for E2 in range(-1074, 1024):
        k = (E2 * 78913) >> 18
        assert 10 ** k <= 2 ** E2 < 10 ** (k + 1) if k >= 0 and E2 >= 0 else \
            Fraction(10) ** k <= Fraction(2) ** E2 < Fraction(10) ** (k + 1)


def test_stress_set_equals_python_writer(host):
    x = FC.stress_set()
    assert x.size > 2700000
    got, st, slow, bad = host.format(x)
    assert bad == 0 and set(np.unique(st)) <= {0, 1, 2}
    got = got.tobytes()
    for i, v in enumerate(x.tolist()):
        if got[14 * i:14 * i + 14].decode() != fortran_e14_7(v) and not (v == 0.0 and math.copysign(1, v) < 0):
            pytest.fail("%r (%s): header %r, python %r" % (v, float(v).hex(), got[14 * i:14 * i + 14],
                                                          fortran_e14_7(v)))


def test_ties_take_the_exact_path_and_others_do_not(host):
    """Status 1: ambiguous to the fast path, decided by the exact test for a
    (half-)integer; 2: decided by the multi-limb path (all of them with the
    shortcut off, and the bytes are the same)."""
    ties = FC.decimal_ties()
    got, st, slow, bad = host.format(ties)
    assert slow == ties.size and np.all(st == 1)
    got2, st2, slow2, _ = host.format(ties, multilimb=True)
    assert slow2 == ties.size and np.all(st2 == 2) and np.array_equal(got, got2)
    x = FC.stress_set()[:900000]
    a, sa, na, _ = host.format(x)
    b, sb, nb, _ = host.format(x, multilimb=True)
    assert np.array_equal(a, b) and na == nb > 1000 and np.array_equal(sa > 0, sb > 0) and np.all(sb[sb > 0] == 2)
    round_values = np.array([1e16, 3e15, 1e7, 1e22])                  # 1e16: an escape on the grid's boundary
    assert list(host.format(round_values)[1]) == [1, 1, 1, 1]
    # round half to even: the last kept digit is even
    last = got[:, 9] - ord("0")
    assert np.all(last % 2 == 0)
    _, st, slow, _ = host.format(FC.random_bits(20000, seed=3))
    assert slow == 0 and np.all(st == 0)
    _, st, _, _ = host.format(np.array([-3.1415926536, 0.12345675, 1e-100]))
    assert np.all(st == 0)


def test_exact_path_against_python_integers(host):
    """c2d_fmt_exact on its own (the fast path almost never sends it a value
    that is not a tie): floor and rounding class of m 2^e 10^q."""
    rng = np.random.default_rng(5)
    x = np.concatenate([FC.random_bits(3000, seed=9), FC.powers_of_ten()[::5], FC.extremes(),
                        FC.decimal_ties(20)])
    x = np.abs(x[x != 0])
    for v in x.tolist():
        m, e = math.frexp(v)
        m, e = int(m * 2 ** 53), e - 53
        while e < -1074:
            assert m % 2 == 0
            m, e = m // 2, e + 1
        k = math.floor(math.log10(v))
        for q in {6 - k, 6 - k + int(rng.integers(-1, 2))}:
            V = Fraction(m) * Fraction(2) ** e * Fraction(10) ** q
            if not (1 <= V < 2 ** 27) or not (FC_QMIN <= q <= FC_QMAX):
                continue
            D = V.numerator // V.denominator
            fr = V - D
            r = 0 if fr < Fraction(1, 2) else (1 if fr == Fraction(1, 2) else 2)
            assert host.exact(m, e, q) == (D, r), (v, q)


FC_QMIN, FC_QMAX = -304, 331


def test_nonfinite_is_an_error_and_writes_nothing(host):
    x = np.array([np.inf, 1.5, -np.inf, np.nan, -np.nan])
    got, st, slow, bad = host.format(x, fill=b"#")
    assert bad == 4 and list(st) == [-1, 0, -1, -1, -1]
    for i in (0, 2, 3, 4):
        assert bytes(got[i]) == b"#" * 14
    assert bytes(got[1]).decode() == fortran_e14_7(1.5)


def test_glibc_baseline_route_agrees(host):
    """fw_format_glibc (the benchmark's snprintf baseline) gives the same bytes."""
    import ctypes as C
    x = np.ascontiguousarray(np.concatenate([FC.random_bits(50000, seed=4), [v for v, _ in FC.DIRECTED]]))
    out = C.create_string_buffer(14 * x.size)
    host.lib.fw_format_glibc(x.ctypes.data_as(C.POINTER(C.c_double)), x.size, out)
    assert out.raw == host.format(x)[0].tobytes()


def test_standalone_program_under_host_sanitizers(tmp_path):
    """Host C only: the harness with its own main, built with ASan + UBSan and run as a program."""
    exe = tmp_path / "fmt_main"
    subprocess.run(["gcc", "-O1", "-g"] + FC.GCC_FLAGS + ["-fsanitize=address,undefined", "-static-libasan",
                    "-static-libubsan", "-fno-sanitize-recover=undefined", "-DFMT_WRAP_MAIN", "-o", str(exe), str(FC.WRAP)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "18 cases, 0 failures" in p.stdout
