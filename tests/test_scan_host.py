"""The E14.7 field parser of the escape-event reader
(compton2d_amd/csrc/c2d_scan.h) on the CPU, compiled with gcc as C99 into a
small harness (tests/c/scan_wrap.c): every field the formatter writes for its
own stress inputs, constructed decimal-to-binary ties and their neighbours,
leading-zero digit strings, signed zeros and the E-less three-digit-exponent
form at both ends of the double range give the bits of Python's float() of the
E-form, -0.0 included.  Ties must take the exact (multi-limb) path and come
out even; random fields essentially never take it; with every field forced
through it the bits are the same.  What is not canonical is reported and
writes nothing.  The same harness runs as a stand-alone program under
-fsanitize=address,undefined."""
import subprocess

import numpy as np
import pytest

import fmt_cases as FC
import scan_cases as SC


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("scan")


@pytest.fixture(scope="module")
def host(work):
    return SC.HostScan(work)


@pytest.fixture(scope="module")
def fields(work):
    return SC.field_set(work)


def first_mismatch(fields, got, want):
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        return "%d of %d differ; first %r: header %016x, python %016x" % (bad.size, len(fields), fields[i],
                                                                         int(got[i]), int(want[i]))
    return None


def test_field_set_equals_python_float(host, fields):
    assert len(fields) > 500000
    want = SC.expected_bits(fields)
    got, st, slow = host.scan(fields)
    assert set(np.unique(st)) <= {0, 1}
    assert first_mismatch(fields, got, want) is None, first_mismatch(fields, got, want)
    # both forms, both signs of zero, both ends of the range are in the set
    assert any(f[10] != "E" for f in fields) and any(f[10] == "E" for f in fields)
    z = got[[fields.index(" 0.0000000E+00"), fields.index("-0.0000000E+00")]]
    assert list(z) == [0, 1 << 63]
    e = dict(zip(fields, got))
    assert e[" 0.4940656-323"] == 1 and e[" 0.2470328-323"] == 0 and e[" 0.2470329-323"] == 1
    assert e[" 0.1797693+309"] == np.float64(1.797693e308).view(np.uint64)
    assert e[" 0.9999999+309"] == e[" 0.1797694+309"] == np.float64(np.inf).view(np.uint64)
    assert e["-0.1797693+309"] == np.float64(-1.797693e308).view(np.uint64)


def test_exact_path_everywhere_gives_the_same_bits(host, fields):
    sub = fields[::5] + tuple(SC.HAND) + tuple(f for f, _, _ in SC.constructed_ties())
    a, sa, _ = host.scan(sub)
    b, sb, nb = host.scan(sub, exact=True)
    assert np.array_equal(a, b)
    nonzero = np.array([f[3:10] != "0000000" for f in sub])
    inrange = np.array([-324 < int(SC.e_form(f).split("E")[1]) <= 315 for f in sub])
    assert np.all(sb[nonzero & inrange] == 1) and np.all(sb[~nonzero] == 0) and nb == np.count_nonzero(sb == 1)
    assert first_mismatch(sub, b, SC.expected_bits(sub)) is None


def test_constructed_ties_take_the_exact_path_and_round_to_even(host):
    ties = SC.constructed_ties()
    assert len(ties) > 100 and {k for _, _, k in ties} == set(range(13, 24))
    for f, m, k in ties:                                   # a tie indeed: the odd part has 54 bits
        assert m % 2 == 1 and (m * 5 ** k).bit_length() == 54 and abs(float(SC.e_form(f))) != m * 10 ** k
    fl = [f for f, _, _ in ties]
    got, st, slow = host.scan(fl)
    assert slow == len(fl) and np.all(st == 1)
    assert np.all(got & np.uint64(1) == 0)
    assert np.array_equal(got, SC.expected_bits(fl))
    nb = SC.tie_neighbours(ties)
    got, st, slow = host.scan(nb)
    assert np.array_equal(got, SC.expected_bits(nb))


def test_random_fields_stay_on_the_fast_path(host):
    """The fast path is ambiguous only if 64 bits of the product are all ones,
    or the round bit is followed by 73 zeros or more: about 2^-60 per field
    that is not a tie.  Genuine ties are not rare among random fields with
    exponents of 20 to 30 (D 10^(x-7) with a 54-bit odd part: 1.1 % of this
    draw); they must take the exact path like the constructed ones, so they
    are told apart with Python's integers and the bound of 1 in 10^4 is held
    on the fields that are not ties, and on all fields with exponents below
    20, where no tie exists."""
    fl = SC.random_fields()
    got, st, slow = host.scan(fl)
    assert np.array_equal(got, SC.expected_bits(fl))

    def is_tie(f):
        v, p = int(f[3:10]), int(f[11:]) - 7
        if v == 0 or p < 0:            # D / 10^n has at most 24 significant bits
            return False
        v *= 5 ** p
        return (v >> ((v & -v).bit_length() - 1)).bit_length() == 54

    tie = np.array([is_tie(f) for f in fl])
    assert np.all(st[tie] == 1)
    print("random fields: %d, exact path %d, genuine ties %d" % (len(fl), slow, np.count_nonzero(tie)))
    assert np.count_nonzero(st[~tie] == 1) < len(fl) / 10 ** 4
    low = np.array([int(f[11:]) < 20 for f in fl])
    assert not np.any(tie[low]) and np.count_nonzero(st[low] == 1) < np.count_nonzero(low) / 10 ** 4


def test_not_canonical_is_reported_and_writes_nothing(host):
    assert all(len(f) == 14 for f in SC.NOT_CANONICAL)
    got, st, slow = host.scan(SC.NOT_CANONICAL, fill=777.0)
    assert list(st) == [-1] * len(SC.NOT_CANONICAL) and slow == 0
    assert np.all(got.view(np.float64) == 777.0)
    got, st, _ = host.scan(SC.NOT_CANONICAL, exact=True, fill=777.0)
    assert list(st) == [-1] * len(SC.NOT_CANONICAL) and np.all(got.view(np.float64) == 777.0)
    # every single byte of a good field replaced by a byte that cannot stand there
    good = " 0.1234567E+01"
    for i in range(14):
        for ch in "\x00x~\xff":
            f = good[:i] + ch + good[i + 1:]
            assert host.scan([f])[1][0] == -1, (i, ch)


def test_standalone_program_under_host_sanitizers(tmp_path):
    """Host C only: the harness with its own main, built with ASan + UBSan and run as a program."""
    exe = tmp_path / "scan_main"
    subprocess.run(["gcc", "-O1", "-g"] + FC.GCC_FLAGS + ["-fsanitize=address,undefined", "-static-libasan",
                    "-static-libubsan", "-fno-sanitize-recover=undefined", "-DSCAN_WRAP_MAIN", "-o", str(exe),
                    str(SC.WRAP)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "34 cases, 0 failures" in p.stdout
