"""Census splitting without a GPU: the rule of csrc/c2d_split.h through its
host twins (c2d_census_split_host, c2d_census_split_keys_host) against the
numpy yardstick (compton2d_amd/popcontrol.py), the conservation of weight in
exact arithmetic, the separation and independence of the copies' streams,
and the policy functions.

The statistical bounds are stated before the data: the sample correlation of
two independent uniform samples of n pairs has standard deviation 1/sqrt(n),
the bound is 4 of them; a 16-bin chi-square of uniform draws has 15 degrees
of freedom, whose 99.9 % point is 37.7.  Seeds are fixed, so both outcomes
are deterministic.
"""
import ctypes
import dataclasses
from fractions import Fraction

import numpy as np
import pytest

import split_case as SC
from compton2d_amd import abi, engine, popcontrol as PC

NZ, NR, NG = 2, 3, 3


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def case():
    g = SC.group_table(NG)
    w = SC.ceilings(NZ, NR, NG)
    d6, i5, keys = SC.synthetic_records(4096, NZ, NR, w, g)
    for a in (d6, i5, keys, g, w):
        a.setflags(write=False)
    return d6, i5, keys, g, w


def test_derive_keys_matches_the_python_integers():
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 2 ** 64, 48, dtype=np.uint64)
    sub = rng.integers(0, 64, 48).astype(np.uint64)
    for salt in (0, 1, 2 ** 32 + 5, 2 ** 63, 2 ** 64 - 1):
        got = PC.derive_keys(keys, abi.TAG_SPLIT, salt & PC.M32, salt >> 32, sub)
        assert [PC.derive_int(int(k), abi.TAG_SPLIT, salt & PC.M32, salt >> 32, int(s)) for k, s in zip(keys, sub)] \
            == [int(x) for x in got]
    u = PC.draw_keys(keys, 3, 2)
    assert [PC.draw_int(int(k), 3, 2) for k in keys] == list(u)
    assert abi.TAG_SPLIT == 0x0D != abi.TAG_ROULETTE


def test_host_twin_equals_numpy_bit_for_bit(case):
    d6, i5, keys, g, w = case
    W = SC.record_ceilings(i5, NZ, NR, w, g)
    ew = d6[:, 4]
    plain = np.isfinite(W) & (W > 0)
    # every case the rule names is among the records
    assert (ew == W).sum() >= 100 and (ew[plain] == np.nextafter(W[plain], np.inf)).sum() >= 50
    assert (ew == 0).sum() >= 50 and (ew[plain] / W[plain] > 64).sum() >= 20
    assert (W == 0).any() and np.isinf(W).any() and np.isnan(W).any() and (W < 0).any()
    assert (i5[:, 0] == 0).any() and (i5[:, 0] == 255).any()
    ratio = np.log10(ew[plain & (ew > 0)] / W[plain & (ew > 0)])
    assert ratio.min() < -2.5 and ratio.max() > 2.5              # six decades around the ceilings
    for mc in (2, 3, 64):
        for salt in (0, 1, 2 ** 63):
            m_n, ew_n, (d6o, i5o, keyso) = PC.split_numpy(d6, i5, keys, NZ, NR, g, NG, w, mc, salt)
            m_h, ew_h, ck_h = PC.split_host(d6, i5, keys, NZ, NR, g, NG, w, mc, salt)
            assert np.array_equal(m_n, m_h) and np.array_equal(bits(ew_n), bits(ew_h))
            assert np.array_equal(keyso[len(keys):], ck_h)
            assert m_n.min() == 1 and m_n.max() == mc
            # every special ceiling, ew == W and ew == 0 give m = 1 and the weight as it was
            one = ~plain | (ew == W) | (ew == 0)
            assert np.all(m_n[one] == 1) and np.array_equal(bits(ew_n[m_n == 1]), bits(ew[m_n == 1]))
            assert np.all(m_n[plain & (ew == np.nextafter(W, np.inf))] == 2)
            assert np.all(m_n[plain & (ew / np.where(plain, W, 1.0) > 64)] == mc)
            # the output census: the originals in place, the copies behind them by (source, i)
            n, extra = len(keys), m_n.astype(np.int64) - 1
            assert len(keyso) == n + extra.sum() == len(d6o) == len(i5o)
            assert np.array_equal(keyso[:n], keys) and np.array_equal(i5o[:n], i5)
            assert np.array_equal(bits(d6o[:n, 4]), bits(ew_n))
            assert np.array_equal(bits(d6o[:n, [0, 1, 2, 3, 5]]), bits(d6[:, [0, 1, 2, 3, 5]]))
            src = np.repeat(np.arange(n), extra)
            assert np.array_equal(bits(d6o[n:, [0, 1, 2, 3, 5]]), bits(d6[src][:, [0, 1, 2, 3, 5]]))
            assert np.array_equal(bits(d6o[n:, 4]), bits(ew_n[src])) and np.array_equal(i5o[n:], i5[src])
    # the first and the last copy of one record, spelled out
    m_n, _, (_, _, keyso) = PC.split_numpy(d6, i5, keys, NZ, NR, g, NG, w, 64, 2 ** 63 + 9)
    k = int(np.flatnonzero(m_n == 64)[0])
    at = len(keys) + int((m_n[:k].astype(np.int64) - 1).sum())
    assert int(keyso[at]) == PC.derive_int(int(keys[k]), 0x0D, 9, 2 ** 31, 1)
    assert int(keyso[at + 62]) == PC.derive_int(int(keys[k]), 0x0D, 9, 2 ** 31, 63)
    # another salt gives other keys, the same counts
    a = PC.split_numpy(d6, i5, keys, NZ, NR, g, NG, w, 8, 0)
    b = PC.split_numpy(d6, i5, keys, NZ, NR, g, NG, w, 8, 1)
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[2][2], b[2][2])


def test_weight_is_conserved_in_exact_arithmetic(case):
    d6, i5, keys, g, w = case
    W = SC.record_ceilings(i5, NZ, NR, w, g)
    ew = d6[:, 4]
    tiny = np.finfo(np.float64).tiny
    on_integer = 0
    for mc in (2, 3, 64):
        m, ew_new = PC.split_copies(ew, W, mc)
        for k in np.flatnonzero(m > 1):
            e, c, mk = Fraction(float(ew[k])), Fraction(float(W[k])), int(m[k])
            if ew_new[k] >= tiny:                                   # normal: one rounding of one division
                assert abs(mk * Fraction(float(ew_new[k])) - e) <= e * Fraction(1, 2 ** 53)
            q = e / c
            exact = min(mc, -((-q.numerator) // q.denominator))     # ceil in exact arithmetic
            if mk != exact:
                # the named exception: the exact quotient lies above an integer by less than half a
                # step of the doubles there, so the rounded quotient is that integer and m is it
                fq = float(ew[k]) / float(W[k])
                assert fq == np.floor(fq) and Fraction(fq) < q and mk == int(fq) == exact - 1
                on_integer += 1
    print("records whose rounded quotient sits on an integer below the exact one:", on_integer)


def test_copy_keys_are_separate_from_everything_else(case):
    _, _, keys, _, _ = case
    salt = 12345
    m = np.full(len(keys), 64, np.int32)
    ck = PC.split_keys(keys, m, salt)
    assert len(ck) == 63 * 4096                                    # 2.6e5 keys: a chance collision ~2e-9
    rk = PC.derive_keys(keys, abi.TAG_ROULETTE, salt & PC.M32, salt >> 32)
    everything = np.concatenate([ck, keys, rk])
    assert len(np.unique(everything)) == len(everything)
    # and through the host twin
    lib = engine.load_library()
    out = np.zeros(len(ck), np.uint64)
    assert lib.c2d_census_split_keys_host(np.ascontiguousarray(keys).ctypes.data, m.ctypes.data, len(keys), salt,
                                          out.ctypes.data) == 0
    assert np.array_equal(out, ck)


def test_copies_fly_on_independent_streams():
    rng = np.random.default_rng(41)
    keys = rng.integers(0, 2 ** 64, 2000, dtype=np.uint64)
    m = np.full(2000, 8, np.int32)
    ck = PC.split_keys(keys, m, 7)
    n = len(ck)
    assert n == 14000
    u_copy, u_parent = PC.draw_keys(ck, 0), np.repeat(PC.draw_keys(keys, 0), 7)
    r = float(np.corrcoef(u_copy, u_parent)[0, 1])
    hist = np.bincount(np.minimum((u_copy * 16).astype(np.int64), 15), minlength=16)
    chi2 = float(((hist - n / 16.0) ** 2 / (n / 16.0)).sum())
    # the copies of one record among each other: copy 1 against copy 2
    r12 = float(np.corrcoef(u_copy[0::7], u_copy[1::7])[0, 1])
    print("r(copy, parent) = %.4f (bound %.4f); r(copy 1, copy 2) = %.4f (bound %.4f); chi2 = %.2f"
          % (r, 4 / np.sqrt(n), r12, 4 / np.sqrt(2000), chi2))
    assert abs(r) <= 4.0 / np.sqrt(n)
    assert abs(r12) <= 4.0 / np.sqrt(2000)
    assert chi2 < 37.7


def test_policy_functions():
    rng = np.random.default_rng(23)
    nz, nr, ng = 3, 3, 4
    count = rng.integers(40, 400, (nz, nr, ng))
    count[0, 0, 3] = 5                                              # one sparse group
    energy = count * 10.0 ** rng.uniform(-3, 3, (nz, nr, ng))
    w = PC.weight_ceiling(count, energy, 4.0)
    dense = count >= 32
    assert w.shape == count.shape and w[0, 0, 3] == 0.0 and np.all(w[dense] > 0)
    assert np.all(np.frexp(w[dense])[0] == 0.5)                     # powers of two
    raw = 4.0 * energy[dense] / count[dense]
    assert np.all(w[dense] >= raw) and np.all(w[dense] < 2.0 * raw)
    assert np.array_equal(w, PC.weight_ceiling(count, energy * (1.0 + 2.0 ** -50), 4.0))
    assert not PC.weight_ceiling(count, energy, 4.0, min_per_group=1000).any()
    for bad in (1.0, 0.5, -3.0, float("nan")):
        with pytest.raises(ValueError):
            PC.weight_ceiling(count, energy, bad)
    # multiply's tables: m = k for every positive finite ew, 1 for 0 and NaN (and inf, negative)
    g, ng1, wm = PC.multiply_tables(nz, nr)
    assert ng1 == 1 and g.shape == (abi.ROULETTE_NSP,) and wm.shape == (nz, nr, 1)
    ew = np.array([1.0, 1e-300, 1e300, 2.0 ** -1022, 0.0, np.nan, np.inf, -1.0])
    i5 = np.zeros((len(ew), 5), np.int32)
    i5[:, 0], i5[:, 3], i5[:, 4] = [0, 1, 77, 128, 255, 3, 4, 5], 1 + np.arange(len(ew)) % nz, 1
    W = SC.record_ceilings(i5, nz, nr, wm, g)
    for k in (2, 5, 64):
        m, out = PC.split_copies(ew, W, k)
        assert m.tolist() == [k, k, k, k, 1, 1, 1, 1]
        assert np.array_equal(bits(out[:4]), bits(ew[:4] / k)) and np.array_equal(bits(out[4:]), bits(ew[4:]))
    # the one corner: a subnormal weight of j steps of 5e-324 cannot become more than j records
    assert PC.split_copies(np.array([16 * 5e-324, 5e-324]), np.full(2, 5e-324), 64)[0].tolist() == [16, 1]
    ctl = PC.CensusControl(target=100)
    assert ctl.ceiling_ratio is None and ctl.max_copies == 8


class FakeEngine:
    """What apply_control asks of an engine, with a census of n records of which `heavy` would
    be split 4-fold."""

    def __init__(self, n, heavy):
        self.n, self.heavy, self.calls = n, heavy, []

    def census_count(self):
        return self.n

    def census_stats(self, g, ng):
        self.calls.append("stats")
        return np.full((1, 1, ng), self.n // ng, np.int64), np.full((1, 1, ng), float(self.n // ng))

    def census_roulette(self, g, ng, w, salt):
        raise AssertionError("the census is within its target: no roulette")

    def census_split(self, g, ng, w, mc, salt, dry_run=False):
        self.calls.append("dry" if dry_run else "split")
        assert mc == 8 and np.all(w == 4.0)                         # ratio 4 times a mean weight of 1
        out = dict(n_before=self.n, n_after=self.n + 3 * self.heavy, n_split=self.heavy, e_before=1.0, e_after=1.0,
                   kernel_ms=0.5)
        if not dry_run:
            self.n = out["n_after"]
        return out


def test_apply_control_commits_a_split_only_within_the_target():
    groups = (np.zeros(abi.ROULETTE_NSP, np.int32), 1)
    ctl = PC.CensusControl(target=1000, slack=0.25, ceiling_ratio=4.0, max_copies=8)
    e = FakeEngine(800, 100)                                        # 800 + 300 = 1100 <= 1250: committed
    row = PC.apply_control(e, ctl, groups, 3)
    assert e.calls == ["stats", "dry", "split"] and e.n == 1100
    assert (row["census_before"], row["census_after"], row["split_copies"], row["split_skipped"]) == (800, 1100, 300, False)
    assert row["split_ms"] == 1.0 and row["roulette_ms"] == 0.0
    e = FakeEngine(800, 151)                                        # 800 + 453 = 1253 > 1250: skipped
    row = PC.apply_control(e, ctl, groups, 3)
    assert e.calls == ["stats", "dry"] and e.n == 800
    assert (row["census_after"], row["split_copies"], row["split_skipped"], row["split_ms"]) == (800, 0, True, 0.5)
    e = FakeEngine(800, 0)                                          # nothing above its ceiling
    row = PC.apply_control(e, ctl, groups, 3)
    assert e.calls == ["stats", "dry"] and (row["split_copies"], row["split_skipped"]) == (0, False)
    # two ranks of 800 + 300 each: the sum 2200 decides, through stats_allreduce
    both = dataclasses.replace(ctl, stats_allreduce=lambda c, en: (2 * np.asarray(c), 2 * np.asarray(en)))
    e = FakeEngine(800, 100)
    row = PC.apply_control(e, dataclasses.replace(both, target=1600), groups, 3)
    assert row["split_skipped"] and e.n == 800 and e.calls == ["stats", "dry"]      # 2200 > 2000
    e = FakeEngine(800, 100)
    row = PC.apply_control(e, dataclasses.replace(both, target=1800), groups, 3)
    assert not row["split_skipped"] and e.n == 1100                                   # 2200 <= 2250
    # without a ratio: today's row, and the engine is not asked for a split
    e = FakeEngine(800, 100)
    row = PC.apply_control(e, PC.CensusControl(target=1000), groups, 3)
    assert row == dict(census_before=800, census_after=800, roulette_ms=0.0) and e.calls == []


def test_host_twin_refuses_bad_arguments(case):
    d6, i5, keys, g, w = case
    d6, i5, keys = d6[:16], i5[:16], keys[:16]
    ok = PC.split_host(d6, i5, keys, NZ, NR, g, NG, w, 8, 0)
    assert len(ok[0]) == 16
    for bad_ng in (0, abi.ROULETTE_GROUPS_MAX + 1):
        with pytest.raises(engine.C2DError) as e:
            PC.split_host(d6, i5, keys, NZ, NR, g, bad_ng, w, 8, 0)
        assert e.value.code == -1                                   # C2D_E_ARG
    for bad in (-1, NG):
        gb = g.copy()
        gb[77] = bad
        with pytest.raises(engine.C2DError) as e:
            PC.split_host(d6, i5, keys, NZ, NR, gb, NG, w, 8, 0)
        assert e.value.code == -1
    for bad_mc in (-1, 0, 1, abi.SPLIT_COPIES_MAX + 1):
        with pytest.raises(engine.C2DError) as e:
            PC.split_host(d6, i5, keys, NZ, NR, g, NG, w, bad_mc, 0)
        assert e.value.code == -1
    for col, val in ((3, NZ + 1), (3, 0), (4, NR + 1), (0, 256), (0, -1)):
        off = i5.copy()
        off[3, col] = val
        with pytest.raises(engine.C2DError) as e:
            PC.split_host(d6, off, keys, NZ, NR, g, NG, w, 8, 0)
        assert e.value.code == -1
    lib = engine.load_library()
    m, out = np.zeros(16, np.int32), np.zeros(16)
    args = [d6.ctypes.data, i5.ctypes.data, keys.ctypes.data, 16, NZ, NR, g.ctypes.data, NG, w.ctypes.data, 8, 0,
            m.ctypes.data, out.ctypes.data]
    assert lib.c2d_census_split_host(*args) == 0
    for k in (0, 1, 2, 6, 8, 11, 12):                               # a null pointer
        a = list(args)
        a[k] = None
        assert lib.c2d_census_split_host(*a) == -1
    assert lib.c2d_census_split_keys_host(keys.ctypes.data, np.zeros(16, np.int32).ctypes.data, 16, 0,
                                          out.ctypes.data) == -1    # copies of 0


def test_library_exports_the_entry_points():
    lib = ctypes.CDLL(str(engine.LIB_PATH))
    for name in ("c2d_census_split", "c2d_census_split_host", "c2d_census_split_keys_host"):
        assert hasattr(lib, name), name
