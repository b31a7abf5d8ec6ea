"""Census population control without a GPU: the rule of csrc/c2d_roulette.h
through its host twin (c2d_census_roulette_host) against the numpy yardstick
(compton2d_amd/popcontrol.py), the yardstick's unbiasedness, and the default
policy.

The unbiasedness bounds are derived, not measured.  One pass keeps a tested
record (ew < w) with probability p = ew / w and weight w, so its energy
afterwards has mean ew and variance ew (w - ew), and its survival is a
Bernoulli(p).  Over S = 256 independent salts the mean of E_after has
variance V / S with V = sum_tested ew (w - ew), and the mean survivor count
has variance sum p (1 - p) / S; both checks allow 4 sigma.  The inputs are
fixed, so the outcome is deterministic: with these records the energy mean is
1.09 sigma and the count mean 0.09 sigma above their expectations.
"""
import ctypes

import numpy as np
import pytest

import roulette_case as RC
from compton2d_amd import abi, engine, popcontrol as PC


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_python_integer_rng_matches_the_vectorised_one():
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 2 ** 64, 64, dtype=np.uint64)
    for salt in (0, 1, 7, 2 ** 32 + 5, 2 ** 64 - 1):
        u = PC.roulette_u(keys, salt)
        assert [PC.roulette_u_int(int(k), salt) for k in keys] == list(u)
        assert np.all((u > 0) & (u <= 1))
    # the decision does not use the packet's own stream: draw 0 of the key itself differs
    assert PC.draw_int(int(keys[0]), 0) != PC.roulette_u_int(int(keys[0]), 0)


def test_host_twin_equals_numpy_bit_for_bit():
    nz, nr, ng = 2, 3, 3
    g = RC.group_table(ng)
    w = RC.floors(nz, nr, ng)
    d6, i5, keys = RC.synthetic_records(4096, nz, nr, w, g)
    wr = PC.record_floors(i5, nz, nr, g, ng, w)
    ew = d6[:, 4]
    # every case the rule names is among the records
    assert (ew == wr).sum() >= 100 and (ew == 0).sum() >= 50
    assert (wr == 0).any() and np.isinf(wr).any() and np.isnan(wr).any() and (wr < 0).any()
    assert (i5[:, 0] == 0).any() and (i5[:, 0] == 255).any()
    plain = np.isfinite(wr) & (wr > 0) & (ew > 0)
    ratio = np.log10(ew[plain] / wr[plain])
    assert ratio.min() < -2.5 and ratio.max() > 2.5              # six decades around the floors
    for salt in (0, 3, 2 ** 40 + 9):
        keep_n, ew_n = PC.roulette_numpy(d6, i5, keys, nz, nr, g, ng, w, salt)
        keep_h, ew_h = PC.roulette_host(d6, i5, keys, nz, nr, g, ng, w, salt)
        assert np.array_equal(keep_n, keep_h)
        assert np.array_equal(bits(ew_n), bits(ew_h))
        t = PC.tested(ew, wr)
        assert keep_n[~t].all() and np.array_equal(bits(ew_n[~t]), bits(ew[~t]))
        assert np.array_equal(bits(ew_n[t & keep_n]), bits(wr[t & keep_n]))
        assert 0 < (t & keep_n).sum() < t.sum()
        assert not keep_n[t & (ew == 0)].any()
    # another salt decides differently
    assert not np.array_equal(PC.roulette_numpy(d6, i5, keys, nz, nr, g, ng, w, 0)[0],
                              PC.roulette_numpy(d6, i5, keys, nz, nr, g, ng, w, 1)[0])


def test_host_twin_refuses_bad_arguments():
    nz, nr, ng = 2, 3, 3
    g = RC.group_table(ng)
    w = RC.floors(nz, nr, ng)
    d6, i5, keys = RC.synthetic_records(16, nz, nr, w, g)
    for bad_ng in (0, abi.ROULETTE_GROUPS_MAX + 1):
        with pytest.raises(engine.C2DError) as e:
            PC.roulette_host(d6, i5, keys, nz, nr, g, bad_ng, w, 0)
        assert e.value.code == -1                                 # C2D_E_ARG
    for bad in (-1, ng):
        gb = g.copy()
        gb[77] = bad
        with pytest.raises(engine.C2DError) as e:
            PC.roulette_host(d6, i5, keys, nz, nr, gb, ng, w, 0)
        assert e.value.code == -1
    off = i5.copy()
    off[3, 3] = nz + 1
    with pytest.raises(engine.C2DError):
        PC.roulette_host(d6, off, keys, nz, nr, g, ng, w, 0)


def test_rule_is_unbiased_over_256_salts():
    nz, nr, ng = 2, 3, 3
    g = RC.group_table(ng)
    w = RC.floors(nz, nr, ng, specials=False)
    d6, i5, keys = RC.synthetic_records(20000, nz, nr, w, g, seed=17)
    ew = d6[:, 4]
    wr = PC.record_floors(i5, nz, nr, g, ng, w)
    t = PC.tested(ew, wr)
    assert t.sum() > 8000
    p = ew[t] / wr[t]
    V = float(np.sum(ew[t] * (wr[t] - ew[t])))
    e_before = float(ew.sum())
    n_expect = PC.expected_survivors(ew, wr)
    assert n_expect == pytest.approx((~t).sum() + p.sum())
    S = 256
    e_after, n_after = np.zeros(S), np.zeros(S)
    for salt in range(S):
        keep, out = PC.roulette_numpy(d6, i5, keys, nz, nr, g, ng, w, salt)
        e_after[salt] = out[keep].sum()
        n_after[salt] = keep.sum()
    sig_e = np.sqrt(V / S)
    sig_n = np.sqrt(float(np.sum(p * (1.0 - p))) / S)
    print("energy: mean - before = %.3f sigma; count: mean - expected = %.3f sigma"
          % ((e_after.mean() - e_before) / sig_e, (n_after.mean() - n_expect) / sig_n))
    assert abs(e_after.mean() - e_before) <= 4.0 * sig_e
    assert abs(n_after.mean() - n_expect) <= 4.0 * sig_n


def test_default_policy():
    rng = np.random.default_rng(23)
    nz, nr, ng = 3, 3, 4
    g = RC.group_table(ng)
    d6, i5, keys = RC.synthetic_records(6000, nz, nr, np.ones((nz, nr, ng)), g, seed=29)
    # one sparse group: a handful of records in cell (1, 1), group 3
    sparse = (i5[:, 3] == 1) & (i5[:, 4] == 1) & (g[np.minimum(i5[:, 0], abi.NPHOMAX)] == 3)
    drop = np.flatnonzero(sparse)[5:]
    sel = np.setdiff1d(np.arange(len(keys)), drop)
    d6, i5, keys = d6[sel], i5[sel], keys[sel]
    d6[:, 4] *= 10.0 ** rng.uniform(-2, 2, len(keys))
    cell = (i5[:, 3] - 1) * nr + (i5[:, 4] - 1)
    b = cell * ng + g[np.minimum(i5[:, 0], abi.NPHOMAX)]
    count = np.bincount(b, minlength=nz * nr * ng).reshape(nz, nr, ng)
    energy = np.bincount(b, weights=d6[:, 4], minlength=nz * nr * ng).reshape(nz, nr, ng)
    N = int(count.sum())
    # at or below the target: nothing
    assert not PC.weight_floor(count, energy, N).any()
    assert not PC.weight_floor(count, energy, 2 * N).any()
    target = N // 3
    w = PC.weight_floor(count, energy, target)
    assert w.shape == count.shape and count[0, 0, 3] == 5 and w[0, 0, 3] == 0.0
    dense = count >= 32
    assert dense.sum() == count.size - 1 and np.all(w[dense] > 0) and not w[~dense].any()
    m, _ = np.frexp(w[dense])
    assert np.all(m == 0.5)                                  # powers of two
    raw = (N / target) * energy[dense] / count[dense]
    assert np.all(w[dense] >= raw) and np.all(w[dense] < 2.0 * raw)
    # last-bit noise of the sums does not move a floor
    assert np.array_equal(w, PC.weight_floor(count, energy * (1.0 + 2.0 ** -50), target))
    # the bound: E[n_after] <= target + records in sparse groups
    wr = PC.record_floors(i5, nz, nr, g, ng, w)
    assert PC.expected_survivors(d6[:, 4], wr) <= target + int(count[~dense].sum())
    keep, _ = PC.roulette_numpy(d6, i5, keys, nz, nr, g, ng, w, 0)
    assert keep[b == 3].all()                                 # the sparse group is never touched
    assert keep.sum() < N
    assert PC.pow2_ceil(np.array([1.0, 1.5, 2.0, 3e-7, 2.0 ** -40])).tolist() == [1.0, 2.0, 2.0, 2.0 ** -21, 2.0 ** -40]


def test_groups_by_decade():
    from compton2d_amd import synth
    hu = synth.photon_grid()
    g, ng = PC.groups_by_decade(hu)
    assert g.shape == (abi.ROULETTE_NSP,) and g.dtype == np.int32
    assert ng == 18 and g.min() == 0 and g.max() == ng - 1       # 1e-7 .. 1e11: 18 decades
    assert g[0] == 0 and g[1] == 0 and np.all(np.diff(g[1:]) >= 0)
    assert g[11] == 4 and g[10] == 3                              # the bin that starts at 1e-3
    wide = 10.0 ** np.arange(-20.0, 21.0)
    g2, ng2 = PC.groups_by_decade(wide)
    assert ng2 == abi.ROULETTE_GROUPS_MAX and g2.max() == ng2 - 1


def test_library_exports_the_entry_points():
    lib = ctypes.CDLL(str(engine.LIB_PATH))
    for name in ("c2d_census_stats", "c2d_census_roulette", "c2d_census_roulette_host"):
        assert hasattr(lib, name), name
