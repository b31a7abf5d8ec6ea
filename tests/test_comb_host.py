"""The census comb without a GPU: the critical floor of csrc/c2d_comb.h in
numpy (popcontrol.comb_critical) against the library's host twin
(c2d_census_comb_host), the search for the comb's t, its agreement with the
roulette, and its unbiasedness.

The unbiasedness bound is derived, not measured.  Given the floors, one pass
keeps a tested record (ew < w) with probability ew / w and weight w, so a
tally sum coef_i ew'_i has variance sum coef_i^2 ew_i max(0, w_i - ew_i).  The
comb's floors depend on the salt, so V is the mean of that sum over the
salts at the floors each realised; conditional on the other records'
priorities a record's survival is still the roulette's (Duffield, Lund &
Thorup 2007), and priority sampling's covariances are zero, so V is the
variance scale of the tally and the mean over S = 256 salts is allowed
4 sqrt(V / S).  The inputs are fixed, so the outcome is deterministic.
"""
import numpy as np
import pytest

import comb_case as CC
from compton2d_amd import abi, engine, popcontrol as PC

NZ, NR, NG = CC.NZ, CC.NR, CC.NG
DBL_MAX = np.finfo(np.float64).max
TINY_NORMAL = np.finfo(np.float64).tiny


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_critical(ew, u, w):
    """w = w*: S(w) holds and S one step above does not."""
    pos = ew > 0
    assert np.all(w[~pos] == 0) and not np.signbit(w[~pos]).any()
    assert np.all(np.isfinite(w)) and np.all(w[pos] > 0)
    assert PC._survives(ew[pos], u[pos], w[pos]).all()
    with np.errstate(over="ignore"):                         # the step above DBL_MAX is +inf
        above = np.nextafter(w[pos], np.inf)
    assert not PC._survives(ew[pos], u[pos], above).any()


# ------------------------------------------------------- 1. the critical floor
def test_critical_floor_is_the_last_floor_survived():
    g, nm = CC.groups(), CC.norms(specials=False)
    d6, i5, keys = CC.records(4096, nm, bad=False)
    ew = d6[:, 4]
    assert (ew == 0).sum() >= 50 and np.log10(ew[ew > 0].max() / ew[ew > 0].min()) > 6
    for salt in (0, 5, 2 ** 40 + 9):
        u = PC.roulette_u(keys, salt)
        check_critical(ew, u, PC.comb_wstar(ew, u))
    # the smallest normal, a weight whose quotient overflows for a small draw, exact quotients
    u = PC.roulette_u(keys, 1)
    u[:64] = 2.0 ** -np.arange(1, 65)[::-1] * 1.5        # down to 1.5 * 2^-64: 1e300 / u is infinite
    for ew1 in (np.full(len(u), TINY_NORMAL), np.full(len(u), 1e300), u * 8.0, u * 2.0 ** -1000):
        w = PC.comb_wstar(ew1, u)
        check_critical(ew1, u, w)
    w = PC.comb_wstar(np.full(len(u), 1e300), u)
    assert (w[:8] == DBL_MAX).all() and (w < DBL_MAX).any()
    exact = PC.comb_wstar(u * 8.0, u)                      # ew / u = 8 exactly: S(8) is u < u
    assert (exact == np.nextafter(8.0, 0.0)).all()
    assert PC.comb_wstar(np.zeros(3), u[:3]).tolist() == [0.0, 0.0, 0.0]


def test_host_twin_equals_numpy_bit_for_bit():
    g, nm = CC.groups(), CC.norms()
    d6, i5, keys = CC.records(4096, nm)
    d6[30, 4], d6[31, 4] = TINY_NORMAL, 1e300
    i5[40, 3], i5[41, 4], i5[42, 3], i5[43, 4] = 0, 0, NZ + 1, NR + 1          # cells off the grid
    rec_norm = np.where((i5[:, 3] >= 1) & (i5[:, 3] <= NZ) & (i5[:, 4] >= 1) & (i5[:, 4] <= NR),
                        nm[np.clip(i5[:, 3], 1, NZ) - 1, np.clip(i5[:, 4], 1, NR) - 1,
                           g[np.minimum(i5[:, 0], abi.NPHOMAX)]], -1.0)
    ew = d6[:, 4]
    # every case the rule names is among the records
    assert (ew < 0).any() and np.isnan(ew).any() and np.isposinf(ew).any() and np.isneginf(ew).any()
    assert (ew == 0).sum() >= 50 and (i5[:, 0] == 0).any() and (i5[:, 0] == 255).any()
    assert (rec_norm == 0).any() and np.isinf(rec_norm).any() and np.isnan(rec_norm).any()
    with np.errstate(invalid="ignore"):
        want_fixed = ~((rec_norm > 0) & np.isfinite(rec_norm) & (ew >= 0) & np.isfinite(ew))
    for salt in (0, 3, 2 ** 40 + 9):
        c_n, f_n = PC.comb_critical(d6, i5, keys, NZ, NR, g, NG, nm, salt)
        c_h, f_h = PC.comb_critical_host(d6, i5, keys, NZ, NR, g, NG, nm, salt)
        assert np.array_equal(f_n, f_h) and np.array_equal(f_n, want_fixed)
        assert np.array_equal(bits(c_n), bits(c_h))
        assert 300 < f_n.sum() < 1500 and (c_n[f_n] == 0).all() and (c_n[~f_n & (ew > 0)] > 0).all()
        # c is w* / norm, exactly unless it leaves the normal range (the smallest normal weight's
        # does): the record survives the floor c * norm and not the next one
        p = ~f_n & ~((c_n > 0) & (c_n < TINY_NORMAL)) & np.isfinite(c_n)
        assert p.sum() >= (~f_n).sum() - 1
        check_critical(ew[p], PC.roulette_u(keys[p], salt), c_n[p] * rec_norm[p])
    assert not np.array_equal(bits(PC.comb_critical(d6, i5, keys, NZ, NR, g, NG, nm, 0)[0]),
                              bits(PC.comb_critical(d6, i5, keys, NZ, NR, g, NG, nm, 1)[0]))


# ------------------------------------------- 2. consistency with the roulette
def test_floors_keep_exactly_the_records_above_t():
    g = CC.groups()
    d6, i5, keys = CC.records(4096)
    n = len(keys)
    seen = set()
    for salt in range(64):
        n_fixed = None
        for target in (None, 1500, 3000, n - 100):           # n - 100: all but the 64 of weight 0 and 36 more
            if target is None:                               # the least a pass can leave: one pool record
                target = int(CC.policy_cpu(d6, i5, keys, g, NG, n - 1, salt)[4].sum()) + 1
            w_min, t, norm, crit, fixed, info = CC.policy_cpu(d6, i5, keys, g, NG, target, salt)
            n_fixed = int(fixed.sum())
            assert 300 < n_fixed < 1400                      # the bins of the NaN and infinite weights
            keep, ew_new = PC.roulette_numpy(d6, i5, keys, NZ, NR, g, NG, w_min, salt)
            assert np.array_equal(keep, fixed | (crit >= t))
            assert int(keep.sum()) == target
            assert info["quota"] == target - n_fixed and info["n_pool"] == n - n_fixed
            # a survivor weighs max(ew, floor)
            wr = PC.record_floors(i5, NZ, NR, g, NG, w_min)
            s = keep & ~fixed
            assert np.array_equal(bits(ew_new[s]), bits(np.maximum(d6[s, 4], wr[s])))
            seen.add(info["passes"])
    assert seen == {1}                                       # 4096 values: one histogram, then collect


def test_ties_leave_at_most_the_target():
    g = CC.groups()
    d6, i5, keys = CC.records(2048, bad=False)
    d6, i5, keys = np.tile(d6, (2, 1)), np.tile(i5, (2, 1)), np.tile(keys, 2)
    hit = []
    for target in (1000, 1001, 2500, 2501):
        w_min, t, norm, crit, fixed, info = CC.policy_cpu(d6, i5, keys, g, NG, target, 9, collect_cap=1)
        assert info["passes"] == 6 and info["collected"] == 0      # a pair of equal values never shrinks to one
        keep, _ = PC.roulette_numpy(d6, i5, keys, NZ, NR, g, NG, w_min, 9)
        n_after = int(keep.sum())
        assert n_after == int((fixed | (crit >= t)).sum()) and target - 1 <= n_after <= target
        hit.append(n_after == target)
    assert sorted(hit[:2]) == [False, True] and sorted(hit[2:]) == [False, True]


# ------------------------------------------------------------ 3. unbiasedness
def test_comb_is_unbiased_and_exact_over_256_salts():
    d6, i5, keys, g, ng, b = CC.lognormal_case()
    ew = d6[:, 4]
    n, target, S = len(ew), 1000, 256
    rng = np.random.default_rng(77)
    coefs = dict(random=rng.uniform(0.0, 2.0, n), group=(b == 3).astype(float),
                 cell=(i5[:, 3] == 1).astype(float))
    got = {k: np.zeros(S) for k in coefs}
    var = {k: np.zeros(S) for k in coefs}
    for salt in range(S):
        w_min, t, norm, crit, fixed, info = CC.policy_cpu(d6, i5, keys, g, ng, target, salt)
        assert not fixed.any()
        keep, ew_new = PC.roulette_numpy(d6, i5, keys, NZ, NR, g, ng, w_min, salt)
        assert int(keep.sum()) == target                     # exactly, on every salt
        wr = PC.record_floors(i5, NZ, NR, g, ng, w_min)
        for k, c in coefs.items():
            got[k][salt] = float((c * ew_new)[keep].sum())
            var[k][salt] = float((c * c * ew * np.maximum(0.0, wr - ew)).sum())
    for k, c in coefs.items():
        truth, V = float((c * ew).sum()), float(var[k].mean())
        dev = (got[k].mean() - truth) / np.sqrt(V / S)
        print("%s: truth %.6g, mean %.6g, deviation %.2f sigma, realised variance %.2f V, scatter %.1f %%" % (
            k, truth, got[k].mean(), dev, got[k].var() / V, 100 * got[k].std() / truth))
        assert abs(dev) <= 4.0


# ---------------------------------------------------- 4. sharding, both routes
def test_shards_and_routes_give_the_same_t():
    g = CC.groups()
    d6, i5, keys = CC.records(4096)
    for salt, target in ((0, 1500), (1, 700), (2, 4000)):
        t0, info0 = CC.policy_cpu(d6, i5, keys, g, NG, target, salt)[1::4]
        assert info0["passes"] == 1 and info0["collected"] > 0
        t_sh = CC.policy_cpu(d6, i5, keys, g, NG, target, salt, shards=2)[1]
        t_hist, info_h = CC.policy_cpu(d6, i5, keys, g, NG, target, salt, collect=False)[1::4]
        t_mix, info_m = CC.policy_cpu(d6, i5, keys, g, NG, target, salt, shards=2, collect_cap=20)[1::4]
        assert info_h["passes"] == 6 and info_h["collected"] == 0
        assert 1 < info_m["passes"] < 6 and 0 < info_m["collected"] <= 20
        assert bits(t0) == bits(t_sh) == bits(t_hist) == bits(t_mix)


def test_histogram_digits():
    """The six digits of comb_hist_numpy put a value's 64 bits together again."""
    rng = np.random.default_rng(1)
    c = np.abs(rng.standard_normal(500)) * 10.0 ** rng.integers(-300, 300, 500)
    fixed = np.zeros(500, bool)
    fixed[::7] = True
    v = bits(c)[13]
    prefix = 0
    for pb in abi.COMB_PREFIX_BITS:
        hist, counts = PC.comb_hist_numpy(c, fixed, prefix, pb)
        assert counts.tolist()[:3] == [500, 72, 428] and hist.sum() == counts[3] >= 1
        width = 9 if pb == 55 else 11
        d = int(v >> np.uint64(64 - pb - width)) & ((1 << width) - 1)
        assert hist[d] >= 1 and hist[1 << width:].sum() == 0
        prefix = (prefix << width) | d
    assert prefix == int(v)


# ------------------------------------------------- 5. refusals, special cases
def test_refusals_and_special_cases():
    g, nm = CC.groups(), CC.norms()
    d6, i5, keys = CC.records(500, nm)
    bad = nm.copy()
    bad[2, 1, 3] = 3.0
    with pytest.raises(ValueError, match="power of two"):
        PC.comb_critical(d6, i5, keys, NZ, NR, g, NG, bad, 0)
    with pytest.raises(engine.C2DError) as err:
        PC.comb_critical_host(d6, i5, keys, NZ, NR, g, NG, bad, 0)
    assert err.value.code == -1
    bad[2, 1, 3] = 2.0 ** -1074                              # the smallest power of two there is
    assert np.array_equal(bits(PC.comb_critical(d6, i5, keys, NZ, NR, g, NG, bad, 0)[0]),
                          bits(PC.comb_critical_host(d6, i5, keys, NZ, NR, g, NG, bad, 0)[0]))
    gb = np.array(g)
    gb[5] = NG
    for call in (PC.comb_critical, PC.comb_critical_host):
        with pytest.raises((ValueError, engine.C2DError)):
            call(d6, i5, keys, NZ, NR, gb, NG, nm, 0)
    crit, fixed = PC.comb_critical(d6, i5, keys, NZ, NR, g, NG, nm, 0)
    for prefix, pb in ((0, 7), (0, 66), (1, 0), (1 << 11, 11), (-1, 11)):
        with pytest.raises(ValueError, match="prefix"):
            PC.comb_hist_numpy(crit, fixed, prefix, pb)
    # the target against what the protected records hold, and against the census
    d6, i5, keys = CC.records(4096)
    n = len(keys)
    n_fixed = int(CC.policy_cpu(d6, i5, keys, g, NG, n - 1, 4)[4].sum())
    assert 0 < n_fixed < n
    for target in (n_fixed, n_fixed - 5, 1):
        with pytest.raises(ValueError, match="protected"):
            CC.policy_cpu(d6, i5, keys, g, NG, target, 4)
    with pytest.raises(ValueError):
        CC.policy_cpu(d6, i5, keys, g, NG, 0, 4)
    assert int(PC.roulette_numpy(d6, i5, keys, NZ, NR, g, NG,
                                 CC.policy_cpu(d6, i5, keys, g, NG, n_fixed + 1, 4)[0], 4)[0].sum()) == n_fixed + 1
    for target in (n, n + 1, 10 * n):
        w_min, t, norm, _, _, info = CC.policy_cpu(d6, i5, keys, g, NG, target, 4)
        assert t is None and not w_min.any() and w_min.shape == (NZ, NR, NG) and info["passes"] == 1
