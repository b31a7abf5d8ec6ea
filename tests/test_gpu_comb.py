"""The census comb on the GPU (c2d_census_comb_hist, c2d_census_comb_collect;
csrc/comb.hip) against the host twin and the numpy yardstick
(compton2d_amd/popcontrol.py): the digit histograms and the collected values
in both census modes and both builds, that the census is only read, the whole
policy followed by the roulette pass, two contexts, the refusals, and
CoupledRun with CensusControl(exact=True).

Counts, histograms, values, keys and ew are exact.  The roulette's e_after is
a sum of f64 atomics in any order: 1e-12 relative (at most 5137 terms of one
sign: n * 2^-53 = 6e-13), as in test_gpu_roulette.py.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import comb_case as CC
from compton2d_amd import abi, popcontrol as PC, synth
from compton2d_amd.coupled import CoupledRun
from compton2d_amd.engine import C2DError, Engine
from golden_io import GoldenCase

pytestmark = pytest.mark.gpu

NZ, NR, NG = CC.NZ, CC.NR, CC.NG
CAP = 1 << 17
SALT = 5
MODES = [(0, abi.COMTOT_EXACT), (1, abi.COMTOT_EXACT), (0, abi.COMTOT_TABLE), (1, abi.COMTOT_TABLE)]


def grid_of(inplace, mode, capacity=CAP):
    wl = synth.c2_workload(nz=NZ, nr=NR, sources=9, comtot_mode=mode, census_capacity=capacity,
                           event_capacity=1 << 10)
    return dataclasses.replace(wl.grid, census_inplace=inplace, queue_capacity=1 << 10)


@pytest.fixture(scope="module")
def pool():
    """(d6, i5, keys, g, norm, crit, fixed): 70 000 records with every kind of
    fixed record among the first 40, normalisers with 0, inf and NaN, and the
    host twin's (crit, fixed) under SALT; left unchanged by every test."""
    g, nm = CC.groups(), CC.norms()
    d6, i5, keys = CC.records(CC.N_GRID3, nm)
    assert len(np.unique(keys)) == len(keys)
    crit, fixed = PC.comb_critical_host(d6, i5, keys, NZ, NR, g, NG, nm, SALT)
    for a in (d6, i5, keys, g, nm, crit, fixed):
        a.setflags(write=False)
    return d6, i5, keys, g, nm, crit, fixed


@pytest.fixture(scope="module", params=MODES, ids=lambda p: "inplace%d-%s" % (p[0], "fast" if p[1] else "exact"))
def eng(request):
    inplace, mode = request.param
    with Engine(grid_of(inplace, mode)) as e:
        yield e


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), a.nbytes // max(len(a), 1))


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def by_key(d6, i5, keys):
    o = np.argsort(keys, kind="stable")
    return d6[o], i5[o], keys[o]


def median_bits(crit, fixed) -> int:
    """The bit pattern of the pool's median value (0 for an empty pool)."""
    p = np.sort(u64(crit[~fixed]))
    return int(p[len(p) // 2]) if len(p) else 0


def check_hists(e, d6, i5, keys, g, nm, crit, fixed):
    n = len(keys)
    e.import_census(d6, i5, keys)
    pre = e.census()
    v = median_bits(crit, fixed)
    for pb in (0, 11, 22, 55):
        prefix = v >> (64 - pb) if pb else 0
        hist, out = e.census_comb_hist(g, NG, nm, SALT, prefix, pb)
        want, counts = PC.comb_hist_numpy(crit, fixed, prefix, pb)
        np.testing.assert_array_equal(hist, want)
        assert [out["n_records"], out["n_fixed"], out["n_pool"], out["n_match"]] == counts.tolist()
        assert out["n_records"] == n and out["n_match"] == hist.sum() and out["kernel_ms"] > 0
        if counts[2]:
            assert out["n_match"] >= 1                                  # the median itself
    assert e.census_count() == n
    for a, b in zip(pre, e.census()):
        np.testing.assert_array_equal(bits(a), bits(b))


# ------------------------------------------------------------- 1. histograms
def test_hist_equals_the_yardstick(eng, pool, monkeypatch):
    d6, i5, keys, g, nm, crit, fixed = pool
    assert fixed[:64].any() and not fixed[:64].all()
    for n in CC.SIZES:
        check_hists(eng, d6[:n], i5[:n], keys[:n], g, nm, crit[:n], fixed[:n])
    monkeypatch.setenv("C2D_COMB_GRID", "3")                            # 69 tiles over 3 workgroups
    check_hists(eng, d6, i5, keys, g, nm, crit, fixed)
    # an empty census: zeros, and no kernel
    eng.census_truncate(0)
    hist, out = eng.census_comb_hist(g, NG, nm, SALT)
    assert not hist.any() and (out["n_records"], out["n_pool"], out["n_match"]) == (0, 0, 0)


# ---------------------------------------------------------------- 2. collect
def test_collect_equals_the_yardstick(eng, pool, monkeypatch):
    d6, i5, keys, g, nm, crit, fixed = pool
    for n, grid in ((CC.SIZES[1], None), (CC.SIZES[-1], None), (CC.N_GRID3, "3")):
        if grid:
            monkeypatch.setenv("C2D_COMB_GRID", grid)
        eng.import_census(d6[:n], i5[:n], keys[:n])
        pre = eng.census()
        v = median_bits(crit[:n], fixed[:n])
        for pb in (0, 11, 55):
            prefix = v >> (64 - pb) if pb else 0
            p = crit[:n][~fixed[:n]]
            want = np.sort(u64(p[PC.comb_match(p, prefix, pb)]))
            vals, cnt = eng.census_comb_collect(g, NG, nm, SALT, prefix, pb, len(want) + 3)
            assert cnt == len(want) >= 1 and len(vals) == cnt
            np.testing.assert_array_equal(np.sort(u64(vals)), want)
        # a short buffer: the full count, and nothing past cap
        p = crit[:n][~fixed[:n]]
        cap = len(p) // 2
        buf = np.full(len(p), -7.0)
        cnt = C.c_int64()
        assert eng.lib.c2d_census_comb_collect(eng.ctx, g.ctypes.data, NG, nm.ctypes.data, SALT, 0, 0,
                                               buf.ctypes.data, cap, C.byref(cnt)) == 0
        assert cnt.value == len(p) > cap
        assert (buf[cap:] == -7.0).all() and np.isin(u64(buf[:cap]), u64(p)).all()
        assert eng.census_comb_collect(g, NG, nm, SALT, 0, 0, 0)[1] == len(p)
        for a, b in zip(pre, eng.census()):
            np.testing.assert_array_equal(bits(a), bits(b))


# ------------------------------------------------------------- 3. end to end
def finite_records(pool, n):
    d6, i5, keys = pool[0][:n].copy(), pool[1][:n], pool[2][:n]
    d6[20:24, 4] = (3.0, 0.25, 40.0, 1e-3)                  # for the NaN and infinite weights: e_after is checked
    return d6, i5, keys


def check_end_to_end(e, d6, i5, keys, g, target, salt, **kw):
    n = len(keys)
    e.import_census(d6, i5, keys)
    count, energy = e.census_stats(g, NG)
    w_min, info = PC.comb_floor(e, (g, NG), count, energy, target, salt, **kw)
    assert e.census_count() == n
    out = e.census_roulette(g, NG, w_min, salt)
    keep, ew_new = PC.roulette_numpy(d6, i5, keys, NZ, NR, g, NG, w_min, salt)
    assert out["n_after"] == target == int(keep.sum()) == e.census_count()
    post = by_key(*e.census())
    np.testing.assert_array_equal(post[2], np.sort(keys[keep]))
    o = np.argsort(keys, kind="stable")
    np.testing.assert_array_equal(u64(post[0][:, 4]), u64(ew_new[o][keep[o]]))
    assert out["e_after"] == pytest.approx(float(ew_new[keep].sum()), rel=1e-12, abs=0.0)
    # the yardstick's own policy finds the same t from the same statistics
    norm = PC.comb_norm(count, energy)
    crit, fixed = PC.comb_critical(d6, i5, keys, NZ, NR, g, NG, norm, salt)
    hp, cp = CC.passes([(crit, fixed)])
    assert PC.comb_threshold(hp, cp, target)[0] == info["t"]
    np.testing.assert_array_equal(keep, fixed | (crit >= info["t"]))
    return w_min, info


def test_comb_floor_then_roulette_leaves_the_target(eng, pool):
    g = pool[3]
    d6, i5, keys = finite_records(pool, CC.SIZES[-1])
    n = len(keys)
    for salt, target in ((1, n // 4), (2, 1000), (3, n - 200)):
        w_a, info_a = check_end_to_end(eng, d6, i5, keys, g, target, salt)
        assert info_a["passes"] == 1 and 0 < info_a["collected"] <= n
        w_b, info_b = check_end_to_end(eng, d6, i5, keys, g, target, salt, collect_cap=8)
        assert 1 < info_b["passes"] <= 6 and info_b["collected"] <= 8
        w_c, info_c = check_end_to_end(eng, d6, i5, keys, g, target, salt, hist_allreduce=lambda h, c: (h, c))
        assert info_c["passes"] == 6 and info_c["collected"] == 0 and info_c["comb_ms"] > 0
        np.testing.assert_array_equal(w_a, w_b)
        np.testing.assert_array_equal(w_a, w_c)
    # a target the census already meets: no floor, the census stays
    eng.import_census(d6, i5, keys)
    count, energy = eng.census_stats(g, NG)
    w0, info = PC.comb_floor(eng, (g, NG), count, energy, n, 4)
    assert not w0.any() and info["t"] is None and info["passes"] == 1
    with pytest.raises(ValueError, match="protected"):
        PC.comb_floor(eng, (g, NG), count, energy, 1, 4, min_per_group=n)      # every group sparse: all fixed


# ----------------------------------------------------------- 4. two contexts
class Rank:
    """One context of two: remembers its last call, so that the host-side
    `allreduce` and `gather` can ask the other context for the same pass."""

    def __init__(self, eng, other):
        self.eng, self.other, self.last = eng, other, None

    def census_comb_hist(self, *a):
        self.last = a
        return self.eng.census_comb_hist(*a)

    def census_comb_collect(self, *a):
        self.last = a
        return self.eng.census_comb_collect(*a)

    def allreduce(self, hist, counts):
        h, out = self.other.census_comb_hist(*self.last)
        return hist + h, counts + np.array([out["n_records"], out["n_fixed"], out["n_pool"], out["n_match"]])

    def gather(self, vals):
        return np.concatenate([vals, self.other.census_comb_collect(*self.last)[0]])


def test_two_contexts_share_one_comb(pool):
    g = pool[3]
    d6, i5, keys = finite_records(pool, CC.SIZES[-1])
    n, target, salt = len(keys), len(keys) // 3, 6
    with Engine(grid_of(1, abi.COMTOT_EXACT)) as one:
        one.import_census(d6, i5, keys)
        count, energy = one.census_stats(g, NG)
        w, info = PC.comb_floor(one, (g, NG), count, energy, target, salt)
        assert one.census_roulette(g, NG, w, salt)["n_after"] == target
        single = by_key(*one.census())
    shards = [Engine(grid_of(r, abi.COMTOT_EXACT)) for r in (0, 1)]
    try:
        c_sum, e_sum = np.zeros_like(count), np.zeros_like(energy)
        for r, e in enumerate(shards):
            e.import_census(d6[r::2], i5[r::2], keys[r::2])
            c, en = e.census_stats(g, NG)
            c_sum += c
            e_sum += en
        np.testing.assert_array_equal(PC.comb_norm(c_sum, e_sum), PC.comb_norm(count, energy))
        parts, total = [], 0
        for r, e in enumerate(shards):
            rank = Rank(e, shards[1 - r])
            w_r, info_r = PC.comb_floor(rank, (g, NG), c_sum, e_sum, target, salt, hist_allreduce=rank.allreduce,
                                        gather=rank.gather)
            np.testing.assert_array_equal(w_r, w)
            assert info_r["t"] == info["t"] and info_r["n_pool"] == info["n_pool"] and info_r["collected"] > 0
            w_h, info_h = PC.comb_floor(rank, (g, NG), c_sum, e_sum, target, salt, hist_allreduce=rank.allreduce)
            np.testing.assert_array_equal(w_h, w)
            assert info_h["passes"] == 6 and info_h["collected"] == 0
        for e in shards:
            total += e.census_roulette(g, NG, w, salt)["n_after"]
            parts.append(e.census())
    finally:
        for e in shards:
            e.close()
    assert total == target
    union = by_key(*[np.concatenate([p[i] for p in parts]) for i in range(3)])
    for a, b in zip(union, single):
        np.testing.assert_array_equal(bits(a), bits(b))


# ---------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_census_unchanged(eng, pool):
    d6, i5, keys, g, nm, _, _ = pool
    eng.import_census(d6[:500], i5[:500], keys[:500])
    pre = eng.census()
    lib, out, cnt = eng.lib, abi.CombOut(), C.c_int64()
    hist, vals = np.zeros(abi.COMB_BINS, np.uint64), np.zeros(500)

    def both(gt, ng, nt=nm, prefix=0, pb=0):
        gp = gt.ctypes.data if gt is not None else None
        npt = nt.ctypes.data if nt is not None else None
        return (lib.c2d_census_comb_hist(eng.ctx, gp, ng, npt, 1, prefix, pb, hist.ctypes.data, C.byref(out)),
                lib.c2d_census_comb_collect(eng.ctx, gp, ng, npt, 1, prefix, pb, vals.ctypes.data, 500, C.byref(cnt)))

    assert both(g, NG) == (0, 0)
    assert both(g, 0) == (-1, -1) and both(g, abi.ROULETTE_GROUPS_MAX + 1) == (-1, -1)
    gb = np.array(g)
    gb[128] = NG
    assert both(gb, NG) == (-1, -1)
    assert both(None, NG) == (-1, -1) and both(g, NG, None) == (-1, -1)
    for bad in (3.0, 0.75, 1.0 + 2.0 ** -52):
        nb = np.array(nm)
        nb[2, 1, 3] = bad
        assert both(g, NG, nb) == (-1, -1)
    for prefix, pb in ((0, 7), (0, 64), (0, -11), (1, 0), (1 << 11, 11), (1 << 63, 55)):
        assert both(g, NG, nm, prefix, pb) == (-1, -1)
    assert both(g, NG, nm, (1 << 55) - 1, 55) == (0, 0)
    assert lib.c2d_census_comb_hist(eng.ctx, g.ctypes.data, NG, nm.ctypes.data, 1, 0, 0, None, C.byref(out)) == -1
    assert lib.c2d_census_comb_hist(eng.ctx, g.ctypes.data, NG, nm.ctypes.data, 1, 0, 0, hist.ctypes.data, None) == -1
    assert lib.c2d_census_comb_collect(eng.ctx, g.ctypes.data, NG, nm.ctypes.data, 1, 0, 0, None, 5, C.byref(cnt)) == -1
    assert lib.c2d_census_comb_collect(eng.ctx, g.ctypes.data, NG, nm.ctypes.data, 1, 0, 0, vals.ctypes.data, -1,
                                       C.byref(cnt)) == -1
    assert lib.c2d_census_comb_collect(eng.ctx, g.ctypes.data, NG, nm.ctypes.data, 1, 0, 0, vals.ctypes.data, 5,
                                       None) == -1
    with pytest.raises(C2DError) as err:
        eng.census_comb_hist(g, NG, nm, 1, 0, 7)
    assert err.value.code == -1 and "prefix" in str(err.value)
    for a, b in zip(pre, eng.census()):
        np.testing.assert_array_equal(bits(a), bits(b))


def test_lost_census_is_a_state_error():
    """The census lost as in test_gpu_census_restart.py test_chunked_census_lost_after_failed_step."""
    gc = GoldenCase("ssc_tau")
    with Engine(gc.grid(comtot_mode=abi.COMTOT_EXACT, census_inplace=1)) as e:
        e.transport_step(gc.step_inputs(0))
        d6, i5, keys = e.census()
    g = CC.groups()
    with Engine(gc.grid(comtot_mode=abi.COMTOT_EXACT, census_inplace=1, queue_capacity=1)) as e:
        e.import_census(d6, i5, keys)
        with pytest.raises(C2DError) as err:
            e.transport_step(gc.step_inputs(1))
        assert err.value.code == -5 and e.census_count() == 0
        nm = np.ones((e.nz, e.nr, NG))
        for call in (lambda: e.census_comb_hist(g, NG, nm, 0), lambda: e.census_comb_collect(g, NG, nm, 0, 0, 0, 10)):
            with pytest.raises(C2DError) as err:
                call()
            assert err.value.code == abi.C2D_E_STATE
        with pytest.raises(C2DError) as err:                  # the arguments are judged first
            e.census_comb_hist(g, NG, nm, 0, 0, 7)
        assert err.value.code == -1
        e.import_census(d6, i5, keys)
        assert e.census_comb_hist(g, NG, nm, 0)[1]["n_records"] == len(keys)


# ---------------------------------------------- 6. CoupledRun with exact=True
def c3_small(sources=3000):
    deck = dict(synth.C3_DECK, nz=3, nr=3, T_const=1)
    return synth.c3_workload(sources=sources, comtot_mode=abi.COMTOT_TABLE, census_capacity=1 << 18,
                             event_capacity=1 << 18, deck=deck)


def coupled_rows(ctl, steps=6, by_hand=None):
    """Rows of `steps` steps and the final census keys.  by_hand: a
    CensusControl applied by the test itself after every step, call by call
    as apply_control did before it knew `exact`."""
    wl = c3_small()
    with Engine(dataclasses.replace(wl.grid, census_inplace=1)) as eng:
        run = CoupledRun(eng, wl, census_control=ctl)
        groups = PC.groups_by_decade(wl.grid.hu)
        rows = []
        for _ in range(steps):
            row = dict(run.step())
            if by_hand is not None:
                before = eng.census_count()
                row.update(census_before=before, census_after=before)
                if before > by_hand.target * (1.0 + by_hand.slack):
                    count, energy = eng.census_stats(*groups)
                    w = PC.weight_floor(count, energy, by_hand.target, by_hand.min_per_group)
                    row["census_after"] = eng.census_roulette(groups[0], groups[1], w, row["ncycle"])["n_after"]
            rows.append(row)
        return rows, np.sort(eng.census()[2])


def test_coupled_run_with_exact_census_control():
    free, keys_free = coupled_rows(None)
    n6 = len(keys_free)
    assert n6 > 2000
    target = n6 // 2
    rows, keys_x = coupled_rows(PC.CensusControl(target=target, exact=True))
    print([(r["census_before"], r["census_after"], r["comb_passes"], round(r["comb_ms"], 3)) for r in rows],
          "target", target)
    ran = [r for r in rows if r["roulette_ms"] > 0]
    assert ran and all(r["census_after"] == target and r["comb_passes"] >= 1 and r["comb_ms"] > 0 for r in ran)
    assert all(r["census_after"] == r["census_before"] and r["comb_passes"] == 0 for r in rows if r not in ran)
    assert all(r["aborted"] == 0 for r in rows) and rows[-1]["ncycle"] == free[-1]["ncycle"]
    assert len(keys_x) == rows[-1]["census_after"]
    assert rows.index(ran[0]) < len(rows) - 1 and rows[-1]["census"] > 0         # the run went on after a pass
    # exact=False: the rows and the census of the policy as it was
    ctl = PC.CensusControl(target=target)
    rows_w, keys_w = coupled_rows(ctl)
    rows_h, keys_h = coupled_rows(None, by_hand=ctl)
    assert "comb_ms" not in rows_w[0] and "comb_passes" not in rows_w[0]
    assert [(r["census_before"], r["census_after"], r["census"], r["escapes"]) for r in rows_w] == \
           [(r["census_before"], r["census_after"], r["census"], r["escapes"]) for r in rows_h]
    np.testing.assert_array_equal(keys_w, keys_h)
    assert any(r["census_after"] < r["census_before"] for r in rows_w)
