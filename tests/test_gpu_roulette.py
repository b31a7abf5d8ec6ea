"""Census population control on the GPU (c2d_census_stats, c2d_census_roulette;
csrc/roulette.hip) against the numpy yardstick (compton2d_amd/popcontrol.py):
the statistics, the pass in both census modes and both builds, its edge
outcomes, that the census still runs afterwards, sharding, the refusals, and
CoupledRun with a census_control.

The records are real ones: the census a 3x3 C2 workload leaves, so a
transport step can carry them on, with their ew replaced by a spread of six
decades around the floors (roulette_case.spread_ew).  Tolerances: counts,
keys and ew are exact; the energy sums come from f64 atomics in any order,
1e-12 relative (n <= 5137 terms of one sign: n * 2^-53 = 6e-13).
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import roulette_case as RC
from compton2d_amd import abi, popcontrol as PC, synth
from compton2d_amd.coupled import CoupledRun
from compton2d_amd.engine import C2DError, Engine
from golden_io import GoldenCase

pytestmark = pytest.mark.gpu

NZ = NR = 3
CAP = 8192
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 5 * 1024 + 17)
NG = 32
MODES = [(0, abi.COMTOT_EXACT), (1, abi.COMTOT_EXACT), (0, abi.COMTOT_TABLE), (1, abi.COMTOT_TABLE)]
TALLY_KEYS = ("edep", "prdep", "ecens", "npcen", "n_field", "E_IC", "nelectron", "fout", "edout",
              "erlki", "erlko", "erlku", "erlkl", "Ed_in")


def workload(mode=abi.COMTOT_EXACT, sources=9, capacity=CAP):
    return synth.c2_workload(nz=NZ, nr=NR, sources=sources, comtot_mode=mode, census_capacity=capacity,
                             event_capacity=1 << 16)


def grid_of(inplace, mode, capacity=CAP):
    return dataclasses.replace(workload(mode, capacity=capacity).grid, census_inplace=inplace,
                               queue_capacity=1 << 16)


@pytest.fixture(scope="module")
def pool():
    """(d6, i5, keys, g, w): at least 5137 census records of a 3x3 C2 run, their
    ew spread around the floors w [3, 3, 32]; left unchanged by every test."""
    wl = workload(sources=6000, capacity=1 << 16)
    with Engine(dataclasses.replace(wl.grid, queue_capacity=1 << 18)) as eng:
        for n in range(4):
            nc, t = wl.clock(n)
            eng.transport_step(dataclasses.replace(wl.step0, ncycle=nc, time=t))
            if eng.census_count() >= SIZES[-1]:
                break
        d6, i5, keys = eng.census()
    assert len(keys) >= SIZES[-1] and len(np.unique(keys)) == len(keys)
    d6, i5, keys = d6[:SIZES[-1]].copy(), i5[:SIZES[-1]].copy(), keys[:SIZES[-1]].copy()
    g = RC.group_table(NG)
    w = RC.floors(NZ, NR, NG)
    d6[:, 4] = RC.spread_ew(i5, NZ, NR, w, g)
    for a in (d6, i5, keys, g, w):
        a.setflags(write=False)
    return d6, i5, keys, g, w


@pytest.fixture(scope="module", params=MODES, ids=lambda p: "inplace%d-%s" % (p[0], "fast" if p[1] else "exact"))
def eng(request):
    inplace, mode = request.param
    with Engine(grid_of(inplace, mode)) as e:
        yield e


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), a.nbytes // max(len(a), 1))


def by_key(d6, i5, keys):
    o = np.argsort(keys, kind="stable")
    return d6[o], i5[o], keys[o]


def numpy_stats(d6, i5, g, ng):
    b = ((i5[:, 3].astype(np.int64) - 1) * NR + (i5[:, 4] - 1)) * ng + g[np.minimum(i5[:, 0], abi.NPHOMAX)]
    count = np.bincount(b, minlength=NZ * NR * ng).reshape(NZ, NR, ng)
    energy = np.bincount(b, weights=d6[:, 4], minlength=NZ * NR * ng).reshape(NZ, NR, ng)
    return count, energy


def check_pass(e, d6, i5, keys, g, ng, w, salt):
    """Import the records, run the pass, compare with the yardstick; returns the out dict."""
    n = len(keys)
    e.import_census(d6, i5, keys)
    pre = by_key(*e.census())
    out = e.census_roulette(g, ng, w, salt)
    keep, ew_new = PC.roulette_numpy(d6, i5, keys, NZ, NR, g, ng, w, salt)
    wr = PC.record_floors(i5, NZ, NR, g, ng, w)
    assert (out["n_before"], out["n_after"], out["n_tested"]) == (n, int(keep.sum()), int(PC.tested(d6[:, 4], wr).sum()))
    assert e.census_count() == out["n_after"]
    e_b, e_a = float(d6[:, 4].sum()), float(ew_new[keep].sum())
    print("n=%d: kept %d of %d tested %d; e_before rel %.2e, e_after rel %.2e" % (
        n, out["n_after"], n, out["n_tested"], abs(out["e_before"] - e_b) / max(e_b, 1e-300),
        abs(out["e_after"] - e_a) / max(e_a, 1e-300)))
    assert out["e_before"] == pytest.approx(e_b, rel=1e-12, abs=0.0)
    assert out["e_after"] == pytest.approx(e_a, rel=1e-12, abs=0.0)
    post = by_key(*e.census())
    want = np.sort(keys[keep])
    np.testing.assert_array_equal(post[2], want)                       # the yardstick's key set
    o = np.argsort(keys, kind="stable")
    np.testing.assert_array_equal(post[0][:, 4].view(np.uint64),       # its ew, bit for bit
                                  ew_new[o][keep[o]].view(np.uint64))
    sel = np.isin(pre[2], want)
    cols = [0, 1, 2, 3, 5]
    np.testing.assert_array_equal(bits(post[0][:, cols]), bits(pre[0][sel][:, cols]))   # every other column
    np.testing.assert_array_equal(post[1], pre[1][sel])
    return out


# ------------------------------------------------------------------ 1. stats
@pytest.mark.parametrize("ng", [1, NG])
def test_stats_equal_numpy(eng, pool, ng):
    d6, i5, keys, _, _ = pool
    g = RC.group_table(ng)
    for n in SIZES:
        eng.import_census(d6[:n], i5[:n], keys[:n])
        count, energy = eng.census_stats(g, ng)
        c_np, e_np = numpy_stats(d6[:n], i5[:n], g, ng)
        np.testing.assert_array_equal(count, c_np)
        np.testing.assert_allclose(energy, e_np, rtol=1e-12, atol=0.0)
        assert eng.census_count() == n


def test_stats_without_lds(pool):
    """A histogram past the LDS plan (30 x 30 cells x 32 groups = 460 KB) takes the global atomics."""
    d6, i5, keys, g, _ = pool
    wl = synth.c2_workload(nz=30, nr=30, sources=9, comtot_mode=abi.COMTOT_EXACT, census_capacity=CAP,
                           event_capacity=1 << 10)
    i5 = i5.copy()
    rng = np.random.default_rng(5)
    i5[:, 3], i5[:, 4] = rng.integers(1, 31, len(keys)), rng.integers(1, 31, len(keys))
    with Engine(dataclasses.replace(wl.grid, queue_capacity=1 << 10)) as e:
        e.import_census(d6, i5, keys)
        count, energy = e.census_stats(g, NG)
    b = ((i5[:, 3].astype(np.int64) - 1) * 30 + (i5[:, 4] - 1)) * NG + g[np.minimum(i5[:, 0], abi.NPHOMAX)]
    np.testing.assert_array_equal(count.reshape(-1), np.bincount(b, minlength=30 * 30 * NG))
    np.testing.assert_allclose(energy.reshape(-1), np.bincount(b, weights=d6[:, 4], minlength=30 * 30 * NG),
                               rtol=1e-12, atol=0.0)


# --------------------------------------------------- 2. against the yardstick
def test_roulette_equals_yardstick(eng, pool, monkeypatch):
    d6, i5, keys, g, w = pool
    for n in SIZES:
        out = check_pass(eng, d6[:n], i5[:n], keys[:n], g, NG, w, salt=n + 1)
        if n >= 63:
            assert 0 < out["n_tested"] and out["n_after"] < n
    # the same census in slices of 1000 records: several rounds of pack, unpack, advance
    monkeypatch.setenv("C2D_ROULETTE_SLICE", "1000")
    for n in (1, 1000, 1001, SIZES[-1]):
        check_pass(eng, d6[:n], i5[:n], keys[:n], g, NG, w, salt=7)
    monkeypatch.setenv("C2D_ROULETTE_SLICE", "1")
    check_pass(eng, d6[:65], i5[:65], keys[:65], g, NG, w, salt=7)


@pytest.mark.parametrize("inplace", [0, 1])
def test_roulette_more_tiles_than_scratch_regions(pool, inplace):
    """70 001 records are 69 tiles of 1024 over the scratch's 64 regions: five regions take two
    tiles, and the unpack joins regions of different fill."""
    d6, i5, keys, g, w = pool
    reps = 14
    big = (np.tile(d6, (reps, 1))[:70001], np.tile(i5, (reps, 1))[:70001],
           np.concatenate([keys ^ np.uint64(0x9E3779B97F4A7C15 * k & 0xFFFFFFFFFFFFFFFF) for k in range(reps)])[:70001])
    assert len(np.unique(big[2])) == 70001
    with Engine(grid_of(inplace, abi.COMTOT_EXACT, capacity=1 << 17)) as e:
        out = check_pass(e, *big, g, NG, w, salt=3)
        assert 30000 < out["n_after"] < 50000
        if inplace:
            assert e.last_census_chunks()[0] == -(-out["n_after"] // 1024)


# ------------------------------------------------------------ 3. edge outcomes
def device_records(donor, d6, i5, keys):
    """The records packed in device memory (a torch buffer), through `donor`."""
    import torch
    donor.import_census(d6, i5, keys)
    raw = torch.empty(len(keys) * abi.CENSUS_REC_WORDS, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    donor.census_pack(0, len(keys), raw.data_ptr())
    return raw


def test_edge_outcomes(eng, pool):
    d6, i5, keys, g, w = pool
    n = SIZES[-1]
    chunked = eng.grid.census_inplace == 1
    # floors that test nothing: byte-identical, order included
    for w0 in (np.zeros((NZ, NR, NG)), np.full((NZ, NR, NG), np.nan), np.full((NZ, NR, NG), -np.inf)):
        eng.import_census(d6, i5, keys)
        pre = eng.census()
        out = eng.census_roulette(g, NG, w0, 3)
        assert (out["n_before"], out["n_after"], out["n_tested"]) == (n, n, 0)
        assert out["e_before"] == pytest.approx(d6[:, 4].sum(), rel=1e-12) and out["e_after"] == out["e_before"]
        for a, b in zip(pre, eng.census()):
            np.testing.assert_array_equal(bits(a), bits(b))
    # floors of 1e300 everywhere but the fullest (cell, group): what stays is that bin, whatever the salt
    c_np = numpy_stats(d6, i5, g, NG)[0]
    full = np.unravel_index(np.argmax(c_np), c_np.shape)
    huge = np.full((NZ, NR, NG), 1e300)
    huge[full] = 0.0
    for salt in (0, 1, 2 ** 63):
        out = check_pass(eng, d6, i5, keys, g, NG, huge, salt)
        assert out["n_after"] == c_np[full] > 0 and out["n_tested"] == n - c_np[full]
        if chunked:
            assert eng.last_census_chunks()[0] == -(-out["n_after"] // 1024)
    # the yardstick keeps nothing: an empty census, and the context goes on
    huge[:] = 1e300
    assert not PC.roulette_numpy(d6, i5, keys, NZ, NR, g, NG, huge, 9)[0].any()
    out = check_pass(eng, d6, i5, keys, g, NG, huge, 9)
    assert out["n_after"] == 0 and eng.census_count() == 0 and out["e_after"] == 0.0
    if chunked:
        assert eng.last_census_chunks()[0] == 0
    assert eng.census_roulette(g, NG, huge, 9)["n_before"] == 0          # a pass over nothing
    eng.import_census(d6[:100], i5[:100], keys[:100])
    assert eng.census_count() == 100
    # the freed chunks are free again: the census shrinks, then takes 2000 records
    out = check_pass(eng, d6, i5, keys, g, NG, w, 11)
    if chunked:
        assert eng.last_census_chunks()[0] == -(-out["n_after"] // 1024) < 6
    kept = by_key(*eng.census())
    with Engine(grid_of(0, eng.grid.comtot_mode)) as donor:
        extra = (d6[:2000], i5[:2000], keys[:2000] ^ np.uint64(1 << 63))
        raw = device_records(donor, *extra)
        eng.census_append(raw.data_ptr(), 2000)
        want = by_key(*donor.census())
    assert eng.census_count() == out["n_after"] + 2000
    got = eng.census()
    np.testing.assert_array_equal(bits(got[0][:out["n_after"]][np.argsort(got[2][:out["n_after"]])]), bits(kept[0]))
    tail = by_key(got[0][out["n_after"]:], got[1][out["n_after"]:], got[2][out["n_after"]:])
    for a, b in zip(tail, want):
        np.testing.assert_array_equal(bits(a), bits(b))


# --------------------------------------------------- 4. the census still runs
@pytest.mark.parametrize("inplace", [0, 1])
def test_census_runs_after_roulette(pool, inplace):
    d6, i5, keys, g, w = pool
    wl = workload()
    # one volume source per zone, carrying the zone's whole emission (ewsv = Eloss_tot / nsv)
    # (ncycle 1: a step of ncycle 0 writes no escape events)
    nc, t = wl.clock(1)
    step = dataclasses.replace(wl.step0, ncycle=nc, time=t, nsv=np.ones((NZ, NR), np.int32),
                               ewsv=np.array(wl.step0.Eloss_tot))
    keep, ew_new = PC.roulette_numpy(d6, i5, keys, NZ, NR, g, NG, w, 21)
    res = []
    for rouletted in (True, False):
        with Engine(grid_of(inplace, abi.COMTOT_EXACT, capacity=1 << 16)) as e:
            if rouletted:
                e.import_census(d6, i5, keys)
                assert e.census_roulette(g, NG, w, 21)["n_after"] == keep.sum()
            else:                                   # the yardstick's survivors into a fresh context
                s = d6[keep].copy()
                s[:, 4] = ew_new[keep]
                e.import_census(s, i5[keep], keys[keep])
            e.transport_step(step)
            ev = e.events()
            res.append((np.sort(e.census()[2]), ev[np.lexsort(ev.T[::-1])], e.tallies()))
    (k_a, ev_a, t_a), (k_b, ev_b, t_b) = res
    assert len(k_a) > 0 and len(ev_a) > 0 and ev_a.shape == ev_b.shape
    np.testing.assert_array_equal(k_a, k_b)
    np.testing.assert_array_equal(ev_a.view(np.uint64), ev_b.view(np.uint64))
    for k in TALLY_KEYS:
        a, b = np.asarray(t_a[k]), np.asarray(t_b[k])
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * max(float(np.abs(b).max()), 0.0), err_msg=k)


# ---------------------------------------------------------------- 5. sharding
def test_sharded_union_equals_single_context(pool):
    d6, i5, keys, _, _ = pool
    g, ng = RC.group_table(4), 4
    n = len(keys)
    with Engine(grid_of(1, abi.COMTOT_EXACT)) as one:
        one.import_census(d6, i5, keys)
        count, energy = one.census_stats(g, ng)
        w = PC.weight_floor(count, energy, n // 3)
        assert (w > 0).any()
        out = one.census_roulette(g, ng, w, 5)
        single = by_key(*one.census())
    assert out["n_after"] < n
    parts, c_sum, e_sum = [], np.zeros_like(count), np.zeros_like(energy)
    shards = [Engine(grid_of(r, abi.COMTOT_EXACT)) for r in (0, 1)]
    try:
        for r, e in enumerate(shards):
            e.import_census(d6[r::2], i5[r::2], keys[r::2])
            c, en = e.census_stats(g, ng)
            c_sum += c
            e_sum += en
        np.testing.assert_array_equal(c_sum, count)
        w2 = PC.weight_floor(c_sum, e_sum, n // 3)          # once, from the summed statistics
        np.testing.assert_array_equal(w2, w)                  # the power-of-two floors absorb the sums' last bits
        for e in shards:
            e.census_roulette(g, ng, w2, 5)
            parts.append(e.census())
    finally:
        for e in shards:
            e.close()
    union = by_key(*[np.concatenate([p[i] for p in parts]) for i in range(3)])
    for a, b in zip(union, single):
        np.testing.assert_array_equal(bits(a), bits(b))
    keep, _ = PC.roulette_numpy(d6, i5, keys, NZ, NR, g, ng, w, 5)
    np.testing.assert_array_equal(single[2], np.sort(keys[keep]))


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_census_unchanged(eng, pool):
    d6, i5, keys, g, w = pool
    eng.import_census(d6[:500], i5[:500], keys[:500])
    pre = eng.census()
    lib, out = eng.lib, abi.RouletteOut()
    cnt, en = np.zeros((NZ, NR, NG), np.int64), np.zeros((NZ, NR, NG))

    def both(gt, ng, wt=w):
        gp = gt.ctypes.data if gt is not None else None
        wp = wt.ctypes.data if wt is not None else None
        return (lib.c2d_census_roulette(eng.ctx, gp, ng, wp, 1, C.byref(out)),
                lib.c2d_census_stats(eng.ctx, gp, ng, cnt.ctypes.data, en.ctypes.data))

    assert both(g, 0) == (-1, -1) and both(g, abi.ROULETTE_GROUPS_MAX + 1) == (-1, -1)
    for bad in (-1, NG):
        gb = np.array(g)
        gb[128] = bad
        assert both(gb, NG) == (-1, -1)
    assert both(None, NG) == (-1, -1)
    assert both(g, NG, None)[0] == -1
    assert lib.c2d_census_roulette(eng.ctx, g.ctypes.data, NG, w.ctypes.data, 1, None) == -1
    assert lib.c2d_census_stats(eng.ctx, g.ctypes.data, NG, None, en.ctypes.data) == -1
    assert lib.c2d_census_stats(eng.ctx, g.ctypes.data, NG, cnt.ctypes.data, None) == -1
    with pytest.raises(C2DError) as err:
        eng.census_roulette(g, 0, w, 1)
    assert err.value.code == -1 and "ngroup" in str(err.value)
    for a, b in zip(pre, eng.census()):
        np.testing.assert_array_equal(bits(a), bits(b))


def test_lost_census_is_a_state_error(pool):
    """The census lost as in test_gpu_census_restart.py test_chunked_census_lost_after_failed_step."""
    gc = GoldenCase("ssc_tau")
    with Engine(gc.grid(comtot_mode=abi.COMTOT_EXACT, census_inplace=1)) as e:
        e.transport_step(gc.step_inputs(0))
        d6, i5, keys = e.census()
    g = RC.group_table(NG)
    with Engine(gc.grid(comtot_mode=abi.COMTOT_EXACT, census_inplace=1, queue_capacity=1)) as e:
        e.import_census(d6, i5, keys)
        with pytest.raises(C2DError) as err:
            e.transport_step(gc.step_inputs(1))
        assert err.value.code == -5 and e.census_count() == 0
        w = np.ones((e.nz, e.nr, NG))
        for call in (lambda: e.census_stats(g, NG), lambda: e.census_roulette(g, NG, w, 0)):
            with pytest.raises(C2DError) as err:
                call()
            assert err.value.code == abi.C2D_E_STATE
        with pytest.raises(C2DError) as err:                  # the arguments are judged first
            e.census_roulette(g, 0, w, 0)
        assert err.value.code == -1
        e.import_census(d6, i5, keys)
        assert e.census_roulette(g, NG, w * 0.0, 0)["n_after"] == len(keys)


# ------------------------------------------------ 7. CoupledRun with control
def c3_small(sources=3000):
    deck = dict(synth.C3_DECK, nz=NZ, nr=NR, T_const=1)
    return synth.c3_workload(sources=sources, comtot_mode=abi.COMTOT_TABLE, census_capacity=1 << 18,
                             event_capacity=1 << 18, deck=deck)


def coupled_rows(ctl, steps=6, cut=None, tmp_path=None):
    """Rows of `steps` steps and the final census keys; cut: save after that many steps and
    carry on in a fresh context."""
    wl = c3_small()
    eng = Engine(dataclasses.replace(wl.grid, census_inplace=1))
    try:
        run = CoupledRun(eng, wl, census_control=ctl)
        rows = []
        for n in range(steps):
            if cut is not None and n == cut:
                p = tmp_path / "cut.ckpt"
                run.save(p)
                eng.close()
                wl = c3_small()
                eng = Engine(dataclasses.replace(wl.grid, census_inplace=1))
                run = CoupledRun.restore(eng, wl, p, census_control=ctl)
            rows.append(dict(run.step()))
        g, ng = PC.groups_by_decade(wl.grid.hu)
        count, _ = eng.census_stats(g, ng)
        return rows, np.sort(eng.census()[2]), count
    finally:
        eng.close()


def test_coupled_run_with_census_control(tmp_path):
    free, keys_free, _ = coupled_rows(None)
    assert "census_before" not in free[0]                      # None changes nothing
    n6 = len(keys_free)
    assert n6 > 2000
    ctl = PC.CensusControl(target=n6 // 2)
    rows, keys_a, count = coupled_rows(ctl)
    limit = ctl.target * (1.0 + ctl.slack)
    sparse = int(count[count < ctl.min_per_group].sum())
    print([(r["census_before"], r["census_after"], round(r["roulette_ms"], 3)) for r in rows], "target", ctl.target,
          "sparse", sparse)
    assert all(r["census_after"] <= r["census_before"] for r in rows)
    assert any(r["census_after"] < r["census_before"] and r["roulette_ms"] > 0 for r in rows)
    assert all(r["census_after"] <= limit + sparse for r in rows[-3:])
    assert len(keys_a) == rows[-1]["census_after"] < n6
    rows_b, keys_b, _ = coupled_rows(ctl)
    np.testing.assert_array_equal(keys_a, keys_b)
    assert [(r["census_before"], r["census_after"]) for r in rows] == \
           [(r["census_before"], r["census_after"]) for r in rows_b]
    _, keys_c, _ = coupled_rows(ctl, cut=3, tmp_path=tmp_path)
    np.testing.assert_array_equal(keys_a, keys_c)
