"""Compton reflection through the engine (c2d_config.cr_sent 1..4): init,
the specular deck's invariants, the statistical comparison with the
reference's own runs (tests/golden/reflect_*.npz, made by
tests/golden/make_reflect_golden.py), lineage sharding, and the table and
result calls.

The compared spectral bins are groups of adjacent hu bins, each populated in
every reference run (reflect_case.select_groups: single hu bins populated in
every run carry only 35-52 % of the escaping energy at nst = 2000, which sits
in the rarely populated top bins; the groups carry all of it above 1e-3 keV,
the last group being everything above ~3e5 keV).  The fixtures' generator and
this test both hold the share of the reference's summed fout energy in the
compared bins to 90 % at least.

The seed counts per deck (reflect_case.REF_SEEDS, GPU_RUNS below) were fixed
before the groups were introduced and the fixtures' meta recomputed; how the
specular deck came to 256 reference runs is in profiles/r16a/README.md.
"""
import numpy as np
import pytest

import reflect_case as RF
from compton2d_amd import abi, engine
from compton2d_amd.engine import C2DError, Engine
from golden_io import GoldenCase

pytestmark = pytest.mark.gpu

GPU_RUNS = {"spec": 128, "both": 64, "disk": 64}      # lineage seeds per deck (>= 64)
MODES = {"exact": abi.COMTOT_EXACT, "fast": abi.COMTOT_TABLE}


@pytest.fixture(scope="module")
def fixtures():
    return {k: RF.ReflectFixture(k) for k in ("spec", "both", "disk")}


def test_init_accepts_cr_sent_1_to_4():
    gc = GoldenCase("ssc_tau")
    for cr in (1, 2, 3, 4):
        Engine(gc.grid(cr_sent=cr)).close()
    for cr in (5, -1):
        with pytest.raises(C2DError) as e:
            Engine(gc.grid(cr_sent=cr))
        assert e.value.code == abi.C2D_E_ARG


@pytest.mark.parametrize("spec_switch", [0, 1])
@pytest.mark.parametrize("mode", list(MODES))
def test_specular_deck(fixtures, mode, spec_switch):
    fx = fixtures["spec"]
    eng = Engine(fx.grid(comtot_mode=MODES[mode], spec_switch=spec_switch))
    rows = RF.engine_run(fx, eng)
    eng.close()
    zmin = fx.meta["zmin"]
    n_spec = 0
    for n, row in enumerate(rows):
        ev, cnt = row["events"], row["counters"]
        assert not ((ev[:, 4] == zmin) & (ev[:, 5] < 0)).any()       # nothing leaves downwards
        assert (row["erlkl"] == 0).all() and (row["Ed_in"] == 0).all()
        assert cnt[abi.CNT_ABORTED] == 0
        assert cnt[abi.CNT_EVENTS] == len(ev)
        assert row["counts"][1] == 0 and row["counts"][2] == 0 and (row["Ed_ref"] == 0).all()
        n_spec += row["counts"][0]
        if n > 0:
            assert len(ev) > 0
            assert np.sum(row["fout"]) > 0        # 1: the spectrum incident on the boundary, 0: the escaping one
    assert n_spec > 0


@pytest.mark.parametrize("mode", list(MODES))
def test_specular_fout_uses_the_bins_from_before(fixtures, mode):
    """spec_switch = 1 with two angular bins (wmu <= 0, wmu > 0): a packet
    reaches the lower boundary heading down, so the fout line of the specular
    branch, which takes the bins from before the reflection
    (imcleak2d.f:116-117), fills the first angular row only, and nothing else
    adds to fout (escapes skip it when spec_switch = 1).  The reflected packet
    is rebinned: events that leave upwards afterwards carry no fout either."""
    fx = fixtures["spec"]
    eng = Engine(fx.grid(comtot_mode=MODES[mode], spec_switch=1, mu=np.array([0.0, 1.0])))
    down = up = 0.0
    for n in range(fx.nsteps):
        eng.transport_step(fx.step_inputs(n))
        f = np.asarray(eng.tallies()["fout"])
        assert f.shape[0] == 2
        down += f[0].sum()
        up += f[1].sum()
        assert eng.reflect_result()[1][0] > 0
    eng.close()
    assert down > 0 and up == 0.0


def test_reflect_result_world_sum_and_coupled_run():
    """c2d_reflect_result's RCCL sum on a world of 1 (the identity, as
    tests/test_gpu_rccl_cabi.py does for the tallies), and a reflecting deck
    through CoupledRun: the C3 workload with cr_sent = 3 (tbbl = 0: specular
    below, the disk outside), transport and FP coupled, three steps."""
    from compton2d_amd import synth
    from compton2d_amd.coupled import CoupledRun
    wl = synth.c3_workload(sources=50_000, comtot_mode=abi.COMTOT_TABLE)
    wl.grid.cr_sent = 3
    eng = Engine(wl.grid)
    eng.comm_init(eng.comm_unique_id(), 0, 1)
    run = CoupledRun(eng, wl)
    tot = np.zeros(3)
    for _ in range(3):
        row = run.step()
        assert row["aborted"] == 0
        ed, cnt = eng.reflect_result()
        ed2, cnt2 = eng.reflect_result(world_sum=True)
        np.testing.assert_array_equal(ed, ed2)
        np.testing.assert_array_equal(cnt, cnt2)
        tot += cnt
    eng.close()
    assert tot[0] > 0 and tot[1] == 0 and tot[2] > 0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("deck", ["spec", "both", "disk"])
def test_reflecting_deck_vs_reference(fixtures, deck, mode, capsys):
    fx = fixtures[deck]
    assert len(fx.a["seeds"]) >= 32
    n_runs = GPU_RUNS[deck]
    runs, counts, disk_events = [], np.zeros(3), 0
    for k in range(n_runs):
        eng = Engine(fx.grid(comtot_mode=MODES[mode], seed=RF.lin_seed(k)))
        rows = RF.engine_run(fx, eng)
        eng.close()
        for n, row in enumerate(rows):
            assert row["counters"][abi.CNT_ABORTED] == 0
            assert np.isfinite(row["events"]).all()
            counts += row["counts"]
            if fx.meta["step%d" % n]["ncycle"] > 0:      # events are written for ncycle > 0 only
                disk_events += row["counts"][2]
        runs.append(rows)
    A = RF.stack_runs(runs)
    B = {k: v for k, v in fx.a.items() if k.startswith("run_")}
    assert fx.meta["fout_share"] >= 0.9                 # the compared bins' share of the reference's fout energy
    assert fx.meta["split_half"]["ok"]                  # the reference against itself meets the thresholds
    res = RF.compare(A, slice(None), B, slice(None), fx.groups)
    with capsys.disabled():
        print("\nreflect_%s, %s build, %d runs vs %d reference runs (counts specular/matrix/disk %s, "
              "fout share of the compared bins %.3f): %s" % (deck, mode, n_runs, len(fx.a["seeds"]),
                                                            counts.tolist(), fx.meta["fout_share"], res))
    cr = fx.meta["cr_sent"]
    assert (counts[0] > 0) == (cr == 4)                # tbbl > 0 on both rings of the cr_sent = 3 deck
    assert (counts[1] > 0) == (cr == 3)
    assert (counts[2] > 0) == (cr in (2, 3))
    if cr in (2, 3):
        # a tenth of the events at least are disk reflections, as in the reference
        assert A["run_refl_xnu"].sum() >= 0.1 * A["run_n_events"].sum()
        assert A["run_refl_xnu"].sum() == disk_events  # every one of them is an event (all >= 1 keV: in hu)
    sp = res["spectrum"]
    assert sp["bins"] == len(fx.groups)
    for name in ("spectrum", "refl_xnu", "refl_wmu"):
        d = res[name]
        assert d["p_value"] > RF.P_MIN, (name, d)
        assert d["rms_z"] <= RF.RMS_Z_MAX, (name, d)
        assert d["max_abs_z"] <= RF.MAX_Z, (name, d)
    for i, z in enumerate(sp["band_z"]):
        assert abs(z) <= RF.BAND_Z, (i, sp)
    assert abs(res["events_z"]) <= RF.COUNT_Z, res
    assert abs(res["census_z"]) <= RF.COUNT_Z, res


def _close(a, b, what):
    scale = max(np.max(np.abs(b)), 1e-300)
    np.testing.assert_allclose(a, b, rtol=1e-11, atol=1e-13 * scale, err_msg=what)


def test_sharded_reflecting_deck_sums_to_world_one(fixtures):
    """Ranks 0 and 1 of a world of 2 (lineage sharding) against the one-rank
    run, to tests/test_gpu_sharding.py's tolerances."""
    fx = fixtures["both"]
    one = Engine(fx.grid(comtot_mode=abi.COMTOT_EXACT))
    want = RF.engine_run(fx, one)
    one.close()
    engs = [Engine(fx.grid(comtot_mode=abi.COMTOT_EXACT, rank=r, world=2)) for r in range(2)]
    keys = ("fout", "edout", "erlki", "erlko", "erlku", "erlkl", "Ed_in", "edep", "ecens", "Ed_ref")
    for n in range(fx.nsteps):
        si = fx.step_inputs(n)
        parts = []
        for e in engs:
            e.transport_step(si)
            t = e.tallies()
            ed, cnt = e.reflect_result()
            parts.append(dict(t, Ed_ref=ed, counts=cnt, events=e.events(), edep=np.sum(t["edep"]),
                              ecens=np.sum(t["ecens"]), ncens=e.census_count()))
        w = want[n]
        for k in keys:
            _close(sum(np.asarray(p[k], float) for p in parts), np.asarray(w[k], float), "%s step %d" % (k, n))
        np.testing.assert_array_equal(sum(p["counts"] for p in parts), w["counts"])
        for c in (abi.CNT_STEPS, abi.CNT_ESCAPES, abi.CNT_CENSUS, abi.CNT_COLLIDE, abi.CNT_EVENTS):
            assert sum(p["counters"][c] for p in parts) == w["counters"][c], c
        assert sum(p["ncens"] for p in parts) == w["n_census"]
        ev = np.concatenate([p["events"] for p in parts])
        order = lambda x: x[np.lexsort(x.T[::-1])]
        np.testing.assert_array_equal(order(ev), order(w["events"]))   # the event multiset, bit for bit
    assert sum(w["counts"][1] for w in want) > 0 and sum(w["counts"][2] for w in want) > 0
    for e in engs:
        e.close()


def test_reflect_tables_and_result_calls(fixtures):
    host = abi.reflect_tables_host()
    fx = fixtures["both"]
    eng = Engine(fx.grid())
    for a, b in zip(eng.reflect_tables(), host):
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    with pytest.raises(C2DError) as e:
        eng.reflect_result()                         # before the first step
    assert e.value.code == abi.C2D_E_STATE
    eng.close()
    for cr in (0, 4):
        eng = Engine(fx.grid(cr_sent=cr))
        with pytest.raises(C2DError) as e:
            eng.reflect_tables()
        assert e.value.code == abi.C2D_E_STATE
        if cr == 0:
            eng.transport_step(fx.step_inputs(0))
            eng.transport_step(fx.step_inputs(1))
            ed, cnt = eng.reflect_result()
            assert (ed == 0).all() and (cnt == 0).all()
        eng.close()
