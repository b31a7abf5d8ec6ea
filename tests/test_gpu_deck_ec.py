"""A coupled external-Compton run driven from its deck on the GPU: the deck of
tests/ec_deck.py (2x2 grid of the golden case ec_lower, Gamma = 25, nst = 3000,
FP on, `disk/blackbody_G25_4spectra.in` on both lower rings in window 1 of two;
steps 0-2 fall in window 1, steps 3 and 4 in window 2).  The exact build
(COMTOT_EXACT, FP_EXACT) against the oracle step by step, the FP update from
the device tallies, the packet counts per window, the device-resident loop
against the host loop, lineage sharding, a checkpoint that crosses the window
edge, and the fast build (COMTOT_TABLE, FP_AUTO)."""
import dataclasses

import numpy as np
import pytest

import ec_deck as D
import oracle_lib as OL
from compton2d_amd import abi, deck
from compton2d_amd.coupled import CoupledRun
from compton2d_amd.engine import Engine
from test_gpu_parity import COUNTERS, TALLY_KEYS, sort_rows

pytestmark = pytest.mark.gpu

NSTEPS = 4


@pytest.fixture(scope="module")
def decks(tmp_path_factory):
    """The EC deck and its twin without boundary sources, as read_deck returns them."""
    d = tmp_path_factory.mktemp("ec_deck")
    D.write_deck(d / "ec", D.ec_windows())
    D.write_deck(d / "dark", D.ec_windows(tbbl=0.0))
    return deck.read_deck(d / "ec"), deck.read_deck(d / "dark")


def workload(dk, mode=abi.COMTOT_EXACT, **kw):
    return deck.deck_workload(dk, dk["nst"] // 2, comtot_mode=mode, **kw)


def close(got, ref, what):
    ref = np.asarray(ref)
    scale = max(np.max(np.abs(ref)), 1e-300)
    np.testing.assert_allclose(got, ref, rtol=1e-11, atol=1e-13 * scale, err_msg=what)


def same_census(a, b):
    (d6a, i5a, ka), (d6b, i5b, kb) = a, b
    oa, ob = np.argsort(ka), np.argsort(kb)
    np.testing.assert_array_equal(ka[oa], kb[ob])
    np.testing.assert_array_equal(d6a[oa].view(np.uint64), d6b[ob].view(np.uint64))
    np.testing.assert_array_equal(i5a[oa], i5b[ob])


@pytest.fixture(scope="module")
def replay(decks):
    """The exact build's four steps, each replayed on the oracle from the
    step's own host inputs (next_step_inputs): per step the inputs, the row
    and what both sides hold afterwards."""
    wl = workload(decks[0])
    assert wl.boundary is not None
    eng = Engine(wl.grid)
    run = CoupledRun(eng, wl, fp_mode=abi.FP_EXACT)
    orc = OL.Oracle(dataclasses.replace(wl.grid), OL.RNG_LINEAGE, "det")
    out = []
    for n in range(NSTEPS):
        si = run.next_step_inputs()
        row = run.step()
        assert orc.step(si) == 0
        out.append(dict(si=si, row=dict(row), gpu=eng.tallies(), orc=orc.split(), gpu_census=eng.census(),
                        orc_census=orc.census(), gpu_events=eng.events(), orc_events=orc.events()))
    fp = fp_from_device_tallies(eng, run, wl)
    eng.close()
    orc.close()
    return out, fp


def fp_from_device_tallies(eng, run, wl):
    """One more FP update on the run's state after its last step, reading
    n_field / ecens from the device tally buffer, and the oracle's update on
    the same call with the tallies as host arrays (fp_call_host)."""
    ncycle, tm, dt, inputs, state = run.fp_call_host()
    g = eng.fp_step(ncycle, tm, dt, dict(inputs, n_field=None, ecens=None), state)
    o = OL.fp_step(dataclasses.replace(wl.grid), wl.fp_const, ncycle, tm, dt, inputs, state, flavor="det")
    return g, o, inputs


def test_every_step_equals_the_oracle(replay):
    steps, _ = replay
    events = 0
    for n, s in enumerate(steps):
        np.testing.assert_array_equal(s["gpu"]["counters"][list(COUNTERS)], s["orc"]["counters"][list(COUNTERS)],
                                      err_msg="step %d counters" % n)
        for k in TALLY_KEYS:
            close(s["gpu"][k], s["orc"][k], "step %d %s" % (n, k))
        assert len(s["gpu_census"][2]) == len(s["orc_census"][2]) > 0
        same_census(s["gpu_census"], s["orc_census"])
        eg, eo = s["gpu_events"], s["orc_events"]
        assert eg.shape == eo.shape
        np.testing.assert_array_equal(sort_rows(eg).view(np.uint64), sort_rows(eo).view(np.uint64))
        events += len(eg)
        assert s["row"]["aborted"] == 0
    assert events > 0
    assert [s["row"]["fp_mode"] for s in steps] == [None] + ["exact"] * (NSTEPS - 1)


def test_fp_from_device_tallies_equals_the_oracle(replay):
    _, (g, o, inputs) = replay
    assert np.asarray(inputs["n_field"]).sum() > 0
    for j in range(2):
        for k in range(2):
            np.testing.assert_allclose(g["f_nt"][j, k], o["f_nt"][j, k], rtol=1e-8,
                                       atol=1e-12 * np.max(o["f_nt"][j, k]))
            assert abs(g["Te_new"][j, k] - o["Te_new"][j, k]) <= 1e-8 * o["Te_new"][j, k]


def test_packet_counts_follow_the_windows(replay, decks):
    steps, _ = replay
    rows = [s["row"] for s in steps]
    assert [r["window"] for r in rows] == [0, 0, 0, 1]
    assert all(r["ec_on"] for r in rows) and all(r["fbias"] == 1.0 for r in rows)
    for s in steps[:3]:
        assert s["row"]["surface_packets"] == int(s["si"].nsurfl.sum()) > 0
        assert s["row"]["sources"] >= s["row"]["surface_packets"]
        assert s["gpu"]["counters"][abi.CNT_SOURCES] == s["row"]["sources"]
    assert rows[3]["surface_packets"] == 0 and not np.any(steps[3]["si"].nsurfl)
    # the boundary photons reach the zones' radiation field
    wl = workload(decks[1])
    assert wl.boundary is None
    with Engine(wl.grid) as eng:
        run = CoupledRun(eng, wl, fp_mode=abi.FP_EXACT)
        for _ in range(2):
            dark = run.step()
        dark_field = float(np.sum(eng.tallies()["n_field"]))
    assert dark["surface_packets"] == 0 and dark["window"] is None
    assert float(np.sum(steps[1]["gpu"]["n_field"])) > dark_field


def test_device_resident_loop_equals_host_loop(decks):
    runs = []
    for dev in (True, False):
        wl = workload(decks[0])
        with Engine(wl.grid) as eng:
            run = CoupledRun(eng, wl, device_resident=dev, fp_mode=abi.FP_EXACT)
            rows = [dict(run.step()) for _ in range(NSTEPS)]
            f, p = run.electrons()
            runs.append((rows, f, p, dict(run.state)))
    (ra, fa, pa, sa), (rb, fb, pb, sb) = runs
    for a, b in zip(ra, rb):
        assert a["volume_packets"] == b["volume_packets"]
        assert a["surface_packets"] == b["surface_packets"] and a["window"] == b["window"]
        assert abs(a["packet_steps"] - b["packet_steps"]) <= 1e-3 * b["packet_steps"]
    np.testing.assert_allclose(fa, fb, rtol=1e-6, atol=1e-12 * np.max(np.abs(fb)))
    np.testing.assert_allclose(pa, pb, rtol=1e-6, atol=1e-12)
    np.testing.assert_array_equal(sa["tea"], sb["tea"])
    assert rb[-1]["aborted"] == 0 and ra[-1]["aborted"] == 0


def test_sharded_contexts_sum_to_world_one(replay, decks):
    """One window-1 step on contexts (0,2) and (1,2): boundary sources shard
    by lineage inside the engine, the budgets are global."""
    ref = replay[0][0]
    parts, keys = [], []
    for rank in range(2):
        wl = workload(decks[0], rank=rank, world=2)
        with Engine(wl.grid) as eng:
            row = CoupledRun(eng, wl, fp_mode=abi.FP_EXACT).step()
            assert row["surface_packets"] == ref["row"]["surface_packets"]
            parts.append(eng.tallies())
            keys += eng.census()[2].tolist()
    cnt = sum(p["counters"] for p in parts)
    np.testing.assert_array_equal(cnt[list(COUNTERS)], ref["gpu"]["counters"][list(COUNTERS)])
    for k in TALLY_KEYS:
        close(sum(np.asarray(p[k]) for p in parts), ref["gpu"][k], k)
    k_ref = set(ref["gpu_census"][2].tolist())
    assert len(keys) == len(set(keys)) == len(k_ref) and set(keys) == k_ref
    assert all(p["counters"][abi.CNT_SOURCES] > 0 for p in parts)


def test_a_checkpoint_crosses_the_window_edge(tmp_path, decks):
    """Saved after step 2, the last of window 1: the restored run finds window 2
    from its step number alone, and its steps 3 and 4 equal the uninterrupted
    run's (counters equal, tallies to atomic order, census and events bit for
    bit).

    Step 3 is compared between the two coupled runs: everything it reads was
    saved.  Step 4 follows an FP update that read n_field from the tally
    buffer, which atomics sum in another order on every context, so the two
    runs' electrons agree to rounding, not bit for bit; on an MI355X their
    step-4 census then differed in 945 of 25086 words by at most 15 ulp, and
    two uninterrupted runs of this deck differ likewise from their third step
    on (profiles/r21a).  For the bit-for-bit comparison the uninterrupted engine therefore tracks step 4
    from the restored run's own step inputs, as tests/test_gpu_checkpoint.py
    compares a restored context's transport."""
    from test_gpu_checkpoint import compare_transport
    wl = workload(decks[0])
    eng = Engine(wl.grid)
    run = CoupledRun(eng, wl, fp_mode=abi.FP_EXACT)
    for _ in range(3):
        last = run.step()
    assert last["window"] == 0 and last["surface_packets"] > 0
    p = tmp_path / "ec.ckpt"
    assert run.save(p) == eng.census_count() > 0
    wl2 = workload(decks[0])
    eng2 = Engine(wl2.grid)
    back = CoupledRun.restore(eng2, wl2, p, fp_mode=abi.FP_EXACT)
    assert back.n == run.n == 3
    ra, rb = run.step(), back.step()
    for k in ("window", "ec_on", "surface_packets", "fbias", "sources", "census", "escapes", "aborted",
              "packet_steps", "volume_packets", "fp_mode"):
        assert ra[k] == rb[k], k
    assert rb["window"] == 1 and rb["surface_packets"] == 0 and rb["fp_mode"] == "exact"
    compare_transport(eng, eng2)
    np.testing.assert_array_equal(run.state["tea"], back.state["tea"])
    np.testing.assert_array_equal(run.state["Te_new"], back.state["Te_new"])
    for x, y in zip(run.electrons(), back.electrons()):
        assert np.all(np.abs(x - y) <= 1e-10 * np.max(np.abs(x), axis=-1, keepdims=True))
    si = back.next_step_inputs()
    assert not np.any(si.nsurfl) and not np.any(si.nsurfu)
    rb = back.step()
    assert rb["window"] == 1 and rb["surface_packets"] == 0 and rb["aborted"] == 0
    eng.transport_step(si)
    compare_transport(eng, eng2)
    eng.close()
    eng2.close()


def test_fast_build_runs_the_same_windows(replay, decks):
    wl = workload(decks[0], mode=abi.COMTOT_TABLE)
    with Engine(wl.grid) as eng:
        run = CoupledRun(eng, wl)                     # FP_AUTO
        rows = []
        for _ in range(NSTEPS):
            rows.append(dict(run.step()))
            t = eng.tallies()
            for k in TALLY_KEYS:
                assert np.isfinite(np.asarray(t[k], dtype=np.float64)).all(), k
    assert all(r["aborted"] == 0 for r in rows)
    assert [r["surface_packets"] for r in rows] == [s["row"]["surface_packets"] for s in replay[0]]
    assert [r["window"] for r in rows] == [0, 0, 0, 1]
