"""The bundle kernel's per-wave escape queue (KParams.evq_cap, transport.hip
evq_flush) against its inline escape path.

A context made with C2D_EVQ=0 handles every escape inline (imcleak in the lane
loop); contexts with a queue of 1, 5 and 64 entries per wave, and with the
default sizing, must give the same step: the same counters, the same number of
events, the same event rows and census records (as sets: their order within a
shard or chunk is run-dependent either way), and tallies that differ only by
summation order.  Both builds (exact, tabulated comtot), three steps each, so
step 0 runs imcleak's ncycle == 0 branch (no events).

The cases, on the 2 x 2 grid of ssc_tau and a 3 x 3 cut of grid3x4 (thin media:
most packets leave), reach every branch of imcleak:
  axis2x2   rmin = 0: axis pass-through; outer side; top with wmu on both
            sides of 0.98; bottom with tbbl > 0 in zone 1 and tbbl = 0 in zone 2
  inner3x3  rmin > 1e-10: the inner surface ends the copy (erlki)
  few       12 sources per step: fewer escapes in a step (its census packets
            and scattered copies included) than a 64-entry queue holds, so only
            the drain after the lane loop runs
  census    a time step so short that no packet reaches a boundary: no escape
            at all (the queue stays empty and the drain finds nothing)
"""
import dataclasses

import numpy as np
import pytest

from compton2d_amd import abi
from compton2d_amd.engine import C2DError, Engine
from golden_io import IN_KEYS, GoldenCase
from test_gpu_edge import TALLY_KEYS, _no_sources

pytestmark = pytest.mark.gpu

NSTEPS = 3
CAPS = ("1", "5", "64", None)           # C2D_EVQ of the contexts under test (None: default sizing)
BUILDS = {"exact": abi.COMTOT_EXACT, "fast": abi.COMTOT_TABLE}


def _steps(gc, nsteps, edit=lambda si: si):
    """nsteps step inputs of a golden case (the last one repeated, on the clock's next ticks)."""
    out = []
    for n in range(nsteps):
        si = gc.step_inputs(min(n, gc.nsteps - 1))
        if n >= gc.nsteps:
            si = dataclasses.replace(si, ncycle=n, time=si.time + (n - gc.nsteps + 1) * si.dt)
        out.append(edit(si))
    return out


def _cut_r(si, nr):
    """si with its radial zones cut to the inner nr."""
    rep = {}
    for k in IN_KEYS:
        a = getattr(si, k)
        if a is None:
            continue
        if k in ("nsurfu", "nsurfl", "ewsurfu", "ewsurfl", "tbbu", "tbbl"):
            rep[k] = np.ascontiguousarray(a[:nr])
        elif a.ndim >= 2:
            rep[k] = np.ascontiguousarray(a[:, :nr])
    return dataclasses.replace(si, **rep)


def _case(name):
    """(grid overrides -> GridConfig, step inputs) of a case."""
    if name == "axis2x2":
        gc = GoldenCase("ssc_tau")
        tbbl = np.array([0.5, 0.0])
        return gc.grid, _steps(gc, NSTEPS, lambda si: dataclasses.replace(si, tbbl=tbbl))
    if name == "inner3x3":
        gc = GoldenCase("grid3x4")

        def grid(**over):
            g = gc.grid(nr=3, rmin=5.0e14, **over)
            g.r = np.ascontiguousarray(g.r[:3])
            return g
        # 20 x the fixture's sources: a few thousand, several waves
        return grid, _steps(gc, NSTEPS, lambda si: (lambda s: dataclasses.replace(s, nsv=20 * s.nsv))(_cut_r(si, 3)))
    if name == "few":
        gc = GoldenCase("ssc_tau")

        def few(si):
            nsv = np.zeros_like(si.nsv)
            nsv.flat[1] = 12
            return dataclasses.replace(_no_sources(si), nsv=nsv)
        return gc.grid, _steps(gc, NSTEPS, few)
    if name == "census":
        gc = GoldenCase("ssc_tau")
        # c dt = 3e7 cm against zones of 1e15 cm
        return gc.grid, _steps(gc, NSTEPS, lambda si: dataclasses.replace(si, dt=1.0e-3, time=si.ncycle * 1.0e-3))
    raise KeyError(name)


CASES = ("axis2x2", "inner3x3", "few", "census")


def _rows_sorted(a):
    a = np.ascontiguousarray(a)
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def _run(monkeypatch, case, build, evq, **over):
    """One context's results per step: counters, event count, sorted events,
    sorted census, tallies."""
    if evq is None:
        monkeypatch.delenv("C2D_EVQ", raising=False)
    else:
        monkeypatch.setenv("C2D_EVQ", evq)
    grid, steps = _case(case)
    out = []
    with Engine(grid(comtot_mode=BUILDS[build], **over)) as eng:
        for si in steps:
            eng.transport_step(si)
            t = eng.tallies()
            d6, i5, keys = eng.census()
            rec = np.concatenate([keys[:, None].astype(np.float64), (keys[:, None] >> np.uint64(32)).astype(np.float64),
                                  d6, i5.astype(np.float64)], axis=1)
            out.append({"counters": np.array(t["counters"]), "n_ev": eng.last_event_count(),
                        "events": _rows_sorted(eng.events()), "census": _rows_sorted(rec),
                        "tallies": {k: np.array(t[k]) for k in TALLY_KEYS}})
    return out


_REF = {}


def _inline(monkeypatch, case, build):
    """The C2D_EVQ=0 run of (case, build), made once and shared."""
    if (case, build) not in _REF:
        _REF[(case, build)] = _run(monkeypatch, case, build, "0")
    return _REF[(case, build)]


@pytest.mark.parametrize("evq", CAPS, ids=lambda e: "evq_" + (e or "default"))
@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("case", CASES)
def test_queue_matches_inline(monkeypatch, case, build, evq):
    ref = _inline(monkeypatch, case, build)
    got = _run(monkeypatch, case, build, evq)
    for n, (r, g) in enumerate(zip(ref, got)):
        tag = "%s %s evq=%s step %d" % (case, build, evq, n)
        np.testing.assert_array_equal(g["counters"], r["counters"], err_msg=tag + " counters")
        assert g["n_ev"] == r["n_ev"], tag
        np.testing.assert_array_equal(g["events"], r["events"], err_msg=tag + " events")
        np.testing.assert_array_equal(g["census"], r["census"], err_msg=tag + " census")
        for k in TALLY_KEYS:
            np.testing.assert_allclose(g["tallies"][k], r["tallies"][k], rtol=1e-12, atol=0.0,
                                       err_msg="%s %s" % (tag, k))


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_cases_reach_every_branch(monkeypatch, build):
    """What the cases are there for, read off the inline runs."""
    ax = _inline(monkeypatch, "axis2x2", build)
    assert ax[0]["counters"][abi.CNT_ESCAPES] > 0 and ax[0]["n_ev"] == 0      # ncycle == 0: no events
    t = ax[1]["tallies"]
    assert not np.any(t["erlki"])                                             # the axis is no surface
    assert np.any(t["erlko"] > 0) and np.all(t["erlku"] > 0)
    assert t["erlkl"][0] > 0 and t["erlkl"][1] == 0 and t["Ed_in"][0] > 0     # tbbl > 0 / tbbl <= 0
    ev = ax[1]["events"]
    z_top = GoldenCase("ssc_tau").grid().z[-1]
    top = ev[ev[:, 4] == z_top]
    assert len(top) and np.all(top[:, 5] < np.float32(0.98))                  # only wmu < 0.98 is written ...
    assert ax[1]["n_ev"] < ax[1]["counters"][abi.CNT_ESCAPES]                 # ... and some were not
    assert np.any(ev[:, 4] == 0.0)                                            # bottom events, either tbbl
    inn = _inline(monkeypatch, "inner3x3", build)
    assert np.all(inn[1]["tallies"]["erlki"] > 0)
    # a wave takes its sources 1024 at a time (C2D_WORK_CHUNK), so at most
    # ceil(sources / 1024) waves have any: more than 64 escapes each on average,
    # and a 64-entry queue is flushed inside the lane loop too
    for s in (ax[1], inn[1]):
        c = s["counters"]
        assert c[abi.CNT_ESCAPES] > 64 * -(-int(c[abi.CNT_SOURCES]) // 1024)
    assert inn[1]["counters"][abi.CNT_SOURCES] > 2 * 1024                     # several waves at work
    few = _inline(monkeypatch, "few", build)
    # all escapes of a step, the later generations' among them: the bundle kernel's are fewer
    fig = [(int(s["counters"][abi.CNT_ESCAPES]), int(s["counters"][abi.CNT_SOURCES])) for s in few]
    print("few: (escapes, bundle-kernel packets) per step:", fig)
    assert all(0 < e < 64 for e, n in fig), fig
    cen = _inline(monkeypatch, "census", build)
    assert all(s["counters"][abi.CNT_ESCAPES] == 0 and s["n_ev"] == 0 for s in cen)
    assert all(s["counters"][abi.CNT_CENSUS] > 0 for s in cen)


@pytest.mark.parametrize("evq", ("5", None), ids=lambda e: "evq_" + (e or "default"))
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_event_overflow_still_reported(monkeypatch, build, evq):
    """Two events per shard: the first step that writes events overflows."""
    with pytest.raises(C2DError) as ei:
        _run(monkeypatch, "axis2x2", build, evq, event_capacity=64)
    assert abi.ERRORS[ei.value.code] == "C2D_E_EVENT_OVERFLOW"
