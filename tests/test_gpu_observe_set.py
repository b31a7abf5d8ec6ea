"""Observer sets on the GPU (c2d_obs_set_*, c2d_obs_set_kernel in
compton2d_amd/csrc/observe.hip): several pspt SEDs and plcm light curves
filled by one pass over the escape events, against the oracle
(oracle/c2d_obs_oracle.c) per member and against the reference tools' own
output files (tests/golden/obs.npz), with the tolerances of
tests/test_gpu_observe.py and for its reason: counts are exact (the bin
decisions are integer work on the same fdlibm cos as the det oracle); the ew
sums are accumulated with atomics in an unspecified order, rtol 1e-12 on the
raw sums, and the printed %e text then matches the reference's up to a
last-digit flip (rel 2e-6 per number)."""
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as OL
from compton2d_amd import abi, observer, synth
from compton2d_amd.engine import C2DError, Engine, obs_engine
from test_gpu_observe import _check_sums, _many_events, _same_text

pytestmark = pytest.mark.gpu

G = np.load(Path(__file__).resolve().parent / "golden" / "obs.npz", allow_pickle=False)
FOUR = ("sed_mrk421", "sed_wide", "lc_mrk421", "lc_wide")
_ORACLE = {}


def _tool(name):
    return str(G["tool_" + name])


def _deck(name):
    return str(G["deck_" + name])


def _binning(name):
    return observer.parse_pspt_deck(_deck(name)) if _tool(name) == "pspt" else observer.parse_plcm_deck(_deck(name))


def _add(eng, name):
    return eng.obs_set_add_pspt(_deck(name)) if _tool(name) == "pspt" else eng.obs_set_add_plcm(_deck(name))


def _oracle(key, b, ev):
    """The det oracle's sums, computed once per (deck, event set)."""
    if key not in _ORACLE:
        _ORACLE[key] = OL.obs_bin(b, ev, "det")
    return _ORACLE[key]


def _hist(eng, i):
    return observer.Histogram(*eng.obs_set_result(i))


def _sed_overlap():
    b = observer.sed_binning(33., 1e16, 12, -4000., 2e4, 0.999, 1.0,
                             ((1e-2, 1e4, 12, False), (1e-4, 1e2, 10, True), (5., 5e5, 3, False)))
    assert not np.all(np.diff(b.E0) >= 0)
    return b


@pytest.fixture(scope="module")
def eng():
    e = obs_engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def many():
    return _many_events(600_007)


def test_set_fixture_events_match_oracle_and_reference_files(eng, tmp_path):
    ev = G["events"]
    n1 = int(G["n_file1"])
    eng.obs_set_clear()
    ids = {name: _add(eng, name) for name in FOUR}
    assert sorted(ids.values()) == [0, 1, 2, 3]
    eng.obs_set_accumulate(ev[:n1])
    eng.obs_set_accumulate(ev[n1:])
    ms, launches = eng.obs_set_kernel_ms()
    assert launches == 2 and ms > 0                      # one launch per batch, whatever the members
    for name in FOUR:
        b = _binning(name)
        assert eng.obs_set_shape(ids[name])[:3] == (b.n_t, b.n_mu, b.n_e)
        h = _hist(eng, ids[name])
        _check_sums(h, _oracle((name, "fixture"), b, ev))
        out = tmp_path / name
        out.mkdir()
        if _tool(name) == "pspt":
            eng.obs_set_write(ids[name], str(out / b.outfiles[0]), factor=1)
        else:
            eng.obs_set_write(ids[name], str(out), factor=1)
            (out / "py").mkdir()
            for p in observer.write_lc(out / "py", b, h, 1):   # the library's writer = the Python's, byte for byte
                assert (out / p.name).read_bytes() == p.read_bytes(), p.name
        files = list(G["files_" + name])
        assert sorted(p.name for p in out.iterdir() if p.is_file()) == sorted(files)
        for f in files:
            _same_text((out / f).read_text(), str(G["out_%s__%s" % (name, f)]))


def test_set_many_events_both_paths_and_any_order(eng, many):
    """600 007 events: more than one grid sweep at 4 workgroups per CU on 256
    CUs (524 288), partial last wave and block; both light curves keep rows
    on both sides of the LDS split and events land on both sides."""
    eng.obs_set_clear()
    ids = {name: _add(eng, name) for name in FOUR}
    eng.obs_set_accumulate(many)
    assert eng.obs_set_kernel_ms()[1] == 1
    counts = {}
    for name in FOUR:
        b = _binning(name)
        h = _hist(eng, ids[name])
        _check_sums(h, _oracle((name, "many"), b, many))
        counts[name] = h.count
        n_t, _, _, lds_rows = eng.obs_set_shape(ids[name])
        assert 0 <= lds_rows <= n_t
        if _tool(name) == "plcm":
            assert 0 < lds_rows < n_t
            assert h.count[:lds_rows].sum() > 0 and h.count[lds_rows:].sum() > 0, (name, lds_rows)
    eng.obs_set_clear()
    rev = {name: _add(eng, name) for name in reversed(FOUR)}
    assert rev["lc_wide"] == 0 and rev["sed_mrk421"] == 3
    eng.obs_set_accumulate(many)
    for name in FOUR:
        assert np.array_equal(eng.obs_set_result(rev[name])[2], counts[name]), name


def test_set_unsorted_member_beside_sorted(eng, many):
    """Overlapping, unsorted energy regions (the tools' linear first-match
    scan) next to lc_wide (binary search) in one launch."""
    bs, bl = _sed_overlap(), _binning("lc_wide")
    hs = observer.bin_events_set(eng, [bs, bl], [many])
    _check_sums(hs[0], OL.obs_bin(bs, many, "det"))
    _check_sums(hs[1], _oracle(("lc_wide", "many"), bl, many))
    assert hs[0].count.sum() > 1e4 and hs[1].count.sum() > 1e4


def test_set_edge_sizes(eng):
    ev = G["events"]
    b = _binning("sed_wide")
    for n in (0, 1):
        hs = observer.bin_events_set(eng, [b, _binning("lc_wide")], [ev[:n]])
        for h, bb in zip(hs, (b, _binning("lc_wide"))):
            want = OL.obs_bin(bb, ev[:n], "det") if n else tuple(np.zeros((bb.n_t, bb.n_mu, bb.n_e)) for _ in range(3))
            _check_sums(h, want)
    # a set of one member = the single observer
    for name in ("sed_wide", "lc_mrk421"):
        bb = _binning(name)
        one = observer.bin_events_set(eng, [bb], [ev])[0]
        single = observer.bin_events(eng, bb, [ev])
        assert np.array_equal(one.count, single.count)
        np.testing.assert_allclose(one.F, single.F, rtol=1e-12, atol=0)
        np.testing.assert_allclose(one.F2, single.F2, rtol=1e-12, atol=0)
        assert one.count.sum() > 0


def test_set_accumulate_device_pointer(eng):
    """Events already in device memory (a torch tensor on the context's GPU)."""
    import torch
    ev = G["events"]
    dev = torch.from_numpy(ev).to("cuda:0")
    torch.cuda.synchronize()
    eng.obs_set_clear()
    ids = [_add(eng, name) for name in ("sed_mrk421", "lc_mrk421")]
    eng.obs_set_accumulate_device(dev.data_ptr(), len(ev))
    for i, name in zip(ids, ("sed_mrk421", "lc_mrk421")):
        _check_sums(_hist(eng, i), _oracle((name, "fixture"), _binning(name), ev))


def test_set_bins_device_event_buffer_of_two_steps():
    """events=None after each of two transport steps: the sums are the
    oracle's over both steps' events, so the second step waited for the first
    binning before rewriting the event buffer.  A single-observer histogram
    accumulated after the same steps is what it is alone."""
    wl = synth.c2_workload(nz=3, nr=3, sources=100_000, census_capacity=400_000,
                           event_capacity=400_000)
    si = wl.step0
    si.ncycle = 1
    bs = observer.sed_binning(33., 7.5e15, 20, -2e4, 2e4, 0.99, 1.0,
                              ((1e-6, 1e2, 30, False), (1e2, 1e8, 30, False)))
    bl = observer.lc_binning(33., 7.5e15, ((0.99, 0.999), (0.999, 1.0)), 5e2, -2e4, 2e4,
                             ((1e-6, 1e2, 2, False), (1e-3, 1e3, 1, False), (1e2, 1e8, 2, False)))
    with Engine(wl.grid) as e:
        e.obs_set_clear()
        i_s, i_l = e.obs_set_add(bs), e.obs_set_add(bl)
        e.obs_begin(bs)
        e.transport_step(si)
        ev1 = e.events()
        e.obs_accumulate(None)                    # single observer, then the set, after the same step
        e.obs_set_accumulate(None)
        e.transport_step(si)                      # rewrites the event buffer
        ev2 = e.events()
        e.obs_set_accumulate(None)                # the other way round
        e.obs_accumulate(None)
        assert len(ev1) > 10_000 and len(ev2) > 10_000
        ev = np.concatenate([ev1, ev2])
        for i, b in ((i_s, bs), (i_l, bl)):
            h = _hist(e, i)
            _check_sums(h, OL.obs_bin(b, ev, "det"))
            assert h.count.sum() > 1000
        assert e.obs_set_kernel_ms()[1] == 2
        F, F2, cnt, _ = e.obs_result()
        _check_sums(observer.Histogram(F, F2, cnt), OL.obs_bin(bs, ev, "det"))
        alone = observer.bin_events(e, bs, [ev1, ev2])
        assert np.array_equal(cnt, alone.count)
        np.testing.assert_allclose(F, alone.F, rtol=1e-12, atol=0)


def _raises(code):
    return pytest.raises(C2DError, match=code)


def test_set_state_and_argument_errors(eng, tmp_path):
    ev = G["events"]
    small = observer.sed_binning(33., 1e16, 4, 0., 4e4, 0.99, 1.0, ((1e-3, 1e3, 6, False),))
    b0 = _binning("sed_wide")
    eng.obs_begin(b0)                                  # a single-observer histogram the set must not touch
    eng.obs_accumulate(ev)
    before = eng.obs_result()[:3]
    eng.obs_set_clear()
    with _raises("C2D_E_STATE"):
        eng.obs_set_accumulate(ev)                     # empty set
    with _raises("C2D_E_STATE"):
        eng.obs_set_accumulate(None)
    for bad in (0, -1):
        with _raises("C2D_E_ARG"):
            eng.obs_set_shape(bad)
        with _raises("C2D_E_ARG"):
            eng.obs_set_result(bad)
        with _raises("C2D_E_ARG"):
            eng.obs_set_write(bad, str(tmp_path / "x.dat"))
    # the per-member checks of c2d_obs_begin
    import copy
    low = copy.copy(small)
    low.gam_bulk = 0.5
    with _raises("C2D_E_ARG"):
        eng.obs_set_add(low)
    two = copy.copy(small)
    two.mu0, two.mu1 = np.array([0.9, 0.95]), np.array([0.95, 1.0])
    with _raises("C2D_E_ARG"):
        eng.obs_set_add(two)                           # the SED mode has one angular window
    with _raises("C2D_E_ARG"):
        eng.obs_set_add_pspt("p001_evb.dat\n33\n1e16\nx\n30\n1.6e4\n6e4\n0.99944\n0.99964\n1\n1e-7\n1e10\n201\n")
    with _raises("C2D_E_ARG"):
        eng.obs_set_add_plcm("p001_evb.dat\n33\n1e16\nx\n1\n\n\n\n7e2\n0\n7e4\n1\n1e-3\n1\n21\n0\n")
    with _raises("C2D_E_ARG"):
        eng.obs_set_shape(0)                           # the failed adds left nothing behind
    # edges that do not fit one workgroup's LDS: three light curves fit, the fourth does not
    for k in range(3):
        assert eng.obs_set_add_plcm(_deck("lc_wide")) == k
    with _raises("C2D_E_ARG"):
        eng.obs_set_add_plcm(_deck("lc_mrk421"))
    with _raises("C2D_E_ARG"):
        eng.obs_set_shape(3)
    eng.obs_set_accumulate(ev)                         # the three still work
    _check_sums(_hist(eng, 2), _oracle(("lc_wide", "fixture"), _binning("lc_wide"), ev))
    # a ninth member
    eng.obs_set_clear()
    for k in range(abi.OBS_SET_MAX):
        assert eng.obs_set_add(small) == k
    with _raises("C2D_E_ARG"):
        eng.obs_set_add(small)
    # write of a member without a deck; add after the first accumulate
    eng.obs_set_accumulate(ev[:100])
    with _raises("C2D_E_STATE"):
        eng.obs_set_write(0, str(tmp_path / "x.dat"))
    with _raises("C2D_E_ARG"):
        eng.obs_set_result(abi.OBS_SET_MAX)
    eng.obs_set_clear()
    i = eng.obs_set_add_pspt(_deck("sed_wide"))
    eng.obs_set_accumulate(ev[:100])
    with _raises("C2D_E_STATE"):
        eng.obs_set_add(small)
    with _raises("C2D_E_STATE"):
        eng.obs_set_add_plcm(_deck("lc_wide"))
    with _raises("C2D_E_ARG"):
        eng.obs_set_write(i + 1, str(tmp_path / "x.dat"))
    eng.obs_set_clear()
    assert eng.obs_set_add(small) == 0                 # clear re-opens the set
    assert not (tmp_path / "x.dat").exists()
    after = eng.obs_result()[:3]
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    eng.obs_accumulate(ev)                             # and it still accumulates
    assert np.array_equal(eng.obs_result()[2], 2 * before[2])


def test_set_world_sum_of_one_rank_is_the_identity(tmp_path):
    ev = G["events"]
    e = obs_engine(0)
    try:
        e.obs_set_clear()
        i_s, i_l = _add(e, "sed_wide"), _add(e, "lc_wide")
        e.obs_set_accumulate(ev)
        for d in ("own", "world"):
            (tmp_path / d).mkdir()
        with _raises("C2D_E_STATE"):
            e.obs_set_write(i_s, str(tmp_path / "world" / "sed_w.dat"), 1, world_sum=True)   # no communicator yet
        e.comm_init(Engine.comm_unique_id(), 0, 1)
        for d, ws in (("own", False), ("world", True)):
            e.obs_set_write(i_s, str(tmp_path / d / "sed_w.dat"), 1, world_sum=ws)
            e.obs_set_write(i_l, str(tmp_path / d), 1, world_sum=ws)
        names = sorted(p.name for p in (tmp_path / "own").iterdir())
        assert names == sorted(list(G["files_sed_wide"]) + list(G["files_lc_wide"]))
        assert sorted(p.name for p in (tmp_path / "world").iterdir()) == names
        for f in names:
            assert (tmp_path / "own" / f).read_bytes() == (tmp_path / "world" / f).read_bytes(), f
    finally:
        e.close()


def test_single_pspt_world_sum_of_one_rank_is_the_identity(tmp_path):
    """c2d_obs_write_pspt reduces and writes through the set's code path: on
    one rank world_sum changes no byte, and it needs the communicator."""
    e = obs_engine(0)
    try:
        e.obs_begin_pspt(_deck("sed_wide"))
        e.obs_accumulate(G["events"])
        with _raises("C2D_E_STATE"):
            e.obs_write_pspt(str(tmp_path / "world.dat"), 1, world_sum=True)   # no communicator yet
        assert not (tmp_path / "world.dat").exists()
        e.comm_init(Engine.comm_unique_id(), 0, 1)
        e.obs_write_pspt(str(tmp_path / "own.dat"), 1, world_sum=False)
        e.obs_write_pspt(str(tmp_path / "world.dat"), 1, world_sum=True)
        own = (tmp_path / "own.dat").read_bytes()
        assert len(own) > 0 and own == (tmp_path / "world.dat").read_bytes()
        _same_text(own.decode(), str(G["out_sed_wide__%s" % list(G["files_sed_wide"])[0]]))
    finally:
        e.close()
