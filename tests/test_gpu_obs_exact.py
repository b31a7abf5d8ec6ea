"""Exact observer sets on the GPU (c2d_obs_set_exact, c2d_obs_set_exact_kernel
in compton2d_amd/csrc/obsacc.hip): the device's integers against the host
twin's (c2d_obs_exact_host), word for word.  The twin itself is pinned to
Python integers in tests/test_obs_exact_host.py; here nothing has a
tolerance: the states are compared as u64 words, the files as bytes."""
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as OL
from compton2d_amd import abi, observer, synth
from compton2d_amd.coupled import CoupledRun
from compton2d_amd.engine import C2DError, Engine, obs_engine
from test_gpu_observe import _check_sums, _many_events
from test_obs_exact_host import CRAFT_W_MAX, craft_events, craft_lc, craft_sed

pytestmark = pytest.mark.gpu

G = np.load(Path(__file__).resolve().parent / "golden" / "obs.npz", allow_pickle=False)
W_MAX = float(G["events"][:, 2].max())          # _many_events keeps the reference's weights
SIZES = (1, 63, 64, 65, 511, 512, 513, 2500)
_TWIN = {}


def small_sed():
    """3 x 1 x 4: every row privatised in LDS."""
    return observer.sed_binning(15., 1e17, 3, 4e4, 9e5, 0.97, 1.0001, ((1e-3, 1e5, 4, False),))


def long_lc():
    """1024 x 2 x 3, overlapping bands: 40 B x 6 bins a row, so the later
    rows cannot fit the workgroup's LDS and go to global memory."""
    return observer.lc_binning(15., 1e17, ((0.97, 0.9995), (0.9995, 1.0001)), 1e3, 4e4, 1.5e6,
                               ((1e-3, 1e2, 1, False), (1., 1e4, 1, False), (1e2, 1e7, 1, False)))


def _deck_binning(name):
    tool, deck = str(G["tool_" + name]), str(G["deck_" + name])
    return observer.parse_pspt_deck(deck) if tool == "pspt" else observer.parse_plcm_deck(deck)


def _add_deck(eng, name):
    deck = str(G["deck_" + name])
    return eng.obs_set_add_pspt(deck) if str(G["tool_" + name]) == "pspt" else eng.obs_set_add_plcm(deck)


def twin(key, b, w_max, ev):
    if key not in _TWIN:
        _TWIN[key] = observer.exact_host(b, w_max, ev)
    return _TWIN[key]


def device_states(eng, binnings, w_max, batches, route="host"):
    """The states of a fresh exact set of `binnings` after `batches`."""
    eng.obs_set_clear()
    eng.obs_set_exact(w_max)
    ids = [eng.obs_set_add(b) for b in binnings]
    for ev in batches:
        if route == "host":
            eng.obs_set_accumulate(ev)
        elif route == "device":
            import torch
            dev = torch.from_numpy(np.ascontiguousarray(ev)).to("cuda:0")
            torch.cuda.synchronize()
            eng.obs_set_accumulate_device(dev.data_ptr(), len(ev))
        else:
            eng.obs_set_accumulate_file(ev)
    return [eng.obs_set_state(i) for i in ids]


def same(a, b):
    assert a.dtype == b.dtype == np.uint64 and a.shape == b.shape
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (bad[:8], a[bad[:8]], b[bad[:8]])


@pytest.fixture(scope="module")
def eng():
    e = obs_engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def many():
    return _many_events(2500)


@pytest.mark.parametrize("n", SIZES)
def test_device_state_is_the_twins(eng, many, n):
    bs, bl = small_sed(), long_lc()
    ev = many[:n]
    ss, sl = device_states(eng, [bs, bl], W_MAX, [ev])
    same(ss, twin(("sed", n), bs, W_MAX, ev))
    same(sl, twin(("lc", n), bl, W_MAX, ev))
    assert eng.obs_set_exact_info(0) == (observer.state_info(ss)["e"], 0)
    if n == 2500:
        n_t, _, _, rows_s = eng.obs_set_shape(0)
        assert rows_s == n_t == 3                              # the SED: all in LDS
        n_t, n_mu, n_e, rows = eng.obs_set_shape(1)
        assert 0 < rows < n_t                                  # the light curve: both paths
        cnt = observer.state_result(sl).count
        assert cnt[:rows].sum() > 100 and cnt[rows:].sum() > 100, (rows, cnt[:rows].sum(), cnt[rows:].sum())
        assert observer.state_result(ss).count.sum() > 100
        # each member alone is what it is in the set of two
        same(device_states(eng, [bs], W_MAX, [ev])[0], ss)
        same(device_states(eng, [bl], W_MAX, [ev])[0], sl)


def test_a_hot_bin(eng, many):
    """Every event of a launch in one bin: in LDS (the SED) and, for the
    light curve, in a global row, where whole waves aggregate."""
    ev = np.repeat(many[:1], 5000, axis=0)
    ev[:, 2] = np.linspace(0.25, 1.0, len(ev)) * W_MAX
    bs = observer.sed_binning(15., 1e17, 1, -1e9, 1e9, -1.0, 1.0, ((1e-30, 1e30, 1, False),))
    bl = observer.lc_binning(15., 1e17, ((-1.0, 1.0), (1.0, 2.0)), 1e-3, -1e9, 1e9, ((1e-30, 1e30, 1, False),) * 3)
    bl.t0[-1], bl.t1[-1] = 0.0, 1e12                            # the last row takes everything
    assert not np.all(np.diff(bl.t0) >= 0)                      # unsorted: the tools' linear scan
    ss, sl = device_states(eng, [bs, bl], W_MAX, [ev])
    same(ss, twin("hot_sed", bs, W_MAX, ev))
    same(sl, twin("hot_lc", bl, W_MAX, ev))
    assert eng.obs_set_shape(1)[3] < bl.n_t
    assert np.all(observer.state_result(sl).count[-1, 0] == len(ev)) and observer.state_result(sl).count.sum() == 3 * len(ev)
    assert observer.state_result(ss).count[0, 0, 0] == len(ev)


def test_the_crafted_set(eng):
    """Weights one ulp below 2^e, below the quantum, across both limbs, 70 000
    maximal ones in a bin, zero, and the rejected ones (test_obs_exact_host.py)."""
    bs, bl, ev = craft_sed(), craft_lc(), craft_events()
    ss, sl = device_states(eng, [bs, bl], CRAFT_W_MAX, [ev])
    same(ss, twin("craft_sed", bs, CRAFT_W_MAX, ev))
    same(sl, twin("craft_lc", bl, CRAFT_W_MAX, ev))
    assert eng.obs_set_exact_info(0) == (3, 5) and eng.obs_set_exact_info(1) == (3, 5)
    with pytest.raises(C2DError, match="C2D_E_NONFINITE") as err:
        eng.obs_set_result(0)
    assert "5 events" in str(err.value) and "w_max = 1" in str(err.value)
    # the same events in rows past the privatised ones: whole waves aggregate, with carries
    bg = observer.lc_binning(1.0, 0.0, ((-1.0, 0.0), (0.0, 1.0)), 1.0, -1000.0, 3.0,
                             ((1., 1e3, 1, False), (10., 1e4, 1, False), (1e3, 1e4, 1, False)))
    sg, = device_states(eng, [bg], CRAFT_W_MAX, [ev[::-1]])
    assert eng.obs_set_shape(0)[3] < 999
    same(sg, twin("craft_lc_global", bg, CRAFT_W_MAX, ev))
    assert observer.state_result(sg).count[1001].sum() >= 140_000


def test_order_splits_and_routes_give_identical_states(eng, many, tmp_path):
    bs, bl = small_sed(), long_lc()
    want = [twin(("sed", 2500), bs, W_MAX, many), twin(("lc", 2500), bl, W_MAX, many)]
    rng = np.random.default_rng(9)
    batches = ([many[rng.permutation(len(many))]], np.split(many, [1]), np.split(many, [700, 701, 1900]),
               np.split(many[::-1], [512, 1024, 1536, 2048]))
    for b in batches:
        for got, ref in zip(device_states(eng, [bs, bl], W_MAX, b), want):
            same(got, ref)
    for got, ref in zip(device_states(eng, [bs, bl], W_MAX, np.split(many, [1300]), route="device"), want):
        same(got, ref)
    # the file route: the text keeps 8 digits, so the twin reads the file's events back
    p = tmp_path / "p001_evb.dat"
    observer.write_events(p, many)
    back = eng.events_read(p)
    assert back.shape == many.shape
    got = device_states(eng, [bs, bl], float(back[:, 2].max()), [p], route="file")
    same(got[0], observer.exact_host(bs, float(back[:, 2].max()), back))
    same(got[1], observer.exact_host(bl, float(back[:, 2].max()), back))
    hs = observer.bin_events_set(eng, [bs, bl], [many], exact_w_max=W_MAX)
    for h, ref in zip(hs, want):
        r = observer.state_result(ref)
        assert np.array_equal(h.F, r.F) and np.array_equal(h.F2, r.F2) and np.array_equal(h.count, r.count)


def test_two_contexts_export_and_merge(many):
    bs, bl = small_sed(), long_lc()
    a, b = obs_engine(0), obs_engine(0)
    try:
        half = 1201
        sa = device_states(a, [bs, bl], W_MAX, [many[:half]])
        sb = device_states(b, [bs, bl], W_MAX, [many[half:]])
        same(observer.state_merge(sa[1], sb[1]), twin(("lc", 2500), bl, W_MAX, many))
        for i in (0, 1):
            a.obs_set_merge(i, sb[i])
        same(a.obs_set_state(0), twin(("sed", 2500), bs, W_MAX, many))
        same(a.obs_set_state(1), twin(("lc", 2500), bl, W_MAX, many))
        with pytest.raises(C2DError, match="C2D_E_STATE"):
            a.obs_set_add(bs)                                  # the set holds sums now
        # refusals leave the member as it was
        keep = b.obs_set_state(1)
        bad = sa[1].copy()
        bad[abi.OBS_STATE_HEAD_WORDS + 3] ^= np.uint64(4)
        for s in (bad, sa[0], sa[1][:-5], observer.exact_host(bl, 4 * W_MAX, many[:10])):
            with pytest.raises(C2DError, match="C2D_E_ARG"):
                b.obs_set_merge(1, s)
        same(b.obs_set_state(1), keep)
    finally:
        a.close()
        b.close()


def test_written_files_are_byte_identical_across_orders_and_world_sum(tmp_path):
    ev = G["events"]
    rng = np.random.default_rng(2)
    e = obs_engine(0)
    try:
        e.comm_init(Engine.comm_unique_id(), 0, 1)
        names = ("sed_wide", "lc_wide")
        for run, order in enumerate((np.arange(len(ev)), rng.permutation(len(ev)), rng.permutation(len(ev)))):
            e.obs_set_clear()
            e.obs_set_exact(W_MAX)
            ids = [_add_deck(e, n) for n in names]
            e.obs_set_accumulate(ev[order][:5000])
            e.obs_set_accumulate(ev[order][5000:])
            states = [e.obs_set_state(i) for i in ids]
            for d, ws in (("own%d" % run, False), ("world%d" % run, True)):
                (tmp_path / d).mkdir()
                e.obs_set_write(ids[0], str(tmp_path / d / "sed_w.dat"), 1, world_sum=ws)
                e.obs_set_write(ids[1], str(tmp_path / d), 1, world_sum=ws)
            for i, s in zip(ids, states):                      # a world sum of one rank changes nothing
                same(e.obs_set_state(i), s)
            for i, n in zip(ids, names):
                same(states[ids.index(i)], observer.exact_host(_deck_binning(n), W_MAX, ev))
        files = sorted(p.name for p in (tmp_path / "own0").iterdir())
        assert files == sorted(list(G["files_sed_wide"]) + list(G["files_lc_wide"]))
        for d in ("world0", "own1", "world1", "own2", "world2"):
            assert sorted(p.name for p in (tmp_path / d).iterdir()) == files
            for f in files:
                assert (tmp_path / d / f).read_bytes() == (tmp_path / "own0" / f).read_bytes(), (d, f)
    finally:
        e.close()


def test_without_exact_the_set_is_what_it_was(eng, many):
    """After an exact set, a cleared set accumulates f64 sums as before:
    the oracle's, at the f64 tests' own tolerance; the state calls refuse."""
    bs, bl = small_sed(), long_lc()
    device_states(eng, [bs, bl], W_MAX, [many])
    rows_exact = eng.obs_set_shape(1)[3]
    hs = observer.bin_events_set(eng, [bs, bl], [many])
    assert eng.obs_set_shape(1)[3] > rows_exact                 # 3 words a bin again, not 5
    _check_sums(hs[0], OL.obs_bin(bs, many, "det"))
    _check_sums(hs[1], OL.obs_bin(bl, many, "det"))
    for call in (lambda: eng.obs_set_state(0), lambda: eng.obs_set_exact_info(0),
                 lambda: eng.obs_set_merge(0, np.zeros(8, np.uint64)), lambda: eng.obs_set_exact(W_MAX)):
        with pytest.raises(C2DError, match="C2D_E_STATE"):
            call()                                             # not exact; and exact after the first accumulate
    eng.obs_set_clear()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(C2DError, match="C2D_E_ARG"):
            eng.obs_set_exact(bad)
    eng.obs_set_add(bs)
    with pytest.raises(C2DError, match="C2D_E_ARG"):
        eng.obs_set_exact(2.0 ** 500)                           # e out of range for the member there is
    eng.obs_set_exact(2.0 ** 480)
    import copy
    big = copy.copy(bs)
    big.gam_bulk = 2.0 ** 20
    with pytest.raises(C2DError, match="C2D_E_ARG"):
        eng.obs_set_add(big)                                    # and for one added later
    with pytest.raises(C2DError, match="C2D_E_ARG"):
        eng.obs_set_shape(1)
    with pytest.raises(C2DError, match="C2D_E_STATE"):
        eng.obs_set_exact(1.0)                                  # exact already
    eng.obs_set_clear()


def test_a_restored_run_carries_its_observer_set(tmp_path):
    """Three coupled steps binned into an exact set, save, restore into a
    fresh engine with the set re-created, one transport step on the same
    inputs in both, binned: the two states are bitwise equal (such a step's
    events are equal as a set: test_gpu_checkpoint.py)."""
    bs = observer.sed_binning(33., 7.5e15, 20, -1e6, 1e6, 0.0, 1.0, ((1e-10, 1e2, 30, False), (1e2, 1e12, 30, False)))
    bl = observer.lc_binning(33., 7.5e15, ((0.0, 0.9), (0.9, 1.0)), 2e3, -1e6, 1e6,
                             ((1e-10, 1e2, 2, False), (1e-3, 1e3, 1, False), (1e2, 1e12, 2, False)))
    w_max = 1e60

    def make_set(e):
        e.obs_set_clear()
        e.obs_set_exact(w_max)
        return [e.obs_set_add(bs), e.obs_set_add(bl)]

    wl = synth.c3_workload(sources=20_000)
    eng = Engine(wl.grid)
    wl2 = synth.c3_workload(sources=20_000)
    eng2 = Engine(wl2.grid)
    try:
        run = CoupledRun(eng, wl)
        ids = make_set(eng)
        for _ in range(3):
            run.step()
            eng.obs_set_accumulate(None)
        p, q = tmp_path / "run.ckpt", tmp_path / "plain.ckpt"
        run.save(p, observer_set=True)
        saved = [eng.obs_set_state(i) for i in ids]
        assert all(observer.state_result(s).count.sum() > 100 for s in saved)
        assert all(observer.state_info(s)["n_rejected"] == 0 for s in saved)
        run.save(q)
        with pytest.raises(ValueError):
            make_set(eng2)
            CoupledRun.restore(eng2, wl2, q, observer_set=True)       # saved without the set
        eng2.obs_set_clear()
        eng2.obs_set_exact(w_max)
        eng2.obs_set_add(bs)
        with pytest.raises(ValueError):
            CoupledRun.restore(eng2, wl2, p, observer_set=True)       # one member, two states
        eng2.obs_set_clear()
        eng2.obs_set_exact(w_max)
        eng2.obs_set_add(bl)
        eng2.obs_set_add(bs)
        with pytest.raises(ValueError):
            CoupledRun.restore(eng2, wl2, p, observer_set=True)       # the members the other way round
        assert observer.state_result(eng2.obs_set_state(0)).count.sum() == 0
        ids2 = make_set(eng2)
        back = CoupledRun.restore(eng2, wl2, p, observer_set=True)
        assert back.n == run.n == 3
        for i, j, s in zip(ids, ids2, saved):
            same(eng2.obs_set_state(j), s)
        si = run.next_step_inputs()
        eng.transport_step(si)
        eng2.transport_step(si)
        eng.obs_set_accumulate(None)
        eng2.obs_set_accumulate(None)
        for i, j, s in zip(ids, ids2, saved):
            a, b = eng.obs_set_state(i), eng2.obs_set_state(j)
            same(a, b)
            assert observer.state_result(a).count.sum() > observer.state_result(s).count.sum()
    finally:
        eng.close()
        eng2.close()
