"""Binary checkpoints (c2d_checkpoint_write / _read / _info, csrc/ckpt.hip)
on the GPU: the census words, the file's bytes against
compton2d_amd/checkpoint.py, ranges, append and shards, the run state a step
hands to the next (kappa_prev, device electrons, the C2D_FP_AUTO flags,
CoupledRun's host state), and the refusals: every damaged or foreign file is
rejected before a kernel uses what it holds."""
import dataclasses
import shutil

import numpy as np
import pytest

from compton2d_amd import abi, checkpoint as CK, engine as E, synth
from compton2d_amd.coupled import CoupledRun
from compton2d_amd.engine import C2DError, Engine
from golden_io import GoldenCase

pytestmark = pytest.mark.gpu

CHUNK = 1000
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500)
TALLY_KEYS = ("edep", "prdep", "ecens", "npcen", "n_field", "E_IC", "nelectron", "fout", "edout",
              "erlki", "erlko", "erlku", "erlkl", "Ed_in")


@pytest.fixture(autouse=True)
def chunk_env(monkeypatch):
    monkeypatch.setenv("C2D_CKPT_CHUNK", str(CHUNK))


def small_grid(nz=3, nr=3, inplace=0, mode=abi.COMTOT_TABLE, capacity=4096, **kw):
    wl = synth.c2_workload(nz=nz, nr=nr, sources=1, comtot_mode=mode, census_capacity=capacity,
                           event_capacity=1 << 10)
    return dataclasses.replace(wl.grid, census_inplace=inplace, queue_capacity=1 << 10, **kw)


def synthetic_records(grid, n, seed=11):
    """n census records on `grid`, every field inside what a census holds."""
    rng = np.random.default_rng(seed + n)
    d6 = np.zeros((n, 6))
    r0, r1 = grid.rmin, float(np.asarray(grid.r)[-1])
    d6[:, 0] = r0 + (r1 - r0) * rng.random(n)
    d6[:, 1] = grid.zmin + (float(np.asarray(grid.z)[-1]) - grid.zmin) * rng.random(n)
    d6[:, 2] = rng.uniform(-0.99, 0.99, n)
    d6[:, 3] = rng.uniform(1e-3, 6.28, n)
    d6[:, 4] = rng.uniform(1.0, 2.0, n) * 1e40
    eph = np.asarray(grid.E_ph)
    d6[:, 5] = np.exp(rng.uniform(np.log(eph[1]), np.log(eph[-2]), n))
    i5 = np.zeros((n, 5), np.int32)
    i5[:, 0] = rng.integers(0, abi.NPHOMAX + 1, n)
    i5[:, 1] = rng.integers(0, 6, n)
    i5[:, 2] = 1
    i5[:, 3] = rng.integers(1, grid.nz + 1, n)
    i5[:, 4] = rng.integers(1, grid.nr + 1, n)
    keys = rng.integers(1, 1 << 62, n, dtype=np.uint64)
    return d6, i5, keys


def words(eng):
    """The census as c2d_census_pack's words [n, 8] u64, through a torch buffer."""
    import torch
    n = eng.census_count()
    raw = torch.empty(max(n, 1) * abi.CENSUS_REC_WORDS, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()        # the pack runs on the context's own stream
    if n:
        eng.census_pack(0, n, raw.data_ptr())
    return raw[:n * abi.CENSUS_REC_WORDS].view(n, abi.CENSUS_REC_WORDS).cpu().numpy().view(np.uint64).copy()


def same_census(a, b):
    for x, y in zip(a.census(), b.census()):
        np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def code(fn, *a, **kw):
    with pytest.raises(C2DError) as e:
        fn(*a, **kw)
    return e.value.code, str(e.value)


# ------------------------------------------------------------ 1. round trip
@pytest.mark.parametrize("wi,ri", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_round_trip_of_the_words_and_the_bytes(tmp_path, wi, ri):
    gw, gr = small_grid(inplace=wi), small_grid(inplace=ri)
    w, r = Engine(gw), Engine(gr)
    for n in SIZES:
        w.import_census(*synthetic_records(gw, n))
        p = tmp_path / ("c%d.ckpt" % n)
        assert w.checkpoint_write(p, b"blob %d" % n) == n
        ww = words(w)
        got, user = r.checkpoint_read(p)
        assert (got, user) == (n, b"blob %d" % n) and r.census_count() == n
        np.testing.assert_array_equal(words(r), ww, err_msg="n = %d" % n)
        same_census(w, r)
        q = tmp_path / ("py%d.ckpt" % n)
        CK.write_file(q, gw, ww, user=b"blob %d" % n)
        assert q.read_bytes() == p.read_bytes(), n
        seen = 0
        for k, off, cw, dg in CK.iter_chunks(p):          # recomputes every digest, and the trailer's
            assert dg == CK.digest(cw, k * CHUNK)
            seen += len(cw)
        assert seen == n
        info = E.checkpoint_info(p)
        assert info["n_records"] == n and info["chunk"] == CHUNK and info["encoded"] == 1
        assert not info["has_kappa"] and not info["has_electrons"]
        lc = w.last_checkpoint()
        assert lc["chunks"] == (n + CHUNK - 1) // CHUNK and lc["bytes"] == p.stat().st_size
    w.close()
    r.close()


# ------------------------------------------------------ 2. ranges and append
@pytest.fixture(scope="module")
def file2500(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckpt")
    g = small_grid()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("C2D_CKPT_CHUNK", str(CHUNK))
        with Engine(g) as e:
            e.import_census(*synthetic_records(g, 2500))
            p = d / "r2500.ckpt"
            e.checkpoint_write(p)
            return p, words(e)


def test_ranges_give_the_matching_slice(file2500):
    p, ww = file2500
    with Engine(small_grid(inplace=1)) as r:
        for first in (0, 1, 999, 1000, 1001, 1500):
            for count in (0, 1, 1000, 1001, -1):
                want = ww[first:] if count < 0 else ww[first:first + count]
                got, _ = r.checkpoint_read(p, first=first, count=count)
                assert got == len(want), (first, count)
                np.testing.assert_array_equal(words(r), want, err_msg="%d %d" % (first, count))


def test_append_gives_the_concatenation(tmp_path, file2500):
    p, ww = file2500
    g = small_grid()
    with Engine(g) as a, Engine(small_grid(inplace=1)) as r:
        a.import_census(*synthetic_records(g, 700, seed=3))
        q = tmp_path / "b.ckpt"
        a.checkpoint_write(q)
        wb = words(a)
        r.checkpoint_read(q)
        assert r.checkpoint_read(p, append=True, census_only=True)[0] == 2500
        np.testing.assert_array_equal(words(r), np.concatenate([wb, ww]))
        assert r.checkpoint_read(q, first=100, count=50, append=True)[0] == 50
        np.testing.assert_array_equal(words(r), np.concatenate([wb, ww, wb[100:150]]))


def by_key(w):
    return w[np.argsort(w[:, 7], kind="stable")]


def test_shards_restore_on_another_number_of_contexts(tmp_path):
    """World 2 -> 1 with plan_shards, then one file -> two contexts by ranges: the union of the keys, the
    records equal per key."""
    gc = GoldenCase("ssc_tau")
    shards, files = [], []
    for rank in range(2):
        with Engine(gc.grid(comtot_mode=abi.COMTOT_EXACT, device=0, rank=rank, world=2)) as e:
            e.transport_step(gc.step_inputs(0))
            f = tmp_path / ("shard%d.ckpt" % rank)
            assert e.checkpoint_write(f) == e.census_count() > 0
            shards.append(words(e))
            files.append(f)
    union = by_key(np.concatenate(shards))
    assert len(np.unique(union[:, 7])) == len(union)
    infos = [(f, E.checkpoint_info(f)) for f in files]
    assert [i["world"] for _, i in infos] == [2, 2] and [i["rank"] for _, i in infos] == [0, 1]
    (plan,) = CK.plan_shards(infos, 1)
    with Engine(gc.grid(comtot_mode=abi.COMTOT_EXACT, device=0)) as one:
        for i, (f, first, count) in enumerate(plan):
            assert one.checkpoint_read(f, first, count, append=i > 0)[0] == count
        np.testing.assert_array_equal(by_key(words(one)), union)
        whole = tmp_path / "whole.ckpt"
        one.checkpoint_write(whole)
    halves = []
    plan = CK.plan_shards([(whole, E.checkpoint_info(whole))], 2)
    assert abs(sum(c for _, _, c in plan[0]) - sum(c for _, _, c in plan[1])) <= 1
    for rank in range(2):
        with Engine(gc.grid(comtot_mode=abi.COMTOT_EXACT, device=0, rank=rank, world=2, census_inplace=1)) as e:
            for i, (f, first, count) in enumerate(plan[rank]):
                e.checkpoint_read(f, first, count, append=i > 0)
            halves.append(words(e))
    np.testing.assert_array_equal(by_key(np.concatenate(halves)), union)


# ------------------------------------------------------------- 3. run state
def sort_rows(a):
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def compare_transport(a, b):
    ta, tb = a.tallies(), b.tallies()
    np.testing.assert_array_equal(ta["counters"], tb["counters"])
    for k in TALLY_KEYS:
        ref = np.asarray(ta[k])
        np.testing.assert_allclose(tb[k], ref, rtol=1e-11, atol=1e-13 * max(np.abs(ref).max(), 1e-300), err_msg=k)
    (d6a, i5a, ka), (d6b, i5b, kb) = a.census(), b.census()
    oa, ob = np.argsort(ka), np.argsort(kb)
    np.testing.assert_array_equal(ka[oa], kb[ob])
    np.testing.assert_array_equal(d6a[oa].view(np.uint64), d6b[ob].view(np.uint64))
    np.testing.assert_array_equal(i5a[oa], i5b[ob])
    np.testing.assert_array_equal(sort_rows(a.events()).view(np.uint64), sort_rows(b.events()).view(np.uint64))


def compare_coupled_step(run, back):
    ra, rb = run.step(), back.step()
    for k in ("sources", "census", "escapes", "aborted", "packet_steps", "volume_packets"):
        assert ra[k] == rb[k], k
    assert ra["fp_mode"] == rb["fp_mode"] and ra["fp_mode"] in ("exact", "fast")
    np.testing.assert_array_equal(run.state["tea"], back.state["tea"])
    np.testing.assert_array_equal(run.state["Te_new"], back.state["Te_new"])
    for x, y in zip(run.electrons(), back.electrons()):
        tol = 1e-10 * np.max(np.abs(x), axis=-1, keepdims=True)          # the fast FP's stated tolerance
        assert np.all(np.abs(x - y) <= tol)
    return ra["fp_mode"]


@pytest.mark.parametrize("mode", [abi.COMTOT_TABLE, abi.COMTOT_EXACT])
def test_run_state_survives_save_and_restore(tmp_path, mode):
    wl = synth.c3_workload(sources=20_000, comtot_mode=mode)
    eng = Engine(wl.grid)
    run = CoupledRun(eng, wl)
    for _ in range(3):
        run.step()
    p = tmp_path / "run.ckpt"
    assert run.save(p) == eng.census_count() > 0
    info = E.checkpoint_info(p)
    assert info["has_kappa"] and info["has_electrons"] and info["fp_auto_known"] == 1
    assert info["encoded"] == int(mode == abi.COMTOT_TABLE) and info["ncycle"] == 2
    wl2 = synth.c3_workload(sources=20_000, comtot_mode=mode)
    eng2 = Engine(wl2.grid)
    back = CoupledRun.restore(eng2, wl2, p)
    assert back.n == run.n == 3
    np.testing.assert_array_equal(back.ecens_prev, run.ecens_prev)
    for x, y in zip(eng.electron_state(), eng2.electron_state()):
        np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64))
    np.testing.assert_array_equal(words(eng), words(eng2))
    # one transport step on the same host-array inputs: it reads kappa_prev (H3)
    si = run.next_step_inputs()
    eng.transport_step(si)
    eng2.transport_step(si)
    compare_transport(eng, eng2)
    # and the coupled step carries on
    compare_coupled_step(run, back)
    eng.close()
    eng2.close()


def test_a_restored_run_writes_the_file_it_came_from(tmp_path):
    """No timestamps, and nothing of the state is lost on the way: the same state gives the same bytes."""
    wl = synth.c3_workload(sources=20_000)
    with Engine(wl.grid) as eng:
        run = CoupledRun(eng, wl)
        for _ in range(2):
            run.step()
        p = tmp_path / "run.ckpt"
        run.save(p)
    wl2 = synth.c3_workload(sources=20_000)
    with Engine(wl2.grid) as eng2:
        back = CoupledRun.restore(eng2, wl2, p)
        q = tmp_path / "again.ckpt"
        back.save(q)
        assert q.read_bytes() == p.read_bytes()


def test_restored_fp_auto_flags_choose_the_same_mode(tmp_path):
    """The zones taken off the tea clamp (tests/test_gpu_c3.py's recipe): the update runs fast and leaves
    C2D_FP_AUTO's carried decision behind; the restored run's next update picks what the original's does."""
    wl = synth.c3_workload(sources=20_000)
    eng = Engine(wl.grid)
    run = CoupledRun(eng, wl)
    run.step()
    run.step()
    nz, nr = wl.grid.nz, wl.grid.nr
    cell = np.arange(nz * nr, dtype=np.float64).reshape(nz, nr)
    run.state["tea"] = 300.0 * (1.0 + 0.007 * (cell % 41))
    assert run.step()["fp_mode"] == "fast"
    p = tmp_path / "off.ckpt"
    run.save(p)
    wl2 = synth.c3_workload(sources=20_000)
    eng2 = Engine(wl2.grid)
    back = CoupledRun.restore(eng2, wl2, p)
    compare_coupled_step(run, back)
    compare_coupled_step(run, back)
    eng.close()
    eng2.close()


# -------------------------------------------------------------- 4. refusals
def flip(path, offset, bit=0):
    raw = bytearray(path.read_bytes())
    raw[offset] ^= 1 << bit
    path.write_bytes(bytes(raw))


def test_a_damaged_chunk_is_refused(tmp_path, file2500):
    good, ww = file2500
    h = CK.read_header(good)
    bad = tmp_path / "bit.ckpt"
    shutil.copy(good, bad)
    flip(bad, CK.chunk_offset(h, 2) + CK.HEAD_BYTES + 64 * 17 + 8 * 4 + 3, 5)      # chunk 2, record 17, ew
    g = small_grid()
    with Engine(g) as r:
        r.import_census(*synthetic_records(g, 300, seed=8))
        before = words(r)
        c, msg = code(r.checkpoint_read, bad, append=True)
        assert c == abi.C2D_E_IO and "chunk 2" in msg and str(CK.chunk_offset(h, 2)) in msg
        assert r.census_count() == 300
        np.testing.assert_array_equal(words(r), before)
        c, msg = code(r.checkpoint_read, bad)
        assert c == abi.C2D_E_IO and "chunk 2" in msg
        assert code(r.census)[0] == abi.C2D_E_STATE                  # replace mode: the census is lost
        assert code(r.checkpoint_write, tmp_path / "x.ckpt")[0] == abi.C2D_E_STATE
        r.census_truncate(0)
        assert r.census_count() == 0 and r.checkpoint_read(good)[0] == 2500
        np.testing.assert_array_equal(words(r), ww)
        # truncated in the middle of a chunk
        cut = tmp_path / "cut.ckpt"
        cut.write_bytes(good.read_bytes()[:CK.chunk_offset(h, 1) + 5000])
        assert code(r.checkpoint_read, cut)[0] == abi.C2D_E_IO
        np.testing.assert_array_equal(words(r), ww)


def test_a_record_off_the_grid_is_refused_by_the_record_check(tmp_path, file2500):
    good, ww = file2500
    g = small_grid()
    w = ww.copy()
    jk = w[1200, 6] & np.uint64(0xffffffff)
    off_grid = (jk & ~np.uint64(0x7f << 16)) | np.uint64((g.nz + 1) << 16)
    w[1200, 6] = (w[1200, 6] & ~np.uint64(0xffffffff)) | off_grid
    bad = tmp_path / "cell.ckpt"
    CK.write_file(bad, g, w)                       # every digest is right: only the record check can see it
    assert sum(len(c) for _, _, c, _ in CK.iter_chunks(bad)) == 2500
    with Engine(g) as r:
        c, msg = code(r.checkpoint_read, bad, first=1000, count=-1)
        assert c == abi.C2D_E_IO and "chunk 1" in msg and "record 200" in msg
        r.census_truncate(0)
        r.import_census(*synthetic_records(g, 10))
        c, msg = code(r.checkpoint_read, bad, append=True)
        assert c == abi.C2D_E_IO and r.census_count() == 10          # chunk 0 taken back, nothing of chunk 1
        for col, val in ((6, np.uint64(0)), (4, np.float64(np.inf).view(np.uint64)),
                         (6, ww[7, 6] | np.uint64(200 << 32))):      # no E_ph bin; Inf; jgpsp = 200
            w = ww.copy()
            w[7, col] = val
            CK.write_file(bad, g, w)
            c, msg = code(r.checkpoint_read, bad, append=True)
            assert c == abi.C2D_E_IO and "chunk 0" in msg and r.census_count() == 10


def test_foreign_files_are_refused_with_the_context_unchanged(tmp_path, file2500):
    good, ww = file2500
    g = small_grid()
    with Engine(g) as r:
        r.import_census(*synthetic_records(g, 40))
        before = words(r)
        for name, other in (("nr", small_grid(nr=4)), ("encoding", small_grid(mode=abi.COMTOT_EXACT)),
                            ("grid digest", dataclasses.replace(g, rmin=1.0))):
            f = tmp_path / "other.ckpt"
            with Engine(other) as o:
                o.import_census(*synthetic_records(other, 5))
                o.checkpoint_write(f)
            c, msg = code(r.checkpoint_read, f)
            assert c == abi.C2D_E_ARG and name in msg, (name, msg)
            np.testing.assert_array_equal(words(r), before)
        with Engine(small_grid(mode=abi.COMTOT_EXACT)) as exact:     # the issue's direction: a TABLE file, an EXACT context
            exact.import_census(*synthetic_records(g, 40))
            kept = words(exact)
            c, msg = code(exact.checkpoint_read, good)
            assert c == abi.C2D_E_ARG and "encoding" in msg
            np.testing.assert_array_equal(words(exact), kept)
        with Engine(small_grid(capacity=1000)) as tight:
            tight.import_census(*synthetic_records(g, 40))
            assert code(tight.checkpoint_read, good)[0] == abi.C2D_E_CENSUS_OVERFLOW
            assert code(tight.checkpoint_read, good, first=0, count=961, append=True)[0] == abi.C2D_E_CENSUS_OVERFLOW
            np.testing.assert_array_equal(words(tight), before)
            assert tight.checkpoint_read(good, first=0, count=960, append=True)[0] == 960
        for damage in (0, 121):                                      # magic; the header's digest
            f = tmp_path / "hdr.ckpt"
            shutil.copy(good, f)
            flip(f, damage)
            assert code(r.checkpoint_read, f)[0] == abi.C2D_E_IO
        assert code(r.checkpoint_read, tmp_path / "missing.ckpt")[0] == abi.C2D_E_IO
        np.testing.assert_array_equal(words(r), before)


def test_a_nan_in_the_census_leaves_the_older_file(tmp_path, file2500):
    good, _ = file2500
    p = tmp_path / "keep.ckpt"
    shutil.copy(good, p)
    g = small_grid(mode=abi.COMTOT_EXACT)
    with Engine(g) as e:
        d6, i5, keys = synthetic_records(g, 1500)
        d6[1234, 4] = np.nan
        e.import_census(d6, i5, keys)
        c, msg = code(e.checkpoint_write, p)
        assert c == abi.C2D_E_NONFINITE and "record 1235" in msg
        assert p.read_bytes() == good.read_bytes() and not (tmp_path / "keep.ckpt.tmp").exists()
        e.census_truncate(1000)                                      # the NaN is gone
        assert code(e.checkpoint_write, tmp_path / "no_such_dir" / "x.ckpt")[0] == abi.C2D_E_IO
        assert e.checkpoint_write(p) == 1000 and E.checkpoint_info(p)["encoded"] == 0


# ------------------------------------- 5. before the first step, empty census
def test_before_the_first_step(tmp_path):
    g = small_grid()
    p = tmp_path / "fresh.ckpt"
    with Engine(g) as a, Engine(small_grid(inplace=1)) as b:
        assert a.checkpoint_write(p, b"") == 0
        info = E.checkpoint_info(p)
        assert info["n_records"] == 0 and not info["has_kappa"] and not info["has_electrons"]
        assert info["fp_auto_known"] == 0 and info["file_bytes"] == 128 + 24 == p.stat().st_size
        b.import_census(*synthetic_records(g, 9))
        assert b.checkpoint_read(p) == (0, b"") and b.census_count() == 0
        assert code(b.run_step)[0] == abi.C2D_E_STATE                # as on a new context
        assert code(b.electron_state)[0] == abi.C2D_E_STATE
