"""The checkpoint file on the CPU: compton2d_amd/checkpoint.py (the format in
numpy) against the library's host code (csrc/c2d_ckpt_host.h behind
c2d_checkpoint_info, which needs no GPU), the digest's properties,
plan_shards, and the host code as a stand-alone program
(tests/c/ckpt_main.cpp) over good and damaged files under
-fsanitize=address,undefined."""
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from compton2d_amd import abi, checkpoint as CK, engine
from golden_io import GoldenCase

HERE = Path(__file__).resolve().parent
MAIN = HERE / "c" / "ckpt_main.cpp"
GXX_FLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Werror"]
CHUNK = 1000
SIZES = (0, 1, 1000, 2 * CHUNK + 1)


def grid():
    return GoldenCase("grid3x4").grid()


def synthetic_words(n, seed=5):
    """n packed records with cells on the 3 x 4 grid (only the host format is under test)."""
    rng = np.random.default_rng(seed)
    w = np.zeros((n, 8), np.uint64)
    w[:, :6] = rng.random((n, 6)).view(np.uint64)
    jk = rng.integers(1, 4, n) | (rng.integers(1, 401, n) << 7) | (rng.integers(1, 4, n) << 16)
    w[:, 6] = jk.astype(np.uint64)
    w[:, 7] = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    return w


def good_file(d, n, user=b"seven b", tables=False):
    g = grid()
    p = d / ("good_%d_%d.ckpt" % (n, tables))
    rng = np.random.default_rng(n)
    kw = {}
    if tables:
        kw = dict(kappa_prev=rng.random((g.nz, g.nr, abi.N_VOL)), f_nt=rng.random((g.nz, g.nr, abi.NUM_NT)),
                  Pnt=rng.random((g.nz, g.nr, abi.NUM_NT)), ncycle=3, time=1.5, dt=0.5, fp_auto_known=True)
    CK.write_file(p, g, synthetic_words(n), user=user, chunk=CHUNK, **kw)
    return p, kw


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tables", (False, True))
def test_write_file_round_trips_through_info_header_and_chunks(tmp_path, n, tables):
    p, kw = good_file(tmp_path, n, tables=tables)
    g = grid()
    info = engine.checkpoint_info(p)
    h = CK.read_header(p)
    assert info["n_records"] == h["n_records"] == n and info["chunk"] == h["chunk"] == CHUNK
    assert (info["nz"], info["nr"], info["nmu"]) == (g.nz, g.nr, int(np.asarray(g.mu).size))
    assert info["grid_digest"] == h["grid_digest"] == CK.grid_digest(g)
    assert info["seed"] == g.seed and info["encoded"] == 0 and info["user_bytes"] == 7
    assert info["has_kappa"] == info["has_electrons"] == tables
    assert info["fp_auto_known"] == int(tables) and info["ncycle"] == (3 if tables else 0)
    assert info["file_bytes"] == p.stat().st_size == CK.file_bytes(h)
    assert CK.read_user(p) == b"seven b"
    chunks = list(CK.iter_chunks(p))
    assert [len(w) for _, _, w, _ in chunks] == [min(CHUNK, n - c) for c in range(0, n, CHUNK)]
    for k, off, w, dg in chunks:
        assert off == CK.chunk_offset(h, k) and dg == CK.digest(w, k * CHUNK)
    assert np.array_equal(CK.read_words(p), synthetic_words(n))
    t = CK.read_tables(p)
    assert set(t) == ({"kappa_prev", "f_nt", "Pnt"} if tables else set())
    for k in t:
        assert np.array_equal(t[k], kw[k])
    # the same state gives the same bytes
    q = tmp_path / "again.ckpt"
    CK.write_file(q, g, synthetic_words(n), user=b"seven b", chunk=CHUNK, **kw)
    assert q.read_bytes() == p.read_bytes()


def test_digest_sees_a_flipped_bit_and_a_swap_but_not_the_reduction_order():
    w = synthetic_words(257, seed=9)
    s0, x0 = CK.digest(w, 4096)
    rng = np.random.default_rng(1)
    for rec, word, bit in itertools.chain([(0, 0, 0), (256, 7, 63), (100, 6, 31)],
                                          zip(rng.integers(0, 257, 40), rng.integers(0, 8, 40), rng.integers(0, 64, 40))):
        v = w.copy()
        v[rec, word] ^= np.uint64(1) << np.uint64(bit)
        assert CK.digest(v, 4096)[0] != s0, (rec, word, bit)
    v = w.copy()
    v[[3, 200]] = v[[200, 3]]
    assert CK.digest(v, 4096)[0] != s0
    assert CK.digest(w, 4097)[0] != s0           # the index enters
    h = CK.hashes(w, 4096)
    for seed in range(3):
        p = np.random.default_rng(seed).permutation(len(h))
        assert int(np.add.reduce(h[p], dtype=np.uint64)) == s0 and int(np.bitwise_xor.reduce(h[p])) == x0
    # a chunk's digest is the sum / xor of its parts: a wave may reduce any subset first
    a, b = CK.digest(w[:100], 4096), CK.digest(w[100:], 4196)
    assert (a[0] + b[0]) % (1 << 64) == s0 and a[1] ^ b[1] == x0
    assert CK.digest(np.zeros((0, 8), np.uint64)) == (0, 0)


def test_mix_is_splitmix64s_finaliser():
    # SplitMix64 seeded with 0: the first output is mix(0x9E3779B97F4A7C15)
    assert int(CK.mix(np.array([0x9E3779B97F4A7C15], np.uint64))[0]) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("sizes,world", [((7,), 2), ((5, 4), 1), ((10, 3, 8), 2), ((0, 5), 3), ((1000, 1, 2501), 4)])
def test_plan_shards_assigns_every_record_exactly_once(sizes, world):
    infos = [("shard%d" % i, {"n_records": n}) for i, n in enumerate(sizes)]
    plan = CK.plan_shards(infos, world)
    assert len(plan) == world
    counts = [sum(c for _, _, c in parts) for parts in plan]
    assert sum(counts) == sum(sizes) and max(counts) - min(counts) <= 1
    seen = {f: np.zeros(n, np.int64) for f, n in zip([i[0] for i in infos], sizes)}
    order = []
    for parts in plan:
        for f, first, count in parts:
            assert count > 0
            seen[f][first:first + count] += 1
            order.append((f, first))
    assert all((v == 1).all() for v in seen.values())
    assert order == sorted(order)                 # the records keep their order over the ranks


def damaged_files(d):
    """{name: (path, n_records or None)}: None must be refused with C2D_E_IO."""
    p, _ = good_file(d, 2 * CHUNK + 1, tables=True)
    raw = p.read_bytes()
    h = CK.read_header(p)
    out = {}

    def put(name, data):
        q = d / (name + ".ckpt")
        q.write_bytes(data)
        out[name] = (q, None)

    for k in range(CK.HEADER_BYTES):
        put("cut_%03d" % k, raw[:k])
    put("cut_mid_chunk", raw[:CK.chunk_offset(h, 1) + 100])
    put("cut_trailer", raw[:-1])
    put("magic", b"X" + raw[1:])
    put("version", raw[:8] + b"\x02" + raw[9:])
    put("header_digest_bit", raw[:120] + bytes([raw[120] ^ 1]) + raw[121:])
    put("header_field_bit", raw[:16] + bytes([raw[16] ^ 1]) + raw[17:])
    t = len(raw) - CK.TRAILER_BYTES
    put("trailer_n", raw[:t + 8] + (2 * CHUNK).to_bytes(8, "little") + raw[t + 16:])
    put("trailer_magic", raw[:t] + b"\0" + raw[t + 1:])
    put("trailer_digest", raw[:-1] + bytes([raw[-1] ^ 0x80]))
    c1 = CK.chunk_offset(h, 1)
    put("chunk_count", raw[:c1] + (CHUNK - 1).to_bytes(8, "little") + raw[c1 + 8:])
    put("chunk_digest_word", raw[:c1 + 8] + bytes([raw[c1 + 8] ^ 1]) + raw[c1 + 9:])
    put("longer", raw + b"\0" * 8)
    return out


def test_info_refuses_damaged_files(tmp_path):
    for name, (path, _) in damaged_files(tmp_path).items():
        with pytest.raises(engine.C2DError) as e:
            engine.checkpoint_info(path)
        assert e.value.code == abi.C2D_E_IO, name
        with pytest.raises((ValueError, OSError)):
            list(CK.iter_chunks(path))
    with pytest.raises(engine.C2DError) as e:
        engine.checkpoint_info(tmp_path / "missing.ckpt")
    assert e.value.code == abi.C2D_E_IO


def test_standalone_program_under_host_sanitizers(tmp_path):
    """Host C++ only: c2d_ckpt_host.h in a program of its own, built with ASan + UBSan, over the good files and
    every damaged one: each gives its code, and the sanitizers report nothing (a report fails the run)."""
    exe = tmp_path / "ckpt_main"
    subprocess.run(["g++", "-O0"] + GXX_FLAGS + ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=undefined", "-o", str(exe), str(MAIN)], check=True)
    rows = []
    for n in SIZES:
        for tables in (False, True):
            rows.append((0, n, good_file(tmp_path, n, tables=tables)[0]))
    for path, _ in damaged_files(tmp_path).values():
        rows.append((abi.C2D_E_IO, 0, path))
    rows.append((abi.C2D_E_IO, 0, tmp_path / "missing.ckpt"))
    lst = tmp_path / "files.lst"
    lst.write_text("".join("%d %d %s\n" % r for r in rows))
    p = subprocess.run([str(exe), "list", str(lst)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "%d files, 0 failures" % len(rows) in p.stdout
    # the program's header fields and digest are numpy's
    good = good_file(tmp_path, 2 * CHUNK + 1, tables=True)[0]
    p = subprocess.run([str(exe), "info", str(good)], capture_output=True, text=True, check=True)
    f = dict(kv.split("=") for kv in p.stdout.split()[1:])
    h = CK.read_header(good)
    for k in ("nz", "nr", "nmu", "grid_digest", "seed", "n_records", "chunk", "user_bytes", "sections", "ncycle"):
        assert int(f[k]) == h[k], k
    assert float(f["time"]) == h["time"] and int(f["file_bytes"]) == good.stat().st_size
    w = synthetic_words(3, seed=2).reshape(-1)[:19]          # a last group that is zero-padded
    p = subprocess.run([str(exe), "digest", "77"] + ["%x" % int(v) for v in w], capture_output=True, text=True,
                       check=True)
    assert tuple(int(v) for v in p.stdout.split()) == CK.digest(w, 77)
