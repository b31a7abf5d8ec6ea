"""The checkpoint file of c2d_checkpoint_write / c2d_checkpoint_read in numpy.

The format is specified in include/compton2d.h ("Checkpoints") and
implemented by csrc/c2d_ckpt_host.h and csrc/ckpt.hip; this module mirrors
it: `read_header`, `iter_chunks` and `digest` read and check a file,
`write_file` writes the same bytes from exported state (the yardstick of the
library's route, as census_io.py is for the text files), and `plan_shards`
spreads the shard files of an old run over another number of ranks.

Little-endian, every part 8-byte aligned:

    header (128 B) | user blob, zero-padded to 8 | kappa_prev | f_nt | Pnt |
    census chunks | trailer (24 B)

A table section and a census chunk begin with (count, digest_sum, digest_xor).
"""
from __future__ import annotations

import os
import struct
from typing import Iterable, Iterator, Optional, Sequence

import numpy as np

from . import abi

MAGIC = 0x0054504B43443243            # "C2DCKPT\0"
TRAILER_MAGIC = 0x00444E4543443243    # "C2DCEND\0"
HEADER_BYTES = 128
HEAD_BYTES = 24
TRAILER_BYTES = 24
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
DEFAULT_CHUNK = 1 << 20
REC_WORDS = abi.CENSUS_REC_WORDS

_HEADER = struct.Struct("<QIIiiiiQQiiiIddqqiiqQQ")
_FIELDS = ("magic", "version", "header_bytes", "nz", "nr", "nmu", "encoded", "grid_digest", "seed", "rank", "world",
           "ncycle", "sections", "time", "dt", "n_records", "chunk", "fp_auto_known", "fp_auto_exact", "user_bytes",
           "user_digest", "header_digest")
assert _HEADER.size == HEADER_BYTES

_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_S30, _S27, _S31 = np.uint64(30), np.uint64(27), np.uint64(31)


def mix(z: np.ndarray) -> np.ndarray:
    """SplitMix64's finaliser on an array of u64 (mod 2^64)."""
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> _S30)) * _M1
    z = (z ^ (z >> _S27)) * _M2
    return z ^ (z >> _S31)


def hashes(words, g0: int = 0) -> np.ndarray:
    """The hash of every group of 8 words (a census record; 8 words of a
    table, the last group zero-padded), group g0 first."""
    w = np.ascontiguousarray(words, np.uint64).reshape(-1)
    pad = (-w.size) % 8
    if pad:
        w = np.concatenate([w, np.zeros(pad, np.uint64)])
    w = w.reshape(-1, 8)
    a = mix(np.arange(len(w), dtype=np.uint64) + np.uint64(g0) + GOLDEN)
    for k in range(8):
        a = mix(a ^ w[:, k])
    return a


def digest(words, g0: int = 0):
    """(sum, xor) mod 2^64 of the group hashes: a chunk's or a table's digest."""
    h = hashes(words, g0)
    if h.size == 0:
        return 0, 0
    return int(np.add.reduce(h, dtype=np.uint64)), int(np.bitwise_xor.reduce(h))


def fold(n_records: int, chunk_digests: Iterable) -> int:
    """The trailer's digest over the chunks' (sum, xor), in order."""
    t = mix(np.array([n_records], np.uint64) + GOLDEN)
    for s, x in chunk_digests:
        t = mix(mix(t ^ np.uint64(s)) ^ np.uint64(x))
    return int(t[0])


def grid_digest(grid: abi.GridConfig) -> int:
    """The header's digest of the grids a census record depends on."""
    w = np.concatenate([np.asarray(grid.z, np.float64).reshape(-1), np.asarray(grid.r, np.float64).reshape(-1),
                        np.array([grid.rmin, grid.zmin], np.float64), np.asarray(grid.E_ph, np.float64).reshape(-1),
                        np.asarray(grid.E_field, np.float64).reshape(-1)])
    return digest(w.view(np.uint64))[0]


def _pad8(n: int) -> int:
    return (n + 7) & ~7


def pack_header(h: dict) -> bytes:
    """The 128 header bytes of the fields of h (its digest computed here)."""
    vals = [h[k] for k in _FIELDS[:-1]]
    raw = _HEADER.pack(*vals, 0)
    hd = digest(np.frombuffer(raw, np.uint64)[:15])[0]
    return _HEADER.pack(*vals, hd)


def parse_header(raw: bytes) -> dict:
    """The header's fields; ValueError says why the bytes are not one."""
    if len(raw) < HEADER_BYTES:
        raise ValueError("shorter than a header")
    h = dict(zip(_FIELDS, _HEADER.unpack(raw[:HEADER_BYTES])))
    if h["magic"] != MAGIC:
        raise ValueError("not a checkpoint (magic)")
    if h["version"] != abi.CKPT_VERSION or h["header_bytes"] != HEADER_BYTES:
        raise ValueError("another format version")
    if h["header_digest"] != digest(np.frombuffer(raw[:HEADER_BYTES], np.uint64)[:15])[0]:
        raise ValueError("the header's digest does not match")
    return h


def table_words(h: dict) -> list:
    """(name, f64 words) of the table sections the header announces, in file order."""
    nc = h["nz"] * h["nr"]
    out = []
    if h["sections"] & abi.CKPT_HAS_KAPPA:
        out.append(("kappa_prev", nc * abi.N_VOL))
    if h["sections"] & abi.CKPT_HAS_ELECTRONS:
        out += [("f_nt", nc * abi.NUM_NT), ("Pnt", nc * abi.NUM_NT)]
    return out


def n_chunks(h: dict) -> int:
    return (h["n_records"] + h["chunk"] - 1) // h["chunk"] if h["n_records"] > 0 else 0


def chunk_offset(h: dict, k: int) -> int:
    """Byte offset of census chunk k."""
    off = HEADER_BYTES + _pad8(h["user_bytes"])
    for _, words in table_words(h):
        off += HEAD_BYTES + 8 * words
    return off + k * (HEAD_BYTES + 8 * REC_WORDS * h["chunk"])


def file_bytes(h: dict) -> int:
    return chunk_offset(h, 0) + n_chunks(h) * HEAD_BYTES + 8 * REC_WORDS * h["n_records"] + TRAILER_BYTES


def read_header(path) -> dict:
    """The header of `path`, checked against its digest."""
    with open(path, "rb") as f:
        return parse_header(f.read(HEADER_BYTES))


def read_user(path) -> bytes:
    h = read_header(path)
    with open(path, "rb") as f:
        f.seek(HEADER_BYTES)
        return f.read(h["user_bytes"])


def read_tables(path) -> dict:
    """The table sections of `path` as f64 arrays, each checked against its digest."""
    h = read_header(path)
    out = {}
    off = HEADER_BYTES + _pad8(h["user_bytes"])
    with open(path, "rb") as f:
        for name, words in table_words(h):
            f.seek(off)
            n, s, x = struct.unpack("<qQQ", f.read(HEAD_BYTES))
            w = np.frombuffer(f.read(8 * words), np.uint64)
            if n != words or w.size != words or digest(w) != (s, x):
                raise ValueError("table %s at offset %d fails its check" % (name, off))
            shape = (h["nz"], h["nr"], words // (h["nz"] * h["nr"]))
            out[name] = w.view(np.float64).reshape(shape).copy()
            off += HEAD_BYTES + 8 * words
    return out


def iter_chunks(path, verify: bool = True) -> Iterator[tuple]:
    """(k, byte offset, words [m, 8] u64, (sum, xor) of the file) for every
    census chunk; verify: the digest is recomputed and a chunk whose own
    differs raises ValueError, as do a short chunk and a trailer that
    disagrees with the header or with the chunks."""
    h = read_header(path)
    seen = []
    if verify and os.path.getsize(path) != file_bytes(h):
        raise ValueError("the file's size is not what its header says")
    with open(path, "rb") as f:
        for k in range(n_chunks(h)):
            off = chunk_offset(h, k)
            f.seek(off)
            head = f.read(HEAD_BYTES)
            if len(head) != HEAD_BYTES:
                raise ValueError("chunk %d at offset %d is truncated" % (k, off))
            m, s, x = struct.unpack("<qQQ", head)
            want = min(h["chunk"], h["n_records"] - k * h["chunk"])
            raw = f.read(8 * REC_WORDS * want)
            if m != want or len(raw) != 8 * REC_WORDS * want:
                raise ValueError("chunk %d at offset %d is truncated or of another count" % (k, off))
            w = np.frombuffer(raw, np.uint64).reshape(-1, REC_WORDS)
            if verify and digest(w, k * h["chunk"]) != (s, x):
                raise ValueError("chunk %d at offset %d fails its digest" % (k, off))
            seen.append((s, x))
            yield k, off, w, (s, x)
        if verify:
            f.seek(file_bytes(h) - TRAILER_BYTES)
            t = f.read(TRAILER_BYTES)
            if len(t) != TRAILER_BYTES or struct.unpack("<QqQ", t) != (TRAILER_MAGIC, h["n_records"],
                                                                     fold(h["n_records"], seen)):
                raise ValueError("the trailer disagrees with the header or the chunks")


def read_words(path) -> np.ndarray:
    """Every census record of `path`: [n, 8] u64, verified."""
    parts = [w for _, _, w, _ in iter_chunks(path)]
    return np.concatenate(parts) if parts else np.zeros((0, REC_WORDS), np.uint64)


def chunk_from_env() -> int:
    e = os.environ.get("C2D_CKPT_CHUNK", "")
    try:
        v = int(e)
    except ValueError:
        v = 0
    return min(v, 1 << 24) if v >= 1 else DEFAULT_CHUNK


def write_file(path, grid: abi.GridConfig, words, user: bytes = b"", kappa_prev=None, f_nt=None, Pnt=None,
               ncycle: int = 0, time: float = 0.0, dt: float = 0.0, fp_auto_known: bool = False,
               fp_auto_exact: bool = False, chunk: Optional[int] = None) -> None:
    """The bytes c2d_checkpoint_write writes for this state: `words` [n, 8]
    u64 are the census's packed records (Engine.census_pack) in census order,
    kappa_prev [nz, nr, 400] and f_nt / Pnt [nz, nr, 200] the tables (None:
    the section is absent), grid the context's configuration."""
    words = np.ascontiguousarray(words, np.uint64).reshape(-1, REC_WORDS)
    chunk = chunk_from_env() if chunk is None else int(chunk)
    user = bytes(user)
    blob = user + b"\0" * (_pad8(len(user)) - len(user))
    tables = []
    if kappa_prev is not None:
        tables.append(np.ascontiguousarray(kappa_prev, np.float64).reshape(-1))
    if f_nt is not None:
        tables += [np.ascontiguousarray(f_nt, np.float64).reshape(-1),
                   np.ascontiguousarray(Pnt, np.float64).reshape(-1)]
    h = dict(magic=MAGIC, version=abi.CKPT_VERSION, header_bytes=HEADER_BYTES, nz=grid.nz, nr=grid.nr,
             nmu=int(np.asarray(grid.mu).size), encoded=int(grid.comtot_mode == abi.COMTOT_TABLE),
             grid_digest=grid_digest(grid), seed=int(grid.seed), rank=int(grid.rank), world=int(grid.world),
             ncycle=int(ncycle),
             sections=(abi.CKPT_HAS_KAPPA if kappa_prev is not None else 0) |
                      (abi.CKPT_HAS_ELECTRONS if f_nt is not None else 0),
             time=float(time), dt=float(dt), n_records=len(words), chunk=chunk,
             fp_auto_known=int(bool(fp_auto_known)), fp_auto_exact=int(bool(fp_auto_exact)), user_bytes=len(user),
             user_digest=digest(np.frombuffer(blob, np.uint64))[0])
    tmp = os.fspath(path) + ".tmp"
    with open(tmp, "wb") as f:
        f.write(pack_header(h))
        f.write(blob)
        for t in tables:
            s, x = digest(t.view(np.uint64))
            f.write(struct.pack("<qQQ", t.size, s, x))
            f.write(t.tobytes())
        seen = []
        for c0 in range(0, len(words), chunk):
            w = words[c0:c0 + chunk]
            s, x = digest(w, c0)
            seen.append((s, x))
            f.write(struct.pack("<qQQ", len(w), s, x))
            f.write(w.tobytes())
        f.write(struct.pack("<QqQ", TRAILER_MAGIC, len(words), fold(len(words), seen)))
    os.replace(tmp, path)


def plan_shards(infos: Sequence, world: int) -> list:
    """Spread the census of an old run's shard files over `world` new ranks.
    infos: (file, header) pairs in the old ranks' order, header a dict with
    n_records (read_header's or engine.checkpoint_info's).  Returns, per new
    rank, the list of (file, first, count) to restore with
    Engine.checkpoint_read(file, first, count, append=...).  The records keep
    their order, no record is read twice, and the ranks' totals differ by at
    most one."""
    if world < 1:
        raise ValueError("world must be at least 1")
    sizes = [(f, int(h["n_records"])) for f, h in infos]
    total = sum(n for _, n in sizes)
    plan = []
    fi, used = 0, 0  # the file in work and its records already given away
    for r in range(world):
        need = total // world + (1 if r < total % world else 0)
        parts = []
        while need > 0:
            f, n = sizes[fi]
            take = min(need, n - used)
            if take > 0:
                parts.append((f, used, take))
                used += take
                need -= take
            if used == n:
                fi, used = fi + 1, 0
        plan.append(parts)
    return plan
