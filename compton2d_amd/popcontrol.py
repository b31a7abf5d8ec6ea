"""Census population control: the weight-window roulette and its default policy.

A long run's census grows until it fills the card: the reference stops at
ucens records a rank (src/imctrk2d.f:573-577), the engine returns
C2D_E_CENSUS_OVERFLOW.  Production Implicit Monte Carlo codes bound it by
rouletting census packets far lighter than their neighbours up to a floor
weight.  A packet's history does not depend on its weight and every tally is
linear in ew, so the expectation of every tally is unchanged; the user
trades census size for noise.

The rule (csrc/c2d_roulette.h; Engine.census_roulette runs it on the device,
c2d_census_roulette_host on the host).  For a record in cell (jph, kph) with
weight ew, spectral bin jgpsp and lineage key `key`, and the floor
w = w_min[jph-1, kph-1, group_of_sp[min(jgpsp, 128)]]:

    untouched   !(w > 0), w not finite, !(ew >= 0), or ew >= w
    otherwise   p = ew / w;  K = derive(key, TAG_ROULETTE, salt lo, salt hi)
                (Philox4x32-10);  u = draw 0 of K (SplitMix64);
                u < p: survives with ew = w exactly;  else removed

`roulette_numpy` is the yardstick of that rule, in the role census_io.py and
checkpoint.py play for their files: numpy uint64 arithmetic, with the
Python-integer `derive_int` / `draw_int` beside it as the plain restatement
of csrc/c2d_rng.h.  `weight_floor` is the default policy that turns
Engine.census_stats into floors, `groups_by_decade` the default spectral
grouping, `CensusControl` what CoupledRun takes.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np

from . import abi

M64 = 0xFFFFFFFFFFFFFFFF
M32 = 0xFFFFFFFF
_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_DERIVE_C3 = 0x9E3779B9
_GAMMA = 0x9E3779B97F4A7C15
_MIX1, _MIX2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


# ---- csrc/c2d_rng.h in Python integers ---------------------------------------
def derive_int(key: int, tag: int, a: int, b: int, sub: int = 0) -> int:
    """c2d_derive_s: the Philox4x32-10 key derivation."""
    c = [a & M32, b & M32, (tag | (sub << 8)) & M32, _DERIVE_C3]
    k0, k1 = key & M32, (key >> 32) & M32
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c[0], _PHILOX_M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + _PHILOX_W0) & M32, (k1 + _PHILOX_W1) & M32
    return (c[1] << 32) | c[0]


def mix64_int(z: int) -> int:
    z = ((z ^ (z >> 30)) * _MIX1) & M64
    z = ((z ^ (z >> 27)) * _MIX2) & M64
    return z ^ (z >> 31)


def draw_int(key: int, n: int, sub: int = 0) -> float:
    """c2d_draw_s: draw n of stream (key, sub), in (0, 1]."""
    x = mix64_int((key + _GAMMA * (((sub << 32) | n) + 1)) & M64)
    return (float(x >> 11) + 0.5) * 2.0 ** -53


def roulette_u_int(key: int, salt: int) -> float:
    """The uniform that decides the record with lineage key `key` under `salt`."""
    return draw_int(derive_int(key, abi.TAG_ROULETTE, salt & M32, (salt >> 32) & M32), 0)


# ---- the same on numpy uint64 arrays -----------------------------------------
def _u64(x) -> np.ndarray:
    return np.asarray(x, np.uint64)


def roulette_u(keys, salt: int) -> np.ndarray:
    """roulette_u_int of every key, vectorised (uint64 products of 32-bit
    words are exact; 64-bit products wrap as the C code's do)."""
    keys = np.ascontiguousarray(keys, np.uint64).reshape(-1)
    m32, s32 = np.uint64(M32), np.uint64(32)
    salt = int(salt) & M64
    c0 = np.full(keys.shape, salt & M32, np.uint64)
    c1 = np.full(keys.shape, salt >> 32, np.uint64)
    c2 = np.full(keys.shape, abi.TAG_ROULETTE, np.uint64)
    c3 = np.full(keys.shape, _DERIVE_C3, np.uint64)
    k0, k1 = keys & m32, keys >> s32
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c0, np.uint64(_PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(_PHILOX_W0)) & m32, (k1 + np.uint64(_PHILOX_W1)) & m32
    z = ((c1 << s32) | c0) + np.uint64(_GAMMA)            # stream (K, sub 0), draw 0
    z = (z ^ (z >> np.uint64(30))) * np.uint64(_MIX1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(_MIX2)
    z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def record_floors(i5, nz: int, nr: int, group_of_sp, ngroup: int, w_min) -> np.ndarray:
    """The floor w of every record: w_min[jph-1, kph-1, group_of_sp[min(jgpsp, 128)]]."""
    i5 = np.asarray(i5, np.int64).reshape(-1, 5)
    g = np.asarray(group_of_sp, np.int64).reshape(-1)
    if g.size != abi.ROULETTE_NSP or not 1 <= ngroup <= abi.ROULETTE_GROUPS_MAX:
        raise ValueError("group_of_sp of %d entries, ngroup %d" % (g.size, ngroup))
    if g.size and (g.min() < 0 or g.max() >= ngroup):
        raise ValueError("a group id outside 0..%d" % (ngroup - 1))
    w = np.asarray(w_min, np.float64).reshape(nz, nr, ngroup)
    if len(i5) and (i5[:, 3].min() < 1 or i5[:, 3].max() > nz or i5[:, 4].min() < 1 or i5[:, 4].max() > nr):
        raise ValueError("a record's cell is off the %d x %d grid" % (nz, nr))
    sp = np.minimum(i5[:, 0] & 0xFF, abi.NPHOMAX)
    return w[i5[:, 3] - 1, i5[:, 4] - 1, g[sp]]


def tested(ew, w) -> np.ndarray:
    """Records the floor tests at all (the rule's first line, negated)."""
    ew, w = np.asarray(ew, np.float64), np.asarray(w, np.float64)
    with np.errstate(invalid="ignore"):
        return (w > 0) & np.isfinite(w) & (ew >= 0) & ~(ew >= w)


def roulette_numpy(d6, i5, keys, nz: int, nr: int, group_of_sp, ngroup: int, w_min,
                   salt: int) -> Tuple[np.ndarray, np.ndarray]:
    """The rule on n records in the layout of Engine.census(): (keep bool [n],
    ew_out f64 [n]); ew_out is the floor for a survivor of a test and ew as
    given otherwise (removed records too)."""
    d6 = np.asarray(d6, np.float64).reshape(-1, 6)
    ew = d6[:, 4].copy()
    w = record_floors(i5, nz, nr, group_of_sp, ngroup, w_min)
    t = tested(ew, w)
    keep = np.ones(len(ew), bool)
    out = ew.copy()
    if t.any():
        p = ew[t] / w[t]                                   # one IEEE division
        u = roulette_u(np.asarray(keys, np.uint64).reshape(-1)[t], salt)
        s = u < p
        keep[t] = s
        out[t] = np.where(s, w[t], ew[t])
    return keep, out


def roulette_host(d6, i5, keys, nz: int, nr: int, group_of_sp, ngroup: int, w_min, salt: int):
    """The same through the library's host twin (c2d_census_roulette_host; no GPU)."""
    from . import engine
    lib = engine.load_library()
    d6 = np.ascontiguousarray(d6, np.float64).reshape(-1, 6)
    i5 = np.ascontiguousarray(i5, np.int32).reshape(-1, 5)
    keys = np.ascontiguousarray(keys, np.uint64).reshape(-1)
    g = np.ascontiguousarray(group_of_sp, np.int32).reshape(-1)
    w = np.ascontiguousarray(w_min, np.float64)
    n = len(keys)
    keep, out = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1))
    rc = lib.c2d_census_roulette_host(d6.ctypes.data, i5.ctypes.data, keys.ctypes.data, n, int(nz), int(nr),
                                      g.ctypes.data, int(ngroup), w.ctypes.data, int(salt) & M64,
                                      keep.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise engine.C2DError(rc, "c2d_census_roulette_host rejected its arguments")
    return keep[:n].astype(bool), out[:n]


# ---- the default policy ------------------------------------------------------
def groups_by_decade(hu) -> Tuple[np.ndarray, int]:
    """(group_of_sp int32 [129], ngroup): one group per decade of the spectral
    grid hu [nphtotal + 1] (bin j = 1..nphtotal spans hu[j-1]..hu[j] and goes
    by its lower edge), the decades past the 32nd folded into the last group.
    jgpsp = 0 (no spectral bin) shares group 0, bins past the grid the last
    bin's group."""
    hu = np.asarray(hu, np.float64).reshape(-1)
    nb = min(hu.size - 1, abi.NPHOMAX)
    if nb < 1 or not np.all(hu[:nb] > 0):
        raise ValueError("groups_by_decade: a spectral grid of positive edges")
    dec = np.floor(np.log10(hu[:nb]) + 1e-9).astype(np.int64)      # an edge meant as 10^k counts as 10^k
    dec = np.minimum(dec - dec[0], abi.ROULETTE_GROUPS_MAX - 1)
    dec = np.maximum.accumulate(np.maximum(dec, 0))
    g = np.zeros(abi.ROULETTE_NSP, np.int32)
    g[1:nb + 1] = dec
    g[nb + 1:] = dec[-1]
    return g, int(dec[-1]) + 1


def pow2_ceil(x) -> np.ndarray:
    """x > 0 rounded up to a power of two (exactly; x itself if it is one)."""
    m, e = np.frexp(np.asarray(x, np.float64))                    # x = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.where(m == 0.5, e - 1, e))


def weight_floor(count, energy, target: int, min_per_group: int = 32) -> np.ndarray:
    """The default floors from the census statistics (summed over ranks).

    N = count.sum().  At or below `target` every floor is 0.  Otherwise, with
    f = N / target, a (cell, group) of at least min_per_group records gets
    f * energy / count, f times its mean weight, rounded up to a power of two
    so that last-bit noise of the f64 sums does not change a decision; sparse
    groups, which hold the rare Compton tail, get 0 and are never touched.
    Hence E[n_after] <= target + (records in sparse groups), because
    sum min(1, ew/w) <= sum ew/w <= N / f."""
    count = np.asarray(count, np.int64)
    energy = np.asarray(energy, np.float64)
    w = np.zeros(count.shape, np.float64)
    n = int(count.sum())
    if target <= 0:
        raise ValueError("weight_floor: target must be positive")
    if n <= target:
        return w
    dense = (count >= max(int(min_per_group), 1)) & (energy > 0) & np.isfinite(energy)
    raw = (n / float(target)) * energy[dense] / count[dense]
    ok = np.isfinite(raw) & (raw > 0)
    fl = np.zeros(raw.shape)
    fl[ok] = pow2_ceil(raw[ok])
    w[dense] = np.where(np.isfinite(fl), fl, 0.0)
    return w


def expected_survivors(ew, w) -> float:
    """sum min(1, ew / w) over the records: E[n_after] of one pass."""
    ew, w = np.asarray(ew, np.float64), np.asarray(w, np.float64)
    t = tested(ew, w)
    return float((~t).sum() + (ew[t] / w[t]).sum())


@dataclass
class CensusControl:
    """What CoupledRun(census_control=...) takes.

    target: the census size (summed over ranks) to come back to; the pass runs
    when the count exceeds target * (1 + slack).  groups: (group_of_sp,
    ngroup), default groups_by_decade of the run's spectral grid.
    stats_allreduce: callable(count, energy) -> (count, energy) summed over
    the ranks of a multi-GPU run, so every rank applies the same floors and
    a record's fate does not depend on the sharding."""
    target: int
    slack: float = 0.25
    groups: Optional[Tuple[np.ndarray, int]] = None
    min_per_group: int = 32
    stats_allreduce: Optional[Callable] = None


def apply_control(eng, ctl: CensusControl, groups: Tuple[np.ndarray, int], salt: int) -> dict:
    """One population-control decision on `eng`'s census: census_before,
    census_after (this context's records) and roulette_ms (0 when the pass
    did not run)."""
    before = eng.census_count()
    row = dict(census_before=before, census_after=before, roulette_ms=0.0)
    limit = ctl.target * (1.0 + ctl.slack)
    if ctl.stats_allreduce is None and before <= limit:
        return row
    g, ng = groups
    count, energy = eng.census_stats(g, ng)
    if ctl.stats_allreduce is not None:
        count, energy = ctl.stats_allreduce(count, energy)
    if int(np.sum(count)) <= limit:
        return row
    out = eng.census_roulette(g, ng, weight_floor(count, energy, ctl.target, ctl.min_per_group), salt)
    row.update(census_after=out["n_after"], roulette_ms=out["kernel_ms"])
    return row
