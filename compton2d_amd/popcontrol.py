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

`weight_floor` only bounds the expected count.  The comb (csrc/c2d_comb.h,
DESIGN.md 4k) picks floors under which the same roulette pass leaves exactly
`target` records: `comb_critical` is the yardstick of a record's normalised
critical floor, `comb_threshold` the search for the (M + 1)-th largest of
them from digit histograms (Engine.census_comb_hist) and a final collection
(Engine.census_comb_collect), `comb_floor` the policy, and
CensusControl(exact=True) what switches CoupledRun to it.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np

from . import abi

M64 = 0xFFFFFFFFFFFFFFFF
_TINY = 5e-324
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


def derive_keys(keys, tag: int, a: int, b: int, sub=0) -> np.ndarray:
    """derive_int of every key, vectorised: c2d_derive_s(key, tag, a, b, sub),
    sub a scalar or one value a key (uint64 products of 32-bit words are
    exact)."""
    keys = np.ascontiguousarray(keys, np.uint64).reshape(-1)
    m32, s32 = np.uint64(M32), np.uint64(32)
    sub = np.broadcast_to(np.asarray(sub, np.uint64), keys.shape)
    c0 = np.full(keys.shape, int(a) & M32, np.uint64)
    c1 = np.full(keys.shape, int(b) & M32, np.uint64)
    c2 = (np.uint64(tag) | (sub << np.uint64(8))) & m32
    c3 = np.full(keys.shape, _DERIVE_C3, np.uint64)
    k0, k1 = keys & m32, keys >> s32
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c0, np.uint64(_PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(_PHILOX_W0)) & m32, (k1 + np.uint64(_PHILOX_W1)) & m32
    return (c1 << s32) | c0


def draw_keys(keys, n: int = 0, sub: int = 0) -> np.ndarray:
    """draw_int(key, n, sub) of every key, vectorised (64-bit products wrap as
    the C code's do)."""
    keys = np.ascontiguousarray(keys, np.uint64).reshape(-1)
    z = keys + np.uint64((_GAMMA * (((int(sub) << 32) | int(n)) + 1)) & M64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(_MIX1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(_MIX2)
    z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def roulette_u(keys, salt: int) -> np.ndarray:
    """roulette_u_int of every key, vectorised."""
    salt = int(salt) & M64
    return draw_keys(derive_keys(keys, abi.TAG_ROULETTE, salt & M32, salt >> 32), 0)


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


# ---- census splitting: the upper weight window (csrc/c2d_split.h) -------------
# A record heavier than its ceiling W = w_max[jph-1, kph-1, g] becomes
# m = min(max_copies, ceil(ew / W)) records of weight ew / m: copy 0 is the
# record itself, copy i = 1..m-1 equals it but for its key,
# derive(key, TAG_SPLIT, salt lo, salt hi; sub i).  Untouched (m = 1):
# !(W > 0), W or ew not finite, !(ew > W).
def split_copies(ew, W, max_copies: int) -> Tuple[np.ndarray, np.ndarray]:
    """(m int32 [n], ew' f64 [n]) of records of weight ew under the ceilings W."""
    if not 2 <= int(max_copies) <= abi.SPLIT_COPIES_MAX:
        raise ValueError("max_copies %d outside 2..%d" % (max_copies, abi.SPLIT_COPIES_MAX))
    ew = np.ascontiguousarray(ew, np.float64).reshape(-1)
    W = np.ascontiguousarray(W, np.float64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = (W > 0) & np.isfinite(W) & np.isfinite(ew) & (ew > W)
        q = ew[t] / W[t]                                   # one IEEE division
        mt = np.where(~(q < max_copies), float(max_copies), np.ceil(np.where(np.isfinite(q), q, 0.0)))
    m = np.ones(len(ew), np.int32)
    m[t] = mt.astype(np.int32)
    out = ew.copy()
    out[t] = ew[t] / m[t].astype(np.float64)               # one IEEE division
    return m, out


def split_keys(keys, copies, salt: int) -> np.ndarray:
    """The keys of the copies i = 1..copies[k]-1 of every record k, ordered by (k, i)."""
    keys = np.ascontiguousarray(keys, np.uint64).reshape(-1)
    extra = np.asarray(copies, np.int64).reshape(-1) - 1
    src = np.repeat(np.arange(len(keys)), extra)
    i = np.arange(len(src)) - np.repeat(np.cumsum(extra) - extra, extra) + 1
    salt = int(salt) & M64
    return derive_keys(keys[src], abi.TAG_SPLIT, salt & M32, salt >> 32, i.astype(np.uint64))


def split_numpy(d6, i5, keys, nz: int, nr: int, group_of_sp, ngroup: int, w_max, max_copies: int, salt: int):
    """The yardstick of c2d_census_split on n records in the layout of
    Engine.census(): (copies int32 [n], ew_out f64 [n], (d6, i5, keys)), the
    last the whole census afterwards in the order the pass guarantees: the n
    records in place with their new ew, the copies behind them ordered by
    (source record, i)."""
    d6 = np.asarray(d6, np.float64).reshape(-1, 6)
    i5 = np.asarray(i5).reshape(-1, 5)
    keys = np.asarray(keys, np.uint64).reshape(-1)
    W = record_floors(i5, nz, nr, group_of_sp, ngroup, w_max)
    m, ew_out = split_copies(d6[:, 4], W, max_copies)
    src = np.repeat(np.arange(len(keys)), m.astype(np.int64) - 1)
    d6o = np.concatenate([d6, d6[src]])
    d6o[:len(keys), 4] = ew_out
    d6o[len(keys):, 4] = ew_out[src]
    return m, ew_out, (d6o, np.concatenate([i5, i5[src]]), np.concatenate([keys, split_keys(keys, m, salt)]))


def split_host(d6, i5, keys, nz: int, nr: int, group_of_sp, ngroup: int, w_max, max_copies: int, salt: int):
    """(copies, ew_out, copy keys) through the library's host twins
    (c2d_census_split_host, c2d_census_split_keys_host; no GPU)."""
    from . import engine
    lib = engine.load_library()
    d6 = np.ascontiguousarray(d6, np.float64).reshape(-1, 6)
    i5 = np.ascontiguousarray(i5, np.int32).reshape(-1, 5)
    keys = np.ascontiguousarray(keys, np.uint64).reshape(-1)
    g = np.ascontiguousarray(group_of_sp, np.int32).reshape(-1)
    w = np.ascontiguousarray(w_max, np.float64)
    n = len(keys)
    if g.size != abi.ROULETTE_NSP or (w.size != int(nz) * int(nr) * int(ngroup)
                                      and 1 <= int(ngroup) <= abi.ROULETTE_GROUPS_MAX):
        raise ValueError("group_of_sp of %d entries, w_max of %d" % (g.size, w.size))
    m, out = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1))
    rc = lib.c2d_census_split_host(d6.ctypes.data, i5.ctypes.data, keys.ctypes.data, n, int(nz), int(nr),
                                   g.ctypes.data, int(ngroup), w.ctypes.data, int(max_copies), int(salt) & M64,
                                   m.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise engine.C2DError(rc, "c2d_census_split_host rejected its arguments")
    m, out = m[:n], out[:n]
    ck = np.zeros(max(int((m.astype(np.int64) - 1).sum()), 1), np.uint64)
    rc = lib.c2d_census_split_keys_host(keys.ctypes.data, m.ctypes.data, n, int(salt) & M64, ck.ctypes.data)
    if rc != 0:
        raise engine.C2DError(rc, "c2d_census_split_keys_host rejected its arguments")
    return m, out, ck[:int((m.astype(np.int64) - 1).sum())]


def weight_ceiling(count, energy, ratio: float, min_per_group: int = 32) -> np.ndarray:
    """The default ceilings from the census statistics (summed over ranks):
    `ratio` times a (cell, group)'s mean weight, rounded up to a power of two
    (so last-bit noise of the f64 sums changes no decision), where the group
    holds at least min_per_group records; 0, no ceiling, for the sparse
    groups, whose mean says little."""
    if not ratio > 1:
        raise ValueError("weight_ceiling: ratio must exceed 1")
    count = np.asarray(count, np.int64)
    energy = np.asarray(energy, np.float64)
    w = np.zeros(count.shape, np.float64)
    dense = (count >= max(int(min_per_group), 1)) & (energy > 0) & np.isfinite(energy)
    with np.errstate(over="ignore"):
        raw = float(ratio) * energy[dense] / count[dense]
    ok = np.isfinite(raw) & (raw > 0)
    cl = np.zeros(raw.shape)
    cl[ok] = pow2_ceil(raw[ok])
    w[dense] = np.where(np.isfinite(cl), cl, 0.0)
    return w


def multiply_tables(nz: int, nr: int) -> Tuple[np.ndarray, int, np.ndarray]:
    """(group_of_sp, ngroup, w_max) under which every record of positive finite
    weight is split max_copies-fold: one group, the smallest double as every
    ceiling (a subnormal weight of j steps of 5e-324, j < max_copies, becomes
    j records: it cannot be divided further)."""
    return np.zeros(abi.ROULETTE_NSP, np.int32), 1, np.full((nz, nr, 1), _TINY)


def multiply(eng, k: int, salt: int) -> dict:
    """k-fold multiplication of `eng`'s census: every record of positive finite
    weight becomes k records of weight ew / k on independent streams
    (Engine.census_split's dict)."""
    g, ng, w = multiply_tables(eng.nz, eng.nr)
    return eng.census_split(g, ng, w, int(k), salt)


# ---- the census comb: floors that leave exactly `target` records -------------
# csrc/c2d_comb.h restated.  Under the roulette a tested record survives the
# floor w iff S(w) := u < ew / w; its critical floor w* is the largest finite
# double with S(w*), and it stays iff w <= w*.  With floors t * norm (norm a
# power of two per (cell, group)) the normalised critical value c = w* / norm
# is the record's priority (Duffield, Lund & Thorup 2007): the floors keep
# exactly the records with c >= t, so t one step above the (M+1)-th largest c
# keeps M of them, and E[ew'] = ew still holds record by record.
_DBL_MAX_BITS = np.uint64(0x7FEFFFFFFFFFFFFF)


def _survives(ew, u, w) -> np.ndarray:
    with np.errstate(divide="ignore", over="ignore", under="ignore", invalid="ignore"):
        return u < ew / w


def comb_wstar(ew, u) -> np.ndarray:
    """w* of records of weight ew >= 0 (finite) whose roulette draws are u:
    start at ew / u (an infinite quotient taken as DBL_MAX), at most
    abi.COMB_STEPS single steps down while S fails, then up while S holds one
    step above (c2d_comb_wstar)."""
    ew = np.ascontiguousarray(ew, np.float64).reshape(-1)
    u = np.ascontiguousarray(u, np.float64).reshape(-1)
    with np.errstate(divide="ignore", over="ignore", under="ignore", invalid="ignore"):
        w = np.minimum((ew / u).view(np.uint64), _DBL_MAX_BITS).view(np.float64)
    for _ in range(abi.COMB_STEPS):
        down = (w > 0) & ~_survives(ew, u, w)
        if not down.any():
            break
        w[down] = np.nextafter(w[down], -np.inf)
    for _ in range(abi.COMB_STEPS):
        with np.errstate(over="ignore"):                   # the step above DBL_MAX is +inf: S fails there
            above = np.nextafter(w, np.inf)
        up = _survives(ew, u, above)
        if not up.any():
            break
        w[up] = above[up]
    return np.where(ew == 0, 0.0, w)


def is_pow2(x) -> np.ndarray:
    """x positive, finite and a power of two."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return (x > 0) & np.isfinite(x) & (np.frexp(np.where(np.isfinite(x), x, 0.0))[0] == 0.5)


def _comb_tables(group_of_sp, ngroup: int, norm, nz: int, nr: int):
    g = np.asarray(group_of_sp, np.int64).reshape(-1)
    if g.size != abi.ROULETTE_NSP or not 1 <= ngroup <= abi.ROULETTE_GROUPS_MAX:
        raise ValueError("group_of_sp of %d entries, ngroup %d" % (g.size, ngroup))
    if g.min() < 0 or g.max() >= ngroup:
        raise ValueError("a group id outside 0..%d" % (ngroup - 1))
    nm = np.asarray(norm, np.float64).reshape(nz, nr, ngroup)
    with np.errstate(invalid="ignore"):
        bad = (nm > 0) & np.isfinite(nm) & ~is_pow2(nm)
    if bad.any():
        raise ValueError("a norm that is not a power of two: %r" % float(nm[bad][0]))
    return g, nm


def comb_critical(d6, i5, keys, nz: int, nr: int, group_of_sp, ngroup: int, norm,
                  salt: int) -> Tuple[np.ndarray, np.ndarray]:
    """The yardstick of c2d_comb.h on n records in the layout of
    Engine.census(): (crit f64 [n], fixed bool [n]).  crit is the normalised
    critical value c = w* / norm of a pool record and 0 for a fixed one: no
    floor t * norm removes a record with !(norm > 0), norm not finite,
    !(ew >= 0), ew not finite or a cell off the grid."""
    d6 = np.asarray(d6, np.float64).reshape(-1, 6)
    i5 = np.asarray(i5, np.int64).reshape(-1, 5)
    keys = np.asarray(keys, np.uint64).reshape(-1)
    g, nm = _comb_tables(group_of_sp, ngroup, norm, nz, nr)
    if len(i5) and (i5[:, 0].min() < 0 or i5[:, 0].max() > 255):
        raise ValueError("a record's jgpsp is outside 0..255")
    ew = d6[:, 4]
    j, k = i5[:, 3], i5[:, 4]
    on = (j >= 1) & (j <= nz) & (k >= 1) & (k <= nr)
    rec_norm = np.where(on, nm[np.clip(j, 1, nz) - 1, np.clip(k, 1, nr) - 1, g[np.minimum(i5[:, 0], abi.NPHOMAX)]],
                        0.0)
    with np.errstate(invalid="ignore"):
        fixed = ~on | ~(rec_norm > 0) | ~np.isfinite(rec_norm) | ~(ew >= 0) | ~np.isfinite(ew)
    crit = np.zeros(len(ew))
    p = ~fixed
    if p.any():
        with np.errstate(over="ignore", under="ignore"):
            crit[p] = comb_wstar(ew[p], roulette_u(keys[p], salt)) / rec_norm[p]
    return crit, fixed


def comb_critical_host(d6, i5, keys, nz: int, nr: int, group_of_sp, ngroup: int, norm, salt: int):
    """The same through the library's host twin (c2d_census_comb_host; no GPU)."""
    from . import engine
    lib = engine.load_library()
    d6 = np.ascontiguousarray(d6, np.float64).reshape(-1, 6)
    i5 = np.ascontiguousarray(i5, np.int32).reshape(-1, 5)
    keys = np.ascontiguousarray(keys, np.uint64).reshape(-1)
    g = np.ascontiguousarray(group_of_sp, np.int32).reshape(-1)
    nm = np.ascontiguousarray(norm, np.float64)
    n = len(keys)
    if g.size != abi.ROULETTE_NSP or nm.size != int(nz) * int(nr) * int(ngroup):
        raise ValueError("group_of_sp of %d entries, norm of %d" % (g.size, nm.size))
    crit, fixed = np.zeros(max(n, 1)), np.zeros(max(n, 1), np.uint8)
    rc = lib.c2d_census_comb_host(d6.ctypes.data, i5.ctypes.data, keys.ctypes.data, n, int(nz), int(nr),
                                  g.ctypes.data, int(ngroup), nm.ctypes.data, int(salt) & M64,
                                  crit.ctypes.data, fixed.ctypes.data)
    if rc != 0:
        raise engine.C2DError(rc, "c2d_census_comb_host rejected its arguments")
    return crit[:n], fixed[:n].astype(bool)


def _comb_prefix_check(prefix: int, prefix_bits: int) -> None:
    if prefix_bits not in abi.COMB_PREFIX_BITS or prefix < 0 or prefix >> prefix_bits:
        raise ValueError("prefix %#x of %d bits: 0, 11, 22, 33, 44 or 55 bits, none above them" % (prefix, prefix_bits))


def comb_match(crit, prefix: int, prefix_bits: int) -> np.ndarray:
    """The values whose top prefix_bits bits are `prefix`."""
    _comb_prefix_check(prefix, prefix_bits)
    b = np.ascontiguousarray(crit, np.float64).view(np.uint64)
    if prefix_bits == 0:
        return np.ones(b.shape, bool)
    return (b >> np.uint64(64 - prefix_bits)) == np.uint64(prefix)


def comb_hist_numpy(crit, fixed, prefix: int = 0, prefix_bits: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """What c2d_census_comb_hist returns for records with these (crit, fixed):
    (hist int64 [2048] of the digit below the prefix, counts int64 [4] =
    n_records, n_fixed, n_pool, n_match)."""
    crit = np.ascontiguousarray(crit, np.float64).reshape(-1)
    fixed = np.asarray(fixed, bool).reshape(-1)
    pool = crit[~fixed]
    b = pool[comb_match(pool, prefix, prefix_bits)].view(np.uint64)
    if prefix_bits == abi.COMB_PREFIX_BITS[-1]:
        digit = b & np.uint64(0x1FF)
    else:
        digit = (b >> np.uint64(64 - 11 - prefix_bits)) & np.uint64(0x7FF)
    hist = np.bincount(digit.astype(np.int64), minlength=abi.COMB_BINS).astype(np.int64)
    return hist, np.array([len(crit), int(fixed.sum()), len(pool), len(b)], np.int64)


def comb_norm(count, energy, min_per_group: int = 32) -> np.ndarray:
    """The comb's normalisers: a (cell, group)'s mean weight rounded up to a
    power of two where it holds at least min_per_group records, 0 (its records
    are fixed) for the sparse ones: weight_floor's groups and protection."""
    count = np.asarray(count, np.int64)
    energy = np.asarray(energy, np.float64)
    norm = np.zeros(count.shape, np.float64)
    dense = (count >= max(int(min_per_group), 1)) & (energy > 0) & np.isfinite(energy)
    raw = energy[dense] / count[dense]
    ok = np.isfinite(raw) & (raw > 0)
    nm = np.zeros(raw.shape)
    nm[ok] = pow2_ceil(raw[ok])
    norm[dense] = np.where(np.isfinite(nm), nm, 0.0)
    return norm


def comb_threshold(hist_pass: Callable, collect_pass: Optional[Callable], target: int,
                   collect_cap: int = 1 << 20) -> Tuple[Optional[float], dict]:
    """The comb's t: one step above the (M + 1)-th largest normalised critical
    value, M = target - n_fixed, by a most-significant-digit search.

    hist_pass(prefix, prefix_bits) -> (hist, counts, ms), as comb_hist_numpy
    gives them, summed over ranks; collect_pass(prefix, prefix_bits, bucket)
    -> the bucket's values of all ranks, or None: then every digit is found
    by histogram.  The search collects as soon as its bucket holds at most
    collect_cap values, and finishes with numpy's partition.  Returns
    (None, info) when the pool is no larger than M (no floor is needed), and
    raises ValueError for M < 1.  info: passes, collected, comb_ms, n_fixed,
    n_pool, quota."""
    if target <= 0:
        raise ValueError("comb_threshold: target must be positive")
    info = dict(passes=0, collected=0, comb_ms=0.0, n_fixed=0, n_pool=0, quota=0)
    prefix, pbits, k = 0, 0, 0
    while True:
        hist, counts, ms = hist_pass(prefix, pbits)
        hist = np.asarray(hist, np.int64)
        info["passes"] += 1
        info["comb_ms"] += float(ms)
        if pbits == 0:
            n_fixed, n_pool = int(counts[1]), int(counts[2])
            quota = int(target) - n_fixed
            info.update(n_fixed=n_fixed, n_pool=n_pool, quota=quota)
            if quota >= n_pool:
                return None, info
            if quota < 1:
                raise ValueError("comb: target %d is below what the %d protected records alone hold"
                                 % (target, n_fixed))
            k = quota + 1                                   # the rank sought, from the top
        if int(hist.sum()) != int(counts[3]) or k > int(counts[3]):
            raise RuntimeError("comb: a histogram of %d values, %d matching, rank %d"
                               % (int(hist.sum()), int(counts[3]), k))
        above = np.cumsum(hist[::-1])                       # values in the top 1, 2, ... bins
        i = int(np.searchsorted(above, k, side="left"))
        d = abi.COMB_BINS - 1 - i
        k -= int(above[i] - hist[d])
        bucket = int(hist[d])
        width = 9 if pbits == abi.COMB_PREFIX_BITS[-1] else 11
        prefix, pbits = (prefix << width) | d, pbits + width
        if pbits == 64:
            cbits = np.uint64(prefix)
            break
        if collect_pass is not None and bucket <= collect_cap:
            vals = np.ascontiguousarray(collect_pass(prefix, pbits, bucket), np.float64)
            if len(vals) != bucket:
                raise RuntimeError("comb: %d values collected of a bucket of %d" % (len(vals), bucket))
            cbits = np.partition(vals.view(np.uint64), bucket - k)[bucket - k]
            info["collected"] = bucket
            break
    return float(np.nextafter(np.array(cbits, np.uint64).view(np.float64), np.inf)), info


def comb_weights(t: Optional[float], norm) -> np.ndarray:
    """The floors t * norm (exact: norm is a power of two), 0 where norm is;
    all 0 for t = None.  A product that underflows to 0 is taken as the
    smallest double, which still removes the records of weight 0 and no other."""
    norm = np.asarray(norm, np.float64)
    if t is None:
        return np.zeros(norm.shape)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        live = (norm > 0) & np.isfinite(norm)
        return np.where(live, np.maximum(t * np.where(live, norm, 1.0), _TINY), 0.0)


def comb_floor(eng, groups: Tuple[np.ndarray, int], count, energy, target: int, salt: int,
               min_per_group: int = 32, collect_cap: int = 1 << 20, hist_allreduce: Optional[Callable] = None,
               gather: Optional[Callable] = None) -> Tuple[np.ndarray, dict]:
    """Floors under which Engine.census_roulette(group_of_sp, ngroup, w_min,
    salt), with the same salt, leaves exactly `target` records (summed over
    ranks): (w_min [nz, nr, ngroup], info).

    count, energy: Engine.census_stats (summed over ranks); the normalisers
    are comb_norm's.  hist_allreduce: callable(hist, counts) -> (hist, counts)
    summed over the ranks after every histogram pass; gather: callable(values)
    -> the values of all ranks.  With hist_allreduce and no gather all six
    digits are found by histogram.  `Exactly`: fewer than target only where
    several records share the (M + 1)-th largest value (duplicated keys)."""
    g, ng = groups
    norm = comb_norm(count, energy, min_per_group)

    def hist_pass(prefix, pbits):
        hist, out = eng.census_comb_hist(g, ng, norm, salt, prefix, pbits)
        counts = np.array([out["n_records"], out["n_fixed"], out["n_pool"], out["n_match"]], np.int64)
        if hist_allreduce is not None:
            hist, counts = hist_allreduce(hist, counts)
        return hist, counts, out["kernel_ms"]

    def collect_pass(prefix, pbits, bucket):
        vals, n = eng.census_comb_collect(g, ng, norm, salt, prefix, pbits, bucket)
        if n > bucket:
            raise RuntimeError("comb: %d values under a prefix the histogram counted %d for" % (n, bucket))
        return gather(vals) if gather is not None else vals

    use_collect = hist_allreduce is None or gather is not None
    t, info = comb_threshold(hist_pass, collect_pass if use_collect else None, target, collect_cap)
    info["t"] = t
    return comb_weights(t, norm), info


@dataclass
class CensusControl:
    """What CoupledRun(census_control=...) takes.

    target: the census size (summed over ranks) to come back to; the pass runs
    when the count exceeds target * (1 + slack).  groups: (group_of_sp,
    ngroup), default groups_by_decade of the run's spectral grid.
    stats_allreduce: callable(count, energy) -> (count, energy) summed over
    the ranks of a multi-GPU run, so every rank applies the same floors and
    a record's fate does not depend on the sharding.  exact: the floors are
    comb_floor's, which leave exactly `target` records, instead of
    weight_floor's, which bound the expected count; a multi-GPU run then also
    gives hist_allreduce and, to shorten the search, gather (comb_floor).  A
    target below what the protected (sparse-group) records alone hold is a
    ValueError there.

    ceiling_ratio: with a value (> 1) the upper window acts as well: after the
    roulette decision, records heavier than ceiling_ratio times their (cell,
    group)'s mean weight (weight_ceiling) are split into at most max_copies
    records, provided the census (summed over ranks) stays within
    target * (1 + slack); a split that would not is skipped.  None: no
    splitting, and nothing about the rows changes."""
    target: int
    slack: float = 0.25
    groups: Optional[Tuple[np.ndarray, int]] = None
    min_per_group: int = 32
    stats_allreduce: Optional[Callable] = None
    exact: bool = False
    hist_allreduce: Optional[Callable] = None
    gather: Optional[Callable] = None
    ceiling_ratio: Optional[float] = None
    max_copies: int = 8


def _roulette_control(eng, ctl: CensusControl, groups, salt: int, row: dict):
    """The lower window's decision; returns the (summed) statistics of the
    census as it now is, or None where they were not taken or no longer hold."""
    before = row["census_before"]
    limit = ctl.target * (1.0 + ctl.slack)
    if ctl.stats_allreduce is None and before <= limit:
        return None
    g, ng = groups
    count, energy = eng.census_stats(g, ng)
    if ctl.stats_allreduce is not None:
        count, energy = ctl.stats_allreduce(count, energy)
    if int(np.sum(count)) <= limit:
        return count, energy
    if ctl.exact:
        w_min, info = comb_floor(eng, groups, count, energy, ctl.target, salt, ctl.min_per_group,
                                 hist_allreduce=ctl.hist_allreduce, gather=ctl.gather)
        row.update(comb_ms=info["comb_ms"], comb_passes=info["passes"])
    else:
        w_min = weight_floor(count, energy, ctl.target, ctl.min_per_group)
    out = eng.census_roulette(g, ng, w_min, salt)
    row.update(census_after=out["n_after"], roulette_ms=out["kernel_ms"])
    return None


def _split_control(eng, ctl: CensusControl, groups, salt: int, row: dict, stats) -> None:
    """The upper window's decision: ceilings from the statistics, a dry run,
    and the split itself only if the census (summed over ranks) stays within
    target * (1 + slack)."""
    g, ng = groups
    if stats is None:
        stats = eng.census_stats(g, ng)
        if ctl.stats_allreduce is not None:
            stats = ctl.stats_allreduce(*stats)
    w_max = weight_ceiling(stats[0], stats[1], ctl.ceiling_ratio, ctl.min_per_group)
    dry = eng.census_split(g, ng, w_max, ctl.max_copies, salt, dry_run=True)
    row.update(split_copies=0, split_ms=dry["kernel_ms"], split_skipped=False)
    total, extra = dry["n_after"], dry["n_after"] - dry["n_before"]
    if ctl.stats_allreduce is not None:
        summed, _ = ctl.stats_allreduce(np.array([total, extra], np.int64), np.zeros(2))
        total, extra = int(summed[0]), int(summed[1])
    if extra == 0:
        return
    if total > ctl.target * (1.0 + ctl.slack):
        row["split_skipped"] = True
        return
    if dry["n_after"] > dry["n_before"]:
        out = eng.census_split(g, ng, w_max, ctl.max_copies, salt)
        row.update(census_after=out["n_after"], split_copies=out["n_after"] - out["n_before"],
                   split_ms=dry["kernel_ms"] + out["kernel_ms"])


def apply_control(eng, ctl: CensusControl, groups: Tuple[np.ndarray, int], salt: int) -> dict:
    """One population-control decision on `eng`'s census: census_before,
    census_after (this context's records) and roulette_ms (0 when the pass
    did not run); with ctl.exact also comb_ms and comb_passes, the device
    time and the histogram passes of comb_floor; with ctl.ceiling_ratio also
    split_copies (the records the split added here), split_ms (its device
    time, the dry run included) and split_skipped (the split would have left
    more than target * (1 + slack) records and was not made)."""
    before = eng.census_count()
    row = dict(census_before=before, census_after=before, roulette_ms=0.0)
    if ctl.exact:
        row.update(comb_ms=0.0, comb_passes=0)
        if ctl.stats_allreduce is not None and ctl.hist_allreduce is None:
            raise ValueError("CensusControl(exact=True) over several ranks needs hist_allreduce")
    stats = _roulette_control(eng, ctl, groups, salt, row)
    if ctl.ceiling_ratio is not None:
        _split_control(eng, ctl, groups, salt, row, stats)
    return row
