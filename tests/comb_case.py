"""Inputs shared by the census-comb tests (test_comb_host.py, test_gpu_comb.py):
a 3 x 2 grid with 4 spectral groups, normalisers with every special value the
rule names, records with every kind of `fixed`, the 4096-record log-normal
case of the unbiasedness test, and the policy on the CPU: comb_threshold fed
with histograms and collections made from the yardstick's values."""
import numpy as np

import roulette_case as RC
from compton2d_amd import abi, popcontrol as PC

NZ, NR, NG = 3, 2, 4
SIZES = (1, 63, 1025, 5 * 1024 + 17)      # shorter than a wave (2), a tile and a record, tiles and a tail
N_GRID3 = 70000                           # with C2D_COMB_GRID=3: 23 tiles a workgroup


def groups() -> np.ndarray:
    return RC.group_table(NG)


def norms(specials: bool = True, seed: int = 3) -> np.ndarray:
    """norm [NZ, NR, NG]: powers of two over four decades and (specials) one
    0, one inf and one NaN, whose records are fixed."""
    rng = np.random.default_rng(seed)
    nm = 2.0 ** rng.integers(-7, 8, (NZ, NR, NG)).astype(np.float64)
    if specials:
        flat = nm.reshape(-1)
        flat[1], flat[flat.size // 2], flat[flat.size // 2 + 1] = 0.0, np.inf, np.nan
    return nm


def records(n: int, nm=None, seed: int = 11, bad: bool = True):
    """(d6, i5, keys): roulette_case.synthetic_records with ew over six decades
    around the record's normaliser (ew == norm, ew = 0, jgpsp 0 and 255 among
    them) and, from 40 records on (bad), one each of ew < 0, NaN, +inf, -inf."""
    nm = norms() if nm is None else nm
    d6, i5, keys = RC.synthetic_records(n, NZ, NR, nm, groups(), seed)
    if bad and n >= 40:
        d6[20:24, 4] = (-1.0, np.nan, np.inf, -np.inf)
    return d6, i5, keys


def stats(d6, i5, g, ng, nz=NZ, nr=NR):
    """Engine.census_stats in numpy for records on the grid."""
    b = ((i5[:, 3].astype(np.int64) - 1) * nr + (i5[:, 4] - 1)) * ng + g[np.minimum(i5[:, 0], abi.NPHOMAX)]
    count = np.bincount(b, minlength=nz * nr * ng).reshape(nz, nr, ng)
    energy = np.bincount(b, weights=d6[:, 4], minlength=nz * nr * ng).reshape(nz, nr, ng)
    return count, energy


def lognormal_case(n: int = 4096, seed: int = 41):
    """The unbiasedness case: n records in 6 groups (the cells (1..3, 1), two
    spectral groups each) whose weights are log-normal, sigma 1.5 in ln,
    around a mean that differs from group to group.  Returns (d6, i5, keys,
    g, ng, bin): bin the record's (cell, group) number 0..5."""
    rng = np.random.default_rng(seed)
    g = RC.group_table(2)
    d6, i5, keys = RC.synthetic_records(n, NZ, NR, np.ones((NZ, NR, 2)), g, seed)
    i5[:, 4] = 1
    b = (i5[:, 3] - 1) * 2 + g[np.minimum(i5[:, 0], abi.NPHOMAX)]
    d6[:, 4] = 10.0 ** (b - 2.0) * np.exp(1.5 * rng.standard_normal(n))
    return d6, i5, keys, g, 2, b


def passes(parts):
    """hist_pass and collect_pass of popcontrol.comb_threshold over `parts`, a
    list of (crit, fixed) of the ranks' records: histograms and counts summed,
    values concatenated."""
    def hist_pass(prefix, pbits):
        hs = [PC.comb_hist_numpy(c, f, prefix, pbits) for c, f in parts]
        return sum(h for h, _ in hs), sum(k for _, k in hs), 0.0

    def collect_pass(prefix, pbits, bucket):
        return np.concatenate([c[~f][PC.comb_match(c[~f], prefix, pbits)] for c, f in parts])

    return hist_pass, collect_pass


def policy_cpu(d6, i5, keys, g, ng, target, salt, collect=True, shards=1, collect_cap=1 << 20, min_per_group=32):
    """popcontrol.comb_floor without an engine: (w_min, t, norm, crit, fixed, info)."""
    count, energy = stats(d6, i5, g, ng)
    norm = PC.comb_norm(count, energy, min_per_group)
    crit, fixed = PC.comb_critical(d6, i5, keys, NZ, NR, g, ng, norm, salt)
    hist_pass, collect_pass = passes([(crit[r::shards], fixed[r::shards]) for r in range(shards)])
    t, info = PC.comb_threshold(hist_pass, collect_pass if collect else None, target, collect_cap)
    return PC.comb_weights(t, norm), t, norm, crit, fixed, info
