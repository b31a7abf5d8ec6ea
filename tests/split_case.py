"""Inputs shared by the census-splitting tests (test_split_host.py,
test_gpu_split.py): ceilings with every special value the rule names, and an
ew for every record that spreads six decades around the record's own
ceiling and sits exactly on every edge of the rule."""
import numpy as np

import roulette_case as RC
from compton2d_amd import abi

group_table = RC.group_table


def ceilings(nz: int, nr: int, ngroup: int, seed: int = 6, specials: bool = True) -> np.ndarray:
    """w_max [nz, nr, ngroup]: powers of two and plain values over four decades,
    and (specials) one 0, one inf, one NaN and one negative ceiling."""
    return RC.floors(nz, nr, ngroup, seed=seed, specials=specials)


def record_ceilings(i5, nz: int, nr: int, w_max, group_of_sp) -> np.ndarray:
    i5 = np.asarray(i5, np.int64)
    ngroup = np.asarray(w_max).shape[-1]
    sp = np.minimum(i5[:, 0], abi.NPHOMAX)
    return np.asarray(w_max, np.float64).reshape(nz, nr, ngroup)[i5[:, 3] - 1, i5[:, 4] - 1,
                                                                np.asarray(group_of_sp)[sp]]


def spread_ew(i5, nz: int, nr: int, w_max, group_of_sp, seed: int = 13) -> np.ndarray:
    """An ew for every record: six decades around the record's own ceiling W
    (around 1 where the ceiling tests nothing); ew == W exactly every 16th
    record, ew = nextafter(W, inf) every 32nd, ew = 0 every 64th, and
    ew = 200 W (a quotient past 64) every 128th."""
    rng = np.random.default_rng(seed)
    n = len(i5)
    w = record_ceilings(i5, nz, nr, w_max, group_of_sp)
    ref = np.where(np.isfinite(w) & (w > 0), w, 1.0)
    ew = ref * 10.0 ** rng.uniform(-3.0, 3.0, n)
    ew[4::16] = ref[4::16]                              # ew == W exactly: untouched
    ew[9::32] = np.nextafter(ref[9::32], np.inf)        # one step above: m = 2
    ew[5::64] = 0.0                                     # ew = 0: untouched
    ew[2::128] = 200.0 * ref[2::128]                    # ew / W > 64: m = max_copies
    return ew


def synthetic_records(n: int, nz: int, nr: int, w_max, group_of_sp, seed: int = 11):
    """(d6, i5, keys): roulette_case's synthetic records with this module's ew."""
    d6, i5, keys = RC.synthetic_records(n, nz, nr, np.ones(np.asarray(w_max).shape), group_of_sp, seed)
    d6[:, 4] = spread_ew(i5, nz, nr, w_max, group_of_sp, seed + 2)
    return d6, i5, keys
