"""Inputs shared by the census population-control tests (test_roulette_host.py,
test_gpu_roulette.py): synthetic census records in the layout of
Engine.census(), a spectral grouping and floors with every special value the
rule names."""
import numpy as np

from compton2d_amd import abi


def group_table(ngroup: int) -> np.ndarray:
    """group_of_sp [129]: bins dealt round-robin, so jgpsp 0, 128 and 255 (taken
    as 128) land in known groups whatever ngroup is."""
    return (np.arange(abi.ROULETTE_NSP) % ngroup).astype(np.int32)


def floors(nz: int, nr: int, ngroup: int, seed: int = 5, specials: bool = True) -> np.ndarray:
    """w_min [nz, nr, ngroup]: powers of two and plain values over four
    decades, and (specials) one 0, one inf, one NaN and one negative floor."""
    rng = np.random.default_rng(seed)
    w = 10.0 ** rng.uniform(-2.0, 2.0, (nz, nr, ngroup))
    w.reshape(-1)[::3] = 2.0 ** np.round(np.log2(w.reshape(-1)[::3]))
    if specials:
        flat = w.reshape(-1)
        n = flat.size
        flat[1 % n] = 0.0
        flat[(n // 2) % n] = np.inf
        flat[(n // 2 + 1) % n] = np.nan
        flat[(n - 1) % n] = -1.0
    return w


def spread_ew(i5, nz: int, nr: int, w_min, group_of_sp, seed: int = 12) -> np.ndarray:
    """An ew for every record: six decades around the record's own floor (around
    1 where the floor tests nothing), ew == w exactly every 16th record and
    ew = 0 every 64th."""
    rng = np.random.default_rng(seed)
    i5 = np.asarray(i5, np.int64)
    n = len(i5)
    ngroup = np.asarray(w_min).shape[-1]
    sp = np.minimum(i5[:, 0], abi.NPHOMAX)
    w = np.asarray(w_min, np.float64).reshape(nz, nr, ngroup)[i5[:, 3] - 1, i5[:, 4] - 1,
                                                             np.asarray(group_of_sp)[sp]]
    ref = np.where(np.isfinite(w) & (w > 0), w, 1.0)
    ew = ref * 10.0 ** rng.uniform(-3.0, 3.0, n)
    ew[4::16] = ref[4::16]             # ew == w exactly: untouched
    ew[5::64] = 0.0                    # ew = 0: removed wherever a floor tests it
    return ew


def synthetic_records(n: int, nz: int, nr: int, w_min, group_of_sp, seed: int = 11):
    """(d6, i5, keys): n records whose ew spreads over six decades around their
    own floor, with ew == w exactly, ew = 0, jgpsp = 0 and jgpsp = 255 among them."""
    rng = np.random.default_rng(seed)
    i5 = np.zeros((n, 5), np.int32)
    i5[:, 0] = rng.integers(0, 256, n)
    i5[:, 1] = rng.integers(0, 6, n)
    i5[:, 2] = 1
    i5[:, 3] = rng.integers(1, nz + 1, n)
    i5[:, 4] = rng.integers(1, nr + 1, n)
    if n >= 8:
        i5[0:2, 0] = 0
        i5[2:4, 0] = 255
    d6 = np.zeros((n, 6))
    d6[:, 0] = rng.uniform(0.1, 1.0, n)
    d6[:, 1] = rng.uniform(0.1, 1.0, n)
    d6[:, 2] = rng.uniform(-1.0, 1.0, n)
    d6[:, 3] = rng.uniform(0.1, 3.0, n)
    d6[:, 4] = spread_ew(i5, nz, nr, w_min, group_of_sp, seed + 1)
    d6[:, 5] = 10.0 ** rng.uniform(-6.0, 3.0, n)
    keys = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    return d6, i5, keys
