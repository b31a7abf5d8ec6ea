"""The kernels' reflection functions (csrc/c2d_reflect.hpp through
c2d_selftest_reflect) on 4096 packet states per boundary against the plain
IEEE restatement (tests/reflect_ref.py): values, idead, n_in, n_out and the
number of draws bit for bit; the Ed_ref adds to 1e-12 (their order is free)."""
import numpy as np
import pytest

import reflect_ref as RR
from compton2d_amd import engine

pytestmark = pytest.mark.gpu

N = 4096


def _states():
    rng = np.random.default_rng(20261020)
    E = RR.tables()[0]
    n5 = N // 5
    xnu = np.concatenate([
        10.0 ** rng.uniform(-6.0, 0.0, n5) * (1 - 1e-12),       # [1e-6, 1): below E_ref(1)
        rng.uniform(1.0, 20.0, n5) + 1e-9,                       # (1, 20]: the albedo columns
        10.0 ** rng.uniform(np.log10(20.0), 3.0, n5) + 1e-9,     # (20, 1000): the matrix
        10.0 ** rng.uniform(3.0, 6.0, n5) + 1.0,                 # > 1000: n_in capped
        E[rng.integers(0, 500, N - 4 * n5)],                     # exactly on grid points
    ])
    xnu[1] = 1.0e-6
    xnu[n5] = 20.0
    wmu = rng.uniform(-1.0, 1.0, N)
    k = np.arange(N)
    wmu[k % 16 == 3] = 0.0
    wmu[k % 16 == 5] = rng.uniform(-1.0e-6, 1.0e-6, (k % 16 == 5).sum())      # |wmu| below 1e-6
    wmu[k % 16 == 7] = -1.0e-6                                                 # not above it
    wmu[k % 16 == 9] = -rng.uniform(1.0e-6, 1.0e-5, (k % 16 == 9).sum())      # just above it
    st = np.zeros((N, 8))
    st[:, 0] = xnu
    st[:, 1] = 10.0 ** rng.uniform(30.0, 50.0, N)
    st[:, 2] = wmu
    st[:, 3] = rng.uniform(0.0, 7.5e15, N)
    st[:, 4] = rng.uniform(0.0, 1.0e16, N)
    st[:, 5] = rng.uniform(0.0, 2.0 * np.pi, N)
    st[:, 6] = rng.uniform(0.0, 3.0e17, N)
    st[:, 7] = np.where(k % 3 == 0, 0.0, np.where(k % 3 == 1, -1.0, 1.0e-3))   # tbbl <= 0 and > 0
    st = st[rng.permutation(N)]
    keys = rng.integers(0, 2 ** 63, N, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    return st, keys


@pytest.fixture(scope="module")
def states():
    return _states()


_ref_cache = {}


def _reference(boundary, cr_sent, states):
    if (boundary, cr_sent) not in _ref_cache:
        _ref_cache[(boundary, cr_sent)] = RR.reflect_many(boundary, cr_sent, *states)
    return _ref_cache[(boundary, cr_sent)]


@pytest.mark.parametrize("spec_switch", [0, 1])
@pytest.mark.parametrize("cr_sent", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("boundary", [0, 1])
def test_reflection_bitwise(boundary, cr_sent, spec_switch, states):
    st, keys = states
    out, ed = engine.device_reflect(boundary, cr_sent, spec_switch, st, keys)
    want, ed_want = _reference(boundary, cr_sent, states)
    assert out.shape == want.shape == (N, 10)
    bad = np.nonzero((out.view(np.uint64) != want.view(np.uint64)).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], st[bad[:3]], out[bad[:3]], want[bad[:3]])
    assert abs(ed - ed_want) <= 1e-12 * abs(ed_want)
    reflects_lower = boundary == 0 and cr_sent in (1, 3, 4)
    reflects_outer = boundary == 1 and cr_sent in (2, 3)
    matrix = (boundary == 0 and cr_sent in (1, 3)) or reflects_outer
    assert (ed_want > 0) == (boundary == 0 and cr_sent in (1, 3))
    # the states that must not reflect come back untouched
    if reflects_lower:
        still = np.zeros(N, bool)
    elif reflects_outer:
        still = st[:, 2] > 0.0
    else:
        still = np.ones(N, bool)
    assert (out[still][:, :5].view(np.uint64) == st[still][:, :5].view(np.uint64)).all()
    assert (out[still][:, 6:] == [0.0, 1.0, 0.0, 0.0]).all()
    moved = ~still
    if reflects_lower:
        assert (out[moved, 7] == 0.0).all()                    # lives on
        spec = (st[:, 7] <= 0.0) | (cr_sent == 4)
        assert (out[spec, 6] == 0).all() and (out[spec, 2].view(np.uint64) == (-st[spec, 2]).view(np.uint64)).all()
        assert (out[~spec, 2] >= 0).all()
    if reflects_outer:
        assert moved.any() and (out[moved, 7] == 1.0).all()
        big = moved & (np.abs(st[:, 2]) > 1.0e-6)
        assert (out[big, 4] == 0.0).all()                      # zpre = 0 before f
        small = moved & ~big
        assert small.any() and (out[small, 5] == 1.0e20).all() and (out[small, 4] == st[small, 4]).all()
        assert ((out[moved, 2] > 0) & (out[moved, 2] < 1)).all()
    if matrix:
        m = moved if reflects_outer else (st[:, 7] > 0.0)
        assert (out[m, 8] >= 1).all() and (out[m, 8] <= 500).all() and (out[m, 9] <= out[m, 8]).all()
        assert (out[m & (st[:, 0] > 1000.0), 8] == 500).all()  # n_in capped
        low = m & (st[:, 0] < 1.0)
        assert low.any() and (out[low, 0] == 1.0).all()        # below E_ref(1): leaves at exactly 1 keV
        draws = out[m, 6] - (1 if reflects_outer else 0)
        assert ((draws == 2) == (out[m, 9] > 1)).all() and ((draws == 1) == (out[m, 9] == 1)).all()
