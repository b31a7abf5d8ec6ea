"""The Compton-reflection tables built on the host (c2d_reflect_tables_host,
csrc/reflect_host.h) against the plain restatement of src/ref_matrix.f in
tests/reflect_ref.py, and their structure.  Both sides call glibc's
pow/exp/log/sqrt in the same order, so they should agree to the last bits;
the P_ref / W_abs bound of 1e-12 is 500 summed terms at a few ulp each."""
import math

import numpy as np
import pytest

import reflect_ref as RR
from compton2d_amd import abi


@pytest.fixture(scope="module")
def host():
    return abi.reflect_tables_host()


@pytest.fixture(scope="module")
def ref():
    return RR.tables()


def test_tables_match_the_restatement(host, ref):
    E, P, W = host
    Er, Pr, Wr = ref
    assert E.shape == (500,) and P.shape == (500, 500) and W.shape == (500, 500)
    np.testing.assert_allclose(E, Er, rtol=1e-14, atol=0)
    np.testing.assert_allclose(P, Pr, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(W, Wr, rtol=1e-12, atol=1e-300)


def test_energy_grid(host):
    E = host[0]
    dE = math.exp(math.log(1.0e3) / 500.0)
    assert E[0] == 1.0
    assert abs(E[499] * dE - 1000.0) <= 1e-12 * 1000.0
    assert (np.diff(E) > 0).all()


def test_structure(host):
    E, P, W = host
    upper = np.triu(np.ones((500, 500), bool), k=1)          # n_out > n_in, layout [n_in][n_out]
    assert (P[upper] == 1.0).all()
    assert (W[upper] == 0.0).all()
    assert (np.diff(P, axis=1) >= 0).all()                   # non-decreasing in n_out
    assert (P[:, -1] == 1.0).all()
    assert (P[np.arange(500), np.arange(500)] == 1.0).all()  # the normalised running sum ends at 1
    low = np.nonzero(E <= 20.0)[0]
    assert len(low) > 0 and len(low) < 500
    for ni in low:                                           # the step at the diagonal
        assert (P[ni, :ni] == 0.0).all() and (P[ni, ni:] == 1.0).all()
        assert (W[ni, :ni + 1] == W[ni, 0]).all()            # one albedo per incoming energy
    assert (W >= 0.0).all() and (W <= 1.0).all()
    assert (P >= 0.0).all() and (P <= 1.0).all()
    # above 20 keV down-scattering spreads over many n_out and absorbs nothing at the diagonal
    hi = np.nonzero(E > 20.0)[0]
    assert (W[hi, hi] == 1.0).all()
    assert (P[hi[-1], :hi[-1]] > 0).all() and (P[hi[-1], :hi[-1]] < 1).all()


def test_tables_equal_the_references_own(host):
    """Against the reference's own Pref_calc / Wref_calc output
    (tests/golden/reflect_tables.npz, tests/golden/make_reflect_golden.py
    tables): E_ref whole, every 7th column and row of P_ref and W_abs, their
    diagonals and every column's sum, bit for bit."""
    import sys
    from pathlib import Path
    gold = Path(__file__).resolve().parent / "golden"
    sys.path.insert(0, str(gold))
    import make_reflect_golden as MG
    want = np.load(gold / "reflect_tables.npz", allow_pickle=False)
    got = MG.sample_tables(*host)
    assert set(got) == set(want.files)
    for k, v in got.items():
        np.testing.assert_array_equal(np.ascontiguousarray(v).view(np.uint64), want[k].view(np.uint64), err_msg=k)


def test_null_pointers_are_skipped():
    from compton2d_amd import engine
    lib = engine.load_library()
    E = np.zeros(500)
    assert lib.c2d_reflect_tables_host(E.ctypes.data_as(abi.PD), None, None) == 0
    assert E[0] == 1.0
