"""The exact observer accumulation on the host (c2d_obs_exact_host,
c2d_obs_state_merge, c2d_obs_state_result; compton2d_amd/csrc/c2d_obsacc.h,
c2d_obsacc_host.h) against a yardstick of Python integers.

Yardstick, per event: the bins are the non-zero count entries of the det
oracle on that event alone (oracle/c2d_obs_oracle.c); the boosted weight is
numpy's ew * (G * (1 + (-wmu) * sqrt(1 - 1/(G*G)))), every operation rounded
once, the doubles the f64 kernels add.  Per bin the integers are
sum(floor(w / 2^qF)) and sum(floor(fl(w*w) / 2^qF2)) in exact rational
arithmetic, e = E(w_max) + E(2 G), qF = e - 84, qF2 = 2e - 84.  The twin's
state must equal the yardstick's word for word, head and digests included
(the digests by compton2d_amd/checkpoint.py), and its doubles the integers
rounded by Fraction -> float (to nearest, ties to even)."""
import copy
from fractions import Fraction
from math import frexp
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as OL
from compton2d_amd import abi, checkpoint, observer
from compton2d_amd.engine import C2DError

G = np.load(Path(__file__).resolve().parent / "golden" / "obs.npz", allow_pickle=False)
DECKS = sorted(k[5:] for k in G.files if k.startswith("deck_"))
MASK = (1 << 64) - 1
_BINS = {}                 # (binning key, event bytes) -> flat bins of that event
_YARD = {}


def _binning(name):
    tool, deck = str(G["tool_" + name]), str(G["deck_" + name])
    return observer.parse_pspt_deck(deck) if tool == "pspt" else observer.parse_plcm_deck(deck)


def _event_bins(key, b, row):
    k = (key, row.tobytes())
    if k not in _BINS:
        _BINS[k] = np.flatnonzero(OL.obs_bin(b, row.reshape(1, 7), flavor="det")[2].reshape(-1))
    return _BINS[k]


def exponent(b, w_max):
    return frexp(w_max)[1] + frexp(2.0 * b.gam_bulk)[1]


def yardstick(key, b, w_max, ev):
    """(F, F2, count, n_rejected, exact sums of w) as Python integers / Fractions per flat bin."""
    e = exponent(b, w_max)
    qF, qF2 = Fraction(2) ** (e - 84), Fraction(2) ** (2 * e - 84)
    nh = b.n_t * b.n_mu * b.n_e
    F, F2, cnt, S = [0] * nh, [0] * nh, [0] * nh, [Fraction(0)] * nh
    rejected = 0
    Gm = np.float64(b.gam_bulk)
    betta = np.sqrt(np.float64(1.) - np.float64(1.) / (Gm * Gm))
    ev = np.ascontiguousarray(ev, np.float64).reshape(-1, 7)
    with np.errstate(all="ignore"):
        W = ev[:, 2] * (Gm * (np.float64(1.) + (-ev[:, 5]) * betta))
        WW = W * W
    lim = 2.0 ** e
    for i in range(len(ev)):
        bins = _event_bins(key, b, ev[i])
        if bins.size == 0:
            continue
        w = float(W[i])
        if not (w >= 0.0 and w < lim):
            rejected += 1
            continue
        a, a2 = int(Fraction(w) // qF), int(Fraction(float(WW[i])) // qF2)
        for h in bins:
            F[h] += a
            F2[h] += a2
            cnt[h] += 1
            S[h] += Fraction(w)
    return F, F2, cnt, rejected, S


def yard_state(b, w_max, y):
    """The yardstick's integers as the state's words."""
    F, F2, cnt, rejected, _ = y
    e = exponent(b, w_max)
    nh = len(F)
    words = []
    for h in range(nh):
        assert F[h] < 1 << 128 and F2[h] < 1 << 128
        words += [F[h] & MASK, F[h] >> 64, F2[h] & MASK, F2[h] >> 64, cnt[h]]
    pay = np.array(words, dtype=np.uint64)
    edges = np.concatenate([np.asarray(x, np.float64) for x in (b.t0, b.t1, b.mu0, b.mu1, b.E0, b.E1)])
    binw = np.concatenate([np.array([b.gam_bulk, b.rmax, b.t_offset], np.float64), edges]).view(np.uint64)
    head = np.array([abi.OBS_STATE_MAGIC, 1 | (b.mode << 32), b.n_t | (b.n_mu << 32), b.n_e, e & MASK,
                     checkpoint.digest(binw)[0], rejected, checkpoint.digest(pay)[0]], dtype=np.uint64)
    return np.concatenate([head, pay])


def yard_doubles(b, w_max, y):
    F, F2, cnt, _, _ = y
    e = exponent(b, w_max)
    shape = (b.n_t, b.n_mu, b.n_e)
    qF, qF2 = Fraction(2) ** (e - 84), Fraction(2) ** (2 * e - 84)
    return (np.array([float(x * qF) for x in F]).reshape(shape),
            np.array([float(x * qF2) for x in F2]).reshape(shape),
            np.array([float(x) for x in cnt]).reshape(shape))


def _check(b, w_max, y, state):
    want = yard_state(b, w_max, y)
    assert state.dtype == np.uint64 and state.shape == want.shape
    bad = np.flatnonzero(state != want)
    assert bad.size == 0, (bad[:8], state[bad[:8]], want[bad[:8]])
    h = observer.state_result(state)
    for got, ref in zip((h.F, h.F2, h.count), yard_doubles(b, w_max, y)):
        assert np.array_equal(got, ref)


def _fixture_yard(name):
    if name not in _YARD:
        b = _binning(name)
        ev = G["events"]
        w_max = float(ev[:, 2].max())
        _YARD[name] = (b, w_max, yardstick(name, b, w_max, ev))
    return _YARD[name]


# ---------------------------------------------------------------------------
# the crafted set: G = 1 (beta = 0, w = ew exactly), r = z = 0 (time = t_bound)
# ---------------------------------------------------------------------------
CRAFT_W_MAX = 1.0                      # e = E(1) + E(2) = 1 + 2 = 3: weights below 8


def craft_sed():
    return observer.sed_binning(1.0, 0.0, 3, 0., 3., -1.0, 1.0, ((1., 1e4, 4, False),))


def craft_lc():
    """Two angular bins, energy bands that overlap (10..1000 lies in two)."""
    return observer.lc_binning(1.0, 0.0, ((-1.0, 0.0), (0.0, 1.0)), 1.0, 0.0, 3.0,
                               ((1., 1e3, 1, False), (10., 1e4, 1, False), (1e3, 1e4, 1, False)))


def craft_events(e=3, hot=70_000):
    top = float(np.nextafter(2.0 ** e, 0.0))                    # one ulp below 2^e
    q = 2.0 ** (e - 84)
    rows = []

    def ev(t, E, ew, wmu=-0.5):
        rows.append([t, E, ew, 0.0, 0.0, wmu, 0.0])
    for ew in (top, q * 0.75, q, q * 1.5, 5e-324, 0.0, -0.0, 1.2345678 * 2.0 ** (e - 3),
               2.0 ** (e - 20) * (1 + 2.0 ** -52), 2.0 ** (e - 42), 2.0 ** e / 3):
        ev(0.5, 20., ew)
        ev(1.5, 2000., ew, 0.5)
        ev(2.5, 5., ew)
    for ew in (float("nan"), -1.0, -5e-324, 2.0 ** e, float("inf")):   # rejected: in a bin, weight not admitted
        ev(0.5, 20., ew)
    for ew in (float("nan"), 2.0 ** e, 1.0):                   # outside every bin: neither added nor rejected
        ev(-1.0, 20., ew)
        ev(0.5, 1e5, ew)
    for _ in range(hot):                                        # limb carries: maximal weights in one bin
        ev(1.5, 20., top)
    return np.array(rows, np.float64)


def _craft(which):
    if which not in _YARD:
        b = craft_sed() if which == "craft_sed" else craft_lc()
        ev = craft_events()
        _YARD[which] = (b, ev, yardstick(which, b, CRAFT_W_MAX, ev))
    return _YARD[which]


@pytest.mark.parametrize("name", DECKS)
def test_twin_equals_the_integers_on_the_reference_events(name):
    b, w_max, y = _fixture_yard(name)
    ev = G["events"]
    assert y[3] == 0                                   # w_max = max(ew): the reference data rejects nothing
    assert sum(y[2]) > 0
    state = observer.exact_host(b, w_max, ev)
    _check(b, w_max, y, state)
    assert observer.state_info(state)["n_rejected"] == 0
    # the f64 sums agree with the integers to their own rounding and the integers' truncation
    F, F2, cnt = OL.obs_bin(b, ev, flavor="det")
    h = observer.state_result(state)
    assert np.array_equal(h.count, cnt)
    e = exponent(b, w_max)                             # truncation: below one quantum per addend
    assert np.all(np.abs(h.F - F) <= 1e-12 * F + cnt * 2.0 ** (e - 84))
    assert np.all(np.abs(h.F2 - F2) <= 1e-12 * F2 + cnt * 2.0 ** (2 * e - 84))


@pytest.mark.parametrize("which", ["craft_sed", "craft_lc"])
def test_twin_equals_the_integers_on_the_crafted_set(which):
    b, ev, y = _craft(which)
    state = observer.exact_host(b, CRAFT_W_MAX, ev)
    _check(b, CRAFT_W_MAX, y, state)
    F, F2, cnt, rejected, _ = y
    assert rejected == 5 and observer.state_info(state)["n_rejected"] == 5
    assert observer.state_info(state)["e"] == 3
    assert max(F) >> 64 and max(F2) >> 64              # the hot bin's sums fill both limbs
    assert max(cnt) >= 70_000
    if which == "craft_lc":                            # E = 20 lies in two bands, E = 2000 in two others
        c = np.array(cnt).reshape(b.n_t, b.n_mu, b.n_e)
        assert c[0, 1, 0] == c[0, 1, 1] > 0 and c[1, 0, 1] == c[1, 0, 2] > 0


@pytest.mark.parametrize("which", ["craft_sed", "craft_lc", "lc_wide"])
def test_any_order_and_any_split_give_the_same_state(which):
    if which.startswith("craft"):
        b, ev, _ = _craft(which)
        w_max = CRAFT_W_MAX
    else:
        b, w_max, _ = _fixture_yard(which)
        ev = G["events"]
    whole = observer.exact_host(b, w_max, ev)
    rng = np.random.default_rng(5)
    for _ in range(2):
        assert np.array_equal(observer.exact_host(b, w_max, ev[rng.permutation(len(ev))]), whole)
    for cuts in ((1,), (len(ev) // 3, len(ev) // 2), (7, 8, 9, len(ev) - 1)):
        s = None
        for part in np.split(ev, cuts):
            s = observer.exact_host(b, w_max, part, state=s)
        assert np.array_equal(s, whole)
    # merge of two halves = the whole, n_rejected included
    half = len(ev) // 2
    a, c = observer.exact_host(b, w_max, ev[:half]), observer.exact_host(b, w_max, ev[half:])
    assert np.array_equal(observer.state_merge(a, c), whole)
    assert np.array_equal(observer.state_merge(c, a), whole)
    empty = observer.exact_host(b, w_max, ev[:0])
    assert np.array_equal(observer.state_merge(empty, whole), whole)


def test_the_truncation_bound():
    """0 <= sum(w) - F 2^qF < count 2^qF, per bin, in exact arithmetic."""
    for b, w_max, y in (_fixture_yard("sed_wide"), (_craft("craft_lc")[0], CRAFT_W_MAX, _craft("craft_lc")[2])):
        F, _, cnt, _, S = y
        q = Fraction(2) ** (exponent(b, w_max) - 84)
        for h in range(len(F)):
            d = S[h] - F[h] * q
            assert 0 <= d and (d < cnt[h] * q or cnt[h] == 0 == d)


def test_the_exponent_range_is_enforced():
    ev = np.array([[0.5, 20., 0.0, 0., 0., -0.5, 0.]])
    b = craft_sed()
    for w_max, ok in ((2.0 ** -472, True), (2.0 ** -473, False), (2.0 ** 486, True), (2.0 ** 487, False)):
        if not ok:
            with pytest.raises(C2DError, match="C2D_E_ARG"):
                observer.exact_host(b, w_max, ev)
            continue
        e = exponent(b, w_max)
        assert e in (-469, 489)
        top = float(np.nextafter(2.0 ** e, 0.0))
        evs = np.array([[0.5, 20., w, 0., 0., -0.5, 0.] for w in (top, top, 2.0 ** e, top / 3, 2.0 ** (e - 84))])
        y = yardstick(("range", e), b, w_max, evs)
        assert y[3] == 1
        _check(b, w_max, y, observer.exact_host(b, w_max, evs))
    for w_max in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(C2DError, match="C2D_E_ARG"):
            observer.exact_host(b, w_max, ev)


def test_damaged_and_foreign_states_are_refused():
    b, ev, _ = _craft("craft_sed")
    ev = ev[:60]
    good = observer.exact_host(b, CRAFT_W_MAX, ev)
    bad = good.copy()
    bad[abi.OBS_STATE_HEAD_WORDS + 7] ^= np.uint64(1)            # one bit of the payload
    for s in (bad, good[:-1], good[:5]):
        with pytest.raises(C2DError, match="C2D_E_ARG"):
            observer.state_result(s)
        with pytest.raises(C2DError, match="C2D_E_ARG"):
            observer.state_merge(good, s)
    with pytest.raises(C2DError, match="C2D_E_ARG"):
        observer.state_merge(bad, good)
    with pytest.raises(C2DError, match="C2D_E_ARG"):
        observer.exact_host(b, CRAFT_W_MAX, ev, state=bad)
    # the same shape, another edge / rmax / bound: refused, and nothing is changed
    other = copy.copy(b)
    other.E1 = b.E1.copy()
    other.E1[-1] *= 2
    far = copy.copy(b)
    far.rmax = 1.0
    for foreign in (observer.exact_host(other, CRAFT_W_MAX, ev), observer.exact_host(far, CRAFT_W_MAX, ev),
                    observer.exact_host(b, 4 * CRAFT_W_MAX, ev)):
        keep = good.copy()
        with pytest.raises(C2DError, match="C2D_E_ARG"):
            observer.state_merge(keep, foreign)
        assert np.array_equal(keep, good)
    with pytest.raises(C2DError, match="C2D_E_ARG"):
        observer.exact_host(other, CRAFT_W_MAX, ev, state=good)
    # a sum that would carry out of bit 127
    full = good.copy()
    pay = full[abi.OBS_STATE_HEAD_WORDS:].reshape(-1, 5)
    pay[0, 1] = np.uint64(MASK)
    full[7] = np.uint64(checkpoint.digest(pay)[0])
    assert observer.state_info(observer.state_merge(full, observer.exact_host(b, CRAFT_W_MAX, ev[:0])))["n_t"] == 3
    with pytest.raises(C2DError, match="C2D_E_ARG"):
        observer.state_merge(full, full)
