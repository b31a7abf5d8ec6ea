"""Test systems, exact reference and float64 models for the fast FP kernel's
tridiagonal solvers (compton2d_amd/csrc/fp_fast.hip spike_solve / pcr_solve) —
TEST INFRASTRUCTURE (tests/test_gpu_fp_solver.py).

Every system is an M-matrix as the Chang-Cooper step produces: a, c <= 0,
b_i >= 1 + |a_{i+1}| + |c_{i-1}| (column dominance: the scheme conserves
particles), rows 1 and 200 identity rows.  For such a matrix M^-1 >= 0, so the
componentwise condition vector e = u M^-1 (|M| |x| + |d|), u = 2^-53, is one
more solve.  The reference is Thomas elimination in 100-digit arithmetic
(mpmath): one factorisation per matrix, any number of right-hand sides."""
import functools
from fractions import Fraction

import numpy as np
from mpmath import mp, mpf

from tridag_ref import tridag_ref

NT = 200
FPB = 64
U = mpf(2) ** -53
DPS = 100                     # digits of the reference arithmetic
CAP = 8                       # |x - x_exact| <= CAP * e, per row

# rows (1-based) next to a wave interface of spike_solve, and the ends
EDGE_ROWS = (1, 2, 63, 64, 65, 66, 127, 128, 129, 130, 191, 192, 193, 194, 199, 200)
FAMILIES = {"weak": (-6.0, -2.0, False), "mid": (-1.0, 1.0, False), "stiff": (2.0, 6.0, False),
            "mixed": (-8.0, 8.0, True)}
PER_FAMILY = 6


def m_matrix(rng, lo, hi, per_row):
    """a, b, c [NT]: |a|, |c| log-uniform in 10^lo..10^hi, drawn per entry, or
    (per_row) one magnitude per row with a and c within a factor 2 of it."""
    if per_row:
        m = 10.0 ** rng.uniform(lo, hi, NT)
        a, c = -m * rng.uniform(0.5, 1.0, NT), -m * rng.uniform(0.5, 1.0, NT)
    else:
        a, c = -(10.0 ** rng.uniform(lo, hi, NT)), -(10.0 ** rng.uniform(lo, hi, NT))
    a[0] = c[0] = a[NT - 1] = c[NT - 1] = 0.0
    col = np.zeros(NT)                        # |a_{i+1}| + |c_{i-1}|
    col[:-1] += np.abs(a[1:])
    col[1:] += np.abs(c[:-1])
    b = 1.0 + col + rng.uniform(0.0, 0.1, NT) * (1.0 + col)    # the escape term's share
    b[0] = b[NT - 1] = 1.0
    return a, b, c


def decaying_rhs(rng):
    """d [NT] >= 0: falls by e^-40 over rows 1..150, then down to 1e-300 at
    row 199; scattered tail entries are exact zeros and denormals."""
    i = np.arange(NT, dtype=np.float64)
    d = np.exp(-40.0 * i / 150.0) * rng.uniform(0.5, 1.5, NT)
    t = np.arange(150, NT)
    d[t] = 10.0 ** (-17.4 - 282.6 * (t - 150) / 48.0) * rng.uniform(0.5, 1.5, len(t))
    d[NT - 1] = 0.0
    tail = rng.permutation(np.arange(120, NT - 2))      # row 199 keeps its ~1e-300
    d[tail[:6]] = 0.0
    d[tail[6:12]] = 5e-324 * rng.integers(1, 1000, 6)
    return d


@functools.lru_cache(maxsize=None)
def systems():
    """Ordered {label: (a, b, c, d)}; seeded, the same in every process."""
    out = {}
    ident = np.zeros(NT), np.ones(NT), np.zeros(NT)
    out["identity"] = ident + (decaying_rhs(np.random.default_rng(11)),)
    rng = np.random.default_rng(12)
    b = 1.0 + 10.0 ** rng.uniform(-6.0, 6.0, NT)
    b[0] = b[NT - 1] = 1.0
    d = decaying_rhs(rng)
    d[(d > 0.0) & (d < 1e-300)] = 0.0         # d / b of a denormal has no relative bound
    out["diagonal"] = (np.zeros(NT), b, np.zeros(NT), d)
    a, b, c = m_matrix(np.random.default_rng(13), -1.0, 1.0, False)
    for r in EDGE_ROWS:
        d = np.zeros(NT)
        d[r - 1] = 1.0
        out["onehot%d" % r] = (a, b, c, d)
    for f, (name, (lo, hi, per_row)) in enumerate(FAMILIES.items()):
        rng = np.random.default_rng(100 + f)
        for k in range(PER_FAMILY):
            out["%s%d" % (name, k)] = m_matrix(rng, lo, hi, per_row) + (decaying_rhs(rng),)
    return out


def family(label):
    return label.rstrip("0123456789")


def stacked():
    """labels, a, b, c, d [nsys, NT] in systems() order (one launch solves all)."""
    s = systems()
    return (list(s),) + tuple(np.array([v[q] for v in s.values()]) for q in range(4))


class ExactTridiag:
    """Thomas elimination at DPS digits: factor once, solve many.  Elimination
    of a column-dominant tridiagonal matrix needs no pivoting and is
    componentwise backward stable, so its own error is ~10^(16 - DPS) e: it
    plays no part in a comparison against CAP * e.  Inputs convert exactly
    (denormals too: the exponent range is unbounded), sums of non-negative
    terms do not cancel, so e_i = 0 exactly where the rationals give 0."""

    def __init__(self, a, b, c):
        with mp.workdps(DPS):
            self.a, self.b, self.c = ([mpf(float(v)) for v in x] for x in (a, b, c))
            n = len(self.b)
            self.bet, self.gam = [self.b[0]] * n, [mpf(0)] * n
            for i in range(1, n):
                self.gam[i] = self.c[i - 1] / self.bet[i - 1]
                self.bet[i] = self.b[i] - self.a[i] * self.gam[i]

    def solve(self, d):
        with mp.workdps(DPS):
            n = len(self.b)
            f = [mpf(0)] * n
            f[0] = mpf(d[0]) / self.bet[0]
            for i in range(1, n):
                f[i] = (mpf(d[i]) - self.a[i] * f[i - 1]) / self.bet[i]
            for i in range(n - 2, -1, -1):
                f[i] = f[i] - self.gam[i + 1] * f[i + 1]
            return f

    def condition(self, d, x):
        """e = u M^-1 (|M| |x| + |d|) for the solution x of M x = d."""
        with mp.workdps(DPS):
            n = len(self.b)
            ax = [abs(v) for v in x]
            r = []
            for i in range(n):
                s = self.b[i] * ax[i] + abs(mpf(d[i]))
                if i > 0:
                    s += abs(self.a[i]) * ax[i - 1]
                if i < n - 1:
                    s += abs(self.c[i]) * ax[i + 1]
                r.append(s)
            return [U * v for v in self.solve(r)]


@functools.lru_cache(maxsize=None)
def exact():
    """{label: (x_exact, e)}, lists of mpf; computed once per process."""
    out, fac = {}, {}
    for label, (a, b, c, d) in systems().items():
        key = (a.tobytes(), b.tobytes(), c.tobytes())
        if key not in fac:
            fac[key] = ExactTridiag(a, b, c)
        x = fac[key].solve([float(v) for v in d])
        out[label] = (x, fac[key].condition([float(v) for v in d], x))
    return out


def ratios(label, x):
    """max_i |x_i - x_exact,i| / e_i of a float64 solution x [NT]; inf where a
    row with e_i = 0 is not exact."""
    xe, e = exact()[label]
    worst = 0.0
    with mp.workdps(DPS):
        for i in range(NT):
            err = abs(mpf(float(x[i])) - xe[i])
            if err == 0:
                continue
            if e[i] == 0:
                return float("inf")
            worst = max(worst, float(err / e[i]))
    return worst


def is_m_matrix(a, b, c):
    """The stated conditions, checked on the float64 values over the rationals."""
    fa, fb, fc = ([Fraction(float(v)) for v in x] for x in (a, b, c))
    ok = all(v <= 0 for v in fa) and all(v <= 0 for v in fc)
    ok = ok and fa[0] == fc[0] == fa[NT - 1] == fc[NT - 1] == 0 and fb[0] == fb[NT - 1] == 1
    for i in range(1, NT - 1):
        ok = ok and fb[i] >= 1 + abs(fa[i + 1]) + abs(fc[i - 1])
    return ok


# ---- float64 models of the three algorithms (IEEE division where the GPU
# ---- takes v_rcp_f64 and two Newton steps; no fused multiply-add, as the
# ---- library is built) ------------------------------------------------------

def thomas_model(a, b, c, d):
    return tridag_ref(a, b, c, d, np.zeros(NT))


def _shift(v, s, fill):
    """(v[i - s], v[i + s]) with `fill` outside the last axis."""
    m, p = np.full_like(v, fill), np.full_like(v, fill)
    m[..., s:] = v[..., :-s]
    p[..., :-s] = v[..., s:]
    return m, p


def pcr_model(a, b, c, d):
    """pcr_solve: parallel cyclic reduction over rows 1..NT, 8 levels."""
    a, b, c, d = (np.array(v, np.float64) for v in (a, b, c, d))
    s = 1
    while s < NT:
        (am, ap), (bm, bp), (cm, cp), (dm, dp) = _shift(a, s, 0.0), _shift(b, s, 1.0), _shift(c, s, 0.0), \
            _shift(d, s, 0.0)
        k1, k2 = a * (1.0 / bm), c * (1.0 / bp)
        a, c, b, d = -am * k1, -cp * k2, b - cm * k1 - ap * k2, d - dm * k1 - dp * k2
        s <<= 1
    return d / b


def spike_model(a, b, c, d, bs=256):
    """spike_solve: per-wave cyclic reduction of d and the two spikes, the
    chain over the wave interfaces, the combination; rows past NT identity."""
    W = bs // FPB

    def pad(v, fill):
        return np.concatenate([np.asarray(v, np.float64), np.full(bs - NT, fill)]).reshape(W, FPB)

    a, b, c, d = pad(a, 0.0), pad(b, 1.0), pad(c, 0.0), pad(d, 0.0)
    v, w = np.zeros((W, FPB)), np.zeros((W, FPB))
    v[:, 0], w[:, -1] = a[:, 0], c[:, -1]
    a[:, 0] = 0.0
    c[:, -1] = 0.0
    r = 1.0 / b
    a, c, d, v, w = a * r, c * r, d * r, v * r, w * r
    s = 1
    while s < FPB:
        (am, ap), (cm, cp), (dm, dp), (vm, vp), (wm, wp) = (_shift(q, s, 0.0) for q in (a, c, d, v, w))
        r = 1.0 / (1.0 - a * cm - c * ap)
        na, nc = -(a * am), -(c * cp)
        d = (d - a * dm - c * dp) * r
        v = (v - a * vm - c * vp) * r
        w = (w - a * wm - c * wp) * r
        a, c = na * r, nc * r
        s <<= 1
    first = np.stack([d[:, 0], v[:, 0], w[:, 0]], 1)           # f_if[p][0..2]
    last = np.stack([d[:, -1], v[:, -1], w[:, -1]], 1)         # f_if[p][3..5]
    A, Bp, G, H = ([np.float64(0.0)] * (W + 1) for _ in range(4))
    A[1], Bp[1] = last[0][0], -last[0][2]
    for p in range(1, W):
        yf, vf, wf = first[p]
        q = 1.0 / (1.0 + vf * Bp[p])
        G[p] = (yf - vf * A[p]) * q
        H[p] = -(wf * q)
        if p + 1 < W:
            yl, vl, wl = last[p]
            A[p + 1] = yl - vl * (A[p] + Bp[p] * G[p])
            Bp[p + 1] = -(vl * Bp[p] * H[p] + wl)
    F, L = [np.float64(0.0)] * (W + 1), [np.float64(0.0)] * W
    for p in range(W - 1, 0, -1):
        F[p] = G[p] + H[p] * F[p + 1]
        L[p - 1] = A[p] + Bp[p] * F[p]
    x = np.zeros((W, FPB))
    for p in range(W):
        xl = L[p - 1] if p >= 1 else 0.0
        xr = F[p + 1] if p + 1 < W else 0.0
        x[p] = d[p] - v[p] * xl - w[p] * xr
    return x.reshape(-1)[:NT]


MODELS = {"thomas": thomas_model, "pcr": pcr_model, "spike": spike_model}
