"""Plain-IEEE restatement of the Compton reflection — TEST INFRASTRUCTURE.

* `tables()`: E_ref, P_ref, W_abs as src/ref_matrix.f builds them, written
  from the description in include/compton2d.h / csrc/reflect_host.h with
  Python floats and `math` (glibc's pow/exp/log/sqrt, one call per element in
  the reference's order), layout [n_in][n_out].
* `draw(key, sub, n)`: draw n of the lineage stream (key, sub), csrc/c2d_rng.h
  c2d_draw_s (SplitMix64).
* `get_bin(...)`: the spectral, light-curve and angular bin of a photon
  (imcleak2d.f get_bin), 1-based, 0 = none.
* `reflect_lower`, `reflect_outer`: the two branches on one packet state, in
  the reference's order of operations; every product and sum is one rounded
  IEEE operation, as the device code with contraction off.
"""
from __future__ import annotations

import math
import struct

import numpy as np

N_REF = 500
RAD_CP = 3.333564097e-11
TIME, DT = 100.0, 10.0          # c2d_selftest_reflect's clock
M64 = (1 << 64) - 1


def f32(x: float) -> float:
    """A Fortran REAL literal promoted to double."""
    return struct.unpack("f", struct.pack("f", x))[0]


# neutral ions: abundance, K-edge sigma and energy, L-edge sigma and energy
IONS = (
    (6.33e-2, 9.0e-18, f32(.024), 0.0, 0.0),
    (3.90e-4, 1.e-18, f32(.30), 3.e-16, f32(.011)),
    (8.12e-5, 9.e-19, f32(.40), 3.e-16, f32(.014)),
    (6.47e-4, 6.e-19, f32(.52), 5.e-16, f32(.013)),
    (9.14e-5, 4.e-19, f32(.88), 1.e-15, f32(.021)),
    (3.73e-5, 2.e-19, f32(1.2), 4.e-17, f32(.054)),
    (3.52e-5, 1.3e-19, f32(1.8), 4.e-17, f32(.11)),
    (1.76e-5, 1.e-19, f32(2.4), 1.e-17, f32(.16)),
    (3.73e-6, 8.e-20, f32(3.1), 7.e-18, f32(.23)),
    (2.20e-6, 7.e-20, f32(4.1), 4.e-18, f32(.35)),
    (3.16e-5, 3.e-20, f32(7.1), 2.5e-18, f32(.71)),
    (f32(1.68e-6), 3.e-20, f32(8.2), 2.e-18, f32(.89)),
)

_tables = None


def tables():
    """(E_ref [500], P_ref [n_in, n_out], W_abs [n_in, n_out]); computed once."""
    global _tables
    if _tables is not None:
        return _tables
    N = N_REF
    pw, sq = math.pow, math.sqrt
    dE = math.exp(math.log(1.e3) / float(N))
    E = [1.0]
    for _ in range(1, N):
        E.append(E[-1] * dE)
    P = np.zeros((N, N))
    W = np.zeros((N, N))
    for ni in range(N):
        if E[ni] <= 20.0:
            P[ni, ni:] = 1.0
            continue
        x0 = 1.957e-3 * E[ni]
        y0 = 1.0 / x0
        dyc = 1.e3 - y0
        A = 5.6e-1 + f32(1.12) / pw(y0, f32(0.785)) - 3.4e-1 / pw(y0, f32(1.04))
        al = -3.e-1 / pw(y0, f32(.51)) + 6.e-2 / pw(y0, f32(.824))
        beta = 3.7e-1 - pw(y0, f32(.85))
        den = pw(y0, 1.0 - beta) * pw(y0 + 2.0, beta) * (pw(1.0 + 2.0 / y0, 1.0 - beta) - 1.0)
        if abs(al + .5) < 1.e-4:
            B = (1.0 - A * (2.0 + math.log(.5 * dyc)) / sq(dyc)) / den * (1.0 - beta)
        else:
            B = (1.0 - A * (2.0 + (pw(.5 * dyc, al + .5) - 1.0) / (al + .5)) / sq(dyc)) / den * (1.0 - beta)
        s = 0.0
        col = [0.0] * (ni + 1)
        for no in range(ni + 1):
            x1 = 1.957e-3 * E[no]
            dy = 1.0 / x1 - y0
            if dy < 2.0:
                Gy = B * pw((y0 + 2.0) / (y0 + dy), beta)
            elif dy < dyc:
                Gy = A * pw(dyc / dy, al) / pw(dy, 1.5)
            else:
                Gy = A / pw(dy, 1.5)
            s = s + (Gy / (x1 * x1)) * (dE * x1)
            col[no] = s
        P[ni, :ni + 1] = [c / s for c in col]
        P[ni, ni + 1:] = 1.0
    n_disk = 1.e18
    kappa_c = 6.65e-25 * n_disk
    eps = []
    for n in range(N):
        s = 0.0
        for i, (ab, sg, ed, sg2, ed2) in enumerate(IONS):
            if i == 0 or E[n] > ed:
                q = E[n] / ed
                s = s + sg * ab / (q * q * q)
            if i > 0 and E[n] > ed2:
                q = E[n] / ed2
                s = s + sg2 * ab / (q * q * q)
        k_nu = s * n_disk
        eps.append(k_nu / (k_nu + kappa_c))
    for ni in range(N):
        x0 = 1.957e-3 * E[ni]
        for no in range(ni + 1):
            if E[ni] > 20.0:
                x1 = 1.957e-3 * E[no]
                y = 2.5e-6 * (1.0 / (x0 * x0 * x0 * x0) - 1.0 / (x1 * x1 * x1 * x1))
                W[ni, no] = min(1.0, math.exp(y)) if y >= -50.0 else 0.0
            else:
                W[ni, no] = (1.0 - sq(eps[ni])) / (1.0 + sq(eps[ni]))
    _tables = (np.array(E), P, W)
    return _tables


def mix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(key: int, sub: int, n: int) -> float:
    """c2d_draw_s: 53 bits of SplitMix64 output (sub << 32 | n) of the key's sequence, in (0, 1)."""
    x = mix64((int(key) + 0x9E3779B97F4A7C15 * ((((int(sub) << 32) | int(n)) + 1) & M64)) & M64)
    return (float(x >> 11) + 0.5) * 1.1102230246251565404e-16


def get_bin(xnu, wmu, hu, Elcmin, Elcmax, mu):
    """(jgpsp, jgplc, jgpmu) of imcleak2d.f's get_bin: hu[0..nphtotal] etc. 0-based arrays."""
    nph = len(hu) - 1
    jgpsp = 0
    if not (xnu >= f32(.999999) * hu[nph] or xnu <= f32(1.000001) * hu[0]):
        jbot, jtop = 1, nph + 1
        while True:
            jmid = (jbot + jtop) // 2
            if jmid == jbot or xnu == hu[jmid - 1]:
                break
            if xnu < hu[jmid - 1]:
                jtop = jmid
            else:
                jbot = jmid
        jgpsp = jmid
    jgplc = 0
    for m in range(len(Elcmin)):
        if Elcmin[m] < xnu <= Elcmax[m]:
            jgplc = m + 1
            break
    jgpmu = len(mu)
    for n in range(len(mu)):
        if wmu <= mu[n]:
            jgpmu = n + 1
            break
    return jgpsp, jgplc, jgpmu


def _sample(st, key):
    """n_in, rnum, n_out, the new xnu and ew; st = dict(xnu, ew, ..., ctr)."""
    E, P, W = tables()
    xnu_sv = st["xnu"]
    # first n_in with E_ref(n_in) >= xnu, capped at n_ref (the reference scans linearly)
    n_in = min(int(np.searchsorted(E, st["xnu"], side="left")) + 1, N_REF)
    rnum = draw(key, 0, st["ctr"])
    st["ctr"] += 1
    col = P[n_in - 1]
    # first n_out with P_ref(n_out, n_in) >= rnum, capped (the column is non-decreasing)
    n_out = min(int(np.searchsorted(col, rnum, side="left")) + 1, N_REF)
    if n_out > 1:
        e0, e1 = float(E[n_out - 2]), float(E[n_out - 1])
        u = draw(key, 0, st["ctr"])
        st["ctr"] += 1
        st["xnu"] = e0 + u * (e1 - e0)
    else:
        st["xnu"] = float(E[0])
    st["ew"] = st["ew"] * float(W[n_in - 1, n_out - 1]) * st["xnu"] / xnu_sv
    st["n_in"], st["n_out"] = n_in, n_out


def _state(s):
    return dict(xnu=float(s[0]), ew=float(s[1]), wmu=float(s[2]), rpre=float(s[3]), zpre=float(s[4]),
                phi=float(s[5]), dcen=float(s[6]), tbbl=float(s[7]), ctr=0, n_in=0, n_out=0, idead=1)


def _row(st, tb):
    return [st["xnu"], st["ew"], st["wmu"], st["rpre"], st["zpre"], tb, float(st["ctr"]), float(st["idead"]),
            float(st["n_in"]), float(st["n_out"])]


def reflect_lower(s, key: int, cr_sent: int):
    """One state at the lower boundary: (the selftest's output row, the Ed_ref add)."""
    st = _state(s)
    tb = TIME + DT - RAD_CP * st["dcen"]
    ed = 0.0
    if cr_sent in (1, 3, 4):
        if st["tbbl"] <= 0.0 or cr_sent == 4:
            st["wmu"] = -st["wmu"]
        else:
            _sample(st, key)
            ed = st["ew"]
            st["wmu"] = abs(st["wmu"])
        st["idead"] = 0
    return _row(st, tb), ed


def reflect_outer(s, key: int, cr_sent: int):
    """One state at the outer r-boundary: the selftest's output row."""
    st = _state(s)
    tb = TIME + DT - RAD_CP * st["dcen"]
    if not (st["wmu"] > 0.0) and cr_sent in (2, 3):
        _sample(st, key)
        if abs(st["wmu"]) > 1.0e-6:
            tb = TIME + DT - RAD_CP * (st["dcen"] + st["zpre"] / st["wmu"])
            st["zpre"] = 0.0
            f = st["zpre"] * math.sqrt(1.0 - st["wmu"] ** 2) / abs(st["wmu"])
            st["rpre"] = math.sqrt(st["rpre"] ** 2 + f ** 2 + 2.0 * st["rpre"] * f * math.cos(st["phi"]))
        else:
            tb = 1.0e20
        st["wmu"] = draw(key, 0, st["ctr"])
        st["ctr"] += 1
    return _row(st, tb), 0.0


def reflect_many(boundary: int, cr_sent: int, states, keys):
    """Rows [n, 10] and the sum of the Ed_ref adds."""
    fn = reflect_lower if boundary == 0 else reflect_outer
    rows, tot = [], []
    for s, k in zip(np.asarray(states, float).reshape(-1, 8), np.asarray(keys, np.uint64).ravel()):
        r, ed = fn(s, int(k), cr_sent)
        rows.append(r)
        tot.append(ed)
    return np.array(rows), math.fsum(tot)
