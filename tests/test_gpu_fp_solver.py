"""The fast FP kernel's parts on their own (compton2d_amd/csrc/fp_fast.hip):
its tridiagonal solvers row by row against a 100-digit reference, and its block
reductions, scans and searches per thread.

Solvers (spike_solve, what the kernel runs, and pcr_solve, the C2D_FPF_SPIKE=0
alternative, both through c2d_selftest_fp_solve): every system is an M-matrix
as the Chang-Cooper step produces (tests/fp_solver_ref.py), so with
u = 2^-53 the componentwise condition vector e = u M^-1 (|M| |x| + |d|) is one
more solve, and each row must satisfy |x_i - x_exact,i| <= 8 e_i.  A float64
numpy model of Thomas elimination (tests/tridag_ref.py), of pcr_solve and of
spike_solve (IEEE division where the GPU takes v_rcp_f64 and two Newton steps)
reaches at most 1.4, 2.4 and 3.1 e_i on these systems; 8 is ~3x the worst
model figure, about one rounding per reduction level plus the interface chain
and the final combination.  The CPU tests below hold the three models to the
same cap on every system, so a GPU failure is a defect of the kernel, not of
the algorithm or of the inputs.  Measured on an MI355X, max over each family's
systems (identity, diagonal, one-hot, weak, mid, stiff, mixed):
  spike_solve 0, 0.67, 0.83, 2.94, 1.66, 1.70, 3.06
  pcr_solve   0, 0.47, 0.53, 2.42, 1.89, 1.73, 1.89  (its model's figures exactly)

Block primitives (Blk::sum2, scan, scan_sum, minmax, min2, firsts through
c2d_selftest_fp_block): the kernel's `while` loops contain barriers and stay
uniform only because every thread gets the same bits from a reduction, so
every thread's result is returned and compared."""
import math

import numpy as np
import pytest

import fp_solver_ref as R

CAP = R.CAP
U = 2.0 ** -53
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


# ---- CPU: the inputs and the algorithms themselves stay inside the cap -------

def test_fp_solver_systems_are_m_matrices():
    for label, (a, b, c, d) in R.systems().items():
        assert R.is_m_matrix(a, b, c), label
        assert np.all(d >= 0.0) and np.all(np.isfinite(d)), label
    fam = [d for label, (_, _, _, d) in R.systems().items() if R.family(label) in R.FAMILIES]
    assert len(fam) == len(R.FAMILIES) * R.PER_FAMILY
    for d in fam:
        tiny = d[(d > 0.0) & (d < 2.2250738585072014e-308)]
        assert len(tiny) >= 1 and np.sum(d[1:-1] == 0.0) >= 1 and d.max() > 0.4
        assert np.any((d >= 2.2250738585072014e-308) & (d < 2e-300))


@pytest.mark.parametrize("model", list(R.MODELS))
def test_fp_solver_float64_models_within_cap(model, capsys):
    """Thomas elimination as tests/tridag_ref.py states it, and the numpy
    models of pcr_solve and spike_solve, in float64 on every system used on
    the GPU: each row within CAP e_i (a row with e_i = 0 exact)."""
    worst = {}
    for label, (a, b, c, d) in R.systems().items():
        r = R.ratios(label, R.MODELS[model](a, b, c, d))
        worst[R.family(label)] = max(worst.get(R.family(label), 0.0), r)
    with capsys.disabled():
        print("\nfloat64 %s model, max |x - x_exact| / e per family: %s"
              % (model, {k: "%.2f" % v for k, v in worst.items()}))
    assert max(worst.values()) <= CAP, worst


def test_fp_solver_models_solve_the_identity_exactly():
    a, b, c, d = R.systems()["identity"]
    for name, f in R.MODELS.items():
        np.testing.assert_array_equal(f(a, b, c, d).view(np.uint64), d.view(np.uint64), err_msg=name)


# ---- GPU: the solvers ----------------------------------------------------------

SOLVERS = {"spike": 0, "pcr": 1}
_solved = {}


def solved(name):
    """Every system of fp_solver_ref.systems() in one launch, one after another
    through the same workgroup; once per solver."""
    if name not in _solved:
        from compton2d_amd.engine import device_fp_solve
        labels, a, b, c, d = R.stacked()
        _solved[name] = dict(zip(labels, device_fp_solve(SOLVERS[name], a, b, c, d)))
    return _solved[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SOLVERS))
def test_gpu_fp_solver_rows_within_cap(name, capsys):
    """Identity, diagonal, one-hot right-hand sides at the rows next to each
    wave interface and at the ends, and the four coefficient families: every
    row within CAP e_i of the reference, a row with e_i = 0 exact, and the
    threads past row 200 return 0."""
    x = solved(name)
    worst, ratio = {}, {label: R.ratios(label, x[label][:R.NT]) for label in R.systems()}
    for label, r in ratio.items():
        worst[R.family(label)] = max(worst.get(R.family(label), 0.0), r)
    with capsys.disabled():
        print("\n%s_solve on the GPU, max |x - x_exact| / e per family: %s"
              % (name, {k: "%.2f" % v for k, v in worst.items()}))
    for label in R.systems():
        assert ratio[label] <= CAP, (name, label, ratio[label])
        tail = x[label][R.NT:]
        assert np.all(tail == 0.0), (name, label, tail[tail != 0.0][:4])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SOLVERS))
def test_gpu_fp_solver_identity_is_bitwise(name):
    d = R.systems()["identity"][3]
    np.testing.assert_array_equal(solved(name)["identity"][:R.NT].view(np.uint64), d.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SOLVERS))
def test_gpu_fp_solver_result_does_not_depend_on_the_call_before(name):
    """The solvers keep rows in LDS between their steps, and the kernel calls
    them sub-step after sub-step: a system solved after 40 others gives the
    bits it gives alone and after a different one."""
    from compton2d_amd.engine import device_fp_solve
    s = R.systems()
    for label, before in (("mixed5", "stiff0"), ("onehot129", "weak3"), ("weak0", "mixed2")):
        pair = [np.array([s[before][q], s[label][q]]) for q in range(4)]
        alone = [v[1:] for v in pair]
        xa = device_fp_solve(SOLVERS[name], *alone)[0]
        xp = device_fp_solve(SOLVERS[name], *pair)[1]
        np.testing.assert_array_equal(xa.view(np.uint64), solved(name)[label].view(np.uint64), err_msg=label)
        np.testing.assert_array_equal(xp.view(np.uint64), xa.view(np.uint64), err_msg=label)


# ---- GPU: the block primitives -------------------------------------------------

def dims():
    from compton2d_amd.engine import fp_fast_dims
    return fp_fast_dims()


def same_in_every_thread(v, what):
    """v [nvec, block]: bit-identical across the threads; returns thread 0's."""
    bits = np.ascontiguousarray(v).view(np.uint64 if v.dtype == np.float64 else np.uint32)
    bad = np.nonzero(np.any(bits != bits[:, :1], axis=1))[0]
    assert bad.size == 0, (what, "vector", int(bad[0]), v[bad[0]][:8])
    return v[:, 0]


ONE_HOT = (1.5, -0.0, 5e-324, 1e308)


def one_hot(bs):
    """[4 * bs, bs]: each value at each thread, zeros elsewhere."""
    v = np.zeros((len(ONE_HOT) * bs, bs))
    for q, val in enumerate(ONE_HOT):
        v[q * bs + np.arange(bs), np.arange(bs)] = val
    return v, np.repeat(ONE_HOT, bs)


@pytest.mark.gpu
def test_gpu_fp_block_sums_and_scans_one_hot():
    """One value at thread t, zeros elsewhere, for every t: nothing is rounded,
    so the sum is the value in every thread, the prefix is 0 below t and the
    value from t on, and the total has the last prefix's bits.  (-0.0 + 0.0 is
    +0.0 in IEEE arithmetic: the zero's sign is not asked for.)  Both channels
    of sum2 and scan_sum are used, the second with the threads reversed."""
    from compton2d_amd import engine as E
    bs, _ = dims()
    v, val = one_hot(bs)
    vr = np.ascontiguousarray(v[:, ::-1])
    s = E.device_fp_block(E.FP_BLK_SUM2, v, vr)
    for ch in (0, 1):
        got = same_in_every_thread(s[:, ch], "sum2 channel %d" % ch)
        np.testing.assert_array_equal(got, val, err_msg="sum2 channel %d" % ch)
    t = np.tile(np.arange(bs), len(ONE_HOT))
    want = np.where(np.arange(bs)[None, :] >= t[:, None], val[:, None], 0.0)
    for op, out in (("scan", E.device_fp_block(E.FP_BLK_SCAN, v)),
                    ("scan_sum", E.device_fp_block(E.FP_BLK_SCAN_SUM, v, vr))):
        np.testing.assert_array_equal(out[:, 0], want, err_msg=op)
        tot = same_in_every_thread(out[:, 1], op + " total")
        np.testing.assert_array_equal(tot.view(np.uint64), out[:, 0, bs - 1].view(np.uint64), err_msg=op)
        if op == "scan_sum":
            np.testing.assert_array_equal(same_in_every_thread(out[:, 2], "scan_sum w"), val)


def rounding_vectors(bs):
    rng = np.random.default_rng(7)
    big = np.where(np.arange(bs) % 2 == 0, 1e16, rng.uniform(-2.0, 2.0, bs))
    big[2::4] = -1e16
    v = [rng.uniform(-1.0, 1.0, bs), rng.uniform(0.0, 1.0, bs), rng.standard_normal(bs) * 10.0 ** rng.uniform(-8, 8, bs),
         big, big[::-1].copy(), np.full(bs, 0.1), np.full(bs, -3.0), np.full(bs, 1e-310),
         np.where(np.arange(bs) < 200, rng.uniform(0.0, 1.0, bs), 0.0)]
    return np.array(v)


@pytest.mark.gpu
def test_gpu_fp_block_sums_and_scans_round_as_counted(capsys):
    """Random, cancelling (+-1e16 between O(1) values) and all-equal vectors:
    every thread holds the same bits of each sum and total, and they lie
    within k u sum|v_j| of math.fsum over the terms that enter.  k is the
    number of additions on the longest path, counted in fp_fast.hip for a
    block of W waves: a sum takes 4 DPP steps within a row, 3 additions of
    the rows' sums (wsum) and W of the waves' partials, k = 7 + W (11 at 256
    threads); a prefix takes the 4 row-shift steps, 3 for the rows before
    (v + ((r0 + r1) + r2)), W for the waves before and 1 to combine,
    k = 8 + W (12).  The first of the W additions adds to 0.0 and is exact,
    which covers fsum's own rounding.  Measured on an MI355X: sums and totals
    1.25, prefixes 1.98 u sum|v_j|."""
    from compton2d_amd import engine as E
    bs, _ = dims()
    W = bs // 64
    ks, kp = 7 + W, 8 + W
    v = rounding_vectors(bs)
    w = np.ascontiguousarray(v[::-1])
    absum = np.array([math.fsum(np.abs(x)) for x in v])
    fs = np.array([math.fsum(x) for x in v])
    figures = {}

    def check_sum(got, ref, scale, k, what):
        err, unit = np.abs(got - ref), U * scale           # the denormal vector's unit underflows to 0
        figures[what] = max(figures.get(what, 0.0), float(np.max(err[unit > 0.0] / unit[unit > 0.0])))
        assert np.all(err <= k * unit), (what, np.argwhere(~(err <= k * unit))[:4])

    s = E.device_fp_block(E.FP_BLK_SUM2, v, w)
    check_sum(same_in_every_thread(s[:, 0], "sum2 a"), fs, absum, ks, "sum")
    check_sum(same_in_every_thread(s[:, 1], "sum2 b"), fs[::-1], absum[::-1], ks, "sum")
    for op, out in (("scan", E.device_fp_block(E.FP_BLK_SCAN, v)),
                    ("scan_sum", E.device_fp_block(E.FP_BLK_SCAN_SUM, v, w))):
        check_sum(same_in_every_thread(out[:, 1], op + " total"), fs, absum, ks, "total")
        pref = np.array([[math.fsum(x[:t + 1]) for t in range(bs)] for x in v])
        pabs = np.array([[math.fsum(np.abs(x[:t + 1])) for t in range(bs)] for x in v])
        check_sum(out[:, 0], pref, pabs, kp, "prefix")
        np.testing.assert_array_equal(out[:, 1, 0].view(np.uint64), out[:, 0, bs - 1].view(np.uint64), err_msg=op)
        if op == "scan_sum":
            check_sum(same_in_every_thread(out[:, 2], "scan_sum w"), fs[::-1], absum[::-1], ks, "sum")
    with capsys.disabled():
        print("\nblock sums, max |got - fsum| / (u sum|v|): %s (counted: sum %d, prefix %d)"
              % ({k: "%.2f" % x for k, x in figures.items()}, ks, kp))


@pytest.mark.gpu
@pytest.mark.parametrize("special", [np.inf, -np.inf, np.nan])
def test_gpu_fp_block_sums_carry_inf_and_nan_to_every_thread(special):
    """One inf or NaN among finite values, in each wave and at the wave edges:
    every thread holds the same inf or NaN (same bits)."""
    from compton2d_amd import engine as E
    bs, _ = dims()
    rng = np.random.default_rng(9)
    at = [t for t in (0, 15, 16, 63, 64, 100, 127, 128, 191, 192, bs - 1) if t < bs]
    v = rng.uniform(0.0, 1.0, (len(at), bs))
    v[np.arange(len(at)), at] = special
    w = np.ascontiguousarray(v[:, ::-1])

    def check(x, what):
        x = same_in_every_thread(x, what)
        assert np.all(np.isnan(x)) if np.isnan(special) else np.all(x == special), (what, x)

    s = E.device_fp_block(E.FP_BLK_SUM2, v, w)
    check(s[:, 0], "sum2 a")
    check(s[:, 1], "sum2 b")
    check(E.device_fp_block(E.FP_BLK_SCAN, v)[:, 1], "scan total")
    o = E.device_fp_block(E.FP_BLK_SCAN_SUM, v, w)
    check(o[:, 1], "scan_sum total")
    check(o[:, 2], "scan_sum w")
    for n, t in enumerate(at):                      # the prefix: finite below, special from t on
        assert np.all(np.isfinite(o[n, 0, :t]))
        assert np.all(np.isnan(o[n, 0, t:])) if np.isnan(special) else np.all(o[n, 0, t:] == special)


@pytest.mark.gpu
def test_gpu_fp_block_minmax_and_min2_exact():
    """Block minima and maxima of ints against numpy: random values, the
    extreme at each thread next to a wave edge, INT_MAX / INT_MIN themselves
    and all-equal vectors; the two series differ."""
    from compton2d_amd import engine as E
    bs, _ = dims()
    rng = np.random.default_rng(3)
    a = [rng.integers(INT_MIN, INT_MAX, bs, endpoint=True), rng.integers(-5, 5, bs), np.full(bs, INT_MAX),
         np.full(bs, INT_MIN), np.full(bs, 17)]
    for t in (0, 63, 64, 127, 128, 191, 192, bs - 1):
        x = rng.integers(-1000, 1000, bs)
        x[t] = -5000 if t % 2 else 5000
        a.append(x)
        y = np.full(bs, INT_MAX)
        y[t] = 4 + t                     # the kernel's use: a bin index where a test holds, INT_MAX elsewhere
        a.append(y)
    a = np.array(a, np.int32)
    b = np.ascontiguousarray(-(a[::-1].astype(np.int64) + 1)).astype(np.int32)      # differs from a
    mm = E.device_fp_block(E.FP_BLK_MINMAX, a, b)
    np.testing.assert_array_equal(same_in_every_thread(mm[:, 0], "minmax min"), a.min(axis=1))
    np.testing.assert_array_equal(same_in_every_thread(mm[:, 1], "minmax max"), b.max(axis=1))
    m2 = E.device_fp_block(E.FP_BLK_MIN2, a, b)
    np.testing.assert_array_equal(same_in_every_thread(m2[:, 0], "min2 a"), a.min(axis=1))
    np.testing.assert_array_equal(same_in_every_thread(m2[:, 1], "min2 b"), b.min(axis=1))


@pytest.mark.gpu
def test_gpu_fp_block_firsts_lowest_term_wins():
    """firsts<TPT>: term k*block + t is flag [k][t]; the lowest set term of
    each series in every thread, INT_MAX where none is set."""
    from compton2d_amd import engine as E
    bs, tpt = dims()
    cases = [[]]                                           # no flag set
    cases.append([(tpt - 1, bs - 1)])                      # only the last thread of the last k
    cases.append([(0, 0)])                                 # thread 0
    for lo in (63, 127, 191):                              # both sides of each wave edge
        for k in range(tpt):
            cases += [[(k, lo)], [(k, lo + 1)], [(k, lo), (k, lo + 1)], [(k, lo + 1), (tpt - 1, lo)]]
    cases.append([(tpt - 1, 5), (1, 200)])                 # a higher k in an earlier lane: the lower k wins
    cases.append([(1, 3), (0, bs - 1)])
    cases.append([(tpt - 1, 0), (tpt - 2, 70), (tpt - 2, 130)])
    rng = np.random.default_rng(4)
    for p in (0.001, 0.01, 0.5):
        cases.append([(k, t) for k in range(tpt) for t in range(bs) if rng.random() < p])
    fa = np.zeros((len(cases), tpt, bs), np.uint8)
    for n, c in enumerate(cases):
        for k, t in c:
            fa[n, k, t] = 1
    fb = np.ascontiguousarray(np.roll(fa, 1, axis=0)[:, :, ::-1])    # another case's flags, threads reversed

    def want(f):
        term = np.arange(tpt)[:, None] * bs + np.arange(bs)[None, :]
        return np.array([term[x != 0].min() if x.any() else INT_MAX for x in f])

    out = E.device_fp_block(E.FP_BLK_FIRSTS, fa, fb)
    assert np.any(want(fa) != want(fb))
    np.testing.assert_array_equal(same_in_every_thread(out[:, 0], "firsts a"), want(fa))
    np.testing.assert_array_equal(same_in_every_thread(out[:, 1], "firsts b"), want(fb))
