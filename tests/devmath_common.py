"""Input sets, exact references and the checks shared by tests/test_devmath_spec.py (host build of the probe, CPU tier) and
tests/test_gpu_devmath.py (gfx950 build): see tests/devmath/probe.hip.

References are exact: mpmath at 250 bits for sine, cosine (an mpf argument is reduced exactly, whatever its size), and
fractions.Fraction for reciprocals and quotients.  Errors are taken against those, never against another build.
Every set is seeded; each reference is computed once per session (functools.lru_cache) and never modified (the arrays
are made read-only).
"""
import functools
import math
from fractions import Fraction

import numpy as np

SINCOS_MEDIUM_MAX = 3.5e15          # csrc/anm_device.hpp
DBL_MAX = np.finfo(np.float64).max
SIN_BOUND = 2.0 ** -51              # absolute, paths 0-3 (derivation: test_gpu_devmath.py)


def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def report(name, value):
    """every measured figure goes to stdout before anything is asserted on it (pytest -s shows them)"""
    print("devmath: %-58s %s" % (name, ("%.4g" % value) if isinstance(value, float) else value))


# ------------------------------------------------------------------------------------------------------------------
# sine and cosine
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sincos_sets():
    """{'a'..'f': x}: see the docstring of test_gpu_devmath.py"""
    import mpmath

    rng = np.random.default_rng(20240917)
    sets = {}
    sets["a"] = np.concatenate((rng.uniform(-0.78, 0.78, 20000), [0.0, -0.0, 0.78, -0.78, 5e-324, -5e-324, 1e-300]))
    # (b) per decade from 0.78 to 3.5e15 (the last one is cut there)
    b = []
    lo = 0.78
    while lo < SINCOS_MEDIUM_MAX:
        hi = min(lo * 10.0, SINCOS_MEDIUM_MAX)
        v = np.exp(rng.uniform(np.log(lo), np.log(hi), 3000))
        b.append(np.clip(v, lo, np.nextafter(hi, 0.0)) * rng.choice([-1.0, 1.0], 3000))
        lo *= 10.0
    sets["b"] = np.concatenate(b)
    # (c), (d): multiples and half-odd multiples of pi/2; k = 1..1999 and 3 000 random k < 2^50 (log-uniform, so that
    # every binade of the quotient is visited)
    ks = np.concatenate((np.arange(1, 2000), np.floor(2.0 ** rng.uniform(11, 50, 3000)))).astype(np.int64)
    with mpmath.workprec(250):
        h = mpmath.pi / 2
        near = np.array([float(int(k) * h) for k in ks])                      # float(mpf) rounds to nearest
        tie = np.array([float((int(k) + mpmath.mpf(0.5)) * h) for k in ks])
    assert near.max() < SINCOS_MEDIUM_MAX and tie.max() < SINCOS_MEDIUM_MAX
    c = np.concatenate((near, np.nextafter(near, 0.0), np.nextafter(near, np.inf)))
    sets["c"] = np.concatenate((c, -c))
    sets["d"] = np.concatenate((tie, -tie))
    e = np.array([np.nextafter(SINCOS_MEDIUM_MAX, 0.0), 2.0 ** 51, 1.5 * 2.0 ** 51])
    sets["e"] = np.concatenate((e, -e))
    f = np.exp(rng.uniform(np.log(SINCOS_MEDIUM_MAX), np.log(1e300), 3000)) * rng.choice([-1.0, 1.0], 3000)
    sets["f"] = np.concatenate((f, [SINCOS_MEDIUM_MAX, DBL_MAX, -DBL_MAX, np.inf, -np.inf, np.nan]))
    return {k: _ro(v) for k, v in sets.items()}


def _exact_sincos(x):
    """sin and cos of every finite x as double-double (hi, lo) pairs: hi + lo is exact to ~2^-106 relative"""
    import mpmath

    out = np.zeros((4, x.size))
    with mpmath.workprec(250):
        for i, v in enumerate(x):
            if not np.isfinite(v):
                out[:, i] = np.nan
                continue
            m = mpmath.mpf(float(v))
            c, s = mpmath.cos_sin(m)
            sh, ch = float(s), float(c)
            out[0, i], out[1, i], out[2, i], out[3, i] = sh, float(s - sh), ch, float(c - ch)
    return out


@functools.lru_cache(maxsize=None)
def sincos_reference(name):
    return _ro(_exact_sincos(sincos_sets()[name]))


def sincos_abs_error(name, s, c):
    """max |s - sin x|, max |c - cos x| over the finite x of set `name` (s - hi is exact when they are close)"""
    sh, sl, ch, cl = sincos_reference(name)
    fin = np.isfinite(sincos_sets()[name])
    es = np.abs((s - sh) - sl)[fin]
    ec = np.abs((c - ch) - cl)[fin]
    assert not np.isnan(es).any() and not np.isnan(ec).any(), "NaN for a finite argument in set (%s)" % name
    return float(es.max()), float(ec.max())


def sincos_ulp_error(name, s, c):
    """the same in units of the last place of the exact value"""
    sh, sl, ch, cl = sincos_reference(name)
    fin = np.isfinite(sincos_sets()[name])
    es = (np.abs((s - sh) - sl) / np.spacing(np.abs(sh)))[fin]
    ec = (np.abs((c - ch) - cl) / np.spacing(np.abs(ch)))[fin]
    assert not np.isnan(es).any() and not np.isnan(ec).any(), "NaN for a finite argument in set (%s)" % name
    return float(es.max()), float(ec.max())


def check_sincos(probe, tag):
    """Conditions 1-4 on one build of the probe; returns {(path, set): (sin, cos)} for cross-build comparisons."""
    sets = sincos_sets()
    got = {}
    for name in "abcde":
        for path in range(4):
            got[path, name] = probe.sincos(path, sets[name])
    # 1. a small step through the reduction: (d, quadrant 0) exactly, i.e. the bits of the short path
    for long, short in ((2, 0), (3, 1)):
        for k in (0, 1):
            n_diff = int((bits(got[long, "a"][k]) != bits(got[short, "a"][k])).sum())
            report("%s (a) path %d != path %d, %s: count" % (tag, long, short, "sc"[k]), n_diff)
            assert n_diff == 0
    # 2. the interleaved asm statement issues the same two Horner chains
    for name in "abcde":
        for vc, plain in ((1, 0), (3, 2)):
            n_diff = sum(int((bits(got[vc, name][k]) != bits(got[plain, name][k])).sum()) for k in (0, 1))
            report("%s (%s) path %d != path %d: count" % (tag, name, vc, plain), n_diff)
            assert n_diff == 0
    # 3. against mpmath.  Paths 2, 3 on (a)-(e); paths 0, 1 on (a), the domain of the bare kernels (they reduce nothing:
    # beyond pi/4 they are compared bit for bit above, not against the sine)
    worst = {}
    for name in "abcde":
        for path in (range(4) if name == "a" else (2, 3)):
            es, ec = sincos_abs_error(name, *got[path, name])
            report("%s (%s) path %d: max |sin err|, |cos err|" % (tag, name, path), "%.4g  %.4g" % (es, ec))
            worst[path, name] = max(es, ec)
    for key, w in worst.items():
        assert w <= SIN_BOUND, (key, w)
    return got


def check_sincos_huge(probe, tag):
    x = sincos_sets()["f"]
    s, c = probe.sincos(4, x)
    fin = np.isfinite(x)
    es, ec = sincos_ulp_error("f", s, c)
    report("%s (f) path 4: max sin, cos error in ulp" % tag, "%.4g  %.4g" % (es, ec))
    assert np.isnan(s[~fin]).all() and np.isnan(c[~fin]).all()
    assert es <= 4.0 and ec <= 4.0    # OpenCL's bound for double sin / cos
    return s, c


# ------------------------------------------------------------------------------------------------------------------
# reciprocals and quotients
# ------------------------------------------------------------------------------------------------------------------
def _magnitudes(rng, lo, hi, n_uniform):
    """log-uniform magnitudes in [lo, hi] with random sign; every power of two in that range; 1 +- 1 ulp; 1 000 values
    within 8 ulp of powers of two"""
    x = np.exp(rng.uniform(np.log(lo), np.log(hi), n_uniform)) * rng.choice([-1.0, 1.0], n_uniform)
    e_lo, e_hi = math.ceil(math.log2(lo)), math.floor(math.log2(hi))
    pw = 2.0 ** np.arange(e_lo, e_hi + 1)
    near = 2.0 ** rng.integers(e_lo + 1, e_hi, 1000)
    k = rng.integers(-8, 9, 1000)
    near = near.view(np.int64) + k   # k ulp away (below a power of two the ulp is half as large: still within 8)
    near = near.view(np.float64) * rng.choice([-1.0, 1.0], 1000)
    return np.concatenate((x, pw, -pw, [1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)], near))


@functools.lru_cache(maxsize=None)
def recip_inputs():
    return _ro(_magnitudes(np.random.default_rng(11), 1e-290, 1e290, 100000))


def _split(v):
    m, e = math.frexp(v)
    return int(m * 9007199254740992.0), e - 53        # v = mantissa * 2^exponent, exactly


def recip_rel_error(x, r):
    """max |r x - 1| = |r - 1/x| / |1/x|, exactly (Fraction), over finite normal x and r"""
    wn, wd = 0, 1                                     # the worst error so far as the fraction wn / wd
    for xv, rv in zip(x.tolist(), r.tolist()):
        assert math.isfinite(rv), (xv, rv)
        mx, ex = _split(xv)
        mr, er = _split(rv)
        sh = -(ex + er)                               # r x = mx mr / 2^sh
        assert sh > 0, (xv, rv)
        n, d = abs(mx * mr - (1 << sh)), 1 << sh
        if n * wd > wn * d:
            wn, wd = n, d
    return float(Fraction(wn, wd))


@functools.lru_cache(maxsize=None)
def blk_inputs():
    """2 000 random blocks {a, b, c, d} with |det| >= 1e-3 |m|^2 (Frobenius), each at a scale of its own"""
    rng = np.random.default_rng(12)
    m = rng.normal(size=(4000, 4)) * 10.0 ** rng.uniform(-3, 3, size=(4000, 1))
    det = m[:, 0] * m[:, 3] - m[:, 1] * m[:, 2]
    ok = np.abs(det) >= 1.001e-3 * (m * m).sum(axis=1)
    m = m[ok][:2000]
    assert m.shape[0] == 2000
    return _ro(m)


def blk_inv_rel_error(m, inv):
    """Largest relative distance of an entry of `inv` from the exact {d, -b, -c, a} / det, det = fl(a d - fl(b c)): the
    determinant as blk_inv rounds it (one product, one fma), its inverse exact."""
    worst = Fraction(0)
    for (a, b, c, d), got in zip(m.tolist(), inv.tolist()):
        bc = b * c                                                       # IEEE product
        det = float(Fraction(a) * Fraction(d) - Fraction(bc))            # fma: one rounding (float(Fraction) rounds to nearest)
        for num, g in zip((d, -b, -c, a), got):
            exact = Fraction(num) / Fraction(det)
            err = abs(Fraction(g) - exact) / abs(exact)
            if err > worst:
                worst = err
    return float(worst)


RECIP_SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** 1022 * 1.5, -(2.0 ** 1022) * 1.5, 2.0 ** 1023, DBL_MAX,
                           -DBL_MAX])  # fmt: skip
RECIP_SUBNORMALS = np.array([5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072009e-308, -2.2250738585072009e-308])


def recip_specials_table(xs, r):
    """['x -> r  (IEEE | NaN | OTHER: IEEE gives v)'] for the inputs xs and whether every row is IEEE or NaN"""
    with np.errstate(divide="ignore", over="ignore", under="ignore"):
        ieee = 1.0 / xs
    rows, ok = [], True
    for x, want, got in zip(xs, ieee, r):
        same = bits(np.array([got]))[0] == bits(np.array([want]))[0] or (np.isnan(got) and np.isnan(want))
        kind = "IEEE" if same else ("NaN" if np.isnan(got) else "OTHER: IEEE gives %r" % float(want))
        ok = ok and not kind.startswith("OTHER")
        rows.append("%-24r -> %-24r %s" % (float(x), float(got), kind))
    return rows, ok


DIVISORS = (100.0, 1.0, 10.0, 3.0, 7.5, 1e-3, 1e3)


@functools.lru_cache(maxsize=None)
def div_by_inputs():
    """(x, d): for every divisor the reciprocal set's construction scaled into [1e-6, 1e6] -- 20 000 log-uniform values,
    the powers of two, 1 +- 1 ulp, 1 000 values next to powers of two (7 x ~21 000 elements, one launch)"""
    x = _magnitudes(np.random.default_rng(13), 1e-6, 1e6, 20000)
    return _ro(np.tile(x, len(DIVISORS))), _ro(np.repeat(DIVISORS, x.size))


def quotient_ulp_error(num, den, q):
    """(max |q - num/den| in ulp of the exact quotient, number of q that are not the correctly rounded quotient)"""
    worst, n_wrong = Fraction(0), 0
    for nv, dv, qv in zip(num.tolist(), den.tolist(), q.tolist()):
        assert math.isfinite(qv), (nv, dv, qv)
        exact = Fraction(nv) / Fraction(dv)
        rounded = float(exact)                                           # correctly rounded
        if qv != rounded:
            n_wrong += 1
            err = abs(Fraction(qv) - exact) / Fraction(math.ulp(rounded))
            if err > worst:
                worst = err
    # (a correctly rounded q is within half an ulp: only the others need the exact distance)
    return (float(worst) if n_wrong else 0.5), n_wrong


def check_div_by(probe, tag):
    x, d = div_by_inputs()
    q = probe.div_by(x, d)
    err, n_wrong = quotient_ulp_error(x, d, q)
    report("%s div_by: max error in ulp (0.5: all correctly rounded)" % tag, err)
    report("%s div_by: not correctly rounded, of %d" % (tag, x.size), n_wrong)
    assert err <= 1.0
    for dv in DIVISORS:
        sx = np.array([0.0, -0.0, np.inf, -np.inf, np.nan])
        got = probe.div_by(sx, dv)
        assert got[0] == 0.0 and not np.signbit(got[0]) and got[1] == 0.0 and np.signbit(got[1]), (dv, got)
        assert got[2] == np.inf and got[3] == -np.inf, (dv, got)          # "an infinite potential must stay +inf"
        assert np.isnan(got[4]), (dv, got)
    return n_wrong


@functools.lru_cache(maxsize=None)
def dump_div_inputs():
    rng = np.random.default_rng(14)
    n = 100000
    return (_ro(rng.normal(size=n) * 10.0 ** rng.uniform(-6, 6, size=n)),
            _ro(rng.normal(size=n) * 10.0 ** rng.uniform(-6, 6, size=n)))


def check_dump_div(probe, tag):
    num, den = dump_div_inputs()
    err, n_wrong = quotient_ulp_error(num, den, probe.dump_div(num, den))
    report("%s dump_div: max error in ulp (0.5: all correctly rounded)" % tag, err)
    report("%s dump_div: not correctly rounded, of %d" % (tag, num.size), n_wrong)
    assert err <= 1.0


def check_dump_abs_arg(probe, tag):
    """test_hostsim_parity.py::test_dump_abs_and_arg_against_numpy on this build: the same generator, edge cases, signed
    zeros and bounds (2e-15 absolute on the angle, 1e-15 relative on the magnitude); 2e5 elements instead of 4e5."""
    rng = np.random.default_rng(7)
    n = 200000 - 15
    x = rng.normal(size=n) * 10.0 ** rng.uniform(-6, 6, size=n)
    y = rng.normal(size=n) * 10.0 ** rng.uniform(-6, 6, size=n)
    edge = np.array([[1, 0], [-1, 0], [0, 1], [0, -1], [0, 0], [1, 1], [-1, -1], [-1, 1], [1, -1], [1e-300, 1e-300], [3, 4],
                     [np.tan(np.pi / 8), 1.0], [1.0, np.tan(np.pi / 8)], [np.nan, 1.0], [1.0, np.nan]], dtype=float)  # fmt: skip
    x = np.concatenate((x, edge[:, 0]))
    y = np.concatenate((y, edge[:, 1]))
    mag, ang = probe.dump_abs_arg(x, y)
    z = x + 1j * y
    fin = np.isfinite(x) & np.isfinite(y)
    e_ang = float(np.max(np.abs(ang[fin] - np.angle(z[fin]))))
    big = fin & (np.maximum(np.abs(x), np.abs(y)) > 1e-150)   # (per-unit quantities: |z| is formed without scaling against underflow)
    e_mag = float(np.max(np.abs(mag[big] / np.abs(z[big]) - 1.0)))
    report("%s dump_arg: max |angle - np.angle|" % tag, e_ang)
    report("%s dump_abs: max relative distance from np.abs" % tag, e_mag)
    assert e_ang < 2e-15
    np.testing.assert_allclose(mag[big], np.abs(z[big]), rtol=1e-15, atol=0)
    assert np.isnan(ang[~fin]).all() and np.isnan(mag[~fin]).all()
    # zeros, signs included: np.angle / np.arctan2 distinguish (+0, +-0) -> +-0 from (-0, +-0) -> +-pi
    xs = np.array([0.0, 0.0, -0.0, -0.0, -0.0, 0.0])
    ys = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0])
    _, a2 = probe.dump_abs_arg(xs, ys)
    ref = np.arctan2(ys, xs)
    np.testing.assert_array_equal(a2, ref)
    np.testing.assert_array_equal(np.signbit(a2), np.signbit(ref))


def check_dump_arg_subnormal_axis(probe, tag):
    """the last two inputs of test_dump_abs_and_arg_against_numpy: (+-5e-324, 0) -> 0, pi"""
    xs, ys = np.array([5e-324, -5e-324]), np.array([0.0, 0.0])
    _, a2 = probe.dump_abs_arg(xs, ys)
    report("%s dump_arg(0, +-5e-324)" % tag, "%r %r" % (float(a2[0]), float(a2[1])))
    ref = np.arctan2(ys, xs)
    np.testing.assert_array_equal(a2, ref)
    np.testing.assert_array_equal(np.signbit(a2), np.signbit(ref))
    # off the axes, one or both components subnormal: the bound of the plane (2e-15 absolute)
    xs = np.array([3e-320, -5e-320, 1e-310, -2e-309, 5e-324, 2.2250738585072009e-308, 1e-300, -4e-308])
    ys = np.array([5e-320, 3e-320, -2e-309, -1e-310, 5e-324, -5e-324, 3e-315, 2.5e-308])
    _, a3 = probe.dump_abs_arg(xs, ys)
    e = float(np.max(np.abs(a3 - np.arctan2(ys, xs))))
    report("%s dump_arg, subnormal components: max |angle - np.arctan2|" % tag, e)
    assert e < 2e-15


def check_max_min(probe, tag):
    rng = np.random.default_rng(15)
    a = rng.normal(size=10000) * 10.0 ** rng.uniform(-6, 6, size=10000)
    b = rng.normal(size=10000) * 10.0 ** rng.uniform(-6, 6, size=10000)
    b[:500] = a[:500]                                            # equal operands too
    mx, mn = probe.max_min(a, b)
    assert (bits(mx) == bits(np.fmax(a, b))).all() and (bits(mn) == bits(np.fmin(a, b))).all()
    inf, nan = np.inf, np.nan
    sa = np.array([nan, 2.5, nan, -3.0, inf, -inf, inf, 1.0, -inf, 1.0, nan, inf, nan, -inf])
    sb = np.array([2.5, nan, -3.0, nan, -inf, inf, 1.0, inf, 1.0, -inf, inf, nan, -inf, nan])
    mx, mn = probe.max_min(sa, sb)
    assert (bits(mx) == bits(np.fmax(sa, sb))).all() and (bits(mn) == bits(np.fmin(sa, sb))).all()   # a NaN is dropped
    mx, mn = probe.max_min(np.array([nan]), np.array([nan]))
    assert np.isnan(mx[0]) and np.isnan(mn[0])
    # (+0, -0): recorded, not asserted (fmax / fmin may return either)
    mx, mn = probe.max_min(np.array([0.0, -0.0]), np.array([-0.0, 0.0]))
    sign = lambda v: "-0" if np.signbit(v) else "+0"  # noqa: E731
    report("%s vmax(+0,-0), vmax(-0,+0), vmin(+0,-0), vmin(-0,+0)" % tag, " ".join(map(sign, (mx[0], mx[1], mn[0], mn[1]))))
    assert (mx == 0.0).all() and (mn == 0.0).all()
