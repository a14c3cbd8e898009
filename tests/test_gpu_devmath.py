"""GPU tier: the device-only arithmetic of csrc/anm_device.hpp and csrc/anm_group.hpp, function by function, against
exact references (tests/devmath/probe.hip built for gfx950 with the flags of the stock libraries; tests/devmath_common.py
holds the input sets, the references and the checks, which tests/test_devmath_spec.py runs on the host build too).

Every `#if defined(__HIP_DEVICE_COMPILE__)` branch of the two headers has a different `#else` for the host test double, and
the transitions of the rest of the GPU tier allow 1e-12 on injections, 1e-9 on the state and 2 eps cond(J) on diverging
solves: a range reduction that is 1e-10 off or a reciprocal good to 40 bits passes all of them.  Here each function is one
launch over <= 2e5 elements.

Sine and cosine: paths 0/1 = sincos_kernel<false/true>(x, 0), 2/3 = sincos_medium<false/true>, 4 = sincos_huge.  Sets:
  (a) 20 000 uniform in [-0.78, 0.78], +-0, +-0.78, +-5e-324, 1e-300            (the steps of a converging solve)
  (b) 3 000 log-uniform per decade from 0.78 to 3.5e15, random sign
  (c) the doubles nearest k pi/2 and both neighbours, k = 1..1999 and 3 000 random k < 2^50, both signs
  (d) the doubles nearest (k + 1/2) pi/2 for the same k: the quotients at the rounding tie
  (e) the predecessor of 3.5e15, 2^51, 1.5 * 2^51, both signs
  (f) path 4: 3 000 log-uniform in [3.5e15, 1e300], 3.5e15, +-DBL_MAX, +-inf, NaN
The bound on paths 0-3, 2^-51 absolute: the fdlibm kernels are below 1 ulp of a value <= 1, i.e. 2^-52; the reduced
argument carries at most two roundings at |r| < 1 after the second stage, 2^-53 each; the error of the constants P1 + P2 +
P3 times the largest quotient 2.2e15 is below 1e-33.  Paths 0 and 1 reduce nothing, so they are held to it on (a), their
domain; on (b)-(e) they are compared bit for bit with each other and with the host build (no overflow occurs below 3.5e15:
every intermediate is finite).  Path 4: 4 ulp, the OpenCL bound for double sin / cos that ocml is built to.

Measured on an MI355X: profiles/devmath_probe.txt."""
import numpy as np
import pytest

import devmath_common as dc
from devmath_probe import device_probe, host_probe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    p = device_probe()
    assert p.on_device and "tests/devmath/_build/libdevmath_probe_gfx950" in p.lib._name
    return p


@pytest.fixture(scope="module")
def rcp_e0(probe):
    """the largest relative error of the raw v_rcp_f64 estimate: a property of the hardware, measured, not asserted"""
    x = dc.recip_inputs()
    e0 = dc.recip_rel_error(x, probe.rcp(x))
    dc.report("gfx950 v_rcp_f64: max relative error e0", e0)
    dc.report("gfx950 v_rcp_f64: bits", -np.log2(e0))
    return e0


def test_sincos_paths_bitwise_and_against_mpmath(probe):
    """1. on (a) the reduction returns (d, quadrant 0) exactly: paths 2, 3 give the bits of paths 0, 1 (update_angles sends
    every lane of a wavefront through the reduction when one lane needs it, and the three lane-group loops do the same).
    2. on (a)-(e) the interleaved asm statement (VCOEF) gives the bits of the C++ Horner chains, and paths 0 and 2 give the
    bits of the host build.  3. on (a)-(e) within 2^-51 of mpmath."""
    got = dc.check_sincos(probe, "gfx950")
    host = host_probe()
    for name in "abcde":
        x = dc.sincos_sets()[name]
        for path in (0, 2):
            hs, hc = host.sincos(path, x)
            n_diff = int((dc.bits(got[path, name][0]) != dc.bits(hs)).sum() + (dc.bits(got[path, name][1]) != dc.bits(hc)).sum())
            dc.report("gfx950 (%s) path %d != host build: count" % (name, path), n_diff)
            assert n_diff == 0


def test_sincos_huge_against_mpmath(probe):
    """4. ocml's sincos beyond 3.5e15: finite arguments within 4 ulp of the exact value, non-finite ones give NaN"""
    dc.check_sincos_huge(probe, "gfx950")


def test_recip_and_blk_inv_fast_against_fraction(probe, rcp_e0):
    """recip: two Newton steps square the estimate's error twice, the last fma and multiply round once each:
    <= e0^4 + 2^-51.  blk_inv_fast on {x, 0, 0, 1} (its .a is the reciprocal of x): one step, <= e0^2 + 2^-51."""
    x = dc.recip_inputs()
    e2 = dc.recip_rel_error(x, probe.recip(x))
    dc.report("gfx950 recip: max relative error", e2)
    dc.report("gfx950 recip: bits", -np.log2(e2))
    m = np.zeros((x.size, 4))
    m[:, 0], m[:, 3] = x, 1.0
    inv = probe.blk_inv(m, fast=True)
    e1 = dc.recip_rel_error(x, inv[:, 0])
    dc.report("gfx950 blk_inv_fast: max relative error", e1)
    dc.report("gfx950 blk_inv_fast: bits", -np.log2(e1))
    assert e2 <= rcp_e0 ** 4 + 2.0 ** -51
    assert e1 <= rcp_e0 ** 2 + 2.0 ** -51
    assert (inv[:, 1] == 0.0).all() and (inv[:, 2] == 0.0).all()


def test_blk_inv_against_fraction(probe):
    """every entry within 2^-50 relative of the exact entry times the exact inverse of the ROUNDED determinant"""
    m = dc.blk_inputs()
    e = dc.blk_inv_rel_error(m, probe.blk_inv(m))
    dc.report("gfx950 blk_inv: max relative error of an entry", e)
    assert e <= 2.0 ** -50


def test_recip_special_values(probe):
    """+-0, +-inf, NaN, |x| > 2^1022: the IEEE value or NaN (a singular pivot is a diverged solve either way).  Measured:
    +-0 and +-inf give NaN, NaN gives NaN, |x| > 2^1022 the IEEE (subnormal) reciprocal."""
    rows, ok = dc.recip_specials_table(dc.RECIP_SPECIALS, probe.recip(dc.RECIP_SPECIALS))
    for r in rows:
        dc.report("gfx950 recip", r)
    assert ok, rows


def test_recip_subnormal_values(probe):
    """Subnormal x: the IEEE value or NaN.  recip returns NaN for every subnormal x, by a select on the high word of its
    result.  Without it v_rcp_f64 gives inf below 2^-1024 and the Newton step r (2 - x r) = inf (2 - inf) turned that into
    -inf: recip(5e-324) = recip(1e-310) = -inf, an infinity of the WRONG sign, neither 1 / x nor NaN, which is what this
    test found on an MI355X; and the largest subnormal, whose reciprocal is an ordinary number, came out one ulp off."""
    rows, ok = dc.recip_specials_table(dc.RECIP_SUBNORMALS, probe.recip(dc.RECIP_SUBNORMALS))
    for r in rows:
        dc.report("gfx950 recip", r)
    assert ok, rows


def test_div_by_against_fraction(probe):
    """finite quotients within 1 ulp; zeros keep their sign; +inf -> +inf, -inf -> -inf, NaN -> NaN"""
    dc.check_div_by(probe, "gfx950")


def test_dump_div_against_fraction(probe):
    dc.check_dump_div(probe, "gfx950")


def test_dump_abs_and_arg_against_numpy(probe):
    """test_hostsim_parity.py::test_dump_abs_and_arg_against_numpy with dump_div inside: the plane, the axes, the origin,
    NaNs and the signed zeros (its two subnormal inputs: the next test)"""
    dc.check_dump_abs_arg(probe, "gfx950")


def test_dump_arg_on_a_subnormal_axis(probe):
    """The last two inputs of test_dump_abs_and_arg_against_numpy, (x, y) = (+-5e-324, 0): np.arctan2 gives 0 and pi.
    dump_arg scales magnitudes below 2^-900 by 2^200 before it divides.  Without that both came back NaN on an MI355X:
    dump_div(0, 5e-324) starts from v_rcp_f64(5e-324) = inf, and 0 * inf is NaN (the host build divides exactly)."""
    dc.check_dump_arg_subnormal_axis(probe, "gfx950")


def test_vmax_vmin_like_fmax_fmin(probe):
    dc.check_max_min(probe, "gfx950")
