"""CPU tier: the HOST build of tests/devmath/probe.hip (the `#else` branches of csrc/anm_device.hpp) against exact
references, on the input sets of tests/test_gpu_devmath.py.

For the minimax kernels and reduce_medium (paths 0-3) the arithmetic is IEEE fma / rint / multiply in a fixed order, the
same on the host and on the GPU, so this file already pins the two polynomials and the two-stage reduction -- their
coefficients, the constants P1..P3, the quadrant bits -- without a GPU.  The reciprocal and quotient functions are the plain
IEEE operations here; they are run so that the shared checks (tests/devmath_common.py) are themselves exercised in this
tier, and so that test_gpu_devmath.py has the host bits to compare with."""
import numpy as np

import devmath_common as dc
from devmath_probe import device_probe, host_probe


def test_both_probe_builds_compile():
    """the g++ host build and the gfx950 cross-compile with the flags of the stock libraries (no GPU needed to build);
    the entry points that exist only on the device say so on the host"""
    assert not host_probe().on_device
    assert device_probe().on_device
    assert host_probe().lib.anm_probe_rcp(0, None, None, None) == -1
    assert host_probe().lib.anm_probe_blk_inv_fast(0, None, None, None) == -1


def test_sincos_paths_against_mpmath():
    """Conditions 1-3 of test_gpu_devmath.py on the host build: small steps come out of the reduction with the bits of the
    short path; the VCOEF instantiations (plain C++ here) equal the others; every path is within 2^-51 of mpmath.
    Measured on the host: 1.9e-16 at most."""
    dc.check_sincos(host_probe(), "host")


def test_sincos_huge_against_mpmath():
    dc.check_sincos_huge(host_probe(), "host")


def test_recip_and_blk_inv_host_are_ieee():
    p = host_probe()
    x = dc.recip_inputs()
    e = dc.recip_rel_error(x, p.recip(x))
    dc.report("host recip: max relative error", e)
    assert e <= 2.0 ** -53                       # the correctly rounded reciprocal
    m = dc.blk_inputs()
    eb = dc.blk_inv_rel_error(m, p.blk_inv(m))
    dc.report("host blk_inv: max relative error of an entry", eb)
    assert eb <= 2.0 ** -50
    for xs in (dc.RECIP_SPECIALS, dc.RECIP_SUBNORMALS):
        rows, ok = dc.recip_specials_table(xs, p.recip(xs))
        assert ok, rows


def test_quotients_host_are_ieee():
    p = host_probe()
    assert dc.check_div_by(p, "host") == 0       # x / d: correctly rounded everywhere
    dc.check_dump_div(p, "host")


def test_dump_abs_arg_and_max_min_host():
    p = host_probe()
    dc.check_dump_abs_arg(p, "host")
    dc.check_dump_arg_subnormal_axis(p, "host")
    dc.check_max_min(p, "host")
    x = np.array([1.0, -2.0])
    assert (p.max_min(x, x[::-1])[0] == 1.0).all()
