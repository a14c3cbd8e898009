"""Test-only loader of tests/devmath/probe.hip: the scalar arithmetic of csrc/anm_device.hpp / csrc/anm_group.hpp, one call
per element.

``device_probe()`` is the hipcc build for gfx950 with exactly the flags of the stock libraries (the device branches of the
two headers, run on cuda:0); ``host_probe()`` is the g++ build of the same file (the host branches, plain loops).  Both give
a :class:`Probe` whose methods take and return NumPy arrays.  The product never imports this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from gym_anm_amd import codegen

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "devmath", "probe.hip")
OUT = os.path.join(HERE, "devmath", "_build")
_CACHE = {}

_P = C.c_void_p
_SIGS = {  # name: number of pointer arguments (after the leading int64 count; a stream follows)
    "anm_probe_recip": 2, "anm_probe_rcp": 2, "anm_probe_blk_inv": 2, "anm_probe_blk_inv_fast": 2, "anm_probe_div_by": 3,
    "anm_probe_dump_div": 3, "anm_probe_dump_abs_arg": 4, "anm_probe_max_min": 4,
}  # fmt: skip


def _build(lib, cmd):
    os.makedirs(OUT, exist_ok=True)
    srcs = [SRC] + [os.path.join(codegen.CSRC, f) for f in os.listdir(codegen.CSRC) if f.endswith(".hpp")]
    newest = max(os.path.getmtime(p) for p in srcs)
    if not os.path.exists(lib) or os.path.getmtime(lib) < newest:
        tmp = "%s.tmp%d" % (lib, os.getpid())
        res = subprocess.run(cmd + ["-I", codegen.CSRC, SRC, "-o", tmp], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("building %s failed:\n%s" % (os.path.basename(lib), res.stderr[-4000:]))
        os.replace(tmp, lib)
    return C.CDLL(lib)


class Probe:
    """One build of the probe.  Arrays in, arrays out (float64, C order); on the device build the arrays go through cuda:0
    and the launch runs on torch's current stream."""

    def __init__(self, lib):
        self.lib = lib
        lib.anm_probe_is_device.restype, lib.anm_probe_is_device.argtypes = C.c_int, []
        self.on_device = bool(lib.anm_probe_is_device())
        lib.anm_probe_sincos.restype = C.c_int
        lib.anm_probe_sincos.argtypes = [C.c_int, C.c_int64, _P, _P, _P, _P]
        for name, n_ptr in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = C.c_int, [C.c_int64] + [_P] * (n_ptr + 1)

    def _call(self, name, n, ins, out_shapes, lead=()):
        ins = [np.ascontiguousarray(a, dtype=np.float64) for a in ins]
        fn = getattr(self.lib, name)
        if not self.on_device:
            outs = [np.full(s, np.nan) for s in out_shapes]
            rc = fn(*lead, n, *[a.ctypes.data for a in ins + outs], None)
            assert rc == 0, "%s returned %d" % (name, rc)
            return outs
        import torch

        d_in = [torch.from_numpy(np.array(a)).to("cuda:0") for a in ins]      # (np.array: a writable copy)
        d_out = [torch.full(tuple(s) if not np.isscalar(s) else (s,), float("nan"), dtype=torch.float64, device="cuda:0")
                 for s in out_shapes]  # fmt: skip
        rc = fn(*lead, n, *[t.data_ptr() for t in d_in + d_out], torch.cuda.current_stream().cuda_stream)
        assert rc == 0, "%s returned HIP error %d" % (name, rc)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in d_out]

    def sincos(self, path, x):
        """(sin, cos) by path 0/1: sincos_kernel<false/true>(x, 0); 2/3: sincos_medium<false/true>; 4: sincos_huge"""
        x = np.asarray(x, dtype=np.float64)
        return self._call("anm_probe_sincos", x.size, [x], [x.size, x.size], lead=(int(path),))

    def rcp(self, x):
        return self._call("anm_probe_rcp", np.size(x), [x], [np.size(x)])[0]

    def recip(self, x):
        return self._call("anm_probe_recip", np.size(x), [x], [np.size(x)])[0]

    def blk_inv(self, m, fast=False):
        """m: [n, 4] blocks {a, b, c, d}; fast: group::blk_inv_fast (device build only)"""
        m = np.asarray(m, dtype=np.float64)
        assert m.ndim == 2 and m.shape[1] == 4
        return self._call("anm_probe_blk_inv_fast" if fast else "anm_probe_blk_inv", m.shape[0], [m], [m.shape])[0]

    def div_by(self, x, d):
        """div_by(x, make_recip(d)), elementwise"""
        x, d = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(d, dtype=np.float64))
        return self._call("anm_probe_div_by", x.size, [x, d], [x.size])[0]

    def dump_div(self, num, den):
        return self._call("anm_probe_dump_div", np.size(num), [num, den], [np.size(num)])[0]

    def dump_abs_arg(self, x, y):
        """(dump_abs(x, y), dump_arg(y, x))"""
        return self._call("anm_probe_dump_abs_arg", np.size(x), [x, y], [np.size(x)] * 2)

    def max_min(self, a, b):
        """(vmax(a, b), vmin(a, b))"""
        return self._call("anm_probe_max_min", np.size(a), [a, b], [np.size(a)] * 2)


def host_probe():
    """The host branches: g++ with the flags of the host test double (tests/hostsim_backend.py)."""
    if "host" not in _CACHE:
        lib = os.path.join(OUT, "libdevmath_probe_host.so")
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-x", "c++"]
        _CACHE["host"] = Probe(_build(lib, cmd))
        assert not _CACHE["host"].on_device
    return _CACHE["host"]


def device_probe():
    """The device branches: hipcc for gfx950 with exactly the flags of the stock libraries (codegen.HIPCC_FLAGS)."""
    if "device" not in _CACHE:
        hipcc = codegen.hipcc_path()
        if hipcc is None:
            raise RuntimeError("hipcc not found: the device probe cannot be built")
        lib = os.path.join(OUT, "libdevmath_probe_gfx950.so")
        _CACHE["device"] = Probe(_build(lib, [hipcc] + list(codegen.HIPCC_FLAGS)))
        assert _CACHE["device"].on_device
    return _CACHE["device"]
