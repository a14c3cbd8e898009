// probe.hip -- TEST ONLY: the scalar arithmetic of csrc/anm_device.hpp and csrc/anm_group.hpp, one call per element.
//
// The step kernels carry arithmetic that exists only in the gfx950 build (every `#if defined(__HIP_DEVICE_COMPILE__)`
// branch of the two headers has a different `#else` for the host test double), and the suite sees it only through
// whole transitions.  This file includes the two headers unchanged and wraps each such function in an elementwise
// kernel -- one thread per element, plain loads and stores, no LDS -- behind an extern "C" launcher that takes device
// pointers, a count and a stream, so that tests/test_gpu_devmath.py can compare each function with an exact reference.
//
// The same file compiles with g++ (tests/devmath_probe.py: host_probe) into plain loops over the same functions, i.e.
// over the HOST branches; tests/test_devmath_spec.py runs that build in the CPU tier.  Entry points that exist only on
// the device (the raw reciprocal estimate, group::blk_inv_fast) return -1 there.
//
// Nothing here is part of the product or of the C ABI (include/anm_mi355x.h).
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PROBE_D __device__ __forceinline__
#endif

#include "anm_device.hpp"
#include "anm_group.hpp"

namespace {

// ---- one functor per probed function: operator()(i, pointers...) handles element i ----
template <int PATH>
struct OpSinCos {   // 0/1: sincos_kernel<false/true>(x, 0)   2/3: sincos_medium<false/true>   4: sincos_huge
  ANM_HD void operator()(int64_t i, const double* x, double* s, double* c) const {
    double sn, cs;
    if constexpr (PATH == 0) anm::sincos_kernel<false>(x[i], 0, sn, cs);
    else if constexpr (PATH == 1) anm::sincos_kernel<true>(x[i], 0, sn, cs);
    else if constexpr (PATH == 2) anm::sincos_medium<false>(x[i], sn, cs);
    else if constexpr (PATH == 3) anm::sincos_medium<true>(x[i], sn, cs);
    else {
      const anm::SinCos r = anm::sincos_huge(x[i]);
      sn = r.s;
      cs = r.c;
    }
    s[i] = sn;
    c[i] = cs;
  }
};
struct OpRecip {
  ANM_HD void operator()(int64_t i, const double* x, double* out) const { out[i] = anm::recip(x[i]); }
};
struct OpBlkInv {   // blocks as {a, b, c, d} rows of four doubles
  ANM_HD void operator()(int64_t i, const double* m, double* out) const {
    const anm::Blk<double> r = anm::blk_inv(anm::Blk<double>{m[4 * i], m[4 * i + 1], m[4 * i + 2], m[4 * i + 3]});
    out[4 * i] = r.a;
    out[4 * i + 1] = r.b;
    out[4 * i + 2] = r.c;
    out[4 * i + 3] = r.d;
  }
};
struct OpDivBy {
  ANM_HD void operator()(int64_t i, const double* x, const double* d, double* out) const {
    out[i] = anm::div_by(x[i], anm::make_recip(d[i]));
  }
};
struct OpDumpDiv {
  ANM_HD void operator()(int64_t i, const double* num, const double* den, double* out) const {
    out[i] = anm::dump_div(num[i], den[i]);
  }
};
struct OpDumpAbsArg {
  ANM_HD void operator()(int64_t i, const double* x, const double* y, double* mag, double* ang) const {
    mag[i] = anm::dump_abs(x[i], y[i]);
    ang[i] = anm::dump_arg(y[i], x[i]);
  }
};
struct OpMaxMin {
  ANM_HD void operator()(int64_t i, const double* a, const double* b, double* mx, double* mn) const {
    mx[i] = anm::vmax(a[i], b[i]);
    mn[i] = anm::vmin(a[i], b[i]);
  }
};
#if defined(__HIPCC__)
struct OpRcp {      // the hardware estimate itself: what recip, dump_div and blk_inv_fast start from
  PROBE_D void operator()(int64_t i, const double* x, double* out) const { out[i] = __builtin_amdgcn_rcp(x[i]); }
};
struct OpBlkInvFast {
  PROBE_D void operator()(int64_t i, const double* m, double* out) const {
    const anm::Blk<double> r =
        anm::group::blk_inv_fast(anm::Blk<double>{m[4 * i], m[4 * i + 1], m[4 * i + 2], m[4 * i + 3]});
    out[4 * i] = r.a;
    out[4 * i + 1] = r.b;
    out[4 * i + 2] = r.c;
    out[4 * i + 3] = r.d;
  }
};
#endif

#if defined(__HIPCC__)
template <class OP, class... A>
__global__ void __launch_bounds__(256) k_each(int64_t n, A... a) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) OP{}(i, a...);
}
template <class OP, class... A>
int run(int64_t n, void* stream, A... a) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL((k_each<OP, A...>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, a...);
  return (int)hipGetLastError();
}
#else
template <class OP, class... A>
int run(int64_t n, void*, A... a) {
  for (int64_t i = 0; i < n; ++i) OP{}(i, a...);
  return 0;
}
#endif

}  // namespace

extern "C" {

int anm_probe_is_device(void) {
#if defined(__HIPCC__)
  return 1;
#else
  return 0;
#endif
}
int anm_probe_sincos(int path, int64_t n, const double* x, double* s, double* c, void* stream) {
  switch (path) {
    case 0: return run<OpSinCos<0>>(n, stream, x, s, c);
    case 1: return run<OpSinCos<1>>(n, stream, x, s, c);
    case 2: return run<OpSinCos<2>>(n, stream, x, s, c);
    case 3: return run<OpSinCos<3>>(n, stream, x, s, c);
    case 4: return run<OpSinCos<4>>(n, stream, x, s, c);
  }
  return -2;
}
int anm_probe_recip(int64_t n, const double* x, double* out, void* stream) { return run<OpRecip>(n, stream, x, out); }
int anm_probe_blk_inv(int64_t n, const double* m, double* out, void* stream) { return run<OpBlkInv>(n, stream, m, out); }
int anm_probe_div_by(int64_t n, const double* x, const double* d, double* out, void* stream) {
  return run<OpDivBy>(n, stream, x, d, out);
}
int anm_probe_dump_div(int64_t n, const double* num, const double* den, double* out, void* stream) {
  return run<OpDumpDiv>(n, stream, num, den, out);
}
int anm_probe_dump_abs_arg(int64_t n, const double* x, const double* y, double* mag, double* ang, void* stream) {
  return run<OpDumpAbsArg>(n, stream, x, y, mag, ang);
}
int anm_probe_max_min(int64_t n, const double* a, const double* b, double* mx, double* mn, void* stream) {
  return run<OpMaxMin>(n, stream, a, b, mx, mn);
}
// device only
int anm_probe_rcp(int64_t n, const double* x, double* out, void* stream) {
#if defined(__HIPCC__)
  return run<OpRcp>(n, stream, x, out);
#else
  return -1;
#endif
}
int anm_probe_blk_inv_fast(int64_t n, const double* m, double* out, void* stream) {
#if defined(__HIPCC__)
  return run<OpBlkInvFast>(n, stream, m, out);
#else
  return -1;
#endif
}

}  // extern "C"
