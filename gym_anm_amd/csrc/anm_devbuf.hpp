// anm_devbuf.hpp -- DevBuf<T>: a device allocation and its one owner.  The memory is freed when the owner goes, is
// reset or is given another buffer; owners are moved, never copied.  Host code only.  The includer brings hipMalloc,
// hipFree and hipMemcpy (anm_capi.hip: <hip/hip_runtime.h>; tests/hostsim/devbuf_check.cpp: counting stand-ins over
// malloc / free / memcpy, for a sanitizer run on the CPU).
#pragma once

#include <algorithm>
#include <cstddef>

namespace anm {

template <class T>
struct DevBuf {
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      o.p_ = nullptr;
    }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }

  T* get() const { return p_; }
  void reset() {
    if (p_) hipFree(p_);
    p_ = nullptr;
  }
  // room for `count` elements and pad_bytes behind them (at least 8 bytes), uninitialised; what was held is freed first
  hipError_t alloc(size_t count, size_t pad_bytes = 0) {
    reset();
    hipError_t e = hipMalloc(&p_, std::max(count * sizeof(T) + pad_bytes, size_t(8)));
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  // ... filled with `count` elements from the host.  After a failure get() tells which half it was: null, the allocation
  hipError_t assign(const T* host, size_t count, size_t pad_bytes = 0) {
    hipError_t e = alloc(count, pad_bytes);
    return e == hipSuccess ? hipMemcpy(p_, host, count * sizeof(T), hipMemcpyHostToDevice) : e;
  }

 private:
  T* p_ = nullptr;
};

}  // namespace anm
