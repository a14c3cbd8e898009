// devbuf_check.cpp -- DevBuf<T> (gym_anm_amd/csrc/anm_devbuf.hpp) on the host: the three HIP calls it makes are
// stand-ins over malloc / free / memcpy that count live allocations, so that its move, reset and replace logic runs
// under the address and undefined-behaviour sanitizers on a CPU (tests/test_devbuf.py).  A double free, a use after
// free or a leak is the sanitizers' to find; the counts and contents are checked here.  Exit status 0: all held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1;
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };

static int g_live = 0, g_allocs = 0;
static size_t g_last_bytes = 0;
static int g_fail_malloc = 0, g_fail_copy = 0;   // the next call of that kind fails

template <class T>
hipError_t hipMalloc(T** p, size_t bytes) {
  g_last_bytes = bytes;
  if (g_fail_malloc) { g_fail_malloc = 0; return hipErrorOutOfMemory; }   // (*p left as it was, like a failed allocation may)
  *p = static_cast<T*>(std::malloc(bytes));
  ++g_live;
  ++g_allocs;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  std::free(p);
  --g_live;
  return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  if (g_fail_copy) { g_fail_copy = 0; return hipErrorInvalidValue; }
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}

#include "../../gym_anm_amd/csrc/anm_devbuf.hpp"

using anm::DevBuf;

static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

struct Model {   // owners as members, like anm_model: `delete` is all a destroy has to do
  DevBuf<double> a, b;
  DevBuf<int> c;
};

int main() {
  const std::vector<double> v{1.0, 2.0, 3.0};
  {
    DevBuf<double> x;
    CHECK(x.get() == nullptr && g_live == 0);
    x.reset();   // of an empty owner: nothing
    CHECK(x.assign(v.data(), v.size()) == hipSuccess && g_live == 1 && g_last_bytes == 24);
    CHECK(x.get()[0] == 1.0 && x.get()[2] == 3.0);
    CHECK(x.assign(v.data(), 2, 8) == hipSuccess && g_live == 1 && g_last_bytes == 24);   // the old buffer went first
    CHECK(x.assign(v.data(), 0) == hipSuccess && g_live == 1 && g_last_bytes == 8);        // never less than 8 bytes
    CHECK(x.assign(v.data(), 0, 8) == hipSuccess && g_last_bytes == 8);
    DevBuf<int> one;
    const int zero = 0;
    CHECK(one.assign(&zero, 1) == hipSuccess && g_last_bytes == 8 && one.get()[0] == 0 && g_live == 2);
    // move construction and move assignment: one owner at a time, the target's old buffer freed
    double* p = x.get();
    DevBuf<double> y(std::move(x));
    CHECK(y.get() == p && x.get() == nullptr && g_live == 2);
    DevBuf<double> z;
    CHECK(z.alloc(5) == hipSuccess && g_last_bytes == 40 && g_live == 3);
    z = std::move(y);
    CHECK(z.get() == p && y.get() == nullptr && g_live == 2);
    DevBuf<double>& zr = z;
    z = std::move(zr);   // onto itself: kept
    CHECK(z.get() == p && g_live == 2);
    z = DevBuf<double>();   // an empty owner moved in: freed
    CHECK(z.get() == nullptr && g_live == 1);
    // a failed allocation leaves the owner empty; a failed copy leaves it holding the new buffer (get() tells which)
    CHECK(z.assign(v.data(), 3) == hipSuccess && g_live == 2);
    g_fail_malloc = 1;
    CHECK(z.assign(v.data(), 3) != hipSuccess && z.get() == nullptr && g_live == 1);
    g_fail_copy = 1;
    CHECK(z.assign(v.data(), 3) != hipSuccess && z.get() != nullptr && g_live == 2);
    // stage, then commit: the staged owner replaces the member only when everything before it worked
    Model* m = new Model;
    CHECK(m->a.assign(v.data(), 3) == hipSuccess && m->c.assign(&zero, 1) == hipSuccess && g_live == 4);
    double* kept = m->a.get();
    {
      DevBuf<double> staged;
      g_fail_malloc = 1;
      if (staged.assign(v.data(), 2) == hipSuccess) m->a = std::move(staged);
    }
    CHECK(m->a.get() == kept && kept[1] == 2.0 && g_live == 4);   // refused: as it was
    {
      DevBuf<double> staged;
      if (staged.assign(v.data() + 1, 2) == hipSuccess) m->a = std::move(staged);
    }
    CHECK(m->a.get()[0] == 2.0 && g_live == 4);
    delete m;
    CHECK(g_live == 2);
  }
  CHECK(g_live == 0 && g_allocs > 0);
  if (g_bad == 0) std::printf("devbuf ok: %d allocations, none live\n", g_allocs);
  return g_bad == 0 ? 0 : 1;
}
