// rt::Owned (raytracedggx_amd/csrc/rt_owned.h) on its own, with a release functor that counts: a stand-alone program, built with
// AddressSanitizer and UBSan by tests/test_owned_host.py and run as a child process.  Nothing of HIP is included.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include "../raytracedggx_amd/csrc/rt_owned.h"

static int g_released = 0;      // calls of the functor
static long g_sum = 0;          // sum of the values it was given: WHICH value was released
struct Count { void operator()(int* p) const { ++g_released; g_sum += *p; } };
struct CountHandle { void operator()(long h) const { ++g_released; g_sum += h; } };
using IntPtr = rt::Owned<int*, Count>;
using Handle = rt::Owned<long, CountHandle>;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (released %d, sum %ld)\n", __LINE__, #cond, g_released, g_sum); return 1; } } while (0)
static void fresh() { g_released = 0; g_sum = 0; }

int main() {
  int a = 1, b = 10, c = 100;
  {  // an empty owner never calls the functor: destructor, reset, release, moves
    fresh();
    { IntPtr e; CHECK(!e && e.get() == nullptr); e.reset(); CHECK(e.release() == nullptr); IntPtr f(std::move(e)); IntPtr g; g = std::move(f); CHECK(!g); }
    CHECK(g_released == 0);
  }
  {  // the destructor releases once
    fresh();
    { IntPtr p; *p.put() = &a; CHECK(p.get() == &a && p && *p == 1 && p + 0 == &a); CHECK(g_released == 0); }
    CHECK(g_released == 1 && g_sum == 1);
  }
  {  // move construction: the source is left empty, nothing is released until the target goes
    fresh();
    { IntPtr p; *p.put() = &a; IntPtr q(std::move(p)); CHECK(!p && q.get() == &a && g_released == 0); }
    CHECK(g_released == 1 && g_sum == 1);
  }
  {  // move assignment: the overwritten value is released exactly once, then and there; the source is left empty
    fresh();
    { IntPtr p, q; *p.put() = &a; *q.put() = &b;
      q = std::move(p);
      CHECK(g_released == 1 && g_sum == 10 && !p && q.get() == &a); }
    CHECK(g_released == 2 && g_sum == 11);
  }
  {  // self-move-assignment releases nothing and keeps the value
    fresh();
    { IntPtr p; *p.put() = &c; IntPtr& same = p; p = std::move(same); CHECK(g_released == 0 && p.get() == &c); }
    CHECK(g_released == 1 && g_sum == 100);
  }
  {  // reset releases and empties; a second reset does nothing
    fresh();
    IntPtr p; *p.put() = &b;
    p.reset(); CHECK(g_released == 1 && g_sum == 10 && !p);
    p.reset(); CHECK(g_released == 1);
  }
  {  // release gives the value up: the functor is never called for it
    fresh();
    { IntPtr p; *p.put() = &b; CHECK(p.release() == &b && !p); }
    CHECK(g_released == 0);
  }
  {  // put() on a full owner releases what it held before it hands out the address
    fresh();
    { IntPtr p; *p.put() = &a; int** slot = p.put(); CHECK(g_released == 1 && g_sum == 1 && *slot == nullptr); *slot = &c; CHECK(p.get() == &c); }
    CHECK(g_released == 2 && g_sum == 101);
  }
  {  // an array of owners with only entry 0 filled (a static mesh's per-set arrays) releases once
    fresh();
    { IntPtr sets[4]; *sets[0].put() = &c; int* views[4]; for (auto& v : views) v = sets[0]; CHECK(views[3] == &c); }
    CHECK(g_released == 1 && g_sum == 100);
  }
  {  // a handle that is no pointer: 0 is "empty"
    fresh();
    { Handle h; *h.put() = 7; Handle k(std::move(h)); long raw = k; CHECK(raw == 7 && h.get() == 0); }
    CHECK(g_released == 1 && g_sum == 7);
  }
  std::printf("owned: all checks passed\n");
  return 0;
}
