// A move-only owner of one value -- a pointer or a handle -- that a functor releases.  Nothing here knows HIP (rt_owned_hip.h names the
// device types), so a host compiler tests it alone (tests/owned_main.cpp).  The conversion to the held value is implicit on purpose: an
// owner goes wherever the raw value went -- kernel arguments, pointer arithmetic, `if (!p)`, `*p` -- and only who releases it has changed.
#pragma once
namespace rt {
template <class T, class Release> class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : v(o.release()) {}
  Owned& operator=(Owned&& o) noexcept { if (this != &o) { reset(); v = o.release(); } return *this; }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { reset(); }
  void reset() { if (v != T{}) Release{}(v); v = T{}; }
  T release() { const T r = v; v = T{}; return r; }      // gives the value up without releasing it
  T get() const { return v; }
  operator T() const { return v; }
  T operator->() const { return v; }
  T* put() { reset(); return &v; }      // for hipMalloc(p.put(), ...): releases what is held, then the address to fill
 private:
  T v{};
};
}  // namespace rt
