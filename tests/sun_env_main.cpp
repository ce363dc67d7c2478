// The host side of rtggx_sun_from_env (raytracedggx_amd/csrc/rt_sun_env.h) on its own: the arguments and their defaults, the squared
// cosines, a texel's integer direction, the rounding to binary16, the background, the found decision, direction and irradiance.  A
// stand-alone program, built with AddressSanitizer and UBSan by tests/test_sunenv_host.py and run as a child process.  Nothing of HIP is
// included.
//   sun_env                 the checks written out below; ends with "sun env: all N checks passed"
//   sun_env record <13 doubles as hex floats> <contrast>
//                           ring_rgb[3] weight_ring peak_luma sum_wy weight_all moment[3] excess[3]: prints what the host derives from them,
//                           floats and doubles by their bits, for the comparison with tests/sunenv_ref.py
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include "../raytracedggx_amd/csrc/rt_sun_env.h"

static int g_failed = 0, g_checked = 0;
static void expect(const char* what, bool ok) {
  ++g_checked;
  if (!ok && g_failed++ < 40) std::printf("FAILED %s\n", what);
}
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static uint64_t bits(double f) { uint64_t u; std::memcpy(&u, &f, 8); return u; }
static double ulps(double a, double b) { return std::fabs(a - b) / (std::nextafter(std::fabs(b), INFINITY) - std::fabs(b)); }

static int record(char** argv) {
  double v[13];
  for (int k = 0; k < 13; ++k) v[k] = std::strtod(argv[k], nullptr);
  const float contrast = std::strtof(argv[13], nullptr);
  const rt::SunEnvBackground bg = rt::sunEnvBackground(v, v[3]);
  double mean = 0.0;
  const bool found = rt::sunEnvFound(v[4], v[5], v[6], contrast, mean);
  float dir[3], irr[3];
  const bool ok = rt::sunEnvResult(v + 7, v + 10, v[6], dir, irr);
  std::printf("background %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits(bg.background[0]), bits(bg.background[1]), bits(bg.background[2]));
  std::printf("half %04x %04x %04x\n", (unsigned)bg.half[0], (unsigned)bg.half[1], (unsigned)bg.half[2]);
  std::printf("half_as_float %08x %08x %08x\n", bits(bg.halfAsFloat[0]), bits(bg.halfAsFloat[1]), bits(bg.halfAsFloat[2]));
  std::printf("mean %016" PRIx64 " found %d result %d\n", bits(mean), found ? 1 : 0, ok ? 1 : 0);
  std::printf("direction %08x %08x %08x\n", bits(dir[0]), bits(dir[1]), bits(dir[2]));
  std::printf("irradiance %08x %08x %08x\n", bits(irr[0]), bits(irr[1]), bits(irr[2]));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 16 && std::strcmp(argv[1], "record") == 0) return record(argv + 2);
  if (argc != 1) { std::printf("usage: sun_env [record <13 hex doubles> <contrast>]\n"); return 2; }
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

  // ---- the arguments: 0 selects the defaults; the header's list of refusals
  rt::SunEnvAngles a;
  expect("defaults accepted", rt::sunEnvAngles(0.0f, 0.0f, 0.0f, a) == nullptr);
  expect("default cone 4, ring 12, contrast 16", a.cone == 4.0f && a.ring == 12.0f && a.minContrast == 16.0f);
  expect("cos2 of the defaults", a.cos2Cone == rt::sunEnvCos2(4.0f) && a.cos2Ring == rt::sunEnvCos2(12.0f) && a.cos2Cone > a.cos2Ring);
  expect("a given cone keeps 3 x for the ring", rt::sunEnvAngles(20.0f, 0.0f, 0.0f, a) == nullptr && a.ring == 60.0f);
  expect("45 / 89 are the ends", rt::sunEnvAngles(45.0f, 89.0f, 0.0f, a) == nullptr);
  expect("everything given", rt::sunEnvAngles(20.0f, 40.0f, 2.0f, a) == nullptr && a.cone == 20.0f && a.ring == 40.0f && a.minContrast == 2.0f);
  const float badCones[] = {-1.0f, 45.5f, 90.0f, nan, inf, -inf};
  for (float c : badCones) expect("a cone outside (0, 45] is refused", rt::sunEnvAngles(c, 0.0f, 0.0f, a) != nullptr);
  expect("the default ring of a 40 degree cone is 120: refused", rt::sunEnvAngles(40.0f, 0.0f, 0.0f, a) != nullptr);
  const float badRings[] = {20.0f, 10.0f, -3.0f, 89.5f, nan, inf};
  for (float r : badRings) expect("a ring outside (cone, 89] is refused", rt::sunEnvAngles(20.0f, r, 0.0f, a) != nullptr);
  const float badContrasts[] = {-1.0f, nan, inf, -inf};
  for (float m : badContrasts) expect("a negative or non-finite contrast is refused", rt::sunEnvAngles(4.0f, 12.0f, m, a) != nullptr);

  // ---- the cosines: within 4 ulp of the values known in closed form
  expect("cos2(60) = 1/4", ulps(rt::sunEnvCos2(60.0f), 0.25) <= 4.0);
  expect("cos2(45) = 1/2", ulps(rt::sunEnvCos2(45.0f), 0.5) <= 4.0);
  expect("cos2(30) = 3/4", ulps(rt::sunEnvCos2(30.0f), 0.75) <= 4.0);

  // ---- directions: the face's axis carries +-S, the other two the odd integers a, b with cubeFaceDir's signs
  const uint32_t sides[] = {1u, 2u, 5u, 8192u};
  for (uint32_t S : sides) {
    const uint32_t x = S - 1u, y = 0u;
    const double s = (double)S, p = (double)S - 1.0, m = 1.0 - (double)S;      // a = 2 x + 1 - S = S - 1, b = 1 - S
    const double want[6][3] = {{s, -m, -p}, {-s, -m, p}, {p, s, m}, {p, -s, -m}, {p, -m, s}, {-p, -m, -s}};
    for (uint32_t f = 0; f < 6u; ++f) {
      double D[3];
      rt::sunEnvDirection(S, f, x, y, D);
      expect("integer direction of a corner texel", D[0] == want[f][0] && D[1] == want[f][1] && D[2] == want[f][2]);
    }
  }

  // ---- binary16: every non-negative finite half survives the round trip, halfway cases go to even, 65504 is the cap
  bool roundTrip = true, ties = true;
  for (uint32_t h = 0; h <= 0x7BFFu; ++h) {
    const float f = rt::sunEnvHalfToFloat((uint16_t)h);
    roundTrip = roundTrip && rt::sunEnvHalf(f) == h;
    if (h < 0x7BFFu) {
      const float g = rt::sunEnvHalfToFloat((uint16_t)(h + 1u)), mid = 0.5f * (f + g);      // exact: 12 significant bits
      ties = ties && rt::sunEnvHalf(mid) == ((h & 1u) ? h + 1u : h);
      ties = ties && rt::sunEnvHalf(std::nextafter(mid, 0.0f)) == h && rt::sunEnvHalf(std::nextafter(mid, inf)) == h + 1u;
    }
  }
  expect("half -> float -> half is the identity", roundTrip);
  expect("halfway between two halves goes to the even one, either side to its neighbour", ties);
  expect("1 and 65504", rt::sunEnvHalf(1.0f) == 0x3C00u && rt::sunEnvHalf(65504.0f) == 0x7BFFu && rt::sunEnvHalfToFloat(0x7BFFu) == 65504.0f);

  // ---- the background
  { const double ring[3] = {3.0, 1.5, 0.75};
    rt::SunEnvBackground b = rt::sunEnvBackground(ring, 0.0);
    expect("an empty ring: background 0", b.background[0] == 0.0 && b.half[1] == 0u && b.halfAsFloat[2] == 0.0f);
    b = rt::sunEnvBackground(ring, 3.0);
    expect("ring_rgb / weight_ring", b.background[0] == 1.0 && b.background[1] == 0.5 && b.background[2] == 0.25 && b.half[0] == 0x3C00u && b.halfAsFloat[1] == 0.5f);
    const double big[3] = {65519.0, 1e9, 65504.0};
    b = rt::sunEnvBackground(big, 1.0);
    expect("capped at 65504", b.half[0] == 0x7BFFu && b.half[1] == 0x7BFFu && b.half[2] == 0x7BFFu && b.halfAsFloat[1] == 65504.0f); }

  // ---- found
  { double mean = -1.0;
    expect("a black cube has no sun", !rt::sunEnvFound(0.0, 0.0, 12.5, 16.0f, mean) && mean == 0.0);
    expect("a constant cube has no sun", !rt::sunEnvFound(0.75, 0.75 * 12.5, 12.5, 16.0f, mean) && mean == 0.75);
    expect("peak = contrast x mean is a sun", rt::sunEnvFound(12.0, 0.75 * 12.5, 12.5, 16.0f, mean));
    expect("just below is not", !rt::sunEnvFound(std::nextafter(12.0, 0.0), 0.75 * 12.5, 12.5, 16.0f, mean));
    expect("contrast 0 here means any peak above black", rt::sunEnvFound(1e-7, 5.0, 12.5, 0.0f, mean)); }

  // ---- direction and irradiance
  { float d[3], e[3];
    const double zero[3] = {0.0, 0.0, 0.0}, m[3] = {3.0, -4.0, 12.0}, x[3] = {1.0, 2.0, 0.0};
    const double bad[3] = {0.0, std::numeric_limits<double>::quiet_NaN(), 1.0}, huge[3] = {1e200, 1e200, 0.0};
    expect("a zero moment: nothing found, zeros", !rt::sunEnvResult(zero, x, 12.5, d, e) && d[0] == 0.0f && e[1] == 0.0f);
    expect("a NaN moment: nothing found", !rt::sunEnvResult(bad, x, 12.5, d, e));
    expect("a moment whose square overflows: nothing found", !rt::sunEnvResult(huge, x, 12.5, d, e));
    expect("a 3-4-12 moment", rt::sunEnvResult(m, x, 12.5, d, e) && d[0] == (float)(3.0 / 13.0) && d[1] == (float)(-4.0 / 13.0) && d[2] == (float)(12.0 / 13.0));
    const double scale = 4.0 * 3.14159265358979323846 / 12.5;
    expect("irradiance = excess x 4 pi / weight_all", e[0] == (float)(1.0 * scale) && e[1] == (float)(2.0 * scale) && e[2] == 0.0f); }

  if (g_failed) { std::printf("sun env: %d of %d checks FAILED\n", g_failed, g_checked); return 1; }
  std::printf("sun env: all %d checks passed\n", g_checked);
  return 0;
}
