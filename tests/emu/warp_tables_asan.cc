// CPU-TEST-ONLY.  The host code of the warp stage that works on a map alone (libheif_amd/csrc/warp_host.h: warp_map_check, warp_fixed_values,
// warp_scale_table) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program.  Built and run by tools/warp_tables_sanitizer.sh:
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=all -Ilibheif_amd/csrc tests/emu/warp_tables_asan.cc
// Every table is allocated with exactly the elements it is to hold (a write one element past them is a heap overflow the sanitizer reports); every map that
// passes warp_map_check goes through the double -> int conversions of both NEAREST paths (an out-of-range conversion is what UBSan reports), at the edges of
// the refusal bounds included.
#include "warp_host.h"
#include <cstdio>
#include <limits>
#include <memory>

using namespace hipdec;

static long long g_tables = 0, g_fixed = 0, g_refused = 0;

static int run(const double (&a)[6], int ow, int oh, int sw, int sh)
{
  int which = -1;
  const int rc = warp_map_check(a, ow, oh, &which);
  if (rc) {
    if (which < 0 || which > 5) { fprintf(stderr, "refusal %d names %d\n", rc, which); return 1; }
    g_refused++;
    return 0;
  }
  if (warp_scale_only(a)) {
    std::unique_ptr<int32_t[]> xt(new int32_t[ow]), yt(new int32_t[oh]);   // exactly ow and oh elements
    warp_scale_table(a[2], a[0], ow, xt.get());
    warp_scale_table(a[5], a[4], oh, yt.get());
    for (int x = 0; x < ow; x++) if (xt[x] < -1 || xt[x] > 32000) { fprintf(stderr, "xt[%d] = %d\n", x, xt[x]); return 2; }
    for (int y = 0; y < oh; y++) if (yt[y] < -1 || yt[y] > 32000) { fprintf(stderr, "yt[%d] = %d\n", y, yt[y]); return 2; }
    g_tables++;
  }
  int32_t A[6];
  warp_fixed_values(a, A);
  // the sums of the fixed-point path at the four corner pixels stay inside 64 bits by a wide margin and, shifted, inside the coordinate bound
  const int xs[2] = {0, ow - 1}, ys[2] = {0, oh - 1};
  for (int x : xs)
    for (int y : ys) {
      const int64_t cx = ((int64_t)A[2] + (int64_t)y * A[1] + (int64_t)x * A[0]) >> 16, cy = ((int64_t)A[5] + (int64_t)y * A[4] + (int64_t)x * A[3]) >> 16;
      if (cx < -32769 || cx > 32768 || cy < -32769 || cy > 32768) { fprintf(stderr, "fixed-point corner (%d, %d) -> (%lld, %lld)\n", x, y, (long long)cx, (long long)cy); return 3; }
    }
  (void)sw; (void)sh;
  g_fixed++;
  return 0;
}

int main()
{
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const int sizes[][2] = {{1, 1}, {5, 7}, {65, 17}, {224, 224}, {4096, 3}, {3, 4096}};
  const double vals[] = {0.0, -0.0, 1.0, -1.0, 0.5, 2.0, -0.75, 1e-9, -1e-9, 7.8125, -7.8125, 31999.0, -31999.0, 31999.999, 32000.0, -32000.0, 1e300, inf, -inf, nan, 4.9e-324};
  const int nv = (int)(sizeof(vals) / sizeof(vals[0]));
  for (const auto& s : sizes)
    for (int i0 = 0; i0 < nv; i0++)
      for (int i1 = 0; i1 < nv; i1 += 3)
        for (int i2 = 0; i2 < nv; i2++) {
          const double a[6] = {vals[i0], vals[i1], vals[i2], vals[(i1 + 5) % nv], vals[(i0 + 2) % nv], vals[(i2 + 7) % nv]};
          if (int rc = run(a, s[0], s[1], 33, 17)) return rc;
          const double b[6] = {vals[i0], 0.0, vals[i2], 0.0, vals[(i0 + 2) % nv], vals[(i2 + 7) % nv]};   // Pillow's scale path
          if (int rc = run(b, s[0], s[1], 33, 17)) return rc;
        }
  // maps whose corners sit just inside the bound: the largest values the conversions see
  for (const auto& s : sizes) {
    const double w = (double)s[0], h = (double)s[1];
    const double edge[][6] = {{31999.0 / w, 0, 0.5, 0, 31999.0 / h, 0.5}, {-31999.0 / w, 0, -0.5, 0, -31999.0 / h, -0.5}, {1, 0, 31999.0 - w, 0, 1, 31999.0 - h},
                              {1, 0, -31999.0, 0, 1, -31999.0}, {15999.0 / w, 15999.0 / h, 1.5, -15999.0 / w, -15999.0 / h, -1.5}};
    for (const auto& a : edge) {
      int which = -1;
      if (warp_map_check(a, s[0], s[1], &which) != 0) { fprintf(stderr, "an edge map of %d x %d is refused\n", s[0], s[1]); return 4; }
      if (int rc = run(a, s[0], s[1], 33, 17)) return rc;
    }
  }
  if (g_tables < 100 || g_fixed < 100 || g_refused < 100) { fprintf(stderr, "%lld tables, %lld fixed, %lld refused\n", g_tables, g_fixed, g_refused); return 5; }
  printf("WARP TABLES SANITIZER OK %lld tables %lld fixed-point maps %lld refused\n", g_tables, g_fixed, g_refused);
  return 0;
}
