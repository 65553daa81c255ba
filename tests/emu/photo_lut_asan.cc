// CPU-TEST-ONLY.  The arithmetic of the photometric stage that works on a value, an operation or a histogram alone (libheif_amd/csrc/photo_lut.h: the
// contrast mean, the autocontrast and equalize tables, BLEND, the point operations, the refusals) under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// stand-alone program.  Built and run by tests/test_photo_lut_host.py and tools/photo_lut_sanitizer.sh:
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=all -Ilibheif_amd/csrc tests/emu/photo_lut_asan.cc
// Every histogram and table is allocated with exactly its 256 elements (an access one element past them is a heap overflow the sanitizer reports); the
// float -> int conversions of BLEND and of the autocontrast table run at the edges of the refusal bound (an out-of-range conversion is what UBSan
// reports).  Modes - requests on stdin as text, results on stdout as raw bytes, which the test compares with tests/photo_ref.py:
//   autocontrast            the 256-byte table of every pair lo < hi, lo-major: 32 640 tables
//   equalize                per line 256 bin counts: the 256-byte table
//   mean                    per line "sum pixels": the mean as one byte
//   blend                   per line a factor: 65 536 bytes, BLEND(D, V, f) for D = 0 .. 255 (major), V = 0 .. 255
//   point                   per line "op value": the 256-byte table of the point operation
//   check                   per line "op reserved value": photo_op_check's result as one byte
//   (none)                  a self-check of the bounds: everything above at its extremes, results not printed
#include "photo_lut.h"
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

using namespace hipdec;

static int put(const uint8_t* p, size_t n) { return fwrite(p, 1, n, stdout) == n ? 0 : 1; }

static int self_check()
{
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  long long taken = 0, refused = 0;
  const double vals[] = {0.0, -0.0, 1.0, 0.5, -0.5, 1.5, 8.0, 8.5, 9.0, -1.0, 255.0, 256.0, 65536.0, -65536.0, 65536.000001, 1e300, -1e300, inf, -inf, nan, 4.9e-324};
  for (int op = -2; op <= 11; op++)
    for (int reserved = 0; reserved < 2; reserved++)
      for (double v : vals) {
        if (photo_op_check(op, reserved, v)) { refused++; continue; }
        taken++;
        std::unique_ptr<uint8_t[]> lut(new uint8_t[256]);
        for (int x = 0; x < 256; x++) lut[x] = (uint8_t)photo_point(op, v, x);
        for (int D = 0; D < 256; D += 5)
          for (int V = 0; V < 256; V++) {
            const int r = photo_blend(D, V, (float)v);
            if (r < 0 || r > 255) { fprintf(stderr, "BLEND(%d, %d, %g) = %d\n", D, V, v, r); return 2; }
          }
      }
  std::unique_ptr<uint32_t[]> H(new uint32_t[256]);
  std::unique_ptr<uint8_t[]> lut(new uint8_t[256]);
  const uint32_t counts[] = {1u, 2u, 254u, 255u, 256u, 32767u * 32767u - 1u};
  for (uint32_t big : counts)
    for (int lo = 0; lo < 256; lo += 17)
      for (int hi = lo; hi < 256; hi += 15) {
        memset(H.get(), 0, 256 * sizeof(uint32_t));
        H[lo] += big; H[hi] += 1;
        int l = -1, h = -1;
        photo_hist_range(H.get(), &l, &h);
        if (l != lo || h != hi) { fprintf(stderr, "range of (%d, %d) is (%d, %d)\n", lo, hi, l, h); return 3; }
        photo_autocontrast_lut(H.get(), lut.get());
        photo_equalize_lut(H.get(), lut.get());
        const int m = photo_contrast_mean(photo_hist_weighted_sum(H.get()), (uint64_t)big + 1);
        if (m < 0 || m > 255) { fprintf(stderr, "mean %d\n", m); return 4; }
      }
  if (taken < 100 || refused < 100) { fprintf(stderr, "%lld taken, %lld refused\n", taken, refused); return 5; }
  printf("PHOTO LUT SANITIZER OK %lld operations taken %lld refused\n", taken, refused);
  return 0;
}

int main(int argc, char** argv)
{
  if (argc < 2) return self_check();
  const char* mode = argv[1];
  std::unique_ptr<uint32_t[]> H(new uint32_t[256]);     // exactly 256 bins
  std::unique_ptr<uint8_t[]> lut(new uint8_t[256]);     // exactly 256 entries
  if (!strcmp(mode, "autocontrast")) {
    for (int lo = 0; lo < 256; lo++)
      for (int hi = lo + 1; hi < 256; hi++) {
        memset(H.get(), 0, 256 * sizeof(uint32_t));
        H[lo] = 1; H[hi] = 1;
        photo_autocontrast_lut(H.get(), lut.get());
        if (put(lut.get(), 256)) return 1;
      }
    return 0;
  }
  if (!strcmp(mode, "equalize")) {
    for (;;) {
      for (int v = 0; v < 256; v++)
        if (scanf("%u", &H[v]) != 1) return v == 0 ? 0 : 1;
      photo_equalize_lut(H.get(), lut.get());
      if (put(lut.get(), 256)) return 1;
    }
  }
  if (!strcmp(mode, "mean")) {
    unsigned long long sum, pixels;
    while (scanf("%llu %llu", &sum, &pixels) == 2) {
      const uint8_t m = (uint8_t)photo_contrast_mean(sum, pixels);
      if (put(&m, 1)) return 1;
    }
    return 0;
  }
  if (!strcmp(mode, "blend")) {
    double f;
    while (scanf("%lf", &f) == 1)
      for (int D = 0; D < 256; D++) {
        for (int V = 0; V < 256; V++) lut[V] = (uint8_t)photo_blend(D, V, (float)f);
        if (put(lut.get(), 256)) return 1;
      }
    return 0;
  }
  if (!strcmp(mode, "point")) {
    int op;
    double value;
    while (scanf("%d %lf", &op, &value) == 2) {
      for (int V = 0; V < 256; V++) lut[V] = (uint8_t)photo_point(op, value, V);
      if (put(lut.get(), 256)) return 1;
    }
    return 0;
  }
  if (!strcmp(mode, "check")) {
    int op, reserved;
    double value;
    while (scanf("%d %d %lf", &op, &reserved, &value) == 3) {
      const uint8_t r = (uint8_t)photo_op_check(op, reserved, value);
      if (put(&r, 1)) return 1;
    }
    return 0;
  }
  fprintf(stderr, "unknown mode %s\n", mode);
  return 2;
}
