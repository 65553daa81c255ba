// CPU-TEST-ONLY.  The arithmetic of the augment stage that works on a pixel, an operation or a radius alone (libheif_amd/csrc/augment_lut.h: Pillow's
// RGB <-> HSV conversions, the hue shift, the extended-box parameters of ImageFilter.GaussianBlur, one box pass over a line, the refusals) under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program.  Built and run by tests/test_augment_lut_host.py and
// tools/augment_lut_sanitizer.sh:
//   g++ -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Ilibheif_amd/csrc tests/emu/augment_lut_asan.cc
// Every line a box pass reads or writes is allocated with exactly its samples (an access one element outside is a heap overflow the sanitizer reports);
// the float -> int conversions of the HSV functions and of the box parameters run over their whole domain (an out-of-range conversion is what UBSan
// reports).  Modes - requests on stdin as text, results on stdout as raw bytes, which the test compares with tests/augment_ref.py:
//   rgb2hsv step            H, S, V of every (R, G, B) of the lattice 0, step, 2 step, .. with 255 added, R-major: 3 bytes each
//   hsv2rgb step            likewise R, G, B of every (H, S, V)
//   hue                     per line "d step": R', G', B' of the lattice through HUE with shift d
//   box                     per line a radius: r, ww, fw as three little-endian uint32
//   line                    per line "radius n stride v0 v1 .. v(n-1)": the n bytes of one box pass over the line
//   check                   per line "op reserved value": augment_op_check's result as one byte
//   (none)                  a self-check of the bounds: everything above at its extremes, results not printed
#include "augment_lut.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

using namespace hipdec;

static int put(const uint8_t* p, size_t n) { return fwrite(p, 1, n, stdout) == n ? 0 : 1; }

static std::vector<int> lattice(int step)
{
  std::vector<int> v;
  for (int x = 0; x < 255; x += step) v.push_back(x);
  v.push_back(255);
  return v;
}

// one box pass over a line whose buffers hold exactly (n - 1) * stride + 1 bytes
static std::vector<uint8_t> pass(const std::vector<uint8_t>& vals, int stride, int r, uint32_t ww, uint32_t fw)
{
  const int n = (int)vals.size();
  const size_t bytes = (size_t)(n - 1) * (size_t)stride + 1;
  std::unique_ptr<uint8_t[]> in(new uint8_t[bytes]), out(new uint8_t[bytes]);
  memset(in.get(), 0xEE, bytes);
  memset(out.get(), 0xEE, bytes);
  for (int i = 0; i < n; i++) in[(size_t)i * stride] = vals[(size_t)i];
  augment_box_line(in.get(), out.get(), n, stride, r, ww, fw);
  std::vector<uint8_t> res((size_t)n);
  for (int i = 0; i < n; i++) res[(size_t)i] = out[(size_t)i * stride];
  return res;
}

static int self_check()
{
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  long long taken = 0, refused = 0, pixels = 0, lines = 0;
  const double vals[] = {0.0, -0.0, 1.0, 0.5, -0.5, 2.5, 8.0, 8.000001, 9.0, -1.0, 255.0, 255.5, 256.0, 65536.0, -65536.0, 1e300, -1e300, inf, -inf, nan, 4.9e-324};
  for (int op = -2; op <= 19; op++)
    for (int reserved = 0; reserved < 2; reserved++)
      for (double v : vals) {
        if (augment_op_check(op, reserved, v)) { refused++; continue; }
        taken++;
      }
  if (augment_op_check(AUGMENT_HUE, 0, 255.0) || !augment_op_check(AUGMENT_HUE, 0, 256.0) || augment_op_check(AUGMENT_GAUSSIAN_BLUR, 0, 8.0) ||
      !augment_op_check(AUGMENT_GAUSSIAN_BLUR, 0, nan) || !augment_op_check(10, 0, 1.0) || augment_op_check(PHOTO_INVERT, 0, 0.0)) {
    fprintf(stderr, "augment_op_check\n");
    return 2;
  }
  // both HSV functions and the shift over a lattice that holds both ends
  for (int a : lattice(3))
    for (int b : lattice(3))
      for (int c : lattice(3)) {
        int x, y, z, u, v, w;
        augment_rgb2hsv(a, b, c, &x, &y, &z);
        augment_hsv2rgb(a, b, c, &u, &v, &w);
        if ((x | y | z | u | v | w) & ~255) { fprintf(stderr, "HSV of (%d, %d, %d) leaves 0 .. 255\n", a, b, c); return 2; }
        if (z != (a > b ? (a > c ? a : c) : (b > c ? b : c))) { fprintf(stderr, "V of (%d, %d, %d)\n", a, b, c); return 2; }
        for (int d : {0, 1, 128, 255}) {
          augment_hue(d, a, b, c, &u, &v, &w);
          if ((u | v | w) & ~255) { fprintf(stderr, "HUE %d of (%d, %d, %d)\n", d, a, b, c); return 2; }
        }
        pixels++;
      }
  // the box parameters over a radius sweep to the cap, and passes over lines shorter and longer than the window at byte and row strides
  int r_last = 0;
  for (int k = 0; k <= 8000; k++) {
    const double radius = k / 1000.0;
    int r;
    uint32_t ww, fw;
    augment_gaussian_box(radius, &r, &ww, &fw);
    if (r < r_last || r > kAugmentBlurMaxR || (uint64_t)(2 * r + 1) * ww + 2ull * fw > (1u << 24)) { fprintf(stderr, "box of radius %g: %d %u %u\n", radius, r, ww, fw); return 2; }
    r_last = r;
    if (k % 250) continue;
    for (int n : {1, 2, 3, 7, 16, 17, 112})
      for (int stride : {1, 3, 340}) {
        std::vector<uint8_t> v((size_t)n);
        for (int i = 0; i < n; i++) v[(size_t)i] = (uint8_t)((i * 89 + k) & 255);
        const std::vector<uint8_t> o = pass(v, stride, r, ww, fw);
        std::vector<uint8_t> flat((size_t)n, (uint8_t)(k & 255));
        if (pass(flat, stride, r, ww, fw) != flat) { fprintf(stderr, "a flat line of %d through radius %g\n", n, radius); return 2; }
        if (k == 0 && o != v) { fprintf(stderr, "radius 0 is not the identity\n"); return 2; }
        lines++;
      }
  }
  if (r_last != kAugmentBlurMaxR) { fprintf(stderr, "the cap gives r = %d\n", r_last); return 2; }
  printf("AUGMENT LUT SANITIZER OK: %lld operations taken, %lld refused, %lld pixels, %lld lines\n", taken, refused, pixels, lines);
  return 0;
}

int main(int argc, char** argv)
{
  if (argc < 2) return self_check();
  const char* mode = argv[1];
  char line[1 << 16];
  if (!strcmp(mode, "rgb2hsv") || !strcmp(mode, "hsv2rgb")) {
    const std::vector<int> L = lattice(argc > 2 ? atoi(argv[2]) : 5);
    const bool to_hsv = !strcmp(mode, "rgb2hsv");
    for (int a : L)
      for (int b : L)
        for (int c : L) {
          int x, y, z;
          if (to_hsv) augment_rgb2hsv(a, b, c, &x, &y, &z);
          else augment_hsv2rgb(a, b, c, &x, &y, &z);
          const uint8_t o[3] = {(uint8_t)x, (uint8_t)y, (uint8_t)z};
          if (put(o, 3)) return 1;
        }
    return 0;
  }
  while (fgets(line, sizeof line, stdin)) {
    if (!strcmp(mode, "hue")) {
      int d, step;
      if (sscanf(line, "%d %d", &d, &step) != 2) return 1;
      const std::vector<int> L = lattice(step);
      for (int a : L)
        for (int b : L)
          for (int c : L) {
            int x, y, z;
            augment_hue(d, a, b, c, &x, &y, &z);
            const uint8_t o[3] = {(uint8_t)x, (uint8_t)y, (uint8_t)z};
            if (put(o, 3)) return 1;
          }
    } else if (!strcmp(mode, "box")) {
      double radius;
      if (sscanf(line, "%lf", &radius) != 1) return 1;
      int r;
      uint32_t o[3];
      augment_gaussian_box(radius, &r, &o[1], &o[2]);
      o[0] = (uint32_t)r;
      if (put((const uint8_t*)o, sizeof o)) return 1;
    } else if (!strcmp(mode, "line")) {
      char* p = line;
      const double radius = strtod(p, &p);
      const int n = (int)strtol(p, &p, 10), stride = (int)strtol(p, &p, 10);
      if (n < 1 || stride < 1) return 1;
      std::vector<uint8_t> v((size_t)n);
      for (int i = 0; i < n; i++) v[(size_t)i] = (uint8_t)strtol(p, &p, 10);
      int r;
      uint32_t ww, fw;
      augment_gaussian_box(radius, &r, &ww, &fw);
      const std::vector<uint8_t> o = pass(v, stride, r, ww, fw);
      if (put(o.data(), o.size())) return 1;
    } else if (!strcmp(mode, "check")) {
      int op, reserved;
      double v;
      if (sscanf(line, "%d %d %lf", &op, &reserved, &v) != 3) return 1;
      const uint8_t o = (uint8_t)augment_op_check(op, reserved, v);
      if (put(&o, 1)) return 1;
    } else {
      fprintf(stderr, "unknown mode %s\n", mode);
      return 1;
    }
  }
  return 0;
}
