// photo_lut.h — the arithmetic of the photometric stage (include/heif_hipdec.h, hipdec_tensor_photo) that works on a value, an operation or a histogram
// alone: BLEND, LUM, the point operations, and what derives a step's parameters from a sample's histogram - the contrast mean, the autocontrast table,
// the equalize table.  Also the record an entry has in the per-step table of k_photo_hist / k_photo_apply (photo_kernels.h) and the refusals an operation
// alone decides.  Plain C++ without a HIP dependency: photo_kernels.h compiles these very functions for the device (PHOTO_FN carries the qualifiers
// there), color.hip uses them on the host, and tests/emu/photo_lut_asan.cc runs them under AddressSanitizer as a stand-alone program.
// Every floating-point statement below is one IEEE operation per written operator - the builds have -ffp-contract=off, and the definition depends on it:
// a fused multiply-add would round BLEND's and the autocontrast table's a * b + c once instead of twice.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef PHOTO_FN
#define PHOTO_FN inline
#endif

namespace hipdec {

// hipdec_photo_opcode (color.hip asserts that the values are the header's); PHOTO_NONE: an empty chain's only step, the identity
enum PhotoOp { PHOTO_NONE = 0, PHOTO_BRIGHTNESS = 1, PHOTO_COLOR = 2, PHOTO_CONTRAST = 3, PHOTO_SHARPNESS = 4, PHOTO_POSTERIZE = 5, PHOTO_SOLARIZE = 6,
               PHOTO_INVERT = 7, PHOTO_AUTOCONTRAST = 8, PHOTO_EQUALIZE = 9 };

constexpr double kPhotoValueLimit = 65536.0;   // |value| stays at or below it: BLEND's float then stays far inside what converts to int

// One entry of a step's table, 8 words of 8 bytes: uniform per workgroup, read by scalar loads (photo_kernels.h photo_entry_load)
struct PhotoEntry {
  const uint8_t* src;    // the h x w x 3 sample this step reads
  uint8_t* dst;          // what it writes: the U8 / NHWC sample of the other ping-pong buffer, or - last - the entry's first tensor element
  uint32_t* hist;        // the entry's 4 x 256 histogram of src (R, G, B, LUM), or NULL where the step needs none
  double value;
  int32_t op, last;      // PhotoOp; the entry's last step: dst is the tensor
  uint64_t reserved[3];
};
static_assert(sizeof(PhotoEntry) == 64, "the kernels read 8 words");

PHOTO_FN bool photo_needs_statistics(int op) { return op == PHOTO_CONTRAST || op == PHOTO_AUTOCONTRAST || op == PHOTO_EQUALIZE; }

// What an operation alone decides.  0: taken; 1: unknown op; 2: reserved is not 0; 3: the value is not finite; 4: |value| > 65536;
// 5: POSTERIZE with a value that is not an integer 0 .. 8
inline int photo_op_check(int op, int reserved, double value)
{
  if (op < PHOTO_BRIGHTNESS || op > PHOTO_EQUALIZE) return 1;
  if (reserved) return 2;
  if (!std::isfinite(value)) return 3;
  if (std::fabs(value) > kPhotoValueLimit) return 4;
  if (op == PHOTO_POSTERIZE && (value < 0.0 || value > 8.0 || value != (double)(int)value)) return 5;
  return 0;
}

// Image.blend(degenerate, image, alpha) for one component: single precision, the product rounded, then the sum
PHOTO_FN int photo_blend(int D, int V, float alpha)
{
  const float t = (float)D + alpha * (float)(V - D);
  if (alpha >= 0.0f && alpha <= 1.0f) return (int)t & 255;
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// convert("L")
PHOTO_FN int photo_lum(int R, int G, int B) { return (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16; }

// the grey value CONTRAST blends with: the mean of LUM over the sample, in double, rounded half up
PHOTO_FN int photo_contrast_mean(uint64_t lum_sum, uint64_t pixels) { return (int)((double)lum_sum / (double)pixels + 0.5); }

// the point operations that need nothing but the value (NONE, BRIGHTNESS, POSTERIZE, SOLARIZE, INVERT)
PHOTO_FN int photo_point(int op, double value, int v)
{
  switch (op) {
    case PHOTO_BRIGHTNESS: return photo_blend(0, v, (float)value);
    case PHOTO_POSTERIZE: return v & ((0xFF << (8 - (int)value)) & 0xFF);
    case PHOTO_SOLARIZE: return (double)v < value ? v : 255 - v;
    case PHOTO_INVERT: return 255 - v;
    default: return v;
  }
}

// ImageOps.autocontrast, cutoff 0, for a channel whose least and greatest value present are lo and hi: double, the product rounded, then the sum,
// truncated toward zero, clamped
PHOTO_FN int photo_autocontrast(int v, int lo, int hi)
{
  if (hi <= lo) return v;
  const double scale = 255.0 / (double)(hi - lo), offset = (double)(-lo) * scale;
  const int ix = (int)((double)v * scale + offset);
  return ix < 0 ? 0 : (ix > 255 ? 255 : ix);
}

// ImageOps.equalize for a channel: `before` = H[0] + .. + H[v - 1], total = w * h, lo / hi the first and last non-zero bin, h_last = H[hi]
PHOTO_FN int photo_equalize(int v, uint32_t before, uint32_t total, uint32_t h_last, int lo, int hi)
{
  if (hi <= lo) return v;                       // fewer than two bins are non-zero
  const uint32_t step = (total - h_last) / 255u;
  if (step == 0) return v;
  const uint32_t r = (step / 2u + before) / step;
  return r > 255u ? 255 : (int)r;
}

// ---- whole-histogram forms (host): H has 256 bins and at least one is non-zero
inline void photo_hist_range(const uint32_t* H, int* lo, int* hi)
{
  int l = 0, h = 255;
  while (l < 255 && !H[l]) l++;
  while (h > 0 && !H[h]) h--;
  *lo = l; *hi = h;
}

inline uint64_t photo_hist_weighted_sum(const uint32_t* H)
{
  uint64_t s = 0;
  for (int v = 0; v < 256; v++) s += (uint64_t)v * (uint64_t)H[v];
  return s;
}

inline void photo_autocontrast_lut(const uint32_t* H, uint8_t* lut)
{
  int lo, hi;
  photo_hist_range(H, &lo, &hi);
  for (int v = 0; v < 256; v++) lut[v] = (uint8_t)photo_autocontrast(v, lo, hi);
}

inline void photo_equalize_lut(const uint32_t* H, uint8_t* lut)
{
  int lo, hi;
  photo_hist_range(H, &lo, &hi);
  uint32_t total = 0;
  for (int v = 0; v < 256; v++) total += H[v];
  uint32_t before = 0;
  for (int v = 0; v < 256; v++) { lut[v] = (uint8_t)photo_equalize(v, before, total, H[hi], lo, hi); before += H[v]; }
}

}  // namespace hipdec
