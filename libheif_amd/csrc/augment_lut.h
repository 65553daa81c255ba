// augment_lut.h — the arithmetic of the augment stage (include/heif_hipdec.h, hipdec_tensor_augment) that works on a pixel, an operation or a radius alone:
// Pillow's RGB <-> HSV conversions (HUE), the extended-box parameters of ImageFilter.GaussianBlur and one box pass over a line (GAUSSIAN_BLUR), the refusals
// an operation alone decides, and the record an entry has in the per-step tables of k_augment_hue / k_augment_blur (augment_kernels.h).  Operations 1 .. 9
// are the photo stage's (photo_lut.h).  Plain C++ without a HIP dependency, as photo_lut.h is: augment_kernels.h compiles these very functions for the
// device (PHOTO_FN carries the qualifiers there), color.hip uses them on the host, and tests/emu/augment_lut_asan.cc runs them under AddressSanitizer as a
// stand-alone program.
// Every floating-point statement below is one IEEE operation per written operator (-ffp-contract=off); where the definition says float or double the
// casts are written out.  Single-precision divisions are correctly rounded (hipcc's default; no fast-math).
#pragma once
#include "photo_lut.h"

namespace hipdec {

enum AugmentOp { AUGMENT_HUE = 16, AUGMENT_GAUSSIAN_BLUR = 17 };

constexpr double kAugmentBlurMaxRadius = 8.0;   // HIPDEC_AUGMENT_BLUR_MAX_RADIUS: r <= 7
constexpr int kAugmentBlurMaxR = 7;

// One entry of a step's hue or blur table, 8 words of 8 bytes like PhotoEntry: uniform per workgroup, read by scalar loads (augment_entry_load)
struct AugmentEntry {
  const uint8_t* src;    // the h x w x 3 sample this step reads
  uint8_t* dst;          // the U8 / NHWC sample of the other ping-pong buffer, or - last - the entry's first tensor element
  int32_t op, last;      // AugmentOp; the entry's last step: dst is the tensor
  int32_t shift, r;      // HUE: d.  GAUSSIAN_BLUR: the box's whole radius r ...
  uint32_t ww, fw;       // ... the weight of a whole sample and of the two fractional ones, of 1 << 24 (augment_gaussian_box)
  uint64_t reserved[3];
};
static_assert(sizeof(AugmentEntry) == 64, "the kernels read 5 of 8 words");

PHOTO_FN bool augment_is_photo_op(int op) { return op >= PHOTO_NONE && op <= PHOTO_EQUALIZE; }

// What an operation alone decides.  0 .. 5: photo_op_check's answers; 6: HUE with a value that is not an integer 0 .. 255; 7: GAUSSIAN_BLUR with a
// radius below 0 or above the cap
inline int augment_op_check(int op, int reserved, double value)
{
  if (op != AUGMENT_HUE && op != AUGMENT_GAUSSIAN_BLUR) return photo_op_check(op, reserved, value);
  if (reserved) return 2;
  if (!std::isfinite(value)) return 3;
  if (op == AUGMENT_HUE) return value < 0.0 || value > 255.0 || value != (double)(int)value ? 6 : 0;
  return value < 0.0 || value > kAugmentBlurMaxRadius ? 7 : 0;
}

PHOTO_FN int augment_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// convert("HSV") of one pixel
PHOTO_FN void augment_rgb2hsv(int R, int G, int B, int* H, int* S, int* V)
{
  const int mx = R > G ? (R > B ? R : B) : (G > B ? G : B), mn = R < G ? (R < B ? R : B) : (G < B ? G : B);
  *V = mx;
  if (mx == mn) { *H = 0; *S = 0; return; }
  const float cr = (float)(mx - mn);
  const float s = cr / (float)mx;
  const float rc = (float)(mx - R) / cr, gc = (float)(mx - G) / cr, bc = (float)(mx - B) / cr;
  float h;
  if (R == mx) h = bc - gc;
  else if (G == mx) h = (float)((2.0 + (double)rc) - (double)bc);
  else h = (float)((4.0 + (double)gc) - (double)rc);
  const double t = (double)h / 6.0 + 1.0;            // in [2/3, 11/6]
  h = (float)(t >= 1.0 ? t - 1.0 : t);               // fmod(t, 1.0): both are exact there
  *H = augment_clip8((int)((double)h * 255.0));
  *S = augment_clip8((int)((double)s * 255.0));
}

// round half away from zero of a value that is not negative, clipped to 0 .. 255
PHOTO_FN int augment_round8(double v) { return augment_clip8((int)std::round(v)); }

// convert("RGB") of one HSV pixel
PHOTO_FN void augment_hsv2rgb(int H, int S, int V, int* R, int* G, int* B)
{
  if (S == 0) { *R = V; *G = V; *B = V; return; }
  const double hf = (double)(float)H * 6.0 / 255.0;
  const int i = (int)std::floor(hf);
  const float f = (float)(hf - (double)(float)i);
  const float fs = (float)((double)S / 255.0);
  const double v = (double)V;
  const int p = augment_round8(v * (1.0 - (double)fs));
  const int q = augment_round8(v * (1.0 - (double)(fs * f)));                   // (the product in float)
  const int t = augment_round8(v * (1.0 - (double)fs * (1.0 - (double)f)));     // (all in double)
  switch (i % 6) {
    case 0: *R = V; *G = t; *B = p; break;
    case 1: *R = q; *G = V; *B = p; break;
    case 2: *R = p; *G = V; *B = t; break;
    case 3: *R = p; *G = q; *B = V; break;
    case 4: *R = t; *G = p; *B = V; break;
    default: *R = V; *G = p; *B = q; break;
  }
}

// HUE with shift d for one pixel
PHOTO_FN void augment_hue(int d, int R, int G, int B, int* r, int* g, int* b)
{
  int H, S, V;
  augment_rgb2hsv(R, G, B, &H, &S, &V);
  augment_hsv2rgb((H + d) & 255, S, V, r, g, b);
}

// ImageFilter.GaussianBlur(radius) as three extended box blurs: the box's real radius in single precision, one rounding per operation, then its whole
// part r, the weight ww of a whole sample and fw of the two fractional ones (of 1 << 24).  radius: finite, 0 .. kAugmentBlurMaxRadius.
inline void augment_gaussian_box(double radius, int* r, uint32_t* ww, uint32_t* fw)
{
  const float rho = (float)radius;
  const float sigma2 = rho * rho / 3.0f;
  const float L = (float)std::sqrt(12.0 * (double)sigma2 + 1.0);
  const float l = (float)std::floor(((double)L - 1.0) / 2.0);
  float a = (2.0f * l + 1.0f) * (l * (l + 1.0f) - 3.0f * sigma2);
  a = a / (6.0f * (sigma2 - (l + 1.0f) * (l + 1.0f)));
  const float fr = l + a;
  *r = (int)fr;
  *ww = (uint32_t)((float)(1 << 24) / (fr * 2.0f + 1.0f));
  *fw = ((1u << 24) - (uint32_t)(2 * *r + 1) * *ww) / 2u;
}

// one sample of a box pass: sum over the 2 r + 1 whole samples, le and re the two beyond them (32-bit unsigned, as Pillow's accumulator)
PHOTO_FN uint32_t augment_box_sample(uint32_t sum, uint32_t le, uint32_t re, uint32_t ww, uint32_t fw)
{
  return (ww * sum + fw * (le + re) + (1u << 23)) >> 24;
}

// One box pass over a line of n samples `stride` bytes apart, with a running window sum; indices clamp to 0 .. n - 1.  in and out do not overlap.
PHOTO_FN void augment_box_line(const uint8_t* in, uint8_t* out, int n, int stride, int r, uint32_t ww, uint32_t fw)
{
  const int last = n - 1;
  uint32_t sum = 0;
  for (int k = -r; k <= r; k++) sum += in[(k < 0 ? 0 : (k > last ? last : k)) * stride];
  uint32_t le = in[0];                                       // in[c(x - r - 1)], x = 0
  for (int x = 0; x < n; x++) {
    const int ir = x + r + 1, il = x - r;
    const uint32_t re = in[(ir > last ? last : ir) * stride];
    out[x * stride] = (uint8_t)augment_box_sample(sum, le, re, ww, fw);
    le = in[(il < 0 ? 0 : il) * stride];                     // (il <= x <= last)
    sum += re - le;
  }
}

}  // namespace hipdec
