// warp_host.h — the host side of the warp stage's arithmetic (include/heif_hipdec.h, hipdec_tensor_warp): the record an entry has in the per-call table of
// k_warp (warp_kernels.h), the refusals a map alone decides, Pillow's fixed-point values and the running-sum index tables of its scale path.
// Plain C++ without a HIP dependency: color.hip includes it, and tests/emu/warp_tables_asan.cc runs it under AddressSanitizer as a stand-alone program.
#pragma once
#include <cmath>
#include <cstdint>

namespace hipdec {

enum WarpPath { WARP_PATH_DOUBLE = 0,   // BILINEAR / BICUBIC: the six doubles
                WARP_PATH_FIXED = 1,    // NEAREST, a1 or a3 non-zero: 16.16 fixed point
                WARP_PATH_TABLE = 2 };  // NEAREST, a1 == 0 && a3 == 0: the index tables xt / yt

// One entry of the per-call table, 16 words of 8 bytes: uniform per workgroup, read by scalar loads (warp_kernels.h warp_entry_load)
struct WarpEntry {
  const uint8_t* src;       // the entry's sh x sw x 3 sample
  uint8_t* o0;              // the entry's first output element
  double m[6];              // WARP_PATH_DOUBLE
  int32_t A[6];             // WARP_PATH_FIXED: A0 .. A5
  const int32_t* xt;        // WARP_PATH_TABLE: ow column indices, oh row indices (device memory, behind the entries)
  const int32_t* yt;
  int32_t path, domain;     // WarpPath, hipdec_fill_domain
  float value[3];           // the fill
  int32_t reserved;
};
static_assert(sizeof(WarpEntry) == 128, "the kernel reads 16 words");

constexpr double kWarpCoordLimit = 32000.0;   // |coefficient| and |mapped corner| stay below it (Pillow's own bound is 32768)

inline int warp_floor(double v) { return v < 0.0 ? (int)std::floor(v) : (int)v; }
inline int warp_coord(double v) { return v < 0.0 ? -1 : (int)v; }

// What a map alone decides for an output of ow x oh.  0: taken; 1: a non-finite coefficient; 2: |m[i]| >= 32000; 3: a corner of [0, ow] x [0, oh] maps to a
// coordinate of magnitude >= 32000.  *which: the coefficient's index (1, 2) or the corner's (3: bit 0 the x end, bit 1 the y end).
inline int warp_map_check(const double* a, int ow, int oh, int* which)
{
  for (int i = 0; i < 6; i++) if (!std::isfinite(a[i])) { *which = i; return 1; }
  for (int i = 0; i < 6; i++) if (std::fabs(a[i]) >= kWarpCoordLimit) { *which = i; return 2; }
  for (int k = 0; k < 4; k++) {
    const double cx = (k & 1) ? (double)ow : 0.0, cy = (k & 2) ? (double)oh : 0.0;
    const double xin = a[0] * cx + a[1] * cy + a[2], yin = a[3] * cx + a[4] * cy + a[5];
    if (!(std::fabs(xin) < kWarpCoordLimit) || !(std::fabs(yin) < kWarpCoordLimit)) { *which = k; return 3; }
  }
  return 0;
}

inline bool warp_scale_only(const double* a) { return a[1] == 0.0 && a[3] == 0.0; }

// FIX(v) = FLOOR(v * 65536.0 + 0.5); a checked map keeps every product below 2^31
inline int32_t warp_fix(double v) { return (int32_t)warp_floor(v * 65536.0 + 0.5); }
inline void warp_fixed_values(const double* a, int32_t (&A)[6])
{
  A[0] = warp_fix(a[0]); A[1] = warp_fix(a[1]); A[3] = warp_fix(a[3]); A[4] = warp_fix(a[4]);
  A[2] = warp_fix(a[2] + a[0] * 0.5 + a[1] * 0.5);
  A[5] = warp_fix(a[5] + a[3] * 0.5 + a[4] * 0.5);
}

// t[i] = COORD(o), o starting at offset + step * 0.5 and o += step after each i: a running sum, sequential as Pillow's
inline void warp_scale_table(double offset, double step, int n, int32_t* t)
{
  double o = offset + step * 0.5;
  for (int i = 0; i < n; i++) { t[i] = warp_coord(o); o += step; }
}

}  // namespace hipdec
