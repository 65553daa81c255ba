// project_host.h — the host side of the projective stage's arithmetic (include/heif_hipdec.h, hipdec_tensor_project): the record an entry has in the per-call
// table of k_project (project_kernels.h), the refusals a map alone decides, and the two map helpers (hipdec_quad_map, hipdec_perspective_map).
// Plain C++ without a HIP dependency, as warp_host.h: color.hip includes it.
#pragma once
#include <cmath>
#include <cstdint>

namespace hipdec {

enum ProjectKind { PROJECT_PERSPECTIVE = 0, PROJECT_QUAD = 1 };   // hipdec_tensor_projection.kind

// One entry of the per-call table, 16 words of 8 bytes: uniform per workgroup, read by scalar loads (project_kernels.h project_entry_load)
struct ProjectEntry {
  const uint8_t* src;       // the entry's sh x sw x 3 sample
  uint8_t* o0;              // the entry's first output element
  double a[8];              // the map
  int32_t kind, domain;     // ProjectKind, hipdec_fill_domain
  float value[3];           // the fill
  int32_t reserved;
  uint64_t pad[3];
};
static_assert(sizeof(ProjectEntry) == 128, "the kernel reads 16 words");

constexpr double kProjectCoordLimit = 32000.0;           // |coefficient| and |mapped corner| stay below it, as kWarpCoordLimit
constexpr double kProjectMinDenominator = 1.0 / 1048576;   // 2^-20

// the two coordinate functions, operator for operator as the header states them (-ffp-contract=off: no fused multiply-add)
inline double project_denominator(const double* a, double xc, double yc) { return a[6] * xc + a[7] * yc + 1.0; }
inline void project_point(const double* a, int kind, double xc, double yc, double* xin, double* yin)
{
  if (kind == PROJECT_QUAD) {
    *xin = a[0] + a[1] * xc + a[2] * yc + a[3] * xc * yc;
    *yin = a[4] + a[5] * xc + a[6] * yc + a[7] * xc * yc;
  } else {
    *xin = (a[0] * xc + a[1] * yc + a[2]) / project_denominator(a, xc, yc);
    *yin = (a[3] * xc + a[4] * yc + a[5]) / project_denominator(a, xc, yc);
  }
}

// What a map alone decides for an output of ow x oh.  0: taken; 1: a non-finite coefficient; 2: |a[i]| >= 32000; 3: a corner of [0, ow] x [0, oh] maps to a
// coordinate of magnitude >= 32000; 4: PERSPECTIVE, the denominator at a corner is below 2^-20.  *which: the coefficient's index (1, 2) or the corner's
// (3, 4: bit 0 the x end, bit 1 the y end).
// Why the four corners decide for every pixel centre (all of which lie inside the rectangle): the denominator a6 * x + a7 * y + 1 is linear, so its minimum
// over the rectangle is at a corner.  Over a region where the denominator is positive a linear-fractional function is quasi-linear (its sets {f <= t} and
// {f >= t} are half-planes cut by the region), so it takes its extremes at the vertices; a QUAD map is bilinear - linear along every row and every column
// - and takes its extremes there too.  So the true |xin|, |yin| are below 32000 at every pixel centre.
// The floor of 2^-20, not 0, is what carries this over to the COMPUTED values.  The computed denominator is three rounded operations on terms of magnitude
// T < 32000 * max(ow, oh); its absolute error is at most 3 * T * 2^-53.  For outputs up to 2^15 a side that is 3 * 2^-23 < 2^-21: a true denominator of
// 2^-20 or more cannot become zero or negative (no division by zero, no NaN, no change of sign), and it is computed to a relative error below 1 / 2, so a
// computed quotient stays within a factor of two of the true one - far inside what Pillow's (int) conversions hold.  Pillow therefore never leaves the
// paths the header restates, and neither does the kernel.
inline int project_map_check(const double* a, int kind, int ow, int oh, int* which)
{
  for (int i = 0; i < 8; i++) if (!std::isfinite(a[i])) { *which = i; return 1; }
  for (int i = 0; i < 8; i++) if (std::fabs(a[i]) >= kProjectCoordLimit) { *which = i; return 2; }
  for (int k = 0; k < 4; k++) {
    const double cx = (k & 1) ? (double)ow : 0.0, cy = (k & 2) ? (double)oh : 0.0;
    if (kind == PROJECT_PERSPECTIVE && !(project_denominator(a, cx, cy) >= kProjectMinDenominator)) { *which = k; return 4; }
    double xin, yin;
    project_point(a, kind, cx, cy, &xin, &yin);
    if (!(std::fabs(xin) < kProjectCoordLimit) || !(std::fabs(yin) < kProjectCoordLimit)) { *which = k; return 3; }
  }
  return 0;
}

// Pillow's Python arithmetic for Image.transform(size, QUAD, corners): corners = (nw, sw, se, ne) as x, y pairs, width x height the OUTPUT size
inline void project_quad_map(const double* c, int width, int height, double* a)
{
  const double nwx = c[0], nwy = c[1], swx = c[2], swy = c[3], sex = c[4], sey = c[5], nex = c[6], ney = c[7];
  const double As = 1.0 / (double)width, At = 1.0 / (double)height;
  a[0] = nwx; a[1] = (nex - nwx) * As; a[2] = (swx - nwx) * At; a[3] = (sex - swx - nex + nwx) * As * At;
  a[4] = nwy; a[5] = (ney - nwy) * As; a[6] = (swy - nwy) * At; a[7] = (sey - swy - ney + nwy) * As * At;
}

// torchvision's _get_perspective_coeffs as a linear system: per point pair (s: startpoint, e: endpoint) the rows [ex, ey, 1, 0, 0, 0, -sx*ex, -sx*ey | sx]
// and [0, 0, 0, ex, ey, 1, -sy*ex, -sy*ey | sy]; solved in double by Gaussian elimination with partial pivoting.  false: the system is singular - a pivot is
// zero up to the rounding of the elimination (64 ulps of its column's largest entry: three collinear points leave a residue, not a zero) - or the
// solution is not finite.
inline bool project_perspective_map(const double* start, const double* end, double* a)
{
  double M[8][9];
  for (int p = 0; p < 4; p++) {
    const double sx = start[2 * p], sy = start[2 * p + 1], ex = end[2 * p], ey = end[2 * p + 1];
    const double r0[9] = {ex, ey, 1.0, 0.0, 0.0, 0.0, -sx * ex, -sx * ey, sx};
    const double r1[9] = {0.0, 0.0, 0.0, ex, ey, 1.0, -sy * ex, -sy * ey, sy};
    for (int j = 0; j < 9; j++) { M[2 * p][j] = r0[j]; M[2 * p + 1][j] = r1[j]; }
  }
  for (int i = 0; i < 8; i++)
    for (int j = 0; j < 9; j++)
      if (!std::isfinite(M[i][j])) return false;
  double scale[8];
  for (int j = 0; j < 8; j++) {
    scale[j] = 0.0;
    for (int i = 0; i < 8; i++) scale[j] = std::fmax(scale[j], std::fabs(M[i][j]));
  }
  for (int col = 0; col < 8; col++) {
    int piv = col;
    for (int r = col + 1; r < 8; r++) if (std::fabs(M[r][col]) > std::fabs(M[piv][col])) piv = r;
    if (std::fabs(M[piv][col]) <= 64.0 * 2.220446049250313e-16 * scale[col]) return false;
    if (piv != col) for (int j = 0; j < 9; j++) { const double t = M[col][j]; M[col][j] = M[piv][j]; M[piv][j] = t; }
    for (int r = col + 1; r < 8; r++) {
      const double f = M[r][col] / M[col][col];
      if (f == 0.0) continue;
      for (int j = col; j < 9; j++) M[r][j] -= f * M[col][j];
    }
  }
  for (int i = 7; i >= 0; i--) {
    double v = M[i][8];
    for (int j = i + 1; j < 8; j++) v -= M[i][j] * a[j];
    a[i] = v / M[i][i];
    if (!std::isfinite(a[i])) return false;
  }
  return true;
}

}  // namespace hipdec
