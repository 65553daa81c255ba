// color.hip — fused colour stage over decoded planes in HBM (hand-written HIP for gfx950).
//
// Restates, bit-exactly, the ColorConversionOperations that libheif's pipeline planner selects for
// HEIC stills:
//   a9   Op_YCbCr420_to_RGB24/_RGB32        libheif/color-conversion/yuv2rgb.cc:345-426, :481-562
//   a10  Op_YCbCr_to_RGB<u8/u16>            libheif/color-conversion/yuv2rgb.cc:92-292
//   a11  Op_RGB_to_RGB24_32                 libheif/color-conversion/rgb2rgb.cc:72-150 (fused into a10)
//   a12  Op_YCbCr420_to_RRGGBBaa            libheif/color-conversion/yuv2rgb.cc:622-734
//   a13  Op_YCbCr420_bilinear_to_YCbCr444   libheif/color-conversion/chroma_sampling.cc:501-724
//   a14  Op_to_sdr_planes                   libheif/color-conversion/hdr_sdr.cc:146-244
//   a15  get_YCbCr_to_RGB_coefficients      libheif/nclx.cc:84-173
//
// Roofline: pure streaming, HBM-bound.  Algorithmic bytes per luma pixel: 1.5*s in + 3*s_out out
// (RGB24 from 8-bit 4:2:0: 4.5 B/px).  Each thread converts a 4x2 luma block so that the chroma
// pair is read once, Y is read as one dword per row and RGB24 leaves as one 12-byte store per row
// (64 lanes -> 768 contiguous bytes per wave-store).
// Float parity: compiled with -ffp-contract=off; the reference build (x86-64 baseline) has no FMA.
#include "hipdec_internal.h"
#include "color_device.h"
#include "warp_host.h"
#include "project_host.h"
#define PHOTO_FN __host__ __device__ inline
#include "photo_lut.h"
#include "augment_lut.h"
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <atomic>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>

namespace {

using namespace hipdec::colordev;


// the store paths of a 4-pixel group of row yy starting at pixel x0 (npx of them inside the picture): one 12-byte store for RGB24, 16 bytes for RGBA32,
// two 12-byte stores for RRGGBB, dwords per plane for the planar layout; byte stores where the group is cut or the destination is not aligned
template <typename Pix, int LAYOUT>
__device__ __forceinline__ void store_rgb4(const ColorParams& p, int x0, int yy, int npx, const int (&R)[4], const int (&G)[4], const int (&B)[4], const uint32_t (&A)[4])
{
  if (LAYOUT == LO_PLANAR) {
    HIPDEC_GLOBAL Pix* r = (HIPDEC_GLOBAL Pix*)((HIPDEC_GLOBAL uint8_t*)p.o0 + (size_t)yy * p.os) + x0;
    HIPDEC_GLOBAL Pix* g = (HIPDEC_GLOBAL Pix*)((HIPDEC_GLOBAL uint8_t*)p.o1 + (size_t)yy * p.os) + x0;
    HIPDEC_GLOBAL Pix* b = (HIPDEC_GLOBAL Pix*)((HIPDEC_GLOBAL uint8_t*)p.o2 + (size_t)yy * p.os) + x0;
    if (npx == 4 && sizeof(Pix) == 1 && ((p.os | (uintptr_t)p.o0 | (uintptr_t)p.o1 | (uintptr_t)p.o2) & 3) == 0) {
      *(HIPDEC_GLOBAL uint32_t*)r = R[0] | (R[1] << 8) | (R[2] << 16) | ((uint32_t)R[3] << 24);
      *(HIPDEC_GLOBAL uint32_t*)g = G[0] | (G[1] << 8) | (G[2] << 16) | ((uint32_t)G[3] << 24);
      *(HIPDEC_GLOBAL uint32_t*)b = B[0] | (B[1] << 8) | (B[2] << 16) | ((uint32_t)B[3] << 24);
    } else if (npx == 4 && sizeof(Pix) == 2 && ((p.os | (uintptr_t)p.o0 | (uintptr_t)p.o1 | (uintptr_t)p.o2) & 7) == 0) {
      *(HIPDEC_GLOBAL uint2*)r = make_uint2(R[0] | (R[1] << 16), R[2] | (R[3] << 16));
      *(HIPDEC_GLOBAL uint2*)g = make_uint2(G[0] | (G[1] << 16), G[2] | (G[3] << 16));
      *(HIPDEC_GLOBAL uint2*)b = make_uint2(B[0] | (B[1] << 16), B[2] | (B[3] << 16));
    } else {
      for (int i = 0; i < npx; i++) { r[i] = (Pix)R[i]; g[i] = (Pix)G[i]; b[i] = (Pix)B[i]; }
    }
  } else if (LAYOUT == LO_RGB24) {
    HIPDEC_GLOBAL uint8_t* o = (HIPDEC_GLOBAL uint8_t*)p.o0 + (size_t)yy * p.os + (size_t)x0 * 3;
    if (npx == 4 && ((p.os | (uintptr_t)p.o0) & 3) == 0) {
      U3 v;
      v.a = R[0] | (G[0] << 8) | (B[0] << 16) | ((uint32_t)R[1] << 24);
      v.b = G[1] | (B[1] << 8) | (R[2] << 16) | ((uint32_t)G[2] << 24);
      v.c = B[2] | (R[3] << 8) | (G[3] << 16) | ((uint32_t)B[3] << 24);
      *(HIPDEC_GLOBAL U3*)o = v;
    } else {
      for (int i = 0; i < npx; i++) { o[3 * i] = (uint8_t)R[i]; o[3 * i + 1] = (uint8_t)G[i]; o[3 * i + 2] = (uint8_t)B[i]; }
    }
  } else if (LAYOUT == LO_RGBA32) {
    HIPDEC_GLOBAL uint8_t* o = (HIPDEC_GLOBAL uint8_t*)p.o0 + (size_t)yy * p.os + (size_t)x0 * 4;
    if (npx == 4 && ((p.os | (uintptr_t)p.o0) & 15) == 0) {
      uint4 v;
      v.x = R[0] | (G[0] << 8) | (B[0] << 16) | (A[0] << 24);
      v.y = R[1] | (G[1] << 8) | (B[1] << 16) | (A[1] << 24);
      v.z = R[2] | (G[2] << 8) | (B[2] << 16) | (A[2] << 24);
      v.w = R[3] | (G[3] << 8) | (B[3] << 16) | (A[3] << 24);
      *(HIPDEC_GLOBAL uint4*)o = v;
    } else {
      for (int i = 0; i < npx; i++) { o[4 * i] = (uint8_t)R[i]; o[4 * i + 1] = (uint8_t)G[i]; o[4 * i + 2] = (uint8_t)B[i]; o[4 * i + 3] = (uint8_t)A[i]; }
    }
  } else {  // RRGGBB BE / LE, yuv2rgb.cc:717-723
    HIPDEC_GLOBAL uint8_t* o = (HIPDEC_GLOBAL uint8_t*)p.o0 + (size_t)yy * p.os + (size_t)x0 * 6;
    const bool le = LAYOUT == LO_RRGGBB_LE;
    uint16_t s[12];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      int r = R[i], g = G[i], b = B[i];
      if (!le) { r = ((r & 255) << 8) | (r >> 8); g = ((g & 255) << 8) | (g >> 8); b = ((b & 255) << 8) | (b >> 8); }
      s[3 * i] = (uint16_t)r; s[3 * i + 1] = (uint16_t)g; s[3 * i + 2] = (uint16_t)b;
    }
    if (npx == 4 && ((p.os | (uintptr_t)p.o0) & 3) == 0) {
      U3 v0, v1;
      v0.a = s[0] | ((uint32_t)s[1] << 16); v0.b = s[2] | ((uint32_t)s[3] << 16); v0.c = s[4] | ((uint32_t)s[5] << 16);
      v1.a = s[6] | ((uint32_t)s[7] << 16); v1.b = s[8] | ((uint32_t)s[9] << 16); v1.c = s[10] | ((uint32_t)s[11] << 16);
      ((HIPDEC_GLOBAL U3*)o)[0] = v0; ((HIPDEC_GLOBAL U3*)o)[1] = v1;
    } else {
      for (int i = 0; i < npx * 3; i++) { o[2 * i] = (uint8_t)(s[i] & 255); o[2 * i + 1] = (uint8_t)(s[i] >> 8); }
    }
  }
}

template <typename Pix, int LAYOUT>
__device__ __forceinline__ void rgb_block(const ColorParams& p)
{
  const int bx = blockIdx.x * blockDim.x + threadIdx.x;  // 4-pixel column group
  const int by = blockIdx.y * blockDim.y + threadIdx.y;  // row pair
  const int x0 = bx * 4, y0 = by * 2;
  if (x0 >= p.w || y0 >= p.h) return;
  const int npx = min(4, p.w - x0);
#pragma unroll
  for (int dy = 0; dy < 2; dy++) {
    const int yy = y0 + dy;
    if (yy >= p.h) break;
    HIPDEC_GLOBAL const Pix* yrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.y + (size_t)yy * p.ys);   // (address space 1: see color_device.h)
    HIPDEC_GLOBAL const Pix* cbrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.cb + (size_t)(yy >> p.shiftV) * p.cbs);
    HIPDEC_GLOBAL const Pix* crrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.cr + (size_t)(yy >> p.shiftV) * p.crs);
    int Y[4], CB[4], CR[4];
    if (npx == 4 && sizeof(Pix) == 1 && (((uintptr_t)(yrow + x0)) & 3) == 0) {
      uint32_t v = *(HIPDEC_GLOBAL const uint32_t*)(yrow + x0);
      Y[0] = v & 255; Y[1] = (v >> 8) & 255; Y[2] = (v >> 16) & 255; Y[3] = v >> 24;
    } else if (npx == 4 && sizeof(Pix) == 2 && (((uintptr_t)(yrow + x0)) & 7) == 0) {
      uint2 v = *(HIPDEC_GLOBAL const uint2*)(yrow + x0);
      Y[0] = v.x & 0xffff; Y[1] = v.x >> 16; Y[2] = v.y & 0xffff; Y[3] = v.y >> 16;
    } else {
      for (int i = 0; i < 4; i++) Y[i] = i < npx ? yrow[x0 + i] : 0;
    }
    if (p.arith == AR_MONO) {
#pragma unroll
      for (int i = 0; i < 4; i++) { CB[i] = 0; CR[i] = 0; }
    } else if (p.shiftH) {
      int c0 = x0 >> 1;
      int cbA = cbrow[c0], crA = crrow[c0];
      int cbB = cbA, crB = crA;
      if (npx > 2) { cbB = cbrow[c0 + 1]; crB = crrow[c0 + 1]; }
      CB[0] = CB[1] = cbA; CB[2] = CB[3] = cbB;
      CR[0] = CR[1] = crA; CR[2] = CR[3] = crB;
    } else {
      for (int i = 0; i < 4; i++) { CB[i] = i < npx ? cbrow[x0 + i] : 0; CR[i] = i < npx ? crrow[x0 + i] : 0; }
    }
    int R[4], G[4], B[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (sizeof(Pix) == 2 && (LAYOUT == LO_RGB24 || LAYOUT == LO_RGBA32)) {   // > 8-bit planes to 8-bit interleaved output: Op_to_sdr_planes on either side
        convert_px(p, Y[i] >> p.in_shift, CB[i] >> p.in_shift, CR[i] >> p.in_shift, R[i], G[i], B[i]);
        R[i] >>= p.out_shift; G[i] >>= p.out_shift; B[i] >>= p.out_shift;
      } else convert_px(p, Y[i], CB[i], CR[i], R[i], G[i], B[i]);
    }

    uint32_t A[4] = {255u, 255u, 255u, 255u};
    if (LAYOUT == LO_RGBA32 && p.a) {
      HIPDEC_GLOBAL const uint8_t* arow = (HIPDEC_GLOBAL const uint8_t*)p.a + (size_t)yy * p.as + x0;
      if (npx == 4 && (((uintptr_t)arow) & 3) == 0) {
        const uint32_t v = *(HIPDEC_GLOBAL const uint32_t*)arow;
        A[0] = v & 255u; A[1] = (v >> 8) & 255u; A[2] = (v >> 16) & 255u; A[3] = v >> 24;
      } else {
        for (int i = 0; i < npx; i++) A[i] = arow[i];
      }
    }
    store_rgb4<Pix, LAYOUT>(p, x0, yy, npx, R, G, B, A);
  }
}

template <typename Pix, int LAYOUT>
__global__ __launch_bounds__(256) void k_ycbcr_to_rgb(ColorParams p) { rgb_block<Pix, LAYOUT>(p); }

// all pictures of a batch in ONE launch: blockIdx.z selects the picture's parameter block (grid x / y cover the largest one)
template <typename Pix, int LAYOUT>
__global__ __launch_bounds__(256) void k_ycbcr_to_rgb_batch(const ColorParams* __restrict__ ps)
{
  const ColorParams p = ps[blockIdx.z];   // wave-uniform: scalar loads into SGPRs
  rgb_block<Pix, LAYOUT>(p);
}

// ---- scaled output (thumbnails): nearest neighbour = HeifPixelImage::scale_nearest_neighbor (libheif/image/pixelimage.cc:1783-1972) bit for bit, box =
// the area average defined in include/heif_hipdec.h (not in the reference; integer-exact).  Two forms of each: a plane scaler (Pix in, Pix out) and a
// kernel fused with the colour conversion above (planes in, scaled interleaved RGB out: no full-size or scaled intermediate goes through HBM).
//
// Box, the streaming one.  Bytes per input luma pixel of 8-bit 4:2:0: 1.5 read, 3 / (scale factor)^2 written.  A workgroup of 256 threads owns `tile`
// output pixels of one output row; their boxes tile a span of at most kBoxSpan input columns (the host chooses `tile` that way) and rows [y0, y1).  Every
// thread walks those rows over ITS four columns - one aligned 32-bit load per row for 8-bit samples, 64-bit for 16-bit ones, a wave reads 256 / 512
// contiguous bytes of a row - and keeps four column sums in registers, for the three planes at once so that their loads are in flight together; the column
// sums go to LDS, and after one barrier the thread that owns an output pixel adds the columns of its box, divides ONCE (S + n / 2) / n and hands the three
// averages to the 4-pixel store path.  No division per input sample, no edge case inside the row loop (the cut group at a row's end takes the byte loop
// as a whole), every input sample comes from HBM once (the 4-column group in front of the tile's first box is the neighbour tile's last: L2).
// A box wider than kBoxSpan columns (a 4K plane to 1 x 1 is legal) takes the chunk loop more than once.
constexpr int kBoxSpan = 1024;
template <typename Pix> struct BoxAcc { typedef uint32_t T; };        // 8-bit samples: 2^24 rows fit
template <> struct BoxAcc<uint16_t> { typedef uint64_t T; };          // 16-bit samples: any legal number of rows

struct ScaledParams {
  ColorParams c;     // planes, destination and arithmetic as the full-size kernels get them (c.w / c.h: the SOURCE luma size)
  int ow, oh;        // output size
  int sH, sV;        // subsampling shifts of the source chroma planes (box: c.shiftH / c.shiftV describe the 4:4:4 image the arithmetic was planned for)
  int tile;          // box: output pixels per workgroup
};

// a value every lane of the wave holds alike, moved to a scalar register (a 64-bit division runs on the vector unit even for uniform operands)
__device__ __forceinline__ int wave_uniform(int v)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HIPDEC_HOST_EMU)
  return __builtin_amdgcn_readfirstlane(v);
#else
  return v;
#endif
}

__device__ __forceinline__ void box_range(int o, int pn, int qn, int& a, int& b)
{
  a = (int)((uint64_t)o * (uint64_t)pn / (uint64_t)qn);
  b = (int)((uint64_t)(o + 1) * (uint64_t)pn / (uint64_t)qn);
  if (b <= a) b = a + 1;
}

// sums of rows [y0, y1) over the four columns xs .. xs + 3 of a plane (columns at or behind xend: nothing)
template <typename Pix, typename Acc>
__device__ __forceinline__ void box_columns(const uint8_t* plane, size_t stride, int pw, int xs, int xend, int y0, int y1, Acc (&a)[4])
{
  a[0] = a[1] = a[2] = a[3] = 0;
  if (xs >= xend) return;
  HIPDEC_GLOBAL const uint8_t* row = (HIPDEC_GLOBAL const uint8_t*)plane + (size_t)y0 * stride + (size_t)xs * sizeof(Pix);
  if (xs + 4 <= pw && ((((uintptr_t)plane + (size_t)xs * sizeof(Pix)) | stride) & (4 * sizeof(Pix) - 1)) == 0) {
#pragma unroll 4
    for (int y = y0; y < y1; y++, row += stride) {
      if (sizeof(Pix) == 1) {
        const uint32_t v = *(HIPDEC_GLOBAL const uint32_t*)row;
        a[0] += v & 255u; a[1] += (v >> 8) & 255u; a[2] += (v >> 16) & 255u; a[3] += v >> 24;
      } else {
        const uint2 v = *(HIPDEC_GLOBAL const uint2*)row;
        a[0] += v.x & 0xffffu; a[1] += v.x >> 16; a[2] += v.y & 0xffffu; a[3] += v.y >> 16;
      }
    }
  } else {
    const int n = min(4, pw - xs);
    for (int y = y0; y < y1; y++, row += stride)
      for (int k = 0; k < n; k++) a[k] += ((HIPDEC_GLOBAL const Pix*)row)[k];
  }
}

// pw x ph: the samples that are scaled - the whole plane, or a window of it at (wx, wy) (tensor output); fw: the plane's full width, which bounds the
// row loads.  The pointer is the PLANE's in either case: a window is carried as an offset so that the span still starts at a 4-sample boundary of the plane.
struct BoxPlane { const uint8_t* p; size_t stride; int pw, ph, fw, wx, wy; };

// Box averages of NP planes for output pixel (oxA + threadIdx.x, oy) of a qw x qh result; all 256 threads of the workgroup call it (barriers inside),
// `val` is meaningful where threadIdx.x < nox.  live: planes [0, live) are worked on (wave-uniform).  WINDOW: the planes' wx / wy are applied.
template <typename Pix, int NP, bool WINDOW = false>
__device__ __forceinline__ void box_tile(const BoxPlane (&pl)[NP], int live, int qw, int qh, int oxA, int nox, int oy, typename BoxAcc<Pix>::T (*colsum)[kBoxSpan],
                                         uint32_t (&val)[NP])
{
  typedef typename BoxAcc<Pix>::T Acc;
  const int tid = threadIdx.x;
  const bool owner = tid < nox;
  int x0[NP], x1[NP], y0[NP], y1[NP], base[NP], xb[NP];
  uint64_t S[NP];
  int chunks = 0;
#pragma unroll
  for (int k = 0; k < NP; k++) {
    S[k] = 0; x0[k] = x1[k] = y0[k] = y1[k] = base[k] = xb[k] = 0;
    if (k >= live) continue;
    int xa, t;
    box_range(oxA, pl[k].pw, qw, xa, t);                    // the tile's span of input columns [xa, xb): wave-uniform
    box_range(oxA + nox - 1, pl[k].pw, qw, t, xb[k]);
    box_range(oy, pl[k].ph, qh, y0[k], y1[k]);
    box_range(owner ? oxA + tid : oxA, pl[k].pw, qw, x0[k], x1[k]);
    if (WINDOW) {   // columns and rows of the PLANE from here on; the wave-uniform ones in scalar registers (3 planes x 4 of them: the window form's budget)
      xa = wave_uniform(xa) + pl[k].wx; xb[k] = wave_uniform(xb[k]) + pl[k].wx; x0[k] += pl[k].wx; x1[k] += pl[k].wx;
      y0[k] = wave_uniform(y0[k]) + pl[k].wy; y1[k] = wave_uniform(y1[k]) + pl[k].wy;
    }
    base[k] = xa & ~3;
    chunks = max(chunks, (xb[k] - base[k] + kBoxSpan - 1) / kBoxSpan);
  }
  for (int j = 0; j < chunks; j++) {
    Acc a[NP][4];
#pragma unroll
    for (int k = 0; k < NP; k++) {
      if (k < live) box_columns<Pix, Acc>(pl[k].p, pl[k].stride, pl[k].fw, base[k] + j * kBoxSpan + tid * 4, xb[k], y0[k], y1[k], a[k]);
    }
    if (j) __syncthreads();                                // the owners have finished with the previous chunk's sums
#pragma unroll
    for (int k = 0; k < NP; k++) {
      if (k < live) { colsum[k][tid * 4] = a[k][0]; colsum[k][tid * 4 + 1] = a[k][1]; colsum[k][tid * 4 + 2] = a[k][2]; colsum[k][tid * 4 + 3] = a[k][3]; }
    }
    __syncthreads();
    if (owner) {
#pragma unroll
      for (int k = 0; k < NP; k++) {
        if (k >= live) continue;
        const int cs = base[k] + j * kBoxSpan;
        const int lo = max(x0[k], cs) - cs, hi = min(x1[k], cs + kBoxSpan) - cs;
        for (int x = lo; x < hi; x++) S[k] += colsum[k][x];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NP; k++) {
    const uint64_t n = (uint64_t)(x1[k] - x0[k]) * (uint64_t)(y1[k] - y0[k]);
    val[k] = (k < live && owner) ? (uint32_t)((S[k] + n / 2) / n) : 0u;
  }
}

// the per-pixel arithmetic of rgb_block for one group of four
template <typename Pix, int LAYOUT>
__device__ __forceinline__ void convert4(const ColorParams& p, const int (&Y)[4], const int (&CB)[4], const int (&CR)[4], int (&R)[4], int (&G)[4], int (&B)[4])
{
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (sizeof(Pix) == 2 && (LAYOUT == LO_RGB24 || LAYOUT == LO_RGBA32)) {
      convert_px(p, Y[i] >> p.in_shift, CB[i] >> p.in_shift, CR[i] >> p.in_shift, R[i], G[i], B[i]);
      R[i] >>= p.out_shift; G[i] >>= p.out_shift; B[i] >>= p.out_shift;
    } else convert_px(p, Y[i], CB[i], CR[i], R[i], G[i], B[i]);
  }
}

template <typename Pix, int LAYOUT>
__device__ __forceinline__ void box_rgb_block(const ScaledParams& sp)
{
  __shared__ typename BoxAcc<Pix>::T colsum[3][kBoxSpan];
  __shared__ uint32_t avg[3][256];
  const ColorParams& p = sp.c;
  const int tid = threadIdx.x;
  const int oxA = blockIdx.x * sp.tile;
  if (oxA >= sp.ow) return;                               // (the whole workgroup)
  const int nox = min(sp.tile, sp.ow - oxA);
  const bool mono = p.arith == AR_MONO;
  const int cw = (p.w + (1 << sp.sH) - 1) >> sp.sH, ch = (p.h + (1 << sp.sV) - 1) >> sp.sV;
  const BoxPlane pl[3] = {{p.y, p.ys, p.w, p.h, p.w, 0, 0}, {p.cb, p.cbs, cw, ch, cw, 0, 0}, {p.cr, p.crs, cw, ch, cw, 0, 0}};
  for (int oy = blockIdx.y; oy < sp.oh; oy += gridDim.y) {
    uint32_t v[3];
    box_tile<Pix, 3>(pl, mono ? 1 : 3, sp.ow, sp.oh, oxA, nox, oy, colsum, v);
    avg[0][tid] = v[0]; avg[1][tid] = v[1]; avg[2][tid] = v[2];
    __syncthreads();
    if (tid * 4 < nox) {
      const int npx = min(4, nox - tid * 4);
      int Y[4], CB[4], CR[4], R[4], G[4], B[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { Y[i] = (int)avg[0][(tid * 4 + i) & 255]; CB[i] = (int)avg[1][(tid * 4 + i) & 255]; CR[i] = (int)avg[2][(tid * 4 + i) & 255]; }
      convert4<Pix, LAYOUT>(p, Y, CB, CR, R, G, B);
      const uint32_t A[4] = {255u, 255u, 255u, 255u};
      store_rgb4<Pix, LAYOUT>(p, oxA + tid * 4, oy, npx, R, G, B, A);
    }
    __syncthreads();                                      // avg and colsum are written again by the next row
  }
}

// nearest neighbour: out(x, y) = full(x * W / ow, y * H / oh) where `full` is what rgb_block writes - only the sampled pixels are read
template <typename Pix, int LAYOUT>
__device__ __forceinline__ void nearest_rgb_block(const ScaledParams& sp)
{
  const ColorParams& p = sp.c;
  const int ox0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (ox0 >= sp.ow) return;
  const int npx = min(4, sp.ow - ox0);
  const bool mono = p.arith == AR_MONO;
  for (int oy = blockIdx.y * blockDim.y + threadIdx.y; oy < sp.oh; oy += gridDim.y * blockDim.y) {
    const int iy = (int)((uint64_t)oy * (uint64_t)p.h / (uint64_t)sp.oh);
    HIPDEC_GLOBAL const Pix* yrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.y + (size_t)iy * p.ys);
    HIPDEC_GLOBAL const Pix* cbrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.cb + (size_t)(iy >> sp.sV) * p.cbs);
    HIPDEC_GLOBAL const Pix* crrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.cr + (size_t)(iy >> sp.sV) * p.crs);
    int Y[4], CB[4], CR[4], R[4], G[4], B[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int ix = (int)((uint64_t)min(ox0 + i, sp.ow - 1) * (uint64_t)p.w / (uint64_t)sp.ow);
      Y[i] = yrow[ix];
      CB[i] = mono ? 0 : cbrow[ix >> sp.sH];
      CR[i] = mono ? 0 : crrow[ix >> sp.sH];
    }
    convert4<Pix, LAYOUT>(p, Y, CB, CR, R, G, B);
    const uint32_t A[4] = {255u, 255u, 255u, 255u};
    store_rgb4<Pix, LAYOUT>(p, ox0, oy, npx, R, G, B, A);
  }
}

template <typename Pix, int LAYOUT>
__global__ __launch_bounds__(256) void k_scale_rgb_box(ScaledParams sp) { box_rgb_block<Pix, LAYOUT>(sp); }
template <typename Pix, int LAYOUT>
__global__ __launch_bounds__(256) void k_scale_rgb_nearest(ScaledParams sp) { nearest_rgb_block<Pix, LAYOUT>(sp); }
// all items of a batch in ONE launch, as k_ycbcr_to_rgb_batch: blockIdx.z selects the parameter block
template <typename Pix, int LAYOUT>
__global__ __launch_bounds__(256) void k_scale_rgb_box_batch(const ScaledParams* __restrict__ ps)
{
  const ScaledParams sp = ps[blockIdx.z];
  box_rgb_block<Pix, LAYOUT>(sp);
}
template <typename Pix, int LAYOUT>
__global__ __launch_bounds__(256) void k_scale_rgb_nearest_batch(const ScaledParams* __restrict__ ps)
{
  const ScaledParams sp = ps[blockIdx.z];
  nearest_rgb_block<Pix, LAYOUT>(sp);
}

// ---- tensor output: a window of the picture, scaled to one common size, as float16 / bfloat16 / float32 / uint8 in a dense N x 3 x H x W or N x H x W x 3
// tensor (include/heif_hipdec.h).  The integer stage is the scaled kernels' - box_tile over the window, convert4 - and the store path is new: the component
// value V becomes (float)V * scale[c] + bias[c] (a multiply and an add, each rounded once: -ffp-contract=off), narrowed with round-to-nearest-even, and a lane
// writes its four pixels as one 16 / 8 / 4-byte store per channel plane (NCHW) or as one run of 12 elements (NHWC).  A horizontal flip is a store index.
// Traffic is the box kernel's: 1.5 bytes read per luma pixel of the window (8-bit 4:2:0), 3 * sizeof(element) written per OUTPUT pixel.
enum TensorDtype { TD_U8 = 0, TD_F32 = 1, TD_F16 = 2, TD_BF16 = 3 };

struct TensorParams {
  ColorParams c;            // planes and arithmetic (c.w / c.h: the source luma size; c.o0: the entry's first element)
  int ow, oh;               // output size
  int sH, sV;               // subsampling shifts of the source chroma planes
  int tile;                 // box: output pixels per workgroup
  int left, top, rw, rh;    // the window, in luma samples
  int flip, nhwc;
  float scale[3], bias[3];
};

// IEEE round-to-nearest-even narrowing in integer arithmetic (subnormals included): the host build's conversions, and the statement the device's
// v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32 are held to bit for bit (tests/test_tensor_gpu.py compares bit patterns)
__host__ __device__ __attribute__((unused)) inline uint32_t f32_to_f16_rne(uint32_t x)
{
  const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
  if (a >= 0x7f800000u) return sign | 0x7c00u | (a > 0x7f800000u ? 0x200u : 0u);
  if (a >= 0x47800000u) return sign | 0x7c00u;                     // 2^16 and above
  const uint32_t e = a >> 23;
  if (e < 113) {                                                     // below 2^-14: a multiple of 2^-24
    if (e < 102) return sign;                                        // below 2^-25
    const uint32_t m = (a & 0x7fffffu) | 0x800000u, sh = 126 - e, half = 1u << (sh - 1), rem = m & ((1u << sh) - 1u);
    uint32_t r = m >> sh;
    if (rem > half || (rem == half && (r & 1u))) r++;
    return sign | r;
  }
  uint32_t r = ((e - 112) << 10) | ((a & 0x7fffffu) >> 13);
  const uint32_t rem = a & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) r++;           // (a carry runs into the exponent, up to infinity)
  return sign | r;
}
__host__ __device__ __attribute__((unused)) inline uint32_t f32_to_bf16_rne(uint32_t x)
{
  if ((x & 0x7fffffffu) > 0x7f800000u) return (x >> 16) | 0x40u;
  return (x + 0x7fffu + ((x >> 16) & 1u)) >> 16;
}

template <int DT> struct TensorElem { typedef uint16_t T; };
template <> struct TensorElem<TD_U8> { typedef uint8_t T; };
template <> struct TensorElem<TD_F32> { typedef uint32_t T; };

// the element (its bit pattern) of component value v
template <int DT>
__device__ __forceinline__ uint32_t tensor_elem(int v, float scale, float bias)
{
  if (DT == TD_U8) return (uint32_t)v;
  const float f = (float)v * scale + bias;
  if (DT == TD_F32) return __builtin_bit_cast(uint32_t, f);
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HIPDEC_HOST_EMU)
  if (DT == TD_F16) return __builtin_bit_cast(uint16_t, (_Float16)f);
  return __builtin_bit_cast(uint16_t, (__bf16)f);
#else
  return DT == TD_F16 ? f32_to_f16_rne(__builtin_bit_cast(uint32_t, f)) : f32_to_bf16_rne(__builtin_bit_cast(uint32_t, f));
#endif
}

// four elements as the 4 * sizeof(element) bytes they occupy in memory
template <int DT> struct TensorQuad;
template <> struct TensorQuad<TD_U8> {
  typedef uint32_t V;
  static __device__ __forceinline__ V pack(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return a | (b << 8) | (c << 16) | (d << 24); }
};
template <> struct TensorQuad<TD_F16> {
  typedef uint2 V;
  static __device__ __forceinline__ V pack(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return make_uint2(a | (b << 16), c | (d << 16)); }
};
template <> struct TensorQuad<TD_BF16> : TensorQuad<TD_F16> {};
template <> struct TensorQuad<TD_F32> {
  typedef uint4 V;
  static __device__ __forceinline__ V pack(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { uint4 v; v.x = a; v.y = b; v.z = c; v.w = d; return v; }
};

// The store path of a 4-pixel group of output row oy starting at pixel x0 (npx of them inside the row).  Flip: pixel x goes to column ow - 1 - x, so a
// whole group lands, reversed, on the four columns from ow - 4 - x0.  Vector stores where the group is whole and its destination aligned to them
// (always, for output widths that are multiples of 4), element stores otherwise.
template <int DT>
__device__ __forceinline__ void store_tensor4(const TensorParams& tp, int x0, int oy, int npx, const int (&R)[4], const int (&G)[4], const int (&B)[4])
{
  typedef typename TensorElem<DT>::T E;
  typedef TensorQuad<DT> Q;
  typedef typename Q::V V;
  uint32_t v[3][4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    v[0][i] = tensor_elem<DT>(tp.flip ? R[3 - i] : R[i], tp.scale[0], tp.bias[0]);
    v[1][i] = tensor_elem<DT>(tp.flip ? G[3 - i] : G[i], tp.scale[1], tp.bias[1]);
    v[2][i] = tensor_elem<DT>(tp.flip ? B[3 - i] : B[i], tp.scale[2], tp.bias[2]);
  }
  const size_t ow = (size_t)tp.ow, oh = (size_t)tp.oh;
  const size_t xs = tp.flip ? ow - (size_t)npx - (size_t)x0 : (size_t)x0;   // the group's first column in memory
  HIPDEC_GLOBAL E* o = (HIPDEC_GLOBAL E*)tp.c.o0;
  if (tp.nhwc) {
    HIPDEC_GLOBAL E* d = o + ((size_t)oy * ow + xs) * 3;
    if (npx == 4 && (((uintptr_t)d) & (4 * sizeof(E) - 1)) == 0) {   // 12 elements in a row: R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
      ((HIPDEC_GLOBAL V*)d)[0] = Q::pack(v[0][0], v[1][0], v[2][0], v[0][1]);
      ((HIPDEC_GLOBAL V*)d)[1] = Q::pack(v[1][1], v[2][1], v[0][2], v[1][2]);
      ((HIPDEC_GLOBAL V*)d)[2] = Q::pack(v[2][2], v[0][3], v[1][3], v[2][3]);
      return;
    }
  } else {
    HIPDEC_GLOBAL E* r = o + ((size_t)oy) * ow + xs;
    HIPDEC_GLOBAL E* g = r + oh * ow;
    HIPDEC_GLOBAL E* b = g + oh * ow;
    if (npx == 4 && ((((uintptr_t)r) | ((uintptr_t)g) | ((uintptr_t)b)) & (4 * sizeof(E) - 1)) == 0) {
      *(HIPDEC_GLOBAL V*)r = Q::pack(v[0][0], v[0][1], v[0][2], v[0][3]);
      *(HIPDEC_GLOBAL V*)g = Q::pack(v[1][0], v[1][1], v[1][2], v[1][3]);
      *(HIPDEC_GLOBAL V*)b = Q::pack(v[2][0], v[2][1], v[2][2], v[2][3]);
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i >= npx) break;
    const int k = tp.flip ? 3 - i : i;                               // where pixel x0 + i sits in v
    const size_t col = tp.flip ? ow - 1 - (size_t)(x0 + i) : (size_t)(x0 + i);
    if (tp.nhwc) {
      HIPDEC_GLOBAL E* d = o + ((size_t)oy * ow + col) * 3;
      d[0] = (E)v[0][k]; d[1] = (E)v[1][k]; d[2] = (E)v[2][k];
    } else {
      HIPDEC_GLOBAL E* d = o + (size_t)oy * ow + col;
      d[0] = (E)v[0][k]; d[oh * ow] = (E)v[1][k]; d[2 * oh * ow] = (E)v[2][k];
    }
  }
}

// > 8-bit planes: the to-SDR shifts of the parameter block apply where the entry point set them (TD_U8) and are zero for the native-depth value of the
// float dtypes, so one statement of the arithmetic serves both
template <typename Pix>
__device__ __forceinline__ void tensor_convert4(const ColorParams& p, const int (&Y)[4], const int (&CB)[4], const int (&CR)[4], int (&R)[4], int (&G)[4], int (&B)[4])
{
  convert4<Pix, LO_RGB24>(p, Y, CB, CR, R, G, B);
}

// all entries of a tensor in ONE launch: blockIdx.z selects the entry's parameter block
template <typename Pix, int DT>
__global__ __launch_bounds__(256) void k_tensor_box(const TensorParams* __restrict__ ps)
{
  __shared__ typename BoxAcc<Pix>::T colsum[3][kBoxSpan];
  __shared__ uint32_t avg[3][256];
  const TensorParams tp = ps[blockIdx.z];   // wave-uniform: scalar loads into SGPRs
  const ColorParams& p = tp.c;
  const int tid = threadIdx.x;
  const int oxA = blockIdx.x * tp.tile;
  if (oxA >= tp.ow) return;                               // (the whole workgroup)
  const int nox = min(tp.tile, tp.ow - oxA);
  const bool mono = p.arith == AR_MONO;
  // each plane cropped to the window: luma columns [left, left + rw), chroma columns [left >> sH, ((left + rw - 1) >> sH) + 1), the same in y
  const int cl = tp.left >> tp.sH, ct = tp.top >> tp.sV;
  const int cw = ((tp.left + tp.rw - 1) >> tp.sH) - cl + 1, ch = ((tp.top + tp.rh - 1) >> tp.sV) - ct + 1;
  const int fcw = (p.w + (1 << tp.sH) - 1) >> tp.sH;
  const BoxPlane pl[3] = {{p.y, p.ys, tp.rw, tp.rh, p.w, tp.left, tp.top}, {p.cb, p.cbs, cw, ch, fcw, cl, ct}, {p.cr, p.crs, cw, ch, fcw, cl, ct}};
  for (int oy = blockIdx.y; oy < tp.oh; oy += gridDim.y) {
    uint32_t v[3];
    box_tile<Pix, 3, true>(pl, mono ? 1 : 3, tp.ow, tp.oh, oxA, nox, oy, colsum, v);
    avg[0][tid] = v[0]; avg[1][tid] = v[1]; avg[2][tid] = v[2];
    __syncthreads();
    if (tid * 4 < nox) {
      const int npx = min(4, nox - tid * 4);
      int Y[4], CB[4], CR[4], R[4], G[4], B[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { Y[i] = (int)avg[0][(tid * 4 + i) & 255]; CB[i] = (int)avg[1][(tid * 4 + i) & 255]; CR[i] = (int)avg[2][(tid * 4 + i) & 255]; }
      tensor_convert4<Pix>(p, Y, CB, CR, R, G, B);
      store_tensor4<DT>(tp, oxA + tid * 4, oy, npx, R, G, B);
    }
    __syncthreads();                                      // avg and colsum are written again by the next row
  }
}

// nearest neighbour: V(x, y) = full(left + x * rw / ow, top + y * rh / oh), `full` what rgb_block writes - only the sampled pixels are read
template <typename Pix, int DT>
__global__ __launch_bounds__(256) void k_tensor_nearest(const TensorParams* __restrict__ ps)
{
  const TensorParams tp = ps[blockIdx.z];
  const ColorParams& p = tp.c;
  const int ox0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (ox0 >= tp.ow) return;
  const int npx = min(4, tp.ow - ox0);
  const bool mono = p.arith == AR_MONO;
  for (int oy = blockIdx.y * blockDim.y + threadIdx.y; oy < tp.oh; oy += gridDim.y * blockDim.y) {
    const int iy = tp.top + (int)((uint64_t)oy * (uint64_t)tp.rh / (uint64_t)tp.oh);
    HIPDEC_GLOBAL const Pix* yrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.y + (size_t)iy * p.ys);
    HIPDEC_GLOBAL const Pix* cbrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.cb + (size_t)(iy >> tp.sV) * p.cbs);
    HIPDEC_GLOBAL const Pix* crrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.cr + (size_t)(iy >> tp.sV) * p.crs);
    int Y[4], CB[4], CR[4], R[4], G[4], B[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int ix = tp.left + (int)((uint64_t)min(ox0 + i, tp.ow - 1) * (uint64_t)tp.rw / (uint64_t)tp.ow);
      Y[i] = yrow[ix];
      CB[i] = mono ? 0 : cbrow[ix >> tp.sH];
      CR[i] = mono ? 0 : crrow[ix >> tp.sH];
    }
    tensor_convert4<Pix>(p, Y, CB, CR, R, G, B);
    store_tensor4<DT>(tp, ox0, oy, npx, R, G, B);
  }
}

// ---- oriented output: the tensor kernels with the picture's orientation (irot / imir, include/heif_hipdec.h hipdec_orientation) folded into the store.
// The integer stage runs on the PRE-orientation picture P of t.ow x t.oh pixels exactly as the tensor kernels run it; pixel (x, y) of P is stored at
// displayed position (X, Y).  With code = r + 4 * m:
//   r even:  X = fx ? W - 1 - x : x,  Y = fy ? H - 1 - y : y      (W x H = t.ow x t.oh, displayed W x H)
//   r odd:   X = fx ? H - 1 - y : y,  Y = fy ? W - 1 - x : x      (displayed H x W: a row of P becomes a column)
//   fx = bit 1 of r XOR m, fy = bit 1 of r XOR bit 0 of r.
// An entry's flip is folded into the code by the host, the code is wave-uniform, and entries of all eight codes share a launch.
struct OrientedParams {
  TensorParams t;     // t.ow x t.oh: the size of P; t.flip is 0; t.c.o0: the entry's first element
  uint16_t code;      // hipdec_orientation, 0 .. 7
  uint16_t rb;        // box: rows of P a workgroup takes at a time - the kernel's RB for a quarter turn, fewer (more workgroups) where rows stay rows
  int plane_rows;     // NCHW: a channel plane is plane_rows * pitch elements - the displayed rows for a dense sample, the canvas' rows for a placed one
  uint64_t pitch;     // elements from one DISPLAYED row to the next (dense for tensors, out_stride for RGB24, the canvas row for placed tensors)
};
static_assert(sizeof(OrientedParams) == sizeof(TensorParams) + 16, "the block keeps the size it had before the plane stride: code and rb share a word with it");

// store_tensor4's shape with a row pitch: a 4-pixel group of displayed row `row` (of dh rows of dw pixels) whose pixels are columns x0 .. x0 + npx - 1 before
// the reversal `rev` (column x goes to dw - 1 - x).  Vector stores where the group is whole and its destination aligned, element stores otherwise.
template <int DT>
__device__ __forceinline__ void store_oriented4(const OrientedParams& op, int dw_, int dh_, int rev, int x0, int row, int npx, const int (&R)[4], const int (&G)[4],
                                                const int (&B)[4])
{
  typedef typename TensorElem<DT>::T E;
  typedef TensorQuad<DT> Q;
  typedef typename Q::V V;
  const TensorParams& tp = op.t;
  uint32_t v[3][4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    v[0][i] = tensor_elem<DT>(rev ? R[3 - i] : R[i], tp.scale[0], tp.bias[0]);
    v[1][i] = tensor_elem<DT>(rev ? G[3 - i] : G[i], tp.scale[1], tp.bias[1]);
    v[2][i] = tensor_elem<DT>(rev ? B[3 - i] : B[i], tp.scale[2], tp.bias[2]);
  }
  const size_t dw = (size_t)dw_, pitch = (size_t)op.pitch, plane = (size_t)op.plane_rows * pitch;
  const size_t xs = rev ? dw - (size_t)npx - (size_t)x0 : (size_t)x0;   // the group's first column in memory
  HIPDEC_GLOBAL E* o = (HIPDEC_GLOBAL E*)tp.c.o0 + (size_t)row * pitch;
  if (tp.nhwc) {
    HIPDEC_GLOBAL E* d = o + xs * 3;
    if (npx == 4 && (((uintptr_t)d) & (4 * sizeof(E) - 1)) == 0) {
      ((HIPDEC_GLOBAL V*)d)[0] = Q::pack(v[0][0], v[1][0], v[2][0], v[0][1]);
      ((HIPDEC_GLOBAL V*)d)[1] = Q::pack(v[1][1], v[2][1], v[0][2], v[1][2]);
      ((HIPDEC_GLOBAL V*)d)[2] = Q::pack(v[2][2], v[0][3], v[1][3], v[2][3]);
      return;
    }
  } else {
    HIPDEC_GLOBAL E* r = o + xs;
    HIPDEC_GLOBAL E* g = r + plane;
    HIPDEC_GLOBAL E* b = g + plane;
    if (npx == 4 && ((((uintptr_t)r) | ((uintptr_t)g) | ((uintptr_t)b)) & (4 * sizeof(E) - 1)) == 0) {
      *(HIPDEC_GLOBAL V*)r = Q::pack(v[0][0], v[0][1], v[0][2], v[0][3]);
      *(HIPDEC_GLOBAL V*)g = Q::pack(v[1][0], v[1][1], v[1][2], v[1][3]);
      *(HIPDEC_GLOBAL V*)b = Q::pack(v[2][0], v[2][1], v[2][2], v[2][3]);
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i >= npx) break;
    const int k = rev ? 3 - i : i;                                   // where pixel x0 + i sits in v
    const size_t col = rev ? dw - 1 - (size_t)(x0 + i) : (size_t)(x0 + i);
    if (tp.nhwc) {
      HIPDEC_GLOBAL E* d = o + col * 3;
      d[0] = (E)v[0][k]; d[1] = (E)v[1][k]; d[2] = (E)v[2][k];
    } else {
      HIPDEC_GLOBAL E* d = o + col;
      d[0] = (E)v[0][k]; d[plane] = (E)v[1][k]; d[2 * plane] = (E)v[2][k];
    }
  }
}

// ---- clip output (include/heif_hipdec.h hipdec_clips_to_tensor): the box kernel of the frames of a clip whose rows stay rows and whose row order stays -
// folded codes 0 and 4.  A frame of an N x C x T x H x W clip has its channel planes T * H rows apart, so it needs the row pitch and the plane stride of the
// oriented store, but nothing of k_oriented_box's quarter-turn stage, which caps the column tile at 96 / 64 and stages every pixel in LDS a second time.
// The integer stage is k_tensor_box's, statement for statement - the same box_tile, tile choice (up to 256 columns), LDS and flip as a store index - and
// the store is store_oriented4: vector stores behind its run-time alignment test (a plane stride that is no multiple of four elements leaves the G and B
// planes unaligned: element stores).  A sibling text, as k_patch_box is one of k_oriented_box: k_tensor_box's code object does not change.
// (the occupancy step is stated, as for k_patch_box: left to itself the scheduler took 176 VGPRs for the float dtypes from 16-bit samples, past the 168 step)
template <typename Pix, int DT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sizeof(Pix) == 1 ? 4 : 3))) void k_clip_box(const OrientedParams* __restrict__ ps)
{
  __shared__ typename BoxAcc<Pix>::T colsum[3][kBoxSpan];
  __shared__ uint32_t avg[3][256];
  const OrientedParams op = ps[blockIdx.z];   // wave-uniform: scalar loads into SGPRs
  const TensorParams& tp = op.t;
  const ColorParams& p = tp.c;
  const int tid = threadIdx.x;
  const int oxA = blockIdx.x * tp.tile;
  if (oxA >= tp.ow) return;                               // (the whole workgroup)
  const int nox = min(tp.tile, tp.ow - oxA);
  const bool mono = p.arith == AR_MONO;
  const int fx = (op.code >> 2) & 1;                      // code 0 or 4: the mirror is the only thing left of the orientation
  const int cl = tp.left >> tp.sH, ct = tp.top >> tp.sV;
  const int cw = ((tp.left + tp.rw - 1) >> tp.sH) - cl + 1, ch = ((tp.top + tp.rh - 1) >> tp.sV) - ct + 1;
  const int fcw = (p.w + (1 << tp.sH) - 1) >> tp.sH;
  const BoxPlane pl[3] = {{p.y, p.ys, tp.rw, tp.rh, p.w, tp.left, tp.top}, {p.cb, p.cbs, cw, ch, fcw, cl, ct}, {p.cr, p.crs, cw, ch, fcw, cl, ct}};
  for (int oy = blockIdx.y; oy < tp.oh; oy += gridDim.y) {
    uint32_t v[3];
    box_tile<Pix, 3, true>(pl, mono ? 1 : 3, tp.ow, tp.oh, oxA, nox, oy, colsum, v);
    avg[0][tid] = v[0]; avg[1][tid] = v[1]; avg[2][tid] = v[2];
    __syncthreads();
    if (tid * 4 < nox) {
      const int npx = min(4, nox - tid * 4);
      int Y[4], CB[4], CR[4], R[4], G[4], B[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { Y[i] = (int)avg[0][(tid * 4 + i) & 255]; CB[i] = (int)avg[1][(tid * 4 + i) & 255]; CR[i] = (int)avg[2][(tid * 4 + i) & 255]; }
      tensor_convert4<Pix>(p, Y, CB, CR, R, G, B);
      store_oriented4<DT>(op, tp.ow, tp.oh, fx, oxA + tid * 4, oy, npx, R, G, B);
    }
    __syncthreads();                                      // avg and colsum are written again by the next row
  }
}

// ---- packed tensor output, patch sequences (include/heif_hipdec.h hipdec_batch_to_tensor_packed): the sample of an entry is stored as tokens of P x P
// pixels - token t of the sample starts at element t * 3 * P * P of it - instead of rows.  The element offset of displayed pixel (Y, X), channel 0, is a
// sum of a row part and a column part: with gy = Y / P, py = Y % P, gx = X / P, px = X % P and the merge size m
//   t * 3PP = ((gy / m) * (gw / m) + gx / m) * m * m * 3PP + ((gy % m) * m + gx % m) * 3PP
//   rowoff(Y) = (gy / m) * rowtok + (gy % m) * mtok + py * prow          rowtok = (gw / m) * m * m * 3PP, mtok = m * 3PP, prow = P * pxs
//   coloff(X) = (gx / m) * tokm + (gx % m) * tok + px * pxs              tokm = m * m * 3PP, tok = 3PP
// where pxs is the distance of horizontal neighbours inside a token (1 in Conv2d weight order, 3 in NaFlex order) and chs the distance of the channels
// (P * P, or 1).  Everything in the block is wave-uniform and computed by the host; the divisions by P and m are a multiply-high with floor(2^32 / d) and
// one correction step (exact for every 32-bit dividend: the estimate is short by at most one), five VALU operations each.
struct PatchInfo {
  uint32_t P, m;
  uint32_t magicP, magicM;   // min(floor(2^32 / d), 2^32 - 1)
  uint32_t tok, tokm, mtok;
  uint32_t prow, pxs, chs;
  uint64_t rowtok;
};
static_assert(sizeof(PatchInfo) == 48, "the blocks behind it stay 16-byte multiples");
struct PatchParams { OrientedParams in; PatchInfo b; };

__device__ __forceinline__ uint32_t patch_divmod(uint32_t n, uint32_t d, uint32_t magic, uint32_t& rem)
{
  uint32_t q = (uint32_t)(((uint64_t)n * (uint64_t)magic) >> 32);
  rem = n - q * d;
  if (rem >= d) { q++; rem -= d; }
  return q;
}
__device__ __forceinline__ size_t patch_rowoff(const PatchInfo& b, uint32_t Y)
{
  uint32_t py, ry;
  const uint32_t gy = patch_divmod(Y, b.P, b.magicP, py), my = patch_divmod(gy, b.m, b.magicM, ry);
  return (size_t)my * (size_t)b.rowtok + (size_t)(ry * b.mtok + py * b.prow);
}
__device__ __forceinline__ size_t patch_coloff(const PatchInfo& b, uint32_t X)
{
  uint32_t px, rx;
  const uint32_t gx = patch_divmod(X, b.P, b.magicP, px), mx = patch_divmod(gx, b.m, b.magicM, rx);
  return (size_t)mx * (size_t)b.tokm + (size_t)(rx * b.tok + px * b.pxs);
}

// store_oriented4's shape in token order.  A whole group whose first column in memory is a multiple of 4 lies inside one patch when P % 4 == 0: there it is
// what the dense store has - one vector store per channel (the channels P * P apart) or one run of 12 elements - behind the same runtime alignment test.
// Every other group - any other P, a ragged or unaligned group - takes element stores with the patch found per pixel (the row part once).
template <int DT>
__device__ __forceinline__ void store_patch4(const OrientedParams& op, const PatchInfo& b, int dw_, int rev, int x0, int row, int npx, const int (&R)[4],
                                             const int (&G)[4], const int (&B)[4])
{
  typedef typename TensorElem<DT>::T E;
  typedef TensorQuad<DT> Q;
  typedef typename Q::V V;
  const TensorParams& tp = op.t;
  uint32_t v[3][4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    v[0][i] = tensor_elem<DT>(rev ? R[3 - i] : R[i], tp.scale[0], tp.bias[0]);
    v[1][i] = tensor_elem<DT>(rev ? G[3 - i] : G[i], tp.scale[1], tp.bias[1]);
    v[2][i] = tensor_elem<DT>(rev ? B[3 - i] : B[i], tp.scale[2], tp.bias[2]);
  }
  const uint32_t dw = (uint32_t)dw_;
  const uint32_t xs = rev ? dw - (uint32_t)npx - (uint32_t)x0 : (uint32_t)x0;   // the group's first column in memory
  HIPDEC_GLOBAL E* o = (HIPDEC_GLOBAL E*)tp.c.o0 + patch_rowoff(b, (uint32_t)row);
  if (npx == 4 && ((b.P | xs) & 3u) == 0) {
    HIPDEC_GLOBAL E* d = o + patch_coloff(b, xs);
    if (tp.nhwc) {
      if ((((uintptr_t)d) & (4 * sizeof(E) - 1)) == 0) {
        ((HIPDEC_GLOBAL V*)d)[0] = Q::pack(v[0][0], v[1][0], v[2][0], v[0][1]);
        ((HIPDEC_GLOBAL V*)d)[1] = Q::pack(v[1][1], v[2][1], v[0][2], v[1][2]);
        ((HIPDEC_GLOBAL V*)d)[2] = Q::pack(v[2][2], v[0][3], v[1][3], v[2][3]);
        return;
      }
    } else {
      HIPDEC_GLOBAL E* g = d + b.chs;
      HIPDEC_GLOBAL E* bl = g + b.chs;
      if (((((uintptr_t)d) | ((uintptr_t)g) | ((uintptr_t)bl)) & (4 * sizeof(E) - 1)) == 0) {
        *(HIPDEC_GLOBAL V*)d = Q::pack(v[0][0], v[0][1], v[0][2], v[0][3]);
        *(HIPDEC_GLOBAL V*)g = Q::pack(v[1][0], v[1][1], v[1][2], v[1][3]);
        *(HIPDEC_GLOBAL V*)bl = Q::pack(v[2][0], v[2][1], v[2][2], v[2][3]);
        return;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i >= npx) break;
    const int k = rev ? 3 - i : i;                                   // where pixel x0 + i sits in v
    const uint32_t col = rev ? dw - 1u - (uint32_t)(x0 + i) : (uint32_t)(x0 + i);
    HIPDEC_GLOBAL E* d = o + patch_coloff(b, col);
    d[0] = (E)v[0][k]; d[b.chs] = (E)v[1][k]; d[2 * b.chs] = (E)v[2][k];
  }
}

// The store policies of the nearest and resampling kernel bodies: the dense one is the store the kernels have had (rows of `pitch` elements), the blocked
// one writes token order.  A policy is an argument of the body the way LAYOUT is one of rgb_block.
// Block: the parameter block the kernel reads (the body loads it, as the kernels did); inner(): the block the body works on.
// shown_*(): does a piece of the sample hold a pixel the policy stores?  Constant true for the dense and the blocked store (their kernels' code does not
// know the question was asked); the clipping store of the framed output (FrameStore below) answers from the entry's window, and a body skips the loads of
// a piece that is not shown.  _p: columns / rows of P (the resampler's tiles and bands), _d: of the displayed sample (the nearest kernel's groups and rows).
struct ShowsEverything {
  static __device__ __forceinline__ constexpr bool shown_cols_p(int, int) { return true; }
  static __device__ __forceinline__ constexpr bool shown_rows_p(int, int) { return true; }
  static __device__ __forceinline__ constexpr bool shown_cols_d(int, int) { return true; }
  static __device__ __forceinline__ constexpr bool shown_row_d(int) { return true; }
  static __device__ __forceinline__ constexpr int origin_x() { return 0; }   // what a workgroup adds to blockIdx.x / .y (the framed grid starts at the window)
  static __device__ __forceinline__ constexpr int origin_y() { return 0; }
};
template <typename Blk> struct DenseStore : ShowsEverything {
  typedef Blk Block;
  __device__ __forceinline__ explicit DenseStore(const Blk&) {}
  static __device__ __forceinline__ const Blk& inner(const Blk& k) { return k; }
  template <int DT>
  __device__ __forceinline__ void group4(const OrientedParams& op, int dw, int dh, int rev, int x0, int row, int npx, const int (&R)[4], const int (&G)[4],
                                         const int (&B)[4]) const
  {
    store_oriented4<DT>(op, dw, dh, rev, x0, row, npx, R, G, B);
  }
};
template <typename Blk> struct PatchStore : ShowsEverything {   // Blk: PatchParams, or PatchResampleParams - {the dense block `in`, PatchInfo b}
  typedef Blk Block;
  const PatchInfo& b;
  __device__ __forceinline__ explicit PatchStore(const Blk& k) : b(k.b) {}
  static __device__ __forceinline__ auto inner(const Blk& k) -> decltype((k.in)) { return k.in; }
  template <int DT>
  __device__ __forceinline__ void group4(const OrientedParams& op, int dw, int, int rev, int x0, int row, int npx, const int (&R)[4], const int (&G)[4],
                                         const int (&B)[4]) const
  {
    store_patch4<DT>(op, b, dw, rev, x0, row, npx, R, G, B);
  }
};

// The quarter-turn store of the box kernel.  The box stage has to walk SOURCE rows (box_columns lives on aligned row loads), but a row of P is a COLUMN of
// the displayed picture: stored as it is computed, every element would open a 64-byte segment of its own.  So a workgroup takes RB consecutive rows of P for
// its tile of at most TC columns, stages the converted integer components in LDS (one row of the stage per row of P, one 32-bit word per pixel where the
// component values are 8 bits wide - 8-bit sources, and the U8 dtype of any source - and 64 bits for native-depth values), and then writes along DISPLAYED
// rows: column x of the tile is displayed row Y and receives ONE contiguous run of RB pixels - RB elements per channel plane (NCHW), 3 * RB elements
// (NHWC / RGB24) - with consecutive lanes on consecutive elements.  The float stage runs at that store.
//   RB:  64 where the narrowest element is one byte (a run of 64 bytes per channel plane, 192 interleaved), 32 for native-depth values, whose narrowest
//        element is two bytes (64 / 192 bytes again).  An output lower than RB, or the last block of one, gets the shorter run it has.
//   TC:  96 columns for 8-bit samples, 64 for 16-bit ones (whose column sums are 64-bit).  The host caps the box tile at TC.  (TC = 128 was measured first:
//        48 KB of LDS left three workgroups per CU where k_tensor_box has four, and the kernel ran 30 - 58 % behind it.)
//   LDS: stage rows are padded by one element, so lanes on consecutive stage ROWS of one column - what the write-out reads - are TC + 1 words apart: an odd
//        number of 32-bit banks (twice an odd number for the 64-bit stage, read as b64 over 64 banks), conflict-free over a 32-lane group.  The staging
//        write is lane = column: consecutive words.
//        8-bit:            colsum 3 * 1024 * 4 + stage 64 * 97 * 4  = 12288 + 24832 = 37120 bytes: FOUR workgroups per CU, the step its 120 VGPRs allow
//        16-bit, U8:       colsum 3 * 1024 * 8 + stage 64 * 65 * 4  = 24576 + 16640 = 41216 bytes
//        16-bit, floats:   colsum 24576 + stage 32 * 65 * 8         = 41216 bytes
//        16-bit: below 160 KiB / 3 = 54613, three workgroups per CU, the step of its 168 VGPRs.
// Row-preserving codes go through the same stage - one box loop, one set of registers: with k_tensor_box's avg path beside the stage the kernel took 130 - 138
// VGPRs (8-bit) and 178 - 186 (16-bit), past the 128 / 168 steps - and leave it with k_tensor_box's store shape: 4-pixel groups of row oy or H - 1 - oy,
// columns forward or reversed, vector stores where aligned (store_oriented4).
template <typename Pix, int DT> struct OrientedTile {
  static constexpr bool kNarrow = sizeof(Pix) == 1 || DT == TD_U8;
  static constexpr int TC = sizeof(Pix) == 1 ? 96 : 64;
  static constexpr int RB = kNarrow ? 64 : 32;
};
template <bool NARROW> struct OrientedStage {
  typedef uint32_t S;
  static __device__ __forceinline__ S pack(int r, int g, int b) { return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16); }
  static __device__ __forceinline__ int get(S s, uint32_t ch) { return (int)((s >> (8u * ch)) & 255u); }
};
template <> struct OrientedStage<false> {
  typedef uint2 S;
  static __device__ __forceinline__ S pack(int r, int g, int b) { return make_uint2((uint32_t)r | ((uint32_t)g << 16), (uint32_t)b); }
  static __device__ __forceinline__ int get(S s, uint32_t ch) { return (int)(ch == 0 ? (s.x & 0xffffu) : (ch == 1 ? (s.x >> 16) : s.y)); }
};

template <typename Pix, int DT>
__global__ __launch_bounds__(256) void k_oriented_box(const OrientedParams* __restrict__ ps)
{
  typedef OrientedTile<Pix, DT> T;
  typedef OrientedStage<T::kNarrow> St;
  typedef typename TensorElem<DT>::T E;
  constexpr int RB = T::RB, TC = T::TC;
  __shared__ typename BoxAcc<Pix>::T colsum[3][kBoxSpan];
  __shared__ typename St::S stage[RB][TC + 1];
  const OrientedParams op = ps[blockIdx.z];   // wave-uniform: scalar loads into SGPRs
  const TensorParams& tp = op.t;
  const ColorParams& p = tp.c;
  const int tid = threadIdx.x;
  const int oxA = blockIdx.x * tp.tile;
  if (oxA >= tp.ow) return;                               // (the whole workgroup)
  const int nox = min(tp.tile, tp.ow - oxA);              // <= TC: the host caps the tile
  const bool mono = p.arith == AR_MONO;
  const int quarter = op.code & 1, fx = ((op.code >> 1) ^ (op.code >> 2)) & 1, fy = ((op.code >> 1) ^ op.code) & 1;
  const int cl = tp.left >> tp.sH, ct = tp.top >> tp.sV;
  const int cw = ((tp.left + tp.rw - 1) >> tp.sH) - cl + 1, ch = ((tp.top + tp.rh - 1) >> tp.sV) - ct + 1;
  const int fcw = (p.w + (1 << tp.sH) - 1) >> tp.sH;
  const BoxPlane pl[3] = {{p.y, p.ys, tp.rw, tp.rh, p.w, tp.left, tp.top}, {p.cb, p.cbs, cw, ch, fcw, cl, ct}, {p.cr, p.crs, cw, ch, fcw, cl, ct}};
  const int rb = max(1, min((int)op.rb, RB));                  // (the stage has RB rows whatever the block says)
  for (int yb = blockIdx.y * rb; yb < tp.oh; yb += gridDim.y * rb) {
    const int nrows = min(rb, tp.oh - yb);
    for (int r = 0; r < nrows; r++) {
      uint32_t v[3];
      box_tile<Pix, 3, true>(pl, mono ? 1 : 3, tp.ow, tp.oh, oxA, nox, yb + r, colsum, v);
      if (tid < nox) {                                    // the owner of column oxA + tid converts its own pixel (four copies of it: one statement of the arithmetic)
        const int Y[4] = {(int)v[0], (int)v[0], (int)v[0], (int)v[0]}, CB[4] = {(int)v[1], (int)v[1], (int)v[1], (int)v[1]}, CR[4] = {(int)v[2], (int)v[2], (int)v[2], (int)v[2]};
        int R[4], G[4], B[4];
        tensor_convert4<Pix>(p, Y, CB, CR, R, G, B);
        stage[r][tid] = St::pack(R[0], G[0], B[0]);
      }
      __syncthreads();                                    // colsum is written again by the next row; after the last one the stage is complete
    }
    if (!quarter) {   // k_tensor_box's store shape: 4-pixel groups of row oy or H - 1 - oy, columns forward or reversed, vector stores where aligned
      const uint32_t ng = ((uint32_t)nox + 3u) >> 2, total = ng * (uint32_t)nrows;
      for (uint32_t idx = (uint32_t)tid; idx < total; idx += 256u) {
        const uint32_t r = idx / ng, g = idx - r * ng;
        int R[4], G[4], B[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {                     // (past the tile's last pixel: inside the padded stage row, not stored)
          const typename St::S s = stage[r][g * 4u + (uint32_t)i];
          R[i] = St::get(s, 0); G[i] = St::get(s, 1); B[i] = St::get(s, 2);
        }
        const int oy = yb + (int)r;
        store_oriented4<DT>(op, tp.ow, tp.oh, fx, oxA + (int)g * 4, fy ? tp.oh - 1 - oy : oy, min(4, nox - (int)g * 4), R, G, B);
      }
      __syncthreads();                                    // the stage is written again by the next block of rows
      continue;
    }
    // rows yb .. yb + nrows - 1 of P are displayed columns Xrun .. Xrun + nrows - 1 (in reverse order where fx), column x of P is displayed row Y
    const uint32_t n = (uint32_t)nrows;
    const size_t pitch = (size_t)op.pitch, xrun = (size_t)(fx ? tp.oh - yb - nrows : yb);
    HIPDEC_GLOBAL E* o = (HIPDEC_GLOBAL E*)p.o0;
    if (tp.nhwc) {
      const uint32_t per = 3u * n, total = per * (uint32_t)nox;
      for (uint32_t idx = (uint32_t)tid; idx < total; idx += 256u) {
        const uint32_t c = idx / per, e = idx - c * per, j = e / 3u, k = e - 3u * j;
        const int x = oxA + (int)c;
        const size_t Yd = (size_t)(fy ? tp.ow - 1 - x : x);
        const int val = St::get(stage[fx ? n - 1u - j : j][c], k);
        o[Yd * pitch + xrun * 3 + e] = (E)tensor_elem<DT>(val, k == 0 ? tp.scale[0] : (k == 1 ? tp.scale[1] : tp.scale[2]), k == 0 ? tp.bias[0] : (k == 1 ? tp.bias[1] : tp.bias[2]));
      }
    } else {
      const uint32_t total = n * (uint32_t)nox;
      const size_t plane = (size_t)op.plane_rows * pitch;   // (the displayed picture's t.ow rows, or the canvas')
      for (uint32_t idx = (uint32_t)tid; idx < total; idx += 256u) {
        const uint32_t c = idx / n, j = idx - c * n;
        const int x = oxA + (int)c;
        const size_t Yd = (size_t)(fy ? tp.ow - 1 - x : x);
        const typename St::S s = stage[fx ? n - 1u - j : j][c];
        HIPDEC_GLOBAL E* d = o + Yd * pitch + xrun + j;
        d[0] = (E)tensor_elem<DT>(St::get(s, 0), tp.scale[0], tp.bias[0]);
        d[plane] = (E)tensor_elem<DT>(St::get(s, 1), tp.scale[1], tp.bias[1]);
        d[2 * plane] = (E)tensor_elem<DT>(St::get(s, 2), tp.scale[2], tp.bias[2]);
      }
    }
    __syncthreads();                                      // the stage is written again by the next block of rows
  }
}

// k_oriented_box with the blocked store: the box kernel of a patch sequence.  Its integer stage is k_oriented_box's, statement for statement; the two texts
// differ in the store only.  (k_oriented_box is not built from a body shared with this kernel, as k_oriented_nearest and k_resample are from theirs: as a
// wrapper of one it allocated 122 / 170 VGPRs where it has 119 / 166 - the difference is lanes that hold spilled SGPRs - and left the 168 step of the 16-bit
// kernel.)  The patch constants are read where the store needs them, behind the box stage, not held in SGPRs across it: the stage is where the kernel's
// register pressure peaks.
//   row-preserving codes:  4-pixel groups through store_patch4.
//   quarter turns:         column x of the tile is displayed row Y and receives a run of RB pixels, as in k_oriented_box; in token order the run is cut where
//                          it crosses a patch: consecutive lanes stay on consecutive elements inside each piece of P pixels (3 * P elements in NaFlex
//                          order), and the pieces of one run lie a token apart.  The patch of an element is found per element.
__device__ __forceinline__ PatchInfo patch_info_late(const PatchParams* q)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HIPDEC_HOST_EMU)
  asm volatile("" : "+s"(q));   // (the loads stay behind this point)
#endif
  return q->b;
}

// (the occupancy step is stated - four workgroups per CU for 8-bit samples, 128 VGPRs; three for 16-bit ones, 168 - so that the scheduler orders the store for
// registers: left to itself it took 130 - 132 / 180 for the float dtypes)
template <typename Pix, int DT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sizeof(Pix) == 1 ? 4 : 3))) void k_patch_box(const PatchParams* __restrict__ ps)
{
  typedef OrientedTile<Pix, DT> T;
  typedef OrientedStage<T::kNarrow> St;
  typedef typename TensorElem<DT>::T E;
  constexpr int RB = T::RB, TC = T::TC;
  __shared__ typename BoxAcc<Pix>::T colsum[3][kBoxSpan];
  __shared__ typename St::S stage[RB][TC + 1];
  const OrientedParams op = ps[blockIdx.z].in;   // wave-uniform: scalar loads into SGPRs
  const TensorParams& tp = op.t;
  const ColorParams& p = tp.c;
  const int tid = threadIdx.x;
  const int oxA = blockIdx.x * tp.tile;
  if (oxA >= tp.ow) return;                               // (the whole workgroup)
  const int nox = min(tp.tile, tp.ow - oxA);              // <= TC: the host caps the tile
  const bool mono = p.arith == AR_MONO;
  const int quarter = op.code & 1, fx = ((op.code >> 1) ^ (op.code >> 2)) & 1, fy = ((op.code >> 1) ^ op.code) & 1;
  const int cl = tp.left >> tp.sH, ct = tp.top >> tp.sV;
  const int cw = ((tp.left + tp.rw - 1) >> tp.sH) - cl + 1, ch = ((tp.top + tp.rh - 1) >> tp.sV) - ct + 1;
  const int fcw = (p.w + (1 << tp.sH) - 1) >> tp.sH;
  const BoxPlane pl[3] = {{p.y, p.ys, tp.rw, tp.rh, p.w, tp.left, tp.top}, {p.cb, p.cbs, cw, ch, fcw, cl, ct}, {p.cr, p.crs, cw, ch, fcw, cl, ct}};
  const int rb = max(1, min((int)op.rb, RB));                  // (the stage has RB rows whatever the block says)
  for (int yb = blockIdx.y * rb; yb < tp.oh; yb += gridDim.y * rb) {
    const int nrows = min(rb, tp.oh - yb);
    for (int r = 0; r < nrows; r++) {
      uint32_t v[3];
      box_tile<Pix, 3, true>(pl, mono ? 1 : 3, tp.ow, tp.oh, oxA, nox, yb + r, colsum, v);
      if (tid < nox) {                                    // the owner of column oxA + tid converts its own pixel (four copies of it: one statement of the arithmetic)
        const int Y[4] = {(int)v[0], (int)v[0], (int)v[0], (int)v[0]}, CB[4] = {(int)v[1], (int)v[1], (int)v[1], (int)v[1]}, CR[4] = {(int)v[2], (int)v[2], (int)v[2], (int)v[2]};
        int R[4], G[4], B[4];
        tensor_convert4<Pix>(p, Y, CB, CR, R, G, B);
        stage[r][tid] = St::pack(R[0], G[0], B[0]);
      }
      __syncthreads();                                    // colsum is written again by the next row; after the last one the stage is complete
    }
    const PatchInfo b = patch_info_late(ps + blockIdx.z);
    if (!quarter) {
      const uint32_t ng = ((uint32_t)nox + 3u) >> 2, total = ng * (uint32_t)nrows;
#pragma unroll 1
      for (uint32_t idx = (uint32_t)tid; idx < total; idx += 256u) {
        const uint32_t r = idx / ng, g = idx - r * ng;
        int R[4], G[4], B[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {                     // (past the tile's last pixel: inside the padded stage row, not stored)
          const typename St::S s = stage[r][g * 4u + (uint32_t)i];
          R[i] = St::get(s, 0); G[i] = St::get(s, 1); B[i] = St::get(s, 2);
        }
        const int oy = yb + (int)r;
        store_patch4<DT>(op, b, tp.ow, fx, oxA + (int)g * 4, fy ? tp.oh - 1 - oy : oy, min(4, nox - (int)g * 4), R, G, B);
      }
      __syncthreads();                                    // the stage is written again by the next block of rows
      continue;
    }
    // rows yb .. yb + nrows - 1 of P are displayed columns xrun .. xrun + nrows - 1 (in reverse order where fx), column x of P is displayed row Y
    const uint32_t n = (uint32_t)nrows, xrun = (uint32_t)(fx ? tp.oh - yb - nrows : yb);
    HIPDEC_GLOBAL E* o = (HIPDEC_GLOBAL E*)p.o0;
    if (tp.nhwc) {
      const uint32_t per = 3u * n, total = per * (uint32_t)nox;
#pragma unroll 1
      for (uint32_t idx = (uint32_t)tid; idx < total; idx += 256u) {
        const uint32_t c = idx / per, e = idx - c * per, j = e / 3u, k = e - 3u * j;
        const int x = oxA + (int)c;
        const int val = St::get(stage[fx ? n - 1u - j : j][c], k);
        o[patch_rowoff(b, (uint32_t)(fy ? tp.ow - 1 - x : x)) + patch_coloff(b, xrun + j) + k] =
            (E)tensor_elem<DT>(val, k == 0 ? tp.scale[0] : (k == 1 ? tp.scale[1] : tp.scale[2]), k == 0 ? tp.bias[0] : (k == 1 ? tp.bias[1] : tp.bias[2]));
      }
    } else {
      const uint32_t total = n * (uint32_t)nox;
#pragma unroll 1
      for (uint32_t idx = (uint32_t)tid; idx < total; idx += 256u) {
        const uint32_t c = idx / n, j = idx - c * n;
        const int x = oxA + (int)c;
        const typename St::S s = stage[fx ? n - 1u - j : j][c];
        HIPDEC_GLOBAL E* d = o + patch_rowoff(b, (uint32_t)(fy ? tp.ow - 1 - x : x)) + patch_coloff(b, xrun + j);
        d[0] = (E)tensor_elem<DT>(St::get(s, 0), tp.scale[0], tp.bias[0]);
        d[b.chs] = (E)tensor_elem<DT>(St::get(s, 1), tp.scale[1], tp.bias[1]);
        d[2 * b.chs] = (E)tensor_elem<DT>(St::get(s, 2), tp.scale[2], tp.bias[2]);
      }
    }
    __syncthreads();                                      // the stage is written again by the next block of rows
  }
}

// Nearest neighbour runs in OUTPUT space for all eight codes: a lane owns four pixels of a DISPLAYED row, maps each back to its pixel (x, y) of P and from
// there to the source sample k_tensor_nearest reads, and stores them with store_tensor4's shape.  The stores are as coalesced as the unoriented kernel's; the
// reads of a quarter turn walk down source columns, which a down-scaling nearest kernel - it reads one sample in (scale factor)^2 - does sparsely either way.
// No LDS.
template <typename Pix, int DT, typename Store>
__device__ __forceinline__ void oriented_nearest_body(const typename Store::Block* ps, const int tx, const int ty)   // tx, ty: threadIdx.x / .y, as in oriented_box_body
{
  const typename Store::Block blk = ps[blockIdx.z];
  const OrientedParams& op = Store::inner(blk);
  const Store st(blk);
  const TensorParams& tp = op.t;
  const ColorParams& p = tp.c;
  const int quarter = op.code & 1, fx = ((op.code >> 1) ^ (op.code >> 2)) & 1, fy = ((op.code >> 1) ^ op.code) & 1;
  const int dw = quarter ? tp.oh : tp.ow, dh = quarter ? tp.ow : tp.oh;   // the displayed size
  const int X0 = ((blockIdx.x + st.origin_x()) * blockDim.x + tx) * 4;
  if (X0 >= dw) return;
  const int npx = min(4, dw - X0);
  if (!st.shown_cols_d(X0, npx)) return;                  // (the framed store: a group outside the window reads nothing)
  const bool mono = p.arith == AR_MONO;
  const int ra = quarter ? tp.rh : tp.rw, rc = quarter ? tp.rw : tp.rh;   // the window's extent along a displayed row, and across the rows
  for (int Yd = (blockIdx.y + st.origin_y()) * blockDim.y + ty; Yd < dh; Yd += gridDim.y * blockDim.y) {
    if (!st.shown_row_d(Yd)) continue;
    const int c = fy ? dh - 1 - Yd : Yd;
    const int sc = (int)((uint64_t)c * (uint64_t)rc / (uint64_t)dh);
    int Y[4], CB[4], CR[4], R[4], G[4], B[4];
    if (!quarter) {   // rows stay rows: k_tensor_nearest's row pointers, one source row per lane
      const int iy = tp.top + sc;
      HIPDEC_GLOBAL const Pix* yrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.y + (size_t)iy * p.ys);
      HIPDEC_GLOBAL const Pix* cbrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.cb + (size_t)(iy >> tp.sV) * p.cbs);
      HIPDEC_GLOBAL const Pix* crrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.cr + (size_t)(iy >> tp.sV) * p.crs);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int X = min(X0 + i, dw - 1), a = fx ? dw - 1 - X : X;
        const int ix = tp.left + (int)((uint64_t)a * (uint64_t)ra / (uint64_t)dw);
        Y[i] = yrow[ix];
        CB[i] = mono ? 0 : cbrow[ix >> tp.sH];
        CR[i] = mono ? 0 : crrow[ix >> tp.sH];
      }
    } else {
      const int ix = tp.left + sc;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int X = min(X0 + i, dw - 1), a = fx ? dw - 1 - X : X;
        const int iy = tp.top + (int)((uint64_t)a * (uint64_t)ra / (uint64_t)dw);
        Y[i] = *(HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.y + (size_t)iy * p.ys + (size_t)ix * sizeof(Pix));
        CB[i] = mono ? 0 : *(HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.cb + (size_t)(iy >> tp.sV) * p.cbs + (size_t)(ix >> tp.sH) * sizeof(Pix));
        CR[i] = mono ? 0 : *(HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.cr + (size_t)(iy >> tp.sV) * p.crs + (size_t)(ix >> tp.sH) * sizeof(Pix));
      }
    }
    tensor_convert4<Pix>(p, Y, CB, CR, R, G, B);
    st.template group4<DT>(op, dw, dh, 0, X0, Yd, npx, R, G, B);
  }
}

template <typename Pix, int DT>
__global__ __launch_bounds__(256) void k_oriented_nearest(const OrientedParams* __restrict__ ps)
{
  oriented_nearest_body<Pix, DT, DenseStore<OrientedParams>>(ps, threadIdx.x, threadIdx.y);
}

template <typename Pix, int DT>
__global__ __launch_bounds__(256) void k_patch_nearest(const PatchParams* __restrict__ ps)
{
  oriented_nearest_body<Pix, DT, PatchStore<PatchParams>>(ps, threadIdx.x, threadIdx.y);
}

// ---- framed tensor output (include/heif_hipdec.h hipdec_batch_to_tensor_framed): the entry's rectangle may leave its canvas, and only the part of the
// sample on the canvas - the window, hipdec::FrameWindow - is computed and stored.  o0 is where the whole sample's first element would lie (in front of the
// canvas for a negative offset), pitch and plane are the canvas', as for a placed entry; k_canvas_margin writes everything outside the window.
// The kernels are siblings of the oriented ones with a clipping store, built as the k_patch_* kernels are: the nearest and resampling bodies take the store
// as a policy, the box kernel is a sibling text of k_oriented_box.  The window is wave-uniform and comes from the entry's block through scalar loads.
struct FrameParams { OrientedParams in; hipdec::FrameWindow b; };
static_assert(sizeof(hipdec::FrameWindow) == 48, "the blocks behind it stay 16-byte multiples");

// store_oriented4 inside the window: a group wholly outside it is neither converted nor stored, a whole group inside it is store_oriented4's (vector stores
// behind the run-time alignment test), a group the window's edge cuts goes out as element stores - for a quarter turn the resampler's groups run along a
// column of P, and reversed groups are cut from the other end: both are columns xs .. xs + npx - 1 of displayed row `row` here.
template <int DT>
__device__ __forceinline__ void store_frame4(const OrientedParams& op, const hipdec::FrameWindow& f, int dw_, int dh_, int rev, int x0, int row, int npx,
                                             const int (&R)[4], const int (&G)[4], const int (&B)[4])
{
  typedef typename TensorElem<DT>::T E;
  if (row < f.vy0 || row >= f.vy1) return;
  const int xs = rev ? dw_ - npx - x0 : x0;   // the group's first column in memory
  if (xs + npx <= f.vx0 || xs >= f.vx1) return;
  if (xs >= f.vx0 && xs + npx <= f.vx1) { store_oriented4<DT>(op, dw_, dh_, rev, x0, row, npx, R, G, B); return; }
  const TensorParams& tp = op.t;
  const size_t pitch = (size_t)op.pitch, plane = (size_t)op.plane_rows * pitch;
  HIPDEC_GLOBAL E* o = (HIPDEC_GLOBAL E*)tp.c.o0 + (size_t)row * pitch;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i >= npx) break;
    const int col = rev ? dw_ - 1 - (x0 + i) : x0 + i;
    if (col < f.vx0 || col >= f.vx1) continue;
    const uint32_t r = tensor_elem<DT>(R[i], tp.scale[0], tp.bias[0]), g = tensor_elem<DT>(G[i], tp.scale[1], tp.bias[1]), b = tensor_elem<DT>(B[i], tp.scale[2], tp.bias[2]);
    if (tp.nhwc) {
      HIPDEC_GLOBAL E* d = o + (size_t)col * 3;
      d[0] = (E)r; d[1] = (E)g; d[2] = (E)b;
    } else {
      HIPDEC_GLOBAL E* d = o + (size_t)col;
      d[0] = (E)r; d[plane] = (E)g; d[2 * plane] = (E)b;
    }
  }
}

template <typename Blk> struct FrameStore {   // Blk: FrameParams, or FrameResampleParams - {the dense block `in`, hipdec::FrameWindow b}
  typedef Blk Block;
  const hipdec::FrameWindow& f;
  __device__ __forceinline__ explicit FrameStore(const Blk& k) : f(k.b) {}
  static __device__ __forceinline__ auto inner(const Blk& k) -> decltype((k.in)) { return k.in; }
  __device__ __forceinline__ bool shown_cols_p(int x0, int n) const { return x0 + n > f.px0 && x0 < f.px1; }
  __device__ __forceinline__ bool shown_rows_p(int y0, int n) const { return y0 + n > f.py0 && y0 < f.py1; }
  __device__ __forceinline__ bool shown_cols_d(int x0, int n) const { return x0 + n > f.vx0 && x0 < f.vx1; }
  __device__ __forceinline__ bool shown_row_d(int y) const { return y >= f.vy0 && y < f.vy1; }
  __device__ __forceinline__ int origin_x() const { return f.tx0; }
  __device__ __forceinline__ int origin_y() const { return f.ty0; }
  template <int DT>
  __device__ __forceinline__ void group4(const OrientedParams& op, int dw, int dh, int rev, int x0, int row, int npx, const int (&R)[4], const int (&G)[4],
                                         const int (&B)[4]) const
  {
    store_frame4<DT>(op, f, dw, dh, rev, x0, row, npx, R, G, B);
  }
};

__device__ __forceinline__ hipdec::FrameWindow frame_window_late(const FrameParams* q)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HIPDEC_HOST_EMU)
  asm volatile("" : "+s"(q));   // (the loads stay behind this point, as patch_info_late's)
#endif
  return q->b;
}

// k_oriented_box with the clipping store.  Its integer stage is k_oriented_box's, statement for statement, over the rows and column tiles of P that hold a
// visible pixel: a workgroup whose column tile lies outside the window returns before it loads a sample, a block of rows outside it is passed over, and
// inside a block the rows of P outside the window are not accumulated (their stage rows are never read: the write-out below stores inside the window only).
//   row-preserving codes:  4-pixel groups through store_frame4.
//   quarter turns:         k_oriented_box's runs along displayed rows, element by element as there, each element behind the window test.
// The displayed window is read where the store needs it, behind the box stage (k_patch_box's reason), the window in P in front of it.
// (the occupancy step is stated as for k_patch_box and k_clip_box)
template <typename Pix, int DT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sizeof(Pix) == 1 ? 4 : 3))) void k_frame_box(const FrameParams* __restrict__ ps)
{
  typedef OrientedTile<Pix, DT> T;
  typedef OrientedStage<T::kNarrow> St;
  typedef typename TensorElem<DT>::T E;
  constexpr int RB = T::RB, TC = T::TC;
  __shared__ typename BoxAcc<Pix>::T colsum[3][kBoxSpan];
  __shared__ typename St::S stage[RB][TC + 1];
  const OrientedParams op = ps[blockIdx.z].in;   // wave-uniform: scalar loads into SGPRs
  const TensorParams& tp = op.t;
  const ColorParams& p = tp.c;
  const int tid = threadIdx.x;
  const int oxA = ((int)blockIdx.x + ps[blockIdx.z].b.tx0) * tp.tile;   // (the grid starts at the first column tile and block of rows with a visible pixel)
  if (oxA >= tp.ow) return;                               // (the whole workgroup)
  const int nox = min(tp.tile, tp.ow - oxA);              // <= TC: the host caps the tile
  const int px0 = ps[blockIdx.z].b.px0, px1 = ps[blockIdx.z].b.px1, py0 = ps[blockIdx.z].b.py0, py1 = ps[blockIdx.z].b.py1;
  if (oxA + nox <= px0 || oxA >= px1) return;             // no visible pixel in this column tile: nothing is loaded
  const bool mono = p.arith == AR_MONO;
  const int quarter = op.code & 1, fx = ((op.code >> 1) ^ (op.code >> 2)) & 1, fy = ((op.code >> 1) ^ op.code) & 1;
  const int cl = tp.left >> tp.sH, ct = tp.top >> tp.sV;
  const int cw = ((tp.left + tp.rw - 1) >> tp.sH) - cl + 1, ch = ((tp.top + tp.rh - 1) >> tp.sV) - ct + 1;
  const int fcw = (p.w + (1 << tp.sH) - 1) >> tp.sH;
  const BoxPlane pl[3] = {{p.y, p.ys, tp.rw, tp.rh, p.w, tp.left, tp.top}, {p.cb, p.cbs, cw, ch, fcw, cl, ct}, {p.cr, p.crs, cw, ch, fcw, cl, ct}};
  const int rb = max(1, min((int)op.rb, RB));                  // (the stage has RB rows whatever the block says)
  for (int yb = ((int)blockIdx.y + ps[blockIdx.z].b.ty0) * rb; yb < tp.oh; yb += gridDim.y * rb) {
    const int nrows = min(rb, tp.oh - yb);
    if (yb >= py1) break;                                 // no visible pixel from this block of rows on (uniform over the workgroup)
    if (yb + nrows <= py0) continue;
    for (int r = 0; r < nrows; r++) {
      if (yb + r < py0 || yb + r >= py1) continue;        // a row of P outside the window is not accumulated
      uint32_t v[3];
      box_tile<Pix, 3, true>(pl, mono ? 1 : 3, tp.ow, tp.oh, oxA, nox, yb + r, colsum, v);
      if (tid < nox) {                                    // the owner of column oxA + tid converts its own pixel (four copies of it: one statement of the arithmetic)
        const int Y[4] = {(int)v[0], (int)v[0], (int)v[0], (int)v[0]}, CB[4] = {(int)v[1], (int)v[1], (int)v[1], (int)v[1]}, CR[4] = {(int)v[2], (int)v[2], (int)v[2], (int)v[2]};
        int R[4], G[4], B[4];
        tensor_convert4<Pix>(p, Y, CB, CR, R, G, B);
        stage[r][tid] = St::pack(R[0], G[0], B[0]);
      }
      __syncthreads();                                    // colsum is written again by the next row; after the last one the stage is complete
    }
    const hipdec::FrameWindow f = frame_window_late(ps + blockIdx.z);
    if (!quarter) {
      const uint32_t ng = ((uint32_t)nox + 3u) >> 2, total = ng * (uint32_t)nrows;
#pragma unroll 1
      for (uint32_t idx = (uint32_t)tid; idx < total; idx += 256u) {
        const uint32_t r = idx / ng, g = idx - r * ng;
        int R[4], G[4], B[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {                     // (past the tile's last pixel: inside the padded stage row, not stored)
          const typename St::S s = stage[r][g * 4u + (uint32_t)i];
          R[i] = St::get(s, 0); G[i] = St::get(s, 1); B[i] = St::get(s, 2);
        }
        const int oy = yb + (int)r;
        store_frame4<DT>(op, f, tp.ow, tp.oh, fx, oxA + (int)g * 4, fy ? tp.oh - 1 - oy : oy, min(4, nox - (int)g * 4), R, G, B);
      }
      __syncthreads();                                    // the stage is written again by the next block of rows
      continue;
    }
    // rows yb .. yb + nrows - 1 of P are displayed columns xrun .. xrun + nrows - 1 (in reverse order where fx), column x of P is displayed row Y
    const uint32_t n = (uint32_t)nrows;
    const int xrun = fx ? tp.oh - yb - nrows : yb;
    const size_t pitch = (size_t)op.pitch;
    HIPDEC_GLOBAL E* o = (HIPDEC_GLOBAL E*)p.o0;
    if (tp.nhwc) {
      const uint32_t per = 3u * n, total = per * (uint32_t)nox;
#pragma unroll 1
      for (uint32_t idx = (uint32_t)tid; idx < total; idx += 256u) {
        const uint32_t c = idx / per, e = idx - c * per, j = e / 3u, k = e - 3u * j;
        const int x = oxA + (int)c;
        const int Yd = fy ? tp.ow - 1 - x : x, Xd = xrun + (int)j;
        if (Yd < f.vy0 || Yd >= f.vy1 || Xd < f.vx0 || Xd >= f.vx1) continue;
        const int val = St::get(stage[fx ? n - 1u - j : j][c], k);
        o[(size_t)Yd * pitch + (size_t)xrun * 3 + e] = (E)tensor_elem<DT>(val, k == 0 ? tp.scale[0] : (k == 1 ? tp.scale[1] : tp.scale[2]), k == 0 ? tp.bias[0] : (k == 1 ? tp.bias[1] : tp.bias[2]));
      }
    } else {
      const uint32_t total = n * (uint32_t)nox;
      const size_t plane = (size_t)op.plane_rows * pitch;   // (the canvas' rows)
#pragma unroll 1
      for (uint32_t idx = (uint32_t)tid; idx < total; idx += 256u) {
        const uint32_t c = idx / n, j = idx - c * n;
        const int x = oxA + (int)c;
        const int Yd = fy ? tp.ow - 1 - x : x, Xd = xrun + (int)j;
        if (Yd < f.vy0 || Yd >= f.vy1 || Xd < f.vx0 || Xd >= f.vx1) continue;
        const typename St::S s = stage[fx ? n - 1u - j : j][c];
        HIPDEC_GLOBAL E* d = o + (size_t)Yd * pitch + (size_t)Xd;
        d[0] = (E)tensor_elem<DT>(St::get(s, 0), tp.scale[0], tp.bias[0]);
        d[plane] = (E)tensor_elem<DT>(St::get(s, 1), tp.scale[1], tp.bias[1]);
        d[2 * plane] = (E)tensor_elem<DT>(St::get(s, 2), tp.scale[2], tp.bias[2]);
      }
    }
    __syncthreads();                                      // the stage is written again by the next block of rows
  }
}

template <typename Pix, int DT>
__global__ __launch_bounds__(256) void k_frame_nearest(const FrameParams* __restrict__ ps)
{
  oriented_nearest_body<Pix, DT, FrameStore<FrameParams>>(ps, threadIdx.x, threadIdx.y);
}

// ---- placed tensor output (include/heif_hipdec.h hipdec_batch_to_tensor_placed): the oriented / resampling kernels write an entry's sample into its
// rectangle of the canvas - o0 the rectangle's first element, pitch the canvas row, plane the canvas plane - and k_canvas_margin writes everything else:
// the fill element of each channel outside the rectangle and, where asked for, the whole mask (1 outside, 0 inside).  ONE launch for all entries of a call,
// blockIdx.z the entry.  Store-only, no LDS.
// Shape: an entry's canvas is one run of 3 * W * H elements, cut into the 16-byte blocks of MEMORY it touches (the first and last may be partial); a lane owns
// one block at a time, finds (channel, row, column) of its first element with two divisions (32-bit while the entry has fewer than 2^31 elements) and walks
// its 16 / 8 / 4 elements from there with compares only.  A block that is margin throughout - the rows above and below the rectangle, and, since the run
// right of the rectangle in one row continues as the run left of it in the next, most of what lies beside it - goes out as ONE 16-byte store; a block the
// rectangle's edge or the entry's end cuts goes out element by element, margin elements only; a block inside the rectangle is not touched.  Consecutive lanes
// own consecutive blocks, so a wave's vector stores cover 1 KiB of consecutive memory.
// Bytes: the margin's elements once (plus W * H mask bytes), nothing read but the parameter block.
template <int DT>
__device__ __forceinline__ uint32_t canvas_fill_elem(const hipdec::CanvasMargin& m, float value, float scale, float bias)
{
  if (m.domain == HIPDEC_FILL_COMPONENT) return tensor_elem<DT>((int)value, scale, bias);   // what a pixel of that component value gets
  if (DT == TD_U8) return (uint32_t)(int)value;
  if (DT == TD_F32) return __builtin_bit_cast(uint32_t, value);
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HIPDEC_HOST_EMU)
  if (DT == TD_F16) return __builtin_bit_cast(uint16_t, (_Float16)value);
  return __builtin_bit_cast(uint16_t, (__bf16)value);
#else
  return DT == TD_F16 ? f32_to_f16_rne(__builtin_bit_cast(uint32_t, value)) : f32_to_bf16_rne(__builtin_bit_cast(uint32_t, value));
#endif
}

// MASK: `base` is the entry's W * H mask bytes - one plane, 1 outside the rectangle and 0 inside, every byte written
template <typename E, bool MASK, typename Idx>
__device__ __forceinline__ void canvas_margin_blocks(const hipdec::CanvasMargin& m, HIPDEC_GLOBAL E* base, uint32_t f0, uint32_t f1, uint32_t f2)
{
  constexpr int N = 16 / (int)sizeof(E), PER = 4 / (int)sizeof(E);
  constexpr uint32_t kAll = N == 16 ? 0xffffu : (N == 8 ? 0xffu : 0xfu);
  const bool nhwc = !MASK && m.nhwc;
  const int W = m.W, H = m.H, x0 = m.x, x1 = m.x + m.w, y0 = m.y, y1 = m.y + m.h;
  const Idx px = (Idx)W * (Idx)H, total = MASK ? px : px * 3;
  const uintptr_t addr = (uintptr_t)base;
  const bool aligned = (addr & (sizeof(E) - 1)) == 0;                 // (an output that is not even element-aligned takes element stores throughout)
  const uint32_t lead = (uint32_t)((addr & 15) / sizeof(E));          // elements between the 16-byte boundary below the entry and its first element
  HIPDEC_GLOBAL E* origin = base - lead;
  const Idx nblocks = (total + lead + (Idx)(N - 1)) / (Idx)N;
  for (Idx j = (Idx)blockIdx.x * 256u + threadIdx.x; j < nblocks; j += (Idx)gridDim.x * 256u) {
    const Idx v0 = j * (Idx)N;
    const uint32_t skip = v0 < (Idx)lead ? lead - (uint32_t)v0 : 0u;  // (block 0 only: its elements in front of the entry)
    Idx e = v0 + skip - lead;
    int c, y, x;
    if (nhwc) {
      const Idx pix = e / 3u, row = pix / (Idx)W;
      c = (int)(e - pix * 3u); y = (int)row; x = (int)(pix - row * (Idx)W);
    } else {
      const Idx pl = e / px, r = e - pl * px, row = r / (Idx)W;
      c = (int)pl; y = (int)row; x = (int)(r - row * (Idx)W);
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u}, bits = 0u;
#pragma unroll
    for (int i = 0; i < N; i++) {
      if ((uint32_t)i >= skip && e < total) {
        const bool in = y >= y0 && y < y1 && x >= x0 && x < x1;
        const uint32_t el = MASK ? (in ? 0u : 1u) : (c == 0 ? f0 : (c == 1 ? f1 : f2));
        w[i / PER] |= el << (8u * (uint32_t)sizeof(E) * (uint32_t)(i % PER));
        if (MASK || !in) bits |= 1u << i;
        e++;
        if (nhwc) {
          if (++c == 3) { c = 0; if (++x == W) { x = 0; y++; } }
        } else if (++x == W) {
          x = 0;
          if (++y == H) { y = 0; c++; }
        }
      }
    }
    HIPDEC_GLOBAL E* d = origin + v0;
    if (bits == kAll && aligned) {
      uint4 v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
      *(HIPDEC_GLOBAL uint4*)d = v;
    } else if (bits) {
#pragma unroll
      for (int i = 0; i < N; i++)
        if ((bits >> i) & 1u) d[i] = (E)(w[i / PER] >> (8u * (uint32_t)sizeof(E) * (uint32_t)(i % PER)));
    }
  }
}

template <int DT>
__global__ __launch_bounds__(256) void k_canvas_margin(const hipdec::CanvasMargin* __restrict__ ms)
{
  typedef typename TensorElem<DT>::T E;
  const hipdec::CanvasMargin m = ms[blockIdx.z];   // wave-uniform: scalar loads into SGPRs
  const bool small = (uint64_t)m.W * (uint64_t)m.H * 3ull < (1ull << 31);
  if (m.margin) {
    const uint32_t f0 = canvas_fill_elem<DT>(m, m.value[0], m.scale[0], m.bias[0]), f1 = canvas_fill_elem<DT>(m, m.value[1], m.scale[1], m.bias[1]),
                   f2 = canvas_fill_elem<DT>(m, m.value[2], m.scale[2], m.bias[2]);
    if (small) canvas_margin_blocks<E, false, uint32_t>(m, (HIPDEC_GLOBAL E*)m.o0, f0, f1, f2);
    else canvas_margin_blocks<E, false, uint64_t>(m, (HIPDEC_GLOBAL E*)m.o0, f0, f1, f2);
  }
  if (m.mask) {
    if (small) canvas_margin_blocks<uint8_t, true, uint32_t>(m, (HIPDEC_GLOBAL uint8_t*)m.mask, 0u, 0u, 0u);
    else canvas_margin_blocks<uint8_t, true, uint64_t>(m, (HIPDEC_GLOBAL uint8_t*)m.mask, 0u, 0u, 0u);
  }
}

// ---- composed tensor output (include/heif_hipdec.h hipdec_batch_to_tensor_composed): several entries share a canvas - the k_frame_* kernels write each
// entry's pieces, and k_compose_cover writes everything NO entry's region covers: the fill element of each channel and, where asked for, the whole mask (1
// uncovered, 0 covered).  ONE launch for all canvases of a call, blockIdx.z the canvas.  k_canvas_margin's shape - a canvas is one run of 3 * W * H elements
// cut into the 16-byte blocks of memory it touches, a lane owns one block at a time, consecutive lanes own consecutive blocks, the canvas' block is
// wave-uniform - with a cover table (hipdec::CanvasCover) in place of the one rectangle: a lane finds (channel, row, column) of its first element with two
// divisions, the band of its row by binary search over the canvas' edges and, in the band, the first interval that ends right of its column; from there it
// walks its 16 / 8 / 4 elements with compares only - the interval cursor moves on when the column reaches the interval's end, the band is looked up again
// when a row ends (bands are contiguous: the next one).  A block that is fill throughout goes out as ONE 16-byte store, a block an interval's edge or the
// tensor's end cuts element by element, fill elements only, a covered block is not touched.  The table is read from global memory - a few words per lane,
// most of them the same for the lanes of a wave; store-only otherwise, no LDS.
template <typename E, bool MASK, typename Idx>
__device__ __forceinline__ void compose_cover_blocks(const hipdec::CanvasCover& cv, HIPDEC_GLOBAL E* base, uint32_t f0, uint32_t f1, uint32_t f2)
{
  constexpr int N = 16 / (int)sizeof(E), PER = 4 / (int)sizeof(E);
  constexpr uint32_t kAll = N == 16 ? 0xffffu : (N == 8 ? 0xffu : 0xfu);
  constexpr int kNone = 0x7fffffff;                                   // the cursor behind a band's last interval: no column reaches it
  const bool nhwc = !MASK && cv.m.nhwc;
  const int W = cv.m.W, H = cv.m.H, nb = cv.n_bands;
  const HIPDEC_GLOBAL int32_t* edge = (const HIPDEC_GLOBAL int32_t*)(uintptr_t)cv.table;
  const HIPDEC_GLOBAL int32_t* first = edge + nb + 1;
  const HIPDEC_GLOBAL int32_t* iv = first + nb + 1;
  const Idx px = (Idx)W * (Idx)H, total = MASK ? px : px * 3;
  const uintptr_t addr = (uintptr_t)base;
  const bool aligned = (addr & (sizeof(E) - 1)) == 0;                 // (an output that is not even element-aligned takes element stores throughout)
  const uint32_t lead = (uint32_t)((addr & 15) / sizeof(E));          // elements between the 16-byte boundary below the canvas and its first element
  HIPDEC_GLOBAL E* origin = base - lead;
  const Idx nblocks = (total + lead + (Idx)(N - 1)) / (Idx)N;
  for (Idx j = (Idx)blockIdx.x * 256u + threadIdx.x; j < nblocks; j += (Idx)gridDim.x * 256u) {
    const Idx v0 = j * (Idx)N;
    const uint32_t skip = v0 < (Idx)lead ? lead - (uint32_t)v0 : 0u;  // (block 0 only: its elements in front of the canvas)
    Idx e = v0 + skip - lead;
    int c, y, x;
    if (nhwc) {
      const Idx pix = e / 3u, row = pix / (Idx)W;
      c = (int)(e - pix * 3u); y = (int)row; x = (int)(pix - row * (Idx)W);
    } else {
      const Idx pl = e / px, r = e - pl * px, row = r / (Idx)W;
      c = (int)pl; y = (int)row; x = (int)(r - row * (Idx)W);
    }
    int b = 0;                                                        // the band of y: the last one whose first row is not below it
    for (int hi = nb - 1; b < hi;) {
      const int mid = (b + hi + 1) >> 1;
      if (edge[mid] <= y) b = mid; else hi = mid - 1;
    }
    int next = edge[b + 1], k = first[b], kend = first[b + 1];
    for (int hi = kend; k < hi;) {                                    // the first interval that ends right of x
      const int mid = (k + hi) >> 1;
      if (iv[2 * mid + 1] <= x) k = mid + 1; else hi = mid;
    }
    int cx0 = k < kend ? iv[2 * k] : kNone, cx1 = k < kend ? iv[2 * k + 1] : kNone;   // x < cx1 holds from here on
    uint32_t w[4] = {0u, 0u, 0u, 0u}, bits = 0u;
#pragma unroll
    for (int i = 0; i < N; i++) {
      if ((uint32_t)i >= skip && e < total) {
        const bool in = x >= cx0;
        const uint32_t el = MASK ? (in ? 0u : 1u) : (c == 0 ? f0 : (c == 1 ? f1 : f2));
        w[i / PER] |= el << (8u * (uint32_t)sizeof(E) * (uint32_t)(i % PER));
        if (MASK || !in) bits |= 1u << i;
        e++;
        bool step = true;
        if (nhwc) { step = ++c == 3; if (step) c = 0; }
        if (step) {
          if (++x == W) {
            x = 0;
            if (++y == H) { y = 0; c++; b = 0; next = edge[1]; }      // the next plane (NHWC and the mask: the canvas' end, nothing follows)
            else if (y == next) { b++; next = edge[b + 1]; }
            k = first[b]; kend = first[b + 1];
            cx0 = k < kend ? iv[2 * k] : kNone; cx1 = k < kend ? iv[2 * k + 1] : kNone;
          } else if (x == cx1) {                                      // (merged intervals: the next one starts right of x)
            k++;
            cx0 = k < kend ? iv[2 * k] : kNone; cx1 = k < kend ? iv[2 * k + 1] : kNone;
          }
        }
      }
    }
    HIPDEC_GLOBAL E* d = origin + v0;
    if (bits == kAll && aligned) {
      uint4 v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
      *(HIPDEC_GLOBAL uint4*)d = v;
    } else if (bits) {
#pragma unroll
      for (int i = 0; i < N; i++)
        if ((bits >> i) & 1u) d[i] = (E)(w[i / PER] >> (8u * (uint32_t)sizeof(E) * (uint32_t)(i % PER)));
    }
  }
}

template <int DT>
__global__ __launch_bounds__(256) void k_compose_cover(const hipdec::CanvasCover* __restrict__ cs)
{
  typedef typename TensorElem<DT>::T E;
  const hipdec::CanvasCover cv = cs[blockIdx.z];   // wave-uniform: scalar loads into SGPRs
  const bool small = (uint64_t)cv.m.W * (uint64_t)cv.m.H * 3ull < (1ull << 31);
  if (cv.m.margin) {
    const uint32_t f0 = canvas_fill_elem<DT>(cv.m, cv.m.value[0], cv.m.scale[0], cv.m.bias[0]),
                   f1 = canvas_fill_elem<DT>(cv.m, cv.m.value[1], cv.m.scale[1], cv.m.bias[1]),
                   f2 = canvas_fill_elem<DT>(cv.m, cv.m.value[2], cv.m.scale[2], cv.m.bias[2]);
    if (small) compose_cover_blocks<E, false, uint32_t>(cv, (HIPDEC_GLOBAL E*)cv.m.o0, f0, f1, f2);
    else compose_cover_blocks<E, false, uint64_t>(cv, (HIPDEC_GLOBAL E*)cv.m.o0, f0, f1, f2);
  }
  if (cv.m.mask) {
    if (small) compose_cover_blocks<uint8_t, true, uint32_t>(cv, (HIPDEC_GLOBAL uint8_t*)cv.m.mask, 0u, 0u, 0u);
    else compose_cover_blocks<uint8_t, true, uint64_t>(cv, (HIPDEC_GLOBAL uint8_t*)cv.m.mask, 0u, 0u, 0u);
  }
}

// ---- warped tensor output (include/heif_hipdec.h hipdec_tensor_warp): k_warp_nearest / _bilinear / _bicubic
#include "warp_kernels.h"
// ---- projective tensor output (include/heif_hipdec.h hipdec_tensor_project): k_project_nearest / _bilinear / _bicubic
#include "project_kernels.h"

// ---- photometric tensor output (include/heif_hipdec.h hipdec_tensor_photo): k_photo_hist, k_photo_apply
#include "photo_kernels.h"
// ---- augment stage (include/heif_hipdec.h hipdec_tensor_augment): k_augment_hue, k_augment_blur beside the photo stage's kernels
#include "augment_kernels.h"
// ---- recipe stage (include/heif_hipdec.h hipdec_tensor_recipe): k_recipe_affine_nearest / _bilinear / _bicubic, an affine step inside a chain
#include "recipe_kernels.h"

// the plane scalers: blockIdx.z selects the plane (all planes of an image, or of all items of a batch, are ONE launch)
// ---- Pillow's bilinear / bicubic resampling of 8-bit pictures (HIPDEC_SCALE_BILINEAR / _BICUBIC, include/heif_hipdec.h), bit for bit: two separable passes
// with integer coefficients of 22 fractional bits, the horizontal result rounded and clipped to 8 bits before the vertical pass.  The coefficient tables come
// from the host (resample_table_fill below): n_out records (first tap, tap count), then n_out rows of `stride` coefficients.
// A workgroup of 256 threads owns kResTR output rows x at most kResTC output columns of the PRE-orientation picture P of one entry.  It walks the source rows
// its vertical taps cover, kResSR at a time:
//   stage   the source columns the run's horizontal taps cover - at most kResSpan per chunk, from a 4-sample boundary of the plane - are read as the full-size
//           kernel reads them (one aligned load of four luma samples, nearest-neighbour chroma) and converted with convert4<Pix, LO_RGB24>, the statement
//           hipdec_batch_to_rgb's picture is made of; one packed 32-bit word per pixel goes to LDS.  Every source pixel is converted once per band.
//   H       thread (column c, source row j) adds its taps that lie inside the chunk (int32, carried across chunks: a row of 4096 samples to 1 is legal),
//           rounds, clips and leaves the 8-bit triple in LDS.
//   V       thread (column c, row group g) feeds that triple into the sums of its four output rows; the row group is the wave, so the vertical records and
//           coefficients are wave-uniform.  The sums stay in registers across all source rows of the band: no bound on the number of taps on either axis.
// The finished band goes through LDS to store_oriented4 in 4-pixel groups along DISPLAYED rows (for a quarter turn: four rows of P at one column), so flip,
// layout, dtype, pitch and orientation are the oriented kernels' store path; the unoriented calls use code 0 (4 with a flip) and a dense pitch.
// LDS: 4 * 1024 * 4 + 4 * 64 * 4 + 16 * 65 * 4 = 21568 bytes - seven workgroups per CU.  Both tap loops are runtime loops.
constexpr int kResTC = 64, kResTR = 16, kResSR = 4, kResSpan = 1024;
constexpr uint64_t kResampleTableBytes = 64ull << 20;   // bound on the tables of one call (include/heif_hipdec.h): HIPDEC_ERR_LIMIT above it

struct ResampleParams {
  OrientedParams o;         // o.t.ow x o.t.oh: the size of P; o.t.tile: output columns per workgroup (<= kResTC); o.t.flip is 0
  const int32_t* xt;        // the table of the horizontal axis (o.t.rw -> o.t.ow) and its coefficient row stride
  const int32_t* yt;        // ... of the vertical axis (o.t.rh -> o.t.oh)
  int xstride, ystride;
};

// four pixels of plane row yy from plane column x0 (a multiple of 4, inside the picture), as rgb_block loads them
template <typename Pix>
__device__ __forceinline__ void resample_load4(const ColorParams& p, int sH, int sV, bool mono, int x0, int yy, int (&Y)[4], int (&CB)[4], int (&CR)[4])
{
  const int npx = min(4, p.w - x0);
  HIPDEC_GLOBAL const Pix* yrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.y + (size_t)yy * p.ys) + x0;
  if (npx == 4 && sizeof(Pix) == 1 && (((uintptr_t)yrow) & 3) == 0) {
    const uint32_t v = *(HIPDEC_GLOBAL const uint32_t*)yrow;
    Y[0] = v & 255; Y[1] = (v >> 8) & 255; Y[2] = (v >> 16) & 255; Y[3] = v >> 24;
  } else if (npx == 4 && sizeof(Pix) == 2 && (((uintptr_t)yrow) & 7) == 0) {
    const uint2 v = *(HIPDEC_GLOBAL const uint2*)yrow;
    Y[0] = v.x & 0xffff; Y[1] = v.x >> 16; Y[2] = v.y & 0xffff; Y[3] = v.y >> 16;
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) Y[i] = i < npx ? yrow[i] : 0;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) { CB[i] = 0; CR[i] = 0; }
  if (mono) return;
  HIPDEC_GLOBAL const Pix* cbrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.cb + (size_t)(yy >> sV) * p.cbs);
  HIPDEC_GLOBAL const Pix* crrow = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.cr + (size_t)(yy >> sV) * p.crs);
  if (sH) {
    const int c0 = x0 >> 1;
    const int cbA = cbrow[c0], crA = crrow[c0];
    int cbB = cbA, crB = crA;
    if (npx > 2) { cbB = cbrow[c0 + 1]; crB = crrow[c0 + 1]; }
    CB[0] = CB[1] = cbA; CB[2] = CB[3] = cbB;
    CR[0] = CR[1] = crA; CR[2] = CR[3] = crB;
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) if (i < npx) { CB[i] = cbrow[x0 + i]; CR[i] = crrow[x0 + i]; }
  }
}

__device__ __forceinline__ uint32_t resample_pack(const int (&s)[3])
{
  return (uint32_t)clip_i(s[0] >> 22, 255) | ((uint32_t)clip_i(s[1] >> 22, 255) << 8) | ((uint32_t)clip_i(s[2] >> 22, 255) << 16);
}

template <typename Pix, int DT, typename Store>
__device__ __forceinline__ void resample_body(const typename Store::Block* ps, const int tid)   // tid: threadIdx.x, as in oriented_box_body
{
  __shared__ uint32_t src[kResSR][kResSpan];
  __shared__ uint32_t hrow[kResSR][kResTC];
  __shared__ uint32_t otile[kResTR][kResTC + 1];
  const typename Store::Block blk = ps[blockIdx.z];   // wave-uniform: scalar loads into SGPRs
  const ResampleParams& rp = Store::inner(blk);
  const Store st(blk);
  const OrientedParams& op = rp.o;
  const TensorParams& tp = op.t;
  const ColorParams& p = tp.c;
  const int c = tid & (kResTC - 1), rg = tid / kResTC;   // rg: the wave - source row of the chunk in H, row group of the band in V   // rg: the wave - source row of the chunk in H, row group of the band in V
  const int tile = max(1, min(tp.tile, kResTC));
  const int ox0 = (blockIdx.x + st.origin_x()) * tile;
  if (ox0 >= tp.ow) return;                               // (the whole workgroup)
  const int ncol = min(tile, tp.ow - ox0);
  if (!st.shown_cols_p(ox0, ncol)) return;                // (the framed store: a column tile outside the window - the whole workgroup, before any load)
  const bool mono = p.arith == AR_MONO;
  const int quarter = op.code & 1, fx = ((op.code >> 1) ^ (op.code >> 2)) & 1, fy = ((op.code >> 1) ^ op.code) & 1;
  HIPDEC_GLOBAL const int32_t* xt = (HIPDEC_GLOBAL const int32_t*)rp.xt;
  HIPDEC_GLOBAL const int32_t* yt = (HIPDEC_GLOBAL const int32_t*)rp.yt;
  HIPDEC_GLOBAL const int32_t* xk = xt + 2 * (size_t)tp.ow;
  HIPDEC_GLOBAL const int32_t* yk = yt + 2 * (size_t)tp.oh;
  // plane columns [base, send) hold every tap of the run (first taps and ends do not decrease along an axis); base is a 4-sample boundary of the plane
  const int base = (tp.left + xt[2 * ox0]) & ~3;
  const int send = tp.left + xt[2 * (ox0 + ncol - 1)] + xt[2 * (ox0 + ncol - 1) + 1];
  const int nchunks = (send - base + kResSpan - 1) / kResSpan;
  const bool hascol = c < ncol;
  const int cx = ox0 + (hascol ? c : 0);
  const int xa = tp.left + xt[2 * cx], xn = hascol ? xt[2 * cx + 1] : 0;   // this thread's column: its first tap as a plane column, and its tap count
  HIPDEC_GLOBAL const int32_t* kx = xk + (size_t)cx * (size_t)rp.xstride;
  for (int oy0 = (blockIdx.y + st.origin_y()) * kResTR; oy0 < tp.oh; oy0 += gridDim.y * kResTR) {
    const int nrow = min(kResTR, tp.oh - oy0);
    if (!st.shown_rows_p(oy0, nrow)) continue;            // (the framed store: a band outside the window is not staged; uniform over the workgroup)
    const int srow0 = yt[2 * oy0], srow1 = yt[2 * (oy0 + nrow - 1)] + yt[2 * (oy0 + nrow - 1) + 1];   // window rows [srow0, srow1) hold every tap of the band
    int ymin[4], yn[4], acc[4][3];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int r = rg * 4 + i;
      ymin[i] = r < nrow ? wave_uniform(yt[2 * (oy0 + r)]) : 0;
      yn[i] = r < nrow ? wave_uniform(yt[2 * (oy0 + r) + 1]) : 0;
      acc[i][0] = acc[i][1] = acc[i][2] = 1 << 21;
    }
    for (int sr = srow0; sr < srow1; sr += kResSR) {
      int h[3] = {1 << 21, 1 << 21, 1 << 21};
      for (int k = 0; k < nchunks; k++) {
        const int cs = base + k * kResSpan;
        if (k) __syncthreads();                           // H has finished with the previous chunk
        const int x0 = cs + tid * 4;
        if (x0 < send) {
#pragma unroll
          for (int j = 0; j < kResSR; j++) {
            if (sr + j >= srow1) break;
            int Y[4], CB[4], CR[4], R[4], G[4], B[4];
            resample_load4<Pix>(p, tp.sH, tp.sV, mono, x0, tp.top + sr + j, Y, CB, CR);
            convert4<Pix, LO_RGB24>(p, Y, CB, CR, R, G, B);
#pragma unroll
            for (int i = 0; i < 4; i++) src[j][tid * 4 + i] = (uint32_t)R[i] | ((uint32_t)G[i] << 8) | ((uint32_t)B[i] << 16);
          }
        }
        __syncthreads();
        if (sr + rg < srow1) {
          const int lo = max(xa, cs), hi = min(xa + xn, cs + kResSpan);
          for (int x = lo; x < hi; x++) {
            const uint32_t v = src[rg][x - cs];
            const int kk = kx[x - xa];
            h[0] += (int)(v & 255u) * kk; h[1] += (int)((v >> 8) & 255u) * kk; h[2] += (int)((v >> 16) & 255u) * kk;
          }
        }
      }
      hrow[rg][c] = resample_pack(h);                     // rounded and clipped to 8 bits BEFORE the vertical pass
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kResSR; j++) {
        const int sy = sr + j;
        if (sy >= srow1) break;
        const uint32_t v = hrow[j][c];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int t = sy - ymin[i];
          if ((unsigned)t < (unsigned)yn[i]) {
            const int kk = yk[(size_t)(oy0 + rg * 4 + i) * (size_t)rp.ystride + (size_t)t];
            acc[i][0] += (int)(v & 255u) * kk; acc[i][1] += (int)((v >> 8) & 255u) * kk; acc[i][2] += (int)((v >> 16) & 255u) * kk;
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) otile[rg * 4 + i][c] = resample_pack(acc[i]);
    __syncthreads();
    if (!quarter) {   // 4-pixel groups of row oy or H - 1 - oy, columns forward or reversed
      const uint32_t ng = ((uint32_t)ncol + 3u) >> 2, total = ng * (uint32_t)nrow;
      for (uint32_t idx = (uint32_t)tid; idx < total; idx += 256u) {
        const uint32_t r = idx / ng, g = idx - r * ng;
        int R[4], G[4], B[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {                     // (past the run's last pixel: inside the tile row, not stored)
          const uint32_t s = otile[r][g * 4u + (uint32_t)i];
          R[i] = (int)(s & 255u); G[i] = (int)((s >> 8) & 255u); B[i] = (int)((s >> 16) & 255u);
        }
        const int oy = oy0 + (int)r;
        st.template group4<DT>(op, tp.ow, tp.oh, fx, ox0 + (int)g * 4, fy ? tp.oh - 1 - oy : oy, min(4, ncol - (int)g * 4), R, G, B);
      }
    } else {          // a row of P is a displayed column: four rows of P at column x are four neighbours of displayed row Y
      const uint32_t ng = ((uint32_t)nrow + 3u) >> 2, total = ng * (uint32_t)ncol;
      for (uint32_t idx = (uint32_t)tid; idx < total; idx += 256u) {
        const uint32_t cc = idx / ng, g = idx - cc * ng;
        int R[4], G[4], B[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {                     // (past the band's last row: inside the tile, not stored)
          const uint32_t s = otile[g * 4u + (uint32_t)i][cc];
          R[i] = (int)(s & 255u); G[i] = (int)((s >> 8) & 255u); B[i] = (int)((s >> 16) & 255u);
        }
        const int x = ox0 + (int)cc;
        st.template group4<DT>(op, tp.oh, tp.ow, fx, oy0 + (int)g * 4, fy ? tp.ow - 1 - x : x, min(4, nrow - (int)g * 4), R, G, B);
      }
    }
    __syncthreads();                                      // the tile is written again by the next band
  }
}

template <typename Pix, int DT>
__global__ __launch_bounds__(256) void k_resample(const ResampleParams* __restrict__ ps)
{
  resample_body<Pix, DT, DenseStore<ResampleParams>>(ps, threadIdx.x);
}

// the resampler of a patch sequence: its quarter-turn write-out already goes in 4-pixel groups along displayed rows (bands of kResTR = 16 rows of P start at
// multiples of 16), so the blocked group store serves both write-outs
struct PatchResampleParams { ResampleParams in; PatchInfo b; };
template <typename Pix, int DT>
__global__ __launch_bounds__(256) void k_patch_resample(const PatchResampleParams* __restrict__ ps)
{
  resample_body<Pix, DT, PatchStore<PatchResampleParams>>(ps, threadIdx.x);
}

// the resampler of a framed entry: column tiles and bands of P with no visible pixel are not staged (the body asks the store), the write-out's groups go
// through store_frame4
struct FrameResampleParams { ResampleParams in; hipdec::FrameWindow b; };
template <typename Pix, int DT>
__global__ __launch_bounds__(256) void k_frame_resample(const FrameResampleParams* __restrict__ ps)
{
  resample_body<Pix, DT, FrameStore<FrameResampleParams>>(ps, threadIdx.x);
}

template <typename Pix>
__global__ __launch_bounds__(256) void k_scale_plane_nearest(const hipdec::PlaneScaleParams* __restrict__ ps)
{
  const hipdec::PlaneScaleParams p = ps[blockIdx.z];
  const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (x0 >= p.qw) return;
  for (int y = blockIdx.y * blockDim.y + threadIdx.y; y < p.qh; y += gridDim.y * blockDim.y) {
    // pixelimage.cc:1936-1943: the IMAGE's sizes, also for the chroma planes (the index stays inside the plane: x < (ow + 1) / 2 gives ix < (W + 1) / 2)
    const int iy = min((int)((uint64_t)y * (uint64_t)p.ih / (uint64_t)p.oh), p.ph - 1);
    HIPDEC_GLOBAL const Pix* src = (HIPDEC_GLOBAL const Pix*)((HIPDEC_GLOBAL const uint8_t*)p.in + (size_t)iy * p.is);
    HIPDEC_GLOBAL Pix* dst = (HIPDEC_GLOBAL Pix*)((HIPDEC_GLOBAL uint8_t*)p.out + (size_t)y * p.os);
    for (int i = 0; i < 4 && x0 + i < p.qw; i++) dst[x0 + i] = src[min((int)((uint64_t)(x0 + i) * (uint64_t)p.iw / (uint64_t)p.ow), p.pw - 1)];
  }
}

template <typename Pix>
__global__ __launch_bounds__(256) void k_scale_plane_box(const hipdec::PlaneScaleParams* __restrict__ ps)
{
  __shared__ typename BoxAcc<Pix>::T colsum[1][kBoxSpan];
  const hipdec::PlaneScaleParams p = ps[blockIdx.z];
  const int oxA = blockIdx.x * p.tile;
  if (oxA >= p.qw) return;
  const int nox = min(p.tile, p.qw - oxA);
  const BoxPlane pl[1] = {{p.in, p.is, p.pw, p.ph, p.pw, 0, 0}};
  for (int oy = blockIdx.y; oy < p.qh; oy += gridDim.y) {
    uint32_t v[1];
    box_tile<Pix, 1>(pl, 1, p.qw, p.qh, oxA, nox, oy, colsum, v);
    if ((int)threadIdx.x < nox) ((HIPDEC_GLOBAL Pix*)((HIPDEC_GLOBAL uint8_t*)p.out + (size_t)oy * p.os))[oxA + threadIdx.x] = (Pix)v[0];
    __syncthreads();                                      // colsum is written again by the next row
  }
}

// a13: one thread per 4 output samples of one row
template <typename Pix>
__device__ __forceinline__ int bilinear_at(const Pix* in, size_t is /*samples*/, int w, int h, int x, int y)
{
  // chroma_sampling.cc:611-708, expressed per output sample.  `is` is the input stride in samples.
  if (x == 0 && y == 0) return in[0];
  if (y == 0) {  // top border (note the reference's cx / 2 indexing, :620-626)
    if ((x & 1) && (x - 1) / 2 < (w - 1) / 2) { int cx = (x - 1) / 2; return (3 * in[cx / 2] + 1 * in[cx / 2 + 1] + 2) / 4; }
    if (!(x & 1) && (x - 2) / 2 < (w - 1) / 2) { int cx = (x - 2) / 2; return (1 * in[cx / 2] + 3 * in[cx / 2 + 1] + 2) / 4; }
    if (w % 2 == 0 && x == w - 1) return in[w / 2 - 1];
    return 0;
  }
  if (x == 0) {  // left border :635-640
    if ((y & 1) && (y - 1) / 2 < (h - 1) / 2) { int cy = (y - 1) / 2; return (3 * in[(cy / 2) * is] + 1 * in[(cy / 2 + 1) * is] + 2) / 4; }
    if (!(y & 1) && (y - 2) / 2 < (h - 1) / 2) { int cy = (y - 2) / 2; return (1 * in[(cy / 2) * is] + 3 * in[(cy / 2 + 1) * is] + 2) / 4; }
    if (h % 2 == 0 && y == h - 1) return in[(h / 2 - 1) * is];
    return 0;
  }
  if (w % 2 == 0 && x == w - 1) {  // right border :649-656
    if (h % 2 == 0 && y == h - 1) return in[(h / 2 - 1) * is + w / 2 - 1];
    if ((y & 1) && (y - 1) / 2 < (h - 1) / 2) { int cy = (y - 1) / 2; return (3 * in[(cy / 2) * is + w / 2 - 1] + 1 * in[(cy / 2 + 1) * is + w / 2 - 1] + 2) / 4; }
    if (!(y & 1) && (y - 2) / 2 < (h - 1) / 2) { int cy = (y - 2) / 2; return (1 * in[(cy / 2) * is + w / 2 - 1] + 3 * in[(cy / 2 + 1) * is + w / 2 - 1] + 2) / 4; }
    return 0;
  }
  if (h % 2 == 0 && y == h - 1) {  // bottom border :660-667
    const Pix* row = in + (size_t)(h / 2 - 1) * is;
    if ((x & 1) && (x - 1) / 2 < (w - 1) / 2) { int cx = (x - 1) / 2; return (3 * row[cx / 2] + 1 * row[cx / 2 + 1] + 2) / 4; }
    if (!(x & 1) && (x - 2) / 2 < (w - 1) / 2) { int cx = (x - 2) / 2; return (1 * row[cx / 2] + 3 * row[cx / 2 + 1] + 2) / 4; }
    return 0;
  }
  // interior :678-708
  int xb = (x & 1) ? x : x - 1, yb = (y & 1) ? y : y - 1;
  if (xb >= w - 1 || yb >= h - 1) return 0;
  int cx = xb / 2, cy = yb / 2;
  int c00 = in[cy * is + cx], c01 = in[cy * is + cx + 1], c10 = in[(cy + 1) * is + cx], c11 = in[(cy + 1) * is + cx + 1];
  int wx1 = (x == xb) ? 1 : 3, wx0 = 4 - wx1;  // weight of the right / left chroma sample
  int wy1 = (y == yb) ? 1 : 3, wy0 = 4 - wy1;
  return (c00 * wx0 * wy0 + c01 * wx1 * wy0 + c10 * wx0 * wy1 + c11 * wx1 * wy1 + 8) / 16;
}

template <typename Pix>
__global__ __launch_bounds__(256) void k_bilinear_420_to_444(const uint8_t* in, size_t is, int w, int h, uint8_t* out, size_t os)
{
  const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x0 >= w || y >= h) return;
  const Pix* src = (const Pix*)in;
  Pix* dst = (Pix*)(out + (size_t)y * os);
  const size_t iss = is / sizeof(Pix);
  for (int i = 0; i < 4 && x0 + i < w; i++) dst[x0 + i] = (Pix)bilinear_at<Pix>(src, iss, w, h, x0 + i, y);
}

// Op_YCbCr422_bilinear_to_YCbCr444 (libheif/color-conversion/chroma_sampling.cc:732-954) for one chroma plane: out(0) = in(0); for even widths
// out(w - 1) = in(w / 2 - 1); the pairs (x, x + 1), x odd, between them are (3 a + b + 2) / 4 and (a + 3 b + 2) / 4 of the chroma samples
// a = in(x / 2), b = in(x / 2 + 1) (:911-927).  Four output samples per lane.
template <typename Pix>
__global__ __launch_bounds__(256) void k_bilinear_422_to_444(const uint8_t* in, size_t is, int w, int h, uint8_t* out, size_t os)
{
  const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x0 >= w || y >= h) return;
  const Pix* src = (const Pix*)(in + (size_t)y * is);
  Pix* dst = (Pix*)(out + (size_t)y * os);
  for (int i = 0; i < 4 && x0 + i < w; i++) {
    const int x = x0 + i;
    int v;
    if (x == 0) v = src[0];
    else if (x == w - 1 && (w & 1) == 0) v = src[w / 2 - 1];
    else {
      const int cx = (x - 1) >> 1, a = src[cx], b = src[cx + 1];     // x odd: first of the pair, x even: second
      v = (x & 1) ? (a * 3 + b + 2) / 4 : (a + b * 3 + 2) / 4;
    }
    dst[x] = (Pix)v;
  }
}

__global__ __launch_bounds__(256) void k_to_sdr(const uint8_t* in, size_t is, int w, int h, int shift, uint8_t* out, size_t os)
{
  const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x0 >= w || y >= h) return;
  const uint16_t* src = (const uint16_t*)(in + (size_t)y * is);
  uint8_t* dst = out + (size_t)y * os;
  if (x0 + 3 < w && ((is | (uintptr_t)in) & 7) == 0 && ((os | (uintptr_t)out) & 3) == 0) {
    uint2 v = *(const uint2*)(src + x0);
    uint32_t o = ((v.x & 0xffff) >> shift) | (((v.x >> 16) >> shift) << 8) | (((v.y & 0xffff) >> shift) << 16) | (((v.y >> 16) >> shift) << 24);
    *(uint32_t*)(dst + x0) = o;
  } else {
    for (int i = 0; i < 4 && x0 + i < w; i++) dst[x0 + i] = (uint8_t)(src[x0 + i] >> shift);
  }
}

// Op_to_hdr_planes (libheif/color-conversion/hdr_sdr.cc:25-109): 8-bit plane -> out_bits (<= 16) by replicating the bit pattern
__global__ __launch_bounds__(256) void k_to_hdr(const uint8_t* in, size_t is, int w, int h, int out_bits, uint8_t* out, size_t os)
{
  const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x0 >= w || y >= h) return;
  const uint8_t* src = in + (size_t)y * is;
  uint16_t* dst = (uint16_t*)(out + (size_t)y * os);
  const int shift1 = out_bits - 8, shift2 = 16 - out_bits;
  for (int i = 0; i < 4 && x0 + i < w; i++) { const int v = src[x0 + i]; dst[x0 + i] = (uint16_t)((v << shift1) | (v >> shift2)); }
}

// Op_RRGGBBaa_swap_endianness (libheif/color-conversion/rgb2rgb.cc:647-764): the two bytes of every 16-bit component trade places
__global__ __launch_bounds__(256) void k_swap16(const uint8_t* in, size_t is, int row_bytes, int h, uint8_t* out, size_t os)
{
  const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;     // byte offset, two components per thread
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x0 >= row_bytes || y >= h) return;
  const uint8_t* src = in + (size_t)y * is + x0;
  uint8_t* dst = out + (size_t)y * os + x0;
  if (x0 + 4 <= row_bytes && ((((uintptr_t)src) | ((uintptr_t)dst)) & 3) == 0) {
    const uint32_t v = *(const uint32_t*)src;
    *(uint32_t*)dst = ((v & 0x00ff00ffu) << 8) | ((v >> 8) & 0x00ff00ffu);
  } else {
    for (int i = 0; i + 1 < 4 && x0 + i + 1 < row_bytes; i += 2) { dst[i] = src[i + 1]; dst[i + 1] = src[i]; }
  }
}

// SMPTE ST 2084 / Rec. ITU-R BT.2100 PQ EOTF on code values: E' = v / (2^bits - 1), Y = (max(E'^(1/m2) - c1, 0) / (c2 - c3 E'^(1/m2)))^(1/m1),
// output linear light normalised to 1.0 = 10000 cd/m2, float32.  NOT in the reference (libheif has no transfer-function maths, SURVEY.md §0
// fact 5): BASELINE.json's config 4 asks for it, the oracle is the published formula in fp64 (tests), tolerance 1e-6 relative (the fp32 result's rounding).
__global__ __launch_bounds__(256) void k_pq_to_linear(const uint8_t* in, size_t is, int n_per_row, int h, int bits, int big_endian, float* out, size_t os)
{
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= n_per_row || y >= h) return;
  uint32_t v = ((const uint16_t*)(in + (size_t)y * is))[x];
  if (big_endian) v = ((v & 255u) << 8) | (v >> 8);
  // evaluated in fp64 (the two pow() calls amplify fp32 rounding to ~5e-5 relative; the MI355X has the fp64 rate to spare on a streaming op)
  const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0, c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
  const double e = (double)v / (double)((1u << bits) - 1u);
  const double p = pow(e, 1.0 / m2);
  const double num = fmax(p - c1, 0.0), den = c2 - c3 * p;
  ((float*)((uint8_t*)out + (size_t)y * os))[x] = (float)pow(num / den, 1.0 / m1);
}

// The same for code values of at most 12 bits through a table: the EOTF is a function of the code value alone, so every workgroup evaluates it
// once per code (fp64, exactly the expression above: the entries ARE the per-sample results) into LDS - 4 KB for 10 bit, 16 KB for 12 - and the
// samples become one LDS read each.  A workgroup covers 16 rows x 1024 samples (64 per thread, 8-byte loads / 16-byte stores), so the table costs
// 4 (16) evaluations per thread against 64 samples.  HBM-bound: 2 B in + 4 B out per sample.  (round 4: the per-sample fp64 pow pair ran at
// 0.5 TB/s on BASELINE config 4.)
__global__ __launch_bounds__(256) void k_pq_to_linear_lut(const uint8_t* in, size_t is, int n_per_row, int h, int bits, int big_endian, float* out, size_t os)
{
  __shared__ float lut[4096];
  const int n_codes = 1 << bits;
  const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0, c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
  for (int v = threadIdx.x; v < n_codes; v += 256) {
    const double e = (double)v / (double)((1u << bits) - 1u);
    const double p = pow(e, 1.0 / m2);
    const double num = fmax(p - c1, 0.0), den = c2 - c3 * p;
    lut[v] = (float)pow(num / den, 1.0 / m1);
  }
  __syncthreads();
  const int x0 = blockIdx.x * 1024 + (int)threadIdx.x * 4;
  const int y0 = blockIdx.y * 16;
  const uint32_t mask = (uint32_t)n_codes - 1u;
  for (int r = 0; r < 16; r++) {
    const int y = y0 + r;
    if (y >= h || x0 >= n_per_row) break;
    const uint16_t* src = (const uint16_t*)(in + (size_t)y * is) + x0;
    float* dst = (float*)((uint8_t*)out + (size_t)y * os) + x0;
    uint32_t v[4];
    const bool full = x0 + 4 <= n_per_row && (((uintptr_t)src & 7u) == 0) && (((uintptr_t)dst & 15u) == 0);
    if (full) { const uint2 w = *(const uint2*)src; v[0] = w.x & 0xffffu; v[1] = w.x >> 16; v[2] = w.y & 0xffffu; v[3] = w.y >> 16; }
    else for (int k = 0; k < 4; k++) v[k] = x0 + k < n_per_row ? src[k] : 0u;
    float f[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint32_t c = v[k];
      if (big_endian) c = ((c & 255u) << 8) | (c >> 8);
      if (c <= mask) f[k] = lut[c];
      else {   // a code above 2^bits - 1 (not produced by the colour stage): the formula itself, as k_pq_to_linear
        const double e = (double)c / (double)((1u << bits) - 1u);
        const double p = pow(e, 1.0 / m2);
        f[k] = (float)pow(fmax(p - c1, 0.0) / (c2 - c3 * p), 1.0 / m1);
      }
    }
    if (full) *(float4*)dst = make_float4(f[0], f[1], f[2], f[3]);
    else for (int k = 0; k < 4; k++) if (x0 + k < n_per_row) dst[k] = f[k];
  }
}

// Hybrid log-gamma (ARIB STD-B67 / Rec. ITU-R BT.2100 table 5, the inverse OETF): E = E'^2 / 3 for E' <= 1/2, (exp((E' - c) / a) + b) / 12 above, with
// a = 0.17883277, b = 1 - 4a, c = 1/2 - a ln(4a); per component, scene linear light normalised to 1.0, float32.  (The display's OOTF - a gain over the
// scene luminance with the system gamma of the viewing environment - is the renderer's business and mixes the components; it is not applied.)  Like
// the PQ stage it is NOT in the reference (libheif has no transfer-function maths) and it is the PQ kernels' structure with another curve.
__device__ __forceinline__ double hlg_inverse_oetf(double e)
{
  const double a = 0.17883277, b = 1.0 - 4.0 * a, c = 0.5 - a * log(4.0 * a);
  return e <= 0.5 ? e * e / 3.0 : (exp((e - c) / a) + b) / 12.0;
}
__global__ __launch_bounds__(256) void k_hlg_to_linear(const uint8_t* in, size_t is, int n_per_row, int h, int bits, int big_endian, float* out, size_t os)
{
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= n_per_row || y >= h) return;
  uint32_t v = ((const uint16_t*)(in + (size_t)y * is))[x];
  if (big_endian) v = ((v & 255u) << 8) | (v >> 8);
  ((float*)((uint8_t*)out + (size_t)y * os))[x] = (float)hlg_inverse_oetf((double)v / (double)((1u << bits) - 1u));
}
__global__ __launch_bounds__(256) void k_hlg_to_linear_lut(const uint8_t* in, size_t is, int n_per_row, int h, int bits, int big_endian, float* out, size_t os)
{
  __shared__ float lut[4096];
  const int n_codes = 1 << bits;
  for (int v = threadIdx.x; v < n_codes; v += 256) lut[v] = (float)hlg_inverse_oetf((double)v / (double)((1u << bits) - 1u));
  __syncthreads();
  const int x0 = blockIdx.x * 1024 + (int)threadIdx.x * 4;
  const int y0 = blockIdx.y * 16;
  const uint32_t mask = (uint32_t)n_codes - 1u;
  for (int r = 0; r < 16; r++) {
    const int y = y0 + r;
    if (y >= h || x0 >= n_per_row) break;
    const uint16_t* src = (const uint16_t*)(in + (size_t)y * is) + x0;
    float* dst = (float*)((uint8_t*)out + (size_t)y * os) + x0;
    uint32_t v[4];
    const bool full = x0 + 4 <= n_per_row && (((uintptr_t)src & 7u) == 0) && (((uintptr_t)dst & 15u) == 0);
    if (full) { const uint2 w = *(const uint2*)src; v[0] = w.x & 0xffffu; v[1] = w.x >> 16; v[2] = w.y & 0xffffu; v[3] = w.y >> 16; }
    else for (int k = 0; k < 4; k++) v[k] = x0 + k < n_per_row ? src[k] : 0u;
    float f[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint32_t c = v[k];
      if (big_endian) c = ((c & 255u) << 8) | (c >> 8);
      f[k] = c <= mask ? lut[c] : (float)hlg_inverse_oetf((double)c / (double)((1u << bits) - 1u));   // (a code above 2^bits - 1: the formula itself)
    }
    if (full) *(float4*)dst = make_float4(f[0], f[1], f[2], f[3]);
    else for (int k = 0; k < 4; k++) if (x0 + k < n_per_row) dst[k] = f[k];
  }
}

// ---- host side -------------------------------------------------------------------------------

// libheif/nclx.cc:45-72
bool primaries_of(int idx, float p[8])
{
  static const float t[][9] = {
      {1, 0.300f, 0.600f, 0.150f, 0.060f, 0.640f, 0.330f, 0.3127f, 0.3290f},
      {4, 0.21f, 0.71f, 0.14f, 0.08f, 0.67f, 0.33f, 0.310f, 0.316f},
      {5, 0.29f, 0.60f, 0.15f, 0.06f, 0.64f, 0.33f, 0.3127f, 0.3290f},
      {6, 0.310f, 0.595f, 0.155f, 0.070f, 0.630f, 0.340f, 0.3127f, 0.3290f},
      {7, 0.310f, 0.595f, 0.155f, 0.070f, 0.630f, 0.340f, 0.3127f, 0.3290f},
      {8, 0.243f, 0.692f, 0.145f, 0.049f, 0.681f, 0.319f, 0.310f, 0.316f},
      {9, 0.170f, 0.797f, 0.131f, 0.046f, 0.708f, 0.292f, 0.3127f, 0.3290f},
      {10, 0.0f, 1.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.333333f, 0.33333f},
      {11, 0.265f, 0.690f, 0.150f, 0.060f, 0.680f, 0.320f, 0.314f, 0.351f},
      {12, 0.265f, 0.690f, 0.150f, 0.060f, 0.680f, 0.320f, 0.3127f, 0.3290f},
      {22, 0.295f, 0.605f, 0.155f, 0.077f, 0.630f, 0.340f, 0.3127f, 0.3290f}};
  for (auto& r : t)
    if ((int)r[0] == idx) { memcpy(p, &r[1], 8 * sizeof(float)); return true; }
  memset(p, 0, 8 * sizeof(float));
  return false;
}

// libheif/nclx.cc:84-173.  Host float arithmetic, contraction off, same operation order.
void coefficients(const hipdec_nclx* n, float out[4])
{
  float Kr = 0, Kb = 0;
  if (n && n->has_nclx) {
    int m = n->matrix_coefficients;
    if (m == 12 || m == 13) {
      float p[8];
      primaries_of(n->colour_primaries, p);
      float gx = p[0], gy = p[1], bx = p[2], by = p[3], rx = p[4], ry = p[5], wx = p[6], wy = p[7];
      float zr = 1 - (rx + ry), zg = 1 - (gx + gy), zb = 1 - (bx + by), zw = 1 - (wx + wy);
      float denom = wy * (rx * (gy * zb - by * zg) + gx * (by * zr - ry * zb) + bx * (ry * zg - gy * zr));
      if (denom != 0.0f) {
        Kr = (ry * (wx * (gy * zb - by * zg) + wy * (bx * zg - gx * zb) + zw * (gx * by - bx * gy))) / denom;
        Kb = (by * (wx * (ry * zg - gy * zr) + wy * (gx * zr - rx * zg) + zw * (rx * gy - gx * ry))) / denom;
      }
    } else {
      switch (m) {
        case 1: Kr = 0.2126f; Kb = 0.0722f; break;
        case 4: Kr = 0.30f; Kb = 0.11f; break;
        case 5: case 6: Kr = 0.299f; Kb = 0.114f; break;
        case 7: Kr = 0.212f; Kb = 0.087f; break;
        case 9: case 10: Kr = 0.2627f; Kb = 0.0593f; break;
        default: break;
      }
    }
  }
  if (Kb != 0 || Kr != 0) {
    out[0] = 2 * (-Kr + 1);
    out[1] = 2 * Kb * (-Kb + 1) / (Kb + Kr - 1);
    out[2] = 2 * Kr * (-Kr + 1) / (Kb + Kr - 1);
    out[3] = 2 * (-Kb + 1);
  } else {
    out[0] = 1.402f; out[1] = -0.344136f; out[2] = -0.714136f; out[3] = 1.772f;
  }
}

// Capture mode (hipdec_batch_to_rgb_all): the per-picture entry points run their argument checks and the planner rules
// as usual, but instead of launching they record the parameter block; the recorded blocks then go out as one launch.
struct Captured { ColorParams p; int variant; };
thread_local std::vector<Captured> t_captured;
thread_local bool t_capture = false;

// Scaled output: a request set on this thread (hipdec::color_scale_request) turns the NEXT launch of an interleaved layout into the fused scale + colour
// kernel - run at once, or recorded in capture mode (hipdec_batch_to_rgb_scaled_all).  The launch that takes the request clears it, and the caller checks
// that it was taken (hipdec::color_scale_pending), so an entry point that does not come through launch_rgb is refused instead of writing a full-size picture.
struct ScaleReq { bool on = false; int ow = 0, oh = 0, filter = 0, sH = 0, sV = 0; };
thread_local ScaleReq t_scale;
struct CapturedScaled { ScaledParams p; int variant; int filter; };
thread_local std::vector<CapturedScaled> t_captured_scaled;

// Tensor output: a request set on this thread (hipdec::color_tensor_request) makes the NEXT launch of an interleaved layout RECORD a tensor block instead;
// the recorded blocks go out as one launch (hipdec::color_tensor_launch).  Taken and checked like a scale request.
struct TensorReq { bool on = false; hipdec::TensorRequest r; };
thread_local TensorReq t_tensor;
struct CapturedTensor {
  TensorParams p;
  int wide;          // the source planes hold uint16_t samples
  int oriented;      // for the k_oriented_* kernels, with a code, a row pitch and the rows of a channel plane
  int code;          // (set for every resampled entry too)
  uint64_t pitch;
  int plane_rows;
  int resample;      // the filter, for k_resample
  int patch, merge;  // patch > 0: a patch sequence, for the k_patch_* kernels
  int tpatch;        // clips: frames per token
  int strided;       // clips: the entry goes to k_clip_box
  int framed;        // for the k_frame_* kernels: vis is the window in displayed coordinates of the sample
  int vis[4];
};
thread_local std::vector<CapturedTensor> t_captured_tensor;

// ---- the coefficient tables of HIPDEC_SCALE_BILINEAR / _BICUBIC: Pillow's precompute_coeffs + normalize_coeffs_8bpc (src/libImaging/Resample.c), statement
// by statement as include/heif_hipdec.h gives them.  IEEE double, no contraction (this file is built with -ffp-contract=off): the ORDER of operations is
// part of the definition.
double resample_filter_value(int filter, double x)
{
  if (x < 0.0) x = -x;
  if (filter == HIPDEC_SCALE_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
  const double a = -0.5;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

struct ResampleAxis {
  double scale, support, ss;
  int n_in, filter, stride;   // stride: taps an output sample can have ((int)ceil(support) * 2 + 1, Pillow's ksize)
};
ResampleAxis resample_axis_of(int n_in, int n_out, int filter)
{
  ResampleAxis a;
  a.n_in = n_in; a.filter = filter;
  a.scale = (double)n_in / n_out;
  const double fs = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = (filter == HIPDEC_SCALE_BILINEAR ? 1.0 : 2.0) * fs;
  a.ss = 1.0 / fs;
  a.stride = (int)std::ceil(a.support) * 2 + 1;
  return a;
}

// the taps of output sample xx: *first = xmin, k[0 .. n) the coefficients (k and w hold a.stride elements); returns n
int resample_taps_of(const ResampleAxis& a, int xx, int* first, int32_t* k, double* w)
{
  const double center = (xx + 0.5) * a.scale;
  int xmin = (int)(center - a.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + a.support + 0.5);
  if (xmax > a.n_in) xmax = a.n_in;
  int n = xmax - xmin;
  if (n > a.stride) n = a.stride;   // (cannot happen: ceil(support) * 2 + 1 covers the range)
  double ww = 0.0;
  for (int x = 0; x < n; x++) {
    w[x] = resample_filter_value(a.filter, (x + xmin - center + 0.5) * a.ss);
    ww += w[x];
  }
  for (int x = 0; x < n; x++) {
    if (ww != 0.0) w[x] /= ww;
    k[x] = (int)(w[x] * 4194304.0 + (w[x] < 0 ? -0.5 : 0.5));
  }
  *first = xmin;
  return n < 0 ? 0 : n;
}

// ints of the table of an axis: n_out records (first, count), then n_out rows of `stride` coefficients
uint64_t resample_table_ints(int n_in, int n_out, int filter)
{
  return (uint64_t)n_out * (2ull + (uint64_t)resample_axis_of(n_in, n_out, filter).stride);
}

void resample_table_fill(int n_in, int n_out, int filter, int32_t* t)
{
  const ResampleAxis a = resample_axis_of(n_in, n_out, filter);
  std::vector<double> w((size_t)a.stride);
  int32_t* k = t + 2 * (size_t)n_out;
  for (int xx = 0; xx < n_out; xx++, k += a.stride) {
    int first = 0;
    const int n = resample_taps_of(a, xx, &first, k, w.data());
    for (int x = n; x < a.stride; x++) k[x] = 0;
    t[2 * (size_t)xx] = first; t[2 * (size_t)xx + 1] = n;
  }
}

// output columns per workgroup of k_resample: as many (whole 4-pixel groups, at most kResTC) as have their taps inside one staged chunk of kResSpan columns
int resample_tile_of(int n_in, int n_out, int filter)
{
  const ResampleAxis a = resample_axis_of(n_in, n_out, filter);
  double t = ((double)kResSpan - 6.0 - 2.0 * a.support) / a.scale;
  if (t > kResTC) t = kResTC;
  if (t < 1) t = 1;                                     // taps wider than the chunk: the kernel's chunk loop
  int ti = (int)t;
  if (ti >= 4) ti &= ~3;
  return ti;
}

int box_tile_of(int pw, int qw)
{
  long long t = (long long)(kBoxSpan - 4) * qw / pw;   // span of t boxes <= t * pw / qw + 1 columns, + 3 in front of it for the aligned start
  if (t > 256) t = 256;
  if (t < 1) t = 1;                                     // a box wider than the span: the kernel's chunk loop
  if (t >= 4) t &= ~3ll;                                // whole 4-pixel store groups
  return (int)t;
}

// ---- the launch kit: what the batched launches of every output form share
// A launch's block array lives in st.dev, the bytes last sent to it in st.host.  blocks_reserve makes room (from the arena pool: hipFree() would synchronise
// the device every time a batch is retired) and forgets st.host when the memory is new, so that the next compare cannot match stale bytes; blocks_upload
// sends `host` unless the device already holds these bytes - the steady state of a training loop.  A form that writes addresses inside st.dev into its
// blocks fills them between the two.
int blocks_reserve(hipdec::ColorBatchState& st, size_t bytes)
{
  if (st.dev_bytes >= bytes) return 0;
  if (st.dev) hipdec::arena_release(st.dev, st.dev_bytes);
  st.dev = nullptr; st.dev_bytes = 0; st.host.clear();
  HIPDEC_CHECK_HIP(hipdec::arena_acquire(&st.dev, bytes, &st.dev_bytes));
  return 0;
}
int blocks_upload(hipdec::ColorBatchState& st, std::vector<uint8_t>& host, hipStream_t s)
{
  if (st.host == host) return 0;
  st.prev.swap(st.host);   // (not freed while its copy may be pending)
  st.host.swap(host);
  HIPDEC_CHECK_HIP(hipMemcpyAsync(st.dev, st.host.data(), st.host.size(), hipMemcpyHostToDevice, s));
  return 0;
}
// the parameter blocks `p` of recorded entries, in recording order, as the block array of st
template <typename Cap>
int blocks_of_captured(const std::vector<Cap>& caps, hipdec::ColorBatchState& st, hipStream_t s)
{
  const size_t each = sizeof(caps[0].p);
  std::vector<uint8_t> host(caps.size() * each);
  for (size_t i = 0; i < caps.size(); i++) memcpy(host.data() + i * each, &caps[i].p, each);
  if (int rc = blocks_reserve(st, host.size())) return rc;
  return blocks_upload(st, host, s);
}

// f(DtypeTag) for a hipdec_tensor_dtype, f(PixTag, DtypeTag) for a source width and a dtype: the kernel's template arguments as the types of a generic
// lambda's parameters.  false: no such dtype (the caller refuses it in its own words)
template <int DT> using DtypeTag = std::integral_constant<int, DT>;
template <typename Pix> struct PixTag { typedef Pix type; };
template <typename F>
bool dispatch_dtype(int dtype, F&& f)
{
  switch (dtype) {
    case TD_U8: f(DtypeTag<TD_U8>()); return true;
    case TD_F32: f(DtypeTag<TD_F32>()); return true;
    case TD_F16: f(DtypeTag<TD_F16>()); return true;
    case TD_BF16: f(DtypeTag<TD_BF16>()); return true;
    default: return false;
  }
}
template <typename F>
bool dispatch_pix_dtype(int wide, int dtype, F&& f)
{
  if (wide) return dispatch_dtype(dtype, [&](auto dt) { f(PixTag<uint16_t>(), dt); });
  return dispatch_dtype(dtype, [&](auto dt) { f(PixTag<uint8_t>(), dt); });
}

// the two grid shapes of the scaling kernels over n entries.  Box (and the resampling filters): a workgroup per column tile and row (the kernels stride over
// rows beyond the grid's y extent); nearest: a lane per 4 x 4 pixels of the largest output
struct LaunchShape { dim3 block, grid; };
LaunchShape box_grid(int tiles, int rows, size_t n) { return {dim3(256), dim3(tiles, std::min(rows, 65535), (unsigned)n)}; }
LaunchShape nearest_grid(int ow, int oh, size_t n) { return {dim3(64, 4), dim3(((ow + 3) / 4 + 63) / 64, std::min((oh + 3) / 4, 16384), (unsigned)n)}; }
// HIPDEC_SCALE_BOX: `box` over box_grid(tiles, rows, n); otherwise `nearest` over nearest_grid(ow, oh, n)
template <typename Box, typename Nearest, typename Arg>
void launch_box_or_nearest(int filter, Box box, Nearest nearest, int tiles, int rows, int ow, int oh, size_t n, hipStream_t s, const Arg& arg)
{
  const LaunchShape g = filter == HIPDEC_SCALE_BOX ? box_grid(tiles, rows, n) : nearest_grid(ow, oh, n);
  if (filter == HIPDEC_SCALE_BOX) hipLaunchKernelGGL(box, g.grid, g.block, 0, s, arg);
  else hipLaunchKernelGGL(nearest, g.grid, g.block, 0, s, arg);
}

// A grid's z extent is 65535: entries [first, end) go out in as few launches as that allows.  launch(first, n) issues one (non-zero: its refusal ends the
// loop); a launch that fails is reported as "<what>: <error>", one that went out is counted in *launches
template <typename F>
int launch_z_chunks(size_t first, size_t end, const char* what, std::atomic<uint64_t>* launches, F&& launch)
{
  for (; first < end; first += 65535) {
    if (int rc = launch(first, end - first < 65535 ? end - first : (size_t)65535)) return rc;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hipdec::set_error(HIPDEC_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
    if (launches) ++*launches;
  }
  return 0;
}

template <typename Pix, int LAYOUT>
int launch_rgb_scaled(const ColorParams& p, hipStream_t s)
{
  if constexpr (LAYOUT == LO_PLANAR) return hipdec::set_error(HIPDEC_ERR_UNSUPPORTED, "scaled colour stage: interleaved outputs only");
  else {
  if (p.a) return hipdec::set_error(HIPDEC_ERR_UNSUPPORTED, "scaled colour stage: no alpha plane");
  ScaledParams sp;
  memset(&sp, 0, sizeof(sp));
  sp.c = p; sp.ow = t_scale.ow; sp.oh = t_scale.oh; sp.sH = t_scale.sH; sp.sV = t_scale.sV;
  sp.tile = box_tile_of(p.w, sp.ow);
  const int filter = t_scale.filter;
  t_scale.on = false;   // taken
  if (t_capture) { t_captured_scaled.push_back(CapturedScaled{sp, (int)sizeof(Pix) * 16 + LAYOUT, filter}); return 0; }
  launch_box_or_nearest(filter, k_scale_rgb_box<Pix, LAYOUT>, k_scale_rgb_nearest<Pix, LAYOUT>, (sp.ow + sp.tile - 1) / sp.tile, sp.oh, sp.ow, sp.oh, 1, s, sp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hipdec::set_error(HIPDEC_ERR_DEVICE, "scaled colour kernel launch: %s", hipGetErrorString(e));
  return 0;
  }
}

// the entry points a tensor request reaches end in RGB24 (the 8-bit value, to-SDR shifts included) or little-endian RRGGBB (the native-depth value)
template <typename Pix, int LAYOUT>
int record_tensor(const ColorParams& p)
{
  if constexpr (LAYOUT != LO_RGB24 && LAYOUT != LO_RRGGBB_LE) return hipdec::set_error(HIPDEC_ERR_UNSUPPORTED, "tensor output: not a colour entry point it takes");
  else {
  if (p.a) return hipdec::set_error(HIPDEC_ERR_UNSUPPORTED, "tensor output: no alpha plane");
  const hipdec::TensorRequest& r = t_tensor.r;
  TensorParams tp;
  memset(&tp, 0, sizeof(tp));
  tp.c = p; tp.ow = r.ow; tp.oh = r.oh; tp.sH = r.sH; tp.sV = r.sV;
  tp.left = r.left; tp.top = r.top; tp.rw = r.rw; tp.rh = r.rh; tp.flip = r.flip ? 1 : 0; tp.nhwc = r.nhwc ? 1 : 0;
  for (int c = 0; c < 3; c++) { tp.scale[c] = r.scale[c]; tp.bias[c] = r.bias[c]; }
  tp.tile = r.resample ? resample_tile_of(r.rw, r.ow, r.resample) : box_tile_of(r.rw, r.ow);
  if (r.resample) {
    if constexpr (LAYOUT != LO_RGB24) return hipdec::set_error(HIPDEC_ERR_UNSUPPORTED, "resampled output: 8-bit component values only");
    tp.flip = 0;      // folded into the code
  } else if (r.oriented && r.strided_box) {   // k_clip_box: k_tensor_box's tile, no quarter-turn stage to fit
    tp.flip = 0;      // folded into the code
  } else if (r.oriented) {   // (r.ow x r.oh: the pre-orientation size; the quarter-turn stage holds kOrientedTile columns)
    const int cap = sizeof(Pix) == 1 ? OrientedTile<uint8_t, TD_U8>::TC : OrientedTile<uint16_t, TD_U8>::TC;
    tp.tile = tp.tile < cap ? tp.tile : cap;
    tp.flip = 0;      // folded into the code
  }
  t_tensor.on = false;   // taken
  t_captured_tensor.push_back(CapturedTensor{tp, sizeof(Pix) == 2, r.oriented ? 1 : 0, r.code, (uint64_t)r.pitch, r.plane_rows, r.resample, r.patch, r.merge, r.tpatch > 1 ? r.tpatch : 1,
                                             r.oriented && !r.resample && !r.patch && r.strided_box ? 1 : 0, r.oriented && !r.patch ? r.framed : 0,
                                             {r.frame_vis[0], r.frame_vis[1], r.frame_vis[2], r.frame_vis[3]}});
  return 0;
  }
}

template <typename Pix, int LAYOUT>
int launch_rgb(const ColorParams& p, hipStream_t s)
{
  if (t_tensor.on) return record_tensor<Pix, LAYOUT>(p);
  if (t_scale.on) return launch_rgb_scaled<Pix, LAYOUT>(p, s);
  if (t_capture) { t_captured.push_back(Captured{p, (int)sizeof(Pix) * 16 + LAYOUT}); return 0; }
  dim3 block(64, 4);
  dim3 grid(((p.w + 3) / 4 + 63) / 64, ((p.h + 1) / 2 + 3) / 4);
  hipLaunchKernelGGL((k_ycbcr_to_rgb<Pix, LAYOUT>), grid, block, 0, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hipdec::set_error(HIPDEC_ERR_DEVICE, "colour kernel launch: %s", hipGetErrorString(e));
  return 0;
}

int fill_common(ColorParams& p, const void* y, size_t ys, const void* cb, size_t cbs, const void* cr, size_t crs, int w,
                int h, int bpp, int chroma, const hipdec_nclx* nclx)
{
  if (!y || !cb || !cr || w <= 0 || h <= 0) return hipdec::set_error(HIPDEC_ERR_INVALID_ARGUMENT, "colour: bad plane arguments");
  if (chroma < 1 || chroma > 3) return hipdec::set_error(HIPDEC_ERR_INVALID_ARGUMENT, "colour: chroma must be 1 (420), 2 (422) or 3 (444)");
  memset(&p, 0, sizeof(p));
  p.y = (const uint8_t*)y; p.cb = (const uint8_t*)cb; p.cr = (const uint8_t*)cr;
  p.ys = ys; p.cbs = cbs; p.crs = crs; p.w = w; p.h = h; p.bpp = bpp;
  p.shiftH = chroma == 3 ? 0 : 1;
  p.shiftV = chroma == 1 ? 1 : 0;
  float c[4];
  coefficients(nclx, c);
  p.f_r_cr = c[0]; p.f_g_cb = c[1]; p.f_g_cr = c[2]; p.f_b_cb = c[3];
  p.i_r_cr = (int)std::lround(256 * c[0]); p.i_g_cb = (int)std::lround(256 * c[1]);
  p.i_g_cr = (int)std::lround(256 * c[2]); p.i_b_cb = (int)std::lround(256 * c[3]);
  p.full_range = (nclx && nclx->has_nclx) ? nclx->full_range_flag : 1;
  return 0;
}

// arithmetic selection of Op_YCbCr_to_RGB (yuv2rgb.cc:208-282)
int generic_arith(const hipdec_nclx* nclx)
{
  int matrix = (nclx && nclx->has_nclx) ? nclx->matrix_coefficients : 2;
  int full = (nclx && nclx->has_nclx) ? nclx->full_range_flag : 1;
  if (matrix == 0) return full ? AR_GBR_FULL : AR_GBR_LIMITED;
  if (matrix == 8) return AR_YCGCO;
  if (matrix == 16) return AR_YCGCO_RE;
  return AR_FLOAT;
}

template <typename Pix, int LAYOUT>
void launch_rgb_batch(const ColorParams* dev, int n, int max_w, int max_h, hipStream_t s)
{
  dim3 block(64, 4);
  dim3 grid(((max_w + 3) / 4 + 63) / 64, ((max_h + 1) / 2 + 3) / 4, n);
  hipLaunchKernelGGL((k_ycbcr_to_rgb_batch<Pix, LAYOUT>), grid, block, 0, s, dev);
}

}  // namespace

// variant = sizeof(Pix) * 16 + LAYOUT, as recorded by launch_rgb
#define HIPDEC_RGB_VARIANTS(X)                                                                                     \
  X(16 + LO_PLANAR, uint8_t, LO_PLANAR) X(32 + LO_PLANAR, uint16_t, LO_PLANAR) X(16 + LO_RGB24, uint8_t, LO_RGB24) \
  X(16 + LO_RGBA32, uint8_t, LO_RGBA32) X(32 + LO_RRGGBB_BE, uint16_t, LO_RRGGBB_BE) X(32 + LO_RRGGBB_LE, uint16_t, LO_RRGGBB_LE)                     \
  X(32 + LO_RGB24, uint16_t, LO_RGB24) X(32 + LO_RGBA32, uint16_t, LO_RGBA32)

#define HIPDEC_RGB_SCALED_VARIANTS(X)                                                                              \
  X(16 + LO_RGB24, uint8_t, LO_RGB24) X(16 + LO_RGBA32, uint8_t, LO_RGBA32) X(32 + LO_RRGGBB_BE, uint16_t, LO_RRGGBB_BE) \
  X(32 + LO_RRGGBB_LE, uint16_t, LO_RRGGBB_LE) X(32 + LO_RGB24, uint16_t, LO_RGB24) X(32 + LO_RGBA32, uint16_t, LO_RGBA32)

namespace hipdec {

void color_capture_begin()
{
  t_captured_scaled.clear();
  t_captured.clear();
  t_capture = true;
}

void color_capture_abort()
{
  t_captured_scaled.clear();
  t_captured.clear();
  t_capture = false;
}

// Ends capture mode WITHOUT launching: uploads the recorded parameter blocks (one per captured call, in call order) and hands back the
// device array — for a kernel of another translation unit that consumes them (SAO with fused RGB emission, filter_kernels.hip).
// *uniform_variant = the kernel variant all blocks share (sizeof(Pix) * 16 + LAYOUT), or -1 when they differ.
int color_capture_take(ColorBatchState& st, hipStream_t s, const void** dev, int* uniform_variant, int* count)
{
  t_capture = false;
  std::vector<Captured> caps;
  caps.swap(t_captured);
  *dev = nullptr; *uniform_variant = -1; *count = (int)caps.size();
  if (caps.empty()) return 0;
  bool same = true;
  for (const auto& c : caps) same = same && c.variant == caps[0].variant;
  if (int rc = blocks_of_captured(caps, st, s)) return rc;
  *dev = st.dev;
  if (same) *uniform_variant = caps[0].variant;
  return 0;
}
int color_variant_rgb24_u8() { return (int)sizeof(uint8_t) * 16 + LO_RGB24; }

int color_capture_launch(ColorBatchState& st, hipStream_t s)
{
  t_capture = false;
  std::vector<Captured> caps;
  caps.swap(t_captured);
  if (caps.empty()) return 0;
  bool same = true;
  int max_w = 0, max_h = 0;
  for (const auto& c : caps) { same = same && c.variant == caps[0].variant; max_w = c.p.w > max_w ? c.p.w : max_w; max_h = c.p.h > max_h ? c.p.h : max_h; }
  if (!same || caps.size() == 1) {   // mixed kernel variants cannot share a launch
    for (const auto& c : caps) {
      int rc = HIPDEC_ERR_UNSUPPORTED;
      switch (c.variant) {
#define X(id, Pix, LO) case id: rc = launch_rgb<Pix, LO>(c.p, s); break;
        HIPDEC_RGB_VARIANTS(X)
#undef X
        default: break;
      }
      if (rc) return rc;
    }
    return 0;
  }
  if (int rc = blocks_of_captured(caps, st, s)) return rc;
  const ColorParams* dev = (const ColorParams*)st.dev;
  switch (caps[0].variant) {
#define X(id, Pix, LO) case id: launch_rgb_batch<Pix, LO>(dev, (int)caps.size(), max_w, max_h, s); break;
    HIPDEC_RGB_VARIANTS(X)
#undef X
    default: return set_error(HIPDEC_ERR_UNSUPPORTED, "colour batch: unknown kernel variant");
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(HIPDEC_ERR_DEVICE, "colour batch launch: %s", hipGetErrorString(e));
  return 0;
}

void color_scale_request(int out_width, int out_height, int filter, int sH, int sV)
{
  t_scale.on = true; t_scale.ow = out_width; t_scale.oh = out_height; t_scale.filter = filter; t_scale.sH = sH; t_scale.sV = sV;
}
void color_scale_clear() { t_scale.on = false; }
bool color_scale_pending() { return t_scale.on; }

// hipdec_batch_to_rgb_scaled_all: the scaled blocks recorded since color_capture_begin() as one launch
int color_capture_launch_scaled(ColorBatchState& st, int filter, hipStream_t s)
{
  t_capture = false;
  std::vector<CapturedScaled> caps;
  caps.swap(t_captured_scaled);
  if (caps.empty()) return 0;
  int max_ow = 0, max_oh = 0, max_tiles = 0;
  for (const auto& c : caps) {
    if (c.variant != caps[0].variant || c.filter != filter) return set_error(HIPDEC_ERR_UNSUPPORTED, "scaled colour batch: the items select different kernel variants");
    max_ow = c.p.ow > max_ow ? c.p.ow : max_ow; max_oh = c.p.oh > max_oh ? c.p.oh : max_oh;
    const int tiles = (c.p.ow + c.p.tile - 1) / c.p.tile;
    max_tiles = tiles > max_tiles ? tiles : max_tiles;
  }
  if (int rc = blocks_of_captured(caps, st, s)) return rc;
  const ScaledParams* dev = (const ScaledParams*)st.dev;
  switch (caps[0].variant) {
#define X(id, Pix, LO) \
  case id: launch_box_or_nearest(filter, k_scale_rgb_box_batch<Pix, LO>, k_scale_rgb_nearest_batch<Pix, LO>, max_tiles, max_oh, max_ow, max_oh, caps.size(), s, dev); break;
    HIPDEC_RGB_SCALED_VARIANTS(X)
#undef X
    default: return set_error(HIPDEC_ERR_UNSUPPORTED, "scaled colour batch: unknown kernel variant");
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(HIPDEC_ERR_DEVICE, "scaled colour batch launch: %s", hipGetErrorString(e));
  return 0;
}

void color_tensor_request(const TensorRequest& r) { t_tensor.on = true; t_tensor.r = r; }
void color_tensor_clear() { t_tensor.on = false; }
bool color_tensor_pending() { return t_tensor.on; }
void color_tensor_begin() { t_captured_tensor.clear(); }
void color_tensor_abort() { t_captured_tensor.clear(); t_tensor.on = false; }

namespace {
std::atomic<uint64_t> g_oriented_launches{0}, g_oriented_entries{0}, g_oriented_quarter{0};

// the blocked store's constants of an entry (PatchInfo above): its displayed width is a multiple of patch * merge
PatchInfo patch_info_of(const CapturedTensor& c)
{
  PatchInfo b;
  memset(&b, 0, sizeof(b));
  const uint32_t P = (uint32_t)c.patch, m = (uint32_t)c.merge, dw = (uint32_t)(c.code & 1 ? c.p.oh : c.p.ow);
  auto magic = [](uint32_t d) { const uint64_t v = (1ull << 32) / d; return (uint32_t)(v > 0xffffffffull ? 0xffffffffull : v); };
  b.P = P; b.m = m; b.magicP = magic(P); b.magicM = magic(m);
  const uint32_t Tp = c.tpatch > 1 ? (uint32_t)c.tpatch : 1u;   // a clip's token holds Tp frames: the frame's place in it is part of the entry's first element
  b.tok = 3u * Tp * P * P; b.tokm = m * m * b.tok; b.mtok = m * b.tok;
  b.pxs = c.p.nhwc ? 3u : 1u; b.chs = c.p.nhwc ? 1u : Tp * P * P; b.prow = P * b.pxs;
  b.rowtok = (uint64_t)(dw / P / m) * (uint64_t)b.tokm;
  return b;
}

std::atomic<uint64_t> g_packed_calls{0}, g_packed_entries{0}, g_packed_patch_entries{0};
std::atomic<uint64_t> g_clip_box_entries{0};

// the window of a framed entry (hipdec::FrameWindow): the displayed one as recorded, and the columns and rows of P it covers - with code = r + 4 * m
// (OrientedParams above) a displayed axis is an axis of P, forward or reversed: X in [lo, hi) reversed over n is n - hi .. n - lo
hipdec::FrameWindow frame_window_of(const CapturedTensor& c)
{
  hipdec::FrameWindow f;
  memset(&f, 0, sizeof(f));
  f.vx0 = c.vis[0]; f.vy0 = c.vis[1]; f.vx1 = c.vis[2]; f.vy1 = c.vis[3];
  const int quarter = c.code & 1, fx = ((c.code >> 1) ^ (c.code >> 2)) & 1, fy = ((c.code >> 1) ^ c.code) & 1;
  auto back = [](int lo, int hi, int n, int flip, int* a, int* b) { *a = flip ? n - hi : lo; *b = flip ? n - lo : hi; };
  if (!quarter) { back(f.vx0, f.vx1, c.p.ow, fx, &f.px0, &f.px1); back(f.vy0, f.vy1, c.p.oh, fy, &f.py0, &f.py1); }
  else { back(f.vx0, f.vx1, c.p.oh, fx, &f.py0, &f.py1); back(f.vy0, f.vy1, c.p.ow, fy, &f.px0, &f.px1); }
  return f;
}

// hipdec_framed_stats: the pieces of work of the framed entries - a column tile x a block of rows (box), a column tile x a band (the resampling filters),
// a workgroup's 256 x 4 displayed pixels (nearest) - that hold a visible pixel, and those that hold none: the host's geometry, counted per launch
std::atomic<uint64_t> g_framed_calls{0}, g_framed_entries{0}, g_framed_tiles{0}, g_framed_skipped{0};
struct FrameTileCount {
  uint64_t tiles = 0, skipped = 0;
  int max_x = 0, max_y = 0;   // the most pieces with a visible pixel an entry has along either axis: the grid
  // nx x ny samples in pieces of ux x uy, of which [x0, x1) x [y0, y1) is visible; sets the entry's origin
  void add(hipdec::FrameWindow* f, int nx, int ux, int x0, int x1, int ny, int uy, int y0, int y1)
  {
    f->tx0 = x0 / ux; f->ty0 = y0 / uy;
    const int hx = (x1 - 1) / ux - f->tx0 + 1, hy = (y1 - 1) / uy - f->ty0 + 1;
    const uint64_t all = (uint64_t)((nx + ux - 1) / ux) * (uint64_t)((ny + uy - 1) / uy), hit = (uint64_t)hx * (uint64_t)hy;
    tiles += hit; skipped += all - hit;
    max_x = hx > max_x ? hx : max_x; max_y = hy > max_y ? hy : max_y;
  }
  // (composed: the pieces of a composed call - framed 2 - are hipdec_composed_stats', counted by the call)
  void commit(bool composed) const { if (!composed) { g_framed_tiles += tiles; g_framed_skipped += skipped; } }
};

// the oriented form of color_tensor_launch: entries of all codes and (RGB form) sizes share the launch, so the grid covers the largest of each extent
int oriented_launch(std::vector<CapturedTensor>& caps, ColorBatchState& st, int filter, int dtype, hipStream_t s)
{
  int max_tiles = 0, max_dw = 0, max_dh = 0, max_blocks = 0;
  uint64_t quarter = 0;
  // rows of P per workgroup: the kernel's RB where a row of P becomes a column (the length of a contiguous run), 16 where rows stay rows (more workgroups)
  const int RB = !caps[0].wide || dtype == TD_U8 ? OrientedTile<uint8_t, TD_U8>::RB : OrientedTile<uint16_t, TD_F32>::RB;
  auto block_rows = [&](const CapturedTensor& c) { return c.code & 1 ? RB : 16; };
  // clips: the box entries for k_clip_box come first in the block array and go out as a launch of their own, with k_tensor_box's grid
  size_t n_clip = 0;
  int clip_tiles = 0, clip_oh = 0;
  if (filter == HIPDEC_SCALE_BOX) {
    std::stable_partition(caps.begin(), caps.end(), [](const CapturedTensor& c) { return c.strided != 0; });
    while (n_clip < caps.size() && caps[n_clip].strided) n_clip++;
  }
  for (size_t i = 0; i < caps.size(); i++) {
    const CapturedTensor& c = caps[i];
    if (c.wide != caps[0].wide) return set_error(HIPDEC_ERR_UNSUPPORTED, "oriented output: the entries mix 8-bit and wider sources");
    const int tiles = (c.p.ow + c.p.tile - 1) / c.p.tile;
    if (i < n_clip) { clip_tiles = tiles > clip_tiles ? tiles : clip_tiles; clip_oh = c.p.oh > clip_oh ? c.p.oh : clip_oh; continue; }
    const int dw = c.code & 1 ? c.p.oh : c.p.ow, dh = c.code & 1 ? c.p.ow : c.p.oh;
    max_tiles = tiles > max_tiles ? tiles : max_tiles;
    const int blocks = (c.p.oh + block_rows(c) - 1) / block_rows(c);
    max_dw = dw > max_dw ? dw : max_dw; max_dh = dh > max_dh ? dh : max_dh; max_blocks = blocks > max_blocks ? blocks : max_blocks;
    quarter += (uint64_t)(c.code & 1);
  }
  const bool blocked = caps[0].patch > 0;   // (a call's entries are all patch sequences, or none is): PatchParams blocks for the k_patch_* kernels
  const bool framed = !blocked && caps[0].framed;   // (... are all framed, or none is): FrameParams blocks for the k_frame_* kernels
  const size_t block_bytes = blocked ? sizeof(PatchParams) : (framed ? sizeof(FrameParams) : sizeof(OrientedParams));
  const size_t bytes = caps.size() * block_bytes;
  std::vector<uint8_t> host(bytes);
  FrameTileCount frame_tiles;
  for (size_t i = 0; i < caps.size(); i++) {
    OrientedParams op;
    memset(&op, 0, sizeof(op));
    op.t = caps[i].p; op.code = (uint16_t)caps[i].code; op.rb = (uint16_t)block_rows(caps[i]); op.pitch = caps[i].pitch; op.plane_rows = caps[i].plane_rows;
    memcpy(host.data() + i * block_bytes, &op, sizeof(op));
    if (blocked) {
      const PatchInfo b = patch_info_of(caps[i]);
      memcpy(host.data() + i * block_bytes + offsetof(PatchParams, b), &b, sizeof(b));
    }
    if (framed) {
      hipdec::FrameWindow f = frame_window_of(caps[i]);
      const int dw = caps[i].code & 1 ? caps[i].p.oh : caps[i].p.ow, dh = caps[i].code & 1 ? caps[i].p.ow : caps[i].p.oh;
      if (filter == HIPDEC_SCALE_BOX) frame_tiles.add(&f, caps[i].p.ow, caps[i].p.tile, f.px0, f.px1, caps[i].p.oh, block_rows(caps[i]), f.py0, f.py1);
      else frame_tiles.add(&f, dw, 256, f.vx0, f.vx1, dh, 4, f.vy0, f.vy1);
      memcpy(host.data() + i * block_bytes + offsetof(FrameParams, b), &f, sizeof(f));
    }
  }
  if (framed) {   // the grid covers the pieces of work with a visible pixel (nearest: their 256 x 4 displayed pixels)
    max_tiles = frame_tiles.max_x; max_blocks = frame_tiles.max_y;
    max_dw = frame_tiles.max_x * 256; max_dh = frame_tiles.max_y * 4;
  }
  if (int rc = blocks_reserve(st, bytes)) return rc;
  if (int rc = blocks_upload(st, host, s)) return rc;
  const int wide = caps[0].wide;
  int rc = launch_z_chunks(0, n_clip, "clip kernel launch", &g_oriented_launches, [&](size_t first, size_t n) {
    const OrientedParams* dev = (const OrientedParams*)st.dev + first;
    const LaunchShape g = box_grid(clip_tiles, clip_oh, n);
    if (dispatch_pix_dtype(wide, dtype, [&](auto pix, auto dt) {
          hipLaunchKernelGGL((k_clip_box<typename decltype(pix)::type, decltype(dt)::value>), g.grid, g.block, 0, s, dev);
        })) return 0;
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "clip output: unknown dtype %d", dtype);
  });
  if (rc) return rc;
  g_clip_box_entries += (uint64_t)n_clip;
  // box: the most column tiles and row blocks an entry has; nearest: the largest DISPLAYED size among the entries
  rc = launch_z_chunks(n_clip, caps.size(), "oriented kernel launch", &g_oriented_launches, [&](size_t first, size_t n) {
    if (dispatch_pix_dtype(wide, dtype, [&](auto pix, auto dt) {
          typedef typename decltype(pix)::type Pix;
          constexpr int DT = decltype(dt)::value;
          if (blocked) launch_box_or_nearest(filter, k_patch_box<Pix, DT>, k_patch_nearest<Pix, DT>, max_tiles, max_blocks, max_dw, max_dh, n, s, (const PatchParams*)st.dev + first);
          else if (framed) launch_box_or_nearest(filter, k_frame_box<Pix, DT>, k_frame_nearest<Pix, DT>, max_tiles, max_blocks, max_dw, max_dh, n, s, (const FrameParams*)st.dev + first);
          else launch_box_or_nearest(filter, k_oriented_box<Pix, DT>, k_oriented_nearest<Pix, DT>, max_tiles, max_blocks, max_dw, max_dh, n, s, (const OrientedParams*)st.dev + first);
        })) return 0;
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "oriented output: unknown dtype %d", dtype);
  });
  if (rc) return rc;
  g_oriented_entries += (uint64_t)caps.size(); g_oriented_quarter += quarter;
  frame_tiles.commit(caps[0].framed == 2);
  return 0;
}

// HIPDEC_SCALE_BILINEAR / _BICUBIC: the recorded blocks with their coefficient tables as ONE launch of k_resample.  The tables of a call are deduplicated by
// (input samples, output samples) - the filter is the call's - and travel behind the parameter blocks in the same buffer, so ONE asynchronous copy brings
// both to the device and the staging memory is kept as the other launches keep theirs (st.host, st.prev).
int resample_launch(std::vector<CapturedTensor>& caps, ColorBatchState& st, int filter, int dtype, hipStream_t s)
{
  std::map<std::pair<int, int>, uint64_t> where;   // axis -> the table's first int
  uint64_t ints = 0;
  auto want = [&](int n_in, int n_out) {
    if (where.emplace(std::make_pair(n_in, n_out), ints).second) ints += resample_table_ints(n_in, n_out, filter);
  };
  int max_tiles = 0, max_bands = 0;
  uint64_t quarter = 0;
  for (const auto& c : caps) {
    if (c.wide != caps[0].wide) return set_error(HIPDEC_ERR_UNSUPPORTED, "resampled output: the entries mix 8-bit and wider sources");
    if (c.resample != filter) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "resampled output: the entries were recorded for filter %d, the launch is for %d", c.resample, filter);
    want(c.p.rw, c.p.ow); want(c.p.rh, c.p.oh);
    if (ints > kResampleTableBytes / 4)
      return set_error(HIPDEC_ERR_LIMIT, "resampled output: the coefficient tables of this call exceed %llu bytes", (unsigned long long)kResampleTableBytes);
    const int tile = c.p.tile < kResTC ? (c.p.tile > 0 ? c.p.tile : 1) : kResTC;   // (as the kernel reads it)
    const int tiles = (c.p.ow + tile - 1) / tile, bands = (c.p.oh + kResTR - 1) / kResTR;
    max_tiles = tiles > max_tiles ? tiles : max_tiles; max_bands = bands > max_bands ? bands : max_bands;
    quarter += (uint64_t)(c.code & 1);
  }
  const bool blocked = caps[0].patch > 0;   // (as in oriented_launch): PatchResampleParams blocks for k_patch_resample
  const bool framed = !blocked && caps[0].framed;   // ... FrameResampleParams blocks for k_frame_resample
  const size_t block_bytes = blocked ? sizeof(PatchResampleParams) : (framed ? sizeof(FrameResampleParams) : sizeof(ResampleParams));
  FrameTileCount frame_tiles;
  const size_t params_bytes = (caps.size() * block_bytes + 15) & ~(size_t)15;
  const size_t bytes = params_bytes + (size_t)ints * sizeof(int32_t);
  std::vector<uint8_t> host(bytes);
  for (const auto& w : where) resample_table_fill(w.first.first, w.first.second, filter, (int32_t*)(host.data() + params_bytes) + w.second);
  if (int rc = blocks_reserve(st, bytes)) return rc;   // (the blocks below hold addresses inside it)
  const int32_t* tables_dev = (const int32_t*)((const uint8_t*)st.dev + params_bytes);
  for (size_t i = 0; i < caps.size(); i++) {
    const CapturedTensor& c = caps[i];
    ResampleParams rp;
    memset(&rp, 0, sizeof(rp));
    rp.o.t = c.p; rp.o.code = (uint16_t)c.code; rp.o.rb = (uint16_t)kResTR; rp.o.pitch = c.pitch; rp.o.plane_rows = c.plane_rows;
    rp.xt = tables_dev + where[std::make_pair(c.p.rw, c.p.ow)]; rp.xstride = resample_axis_of(c.p.rw, c.p.ow, filter).stride;
    rp.yt = tables_dev + where[std::make_pair(c.p.rh, c.p.oh)]; rp.ystride = resample_axis_of(c.p.rh, c.p.oh, filter).stride;
    memcpy(host.data() + i * block_bytes, &rp, sizeof(rp));
    if (blocked) {
      const PatchInfo b = patch_info_of(c);
      memcpy(host.data() + i * block_bytes + offsetof(PatchResampleParams, b), &b, sizeof(b));
    }
    if (framed) {
      hipdec::FrameWindow f = frame_window_of(c);
      frame_tiles.add(&f, c.p.ow, c.p.tile < kResTC ? (c.p.tile > 0 ? c.p.tile : 1) : kResTC, f.px0, f.px1, c.p.oh, kResTR, f.py0, f.py1);
      memcpy(host.data() + i * block_bytes + offsetof(FrameResampleParams, b), &f, sizeof(f));
    }
  }
  if (int rc = blocks_upload(st, host, s)) return rc;
  const int wide = caps[0].wide;
  if (framed) { max_tiles = frame_tiles.max_x; max_bands = frame_tiles.max_y; }   // the grid covers the tiles and bands with a visible pixel
  const int rc = launch_z_chunks(0, caps.size(), "resample kernel launch", caps[0].oriented ? &g_oriented_launches : nullptr, [&](size_t first, size_t n) {
    const LaunchShape g = box_grid(max_tiles, max_bands, n);
    if (dispatch_pix_dtype(wide, dtype, [&](auto pix, auto dt) {
          typedef typename decltype(pix)::type Pix;
          constexpr int DT = decltype(dt)::value;
          if (blocked) hipLaunchKernelGGL((k_patch_resample<Pix, DT>), g.grid, g.block, 0, s, (const PatchResampleParams*)st.dev + first);
          else if (framed) hipLaunchKernelGGL((k_frame_resample<Pix, DT>), g.grid, g.block, 0, s, (const FrameResampleParams*)st.dev + first);
          else hipLaunchKernelGGL((k_resample<Pix, DT>), g.grid, g.block, 0, s, (const ResampleParams*)st.dev + first);
        })) return 0;
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "resampled output: unknown dtype %d", dtype);
  });
  if (rc) return rc;
  if (caps[0].oriented) { g_oriented_entries += (uint64_t)caps.size(); g_oriented_quarter += quarter; }
  frame_tiles.commit(caps[0].framed == 2);
  return 0;
}
}  // namespace

// the tensor blocks recorded on this thread since color_tensor_begin() as ONE launch (a grid's z extent is 65535: more entries take as few launches as that allows)
int color_tensor_launch(ColorBatchState& st, int filter, int dtype, hipStream_t s)
{
  std::vector<CapturedTensor> caps;
  caps.swap(t_captured_tensor);
  if (caps.empty()) return 0;
  if (caps[0].resample) return resample_launch(caps, st, filter, dtype, s);   // (the filter is the call's: all entries, or none)
  if (caps[0].oriented) return oriented_launch(caps, st, filter, dtype, s);   // (a call's entries are all oriented, or none is)
  int max_tiles = 0;
  for (const auto& c : caps) {
    if (c.wide != caps[0].wide) return set_error(HIPDEC_ERR_UNSUPPORTED, "tensor output: the entries mix 8-bit and wider sources");
    const int tiles = (c.p.ow + c.p.tile - 1) / c.p.tile;
    max_tiles = tiles > max_tiles ? tiles : max_tiles;
  }
  if (int rc = blocks_of_captured(caps, st, s)) return rc;
  const int ow = caps[0].p.ow, oh = caps[0].p.oh, wide = caps[0].wide;
  return launch_z_chunks(0, caps.size(), "tensor kernel launch", nullptr, [&](size_t first, size_t n) {
    const TensorParams* dev = (const TensorParams*)st.dev + first;
    if (dispatch_pix_dtype(wide, dtype, [&](auto pix, auto dt) {
          typedef typename decltype(pix)::type Pix;
          constexpr int DT = decltype(dt)::value;
          launch_box_or_nearest(filter, k_tensor_box<Pix, DT>, k_tensor_nearest<Pix, DT>, max_tiles, oh, ow, oh, n, s, dev);
        })) return 0;
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor output: unknown dtype %d", dtype);
  });
}

// ---- placed tensor output: the margins (and masks) of all entries of a call as ONE launch of k_canvas_margin; the blocks are kept and re-uploaded only
// when they change, as the picture blocks are
std::atomic<uint64_t> g_placed_calls{0}, g_placed_entries{0}, g_placed_margin_launches{0};
void placed_note_call(uint64_t entries) { g_placed_calls++; g_placed_entries += entries; }
void framed_note_call(uint64_t entries) { g_framed_calls++; g_framed_entries += entries; }
uint64_t clip_box_entries() { return g_clip_box_entries.load(); }
void packed_note_call(uint64_t entries, bool patches) { g_packed_calls++; g_packed_entries += entries; if (patches) g_packed_patch_entries += entries; }

int canvas_margin_launch(ColorBatchState& st, const CanvasMargin* blocks, int n, int dtype, hipStream_t s)
{
  bool any = false;
  uint64_t max_elems = 0;
  for (int i = 0; i < n; i++) {
    if (!blocks[i].margin && !blocks[i].mask) continue;
    any = true;
    const uint64_t elems = 3ull * (uint64_t)blocks[i].W * (uint64_t)blocks[i].H;
    max_elems = elems > max_elems ? elems : max_elems;
  }
  if (!any) return 0;
  const size_t bytes = (size_t)n * sizeof(CanvasMargin);
  std::vector<uint8_t> host(bytes);
  memcpy(host.data(), blocks, bytes);
  if (int rc = blocks_reserve(st, bytes)) return rc;
  if (int rc = blocks_upload(st, host, s)) return rc;
  // a lane owns one 16-byte block at a time: an entry touches at most elements / (elements per block) + 2 of them (the kernel's loop strides over what the
  // grid leaves; a mask has fewer)
  const uint64_t per = dtype == TD_U8 ? 16 : (dtype == TD_F32 ? 4 : 8);
  const uint64_t gx = (max_elems / per + 2 + 255) / 256;
  return launch_z_chunks(0, (size_t)n, "margin kernel launch", &g_placed_margin_launches, [&](size_t first, size_t count) {
    const CanvasMargin* dev = (const CanvasMargin*)st.dev + first;
    dim3 block(256), grid((unsigned)(gx < 65536 ? gx : 65536), 1, (unsigned)count);
    if (dispatch_dtype(dtype, [&](auto dt) { hipLaunchKernelGGL((k_canvas_margin<decltype(dt)::value>), grid, block, 0, s, dev); })) return 0;
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "placed output: unknown dtype %d", dtype);
  });
}

// ---- composed tensor output: the fill and the masks of all canvases of a call as ONE launch of k_compose_cover; the cover tables travel behind the
// per-canvas blocks in the same upload (the blocks hold addresses inside it, as the resampling blocks do)
std::atomic<uint64_t> g_composed_calls{0}, g_composed_entries{0}, g_composed_pieces{0}, g_composed_hidden{0}, g_composed_cover_launches{0};
void composed_note_call(uint64_t entries, uint64_t pieces, uint64_t hidden)
{
  g_composed_calls++; g_composed_entries += entries; g_composed_pieces += pieces; g_composed_hidden += hidden;
}

int canvas_cover_launch(ColorBatchState& st, const CanvasCover* blocks, int n, const int32_t* words, size_t n_words, int dtype, hipStream_t s)
{
  bool any = false;
  uint64_t max_elems = 0;
  for (int i = 0; i < n; i++) {
    if (!blocks[i].m.margin && !blocks[i].m.mask) continue;
    any = true;
    const uint64_t elems = 3ull * (uint64_t)blocks[i].m.W * (uint64_t)blocks[i].m.H;
    max_elems = elems > max_elems ? elems : max_elems;
  }
  if (!any) return 0;
  const size_t blocks_bytes = ((size_t)n * sizeof(CanvasCover) + 15) & ~(size_t)15;
  const size_t bytes = blocks_bytes + n_words * sizeof(int32_t);
  std::vector<uint8_t> host(bytes);
  if (int rc = blocks_reserve(st, bytes)) return rc;   // (the blocks below hold addresses inside it)
  const int32_t* words_dev = (const int32_t*)((const uint8_t*)st.dev + blocks_bytes);
  for (int i = 0; i < n; i++) {
    CanvasCover c = blocks[i];
    c.table = (uint64_t)(uintptr_t)(words_dev + c.table);
    memcpy(host.data() + (size_t)i * sizeof(CanvasCover), &c, sizeof(c));
  }
  if (n_words) memcpy(host.data() + blocks_bytes, words, n_words * sizeof(int32_t));
  if (int rc = blocks_upload(st, host, s)) return rc;
  const uint64_t per = dtype == TD_U8 ? 16 : (dtype == TD_F32 ? 4 : 8);   // (as canvas_margin_launch: a lane owns one 16-byte block at a time)
  const uint64_t gx = (max_elems / per + 2 + 255) / 256;
  return launch_z_chunks(0, (size_t)n, "cover kernel launch", &g_composed_cover_launches, [&](size_t first, size_t count) {
    const CanvasCover* dev = (const CanvasCover*)st.dev + first;
    dim3 block(256), grid((unsigned)(gx < 65536 ? gx : 65536), 1, (unsigned)count);
    if (dispatch_dtype(dtype, [&](auto dt) { hipLaunchKernelGGL((k_compose_cover<decltype(dt)::value>), grid, block, 0, s, dev); })) return 0;
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "composed output: unknown dtype %d", dtype);
  });
}

// ---- warped tensor output: what the arguments alone decide, the per-entry table, ONE launch of k_warp_* for all entries of a call
std::atomic<uint64_t> g_warp_calls{0}, g_warp_entries{0};

// what the warp desc, the fill and the presence of the maps decide (the warped and the projected calls)
static int warp_check_call(const char* who, const hipdec_warp_desc* w, const void* maps, const hipdec_tensor_fill* fill, const hipdec_tensor_desc* d, int n)
{
  if (!w || (!maps && n > 0)) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
  if (w->src_width < 1 || w->src_height < 1 || w->src_width >= 32768 || w->src_height >= 32768)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: source size %d x %d (1 .. 32767 each way)", who, w->src_width, w->src_height);
  if (w->filter != HIPDEC_SCALE_NEAREST && w->filter != HIPDEC_SCALE_BILINEAR && w->filter != HIPDEC_SCALE_BICUBIC)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: warp filter %d (nearest 0, bilinear 16, bicubic 17)", who, w->filter);
  if (w->reserved) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: warp.reserved is %d, not 0", who, w->reserved);
  if (fill) {
    if (fill->domain != HIPDEC_FILL_COMPONENT && fill->domain != HIPDEC_FILL_ELEMENT) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: unknown fill domain %d", who, fill->domain);
    if (fill->reserved) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: fill.reserved is %d, not 0", who, fill->reserved);
    for (int c = 0; c < 3; c++) {
      const float v = fill->value[c];
      if (!std::isfinite(v)) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: fill of channel %d is not finite", who, c);
      const bool byte = v == std::floor(v) && v >= 0.0f && v <= 255.0f;
      if (fill->domain == HIPDEC_FILL_COMPONENT && !byte)
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: component fill %g of channel %d is not an integer a pixel can have", who, (double)v, c);
      if (fill->domain == HIPDEC_FILL_ELEMENT && d->dtype == HIPDEC_TENSOR_U8 && !byte)
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: element fill %g of channel %d is not an integer in 0 .. 255", who, (double)v, c);
    }
  }
  return 0;
}

static int warp_check_tiles(const char* who, const hipdec_tensor_desc* d, int n)
{
  const uint64_t tiles = (uint64_t)((d->width + kWarpTC - 1) / kWarpTC) * (uint64_t)((d->height + kWarpTR - 1) / kWarpTR);
  if (tiles * (uint64_t)(n > 0 ? n : 1) > 0x7fffffffull) return set_error(HIPDEC_ERR_LIMIT, "%s: %d entries of %d x %d are more than 2^31 - 1 tiles", who, n, d->width, d->height);
  return 0;
}

int warp_check(const char* who, const hipdec_warp_desc* w, const hipdec_tensor_map* maps, const hipdec_tensor_fill* fill, const hipdec_tensor_desc* d, int n)
{
  if (int rc = warp_check_call(who, w, maps, fill, d, n)) return rc;
  for (int e = 0; e < n; e++) {
    int which = 0;
    switch (warp_map_check(maps[e].m, d->width, d->height, &which)) {
      case 0: break;
      case 1: return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: map coefficient %d is not finite", who, e, which);
      case 2: return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: map coefficient %d is %g (magnitude 32000 or more)", who, e, which, maps[e].m[which]);
      default:
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: corner (%d, %d) of the output maps to a coordinate of magnitude 32000 or more", who, e,
                         (which & 1) ? d->width : 0, (which & 2) ? d->height : 0);
    }
  }
  return warp_check_tiles(who, d, n);
}

// the state's device memory is about to be rewritten or handed back: not before the last launch that read it has passed
static int warp_state_order(WarpState& st, hipStream_t s, bool release)
{
  if (!st.done) return 0;
  if (release) HIPDEC_CHECK_HIP(hipEventSynchronize(st.done));
  else if (st.last != s) HIPDEC_CHECK_HIP(hipStreamWaitEvent(s, st.done, 0));
  return 0;
}

int warp_scratch(WarpState& st, size_t bytes, hipStream_t s, void** out)
{
  if (st.scratch_bytes < bytes) {
    if (int rc = warp_state_order(st, s, true)) return rc;
    if (st.scratch) arena_release(st.scratch, st.scratch_bytes);
    st.scratch = nullptr; st.scratch_bytes = 0;
    HIPDEC_CHECK_HIP(arena_acquire(&st.scratch, bytes, &st.scratch_bytes));
  } else if (int rc = warp_state_order(st, s, false)) {
    return rc;
  }
  *out = st.scratch;
  return 0;
}

void warp_state_free(WarpState& st)
{
  if (st.done) { (void)hipEventSynchronize(st.done); (void)hipEventDestroy(st.done); st.done = nullptr; }
  if (st.scratch) arena_release(st.scratch, st.scratch_bytes);
  st.scratch = nullptr; st.scratch_bytes = 0;
  color_batch_state_free(st.table);
}

int warp_launch(WarpState& st, const void* src_dev, const hipdec_warp_desc* w, const hipdec_tensor_map* maps, const hipdec_tensor_fill* fill,
                const hipdec_tensor_desc* d, int n, void* out_dev, hipStream_t s)
{
  if (n <= 0) return 0;
  const int sw = w->src_width, sh = w->src_height, ow = d->width, oh = d->height;
  const size_t src_entry = (size_t)sw * (size_t)sh * 3, out_entry = (size_t)ow * (size_t)oh * 3 * (d->dtype == TD_U8 ? 1 : (d->dtype == TD_F32 ? 4 : 2));
  // the table: n records, then the index tables (ow + oh values) of the entries on Pillow's scale path
  size_t n_tables = 0;
  if (w->filter == HIPDEC_SCALE_NEAREST) for (int e = 0; e < n; e++) n_tables += warp_scale_only(maps[e].m) ? 1 : 0;
  const size_t table_ints = (size_t)ow + (size_t)oh, bytes = (size_t)n * sizeof(WarpEntry) + n_tables * table_ints * sizeof(int32_t);
  std::vector<uint8_t> host(bytes);
  if (int rc = warp_state_order(st, s, st.table.dev_bytes < bytes)) return rc;
  if (int rc = blocks_reserve(st.table, bytes)) return rc;   // (the entries below hold addresses inside it)
  const uint8_t* dev_tables = (const uint8_t*)st.table.dev + (size_t)n * sizeof(WarpEntry);
  int32_t* host_tables = (int32_t*)(host.data() + (size_t)n * sizeof(WarpEntry));
  size_t t = 0;
  for (int e = 0; e < n; e++) {
    WarpEntry E;
    memset(&E, 0, sizeof(E));
    E.src = (const uint8_t*)src_dev + (size_t)e * src_entry;
    E.o0 = (uint8_t*)out_dev + (size_t)e * out_entry;
    const double* a = maps[e].m;
    for (int i = 0; i < 6; i++) E.m[i] = a[i];
    if (w->filter != HIPDEC_SCALE_NEAREST) {
      E.path = WARP_PATH_DOUBLE;
    } else if (warp_scale_only(a)) {
      E.path = WARP_PATH_TABLE;
      warp_scale_table(a[2], a[0], ow, host_tables + t * table_ints);
      warp_scale_table(a[5], a[4], oh, host_tables + t * table_ints + (size_t)ow);
      E.xt = (const int32_t*)dev_tables + t * table_ints;
      E.yt = E.xt + ow;
      t++;
    } else {
      E.path = WARP_PATH_FIXED;
      warp_fixed_values(a, E.A);
    }
    E.domain = fill ? fill->domain : HIPDEC_FILL_COMPONENT;
    for (int c = 0; c < 3; c++) E.value[c] = fill ? fill->value[c] : 0.0f;
    memcpy(host.data() + (size_t)e * sizeof(WarpEntry), &E, sizeof(E));
  }
  if (int rc = blocks_upload(st.table, host, s)) return rc;
  WarpCall c;
  memset(&c, 0, sizeof(c));
  c.sw = sw; c.sh = sh; c.ow = ow; c.oh = oh; c.nhwc = d->layout == HIPDEC_TENSOR_NHWC;
  c.tiles_x = (uint32_t)((ow + kWarpTC - 1) / kWarpTC);
  c.tiles = c.tiles_x * (uint32_t)((oh + kWarpTR - 1) / kWarpTR);
  for (int k = 0; k < 3; k++) { c.scale[k] = d->scale[k]; c.bias[k] = d->bias[k]; }
  const WarpEntry* dev = (const WarpEntry*)st.table.dev;
  dim3 block(256), grid((unsigned)((uint64_t)c.tiles * (uint64_t)n));   // (warp_check: below 2^31)
  if (!dispatch_dtype(d->dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (w->filter == HIPDEC_SCALE_NEAREST) hipLaunchKernelGGL((k_warp_nearest<DT>), grid, block, 0, s, dev, c);
        else if (w->filter == HIPDEC_SCALE_BILINEAR) hipLaunchKernelGGL((k_warp_bilinear<DT>), grid, block, 0, s, dev, c);
        else hipLaunchKernelGGL((k_warp_bicubic<DT>), grid, block, 0, s, dev, c);
      })) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_warp: unknown dtype %d", d->dtype);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(HIPDEC_ERR_DEVICE, "warp kernel launch: %s", hipGetErrorString(e));
  if (!st.done) HIPDEC_CHECK_HIP(hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
  HIPDEC_CHECK_HIP(hipEventRecord(st.done, s));
  st.last = s;
  g_warp_calls++; g_warp_entries += (uint64_t)n;
  return 0;
}

// ---- projective tensor output: warp_check's refusals and those of the maps (project_host.h), the per-entry table, ONE launch of k_project_* per call
std::atomic<uint64_t> g_project_calls{0}, g_project_entries{0};
static_assert((int)HIPDEC_PROJECT_PERSPECTIVE == (int)PROJECT_PERSPECTIVE && (int)HIPDEC_PROJECT_QUAD == (int)PROJECT_QUAD, "project_host.h restates the kinds");

int project_check(const char* who, const hipdec_warp_desc* w, const hipdec_tensor_projection* maps, const hipdec_tensor_fill* fill, const hipdec_tensor_desc* d, int n)
{
  if (int rc = warp_check_call(who, w, maps, fill, d, n)) return rc;
  for (int e = 0; e < n; e++) {
    const hipdec_tensor_projection& m = maps[e];
    if (m.kind != HIPDEC_PROJECT_PERSPECTIVE && m.kind != HIPDEC_PROJECT_QUAD)
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: map kind %d (perspective 0, quad 1)", who, e, m.kind);
    if (m.reserved) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: map.reserved is %d, not 0", who, e, m.reserved);
    int which = 0;
    switch (project_map_check(m.a, m.kind, d->width, d->height, &which)) {
      case 0: break;
      case 1: return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: map coefficient %d is not finite", who, e, which);
      case 2: return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: map coefficient %d is %g (magnitude 32000 or more)", who, e, which, m.a[which]);
      case 3:
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: corner (%d, %d) of the output maps to a coordinate of magnitude 32000 or more", who, e,
                         (which & 1) ? d->width : 0, (which & 2) ? d->height : 0);
      default:
        return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: the denominator at corner (%d, %d) of the output is below 2^-20", who, e,
                         (which & 1) ? d->width : 0, (which & 2) ? d->height : 0);
    }
  }
  return warp_check_tiles(who, d, n);
}

int project_launch(WarpState& st, const void* src_dev, const hipdec_warp_desc* w, const hipdec_tensor_projection* maps, const hipdec_tensor_fill* fill,
                   const hipdec_tensor_desc* d, int n, void* out_dev, hipStream_t s)
{
  if (n <= 0) return 0;
  const int sw = w->src_width, sh = w->src_height, ow = d->width, oh = d->height;
  const size_t src_entry = (size_t)sw * (size_t)sh * 3, out_entry = (size_t)ow * (size_t)oh * 3 * (d->dtype == TD_U8 ? 1 : (d->dtype == TD_F32 ? 4 : 2));
  const size_t bytes = (size_t)n * sizeof(ProjectEntry);
  std::vector<uint8_t> host(bytes);
  if (int rc = warp_state_order(st, s, st.table.dev_bytes < bytes)) return rc;
  if (int rc = blocks_reserve(st.table, bytes)) return rc;
  for (int e = 0; e < n; e++) {
    ProjectEntry E;
    memset(&E, 0, sizeof(E));
    E.src = (const uint8_t*)src_dev + (size_t)e * src_entry;
    E.o0 = (uint8_t*)out_dev + (size_t)e * out_entry;
    for (int i = 0; i < 8; i++) E.a[i] = maps[e].a[i];
    E.kind = maps[e].kind;
    E.domain = fill ? fill->domain : HIPDEC_FILL_COMPONENT;
    for (int c = 0; c < 3; c++) E.value[c] = fill ? fill->value[c] : 0.0f;
    memcpy(host.data() + (size_t)e * sizeof(ProjectEntry), &E, sizeof(E));
  }
  if (int rc = blocks_upload(st.table, host, s)) return rc;
  WarpCall c;
  memset(&c, 0, sizeof(c));
  c.sw = sw; c.sh = sh; c.ow = ow; c.oh = oh; c.nhwc = d->layout == HIPDEC_TENSOR_NHWC;
  c.tiles_x = (uint32_t)((ow + kWarpTC - 1) / kWarpTC);
  c.tiles = c.tiles_x * (uint32_t)((oh + kWarpTR - 1) / kWarpTR);
  for (int k = 0; k < 3; k++) { c.scale[k] = d->scale[k]; c.bias[k] = d->bias[k]; }
  const ProjectEntry* dev = (const ProjectEntry*)st.table.dev;
  dim3 block(256), grid((unsigned)((uint64_t)c.tiles * (uint64_t)n));   // (project_check: below 2^31)
  if (!dispatch_dtype(d->dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (w->filter == HIPDEC_SCALE_NEAREST) hipLaunchKernelGGL((k_project_nearest<DT>), grid, block, 0, s, dev, c);
        else if (w->filter == HIPDEC_SCALE_BILINEAR) hipLaunchKernelGGL((k_project_bilinear<DT>), grid, block, 0, s, dev, c);
        else hipLaunchKernelGGL((k_project_bicubic<DT>), grid, block, 0, s, dev, c);
      })) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_project: unknown dtype %d", d->dtype);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(HIPDEC_ERR_DEVICE, "project kernel launch: %s", hipGetErrorString(e));
  if (!st.done) HIPDEC_CHECK_HIP(hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
  HIPDEC_CHECK_HIP(hipEventRecord(st.done, s));
  st.last = s;
  g_project_calls++; g_project_entries += (uint64_t)n;
  return 0;
}

// ---- photometric tensor output: what the arguments alone decide, the per-step tables, at most one k_photo_hist and one k_photo_apply launch per chain step
#define HIPDEC_PHOTO_SAME(NAME) ((int)HIPDEC_PHOTO_##NAME == (int)PHOTO_##NAME)
static_assert(HIPDEC_PHOTO_SAME(BRIGHTNESS) && HIPDEC_PHOTO_SAME(COLOR) && HIPDEC_PHOTO_SAME(CONTRAST) && HIPDEC_PHOTO_SAME(SHARPNESS) &&
              HIPDEC_PHOTO_SAME(POSTERIZE) && HIPDEC_PHOTO_SAME(SOLARIZE) && HIPDEC_PHOTO_SAME(INVERT) && HIPDEC_PHOTO_SAME(AUTOCONTRAST) &&
              HIPDEC_PHOTO_SAME(EQUALIZE), "photo_lut.h restates hipdec_photo_opcode");
#undef HIPDEC_PHOTO_SAME
static_assert((int)HIPDEC_AUGMENT_HUE == (int)AUGMENT_HUE && (int)HIPDEC_AUGMENT_GAUSSIAN_BLUR == (int)AUGMENT_GAUSSIAN_BLUR &&
              HIPDEC_AUGMENT_BLUR_MAX_RADIUS == kAugmentBlurMaxRadius, "augment_lut.h restates the augment opcodes and the cap");
std::atomic<uint64_t> g_photo_calls{0}, g_photo_entries{0}, g_photo_launches{0};
std::atomic<uint64_t> g_augment_calls{0}, g_augment_entries{0}, g_augment_launches{0};
std::atomic<uint64_t> g_recipe_calls{0}, g_recipe_entries{0}, g_recipe_launches{0}, g_recipe_affine_steps{0};

// what an affine step of a recipe chain alone decides: its index, and of the record it names what warp_check refuses of a map for an output of the
// sample's size, the filter and the fill
static int recipe_affine_check(const char* who, const ChainView& chains, const hipdec_tensor_desc* d, int e, int k, const hipdec_photo_op& o)
{
  if (o.reserved) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (AFFINE): reserved is %d, not 0", who, e, k, o.reserved);
  if (!std::isfinite(o.value)) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (AFFINE): the value is not finite", who, e, k);
  if (o.value != std::floor(o.value) || o.value < 0.0 || o.value >= (double)chains.n_affines)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (AFFINE): the value %g is not an index into the %d affine records", who, e, k, o.value,
                     chains.n_affines);
  if (!chains.affines) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (AFFINE): affines is NULL", who, e, k);
  const int i = (int)o.value;
  const hipdec_recipe_affine& a = chains.affines[i];
  int which = 0;
  switch (warp_map_check(a.map.m, d->width, d->height, &which)) {
    case 0: break;
    case 1: return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (AFFINE): map coefficient %d of record %d is not finite", who, e, k, which, i);
    case 2:
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (AFFINE): map coefficient %d of record %d is %g (magnitude 32000 or more)", who, e, k,
                       which, i, a.map.m[which]);
    default:
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (AFFINE): record %d maps corner (%d, %d) of the output to a coordinate of magnitude 32000 or more",
                       who, e, k, i, (which & 1) ? d->width : 0, (which & 2) ? d->height : 0);
  }
  if (a.filter != HIPDEC_SCALE_NEAREST && a.filter != HIPDEC_SCALE_BILINEAR && a.filter != HIPDEC_SCALE_BICUBIC)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (AFFINE): warp filter %d of record %d (nearest 0, bilinear 16, bicubic 17)", who, e, k,
                     a.filter, i);
  for (int c = 0; c < 3; c++)
    if (a.fill[c] < 0 || a.fill[c] > 255)
      return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (AFFINE): fill %d of channel %d of record %d is not 0 .. 255", who, e, k, a.fill[c], c, i);
  return 0;
}

// the photo stage's checks, the augment stage's and the recipe stage's: the chain length and the operations a view admits are what differs
int chain_check(const char* who, const hipdec_photo_desc* p, const ChainView& chains, const hipdec_tensor_desc* d, int n)
{
  static const char* const names[] = {"none", "BRIGHTNESS", "COLOR", "CONTRAST", "SHARPNESS", "POSTERIZE", "SOLARIZE", "INVERT", "AUTOCONTRAST", "EQUALIZE"};
  if (!p || (!chains.base && n > 0)) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
  if (chains.recipe && chains.n_affines < 0) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: n_affines is %d", who, chains.n_affines);
  if (p->src_width < 1 || p->src_height < 1 || p->src_width >= 32768 || p->src_height >= 32768)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: source size %d x %d (1 .. 32767 each way)", who, p->src_width, p->src_height);
  if (p->reserved[0] || p->reserved[1]) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: photo.reserved is not 0", who);
  if (d->width != p->src_width || d->height != p->src_height)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: the tensor's size %d x %d is not the source size %d x %d (the stage does not resize)", who, d->width, d->height,
                     p->src_width, p->src_height);
  for (int e = 0; e < n; e++) {
    const int n_ops = chains.n_ops(e);
    if (n_ops < 0 || n_ops > chains.max_ops) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: n_ops is %d (0 .. %d)", who, e, n_ops, chains.max_ops);
    if (chains.reserved(e)) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: chain.reserved is %d, not 0", who, e, chains.reserved(e));
    for (int k = 0; k < n_ops; k++) {
      const hipdec_photo_op& o = chains.op(e, k);
      if (chains.recipe && o.op == HIPDEC_RECIPE_AFFINE) {
        if (int rc = recipe_affine_check(who, chains, d, e, k, o)) return rc;
        continue;
      }
      const char* name = o.op >= PHOTO_BRIGHTNESS && o.op <= PHOTO_EQUALIZE ? names[o.op]
                         : (chains.augment && o.op == AUGMENT_HUE ? "HUE" : (chains.augment && o.op == AUGMENT_GAUSSIAN_BLUR ? "GAUSSIAN_BLUR" : "unknown"));
      switch (chains.augment ? augment_op_check(o.op, o.reserved, o.value) : photo_op_check(o.op, o.reserved, o.value)) {
        case 0: break;
        case 1: return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d: unknown op %d", who, e, k, o.op);
        case 2: return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (%s): reserved is %d, not 0", who, e, k, name, o.reserved);
        case 3: return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (%s): the value is not finite", who, e, k, name);
        case 4: return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (%s): the value %g has a magnitude above 65536", who, e, k, name, o.value);
        case 6: return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (%s): the shift %g is not an integer 0 .. 255", who, e, k, name, o.value);
        case 7: return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (%s): the radius %g is not 0 .. %g", who, e, k, name, o.value, kAugmentBlurMaxRadius);
        default: return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: entry %d: operation %d (%s): %g bits (an integer 0 .. 8)", who, e, k, name, o.value);
      }
    }
  }
  const uint64_t tiles = (uint64_t)((d->width + kWarpTC - 1) / kWarpTC) * (uint64_t)((d->height + kWarpTR - 1) / kWarpTR);
  if (tiles * (uint64_t)(n > 0 ? n : 1) > 0x7fffffffull)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: %d entries of %d x %d are more than 2^31 - 1 tiles", who, n, d->width, d->height);
  return 0;
}

int photo_scratch(PhotoState& st, size_t bytes, hipStream_t s, void** out) { return warp_scratch(st.base, bytes, s, out); }

void photo_state_free(PhotoState& st)
{
  warp_state_free(st.base);   // (waits for the last launch)
  if (st.work) arena_release(st.work, st.work_bytes);
  st.work = nullptr; st.work_bytes = 0;
}

namespace {
enum ChainKind { KIND_APPLY = 0, KIND_HIST = 1, KIND_HUE = 2, KIND_BLUR = 3,
                 KIND_AFFINE_NEAREST = 4, KIND_AFFINE_BILINEAR = 5, KIND_AFFINE_BICUBIC = 6, KIND_COUNT = 7 };   // a step's records, in this order
inline int chain_kind(int op) { return op == AUGMENT_HUE ? KIND_HUE : (op == AUGMENT_GAUSSIAN_BLUR ? KIND_BLUR : KIND_APPLY); }
// the table is counted in units of a PhotoEntry: an affine record (a WarpEntry) takes two
static_assert(sizeof(WarpEntry) == 2 * sizeof(PhotoEntry), "an affine record is two units of a step's table");
inline size_t kind_units(int kind) { return kind >= KIND_AFFINE_NEAREST ? 2 : 1; }
// the affine record of step t of entry e, or NULL (a checked chain: the index is in range)
inline const hipdec_recipe_affine* step_affine(const ChainView& chains, int e, int t)
{
  if (!chains.recipe || !chains.n_ops(e) || chains.op(e, t).op != HIPDEC_RECIPE_AFFINE) return nullptr;
  return chains.affines + (int)chains.op(e, t).value;
}
inline int affine_kind(const hipdec_recipe_affine* a)
{
  return a->filter == HIPDEC_SCALE_NEAREST ? KIND_AFFINE_NEAREST : (a->filter == HIPDEC_SCALE_BILINEAR ? KIND_AFFINE_BILINEAR : KIND_AFFINE_BICUBIC);
}
inline const char* chain_stage_name(const ChainView& chains) { return chains.recipe ? "tensor_recipe" : (chains.augment ? "tensor_augment" : "tensor_photo"); }
}

int chain_launch(PhotoState& st, const void* src_dev, const hipdec_photo_desc* p, const ChainView& chains, const hipdec_tensor_desc* d, int n, void* out_dev,
                 hipStream_t s)
{
  if (n <= 0) return 0;
  const int w = p->src_width, h = p->src_height;
  const size_t sample = (size_t)w * (size_t)h * 3, out_entry = sample * (d->dtype == TD_U8 ? 1 : (d->dtype == TD_F32 ? 4 : 2));
  // Chains are aligned at their first step: entry e takes part in steps 0 .. max(n_ops, 1) - 1, and its last step writes the tensor (an empty chain is
  // one identity step).  Step t of the call is the launches of all entries that have a step t: per kind - apply, histogram, hue, blur - one launch over
  // the compacted records of the entries whose operation at t is of that kind (a histogram record goes with the apply record of the same entry).
  int steps = 1;
  for (int e = 0; e < n; e++) steps = std::max(steps, chains.n_ops(e));
  // (the recipe surface: an affine step is three more kinds, one per warp filter, with records of their own behind the step's others)
  std::vector<std::array<int, KIND_COUNT>> count((size_t)steps, std::array<int, KIND_COUNT>{});
  std::vector<int> blur_r((size_t)steps, 0);   // the step's largest box radius
  size_t n_tables = 0;                         // affine steps on Pillow's NEAREST scale path: w + h indices each, behind all records
  uint64_t affine_steps = 0;
  for (int e = 0; e < n; e++)
    for (int t = 0; t < std::max(chains.n_ops(e), 1); t++) {
      if (const hipdec_recipe_affine* a = step_affine(chains, e, t)) {
        count[(size_t)t][affine_kind(a)]++;
        affine_steps++;
        if (a->filter == HIPDEC_SCALE_NEAREST && warp_scale_only(a->map.m)) n_tables++;
        continue;
      }
      const int op = chains.n_ops(e) ? chains.op(e, t).op : PHOTO_NONE;
      count[(size_t)t][chain_kind(op)]++;
      if (photo_needs_statistics(op)) count[(size_t)t][KIND_HIST]++;
    }
  size_t records = 0;   // in units of a PhotoEntry
  int max_hist = 0;
  for (int t = 0; t < steps; t++) {
    for (int k = 0; k < KIND_COUNT; k++) records += (size_t)count[(size_t)t][k] * kind_units(k);
    max_hist = std::max(max_hist, count[(size_t)t][KIND_HIST]);
  }
  const size_t table_ints = (size_t)w + (size_t)h;
  // the work memory: up to two ping-pong buffers of n samples, then the histograms of the step with the most of them
  const int n_pp = std::min(steps - 1, 2);
  const size_t pp_bytes = ((size_t)n * sample + 255) & ~(size_t)255, hist_bytes = (size_t)max_hist * 4 * 256 * sizeof(uint32_t);
  static_assert(sizeof(PhotoEntry) == sizeof(AugmentEntry), "a step's records share one table");
  const size_t work_bytes = (size_t)n_pp * pp_bytes + hist_bytes, bytes = records * sizeof(PhotoEntry) + n_tables * table_ints * sizeof(int32_t);
  const bool grow_work = st.work_bytes < work_bytes;
  if (int rc = warp_state_order(st.base, s, grow_work || st.base.table.dev_bytes < bytes)) return rc;
  if (grow_work) {
    if (st.work) arena_release(st.work, st.work_bytes);
    st.work = nullptr; st.work_bytes = 0;
    HIPDEC_CHECK_HIP(arena_acquire(&st.work, work_bytes, &st.work_bytes));
  }
  if (int rc = blocks_reserve(st.base.table, bytes)) return rc;
  uint8_t* pp[2] = {(uint8_t*)st.work, (uint8_t*)st.work + pp_bytes};
  uint32_t* hist = (uint32_t*)((uint8_t*)st.work + (size_t)n_pp * pp_bytes);
  std::vector<uint8_t> host(bytes);
  std::vector<size_t> first((size_t)steps);   // the step's first record: its apply records, then its histogram, hue, blur and affine records
  int32_t* host_tables = (int32_t*)(host.data() + records * sizeof(PhotoEntry));
  const int32_t* dev_tables = (const int32_t*)((const uint8_t*)st.base.table.dev + records * sizeof(PhotoEntry));
  size_t at = 0, tables_at = 0;
  for (int t = 0; t < steps; t++) {
    first[(size_t)t] = at;
    const std::array<int, KIND_COUNT>& cnt = count[(size_t)t];
    PhotoEntry* apply = (PhotoEntry*)host.data() + at;
    PhotoEntry* stat = apply + cnt[KIND_APPLY];
    AugmentEntry* hue = (AugmentEntry*)(stat + cnt[KIND_HIST]);
    AugmentEntry* blur = hue + cnt[KIND_HUE];
    WarpEntry* affine[3];   // by kind: nearest, bilinear, bicubic
    affine[0] = (WarpEntry*)(blur + cnt[KIND_BLUR]);
    affine[1] = affine[0] + cnt[KIND_AFFINE_NEAREST];
    affine[2] = affine[1] + cnt[KIND_AFFINE_BILINEAR];
    int ia = 0, ih = 0, iu = 0, ib = 0, iw[3] = {0, 0, 0};
    for (int e = 0; e < n; e++) {
      const int len = std::max(chains.n_ops(e), 1);
      if (t >= len) continue;
      const uint8_t* src = t == 0 ? (const uint8_t*)src_dev + (size_t)e * sample : pp[(t - 1) & 1] + (size_t)e * sample;
      const int last = t == len - 1;
      uint8_t* dst = last ? (uint8_t*)out_dev + (size_t)e * out_entry : pp[t & 1] + (size_t)e * sample;
      if (const hipdec_recipe_affine* a = step_affine(chains, e, t)) {   // warp_launch's record, the sample's size both ways, `last` in the reserved word
        WarpEntry E;
        memset(&E, 0, sizeof(E));
        E.src = src; E.o0 = dst;
        const double* m = a->map.m;
        for (int i = 0; i < 6; i++) E.m[i] = m[i];
        if (a->filter != HIPDEC_SCALE_NEAREST) {
          E.path = WARP_PATH_DOUBLE;
        } else if (warp_scale_only(m)) {
          E.path = WARP_PATH_TABLE;
          warp_scale_table(m[2], m[0], w, host_tables + tables_at * table_ints);
          warp_scale_table(m[5], m[4], h, host_tables + tables_at * table_ints + (size_t)w);
          E.xt = dev_tables + tables_at * table_ints;
          E.yt = E.xt + w;
          tables_at++;
        } else {
          E.path = WARP_PATH_FIXED;
          warp_fixed_values(m, E.A);
        }
        E.domain = HIPDEC_FILL_COMPONENT;
        for (int c = 0; c < 3; c++) E.value[c] = (float)a->fill[c];
        E.reserved = last;
        const int f = affine_kind(a) - KIND_AFFINE_NEAREST;
        affine[f][iw[f]++] = E;
        continue;
      }
      const int op = chains.n_ops(e) ? chains.op(e, t).op : PHOTO_NONE;
      const double value = chains.n_ops(e) ? chains.op(e, t).value : 0.0;
      if (chain_kind(op) == KIND_APPLY) {
        PhotoEntry E;
        memset(&E, 0, sizeof(E));
        E.src = src; E.dst = dst; E.last = last; E.op = op; E.value = value;
        if (photo_needs_statistics(E.op)) {
          E.hist = hist + (size_t)ih * 4 * 256;
          stat[ih++] = E;
        }
        apply[ia++] = E;
      } else {
        AugmentEntry E;
        memset(&E, 0, sizeof(E));
        E.src = src; E.dst = dst; E.last = last; E.op = op;
        if (op == AUGMENT_HUE) {
          E.shift = (int32_t)value;
          hue[iu++] = E;
        } else {
          augment_gaussian_box(value, &E.r, &E.ww, &E.fw);
          blur_r[(size_t)t] = std::max(blur_r[(size_t)t], (int)E.r);
          blur[ib++] = E;
        }
      }
    }
    for (int k = 0; k < KIND_COUNT; k++) at += (size_t)cnt[k] * kind_units(k);
  }
  if (int rc = blocks_upload(st.base.table, host, s)) return rc;
  PhotoCall c;
  memset(&c, 0, sizeof(c));
  c.w = w; c.h = h; c.nhwc = d->layout == HIPDEC_TENSOR_NHWC;
  c.tiles_x = (uint32_t)((w + kWarpTC - 1) / kWarpTC);
  c.tiles = c.tiles_x * (uint32_t)((h + kWarpTR - 1) / kWarpTR);
  c.slices = (uint32_t)((h + kPhotoHistRows - 1) / kPhotoHistRows);
  for (int k = 0; k < 3; k++) { c.scale[k] = d->scale[k]; c.bias[k] = d->bias[k]; }
  BlurCall bc;
  memset(&bc, 0, sizeof(bc));
  bc.p = c;
  bc.tiles_x = (uint32_t)((w + kBlurTC - 1) / kBlurTC);
  bc.tiles = bc.tiles_x * (uint32_t)((h + kBlurTR - 1) / kBlurTR);
  WarpCall wc;   // the affine steps': the source and the output are the sample's size
  memset(&wc, 0, sizeof(wc));
  wc.sw = w; wc.sh = h; wc.ow = w; wc.oh = h; wc.nhwc = c.nhwc; wc.tiles_x = c.tiles_x; wc.tiles = c.tiles;
  for (int k = 0; k < 3; k++) { wc.scale[k] = d->scale[k]; wc.bias[k] = d->bias[k]; }
  const PhotoEntry* dev = (const PhotoEntry*)st.base.table.dev;
  uint64_t launches = 0;
  bool known = true;
  for (int t = 0; t < steps && known; t++) {
    const std::array<int, KIND_COUNT>& cnt = count[(size_t)t];
    const PhotoEntry* tab = dev + first[(size_t)t];
    const AugmentEntry* hue = (const AugmentEntry*)(tab + cnt[KIND_APPLY] + cnt[KIND_HIST]);
    const AugmentEntry* blur = hue + cnt[KIND_HUE];
    dim3 block(256);
    if (cnt[KIND_HIST]) {
      HIPDEC_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)cnt[KIND_HIST] * 4 * 256 * sizeof(uint32_t), s));
      hipLaunchKernelGGL(k_photo_hist, dim3((unsigned)((uint64_t)c.slices * (uint64_t)cnt[KIND_HIST])), block, 0, s, tab + cnt[KIND_APPLY], c);
      launches++;
    }
    if (cnt[KIND_APPLY]) {
      dim3 grid((unsigned)((uint64_t)c.tiles * (uint64_t)cnt[KIND_APPLY]));   // (chain_check: below 2^31)
      known = dispatch_dtype(d->dtype, [&](auto dt) { hipLaunchKernelGGL((k_photo_apply<decltype(dt)::value>), grid, block, 0, s, tab, c); });
      launches++;
    }
    if (known && cnt[KIND_HUE]) {
      dim3 grid((unsigned)((uint64_t)c.tiles * (uint64_t)cnt[KIND_HUE]));
      known = dispatch_dtype(d->dtype, [&](auto dt) { hipLaunchKernelGGL((k_augment_hue<decltype(dt)::value>), grid, block, 0, s, hue, c); });
      launches++;
    }
    if (known && cnt[KIND_BLUR]) {
      dim3 grid((unsigned)((uint64_t)bc.tiles * (uint64_t)cnt[KIND_BLUR]));   // (fewer than the 64 x 16 tiles chain_check bounds)
      const int rmax = blur_r[(size_t)t];
      known = dispatch_dtype(d->dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (rmax <= 1) hipLaunchKernelGGL((k_augment_blur<DT, 1>), grid, block, 0, s, blur, bc);
        else if (rmax <= 3) hipLaunchKernelGGL((k_augment_blur<DT, 3>), grid, block, 0, s, blur, bc);
        else hipLaunchKernelGGL((k_augment_blur<DT, kAugmentBlurMaxR>), grid, block, 0, s, blur, bc);
      });
      launches++;
    }
    const WarpEntry* affine = (const WarpEntry*)(blur + cnt[KIND_BLUR]);
    for (int f = 0; f < 3 && known; f++) {   // nearest, bilinear, bicubic: the step's affine records of that filter
      const int na = cnt[KIND_AFFINE_NEAREST + f];
      if (!na) continue;
      dim3 grid((unsigned)((uint64_t)wc.tiles * (uint64_t)na));   // (chain_check: below 2^31)
      known = dispatch_dtype(d->dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (f == 0) hipLaunchKernelGGL((k_recipe_affine_nearest<DT>), grid, block, 0, s, affine, wc);
        else if (f == 1) hipLaunchKernelGGL((k_recipe_affine_bilinear<DT>), grid, block, 0, s, affine, wc);
        else hipLaunchKernelGGL((k_recipe_affine_bicubic<DT>), grid, block, 0, s, affine, wc);
      });
      launches++;
      affine += na;
    }
  }
  if (!known) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: unknown dtype %d", chain_stage_name(chains), d->dtype);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(HIPDEC_ERR_DEVICE, "%s kernel launch: %s", chains.recipe ? "recipe" : (chains.augment ? "augment" : "photo"), hipGetErrorString(e));
  if (!st.base.done) HIPDEC_CHECK_HIP(hipEventCreateWithFlags(&st.base.done, hipEventDisableTiming));
  HIPDEC_CHECK_HIP(hipEventRecord(st.base.done, s));
  st.base.last = s;
  if (chains.recipe) { g_recipe_calls++; g_recipe_entries += (uint64_t)n; g_recipe_launches += launches; g_recipe_affine_steps += affine_steps; }
  else if (chains.augment) { g_augment_calls++; g_augment_entries += (uint64_t)n; g_augment_launches += launches; }
  else { g_photo_calls++; g_photo_entries += (uint64_t)n; g_photo_launches += launches; }
  return 0;
}

// debug inspection of the blocks last handed to the tensor kernels: plane `plane` of entry `entry` as the kernel receives it - the pointer and stride of the
// PLANE, and the window of it that is scaled
int color_tensor_inspect(const ColorBatchState& st, int entry, int plane, const void** plane_dev, size_t* stride, int* x, int* y, int* w, int* h)
{
  if (entry < 0 || plane < 0 || plane > 2 || (size_t)(entry + 1) * sizeof(TensorParams) > st.host.size()) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_block: no such block");
  TensorParams tp;
  memcpy(&tp, st.host.data() + (size_t)entry * sizeof(TensorParams), sizeof(tp));
  const int sH = plane ? tp.sH : 0, sV = plane ? tp.sV : 0;
  *plane_dev = plane == 0 ? tp.c.y : (plane == 1 ? tp.c.cb : tp.c.cr);
  *stride = plane == 0 ? tp.c.ys : (plane == 1 ? tp.c.cbs : tp.c.crs);
  *x = tp.left >> sH; *y = tp.top >> sV;
  *w = ((tp.left + tp.rw - 1) >> sH) - *x + 1; *h = ((tp.top + tp.rh - 1) >> sV) - *y + 1;
  return 0;
}

int scale_planes_launch(PlaneScaleParams* jobs, int n, int bytes_per_sample, int filter, void* dev_params, hipStream_t s)
{
  if (n <= 0) return 0;
  int max_qw = 0, max_qh = 0, max_tiles = 0;
  for (int i = 0; i < n; i++) {
    PlaneScaleParams& j = jobs[i];
    j.tile = box_tile_of(j.pw, j.qw);
    max_qw = j.qw > max_qw ? j.qw : max_qw; max_qh = j.qh > max_qh ? j.qh : max_qh;
    const int tiles = (j.qw + j.tile - 1) / j.tile;
    max_tiles = tiles > max_tiles ? tiles : max_tiles;
  }
  HIPDEC_CHECK_HIP(hipMemcpyAsync(dev_params, jobs, (size_t)n * sizeof(PlaneScaleParams), hipMemcpyHostToDevice, s));
  const PlaneScaleParams* dev = (const PlaneScaleParams*)dev_params;
  if (bytes_per_sample == 1) launch_box_or_nearest(filter, k_scale_plane_box<uint8_t>, k_scale_plane_nearest<uint8_t>, max_tiles, max_qh, max_qw, max_qh, n, s, dev);
  else launch_box_or_nearest(filter, k_scale_plane_box<uint16_t>, k_scale_plane_nearest<uint16_t>, max_tiles, max_qh, max_qw, max_qh, n, s, dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(HIPDEC_ERR_DEVICE, "plane scaler launch: %s", hipGetErrorString(e));
  return 0;
}

void color_batch_state_free(ColorBatchState& st)
{
  if (st.dev) arena_release(st.dev, st.dev_bytes);
  st.dev = nullptr; st.dev_bytes = 0; st.host.clear();
}

}  // namespace hipdec

using namespace hipdec;

extern "C" {

int hipdec_resample_taps(int in_size, int out_size, int filter, int out_index, int* first, int32_t* coeffs, int capacity)
{
  if (filter != HIPDEC_SCALE_BILINEAR && filter != HIPDEC_SCALE_BICUBIC) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "resample_taps: filter %d has no taps (bilinear 16, bicubic 17)", filter);
  if (in_size < 1 || out_size < 1 || out_index < 0 || out_index >= out_size || !first || capacity < 0 || (capacity > 0 && !coeffs))
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "resample_taps: bad arguments");
  return guarded("resample_taps", [&]() -> int {
    const ResampleAxis a = resample_axis_of(in_size, out_size, filter);
    std::vector<double> w((size_t)a.stride);
    std::vector<int32_t> k((size_t)a.stride);
    const int n = resample_taps_of(a, out_index, first, k.data(), w.data());
    for (int x = 0; x < n && x < capacity; x++) coeffs[x] = k[x];
    return n;
  });
}

void hipdec_oriented_stats(uint64_t* launches, uint64_t* entries, uint64_t* quarter_turn_entries)
{
  if (launches) *launches = g_oriented_launches.load();
  if (entries) *entries = g_oriented_entries.load();
  if (quarter_turn_entries) *quarter_turn_entries = g_oriented_quarter.load();
}

void hipdec_packed_stats(uint64_t* calls, uint64_t* entries, uint64_t* patch_entries)
{
  if (calls) *calls = g_packed_calls.load();
  if (entries) *entries = g_packed_entries.load();
  if (patch_entries) *patch_entries = g_packed_patch_entries.load();
}

void hipdec_framed_stats(uint64_t* calls, uint64_t* entries, uint64_t* tiles, uint64_t* tiles_skipped)
{
  if (calls) *calls = g_framed_calls.load();
  if (entries) *entries = g_framed_entries.load();
  if (tiles) *tiles = g_framed_tiles.load();
  if (tiles_skipped) *tiles_skipped = g_framed_skipped.load();
}

void hipdec_composed_stats(uint64_t* calls, uint64_t* entries, uint64_t* pieces, uint64_t* hidden_entries, uint64_t* cover_launches)
{
  if (calls) *calls = g_composed_calls.load();
  if (entries) *entries = g_composed_entries.load();
  if (pieces) *pieces = g_composed_pieces.load();
  if (hidden_entries) *hidden_entries = g_composed_hidden.load();
  if (cover_launches) *cover_launches = g_composed_cover_launches.load();
}

void hipdec_placed_stats(uint64_t* calls, uint64_t* entries, uint64_t* margin_launches)
{
  if (calls) *calls = g_placed_calls.load();
  if (entries) *entries = g_placed_entries.load();
  if (margin_launches) *margin_launches = g_placed_margin_launches.load();
}

void hipdec_warp_stats(uint64_t* calls, uint64_t* entries)
{
  if (calls) *calls = g_warp_calls.load();
  if (entries) *entries = g_warp_entries.load();
}

void hipdec_photo_stats(uint64_t* calls, uint64_t* entries, uint64_t* launches)
{
  if (calls) *calls = g_photo_calls.load();
  if (entries) *entries = g_photo_entries.load();
  if (launches) *launches = g_photo_launches.load();
}

// the stage alone (hipdec_tensor_photo, hipdec_tensor_augment); its tables and work memory live in a state the process keeps per device, as
// hipdec_tensor_warp's do
static int tensor_chain_stage(const char* who, const void* src_dev, size_t src_bytes, const hipdec_photo_desc* photo, const ChainView& chains,
                              const hipdec_tensor_desc* desc, int n, void* out_dev, size_t out_bytes, void* stream)
{
  static std::mutex mu;
  static std::map<int, PhotoState> states;   // by device
  if (!desc || n < 0) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
  if (desc->dtype < HIPDEC_TENSOR_U8 || desc->dtype > HIPDEC_TENSOR_BF16) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: unknown dtype %d", who, desc->dtype);
  if (desc->layout != HIPDEC_TENSOR_NCHW && desc->layout != HIPDEC_TENSOR_NHWC) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: unknown layout %d", who, desc->layout);
  if (desc->dtype != HIPDEC_TENSOR_U8)
    for (int c = 0; c < 3; c++)
      if (!std::isfinite(desc->scale[c]) || !std::isfinite(desc->bias[c])) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: scale / bias of channel %d is not finite", who, c);
  if (int rc = chain_check(who, photo, chains, desc, n)) return rc;
  const uint64_t es = desc->dtype == HIPDEC_TENSOR_U8 ? 1 : (desc->dtype == HIPDEC_TENSOR_F32 ? 4 : 2);
  const uint64_t per_src = 3ull * (uint64_t)photo->src_width * (uint64_t)photo->src_height;   // (below 2^32: sizes below 2^15; times n below 2^31, times 4: below 2^63)
  if (src_bytes < per_src * (uint64_t)n) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: src_bytes %zu is smaller than the %d samples of %llu bytes", who, src_bytes, n, (unsigned long long)per_src);
  if (out_bytes < per_src * es * (uint64_t)n) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: out_bytes %zu is smaller than the tensor of %llu bytes", who, out_bytes, (unsigned long long)(per_src * es * (uint64_t)n));
  if (n == 0) return 0;
  if (!src_dev || !out_dev) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
  // (everything above is decided without a device)
  if (int rc = ensure_init()) return rc;
  return guarded(who, [&]() -> int {
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    HIPDEC_CHECK_HIP(hipGetDevice(&dev));
    return chain_launch(states[dev], src_dev, photo, chains, desc, n, out_dev, stream ? (hipStream_t)stream : default_stream());
  });
}

int hipdec_tensor_photo(const void* src_dev, size_t src_bytes, const hipdec_photo_desc* photo, const hipdec_photo_chain* chains, const hipdec_tensor_desc* desc,
                        int n, void* out_dev, size_t out_bytes, void* stream)
{
  return tensor_chain_stage("tensor_photo", src_dev, src_bytes, photo, chain_view(chains), desc, n, out_dev, out_bytes, stream);
}

int hipdec_tensor_augment(const void* src_dev, size_t src_bytes, const hipdec_photo_desc* photo, const hipdec_augment_chain* chains,
                          const hipdec_tensor_desc* desc, int n, void* out_dev, size_t out_bytes, void* stream)
{
  return tensor_chain_stage("tensor_augment", src_dev, src_bytes, photo, chain_view(chains), desc, n, out_dev, out_bytes, stream);
}

void hipdec_augment_stats(uint64_t* calls, uint64_t* entries, uint64_t* launches)
{
  if (calls) *calls = g_augment_calls.load();
  if (entries) *entries = g_augment_entries.load();
  if (launches) *launches = g_augment_launches.load();
}

int hipdec_tensor_recipe(const void* src_dev, size_t src_bytes, const hipdec_photo_desc* photo, const hipdec_augment_chain* chains,
                         const hipdec_recipe_affine* affines, int n_affines, const hipdec_tensor_desc* desc, int n, void* out_dev, size_t out_bytes, void* stream)
{
  return tensor_chain_stage("tensor_recipe", src_dev, src_bytes, photo, recipe_view(chains, affines, n_affines), desc, n, out_dev, out_bytes, stream);
}

void hipdec_recipe_stats(uint64_t* calls, uint64_t* entries, uint64_t* launches, uint64_t* affine_steps)
{
  if (calls) *calls = g_recipe_calls.load();
  if (entries) *entries = g_recipe_entries.load();
  if (launches) *launches = g_recipe_launches.load();
  if (affine_steps) *affine_steps = g_recipe_affine_steps.load();
}

int hipdec_gaussian_box(double radius, int* r, uint32_t* ww, uint32_t* fw)
{
  if (!r || !ww || !fw) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "gaussian_box: bad arguments"), -1;
  if (!std::isfinite(radius) || radius < 0.0 || radius > kAugmentBlurMaxRadius)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "gaussian_box: the radius %g is not 0 .. %g", radius, kAugmentBlurMaxRadius), -1;
  augment_gaussian_box(radius, r, ww, fw);
  return 0;
}

// Pillow's Image.rotate matrix without expand (Image.py rotate): cos and sin of -radians(angle mod 360) rounded to 15 decimal places - printed with 15
// places and read back, which is what Python's round(x, 15) does -, the centre (width / 2, height / 2), the translation as Pillow computes it
int hipdec_rotate_map(double angle, int width, int height, hipdec_tensor_map* out)
{
  if (!out || !std::isfinite(angle) || width < 1 || height < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "rotate_map: angle %g, size %d x %d", angle, width, height), -1;
  angle = std::fmod(angle, 360.0);
  if (angle < 0.0) angle += 360.0;                                   // (Python's %: the result has the divisor's sign)
  if (angle == 0.0) angle = 0.0;                                     // (... and a zero result is +0)
  const double rad = -(angle * (3.14159265358979323846 / 180.0));   // math.radians
  auto round15 = [](double v) { char buf[64]; snprintf(buf, sizeof buf, "%.15f", v); return strtod(buf, nullptr); };
  const double c = round15(std::cos(rad)), s = round15(std::sin(rad)), ms = round15(-std::sin(rad));
  const double cx = (double)width / 2.0, cy = (double)height / 2.0;
  double* m = out->m;
  m[0] = c; m[1] = s; m[2] = 0.0; m[3] = ms; m[4] = c; m[5] = 0.0;
  const double tx = m[0] * -cx + m[1] * -cy + m[2], ty = m[3] * -cx + m[4] * -cy + m[5];
  m[2] = tx + cx; m[5] = ty + cy;
  return 0;
}

// the stage alone; its table lives in a state the process keeps per device (calls on different streams are ordered against each other by the state's event)
int hipdec_tensor_warp(const void* src_dev, size_t src_bytes, const hipdec_warp_desc* warp, const hipdec_tensor_map* maps, const hipdec_tensor_fill* fill,
                       const hipdec_tensor_desc* desc, int n, void* out_dev, size_t out_bytes, void* stream)
{
  static std::mutex mu;
  static std::map<int, WarpState> states;   // by device: the table is device memory
  if (!desc || n < 0) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_warp: bad arguments");
  if (desc->width < 1 || desc->height < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_warp: output size %d x %d", desc->width, desc->height);
  if (desc->dtype < HIPDEC_TENSOR_U8 || desc->dtype > HIPDEC_TENSOR_BF16) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_warp: unknown dtype %d", desc->dtype);
  if (desc->layout != HIPDEC_TENSOR_NCHW && desc->layout != HIPDEC_TENSOR_NHWC) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_warp: unknown layout %d", desc->layout);
  if (desc->dtype != HIPDEC_TENSOR_U8)
    for (int c = 0; c < 3; c++)
      if (!std::isfinite(desc->scale[c]) || !std::isfinite(desc->bias[c])) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_warp: scale / bias of channel %d is not finite", c);
  if (int rc = warp_check("tensor_warp", warp, maps, fill, desc, n)) return rc;
  const uint64_t es = desc->dtype == HIPDEC_TENSOR_U8 ? 1 : (desc->dtype == HIPDEC_TENSOR_F32 ? 4 : 2);
  const uint64_t need_src = 3ull * (uint64_t)warp->src_width * (uint64_t)warp->src_height * (uint64_t)n;   // (below 2^63: sizes below 2^15, n below 2^31)
  const uint64_t per_out = 3ull * (uint64_t)desc->width * (uint64_t)desc->height * es;
  if ((uint64_t)desc->width * (uint64_t)desc->height > (1ull << 40) || (n > 0 && per_out > (~0ull) / (uint64_t)n))
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_warp: tensor too large");
  if (src_bytes < need_src) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_warp: src_bytes %zu is smaller than the %d samples of %llu bytes", src_bytes, n, (unsigned long long)need_src);
  if (out_bytes < per_out * (uint64_t)n) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_warp: out_bytes %zu is smaller than the tensor of %llu bytes", out_bytes, (unsigned long long)(per_out * (uint64_t)n));
  if (n == 0) return 0;
  if (!src_dev || !out_dev) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_warp: bad arguments");
  // (everything above is decided without a device)
  if (int rc = ensure_init()) return rc;
  return guarded("tensor_warp", [&]() -> int {
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    HIPDEC_CHECK_HIP(hipGetDevice(&dev));
    return warp_launch(states[dev], src_dev, warp, maps, fill, desc, n, out_dev, stream ? (hipStream_t)stream : default_stream());
  });
}

void hipdec_project_stats(uint64_t* calls, uint64_t* entries)
{
  if (calls) *calls = g_project_calls.load();
  if (entries) *entries = g_project_entries.load();
}

int hipdec_perspective_map(const double startpoints[8], const double endpoints[8], hipdec_tensor_projection* out)
{
  if (!startpoints || !endpoints || !out) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "perspective_map: bad arguments");
  hipdec_tensor_projection p;
  memset(&p, 0, sizeof(p));
  p.kind = HIPDEC_PROJECT_PERSPECTIVE;
  if (!project_perspective_map(startpoints, endpoints, p.a))
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "perspective_map: the system of the four point pairs is singular or not finite");
  *out = p;
  return 0;
}

int hipdec_quad_map(const double corners[8], int width, int height, hipdec_tensor_projection* out)
{
  if (!corners || !out || width < 1 || height < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "quad_map: bad arguments (size %d x %d)", width, height);
  for (int i = 0; i < 8; i++)
    if (!std::isfinite(corners[i])) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "quad_map: corner value %d is not finite", i);
  memset(out, 0, sizeof(*out));
  out->kind = HIPDEC_PROJECT_QUAD;
  project_quad_map(corners, width, height, out->a);
  return 0;
}

// the stage alone; its table lives in a state the process keeps per device, as hipdec_tensor_warp's does
int hipdec_tensor_project(const void* src_dev, size_t src_bytes, const hipdec_warp_desc* warp, const hipdec_tensor_projection* maps, const hipdec_tensor_fill* fill,
                          const hipdec_tensor_desc* desc, int n, void* out_dev, size_t out_bytes, void* stream)
{
  static std::mutex mu;
  static std::map<int, WarpState> states;   // by device: the table is device memory
  if (!desc || n < 0) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_project: bad arguments");
  if (desc->width < 1 || desc->height < 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_project: output size %d x %d", desc->width, desc->height);
  if (desc->dtype < HIPDEC_TENSOR_U8 || desc->dtype > HIPDEC_TENSOR_BF16) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_project: unknown dtype %d", desc->dtype);
  if (desc->layout != HIPDEC_TENSOR_NCHW && desc->layout != HIPDEC_TENSOR_NHWC) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_project: unknown layout %d", desc->layout);
  if (desc->dtype != HIPDEC_TENSOR_U8)
    for (int c = 0; c < 3; c++)
      if (!std::isfinite(desc->scale[c]) || !std::isfinite(desc->bias[c])) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_project: scale / bias of channel %d is not finite", c);
  if (int rc = project_check("tensor_project", warp, maps, fill, desc, n)) return rc;
  const uint64_t es = desc->dtype == HIPDEC_TENSOR_U8 ? 1 : (desc->dtype == HIPDEC_TENSOR_F32 ? 4 : 2);
  const uint64_t need_src = 3ull * (uint64_t)warp->src_width * (uint64_t)warp->src_height * (uint64_t)n;   // (below 2^63: sizes below 2^15, n below 2^31)
  const uint64_t per_out = 3ull * (uint64_t)desc->width * (uint64_t)desc->height * es;
  if ((uint64_t)desc->width * (uint64_t)desc->height > (1ull << 40) || (n > 0 && per_out > (~0ull) / (uint64_t)n))
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_project: tensor too large");
  if (src_bytes < need_src) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_project: src_bytes %zu is smaller than the %d samples of %llu bytes", src_bytes, n, (unsigned long long)need_src);
  if (out_bytes < per_out * (uint64_t)n) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_project: out_bytes %zu is smaller than the tensor of %llu bytes", out_bytes, (unsigned long long)(per_out * (uint64_t)n));
  if (n == 0) return 0;
  if (!src_dev || !out_dev) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "tensor_project: bad arguments");
  // (everything above is decided without a device)
  if (int rc = ensure_init()) return rc;
  return guarded("tensor_project", [&]() -> int {
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    HIPDEC_CHECK_HIP(hipGetDevice(&dev));
    return project_launch(states[dev], src_dev, warp, maps, fill, desc, n, out_dev, stream ? (hipStream_t)stream : default_stream());
  });
}

void hipdec_color_coefficients(const hipdec_nclx* nclx, float out[4]) { if (out) coefficients(nclx, out); }   // (nclx NULL: the reference's defaults)

int hipdec_color_420_to_rgb24(const void* y, size_t ys, const void* cb, size_t cbs, const void* cr, size_t crs, int w, int h,
                              const hipdec_nclx* nclx, void* out, size_t out_stride, int with_alpha, void* stream)
{
  if (int rc = ensure_init()) return rc;
  // Op_YCbCr420_to_RGB24::state_after_conversion (yuv2rgb.cc:298-341) refuses these inputs
  if (nclx && nclx->has_nclx) {
    int m = nclx->matrix_coefficients;
    if (m == 0 || m == 8 || m == 11 || m == 14)
      return set_error(HIPDEC_ERR_UNSUPPORTED, "420_to_rgb24: matrix_coefficients %d is not handled by this op", m);
    if (!nclx->full_range_flag) return set_error(HIPDEC_ERR_UNSUPPORTED, "420_to_rgb24: limited range is not handled by this op");
  }
  ColorParams p;
  if (int rc = fill_common(p, y, ys, cb, cbs, cr, crs, w, h, 8, 1, nclx)) return rc;
  if (!out) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "420_to_rgb24: out is NULL");
  p.arith = AR_INT88; p.o0 = (uint8_t*)out; p.os = out_stride;
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  return with_alpha ? launch_rgb<uint8_t, LO_RGBA32>(p, s) : launch_rgb<uint8_t, LO_RGB24>(p, s);
}

/* RGBA with a real alpha plane (Op_YCbCr420_to_RGB32 with an alpha channel, yuv2rgb.cc:521-553; the float chain copies the alpha
 * plane the same way, rgb2rgb.cc:72-150): `alpha` NULL fills 0xFF */
int hipdec_color_420_to_rgba_alpha(const void* y, size_t ys, const void* cb, size_t cbs, const void* cr, size_t crs, int w, int h,
                                   const hipdec_nclx* nclx, const void* alpha, size_t alpha_stride, int integer_op, int chroma,
                                   void* out, size_t out_stride, void* stream)
{
  if (int rc = ensure_init()) return rc;
  ColorParams p;
  if (int rc = fill_common(p, y, ys, cb, cbs, cr, crs, w, h, 8, integer_op ? 1 : chroma, nclx)) return rc;
  if (!out) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "420_to_rgba: out is NULL");
  p.arith = integer_op ? AR_INT88 : generic_arith(nclx);
  p.o0 = (uint8_t*)out; p.os = out_stride; p.a = (const uint8_t*)alpha; p.as = alpha_stride;
  return launch_rgb<uint8_t, LO_RGBA32>(p, stream ? (hipStream_t)stream : default_stream());
}

int hipdec_color_ycbcr_to_rgb_planar(const void* y, size_t ys, const void* cb, size_t cbs, const void* cr, size_t crs, int w,
                                     int h, int bpp, int chroma, const hipdec_nclx* nclx, void* r, void* g, void* b,
                                     size_t out_stride, void* stream)
{
  if (int rc = ensure_init()) return rc;
  if (bpp < 8 || bpp > 14) return set_error(HIPDEC_ERR_UNSUPPORTED, "ycbcr_to_rgb: bits per pixel %d outside 8..14", bpp);
  if (nclx && nclx->has_nclx && (nclx->matrix_coefficients == 11 || nclx->matrix_coefficients == 14))
    return set_error(HIPDEC_ERR_UNSUPPORTED, "ycbcr_to_rgb: matrix_coefficients %d unsupported (as in the reference)", nclx->matrix_coefficients);
  ColorParams p;
  if (int rc = fill_common(p, y, ys, cb, cbs, cr, crs, w, h, bpp, chroma, nclx)) return rc;
  if (!r || !g || !b) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "ycbcr_to_rgb: output plane is NULL");
  p.arith = generic_arith(nclx); p.o0 = (uint8_t*)r; p.o1 = (uint8_t*)g; p.o2 = (uint8_t*)b; p.os = out_stride;
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  return bpp == 8 ? launch_rgb<uint8_t, LO_PLANAR>(p, s) : launch_rgb<uint16_t, LO_PLANAR>(p, s);
}

int hipdec_color_ycbcr_to_rgb24_float(const void* y, size_t ys, const void* cb, size_t cbs, const void* cr, size_t crs, int w,
                                      int h, int chroma, const hipdec_nclx* nclx, void* out, size_t out_stride, int with_alpha,
                                      void* stream)
{
  if (int rc = ensure_init()) return rc;
  if (nclx && nclx->has_nclx && (nclx->matrix_coefficients == 11 || nclx->matrix_coefficients == 14))
    return set_error(HIPDEC_ERR_UNSUPPORTED, "ycbcr_to_rgb24: matrix_coefficients %d unsupported (as in the reference)", nclx->matrix_coefficients);
  ColorParams p;
  if (int rc = fill_common(p, y, ys, cb, cbs, cr, crs, w, h, 8, chroma, nclx)) return rc;
  if (!out) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "ycbcr_to_rgb24: out is NULL");
  p.arith = generic_arith(nclx); p.o0 = (uint8_t*)out; p.os = out_stride;
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  return with_alpha ? launch_rgb<uint8_t, LO_RGBA32>(p, s) : launch_rgb<uint8_t, LO_RGB24>(p, s);
}

int hipdec_color_420_to_rrggbb(const void* y, size_t ys, const void* cb, size_t cbs, const void* cr, size_t crs, int w, int h,
                               int bpp, const hipdec_nclx* nclx, void* out, size_t out_stride, int little_endian, void* stream)
{
  if (int rc = ensure_init()) return rc;
  if (bpp <= 8 || bpp > 16) return set_error(HIPDEC_ERR_UNSUPPORTED, "420_to_rrggbb: needs more than 8 bits per pixel");
  if (nclx && nclx->has_nclx) {
    int m = nclx->matrix_coefficients;  // yuv2rgb.cc:590-593
    if (m == 0 || m == 8 || m == 11 || m == 14)
      return set_error(HIPDEC_ERR_UNSUPPORTED, "420_to_rrggbb: matrix_coefficients %d is not handled by this op", m);
  }
  ColorParams p;
  if (int rc = fill_common(p, y, ys, cb, cbs, cr, crs, w, h, bpp, 1, nclx)) return rc;
  if (!out) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "420_to_rrggbb: out is NULL");
  p.arith = AR_FLOAT; p.o0 = (uint8_t*)out; p.os = out_stride;
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  return little_endian ? launch_rgb<uint16_t, LO_RRGGBB_LE>(p, s) : launch_rgb<uint16_t, LO_RRGGBB_BE>(p, s);
}

/* Op_mono_to_RGB24_32 (libheif/color-conversion/monochrome.cc): an 8-bit monochrome plane to interleaved RGB24 / RGBA32, R = G = B = Y; the alpha
 * plane of the image is copied when there is one (NULL: 0xFF) */
int hipdec_color_mono_to_rgb24(const void* y, size_t ys, const void* alpha, size_t alpha_stride, int w, int h, void* out, size_t out_stride,
                               int with_alpha, void* stream)
{
  if (int rc = ensure_init()) return rc;
  if (!y || !out || w <= 0 || h <= 0) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "mono_to_rgb24: bad arguments");
  if (alpha && !with_alpha) return set_error(HIPDEC_ERR_UNSUPPORTED, "mono_to_rgb24: dropping an alpha plane is left to the stock ops");
  ColorParams p;
  memset(&p, 0, sizeof(p));
  p.y = (const uint8_t*)y; p.ys = ys; p.cb = p.cr = (const uint8_t*)y; p.cbs = p.crs = ys;   // (never read: AR_MONO)
  p.w = w; p.h = h; p.bpp = 8; p.arith = AR_MONO; p.full_range = 1;
  p.a = (const uint8_t*)alpha; p.as = alpha_stride;
  p.o0 = (uint8_t*)out; p.os = out_stride;
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  return with_alpha ? launch_rgb<uint8_t, LO_RGBA32>(p, s) : launch_rgb<uint8_t, LO_RGB24>(p, s);
}

/* > 8-bit planes to 8-bit interleaved RGB(A), one pass, as the two chains the reference's planner builds for it (which one: hipdec_color_plan):
 *   sdr_first = 1: Op_to_sdr_planes on Y, Cb, Cr, then Op_YCbCr420_to_RGB24 / _RGB32 (4:2:0, full range, a matrix the integer op takes)
 *   sdr_first = 0: Op_YCbCr_to_RGB<uint16_t> at the input depth, Op_to_sdr_planes on R, G, B, Op_RGB_to_RGB24_32 (everything else) */
int hipdec_color_hdr_to_rgb24(const void* y, size_t ys, const void* cb, size_t cbs, const void* cr, size_t crs, int w, int h, int bpp, int chroma,
                              const hipdec_nclx* nclx, void* out, size_t out_stride, int with_alpha, int sdr_first, void* stream)
{
  if (int rc = ensure_init()) return rc;
  if (bpp <= 8 || bpp > 14) return set_error(HIPDEC_ERR_UNSUPPORTED, "hdr_to_rgb24: bits per pixel %d outside 9..14", bpp);
  if (nclx && nclx->has_nclx && (nclx->matrix_coefficients == 11 || nclx->matrix_coefficients == 14))
    return set_error(HIPDEC_ERR_UNSUPPORTED, "hdr_to_rgb24: matrix_coefficients %d unsupported (as in the reference)", nclx->matrix_coefficients);
  ColorParams p;
  if (sdr_first) {
    if (chroma != 1) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "hdr_to_rgb24: the sdr-first chain is the 4:2:0 integer op's");
    if (nclx && nclx->has_nclx) {   // Op_YCbCr420_to_RGB24::state_after_conversion (yuv2rgb.cc:298-341)
      const int m = nclx->matrix_coefficients;
      if (m == 0 || m == 8 || !nclx->full_range_flag) return set_error(HIPDEC_ERR_UNSUPPORTED, "hdr_to_rgb24: the integer op does not take this colour profile");
    }
    if (int rc = fill_common(p, y, ys, cb, cbs, cr, crs, w, h, 8, 1, nclx)) return rc;
    p.arith = AR_INT88; p.in_shift = bpp - 8;
  } else {
    if (int rc = fill_common(p, y, ys, cb, cbs, cr, crs, w, h, bpp, chroma, nclx)) return rc;
    p.arith = generic_arith(nclx); p.out_shift = bpp - 8;
  }
  if (!out) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "hdr_to_rgb24: out is NULL");
  p.o0 = (uint8_t*)out; p.os = out_stride;
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  return with_alpha ? launch_rgb<uint16_t, LO_RGBA32>(p, s) : launch_rgb<uint16_t, LO_RGB24>(p, s);
}

/* Op_YCbCr_to_RGB<uint16_t> (yuv2rgb.cc:92-292, nearest-neighbour chroma for 4:2:0 / 4:2:2 inputs) + Op_RGB_HDR_to_RRGGBBaa_BE (rgb2rgb.cc)
 * [+ Op_RRGGBBaa_swap_endianness for little endian] as ONE pass: what the reference's planner chains for > 8-bit planes of any chroma format that
 * the 4:2:0-only op above does not take (4:2:2, 4:4:4, matrix_coefficients 0 / 8); the components keep the input bit depth */
int hipdec_color_ycbcr_to_rrggbb_float(const void* y, size_t ys, const void* cb, size_t cbs, const void* cr, size_t crs, int w, int h,
                                       int bpp, int chroma, const hipdec_nclx* nclx, void* out, size_t out_stride, int little_endian, void* stream)
{
  if (int rc = ensure_init()) return rc;
  if (bpp <= 8 || bpp > 14) return set_error(HIPDEC_ERR_UNSUPPORTED, "ycbcr_to_rrggbb: bits per pixel %d outside 9..14", bpp);
  if (nclx && nclx->has_nclx && (nclx->matrix_coefficients == 11 || nclx->matrix_coefficients == 14))
    return set_error(HIPDEC_ERR_UNSUPPORTED, "ycbcr_to_rrggbb: matrix_coefficients %d unsupported (as in the reference)", nclx->matrix_coefficients);
  ColorParams p;
  if (int rc = fill_common(p, y, ys, cb, cbs, cr, crs, w, h, bpp, chroma, nclx)) return rc;
  if (!out) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "ycbcr_to_rrggbb: out is NULL");
  p.arith = generic_arith(nclx); p.o0 = (uint8_t*)out; p.os = out_stride;
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  return little_endian ? launch_rgb<uint16_t, LO_RRGGBB_LE>(p, s) : launch_rgb<uint16_t, LO_RRGGBB_BE>(p, s);
}

int hipdec_color_bilinear_420_to_444(const void* in, size_t is, int w, int h, int bpp, void* out, size_t os, void* stream)
{
  if (int rc = ensure_init()) return rc;
  if (!in || !out || w <= 0 || h <= 0) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "bilinear: bad arguments");
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  dim3 block(64, 4), grid(((w + 3) / 4 + 63) / 64, (h + 3) / 4);
  if (bpp <= 8) hipLaunchKernelGGL(k_bilinear_420_to_444<uint8_t>, grid, block, 0, s, (const uint8_t*)in, is, w, h, (uint8_t*)out, os);
  else hipLaunchKernelGGL(k_bilinear_420_to_444<uint16_t>, grid, block, 0, s, (const uint8_t*)in, is, w, h, (uint8_t*)out, os);
  HIPDEC_CHECK_HIP(hipGetLastError());
  return 0;
}

int hipdec_color_bilinear_422_to_444(const void* in, size_t is, int w, int h, int bpp, void* out, size_t os, void* stream)
{
  if (int rc = ensure_init()) return rc;
  if (!in || !out || w <= 0 || h <= 0) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "bilinear 4:2:2: bad arguments");
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  dim3 block(64, 4), grid(((w + 3) / 4 + 63) / 64, (h + 3) / 4);
  if (bpp <= 8) hipLaunchKernelGGL(k_bilinear_422_to_444<uint8_t>, grid, block, 0, s, (const uint8_t*)in, is, w, h, (uint8_t*)out, os);
  else hipLaunchKernelGGL(k_bilinear_422_to_444<uint16_t>, grid, block, 0, s, (const uint8_t*)in, is, w, h, (uint8_t*)out, os);
  HIPDEC_CHECK_HIP(hipGetLastError());
  return 0;
}

int hipdec_color_to_sdr(const void* in, size_t is, int w, int h, int bits, void* out, size_t os, void* stream)
{
  if (int rc = ensure_init()) return rc;
  if (!in || !out || w <= 0 || h <= 0 || bits <= 8 || bits > 16) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_sdr: bad arguments");
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  dim3 block(64, 4), grid(((w + 3) / 4 + 63) / 64, (h + 3) / 4);
  hipLaunchKernelGGL(k_to_sdr, grid, block, 0, s, (const uint8_t*)in, is, w, h, bits - 8, (uint8_t*)out, os);
  HIPDEC_CHECK_HIP(hipGetLastError());
  return 0;
}

int hipdec_color_to_hdr(const void* in, size_t is, int w, int h, int out_bits, void* out, size_t os, void* stream)
{
  if (int rc = ensure_init()) return rc;
  if (!in || !out || w <= 0 || h <= 0 || out_bits <= 8 || out_bits > 16) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "to_hdr: bad arguments");
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  dim3 block(64, 4), grid(((w + 3) / 4 + 63) / 64, (h + 3) / 4);
  hipLaunchKernelGGL(k_to_hdr, grid, block, 0, s, (const uint8_t*)in, is, w, h, out_bits, (uint8_t*)out, os);
  HIPDEC_CHECK_HIP(hipGetLastError());
  return 0;
}

int hipdec_color_swap_endianness(const void* in, size_t is, int w, int h, int components, void* out, size_t os, void* stream)
{
  if (int rc = ensure_init()) return rc;
  if (!in || !out || w <= 0 || h <= 0 || (components != 3 && components != 4)) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "swap_endianness: bad arguments");
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  const int row_bytes = w * components * 2;
  dim3 block(64, 4), grid(((row_bytes + 3) / 4 + 63) / 64, (h + 3) / 4);
  hipLaunchKernelGGL(k_swap16, grid, block, 0, s, (const uint8_t*)in, is, row_bytes, h, (uint8_t*)out, os);
  HIPDEC_CHECK_HIP(hipGetLastError());
  return 0;
}

/* one plane through the plane scaler (HIPDEC_SCALE_NEAREST: HeifPixelImage::scale_nearest_neighbor's per-plane loop, libheif/image/pixelimage.cc:1936-1967;
 * HIPDEC_SCALE_BOX: the area average of heif_hipdec.h); runs on `stream` and waits for it (the parameter block is this call's) */
int hipdec_plane_scale(const void* in, size_t in_stride, int in_w, int in_h, int bytes_per_sample, int image_w, int image_h, int image_out_w, int image_out_h,
                       int out_w, int out_h, int filter, void* out, size_t out_stride, void* stream)
{
  if (int rc = ensure_init()) return rc;
  if (!in || !out || in_w <= 0 || in_h <= 0 || out_w <= 0 || out_h <= 0 || image_w <= 0 || image_h <= 0 || image_out_w <= 0 || image_out_h <= 0 ||
      (bytes_per_sample != 1 && bytes_per_sample != 2))
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "plane_scale: bad arguments");
  if (filter != HIPDEC_SCALE_NEAREST && filter != HIPDEC_SCALE_BOX) return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "plane_scale: unknown filter %d", filter);
  if (in_stride < (size_t)in_w * bytes_per_sample || out_stride < (size_t)out_w * bytes_per_sample)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "plane_scale: a stride is smaller than its rows");
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  PlaneScaleParams j{(const uint8_t*)in, in_stride, in_w, in_h, (uint8_t*)out, out_stride, out_w, out_h, image_w, image_h, image_out_w, image_out_h, 0};
  void* dev = nullptr; size_t cap = 0;
  HIPDEC_CHECK_HIP(arena_acquire(&dev, sizeof(j), &cap));
  int rc = scale_planes_launch(&j, 1, bytes_per_sample, filter, dev, s);
  hipError_t e = hipStreamSynchronize(s);   // (the parameter block and its pageable source are this call's)
  arena_release(dev, cap);
  if (!rc && e != hipSuccess) rc = set_error(HIPDEC_ERR_DEVICE, "plane_scale: %s", hipGetErrorString(e));
  return rc;
}

int hipdec_color_pq_to_linear(const void* in, size_t is, int w, int h, int components, int bits, int big_endian, void* out, size_t os, void* stream)
{
  if (int rc = ensure_init()) return rc;
  if (!in || !out || w <= 0 || h <= 0 || components < 1 || components > 4 || bits < 8 || bits > 16)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "pq_to_linear: bad arguments");
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  const int n = w * components;
  if (bits <= 12) {
    hipLaunchKernelGGL(k_pq_to_linear_lut, dim3((n + 1023) / 1024, (h + 15) / 16), dim3(256), 0, s, (const uint8_t*)in, is, n, h, bits, big_endian, (float*)out, os);
  } else {
    dim3 block(64, 4), grid((n + 63) / 64, (h + 3) / 4);
    hipLaunchKernelGGL(k_pq_to_linear, grid, block, 0, s, (const uint8_t*)in, is, n, h, bits, big_endian, (float*)out, os);
  }
  HIPDEC_CHECK_HIP(hipGetLastError());
  return 0;
}

int hipdec_color_hlg_to_linear(const void* in, size_t is, int w, int h, int components, int bits, int big_endian, void* out, size_t os, void* stream)
{
  if (int rc = ensure_init()) return rc;
  if (!in || !out || w <= 0 || h <= 0 || components < 1 || components > 4 || bits < 8 || bits > 16)
    return set_error(HIPDEC_ERR_INVALID_ARGUMENT, "hlg_to_linear: bad arguments");
  hipStream_t s = stream ? (hipStream_t)stream : default_stream();
  const int n = w * components;
  if (bits <= 12) {
    hipLaunchKernelGGL(k_hlg_to_linear_lut, dim3((n + 1023) / 1024, (h + 15) / 16), dim3(256), 0, s, (const uint8_t*)in, is, n, h, bits, big_endian, (float*)out, os);
  } else {
    dim3 block(64, 4), grid((n + 63) / 64, (h + 3) / 4);
    hipLaunchKernelGGL(k_hlg_to_linear, grid, block, 0, s, (const uint8_t*)in, is, n, h, bits, big_endian, (float*)out, os);
  }
  HIPDEC_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
