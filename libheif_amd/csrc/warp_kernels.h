// warp_kernels.h — the warp stage of the tensor output (include/heif_hipdec.h, hipdec_tensor_warp): PIL.Image.transform(size, AFFINE, data, resample,
// fillcolor) of dense 8-bit interleaved RGB samples, bit for bit, into the normalised tensor.  Included by color.hip inside its kernel namespace, behind the
// tensor store helpers (TensorElem, TensorQuad, tensor_elem).
// Shape: ONE launch for all entries of a call.  A workgroup of 256 threads owns a tile of kWarpTC x kWarpTR output pixels of one entry; all entries have the
// same output size, so block b is tile b % tiles of entry b / tiles.  The entry's record (hipdec::WarpEntry: map, fill, pointers) is uniform per workgroup
// and comes through the constant address space - scalar loads into SGPRs, as k_recon8 reads its block plan; the description of the call is a kernel argument.
// A lane owns four consecutive pixels of a row, computes each as the definition states it - IEEE double, no contraction (-ffp-contract=off) - gathers its
// 2 x 2 or 4 x 4 source pixels straight from global memory (a 224 x 224 sample is 150 KB and was written by the launch in front: L2), and stores the group
// as the dense tensor kernels do: one 16 / 8 / 4-byte store per channel plane (NCHW) or three of them for its run of 12 elements (NHWC).
// The bicubic kernels loop over the channels so that one channel's sixteen taps are live at a time.

constexpr int kWarpTC = 64, kWarpTR = 16;   // the tile: 16 lanes x 4 pixels across, 16 rows

struct WarpCall {
  int sw, sh, ow, oh;
  int nhwc;
  uint32_t tiles_x, tiles;   // tiles across, tiles per entry
  float scale[3], bias[3];
};

__device__ __forceinline__ uint64_t warp_word(const hipdec::WarpEntry* p, uint32_t entry, int i)
{
  const uint64_t* w = (const uint64_t*)(p + entry) + i;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HIPDEC_HOST_EMU)
  return *(const __attribute__((address_space(4))) uint64_t*)(uintptr_t)w;
#else
  return *w;
#endif
}

__device__ __forceinline__ hipdec::WarpEntry warp_entry_load(const hipdec::WarpEntry* p, uint32_t entry)
{
  uint64_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = warp_word(p, entry, i);
  hipdec::WarpEntry E;
  E.src = (const uint8_t*)(uintptr_t)w[0]; E.o0 = (uint8_t*)(uintptr_t)w[1];
#pragma unroll
  for (int i = 0; i < 6; i++) E.m[i] = __builtin_bit_cast(double, w[2 + i]);
#pragma unroll
  for (int i = 0; i < 6; i++) E.A[i] = (int32_t)(uint32_t)(w[8 + i / 2] >> (32 * (i & 1)));
  E.xt = (const int32_t*)(uintptr_t)w[11]; E.yt = (const int32_t*)(uintptr_t)w[12];
  E.path = (int32_t)(uint32_t)w[13]; E.domain = (int32_t)(uint32_t)(w[13] >> 32);
  E.value[0] = __builtin_bit_cast(float, (uint32_t)w[14]); E.value[1] = __builtin_bit_cast(float, (uint32_t)(w[14] >> 32));
  E.value[2] = __builtin_bit_cast(float, (uint32_t)w[15]); E.reserved = 0;
  return E;
}

// the fill element of a channel: what a pixel of that component value gets, or the element itself (canvas_fill_elem's statement)
template <int DT>
__device__ __forceinline__ uint32_t warp_fill_elem(int domain, float value, float scale, float bias)
{
  if (domain == HIPDEC_FILL_COMPONENT) return tensor_elem<DT>((int)value, scale, bias);
  if (DT == TD_U8) return (uint32_t)(int)value;
  if (DT == TD_F32) return __builtin_bit_cast(uint32_t, value);
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HIPDEC_HOST_EMU)
  if (DT == TD_F16) return __builtin_bit_cast(uint16_t, (_Float16)value);
  return __builtin_bit_cast(uint16_t, (__bf16)value);
#else
  return DT == TD_F16 ? f32_to_f16_rne(__builtin_bit_cast(uint32_t, value)) : f32_to_bf16_rne(__builtin_bit_cast(uint32_t, value));
#endif
}

__device__ __forceinline__ int warp_floor_d(double v) { return v < 0.0 ? (int)floor(v) : (int)v; }

// component k of source pixel (xx, yy), both inside the sample
__device__ __forceinline__ int warp_src(const HIPDEC_GLOBAL uint8_t* src, int sw, int xx, int yy, int k)
{
  return (int)src[((size_t)yy * (size_t)sw + (size_t)xx) * 3 + (size_t)k];
}

// L(p, q, d) = p + (q - p) * d
__device__ __forceinline__ double warp_lerp(double p, double q, double d) { return p + (q - p) * d; }

// B(v1, v2, v3, v4, d)
__device__ __forceinline__ double warp_cubic(double v1, double v2, double v3, double v4, double d)
{
  const double p1 = v2, p2 = -v1 + v3, p3 = 2.0 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// the inside test of the BILINEAR / BICUBIC statements
__device__ __forceinline__ bool warp_inside(int sw, int sh, double xin, double yin) { return !(xin < 0.0 || xin >= (double)sw || yin < 0.0 || yin >= (double)sh); }

// xin, yin of output pixel (x, y); false: outside
__device__ __forceinline__ bool warp_map_pixel(const hipdec::WarpEntry& E, const WarpCall& c, int x, int y, double& xin, double& yin)
{
  const double xc = (double)x + 0.5, yc = (double)y + 0.5;
  xin = E.m[0] * xc + E.m[1] * yc + E.m[2];
  yin = E.m[3] * xc + E.m[4] * yc + E.m[5];
  return warp_inside(c.sw, c.sh, xin, yin);
}

// The sampling half of the BILINEAR / BICUBIC statements, from an inside (xin, yin) on: V[k], the 8-bit component values.  Stated once: k_warp_*,
// k_recipe_affine_* (through warp_pixel) and k_project_* (project_kernels.h) call it.
template <int FILTER>
__device__ __forceinline__ void warp_sample(const HIPDEC_GLOBAL uint8_t* src, int sw, int sh, double xin, double yin, int (&V)[3])
{
  xin -= 0.5; yin -= 0.5;
  const int ix = warp_floor_d(xin), iy = warp_floor_d(yin);
  const double dx = xin - (double)ix, dy = yin - (double)iy;
  if (FILTER == HIPDEC_SCALE_BILINEAR) {
    const int x0 = clip_i(ix, sw - 1), x1 = clip_i(ix + 1, sw - 1), y0 = clip_i(iy, sh - 1);
    const bool second = iy + 1 >= 0 && iy + 1 < sh;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double v1 = warp_lerp((double)warp_src(src, sw, x0, y0, k), (double)warp_src(src, sw, x1, y0, k), dx);
      double v2 = v1;
      if (second) v2 = warp_lerp((double)warp_src(src, sw, x0, iy + 1, k), (double)warp_src(src, sw, x1, iy + 1, k), dx);
      V[k] = (int)warp_lerp(v1, v2, dy);
    }
    return;
  }
  // bicubic: columns ix - 1 .. ix + 2 clamped; row iy - 1 clamped, rows iy .. iy + 2 used only where they exist
  int xs[4];
#pragma unroll
  for (int j = 0; j < 4; j++) xs[j] = clip_i(ix - 1 + j, sw - 1);
  const int yfirst = clip_i(iy - 1, sh - 1);
#pragma unroll 1
  for (int k = 0; k < 3; k++) {
    double r[4];
    r[0] = warp_cubic((double)warp_src(src, sw, xs[0], yfirst, k), (double)warp_src(src, sw, xs[1], yfirst, k), (double)warp_src(src, sw, xs[2], yfirst, k),
                      (double)warp_src(src, sw, xs[3], yfirst, k), dx);
#pragma unroll
    for (int j = 1; j < 4; j++) {
      const int yy = iy - 1 + j;
      r[j] = r[j - 1];
      if (yy >= 0 && yy < sh)
        r[j] = warp_cubic((double)warp_src(src, sw, xs[0], yy, k), (double)warp_src(src, sw, xs[1], yy, k), (double)warp_src(src, sw, xs[2], yy, k),
                          (double)warp_src(src, sw, xs[3], yy, k), dx);
    }
    const double v = warp_cubic(r[0], r[1], r[2], r[3], dy);
    const int val = v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (int)v);
    V[0] = k == 0 ? val : V[0]; V[1] = k == 1 ? val : V[1]; V[2] = k == 2 ? val : V[2];   // (selects: a runtime index would put V into scratch memory)
  }
}

// FILTER: hipdec_scale_filter.  V[k]: the 8-bit component values of output pixel (x, y); false: the pixel is outside and holds the fill
template <int FILTER>
__device__ __forceinline__ bool warp_pixel(const hipdec::WarpEntry& E, const WarpCall& c, int x, int y, int (&V)[3])
{
  const HIPDEC_GLOBAL uint8_t* src = (const HIPDEC_GLOBAL uint8_t*)E.src;
  const int sw = c.sw, sh = c.sh;
  if (FILTER == HIPDEC_SCALE_NEAREST) {
    int sx, sy;
    if (E.path == hipdec::WARP_PATH_TABLE) {
      sx = ((const HIPDEC_GLOBAL int32_t*)E.xt)[x];
      sy = ((const HIPDEC_GLOBAL int32_t*)E.yt)[y];
    } else {
      sx = (int)(((int64_t)E.A[2] + (int64_t)y * (int64_t)E.A[1] + (int64_t)x * (int64_t)E.A[0]) >> 16);
      sy = (int)(((int64_t)E.A[5] + (int64_t)y * (int64_t)E.A[4] + (int64_t)x * (int64_t)E.A[3]) >> 16);
    }
    if (sx < 0 || sx >= sw || sy < 0 || sy >= sh) return false;
#pragma unroll
    for (int k = 0; k < 3; k++) V[k] = warp_src(src, sw, sx, sy, k);
    return true;
  }
  double xin, yin;
  if (!warp_map_pixel(E, c, x, y, xin, yin)) return false;
  warp_sample<FILTER>(src, sw, sh, xin, yin, V);
  return true;
}

// The store path of a 4-pixel group of output row y from column x0 (npx of them inside the row); v[k][i]: the element of channel k of pixel x0 + i.
// Vector stores where the group is whole and its destination aligned to them, element stores otherwise - store_tensor4's rule.
template <int DT>
__device__ __forceinline__ void warp_store4(uint8_t* o0, const WarpCall& c, int x0, int y, int npx, const uint32_t (&v)[3][4])
{
  typedef typename TensorElem<DT>::T E;
  typedef TensorQuad<DT> Q;
  typedef typename Q::V V;
  const size_t ow = (size_t)c.ow, plane = (size_t)c.oh * ow;
  HIPDEC_GLOBAL E* o = (HIPDEC_GLOBAL E*)o0;
  if (c.nhwc) {
    HIPDEC_GLOBAL E* d = o + ((size_t)y * ow + (size_t)x0) * 3;
    if (npx == 4 && (((uintptr_t)d) & (4 * sizeof(E) - 1)) == 0) {
      ((HIPDEC_GLOBAL V*)d)[0] = Q::pack(v[0][0], v[1][0], v[2][0], v[0][1]);
      ((HIPDEC_GLOBAL V*)d)[1] = Q::pack(v[1][1], v[2][1], v[0][2], v[1][2]);
      ((HIPDEC_GLOBAL V*)d)[2] = Q::pack(v[2][2], v[0][3], v[1][3], v[2][3]);
      return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (i >= npx) break;
      d[3 * i] = (E)v[0][i]; d[3 * i + 1] = (E)v[1][i]; d[3 * i + 2] = (E)v[2][i];
    }
    return;
  }
  HIPDEC_GLOBAL E* r = o + (size_t)y * ow + (size_t)x0;
  HIPDEC_GLOBAL E* g = r + plane;
  HIPDEC_GLOBAL E* b = g + plane;
  if (npx == 4 && ((((uintptr_t)r) | ((uintptr_t)g) | ((uintptr_t)b)) & (4 * sizeof(E) - 1)) == 0) {
    *(HIPDEC_GLOBAL V*)r = Q::pack(v[0][0], v[0][1], v[0][2], v[0][3]);
    *(HIPDEC_GLOBAL V*)g = Q::pack(v[1][0], v[1][1], v[1][2], v[1][3]);
    *(HIPDEC_GLOBAL V*)b = Q::pack(v[2][0], v[2][1], v[2][2], v[2][3]);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i >= npx) break;
    r[i] = (E)v[0][i]; g[i] = (E)v[1][i]; b[i] = (E)v[2][i];
  }
}

template <int DT, int FILTER>
__device__ __forceinline__ void warp_tile(const hipdec::WarpEntry* __restrict__ tab, const WarpCall& c)
{
  const uint32_t entry = blockIdx.x / c.tiles, t = blockIdx.x - entry * c.tiles;
  const uint32_t ty = t / c.tiles_x, tx = t - ty * c.tiles_x;
  const int x0 = (int)tx * kWarpTC + (int)(threadIdx.x & 15u) * 4, y = (int)ty * kWarpTR + (int)(threadIdx.x >> 4);
  if (y >= c.oh || x0 >= c.ow) return;
  const hipdec::WarpEntry E = warp_entry_load(tab, entry);   // uniform: SGPRs
  const int npx = c.ow - x0 < 4 ? c.ow - x0 : 4;
  uint32_t f[3];
#pragma unroll
  for (int k = 0; k < 3; k++) f[k] = warp_fill_elem<DT>(E.domain, E.value[k], c.scale[k], c.bias[k]);
  uint32_t v[3][4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    int V[3] = {0, 0, 0};
    const bool in = i < npx && warp_pixel<FILTER>(E, c, x0 + i, y, V);
#pragma unroll
    for (int k = 0; k < 3; k++) v[k][i] = in ? tensor_elem<DT>(V[k], c.scale[k], c.bias[k]) : f[k];
  }
  warp_store4<DT>(E.o0, c, x0, y, npx, v);
}

template <int DT>
__global__ __launch_bounds__(256) void k_warp_nearest(const hipdec::WarpEntry* __restrict__ tab, const WarpCall c) { warp_tile<DT, HIPDEC_SCALE_NEAREST>(tab, c); }
template <int DT>
__global__ __launch_bounds__(256) void k_warp_bilinear(const hipdec::WarpEntry* __restrict__ tab, const WarpCall c) { warp_tile<DT, HIPDEC_SCALE_BILINEAR>(tab, c); }
template <int DT>
__global__ __launch_bounds__(256) void k_warp_bicubic(const hipdec::WarpEntry* __restrict__ tab, const WarpCall c) { warp_tile<DT, HIPDEC_SCALE_BICUBIC>(tab, c); }
