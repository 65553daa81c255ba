// project_kernels.h — the projective stage of the tensor output (include/heif_hipdec.h, hipdec_tensor_project): PIL.Image.transform(size, PERSPECTIVE | QUAD,
// data, resample, fillcolor) of dense 8-bit interleaved RGB samples, bit for bit, into the normalised tensor.  Included by color.hip inside its kernel
// namespace, behind warp_kernels.h (WarpCall, warp_fill_elem, warp_inside, warp_sample, warp_src, warp_store4, kWarpTC, kWarpTR).
// Shape: k_warp_*'s.  ONE launch for all entries of a call; a workgroup of 256 threads owns a tile of kWarpTC x kWarpTR output pixels of one entry, a lane
// four consecutive pixels of a row.  The entry's record (hipdec::ProjectEntry: the eight doubles, the kind, the fill, the pointers) is uniform per workgroup
// and comes through the constant address space - scalar loads into SGPRs -, so the branch on `kind` is taken by the whole workgroup and the entries of a call
// may mix the two kinds.  The coordinate function is the only new arithmetic: IEEE double, no contraction (-ffp-contract=off), the PERSPECTIVE quotients by
// the plain division operator - no reciprocal, no builtin.  What follows (xin, yin) for BILINEAR / BICUBIC is warp_sample, the statement k_warp_* makes;
// NEAREST is Pillow's generic COORD path, not the affine call's fixed-point or table paths.  No LDS.

__device__ __forceinline__ hipdec::ProjectEntry project_entry_load(const hipdec::ProjectEntry* p, uint32_t entry)
{
  const uint64_t* q = (const uint64_t*)(p + entry);
  uint64_t w[13];   // (words 13 .. 15 of the record are padding)
#pragma unroll
  for (int i = 0; i < 13; i++) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HIPDEC_HOST_EMU)
    w[i] = *(const __attribute__((address_space(4))) uint64_t*)(uintptr_t)(q + i);
#else
    w[i] = q[i];
#endif
  }
  hipdec::ProjectEntry E;
  E.src = (const uint8_t*)(uintptr_t)w[0]; E.o0 = (uint8_t*)(uintptr_t)w[1];
#pragma unroll
  for (int i = 0; i < 8; i++) E.a[i] = __builtin_bit_cast(double, w[2 + i]);
  E.kind = (int32_t)(uint32_t)w[10]; E.domain = (int32_t)(uint32_t)(w[10] >> 32);
  E.value[0] = __builtin_bit_cast(float, (uint32_t)w[11]); E.value[1] = __builtin_bit_cast(float, (uint32_t)(w[11] >> 32));
  E.value[2] = __builtin_bit_cast(float, (uint32_t)w[12]); E.reserved = 0;
  E.pad[0] = E.pad[1] = E.pad[2] = 0;
  return E;
}

// xin, yin of output pixel (x, y): every written operator is one double operation, in this order
__device__ __forceinline__ void project_map_pixel(const hipdec::ProjectEntry& E, int x, int y, double& xin, double& yin)
{
  const double xc = (double)x + 0.5, yc = (double)y + 0.5;
  if (E.kind == hipdec::PROJECT_QUAD) {
    xin = E.a[0] + E.a[1] * xc + E.a[2] * yc + E.a[3] * xc * yc;
    yin = E.a[4] + E.a[5] * xc + E.a[6] * yc + E.a[7] * xc * yc;
  } else {
    xin = (E.a[0] * xc + E.a[1] * yc + E.a[2]) / (E.a[6] * xc + E.a[7] * yc + 1.0);
    yin = (E.a[3] * xc + E.a[4] * yc + E.a[5]) / (E.a[6] * xc + E.a[7] * yc + 1.0);
  }
}

// COORD(v) = -1 for v < 0, else (int)v
__device__ __forceinline__ int project_coord(double v) { return v < 0.0 ? -1 : (int)v; }

// FILTER: hipdec_scale_filter.  V[k]: the 8-bit component values of output pixel (x, y); false: the pixel is outside and holds the fill
template <int FILTER>
__device__ __forceinline__ bool project_pixel(const hipdec::ProjectEntry& E, const WarpCall& c, int x, int y, int (&V)[3])
{
  const HIPDEC_GLOBAL uint8_t* src = (const HIPDEC_GLOBAL uint8_t*)E.src;
  const int sw = c.sw, sh = c.sh;
  double xin, yin;
  project_map_pixel(E, x, y, xin, yin);
  if (FILTER == HIPDEC_SCALE_NEAREST) {
    const int sx = project_coord(xin), sy = project_coord(yin);
    if (sx < 0 || sx >= sw || sy < 0 || sy >= sh) return false;
#pragma unroll
    for (int k = 0; k < 3; k++) V[k] = warp_src(src, sw, sx, sy, k);
    return true;
  }
  if (!warp_inside(sw, sh, xin, yin)) return false;
  warp_sample<FILTER>(src, sw, sh, xin, yin, V);
  return true;
}

template <int DT, int FILTER>
__device__ __forceinline__ void project_tile(const hipdec::ProjectEntry* __restrict__ tab, const WarpCall& c)
{
  const uint32_t entry = blockIdx.x / c.tiles, t = blockIdx.x - entry * c.tiles;
  const uint32_t ty = t / c.tiles_x, tx = t - ty * c.tiles_x;
  const int x0 = (int)tx * kWarpTC + (int)(threadIdx.x & 15u) * 4, y = (int)ty * kWarpTR + (int)(threadIdx.x >> 4);
  if (y >= c.oh || x0 >= c.ow) return;
  const hipdec::ProjectEntry E = project_entry_load(tab, entry);   // uniform: SGPRs
  const int npx = c.ow - x0 < 4 ? c.ow - x0 : 4;
  uint32_t f[3];
#pragma unroll
  for (int k = 0; k < 3; k++) f[k] = warp_fill_elem<DT>(E.domain, E.value[k], c.scale[k], c.bias[k]);
  uint32_t v[3][4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    int V[3] = {0, 0, 0};
    const bool in = i < npx && project_pixel<FILTER>(E, c, x0 + i, y, V);
#pragma unroll
    for (int k = 0; k < 3; k++) v[k][i] = in ? tensor_elem<DT>(V[k], c.scale[k], c.bias[k]) : f[k];
  }
  warp_store4<DT>(E.o0, c, x0, y, npx, v);
}

template <int DT>
__global__ __launch_bounds__(256) void k_project_nearest(const hipdec::ProjectEntry* __restrict__ tab, const WarpCall c)
{
  project_tile<DT, HIPDEC_SCALE_NEAREST>(tab, c);
}
template <int DT>
__global__ __launch_bounds__(256) void k_project_bilinear(const hipdec::ProjectEntry* __restrict__ tab, const WarpCall c)
{
  project_tile<DT, HIPDEC_SCALE_BILINEAR>(tab, c);
}
template <int DT>
__global__ __launch_bounds__(256) void k_project_bicubic(const hipdec::ProjectEntry* __restrict__ tab, const WarpCall c)
{
  project_tile<DT, HIPDEC_SCALE_BICUBIC>(tab, c);
}
