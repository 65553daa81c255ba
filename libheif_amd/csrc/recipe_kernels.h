// recipe_kernels.h — the affine step of a recipe chain (include/heif_hipdec.h, hipdec_tensor_recipe): PIL.Image.transform((w, h), AFFINE, data, resample,
// fillcolor) of the 8-bit result of the step before, bit for bit, as one more kind of step beside the photo and augment kernels.  Included by color.hip
// inside its kernel namespace, behind warp_kernels.h (WarpCall, warp_word, warp_pixel, warp_store4, kWarpTC, kWarpTR) and augment_kernels.h.
// Shape: k_warp_*'s.  A workgroup of 256 threads owns a tile of kWarpTC x kWarpTR pixels of one entry of the step's compacted table; the entry's record is
// a hipdec::WarpEntry whose `reserved` word carries the `last` flag - uniform per workgroup, through the constant address space, scalar loads into SGPRs.
// A lane owns four consecutive pixels of a row and computes each with warp_pixel<FILTER> itself: the arithmetic is stated once, in warp_kernels.h.
// A step that is not the entry's last stores U8 / NHWC into the other ping-pong buffer, the fill and the values unscaled; the last step stores the call's
// dtype and layout through tensor_elem<DT>, the fill normalised as a pixel is (the component domain: an 8-bit intermediate holds no element-domain fill).
// The source and the output have the same size (the stage does not resize): c.sw x c.sh == c.ow x c.oh.  No LDS.

// the record with its `last` flag: word 15 is value[2] and, in its upper half, `reserved`
__device__ __forceinline__ hipdec::WarpEntry recipe_entry_load(const hipdec::WarpEntry* p, uint32_t entry)
{
  hipdec::WarpEntry E = warp_entry_load(p, entry);
  E.reserved = (int32_t)(uint32_t)(warp_word(p, entry, 15) >> 32);
  return E;
}

template <int DT, int FILTER>
__device__ __forceinline__ void recipe_affine_tile(const hipdec::WarpEntry* __restrict__ tab, const WarpCall& c)
{
  const uint32_t entry = blockIdx.x / c.tiles, t = blockIdx.x - entry * c.tiles;
  const uint32_t ty = t / c.tiles_x, tx = t - ty * c.tiles_x;
  const int x0 = (int)tx * kWarpTC + (int)(threadIdx.x & 15u) * 4, y = (int)ty * kWarpTR + (int)(threadIdx.x >> 4);
  if (y >= c.oh || x0 >= c.ow) return;
  const hipdec::WarpEntry E = recipe_entry_load(tab, entry);   // uniform: SGPRs; the branch on `last` below is taken by the whole workgroup
  const bool last = E.reserved != 0;
  const int npx = c.ow - x0 < 4 ? c.ow - x0 : 4;
  int V[4][3];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    int P[3] = {0, 0, 0};
    const bool in = i < npx && warp_pixel<FILTER>(E, c, x0 + i, y, P);
#pragma unroll
    for (int k = 0; k < 3; k++) V[i][k] = in ? P[k] : (int)E.value[k];   // the fill is a component value: checked to be an integer 0 .. 255
  }
  uint32_t v[3][4];
  if (DT == TD_U8 || !last) {   // 8-bit samples either way; the intermediate is NHWC whatever the call's layout
    WarpCall wc = c;
    wc.nhwc = last ? c.nhwc : 1;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) v[k][i] = (uint32_t)V[i][k];
    warp_store4<TD_U8>(E.o0, wc, x0, y, npx, v);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) v[k][i] = tensor_elem<DT>(V[i][k], c.scale[k], c.bias[k]);
    warp_store4<DT>(E.o0, c, x0, y, npx, v);
  }
}

template <int DT>
__global__ __launch_bounds__(256) void k_recipe_affine_nearest(const hipdec::WarpEntry* __restrict__ tab, const WarpCall c)
{
  recipe_affine_tile<DT, HIPDEC_SCALE_NEAREST>(tab, c);
}
template <int DT>
__global__ __launch_bounds__(256) void k_recipe_affine_bilinear(const hipdec::WarpEntry* __restrict__ tab, const WarpCall c)
{
  recipe_affine_tile<DT, HIPDEC_SCALE_BILINEAR>(tab, c);
}
template <int DT>
__global__ __launch_bounds__(256) void k_recipe_affine_bicubic(const hipdec::WarpEntry* __restrict__ tab, const WarpCall c)
{
  recipe_affine_tile<DT, HIPDEC_SCALE_BICUBIC>(tab, c);
}
