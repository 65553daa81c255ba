// augment_kernels.h — the two kernels the augment stage (include/heif_hipdec.h, hipdec_tensor_augment) adds to the photo stage's: Pillow's hue shift and
// ImageFilter.GaussianBlur of dense 8-bit interleaved RGB samples, bit for bit, as steps of a chain.  Included by color.hip inside its kernel namespace,
// behind photo_kernels.h (PhotoCall, warp_store4, kWarpTC, kWarpTR).  Per chain step at most one launch of each, over the compacted table of the entries
// whose operation at that step is of its kind.
//   k_augment_hue   k_photo_apply's shape: a workgroup owns a tile of kWarpTC x kWarpTR pixels of one entry, a lane four consecutive pixels of a row, 12-byte
//                   loads where aligned.  Point-wise (augment_lut.h augment_hue): no LDS.
//   k_augment_blur  all six box passes of a step in ONE launch, no 8-bit intermediate in HBM between them.  A workgroup of 256 threads owns a tile of
//                   kBlurTC x kBlurTR pixels.  It stages the tile and a halo of 3 (r + 1) pixels on every side - clipped to the picture, its columns
//                   widened to multiples of four so that rows are staged as dwords - into LDS as interleaved bytes, rows `pitch` bytes apart with an odd
//                   dword count.  Three horizontal passes run over every staged row, one thread per (row, channel) with a running window sum; three
//                   vertical passes over the tile's own columns, one thread per (column, channel); two LDS buffers in turn.  A pass clamps at the bounds
//                   of the STAGED region: where that is the picture's edge this is Pillow's clamp; where it is a tile cut the samples it spoils lie
//                   within j (r + 1) of the cut after j passes, and the tile is 3 (r + 1) away.  RMAX - 1, 3 or 7, chosen from the call's largest r -
//                   sizes the LDS; entries of one launch have their own r, ww, fw in their records.
// An intermediate step stores U8 / NHWC into the other ping-pong buffer; the entry's last step stores the normalised tensor through tensor_elem<DT> and
// warp_store4.  The entry's record (hipdec::AugmentEntry) is uniform per workgroup and comes through the constant address space.
// LDS: k_augment_hue none; k_augment_blur 2 x rows x pitch: RMAX 1: 2 x 44 x 244 = 21472 B, RMAX 3: 2 x 56 x 268 = 30016 B, RMAX 7: 2 x 80 x 340 = 54400 B.

constexpr int kBlurTC = 64, kBlurTR = 32;   // the blur tile

// the staged region of a tile for boxes of whole radius up to RMAX
template <int RMAX>
struct BlurStage {
  static constexpr int kHalo = 3 * (RMAX + 1);
  static constexpr int kCols = kBlurTC + 2 * ((kHalo + 3) & ~3), kRows = kBlurTR + 2 * kHalo;
  static constexpr int kDwords = (kCols * 3 + 3) / 4, kPitch = 4 * (kDwords | 1);
};

struct BlurCall {
  PhotoCall p;
  uint32_t tiles_x, tiles;   // blur tiles across, blur tiles per entry
};

__device__ __forceinline__ hipdec::AugmentEntry augment_entry_load(const hipdec::AugmentEntry* p, uint32_t entry)
{
  uint64_t w[5];
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const uint64_t* q = (const uint64_t*)(p + entry) + i;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(HIPDEC_HOST_EMU)
    w[i] = *(const __attribute__((address_space(4))) uint64_t*)(uintptr_t)q;
#else
    w[i] = *q;
#endif
  }
  hipdec::AugmentEntry E;
  E.src = (const uint8_t*)(uintptr_t)w[0]; E.dst = (uint8_t*)(uintptr_t)w[1];
  E.op = (int32_t)(uint32_t)w[2]; E.last = (int32_t)(uint32_t)(w[2] >> 32);
  E.shift = (int32_t)(uint32_t)w[3]; E.r = (int32_t)(uint32_t)(w[3] >> 32);
  E.ww = (uint32_t)w[4]; E.fw = (uint32_t)(w[4] >> 32);
  E.reserved[0] = E.reserved[1] = E.reserved[2] = 0;
  return E;
}

// the store of four pixels V[i][k] of row y from column x0: the tensor (last) or the U8 / NHWC sample of the next step
template <int DT>
__device__ __forceinline__ void augment_store4(const hipdec::AugmentEntry& E, const PhotoCall& c, int x0, int y, int npx, const int (&V)[4][3])
{
  WarpCall wc;
  wc.ow = c.w; wc.oh = c.h; wc.nhwc = E.last ? c.nhwc : 1;
  uint32_t v[3][4];
  if (E.last) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) v[k][i] = tensor_elem<DT>(V[i][k], c.scale[k], c.bias[k]);
    warp_store4<DT>(E.dst, wc, x0, y, npx, v);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) v[k][i] = (uint32_t)V[i][k];
    warp_store4<TD_U8>(E.dst, wc, x0, y, npx, v);
  }
}

template <int DT>
__global__ __launch_bounds__(256) void k_augment_hue(const hipdec::AugmentEntry* __restrict__ tab, const PhotoCall c)
{
  const uint32_t entry = blockIdx.x / c.tiles, t = blockIdx.x - entry * c.tiles;
  const uint32_t ty = t / c.tiles_x, tx = t - ty * c.tiles_x;
  const hipdec::AugmentEntry E = augment_entry_load(tab, entry);   // uniform: SGPRs
  const int w = c.w, h = c.h;
  const int x0 = (int)tx * kWarpTC + (int)(threadIdx.x & 15u) * 4, y = (int)ty * kWarpTR + (int)(threadIdx.x >> 4);
  if (y >= h || x0 >= w) return;
  const int npx = w - x0 < 4 ? w - x0 : 4;
  const HIPDEC_GLOBAL uint8_t* p = (const HIPDEC_GLOBAL uint8_t*)E.src + ((size_t)y * (size_t)w + (size_t)x0) * 3;
  int P[4][3];
#pragma unroll
  for (int i = 0; i < 4; i++) P[i][0] = P[i][1] = P[i][2] = 0;
  if (npx == 4 && (((uintptr_t)p) & 3) == 0) {
    const HIPDEC_GLOBAL uint32_t* p4 = (const HIPDEC_GLOBAL uint32_t*)p;
    const uint32_t wd[3] = {p4[0], p4[1], p4[2]};
#pragma unroll
    for (int j = 0; j < 12; j++) P[j / 3][j % 3] = (int)((wd[j >> 2] >> (8 * (j & 3))) & 255u);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (i >= npx) break;
      P[i][0] = (int)p[3 * i]; P[i][1] = (int)p[3 * i + 1]; P[i][2] = (int)p[3 * i + 2];
    }
  }
  int V[4][3];
#pragma unroll
  for (int i = 0; i < 4; i++) hipdec::augment_hue(E.shift, P[i][0], P[i][1], P[i][2], &V[i][0], &V[i][1], &V[i][2]);
  augment_store4<DT>(E, c, x0, y, npx, V);
}

template <int DT, int RMAX>
__global__ __launch_bounds__(256) void k_augment_blur(const hipdec::AugmentEntry* __restrict__ tab, const BlurCall bc)
{
  typedef BlurStage<RMAX> St;
  constexpr int kPitch = St::kPitch;
  __shared__ __attribute__((aligned(16))) uint8_t s_a[St::kRows * kPitch];
  __shared__ __attribute__((aligned(16))) uint8_t s_b[St::kRows * kPitch];
  const PhotoCall& c = bc.p;
  const uint32_t entry = blockIdx.x / bc.tiles, t = blockIdx.x - entry * bc.tiles;
  const uint32_t ty = t / bc.tiles_x, tx = t - ty * bc.tiles_x;
  const int tid = (int)threadIdx.x;
  const hipdec::AugmentEntry E = augment_entry_load(tab, entry);   // uniform: SGPRs
  const HIPDEC_GLOBAL uint8_t* src = (const HIPDEC_GLOBAL uint8_t*)E.src;
  const int w = c.w, h = c.h;
  const int r = E.r < RMAX ? E.r : RMAX;                            // (the host chose RMAX >= every r of the launch)
  const int halo = 3 * (r + 1);
  // the staged region, clipped to the picture; its columns [sx0, sx1) widened to multiples of four (or the row's end)
  const int tx0 = (int)tx * kBlurTC, ty0 = (int)ty * kBlurTR;
  const int tw = w - tx0 < kBlurTC ? w - tx0 : kBlurTC, th = h - ty0 < kBlurTR ? h - ty0 : kBlurTR;
  const int sx0 = (tx0 - halo < 0 ? 0 : tx0 - halo) & ~3;
  const int sx1r = (tx0 + tw + halo + 3) & ~3, sx1 = sx1r > w ? w : sx1r;
  const int sy0 = ty0 - halo < 0 ? 0 : ty0 - halo, sy1 = ty0 + th + halo > h ? h : ty0 + th + halo;
  const int sw = sx1 - sx0, sh = sy1 - sy0, row_bytes = sw * 3;     // sw <= St::kCols, sh <= St::kRows

  // ---- stage: rows of row_bytes bytes; as dwords where every staged row starts and ends on one
  if ((((uintptr_t)src) & 3) == 0 && (w & 3) == 0) {
    const int row_dw = row_bytes >> 2;
    for (int i = tid; i < sh * row_dw; i += 256) {
      const int rr = i / row_dw, cc = i - rr * row_dw;
      const HIPDEC_GLOBAL uint32_t* g = (const HIPDEC_GLOBAL uint32_t*)(src + ((size_t)(sy0 + rr) * (size_t)w + (size_t)sx0) * 3);
      *(uint32_t*)(s_a + rr * kPitch + cc * 4) = g[cc];
    }
  } else {
    for (int i = tid; i < sh * row_bytes; i += 256) {
      const int rr = i / row_bytes, cc = i - rr * row_bytes;
      s_a[rr * kPitch + cc] = src[((size_t)(sy0 + rr) * (size_t)w + (size_t)sx0) * 3 + (size_t)cc];
    }
  }
  __syncthreads();

  // ---- three horizontal passes over every staged row: a -> b -> a -> b
  {
    const int row = tid / 3, ch = tid - row * 3;
    const bool mine = row < sh;
    const int at = row * kPitch + ch;
    if (mine) hipdec::augment_box_line(s_a + at, s_b + at, sw, 3, r, E.ww, E.fw);
    __syncthreads();
    if (mine) hipdec::augment_box_line(s_b + at, s_a + at, sw, 3, r, E.ww, E.fw);
    __syncthreads();
    if (mine) hipdec::augment_box_line(s_a + at, s_b + at, sw, 3, r, E.ww, E.fw);
    __syncthreads();
  }
  // ---- three vertical passes over the tile's own columns: b -> a -> b -> a
  {
    const bool mine = tid < tw * 3;
    const int at = (tx0 - sx0) * 3 + tid;
    if (mine) hipdec::augment_box_line(s_b + at, s_a + at, sh, kPitch, r, E.ww, E.fw);
    __syncthreads();
    if (mine) hipdec::augment_box_line(s_a + at, s_b + at, sh, kPitch, r, E.ww, E.fw);
    __syncthreads();
    if (mine) hipdec::augment_box_line(s_b + at, s_a + at, sh, kPitch, r, E.ww, E.fw);
    __syncthreads();
  }

  // ---- store: four pixels of a row per lane, two groups per thread
  const int lx = (tid & 15) * 4;
#pragma unroll
  for (int half = 0; half < 2; half++) {
    const int ly = (tid >> 4) + half * 16;
    if (ly >= th || lx >= tw) continue;
    const int npx = tw - lx < 4 ? tw - lx : 4;
    const uint8_t* q = s_a + (ty0 - sy0 + ly) * kPitch + (tx0 - sx0 + lx) * 3;   // (a dword boundary: sx0, tx0 and lx are multiples of four)
    int V[4][3];
    if (npx == 4) {
      const uint32_t* q4 = (const uint32_t*)q;
      const uint32_t wd[3] = {q4[0], q4[1], q4[2]};
#pragma unroll
      for (int j = 0; j < 12; j++) V[j / 3][j % 3] = (int)((wd[j >> 2] >> (8 * (j & 3))) & 255u);
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) V[i][k] = i < npx ? (int)q[3 * i + k] : 0;
    }
    augment_store4<DT>(E, c, tx0 + lx, ty0 + ly, npx, V);
  }
}
