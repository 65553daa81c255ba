// photo_kernels.h — the photometric stage of the tensor output (include/heif_hipdec.h, hipdec_tensor_photo): ImageEnhance.Brightness / Color / Contrast /
// Sharpness and ImageOps.posterize / solarize / invert / autocontrast / equalize of dense 8-bit interleaved RGB samples, bit for bit, chained, into the
// normalised tensor.  Included by color.hip inside its kernel namespace, behind the tensor store helpers and warp_kernels.h (warp_store4, kWarpTC, kWarpTR).
// Shape: per chain step at most one launch of k_photo_hist and one of k_photo_apply, for all entries that have that step.
//   k_photo_hist   a workgroup of 256 threads owns kPhotoHistRows rows of one entry.  It counts R, G, B and LUM of its pixels into LDS histograms with
//                  integer atomicAdd - one copy per wave, so that a flat picture's single bin is contended by 64 lanes, not 256 - and adds its non-zero
//                  bins into the entry's 4 x 256 uint32 histogram in global memory (zeroed by a hipMemsetAsync in front).  Integer sums: the result does
//                  not depend on scheduling.
//   k_photo_apply  a workgroup owns a tile of kWarpTC x kWarpTR pixels of one entry, a lane four consecutive pixels of a row, as in k_warp.  The prologue
//                  turns the step's operation into LDS parameters: every operation but COLOR and SHARPNESS is a 256-entry table per channel - thread v
//                  computes entry v with the functions of photo_lut.h, after a 256-bin prefix sum (EQUALIZE, AUTOCONTRAST: also the first and last
//                  non-zero bin) or a weighted sum (CONTRAST) of the entry's histogram -, COLOR blends with the pixel's own LUM, SHARPNESS stages the
//                  tile and a one-pixel halo.  An intermediate step stores U8 / NHWC into the other ping-pong buffer (never in place: SHARPNESS reads
//                  its neighbours); the entry's last step stores the normalised tensor through tensor_elem<DT> and warp_store4.
// The entry's record (hipdec::PhotoEntry) is uniform per workgroup and comes through the constant address space: scalar loads into SGPRs.
// Arithmetic: photo_lut.h; single and double precision, one rounding per written operation (-ffp-contract=off - the definition depends on it).
// LDS: k_photo_hist 16 KiB; k_photo_apply 6 KiB scan + 2 KiB sum + 768 B tables + 3564 B tile + 36 B = 12.3 KiB.

constexpr int kPhotoHistRows = 64;                        // rows of a sample per k_photo_hist workgroup
constexpr int kPhotoHaloC = kWarpTC + 2, kPhotoHaloR = kWarpTR + 2;

struct PhotoCall {
  int w, h;
  int nhwc;
  uint32_t tiles_x, tiles;   // k_photo_apply: tiles across, tiles per entry
  uint32_t slices;           // k_photo_hist: workgroups per entry
  float scale[3], bias[3];
};

__device__ __forceinline__ hipdec::PhotoEntry photo_entry_load(const hipdec::PhotoEntry* p, uint32_t entry)
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
  hipdec::PhotoEntry E;
  E.src = (const uint8_t*)(uintptr_t)w[0]; E.dst = (uint8_t*)(uintptr_t)w[1]; E.hist = (uint32_t*)(uintptr_t)w[2];
  E.value = __builtin_bit_cast(double, w[3]);
  E.op = (int32_t)(uint32_t)w[4]; E.last = (int32_t)(uint32_t)(w[4] >> 32);
  E.reserved[0] = E.reserved[1] = E.reserved[2] = 0;
  return E;
}

__device__ __forceinline__ void photo_count(uint32_t (*mine)[256], int R, int G, int B)
{
  atomicAdd(&mine[0][R], 1u);
  atomicAdd(&mine[1][G], 1u);
  atomicAdd(&mine[2][B], 1u);
  atomicAdd(&mine[3][hipdec::photo_lum(R, G, B)], 1u);
}

__global__ __launch_bounds__(256) void k_photo_hist(const hipdec::PhotoEntry* __restrict__ tab, const PhotoCall c)
{
  __shared__ uint32_t s_h[4][4][256];   // [wave][R, G, B, LUM][bin]
  const uint32_t entry = blockIdx.x / c.slices, slice = blockIdx.x - entry * c.slices;
  const int tid = (int)threadIdx.x;
  const hipdec::PhotoEntry E = photo_entry_load(tab, entry);   // uniform: SGPRs
  uint32_t* flat = &s_h[0][0][0];
  for (int i = tid; i < 4 * 4 * 256; i += 256) flat[i] = 0;
  __syncthreads();
  // the slice's rows are contiguous bytes of the dense sample
  const int y0 = (int)slice * kPhotoHistRows, y1 = y0 + kPhotoHistRows < c.h ? y0 + kPhotoHistRows : c.h;
  const size_t count = (size_t)(y1 - y0) * (size_t)c.w;
  const HIPDEC_GLOBAL uint8_t* src = (const HIPDEC_GLOBAL uint8_t*)E.src + (size_t)y0 * (size_t)c.w * 3;
  uint32_t (*mine)[256] = s_h[tid >> 6];
  size_t done = 0;
  if ((((uintptr_t)src) & 3) == 0) {     // four pixels as three 4-byte loads
    const size_t groups = count / 4;
    const HIPDEC_GLOBAL uint32_t* s4 = (const HIPDEC_GLOBAL uint32_t*)src;
    for (size_t g = (size_t)tid; g < groups; g += 256) {
      const uint32_t a = s4[3 * g], b = s4[3 * g + 1], d = s4[3 * g + 2];
      photo_count(mine, (int)(a & 255u), (int)((a >> 8) & 255u), (int)((a >> 16) & 255u));
      photo_count(mine, (int)(a >> 24), (int)(b & 255u), (int)((b >> 8) & 255u));
      photo_count(mine, (int)((b >> 16) & 255u), (int)(b >> 24), (int)(d & 255u));
      photo_count(mine, (int)((d >> 8) & 255u), (int)((d >> 16) & 255u), (int)(d >> 24));
    }
    done = groups * 4;
  }
  for (size_t p = done + (size_t)tid; p < count; p += 256) photo_count(mine, (int)src[3 * p], (int)src[3 * p + 1], (int)src[3 * p + 2]);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t v = s_h[0][k][tid] + s_h[1][k][tid] + s_h[2][k][tid] + s_h[3][k][tid];
    if (v) atomicAdd(E.hist + k * 256 + tid, v);
  }
}

// (uint8)clip(0.5f + row(y - 1) + row(y) + row(y + 1)) of ImageFilter.SMOOTH, the top row first; t: the staged tile, (r, col) the pixel's place in it
__device__ __forceinline__ int photo_smooth(const uint8_t (*t)[kPhotoHaloC * 3], int r, int col, int k)
{
  const float w = (float)(1.0 / 13), wc = (float)(5.0 / 13);
  float ss = 0.5f;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++) {
    const uint8_t* row = t[r + dy];
    ss += ((float)row[(col - 1) * 3 + k] * w + (float)row[col * 3 + k] * (dy == 0 ? wc : w)) + (float)row[(col + 1) * 3 + k] * w;
  }
  return ss <= 0.0f ? 0 : (ss >= 255.0f ? 255 : (int)ss);
}

template <int DT>
__global__ __launch_bounds__(256) void k_photo_apply(const hipdec::PhotoEntry* __restrict__ tab, const PhotoCall c)
{
  __shared__ uint32_t s_scan[2][3][256];
  __shared__ unsigned long long s_sum[256];
  __shared__ uint8_t s_lut[3][256];
  __shared__ uint8_t s_tile[kPhotoHaloR][kPhotoHaloC * 3];
  __shared__ int s_lo[3], s_hi[3];
  __shared__ uint32_t s_last[3];
  const uint32_t entry = blockIdx.x / c.tiles, t = blockIdx.x - entry * c.tiles;
  const uint32_t ty = t / c.tiles_x, tx = t - ty * c.tiles_x;
  const int tid = (int)threadIdx.x;
  const hipdec::PhotoEntry E = photo_entry_load(tab, entry);   // uniform: SGPRs; every branch on E.op below is taken by the whole workgroup
  const HIPDEC_GLOBAL uint8_t* src = (const HIPDEC_GLOBAL uint8_t*)E.src;
  const int op = E.op, w = c.w, h = c.h;
  const float alpha = (float)E.value;

  // ---- the prologue: the step's parameters in LDS
  if (op == hipdec::PHOTO_SHARPNESS) {
    const int tx0 = (int)tx * kWarpTC - 1, ty0 = (int)ty * kWarpTR - 1;
    for (int i = tid; i < kPhotoHaloR * kPhotoHaloC; i += 256) {
      const int r = i / kPhotoHaloC, cc = i - r * kPhotoHaloC;
      const int yy = clip_i(ty0 + r, h - 1), xx = clip_i(tx0 + cc, w - 1);   // (what a clamp duplicates is read by border pixels only, which do not use it)
      const HIPDEC_GLOBAL uint8_t* p = src + ((size_t)yy * (size_t)w + (size_t)xx) * 3;
      s_tile[r][cc * 3] = p[0]; s_tile[r][cc * 3 + 1] = p[1]; s_tile[r][cc * 3 + 2] = p[2];
    }
  } else if (op == hipdec::PHOTO_CONTRAST) {
    const HIPDEC_GLOBAL uint32_t* H = (const HIPDEC_GLOBAL uint32_t*)E.hist;
    s_sum[tid] = (unsigned long long)tid * (unsigned long long)H[3 * 256 + tid];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) s_sum[tid] += s_sum[tid + off];
      __syncthreads();
    }
    const int m = hipdec::photo_contrast_mean((uint64_t)s_sum[0], (uint64_t)w * (uint64_t)h);
    const uint8_t v = (uint8_t)hipdec::photo_blend(m, tid, alpha);
    s_lut[0][tid] = v; s_lut[1][tid] = v; s_lut[2][tid] = v;
  } else if (op == hipdec::PHOTO_AUTOCONTRAST || op == hipdec::PHOTO_EQUALIZE) {
    const HIPDEC_GLOBAL uint32_t* H = (const HIPDEC_GLOBAL uint32_t*)E.hist;
    uint32_t own[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { own[k] = H[k * 256 + tid]; s_scan[0][k][tid] = own[k]; }
    __syncthreads();
    int b = 0;
    for (int off = 1; off < 256; off <<= 1) {        // inclusive prefix sums of the three channels, eight doubling steps between two buffers
#pragma unroll
      for (int k = 0; k < 3; k++) s_scan[b ^ 1][k][tid] = s_scan[b][k][tid] + (tid >= off ? s_scan[b][k][tid - off] : 0u);
      b ^= 1;
      __syncthreads();
    }
    uint32_t before[3], total[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const uint32_t incl = s_scan[b][k][tid];
      total[k] = s_scan[b][k][255];                  // w * h
      before[k] = incl - own[k];
      if (own[k] && before[k] == 0) s_lo[k] = tid;   // exactly one thread each: the first and the last non-zero bin
      if (own[k] && incl == total[k]) { s_hi[k] = tid; s_last[k] = own[k]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; k++)
      s_lut[k][tid] = (uint8_t)(op == hipdec::PHOTO_AUTOCONTRAST ? hipdec::photo_autocontrast(tid, s_lo[k], s_hi[k])
                                                                 : hipdec::photo_equalize(tid, before[k], total[k], s_last[k], s_lo[k], s_hi[k]));
  } else if (op != hipdec::PHOTO_COLOR) {
    const uint8_t v = (uint8_t)hipdec::photo_point(op, E.value, tid);
    s_lut[0][tid] = v; s_lut[1][tid] = v; s_lut[2][tid] = v;
  }
  __syncthreads();

  // ---- four pixels of a row per lane
  const int lx = (int)(threadIdx.x & 15u) * 4, ly = (int)(threadIdx.x >> 4);
  const int x0 = (int)tx * kWarpTC + lx, y = (int)ty * kWarpTR + ly;
  if (y >= h || x0 >= w) return;
  const int npx = w - x0 < 4 ? w - x0 : 4;
  int P[4][3];
#pragma unroll
  for (int i = 0; i < 4; i++) P[i][0] = P[i][1] = P[i][2] = 0;
  if (op == hipdec::PHOTO_SHARPNESS) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) P[i][k] = (int)s_tile[ly + 1][(lx + 1 + i) * 3 + k];   // (columns past the row's end hold clamped copies, not stored)
  } else {
    const HIPDEC_GLOBAL uint8_t* p = src + ((size_t)y * (size_t)w + (size_t)x0) * 3;
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
  }
  int V[4][3];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (op == hipdec::PHOTO_COLOR) {
      const int L = hipdec::photo_lum(P[i][0], P[i][1], P[i][2]);
#pragma unroll
      for (int k = 0; k < 3; k++) V[i][k] = hipdec::photo_blend(L, P[i][k], alpha);
    } else if (op == hipdec::PHOTO_SHARPNESS) {
      const int x = x0 + i;
      const bool border = x <= 0 || y <= 0 || x >= w - 1 || y >= h - 1;   // the first and last row and column are the source's
#pragma unroll
      for (int k = 0; k < 3; k++) V[i][k] = border ? P[i][k] : hipdec::photo_blend(photo_smooth(s_tile, ly + 1, lx + 1 + i, k), P[i][k], alpha);
    } else {
#pragma unroll
      for (int k = 0; k < 3; k++) V[i][k] = (int)s_lut[k][P[i][k]];
    }
  }
  WarpCall wc;
  wc.ow = w; wc.oh = h; wc.nhwc = E.last ? c.nhwc : 1;
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
