// CPU-test-only probe of the reconstruction plan (tests/test_recon_plan_emu.py).  It compiles libheif_amd/csrc/recon_kernel.hip into a small library
// of its own (flags of tests/emu/Makefile), so that it can run k_recon_plan alone on a batch that libparse_emu.so has parsed and turn its records into
// lane masks with the kernel's own plan_mask() / plan_last() - and it restates, in plain sequential code, the front end the plan replaces: the unit
// words, the z-scan walk over them and the availability bitmap that every block reads per reference sample and marks when it is done.  The test
// compares the two block by block.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "emu_batch.h"
#include "../../libheif_amd/csrc/recon_kernel.hip"

using namespace hipdec;

namespace {

// one block as either path sees it: 8 words
//   [0] CTB (raster) | list << 32 (0 luma, 1 the chroma pair)   [1] x | y << 8 | log2 size << 16 (component samples inside the CTB)
//   [2] z index the residual is addressed with | mode << 16 | flags << 32
//   [3] reference samples are smoothed (size and mode; luma)   [4], [5] lane masks of the passes (scan order e = 64 j + lane; the chroma pair: e < 32 J in [4])
//   [6] the last sample of the top row where the block form handles it apart (else 1)   [7] 0
struct Row { uint64_t w[8]; };

void push(std::vector<Row>& out, int ctb, int list, int xb, int yb, int lg, int z, int mode, int fl, int smooth, uint64_t m0, uint64_t m1, int ax)
{
  Row r;
  r.w[0] = (uint64_t)ctb | ((uint64_t)list << 32); r.w[1] = (uint64_t)xb | ((uint64_t)yb << 8) | ((uint64_t)lg << 16);
  r.w[2] = (uint64_t)z | ((uint64_t)mode << 16) | ((uint64_t)fl << 32); r.w[3] = (uint64_t)smooth; r.w[4] = m0; r.w[5] = m1; r.w[6] = (uint64_t)ax; r.w[7] = 0;
  out.push_back(r);
}

ReconArgs recon_args(EmuBatch* b)
{
  uint8_t* a = b->arena.data();
  const BatchLayout& L = b->L;
  return ReconArgs{(const PicParams*)(a + L.off_pics), (const ReconWave*)(a + L.off_rwaves), L.num_rwaves, a,
                   (uint32_t*)(a + L.off_row_progress), (uint32_t*)(a + L.off_ticket) + 1, (int32_t*)(a + L.off_status)};
}

// the masks of one block as the block functions build them from a record's counts (reconstruct_block / _reg / _chroma_pair / _chroma_pair_reg4)
void plan_block_masks(const PlanAvail& V, int list, int lg, uint64_t& m0, uint64_t& m1, int& ax)
{
  const int n = 1 << lg;
  m0 = m1 = 0; ax = 1;
  if (list == 0) {
    if (lg <= 3) m0 = plan_mask(V, n, 0);
    else { m0 = plan_mask(V, n, 0); if (n == 32) m1 = plan_mask(V, n, 1); ax = plan_last(V, n); }
  } else if (lg == 2) m0 = (uint32_t)plan_mask(V, n, 0);
  else { m0 = plan_mask(V, n, 0) & (n == 16 ? ~0ull : 0xffffffffull); ax = plan_last(V, n); }
}

// ... and as the bitmap gives them: avrow[uy + 1] bit ux + 1 for the 4x4-luma units ux, uy in [-1, 2 * side); sh / shy: component samples -> units
void bitmap_block_masks(const uint64_t* avrow, int list, int xb, int yb, int lg, int sh, uint64_t& m0, uint64_t& m1, int& ax)
{
  const int n = 1 << lg, n2 = 2 * n, N = 4 * n + 1;
  auto at = [&](int X, int Y) -> int { return (int)((avrow[(Y >> sh) + 1] >> ((X >> sh) + 1)) & 1u); };
  auto sample = [&](int e) -> int { return e < n2 ? at(xb - 1, yb + n2 - 1 - e) : at(xb + e - n2 - 1, yb - 1); };
  m0 = m1 = 0; ax = 1;
  int passes_end;   // scan positions the lane passes cover
  if (list == 0) passes_end = lg <= 3 ? N : (n == 32 ? 128 : 64);
  else passes_end = lg == 2 ? N : (n == 16 ? 64 : 32);
  for (int e = 0; e < passes_end && e < N; e++)
    if (sample(e)) { if (e < 64) m0 |= 1ull << e; else m1 |= 1ull << (e - 64); }
  if (passes_end < N) ax = sample(N - 1);
}

}  // namespace

extern "C" {

// k_recon_plan alone on a parsed batch; returns the device status word
int emu_plan_run(EmuBatch* b)
{
  const ReconArgs ra = recon_args(b);
  if (ra.num_waves) hipLaunchKernelGGL(k_recon_plan, dim3(ra.num_waves), dim3(64), 0, nullptr, ra);
  return *(int32_t*)(b->arena.data() + b->L.off_status);
}
void emu_plan_clear_status(EmuBatch* b) { *(int32_t*)(b->arena.data() + b->L.off_status) = 0; }

// overwrite one byte of picture i's u_size map (a broken map for the plan kernel to refuse)
void emu_plan_poke_size(EmuBatch* b, int i, int ctb, int z, int value)
{
  const PicParams& P = b->L.params[i];
  b->arena[P.off_u_size + ((size_t)ctb << P.units_per_ctb_log2) + (size_t)z] = (uint8_t)value;
}

// fills the plan's region of picture i with a byte (so that what the kernel did not write is recognisable)
void emu_plan_fill(EmuBatch* b, int i, int value)
{
  const PicParams& P = b->L.params[i];
  const size_t nctb = (size_t)P.ctb_w * P.ctb_h, units = (size_t)1 << P.units_per_ctb_log2;
  if (!P.off_plan_cnt) return;
  memset(b->arena.data() + P.off_plan, value, nctb * (units + units / 4) * sizeof(PlanRecord));
  memset(b->arena.data() + P.off_plan_cnt, value, nctb * 4);
}

// The blocks of picture i from the plan (after emu_plan_run), 8 words each, CTB by CTB, luma list then chroma list.  Returns their number, -1 when `cap`
// rows do not hold them, -2 for a count beyond its list's slots, -3 for a record that leaves its CTB or carries an impossible size.
long emu_plan_blocks(EmuBatch* b, int i, uint64_t* dst, long cap)
{
  const PicParams& P = b->L.params[i];
  if (!P.off_plan_cnt) return 0;
  const uint8_t* a = b->arena.data();
  const int units = 1 << P.units_per_ctb_log2, nctb = P.ctb_w * P.ctb_h;
  std::vector<Row> out;
  for (int c = 0; c < nctb; c++) {
    const PlanRecord* recs = (const PlanRecord*)(a + P.off_plan) + (size_t)c * (size_t)(units + units / 4);
    const uint32_t counts = ((const uint32_t*)(a + P.off_plan_cnt))[c];
    for (int list = 0; list < 2; list++) {
      const int count = (int)(list ? counts >> 16 : counts & 0xffffu), slots = list ? units / 4 : units;
      if (count > slots) return -2;
      const PlanRecord* r = recs + (list ? units : 0);
      for (int k = 0; k < count; k++) {
        const uint32_t w0 = r[k].w0, w1 = r[k].w1;
        const int xb = (int)(w0 & 15u) << 2, yb = (int)((w0 >> 4) & 15u) << 2, lg = (int)((w0 >> 8) & 7u), z = (int)(w0 >> 24);
        const int ctbc = (1 << P.log2_ctb) >> list;
        if (lg < 2 || lg > 5 || xb + (1 << lg) > ctbc || yb + (1 << lg) > ctbc || z >= units) return -3;
        PlanAvail V;
        V.nl = (int)((w0 >> 12) & 31u); V.nt = (int)((w0 >> 17) & 31u); V.above = (int)((w0 >> 22) & 1u); V.corner = (int)((w0 >> 23) & 1u); V.smooth = (int)((w0 >> 11) & 1u);
        uint64_t m0, m1; int ax;
        plan_block_masks(V, list, lg, m0, m1, ax);
        push(out, c, list, xb, yb, lg, z, (int)(w1 & 255u), (int)((w1 >> 8) & 255u), V.smooth, m0, m1, ax);
      }
    }
  }
  if ((long)out.size() > cap) return -1;
  if (!out.empty()) memcpy(dst, out.data(), out.size() * sizeof(Row));
  return (long)out.size();
}

// The same blocks from the unit maps by the sequential front end: per CTB the border rows of the bitmap from CtbInfo::avail and the picture size, then the
// z-scan walk (units outside the picture skipped, the chroma pair's 4x4 blocks at a quad's fourth unit), every block reading the bitmap and then marking
// its own units.  Intra pictures with 4:0:0 / 4:2:0 sampling.  Returns the number of blocks, -1 when `cap` rows do not hold them, -4 for an impossible size.
long emu_bitmap_blocks(EmuBatch* b, int i, uint64_t* dst, long cap)
{
  const PicParams& P = b->L.params[i];
  const uint8_t* a = b->arena.data();
  const int units = 1 << P.units_per_ctb_log2, nctb = P.ctb_w * P.ctb_h, side = 1 << (P.log2_ctb - 2), ctb = 1 << P.log2_ctb;
  const CtbInfo* info = (const CtbInfo*)(a + P.off_ctb_info);
  std::vector<Row> out;
  for (int c = 0; c < nctb; c++) {
    const int cx = c % P.ctb_w, cy = c / P.ctb_w, x_ctb = cx * ctb, y_ctb = cy * ctb;
    const uint8_t* u_size = a + P.off_u_size + (size_t)c * units;
    const uint8_t* u_flags = a + P.off_u_flags + (size_t)c * units;
    for (int list = 0; list < (P.chroma_format_idc == 1 ? 2 : 1); list++) {
      const uint8_t* u_mode = a + (list ? P.off_u_ipmc : P.off_u_ipm) + (size_t)c * units;
      const int sub = list ? 2 : 1, sh = list ? 1 : 2;                      // component samples per luma sample; component samples -> units: >> sh
      const int Wc = list ? P.cwidth : P.width, Hc = list ? P.cheight : P.height, xc0 = x_ctb / sub, yc0 = y_ctb / sub, usz = 4 / sub;
      uint64_t avrow[33];
      memset(avrow, 0, sizeof(avrow));
      {
        int nu = (Wc - xc0 + usz - 1) / usz;
        nu = nu > 2 * side ? 2 * side : nu;
        const int n_up = nu < side ? nu : side;
        const uint8_t av = info[c].avail;
        if (av & AV_UPLEFT) avrow[0] |= 1ull;
        if (av & AV_UP) avrow[0] |= ((1ull << n_up) - 1ull) << 1;
        if ((av & AV_UPRIGHT) && nu > side) avrow[0] |= ((1ull << (nu - side)) - 1ull) << (side + 1);
        for (int r = 1; r <= side; r++) if ((av & AV_LEFT) && yc0 + (r - 1) * usz < Hc) avrow[r] = 1ull;
      }
      int z = 0;
      while (z < units) {
        const int ux = (int)compact1by1((uint32_t)z), uy = (int)compact1by1((uint32_t)z >> 1);
        if (x_ctb + ux * 4 >= P.width || y_ctb + uy * 4 >= P.height) { z++; continue; }
        const int tb = u_size[z] & 15;
        if (tb < 2 || tb > 5) return -4;
        if (list && tb == 2 && (z & 3) != 3) { z |= 3; continue; }
        int xb, yb, lg, zr;
        if (!list) { xb = ux * 4; yb = uy * 4; lg = tb; zr = z; }
        else { const int quad = tb == 2; xb = (quad ? (ux & ~1) : ux) * 2; yb = (quad ? (uy & ~1) : uy) * 2; lg = quad ? 2 : tb - 1; zr = quad ? (z & ~3) : z; }
        const int mode = list ? u_mode[z] : (u_mode[z] & 63), n = 1 << lg;
        int smooth = 0;
        if (!list && n != 4) {
          const int d1 = mode > 26 ? mode - 26 : 26 - mode, d2 = mode > 10 ? mode - 10 : 10 - mode, thres = n == 8 ? 7 : (n == 16 ? 1 : 0);
          smooth = mode != 1 && (d1 < d2 ? d1 : d2) > thres;
        }
        uint64_t m0, m1; int ax;
        bitmap_block_masks(avrow, list, xb, yb, lg, sh, m0, m1, ax);
        push(out, c, list, xb, yb, lg, zr, mode, u_flags[z], smooth, m0, m1, ax);
        const int k = n >> sh;   // units per side
        for (int r = 0; r < k; r++) avrow[(yb >> sh) + 1 + r] |= ((1ull << k) - 1ull) << ((xb >> sh) + 1);
        z += 1 << (2 * (tb - 2));
      }
    }
  }
  if ((long)out.size() > cap) return -1;
  if (!out.empty()) memcpy(dst, out.data(), out.size() * sizeof(Row));
  return (long)out.size();
}

}  // extern "C"
