// CPU-test-only access to the coefficient regions of an emulated batch (tests/test_parse_lds_window_emu.py): the parser stores a coded block's levels
// straight into the arena and zero-fills the sub-blocks it did not parse, so the test poisons the regions BEFORE the parse and afterwards asks which
// int16 words outside the coded blocks (and the PCM units' sample blocks) no longer hold the poison.  The words inside coded blocks are compared with
// the oracle through emu_coeffs() of libparse_emu*.so.  Built into a library of its own with the flags of tests/emu/Makefile.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "hevc_device.h"
#include "emu_batch.h"

using namespace hipdec;

static inline uint32_t c1by1(uint32_t v)
{
  v &= 0x55555555u; v = (v | (v >> 1)) & 0x33333333u; v = (v | (v >> 2)) & 0x0f0f0f0fu; v = (v | (v >> 4)) & 0x00ff00ffu;
  return v;
}
// int16 words of the coefficient region of component c of picture P
static size_t region_words(const PicParams& P, int c)
{
  const size_t ctb = (size_t)1 << P.log2_ctb;
  const int sh = c == 0 ? 0 : (P.chroma_format_idc == 3 ? 0 : (P.chroma_format_idc == 2 ? 1 : 2));
  if (c && !P.chroma_format_idc) return 0;
  return (size_t)P.ctb_w * P.ctb_h * ((ctb * ctb) >> sh);
}

extern "C" {

// fills the coefficient regions of picture i with `poison`; returns the int16 words written
long emu_poison_coeffs(EmuBatch* b, int i, int poison)
{
  const PicParams& P = b->L.params[i];
  long n = 0;
  for (int c = 0; c < 3; c++) {
    int16_t* p = (int16_t*)(b->arena.data() + P.off_coeff[c]);
    const size_t w = region_words(P, c);
    for (size_t k = 0; k < w; k++) p[k] = (int16_t)poison;
    n += (long)w;
  }
  return n;
}

// after the parse: out[0] = words inside coded blocks and PCM sample blocks, out[1] = words outside them that still hold the poison, out[2] = words
// outside them that do not (must be 0).  The walk over the published maps is emu_coeffs()'s: units outside the picture are never parsed, so
// nothing may be written for them.
int emu_coeffs_outside(EmuBatch* b, int i, int poison, long* out)
{
  const PicParams& P = b->L.params[i];
  const uint8_t* a = b->arena.data();
  const int ctb = 1 << P.log2_ctb, units = 1 << P.units_per_ctb_log2;
  const int cfi = P.chroma_format_idc;
  std::vector<uint8_t> cov[3];
  for (int c = 0; c < 3; c++) cov[c].assign(region_words(P, c), 0);
  for (int ctb_rs = 0; ctb_rs < P.ctb_w * P.ctb_h; ctb_rs++) {
    const size_t base = (size_t)ctb_rs * units;
    int z = 0;
    while (z < units) {
      const int ux = (int)c1by1((uint32_t)z), uy = (int)c1by1((uint32_t)z >> 1);
      if ((ctb_rs % P.ctb_w) * ctb + ux * 4 >= P.width || (ctb_rs / P.ctb_w) * ctb + uy * 4 >= P.height) { z++; continue; }   // outside the picture: never parsed
      const int t = a[P.off_u_size + base + z] & 15;
      if (t < 2 || t > 5) return -1;
      const int fl = a[P.off_u_flags + base + z];
      const bool pcm = (fl & UF_PCM) != 0;
      if ((fl & UF_CBF_LUMA) || pcm) {
        const size_t o = (size_t)ctb_rs * ctb * ctb + (size_t)z * 16;
        memset(&cov[0][o], 1, (size_t)1 << (2 * t));
      }
      if (cfi) {
        const bool c444 = cfi == 3;
        int do_c = 0, zc = z, tc = t - 1;
        if (c444) { do_c = 1; tc = t; }
        else if (t > 2) do_c = 1; else if ((z & 3) == 3) { do_c = 1; zc = z & ~3; tc = 2; }
        if (do_c) {
          const int mult = c444 ? 16 : (cfi == 2 ? 8 : 4), n2 = 1 << (2 * tc);
          const int sh = c444 ? 0 : (cfi == 2 ? 1 : 2);
          for (int c = 1; c < 3; c++)
            for (int low = 0; low < (cfi == 2 ? 2 : 1); low++) {
              const int f = low ? a[P.off_u_flags + base + (z ^ 1)] : fl;
              if (!(f & (c == 1 ? UF_CBF_CB : UF_CBF_CR)) && !pcm) continue;
              const size_t o = (size_t)ctb_rs * ((size_t)(ctb * ctb) >> sh) + (size_t)zc * mult + (size_t)low * n2;
              memset(&cov[c][o], 1, (size_t)n2);
            }
        }
      }
      z += 1 << (2 * (t - 2));
    }
  }
  out[0] = out[1] = out[2] = 0;
  for (int c = 0; c < 3; c++) {
    const int16_t* p = (const int16_t*)(a + P.off_coeff[c]);
    for (size_t k = 0; k < cov[c].size(); k++) {
      if (cov[c][k]) out[0]++;
      else if (p[k] == (int16_t)poison) out[1]++;
      else out[2]++;
    }
  }
  return 0;
}

}  // extern "C"
