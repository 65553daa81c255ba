// CPU-test-only reader of the reconstruction plan's raw records (tests/test_recon_record_emu.py).  It includes no kernel source: after k_recon_plan has
// run on a parsed batch (recon_plan_probe.cc: emu_plan_run) it copies the four words of every record out of the arena as they are, so that the test can
// restate in Python what the third and fourth word and the upper half of the second must hold.  Compiled with the flags of tests/emu/Makefile (same
// layout of the batch object).
#include <stdint.h>
#include <string.h>
#include <vector>
#include "emu_batch.h"

using namespace hipdec;

extern "C" {

// The records of picture i, 6 words each: CTB (raster), list (0 luma, 1 the chroma pair), w0, w1, w2, w3 - CTB by CTB, luma list then chroma list.
// Returns their number, -1 when `cap` rows do not hold them, -2 for a count beyond its list's slots.
long emu_plan_records(EmuBatch* b, int i, uint32_t* dst, long cap)
{
  const PicParams& P = b->L.params[i];
  if (!P.off_plan_cnt) return 0;
  const uint8_t* a = b->arena.data();
  const int units = 1 << P.units_per_ctb_log2, nctb = P.ctb_w * P.ctb_h;
  std::vector<uint32_t> out;
  for (int c = 0; c < nctb; c++) {
    const PlanRecord* recs = (const PlanRecord*)(a + P.off_plan) + (size_t)c * (size_t)(units + units / 4);
    const uint32_t counts = ((const uint32_t*)(a + P.off_plan_cnt))[c];
    for (int list = 0; list < 2; list++) {
      const int count = (int)(list ? counts >> 16 : counts & 0xffffu), slots = list ? units / 4 : units;
      if (count > slots) return -2;
      const PlanRecord* r = recs + (list ? units : 0);
      for (int k = 0; k < count; k++) {
        const uint32_t row[6] = {(uint32_t)c, (uint32_t)list, r[k].w0, r[k].w1, r[k].w2, r[k].w3};
        out.insert(out.end(), row, row + 6);
      }
    }
  }
  if ((long)(out.size() / 6) > cap) return -1;
  if (!out.empty()) memcpy(dst, out.data(), out.size() * sizeof(uint32_t));
  return (long)(out.size() / 6);
}

// log2 of the CTB size of picture i (the tile offsets in the records are in rows of the CTB's width in component samples)
int emu_plan_log2_ctb(EmuBatch* b, int i) { return b->L.params[i].log2_ctb; }

}  // extern "C"
