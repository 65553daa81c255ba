// CPU-test-only reader of an emulated batch (tests/test_parse_unit_maps_lds.py): the five unit maps of picture i as the parser published them -
// CTBs in raster order, 1 << units_per_ctb_log2 bytes per CTB in z-scan order, units outside the picture included - and its hand-off records
// (HANDOFF_DWORDS per CTB).  Built into a library of its own with the flags of tests/emu/Makefile; the batch handle comes from libparse_emu*.so.
#include <stdint.h>
#include <string.h>
#include "hevc_device.h"
#include "emu_batch.h"

using namespace hipdec;

extern "C" long emu_raw_unit_maps(EmuBatch* b, int i, uint8_t* size, uint8_t* flags, uint8_t* ipm, uint8_t* ipmc, uint8_t* qp, uint32_t* handoff, long cap)
{
  const PicParams& P = b->L.params[i];
  const uint8_t* a = b->arena.data();
  const long n = ((long)P.ctb_w * P.ctb_h) << P.units_per_ctb_log2;
  if (n > cap) return -1;   // bytes per map
  memcpy(size, a + P.off_u_size, n); memcpy(flags, a + P.off_u_flags, n); memcpy(ipm, a + P.off_u_ipm, n); memcpy(ipmc, a + P.off_u_ipmc, n);
  memcpy(qp, a + P.off_u_qp, n);
  memcpy(handoff, a + P.off_handoff, (size_t)P.ctb_w * P.ctb_h * HANDOFF_DWORDS * 4);
  return n;
}
