// CPU-test-only access to the TU tables of the throughput CABAC parser (tests/test_parse_tu_tables_emu.py): the sig_coeff_flag context rows and the
// sub-block scans as load_tu_tables() leaves them in the (emulated) LDS, the transform-block descriptors, and the row arithmetic residual_coding does
// per sub-block - the parser's own functions, so that the test can set every entry against a plain restatement of the standard.  Built into a
// library of its own with the flags of tests/emu/Makefile and the layout of the throughput build (-DHIPDEC_PARSE_LDS_CTX=1).
#include <stdint.h>
#include <string.h>
#include "hevc_device.h"
#include "kernels.h"
#define pcore pcore_tu_probe   // this translation unit's own instance of the parser
#include "parse_core.h"

using namespace hipdec;
using namespace hipdec::pcore;

extern "C" {

// 0 number of sig-context rows in LDS, 1 LDS byte address of row 0, 2 of context variable B_SIG_COEFF + 0, 3 of the sub-block scans, 4 sizeof(Lds),
// 5 the rows a 4:0:0 / 4:2:0 build keeps, 6 number of descriptor kinds, 7 bytes of the sub-block scans
void tu_layout(int32_t* out)
{
  out[0] = PC_SIG_ROWS; out[1] = (int32_t)__builtin_offsetof(Lds, sigrow); out[2] = (int32_t)PC_LDS_CTX_B_ADDR;
  out[3] = (int32_t)__builtin_offsetof(Lds, sbscan); out[4] = (int32_t)sizeof(Lds); out[5] = PC_SIG_ROWS_420; out[6] = PC_TU_KINDS; out[7] = PC_SBSCAN_BYTES;
}

// the whole emulated LDS behind load_tu_tables() on a block of 0xa5 bytes: the test looks at the tables and at everything around them
void tu_loaded_lds(uint8_t* out)
{
  static Lds lds;
  memset(&lds, 0xa5, sizeof lds);
  load_tu_tables(&lds);
  memcpy(out, &lds, sizeof lds);
}

int tu_kind(int log2n, int c_idx, int scan_idx) { return pc_tu_kind(log2n, c_idx, scan_idx); }
void tu_desc(int kind, uint32_t* out) { for (int k = 0; k < 4; k++) out[k] = c_tu_desc.w[kind][k]; }

// the scan index residual_coding derives (7.4.9.11) for a picture of the given chroma format
int tu_scan_idx_of(int chroma_format_idc, int log2n, int c_idx, int pred_mode)
{
  static PS s;
  s.chroma_format_idc = chroma_format_idc;
  return tu_scan_idx(s, log2n, c_idx, pred_mode);
}

// LDS byte address of the sig-context row of a sub-block at bitmap position pos (ys * 8 + xs) whose right / lower neighbour is coded, from the
// descriptor's first dword, as residual_coding computes it (nb: bit 1 right, bit 8 below)
uint32_t tu_row_of(uint32_t d0, int right, int below, int pos) { return tu_sig_row(d0 & 0xffffu, d0 >> 16, (right ? 2u : 0u) | (below ? 0x100u : 0u), pos); }

}  // extern "C"
