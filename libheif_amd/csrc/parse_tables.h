// parse_tables.h — HEVC constant tables of the entropy decoder (context initValues for slice_type I, rangeTabLps, transIdxLps, scans,
// sig_coeff_flag context patterns) shared by the two parser kernels: parse_core.h (one wave per substream) and parse_lanes_kernel.hip
// (one LANE per substream).  The including file defines PC_CONST (the storage qualifier of the tables) first.
#pragma once
#include <stdint.h>
#ifndef PC_CONST
#define PC_CONST static const
#endif

namespace hipdec {
namespace pcore {

// ---- context variables: group (VGPR) and lane -------------------------------------------------
// group A
enum : int {
  A_SAO_MERGE = 0, A_SAO_TYPE = 1, A_SPLIT_CU = 2 /*3*/, A_CU_TQ_BYPASS = 5, A_PART_MODE = 6, A_PREV_INTRA_LUMA = 7,
  A_INTRA_CHROMA = 8, A_SPLIT_TRANSFORM = 9 /*3*/, A_CBF_LUMA = 12 /*2*/, A_CBF_CHROMA = 14 /*4*/, A_CU_QP_DELTA = 18 /*2*/,
  A_TRANSFORM_SKIP = 20 /*2*/, A_LAST_X = 22 /*18*/, A_LAST_Y = 40 /*18*/, A_CODED_SUB_BLOCK = 58 /*4*/,
  A_CBF_CHROMA4 = 62 /* cbf_cb / cbf_cr at trafoDepth 4 (ChromaArrayType 3 only; initValue 154 like the padding lanes) */,
  // group B: sig_coeff_flag 0..43 (42 used by version 1), greater2 44..49
  B_SIG_COEFF = 0, B_GREATER2 = 44,
  // group C: greater1 0..23, then the contexts P slices add (parse_core.h with HIPDEC_PARSE_INTER)
  C_GREATER1 = 0,
  C_SKIP_FLAG = 24 /*3*/, C_PRED_MODE = 27, C_PART_MODE_INTER = 28 /*3: part_mode bin 1, bin 2 at the minimum CB size, bin 2 with AMP*/, C_MERGE_FLAG = 31,
  C_MERGE_IDX = 32, C_REF_IDX = 33 /*2*/, C_MVD_GT0 = 35, C_MVD_GT1 = 36, C_MVP_FLAG = 37, C_RQT_ROOT_CBF = 38,
  C_INTER_PRED_IDC = 39 /*5: bin 0 by coding quadtree depth 0..3, bin 1*/
};

// initValue for slice_type I (9.3.2.2, tables 9-5 .. 9-37), laid out per group / lane
PC_CONST uint8_t c_init[3][64] = {
  {153, 200, 139, 141, 157, 154, 184, 184, 63, 153, 138, 138, 111, 141, 94, 138, 182, 154, 154, 154, 139, 139,
   110, 110, 124, 125, 140, 153, 125, 127, 140, 109, 111, 143, 127, 111, 79, 108, 123, 63,
   110, 110, 124, 125, 140, 153, 125, 127, 140, 109, 111, 143, 127, 111, 79, 108, 123, 63,
   91, 171, 134, 141, 154, 154},
  {111, 111, 125, 110, 110, 94, 124, 108, 124, 107, 125, 141, 179, 153, 125, 107, 125, 141, 179, 153, 125, 107, 125, 141,
   179, 153, 125, 140, 139, 182, 182, 152, 136, 152, 136, 153, 136, 139, 111, 136, 139, 111, 141, 111,
   138, 153, 136, 167, 152, 152, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154},
  {140, 92, 137, 138, 140, 152, 138, 139, 153, 74, 149, 92, 139, 107, 122, 152, 140, 179, 166, 182, 140, 227, 122, 197,
   154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154,
   154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154}};

// initValue for initType 1 and 2 (9.3.2.2: a P slice takes 2 when cabac_init_flag is set, else 1), same lanes
PC_CONST uint8_t c_init_p[2][3][64] = {
 {{153, 185, 107, 139, 126, 154, 154, 154, 152, 124, 138, 94, 153, 111, 149, 107, 167, 154, 154, 154, 139, 139,
   125, 110, 94, 110, 95, 79, 125, 111, 110, 78, 110, 111, 111, 95, 94, 108, 123, 108,
   125, 110, 94, 110, 95, 79, 125, 111, 110, 78, 110, 111, 111, 95, 94, 108, 123, 108,
   121, 140, 61, 154, 154, 154},
  {155, 154, 139, 153, 139, 123, 123, 63, 153, 166, 183, 140, 136, 153, 154, 166, 183, 140, 136, 153, 154, 166, 183, 140,
   136, 153, 154, 170, 153, 123, 123, 107, 121, 107, 121, 167, 151, 183, 140, 151, 183, 140, 140, 140,
   107, 167, 91, 122, 107, 167, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154},
  {154, 196, 196, 167, 154, 152, 167, 182, 182, 134, 149, 136, 153, 121, 136, 137, 169, 194, 166, 167, 154, 167, 137, 182,
   197, 185, 201, 149, 139, 154, 154, 110, 122, 153, 153, 140, 198, 168, 79, 95,
   79, 63, 31, 31, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154}},
 {{153, 160, 107, 139, 126, 154, 154, 183, 152, 224, 167, 122, 153, 111, 149, 92, 167, 154, 154, 154, 139, 139,
   125, 110, 124, 110, 95, 94, 125, 111, 111, 79, 125, 126, 111, 111, 79, 108, 123, 93,
   125, 110, 124, 110, 95, 94, 125, 111, 111, 79, 125, 126, 111, 111, 79, 108, 123, 93,
   121, 140, 61, 154, 154, 154},
  {170, 154, 139, 153, 139, 123, 123, 63, 124, 166, 183, 140, 136, 153, 154, 166, 183, 140, 136, 153, 154, 166, 183, 140,
   136, 153, 154, 170, 153, 138, 138, 122, 121, 122, 121, 167, 151, 183, 140, 151, 183, 140, 140, 140,
   107, 167, 91, 107, 107, 167, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154},
  {154, 196, 167, 167, 154, 152, 167, 182, 182, 134, 149, 136, 153, 121, 136, 122, 169, 208, 166, 167, 154, 152, 167, 182,
   197, 185, 201, 134, 139, 154, 154, 154, 137, 153, 153, 169, 198, 168, 79, 95,
   79, 63, 31, 31, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154}}};

// Table 8-3: the intra prediction direction of a 4:2:2 chroma block from the mode the 4:2:0 / 4:4:4 derivation yields (8.4.3)
PC_CONST uint8_t c_map422[35] = {0, 1, 2, 2, 2, 2, 3, 5, 7, 8, 10, 11, 13, 15, 16, 18, 19, 20, 21, 22, 23, 23, 24, 24, 25, 25, 26, 27, 27, 28, 28, 29, 29, 30, 31};

// lane p: rangeTabLps[p][0..3] packed little-endian (table 9-46)
PC_CONST uint8_t c_range_lps[64 * 4] = {
  128,176,208,240, 128,167,197,227, 128,158,187,216, 123,150,178,205, 116,142,169,195, 111,135,160,185,
  105,128,152,175, 100,122,144,166,  95,116,137,158,  90,110,130,150,  85,104,123,142,  81, 99,117,135,
   77, 94,111,128,  73, 89,105,122,  69, 85,100,116,  66, 80, 95,110,  62, 76, 90,104,  59, 72, 86, 99,
   56, 69, 81, 94,  53, 65, 77, 89,  51, 62, 73, 85,  48, 59, 69, 80,  46, 56, 66, 76,  43, 53, 63, 72,
   41, 50, 59, 69,  39, 48, 56, 65,  37, 45, 54, 62,  35, 43, 51, 59,  33, 41, 48, 56,  32, 39, 46, 53,
   30, 37, 43, 50,  29, 35, 41, 48,  27, 33, 39, 45,  26, 31, 37, 43,  24, 30, 35, 41,  23, 28, 33, 39,
   22, 27, 32, 37,  21, 26, 30, 35,  20, 24, 29, 33,  19, 23, 27, 31,  18, 22, 26, 30,  17, 21, 25, 28,
   16, 20, 23, 27,  15, 19, 22, 25,  14, 18, 21, 24,  14, 17, 20, 23,  13, 16, 19, 22,  12, 15, 18, 21,
   12, 14, 17, 20,  11, 14, 16, 19,  11, 13, 15, 18,  10, 12, 15, 17,  10, 12, 14, 16,   9, 11, 13, 15,
    9, 11, 12, 14,   8, 10, 12, 14,   8,  9, 11, 13,   7,  9, 11, 12,   7,  9, 10, 12,   7,  8, 10, 11,
    6,  8,  9, 11,   6,  7,  9, 10,   6,  7,  8,  9,   2,  2,  2,  2};
// lane p: byte 0 transIdxLps[p] (table 9-47; load_tables adds bit 6 for p = 0, where an LPS flips valMps), byte 1 the p-th position of the up-right diagonal
// scan of an 8x8 array (6.5.3) as x | y << 3, byte 2 the inverse of that scan (lane x | y << 3 -> scan position)
PC_CONST uint8_t c_next_lps[64] = {
   0, 0, 1, 2, 2, 4, 4, 5, 6, 7, 8, 9, 9,11,11,12, 13,13,15,15,16,16,18,18,19,19,21,21,22,22,23,24,
  24,25,26,26,27,27,28,29,29,30,30,30,31,32,32,33, 33,33,34,34,35,35,35,36,36,36,37,37,37,38,38,63};
PC_CONST uint8_t c_diag8[64] = {
  0, 8, 1, 16, 9, 2, 24, 17, 10, 3, 32, 25, 18, 11, 4, 40, 33, 26, 19, 12, 5, 48, 41, 34, 27, 20, 13, 6, 56, 49, 42, 35,
  28, 21, 14, 7, 57, 50, 43, 36, 29, 22, 15, 58, 51, 44, 37, 30, 23, 59, 52, 45, 38, 31, 60, 53, 46, 39, 61, 54, 47, 62, 55, 63};

// 4x4 scans: nibble k = raster index (x | y << 2) of the k-th scan position
#define PC_DIAG4 0xFBE7AD369C258140ULL
#define PC_HORZ4 0xFEDCBA9876543210ULL
#define PC_VERT4 0xFB73EA62D951C840ULL
// their inverses: nibble r = scan position of raster index r (constexpr-derived, so they cannot drift from the scans)
constexpr uint64_t pc_invert_scan4(uint64_t scan)
{
  uint64_t inv = 0;
  for (int k = 0; k < 16; k++) inv |= (uint64_t)k << (4 * ((scan >> (4 * k)) & 15u));
  return inv;
}
constexpr uint64_t PC_INV_DIAG4 = pc_invert_scan4(PC_DIAG4), PC_INV_HORZ4 = pc_invert_scan4(PC_HORZ4), PC_INV_VERT4 = pc_invert_scan4(PC_VERT4);
static_assert(PC_INV_HORZ4 == PC_HORZ4 && ((PC_INV_DIAG4 >> (4 * 4)) & 15u) == 1u && ((PC_INV_VERT4 >> (4 * 1)) & 15u) == 4u, "inverse scans");
// the vertical scan is the transpose of the raster order: position ((x << 2) | y) holds raster index (x | (y << 2)), and so does its inverse
constexpr bool pc_vert4_is_transpose()
{
  for (unsigned r = 0; r < 16; r++) if (((PC_INV_VERT4 >> (r * 4)) & 15u) != (((r & 3u) << 2) | (r >> 2))) return false;
  return true;
}
static_assert(pc_vert4_is_transpose(), "inverse vertical scan");
// sig_coeff_flag ctxIdxMap for 4x4 blocks (9.3.4.2.5), nibble r = ctxIdxMap[raster index r]
#define PC_CTXIDXMAP4 0x8877886654325410ULL
// sigCtx of 9.3.4.2.5 for larger blocks before the size / component offsets, two bits per raster
// position r = x | y << 2 of the 4x4 sub-block, one word per prevCsbf (bit0 right, bit1 below)
//   0: x+y == 0 ? 2 : x+y < 3 ? 1 : 0      1: y == 0 ? 2 : y == 1 ? 1 : 0
//   2: x == 0 ? 2 : x == 1 ? 1 : 0          3: 2
constexpr uint32_t pc_sigpat(int prev_csbf)
{
  uint32_t w = 0;
  for (int r = 0; r < 16; r++) {
    const int x = r & 3, y = r >> 2;
    int v = 2;
    if (prev_csbf == 0) v = (x + y == 0) ? 2 : (x + y < 3) ? 1 : 0;
    else if (prev_csbf == 1) v = (y == 0) ? 2 : (y == 1) ? 1 : 0;
    else if (prev_csbf == 2) v = (x == 0) ? 2 : (x == 1) ? 1 : 0;
    else v = 2;
    w |= (uint32_t)v << (2 * r);
  }
  return w;
}
constexpr uint32_t PC_SIGPAT0 = pc_sigpat(0), PC_SIGPAT1 = pc_sigpat(1), PC_SIGPAT2 = pc_sigpat(2), PC_SIGPAT3 = pc_sigpat(3);
static_assert(PC_SIGPAT0 == 0x00010516u && PC_SIGPAT1 == 0x000055AAu && PC_SIGPAT2 == 0x06060606u && PC_SIGPAT3 == 0xAAAAAAAAu, "sig patterns");

// ---- sig_coeff_flag context rows (HIPDEC_PARSE_TU_TABLES) -----------------------------------------
// sigCtx (9.3.4.2.5, before the B_SIG_COEFF base) of scan position k of a 4x4 sub-block, as residual_coding derives it per sub-block: the block's
// log2 size, luma / chroma, scan index, the coded_sub_block_flag of the right / lower neighbour, "this is the block's DC sub-block"
constexpr uint32_t pc_sig_ctx(int log2n, int c_idx, int scan_idx, int right, int below, int dc_sb, int k)
{
  const uint64_t scan4 = scan_idx == 0 ? PC_DIAG4 : (scan_idx == 1 ? PC_HORZ4 : PC_VERT4);
  const uint32_t r = (uint32_t)(scan4 >> (k * 4)) & 15u;
  if (log2n == 2) return (c_idx ? 27u : 0u) + (uint32_t)((PC_CTXIDXMAP4 >> (r * 4)) & 15u);
  if (dc_sb && r == 0) return c_idx ? 27u : 0u;
  const uint32_t pat = pc_sigpat(right | (below << 1));
  const uint32_t off = c_idx == 0 ? (dc_sb ? 0u : 3u) + (log2n == 3 ? (scan_idx == 0 ? 9u : 15u) : 21u) : 27u + (log2n == 3 ? 9u : 12u);
  return off + ((pat >> (r * 2)) & 3u);
}
// That value depends on less than its arguments: a 4x4 block has one sub-block without neighbours; luma 16x16 and 32x32 blocks share their contexts, and
// so do chroma 16x16 and 32x32; above 8x8 only the diagonal scan occurs; a chroma block's DC sub-block differs from its others in position 0 alone,
// which the parser takes from a constant.  What is left are PC_SIG_ROWS_420 = 46 rows of 16 positions for 4:0:0 / 4:2:0 pictures (8x8 chroma blocks
// are scanned diagonally there, 7.4.9.11) and 8 more for the horizontal and vertical scan of 8x8 chroma blocks (ChromaArrayType 3):
//   0 .. 5    4x4 blocks: 3 * chroma + scan index
//   6 .. 29   luma 8x8: 6 + 8 * scan index + 4 * DC + right + 2 * below
//   30 .. 37  luma 16x16 / 32x32: 30 + 4 * DC + right + 2 * below
//   38 .. 41  chroma 8x8, diagonal: 38 + right + 2 * below           42 .. 45  chroma 16x16 / 32x32: 42 + right + 2 * below
//   46 .. 53  chroma 8x8, horizontal / vertical: 46 + 4 * (scan index - 1) + right + 2 * below
enum : int { PC_SIG_ROWS_420 = 46, PC_SIG_ROWS_ALL = 54, PC_SIG_ROW_BYTES = 32, PC_SIG_DC_STEP = 4 * PC_SIG_ROW_BYTES };
// first row of a block's group (right = below = 0, not the DC sub-block) ...
constexpr int pc_sig_row_group(int log2n, int c_idx, int scan_idx)
{
  if (log2n == 2) return (c_idx ? 3 : 0) + scan_idx;
  if (c_idx == 0) return log2n == 3 ? 6 + 8 * scan_idx : 30;
  return log2n == 3 ? (scan_idx == 0 ? 38 : 46 + 4 * (scan_idx - 1)) : 42;
}
// ... and the step to the rows of its DC sub-block, in bytes
constexpr int pc_sig_dc_step(int log2n, int c_idx) { return (c_idx == 0 && log2n > 2) ? PC_SIG_DC_STEP : 0; }
// the row's entries are what the sig_coeff_flag run reads instead of computing them: the LDS byte address of the context variable of every scan
// position, 16 bits each.  ctx_b_addr: the LDS byte address of context variable B_SIG_COEFF + 0 (the including file knows its LDS layout)
struct alignas(4) SigRowTable { uint16_t a[PC_SIG_ROWS_ALL * 16]; };
constexpr SigRowTable pc_make_sig_rows(uint32_t ctx_b_addr)
{
  SigRowTable t = {};
  for (int c_idx = 0; c_idx < 2; c_idx++)
    for (int log2n = 2; log2n <= 5; log2n++)
      for (int scan_idx = 0; scan_idx < (log2n <= 3 ? 3 : 1); scan_idx++)
        for (int nbp = 0; nbp < (log2n == 2 ? 1 : 4); nbp++)
          for (int dc = 0; dc < 2; dc++) {
            if (dc && pc_sig_dc_step(log2n, c_idx) == 0 && log2n > 2) continue;   // (a chroma block's DC sub-block reads the rows of the others)
            if (log2n == 2 && !dc) continue;                                      // (a 4x4 block's only sub-block is its DC sub-block)
            const int row = pc_sig_row_group(log2n, c_idx, scan_idx) + nbp + (dc && log2n > 2 ? PC_SIG_DC_STEP / PC_SIG_ROW_BYTES : 0);
            for (int k = 0; k < 16; k++) t.a[row * 16 + k] = (uint16_t)(ctx_b_addr + 4u * pc_sig_ctx(log2n, c_idx, scan_idx, nbp & 1, nbp >> 1, dc, k));
          }
  return t;
}
// the table against the per-sub-block derivation it replaces, by the row arithmetic the parser does at run time: group + 32 * right + 64 * below +
// the DC step, position 0 of a DC sub-block from entry 0 of the component's 4x4 row
constexpr bool pc_sig_rows_match(uint32_t ctx_b_addr)
{
  const SigRowTable t = pc_make_sig_rows(ctx_b_addr);
  for (int c_idx = 0; c_idx < 2; c_idx++)
    for (int log2n = 2; log2n <= 5; log2n++)
      for (int scan_idx = 0; scan_idx < (log2n <= 3 ? 3 : 1); scan_idx++)
        for (int nbp = 0; nbp < (log2n == 2 ? 1 : 4); nbp++)
          for (int dc = (log2n == 2 ? 1 : 0); dc < 2; dc++) {
            const int row_bytes = pc_sig_row_group(log2n, c_idx, scan_idx) * PC_SIG_ROW_BYTES + (nbp & 1) * 32 + (nbp >> 1) * 64 + (dc ? pc_sig_dc_step(log2n, c_idx) : 0);
            if (row_bytes % PC_SIG_ROW_BYTES || row_bytes / PC_SIG_ROW_BYTES >= PC_SIG_ROWS_ALL) return false;
            if (!(c_idx && log2n == 3 && scan_idx) && row_bytes / PC_SIG_ROW_BYTES >= PC_SIG_ROWS_420) return false;
            for (int k = 0; k < 16; k++) {
              const int at = (k == 0 && dc) ? pc_sig_row_group(2, c_idx, 0) * 16 : row_bytes / 2 + k;
              if (t.a[at] != ctx_b_addr + 4u * pc_sig_ctx(log2n, c_idx, scan_idx, nbp & 1, nbp >> 1, dc, k)) return false;
            }
          }
  return true;
}


// ---- transform-block descriptor and sub-block scans (HIPDEC_PARSE_TU_DESC) --------------------------
// What residual_coding sets up per transform block is a function of the block's kind alone: log2 size, luma / chroma, scan index (7.4.9.11: 1 and 2
// only occur up to 8x8; those kinds above are never looked up)
enum : int { PC_TU_KINDS = 24 };
constexpr int pc_tu_kind(int log2n, int c_idx, int scan_idx) { return ((c_idx ? 4 : 0) + log2n - 2) * 3 + scan_idx; }
// 6.5.3: the up-right diagonal scan of an n x n array, entry k = x | y << shift of the k-th position
struct DiagScan { uint8_t a[64]; };
constexpr DiagScan pc_diag_scan(int n, int shift)
{
  DiagScan d = {};
  int i = 0, x = 0, y = 0;
  for (;;) {
    while (y >= 0) { if (x < n && y < n) d.a[i++] = (uint8_t)(x | (y << shift)); y--; x++; }
    y = x; x = 0;
    if (i >= n * n) break;
  }
  return d;
}
static_assert(pc_diag_scan(4, 2).a[3] == ((PC_DIAG4 >> 12) & 15u) && pc_diag_scan(4, 2).a[9] == ((PC_DIAG4 >> 36) & 15u) && pc_diag_scan(4, 2).a[15] == 15, "6.5.3 against PC_DIAG4");
// the scan of a block's sub-blocks as bytes ys << 3 | xs (the bit of the sub-block in the coded_sub_block_flag bitmap), one run per grid: 1x1; 2x2
// diagonal (= vertical), 2x2 horizontal; 4x4 and 8x8 diagonal (blocks above 8x8 are scanned diagonally)
enum : int { PC_SBSCAN_1 = 0, PC_SBSCAN_2D = 4, PC_SBSCAN_2H = 8, PC_SBSCAN_4 = 12, PC_SBSCAN_8 = 28, PC_SBSCAN_BYTES = 92 };
struct alignas(4) SbScanTable { uint8_t a[PC_SBSCAN_BYTES]; };
constexpr SbScanTable pc_make_sbscan()
{
  SbScanTable t = {};
  for (int i = 0; i < 4; i++) { t.a[PC_SBSCAN_2D + i] = (uint8_t)((i >> 1) | ((i & 1) << 3)); t.a[PC_SBSCAN_2H + i] = (uint8_t)((i & 1) | ((i >> 1) << 3)); }
  for (int i = 0; i < 16; i++) t.a[PC_SBSCAN_4 + i] = pc_diag_scan(4, 3).a[i];
  for (int i = 0; i < 64; i++) t.a[PC_SBSCAN_8 + i] = pc_diag_scan(8, 3).a[i];
  return t;
}
constexpr int pc_sbscan_of(int log2n, int scan_idx) { return log2n == 2 ? PC_SBSCAN_1 : (log2n == 3 ? (scan_idx == 1 ? PC_SBSCAN_2H : PC_SBSCAN_2D) : (log2n == 4 ? PC_SBSCAN_4 : PC_SBSCAN_8)); }
// one descriptor per kind, four dwords:
//   w0  15:0 LDS byte address of the block's first sig-context row, 31:16 of the first row of its DC sub-block
//   w1  4:0 ctxOffset and 6:5 ctxShift of last_sig_coeff_x / y_prefix (9.3.4.2.3), 10:7 their cMax (2 * log2 size - 1), 17:11 the sub-block scan's
//       offset in SbScanTable, 30:18 the LDS byte address of the row whose entry 0 is the context of position 0 of a DC sub-block
//   w2, w3  the 4x4 scan inside a sub-block, nibble k = x | y << 2 of scan position k
// sigrow_addr: the LDS byte address of row 0 of the sig-context rows
struct alignas(16) TuDescTable { uint32_t w[PC_TU_KINDS][4]; };
constexpr TuDescTable pc_make_tu_desc(uint32_t sigrow_addr)
{
  TuDescTable t = {};
  for (int c_idx = 0; c_idx < 2; c_idx++)
    for (int log2n = 2; log2n <= 5; log2n++)
      for (int scan_idx = 0; scan_idx < (log2n <= 3 ? 3 : 1); scan_idx++) {
        uint32_t* const w = t.w[pc_tu_kind(log2n, c_idx, scan_idx)];
        const uint32_t rows = sigrow_addr + (uint32_t)(pc_sig_row_group(log2n, c_idx, scan_idx) * PC_SIG_ROW_BYTES);
        w[0] = rows | ((rows + (uint32_t)pc_sig_dc_step(log2n, c_idx)) << 16);
        const uint32_t ctx_offset = c_idx == 0 ? (uint32_t)(3 * (log2n - 2) + ((log2n - 1) >> 2)) : 15u;
        const uint32_t ctx_shift = c_idx == 0 ? (uint32_t)((log2n + 1) >> 2) : (uint32_t)(log2n - 2);
        const uint32_t dc0 = sigrow_addr + (uint32_t)(pc_sig_row_group(2, c_idx, 0) * PC_SIG_ROW_BYTES);
        w[1] = ctx_offset | (ctx_shift << 5) | ((uint32_t)(2 * log2n - 1) << 7) | ((uint32_t)pc_sbscan_of(log2n, scan_idx) << 11) | (dc0 << 18);
        const uint64_t scan4 = scan_idx == 0 ? PC_DIAG4 : (scan_idx == 1 ? PC_HORZ4 : PC_VERT4);
        w[2] = (uint32_t)scan4; w[3] = (uint32_t)(scan4 >> 32);
      }
  return t;
}

}  // namespace pcore
}  // namespace hipdec
