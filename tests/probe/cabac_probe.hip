// cabac_probe.hip — TEST-ONLY probe of the arithmetic decoder of libheif_amd/csrc/parse_core.h (9.3.4.3): runs scripts of single decoder
// operations, one script per workgroup of one wave, and records the decoder's state after every operation, so that tests/test_cabac_engine_*.py
// can compare it bin by bin with the plain restatement of the standard in tests/cabac_ref.py.  Never linked into libheifhip.so.
//
// Builds (tests/probe/Makefile): gfx950 with HIPDEC_PARSE_LDS_CTX = 0 / 1 (the hand-scheduled statements of parse_bins_gfx950.h /
// parse_bins_lds_gfx950.h), the same two with -DHIPDEC_PARSE_CXX_BINS (the compiler's form of the C++ twins on the device), and the same two
// with -DHIPDEC_HOST_EMU for the CPU tier.  The probe itself is plain C++: every record is written by lane 0 with ordinary stores.
//
// A script is an array of 32-bit words: an operation word (opcode in bits 7:0, bit 31 = write no record) followed by the operation's
// arguments (OP_ARGS below).  A script is a finite list and every operation is bounded, so a probe cannot spin on its data; every position a
// script names is checked against the size of the bitstream buffer before it is used, every record against the size of the record buffer.
#if !defined(HIPDEC_HOST_EMU)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "hevc_device.h"
#include "kernels.h"
#define HIPDEC_PARSE_CHROMA_GENERAL 0
#define pcore pcore_probe   // this translation unit's own instance of the parser (as every parse_kernel*.hip has)
#include "parse_core.h"

namespace hipdec {
namespace pcore {

enum : uint32_t {
  OP_END = 0, OP_START, OP_SET_CTX, OP_SET_STATE, OP_BIN, OP_BYPASS, OP_BYPASS_MULTI, OP_BYPASS_BITS, OP_TERMINATE, OP_UNARY, OP_G1_RUN, OP_SIG_RUN,
  OP_REMAINING_V, OP_REMAINING, OP_DUMP_CTX, OP_RESTART, OP_READ_BYTES, OP_COUNT
};
// argument words behind the operation word
//   START pos end | SET_CTX group lane pStateIdx valMps | SET_STATE range value bits_needed pos zeros | BIN group lane | BYPASS | BYPASS_MULTI n |
//   BYPASS_BITS n | TERMINATE | UNARY group base shift max | G1_RUN base n g | SIG_RUN n_start idx[16] | REMAINING_V rice | REMAINING rice |
//   DUMP_CTX group | RESTART | READ_BYTES n
PC_CONST uint8_t c_op_args[OP_COUNT] = {0, 2, 4, 5, 2, 0, 1, 1, 0, 4, 3, 17, 1, 1, 1, 0, 1};
enum : int { REC_WORDS = 12 };   // op, result, range, value, bits_needed, pos, fast_limit, err, zeros, context variable, aux, win_base

#if HIPDEC_PARSE_LDS_CTX
PC_DEV uint32_t probe_ctx_get(PS& s, int group, int lane) { return pc_uni(s.L->ctx[group * 64 + (lane & 63)]); }
PC_DEV void probe_ctx_set(PS& s, int group, int ctx_lane, uint32_t p_state, uint32_t mps)
{
  PC_VEC_BEGIN if (lane == 0) s.L->ctx[group * 64 + (ctx_lane & 63)] = ((62u - p_state) << 2) | (mps << 16); PC_VEC_END
  PC_LDS_SYNC();
}
#define PROBE_GROUP(s, g) ((g) == 0 ? PS::ctxA : ((g) == 1 ? PS::ctxB : PS::ctxC))
#else
PC_DEV VReg& probe_group(PS& s, int g) { return g == 0 ? s.ctxA : (g == 1 ? s.ctxB : s.ctxC); }
PC_DEV uint32_t probe_ctx_get(PS& s, int group, int lane) { return pc_rdlane(probe_group(s, group), lane); }
PC_DEV void probe_ctx_set(PS& s, int group, int ctx_lane, uint32_t p_state, uint32_t mps)
{
  const uint32_t v = (62u - p_state) | (mps << 16);
  // (one call per group: the register a reference binds to has to be known at compile time on the device)
  if (group == 0) pc_wrlane(s.ctxA, ctx_lane & 63, v); else if (group == 1) pc_wrlane(s.ctxB, ctx_lane & 63, v); else pc_wrlane(s.ctxC, ctx_lane & 63, v);
}
#endif

// `words` / `rec`: the script and its record area (rec_cap words); bs / bs_len: the bitstream buffer (padded by the caller as batch_layout.hip pads
// the product's: zeroed up to the next multiple of 256 behind len + 512, the parser's window loads run up to 512 bytes past a substream's end)
PC_DEV void probe_script(const uint32_t* words, uint32_t n_words, uint32_t* rec, uint32_t rec_cap, const uint8_t* bs, uint32_t bs_len, Lds* lds)
{
  PS s;
  s.L = lds;
  s.bs = bs;
  s.err = 0; s.zeros = 0; s.pos = 0; s.end = 0; s.win_base = 0xfffff000u; s.fast_limit = 0;
  s.range = pc_vec(510u << 7); s.value = pc_vec(0u); s.bits_needed = pc_vec((uint32_t)-8);
  s.slice_qp_y = 26;
#if HIPDEC_PARSE_INTER
  s.init_type = 0;
#endif
  PC_VEC_BEGIN PC_L(s.win) = 0u; PC_L(s.win_next) = 0u; PC_VEC_END
  load_tables(s);
  init_contexts(s);
  uint32_t pc = 0, rp = 0;
  bool started = false;
  while (pc < n_words) {
    const uint32_t opw = pc_uni(words[pc]);
    const uint32_t op = opw & 255u;
    if (op == OP_END || op >= OP_COUNT) break;
    const uint32_t na = c_op_args[op];
    if (pc + 1u + na > n_words) break;
    uint32_t a[5] = {0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < na && i < 5u; i++) a[i] = pc_uni(words[pc + 1u + i]);
    uint32_t result = 0, ctxv = 0, aux = 0;
    // nothing reads the bitstream before a START / SET_STATE has passed the bounds check
    if (!started && op != OP_START && op != OP_SET_STATE && op != OP_SET_CTX && op != OP_DUMP_CTX) break;
    switch (op) {
    case OP_START:
      if (a[0] > a[1] || a[1] > bs_len) { pc = n_words; continue; }
      cabac_start(s, a[0], a[1]);
      started = true;
      break;
    case OP_SET_CTX:
      probe_ctx_set(s, (int)(a[0] % 3u), (int)a[1], a[2] > 62u ? 62u : a[2], a[3] & 1u);
      ctxv = probe_ctx_get(s, (int)(a[0] % 3u), (int)a[1]);
      break;
    case OP_SET_STATE:   // the way a parked row resumes (load_row_state): the window is loaded again by the first byte read
      if (a[3] > s.end || s.end > bs_len || !started) { pc = n_words; continue; }
      s.range = pc_vec(a[0]); s.value = pc_vec(a[1]); s.bits_needed = pc_vec(a[2]);
      s.pos = a[3]; s.zeros = (int32_t)a[4]; s.win_base = 0xfffff000u; s.fast_limit = 0;
      break;
    case OP_BIN: {
      const int g = (int)(a[0] % 3u), l = (int)(a[1] & 63u);
#if HIPDEC_PARSE_LDS_CTX
      result = (uint32_t)decode_bin(s, PROBE_GROUP(s, g), l);
#else
      result = (uint32_t)(g == 0 ? decode_bin(s, s.ctxA, l) : (g == 1 ? decode_bin(s, s.ctxB, l) : decode_bin(s, s.ctxC, l)));
#endif
      ctxv = probe_ctx_get(s, g, l);
      break;
    }
    case OP_BYPASS: result = (uint32_t)decode_bypass(s); break;
    case OP_BYPASS_MULTI: {
      const int n = (int)(a[0] < 1u ? 1u : (a[0] > 8u ? 8u : a[0]));
      result = decode_bypass_multi(s, n);
      // the quotient estimate of the division before its repair, recomputed from the exact dividend result * range + remainder (never in product code)
      const UReg dividend = pc_mul24(pc_vec(result), s.range) + s.value;
      aux = pc_uni((UReg)((float)dividend * pc_rcp((float)s.range)));
      break;
    }
    case OP_BYPASS_BITS: result = (uint32_t)decode_bypass_bits(s, (int)(a[0] > 32u ? 32u : a[0])); break;
    case OP_TERMINATE: result = (uint32_t)decode_terminate(s); break;
    case OP_UNARY: {
      const int g = (int)(a[0] % 3u), base = (int)(a[1] & 63u), sh = (int)(a[2] & 3u), mx = (int)(a[3] > 32u ? 32u : a[3]);
#if HIPDEC_PARSE_LDS_CTX
      result = (uint32_t)decode_unary_ctx_run(s, PROBE_GROUP(s, g), base, sh, mx);
#else
      result = (uint32_t)(g == 0 ? decode_unary_ctx_run(s, s.ctxA, base, sh, mx) : (g == 1 ? decode_unary_ctx_run(s, s.ctxB, base, sh, mx) : decode_unary_ctx_run(s, s.ctxC, base, sh, mx)));
#endif
      break;
    }
    case OP_G1_RUN: {
      int g = (int)(a[2] & 3u);
      const int n = (int)(a[1] < 1u ? 1u : (a[1] > 8u ? 8u : a[1]));
      result = decode_g1_run(s, (int)(a[0] & 63u), n, g);
      aux = (uint32_t)g;
      break;
    }
    case OP_SIG_RUN: {
      const int n_start = (int)(a[0] < 1u ? 1u : (a[0] > 15u ? 15u : a[0]));
      VReg vctx;
      PC_VEC_BEGIN
        const uint32_t c = words[pc + 2u + ((uint32_t)lane & 15u)] & 63u;
        PC_L(vctx) = c;
#if HIPDEC_PARSE_LDS_CTX
        if (lane < 16) s.L->vctx[lane] = (uint32_t)__builtin_offsetof(Lds, ctx) + 4u * (uint32_t)PS::ctxB.base + 4u * c;
#endif
      PC_VEC_END
      PC_LDS_SYNC();
      result = decode_sig_run(s, vctx, n_start);
      break;
    }
    case OP_REMAINING_V: result = pc_uni(decode_remaining_v(s, pc_vec(a[0] > 4u ? 4u : a[0]))); break;
    case OP_REMAINING: result = (uint32_t)decode_remaining(s, (int)(a[0] > 4u ? 4u : a[0])); break;
    case OP_DUMP_CTX: {
      const int g = (int)(a[0] % 3u);
      if (!(opw >> 31) && rp + 64u <= rec_cap) {
#if HIPDEC_PARSE_LDS_CTX
        PC_LDS_SYNC();
        PC_VEC_BEGIN rec[rp + (uint32_t)lane] = s.L->ctx[g * 64 + lane]; PC_VEC_END
#else
        PC_VEC_BEGIN rec[rp + (uint32_t)lane] = g == 0 ? PC_L(s.ctxA) : (g == 1 ? PC_L(s.ctxB) : PC_L(s.ctxC)); PC_VEC_END
#endif
        rp += 64u;
      }
      pc += 1u + na;
      continue;
    }
    case OP_RESTART: cabac_restart(s); break;   // 9.3.2.5 behind pcm_flag / the PCM samples: the function pcm_coding_unit calls
    case OP_READ_BYTES: {   // pcm_sample bytes: read_byte() as pcm_coding_unit calls it
      const uint32_t n = a[0] > 64u ? 64u : a[0];
      for (uint32_t i = 0; i < n; i++) result = (result << 8) | read_byte(s);
      break;
    }
    default: break;
    }
    if (!(opw >> 31) && rp + REC_WORDS <= rec_cap) {
      const uint32_t r_range = pc_uni(s.range), r_value = pc_uni(s.value), r_bits = pc_uni(s.bits_needed);
      PC_VEC_BEGIN
        if (lane == 0) {
          uint32_t* o = rec + rp;
          o[0] = op; o[1] = result; o[2] = r_range; o[3] = r_value; o[4] = r_bits; o[5] = s.pos; o[6] = s.fast_limit; o[7] = (uint32_t)s.err;
          o[8] = (uint32_t)s.zeros; o[9] = ctxv; o[10] = aux; o[11] = s.win_base;
        }
      PC_VEC_END
      rp += REC_WORDS;
    }
    pc += 1u + na;
  }
}

}  // namespace pcore

#if !defined(HIPDEC_HOST_EMU)
__global__ __launch_bounds__(64) void k_cabac_probe(const uint32_t* words, const uint32_t* script_off, const uint32_t* rec_off, uint32_t* rec, const uint8_t* bs,
                                                    uint32_t bs_len)
{
  __shared__ pcore::Lds lds;   // the kernel's only __shared__ object: the LDS statements address it from LDS address 0
  const uint32_t k = blockIdx.x;
  pcore::probe_script(words + script_off[k], script_off[k + 1] - script_off[k], rec + rec_off[k], rec_off[k + 1] - rec_off[k], bs, bs_len, &lds);
}
#endif

}  // namespace hipdec

#if defined(HIPDEC_HOST_EMU)
// the path counters of parse_core.h (PC_COUNT) since the last call; reading resets them
extern "C" __attribute__((visibility("default"))) void cabac_probe_path_counts(uint64_t* out) { for (int k = 0; k < 8; k++) { out[k] = hipdec_emu_path_counts[k]; hipdec_emu_path_counts[k] = 0; } }
#endif

// script_off / rec_off: n_scripts + 1 word offsets into words / rec.  bs must be readable up to bs_alloc >= align_up(bs_len + 512, 256) bytes.
// Returns 0, or a negative / HIP error code.
extern "C" __attribute__((visibility("default"))) int cabac_probe_run(const uint32_t* words, const uint32_t* script_off, const uint32_t* rec_off, int n_scripts, uint32_t* rec, const uint8_t* bs,
                               uint32_t bs_len, uint32_t bs_alloc)
{
  using namespace hipdec;
  if (n_scripts <= 0) return 0;
  if ((uint64_t)bs_alloc < (((uint64_t)bs_len + 512u + 255u) & ~(uint64_t)255u)) return -1;
  for (int k = 0; k < n_scripts; k++) if (script_off[k + 1] < script_off[k] || rec_off[k + 1] < rec_off[k]) return -2;
#if defined(HIPDEC_HOST_EMU)
  pcore::Lds* lds = new pcore::Lds();
  for (int k = 0; k < n_scripts; k++) {
    memset((void*)lds, 0, sizeof(*lds));
    pcore::probe_script(words + script_off[k], script_off[k + 1] - script_off[k], rec + rec_off[k], rec_off[k + 1] - rec_off[k], bs, bs_len, lds);
  }
  delete lds;
  return 0;
#else
  const size_t nw = script_off[n_scripts], nr = rec_off[n_scripts];
  uint32_t *d_words = nullptr, *d_soff = nullptr, *d_roff = nullptr, *d_rec = nullptr;
  uint8_t* d_bs = nullptr;
  hipError_t e = hipSuccess;
#define PROBE_TRY(x) do { if (e == hipSuccess) e = (x); } while (0)
  PROBE_TRY(hipMalloc((void**)&d_words, (nw + 1) * 4));
  PROBE_TRY(hipMalloc((void**)&d_soff, (size_t)(n_scripts + 1) * 4));
  PROBE_TRY(hipMalloc((void**)&d_roff, (size_t)(n_scripts + 1) * 4));
  PROBE_TRY(hipMalloc((void**)&d_rec, (nr + 1) * 4));
  PROBE_TRY(hipMalloc((void**)&d_bs, bs_alloc));
  PROBE_TRY(hipMemcpy(d_words, words, nw * 4, hipMemcpyHostToDevice));
  PROBE_TRY(hipMemcpy(d_soff, script_off, (size_t)(n_scripts + 1) * 4, hipMemcpyHostToDevice));
  PROBE_TRY(hipMemcpy(d_roff, rec_off, (size_t)(n_scripts + 1) * 4, hipMemcpyHostToDevice));
  PROBE_TRY(hipMemset(d_rec, 0xee, (nr + 1) * 4));
  PROBE_TRY(hipMemcpy(d_bs, bs, bs_alloc, hipMemcpyHostToDevice));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_cabac_probe, dim3((unsigned)n_scripts), dim3(64), 0, 0, d_words, d_soff, d_roff, d_rec, d_bs, bs_len);
    e = hipGetLastError();
  }
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(hipMemcpy(rec, d_rec, nr * 4, hipMemcpyDeviceToHost));
#undef PROBE_TRY
  (void)hipFree(d_words); (void)hipFree(d_soff); (void)hipFree(d_roff); (void)hipFree(d_rec); (void)hipFree(d_bs);
  return (int)e;
#endif
}
