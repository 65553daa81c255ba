// parse_kernel_inter_general.hip — the CABAC parse kernel for batches that hold P / B pictures AND 4:2:2 or 4:4:4 pictures (sequence tracks of those
// formats, or such a track coalesced with others into one launch set): parse_core.h compiled with both the inter syntax (parse_kernel_inter.hip) and
// the ChromaArrayType 2 / 3 paths (parse_kernel_general.hip).  Kept apart from k_parse_inter so that the 4:0:0 / 4:2:0 tracks keep the build without
// the chroma block loops; launch_parse() sends a batch here when the host found both (ParseArgs::inter, ParseArgs::general_chroma).  One register
// budget, as k_parse_inter (sequences are a latency path).
#include <hip/hip_runtime.h>
#include "hevc_device.h"
#include "kernels.h"
#define HIPDEC_PARSE_CHROMA_GENERAL 1
#define HIPDEC_PARSE_INTER 1
#define pcore pcore_inter_general    // own namespace: this translation unit's inline functions differ from the other parse kernels'
#include "parse_core.h"

namespace hipdec {

__global__ __launch_bounds__(64) void k_parse_inter_gen(ParseArgs A)
{
  __shared__ pcore::Lds lds;
  const int lane = (int)threadIdx.x;
  uint32_t t = 0;
  if (lane == 0) t = atomicAdd(A.ticket, 1u);
  const uint32_t wave_idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
  if (wave_idx >= A.num_waves) return;
  pcore::parse_wave(A, wave_idx, &lds);
}

void launch_parse_inter_general(const ParseArgs& a, hipStream_t s)
{
  if (!a.num_waves) return;
  hipLaunchKernelGGL(k_parse_inter_gen, dim3(a.num_waves), dim3(64), 0, s, a);
}

}  // namespace hipdec
