// inter_deblock.hip — device entry point and launch of the band filter driven by bS records (deblock_kernel.h,
// deblock_wave<LUMA, true>) for gfx950: the deblocking of the inter stage's P and B pictures. Wave roles, workgroup shape and
// residency are those measured for the intra filter (deblock.hip).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "deblock_kernel.h"
#include "deblock_params.h"
#include "inter_launch.h"

namespace dryv {
namespace inter {

#ifndef DRYV_DEBLOCK_WAVES
#define DRYV_DEBLOCK_WAVES 3
#endif
#ifndef DRYV_DEBLOCK_CHROMA_EVERY
#define DRYV_DEBLOCK_CHROMA_EVERY 3
#endif
#ifndef DRYV_DEBLOCK_WGS_PER_CU
#define DRYV_DEBLOCK_WGS_PER_CU 2
#endif

__global__ void __launch_bounds__(64 * DRYV_DEBLOCK_WAVES) inter_deblock_kernel(const deblock::DParams P, deblock::Args A) {
  extern __shared__ __attribute__((aligned(64))) unsigned char lds[];
  const int ldsBase = (int)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds;
  deblock::build_tables(P, ldsBase, (int)threadIdx.x, (int)blockDim.x);
  deblock::build_tables_bs(P, ldsBase, (int)threadIdx.x, (int)blockDim.x);
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ts = ldsBase + deblock::T_END_BS + wave * deblock::S_BYTES;
  if (wave % DRYV_DEBLOCK_CHROMA_EVERY == DRYV_DEBLOCK_CHROMA_EVERY - 1) deblock::deblock_wave<false, true>(P, A, ldsBase, ts);
  else deblock::deblock_wave<true, true>(P, A, ldsBase, ts);
}

int inter_deblock_waves_per_block() { return DRYV_DEBLOCK_WAVES; }
int inter_deblock_blocks_per_cu() { return DRYV_DEBLOCK_WGS_PER_CU; }

hipError_t inter_deblock_launch(const deblock::DParams& P, const void* d_recs, unsigned rec_stride, const void* d_bs, void* d_yuv,
                                unsigned* d_status, void* d_workspace, int grid, hipStream_t stream, hipEvent_t ev_start,
                                hipEvent_t ev_stop) {
  deblock::Args A;
  A.mbs = nullptr;
  A.yuv = (uint8_t*)d_yuv;
  A.status = d_status;
  A.recs = (const uint8_t*)d_recs;
  A.bs = (const u32x4*)d_bs;
  A.recStride = rec_stride;
  deblock::place_workspace(P, (unsigned char*)d_workspace, &A);
  const unsigned ldsBytes = (unsigned)(deblock::T_END_BS + DRYV_DEBLOCK_WAVES * deblock::S_BYTES);
  hipExtLaunchKernelGGL(inter_deblock_kernel, dim3(grid), dim3(64 * DRYV_DEBLOCK_WAVES), ldsBytes, stream, ev_start, ev_stop, 0, P, A);
  return hipGetLastError();
}

}  // namespace inter
}  // namespace dryv
