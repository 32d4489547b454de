// deblock_bs.hip — device entry points and launch of the boundary-strength kernel (deblock_bs_kernel.h) for gfx950.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "deblock_bs_kernel.h"
#include "inter_launch.h"

namespace dryv {
namespace inter {

#ifndef DRYV_BS_WAVES
#define DRYV_BS_WAVES 4   // independent waves per workgroup (four macroblocks each), each on an LDS slice of its own
#endif

template <bool BI>
__global__ void __launch_bounds__(64 * DRYV_BS_WAVES) deblock_bs_kernel(const deblock_bs::Args A) {
  __shared__ __attribute__((aligned(64))) unsigned char lds[DRYV_BS_WAVES * deblock_bs::S_BYTES];
  const int ldsBase = (int)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  deblock_bs::bs_wave<BI>(A, ldsBase + wave * deblock_bs::S_BYTES, (int)blockIdx.x * DRYV_BS_WAVES + wave);
}

hipError_t deblock_bs_launch(const IParams& P, bool bipred, const void* d_mbs, const void* d_coeffs, const void* d_ids, void* d_bs,
                             void* d_bs_copy, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop) {
  deblock_bs::Args A;
  A.recs = (const uint8_t*)d_mbs;
  A.coeffs = (const int16_t*)d_coeffs;
  A.ids = (const uint8_t*)d_ids;
  A.bs = (u32x4*)d_bs;
  A.bs_copy = (u32x4*)d_bs_copy;
  A.W = P.W;
  A.H = P.H;
  A.n_mbs = P.n_mbs;
  const int grid = (A.n_mbs + 4 * DRYV_BS_WAVES - 1) / (4 * DRYV_BS_WAVES);
  if (bipred) hipExtLaunchKernelGGL(deblock_bs_kernel<true>, dim3(grid), dim3(64 * DRYV_BS_WAVES), 0, stream, ev_start, ev_stop, 0, A);
  else hipExtLaunchKernelGGL(deblock_bs_kernel<false>, dim3(grid), dim3(64 * DRYV_BS_WAVES), 0, stream, ev_start, ev_stop, 0, A);
  return hipGetLastError();
}

}  // namespace inter
}  // namespace dryv
