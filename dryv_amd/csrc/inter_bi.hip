// inter_bi.hip — device entry point and launch of the bi-predictive / weighted inter prediction kernel (inter_bi_kernel.h) for
// gfx950.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "inter_bi_kernel.h"
#include "inter_launch.h"

namespace dryv {
namespace inter {

#ifndef DRYV_INTER_BI_WAVES
#define DRYV_INTER_BI_WAVES 4      // independent macroblock waves per workgroup, each on an LDS slice of its own
#endif
#ifndef DRYV_INTER_BI_WGS_PER_CU
#define DRYV_INTER_BI_WGS_PER_CU 2 // what the registers allow (two waves per SIMD); 2 x 28.8 KB of the CU's 160 KB of LDS
#endif

__global__ void __launch_bounds__(64 * DRYV_INTER_BI_WAVES) inter_bi_kernel(const IParams P, const BArgs A) {
  extern __shared__ __attribute__((aligned(64))) unsigned char lds[];
  const int ldsBase = (int)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds;
  build_tables(P, ldsBase, (int)threadIdx.x, (int)blockDim.x);
  __syncthreads();  // the only workgroup-level synchronisation: the waves are independent from here on
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  bi_wave(P, A, ldsBase, ldsBase + T_END + wave * B_BYTES, (int)blockIdx.x * DRYV_INTER_BI_WAVES + wave, (int)gridDim.x * DRYV_INTER_BI_WAVES);
}

int inter_bi_waves_per_block() { return DRYV_INTER_BI_WAVES; }
int inter_bi_blocks_per_cu() { return DRYV_INTER_BI_WGS_PER_CU; }

hipError_t inter_bi_launch(const IParams& P, const BArgs& A, int grid, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop) {
  const unsigned ldsBytes = (unsigned)(T_END + DRYV_INTER_BI_WAVES * B_BYTES);
  hipExtLaunchKernelGGL(inter_bi_kernel, dim3(grid), dim3(64 * DRYV_INTER_BI_WAVES), ldsBytes, stream, ev_start, ev_stop, 0, P, A);
  return hipGetLastError();
}

}  // namespace inter
}  // namespace dryv
