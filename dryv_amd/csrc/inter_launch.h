// inter_launch.h — launch interface between the host API of the inter prediction stage (inter_api.hip) and its gfx950 kernel
// (inter.hip, inter_kernel.h).
#pragma once
#include <hip/hip_runtime.h>

#include "inter_params.h"

namespace dryv {
namespace inter {

int inter_waves_per_block();
int inter_blocks_per_cu();
// grid = number of workgroups; any grid >= 1 is correct (the waves stride over the batch's macroblocks). The events, where
// given, take the dispatch's own start and end.
hipError_t inter_launch(const IParams& P, const Args& A, int grid, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);
// the same for the bi-predictive / weighted kernel (inter_bi.hip, inter_bi_kernel.h)
int inter_bi_waves_per_block();
int inter_bi_blocks_per_cu();
hipError_t inter_bi_launch(const IParams& P, const BArgs& A, int grid, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);

}  // namespace inter
}  // namespace dryv
