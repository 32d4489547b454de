// inter_launch.h — launch interface between the host API of the inter prediction stage (inter_api.hip) and its gfx950 kernel
// (inter.hip, inter_kernel.h).
#pragma once
#include <hip/hip_runtime.h>

#include "deblock_kernel_params.h"
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

// Deblocking of the stage's pictures. Kernel A (deblock_bs.hip, deblock_bs_kernel.h): one dryv_bs_rec per macroblock of the batch
// into d_bs and, where given, d_bs_copy; d_ids: [n_frames][2][16] picture ids. A flat grid of its own size.
hipError_t deblock_bs_launch(const IParams& P, bool bipred, const void* d_mbs, const void* d_coeffs, const void* d_ids, void* d_bs,
                             void* d_bs_copy, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);
// Kernel B (inter_deblock.hip, deblock_kernel.h's bS-record variant): filters d_yuv in place. d_workspace: deblock::workspace_bytes,
// its first deblock::reset_bytes zero. Any grid >= 1 is correct (bands come off one queue).
int inter_deblock_waves_per_block();
int inter_deblock_blocks_per_cu();
hipError_t inter_deblock_launch(const deblock::DParams& P, const void* d_recs, unsigned rec_stride, const void* d_bs, void* d_yuv,
                                unsigned* d_status, void* d_workspace, int grid, hipStream_t stream, hipEvent_t ev_start,
                                hipEvent_t ev_stop);

}  // namespace inter
}  // namespace dryv
