// inter_api.hip — the extern "C" boundary of the inter prediction stage (include/dryv_recon.h: dryv_inter_*): a stage object
// of its own next to dryv_recon_ctx, on a stream of its own or on a borrowed one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "inter_launch.h"

using dryv::inter::Args;
using dryv::inter::IParams;

struct dryv_inter_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;   // the most recent launch's own start and end
  hipEvent_t ev_tab = nullptr;                        // the most recent copy of the reference table has left h_refs
  bool timed = false, tab_pending = false;
  unsigned* d_status = nullptr;
  unsigned* h_status = nullptr;   // pinned
  // the reference table of the most recent submit: pinned staging + device copy, grow-only (a device copy is replaced in
  // stream order, behind the launch that read it; the staging waits for its own copy)
  void** h_refs = nullptr;
  void** d_refs = nullptr;
  size_t cap_refs = 0;
  int num_cus = 256;
};

namespace {

int ensure_refs(dryv_inter_ctx* ctx, size_t n) {
  if (ctx->cap_refs >= n) return DRYV_OK;
  // (the old table may still be read by launches in flight)
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return DRYV_E_DEVICE;
  if (ctx->h_refs) (void)hipHostFree(ctx->h_refs);
  if (ctx->d_refs) (void)hipFree(ctx->d_refs);
  ctx->h_refs = ctx->d_refs = nullptr;
  ctx->cap_refs = 0;
  ctx->tab_pending = false;
  const size_t cap = std::max<size_t>(n, 1024);
  if (hipHostMalloc((void**)&ctx->h_refs, cap * sizeof(void*), hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void**)&ctx->d_refs, cap * sizeof(void*)) != hipSuccess)
    return DRYV_E_NOMEM;
  ctx->cap_refs = cap;
  return DRYV_OK;
}

}  // namespace

extern "C" {

int dryv_inter_check(const dryv_frame_params* fp, uint32_t n_frames, uint32_t n_refs) {
  return dryv::inter::build_iparams(fp, n_frames, n_refs, nullptr);
}

int dryv_inter_create(dryv_inter_ctx** out, int device_ordinal, void* stream) {
  if (!out) return DRYV_E_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return DRYV_E_NODEVICE;
  if (device_ordinal < 0 || device_ordinal >= n) return DRYV_E_INVALID;
  if (hipSetDevice(device_ordinal) != hipSuccess) return DRYV_E_NODEVICE;
  dryv_inter_ctx* ctx = new (std::nothrow) dryv_inter_ctx();
  if (!ctx) return DRYV_E_NOMEM;
  ctx->device = device_ordinal;
  ctx->stream = (hipStream_t)stream;
  if (!stream) {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
      delete ctx;
      return DRYV_E_DEVICE;
    }
    ctx->own_stream = true;
  }
  if (hipMalloc((void**)&ctx->d_status, 16) != hipSuccess || hipMemset(ctx->d_status, 0, 16) != hipSuccess ||
      hipHostMalloc((void**)&ctx->h_status, 16, hipHostMallocDefault) != hipSuccess || hipEventCreate(&ctx->ev_start) != hipSuccess ||
      hipEventCreate(&ctx->ev_stop) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_tab, hipEventDisableTiming) != hipSuccess) {
    dryv_inter_destroy(ctx);
    return DRYV_E_DEVICE;
  }
  *ctx->h_status = 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess && prop.multiProcessorCount > 0) ctx->num_cus = prop.multiProcessorCount;
  *out = ctx;
  return DRYV_OK;
}

void dryv_inter_destroy(dryv_inter_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->h_refs) (void)hipHostFree(ctx->h_refs);
  if (ctx->d_refs) (void)hipFree(ctx->d_refs);
  if (ctx->d_status) (void)hipFree(ctx->d_status);
  if (ctx->h_status) (void)hipHostFree(ctx->h_status);
  if (ctx->ev_start) (void)hipEventDestroy(ctx->ev_start);
  if (ctx->ev_stop) (void)hipEventDestroy(ctx->ev_stop);
  if (ctx->ev_tab) (void)hipEventDestroy(ctx->ev_tab);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int dryv_inter_submit_device(dryv_inter_ctx* ctx, const dryv_frame_params* fp, uint32_t n_frames, uint32_t n_refs,
                             const void* const* d_refs, const void* d_mbs, const void* d_coeffs, void* d_yuv_out) {
  if (!ctx || !d_refs || !d_mbs || !d_coeffs || !d_yuv_out) return DRYV_E_INVALID;
  IParams P;
  int st = dryv::inter::build_iparams(fp, n_frames, n_refs, &P);
  if (st != DRYV_OK) return st;
  // 16-byte loads of records and coefficients, 16-byte stores of the rows, aligned dword loads of the references
  if (((uintptr_t)d_mbs | (uintptr_t)d_coeffs | (uintptr_t)d_yuv_out) & 15u) return DRYV_E_INVALID;
  const size_t n_tab = (size_t)n_frames * n_refs;
  for (size_t k = 0; k < n_tab; k++)
    if (!d_refs[k] || ((uintptr_t)d_refs[k] & 15u)) return DRYV_E_INVALID;
  (void)hipSetDevice(ctx->device);
  if ((st = ensure_refs(ctx, n_tab)) != DRYV_OK) return st;
  if (ctx->tab_pending && hipEventSynchronize(ctx->ev_tab) != hipSuccess) return DRYV_E_DEVICE;
  std::copy(d_refs, d_refs + n_tab, (const void**)ctx->h_refs);
  if (hipMemcpyAsync(ctx->d_refs, ctx->h_refs, n_tab * sizeof(void*), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipEventRecord(ctx->ev_tab, ctx->stream) != hipSuccess)
    return DRYV_E_DEVICE;
  ctx->tab_pending = true;
  Args A;
  A.refs = (const uint8_t* const*)ctx->d_refs;
  A.mbs = (const dryv_inter_mb*)d_mbs;
  A.coeffs = (const int16_t*)d_coeffs;
  A.yuv = (uint8_t*)d_yuv_out;
  A.status = ctx->d_status;
  // a persistent grid: the waves stride over the macroblocks, so a smaller grid is merely slower
  const int wpb = dryv::inter::inter_waves_per_block();
  const long long want = ((long long)P.n_mbs + wpb - 1) / wpb;
  const int grid = (int)std::max(1ll, std::min(want, (long long)ctx->num_cus * dryv::inter::inter_blocks_per_cu()));
  if (dryv::inter::inter_launch(P, A, grid, ctx->stream, ctx->ev_start, ctx->ev_stop) != hipSuccess) return DRYV_E_DEVICE;
  ctx->timed = true;
  return DRYV_OK;
}

int dryv_inter_sync(dryv_inter_ctx* ctx) {
  if (!ctx) return DRYV_E_INVALID;
  (void)hipSetDevice(ctx->device);
  // the status word of everything submitted since the last sync, then cleared for what follows
  if (hipMemcpyAsync(ctx->h_status, ctx->d_status, 16, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipMemsetAsync(ctx->d_status, 0, 16, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
    return DRYV_E_DEVICE;
  ctx->tab_pending = false;
  return (*ctx->h_status & 1u) ? DRYV_E_UNSUPPORTED : DRYV_OK;
}

int dryv_inter_last_kernel_ms(dryv_inter_ctx* ctx, float* ms) {
  if (!ctx || !ms) return DRYV_E_INVALID;
  if (!ctx->timed) return DRYV_E_STATE;
  if (hipEventSynchronize(ctx->ev_stop) != hipSuccess || hipEventElapsedTime(ms, ctx->ev_start, ctx->ev_stop) != hipSuccess)
    return DRYV_E_DEVICE;
  return DRYV_OK;
}

}  // extern "C"
