// inter_api.hip — the extern "C" boundary of the inter prediction stage (include/dryv_recon.h: dryv_inter_*): a stage object
// of its own next to dryv_recon_ctx, on a stream of its own or on a borrowed one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "deblock_params.h"
#include "inter_launch.h"
#include "status_words.h"

using dryv::inter::Args;
using dryv::inter::BArgs;
using dryv::inter::IParams;

struct dryv_inter_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;   // the most recent launch's own start and end
  hipEvent_t ev_tab = nullptr;                        // the most recent submit's copies have left the staging buffers
  bool timed = false, tab_pending = false;
  unsigned* d_status = nullptr;
  unsigned* h_status = nullptr;   // pinned
  // what the most recent submit copied in: pinned staging + device copy, grow-only (a device copy is replaced in stream order,
  // behind the launch that read it; the staging waits for its own copy). The reference table (list 0's for a bi-predictive
  // submit), list 1's table, the pictures' weights.
  struct Staged {
    void* h = nullptr;
    void* d = nullptr;
    size_t cap = 0;   // bytes
  } refs, refs1, weights, ids;   // ids: the deblocking call's picture-id tables, [n_frames][2][16] bytes
  // deblocking workspace, device only, grow-only: [the filter's counters, progress words and side buffers (deblock_params.h)]
  // [one dryv_bs_rec per macroblock]
  void* d_dbwork = nullptr;
  size_t cap_dbwork = 0;
  hipEvent_t ev_bs_start = nullptr, ev_bs_stop = nullptr;   // the most recent boundary-strength launch's own start and end
  bool deblock_timed = false;
  int num_cus = 256;
};

namespace {

void release(dryv_inter_ctx::Staged& s) {
  if (s.h) (void)hipHostFree(s.h);
  if (s.d) (void)hipFree(s.d);
  s = dryv_inter_ctx::Staged();
}

int ensure(dryv_inter_ctx* ctx, dryv_inter_ctx::Staged& s, size_t bytes) {
  if (s.cap >= bytes) return DRYV_OK;
  // (the old copy may still be read by launches in flight)
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return DRYV_E_DEVICE;
  release(s);
  ctx->tab_pending = false;
  const size_t cap = std::max<size_t>(bytes, 8192);
  if (hipHostMalloc(&s.h, cap, hipHostMallocDefault) != hipSuccess || hipMalloc(&s.d, cap) != hipSuccess) return DRYV_E_NOMEM;
  s.cap = cap;
  return DRYV_OK;
}

// every pointer of a reference table present and 16-byte aligned
bool refs_ok(const void* const* tab, size_t n) {
  for (size_t k = 0; k < n; k++)
    if (!tab[k] || ((uintptr_t)tab[k] & 15u)) return false;
  return true;
}

// the persistent grid of a kernel with wpb waves per workgroup and room for per_cu workgroups on a CU: the waves stride over
// the macroblocks, so a smaller grid is merely slower
int grid_for(const dryv_inter_ctx* ctx, int n_mbs, int wpb, int per_cu) {
  const long long want = ((long long)n_mbs + wpb - 1) / wpb;
  return (int)std::max(1ll, std::min(want, (long long)ctx->num_cus * per_cu));
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
      hipEventCreate(&ctx->ev_stop) != hipSuccess || hipEventCreate(&ctx->ev_bs_start) != hipSuccess ||
      hipEventCreate(&ctx->ev_bs_stop) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_tab, hipEventDisableTiming) != hipSuccess) {
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
  release(ctx->refs);
  release(ctx->refs1);
  release(ctx->weights);
  release(ctx->ids);
  if (ctx->d_dbwork) (void)hipFree(ctx->d_dbwork);
  if (ctx->ev_bs_start) (void)hipEventDestroy(ctx->ev_bs_start);
  if (ctx->ev_bs_stop) (void)hipEventDestroy(ctx->ev_bs_stop);
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
  if (!refs_ok(d_refs, n_tab)) return DRYV_E_INVALID;
  (void)hipSetDevice(ctx->device);
  if ((st = ensure(ctx, ctx->refs, n_tab * sizeof(void*))) != DRYV_OK) return st;
  if (ctx->tab_pending && hipEventSynchronize(ctx->ev_tab) != hipSuccess) return DRYV_E_DEVICE;
  std::copy(d_refs, d_refs + n_tab, (const void**)ctx->refs.h);
  if (hipMemcpyAsync(ctx->refs.d, ctx->refs.h, n_tab * sizeof(void*), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipEventRecord(ctx->ev_tab, ctx->stream) != hipSuccess)
    return DRYV_E_DEVICE;
  ctx->tab_pending = true;
  Args A;
  A.refs = (const uint8_t* const*)ctx->refs.d;
  A.mbs = (const dryv_inter_mb*)d_mbs;
  A.coeffs = (const int16_t*)d_coeffs;
  A.yuv = (uint8_t*)d_yuv_out;
  A.status = ctx->d_status;
  const int grid = grid_for(ctx, P.n_mbs, dryv::inter::inter_waves_per_block(), dryv::inter::inter_blocks_per_cu());
  if (dryv::inter::inter_launch(P, A, grid, ctx->stream, ctx->ev_start, ctx->ev_stop) != hipSuccess) return DRYV_E_DEVICE;
  ctx->timed = true;
  return DRYV_OK;
}

int dryv_inter_check_bipred(const dryv_frame_params* fp, uint32_t n_frames, uint32_t n_refs0, uint32_t n_refs1,
                            const dryv_inter_weights* weights) {
  return dryv::inter::build_bparams(fp, n_frames, n_refs0, n_refs1, weights, nullptr);
}

int dryv_inter_submit_device_bipred(dryv_inter_ctx* ctx, const dryv_frame_params* fp, uint32_t n_frames, uint32_t n_refs0,
                                    uint32_t n_refs1, const void* const* d_refs0, const void* const* d_refs1,
                                    const dryv_inter_weights* weights, const void* d_mbs, const void* d_coeffs, void* d_yuv_out) {
  if (!ctx || !d_refs0 || (n_refs1 && !d_refs1) || !d_mbs || !d_coeffs || !d_yuv_out) return DRYV_E_INVALID;
  IParams P;
  int st = dryv::inter::build_bparams(fp, n_frames, n_refs0, n_refs1, weights, &P);
  if (st != DRYV_OK) return st;
  if (((uintptr_t)d_mbs | (uintptr_t)d_coeffs | (uintptr_t)d_yuv_out) & 15u) return DRYV_E_INVALID;
  const size_t n0 = (size_t)n_frames * n_refs0, n1 = (size_t)n_frames * n_refs1, wb = weights ? (size_t)n_frames * sizeof(dryv_inter_weights) : 0;
  if (!refs_ok(d_refs0, n0) || !refs_ok(d_refs1, n1)) return DRYV_E_INVALID;
  (void)hipSetDevice(ctx->device);
  if ((st = ensure(ctx, ctx->refs, n0 * sizeof(void*))) != DRYV_OK || (st = ensure(ctx, ctx->refs1, n1 * sizeof(void*))) != DRYV_OK ||
      (st = ensure(ctx, ctx->weights, wb)) != DRYV_OK)
    return st;
  if (ctx->tab_pending && hipEventSynchronize(ctx->ev_tab) != hipSuccess) return DRYV_E_DEVICE;
  std::copy(d_refs0, d_refs0 + n0, (const void**)ctx->refs.h);
  if (n1) std::copy(d_refs1, d_refs1 + n1, (const void**)ctx->refs1.h);
  if (wb) memcpy(ctx->weights.h, weights, wb);
  if (hipMemcpyAsync(ctx->refs.d, ctx->refs.h, n0 * sizeof(void*), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      (n1 && hipMemcpyAsync(ctx->refs1.d, ctx->refs1.h, n1 * sizeof(void*), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) ||
      (wb && hipMemcpyAsync(ctx->weights.d, ctx->weights.h, wb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) ||
      hipEventRecord(ctx->ev_tab, ctx->stream) != hipSuccess)
    return DRYV_E_DEVICE;
  ctx->tab_pending = true;
  BArgs A;
  A.refs[0] = (const uint8_t* const*)ctx->refs.d;
  A.refs[1] = n1 ? (const uint8_t* const*)ctx->refs1.d : nullptr;
  A.weights = wb ? (const dryv_inter_weights*)ctx->weights.d : nullptr;
  A.mbs = (const dryv_inter_bmb*)d_mbs;
  A.coeffs = (const int16_t*)d_coeffs;
  A.yuv = (uint8_t*)d_yuv_out;
  A.status = ctx->d_status;
  A.n_refs1 = (int)n_refs1;
  const int grid = grid_for(ctx, P.n_mbs, dryv::inter::inter_bi_waves_per_block(), dryv::inter::inter_bi_blocks_per_cu());
  if (dryv::inter::inter_bi_launch(P, A, grid, ctx->stream, ctx->ev_start, ctx->ev_stop) != hipSuccess) return DRYV_E_DEVICE;
  ctx->timed = true;
  return DRYV_OK;
}

int dryv_inter_check_deblock(const dryv_frame_params* fp, const dryv_deblock_params* dp, uint32_t n_frames, int bipred,
                             uint32_t n_refs0, uint32_t n_refs1) {
  // the matching submit's checks (a P submit has one list), then build_dparams' checks of dp
  if (!bipred && n_refs1) return DRYV_E_INVALID;
  int st = dryv::inter::build_bparams(fp, n_frames, n_refs0, n_refs1, nullptr, nullptr);
  if (st != DRYV_OK) return st;
  dryv::deblock::DParams DP;
  int skip = 0;
  return dryv::deblock::build_dparams(fp, dp, n_frames, &DP, &skip);
}

int dryv_inter_deblock_device(dryv_inter_ctx* ctx, const dryv_frame_params* fp, const dryv_deblock_params* dp, uint32_t n_frames,
                              int bipred, uint32_t n_refs0, uint32_t n_refs1, const void* const* d_refs0, const void* const* d_refs1,
                              const void* d_mbs, const void* d_coeffs, void* d_yuv, void* d_bs_out) {
  if (!ctx || !d_refs0 || (n_refs1 && !d_refs1) || !d_mbs || !d_coeffs || !d_yuv) return DRYV_E_INVALID;
  int st = dryv_inter_check_deblock(fp, dp, n_frames, bipred, n_refs0, n_refs1);
  if (st != DRYV_OK) return st;
  IParams P;
  dryv::deblock::DParams DP;
  int skip = 0;
  (void)dryv::inter::build_iparams(fp, n_frames, n_refs0, &P);
  (void)dryv::deblock::build_dparams(fp, dp, n_frames, &DP, &skip);
  if (((uintptr_t)d_mbs | (uintptr_t)d_coeffs | (uintptr_t)d_yuv | (uintptr_t)d_bs_out) & 15u) return DRYV_E_INVALID;
  const size_t n0 = (size_t)n_frames * n_refs0, n1 = (size_t)n_frames * n_refs1;
  if (!refs_ok(d_refs0, n0) || !refs_ok(d_refs1, n1)) return DRYV_E_INVALID;
  if (skip) return DRYV_OK;  // disable_deblocking_filter_idc = 1
  (void)hipSetDevice(ctx->device);
  const size_t idBytes = (size_t)n_frames * 32, wsBytes = (dryv::deblock::workspace_bytes(DP) + 255) & ~(size_t)255;
  if ((st = ensure(ctx, ctx->ids, idBytes)) != DRYV_OK) return st;
  if (ctx->cap_dbwork < wsBytes + (size_t)P.n_mbs * 16) {
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return DRYV_E_DEVICE;   // (launches in flight may still use the old one)
    if (ctx->d_dbwork) (void)hipFree(ctx->d_dbwork);
    ctx->d_dbwork = nullptr;
    ctx->cap_dbwork = 0;
    if (hipMalloc(&ctx->d_dbwork, wsBytes + (size_t)P.n_mbs * 16) != hipSuccess) return DRYV_E_NOMEM;
    ctx->cap_dbwork = wsBytes + (size_t)P.n_mbs * 16;
  }
  if (ctx->tab_pending && hipEventSynchronize(ctx->ev_tab) != hipSuccess) return DRYV_E_DEVICE;
  // picture ids: position (list * 16 + refIdx) of the first entry of the picture's two tables with the same pointer
  uint8_t* ids = (uint8_t*)ctx->ids.h;
  memset(ids, 0xFF, idBytes);
  for (uint32_t f = 0; f < n_frames; f++) {
    const void* tab[32] = {};
    for (uint32_t k = 0; k < n_refs0; k++) tab[k] = d_refs0[(size_t)f * n_refs0 + k];
    for (uint32_t k = 0; k < n_refs1; k++) tab[16 + k] = d_refs1[(size_t)f * n_refs1 + k];
    for (int k = 0; k < 32; k++)
      if (tab[k]) ids[f * 32 + k] = (uint8_t)(std::find(tab, tab + 32, tab[k]) - tab);
  }
  if (hipMemcpyAsync(ctx->ids.d, ctx->ids.h, idBytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipEventRecord(ctx->ev_tab, ctx->stream) != hipSuccess)
    return DRYV_E_DEVICE;
  ctx->tab_pending = true;
  if (hipMemsetAsync(ctx->d_dbwork, 0, dryv::deblock::reset_bytes(DP), ctx->stream) != hipSuccess) return DRYV_E_DEVICE;
  void* d_bs = (unsigned char*)ctx->d_dbwork + wsBytes;
  if (dryv::inter::deblock_bs_launch(P, bipred != 0, d_mbs, d_coeffs, ctx->ids.d, d_bs, d_bs_out, ctx->stream, ctx->ev_bs_start,
                                     ctx->ev_bs_stop) != hipSuccess)
    return DRYV_E_DEVICE;
  // the whole resident grid, capped at one wave per band and plane kind
  const int wpb = dryv::inter::inter_deblock_waves_per_block();
  const long long bands = (long long)n_frames * ((DP.H + 3) / 4);
  const int grid = (int)std::max(1ll, std::min((long long)ctx->num_cus * dryv::inter::inter_deblock_blocks_per_cu(), (2 * bands + wpb - 1) / wpb));
  if (dryv::inter::inter_deblock_launch(DP, d_mbs, bipred ? 144u : 80u, d_bs, d_yuv, ctx->d_status, ctx->d_dbwork, grid, ctx->stream,
                                        ctx->ev_start, ctx->ev_stop) != hipSuccess)
    return DRYV_E_DEVICE;
  ctx->timed = ctx->deblock_timed = true;
  return DRYV_OK;
}

int dryv_inter_last_deblock_ms(dryv_inter_ctx* ctx, float* bs_ms, float* filter_ms) {
  if (!ctx || !bs_ms || !filter_ms) return DRYV_E_INVALID;
  if (!ctx->deblock_timed) return DRYV_E_STATE;
  if (hipEventSynchronize(ctx->ev_stop) != hipSuccess || hipEventElapsedTime(bs_ms, ctx->ev_bs_start, ctx->ev_bs_stop) != hipSuccess ||
      hipEventElapsedTime(filter_ms, ctx->ev_start, ctx->ev_stop) != hipSuccess)
    return DRYV_E_DEVICE;
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
  if (*ctx->h_status & dryv::kStatusGaveUp) return DRYV_E_DEVICE;   // (a band of the deblocking filter)
  return (*ctx->h_status & dryv::kStatusUnsupported) ? DRYV_E_UNSUPPORTED : DRYV_OK;
}

int dryv_inter_last_kernel_ms(dryv_inter_ctx* ctx, float* ms) {
  if (!ctx || !ms) return DRYV_E_INVALID;
  if (!ctx->timed) return DRYV_E_STATE;
  if (hipEventSynchronize(ctx->ev_stop) != hipSuccess || hipEventElapsedTime(ms, ctx->ev_start, ctx->ev_stop) != hipSuccess)
    return DRYV_E_DEVICE;
  return DRYV_OK;
}

}  // extern "C"
