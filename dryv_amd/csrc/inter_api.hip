// inter_api.hip — the extern "C" boundary of the inter prediction stage (include/dryv_recon.h: dryv_inter_*): a stage object
// of its own next to dryv_recon_ctx, on a stream of its own or on a borrowed one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <new>

#include "deblock_params.h"
#include "inter_launch.h"
#include "status_words.h"

using dryv::deblock::DParams;
using dryv::inter::Args;
using dryv::inter::BArgs;
using dryv::inter::IParams;

// Grow-only device memory (ensure()) with a pinned staging side where the host fills it (stage()): a device copy is replaced in
// stream order, behind the launch that read it; the staging waits for its own copy.
struct Staged {
  void* h = nullptr;
  void* d = nullptr;
  size_t cap = 0;   // bytes
};

struct dryv_inter_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;   // the most recent launch's own start and end
  hipEvent_t ev_tab = nullptr;                        // the most recent call's copies have left the staging buffers
  bool timed = false, tab_pending = false;
  unsigned* d_status = nullptr;
  unsigned* h_status = nullptr;   // pinned
  // what the most recent call copied in: the reference table (list 0's for a bi-predictive submit), list 1's table, the
  // pictures' weights, the deblocking call's picture-id tables ([n_frames][2][16] bytes)
  Staged refs, refs1, weights, ids;
  // deblocking workspace, device only: [the filter's counters, progress words and side buffers (deblock_params.h)]
  // [one dryv_bs_rec per macroblock]
  Staged dbwork;
  hipEvent_t ev_bs_start = nullptr, ev_bs_stop = nullptr;   // the most recent boundary-strength launch's own start and end
  bool deblock_timed = false;
  int num_cus = 256;
};

namespace {

void release(Staged& s) {
  if (s.h) (void)hipHostFree(s.h);
  if (s.d) (void)hipFree(s.d);
  s = Staged();
}

// The one grow path: s.d (and s.h, unless device_only) hold at least `bytes` afterwards.
int ensure(dryv_inter_ctx* ctx, Staged& s, size_t bytes, bool device_only = false) {
  if (s.cap >= bytes) return DRYV_OK;
  // (the old copy may still be read by launches in flight)
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return DRYV_E_DEVICE;
  release(s);
  ctx->tab_pending = false;
  const size_t cap = device_only ? bytes : std::max<size_t>(bytes, 8192);
  if ((!device_only && hipHostMalloc(&s.h, cap, hipHostMallocDefault) != hipSuccess) || hipMalloc(&s.d, cap) != hipSuccess) return DRYV_E_NOMEM;
  s.cap = cap;
  return DRYV_OK;
}

struct Table {
  Staged* s;
  const void* src;   // host; NULL: `fill` writes s->h in place
  size_t bytes;      // 0: not part of this call, nothing is copied
};

// The one staging path, host tables -> device copies in stream order: grow where needed; one wait until the previous call's
// copies have left the pinned side; the host copies (and `fill`); the async copies; one event behind them.
template <class Fill = void (*)()>
int stage(dryv_inter_ctx* ctx, std::initializer_list<Table> tabs, Fill fill = [] {}) {
  for (const Table& t : tabs) {
    const int st = ensure(ctx, *t.s, t.bytes);
    if (st != DRYV_OK) return st;
  }
  if (ctx->tab_pending && hipEventSynchronize(ctx->ev_tab) != hipSuccess) return DRYV_E_DEVICE;
  for (const Table& t : tabs)
    if (t.bytes && t.src) memcpy(t.s->h, t.src, t.bytes);
  fill();
  for (const Table& t : tabs)
    if (t.bytes && hipMemcpyAsync(t.s->d, t.s->h, t.bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return DRYV_E_DEVICE;
  if (hipEventRecord(ctx->ev_tab, ctx->stream) != hipSuccess) return DRYV_E_DEVICE;
  ctx->tab_pending = true;
  return DRYV_OK;
}

// The argument checks of the three launching entry points, in the order that decides which status wins: everything required
// is present; the entry point's own parameter checks passed (params_st: its build_*'s status); the buffers (`optional` may be
// NULL) and every entry of the reference tables (n0 / n1 entries; a P submit has list 0 only) are 16-byte aligned: 16-byte
// loads of records and coefficients, 16-byte stores of the rows, aligned dword loads of the references.
int check_args(const dryv_inter_ctx* ctx, int params_st, std::initializer_list<const void*> required, const void* optional,
               const void* const* refs0, size_t n0, const void* const* refs1, size_t n1) {
  bool present = ctx && refs0 && (!n1 || refs1);
  uintptr_t bits = (uintptr_t)optional;
  for (const void* p : required) present = present && p, bits |= (uintptr_t)p;
  if (!present) return DRYV_E_INVALID;
  if (params_st != DRYV_OK) return params_st;
  for (size_t k = 0; k < n0 + n1; k++) {
    const void* ref = k < n0 ? refs0[k] : refs1[k - n0];
    if (!ref) return DRYV_E_INVALID;
    bits |= (uintptr_t)ref;
  }
  return (bits & 15u) ? DRYV_E_INVALID : DRYV_OK;
}

// Validation and parameter blocks of the deblocking call: the matching submit's checks (a P submit has one list), then
// build_dparams' checks of dp. P may be NULL.
int build_deblock(const dryv_frame_params* fp, const dryv_deblock_params* dp, uint32_t n_frames, int bipred, uint32_t n_refs0,
                  uint32_t n_refs1, IParams* P, DParams* DP, int* skip) {
  if (!bipred && n_refs1) return DRYV_E_INVALID;
  const int st = dryv::inter::build_bparams(fp, n_frames, n_refs0, n_refs1, nullptr, P);
  return st != DRYV_OK ? st : dryv::deblock::build_dparams(fp, dp, n_frames, DP, skip);
}

// the persistent grid of a kernel with wpb waves per workgroup and room for per_cu workgroups on a CU, for n_waves waves' worth
// of work (the waves stride over it: a smaller grid is merely slower, a larger one idles)
int grid_for(const dryv_inter_ctx* ctx, long long n_waves, int wpb, int per_cu) {
  return (int)std::max(1ll, std::min((n_waves + wpb - 1) / wpb, (long long)ctx->num_cus * per_cu));
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
  bool ok = hipMalloc((void**)&ctx->d_status, 16) == hipSuccess && hipMemset(ctx->d_status, 0, 16) == hipSuccess &&
            hipHostMalloc((void**)&ctx->h_status, 16, hipHostMallocDefault) == hipSuccess;
  for (hipEvent_t* e : {&ctx->ev_start, &ctx->ev_stop, &ctx->ev_bs_start, &ctx->ev_bs_stop}) ok = ok && hipEventCreate(e) == hipSuccess;
  if (!ok || hipEventCreateWithFlags(&ctx->ev_tab, hipEventDisableTiming) != hipSuccess) {
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
  for (Staged* s : {&ctx->refs, &ctx->refs1, &ctx->weights, &ctx->ids, &ctx->dbwork}) release(*s);
  if (ctx->d_status) (void)hipFree(ctx->d_status);
  if (ctx->h_status) (void)hipHostFree(ctx->h_status);
  for (hipEvent_t e : {ctx->ev_start, ctx->ev_stop, ctx->ev_bs_start, ctx->ev_bs_stop, ctx->ev_tab})
    if (e) (void)hipEventDestroy(e);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int dryv_inter_submit_device(dryv_inter_ctx* ctx, const dryv_frame_params* fp, uint32_t n_frames, uint32_t n_refs,
                             const void* const* d_refs, const void* d_mbs, const void* d_coeffs, void* d_yuv_out) {
  IParams P;
  const size_t n_tab = (size_t)n_frames * n_refs;
  int st = check_args(ctx, dryv::inter::build_iparams(fp, n_frames, n_refs, &P), {d_mbs, d_coeffs, d_yuv_out}, nullptr, d_refs, n_tab, nullptr, 0);
  if (st != DRYV_OK) return st;
  (void)hipSetDevice(ctx->device);
  if ((st = stage(ctx, {{&ctx->refs, d_refs, n_tab * sizeof(void*)}})) != DRYV_OK) return st;
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
  IParams P;
  const size_t n0 = (size_t)n_frames * n_refs0, n1 = (size_t)n_frames * n_refs1, wb = weights ? (size_t)n_frames * sizeof(dryv_inter_weights) : 0;
  int st = check_args(ctx, dryv::inter::build_bparams(fp, n_frames, n_refs0, n_refs1, weights, &P), {d_mbs, d_coeffs, d_yuv_out}, nullptr,
                      d_refs0, n0, d_refs1, n1);
  if (st != DRYV_OK) return st;
  (void)hipSetDevice(ctx->device);
  if ((st = stage(ctx, {{&ctx->refs, d_refs0, n0 * sizeof(void*)}, {&ctx->refs1, d_refs1, n1 * sizeof(void*)}, {&ctx->weights, weights, wb}})) != DRYV_OK)
    return st;
  BArgs A;
  A.refs[0] = (const uint8_t* const*)ctx->refs.d;
  A.refs[1] = n_refs1 ? (const uint8_t* const*)ctx->refs1.d : nullptr;
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
  DParams DP;
  int skip = 0;
  return build_deblock(fp, dp, n_frames, bipred, n_refs0, n_refs1, nullptr, &DP, &skip);
}

int dryv_inter_deblock_device(dryv_inter_ctx* ctx, const dryv_frame_params* fp, const dryv_deblock_params* dp, uint32_t n_frames,
                              int bipred, uint32_t n_refs0, uint32_t n_refs1, const void* const* d_refs0, const void* const* d_refs1,
                              const void* d_mbs, const void* d_coeffs, void* d_yuv, void* d_bs_out) {
  IParams P;
  DParams DP;
  int skip = 0;
  int st = check_args(ctx, build_deblock(fp, dp, n_frames, bipred, n_refs0, n_refs1, &P, &DP, &skip), {d_mbs, d_coeffs, d_yuv}, d_bs_out,
                      d_refs0, (size_t)n_frames * n_refs0, d_refs1, (size_t)n_frames * n_refs1);
  if (st != DRYV_OK) return st;
  if (skip) return DRYV_OK;  // disable_deblocking_filter_idc = 1
  (void)hipSetDevice(ctx->device);
  const size_t idBytes = (size_t)n_frames * 32, wsBytes = (dryv::deblock::workspace_bytes(DP) + 255) & ~(size_t)255;
  if ((st = ensure(ctx, ctx->dbwork, wsBytes + (size_t)P.n_mbs * 16, true)) != DRYV_OK) return st;
  // picture ids: position (list * 16 + refIdx) of the first entry of the picture's two tables with the same pointer
  st = stage(ctx, {{&ctx->ids, nullptr, idBytes}}, [&] {
    uint8_t* ids = (uint8_t*)ctx->ids.h;
    memset(ids, 0xFF, idBytes);
    for (uint32_t f = 0; f < n_frames; f++) {
      const void* tab[32] = {};
      for (uint32_t k = 0; k < n_refs0; k++) tab[k] = d_refs0[(size_t)f * n_refs0 + k];
      for (uint32_t k = 0; k < n_refs1; k++) tab[16 + k] = d_refs1[(size_t)f * n_refs1 + k];
      for (int k = 0; k < 32; k++)
        if (tab[k]) ids[f * 32 + k] = (uint8_t)(std::find(tab, tab + 32, tab[k]) - tab);
    }
  });
  if (st != DRYV_OK) return st;
  if (hipMemsetAsync(ctx->dbwork.d, 0, dryv::deblock::reset_bytes(DP), ctx->stream) != hipSuccess) return DRYV_E_DEVICE;
  void* d_bs = (unsigned char*)ctx->dbwork.d + wsBytes;
  if (dryv::inter::deblock_bs_launch(P, bipred != 0, d_mbs, d_coeffs, ctx->ids.d, d_bs, d_bs_out, ctx->stream, ctx->ev_bs_start,
                                     ctx->ev_bs_stop) != hipSuccess)
    return DRYV_E_DEVICE;
  // the whole resident grid, capped at one wave per band and plane kind
  const long long bands = (long long)n_frames * ((DP.H + 3) / 4);
  const int grid = grid_for(ctx, 2 * bands, dryv::inter::inter_deblock_waves_per_block(), dryv::inter::inter_deblock_blocks_per_cu());
  if (dryv::inter::inter_deblock_launch(DP, d_mbs, bipred ? 144u : 80u, d_bs, d_yuv, ctx->d_status, ctx->dbwork.d, grid, ctx->stream,
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
