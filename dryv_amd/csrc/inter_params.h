// inter_params.h — the constant block a launch of the inter prediction kernel (inter_kernel.h) gets, and its host-side
// derivation from a dryv_frame_params. Plain C++ (no HIP).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/dryv_recon.h"
#include "recon_params.h"

namespace dryv {
namespace inter {

// Per-workgroup LDS tables (byte offsets), copied from IParams::tab once per workgroup.
constexpr int T_LS4 = 0;              // u16 [3 (Y, Cb, Cr: scaling lists 3, 4, 5)][6 (qp % 6)][16]: LevelScale4x4 in zig-zag LIST order
constexpr int T_LS8 = T_LS4 + 576;    // u16 [6][64]: LevelScale8x8 of scaling list 1 (8x8 inter Y), LIST order
constexpr int T_ZZ8I = T_LS8 + 768;   // u8 [64]: raster position i * 8 + j -> index in the 8x8 zig-zag list
constexpr int T_QPC = T_ZZ8I + 64;    // u8 [2 (Cb, Cr)][52]: QPc of QPY with the plane's chroma_qp_index_offset (8.5.8), padded to 112
constexpr int T_END = T_QPC + 112;    // 1520

struct IParams {
  int W, H;          // picture size in macroblocks
  int n_mbs;         // n_frames * W * H
  int n_refs;        // reference pictures per frame, 1..16
  unsigned tab[T_END / 4];
};

struct Args {
  const uint8_t* const* refs;   // device copy of the caller's table: [n_frames][n_refs] reference pictures
  const dryv_inter_mb* mbs;
  const int16_t* coeffs;
  uint8_t* yuv;
  unsigned* status;             // bit 0: a record outside the supported domain
};

// The bi-predictive / weighted kernel's (inter_bi_kernel.h); n_refs0 is IParams::n_refs.
struct BArgs {
  const uint8_t* const* refs[2];       // device copies of the caller's tables: [n_frames][n_refsX]
  const dryv_inter_weights* weights;   // device copy, [n_frames]; NULL: default prediction everywhere
  const dryv_inter_bmb* mbs;
  const int16_t* coeffs;
  uint8_t* yuv;
  unsigned* status;                    // bit 0: a record outside the supported domain
  int n_refs1;                         // 0..16
};

// dryv_recon_check_params + the bound on n_refs; fills P when given.
inline int build_iparams(const dryv_frame_params* fp, uint32_t n_frames, uint32_t n_refs, IParams* P) {
  KParams K;
  const int st = params::build_params(fp, n_frames, &K);
  if (st != DRYV_OK) return st;
  if (n_refs < 1 || n_refs > 16) return DRYV_E_INVALID;
  if (!P) return DRYV_OK;
  memset(P, 0, sizeof(*P));
  P->W = K.W;
  P->H = K.H;
  P->n_mbs = K.n_frames * K.W * K.H;
  P->n_refs = (int)n_refs;
  unsigned char* t = (unsigned char*)P->tab;
  static const int V4[6][3] = {{10, 16, 13}, {11, 18, 14}, {13, 20, 16}, {14, 23, 18}, {16, 25, 20}, {18, 29, 23}};
  static const int V8[6][6] = {{20, 18, 32, 19, 25, 24}, {22, 19, 35, 21, 28, 26}, {26, 23, 42, 24, 33, 31},
                               {28, 25, 45, 26, 35, 33}, {32, 28, 51, 30, 40, 38}, {36, 32, 58, 34, 46, 43}};
  uint16_t* ls4 = (uint16_t*)(t + T_LS4);
  uint16_t* ls8 = (uint16_t*)(t + T_LS8);
  for (int l = 0; l < 3; l++)
    for (int m = 0; m < 6; m++)
      for (int k = 0; k < 16; k++) {
        const int i = params::ZZ4[k][0], j = params::ZZ4[k][1];
        const int cls = (i % 2 == 0 && j % 2 == 0) ? 0 : ((i % 2 == 1 && j % 2 == 1) ? 1 : 2);
        ls4[(l * 6 + m) * 16 + k] = (uint16_t)(fp->scaling_list4x4[3 + l][k] * V4[m][cls]);
      }
  for (int m = 0; m < 6; m++)
    for (int k = 0; k < 64; k++) {
      const int i = params::ZZ8[k][0], j = params::ZZ8[k][1];
      int cls;
      if (i % 4 == 0 && j % 4 == 0) cls = 0;
      else if (i % 2 == 1 && j % 2 == 1) cls = 1;
      else if (i % 4 == 2 && j % 4 == 2) cls = 2;
      else if ((i % 4 == 0 && j % 2 == 1) || (i % 2 == 1 && j % 4 == 0)) cls = 3;
      else if ((i % 4 == 0 && j % 4 == 2) || (i % 4 == 2 && j % 4 == 0)) cls = 4;
      else cls = 5;
      ls8[m * 64 + k] = (uint16_t)(fp->scaling_list8x8[1][k] * V8[m][cls]);
    }
  for (int k = 0; k < 64; k++) t[T_ZZ8I + params::ZZ8[k][0] * 8 + params::ZZ8[k][1]] = (uint8_t)k;
  static const uint8_t QPC[22] = {29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39};  // table 8-15
  for (int pl = 0; pl < 2; pl++)
    for (int qp = 0; qp < 52; qp++) {
      const int qpi = std::min(std::max(qp + (pl ? K.cqo_cr : K.cqo_cb), 0), 51);
      t[T_QPC + pl * 52 + qp] = (uint8_t)(qpi < 30 ? qpi : QPC[qpi - 30]);
    }
  return DRYV_OK;
}

// The same for the bi-predictive entry points: n_refs0 1..16, n_refs1 0..16, and the weights (host, [n_frames], or NULL) within
// what the kernel shifts by and indexes with.
inline int build_bparams(const dryv_frame_params* fp, uint32_t n_frames, uint32_t n_refs0, uint32_t n_refs1,
                         const dryv_inter_weights* weights, IParams* P) {
  const int st = build_iparams(fp, n_frames, n_refs0, P);
  if (st != DRYV_OK) return st;
  if (n_refs1 > 16) return DRYV_E_INVALID;
  for (uint32_t f = 0; weights && f < n_frames; f++) {
    if (weights[f].mode > 2) return DRYV_E_INVALID;
    if (weights[f].mode == 1 && (weights[f].luma_log2_denom > 7 || weights[f].chroma_log2_denom > 7)) return DRYV_E_INVALID;
  }
  return DRYV_OK;
}

}  // namespace inter
}  // namespace dryv
