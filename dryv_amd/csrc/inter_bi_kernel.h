// inter_bi_kernel.h — bi-predictive and weighted inter prediction for gfx950 (ITU-T H.264 8.4.2.3 over up to two predictions of
// 8.4.2.2 per partition): B macroblocks and weighted P macroblocks. The interpolation, the residual path and the output rows
// are inter_kernel.h's, on LDS addresses of this kernel's slice; what two lists add is here.
//
// One wave64 per macroblock, independent waves, as in the P kernel. Per macroblock:
//   1. the 144-byte record -> LDS; validation (wave-uniform); the vectors of quadrants that do not use a list are zeroed in
//      LDS (so that they neither split a window level nor wake an interpolation filter); lanes 0..7 fetch the (list, quadrant)
//      reference pointers, lanes 0..11 resolve the (quadrant, plane) weights of 8.4.2.3 into (w0 | w1 << 16, rnd, sh, off)
//   2. each list picks its own window level (21x21 / 13x13 / 9x9, inter_kernel.h) and stages into a window set of its own;
//      items of unused quadrants issue no loads, an unused list is skipped. Both lists' loads are requested before the one
//      wave_sync in front of the prediction: a bi-predicted macroblock has both in flight at once
//   3. the prediction of each used list, then per pixel Clip1(((p0 * w0 + p1 * w1 + rnd) >> sh) + off): the sum of products is
//      one v_dot2_i32_i16 on (p0 | p1 << 16) x (w0 | w1 << 16) with rnd as the accumulator. A wave whose every entry is the
//      default single-list case selects instead
//   4. residual, output rows, status: inter_kernel.h
#pragma once
#include "inter_kernel.h"

namespace dryv {
namespace inter {

// per-wave LDS slice (byte offsets)
constexpr int B_REC = 0;                     // the record: 144 bytes (vectors of list X at 16 + 64 X)
constexpr int B_REFP = 144;                  // [2][4] x 8: the quadrants' reference pictures per list
constexpr int B_WGT = B_REFP + 64;           // [4 quadrants][3 planes] x 16: w0 | w1 << 16, rnd, sh, off
constexpr int B_COEF = B_WGT + 192;          // i16 [384]
constexpr int B_WIN = B_COEF + 768;          // per list: luma windows (1728; list 0's are the 8x8 transform's scratch later), chroma (784)
constexpr int B_WINSET = 1728 + 784;         // one list's window set
constexpr int B_RESC = B_WIN + 2 * B_WINSET; // i16 [2][64]: chroma residual
constexpr int B_OUT = B_RESC + 256;          // u8 [256] Y, [64] Cb, [64] Cr
constexpr int B_BYTES = B_OUT + 384;         // 6832
static_assert(B_OUT + 384 - B_RESC >= 512, "list 0's samples wait here while list 1 is interpolated");
static_assert(B_BYTES % 16 == 0 && B_WGT % 16 == 0 && B_COEF % 16 == 0 && B_WIN % 16 == 0 && B_WINSET % 16 == 0 && B_OUT % 16 == 0,
              "16-byte LDS accesses");

typedef short i16x2 __attribute__((ext_vector_type(2)));
// a.lo * b.lo + a.hi * b.hi + acc on signed halves (v_dot2_i32_i16 / v_dot2c_i32_i16)
WV int dot2(unsigned a, unsigned b, int acc) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(i16x2, a), __builtin_bit_cast(i16x2, b), acc, false);
}

// 8.4.2.3 for quadrant q, plane pl (0 Y, 1 Cb, 2 Cr) with reference indices r0 / r1 (< 0: list unused; not both).
WV u32x4 resolve_weights(const dryv_inter_weights* wp, int pl, int r0, int r1) {
  const bool both = r0 >= 0 && r1 >= 0;
  int w0 = r0 >= 0 ? 1 : 0, w1 = r1 >= 0 ? 1 : 0, rnd = both ? 1 : 0, sh = both ? 1 : 0, off = 0;   // default (8.4.2.3.1)
  const int mode = wp ? (int)wp->mode : 0;
  if (mode == 1) {
    const int denom = pl == 0 ? (int)wp->luma_log2_denom : (int)wp->chroma_log2_denom;
    const int e0 = r0 >= 0 ? r0 : 0, e1 = r1 >= 0 ? r1 : 0;
    const int x0 = wp->expl[0][e0].w[pl], o0 = wp->expl[0][e0].o[pl], x1 = wp->expl[1][e1].w[pl], o1 = wp->expl[1][e1].o[pl];
    w0 = r0 >= 0 ? x0 : 0;
    w1 = r1 >= 0 ? x1 : 0;
    if (both) {
      rnd = 1 << denom;
      sh = denom + 1;
      off = (o0 + o1 + 1) >> 1;
    } else {
      rnd = denom >= 1 ? 1 << (denom - 1) : 0;
      sh = denom;
      off = r0 >= 0 ? o0 : o1;
    }
  } else if (mode == 2 && both) {
    w1 = wp->implicit_w1[r0][r1];
    w0 = 64 - w1;
    rnd = 32;
    sh = 6;
  }
  return (u32x4){((unsigned)w0 & 0xffffu) | (unsigned)w1 << 16, (unsigned)rnd, (unsigned)sh, (unsigned)off};
}

WV int weigh(unsigned p0, unsigned p1, u32x4 w) { return clip255((dot2(p0 | p1 << 16, w[0], (int)w[1]) >> (int)w[2]) + (int)w[3]); }

// The level of list X's windows (4 / 2 / 0 = log2 of blocks per window), wave-uniform. Vectors of unused quadrants are 0.
WV int list_level(int mvA, int lane, unsigned used, int myRef, int ref0) {
  const unsigned myMv = wv::lds_u32(mvA + 4 * (lane & 15));
  if (used == 0xfu && !wv::any(myMv != wv::lds_u32(mvA) || myRef != ref0)) return 4;
  return wv::any(myMv != wv::lds_u32(mvA + 4 * (lane & 12))) ? 0 : 2;
}

template <int LS>
WV void stage_list(int mvA, int refpA, int winA, int lane, unsigned used, int mbx, int mby, int wl, int hl, unsigned cOff, unsigned cStep) {
  stage<LS, false, true>(mvA, refpA, winA, lane, mbx, mby, wl, hl, 0u, 0u, used);
  stage<LS, true, true>(mvA, refpA, winA + 1728, lane, mbx, mby, wl >> 1, hl >> 1, cOff, cStep, used);
}

// One macroblock: index a of the batch.
WV void bi_mb(const IParams& P, const BArgs& A, int T, int S, int lane, int a) {
  const int per = P.W * P.H;
  const int f = a / per, within = a - f * per, mby = within / P.W, mbx = within - mby * P.W;
  const unsigned cOff = 256u * (unsigned)per, cStep = 64u * (unsigned)per;
  const OutGeo G = {A.yuv + (size_t)f * (size_t)per * 384u, 16u * (unsigned)P.W, cOff, cStep, mbx, mby};

  if (lane < 36) wv::lds_st32(S + B_REC + 4 * lane, ((const unsigned*)(A.mbs + a))[lane]);
  wv::wave_sync();
  const unsigned head = (unsigned)wv::rfl((int)wv::lds_u32(S + B_REC));
  const int qp = (int)((head >> 8) & 255u);
  const unsigned flags = (head >> 16) & 255u;
  // every lane: its quadrant's (lane & 3) two reference indices
  const int r0 = (int)(signed char)wv::lds_u8(S + B_REC + 4 + (lane & 3)), r1 = (int)(signed char)wv::lds_u8(S + B_REC + 8 + (lane & 3));
  const bool bad = (head & 255u) != 0u || qp > 51 || wv::any(r0 >= P.n_refs || r1 >= A.n_refs1 || (r0 < 0 && r1 < 0));
  if (bad) {   // outside the supported domain: zero-filled, reported; the reference tables are not read
    zero_fill(G, lane, A.status);
    return;
  }
  const unsigned used0 = (unsigned)wv::ballot(r0 >= 0) & 0xfu, used1 = (unsigned)wv::ballot(r1 >= 0) & 0xfu;   // lanes 0..3: quadrants
  if (lane < 8) {   // list lane >> 2, quadrant lane & 3
    const int X = lane >> 2, r = X ? r1 : r0;
    if (r >= 0) {
      const uint8_t* const* tab = X ? A.refs[1] : A.refs[0];
      const unsigned long long rp = (unsigned long long)tab[(size_t)f * (size_t)(X ? A.n_refs1 : P.n_refs) + (size_t)r];
      wv::lds_st64(S + B_REFP + 8 * lane, (u32x2){(unsigned)rp, (unsigned)(rp >> 32)});
    }
  }
  if (lane < 32 && !(((lane >> 4 ? used1 : used0) >> ((lane >> 2) & 3)) & 1u)) wv::lds_st32(S + B_REC + 16 + 4 * lane, 0u);
  if (lane < 12) {   // quadrant lane / 3, plane lane % 3
    const int q = lane / 3, pl = lane - 3 * q;
    const int q0 = (int)(signed char)wv::lds_u8(S + B_REC + 4 + q), q1 = (int)(signed char)wv::lds_u8(S + B_REC + 8 + q);
    wv::lds_st128(S + B_WGT + 16 * lane, resolve_weights(A.weights ? A.weights + f : nullptr, pl, q0, q1));
  }
  const bool hasRes = !(flags & 2u);
  u32x4 cq = {0u, 0u, 0u, 0u};
  if (hasRes && lane < 48) cq = ((const u32x4*)(A.coeffs + (size_t)a * 384u))[lane];
  wv::wave_sync();   // the reference pointers, the zeroed vectors, the weights

  const int mv0 = S + B_REC + 16, mv1 = mv0 + 64, win0 = S + B_WIN, win1 = win0 + B_WINSET;
  const int wl = 16 * P.W, hl = 16 * P.H;
  int lv0 = -1, lv1 = -1;   // (-1: no quadrant uses the list)
  if (used0) {
    lv0 = list_level(mv0, lane, used0, r0, (int)(signed char)wv::lds_u8(S + B_REC + 4));
    if (lv0 == 4) stage_list<4>(mv0, S + B_REFP, win0, lane, used0, mbx, mby, wl, hl, cOff, cStep);
    else if (lv0 == 2) stage_list<2>(mv0, S + B_REFP, win0, lane, used0, mbx, mby, wl, hl, cOff, cStep);
    else stage_list<0>(mv0, S + B_REFP, win0, lane, used0, mbx, mby, wl, hl, cOff, cStep);
  }
  if (used1) {
    lv1 = list_level(mv1, lane, used1, r1, (int)(signed char)wv::lds_u8(S + B_REC + 8));
    if (lv1 == 4) stage_list<4>(mv1, S + B_REFP + 32, win1, lane, used1, mbx, mby, wl, hl, cOff, cStep);
    else if (lv1 == 2) stage_list<2>(mv1, S + B_REFP + 32, win1, lane, used1, mbx, mby, wl, hl, cOff, cStep);
    else stage_list<0>(mv1, S + B_REFP + 32, win1, lane, used1, mbx, mby, wl, hl, cOff, cStep);
  }
  wv::wave_sync();   // both lists' windows
  // (registers: the interpolation is the kernel's peak; what it need not carry waits in lane-private LDS: the coefficients,
  // which have landed with the windows, in their place, list 0's samples (512 bytes) over B_RESC and B_OUT)
  const bool anyRes = wv::any((cq[0] | cq[1] | cq[2] | cq[3]) != 0u);   // (never under flag bit1: cq is 0 then)
  if (anyRes && lane < 48) wv::lds_st128(S + B_COEF + 16 * lane, cq);
  unsigned y0 = 0u, c0 = 0u, y1 = 0u, c1 = 0u;
  if (lv0 == 4) predict<4>(mv0, win0, win0 + 1728, lane, mbx, mby, &y0, &c0);
  else if (lv0 == 2) predict<2>(mv0, win0, win0 + 1728, lane, mbx, mby, &y0, &c0);
  else if (lv0 == 0) predict<0>(mv0, win0, win0 + 1728, lane, mbx, mby, &y0, &c0);
  if (used1) wv::lds_st64(S + B_RESC + 8 * lane, (u32x2){y0, c0});
  if (lv1 == 4) predict<4>(mv1, win1, win1 + 1728, lane, mbx, mby, &y1, &c1);
  else if (lv1 == 2) predict<2>(mv1, win1, win1 + 1728, lane, mbx, mby, &y1, &c1);
  else if (lv1 == 0) predict<0>(mv1, win1, win1 + 1728, lane, mbx, mby, &y1, &c1);
  if (used1) {
    const u32x2 v = wv::lds_u64(S + B_RESC + 8 * lane);
    y0 = v[0];
    c0 = v[1];
  }

  // 8.4.2.3: the luma lane's quadrant is lane >> 4, the chroma lane's (lane & 31) >> 3 in plane 1 + (lane >> 5)
  const u32x4 wy = wv::lds_u128(S + B_WGT + 16 * (3 * (lane >> 4))), wc = wv::lds_u128(S + B_WGT + 16 * (3 * ((lane & 31) >> 3) + 1 + (lane >> 5)));
  const bool plainY = (wy[0] == 1u || wy[0] == 0x10000u) && (wy[1] | wy[2] | wy[3]) == 0u;
  const bool plainC = (wc[0] == 1u || wc[0] == 0x10000u) && (wc[1] | wc[2] | wc[3]) == 0u;
  unsigned predY, predC;
  if (wv::any(!plainY || !plainC)) {
    predY = predC = 0u;
#pragma unroll
    for (int p = 0; p < 4; p++) predY |= (unsigned)weigh((y0 >> (8 * p)) & 255u, (y1 >> (8 * p)) & 255u, wy) << (8 * p);
#pragma unroll
    for (int p = 0; p < 2; p++) predC |= (unsigned)weigh((c0 >> (8 * p)) & 255u, (c1 >> (8 * p)) & 255u, wc) << (8 * p);
  } else {   // every lane: the one list's samples as they are
    predY = wy[0] == 1u ? y0 : y1;
    predC = wc[0] == 1u ? c0 : c1;
  }
  wv::wave_sync();   // the windows are read: list 0's luma windows are the 8x8 transform's scratch from here on

  if (anyRes) add_residual(S + B_COEF, win0, S + B_RESC, T, lane, qp, flags, wv::lds_u128(S + B_COEF + 16 * (lane < 48 ? lane : 0)), &predY, &predC);
  write_out(G, S + B_OUT, lane, predY, predC);
}

// The wave's loop: macroblocks first, first + stride, ...
WV void bi_wave(const IParams& P, const BArgs& A, int T, int S, int first, int stride) {
  const int lane = wv::lane_id();
  for (long long a = first; a < (long long)P.n_mbs; a += stride) {
    bi_mb(P, A, T, S, lane, (int)a);
    wv::wave_sync();   // the slice is the next macroblock's
  }
}

}  // namespace inter
}  // namespace dryv
