// inter_kernel.h — motion-compensated reconstruction of P macroblocks for gfx950 (ITU-T H.264 8.4.2.2, 8.5.8 - 8.5.13).
//
// One wave64 per macroblock, the waves of a workgroup stride over the batch and never talk to each other (one barrier, behind
// the per-workgroup tables). A wave works in an LDS slice of its own:
//   1. the 80-byte record -> LDS; validation (wave-uniform); the four reference pointers -> LDS; the 768 bytes of coefficients
//      are requested (one 16-byte load on lanes 0..47) and land while the windows are staged
//   2. the reference windows -> LDS, at one of three wave-uniform levels: all 16 vectors and 4 references equal: ONE 21x21 luma
//      window (+ 9x9 per chroma plane); else every quadrant's four vectors equal: four 13x13 (5x5); else sixteen 9x9 (3x3).
//      A window is staged as the aligned dwords that cover it, row by row; rows are clamped by index; a dword that lies inside
//      [0, width) is one aligned load, any other is gathered byte-wise with clamped x (picture borders only)
//   3. luma: lane l owns row l & 3 of 4x4 block l >> 2 (four pixels); it reads six window rows of 12 bytes, filters them with
//      the 6-tap (1, -5, 20, 20, -5, 1) on packed bytes (v_perm_b32 + v_dot4_u32_u8 + v_sad_u8 horizontally, packed 16-bit
//      vertically, 32-bit for the centre sample j) and picks / averages per table 8-12 by its block's own fractional position
//      chroma: lanes 0..31 Cb, 32..63 Cr, two pixels each; the eighth-sample bilinear is one v_dot4_u32_u8 per pixel
//   4. residual (skipped under flag bit1 and when the wave-wide OR of the coefficients is zero): LevelScale from the LDS
//      table, 4x4 butterflies with rows in-lane and columns across the block's four lanes (DPP quad_perm), 8x8 per quadrant
//      through LDS (rows, then columns, eight lanes each), chroma DC Hadamard + AC on lanes 0..31
//   5. prediction + residual, clip -> LDS -> sixteen 16-byte luma rows and sixteen 8-byte chroma rows
// All arithmetic is 32 bit (see include/dryv_recon.h).
#pragma once
#include "wave.h"
#include "inter_params.h"

namespace dryv {
namespace inter {

// per-wave LDS slice (byte offsets)
constexpr int S_REC = 0;                    // the record: 80 bytes
constexpr int S_REFP = 80;                  // 4 x 8: the quadrants' reference pictures
constexpr int S_COEF = 112;                 // i16 [384]
constexpr int S_LWIN = S_COEF + 768;        // luma windows: 21 x 24 | 4 x 13 x 16 | 16 x 9 x 12 (1728); then the 8x8 transform's scratch
constexpr int S_CWIN = S_LWIN + 1728;       // chroma windows, per plane 9 x 12 | 4 x 5 x 8 | 16 x 3 x 8 (384); + 16: the last row's second dword
constexpr int S_RESC = S_CWIN + 768 + 16;   // i16 [2][64]: chroma residual
constexpr int S_OUT = S_RESC + 256;         // u8 [256] Y, [64] Cb, [64] Cr: the reconstructed macroblock
constexpr int S_BYTES = S_OUT + 384;        // 4032
// over the luma windows, once they are read: i32 [4][64], the 8x8 rows after the first pass; at + 1024 i16 [4][64]: 8x8 residual
static_assert(S_BYTES % 16 == 0 && S_COEF % 16 == 0 && S_LWIN % 16 == 0 && S_OUT % 16 == 0, "16-byte LDS accesses");

WV void build_tables(const IParams& P, int ldsBase, int tid, int nthreads) {
  for (int k = tid; k < T_END / 4; k += nthreads) wv::lds_st32(ldsBase + 4 * k, P.tab[k]);
}

// (x, y) of 4x4 block b inside the macroblock (figure 6-10)
WV int blk_x(int b) { return ((b & 1) << 2) | ((b & 4) << 1); }
WV int blk_y(int b) { return ((b & 2) << 1) | (b & 8); }

// geometry of a window level; LS = log2(blocks per window)
template <int LS> struct Geo;
template <> struct Geo<4> { static constexpr int ROWS = 21, ND = 6, CROWS = 9, CND = 3, MASK = 12; };
template <> struct Geo<2> { static constexpr int ROWS = 13, ND = 4, CROWS = 5, CND = 2, MASK = 4; };
template <> struct Geo<0> { static constexpr int ROWS = 9, ND = 3, CROWS = 3, CND = 2, MASK = 0; };

// One dword of a window row: bytes x .. x + 3 of row p (x a multiple of 4, anywhere), samples outside [0, wp) clamped.
WV unsigned fetch_dword(const uint8_t* p, int x, int wp) {
  if (x >= 0 && x + 3 < wp) return *(const unsigned*)(p + x);
  unsigned v = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) v |= (unsigned)p[min(max(x + k, 0), wp - 1)] << (8 * k);
  return v;
}

// Stages the windows of one plane kind. Luma: window w covers blocks w << LS .. of the macroblock, origin 2 left of and 2
// above the first block's integer position, Geo::ROWS rows of Geo::ND dwords from the aligned x at or below the origin.
// Chroma (both planes, items interleaved): origin at the integer position. mvA: LDS address of the sixteen vectors; refpA: of the
// four quadrants' reference pointers; winA: of the windows. MASKED: items of a quadrant whose bit in `used` is clear are
// neither loaded nor stored.
template <int LS, bool CHROMA, bool MASKED = false>
WV void stage(int mvA, int refpA, int winA, int lane, int mbx, int mby, int wpix, int hpix, unsigned planeOff, unsigned planeStep,
              unsigned used = 0xfu) {
  using G = Geo<LS>;
  constexpr int ROWS = CHROMA ? G::CROWS : G::ROWS, ND = CHROMA ? G::CND : G::ND;
  constexpr int NWIN = 16 >> LS, PER = NWIN * ROWS * ND, N = CHROMA ? 2 * PER : PER;
  for (int i = lane; i < N; i += 64) {
    const int pl = CHROMA ? i / PER : 0, r0 = i - pl * PER;
    const int w = r0 / (ROWS * ND), r1 = r0 - w * (ROWS * ND), row = r1 / ND, dw = r1 - row * ND;
    const int b = w << LS;
    if (MASKED && !((used >> (b >> 2)) & 1u)) continue;
    const unsigned mv = wv::lds_u32(mvA + 4 * b);
    const int mvx = (int)(short)(mv & 0xffffu), mvy = (int)mv >> 16;
    const u32x2 rp = wv::lds_u64(refpA + 8 * (b >> 2));
    const uint8_t* ref = (const uint8_t*)(((unsigned long long)rp[1] << 32) | rp[0]);
    int x0, y0;
    if (CHROMA) {
      x0 = mbx * 8 + (blk_x(b) >> 1) + (mvx >> 3);
      y0 = mby * 8 + (blk_y(b) >> 1) + (mvy >> 3);
    } else {
      x0 = mbx * 16 + blk_x(b) + (mvx >> 2) - 2;
      y0 = mby * 16 + blk_y(b) + (mvy >> 2) - 2;
    }
    const int yy = min(max(y0 + row, 0), hpix - 1);
    const uint8_t* p = ref + (size_t)planeOff + (size_t)pl * planeStep + (size_t)((unsigned)yy * (unsigned)wpix);
    const unsigned v = fetch_dword(p, (x0 & ~3) + 4 * dw, wpix);
    wv::lds_st32(winA + ((pl * NWIN + w) * ROWS + row) * (ND * 4) + 4 * dw, v);
  }
}

// 6-tap on bytes p .. p + 5 of the 12 bytes {w2, w1, w0}, unrounded: the positive taps as one dot4 on a perm window, the
// negative pair as a byte sum
template <int PX>
WV int tap6(unsigned w0, unsigned w1, unsigned w2) {
  const unsigned lo = PX ? wv::alignbit(w1, w0, 8 * PX) : w0, hi = PX ? wv::alignbit(w2, w1, 8 * PX) : w1;
  const unsigned pos = wv::perm(hi, lo, 0x05030200u), neg = wv::perm(hi, lo, 0x0c0c0401u);
  return (int)wv::dot4(pos, 0x01141401u, 0u) - 5 * (int)wv::sum4(neg, 0u);
}
WV int clip255(int v) { return wv::med3(v, 0, 255); }
WV int lo16(unsigned v) { return (int)(v << 16) >> 16; }
WV int hi16(unsigned v) { return (int)v >> 16; }
WV int pick4(int code, int a, int b, int c, int d) { return code == 0 ? a : code == 1 ? b : code == 2 ? c : d; }

// 8.4.2.2.1: the lane's four luma prediction samples (packed bytes). A: LDS address of the lane's first window row (the row 2
// above its own), at the dword that holds the byte 2 left of its first pixel; sh: that byte's position in the dword.
WV unsigned luma_pred(int A, int pitch, int sh, int xf, int yf) {
  unsigned w0[6], w1[6], w2[6];
  const unsigned s8 = 8u * (unsigned)sh;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const unsigned d0 = wv::lds_u32(A + k * pitch), d1 = wv::lds_u32(A + k * pitch + 4), d2 = wv::lds_u32(A + k * pitch + 8);
    w0[k] = wv::alignbit(d1, d0, s8);
    w1[k] = wv::alignbit(d2, d1, s8);
    w2[k] = d2 >> s8;
  }
  // which of the integer sample I, the half samples H (b / s), V (h / m) and the centre J the position takes (table 8-12):
  // two 2-bit codes per position yf * 4 + xf; a position that is one of them alone names it twice
  const int idx = 2 * (yf * 4 + xf);
  const int ca = (int)((0x54BA5410u >> idx) & 3u), cb = (int)((0xBAFEBA54u >> idx) & 3u);
  const bool needH = ca == 1 || cb == 1, needV = ca == 2 || cb == 2, needJ = cb == 3;
  int H[4] = {0, 0, 0, 0}, V[4] = {0, 0, 0, 0}, J[4] = {0, 0, 0, 0};
  if (wv::any(needH)) {   // b on the lane's own row, or s one row on (yf == 3)
    const bool dn = yf == 3;
    const unsigned a0 = dn ? w0[3] : w0[2], a1 = dn ? w1[3] : w1[2], a2 = dn ? w2[3] : w2[2];
    H[0] = clip255((tap6<0>(a0, a1, a2) + 16) >> 5);
    H[1] = clip255((tap6<1>(a0, a1, a2) + 16) >> 5);
    H[2] = clip255((tap6<2>(a0, a1, a2) + 16) >> 5);
    H[3] = clip255((tap6<3>(a0, a1, a2) + 16) >> 5);
  }
  if (wv::any(needV)) {   // h in the lane's own columns, or m one column on (xf == 3): packed 16-bit, |value| <= 10710
    const unsigned cs = xf == 3 ? 24u : 16u;
    unsigned pl[6], ph[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const unsigned g = wv::alignbit(w1[k], w0[k], cs);
      pl[k] = wv::perm(0u, g, 0x0c010c00u);
      ph[k] = wv::perm(0u, g, 0x0c030c02u);
    }
    const unsigned vl = wv::pk_sub(wv::pk_mad(wv::pk_add(pl[2], pl[3]), 0x00140014u, wv::pk_add(pl[0], pl[5])),
                                   wv::pk_mad(wv::pk_add(pl[1], pl[4]), 0x00050005u, 0u));
    const unsigned vh = wv::pk_sub(wv::pk_mad(wv::pk_add(ph[2], ph[3]), 0x00140014u, wv::pk_add(ph[0], ph[5])),
                                   wv::pk_mad(wv::pk_add(ph[1], ph[4]), 0x00050005u, 0u));
    V[0] = clip255((lo16(vl) + 16) >> 5);
    V[1] = clip255((hi16(vl) + 16) >> 5);
    V[2] = clip255((lo16(vh) + 16) >> 5);
    V[3] = clip255((hi16(vh) + 16) >> 5);
  }
  if (wv::any(needJ)) {   // j: the 6-tap down the unrounded horizontal intermediates
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const int c = (k == 0 || k == 5) ? 1 : (k == 1 || k == 4) ? -5 : 20;
      J[0] += c * tap6<0>(w0[k], w1[k], w2[k]);
      J[1] += c * tap6<1>(w0[k], w1[k], w2[k]);
      J[2] += c * tap6<2>(w0[k], w1[k], w2[k]);
      J[3] += c * tap6<3>(w0[k], w1[k], w2[k]);
    }
#pragma unroll
    for (int p = 0; p < 4; p++) J[p] = clip255((J[p] + 512) >> 10);
  }
  // the integer sample: G, or H one column on (xf == 3, yf == 0), or M one row on (xf == 0, yf == 3)
  const bool dn = xf == 0 && yf == 3;
  const unsigned I = wv::alignbit(dn ? w1[3] : w1[2], dn ? w0[3] : w0[2], (xf == 3 && yf == 0) ? 24u : 16u);
  unsigned out = 0;
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int i = (int)((I >> (8 * p)) & 255u);
    const int a = pick4(ca, i, H[p], V[p], J[p]), b = pick4(cb, i, H[p], V[p], J[p]);
    out |= (unsigned)((a + b + 1) >> 1) << (8 * p);
  }
  return out;
}

// 8.4.2.2.2: the lane's two chroma prediction samples (bits 15:0). A: LDS address of the dword that holds the lane's first
// reference byte on its row; the row below is `pitch` on.
WV unsigned chroma_pred(int A, int pitch, int sh, int xf, int yf) {
  const unsigned s8 = 8u * (unsigned)sh;
  const unsigned v0 = wv::alignbit(wv::lds_u32(A + 4), wv::lds_u32(A), s8);
  const unsigned v1 = wv::alignbit(wv::lds_u32(A + pitch + 4), wv::lds_u32(A + pitch), s8);
  const unsigned wgt = (unsigned)((8 - xf) * (8 - yf)) | (unsigned)(xf * (8 - yf)) << 8 | (unsigned)((8 - xf) * yf) << 16 | (unsigned)(xf * yf) << 24;
  const unsigned p0 = wv::dot4(wv::perm(v1, v0, 0x05040100u), wgt, 32u) >> 6;
  const unsigned p1 = wv::dot4(wv::perm(v1, v0, 0x06050201u), wgt, 32u) >> 6;
  return p0 | p1 << 8;
}

// The lane's luma and chroma prediction samples from the windows stage<LS> left at lwinA / cwinA (vectors at mvA).
template <int LS>
WV void predict(int mvA, int lwinA, int cwinA, int lane, int mbx, int mby, unsigned* lumaOut, unsigned* chromaOut) {
  using G = Geo<LS>;
  {
    const int b = lane >> 2, r = lane & 3;
    const unsigned mv = wv::lds_u32(mvA + 4 * b);
    const int mvx = (int)(short)(mv & 0xffffu), mvy = (int)mv >> 16;
    const int ox = blk_x(b) & G::MASK, oy = blk_y(b) & G::MASK;
    const int x0 = mbx * 16 + blk_x(b) - ox + (mvx >> 2) - 2;
    const int o = (x0 & 3) + ox;
    const int A = lwinA + (((b >> LS) * G::ROWS) + oy + r) * (G::ND * 4) + (o & ~3);
    *lumaOut = luma_pred(A, G::ND * 4, o & 3, mvx & 3, mvy & 3);
  }
  {
    const int pl = lane >> 5, b = (lane & 31) >> 1, r = lane & 1;
    const unsigned mv = wv::lds_u32(mvA + 4 * b);
    const int mvx = (int)(short)(mv & 0xffffu), mvy = (int)mv >> 16;
    const int cx = blk_x(b) >> 1, cy = blk_y(b) >> 1;
    const int ox = cx & (G::MASK >> 1), oy = cy & (G::MASK >> 1);
    const int x0 = mbx * 8 + cx - ox + (mvx >> 3);
    const int o = (x0 & 3) + ox;
    const int A = cwinA + (((pl * (16 >> LS) + (b >> LS)) * G::CROWS) + oy + r) * (G::CND * 4) + (o & ~3);
    *chromaOut = chroma_pred(A, G::CND * 4, o & 3, mvx & 7, mvy & 7);
  }
}

// 8.5.12.1: one scaled coefficient; qd = qp / 6, lim = 4 (4x4) or 6 (8x8)
WV int dequant(int c, int ls, int qd, int lim) {
  const int p = c * ls;
  return qd >= lim ? p << (qd - lim) : (p + (1 << (lim - 1 - qd))) >> (lim - qd);
}

WV void bf4(int d0, int d1, int d2, int d3, int* o) {
  const int e0 = d0 + d2, e1 = d0 - d2, e2 = (d1 >> 1) - d3, e3 = d1 + (d3 >> 1);
  o[0] = e0 + e3;
  o[1] = e1 + e2;
  o[2] = e1 - e2;
  o[3] = e0 - e3;
}

// 8.5.12: row `row` (the lane's, lane & 3) of a 4x4 block's residual. coefA: LDS address where list entry 0 stands (or
// would stand: chroma AC lists start at entry 1); lsA: LDS address of the block's LevelScale list; dc: entry 0 is dcVal,
// already scaled. The four lanes of a quad hold the four rows; all four must be here.
WV void resid4x4_row(int coefA, int lsA, int qd, int row, bool dc, int dcVal, int* r) {
  const unsigned zz = (0xFEA9DB83C7426510ull >> (16 * row)) & 0xffffu;   // list index of (row, 0..3), a nibble each
  int d[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int k = (int)((zz >> (4 * j)) & 15u);
    d[j] = dequant(wv::lds_i16(coefA + 2 * k), (int)wv::lds_u16(lsA + 2 * k), qd, 4);
  }
  if (dc && row == 0) d[0] = dcVal;
  int f[4];
  bf4(d[0], d[1], d[2], d[3], f);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    int g[4];
    bf4(wv::dppx<DPP_QUAD(0, 0, 0, 0)>(f[j]), wv::dppx<DPP_QUAD(1, 1, 1, 1)>(f[j]), wv::dppx<DPP_QUAD(2, 2, 2, 2)>(f[j]),
        wv::dppx<DPP_QUAD(3, 3, 3, 3)>(f[j]), g);
    r[j] = (pick4(row, g[0], g[1], g[2], g[3]) + 32) >> 6;
  }
}

WV void bf8(const int* d, int* o) {
  const int e0 = d[0] + d[4], e1 = -d[3] + d[5] - d[7] - (d[7] >> 1), e2 = d[0] - d[4], e3 = d[1] + d[7] - d[3] - (d[3] >> 1);
  const int e4 = (d[2] >> 1) - d[6], e5 = -d[1] + d[7] + d[5] + (d[5] >> 1), e6 = d[2] + (d[6] >> 1), e7 = d[3] + d[5] + d[1] + (d[1] >> 1);
  const int f0 = e0 + e6, f1 = e1 + (e7 >> 2), f2 = e2 + e4, f3 = e3 + (e5 >> 2), f4 = e2 - e4, f5 = (e3 >> 2) - e5, f6 = e0 - e6, f7 = e7 - (e1 >> 2);
  o[0] = f0 + f7;
  o[1] = f2 + f5;
  o[2] = f4 + f3;
  o[3] = f6 + f1;
  o[4] = f6 - f1;
  o[5] = f4 - f3;
  o[6] = f2 - f5;
  o[7] = f0 - f7;
}

// 8.5.13 for the macroblock's four 8x8 blocks: lanes 0..31, eight per block, take a row each, then a column each, through
// LDS; the residual lands at res8A as i16 [4][8][8]; tmp8A: i32 [4][64] of scratch. (Behind the prediction: both lie over the
// luma windows.)
WV void resid8x8(int coefA, int tmp8A, int res8A, int T, int lane, int qp) {
  const int qd = qp / 6, m = qp - 6 * qd;
  const int q = (lane >> 3) & 3, i = lane & 7;
  if (lane < 32) {
    int d[8], g[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int k = (int)wv::lds_u8(T + T_ZZ8I + i * 8 + j);
      d[j] = dequant(wv::lds_i16(coefA + 2 * (q * 64 + k)), (int)wv::lds_u16(T + T_LS8 + 2 * (m * 64 + k)), qd, 6);
    }
    bf8(d, g);
#pragma unroll
    for (int j = 0; j < 8; j++) wv::lds_st32(tmp8A + 4 * (q * 64 + i * 8 + j), (unsigned)g[j]);
  }
  wv::wave_sync();
  if (lane < 32) {
    int d[8], g[8];
#pragma unroll
    for (int y = 0; y < 8; y++) d[y] = (int)wv::lds_u32(tmp8A + 4 * (q * 64 + y * 8 + i));
    bf8(d, g);
#pragma unroll
    for (int y = 0; y < 8; y++) wv::lds_st16(res8A + 2 * (q * 64 + y * 8 + i), (unsigned)((g[y] + 32) >> 6));
  }
  wv::wave_sync();
}

WV unsigned add_clip4(unsigned pred, const int* r) {
  unsigned out = 0;
#pragma unroll
  for (int p = 0; p < 4; p++) out |= (unsigned)clip255((int)((pred >> (8 * p)) & 255u) + r[p]) << (8 * p);
  return out;
}

// Where a macroblock's rows go: its picture, the row pitch of the luma plane, the chroma planes' offset and distance.
struct OutGeo {
  uint8_t* out;
  unsigned yStride, cOff, cStep;
  int mbx, mby;
};

// A record outside the supported domain: the macroblock zero-filled, the status bit set.
WV void zero_fill(const OutGeo& G, int lane, unsigned* status) {
  if (lane < 16) wv::st_g128(G.out + (16u * (unsigned)G.mby + (unsigned)lane) * G.yStride + 16u * (unsigned)G.mbx, (u32x4){0u, 0u, 0u, 0u});
  else if (lane < 32) {
    const unsigned pl = (unsigned)(lane - 16) >> 3, row = (unsigned)lane & 7u;
    wv::st_g64(G.out + G.cOff + pl * G.cStep + (8u * (unsigned)G.mby + row) * (G.yStride >> 1) + 8u * (unsigned)G.mbx, (u32x2){0u, 0u});
  }
  if (lane == 0) wv::atomic_or(status, 1u);
}

// The residual of the macroblock whose coefficients the lanes 0..47 hold in cq, added to the lanes' prediction samples and
// clipped. coefA: i16 [384]; scrA: 1536 bytes of scratch for the 8x8 transform (the dead luma windows); rescA: i16 [2][64].
WV void add_residual(int coefA, int scrA, int rescA, int T, int lane, int qp, unsigned flags, u32x4 cq, unsigned* predY, unsigned* predC) {
  if (lane < 48) wv::lds_st128(coefA + 16 * lane, cq);
  wv::wave_sync();
  int r[4];
  const int b = lane >> 2, row = lane & 3;
  if (flags & 1u) {
    resid8x8(coefA, scrA, scrA + 1024, T, lane, qp);
    const u32x2 v = wv::lds_u64(scrA + 1024 + 2 * ((b >> 2) * 64 + (((b >> 1) & 1) * 4 + row) * 8 + (b & 1) * 4));
    r[0] = lo16(v[0]);
    r[1] = hi16(v[0]);
    r[2] = lo16(v[1]);
    r[3] = hi16(v[1]);
  } else {
    const int qd = qp / 6, m = qp - 6 * qd;
    resid4x4_row(coefA + 32 * b, T + T_LS4 + 32 * m, qd, row, false, 0, r);
  }
  *predY = add_clip4(*predY, r);
  // chroma (8.5.11): plane (l >> 4) & 1, block (l >> 2) & 3, row l & 3 (lanes 32..63 repeat 0..31: the quads stay whole);
  // the residual goes through LDS to the lanes that own the pixels
  {
    const int cl = lane & 31, pl = cl >> 4, blk = (cl >> 2) & 3;
    const int qpc = (int)wv::lds_u8(T + T_QPC + pl * 52 + qp), qd = qpc / 6, m = qpc - 6 * qd;
    const int base = coefA + 2 * (256 + 64 * pl), lsA = T + T_LS4 + 32 * ((1 + pl) * 6 + m);
    const int c0 = wv::lds_i16(base), c1 = wv::lds_i16(base + 2), c2 = wv::lds_i16(base + 4), c3 = wv::lds_i16(base + 6);
    const int fdc = blk == 0 ? c0 + c1 + c2 + c3 : blk == 1 ? c0 - c1 + c2 - c3 : blk == 2 ? c0 + c1 - c2 - c3 : c0 - c1 - c2 + c3;
    const int dcv = ((fdc * (int)wv::lds_u16(lsA)) << qd) >> 5;
    int rc[4];
    resid4x4_row(base + 8 + 30 * blk - 2, lsA, qd, row, true, dcv, rc);
    const int at = rescA + 2 * (pl * 64 + ((blk >> 1) * 4 + row) * 8 + (blk & 1) * 4);
    if (lane < 32)
      wv::lds_st64(at, (u32x2){((unsigned)rc[0] & 0xffffu) | (unsigned)rc[1] << 16, ((unsigned)rc[2] & 0xffffu) | (unsigned)rc[3] << 16});
  }
  wv::wave_sync();
  {
    const int pl = lane >> 5, bb = (lane & 31) >> 1, rr = lane & 1;
    const int cx = blk_x(bb) >> 1, cy = (blk_y(bb) >> 1) + rr;
    const unsigned v = wv::lds_u32(rescA + 2 * (pl * 64 + cy * 8 + cx));
    const unsigned c = *predC;
    *predC = (unsigned)clip255((int)(c & 255u) + lo16(v)) | (unsigned)clip255((int)((c >> 8) & 255u) + hi16(v)) << 8;
  }
}

// The lanes' reconstructed samples through LDS (outA: u8 [256] Y, [64] Cb, [64] Cr) to whole rows of the picture.
WV void write_out(const OutGeo& G, int outA, int lane, unsigned predY, unsigned predC) {
  {
    const int b = lane >> 2, row = lane & 3;
    wv::lds_st32(outA + (blk_y(b) + row) * 16 + blk_x(b), predY);
    const int pl = lane >> 5, bb = (lane & 31) >> 1, rr = lane & 1;
    wv::lds_st16(outA + 256 + pl * 64 + ((blk_y(bb) >> 1) + rr) * 8 + (blk_x(bb) >> 1), predC);
  }
  wv::wave_sync();
  if (lane < 16) wv::st_g128(G.out + (16u * (unsigned)G.mby + (unsigned)lane) * G.yStride + 16u * (unsigned)G.mbx, wv::lds_u128(outA + 16 * lane));
  else if (lane < 32) {
    const unsigned pl = (unsigned)(lane - 16) >> 3, row = (unsigned)lane & 7u;
    wv::st_g64(G.out + G.cOff + pl * G.cStep + (8u * (unsigned)G.mby + row) * (G.yStride >> 1) + 8u * (unsigned)G.mbx,
               wv::lds_u64(outA + 256 + 8 * (lane - 16)));
  }
}

// One macroblock: index a of the batch.
WV void inter_mb(const IParams& P, const Args& A, int T, int S, int lane, int a) {
  const int per = P.W * P.H;
  const int f = a / per, within = a - f * per, mby = within / P.W, mbx = within - mby * P.W;
  const unsigned cOff = 256u * (unsigned)per, cStep = 64u * (unsigned)per;
  const OutGeo G = {A.yuv + (size_t)f * (size_t)per * 384u, 16u * (unsigned)P.W, cOff, cStep, mbx, mby};

  if (lane < 20) wv::lds_st32(S + S_REC + 4 * lane, ((const unsigned*)(A.mbs + a))[lane]);
  wv::wave_sync();
  const unsigned head = (unsigned)wv::rfl((int)wv::lds_u32(S + S_REC));
  const int qp = (int)((head >> 8) & 255u);
  const unsigned flags = (head >> 16) & 255u;
  const int myRef = (int)(signed char)wv::lds_u8(S + S_REC + 4 + (lane & 3));
  const bool bad = (head & 255u) != 0u || qp > 51 || wv::any(myRef < 0 || myRef >= P.n_refs);
  if (bad) {   // outside the supported domain: zero-filled, reported; the reference table is not read
    zero_fill(G, lane, A.status);
    return;
  }
  if (lane < 4) {
    const unsigned long long rp = (unsigned long long)A.refs[(size_t)f * (size_t)P.n_refs + (size_t)myRef];
    wv::lds_st64(S + S_REFP + 8 * lane, (u32x2){(unsigned)rp, (unsigned)(rp >> 32)});
  }
  const bool hasRes = !(flags & 2u);
  u32x4 cq = {0u, 0u, 0u, 0u};
  if (hasRes && lane < 48) cq = ((const u32x4*)(A.coeffs + (size_t)a * 384u))[lane];
  // the level of the windows: wave-uniform
  const int mvA = S + S_REC + 16, refpA = S + S_REFP, lwinA = S + S_LWIN, cwinA = S + S_CWIN;
  const unsigned myMv = wv::lds_u32(mvA + 4 * (lane & 15));
  const bool same16 = !wv::any(myMv != wv::lds_u32(mvA) || myRef != (int)(signed char)wv::lds_u8(S + S_REC + 4));
  const bool same4 = !wv::any(myMv != wv::lds_u32(mvA + 4 * (lane & 12)));
  wv::wave_sync();   // the reference pointers
  unsigned predY, predC;
  const int wl = 16 * P.W, hl = 16 * P.H;
  if (same16) {
    stage<4, false>(mvA, refpA, lwinA, lane, mbx, mby, wl, hl, 0u, 0u);
    stage<4, true>(mvA, refpA, cwinA, lane, mbx, mby, wl >> 1, hl >> 1, cOff, cStep);
    wv::wave_sync();
    predict<4>(mvA, lwinA, cwinA, lane, mbx, mby, &predY, &predC);
  } else if (same4) {
    stage<2, false>(mvA, refpA, lwinA, lane, mbx, mby, wl, hl, 0u, 0u);
    stage<2, true>(mvA, refpA, cwinA, lane, mbx, mby, wl >> 1, hl >> 1, cOff, cStep);
    wv::wave_sync();
    predict<2>(mvA, lwinA, cwinA, lane, mbx, mby, &predY, &predC);
  } else {
    stage<0, false>(mvA, refpA, lwinA, lane, mbx, mby, wl, hl, 0u, 0u);
    stage<0, true>(mvA, refpA, cwinA, lane, mbx, mby, wl >> 1, hl >> 1, cOff, cStep);
    wv::wave_sync();
    predict<0>(mvA, lwinA, cwinA, lane, mbx, mby, &predY, &predC);
  }
  wv::wave_sync();   // the windows are read: their LDS is the 8x8 transform's scratch from here on

  if (wv::any((cq[0] | cq[1] | cq[2] | cq[3]) != 0u))   // (never under flag bit1: cq is 0 then)
    add_residual(S + S_COEF, S + S_LWIN, S + S_RESC, T, lane, qp, flags, cq, &predY, &predC);
  write_out(G, S + S_OUT, lane, predY, predC);
}

// The wave's loop: macroblocks first, first + stride, ...
WV void inter_wave(const IParams& P, const Args& A, int T, int S, int first, int stride) {
  const int lane = wv::lane_id();
  for (long long a = first; a < (long long)P.n_mbs; a += stride) {
    inter_mb(P, A, T, S, lane, (int)a);
    wv::wave_sync();   // the slice is the next macroblock's
  }
}

}  // namespace inter
}  // namespace dryv
