// deblock_bs_kernel.h — boundary strengths (ITU-T H.264 8.7.2.1, frame macroblocks) of the inter stage's P and B pictures for
// gfx950, as wave-level code (wave.h): one dryv_bs_rec per macroblock, which the bS-record variant of deblock_kernel.h filters by.
//
// No macroblock depends on another one's result, so the grid is flat: a wave takes four raster-consecutive macroblocks of the
// batch, lane = (macroblock l >> 4, 4x4 block l & 15 in figure 6-10 order: the order of the vectors and of the coefficient lists).
//   * Every lane reduces its block to an entry {non-zero flag, intra flag, two picture ids, two vectors} and leaves it in the
//     wave's LDS slice; the block to the left and the block above are read back from there.
//   * Non-zero flag: the OR of the block's 32 bytes of luma coefficients; under transform 8x8 list q of 64 is the bytes of lanes
//     4q .. 4q+3, so the flag is ORed over the quad (DPP quad_perm). A slot under flag bit1 is not read. Chroma never counts.
//   * Picture ids: bS compares pictures, not indices. The host turns each picture's two pointer tables into 32 bytes indexed by
//     (list, refIdx): the first position with the same device pointer; 0xFF: the list is unused.
//   * Halos: the lanes of block row 0 build the entry of the block above them (the bottom block row of the macroblock above), the
//     lanes of block column 0 of the wave's first macroblock that of the block to their left, from those macroblocks' records and
//     coefficients. A halo block of a transform-8x8 macroblock reads its whole list of 64 (128 bytes): the quadrant's flag is
//     not in the block's own 32 bytes alone.
//   * Output: a lane's two strengths are two nibbles of the 128-bit record; the sixteen lanes of a macroblock OR them together
//     over their DPP row (row_ror 8, 4, 2, 1) and lane 0 of the row stores 16 bytes (twice, when the caller wants a copy).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/dryv_recon.h"
#include "wave.h"

namespace dryv {
namespace deblock_bs {

struct Args {
  const uint8_t* recs;     // dryv_inter_mb (BI = false) or dryv_inter_bmb (BI = true) records
  const int16_t* coeffs;
  const uint8_t* ids;      // [n_frames][2][16] picture ids
  u32x4* bs;               // [n_mbs] dryv_bs_rec: the library's workspace
  u32x4* bs_copy;          // NULL, or the caller's copy
  int W, H, n_mbs;
};

constexpr int S_OWN = 0;                // u32x4 [4 macroblocks][16 blocks]
constexpr int S_TOP = 1024;             // u32x4 [4][4]: the bottom block row of the macroblock above each
constexpr int S_LEFT = S_TOP + 256;     // u32x4 [4]: the right block column of the macroblock left of the first
constexpr int S_BYTES = S_LEFT + 64 + 64;
constexpr unsigned E_NZ = 1u, E_INTRA = 2u;   // entry.x: bit0, bit1; byte 1: list 0's picture id; byte 2: list 1's; .y, .z: the vectors

WV int blk_of(int bx, int by) { return (bx & 1) | ((by & 1) << 1) | ((bx & 2) << 1) | ((by & 2) << 2); }
WV unsigned or4(u32x4 v) { return v.x | v.y | v.z | v.w; }

// The entry of block blk of macroblock a (of picture f). quadAlone: the caller cannot OR over the quad, so a transform-8x8
// macroblock's whole list of 64 is read here.
template <bool BI>
WV u32x4 entry_of(const Args& A, size_t a, int f, int blk, bool quadAlone, bool& t8) {
  constexpr int STRIDE = BI ? 144 : 80;
  const uint8_t* rec = A.recs + a * STRIDE;
  const unsigned hdr = *(const unsigned*)rec;
  const unsigned flags = (hdr >> 16) & 0xffu;
  t8 = (flags & 1u) != 0;
  const int r0 = ((const int8_t*)rec)[4 + (blk >> 2)], r1 = BI ? ((const int8_t*)rec)[8 + (blk >> 2)] : -1;
  const uint8_t* tab = A.ids + (size_t)f * 32;
  const unsigned id0 = r0 < 0 ? 0xffu : tab[r0 & 15], id1 = r1 < 0 ? 0xffu : tab[16 + (r1 & 15)];
  u32x4 e = {0, 0, 0, 0};
  e.y = *(const unsigned*)(rec + 16 + 4 * blk);
  if (BI) e.z = *(const unsigned*)(rec + 80 + 4 * blk);
  unsigned nz = 0;
  if (!(flags & 2u)) {
    const u32x4* c = (const u32x4*)(A.coeffs + a * DRYV_COEFFS_PER_MB);
    if (t8 && quadAlone) {
#pragma unroll
      for (int k = 0; k < 8; k++) nz |= or4(c[8 * (blk >> 2) + k]);
    } else {
      nz = or4(c[2 * blk]) | or4(c[2 * blk + 1]);
    }
  }
  e.x = (nz ? E_NZ : 0u) | ((hdr & 0xffu) ? E_INTRA : 0u) | (id0 << 8) | (id1 << 16);
  return e;
}

WV bool far(unsigned u, unsigned v) {  // 8.7.2.1: a vector component differs by 4 or more quarter samples
  const int dx = (int)(short)(u & 0xffffu) - (int)(short)(v & 0xffffu), dy = ((int)u >> 16) - ((int)v >> 16);
  return (dx < 0 ? -dx : dx) >= 4 || (dy < 0 ? -dy : dy) >= 4;
}

// bS of the edge between block p (left or above) and block q. mbEdge: a macroblock edge.
WV unsigned strength(const u32x4 p, const u32x4 q, bool mbEdge) {
  if ((p.x | q.x) & E_INTRA) return mbEdge ? 4u : 3u;
  if ((p.x | q.x) & E_NZ) return 2u;
  const unsigned pa = (p.x >> 8) & 0xffu, pb = (p.x >> 16) & 0xffu, qa = (q.x >> 8) & 0xffu, qb = (q.x >> 16) & 0xffu;
  // the same pictures list by list, or crosswise (both when all four are one picture: either pairing may pass)
  const bool straight = pa == qa && pb == qb && !(pa != 0xffu && far(p.y, q.y)) && !(pb != 0xffu && far(p.z, q.z));
  const bool cross = pa == qb && pb == qa && !(pa != 0xffu && far(p.y, q.z)) && !(pb != 0xffu && far(p.z, q.y));
  return (straight || cross) ? 0u : 1u;
}

template <int CTRL>
WV u32x4 or_dpp(u32x4 v) {
  v.x |= (unsigned)wv::dppx<CTRL>((int)v.x);
  v.y |= (unsigned)wv::dppx<CTRL>((int)v.y);
  v.z |= (unsigned)wv::dppx<CTRL>((int)v.z);
  v.w |= (unsigned)wv::dppx<CTRL>((int)v.w);
  return v;
}

// One wave: macroblocks 4 * group .. 4 * group + 3 of the batch. ts: the wave's LDS slice.
template <bool BI>
WV void bs_wave(const Args& A, const int ts, const int group) {
  const int lane = wv::lane_id();
  const int m = lane >> 4, b = lane & 15;
  const int bx = (b & 1) | ((b >> 1) & 2), by = ((b >> 1) & 1) | ((b >> 2) & 2);
  const int per = A.W * A.H;
  const int a = 4 * group + m;
  const bool live = a < A.n_mbs;
  const int f = a / per, x = (a % per) % A.W, y = (a % per) / A.W;

  bool t8 = false, t8n;
  u32x4 own = {0, 0, 0, 0};
  if (live) {
    own = entry_of<BI>(A, (size_t)a, f, b, false, t8);
    // the macroblock above (its block (bx, 3)); the macroblock left of the wave's first one (its block (3, by))
    if (by == 0 && y > 0) wv::lds_st128(ts + S_TOP + 16 * (4 * m + bx), entry_of<BI>(A, (size_t)(a - A.W), f, blk_of(bx, 3), true, t8n));
    if (m == 0 && bx == 0 && x > 0) wv::lds_st128(ts + S_LEFT + 16 * by, entry_of<BI>(A, (size_t)(a - 1), f, blk_of(3, by), true, t8n));
  }
  // transform 8x8: the quadrant's flag (lanes 4q .. 4q+3 are one DPP quad)
  unsigned nzq = own.x & E_NZ;
  nzq |= (unsigned)wv::dppx<DPP_QUAD(1, 0, 3, 2)>((int)nzq);
  nzq |= (unsigned)wv::dppx<DPP_QUAD(2, 3, 0, 1)>((int)nzq);
  if (t8) own.x |= nzq;
  wv::lds_st128(ts + S_OWN + 16 * lane, own);
  wv::wave_sync();

  u32x4 out = {0, 0, 0, 0};
  if (live) {
    // vertical edge: left of this block (x > 0 with bx == 0: macroblock a - 1, in this wave unless m == 0)
    const int la = bx > 0 ? ts + S_OWN + 16 * (16 * m + blk_of(bx - 1, by)) : m > 0 ? ts + S_OWN + 16 * (16 * (m - 1) + blk_of(3, by)) : ts + S_LEFT + 16 * by;
    const int ta = by > 0 ? ts + S_OWN + 16 * (16 * m + blk_of(bx, by - 1)) : ts + S_TOP + 16 * (4 * m + bx);
    unsigned bv = 0, bh = 0;
    if (!(bx == 0 && x == 0) && !(t8 && (bx & 1))) bv = strength(wv::lds_u128(la), own, bx == 0);
    if (!(by == 0 && y == 0) && !(t8 && (by & 1))) bh = strength(wv::lds_u128(ta), own, by == 0);
    // v[0][bx] segment by: bit 16 * bx + 4 * by of the record; v[1][by] segment bx: bit 64 + 16 * by + 4 * bx
    const unsigned sv = bv << (16 * (bx & 1) + 4 * by), sh = bh << (16 * (by & 1) + 4 * bx);
    out.x = bx < 2 ? sv : 0u;
    out.y = bx < 2 ? 0u : sv;
    out.z = by < 2 ? sh : 0u;
    out.w = by < 2 ? 0u : sh;
  }
  out = or_dpp<DPP_ROW_ROR(8)>(out);
  out = or_dpp<DPP_ROW_ROR(4)>(out);
  out = or_dpp<DPP_ROW_ROR(2)>(out);
  out = or_dpp<DPP_ROW_ROR(1)>(out);
  if (live && b == 0) {
    A.bs[a] = out;
    if (A.bs_copy) A.bs_copy[a] = out;
  }
}

}  // namespace deblock_bs
}  // namespace dryv
