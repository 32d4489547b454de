"""The inter stage's restatement of ITU-T H.264 on plain Python ints — TEST INFRASTRUCTURE ONLY (dryv has no inter prediction:
nothing here is parity with the reference).

* 8.4.2.2 (fractional sample interpolation) and the inter residual path: luma_sample, chroma_sample, predict_p. The residual
  arithmetic is spec_model's (level_scale4/8, residual4x4/8x8, qp_chroma).
* 8.4.2.3 (weighted sample prediction) on top of predict_p: resolve, predict_b.
* 8.7.2.1's bS rule for frame macroblocks and 8.7 with bS per edge segment: block, strength, bs_reference, filter_line,
  deblock_reference, words. Tables 8-16 and 8-17's bS-3 column are deblock_model's; the bS 1 and 2 columns are here.
"""
import numpy as np

from dryv_amd import abi

from . import deblock_model as dm
from . import spec_model as sm

TAP = lambda v: v[0] - 5 * v[1] + 20 * v[2] + 20 * v[3] - 5 * v[4] + v[5]
CLIP = lambda v: min(max(v, 0), 255)


# ---- 8.4.2.2 + the inter residual path: P macroblocks ---------------------------------------------------------------------------
def luma_sample(P, x, y, xf, yf):
    """8.4.2.2.1 at integer position (x, y), fraction (xf, yf); samples outside the plane are the nearest inside."""
    g = lambda dx, dy: int(P[min(max(y + dy, 0), P.shape[0] - 1), min(max(x + dx, 0), P.shape[1] - 1)])
    b1 = lambda dx, dy: TAP([g(dx + k, dy) for k in range(-2, 4)])
    h1 = lambda dx, dy: TAP([g(dx, dy + k) for k in range(-2, 4)])
    half = lambda v: CLIP((v + 16) >> 5)
    avg = lambda p, q: (p() + q() + 1) >> 1
    G, H, M = (lambda: g(0, 0)), (lambda: g(1, 0)), (lambda: g(0, 1))
    b, h, s, m = (lambda: half(b1(0, 0))), (lambda: half(h1(0, 0))), (lambda: half(b1(0, 1))), (lambda: half(h1(1, 0)))
    j = lambda: CLIP((TAP([b1(0, k) for k in range(-2, 4)]) + 512) >> 10)
    pos = {(0, 0): (G, G), (0, 1): (G, h), (0, 2): (h, h), (0, 3): (M, h), (1, 0): (G, b), (1, 1): (b, h), (1, 2): (h, j), (1, 3): (h, s),
           (2, 0): (b, b), (2, 1): (b, j), (2, 2): (j, j), (2, 3): (j, s), (3, 0): (H, b), (3, 1): (b, m), (3, 2): (j, m), (3, 3): (m, s)}
    return avg(*pos[xf, yf])   # table 8-12


def chroma_sample(P, x, y, xf, yf):
    g = lambda dx, dy: int(P[min(max(y + dy, 0), P.shape[0] - 1), min(max(x + dx, 0), P.shape[1] - 1)])
    return ((8 - xf) * (8 - yf) * g(0, 0) + xf * (8 - yf) * g(1, 0) + (8 - xf) * yf * g(0, 1) + xf * yf * g(1, 1) + 32) >> 6


def _bounded(r, d_sum, gain):
    """The 16-bit bound of 8.5.12 / 8.5.13 on every intermediate: no intermediate exceeds gain * sum |d| (+ rounding)."""
    assert gain * d_sum + 64 < 32768, d_sum
    return r


def _scaled_sum(coefs, ls_flat, qp, lim):
    qd = qp // 6
    return sum(abs(c * l * (1 << (qd - lim)) if qd >= lim else (c * l + (1 << (lim - 1 - qd))) >> (lim - qd)) for c, l in zip(coefs, ls_flat))


def predict_p(fp, frames, refs, mbs, co):
    """(status, yuv): refs[f][i] a picture (uint8, this library's layout). Follows the header's contract for unsupported records."""
    W, H = fp.pic_width_in_mbs, fp.pic_height_in_mbs
    nl, nc = 256 * W * H, 64 * W * H
    ls4 = [sm.level_scale4(fp.scaling_list4x4[3 + i]) for i in range(3)]
    ls8 = sm.level_scale8(fp.scaling_list8x8[1])
    zz4 = lambda lst: [[lst[sm.ZZ4.index((i, j))] for j in range(4)] for i in range(4)]
    flat4 = lambda ls, qp: [int(ls[qp % 6][i][j]) for (i, j) in sm.ZZ4]
    out, status = np.zeros(frames * 384 * W * H, dtype=np.uint8), 0
    for a in range(frames * W * H):
        f, mby, mbx = a // (W * H), (a % (W * H)) // W, a % W
        mb, c = mbs[a], [int(v) for v in co[a]]
        qp = int(mb["qp"])
        if mb["mb_type"] != 0 or qp > 51 or any(not 0 <= int(r) < len(refs[f]) for r in mb["ref_idx"]):
            status = abi.DRYV_E_UNSUPPORTED
            continue
        o = out[f * 384 * W * H:(f + 1) * 384 * W * H]
        planes = [o[:nl].reshape(16 * H, 16 * W), o[nl:nl + nc].reshape(8 * H, 8 * W), o[nl + nc:].reshape(8 * H, 8 * W)]
        res = [np.zeros((16, 16), dtype=np.int64), np.zeros((8, 8), dtype=np.int64), np.zeros((8, 8), dtype=np.int64)]
        if not mb["flags"] & 2:
            for q in range(4) if mb["flags"] & 1 else ():
                lst = c[64 * q:64 * q + 64]
                r = _bounded(sm.residual8x8(lst, ls8, qp), _scaled_sum(lst, [int(ls8[qp % 6][i][j]) for (i, j) in sm.ZZ8], qp, 6), 2.25)
                res[0][8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8] = r
            for b in () if mb["flags"] & 1 else range(16):
                lst, (x, y) = c[16 * b:16 * b + 16], sm.BLK_XY[b]
                res[0][y:y + 4, x:x + 4] = _bounded(sm.residual4x4(zz4(lst), ls4[0], qp, False), _scaled_sum(lst, flat4(ls4[0], qp), qp, 4), 1)
            for pl in range(2):
                qpc = sm.qp_chroma(qp, (fp.chroma_qp_index_offset, fp.second_chroma_qp_index_offset)[pl])
                base, ls = 256 + 64 * pl, ls4[1 + pl]
                d = c[base:base + 4]
                fdc = [d[0] + d[1] + d[2] + d[3], d[0] - d[1] + d[2] - d[3], d[0] + d[1] - d[2] - d[3], d[0] - d[1] - d[2] + d[3]]
                for blk in range(4):
                    dc = ((fdc[blk] * int(ls[qpc % 6, 0, 0])) * (1 << (qpc // 6))) >> 5
                    ac = c[base + 4 + 15 * blk:base + 19 + 15 * blk]
                    r = _bounded(sm.residual4x4(zz4([dc] + ac), ls, qpc, True), abs(dc) + _scaled_sum(ac, flat4(ls, qpc)[1:], qpc, 4), 1)
                    res[1 + pl][4 * (blk >> 1):4 * (blk >> 1) + 4, 4 * (blk & 1):4 * (blk & 1) + 4] = r
        for b in range(16):
            ref = refs[f][int(mb["ref_idx"][b >> 2])]
            rp = [ref[:nl].reshape(16 * H, 16 * W), ref[nl:nl + nc].reshape(8 * H, 8 * W), ref[nl + nc:].reshape(8 * H, 8 * W)]
            (bx, by), (mvx, mvy) = sm.BLK_XY[b], (int(mb["mv"][b][0]), int(mb["mv"][b][1]))
            for y in range(4):
                for x in range(4):
                    p = luma_sample(rp[0], 16 * mbx + bx + x + (mvx >> 2), 16 * mby + by + y + (mvy >> 2), mvx & 3, mvy & 3)
                    planes[0][16 * mby + by + y, 16 * mbx + bx + x] = CLIP(p + int(res[0][by + y, bx + x]))
            for pl in (1, 2):
                for y in range(by // 2, by // 2 + 2):
                    for x in range(bx // 2, bx // 2 + 2):
                        p = chroma_sample(rp[pl], 8 * mbx + x + (mvx >> 3), 8 * mby + y + (mvy >> 3), mvx & 7, mvy & 7)
                        planes[pl][8 * mby + y, 8 * mbx + x] = CLIP(p + int(res[pl][y, x]))
    return status, out


# ---- 8.4.2.3: B macroblocks and weighted prediction -----------------------------------------------------------------------------
def resolve(wt, pl, r0, r1):
    """8.4.2.3: (w0, w1, rnd, sh, off) of a quadrant with reference indices r0 / r1 (< 0: unused) in plane pl."""
    both, mode = r0 >= 0 and r1 >= 0, 0 if wt is None else int(wt["mode"])
    if mode == 1:
        d = int(wt["luma_log2_denom"] if pl == 0 else wt["chroma_log2_denom"])
        w, o = [int(wt["expl"]["w"][X, max(r, 0), pl]) for X, r in ((0, r0), (1, r1))], [int(wt["expl"]["o"][X, max(r, 0), pl]) for X, r in ((0, r0), (1, r1))]
        if both:
            return w[0], w[1], 1 << d, d + 1, (o[0] + o[1] + 1) >> 1
        X = 0 if r0 >= 0 else 1
        return w[0] * (X == 0), w[1] * (X == 1), (1 << (d - 1)) if d >= 1 else 0, d, o[X]
    if mode == 2 and both:
        w1 = int(wt["implicit_w1"][r0, r1])
        return 64 - w1, w1, 32, 6, 0
    return (1, 1, 1, 1, 0) if both else (int(r0 >= 0), int(r1 >= 0), 0, 0, 0)


def predict_b(fp, frames, refs0, refs1, wts, mbs, co):
    """(status, yuv). Each list's prediction is predict_p over P records without residual; the weighted combination is Python
    ints; the residual is added by predict_p predicting, with zero vectors, from the combined picture."""
    W, H = fp.pic_width_in_mbs, fp.pic_height_in_mbs
    n, per, n1 = len(mbs), W * H, len(refs1[0])
    r = mbs["ref_idx"].astype(int)
    bad = (mbs["mb_type"] != 0) | (mbs["qp"] > 51) | ((r[:, 0] >= len(refs0[0])) | (r[:, 1] >= n1) | ((r[:, 0] < 0) & (r[:, 1] < 0))).any(axis=1)
    pred = []
    for X, refs in ((0, refs0), (1, refs1)):
        p = np.zeros(n, dtype=abi.INTER_MB_DTYPE)
        p["flags"], p["mv"] = 2, mbs["mv"][:, X]
        p["ref_idx"] = np.where(bad[:, None] | (r[:, X] < 0), 0, r[:, X])
        p["mv"][bad | (r[:, X] < 0).all(axis=1)] = 0
        pred.append(predict_p(fp, frames, refs if n1 or X == 0 else refs0, p, co)[1].astype(np.int64))
    comb = np.zeros(frames * per * 384, dtype=np.uint8)
    for a in np.flatnonzero(~bad):
        f, mby, mbx = a // per, (a % per) // W, a % W
        for pl in range(3):
            s, off = (16, 0) if pl == 0 else (8, 256 * per + (pl - 1) * 64 * per)
            view = lambda v: v[f * 384 * per + off:f * 384 * per + off + s * s * per].reshape(s * H, s * W)
            for q in range(4):
                w0, w1, rnd, sh, o = resolve(None if wts is None else wts[f], pl, r[a, 0, q], r[a, 1, q])
                ys, xs = slice(s * mby + (q >> 1) * s // 2, s * mby + (q >> 1) * s // 2 + s // 2), slice(s * mbx + (q & 1) * s // 2, s * mbx + (q & 1) * s // 2 + s // 2)
                view(comb)[ys, xs] = np.clip(((view(pred[0])[ys, xs] * w0 + view(pred[1])[ys, xs] * w1 + rnd) >> sh) + o, 0, 255)
    p = np.zeros(n, dtype=abi.INTER_MB_DTYPE)
    p["flags"], p["qp"], p["mb_type"] = mbs["flags"], np.where(bad, 0, mbs["qp"]), bad
    st, out = predict_p(fp, frames, [[comb[f * 384 * per:(f + 1) * 384 * per]] for f in range(frames)], p, co)
    return st, out


# ---- 8.7: boundary strengths of P and B pictures, the filter with bS per edge segment --------------------------------------------
TC0 = {1: [0] * 23 + [1] * 10 + [2] * 4 + [3] * 3 + [4] * 3 + [5, 6, 6, 7, 8, 9, 10, 11, 13],
       2: [0] * 21 + [1] * 10 + [2] * 4 + [3] * 3 + [4, 4, 5, 5, 6, 7, 8, 8, 10, 11, 12, 13, 15, 17], 3: dm.TC0_BS3}
BIDX = {xy: b for b, xy in enumerate(sm.BLK_XY)}   # (x, y) in samples -> 4x4 block index (figure 6-10)
CLIP3 = lambda lo, hi, v: min(max(v, lo), hi)


def block(mbs, co, keys, a, per, bx, by):
    """What 8.7.2.1 asks of the 4x4 block (bx, by) of macroblock a: "intra", or (non-zero coefficients, [(picture, vector)])."""
    mb, b = mbs[a], BIDX[4 * bx, 4 * by]
    if mb["mb_type"] != 0:
        return "intra"
    c = co[a, 64 * (b >> 2):64 * (b >> 2) + 64] if mb["flags"] & 1 else co[a, 16 * b:16 * b + 16]
    r, mv = mb["ref_idx"].reshape(-1, 4)[:, b >> 2], mb["mv"].reshape(-1, 16, 2)[:, b]
    return (not mb["flags"] & 2 and bool(np.any(c)),
            [(keys[X][a // per][int(r[X])], (int(mv[X][0]), int(mv[X][1]))) for X in range(len(r)) if r[X] >= 0])


def strength(p, q, mb_edge):
    if "intra" in (p, q):
        return 4 if mb_edge else 3
    if p[0] or q[0]:
        return 2
    P, Q = p[1], q[1]
    if sorted(k for k, _ in P) != sorted(k for k, _ in Q):
        return 1
    near = lambda u, v: abs(u[0] - v[0]) < 4 and abs(u[1] - v[1]) < 4
    if len(P) == 1 or P[0][0] != P[1][0]:   # every vector against the other block's vector on the same picture
        return int(not all(near(v, dict(Q)[k]) for k, v in P))
    return int(not (near(P[0][1], Q[0][1]) and near(P[1][1], Q[1][1]) or near(P[0][1], Q[1][1]) and near(P[1][1], Q[0][1])))


def bs_reference(W, H, mbs, co, keys):
    """bS[a, dir, edge, segment]; keys[list][frame][refIdx]: an identity per reference PICTURE."""
    per, bs = W * H, np.zeros((len(mbs), 2, 4, 4), dtype=np.int64)
    for a in range(len(mbs)):
        x, y, t8 = a % W, (a % per) // W, mbs[a]["flags"] & 1
        cur = lambda bx, by: block(mbs, co, keys, a, per, bx, by)
        for bx in range(4):
            for by in range(4):
                if not (bx == 0 and x == 0) and not (t8 and bx & 1):
                    bs[a, 0, bx, by] = strength(cur(bx - 1, by) if bx else block(mbs, co, keys, a - 1, per, 3, by), cur(bx, by), bx == 0)
                if not (by == 0 and y == 0) and not (t8 and by & 1):
                    bs[a, 1, by, bx] = strength(cur(bx, by - 1) if by else block(mbs, co, keys, a - W, per, bx, 3), cur(bx, by), by == 0)
    return bs


def filter_line(s, i, bS, qp_p, qp_q, chroma, offA, offB):
    """8.7.2.2 - 8.7.2.4 on one line of samples: p_k = s[i - 1 - k], q_k = s[i + k]."""
    ia, ib = CLIP3(0, 51, ((qp_p + qp_q + 1) >> 1) + offA), CLIP3(0, 51, ((qp_p + qp_q + 1) >> 1) + offB)
    alpha, beta, n = dm.ALPHA[ia], dm.BETA[ib], 2 if chroma else 4
    p, q = [int(s[i - 1 - k]) for k in range(n)], [int(s[i + k]) for k in range(n)]
    if not (abs(p[0] - q[0]) < alpha and abs(p[1] - p[0]) < beta and abs(q[1] - q[0]) < beta):
        return
    ap, aq = (not chroma and abs(p[2] - p[0]) < beta), (not chroma and abs(q[2] - q[0]) < beta)
    if bS < 4:
        tc0 = TC0[bS][ia]
        tc = tc0 + 1 if chroma else tc0 + ap + aq
        d = CLIP3(-tc, tc, (((q[0] - p[0]) << 2) + (p[1] - q[1]) + 4) >> 3)
        s[i - 1], s[i] = CLIP3(0, 255, p[0] + d), CLIP3(0, 255, q[0] - d)
        if ap:
            s[i - 2] = p[1] + CLIP3(-tc0, tc0, (p[2] + ((p[0] + q[0] + 1) >> 1) - (p[1] << 1)) >> 1)
        if aq:
            s[i + 1] = q[1] + CLIP3(-tc0, tc0, (q[2] + ((p[0] + q[0] + 1) >> 1) - (q[1] << 1)) >> 1)
        return
    small, s[i - 1], s[i] = abs(p[0] - q[0]) < (alpha >> 2) + 2, (2 * p[1] + p[0] + q[1] + 2) >> 2, (2 * q[1] + q[0] + p[1] + 2) >> 2
    if ap and small:
        s[i - 1], s[i - 2], s[i - 3] = (p[2] + 2 * p[1] + 2 * p[0] + 2 * q[0] + q[1] + 4) >> 3, (p[2] + p[1] + p[0] + q[0] + 2) >> 2, (2 * p[3] + 3 * p[2] + p[1] + p[0] + q[0] + 4) >> 3
    if aq and small:
        s[i], s[i + 1], s[i + 2] = (p[1] + 2 * p[0] + 2 * q[0] + 2 * q[1] + q[2] + 4) >> 3, (p[0] + q[0] + q[1] + q[2] + 2) >> 2, (2 * q[3] + 3 * q[2] + q[1] + q[0] + p[0] + 4) >> 3


def deblock_reference(fp, dp, frames, mbs, yuv, bs):
    """8.7, macroblocks in raster order: per plane vertical edges left to right, then horizontal. Chroma line k: luma segment k >> 1; chroma edge 4: luma edge 8."""
    W, H = fp.pic_width_in_mbs, fp.pic_height_in_mbs
    per, out = W * H, yuv.astype(np.int64)
    offA, offB = 2 * dp.slice_alpha_c0_offset_div2, 2 * dp.slice_beta_offset_div2
    for a in range(frames * per if dp.disable_deblocking_filter_idc != 1 else 0):
        o, mx, my = out[a // per * 384 * per:(a // per + 1) * 384 * per], a % W, (a % per) // W
        for pl, P in enumerate((o[:256 * per].reshape(16 * H, 16 * W), o[256 * per:320 * per].reshape(8 * H, 8 * W), o[320 * per:].reshape(8 * H, 8 * W))):
            n = 8 if pl else 16
            qp = lambda k: dm.qpc(int(mbs[k]["qp"]), (fp.chroma_qp_index_offset, fp.second_chroma_qp_index_offset)[pl - 1]) if pl else int(mbs[k]["qp"])
            for d, e, k in ((d, e, k) for d in (0, 1) for e in ((0, 2) if pl else range(4)) for k in range(n)):
                b, line = int(bs[a, d, e, k * 4 // n]), P[n * my + k] if d == 0 else P[:, n * mx + k]
                if b:
                    filter_line(line, n * (my if d else mx) + e * n // 4, b, qp(a if e else a - (W if d else 1)), qp(a), pl > 0, offA, offB)
    return out.astype(np.uint8)


words = lambda bs: (bs << (4 * np.arange(4))).sum(axis=-1).astype(np.uint16)   # the records' 16-bit words
