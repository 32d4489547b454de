"""In-loop deblocking of the inter stage's P and B pictures (dryv_inter_deblock_device) against a plain-integer restatement of ITU-T H.264 8.7 with bS per
edge segment, and of 8.7.2.1's bS rule for frame macroblocks, bit for bit. Tables 8-16 and 8-17's bS-3 column: oracle.deblock_model's; bS 1 and 2: here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle
import test_inter as ti
import test_inter_bipred as tb
from dryv_amd import abi, synth
from oracle import deblock_model as dm
from oracle import spec_model as sm
from test_inter import inter_ctx  # noqa: F401  (the module's stage fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def run(ctx, fp, dp, frames, pool, keys, mbs, co, yuv=None):
    """Submits the records (unless yuv is given), reads the picture, deblocks it in place: (unfiltered, filtered, bS words)."""
    import torch
    bi = mbs.dtype == abi.INTER_BMB_DTYPE
    d_pool = [torch.from_numpy(p).cuda() for p in pool]
    ptrs = [[[d_pool[k].data_ptr() for k in fr] for fr in keys[X]] for X in (0, 1)]
    d_m, d_c, d_bs = torch.from_numpy(mbs.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(co).cuda(), torch.zeros(len(mbs) * 16, dtype=torch.uint8, device="cuda")
    d_y = torch.full((len(mbs) * 384,), 0xAA, dtype=torch.uint8, device="cuda") if yuv is None else torch.from_numpy(yuv).cuda()
    if yuv is None:
        (ctx.submit_device_bipred(fp, frames, ptrs[0], ptrs[1], None, d_m.data_ptr(), d_c.data_ptr(), d_y.data_ptr()) if bi else
         ctx.submit_device(fp, frames, ptrs[0], d_m.data_ptr(), d_c.data_ptr(), d_y.data_ptr()))
        ctx.sync(allow_unsupported=True)
    before = d_y.cpu().numpy()
    ctx.deblock_device(fp, dp, frames, bi, ptrs[0], ptrs[1], d_m.data_ptr(), d_c.data_ptr(), d_y.data_ptr(), d_bs.data_ptr())
    assert ctx.sync() == 0
    return before, d_y.cpu().numpy(), d_bs.cpu().numpy().view(np.uint16).reshape(-1, 2, 4)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_layout_validation_tables_and_kernel_resources():
    assert C.sizeof(abi.BsRec) == 16 == abi.BS_REC_DTYPE.itemsize
    lib, fp, ok = abi.load_library(), abi.make_frame_params(4, 3), abi.make_deblock_params(0, -6, 6)
    check = lambda dp, bi, n0, n1: lib.dryv_inter_check_deblock(C.byref(fp), C.byref(dp), 2, bi, n0, n1)
    assert [check(ok, 0, 1, 0), check(ok, 1, 16, 16), check(abi.make_deblock_params(1, 0, 0), 1, 1, 0)] == [abi.DRYV_OK] * 3
    assert [check(abi.make_deblock_params(*d), 0, 1, 0) for d in ((3, 0, 0), (0, 7, 0), (0, 0, -7))] + [check(ok, 0, 0, 0), check(ok, 0, 17, 0), check(ok, 0, 1, 1), check(ok, 1, 1, 17)] == [abi.DRYV_E_INVALID] * 7
    fp.bit_depth_y = 10
    assert check(ok, 0, 1, 0) == abi.DRYV_E_UNSUPPORTED
    assert all(len(TC0[b]) == 52 for b in TC0) and all(TC0[1][k] <= TC0[2][k] <= TC0[3][k] for k in range(52))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from resource_usage import resource_usage
    usage = {k: v for src in ("deblock_bs.hip", "inter_deblock.hip") for k, v in resource_usage(os.path.join(ROOT, "dryv_amd", "csrc", src)).items()}
    assert len(usage) == 3 and all(g["VGPRs Spill"] == 0 and g["ScratchSize"] == 0 for g in usage.values()), usage


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _set(m, a, l0=None, l1=None, **kw):   # macroblock a of hand-made B records: list X = (refIdx, vector) on all blocks, or None: unused
    for X, l in ((0, l0), (1, l1)):
        m["ref_idx"][a, X], m["mv"][a, X] = (-1, 0) if l is None else l
    for k, v in kw.items():
        m[k][a] = v


_coef = lambda co, a, pos, v=1: co.__setitem__((a, pos), v)
# 3 x 2 macroblocks, two frames; pictures A = 0, B = 1; list 0 of frame 0: [A, B, A], of frame 1: [B, A, A]; list 1: [A, B] in both.
# Every macroblock starts as (L0 index 0, zero vector, no residual). Probes: (macroblock, dir, edge, segment) -> bS; E: macroblock 1's left edge.
KEYS, E = ([[0, 1, 0], [1, 0, 0]], [[0, 1], [0, 1]]), (1, 0, 0, 0)
BS_CASES = [("d%s" % (v,), lambda m, c, v=v: _set(m, 1, (0, v)), {E: w}) for v, w in (((3, 0), 0), ((4, 0), 1), ((0, 3), 0), ((0, 4), 1), ((-4, 0), 1), ((-3, -3), 0))] + [
    ("same-picture-other-index", lambda m, c: (_set(m, 1, (2, (0, 0))), _set(m, 7, (2, (0, 0)))), {E: 0, (7, 0, 0, 0): 1}),
    ("lists-swapped", lambda m, c: (_set(m, 0, (0, (8, 0)), (1, (-8, 4))), _set(m, 1, (1, (-8, 4)), (0, (8, 0)))), {E: 0}),
    ("one-picture-cross", lambda m, c: (_set(m, 0, (0, (0, 0)), (0, (20, 0))), _set(m, 1, (2, (20, 0)), (0, (0, 0)))), {E: 0}),
    ("one-picture-neither", lambda m, c: (_set(m, 0, (0, (0, 0)), (0, (20, 0))), _set(m, 1, (0, (20, 0)), (0, (8, 0)))), {E: 1}),
    ("one-against-two", lambda m, c: _set(m, 1, (0, (0, 0)), (0, (0, 0))), {E: 1}),
    ("neighbour-coefficient", lambda m, c: (_set(m, 0, (0, (0, 0)), flags=0), _coef(c, 0, 16 * 5 + 3)), {E: 2, (1, 0, 0, 1): 0, (0, 0, 3, 0): 2}),
    ("chroma-only", lambda m, c: (_set(m, 1, (0, (0, 0)), flags=0), _coef(c, 1, slice(256, 384), 7)), {E: 0}),
    # list 2 of 64, an entry in the bytes of block 8: the whole lower-left quadrant, seen from inside and from the macroblock below
    ("t8-one-entry", lambda m, c: (_set(m, 1, (0, (0, 0)), flags=1), _coef(c, 1, 128 + 5)),
     {E: 0, (1, 0, 0, 2): 2, (1, 0, 0, 3): 2, (1, 0, 1, 2): 0, (1, 0, 2, 2): 2, (1, 0, 3, 2): 0, (1, 1, 1, 0): 0, (1, 1, 2, 0): 2,
      (1, 1, 2, 1): 2, (1, 1, 3, 0): 0, (4, 1, 0, 0): 2, (4, 1, 0, 1): 2, (4, 1, 0, 2): 0}),
    ("no-residual-garbage", lambda m, c: (_set(m, 1, (0, (0, 0)), flags=2), _coef(c, 1, slice(0, 384), 0x7FFF)), {E: 0}),
    ("intra-neighbour", lambda m, c: _set(m, 1, (0, (0, 0)), mb_type=1), {E: 4, (1, 0, 1, 0): 3, (1, 1, 3, 2): 3, (2, 0, 0, 3): 4, (4, 1, 0, 0): 4}),
    ("picture-border", lambda m, c: _set(m, 0, (0, (0, 0)), mb_type=1), {(0, 0, 0, 0): 0, (0, 1, 0, 3): 0, (0, 0, 1, 0): 3, (3, 0, 0, 0): 0, (3, 1, 0, 0): 4})]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BS_CASES, ids=lambda c: c[0])
def test_bs_records(inter_ctx, case):  # noqa: F811
    fp, rng, m, co = abi.make_frame_params(3, 2), np.random.default_rng(1), np.zeros(12, dtype=abi.INTER_BMB_DTYPE), np.zeros((12, 384), dtype=np.int16)
    m["qp"], m["flags"], m["ref_idx"][:, 1] = 30, 2, -1
    case[1](m, co)
    pool, yuv = [rng.integers(0, 256, size=384 * 6, dtype=np.uint8) for _ in range(2)], rng.integers(0, 256, size=384 * 12, dtype=np.uint8)
    got = run(inter_ctx, fp, abi.make_deblock_params(), 2, pool, KEYS, m, co, yuv)[2]
    for (a, d, e, k), want in case[2].items():
        assert (got[a, d, e] >> (4 * k)) & 15 == want, ((a, d, e, k), hex(got[a, d, e]))
    assert np.array_equal(got, words(bs_reference(3, 2, m, co, KEYS)))


def _random_case(W, H, frames, bi, seed):
    fp, r0, r1, _, mbs, co = tb.make_case(W, H, frames, 2, 2, "default", "mixed", "mixed", seed) if bi else (
        lambda c: (c[0], c[1], [[]] * frames, None, c[2], c[3]))(ti.make_case(W, H, frames, 2, "mixed", "mixed", (0, 51), 3, seed))
    mbs["mv"] //= 8 if bi else 1   # both kinds within +-3 samples: differences on either side of 4 quarter samples
    mbs["mb_type"][5::7] = 1       # a few intra macroblocks (zero-filled by the stage): bS 4 / 3
    rng, n = np.random.default_rng(seed), sum(len(per) for per in r0 + r1)   # smooth pictures on different levels: steps that pass the thresholds
    pool = [(rng.integers(60, 196) + rng.integers(-6, 7, size=384 * W * H)).astype(np.uint8) for _ in range(n)]
    keys = ([[2 * f, 2 * f + 1] for f in range(frames)], [[2 * frames + 2 * f, 2 * frames + 2 * f + 1] if bi else [] for f in range(frames)])
    return fp, pool, keys, mbs, co


@pytest.mark.gpu
@pytest.mark.parametrize("bi", [False, True], ids=["P", "B"])
@pytest.mark.parametrize("geo", [(1, 1, 1), (5, 1, 1), (1, 5, 2), (5, 5, 2), (9, 6, 2)], ids=lambda g: "%dx%dx%d" % g)
def test_filtered_pictures(inter_ctx, geo, bi):  # noqa: F811
    (W, H, frames), dp = geo, abi.make_deblock_params(0, 2, -3)
    fp, pool, keys, mbs, co = _random_case(W, H, frames, bi, seed=13 * W + H)
    before, got, got_bs = run(inter_ctx, fp, dp, frames, pool, keys, mbs, co)
    bs = bs_reference(W, H, mbs, co, keys)
    assert np.array_equal(got_bs, words(bs)) and (W * H == 1 or not np.array_equal(got, before))
    want = deblock_reference(fp, dp, frames, mbs, before, bs)
    assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0])


@pytest.mark.gpu
def test_anchors_leave_the_picture_unchanged(inter_ctx):  # noqa: F811
    fp, pool, keys, mbs, co = _random_case(5, 5, 2, False, seed=3)
    before, got, _ = run(inter_ctx, fp, abi.make_deblock_params(1, 0, 0), 2, pool, keys, mbs, co)
    assert np.array_equal(got, before)                                  # disable_deblocking_filter_idc = 1
    mbs["mb_type"], mbs["flags"], mbs["ref_idx"], mbs["mv"] = 0, mbs["flags"] | 2, 1, (5, -9)
    before, got, got_bs = run(inter_ctx, fp, abi.make_deblock_params(0, 6, 6), 2, pool, keys, mbs, co)
    assert not got_bs.any() and np.array_equal(got, before)            # one vector, one picture, no residual: bS 0 everywhere


@pytest.mark.gpu
def test_chain_i_p_deblock_p_deblock(inter_ctx, recon_ctx):  # noqa: F811
    """I -> P -> deblock -> the reference of a second P -> deblock on the device, against oracle reconstruction, test_inter.reference and the filter above."""
    import torch
    (fp, _, mbs, co), dp, keys = ti.make_case(5, 5, 2, 1, "mixed", "mixed", (10, 44), 6, seed=8), abi.make_deblock_params(0, 1, 1), ([[0]], [[]])
    imbs, ico = synth.generate(fp, synth.config(i4x4=0.5, i8x8=0.0), 21, 0, 1)
    want = oracle.reconstruct(fp, 1, imbs, ico)[1]
    d = [torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).cuda() for v in (imbs, ico, mbs[:25], co[:25], mbs[25:], co[25:])]
    pics = [torch.zeros(384 * 25, dtype=torch.uint8, device="cuda") for _ in range(3)]
    recon_ctx.submit_device(fp, 1, d[0].data_ptr(), d[1].data_ptr(), pics[0].data_ptr())
    recon_ctx.sync()
    for k in (0, 1):   # no sync between a submit and its deblocking: the stage's stream orders them
        refs, m, c = [[pics[k].data_ptr()]], mbs[25 * k:25 * k + 25], co[25 * k:25 * k + 25]
        inter_ctx.submit_device(fp, 1, refs, d[2 + 2 * k].data_ptr(), d[3 + 2 * k].data_ptr(), pics[k + 1].data_ptr())
        inter_ctx.deblock_device(fp, dp, 1, False, refs, None, d[2 + 2 * k].data_ptr(), d[3 + 2 * k].data_ptr(), pics[k + 1].data_ptr())
        assert inter_ctx.sync() == 0
        want = deblock_reference(fp, dp, 1, m, ti.reference(fp, 1, [[want]], m, c)[1], bs_reference(5, 5, m, c, keys))
        assert np.array_equal(pics[k + 1].cpu().numpy(), want)
