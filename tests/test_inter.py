"""The inter prediction stage (dryv_inter_*: P macroblocks, ITU-T H.264 8.4.2.2 + the inter residual path) against a plain
restatement of the standard on Python ints, bit for bit. dryv has no inter prediction (README.md:12 unchecked): nothing here
is parity with the reference; the residual arithmetic is oracle.spec_model's (level_scale4/8, residual4x4/8x8, qp_chroma)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from dryv_amd import abi
from oracle import spec_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAP = lambda v: v[0] - 5 * v[1] + 20 * v[2] + 20 * v[3] - 5 * v[4] + v[5]
CLIP = lambda v: min(max(v, 0), 255)


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


def reference(fp, frames, refs, mbs, co):
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


def make_case(W, H, frames, n_refs, mode, t8, qps, span, seed):
    """Random records / coefficients / reference pictures. span: vector range in luma samples, or "far": beyond the picture.
    Coefficients are bounded by construction: per 4x4 block two AC entries of at most 10000 / max scaled LevelScale each and
    a DC share of 10000 (8x8: two entries of 6000 / ...: gain 2.25), so that no value of 8.5.12 - 8.5.13 leaves 16 bits."""
    rng = np.random.default_rng(seed)
    lists4, lists8 = rng.integers(8, 21, size=(6, 16)), rng.integers(8, 21, size=(6, 64))
    fp = abi.make_frame_params(W, H, cqo_cb=int(rng.integers(-6, 7)), cqo_cr=int(rng.integers(-6, 7)), transform_8x8=t8 != "no",
                               scaling4x4=lists4, scaling8x8=lists8)
    refs = [[rng.integers(0, 256, size=384 * W * H, dtype=np.uint8) for _ in range(n_refs)] for _ in range(frames)]
    n = frames * W * H
    mbs, co = np.zeros(n, dtype=abi.INTER_MB_DTYPE), np.zeros((n, 384), dtype=np.int16)
    k = 0   # running count of per-block vectors: every luma and chroma fraction occurs by construction
    for a in range(n):
        qp = int(rng.integers(qps[0], qps[1] + 1))
        m = mode if mode != "mixed" else ("uniform", "quadrant", "block")[int(rng.integers(0, 3))]
        far = lambda: int(rng.integers(200, 4001)) * (1 if rng.random() < 0.5 else -1)
        vec = lambda: (far(), far()) if span == "far" else tuple(int(v) for v in rng.integers(-4 * span, 4 * span + 1, size=2))
        if m == "block":
            for b in range(16):
                vx, vy = vec()
                mbs["mv"][a][b] = ((vx & ~7) | (k & 7), (vy & ~7) | ((k >> 3) & 7))
                k += 1
        else:
            v4 = [vec() for _ in range(4)]
            for b in range(16):
                mbs["mv"][a][b] = v4[0] if m == "uniform" else v4[b >> 2]
        one_ref = m == "uniform" and rng.random() < 0.8   # (a single vector over different references: the per-quadrant path)
        mbs["ref_idx"][a] = int(rng.integers(0, n_refs)) if one_ref else rng.integers(0, n_refs, size=4)
        use8 = t8 == "yes" or (t8 == "mixed" and rng.random() < 0.5)
        mbs["qp"][a], mbs["flags"][a] = qp, int(use8)
        kind = rng.random()
        if kind < 1 / 3:            # no residual: the slot must not be read
            mbs["flags"][a] |= 2
            co[a] = 0x7FFF
            continue
        if kind < 0.4:              # a coded macroblock whose coefficients are all zero
            continue
        cap4 = lambda q: max(1, (29 * 20) << max(q // 6 - 4, 0) >> max(4 - q // 6, 0))
        if use8:
            cmax = min(500, 6000 // max(1, (58 * 20) << max(qp // 6 - 6, 0) >> max(6 - qp // 6, 0)))
            for q in range(4):
                co[a, 64 * q + rng.choice(64, size=2, replace=False)] = rng.integers(-cmax, cmax + 1, size=2)
        else:
            cmax = min(500, 10000 // cap4(qp))
            for b in range(16):
                co[a, 16 * b + rng.choice(16, size=2, replace=False)] = rng.integers(-cmax, cmax + 1, size=2)
        for pl in range(2):
            qpc = sm.qp_chroma(qp, (fp.chroma_qp_index_offset, fp.second_chroma_qp_index_offset)[pl])
            cmax, dmax = min(500, 10000 // cap4(qpc)), min(500, 10000 // (4 * max(1, (18 * 20 << (qpc // 6)) >> 5)))
            co[a, 256 + 64 * pl:260 + 64 * pl] = rng.integers(-dmax, dmax + 1, size=4)
            for blk in range(4):
                co[a, 260 + 64 * pl + 15 * blk + rng.choice(15, size=2, replace=False)] = rng.integers(-cmax, cmax + 1, size=2)
    return fp, refs, mbs, co


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_layout_and_validation():
    assert C.sizeof(abi.InterMb) == 80 == abi.INTER_MB_DTYPE.itemsize and abi.InterMb.mv.offset == 16 == abi.INTER_MB_DTYPE.fields["mv"][1]
    lib, fp = abi.load_library(), abi.make_frame_params(4, 3)
    assert [lib.dryv_inter_check(C.byref(fp), 2, r) for r in (1, 16, 0, 17)] == [abi.DRYV_OK, abi.DRYV_OK, abi.DRYV_E_INVALID, abi.DRYV_E_INVALID]
    fp.chroma_array_type = 2
    assert lib.dryv_inter_check(C.byref(fp), 2, 1) == abi.DRYV_E_UNSUPPORTED


def test_kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from resource_usage import resource_usage
    usage = resource_usage(os.path.join(ROOT, "dryv_amd", "csrc", "inter.hip"))
    assert usage
    for name, got in usage.items():
        assert got["VGPRs Spill"] == 0 and got["ScratchSize"] == 0, (name, got)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inter_ctx():
    import dryv_amd
    with dryv_amd.InterContext(0) as ctx:
        yield ctx


def run(ctx, fp, frames, refs, mbs, co, allow_unsupported=False):
    import torch
    d_refs = [[torch.from_numpy(r).cuda() for r in per] for per in refs]
    d_m, d_c = torch.from_numpy(mbs.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(co).cuda()
    d_y = torch.full((frames * 384 * fp.pic_width_in_mbs * fp.pic_height_in_mbs,), 0xAA, dtype=torch.uint8, device="cuda")
    ctx.submit_device(fp, frames, [[t.data_ptr() for t in per] for per in d_refs], d_m.data_ptr(), d_c.data_ptr(), d_y.data_ptr())
    st = ctx.sync(allow_unsupported=allow_unsupported)
    return st, d_y.cpu().numpy()


@pytest.mark.gpu
def test_known_answers(inter_ctx):
    fp = abi.make_frame_params(1, 1)
    mbs, co = np.zeros(1, dtype=abi.INTER_MB_DTYPE), np.zeros((1, 384), dtype=np.int16)
    mbs["flags"], mbs["qp"] = 2, 26
    ref = np.random.default_rng(3).integers(0, 256, size=384, dtype=np.uint8)
    assert np.array_equal(run(inter_ctx, fp, 1, [[ref]], mbs, co)[1], ref)            # zero vector: the reference picture
    mbs["mv"][0, :, 0] = 2                                                              # half sample to the right
    for row, want in (([10] * 3 + [50] * 13, [11, 5, 30, 55, 49] + [50] * 11),          # (10 - 50 + 200 + 1000 - 250 + 50 + 16) >> 5 = 30
                      ([0, 0, 255, 255] + [0] * 12, [0, 120, 255, 120, 0, 8] + [0] * 10)):   # (10200 + 16) >> 5 = 319 -> 255
        ref[:256] = np.tile(np.array(row, dtype=np.uint8), 16)
        got = run(inter_ctx, fp, 1, [[ref]], mbs, co)[1]
        assert got[:256].reshape(16, 16).tolist() == [want] * 16
    ref = np.random.default_rng(4).integers(0, 256, size=384, dtype=np.uint8)
    mbs["mv"][0, :] = (-4 * 1000, 4 * 1000)                                             # far off the bottom-left corner
    got = run(inter_ctx, fp, 1, [[ref]], mbs, co)[1]
    assert np.all(got[:256] == ref[240]) and np.all(got[256:320] == ref[256 + 56]) and np.all(got[320:] == ref[320 + 56])


CASES = [(1, 1, 1, 1, "uniform", "no", (0, 51), "far"), (3, 2, 2, 1, "uniform", "no", (0, 51), 24), (3, 2, 1, 3, "quadrant", "yes", (0, 51), 24),
         (5, 3, 2, 2, "block", "no", (20, 30), 40), (5, 3, 1, 16, "mixed", "mixed", (0, 51), "2 x picture"), (20, 2, 1, 1, "uniform", "yes", (36, 51), 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-%dref-%s-%s" % c[:6])
def test_against_reference(inter_ctx, case):
    W, H, frames, n_refs, mode, t8, qps, span = case
    span = 2 * 16 * max(W, H) if span == "2 x picture" else span
    fp, refs, mbs, co = make_case(W, H, frames, n_refs, mode, t8, qps, span, seed=7 * W + H)
    st, want = reference(fp, frames, refs, mbs, co)
    got = run(inter_ctx, fp, frames, refs, mbs, co)[1]
    from util import first_mismatch
    assert st == 0 and np.array_equal(got, want), first_mismatch(got, want, W, H)


@pytest.mark.gpu
def test_status_and_alignment(inter_ctx):
    import dryv_amd
    import torch
    fp, refs, mbs, co = make_case(3, 2, 1, 2, "mixed", "no", (10, 40), 12, seed=99)
    mbs["mb_type"][1], mbs["ref_idx"][4][2] = 1, 2
    st, want = reference(fp, 1, refs, mbs, co)
    got_st, got = run(inter_ctx, fp, 1, refs, mbs, co, allow_unsupported=True)
    assert st == got_st == abi.DRYV_E_UNSUPPORTED and np.array_equal(got, want)
    Y = got[:256 * 6].reshape(32, 48)
    assert not Y[:16, 16:32].any() and not Y[16:, 16:32].any() and Y[:16, :16].any()
    buf = torch.zeros(384 * 6 + 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(dryv_amd.ReconError) as e:
        inter_ctx.submit_device(fp, 1, [[buf.data_ptr() + 4, buf.data_ptr()]], buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
    assert e.value.status == abi.DRYV_E_INVALID


@pytest.mark.gpu
def test_chained_with_reconstruction(recon_ctx):
    """An I picture through ReconContext, then a P picture predicted from it by a stage that borrows the context's stream."""
    import dryv_amd
    import oracle
    import torch
    from dryv_amd import synth
    W, H = 4, 3
    fp, _, mbs, co = make_case(W, H, 1, 1, "mixed", "no", (10, 40), 20, seed=5)
    imbs, ico = synth.generate(fp, synth.config(i4x4=0.5, i8x8=0.0), 21, 0, 1)
    st, ipic = oracle.reconstruct(fp, 1, imbs, ico)
    assert st == 0
    d = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda() for x in (imbs, ico, mbs, co)]
    d_i, d_p = (torch.zeros(384 * W * H, dtype=torch.uint8, device="cuda") for _ in range(2))
    with dryv_amd.InterContext(0, stream=recon_ctx.stream) as ictx:
        recon_ctx.submit_device(fp, 1, d[0].data_ptr(), d[1].data_ptr(), d_i.data_ptr())
        recon_ctx.sync()
        ictx.submit_device(fp, 1, [[d_i.data_ptr()]], d[2].data_ptr(), d[3].data_ptr(), d_p.data_ptr())
        ictx.sync()
        assert ictx.last_kernel_ms() > 0
    assert np.array_equal(d_i.cpu().numpy(), ipic)
    assert np.array_equal(d_p.cpu().numpy(), reference(fp, 1, [[ipic]], mbs, co)[1])
