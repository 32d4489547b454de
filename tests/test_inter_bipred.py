"""The two-list inter prediction entry point (dryv_inter_submit_device_bipred: B macroblocks, weighted prediction) against a
plain-integer restatement of ITU-T H.264 8.4.2.3 on top of test_inter.py's restatement of 8.4.2.2 and the residual path, bit
for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import test_inter as ti
from dryv_amd import abi
from test_inter import inter_ctx  # noqa: F401  (the module's stage fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENOMS = ((0, 5, 7), (7, 0, 3))   # explicit mode: luma / chroma log2 denominators of pictures 0, 1, 2


def make_case(W, H, frames, n0, n1, mode, vectors, t8, seed):
    """Two P cases of test_inter.make_case (vectors, references; the first one's coefficients and flags) widened into one batch of
    dryv_inter_bmb records: every quadrant draws L0 / L1 / both, per quadrant or as a 16x8 / 8x16 split (all L0 without list 1,
    all both on a one-macroblock picture)."""
    rng = np.random.default_rng(seed)
    span = "far" if vectors == "far" else 24
    fp, refs0, p0, co = ti.make_case(W, H, frames, n0, "uniform" if vectors == "far" else vectors, t8, (0, 51), span, seed)
    _, refs1, p1, _ = ti.make_case(W, H, frames, max(n1, 1), "uniform" if vectors == "far" else vectors, t8, (0, 51), span, seed + 1)
    mbs = np.zeros(len(p0), dtype=abi.INTER_BMB_DTYPE)
    for k in ("qp", "flags"):
        mbs[k] = p0[k]
    mbs["mv"][:, 0], mbs["mv"][:, 1] = p0["mv"], p1["mv"]
    mbs["ref_idx"][:, 0], mbs["ref_idx"][:, 1] = p0["ref_idx"], p1["ref_idx"]
    for a in range(len(mbs)):
        d = rng.integers(0, 3, size=4)
        use = [d[q] for q in ((0, 1, 2, 3), (0, 0, 2, 2), (0, 1, 0, 1))[int(rng.integers(0, 3))]]   # 0 L0, 1 L1, 2 both
        use = [0] * 4 if n1 == 0 else [2] * 4 if W * H == 1 else use
        for q in range(4):
            if use[q] != 2:
                mbs["ref_idx"][a, 1 - use[q], q] = -1
    wts = None
    if mode != "default":
        wts = np.zeros(frames, dtype=abi.INTER_WEIGHTS_DTYPE)
        wts["mode"] = 1 if mode == "explicit" else 2
        for f in range(frames if mode == "explicit" else 0):
            wts["luma_log2_denom"][f], wts["chroma_log2_denom"][f] = DENOMS[0][f % 3], DENOMS[1][f % 3]
            w = rng.integers(-128, 128, size=(2, 16, 3))
            unit = np.array([1 << DENOMS[0][f % 3]] + [1 << DENOMS[1][f % 3]] * 2)
            wts["expl"]["w"][f] = np.where(rng.random((2, 16, 3)) < 0.25, unit, w)
            wts["expl"]["o"][f] = rng.integers(-128, 128, size=(2, 16, 3))
        if mode == "implicit":
            wts["implicit_w1"] = rng.integers(-64, 129, size=(frames, 16, 16))
            wts["implicit_w1"][:, 0, 0], wts["implicit_w1"][:, 0, 1 % max(n1, 1)] = -64, 128
    return fp, refs0, (refs1 if n1 else [[] for _ in range(frames)]), wts, mbs, co


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


def reference(fp, frames, refs0, refs1, wts, mbs, co):
    """(status, yuv). Each list's prediction is test_inter.reference over P records without residual; the weighted combination
    is Python ints; the residual is added by test_inter.reference predicting, with zero vectors, from the combined picture."""
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
        pred.append(ti.reference(fp, frames, refs if n1 or X == 0 else refs0, p, co)[1].astype(np.int64))
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
    st, out = ti.reference(fp, frames, [[comb[f * 384 * per:(f + 1) * 384 * per]] for f in range(frames)], p, co)
    return st, out


def run(ctx, fp, frames, refs0, refs1, wts, mbs, co, allow_unsupported=False):
    import torch
    d0, d1 = ([[torch.from_numpy(x).cuda() for x in per] for per in refs] for refs in (refs0, refs1))
    d_m, d_c = torch.from_numpy(mbs.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(co).cuda()
    d_y = torch.full((frames * 384 * fp.pic_width_in_mbs * fp.pic_height_in_mbs,), 0xAA, dtype=torch.uint8, device="cuda")
    ctx.submit_device_bipred(fp, frames, [[t.data_ptr() for t in per] for per in d0], [[t.data_ptr() for t in per] for per in d1], wts,
                             d_m.data_ptr(), d_c.data_ptr(), d_y.data_ptr())
    return ctx.sync(allow_unsupported=allow_unsupported), d_y.cpu().numpy()


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_layout_and_validation():
    assert C.sizeof(abi.InterBmb) == 144 == abi.INTER_BMB_DTYPE.itemsize and abi.InterBmb.mv.offset == 16 == abi.INTER_BMB_DTYPE.fields["mv"][1]
    assert C.sizeof(abi.InterWeights) == 1040 == abi.INTER_WEIGHTS_DTYPE.itemsize
    assert abi.InterWeights.expl.offset == 16 == abi.INTER_WEIGHTS_DTYPE.fields["expl"][1]
    assert abi.InterWeights.implicit_w1.offset == 528 == abi.INTER_WEIGHTS_DTYPE.fields["implicit_w1"][1]
    lib, fp = abi.load_library(), abi.make_frame_params(4, 3)
    check = lambda n0, n1, w=None: lib.dryv_inter_check_bipred(C.byref(fp), 2, n0, n1, None if w is None else w.ctypes.data)
    assert [check(1, 0), check(16, 16)] == [abi.DRYV_OK] * 2
    assert [check(0, 1), check(17, 1), check(1, 17)] == [abi.DRYV_E_INVALID] * 3
    w = np.zeros(2, dtype=abi.INTER_WEIGHTS_DTYPE)
    w["mode"], w["luma_log2_denom"], w["chroma_log2_denom"] = 1, 7, 7
    assert check(1, 1, w) == abi.DRYV_OK
    w["mode"][1] = 3
    assert check(1, 1, w) == abi.DRYV_E_INVALID
    w["mode"][1], w["chroma_log2_denom"][1] = 1, 8
    assert check(1, 1, w) == abi.DRYV_E_INVALID
    fp.chroma_array_type = 2
    assert check(1, 1) == abi.DRYV_E_UNSUPPORTED


def test_kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from resource_usage import resource_usage
    usage = resource_usage(os.path.join(ROOT, "dryv_amd", "csrc", "inter_bi.hip"))
    assert usage
    for name, got in usage.items():
        assert got["VGPRs Spill"] == 0 and got["ScratchSize"] == 0, (name, got)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
# (mode, luma denom, chroma denom, luma w, o, chroma w, o, implicit w1, lists) -> (Y, C) from flat references 200 / 100
KNOWN = [(0, 0, 0, None, None, None, None, None, (0, 0), (150, 150)),
         (1, 5, 2, (64, -32), (3, 3), (3, 2), (-5, -6), None, (0, 0), (153, 95)),        # C: (804 >> 3) + (-10 >> 1) = 100 - 5
         (1, 7, 0, (-128, 127), (127, 127), (1, -1), (-20, -21), None, (0, 0), (77, 30)),  # Y: (-12772 >> 8) + 127; C: (101 >> 1) - 20
         (1, 0, 3, (0, -1), (0, 10), (0, 20), (0, -7), None, (-1, 0), (0, 243)),          # list 1 only; C: (2004 >> 3) - 7
         (2, 0, 0, None, None, None, None, 128, (0, 0), (0, 0)),
         (2, 0, 0, None, None, None, None, -64, (0, 0), (255, 255))]


@pytest.mark.gpu
@pytest.mark.parametrize("row", KNOWN, ids=lambda r: "mode%d-d%d" % r[:2])
def test_known_answers(inter_ctx, row):  # noqa: F811
    mode, dl, dc, wl, ol, wc, oc, w1, lists, want = row
    fp = abi.make_frame_params(1, 1)
    mbs, co = np.zeros(1, dtype=abi.INTER_BMB_DTYPE), np.zeros((1, 384), dtype=np.int16)
    mbs["flags"], mbs["qp"], mbs["ref_idx"][0] = 2, 26, np.array(lists)[:, None]
    wts = np.zeros(1, dtype=abi.INTER_WEIGHTS_DTYPE)
    wts["mode"], wts["luma_log2_denom"], wts["chroma_log2_denom"] = mode, dl, dc
    if mode == 1:
        wts["expl"]["w"][0, :, 0, 0], wts["expl"]["o"][0, :, 0, 0] = wl, ol
        wts["expl"]["w"][0, :, 0, 1:], wts["expl"]["o"][0, :, 0, 1:] = np.array(wc)[:, None], np.array(oc)[:, None]
    if mode == 2:
        wts["implicit_w1"][0, 0, 0] = w1
    refs = [[np.full(384, v, dtype=np.uint8)] for v in (200, 100)]
    got = run(inter_ctx, fp, 1, [refs[0]], [refs[1]], wts if mode else None, mbs, co)[1]
    assert np.all(got[:256] == want[0]) and np.all(got[256:] == want[1]), (got[:4], got[256:260])


CASES = [(1, 1, 1, 1, 1, "default", "far", "no"), (3, 2, 2, 2, 2, "default", "block", "no"), (3, 2, 3, 3, 2, "explicit", "quadrant", "yes"),
         (5, 3, 1, 16, 16, "implicit", "mixed", "mixed"), (3, 2, 1, 2, 0, "explicit", "mixed", "no")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-%d+%dref-%s-%s-%s" % c)
def test_against_reference(inter_ctx, case):  # noqa: F811
    W, H, frames = case[:3]
    fp, refs0, refs1, wts, mbs, co = make_case(*case, seed=11 * W + H + frames)
    st, want = reference(fp, frames, refs0, refs1, wts, mbs, co)
    got = run(inter_ctx, fp, frames, refs0, refs1, wts, mbs, co)[1]
    from util import first_mismatch
    assert st == 0 and np.array_equal(got, want), first_mismatch(got, want, W, H)


@pytest.mark.gpu
def test_single_list_equals_p_kernel(inter_ctx):  # noqa: F811
    """The same P records through both entry points on one context, before one sync."""
    import torch
    fp, refs, p, co = ti.make_case(5, 3, 2, 3, "mixed", "mixed", (0, 51), 24, seed=41)
    b = np.zeros(len(p), dtype=abi.INTER_BMB_DTYPE)
    for k in ("mb_type", "qp", "flags"):
        b[k] = p[k]
    b["ref_idx"][:, 0], b["ref_idx"][:, 1], b["mv"][:, 0] = p["ref_idx"], -1, p["mv"]
    d_refs = [[torch.from_numpy(r).cuda() for r in per] for per in refs]
    ptrs = [[t.data_ptr() for t in per] for per in d_refs]
    d_p, d_b, d_c = (torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda() for x in (p, b, co))
    out = [torch.full((2 * 384 * 15,), 0xAA, dtype=torch.uint8, device="cuda") for _ in range(2)]
    inter_ctx.submit_device(fp, 2, ptrs, d_p.data_ptr(), d_c.data_ptr(), out[0].data_ptr())
    inter_ctx.submit_device_bipred(fp, 2, ptrs, [[], []], None, d_b.data_ptr(), d_c.data_ptr(), out[1].data_ptr())
    assert inter_ctx.sync() == 0 and torch.equal(out[0], out[1]) and not bool((out[0] == 0xAA).all())


@pytest.mark.gpu
def test_status_and_alignment(inter_ctx):  # noqa: F811
    import dryv_amd
    import torch
    fp, refs0, refs1, wts, mbs, co = make_case(3, 2, 1, 2, 2, "default", "mixed", "no", seed=77)
    mbs["ref_idx"][0, :, 2] = -1                        # a quadrant that uses no list
    mbs["ref_idx"][2, 1, 1] = 2                         # >= n_refs1
    mbs["mb_type"][4] = 1
    st, want = reference(fp, 1, refs0, refs1, wts, mbs, co)
    got_st, got = run(inter_ctx, fp, 1, refs0, refs1, wts, mbs, co, allow_unsupported=True)
    assert st == got_st == abi.DRYV_E_UNSUPPORTED and np.array_equal(got, want)
    Y = got[:256 * 6].reshape(32, 48)
    assert not Y[:16, :16].any() and not Y[:16, 32:].any() and not Y[16:, 16:32].any() and Y[:16, 16:32].any() and Y[16:, :16].any()
    buf = torch.zeros(384 * 6 + 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(dryv_amd.ReconError) as e:
        inter_ctx.submit_device_bipred(fp, 1, [[buf.data_ptr()] * 2], [[buf.data_ptr(), buf.data_ptr() + 4]], None, buf.data_ptr(),
                                       buf.data_ptr(), buf.data_ptr())
    assert e.value.status == abi.DRYV_E_INVALID
