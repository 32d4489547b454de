"""In-loop deblocking of the inter stage's P and B pictures (dryv_inter_deblock_device) against the plain-integer restatement of ITU-T H.264 8.7 with bS
per edge segment, and of 8.7.2.1's bS rule for frame macroblocks, in oracle/inter_model.py (bs_reference, deblock_reference), bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle
from dryv_amd import abi, synth
from oracle.inter_model import TC0, bs_reference, deblock_reference, predict_p, words
from util import BS_CASES, KEYS, bs_case, inter_ctx, make_b_case, make_p_case  # noqa: F401  (inter_ctx: the module's stage fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
@pytest.mark.gpu
@pytest.mark.parametrize("case", BS_CASES, ids=lambda c: c[0])
def test_bs_records(inter_ctx, case):  # noqa: F811
    (fp, m, co), rng = bs_case(case), np.random.default_rng(1)
    pool, yuv = [rng.integers(0, 256, size=384 * 6, dtype=np.uint8) for _ in range(2)], rng.integers(0, 256, size=384 * 12, dtype=np.uint8)
    got = run(inter_ctx, fp, abi.make_deblock_params(), 2, pool, KEYS, m, co, yuv)[2]
    for (a, d, e, k), want in case[2].items():
        assert (got[a, d, e] >> (4 * k)) & 15 == want, ((a, d, e, k), hex(got[a, d, e]))
    assert np.array_equal(got, words(bs_reference(3, 2, m, co, KEYS)))


def _random_case(W, H, frames, bi, seed):
    fp, r0, r1, _, mbs, co = make_b_case(W, H, frames, 2, 2, "default", "mixed", "mixed", seed) if bi else (
        lambda c: (c[0], c[1], [[]] * frames, None, c[2], c[3]))(make_p_case(W, H, frames, 2, "mixed", "mixed", (0, 51), 3, seed))
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
    """I -> P -> deblock -> the reference of a second P -> deblock on the device, against oracle reconstruction, predict_p and the model's filter."""
    import torch
    (fp, _, mbs, co), dp, keys = make_p_case(5, 5, 2, 1, "mixed", "mixed", (10, 44), 6, seed=8), abi.make_deblock_params(0, 1, 1), ([[0]], [[]])
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
        want = deblock_reference(fp, dp, 1, m, predict_p(fp, 1, [[want]], m, c)[1], bs_reference(5, 5, m, c, keys))
        assert np.array_equal(pics[k + 1].cpu().numpy(), want)
