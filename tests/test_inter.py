"""The inter prediction stage (dryv_inter_*: P macroblocks, ITU-T H.264 8.4.2.2 + the inter residual path) against the plain
restatement of the standard on Python ints in oracle/inter_model.py (predict_p), bit for bit. dryv has no inter prediction
(README.md:12 unchecked): nothing here is parity with the reference."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from dryv_amd import abi
from oracle.inter_model import predict_p
from util import P_HALF_ROWS, first_mismatch, inter_ctx, make_p_case  # noqa: F401  (inter_ctx: the module's stage fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
def run(ctx, fp, frames, refs, mbs, co, allow_unsupported=False):
    import torch
    d_refs = [[torch.from_numpy(r).cuda() for r in per] for per in refs]
    d_m, d_c = torch.from_numpy(mbs.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(co).cuda()
    d_y = torch.full((frames * 384 * fp.pic_width_in_mbs * fp.pic_height_in_mbs,), 0xAA, dtype=torch.uint8, device="cuda")
    ctx.submit_device(fp, frames, [[t.data_ptr() for t in per] for per in d_refs], d_m.data_ptr(), d_c.data_ptr(), d_y.data_ptr())
    st = ctx.sync(allow_unsupported=allow_unsupported)
    return st, d_y.cpu().numpy()


@pytest.mark.gpu
def test_known_answers(inter_ctx):  # noqa: F811
    fp = abi.make_frame_params(1, 1)
    mbs, co = np.zeros(1, dtype=abi.INTER_MB_DTYPE), np.zeros((1, 384), dtype=np.int16)
    mbs["flags"], mbs["qp"] = 2, 26
    ref = np.random.default_rng(3).integers(0, 256, size=384, dtype=np.uint8)
    assert np.array_equal(run(inter_ctx, fp, 1, [[ref]], mbs, co)[1], ref)            # zero vector: the reference picture
    mbs["mv"][0, :, 0] = 2                                                              # half sample to the right
    for row, want in P_HALF_ROWS:
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
def test_against_reference(inter_ctx, case):  # noqa: F811
    W, H, frames, n_refs, mode, t8, qps, span = case
    span = 2 * 16 * max(W, H) if span == "2 x picture" else span
    fp, refs, mbs, co = make_p_case(W, H, frames, n_refs, mode, t8, qps, span, seed=7 * W + H)
    st, want = predict_p(fp, frames, refs, mbs, co)
    got = run(inter_ctx, fp, frames, refs, mbs, co)[1]
    assert st == 0 and np.array_equal(got, want), first_mismatch(got, want, W, H)


@pytest.mark.gpu
def test_status_and_alignment(inter_ctx):  # noqa: F811
    import dryv_amd
    import torch
    fp, refs, mbs, co = make_p_case(3, 2, 1, 2, "mixed", "no", (10, 40), 12, seed=99)
    mbs["mb_type"][1], mbs["ref_idx"][4][2] = 1, 2
    st, want = predict_p(fp, 1, refs, mbs, co)
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
    fp, _, mbs, co = make_p_case(W, H, 1, 1, "mixed", "no", (10, 40), 20, seed=5)
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
    assert np.array_equal(d_p.cpu().numpy(), predict_p(fp, 1, [[ipic]], mbs, co)[1])
