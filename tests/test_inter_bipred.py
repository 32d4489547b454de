"""The two-list inter prediction entry point (dryv_inter_submit_device_bipred: B macroblocks, weighted prediction) against the
plain-integer restatement of ITU-T H.264 8.4.2.3 in oracle/inter_model.py (predict_b, on top of predict_p's 8.4.2.2 and residual
path), bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from dryv_amd import abi
from oracle.inter_model import predict_b
from util import KNOWN, first_mismatch, inter_ctx, known_b_case, make_b_case, make_p_case, single_list  # noqa: F401  (inter_ctx: the module's stage fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
@pytest.mark.gpu
@pytest.mark.parametrize("row", KNOWN, ids=lambda r: "mode%d-d%d" % r[:2])
def test_known_answers(inter_ctx, row):  # noqa: F811
    fp, refs0, refs1, wts, mbs, co, want = known_b_case(row)
    got = run(inter_ctx, fp, 1, refs0, refs1, wts, mbs, co)[1]
    assert np.all(got[:256] == want[0]) and np.all(got[256:] == want[1]), (got[:4], got[256:260])


CASES = [(1, 1, 1, 1, 1, "default", "far", "no"), (3, 2, 2, 2, 2, "default", "block", "no"), (3, 2, 3, 3, 2, "explicit", "quadrant", "yes"),
         (5, 3, 1, 16, 16, "implicit", "mixed", "mixed"), (3, 2, 1, 2, 0, "explicit", "mixed", "no")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-%d+%dref-%s-%s-%s" % c)
def test_against_reference(inter_ctx, case):  # noqa: F811
    W, H, frames = case[:3]
    fp, refs0, refs1, wts, mbs, co = make_b_case(*case, seed=11 * W + H + frames)
    st, want = predict_b(fp, frames, refs0, refs1, wts, mbs, co)
    got = run(inter_ctx, fp, frames, refs0, refs1, wts, mbs, co)[1]
    assert st == 0 and np.array_equal(got, want), first_mismatch(got, want, W, H)


@pytest.mark.gpu
def test_single_list_equals_p_kernel(inter_ctx):  # noqa: F811
    """The same P records through both entry points on one context, before one sync."""
    import torch
    fp, refs, p, co = make_p_case(5, 3, 2, 3, "mixed", "mixed", (0, 51), 24, seed=41)
    b = single_list(p)
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
    fp, refs0, refs1, wts, mbs, co = make_b_case(3, 2, 1, 2, 2, "default", "mixed", "no", seed=77)
    mbs["ref_idx"][0, :, 2] = -1                        # a quadrant that uses no list
    mbs["ref_idx"][2, 1, 1] = 2                         # >= n_refs1
    mbs["mb_type"][4] = 1
    st, want = predict_b(fp, 1, refs0, refs1, wts, mbs, co)
    got_st, got = run(inter_ctx, fp, 1, refs0, refs1, wts, mbs, co, allow_unsupported=True)
    assert st == got_st == abi.DRYV_E_UNSUPPORTED and np.array_equal(got, want)
    Y = got[:256 * 6].reshape(32, 48)
    assert not Y[:16, :16].any() and not Y[:16, 32:].any() and not Y[16:, 16:32].any() and Y[:16, 16:32].any() and Y[16:, :16].any()
    buf = torch.zeros(384 * 6 + 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(dryv_amd.ReconError) as e:
        inter_ctx.submit_device_bipred(fp, 1, [[buf.data_ptr()] * 2], [[buf.data_ptr(), buf.data_ptr() + 4]], None, buf.data_ptr(),
                                       buf.data_ptr(), buf.data_ptr())
    assert e.value.status == abi.DRYV_E_INVALID
