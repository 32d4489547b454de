"""oracle/inter_model.py on its own, without a GPU: the restatement that the inter stage's GPU tests compare the kernels with,
against the hand-computed answers those tests carry (the same tables: tests/util.py) and against itself where two of its parts
must agree. A slip in the model shows here, where it cannot be mistaken for a kernel bug."""
import numpy as np
import pytest

from dryv_amd import abi
from oracle import deblock_model
from oracle.inter_model import bs_reference, deblock_reference, predict_b, predict_p
from util import BS_CASES, KEYS, KNOWN, P_HALF_ROWS, bs_case, known_b_case, make_p_case, single_list, split_planes


def test_p_known_answers():
    fp = abi.make_frame_params(1, 1)
    mbs, co = np.zeros(1, dtype=abi.INTER_MB_DTYPE), np.zeros((1, 384), dtype=np.int16)
    mbs["flags"], mbs["qp"] = 2, 26
    ref = np.random.default_rng(3).integers(0, 256, size=384, dtype=np.uint8)
    st, got = predict_p(fp, 1, [[ref]], mbs, co)
    assert st == 0 and np.array_equal(got, ref)                                         # zero vector: the reference picture
    mbs["mv"][0, :, 0] = 2                                                              # half sample to the right
    for row, want in P_HALF_ROWS:
        ref[:256] = np.tile(np.array(row, dtype=np.uint8), 16)
        got = predict_p(fp, 1, [[ref]], mbs, co)[1]
        assert got[:256].reshape(16, 16).tolist() == [want] * 16
    ref = np.random.default_rng(4).integers(0, 256, size=384, dtype=np.uint8)
    mbs["mv"][0, :] = (-4 * 1000, 4 * 1000)                                             # far off the bottom-left corner
    got = predict_p(fp, 1, [[ref]], mbs, co)[1]
    assert np.all(got[:256] == ref[240]) and np.all(got[256:320] == ref[256 + 56]) and np.all(got[320:] == ref[320 + 56])


@pytest.mark.parametrize("row", KNOWN, ids=lambda r: "mode%d-d%d" % r[:2])
def test_b_known_answers(row):
    fp, refs0, refs1, wts, mbs, co, want = known_b_case(row)
    st, got = predict_b(fp, 1, refs0, refs1, wts, mbs, co)
    assert st == 0 and np.all(got[:256] == want[0]) and np.all(got[256:] == want[1]), (got[:4], got[256:260])


@pytest.mark.parametrize("case", BS_CASES, ids=lambda c: c[0])
def test_bs_probes(case):
    fp, m, co = bs_case(case)
    bs = bs_reference(3, 2, m, co, KEYS)
    for (a, d, e, k), want in case[2].items():
        assert bs[a, d, e, k] == want, (a, d, e, k)


def test_single_list_b_equals_p():
    fp, refs, p, co = make_p_case(3, 2, 1, 2, "mixed", "mixed", (0, 51), 24, seed=41)
    st, want = predict_p(fp, 1, refs, p, co)
    got_st, got = predict_b(fp, 1, refs, [[]], None, single_list(p), co)
    assert st == got_st == 0 and np.array_equal(got, want) and want.any()


def test_filter_with_intra_bs_equals_the_intra_model():
    """All macroblocks intra: bs_reference gives 4 on macroblock edges and 3 inside (no odd edges where the 8x8 transform is on),
    and the per-segment filter must then be deblock_model's. Smooth macroblocks on different levels: steps that pass the thresholds."""
    W, H, rng = 3, 2, np.random.default_rng(17)
    fp, dp = abi.make_frame_params(W, H, cqo_cb=2, cqo_cr=-3, transform_8x8=True), abi.make_deblock_params(0, 2, -3)
    mbs, co = np.zeros(W * H, dtype=abi.INTER_MB_DTYPE), np.zeros((W * H, 384), dtype=np.int16)
    mbs["mb_type"], mbs["qp"], mbs["flags"] = 1, rng.integers(28, 46, size=W * H), [0, 1, 0, 1, 1, 0]
    yuv = np.zeros(384 * W * H, dtype=np.uint8)
    for plane, n in zip(split_planes(yuv, W, H), (16, 8, 8)):
        level = np.kron(rng.integers(100, 141, size=(H, W)), np.ones((n, n), dtype=np.int64))
        plane[:] = level + rng.integers(-6, 7, size=level.shape)
    bs = bs_reference(W, H, mbs, co, ([[]], [[]]))
    assert sorted(np.unique(bs)) == [0, 3, 4]
    got = deblock_reference(fp, dp, 1, mbs, yuv, bs)
    want = deblock_model.deblock(W, H, mbs["qp"], mbs["flags"] & 1, yuv, cqo_cb=2, cqo_cr=-3, alpha_div2=2, beta_div2=-3)
    assert np.array_equal(got, want)
    assert all((a != b).any() for a, b in zip(split_planes(got, W, H), split_planes(yuv, W, H)))   # every plane was filtered
