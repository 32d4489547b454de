"""The oracle against the hand-derived known-answer vectors (tests/golden/kat_vectors.json).

CPU only. These vectors are what pins the oracle (the reference has no fixtures of its own and
cannot be run here: "parity unpinned")."""
import json
import os

import numpy as np
import pytest

import oracle
from dryv_amd import abi
from util import build_frame_kat, check_luma, kat_mb, make_coeffs, make_mb, split_planes

with open(os.path.join(os.path.dirname(__file__), "golden", "kat_vectors.json")) as f:
    KAT = json.load(f)["vectors"]


FRAME_KATS = [v for v in KAT if "mbs" in v]
SINGLE_KATS = [v for v in KAT if v.get("kind") == "single_mb"]


@pytest.mark.parametrize("v", FRAME_KATS, ids=[v["name"] for v in FRAME_KATS])
def test_frame_kat(v):
    fp, mbs, co = build_frame_kat(v)
    st, yuv = oracle.reconstruct(fp, 1, mbs, co)
    assert st == 0
    Y, Cb, Cr = split_planes(yuv, v["W"], v["H"])
    check_luma(Y, v["expect"])
    assert np.all(Cb == v["expect"]["Cb"]), Cb
    assert np.all(Cr == v["expect"]["Cr"]), Cr


def build_single_kat(v):
    W, H = v["W"], v["H"]
    fp = abi.make_frame_params(W, H, transform_8x8=True)
    nb = v["neighbours"]
    yuv = np.zeros(384 * W * H, dtype=np.uint8)
    Y, Cb, Cr = split_planes(yuv, W, H)
    Y[:] = nb["Y"]
    Cb[:] = nb["Cb"]
    Cr[:] = nb["Cr"]
    if "Cb_bottom_row" in nb:
        Cb[7, :8] = nb["Cb_bottom_row"]
    kinds = np.full(W * H, nb["kind"], dtype=np.uint8)
    return fp, yuv, kinds, kat_mb(v["mb"]), make_coeffs(v["mb"]["coeffs"])


@pytest.mark.parametrize("v", SINGLE_KATS, ids=[v["name"] for v in SINGLE_KATS])
def test_single_mb_kat(v):
    fp, yuv, kinds, mb, co = build_single_kat(v)
    st, _ = oracle.decode_mb(fp, v["mbaddr"], mb, co, yuv, nb_kind=kinds)
    assert st == 0
    planes = dict(zip(("Y", "Cb", "Cr"), split_planes(yuv, v["W"], v["H"])))
    e = v["expect_region"]
    got = planes[e["plane"]][e["y0"]:e["y0"] + e["h"], e["x0"]:e["x0"] + e["w"]]
    assert np.array_equal(got, np.array(e["rows"], dtype=np.uint8)), got


def test_math_helpers():
    v = next(v for v in KAT if v["name"] == "math")
    lib = oracle.load()
    for val, lo, hi, want in v["clamp"]:
        assert lib.dryv_oracle_clamp(val, lo, hi) == want
    for a, b, c, d, e, want in v["inverse_raster_scan"]:
        assert lib.dryv_oracle_inverse_raster_scan(a, b, c, d, e) == want


def test_qpc_table():
    v = next(v for v in KAT if v["name"] == "qpc_table")
    for qpy, off, want in v["cases"]:
        fp = abi.make_frame_params(1, 1, cqo_cb=off, cqo_cr=off)
        assert oracle.get_qpc(fp, qpy, True) == want
        assert oracle.get_qpc(fp, qpy, False) == want


def test_residual_linearity_dc_only():
    # a lone DC coefficient gives a flat residual block: (d00 + 32) >> 6 everywhere
    fp = abi.make_frame_params(1, 1)
    for qp in range(0, 52):
        c = np.zeros((4, 4), dtype=np.int64)
        c[0, 0] = 7
        r = oracle.residual4x4(fp, qp, c)
        assert np.all(r == r[0, 0])
        ls = 16 * [10, 11, 13, 14, 16, 18][qp % 6]
        d = (7 * ls) << (qp // 6 - 4) if qp >= 24 else (7 * ls + (1 << (3 - qp // 6))) >> (4 - qp // 6)
        assert r[0, 0] == (d + 32) >> 6


def test_unsupported_records_are_reported():
    fp = abi.make_frame_params(2, 1)
    mbs = np.array([make_mb(kind=3), make_mb(kind=2)], dtype=abi.MB_DESC_DTYPE)
    co = np.zeros((2, 384), dtype=np.int16)
    st, yuv = oracle.reconstruct(fp, 1, mbs, co)
    assert st == abi.DRYV_E_UNSUPPORTED
    Y, _, _ = split_planes(yuv, 2, 1)
    assert np.all(Y[:, :16] == 0)          # the bad macroblock stays zero-filled
    assert np.all(Y[:, 16:] == 0)          # its neighbour DC-predicts from the zero column


def test_unsupported_params():
    fp = abi.make_frame_params(1, 1)
    fp.chroma_array_type = 3
    st, _ = oracle.reconstruct(fp, 1, np.array([make_mb()], dtype=abi.MB_DESC_DTYPE), np.zeros((1, 384), np.int16))
    assert st == abi.DRYV_E_UNSUPPORTED
