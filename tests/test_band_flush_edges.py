"""The band kernel's write-out at the edges of its staging groups: the luma flush (groups of NSY = 4 macroblocks), the
chroma flush (NSC = 8), the bottom-line / hand-off stores and the block chain's DC rounds, on the smallest pictures at which
a restructured flush, write-out or chain can go wrong. Every case is compared with oracle.reconstruct bit for bit, once
under the lane emulator (no GPU) and once through the C ABI (`-m gpu`).

Widths 1, 2, 3, 4, 5, 7, 8, 9, 13 give every residue of W mod 4 and mod 8, rows shorter than one flush group, and a last
macroblock that does and does not end a group; heights 1, 2, 3, 4, 5, 9 give bands of fewer than four rows, a last band of
one row, and pictures with and without a band below. Two pictures per batch: a team's second task starts from the first
one's leftover state. Three mixes: Intra16x16 only (no step has a DC round), Intra4x4 with every block predicted DC (every
round is a DC round: all prev_intra4x4_pred_mode flags set, so every mode is the default, DC), and a mixed batch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from dryv_amd import abi, synth
from util import first_mismatch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import emu  # noqa: E402

WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 13)
HEIGHTS = (1, 2, 3, 4, 5, 9)
FRAMES = 2
MIXES = {"i16_only": dict(i4x4=0.0, i8x8=0.0), "i4x4_all_dc": dict(i4x4=1.0, i8x8=0.0), "mixed": dict(i4x4=0.6, i8x8=0.0)}
_batches = {}


def batch(W, H, mix, t8=False):
    """(frame parameters, macroblocks, coefficients, the oracle's pictures): made once, shared by the emulator and GPU tests."""
    key = (W, H, mix, t8)
    if key not in _batches:
        fp = abi.make_frame_params(W, H, transform_8x8=t8)
        cfg = dict(i4x4=0.35, i8x8=0.4) if t8 else MIXES[mix]
        mbs, co = synth.generate(fp, synth.config(**cfg), 7000 + 100 * W + H, 0, FRAMES)
        if mix == "i4x4_all_dc":
            mbs = mbs.copy()
            mbs["prev_flags"] = 0xFFFF
        st, want = oracle.reconstruct(fp, FRAMES, mbs, co)
        assert st == 0
        want.setflags(write=False)
        _batches[key] = (fp, mbs, co, want)
    return _batches[key]


@pytest.mark.parametrize("mix", sorted(MIXES))
@pytest.mark.parametrize("W", WIDTHS)
def test_emulated_flush_edges(W, mix):
    for H in HEIGHTS:
        fp, mbs, co, want = batch(W, H, mix)
        st, got = emu_reconstruct(fp, mbs, co, teams=2 if H > 4 else 1)
        assert st == 0
        assert np.array_equal(got, want), "H=%d: %s" % (H, first_mismatch(got, want, W, H))


def emu_reconstruct(fp, mbs, co, teams=1):
    return emu.reconstruct(fp, FRAMES, mbs, co, teams)


@pytest.mark.parametrize("geo", [(5, 5), (9, 9)])
def test_emulated_flush_edges_8x8_build(geo):
    fp, mbs, co, want = batch(geo[0], geo[1], "mixed", t8=True)
    assert (mbs["mb_kind"] == 1).any()
    st, got = emu_reconstruct(fp, mbs, co, teams=2)
    assert st == 0
    assert np.array_equal(got, want), first_mismatch(got, want, *geo)


@pytest.mark.gpu
@pytest.mark.parametrize("mix", sorted(MIXES))
@pytest.mark.parametrize("W", WIDTHS)
def test_gpu_flush_edges(recon_ctx, W, mix):
    for H in HEIGHTS:
        fp, mbs, co, want = batch(W, H, mix)
        got = recon_ctx.reconstruct(fp, FRAMES, mbs, co)
        assert recon_ctx.last_status == 0
        assert np.array_equal(got, want), "H=%d: %s" % (H, first_mismatch(got, want, W, H))


@pytest.mark.gpu
@pytest.mark.parametrize("geo", [(5, 5), (9, 9)])
def test_gpu_flush_edges_8x8_build(recon_ctx, geo):
    fp, mbs, co, want = batch(geo[0], geo[1], "mixed", t8=True)
    assert (mbs["mb_kind"] == 1).any()
    got = recon_ctx.reconstruct(fp, FRAMES, mbs, co)
    assert recon_ctx.last_status == 0
    assert np.array_equal(got, want), first_mismatch(got, want, *geo)


_WIDE_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import dryv_amd
from test_band_flush_edges import batch, FRAMES
from util import first_mismatch
fp, mbs, co, want = batch(13, 9, "mixed")
with dryv_amd.ReconContext(0) as ctx:
    got = ctx.reconstruct(fp, FRAMES, mbs, co)
    assert ctx.last_status == 0
assert np.array_equal(got, want), first_mismatch(got, want, 13, 9)
print("wide ok")
"""


@pytest.mark.gpu
def test_gpu_flush_edges_wide_build():
    """The WIDE build of the kernel, forced through DRYV_RECON_FORCE_WIDE (read when the library loads: a child process)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, DRYV_RECON_FORCE_WIDE="1")
    r = subprocess.run([sys.executable, "-c", _WIDE_CHILD, os.path.dirname(here), here], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "wide ok" in r.stdout, r.stdout
