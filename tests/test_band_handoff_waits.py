"""The band kernel's hand-off between bands, at the shapes where a granule that is looked at too early, requested for the
wrong macroblock or served from the launch before shows: pictures 1, 2, 3, 4 and 130 macroblocks wide (the `s + 1 < W` /
`s + 2 < W` edges of the look and the request; more than one batch of 64 of the mode pre-pass), 5, 8 and 9 macroblock rows
(a partial last band; two or three bands that follow each other directly), both transform settings, 1 and 40 pictures,
and grids of one and two workgroups (DRYV_RECON_GRID), where the bands of a picture are run by the same team or by two
neighbours in immediate succession: the band below then really arrives before the band above has published, and the poll
behind the first look is taken. Every geometry is launched four times on one context with different content (a granule's
tag is the launch's generation: the launch before left a complete set of valid-looking records at the same addresses).
Bit-exact against oracle.reconstruct."""
import os

import numpy as np
import pytest

import oracle
from dryv_amd import abi, synth, ReconContext
from util import first_mismatch

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 4, 130)
HEIGHTS = (5, 8, 9)
FRAMES = (1, 40)
LAUNCHES = 4
_cache = {}


def batch(W, H, t8, frames, k):
    """Content k of a geometry with its expected pictures: computed once, shared by every test, never written to."""
    key = (W, H, t8, frames, k)
    if key not in _cache:
        fp = abi.make_frame_params(W, H, transform_8x8=t8)
        cfg = synth.config(i4x4=0.4, i8x8=0.3) if t8 else synth.config(i4x4=0.6, i8x8=0.0)
        mbs, co = synth.generate(fp, cfg, 7300 + 10 * k + W, 0, frames)
        st, want = oracle.reconstruct(fp, frames, mbs, co)
        assert st == 0
        want.setflags(write=False)
        _cache[key] = (fp, mbs, co, want)
    return _cache[key]


def context(**env):
    """A context created under the given DRYV_RECON_* settings (the library reads them when a context is created)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return ReconContext(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def run_geometries(ctx, t8, widths=WIDTHS, heights=HEIGHTS, frames_list=FRAMES):
    for W in widths:
        for H in heights:
            for frames in frames_list:
                for k in range(LAUNCHES):
                    fp, mbs, co, want = batch(W, H, t8, frames, k)
                    got = ctx.reconstruct(fp, frames, mbs, co)
                    assert ctx.last_status == 0, (W, H, frames, k, ctx.last_status)
                    assert np.array_equal(got, want), ((W, H, frames, k), first_mismatch(got, want, W, H))


@pytest.mark.parametrize("t8", [False, True], ids=["no8x8", "8x8"])
@pytest.mark.parametrize("grid", ["1", "2"])
def test_handoff_small_grids(grid, t8):
    run_geometries(context(DRYV_RECON_GRID=grid), t8)


@pytest.mark.parametrize("t8", [False, True], ids=["no8x8", "8x8"])
def test_handoff_default_grid(recon_ctx, t8):
    run_geometries(recon_ctx, t8)


def test_handoff_wide_build():
    """The WIDE builds' step loops are the same source under other register pressure: once, through the test hook."""
    ctx = context(DRYV_RECON_GRID="2", DRYV_RECON_FORCE_WIDE="1")
    for t8 in (False, True):
        run_geometries(ctx, t8, widths=(3, 130), heights=(9,), frames_list=(1, 40))
