"""Without a GPU: (1) the restructured look / poll of the hand-off granules under the CPU lane emulator, at the geometries of
tests/test_band_handoff_waits.py; (2) what the compiler made of it: tools/handoff_waits.py cross-compiles the four builds
of the band kernel for gfx950 (as tests/test_kernel_resources.py does) and lists the vmcnt waits inside the marked regions
of FRONT's and CHROMA's step loops."""
import os
import sys

import numpy as np
import pytest

import oracle
from dryv_amd import abi, synth
from util import first_mismatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import emu  # noqa: E402
from handoff_waits import waits  # noqa: E402

BUILDS = ("<false,false>", "<true,false>", "<false,true>", "<true,true>")
# The regions of a step that every step runs through (the poll and a band's first step are blocks of their own, outside the
# marks). None of them may drain the wave's vector-memory queue ...
FAST = ("front.look", "front.request", "front.prefetch", "front.free", "front.record",
        "chroma.look", "chroma.request", "chroma.prefetch", "chroma.stores")
# ... and the waits that remain are the ones the source places and says why (band_kernel.h): CHROMA waits for its step's
# loads once, in front of its stores, with vmcnt(0) (loads and stores share the counter and are not counted across).
COUNTED = {"chroma.settle": [0]}


@pytest.fixture(scope="module")
def listing():
    return waits()


@pytest.mark.parametrize("build", BUILDS)
def test_fast_path_regions_do_not_drain(listing, build):
    regions = listing[build]
    for name in FAST:
        assert name in regions, (build, sorted(regions))
        assert regions[name]["waits"] == [], (build, name, regions[name])
    # the regions are where the source says: the request is the one granule load, the stores are stores
    assert regions["front.request"]["vmem"] == ["global_load_dwordx2"]
    assert regions["chroma.request"]["vmem"] == ["global_load_dwordx2"]
    assert regions["chroma.stores"]["vmem"] and all(m.startswith("global_store") for m in regions["chroma.stores"]["vmem"])


@pytest.mark.parametrize("build", BUILDS)
def test_counted_waits_are_what_the_source_derives(listing, build):
    for name, want in COUNTED.items():
        assert [n for n, _ in listing[build][name]["waits"]] == want, (build, name, listing[build][name])


@pytest.mark.parametrize("t8", [False, True], ids=["no8x8", "8x8"])
@pytest.mark.parametrize("teams", [1, 2])
def test_emulated_handoff_geometries(teams, t8):
    """One and two teams: the bands of a picture follow each other on the same team, or the band below runs beside the
    band above and finds its granules missing at the first look (the emulator runs a wave until it polls in vain)."""
    cfg = synth.config(i4x4=0.4, i8x8=0.3) if t8 else synth.config(i4x4=0.6, i8x8=0.0)
    for W in (1, 2, 3, 4, 130):
        for H in (5, 8, 9):
            for frames in (1, 40) if W < 130 and H == 9 else (1,):   # (40 pictures where the emulator takes under a second)
                fp = abi.make_frame_params(W, H, transform_8x8=t8)
                mbs, co = synth.generate(fp, cfg, 7300 + W, 0, frames)
                st, want = oracle.reconstruct(fp, frames, mbs, co)
                st2, got = emu.reconstruct(fp, frames, mbs, co, teams, 0, 1)
                assert st == 0 and st2 == 0
                assert np.array_equal(got, want), ((W, H, frames), first_mismatch(got, want, W, H))
