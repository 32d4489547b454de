"""bench.py's plain and --full runs and --dump-outputs: the inputs a run generates (block-wise on host threads) are those
of one synth.generate call, the dump is a fixed choice of the output buffer's 384-byte runs, and on the GPU the dumped
array of the last timed step equals the oracle's reconstruction of the same frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import dryv_amd
from dryv_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
PER_1080P = 120 * 68


@pytest.mark.parametrize("first,frames", [(0, 1), (3, 5), (7, 37)])
def test_threaded_generation_is_the_single_call(first, frames):
    fp = dryv_amd.make_frame_params(6, 5, transform_8x8=True)
    cfg = synth.config(i4x4=0.35, i8x8=0.40)
    mbs, coeffs = bench.generate_shard(fp, cfg, 3, first, frames)
    want_mbs, want_coeffs = synth.generate(fp, cfg, 3, first, frames)
    assert mbs.dtype == want_mbs.dtype and mbs.tobytes() == want_mbs.tobytes()
    assert coeffs.dtype == want_coeffs.dtype and np.array_equal(coeffs, want_coeffs)


def test_dump_rows_are_fixed_and_bounded(tmp_path):
    import torch
    k = bench.DUMP_MAX_VALUES // 384
    assert bench.dump_rows(k) is None                       # up to the bound: the whole buffer
    rows = bench.dump_rows(300 * PER_1080P)                 # the default workload: sampled
    assert len(rows) == k and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 300 * PER_1080P
    assert np.array_equal(rows, bench.dump_rows(300 * PER_1080P))
    assert k * 384 * 4 <= 64 << 20
    # one run more than the bound: sampled, and the file holds exactly the chosen runs as float32
    n = k + 1
    buf = torch.from_numpy((np.arange(n * 384, dtype=np.int64) * 7 % 256).astype(np.uint8))
    bench.dump_outputs(str(tmp_path / "d" / "recon.npy"), buf, n)
    got = np.load(tmp_path / "d" / "recon.npy")
    assert got.dtype == np.float32 and got.shape == (k, 384)
    assert np.array_equal(got, buf.numpy().reshape(n, 384)[bench.dump_rows(n)].astype(np.float32))


def _run_bench(tmp_path, frames, steps, extra):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--frames-per-gpu", str(frames),
                        "--dump-outputs", str(tmp_path)] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["unit"] == "macroblocks/s" and d["higher_is_better"] is True and d["dtype"] == "i32"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(frames * PER_1080P / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert os.listdir(tmp_path) == ["recon.npy"]
    got = np.load(tmp_path / "recon.npy")
    assert got.dtype == np.float32
    # the oracle on the same seeded frames, the rows the dump holds
    import oracle
    cid, w, h, _, t8, kw = synth.WORKLOADS["C2_1080p_intra_4x4"]
    fp = dryv_amd.make_frame_params(w, h, transform_8x8=t8)
    mbs, coeffs = synth.generate(fp, synth.config(**kw), cid, 0, frames)
    st, want = oracle.reconstruct(fp, frames, mbs, coeffs)
    assert st == 0
    want = want.reshape(frames * PER_1080P, 384)
    rows = bench.dump_rows(frames * PER_1080P)
    assert np.array_equal(got, (want if rows is None else want[rows]).astype(np.float32))
    return d, rows


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_a_sample(tmp_path):
    # three 1080p frames have more 384-byte runs than the dump holds: the sampled path
    d, rows = _run_bench(tmp_path, frames=3, steps=3, extra=[])
    assert rows is not None
    assert not {"cpu_baseline", "pipelined", "secondary"} & set(d)
    assert d["config"]["shards_verified_bit_exact"] == 0


@pytest.mark.gpu
def test_full_run_checks_and_measures_the_rest(tmp_path):
    d, rows = _run_bench(tmp_path, frames=2, steps=2, extra=["--full", "--no-secondary", "--cpu-sample-frames", "2"])
    assert rows is None                                     # two frames: the whole buffer
    assert d["config"]["shards_verified_bit_exact"] == 1 and len(d["config"]["shard_checksums"]) == 1
    assert d["cpu_baseline"]["gpu_output_verified_bit_exact"] is True and d["cpu_baseline"]["value"] > 0
    assert d["pipelined"]["outputs_equal_primary_run"] is True and d["pipelined"]["steps"] == 2
