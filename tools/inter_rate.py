#!/usr/bin/env python3
"""Rate of the inter prediction kernel on the bench geometry: 300 x 1080p P pictures, each predicted from the reconstructed I
picture of the same index (the bench batch, resident in HBM). Random vectors within +-16 samples; 70 % of the macroblocks carry
one vector (half of those without residual: P_Skip), 15 % one per quadrant, 15 % one per 4x4 block. Kernel time from the
stage's HIP events, macroblocks/s, and the roofline arithmetic of bench.py with 1616 algorithmic bytes per macroblock (80 of
the record + 768 of coefficients + 384 of the reference read once + 384 written). Checks the first picture against the
restatement of the standard in tests/test_inter.py. usage: inter_rate.py [frames] [--out file.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dryv_amd import abi, synth  # noqa: E402
from dryv_amd.frame import InterContext, ReconContext  # noqa: E402

BYTES_PER_MB = 80 + 768 + 384 + 384
DISTINCT = 10   # pictures' worth of records / coefficients generated on the host; the batch repeats them


def p_pictures(per, rng):
    n = DISTINCT * per
    mbs, co = np.zeros(n, dtype=abi.INTER_MB_DTYPE), np.zeros((n, 24, 16), dtype=np.int16)
    kind = rng.random(n)
    mv = rng.integers(-64, 65, size=(n, 16, 2), dtype=np.int16)
    one, quad = kind < 0.70, (kind >= 0.70) & (kind < 0.85)
    mv[one] = mv[one][:, :1]
    mv[quad] = np.repeat(mv[quad][:, ::4], 4, axis=1)
    mbs["mv"], mbs["qp"] = mv, 26
    skip = kind < 0.35
    mbs["flags"][skip] = abi.INTER_NO_RESIDUAL
    # two entries of at most 4 in every run of 16 coefficients: far inside the 16-bit bound of 8.5.12 at qp 26
    coded = np.flatnonzero(~skip)
    for k in range(2):
        pos = rng.integers(0, 16, size=(coded.size, 24))
        co[coded[:, None], np.arange(24)[None, :], pos] = rng.integers(-4, 5, size=(coded.size, 24))
    return mbs, co.reshape(n, 384)


def main():
    import torch
    from test_inter import reference
    frames = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 300
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    fp, imbs, ico, n = synth.workload("C2_1080p_intra_4x4", n_frames=frames)
    per = fp.pic_width_in_mbs * fp.pic_height_in_mbs
    mbs, co = p_pictures(per, np.random.default_rng(12))
    reps = (n + DISTINCT - 1) // DISTINCT
    d_m = torch.from_numpy(mbs.view(np.uint8).reshape(-1, 80)).cuda().repeat(reps, 1)[:n * per].contiguous()
    d_c = torch.from_numpy(co).cuda().repeat(reps, 1)[:n * per].contiguous()
    d_im, d_ic = torch.from_numpy(imbs.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(ico).cuda()
    d_i = torch.zeros(n * per * 384, dtype=torch.uint8, device="cuda")
    d_p = torch.zeros(n * per * 384, dtype=torch.uint8, device="cuda")
    with ReconContext(0) as rctx, InterContext(0, stream=rctx.stream) as ictx:
        rctx.submit_device(fp, n, d_im.data_ptr(), d_ic.data_ptr(), d_i.data_ptr())
        rctx.sync()
        refs = [[d_i.data_ptr() + f * per * 384] for f in range(n)]
        times = []
        for rep in range(12):
            ictx.submit_device(fp, n, refs, d_m.data_ptr(), d_c.data_ptr(), d_p.data_ptr())
            ictx.sync()
            if rep >= 2:
                times.append(ictx.last_kernel_ms())
    ms = float(np.mean(times))
    st, want = reference(fp, 1, [[d_i[:per * 384].cpu().numpy()]], mbs[:per], co[:per])
    ok = bool(st == 0 and np.array_equal(d_p[:per * 384].cpu().numpy(), want))
    mbps = n * per / (ms * 1e-3)
    res = {"frames": n, "kernel_ms_avg": ms, "kernel_ms_min": float(np.min(times)), "macroblocks_per_s": mbps,
           "algorithmic_bytes_per_macroblock": BYTES_PER_MB, "achieved_GBps": mbps * BYTES_PER_MB / 1e9,
           "frac_of_8TBps": mbps * BYTES_PER_MB / 8e12, "first_picture_matches_reference": ok}
    print("inter: %.3f ms per %d frames = %.2f G macroblocks/s = %.0f GB/s algorithmic (%.3f of 8 TB/s); first picture == reference: %s"
          % (ms, n, mbps / 1e9, mbps * BYTES_PER_MB / 1e9, mbps * BYTES_PER_MB / 8e12, ok))
    assert ok
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
