#!/usr/bin/env python3
"""Rate of the inter prediction kernel on the bench geometry: 300 x 1080p P pictures, each predicted from the reconstructed I
picture of the same index (the bench batch, resident in HBM). Random vectors within +-16 samples; 70 % of the macroblocks carry
one vector (half of those without residual: P_Skip), 15 % one per quadrant, 15 % one per 4x4 block. Kernel time from the
stage's HIP events, macroblocks/s, and the roofline arithmetic of bench.py with 1616 algorithmic bytes per macroblock (80 of
the record + 768 of coefficients + 384 of the reference read once + 384 written). Checks the first picture against the
restatement of the standard in oracle/inter_model.py (predict_p). usage: inter_rate.py [frames] [--out file.json]

--bipred: after the P run, in the same process, the same number of B pictures through dryv_inter_submit_device_bipred: list 0 is
picture f's I picture, list 1 picture f + 1's; both lists' vectors have the P run's statistics; every quadrant draws L0 / L1 /
both with a third each; default weights. Records both kernel times and their ratio (expected: below 2, since residual and
output are shared) and checks the top of the first B picture against oracle.inter_model.predict_b. Default --out:
profiles/inter_rate_bipred.json.

--deblock: after the P run, in the same process, dryv_inter_deblock_device on that P batch: the device times of the boundary-
strength kernel and of the band filter separately (the stage's events), then the intra deblocking stage on the reconstructed I
pictures (what tools/deblock_rate.py measures), for comparison. Checks the top macroblock rows of the first filtered P picture and
its bS records against oracle.inter_model's bs_reference and deblock_reference. Default --out: profiles/inter_deblock_rate.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dryv_amd import abi, synth  # noqa: E402
from dryv_amd.frame import InterContext, ReconContext  # noqa: E402
from oracle import inter_model  # noqa: E402

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


def b_pictures(per, mbs, rng):
    """The P records widened: list 1's vectors drawn like list 0's, every quadrant on L0 / L1 / both."""
    other, _ = p_pictures(per, rng)
    b = np.zeros(len(mbs), dtype=abi.INTER_BMB_DTYPE)
    b["qp"], b["flags"] = mbs["qp"], mbs["flags"]
    b["mv"][:, 0], b["mv"][:, 1] = mbs["mv"], other["mv"]
    use = rng.integers(0, 3, size=(len(mbs), 4))   # 0 L0, 1 L1, 2 both
    b["ref_idx"][:, 0][use == 1] = -1
    b["ref_idx"][:, 1][use == 0] = -1
    return b


def timed(ictx, submit):
    times = []
    for rep in range(12):
        submit()
        ictx.sync()
        if rep >= 2:
            times.append(ictx.last_kernel_ms())
    return times


def main():
    import torch
    frames = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 300
    bipred, deblock = "--bipred" in sys.argv, "--deblock" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else (
        os.path.join(ROOT, "profiles", "inter_rate_bipred.json") if bipred else
        os.path.join(ROOT, "profiles", "inter_deblock_rate.json") if deblock else None)
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
        times = timed(ictx, lambda: ictx.submit_device(fp, n, refs, d_m.data_ptr(), d_c.data_ptr(), d_p.data_ptr()))
        if bipred:
            bmbs = b_pictures(per, mbs, np.random.default_rng(13))
            d_bm = torch.from_numpy(bmbs.view(np.uint8).reshape(-1, 144)).cuda().repeat(reps, 1)[:n * per].contiguous()
            d_b = torch.zeros(n * per * 384, dtype=torch.uint8, device="cuda")
            refs1 = [[d_i.data_ptr() + ((f + 1) % n) * per * 384] for f in range(n)]
            btimes = timed(ictx, lambda: ictx.submit_device_bipred(fp, n, refs, refs1, None, d_bm.data_ptr(), d_c.data_ptr(), d_b.data_ptr()))
        if deblock:
            dp = abi.make_deblock_params(0, 0, 0)
            unfiltered, d_bs = d_p.clone(), torch.zeros(n * per * 16, dtype=torch.uint8, device="cuda")
            dtimes = []
            for rep in range(12):
                d_p.copy_(unfiltered)
                torch.cuda.synchronize()
                ictx.deblock_device(fp, dp, n, False, refs, None, d_m.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), d_bs.data_ptr())
                ictx.sync()
                if rep >= 2:
                    dtimes.append(ictx.last_deblock_ms())
            filtered, d_p = d_p, unfiltered
            itimes = []
            for rep in range(12):
                d_f = d_i.clone()
                torch.cuda.synchronize()
                rctx.deblock_device(fp, dp, n, d_im.data_ptr(), d_f.data_ptr())
                rctx.sync()
                if rep >= 2:
                    itimes.append(rctx.last_kernel_ms())
    ms = float(np.mean(times))
    st, want = inter_model.predict_p(fp, 1, [[d_i[:per * 384].cpu().numpy()]], mbs[:per], co[:per])
    ok = bool(st == 0 and np.array_equal(d_p[:per * 384].cpu().numpy(), want))
    mbps = n * per / (ms * 1e-3)
    res = {"frames": n, "kernel_ms_avg": ms, "kernel_ms_min": float(np.min(times)), "macroblocks_per_s": mbps,
           "algorithmic_bytes_per_macroblock": BYTES_PER_MB, "achieved_GBps": mbps * BYTES_PER_MB / 1e9,
           "frac_of_8TBps": mbps * BYTES_PER_MB / 8e12, "first_picture_matches_reference": ok}
    print("inter: %.3f ms per %d frames = %.2f G macroblocks/s = %.0f GB/s algorithmic (%.3f of 8 TB/s); first picture == reference: %s"
          % (ms, n, mbps / 1e9, mbps * BYTES_PER_MB / 1e9, mbps * BYTES_PER_MB / 8e12, ok))
    assert ok
    if bipred:
        # (the reference is three passes of Python ints: the top eight macroblock rows as a picture of their own, compared on the
        # top six, which no vector of +-16 samples takes below the eighth)
        W, H = fp.pic_width_in_mbs, fp.pic_height_in_mbs
        R, keep = min(8, H), min(8, H) - (2 if H > 8 else 0)
        top = lambda pic, tot, rows: np.concatenate([pic[:256 * W * rows], pic[256 * W * tot:256 * W * tot + 64 * W * rows],
                                                     pic[320 * W * tot:320 * W * tot + 64 * W * rows]])
        fpc = abi.FrameParams.from_buffer_copy(fp)
        fpc.pic_height_in_mbs = R
        pics = [[top(d_i[f * per * 384:(f + 1) * per * 384].cpu().numpy(), H, R)] for f in (0, 1 % n)]
        st, want = inter_model.predict_b(fpc, 1, pics[:1], pics[1:], None, bmbs[:W * R], co[:W * R])
        bok = bool(st == 0 and np.array_equal(top(d_b[:per * 384].cpu().numpy(), H, keep), top(want, R, keep)))
        bms = float(np.mean(btimes))
        res = {"frames": n, "p": res, "bipred": {"kernel_ms_avg": bms, "kernel_ms_min": float(np.min(btimes)),
                                                 "macroblocks_per_s": n * per / (bms * 1e-3), "first_picture_matches_reference": bok},
               "bipred_over_p": bms / ms, "expected": "below 2: residual and output are shared", "expectation_held": bool(bms / ms < 2)}
        print("bipred: %.3f ms per %d frames = %.2f x the P batch of this session (expected below 2); first picture == reference: %s"
              % (bms, n, bms / ms, bok))
        assert bok
    if deblock:
        # (the top three macroblock rows as a picture of their own, compared on the top two: no filtered sample of those depends
        # on the third row's bottom edge)
        W, H, R = fp.pic_width_in_mbs, fp.pic_height_in_mbs, 3
        top = lambda pic, rows: np.concatenate([pic[:256 * W * rows], pic[256 * W * H:256 * W * H + 64 * W * rows],
                                                pic[320 * W * H:320 * W * H + 64 * W * rows]])
        fpc = abi.FrameParams.from_buffer_copy(fp)
        fpc.pic_height_in_mbs = R
        bs = inter_model.bs_reference(W, R, mbs[:W * R], co[:W * R], ([[0]], [[]]))
        want = inter_model.deblock_reference(fpc, dp, 1, mbs[:W * R], top(d_p[:per * 384].cpu().numpy(), R), bs)
        cut = lambda pic: np.concatenate([pic[:256 * W * 2], pic[256 * W * R:256 * W * R + 64 * W * 2], pic[320 * W * R:320 * W * R + 64 * W * 2]])
        dok = bool(np.array_equal(cut(top(filtered[:per * 384].cpu().numpy(), R)), cut(want)) and
                   np.array_equal(d_bs[:W * 2 * 16].cpu().numpy().view(np.uint16).reshape(-1, 2, 4), inter_model.words(bs)[:W * 2]))
        a_ms, b_ms, i_ms = float(np.mean([t[0] for t in dtimes])), float(np.mean([t[1] for t in dtimes])), float(np.mean(itimes))
        hist = np.bincount((d_bs.cpu().numpy()[:, None] >> np.array([0, 4]) & 15).reshape(-1), minlength=5)
        res = {"frames": n, "p": res, "deblock": {
            "bs_kernel_ms_avg": a_ms, "bs_kernel_ms_min": float(np.min([t[0] for t in dtimes])),
            "filter_kernel_ms_avg": b_ms, "filter_kernel_ms_min": float(np.min([t[1] for t in dtimes])),
            "bs_share_of_segments": {str(k): float(v) / hist.sum() for k, v in enumerate(hist)},
            "first_picture_matches_restatement": dok},
            "intra_deblock": {"kernel_ms_avg": i_ms, "kernel_ms_min": float(np.min(itimes))},
            "filter_over_intra": b_ms / i_ms, "expected": "near 1: the same picture bytes plus 16 bytes per macroblock"}
        print("deblock of the P batch: bS kernel %.3f ms, filter %.3f ms; intra deblocking of the I batch %.3f ms: filter / intra = %.2f; "
              "first picture == restatement: %s" % (a_ms, b_ms, i_ms, b_ms / i_ms, dok))
        assert dok
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
