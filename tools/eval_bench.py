"""Device time of ops.quality_u8 next to the composition the kernels before it allowed, and of a whole Evaluator.run.

    python tools/eval_bench.py [--rounds 30] [--inner 10] [--out profiles/eval_bench.txt]

Per image size (2040 x 1356, a DIV2K picture; 480 x 320, a BSD100 one) and channel:
  * fused     : ops.quality_u8 on the uint8 frames, shave 4 -- one launch plus the fixed-order reduction;
  * composed  : torch elementwise ops that build float planes in [-1, 1] from the same bytes (luma: 16 + the weighted sum, over 127.5,
                minus 1; shaved views), then ops.ssim_sse -- which takes three channels, so the luma plane is handed in three times
                through a zero channel stride.
The candidates are INTERLEAVED round by round; the figure is the median over the rounds, the spread the 10th to 90th percentile.
Then Evaluator.run (host wall time, synchronised) over synthetic images with a default-size generator of random weights, and the share
of it that the metric launches take.  Nothing is gated on these figures."""
import argparse
import importlib
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("fast-srgan_amd")
ops = importlib.import_module("fast-srgan_amd.ops")
evaluate = importlib.import_module("fast-srgan_amd.evaluate")

Y_COEF = (65.481 / 255.0, 128.553 / 255.0, 24.966 / 255.0)


def composed(a, b, shave, channel):
    h, w = a.shape[1:3]
    planes = []
    for t in (a, b):
        x = t[:, shave:h - shave, shave:w - shave].float()
        if channel == "y":
            y = 16.0 + (Y_COEF[0] * x[..., 0] + Y_COEF[1] * x[..., 1] + Y_COEF[2] * x[..., 2])
            planes.append((y / 127.5 - 1.0)[:, None].expand(-1, 3, -1, -1))
        else:
            planes.append((x / 127.5 - 1.0).permute(0, 3, 1, 2))
    return ops.ssim_sse(planes[0], planes[1])


def timed(cands, rounds, inner):
    for _, fn in cands:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in cands]
    for _ in range(rounds):
        for k, (_, fn) in enumerate(cands):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / inner)
    return times


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed interval")
    ap.add_argument("--images", type=int, default=8, help="synthetic images of the Evaluator.run part")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    lines = ["# tools/eval_bench.py --rounds %d --inner %d on %s" % (a.rounds, a.inner, torch.cuda.get_device_name(0)),
             "# us per call: median over the rounds [p10 .. p90]; candidates interleaved round by round; n = 1, shave 4",
             "%-12s %-4s %-9s %10s %21s" % ("size", "ch", "path", "us", "[p10 .. p90]")]
    shave = 4
    for w, h in ((2040, 1356), (480, 320)):
        hr = torch.from_numpy(rs.randint(0, 256, size=(1, h, w, 3), dtype=np.uint8)).to(dev)
        sr = (hr.int() + torch.from_numpy(rs.randint(-6, 7, size=(1, h, w, 3))).to(dev)).clamp(0, 255).to(torch.uint8)
        for channel in ("y", "rgb"):
            want, got = composed(sr, hr, shave, channel).double().cpu(), ops.quality_u8(sr, hr, shave, channel).double().cpu()
            c = 1 if channel == "y" else 3
            # same metric: ssim_sse's sums are over 3 planes of data range 1
            ssim_rel = abs(float(got[0, 0]) / c - float(want[0, 0]) / 3) / (float(want[0, 0]) / 3)
            sse_rel = abs(float(got[0, 1]) / c - float(want[0, 1]) * 255.0 ** 2 / 3) / (float(got[0, 1]) / c)
            assert ssim_rel < 1e-4 and sse_rel < 1e-4, (channel, ssim_rel, sse_rel)
            cands = [("fused", lambda ch=channel: ops.quality_u8(sr, hr, shave, ch)), ("composed", lambda ch=channel: composed(sr, hr, shave, ch))]
            for (name, _), t in zip(cands, timed(cands, a.rounds, a.inner)):
                lines.append("%-12s %-4s %-9s %10.2f [%8.2f .. %8.2f]" % ("%dx%d" % (w, h), channel, name, np.median(t), np.percentile(t, 10), np.percentile(t, 90)))
    # a whole evaluation: a default-size generator (random weights), synthetic HR images, LR made on the device
    torch.manual_seed(0)
    G = pkg.Generator(types.SimpleNamespace(n_filters=64, n_layers=8, n_upsample=2)).to(dev).eval()
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i in range(a.images):
            paths.append(os.path.join(tmp, "img%02d.npy" % i))
            np.save(paths[-1], rs.randint(0, 256, size=(3, 320, 480), dtype=np.uint8))
        t0 = time.perf_counter()
        ev = evaluate.Evaluator(paths, 4, device=dev, batch=8)
        torch.cuda.synchronize()
        t_build = time.perf_counter() - t0
    ev.run(G)                                              # warm-up: code objects, allocator, filter packs
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):
        t0 = time.perf_counter()
        res = ev.run(G)
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    b = ev.buckets[0]
    sr = G.forward_u8(b.lr)
    q = timed([("q", lambda: ops.quality_u8(sr, b.hr, ev.shave, ev.channel))], a.rounds, a.inner)[0]
    lines += ["# Evaluator over %d synthetic 480x320 images, generator 64 filters x 8 blocks (%s), batch 8, channel y, shave 4" % (a.images, G.compute.name),
              "evaluator build (read, upload, device LR)   %9.2f ms" % (t_build * 1e3),
              "Evaluator.run, median of 5                  %9.2f ms   (mean PSNR %.3f dB, SSIM %.5f)" % (np.median(runs) * 1e3, res["psnr"], res["ssim"]),
              "  of which quality_u8, one launch of %d     %9.3f ms" % (a.images, np.median(q) / 1e3)]
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
