"""Device time of the training degradations next to the crop + down-scale pair they follow.

    python tools/degrade_bench.py [--batch 32] [--sizes 96,128] [--rounds 30] [--out profiles/degrade_bench.txt]

Per LR size l (HR = 4 l): the fsr_crop_resize pair, blur, noise only, blur + noise, and the JPEG round trip at 4:2:0 and 4:4:4, each
from its own device events.  The candidates are INTERLEAVED: every round times each of them once, in turn, so clock and thermal drift
fall on all of them alike; the figure is the median over the rounds, the spread the 10th to 90th percentile.  Nothing is gated on it."""
import argparse
import importlib
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = importlib.import_module("fast-srgan_amd._lib")
ops = importlib.import_module("fast-srgan_amd.ops")
dataloader = importlib.import_module("fast-srgan_amd.dataloader")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--sizes", default="96,128")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10, help="launches per timed interval")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "degrade_bench.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    n = a.batch
    lines = ["# tools/degrade_bench.py --batch %d --sizes %s --rounds %d --inner %d on %s" % (n, a.sizes, a.rounds, a.inner, torch.cuda.get_device_name(0)),
             "# us per call: median over the rounds [p10 .. p90]; candidates interleaved round by round; MB = bytes read + written by the stage",
             "%-6s %-22s %8s %9s %19s %8s" % ("l", "stage", "launches", "us", "[p10 .. p90]", "MB")]
    rs = np.random.RandomState(0)
    for l in (int(v) for v in a.sizes.split(",")):
        hr = 4 * l
        with tempfile.TemporaryDirectory() as tmp:
            np.save(os.path.join(tmp, "img.npy"), rs.randint(0, 256, size=(3, hr + 64, hr + 64), dtype=np.uint8))
            ds = dataloader.NumpyImagesDataset([os.path.join(tmp, "img.npy")], l, 4, device=dev)
            ds[0]                                      # uploads the image; the file is not read again
        idx, crops = [0] * n, [(int(y), int(x)) for y, x in rs.randint(0, 65, size=(n, 2))]
        lr, _ = ds.batch(idx, crops)
        words = ops.upload_words(ops.degrade_words(n, [float(v) for v in rs.uniform(0.2, 2.0, size=n)], [float(v) for v in rs.uniform(1, 10, size=n)],
                                                   [(int(p), int(q)) for p, q in rs.randint(0, 2 ** 32, size=(n, 2), dtype=np.int64)],
                                                   [int(v) for v in rs.randint(30, 96, size=n)]), dev)
        mb_lr = lr.numel() * 4 / 1e6
        cands = [("crop_resize pair", 2, lambda: ds.batch(idx, crops), n * 3 * hr * hr / 1e6 + 4 * n * 3 * hr * (hr + 2 * l) / 1e6 + mb_lr),
                 ("blur", 2, lambda: ops.degrade_blur_noise_dev(lr, words, True, False), 4 * mb_lr),
                 ("noise only", 1, lambda: ops.degrade_blur_noise_dev(lr, words, False, True), 2 * mb_lr),
                 ("blur + noise", 2, lambda: ops.degrade_blur_noise_dev(lr, words, True, True), 4 * mb_lr),
                 ("jpeg 4:2:0", 1, lambda: ops.jpeg_roundtrip_dev(lr, words, "420"), 2 * mb_lr),
                 ("jpeg 4:4:4", 1, lambda: ops.jpeg_roundtrip_dev(lr, words, "444"), 2 * mb_lr)]
        for _, _, fn, _ in cands:                      # warm-up: code objects, allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in cands]
        for _ in range(a.rounds):
            for k, (_, _, fn, _) in enumerate(cands):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.inner)
        for (name, launches, _, mb), t in zip(cands, times):
            lines.append("%-6d %-22s %8d %9.2f [%7.2f .. %7.2f] %8.2f" % (l, name, launches, np.median(t), np.percentile(t, 10), np.percentile(t, 90), mb))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
