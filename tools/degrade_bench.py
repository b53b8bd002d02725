"""Device time of the training degradations next to the crop + down-scale pair they follow.

    python tools/degrade_bench.py [--batch 32] [--sizes 96,128] [--rounds 30] [--out profiles/degrade_bench.txt]

Per LR size l (HR = 4 l): the fsr_crop_resize pair, blur, noise only, blur + noise, and the JPEG round trip at 4:2:0 and 4:4:4, each
from its own device events.  The candidates are INTERLEAVED: every round times each of them once, in turn, so clock and thermal drift
fall on all of them alike; the figure is the median over the rounds, the spread the 10th to 90th percentile.  Nothing is gated on it.

    python tools/degrade_bench.py --high-order [--out profiles/degrade_bench_ho.txt]

adds the stages of the high-order model in the same form: fsr_filter2d on the HR batch at K = 7, 13, 21 and on the LR
batch at K = 21, each next to the same filter composed in torch (replicate pad + grouped F.conv2d with per-sample kernels: the yardstick,
which exists in this tool only) and with its two floors -- 2 K^2 flops per element at 157.3 TFLOP/s of fp32 vector rate, and the bytes
read and written at 8 TB/s --, the fsr_resize_select pair, the noise forms, and the whole loader batch, first-order against high-order."""
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


def _time(cands, rounds, inner):
    """[[us per call] per candidate]: every round times each candidate once, in turn."""
    for fn in cands:                                   # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in cands]
    for _ in range(rounds):
        for k, fn in enumerate(cands):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / inner)
    return times


def _torch_filter2d(x, kernels):
    """The yardstick: replicate pad + grouped conv2d (cross-correlation, like fsr_filter2d) with one K x K kernel per sample."""
    n, c, h, w = x.shape
    k = kernels.shape[-1]
    wt = kernels[:, None, None].expand(n, c, 1, k, k).reshape(n * c, 1, k, k)
    xp = torch.nn.functional.pad(x.reshape(1, n * c, h, w), (k // 2,) * 4, mode="replicate")
    return torch.nn.functional.conv2d(xp, wt, groups=n * c).reshape(n, c, h, w)


def high_order(a):
    kb = importlib.import_module("fast-srgan_amd.kernel_bank")
    dev = torch.device("cuda:0")
    n = a.batch
    rs = np.random.RandomState(0)
    lines = ["# tools/degrade_bench.py --high-order --batch %d --sizes %s --rounds %d --inner %d on %s" % (n, a.sizes, a.rounds, a.inner, torch.cuda.get_device_name(0)),
             "# us per call: median over the rounds [p10 .. p90]; candidates interleaved round by round; floors: 2 K^2 flops per element at 157.3 TFLOP/s,",
             "# bytes read + written at 8 TB/s; `torch` = replicate pad + grouped conv2d with per-sample kernels (the yardstick)",
             "%-6s %-30s %8s %9s %19s %9s %9s" % ("l", "stage", "launches", "us", "[p10 .. p90]", "flop us", "byte us")]
    for l in (int(v) for v in a.sizes.split(",")):
        hr = 4 * l
        with tempfile.TemporaryDirectory() as tmp:
            np.save(os.path.join(tmp, "img.npy"), rs.randint(0, 256, size=(3, hr + 64, hr + 64), dtype=np.uint8))
            ds = dataloader.NumpyImagesDataset([os.path.join(tmp, "img.npy")], l, 4, device=dev)
            ds[0]
        idx, crops = [0] * n, [(int(y), int(x)) for y, x in rs.randint(0, 65, size=(n, 2))]
        lr_x, hr_x = ds.batch(idx, crops)
        rows = []                                      # (name, launches, fn, flops, bytes)
        for x, where, sizes in ((hr_x, "HR", (7, 13, 21)), (lr_x, "LR", (21,))):
            for k in sizes:
                ks = [kb.bank_kernel("aniso", k, float(sx), float(sy), float(th)) for sx, sy, th in
                      zip(rs.uniform(0.5, 3.0, size=n), rs.uniform(0.5, 3.0, size=n), rs.uniform(-3.1, 3.1, size=n))]
                words = ops.upload_words(ops.filter2d_words(n, ks), dev)
                kt = torch.from_numpy(np.stack(ks)).to(dev)
                err = float((ops.filter2d_dev(x, words) - _torch_filter2d(x, kt)).abs().max())
                assert err < 1e-4, err                 # both compute the same filter
                flops, nbytes = 2.0 * k * k * x.numel(), 8.0 * x.numel()
                rows.append(("filter2d %s K=%d" % (where, k), 1, lambda x=x, words=words: ops.filter2d_dev(x, words), flops, nbytes))
                rows.append(("  torch pad + grouped conv2d", 2, lambda x=x, kt=kt: _torch_filter2d(x, kt), flops, nbytes))
        tables = ds.resize_tables()
        sel = ops.upload_words(rs.randint(0, 3, size=n).astype(np.int32), dev)
        rows.append(("resize_select pair", 2, lambda: ops.resize_select_dev(hr_x, tables, sel), 0.0, 4.0 * (hr_x.numel() + 2 * n * 3 * hr * l + lr_x.numel())))
        seeds = [(int(p), int(q)) for p, q in rs.randint(0, 2 ** 32, size=(n, 2), dtype=np.int64)]
        for name, st, fl in (("noise kinds: gaussian", rs.uniform(1, 10, size=n), 0), ("noise kinds: shot", rs.uniform(0.05, 1.5, size=n), L.NOISE_SHOT),
                             ("noise kinds: shot + grey", rs.uniform(0.05, 1.5, size=n), L.NOISE_SHOT | L.NOISE_GREY)):
            w = ops.upload_words(ops.noise_kind_words(n, [float(v) for v in st], [fl] * n, seeds), dev)
            rows.append((name, 1, lambda w=w: ops.degrade_noise_kinds_dev(lr_x, w), 0.0, 8.0 * lr_x.numel()))
        first = dict(blur_sigma=(0.2, 2.0), blur_prob=0.5, noise_sigma=(1, 10), noise_prob=0.5, jpeg_quality=(30, 95), jpeg_prob=0.7)
        full = dict(first, kernel_prob=1.0, sinc_prob=0.1, resize_filters=(1, 1, 1), noise_shot_prob=0.4, noise_grey_prob=0.4, final_sinc_prob=0.8,
                    second=dict(kernel_prob=0.8, sinc_prob=0.1, noise_prob=0.5, noise_shot_prob=0.4, noise_grey_prob=0.4, jpeg_prob=0.7))
        d1, d2 = dataloader.Degradation(seed=1, **first), dataloader.Degradation(seed=1, **full)
        p1, p2 = d1.draw(n), d2.draw(n)
        rows.append(("crop_resize pair", 2, lambda: ds.batch(idx, crops), 0.0, 0.0))
        rows.append(("loader batch, first-order", 5, lambda: ds.batch(idx, crops, (d1, p1)), 0.0, 0.0))
        rows.append(("loader batch, high-order", 14, lambda: ds.batch(idx, crops, (d2, p2)), 0.0, 0.0))
        times = _time([r[2] for r in rows], a.rounds, a.inner)
        for (name, launches, _, flops, nbytes), t in zip(rows, times):
            lines.append("%-6d %-30s %8d %9.2f [%7.2f .. %7.2f] %9s %9s" % (
                l, name, launches, np.median(t), np.percentile(t, 10), np.percentile(t, 90),
                "%.2f" % (flops / 157.3e12 * 1e6) if flops else "-", "%.2f" % (nbytes / 8e12 * 1e6) if nbytes else "-"))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    out = a.out if a.out else os.path.join(ROOT, "profiles", "degrade_bench_ho.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--high-order", action="store_true", help="the stages of DESIGN.md 6l; writes profiles/degrade_bench_ho.txt")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--sizes", default="96,128")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10, help="launches per timed interval")
    ap.add_argument("--out", default=None, help="default: profiles/degrade_bench.txt, or profiles/degrade_bench_ho.txt with --high-order")
    a = ap.parse_args(argv)
    if a.high_order:
        return high_order(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "degrade_bench.txt")
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
        times = _time([fn for _, _, fn, _ in cands], a.rounds, a.inner)
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
