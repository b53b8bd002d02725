"""Device time of self-ensemble inference and of the augmented crop.

    python tools/ensemble_bench.py [--batch 4] [--rounds 20] [--out profiles/ensemble_bench.txt]

Per input size (180x320 and 90x160) and compute mode (f16 and x3), on a default-size generator with random weights, eager launches:
  (a) the plain Generator.forward_u8;
  (b) the self-ensemble composed in torch, what a user could do before: eight forwards of batch N on torch.flip / transpose copies of
      the input, the float outputs brought back with torch.flip / transpose, sequential adds, x 0.125 and the uint8 cast;
  (c) Generator.forward_u8(ensemble=True);
  and the share of (c) spent in the dihedral kernels (ops.PROFILE_DIHEDRAL: device events around each of their launches, taken in
  rounds of their own so that the events do not sit inside the timed intervals of (c)).
Then one augmented batch (fsr_crop_resize_aug, random codes) against a plain one (fsr_crop_resize) at 96 -> 384, batch 32.
The candidates are INTERLEAVED: every round times each of them once, in turn, so clock and thermal drift fall on all of them alike; the
figure is the median over the rounds, the spread the 10th to 90th percentile.  Nothing is gated on it."""
import argparse
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("fast-srgan_amd")
ops = importlib.import_module("fast-srgan_amd.ops")
dataloader = importlib.import_module("fast-srgan_amd.dataloader")


def D(x, k):
    """D_k of an (N,3,H,W) tensor with torch index operations."""
    if k & 1:
        x = x.flip(3)
    if k & 2:
        x = x.flip(2)
    if k & 4:
        x = x.transpose(2, 3)
    return x


def torch_ensemble(G, frames):
    x = ops.u8_to_image(frames)
    s = None
    for k in range(8):
        y = D(G.forward(D(x, k).contiguous()), ops.DIHEDRAL_INVERSE[k])
        s = y if s is None else s + y
    return (((s * 0.125 + 1.0) / 2.0).clamp(0.0, 1.0) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def timed(cands, rounds, inner):
    for _, fn in cands:                                # warm-up: code objects, filter packs, allocator
        for _ in range(2):
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
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3, help="calls per timed interval")
    ap.add_argument("--sizes", default="180x320,90x160")
    ap.add_argument("--dtypes", default="f16,x3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    n = a.batch
    lines = ["# tools/ensemble_bench.py --batch %d --rounds %d --inner %d on %s" % (n, a.rounds, a.inner, torch.cuda.get_device_name(0)),
             "# us per call, eager launches: median over the rounds [p10 .. p90]; candidates interleaved round by round",
             "# (a) forward_u8   (b) torch composition: 8 forwards of batch N, flips, adds, cast   (c) forward_u8(ensemble=True)",
             "%-9s %-5s %-32s %10s %23s" % ("size", "dtype", "candidate", "us", "[p10 .. p90]")]
    rs = np.random.RandomState(0)
    with torch.no_grad():
        for size in a.sizes.split(","):
            h, w = (int(v) for v in size.split("x"))
            frames = torch.from_numpy(rs.randint(0, 256, size=(n, h, w, 3), dtype=np.uint8)).to(dev)
            for cdn in a.dtypes.split(","):
                torch.manual_seed(0)
                G = pkg.Generator(types.SimpleNamespace(n_filters=64, n_layers=8, n_upsample=2), compute_dtype=cdn).to(dev).eval()
                cands = [("(a) forward_u8", lambda: G.forward_u8(frames)),
                         ("(b) torch composition", lambda: torch_ensemble(G, frames)),
                         ("(c) forward_u8(ensemble=True)", lambda: G.forward_u8(frames, ensemble=True))]
                times = timed(cands, a.rounds, a.inner)
                for (name, _), t in zip(cands, times):
                    lines.append("%-9s %-5s %-32s %10.1f [%9.1f .. %9.1f]" % (size, cdn, name, np.median(t), np.percentile(t, 10), np.percentile(t, 90)))
                med = [float(np.median(t)) for t in times]
                lines.append("%-9s %-5s %-32s %10.3f" % (size, cdn, "(c) / (b)", med[2] / med[1]))
                lines.append("%-9s %-5s %-32s %10.3f" % (size, cdn, "(c) / (a)", med[2] / med[0]))
                # the dihedral kernels inside (c): device events around their launches, in rounds of their own
                kern = {"members": [], "accumulate": []}
                for _ in range(a.rounds):
                    ops.PROFILE_DIHEDRAL = []
                    G.forward_u8(frames, ensemble=True)
                    torch.cuda.synchronize()
                    got = {"members": 0.0, "accumulate": 0.0}
                    for what, e0, e1 in ops.PROFILE_DIHEDRAL:
                        got[what] += e0.elapsed_time(e1) * 1e3
                    ops.PROFILE_DIHEDRAL = None
                    for what in kern:
                        kern[what].append(got[what])
                mem, acc = float(np.median(kern["members"])), float(np.median(kern["accumulate"]))
                lines.append("%-9s %-5s %-32s %10.1f" % (size, cdn, "  member input, 2 launches", mem))
                lines.append("%-9s %-5s %-32s %10.1f" % (size, cdn, "  accumulate, 2 launches", acc))
                lines.append("%-9s %-5s %-32s %10.4f" % (size, cdn, "  share of (c) in these kernels", (mem + acc) / med[2]))
                del G
        # the augmented crop against the plain one
        l, bs = 96, 32
        hr = 4 * l
        with tempfile.TemporaryDirectory() as tmp:
            np.save(os.path.join(tmp, "img.npy"), rs.randint(0, 256, size=(3, hr + 64, hr + 64), dtype=np.uint8))
            ds = dataloader.NumpyImagesDataset([os.path.join(tmp, "img.npy")], l, 4, device=dev)
            ds[0]                                      # uploads the image; the file is not read again
        idx, crops = [0] * bs, [(int(y), int(x)) for y, x in rs.randint(0, 65, size=(bs, 2))]
        codes = [int(k) for k in rs.randint(0, 8, size=bs)]
        cands = [("plain batch (fsr_crop_resize)", lambda: ds.batch(idx, crops)),
                 ("augmented, random codes", lambda: ds.batch(idx, crops, xforms=codes)),
                 ("augmented, all code 0", lambda: ds.batch(idx, crops, xforms=[0] * bs)),
                 ("augmented, all code 5", lambda: ds.batch(idx, crops, xforms=[5] * bs))]
        times = timed(cands, a.rounds, 10)
        lines.append("# crop + down-scale %d -> %d, batch %d: us per batch (host descriptor copy and two launches)" % (hr, l, bs))
        for (name, _), t in zip(cands, times):
            lines.append("%-9s %-5s %-32s %10.1f [%9.1f .. %9.1f]" % ("%d->%d" % (l, hr), "-", name, np.median(t), np.percentile(t, 10), np.percentile(t, 90)))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
