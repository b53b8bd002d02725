"""What a degradation setting does to a picture, through the operators the training loader uses.

    python tools/degrade.py --image in.png --output out.png [--blur S] [--noise S] [--jpeg Q] [--subsampling 420|444] [--seed N]
                            [--kernel KIND:K:SX[:SY:THETA[:BETA]]] [--sinc OMEGA:K] [--filter bicubic|bilinear|area --scale S]
                            [--shot G] [--grey] [--second "--kernel ... --sinc ... --noise S --shot G --grey --jpeg Q --sinc-first"]

--blur: Gaussian sigma in pixels (<= 3); --noise: sigma in 8-bit code units (<= 25); --jpeg: quality 1..100.  The order is the loader's:
blur, noise, JPEG.  A stage that is not named is not run; with none the picture is copied.

The high-order stages, in the loader's order around those: --kernel, a blur kernel of the bank (KIND: iso, aniso,
generalized_iso, generalized_aniso, plateau_iso, plateau_aniso; odd size K <= 21; sigmas in pixels, THETA in radians) or --sinc, a
circular low-pass of cut-off OMEGA <= pi, on the picture as it comes; --filter with --scale S, the down-scale by S through that filter;
then blur, noise, JPEG -- with --shot G the noise is shot noise of gain G (<= 3) in place of --noise, with --grey one field for the three
channels; then the round of --second: its kernel, its noise, its JPEG, and its --sinc behind that JPEG (--sinc-first: in front of it)."""
import argparse
import importlib
import os
import random
import shlex
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def seed_words(seed):
    """The two 32-bit words that name the noise field of --seed N."""
    rng = random.Random(seed)
    return rng.getrandbits(32), rng.getrandbits(32)


def parse_kernel(text):
    """KIND:K:SX[:SY:THETA[:BETA]] -> the float32 kernel of the bank."""
    kb = importlib.import_module("fast-srgan_amd.kernel_bank")
    f = text.split(":")
    if not 3 <= len(f) <= 6 or len(f) == 4:
        raise SystemExit("--kernel takes KIND:K:SX[:SY:THETA[:BETA]], got %r" % text)
    sx = float(f[2])
    sy, theta = (float(f[3]), float(f[4])) if len(f) >= 5 else (sx, 0.0)
    return kb.bank_kernel(f[0], int(f[1]), sx, sy, theta, float(f[5]) if len(f) == 6 else 1.0)


def parse_sinc(text):
    """OMEGA:K -> the float32 sinc kernel."""
    kb = importlib.import_module("fast-srgan_amd.kernel_bank")
    f = text.split(":")
    if len(f) != 2:
        raise SystemExit("--sinc takes OMEGA:K, got %r" % text)
    return kb.sinc_kernel(float(f[0]), int(f[1]))


def _noise(ops, L, x, a, seed):
    """--noise / --shot / --grey of one round."""
    if not (a.noise or a.shot):
        return x
    if not (a.shot or a.grey):
        return ops.degrade_blur_noise(x, None, [a.noise], [seed])
    return ops.degrade_noise_kinds(x, [a.shot or a.noise], [(L.NOISE_SHOT if a.shot else 0) | (L.NOISE_GREY if a.grey else 0)], [seed])


def _second_parser():
    sp = argparse.ArgumentParser(prog="--second", add_help=False)
    sp.add_argument("--kernel")
    sp.add_argument("--sinc")
    sp.add_argument("--sinc-first", action="store_true")
    sp.add_argument("--noise", type=float, default=0.0)
    sp.add_argument("--shot", type=float, default=0.0)
    sp.add_argument("--grey", action="store_true")
    sp.add_argument("--jpeg", type=int, default=0)
    return sp


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--kernel", help="KIND:K:SX[:SY:THETA[:BETA]]: a blur kernel of the bank, applied first")
    ap.add_argument("--sinc", help="OMEGA:K: a sinc kernel in place of --kernel")
    ap.add_argument("--filter", choices=("bicubic", "bilinear", "area"), help="down-scale by --scale through this filter")
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--shot", type=float, default=0.0, help="shot noise of this gain (normal approximation) in place of --noise")
    ap.add_argument("--grey", action="store_true", help="one noise field for the three channels")
    ap.add_argument("--second", help="the second round's own flags, as one quoted string")
    ap.add_argument("--image", required=True)
    ap.add_argument("--output", required=True)
    ap.add_argument("--blur", type=float, default=0.0)
    ap.add_argument("--noise", type=float, default=0.0)
    ap.add_argument("--jpeg", type=int, default=0)
    ap.add_argument("--subsampling", choices=("420", "444"), default="420")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    from PIL import Image
    L = importlib.import_module("fast-srgan_amd._lib")
    ops = importlib.import_module("fast-srgan_amd.ops")
    dev = torch.device("cpu" if L.is_emulation() else "cuda")
    img = np.array(Image.open(a.image).convert("RGB"))
    x = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).to(dev).float().div(127.5).sub(1.0)[None].contiguous()
    if a.kernel and a.sinc:
        raise SystemExit("--kernel and --sinc are one stage: name one of them")
    if a.kernel or a.sinc:
        x = ops.filter2d(x, [parse_kernel(a.kernel) if a.kernel else parse_sinc(a.sinc)])
    if a.filter:
        dl = importlib.import_module("fast-srgan_amd.dataloader")
        h, w = x.shape[2:]
        if a.scale < 1 or h % a.scale or w % a.scale:
            raise SystemExit("--scale must divide the picture's %d x %d pixels" % (w, h))
        tables = ops.ResizeTables([dl.resize_taps(w, w // a.scale, a.filter)], [dl.resize_taps(h, h // a.scale, a.filter)], h, w, dev)
        x = ops.resize_select(x, tables, [0])
    if not (a.shot or a.grey):                               # the first-order stages as ever
        if a.blur or a.noise:
            x = ops.degrade_blur_noise(x, [a.blur] if a.blur else None, [a.noise] if a.noise else None, [seed_words(a.seed)] if a.noise else None)
    else:
        if a.blur:
            x = ops.degrade_blur_noise(x, [a.blur], None, None)
        x = _noise(ops, L, x, a, seed_words(a.seed))
    if a.jpeg:
        x = ops.jpeg_roundtrip(x, [a.jpeg], a.subsampling)
    if a.second:
        b = _second_parser().parse_args(shlex.split(a.second))
        if b.kernel:
            x = ops.filter2d(x, [parse_kernel(b.kernel)])
        x = _noise(ops, L, x, b, seed_words(a.seed + 1))
        if b.sinc and b.sinc_first:
            x = ops.filter2d(x, [parse_sinc(b.sinc)])
        if b.jpeg:
            x = ops.jpeg_roundtrip(x, [b.jpeg], a.subsampling)
        if b.sinc and not b.sinc_first:
            x = ops.filter2d(x, [parse_sinc(b.sinc)])
    out = x[0].add(1.0).mul(127.5).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    Image.fromarray(out).save(a.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
