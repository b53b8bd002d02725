"""What a degradation setting does to a picture, through the operators the training loader uses.

    python tools/degrade.py --image in.png --output out.png [--blur S] [--noise S] [--jpeg Q] [--subsampling 420|444] [--seed N]

--blur: Gaussian sigma in pixels (<= 3); --noise: sigma in 8-bit code units (<= 25); --jpeg: quality 1..100.  The order is the loader's:
blur, noise, JPEG.  A stage that is not named is not run; with none the picture is copied."""
import argparse
import importlib
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def seed_words(seed):
    """The two 32-bit words that name the noise field of --seed N."""
    rng = random.Random(seed)
    return rng.getrandbits(32), rng.getrandbits(32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
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
    if a.blur or a.noise:
        x = ops.degrade_blur_noise(x, [a.blur] if a.blur else None, [a.noise] if a.noise else None, [seed_words(a.seed)] if a.noise else None)
    if a.jpeg:
        x = ops.jpeg_roundtrip(x, [a.jpeg], a.subsampling)
    out = x[0].add(1.0).mul(127.5).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    Image.fromarray(out).save(a.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
