"""`python evaluate.py --hr_dir D [--lr_dir L] [--model a.pt b.pt ...]`: benchmark PSNR / SSIM of generator checkpoints.

The protocol of the super-resolution literature (Set5, Set14, BSD100, Urban100, DIV2K-val), on the device:
  * whole images, mod-cropped to a multiple of the scale (the top-left corner);
  * the luma of BT.601 "studio" YCbCr (`--channel rgb`: the three channels instead);
  * a border of `--shave` pixels (default: the scale) left out;
  * Wang's SSIM (11 x 11 Gaussian, sigma 1.5, data range 255, only windows inside the shaved region);
  * the dataset figure is the MEAN OF THE PER-IMAGE values -- unlike Trainer._calculate_metrics_over_dataset, which follows the
    reference's torchmetrics objects: PSNR from the mean squared error of everything it saw, in RGB, on random crops.
The super-resolved image is what inference.py would write: Generator.forward_u8's bytes, truncating cast included.  Both metrics
come from one launch per batch (ops.quality_u8) that reads those bytes and the mod-cropped view of the HR upload in place;
one (N, 2) float32 copy per batch reaches the host, which finishes in float64:
    psnr = 10 log10(255^2 count / sse)  (inf at sse == 0),    ssim = ssim_sum / (channels (eh - 10)(ew - 10)).
Without `--lr_dir` the LR images are made on the device by the training contract -- the dataloader's antialiased bicubic
(ops.resample_image) of the mod-cropped HR image, quantised with rint and a clamp -- once per image, cached in the Evaluator.
Evaluation runs eagerly (no graph capture: it happens once per checkpoint).
`--self_ensemble` adds, beside every model's column, a column `<path>+` of its self-ensemble result (Generator.forward_u8 with
ensemble=True): the EDSR+ / RCAN+ convention of the same tables.
"""
import json
import math
import os
import sys
from argparse import ArgumentParser

import numpy as np
import torch

from . import ops
from .config import load_config

IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".npy")

parser = ArgumentParser("Benchmark PSNR / SSIM of super-resolution checkpoints")
parser.add_argument("--hr_dir", required=True, type=str, help="high-resolution images: .png / .jpg, or uint8 (3,H,W) .npy")
parser.add_argument("--lr_dir", default=None, type=str, help="low-resolution inputs by basename (also <name>x<scale>); default: made on the device")
parser.add_argument("--model", default=["models/model.pt"], nargs="+", type=str, help="generator checkpoints: one table column each")
parser.add_argument("--compute_dtype", default=None, choices=["bf16", "f16", "x3", "x3v", "f32"], help="kernel precision")
parser.add_argument("--shave", default=None, type=int, help="border left out of both metrics (default: the scale)")
parser.add_argument("--channel", default="y", choices=["y", "rgb"])
parser.add_argument("--baseline", action="store_true", help="add a column for antialiased-bicubic up-scaling of the same LR images")
parser.add_argument("--batch", default=8, type=int, help="images of one shape per device batch")
parser.add_argument("--bands", default="auto", choices=["auto", "on", "off"], help="as inference.py: the generator's tail in row bands")
parser.add_argument("--band_rows", default=128, type=int)
parser.add_argument("--self_ensemble", action="store_true",
                    help="add a column <path>+ per model: the mean over the 8 flipped / transposed inputs (8x the generator work)")
parser.add_argument("--json", default=None, type=str, help="write the settings, the per-image rows and the means here")
parser.add_argument("--save_dir", default=None, type=str, help="write the super-resolved PNGs here (one sub-directory per model if several)")


def list_images(directory):
    return sorted(os.path.join(directory, f) for f in os.listdir(directory) if f.lower().endswith(IMAGE_EXTENSIONS))


def read_image(path):
    """uint8 (H,W,3): .png / .jpg via PIL, or the dataset's uint8 (3,H,W) .npy."""
    if path.lower().endswith(".npy"):
        arr = np.load(path)
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[0] != 3:
            raise ValueError("%s: expected a uint8 (3,H,W) array, got %s %s" % (path, arr.dtype, arr.shape))
        return np.ascontiguousarray(arr.transpose(1, 2, 0))
    from PIL import Image
    return np.array(Image.open(path).convert("RGB"))


def quantise(image):
    """float32 (N,3,H,W) view in [-1,1] of an NHWC buffer (ops.resample_image "f32") -> uint8 (N,H,W,3): rint of the 0..255 code."""
    return ((image.permute(0, 2, 3, 1) + 1.0) * 127.5).round().clamp(0.0, 255.0).to(torch.uint8)


def bicubic_u8(frames, out_h, out_w):
    """uint8 (N,H,W,3) -> uint8 (N,out_h,out_w,3) by the dataloader's antialiased bicubic, quantised with rint."""
    img = ops.u8_to_image(frames.contiguous())
    return quantise(ops.resample_image(img.permute(0, 2, 3, 1), out_h, out_w, "f32"))


class BicubicModel:
    """The baseline as a "model": antialiased-bicubic up-scaling by `scale` with the Evaluator's quantisation."""

    def __init__(self, scale):
        self.scale = int(scale)

    def forward_u8(self, frames, bands=None):
        return bicubic_u8(frames, self.scale * frames.shape[1], self.scale * frames.shape[2])


class _Bucket:
    """The images of one HR shape: one upload, one LR tensor."""


class Evaluator:
    """PSNR / SSIM of a generator over a set of HR images (module docstring).  hr_paths: image files; scale: the generator's
    up-scaling factor; lr_paths: the LR files in hr_paths' order, or None to make them on the device; shave: None = scale.
    Every HR image is uploaded once, in one tensor per image shape, and mod-cropped as a view; the LR images are cached, so
    several `run` calls (checkpoints, the EMA generator, the baseline) share both."""

    def __init__(self, hr_paths, scale, lr_paths=None, shave=None, channel="y", device="cuda", batch=8):
        self.scale, self.channel, self.device, self.batch = int(scale), channel, torch.device(device), max(1, int(batch))
        self.shave = self.scale if shave is None else int(shave)
        if channel not in ops.QUALITY_CHANNELS:
            raise ValueError("channel must be one of %s, got %r" % (sorted(ops.QUALITY_CHANNELS), channel))
        if self.scale < 1 or self.shave < 0:
            raise ValueError("scale must be positive and shave non-negative, got %d and %d" % (self.scale, self.shave))
        self.paths = list(hr_paths)
        if not self.paths:
            raise ValueError("Evaluator: no HR images")
        if lr_paths is not None and len(lr_paths) != len(self.paths):
            raise ValueError("Evaluator: %d LR files for %d HR images" % (len(lr_paths), len(self.paths)))
        self.names = [os.path.basename(p) for p in self.paths]
        s = self.scale
        groups = {}
        for i, path in enumerate(self.paths):
            hr = read_image(path)
            H, W = hr.shape[0] // s * s, hr.shape[1] // s * s
            if min(H, W) - 2 * self.shave < 11:
                raise ValueError("%s: %dx%d mod-cropped to %dx%d and shaved by %d leaves less than the 11x11 window of SSIM"
                                 % (path, hr.shape[1], hr.shape[0], W, H, self.shave))
            lr = None
            if lr_paths is not None:
                lr = read_image(lr_paths[i])
                if lr.shape[:2] != (H // s, W // s):
                    raise ValueError("%s is %dx%d, but %s mod-crops to %dx%d, which needs an LR image of %dx%d"
                                     % (lr_paths[i], lr.shape[1], lr.shape[0], path, W, H, W // s, H // s))
            groups.setdefault(hr.shape[:2], []).append((i, hr, lr))
        self.buckets = []
        for (h, w), items in groups.items():
            b = _Bucket()
            b.index = [i for i, _, _ in items]
            b.H, b.W = h // s * s, w // s * s
            b.hr_full = torch.from_numpy(np.stack([hr for _, hr, _ in items])).to(self.device)
            b.hr = b.hr_full[:, :b.H, :b.W]                                     # the mod-crop: a view
            if lr_paths is not None:
                b.lr = torch.from_numpy(np.stack([lr for _, _, lr in items])).to(self.device)
            else:
                with torch.no_grad():
                    b.lr = torch.cat([bicubic_u8(b.hr[j:j + 1], b.H // s, b.W // s) for j in range(len(items))])
            self.buckets.append(b)

    def _limits(self, model, bands, band_rows, ensemble=False):
        """(h, w) -> (images per batch, rows per band or None) by InferencePipeline's rules."""
        if not hasattr(model, "max_batch"):
            return lambda h, w: (self.batch, None)
        from .inference import InferencePipeline
        pipe = InferencePipeline(model, self.device, batch=self.batch, use_graph=False, bands=bands, band_rows=band_rows, ensemble=ensemble)
        return lambda h, w: (pipe._batch_for(h, w), pipe._bands_for(h, w))

    @torch.no_grad()
    def run(self, model, bands="auto", band_rows=128, save_dir=None, ensemble=False):
        """{"images": [{"name", "psnr", "ssim"} in hr_paths' order], "psnr": mean, "ssim": mean} of `model` (anything with
        Generator.forward_u8's signature).  save_dir: also write the super-resolved images there as PNGs.  ensemble: score the
        model's self-ensemble frames (forward_u8(..., ensemble=True); the argument is passed only when set)."""
        was_training = bool(getattr(model, "training", False))
        if hasattr(model, "eval"):
            model.eval()
        limits = self._limits(model, bands, band_rows, ensemble)
        extra = {"ensemble": True} if ensemble else {}
        channels = ops.QUALITY_CHANNELS[self.channel][1]
        rows = [None] * len(self.paths)
        try:
            for b in self.buckets:
                n, rows_per_band = limits(b.lr.shape[1], b.lr.shape[2])
                eh, ew = b.H - 2 * self.shave, b.W - 2 * self.shave
                for j in range(0, len(b.index), n):
                    sr = model.forward_u8(b.lr[j:j + n], bands=rows_per_band, **extra)
                    if tuple(sr.shape[1:]) != (b.H, b.W, 3):
                        raise ValueError("the model turned %s LR images into %s, expected %dx%d: is its scale %d?"
                                         % (tuple(b.lr.shape[1:3]), tuple(sr.shape[1:3]), b.H, b.W, self.scale))
                    r = ops.quality_u8(sr, b.hr[j:j + n], self.shave, self.channel).cpu().double().numpy()   # the batch's one copy
                    for k in range(r.shape[0]):
                        ssim_sum, sse = float(r[k, 0]), float(r[k, 1])
                        psnr = 10.0 * math.log10(255.0 ** 2 * channels * eh * ew / sse) if sse > 0 else float("inf")
                        i = b.index[j + k]
                        rows[i] = {"name": self.names[i], "psnr": psnr, "ssim": ssim_sum / (channels * (eh - 10) * (ew - 10))}
                    if save_dir is not None:
                        from PIL import Image
                        os.makedirs(save_dir, exist_ok=True)
                        host = sr.cpu().numpy()
                        for k in range(host.shape[0]):
                            name = os.path.splitext(self.names[b.index[j + k]])[0] + ".png"
                            Image.fromarray(host[k]).save(os.path.join(save_dir, name))
        finally:
            if was_training:
                model.train()
        return {"images": rows, "psnr": float(np.mean([r["psnr"] for r in rows])), "ssim": float(np.mean([r["ssim"] for r in rows]))}

    def baseline(self):
        """`run` for antialiased-bicubic up-scaling of the same LR images."""
        return self.run(BicubicModel(self.scale))


def match_lr_files(hr_paths, lr_dir, scale):
    """The LR file of every HR image: the same basename, or <name>x<scale>, with any image extension."""
    have = {os.path.splitext(f)[0]: os.path.join(lr_dir, f) for f in sorted(os.listdir(lr_dir)) if f.lower().endswith(IMAGE_EXTENSIONS)}
    out = []
    for p in hr_paths:
        stem = os.path.splitext(os.path.basename(p))[0]
        hit = have.get(stem) or have.get("%sx%d" % (stem, scale))
        if hit is None:
            raise ValueError("no LR image for %s in %s (looked for %s.* and %sx%d.*)" % (p, lr_dir, stem, stem, scale))
        out.append(hit)
    return out


def format_table(names, columns):
    """Plain-text table: one row per image and a last row of means; per column PSNR (dB) and SSIM."""
    width = max([len(n) for n in names] + [4])
    lines = [" " * width + "".join("  %22s" % c["name"][-22:] for c in columns)]
    for i, n in enumerate(names):
        lines.append(n.ljust(width) + "".join("  %10.4f dB  %8.6f" % (c["images"][i]["psnr"], c["images"][i]["ssim"]) for c in columns))
    lines.append("mean".ljust(width) + "".join("  %10.4f dB  %8.6f" % (c["psnr"], c["ssim"]) for c in columns))
    return "\n".join(lines)


def main(argv=None):
    from .inference import load_generator
    args = parser.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("fast-srgan_amd runs on an MI355X only: no GPU is visible")
    device = "cuda"
    config = load_config("configs/config.yaml")
    scale = 2 ** int(getattr(config.generator, "n_upsample", 2))
    hr_paths = list_images(args.hr_dir)
    if not hr_paths:
        raise SystemExit("no images in %s" % args.hr_dir)
    lr_paths = match_lr_files(hr_paths, args.lr_dir, scale) if args.lr_dir else None
    ev = Evaluator(hr_paths, scale, lr_paths, args.shave, args.channel, device, args.batch)
    columns = []
    if args.baseline:
        columns.append(dict(ev.baseline(), name="bicubic"))
    for path in args.model:
        model = load_generator(config, path, device, args.compute_dtype)
        save = args.save_dir
        if save is not None and len(args.model) > 1:
            save = os.path.join(save, os.path.splitext(os.path.basename(path))[0])
        columns.append(dict(ev.run(model, args.bands, args.band_rows, save), name=path))
        if args.self_ensemble:
            columns.append(dict(ev.run(model, args.bands, args.band_rows, None if save is None else save + "+", ensemble=True),
                                name=path + "+"))
        del model
    print(format_table(ev.names, columns))
    if args.json:
        settings = {"hr_dir": args.hr_dir, "lr_dir": args.lr_dir, "scale": scale, "shave": ev.shave, "channel": ev.channel,
                    "compute_dtype": args.compute_dtype or getattr(config.training, "compute_dtype", "f16"), "batch": args.batch,
                    "bands": args.bands, "band_rows": args.band_rows, "self_ensemble": bool(args.self_ensemble)}
        with open(args.json, "w") as f:
            json.dump({"settings": settings, "columns": columns}, f, indent=1)
    return columns


if __name__ == "__main__":
    main(sys.argv[1:])
