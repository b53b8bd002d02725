"""Video inference at 180x320 -> 720x1280, batch 32 (the README's inference workload), shipped weights (tests/golden/g_model_pt.npz):

  1. model only: Generator.forward_yuv420 (I420 in, I420 planes out of the head's epilogue) against Generator.forward_u8 (RGB
     bytes in and out), each captured as one hipGraph and timed with device events over `--replays` replays; the two are
     interleaved round by round on the same device (`--rounds`), in f16 and x3; medians reported;
  2. end to end: `python video.py --input <file> --output /dev/null` on a seeded synthetic Y4M stream of `--frames` frames
     (f16, --batch 32), run as a child process: its own steady-state figure (frames after the first batch, whose plan build and
     graph capture it excludes) and the wall time of the whole process.

    python tools/video_bench.py [--frames 2048] [--rounds 7] [--replays 20] [--modes f16,x3]
"""
import argparse
import importlib
import os
import re
import statistics
import subprocess
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

H, W, B = 180, 320, 32


def shipped_state_dict():
    z = np.load(os.path.join(ROOT, "tests", "golden", "g_model_pt.npz"))
    return {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("sd.")}


def graphed(fn, x):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn(x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn(x)
    return g


def time_graph(g, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / 1e3 / replays     # seconds per batch


def model_only(sd, mode, rounds, replays):
    dev = "cuda:0"
    G = pkg.Generator(types.SimpleNamespace(n_filters=64, n_layers=8), compute_dtype=mode)
    G.load_state_dict(sd)
    G.to(dev).eval()
    rng = np.random.default_rng(0)
    x_rgb = torch.from_numpy(rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)).to(dev)
    x_yuv = torch.from_numpy(rng.integers(0, 256, size=(B, ops.i420_frame_bytes(H, W)), dtype=np.uint8)).to(dev)
    g_rgb = graphed(G.forward_u8, x_rgb)
    g_yuv = graphed(lambda x: G.forward_yuv420(x, H, W), x_yuv)
    for g in (g_rgb, g_yuv):        # warm
        time_graph(g, 3)
    t_rgb, t_yuv = [], []
    for r in range(rounds):         # interleaved, alternating which goes first
        pair = [(g_rgb, t_rgb), (g_yuv, t_yuv)]
        for g, acc in (pair if r % 2 == 0 else pair[::-1]):
            acc.append(time_graph(g, replays))
    fps_rgb, fps_yuv = B / statistics.median(t_rgb), B / statistics.median(t_yuv)
    print("model only  %-4s batch %d %dx%d -> %dx%d:  forward_u8 %8.1f FPS (%.3f ms/batch)   forward_yuv420 %8.1f FPS (%.3f ms/batch)"
          "   yuv420 / u8 = %.3f   [per-round FPS u8 %s | yuv420 %s]" % (
              mode, B, H, W, 4 * H, 4 * W, fps_rgb, 1e3 * B / fps_rgb, fps_yuv, 1e3 * B / fps_yuv, fps_yuv / fps_rgb,
              " ".join("%.0f" % (B / t) for t in t_rgb), " ".join("%.0f" % (B / t) for t in t_yuv)), flush=True)
    del g_rgb, g_yuv
    torch.cuda.synchronize()
    return fps_rgb, fps_yuv


def end_to_end(sd, frames, mode):
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "configs"))
        os.makedirs(os.path.join(tmp, "models"))
        with open(os.path.join(tmp, "configs", "config.yaml"), "w") as f:
            f.write("generator:\n  n_filters: 64\n  n_layers: 8\ntraining:\n  compute_dtype: %s\n" % mode)
        torch.save(sd, os.path.join(tmp, "models", "model.pt"))
        src = os.path.join(tmp, "in.y4m")
        rng = np.random.default_rng(1234)
        fb = ops.i420_frame_bytes(H, W)
        with open(src, "wb") as f:
            f.write(b"YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 C420jpeg\n" % (W, H))
            for _ in range(frames):
                f.write(b"FRAME\n")
                f.write(rng.integers(0, 256, size=fb, dtype=np.uint8).tobytes())
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "video.py"), "--input", src, "--output", "/dev/null", "--batch", str(B)],
                           cwd=tmp, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("video.py failed:\n" + r.stderr[-4000:])
    last = [ln for ln in r.stderr.splitlines() if ln.startswith("video:")]
    m = re.search(r"([0-9.]+) fps after the first batch", last[-1])
    steady = float(m.group(1)) if m else float("nan")
    print("end to end  %-4s %d frames %dx%d -> %dx%d, Y4M file -> /dev/null, batch %d:  %.1f FPS steady state (CLI: %s)   "
          "process wall %.2f s incl. start-up = %.1f FPS" % (mode, frames, H, W, 4 * H, 4 * W, B, steady, last[-1], wall, frames / wall),
          flush=True)
    return steady


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--modes", default="f16,x3")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("video_bench needs the MI355X")
    sd = shipped_state_dict()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    model = {}
    for mode in args.modes.split(","):
        model[mode] = model_only(sd, mode, args.rounds, args.replays)
    steady = end_to_end(sd, args.frames, "f16")
    if "f16" in model:
        print("end to end / model-only forward_yuv420 (f16): %.3f" % (steady / model["f16"][1]), flush=True)


if __name__ == "__main__":
    main()
