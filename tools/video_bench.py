"""Video inference at 180x320 -> 720x1280, batch 32 (the README's inference workload), shipped weights (tests/golden/g_model_pt.npz):

  1. model only: Generator.forward_yuv420 (I420 in, I420 planes out of the head's epilogue) against Generator.forward_u8 (RGB
     bytes in and out), each captured as one hipGraph and timed with device events over `--replays` replays; the two are
     interleaved round by round on the same device (`--rounds`), in f16 and x3; medians reported;
  2. end to end: `python video.py --input <file> --output /dev/null` on a seeded synthetic Y4M stream of `--frames` frames
     (f16, --batch 32), run as a child process: its own steady-state figure (frames after the first batch, whose plan build and
     graph capture it excludes) and the wall time of the whole process.

  3. `--resize`: the arbitrary-output-size leg alone.  360x640,
     batch 8, f16, every path one hipGraph, device events, interleaved round by round:
       (a) forward_u8 at the native 1440x2560;   (b) forward_u8(out_size=(1080, 1920)), the fused resize after the head;
       (c) the same frames composed in torch from the float head: F.interpolate(bicubic, antialias=True), clamp, x255, uint8, permute;
     then (a) and (b) again for forward_yuv420, and the resample kernel alone from its own events (ops.PROFILE_RESAMPLE) with its
     achieved bytes/s over its algorithmic bytes: 12 B per source pixel + 3 (RGB) or 1.5 (I420) B per output pixel.

  4. `--deep`: samples deeper than 8 bits.  360x640, batch 8, f16, every path one hipGraph, device events,
     interleaved round by round:
       (a) forward_yuv420, 8 bits in and out (the head's I420 epilogue);   (b) 10 bits in, 10 bits out;   (c) 8 bits in, 10 bits out
     -- (b) and (c) are the float head followed by the encode kernel -- then the encode kernel alone from its own events
     (ops.PROFILE_YUV) over its algorithmic bytes: 12 B in + 3 B out per pixel.

  5. `--chroma`: 4:2:2 and 4:4:4.  360x640, batch 8, f16, every path one hipGraph, device events, interleaved round
     by round:
       (a) forward_yuv 420 -> 420, 8 bits (the head's I420 epilogue);   (b) 420 -> 444;   (c) 444 -> 444;   (d) 422 -> 422 at 10 bits
     -- (b), (c), (d) are the float head followed by the encode kernel -- then the decode and encode kernels alone from their own
     events (ops.PROFILE_YUV) over their algorithmic bytes: decode 12 B out + 3 (4:4:4) or 2 (4:2:2) B in per pixel at 8 bits, encode
     12 B in + 3 or 2 B out.

  6. `--bands`: the generator's tail in row bands.  forward_u8, every path one hipGraph, device events, interleaved
     round by round, f16 and x3 (`--modes`):
       (a) 1080p, batch 1: whole against banded at R = 32 / 64 / 128 -- the cost of banding where both paths exist;
       (b) 720p: batch 2 whole against batch 8 banded at R = 128 (the default band_rows), frames per second;
       (c) 1440p (batch 2) and 2160p (batch 1) banded at R = 128: sizes the whole path refuses;
       (d) the row-copy kernel alone from its own events (f16, 1080p, R = 128): the gather of the last up-sampling convolution's
           input and the scatter of the uint8 frame, over the bytes moved (read + written).

  7. `--layout`: semi-planar frames (NV12, P010) beside their planar twins, f16, device events, planar and semi-planar
     interleaved round by round (the order reversed every other round):
       (a) the decode, encode and resample kernels alone at 1080p output, batch 4, 8 and 10 bits, from their own events
           (ops.PROFILE_YUV / PROFILE_RESAMPLE; the resample takes 1440x2560 to 1080p, the 9-tap form);
       (b) model only at 180x320 -> 720x1280, batch 32, one hipGraph each: forward_yuv planar in and out (the head's I420 epilogue),
           planar in / NV12 out (the head's NV12 epilogue) and NV12 in and out.
     Every semi-planar figure is printed with the spread (max - min over the rounds) its planar twin shows on the same device, and
     whether it lies within it.  `--planar_only` measures the planar paths alone (the same code on another build of the library: the
     parent commit's tree, say); `--out FILE` (default profiles/video_bench_nv12.txt) also keeps the lines in a file.

    python tools/video_bench.py [--frames 2048] [--rounds 7] [--replays 20] [--modes f16,x3]
    python tools/video_bench.py --resize [--rounds 7] [--replays 20]
    python tools/video_bench.py --deep [--rounds 7] [--replays 20]
    python tools/video_bench.py --chroma [--rounds 7] [--replays 20]
    python tools/video_bench.py --bands [--rounds 7] [--replays 20] [--modes f16,x3]
    python tools/video_bench.py --layout [--rounds 5] [--replays 20] [--planar_only] [--out FILE]
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


def resize_leg(sd, rounds, replays, mode="f16", h=360, w=640, b=8, size=(1080, 1920)):
    import torch.nn.functional as F
    dev = "cuda:0"
    G = pkg.Generator(types.SimpleNamespace(n_filters=64, n_layers=8), compute_dtype=mode)
    G.load_state_dict(sd)
    G.to(dev).eval()
    rng = np.random.default_rng(0)
    x_rgb = torch.from_numpy(rng.integers(0, 256, size=(b, h, w, 3), dtype=np.uint8)).to(dev)
    x_yuv = torch.from_numpy(rng.integers(0, 256, size=(b, ops.i420_frame_bytes(h, w)), dtype=np.uint8)).to(dev)

    def torch_path(x):
        with torch.no_grad():
            t = G(ops.u8_to_image(x))
            y = F.interpolate(t, size=size, mode="bicubic", antialias=True, align_corners=False)
            return (((y + 1) / 2).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    # the three paths agree before anything is timed (codes within 1: float32 resizes of one head output in two summation orders)
    y_b, y_c = G.forward_u8(x_rgb, out_size=size), torch_path(x_rgb)
    diff = (y_b.int() - y_c.int()).abs()
    print("resize      fused vs torch-composed uint8 frames: max |code difference| %d, %.4f %% of the samples differ"
          % (int(diff.max()), 100.0 * float((diff > 0).float().mean())), flush=True)
    paths = [("u8 native %dx%d" % (4 * h, 4 * w), graphed(G.forward_u8, x_rgb)),
             ("u8 fused resize %dx%d" % size, graphed(lambda x: G.forward_u8(x, out_size=size), x_rgb)),
             ("u8 torch-composed resize", graphed(torch_path, x_rgb)),
             ("yuv420 native", graphed(lambda x: G.forward_yuv420(x, h, w), x_yuv)),
             ("yuv420 fused resize", graphed(lambda x: G.forward_yuv420(x, h, w, out_size=size), x_yuv))]
    times = [[] for _ in paths]
    for _, g in paths:
        time_graph(g, 3)
    for r in range(rounds):
        order = list(range(len(paths)))
        for i in (order if r % 2 == 0 else order[::-1]):
            times[i].append(time_graph(paths[i][1], replays))
    med = [statistics.median(t) for t in times]
    for (name, _), m, t in zip(paths, med, times):
        print("resize      %-4s batch %d %dx%d  %-28s %7.3f ms/batch  %7.1f FPS   [per-round ms %s]" % (
            mode, b, h, w, name, 1e3 * m, b / m, " ".join("%.3f" % (1e3 * v) for v in t)), flush=True)
    print("resize      fused / torch-composed (u8): %.3f x faster;  fused resize - native: u8 %+.3f ms, yuv420 %+.3f ms per batch"
          % (med[2] / med[1], 1e3 * (med[1] - med[0]), 1e3 * (med[4] - med[3])), flush=True)
    # the kernel alone, from its own events, on a real head output
    with torch.no_grad():
        t = G(ops.u8_to_image(x_rgb)).permute(0, 2, 3, 1)
    for kind in ("u8", "i420"):
        for _ in range(5):
            ops.resample_image(t, size[0], size[1], kind)
        torch.cuda.synchronize()
        ops.PROFILE_RESAMPLE = []
        for _ in range(50):
            ops.resample_image(t, size[0], size[1], kind)
        torch.cuda.synchronize()
        prof, ops.PROFILE_RESAMPLE = ops.PROFILE_RESAMPLE, None
        ms = sorted(e0.elapsed_time(e1) for e0, e1, _ in prof)
        nbytes = prof[0][2]
        print("resize      kernel resample_kernel<%s,9> %dx%d -> %dx%d batch %d: median %.1f us, min %.1f us (own events, 50 launches); "
              "%.1f MB algorithmic -> %.2f TB/s at the median" % (kind, h * 4, w * 4, size[0], size[1], b, 1e3 * ms[len(ms) // 2], 1e3 * ms[0],
                                                               nbytes / 1e6, nbytes / (ms[len(ms) // 2] * 1e-3) / 1e12), flush=True)
    return med


def deep_leg(sd, rounds, replays, mode="f16", h=360, w=640, b=8, d=10):
    dev = "cuda:0"
    G = pkg.Generator(types.SimpleNamespace(n_filters=64, n_layers=8), compute_dtype=mode)
    G.load_state_dict(sd)
    G.to(dev).eval()
    rng = np.random.default_rng(0)
    x8 = torch.from_numpy(rng.integers(0, 256, size=(b, ops.i420_frame_bytes(h, w)), dtype=np.uint8)).to(dev)
    deep = rng.integers(0, 2 ** d, size=(b, ops.i420_frame_bytes(h, w)), dtype=np.uint16)
    xd = torch.from_numpy(np.ascontiguousarray(deep.astype("<u2")).view(np.uint8)).to(dev)
    paths = [("8 in, 8 out (head epilogue)", graphed(lambda x: G.forward_yuv420(x, h, w), x8)),
             ("%d in, %d out" % (d, d), graphed(lambda x: G.forward_yuv420(x, h, w, depth=d), xd)),
             ("8 in, %d out" % d, graphed(lambda x: G.forward_yuv420(x, h, w, out_depth=d), x8))]
    times = [[] for _ in paths]
    for _, g in paths:
        time_graph(g, 3)
    for r in range(rounds):
        order = list(range(len(paths)))
        for i in (order if r % 2 == 0 else order[::-1]):
            times[i].append(time_graph(paths[i][1], replays))
    med = [statistics.median(t) for t in times]
    for (name, _), m, t in zip(paths, med, times):
        print("deep        %-4s batch %d %dx%d  yuv420 %-28s %7.3f ms/batch  %7.1f FPS   [per-round ms %s]" % (
            mode, b, h, w, name, 1e3 * m, b / m, " ".join("%.3f" % (1e3 * v) for v in t)), flush=True)
    print("deep        %d/%d - 8/8: %+.3f ms per batch (%+.2f %%);  8/%d - 8/8: %+.3f ms per batch (%+.2f %%)" % (
        d, d, 1e3 * (med[1] - med[0]), 100.0 * (med[1] / med[0] - 1.0), d, 1e3 * (med[2] - med[0]), 100.0 * (med[2] / med[0] - 1.0)), flush=True)
    # the encode kernel alone, from its own events, on a real head output
    with torch.no_grad():
        t = G(ops.i420_to_image(x8, h, w)).permute(0, 2, 3, 1)
    for depth in (8, d):
        for _ in range(5):
            ops.image_to_i420(t, depth=depth)
        torch.cuda.synchronize()
        ops.PROFILE_YUV = []
        for _ in range(50):
            ops.image_to_i420(t, depth=depth)
        torch.cuda.synchronize()
        prof, ops.PROFILE_YUV = ops.PROFILE_YUV, None
        ms = sorted(e0.elapsed_time(e1) for _, _, e0, e1, _ in prof)
        nbytes = prof[0][4]
        print("deep        kernel image_to_i420_kernel<%s> %dx%d batch %d: median %.1f us, min %.1f us (own events, 50 launches); "
              "%.1f MB algorithmic -> %.2f TB/s at the median" % ("u8" if depth == 8 else "u16", 4 * h, 4 * w, b, 1e3 * ms[len(ms) // 2],
                                                               1e3 * ms[0], nbytes / 1e6, nbytes / (ms[len(ms) // 2] * 1e-3) / 1e12), flush=True)
    return med


def chroma_leg(sd, rounds, replays, mode="f16", h=360, w=640, b=8, d=10):
    dev = "cuda:0"
    G = pkg.Generator(types.SimpleNamespace(n_filters=64, n_layers=8), compute_dtype=mode)
    G.load_state_dict(sd)
    G.to(dev).eval()
    rng = np.random.default_rng(0)

    def payload(chroma, depth):
        nb = ops.yuv_frame_bytes(h, w, chroma, depth)
        if depth == 8:
            return torch.from_numpy(rng.integers(0, 256, size=(b, nb), dtype=np.uint8)).to(dev)
        deep = rng.integers(0, 2 ** depth, size=(b, nb // 2), dtype=np.uint16)
        return torch.from_numpy(np.ascontiguousarray(deep.astype("<u2")).view(np.uint8)).to(dev)

    x420, x444, x422d = payload("420", 8), payload("444", 8), payload("422", d)
    paths = [("420 -> 420, 8 bits (head epilogue)", graphed(lambda x: G.forward_yuv(x, h, w), x420)),
             ("420 -> 444, 8 bits", graphed(lambda x: G.forward_yuv(x, h, w, out_chroma="444"), x420)),
             ("444 -> 444, 8 bits", graphed(lambda x: G.forward_yuv(x, h, w, chroma="444"), x444)),
             ("422 -> 422, %d bits" % d, graphed(lambda x: G.forward_yuv(x, h, w, chroma="422", depth=d), x422d))]
    times = [[] for _ in paths]
    for _, g in paths:
        time_graph(g, 3)
    for r in range(rounds):
        order = list(range(len(paths)))
        for i in (order if r % 2 == 0 else order[::-1]):
            times[i].append(time_graph(paths[i][1], replays))
    med = [statistics.median(t) for t in times]
    for (name, _), m, t in zip(paths, med, times):
        print("chroma      %-4s batch %d %dx%d  yuv %-36s %7.3f ms/batch  %7.1f FPS   [per-round ms %s]" % (
            mode, b, h, w, name, 1e3 * m, b / m, " ".join("%.3f" % (1e3 * v) for v in t)), flush=True)
    print("chroma      " + ";  ".join("%s - (a): %+.3f ms per batch (%+.2f %%)" % (paths[i][0].split(",")[0], 1e3 * (med[i] - med[0]),
                                                                                  100.0 * (med[i] / med[0] - 1.0)) for i in (1, 2, 3)), flush=True)
    # the decode and encode kernels alone, from their own events; the encode on a real head output
    with torch.no_grad():
        t = G(ops.i420_to_image(x420, h, w)).permute(0, 2, 3, 1).contiguous()
    x444o, x422o = payload("444", 8), payload("422", 8)
    runs = [("yuv_to_image_kernel<u8,444>", h, w, lambda: ops.yuv_to_image(x444o, h, w, "444")),
            ("yuv_to_image_kernel<u8,422>", h, w, lambda: ops.yuv_to_image(x422o, h, w, "422")),
            ("yuv_to_image_kernel<u16,422>", h, w, lambda: ops.yuv_to_image(x422d, h, w, "422", depth=d)),
            ("image_to_yuv_kernel<u8,444>", 4 * h, 4 * w, lambda: ops.image_to_yuv(t, "444")),
            ("image_to_yuv_kernel<u8,422>", 4 * h, 4 * w, lambda: ops.image_to_yuv(t, "422")),
            ("image_to_yuv_kernel<u16,422>", 4 * h, 4 * w, lambda: ops.image_to_yuv(t, "422", depth=d))]
    for name, kh, kw, fn in runs:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ops.PROFILE_YUV = []
        for _ in range(50):
            fn()
        torch.cuda.synchronize()
        prof, ops.PROFILE_YUV = ops.PROFILE_YUV, None
        ms = sorted(e0.elapsed_time(e1) for _, _, e0, e1, _ in prof)
        nbytes = prof[0][4]
        print("chroma      kernel %-30s %dx%d batch %d: median %.1f us, min %.1f us (own events, 50 launches); "
              "%.1f MB algorithmic -> %.2f TB/s at the median" % (name, kh, kw, b, 1e3 * ms[len(ms) // 2], 1e3 * ms[0], nbytes / 1e6,
                                                               nbytes / (ms[len(ms) // 2] * 1e-3) / 1e12), flush=True)
    return med


def _interleaved(paths, rounds, replays):
    """Per-path lists of seconds per batch: `rounds` rounds over all the graphs, the order reversed every other round."""
    times = [[] for _ in paths]
    for _, g, _ in paths:
        time_graph(g, 2)
    for r in range(rounds):
        order = list(range(len(paths)))
        for i in (order if r % 2 == 0 else order[::-1]):
            times[i].append(time_graph(paths[i][1], replays))
    return times


def bands_leg(sd, rounds, replays, mode, R=128):
    dev = "cuda:0"
    G = pkg.Generator(types.SimpleNamespace(n_filters=64, n_layers=8), compute_dtype=mode)
    G.load_state_dict(sd)
    G.to(dev).eval()
    rng = np.random.default_rng(0)

    def frames(b, h, w):
        return torch.from_numpy(rng.integers(0, 256, size=(b, h, w, 3), dtype=np.uint8)).to(dev)

    def report(tag, paths, times):
        med = [statistics.median(t) for t in times]
        for (name, _, b), m, t in zip(paths, med, times):
            spread = 100.0 * (max(t) - min(t)) / m
            print("bands       %-4s %-4s %-30s %9.3f ms/batch  %7.2f FPS   spread %.2f %%   [per-round ms %s]" % (
                mode, tag, name, 1e3 * m, b / m, spread, " ".join("%.3f" % (1e3 * v) for v in t)), flush=True)
        return med

    # (a) 1080p, batch 1: whole against banded
    x = frames(1, 1080, 1920)
    peaks = []
    for r in (None, R):         # eager, before any graph holds a pool: the same bytes, and the peak activation memory of either path
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        peaks.append((G.forward_u8(x, bands=r), (torch.cuda.max_memory_allocated() - base) / 1e9))
    assert torch.equal(peaks[0][0], peaks[1][0])
    print("bands       %-4s (a)  1080p batch 1 peak activation memory: whole %.2f GB, banded R=%d %.2f GB" % (mode, peaks[0][1], R, peaks[1][1]),
          flush=True)
    del peaks
    paths = [("1080p batch 1 whole", graphed(G.forward_u8, x), 1)]
    paths += [("1080p batch 1 banded R=%d" % r, graphed(lambda t, r=r: G.forward_u8(t, bands=r), x), 1) for r in (32, 64, 128)]
    med = report("(a)", paths, _interleaved(paths, rounds, replays))
    print("bands       %-4s (a)  banded - whole: %s" % (mode, ";  ".join(
        "R=%d %+.3f ms (%+.2f %%)" % (r, 1e3 * (m - med[0]), 100.0 * (m / med[0] - 1.0)) for r, m in zip((32, 64, 128), med[1:]))), flush=True)
    del paths, x
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    # (b) 720p: batch 2 whole against batch 8 banded
    x2, x8 = frames(2, 720, 1280), frames(8, 720, 1280)
    paths = [("720p batch 2 whole", graphed(G.forward_u8, x2), 2), ("720p batch 8 banded R=%d" % R, graphed(lambda t: G.forward_u8(t, bands=R), x8), 8)]
    times = _interleaved(paths, rounds, max(2, replays // 2))
    med = report("(b)", paths, times)
    print("bands       %-4s (b)  FPS banded batch 8 / whole batch 2 = %.4f" % (mode, (8 / med[1]) / (2 / med[0])), flush=True)
    del paths, x2, x8
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    # (c) sizes the whole path refuses
    for b, h, w in ((2, 1440, 2560), (1, 2160, 3840)):
        x = frames(b, h, w)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        paths = [("%dx%d batch %d banded R=%d" % (w, h, b, R), graphed(lambda t: G.forward_u8(t, bands=R), x), b)]
        report("(c)", paths, _interleaved(paths, min(rounds, 3), max(2, replays // 4)))
        print("bands       %-4s (c)  %dx%d batch %d peak activation memory %.2f GB" % (mode, w, h, b, (torch.cuda.max_memory_allocated() - base) / 1e9),
              flush=True)
        del paths, x
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def rows_kernel_leg(sd, mode="f16", h=1080, w=1920, R=128):
    """(d): fsr_copy_rows alone, from its own events: one launch over all the windows of a 1080p frame."""
    dev = "cuda:0"
    G = pkg.Generator(types.SimpleNamespace(n_filters=64, n_layers=8), compute_dtype=mode)
    G.load_state_dict(sd)
    G.to(dev).eval()
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.integers(0, 256, size=(1, h, w, 3), dtype=np.uint8)).to(dev)
    with torch.no_grad():
        m = G._body(ops.u8_to_image(x))
    _, H2, W2, c = m.shape
    nwin, Hw, es = len(ops.tail_windows(H2, R)), R + 4, m.element_size()
    group = torch.empty((nwin, Hw, W2, c), dtype=m.dtype, device=dev)
    y = torch.empty((nwin, 2 * Hw, 2 * W2, 3), dtype=torch.uint8, device=dev)
    out = torch.empty((1, 2 * H2, 2 * W2, 3), dtype=torch.uint8, device=dev)
    row, orow = W2 * c * es, 2 * W2 * 3
    runs = [("gather  %dx%dx%d %s -> %d windows of %d rows" % (H2, W2, c, mode, nwin, Hw), 2 * nwin * Hw * row,
             lambda: ops.copy_rows(m, group, H2 * row, Hw * row, row, 0, nwin, H2, R)),
            ("scatter uint8 frame %dx%d" % (2 * H2, 2 * W2), 2 * 2 * H2 * orow,
             lambda: ops.copy_rows(y, out, 2 * Hw * orow, 2 * H2 * orow, orow, 0, nwin, H2, R, 2, True))]
    for name, nbytes, fn in runs:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        evs = []
        for _ in range(50):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
        print("bands       (d)  kernel %s  %-52s median %.1f us, min %.1f us (own events, 50 launches); %.1f MB read + written -> "
              "%.2f TB/s at the median" % (ops._last_kernel(), name, 1e3 * ms[len(ms) // 2], 1e3 * ms[0], nbytes / 1e6,
                                           nbytes / (ms[len(ms) // 2] * 1e-3) / 1e12), flush=True)


def layout_leg(sd, rounds, replays, planar_only=False, out=None, mode="f16"):
    dev = "cuda:0"
    rounds = max(3, rounds)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    G = pkg.Generator(types.SimpleNamespace(n_filters=64, n_layers=8), compute_dtype=mode)
    G.load_state_dict(sd)
    G.to(dev).eval()
    rng = np.random.default_rng(0)
    layouts = ("planar",) if planar_only else ("planar", "nv12")
    say("layout      device %s, %s, %d rounds, planar and semi-planar interleaved; spread = (max - min) / median over the rounds"
        % (torch.cuda.get_device_name(0), mode, rounds))

    def kw(layout):     # (a build without the keyword measures its planar paths with the same code)
        return {} if layout == "planar" else {"layout": layout}

    def payload(b, h, w, d):
        # random bytes are legal in either layout (16-bit semi-planar samples: the low bits are ignored)
        return torch.from_numpy(rng.integers(0, 256, size=(b, ops.yuv_frame_bytes(h, w, "420", d)), dtype=np.uint8)).to(dev)

    def verdict(name, unit, t):
        """t: layout -> per-round figures.  Prints each path, and for the semi-planar one where it lies against the planar spread."""
        mp = statistics.median(t["planar"])
        sp = max(t["planar"]) - min(t["planar"])
        say("layout      %-46s planar %9.2f %s  spread %5.2f %%  [per round %s]" % (
            name, mp, unit, 100.0 * sp / mp, " ".join("%.2f" % v for v in t["planar"])))
        if "nv12" in t:
            ms = statistics.median(t["nv12"])
            where = "within the planar spread" if abs(ms - mp) <= sp else ("outside it: FASTER" if ms < mp else "outside it: SLOWER")
            say("layout      %-46s nv12   %9.2f %s  %+6.2f %% against planar, %s  [per round %s]" % (
                name, ms, unit, 100.0 * (ms / mp - 1.0), where, " ".join("%.2f" % v for v in t["nv12"])))

    # (a) the kernels alone, from their own events
    b, oh, ow = 4, 1080, 1920
    t_enc = (torch.rand(b, oh, ow, 3, device=dev) * 2.2 - 1.1).contiguous()
    t_rs = (torch.rand(b, 1440, 2560, 3, device=dev) * 2.2 - 1.1).contiguous()
    for d in (8, 10):
        x = payload(b, oh, ow, d)
        runs = [("decode   %dx%d batch %d, %2d bits" % (ow, oh, b, d), "PROFILE_YUV", lambda lay: ops.yuv_to_image(x, oh, ow, depth=d, **kw(lay))),
                ("encode   %dx%d batch %d, %2d bits" % (ow, oh, b, d), "PROFILE_YUV", lambda lay: ops.image_to_yuv(t_enc, depth=d, **kw(lay))),
                ("resample 2560x1440 -> %dx%d batch %d, %2d bits" % (ow, oh, b, d), "PROFILE_RESAMPLE",
                 lambda lay: ops.resample_image(t_rs, oh, ow, "i420", depth=d, **kw(lay)))]
        for name, hook, fn in runs:
            times = {lay: [] for lay in layouts}
            for lay in layouts:
                for _ in range(5):
                    fn(lay)
            torch.cuda.synchronize()
            for r in range(rounds):
                for lay in (layouts if r % 2 == 0 else layouts[::-1]):
                    setattr(ops, hook, [])
                    for _ in range(30):
                        fn(lay)
                    torch.cuda.synchronize()
                    prof = getattr(ops, hook)
                    setattr(ops, hook, None)
                    us = sorted(1e3 * e[-3].elapsed_time(e[-2]) for e in prof)
                    times[lay].append(us[len(us) // 2])
            verdict(name, "us", times)
        del x
    del t_enc, t_rs
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    # (b) model only, one graph per path
    x_p = payload(B, H, W, 8)
    paths = [("planar", graphed(lambda x: G.forward_yuv(x, H, W), x_p))]
    if not planar_only:
        paths += [("nv12 out", graphed(lambda x: G.forward_yuv(x, H, W, out_layout="nv12"), x_p)),
                  ("nv12 in and out", graphed(lambda x: G.forward_yuv(x, H, W, layout="nv12"), x_p))]
    times = [[] for _ in paths]
    for _, g in paths:
        time_graph(g, 3)
    for r in range(rounds):
        order = list(range(len(paths)))
        for i in (order if r % 2 == 0 else order[::-1]):
            times[i].append(1e3 * time_graph(paths[i][1], replays))
    for i in range(1, max(2, len(paths))):
        t = {"planar": times[0]}
        if i < len(paths):
            t["nv12"] = times[i]
        verdict("model %dx%d -> %dx%d batch %d%s" % (W, H, 4 * W, 4 * H, B, ", " + paths[i][0] if i < len(paths) else ""), "ms", t)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


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
    ap.add_argument("--resize", action="store_true", help="run the arbitrary-output-size leg only")
    ap.add_argument("--deep", action="store_true", help="run the deep-sample leg only")
    ap.add_argument("--chroma", action="store_true", help="run the 4:2:2 / 4:4:4 leg only")
    ap.add_argument("--bands", action="store_true", help="run the row-band leg only")
    ap.add_argument("--layout", action="store_true", help="run the semi-planar (NV12 / P010) leg only")
    ap.add_argument("--planar_only", action="store_true", help="--layout: the planar paths alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_bench_nv12.txt"), help="--layout: file the lines are appended to")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("video_bench needs the MI355X")
    sd = shipped_state_dict()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    if args.resize:
        resize_leg(sd, args.rounds, args.replays)
        return
    if args.deep:
        deep_leg(sd, args.rounds, args.replays)
        return
    if args.chroma:
        chroma_leg(sd, args.rounds, args.replays)
        return
    if args.layout:
        layout_leg(sd, min(args.rounds, 5), args.replays, args.planar_only, args.out)
        return
    if args.bands:
        for mode in args.modes.split(","):
            bands_leg(sd, args.rounds, args.replays, mode)
        rows_kernel_leg(sd)
        return
    model = {}
    for mode in args.modes.split(","):
        model[mode] = model_only(sd, mode, args.rounds, args.replays)
    steady = end_to_end(sd, args.frames, "f16")
    if "f16" in model:
        print("end to end / model-only forward_yuv420 (f16): %.3f" % (steady / model["f16"][1]), flush=True)


if __name__ == "__main__":
    main()
