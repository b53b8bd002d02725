"""SHA-256 of every byte the video path produces, over seeded inputs: the listing two builds must share when a change to the video
code is meant to preserve behaviour (profiles/video_refactor_digests.txt holds one, per backend).

One line per case: the digest of the raw output bytes and the fsr_last_kernel note after the call, or the refusal's text.
  decode   ops.yuv_to_image      chroma x depth {8, 10, 16} x siting x matrix / range, odd and narrow frames
  encode   ops.image_to_yuv      the same grid, widths that are no multiple of 4 and that cross 64 columns
  resample ops.resample_image    "i420" at each chroma and depth {8, 12}, "f32", "u8"; the second size crosses a tile border
  forward  Generator.forward_yuv the tests' tiny f32 generator: the head's I420 epilogue, the encode kernels, the fused resize
  pipeline InferencePipeline     the plan keys run_yuv / run_yuv420 build for the forward cases (and, on a GPU, the frames)
  refusals the C entry points    the message of every argument check of the five YUV entry points

    python tools/video_digest.py --backend emu|hip
"""
import argparse
import ctypes
import hashlib
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("fast-srgan_amd")
ops = importlib.import_module("fast-srgan_amd.ops")
L = importlib.import_module("fast-srgan_amd._lib")

CHROMAS = ("420", "422", "444")
COLOURS = [(m, f) for m in ("bt601", "bt709") for f in (False, True)]


def line(name, fn):
    try:
        out = fn()
    except (ValueError, L.FsrError) as e:
        print("%-58s refused: %s" % (name, e))
        return
    raw = out.contiguous().cpu().numpy().tobytes()
    print("%-58s %s  %s" % (name, hashlib.sha256(raw).hexdigest(), L.lib().fsr_last_kernel().decode()))


def payload(rng, n, h, w, chroma, d, dev):
    nb = ops.yuv_frame_bytes(h, w, chroma, d)
    if d == 8:
        return torch.from_numpy(rng.integers(0, 256, size=(n, nb), dtype=np.uint8)).to(dev)
    codes = rng.integers(0, 2 ** d, size=(n, nb // 2))
    return torch.from_numpy(np.ascontiguousarray(codes.astype("<u2")).view(np.uint8)).to(dev)


def tanh_like(seed, n, h, w, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, h, w, 3, generator=g) * 2.2 - 1.1).contiguous().to(dev)


def decode(dev):
    rng = np.random.default_rng(1)
    for chroma in CHROMAS:
        for d in (8, 10, 16):
            for n, h, w in ((2, 5, 7), (1, 6, 70), (1, 3, 2)):
                x = payload(rng, n, h, w, chroma, d, dev)
                for siting in ("jpeg", "mpeg2"):
                    for matrix, full in COLOURS:
                        line("decode %s d%d %dx%dx%d %s %s %d" % (chroma, d, n, h, w, siting, matrix, full),
                             lambda: ops.yuv_to_image(x, h, w, chroma, siting, matrix, full, depth=d))


def encode(dev):
    for chroma in CHROMAS:
        shapes = ((2, 4, 6), (1, 6, 70), (1, 34, 132)) + (((2, 5, 7),) if chroma == "444" else ())
        for n, h, w in shapes:
            t = tanh_like(100 * h + w, n, h, w, dev)
            for d in (8, 10, 16):
                for matrix, full in COLOURS:
                    line("encode %s d%d %dx%dx%d %s %d" % (chroma, d, n, h, w, matrix, full),
                         lambda: ops.image_to_yuv(t, chroma, matrix, full, depth=d))


def resample(dev):
    for (h, w), (oh, ow) in (((9, 14), (20, 26)), ((6, 40), (9, 134))):
        t = tanh_like(9, 2, h, w, dev)
        for chroma in CHROMAS:
            for d in (8, 12):
                line("resample i420 %s d%d %dx%d->%dx%d" % (chroma, d, h, w, oh, ow),
                     lambda: ops.resample_image(t, oh, ow, "i420", "bt709", True, depth=d, chroma=chroma))
        for kind in ("f32", "u8"):
            line("resample %s %dx%d->%dx%d" % (kind, h, w, oh, ow), lambda: ops.resample_image(t, oh, ow, kind))


FORWARD = [   # (chroma, out_chroma, depth, out_depth, out_size)
    ("420", "420", 8, 8, None), ("420", "444", 8, 8, None), ("422", "420", 10, 8, None), ("444", "422", 8, 8, (10, 18))]
COLOUR = dict(matrix="bt709", full_range=True, out_matrix="bt601", out_full_range=False)


def tiny(dev):
    z = np.load(os.path.join(ROOT, "tests", "golden", "g_tiny.npz"))
    G = pkg.Generator(types.SimpleNamespace(n_filters=16, n_layers=1), compute_dtype="f32")
    G.load_state_dict({k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("sd.")})
    return G.to(dev).eval()


def forward(dev, hip):
    G = tiny(dev)
    rng = np.random.default_rng(5)
    h, w = 3, 5
    pipe = pkg.InferencePipeline(G, dev, batch=2, depth=2)
    keys = pkg.InferencePipeline(G, dev, batch=2)
    keys._run = lambda frames, fmt: fmt.key       # the key alone: nothing is staged
    for c, oc, d, od, size in FORWARD:
        x = payload(rng, 2, h, w, c, d, dev)
        name = "%s->%s d%d->d%d %s" % (c, oc, d, od, "native" if size is None else "%dx%d" % size)
        kw = dict(chroma=c, out_chroma=oc, depth=d, out_depth=od, out_size=size, **COLOUR)
        line("forward " + name, lambda: G.forward_yuv(x, h, w, **kw))
        print("%-58s %r" % ("pipeline key run_yuv " + name, keys.run_yuv([], h, w, **kw)))
        if (c, oc) == ("420", "420"):
            kw420 = dict(depth=d, out_depth=od, out_size=size, **COLOUR)
            line("forward420 " + name, lambda: G.forward_yuv420(x, h, w, **kw420))
            print("%-58s %r" % ("pipeline key run_yuv420 " + name, keys.run_yuv420([], h, w, **kw420)))
        if hip:   # two full batches through the graphs and a ragged tail
            frames = list(payload(np.random.default_rng(6), 5, h, w, c, d, "cpu").numpy())
            line("pipeline frames " + name, lambda: torch.from_numpy(np.stack(list(pipe.run_yuv(frames, h, w, **kw)))))
    if hip:
        print("pipeline plans %r" % (list(pipe._plans),))


def refusals(dev):
    """The five YUV entry points with one bad argument at a time: nothing is launched, the message is the listing."""
    lib = L.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
    img = torch.zeros(1024, dtype=torch.float32, device=dev)
    p, q = buf.data_ptr(), img.data_ptr()

    def say(name, rc):
        print("%-58s %d %s" % ("refusal " + name, rc, lib.fsr_last_error().decode() if rc < 0 else "accepted"))

    good = dict(n=1, h=4, w=6, chroma=L.CHROMA_444, siting=0, matrix=0, full=0, depth=8)
    for bad in (dict(chroma=3), dict(depth=7), dict(depth=17), dict(n=0), dict(siting=2), dict(matrix=2), dict(full=2),
                dict(h=65536, w=32768), dict(n=2, h=32768, w=32768), dict(chroma=L.CHROMA_420, n=2, h=32768, w=32768, matrix=2),
                dict(chroma=L.CHROMA_420, siting=2), dict(chroma=L.CHROMA_422, siting=2), dict(chroma=L.CHROMA_420, h=65536, w=32768),
                dict(depth=10, odd=1), dict(chroma=L.CHROMA_420, depth=10, odd=1), dict(misaligned=2), dict(null=1)):
        a = dict(good, **bad)
        src = None if a.get("null") else p + a.get("odd", 0)
        say("yuv_to_image %r" % (bad,), lib.fsr_yuv_to_image(src, q + a.get("misaligned", 0), a["n"], a["h"], a["w"], a["chroma"], a["siting"],
                                                               a["matrix"], a["full"], a["depth"], None))
        say("image_to_yuv %r" % (bad,), lib.fsr_image_to_yuv(None if a.get("null") else q + a.get("misaligned", 0), a["n"], a["h"], a["w"],
                                                               a["chroma"], a["matrix"], a["full"], a["depth"], p + a.get("odd", 0), None))
        if a["chroma"] == L.CHROMA_420:
            say("i420_to_image %r" % (bad,), lib.fsr_i420_to_image(src, q, a["n"], a["h"], a["w"], a["siting"], a["matrix"], a["full"], None))
            say("i420_to_image_deep %r" % (bad,), lib.fsr_i420_to_image_deep(src, q, a["n"], a["h"], a["w"], a["siting"], a["matrix"], a["full"],
                                                                             a["depth"], None))
            say("image_to_i420 %r" % (bad,), lib.fsr_image_to_i420(q, a["n"], a["h"], a["w"], a["matrix"], a["full"], a["depth"],
                                                                     p + a.get("odd", 0), None))
    for chroma, h, w in ((L.CHROMA_420, 5, 6), (L.CHROMA_420, 4, 7), (L.CHROMA_422, 4, 7), (L.CHROMA_422, 5, 6), (L.CHROMA_444, 5, 7)):
        say("image_to_yuv extents %d %dx%d" % (chroma, h, w), lib.fsr_image_to_yuv(q, 1, h, w, chroma, 0, 0, 8, p, None))
    say("image_to_i420 extents 5x6", lib.fsr_image_to_i420(q, 1, 5, 6, 0, 0, 8, p, None))
    # the resampler's share of the same rules (identity taps of a 4 x 6 frame)
    t = tanh_like(3, 1, 4, 6, dev)
    wy, ymin, ysize, ky = ops.aa_taps(4, 4, dev)
    wx, xmin, xsize, kx = ops.aa_taps(6, 6, dev)
    taps = (wy.data_ptr(), ymin.data_ptr(), ysize.data_ptr(), ky, wx.data_ptr(), xmin.data_ptr(), xsize.data_ptr(), kx)
    for bad in (dict(chroma=3), dict(depth=7), dict(depth=10, odd=1), dict(matrix=2), dict(chroma=L.CHROMA_422, ow=5),
                dict(chroma=L.CHROMA_420, oh=3), dict(chroma=L.CHROMA_420, ow=5), dict(oh=0)):
        a = dict(good, oh=4, ow=6)
        a.update(bad)
        say("resample_image_yuv %r" % (bad,), lib.fsr_resample_image_yuv(t.data_ptr(), 1, 4, 6, a["oh"], a["ow"], *taps, a["chroma"], a["matrix"],
                                                                         a["full"], a["depth"], p + a.get("odd", 0), None))
    say("resample_image i420 odd", lib.fsr_resample_image(t.data_ptr(), 1, 4, 6, 3, 6, *taps, L.OUT_I420, 0, 0, p, None))
    say("resample_image i420 matrix", lib.fsr_resample_image(t.data_ptr(), 1, 4, 6, 4, 6, *taps, L.OUT_I420, 2, 0, p, None))
    say("resample_image kind", lib.fsr_resample_image(t.data_ptr(), 1, 4, 6, 4, 6, *taps, 7, 0, 0, p, None))
    say("resample_image_i420_deep depth", lib.fsr_resample_image_i420_deep(t.data_ptr(), 1, 4, 6, 4, 6, *taps, 0, 0, 8, p, None))
    say("resample_image_i420_deep odd", lib.fsr_resample_image_i420_deep(t.data_ptr(), 1, 4, 6, 3, 6, *taps, 0, 0, 10, p, None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=("emu", "hip"), required=True,
                    help="emu: the kernel sources compiled for the host (tests/emu); hip: libfsr_hip.so on cuda:0")
    args = ap.parse_args()
    hip = args.backend == "hip"
    if hip:
        if not torch.cuda.is_available():
            raise SystemExit("video_digest --backend hip needs the MI355X")
        dev = torch.device("cuda:0")
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
        from build_emu import build_emu
        L._install_for_testing(build_emu())
        dev = torch.device("cpu")
    L.lib().fsr_last_error.restype = ctypes.c_char_p
    print("# video digests, backend %s" % args.backend)
    decode(dev)
    encode(dev)
    resample(dev)
    forward(dev, hip)
    refusals(dev)


if __name__ == "__main__":
    main()
