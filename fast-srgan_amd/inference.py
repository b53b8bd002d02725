"""`python inference.py --image_dir D --output_dir O`: drop-in for /root/reference/inference.py.

Reads configs/config.yaml and models/model.pt relative to the working directory (inference.py:26-27), strips
the `_orig_mod.` prefix torch.compile left in the shipped checkpoint (:31-33), accepts .png/.jpg/jpeg in any
case (:37-45), writes each result under the same basename (:57) and converts with the reference's
TRUNCATING uint8 cast (:53-56) -- in the head kernel's epilogue.  Frames travel as bytes in both directions and are
batched and pipelined (InferencePipeline); decoding / encoding runs in worker threads.
"""
import math
import os
import sys
from argparse import ArgumentParser

import numpy as np
import torch

from .config import load_config
from .model import Generator
from .ops import check_depth, layout_code, yuv_frame_bytes

parser = ArgumentParser("Real Time Image Super Resolution")
parser.add_argument("--image_dir", default=None, required=True, type=str)
parser.add_argument("--output_dir", default=None, required=True, type=str)
parser.add_argument("--compute_dtype", default=None, choices=["bf16", "f16", "x3", "x3v", "f32"], help="extension: kernel precision")
parser.add_argument("--batch", default=8, type=int, help="extension: frames per device batch (same-shape frames are batched)")
parser.add_argument("--bands", default="auto", choices=["auto", "on", "off"],
                    help="extension: run the generator's tail in row bands -- auto: for frames too large otherwise (above 1080p); on: whenever "
                         "that allows a larger batch; off: never")
parser.add_argument("--band_rows", default=128, type=int, help="extension: core rows per band")
parser.add_argument("--self_ensemble", action="store_true",
                    help="extension: the self-ensemble (\"+\") result -- the mean over the 8 flipped / transposed inputs, 8x the generator work")
_size_flags = parser.add_mutually_exclusive_group()
_size_flags.add_argument("--size", default=None, type=str, metavar="WxH", help="extension: exact output size (default: 4x the input)")
_size_flags.add_argument("--scale", default=None, type=float, help="extension: output size relative to the INPUT, e.g. 2 or 1.5")


def resolve_out_size(h, w, size=None, scale=None, even=False):
    """The (out_h, out_w) that `--size WxH` / `--scale S` ask for on an h x w input, or None when neither is given (the
    network's native size).  `--size` is exact and puts the WIDTH first -- the only place that does; `--scale` is relative to
    the input: round(S h) x round(S w), halves rounding up.  even (video: 4:2:0 chroma needs even extents): `--scale` results
    are rounded to the nearest even number instead, and an odd `--size` is refused."""
    if size is not None and scale is not None:
        raise ValueError("--size and --scale are mutually exclusive")
    if size is not None:
        parts = str(size).lower().split("x")
        if len(parts) != 2 or not all(p.strip().isdigit() for p in parts):
            raise ValueError("--size must be WxH, e.g. 1920x1080, got %r" % (size,))
        ow, oh = int(parts[0]), int(parts[1])
        if ow <= 0 or oh <= 0:
            raise ValueError("--size must be positive, got %r" % (size,))
        if even and (ow % 2 or oh % 2):
            raise ValueError("--size %dx%d is odd: a YUV 4:2:0 frame holds one chroma sample per 2x2 block of pixels, so the output "
                             "width and height must be even" % (ow, oh))
        return oh, ow
    if scale is not None:
        scale = float(scale)
        if not scale > 0.0 or scale != scale or scale == float("inf"):
            raise ValueError("--scale must be a positive number, got %r" % (scale,))
        if even:
            return tuple(max(2, 2 * int(math.floor(scale * d / 2.0 + 0.5))) for d in (h, w))
        return tuple(max(1, int(math.floor(scale * d + 0.5))) for d in (h, w))
    return None


def load_generator(config, model_path, device="cuda", compute_dtype=None):
    model = Generator(config.generator, compute_dtype=compute_dtype or getattr(config.training, "compute_dtype", "f16"))
    weights = torch.load(model_path, map_location="cpu")
    model.load_state_dict({k.replace("_orig_mod.", ""): v for k, v in weights.items()})
    return model.to(device).eval()


@torch.no_grad()
def super_resolve(model, lr_u8_hwc, device="cuda", out_size=None):
    """uint8 (H,W,3) -> uint8 (4H,4W,3), inference.py:48-56, one frame: bytes up, bytes down; the [-1,1] mapping and the
    (y+1)/2*255 truncating cast run on the device (Generator.forward_u8).  out_size = (out_h, out_w): that size instead."""
    frame = torch.from_numpy(np.ascontiguousarray(lr_u8_hwc)).unsqueeze(0).to(device)
    return model.forward_u8(frame, out_size=out_size)[0].cpu().numpy()


class InferencePipeline:
    """Batched, pipelined super-resolution of a stream of frames (replaces the per-image loop of
    inference.py:47-57).

      host thread   : packs `batch` uint8 frames into a pinned staging buffer
      compute stream: H2D of the bytes (0.17 MB per 180x320 frame) -> ONE hipGraph replay per batch (u8 -> [-1,1],
                      generator, head epilogue storing the uint8 frame)
      copy stream   : D2H of the finished uint8 frames (2.8 MB per 720p frame, 4x less than floats) into pinned memory,
                      overlapped with the next batch's compute (`depth` staging slots, each with its own graph)
    Frames are bucketed by shape; one set of graphs per (H, W), built lazily and kept for the most recently used shapes
    only.  `run` yields results in input order.
    Video: `run_yuv` takes planar YUV payloads (4:2:0, 4:2:2 or 4:4:4 in and out, Generator.forward_yuv) through the same staging,
    slots and streams; its plans are keyed ("i420", H, W, colour parameters), never colliding with the RGB plans' (H, W).
    `run_yuv420` is the same under its I420 name.
    Output size: every run method takes out_size = (out_h, out_w) (Generator.forward_u8 / forward_yuv: the fused resize
    after the head, captured in the same graph).  Plans of a resized output append ("size", out_h, out_w) to the key of the
    native plan, so both coexist; None or the native size IS the native plan.
    Row bands: bands="auto" runs the generator's tail in bands of `band_rows` core rows for the shapes that cannot run
    otherwise (max_batch(h, w) == 0: above 1080p for the shipped model), "on" for every shape whose batch that enlarges, "off" (the
    default) never.  The frames are the same bytes; banded plans append ("bands", band_rows) to their key.
    Self-ensemble: ensemble=True makes `run` and `run_mixed` yield Generator.forward_u8(..., ensemble=True)'s frames;
    such plans append ("ensemble",) to their key and hold a quarter of the frames per batch (`_member_limit`).  The YUV methods do not
    take it."""

    def __init__(self, model, device="cuda", batch=8, depth=2, use_graph=True, copy=True, max_shapes=4, bands="off", band_rows=128,
                 ensemble=False):
        """copy=False: `run` yields VIEWS of the pinned result buffers (valid until `depth` more batches have been
        submitted) instead of private arrays -- for consumers that encode / display a frame right away.
        max_shapes: plans (pinned staging, device buffers, captured graphs with their private pools) are kept for the
        `max_shapes` most recently used frame shapes only; a directory of differently sized images (which the reference's
        per-image loop handles, inference.py:47-57) would otherwise pin a few GB per distinct shape for good."""
        self.model, self.device, self.batch, self.depth, self.use_graph = model.eval(), torch.device(device), batch, depth, use_graph
        self.copy = copy
        if bands not in ("auto", "on", "off"):
            raise ValueError("bands must be 'auto', 'on' or 'off', got %r" % (bands,))
        if isinstance(band_rows, bool) or int(band_rows) != band_rows or band_rows < 1:
            raise ValueError("band_rows must be a positive integer, got %r" % (band_rows,))
        self.bands, self.band_rows = bands, int(band_rows)
        self.ensemble = bool(ensemble)
        self.max_shapes = max(1, int(max_shapes))
        self._plans = {}            # (h, w) -> list of `depth` slots, built lazily (a one-batch bucket only ever builds slot 0)
        self._lru = []              # shapes, least recently used first
        self._copy_stream = None    # the D2H stream, created with the first batch
        self._told = set()          # frame shapes whose reduced batch has been reported

    def _batch_for(self, h, w):
        """Frames per device batch for h x w inputs: min(batch, Generator.max_batch(h, w)) -- the convolution kernels index tensors
        below 2^31 elements, and InstanceNorm statistics are per image, so a smaller batch computes the same frames.  A frame
        that is too large on its own is refused here, before anything is allocated."""
        limit = self.model.max_batch(h, w) if hasattr(self.model, "max_batch") else self.batch
        if self._bands_for(h, w, limit) is not None:
            limit = self._member_limit(self.model.max_batch(h, w, bands=True))
            if limit < 1:
                px = self.model.max_batch(1, 1, bands=True)
                raise ValueError("frames of %dx%d are too large: even with the tail in row bands a frame's largest activation would hold "
                                 "2^31 or more elements, the limit of the convolution kernels (max_batch = 0; the limit is %d input "
                                 "pixels per frame, %.1f M)" % (w, h, px, px / 1e6))
            b = min(self.batch, limit)
            if (h, w) not in self._told:
                self._told.add((h, w))
                print("InferencePipeline: %dx%d frames run banded (the generator's tail in bands of %d rows), in batches of %d"
                      % (w, h, self.band_rows, b), file=sys.stderr)
            return b
        if limit < 1:
            raise ValueError("frames of %dx%d are too large: one frame's largest activation would hold 2^31 or more elements, the limit "
                             "of the convolution kernels (max_batch = 0; 1920x1080 is the largest 16:9 input)" % (w, h))
        limit = self._member_limit(limit)
        b = min(self.batch, limit)
        if b < self.batch and (h, w) not in self._told:
            self._told.add((h, w))
            print("InferencePipeline: %dx%d frames run in batches of %d instead of %d (the kernels index tensors below 2^31 elements)"
                  % (w, h, b, self.batch), file=sys.stderr)
        return b

    def _member_limit(self, limit):
        """The frame limit of a self-ensemble plan: a forward there runs the 4 members of an orientation group of every frame as one
        batch, so a quarter of the kernels' limit keeps the groups whole.  Below 4 the limit stays -- forward_u8 then
        runs the members in chunks, which changes no byte."""
        return limit // 4 if self.ensemble and limit >= 4 else limit

    def _bands_for(self, h, w, whole=None):
        """Core rows per band for h x w inputs, or None when the shape runs whole: "auto" bands a shape that cannot run otherwise,
        "on" every shape whose whole-frame limit is below the batch asked for."""
        if self.bands == "off" or not hasattr(self.model, "max_batch") or not len(self.model.upsampling):
            return None
        if whole is None:
            whole = self.model.max_batch(h, w)
        return self.band_rows if whole < (1 if self.bands == "auto" else self.batch) else None

    class _Slot:
        pass

    def _touch(self, key):
        if key in self._lru:
            self._lru.remove(key)
        self._lru.append(key)
        while len(self._lru) > self.max_shapes:
            old = self._lru.pop(0)
            plan = self._plans.pop(old, None)
            if plan is not None:
                for sl in plan:
                    if sl is not None and sl.pending is not None:
                        sl.copied.synchronize()
                del plan            # graphs (and their private memory pools), device and pinned buffers go with the slots
                torch.cuda.synchronize(self.device)
                torch.cuda.empty_cache()

    def _slot(self, fmt, j):
        """Slot j of the plan for the frame format `fmt` (_Format), created on first use."""
        key = fmt.key
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = [None] * self.depth
        self._touch(key)
        if plan[j] is not None:
            return plan[j]
        sl = self._Slot()
        sl.host_in = torch.empty((fmt.batch,) + fmt.shape, dtype=torch.uint8).pin_memory()
        sl.x = torch.zeros((fmt.batch,) + fmt.shape, dtype=torch.uint8, device=self.device)
        sl.fwd = fmt.fwd
        with torch.no_grad():
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                y = fmt.fwd(sl.x)                          # warm-up: creates every lazily allocated buffer
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            sl.graph = None
            if self.use_graph:
                try:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        y = fmt.fwd(sl.x)
                    sl.graph = g
                except Exception as exc:  # noqa: BLE001 -- eager launches are always available
                    print("InferencePipeline: hipGraph capture failed (%s: %s); eager launches" % (type(exc).__name__, exc),
                          file=sys.stderr)   # (stdout may be the video stream: video.py --output -)
                    torch.cuda.synchronize()
        sl.y = y
        sl.host_out = torch.empty(tuple(y.shape), dtype=torch.uint8).pin_memory()
        # plain numpy views for the host-side packing / unpacking: one memcpy per frame on this thread (torch's
        # multi-threaded copy_ pays a thread-pool wake-up per call, milliseconds when the pool has gone to sleep)
        sl.host_in_np, sl.host_out_np = sl.host_in.numpy(), sl.host_out.numpy()
        sl.done = torch.cuda.Event()
        sl.copied = torch.cuda.Event()
        sl.pending = None
        plan[j] = sl
        return sl

    @torch.no_grad()
    def _eager(self, fmt, frames):
        """A handful of frames of one shape (fewer than a batch): one eager launch at their TRUE count -- no staging plan, no
        graph capture, no padding of the batch with repeated frames."""
        x = torch.from_numpy(np.stack([np.ascontiguousarray(f).reshape(fmt.shape) for f in frames])).to(self.device)
        y = fmt.fwd(x).cpu().numpy()
        return [y[i] for i in range(len(frames))]

    @torch.no_grad()
    def _submit(self, sl, frames):
        """Enqueue one batch on slot `sl` (its previous results have been collected): nothing here waits for the device."""
        n = len(frames)
        for i, f in enumerate(frames):
            np.copyto(sl.host_in_np[i], np.asarray(f).reshape(sl.host_in_np.shape[1:]))
        assert n == sl.x.shape[0]    # (ragged tails run eagerly: InferencePipeline.run)
        main = torch.cuda.current_stream()
        sl.x.copy_(sl.host_in, non_blocking=True)
        if sl.graph is not None:
            sl.graph.replay()
        else:
            sl.y = sl.fwd(sl.x)
        sl.done.record(main)
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(sl.done)
            sl.host_out.copy_(sl.y, non_blocking=True)
            sl.copied.record(self._copy_stream)
        # (a slot is resubmitted only after _collect has waited for `copied`: its y is never overwritten early)
        sl.pending = n

    def _collect(self, sl):
        sl.copied.synchronize()
        out = [sl.host_out_np[i].copy() if self.copy else sl.host_out_np[i] for i in range(sl.pending)]
        sl.pending = None
        return out

    class _Format:
        """What a plan is built for: its key in `_plans`, the shape of one input frame, the device forward of a batch, and the
        frames per batch (InferencePipeline._batch_for)."""

        def __init__(self, key, shape, fwd, batch):
            self.key, self.shape, self.fwd, self.batch = key, shape, fwd, batch

    def _out_size(self, h, w, out_size):
        """out_size normalised: None for the network's native size of an h x w input, else (out_h, out_w) as ints."""
        if out_size is None:
            return None
        oh, ow = int(out_size[0]), int(out_size[1])
        s = 2 ** len(self.model.upsampling)
        return None if (oh, ow) == (s * h, s * w) else (oh, ow)

    def run(self, frames, out_size=None):
        """frames: iterable of uint8 (H,W,3) arrays, all of ONE shape per call (use `run_mixed` otherwise).  Yields uint8
        (4H,4W,3) arrays -- (out_h, out_w, 3) with out_size = (out_h, out_w) -- in order.  Full batches go through the pipelined
        slots; a ragged tail runs eagerly at its true size."""
        return self._run(frames, None, out_size)

    def run_yuv(self, frames, h, w, chroma="420", out_chroma=None, siting=None, matrix="bt601", full_range=False, out_matrix=None,
                out_full_range=None, out_size=None, depth=8, out_depth=None, layout="planar", out_layout=None):
        """frames: iterable of planar YUV payloads of h x w (uint8 arrays or bytes of ops.yuv_frame_bytes(h, w, chroma, depth) each).
        Yields the uint8 payloads of the super-resolved frames, of out_chroma (default: chroma) at out_depth (Generator.forward_yuv with
        these colour parameters), in order, batched and pipelined exactly as `run`.  siting=None: "mpeg2" for 4:2:2, "jpeg" otherwise.
        out_size = (out_h, out_w): payloads of that size.  depth / out_depth (8..16, out_depth defaults to depth): bits per sample in and
        out; payloads deeper than 8 bits are 2 bytes per sample and still travel as uint8 arrays.
        Plan keys: ("i420", h, w, colour parameters), then ("size", out_h, out_w) for a resized output, ("depth", depth, out_depth) for any
        pair but (8, 8), ("chroma", chroma, out_chroma) for any pair but ("420", "420"), ("layout", layout, out_layout) for any pair but
        ("planar", "planar") and ("bands", band_rows) for a banded plan.
        layout / out_layout ("planar" or "nv12"; out_layout defaults to layout): semi-planar 4:2:0 payloads in / out."""
        if self.ensemble:
            raise ValueError("InferencePipeline(ensemble=True) serves RGB frames only (run, run_mixed): the YUV paths have no self-ensemble")
        out_chroma = chroma if out_chroma is None else out_chroma
        out_layout = layout if out_layout is None else out_layout
        layout_code(layout, chroma)
        layout_code(out_layout, out_chroma)
        if siting is None:
            siting = "mpeg2" if chroma == "422" else "jpeg"
        colour = dict(siting=siting, matrix=matrix, full_range=bool(full_range), out_matrix=out_matrix or matrix,
                      out_full_range=bool(full_range if out_full_range is None else out_full_range))
        model = self.model
        depth = check_depth(depth)
        out_depth = depth if out_depth is None else check_depth(out_depth)
        out_size = self._out_size(h, w, out_size)
        key = ("i420", h, w) + tuple(colour.values()) + (() if out_size is None else ("size",) + out_size)
        if (depth, out_depth) != (8, 8):
            key += ("depth", depth, out_depth)
        if (chroma, out_chroma) != ("420", "420"):
            key += ("chroma", chroma, out_chroma)
        if (layout, out_layout) != ("planar", "planar"):
            key += ("layout", layout, out_layout)
        batch, rows = self._batch_for(h, w), self._bands_for(h, w)
        if rows is not None:
            key += ("bands", rows)
        fmt = self._Format(key, (yuv_frame_bytes(h, w, chroma, depth),),
                           lambda x: model.forward_yuv(x, h, w, chroma=chroma, out_chroma=out_chroma, out_size=out_size, depth=depth,
                                                       out_depth=out_depth, bands=rows, layout=layout, out_layout=out_layout, **colour),
                           batch)
        return self._run((np.frombuffer(f, dtype=np.uint8) if isinstance(f, (bytes, bytearray, memoryview)) else f
                          for f in frames), fmt)

    def run_yuv420(self, frames, h, w, siting="jpeg", matrix="bt601", full_range=False, out_matrix=None, out_full_range=None,
                   out_size=None, depth=8, out_depth=None):
        """run_yuv for I420 payloads in and out."""
        return self.run_yuv(frames, h, w, "420", "420", siting, matrix, full_range, out_matrix, out_full_range, out_size, depth, out_depth)

    def _run(self, frames, fmt, out_size=None):
        it = iter(frames)
        k, inflight = 0, []
        first = None
        if fmt is None:                           # RGB frames: plans keyed by (H, W); the first frame says which
            first = next(it, None)
            if first is None:
                return
            h, w = first.shape[0], first.shape[1]
            size = self._out_size(h, w, out_size)
            batch, rows = self._batch_for(h, w), self._bands_for(h, w)
            key = (h, w) if size is None else (h, w, "size") + size
            if self.ensemble:       # self-ensemble plans append ("ensemble",): both kinds coexist
                key += ("ensemble",) if rows is None else ("ensemble", "bands", rows)
                fmt = self._Format(key, (h, w, 3),
                                   lambda x, m=self.model, sz=size, r=rows: m.forward_u8(x, out_size=sz, bands=r, ensemble=True), batch)
            elif rows is not None:
                fmt = self._Format(key + ("bands", rows), (h, w, 3),
                                   lambda x, m=self.model, sz=size, r=rows: m.forward_u8(x, out_size=sz, bands=r), batch)
            elif size is None:
                fmt = self._Format(key, (h, w, 3), self.model.forward_u8, batch)
            else:
                fmt = self._Format(key, (h, w, 3), lambda x, m=self.model, sz=size: m.forward_u8(x, out_size=sz), batch)
        batch = fmt.batch
        while True:
            chunk = [] if first is None else [first]
            first = None
            if len(chunk) < batch:
                for f in it:
                    chunk.append(f)
                    if len(chunk) == batch:
                        break
            if not chunk:
                break
            if len(chunk) < batch:                # the tail (or a bucket smaller than one batch)
                for sl in inflight:
                    yield from self._collect(sl)
                inflight = []
                yield from self._eager(fmt, chunk)
                break
            sl = self._slot(fmt, k % self.depth)
            if sl.pending is not None:
                inflight.remove(sl)
                yield from self._collect(sl)
            self._submit(sl, chunk)
            inflight.append(sl)
            k += 1
        for sl in inflight:
            yield from self._collect(sl)

    def run_mixed(self, frames, out_size=None):
        """Frames of any shapes: bucketed by (H, W), results returned as a list in input order.  out_size: (out_h, out_w) for
        every frame, or a function (h, w) -> (out_h, out_w) (or None: native) asked once per input shape."""
        frames = list(frames)
        out = [None] * len(frames)
        buckets = {}
        for i, f in enumerate(frames):
            buckets.setdefault((f.shape[0], f.shape[1]), []).append(i)
        for (h, w), idx in buckets.items():
            size = out_size(h, w) if callable(out_size) else out_size
            for i, y in zip(idx, self.run((frames[j] for j in idx), size)):
                out[i] = y
        return out


def main(argv=None):
    from concurrent.futures import ThreadPoolExecutor

    from PIL import Image
    args = parser.parse_args(argv)
    os.makedirs(args.output_dir, exist_ok=True)
    if not torch.cuda.is_available():
        raise SystemExit("fast-srgan_amd runs on an MI355X only: no GPU is visible")
    device = "cuda"
    print(f"Using device: {device}")
    config = load_config("configs/config.yaml")
    model = load_generator(config, "models/model.pt", device, args.compute_dtype)
    image_paths = sorted(x for x in os.listdir(args.image_dir)
                         if x.lower().endswith(".png") or x.lower().endswith(".jpg") or x.lower().endswith("jpeg"))
    print(f"Found {len(image_paths)} to super resolve, starting...")
    # (reports a batch it has to reduce for large frames, and a size it runs in row bands, once per size)
    pipe = InferencePipeline(model, device, batch=args.batch, bands=args.bands, band_rows=args.band_rows, ensemble=args.self_ensemble)
    resolve_out_size(1, 1, args.size, args.scale)      # a malformed --size fails before any image is read

    def load(name):
        return np.array(Image.open(os.path.join(args.image_dir, name)).convert("RGB"))

    def save(name, arr):
        Image.fromarray(arr).save(os.path.join(args.output_dir, os.path.basename(name)))

    # decode and encode run in worker threads (PIL releases the GIL), the device pipeline in this one
    with ThreadPoolExecutor(max_workers=8) as pool:
        window = 16 * args.batch
        for start in range(0, len(image_paths), window):
            names = image_paths[start:start + window]
            frames = list(pool.map(load, names))
            results = pipe.run_mixed(frames, lambda h, w: resolve_out_size(h, w, args.size, args.scale))
            saves = [pool.submit(save, n, y) for n, y in zip(names, results)]
            for s_ in saves:
                s_.result()


if __name__ == "__main__":
    main()
