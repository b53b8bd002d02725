"""`python video.py --input IN --output OUT`: super-resolution of a YUV4MPEG2 (Y4M) stream of planar YUV frames.

    ffmpeg -i in.mp4 -f yuv4mpegpipe - | python video.py --input - --output - | ffmpeg -i - -c:v libx264 out.mp4

Y4M is the plain container of uncompressed frames that `ffmpeg -f yuv4mpegpipe` reads and writes on pipes, so no codec
library is involved.  Frames stay planar YUV 4:2:0 end to end: the device converts the input to the generator's [-1, 1]
RGB (fsr_i420_to_image) and the head's epilogue stores finished I420 planes (FSR_OUT_I420), so the host only moves bytes
-- 1.5 per output pixel instead of 3.  The colour contract (matrices, ranges, chroma siting) is DESIGN.md §6c.

`--size WxH` (exact, both even) or `--scale S` (relative to the input, rounded to even numbers) pick the output size -- 640x360 to
1080p is `--size 1920x1080` or `--scale 3`; the default is the network's 4x.  The resize is the antialiased bicubic fused with the
I420 encode after the head, inside the same graph replay.

Streams of 9- to 16-bit samples (`C420p10` and its kin: what `ffmpeg -f yuv4mpegpipe` emits for HEVC Main10, AV1 or VP9 profile 2
sources) are read as they are -- 2 bytes per sample, little-endian -- and `--out_depth` picks the depth of the output, the
input's by default: `--out_depth 10` on an 8-bit source keeps the precision of the float head that 256 levels throw away.
`C420pN` cannot declare a chroma siting; `--siting mpeg2` says what the stream cannot (HD sources are normally left-sited).

4:2:2 and 4:4:4 streams (`C422`, `C444`, `C422p10`, `C444p10` ...: mezzanine and camera material, screen captures) are read as they
are, and `--out_chroma {420,422,444}` picks the subsampling of the output, the input's by default: `--out_chroma 444` on a 4:2:0 source
keeps the chroma samples the network has computed, which a 4:2:0 output averages away.  `--size` must be even in both extents for
4:2:0, in the width for 4:2:2, and may be anything for 4:4:4 (an odd `--size` needs `--out_chroma` spelled out: it is checked before the
stream is opened).  A `C422` stream is co-sited horizontally ("mpeg2"); `--siting jpeg` overrides that too.

Frames above 1080p (2560x1440, up to 3840x2160) run with the generator's tail in row bands (`--bands auto`, the default):
the same bytes a whole frame would give, `--band_rows` rows of the last up-sampling stage at a time.  `--bands on` bands smaller frames
too, for a larger batch; `--bands off` refuses what does not fit whole.

Raw streams (`--in_format` / `--out_format`: `yuv420p`, `nv12`, `p010`, `p012`, `p016`; the default is `y4m`) carry no header: what
`ffmpeg -f rawvideo -pix_fmt nv12` writes, and what a hardware decoder hands over (`ffmpeg -hwaccel vaapi ... -pix_fmt nv12` or `p010le`).
A raw input needs `--in_size WxH`; `--fps N[:D]` (default 25:1) is only used for the Y4M header when raw goes to Y4M.  `yuv420p` is 8-bit
planar 4:2:0; `nv12` is the semi-planar 8-bit frame -- Y, then one plane of (Cb, Cr) pairs --, and `p010` / `p012` / `p016` its 16-bit
forms with the code in the HIGH bits of each little-endian word.  The device reads and writes these layouts itself: no
de-interleaving pass on the host.  `--out_format` defaults to the input's kind: `y4m` for a Y4M input, for a raw input the raw format of
the same family at the output depth.  A `p01x` name fixes the depth, so an `--out_depth` that contradicts `--out_format` is an error.
For a raw output the status line prints the ffmpeg arguments that read it.

    ffmpeg -hwaccel vaapi -i in.mp4 -vf hwdownload,format=nv12 -f rawvideo -pix_fmt nv12 - | \
        python video.py --input - --in_format nv12 --in_size 1920x1080 --fps 30000:1001 --output - | ffmpeg -f rawvideo ...

Like inference.py, the CLI loads configs/config.yaml and models/model.pt from the working directory.  `-` is stdin /
stdout; with `--output -` nothing but the stream goes to stdout (status lines go to stderr).  Frames are read lazily, one
device batch at a time: a stream of any length passes through a pipe.
"""
import sys
import time
from argparse import ArgumentParser

import numpy as np

from .ops import check_depth, i420_frame_bytes, yuv_frame_bytes

MATRICES = ("bt601", "bt709")
SITINGS = ("jpeg", "mpeg2")
CHROMAS = ("420", "422", "444")
# stream formats: name -> (layout, depth, ffmpeg's -pix_fmt); "y4m" is the container, the others are headerless 4:2:0 frames
RAW_FORMATS = {"yuv420p": ("planar", 8, "yuv420p"), "nv12": ("nv12", 8, "nv12"), "p010": ("nv12", 10, "p010le"),
               "p012": ("nv12", 12, "p012le"), "p016": ("nv12", 16, "p016le")}
FORMATS = ("y4m",) + tuple(RAW_FORMATS)


class Y4MError(ValueError):
    pass


# colour-space tags (`C...`) this reader takes, and the chroma siting each declares; a missing tag means C420jpeg
_ACCEPTED_C = {"420jpeg": "jpeg", "420": "jpeg", "420mpeg2": "mpeg2"}
_REJECTED_C = ("420paldv", "411", "422", "444", "444alpha", "mono")


class Y4MReader:
    """Streaming reader: parses the stream header on construction, then `frames()` yields one uint8 payload
    (yuv_frame_bytes(height, width, chroma, depth) bytes, a numpy array) per FRAME, reading only that frame from the file.
    max_depth: the deepest samples the caller takes.  The default, 8, refuses `C420pN` streams: their payloads are 16-bit
    little-endian samples, which a caller that indexes bytes must not be handed silently.  With max_depth >= 9, `C420pN` for
    9 <= N <= max_depth is accepted (`.depth` = N, `.frame_bytes` twice the sample count; siting "jpeg": the tag declares none).
    chroma: the subsamplings the caller takes.  The default, ("420",), refuses `C422` / `C444` and their `pN` forms by the same rule: a
    caller that indexes planes must not be handed another layout silently.  With "422" / "444" in it, `C422`, `C444` and (up to
    max_depth) `C422pN` / `C444pN` are accepted: `.chroma` says which, `.siting` is "mpeg2" for 4:2:2 (horizontally co-sited: what the
    tag means; 4:4:4 has no siting, "jpeg" stands in)."""

    def __init__(self, f, max_depth=8, chroma=("420",)):
        self.f = f
        self.max_depth = check_depth(max_depth)
        self.takes_chroma = tuple(chroma)
        for c in self.takes_chroma:
            if c not in CHROMAS:
                raise ValueError("Y4MReader: chroma must be a tuple of %s, got %r" % (", ".join(CHROMAS), chroma))
        self.depth = 8
        self.chroma = "420"
        line = f.readline()
        if not line.startswith(b"YUV4MPEG2"):
            raise Y4MError("Y4M: the stream does not start with the YUV4MPEG2 signature")
        if not line.endswith(b"\n"):
            raise Y4MError("Y4M: the stream header is not terminated")
        self.width = self.height = None
        self.frame_rate = self.aspect = self.interlace = None
        self.siting = "jpeg"
        self.colour_range = None          # XCOLORRANGE: "full" / "limited", or None when the stream does not say
        self.x_tags = []
        for tok in line[len(b"YUV4MPEG2"):].decode("ascii", "replace").split():
            key, val = tok[0], tok[1:]
            if key == "W":
                self.width = int(val)
            elif key == "H":
                self.height = int(val)
            elif key == "F":
                self.frame_rate = val
            elif key == "A":
                self.aspect = val
            elif key == "I":
                if val in ("t", "b", "m"):
                    raise Y4MError("Y4M: interlaced streams are not supported (tag 'I%s'); deinterlace first" % val)
                self.interlace = val
            elif key == "C":
                self.siting = self._colour_space(val)
            elif key == "X":
                self.x_tags.append(val)
                if val.upper().startswith("COLORRANGE="):
                    r = val.split("=", 1)[1].upper()
                    if r not in ("FULL", "LIMITED"):
                        raise Y4MError("Y4M: unknown tag value 'X%s' (XCOLORRANGE is FULL or LIMITED)" % val)
                    self.colour_range = r.lower()
        if not self.width or not self.height or self.width <= 0 or self.height <= 0:
            raise Y4MError("Y4M: the stream header lacks the frame size (tags 'W' and 'H')")
        self.frame_bytes = yuv_frame_bytes(self.height, self.width, self.chroma, self.depth)

    def _colour_space(self, val):
        takes = "4:2:0 8-bit only: C420jpeg, C420mpeg2" if self.max_depth == 8 else \
            "4:2:0 only: C420jpeg, C420mpeg2, C420p9..C420p%d" % self.max_depth
        more = [c for c in ("422", "444") if c in self.takes_chroma]
        if more:      # (the default reader's messages stay as they were)
            takes = "C420jpeg, C420mpeg2, %s%s" % (", ".join("C" + c for c in more), "" if self.max_depth == 8 else
                                                   "; C420p9..C420p%d and the like" % self.max_depth)
        if val in _ACCEPTED_C:
            self.depth = 8
            return _ACCEPTED_C[val]
        base, bits = val[:3], val[3:]
        if base in ("422", "444") and base in self.takes_chroma and (bits == "" or (bits[0] == "p" and bits[1:].isdigit())):
            if bits and self.max_depth == 8:
                raise Y4MError("Y4M: colour space 'C%s' is deeper than 8 bits (this reader takes 8-bit samples only)" % val)
            if bits and not 9 <= int(bits[1:]) <= self.max_depth:
                raise Y4MError("Y4M: colour space 'C%s': %s bits per sample are outside what this reader takes (9..%d)"
                               % (val, bits[1:], self.max_depth))
            self.depth = int(bits[1:]) if bits else 8
            self.chroma = base
            return "mpeg2" if base == "422" else "jpeg"
        if val in _REJECTED_C:
            raise Y4MError("Y4M: colour space 'C%s' is not supported (%s)" % (val, takes))
        if "p" in val and val.split("p")[-1].isdigit():
            base, bits = val.rsplit("p", 1)
            if self.max_depth == 8:
                raise Y4MError("Y4M: colour space 'C%s' is deeper than 8 bits (4:2:0 8-bit only)" % val)
            if base != "420":
                raise Y4MError("Y4M: colour space 'C%s' is not supported (%s)" % (val, takes))
            if not 9 <= int(bits) <= self.max_depth:
                raise Y4MError("Y4M: colour space 'C%s': %s bits per sample are outside what this reader takes (9..%d)"
                               % (val, bits, self.max_depth))
            self.depth = int(bits)
            return "jpeg"
        raise Y4MError("Y4M: unknown colour space 'C%s' (%s)" % (val, takes))

    def frames(self):
        idx = 0
        while True:
            line = self.f.readline()
            if not line:
                return
            if not line.startswith(b"FRAME") or not line.endswith(b"\n"):
                raise Y4MError("Y4M: frame %d does not start with a FRAME line" % idx)
            buf = bytearray(self.frame_bytes)
            view, got = memoryview(buf), 0
            while got < self.frame_bytes:
                k = self.f.readinto(view[got:])
                if not k:
                    raise Y4MError("Y4M: frame %d is truncated (%d of %d bytes)" % (idx, got, self.frame_bytes))
                got += k
            yield np.frombuffer(buf, dtype=np.uint8)
            idx += 1


class Y4MWriter:
    """Writes the stream header on construction (C420jpeg, or C420p<depth> for samples deeper than 8 bits; chroma "422" / "444":
    C422, C444, C422p<depth>, C444p<depth>; XCOLORRANGE of the output range), then one FRAME per payload."""

    def __init__(self, f, width, height, frame_rate=None, aspect=None, interlace=None, full_range=False, depth=8, chroma="420"):
        self.f = f
        self.depth = check_depth(depth)
        if chroma not in CHROMAS:
            raise ValueError("Y4MWriter: chroma must be one of %s, got %r" % (", ".join(CHROMAS), chroma))
        self.chroma = chroma
        self.frame_bytes = yuv_frame_bytes(height, width, chroma, self.depth)
        tags = ["W%d" % width, "H%d" % height]
        if frame_rate is not None:
            tags.append("F" + frame_rate)
        if interlace is not None:
            tags.append("I" + interlace)
        if aspect is not None:
            tags.append("A" + aspect)
        ctag = ("C420jpeg" if chroma == "420" else "C" + chroma) if self.depth == 8 else "C%sp%d" % (chroma, self.depth)
        tags += [ctag, "XCOLORRANGE=" + ("FULL" if full_range else "LIMITED")]
        f.write(("YUV4MPEG2 " + " ".join(tags) + "\n").encode("ascii"))

    def write_frame(self, payload):
        payload = memoryview(np.ascontiguousarray(payload)).cast("B")
        if payload.nbytes != self.frame_bytes:
            raise Y4MError("Y4M: a frame of %d bytes does not match the stream's %d" % (payload.nbytes, self.frame_bytes))
        self.f.write(b"FRAME\n")
        self.f.write(payload)


class RawReader:
    """Headerless frames of `frame_bytes` bytes each (the caller knows the format: --in_format / --in_size): `frames()` yields one uint8
    payload per frame, reading only that frame from the file.  A truncated last frame is an error, as in Y4MReader."""

    def __init__(self, f, width, height, frame_bytes):
        if width <= 0 or height <= 0 or frame_bytes <= 0:
            raise ValueError("RawReader: bad frame size %dx%d (%d bytes)" % (width, height, frame_bytes))
        self.f, self.width, self.height, self.frame_bytes = f, int(width), int(height), int(frame_bytes)

    def frames(self):
        idx = 0
        while True:
            buf = bytearray(self.frame_bytes)
            view, got = memoryview(buf), 0
            while got < self.frame_bytes:
                k = self.f.readinto(view[got:])
                if not k:
                    if got == 0:
                        return
                    raise Y4MError("raw stream: frame %d is truncated (%d of %d bytes)" % (idx, got, self.frame_bytes))
                got += k
            yield np.frombuffer(buf, dtype=np.uint8)
            idx += 1


class RawWriter:
    """One payload of `frame_bytes` bytes per frame, nothing else."""

    def __init__(self, f, width, height, frame_bytes):
        self.f, self.width, self.height, self.frame_bytes = f, int(width), int(height), int(frame_bytes)

    def write_frame(self, payload):
        payload = memoryview(np.ascontiguousarray(payload)).cast("B")
        if payload.nbytes != self.frame_bytes:
            raise Y4MError("raw stream: a frame of %d bytes does not match the stream's %d" % (payload.nbytes, self.frame_bytes))
        self.f.write(payload)


def resolve_formats(in_format, out_format, out_depth, out_chroma, in_depth=None):
    """The (out_format, out_depth) of a run, or ValueError.  in_depth: the input's depth (None before a Y4M stream is opened: then only
    what the flags alone decide is checked).  out_format defaults to the input's kind: "y4m" for Y4M, for a raw input the raw format of
    its family (planar / semi-planar) at the output depth.  A raw name fixes chroma 4:2:0 and its depth."""
    if in_format != "y4m":
        in_depth = RAW_FORMATS[in_format][1]
    depth = out_depth if out_depth is not None else (RAW_FORMATS[out_format][1] if out_format in RAW_FORMATS else in_depth)
    if out_format is None:
        if in_format == "y4m":
            out_format = "y4m"
        elif depth is not None:
            if RAW_FORMATS[in_format][0] == "planar":
                if depth != 8:
                    raise ValueError("--out_depth %d: raw planar output is yuv420p, 8 bits; pick --out_format y4m or p0%d" % (depth, depth))
                out_format = "yuv420p"
            else:
                out_format = {8: "nv12", 10: "p010", 12: "p012", 16: "p016"}.get(depth)
                if out_format is None:
                    raise ValueError("--out_depth %d has no raw semi-planar format (nv12, p010, p012, p016)" % depth)
    if out_format in RAW_FORMATS:
        if depth is not None and depth != RAW_FORMATS[out_format][1]:
            raise ValueError("--out_depth %d contradicts --out_format %s, which is %d bits per sample"
                             % (depth, out_format, RAW_FORMATS[out_format][1]))
        if out_chroma not in (None, "420"):
            raise ValueError("--out_format %s is a 4:2:0 format: --out_chroma %s needs --out_format y4m" % (out_format, out_chroma))
    return out_format, depth


def parse_size(text, flag):
    try:
        w, h = (int(v) for v in text.lower().split("x"))
        if w <= 0 or h <= 0:
            raise ValueError
    except ValueError:
        raise ValueError("%s must be WxH of positive integers, got %r" % (flag, text))
    return w, h


def parse_fps(text):
    n, _, d = text.partition(":")
    try:
        n, d = int(n), int(d or 1)
        if n <= 0 or d <= 0:
            raise ValueError
    except ValueError:
        raise ValueError("--fps must be N or N:D of positive integers, got %r" % text)
    return "%d:%d" % (n, d)


parser = ArgumentParser("Real Time Video Super Resolution (Y4M, planar YUV)")
parser.add_argument("--input", required=True, type=str, help="Y4M (or raw, --in_format) stream, or - for stdin")
parser.add_argument("--output", required=True, type=str, help="Y4M (or raw, --out_format) stream, or - for stdout")
parser.add_argument("--in_format", default="y4m", choices=FORMATS,
                    help="y4m, or headerless 4:2:0 frames: yuv420p (8-bit planar), nv12 (8-bit semi-planar), p010 / p012 / p016 (16-bit "
                         "semi-planar, the code in the high bits); raw formats need --in_size")
parser.add_argument("--out_format", default=None, choices=FORMATS,
                    help="format of the output (default: the input's kind -- y4m for Y4M, the raw format of the same family at the output depth)")
parser.add_argument("--in_size", default=None, type=str, metavar="WxH", help="frame size of a raw input")
parser.add_argument("--fps", default=None, type=str, metavar="N[:D]", help="frame rate of a raw input, for the Y4M header (default 25:1)")
parser.add_argument("--compute_dtype", default=None, choices=["bf16", "f16", "x3", "x3v", "f32"], help="kernel precision")
parser.add_argument("--batch", default=8, type=int, help="frames per device batch")
parser.add_argument("--matrix", default="bt601", choices=MATRICES, help="colour matrix of the input")
parser.add_argument("--range", default="limited", choices=["limited", "full"], help="input range (XCOLORRANGE overrides it)")
parser.add_argument("--out_matrix", default=None, choices=MATRICES, help="colour matrix of the output (default: the input's)")
parser.add_argument("--out_range", default=None, choices=["limited", "full"], help="output range (default: the input's)")
parser.add_argument("--out_depth", default=None, type=int, choices=[8, 10, 12, 16], help="bits per sample of the output (default: the input's)")
parser.add_argument("--out_chroma", default=None, choices=CHROMAS, help="chroma subsampling of the output (default: the input's)")
parser.add_argument("--siting", default=None, choices=SITINGS,
                    help="chroma siting of the input, overriding the stream's tag (C420pN streams cannot declare one: jpeg is assumed; "
                         "C422 streams are mpeg2)")
parser.add_argument("--bands", default="auto", choices=["auto", "on", "off"],
                    help="run the generator's tail in row bands -- auto: for frames too large otherwise (above 1080p); on: whenever that "
                         "allows a larger batch; off: never.  The output is the same bytes")
parser.add_argument("--band_rows", default=128, type=int, help="core rows per band")
_size_flags = parser.add_mutually_exclusive_group()
_size_flags.add_argument("--size", default=None, type=str, metavar="WxH",
                         help="exact output size (default: 4x the input): both even for 4:2:0, an even width for --out_chroma 422, anything for "
                              "--out_chroma 444")
_size_flags.add_argument("--scale", default=None, type=float, help="output size relative to the INPUT, rounded to even numbers")


def video_out_size(h, w, size, scale, out_chroma):
    """inference.resolve_out_size under the output subsampling's rule: `--size` both even for "420", an even width for "422", anything
    for "444"; `--scale` rounds to even numbers whatever the subsampling."""
    from .inference import resolve_out_size
    if size is None:
        return resolve_out_size(h, w, None, scale, even=True)
    oh, ow = resolve_out_size(h, w, size, None, even=out_chroma == "420")
    if out_chroma == "422" and ow % 2:
        raise ValueError("--size %dx%d has an odd width: a YUV 4:2:2 frame holds one chroma sample per pair of pixels of a row, so the "
                         "output width must be even" % (ow, oh))
    return oh, ow


def _status(msg):
    print(msg, file=sys.stderr, flush=True)


def main(argv=None):
    import torch

    from .config import load_config
    from .inference import InferencePipeline, load_generator
    args = parser.parse_args(argv)
    try:    # a malformed or odd --size fails before the stream is opened; without --out_chroma that is 4:2:0's rule
        video_out_size(2, 2, args.size, args.scale, args.out_chroma or "420")
    except ValueError as exc:
        raise SystemExit("video: %s%s" % (exc, "" if args.out_chroma else " (an odd --size needs --out_chroma 422 or 444 spelled out)"))
    try:    # so do the format flags, as far as they can be judged without the stream
        raw_in = args.in_format != "y4m"
        if raw_in and args.in_size is None:
            raise ValueError("--in_format %s is a headerless stream: it needs --in_size WxH" % args.in_format)
        if not raw_in and args.in_size is not None:
            raise ValueError("--in_size is for raw input formats; a Y4M stream declares its size")
        in_size = parse_size(args.in_size, "--in_size") if raw_in else None
        fps = parse_fps(args.fps) if args.fps is not None else None
        resolve_formats(args.in_format, args.out_format, args.out_depth, args.out_chroma)
    except ValueError as exc:
        raise SystemExit("video: %s" % exc)
    if not torch.cuda.is_available():
        raise SystemExit("fast-srgan_amd runs on an MI355X only: no GPU is visible")
    fin = sys.stdin.buffer if args.input == "-" else open(args.input, "rb")
    fout = sys.stdout.buffer if args.output == "-" else open(args.output, "wb")
    try:
        if raw_in:
            layout, in_depth, _ = RAW_FORMATS[args.in_format]
            reader = RawReader(fin, in_size[0], in_size[1], yuv_frame_bytes(in_size[1], in_size[0], "420", in_depth, layout))
            reader.depth, reader.chroma, reader.siting, reader.colour_range = in_depth, "420", "jpeg", None
            reader.frame_rate, reader.aspect, reader.interlace = fps or "25:1", None, None
        else:
            layout = "planar"
            reader = Y4MReader(fin, max_depth=16, chroma=CHROMAS)
        siting = args.siting or reader.siting
        chroma, out_chroma = reader.chroma, args.out_chroma or reader.chroma
        try:
            out_format, out_depth = resolve_formats(args.in_format, args.out_format, args.out_depth, out_chroma, reader.depth)
        except ValueError as exc:
            raise SystemExit("video: %s" % exc)
        out_layout = RAW_FORMATS[out_format][0] if out_format in RAW_FORMATS else "planar"
        full = (reader.colour_range or args.range) == "full"
        out_full = full if args.out_range is None else args.out_range == "full"
        out_matrix = args.out_matrix or args.matrix
        config = load_config("configs/config.yaml")
        model = load_generator(config, "models/model.pt", "cuda", args.compute_dtype)
        s = 2 ** len(model.upsampling)
        h, w = reader.height, reader.width
        try:
            out_size = video_out_size(h, w, args.size, args.scale, out_chroma)
        except ValueError as exc:
            raise SystemExit("video: %s" % exc)
        oh, ow = out_size or (s * h, s * w)
        _status("video: %dx%d -> %dx%d%s, %s %s %d-bit -> %s %s %d-bit, chroma siting %s%s" % (
            w, h, ow, oh, "" if out_size is None else " (network %dx%d, resized)" % (s * w, s * h),
            args.matrix, "full" if full else "limited", reader.depth, out_matrix, "full" if out_full else "limited", out_depth, siting,
            ", 4:%s:%s -> 4:%s:%s" % (chroma[1], chroma[2], out_chroma[1], out_chroma[2])
            + ("" if (args.in_format, out_format) == ("y4m", "y4m") else ", %s -> %s" % (args.in_format, out_format))))
        if out_format in RAW_FORMATS:
            rate = (fps or reader.frame_rate or "25:1").replace(":", "/")
            _status("video: read the output with: -f rawvideo -pix_fmt %s -s %dx%d -r %s" % (RAW_FORMATS[out_format][2], ow, oh, rate))
        try:
            pipe = InferencePipeline(model, "cuda", batch=args.batch, copy=False, bands=args.bands, band_rows=args.band_rows)
        except ValueError as exc:
            raise SystemExit("video: %s" % exc)
        try:
            frames_out = pipe.run_yuv(reader.frames(), h, w, chroma=chroma, out_chroma=out_chroma, siting=siting, matrix=args.matrix,
                                      full_range=full, out_matrix=out_matrix, out_full_range=out_full, out_size=out_size,
                                      depth=reader.depth, out_depth=out_depth, layout=layout, out_layout=out_layout)
        except ValueError as exc:       # a frame too large for the kernels: refused before anything is allocated or written
            raise SystemExit("video: %s" % exc)
        batch = pipe._batch_for(h, w)       # (the pipeline has reported a batch it had to reduce, or a shape it runs in row bands)
        if out_format in RAW_FORMATS:
            writer = RawWriter(fout, ow, oh, yuv_frame_bytes(oh, ow, "420", out_depth, out_layout))
        else:
            writer = Y4MWriter(fout, ow, oh, reader.frame_rate, reader.aspect, reader.interlace, out_full, depth=out_depth, chroma=out_chroma)
        n, t0, t1 = 0, time.perf_counter(), None
        for y in frames_out:
            writer.write_frame(y)       # (a view of the pinned result buffer: written before the slot is reused)
            n += 1
            if n == batch:
                t1 = time.perf_counter()   # the first batch carries the plan's warm-up and graph capture
        fout.flush()
        t2 = time.perf_counter()
        steady = "%.1f fps after the first batch" % ((n - batch) / (t2 - t1)) if t1 is not None and n > batch else "-"
        _status("video: %d frames in %.3f s (%s)" % (n, t2 - t0, steady))
    finally:
        if fin is not sys.stdin.buffer:
            fin.close()
        if fout is not sys.stdout.buffer:
            fout.close()


if __name__ == "__main__":
    main()
