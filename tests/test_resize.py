"""Arbitrary output size: the fused antialiased bicubic resize after the head (csrc/resample.hip).

The reference is torch's own CPU kernel in float64, F.interpolate(mode="bicubic", antialias=True, align_corners=False):
  * float output to 2e-5 -- three times the 6.7e-6 by which the two CPU float32 restatements (torch's kernel, the oracle's
    resize_bicubic_aa) differ from each other and from float64 on these shapes;
  * uint8 and I420 codes within 1 code, at most 0.1 % differing (float32 against float64 rounding ties, the cap of test_video);
  * identity taps reproduce forward_u8's truncating cast byte for byte.
The kernel tests run on the emulator and, marked gpu, on the device."""
import functools
import importlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from backend import BACKENDS, L, ops, select
from conftest import load_npz, sd_from
from test_video import HEAD_KERNEL, _frames
from yuv_contract import _shipped, _stream, assert_codes_close, np_encode, ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
video = importlib.import_module("fast-srgan_amd.video")
inference = importlib.import_module("fast-srgan_amd.inference")

# (h, w) -> (oh, ow): anisotropic ratios in both directions, ratio 8, several 64 x 32 tiles with partial ones at the right and
# bottom, degenerate extents, the identity; the last one is a ratio-8 down-scale whose row window forces 4-row tiles (5 of them)
PAIRS = [((16, 24), (12, 18)), ((16, 24), (6, 10)), ((16, 24), (22, 30)), ((16, 24), (2, 4)), ((20, 28), (10, 26)),
         ((24, 40), (38, 66)), ((48, 80), (18, 36)), ((5, 7), (5, 7)), ((1, 3), (4, 2)), ((160, 8), (20, 4))]
RESIZING = [p for p in PAIRS if p[0] != p[1]]
EVEN = [p for p in RESIZING if p[1][0] % 2 == 0 and p[1][1] % 2 == 0]
_id = lambda p: "%dx%d-%dx%d" % (p[0] + p[1])   # noqa: E731


@pytest.fixture(params=BACKENDS)
def dev(request):
    return select(request.param)


def _interp(x_nchw, size):
    return F.interpolate(x_nchw.double(), size=size, mode="bicubic", antialias=True, align_corners=False)


@functools.lru_cache(maxsize=None)
def _case(pair):
    """(t NHWC float32 in (-1, 1), float64 resize of t, float64 resize v of c = (t + 1) / 2), computed once per pair."""
    (h, w), size = pair
    g = torch.Generator().manual_seed(1000 * h + w + size[0])
    t = torch.rand(2, h, w, 3, generator=g) * 2 - 1
    nchw = t.permute(0, 3, 1, 2)
    return t, _interp(nchw, size), _interp((nchw.double() + 1) / 2, size)


def _u8_codes(v):
    """(N,3,H,W) float64 v -> (N,H,W,3) uint8 trunc(255 clip(v, 0, 1))."""
    return np.trunc(255.0 * np.clip(np.asarray(v), 0.0, 1.0)).astype(np.uint8).transpose(0, 2, 3, 1)


# ---------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("pair", PAIRS, ids=_id)
def test_float_output_matches_torch_interpolate(dev, pair):
    t, want, _ = _case(pair)
    oh, ow = pair[1]
    got = ops.resample_image(t.to(dev), oh, ow, kind="f32")
    assert got.shape == (2, 3, oh, ow) and got.dtype == torch.float32
    assert L.lib().fsr_last_kernel().decode().startswith("resample_kernel<f32")
    err = float((got.cpu().double() - want).abs().max())
    print("resample f32", pair, "max abs error", err)
    assert err < 2e-5, (pair, err)


@pytest.mark.parametrize("hw", [(5, 7), (33, 70), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_identity_size_reproduces_the_truncating_cast_exactly(dev, hw):
    h, w = hw
    xmin, xsize, taps, _ = importlib.import_module("fast-srgan_amd.dataloader").aa_bicubic_taps(7, 7)
    assert all(taps[i, i - xmin[i]] == 1.0 and np.count_nonzero(taps[i]) == 1 for i in range(7))     # [0, 1, 0, 0]
    t = torch.rand(2, h, w, 3, generator=torch.Generator().manual_seed(7)) * 2 - 1
    got = ops.resample_image(t.to(dev), h, w, kind="u8")
    assert got.shape == (2, h, w, 3) and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), ((t + 1) / 2 * 255).to(torch.uint8))


@pytest.mark.parametrize("pair", RESIZING, ids=_id)
def test_uint8_codes(dev, pair):
    t, _, v = _case(pair)
    got = ops.resample_image(t.to(dev), *pair[1], kind="u8")
    assert got.shape == (2,) + pair[1] + (3,) and got.dtype == torch.uint8
    assert_codes_close(got.cpu().numpy(), _u8_codes(v), 1e-3)


@pytest.mark.parametrize("pair", EVEN, ids=_id)
def test_i420_codes(dev, pair):
    t, _, v = _case(pair)
    oh, ow = pair[1]
    for matrix in ("bt601", "bt709"):
        for full in (False, True):
            got = ops.resample_image(t.to(dev), oh, ow, kind="i420", matrix=matrix, full_range=full)
            assert got.shape == (2, ops.i420_frame_bytes(oh, ow)) and got.dtype == torch.uint8
            want = np_encode(2.0 * np.clip(v.numpy(), 0.0, 1.0) - 1.0, "420", matrix, full)
            assert_codes_close(got.cpu().numpy(), want, 1e-3)


def test_refusals(dev):
    t = (torch.rand(1, 17, 8, 3) * 2 - 1).to(dev)
    with pytest.raises((L.FsrError, ValueError), match="even output extents"):
        ops.resample_image(t, 7, 8, kind="i420")
    with pytest.raises((L.FsrError, ValueError), match="even output extents"):
        ops.resample_image(t, 8, 5, kind="i420")
    with pytest.raises(L.FsrError, match="ratio"):                       # 17 / 2 > 8
        ops.resample_image(t, 2, 8, kind="u8")
    with pytest.raises(L.FsrError, match="ratio"):                       # 17 / 2 > 8 along the width
        ops.resample_image(t.permute(0, 2, 1, 3).contiguous(), 8, 2, kind="f32")
    assert ops.resample_image(t[:, :16], 2, 1, kind="u8").shape == (1, 2, 1, 3)        # exactly 8: served
    with pytest.raises(ValueError, match=r"\(N,H,W,3\)"):
        ops.resample_image(t[0], 8, 8)                                   # rank
    with pytest.raises(ValueError, match=r"\(N,H,W,3\)"):
        ops.resample_image(t.double(), 8, 8)                             # dtype
    with pytest.raises(ValueError, match=r"\(N,H,W,3\)"):
        ops.resample_image(torch.zeros(1, 4, 4, 4).to(dev), 8, 8)        # channel count
    with pytest.raises(ValueError, match="colour matrix"):
        ops.resample_image(t, 8, 8, kind="i420", matrix="bt2020")
    with pytest.raises(ValueError, match="kind"):
        ops.resample_image(t, 8, 8, kind="u16")
    # the C entry point itself: odd I420 extents, unknown kinds / matrices / ranges, null pointers -- nothing is launched
    wy, ymin, ysize, ky = ops.aa_taps(17, 8, dev)
    wx, xmin, xsize, kx = ops.aa_taps(8, 8, dev)
    out = torch.zeros(1, 8 * 8 * 3, dtype=torch.uint8).to(dev)
    p = lambda x: x.data_ptr()   # noqa: E731

    def call(oh=8, ow=8, kind=L.OUT_I420, matrix=0, full=0, tp=p(t), op=p(out)):
        return L.lib().fsr_resample_image(tp, 1, 17, 8, oh, ow, p(wy), p(ymin), p(ysize), ky, p(wx), p(xmin), p(xsize), kx, kind, matrix,
                                          full, op, None if L.is_emulation() else torch.cuda.current_stream().cuda_stream)

    for kwargs, word in ((dict(oh=7), b"even output extents"), (dict(kind=L.OUT_DTYPE), b"output kind"), (dict(kind=9), b"output kind"),
                         (dict(matrix=2), b"colour matrix"), (dict(full=2), b"colour matrix"), (dict(tp=None), b"null"),
                         (dict(op=None), b"null")):
        assert call(**kwargs) < 0 and word in L.lib().fsr_last_error(), (kwargs, L.lib().fsr_last_error())


def test_tap_tables_are_cached_per_size_and_device(dev):
    a, b = ops.aa_taps(24, 66, dev), ops.aa_taps(24, 66, dev)
    assert all(x is y for x, y in zip(a, b)) and a[0].shape == (66, a[3]) and a[0].device.type == dev.type
    assert ops.aa_taps(66, 24, dev)[0] is not a[0]


# ---------------------------------------------------------------------------------------------------- the model
def _tiny(pkg, dev):
    G = pkg.Generator(ns(n_filters=16, n_layers=1), compute_dtype="f32")
    G.load_state_dict(sd_from(load_npz("g_tiny.npz"), "sd."))
    return G.to(dev).eval()


def _resized_v(t_nchw, size):
    """float64 resize of c = (t + 1) / 2 for a model's float forward() output t."""
    return _interp((t_nchw.detach().cpu().double() + 1) / 2, size).numpy()


def test_forward_u8_and_yuv420_out_size_tiny_generator(dev, pkg):
    G = _tiny(pkg, dev)
    rng = np.random.default_rng(11)
    h, w, size = 5, 7, (14, 30)
    fr = torch.from_numpy(rng.integers(0, 256, size=(2, h, w, 3), dtype=np.uint8)).to(dev)
    got = G.forward_u8(fr, out_size=size)
    assert L.lib().fsr_last_kernel().decode() == "resample_kernel<u8,5>"
    assert got.shape == (2, 14, 30, 3) and got.dtype == torch.uint8
    with torch.no_grad():
        t = G(ops.u8_to_image(fr))
    assert_codes_close(got.cpu().numpy(), _u8_codes(_resized_v(t, size)), 1e-3)
    # None and the native size: today's path, the head's own epilogue, the same bytes
    native = G.forward_u8(fr)
    for same in (None, (20, 28)):
        y = G.forward_u8(fr, out_size=same)
        assert L.lib().fsr_last_kernel().decode() == HEAD_KERNEL["f32"]
        assert torch.equal(y, native)
    # I420 in and out
    fy = torch.from_numpy(_frames(rng, 2, h, w)).to(dev)
    colour = dict(siting="mpeg2", matrix="bt709", full_range=True, out_matrix="bt601", out_full_range=False)
    got = G.forward_yuv420(fy, h, w, out_size=size, **colour)
    assert L.lib().fsr_last_kernel().decode() == "resample_kernel<i420,5>"
    assert got.shape == (2, ops.i420_frame_bytes(*size)) and got.dtype == torch.uint8
    with torch.no_grad():
        t = G(ops.i420_to_image(fy, h, w, "mpeg2", "bt709", True))
    want = np_encode(2.0 * np.clip(_resized_v(t, size), 0.0, 1.0) - 1.0, "420", "bt601", False)
    assert_codes_close(got.cpu().numpy(), want, 1e-3)
    native = G.forward_yuv420(fy, h, w, **colour)
    for same in (None, (20, 28)):
        y = G.forward_yuv420(fy, h, w, out_size=same, **colour)
        assert L.lib().fsr_last_kernel().decode() == HEAD_KERNEL["f32"]
        assert torch.equal(y, native)
    with pytest.raises((L.FsrError, ValueError), match="even output extents"):
        G.forward_yuv420(fy, h, w, out_size=(15, 30))
    with pytest.raises(ValueError, match="out_size"):
        G.forward_u8(fr, out_size=(0, 30))


# ---------------------------------------------------------------------------------------------------- host only
def test_resolve_out_size():
    r = inference.resolve_out_size
    assert r(360, 640) is None and r(360, 640, even=True) is None
    assert r(360, 640, size="1920x1080") == (1080, 1920) and r(9, 14, size="1920X1080", even=True) == (1080, 1920)
    assert r(5, 7, scale=1.5) == (8, 11)                         # round(7.5) = 8 (halves up), round(10.5) = 11
    assert r(5, 7, scale=1.5, even=True) == (8, 10)              # the nearest even numbers to 7.5 and 10.5
    assert r(9, 14, scale=3.0, even=True) == (28, 42) and r(9, 14, scale=3.0) == (27, 42)
    assert r(360, 640, scale=3) == (1080, 1920) and r(3, 3, scale=0.1) == (1, 1) and r(3, 3, scale=0.1, even=True) == (2, 2)
    with pytest.raises(ValueError, match="mutually exclusive"):
        r(5, 7, size="20x20", scale=2.0)
    with pytest.raises(ValueError, match="even"):
        r(5, 7, size="31x20", even=True)
    assert r(5, 7, size="31x21") == (21, 31)                     # odd sizes are fine for RGB frames
    for bad in ("1920", "1920x", "axb", "10x-4", "0x8"):
        with pytest.raises(ValueError, match="--size"):
            r(5, 7, size=bad)
    with pytest.raises(ValueError, match="--scale"):
        r(5, 7, scale=0.0)
    # both parsers know the flags and refuse them together
    for parser in (video.parser, inference.parser):
        base = ["--input", "-", "--output", "-"] if parser is video.parser else ["--image_dir", "a", "--output_dir", "b"]
        a = parser.parse_args(base + ["--size", "1920x1080"])
        assert (a.size, a.scale) == ("1920x1080", None)
        assert parser.parse_args(base + ["--scale", "1.5"]).scale == 1.5 and parser.parse_args(base).size is None
        with pytest.raises(SystemExit):
            parser.parse_args(base + ["--size", "1920x1080", "--scale", "2"])


def test_video_cli_refuses_an_odd_size_before_it_opens_the_stream():
    with pytest.raises(SystemExit, match="odd.*even"):
        video.main(["--input", "/nonexistent.y4m", "--output", "/nonexistent/out.y4m", "--size", "641x360"])


def test_y4m_writer_emits_the_resized_extents():
    oh, ow = inference.resolve_out_size(9, 14, scale=1.5, even=True)
    assert (oh, ow) == (14, 22)
    out = io.BytesIO()
    wr = video.Y4MWriter(out, ow, oh, "25:1", None, "p", full_range=True)
    payload = np.arange(ops.i420_frame_bytes(oh, ow), dtype=np.uint8)
    wr.write_frame(payload)
    assert out.getvalue().startswith(b"YUV4MPEG2 W22 H14 F25:1 Ip C420jpeg XCOLORRANGE=FULL\n")
    back = video.Y4MReader(io.BytesIO(out.getvalue()))
    assert (back.width, back.height) == (22, 14) and np.array_equal(next(back.frames()), payload)


# ---------------------------------------------------------------------------------------------------- GPU: shipped weights
@pytest.mark.gpu
@pytest.mark.parametrize("cdn", ["f16", "x3"])
def test_out_size_shipped_weights_gpu(pkg, cdn, monkeypatch):
    dev = select("hip")
    monkeypatch.setenv("FSR_PERSIST_CUS", "5")
    G = _shipped(pkg, dev, cdn)
    rng = np.random.default_rng(12)
    h, w, size = 23, 37, (50, 84)
    fr = torch.from_numpy(rng.integers(0, 256, size=(3, h, w, 3), dtype=np.uint8)).to(dev)
    got = G.forward_u8(fr, out_size=size).cpu().numpy()
    assert L.lib().fsr_last_kernel().decode() == "resample_kernel<u8,9>" and got.shape == (3, 50, 84, 3)     # 92 x 148 -> 50 x 84: 9 taps
    with torch.no_grad():
        t = G(ops.u8_to_image(fr))
    assert_codes_close(got, _u8_codes(_resized_v(t, size)), 1e-3)
    fy = torch.from_numpy(_frames(rng, 3, h, w)).to(dev)
    got = G.forward_yuv420(fy, h, w, siting="jpeg", matrix="bt601", full_range=False, out_matrix="bt709", out_size=size).cpu().numpy()
    assert L.lib().fsr_last_kernel().decode() == "resample_kernel<i420,9>" and got.shape == (3, ops.i420_frame_bytes(*size))
    with torch.no_grad():
        t = G(ops.i420_to_image(fy, h, w, "jpeg", "bt601", False))
    assert_codes_close(got, np_encode(2.0 * np.clip(_resized_v(t, size), 0.0, 1.0) - 1.0, "420", "bt709", False), 1e-3)


@pytest.mark.gpu
def test_pipeline_out_size_graph_eager_single_gpu(pkg):
    """7 frames at batch 3 through run / run_yuv420 with out_size: graph replays, eager pipelines and single calls give the same
    bytes; native and resized plans of one shape live under distinct keys."""
    dev = select("hip")
    G = _shipped(pkg, dev, "f16")
    rng = np.random.default_rng(13)
    h, w, size = 23, 37, (50, 84)
    rgb = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(7)]
    yuv = list(_frames(rng, 7, h, w))
    colour = dict(siting="mpeg2", matrix="bt709", full_range=True, out_matrix="bt601", out_full_range=False)
    pipe = pkg.InferencePipeline(G, dev, batch=3, depth=2)
    eager = pkg.InferencePipeline(G, dev, batch=3, depth=2, use_graph=False)
    outs, outs_eager = list(pipe.run(rgb, out_size=size)), list(eager.run(iter(rgb), out_size=size))
    assert len(outs) == 7 and all(o.shape == (50, 84, 3) for o in outs)
    for f, y, ye in zip(rgb, outs, outs_eager):
        one = G.forward_u8(torch.from_numpy(f).unsqueeze(0).to(dev), out_size=size)[0].cpu().numpy()
        assert np.array_equal(y, one) and np.array_equal(ye, one)
    youts = list(pipe.run_yuv420(yuv, h, w, out_size=size, **colour))
    youts_eager = list(eager.run_yuv420((bytes(f) for f in yuv), h, w, out_size=size, **colour))
    assert len(youts) == 7 and all(o.shape == (ops.i420_frame_bytes(*size),) for o in youts)
    for f, y, ye in zip(yuv, youts, youts_eager):
        one = G.forward_yuv420(torch.from_numpy(f).unsqueeze(0).to(dev), h, w, out_size=size, **colour)[0].cpu().numpy()
        assert np.array_equal(y, one) and np.array_equal(ye, one)
    # native plans of the same shape next to the resized ones; the native size given explicitly IS the native plan
    native = list(pipe.run(rgb[:3]))
    assert native[0].shape == (4 * h, 4 * w, 3)
    assert np.array_equal(list(pipe.run(rgb[:3], out_size=(4 * h, 4 * w)))[0], native[0])
    list(pipe.run_yuv420(yuv[:3], h, w, **colour))
    ykey = ("i420", h, w, "mpeg2", "bt709", True, "bt601", False)
    want_keys = [(h, w, "size", 50, 84), ykey + ("size", 50, 84), (h, w), ykey]
    assert sorted(map(str, pipe._plans)) == sorted(map(str, want_keys))
    assert all(sl.graph is not None for k in want_keys for sl in pipe._plans[k] if sl is not None)
    # run_mixed: one size for all, or a function of the input shape
    small = [rng.integers(0, 256, size=(8, 12, 3), dtype=np.uint8) for _ in range(2)]
    mixed = eager.run_mixed([rgb[0], small[0], small[1]], out_size=lambda hh, ww: (2 * hh, 3 * ww))
    assert [m.shape for m in mixed] == [(46, 111, 3), (16, 36, 3), (16, 36, 3)]
    assert np.array_equal(mixed[1], G.forward_u8(torch.from_numpy(small[0]).unsqueeze(0).to(dev), out_size=(16, 36))[0].cpu().numpy())


@pytest.mark.gpu
def test_video_cli_size_through_pipes_gpu(pkg, tmp_path):
    dev = select("hip")
    sd = sd_from(load_npz("g_model_pt.npz"), "sd.")
    (tmp_path / "models").mkdir()
    (tmp_path / "configs").mkdir()
    torch.save({"_orig_mod." + k: v for k, v in sd.items()}, tmp_path / "models" / "model.pt")
    (tmp_path / "configs" / "config.yaml").write_text("generator:\n  n_filters: 64\n  n_layers: 8\ntraining:\n  compute_dtype: f16\n")
    rng = np.random.default_rng(14)
    h, w, nf = 9, 14, 5
    frames = _frames(rng, nf, h, w)
    data = _stream(b"YUV4MPEG2 W14 H9 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n", frames, frame_line=b"FRAME Ixyz\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "video.py"), "--input", "-", "--output", "-", "--batch", "2",
                        "--matrix", "bt709", "--size", "40x26"], input=data, capture_output=True, cwd=tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"14x9 -> 40x26" in r.stderr
    out = video.Y4MReader(io.BytesIO(r.stdout))
    assert (out.width, out.height, out.frame_rate, out.aspect, out.interlace, out.siting, out.colour_range) == \
        (40, 26, "30000:1001", "1:1", "p", "jpeg", "limited")
    got = list(out.frames())
    assert len(got) == nf
    G = inference.load_generator(importlib.import_module("fast-srgan_amd.config").load_config(str(tmp_path / "configs" / "config.yaml")),
                                 str(tmp_path / "models" / "model.pt"), dev)
    want = list(pkg.InferencePipeline(G, dev, batch=2).run_yuv420(list(frames), h, w, matrix="bt709", out_size=(26, 40)))
    assert len(want) == nf and all(np.array_equal(a, b) for a, b in zip(got, want))
