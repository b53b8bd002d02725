"""Video: 9- to 16-bit 4:2:0 frames in and out (Y4M C420p10 and its kin), and the batch the kernels can index.

The depth contract of DESIGN.md §6c is restated in numpy (float64, tests/yuv_contract.py), independently of the code under test.  Sample depth d,
8 <= d <= 16; a deep payload (d > 8) has the plane order and extents of an 8-bit one, every sample 2 bytes little-endian:
  limited range: Y = (16 + 219 E_Y) 2^(d-8), C = (128 + 224 E_C) 2^(d-8);  full range: Y = (2^d - 1) E_Y, C = 2^(d-1) + (2^d - 1) E_C;
  encode: code = clamp(floor(v + 0.5), 0, 2^d - 1).
Held to it: fsr_i420_to_image_deep (to 2e-6, the 8-bit bound), fsr_image_to_i420 and the 16-bit form of the resampler's I420 stage
(textbook codes exactly; random input within 1 code, the share of differing samples capped, CAP below), Generator.forward_yuv420,
InferencePipeline.run_yuv420 and the video CLI at every pair of depths."""
import importlib
import io
import os

import numpy as np
import pytest
import torch

from backend import BACKENDS, L, ops, select
from conftest import load_npz, sd_from
from yuv_contract import (CAP, _aa_matrix, _cli, _shipped, _stream, _tiny, assert_codes_close, from_payload, np_decode, np_encode, ns,
                          samples_of, to_payload)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
video = importlib.import_module("fast-srgan_amd.video")
inference = importlib.import_module("fast-srgan_amd.inference")

def _rand_payload(rng, n, h, w, d, top=None):
    return to_payload(rng.integers(0, top or 2 ** d, size=(n, samples_of(h, w))), d)


@pytest.fixture(params=BACKENDS)
def dev(request):
    return select(request.param)


COLOURS = [(m, f) for m in ("bt601", "bt709") for f in (False, True)]


# ---------------------------------------------------------------------------------------------------- 1. Y4M (host only)
def test_y4m_deep_streams_need_max_depth():
    rng = np.random.default_rng(0)
    h, w = 5, 7
    payloads = list(_rand_payload(rng, 3, h, w, 10))
    data = _stream(b"YUV4MPEG2 W7 H5 F25:1 Ip C420p10 XCOLORRANGE=LIMITED\n", payloads)
    with pytest.raises(video.Y4MError) as e:          # the default refuses, in today's words
        video.Y4MReader(io.BytesIO(data))
    assert "'C420p10'" in str(e.value) and "deeper than 8 bits" in str(e.value) and "8-bit only" in str(e.value)
    r = video.Y4MReader(io.BytesIO(data), max_depth=16)
    assert r.depth == 10 and r.frame_bytes == 2 * (35 + 2 * 12) == ops.i420_frame_bytes(h, w, 10)
    assert r.siting == "jpeg" and (r.width, r.height) == (7, 5)
    got = list(r.frames())
    assert len(got) == 3 and all(a.dtype == np.uint8 and np.array_equal(a, b) for a, b in zip(got, payloads))
    assert video.Y4MReader(io.BytesIO(data), max_depth=10).depth == 10
    # 8-bit streams: depth 8 at any max_depth
    r8 = video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W7 H5 C420mpeg2\n"), max_depth=16)
    assert r8.depth == 8 and r8.frame_bytes == 35 + 24 and r8.siting == "mpeg2"
    with pytest.raises(video.Y4MError, match="C420p12"):
        video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W7 H5 C420p12\n"), max_depth=10)
    for tag in (b"C422p10", b"C444p16", b"C444", b"Cmono", b"C444alpha", b"Cmono16", b"C420p8", b"C420p17"):
        for md in (8, 10, 16):
            with pytest.raises(video.Y4MError, match=tag.decode()[1:]):
                video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H4 F25:1 %s\n" % tag), max_depth=md)
    assert ops.i420_frame_bytes(5, 7) == 59 and ops.i420_frame_bytes(5, 7, 8) == 59 and ops.i420_frame_bytes(5, 7, 9) == 118
    for bad in (7, 17, 10.5):
        with pytest.raises(ValueError):
            ops.i420_frame_bytes(4, 4, bad)


def test_y4m_writer_round_trip_depth_12():
    rng = np.random.default_rng(1)
    out = io.BytesIO()
    wr = video.Y4MWriter(out, 6, 4, "25:1", None, "p", full_range=True, depth=12)
    p = _rand_payload(rng, 3, 4, 6, 12)
    for f in p:
        wr.write_frame(f)
    data = out.getvalue()
    assert data.startswith(b"YUV4MPEG2 W6 H4 F25:1 Ip C420p12 XCOLORRANGE=FULL\n")
    back = video.Y4MReader(io.BytesIO(data), max_depth=12)
    assert (back.depth, back.colour_range, back.frame_bytes) == (12, "full", 2 * 36)
    assert all(np.array_equal(a, b) for a, b in zip(back.frames(), p))
    with pytest.raises(video.Y4MError):
        wr.write_frame(p[0][:-2])
    with pytest.raises(video.Y4MError):
        wr.write_frame(p[0][:36])                       # the 8-bit size of the same frame
    frames = video.Y4MReader(io.BytesIO(data[:-5]), max_depth=16).frames()
    assert np.array_equal(next(frames), p[0]) and np.array_equal(next(frames), p[1])
    with pytest.raises(video.Y4MError, match="frame 2 is truncated"):
        next(frames)
    # depth 8 (the default) still writes C420jpeg
    out8 = io.BytesIO()
    video.Y4MWriter(out8, 6, 4)
    assert b" C420jpeg " in out8.getvalue()


# ---------------------------------------------------------------------------------------------------- 2. decode
@pytest.mark.parametrize("d", [9, 10, 12, 16])
def test_deep_decode_matches_the_numpy_contract(dev, d):
    rng = np.random.default_rng(20 + d)
    worst = 0.0
    for h, w in ((5, 7), (6, 9), (1, 3), (4, 4)):
        fr = _rand_payload(rng, 2, h, w, d)
        x = torch.from_numpy(fr).to(dev)
        for siting in ("jpeg", "mpeg2"):
            for matrix, full in COLOURS:
                got = ops.i420_to_image(x, h, w, siting, matrix, full, depth=d)
                assert got.shape == (2, 3, h, w) and got.dtype == torch.float32
                err = float(np.abs(got.cpu().double().numpy() - np_decode(from_payload(fr, d), h, w, "420", siting, matrix, full, d)).max())
                worst = max(worst, err)
                assert err < 2e-6, (d, h, w, siting, matrix, full, err)
    print("deep decode, depth %d: max abs error %.3g" % (d, worst))
    assert L.lib().fsr_last_kernel().decode() == "i420_to_image_kernel<u16>"


def test_deep_decode_takes_out_of_range_samples_and_refuses_bad_arguments(dev):
    rng = np.random.default_rng(3)
    h, w = 5, 7
    fr = _rand_payload(rng, 2, h, w, 10, top=65536)     # stored values above 2^10 - 1: taken as they are, the clamp deals with them
    got = ops.i420_to_image(torch.from_numpy(fr).to(dev), h, w, "jpeg", "bt709", False, depth=10)
    assert float(np.abs(got.cpu().double().numpy() - np_decode(from_payload(fr, 10), h, w, "420", "jpeg", "bt709", False, 10)).max()) < 2e-6
    x = torch.from_numpy(fr).to(dev)
    with pytest.raises(ValueError):
        ops.i420_to_image(x, h, w, depth=8)              # the payload size of another depth
    with pytest.raises(ValueError):
        ops.i420_to_image(x[:, :-2].contiguous(), h, w, depth=10)
    with pytest.raises(ValueError, match="siting"):
        ops.i420_to_image(x, h, w, siting="dv", depth=10)
    with pytest.raises(ValueError, match="depth"):
        ops.i420_to_image(x, h, w, depth=17)
    img = torch.empty((2, h, w, 3), dtype=torch.float32, device=dev)
    for bad in (8, 17):                                  # the deep entry point itself
        assert L.lib().fsr_i420_to_image_deep(x.data_ptr(), img.data_ptr(), 2, h, w, 0, 0, 0, bad, None) < 0
        assert b"depth" in L.lib().fsr_last_error()
    assert L.lib().fsr_i420_to_image_deep(x.data_ptr(), img.data_ptr(), 2, h, w, 2, 0, 0, 10, None) < 0
    assert b"siting" in L.lib().fsr_last_error()


# ---------------------------------------------------------------------------------------------------- 3. encode, textbook codes
TEXTBOOK = [   # (depth, matrix, full, (R, G, B) signs, (Y, Cb, Cr))
    (10, "bt601", False, (1, 1, 1), (940, 512, 512)), (10, "bt601", False, (-1, -1, -1), (64, 512, 512)),
    (10, "bt601", False, (1, -1, -1), (326, 361, 960)), (10, "bt709", False, (1, -1, -1), (250, 409, 960)),
    (10, "bt601", True, (1, 1, 1), (1023, 512, 512)), (10, "bt709", True, (-1, -1, 1), (74, 1023, 465)),
    (16, "bt601", False, (1, 1, 1), (60160, 32768, 32768)), (16, "bt601", False, (1, -1, -1), (20859, 23092, 61440)),
    (16, "bt709", True, (-1, -1, 1), (4732, 65535, 29763)),
]


def test_encode_textbook_codes(dev):
    n, h, w = 2, 6, 18
    plane = h * w
    for d, matrix, full, signs, codes in TEXTBOOK:
        t = np.broadcast_to(np.array(signs, np.float32)[None, None, None, :], (n, h, w, 3)).copy()
        want = np.concatenate([np.full((n, plane), codes[0]), np.full((n, plane // 4), codes[1]), np.full((n, plane // 4), codes[2])], axis=1)
        for ft in (np.float32, np.float64):              # the contract itself gives the textbook numbers
            assert np.array_equal(np_encode(t.transpose(0, 3, 1, 2), "420", matrix, full, d, ft), want), (d, matrix, full, signs, ft)
        out = ops.image_to_i420(torch.from_numpy(t).to(dev), matrix, full, depth=d)
        assert out.dtype == torch.uint8 and out.shape == (n, 2 * plane * 3 // 2)
        assert L.lib().fsr_last_kernel().decode() == "image_to_i420_kernel<u16>"
        got = from_payload(out.cpu().numpy(), d)
        assert np.array_equal(got, want), (d, matrix, full, signs, np.unique(got[:, :plane]), np.unique(got[:, plane:]))


# ---------------------------------------------------------------------------------------------------- 4. encode, random
ENC_SHAPES = ((2, 16, 24), (1, 2, 6))


def _enc_input(shape):
    """t uniform in [-1.1, 1.1] (both clamps act), NHWC float32."""
    n, h, w = shape
    g = torch.Generator().manual_seed(100 * h + w)
    return (torch.rand(n, h, w, 3, generator=g) * 2.2 - 1.1).contiguous()


def test_float32_restatement_is_inside_the_caps():
    """The float32 restatement alone against float64, on the inputs of test_encode_random: none differ at d <= 12; at 14 and 16 the
    measured share (see CAP) stays three times below the cap."""
    for d in (8, 10, 12, 14, 16):
        differ = total = 0
        for shape in ENC_SHAPES:
            t = _enc_input(shape).numpy().transpose(0, 3, 1, 2)
            for matrix, full in COLOURS:
                a, b = np_encode(t, "420", matrix, full, d, np.float32), np_encode(t, "420", matrix, full, d, np.float64)
                assert np.abs(a - b).max() <= 1
                differ, total = differ + int((a != b).sum()), total + a.size
        print("float32 restatement, depth %d: %d of %d samples differ (%.4f %%)" % (d, differ, total, 100.0 * differ / total))
        assert 3 * differ <= CAP[d] * total, (d, differ, total)


@pytest.mark.parametrize("d", [8, 10, 12, 14, 16])
def test_encode_random(dev, d):
    for shape in ENC_SHAPES:
        n, h, w = shape
        t = _enc_input(shape)
        for matrix, full in COLOURS:
            out = ops.image_to_i420(t.to(dev), matrix, full, depth=d)
            assert out.dtype == torch.uint8 and out.shape == (n, ops.i420_frame_bytes(h, w, d))
            assert L.lib().fsr_last_kernel().decode() == ("image_to_i420_kernel<u8>" if d == 8 else "image_to_i420_kernel<u16>")
            want = np_encode(t.numpy().transpose(0, 3, 1, 2), "420", matrix, full, d)
            assert_codes_close(from_payload(out.cpu().numpy(), d), want, CAP[d])


@pytest.mark.parametrize("shape", ENC_SHAPES + ((1, 6, 70), (1, 34, 132)), ids=lambda s: "%dx%dx%d" % s)
def test_encode_is_the_resamplers_i420_stage_at_the_native_size(dev, shape):
    """Same helpers, same order, identity taps: byte-identical at depth 8 (to the existing 8-bit resampler), 10 and 16."""
    n, h, w = shape
    t = _enc_input(shape).to(dev)
    for d in (8, 10, 16):
        for matrix, full in (("bt601", False), ("bt709", True)):
            a = ops.image_to_i420(t, matrix, full, depth=d)
            b = ops.resample_image(t, h, w, "i420", matrix, full) if d == 8 else ops.resample_image(t, h, w, "i420", matrix, full, depth=d)
            assert L.lib().fsr_last_kernel().decode() == ("resample_kernel<i420,5>" if d == 8 else "resample_kernel<i420,5,u16>")
            assert a.shape == b.shape and torch.equal(a, b), (d, matrix, full)


def test_deep_resize_against_the_tap_composition(dev):
    (h, w), (oh, ow), d = (9, 14), (20, 26), 10
    t = torch.rand(2, h, w, 3, generator=torch.Generator().manual_seed(9)) * 2.2 - 1.1
    c = (t.numpy().astype(np.float64).transpose(0, 3, 1, 2) + 1.0) / 2.0
    v = np.einsum("oy,ncyx,px->ncop", _aa_matrix(h, oh), c, _aa_matrix(w, ow))
    for matrix, full in COLOURS:
        got = ops.resample_image(t.to(dev), oh, ow, "i420", matrix, full, depth=d)
        assert L.lib().fsr_last_kernel().decode() == "resample_kernel<i420,5,u16>"
        assert got.dtype == torch.uint8 and got.shape == (2, ops.i420_frame_bytes(oh, ow, d))
        assert_codes_close(from_payload(got.cpu().numpy(), d), np_encode(2.0 * np.clip(v, 0.0, 1.0) - 1.0, "420", matrix, full, d), CAP[d])


def test_encode_refusals(dev):
    t = _enc_input((1, 4, 6)).to(dev)
    for bad in (7, 17):
        with pytest.raises((ValueError, L.FsrError), match="depth"):
            ops.image_to_i420(t, "bt601", False, depth=bad)
        with pytest.raises((ValueError, L.FsrError), match="depth"):
            ops.resample_image(t, 8, 8, "i420", depth=bad)
    out = torch.empty((1, 2 * 36), dtype=torch.uint8, device=dev)
    for bad in (7, 17):                                  # the entry points themselves
        assert L.lib().fsr_image_to_i420(t.data_ptr(), 1, 4, 6, 0, 0, bad, out.data_ptr(), None) < 0
        assert b"depth" in L.lib().fsr_last_error()
    for odd in ((1, 3, 6), (1, 4, 5)):
        with pytest.raises((ValueError, L.FsrError), match="even output extents"):
            ops.image_to_i420(_enc_input(odd).to(dev), depth=10)
    assert L.lib().fsr_image_to_i420(t.data_ptr(), 1, 3, 8, 0, 0, 10, out.data_ptr(), None) < 0
    assert b"even output extents" in L.lib().fsr_last_error()
    assert L.lib().fsr_image_to_i420(t.data_ptr(), 1, 4, 6, 2, 0, 10, out.data_ptr(), None) < 0
    assert b"colour matrix" in L.lib().fsr_last_error()
    with pytest.raises((ValueError, L.FsrError), match="even output extents"):
        ops.resample_image(t, 7, 8, "i420", depth=10)
    with pytest.raises(ValueError, match="i420"):
        ops.resample_image(t, 8, 8, "u8", depth=10)
    with pytest.raises(ValueError, match="matrix"):
        ops.image_to_i420(t, "bt2020")


# ---------------------------------------------------------------------------------------------------- 5. the whole generator
def _check_forward(G, fr, h, w, d, od, dev, colour, out_colour):
    """forward_yuv420 at (d, od) against the numpy encode of the same model's float forward() on the device-decoded frames."""
    x = torch.from_numpy(fr).to(dev)
    got = G.forward_yuv420(x, h, w, siting="mpeg2", matrix=colour[0], full_range=colour[1], out_matrix=out_colour[0],
                           out_full_range=out_colour[1], depth=d, out_depth=od)
    kernel = L.lib().fsr_last_kernel().decode()
    od = d if od is None else od
    assert got.dtype == torch.uint8 and got.shape == (fr.shape[0], ops.i420_frame_bytes(4 * h, 4 * w, od))
    with torch.no_grad():
        t = G(ops.i420_to_image(x, h, w, "mpeg2", colour[0], colour[1], depth=d)).cpu().numpy()
    assert_codes_close(from_payload(got.cpu().numpy(), od), np_encode(t, "420", out_colour[0], out_colour[1], od), CAP[od])
    return kernel


def test_forward_yuv420_depths_tiny_generator(dev, pkg):
    G = _tiny(pkg, dev)
    rng = np.random.default_rng(5)
    h, w = 3, 5
    fr10, fr8 = _rand_payload(rng, 2, h, w, 10), _rand_payload(rng, 2, h, w, 8)
    assert _check_forward(G, fr10, h, w, 10, None, dev, ("bt601", False), ("bt601", False)) == "image_to_i420_kernel<u16>"
    assert _check_forward(G, fr8, h, w, 8, 10, dev, ("bt709", True), ("bt601", False)) == "image_to_i420_kernel<u16>"
    assert _check_forward(G, fr10, h, w, 10, 8, dev, ("bt709", False), ("bt709", True)).startswith("conv_igemm_kernel<f32")
    # depth 8 and no out_depth: exactly the call without the new arguments
    x8 = torch.from_numpy(fr8).to(dev)
    assert torch.equal(G.forward_yuv420(x8, h, w, depth=8, out_depth=None), G.forward_yuv420(x8, h, w))
    assert torch.equal(G.forward_yuv420(x8, h, w, out_size=(14, 30), depth=8), G.forward_yuv420(x8, h, w, out_size=(14, 30)))
    # a resized deep output: the 16-bit form of the resampler
    y = G.forward_yuv420(x8, h, w, out_size=(14, 30), out_depth=12)
    assert L.lib().fsr_last_kernel().decode() == "resample_kernel<i420,5,u16>" and y.shape == (2, ops.i420_frame_bytes(14, 30, 12))
    for bad in (dict(depth=7), dict(out_depth=17)):
        with pytest.raises(ValueError, match="depth"):
            G.forward_yuv420(x8, h, w, **bad)


# ---------------------------------------------------------------------------------------------------- 6. GPU: shipped weights
@pytest.mark.gpu
@pytest.mark.parametrize("cdn, d, od", [("f16", 10, 10), ("x3", 10, 10), ("f32", 8, 16)])
def test_forward_yuv420_depths_shipped_weights_gpu(pkg, cdn, d, od, monkeypatch):
    dev = select("hip")
    monkeypatch.setenv("FSR_PERSIST_CUS", "5")
    G = _shipped(pkg, dev, cdn)
    rng = np.random.default_rng(6)
    h, w = 23, 37
    fr = _rand_payload(rng, 3, h, w, d)
    assert _check_forward(G, fr, h, w, d, od, dev, ("bt601", False), ("bt709", False)) == "image_to_i420_kernel<u16>"
    y = G.forward_yuv420(torch.from_numpy(fr).to(dev), h, w, out_size=(70, 100), depth=d, out_depth=od)
    name = L.lib().fsr_last_kernel().decode()
    assert name.startswith("resample_kernel<i420,") and name.endswith(",u16>"), name
    assert y.shape == (3, ops.i420_frame_bytes(70, 100, od))


# ---------------------------------------------------------------------------------------------------- 7. GPU: the pipeline
@pytest.mark.gpu
def test_pipeline_deep_graph_eager_single_gpu(pkg):
    dev = select("hip")
    G = _shipped(pkg, dev, "f16")
    rng = np.random.default_rng(7)
    h, w, d = 17, 29, 10
    frames = list(_rand_payload(rng, 7, h, w, d))
    colour = dict(siting="mpeg2", matrix="bt709", full_range=True, out_matrix="bt601", out_full_range=False)
    pipe = pkg.InferencePipeline(G, dev, batch=3, depth=2, copy=False)
    outs = []
    for y in pipe.run_yuv420(frames, h, w, depth=d, **colour):
        assert y.shape == (ops.i420_frame_bytes(4 * h, 4 * w, d),) and y.dtype == np.uint8     # views of the pinned buffers
        outs.append(y.copy())
    assert len(outs) == 7
    key = ("i420", h, w, "mpeg2", "bt709", True, "bt601", False, "depth", 10, 10)
    assert list(pipe._plans) == [key] and all(sl is not None and sl.graph is not None for sl in pipe._plans[key])
    eager = pkg.InferencePipeline(G, dev, batch=3, depth=2, use_graph=False)
    outs_eager = list(eager.run_yuv420((bytes(f) for f in frames), h, w, depth=d, out_depth=None, **colour))
    for f, y, ye in zip(frames, outs, outs_eager):
        one = G.forward_yuv420(torch.from_numpy(f).unsqueeze(0).to(dev), h, w, depth=d, **colour)[0].cpu().numpy()
        assert np.array_equal(y, one) and np.array_equal(ye, one)
    # an 8-bit run through the same pipeline: the key of the existing plans, next to the deep one
    frames8 = list(_rand_payload(rng, 3, h, w, 8))
    outs8 = list(pipe.run_yuv420(frames8, h, w, **colour))
    assert list(pipe._plans) == [key, key[:-3]]
    assert np.array_equal(outs8[0], G.forward_yuv420(torch.from_numpy(frames8[0]).unsqueeze(0).to(dev), h, w, **colour)[0].cpu().numpy())
    # 8 in, 10 out: its own plan
    list(pipe.run_yuv420(frames8, h, w, out_depth=10, **colour))
    assert list(pipe._plans)[-1] == key[:-3] + ("depth", 8, 10)


# ---------------------------------------------------------------------------------------------------- 8. GPU: the CLI
@pytest.fixture(scope="module")
def cli_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("deep_cli")
    sd = sd_from(load_npz("g_model_pt.npz"), "sd.")
    (d / "models").mkdir()
    (d / "configs").mkdir()
    torch.save({"_orig_mod." + k: v for k, v in sd.items()}, d / "models" / "model.pt")
    (d / "configs" / "config.yaml").write_text("generator:\n  n_filters: 64\n  n_layers: 8\ntraining:\n  compute_dtype: f16\n")
    return d


@pytest.mark.gpu
def test_video_cli_deep_stream_gpu(cli_dir):
    dev = select("hip")
    rng = np.random.default_rng(8)
    h, w, nf = 9, 14, 5
    frames = _rand_payload(rng, nf, h, w, 10)
    data = _stream(b"YUV4MPEG2 W14 H9 F30000:1001 Ip A1:1 C420p10 XCOLORRANGE=LIMITED\n", frames)
    r = _cli(cli_dir, data)
    assert r.stdout.split(b"\n", 1)[0].startswith(b"YUV4MPEG2 W56 H36 ") and b" C420p10 " in r.stdout.split(b"\n", 1)[0]
    assert b"10-bit -> bt601 limited 10-bit" in r.stderr
    out = video.Y4MReader(io.BytesIO(r.stdout), max_depth=16)
    assert (out.width, out.height, out.depth, out.frame_rate, out.colour_range) == (56, 36, 10, "30000:1001", "limited")
    got = list(out.frames())
    assert len(got) == nf
    G = inference.load_generator(importlib.import_module("fast-srgan_amd.config").load_config(str(cli_dir / "configs" / "config.yaml")),
                                 str(cli_dir / "models" / "model.pt"), dev)
    want = G.forward_yuv420(torch.from_numpy(frames[:1]).to(dev), h, w, depth=10)[0].cpu().numpy()
    assert np.array_equal(got[0], want)


@pytest.mark.gpu
def test_video_cli_deep_to_8_bit_gpu(cli_dir):
    select("hip")
    rng = np.random.default_rng(8)
    frames = _rand_payload(rng, 5, 9, 14, 10)
    r = _cli(cli_dir, _stream(b"YUV4MPEG2 W14 H9 F25:1 C420p10\n", frames), "--out_depth", "8", "--siting", "mpeg2")
    assert b" C420jpeg " in r.stdout.split(b"\n", 1)[0] and b"chroma siting mpeg2" in r.stderr
    out = video.Y4MReader(io.BytesIO(r.stdout))             # an existing reader, its defaults
    assert (out.width, out.height, out.depth, out.frame_bytes) == (56, 36, 8, 56 * 36 * 3 // 2)
    assert len(list(out.frames())) == 5


@pytest.mark.gpu
def test_video_cli_8_bit_to_deep_resized_gpu(cli_dir):
    select("hip")
    rng = np.random.default_rng(8)
    frames = _rand_payload(rng, 3, 9, 14, 8)
    r = _cli(cli_dir, _stream(b"YUV4MPEG2 W14 H9 F25:1 C420jpeg\n", frames), "--out_depth", "10", "--size", "40x30")
    assert r.stdout.split(b"\n", 1)[0].startswith(b"YUV4MPEG2 W40 H30 ") and b" C420p10 " in r.stdout.split(b"\n", 1)[0]
    out = video.Y4MReader(io.BytesIO(r.stdout), max_depth=10)
    assert (out.width, out.height, out.depth) == (40, 30, 10) and len(list(out.frames())) == 3


# ---------------------------------------------------------------------------------------------------- 9. the batch limit
def test_max_batch_and_the_pipelines_refusal(pkg):
    G = pkg.Generator(ns(n_filters=64, n_layers=8), compute_dtype="f32")
    got = {hw: G.max_batch(*hw) for hw in ((360, 640), (480, 854), (720, 1280), (1080, 1920), (1440, 2560))}
    assert got == {(360, 640): 9, (480, 854): 5, (720, 1280): 2, (1080, 1920): 1, (1440, 2560): 0}
    # no up-sampling block: the neck's output sets the limit
    assert pkg.Generator(ns(n_filters=16, n_layers=1, n_upsample=0), compute_dtype="f32").max_batch(1024, 1024) == 127
    pipe = pkg.InferencePipeline(G, "cpu", batch=8)
    assert pipe._batch_for(360, 640) == 8 and pipe._batch_for(480, 854) == 5 and pipe._batch_for(1080, 1920) == 1
    with pytest.raises(ValueError, match="2560x1440") as e:
        pipe.run_yuv420([], 1440, 2560, depth=10)
    assert "2^31" in str(e.value)
    with pytest.raises(ValueError, match="2560x1440"):
        list(pipe.run([np.zeros((1440, 2560, 3), np.uint8)]))
    assert not pipe._plans


@pytest.mark.gpu
def test_pipeline_reduced_batch_gpu(pkg, monkeypatch, capfd):
    dev = select("hip")
    G = _shipped(pkg, dev, "f16")
    monkeypatch.setattr(G, "max_batch", lambda h, w: 2)
    rng = np.random.default_rng(9)
    h, w = 8, 12
    frames = list(_rand_payload(rng, 6, h, w, 8))
    pipe = pkg.InferencePipeline(G, dev, batch=4, depth=2)
    outs = list(pipe.run_yuv420(frames, h, w))
    outs_again = list(pipe.run_yuv420(frames[:3], h, w))     # the tail of 1 runs eagerly
    assert len(outs) == 6 and len(outs_again) == 3
    (key, plan), = pipe._plans.items()
    assert all(sl is not None and sl.x.shape[0] == 2 and sl.host_in.shape[0] == 2 and sl.y.shape[0] == 2 for sl in plan)
    for f, y in zip(frames, outs):
        assert np.array_equal(y, G.forward_yuv420(torch.from_numpy(f).unsqueeze(0).to(dev), h, w)[0].cpu().numpy())
    assert all(np.array_equal(a, b) for a, b in zip(outs[:3], outs_again))
    assert capfd.readouterr().err.count("batches of 2 instead of 4") == 1       # said once
    # RGB frames take the same limit
    rgb = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(5)]
    got = list(pipe.run(rgb))
    assert all(sl is None or sl.x.shape[0] == 2 for sl in pipe._plans[(h, w)])
    for f, y in zip(rgb, got):
        assert np.array_equal(y, G.forward_u8(torch.from_numpy(f).unsqueeze(0).to(dev))[0].cpu().numpy())
