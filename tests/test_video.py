"""Video super-resolution: I420 (planar YUV 4:2:0) frames in and out, and the Y4M stream CLI (fast-srgan_amd/video.py).

The colour contract of DESIGN.md §6c is restated in numpy (float64, tests/yuv_contract.py) and every device path is held to it:
  * fsr_i420_to_image (decode + bilinear chroma upsampling at the declared siting) to 2e-6;
  * the FSR_OUT_I420 epilogues of the head kernels (conv_igemm's thin path for f32, conv64_thin_kernel's 16-bit and x3 forms)
    to the textbook codes, and, on real models, to the numpy encode of the same model's float forward() output."""
import importlib
import io
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from backend import BACKENDS, L, ops, select
from conftest import load_npz, sd_from
from oracle import srgan_cpu as O
from yuv_contract import _shipped, _stream, _tiny, assert_codes_close, np_decode, np_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
video = importlib.import_module("fast-srgan_amd.video")

def _frames(rng, n, h, w):
    return rng.integers(0, 256, size=(n, ops.i420_frame_bytes(h, w)), dtype=np.uint8)


@pytest.fixture(params=BACKENDS)
def dev(request):
    return select(request.param)


# ---------------------------------------------------------------------------------------------------- Y4M (host only)
def test_y4m_round_trip_tags_and_frame_parameters():
    rng = np.random.default_rng(0)
    h, w = 5, 7
    payloads = list(_frames(rng, 3, h, w))
    hdr = b"YUV4MPEG2 W7 H5 F30000:1001 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL\n"
    r = video.Y4MReader(io.BytesIO(_stream(hdr, payloads, frame_line=b"FRAME Ixyz XFOO=1\n")))
    assert (r.width, r.height, r.frame_rate, r.aspect, r.interlace) == (7, 5, "30000:1001", "1:1", "p")
    assert r.siting == "mpeg2" and r.colour_range == "full" and r.frame_bytes == 35 + 2 * 3 * 4
    got = list(r.frames())
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, payloads))
    # no C tag: C420jpeg; XCOLORRANGE absent: the command line decides
    r = video.Y4MReader(io.BytesIO(_stream(b"YUV4MPEG2 W7 H5 F25:1\n", payloads[:1])))
    assert r.siting == "jpeg" and r.colour_range is None and r.aspect is None
    # the writer: W, H (scaled by the caller), F / I / A copied, C420jpeg, XCOLORRANGE of the output range; FRAME + payload
    out = io.BytesIO()
    wr = video.Y4MWriter(out, 28, 20, "30000:1001", "1:1", "p", full_range=False)
    big = _frames(rng, 2, 20, 28)
    for p in big:
        wr.write_frame(p)
    data = out.getvalue()
    assert data.startswith(b"YUV4MPEG2 W28 H20 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n")
    back = video.Y4MReader(io.BytesIO(data))
    assert (back.width, back.height, back.siting, back.colour_range) == (28, 20, "jpeg", "limited")
    assert all(np.array_equal(a, b) for a, b in zip(back.frames(), big))
    with pytest.raises(video.Y4MError):
        wr.write_frame(big[0][:-1])


@pytest.mark.parametrize("tag, words", [
    ("It", ["'It'", "interlaced"]), ("Ib", ["'Ib'", "interlaced"]), ("Im", ["'Im'", "interlaced"]),
    ("C420paldv", ["'C420paldv'"]), ("C411", ["'C411'"]), ("C422", ["'C422'"]), ("C444", ["'C444'"]),
    ("C444alpha", ["'C444alpha'"]), ("Cmono", ["'Cmono'"]),
    ("C420p10", ["'C420p10'", "8 bits"]), ("C420p12", ["'C420p12'", "8 bits"]), ("C444p16", ["'C444p16'", "8 bits"]),
])
def test_y4m_rejects_what_it_cannot_decode(tag, words):
    with pytest.raises(video.Y4MError) as e:
        video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H4 F25:1 %s\n" % tag.encode()))
    for word in words:
        assert word in str(e.value), (tag, str(e.value))


def test_y4m_truncated_last_frame_is_an_error_naming_it():
    rng = np.random.default_rng(1)
    p = _frames(rng, 3, 4, 6)
    data = _stream(b"YUV4MPEG2 W6 H4 F25:1\n", p)[:-5]
    frames = video.Y4MReader(io.BytesIO(data)).frames()
    assert np.array_equal(next(frames), p[0]) and np.array_equal(next(frames), p[1])
    with pytest.raises(video.Y4MError, match="frame 2 is truncated"):
        next(frames)


def test_y4m_reader_is_lazy_on_an_endless_stream():
    """Frames are read one at a time: the first frames of a stream that never ends (a pipe) come out."""
    fb = ops.i420_frame_bytes(4, 6)

    class Endless(io.RawIOBase):
        def __init__(self):
            self.buf = b"YUV4MPEG2 W6 H4 F25:1\n"
            self.k = 0

        def readable(self):
            return True

        def readinto(self, b):
            while len(self.buf) < len(b):
                self.buf += b"FRAME\n" + bytes([self.k % 256]) * fb
                self.k += 1
            n = len(b)
            b[:n], self.buf = self.buf[:n], self.buf[n:]
            return n

    r = video.Y4MReader(io.BufferedReader(Endless(), buffer_size=4096))
    got = list(itertools.islice(r.frames(), 5))
    assert [int(f[0]) for f in got] == [0, 1, 2, 3, 4] and all(f.size == fb for f in got)


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("siting", ["jpeg", "mpeg2"])
def test_i420_to_image_matches_the_numpy_contract(dev, siting):
    rng = np.random.default_rng(2)
    for (h, w), matrix, full in (((5, 7), "bt601", False), ((6, 9), "bt709", True), ((1, 3), "bt709", False), ((4, 4), "bt601", True)):
        fr = _frames(rng, 2, h, w)
        got = ops.i420_to_image(torch.from_numpy(fr).to(dev), h, w, siting, matrix, full)
        assert got.shape == (2, 3, h, w) and got.dtype == torch.float32
        want = np_decode(fr, h, w, "420", siting, matrix, full)
        err = float(np.abs(got.cpu().double().numpy() - want).max())
        assert err < 2e-6, (h, w, matrix, full, err)
    with pytest.raises(ValueError):
        ops.i420_to_image(torch.from_numpy(_frames(rng, 1, 4, 4)).to(dev), 4, 5)


# zero weights and biases of +-20 / 0 make tanh exactly -1, 0 or 1 per channel: the codes are the textbook ones
TEXTBOOK = [   # (matrix, full, (R, G, B) signs, (Y, Cb, Cr))
    ("bt601", False, (1, 1, 1), (235, 128, 128)), ("bt601", False, (-1, -1, -1), (16, 128, 128)),
    ("bt601", False, (1, -1, -1), (81, 90, 240)), ("bt709", False, (1, -1, -1), (63, 102, 240)),
    ("bt601", True, (1, 1, 1), (255, 128, 128)), ("bt601", True, (-1, -1, -1), (0, 128, 128)),
    ("bt709", True, (-1, -1, 1), (18, 255, 116)),
]
HEADS = [("f32", 16, "conv_igemm_kernel<f32,8,16,4,1,16,1,1,0>"), ("f16", 64, "conv64_thin_kernel"),
         ("x3", 64, "conv64_thin_kernel<x3>")]


@pytest.mark.parametrize("cdn, cin, kernel", HEADS, ids=[h[0] for h in HEADS])
def test_i420_head_epilogue_textbook_codes(dev, cdn, cin, kernel, monkeypatch):
    monkeypatch.setenv("FSR_PERSIST_CUS", "3")        # persistent kernels: tile ranges straddle image borders
    cd = ops.Compute(cdn)
    n, h, w = 2, 6, 18                                   # partial tiles at the right and bottom edges
    x = ops.to_storage(cd, torch.randn(n, h, w, cin)).to(dev)
    wpk = ops.packed_filter(cd, torch.zeros(3, cin, 3, 3).to(dev), L.PACK_FWD, cin)
    for matrix, full, signs, codes in TEXTBOOK:
        bias = torch.tensor([20.0 * s for s in signs]).to(dev)
        out, _, _ = ops.conv3x3_raw(cd, x, wpk, 3, bias=bias, act=L.ACT_TANH, out_f32=True,
                                    out_i420=(ops.yuv_matrix_code(matrix), int(full)))
        assert L.lib().fsr_last_kernel().decode() == kernel, L.lib().fsr_last_kernel()
        assert out.dtype == torch.uint8 and out.shape == (n, h * w * 3 // 2)
        o = out.cpu().numpy()
        plane = h * w
        for name, lo, hi, code in (("Y", 0, plane, codes[0]), ("Cb", plane, plane * 5 // 4, codes[1]),
                                   ("Cr", plane * 5 // 4, plane * 3 // 2, codes[2])):
            assert (o[:, lo:hi] == code).all(), (cdn, matrix, full, signs, name, np.unique(o[:, lo:hi]))
        assert np.array_equal(o, np_encode(np.broadcast_to(np.array(signs, float)[None, :, None, None], (n, 3, h, w)), "420", matrix, full))
    # refused: odd output extents, other channel counts, tensors the epilogue does not write
    x_odd = ops.to_storage(cd, torch.randn(1, 5, 6, cin)).to(dev)
    with pytest.raises(L.FsrError, match="even output extents"):
        ops.conv3x3_raw(cd, x_odd, wpk, 3, bias=bias, act=L.ACT_TANH, out_f32=True, out_i420=(0, 0))
    with pytest.raises(L.FsrError, match="I420"):
        ops.conv3x3_raw(cd, x, wpk, 3, act=L.ACT_NONE, out_f32=True, out_i420=(0, 0))
    with pytest.raises(L.FsrError, match="colour matrix"):
        ops.conv3x3_raw(cd, x, wpk, 3, bias=bias, act=L.ACT_TANH, out_f32=True, out_i420=(2, 0))


def test_forward_yuv420_small_f32_generator(dev, pkg):
    """The whole Generator.forward_yuv420 (decode kernel, network, I420 head epilogue) against the numpy encode of the same
    model's float forward() on the device-decoded frames: only float32 / float64 rounding ties may differ."""
    G = _tiny(pkg, dev)
    rng = np.random.default_rng(3)
    h, w = 3, 5
    fr = torch.from_numpy(_frames(rng, 2, h, w)).to(dev)
    for matrix, full, out_matrix, out_full in (("bt601", False, None, None), ("bt709", True, "bt601", False)):
        got = G.forward_yuv420(fr, h, w, siting="mpeg2", matrix=matrix, full_range=full, out_matrix=out_matrix, out_full_range=out_full)
        assert got.dtype == torch.uint8 and got.shape == (2, ops.i420_frame_bytes(4 * h, 4 * w))
        with torch.no_grad():
            t = G(ops.i420_to_image(fr, h, w, "mpeg2", matrix, full)).cpu().numpy()
        want = np_encode(t, "420", out_matrix or matrix, full if out_full is None else out_full)
        assert_codes_close(got.cpu().numpy(), want, 1e-3)
    with pytest.raises(ValueError):
        G.forward_yuv420(fr, h, w, matrix="bt2020")


# ---------------------------------------------------------------------------------------------------- GPU: shipped weights
HEAD_KERNEL = {"f32": "conv_igemm_kernel<f32,8,16,4,1,16,1,1,0>", "f16": "conv64_thin_kernel", "bf16": "conv64_thin_kernel",
               "x3": "conv64_thin_kernel<x3>"}


@pytest.mark.gpu
@pytest.mark.parametrize("cdn", ["f32", "f16", "bf16", "x3"])
def test_forward_yuv420_shipped_weights_gpu(pkg, cdn, monkeypatch):
    dev = select("hip")
    monkeypatch.setenv("FSR_PERSIST_CUS", "5")          # tile ranges of the persistent head straddle image borders
    G = _shipped(pkg, dev, cdn)
    rng = np.random.default_rng(4)
    h, w = 23, 37                                        # odd: partial output tiles at the right and bottom edges
    fr = torch.from_numpy(_frames(rng, 3, h, w)).to(dev)
    got = G.forward_yuv420(fr, h, w, siting="jpeg", matrix="bt601", full_range=False, out_matrix="bt709").cpu().numpy()
    assert L.lib().fsr_last_kernel().decode() == HEAD_KERNEL[cdn], L.lib().fsr_last_kernel()
    assert got.shape == (3, ops.i420_frame_bytes(4 * h, 4 * w))
    with torch.no_grad():
        t = G(ops.i420_to_image(fr, h, w, "jpeg", "bt601", False)).cpu().numpy()
    assert_codes_close(got, np_encode(t, "420", "bt709", False), 1e-3)
    if cdn == "f32":
        # and against the CPU oracle on the numpy decode (host and device tanh differ by an ulp: 1 code on at most 2 %)
        sd = sd_from(load_npz("g_model_pt.npz"), "sd.")
        x = torch.from_numpy(np_decode(fr.cpu().numpy(), h, w, "420", "jpeg", "bt601", False)).float()
        want = np_encode(O.generator_forward(sd, x).numpy(), "420", "bt709", False)
        assert_codes_close(got, want, 2e-2)


@pytest.mark.gpu
def test_pipeline_yuv420_mixed_shapes_ragged_tail_gpu(pkg):
    """InferencePipeline.run_yuv420: full batches as graph replays, the tail eagerly; every frame byte-identical to a single
    forward_yuv420 call, graph replay identical to eager launches; I420 plans never collide with RGB plans of the same shape."""
    dev = select("hip")
    G = _shipped(pkg, dev, "f16")
    rng = np.random.default_rng(5)
    h, w = 17, 29
    frames = list(_frames(rng, 7, h, w))
    colour = dict(siting="mpeg2", matrix="bt709", full_range=True, out_matrix="bt601", out_full_range=False)
    pipe = pkg.InferencePipeline(G, dev, batch=3, depth=2)
    outs = list(pipe.run_yuv420(frames, h, w, **colour))
    assert len(outs) == 7
    key = ("i420", h, w, "mpeg2", "bt709", True, "bt601", False)
    assert list(pipe._plans) == [key] and all(sl is not None and sl.graph is not None for sl in pipe._plans[key])
    # RGB frames of the same (h, w) get their own plan, keyed (h, w) as before
    rgb = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(3)]
    list(pipe.run(rgb))
    assert sorted(map(str, pipe._plans)) == sorted(map(str, [key, (h, w)]))
    eager = pkg.InferencePipeline(G, dev, batch=3, depth=2, use_graph=False)
    outs_eager = list(eager.run_yuv420((bytes(f) for f in frames), h, w, **colour))
    for f, y, ye in zip(frames, outs, outs_eager):
        one = G.forward_yuv420(torch.from_numpy(f).unsqueeze(0).to(dev), h, w, **colour)[0].cpu().numpy()
        assert np.array_equal(y, one) and np.array_equal(ye, one)
    # a second shape through the same pipeline
    h2, w2 = 8, 12
    more = list(_frames(rng, 3, h2, w2))
    outs2 = list(pipe.run_yuv420(more, h2, w2))
    for f, y in zip(more, outs2):
        assert np.array_equal(y, G.forward_yuv420(torch.from_numpy(f).unsqueeze(0).to(dev), h2, w2)[0].cpu().numpy())


@pytest.mark.gpu
def test_video_cli_streams_y4m_through_pipes_gpu(tmp_path):
    dev = select("hip")
    sd = sd_from(load_npz("g_model_pt.npz"), "sd.")
    (tmp_path / "models").mkdir()
    (tmp_path / "configs").mkdir()
    torch.save({"_orig_mod." + k: v for k, v in sd.items()}, tmp_path / "models" / "model.pt")
    (tmp_path / "configs" / "config.yaml").write_text("generator:\n  n_filters: 64\n  n_layers: 8\ntraining:\n  compute_dtype: f16\n")
    rng = np.random.default_rng(6)
    h, w, nf = 9, 14, 5
    frames = _frames(rng, nf, h, w)
    data = _stream(b"YUV4MPEG2 W14 H9 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n", frames, frame_line=b"FRAME Ixyz\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "video.py"), "--input", "-", "--output", "-", "--batch", "2",
                        "--matrix", "bt709"], input=data, capture_output=True, cwd=tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = video.Y4MReader(io.BytesIO(r.stdout))
    assert (out.width, out.height, out.frame_rate, out.aspect, out.interlace, out.siting, out.colour_range) == \
        (56, 36, "30000:1001", "1:1", "p", "jpeg", "limited")
    got = list(out.frames())
    assert len(got) == nf
    G = importlib.import_module("fast-srgan_amd.inference").load_generator(
        importlib.import_module("fast-srgan_amd.config").load_config(str(tmp_path / "configs" / "config.yaml")),
        str(tmp_path / "models" / "model.pt"), dev)
    want = G.forward_yuv420(torch.from_numpy(frames[:1]).to(dev), h, w, matrix="bt709")[0].cpu().numpy()
    assert np.array_equal(got[0], want)
