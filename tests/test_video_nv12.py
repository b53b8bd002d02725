"""Video: semi-planar 4:2:0 frames in and out (NV12, P010, P012, P016), and raw-stream input and output.

Layout "nv12": the Y plane h x w, then ONE plane of ceil(h/2) rows of ceil(w/2) (Cb, Cr) pairs, Cb first.  Depth 8: one byte per sample
(NV12).  Depth 9..16: two little-endian bytes per sample with the code in the HIGH `depth` bits (P010, P012, P016): zero low bits on
output, ignored low bits on input.  The colour arithmetic is the planar paths' in every detail, so a semi-planar payload is a fixed
rearrangement of the planar one: `nv12()` below restates that rearrangement in numpy, and every comparison of a semi-planar path with
its planar twin is bit equality (torch.equal / np.array_equal) -- no tolerance.  The planar twins are pinned to the numpy contract by
test_video.py, test_video_deep.py and test_video_chroma.py; one decode and one encode case here go against that contract directly, at
the planar tests' own bounds."""
import ctypes
import importlib
import io

import numpy as np
import pytest
import torch

from backend import BACKENDS, L, ops, select
from conftest import load_npz, sd_from
from yuv_contract import CAP, _cli, _shipped, _stream, _tiny, assert_codes_close, from_payload, np_decode, np_encode, ns, samples_of, to_payload

video = importlib.import_module("fast-srgan_amd.video")
inference = importlib.import_module("fast-srgan_amd.inference")

COLOURS = [(m, f) for m in ("bt601", "bt709") for f in (False, True)]


# ---------------------------------------------------------------------------------------------------- 1. the interleave, in numpy
def nv12(payload, h, w, d=8):
    """(N, bytes) uint8 planar 4:2:0 payloads at depth d -> the semi-planar payloads: Y unchanged, Cb / Cr zipped into pairs, and for
    d > 8 every code moved to the high bits of its 16-bit word (<< (16 - d))."""
    codes = from_payload(np.asarray(payload), d)
    n, ch, cw = codes.shape[0], (h + 1) // 2, (w + 1) // 2
    assert codes.shape[1] == h * w + 2 * ch * cw
    y, cb, cr = codes[:, :h * w], codes[:, h * w:h * w + ch * cw], codes[:, h * w + ch * cw:]
    semi = np.concatenate([y, np.stack([cb, cr], axis=2).reshape(n, 2 * ch * cw)], axis=1)
    return to_payload(semi << (16 - d) if d > 8 else semi, d)


def _nv12_t(t, h, w, d=8):
    """nv12() of a device tensor of payloads, as a numpy array."""
    return nv12(t.cpu().numpy(), h, w, d)


def _rand_420(rng, n, h, w, d):
    return to_payload(rng.integers(0, 2 ** d, size=(n, samples_of(h, w, "420"))), d)


def _enc_input(shape, seed=0):
    """t uniform in [-1.1, 1.1] (both clamps act), NHWC float32."""
    n, h, w = shape
    g = torch.Generator().manual_seed(1000 * seed + 100 * h + w)
    return (torch.rand(n, h, w, 3, generator=g) * 2.2 - 1.1).contiguous()


def _kernel():
    return L.lib().fsr_last_kernel().decode()


@pytest.fixture(params=BACKENDS)
def dev(request):
    return select(request.param)


def test_the_interleave_helper():
    p = np.arange(6, dtype=np.uint8)[None]                                  # 2 x 2: Y0..Y3, Cb, Cr
    assert nv12(p, 2, 2).tolist() == [[0, 1, 2, 3, 4, 5]]
    p = np.arange(4 * 2 + 4, dtype=np.uint8)[None]                          # 2 x 4: Y0..Y7, Cb0 Cb1, Cr0 Cr1
    assert nv12(p, 2, 4).tolist() == [[0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 9, 11]]
    p = to_payload(np.array([[1, 2, 3, 1023, 5, 6]]), 10)
    assert from_payload(nv12(p, 2, 2, 10), 10).tolist() == [[64, 128, 192, 1023 * 64, 5 * 64, 6 * 64]]
    assert nv12(p, 2, 2, 10).shape == p.shape and nv12(to_payload(np.arange(17)[None], 8), 3, 3).shape == (1, 17)   # 9 + 2 * 4


# ---------------------------------------------------------------------------------------------------- 2. decode
DEC_SHAPES = ((5, 7), (6, 9), (1, 3), (3, 1), (2, 2), (4, 4), (6, 1030))


@pytest.mark.parametrize("d", [8, 10, 16])
def test_decode_equals_the_planar_decode(dev, d):
    rng = np.random.default_rng(60 + d)
    for h, w in DEC_SHAPES:
        fr = _rand_420(rng, 2, h, w, d)
        x, xs = torch.from_numpy(fr).to(dev), torch.from_numpy(nv12(fr, h, w, d)).to(dev)
        assert xs.shape[1] == ops.yuv_frame_bytes(h, w, "420", d, "nv12") == ops.yuv_frame_bytes(h, w, "420", d)
        for siting in ("jpeg", "mpeg2"):
            for matrix, full in COLOURS:
                got = ops.yuv_to_image(xs, h, w, "420", siting, matrix, full, depth=d, layout="nv12")
                assert _kernel() == "nv12_to_image_kernel<%s>" % ("u8" if d == 8 else "u16")
                want = ops.yuv_to_image(x, h, w, "420", siting, matrix, full, depth=d)
                assert got.shape == (2, 3, h, w) and got.dtype == torch.float32
                assert torch.equal(got, want), (d, h, w, siting, matrix, full)


def test_decode_ignores_the_low_bits_of_p010_and_meets_the_contract(dev):
    rng = np.random.default_rng(61)
    h, w, d = 5, 7, 10
    fr = _rand_420(rng, 2, h, w, d)
    clean = nv12(fr, h, w, d)
    dirty = to_payload(from_payload(clean, d) | rng.integers(0, 64, size=(2, samples_of(h, w))), d)
    assert not np.array_equal(clean, dirty)
    a = ops.yuv_to_image(torch.from_numpy(dirty).to(dev), h, w, depth=d, layout="nv12")
    assert torch.equal(a, ops.yuv_to_image(torch.from_numpy(clean).to(dev), h, w, depth=d, layout="nv12"))
    assert torch.equal(a, ops.yuv_to_image(torch.from_numpy(fr).to(dev), h, w, depth=d))
    # the independent check: the numpy decode of the planar codes, at the planar tests' bound
    for siting, (matrix, full) in (("jpeg", ("bt601", False)), ("mpeg2", ("bt709", True))):
        got = ops.yuv_to_image(torch.from_numpy(dirty).to(dev), h, w, "420", siting, matrix, full, depth=d, layout="nv12")
        err = float(np.abs(got.cpu().double().numpy() - np_decode(from_payload(fr, d), h, w, "420", siting, matrix, full, d)).max())
        print("P010 decode against the contract: max abs error %.3g" % err)
        assert err < 2e-6, err
    with pytest.raises(ValueError):                                         # the payload size is checked as for planar
        ops.yuv_to_image(torch.from_numpy(clean[:, :-2].copy()).to(dev), h, w, depth=d, layout="nv12")


# ---------------------------------------------------------------------------------------------------- 3. encode
ENC_SHAPES = ((2, 2, 2), (2, 4, 6), (1, 6, 10), (1, 8, 1028), (1, 2, 4098))      # (n, h, w): widths = 0 and = 2 mod 4


@pytest.mark.parametrize("d", [8, 10, 12, 16])
def test_encode_equals_the_interleaved_planar_encode(dev, d):
    for shape in ENC_SHAPES:
        n, h, w = shape
        t = _enc_input(shape).to(dev)
        for matrix, full in COLOURS:
            got = ops.image_to_yuv(t, "420", matrix, full, depth=d, layout="nv12")
            assert _kernel() == "image_to_nv12_kernel<%s>" % ("u8" if d == 8 else "u16")
            assert got.dtype == torch.uint8 and got.shape == (n, ops.yuv_frame_bytes(h, w, "420", d, "nv12"))
            want = _nv12_t(ops.image_to_yuv(t, "420", matrix, full, depth=d), h, w, d)
            assert np.array_equal(got.cpu().numpy(), want), (d, shape, matrix, full)
            if d > 8:                                                       # the low 16 - d bits are zero
                assert not (from_payload(got.cpu().numpy(), d) & ((1 << (16 - d)) - 1)).any()


@pytest.mark.parametrize("d", [8, 10, 16])
def test_encode_meets_the_numpy_contract(dev, d):
    """The independent check: the semi-planar encode, un-shifted and de-interleaved by plain indexing, against np_encode at CAP[d]."""
    got, want = [], []
    for shape in ((2, 16, 24), (1, 6, 10)):
        n, h, w = shape
        t = _enc_input(shape, seed=1)
        for matrix, full in COLOURS:
            out = from_payload(ops.image_to_yuv(t.to(dev), "420", matrix, full, depth=d, layout="nv12").cpu().numpy(), d) >> (16 - d if d > 8 else 0)
            uv = out[:, h * w:].reshape(n, -1, 2)
            got.append(np.concatenate([out[:, :h * w], uv[:, :, 0], uv[:, :, 1]], axis=1).reshape(-1))
            want.append(np_encode(t.numpy().transpose(0, 3, 1, 2), "420", matrix, full, d).reshape(-1))
    assert_codes_close(np.concatenate(got), np.concatenate(want), CAP[d])


@pytest.mark.gpu
def test_encode_grid_stride_wrap_gpu():
    """More 4 x 2 units than the 4096 x 256 threads of the capped grid (2050 x 4098: 1 050 625 units), so threads take a second unit;
    the shapes of the test above end inside the first pass."""
    dev = select("hip")
    h, w = 2050, 4098
    t = (torch.rand(1, h, w, 3, generator=torch.Generator().manual_seed(3)) * 2.2 - 1.1).to(dev)
    got = ops.image_to_yuv(t, layout="nv12")
    assert np.array_equal(got.cpu().numpy(), _nv12_t(ops.image_to_yuv(t), h, w))


# ---------------------------------------------------------------------------------------------------- 4. the head's epilogue
HEADS = [("f32", 16, "conv_igemm_kernel<f32,8,16,4,1,16,1,1,0>"), ("f16", 64, "conv64_thin_kernel"), ("x3", 64, "conv64_thin_kernel<x3>")]


@pytest.mark.parametrize("cdn, cin, kernel", HEADS, ids=[h[0] for h in HEADS])
def test_head_epilogue_kernels(dev, cdn, cin, kernel, monkeypatch):
    """One launch of each kernel that carries the epilogue, random filters: FSR_OUT_NV12 is the interleave of FSR_OUT_I420."""
    monkeypatch.setenv("FSR_PERSIST_CUS", "3")        # persistent kernels: tile ranges straddle image borders
    cd = ops.Compute(cdn)
    g = torch.Generator().manual_seed(7)
    for n, h, w in ((2, 6, 18), (1, 36, 28)):         # partial tiles at the right and bottom edges; more than one tile each way
        x = ops.to_storage(cd, torch.randn(n, h, w, cin, generator=g)).to(dev)
        wpk = ops.packed_filter(cd, (torch.randn(3, cin, 3, 3, generator=g) * 0.1).to(dev), L.PACK_FWD, cin)
        bias = torch.tensor([0.3, -0.2, 0.1]).to(dev)
        for matrix, full in ((0, 0), (1, 1)):
            a, _, _ = ops.conv3x3_raw(cd, x, wpk, 3, bias=bias, act=L.ACT_TANH, out_f32=True, out_i420=(matrix, full))
            assert _kernel() == kernel
            b, _, _ = ops.conv3x3_raw(cd, x, wpk, 3, bias=bias, act=L.ACT_TANH, out_f32=True, out_i420=(matrix, full, 1))
            assert _kernel() == kernel + "[nv12]"
            assert b.dtype == torch.uint8 and b.shape == a.shape == (n, h * w * 3 // 2)
            assert len(np.unique(a.cpu().numpy()[:, h * w:])) > 4           # (a frame of one colour would show nothing)
            assert np.array_equal(b.cpu().numpy(), _nv12_t(a, h, w))


def _forward_pair(G, x, h, w, dev, **kw):
    """forward_yuv with out_layout "nv12" and its planar twin, as numpy payloads, and the kernel the semi-planar call ended on."""
    got = G.forward_yuv(x, h, w, out_layout="nv12", **kw)
    kernel = _kernel()
    return got.cpu().numpy(), G.forward_yuv(x, h, w, out_layout="planar", **kw).cpu().numpy(), kernel


def _check_head_route(G, dev, head_kernel):
    rng = np.random.default_rng(62)
    for (h, w), n, colour in (((6, 10), 1, dict()), ((9, 7), 2, dict(matrix="bt709", out_matrix="bt601")),
                              ((9, 7), 1, dict(full_range=True, out_matrix="bt709"))):
        fr = _rand_420(rng, n, h, w, 8)
        got, want, kernel = _forward_pair(G, torch.from_numpy(fr).to(dev), h, w, dev, **colour)
        assert kernel == head_kernel + "[nv12]", kernel
        assert got.shape == (n, ops.yuv_frame_bytes(4 * h, 4 * w, "420", 8, "nv12"))
        assert np.array_equal(got, nv12(want, 4 * h, 4 * w)), (h, w, colour)
    # semi-planar on the input as well: the same frames, so the same bytes
    h, w = 9, 7
    fr = _rand_420(rng, 2, h, w, 8)
    got, want, kernel = _forward_pair(G, torch.from_numpy(nv12(fr, h, w)).to(dev), h, w, dev, layout="nv12")
    assert kernel == head_kernel + "[nv12]"
    assert np.array_equal(want, G.forward_yuv(torch.from_numpy(fr).to(dev), h, w).cpu().numpy())     # (nv12 in, planar out)
    assert np.array_equal(got, nv12(want, 4 * h, 4 * w))
    # out_layout is independent of layout and defaults to it
    x = torch.from_numpy(nv12(fr, h, w)).to(dev)
    assert torch.equal(G.forward_yuv(x, h, w, layout="nv12"), G.forward_yuv(x, h, w, layout="nv12", out_layout="nv12"))
    assert torch.equal(G.forward_yuv(x, h, w, layout="nv12", out_layout="planar"), G.forward_yuv(torch.from_numpy(fr).to(dev), h, w))


def test_forward_yuv_head_epilogue_tiny(dev, pkg):
    _check_head_route(_tiny(pkg, dev), dev, HEADS[0][2])


@pytest.mark.gpu
def test_forward_yuv_head_epilogue_shipped_f16_gpu(pkg, monkeypatch):
    dev = select("hip")
    monkeypatch.setenv("FSR_PERSIST_CUS", "5")          # tile ranges of the persistent head straddle image borders
    _check_head_route(_shipped(pkg, dev, "f16"), dev, "conv64_thin_kernel")


def test_forward_yuv_banded_equals_whole(dev, pkg):
    G = _tiny(pkg, dev)
    h, w = 12, 8
    x = torch.from_numpy(_rand_420(np.random.default_rng(63), 2, h, w, 8)).to(dev)
    whole = G.forward_yuv(x, h, w, out_layout="nv12")
    assert _kernel().endswith("[nv12]")
    banded = G.forward_yuv(x, h, w, out_layout="nv12", bands=2)
    assert torch.equal(whole, banded)
    assert np.array_equal(whole.cpu().numpy(), _nv12_t(G.forward_yuv(x, h, w, bands=2), 4 * h, 4 * w))


def test_banded_equals_whole_f16_head_emu(pkg):
    """The 16-bit head kernel under the banded tail, on the emulator (a random 64-filter generator, as test_bands.py's)."""
    dev = select("emu")
    torch.manual_seed(11)
    G = pkg.Generator(ns(n_filters=64, n_layers=1), compute_dtype="f16").to(dev).eval()
    h, w = 9, 7
    x = torch.from_numpy(_rand_420(np.random.default_rng(64), 1, h, w, 8)).to(dev)
    whole = G.forward_yuv(x, h, w, out_layout="nv12")
    assert _kernel() == "conv64_thin_kernel[nv12]"
    assert torch.equal(whole, G.forward_yuv(x, h, w, out_layout="nv12", bands=4))
    assert np.array_equal(whole.cpu().numpy(), _nv12_t(G.forward_yuv(x, h, w), 4 * h, 4 * w))


# ---------------------------------------------------------------------------------------------------- 5. resample
@pytest.mark.parametrize("src, dst, form", [((5, 7), (10, 14), 5), ((12, 8), (6, 4), 9), ((4, 5), (10, 14), 5), ((11, 7), (6, 4), 9)],
                         ids=lambda v: str(v) if isinstance(v, int) else "%dx%d" % v)
def test_resample_equals_the_interleaved_planar_resample(dev, src, dst, form):
    (h, w), (oh, ow) = src, dst
    t = _enc_input((2, h, w), seed=2).to(dev)
    for d in (8, 10):
        for matrix, full in (("bt601", False), ("bt709", True)):
            got = ops.resample_image(t, oh, ow, "i420", matrix, full, depth=d, layout="nv12")
            assert _kernel() == "resample_kernel<nv12,%d,%s>" % (form, "u8" if d == 8 else "u16")
            assert got.dtype == torch.uint8 and got.shape == (2, ops.yuv_frame_bytes(oh, ow, "420", d, "nv12"))
            want = ops.resample_image(t, oh, ow, "i420", matrix, full, depth=d)
            assert _kernel() == "resample_kernel<i420,%d%s>" % (form, "" if d == 8 else ",u16")
            assert np.array_equal(got.cpu().numpy(), _nv12_t(want, oh, ow, d)), (d, matrix, full)


def test_resample_identity_taps_reproduce_the_encode(dev):
    for shape in ((2, 6, 10), (1, 4, 70), (1, 34, 132)):                    # across the 64-column tile border; more than one tile of rows
        n, h, w = shape
        t = _enc_input(shape, seed=3).to(dev)
        for d in (8, 10):
            a = ops.image_to_yuv(t, "420", "bt709", True, depth=d, layout="nv12")
            b = ops.resample_image(t, h, w, "i420", "bt709", True, depth=d, layout="nv12")
            assert _kernel().startswith("resample_kernel<nv12,5,")
            assert a.shape == b.shape and torch.equal(a, b), (shape, d)


# ---------------------------------------------------------------------------------------------------- 6. deep and mixed routes
def test_forward_yuv_deep_and_resized_routes(dev, pkg):
    G = _tiny(pkg, dev)
    rng = np.random.default_rng(65)
    h, w = 5, 7
    fr10, fr8 = _rand_420(rng, 2, h, w, 10), _rand_420(rng, 2, h, w, 8)
    x10 = torch.from_numpy(fr10).to(dev)
    # P010 in, P010 out: the float head and the encode kernel
    got = G.forward_yuv(torch.from_numpy(nv12(fr10, h, w, 10)).to(dev), h, w, depth=10, layout="nv12", out_depth=10, out_layout="nv12")
    assert _kernel() == "image_to_nv12_kernel<u16>"
    assert np.array_equal(got.cpu().numpy(), _nv12_t(G.forward_yuv(x10, h, w, depth=10, out_depth=10), 4 * h, 4 * w, 10))
    # 8 bits in, P016 out, another matrix
    got = G.forward_yuv(torch.from_numpy(fr8).to(dev), h, w, out_depth=16, out_matrix="bt709", out_layout="nv12")
    assert _kernel() == "image_to_nv12_kernel<u16>"
    assert np.array_equal(got.cpu().numpy(), _nv12_t(G.forward_yuv(torch.from_numpy(fr8).to(dev), h, w, out_depth=16, out_matrix="bt709"),
                                                     4 * h, 4 * w, 16))
    # out_size: the fused resize + encode, 8 and 10 bits, an up- and a down-scale of the head output
    for od, size in ((8, (14, 30)), (10, (14, 30)), (8, (30, 22))):
        got = G.forward_yuv(torch.from_numpy(nv12(fr8, h, w)).to(dev), h, w, layout="nv12", out_size=size, out_depth=od)
        assert _kernel().startswith("resample_kernel<nv12,")
        want = G.forward_yuv(torch.from_numpy(fr8).to(dev), h, w, out_size=size, out_depth=od)
        assert np.array_equal(got.cpu().numpy(), _nv12_t(want, size[0], size[1], od)), (od, size)
    # refusals name the rule
    for bad in (dict(chroma="422", layout="nv12"), dict(out_chroma="444", out_layout="nv12"), dict(chroma="444", out_chroma="420", layout="nv12")):
        with pytest.raises(ValueError, match="nv12.*420"):
            G.forward_yuv(x10, h, w, **bad)
    with pytest.raises(ValueError, match="layout"):
        G.forward_yuv(x10, h, w, layout="nv21")


# ---------------------------------------------------------------------------------------------------- 7. host
def test_frame_bytes_and_layout_refusals(dev):
    for h, w in ((5, 7), (6, 10), (1, 1)):
        for d in (8, 10, 16):
            assert ops.yuv_frame_bytes(h, w, "420", d, "nv12") == ops.yuv_frame_bytes(h, w, "420", d) == ops.yuv_frame_bytes(h, w, "420", d, "planar")
    assert ops.yuv_frame_bytes(5, 7, layout="nv12") == 59
    for c in ("422", "444"):
        with pytest.raises(ValueError, match="nv12.*420"):
            ops.yuv_frame_bytes(4, 4, c, 8, "nv12")
    with pytest.raises(ValueError, match="layout"):
        ops.yuv_frame_bytes(4, 4, "420", 8, "nv21")
    t = _enc_input((1, 4, 6)).to(dev)
    fr = torch.zeros((1, ops.yuv_frame_bytes(4, 6, "444")), dtype=torch.uint8, device=dev)
    for c in ("422", "444"):
        with pytest.raises(ValueError, match="nv12.*420"):
            ops.image_to_yuv(t, c, layout="nv12")
        with pytest.raises(ValueError, match="nv12.*420"):
            ops.resample_image(t, 8, 12, "i420", chroma=c, layout="nv12")
        with pytest.raises(ValueError, match="nv12.*420"):
            ops.yuv_to_image(fr, 4, 6, c, layout="nv12")
    for kind in ("f32", "u8"):
        with pytest.raises(ValueError, match="layout.*i420"):
            ops.resample_image(t, 8, 12, kind, layout="nv12")
    with pytest.raises((ValueError, L.FsrError), match="even output extents"):
        ops.image_to_yuv(_enc_input((1, 4, 5)).to(dev), layout="nv12")
    with pytest.raises((ValueError, L.FsrError), match="even output extents"):
        ops.resample_image(t, 7, 12, "i420", layout="nv12")


def test_raw_reader_and_writer():
    rng = np.random.default_rng(66)
    w, h = 6, 4
    assert set(video.RAW_FORMATS) == {"yuv420p", "nv12", "p010", "p012", "p016"} and video.FORMATS[0] == "y4m"
    for name, (layout, d, pix_fmt) in video.RAW_FORMATS.items():
        assert (layout, d) == {"yuv420p": ("planar", 8), "nv12": ("nv12", 8), "p010": ("nv12", 10), "p012": ("nv12", 12), "p016": ("nv12", 16)}[name]
        assert pix_fmt == (name if d == 8 else name + "le")
        fb = ops.yuv_frame_bytes(h, w, "420", d, layout)
        assert fb == 36 * (2 if d > 8 else 1)
        frames = [rng.integers(0, 256, size=fb, dtype=np.uint8) for _ in range(3)]
        out = io.BytesIO()
        wr = video.RawWriter(out, w, h, fb)
        for f in frames:
            wr.write_frame(f)
        assert out.getvalue() == b"".join(bytes(f) for f in frames)         # nothing but the payloads
        rd = video.RawReader(io.BytesIO(out.getvalue()), w, h, fb)
        assert (rd.width, rd.height, rd.frame_bytes) == (w, h, fb)
        back = list(rd.frames())
        assert len(back) == 3 and all(a.dtype == np.uint8 and np.array_equal(a, b) for a, b in zip(back, frames))
        with pytest.raises(video.Y4MError, match="does not match"):
            wr.write_frame(frames[0][:-1])
        with pytest.raises(video.Y4MError, match="frame 2 is truncated \\(%d of %d" % (fb - 5, fb)):
            list(video.RawReader(io.BytesIO(out.getvalue()[:-5]), w, h, fb).frames())
    assert list(video.RawReader(io.BytesIO(b""), w, h, 36).frames()) == []


def test_cli_format_rules():
    f = video.resolve_formats
    assert f("y4m", None, None, None) == ("y4m", None) and f("y4m", None, None, None, 10) == ("y4m", 10)
    assert f("nv12", None, None, None) == ("nv12", 8) and f("nv12", None, 10, None) == ("p010", 10) and f("p010", None, None, None) == ("p010", 10)
    assert f("p010", None, 8, None) == ("nv12", 8) and f("p016", None, 12, None) == ("p012", 12) and f("yuv420p", None, None, None) == ("yuv420p", 8)
    assert f("y4m", "p010", None, None, 8) == ("p010", 10) and f("nv12", "y4m", None, "444") == ("y4m", 8) and f("y4m", "nv12", None, None, 8) == ("nv12", 8)
    assert f("p010", "y4m", None, None) == ("y4m", 10) and f("yuv420p", "nv12", 8, "420") == ("nv12", 8)
    assert f("y4m", "nv12", None, None, 10) == ("nv12", 8)                  # a raw name fixes the depth, whatever the input's
    for args, msg in ((("y4m", "p010", 8, None), "contradicts.*p010"), (("nv12", "nv12", 10, None), "contradicts.*nv12"),
                      (("nv12", None, 14, None), "no raw semi-planar"),
                      (("yuv420p", None, 10, None), "yuv420p, 8 bits"), (("y4m", "nv12", None, "444"), "4:2:0 format")):
        with pytest.raises(ValueError, match=msg):
            f(*args)
    a = video.parser.parse_args(["--input", "-", "--output", "-"])
    assert (a.in_format, a.out_format, a.in_size, a.fps) == ("y4m", None, None, None)
    assert video.parse_size("1920x1080", "--in_size") == (1920, 1080) and video.parse_fps("30000:1001") == "30000:1001" and video.parse_fps("25") == "25:1"
    # refused before the input is opened
    none = ["--input", "/nonexistent.yuv", "--output", "/nonexistent/out.yuv"]
    with pytest.raises(SystemExit, match="needs --in_size"):
        video.main(none + ["--in_format", "nv12"])
    with pytest.raises(SystemExit, match="--out_depth 8 contradicts --out_format p010"):
        video.main(none + ["--out_format", "p010", "--out_depth", "8"])
    with pytest.raises(SystemExit, match="--out_depth 10 contradicts --out_format nv12"):
        video.main(none + ["--in_format", "nv12", "--in_size", "14x9", "--out_format", "nv12", "--out_depth", "10"])
    with pytest.raises(SystemExit, match="in_size must be WxH"):
        video.main(none + ["--in_format", "nv12", "--in_size", "14"])
    with pytest.raises(SystemExit, match="--in_size is for raw"):
        video.main(none + ["--in_size", "14x9"])
    with pytest.raises(SystemExit, match="fps"):
        video.main(none + ["--in_format", "nv12", "--in_size", "14x9", "--fps", "0"])
    with pytest.raises(SystemExit, match="4:2:0 format"):
        video.main(none + ["--out_format", "nv12", "--out_chroma", "444"])


def test_pipeline_refuses_layouts_before_it_allocates(pkg):
    G = pkg.Generator(ns(n_filters=64, n_layers=8), compute_dtype="f32")
    pipe = pkg.InferencePipeline(G, "cpu", batch=8)
    with pytest.raises(ValueError, match="nv12.*420"):
        pipe.run_yuv([], 8, 12, chroma="422", layout="nv12")
    with pytest.raises(ValueError, match="nv12.*420"):
        pipe.run_yuv([], 8, 12, out_chroma="444", out_layout="nv12")
    with pytest.raises(ValueError, match="layout"):
        pipe.run_yuv([], 8, 12, layout="nv21")
    assert not pipe._plans


@pytest.mark.gpu
def test_pipeline_run_yuv_layouts_gpu(pkg):
    dev = select("hip")
    G = _shipped(pkg, dev, "f16")
    rng = np.random.default_rng(67)
    h, w = 9, 14
    frames = _rand_420(rng, 5, h, w, 8)
    semi = list(nv12(frames, h, w))
    pipe = pkg.InferencePipeline(G, dev, batch=2, depth=2)
    outs = list(pipe.run_yuv(semi, h, w, layout="nv12", out_layout="nv12", matrix="bt709"))     # two graph batches and an eager tail
    key = ("i420", h, w, "jpeg", "bt709", False, "bt709", False, "layout", "nv12", "nv12")
    assert list(pipe._plans) == [key] and all(sl is not None and sl.graph is not None for sl in pipe._plans[key])
    want = G.forward_yuv(torch.from_numpy(np.stack(semi)).to(dev), h, w, layout="nv12", out_layout="nv12", matrix="bt709").cpu().numpy()
    assert len(outs) == 5 and all(np.array_equal(a, b) for a, b in zip(outs, want))
    planar = list(pipe.run_yuv(list(frames), h, w, matrix="bt709"))
    assert list(pipe._plans)[-1] == ("i420", h, w, "jpeg", "bt709", False, "bt709", False)      # planar / planar: the key it has always had
    assert all(np.array_equal(a, nv12(b[None], 4 * h, 4 * w)[0]) for a, b in zip(outs, planar))
    mixed = list(pipe.run_yuv(list(frames), h, w, out_layout="nv12", out_depth=10, matrix="bt709"))
    assert list(pipe._plans)[-1] == ("i420", h, w, "jpeg", "bt709", False, "bt709", False, "depth", 8, 10, "layout", "planar", "nv12")
    want10 = G.forward_yuv(torch.from_numpy(frames).to(dev), h, w, out_depth=10, matrix="bt709").cpu().numpy()
    assert all(np.array_equal(a, b) for a, b in zip(mixed, nv12(want10, 4 * h, 4 * w, 10)))


@pytest.fixture(scope="module")
def cli_dir(tmp_path_factory):
    """The tiny generator as the CLI loads one."""
    d = tmp_path_factory.mktemp("nv12_cli")
    sd = sd_from(load_npz("g_tiny.npz"), "sd.")
    (d / "models").mkdir()
    (d / "configs").mkdir()
    torch.save({"_orig_mod." + k: v for k, v in sd.items()}, d / "models" / "model.pt")
    (d / "configs" / "config.yaml").write_text("generator:\n  n_filters: 16\n  n_layers: 1\ntraining:\n  compute_dtype: f32\n")
    return d


CLI_H, CLI_W, CLI_N = 9, 14, 3
CLI_Y4M = b"YUV4MPEG2 W14 H9 F30000:1001 Ip C420jpeg XCOLORRANGE=LIMITED\n"


@pytest.fixture(scope="module")
def cli_ref(cli_dir):
    """(input payloads, the output payloads of the Y4M -> Y4M run): one CLI run shared by the tests below."""
    select("hip")
    frames = _rand_420(np.random.default_rng(68), CLI_N, CLI_H, CLI_W, 8)
    ref = list(video.Y4MReader(io.BytesIO(_cli(cli_dir, _stream(CLI_Y4M, frames)).stdout)).frames())
    assert len(ref) == CLI_N
    return frames, ref


def _joined(payloads):
    return b"".join(bytes(p) for p in payloads)


@pytest.mark.gpu
def test_video_cli_y4m_to_nv12_and_back_gpu(cli_dir, cli_ref):
    frames, ref = cli_ref
    h, w = CLI_H, CLI_W
    # Y4M in -> raw NV12 out: the interleave of the Y4M run's payloads, and nothing else in the stream
    r = _cli(cli_dir, _stream(CLI_Y4M, frames), "--out_format", "nv12")
    assert r.stdout == _joined(nv12(f[None], 4 * h, 4 * w)[0] for f in ref)
    assert b"-f rawvideo -pix_fmt nv12 -s 56x36 -r 30000/1001" in r.stderr and b"y4m -> nv12" in r.stderr
    # raw NV12 in -> Y4M out: the Y4M -> Y4M run, under the frame rate given
    r = _cli(cli_dir, _joined(nv12(frames, h, w)), "--in_format", "nv12", "--in_size", "14x9", "--fps", "30000:1001", "--out_format", "y4m")
    out = video.Y4MReader(io.BytesIO(r.stdout))
    assert (out.width, out.height, out.frame_rate, out.depth) == (56, 36, "30000:1001", 8)
    got = list(out.frames())
    assert len(got) == CLI_N and all(np.array_equal(a, b) for a, b in zip(got, ref))


@pytest.mark.gpu
def test_video_cli_raw_in_raw_out_gpu(cli_dir, cli_ref):
    """Raw in, raw out by default: NV12 stays NV12 (25 fps unless told), yuv420p stays planar."""
    frames, ref = cli_ref
    h, w = CLI_H, CLI_W
    r = _cli(cli_dir, _joined(nv12(frames, h, w)), "--in_format", "nv12", "--in_size", "14x9")
    assert r.stdout == _joined(nv12(f[None], 4 * h, 4 * w)[0] for f in ref)
    assert b"-pix_fmt nv12 -s 56x36 -r 25/1" in r.stderr and b"nv12 -> nv12" in r.stderr
    r = _cli(cli_dir, _joined(frames), "--in_format", "yuv420p", "--in_size", "14x9")
    assert r.stdout == _joined(ref) and b"-pix_fmt yuv420p" in r.stderr


@pytest.mark.gpu
def test_video_cli_nv12_to_p010_gpu(cli_dir, cli_ref):
    """--out_depth 10 on a raw NV12 input makes the output P010: the interleave of the planar 10-bit frames of the same model."""
    dev = select("hip")
    frames, _ = cli_ref
    h, w = CLI_H, CLI_W
    r = _cli(cli_dir, _joined(nv12(frames, h, w)), "--in_format", "nv12", "--in_size", "14x9", "--out_depth", "10")
    assert b"-pix_fmt p010le -s 56x36" in r.stderr and b"nv12 -> p010" in r.stderr
    G = inference.load_generator(importlib.import_module("fast-srgan_amd.config").load_config(str(cli_dir / "configs" / "config.yaml")),
                                 str(cli_dir / "models" / "model.pt"), dev)
    want = G.forward_yuv(torch.from_numpy(frames).to(dev), h, w, out_depth=10).cpu().numpy()
    assert r.stdout == _joined(nv12(want, 4 * h, 4 * w, 10))


# ---------------------------------------------------------------------------------------------------- 8. the C ABI
def test_c_abi_refusals(dev):
    """Every refusal returns -2 with a message, and nothing is launched: the kernel note stays what it was."""
    lib = L.lib()
    assert lib.fsr_version() == L.ABI_VERSION == 16 and (L.OUT_NV12, L.LAYOUT_PLANAR, L.LAYOUT_NV12) == (4, 0, 1)
    h, w = 4, 6
    t = _enc_input((1, h, w)).to(dev)
    out = torch.zeros((1, 2 * 3 * h * w + 2), dtype=torch.uint8, device=dev)
    img = torch.empty((1, h, w, 3), dtype=torch.float32, device=dev)
    ops.image_to_yuv(t)                                                     # a launch whose note the refused calls must leave alone
    note = _kernel()
    tp, op, ip = t.data_ptr(), out.data_ptr(), img.data_ptr()
    assert op % 2 == 0
    wy, ymin, ysize, ky = ops.aa_taps(h, 8, dev)
    wx, xmin, xsize, kx = ops.aa_taps(w, 12, dev)

    def rs(oh, ow, chroma, layout, depth, o):
        return lib.fsr_resample_image_yuv_ex(tp, 1, h, w, oh, ow, wy.data_ptr(), ymin.data_ptr(), ysize.data_ptr(), ky, wx.data_ptr(),
                                             xmin.data_ptr(), xsize.data_ptr(), kx, chroma, layout, 0, 0, depth, o, None)
    NV, C420 = L.LAYOUT_NV12, L.CHROMA_420
    cases = [
        # semi-planar with a chroma other than 4:2:0
        (lambda: lib.fsr_yuv_to_image_ex(op, ip, 1, h, w, L.CHROMA_422, NV, 0, 0, 0, 8, None), b"4:2:0"),
        (lambda: lib.fsr_yuv_to_image_ex(op, ip, 1, h, w, L.CHROMA_444, NV, 0, 0, 0, 8, None), b"4:2:0"),
        (lambda: lib.fsr_image_to_yuv_ex(tp, 1, h, w, L.CHROMA_444, NV, 0, 0, 8, op, None), b"4:2:0"),
        (lambda: rs(8, 12, L.CHROMA_422, NV, 8, op), b"4:2:0"),
        # an unknown layout or chroma
        (lambda: lib.fsr_yuv_to_image_ex(op, ip, 1, h, w, C420, 2, 0, 0, 0, 8, None), b"layout"),
        (lambda: lib.fsr_image_to_yuv_ex(tp, 1, h, w, C420, -1, 0, 0, 8, op, None), b"layout"),
        (lambda: rs(8, 12, 3, NV, 8, op), b"chroma"),
        # odd output extents
        (lambda: lib.fsr_image_to_yuv_ex(tp, 1, 3, 8, C420, NV, 0, 0, 8, op, None), b"even output extents"),
        (lambda: lib.fsr_image_to_yuv_ex(tp, 1, 4, 5, C420, NV, 0, 0, 8, op, None), b"even output extents"),
        (lambda: rs(7, 12, C420, NV, 8, op), b"even output extents"),
        (lambda: rs(8, 11, C420, NV, 10, op), b"even output extents"),
        # depth outside 8..16
        (lambda: lib.fsr_yuv_to_image_ex(op, ip, 1, h, w, C420, NV, 0, 0, 0, 7, None), b"depth"),
        (lambda: lib.fsr_yuv_to_image_ex(op, ip, 1, h, w, C420, NV, 0, 0, 0, 17, None), b"depth"),
        (lambda: lib.fsr_image_to_yuv_ex(tp, 1, h, w, C420, NV, 0, 0, 17, op, None), b"depth"),
        (lambda: rs(8, 12, C420, NV, 7, op), b"depth"),
        # a misaligned 16-bit payload
        (lambda: lib.fsr_yuv_to_image_ex(op + 1, ip, 1, h, w, C420, NV, 0, 0, 0, 10, None), b"aligned"),
        (lambda: lib.fsr_image_to_yuv_ex(tp, 1, h, w, C420, NV, 0, 0, 10, op + 1, None), b"aligned"),
        (lambda: rs(8, 12, C420, NV, 10, op + 1), b"aligned"),
        # what the planar calls refuse besides
        (lambda: lib.fsr_yuv_to_image_ex(op, ip, 1, h, w, C420, NV, 2, 0, 0, 8, None), b"siting"),
        (lambda: lib.fsr_image_to_yuv_ex(tp, 1, h, w, C420, NV, 2, 0, 8, op, None), b"colour matrix"),
    ]
    for i, (call, msg) in enumerate(cases):
        assert call() == -2, i
        assert msg in lib.fsr_last_error(), (i, lib.fsr_last_error())
        assert _kernel() == note, i
    # the planar layout through the _ex forms is the plain call
    assert lib.fsr_image_to_yuv_ex(tp, 1, h, w, C420, L.LAYOUT_PLANAR, 1, 1, 8, op, None) == 0
    assert torch.equal(out[0, :h * w * 3 // 2], ops.image_to_yuv(t, "420", "bt709", True)[0])


def test_c_abi_nv12_head_is_refused_where_the_i420_head_is(dev):
    cd = ops.Compute("f32")
    x = ops.to_storage(cd, torch.randn(1, 6, 6, 16)).to(dev)
    x_odd = ops.to_storage(cd, torch.randn(1, 5, 6, 16)).to(dev)
    wpk = ops.packed_filter(cd, torch.zeros(3, 16, 3, 3).to(dev), L.PACK_FWD, 16)
    wpk4 = ops.packed_filter(cd, torch.zeros(4, 16, 3, 3).to(dev), L.PACK_FWD, 16)
    bias = torch.zeros(3).to(dev)
    ops.image_to_yuv(_enc_input((1, 2, 2)).to(dev))
    note = _kernel()
    for kind in ((0, 0), (0, 0, 1)):                                        # FSR_OUT_I420, FSR_OUT_NV12: the same refusals
        for kw, xx, ww, cout, msg in ((dict(act=L.ACT_TANH, bias=bias), x_odd, wpk, 3, "even output extents"),
                                      (dict(act=L.ACT_NONE), x, wpk, 3, "3-channel tanh heads"),
                                      (dict(act=L.ACT_TANH), x, wpk4, 4, "3-channel tanh heads"),
                                      (dict(act=L.ACT_TANH, oscale=torch.ones(3).to(dev)), x, wpk, 3, "3-channel tanh heads"),
                                      (dict(act=L.ACT_TANH, stride=2), x, wpk, 3, "3-channel tanh heads")):
            with pytest.raises(L.FsrError, match=r"\(-2\).*" + msg):
                ops.conv3x3_raw(cd, xx, ww, cout, out_f32=True, out_i420=kind, **kw)
            assert _kernel() == note
        with pytest.raises(L.FsrError, match=r"\(-2\).*colour matrix"):
            ops.conv3x3_raw(cd, x, wpk, 3, act=L.ACT_TANH, bias=bias, out_f32=True, out_i420=(2,) + kind[1:])
    d = L.ConvDesc(cd.code, L.CONV_FWD, 1, 6, 6, 16, 6, 6, 3, 1, L.ACT_TANH, 0.0, 0, 0, 5, 0, 0, 0, 0, 0)      # past the last output kind
    out = torch.zeros(64, dtype=torch.uint8, device=dev)
    assert L.lib().fsr_conv3x3(ctypes.byref(d), x.data_ptr(), wpk.data_ptr(), None, None, None, None, 0.0, out.data_ptr(), None, None, None, None) == -2
    assert b"unknown output kind 5" in L.lib().fsr_last_error()
