"""Video: 4:2:2 and 4:4:4 frames in and out at 8 to 16 bits (Y4M C422, C444 and their pN forms).

The contract of DESIGN.md §6c for the two formats is restated in numpy (float64, tests/yuv_contract.py), independently of the code under test.
Storage: planar, Y h x w, then Cb, then Cr of h x ceil(w/2) (4:2:2) or h x w (4:4:4); 1 byte per sample at depth 8, 2 little-endian
above.  Matrices, ranges, codes at depth d and the clamp are those of 4:2:0:
  limited range: Y = (16 + 219 E_Y) 2^(d-8), C = (128 + 224 E_C) 2^(d-8);  full range: Y = (2^d - 1) E_Y, C = 2^(d-1) + (2^d - 1) E_C;
  encode: code = clamp(floor(v + 0.5), 0, 2^d - 1).
Decode: 4:4:4 no interpolation; 4:2:2 chroma interpolated horizontally only, linearly with edge clamp -- luma column x reads chroma at
x / 2 ("mpeg2", what C422 means) or (x - 1/2) / 2 ("jpeg"); inverse matrix, R, G, B clamped to [0, 1], output 2c - 1.
Encode of c = clamp((t + 1) / 2, 0, 1): Y per pixel; 4:4:4 Cb, Cr per pixel; 4:2:2 chroma column j co-sited with luma column 2j:
s = (d[2j-1] + d[2j+1]) + 2 d[2j] (d = B - E_Y or R - E_Y, columns -1 and w clamped), E_C = s * 0.25 / (2 (1 - K))."""
import importlib
import io
import os

import numpy as np
import pytest
import torch

from backend import BACKENDS, L, ops, select
from conftest import load_npz, sd_from
from yuv_contract import (CAP, _aa_matrix, _cli, _shipped, _stream, _tiny, assert_codes_close, chroma_w, from_payload, np_decode, np_encode,
                          ns, samples_of, to_payload)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
video = importlib.import_module("fast-srgan_amd.video")
inference = importlib.import_module("fast-srgan_amd.inference")

COLOURS = [(m, f) for m in ("bt601", "bt709") for f in (False, True)]
ALL3 = ("420", "422", "444")


def _rand_payload(rng, n, h, w, chroma, d):
    return to_payload(rng.integers(0, 2 ** d, size=(n, samples_of(h, w, chroma))), d)


def _kernel():
    return L.lib().fsr_last_kernel().decode()


@pytest.fixture(params=BACKENDS)
def dev(request):
    return select(request.param)


# ---------------------------------------------------------------------------------------------------- 1. Y4M (host only)
def test_y4m_reader_takes_422_and_444_only_when_asked():
    for tag in (b"C422", b"C444", b"C422p10"):
        for md in (8, 16):
            with pytest.raises(video.Y4MError, match=tag.decode()[1:]):      # the default reader: another layout is never handed out silently
                video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W7 H5 F25:1 %s\n" % tag), max_depth=md)
    rng = np.random.default_rng(0)
    for tag, chroma, d, nbytes, siting in ((b"C422", "422", 8, 35 + 2 * 5 * 4, "mpeg2"), (b"C444", "444", 8, 105, "jpeg"),
                                           (b"C422p10", "422", 10, 150, "mpeg2")):
        payloads = list(_rand_payload(rng, 3, 5, 7, chroma, d))
        data = _stream(b"YUV4MPEG2 W7 H5 F25:1 Ip %s XCOLORRANGE=FULL\n" % tag, payloads)
        r = video.Y4MReader(io.BytesIO(data), max_depth=16, chroma=ALL3)
        assert (r.chroma, r.depth, r.frame_bytes, r.siting) == (chroma, d, nbytes, siting)
        assert r.frame_bytes == ops.yuv_frame_bytes(5, 7, chroma, d) and (r.width, r.height, r.colour_range) == (7, 5, "full")
        got = list(r.frames())
        assert len(got) == 3 and all(a.dtype == np.uint8 and np.array_equal(a, b) for a, b in zip(got, payloads))
    # 4:2:0 streams through such a reader are what they were
    r = video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W7 H5 C420mpeg2\n"), max_depth=16, chroma=ALL3)
    assert (r.chroma, r.depth, r.frame_bytes, r.siting) == ("420", 8, 59, "mpeg2")
    assert video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W7 H5 C420p10\n"), max_depth=16, chroma=ALL3).frame_bytes == 118
    assert video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W7 H5 C444\n"), chroma=("420", "444")).chroma == "444"
    with pytest.raises(video.Y4MError, match="422"):                        # asked for 4:4:4 only
        video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W7 H5 C422\n"), chroma=("420", "444"))
    with pytest.raises(video.Y4MError, match="C444p12"):
        video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W7 H5 C444p12\n"), max_depth=10, chroma=ALL3)
    with pytest.raises(video.Y4MError, match="C444p10"):                    # max_depth stays 8 unless raised
        video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W7 H5 C444p10\n"), chroma=ALL3)
    for tag in (b"Cmono", b"C444alpha", b"C411", b"Cmono16", b"C420paldv", b"C422p8", b"C444p17", b"C422p"):
        with pytest.raises(video.Y4MError, match=tag.decode()[1:]):
            video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H4 F25:1 %s\n" % tag), max_depth=16, chroma=ALL3)
    with pytest.raises(video.Y4MError, match="interlaced"):
        video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H4 F25:1 It C422\n"), max_depth=16, chroma=ALL3)
    with pytest.raises(ValueError):
        video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H4 C422\n"), chroma=("411",))
    assert ops.yuv_frame_bytes(5, 7) == ops.i420_frame_bytes(5, 7) == 59 and ops.yuv_frame_bytes(5, 7, "420", 10) == 118
    assert ops.yuv_frame_bytes(5, 7, "422") == 75 and ops.yuv_frame_bytes(5, 7, "444", 16) == 210
    with pytest.raises(ValueError, match="chroma"):
        ops.yuv_frame_bytes(4, 4, "411")
    with pytest.raises(ValueError, match="depth"):
        ops.yuv_frame_bytes(4, 4, "444", 17)


def test_y4m_writer_round_trips_422_and_444():
    rng = np.random.default_rng(1)
    for chroma, d, tag in (("422", 8, b" C422 "), ("444", 10, b" C444p10 ")):
        out = io.BytesIO()
        wr = video.Y4MWriter(out, 6, 5, "25:1", None, "p", full_range=False, depth=d, chroma=chroma)
        p = _rand_payload(rng, 3, 5, 6, chroma, d)
        for f in p:
            wr.write_frame(f)
        data = out.getvalue()
        assert data.startswith(b"YUV4MPEG2 W6 H5 F25:1 Ip" + tag + b"XCOLORRANGE=LIMITED\n")
        back = video.Y4MReader(io.BytesIO(data), max_depth=16, chroma=ALL3)
        assert (back.chroma, back.depth, back.colour_range, back.frame_bytes) == (chroma, d, "limited", p.shape[1])
        assert all(np.array_equal(a, b) for a, b in zip(back.frames(), p))
        with pytest.raises(video.Y4MError):
            wr.write_frame(p[0][:-2])
        with pytest.raises(video.Y4MError):
            wr.write_frame(np.zeros(ops.yuv_frame_bytes(5, 6, "420", d), np.uint8))     # the 4:2:0 size of the same frame
    with pytest.raises(ValueError):
        video.Y4MWriter(io.BytesIO(), 6, 4, chroma="411")
    out = io.BytesIO()
    video.Y4MWriter(out, 6, 4, chroma="420")                                # the default still writes C420jpeg
    assert b" C420jpeg " in out.getvalue()


def test_cli_size_rule_per_output_subsampling():
    f = video.video_out_size
    assert f(9, 14, "41x31", None, "444") == (31, 41) and f(9, 14, "40x31", None, "422") == (31, 40)
    assert f(9, 14, "40x30", None, "420") == (30, 40) and f(9, 14, None, None, "444") is None
    with pytest.raises(ValueError, match="odd width.*even"):
        f(9, 14, "41x30", None, "422")
    for size in ("41x30", "40x31"):
        with pytest.raises(ValueError, match="odd.*even"):
            f(9, 14, size, None, "420")
    for c in ALL3:                                                          # --scale rounds to even numbers as before
        assert f(9, 14, None, 1.5, c) == (14, 22)
    a = video.parser.parse_args(["--input", "-", "--output", "-", "--out_chroma", "444"])
    assert a.out_chroma == "444" and video.parser.parse_args(["--input", "-", "--output", "-"]).out_chroma is None
    with pytest.raises(SystemExit, match="odd width.*even"):                # before the stream is opened
        video.main(["--input", "/nonexistent.y4m", "--output", "/nonexistent/out.y4m", "--size", "641x360", "--out_chroma", "422"])


# ---------------------------------------------------------------------------------------------------- 2. decode
DEC_SHAPES = ((5, 7), (6, 9), (1, 3), (4, 4), (3, 1))


@pytest.mark.parametrize("d", [8, 10, 16])
def test_decode_matches_the_numpy_contract(dev, d):
    rng = np.random.default_rng(40 + d)
    worst = 0.0
    for h, w in DEC_SHAPES:
        for chroma, sitings in (("422", ("mpeg2", "jpeg")), ("444", ("jpeg",))):
            fr = _rand_payload(rng, 2, h, w, chroma, d)
            assert fr.shape[1] == ops.yuv_frame_bytes(h, w, chroma, d)
            x = torch.from_numpy(fr).to(dev)
            for siting in sitings:
                for matrix, full in COLOURS:
                    got = ops.yuv_to_image(x, h, w, chroma, siting, matrix, full, depth=d)
                    assert _kernel() == "yuv_to_image_kernel<%s,%s>" % ("u8" if d == 8 else "u16", chroma)
                    assert got.shape == (2, 3, h, w) and got.dtype == torch.float32
                    err = float(np.abs(got.cpu().double().numpy() - np_decode(from_payload(fr, d), h, w, chroma, siting, matrix, full, d)).max())
                    worst = max(worst, err)
                    assert err < 2e-6, (d, h, w, chroma, siting, matrix, full, err)
    print("decode, depth %d: max abs error %.3g" % (d, worst))


def test_decode_defaults_420_and_refusals(dev):
    rng = np.random.default_rng(41)
    h, w = 5, 7
    for d in (8, 10):
        fr = torch.from_numpy(to_payload(rng.integers(0, 2 ** d, size=(2, h * w + 2 * 3 * 4)), d)).to(dev)
        for siting in ("jpeg", "mpeg2"):                                    # "420" IS i420_to_image
            assert torch.equal(ops.yuv_to_image(fr, h, w, "420", siting, "bt709", True, depth=d),
                               ops.i420_to_image(fr, h, w, siting, "bt709", True, depth=d))
        assert torch.equal(ops.yuv_to_image(fr, h, w, depth=d), ops.i420_to_image(fr, h, w, depth=d))
    x2 = torch.from_numpy(_rand_payload(rng, 2, h, w, "422", 8)).to(dev)
    x4 = torch.from_numpy(_rand_payload(rng, 2, h, w, "444", 8)).to(dev)
    # siting=None: mpeg2 for 4:2:2; ignored for 4:4:4
    assert torch.equal(ops.yuv_to_image(x2, h, w, "422"), ops.yuv_to_image(x2, h, w, "422", "mpeg2"))
    assert not torch.equal(ops.yuv_to_image(x2, h, w, "422"), ops.yuv_to_image(x2, h, w, "422", "jpeg"))
    assert torch.equal(ops.yuv_to_image(x4, h, w, "444", "mpeg2"), ops.yuv_to_image(x4, h, w, "444"))
    with pytest.raises(ValueError):
        ops.yuv_to_image(x2, h, w, "444")                                   # the payload size of another format
    with pytest.raises(ValueError):
        ops.yuv_to_image(x4[:, :-1].contiguous(), h, w, "444")
    with pytest.raises(ValueError):
        ops.yuv_to_image(x4, h, w, "444", depth=10)
    for bad in (7, 17):
        with pytest.raises(ValueError, match="depth"):
            ops.yuv_to_image(x4, h, w, "444", depth=bad)
    with pytest.raises(ValueError, match="chroma"):
        ops.yuv_to_image(x4, h, w, "411")
    with pytest.raises(ValueError, match="siting"):
        ops.yuv_to_image(x2, h, w, "422", "dv")
    # the entry point itself: nothing is launched for a refused call
    img = torch.empty((2, h, w, 3), dtype=torch.float32, device=dev)
    lib = L.lib()
    for bad in (7, 17):
        assert lib.fsr_yuv_to_image(x4.data_ptr(), img.data_ptr(), 2, h, w, L.CHROMA_444, 0, 0, 0, bad, None) < 0
        assert b"depth" in lib.fsr_last_error()
    assert lib.fsr_yuv_to_image(x4.data_ptr(), img.data_ptr(), 2, h, w, 3, 0, 0, 0, 8, None) < 0
    assert b"chroma" in lib.fsr_last_error()
    assert lib.fsr_yuv_to_image(x2.data_ptr(), img.data_ptr(), 2, h, w, L.CHROMA_422, 2, 0, 0, 8, None) < 0
    assert b"siting" in lib.fsr_last_error()
    assert lib.fsr_yuv_to_image(x4.data_ptr() + 1, img.data_ptr(), 1, 2, 2, L.CHROMA_444, 0, 0, 0, 10, None) < 0
    assert b"aligned" in lib.fsr_last_error()
    assert lib.fsr_yuv_to_image(x4.data_ptr(), img.data_ptr(), 2, 65536, 32768, L.CHROMA_444, 0, 0, 0, 8, None) < 0
    assert b"2^31" in lib.fsr_last_error()


# ---------------------------------------------------------------------------------------------------- 3. encode, textbook codes
TEXTBOOK = [   # (depth, matrix, full, (R, G, B) signs, (Y, Cb, Cr)): BT.601 / BT.709 colour-bar codes
    (8, "bt601", False, (1, 1, 1), (235, 128, 128)), (8, "bt601", False, (-1, -1, -1), (16, 128, 128)),
    (8, "bt601", False, (1, -1, -1), (81, 90, 240)), (8, "bt709", False, (1, -1, -1), (63, 102, 240)),
    (8, "bt601", True, (1, 1, 1), (255, 128, 128)),
    (10, "bt601", False, (1, 1, 1), (940, 512, 512)), (10, "bt601", False, (-1, -1, -1), (64, 512, 512)),
    (10, "bt601", False, (1, -1, -1), (326, 361, 960)), (10, "bt709", False, (1, -1, -1), (250, 409, 960)),
    (10, "bt601", True, (1, 1, 1), (1023, 512, 512)), (10, "bt709", True, (-1, -1, 1), (74, 1023, 465)),
    (16, "bt601", False, (1, 1, 1), (60160, 32768, 32768)), (16, "bt601", False, (1, -1, -1), (20859, 23092, 61440)),
    (16, "bt709", True, (-1, -1, 1), (4732, 65535, 29763)),
]


@pytest.mark.parametrize("chroma", ["422", "444"])
def test_encode_textbook_codes(dev, chroma):
    n, h, w = 2, 6, 18
    plane, cplane = h * w, h * chroma_w(w, chroma)
    for d, matrix, full, signs, codes in TEXTBOOK:
        t = np.broadcast_to(np.array(signs, np.float32)[None, None, None, :], (n, h, w, 3)).copy()
        want = np.concatenate([np.full((n, plane), codes[0]), np.full((n, cplane), codes[1]), np.full((n, cplane), codes[2])], axis=1)
        for ft in (np.float32, np.float64):              # the contract itself gives the textbook numbers
            assert np.array_equal(np_encode(t.transpose(0, 3, 1, 2), chroma, matrix, full, d, ft), want), (d, matrix, full, signs, ft)
        out = ops.image_to_yuv(torch.from_numpy(t).to(dev), chroma, matrix, full, depth=d)
        assert out.dtype == torch.uint8 and out.shape == (n, ops.yuv_frame_bytes(h, w, chroma, d))
        assert _kernel() == "image_to_yuv_kernel<%s,%s>" % ("u8" if d == 8 else "u16", chroma)
        got = from_payload(out.cpu().numpy(), d)
        assert np.array_equal(got, want), (d, matrix, full, signs, np.unique(got[:, :plane]), np.unique(got[:, plane:]))


# ---------------------------------------------------------------------------------------------------- 4. encode, random
ENC_SHAPES = {"444": ((2, 16, 24), (1, 2, 6), (1, 5, 7), (1, 1, 1)), "422": ((2, 16, 24), (1, 2, 6), (1, 5, 10), (1, 1, 2))}


def _enc_input(shape):
    """t uniform in [-1.1, 1.1] (both clamps act), NHWC float32."""
    n, h, w = shape
    g = torch.Generator().manual_seed(100 * h + w)
    return (torch.rand(n, h, w, 3, generator=g) * 2.2 - 1.1).contiguous()


@pytest.mark.parametrize("chroma", ["422", "444"])
def test_float32_restatement_is_inside_a_third_of_the_caps(chroma):
    """The float32 restatement alone against float64, on the inputs of test_encode_random: at most a third of the cap at every depth."""
    for d in (8, 10, 12, 14, 16):
        differ = total = 0
        for shape in ENC_SHAPES[chroma]:
            t = _enc_input(shape).numpy().transpose(0, 3, 1, 2)
            for matrix, full in COLOURS:
                a, b = np_encode(t, chroma, matrix, full, d, np.float32), np_encode(t, chroma, matrix, full, d, np.float64)
                assert np.abs(a - b).max() <= 1
                differ, total = differ + int((a != b).sum()), total + a.size
        print("float32 restatement, 4:%s:%s, depth %d: %d of %d samples differ (%.4f %%)" % (chroma[1], chroma[2], d, differ, total,
                                                                                            100.0 * differ / total))
        assert total == (9792 if chroma == "444" else 6656)
        assert 3 * differ <= CAP[d] * total, (d, differ, total)


@pytest.mark.parametrize("d", [8, 10, 12, 14, 16])
@pytest.mark.parametrize("chroma", ["422", "444"])
def test_encode_random(dev, chroma, d):
    """Every code within 1 of the float64 contract; the share that differs at all, over the shapes and colour pairs of one depth (the
    9792 / 6656 samples the float32 test above counts -- the smallest shapes hold 3 and 4 samples, no share of them is below a cap),
    at most the cap."""
    got, want = [], []
    for shape in ENC_SHAPES[chroma]:
        n, h, w = shape
        t = _enc_input(shape)
        for matrix, full in COLOURS:
            out = ops.image_to_yuv(t.to(dev), chroma, matrix, full, depth=d)
            assert out.dtype == torch.uint8 and out.shape == (n, ops.yuv_frame_bytes(h, w, chroma, d))
            assert _kernel() == "image_to_yuv_kernel<%s,%s>" % ("u8" if d == 8 else "u16", chroma)
            got.append(from_payload(out.cpu().numpy(), d).reshape(-1))
            want.append(np_encode(t.numpy().transpose(0, 3, 1, 2), chroma, matrix, full, d).reshape(-1))
    assert_codes_close(np.concatenate(got), np.concatenate(want), CAP[d])


def test_encode_420_forwards_and_refusals(dev):
    t = _enc_input((2, 4, 6)).to(dev)
    for d in (8, 10):
        assert torch.equal(ops.image_to_yuv(t, "420", "bt709", True, depth=d), ops.image_to_i420(t, "bt709", True, depth=d))
    assert torch.equal(ops.image_to_yuv(t), ops.image_to_i420(t))
    for bad in (7, 17):
        with pytest.raises((ValueError, L.FsrError), match="depth"):
            ops.image_to_yuv(t, "444", depth=bad)
    with pytest.raises(ValueError, match="chroma"):
        ops.image_to_yuv(t, "411")
    with pytest.raises(ValueError, match="matrix"):
        ops.image_to_yuv(t, "444", "bt2020")
    with pytest.raises((ValueError, L.FsrError), match="even output width.*5"):
        ops.image_to_yuv(_enc_input((1, 4, 5)).to(dev), "422")
    assert ops.image_to_yuv(_enc_input((1, 3, 6)).to(dev), "422").shape == (1, 36)      # an odd height is legal
    lib = L.lib()
    out = torch.empty((2, 3 * 2 * 24), dtype=torch.uint8, device=dev)
    assert lib.fsr_image_to_yuv(t.data_ptr(), 2, 4, 6, 3, 0, 0, 8, out.data_ptr(), None) < 0
    assert b"chroma" in lib.fsr_last_error()
    assert lib.fsr_image_to_yuv(t.data_ptr(), 2, 4, 5, L.CHROMA_422, 0, 0, 8, out.data_ptr(), None) < 0
    assert b"even output width" in lib.fsr_last_error()
    for bad in (7, 17):
        assert lib.fsr_image_to_yuv(t.data_ptr(), 2, 4, 6, L.CHROMA_444, 0, 0, bad, out.data_ptr(), None) < 0
        assert b"depth" in lib.fsr_last_error()
    assert lib.fsr_image_to_yuv(t.data_ptr(), 2, 4, 6, L.CHROMA_444, 0, 0, 10, out.data_ptr() + 1, None) < 0
    assert b"misaligned" in lib.fsr_last_error()
    assert lib.fsr_image_to_yuv(t.data_ptr(), 2, 65536, 32768, L.CHROMA_444, 0, 0, 8, out.data_ptr(), None) < 0
    assert b"2^31" in lib.fsr_last_error()
    assert lib.fsr_image_to_yuv(t.data_ptr(), 2, 4, 6, L.CHROMA_444, 2, 0, 8, out.data_ptr(), None) < 0
    assert b"colour matrix" in lib.fsr_last_error()


# ---------------------------------------------------------------------------------------------------- 5. encode == resampler at identity taps
IDENTITY_SHAPES = [(c, s) for c in ("422", "444") for s in ENC_SHAPES[c] + ((1, 6, 70), (1, 34, 132))] + [("444", (1, 7, 67))]


@pytest.mark.parametrize("chroma, shape", IDENTITY_SHAPES, ids=lambda v: v if isinstance(v, str) else "%dx%dx%d" % v)
def test_encode_is_the_resamplers_planar_stage_at_the_native_size(dev, chroma, shape):
    """Same helpers, same order, identity taps: byte-identical, across the 64-column tile border too (the 4:2:2 left neighbour)."""
    n, h, w = shape
    t = _enc_input(shape).to(dev)
    for d in (8, 10, 16):
        for matrix, full in (("bt601", False), ("bt709", True)):
            a = ops.image_to_yuv(t, chroma, matrix, full, depth=d)
            assert _kernel() == "image_to_yuv_kernel<%s,%s>" % ("u8" if d == 8 else "u16", chroma)
            b = ops.resample_image(t, h, w, "i420", matrix, full, depth=d, chroma=chroma)
            assert _kernel() == "resample_kernel<yuv%s,5,%s>" % (chroma, "u8" if d == 8 else "u16")
            assert a.shape == b.shape and torch.equal(a, b), (d, matrix, full)


# ---------------------------------------------------------------------------------------------------- 6. resize
def _np_resize(t_nchw, oh, ow):
    """float64 tap composition of the antialiased bicubic on c = (t + 1) / 2, clamped, back as a tanh-range tensor."""
    c = (np.asarray(t_nchw).astype(np.float64) + 1.0) / 2.0
    v = np.einsum("oy,ncyx,px->ncop", _aa_matrix(c.shape[2], oh), c, _aa_matrix(c.shape[3], ow))
    return 2.0 * np.clip(v, 0.0, 1.0) - 1.0


@pytest.mark.parametrize("chroma, src, dst", [("422", (9, 14), (20, 26)), ("422", (6, 40), (9, 134)), ("444", (9, 14), (21, 27)),
                                              ("444", (6, 40), (9, 131))], ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_resize_against_the_tap_composition(dev, chroma, src, dst):
    (h, w), (oh, ow) = src, dst
    t = torch.rand(2, h, w, 3, generator=torch.Generator().manual_seed(9)) * 2.2 - 1.1
    v = _np_resize(t.numpy().transpose(0, 3, 1, 2), oh, ow)
    for d in (8, 10):
        for matrix, full in COLOURS:
            got = ops.resample_image(t.to(dev), oh, ow, "i420", matrix, full, depth=d, chroma=chroma)
            assert _kernel() == "resample_kernel<yuv%s,5,%s>" % (chroma, "u8" if d == 8 else "u16")
            assert got.dtype == torch.uint8 and got.shape == (2, ops.yuv_frame_bytes(oh, ow, chroma, d))
            assert_codes_close(from_payload(got.cpu().numpy(), d), np_encode(v, chroma, matrix, full, d), CAP[d])


def test_resize_refusals_and_tap_forms(dev):
    t = _enc_input((1, 8, 12)).to(dev)
    with pytest.raises((ValueError, L.FsrError), match="even output width.*27"):
        ops.resample_image(t, 20, 27, "i420", chroma="422")
    with pytest.raises(ValueError, match="chroma"):
        ops.resample_image(t, 20, 26, "i420", chroma="411")
    with pytest.raises(ValueError, match="i420"):
        ops.resample_image(t, 20, 26, "u8", chroma="444")
    with pytest.raises((ValueError, L.FsrError), match="depth"):
        ops.resample_image(t, 20, 26, "i420", depth=17, chroma="444")
    # chroma "420" is the call without the keyword
    assert torch.equal(ops.resample_image(t, 20, 26, "i420", "bt709", True, 10, "420"), ops.resample_image(t, 20, 26, "i420", "bt709", True, 10))
    # the entry point: odd 4:2:2 width, unknown chroma, misaligned 16-bit payload -- nothing launched
    wy, ymin, ysize, ky = ops.aa_taps(8, 8, dev)
    wx, xmin, xsize, kx = ops.aa_taps(12, 13, dev)
    out = torch.empty((1, 4 * 8 * 14), dtype=torch.uint8, device=dev)
    lib = L.lib()

    def call(ow, chroma, depth, o):
        return lib.fsr_resample_image_yuv(t.data_ptr(), 1, 8, 12, 8, ow, wy.data_ptr(), ymin.data_ptr(), ysize.data_ptr(), ky, wx.data_ptr(),
                                          xmin.data_ptr(), xsize.data_ptr(), kx, chroma, 0, 0, depth, o, None)
    assert call(13, L.CHROMA_422, 8, out.data_ptr()) < 0 and b"even output width (13)" in lib.fsr_last_error()
    assert call(13, 3, 8, out.data_ptr()) < 0 and b"chroma" in lib.fsr_last_error()
    assert call(13, L.CHROMA_444, 10, out.data_ptr() + 1) < 0 and b"aligned" in lib.fsr_last_error()
    assert call(13, L.CHROMA_444, 7, out.data_ptr()) < 0 and b"depth" in lib.fsr_last_error()
    # down-scales: the 9-tap and the any-tap forms of the horizontal pass, against the composition
    big = torch.rand(1, 12, 150, 3, generator=torch.Generator().manual_seed(10)) * 2.2 - 1.1
    for chroma, (oh, ow), form in (("422", (7, 90), 9), ("444", (7, 91), 9), ("422", (5, 40), 0), ("444", (5, 41), 0)):
        got = ops.resample_image(big.to(dev), oh, ow, "i420", depth=10, chroma=chroma)
        assert _kernel() == "resample_kernel<yuv%s,%d,u16>" % (chroma, form)
        want = np_encode(_np_resize(big.numpy().transpose(0, 3, 1, 2), oh, ow), chroma, d=10)
        assert_codes_close(from_payload(got.cpu().numpy(), 10), want, CAP[10])


# ---------------------------------------------------------------------------------------------------- 7. the whole generator
def _rand_420(rng, n, h, w, d):
    return to_payload(rng.integers(0, 2 ** d, size=(n, samples_of(h, w, "420"))), d)


def _check_forward(G, fr, h, w, c, oc, d, od, dev, out_size=None, colour=("bt601", False), out_colour=("bt709", True), cap=1e-3):
    """forward_yuv against the numpy encode of the same model's float forward() on the device-decoded frames (resized in float64 for
    an out_size)."""
    x = torch.from_numpy(fr).to(dev)
    got = G.forward_yuv(x, h, w, chroma=c, out_chroma=oc, matrix=colour[0], full_range=colour[1], out_matrix=out_colour[0],
                        out_full_range=out_colour[1], out_size=out_size, depth=d, out_depth=od)
    kernel = _kernel()
    oh, ow = out_size or (4 * h, 4 * w)
    assert got.dtype == torch.uint8 and got.shape == (fr.shape[0], ops.yuv_frame_bytes(oh, ow, oc, od))
    with torch.no_grad():
        t = G(ops.yuv_to_image(x, h, w, c, None, colour[0], colour[1], depth=d)).cpu().numpy()
    if out_size is not None:
        t = _np_resize(t, oh, ow)
    assert_codes_close(from_payload(got.cpu().numpy(), od), np_encode(t, oc, out_colour[0], out_colour[1], od), cap)
    return kernel


def test_forward_yuv_tiny_generator(dev, pkg):
    G = _tiny(pkg, dev)
    rng = np.random.default_rng(5)
    h, w = 3, 5
    fr = {(c, d): (_rand_420(rng, 2, h, w, d) if c == "420" else _rand_payload(rng, 2, h, w, c, d)) for c in ALL3 for d in (8, 10)}
    for c in ALL3:
        for oc in ALL3:
            k = _check_forward(G, fr[c, 8], h, w, c, oc, 8, 8, dev)
            assert k.startswith("conv_igemm_kernel<f32") if oc == "420" else k == "image_to_yuv_kernel<u8,%s>" % oc, k    # (the head's own epilogue)
    for c, oc in (("422", "422"), ("420", "444")):
        assert _check_forward(G, fr[c, 10], h, w, c, oc, 10, 10, dev) == "image_to_yuv_kernel<u16,%s>" % oc
        assert _check_forward(G, fr[c, 8], h, w, c, oc, 8, 10, dev) == "image_to_yuv_kernel<u16,%s>" % oc
        assert _check_forward(G, fr[c, 8], h, w, c, oc, 8, 8, dev, out_size=(10, 18)).startswith("resample_kernel<yuv%s," % oc)
    assert _check_forward(G, fr["444", 8], h, w, "444", "420", 8, 10, dev) == "image_to_i420_kernel<u16>"
    assert _check_forward(G, fr["422", 8], h, w, "422", "420", 8, 8, dev, out_size=(10, 18)).startswith("resample_kernel<i420,")
    assert _check_forward(G, fr["420", 8], h, w, "420", "444", 8, 8, dev, out_size=(11, 17)).startswith("resample_kernel<yuv444,")
    # chroma "420" in and out IS forward_yuv420
    x8, x10 = torch.from_numpy(fr["420", 8]).to(dev), torch.from_numpy(fr["420", 10]).to(dev)
    assert torch.equal(G.forward_yuv(x8, h, w), G.forward_yuv420(x8, h, w))
    assert torch.equal(G.forward_yuv(x8, h, w, chroma="420", siting="mpeg2", matrix="bt709", out_full_range=True, out_size=(14, 30)),
                       G.forward_yuv420(x8, h, w, siting="mpeg2", matrix="bt709", out_full_range=True, out_size=(14, 30)))
    assert torch.equal(G.forward_yuv(x10, h, w, depth=10, out_depth=12), G.forward_yuv420(x10, h, w, depth=10, out_depth=12))
    # out_chroma defaults to chroma
    x2 = torch.from_numpy(fr["422", 8]).to(dev)
    assert torch.equal(G.forward_yuv(x2, h, w, chroma="422"), G.forward_yuv(x2, h, w, chroma="422", out_chroma="422", siting="mpeg2"))
    for bad in (dict(chroma="411"), dict(out_chroma="440"), dict(chroma="422", depth=7), dict(chroma="422", out_depth=17)):
        with pytest.raises(ValueError, match="chroma|depth"):
            G.forward_yuv(x2, h, w, **bad)
    with pytest.raises((ValueError, L.FsrError), match="even output width"):
        G.forward_yuv(x2, h, w, chroma="422", out_size=(10, 17))


def test_pipeline_run_yuv_keys_and_frame_sizes(pkg):
    """No device: the plan key and the staging size of run_yuv (the pipeline refuses a frame the kernels cannot index before it
    allocates, which shows both)."""
    G = pkg.Generator(ns(n_filters=64, n_layers=8), compute_dtype="f32")
    pipe = pkg.InferencePipeline(G, "cpu", batch=8)
    with pytest.raises(ValueError, match="2560x1440"):
        pipe.run_yuv([], 1440, 2560, chroma="422", out_chroma="444")
    assert not pipe._plans


# ---------------------------------------------------------------------------------------------------- 8. GPU only
@pytest.mark.gpu
@pytest.mark.parametrize("cdn", ["f16", "x3"])
def test_forward_yuv_shipped_weights_gpu(pkg, cdn, monkeypatch):
    dev = select("hip")
    monkeypatch.setenv("FSR_PERSIST_CUS", "5")
    G = _shipped(pkg, dev, cdn)
    rng = np.random.default_rng(6)
    h, w = 23, 37
    for c, oc, d in (("420", "444", 8), ("422", "422", 10), ("444", "444", 8)):
        fr = _rand_420(rng, 2, h, w, d) if c == "420" else _rand_payload(rng, 2, h, w, c, d)
        assert _check_forward(G, fr, h, w, c, oc, d, d, dev) == "image_to_yuv_kernel<%s,%s>" % ("u8" if d == 8 else "u16", oc)


@pytest.mark.gpu
def test_pipeline_run_yuv_graph_equals_eager_gpu(pkg):
    dev = select("hip")
    G = _shipped(pkg, dev, "f16")
    rng = np.random.default_rng(7)
    h, w, d = 17, 29, 10
    frames = list(_rand_payload(rng, 5, h, w, "422", d))
    colour = dict(matrix="bt709", full_range=True, out_matrix="bt601", out_full_range=False)
    pipe = pkg.InferencePipeline(G, dev, batch=2, depth=2, copy=False)
    outs = []
    for y in pipe.run_yuv(frames, h, w, chroma="422", out_chroma="444", depth=d, **colour):
        assert y.shape == (ops.yuv_frame_bytes(4 * h, 4 * w, "444", d),) and y.dtype == np.uint8
        outs.append(y.copy())
    assert len(outs) == 5                                                   # two full batches through the graphs, a ragged tail of one
    key = ("i420", h, w, "mpeg2", "bt709", True, "bt601", False, "depth", 10, 10, "chroma", "422", "444")
    assert list(pipe._plans) == [key] and all(sl is not None and sl.graph is not None for sl in pipe._plans[key])
    eager = pkg.InferencePipeline(G, dev, batch=2, depth=2, use_graph=False)
    outs_eager = list(eager.run_yuv((bytes(f) for f in frames), h, w, chroma="422", out_chroma="444", depth=d, **colour))
    assert len(outs_eager) == 5 and all(np.array_equal(a, b) for a, b in zip(outs, outs_eager))
    one = G.forward_yuv(torch.from_numpy(frames[4]).unsqueeze(0).to(dev), h, w, chroma="422", out_chroma="444", depth=d, **colour)[0]
    assert np.array_equal(outs[4], one.cpu().numpy())
    # ("420", "420") through run_yuv is run_yuv420's plan
    frames8 = list(_rand_420(rng, 2, h, w, 8))
    a = list(pipe.run_yuv(frames8, h, w, **colour))
    assert list(pipe._plans)[-1] == ("i420", h, w, "jpeg", "bt709", True, "bt601", False)
    assert all(np.array_equal(x, y) for x, y in zip(a, eager.run_yuv420(frames8, h, w, **colour)))


@pytest.fixture(scope="module")
def cli_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("chroma_cli")
    sd = sd_from(load_npz("g_model_pt.npz"), "sd.")
    (d / "models").mkdir()
    (d / "configs").mkdir()
    torch.save({"_orig_mod." + k: v for k, v in sd.items()}, d / "models" / "model.pt")
    (d / "configs" / "config.yaml").write_text("generator:\n  n_filters: 64\n  n_layers: 8\ntraining:\n  compute_dtype: f16\n")
    return d


def _cli_model(cli_dir, dev):
    return inference.load_generator(importlib.import_module("fast-srgan_amd.config").load_config(str(cli_dir / "configs" / "config.yaml")),
                                    str(cli_dir / "models" / "model.pt"), dev)


@pytest.mark.gpu
def test_video_cli_422_deep_stream_gpu(cli_dir):
    dev = select("hip")
    rng = np.random.default_rng(8)
    h, w, nf = 9, 14, 3
    frames = _rand_payload(rng, nf, h, w, "422", 10)
    r = _cli(cli_dir, _stream(b"YUV4MPEG2 W14 H9 F30000:1001 Ip A1:1 C422p10 XCOLORRANGE=LIMITED\n", frames))
    head = r.stdout.split(b"\n", 1)[0]
    assert head.startswith(b"YUV4MPEG2 W56 H36 ") and b" C422p10 " in head
    assert b"4:2:2 -> 4:2:2" in r.stderr and b"chroma siting mpeg2" in r.stderr
    out = video.Y4MReader(io.BytesIO(r.stdout), max_depth=16, chroma=ALL3)
    assert (out.width, out.height, out.depth, out.chroma, out.frame_rate) == (56, 36, 10, "422", "30000:1001")
    got = list(out.frames())
    assert len(got) == nf
    want = _cli_model(cli_dir, dev).forward_yuv(torch.from_numpy(frames).to(dev), h, w, chroma="422", depth=10).cpu().numpy()
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
def test_video_cli_420_to_444_resized_gpu(cli_dir):
    dev = select("hip")
    rng = np.random.default_rng(8)
    h, w, nf = 9, 14, 3
    frames = _rand_420(rng, nf, h, w, 8)
    r = _cli(cli_dir, _stream(b"YUV4MPEG2 W14 H9 F25:1 C420jpeg\n", frames), "--out_chroma", "444", "--size", "50x30")
    head = r.stdout.split(b"\n", 1)[0]
    assert head.startswith(b"YUV4MPEG2 W50 H30 ") and b" C444 " in head and b"4:2:0 -> 4:4:4" in r.stderr
    out = video.Y4MReader(io.BytesIO(r.stdout), chroma=ALL3)
    assert (out.width, out.height, out.depth, out.chroma, out.frame_bytes) == (50, 30, 8, "444", 4500)
    got = list(out.frames())
    assert len(got) == nf
    want = _cli_model(cli_dir, dev).forward_yuv(torch.from_numpy(frames).to(dev), h, w, out_chroma="444", out_size=(30, 50)).cpu().numpy()
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
