"""Row bands of the generator's tail: the band geometry, the strided row-block copy (fsr_copy_rows), banded
forwards against whole-frame forwards bit for bit on every route, the batch limits, the pipeline and the CLI."""
import importlib
import io

import numpy as np
import pytest
import torch

from backend import BACKENDS, L, ops, select
from conftest import load_npz, sd_from
from yuv_contract import _cli, _shipped, _stream, _tiny, ns

inference = importlib.import_module("fast-srgan_amd.inference")
video = importlib.import_module("fast-srgan_amd.video")


# ---------------------------------------------------------------------------------------------------- 1. geometry (host)
def test_tail_windows_geometry():
    for H2 in range(1, 65):
        for R in range(1, 17):
            wins = ops.tail_windows(H2, R)
            Hw = R + 4
            if H2 <= Hw:
                assert wins == [(0, 0, H2)], (H2, R)
                continue
            assert len(wins) == (H2 + R - 1) // R
            covered = []
            for k, (s, lo, hi) in enumerate(wins):
                assert (lo, hi) == (k * R, min((k + 1) * R, H2)) and lo < hi
                assert 0 <= s and s + Hw <= H2, (H2, R, k)                 # the window lies inside the frame
                assert s == max(0, min(k * R - 2, H2 - Hw))
                # every core row is 2 rows or more from a window edge that is not the frame's edge
                assert s == 0 or lo - s >= 2, (H2, R, k)
                assert s + Hw == H2 or (s + Hw) - hi >= 2, (H2, R, k)
                covered += list(range(lo, hi))
            assert covered == list(range(H2)), (H2, R)                      # the cores tile [0, H2) exactly once
    with pytest.raises(ValueError):
        ops.tail_windows(8, 0)


# ---------------------------------------------------------------------------------------------------- 2. the row-copy kernel
def _bytes(dev, n, rng=None, fill=None):
    """A 128-byte aligned uint8 tensor of n bytes on `dev`: random, or filled with `fill`."""
    t = ops._empty((n,), torch.uint8, dev)
    if rng is not None:
        t.copy_(torch.from_numpy(rng.integers(0, 256, size=n, dtype=np.uint8)))
    else:
        t.fill_(fill)
    return t


def _width_rule(*values):
    a = 0
    for v in values:
        a |= v
    return 16 if a % 16 == 0 else (4 if a % 4 == 0 else 1)


@pytest.mark.parametrize("backend", BACKENDS)
def test_copy_rows_against_numpy_slicing(backend):
    dev = select(backend)
    rng = np.random.default_rng(15)
    n, H2, R = 2, 11, 3
    Hw, wins = R + 4, ops.tail_windows(H2, R)
    assert wins == [(0, 0, 3), (1, 3, 6), (4, 6, 9), (4, 9, 11)]           # four windows, the last one clamped
    nwin, seen = len(wins), set()
    for rb in (14, 20, 48, 80):
        for off in (0, 4, 7):
            for mul in (1, 2):
                first, count = (1, 6) if mul == 1 else (0, n * nwin)
                pad = 32                                                    # bytes between images that no copy may touch
                # gather: frames of H2 rows -> windows of Hw rows
                fp, gp = H2 * rb + pad, Hw * rb
                src = _bytes(dev, off + n * fp, rng)
                dst = _bytes(dev, off + count * gp + pad, fill=0xA5)
                ops.copy_rows(src, dst, fp, gp, rb, first, count, H2, R, src_offset=off, dst_offset=off)
                kern = ops._last_kernel()
                assert kern == "copy_rows_kernel<%d>" % _width_rule(off, fp, gp, rb), (rb, off, kern)
                seen.add(kern)
                s_np, want = src.cpu().numpy(), np.full(dst.numel(), 0xA5, np.uint8)
                for j in range(count):
                    img, k = divmod(first + j, nwin)
                    a = off + img * fp + wins[k][0] * rb
                    want[off + j * gp: off + (j + 1) * gp] = s_np[a: a + Hw * rb]
                assert np.array_equal(dst.cpu().numpy(), want), ("gather", rb, off, mul)
                # scatter: `mul` rows per core row of every window -> their place in the frames
                wp, fp = Hw * mul * rb, H2 * mul * rb + pad
                src = _bytes(dev, off + count * wp, rng)
                dst = _bytes(dev, off + n * fp, fill=0xA5)
                ops.copy_rows(src, dst, wp, fp, rb, first, count, H2, R, mul, True, off, off)
                assert ops._last_kernel() == "copy_rows_kernel<%d>" % _width_rule(off, wp, fp, rb)
                s_np, want = src.cpu().numpy(), np.full(dst.numel(), 0xA5, np.uint8)
                for j in range(count):
                    img, k = divmod(first + j, nwin)
                    s, lo, hi = wins[k]
                    a = off + j * wp + (lo - s) * mul * rb
                    b = off + img * fp + lo * mul * rb
                    want[b: b + (hi - lo) * mul * rb] = s_np[a: a + (hi - lo) * mul * rb]
                assert np.array_equal(dst.cpu().numpy(), want), ("scatter", rb, off, mul)     # the cores, and nothing else
    assert seen == {"copy_rows_kernel<16>", "copy_rows_kernel<4>", "copy_rows_kernel<1>"}


@pytest.mark.parametrize("backend", BACKENDS)
def test_copy_rows_refuses_bad_arguments(backend):
    dev = select(backend)
    lib = L.lib()
    src, dst = _bytes(dev, 4096, fill=1), _bytes(dev, 4096, fill=0xA5)
    s, d = src.data_ptr(), dst.data_ptr()
    st = ops._stream()
    good = (s, 11 * 16, d, 7 * 16, 16, 0, 2, 11, 7, 3, 1, 0, st)

    def call(**kw):
        names = ("src", "src_pitch", "dst", "dst_pitch", "row_bytes", "first", "count", "H2", "Hw", "R", "mul", "scatter", "stream")
        a = dict(zip(names, good))
        a.update(kw)
        return lib.fsr_copy_rows(*[a[k] for k in names])

    for bad in (dict(src=None), dict(dst=None), dict(src_pitch=0), dict(dst_pitch=-16), dict(row_bytes=0), dict(count=0), dict(H2=0),
                dict(mul=0), dict(first=-1), dict(R=0, Hw=4), dict(H2=6), dict(Hw=6), dict(count=65536)):
        assert call(**bad) < 0, bad
        assert lib.fsr_last_error()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert bool((dst == 0xA5).all())                                        # nothing was launched
    # the wrapper: windows beyond the tensors are refused on the host, a frame smaller than a window by the library
    with pytest.raises(ValueError, match="beyond"):
        ops.copy_rows(src, dst, 11 * 16, 7 * 16, 16, 0, 40, 11, 3)
    with pytest.raises(L.FsrError, match="does not fit"):
        ops.copy_rows(src, dst, 5 * 16, 7 * 16, 16, 0, 1, 5, 3)
    assert call() == 0


# ---------------------------------------------------------------------------------------------------- 3. offsets past 2^32 bytes
@pytest.mark.gpu
def test_copy_rows_past_4_gib_gpu():
    """A buffer of 2^32 + 2^20 bytes taken as one frame of 64 KiB rows: the last 16 rows lie past 2^32, where a 32-bit byte offset
    wraps to the front of the buffer.  Only the windows of the last 64 rows move: a few MB."""
    dev = select("hip")
    rng = np.random.default_rng(16)
    rb, R = 1 << 16, 12
    total = (1 << 32) + (1 << 20)
    H2, Hw = total // rb, R + 4
    nwin = (H2 + R - 1) // R
    first = next(k for k in range(nwin) if max(0, min(k * R - 2, H2 - Hw)) >= H2 - 64)
    count = nwin - first
    assert count >= 4 and (first * R + R) * rb < (1 << 32) < (nwin - 1) * R * rb
    starts = [max(0, min(k * R - 2, H2 - Hw)) for k in range(first, nwin)]
    # gather out of the far end
    big = torch.empty(total, dtype=torch.uint8, device=dev)
    tail = torch.from_numpy(rng.integers(0, 256, size=(64, rb), dtype=np.uint8))
    big[:16 * rb].zero_()
    big[total - 64 * rb:].copy_(tail.reshape(-1))
    out = torch.empty((count, Hw * rb), dtype=torch.uint8, device=dev)
    ops.copy_rows(big, out, total, Hw * rb, rb, first, count, H2, R)
    got = out.cpu().numpy().reshape(count, Hw, rb)
    for j, s in enumerate(starts):
        assert np.array_equal(got[j], tail.numpy()[s - (H2 - 64): s - (H2 - 64) + Hw]), j
    # scatter into the far end
    big[total - 64 * rb:].fill_(0xA5)
    src = torch.from_numpy(rng.integers(0, 256, size=(count, Hw, rb), dtype=np.uint8)).to(dev)
    ops.copy_rows(src, big, Hw * rb, total, rb, first, count, H2, R, 1, True)
    got = big[total - 64 * rb:].cpu().numpy().reshape(64, rb)
    want = np.full((64, rb), 0xA5, np.uint8)
    for j, s in enumerate(starts):
        lo, hi = (first + j) * R, min((first + j + 1) * R, H2)
        want[lo - (H2 - 64): hi - (H2 - 64)] = src[j, lo - s: hi - s].cpu().numpy()
    assert np.array_equal(got, want)
    assert bool((big[:16 * rb] == 0).all())                                 # where a wrapped offset would have landed
    del big, src, out


# ---------------------------------------------------------------------------------------------------- 4. banded = whole frame
# (n, h, w, R): several windows with a clamped last one, odd extents and partial head tiles; a wide frame; R >= H2: one window
SHAPES = [(2, 9, 7, 4), (1, 5, 20, 3), (1, 5, 20, 64)]


def _random_generator(pkg, dev, cdn):
    torch.manual_seed(11)
    return pkg.Generator(ns(n_filters=64, n_layers=1), compute_dtype=cdn).to(dev).eval()


def _routes(G, u8, yuv, h, w):
    """name -> function of `bands` for every route of the public surface, on the same inputs."""
    x = ops.u8_to_image(u8)
    return {
        "forward": lambda b: G.forward(x, bands=b),
        "forward_u8": lambda b: G.forward_u8(u8, bands=b),
        "yuv420_8": lambda b: G.forward_yuv(yuv, h, w, bands=b),                                        # the head's I420 epilogue
        "yuv444_10": lambda b: G.forward_yuv(yuv, h, w, out_chroma="444", out_depth=10, bands=b),       # float head + encode
        "resized": lambda b: G.forward_u8(u8, out_size=(3 * h + 1, 3 * w - 2), bands=b),                # float head + resampler
    }


def _assert_banded_equals_whole(G, dev, shapes, routes=None):
    rng = np.random.default_rng(17)
    for n, h, w, R in shapes:
        u8 = torch.from_numpy(rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)).to(dev)
        yuv = torch.from_numpy(rng.integers(0, 256, size=(n, ops.yuv_frame_bytes(h, w)), dtype=np.uint8)).to(dev)
        with torch.no_grad():
            for name, f in _routes(G, u8, yuv, h, w).items():
                if routes is not None and name not in routes:
                    continue
                whole, banded = f(None), f(R)
                assert whole.shape == banded.shape and whole.dtype == banded.dtype, (name, n, h, w, R)
                assert torch.equal(whole, banded), (name, n, h, w, R)


@pytest.mark.parametrize("backend", BACKENDS)
def test_banded_equals_whole_tiny_f32(pkg, backend):
    dev = select(backend)
    G = _tiny(pkg, dev)
    _assert_banded_equals_whole(G, dev, SHAPES)
    x = torch.zeros((1, 3, 9, 7), device=dev)
    with torch.enable_grad(), pytest.raises(L.FsrError, match="inference-only"):
        G.forward(x, bands=4)
    with torch.no_grad(), pytest.raises(ValueError, match="bands"):
        G.forward(x, bands=0)


@pytest.mark.parametrize("cdn", ["f16", "x3"])
def test_banded_equals_whole_64_filters_emu(pkg, cdn):
    """The 64-channel kernels (the ones the shipped model runs) on the emulator: one 16-bit mode and x3."""
    dev = select("emu")
    _assert_banded_equals_whole(_random_generator(pkg, dev, cdn), dev, SHAPES[:1], routes=("forward", "yuv420_8"))


@pytest.mark.gpu
@pytest.mark.parametrize("cdn", ["f16", "bf16", "x3", "f32"])
def test_banded_equals_whole_shipped_gpu(pkg, cdn):
    dev = select("hip")
    _assert_banded_equals_whole(_shipped(pkg, dev, cdn), dev, SHAPES)


def test_no_upsampling_block_ignores_bands(pkg):
    dev = select("emu")
    torch.manual_seed(12)
    G = pkg.Generator(ns(n_filters=16, n_layers=1, n_upsample=0), compute_dtype="f32").to(dev).eval()
    x = torch.rand((1, 3, 9, 7), device=dev) * 2 - 1
    with torch.no_grad():
        assert torch.equal(G.forward(x), G.forward(x, bands=2))
    assert G.max_batch(1024, 1024, bands=True) == G.max_batch(1024, 1024) == 127


# ---------------------------------------------------------------------------------------------------- 5. limits (host)
def test_max_batch_banded_and_the_pipelines_modes(pkg, capfd):
    G = pkg.Generator(ns(n_filters=64, n_layers=8), compute_dtype="f32")
    sizes = ((360, 640), (720, 1280), (1080, 1920), (1440, 2560), (2160, 3840), (2160, 4096))
    assert [G.max_batch(h, w, bands=True) for h, w in sizes] == [36, 9, 4, 2, 1, 0]
    assert [G.max_batch(h, w) for h, w in sizes] == [9, 2, 1, 0, 0, 0]
    assert [G.max_batch(h, w, bands=False) for h, w in sizes] == [9, 2, 1, 0, 0, 0]
    auto = pkg.InferencePipeline(G, "cpu", batch=8, bands="auto")
    assert auto._batch_for(1440, 2560) == 2 and auto._batch_for(720, 1280) == 2
    assert auto._bands_for(1440, 2560) == 128 and auto._bands_for(720, 1280) is None
    assert auto._batch_for(1440, 2560) == 2
    err = capfd.readouterr().err
    assert err.count("2560x1440 frames run banded") == 1 and "in batches of 2" in err       # said once
    on = pkg.InferencePipeline(G, "cpu", batch=8, bands="on", band_rows=32)
    assert on._batch_for(720, 1280) == 8 and on._bands_for(720, 1280) == 32
    assert on._batch_for(180, 320) == 8 and on._bands_for(180, 320) is None                 # already a full batch whole
    off = pkg.InferencePipeline(G, "cpu", batch=8, bands="off")
    with pytest.raises(ValueError, match="2560x1440"):
        off._batch_for(1440, 2560)
    assert pkg.InferencePipeline(G, "cpu", batch=8).bands == "off"                          # the library default
    for pipe in (auto, on, off):
        with pytest.raises(ValueError, match="4096x2160") as e:
            pipe.run_yuv420([], 2160, 4096)
        assert "2^31" in str(e.value)
        with pytest.raises(ValueError, match="4096x2160"):
            list(pipe.run([np.zeros((2160, 4096, 3), np.uint8)]))
        assert not pipe._plans
    with pytest.raises(ValueError, match="4096x2160") as e:
        auto._batch_for(2160, 4096)
    assert "8388607 input pixels" in str(e.value)                                           # the new limit, about 8.4 M
    with pytest.raises(ValueError):
        pkg.InferencePipeline(G, "cpu", bands="maybe")
    with pytest.raises(ValueError):
        pkg.InferencePipeline(G, "cpu", bands="on", band_rows=0)


def test_cli_flags_are_declared():
    for p in (video.parser, inference.parser):
        opts = {a.dest: a for a in p._actions}
        assert opts["bands"].default == "auto" and sorted(opts["bands"].choices) == ["auto", "off", "on"]
        assert opts["band_rows"].default == 128 and opts["band_rows"].type is int


# ---------------------------------------------------------------------------------------------------- 6. pipeline under hipGraph
@pytest.mark.gpu
def test_pipeline_banded_under_graph_gpu(pkg, monkeypatch, capfd):
    dev = select("hip")
    G = _shipped(pkg, dev, "f16")
    monkeypatch.setattr(G, "max_batch", lambda h, w, bands=False: 2 if bands else 0)        # 8 x 12 is "too large" whole
    rng = np.random.default_rng(18)
    h, w = 8, 12
    frames = [rng.integers(0, 256, size=ops.yuv_frame_bytes(h, w), dtype=np.uint8) for _ in range(5)]
    pipe = pkg.InferencePipeline(G, dev, batch=4, depth=2, bands="on", band_rows=4)
    outs = list(pipe.run_yuv420(frames, h, w))                                              # two graph batches and an eager tail
    assert len(outs) == 5
    (key, plan), = pipe._plans.items()
    assert key[-2:] == ("bands", 4)
    assert all(sl is not None and sl.graph is not None and sl.x.shape[0] == 2 for sl in plan)
    for f, y in zip(frames, outs):
        assert np.array_equal(y, G.forward_yuv420(torch.from_numpy(f).unsqueeze(0).to(dev), h, w)[0].cpu().numpy())
    rgb = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(5)]
    got = list(pipe.run(rgb))
    assert (h, w, "bands", 4) in pipe._plans
    for f, y in zip(rgb, got):
        assert np.array_equal(y, G.forward_u8(torch.from_numpy(f).unsqueeze(0).to(dev))[0].cpu().numpy())
    assert capfd.readouterr().err.count("run banded") == 1                                  # said once for the shape


# ---------------------------------------------------------------------------------------------------- 7. the CLI
@pytest.fixture(scope="module")
def cli_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("bands_cli")
    sd = sd_from(load_npz("g_model_pt.npz"), "sd.")
    (d / "models").mkdir()
    (d / "configs").mkdir()
    torch.save({"_orig_mod." + k: v for k, v in sd.items()}, d / "models" / "model.pt")
    (d / "configs" / "config.yaml").write_text("generator:\n  n_filters: 64\n  n_layers: 8\ntraining:\n  compute_dtype: f16\n")
    return d


@pytest.mark.gpu
def test_video_cli_bands_flags_gpu(cli_dir):
    """`--bands on --band_rows 4` writes the bytes of the default run.  (A frame this small fills its batch whole, so "on" has nothing
    to band here: the banded pipeline is test_pipeline_banded_under_graph_gpu's subject, this is the flags'.)"""
    select("hip")
    rng = np.random.default_rng(19)
    frames = [rng.integers(0, 256, size=ops.yuv_frame_bytes(9, 14), dtype=np.uint8) for _ in range(5)]
    data = _stream(b"YUV4MPEG2 W14 H9 F25:1 C420jpeg\n", frames)
    banded = _cli(cli_dir, data, "--bands", "on", "--band_rows", "4")
    assert banded.stdout == _cli(cli_dir, data).stdout
    out = video.Y4MReader(io.BytesIO(banded.stdout))
    assert (out.width, out.height) == (56, 36) and len(list(out.frames())) == 5


# ---------------------------------------------------------------------------------------------------- 8. the first size that needs it
@pytest.mark.gpu
def test_first_frame_size_that_needs_bands_gpu(pkg):
    """1024 x 2048: h w 1024 = 2^31 exactly, the smallest frame the whole path refuses.  (a) two band heights give the same bytes;
    (b) the bottom 64 output rows equal the unbanded tail on the last 34 rows of the same body output -- 2 halo rows (4 output rows)
    dropped at the top, the frame's edge at the bottom: the windows at the highest addresses against code that knows no bands."""
    dev = select("hip")
    G = _shipped(pkg, dev, "f16")
    h, w = 1024, 2048
    assert G.max_batch(h, w) == 0 and G.max_batch(h, w, bands=True) >= 1
    rng = np.random.default_rng(20)
    u8 = torch.from_numpy(rng.integers(0, 256, size=(1, h, w, 3), dtype=np.uint8)).to(dev)
    with torch.no_grad():
        a = G.forward_u8(u8, bands=64)
        assert a.shape == (1, 4 * h, 4 * w, 3)
        b = G.forward_u8(u8, bands=200)
        assert torch.equal(a, b)
        del b
        m = G._body(ops.u8_to_image(u8))
        H2 = m.shape[1]
        assert H2 == 2 * h
        ref = G._tail(m[:, H2 - 34:].contiguous(), G._cfg_head_u8)
        assert ref.shape == (1, 68, 4 * w, 3)
        assert torch.equal(a[:, -64:], ref[:, 4:])
    del a, m, ref
    torch.cuda.empty_cache()
