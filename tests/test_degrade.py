"""Training degradations (csrc/degrade.hip): blur, noise and the JPEG round trip against the numpy contract of
degrade_contract.py, the loader option, the configuration keys and the CLI tool.  Every device case runs on the emulator and, under
`-m gpu`, on the MI355X."""
import ctypes
import importlib
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

import degrade_contract as C
from backend import BACKENDS, L, ROOT, ops, select

pkg = importlib.import_module("fast-srgan_amd")
dataloader = importlib.import_module("fast-srgan_amd.dataloader")
train = importlib.import_module("fast-srgan_amd.train")

CAP = 1e-3                 # share of codes that may differ (by one) from the float64 contract: float32 against float64 rounding ties


@pytest.fixture(params=BACKENDS)
def dev(request):
    return select(request.param)


def _rand(shape, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------- 1. contract self-checks (CPU only)
def test_hash_statistics():
    n = 1 << 18
    z0, z1 = C.np_z(n, 0x1234567, 0x89abcdef), C.np_z(n, 0x1234568, 0x89abcdef)
    tol = 4.0 / np.sqrt(n)
    corr = lambda a, b: float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))
    print("mean %.3e var-1 %.3e corr(seeds) %.3e corr(e, e+1) %.3e (tolerance %.3e)"
          % (z0.mean(), z0.var() - 1, corr(z0, z1), corr(z0[:-1], z0[1:]), tol))
    assert np.isfinite(z0).all()
    assert abs(z0.mean()) < tol and abs(z0.var() - 1.0) < 4.0 * np.sqrt(2.0 / n)
    assert abs(corr(z0, z1)) < tol and abs(corr(z0[:-1], z0[1:])) < tol


# Margins [dB] by which PSNR(contract, libjpeg) must exceed PSNR(libjpeg, source): half the smallest value measured per class on
# C.synthetic_image at 24^2, 96^2 and 40x56 (DESIGN.md §6g lists the measurements).  "420" is lower: libjpeg up-samples chroma with a
# triangle filter, the contract replicates.
# Smallest measured: "444" q <= 50: 15.87 dB (96^2, q = 20 and 24^2, q = 50); "444" q = 95: 3.98 dB (24^2); "420" q <= 75: 4.38 dB (96^2, q = 75).
PIL_MARGIN = {("444", "low"): 7.9, ("444", 95): 1.99, ("420", "low"): 2.19}


@pytest.mark.parametrize("sub,q", [("444", 20), ("444", 50), ("444", 95), ("420", 20), ("420", 50), ("420", 75)])
def test_jpeg_contract_against_libjpeg(sub, q):
    from PIL import Image
    worst = 1e9
    for h, w in ((24, 24), (96, 96), (40, 56)):
        src = C.synthetic_image(h, w)
        buf = io.BytesIO()
        Image.fromarray(src.transpose(1, 2, 0)).save(buf, "JPEG", quality=q, subsampling=0 if sub == "444" else 2)
        pil = np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")).transpose(2, 0, 1)
        ours = C.np_jpeg_codes(src.astype(np.float32) / np.float32(127.5) - np.float32(1), q, sub)
        margin = C.psnr(ours, pil) - C.psnr(pil, src)
        print("libjpeg %s q=%d %dx%d: PSNR(contract, PIL) %.2f dB, PSNR(PIL, source) %.2f dB, margin %.2f dB"
              % (sub, q, h, w, C.psnr(ours, pil), C.psnr(pil, src), margin))
        worst = min(worst, margin)
    assert worst >= PIL_MARGIN[(sub, 95 if q == 95 else "low")], worst


# --------------------------------------------------------------------------------------------------------------------- 2. blur
BLUR_SHAPES = [(1, 1), (3, 5), (8, 8), (24, 24), (40, 56), (19, 130)]


@pytest.mark.parametrize("h,w", BLUR_SHAPES)
def test_blur_against_contract(dev, h, w):
    sig = [0.3, 0.0, 1.0, 3.0]
    x = _rand((4, 3, h, w), 10 + h)
    x[1, 0, 0, 0] = -0.0                                           # a copy keeps the sign of a zero; 0 + 1 * (-0) would not
    got = ops.degrade_blur_noise(_t(x, dev), sig, None, None).cpu().numpy()
    err = np.abs(got - C.np_blur(x, sig)).max()
    print("blur %dx%d: max |error| %.3e" % (h, w, err))
    assert err < 1e-5
    assert got[1].tobytes() == x[1].tobytes()                      # sigma = 0: bit-identical
    assert L.lib().fsr_last_kernel() == b"blur_hpass_kernel+blur_vpass_kernel"
    const = np.broadcast_to(np.float32([0.7, -0.31, 1.0])[None, :, None, None], (3, 3, h, w)).copy()
    got = ops.degrade_blur_noise(_t(const, dev), [0.3, 1.0, 3.0], None, None).cpu().numpy()
    assert np.abs(got - const).max() < 1e-6


# -------------------------------------------------------------------------------------------------------------------- 3. noise
def test_noise_against_contract(dev):
    x = _rand((3, 3, 19, 30), 3)
    sig, seeds = [25.0, 0.0, 0.7], [(0, 0), (5, 6), (0xffffffff, 0xfffffffe)]
    got = ops.degrade_blur_noise(_t(x, dev), None, sig, seeds).cpu().numpy()
    assert L.lib().fsr_last_kernel() == b"noise_kernel"
    want = C.np_noise(x, sig, seeds)
    for i, s in enumerate(sig):
        err = np.abs(got[i] - want[i]).max()
        gate = 2e-5 * s * (2.0 / 255.0) + 1e-7
        print("noise sigma %g: max |error| %.3e (gate %.3e)" % (s, err, gate))
        assert err < gate
    assert got[1].tobytes() == x[1].tobytes()                      # sigma_n = 0: untouched
    field = (got[0].astype(np.float64) - x[0]) / (25.0 * 2.0 / 255.0)
    assert 0.9 < field.std() < 1.1 and abs(field.mean()) < 0.15


def test_noise_fields_follow_the_seed_not_the_batch_position(dev):
    x = _rand((4, 3, 9, 13), 4)
    x[3] = x[0]
    a = ops.degrade_blur_noise(_t(x, dev), None, [5.0] * 4, [(1, 2), (1, 3), (2, 2), (1, 2)]).cpu().numpy()
    assert a[0].tobytes() == a[3].tobytes()                        # same seed, same input: same field at another batch position
    f = a - x
    assert not np.array_equal(f[0], f[1]) and not np.array_equal(f[0], f[2]) and not np.array_equal(f[1], f[2])
    b = ops.degrade_blur_noise(_t(x[3:], dev), None, [5.0], [(1, 2)]).cpu().numpy()
    assert b[0].tobytes() == a[0].tobytes()


@pytest.mark.parametrize("h,w", [(3, 5), (40, 56)])
def test_blur_plus_noise_is_blur_then_noise(dev, h, w):
    x = _t(_rand((4, 3, h, w), 5), dev)
    bs, ns, seeds = [0.0, 0.5, 2.2, 3.0], [3.0, 0.0, 12.0, 25.0], [(i, 7 * i + 1) for i in range(4)]
    fused = ops.degrade_blur_noise(x, bs, ns, seeds)
    assert L.lib().fsr_last_kernel() == b"blur_hpass_kernel+blur_vpass_noise_kernel"
    two = ops.degrade_blur_noise(ops.degrade_blur_noise(x, bs, None, None), None, ns, seeds)
    assert torch.equal(fused, two)


# ---------------------------------------------------------------------------------------------------- 4. JPEG on tie-free inputs
@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("q", [20, 50, 90])
def test_jpeg_tie_free(dev, q, sub):
    for h, w in ((16, 16), (32, 48), (96, 96)):
        x = C.tie_free_image(h, w, q, sub, seed=q + h)
        got = ops.jpeg_roundtrip(_t(x[None], dev), [q], sub).cpu().numpy()[0]
        C.assert_codes_close(C.value_to_codes(got), C.np_jpeg_codes(x, q, sub), CAP)
    assert L.lib().fsr_last_kernel() == b"jpeg_roundtrip_kernel<%s>" % sub.encode()


def test_float32_contract_is_inside_the_cap():
    """The room under CAP: the contract evaluated in float32 against itself in float64, on the tie-free inputs."""
    diff = total = 0
    for sub in ("420", "444"):
        for q in (20, 50, 90):
            x = C.tie_free_image(96, 96, q, sub, seed=q + 96)
            d = C.np_jpeg_codes(x, q, sub, np.float32) != C.np_jpeg_codes(x, q, sub)
            diff, total = diff + int(d.sum()), total + d.size
    print("float32 contract: %d of %d codes differ (%.2e)" % (diff, total, diff / total))
    assert diff <= CAP / 3 * total


# -------------------------------------------------------------------------------------------------- 5. JPEG on arbitrary inputs
# Fixture seeds chosen so that the contract alone leaves out at most a quarter of the pixels at q = 10 (0, 11, 23, 0, 0, 24 and 23 % here):
# a small picture has few blocks, and one coefficient near a tie takes a whole 16x16 MCU out.  The smallest seed that does is taken.
ARBITRARY_SEED = {(8, 8): 0, (24, 24): 14, (40, 56): 4, (17, 9): 2, (1, 1): 0, (16, 17): 0, (15, 33): 0}


def _arbitrary(h, w):
    seed = ARBITRARY_SEED[(h, w)]
    rs = np.random.RandomState(h * 131 + w + 1000 * seed)
    return ((C.synthetic_image(h, w, seed=h + w + seed) + rs.uniform(-0.5, 0.5, size=(3, h, w))) / 127.5 - 1.0).astype(np.float32)


@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("h,w", [(8, 8), (24, 24), (40, 56), (17, 9), (1, 1), (16, 17), (15, 33)])
def test_jpeg_arbitrary(dev, h, w, sub):
    x = _arbitrary(h, w)
    skip = C.tie_pixel_mask(x, 10, sub)
    print("jpeg %s %dx%d: %.1f %% of the pixels lie in a block with a coefficient near a tie" % (sub, h, w, 100.0 * skip.mean()))
    assert skip.mean() <= 0.40
    got = C.value_to_codes(ops.jpeg_roundtrip(_t(x[None], dev), [10], sub).cpu().numpy()[0])
    want = C.np_jpeg_codes(x, 10, sub)
    C.assert_codes_close(got[:, ~skip], want[:, ~skip], CAP)


@pytest.mark.parametrize("sub", ["420", "444"])
def test_jpeg_quality_100_and_quality_0(dev, sub):
    """q = 100 (every Q = 1) returns an image of integer codes within 1 code -- asserted on a GREY image.  Rounding 64 coefficients to
    integers leaves an error of standard deviation sqrt(1/12) = 0.29 codes in each plane, so a plane stays within 1 code (1.5 is more
    than 5 sigma); the inverse colour transform multiplies the chroma planes' errors by up to 1.772, and on a COLOURED image the float64
    contract itself is 2 codes away on 0.52 % ("444") and 0.35 % ("420", chroma constant over 2x2 blocks) of the codes of
    C.synthetic_image(24, 40).  The coloured image is therefore held to the contract instead: every code within 1 (a coefficient that
    rounds the other way moves a pixel by at most 0.25 * 1.772 < 0.5), at most 2 % of them different (64 coefficients per block, each
    within 1e-4 of a tie with probability 2e-4: about 1.3 % of the blocks hold one)."""
    img = C.synthetic_image(24, 40)
    if sub == "420":                       # chroma constant over 2x2 blocks: the subsampling then loses nothing
        img = np.repeat(np.repeat(img[:, ::2, ::2], 2, axis=1), 2, axis=2)
    grey = np.repeat(img[1:2], 3, axis=0)
    to_x = lambda a: a.astype(np.float32) / np.float32(127.5) - np.float32(1)
    x = np.stack([to_x(grey), to_x(img), _rand((3, 24, 40), 9)])
    x[2, 2, 3, 4] = -0.0
    got = ops.jpeg_roundtrip(_t(x, dev), [100, 100, 0], sub).cpu().numpy()
    d = np.abs(C.value_to_codes(got[0]) - grey.astype(np.int64))
    print("q = 100 %s, grey: max difference %d; coloured: max difference %d"
          % (sub, d.max(), np.abs(C.value_to_codes(got[1]) - img.astype(np.int64)).max()))
    assert d.max() <= 1
    C.assert_codes_close(C.value_to_codes(got[0]), C.np_jpeg_codes(x[0], 100, sub), 2e-2)
    C.assert_codes_close(C.value_to_codes(got[1]), C.np_jpeg_codes(x[1], 100, sub), 2e-2)
    assert got[2].tobytes() == x[2].tobytes()                      # q = 0: bit-identical


# ------------------------------------------------------------------------------------------------------------------- 6. loader
def _dataset(tmp_path, dev, count=3):
    paths = []
    for i in range(count):
        p = str(tmp_path / ("img%d.npy" % i))
        np.save(p, C.synthetic_image(40 + 3 * i, 44, seed=i))
        paths.append(p)
    return pkg.NumpyImagesDataset(paths, lr_image_size=8, scale_factor=4, device=dev)


def _batches(loader):
    return [(lr.clone(), hr.clone()) for lr, hr in loader]


ON = dict(blur_sigma=(0.2, 2.0), blur_prob=0.5, noise_sigma=(1, 10), noise_prob=0.5, jpeg_quality=(30, 95), jpeg_prob=0.7)


def test_loader_off_is_the_parent_path(dev, tmp_path):
    ds = _dataset(tmp_path, dev)
    base = _batches(pkg.DeviceBatchLoader(ds, 2, 3, seed=5))
    none = pkg.DeviceBatchLoader(ds, 2, 3, seed=5, degradation=None)
    zero = pkg.DeviceBatchLoader(ds, 2, 3, seed=5, degradation=dataloader.Degradation(seed=1))
    assert none.degradation is None and zero.degradation is None
    for other in (_batches(none), _batches(zero)):
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(base, other))


def test_loader_on(dev, tmp_path):
    ds = _dataset(tmp_path, dev)
    off = _batches(pkg.DeviceBatchLoader(ds, 2, 3, seed=5))
    on = _batches(pkg.DeviceBatchLoader(ds, 2, 3, seed=5, degradation=dataloader.Degradation(seed=1, **ON)))
    again = _batches(pkg.DeviceBatchLoader(ds, 2, 3, seed=5, degradation=dataloader.Degradation(seed=1, **ON)))
    other = _batches(pkg.DeviceBatchLoader(ds, 2, 3, seed=5, degradation=dataloader.Degradation(seed=2, **ON)))
    assert all(torch.equal(a[1], b[1]) for a, b in zip(off, on))                   # hr, and with it the crop and index sequence
    assert all(torch.equal(a[0], b[0]) for a, b in zip(on, again))
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(on, other))
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(on, off))
    # apply = the two operators called by hand with draw's parameters
    deg, twin = dataloader.Degradation(seed=1, **ON), dataloader.Degradation(seed=1, **ON)
    for (lr_off, _), (lr_on, _) in zip(off, on):
        p = deg.draw(2)
        assert p == twin.draw(2)
        by_hand = ops.jpeg_roundtrip(ops.degrade_blur_noise(lr_off, p.blur_sigma, p.noise_sigma, p.seeds), p.quality, "420")
        assert torch.equal(by_hand, lr_on) and torch.equal(deg.apply(lr_off, p), lr_on)


def test_draw_is_pinned():
    p = dataloader.Degradation(seed=0, **ON).draw(4)
    print(p)
    assert p == DRAW_SEED0
    # a stage's probability does not shift another stage's values
    q = dataloader.Degradation(seed=0, **dict(ON, blur_prob=1.0, jpeg_prob=1.0)).draw(4)
    assert q.seeds == p.seeds and all(a in (0.0, b) for a, b in zip(p.noise_sigma, q.noise_sigma))
    assert all(a in (0, b) for a, b in zip(p.quality, q.quality)) and all(a in (0.0, b) for a, b in zip(p.blur_sigma, q.blur_sigma))
    assert all(v > 0 for v in q.blur_sigma) and all(v > 0 for v in q.quality)


DRAW_SEED0 = dataloader.DegradeParams(
    blur_sigma=[0.0, 0.0, 0.0, 0.33273638053170523], noise_sigma=[3.3302507526366703, 0.0, 0.0, 0.0],
    seeds=[(2195908194, 2087043557), (598176026, 1210484339), (3479856542, 2585149702), (2404381470, 432508404)], quality=[68, 42, 0, 70])


def test_config_overrides_reach_the_loaders(tmp_path):
    dev = select("emu")
    ds = _dataset(tmp_path, dev)
    ov = ["training.batch_size=2", "training.iterations=2", "training.pretrain_iterations=1", "experiment.seed=11"]
    assert all(l.degradation is None for l in train.build_loaders(pkg.load_config(None, ov), ds))
    assert all(l.degradation is None for l in train.build_loaders(pkg.load_config(None, ov + ["data.degradation.jpeg_prob=0"]), ds))
    cfg = pkg.load_config(os.path.join(ROOT, "configs", "config.yaml"), ov + [
        "data.degradation.jpeg_prob=0.7", "data.degradation.jpeg_quality=[30,95]", "data.degradation.blur_prob=0.5",
        "data.degradation.blur_sigma=[0.2,2.0]", "data.degradation.noise_prob=0.5", "data.degradation.noise_sigma=[1,10]",
        "data.degradation.jpeg_subsampling=444"])
    loaders = train.build_loaders(cfg, ds, rank=0)
    for l in loaders:
        d = l.degradation
        assert (d.blur_sigma, d.blur_prob, d.noise_sigma, d.noise_prob) == ((0.2, 2.0), 0.5, (1.0, 10.0), 0.5)
        assert (d.jpeg_quality, d.jpeg_prob, d.jpeg_subsampling) == ((30, 95), 0.7, "444")
    seeds = [l.degradation.seed for l in loaders] + [l.degradation.seed for l in train.build_loaders(cfg, ds, rank=1)]
    assert len(set(seeds)) == 6
    lr, hr = next(iter(loaders[2]))
    assert lr.shape == (2, 3, 8, 8) and hr.shape == (2, 3, 32, 32) and torch.isfinite(lr).all()
    with pytest.raises(ValueError, match="unknown data.degradation"):
        train.build_loaders(pkg.load_config(None, ov + ["data.degradation.jpg_prob=1"]), ds)


@pytest.mark.gpu
def test_train_entry_point_trains_on_degraded_inputs(tmp_path, monkeypatch):
    """`python train.py data.degradation...` end to end, as tests/test_cli.py runs the plain command line."""
    import warnings
    select("hip")
    trainer_mod = importlib.import_module("fast-srgan_amd.trainer")
    npdir = tmp_path / "np"
    npdir.mkdir()
    for i in range(3):
        np.save(npdir / ("img%d.npy" % i), C.synthetic_image(90 + 7 * i, 120, seed=i))
    (tmp_path / "configs").mkdir()
    monkeypatch.chdir(tmp_path)
    real_vgg = trainer_mod.VGG19
    monkeypatch.setattr(trainer_mod, "VGG19", lambda **kw: real_vgg(width_div=8 if kw.get("compute_dtype") == "f32" else 2, seed=1, **kw))
    seen = []
    real_apply = dataloader.Degradation.apply
    monkeypatch.setattr(dataloader.Degradation, "apply", lambda self, lr, p, w=None: seen.append(p) or real_apply(self, lr, p, w))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        train.main(["data.numpy_dir=%s" % npdir, "data.lr_image_size=16", "data.scale_factor=4", "generator.n_filters=32",
                    "generator.n_layers=1", "discriminator.n_filters=32", "training.batch_size=2", "training.pretrain_iterations=2",
                    "training.iterations=3", "training.log_iter=1", "training.checkpoint_iter=3", "experiment.name=deg", "hydra.run.dir=run1",
                    "data.degradation.jpeg_prob=0.7", "data.degradation.jpeg_quality=[30,95]", "data.degradation.blur_prob=0.5",
                    "data.degradation.blur_sigma=[0.2,2.0]", "data.degradation.noise_prob=0.5", "data.degradation.noise_sigma=[1,10]"])
    assert len(seen) >= 5 and any(any(p.quality) for p in seen)          # 2 pre-training + 3 training batches, and validation
    sd = torch.load(tmp_path / "run1" / "runs" / "deg" / "generator_epoch_3.pt", map_location="cpu")
    assert all(torch.isfinite(v).all() for v in sd.values())


# ---------------------------------------------------------------------------------------------- 7. full size (-m gpu only)
@pytest.mark.gpu
@pytest.mark.parametrize("n,l", [(32, 96), (4, 128)])
def test_full_size(n, l):
    dev = select("hip")
    rs = np.random.RandomState(l)
    x = np.stack([(C.synthetic_image(l, l, seed=i % 3) / 127.5 - 1.0).astype(np.float32) for i in range(n)])
    x = np.clip(x + rs.uniform(-0.003, 0.003, size=x.shape), -1, 1).astype(np.float32)
    bs = [3.0] + [float(v) for v in rs.uniform(0.2, 3.0, size=n - 2)] + [0.8]
    ns = [25.0] + [float(v) for v in rs.uniform(0.5, 25.0, size=n - 2)] + [2.0]
    seeds = [(int(a), int(b)) for a, b in rs.randint(0, 2 ** 32, size=(n, 2), dtype=np.int64)]
    qs = [10] + [int(v) for v in rs.randint(1, 101, size=n - 2)] + [10]
    xt = _t(x, dev)
    blurred = ops.degrade_blur_noise(xt, bs, None, None)
    noisy = ops.degrade_blur_noise(blurred, None, ns, seeds)
    assert torch.equal(ops.degrade_blur_noise(xt, bs, ns, seeds), noisy)
    out = {s: ops.jpeg_roundtrip(noisy, qs, s) for s in ("420", "444")}
    b_np, n_np = blurred.cpu().numpy(), noisy.cpu().numpy()
    for i in (0, n - 1):
        one = slice(i, i + 1)
        err = np.abs(b_np[one] - C.np_blur(x[one], bs[one])).max()
        print("sample %d: blur error %.3e" % (i, err))
        assert err < 1e-5
        err = np.abs(n_np[one] - C.np_noise(b_np[one], ns[one], seeds[one])).max()
        print("sample %d: noise error %.3e" % (i, err))
        assert err < 2e-5 * ns[i] * (2.0 / 255.0) + 1e-7
        for s in ("420", "444"):
            skip = C.tie_pixel_mask(n_np[i], qs[i], s)
            print("sample %d %s: %.1f %% of the pixels left out" % (i, s, 100.0 * skip.mean()))
            assert skip.mean() <= 0.40
            got = C.value_to_codes(out[s][i].cpu().numpy())
            C.assert_codes_close(got[:, ~skip], C.np_jpeg_codes(n_np[i], qs[i], s)[:, ~skip], CAP)
            # the same sample at batch 1
            alone = ops.jpeg_roundtrip(ops.degrade_blur_noise(xt[one].contiguous(), bs[one], ns[one], seeds[one]), qs[one], s)
            assert torch.equal(alone[0], out[s][i])


# ------------------------------------------------------------------------------------- 8. argument errors and the CLI tool
def test_argument_errors(dev):
    lib = L.lib()
    x = _t(_rand((2, 3, 4, 4), 0), dev)
    p = x.data_ptr()
    err = lambda: lib.fsr_last_error().decode()
    assert lib.fsr_version() == L.ABI_VERSION
    assert lib.fsr_jpeg_roundtrip(p, p, 1, 32768, 32768, p, L.CHROMA_420, None) == -2 and "31 bits" in err()
    assert lib.fsr_degrade_blur_noise(p, p, p + 4, 1, 32768, 32768, p, p, None, None, None) == -2 and "31 bits" in err()
    assert lib.fsr_jpeg_roundtrip(p, p, 2, 4, 4, p, L.CHROMA_422, None) == -2 and "subsampling" in err()
    assert lib.fsr_jpeg_roundtrip(p, p, 0, 4, 4, p, L.CHROMA_420, None) == -2 and "positive" in err()
    assert lib.fsr_jpeg_roundtrip(None, p, 2, 4, 4, p, L.CHROMA_420, None) == -1 and "null" in err()
    assert lib.fsr_degrade_blur_noise(p, p, None, 2, 4, 4, p, p, None, None, None) == -1 and "tmp" in err()
    assert lib.fsr_degrade_blur_noise(p, p, p, 2, 4, 4, p, p, None, None, None) == -2 and "tmp" in err()
    assert lib.fsr_degrade_blur_noise(p, p, None, 2, 4, 4, None, None, p, None, None) == -1 and "seeds" in err()
    assert lib.fsr_degrade_blur_noise(p, p, None, 2, 4, 4, None, None, None, None, None) == -1 and "neither" in err()
    with pytest.raises(ValueError, match="blur sigma"):
        ops.degrade_blur_noise(x, [0.5, 3.5], None, None)
    with pytest.raises(ValueError, match="noise sigma"):
        ops.degrade_blur_noise(x, None, [1.0, 26.0], [(0, 0), (0, 0)])
    with pytest.raises(ValueError, match="seed"):
        ops.degrade_blur_noise(x, None, [1.0, 2.0], None)
    with pytest.raises(ValueError, match="quality"):
        ops.jpeg_roundtrip(x, [50, 101])
    with pytest.raises(ValueError, match="subsampling"):
        ops.jpeg_roundtrip(x, [50, 50], "422")
    with pytest.raises(ValueError, match="per-sample"):
        ops.jpeg_roundtrip(x, [50])
    with pytest.raises(ValueError, match="autograd"):
        ops.jpeg_roundtrip(x.clone().requires_grad_(), [50, 50])
    with pytest.raises(ValueError, match="autograd"):
        ops.degrade_blur_noise(x.clone().requires_grad_(), [1.0, 1.0], None, None)
    with pytest.raises(ValueError, match="float32"):
        ops.jpeg_roundtrip(x.double(), [50, 50])
    with pytest.raises(ValueError, match="blur_sigma"):
        dataloader.Degradation(blur_sigma=(0.5, 4.0))
    # per-sample arguments may be tensors
    a = ops.jpeg_roundtrip(x, torch.tensor([40, 0]), "444")
    assert torch.equal(a, ops.jpeg_roundtrip(x, [40, 0], "444"))


def test_cli_tool_round_trips_a_png(tmp_path):
    from PIL import Image
    select("emu")
    spec = importlib.util.spec_from_file_location("degrade_tool", os.path.join(ROOT, "tools", "degrade.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src = C.synthetic_image(20, 28)
    Image.fromarray(src.transpose(1, 2, 0)).save(str(tmp_path / "in.png"))
    assert tool.main(["--image", str(tmp_path / "in.png"), "--output", str(tmp_path / "same.png")]) == 0
    assert np.array_equal(np.array(Image.open(str(tmp_path / "same.png"))).transpose(2, 0, 1), src)       # nothing asked for: a copy
    args = ["--image", str(tmp_path / "in.png"), "--output", str(tmp_path / "out.png"), "--blur", "1.2", "--noise", "4", "--jpeg", "40",
            "--subsampling", "444", "--seed", "3"]
    assert tool.main(args) == 0
    out = np.array(Image.open(str(tmp_path / "out.png"))).transpose(2, 0, 1)
    x = _t((src.astype(np.float32) / np.float32(127.5) - np.float32(1))[None], torch.device("cpu"))
    want = ops.jpeg_roundtrip(ops.degrade_blur_noise(x, [1.2], [4.0], [tool.seed_words(3)]), [40], "444").numpy()[0]
    assert np.array_equal(out, C.value_to_codes(want)) and not np.array_equal(out, src)
