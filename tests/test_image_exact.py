"""Bit-exact and float64-referenced parity of the image path: fsr_crop_resize (data.hip), fsr_resample_image and its relatives
(resample.hip) and fsr_ssim_sse (metrics.hip), at the shapes where each kernel takes another path.

test_exact.py holds the convolutions bit for bit on integers, test_stream_exact.py the elementwise kernels per element against
float64.  The three files here had whole-tensor tolerances only (1e-5 and 2e-5 absolute: 80 and 170 float32 ulp at 1; a per-image
SSIM mean in which one pixel of the map weighs 1 / 5670).  All three take their inputs in a form that allows an exact test:

  * The crop and the resampler receive their TAP TABLES from the caller.  The index tables stay the contract's (xmin, xsize of
    dataloader.aa_bicubic_taps: window_rows and the LDS budget stay valid); only the weights are replaced by multiples of 1/16 --
    integers in [-3, 7] over 16, one entry of a row moved so that the row sums to 16/16 (dyadic_taps, pinned seed).  With inputs
    on a coarse binary grid (u8 codes for the crop; c = (t + 1) / 2 in steps of 1/64 for the resampler) every product and every
    partial sum of both passes is exactly representable in float32, in any order, fused or not.  PREMISE, asserted on the float64
    reference before a kernel's result is looked at: the composition of magnitudes |My| |c| |Mx|^T times the reciprocal of the
    lsb (2^-8 for the crop, 2^-14 for the resampler) is below 2^24, and the reference times that reciprocal is an integer.  The
    kernel must then reproduce float64 with NO tolerance, negative weights and results far outside [0, 1] included (the clamp of
    the u8 and planar kinds is exercised: the reference runs from about -2.5 to 3.5).  A premise failure is a bug of the input
    generator, never a skip.
      crop     : hr_out == float32(u8) / 127.5f - 1 (one correctly rounded division, one subtraction); tmp == the exact row sums,
                 so a fault localises to a pass; lr_out == the same two operations on the exact s.
      resample : f32 == 2 v - 1; u8 == trunc(255 clip(v, 0, 1)); the planar kinds (4:2:0 planar and NV12, 4:2:2, 4:4:4, depths 8,
                 10 and 16, (bt601, limited) and (bt709, full)) == ops.image_to_yuv of the exact float32 image 2 clip(v, 0, 1) - 1,
                 byte for byte: the comparison test_encode_is_the_resamplers_planar_stage_at_the_native_size makes at identity
                 taps, carried to real resizes.  fsr_resample_image(FSR_OUT_I420) and fsr_resample_image_i420_deep, which the
                 Python wrapper never reaches, are called directly on the same tables.
  * fsr_ssim_sse takes caller-owned scratch: the [n][3 * tiles][2] per-tile partials are read back after the call.  With inputs in
    steps of 1/16 the squared error is exact per tile (a tile owns its 32 x 32 block; the last tile row and column also own the
    image's last 10 rows and columns) and per image.  The SSIM sums are held per tile to the float64 evaluation of the documented
    formula with the kernel's float32 taps.

Paths reached, asserted: the tap instantiation from fsr_last_kernel (",5" every up-scale, ",9" down-scales up to 2, ",0" above);
the row-tile height from a Python restatement of window_rows and the halving loop of resample_launch.  th = 32, 16, 8 and 4 are each
reached with at least two tile rows and a partial last one.  th = 2 is UNREACHABLE under the ratio cap of 8: a 4-row tile at ratio
8 needs at most int(8 * 3.5 + 16.5) - int(8 * 0.5 - 15.5) = 57 source rows, and 85 fit the LDS budget (83 rows of the 196-float rows
of 4:2:2) -- no case is invented for it.  Output widths 4, 64, 66 and 130 (a narrow tile, a full one, a tile plus 2 columns, two
seams and a partial third tile: the 4:2:2 left-neighbour column is taken at x0 = 64 and 128 and clamped at x0 = 0); 65 and 67 for
the f32 / u8 / 4:4:4 kinds (cnt = 1 .. 3 and the unaligned-store branch of the f32 path).  n = 2 everywhere (n = 3 for the crop).
Crop: scales 2, 3, 4 and 8 at hr = 48, 64, 256, 258, 300 and 516 wherever the scale divides hr -- 257, the size just past the
256-thread stride, is prime and divides by no scale (it is one of the refusals); 258 = 2 * 3 * 43 takes its place -- each batch with
three image sizes (odd widths among them), one crop at (0, 0), one flush with the bottom right corner, one interior; and
(lr 212, scale 2, n 4), whose 539 328 outputs exceed the 2048 x 256 threads of crop_vpass_kernel's capped grid (it runs on the
emulator too: under a second).

Where real weights are used (the CONTRACT legs, dataloader.aa_bicubic_taps) the result is held per element to the float64
evaluation from the same float32 tables:
    crop     |lr  - ref64| <= K 2^-23 (sum_jk |wy_j| |wx_k| |x_jk| / 127.5 + 1)
    resample |got - ref64| <= K 2^-23 (2 sum_jk |wy_j| |wx_k| |c_jk| + 1)
    SSIM     |tile sum - ref64| <= K 2^-23 sum_i s_i + (terms + 8) 2^-24 sum_i |ssim_i|
             s_i = |ssim_i| + |N1| E / (D1 D2) + |ssim_i| E / D2,  N1 = 2 mu_ab + c1,  D1 = mu_aa + mu_bb + c1,
             D2 = var_a + var_b + c2,  E = E[aa] + E[bb] + 2 |E[ab]| + mu_aa + mu_bb + 2 |mu_ab|  (the magnitudes entering the two
             cancellations var = E[xx] - mu_xx and cov = E[ab] - mu_ab); the per-image sums take the same form over all their terms.
K is found as in test_stream_exact.py: the smallest power of two (>= 1) for which a float32 numpy restatement of the kernel's
statements stays inside ONE THIRD of the cap on the very inputs of the cases (test_float32_restatements_are_inside_a_third_of_the_caps
asserts it, and that K is the smallest such power).  The other two thirds are the room for fused multiply-adds and another
association on the device.  Largest |result - ref64|, for the crop and the resampler in units of 2^-23 s (the units K counts), for
SSIM as a share of the K = 1 cap:

    kernel                 K    restatement   emulator   MI355X
    crop lr                4    1.16          1.16       1.05
    resample f32           8    1.43          1.43       1.58
    ssim per tile          1    0.197         0.197      0.207
    ssim per image         1    0.102         0.102      0.141

(The emulator does not contract and reproduces the restatement to the digit; the MI355X fuses.  Per PIXEL the SSIM restatement
reaches 0.436 of 2^-23 s_i.  Identical images give exactly the pixel count per tile on the emulator and come within 0.10 of the
cap on the MI355X, whose fused var = E[aa] - mu_aa no longer cancels to the bit.  Every exact leg, all 24 planar combinations of
every shape included, is bit-equal on the MI355X as well: no combination had to fall back to np_encode under yuv_contract's cap.)

What the SSIM gate resolves (test_image_gates_are_sharper_than_the_tolerance_gates): at test_ops.py's 45 x 64 shape a 1 % error in
one pixel of the map is 19.8 caps in the 3 x 22 corner tile and 11.4 in the 3 x 32 one, against a sixth of the old gate; in a full
32 x 32 tile it is 0.15 of the cap, which the fixed-order summation term (terms + 8) 2^-24 sum |ssim_i| dominates there -- a full
tile resolves 7 % of one pixel.  The shapes above therefore put 1 x 1, 1 x 32, 32 x 1, 2 x 1 and 32 x 2 tiles next to full ones.

Every figure goes to the parity-error log through backend.report as image.<backend>.<key>, when it exceeds the previous maximum.
"""
import collections
import functools
import importlib

import numpy as np
import pytest
import torch

from backend import BACKENDS, L, ops, report, select

data = importlib.import_module("fast-srgan_amd.dataloader")

F32, F64 = np.float32, np.float64
U = 2.0 ** -23
GPU = pytest.mark.gpu
K_CROP, K_RESAMPLE, K_SSIM = 4, 8, 1
CROP_LSB, RS_LSB = 2.0 ** -8, 2.0 ** -14
RS_TW, RS_LDS_BUDGET = 64, 64 * 1024         # resample.hip
TILE, PADW = 32, 5                           # metrics.hip

Taps = collections.namedtuple("Taps", "xmin xsize w kmax M")     # M: the dense float64 (out, in) matrix of the table


def _cases(both=(), hip=()):
    """(backend, *case): `both` on the emulator and the MI355X, `hip` on the MI355X only."""
    return [pytest.param("emu", *c) for c in both] + [pytest.param("hip", *c, marks=GPU) for c in tuple(both) + tuple(hip)]


_worst, _backend = {}, ["-"]


def _select(backend):
    _backend[0] = backend
    return select(backend)


def _note(key, value):
    """The largest figure of a key so far goes to the parity-error log as image.<backend>.<key>."""
    key = "image.%s.%s" % (_backend[0], key)
    if value > _worst.get(key, -1.0):
        _worst[key] = value
        report(key, value)


# ------------------------------------------------------------------------------------------------- tap tables
def dense(xmin, xsize, w, in_size):
    """The (out, in) float64 matrix a tap table stands for."""
    M = np.zeros((len(xmin), in_size), F64)
    for i in range(len(xmin)):
        M[i, xmin[i]:xmin[i] + xsize[i]] = w[i, :xsize[i]].astype(F64)
    return M


def dyadic_taps(xmin, xsize, kmax, rng):
    """Weights for the contract's index tables: per row integers in [-3, 7] over 16, one entry moved so that the row sums to 16/16."""
    w = np.zeros((len(xmin), kmax), F32)
    for i in range(len(xmin)):
        n = int(xsize[i])
        row = rng.integers(-3, 8, size=n)
        row[int(rng.integers(0, n))] += 16 - int(row.sum())
        assert row.sum() == 16
        w[i, :n] = row.astype(F32) / F32(16)
    return w


@functools.lru_cache(maxsize=None)
def _taps(in_size, out_size, dyadic=True):
    xmin, xsize, w, kmax = data.aa_bicubic_taps(in_size, out_size)
    if dyadic:
        w = dyadic_taps(xmin, xsize, kmax, np.random.default_rng(7919 * in_size + out_size))
    for a in (xmin, xsize, w):
        a.setflags(write=False)
    return Taps(xmin, xsize, w, int(kmax), dense(xmin, xsize, w, in_size))


def _dev_taps(T, dev):
    return torch.from_numpy(T.w.copy()).to(dev), torch.from_numpy(T.xmin.copy()).to(dev), torch.from_numpy(T.xsize.copy()).to(dev), T.kmax


def premise(what, ref, mag, lsb):
    """The exactness premise, on the float64 reference alone."""
    top = float(np.max(mag)) / lsb
    assert top < 2 ** 24, "premise (an input bug): %s: sum of magnitudes %g lsb reaches 2^24" % (what, top)
    q = np.asarray(ref) / lsb
    assert np.array_equal(q, np.rint(q)), "premise (an input bug): %s: the reference is not a multiple of the lsb %g" % (what, lsb)
    _note("premise.%s.max_magnitude_in_lsb" % what, top)
    _note("premise.%s.max_abs_reference" % what, float(np.abs(ref).max()))


# ------------------------------------------------------------------------------------------------- comparisons
def _where(got, ref, th=None):
    """Mismatch pattern of a (..., y, x) array: the first indices and, for 4-D results, the counts per tile row and column."""
    bad = np.argwhere(got != ref)
    msg = "%d of %d differ; first (index: got, want): %s" % (len(bad), ref.size, [
        (tuple(int(v) for v in i), float(got[tuple(i)]), float(ref[tuple(i)])) for i in bad[:6]])
    if ref.ndim == 4 and len(bad):
        th = th or 32
        msg += "; per tile row (y // %d) %s, per tile column (x // 64) %s, x %% 4 %s, images %s, channels %s" % (
            th, np.bincount(bad[:, 2] // th).tolist(), np.bincount(bad[:, 3] // RS_TW).tolist(), sorted(set(int(v) % 4 for v in bad[:, 3])),
            sorted(set(int(v) for v in bad[:, 0])), sorted(set(int(v) for v in bad[:, 1])))
    return msg


def exact(what, got, ref, th=None):
    """THE comparison of the exact legs: np.array_equal, dtype included."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    assert np.array_equal(got, ref), "%s: %s" % (what, _where(got, ref, th))


def gate(key, what, got, ref, scale, K):
    """THE per-element comparison of the contract legs: |got - ref| <= K 2^-23 scale.  Returns the largest error in units of 2^-23 scale."""
    got, ref, scale = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(scale, F64)
    assert got.shape == ref.shape == scale.shape, (what, got.shape, ref.shape, scale.shape)
    assert np.isfinite(got).all(), "%s: non-finite values" % what
    units = np.abs(got - ref) / (U * scale)
    if key:
        _note(key, float(units.max()))
    i = np.unravel_index(int(np.argmax(units)), units.shape)
    assert units.max() <= K, "%s: %d of %d over the cap; worst at %s: got %.9g, want %.9g, %.3g units of 2^-23 s (K = %d)" % (
        what, int((units > K).sum()), units.size, tuple(int(v) for v in i), got[i], ref[i], units[i], K)
    return float(units.max())


def _apply32(x, T, axis):
    """One pass of either kernel in float32 numpy: acc = 0; acc += w[o][k] * x[xmin[o] + k] for k = 0 .. kmax - 1, one rounding per
    operation (the weights beyond xsize are zero: adding 0 changes nothing)."""
    x = np.moveaxis(x, axis, -1)
    acc = np.zeros(x.shape[:-1] + (len(T.xmin),), F32)
    for k in range(T.kmax):
        acc = acc + T.w[:, k] * x[..., np.minimum(T.xmin + k, x.shape[-1] - 1)]
    return np.moveaxis(acc, -1, axis)


# ------------------------------------------------------------------------------------------------- 1. fsr_crop_resize
CROP_SCALES = (2, 3, 4, 8)
CROP_HR = (48, 64, 256, 258, 300, 516)
CROP_EXACT = [(hr, s, 3) for s in CROP_SCALES for hr in CROP_HR if hr % s == 0]
CROP_CAPPED = (424, 2, 4)                    # lr 212: 4 * 3 * 212 * 212 = 539 328 > 2048 * 256
CROP_CONTRACT = [(48, 4, 3), (64, 2, 3), (300, 3, 3)]
assert CROP_CAPPED[2] * 3 * (CROP_CAPPED[0] // CROP_CAPPED[1]) ** 2 > 2048 * 256


@functools.lru_cache(maxsize=4)
def _crop_batch(hr, n):
    """n uint8 (3, H, W) images of n different sizes, odd widths among them; crops: (0, 0), flush with the bottom right corner,
    interior, ..."""
    rng = np.random.default_rng(1000 + hr)
    pads = [(3, 5), (6, 9), (8, 4), (1, 2)][:n]
    imgs = [rng.integers(0, 256, size=(3, hr + dy, hr + dx), dtype=np.uint8) for dy, dx in pads]
    crops = [(0, 0), pads[1], (3, 2), (1, 0)][:n]
    assert len(set(im.shape for im in imgs)) == n and any(im.shape[2] % 2 for im in imgs)
    assert crops[1] == (imgs[1].shape[1] - hr, imgs[1].shape[2] - hr) and 0 < crops[2][0] < pads[2][0] and 0 < crops[2][1] < pads[2][1]
    x = np.stack([im[:, cy:cy + hr, cx:cx + hr] for im, (cy, cx) in zip(imgs, crops)])
    return imgs, crops, x


def _crop_call(dev, imgs, crops, hr, scale, T, hr_out=None, lr_out=None, tmp=None, check=True, over=()):
    """fsr_crop_resize as dataloader.NumpyImagesDataset.batch calls it; `over`: arguments replaced for the refusals."""
    n, lr = len(imgs), max(hr // scale, 1)
    dimgs = [torch.from_numpy(im).to(dev) for im in imgs]
    ptrs = torch.tensor([t.data_ptr() for t in dimgs], dtype=torch.int64).to(dev)
    meta = torch.tensor([[im.shape[1] for im in imgs], [im.shape[2] for im in imgs], [c[0] for c in crops], [c[1] for c in crops]],
                        dtype=torch.int32).to(dev)
    w, xmin, xsize, kmax = _dev_taps(T, dev)
    nan = float("nan")
    hr_out = torch.full((n, 3, hr, hr), nan, dtype=torch.float32, device=dev) if hr_out is None else hr_out
    lr_out = torch.full((n, 3, lr, lr), nan, dtype=torch.float32, device=dev) if lr_out is None else lr_out
    tmp = torch.full((n, 3, hr, lr), nan, dtype=torch.float32, device=dev) if tmp is None else tmp
    a = dict(images=ptrs.data_ptr(), img_h=meta[0].data_ptr(), img_w=meta[1].data_ptr(), crop_y=meta[2].data_ptr(), crop_x=meta[3].data_ptr(),
             n=n, hr=hr, scale=scale, w=w.data_ptr(), xmin=xmin.data_ptr(), xsize=xsize.data_ptr(), kmax=kmax, hr_out=hr_out.data_ptr(),
             lr_out=lr_out.data_ptr(), tmp=tmp.data_ptr())
    a.update(dict(over))
    rc = L.lib().fsr_crop_resize(a["images"], a["img_h"], a["img_w"], a["crop_y"], a["crop_x"], a["n"], a["hr"], a["scale"], a["w"], a["xmin"],
                                 a["xsize"], a["kmax"], a["hr_out"], a["lr_out"], a["tmp"], ops._stream())
    if check:
        L.check(rc, "fsr_crop_resize")
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return rc, hr_out, lr_out, tmp


def _to_pm1(s):
    """s / 127.5f - 1 in float32 numpy: one correctly rounded division and one subtraction."""
    return s.astype(F32) / F32(127.5) - F32(1)


def _crop_exact(backend, hr, scale, n):
    dev = _select(backend)
    imgs, crops, x = _crop_batch(hr, n)
    T = _taps(hr, hr // scale)
    x64 = x.astype(F64)
    tmp_ref = x64 @ T.M.T                                          # (n, 3, hr, lr)
    s_ref = np.einsum("oy,ncyx->ncox", T.M, tmp_ref)               # (n, 3, lr, lr)
    aM = np.abs(T.M)
    premise("crop.%d.x%d" % (hr, scale), s_ref, np.einsum("oy,ncyx->ncox", aM, x64 @ aM.T), CROP_LSB)
    assert np.array_equal(tmp_ref * 16, np.rint(tmp_ref * 16))
    _, hr_out, lr_out, tmp = _crop_call(dev, imgs, crops, hr, scale, T)
    exact("hr_out", hr_out, _to_pm1(x))
    exact("tmp (the horizontal pass)", tmp, tmp_ref.astype(F32))
    exact("lr_out (the vertical pass)", lr_out, _to_pm1(s_ref))


@pytest.mark.parametrize("backend,hr,scale,n", _cases(both=CROP_EXACT))
def test_crop_resize_is_exact_with_dyadic_taps(backend, hr, scale, n):
    """fsr_crop_resize at every scale and at hr below, at and beyond the 256-thread stride of crop_hpass_kernel, three images of
    different sizes in one call: hr_out, tmp and lr_out bit for bit."""
    _crop_exact(backend, hr, scale, n)


@pytest.mark.parametrize("backend", BACKENDS)
def test_crop_resize_is_exact_past_the_capped_grid(backend):
    """lr 212, scale 2, n 4: crop_vpass_kernel's grid is capped at 2048 workgroups and every thread takes a second element."""
    _crop_exact(backend, *CROP_CAPPED)


def _crop_contract_case(hr, scale, n):
    """(float64 reference of lr, the cap's scale, the float32 restatement) for the real taps."""
    _, _, x = _crop_batch(hr, n)
    T = _taps(hr, hr // scale, dyadic=False)
    x64, aM = x.astype(F64), np.abs(T.M)
    ref = np.einsum("oy,ncyx->ncox", T.M, x64 @ T.M.T) / 127.5 - 1
    scale_ = np.einsum("oy,ncyx->ncox", aM, x64 @ aM.T) / 127.5 + 1
    return T, ref, scale_, _to_pm1(_apply32(_apply32(x.astype(F32), T, 3), T, 2))


@pytest.mark.parametrize("backend,hr,scale,n", _cases(both=CROP_CONTRACT))
def test_crop_resize_contract_taps_against_float64(backend, hr, scale, n):
    """The real aa_bicubic_taps weights: lr_out per element within K 2^-23 (sum |wy| |wx| |x| / 127.5 + 1) of float64."""
    dev = _select(backend)
    imgs, crops, x = _crop_batch(hr, n)
    T, ref, scale_, _ = _crop_contract_case(hr, scale, n)
    _, hr_out, lr_out, _ = _crop_call(dev, imgs, crops, hr, scale, T)
    exact("hr_out", hr_out, _to_pm1(x))
    gate("crop_lr.%d.x%d" % (hr, scale), "lr_out", lr_out.cpu().numpy(), ref, scale_, K_CROP)


@pytest.mark.parametrize("backend", BACKENDS)
def test_crop_resize_refusals_leave_the_outputs_untouched(backend):
    """Null pointers, hr % scale != 0 (257 among them), non-positive sizes and a crop row beyond 60 KiB of LDS: a negative code, its
    message in fsr_last_error, and not one output element written."""
    dev = _select(backend)
    imgs, crops, _ = _crop_batch(48, 3)
    T = _taps(48, 12)
    bufs = [torch.full((3, 3, 48, s), 777.0, dtype=torch.float32, device=dev) for s in (48, 12, 12)]
    rows = [(dict(images=None), b"null"), (dict(img_h=None), b"null"), (dict(crop_x=None), b"null"), (dict(w=None), b"null"),
            (dict(xsize=None), b"null"), (dict(hr_out=None), b"null"), (dict(lr_out=None), b"null"), (dict(tmp=None), b"null"),
            (dict(hr=50, scale=4), b"bad sizes"), (dict(hr=257, scale=2), b"bad sizes"), (dict(hr=257, scale=8), b"bad sizes"),
            (dict(n=0), b"bad sizes"), (dict(n=-1), b"bad sizes"), (dict(hr=0), b"bad sizes"), (dict(hr=-48), b"bad sizes"),
            (dict(scale=0), b"bad sizes"), (dict(scale=-4), b"bad sizes"), (dict(hr=15364, scale=4), b"does not fit in LDS")]
    for over, word in rows:
        rc, _, _, _ = _crop_call(dev, imgs, crops, 48, 4, T, bufs[0], bufs[1], bufs[2], check=False, over=over)
        assert rc < 0 and word in L.lib().fsr_last_error(), (over, rc, L.lib().fsr_last_error())
        assert all(bool((b == 777.0).all()) for b in bufs), over
    assert _crop_call(dev, imgs, crops, 48, 4, T, bufs[0], bufs[1], bufs[2])[0] == 0              # ... and the same call, whole, is served
    assert not bool((bufs[1].flatten()[:3 * 3 * 12 * 12] == 777.0).any())


# ------------------------------------------------------------------------------------------------- 2. fsr_resample_image and its relatives
def window_rows(n_in, n_out, th):
    """resample.hip's window_rows: the largest source-row window of any tile of th output rows."""
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    rows = 1
    for y0 in range(0, n_out, th):
        y1 = min(y0 + th, n_out) - 1
        lo = max(int(scale * (y0 + 0.5) - support + 0.5), 0)
        hi = min(int(scale * (y1 + 0.5) + support + 0.5), n_in)
        rows = max(rows, hi - lo)
    return rows


def tile_rows(n_in, n_out, rowf):
    """The halving loop of resample_launch: the largest th of 32, 16, 8, 4, 2 whose window fits the LDS budget; None: refused."""
    th = 32
    while window_rows(n_in, n_out, th) * rowf * 4 > RS_LDS_BUDGET:
        if th == 2:
            return None
        th >>= 1
    return th


#            (h, w) -> (oh, ow)           th   taps    what it reaches
RS_SHAPES = [((60, 44), (40, 66), 32, 5),      # up-scale along x: a tile plus 2 columns; tile rows of 32 + 8
             ((120, 128), (40, 64), 16, 9),    # ratio 2 along x: one full tile; tile rows of 16 + 16 + 8
             ((120, 390), (20, 130), 8, 0),    # ratio 3 along x: two seams and a partial third tile; tile rows of 8 + 8 + 4
             ((144, 8), (18, 4), 4, 9)]        # ratio 8 along y: tile rows of 4 + 4 + 4 + 4 + 2; one narrow tile
RS_ODD = [((24, 40), (38, 65), 32, 5),         # a tile plus 1 column
          ((24, 134), (38, 67), 32, 9)]        # a tile plus 3 columns
RS_CONTRACT = RS_SHAPES[:3]
RS_COLOURS = (("bt601", False), ("bt709", True))
RS_DEPTHS = (8, 10, 16)
RS_PLANAR = (("420", "planar"), ("420", "nv12"), ("422", "planar"), ("444", "planar"))
_rs_id = lambda v: "%dx%d" % v if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], int) else None   # noqa: E731


def test_resample_shapes_reach_every_tile_height_and_th_2_is_unreachable():
    """The cases reach th = 32, 16, 8 and 4 with at least two tile rows and a partial last one, for the 192-float rows and for the
    196-float rows of 4:2:2; under the ratio cap of 8 no size reaches th = 2."""
    for rowf in (192, 196):
        seen = set()
        for (h, w), (oh, ow), th, _ in RS_SHAPES + RS_ODD:
            assert tile_rows(h, oh, rowf) == th, ((h, oh), rowf, tile_rows(h, oh, rowf))
            assert oh > th and oh % th, "%d -> %d: th %d needs two tile rows and a partial last one" % (h, oh, th)
            seen.add(th)
        assert seen == {32, 16, 8, 4}
        for oh in list(range(1, 70)) + [128, 270, 1080]:
            for h in (8 * oh, 8 * oh - 1, 8 * oh - 7):
                assert tile_rows(h, oh, rowf) >= 4, (h, oh, rowf)
    assert sorted(set(ow for _, (_, ow), _, _ in RS_SHAPES)) == [4, 64, 66, 130] and [ow for _, (_, ow), _, _ in RS_ODD] == [65, 67]


@functools.lru_cache(maxsize=None)
def _rs_case(hw, size, dyadic=True):
    """(t NHWC float32, float64 v = My c Mx^T as (n, oh, ow, 3), |My| |c| |Mx|^T, the two tables).  dyadic: c in steps of 1/64."""
    (h, w), (oh, ow) = hw, size
    rng = np.random.default_rng(100000 * h + 1000 * w + oh)
    if dyadic:
        c = rng.integers(0, 65, size=(2, h, w, 3)).astype(F64) / 64
        t = (2 * c - 1).astype(F32)
        assert np.array_equal(t.astype(F64), 2 * c - 1)
    else:
        t = (rng.random((2, h, w, 3)) * 2 - 1).astype(F32)
        c = (t.astype(F64) + 1) / 2
    Ty, Tx = _taps(h, oh, dyadic), _taps(w, ow, dyadic)
    v = np.einsum("px,noxc->nopc", Tx.M, np.einsum("oy,nyxc->noxc", Ty.M, c))
    mag = np.einsum("px,noxc->nopc", np.abs(Tx.M), np.einsum("oy,nyxc->noxc", np.abs(Ty.M), np.abs(c)))
    for a in (t, v, mag):
        a.setflags(write=False)
    return t, v, mag, Ty, Tx


def _plant(monkeypatch, dev, hw, size, Ty, Tx):
    """The tables the wrapper will find in its cache, for this test only: monkeypatch puts the real ones back."""
    for n_in, n_out, T in ((hw[0], size[0], Ty), (hw[1], size[1], Tx)):
        monkeypatch.setitem(ops._aa_taps_cache, (n_in, n_out, str(torch.device(dev))), _dev_taps(T, dev))


def _kernel_is(kind, kxs, sample=""):
    name = L.lib().fsr_last_kernel().decode()
    assert name == "resample_kernel<%s,%d%s>" % (kind, kxs, sample), name


def _nchw(a):
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))


@pytest.mark.parametrize("kind", ("f32", "u8"))
@pytest.mark.parametrize("backend,hw,size,th,kxs", _cases(both=RS_SHAPES + RS_ODD), ids=_rs_id)
def test_resample_f32_and_u8_are_exact_with_dyadic_taps(backend, hw, size, th, kxs, kind, monkeypatch):
    """f32 == 2 v - 1 and u8 == trunc(255 clip(v, 0, 1)), bit for bit, at every tile height, tap instantiation and output width."""
    dev = _select(backend)
    t, v, mag, Ty, Tx = _rs_case(hw, size)
    premise("resample.%dx%d-%dx%d" % (hw + size), v, mag, RS_LSB)
    clipped = float(((v < 0) | (v > 1)).mean())
    assert clipped > 0.01 and v.min() < -0.5 and v.max() > 1.5, "premise (an input bug): the clamp is not exercised (%g clipped)" % clipped
    _plant(monkeypatch, dev, hw, size, Ty, Tx)
    got = ops.resample_image(torch.from_numpy(t.copy()).to(dev), *size, kind=kind)
    _kernel_is(kind, kxs)
    if kind == "f32":
        assert got.shape == (2, 3) + size
        exact("f32 output", got, _nchw((2 * v - 1).astype(F32)), th)
    else:
        assert got.shape == (2,) + size + (3,)
        exact("u8 codes", _nchw(got.cpu().numpy()), _nchw(np.trunc(255 * np.clip(v, 0, 1)).astype(np.uint8)), th)


def _planar_shapes(chroma):
    rows = RS_SHAPES + (RS_ODD if chroma == "444" else [])
    return [r for r in rows if (chroma == "444" or r[1][1] % 2 == 0) and (chroma != "420" or r[1][0] % 2 == 0)]


def _planes(payload, n, oh, ow, chroma, depth, layout):
    """(n, bytes) payload -> the list of its planes as 4-D arrays (n, 1, rows, columns), for the mismatch message."""
    s = payload if depth == 8 else np.ascontiguousarray(payload).view("<u2")
    ch, cw = (oh // 2 if chroma == "420" else oh), (ow if chroma == "444" else ow // 2)
    y = s[:, :oh * ow].reshape(n, 1, oh, ow)
    if layout == "nv12":
        return [y, s[:, oh * ow:].reshape(n, 1, ch, 2 * cw)]
    return [y, s[:, oh * ow:oh * ow + ch * cw].reshape(n, 1, ch, cw), s[:, oh * ow + ch * cw:].reshape(n, 1, ch, cw)]


RS_PLANAR_CASES = [shape + kind for kind in RS_PLANAR for shape in _planar_shapes(kind[0])]     # odd extents: only where the subsampling holds them


@pytest.mark.parametrize("backend,hw,size,th,kxs,chroma,layout", _cases(both=RS_PLANAR_CASES), ids=_rs_id)
def test_resample_planar_kinds_equal_the_encode_of_the_exact_image(backend, hw, size, th, kxs, chroma, layout, monkeypatch):
    """4:2:0 planar and NV12, 4:2:2 and 4:4:4 at depths 8, 10 and 16 in (bt601, limited) and (bt709, full): the bytes equal
    ops.image_to_yuv of the exact float32 image 2 clip(v, 0, 1) - 1.  4:2:0 planar also through fsr_resample_image(FSR_OUT_I420)
    and fsr_resample_image_i420_deep, the entry points the wrapper does not use."""
    dev = _select(backend)
    t, v, mag, Ty, Tx = _rs_case(hw, size)
    premise("resample.%dx%d-%dx%d" % (hw + size), v, mag, RS_LSB)
    assert tile_rows(hw[0], size[0], 196 if chroma == "422" else 192) == th
    _plant(monkeypatch, dev, hw, size, Ty, Tx)
    img = (2 * np.clip(v, 0, 1) - 1).astype(F32)
    assert np.array_equal(img.astype(F64), 2 * np.clip(v, 0, 1) - 1)
    td, imgd = torch.from_numpy(t.copy()).to(dev), torch.from_numpy(img).to(dev)
    (h, w), (oh, ow) = hw, size
    name = {("420", "planar"): "i420", ("420", "nv12"): "nv12", ("422", "planar"): "yuv422", ("444", "planar"): "yuv444"}[(chroma, layout)]
    for depth in RS_DEPTHS:
        for matrix, full in RS_COLOURS:
            want = ops.image_to_yuv(imgd, chroma, matrix, full, depth, layout).cpu().numpy()
            got = ops.resample_image(td, oh, ow, kind="i420", matrix=matrix, full_range=full, depth=depth, chroma=chroma, layout=layout)
            _kernel_is(name, kxs, ",u16" if depth != 8 else (",u8" if name != "i420" else ""))
            gots = [("wrapper", got.cpu().numpy())]
            if (chroma, layout) == ("420", "planar"):
                tabs = [x for T in (Ty, Tx) for x in _dev_taps(T, dev)]
                ptrs = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in tabs]
                out = torch.zeros_like(got)
                if depth == 8:
                    L.check(L.lib().fsr_resample_image(td.data_ptr(), 2, h, w, oh, ow, *ptrs, L.OUT_I420, ops.yuv_matrix_code(matrix), int(full),
                                                       out.data_ptr(), ops._stream()), "fsr_resample_image")
                else:
                    L.check(L.lib().fsr_resample_image_i420_deep(td.data_ptr(), 2, h, w, oh, ow, *ptrs, ops.yuv_matrix_code(matrix), int(full), depth,
                                                                 out.data_ptr(), ops._stream()), "fsr_resample_image_i420_deep")
                _kernel_is(name, kxs, ",u16" if depth != 8 else "")
                gots.append(("C entry point", out.cpu().numpy()))
            for via, g in gots:
                assert g.shape == want.shape == (2, ops.yuv_frame_bytes(oh, ow, chroma, depth, layout))
                for pname, gp, wp in zip(("Y", "Cb or CbCr", "Cr"), _planes(g, 2, oh, ow, chroma, depth, layout),
                                         _planes(want, 2, oh, ow, chroma, depth, layout)):
                    exact("%s %s depth %d %s %s: plane %s (%s)" % (chroma, layout, depth, matrix, "full" if full else "limited", pname, via),
                          gp, wp, th if pname == "Y" or chroma != "420" else th // 2)


def _rs_contract_case(hw, size):
    """(t, float64 reference 2 v - 1, the cap's scale, the float32 restatement), all NHWC, for the real tables."""
    t, v, mag, Ty, Tx = _rs_case(hw, size, False)
    c32 = (t + F32(1)) / F32(2)
    return t, 2 * v - 1, 2 * mag + 1, F32(2) * _apply32(_apply32(c32, Tx, 2), Ty, 1) - F32(1), Ty, Tx


@pytest.mark.parametrize("backend,hw,size,th,kxs", _cases(both=RS_CONTRACT), ids=_rs_id)
def test_resample_contract_taps_against_float64(backend, hw, size, th, kxs):
    """The real tables on random t: the float kind per element within K 2^-23 (2 sum |wy| |wx| |c| + 1) of float64."""
    dev = _select(backend)
    t, ref, scale_, _, _, _ = _rs_contract_case(hw, size)
    got = ops.resample_image(torch.from_numpy(t.copy()).to(dev), *size, kind="f32")
    _kernel_is("f32", kxs)
    gate("resample_f32.%dx%d-%dx%d" % (hw + size), "f32 output", got.cpu().numpy(), _nchw(ref), _nchw(scale_), K_RESAMPLE)


HOSTILE = ("negative xmin", "xsize beyond kx", "xmin beyond w", "ymin + ysize beyond h", "negative ymin", "ymin beyond h", "negative counts")


@pytest.mark.parametrize("kind", ("f32", "u8", "i420", "422", "444"))
@pytest.mark.parametrize("what", HOSTILE)
def test_resample_hostile_tables_stay_inside_the_tensors(what, kind):
    """Emulator only.  Tables that are not the contract's give wrong pixels, never an access outside the tensors: the call
    returns 0, the sentinels around the output are intact, and every output is finite although the input lies between NaNs."""
    dev = _select("emu")
    (h, w), (oh, ow) = (60, 90), (40, 130)
    Ty, Tx = _taps(h, oh), _taps(w, ow)
    ymin, ysize, xmin, xsize = (a.copy() for a in (Ty.xmin, Ty.xsize, Tx.xmin, Tx.xsize))
    if what == "negative xmin":
        xmin -= 7
    elif what == "xsize beyond kx":
        xsize += Tx.kmax + 3
    elif what == "xmin beyond w":
        xmin[1::2] += w
    elif what == "ymin + ysize beyond h":
        ymin += 3
        ysize += 2
    elif what == "negative ymin":
        ymin -= 9
    elif what == "ymin beyond h":
        ymin[5::3] += h
    else:
        xsize[::2], ysize[::3] = -2, -1
    t_all = torch.full((2 * h * w * 3 + 2 * 4096,), float("nan"))
    t = t_all[4096:4096 + 2 * h * w * 3]
    t.copy_(torch.from_numpy(_rs_case((60, 44), (40, 66))[0].copy()).flatten().repeat(4)[:t.numel()])
    if kind in ("f32", "u8"):
        count, dtype, sentinel = 2 * oh * ow * 3, (torch.float32 if kind == "f32" else torch.uint8), 77
    else:
        chroma = "420" if kind == "i420" else kind
        count, dtype, sentinel = 2 * ops.yuv_frame_bytes(oh, ow, chroma, 10), torch.uint8, 0xA5
    pad = 8192
    buf = torch.full((count + 2 * pad,), sentinel, dtype=dtype)
    out = buf[pad:pad + count]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))   # noqa: E731
    keep = [torch.from_numpy(Ty.w.copy()), i32(ymin), i32(ysize), torch.from_numpy(Tx.w.copy()), i32(xmin), i32(xsize)]
    tabs = (keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), Ty.kmax, keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), Tx.kmax)
    if kind in ("f32", "u8"):
        rc = L.lib().fsr_resample_image(t.data_ptr(), 2, h, w, oh, ow, *tabs, ops.RESAMPLE_KINDS[kind], 0, 0, out.data_ptr(), ops._stream())
    else:
        rc = L.lib().fsr_resample_image_yuv(t.data_ptr(), 2, h, w, oh, ow, *tabs, ops.CHROMAS[chroma], 0, 0, 10, out.data_ptr(), ops._stream())
    assert rc == 0, L.lib().fsr_last_error()
    assert bool((buf[:pad] == sentinel).all()) and bool((buf[pad + count:] == sentinel).all()), "a store outside the output"
    if kind == "f32":
        assert bool(torch.isfinite(out).all()), "a NaN from outside the input reached the output"
    elif kind != "u8":
        codes = out.numpy().view("<u2")
        assert int(codes.max()) <= 1023        # (a NaN would have passed the clamp as any code; 10-bit codes stay 10-bit)


# ------------------------------------------------------------------------------------------------- 3. fsr_ssim_sse
SSIM_SHAPES = [(11, 11),     # one window
               (12, 43),     # vw = 33: a 2 x 1 tile next to a 2 x 32 one
               (42, 42),     # vh = vw = 32: exactly one tile, which owns all 42 rows and columns for the squared error
               (43, 43),     # vh = vw = 33: a full tile, a 32 x 1, a 1 x 32 and a one-pixel tile
               (75, 12),     # three tile rows
               (74, 76)]     # 2 x 3 tiles of 32 x 32 .. 32 x 2
SSIM_LAYOUTS = ("nhwc+nchw", "cropped")


def gauss_taps32():
    """The kernel's window: g[k] = expf(-(d * d) / 2) / sum, d = (k - 5) / 1.5f, in float32, summed in order (expf correctly rounded)."""
    d = (np.arange(11) - 5).astype(F32) / F32(1.5)
    g = np.exp((-(d * d) / F32(2)).astype(F64)).astype(F32)
    s = F32(0)
    for v in g:
        s = F32(s + v)
    return g / s


def _tiles(h, w):
    vh, vw = h - 2 * PADW, w - 2 * PADW
    return (vh + TILE - 1) // TILE, (vw + TILE - 1) // TILE


def _blur(x, g, axis):
    """Valid 11-tap correlation along `axis`, accumulated in order in x's dtype."""
    n = x.shape[axis] - 10
    acc = np.zeros_like(np.take(x, range(n), axis))
    for k in range(11):
        acc = acc + g[k] * np.take(x, range(k, k + n), axis)
    return acc


def ssim_map(a, b, ft):
    """The kernel's documented formula on (n, 3, h, w) inputs in [-1, 1], evaluated in `ft` with the float32 taps: the map over the
    (h - 10) x (w - 10) windows inside the image and, in float64, the cap's per-pixel scale s_i."""
    g = gauss_taps32().astype(ft)
    c1, c2 = ft(F32(0.01) * F32(0.01)), ft(F32(0.03) * F32(0.03))
    va, vb = (ft(1) + a.astype(ft)) * ft(0.5), (ft(1) + b.astype(ft)) * ft(0.5)
    m = [_blur(_blur(x, g, 3), g, 2) for x in (va, vb, va * va, vb * vb, va * vb)]
    mu_aa, mu_bb, mu_ab = m[0] * m[0], m[1] * m[1], m[0] * m[1]
    var_a, var_b, cov = np.maximum(m[2] - mu_aa, ft(0)), np.maximum(m[3] - mu_bb, ft(0)), m[4] - mu_ab
    n1, d1, d2 = ft(2) * mu_ab + c1, mu_aa + mu_bb + c1, var_a + var_b + c2
    ssim = (n1 * (ft(2) * cov + c2)) / (d1 * d2)
    if ft is F32:
        return ssim, None
    e = m[2] + m[3] + 2 * np.abs(m[4]) + mu_aa + mu_bb + 2 * np.abs(mu_ab)
    return ssim, np.abs(ssim) + np.abs(n1) * e / (d1 * d2) + np.abs(ssim) * e / d2


def _per_tile(x, h, w):
    """(n, 3, vh, vw) -> (n, 3, tiles) sums over the 32 x 32 tiles of the map, row-major."""
    ty, tx = _tiles(h, w)
    return np.stack([x[:, :, r * TILE:(r + 1) * TILE, c * TILE:(c + 1) * TILE].sum((2, 3)) for r in range(ty) for c in range(tx)], -1)


def _sse_per_tile(d2, h, w):
    """(n, 3, h, w) squared errors -> (n, 3, tiles): a tile owns its 32 x 32 block, the last tile row and column the rest as well."""
    ty, tx = _tiles(h, w)
    ys = [(r * TILE, h if r == ty - 1 else (r + 1) * TILE) for r in range(ty)]
    xs = [(c * TILE, w if c == tx - 1 else (c + 1) * TILE) for c in range(tx)]
    return np.stack([d2[:, :, y0:y1, x0:x1].sum((2, 3)) for y0, y1 in ys for x0, x1 in xs], -1)


def ssim_caps(ssim, s, h, w, K):
    """(per-tile reference sums, per-tile caps, per-image reference, per-image cap) of a float64 map and its scale."""
    ones = np.ones_like(ssim)
    terms = _per_tile(ones, h, w)
    ref, cap = _per_tile(ssim, h, w), K * U * _per_tile(s, h, w) + (terms + 8) * 2.0 ** -24 * _per_tile(np.abs(ssim), h, w)
    iterms = 3 * (h - 10) * (w - 10)
    return ref, cap, ssim.sum((1, 2, 3)), K * U * s.sum((1, 2, 3)) + (iterms + 8) * 2.0 ** -24 * np.abs(ssim).sum((1, 2, 3))


def _layout(x, kind, which, dev):
    """x: (n, 3, h, w) float32 numpy -> a device view of the same values with the strides of the case."""
    n, _, h, w = x.shape
    t = torch.from_numpy(np.array(x)).to(dev)
    if kind == "nhwc+nchw":
        if which == "b":
            return t
        v = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert v.stride() == (h * w * 3, 1, w * 3, 3)
        return v
    big = torch.full((n, 3, h, w + 7), float("nan"), dtype=torch.float32, device=dev)
    off = 3 if which == "a" else 4
    big[:, :, :, off:off + w] = t
    v = big[:, :, :, off:off + w]
    assert v.stride(2) == w + 7
    return v


def _ssim_call(dev, a, b, check=True, over=()):
    """fsr_ssim_sse on caller-owned scratch: (rc, out (n, 2), partials (n, 3, tiles, 2))."""
    n, _, h, w = a.shape
    lib = L.lib()
    tiles = max(_tiles(h, w)[0] * _tiles(h, w)[1], 1)
    nbytes = lib.fsr_ssim_sse_scratch(n, h, w)
    assert nbytes == (n * 3 * tiles * 2 * 4 if min(h, w) > 10 and n > 0 else 0)
    scr = torch.full((max(n, 1) * 3 * tiles * 2,), float("nan"), dtype=torch.float32, device=dev)
    out = torch.full((max(n, 1), 2), float("nan"), dtype=torch.float32, device=dev)
    p = dict(a=a.data_ptr(), b=b.data_ptr(), n=n, h=h, w=w, out=out.data_ptr(), scratch=scr.data_ptr())
    p.update(dict(over))
    rc = lib.fsr_ssim_sse(p["a"], *a.stride(), p["b"], *b.stride(), p["n"], p["h"], p["w"], p["out"], p["scratch"], ops._stream())
    if check:
        L.check(rc, "fsr_ssim_sse")
    return rc, out.cpu().numpy().astype(F64), scr.cpu().numpy().astype(F64).reshape(max(n, 1), 3, tiles, 2)


@functools.lru_cache(maxsize=None)
def _ssim_inputs(h, w, kind):
    """kind "grid": both images in steps of 1/16 in [-1, 1];  "contrast": b uniform, a = clip(b + 0.2 randn);  "smooth": a smooth
    pair with small noise."""
    rng = np.random.default_rng(31 * h + w)
    if kind == "grid":
        a, b = (rng.integers(-16, 17, size=(2, 3, h, w)).astype(F32) / F32(16) for _ in range(2))
    elif kind == "contrast":
        b = (rng.random((2, 3, h, w)) * 2 - 1).astype(F32)
        a = np.clip(b + F32(0.2) * rng.standard_normal((2, 3, h, w)).astype(F32), -1, 1).astype(F32)
    else:
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        base = 0.6 * np.sin(0.11 * yy + 0.3)[None, None] * np.cos(0.07 * xx + np.arange(3)[None, :, None, None] + np.arange(2)[:, None, None, None])
        b = base.astype(F32)
        a = np.clip(b + F32(0.01) * rng.standard_normal((2, 3, h, w)).astype(F32), -1, 1).astype(F32)
    for x in (a, b):
        x.setflags(write=False)
    return a, b


@pytest.mark.parametrize("layout", SSIM_LAYOUTS)
@pytest.mark.parametrize("backend,h,w", _cases(both=SSIM_SHAPES))
def test_ssim_sse_squared_error_is_exact_per_tile(backend, h, w, layout):
    """Inputs in steps of 1/16: every tile's squared-error partial equals the float64 sum over the pixels the tile owns, and the
    per-image result the whole sum.  a and b with different strides; then both as column-cropped views of wider tensors."""
    dev = _select(backend)
    a, b = _ssim_inputs(h, w, "grid")
    d2 = ((1 + a.astype(F64)) / 2 - (1 + b.astype(F64)) / 2) ** 2
    premise("sse.%dx%d" % (h, w), d2, d2.sum((1, 2, 3)), 2.0 ** -10)
    _, out, part = _ssim_call(dev, _layout(a, layout, "a", dev), _layout(b, layout, "b", dev))
    exact("squared error per tile", part[..., 1], _sse_per_tile(d2, h, w))
    exact("squared error per image", out[:, 1], d2.sum((1, 2, 3)))
    assert np.isfinite(part).all()


@pytest.mark.parametrize("kind", ("contrast", "smooth"))
@pytest.mark.parametrize("backend,h,w", _cases(both=SSIM_SHAPES))
def test_ssim_sse_tile_sums_against_float64(backend, h, w, kind):
    """The SSIM partial of every tile, and the per-image sum, within the cap of the float64 evaluation of the formula; the squared
    error within the sum bound."""
    dev = _select(backend)
    a, b = _ssim_inputs(h, w, kind)
    ssim, s = ssim_map(a, b, F64)
    ref, cap, iref, icap = ssim_caps(ssim, s, h, w, K_SSIM)
    _, out, part = _ssim_call(dev, _layout(a, "nhwc+nchw", "a", dev), _layout(b, "nhwc+nchw", "b", dev))
    ratio, iratio = np.abs(part[..., 0] - ref) / cap, np.abs(out[:, 0] - iref) / icap
    print("ssim %dx%d %s: per tile %.3g of the cap, per image %.3g" % (h, w, kind, ratio.max(), iratio.max()))
    _note("ssim_tile.%dx%d.%s" % (h, w, kind), float(ratio.max()))
    _note("ssim_image.%dx%d.%s" % (h, w, kind), float(iratio.max()))
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert ratio.max() <= 1, "tile (image, channel, tile) %s: got %.9g, want %.9g, cap %.3g (%.3g x)" % (i, part[..., 0][i], ref[i], cap[i], ratio[i])
    assert iratio.max() <= 1, (out[:, 0], iref, icap)
    d2 = ((1 + a.astype(F64)) / 2 - (1 + b.astype(F64)) / 2) ** 2
    # the sum bound, plus the roundings of 1 + x (2^-25 of either value after the halving, so 2^-24 of d and 2 |d| 2^-24 of d^2) and of d, d * d
    sse_cap = (3 * h * w + 8) * 2.0 ** -24 * d2.sum((1, 2, 3)) + U * np.sqrt(d2).sum((1, 2, 3)) + 4 * 2.0 ** -24 * d2.sum((1, 2, 3))
    assert (np.abs(out[:, 1] - d2.sum((1, 2, 3))) <= sse_cap).all(), (out[:, 1], d2.sum((1, 2, 3)))


@pytest.mark.parametrize("backend,h,w", _cases(both=SSIM_SHAPES))
def test_ssim_sse_of_identical_images(backend, h, w):
    """a == b: every tile's SSIM partial is within the cap of its pixel count, and every squared error is exactly 0."""
    dev = _select(backend)
    _, b = _ssim_inputs(h, w, "contrast")
    ssim, s = ssim_map(b, b, F64)
    ref, cap, iref, icap = ssim_caps(ssim, s, h, w, K_SSIM)
    count = _per_tile(np.ones_like(ssim), h, w)
    assert np.abs(ref - count).max() <= 1e-9 * count.max()
    _, out, part = _ssim_call(dev, _layout(b, "nhwc+nchw", "a", dev), _layout(b, "nhwc+nchw", "b", dev))
    ratio = np.abs(part[..., 0] - count) / cap
    _note("ssim_tile.%dx%d.identical" % (h, w), float(ratio.max()))
    assert ratio.max() <= 1, (part[..., 0], count, cap)
    assert (np.abs(out[:, 0] - 3 * (h - 10) * (w - 10)) <= icap).all()
    assert (part[..., 1] == 0).all() and (out[:, 1] == 0).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_ssim_sse_refusals(backend):
    dev = _select(backend)
    x = torch.zeros((2, 3, 12, 12), dtype=torch.float32, device=dev)
    for over, word in ((dict(h=10), b"larger than the 11x11 window"), (dict(w=10), b"larger than the 11x11 window"), (dict(h=3), b"larger than"),
                       (dict(w=0), b"larger than"), (dict(n=0), b"empty batch"), (dict(a=None), b"null"), (dict(b=None), b"null"),
                       (dict(out=None), b"null"), (dict(scratch=None), b"null")):
        rc, out, part = _ssim_call(dev, x, x, check=False, over=over)
        assert rc < 0 and word in L.lib().fsr_last_error(), (over, rc, L.lib().fsr_last_error())
        assert np.isnan(out).all() and np.isnan(part).all(), over
    assert L.lib().fsr_ssim_sse_scratch(2, 10, 40) == 0 and L.lib().fsr_ssim_sse_scratch(0, 40, 40) == 0


# ------------------------------------------------------------------------------------------------- K, and the sharpness of the gates
def _k_for(units):
    """The smallest power of two K >= 1 with units <= K / 3."""
    k = 1
    while units > k / 3:
        k *= 2
    return k


def test_float32_restatements_are_inside_a_third_of_the_caps():
    """No kernel is launched.  The float32 numpy restatement of each kernel, on the inputs of the contract cases, stays inside a
    third of the cap with the file's K, and K is the smallest power of two for which it does."""
    worst = 0.0
    for hr, scale, n in CROP_CONTRACT:
        _, ref, scale_, r32 = _crop_contract_case(hr, scale, n)
        worst = max(worst, float((np.abs(r32.astype(F64) - ref) / (U * scale_)).max()))
    crop, worst = worst, 0.0
    for hw, size, _, _ in RS_CONTRACT:
        _, ref, scale_, r32, _, _ = _rs_contract_case(hw, size)
        worst = max(worst, float((np.abs(r32.astype(F64) - ref) / (U * scale_)).max()))
    print("restatements: crop %.3g, resample %.3g units of 2^-23 s" % (crop, worst))
    worst_tile = worst_image = worst_pixel = 0.0
    for h, w in SSIM_SHAPES:
        for kind in ("contrast", "smooth"):
            a, b = _ssim_inputs(h, w, kind)
            ssim, s = ssim_map(a, b, F64)
            m32 = ssim_map(a, b, F32)[0]
            ref, cap, iref, icap = ssim_caps(ssim, s, h, w, 1)
            t32 = _per_tile(m32, h, w).astype(F64)                      # float32 sums of the float32 map
            worst_tile = max(worst_tile, float((np.abs(t32 - ref) / cap).max()))
            worst_image = max(worst_image, float((np.abs(m32.sum((1, 2, 3), dtype=F32).astype(F64) - iref) / icap).max()))
            worst_pixel = max(worst_pixel, float((np.abs(m32.astype(F64) - ssim) / (U * s)).max()))
    print("ssim restatement: per tile %.3g, per image %.3g of the K = 1 cap; per pixel %.3g of 2^-23 s_i" % (worst_tile, worst_image, worst_pixel))
    assert (_k_for(crop), _k_for(worst), _k_for(max(worst_tile, worst_image))) == (K_CROP, K_RESAMPLE, K_SSIM), (crop, worst, worst_tile, worst_image)
    assert worst_pixel <= 1


def test_image_gates_are_sharper_than_the_tolerance_gates():
    """No kernel is launched.  Three planted one-element errors that the older gates pass and the gates of this file reject: a
    resampled float element off by 1e-5 (test_resize.py: 2e-5), a crop lr element off by 5e-6 (test_trainer.py: 1e-5), one pixel of
    the SSIM map off by 1 % at test_ops.py's 45 x 64 shape (per-image mean within 2e-5)."""
    hw, size = RS_SHAPES[0][:2]
    _, v, _, _, _ = _rs_case(hw, size)
    ref = _nchw((2 * v - 1).astype(F32))
    bad = ref.copy()
    bad[1, 2, 33, 64] += F32(1e-5)
    assert np.abs(bad.astype(F64) - ref).max() < 2e-5                      # the old gate passes it
    with pytest.raises(AssertionError, match="1 of"):
        exact("planted", bad, ref, 32)
    exact("unplanted", ref.copy(), ref, 32)
    _, ref64, scale_, r32, _, _ = _rs_contract_case(hw, size)
    bad = r32.copy()
    bad[1, 33, 64, 2] += F32(1e-5)
    assert np.abs(bad.astype(F64) - ref64).max() < 2e-5
    with pytest.raises(AssertionError, match="over the cap"):
        gate(None, "planted", bad, ref64, scale_, K_RESAMPLE)

    _, _, x = _crop_batch(48, 3)
    T = _taps(48, 12)
    ref = _to_pm1(np.einsum("oy,ncyx->ncox", T.M, x.astype(F64) @ T.M.T))
    bad = ref.copy()
    bad[2, 1, 11, 0] += F32(5e-6)
    assert np.abs(bad.astype(F64) - ref).max() < 1e-5
    with pytest.raises(AssertionError, match="1 of"):
        exact("planted", bad, ref)
    _, ref64, scale_, r32 = _crop_contract_case(48, 4, 3)
    bad = r32.copy()
    bad[2, 1, 11, 0] += F32(5e-6)
    assert np.abs(bad.astype(F64) - ref64).max() < 1e-5
    with pytest.raises(AssertionError, match="over the cap"):
        gate(None, "planted", bad, ref64, scale_, K_CROP)

    torch.manual_seed(21)                                                   # the inputs of test_ops.py's (1, 45, 64) case
    h, w = 45, 64
    b = torch.rand(1, 3, h, w) * 2 - 1
    a = (b + 0.2 * torch.randn(1, 3, h, w)).clamp(-1, 1)
    ssim, s = ssim_map(a.numpy(), b.numpy(), F64)
    ref, cap, _, _ = ssim_caps(ssim, s, h, w, K_SSIM)
    per_image = 3 * (h - 10) * (w - 10)
    for (y, x_), caught in (((34, 53), True), ((33, 5), True), ((17, 9), False)):   # the 3 x 22 corner tile, the 3 x 32 tile, a full tile
        bad = ssim.copy()
        bad[0, 1, y, x_] *= 1.01
        assert abs(bad.sum() - ssim.sum()) / per_image < 2e-5 / 6           # the old gate passes it, six times over
        over = np.abs(_per_tile(bad, h, w) - ref) / cap
        print("1 %% of the SSIM map at (%d, %d): %.3g caps" % (y, x_, over.max()))
        if caught:
            assert (over > 1).sum() == 1, over
