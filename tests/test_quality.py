"""fsr_quality_u8 (metrics.hip): the benchmark protocol -- luma or RGB of uint8 frames, a shaved border, Wang's SSIM at data range
255 and the squared error behind PSNR -- per tile and per image, bit-exact where the arithmetic allows it and against float64
where it does not.  The kernel is fsr_ssim_sse's body with a byte loader, so the file follows test_image_exact.py's third part.

Cases: regions (eh x ew) of 11 x 11 (one window), 12 x 43 (a 2 x 1 tile beside a 2 x 32 one), 42 x 42 (exactly one tile), 43 x 43
(a tile plus one pixel each way), 75 x 12 (three tile rows) and 74 x 76 (2 x 3 tiles, partial last ones); each with shave 0, 1
and 4, so the images are region + 2 shave wide and high: the region's first byte lies 3 shave past a row start (off and on a
dword boundary) and 3 w is a multiple of 4 for none of the odd widths.  n = 2.  a is contiguous; b is contiguous ("plain") or
the [1:h+1, 2:w+2] slice of a buffer 2 rows taller and 3 columns wider that holds other bytes ("slice": other row and image
strides, another byte alignment per row).

  * squared error, RGB, exact: |a - b| <= 15, so every term and every sum is an integer below 2^24 (asserted on the reference
    first: a premise failure is a bug of the input generator).  Every tile partial, read back from caller-owned scratch, and
    every per-image sum equals the integer sum.  A tile owns its 32 x 32 block, the last tile row and column the region's last
    10 rows and columns as well.
  * Y coefficients, analytic: a grey, b = a + d grey (d = 1, 7): the three float32 coefficients sum to 219 / 255, so the squared
    error per image is count (219 d / 255)^2 within
        (count + 8) 2^-24 T  +  count (2 dy e + e^2),   dy = 219 d / 255,  e = 2 (4 2^-24 235) + 2^-23 dy
    (fixed-order float32 summation of count positive terms; each luma value carries at most 4 2^-24 relative error of at most
    235 -- three rounded coefficients, a product, two fused multiply-adds and the sum with 16, all terms positive -- and the
    difference one more rounding).
  * SSIM, both channels, and the Y-mode squared error against float64: the reference evaluates the documented formula in numpy
    float64 from the float32 taps and the float32 luma constants, per tile and per image, on "contrast" (b uniform bytes, a = b
    plus noise of sigma 25 codes) and "smooth" (a smooth pair, noise of sigma 1.3 codes) pairs.  The cap is test_image_exact.py's:
        |tile sum - ref64| <= K 2^-23 sum_i s_i + (terms + 8) 2^-24 sum_i |ssim_i|
        s_i = |ssim_i| + |N1| E / (D1 D2) + |ssim_i| E / D2,   E = E[aa] + E[bb] + 2 |E[ab]| + mu_aa + mu_bb + 2 |mu_ab|
    in 255 units throughout (c1, c2 scale with the data, so s_i does not change its meaning); the luma conversion perturbs each
    input by at most 4 2^-24 relative, a perturbation of the moments that E already scales.  K is the smallest power of two for
    which the float32 numpy restatement of the kernel's statements stays inside ONE THIRD of the cap on these very inputs
    (test_float32_restatement_is_inside_a_third_of_the_cap asserts the bound and the minimality); the rest is the room for fused
    multiply-adds and another association on the device.  The Y-mode squared error is held to the sum bound with the same
    per-value error e as above: (count + 8) 2^-24 S + sum_i (2 |d_i| e_i + e_i^2), e_i = 2 (4 2^-24 235) + 2^-23 |d_i|.
  * identical images: squared error exactly 0, SSIM sums within the cap of the window count.
  * locality: results and partials are bit-identical when the shaved border and the bytes of the wider buffer outside the slice
    are re-randomised, and from run to run.
  * refusals: rc < 0, the message names the argument, out and scratch keep their poison.

Largest share of the cap (K = 1), over all cases, both channels and both kinds:

    quantity               restatement   emulator   MI355X
    ssim per tile          0.232         0.232      0.0843
    ssim per image         0.0349        0.0349     0.0349
    identical, per tile    --            0          0.00745

(The emulator does not contract and reproduces the restatement to the digit; the MI355X fuses, which here comes out closer to
float64.)  The restatement follows the kernel's statements, which evaluate the documented formula on x - 128 and restore its
moments exactly (metrics.hip, U8Loader): taken literally in float32 code units, var = E[xx] - E[x]^2 cancels five digits and the
restatement sat at 0.173 / 0.159 of the same cap, 4e-6 relative on a whole image's SSIM.  Every figure goes to the
parity-error log through backend.report as quality.<backend>.<key>, when it exceeds the previous maximum.
"""
import functools

import numpy as np
import pytest
import torch

from backend import BACKENDS, L, ops, report, select

F32, F64 = np.float32, np.float64
U = 2.0 ** -23
TILE, PADW = 32, 5                            # metrics.hip
K_QUALITY = 1
REGIONS = [(11, 11), (12, 43), (42, 42), (43, 43), (75, 12), (74, 76)]
SHAVES = (0, 1, 4)
LAYOUTS = ("plain", "slice")
CHANNELS = (("y", L.QUALITY_Y, 1), ("rgb", L.QUALITY_RGB, 3))
CASES = [(eh, ew, s, lay) for eh, ew in REGIONS for s in SHAVES for lay in LAYOUTS]
N = 2

_worst, _backend = {}, ["-"]


def _select(backend):
    _backend[0] = backend
    return select(backend)


def _note(key, value, backend=None):
    key = "quality.%s.%s" % (backend or _backend[0], key)
    if value > _worst.get(key, -1.0):
        _worst[key] = value
        report(key, value)


# ------------------------------------------------------------------------------------------------- the reference
def gauss_taps32():
    """The kernel's window: g[k] = expf(-(d * d) / 2) / sum, d = (k - 5) / 1.5f, in float32, summed in order."""
    d = (np.arange(11) - 5).astype(F32) / F32(1.5)
    g = np.exp((-(d * d) / F32(2)).astype(F64)).astype(F32)
    s = F32(0)
    for v in g:
        s = F32(s + v)
    return g / s


Y_COEF = tuple(F32(c / 255.0) for c in (65.481, 128.553, 24.966))


def values(x, channel, ft):
    """(n, eh, ew, 3) uint8 region -> (n, C, eh, ew) in `ft`, in the kernel's order of operations."""
    x = x.astype(ft)
    if channel == "rgb":
        return np.ascontiguousarray(np.moveaxis(x, 3, 1))
    kr, kg, kb = (ft(c) for c in Y_COEF)
    return (ft(16) + ((kr * x[..., 0] + kg * x[..., 1]) + kb * x[..., 2]))[:, None]


def _blur(x, g, axis):
    n = x.shape[axis] - 10
    acc = np.zeros_like(np.take(x, range(n), axis))
    for k in range(11):
        acc = acc + g[k] * np.take(x, range(k, k + n), axis)
    return acc


def shifted_values(x, channel):
    """The float32 values the kernel's windows take: x - 128 (luma: -112 + t, one rounding)."""
    x = x.astype(F32)
    if channel == "rgb":
        return np.ascontiguousarray(np.moveaxis(x, 3, 1)) - F32(128)
    kr, kg, kb = Y_COEF

    def fma(a, b, c):        # float32 fused multiply-add: byte x coefficient plus a float32 of the same range is exact in float64
        return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)

    t = fma(np.full_like(x[..., 2], kb), x[..., 2], fma(np.full_like(x[..., 1], kg), x[..., 1], kr * x[..., 0]))
    return (F32(16 - 128) + t)[:, None]


def ssim_map_restated(sa, sb):
    """The kernel's statements in float32 numpy on the shifted values: the moments of x' = x - 128, then the documented formula's
    moments of x restored with G = the sum of the 11 x 11 float32 window, eps = 1 - G (metrics.hip, U8Loader)."""
    g = gauss_taps32()
    G = float(g.astype(F64).sum()) ** 2
    shift_mean, eps, shift_var = F32(128 * G), F32(1 - G), F32(128 * 128 * G)
    k1, k2 = F32(0.01) * F32(255), F32(0.03) * F32(255)
    c1, c2 = F32(k1 * k1), F32(k2 * k2)
    m = [_blur(_blur(x, g, 3), g, 2) for x in (sa, sb, sa * sa, sb * sb, sa * sb)]
    var_a = (m[2] - m[0] * m[0]) + eps * (F32(256) * m[0] + shift_var)
    var_b = (m[3] - m[1] * m[1]) + eps * (F32(256) * m[1] + shift_var)
    cov = (m[4] - m[0] * m[1]) + eps * (F32(128) * (m[0] + m[1]) + shift_var)
    fa, fb = m[0] + shift_mean, m[1] + shift_mean
    mu_aa, mu_bb, mu_ab = fa * fa, fb * fb, fa * fb
    var_a, var_b = np.maximum(var_a, F32(0)), np.maximum(var_b, F32(0))
    out = ((F32(2) * mu_ab + c1) * (F32(2) * cov + c2)) / ((mu_aa + mu_bb + c1) * (var_a + var_b + c2))
    assert out.dtype == F32
    return out


def ssim_map(va, vb, ft):
    """The documented formula on (n, C, eh, ew) values in 255 units, in `ft` with the float32 taps; in float64 also the cap's s_i."""
    g = gauss_taps32().astype(ft)
    k1, k2 = F32(0.01) * F32(255), F32(0.03) * F32(255)
    c1, c2 = ft(F32(k1 * k1)), ft(F32(k2 * k2))
    m = [_blur(_blur(x, g, 3), g, 2) for x in (va, vb, va * va, vb * vb, va * vb)]
    mu_aa, mu_bb, mu_ab = m[0] * m[0], m[1] * m[1], m[0] * m[1]
    var_a, var_b, cov = np.maximum(m[2] - mu_aa, ft(0)), np.maximum(m[3] - mu_bb, ft(0)), m[4] - mu_ab
    n1, d1, d2 = ft(2) * mu_ab + c1, mu_aa + mu_bb + c1, var_a + var_b + c2
    ssim = (n1 * (ft(2) * cov + c2)) / (d1 * d2)
    if ft is F32:
        return ssim, None
    e = m[2] + m[3] + 2 * np.abs(m[4]) + mu_aa + mu_bb + 2 * np.abs(mu_ab)
    return ssim, np.abs(ssim) + np.abs(n1) * e / (d1 * d2) + np.abs(ssim) * e / d2


def _tiles(eh, ew):
    return (eh - 2 * PADW + TILE - 1) // TILE, (ew - 2 * PADW + TILE - 1) // TILE


def _per_tile(x, eh, ew):
    """(n, C, vh, vw) -> (n, C, tiles) sums over the 32 x 32 tiles of the map, row-major."""
    ty, tx = _tiles(eh, ew)
    return np.stack([x[:, :, r * TILE:(r + 1) * TILE, c * TILE:(c + 1) * TILE].sum((2, 3)) for r in range(ty) for c in range(tx)], -1)


def _sse_per_tile(d2, eh, ew):
    """(n, C, eh, ew) squared errors -> (n, C, tiles): a tile owns its 32 x 32 block, the last tile row and column the rest too."""
    ty, tx = _tiles(eh, ew)
    ys = [(r * TILE, eh if r == ty - 1 else (r + 1) * TILE) for r in range(ty)]
    xs = [(c * TILE, ew if c == tx - 1 else (c + 1) * TILE) for c in range(tx)]
    return np.stack([d2[:, :, y0:y1, x0:x1].sum((2, 3)) for y0, y1 in ys for x0, x1 in xs], -1)


def ssim_caps(ssim, s, eh, ew, K):
    """(per-tile reference sums, per-tile caps, per-image reference, per-image cap) of a float64 map and its scale."""
    terms = _per_tile(np.ones_like(ssim), eh, ew)
    ref, cap = _per_tile(ssim, eh, ew), K * U * _per_tile(s, eh, ew) + (terms + 8) * 2.0 ** -24 * _per_tile(np.abs(ssim), eh, ew)
    iterms = ssim.shape[1] * (eh - 10) * (ew - 10)
    return ref, cap, ssim.sum((1, 2, 3)), K * U * s.sum((1, 2, 3)) + (iterms + 8) * 2.0 ** -24 * np.abs(ssim).sum((1, 2, 3))


def luma_sse_cap(d, count):
    """Cap of a float32 squared-error sum of `count` luma differences d (float64, (n, ...)) -- see the module docstring."""
    d = np.abs(d).reshape(d.shape[0], -1)
    e = 2 * (4 * 2.0 ** -24 * 235) + U * d
    return (count + 8) * 2.0 ** -24 * (d * d).sum(1) + (2 * d * e + e * e).sum(1)


# ------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _inputs(eh, ew, shave, kind):
    """Two (N, h, w, 3) uint8 images, h = eh + 2 shave.  "near": |a - b| <= 15;  "contrast": b uniform, a = b + noise of sigma 25;
    "smooth": a smooth pair with noise of sigma 1.3;  "grey1" / "grey7": a grey, b = a + d."""
    h, w = eh + 2 * shave, ew + 2 * shave
    rng = np.random.default_rng(1000 * eh + 10 * ew + shave)
    if kind == "near":
        b = rng.integers(0, 256, size=(N, h, w, 3))
        a = np.clip(b + rng.integers(-15, 16, size=b.shape), 0, 255)
    elif kind == "contrast":
        b = rng.integers(0, 256, size=(N, h, w, 3))
        a = np.clip(np.rint(b + 25.0 * rng.standard_normal(b.shape)), 0, 255)
    elif kind == "smooth":
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        base = 127.5 + 76.0 * np.sin(0.11 * yy + 0.3)[None, :, :, None] * np.cos(0.07 * xx[None, :, :, None] + np.arange(3)[None, None, None, :]
                                                                                  + np.arange(N)[:, None, None, None])
        b = np.rint(base)
        a = np.clip(np.rint(base + 1.3 * rng.standard_normal(base.shape)), 0, 255)
    else:
        d = int(kind[4:])
        g = rng.integers(0, 256 - d, size=(N, h, w, 1))
        a, b = np.repeat(g, 3, 3), np.repeat(g + d, 3, 3)
    a, b = a.astype(np.uint8), b.astype(np.uint8)
    for x in (a, b):
        x.setflags(write=False)
    return a, b


def _region(x, shave):
    n, h, w, _ = x.shape
    return x[:, shave:h - shave, shave:w - shave]


def _place(x, layout, dev, seed=5):
    """x: (n, h, w, 3) uint8 numpy -> (device view with the strides of the layout, the buffer behind it)."""
    n, h, w, _ = x.shape
    if layout == "plain":
        t = torch.from_numpy(np.array(x)).to(dev)
        return t, t
    big = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(n, h + 2, w + 3, 3)).astype(np.uint8)).to(dev)
    big[:, 1:h + 1, 2:w + 2] = torch.from_numpy(np.array(x)).to(dev)
    v = big[:, 1:h + 1, 2:w + 2]
    assert v.stride() == ((h + 2) * (w + 3) * 3, (w + 3) * 3, 3, 1)
    return v, big


def _call(dev, a, b, shave, code, channels, check=True, over=()):
    """fsr_quality_u8 on caller-owned scratch: (rc, out (n, 2), partials (n, C, tiles, 2)) as float64, and the raw float32 bits."""
    n, h, w, _ = a.shape
    lib = L.lib()
    eh, ew = h - 2 * shave, w - 2 * shave
    tiles = _tiles(eh, ew)[0] * _tiles(eh, ew)[1] if min(eh, ew) > 10 else 1
    nbytes = lib.fsr_quality_u8_scratch(n, h, w, shave, code)
    assert nbytes == (n * channels * tiles * 2 * 4 if min(eh, ew) > 10 and shave >= 0 else 0)
    scr = torch.full((n * channels * tiles * 2,), float("nan"), dtype=torch.float32, device=dev)
    out = torch.full((n, 2), float("nan"), dtype=torch.float32, device=dev)
    p = dict(a=a.data_ptr(), a_image=a.stride(0), a_row=a.stride(1), b=b.data_ptr(), b_image=b.stride(0), b_row=b.stride(1),
             n=n, h=h, w=w, shave=shave, channel=code, out=out.data_ptr(), scratch=scr.data_ptr())
    p.update(dict(over))
    rc = lib.fsr_quality_u8(p["a"], p["a_image"], p["a_row"], p["b"], p["b_image"], p["b_row"], p["n"], p["h"], p["w"], p["shave"],
                            p["channel"], p["out"], p["scratch"], ops._stream())
    if check:
        L.check(rc, "fsr_quality_u8")
    o, s = out.cpu().numpy(), scr.cpu().numpy()
    return rc, o.astype(F64), s.astype(F64).reshape(n, channels, tiles, 2), (o.view(np.uint32).copy(), s.view(np.uint32).copy())


def _case_params():
    return [pytest.param("emu", *c) for c in CASES] + [pytest.param("hip", *c, marks=pytest.mark.gpu) for c in CASES]


def exact(what, got, want):
    bad = got != want
    assert not bad.any(), "%s: %d of %d differ, first got %r want %r" % (what, bad.sum(), bad.size, got[bad][0], want[bad][0])


# ------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("backend,eh,ew,shave,layout", _case_params())
def test_rgb_squared_error_is_exact_per_tile(backend, eh, ew, shave, layout):
    dev = _select(backend)
    a, b = _inputs(eh, ew, shave, "near")
    d2 = np.moveaxis((_region(a, shave).astype(F64) - _region(b, shave).astype(F64)) ** 2, 3, 1)
    assert d2.sum((1, 2, 3)).max() < 2 ** 24 and np.abs(a.astype(int) - b.astype(int)).max() <= 15      # the premise
    ta, tb = _place(a, "plain", dev)[0], _place(b, layout, dev)[0]
    _, out, part, _ = _call(dev, ta, tb, shave, L.QUALITY_RGB, 3)
    exact("squared error per tile", part[..., 1], _sse_per_tile(d2, eh, ew))
    exact("squared error per image", out[:, 1], d2.sum((1, 2, 3)))
    assert np.isfinite(part).all() and np.isfinite(out).all()


@pytest.mark.parametrize("backend,eh,ew,shave,layout", _case_params())
def test_luma_coefficients_sum_to_219(backend, eh, ew, shave, layout):
    dev = _select(backend)
    count = eh * ew
    for d in (1, 7):
        a, b = _inputs(eh, ew, shave, "grey%d" % d)
        _, out, _, _ = _call(dev, _place(a, "plain", dev)[0], _place(b, layout, dev)[0], shave, L.QUALITY_Y, 1)
        dy = 219.0 * d / 255.0
        want = count * dy * dy
        cap = luma_sse_cap(np.full((N, count), dy), count)
        print("grey d = %d: %s, want %.9g, cap %.3g" % (d, out[:, 1], want, cap[0]))
        assert (np.abs(out[:, 1] - want) <= cap).all(), (d, out[:, 1], want, cap)


@functools.lru_cache(maxsize=None)
def _reference(eh, ew, shave, kind, channel, same=False):
    a, b = _inputs(eh, ew, shave, kind)
    if same:
        a = b
    va, vb = values(_region(a, shave), channel, F64), values(_region(b, shave), channel, F64)
    ssim, s = ssim_map(va, vb, F64)
    return ssim, s, va - vb


@pytest.mark.parametrize("backend,eh,ew,shave,layout", _case_params())
def test_sums_against_float64(backend, eh, ew, shave, layout):
    """SSIM per tile and per image within the cap, in both channels and on both kinds of pairs; the squared error within the sum
    bound (exactly, in RGB mode, wherever it stays below 2^24)."""
    dev = _select(backend)
    for kind in ("contrast", "smooth"):
        a, b = _inputs(eh, ew, shave, kind)
        ta, tb = _place(a, "plain", dev)[0], _place(b, layout, dev)[0]
        for name, code, C in CHANNELS:
            ssim, s, d = _reference(eh, ew, shave, kind, name)
            ref, cap, iref, icap = ssim_caps(ssim, s, eh, ew, K_QUALITY)
            _, out, part, _ = _call(dev, ta, tb, shave, code, C)
            ratio, iratio = np.abs(part[..., 0] - ref) / cap, np.abs(out[:, 0] - iref) / icap
            print("quality %dx%d shave %d %s %s %s: per tile %.3g of the cap, per image %.3g" % (eh, ew, shave, layout, kind, name, ratio.max(), iratio.max()))
            _note("ssim_tile", float(ratio.max()))
            _note("ssim_image", float(iratio.max()))
            i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            assert ratio.max() <= 1, "tile (image, channel, tile) %s: got %.9g, want %.9g, cap %.3g" % (i, part[..., 0][i], ref[i], cap[i])
            assert iratio.max() <= 1, (out[:, 0], iref, icap)
            d2 = d * d
            count = C * eh * ew
            sse_cap = luma_sse_cap(d, count) if name == "y" else (count + 8) * 2.0 ** -24 * d2.sum((1, 2, 3))
            assert (np.abs(out[:, 1] - d2.sum((1, 2, 3))) <= sse_cap).all(), (name, out[:, 1], d2.sum((1, 2, 3)), sse_cap)
            if name == "y":
                tile_cap = luma_sse_cap(d, count)[:, None, None]       # a tile's share is below the image's
                assert (np.abs(part[..., 1] - _sse_per_tile(d2, eh, ew)) <= tile_cap).all()


@pytest.mark.parametrize("backend,eh,ew,shave,layout", _case_params())
def test_identical_images(backend, eh, ew, shave, layout):
    dev = _select(backend)
    _, b = _inputs(eh, ew, shave, "contrast")
    ta, tb = _place(b, "plain", dev)[0], _place(b, layout, dev)[0]
    for name, code, C in CHANNELS:
        ssim, s, _ = _reference(eh, ew, shave, "contrast", name, True)
        ref, cap, iref, icap = ssim_caps(ssim, s, eh, ew, K_QUALITY)
        count = _per_tile(np.ones_like(ssim), eh, ew)
        assert np.abs(ref - count).max() <= 1e-9 * count.max()
        _, out, part, _ = _call(dev, ta, tb, shave, code, C)
        ratio = np.abs(part[..., 0] - count) / cap
        _note("identical_tile", float(ratio.max()))
        assert ratio.max() <= 1, (part[..., 0], count, cap)
        assert (np.abs(out[:, 0] - C * (eh - 10) * (ew - 10)) <= icap).all()
        assert (part[..., 1] == 0).all() and (out[:, 1] == 0).all()


@pytest.mark.parametrize("backend,eh,ew,shave,layout", _case_params())
def test_nothing_outside_the_region_counts(backend, eh, ew, shave, layout):
    """Bit-identical results when the shaved border of both images and the bytes of the wider buffer outside the slice are
    re-randomised, and from run to run."""
    dev = _select(backend)
    a, b = _inputs(eh, ew, shave, "contrast")
    h, w = a.shape[1:3]
    rng = np.random.default_rng(77)
    a2, b2 = (rng.integers(0, 256, size=a.shape).astype(np.uint8) for _ in range(2))
    _region(a2, shave)[...] = _region(a, shave)
    _region(b2, shave)[...] = _region(b, shave)
    if shave:
        assert (a2 != a).any() and (b2 != b).any()
    for name, code, C in CHANNELS:
        first = _call(dev, _place(a, "plain", dev)[0], _place(b, layout, dev, seed=5)[0], shave, code, C)[3]
        again = _call(dev, _place(a, "plain", dev)[0], _place(b, layout, dev, seed=5)[0], shave, code, C)[3]
        other = _call(dev, _place(a2, "plain", dev)[0], _place(b2, layout, dev, seed=6)[0], shave, code, C)[3]
        for x, y in zip(first, again):
            assert (x == y).all(), "two runs differ"
        for x, y in zip(first, other):
            assert (x == y).all(), "bytes outside the region changed the result"


@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals(backend):
    dev = _select(backend)
    x = torch.zeros((2, 14, 15, 3), dtype=torch.uint8, device=dev)
    for over, word in ((dict(a=None), b"null"), (dict(b=None), b"null"), (dict(out=None), b"null"), (dict(scratch=None), b"null"),
                       (dict(n=0), b"batch n"), (dict(n=-1), b"batch n"), (dict(n=65536), b"batch n"),
                       (dict(channel=2), b"channel"), (dict(channel=-1), b"channel"), (dict(shave=-1), b"shave"),
                       (dict(shave=2), b"region"), (dict(h=10), b"region"), (dict(w=10), b"region"), (dict(w=0), b"region"),
                       (dict(shave=8), b"region"), (dict(a_row=44), b"row_bytes"), (dict(b_row=44), b"row_bytes")):
        rc, out, part = _refused(dev, x, over)
        assert rc < 0 and word in L.lib().fsr_last_error(), (over, rc, L.lib().fsr_last_error())
        assert np.isnan(out).all() and np.isnan(part).all(), over
    q = L.lib().fsr_quality_u8_scratch
    assert q(2, 10, 40, 0, 0) == 0 and q(2, 40, 30, 10, 0) == 0 and q(0, 40, 40, 0, 0) == 0 and q(2, 40, 40, 0, 1) == 3 * q(2, 40, 40, 0, 0) > 0


def _refused(dev, x, over):
    """One refused call on poisoned out / scratch: the valid base call is shave 1 of 14 x 15 (a 12 x 13 region), luma."""
    lib = L.lib()
    n, h, w, _ = x.shape
    scr = torch.full((64,), float("nan"), dtype=torch.float32, device=dev)
    out = torch.full((n, 2), float("nan"), dtype=torch.float32, device=dev)
    p = dict(a=x.data_ptr(), a_image=x.stride(0), a_row=x.stride(1), b=x.data_ptr(), b_image=x.stride(0), b_row=x.stride(1),
             n=n, h=h, w=w, shave=1, channel=L.QUALITY_Y, out=out.data_ptr(), scratch=scr.data_ptr())
    p.update(over)
    rc = lib.fsr_quality_u8(p["a"], p["a_image"], p["a_row"], p["b"], p["b_image"], p["b_row"], p["n"], p["h"], p["w"], p["shave"],
                            p["channel"], p["out"], p["scratch"], ops._stream())
    return rc, out.cpu().numpy(), scr.cpu().numpy()


def _k_for(units):
    """The smallest power of two K >= 1 with units <= K / 3."""
    k = 1
    while units > k / 3:
        k *= 2
    return k


def test_float32_restatement_is_inside_a_third_of_the_cap():
    """No kernel is launched.  The float32 numpy restatement of the kernel's statements, on the inputs of the cases, stays inside a
    third of the cap with the file's K, and K is the smallest power of two for which it does."""
    worst_tile = worst_image = 0.0
    for eh, ew in REGIONS:
        for shave in SHAVES:
            for kind in ("contrast", "smooth"):
                a, b = _inputs(eh, ew, shave, kind)
                for name, _, _ in CHANNELS:
                    ssim, s, _ = _reference(eh, ew, shave, kind, name)
                    m32 = ssim_map_restated(shifted_values(_region(a, shave), name), shifted_values(_region(b, shave), name))
                    ref, cap, iref, icap = ssim_caps(ssim, s, eh, ew, 1)
                    worst_tile = max(worst_tile, float((np.abs(_per_tile(m32, eh, ew).astype(F64) - ref) / cap).max()))
                    worst_image = max(worst_image, float((np.abs(m32.sum((1, 2, 3), dtype=F32).astype(F64) - iref) / icap).max()))
    print("quality restatement: per tile %.3g, per image %.3g of the K = 1 cap" % (worst_tile, worst_image))
    _note("restatement_tile", worst_tile, "numpy")
    _note("restatement_image", worst_image, "numpy")
    assert _k_for(max(worst_tile, worst_image)) == K_QUALITY, (worst_tile, worst_image)


# ------------------------------------------------------------------------------------------------- the operator
@pytest.mark.parametrize("backend", BACKENDS)
def test_operator_reads_slices_in_place(backend):
    """ops.quality_u8 on a [:, :H, :W] slice of larger frames equals the call on a contiguous copy, bit for bit, in both channels;
    its errors are ValueErrors that name the shape."""
    dev = _select(backend)
    rng = np.random.default_rng(3)
    big = torch.from_numpy(rng.integers(0, 256, size=(3, 50, 61, 3)).astype(np.uint8)).to(dev)
    sr = torch.from_numpy(rng.integers(0, 256, size=(3, 48, 60, 3)).astype(np.uint8)).to(dev)
    hr = big[:, :48, :60]
    assert not hr.is_contiguous()
    for channel, C in (("y", 1), ("rgb", 3)):
        r = ops.quality_u8(sr, hr, shave=4, channel=channel)
        assert r.shape == (3, 2) and r.dtype == torch.float32
        assert torch.equal(r, ops.quality_u8(sr, hr.contiguous(), shave=4, channel=channel))
        va, vb = (values(_region(t.cpu().numpy(), 4), channel, F64) for t in (sr, hr))
        want = ((va - vb) ** 2).sum((1, 2, 3))
        assert np.abs(r[:, 1].cpu().numpy() - want).max() <= 1e-5 * want.max()
        ssim = ssim_map(va, vb, F64)[0].sum((1, 2, 3))
        assert np.abs(r[:, 0].cpu().numpy() - ssim).max() <= 1e-4 * C * 30 * 42
    assert torch.equal(ops.quality_u8(sr, sr)[:, 1], torch.zeros(3, device=dev))
    for bad, word in ((lambda: ops.quality_u8(sr, big), "(3, 50, 61, 3)"), (lambda: ops.quality_u8(sr, hr, channel="luma"), "luma"),
                      (lambda: ops.quality_u8(sr, hr, shave=19), "(3, 48, 60, 3)"), (lambda: ops.quality_u8(sr.float(), hr), "float32"),
                      (lambda: ops.quality_u8(sr[:, :, ::2], hr[:, :, ::2]), "(3, 48, 30, 3)"),
                      (lambda: ops.quality_u8(sr.permute(0, 2, 1, 3), hr.permute(0, 2, 1, 3)), "(3, 60, 48, 3)")):
        with pytest.raises(ValueError) as e:
            bad()
        assert word in str(e.value), (word, str(e.value))
