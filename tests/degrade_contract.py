"""Test helper: the degradation contract of DESIGN.md §6g (blur -> noise -> JPEG round trip on NCHW float32 batches in [-1, 1]),
restated in numpy independently of the code under test, and the fixtures test_degrade.py shares.

Blur: isotropic Gaussian, sigma in LR pixels, r = min(ceil(3 sigma), 9), taps exp(-j^2 / 2 sigma^2) normalised in float64 and cast to
float32, horizontal pass then vertical pass, accumulation in tap order j = -r..r, borders by clamping the source index.
Noise: x += z * sigma_n * (2 / 255), z from the stateless hash below (Box-Muller on two 24-bit uniforms).
JPEG: v = clamp((x + 1) 127.5, 0, 255) unrounded, edge-replicated padding to whole MCUs, JFIF colour transform, 2x2 chroma mean
("420"), orthonormal 8x8 DCT-II, k = rint(coef / Q) with libjpeg's quality-scaled Annex K tables, inverse, chroma replication,
inverse colour transform, code = clamp(rint(.), 0, 255), value code / 127.5 - 1, crop."""
import math

import numpy as np

from yuv_contract import assert_codes_close  # noqa: F401  (re-exported for test_degrade.py)

MAX_RADIUS = 9
TAPS = 2 * MAX_RADIUS + 1

LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                  + [99] * 32, dtype=np.int64).reshape(8, 8)


# ------------------------------------------------------------------------------------------------------------ blur
def blur_taps(sigma):
    """(r, float32 taps j = -r..r) of one sample; sigma = 0 is the identity (r = 0, one tap of 1)."""
    if sigma == 0:
        return 0, np.ones(1, dtype=np.float32)
    r = min(int(math.ceil(3.0 * sigma)), MAX_RADIUS)
    j = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(j * j) / (2.0 * float(sigma) ** 2))
    return r, (w / w.sum()).astype(np.float32)


def np_blur(x, sigmas, ft=np.float64):
    """(N,3,h,w) -> the blurred batch computed in `ft` with the float32 taps; a sample with sigma = 0 is returned as it is."""
    x = np.asarray(x)
    out = x.astype(ft).copy()
    n, _, h, w = x.shape
    for i, s in enumerate(sigmas):
        if s == 0:
            continue
        r, taps = blur_taps(s)
        src = x[i].astype(ft)
        xs = np.arange(w)
        acc = np.zeros_like(src)
        for j in range(-r, r + 1):
            acc = acc + ft(taps[j + r]) * src[:, :, np.clip(xs + j, 0, w - 1)]
        ys = np.arange(h)
        acc2 = np.zeros_like(src)
        for j in range(-r, r + 1):
            acc2 = acc2 + ft(taps[j + r]) * acc[:, np.clip(ys + j, 0, h - 1), :]
        out[i] = acc2
    return out


# ----------------------------------------------------------------------------------------------------------- noise
def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def np_z(count, s0, s1, ft=np.float64):
    """z of the elements e = 0..count-1 of a sample with seed words (s0, s1), evaluated in `ft` from the contract's integers."""
    e = np.arange(count, dtype=np.uint64)
    a = mix32(mix32((np.uint64(s0) + 2 * e) & 0xffffffff) ^ np.uint64(s1))
    b = mix32(mix32((np.uint64(s0) + 2 * e + 1) & 0xffffffff) ^ np.uint64(s1))
    u1 = ((a >> 8) + 1).astype(ft) * ft(2.0 ** -24)
    u2 = (b >> 8).astype(ft) * ft(2.0 ** -24)
    return np.sqrt(ft(-2) * np.log(u1)) * np.cos(ft(np.float32(6.2831855)) * u2)


def np_noise(x, sigmas, seeds):
    """(N,3,h,w) float32 -> float64 x + z sigma_n (2 / 255); a sample with sigma_n = 0 is returned as it is."""
    x = np.asarray(x)
    out = x.astype(np.float64).copy()
    for i, (s, (s0, s1)) in enumerate(zip(sigmas, seeds)):
        if s == 0:
            continue
        z = np_z(x[i].size, s0, s1).reshape(x[i].shape)
        out[i] = out[i] + z * (float(s) * (2.0 / 255.0))
    return out


# ------------------------------------------------------------------------------------------------------------ JPEG
def quant_table(base, q):
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base * s + 50) // 100, 1, 255)


def dct_matrix(ft=np.float64):
    c = np.zeros((8, 8), dtype=np.float64)
    for u in range(8):
        for x in range(8):
            c[u, x] = math.sqrt(1.0 / 8.0) if u == 0 else 0.5 * math.cos((2 * x + 1) * u * math.pi / 16.0)
    return c.astype(ft)


def _blocks(p):
    """(H, W) -> (H/8, W/8, 8, 8)"""
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def _unblocks(b):
    nh, nw = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(nh * 8, nw * 8)


def jpeg_planes(x, subsampling="420", ft=np.float64):
    """(3,h,w) in [-1,1] -> the padded planes (Y, Cb, Cr) of steps 1-4, before the level shift."""
    x = np.asarray(x).astype(ft)
    _, h, w = x.shape
    m = 16 if subsampling == "420" else 8
    hp, wp = -(-h // m) * m, -(-w // m) * m
    v = np.clip((x + ft(1)) * ft(127.5), ft(0), ft(255))
    v = v[:, np.clip(np.arange(hp), 0, h - 1)][:, :, np.clip(np.arange(wp), 0, w - 1)]
    r, g, b = v[0], v[1], v[2]
    y = ft(0.299) * r + ft(0.587) * g + ft(0.114) * b
    cb = ft(128) - ft(0.168736) * r - ft(0.331264) * g + ft(0.5) * b
    cr = ft(128) + ft(0.5) * r - ft(0.418688) * g - ft(0.081312) * b
    if subsampling == "420":
        cb = ((cb[0::2, 0::2] + cb[0::2, 1::2]) + (cb[1::2, 0::2] + cb[1::2, 1::2])) * ft(0.25)
        cr = ((cr[0::2, 0::2] + cr[0::2, 1::2]) + (cr[1::2, 0::2] + cr[1::2, 1::2])) * ft(0.25)
    elif subsampling != "444":
        raise ValueError(subsampling)
    return y, cb, cr


def jpeg_coefs(x, q, subsampling="420", ft=np.float64):
    """[(coef / Q per 8x8 block, Q)] of the three planes: the values step 6 rounds."""
    c = dct_matrix(ft)
    out = []
    for p, base in zip(jpeg_planes(x, subsampling, ft), (LUMA, CHROMA, CHROMA)):
        qt = quant_table(base, q).astype(ft)
        coef = np.einsum("ux,abxy,vy->abuv", c, _blocks(p - ft(128)), c)
        out.append((coef / qt, qt))
    return out


def np_jpeg_codes(x, q, subsampling="420", ft=np.float64):
    """(3,h,w) in [-1,1] -> (3,h,w) integer output codes of the round trip at quality q (1..100)."""
    _, h, w = np.asarray(x).shape
    c = dct_matrix(ft)
    planes = []
    for ratio, qt in jpeg_coefs(x, q, subsampling, ft):
        k = np.rint(ratio)
        planes.append(_unblocks(np.einsum("ux,abuv,vy->abxy", c, k * qt, c)) + ft(128))
    y, cb, cr = planes
    if subsampling == "420":
        cb, cr = (np.repeat(np.repeat(p, 2, axis=0), 2, axis=1) for p in (cb, cr))
    r = y + ft(1.402) * (cr - ft(128))
    g = y - ft(0.344136) * (cb - ft(128)) - ft(0.714136) * (cr - ft(128))
    b = y + ft(1.772) * (cb - ft(128))
    return np.clip(np.rint(np.stack([r, g, b])), 0, 255).astype(np.int64)[:, :h, :w]


def codes_to_value(codes):
    return np.asarray(codes).astype(np.float32) / np.float32(127.5) - np.float32(1)


def value_to_codes(v):
    """The codes of an output that is bit-equal to float32(c) / 127.5 - 1 (asserted)."""
    v = np.asarray(v, dtype=np.float32)
    c = np.rint((v.astype(np.float64) + 1.0) * 127.5).astype(np.int64)
    assert np.array_equal(codes_to_value(c), v), "the output is not float32(code) / 127.5 - 1 of integer codes"
    return c


def tie_pixel_mask(x, q, subsampling="420", margin=0.01):
    """(h,w) bool: pixels whose Y block or one of whose chroma blocks holds a coefficient within `margin` steps of a rounding tie."""
    _, h, w = np.asarray(x).shape
    masks = []
    for i, (ratio, _) in enumerate(jpeg_coefs(x, q, subsampling)):
        near = (np.abs(np.abs(ratio - np.floor(ratio)) - 0.5) < margin).any(axis=(2, 3))
        px = 16 if (i > 0 and subsampling == "420") else 8
        masks.append(np.repeat(np.repeat(near, px, axis=0), px, axis=1)[:h, :w])
    return masks[0] | masks[1] | masks[2]


def tie_free_image(h, w, q, subsampling, seed):
    """(3,h,w) float32 in [-1,1] built from the coefficient domain (h, w multiples of the MCU): per block at most two non-zero integer
    coefficients in the 3x3 low-frequency corner plus offsets of |eps| <= 0.1 quantisation steps (0.04 at q = 20) on every coefficient,
    inverse-transformed in float64; "420" chroma is built at half size and replicated.  Asserts that every value lies in [4, 251] and that
    every coefficient, recomputed in float64 from the float32 image, is at least 0.3 steps from a tie."""
    rng = np.random.RandomState(seed)
    eps = 0.04 if q == 20 else 0.1
    c = dct_matrix()
    planes = []
    for i, base in enumerate((LUMA, CHROMA, CHROMA)):
        sub = 2 if (i > 0 and subsampling == "420") else 1
        nh, nw = h // (8 * sub), w // (8 * sub)
        qt = quant_table(base, q).astype(np.float64)
        k = np.zeros((nh, nw, 8, 8))
        for a in range(nh):
            for b in range(nw):
                for _ in range(2):
                    u, v = rng.randint(0, 3, size=2)
                    lim = 40.0 / qt[u, v]                      # keeps the block inside the code range
                    k[a, b, u, v] = np.round(rng.uniform(-lim, lim)) if (u, v) != (0, 0) else np.round(rng.uniform(-1.0, 1.0) * 300.0 / qt[0, 0])
        k = k + rng.uniform(-eps, eps, size=k.shape)
        p = _unblocks(np.einsum("ux,abuv,vy->abxy", c, k * qt, c)) + 128.0
        planes.append(np.repeat(np.repeat(p, sub, axis=0), sub, axis=1))
    y, cb, cr = planes
    rgb = np.stack([y + 1.402 * (cr - 128.0), y - 0.344136 * (cb - 128.0) - 0.714136 * (cr - 128.0), y + 1.772 * (cb - 128.0)])
    assert rgb.min() >= 4.0 and rgb.max() <= 251.0, (rgb.min(), rgb.max())
    x = (rgb / 127.5 - 1.0).astype(np.float32)
    for ratio, _ in jpeg_coefs(x, q, subsampling):
        dist = np.abs(np.abs(ratio - np.floor(ratio)) - 0.5)
        assert dist.min() >= 0.3, dist.min()
    return x


def synthetic_image(h, w, seed=0):
    """(3,h,w) uint8: smooth gradients, a few edges and mild texture -- a fixed stand-in for a photograph."""
    rng = np.random.RandomState(1000 + seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((3, h, w))
    for ch in range(3):
        a, b, ph = rng.uniform(0.05, 0.35, size=3)
        img[ch] = 128 + 60 * np.sin(a * xx + ph * 6) * np.cos(b * yy) + 40 * ((xx * (ch + 1) + yy * 2) % 17 > 8) + rng.normal(0, 6, size=(h, w))
    img[:, h // 3:h // 2, w // 4:w // 2] += 35
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def psnr(a, b):
    mse = np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)
    return 10.0 * math.log10(255.0 ** 2 / max(mse, 1e-12))
