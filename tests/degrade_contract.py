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


def np_blur_taps(x, radii, taps, ft=np.float64, passes=False):
    """(N,3,h,w) -> the batch blurred in `ft` with the caller's tables: sample i uses taps[i][j + r], j = -r..r, r = radii[i] clamped to
    0..MAX_RADIUS as the kernel documents; r = 0 returns the sample as it is.  passes=True also returns the horizontal pass."""
    x = np.asarray(x)
    out = x.astype(ft).copy()
    mid = out.copy()
    n, _, h, w = x.shape
    for i in range(n):
        r = min(max(int(radii[i]), 0), MAX_RADIUS)
        if r == 0:
            continue
        src = x[i].astype(ft)
        xs = np.arange(w)
        acc = np.zeros_like(src)
        for j in range(-r, r + 1):
            acc = acc + ft(taps[i][j + r]) * src[:, :, np.clip(xs + j, 0, w - 1)]
        ys = np.arange(h)
        acc2 = np.zeros_like(src)
        for j in range(-r, r + 1):
            acc2 = acc2 + ft(taps[i][j + r]) * acc[:, np.clip(ys + j, 0, h - 1), :]
        mid[i], out[i] = acc, acc2
    return (out, mid) if passes else out


def np_blur(x, sigmas, ft=np.float64):
    """(N,3,h,w) -> the blurred batch computed in `ft` with the float32 taps; a sample with sigma = 0 is returned as it is."""
    tables = [blur_taps(s) for s in sigmas]
    return np_blur_taps(x, [r for r, _ in tables], [t for _, t in tables], ft)


def dyadic_taps(radii, seed):
    """(n, TAPS) float32 tables for np_blur_taps / the C entry point: per sample 2r + 1 NON-ZERO signed multiples of 1/16 that sum to 1 and
    differ from their mirror image (a reversed tap order, or j swapped with -j, shows), tap j at slot j + r; the slots behind them hold
    1e30.  A radius outside 0..MAX_RADIUS gets the table of the radius the kernel clamps it to, except that a negative one gets a FULL
    table (which the kernel must not read).  Returns (taps, sum |w| of the widest sample)."""
    rng = np.random.RandomState(seed)
    taps = np.full((len(radii), TAPS), 1e30, dtype=np.float32)
    widest = 1.0
    for i, r in enumerate(radii):
        r = MAX_RADIUS if r < 0 else min(int(r), MAX_RADIUS)
        while True:
            k = rng.choice([-2, -1, 1, 2, 3], size=2 * r + 1)
            k[r] += 16 - k.sum()
            if k[r] != 0 and abs(k[r]) <= 16 and (r == 0 or not np.array_equal(k, k[::-1])):
                break
        taps[i, :2 * r + 1] = k / 16.0
        widest = max(widest, np.abs(k).sum() / 16.0)
    return taps, widest


# ----------------------------------------------------------------------------------------------------------- noise
def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def unmix32(x):
    """The inverse of mix32 (a bijection of the 32-bit words): it names the seed that puts a wanted draw at a wanted element."""
    x = np.asarray(x, dtype=np.uint64) & 0xffffffff
    x ^= x >> 16
    x = (x * pow(0x846ca68b, -1, 1 << 32)) & 0xffffffff
    x ^= (x >> 15) ^ (x >> 30)
    x = (x * pow(0x7feb352d, -1, 1 << 32)) & 0xffffffff
    x ^= x >> 16
    return x


def seed_for_draw(a, e, s1):
    """s0 such that element e of a sample with seed words (s0, s1) draws the 32-bit word `a` for its first uniform."""
    return int((int(unmix32(int(unmix32(a)) ^ s1)) - 2 * e) & 0xffffffff)


def hash_draws(count, s0, s1):
    """The two 24-bit integers (a >> 8, b >> 8) of the elements e = 0..count-1 (or of an array of element indices) of a sample with seed
    words (s0, s1)."""
    e = np.arange(count, dtype=np.uint64) if np.ndim(count) == 0 else np.asarray(count).astype(np.uint64)
    a = mix32(mix32((np.uint64(s0) + 2 * e) & 0xffffffff) ^ np.uint64(s1))
    b = mix32(mix32((np.uint64(s0) + 2 * e + 1) & 0xffffffff) ^ np.uint64(s1))
    return a >> 8, b >> 8


def np_z(count, s0, s1, ft=np.float64, radius=False, plus=1):
    """z of the elements e = 0..count-1 (or of an array of element indices) of a sample with seed words (s0, s1), evaluated in `ft` from
    the contract's integers; with radius=True also R = sqrt(-2 ln u1).  `plus` is the contract's + 1 of u1: the sharpness self-test passes 0 (with 0 kept off the log)."""
    a, b = hash_draws(count, s0, s1)
    u1 = np.maximum(a + plus, 1).astype(ft) * ft(2.0 ** -24)
    u2 = b.astype(ft) * ft(2.0 ** -24)
    rad = np.sqrt(ft(-2) * np.log(u1))
    z = rad * np.cos(ft(np.float32(6.2831855)) * u2)
    return (z, rad) if radius else z


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


def jpeg_coefs(x, q, subsampling="420", ft=np.float64, tables=None):
    """[(coef / Q per 8x8 block, Q)] of the three planes: the values step 6 rounds.  `tables`: (luma, chroma) base tables in place of
    Annex K's, for the tests that ask which entries an input can see."""
    c = dct_matrix(ft)
    out = []
    luma, chroma = (LUMA, CHROMA) if tables is None else tables
    for p, base in zip(jpeg_planes(x, subsampling, ft), (luma, chroma, chroma)):
        qt = quant_table(base, q).astype(ft)
        coef = np.einsum("ux,abxy,vy->abuv", c, _blocks(p - ft(128)), c)
        out.append((coef / qt, qt))
    return out


def np_jpeg_codes(x, q, subsampling="420", ft=np.float64, tables=None, unrounded=False):
    """(3,h,w) in [-1,1] -> (3,h,w) integer output codes of the round trip at quality q (1..100); unrounded=True: the values the last
    step rounds and clamps."""
    _, h, w = np.asarray(x).shape
    c = dct_matrix(ft)
    planes = []
    for ratio, qt in jpeg_coefs(x, q, subsampling, ft, tables):
        k = np.rint(ratio)
        planes.append(_unblocks(np.einsum("ux,abuv,vy->abxy", c, k * qt, c)) + ft(128))
    y, cb, cr = planes
    if subsampling == "420":
        cb, cr = (np.repeat(np.repeat(p, 2, axis=0), 2, axis=1) for p in (cb, cr))
    r = y + ft(1.402) * (cr - ft(128))
    g = y - ft(0.344136) * (cb - ft(128)) - ft(0.714136) * (cr - ft(128))
    b = y + ft(1.772) * (cb - ft(128))
    rgb = np.stack([r, g, b])[:, :h, :w]
    return rgb if unrounded else np.clip(np.rint(rgb), 0, 255).astype(np.int64)


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


def _image_from_coefs(coefs, subsampling):
    """Three planes of dequantised coefficients ((nh, nw, 8, 8) each, chroma at its own resolution) -> float32 (3,h,w) in [-1,1]:
    inverse transform in float64, "420" chroma replicated, inverse colour transform; asserts the code range [4, 251]."""
    c = dct_matrix()
    sub = 2 if subsampling == "420" else 1
    y, cb, cr = (_unblocks(np.einsum("ux,abuv,vy->abxy", c, k, c)) + 128.0 for k in coefs)
    cb, cr = (np.repeat(np.repeat(p, sub, axis=0), sub, axis=1) for p in (cb, cr))
    rgb = np.stack([y + 1.402 * (cr - 128.0), y - 0.344136 * (cb - 128.0) - 0.714136 * (cr - 128.0), y + 1.772 * (cb - 128.0)])
    assert rgb.min() >= 4.0 and rgb.max() <= 251.0, (rgb.min(), rgb.max())
    return (rgb / 127.5 - 1.0).astype(np.float32)


def tie_distance(x, q, subsampling):
    """The smallest distance [steps] of a coefficient of x, recomputed in float64, from a rounding tie."""
    return min(np.abs(np.abs(ratio - np.floor(ratio)) - 0.5).min() for ratio, _ in jpeg_coefs(x, q, subsampling))


def output_ties(x, q, subsampling, margin=1e-4):
    """How many output values of the float64 contract lie within `margin` of a rounding tie: the codes float32 arithmetic may move."""
    v = np_jpeg_codes(x, q, subsampling, unrounded=True)
    return int((np.abs(v - np.floor(v) - 0.5) < margin).sum())


def live_positions(x, q, subsampling):
    """(luma, chroma) (8,8) bool: the table positions at which some block of x is quantised to |k| >= 1."""
    live = [(np.abs(np.rint(ratio)) >= 1).any(axis=(0, 1)) for ratio, _ in jpeg_coefs(x, q, subsampling)]
    return live[0], live[1] | live[2]


CB_POSITIONS = [p for p in range(64) if (p + p // 8) % 2 == 0]       # the chroma table's positions are split between Cb and Cr
CR_POSITIONS = [p for p in range(64) if (p + p // 8) % 2 == 1]       # (a checkerboard): 32 blocks of each instead of 64


def _level(target, qv, skip):
    """The largest integer up to target / qv that is no multiple of 3 or 5 (k Q / Q' then is no integer for Q' = 0.75 Q or 1.25 Q), at
    least 1; skip = s takes the s-th smaller one, as far as there is one."""
    levels = [c for c in range(max(1, int(target / qv)), 0, -1) if c % 3 and c % 5]
    return levels[min(skip, len(levels) - 1)]


def every_position_image(q, subsampling, seed, stagger=None):
    """(3,h,w) float32 in [-1,1] built from the coefficient domain so that at quality q every position of the luminance table is quantised
    to |k| >= 1 in some Y block and every position of the chrominance table in some Cb or Cr block (CB_POSITIONS / CR_POSITIONS).  A
    block carries ONE live coefficient, sign (k + e) Q with |e| <= 0.1, and offsets of at most 0.1 steps (and 2 code units) on the other
    63.  Below q = 49, where one step of a Q = 255 entry is 61 codes before the colour transform, an MCU has ONE live plane and the
    others stay at 128 (64 x 128 pixels at "444", 80 x 256 at "420"); from q = 49 all three planes are live in every MCU (64 x 64 and
    64 x 128).  The OUTPUT of such a block is built from few integers k Q, and some of them put whole blocks on a rounding tie of the
    last step (k Q = 4 mod 8 at positions (0|4, 0|4) is 128 +- n.5 on all 64 pixels): while more than a third of 1e-3 of the float64
    output values lie within 1e-4 of a tie, the MCUs that hold one take the next smaller level.  Asserts: every position live; every
    value in [4, 251]; every coefficient, recomputed in float64 from the float32 image, at least 0.3 steps from a tie."""
    rng = np.random.RandomState(seed)
    ny = 4 if subsampling == "420" else 1                           # Y blocks per MCU
    stagger = q < 49 if stagger is None else stagger                # (stagger=True: the one-live-plane layout at any q, for one batch shape)
    if stagger:
        mh, mw = (5, 16) if subsampling == "420" else (8, 16)        # 64 / ny MCUs for Y, then 32 for Cb, then 32 for Cr
        target = (400.0, 250.0, 250.0)
    else:
        mh, mw = (4, 8) if subsampling == "420" else (8, 8)          # "420": 128 Y blocks, every position twice
        target = (200.0, 100.0, 100.0)
    sy = 2 if subsampling == "420" else 1
    shapes = [(mh * sy, mw * sy), (mh, mw), (mh, mw)]
    qts = [quant_table(base, q).astype(np.float64) for base in (LUMA, CHROMA, CHROMA)]
    offsets = [rng.uniform(-1.0, 1.0, size=(nh, nw, 8, 8)) * np.minimum(0.1, 2.0 / qt) for (nh, nw), qt in zip(shapes, qts)]
    live = []                                                        # (plane, block row, block column, MCU, u, v, sign, e in [0, 1))
    for i, (nh, nw) in enumerate(shapes):
        for a in range(nh):
            for b in range(nw):
                m = (a // sy) * mw + b // sy if i == 0 else a * mw + b
                if i == 0:
                    blk = m * ny + (a % sy) * sy + b % sy
                    p = blk % 64 if (not stagger or blk < 64) else None
                else:
                    first = 64 // ny + 32 * (i - 1) if stagger else 0
                    p = (CB_POSITIONS, CR_POSITIONS)[i - 1][(m - first) % 32] if (not stagger or first <= m < first + 32) else None
                if p is not None:
                    live.append((i, a, b, m, p // 8, p % 8, rng.choice([-1.0, 1.0]), rng.uniform()))
    skip = np.zeros(mh * mw, dtype=np.int64)
    while True:
        coefs = [k.copy() for k in offsets]
        for i, a, b, m, u, v, sign, e in live:
            lvl = _level(target[i], qts[i][u, v], skip[m])
            e = -0.1 * e if lvl * qts[i][u, v] > target[i] else 0.2 * e - 0.1
            coefs[i][a, b, u, v] = sign * (lvl + e)
        x = _image_from_coefs([k * qt for k, qt in zip(coefs, qts)], subsampling)
        out = np_jpeg_codes(x, q, subsampling, unrounded=True)
        tied = (np.abs(out - np.floor(out) - 0.5) < 1e-4).sum(axis=0)
        tied = tied.reshape(mh, 8 * sy, mw, 8 * sy).sum(axis=(1, 3)).reshape(-1)
        if tied.sum() <= 1e-3 / 3 * out.size:
            break
        skip += tied > 0
        assert skip.max() < 8, "no level of some MCU keeps its output off the rounding ties"
    luma, chroma = live_positions(x, q, subsampling)
    assert luma.all() and chroma.all(), (int(luma.sum()), int(chroma.sum()))
    assert tie_distance(x, q, subsampling) >= 0.3
    return x


PROBE_D = 0.012          # distance [steps] of a threshold probe's coefficient from its tie


def probe_level(qv):
    """The smallest K for which an entry off by one moves (K + 0.5 +- PROBE_D) Q / (Q +- 1) at least 0.02 steps, i.e. across the tie."""
    return max(0, int(math.ceil(0.02 * (qv + 1) - 0.5)))


def threshold_probe_image(plane, subsampling):
    """(3,h,w) float32 for q = 50, where Q is the base table: per table entry two blocks whose only coefficient is +-(K + 0.5 + d) Q with
    d = +PROBE_D in one and -PROBE_D in the other, K = probe_level(Q) -- an entry off by +1 flips the rounding of the first, off by -1
    that of the second.  plane "luma": a grey 64 x 128 image, block 2 p holds +d and block 2 p + 1 holds -d of position p.  plane
    "chroma": Y = 128, the Cb block of position p holds +d and the Cr block -d (64 x 64 at "444", 128 x 128 at "420").  Asserts the code
    range, that each probe lies PROBE_D +- 0.002 from its tie when recomputed in float64 from the float32 image, and that every other
    coefficient is at least 0.3 steps from one."""
    base = LUMA if plane == "luma" else CHROMA
    sub = 2 if subsampling == "420" else 1
    want = []                                                        # (plane index, block row, block column, u, v, K + 0.5 + d)
    if plane == "luma":
        coefs = [np.zeros((8, 16, 8, 8)), np.zeros((8 // sub, 16 // sub, 8, 8)), np.zeros((8 // sub, 16 // sub, 8, 8))]
        for p in range(64):
            for s, d in enumerate((PROBE_D, -PROBE_D)):
                a, b = divmod(2 * p + s, 16)
                want.append((0, a, b, p // 8, p % 8, (-1.0) ** p * (probe_level(base[p // 8, p % 8]) + 0.5 + d)))
    else:
        coefs = [np.zeros((8 * sub, 8 * sub, 8, 8)), np.zeros((8, 8, 8, 8)), np.zeros((8, 8, 8, 8))]
        for p in range(64):
            for i, d in ((1, PROBE_D), (2, -PROBE_D)):
                want.append((i, p // 8, p % 8, p // 8, p % 8, (-1.0) ** p * (probe_level(base[p // 8, p % 8]) + 0.5 + d)))
    for i, a, b, u, v, r in want:
        coefs[i][a, b, u, v] = r * base[u, v]
    x = _image_from_coefs(coefs, subsampling)
    ratios = [r.copy() for r, _ in jpeg_coefs(x, 50, subsampling)]
    for i, a, b, u, v, r in want:
        assert abs(ratios[i][a, b, u, v] - r) <= 0.002 and abs(abs(r) % 1.0 - 0.5) >= 0.01, (i, a, b, u, v, ratios[i][a, b, u, v], r)
        ratios[i][a, b, u, v] = 0.0
    assert max(np.abs(r).max() for r in ratios) <= 0.2
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
