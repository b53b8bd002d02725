"""Test helper: the contract of the high-order degradation stages, restated in numpy independently of the code under
test, and the fixtures test_degrade_ho.py shares.

filter2d: out[n][c][y][x] = sum_dy sum_dx k_n[dy + r][dx + r] in[n][c][clamp(y + dy)][clamp(x + dx)] -- correlation, clamped source
index, r = radii[n] clamped to 0..10, K = 2 r + 1, the K x K taps row-major and packed at the start of the sample's 441 slots; r = 0
returns the sample as it is.
resize_select: tmp[y][xo] = sum_k wx[f][xo][k] in[y][xmin[f][xo] + k], out[yo][xo] = sum_k wy[f][yo][k] tmp[ymin[f][yo] + k][xo], f = sel[n].
noise kinds: x += z * amp * (2 / 255); amp = sigma, or sqrt(g v) with v = clamp((x + 1) 127.5, 0, 255) (shot); z of degrade_contract.np_z
at element (c h + y) w + x, or y w + x (grey).
Kernel bank: the formulas of the issue, see bank_reference."""
import math

import numpy as np

import degrade_contract as C

MAX_RADIUS = 10
TAPS = (2 * MAX_RADIUS + 1) ** 2
POISON = np.float32(1e30)


def clamp_radius(r):
    return min(max(int(r), 0), MAX_RADIUS)


def np_filter2d(x, radii, taps, ft=np.float64):
    """(N,3,h,w) -> the filtered batch in `ft`; taps: (N, TAPS), sample i reads taps[i][:K * K] as a K x K row-major kernel.  The sum runs
    dy outer, dx inner, as the contract's float32 accumulation does."""
    x = np.asarray(x)
    out = x.astype(ft).copy()
    n, _, h, w = x.shape
    ys, xs = np.arange(h), np.arange(w)
    for i in range(n):
        r = clamp_radius(radii[i])
        if r == 0:
            continue
        K = 2 * r + 1
        k = np.asarray(taps[i][:K * K]).reshape(K, K)
        src = x[i].astype(ft)
        acc = np.zeros_like(src)
        for dy in range(-r, r + 1):
            rows = src[:, np.clip(ys + dy, 0, h - 1), :]
            for dx in range(-r, r + 1):
                acc = acc + ft(k[dy + r, dx + r]) * rows[:, :, np.clip(xs + dx, 0, w - 1)]
        out[i] = acc
    return out


def dyadic_kernels(radii, seed):
    """(n, TAPS) float32 tables for np_filter2d / the C entry point: per sample K x K NON-ZERO signed multiples of 1/64 that sum to 1 and
    differ from their transpose and from both flips (an x / y swap, or convolution in place of correlation, shows); every slot behind
    K * K holds 1e30, and so does the WHOLE block of a sample whose radius clamps to 0 (a copy reads no tap).  Returns (taps, the
    largest sum |k| of a sample)."""
    rng = np.random.RandomState(seed)
    taps = np.full((len(radii), TAPS), POISON, dtype=np.float32)
    widest = 1.0
    for i, r in enumerate(radii):
        r = clamp_radius(r)
        if r == 0:
            continue
        K = 2 * r + 1
        while True:
            k = rng.choice([-2, -1, 1, 2, 3], size=(K, K))
            k[r, r] += 64 - k.sum()
            if k[r, r] != 0 and not any(np.array_equal(k, v) for v in (k.T, k[::-1], k[:, ::-1], k[::-1, ::-1])):
                break
        taps[i, :K * K] = (k / 64.0).reshape(-1)
        widest = max(widest, np.abs(k).sum() / 64.0)
    return taps, widest


def steps(shape, seed):
    """float32 in steps of 1/64 in [-1, 1]"""
    return (np.random.RandomState(seed).randint(-64, 65, size=shape) / 64.0).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------- kernel bank
def bank_reference(kind, size, sigma_x, sigma_y, theta, beta):
    """The float64 kernel of the issue's formulas BEFORE the float32 cast, through the explicit 2 x 2 inverse of
    S = R(theta) diag(sx^2, sy^2) R(theta)^T (the package rotates the offsets instead)."""
    c = (size - 1) / 2.0
    rot = np.array([[math.cos(theta), -math.sin(theta)], [math.sin(theta), math.cos(theta)]])
    inv = np.linalg.inv(rot @ np.diag([sigma_x ** 2, sigma_y ** 2]) @ rot.T)
    k = np.zeros((size, size))
    for i in range(size):
        for j in range(size):
            u = np.array([j - c, i - c])
            q = float(u @ inv @ u)
            k[i, j] = {"gauss": math.exp(-q / 2.0), "generalized": math.exp(-q ** beta / 2.0), "plateau": 1.0 / (1.0 + q ** beta)}[kind]
    return k / k.sum()


def j1_series(x, terms=120):
    """J1 by its power series in exact rational arithmetic, rounded once: sum_m (-1)^m (x/2)^(2m+1) / (m! (m+1)!).  Slow; a second
    reference for where scipy is absent."""
    from fractions import Fraction
    h = Fraction(x) / 2
    term, total = h, Fraction(0)
    for m in range(terms):
        total += term
        term = -term * h * h / ((m + 1) * (m + 2))
    return float(total)


# ----------------------------------------------------------------------------------------------------------- resize_select
def np_resize_select(x, tables_x, tables_y, sel, ft=np.float64, passes=False):
    """(N,3,H,W) -> (N,3,h,w) in `ft`; tables_?: [(xmin, xsize, w)] per filter, sample i uses filter sel[i]."""
    x = np.asarray(x)
    n, _, H, W = x.shape
    ow, oh = len(tables_x[0][0]), len(tables_y[0][0])
    mid = np.zeros((n, 3, H, ow), dtype=ft)
    out = np.zeros((n, 3, oh, ow), dtype=ft)
    for i in range(n):
        xmin, xsize, wt = tables_x[sel[i]]
        for xo in range(ow):
            acc = np.zeros((3, H), dtype=ft)
            for k in range(int(xsize[xo])):
                acc = acc + ft(wt[xo][k]) * x[i, :, :, int(xmin[xo]) + k].astype(ft)
            mid[i, :, :, xo] = acc
        ymin, ysize, wt = tables_y[sel[i]]
        for yo in range(oh):
            acc = np.zeros((3, ow), dtype=ft)
            for k in range(int(ysize[yo])):
                acc = acc + ft(wt[yo][k]) * mid[i, :, int(ymin[yo]) + k, :]
            out[i, :, yo, :] = acc
    return (out, mid) if passes else out


def dyadic_table(in_size, out_size, kmax, seed):
    """(xmin, xsize, w) with per-output windows of 1..kmax NON-ZERO signed sixteenths summing to 1, asymmetric where longer than one tap;
    the slots behind xsize hold 1e30."""
    rng = np.random.RandomState(seed)
    xmin = np.zeros(out_size, dtype=np.int32)
    xsize = np.zeros(out_size, dtype=np.int32)
    w = np.full((out_size, kmax), POISON, dtype=np.float32)
    for o in range(out_size):
        ks = int(rng.randint(1, min(kmax, in_size) + 1))
        lo = int(rng.randint(0, in_size - ks + 1))
        while True:
            k = rng.choice([-2, -1, 1, 2, 3], size=ks)
            k[ks // 2] += 16 - k.sum()
            if k[ks // 2] != 0 and (ks == 1 or not np.array_equal(k, k[::-1])):
                break
        xmin[o], xsize[o], w[o, :ks] = lo, ks, k / 16.0
    return xmin, xsize, w


# ----------------------------------------------------------------------------------------------------------- noise kinds
SHOT, GREY = 1, 2


def np_noise_kinds(x, strength, flags, seeds):
    """(N,3,h,w) float32 -> (float64 result, float64 per-element amplitude in code units); strength 0 returns the sample as it is."""
    x = np.asarray(x)
    out = x.astype(np.float64).copy()
    amp = np.zeros(x.shape, dtype=np.float64)
    _, _, h, w = x.shape
    for i, (g, f, (s0, s1)) in enumerate(zip(strength, flags, seeds)):
        if g == 0:
            continue
        if f & GREY:
            z = np.broadcast_to(C.np_z(h * w, s0, s1).reshape(1, h, w), (3, h, w))
        else:
            z = C.np_z(3 * h * w, s0, s1).reshape(3, h, w)
        a = np.full((3, h, w), float(g))
        if f & SHOT:
            a = np.sqrt(float(g) * np.clip((x[i].astype(np.float64) + 1.0) * 127.5, 0.0, 255.0))
        out[i] = out[i] + z * a * (2.0 / 255.0)
        amp[i] = a
    return out, amp
