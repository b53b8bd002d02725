"""Test helper: the colour contract of DESIGN.md §6c for planar YUV at 4:2:0, 4:2:2 and 4:4:4, 8 to 16 bits, restated in numpy
independently of the code under test, and the small helpers the video tests share (test_video.py, test_video_deep.py,
test_video_chroma.py).

Storage: planar, Y h x w, then Cb, then Cr of ceil(h/2) x ceil(w/2) (4:2:0), h x ceil(w/2) (4:2:2) or h x w (4:4:4); 1 byte per sample
at depth 8, 2 little-endian above.  Codes at depth d:
  limited range: Y = (16 + 219 E_Y) 2^(d-8), C = (128 + 224 E_C) 2^(d-8);  full range: Y = (2^d - 1) E_Y, C = 2^(d-1) + (2^d - 1) E_C;
  encode: code = clamp(floor(v + 0.5), 0, 2^d - 1)."""
import importlib
import os
import subprocess
import sys
import types

import numpy as np

from conftest import load_npz, sd_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dataloader = importlib.import_module("fast-srgan_amd.dataloader")

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
# Share of samples that may differ (by one code) from the float64 restatement.  1e-3 is the project's cap for float32 against
# float64 rounding ties.  Measured: the float32 restatement below ALONE, against float64, on the inputs of test_video_deep's
# test_encode_random (both shapes, all four matrix / range pairs: 4680 samples per depth) differs on 0 samples at d = 8 and 12, on 1
# (0.021 %) at d = 10, on 3 (0.064 %) at d = 14 and on 10 (0.214 %) at d = 16 -- float32 resolves only 1/1024 and 1/256 of a code at
# the top of the 14- and 16-bit ranges, so more ties fall the other way there, and the cap is 1e-2: more than three times either
# measurement (test_float32_restatement_is_inside_the_caps keeps that true; test_float32_restatement_is_inside_a_third_of_the_caps
# does the same for 4:2:2 and 4:4:4 on the inputs of test_video_chroma's test_encode_random).
CAP = {8: 1e-3, 9: 1e-3, 10: 1e-3, 12: 1e-3, 14: 1e-2, 16: 1e-2}


def _coefs(full, d, ft=np.float64):
    """(Y scale, Y offset, C scale, C offset, top code) at depth d."""
    up, top = ft(2 ** (d - 8)), ft(2 ** d - 1)
    return (top, ft(0), top, ft(128) * up, top) if full else (ft(219) * up, ft(16) * up, ft(224) * up, ft(128) * up, top)


def chroma_h(h, chroma):
    return h if chroma != "420" else (h + 1) // 2


def chroma_w(w, chroma):
    return w if chroma == "444" else (w + 1) // 2


def samples_of(h, w, chroma="420"):
    return h * w + 2 * chroma_h(h, chroma) * chroma_w(w, chroma)


def np_encode(t, chroma, matrix="bt601", full=False, d=8, ft=np.float64):
    """(N,3,H,W) tanh output t -> (N, samples) integer codes of the planes at depth d, computed in `ft`: c = clamp((t + 1) / 2, 0, 1);
    Y per pixel; with e = B - E_Y or R - E_Y, E_C = s / (2 (1 - K)) where s is e itself ("444"), ((e[2j-1] + e[2j+1]) + 2 e[2j]) / 4
    for the chroma column j co-sited with luma column 2j, columns -1 and W clamped ("422"), or the mean of e over the 2x2 block,
    summed in the kernels' order -- the vertical pair first, then the two columns ("420", H and W even: C420jpeg siting)."""
    t = np.asarray(t).astype(ft)
    n, _, h, w = t.shape
    kr, kb = (ft(v) for v in KR_KB[matrix])
    kg = ft(1) - kr - kb
    ys, yo, cs, co, top = _coefs(full, d, ft)
    c = np.clip((t + ft(1)) / ft(2), ft(0), ft(1))
    r, g, b = c[:, 0], c[:, 1], c[:, 2]
    ey = kr * r + kg * g + kb * b

    def sub(e, k):
        if chroma == "444":
            return e / (ft(2) * (ft(1) - k))
        if chroma == "422":
            centre = np.arange(0, w, 2)
            left, right = np.clip(centre - 1, 0, w - 1), np.clip(centre + 1, 0, w - 1)
            s = (e[:, :, left] + e[:, :, right]) + ft(2) * e[:, :, centre]
        else:
            col = e[:, 0::2, :] + e[:, 1::2, :]
            s = col[:, :, 0::2] + col[:, :, 1::2]
        return s * ft(0.25) / (ft(2) * (ft(1) - k))

    def code(v):
        return np.clip(np.floor(v + ft(0.5)), 0, top).astype(np.int64)

    return np.concatenate([p.reshape(n, -1) for p in (code(yo + ys * ey), code(co + cs * sub(b - ey, kb)), code(co + cs * sub(r - ey, kr)))],
                          axis=1)


def np_decode(samples, h, w, chroma, siting, matrix="bt601", full=False, d=8):
    """(N, samples) integer codes of the planes -> (N,3,h,w) float64 generator input 2c - 1.  Chroma is interpolated linearly with edge
    clamp: horizontally ("420", "422") luma column x reads chroma at (x - 1/2) / 2 ("jpeg") or x / 2 ("mpeg2", what C422 means);
    vertically ("420") luma row y reads chroma at (y - 1/2) / 2; "444" has no interpolation.  Then the inverse matrix, R, G, B
    clamped to [0, 1]."""
    s = np.asarray(samples).astype(np.float64)
    n = s.shape[0]
    ch, cw = chroma_h(h, chroma), chroma_w(w, chroma)
    yp = s[:, :h * w].reshape(n, h, w)
    cbp = s[:, h * w:h * w + ch * cw].reshape(n, ch, cw)
    crp = s[:, h * w + ch * cw:].reshape(n, ch, cw)
    cx = (np.arange(w) - 0.5) / 2.0 if siting == "jpeg" else np.arange(w) / 2.0
    x0 = np.floor(cx).astype(int)
    fx = (cx - x0)[None, :]
    xa, xb = np.clip(x0, 0, cw - 1), np.clip(x0 + 1, 0, cw - 1)
    cy = (np.arange(h) - 0.5) / 2.0
    y0 = np.floor(cy).astype(int)
    fy = (cy - y0)[:, None]
    ya, yb = np.clip(y0, 0, ch - 1), np.clip(y0 + 1, 0, ch - 1)

    def across(p):
        return (1 - fx) * p[:, :, xa] + fx * p[:, :, xb]

    def up(p):
        if chroma == "444":
            return p
        if chroma == "422":
            return across(p)
        return (1 - fy) * across(p[:, ya]) + fy * across(p[:, yb])

    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    ys, yo, cs, co, _ = _coefs(full, d)
    ey, ecb, ecr = (yp - yo) / ys, (up(cbp) - co) / cs, (up(crp) - co) / cs
    r = ey + 2.0 * (1.0 - kr) * ecr
    b = ey + 2.0 * (1.0 - kb) * ecb
    g = (ey - kr * r - kb * b) / kg
    return 2.0 * np.clip(np.stack([r, g, b], axis=1), 0.0, 1.0) - 1.0


def to_payload(codes, d):
    """(N, samples) integer codes -> the (N, bytes) uint8 payload at depth d."""
    codes = np.ascontiguousarray(codes)
    return codes.astype(np.uint8) if d == 8 else np.ascontiguousarray(codes.astype("<u2")).view(np.uint8)


def from_payload(payload, d):
    payload = np.ascontiguousarray(np.asarray(payload))
    return payload.astype(np.int64) if d == 8 else payload.view("<u2").astype(np.int64)


def assert_codes_close(got, want, frac):
    """Every sample within 1 code; at most `frac` of them differ at all (float32 against float64 rounding ties)."""
    diff = np.abs(np.asarray(got).astype(np.int64) - np.asarray(want).astype(np.int64))
    print("codes: max difference %d, %d of %d differ (cap %g)" % (diff.max(), (diff > 0).sum(), diff.size, frac))
    assert diff.max() <= 1, diff.max()
    assert (diff > 0).sum() <= frac * diff.size, ((diff > 0).sum(), diff.size)


def _aa_matrix(n_in, n_out):
    """The antialiased bicubic of one axis (dataloader.aa_bicubic_taps) as a float64 (n_out, n_in) matrix."""
    xmin, xsize, taps, _ = dataloader.aa_bicubic_taps(n_in, n_out)
    m = np.zeros((n_out, n_in))
    for i in range(n_out):
        m[i, xmin[i]:xmin[i] + xsize[i]] = taps[i, :xsize[i]].astype(np.float64)
    return m


def ns(**k):
    return types.SimpleNamespace(**k)


def _stream(header, payloads, frame_line=b"FRAME\n"):
    """A Y4M stream: the header line, then every payload behind its FRAME line."""
    return header + b"".join(frame_line + bytes(p) for p in payloads)


def _tiny(pkg, dev):
    G = pkg.Generator(ns(n_filters=16, n_layers=1), compute_dtype="f32")
    G.load_state_dict(sd_from(load_npz("g_tiny.npz"), "sd."))
    return G.to(dev).eval()


def _shipped(pkg, dev, cdn):
    G = pkg.Generator(ns(n_filters=64, n_layers=8), compute_dtype=cdn)
    G.load_state_dict(sd_from(load_npz("g_model_pt.npz"), "sd."))
    return G.to(dev).eval()


def _cli(cli_dir, data, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "video.py"), "--input", "-", "--output", "-", "--batch", "2"] + list(flags),
                       input=data, capture_output=True, cwd=cli_dir, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r
