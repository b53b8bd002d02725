"""Integer-exact cases of the first-layer forward (csrc/conv_c3.hip) at every strip height.  A workgroup of conv_c3_fwd_kernel
covers 16, 32 or 64 rows x 16 columns x 64 output channels (FSR_C3_ROWS forces the height; unset, the host picks one per shape);
wave w owns rows [w ROWS/4, (w+1) ROWS/4) of the strip and a row at or beyond H is skipped.  What can go wrong is index
arithmetic: the (ROWS + 2) x 18 x 3 patch and its up to 14 elements per thread, the row a wave starts at, the ragged last strip
(70 rows = one 64-row strip and a 6-row one, or two 32-row strips and a 6-row one), an image shorter than a strip (17 rows), and
a last strip of ONE row in which three of the four waves have nothing to do (65 rows).

Inputs are test_exact.py's small integers: f32 accumulation is exact in any order, there is no tolerance, and the results of
the four heights are compared with torch.equal on the raw storage as well."""
import functools

import pytest
import torch
import torch.nn.functional as F

from backend import L, ops, select
from test_c3_stream import _leaky02, _round_to_storage
from test_exact import F64, _C3_SCALE, _C3_SHIFT, _c3_image, _cases, _gen, _grads, _nchw, exact, ibias, ints, pm1, premise16

FAM = "c3_strips"
ROWS = ("16", "32", "64", None)          # None: the host's own rule
N = 2


def _set_rows(monkeypatch, rows):
    if rows is None:
        monkeypatch.delenv("FSR_C3_ROWS", raising=False)
    else:
        monkeypatch.setenv("FSR_C3_ROWS", rows)


def _sign_bytes(pos_nchw):
    """bool NCHW -> the [N][H][W][C / 8] sign bytes: bit c & 7 of byte c >> 3."""
    pos = pos_nchw.permute(0, 2, 3, 1)
    want = torch.zeros(pos.shape[:3] + (pos.shape[3] // 8,), dtype=torch.uint8)
    for c in range(pos.shape[3]):
        want[..., c >> 3] |= pos[..., c].to(torch.uint8) << (c & 7)
    return want


@functools.lru_cache(maxsize=None)
def _problem(cdn, cout, variant, h, w):
    """Inputs and float64 references of one case, computed once and shared by the launches of every strip height."""
    cd = ops.Compute(cdn)
    g = _gen(61)
    p = {}
    if variant == "head":
        # the generator head's data gradient: the image is the NHWC 3-channel gradient g3 of a cout -> 3 convolution, the filter
        # that convolution's, packed transposed (PACK_C3T); no bias, no activation
        g3 = ints(g, (N, 3, h, w))
        wh = pm1(g, 3, cout, density=0.5)
        p["img"] = g3.permute(0, 2, 3, 1).float().contiguous().permute(0, 3, 1, 2)       # (N, 3, H, W) view of an NHWC tensor
        p["w"], p["pack"], p["bias"] = wh, ops.PACK_C3T, None
        p["ref"], _ = _grads(torch.zeros(N, cout, h, w, dtype=F64), wh, g3, 1)
        p["z"] = p["ref"]
        premise16(FAM, g3, p["ref"])
        return p
    imgf, xn_scaled = _c3_image(g, N, h, w, "nchw")
    xn = xn_scaled if variant == "scale_shift" else imgf.double()
    wt, bias = pm1(g, cout, 3), ibias(g, cout)
    z = F.conv2d(xn, wt, bias, 1, 1)
    premise16(FAM, xn, z)
    p["img"], p["w"], p["pack"], p["bias"], p["z"] = imgf, wt, ops.PACK_C3, bias, z
    p["ref"] = F.prelu(z, torch.tensor([-0.25], dtype=F64)) if variant == "prelu_preact" else _round_to_storage(cd, _leaky02(z))
    return p


def _launch(cd, dev, p, variant, cout, h, w):
    """One fsr_conv3x3_c3_fwd launch -> (out, pre-activation copy or None, sign bytes or None), raw storage on `dev`."""
    head, prelu = variant == "head", variant == "prelu_preact"
    imgd = p["img"].permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2) if head else p["img"].to(dev)
    biasd = None if p["bias"] is None else p["bias"].float().to(dev)
    out = ops._empty((N, h, w, cout), cd.torch_dtype, dev)
    pre = ops._empty_like(out) if prelu else None
    want_signs = variant == "leaky" and (cd.is16 or cd.x3) and cout % 64 == 0
    signs = torch.zeros((N, h, w, cout // 8), dtype=torch.uint8, device=dev) if want_signs else None
    a = torch.tensor([-0.25]).to(dev) if prelu else None
    wpk = ops.packed_filter(cd, p["w"].float().to(dev), p["pack"], 32)
    scale, shift = (_C3_SCALE, _C3_SHIFT) if variant == "scale_shift" else ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    act = L.ACT_NONE if head else (L.ACT_PRELU if prelu else L.ACT_LEAKY)
    L.check(L.lib().fsr_conv3x3_c3_fwd(cd.code, imgd.data_ptr(), *imgd.stride(), N, h, w, *scale, *shift, wpk.data_ptr(), ops._p(biasd),
                                       act, 0.2, ops._p(a), cout, out.data_ptr(), ops._p(pre), ops._p(signs), ops._stream()),
            "fsr_conv3x3_c3_fwd")
    return out, pre, signs


def _check(cd, p, got, what):
    out, pre, signs = got
    exact("first layer forward, %s" % what, _nchw(out, cd), p["ref"])
    if pre is not None:
        exact("pre-activation copy, %s" % what, _nchw(pre, cd), p["z"])
    if signs is not None:
        assert torch.equal(signs.cpu(), _sign_bytes(p["ref"] > 0)), "sign bytes, %s" % what


_VARIANTS = ("leaky", "prelu_preact", "scale_shift", "head")
_SHAPES = ((70, 35), (17, 35))
_DT = ("x3", "f16", "bf16", "f32")


@pytest.mark.parametrize("backend,cdn,cout,variant,hw", _cases(
    emu=[("bf16", 64, "leaky", (70, 35)), ("f32", 64, "prelu_preact", (17, 35)), ("f32", 32, "head", (70, 35)),
         ("bf16", 128, "scale_shift", (17, 35))],
    hip=[(c, 64, v, s) for c in _DT for v in _VARIANTS for s in _SHAPES] + [(c, 128, "leaky", s) for c in _DT for s in _SHAPES] +
        [("x3", 32, "leaky", (70, 35))]))
def test_c3_forward_at_every_strip_height(backend, cdn, cout, variant, hw, monkeypatch):
    """FSR_C3_ROWS = 16, 32, 64 and unset on N = 2, 70 x 35 (ragged last strip, ragged width) and 17 x 35 (shorter than a strip):
    every storage type; one and two channel blocks, and the narrow 32; bias + LeakyReLU(0.2) with the sign bytes; PReLU(-0.25)
    with the pre-activation copy; scale and shift; the head's data-gradient route (NHWC-strided image, transposed filter).  Each
    result is exact against float64, and all four are the same bits."""
    dev = select(backend)
    cd = ops.Compute(cdn)
    h, w = hw
    p = _problem(cdn, cout, variant, h, w)
    first = None
    for rows in ROWS:
        _set_rows(monkeypatch, rows)
        got = _launch(cd, dev, p, variant, cout, h, w)
        _check(cd, p, got, "FSR_C3_ROWS=%s" % rows)
        if first is None:
            first = got
        else:
            for a, b in zip(first, got):
                assert (a is None and b is None) or torch.equal(a, b), "FSR_C3_ROWS=%s differs from 16 rows" % rows


@pytest.mark.parametrize("backend,cdn,h", _cases(
    emu=[("bf16", 65)],
    hip=[(c, h) for c in ("x3", "f16") for h in (64, 65)]))
def test_c3_forward_strip_switch_at_the_image_edge(backend, cdn, h, monkeypatch):
    """FSR_C3_ROWS=64 at H = 64 (exactly one strip) and H = 65 (a second strip of ONE row: wave 0 does one row, the other three
    waves none, and every patch row below the image is zero)."""
    dev = select(backend)
    cd = ops.Compute(cdn)
    p = _problem(cdn, 64, "leaky", h, 35)
    _set_rows(monkeypatch, "64")
    _check(cd, p, _launch(cd, dev, p, "leaky", 64, h, 35), "H=%d, 64-row strips" % h)
