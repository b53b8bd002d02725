"""The discriminator neck's LeakyReLU backward from packed sign bits in x3 mode, next to test_exact.py's 16-bit case: the x3
form of the first-layer forward writes the [N][H][W][cout / 8] sign bytes of its STORED hi parts (hi > 0: the predicate the
tensor mask applies in conv_s2d3's epilogue), conv_s2d3_kernel<x3> gates its f32 accumulators by them before the x3 split, and
Conv3x3Fn hands the bytes to the data gradient instead of the saved neck output.

Inputs are test_exact.py's small integers (exact in any summation order, no tolerance); the autograd case compares the two
masks of one and the same launch sequence bit for bit."""
import types

import pytest
import torch
import torch.nn.functional as F

from backend import L, ops, select
from test_exact import _cases, _gen, _grads, _kernel, _nchw, _nhwc, exact, gate, ibias, ints, pm1, premise16

FAM = "x3_sign_bits"


def _sign_bytes(pos_nchw):
    """bool NCHW -> the [N][H][W][C / 8] sign bytes: bit c & 7 of byte c >> 3."""
    pos = pos_nchw.permute(0, 2, 3, 1)
    want = torch.zeros(pos.shape[:3] + (pos.shape[3] // 8,), dtype=torch.uint8)
    for c in range(pos.shape[3]):
        want[..., c >> 3] |= pos[..., c].to(torch.uint8) << (c & 7)
    return want


@pytest.mark.parametrize("backend,cout", _cases(emu=[(64,)], hip=[(64,), (128,)]))
def test_x3_forward_writes_the_sign_bytes(backend, cout):
    """fsr_conv3x3_c3_fwd in x3 with bias + LeakyReLU(0.25) on N = 3, 17 x 35: the output is exact and the sign bytes equal
    (out > 0) of the decoded output."""
    dev = select(backend)
    cd = ops.Compute("x3")
    g = _gen(71)
    n, h, w = 3, 17, 35
    img, wt, bias = ints(g, (n, 3, h, w)), pm1(g, cout, 3), ibias(g, cout)
    ref = F.leaky_relu(F.conv2d(img, wt, bias, 1, 1), 0.25)
    premise16(FAM, img, ref)
    imgd, biasd = img.float().to(dev), bias.float().to(dev)
    out = ops._empty((n, h, w, cout), cd.torch_dtype, dev)
    signs = torch.zeros((n, h, w, cout // 8), dtype=torch.uint8, device=dev)
    wpk = ops.packed_filter(cd, wt.float().to(dev), ops.PACK_C3, 32)
    L.check(L.lib().fsr_conv3x3_c3_fwd(cd.code, imgd.data_ptr(), *imgd.stride(), n, h, w, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, wpk.data_ptr(),
                                       biasd.data_ptr(), L.ACT_LEAKY, 0.25, None, cout, out.data_ptr(), None, signs.data_ptr(),
                                       ops._stream()), "fsr_conv3x3_c3_fwd")
    got = _nchw(out, cd)
    exact("x3 first layer", got, ref)
    assert torch.equal(signs.cpu(), _sign_bytes(got > 0))


@pytest.mark.parametrize("backend,cin,cus", _cases(
    emu=[(64, 1)],
    hip=[(c, k) for c in (64, 128) for k in (1, 2)]))
def test_x3_stride2_data_gradient_gated_by_sign_bits(backend, cin, cus, monkeypatch):
    """conv3x3_raw(mode=CONV_DGRAD, stride=2) in x3, `cin` dx channels, dx 37 x 46 (ragged against the 8 x 16 dy tiles), gated by
    the saved tensor and by its sign bytes: the same bits on the raw storage, and exact.  FSR_PERSIST_CUS = 1 and 2: every
    workgroup walks several tiles."""
    dev = select(backend)
    big = dev.type == "cuda"
    monkeypatch.setenv("FSR_PERSIST_CUS", str(cus))
    cd = ops.Compute("x3")
    g = _gen(72)
    n, h, w = (2, 37, 46) if big else (1, 19, 22)
    x, wt = ints(g, (n, cin, h, w)), pm1(g, 64, cin)          # x: the producing layer's output, i.e. the mask
    gy = ints(g, (n, 64, (h - 1) // 2 + 1, (w - 1) // 2 + 1))
    dx_ref, _ = _grads(x, wt, gy, 2)
    premise16(FAM, x, wt, gy, dx_ref)
    want = dx_ref * gate(x, 0.25)
    wpk = ops.packed_filter(cd, wt.float().to(dev), L.PACK_DGRAD, 64)
    gd, xd = _nhwc(gy, cd, dev), _nhwc(x, cd, dev)
    signs = _sign_bytes(x > 0).to(dev)
    d0, _, _ = ops.conv3x3_raw(cd, gd, wpk, cin, mode=L.CONV_DGRAD, out_hw=(h, w), stride=2, dact_mask=xd, dact_slope=0.25)
    assert _kernel(FAM, ".tensor.%d" % cin).startswith("conv_s2d3_kernel"), ops._last_kernel()
    d1, _, _ = ops.conv3x3_raw(cd, gd, wpk, cin, mode=L.CONV_DGRAD, out_hw=(h, w), stride=2, dact_mask=signs, dact_slope=0.25, dact_bits=True)
    assert _kernel(FAM, ".bits.%d" % cin).startswith("conv_s2d3_kernel"), ops._last_kernel()
    assert torch.equal(d0, d1), "gated by the bits differs from gated by the tensor"
    exact("gated by the tensor", _nchw(d0, cd), want)
    exact("gated by the sign bits", _nchw(d1, cd), want)


@pytest.mark.parametrize("backend", _cases(emu=[()], hip=[()]))
def test_x3_neck_and_block0_through_autograd_with_and_without_sign_bits(backend, monkeypatch):
    """The discriminator's neck and first stride-2 block (its _cfg_neck, _cfg_s0) in x3 through autograd, ops.USE_SIGN_BITS on
    and off: image gradient, weight and bias gradients are the same bits, and with the switch on the mask the stride-2 data
    gradient gets is the uint8 tensor."""
    import importlib
    model = importlib.import_module("fast-srgan_amd.model")
    dev = select(backend)
    big = dev.type == "cuda"
    monkeypatch.setenv("FSR_PERSIST_CUS", "2" if big else "1")
    g = _gen(73)
    n, h, w = (2, 37, 46) if big else (1, 19, 22)
    torch.manual_seed(73)
    D = model.Discriminator(types.SimpleNamespace(n_filters=64, n_layers=7), "x3")
    cd = D.compute
    assert cd.x3
    img = ints(g, (n, 3, h, w)).float().to(dev)
    wn, bn, w0 = (pm1(g, 64, 3).float().to(dev), ibias(g, 64).float().to(dev), pm1(g, 64, 64).float().to(dev))
    gu = _nhwc(ints(g, (n, 64, (h - 1) // 2 + 1, (w - 1) // 2 + 1)), cd, dev)
    masks = []
    raw = ops.conv3x3_raw

    def spy(cd_, x, wpk, cout, **kw):
        if kw.get("mode") == L.CONV_DGRAD and kw.get("stride") == 2:
            masks.append((kw["dact_mask"].dtype, bool(kw.get("dact_bits"))))
        return raw(cd_, x, wpk, cout, **kw)

    monkeypatch.setattr(ops, "conv3x3_raw", spy)

    def run(bits):
        monkeypatch.setattr(ops, "USE_SIGN_BITS", bits)
        x = img.clone().requires_grad_(True)
        p = [t.clone().requires_grad_(True) for t in (wn, bn, w0)]
        y, _ = ops.conv3x3(x, p[0], p[1], None, D._cfg_neck)
        u, _ = ops.conv3x3(y, p[2], None, None, D._cfg_s0)
        u.backward(gu)
        return [x.grad] + [t.grad for t in p]

    off = run(False)
    assert masks == [(cd.torch_dtype, False)], masks
    on = run(True)
    assert masks[1:] == [(torch.uint8, True)], masks
    assert ops._last_kernel() != "?"
    for what, a, b in zip(("image gradient", "neck weight gradient", "neck bias gradient", "block-0 weight gradient"), off, on):
        assert a is not None and b is not None and torch.equal(a, b), what
