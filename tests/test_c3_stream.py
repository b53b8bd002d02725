"""Integer-exact cases of the first-layer kernels (csrc/conv_c3.hip) that the pipelined weight-gradient tile loop can get wrong,
next to test_exact.py's single-tile-per-slab shapes: slabs of several tiles (the prefetch of tile i + 1 under the MFMAs of tile i,
the LDS image overwritten between two barriers), a short last slab, one-tile slabs (nothing to prefetch), the role-swapped form
of the generator head, accumulation into pre-filled arenas and the bias gradient from the column of ones.  Forward cases at a
ragged 17 x 35 map ride along: every storage type, channel blocks 16 / 32 / 128, LeakyReLU(0.2) with sign bytes, PReLU with the
pre-activation copy, scale and shift, a channels-last image.

Inputs are test_exact.py's small integers, so f32 accumulation is exact in any order and there is no tolerance.  LeakyReLU(0.2)
is not a power of two: its reference is the kernel's own single f32 product float32(0.2) * z (z an exact integer), rounded to the
storage type by the storage codec (ops.to_storage), which is bit-exact as well."""
import pytest
import torch
import torch.nn.functional as F

from backend import L, ops, select
from test_exact import F64, _C3_SCALE, _C3_SHIFT, _c3_image, _cases, _gen, _grads, _nchw, _nhwc, _wgrad_bound, exact, exact32, ibias, ints, pm1, \
    premise16, premise_sum

FAM = "c3_stream"


# ------------------------------------------------------------------------------------------------- weight gradient
def _c3_wgrad(cd, dev, img, strides, n, h, w, dz, cout, dw, dbias, transposed, scale=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.0)):
    lib = L.lib()
    ws = ops._workspace(lib.fsr_conv3x3_c3_wgrad_workspace(n, h, w, cout), dev)
    L.check(lib.fsr_conv3x3_c3_wgrad(cd.code, img.data_ptr(), *strides, n, h, w, *scale, *shift, dz.data_ptr(), cout, dw.data_ptr(), ops._p(dbias),
                                     ws.data_ptr(), transposed, ops._stream()), "fsr_conv3x3_c3_wgrad")


def _slabs(n, h, w):
    """(tiles, tiles per slab, slabs) of c3_wgrad_slabs (8 x 16 tiles, at most 1024 slabs)."""
    tiles = ((w + 15) // 16) * ((h + 7) // 8) * n
    per = -(-tiles // min(1024, tiles))
    return tiles, per, -(-tiles // per)


# (n, h, w): 2,178 tiles = 726 slabs of three | 1,309 tiles = 654 slabs of two and a last slab of ONE | one tile per slab
_WG_BIG = [(9, 170, 170), (7, 130, 170), (1, 17, 35)]
_WG_PLAN = {(9, 170, 170): (2178, 3, 726), (7, 130, 170): (1309, 2, 655), (1, 17, 35): (9, 1, 9)}


def test_c3_wgrad_slab_plan_of_the_cases():
    """The cases below are what their comments say: several tiles per slab, a short last slab, one tile per slab."""
    for shape, plan in _WG_PLAN.items():
        assert _slabs(*shape) == plan
    tiles, per, slabs = _WG_PLAN[(7, 130, 170)]
    assert tiles - (slabs - 1) * per == 1


@pytest.mark.parametrize("backend,cdn,shape", _cases(
    emu=[("f32", (1, 17, 35)), ("bf16", (1, 17, 35))],
    hip=[(c, s) for c in ("x3", "f16") for s in _WG_BIG]))
def test_c3_wgrad_across_slabs(backend, cdn, shape):
    """fsr_conv3x3_c3_wgrad, 3 -> 64 with scale and shift, accumulating into pre-filled weight and bias arenas; the bias gradient
    is the column of ones (k = 27) of the same MFMAs."""
    dev = select(backend)
    cd = ops.Compute(cdn)
    g = _gen(51)
    n, h, w = shape
    imgf, xn = _c3_image(g, n, h, w, "nchw")
    dz = ints(g, (n, 64, h, w))
    _, dw_ref = _grads(xn, torch.zeros(64, 3, 3, 3, dtype=F64), dz, 1)
    premise16(FAM, xn, dz)
    premise_sum(FAM, _wgrad_bound(xn, dz) + 5.0)
    imgd = imgf.to(dev)
    dzd = ops._aligned(_nhwc(dz, cd, dev))
    dw = torch.full((64, 3, 3, 3), 5.0, dtype=torch.float32, device=dev)
    db = torch.full((64,), -4.0, dtype=torch.float32, device=dev)
    _c3_wgrad(cd, dev, imgd, imgd.stride(), n, h, w, dzd, 64, dw, db, 0, _C3_SCALE, _C3_SHIFT)
    exact32("weight gradient", dw, dw_ref + 5.0)
    exact32("bias gradient (column 27)", db, dz.sum((0, 2, 3)) - 4.0)


@pytest.mark.parametrize("backend,cdn,shape", _cases(
    emu=[("f32", (1, 17, 35))],
    hip=[(c, s) for c in ("x3", "f16") for s in ((9, 170, 170), (1, 17, 35))]))
def test_c3_wgrad_role_swapped_head(backend, cdn, shape):
    """transposed = 1, the generator head's weight gradient: the image operand is the NHWC 3-channel gradient of a 64 -> 3
    convolution, dz that convolution's 64-channel input; row co / column (tap, c3) lands at dW[c3][co][8 - tap]."""
    dev = select(backend)
    cd = ops.Compute(cdn)
    g = _gen(52)
    n, h, w = shape
    x, g3 = ints(g, (n, 64, h, w)), ints(g, (n, 3, h, w))
    _, dw_ref = _grads(x, torch.zeros(3, 64, 3, 3, dtype=F64), g3, 1)
    premise16(FAM, x, g3)
    premise_sum(FAM, _wgrad_bound(x, g3) + 7.0)
    g3d = g3.permute(0, 2, 3, 1).float().contiguous().to(dev)          # (n, h, w, 3) viewed as (N, 3, H, W)
    xd = ops._aligned(_nhwc(x, cd, dev))
    dw = torch.full((3, 64, 3, 3), 7.0, dtype=torch.float32, device=dev)
    _c3_wgrad(cd, dev, g3d, (h * w * 3, 1, w * 3, 3), n, h, w, xd, 64, dw, None, 1)
    exact32("head weight gradient (roles swapped)", dw, dw_ref + 7.0)


# ------------------------------------------------------------------------------------------------- forward
def _round_to_storage(cd, ref_nchw32):
    """float32 NCHW values -> what a tensor of compute mode cd holds of them, as float64 NCHW."""
    t = ref_nchw32.permute(0, 2, 3, 1).contiguous()
    return ops.from_storage(cd, ops.to_storage(cd, t)).permute(0, 3, 1, 2).double()


def _leaky02(z):
    """The kernel's LeakyReLU(0.2) of an exact integer z: one f32 product."""
    z32 = z.float()
    return torch.where(z32 > 0, z32, z32 * torch.tensor(0.2, dtype=torch.float32))


_FWD_VARIANTS = ("leaky", "prelu_preact", "scale_shift", "nhwc")


@pytest.mark.parametrize("backend,cdn,cout,variant", _cases(
    emu=[("f32", 64, "leaky"), ("bf16", 64, "prelu_preact"), ("bf16", 16, "leaky"), ("f32", 64, "nhwc")],
    hip=[(c, 64, v) for c in ("x3", "f16", "bf16", "f32") for v in _FWD_VARIANTS] +
        [(c, co, "leaky") for c in ("x3", "f16", "bf16", "f32") for co in (16, 32, 128) if not (c == "x3" and co == 16)]))
def test_c3_forward_ragged_tiles(backend, cdn, cout, variant):
    """fsr_conv3x3_c3_fwd on N = 3, 17 x 35 (six 16 x 16 tiles per image, ragged both ways): bias + LeakyReLU(0.2) with the sign
    bytes of the 16-bit forms checked against out > 0; PReLU(-0.25) with the pre-activation copy; per-channel scale and shift;
    a channels-last image; the narrow (16), x3-minimum (32) and two-block (128) channel counts.  (The forward kept its one
    workgroup per tile -- a persistent walk measured slower, docs/HISTORY.md -- so there is no grid to shrink.)"""
    dev = select(backend)
    cd = ops.Compute(cdn)
    g = _gen(53)
    n, h, w = 3, 17, 35
    imgf, xn_scaled = _c3_image(g, n, h, w, "nhwc" if variant == "nhwc" else "nchw")
    scaled = variant == "scale_shift"
    xn = xn_scaled if scaled else imgf.double()
    wt, bias = pm1(g, cout, 3), ibias(g, cout)
    z = F.conv2d(xn, wt, bias, 1, 1)
    premise16(FAM, xn, z)
    prelu = variant == "prelu_preact"
    ref = F.prelu(z, torch.tensor([-0.25], dtype=F64)) if prelu else _round_to_storage(cd, _leaky02(z))
    imgd, biasd = imgf.to(dev), bias.float().to(dev)
    out = ops._empty((n, h, w, cout), cd.torch_dtype, dev)
    pre = ops._empty_like(out) if prelu else None
    want_signs = cd.is16 and cout % 64 == 0 and not prelu
    signs = torch.zeros((n, h, w, cout // 8), dtype=torch.uint8, device=dev) if want_signs else None
    a = torch.tensor([-0.25]).to(dev) if prelu else None
    wpk = ops.packed_filter(cd, wt.float().to(dev), ops.PACK_C3, 32)
    scale, shift = (_C3_SCALE, _C3_SHIFT) if scaled else ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    L.check(L.lib().fsr_conv3x3_c3_fwd(cd.code, imgd.data_ptr(), *imgd.stride(), n, h, w, *scale, *shift, wpk.data_ptr(), biasd.data_ptr(),
                                       L.ACT_PRELU if prelu else L.ACT_LEAKY, 0.2, ops._p(a), cout, out.data_ptr(), ops._p(pre), ops._p(signs),
                                       ops._stream()), "fsr_conv3x3_c3_fwd")
    exact("first layer forward", _nchw(out, cd), ref)
    if pre is not None:
        exact("pre-activation copy", _nchw(pre, cd), z)
    if signs is not None:
        pos = (ref > 0).permute(0, 2, 3, 1)
        want = torch.zeros((n, h, w, cout // 8), dtype=torch.uint8)
        for c in range(cout):
            want[..., c >> 3] |= pos[..., c].to(torch.uint8) << (c & 7)
        assert torch.equal(signs.cpu(), want)
