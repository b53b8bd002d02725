"""Integer-exact parity of the 3x3 convolution kernels (and three small relatives) against float64.

The operator tests in test_ops.py / test_x3.py draw randn inputs and gate on max-error / tensor-max at 1e-2 .. 1e-3: bounds that
exist to absorb bf16 rounding and that absorb a one-element indexing error (a dropped halo tap at a tile seam, one pixel left out
of a statistics slot or of a weight gradient's reduction) just as well -- test_exact_gate_is_sharper_than_the_tolerance_gates
below shows both.  Here every operand is a SMALL INTEGER: activations and incoming gradients in [-2, 2], filters +-1 at density
36 / (9 cin), biases in [-3, 3], masks in [-2, 2] (zeros included), every slope a power of two.  Then every product and every
partial sum is an integer (or an integer times a power of two) far below 2^24, f32 accumulation is exact in ANY order, and a
bf16, f16, f32 or x3 kernel has to reproduce the float64 reference bit for bit.  There is no tolerance in this file.

The premise is asserted on the float64 reference before a kernel's result is looked at:
  * max |value| <= 256 for everything stored in 16 bits (bf16 holds the integers up to 256; the same bound serves f16);
  * every sum of magnitudes of a statistics / gradient reduction < 2^24.
A premise failure is a bug in the test's inputs (lower the density), never a reason to skip.  The measured maxima go to the
parity-error log that backend.report appends to, so the margin to 256 and 2^24 can be read there, as do the kernel names the
cases reached.  A mismatch message lists the first mismatching (n, c, y, x) and the counts per 16-row / 16-column tile."""
import types

import pytest
import torch
import torch.nn.functional as F

from backend import L, ops, relerr, report, select

F64 = torch.float64
LIM16 = 256.0            # integers a bf16 value holds exactly
LIM_SUM = float(1 << 24)   # integers an f32 accumulator holds exactly
GPU = pytest.mark.gpu


def _cases(emu, hip):
    """Parameter list (backend, *case): the emulator leg runs a trimmed list of CASES (same shapes), the MI355X leg the full cross."""
    return [pytest.param("emu", *c) for c in emu] + [pytest.param("hip", *c, marks=GPU) for c in hip]


# ------------------------------------------------------------------------------------------------- generators
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, shape, lo=-2, hi=2):
    """Integer-valued float64 tensor, uniform in [lo, hi]: activations, incoming gradients, masks, image planes."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(F64)


def pm1(g, cout, cin, k=3, density=None):
    """Filter of +-1 entries at density 36 / (9 cin): 36 taps per output whatever cin is, so the output range does not grow.
    (`density`: for the 3-channel ends, whose DATA gradient sums over 9 cout taps.)"""
    density = min(1.0, 36.0 / (k * k * cin)) if density is None else density
    sign = torch.randint(0, 2, (cout, cin, k, k), generator=g).to(F64) * 2 - 1
    keep = (torch.rand((cout, cin, k, k), generator=g) < density).to(F64)
    return sign * keep


def ibias(g, c):
    return ints(g, (c,), -3, 3)


def gate(mask, slope):
    """The activation-gradient factor of a fused mask: 1 where mask > 0, else the (power-of-two) slope."""
    return torch.where(mask > 0, torch.ones_like(mask), torch.full_like(mask, slope))


# ------------------------------------------------------------------------------------------------- premise + comparison
_maxima = {}


def _note(family, what, value):
    key = "exact.%s.%s" % (family, what)
    if value > _maxima.get(key, -1.0):
        _maxima[key] = value
        report(key, value)


def premise16(family, *tensors):
    """Every tensor that a kernel reads or writes in 16 bits holds integers (times a power of two) of magnitude <= 256."""
    m = max(float(t.abs().max()) for t in tensors)
    _note(family, "max_abs_ref", m)
    assert m <= LIM16, "premise (input bug, lower the density): |reference| reaches %g > 256" % m


def premise_sum(family, *sums):
    """`sums`: upper bounds (tensors or numbers) of the sums of magnitudes an f32 reduction adds up."""
    m = max(float(s.abs().max()) if torch.is_tensor(s) else float(s) for s in sums)
    _note(family, "max_reduction_sum", m)
    assert m < LIM_SUM, "premise (input bug, lower the density): a reduction reaches %g >= 2^24" % m


def _where(got, ref):
    """Mismatch pattern of an NCHW (or any) tensor: the first indices and the counts per 16 x 16 tile row / column."""
    bad = (got != ref).nonzero()
    msg = "%d of %d differ; first (index: got, want): %s" % (len(bad), ref.numel(), [
        (tuple(int(v) for v in i), float(got[tuple(i)]), float(ref[tuple(i)])) for i in bad[:6]])
    if ref.dim() == 4 and len(bad):
        rows = torch.bincount(bad[:, 2] // 16).tolist()
        cols = torch.bincount(bad[:, 3] // 16).tolist()
        chans = sorted(set(int(c) for c in bad[:, 1]))[:16]
        msg += "; per tile row (y // 16) %s, per tile column (x // 16) %s, y %% 16 %s, x %% 16 %s, channels %s" % (
            rows, cols, sorted(set(int(v) % 16 for v in bad[:, 2])), sorted(set(int(v) % 16 for v in bad[:, 3])), chans)
    return msg


def exact(what, got, ref):
    """THE comparison of this file: torch.equal on float64 values."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.equal(got, ref), "%s: %s" % (what, _where(got, ref))


def exact32(what, got, ref64):
    """Statistics and weight gradients are f32 results: the float64 reference is cast to float32."""
    exact(what, got, ref64.float())


def _kernel(family, tag=""):
    name = ops._last_kernel()
    report("exact.%s.kernel%s %s" % (family, tag, name), 0.0)
    return name


# ------------------------------------------------------------------------------------------------- layout helpers
def _nhwc(x, cd, dev, pad_to=None):
    """float64 NCHW -> the NHWC storage tensor of compute mode `cd` (channels zero-padded to `pad_to`)."""
    t = x.permute(0, 2, 3, 1).float()
    if pad_to is not None and pad_to > t.shape[3]:
        t = F.pad(t, (0, pad_to - t.shape[3]))
    return ops.to_storage(cd, t.contiguous()).to(dev)


def _nchw(y, cd, plain=False):
    v = y.detach().cpu()
    v = v.float() if (plain or not cd.x3) else ops.from_storage(cd, v)
    return v.permute(0, 3, 1, 2).double()


def _grads(x, wt, g, stride, ps=False):
    """float64 data and weight gradient of conv2d(k=3, p=1) [+ PixelShuffle] for the cotangent g, by autograd."""
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, None, stride, 1)
    (F.pixel_shuffle(y, 2) if ps else y).backward(g)
    return xr.grad, wr.grad


def premise_stats(family, ref):
    """The statistics reductions of the pre-activation `ref`: sum |y| and sum y^2 per (image, channel) stay below 2^24."""
    premise_sum(family, ref.abs().sum((2, 3)), (ref * ref).sum((2, 3)))


def _check_stats(what, stats, ref):
    """Sum and sum of squares per (image, channel) of the pre-activation `ref`."""
    s = stats.cpu()
    exact32(what + " sum(y)", s[..., 0], ref.sum((2, 3)))
    exact32(what + " sum(y^2)", s[..., 1], (ref * ref).sum((2, 3)))


def _wgrad_bound(x, g):
    """Upper bound of sum |x| |g| over the K = n oh ow pixels of a weight gradient's reduction."""
    return float(x.abs().max()) * float(g.abs().max()) * g.shape[0] * g.shape[2] * g.shape[3]


# ------------------------------------------------------------------------------------------------- conv_igemm
_IGEMM_ROWS = [(1, 32, 64, False), (2, 64, 128, False), (1, 32, 128, True), (1, 64, 3, False)]


@pytest.mark.parametrize("backend,cdn,stride,cin,cout,ps", _cases(
    emu=[(c,) + r for i, r in enumerate(_IGEMM_ROWS) for c in ("f32", ("bf16", "f16")[i % 2])],
    hip=[(c,) + r for c in ("f32", "bf16", "f16") for r in _IGEMM_ROWS]))
def test_exact_conv_igemm(backend, cdn, stride, cin, cout, ps):
    """Forward with bias (+ statistics), data gradient and weight gradient of the generic implicit-GEMM kernel."""
    dev = select(backend)
    fam = "igemm"
    cd = ops.Compute(cdn)
    g = _gen(1)
    n, h, w = (3, 37, 45) if dev.type == "cuda" else (1, 7, 19)
    x, wt, bias = ints(g, (n, cin, h, w)), pm1(g, cout, cin), ibias(g, cout)
    ref = F.conv2d(x, wt, bias, stride, 1)
    refo = F.pixel_shuffle(ref, 2) if ps else ref
    gy = ints(g, refo.shape)
    dx_ref, dw_ref = _grads(x, wt, gy, stride, ps)
    premise16(fam, x, wt, refo, gy, dx_ref)
    premise_sum(fam, _wgrad_bound(x, gy))
    premise_stats(fam, ref)
    want_stats = not ps and cout % 16 == 0
    xd = _nhwc(x, cd, dev)
    wpk = ops.packed_filter(cd, wt.float().to(dev), L.PACK_FWD_PS if ps else L.PACK_FWD, cin)
    y, _, stats = ops.conv3x3_raw(cd, xd, wpk, cout, stride=stride, bias=bias.float().to(dev), pixel_shuffle=ps, want_stats=want_stats,
                                  out_f32=(cout == 3))
    _kernel(fam, ".fwd.%s.s%d.%d-%d%s" % (cdn, stride, cin, cout, ".ps" if ps else ""))
    exact("forward", _nchw(y, cd, plain=(cout == 3)), refo)
    if want_stats:
        _check_stats("statistics", stats, ref)
    cpad_out = cd.pad(cout)
    gd = _nhwc(gy, cd, dev, pad_to=(cpad_out // 4) if ps else cpad_out)
    wpk_d = ops.packed_filter(cd, wt.float().to(dev), L.PACK_DGRAD_PS if ps else L.PACK_DGRAD, cpad_out)
    dx, _, _ = ops.conv3x3_raw(cd, gd, wpk_d, cin, mode=L.CONV_DGRAD, out_hw=(h, w), stride=stride, in_pixel_shuffled=ps)
    _kernel(fam, ".dgrad.%s.s%d.%d-%d%s" % (cdn, stride, cin, cout, ".ps" if ps else ""))
    exact("data gradient", _nchw(dx, cd), dx_ref)
    dw = ops.conv3x3_wgrad_raw(cd, xd, gd, cout, cin, stride, dy_pixel_shuffled=ps)
    exact32("weight gradient", dw, dw_ref)


# ------------------------------------------------------------------------------------------------- conv64_v2 / conv64_s2fwd
_P64_SHAPES = [(1, 5, 7), (2, 17, 33), (4, 8, 40)]


@pytest.mark.parametrize("backend,cdn,cus,shape", _cases(
    emu=[("bf16", 1, _P64_SHAPES[0]), ("f16", 3, _P64_SHAPES[1]), ("bf16", 256, _P64_SHAPES[2])],
    hip=[(c, u, s) for c in ("bf16", "f16") for u in (1, 3, 256) for s in _P64_SHAPES]))
def test_exact_conv64_v2_epilogues(backend, cdn, cus, shape, monkeypatch):
    """Every epilogue of the persistent 64-input-channel kernel on ragged / sub-tile maps with one, a few and more tile ranges
    than tiles: bias + LeakyReLU + pre-activation copy, statistics, mask, skip addend, fused max-pool, PixelShuffle + PReLU."""
    dev = select(backend)
    monkeypatch.setenv("FSR_PERSIST_CUS", str(cus))
    fam = "conv64_v2"
    cd = ops.Compute(cdn)
    g = _gen(21)
    n, h, w = shape
    x = ints(g, (n, 64, h, w))
    xd = _nhwc(x, cd, dev)

    def v2(tag):
        name = _kernel(fam, ".%s.%s" % (tag, cdn))
        assert name.startswith("conv64_v2_kernel"), name

    for cout in (64, 128):
        wt, bias = pm1(g, cout, 64), ibias(g, cout)
        mask = ints(g, (n, cout, h, w))
        ref = F.conv2d(x, wt, bias, 1, 1)
        raw = F.conv2d(x, wt, None, 1, 1)
        premise16(fam, x, wt, ref, raw, raw + mask)        # (the addend case: the SUM is what gets stored)
        premise_stats(fam, ref)
        wpk = ops.packed_filter(cd, wt.float().to(dev), L.PACK_FWD, 64)
        bd = bias.float().to(dev)
        y, pre, _ = ops.conv3x3_raw(cd, xd, wpk, cout, bias=bd, act=L.ACT_LEAKY, slope=0.25, want_preact=True)
        v2("leaky_preact")
        exact("pre-activation copy", _nchw(pre, cd), ref)
        exact("bias + LeakyReLU", _nchw(y, cd), F.leaky_relu(ref, 0.25))
        y, _, stats = ops.conv3x3_raw(cd, xd, wpk, cout, bias=bd, want_stats=True)
        v2("stats")
        exact("forward (statistics launch)", _nchw(y, cd), ref)
        _check_stats("statistics", stats, ref)
        md = _nhwc(mask, cd, dev)
        y, _, _ = ops.conv3x3_raw(cd, xd, wpk, cout, dact_mask=md, dact_slope=0.5)
        v2("mask")
        exact("masked", _nchw(y, cd), raw * gate(mask, 0.5))
        y, _, _ = ops.conv3x3_raw(cd, xd, wpk, cout, dact_mask=md, dact_add=True)
        v2("addend")
        exact("skip addend", _nchw(y, cd), raw + mask)
        if h % 2 == 0 and w % 2 == 0:
            y, _, _ = ops.conv3x3_raw(cd, xd, wpk, cout, bias=bd, act=L.ACT_RELU, pool2=True)
            v2("pool")
            exact("ReLU + max-pool", _nchw(y, cd), F.max_pool2d(F.relu(ref), 2))
    wt, bias = pm1(g, 256, 64), ibias(g, 256)
    shuffled = F.pixel_shuffle(F.conv2d(x, wt, bias, 1, 1), 2)
    premise16(fam, shuffled)
    wpk = ops.packed_filter(cd, wt.float().to(dev), L.PACK_FWD_PS, 64)
    y, pre, _ = ops.conv3x3_raw(cd, xd, wpk, 256, bias=bias.float().to(dev), pixel_shuffle=True, act=L.ACT_PRELU,
                                prelu=torch.tensor([-0.25]).to(dev), want_preact=True)
    v2("ps_prelu_preact")
    exact("PixelShuffle pre-activation copy", _nchw(pre, cd), shuffled)
    exact("PixelShuffle + PReLU", _nchw(y, cd), F.prelu(shuffled, torch.tensor([-0.25], dtype=F64)))


@pytest.mark.parametrize("backend,cdn,cus,shape", _cases(
    emu=[(("bf16", "f16")[(i + j) % 2], u, s) for i, u in enumerate((1, 3, 256)) for j, s in enumerate(_P64_SHAPES)],
    hip=[(c, u, s) for c in ("bf16", "f16") for u in (1, 3, 256) for s in _P64_SHAPES]))
def test_exact_conv64_s2fwd(backend, cdn, cus, shape, monkeypatch):
    """The persistent 64 -> 64 stride-2 forward: output, statistics, LeakyReLU + pre-activation copy on odd / even / sub-tile maps."""
    dev = select(backend)
    monkeypatch.setenv("FSR_PERSIST_CUS", str(cus))
    fam = "conv64_s2fwd"
    cd = ops.Compute(cdn)
    g = _gen(31)
    n, h, w = shape
    x, wt, bias = ints(g, (n, 64, h, w)), pm1(g, 64, 64), ibias(g, 64)
    ref = F.conv2d(x, wt, bias, 2, 1)
    premise16(fam, x, wt, ref)
    premise_stats(fam, ref)
    xd = _nhwc(x, cd, dev)
    wpk = ops.packed_filter(cd, wt.float().to(dev), L.PACK_FWD, 64)
    y, _, stats = ops.conv3x3_raw(cd, xd, wpk, 64, stride=2, bias=bias.float().to(dev), want_stats=True)
    assert _kernel(fam, "." + cdn) == "conv64_s2fwd_kernel"
    exact("forward", _nchw(y, cd), ref)
    _check_stats("statistics", stats, ref)
    y, pre, _ = ops.conv3x3_raw(cd, xd, wpk, 64, stride=2, bias=bias.float().to(dev), act=L.ACT_LEAKY, slope=0.5, want_preact=True)
    assert ops._last_kernel() == "conv64_s2fwd_kernel"
    exact("pre-activation copy", _nchw(pre, cd), ref)
    exact("bias + LeakyReLU", _nchw(y, cd), F.leaky_relu(ref, 0.5))


# ------------------------------------------------------------------------------------------------- conv_tall3, stride 1
_T3_ALL = ("plain", "pool", "dgrad", "mask", "stats", "into64")


@pytest.mark.parametrize("backend,cdn,cin,cout,rows,parts", _cases(
    emu=[(("bf16", "f16")[(i + j) % 2], ci, co, r, _T3_ALL) for i, (ci, co) in enumerate(((128, 128), (160, 256), (128, 64)))
         for j, r in enumerate((8, 12, 16))],
    hip=[(c, ci, co, r, _T3_ALL) for c in ("bf16", "f16") for (ci, co) in ((128, 128), (160, 256), (128, 64)) for r in (8, 12, 16)]))
def test_exact_conv_tall3(backend, cdn, cin, cout, rows, parts, monkeypatch):
    """conv_tall3 (128- and 64-channel blocks; 8-, 12- and 16-row tiles; more tiles than workgroups): bias + ReLU, the fused
    max-pool, the data gradient with and without the fused mask, the statistics instantiation, and (cout = 64) the data
    gradient of a 64 -> 128 layer INTO 64 channels."""
    dev = select(backend)
    big = dev.type == "cuda"
    monkeypatch.setenv("FSR_PERSIST_CUS", "3" if big else "1")
    monkeypatch.setenv("FSR_T3_ROWS", str(rows))
    fam = "conv_tall3"
    cd = ops.Compute(cdn)
    g = _gen(11)
    n, h, w = (3, 50, 44) if big else (1, 18, 20)
    x, wt, bias = ints(g, (n, cin, h, w)), pm1(g, cout, cin), ibias(g, cout)
    pre = F.conv2d(x, wt, bias, 1, 1)
    premise16(fam, x, wt, pre)
    premise_stats(fam, pre)
    xd = _nhwc(x, cd, dev)
    wpk = ops.packed_filter(cd, wt.float().to(dev), L.PACK_FWD, cin)
    bd = bias.float().to(dev)
    tag = ".%s.%d-%d.r%d" % (cdn, cin, cout, rows)
    for pool in (False, True):
        if ("pool" if pool else "plain") not in parts:
            continue
        y, _, _ = ops.conv3x3_raw(cd, xd, wpk, cout, bias=bd, act=L.ACT_RELU, pool2=pool)
        name = _kernel(fam, (".pool" if pool else ".plain") + tag)
        if not (pool and cout % 128):          # (no fused max-pool on the 64-channel block: that launch is conv_igemm's)
            assert name.startswith("conv_tall3_kernel<%s" % cdn), name
        exact("ReLU + max-pool" if pool else "bias + ReLU", _nchw(y, cd), F.max_pool2d(F.relu(pre), 2) if pool else F.relu(pre))
    if "dgrad" in parts or "mask" in parts:
        gy, mask = ints(g, (n, cout, h, w)), ints(g, (n, cin, h, w))
        dx_ref, _ = _grads(x, wt, gy, 1)
        premise16(fam, gy, dx_ref)
        gd = _nhwc(gy, cd, dev)
        wpk_d = ops.packed_filter(cd, wt.float().to(dev), L.PACK_DGRAD, cout)
        for masked in (False, True):
            if ("mask" if masked else "dgrad") not in parts:
                continue
            dx, _, _ = ops.conv3x3_raw(cd, gd, wpk_d, cin, mode=L.CONV_DGRAD, out_hw=(h, w),
                                       dact_mask=_nhwc(mask, cd, dev) if masked else None, dact_slope=0.25)
            name = _kernel(fam, (".dgrad_mask" if masked else ".dgrad") + tag)
            if cin % 128 == 0 and cout >= 128:
                assert name.startswith("conv_tall3_kernel<%s" % cdn), name
            exact("masked data gradient" if masked else "data gradient", _nchw(dx, cd), dx_ref * gate(mask, 0.25) if masked else dx_ref)
    if "stats" in parts:
        y, _, stats = ops.conv3x3_raw(cd, xd, wpk, cout, bias=bd, act=L.ACT_LEAKY, slope=0.25, want_stats=True)
        name = _kernel(fam, ".stats" + tag)
        if cout % 128 == 0:
            assert name.startswith("conv_tall3_kernel<%s" % cdn) and "stats" in name, name
        exact("LeakyReLU (statistics launch)", _nchw(y, cd), F.leaky_relu(pre, 0.25))
        _check_stats("statistics", stats, pre)
    if "into64" in parts and cout == 64:
        # the data gradient of a 64 -> 128 layer: 128 gradient channels in, 64 out, with the fused mask
        w2, g2, m2 = pm1(g, 128, 64), ints(g, (n, 128, h, w)), ints(g, (n, 64, h, w))
        x2 = ints(g, (n, 64, h, w))
        dx_ref, _ = _grads(x2, w2, g2, 1)
        premise16(fam, dx_ref)
        wpk_d = ops.packed_filter(cd, w2.float().to(dev), L.PACK_DGRAD, 128)
        dx, _, _ = ops.conv3x3_raw(cd, _nhwc(g2, cd, dev), wpk_d, 64, mode=L.CONV_DGRAD, out_hw=(h, w), dact_mask=_nhwc(m2, cd, dev), dact_slope=0.5)
        name = _kernel(fam, ".into64" + tag)
        assert name.startswith("conv_tall3_kernel<%s,64,4,1,4,%d,1>" % (cdn, rows // 4)), name
        exact("masked data gradient into 64 channels", _nchw(dx, cd), dx_ref * gate(m2, 0.5))


# ------------------------------------------------------------------------------------------------- conv_tall3 stride 2, conv_s2d3
_S2F_ROWS = [(128, 128, (19, 22)), (160, 256, (32, 47)), (128, 128, (48, 32)), (128, 256, (17, 33))]
_S2D_ROWS = [(128, 128, (19, 22)), (128, 160, (32, 47)), (192, 128, (48, 32)), (128, 128, (17, 33))]


def _s2_shape(dev, hw):
    return (3,) + tuple(hw) if dev.type == "cuda" else (1, min(hw[0], 19), min(hw[1], 22))


@pytest.mark.parametrize("backend,cdn,cin,cout,hw", _cases(
    emu=[(("bf16", "f16")[i % 2],) + r for i, r in enumerate(_S2F_ROWS)],
    hip=[(c,) + r for c in ("bf16", "f16") for r in _S2F_ROWS]))
def test_exact_conv_tall3_stride2_forward(backend, cdn, cin, cout, hw, monkeypatch):
    """conv_tall3 S = 2 (four parity planes per tile window): the statistics instantiation and bias + mask + LeakyReLU, odd and
    even extents, more tiles than workgroups."""
    dev = select(backend)
    monkeypatch.setenv("FSR_PERSIST_CUS", "3" if dev.type == "cuda" else "1")
    fam = "conv_tall3_s2"
    cd = ops.Compute(cdn)
    g = _gen(12)
    n, h, w = _s2_shape(dev, hw)
    x, wt, bias = ints(g, (n, cin, h, w)), pm1(g, cout, cin), ibias(g, cout)
    raw, pre = F.conv2d(x, wt, None, 2, 1), F.conv2d(x, wt, bias, 2, 1)
    mask = ints(g, raw.shape)
    premise16(fam, x, wt, raw, pre)
    premise_stats(fam, raw)
    xd = _nhwc(x, cd, dev)
    wpk = ops.packed_filter(cd, wt.float().to(dev), L.PACK_FWD, cin)
    y, _, stats = ops.conv3x3_raw(cd, xd, wpk, cout, stride=2, want_stats=True)
    name = _kernel(fam, ".stats.%s.%d-%d" % (cdn, cin, cout))
    assert name.startswith("conv_tall3_kernel<%s" % cdn) and "stats,s2" in name, name
    exact("forward (statistics launch)", _nchw(y, cd), raw)
    _check_stats("statistics", stats, raw)
    y, _, _ = ops.conv3x3_raw(cd, xd, wpk, cout, stride=2, bias=bias.float().to(dev), act=L.ACT_LEAKY, slope=0.25,
                              dact_mask=_nhwc(mask, cd, dev), dact_slope=0.5)
    name = _kernel(fam, ".mask.%s.%d-%d" % (cdn, cin, cout))
    assert name.startswith("conv_tall3_kernel<%s" % cdn) and ",s2>" in name, name
    exact("bias + mask + LeakyReLU", _nchw(y, cd), F.leaky_relu(pre * gate(mask, 0.5), 0.25))


@pytest.mark.parametrize("backend,cdn,cin,cout,hw", _cases(
    emu=[(("f16", "bf16")[i % 2],) + r for i, r in enumerate(_S2D_ROWS)],
    hip=[(c,) + r for c in ("bf16", "f16") for r in _S2D_ROWS]))
def test_exact_conv_s2d3_stride2_data_gradient(backend, cdn, cin, cout, hw, monkeypatch):
    """conv_s2d3 (all four parity classes from one dy halo; two and three 64-channel blocks): masked and unmasked."""
    dev = select(backend)
    monkeypatch.setenv("FSR_PERSIST_CUS", "3" if dev.type == "cuda" else "1")
    fam = "conv_s2d3"
    cd = ops.Compute(cdn)
    g = _gen(13)
    n, h, w = _s2_shape(dev, hw)
    x, wt = ints(g, (n, cin, h, w)), pm1(g, cout, cin)          # x: the forward input, i.e. the mask
    gy = ints(g, (n, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1))
    dx_ref, _ = _grads(x, wt, gy, 2)
    premise16(fam, x, wt, gy, dx_ref)
    wpk = ops.packed_filter(cd, wt.float().to(dev), L.PACK_DGRAD, cout)
    gd, xd = _nhwc(gy, cd, dev), _nhwc(x, cd, dev)
    for masked in (True, False):
        dx, _, _ = ops.conv3x3_raw(cd, gd, wpk, cin, mode=L.CONV_DGRAD, out_hw=(h, w), stride=2, dact_mask=xd if masked else None, dact_slope=0.25)
        name = _kernel(fam, ".%s.%d-%d" % (cdn, cin, cout))
        assert name.startswith("conv_s2d3_kernel<%s>" % cdn), name
        exact("masked data gradient" if masked else "data gradient", _nchw(dx, cd), dx_ref * gate(x, 0.25) if masked else dx_ref)


@pytest.mark.parametrize("backend,cdn", _cases(emu=[("bf16",)], hip=[("bf16",), ("f16",)]))
def test_exact_sign_bit_mask_first_layer_to_stride2_data_gradient(backend, cdn, monkeypatch):
    """The first layer writes its LeakyReLU output and the output's sign bits; the 64 -> 64 stride-2 data gradient (conv_s2d3)
    gated by the bits and by the tensor, both exact."""
    dev = select(backend)
    big = dev.type == "cuda"
    monkeypatch.setenv("FSR_PERSIST_CUS", "2" if big else "1")
    fam = "sign_bits"
    cd = ops.Compute(cdn)
    g = _gen(17)
    n, h, w = (3, 37, 46) if big else (1, 19, 22)
    img, wn, bn = ints(g, (n, 3, h, w)), pm1(g, 64, 3), ibias(g, 64)
    ref = F.leaky_relu(F.conv2d(img, wn, bn, 1, 1), 0.25)
    premise16(fam, img, ref)
    imgd, bnd = img.float().to(dev), bn.float().to(dev)
    out = torch.empty((n, h, w, 64), dtype=cd.torch_dtype, device=dev)
    signs = torch.zeros((n, h, w, 8), dtype=torch.uint8, device=dev)
    wpk = ops.packed_filter(cd, wn.float().to(dev), ops.PACK_C3, 32)
    L.check(L.lib().fsr_conv3x3_c3_fwd(cd.code, imgd.data_ptr(), *imgd.stride(), n, h, w, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, wpk.data_ptr(),
                                       bnd.data_ptr(), L.ACT_LEAKY, 0.25, None, 64, out.data_ptr(), None, signs.data_ptr(),
                                       ops._stream()), "fsr_conv3x3_c3_fwd")
    exact("first layer", _nchw(out, cd), ref)
    want = torch.zeros((n, h, w, 8), dtype=torch.uint8)
    pos = (ref > 0).permute(0, 2, 3, 1)
    for c in range(64):
        want[..., c >> 3] |= (pos[..., c].to(torch.uint8) << (c & 7))
    assert torch.equal(signs.cpu(), want)
    wt = pm1(g, 64, 64)
    gy = ints(g, (n, 64, (h - 1) // 2 + 1, (w - 1) // 2 + 1))
    dx_ref, _ = _grads(ref, wt, gy, 2)
    premise16(fam, gy, dx_ref)
    want_dx = dx_ref * gate(ref, 0.25)
    wpd = ops.packed_filter(cd, wt.float().to(dev), L.PACK_DGRAD, 64)
    gd = _nhwc(gy, cd, dev)
    d0, _, _ = ops.conv3x3_raw(cd, gd, wpd, 64, mode=L.CONV_DGRAD, out_hw=(h, w), stride=2, dact_mask=out, dact_slope=0.25)
    assert _kernel(fam, "." + cdn).startswith("conv_s2d3_kernel"), ops._last_kernel()
    exact("gated by the tensor", _nchw(d0, cd), want_dx)
    d1, _, _ = ops.conv3x3_raw(cd, gd, wpd, 64, mode=L.CONV_DGRAD, out_hw=(h, w), stride=2, dact_mask=signs, dact_slope=0.25, dact_bits=True)
    assert ops._last_kernel().startswith("conv_s2d3_kernel"), ops._last_kernel()
    exact("gated by the sign bits", _nchw(d1, cd), want_dx)


# ------------------------------------------------------------------------------------------------- first layer (conv_c3)
_C3_SCALE, _C3_SHIFT = (1.0, 2.0, 0.5), (1.0, -1.0, 0.0)      # powers of two and integers: the normalised image stays exact


def _c3_image(g, n, h, w, layout):
    img = ints(g, (n, 3, h, w))
    imgf = img.float()
    if layout == "nhwc":
        imgf = imgf.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    xn = img * torch.tensor(_C3_SCALE, dtype=F64).view(1, 3, 1, 1) + torch.tensor(_C3_SHIFT, dtype=F64).view(1, 3, 1, 1)
    return imgf, xn


@pytest.mark.parametrize("backend,cdn,cout,act,layout", _cases(
    emu=[("bf16", 32, L.ACT_NONE, "nchw"), ("f32", 64, L.ACT_PRELU, "nchw"), ("bf16", 128, L.ACT_LEAKY, "nhwc"), ("f32", 128, L.ACT_NONE, "nhwc"),
         ("f32", 32, L.ACT_LEAKY, "nhwc"), ("bf16", 128, L.ACT_PRELU, "nchw")],
    hip=[(c, co, a, l) for c in ("f32", "bf16") for (co, a, l) in ((32, L.ACT_NONE, "nchw"), (64, L.ACT_PRELU, "nchw"), (128, L.ACT_NONE, "nhwc"),
                                                                    (128, L.ACT_LEAKY, "nhwc"), (32, L.ACT_LEAKY, "nhwc"), (128, L.ACT_PRELU, "nchw"))]))
def test_exact_first_layer_forward(backend, cdn, cout, act, layout):
    """fsr_conv3x3_c3_fwd straight from the float image (per-channel scale and shift fused): ragged 16 x 16 tiles, channel blocks
    beyond 64, both image layouts, the PReLU pre-activation copy."""
    dev = select(backend)
    fam = "conv_c3"
    cd = ops.Compute(cdn)
    g = _gen(11)
    n, h, w = (3, 83, 106) if dev.type == "cuda" else (2, 11, 21)
    imgf, xn = _c3_image(g, n, h, w, layout)
    wt, bias = pm1(g, cout, 3), ibias(g, cout)
    z = F.conv2d(xn, wt, bias, 1, 1)
    ref = {L.ACT_NONE: z, L.ACT_LEAKY: F.leaky_relu(z, 0.5), L.ACT_PRELU: F.prelu(z, torch.tensor([-0.25], dtype=F64))}[act]
    premise16(fam, xn, z)
    imgd, biasd = imgf.to(dev), bias.float().to(dev)
    out = torch.empty((n, h, w, cout), dtype=cd.torch_dtype, device=dev)
    pre = torch.empty_like(out) if act == L.ACT_PRELU else None
    wpk = ops.packed_filter(cd, wt.float().to(dev), ops.PACK_C3, 32)
    a = torch.tensor([-0.25]).to(dev) if act == L.ACT_PRELU else None
    L.check(L.lib().fsr_conv3x3_c3_fwd(cd.code, imgd.data_ptr(), *imgd.stride(), n, h, w, *_C3_SCALE, *_C3_SHIFT, wpk.data_ptr(),
                                       biasd.data_ptr(), act, 0.5, ops._p(a), cout, out.data_ptr(), ops._p(pre), None,
                                       ops._stream()), "fsr_conv3x3_c3_fwd")
    exact("first layer forward", _nchw(out, cd), ref)
    if pre is not None:
        exact("pre-activation copy", _nchw(pre, cd), z)


@pytest.mark.parametrize("backend,cdn,cout", _cases(emu=[("bf16", 32), ("f32", 64)], hip=[("f32", 64), ("bf16", 64), ("bf16", 128), ("f32", 32)]))
def test_exact_first_layer_weight_and_bias_gradient(backend, cdn, cout):
    """fsr_conv3x3_c3_wgrad accumulating into pre-filled arenas: the weight gradient, and the bias gradient from the column of
    ones at k = 27 of the same MFMAs, which is exactly sum(dz)."""
    dev = select(backend)
    fam = "conv_c3_wgrad"
    cd = ops.Compute(cdn)
    g = _gen(31)
    n, h, w = (3, 70, 52) if dev.type == "cuda" else (2, 9, 19)
    imgf, xn = _c3_image(g, n, h, w, "nchw")
    wt, bias = pm1(g, cout, 3), ibias(g, cout)
    dz = ints(g, (n, cout, h, w))
    _, dw_ref = _grads(xn, wt, dz, 1)
    premise16(fam, xn, dz)
    premise_sum(fam, _wgrad_bound(xn, dz) + 5.0)
    leaf = lambda t: t.float().to(dev).requires_grad_(True)
    wd, bd = leaf(wt), leaf(bias)
    wd._fsr_grad = torch.full_like(wd, 5.0).detach()           # arenas ACCUMULATE: an integer start keeps the sum exact
    bd._fsr_grad = torch.full_like(bd, -4.0).detach()
    cfg = ops.ConvCfg(cd, act=L.ACT_LEAKY, slope=0.25, image_in=True, act_bwd_by_consumer=True, in_scale=_C3_SCALE, in_shift=_C3_SHIFT)
    y, _ = ops.conv3x3(imgf.to(dev), wd, bd, None, cfg)
    y.backward(_nhwc(dz, cd, dev))
    assert wd.grad is None and bd.grad is None
    exact32("first layer weight gradient", wd._fsr_grad, dw_ref + 5.0)
    exact32("bias gradient (column 27)", bd._fsr_grad, dz.sum((0, 2, 3)) - 4.0)


# ------------------------------------------------------------------------------------------------- weight-gradient forms
_WG_ROWS = [(64, False, 0, 1, 0), (128, False, 0, 1, 0), (128, False, 64, 1, 0), (256, True, 0, 1, 0), (64, False, 0, 2, 0), (128, False, 0, 2, 0),
            (64, False, 64, 1, 0), (64, False, 0, 2, 8), (128, False, 0, 2, 8), (256, True, 64, 1, 0)]


@pytest.mark.parametrize("backend,cdn,cout,ps,bm,stride,s2", _cases(
    emu=[(("bf16", "f16")[i % 2],) + r for i, r in enumerate(_WG_ROWS)],
    hip=[(c,) + r for c in ("bf16", "f16") for r in _WG_ROWS]))
def test_exact_conv_wgrad_forms(backend, cdn, cout, ps, bm, stride, s2, monkeypatch):
    """The 16-bit weight gradients with two slabs (every workgroup walks a range of tiles, ragged edges included): the 128- and
    64-row blocks (FSR_WGRAD_BM=64), pixel-shuffled dy across quadrants, stride 2 in the 4-row and 8-row (FSR_WGRAD_S2=8) forms."""
    dev = select(backend)
    monkeypatch.setenv("FSR_WGRAD_SLABS", "2")
    if bm:
        monkeypatch.setenv("FSR_WGRAD_BM", str(bm))
    if s2:
        monkeypatch.setenv("FSR_WGRAD_S2", str(s2))
    fam = "conv_wgrad"
    cd = ops.Compute(cdn)
    g = _gen(21)
    n, h, w = (3, 37, 45) if dev.type == "cuda" else (2, 11, 21)
    x = ints(g, (n, 64, h, w))
    gy = ints(g, (n, cout, (h - 1) // stride + 1, (w - 1) // stride + 1))
    _, dw_ref = _grads(x, torch.zeros(cout, 64, 3, 3, dtype=F64), gy, stride)
    premise16(fam, x, gy)
    premise_sum(fam, _wgrad_bound(x, gy))
    gd = _nhwc(F.pixel_shuffle(gy, 2) if ps else gy, cd, dev)
    dw = ops.conv3x3_wgrad_raw(cd, _nhwc(x, cd, dev), gd, cout, 64, stride, dy_pixel_shuffled=ps)
    exact32("weight gradient", dw, dw_ref)


@pytest.mark.parametrize("backend,cdn,nlayers", _cases(emu=[("bf16", 3), ("f16", 17), ("f32", 3)], hip=[(c, k) for c in ("f32", "bf16", "f16") for k in (3, 17)]))
def test_exact_conv_wgrad_grouped(backend, cdn, nlayers):
    """The grouped 64 -> 64 weight gradient (one launch for all layers) accumulating into integer-filled arenas."""
    dev = select(backend)
    big = dev.type == "cuda"
    fam = "conv_wgrad_grouped"
    cd = ops.Compute(cdn)
    g = _gen(9)
    n, h, w = (4, 40, 56) if big else (1, 5 if nlayers >= 17 else 9, 20)
    xs = [ints(g, (n, 64, h, w)) for _ in range(nlayers)]
    gs = [ints(g, (n, 64, h, w)) for _ in range(nlayers)]
    premise16(fam, *xs, *gs)
    premise_sum(fam, _wgrad_bound(xs[0], gs[0]) + 7.0)
    cfg = types.SimpleNamespace(stride=1, pixel_shuffle=False)
    arenas = [torch.full((64, 64, 3, 3), 7.0, dtype=torch.float32, device=dev) for _ in range(nlayers)]
    ops.wgrad_stream_begin(dev)
    try:
        for x, gy, a in zip(xs, gs, arenas):
            assert ops._wgrad_defer(cd, _nhwc(x, cd, dev), _nhwc(gy, cd, dev), 64, 64, cfg, a)
        ops.wgrad_stream_join()
    finally:
        ops.wgrad_stream_end()
    if big:
        torch.cuda.synchronize()
    for i, (x, gy, a) in enumerate(zip(xs, gs, arenas)):
        _, dw_ref = _grads(x, torch.zeros(64, 64, 3, 3, dtype=F64), gy, 1)
        exact32("layer %d of %d" % (i, nlayers), a, dw_ref + 7.0)


# ------------------------------------------------------------------------------------------------- x3 mode
# Small integers have a zero low half (lo = bf16(v - bf16(v)) = 0), so hi*hi + lo*hi + hi*lo is the exact product.
@pytest.mark.parametrize("backend,stride,cin,cout", _cases(
    emu=[(1, 128, 128), (1, 128, 64), (1, 64, 64), (2, 64, 64), (2, 128, 128)],
    hip=[(1, 128, 128), (1, 128, 64), (1, 64, 64), (2, 64, 64), (2, 128, 128)]))
def test_exact_x3_conv_families(backend, stride, cin, cout, monkeypatch):
    """x3 forward with statistics, data gradient (masked where conv_s2d3<x3> takes it) and weight gradient on the kernels
    tests/test_x3.py routes: conv_tall3's x3 wide / narrow blocks, conv_s2d3<x3>, the x3 weight gradient."""
    dev = select(backend)
    big = dev.type == "cuda"
    monkeypatch.setenv("FSR_PERSIST_CUS", "3" if big else "1")
    fam = "x3"
    cd = ops.Compute("x3")
    g = _gen(1)
    n, h, w = (3, 37, 45) if big else (1, 18, 20)
    x, wt, bias = ints(g, (n, cin, h, w)), pm1(g, cout, cin), ibias(g, cout)
    ref = F.conv2d(x, wt, bias, stride, 1)
    gy, mask = ints(g, ref.shape), ints(g, x.shape)
    dx_ref, dw_ref = _grads(x, wt, gy, stride)
    premise16(fam, x, wt, ref, gy, dx_ref)
    premise_sum(fam, _wgrad_bound(x, gy))
    premise_stats(fam, ref)
    xd = _nhwc(x, cd, dev)
    y, _, stats = ops.conv3x3_raw(cd, xd, ops.FilterSpec(wt.float().to(dev), L.PACK_FWD, cin), cout, stride=stride, bias=bias.float().to(dev),
                                  want_stats=True)
    name = _kernel(fam, ".fwd.s%d.%d-%d" % (stride, cin, cout))
    assert name.startswith("conv_tall3_kernel<x3") and "stats" in name and ("s2>" in name) == (stride == 2), name
    exact("x3 forward", _nchw(y, cd), ref)
    _check_stats("x3 statistics", stats, ref)
    gd = _nhwc(gy, cd, dev)
    spec_d = ops.FilterSpec(wt.float().to(dev), L.PACK_DGRAD, cout)
    dx, _, _ = ops.conv3x3_raw(cd, gd, spec_d, cin, mode=L.CONV_DGRAD, out_hw=(h, w), stride=stride, dact_mask=_nhwc(mask, cd, dev), dact_slope=0.25)
    name = _kernel(fam, ".dgrad.s%d.%d-%d" % (stride, cin, cout))
    assert name == "conv_s2d3_kernel<x3>" if stride == 2 else name.startswith("conv_tall3_kernel<x3"), name
    exact("x3 masked data gradient", _nchw(dx, cd), dx_ref * gate(mask, 0.25))
    dw = ops.conv3x3_wgrad_raw(cd, xd, gd, cout, cin, stride)
    exact32("x3 weight gradient", dw, dw_ref)


@pytest.mark.parametrize("backend,cus", _cases(emu=[(1,)], hip=[(1,), (3,)]))
def test_exact_x3_thin_head_and_image_gradient(backend, cus, monkeypatch):
    """conv64_thin_kernel<x3>: the 64 -> 3 forward (float output, no tanh: tanh is not exact) and the 64 -> 3 data gradient
    with a per-channel power-of-two scale, plus the weight gradient of the 64 -> 3 layer."""
    dev = select(backend)
    monkeypatch.setenv("FSR_PERSIST_CUS", str(cus))
    fam = "x3_thin"
    cd = ops.Compute("x3")
    g = _gen(4)
    n, h, w = (3, 37, 45) if dev.type == "cuda" else (2, 17, 19)
    x, wt, bias = ints(g, (n, 64, h, w)), pm1(g, 3, 64), ibias(g, 3)
    ref = F.conv2d(x, wt, bias, 1, 1)
    g3 = ints(g, (n, 3, h, w))
    _, dw_ref = _grads(x, wt, g3, 1)
    premise16(fam, x, ref)
    premise_sum(fam, _wgrad_bound(x, g3))
    xd = _nhwc(x, cd, dev)
    wpk = ops.packed_filter(cd, wt.float().to(dev), L.PACK_FWD, 64)
    y, _, _ = ops.conv3x3_raw(cd, xd, wpk, 3, bias=bias.float().to(dev), out_f32=True)
    assert _kernel(fam, ".head") == "conv64_thin_kernel<x3>", ops._last_kernel()
    exact("x3 64 -> 3 forward", _nchw(y, cd, plain=True), ref)
    w1, gy = pm1(g, 64, 3, density=1.0 / 16), ints(g, (n, 64, h, w))        # 36 of the gradient's 9 x 64 taps
    x1 = ints(g, (n, 3, h, w))
    dx_ref, _ = _grads(x1, w1, gy, 1)
    scale = torch.tensor([2.0, 0.5, 4.0], dtype=F64)
    premise16(fam, dx_ref * scale.view(1, 3, 1, 1))
    wpk_d = ops.packed_filter(cd, w1.float().to(dev), L.PACK_DGRAD, 64)
    gd = _nhwc(gy, cd, dev)
    dx, _, _ = ops.conv3x3_raw(cd, gd, wpk_d, 3, mode=L.CONV_DGRAD, out_hw=(h, w), out_f32=True, oscale=scale.float().to(dev))
    assert _kernel(fam, ".image_gradient") == "conv64_thin_kernel<x3>", ops._last_kernel()
    exact("x3 image gradient", _nchw(dx, cd, plain=True), dx_ref * scale.view(1, 3, 1, 1))
    dw = ops.conv3x3_wgrad_raw(cd, xd, _nhwc(g3, cd, dev, pad_to=cd.pad(3)), 3, 64, 1)
    exact32("x3 64 -> 3 weight gradient", dw, dw_ref)


@pytest.mark.parametrize("backend", _cases(emu=[()], hip=[()]))
def test_exact_x3_first_layer(backend):
    """Conv2d(3 -> 64) + LeakyReLU from the float image on x3 storage, through autograd: forward, image gradient, weight and
    bias gradient."""
    dev = select(backend)
    fam = "x3_c3"
    cd = ops.Compute("x3")
    g = _gen(4)
    n, h, w = (2, 37, 45) if dev.type == "cuda" else (1, 9, 20)
    img, wt, bias = ints(g, (n, 3, h, w)), pm1(g, 64, 3, density=0.25), ibias(g, 64)      # 144 of the image gradient's 9 x 64 taps
    r = ints(g, (n, 64, h, w))
    xr, wr, br = (t.clone().requires_grad_(True) for t in (img, wt, bias))
    yr = F.leaky_relu(F.conv2d(xr, wr, br, 1, 1), 0.25)
    yr.backward(r)
    premise16(fam, img, yr.detach(), xr.grad)
    premise_sum(fam, _wgrad_bound(img, r))
    xd = img.float().to(dev).requires_grad_(True)
    p = [t.float().to(dev).requires_grad_(True) for t in (wt, bias)]
    y, _ = ops.conv3x3(xd, p[0], p[1], None, ops.ConvCfg(cd, act=L.ACT_LEAKY, slope=0.25, image_in=True))
    y.backward(_nhwc(r, cd, dev))
    exact("x3 first layer", _nchw(y, cd), yr.detach())
    exact("x3 image gradient", xd.grad, xr.grad)
    exact32("x3 first-layer weight gradient", p[0].grad, wr.grad)
    exact32("x3 first-layer bias gradient", p[1].grad, br.grad)


# ------------------------------------------------------------------------------------------------- stage-contiguous filter pack
@pytest.mark.parametrize("backend,case", _cases(emu=[("fwd128",), ("dgrad_narrow",), ("dgrad_s2",)], hip=[("fwd128",), ("dgrad_narrow",), ("dgrad_s2",)]))
def test_exact_stage_contiguous_filter_pack(backend, case, monkeypatch):
    """Launches that are handed the WEIGHT (ops.FilterSpec) read the stage-contiguous pack: exact against float64, not only
    equal to the launch on the standard pack."""
    dev = select(backend)
    big = dev.type == "cuda"
    monkeypatch.setenv("FSR_PERSIST_CUS", "2" if big else "1")
    fam = "lin_pack"
    cd = ops.Compute("bf16")
    g = _gen(21)
    cin, cout, stride, mode, want_blk = {"fwd128": (160, 256, 1, L.CONV_FWD, 128), "dgrad_narrow": (64, 128, 1, L.CONV_DGRAD, 64),
                                         "dgrad_s2": (128, 160, 2, L.CONV_DGRAD, 64)}[case]
    n, h, w = (2, 34, 40) if big else (1, 18, 20)
    wt = pm1(g, cout, cin)
    wd = wt.float().to(dev)
    x = ints(g, (n, cin, h, w))
    if mode == L.CONV_FWD:
        ref = F.leaky_relu(F.conv2d(x, wt, None, stride, 1), 0.25)
        inp = _nhwc(x, cd, dev)
        kw = dict(stride=stride, act=L.ACT_LEAKY, slope=0.25)
        pmode, kpad, co = L.PACK_FWD, cin, cout
    else:
        gy = ints(g, (n, cout, (h - 1) // stride + 1, (w - 1) // stride + 1))
        mask = ints(g, (n, cin, h, w))
        dx_ref, _ = _grads(x, wt, gy, stride)
        ref = dx_ref * gate(mask, 0.5)
        inp = _nhwc(gy, cd, dev)
        kw = dict(mode=L.CONV_DGRAD, out_hw=(h, w), stride=stride, dact_mask=_nhwc(mask, cd, dev), dact_slope=0.5)
        pmode, kpad, co = L.PACK_DGRAD, cout, cin
    premise16(fam, x, ref)
    y1, _, _ = ops.conv3x3_raw(cd, inp, ops.FilterSpec(wd, pmode, kpad), co, **kw)
    _kernel(fam, "." + case)
    key = [k for k in ops._pack_cache[id(wd)][1] if k[0] == pmode]
    assert [k[3] for k in key] == [want_blk], key           # the launch read the stage-contiguous pack of that block size
    exact("stage-contiguous pack", _nchw(y1, cd), ref)
    y0, _, _ = ops.conv3x3_raw(cd, inp, ops.packed_filter(cd, wd, pmode, kpad), co, **kw)
    exact("standard pack", _nchw(y0, cd), ref)


# ------------------------------------------------------------------------------------------------- fsr_act_bwd
@pytest.mark.parametrize("backend,cdn,c,ps", _cases(
    emu=[(cdn, c, ps) for (cdn, c) in (("bf16", 32), ("bf16", 64), ("bf16", 256), ("bf16", 512), ("f32", 64), ("f32", 512)) for ps in (False, True)],
    hip=[(cdn, c, ps) for (cdn, c) in (("bf16", 32), ("bf16", 64), ("bf16", 256), ("bf16", 512), ("f32", 64), ("f32", 512)) for ps in (False, True)]))
def test_exact_act_bwd(backend, cdn, c, ps):
    """fsr_act_bwd: dz, the bias-gradient column sums (pixel-shuffled: per channel and quadrant) and the PReLU-slope sum, for 4 to
    128 channel units per pixel (both readout branches of the workgroup reduction), several slabs with a partial last one."""
    dev = select(backend)
    fam = "act_bwd"
    cd = ops.Compute(cdn)
    gen = _gen(41)
    n, h, w = 2, 18, 22
    for act, slope in ((L.ACT_PRELU, -0.25), (L.ACT_LEAKY, 0.5)):
        g, saved = ints(gen, (n, h, w, c)), ints(gen, (n, h, w, c), -3, 3)
        dz_ref = g * gate(saved, slope)
        if ps:      # channel 4 ch + 2 (y & 1) + (x & 1) of the conv that was depth-to-space'd
            db_ref = torch.stack([dz_ref[:, dy::2, dx::2].sum((0, 1, 2)) for dy in (0, 1) for dx in (0, 1)], dim=1).reshape(-1)
        else:
            db_ref = dz_ref.sum((0, 1, 2))
        da_ref = (g * saved.clamp(max=0)).sum().reshape(1)
        premise16(fam, g, saved, dz_ref)
        premise_sum(fam, dz_ref.abs().sum((0, 1, 2)).max(), (g * saved.clamp(max=0)).abs().sum())
        gd, sd = g.to(cd.torch_dtype).to(dev), saved.to(cd.torch_dtype).to(dev)
        dz = torch.empty_like(gd)
        dbias = torch.zeros(c * (4 if ps else 1), dtype=torch.float32, device=dev)
        dprelu = torch.zeros(1, dtype=torch.float32, device=dev) if act == L.ACT_PRELU else None
        a = torch.tensor([slope]).to(dev) if act == L.ACT_PRELU else None
        lib = L.lib()
        scr = ops._workspace(lib.fsr_act_bwd_scratch(n, h, w, c, int(ps)), dev)
        L.check(lib.fsr_act_bwd(cd.code, gd.data_ptr(), sd.data_ptr(), act, slope, ops._p(a), dz.data_ptr(), dbias.data_ptr(), ops._p(dprelu),
                                scr.data_ptr(), n, h, w, c, int(ps), ops._stream()), "fsr_act_bwd")
        exact("dz", dz.float(), dz_ref)
        exact32("bias gradient", dbias, db_ref)
        if dprelu is not None:
            exact32("PReLU slope gradient", dprelu, da_ref)


# ------------------------------------------------------------------------------------------------- Conv2d(512 -> 1, k = 1)
@pytest.mark.parametrize("backend,cdn", _cases(emu=[("bf16",), ("f32",)], hip=[("f32",), ("bf16",), ("f16",)]))
def test_exact_conv1x1_at_model_width(backend, cdn):
    """fsr_conv1x1_c1_fwd / _bwd at c = 512, the discriminator's width: logits, dx, dw and db."""
    dev = select(backend)
    fam = "conv1x1"
    cd = ops.Compute(cdn)
    g = _gen(5)
    n, c, h, w = (2, 512, 13, 9) if dev.type == "cuda" else (1, 512, 5, 7)
    x = ints(g, (n, c, h, w))
    wt = pm1(g, 1, c, k=1)                  # density 36 / c: 36 taps per logit
    b = ibias(g, 1)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, wt, b))
    lr = F.conv2d(xr, wr, br)
    gl = ints(g, lr.shape)
    lr.backward(gl)
    premise16(fam, x, lr.detach(), xr.grad)
    premise_sum(fam, _wgrad_bound(x, gl))
    xd = _nhwc(x, cd, dev).requires_grad_(True)
    wd, bd = (t.float().to(dev).requires_grad_(True) for t in (wt, b))
    lg = ops.conv1x1_to_logits(xd, wd, bd, cd)
    exact("logits", lg, lr.detach())
    lg.backward(gl.float().to(dev))
    exact("dx", _nchw(xd.grad, cd), xr.grad)
    exact32("dw", wd.grad, wr.grad)
    exact32("db", bd.grad, br.grad)


# ------------------------------------------------------------------------------------------------- why this file exists
def test_exact_gate_is_sharper_than_the_tolerance_gates():
    """No kernel is launched.  On a (3, 37, 45) 64 -> 64 layer two one-element errors -- (a) one tap dropped at one corner pixel,
    (b) one pixel left out of sum(y^2) -- stay UNDER the relerr bounds the randn tests gate on (1e-2 for 16-bit outputs, 1e-3 for
    statistics); with the integer inputs of this file the exact comparison rejects both.  Turning the exact gate back into a
    tolerance makes this test fail."""
    def corrupt(x, wt, ref):
        a = ref.clone()
        a[0, 5, 0, 0] -= x[0, 7, 0, 0] * wt[5, 7, 1, 1]          # (a) the centre tap of input channel 7 at the top-left corner
        sq = (ref * ref).sum((2, 3))
        b = sq.clone()
        b[1, 9] -= ref[1, 9, 36, 44] ** 2                        # (b) the last pixel of a ragged tile
        return a, sq, b

    torch.manual_seed(1)
    x = torch.randn(3, 64, 37, 45, dtype=F64).bfloat16().double()
    wt = (torch.randn(64, 64, 3, 3, dtype=F64) * 0.1).bfloat16().double()
    x[0, 7, 0, 0], wt[5, 7, 1, 1] = 1.0, 0.1015625               # a typical tap: |x w| ~ 0.1
    ref = F.conv2d(x, wt, None, 1, 1)
    a, sq, b = corrupt(x, wt, ref)
    assert not torch.equal(a, ref) and not torch.equal(b, sq)
    assert relerr(a, ref) < 1e-2 and relerr(b, sq) < 1e-3       # the tolerance gates pass both corruptions

    g = _gen(1)
    x, wt = ints(g, (3, 64, 37, 45)), pm1(g, 64, 64)
    x[0, 7, 0, 0], wt[5, 7, 1, 1] = 2.0, 1.0
    ref = F.conv2d(x, wt, None, 1, 1)
    if ref[1, 9, 36, 44] == 0:
        ref = F.conv2d(x, wt, torch.ones(64, dtype=F64), 1, 1)   # (the left-out pixel must carry a non-zero square)
    premise16("sharpness", x, wt, ref)
    a, sq, b = corrupt(x, wt, ref)
    premise_sum("sharpness", sq)
    with pytest.raises(AssertionError):
        exact("dropped tap", a.float(), ref)
    with pytest.raises(AssertionError):
        exact32("pixel left out of sum(y^2)", b.float(), sq)
    exact("uncorrupted", ref.bfloat16(), ref)                    # ... and bf16 storage of the true result passes
    exact32("uncorrupted sum(y^2)", sq.float(), sq)
