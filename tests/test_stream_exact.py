"""Float64-referenced parity of the HBM-bound kernels (elementwise.hip), the losses / 1x1 convolution (losses.hip), AdamW (optim.hip) and the
second-level reduce (reduce.hip), called through the C ABI at the shapes where each kernel takes another path.

test_exact.py covers the convolution families with integer inputs and no tolerance.  The kernels here divide, take square roots
and exponentials, so only the selections and the exactly representable operations are bit-exact (max-pool and its arg-max
bytes, u8 -> float, add and the 1x1 convolution on integers, the skipped AdamW step, the loss-scale state machine).  Everything
else is held, ELEMENT BY ELEMENT, to the float64 evaluation of the kernel's documented formula from the same float32 inputs
(for InstanceNorm: the same float32 `stats`):

    |got_i - ref64_i|  <=  K * 2^-23 * s_i  (+ half an ulp of the storage type when the output is 16-bit, + 2^-16 |ref_i| for x3:
                                              hi = bf16(v) leaves |v - hi| <= 2^-8 |v|, lo = bf16(v - hi) 2^-8 of that)

where s_i is the magnitude of the element's intermediates (written next to each reference below), and sums to

    |got - ref64|  <=  (terms + 8) * 2^-24 * sum_i |term_i|     (any fixed-order f32 summation plus a few ulp per addend).

An element whose float64 |xh| < 1e-5 may take either activation branch: such elements are left out of the per-element
comparisons (at most 0.1 % of a case), and the cases that check SUMS assert that their input has none (next seed otherwise).
Results below 2^-126 (subnormal f32, e.g. sigmoid(-90)) have no relative precision: the loss gates add that as a floor.

K per kernel is the smallest power of two (>= 1) for which a plain float32 numpy restatement of the formula stays inside ONE
THIRD of the cap on the very inputs of the cases (test_float32_restatement_is_inside_a_third_of_the_caps); the other two thirds
are the room for the device's rsqrtf / expf / log1pf / powf (about 1 ulp each), fused multiply-adds and another association.
Measured maximum of |result - ref64| / (2^-23 s_i), i.e. in the units K counts:

    kernel                         K    restatement   MI355X   s_i
    instnorm_act_fwd               8    2.16          2.16     (|x| + |mean|) rstd max(1, |slope|) + |res|
    instnorm_act_bwd_apply        16    3.53          2.95     rstd (|gz| + |m1| + (|x| + |mean|) rstd |m2|)
    image_to_nhwc                  4    0.85          0.49     |img a| + |b|
    tanh_bwd (both kernels)        4    0.72          0.72     |g| (1 + y^2)
    bce_logits_bwd                 4    1.00          3.26     |gs| (sigmoid(x) + |t|)
    smooth_l1_bwd                  1    0.17          0.17     |gs clamp(a - b)|
    adamw m                        2    0.50          0.46     |m| + |g gs|
    adamw v                        4    0.98          0.98     |v| + (g gs)^2
    adamw update                   4    0.78          0.78     lr / (1 - b1^t) (|m| + |g gs|) / denom (1 + A(t)) + |p|

(MI355X: the largest error of the f32 cases in the same units, i.e. K times the error / cap ratio the log shows.  The BCE figure
comes from the logits whose sigmoid is tiny against a target of 0, where no larger intermediate absorbs the roundings of expf, the
reciprocal and gs: the one kernel that uses the room the factor three leaves.  The
16-bit cases reach 0.9998 of their caps, as round-to-nearest stores must: half an ulp of the storage type is most of those caps; x3
reaches 0.46.  The sums stay below 0.06 of the textbook bound.)

The AdamW update cap is dominated by the bias corrections: 1 - powf(beta, t) cancels, so one ulp of either operand is a relative
error of 2^-23 (1 + beta^t) / (1 - beta^t) of the correction, and A(t) = (1 + b2^t) / (2 (1 - b2^t)) + (1 + b1^t) / (1 - b1^t) carries that
into s_i (the condition number of the subtraction, as |x| + |mean| is for x - mean): A(1) = 1018, A(10) = 102, A(1000) = 2.1 for the
default betas.  That is NOT of ulp size at t = 1: the cap there is 5e-4 of the update.  numpy's float32 power is exact at t = 1, so
the plain restatement cannot show the need; test_adamw_update_cap_holds_one_ulp_of_powf_and_needs_its_amplification moves both
powers by +-1 ulp and asserts both sides.  In units of 2^-23 s_u (K = 4), largest over the rows of each step count:

    t       restatement   powers +-1 ulp   the same without A(t) in s_u   MI355X
    1       0.61          0.61             24.7                           0.61
    10      0.66          0.70             19.1                           0.66
    1000    0.78          0.78             2.20                           0.78

(The MI355X's powf is exact at t = 1 -- with no weight decay its error there is 0.001 units -- and uses the amplification at
t = 10; the t = 1 figure is the rounding of p (1 - lr wd), the |p| in s_u.  The 0.78 at t = 1000 is m' = 0.9 m + 0.1 g gs
cancelling for some elements, the update inheriting m's rounding -- hence |m| + |g gs| in s_u.)

Every ratio error / cap the kernels reach goes to the parity-error log through backend.report (stream.*).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from backend import BACKENDS, L, ops, relerr, report, select

F32, F64 = np.float32, np.float64
U = 2.0 ** -23                 # one unit of the per-element caps
TINY = 2.0 ** -126             # smallest normal f32
GPU = pytest.mark.gpu
K_IN_FWD, K_IN_APPLY, K_IMAGE, K_TANH, K_BCE, K_SL1, K_ADAM_M, K_ADAM_V, K_ADAM_U = 8, 16, 4, 4, 4, 1, 2, 4, 4
GATE_XH = 1e-5                 # |xh| below this: either activation branch
SLOPES = {L.ACT_PRELU: -0.28, L.ACT_LEAKY: 0.2, L.ACT_NONE: 0.0, L.ACT_RELU: 0.0}      # the `slope` ARGUMENT of the call
ACTS = (L.ACT_PRELU, L.ACT_LEAKY, L.ACT_NONE, L.ACT_RELU)


def _cases(both=(), hip=()):
    """(backend, *case): `both` on the emulator and the MI355X, `hip` on the MI355X only (above about 2 M elements)."""
    return [pytest.param("emu", *c) for c in both] + [pytest.param("hip", *c, marks=GPU) for c in tuple(both) + tuple(hip)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------- storage and gates
def _store(cdn, a):
    """float32 values -> (storage tensor of the mode, the float64 values it holds)."""
    cd = ops.Compute(cdn)
    t = ops.to_storage(cd, a.float().contiguous())
    return t, ops.from_storage(cd, t).double().numpy()


def _load(cdn, t):
    return ops.from_storage(ops.Compute(cdn), t.detach().cpu()).double().numpy()


def _out_like(t, dev):
    return ops._empty(tuple(t.shape), t.dtype, dev)


def _half_ulp(v, cdn):
    """Half an ulp of the storage type at magnitude v (the rounding of a 16-bit store; x3: see the module docstring)."""
    if cdn == "f32":
        return 0.0
    if cdn == "x3":
        return 2.0 ** -16 * v
    p, emin = (8, -126) if cdn == "bf16" else (11, -14)
    e = np.maximum(np.frexp(np.maximum(v, 1e-300))[1] - 1, emin)
    return 0.5 * np.ldexp(1.0, e - (p - 1))


_worst, _where = {}, ["-"]


def _select(backend):
    _where[0] = backend
    return select(backend)


def _note(key, value):
    """The largest error / cap ratio of a key so far goes to the parity-error log as stream.<backend>.<key>."""
    key = "stream.%s.%s" % (_where[0], key)
    if value > _worst.get(key, -1.0):
        _worst[key] = value
        report(key, value)


def _first(ratio, got, ref, cap):
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return "%d of %d over the cap; worst at %s: got %.9g, want %.9g, cap %.3g (%.3g x)" % (
        int((ratio > 1).sum()), ratio.size, tuple(int(v) for v in i), got[i], ref[i], cap[i], ratio[i])


def gate(key, what, got, ref, scale, K, cdn="f32", keep=None, floor=0.0):
    """THE per-element comparison of this file: |got - ref| <= K 2^-23 scale (+ floor) + half an ulp of the storage type."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: non-finite values" % what
    cap = K * U * np.broadcast_to(np.asarray(scale, F64), ref.shape) + floor
    cap = cap + _half_ulp(np.abs(ref) + cap, cdn)
    ratio = np.abs(got - ref) / np.maximum(cap, 1e-300)
    if keep is not None:
        assert keep.mean() >= 0.999, "%s: %.3g of the elements sit on the activation's kink" % (what, 1 - keep.mean())
        ratio = np.where(keep, ratio, 0.0)
    if key:
        _note(key, float(ratio.max()))
    assert ratio.max() <= 1.0, "%s: %s" % (what, _first(ratio, got, ref, cap))


def sum_gate(key, what, got, ref, terms, mag, floor=0.0):
    """THE comparison of sums: |got - ref| <= (terms + 8) 2^-24 sum |term| (+ floor)."""
    got, ref, mag = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(mag, F64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: non-finite values" % what
    cap = np.broadcast_to((terms + 8) * 2.0 ** -24 * mag + floor, ref.shape)
    ratio = np.abs(got - ref) / np.maximum(cap, 1e-300)
    if key:
        _note(key, float(ratio.max()))
    assert ratio.max() <= 1.0, "%s: %s" % (what, _first(ratio, got, ref, cap))


def exact(what, got, ref):
    got, ref = torch.as_tensor(got).detach().cpu(), torch.as_tensor(ref).detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        raise AssertionError("%s: %d of %d differ; first (index: got, want): %s" % (what, len(bad), ref.numel(), [
            (tuple(int(v) for v in i), float(got[tuple(i)]), float(ref[tuple(i)])) for i in bad[:6]]))


def _dev32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(dev)


# ------------------------------------------------------------------------------------------------- InstanceNorm (+ activation, + residual)
#           dtype   (n, hw, c)        what it reaches
IN_ROWS = [("f32", (2, 130, 16)),    # cu = 4, 3 slabs of 44 / 44 / 42 pixels, rows = 64 > per
           ("bf16", (2, 130, 64)),   # cu = 8, 3 slabs
           ("f16", (2, 130, 64)),
           ("x3", (2, 130, 64)),     # x3 storage, gated at the f32 cap + the 2^-16 of its hi / lo split (derived above, not the mode's 1e-3)
           ("f32", (1, 2100, 8)),    # 33 slabs: the four-loads-in-flight loop of reduce_partials_kernel; the dprelu reduce has P = 33
           ("bf16", (1, 70, 512)),   # cu = 64, no butterfly
           ("f32", (2, 70, 512)),    # cu = 128, strided wave read-out
           ("f32", (1, 70, 1024)),   # cu = 256, rows = 1
           ("bf16", (1, 70, 2048))]  # cu = 256, rows = 1
IN_BIG = [("f32", (1024, 80, 32)),   # grid capped at 2 blocks per image, units = 640 > step = 512: threads 0..127 take the two-unit
          ("bf16", (1024, 80, 64))]  # trip, 128..511 the tail.  Forward and apply only.


def _eff_slope(act):
    return {L.ACT_PRELU: SLOPES[L.ACT_PRELU], L.ACT_LEAKY: SLOPES[L.ACT_LEAKY], L.ACT_NONE: 1.0, L.ACT_RELU: 0.0}[act]


def _mean_rstd64(stats, hw):
    st = stats.astype(F64)
    mean = st[..., 0] / hw
    var = np.maximum(st[..., 1] / hw - mean * mean, 0.0)
    return mean[:, None, :], (1.0 / np.sqrt(var + float(F32(1e-5))))[:, None, :]


@functools.lru_cache(maxsize=2)
def _in_inputs(cdn, shape):
    """x = 2 randn + 0.5, g, res ~ randn in the storage type; stats = (sum x, sum x^2) in float32.  Premise: no |xh| < 1e-5 where
    sums are checked (the big cases, per-element only, leave at most 0.1 % out instead)."""
    n, hw, c = shape
    big = n * hw * c > (1 << 20)
    for seed in range(100, 164):
        g = _gen(seed)
        xt, x = _store(cdn, torch.randn(shape, generator=g) * 2 + 0.5)
        stats = np.stack([x.sum(1), (x * x).sum(1)], -1).astype(F32)
        mean, rstd = _mean_rstd64(stats, hw)
        keep = np.abs((x - mean) * rstd) >= GATE_XH
        if keep.all() or (big and keep.mean() >= 0.999):      # big: about 20 of 2.6 M elements sit on the kink whatever the seed, so
            break                                               # the first seed is taken and `keep` leaves them out (no sums there)
    else:
        raise AssertionError("premise: no seed without |xh| < 1e-5 at %s" % (shape,))
    gt, gv = _store(cdn, torch.randn(shape, generator=g))
    rt, res = _store(cdn, torch.randn(shape, generator=g))
    return dict(xt=xt, gt=gt, rt=rt, x=x, g=gv, res=res, stats=stats, mean=mean, rstd=rstd, keep=keep, seed=seed)


def in_fwd64(x, mean, rstd, slope, res):
    """y = max(xh, 0) + slope min(xh, 0) + res, xh = (x - mean) rstd;  s = (|x| + |mean|) rstd max(1, |slope|) + |res|."""
    xh = (x - mean) * rstd
    y = np.maximum(xh, 0) + slope * np.minimum(xh, 0)
    s = (np.abs(x) + np.abs(mean)) * rstd * max(1.0, abs(slope))
    return (y, s) if res is None else (y + res, s + np.abs(res))


def in_sums64(x, g, mean, rstd, slope):
    """sums = (sum_p gz, sum_p gz xh) per (image, channel), gz = g (xh > 0 ? 1 : slope); dprelu = sum g min(xh, 0)."""
    xh = (x - mean) * rstd
    gz = g * np.where(xh > 0, 1.0, slope)
    sums = np.stack([gz.sum(1), (gz * xh).sum(1)], -1)
    mags = np.stack([np.abs(gz).sum(1), np.abs(gz * xh).sum(1)], -1)
    dp = g * np.minimum(xh, 0)
    return sums, mags, dp.sum(), np.abs(dp).sum()


def in_apply64(x, g, mean, rstd, sums, hw, slope):
    """dx = rstd (gz - m1 - xh m2), (m1, m2) = sums / hw;  s = rstd (|gz| + |m1| + (|x| + |mean|) rstd |m2|)."""
    m = sums.astype(F64) / hw
    m1, m2 = m[:, None, :, 0], m[:, None, :, 1]
    xh = (x - mean) * rstd
    gz = g * np.where(xh > 0, 1.0, slope)
    return rstd * (gz - m1 - xh * m2), rstd * (np.abs(gz) + np.abs(m1) + (np.abs(x) + np.abs(mean)) * rstd * np.abs(m2))


def _mean_rstd32(stats, hw):
    inv = F32(1) / F32(hw)
    mean = stats[..., 0] * inv
    var = np.maximum(stats[..., 1] * inv - mean * mean, F32(0)) + F32(1e-5)
    return mean[:, None, :], (F32(1) / np.sqrt(var))[:, None, :], inv


def in_fwd32(x, stats, hw, slope, res):
    """The kernel's statements in float32 numpy, one rounding per operation."""
    mean, rstd, _ = _mean_rstd32(stats, hw)
    z = (x - mean) * rstd
    y = np.maximum(z, F32(0)) + F32(slope) * np.minimum(z, F32(0))
    return y if res is None else y + res


def in_apply32(x, g, stats, sums, hw, slope):
    mean, rstd, inv = _mean_rstd32(stats, hw)
    m1, m2 = (sums[..., 0] * inv)[:, None, :], (sums[..., 1] * inv)[:, None, :]
    xh = (x - mean) * rstd
    gz = g * np.where(xh > 0, F32(1), F32(slope))
    return rstd * (gz - m1 - xh * m2)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("backend,cdn,shape", _cases(both=IN_ROWS + IN_BIG))
def test_stream_instnorm_triple(backend, cdn, shape, act):
    """fsr_instnorm_act_fwd (with and without the residual), fsr_instnorm_act_bwd_reduce (sums, dprelu) and
    fsr_instnorm_act_bwd_apply on statistics, activations and channel counts that ops.py never produces."""
    dev = _select(backend)
    n, hw, c = shape
    I = _in_inputs(cdn, shape)
    big = (cdn, shape) in IN_BIG
    cd, lib = ops.Compute(cdn), L.lib()
    slope, tag = _eff_slope(act), "%s.%dx%dx%d.act%d" % (cdn, n, hw, c, act)
    xd, gd, rd = I["xt"].to(dev), I["gt"].to(dev), I["rt"].to(dev)
    stats = _dev32(I["stats"], dev)
    prelu = torch.tensor([SLOPES[act]]).to(dev) if act == L.ACT_PRELU else None
    keep = I["keep"] if act != L.ACT_NONE else None
    for res in (None, I["res"]):
        out = _out_like(xd, dev)
        L.check(lib.fsr_instnorm_act_fwd(cd.code, xd.data_ptr(), stats.data_ptr(), None if res is None else rd.data_ptr(), act, SLOPES[act],
                                         ops._p(prelu), out.data_ptr(), n, hw, c, ops._stream()), "fsr_instnorm_act_fwd")
        ref, s = in_fwd64(I["x"], I["mean"], I["rstd"], slope, res)
        gate("instnorm_fwd." + tag, "forward%s" % ("" if res is None else " + residual"), _load(cdn, out), ref, s, K_IN_FWD, cdn, keep)
    sums_ref, mags, dp_ref, dp_mag = in_sums64(I["x"], I["g"], I["mean"], I["rstd"], slope)
    if not big:
        assert I["keep"].all()
        scr = ops._workspace(lib.fsr_instnorm_act_bwd_scratch(n, hw, c), dev)
        sums = torch.full((n, c, 2), float("nan"), dtype=torch.float32, device=dev)
        dprelu = torch.full((1,), float("nan"), dtype=torch.float32, device=dev) if act == L.ACT_PRELU else None
        L.check(lib.fsr_instnorm_act_bwd_reduce(cd.code, gd.data_ptr(), xd.data_ptr(), stats.data_ptr(), act, SLOPES[act], ops._p(prelu),
                                                sums.data_ptr(), ops._p(dprelu), scr.data_ptr(), n, hw, c, ops._stream()),
                "fsr_instnorm_act_bwd_reduce")
        sum_gate("instnorm_sums." + tag, "sums (sum gz, sum gz xh)", sums.cpu().numpy(), sums_ref, hw, mags)
        if dprelu is not None:
            sum_gate("instnorm_dprelu." + tag, "PReLU slope sum", dprelu.cpu().numpy(), np.reshape(dp_ref, (1,)), n * hw * c, dp_mag)
    sums32 = sums_ref.astype(F32)          # the apply call's `sums` INPUT: the reference's, so the two launches are judged apart
    dx = _out_like(xd, dev)
    L.check(lib.fsr_instnorm_act_bwd_apply(cd.code, gd.data_ptr(), xd.data_ptr(), stats.data_ptr(), _dev32(sums32, dev).data_ptr(), act,
                                           SLOPES[act], ops._p(prelu), dx.data_ptr(), n, hw, c, ops._stream()), "fsr_instnorm_act_bwd_apply")
    ref, s = in_apply64(I["x"], I["g"], I["mean"], I["rstd"], sums32, hw, slope)
    gate("instnorm_apply." + tag, "apply", _load(cdn, dx), ref, s, K_IN_APPLY, cdn, keep)


# ------------------------------------------------------------------------------------------------- MaxPool2d(2, 2)
POOL_VALUES = (-2.0, -0.5, 0.0, 1.0, 3.0)      # exact in every storage type
POOL_ROWS = [("f32", (1, 2, 2, 4)), ("f32", (2, 6, 10, 16)), ("bf16", (2, 6, 10, 16)), ("f16", (2, 6, 10, 16)),
             ("f32", (1, 2, 260, 512)),        # rowunits = 130 * 128 = 16640 > 64 * 256: the in-row grid-stride wraps
             ("bf16", (1, 2, 260, 1024))]      # the same wrap with 8-element units


def _pool_input(shape):
    n, h, w, c = shape
    if shape == (1, 2, 2, 4):     # one window per channel: all negative; tie of positives; tie at zero; maximum in the last position
        x = torch.tensor([[-2.0, 1.0, 0.0, -2.0], [-0.5, 3.0, -2.0, 0.0], [-2.0, 3.0, 0.0, 1.0], [-0.5, 1.0, -0.5, 3.0]]).view(1, 2, 2, 4)
    else:
        x = torch.tensor(POOL_VALUES)[torch.randint(0, 5, shape, generator=_gen(7))]
    win = x.numpy().reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)    # k = 2 dy + dx
    arg, mx = win.argmax(-1), win.max(-1)              # numpy's argmax is the FIRST maximum
    if x.numel() > 256:
        tie = (win == mx[..., None]).sum(-1) > 1
        classes = [(mx < 0).any(), (tie & (mx > 0)).any(), (tie & (mx == 0)).any()] + [(arg == k).any() for k in range(4)]
        assert all(classes), "premise: a window class does not occur: %s" % classes
    return x, arg, mx


@pytest.mark.parametrize("backend,cdn,shape", _cases(both=POOL_ROWS))
def test_stream_maxpool_selection_bytes_and_gradients(backend, cdn, shape):
    """fsr_maxpool2_fwd with its arg-max bytes, fsr_maxpool2_bwd_argmax and fsr_maxpool2_bwd with both relu_mask values: windows
    with a negative maximum, ties (the first in row-major order wins), every arg-max position.  Bit-exact."""
    dev = _select(backend)
    n, h, w, c = shape
    cd, lib = ops.Compute(cdn), L.lib()
    x, arg, mx = _pool_input(shape)
    y_ref = F.max_pool2d(x.permute(0, 3, 1, 2).double(), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(y_ref, torch.from_numpy(mx).double())
    byte_ref = torch.from_numpy((arg | (4 * (mx > 0))).astype(np.uint8))
    g = torch.randint(1, 4, (n, h // 2, w // 2, c), generator=_gen(8)).float() * (torch.randint(0, 2, (n, h // 2, w // 2, c), generator=_gen(9)) * 2 - 1)
    xd, gd = x.to(cd.torch_dtype).to(dev), g.to(cd.torch_dtype).to(dev)
    y = torch.empty((n, h // 2, w // 2, c), dtype=cd.torch_dtype, device=dev)
    idx = torch.full((n, h // 2, w // 2, c), 255, dtype=torch.uint8, device=dev)
    L.check(lib.fsr_maxpool2_fwd(cd.code, xd.data_ptr(), y.data_ptr(), idx.data_ptr(), n, h, w, c, ops._stream()), "fsr_maxpool2_fwd")
    exact("pooled output", y.double(), y_ref)
    exact("arg-max bytes", idx, byte_ref)
    y2 = torch.empty_like(y)
    L.check(lib.fsr_maxpool2_fwd(cd.code, xd.data_ptr(), y2.data_ptr(), None, n, h, w, c, ops._stream()), "fsr_maxpool2_fwd")
    exact("pooled output (no arg-max bytes)", y2.double(), y_ref)
    onehot = np.arange(4) == arg[..., None]                                     # (n, oh, ow, c, 4)
    for relu_mask in (0, 1):
        take = onehot & ((mx > 0)[..., None] if relu_mask else True)
        dwin = np.where(take, g.numpy()[..., None], 0.0)
        dx_ref = torch.from_numpy(dwin.reshape(n, h // 2, w // 2, c, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(n, h, w, c)).double()
        dx = torch.full((n, h, w, c), float("nan"), dtype=cd.torch_dtype, device=dev)
        L.check(lib.fsr_maxpool2_bwd_argmax(cd.code, gd.data_ptr(), idx.data_ptr(), dx.data_ptr(), n, h, w, c, relu_mask, ops._stream()),
                "fsr_maxpool2_bwd_argmax")
        exact("gradient from the arg-max bytes, relu_mask=%d" % relu_mask, dx.double(), dx_ref)
        dx = torch.full((n, h, w, c), float("nan"), dtype=cd.torch_dtype, device=dev)
        L.check(lib.fsr_maxpool2_bwd(cd.code, gd.data_ptr(), xd.data_ptr(), y.data_ptr(), dx.data_ptr(), n, h, w, c, relu_mask, ops._stream()),
                "fsr_maxpool2_bwd")
        exact("gradient from input and output, relu_mask=%d" % relu_mask, dx.double(), dx_ref)


# ------------------------------------------------------------------------------------------------- 3-channel images <-> padded NHWC
IMG_SCALE, IMG_SHIFT = (0.9, 1.7, -2.3), (0.4, -1.2, 0.05)
IMG_ROWS = [("f32", (2, 5, 7, 4)), ("bf16", (2, 5, 7, 8)), ("f16", (2, 5, 7, 8)), ("f32", (2, 5, 7, 32)), ("bf16", (2, 5, 7, 32)), ("f16", (2, 5, 7, 32)),
            ("f32", (1, 3, 1030, 64)),     # w * cpad / 4 = 16480 > 16384: the column loop wraps
            ("f32", (2, 300, 3, 32)),      # 600 rows on 512 row workgroups: the row loop strides, the bias partials take all 512 slots
            ("bf16", (2, 300, 3, 32))]
LAYOUTS = ("nchw", "nhwc", "crop")


@functools.lru_cache(maxsize=4)
def _img_inputs(nhw):
    n, h, w = nhw
    g = _gen(17)
    img, grad = torch.randn((n, 3, h, w), generator=g) * 0.7, torch.randn((n, 3, h, w), generator=g)
    y = (torch.rand((n, h, w, 3), generator=g) * 2 - 1) * 0.999       # any value in (-1, 1) serves as a tanh output
    return img, grad, y


def _layout(a, kind):
    """a: contiguous NCHW on its device -> the same values as NCHW contiguous, a channels-last view, or a cropped view."""
    n, c, h, w = a.shape
    if kind == "nchw":
        return a
    if kind == "nhwc":
        v = a.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert v.stride() == (h * w * 3, 1, w * 3, 3)
        return v
    big = torch.full((n, c, h + 3, w + 5), float("nan"), dtype=a.dtype, device=a.device)
    big[:, :, 1:1 + h, 2:2 + w] = a
    v = big[:, :, 1:1 + h, 2:2 + w]
    assert not v.is_contiguous()
    return v


def image64(img, a, b):
    """out = img a + b per channel;  s = |img a| + |b|."""
    a, b = np.asarray(a, F32).astype(F64).reshape(1, 3, 1, 1), np.asarray(b, F32).astype(F64).reshape(1, 3, 1, 1)
    return img * a + b, np.abs(img * a) + np.abs(b)


def image32(img, a, b):
    return img * np.asarray(a, F32).reshape(1, 3, 1, 1) + np.asarray(b, F32).reshape(1, 3, 1, 1)


def tanh64(g, y):
    """dz = g (1 - y^2);  s = |g| (1 + y^2)."""
    return g * (1 - y * y), np.abs(g) * (1 + y * y)


def tanh32(g, y):
    return g * (F32(1) - y * y)


def _nhwc3(a):
    return np.transpose(a, (0, 2, 3, 1))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("backend,cdn,shape", _cases(both=IMG_ROWS))
def test_stream_image_kernels(backend, cdn, shape, layout):
    """fsr_image_to_nhwc, fsr_tanh_bwd_to_nhwc (dz and the bias sums) and, in f32, fsr_tanh_bwd_image from three source layouts:
    the padding channels are exactly zero, the three real ones meet the per-element gate, the bias sums the sum bound."""
    dev = _select(backend)
    n, h, w, cpad = shape
    cd, lib = ops.Compute(cdn), L.lib()
    img, grad, y = _img_inputs((n, h, w))
    tag = "%s.%dx%dx%dx%d.%s" % (cdn, n, h, w, cpad, layout)
    src = _layout(img.to(dev), layout)
    out = torch.full((n, h, w, cpad), float("nan"), dtype=cd.torch_dtype, device=dev)
    L.check(lib.fsr_image_to_nhwc(cd.code, src.data_ptr(), *src.stride(), n, h, w, *IMG_SCALE, *IMG_SHIFT, out.data_ptr(), cpad, ops._stream()),
            "fsr_image_to_nhwc")
    got = out.cpu().double().numpy()
    assert (got[..., 3:] == 0).all(), "image_to_nhwc: padding channels are not zero"
    ref, s = image64(img.double().numpy(), IMG_SCALE, IMG_SHIFT)
    gate("image_to_nhwc." + tag, "image_to_nhwc", got[..., :3], _nhwc3(ref), _nhwc3(s), K_IMAGE, cdn)

    gsrc, yd = _layout(grad.to(dev), layout), y.to(dev)
    ref, s = tanh64(_nhwc3(grad.double().numpy()), y.double().numpy())
    scr = ops._workspace(lib.fsr_tanh_bwd_scratch(), dev)
    dz = torch.full((n, h, w, cpad), float("nan"), dtype=cd.torch_dtype, device=dev)
    dbias = torch.full((3,), float("nan"), dtype=torch.float32, device=dev)
    L.check(lib.fsr_tanh_bwd_to_nhwc(cd.code, gsrc.data_ptr(), *gsrc.stride(), yd.data_ptr(), n, h, w, dz.data_ptr(), cpad, dbias.data_ptr(),
                                     scr.data_ptr(), ops._stream()), "fsr_tanh_bwd_to_nhwc")
    got = dz.cpu().double().numpy()
    assert (got[..., 3:] == 0).all(), "tanh_bwd_to_nhwc: padding channels are not zero"
    gate("tanh_bwd_to_nhwc." + tag, "tanh_bwd_to_nhwc dz", got[..., :3], ref, s, K_TANH, cdn)
    sum_gate("tanh_bwd_to_nhwc.dbias." + tag, "tanh_bwd_to_nhwc bias sums", dbias.cpu().numpy(), ref.sum((0, 1, 2)), n * h * w, np.abs(ref).sum((0, 1, 2)))
    if cdn == "f32":
        dz3 = torch.full((n, h, w, 3), float("nan"), dtype=torch.float32, device=dev)
        dbias = torch.full((3,), float("nan"), dtype=torch.float32, device=dev)
        L.check(lib.fsr_tanh_bwd_image(gsrc.data_ptr(), *gsrc.stride(), yd.data_ptr(), n, h, w, dz3.data_ptr(), dbias.data_ptr(), scr.data_ptr(),
                                       ops._stream()), "fsr_tanh_bwd_image")
        gate("tanh_bwd_image." + tag, "tanh_bwd_image dz", dz3.cpu().numpy(), ref, s, K_TANH)
        sum_gate("tanh_bwd_image.dbias." + tag, "tanh_bwd_image bias sums", dbias.cpu().numpy(), ref.sum((0, 1, 2)), n * h * w, np.abs(ref).sum((0, 1, 2)))


# ------------------------------------------------------------------------------------------------- u8 -> float, add
@pytest.mark.parametrize("backend,count", _cases(both=[(1,), (2048 * 1024 + 5,)]))
def test_stream_u8_to_image_all_codes(backend, count):
    """fsr_u8_to_image equals uint8 -> float32 / 127.5 - 1 bit for bit on all 256 codes, past the 2048-workgroup grid cap."""
    dev = _select(backend)
    src = (torch.arange(count) % 256).to(torch.uint8) if count > 1 else torch.tensor([255], dtype=torch.uint8)
    ref = src.to(torch.float32) / 127.5 - 1
    sd = src.to(dev)
    out = torch.full((count,), float("nan"), dtype=torch.float32, device=dev)
    L.check(L.lib().fsr_u8_to_image(sd.data_ptr(), out.data_ptr(), count, ops._stream()), "fsr_u8_to_image")
    exact("u8_to_image", out, ref)


@pytest.mark.parametrize("backend,cdn,units", _cases(both=[(c, u) for c in ("f32", "bf16", "f16") for u in (1, 257)],
                                                     hip=[(c, 4096 * 256 + 3) for c in ("f32", "bf16")]))
def test_stream_add_on_integers(backend, cdn, units):
    """fsr_add on integer data (exact in every storage type), one unit up to past the 4096-workgroup grid cap."""
    dev = _select(backend)
    cd = ops.Compute(cdn)
    count = units * (4 if cdn == "f32" else 8)
    g = _gen(3)
    a, b = torch.randint(-60, 61, (count,), generator=g).float(), torch.randint(-60, 61, (count,), generator=g).float()
    ad, bd = a.to(cd.torch_dtype).to(dev), b.to(cd.torch_dtype).to(dev)
    out = torch.full((count,), float("nan"), dtype=cd.torch_dtype, device=dev)
    L.check(L.lib().fsr_add(cd.code, ad.data_ptr(), bd.data_ptr(), out.data_ptr(), count, ops._stream()), "fsr_add")
    exact("add", out.float(), a + b)


# ------------------------------------------------------------------------------------------------- losses
BCE_LOGITS = (0.0, 1e-4, -1e-4, 1.0, -1.0, 20.0, -20.0, 90.0, -90.0, 1e4, -1e4)
BCE_TARGETS = (0.0, 1.0, 0.3)
BCE_GSCALE = 0.37
BCE_COUNTS = (1, 257, 1024 * 2048 + 3)


@functools.lru_cache(maxsize=3)
def _bce_inputs(count):
    i = np.arange(count)
    return np.asarray(BCE_LOGITS, F32)[i % 11], np.asarray(BCE_TARGETS, F32)[(i // 11) % 3]      # every (logit, target) pair from count 33 on


def bce64(x, t, gscale, count):
    """loss = mean(term), term = max(x, 0) - x t + log1p(exp(-|x|)) >= 0, so sum |term| / count is the loss itself;
    dx = gs (sigmoid(x) - t), gs = gscale / count;  s = |gs| (sigmoid(x) + |t|)."""
    x, t = x.astype(F64), t.astype(F64)
    soft = np.log1p(np.exp(-np.abs(x)))
    gs = float(F32(gscale)) / count
    sg = np.where(x >= 0, 1 / (1 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1 + np.exp(-np.abs(x))))
    term = np.maximum(x, 0) - x * t + soft
    assert (term >= 0).all()
    return term.sum() / count, gs * (sg - t), abs(gs) * (sg + np.abs(t))


def bce_grad32(x, t, gscale, count):
    gs = F32(gscale) * (F32(1) / F32(count))
    with np.errstate(over="ignore"):
        e = np.exp(-x.astype(F64)).astype(F32)          # a correctly rounded expf, the same on every host
    return gs * (F32(1) / (F32(1) + e) - t)


@pytest.mark.parametrize("backend,count", _cases(both=[(c,) for c in BCE_COUNTS]))
def test_stream_bce_with_logits(backend, count):
    """fsr_bce_logits_fwd / _bwd on logits from 0 to +-1e4 (exp under- and overflow, subnormal sigmoid) with gscale != 1, one
    element up to past the 1024-workgroup grid cap: the mean meets the sum bound, the gradient the per-element gate."""
    dev = _select(backend)
    lib = L.lib()
    x, t = _bce_inputs(count)
    loss_ref, dx_ref, s = bce64(x, t, BCE_GSCALE, count)
    xd, td = _dev32(x, dev), _dev32(t, dev)
    scr = ops._workspace(lib.fsr_loss_scratch(), dev)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    L.check(lib.fsr_bce_logits_fwd(xd.data_ptr(), td.data_ptr(), loss.data_ptr(), scr.data_ptr(), count, ops._stream()), "fsr_bce_logits_fwd")
    sum_gate("bce_fwd.%d" % count, "BCE mean", loss.cpu().numpy(), np.reshape(loss_ref, (1,)), count, loss_ref, floor=TINY)
    gsc = torch.tensor([BCE_GSCALE]).to(dev)
    dx = torch.full((count,), float("nan"), dtype=torch.float32, device=dev)
    L.check(lib.fsr_bce_logits_bwd(xd.data_ptr(), td.data_ptr(), gsc.data_ptr(), dx.data_ptr(), count, ops._stream()), "fsr_bce_logits_bwd")
    gate("bce_bwd.%d" % count, "BCE gradient", dx.cpu().numpy(), dx_ref, s, K_BCE, floor=TINY)


SL1_DIFFS = (0.0, 1 - 2.0 ** -7, 1.0, 1 + 2.0 ** -7, 5.0)
SL1_UNITS = (1, 257, 1024 * 256 + 3)


@functools.lru_cache(maxsize=3)
def _sl1_inputs(count):
    """(a, b) with a - b in +-SL1_DIFFS, all three exact in bf16 and f16: b = 0 with +-d, b = -1 with +d, b = 1 with -d."""
    i = np.arange(count)
    d = np.asarray(SL1_DIFFS, F64)[i % 5]
    form = (i // 5) % 4
    b = np.choose(form, [0.0, 0.0, -1.0, 1.0])
    a = b + d * np.choose(form, [1.0, -1.0, 1.0, -1.0])
    return a, b


def sl1_64(a, b, gscale, count):
    """loss = mean(d < 1 ? d^2 / 2 : d - 1 / 2), d = |a - b|;  da = gs clamp(a - b, -1, 1), gs = gscale / count;  s = |da|."""
    d = np.abs(a - b)
    term = np.where(d < 1, 0.5 * d * d, d - 0.5)
    da = float(F32(gscale)) / count * np.clip(a - b, -1, 1)
    return term.sum() / count, da, np.abs(da)


def sl1_grad32(a, b, gscale, count):
    return F32(gscale) * (F32(1) / F32(count)) * np.clip(a - b, F32(-1), F32(1))


def _sl1_gscale(cdn):
    return 3.0 * 4096 if cdn == "f16" else 3.0       # f16 gradients of a mean over 2 M values need the loss scale


@pytest.mark.parametrize("backend,cdn,units", _cases(both=[(c, u) for c in ("f32", "bf16", "f16") for u in SL1_UNITS]))
def test_stream_smooth_l1(backend, cdn, units):
    """fsr_smooth_l1_fwd / _bwd on differences 0, 1 - 2^-7, exactly 1, 1 + 2^-7 and 5 of both signs (the branch is unambiguous in
    every storage type), one unit up to past the 1024-workgroup grid cap."""
    dev = _select(backend)
    cd, lib = ops.Compute(cdn), L.lib()
    count = units * (4 if cdn == "f32" else 8)
    a, b = _sl1_inputs(count)
    at, bt = torch.from_numpy(a).to(cd.torch_dtype), torch.from_numpy(b).to(cd.torch_dtype)
    assert torch.equal(at.double(), torch.from_numpy(a)) and torch.equal(bt.double(), torch.from_numpy(b)), "premise: inputs exact in " + cdn
    gscale = _sl1_gscale(cdn)
    loss_ref, da_ref, s = sl1_64(a, b, gscale, count)
    ad, bd = at.to(dev), bt.to(dev)
    scr = ops._workspace(lib.fsr_loss_scratch(), dev)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    L.check(lib.fsr_smooth_l1_fwd(cd.code, ad.data_ptr(), bd.data_ptr(), loss.data_ptr(), scr.data_ptr(), count, ops._stream()), "fsr_smooth_l1_fwd")
    sum_gate("smooth_l1_fwd.%s.%d" % (cdn, units), "smooth-L1 mean", loss.cpu().numpy(), np.reshape(loss_ref, (1,)), count, loss_ref)
    gsc = torch.tensor([gscale]).to(dev)
    da = torch.full((count,), float("nan"), dtype=cd.torch_dtype, device=dev)
    L.check(lib.fsr_smooth_l1_bwd(cd.code, ad.data_ptr(), bd.data_ptr(), gsc.data_ptr(), da.data_ptr(), count, ops._stream()), "fsr_smooth_l1_bwd")
    gate("smooth_l1_bwd.%s.%d" % (cdn, units), "smooth-L1 gradient", da.cpu().double().numpy(), da_ref, s, K_SL1, cdn)


# ------------------------------------------------------------------------------------------------- Conv2d(c -> 1, k = 1), integers
@pytest.mark.parametrize("with_dx", (True, False))
@pytest.mark.parametrize("backend,npix,c", _cases(both=[(1, 4), (7, 1024), (8195, 32)],      # cu = 1; cu = 256; forward grid wraps at 2048
                                                  hip=[(131100, 32)]))                         # backward grid wraps at 512 workgroups
def test_stream_conv1x1_on_integers(backend, npix, c, with_dx):
    """fsr_conv1x1_c1_fwd / _bwd in f32 on small integers: logits, dx, dw and db bit for bit, with and without dx."""
    dev = _select(backend)
    lib = L.lib()
    g = _gen(5)
    x = torch.randint(-2, 3, (npix, c), generator=g).double()
    wt = (torch.randint(0, 2, (c,), generator=g).double() * 2 - 1) * (torch.rand((c,), generator=g) < min(1.0, 36.0 / c)).double()
    b, gl = torch.tensor([3.0], dtype=torch.float64), torch.randint(-2, 3, (npix,), generator=g).double()
    assert float(x.abs().max()) * float(gl.abs().max()) * npix < 2 ** 24, "premise: the reductions stay below 2^24"
    xd, wd, bd, gd = (t.float().to(dev) for t in (x, wt, b, gl))
    logits = torch.full((npix,), float("nan"), dtype=torch.float32, device=dev)
    L.check(lib.fsr_conv1x1_c1_fwd(L.FSR_F32, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), logits.data_ptr(), npix, c, ops._stream()), "fsr_conv1x1_c1_fwd")
    exact("logits", logits, (x @ wt + b).float())
    scr = ops._workspace(lib.fsr_conv1x1_c1_bwd_scratch(c), dev)
    dx = torch.full((npix, c), float("nan"), dtype=torch.float32, device=dev) if with_dx else None
    dw = torch.full((c,), float("nan"), dtype=torch.float32, device=dev)
    db = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    L.check(lib.fsr_conv1x1_c1_bwd(L.FSR_F32, gd.data_ptr(), xd.data_ptr(), wd.data_ptr(), ops._p(dx), dw.data_ptr(), db.data_ptr(), scr.data_ptr(),
                                   npix, c, ops._stream()), "fsr_conv1x1_c1_bwd")
    if with_dx:
        exact("dx", dx, (gl[:, None] * wt[None, :]).float())
    exact("dw", dw, (gl @ x).float())
    exact("db", db, gl.sum().reshape(1).float())


# ------------------------------------------------------------------------------------------------- AdamW
ADAM = dict(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8)
ADAM_GSCALE, ADAM_LOSS_SCALE = 0.5, 1024.0
ADAM_BIG = 2048 * 1024 + 7                        # past the 2048-workgroup grid cap
ADAM_ROWS = [(s, wd, cnt) for s in (0, 9, 999) for wd in (0.0, 0.01) for cnt in (1, 1025)] + [(0, 0.01, ADAM_BIG), (999, 0.0, ADAM_BIG)]


@functools.lru_cache(maxsize=2)
def _adam_inputs(step0, count):
    """p ~ 1e-3 randn (so that the update, ~lr, is resolvable in p), g ~ 0.1 randn with every fifth exactly zero; fresh moments at
    step 0, else m ~ 0.05 randn and v in [1e-4, 1e-2]."""
    g = _gen(6 + step0)
    p, gr = (torch.randn(count, generator=g) * 1e-3).numpy(), (torch.randn(count, generator=g) * 0.1).numpy()
    gr[(np.arange(count) + 2) % 5 == 0] = 0.0
    if step0 == 0:
        m, v = np.zeros(count, F32), np.zeros(count, F32)
    else:
        m, v = (torch.randn(count, generator=g) * 0.05).numpy(), ((torch.rand(count, generator=g) + 0.01) * 0.01).numpy()
    return p, gr, m, v


def adam64(p, g, m, v, t, wd, gs, amplified=True):
    """The float64 recurrences from the float32 inputs and float32 hyper-parameters: m' = m + (g gs - m)(1 - b1),
    v' = v b2 + (1 - b2)(g gs)^2, upd = -(lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps), p' = p (1 - lr wd) + upd."""
    lr, b1, b2, eps, wd = (float(F32(k)) for k in (ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], wd))
    p, g, m, v = (a.astype(F64) for a in (p, g, m, v))
    gi = g * gs
    m1 = m + (gi - m) * (1 - b1)
    v1 = v * b2 + (1 - b2) * gi * gi
    step, denom = lr / (1 - b1 ** t), np.sqrt(v1) / np.sqrt(1 - b2 ** t) + eps
    upd = -step * m1 / denom
    amp = (0.5 * (1 + b2 ** t) / (1 - b2 ** t) + (1 + b1 ** t) / (1 - b1 ** t)) if amplified else 0.0
    s_m = np.abs(m) + np.abs(gi)            # >= |m'|: 0.9 m + 0.1 g gs cancels for some elements, and the update inherits m's error
    return dict(m=m1, v=v1, upd=upd, decayed=p * (1 - lr * wd), s_m=s_m, s_v=np.abs(v) + gi * gi, s_u=step * s_m / denom * (1 + amp) + np.abs(p))


def adam32(p, g, m, v, t, wd, gs, pow_ulps=0):
    """pow_ulps: both powers moved by that many float32 ulps, the error a device powf is allowed."""
    lr, b1, b2, eps, wd, t, one = F32(ADAM["lr"]), F32(ADAM["b1"]), F32(ADAM["b2"]), F32(ADAM["eps"]), F32(wd), F32(t), F32(1)
    pw1, pw2 = F32(float(b1) ** float(t)), F32(float(b2) ** float(t))     # a correctly rounded powf, the same on every host
    for _ in range(abs(pow_ulps)):
        pw1, pw2 = (np.nextafter(w, F32(np.sign(pow_ulps) * np.inf), dtype=F32) for w in (pw1, pw2))
    bc1 = one - pw1
    rs = one / np.sqrt(one - pw2)
    gi = g * F32(gs)
    pi = p * (one - lr * wd)
    mi = m + (gi - m) * (one - b1)
    vi = v * b2 + (one - b2) * gi * gi
    return pi - (lr / bc1) * (mi / (np.sqrt(vi) * rs + eps)), mi, vi


def _adam_check(tag, R, p0, pn, mn, vn):
    gate("adamw_m." + tag, "m", mn, R["m"], R["s_m"], K_ADAM_M)
    gate("adamw_v." + tag, "v", vn, R["v"], R["s_v"], K_ADAM_V)
    gate("adamw_update." + tag, "update p' - p (1 - lr wd)", np.asarray(pn, F64) - R["decayed"], R["upd"], R["s_u"], K_ADAM_U)


@pytest.mark.parametrize("scaled", (False, True))
@pytest.mark.parametrize("backend,step0,wd,count", _cases(both=ADAM_ROWS))
def test_stream_adamw_against_float64_recurrences(backend, step0, wd, count, scaled):
    """fsr_adamw_step and fsr_adamw_step_scaled (loss scale 1024, pre-scaled gradients): m, v and the update, each per element,
    at t = 1, 10 and 1000, with grad_scale = 0.5, zero gradients and both weight decays; the step counter advances by one."""
    dev = _select(backend)
    lib = L.lib()
    p, g, m, v = _adam_inputs(step0, count)
    R = adam64(p, g, m, v, step0 + 1, wd, ADAM_GSCALE)
    pd, md, vd = _dev32(p, dev), _dev32(m, dev), _dev32(v, dev)
    step = torch.tensor([float(step0)]).to(dev)
    hp = (ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], wd)
    if scaled:
        gd = _dev32(g * F32(ADAM_LOSS_SCALE), dev)
        state = torch.tensor([ADAM_LOSS_SCALE, 0.0, 0.0, 0.0]).to(dev)
        L.check(lib.fsr_adamw_step_scaled(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), count, *hp, step.data_ptr(), ADAM_GSCALE,
                                          state.data_ptr(), ops._stream()), "fsr_adamw_step_scaled")
        exact("loss-scale state", state, torch.tensor([ADAM_LOSS_SCALE, 0.0, 0.0, 0.0]))
    else:
        gd = _dev32(g, dev)
        L.check(lib.fsr_adamw_step(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), count, *hp, step.data_ptr(), ADAM_GSCALE,
                                   ops._stream()), "fsr_adamw_step")
    exact("step counter", step, torch.tensor([float(step0 + 1)]))
    _adam_check("%s.t%d.wd%g.%d" % ("scaled" if scaled else "plain", step0 + 1, wd, count), R, p, pd.cpu().numpy(), md.cpu().numpy(), vd.cpu().numpy())


# ------------------------------------------------------------------------------------------------- skipped steps, loss-scale state machine
@pytest.mark.parametrize("backend", BACKENDS)
def test_stream_skipped_step_leaves_everything_bit_identical(backend):
    """state[2] = 1 (a gradient overflowed): fsr_adamw_step_scaled leaves p, m, v and the step counter untouched."""
    dev = _select(backend)
    count = 1025
    p, g, m, v = _adam_inputs(9, count)
    pd, md, vd = _dev32(p, dev), _dev32(m, dev), _dev32(v, dev)
    gd = _dev32(g, dev)
    gd[3] = float("inf")
    step, state = torch.tensor([9.0]).to(dev), torch.tensor([1024.0, 5.0, 1.0, 2.0]).to(dev)
    L.check(L.lib().fsr_adamw_step_scaled(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), count, 1e-4, 0.9, 0.999, 1e-8, 0.01,
                                          step.data_ptr(), 0.5, state.data_ptr(), ops._stream()), "fsr_adamw_step_scaled")
    for what, got, want in (("p", pd, p), ("m", md, m), ("v", vd, v)):
        exact(what, got, torch.from_numpy(want))
    exact("step counter", step, torch.tensor([9.0]))
    exact("loss-scale state", state, torch.tensor([1024.0, 5.0, 1.0, 2.0]))


@pytest.mark.parametrize("backend,count", _cases(both=[(1024 * 256 + 77,), (1024 * 2048 + 3,)]))       # the second: past the 1024-workgroup cap
def test_stream_grad_nonfinite(backend, count):
    """fsr_grad_nonfinite: inf, -inf and nan at index 0, at count - 1 and at an index only the second grid pass reaches set the
    flag; a clean buffer (3.0e38 included) leaves it at 0; a set flag is not cleared."""
    dev = _select(backend)
    lib = L.lib()
    blocks = min(1024, (count + 2047) // 2048)
    second = blocks * 256 + 5                       # the first index of the second grid pass is blocks * 256
    assert blocks * 256 <= second < min(count - 1, 2 * blocks * 256)
    g = torch.randn(count, generator=_gen(2))
    g[1], g[second], g[count - 1] = 3.0e38, -3.0e38, 3.0e38
    gd = g.to(dev)

    def flag(start=0.0):
        state = torch.tensor([64.0, 3.0, start, 1.0]).to(dev)
        L.check(lib.fsr_grad_nonfinite(gd.data_ptr(), count, state.data_ptr(), ops._stream()), "fsr_grad_nonfinite")
        s = state.cpu()
        assert s[0] == 64.0 and s[1] == 3.0 and s[3] == 1.0
        return float(s[2])

    assert flag() == 0.0, "a clean buffer (+-3.0e38 included) was flagged"
    assert flag(1.0) == 1.0, "a set flag was cleared"
    for pos in (0, count - 1, second):
        for bad in (float("inf"), float("-inf"), float("nan")):
            keep = float(g[pos])
            gd[pos] = bad
            assert flag() == 1.0, "%r at index %d of %d was not flagged" % (bad, pos, count)
            gd[pos] = keep
    assert flag() == 0.0


@pytest.mark.parametrize("backend", BACKENDS)
def test_stream_loss_scale_state_machine(backend):
    """fsr_loss_scale_update on state = {scale, clean steps, non-finite flag, skipped steps}: growth exactly at the interval, the
    cap at 2^24, the floor at 1, back-off with the skipped-step counter."""
    dev = _select(backend)
    lib = L.lib()

    def run(state, interval=3.0, growth=2.0, backoff=0.5):
        s = torch.tensor(state).to(dev)
        L.check(lib.fsr_loss_scale_update(s.data_ptr(), interval, growth, backoff, ops._stream()), "fsr_loss_scale_update")
        return s.cpu().tolist()

    assert run([1024.0, 0.0, 0.0, 0.0]) == [1024.0, 1.0, 0.0, 0.0]                 # one below the interval: no growth yet
    assert run([1024.0, 1.0, 0.0, 0.0]) == [1024.0, 2.0, 0.0, 0.0]
    assert run([1024.0, 2.0, 0.0, 7.0]) == [2048.0, 0.0, 0.0, 7.0]                 # exactly at the interval
    assert run([2.0 ** 24, 2.0, 0.0, 0.0]) == [2.0 ** 24, 0.0, 0.0, 0.0]           # capped
    assert run([2.0 ** 23, 2.0, 0.0, 0.0], growth=4.0) == [2.0 ** 24, 0.0, 0.0, 0.0]
    assert run([1024.0, 2.0, 1.0, 0.0]) == [512.0, 0.0, 0.0, 1.0]                  # overflow: back off, count the skipped step
    assert run([1.5, 2.0, 1.0, 4.0]) == [1.0, 0.0, 0.0, 5.0]                       # floor
    assert run([1.0, 0.0, 1.0, 5.0]) == [1.0, 0.0, 0.0, 6.0]
    assert run([8.0, 0.0, 0.0, 0.0], interval=1.0) == [16.0, 0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------- the caps come from the formulas
def _units(got32, ref, s, floor=0.0):
    """max |restatement - ref64| in units of 2^-23 s_i."""
    got32 = np.asarray(got32)
    assert got32.dtype == F32, got32.dtype
    return float((np.abs(got32.astype(F64) - ref) / np.maximum(U * s + floor, 1e-300)).max())


def _restate_instnorm(which):
    worst = 0.0
    for cdn, shape in IN_ROWS + IN_BIG:
        I = _in_inputs(cdn, shape)
        hw = shape[1]
        x32, g32, r32 = I["x"].astype(F32), I["g"].astype(F32), I["res"].astype(F32)      # (storage values are float32 values)
        assert (x32.astype(F64) == I["x"]).all()
        for act in ACTS:
            slope = _eff_slope(act)
            keep = I["keep"] if act != L.ACT_NONE else True
            if which == "fwd":
                for res, res32 in ((None, None), (I["res"], r32)):
                    ref, s = in_fwd64(I["x"], I["mean"], I["rstd"], slope, res)
                    worst = max(worst, _units(in_fwd32(x32, I["stats"], hw, slope, res32), ref, np.where(keep, s, np.inf)))
            else:
                sums32 = in_sums64(I["x"], I["g"], I["mean"], I["rstd"], slope)[0].astype(F32)
                ref, s = in_apply64(I["x"], I["g"], I["mean"], I["rstd"], sums32, hw, slope)
                worst = max(worst, _units(in_apply32(x32, g32, I["stats"], sums32, hw, slope), ref, np.where(keep, s, np.inf)))
    return worst


def _restate_image():
    worst = 0.0
    for nhw in sorted(set(s[:3] for _, s in IMG_ROWS)):
        img = _img_inputs(nhw)[0]
        ref, s = image64(img.double().numpy(), IMG_SCALE, IMG_SHIFT)
        worst = max(worst, _units(image32(img.numpy(), IMG_SCALE, IMG_SHIFT), ref, s))
    return worst


def _restate_tanh():
    worst = 0.0
    for nhw in sorted(set(s[:3] for _, s in IMG_ROWS)):
        _, grad, y = _img_inputs(nhw)
        ref, s = tanh64(_nhwc3(grad.double().numpy()), y.double().numpy())
        worst = max(worst, _units(tanh32(_nhwc3(grad.numpy()), y.numpy()), ref, s))
    return worst


def _restate_bce():
    worst = 0.0
    for count in BCE_COUNTS:
        x, t = _bce_inputs(count)
        _, ref, s = bce64(x, t, BCE_GSCALE, count)
        worst = max(worst, _units(bce_grad32(x, t, BCE_GSCALE, count), ref, s, floor=TINY))
    return worst


def _restate_sl1():
    worst = 0.0
    for cdn in ("f32", "bf16", "f16"):
        for units in SL1_UNITS:
            count = units * (4 if cdn == "f32" else 8)
            a, b = _sl1_inputs(count)
            _, ref, s = sl1_64(a, b, _sl1_gscale(cdn), count)
            worst = max(worst, _units(sl1_grad32(a.astype(F32), b.astype(F32), _sl1_gscale(cdn), count), ref, s))
    return worst


def _restate_adam(which):
    worst = 0.0
    for step0, wd, count in ADAM_ROWS:
        p, g, m, v = _adam_inputs(step0, count)
        R = adam64(p, g, m, v, step0 + 1, wd, ADAM_GSCALE)
        pn, mn, vn = adam32(p, g, m, v, step0 + 1, wd, ADAM_GSCALE)
        if which == "m":
            worst = max(worst, _units(mn, R["m"], R["s_m"]))
        elif which == "v":
            worst = max(worst, _units(vn, R["v"], R["s_v"]))
        else:
            worst = max(worst, float((np.abs(pn.astype(F64) - R["decayed"] - R["upd"]) / (U * R["s_u"])).max()))
    return worst


def _adam_update_units(step0, pow_ulps, amplified=True):
    """Largest |restated update - ref64| / (2^-23 s_u) over the rows of one step count."""
    worst = 0.0
    for s0, wd, count in ADAM_ROWS:
        if s0 == step0:
            p, g, m, v = _adam_inputs(s0, count)
            R = adam64(p, g, m, v, s0 + 1, wd, ADAM_GSCALE, amplified)
            pn = adam32(p, g, m, v, s0 + 1, wd, ADAM_GSCALE, pow_ulps)[0]
            worst = max(worst, float((np.abs(pn.astype(F64) - R["decayed"] - R["upd"]) / (U * R["s_u"])).max()))
    return worst


RESTATEMENTS = {"instnorm_fwd": (K_IN_FWD, lambda: _restate_instnorm("fwd")), "instnorm_apply": (K_IN_APPLY, lambda: _restate_instnorm("apply")),
                "image_to_nhwc": (K_IMAGE, _restate_image), "tanh_bwd": (K_TANH, _restate_tanh), "bce_bwd": (K_BCE, _restate_bce),
                "smooth_l1_bwd": (K_SL1, _restate_sl1), "adamw_m": (K_ADAM_M, lambda: _restate_adam("m")),
                "adamw_v": (K_ADAM_V, lambda: _restate_adam("v")), "adamw_update": (K_ADAM_U, lambda: _restate_adam("u"))}


@pytest.mark.parametrize("family", sorted(RESTATEMENTS))
def test_float32_restatement_is_inside_a_third_of_the_caps(family):
    """No kernel is launched.  The kernel's statements in float32 numpy (one rounding per operation, no fused multiply-add) stay
    within K / 3 units of 2^-23 s_i of the float64 reference on the inputs of every case.  (The module docstring lists the measured
    figures: none of them is inside K / 6, so each K is the smallest power of two that leaves the factor three.)"""
    K, fn = RESTATEMENTS[family]
    worst = report("stream.restatement.%s.K%d" % (family, K), fn())
    assert worst <= K / 3.0, "%s: the float32 restatement reaches %.3g units, the cap is K = %d" % (family, worst, K)


@pytest.mark.parametrize("step0", (0, 9, 999))
def test_adamw_update_cap_holds_one_ulp_of_powf_and_needs_its_amplification(step0):
    """No kernel is launched.  The restatement with BOTH powers off by one float32 ulp (either way), which is what a device powf
    may return, still stays within a third of the update's cap at t = 1, 10 and 1000 -- and at t = 1 and 10, without A(t) in s_i,
    it would overshoot the cap: the amplification is what the formula needs, not slack."""
    t = step0 + 1
    for ulps in (-1, 1):
        with_a = report("stream.restatement.adamw_update.t%d.pow%+dulp" % (t, ulps), _adam_update_units(step0, ulps))
        assert with_a <= K_ADAM_U / 3.0, (t, ulps, with_a)
        without = report("stream.restatement.adamw_update.t%d.pow%+dulp.no_amplification" % (t, ulps), _adam_update_units(step0, ulps, False))
        assert t == 1000 or without > K_ADAM_U, (t, ulps, without)


# ------------------------------------------------------------------------------------------------- why this file exists
def test_stream_gates_are_sharper_than_the_tolerance_gates():
    """No kernel is launched.  Three one-element errors in the float64 reference of the bf16 (2, 130, 64) PReLU case and of one
    AdamW step -- (a) one pixel left out of the middle slab's sum gz xh of one channel, (b) one 8-channel unit normalised with its
    neighbour's mean at one pixel, (c) one element's v decayed as b2 (v + (1 - b2) g^2), a misplaced parenthesis -- stay UNDER the
    gates of test_instnorm_act_residual_fwd_bwd (relerr 1e-2 on the bf16 output, 2e-2 on dx) and of test_losses_and_adamw
    (|p - p_ref| < 1e-6); the gates of this file reject all three and pass the uncorrupted values rounded to storage."""
    cdn, shape, act = "bf16", (2, 130, 64), L.ACT_PRELU
    n, hw, c = shape
    I = _in_inputs(cdn, shape)
    x, g, mean, rstd, slope = I["x"], I["g"], I["mean"], I["rstd"], _eff_slope(act)
    bf = lambda a: torch.from_numpy(a).bfloat16().double().numpy()
    # (a) pixel 87 = the last pixel of slab 1 (pixels 44 .. 87), image 1, channel 9
    sums, mags, _, _ = in_sums64(x, g, mean, rstd, slope)
    xh = (x - mean) * rstd
    gz = g * np.where(xh > 0, 1.0, slope)
    bad = sums.copy()
    bad[1, 9, 1] -= gz[1, 87, 9] * xh[1, 87, 9]
    dx, s_dx = in_apply64(x, g, mean, rstd, sums.astype(F32), hw, slope)
    dx_bad, _ = in_apply64(x, g, mean, rstd, bad.astype(F32), hw, slope)
    assert relerr(torch.from_numpy(bf(dx_bad)), torch.from_numpy(dx)) < 2e-2              # the old gate on dx passes it
    with pytest.raises(AssertionError):
        sum_gate(None, "pixel left out of sum gz xh", bad.astype(F32), sums, hw, mags)
    sum_gate(None, "uncorrupted sums", sums.astype(F32), sums, hw, mags)
    gate(None, "uncorrupted dx", bf(dx), dx, s_dx, K_IN_APPLY, cdn)
    # (b) the (image, pixel, unit) where the neighbour's mean does the least harm: even that one is rejected
    y, s_y = in_fwd64(x, mean, rstd, slope, I["res"])
    shifted = np.roll(mean.reshape(n, 1, c // 8, 8), -1, axis=2).reshape(n, 1, c)          # unit u takes the mean of unit u + 1
    y_all, _ = in_fwd64(x, shifted, rstd, slope, I["res"])
    harm = np.abs(y_all - y).reshape(n, hw, c // 8, 8).max(-1)
    i, p, u = np.unravel_index(int(np.argmin(harm)), harm.shape)
    y_bad = y.copy()
    y_bad[i, p, 8 * u:8 * u + 8] = y_all[i, p, 8 * u:8 * u + 8]
    assert harm[i, p, u] > 0
    assert relerr(torch.from_numpy(bf(y_bad)), torch.from_numpy(y)) < 1e-2                # the old gate on the output passes it
    with pytest.raises(AssertionError):
        gate(None, "neighbour's mean", bf(y_bad), y, s_y, K_IN_FWD, cdn)
    gate(None, "uncorrupted forward", bf(y), y, s_y, K_IN_FWD, cdn)
    # (c) the first step of the old test: lr 1e-4, p ~ N(0, 1); v is never compared there
    gen = _gen(6)
    p0, g0 = torch.randn(3000, generator=gen).numpy(), (torch.randn(3000, generator=gen) * 0.1).numpy()
    z = np.zeros(3000, F32)
    R = adam64(p0, g0, z, z, 1, 0.01, 1.0)
    b2 = float(F32(ADAM["b2"]))
    v_bad = R["v"].copy()
    v_bad[1234] = b2 * (1 - b2) * float(g0[1234]) ** 2
    p_ref = R["decayed"] + R["upd"]
    p_bad = p_ref.copy()
    p_bad[1234] = R["decayed"][1234] - (float(F32(1e-4)) / (1 - float(F32(0.9)))) * R["m"][1234] / (np.sqrt(v_bad[1234] / (1 - b2)) + float(F32(1e-8)))
    assert 0 < np.abs(p_bad - p_ref).max() < 1e-6                                          # the old gate on p passes it
    with pytest.raises(AssertionError):
        gate(None, "v with a misplaced beta2", v_bad.astype(F32), R["v"], R["s_v"], K_ADAM_V)
    gate(None, "uncorrupted v", R["v"].astype(F32), R["v"], R["s_v"], K_ADAM_V)
