"""Float64-referenced parity of the strided element-wise loss family (csrc/elem_loss.hip: fsr_elem_loss_fwd / _bwd, ops.elem_loss),
called through the C ABI on the emulator and the MI355X, with the gates of test_stream_exact.py:

    gradient, element by element    |got_i - ref64_i|  <=  K 2^-23 s_i          s_i = |gs psi'(d_i)|,  gs = gscale / count
    loss                            |got - ref64|      <=  (count + 8) 2^-24 sum_i psi(d_i)

K per kind is derived as in that file: the smallest power of two (>= 1) for which the float32-numpy restatement of the kernel's
statements (one rounding per operation, no fused multiply-add) stays inside ONE THIRD of the cap on the inputs of every case
(test_float32_restatement_is_inside_a_third_of_the_caps; none of the figures is inside K / 6).  The restatement's roundings: gs is
two (1 / count, the product with gscale), the product gs psi' a third; psi' itself is exact for L1 and smooth-L1 (a sign, a clamp)
and for MSE (2 d), and three more for Charbonnier (d d, + eps eps, the square root) plus the division.

Charbonnier is the one kind that calls sqrtf and divides on the device, and either may be an ulp off numpy's correctly rounded
result.  That is allowed EXPLICITLY: its gradient cap is (K + CHARB_DEVICE_ULPS) units with CHARB_DEVICE_ULPS = 2 -- one ulp
(at most one unit of 2^-23 s_i) for the square root, one for the quotient -- and its loss cap carries one ulp of every term
(floor = 2^-23 sum psi) for the square root.  The no-launch test moves both results of the restatement by one float32 ulp either way
and asserts K / 3 + 2 units.  No other kind gets the allowance.

Measured maximum of |result - ref64| / (2^-23 s_i), i.e. in the units K counts (MI355X: the largest error / cap ratio of the
f32 cases times the cap's units, from the parity-error log, elem.*):

    kind           K    restatement   restatement, sqrt and quotient -1 / +1 ulp   emulator   MI355X
    l1             2    0.42          -                                            0.42       0.42
    smooth_l1      2    0.66          -                                            0.66       0.66
    charbonnier    4    0.81          0.95 / 1.07                                  0.81       0.81
    mse            2    0.66          -                                            0.66       0.66

(The emulator and the MI355X reproduce the restatement to the digit on these inputs: gs and its product are plain IEEE operations, and
the MI355X's sqrtf and division returned the correctly rounded results here, so the two allowed units were not used; the fused
d d + eps eps moved no maximum.  The losses stay below 0.021 of the textbook bound of the sum.)

Inputs hit every branch unambiguously: d = a - b is EXACT in float32 (asserted) and takes the values 0, +-2^-20, +-(1 - 2^-7), +-1,
+-(1 + 2^-7), +-5 (smooth-L1's branch, the sign at 0) and, for Charbonnier with eps = float32(1e-3), +-eps 2^-10 (well below),
+-eps (equal) and +-eps 2^6 (well above).  An element with d = 0 has a cap of 0: its gradient must be exactly 0.
"""
import functools

import numpy as np
import pytest
import torch

from backend import BACKENDS, L, ops, report
from test_stream_exact import _select, gate, sum_gate

F32, F64 = np.float32, np.float64
U = 2.0 ** -23
GPU = pytest.mark.gpu
KINDS = ("l1", "smooth_l1", "charbonnier", "mse")
CODES = {"l1": L.LOSS_L1, "smooth_l1": L.LOSS_SMOOTH_L1, "charbonnier": L.LOSS_CHARBONNIER, "mse": L.LOSS_MSE}
K_GRAD = {"l1": 2, "smooth_l1": 2, "charbonnier": 4, "mse": 2}
CHARB_DEVICE_ULPS = 2           # one ulp of the device's sqrtf, one of its division: allowed explicitly, on top of K
EPS32 = F32(1e-3)               # the Python default (LapSRN's), as the float the C call receives
GSCALE = 0.37
DYADIC = (0.0, 2.0 ** -20, 1 - 2.0 ** -7, 1.0, 1 + 2.0 ** -7, 5.0)
AROUND_EPS = (float(EPS32) * 2.0 ** -10, float(EPS32), float(EPS32) * 2.0 ** 6)
SMALL_SHAPES = ((1, 1, 1, 1), (2, 3, 5, 7), (2, 1, 4, 4))
BIG_SHAPE = (1, 3, 520, 513)    # 266760 pixels: 1043 workgroups of 256 wanted, 1024 launched -- the grid-stride loop's second trip
LAYOUTS = ("a_nhwc", "b_nhwc", "contiguous", "b_slice")


# ------------------------------------------------------------------------------------------------- inputs and references
@functools.lru_cache(maxsize=8)
def _inputs(shape):
    """float64 (a, b) of `shape`, both exact in float32, with a - b exact in float32 and cycling through +-DYADIC (b = 0, -1 or 1) and
    +-AROUND_EPS (b = 0: eps is no dyadic number, so a = d itself)."""
    count = int(np.prod(shape))
    i = np.arange(count)
    values = np.asarray(DYADIC + AROUND_EPS, F64)
    which = i % len(values)
    d = values[which]
    form = (i // len(values)) % 4
    form = np.where(which >= len(DYADIC), form % 2, form)
    b = np.choose(form, [0.0, 0.0, -1.0, 1.0])
    a = b + d * np.choose(form, [1.0, -1.0, 1.0, -1.0])
    a32, b32 = a.astype(F32), b.astype(F32)
    assert (a32.astype(F64) == a).all() and (b32.astype(F64) == b).all(), "premise: the operands are float32 numbers"
    assert ((a32 - b32).astype(F64) == a - b).all(), "premise: a - b is exact in float32"
    return a.reshape(shape), b.reshape(shape)


def psi64(kind, d, eps=float(EPS32)):
    """(psi(d), psi'(d)) in float64: the documented formulas of include/fsr_hip.h."""
    if kind == "l1":
        return np.abs(d), np.sign(d)
    if kind == "smooth_l1":
        ad = np.abs(d)
        return np.where(ad < 1, 0.5 * d * d, ad - 0.5), np.clip(d, -1, 1)
    if kind == "charbonnier":
        r = np.sqrt(d * d + eps * eps)
        return r, d / r
    return d * d, 2 * d


def ref64(kind, a, b, gscale=GSCALE, eps=float(EPS32)):
    """(loss, da, s): the mean of psi, gs psi' with gs = float32(gscale) / count, and the gradient's scale s_i = |da_i|."""
    p, dp = psi64(kind, a - b, eps)
    da = float(F32(gscale)) / a.size * dp
    return p.sum() / a.size, da, np.abs(da)


def grad32(kind, a32, b32, gscale=GSCALE, eps32=EPS32, ulps=0):
    """The statements of elem_loss_bwd_kernel in float32 numpy.  ulps: the square root and the quotient moved by that many float32
    ulps (what a device sqrtf / division may return)."""
    assert a32.dtype == F32 and b32.dtype == F32
    d = a32 - b32
    gs = F32(gscale) * (F32(1) / F32(a32.size))
    if kind == "l1":
        dp = np.sign(d)
    elif kind == "smooth_l1":
        dp = np.minimum(np.maximum(d, F32(-1)), F32(1))
    elif kind == "charbonnier":
        r = np.sqrt(d * d + eps32 * eps32)
        q = d / _nudge(r, ulps)
        dp = _nudge(q, ulps)
    else:
        dp = F32(2) * d
    out = gs * dp
    assert out.dtype == F32
    return out


def _nudge(x, ulps):
    """x moved `ulps` float32 steps away from (> 0) or towards (< 0) zero; zeros stay."""
    toward = np.where(x == 0, x, np.copysign(F32(np.inf), x)) if ulps > 0 else np.zeros_like(x)
    for _ in range(abs(ulps)):
        x = np.nextafter(x, toward).astype(F32)
    return x


def _units(got32, ref, s):
    """max |restatement - ref64| in units of 2^-23 s_i (an element with s_i = 0 must be exact)."""
    err = np.abs(np.asarray(got32).astype(F64) - ref)
    assert (err[s == 0] == 0).all()
    return float((err[s > 0] / (U * s[s > 0])).max()) if (s > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------- layouts
def _nhwc_view(x):
    """The (N,C,H,W) view of an NHWC buffer holding x: what the generator's head hands out."""
    return x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _sliced(x, fill):
    """x as the [:, :, 1:-1, 2:-1] slice of a larger tensor whose border holds `fill` (a read of the border shows in every result)."""
    n, c, h, w = x.shape
    big = torch.full((n, c, h + 2, w + 3), fill, dtype=x.dtype, device=x.device)
    view = big[:, :, 1:-1, 2:-1]
    view.copy_(x)
    return view


def _layout(a, b, layout):
    if layout == "a_nhwc":
        return _nhwc_view(a), b.contiguous()
    if layout == "b_nhwc":
        return a.contiguous(), _nhwc_view(b)
    if layout == "b_slice":
        return a.contiguous(), _sliced(b, 1e30)
    return a.contiguous(), b.contiguous()


def _call_fwd(kind, a, b, eps=EPS32):
    lib = L.lib()
    scr = ops._workspace(lib.fsr_elem_loss_scratch(), a.device)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=a.device)
    L.check(lib.fsr_elem_loss_fwd(CODES[kind], float(eps), a.data_ptr(), *a.stride(), b.data_ptr(), *b.stride(), *a.shape, loss.data_ptr(),
                                  scr.data_ptr(), ops._stream()), "fsr_elem_loss_fwd")
    return loss


def _call_bwd(kind, a, b, gscale=GSCALE, eps=EPS32):
    """da: NaN-filled storage with a's strides (for the NHWC view: the whole NHWC buffer), so an element the kernel skips shows."""
    da = torch.full_like(a, float("nan"))          # preserve_format: a's strides for the dense layouts used here
    assert da.stride() == a.stride()
    gsc = torch.tensor([gscale], dtype=torch.float32).to(a.device)
    L.check(L.lib().fsr_elem_loss_bwd(CODES[kind], float(eps), a.data_ptr(), *a.stride(), b.data_ptr(), *b.stride(), gsc.data_ptr(),
                                      da.data_ptr(), *a.shape, ops._stream()), "fsr_elem_loss_bwd")
    return da


def _check_case(backend, kind, shape, layout):
    dev = _select(backend)
    a64, b64 = _inputs(shape)
    a, b = _layout(torch.from_numpy(a64).float().to(dev), torch.from_numpy(b64).float().to(dev), layout)
    loss_ref, da_ref, s = ref64(kind, a64, b64)
    tag = "%s.%s.%s" % (kind, "x".join(map(str, shape)), layout)
    charb = kind == "charbonnier"
    loss = _call_fwd(kind, a, b)
    print("elem_loss %s: loss %.9g, float64 %.17g" % (tag, float(loss), loss_ref))
    sum_gate("elem.fwd." + tag, "%s mean" % kind, loss.cpu().numpy(), np.reshape(loss_ref, (1,)), a64.size, loss_ref,
             floor=U * loss_ref if charb else 0.0)
    da = _call_bwd(kind, a, b)
    assert da.stride() == a.stride()
    K = K_GRAD[kind] + (CHARB_DEVICE_ULPS if charb else 0)
    gate("elem.bwd." + tag, "%s gradient" % kind, da.cpu().double().numpy(), da_ref, s, K)
    exact0 = da.cpu().numpy()[a64 == b64]
    assert (exact0 == 0).all(), "d = 0 must give a gradient of exactly 0"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_elem_loss_against_float64(backend, kind, shape, layout):
    """Loss and gradient of every kind, in every layout pairing, at one element, at an odd shape and at the logits' shape: both
    operands are read through their own strides and the gradient comes back fully written, with a's strides."""
    _check_case(backend, kind, shape, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_elem_loss_past_the_workgroup_cap(backend, kind, layout):
    """266760 pixels want 1043 workgroups and get 1024: the grid-stride loop takes a second trip for some threads, the row / column
    split runs (the slice) or is merged away (the other layouts), and 1024 partials meet in the order-fixed second level."""
    _check_case(backend, kind, BIG_SHAPE, layout)


# ------------------------------------------------------------------------------------------------- against the existing smooth-L1 kernels
def _exact_sum_inputs(shape):
    """d in {0, +-0.5, +-1, +-2}: every smooth-L1 term is a multiple of 2^-3 and every partial sum stays below 2^21, so the sum is exact
    in float32 in ANY order -- the two kernels walk the elements in different orders (pixels vs. 4-float units)."""
    count = int(np.prod(shape))
    i = np.arange(count)
    d = np.asarray([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])[i % 7]
    b = np.asarray([0.0, -1.0, 1.0, 0.25])[(i // 7) % 4]
    return (b + d).reshape(shape), b.reshape(shape)


@pytest.mark.parametrize("backend,shape", [("emu", (2, 3, 4, 6)), ("emu", (2, 1, 4, 4)),
                                           pytest.param("hip", (2, 3, 4, 6), marks=GPU), pytest.param("hip", (2, 1, 4, 4), marks=GPU),
                                           pytest.param("hip", (1, 3, 520, 512), marks=GPU)])
def test_smooth_l1_kind_equals_the_existing_kernels(backend, shape):
    """FSR_LOSS_SMOOTH_L1 on contiguous operands == fsr_smooth_l1_fwd / _bwd, torch.equal: the gradient on the branch-hitting inputs
    of this file and on inputs whose sum is exact, the loss on the latter (see _exact_sum_inputs: the summation orders differ)."""
    dev = _select(backend)
    lib = L.lib()
    count = int(np.prod(shape))

    def old(a, b):
        scr = ops._workspace(lib.fsr_loss_scratch(), dev)
        loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
        L.check(lib.fsr_smooth_l1_fwd(L.FSR_F32, a.data_ptr(), b.data_ptr(), loss.data_ptr(), scr.data_ptr(), count, ops._stream()), "fsr_smooth_l1_fwd")
        gsc = torch.tensor([GSCALE], dtype=torch.float32).to(dev)
        da = torch.full_like(a, float("nan"))
        L.check(lib.fsr_smooth_l1_bwd(L.FSR_F32, a.data_ptr(), b.data_ptr(), gsc.data_ptr(), da.data_ptr(), count, ops._stream()), "fsr_smooth_l1_bwd")
        return loss, da

    a64, b64 = _exact_sum_inputs(shape)
    a, b = torch.from_numpy(a64).float().to(dev), torch.from_numpy(b64).float().to(dev)
    loss_old, da_old = old(a, b)
    terms = psi64("smooth_l1", a64 - b64)[0].reshape(-1)
    assert (np.cumsum(terms.astype(F32), dtype=F32).astype(F64) == np.cumsum(terms)).all(), "premise: float32 adds these terms exactly"
    assert torch.equal(_call_fwd("smooth_l1", a, b), loss_old)
    assert torch.equal(_call_bwd("smooth_l1", a, b), da_old)
    a64, b64 = _inputs(shape)
    a, b = torch.from_numpy(a64).float().to(dev), torch.from_numpy(b64).float().to(dev)
    assert torch.equal(_call_bwd("smooth_l1", a, b), old(a, b)[1])


# ------------------------------------------------------------------------------------------------- ops.elem_loss: autograd, refusals
@pytest.mark.parametrize("backend", BACKENDS)
def test_ops_elem_loss_autograd_keeps_the_strides_and_copies_nothing(backend):
    """ops.elem_loss on the NCHW view of an NHWC buffer against a slice: the values of the direct calls, a gradient with a's strides,
    the dynamic seed read from device memory."""
    dev = _select(backend)
    a64, b64 = _inputs((2, 3, 5, 7))
    a0, b = _nhwc_view(torch.from_numpy(a64).float().to(dev)), _sliced(torch.from_numpy(b64).float().to(dev), 1e30)
    for kind in KINDS:
        a = a0.detach().requires_grad_(True)
        loss = ops.elem_loss(a, b, kind, eps=float(EPS32))
        assert loss.shape == () and torch.equal(loss.detach().reshape(1), _call_fwd(kind, a0, b))
        loss.backward(torch.tensor(GSCALE, dtype=torch.float32, device=dev))
        assert a.grad.stride() == a.stride() and torch.equal(a.grad, _call_bwd(kind, a0, b))


def test_elem_loss_refusals():
    """Nothing is launched for: 16-bit operands, a shape mismatch, a target that requires a gradient, an unknown kind, eps <= 0 (the
    Python layer); an unknown kind code, a bad eps, negative, zero and overlapping strides, 2^31 elements (the C entry points)."""
    dev = _select("emu")
    a, b = torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, 4, 5)
    for bad_a, bad_b in ((a.half(), b.half()), (a.bfloat16(), b.bfloat16()), (a, b.half())):
        with pytest.raises(L.FsrError, match="float32"):
            ops.elem_loss(bad_a, bad_b)
    with pytest.raises(L.FsrError, match="one shape"):
        ops.elem_loss(a, torch.zeros(2, 3, 4, 6))
    with pytest.raises(L.FsrError, match="one shape"):
        ops.elem_loss(a.reshape(6, 4, 5), b.reshape(6, 4, 5))
    with pytest.raises(L.FsrError, match="target"):
        ops.elem_loss(a, b.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="unknown kind"):
        ops.elem_loss(a, b, "huber")
    for eps in (0.0, -1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            ops.elem_loss(a, b, "charbonnier", eps=eps)
    lib = L.lib()
    loss, scr, g, da = torch.zeros(1), torch.zeros(1024), torch.ones(1), torch.zeros(2, 3, 4, 5)
    st = a.stride()

    def fwd(kind=L.LOSS_L1, eps=1e-3, sa=st, sb=st, shape=(2, 3, 4, 5)):
        return lib.fsr_elem_loss_fwd(kind, eps, a.data_ptr(), *sa, b.data_ptr(), *sb, *shape, loss.data_ptr(), scr.data_ptr(), None)

    def bwd(kind=L.LOSS_L1, eps=1e-3, sa=st, sb=st, shape=(2, 3, 4, 5)):
        return lib.fsr_elem_loss_bwd(kind, eps, a.data_ptr(), *sa, b.data_ptr(), *sb, g.data_ptr(), da.data_ptr(), *shape, None)

    for call in (fwd, bwd):
        assert call() == 0
        assert call(kind=4) < 0 and b"unknown loss kind" in lib.fsr_last_error()
        assert call(kind=-1) < 0
        for eps in (0.0, -1.0, float("nan"), float("inf")):
            assert call(kind=L.LOSS_CHARBONNIER, eps=eps) < 0 and b"eps" in lib.fsr_last_error()
        assert call(kind=L.LOSS_MSE, eps=0.0) == 0                       # the other kinds ignore it
        assert call(sa=(60, 20, -5, 1)) < 0 and b"strides" in lib.fsr_last_error()       # negative
        assert call(sb=(0, 20, 5, 1)) < 0                                # every image the same memory
        assert call(sb=(60, 20, 5, 0)) < 0                               # a broadcast column
        assert call(sa=(60, 20, 4, 1)) < 0                               # rows 4 apart hold 5 columns: overlap
        assert call(sb=(3, 1, 15, 3), shape=(2, 3, 4, 5)) < 0            # NHWC strides of ONE image for a batch of two: images overlap
        assert call(sa=(999, 999, 999, 999), sb=(7, 7, 7, 7), shape=(1, 1, 1, 1)) == 0   # axes of length 1: strides are not read
        assert call(shape=(2, 0, 4, 5)) < 0
        assert call(shape=(1 << 15, 1, 1 << 8, 1 << 8), sa=(1 << 16, 1 << 16, 1 << 8, 1), sb=(1 << 16, 1 << 16, 1 << 8, 1)) < 0
        assert b"2^31" in lib.fsr_last_error()
    assert lib.fsr_elem_loss_fwd(L.LOSS_L1, 1e-3, None, *st, b.data_ptr(), *st, 2, 3, 4, 5, loss.data_ptr(), scr.data_ptr(), None) < 0
    assert lib.fsr_elem_loss_bwd(L.LOSS_L1, 1e-3, a.data_ptr(), *st, b.data_ptr(), *st, None, da.data_ptr(), 2, 3, 4, 5, None) < 0


# ------------------------------------------------------------------------------------------------- the caps come from the formulas
ALL_SHAPES = SMALL_SHAPES + (BIG_SHAPE,)


def _restated_units(kind, ulps=0):
    worst = 0.0
    for shape in ALL_SHAPES:
        a64, b64 = _inputs(shape)
        _, ref, s = ref64(kind, a64, b64)
        worst = max(worst, _units(grad32(kind, a64.astype(F32), b64.astype(F32), ulps=ulps), ref, s))
    return worst


@pytest.mark.parametrize("kind", KINDS)
def test_float32_restatement_is_inside_a_third_of_the_caps(kind):
    """No kernel is launched.  The kernel's statements in float32 numpy stay within K / 3 units of 2^-23 s_i of the float64 reference
    on the inputs of every case, and not within K / 6 (K > 1): each K is the smallest power of two that leaves the factor three.
    Charbonnier with the square root and the quotient each one float32 ulp off, either way, stays within K / 3 + CHARB_DEVICE_ULPS."""
    K = K_GRAD[kind]
    worst = report("elem.restatement.%s.K%d" % (kind, K), _restated_units(kind))
    assert worst <= K / 3.0, "%s: the float32 restatement reaches %.3g units, the cap is K = %d" % (kind, worst, K)
    assert K == 1 or worst > K / 6.0, "%s: K = %d is not the smallest power of two (%.3g units)" % (kind, K, worst)
    if kind == "charbonnier":
        for ulps in (-1, 1):
            moved = report("elem.restatement.charbonnier.sqrt_div%+dulp" % ulps, _restated_units(kind, ulps))
            assert worst < moved <= K / 3.0 + CHARB_DEVICE_ULPS, (ulps, moved)


def test_wrong_references_fail_the_gates():
    """No kernel is launched.  Negative control on the inputs of the cases, with the float32 restatement standing for a correct
    kernel: a reference with sign(0) = 1, and a Charbonnier reference with eps where eps eps belongs, fail the gates that the right
    references pass."""
    a64, b64 = _inputs((2, 3, 5, 7))
    a32, b32 = a64.astype(F32), b64.astype(F32)
    d = a64 - b64
    gs = float(F32(GSCALE)) / d.size
    # L1 with sign(0) = 1
    _, da_ref, s = ref64("l1", a64, b64)
    got = grad32("l1", a32, b32).astype(F64)
    gate(None, "l1 gradient", got, da_ref, s, K_GRAD["l1"])
    wrong = gs * np.where(d >= 0, 1.0, -1.0)
    assert (wrong != da_ref).sum() == (d == 0).sum() > 0
    with pytest.raises(AssertionError):
        gate(None, "l1 gradient, sign(0) = 1", got, wrong, np.abs(wrong), K_GRAD["l1"])
    # Charbonnier with sqrt(d d + eps)
    K = K_GRAD["charbonnier"] + CHARB_DEVICE_ULPS
    loss_ref, da_ref, s = ref64("charbonnier", a64, b64)
    got = grad32("charbonnier", a32, b32).astype(F64)
    d32 = a32 - b32
    loss32 = (np.sqrt(d32 * d32 + EPS32 * EPS32).sum(dtype=F32) * (F32(1) / F32(d.size))).reshape(1)
    gate(None, "charbonnier gradient", got, da_ref, s, K)
    sum_gate(None, "charbonnier mean", loss32, np.reshape(loss_ref, (1,)), d.size, loss_ref, floor=U * loss_ref)
    r = np.sqrt(d * d + float(EPS32))
    with pytest.raises(AssertionError):
        gate(None, "charbonnier gradient, eps for eps eps", got, gs * d / r, np.abs(gs * d / r), K)
    with pytest.raises(AssertionError):
        sum_gate(None, "charbonnier mean, eps for eps eps", loss32, np.reshape(r.sum() / d.size, (1,)), d.size, r.sum() / d.size,
                 floor=U * r.sum() / d.size)
