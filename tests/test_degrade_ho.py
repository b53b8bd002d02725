"""High-order degradation stages (csrc/degrade.hip): the per-sample 2-D filter, the kernel bank, the down-scale with a
tap table per sample and the shot / grey noise, against degrade_ho_contract.py.  Every device case runs on the emulator and, under
`-m gpu`, on the MI355X.

A. filter2d, BIT-EXACT: taps are non-zero signed multiples of 1/64 that sum to 1 (H.dyadic_kernels), inputs steps of 1/64 in [-1, 1]:
   every product is a multiple of 2^-12 and every partial sum, in any order and with or without FMA contraction, is bounded by
   sum |k| max |x| <= 2^6 -- 2^18 steps, inside float32's 2^24.  The premise is asserted on the float64 reference; the gate is tobytes().
B. filter2d with the bank's real kernels against float64 on the same float32 taps:
       |delta| <= 1.01 K^2 2^-24 sum |k| max |x|
   (float32 recursive summation of K^2 terms: gamma_n = n u / (1 - n u) with n = K^2 <= 441, u = 2^-24, and 1 / (1 - n u) < 1.01).
C. resize_select: bit-exact with dyadic tables; the three real tables against float64 F.interpolate with 1.01 kmax 2^-24 sum |w| max |x|
   per pass, summed over the two passes (the second pass's max |x| is that of the first pass's output).
D. noise kinds: test_degrade.py's gate, 2e-5 amp (2 / 255) + 1e-7, with amp = sqrt(g v) per element for shot noise.
Measured maxima go to the parity-error log through backend.report (degrade_ho.*)."""
import math
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import degrade_contract as C
import degrade_ho_contract as H
from backend import BACKENDS, L, ROOT, ops, report, select

import importlib

KB = importlib.import_module("fast-srgan_amd.kernel_bank")
DL = importlib.import_module("fast-srgan_amd.dataloader")

F32, F64 = np.float32, np.float64
TH, TW = L.FILTER2D_TILE_H, L.FILTER2D_TILE_W
_where = ["-"]


@pytest.fixture(params=BACKENDS)
def dev(request):
    _where[0] = request.param
    return select(request.param)


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _note(key, value):
    report("degrade_ho.%s.%s" % (_where[0], key), value)


def _filter2d_raw(dev, x, taps, radii):
    """fsr_filter2d through the C ABI with the caller's tables (ops.filter2d_words would refuse poisoned slots and radii out of range)."""
    xt = _t(x, dev)
    out = torch.full_like(xt, float("nan"))
    tt, rr = _t(np.asarray(taps, F32), dev), _t(np.asarray(radii, np.int32), dev)
    p = ops._p
    L.check(L.lib().fsr_filter2d(p(xt), p(out), x.shape[0], x.shape[2], x.shape[3], p(tt), p(rr), ops._stream()), "fsr_filter2d")
    assert L.lib().fsr_last_kernel() == b"filter2d_kernel"
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------- A. filter2d, exact
def test_exported_constants():
    assert (L.FILTER2D_MAX_RADIUS, L.FILTER2D_TAPS) == (H.MAX_RADIUS, H.TAPS) == (10, 441)
    assert ops.FILTER2D_WORDS == 442 and TH >= 1 and TW >= 1


def _exact_case(dev, h, w, radii, seed):
    n = len(radii)
    x = H.steps((n, 3, h, w), seed)
    x[0, 0, 0, 0] = -0.0
    taps, widest = H.dyadic_kernels(radii, seed)
    ref = H.np_filter2d(x, radii, taps)
    assert widest <= 64.0 and np.array_equal(ref * 4096.0, np.rint(ref * 4096.0)) and np.abs(ref).max() <= widest, "premise"
    assert np.array_equal(ref.astype(F32).astype(F64), ref)
    got = _filter2d_raw(dev, x, taps, radii)
    bad = got.view(np.uint32) != ref.astype(F32).view(np.uint32)
    assert got.tobytes() == ref.astype(F32).tobytes(), "filter2d %dx%d r=%s: %d of %d elements differ, first at %s" % (
        h, w, list(radii), bad.sum(), bad.size, tuple(int(v) for v in np.argwhere(bad)[0]))
    for i, r in enumerate(radii):
        if H.clamp_radius(r) == 0:
            assert got[i].tobytes() == x[i].tobytes()


# small shapes with radii 0, 1, 10 mixed in one batch; the tile extents -1, +0, +1 in each axis and two tiles + 1 (a grid of 3 x 3
# workgroups per plane whose last row and column own one pixel); radii -3 and 99 read as 0 and 10.  The launch does not cap its grid.
EXACT_CASES = [(1, 1, (0, 1, 10)), (1, 23, (10, 0, 1)), (23, 1, (1, 10, 0)), (3, 5, (0, 1, 10)),
               (TH - 1, TW - 1, (10, 3)), (TH, TW, (10, 1)), (TH + 1, TW + 1, (1, 10, 0)), (TH - 1, TW + 1, (7,)), (TH + 1, TW - 1, (4,)),
               (2 * TH + 1, 2 * TW + 1, (10, 0, 2)), (7, 11, (-3, 99, 5)), (12, 12, (1, 2, 3, 4, 5, 6, 7, 8, 9, 10))]


@pytest.mark.parametrize("h,w,radii", EXACT_CASES)
def test_filter2d_is_bit_exact(dev, h, w, radii):
    _exact_case(dev, h, w, radii, seed=300 + 7 * h + w)


def test_filter2d_radius_0_is_a_copy(dev):
    """-0.0, a NaN with a payload, infinities and a denormal survive the launch bit for bit; the neighbouring sample is filtered."""
    x = H.steps((2, 3, 9, TW + 3), 1)
    specials = np.array([0x80000000, 0x7fc12345, 0xffc00001, 0x7f800000, 0xff800000, 0x00000001], dtype=np.uint32).view(F32)
    x[0, 1, 4, :6] = specials
    x[0, 2, 8, TW + 2] = specials[1]
    taps, _ = H.dyadic_kernels((0, 2), 2)
    got = _filter2d_raw(dev, x, taps, (0, 2))
    assert got[0].tobytes() == x[0].tobytes()
    assert got[1].tobytes() == H.np_filter2d(x, (0, 2), taps)[1].astype(F32).tobytes()


def test_filter2d_vector_and_scalar_stores_agree(dev):
    """w % 4 == 0 takes 16-byte stores, an output view that is not 16-byte aligned must not."""
    x = H.steps((1, 3, 5, TW + 8), 3)
    taps, _ = H.dyadic_kernels((3,), 3)
    ref = H.np_filter2d(x, (3,), taps).astype(F32)
    assert _filter2d_raw(dev, x, taps, (3,)).tobytes() == ref.tobytes()
    xt, tt, rr = _t(x, dev), _t(taps, dev), _t(np.int32([3]), dev)
    buf = torch.zeros(x.size + 1, dtype=torch.float32, device=dev)
    L.check(L.lib().fsr_filter2d(ops._p(xt), buf.data_ptr() + 4, 1, 5, TW + 8, ops._p(tt), ops._p(rr), ops._stream()), "fsr_filter2d")
    assert buf[1:].cpu().numpy().tobytes() == ref.tobytes() and float(buf[0]) == 0.0


def test_filter2d_refusals():
    select("emu")
    lib = L.lib()
    err = lambda: lib.fsr_last_error().decode()
    x = torch.zeros(1, 3, 4, 4)
    p, q = x.data_ptr(), torch.zeros(1, 3, 4, 4).data_ptr()
    assert lib.fsr_filter2d(None, q, 1, 4, 4, p, p, None) == -1 and "null" in err()
    assert lib.fsr_filter2d(p, q, 1, 4, 4, None, p, None) == -1 and "null" in err()
    assert lib.fsr_filter2d(p, q, 1, 4, 4, p, None, None) == -1 and "null" in err()
    assert lib.fsr_filter2d(p, q, 0, 4, 4, p, p, None) == -2 and "positive" in err()
    assert lib.fsr_filter2d(p, q, 1, 4, 0, p, p, None) == -2 and "positive" in err()
    assert lib.fsr_filter2d(p, p, 1, 4, 4, p, p, None) == -2 and "input" in err()
    assert lib.fsr_filter2d(p, q, 1, 32768, 32768, p, p, None) == -2 and "31 bits" in err()
    with pytest.raises(ValueError, match="odd size"):
        ops.filter2d(x, [np.ones((2, 2))])
    with pytest.raises(ValueError, match="odd size"):
        ops.filter2d(x, [np.ones((23, 23))])
    with pytest.raises(ValueError, match="not finite"):
        ops.filter2d(x, [np.full((3, 3), np.nan)])
    with pytest.raises(ValueError, match="per-sample"):
        ops.filter2d(x, [None, None])
    with pytest.raises(ValueError, match="autograd"):
        ops.filter2d(x.clone().requires_grad_(), [None])


# ------------------------------------------------------------------------------------------- B. filter2d, the bank's kernels
def _bank_kernels(size):
    ks = [KB.bank_kernel(kind, size, 2.3, 0.9, 0.7, 1.7 if "generalized" in kind else 1.3) for kind in KB.KINDS]
    return ks + [KB.sinc_kernel(math.pi / 2.5, size)]


@pytest.mark.parametrize("size", [7, 21])
def test_filter2d_bank_kernels_against_float64(dev, size):
    ks = _bank_kernels(size)
    x = np.random.RandomState(size).uniform(-1.0, 1.0, size=(len(ks), 3, TH + 5, TW + 9)).astype(F32)
    got = ops.filter2d(_t(x, dev), ks).cpu().numpy()
    taps = np.zeros((len(ks), H.TAPS), F32)
    for i, k in enumerate(ks):
        taps[i, :k.size] = k.reshape(-1)
    ref = H.np_filter2d(x, [size // 2] * len(ks), taps)
    worst = worst_abs = 0.0
    for i, k in enumerate(ks):
        gate = 1.01 * size * size * 2.0 ** -24 * float(np.abs(k.astype(F64)).sum()) * float(np.abs(x[i]).max())
        err = float(np.abs(got[i] - ref[i]).max())
        print("filter2d K=%d %s: max |error| %.3e, gate %.3e" % (size, (KB.KINDS + ("sinc",))[i], err, gate))
        worst, worst_abs = max(worst, err / gate), max(worst_abs, err)
        assert err <= gate
    _note("filter2d_bank_K%d_error_over_gate" % size, worst)
    _note("filter2d_bank_K%d_max_error" % size, worst_abs)


def test_filter2d_sample_does_not_depend_on_its_batch(dev):
    ks = [KB.bank_kernel("aniso", 9, 2.0, 0.7, 0.4), None, KB.sinc_kernel(2.0, 13)]
    x = np.random.RandomState(8).uniform(-1.0, 1.0, size=(3, 3, 19, 30)).astype(F32)
    got = ops.filter2d(_t(x, dev), ks).cpu().numpy()
    for i in range(3):
        assert ops.filter2d(_t(x[i:i + 1], dev), ks[i:i + 1]).cpu().numpy().tobytes() == got[i].tobytes()


# ------------------------------------------------------------------------------------------------------- kernel bank (host)
BANK_CASES = [(kind, size) for kind in KB.KINDS for size in (1, 7, 21)]


@pytest.mark.parametrize("kind,size", BANK_CASES)
def test_bank_kernel_against_the_formulas(kind, size):
    sx, sy, th, beta = 2.1, 0.8, -1.1, 1.6
    k = KB.bank_kernel(kind, size, sx, sy, th, beta)
    assert k.dtype == np.float32 and k.shape == (size, size) and abs(float(k.astype(F64).sum()) - 1.0) <= 1e-6
    iso = kind.endswith("iso") and not kind.endswith("aniso")
    base = "generalized" if kind.startswith("generalized") else ("plateau" if kind.startswith("plateau") else "gauss")
    ref = H.bank_reference(base, size, sx, sx if iso else sy, 0.0 if iso else th, beta)
    k64 = KB.bank_kernel(kind, size, sx, sy, th, beta, dtype=F64)
    assert k64.dtype == np.float64 and np.abs(k64 - ref).max() <= 1e-12 and abs(k64.sum() - 1.0) <= 1e-12      # the formulas, before the cast
    assert np.array_equal(k, k64.astype(F32))                                                                # the cast, and nothing else


def test_bank_identities():
    j = np.arange(-10, 11, dtype=F64)
    one = np.exp(-j * j / (2.0 * 1.7 ** 2))
    one /= one.sum()
    raw = lambda kind, size, sx, sy=None, th=0.0, beta=1.0: KB.bank_kernel(kind, size, sx, sy, th, beta, dtype=F64)   # before the float32 cast
    assert np.abs(raw("iso", 21, 1.7) - np.outer(one, one)).max() <= 1e-12                                    # separable
    assert np.abs(raw("aniso", 21, 1.7, 1.7, 0.9) - raw("iso", 21, 1.7)).max() <= 1e-12
    assert np.abs(raw("aniso", 15, 2.5, 0.6, 0.3) - raw("aniso", 15, 2.5, 0.6, 0.3 + math.pi)).max() <= 1e-12
    assert np.abs(raw("generalized_aniso", 15, 2.5, 0.6, 0.3, 1.0) - raw("aniso", 15, 2.5, 0.6, 0.3)).max() <= 1e-12
    assert np.array_equal(KB.bank_kernel("aniso", 15, 2.5, 0.6, 0.3), raw("aniso", 15, 2.5, 0.6, 0.3).astype(F32))
    k = raw("aniso", 15, 3.0, 0.5, 0.0)                       # theta = 0: sigma_x along a row
    assert k[7, 10] > 10 * k[10, 7]
    k = raw("aniso", 15, 3.0, 0.5, math.pi / 4)                # rotated by +45 degrees: along the diagonal x = y
    assert k[10, 10] > 10 * k[4, 10]
    with pytest.raises(ValueError):
        KB.bank_kernel("iso", 8, 1.0)
    with pytest.raises(ValueError):
        KB.bank_kernel("iso", 23, 1.0)
    with pytest.raises(ValueError):
        KB.bank_kernel("box", 7, 1.0)


def test_j1_against_scipy():
    special = pytest.importorskip("scipy.special")
    x = np.concatenate([np.linspace(0.0, 10.0 * math.pi, 4001), np.linspace(10.0 * math.pi, 50.0, 501)])
    err = float(np.abs(KB.j1(x) - special.j1(x)).max())
    print("J1: max |error| against scipy %.3e" % err)
    assert err <= 1e-12


def test_j1_against_its_series():
    for x in (0.0, 0.5, 1.0, 3.8317059702075125, 10.0, 31.4):
        assert abs(float(KB.j1(x)) - H.j1_series(x)) <= 1e-12


def test_sinc_kernel():
    for omega, size in ((math.pi, 7), (math.pi / 3, 21), (1.3, 13)):
        k, k64 = KB.sinc_kernel(omega, size), KB.sinc_kernel(omega, size, dtype=F64)
        assert k.dtype == np.float32 and abs(float(k.astype(F64).sum()) - 1.0) <= 1e-6 and np.array_equal(k, k64.astype(F32))
        c, seen = size // 2, {}
        raw = np.zeros((size, size))
        for i in range(size):
            for j in range(size):
                rad = math.sqrt((i - c) ** 2 + (j - c) ** 2)
                if rad not in seen:
                    seen[rad] = omega * omega / (4 * math.pi) if rad == 0 else omega * H.j1_series(omega * rad) / (2 * math.pi * rad)
                raw[i, j] = seen[rad]
        raw /= raw.sum()
        assert np.abs(k64 - raw).max() <= 1e-12 and abs(k64.sum() - 1.0) <= 1e-12
        assert (k < 0).any()                                   # it rings
    with pytest.raises(ValueError):
        KB.sinc_kernel(4.0, 7)


# the first six draws of KernelBank(kernel_size=(7, 21), sinc_prob=0.3) from random.Random(2024): (kind, size, omega) or
# (kind, size, sigma_x, sigma_y, theta, beta), rounded to 12 places
PINNED_DRAWS = [("sinc", 13, 2.670558905544), ("iso", 13, 2.237725577681, 2.897099013707, -1.196763258502, 1.0),
                ("generalized_iso", 9, 1.511893008568, 2.185297667445, 2.336758916745, 1.019299908434), ("sinc", 11, 1.941099769832),
                ("iso", 11, 2.629841544774, 0.841488526557, -2.88720502126, 1.0), ("sinc", 11, 3.131301348137)]


def test_bank_draws_are_pinned():
    bank = KB.KernelBank(kernel_size=(7, 21), sinc_prob=0.3)
    rng = random.Random(2024)
    draws = [bank.draw(rng) for _ in range(6)]
    rng2 = random.Random(2024)                                 # the same variates are consumed whatever comes out
    other = KB.KernelBank(kernel_size=(7, 21), kernel_kinds=(0, 0, 0, 1, 0, 0), sinc_prob=0.9)
    assert [other.draw(rng2)["size"] for _ in range(6)] == [d["size"] for d in draws] and rng2.getstate() == rng.getstate()
    got = [(d["kind"], d["size"]) + tuple(round(d[k], 12) for k in ("omega", "sigma_x", "sigma_y", "theta", "beta") if k in d) for d in draws]
    print(got)
    assert got == PINNED_DRAWS
    for d in draws:
        k = KB.build(d)
        assert k.shape == (d["size"], d["size"]) and abs(float(k.astype(F64).sum()) - 1.0) <= 1e-6
        if d["kind"] == "sinc":
            assert (math.pi / 3 if d["size"] < 13 else math.pi / 5) <= d["omega"] <= math.pi
    assert KB.build(None) is None
    rng3 = random.Random(2024)                                 # nine variates a draw, whatever the bank holds
    for _ in range(54):
        rng3.random()
    assert rng3.getstate() == rng.getstate()
    sizes = {bank.draw(rng)["size"] for _ in range(400)}
    assert sizes == {7, 9, 11, 13, 15, 17, 19, 21}
    only = KB.KernelBank(kernel_size=(5, 5), kernel_kinds=(0, 0, 0, 0, 1, 0))
    assert {only.draw(rng)["kind"] for _ in range(50)} == {"plateau_iso"}
    with pytest.raises(ValueError):
        KB.KernelBank(kernel_size=(8, 8))
    with pytest.raises(ValueError):
        KB.KernelBank(kernel_kinds=(1, 1))
    with pytest.raises(ValueError):
        KB.KernelBank(sinc_prob=1.5)


# ----------------------------------------------------------------------------------------------------- C. resize_select
def _tables(in_size, out_size, kmaxes, seed):
    return [H.dyadic_table(in_size, out_size, k, seed + 31 * f) for f, k in enumerate(kmaxes)]


@pytest.mark.parametrize("H_,W_,h,w,sel", [(1, 1, 1, 1, (0, 2, 1)), (16, 20, 4, 5, (2, 0, 1, 1)), (23, 300, 7, 70, (1, 2)), (9, 5, 12, 9, (0, 1, 2))])
def test_resize_select_is_bit_exact(dev, H_, W_, h, w, sel):
    """Dyadic tables of different widths per filter (sixteenths; the slots behind xsize hold 1e30), the table index mixed within the
    batch; pass 1 is a multiple of 2^-10, pass 2 of 2^-14, both bounded by (sum |w|)^2 <= 16."""
    tx, ty = _tables(W_, w, (9, 4, 6), 40 + W_), _tables(H_, h, (3, 8, 5), 50 + H_)
    x = H.steps((len(sel), 3, H_, W_), 60 + h)
    x[0, 0, 0, 0] = -0.0
    ref, mid = H.np_resize_select(x, tx, ty, sel, passes=True)
    assert np.array_equal(mid * 2.0 ** 10, np.rint(mid * 2.0 ** 10)) and np.array_equal(ref * 2.0 ** 14, np.rint(ref * 2.0 ** 14))
    assert np.abs(ref).max() <= 16.0 and np.array_equal(ref.astype(F32).astype(F64), ref)
    tabs = ops.ResizeTables([t + (t[2].shape[1],) for t in tx], [t + (t[2].shape[1],) for t in ty], H_, W_, dev)
    assert (tabs.nf, tabs.kx, tabs.ky, tabs.out_h, tabs.out_w) == (3, 9, 8, h, w)                 # rows padded to the widest table
    got = ops.resize_select(_t(x, dev), tabs, sel).cpu().numpy()
    assert L.lib().fsr_last_kernel() == b"resize_select_hpass_kernel+resize_select_vpass_kernel"
    assert got.tobytes() == ref.astype(F32).tobytes()
    for bad in ((3,) + tuple(sel[1:]), (-1,) + tuple(sel[1:])):
        with pytest.raises(ValueError, match="table indices"):
            ops.resize_select(_t(x, dev), tabs, bad)


@pytest.mark.parametrize("big,small", [(16, 4), (24, 6), (20, 5)])
def test_resize_select_real_tables_against_interpolate(dev, big, small):
    tables = [DL.resize_taps(big, small, kind) for kind in DL.RESIZE_FILTERS]
    tabs = ops.ResizeTables(tables, tables, big, big, dev)
    x = np.random.RandomState(big).uniform(-1.0, 1.0, size=(3, 3, big, big)).astype(F32)
    got = ops.resize_select(_t(x, dev), tabs, [0, 1, 2]).cpu().numpy()
    xd = torch.from_numpy(x).double()
    refs = [F.interpolate(xd[0:1], size=(small, small), mode="bicubic", antialias=True, align_corners=False),
            F.interpolate(xd[1:2], size=(small, small), mode="bilinear", antialias=True, align_corners=False),
            F.interpolate(xd[2:3], size=(small, small), mode="area")]
    worst = worst_abs = 0.0
    for i, (kind, (xmin, xsize, wt, kmax)) in enumerate(zip(DL.RESIZE_FILTERS, tables)):
        sw = float(np.abs(wt.astype(F64)).sum(axis=1).max())
        mid = H.np_resize_select(x[i:i + 1], [tables[i][:3]], [tables[i][:3]], [0], passes=True)[1]
        gate = 1.01 * kmax * 2.0 ** -24 * sw * (float(np.abs(x[i]).max()) + float(np.abs(mid).max()))
        err = float(np.abs(got[i] - refs[i][0].numpy()).max())
        print("resize_select %d->%d %s: max |error| %.3e, gate %.3e" % (big, small, kind, err, gate))
        worst = max(worst, err / gate)
        worst_abs = max(worst_abs, err)
        assert err <= gate
    _note("resize_select_%d_error_over_gate" % big, worst)
    _note("resize_select_%d_max_error" % big, worst_abs)


def test_resize_tables_are_checked():
    xmin, xsize, w, kmax = DL.resize_taps(16, 4, "bilinear")
    good = (xmin, xsize, w, kmax)
    ops.ResizeTables([good], [good], 16, 16, "cpu")
    for bad in ((xmin + 9, xsize, w, kmax), (xmin, xsize + kmax, w, kmax), (xmin - 1, xsize, w, kmax), (xmin, xsize * 0, w, kmax)):
        with pytest.raises(ValueError, match="reads outside"):
            ops.ResizeTables([bad], [good], 16, 16, "cpu")
    with pytest.raises(ValueError, match="one table per filter"):
        ops.ResizeTables([good], [good, good], 16, 16, "cpu")
    with pytest.raises(ValueError):
        DL.resize_taps(16, 4, "lanczos")
    select("emu")
    lib, p = L.lib(), torch.zeros(64).data_ptr()
    args = (1, 4, 4, 2, 2, p, p, p, 3, p, p, p, 3, 1, p, None)
    assert lib.fsr_resize_select(None, p + 4, p + 8, *args) == -1
    assert lib.fsr_resize_select(p, p, p + 8, *args) == -2 and lib.fsr_resize_select(p, p + 4, p, *args) == -2
    assert lib.fsr_resize_select(p, p + 4, p + 8, 1, 4, 4, 0, 2, p, p, p, 3, p, p, p, 3, 1, p, None) == -2
    assert lib.fsr_resize_select(p, p + 4, p + 8, 1, 4, 4, 2, 2, p, p, p, 3, p, p, p, 3, 0, p, None) == -2


# ------------------------------------------------------------------------------------------------------- D. noise kinds
def _rand(shape, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, size=shape).astype(F32)


def _noise_gate(what, got, x, strength, flags, seeds):
    """test_degrade.py's noise gate, 2e-5 sigma (2 / 255) + 1e-7, with sigma per element: sqrt(g v) for a shot sample."""
    want, amp = H.np_noise_kinds(x, strength, flags, seeds)
    worst = 0.0
    for i, g in enumerate(strength):
        if g == 0:
            assert got[i].tobytes() == x[i].tobytes(), "%s: sample %d (strength 0) is not a copy" % (what, i)
            continue
        gate = 2e-5 * amp[i] * (2.0 / 255.0) + 1e-7
        ratio = np.abs(got[i].astype(F64) - want[i]) / gate
        print("%s: sample %d flags %d strength %g: largest error / gate %.3f" % (what, i, flags[i], g, ratio.max()))
        worst = max(worst, float(ratio.max()))
        _note("%s_max_error" % what.replace(" ", "_"), float(np.abs(got[i].astype(F64) - want[i]).max()))
        assert ratio.max() < 1.0
    return worst


def test_shot_noise_against_contract(dev):
    x = _rand((4, 3, 19, 30), 3)
    x[0, 0, 0, :4] = [-1.0, 1.0, -1.5, 1.25]                   # v = 0 (no noise at black), 255, and both clamps
    g, flags, seeds = [1.5, 0.0, 0.05, 3.0], [H.SHOT] * 4, [(0, 0), (5, 6), (0xffffffff, 0xfffffffe), (7, 8)]
    got = ops.degrade_noise_kinds(_t(x, dev), g, flags, seeds).cpu().numpy()
    assert L.lib().fsr_last_kernel() == b"noise_kinds_kernel"
    _note("shot_error_over_gate", _noise_gate("shot", got, x, g, flags, seeds))
    assert got[0, 0, 0, 0] == -1.0 and got[0, 0, 0, 2] == -1.5
    field = (got[0].astype(F64) - x[0]) / (2.0 / 255.0) / np.sqrt(1.5 * np.clip((x[0].astype(F64) + 1) * 127.5, 1e-9, 255))
    assert 0.9 < field[1:].std() < 1.1 and abs(field[1:].mean()) < 0.15


def test_noise_kinds_mixed_in_one_batch(dev):
    x = _rand((5, 3, 9, 13), 4)
    st, flags = [5.0, 1.0, 5.0, 0.7, 0.0], [0, H.SHOT, H.GREY, H.SHOT | H.GREY, H.GREY]
    seeds = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10)]
    got = ops.degrade_noise_kinds(_t(x, dev), st, flags, seeds).cpu().numpy()
    _note("kinds_error_over_gate", _noise_gate("kinds", got, x, st, flags, seeds))
    plain = ops.degrade_blur_noise(_t(x[:1], dev), None, st[:1], seeds[:1]).cpu().numpy()
    assert plain.tobytes() == got[:1].tobytes()              # no flag: fsr_degrade_blur_noise's noise, bit for bit


def test_grey_noise_shares_z_among_the_channels(dev):
    x = np.zeros((2, 3, 19, 30), F32)
    got = ops.degrade_noise_kinds(_t(x, dev), [5.0, 5.0], [H.GREY, 0], [(1, 2), (1, 2)]).cpu().numpy()
    assert got[0, 0].tobytes() == got[0, 1].tobytes() == got[0, 2].tobytes() and np.abs(got[0, 0]).max() > 0
    assert not np.array_equal(got[1, 0], got[1, 1]) and not np.array_equal(got[1, 1], got[1, 2])
    assert got[0, 0].tobytes() == got[1, 0].tobytes()        # plane 0 has the element indices y w + x in both forms


def test_noise_kinds_follow_the_seed_not_the_batch_position(dev):
    x = _rand((4, 3, 9, 13), 5)
    x[3] = x[0]
    for f in (H.SHOT, H.GREY, H.SHOT | H.GREY):
        a = ops.degrade_noise_kinds(_t(x, dev), [1.0] * 4, [f] * 4, [(1, 2), (1, 3), (2, 2), (1, 2)]).cpu().numpy()
        assert a[0].tobytes() == a[3].tobytes()
        d = a - x
        assert not np.array_equal(d[0], d[1]) and not np.array_equal(d[0], d[2])
        b = ops.degrade_noise_kinds(_t(x[3:], dev), [1.0], [f], [(1, 2)]).cpu().numpy()
        assert b[0].tobytes() == a[0].tobytes()


def test_noise_kinds_refusals():
    x = torch.zeros(2, 3, 4, 4)
    select("emu")
    with pytest.raises(ValueError, match="shot gain"):
        ops.degrade_noise_kinds(x, [1.0, 3.5], [H.SHOT, H.SHOT], [(0, 0), (0, 0)])
    with pytest.raises(ValueError, match="sigma"):
        ops.degrade_noise_kinds(x, [1.0, 26.0], [0, H.GREY], [(0, 0), (0, 0)])
    with pytest.raises(ValueError, match="flags"):
        ops.degrade_noise_kinds(x, [1.0, 1.0], [0, 4], [(0, 0), (0, 0)])
    with pytest.raises(ValueError, match="32-bit"):
        ops.degrade_noise_kinds(x, [1.0, 1.0], [0, 0], [(0, 0), (0, 1 << 32)])
    lib, p = L.lib(), x.data_ptr()
    assert lib.fsr_degrade_noise_kinds(p, p, 2, 4, 4, p, None, p, None) == -1
    assert lib.fsr_degrade_noise_kinds(p, p, 2, 0, 4, p, p, p, None) == -2


# ------------------------------------------------------------------------------------------------- E. loader, configuration
pkg = importlib.import_module("fast-srgan_amd")
train = importlib.import_module("fast-srgan_amd.train")

ON = dict(blur_sigma=(0.2, 2.0), blur_prob=0.5, noise_sigma=(1, 10), noise_prob=0.8, jpeg_quality=(30, 95), jpeg_prob=0.7)
SECOND = dict(kernel_prob=0.6, kernel_size=(3, 7), sinc_prob=0.3, noise_prob=0.6, noise_shot_prob=0.5, noise_grey_prob=0.5, jpeg_prob=0.6,
              jpeg_quality=(40, 90))
HO = dict(kernel_prob=0.7, kernel_size=(3, 9), sinc_prob=0.2, resize_filters=(1, 1, 1), noise_shot_prob=0.5, noise_grey_prob=0.4,
          second=SECOND, final_sinc_prob=0.8, final_sinc_size=(3, 7))


def _dataset(tmp_path, dev, count=3):
    paths = []
    for i in range(count):
        p = str(tmp_path / ("img%d.npy" % i))
        np.save(p, C.synthetic_image(40 + 3 * i, 44, seed=i))
        paths.append(p)
    return pkg.NumpyImagesDataset(paths, lr_image_size=8, scale_factor=4, device=dev)


class _Recorder:
    """Stands in for the loaded library: every fsr_* call goes through, and (entry point, the kernel names it noted) is appended to
    `seen` -- the names only for the degradation entry points, which all note theirs (fsr_crop_resize leaves the last name as it was)."""
    NOTING = ("fsr_degrade_blur_noise", "fsr_jpeg_roundtrip", "fsr_filter2d", "fsr_resize_select", "fsr_degrade_noise_kinds")

    def __init__(self, lib):
        self._lib, self.seen = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in ("fsr_last_kernel", "fsr_last_error", "fsr_version"):
            return fn

        def call(*args):
            rc = fn(*args)
            self.seen.append((name, self._lib.fsr_last_kernel() if name in self.NOTING else None))
            return rc
        return call


def _run(loader):
    """[(lr, hr)] of a pass and the launch sequence of its batches."""
    rec = _Recorder(L.lib())
    saved = L._lib
    L._lib = rec
    try:
        out = [(lr.clone(), hr.clone()) for lr, hr in loader]
    finally:
        L._lib = saved
    return out, rec.seen


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))


def test_loader_off_is_the_parent_path(dev, tmp_path):
    ds = _dataset(tmp_path, dev)
    off = dict(second=dict(kernel_size=(3, 7), noise_sigma=(2, 3)), kernel_size=(3, 9), resize_filters=(2, 0, 0), noise_shot_gain=(0.1, 0.2))
    for first in ({}, ON):                                     # nothing at all, and the first-order model alone
        plain = pkg.DeviceBatchLoader(ds, 2, 3, seed=5, degradation=DL.Degradation(seed=1, **first) if first else None)
        quiet = pkg.DeviceBatchLoader(ds, 2, 3, seed=5, degradation=DL.Degradation(seed=1, **dict(first, **off)))
        assert (plain.degradation is None) == (quiet.degradation is None)
        assert sorted(plain.state_dict()) == sorted(quiet.state_dict())
        (a, seq_a), (b, seq_b) = _run(plain), _run(quiet)
        assert _same(a, b) and seq_a == seq_b and len(seq_a) >= 3


def test_unknown_keywords():
    """An unknown keyword of Degradation is the TypeError it always was; an unknown key of `second` names the second round's keys."""
    with pytest.raises(TypeError, match="kernel_probability"):
        DL.Degradation(seed=1, kernel_probability=0.5)
    with pytest.raises(ValueError, match="blur_prob.*of `second`.*noise_shot_gain"):
        DL.Degradation(seed=1, second=dict(blur_prob=0.5))


def test_final_sinc_size_is_its_own_key():
    d = DL.Degradation(seed=4, final_sinc_prob=1.0, final_sinc_size=(3, 5), second=dict(kernel_size=(9, 21)))
    ho = d.draw(40).ho
    assert {(a or b)["size"] for a, b in zip(ho.sinc_a, ho.sinc_b)} == {3, 5}
    assert DL.Degradation(seed=4).final_sinc_size == (7, 21)


def test_noise_kind_without_noise_is_off():
    d = DL.Degradation(seed=1, noise_shot_prob=0.5, noise_grey_prob=1.0)
    assert not d.high_order and not d.enabled
    d = DL.Degradation(seed=1, noise_prob=0.5, noise_shot_prob=0.5)
    assert d.high_order and d.noise_kinds and not d.lr_from_hr


def _by_hand(ds, p, hr):
    ho = p.ho
    pick = lambda pairs, i: [v[i] for v in pairs]
    lr = ops.resize_select(ops.filter2d(hr, [KB.build(k) for k in ho.kernel1]), ds.resize_tables(), ho.resize)
    lr = ops.degrade_blur_noise(lr, p.blur_sigma, None, None)
    lr = ops.degrade_noise_kinds(lr, pick(ho.noise1, 0), pick(ho.noise1, 1), p.seeds)
    lr = ops.jpeg_roundtrip(lr, p.quality, "420")
    lr = ops.filter2d(lr, [KB.build(k) for k in ho.kernel2])
    lr = ops.degrade_noise_kinds(lr, pick(ho.noise2, 0), pick(ho.noise2, 1), ho.seeds2)
    lr = ops.filter2d(lr, [KB.build(k) for k in ho.sinc_a])
    lr = ops.jpeg_roundtrip(lr, ho.quality2, "420")
    return ops.filter2d(lr, [KB.build(k) for k in ho.sinc_b])


def test_loader_on(dev, tmp_path):
    ds = _dataset(tmp_path, dev)
    make = lambda seed, **kw: pkg.DeviceBatchLoader(ds, 2, 4, seed=5, degradation=DL.Degradation(seed=seed, **dict(ON, **kw)))
    first, _ = _run(make(1))
    on, seq = _run(make(1, **HO))
    again, seq_again = _run(make(1, **HO))
    other, seq_other = _run(make(2, **HO))
    assert all(torch.equal(a[1], b[1]) for a, b in zip(first, on))                 # hr: the clean crop, the crop and index sequence
    assert _same(on, again) and seq == seq_again
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(on, other)) and any(not torch.equal(a[0], b[0]) for a, b in zip(on, first))
    assert seq == seq_other and len(set(seq)) >= 6                                 # other draws, the same launches
    per_batch = len(seq) // 4
    assert all(seq[i * per_batch:(i + 1) * per_batch] == seq[:per_batch] for i in range(4))
    # the first-order stream does not move; apply = the operators called by hand with draw's parameters
    deg, plain = DL.Degradation(seed=1, **dict(ON, **HO)), DL.Degradation(seed=1, **ON)
    fired = {"kernel1": 0, "kernel2": 0, "sinc": 0, "shot": 0, "grey": 0, "filters": set()}
    for lr_on, hr in on:
        p = deg.draw(2)
        assert tuple(p) == tuple(plain.draw(2)) and isinstance(p, DL.DegradeParams)
        assert torch.equal(_by_hand(ds, p, hr), lr_on)
        fired["kernel1"] += sum(k is not None for k in p.ho.kernel1)
        fired["kernel2"] += sum(k is not None for k in p.ho.kernel2)
        fired["sinc"] += sum(k is not None for k in p.ho.sinc_a + p.ho.sinc_b)
        fired["shot"] += sum(bool(f & H.SHOT) for _, f in p.ho.noise1 + p.ho.noise2)
        fired["grey"] += sum(bool(f & H.GREY) for _, f in p.ho.noise1 + p.ho.noise2)
        fired["filters"] |= set(p.ho.resize)
        assert all(a is None or b is None for a, b in zip(p.ho.sinc_a, p.ho.sinc_b))
    print(fired)
    assert all(fired[k] > 0 for k in ("kernel1", "kernel2", "sinc", "shot", "grey")) and len(fired["filters"]) >= 2


def test_switching_a_stage_on_moves_no_earlier_draw():
    base = DL.Degradation(seed=3, **dict(ON, kernel_prob=0.5)).draw(6)
    more = DL.Degradation(seed=3, **dict(ON, **dict(HO, kernel_prob=0.5, kernel_size=(7, 21), sinc_prob=0.0))).draw(6)
    assert tuple(base) == tuple(more) and base.ho.kernel1 == more.ho.kernel1 and base.ho.seeds2 == more.ho.seeds2
    assert base.ho.quality2 == [0] * 6 and base.ho.sinc_a == [None] * 6 and any(more.ho.quality2)


def test_state_dict_round_trip_mid_pass(dev, tmp_path):
    ds = _dataset(tmp_path, dev)
    make = lambda **kw: pkg.DeviceBatchLoader(ds, 2, 5, seed=5, degradation=DL.Degradation(seed=1, **dict(ON, **kw)))
    whole = [(lr.clone(), hr.clone()) for lr, hr in make(**HO)]
    a = make(**HO)
    it = iter(a)
    head = [tuple(t.clone() for t in next(it)) for _ in range(2)]
    sd = a.state_dict()
    assert "degradation_high_order" in sd and "degradation_high_order" not in make().state_dict()
    b = make(**HO)
    b.load_state_dict(sd)
    tail = [(lr.clone(), hr.clone()) for lr, hr in b]
    assert _same(whole, head + tail)
    with pytest.raises(ValueError, match="high-order"):
        make().load_state_dict(sd)
    with pytest.raises(ValueError, match="high-order"):
        make(**HO).load_state_dict(make().state_dict())
    plain = make()
    plain.load_state_dict(make().state_dict())               # a state without the new stream loads as ever


def test_config_overrides_reach_the_loaders(tmp_path):
    dev = select("emu")
    ds = _dataset(tmp_path, dev)
    ov = ["training.batch_size=2", "training.iterations=2", "training.pretrain_iterations=1", "experiment.seed=11"]
    assert all(l.degradation is None for l in train.build_loaders(pkg.load_config(None, ov + ["data.degradation.kernel_prob=0"]), ds))
    cfg = pkg.load_config(None, ov + [
        "data.degradation.kernel_prob=0.5", "data.degradation.kernel_size=[3,9]", "data.degradation.kernel_kinds=[1,1,1,0,1,0]",
        "data.degradation.kernel_sigma=[0.3,2.5]", "data.degradation.kernel_beta_generalized=[0.6,3]", "data.degradation.kernel_beta_plateau=[1,2]",
        "data.degradation.sinc_prob=0.1", "data.degradation.resize_filters=[2,1,1]", "data.degradation.noise_prob=0.5",
        "data.degradation.noise_shot_prob=0.4", "data.degradation.noise_shot_gain=[0.1,1.0]", "data.degradation.noise_grey_prob=0.4",
        "data.degradation.second.kernel_prob=0.3", "data.degradation.second.kernel_size=[3,5]", "data.degradation.second.jpeg_prob=0.5",
        "data.degradation.second.jpeg_quality=[50,80]", "data.degradation.second.noise_prob=0.2", "data.degradation.final_sinc_prob=0.5",
        "data.degradation.final_sinc_size=[3,5]"])
    loaders = train.build_loaders(cfg, ds, rank=0)
    for l in loaders:
        d = l.degradation
        assert d.high_order and d.hr_blur and d.lr_from_hr and d.noise_kinds and d.final_sinc
        assert (d.first.kernel_prob, d.first.bank.kernel_size, d.first.bank.kernel_kinds) == (0.5, (3, 9), (1.0, 1.0, 1.0, 0.0, 1.0, 0.0))
        assert (d.first.bank.kernel_sigma, d.first.bank.kernel_beta_generalized, d.first.bank.sinc_prob) == ((0.3, 2.5), (0.6, 3.0), 0.1)
        assert (d.resize_filters, d.first.noise_shot_prob, d.first.noise_shot_gain, d.first.noise_grey_prob) == ((2.0, 1.0, 1.0), 0.4, (0.1, 1.0), 0.4)
        assert (d.second.kernel_prob, d.second.bank.kernel_size, d.second.jpeg_prob, d.second.jpeg_quality) == (0.3, (3, 5), 0.5, (50, 80))
        assert (d.second.noise_prob, d.final_sinc_prob, d.final_sinc_size, d.final_sinc_sizes) == (0.2, 0.5, (3, 5), [3, 5])
    lr, hr = next(iter(loaders[2]))
    assert lr.shape == (2, 3, 8, 8) and hr.shape == (2, 3, 32, 32) and torch.isfinite(lr).all()
    with pytest.raises(ValueError, match="unknown data.degradation.*kernel_prob.*final_sinc_prob"):
        train.build_loaders(pkg.load_config(None, ov + ["data.degradation.kernel_probability=1"]), ds)
    with pytest.raises(ValueError, match="unknown data.degradation.second.*noise_shot_gain"):
        train.build_loaders(pkg.load_config(None, ov + ["data.degradation.second.blur_prob=1"]), ds)
    with pytest.raises(ValueError, match="group"):
        train.build_loaders(pkg.load_config(None, ov + ["data.degradation.second=1"]), ds)
    for bad in ("data.degradation.resize_filters=[1,0]", "data.degradation.kernel_size=[8,8]", "data.degradation.noise_shot_gain=[0.5,4]",
                "data.degradation.final_sinc_prob=1.5", "data.degradation.second.kernel_kinds=[1,1]", "data.degradation.final_sinc_size=[8,8]"):
        with pytest.raises(ValueError):
            train.build_loaders(pkg.load_config(None, ov + [bad]), ds)


# ---------------------------------------------------------------------------------------------- F. full size (-m gpu only)
def _one(p, i):
    """The parameters of sample i as a batch of one."""
    q = DL.DegradeParamsHO(*[v[i:i + 1] for v in p])
    q.ho = DL.HighOrderParams(*[v[i:i + 1] for v in p.ho])
    return q


@pytest.mark.gpu
def test_full_size():
    """Batch 32, 96 -> 384, every stage on at K = 21: samples 0 and n - 1 are bit-equal to themselves run at batch 1, and the stages
    of those runs that have a float64 contract with a derived gate (both 2-D filters at K = 21, the down-scale, both noises) meet it."""
    dev = select("hip")
    _where[0] = "hip"
    n, l, s = 32, 96, 4
    hr = np.stack([(C.synthetic_image(l * s, l * s, seed=i % 3) / 127.5 - 1.0).astype(F32) for i in range(n)])
    second = dict(SECOND, kernel_prob=1.0, kernel_size=(21, 21), noise_prob=1.0, jpeg_prob=1.0)
    deg = DL.Degradation(seed=9, **dict(ON, blur_prob=1.0, noise_prob=1.0, jpeg_prob=1.0, **dict(HO, kernel_prob=1.0, kernel_size=(21, 21),
                                                                                              second=second, final_sinc_prob=1.0)))
    p = deg.draw(n)
    assert all(k["size"] == 21 for k in p.ho.kernel1 + p.ho.kernel2) and {f for _, f in p.ho.noise1 + p.ho.noise2} == {0, 1, 2, 3}
    taps = [DL.resize_taps(l * s, l, kind) for kind in DL.RESIZE_FILTERS]
    tables = ops.ResizeTables(taps, taps, l * s, l * s, dev)
    hr_t = _t(hr, dev)
    dummy = torch.empty((n, 3, l, l), dtype=torch.float32, device=dev)
    out = deg.apply_high_order(dummy, hr_t, p, tables)
    assert out.shape == (n, 3, l, l) and bool(torch.isfinite(out).all())
    for i in (0, n - 1):
        q = _one(p, i)
        alone = deg.apply_high_order(dummy[:1], hr_t[i:i + 1].contiguous(), q, tables)
        assert torch.equal(alone[0], out[i]), "sample %d depends on its batch" % i
        # the stages by hand, each against its contract on the input the device gave it
        k1 = KB.build(q.ho.kernel1[0])
        a = ops.filter2d(hr_t[i:i + 1].contiguous(), [k1])
        t1 = np.zeros((1, H.TAPS), F32)
        t1[0] = k1.reshape(-1)
        err = float(np.abs(a.cpu().numpy() - H.np_filter2d(hr[i:i + 1], [10], t1)).max())
        gate = 1.01 * 441 * 2.0 ** -24 * float(np.abs(k1.astype(F64)).sum()) * float(np.abs(hr[i]).max())
        print("sample %d: filter2d at 384^2, K = 21 (%s): max |error| %.3e, gate %.3e" % (i, q.ho.kernel1[0]["kind"], err, gate))
        _note("full_size_filter2d_error_over_gate", err / gate)
        _note("full_size_filter2d_max_error", err)
        assert err <= gate
        f = q.ho.resize[0]
        b = ops.resize_select(a, tables, [f])
        a_np = a.cpu().numpy()
        ref, mid = H.np_resize_select(a_np, [taps[f][:3]], [taps[f][:3]], [0], passes=True)
        sw = float(np.abs(taps[f][2].astype(F64)).sum(axis=1).max())
        gate = 1.01 * taps[f][3] * 2.0 ** -24 * sw * (float(np.abs(a_np).max()) + float(np.abs(mid).max()))
        err = float(np.abs(b.cpu().numpy() - ref).max())
        print("sample %d: resize_select %s: max |error| %.3e, gate %.3e" % (i, DL.RESIZE_FILTERS[f], err, gate))
        assert err <= gate
        c = ops.degrade_blur_noise(b, q.blur_sigma, None, None)
        d = ops.degrade_noise_kinds(c, [q.ho.noise1[0][0]], [q.ho.noise1[0][1]], q.seeds)
        _noise_gate("sample %d noise 1" % i, d.cpu().numpy(), c.cpu().numpy(), [q.ho.noise1[0][0]], [q.ho.noise1[0][1]], q.seeds)
        e = ops.jpeg_roundtrip(d, q.quality, "420")
        k2 = KB.build(q.ho.kernel2[0])
        g = ops.filter2d(e, [k2])
        t2 = np.zeros((1, H.TAPS), F32)
        t2[0] = k2.reshape(-1)
        err = float(np.abs(g.cpu().numpy() - H.np_filter2d(e.cpu().numpy(), [10], t2)).max())
        gate = 1.01 * 441 * 2.0 ** -24 * float(np.abs(k2.astype(F64)).sum()) * float(np.abs(e.cpu().numpy()).max())
        print("sample %d: filter2d at 96^2, K = 21 (%s): max |error| %.3e, gate %.3e" % (i, q.ho.kernel2[0]["kind"], err, gate))
        assert err <= gate
        m = ops.degrade_noise_kinds(g, [q.ho.noise2[0][0]], [q.ho.noise2[0][1]], q.ho.seeds2)
        _noise_gate("sample %d noise 2" % i, m.cpu().numpy(), g.cpu().numpy(), [q.ho.noise2[0][0]], [q.ho.noise2[0][1]], q.ho.seeds2)
        m = ops.filter2d(m, [KB.build(q.ho.sinc_a[0])])
        m = ops.jpeg_roundtrip(m, q.ho.quality2, "420")
        m = ops.filter2d(m, [KB.build(q.ho.sinc_b[0])])
        assert torch.equal(m[0], out[i])


# ------------------------------------------------------------------------------------------------------------------ tool
def test_cli_tool_round_trips_a_png_with_the_new_flags(tmp_path):
    import importlib.util
    import os

    from PIL import Image
    select("emu")
    spec = importlib.util.spec_from_file_location("degrade_tool", os.path.join(ROOT, "tools", "degrade.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src = C.synthetic_image(20, 28)
    Image.fromarray(src.transpose(1, 2, 0)).save(str(tmp_path / "in.png"))
    io_ = ["--image", str(tmp_path / "in.png"), "--output", str(tmp_path / "out.png")]
    x = _t((src.astype(F32) / F32(127.5) - F32(1))[None], torch.device("cpu"))
    codes = lambda t: np.clip(np.rint((t.numpy()[0].astype(F64) + 1.0) * 127.5), 0, 255).astype(np.uint8)
    read = lambda: np.array(Image.open(str(tmp_path / "out.png"))).transpose(2, 0, 1)
    # one new flag
    assert tool.main(io_ + ["--kernel", "aniso:7:2.0:0.6:0.5"]) == 0
    want = ops.filter2d(x, [KB.bank_kernel("aniso", 7, 2.0, 0.6, 0.5)])
    assert np.array_equal(read(), codes(want)) and not np.array_equal(read(), src)
    # all of them, in the loader's order
    assert tool.main(io_ + ["--sinc", "2.0:9", "--filter", "area", "--scale", "2", "--blur", "0.8", "--shot", "1.2", "--grey", "--jpeg", "60",
                            "--seed", "3", "--second", "--kernel plateau_iso:5:1.0:1.0:0:1.5 --noise 3 --grey --jpeg 50 --sinc 2.5:7"]) == 0
    t = ops.filter2d(x, [KB.sinc_kernel(2.0, 9)])
    t = ops.resize_select(t, ops.ResizeTables([DL.resize_taps(28, 14, "area")], [DL.resize_taps(20, 10, "area")], 20, 28, "cpu"), [0])
    t = ops.degrade_blur_noise(t, [0.8], None, None)
    t = ops.degrade_noise_kinds(t, [1.2], [H.SHOT | H.GREY], [tool.seed_words(3)])
    t = ops.jpeg_roundtrip(t, [60], "420")
    t = ops.filter2d(t, [KB.bank_kernel("plateau_iso", 5, 1.0, 1.0, 0.0, 1.5)])
    t = ops.degrade_noise_kinds(t, [3.0], [H.GREY], [tool.seed_words(4)])
    t = ops.filter2d(ops.jpeg_roundtrip(t, [50], "420"), [KB.sinc_kernel(2.5, 7)])
    assert read().shape == (3, 10, 14) and np.array_equal(read(), codes(t))
    with pytest.raises(SystemExit):
        tool.main(io_ + ["--kernel", "iso:7"])
    with pytest.raises(SystemExit):
        tool.main(io_ + ["--filter", "area", "--scale", "3"])
