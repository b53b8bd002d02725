"""Sharp gates for the degradation kernels (csrc/degrade.hip): test_degrade.py holds them to tolerances that a wrong
tap, an off-by-one uniform or a mistyped table entry passes; this file closes those gaps.  Every device case runs on the emulator
and, under `-m gpu`, on the MI355X; none is GPU-only (see the end).

A. Blur, BIT-EXACT.  fsr_degrade_blur_noise takes taps and radii from the caller, so the tables here are C.dyadic_taps: signed
   non-zero multiples of 1/16 that sum to 1 and differ from their mirror image, the slots behind 2 r + 1 poisoned with 1e30; inputs in
   steps of 1/64 in [-1, 1].  Pass 1 then is a multiple of 2^-10 and pass 2 of 2^-14, and every partial sum, in any order, is bounded by
   (sum |w|)^2 -- the weights are SIGNED (nineteen positive sixteenths cannot sum to 1 without a zero tap, and a zero tap hides its
   own index), so the bound is sum |w| <= 4 and not 1: 2^4 / 2^-14 = 2^18 < 2^24, float32 holds every intermediate with or without FMA
   contraction.  The premise is asserted on the float64 reference; the gate is tobytes() equality with float64 cast to float32.

B. Noise, float64 with a derived cap, element by element:
       |got - (x + z64 sigma 2/255)|  <=  K 2^-23 max(R, 1) sigma (2/255) + 2^-24 |ref|,      R = sqrt(-2 ln u1) of that element
   (z = R cos(2 pi u2): one ulp of logf, sqrtf, cosf or of the argument 6.2831855 u2 <= 2 pi is a few 2^-23 of R; the last term is
   the rounding of the sum, which any correct float32 result may use in full and which therefore stays out of the count).  K = 16 is
   the smallest power of two that keeps the float32 numpy restatement of the contract inside a third of K units on the inputs of the
   cases (test_float32_noise_restatement_is_inside_a_third_of_the_cap; project rule of test_stream_exact.py): 8 / 3 = 2.67 is not
   enough for the 2.76 the restatement reaches among the 10^6 elements of the grid-wrap input (2.34 on the others).  Measured beyond
   2^-24 |ref|, in units of 2^-23 max(R, 1) sigma 2/255: restatement 2.76, emulator 2.63, MI355X 2.71 (2.30 at indices >= 2^24) --
   the device's logf / cosf need no more than numpy's.  The u1 off-by-one of the self-test is 34 to 125 units.
   The seeds of the extreme draws (u1 = 2^-24: the largest |z| = 5.77; u1 = 1: z = +-0) are not searched for: mix32 is a bijection,
   C.seed_for_draw inverts it and names the seed word that puts the wanted draw at the wanted element.

C. JPEG, every table entry compared at every regime of the scale, CAP = 1e-3 (the project's assert_codes_close):
   C1 C.every_position_image: per quality (1: every Q clamped to 255; 10: clamped and not; 35, 49, 50, 75; 99: entries clamped to 1)
      and subsampling all 64 luminance and all 64 chrominance positions are quantised to |k| >= 1.  Premises, asserted before a
      kernel runs: all positions live, every coefficient >= 0.3 steps from a tie (0.400 measured), every pixel in [4, 251], float32
      contract against float64: at most CAP / 3 of the codes -- measured 0 of 12288 .. 61440 at every quality but "420" q = 99: 2 of
      24576.  The emulator and the MI355X differ from float64 on those same 2 codes and on no other.
   C2 C.threshold_probe_image at q = 50 (Q = the base table): per entry a coefficient (K + 0.5 +- 0.012) Q, so that an entry off by
      ONE flips a rounding.  All 128 entries have probes; float32 against float64, and both backends: 0 codes on all four images.
   C3 (CPU, contract only) each of the 128 base entries at +-25 % (at least 1) changes the contract's codes on the C1 inputs by more
      than assert_codes_close admits, and at +-1 on the C2 inputs: none is missed, no entry had to be left out of C2.
   C4 a batch of four qualities (10, 50, 0, 90) with several tiles per sample: each sample bit-equal to itself run alone.
   C5 lives in test_degrade.py: (1, 1), (16, 17) and (15, 33) on the arbitrary leg.

GPU only: nothing.  The largest cases -- the grid wrap (n = 3, 344 x 344: 1 065 024 elements, more than the 4096 x 256 threads the
capped grid covers in one trip) and test_noise_beyond_2_to_the_24 (16.8 M elements, 67 MB) -- take 1.0 s and 1.6 s on the emulator,
well under the ten seconds above which a case would go to the GPU alone.

Every measured maximum goes to the parity-error log through backend.report (degrade.*)."""
import functools

import numpy as np
import pytest
import torch

import degrade_contract as C
from backend import BACKENDS, L, ops, report, select

F32, F64 = np.float32, np.float64
U = 2.0 ** -23
K_NOISE = 16
CAP = 1e-3                 # as in test_degrade.py: the share of codes that may differ (by one) from the float64 contract
C1_QUALITIES = (1, 10, 35, 49, 50, 75, 99)
SUBS = ("420", "444")
_where, _worst = ["-"], {}


@pytest.fixture(params=BACKENDS)
def dev(request):
    _where[0] = request.param
    return select(request.param)


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)               # a copy: the shared fixtures are read-only


def _steps(shape, seed):
    """float32 in steps of 1/64 in [-1, 1]"""
    return (np.random.RandomState(seed).randint(-64, 65, size=shape) / 64.0).astype(F32)


def _launch(dev, x, taps=None, radii=None, sigma=None, seeds=None):
    """fsr_degrade_blur_noise through the C ABI with the caller's tables (ops.degrade_words would refuse these taps and radii)."""
    xt = _t(x, dev)
    out = torch.empty_like(xt)
    blur, noise = taps is not None, sigma is not None
    tmp = torch.empty_like(xt) if blur else None
    tt = _t(np.asarray(taps, F32), dev) if blur else None
    rr = _t(np.asarray(radii, np.int32), dev) if blur else None
    ss = _t(np.asarray(sigma, F32), dev) if noise else None
    dd = _t(np.asarray(seeds, np.int64).astype(np.uint32).view(np.int32).reshape(-1), dev) if noise else None
    p = ops._p
    L.check(L.lib().fsr_degrade_blur_noise(p(xt), p(out), p(tmp), x.shape[0], x.shape[2], x.shape[3], p(tt), p(rr), p(ss), p(dd),
                                           ops._stream()), "fsr_degrade_blur_noise")
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ gates
def _note(key, value):
    """The largest value of a key so far goes to the parity-error log as degrade.<backend>.<key>."""
    key = "degrade.%s.%s" % (_where[0], key)
    if value > _worst.get(key, -1.0):
        _worst[key] = value
        report(key, value)


def exact_blur(what, got, x, radii, taps, widest):
    """THE blur comparison: the premise on the float64 reference, then bit equality."""
    ref, mid = C.np_blur_taps(x, radii, taps, passes=True)
    assert widest <= 4.0
    assert np.array_equal(mid * 2.0 ** 10, np.rint(mid * 2.0 ** 10)) and np.abs(mid).max() <= widest, "%s: premise (pass 1)" % what
    assert np.array_equal(ref * 2.0 ** 14, np.rint(ref * 2.0 ** 14)) and np.abs(ref).max() <= widest ** 2, "%s: premise (pass 2)" % what
    assert np.array_equal(ref.astype(F32).astype(F64), ref)
    if got is not None:
        bad = got.view(np.uint32) != ref.astype(F32).view(np.uint32)
        assert got.tobytes() == ref.astype(F32).tobytes(), "%s: %d of %d elements differ, first at %s" % (
            what, bad.sum(), bad.size, tuple(int(v) for v in np.argwhere(bad)[0]))
    return ref


def noise_reference(x, sigma, seed, idx=None):
    """One sample ((3,h,w), or the elements `idx` of its flattened form): (x + z64 sigma 2/255, the unit of B's cap, the cap) in float64."""
    x = np.asarray(x, F64)
    z, rad = C.np_z(x.size if idx is None else idx, seed[0], seed[1], radius=True)
    z, rad = z.reshape(x.shape), rad.reshape(x.shape)
    ref = x + z * (float(sigma) * (2.0 / 255.0))
    unit = U * np.maximum(rad, 1.0) * float(sigma) * (2.0 / 255.0)
    return ref, unit, K_NOISE * unit + 2.0 ** -24 * np.abs(ref)


def _units(got, ref, unit):
    """The error beyond the rounding of the sum (2^-24 |ref|), in the units K counts."""
    return float((np.maximum(np.abs(np.asarray(got, F64) - ref) - 2.0 ** -24 * np.abs(ref), 0.0) / unit).max())


def noise_gate(what, got, x, sigmas, seeds, log=True):
    """THE noise comparison of a batch; the largest error beyond the rounding of the sum, in the units K counts, goes to the log."""
    worst = 0.0
    for i, (s, sd) in enumerate(zip(sigmas, seeds)):
        if s == 0:
            assert got[i].tobytes() == np.asarray(x[i], F32).tobytes(), "%s: sample %d (sigma 0) is not a copy" % (what, i)
            continue
        ref, unit, cap = noise_reference(x[i], s, sd)
        ratio = np.abs(got[i].astype(F64) - ref) / cap
        j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        worst = max(worst, _units(got[i], ref, unit))
        print("%s: sample %d sigma %g: largest error / cap %.3f, %.3f units" % (what, i, s, ratio[j], _units(got[i], ref, unit)))
        assert ratio[j] <= 1.0, "%s: sample %d, element %s: got %.9g, want %.9g, cap %.3g" % (what, i, j, got[i][j], ref[j], cap[j])
    if log:
        _note("noise_units", worst)
    return worst


# ---------------------------------------------------------------------------------------------------------------- A. blur
# (h, w, radii): h or w of 1 with r = 9 (every tap clamped); h, w < r; h, w = r + 1, 2 r, 2 r + 1 for r = 4 and 9; rows that cross the
# 256-thread stride; neighbouring samples with r = 0, 1, 9, 4 (a copy next to the widest blur: a sample index off by one shows);
# radii -3 and 12 with full tables, which the kernel's documented clamp makes a copy and r = 9 -- both stay inside the 19 slots.
BLUR_CASES = [(1, 1, (9, 0, 3)), (1, 23, (9, 1)), (23, 1, (9, 1)), (3, 5, (9, 6, 4)), (5, 5, (4,)), (8, 8, (4,)), (9, 9, (4, 7)),
              (10, 18, (9,)), (18, 10, (9,)), (19, 19, (9, 2)), (6, 7, (0, 1, 9, 4, 0)), (19, 130, (0, 1, 9, 4)), (7, 11, (-3, 12, 5))]
NOISE_SIGMAS = (25.0, 0.0, 0.7)
NOISE_SEEDS = ((0, 0), (5, 6), (0xffffffff, 0xfffffffe))       # the last: s0 + 2 e + 1 wraps through 2^32 inside the sample


def _blur_case(dev, h, w, radii, seed):
    n = len(radii)
    x = _steps((n, 3, h, w), seed)
    x[0, 0, 0, 0] = -0.0
    taps, widest = C.dyadic_taps(radii, seed)
    what = "blur %dx%d r=%s" % (h, w, list(radii))
    got = _launch(dev, x, taps, radii)
    assert L.lib().fsr_last_kernel() == b"blur_hpass_kernel+blur_vpass_kernel"
    ref = exact_blur(what, got, x, radii, taps, widest)
    for i, r in enumerate(radii):
        if r <= 0:
            assert got[i].tobytes() == x[i].tobytes()            # a copy, the sign of a zero included
    # the fused launch = the exact blur, then the noise-only launch, bit for bit; its noise obeys the cap of B
    sig = [NOISE_SIGMAS[i % 3] for i in range(n)]
    seeds = [NOISE_SEEDS[(i + 1) % 3] for i in range(n)]
    fused = _launch(dev, x, taps, radii, sig, seeds)
    assert L.lib().fsr_last_kernel() == b"blur_hpass_kernel+blur_vpass_noise_kernel"
    two = _launch(dev, got, None, None, sig, seeds)
    assert fused.tobytes() == two.tobytes(), what
    noise_gate(what + " fused", fused, ref, sig, seeds)


@pytest.mark.parametrize("h,w,radii", BLUR_CASES)
def test_blur_is_bit_exact(dev, h, w, radii):
    _blur_case(dev, h, w, radii, seed=100 + 7 * h + w)


def test_blur_grid_wrap(dev):
    """3 x 3 x 344 x 344 = 1 065 024 elements: the capped grid of 4096 x 256 threads takes a second trip, with the sample boundaries
    (at 355 008 and 710 016) inside the first."""
    _blur_case(dev, 344, 344, (3, 9, 1), seed=5)


# --------------------------------------------------------------------------------------------------------------- B. noise
def _noise_inputs():
    """[(name, x, sigmas, seeds)] of the emulator-sized noise cases (the restatement test measures K on exactly these)."""
    cases = []
    for name, x in (("zero", np.zeros((3, 3, 19, 30), F32)), ("steps", _steps((3, 3, 19, 30), 1))):
        x[1, 2, 3, 4] = -0.0
        cases.append((name, x, list(NOISE_SIGMAS), list(NOISE_SEEDS)))
    # extreme draws: a >> 8 == 0 (u1 = 2^-24, R = 5.77) and a >> 8 == 0xffffff (u1 = 1, z = +-0) at chosen elements of a 3 x 5 x 7 sample
    want = [(0x00000037, 41, 25.0), (0xffffff12, 100, 25.0), (0x000000ff, 104, 0.7), (0xffffff00, 0, 0.7)]
    seeds = [(C.seed_for_draw(a, e, 0x9e3779b9 + i), 0x9e3779b9 + i) for i, (a, e, _) in enumerate(want)]
    for (a, e, _), (s0, s1) in zip(want, seeds):
        assert int(C.hash_draws(105, s0, s1)[0][e]) == a >> 8
    cases.append(("extreme", _steps((4, 3, 5, 7), 2), [s for _, _, s in want], seeds))
    return cases


@pytest.mark.parametrize("case", range(3))
def test_noise_against_float64(dev, case):
    name, x, sig, seeds = _noise_inputs()[case]
    got = ops.degrade_blur_noise(_t(x, dev), None, sig, seeds).cpu().numpy()
    assert L.lib().fsr_last_kernel() == b"noise_kernel"
    noise_gate("noise " + name, got, x, sig, seeds)
    if name == "extreme":
        z = (got.astype(F64) - x) / (np.asarray(sig)[:, None, None, None] * 2.0 / 255.0)
        z = z.reshape(4, -1)
        print("extreme draws: z = %.4f, %.4g, %.4f, %.4g" % (z[0, 41], z[1, 100], z[2, 104], z[3, 0]))
        assert got[1].reshape(-1)[100] == x[1].reshape(-1)[100] and got[3].reshape(-1)[0] == x[3].reshape(-1)[0]      # z = +-0


def test_noise_grid_wrap(dev):
    """1 065 024 elements (see test_blur_grid_wrap), noise only, three seeds and a copied sample in the middle."""
    x = _steps((3, 3, 344, 344), 6)
    sig, seeds = [0.7, 0.0, 25.0], [(0xffffffff, 0xfffffffe), (1, 2), (0, 0)]
    got = ops.degrade_blur_noise(_t(x, dev), None, sig, seeds).cpu().numpy()
    noise_gate("noise wrap", got, x, sig, seeds)


def _big_noise_input():
    """(x, sigma, seed, the element indices compared) of the 16 822 272-element case."""
    total = 3 * 2368 * 2368
    assert total > 2 ** 24 + 4096
    idx = np.unique(np.concatenate([np.arange(0, total, 4099), np.arange(total - 4096, total), np.arange(2 ** 24 - 64, 2 ** 24 + 64)]))
    return _steps((1, 3, 2368, 2368), 7), 25.0, (0xfffffff0, 12345), idx


def test_noise_beyond_2_to_the_24(dev):
    """16 822 272 elements (67 MB): element indices of 2^24 and above, where a float conversion of the index would lose bits.  Compared:
    the last 4096 elements, 128 around 2^24 and every 4099th."""
    x, sigma, seed, idx = _big_noise_input()
    got = ops.degrade_blur_noise(_t(x, dev), None, [sigma], [seed]).cpu().numpy().reshape(-1)
    ref, unit, cap = noise_reference(x.reshape(-1)[idx], sigma, seed, idx)
    ratio = np.abs(got[idx].astype(F64) - ref) / cap
    print("noise 2^24: %d elements compared, largest error / cap %.3f, %.3f units" % (idx.size, ratio.max(), _units(got[idx], ref, unit)))
    _note("noise_units_2_24", _units(got[idx], ref, unit))
    assert ratio.max() <= 1.0, (int(idx[np.argmax(ratio)]), ratio.max())


def _restatement(x, sigma, seed, idx=None):
    """The contract's noise in plain float32 numpy."""
    z = C.np_z(x.size if idx is None else idx, seed[0], seed[1], ft=F32).reshape(x.shape)
    return x.astype(F32) + z * F32(F32(sigma) * F32(2.0 / 255.0))


def test_float32_noise_restatement_is_inside_a_third_of_the_cap():
    """K_NOISE by the project's rule: the smallest power of two for which the float32 restatement stays within a third of K units, on the
    inputs of the cases (the grid-wrap input and the compared elements of the 2^24 case included).  The other term of the cap,
    2^-24 |ref|, is the rounding of the sum itself: any correct float32 result uses up to all of it (the restatement reaches 0.85 of the
    whole cap at sigma = 0.7, x = 1), so the error is counted beyond it."""
    worst = 0.0
    cases = _noise_inputs() + [("wrap", _steps((3, 3, 344, 344), 6), [0.7, 0.0, 25.0], [(0xffffffff, 0xfffffffe), (1, 2), (0, 0)])]
    for name, x, sig, seeds in cases:
        for i, (s, sd) in enumerate(zip(sig, seeds)):
            if s == 0:
                continue
            ref, unit, cap = noise_reference(x[i], s, sd)
            got = _restatement(x[i], s, sd)
            assert (np.abs(got.astype(F64) - ref) <= cap).all()
            worst = max(worst, _units(got, ref, unit))
    x, sigma, seed, idx = _big_noise_input()
    ref, unit, cap = noise_reference(x.reshape(-1)[idx], sigma, seed, idx)
    got = _restatement(x.reshape(-1)[idx], sigma, seed, idx)
    assert (np.abs(got.astype(F64) - ref) <= cap).all()
    worst = max(worst, _units(got, ref, unit))
    print("float32 restatement of the noise: %.3f units of 2^-23 max(R, 1) sigma 2/255 (K = %d)" % (worst, K_NOISE))
    assert worst <= K_NOISE / 3.0
    assert K_NOISE == 1 or worst > K_NOISE / 6.0, "a smaller K would do"


# ---------------------------------------------------------------------------------------------------------------- C. JPEG
def _float32_premise(what, x, q, sub, want):
    d = int((C.np_jpeg_codes(x, q, sub, F32) != want).sum())
    print("%s: float32 contract against float64: %d of %d codes differ" % (what, d, want.size))
    assert d <= CAP / 3 * want.size, (what, d, want.size)
    return d


@functools.lru_cache(maxsize=None)
def _every_position(q, sub, stagger=None):
    """(image, float64 codes) of C1, shared and left unchanged; the builder asserts liveness, range and tie distance, this the float32 room."""
    x = C.every_position_image(q, sub, seed=q, stagger=stagger)
    want = C.np_jpeg_codes(x, q, sub)
    _float32_premise("every position q=%d %s" % (q, sub), x, q, sub, want)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


@functools.lru_cache(maxsize=None)
def _probes(plane, sub):
    x = C.threshold_probe_image(plane, sub)
    want = C.np_jpeg_codes(x, 50, sub)
    _float32_premise("probes %s %s" % (plane, sub), x, 50, sub, want)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def _jpeg(dev, x, qs, sub):
    got = ops.jpeg_roundtrip(_t(x, dev), qs, sub).cpu().numpy()
    assert L.lib().fsr_last_kernel() == b"jpeg_roundtrip_kernel<%s>" % sub.encode()
    return got


def _codes_gate(key, got, want):
    """assert_codes_close at CAP; the share of codes that differ goes to the log."""
    codes = C.value_to_codes(got)
    _note(key, float((codes != want).mean()))
    C.assert_codes_close(codes, want, CAP)


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("q", C1_QUALITIES)
def test_jpeg_every_position(dev, q, sub):
    x, want = _every_position(q, sub)
    _codes_gate("jpeg_every_position_differ", _jpeg(dev, x[None], [q], sub)[0], want)


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("plane", ["luma", "chroma"])
def test_jpeg_threshold_probes(dev, plane, sub):
    x, want = _probes(plane, sub)
    _codes_gate("jpeg_probes_differ", _jpeg(dev, x[None], [50], sub)[0], want)


def _rejected(got, want):
    """What assert_codes_close(got, want, CAP) refuses."""
    d = np.abs(got - want)
    return d.max() > 1 or (d > 0).sum() > CAP * d.size


def _tables(t, u, v, delta):
    tabs = [C.LUMA.copy(), C.CHROMA.copy()]
    tabs[t][u, v] += delta
    return tabs


def _quarter(t, u, v, sign):
    return sign * max(1, int(round(0.25 * (C.LUMA, C.CHROMA)[t][u, v])))


def test_every_table_entry_is_seen():
    """C3, on the contract alone: no kernel runs.  Each of the 128 base-table entries, moved by +-25 % (at least 1), changes the codes
    of some C1 input beyond what assert_codes_close admits; moved by +-1, those of the C2 inputs."""
    order = sorted(C1_QUALITIES, key=lambda q: abs(q - 42))          # the middle of the scale sees most entries: ask it first
    missed = []
    for t, plane in enumerate(("luma", "chroma")):
        for p in range(64):
            u, v = divmod(p, 8)
            for sign in (1, -1):
                tabs = _tables(t, u, v, _quarter(t, u, v, sign))
                if not any(_rejected(C.np_jpeg_codes(_every_position(q, s)[0], q, s, tables=tabs), _every_position(q, s)[1])
                           for s in reversed(SUBS) for q in order):
                    missed.append((plane, u, v, "%+d %%" % (25 * sign)))
                tabs = _tables(t, u, v, sign)
                for s in SUBS:
                    if not _rejected(C.np_jpeg_codes(_probes(plane, s)[0], 50, s, tables=tabs), _probes(plane, s)[1]):
                        missed.append((plane, u, v, s, "%+d" % sign))
    print("entries not seen:", missed)
    assert not missed


@pytest.mark.parametrize("sub", SUBS)
def test_jpeg_mixed_batch(dev, sub):
    """C4: n = b / tiles_y and quality[n] on a batch whose samples have different live tables and 4 x 8 (5 x 16 at "420") tiles each."""
    qs = [10, 50, 0, 90]
    pairs = [_every_position(q if q else 35, sub, True) for q in qs]
    x = np.stack([p[0] for p in pairs])
    x[2, 1, 3, 5] = -0.0
    got = _jpeg(dev, x, qs, sub)
    for i, q in enumerate(qs):
        alone = _jpeg(dev, x[i:i + 1], [q], sub)[0]
        assert got[i].tobytes() == alone.tobytes(), "sample %d (q = %d) depends on its batch" % (i, q)
        if q == 0:
            assert got[i].tobytes() == x[i].tobytes()
        else:
            _codes_gate("jpeg_mixed_differ", got[i], pairs[i][1])


# ------------------------------------------------------------------------------------------------------------ D. self-test
def test_new_gates_are_sharper_than_the_old_ones():
    """No kernel is launched; each error is applied to the REFERENCE.
    (a) u1 without its + 1: passes the old noise gate (2e-5 sigma 2/255 + 1e-7) on the first sample of the old input (seed (0, 0),
        sigma 25: 3.09e-6 against 4.02e-6) and fails the cap of B on every sample of the new one.  (The old gate does refuse it on its
        third sample, 3.97e-7 against 2.10e-7: sigma = 0.7 leaves less room and that seed draws a smaller u1.)
    (b) one blur tap's weight moved to its neighbour.  By 1/16, the new exact gate fails it -- but so does the old gate on its random
        inputs (error 1.0e-1 against 1e-5: the issue's expectation that it would pass does not hold), so the side "the old gate passes"
        is shown with the largest power of two that it does pass, 2^-18 of weight, which the exact gate fails as well.
    (c) LUMA[6][5] at -25 % (121 -> 91): every code of every tie-free input of test_degrade.py is unchanged, the C1 inputs are refused."""
    # (a)
    old_x = np.random.RandomState(3).uniform(-1.0, 1.0, size=(3, 3, 19, 30)).astype(F32)
    for x, gate_is_old in ((old_x, True), (_noise_inputs()[1][1], False)):
        for i, (s, sd) in enumerate(zip(NOISE_SIGMAS, NOISE_SEEDS)):
            if s == 0:
                continue
            z, zbad = (C.np_z(x[i].size, sd[0], sd[1], plus=plus).reshape(x[i].shape) for plus in (1, 0))
            ref, bad = (x[i].astype(F64) + v * (s * 2.0 / 255.0) for v in (z, zbad))
            if gate_is_old:
                err = np.abs(bad.astype(F32) - ref).max()
                print("u1 off by one, sample %d: max |error| %.3e, old gate %.3e" % (i, err, 2e-5 * s * (2.0 / 255.0) + 1e-7))
                assert i != 0 or 0 < err < 2e-5 * s * (2.0 / 255.0) + 1e-7
            else:
                noise_gate("uncorrupted", ref.astype(F32)[None], x[i:i + 1], [s], [sd], log=False)
                with pytest.raises(AssertionError):
                    noise_gate("u1 off by one", bad.astype(F32)[None], x[i:i + 1], [s], [sd], log=False)
    # (b)
    def moved(taps, r, weight):
        t = np.array(taps, dtype=F64)
        t[r + 2] -= weight
        t[r + 3] += weight
        return t

    old_x = np.random.RandomState(10 + 24).uniform(-1.0, 1.0, size=(1, 3, 24, 24)).astype(F32)
    r, taps = C.blur_taps(3.0)
    ref = C.np_blur(old_x, [3.0])
    for weight, passes in ((1.0 / 16.0, False), (2.0 ** -18, True)):
        err = np.abs(C.np_blur_taps(old_x, [r], [moved(taps, r, weight)]).astype(F32) - ref).max()
        print("tap moved by %g: max |error| on the old input %.3e (old gate 1e-5)" % (weight, err))
        assert (err < 1e-5) == passes
    x = _steps((1, 3, 19, 19), 3)
    taps, widest = C.dyadic_taps([9], 3)
    ref = exact_blur("uncorrupted", None, x, [9], taps, widest)
    exact_blur("uncorrupted", ref.astype(F32), x, [9], taps, widest)
    for weight in (1.0 / 16.0, 2.0 ** -18):
        bad = C.np_blur_taps(x, [9], [moved(taps[0], 9, weight)]).astype(F32)
        with pytest.raises(AssertionError):
            exact_blur("tap moved", bad, x, [9], taps, widest)
    # (c)
    tabs = _tables(0, 6, 5, _quarter(0, 6, 5, -1))
    old = [(C.tie_free_image(h, w, q, s, seed=q + h), q, s) for s in SUBS for q in (20, 50, 90) for h, w in ((16, 16), (32, 48), (96, 96))]
    for x, q, s in old:
        assert np.array_equal(C.np_jpeg_codes(x, q, s, tables=tabs), C.np_jpeg_codes(x, q, s))
    assert any(_rejected(C.np_jpeg_codes(_every_position(q, s)[0], q, s, tables=tabs), _every_position(q, s)[1])
               for s in SUBS for q in C1_QUALITIES)
