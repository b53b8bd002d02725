"""fsr_adamw_step_ex through the C ABI: the AdamW step with a device-side learning-rate schedule and a fused EMA.

The update itself carries NO tolerance anywhere in this file: with the learning rate the kernel reports in lr_used, p, m, v and the step
counter are compared bit for bit with fsr_adamw_step / fsr_adamw_step_scaled (the by-value entry points, which
tests/test_stream_exact.py holds to float64 and tests/test_adamw_bits.py to recorded bits: another instantiation of the same template)
on copies of the same inputs -- at every vector tail length, one workgroup + 1, past the grid cap and through pointers that are not
16-byte aligned.  What is left is the rate and the average:

  * constant / multistep: lr_used == float32(base gamma^k) exactly, the clock counts the calls, slots behind nb are never read (NaN);
  * warm-up and cosine:   |lr_used - lr64| <= K_LR 2^-23 base_lr, lr64 the float64 contract from the block's float32 words;
  * EMA on a 2^-6 grid with dyadic decays: every product exact, so ema' equals the float64 contract bit for bit;
  * EMA in general:       |ema' - ema64| <= K_EMA 2^-23 (|ema| + |p'|) per element, ema64 from the kernel's own float32 p'.

K by the rule of tests/test_stream_exact.py: the smallest power of two (>= 1) for which the float32 numpy restatement
(optim_contract.lr32 / ema32: one rounding per operation) stays inside a THIRD of the cap on the very inputs of the cases
(test_float32_restatement_is_inside_a_third_of_the_caps).  Measured, in units of 2^-23 x the scale:

    quantity       K    restatement   emulator   MI355X   scale
    lr (cosine)    1    0.29          0.29       0.29     base_lr
    lr (warm-up)   1    0.08          0.08       0.08     base_lr
    ema            2    0.42          0.43       0.43     |ema| + |p'|

(the restatement's 0.42 for the average is over a third of K = 1, hence K = 2: p' - ema cancels, the difference's rounding is up to half
an ulp of the LARGER operand, and 1 - 0.999 scales it down before the sum rounds once more.)

A skipped step (non-finite flag up) leaves p, m, v, ema, the step counter, all 32 words of the block and the scale state bit-identical.
"""
import functools

import numpy as np
import pytest
import torch

import optim_contract as C
from backend import BACKENDS, L, ops, report, select

F32, F64 = np.float32, np.float64
U = 2.0 ** -23
HP = dict(b1=0.9, b2=0.999, eps=1e-8)
GSCALE, LOSS_SCALE = 0.5, 1024.0
BIG = 2048 * 1024 + 7                          # past the 2048-workgroup grid cap
COUNTS = (1, 3, 5, 1025, BIG)                  # vector tails of 1..3, one workgroup's 1024 + 1, a second grid pass
K_LR, K_EMA = 1, 2


@functools.lru_cache(maxsize=4)
def _inputs(step0, count):
    return C.adam_inputs(step0, count)


def _dev(a, dev, offset=0):
    """A device copy of `a`; offset = 1: placed one float behind its allocation's start (not 16-byte aligned)."""
    t = torch.zeros(a.size + offset, dtype=torch.float32)
    t[offset:] = torch.from_numpy(np.ascontiguousarray(a, dtype=F32))
    return t.to(dev)[offset:]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(what, got, want):
    want = want if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want, dtype=F32))
    a, b = _bits(got), _bits(want)
    assert a.shape == b.shape, what
    bad = (a != b).nonzero()
    assert bad.numel() == 0, "%s: %d of %d differ, first at %s" % (what, bad.shape[0], a.numel(), bad[0].tolist())


def _ex(p, g, m, v, ema, sched, step, wd=0.0, state=None, decay=0.0, gs=GSCALE):
    L.check(L.lib().fsr_adamw_step_ex(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None if ema is None else ema.data_ptr(),
                                      p.numel(), sched.data_ptr(), HP["b1"], HP["b2"], HP["eps"], wd, step.data_ptr(), gs,
                                      None if state is None else state.data_ptr(), decay, ops._stream()), "fsr_adamw_step_ex")


def _old(p, g, m, v, lr, step, wd=0.0, state=None, gs=GSCALE):
    lib = L.lib()
    if state is None:
        L.check(lib.fsr_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, HP["b1"], HP["b2"], HP["eps"], wd,
                                   step.data_ptr(), gs, ops._stream()), "fsr_adamw_step")
    else:
        L.check(lib.fsr_adamw_step_scaled(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, HP["b1"], HP["b2"], HP["eps"], wd,
                                          step.data_ptr(), gs, state.data_ptr(), ops._stream()), "fsr_adamw_step_scaled")


def _block(dev, *a, **k):
    return torch.from_numpy(C.block(*a, **k)).to(dev)


class _Twin:
    """Two copies of one problem: `a` stepped by fsr_adamw_step_ex, `b` by the by-value entry point at the rate `a` reports."""

    def __init__(self, dev, step0, count, scaled=False, offset=0, ema=None):
        p, g, m, v = _inputs(step0, count)
        self.g = _dev(g * F32(LOSS_SCALE) if scaled else g, dev, offset)
        self.a = [_dev(x, dev, offset) for x in (p, m, v)]
        self.b = [_dev(x, dev, offset) for x in (p, m, v)]
        self.steps = [torch.tensor([float(step0)]).to(dev) for _ in range(2)]
        self.states = [torch.tensor([LOSS_SCALE, 0.0, 0.0, 0.0]).to(dev) for _ in range(2)] if scaled else [None, None]
        self.ema = None if ema is None else _dev(ema, dev, offset)

    def step(self, sched, wd, decay=0.0):
        """One call of each; returns (lr_used, clock) after asserting p, m, v and the step counters bit-equal."""
        (pa, ma, va), (pb, mb, vb) = self.a, self.b
        _ex(pa, self.g, ma, va, self.ema, sched, self.steps[0], wd, self.states[0], decay)
        self.kernel = L.lib().fsr_last_kernel().decode()
        w = sched.cpu().numpy()
        _old(pb, self.g, mb, vb, float(w[C.LR_USED]), self.steps[1], wd, self.states[1])
        for what, x, y in (("p", pa, pb), ("m", ma, mb), ("v", va, vb), ("step counter", self.steps[0], self.steps[1])):
            _same(what, x, y)
        if self.states[0] is not None:
            _same("loss-scale state", self.states[0], self.states[1])
        return w[C.LR_USED], w[C.CLOCK]


# ------------------------------------------------------------------------------------------------- bit identity with the by-value entry points
@pytest.mark.parametrize("scaled", (False, True))
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("wd", (0.0, 0.01))
@pytest.mark.parametrize("step0", (0, 9, 999))
@pytest.mark.parametrize("backend", BACKENDS)
def test_constant_schedule_is_bit_identical_with_the_existing_kernels(backend, step0, wd, count, scaled):
    dev = select(backend)
    T = _Twin(dev, step0, count, scaled)
    sched = _block(dev, "constant", 1e-4)
    lr, clock = T.step(sched, wd)
    assert lr == F32(1e-4) and clock == 1.0
    assert float(T.steps[0]) == step0 + 1
    assert T.kernel == "adamw_ex_kernel<noema,%s,%s>" % ("scaled" if scaled else "plain", "x4" if count >= 4 else "x1"), T.kernel
    assert L.lib().fsr_last_kernel().decode() == ("adamw_scaled_kernel" if scaled else "adamw_kernel")


@pytest.mark.parametrize("scaled", (False, True))
@pytest.mark.parametrize("backend", BACKENDS)
def test_unaligned_pointers_take_the_scalar_path_bit_identically(backend, scaled):
    dev = select(backend)
    T = _Twin(dev, 9, 1025, scaled, offset=1)
    assert all(t.data_ptr() % 16 == 4 for t in T.a + [T.g])
    lr, clock = T.step(_block(dev, "constant", 1e-4), 0.01)
    assert lr == F32(1e-4) and clock == 1.0
    assert T.kernel == "adamw_ex_kernel<noema,%s,x1>" % ("scaled" if scaled else "plain")


# ------------------------------------------------------------------------------------------------- multistep
@pytest.mark.parametrize("milestones", [(2, 3, 7), (1, 2, 4, 5, 6, 8, 9, 11), ()], ids=["nb3", "nb8", "nb0"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_multistep_rates_are_exact_and_the_update_is_the_old_kernels(backend, milestones):
    """Ten consecutive calls: lr_used == float32(base gamma^k) with k = #{milestones <= clock before the call} (a milestone k takes effect
    for update k + 1), the clock equals the call number, and the arena equals a twin stepped by fsr_adamw_step at that rate.  The slots
    behind the nb boundaries and nb + 1 values hold NaN."""
    dev = select(backend)
    base, gamma = 1e-4, 0.5
    T = _Twin(dev, 9, 1029)
    sched = _block(dev, "multistep", base, milestones=milestones, gamma=gamma, poison=True)
    for call in range(1, 11):
        lr, clock = T.step(sched, 0.01)
        k = sum(1 for b in milestones if b <= call - 1)
        assert lr == F32(F64(base) * F64(gamma) ** k), (call, lr)
        assert clock == float(call)
    assert float(T.steps[0]) == 19.0


# ------------------------------------------------------------------------------------------------- warm-up and cosine
LR_BASE = 1e-4
COSINE = [dict(kind="cosine", base=LR_BASE, total=10, min_lr=1e-6, warmup=w, clock=c) for w in (0, 3) for c in (0, 5, 10, 25)]
WARMUP_MULTISTEP = dict(kind="multistep", base=LR_BASE, milestones=(2, 3, 7), gamma=0.5, warmup=4)


def _lr_units(w, got):
    return abs(float(got) - C.lr64(w)) / (U * float(F32(LR_BASE)))


def _lr_rows():
    """Every (block, clock) the rate cases evaluate: the warm-up multistep over ten calls, each cosine block at its preset clock and the
    one after."""
    rows = [(C.block(**WARMUP_MULTISTEP), e) for e in range(10)]
    for kw in COSINE:
        rows += [(C.block(**kw), kw["clock"]), (C.block(**kw), kw["clock"] + 1)]
    return rows


@pytest.mark.parametrize("backend", BACKENDS)
def test_warmup_on_multistep(backend):
    """W = 4 over milestones (2, 3, 7): lr = val (e + 1) / 4 for the first four updates; the update again bit-equal to the by-value entry point's."""
    dev = select(backend)
    T = _Twin(dev, 0, 1029)
    sched = _block(dev, **WARMUP_MULTISTEP)
    worst = 0.0
    for call in range(1, 11):
        before = sched.cpu().numpy().copy()
        lr, clock = T.step(sched, 0.01)
        units = _lr_units(before, lr)
        worst = max(worst, units)
        assert units <= K_LR, (call, lr, C.lr64(before))
        assert clock == float(call)
        if call > 4:        # past the warm-up the value is a table entry again: exact
            assert lr == F32(F64(LR_BASE) * 0.5 ** sum(1 for b in (2, 3, 7) if b <= call - 1))
    report("optim.%s.lr_warmup_units" % backend, worst)


@pytest.mark.parametrize("kw", COSINE, ids=lambda k: "W%d-e%d" % (k["warmup"], k["clock"]))
@pytest.mark.parametrize("backend", BACKENDS)
def test_cosine_with_and_without_warmup(backend, kw):
    """T = 10, min 1e-6, the clock pre-set to 0, 5, 10 and 25 (past T: the rate stays at min); two calls each."""
    dev = select(backend)
    T = _Twin(dev, 9, 1029)
    sched = _block(dev, **kw)
    for call in (1, 2):
        before = sched.cpu().numpy().copy()
        lr, clock = T.step(sched, 0.0)
        units = report("optim.%s.lr_cosine_units.W%d.e%d" % (backend, kw["warmup"], kw["clock"] + call - 1), _lr_units(before, lr))
        assert units <= K_LR, (call, lr, C.lr64(before))
        assert clock == float(kw["clock"] + call)
    if kw["clock"] >= 10:
        assert abs(float(lr) - 1e-6) <= K_LR * U * LR_BASE


# ------------------------------------------------------------------------------------------------- EMA
def _grid(count, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-128, 129, (count,), generator=g).float() / 64.0).numpy()


@pytest.mark.parametrize("decay", (0.0, 0.5, 0.75, 1.0 - 2.0 ** -10))
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_ema_on_a_dyadic_grid_is_exact(backend, count, decay):
    """lr = 0 and wd = 0: p' == p bit for bit (asserted).  p and ema on a 2^-6 grid in [-2, 2], 1 - decay a power of two or 1: p' - ema, the
    product and the sum are all exact in float32, so ema' must equal the float64 contract bit for bit."""
    dev = select(backend)
    p, ema = _grid(count, 11), _grid(count, 12)
    _, g, m, v = _inputs(9, count)
    pd, gd, md, vd, ed = (_dev(x, dev) for x in (p, g, m, v, ema))
    sched, step = _block(dev, "constant", 0.0), torch.tensor([9.0]).to(dev)
    _ex(pd, gd, md, vd, ed, sched, step, 0.0, None, decay)
    _same("p' == p", pd, p)
    want = C.ema64(ema, p, decay)
    assert np.array_equal(want.astype(F32).astype(F64), want)
    _same("ema'", ed, want.astype(F32))
    assert float(step) == 10.0 and sched.cpu().numpy()[C.CLOCK] == 1.0
    assert L.lib().fsr_last_kernel().decode() == "adamw_ex_kernel<ema,plain,%s>" % ("x4" if count >= 4 else "x1")


EMA_DECAY, EMA_COUNT, EMA_STEPS = 0.999, 1029, 3


def _ema_start(count):
    p = _inputs(9, count)[0]
    g = torch.Generator().manual_seed(77)
    return (p + (torch.randn(count, generator=g) * 3e-4).numpy()).astype(F32)


def _ema_units(got, ema_before, p_new):
    ref = C.ema64(ema_before, p_new, EMA_DECAY)
    scale = np.abs(ema_before.astype(F64)) + np.abs(p_new.astype(F64))
    return float((np.abs(got.astype(F64) - ref) / (U * scale)).max())


@pytest.mark.parametrize("scaled", (False, True))
@pytest.mark.parametrize("backend", BACKENDS)
def test_ema_general_over_three_steps(backend, scaled):
    """decay 0.999 over 3 consecutive steps of the AdamW case: ema' within K_EMA units of the float64 contract evaluated from the ema
    before the step and the kernel's OWN float32 p'; p, m, v bit-equal to the by-value entry point's all along."""
    dev = select(backend)
    T = _Twin(dev, 9, EMA_COUNT, scaled, ema=_ema_start(EMA_COUNT))
    sched = _block(dev, "constant", 1e-4)
    worst = 0.0
    for _ in range(EMA_STEPS):
        before = T.ema.cpu().numpy().copy()
        T.step(sched, 0.01, EMA_DECAY)
        worst = max(worst, _ema_units(T.ema.cpu().numpy(), before, T.a[0].cpu().numpy()))
    report("optim.%s.ema_units.%s" % (backend, "scaled" if scaled else "plain"), worst)
    assert worst <= K_EMA, worst


# ------------------------------------------------------------------------------------------------- skipped step
@pytest.mark.parametrize("backend", BACKENDS)
def test_skipped_step_leaves_everything_bit_identical(backend):
    dev = select(backend)
    count = 1029
    p, g, m, v = _inputs(9, count)
    ema = _ema_start(count)
    pd, gd, md, vd, ed = (_dev(x, dev) for x in (p, g, m, v, ema))
    gd[3] = float("inf")
    w = C.block("multistep", 1e-4, milestones=(2, 3, 7), warmup=2, clock=4)
    w[C.LR_USED] = 7e-5
    sched, step, state = torch.from_numpy(w.copy()).to(dev), torch.tensor([9.0]).to(dev), torch.tensor([1024.0, 5.0, 1.0, 2.0]).to(dev)
    _ex(pd, gd, md, vd, ed, sched, step, 0.01, state, 0.9)
    for what, got, want in (("p", pd, p), ("m", md, m), ("v", vd, v), ("ema", ed, ema), ("schedule block", sched, w)):
        _same(what, got, want)
    _same("step counter", step, torch.tensor([9.0]))
    _same("loss-scale state", state, torch.tensor([1024.0, 5.0, 1.0, 2.0]))


# ------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals(backend):
    dev = select(backend)
    lib = L.lib()
    t = torch.zeros(64).to(dev)
    sched = _block(dev, "constant", 1e-4)
    P = t.data_ptr()

    def call(p=P, g=P, m=P, v=P, ema=None, count=64, s=sched.data_ptr(), step=P, decay=0.0):
        return lib.fsr_adamw_step_ex(p, g, m, v, ema, count, s, 0.9, 0.999, 1e-8, 0.0, step, 1.0, None, decay, ops._stream())

    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(s=None), dict(step=None), dict(count=0), dict(count=-5),
               dict(ema=P, decay=1.0), dict(ema=P, decay=-0.25), dict(ema=P, decay=float("nan"))):
        assert call(**kw) == -1, kw
        assert b"fsr_adamw_step_ex" in lib.fsr_last_error(), kw
    assert torch.equal(t.cpu(), torch.zeros(64)) and sched.cpu().numpy()[C.CLOCK] == 0.0      # nothing was launched


# ------------------------------------------------------------------------------------------------- the caps
def _restate_lr():
    return max(abs(float(C.lr32(w, e)) - C.lr64(w, e)) / (U * float(F32(LR_BASE))) for w, e in _lr_rows())


def _restate_ema():
    p, g, m, v = _inputs(9, EMA_COUNT)
    ema, worst = _ema_start(EMA_COUNT), 0.0
    for i in range(EMA_STEPS):          # p' of the case: the parameters drift by about lr per step; the restatement need not be AdamW
        p = (p - F32(1e-4) * np.sign(g) * F32(i + 1)).astype(F32)
        new = C.ema32(ema, p, EMA_DECAY)
        worst = max(worst, _ema_units(new, ema, p))
        ema = new
    return worst


@pytest.mark.parametrize("family", ("lr", "ema"))
def test_float32_restatement_is_inside_a_third_of_the_caps(family):
    """No kernel is launched: the float32 numpy restatement stays within K / 3 units on the inputs of the cases above, and K is the
    smallest power of two (>= 1) of which that is true."""
    K, worst = (K_LR, _restate_lr()) if family == "lr" else (K_EMA, _restate_ema())
    report("optim.restatement.%s.K%d" % (family, K), worst)
    assert worst <= K / 3.0, "%s: the float32 restatement reaches %.3g units, the cap is K = %d" % (family, worst, K)
    assert K == 1 or worst > K / 6.0, "%s: K = %d is not the smallest power of two (%.3g units)" % (family, K, worst)
