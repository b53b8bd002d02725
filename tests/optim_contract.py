"""Test helper: the schedule and EMA contract of fsr_adamw_step_ex (include/fsr_hip.h) restated in numpy,
independently of the code under test, and the fixtures test_optim_ex.py / test_optim_schedule.py / test_long_runs.py share.

The block: 32 floats -- [0] kind (0 constant, 1 multistep, 2 cosine), [1] base lr, [2] warm-up length W, [3] cosine length T, [4] min lr,
[5] number of boundaries nb, [6] lr_used, [7] clock e, [8..15] boundaries, [16..24] nb + 1 values.
The update applied at clock e (updates applied BEFORE it) runs at
    constant / multistep:  val = values[#{boundaries <= e}]
    cosine:                val = min + 0.5 (base - min) (1 + cos(pi min(e, T) / T))
    lr = val (e + 1) / W while e < W, else val
and the average moves by ema' = ema + (p' - ema) (1 - decay)."""
import numpy as np

F32, F64 = np.float32, np.float64
WORDS, KIND, BASE, WARMUP, TOTAL, MIN, NB, LR_USED, CLOCK, BOUNDS, VALUES, MAX_BOUNDARIES = 32, 0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 8
KINDS = {"constant": 0, "multistep": 1, "cosine": 2}
U = 2.0 ** -23


def block(kind, base, warmup=0, milestones=(), gamma=0.5, total=0, min_lr=0.0, clock=0, poison=False):
    """The float32 block the host writes: values base gamma^k computed in float64 and cast.  poison: NaN behind the nb boundaries and
    the nb + 1 values (the slots the kernel must not read)."""
    w = np.zeros(WORDS, F32)
    if poison:
        w[BOUNDS:VALUES + MAX_BOUNDARIES + 1] = np.nan
    nb = len(milestones) if kind == "multistep" else 0
    w[KIND], w[BASE], w[WARMUP], w[TOTAL], w[MIN], w[NB], w[CLOCK] = KINDS[kind], base, warmup, total, min_lr, nb, clock
    w[BOUNDS:BOUNDS + nb] = np.asarray(milestones[:nb], F64)
    w[VALUES:VALUES + nb + 1] = [F64(base) * F64(gamma) ** k for k in range(nb + 1)]
    return w


def lr64(w, e=None):
    """The contract in float64 from the float32 words of a block (e: the clock, default the block's own)."""
    w = np.asarray(w, F32).astype(F64)
    e = w[CLOCK] if e is None else F64(e)
    if w[KIND] == 2:
        val = w[MIN] + 0.5 * (w[BASE] - w[MIN]) * (1.0 + np.cos(np.pi * min(e, w[TOTAL]) / w[TOTAL]))
    else:
        nb = int(w[NB])
        val = w[VALUES + int(np.sum(w[BOUNDS:BOUNDS + nb] <= e))]
    return float(val * ((e + 1.0) / w[WARMUP]) if e < w[WARMUP] else val)


def lr32(w, e=None):
    """The kernel's statements in float32 numpy: one rounding per operation, no fused multiply-add, numpy's float32 cosine."""
    w = np.asarray(w, F32)
    e = w[CLOCK] if e is None else F32(e)
    one, half = F32(1), F32(0.5)
    if w[KIND] == 2:
        arg = F32(np.pi) * min(e, w[TOTAL]) / w[TOTAL]
        val = w[MIN] + half * (w[BASE] - w[MIN]) * (one + np.cos(arg, dtype=F32))
    else:
        nb = int(w[NB])
        val = w[VALUES + int(np.sum(w[BOUNDS:BOUNDS + nb] <= e))]
    return F32(val * ((e + one) / w[WARMUP])) if e < w[WARMUP] else F32(val)


def ema64(ema, p_new, decay):
    """ema + (p' - ema) (1 - decay) in float64 from float32 operands (decay as the float32 the kernel is handed)."""
    ema, p_new = np.asarray(ema, F32).astype(F64), np.asarray(p_new, F32).astype(F64)
    return ema + (p_new - ema) * (1.0 - F64(F32(decay)))


def ema32(ema, p_new, decay):
    ema, p_new = np.asarray(ema, F32), np.asarray(p_new, F32)
    return ema + (p_new - ema) * (F32(1) - F32(decay))


def adam_inputs(step0, count, seed=6):
    """As tests/test_stream_exact.py builds them: p ~ 1e-3 randn, g ~ 0.1 randn with every fifth exactly zero; fresh moments at step 0,
    else m ~ 0.05 randn and v in [1e-4, 1e-2]."""
    import torch
    g = torch.Generator().manual_seed(seed + step0)
    p, gr = (torch.randn(count, generator=g) * 1e-3).numpy(), (torch.randn(count, generator=g) * 0.1).numpy()
    gr[(np.arange(count) + 2) % 5 == 0] = 0.0
    if step0 == 0:
        m, v = np.zeros(count, F32), np.zeros(count, F32)
    else:
        m, v = (torch.randn(count, generator=g) * 0.05).numpy(), ((torch.rand(count, generator=g) + 0.01) * 0.01).numpy()
    return p, gr, m, v
