"""The AdamW entry points against bits recorded on the MI355X from the two scalar kernels they used to have.

tests/test_optim_ex.py compares the block-rate entry point with the by-value entry points, which are instantiations of one kernel
template: it checks the rate plumbing, and cannot see a change that moves all of them together.  tests/golden/adamw_bits.npz
(tests/golden/make_adamw_bits.py) holds p, g, m, v of optim_contract.adam_inputs and p', m', v' and the step counter after THREE
consecutive calls of fsr_adamw_step / fsr_adamw_step_scaled, recorded from a library built before the kernels were merged, for every
combination of

    count   1, 3, 5 (the scalar tail alone, one vector + tails), 1025 (256 vectors + 1, a second workgroup)
    step0   0, 9, 999                      weight decay   0, 0.01
    plain / scaled (loss scale 1024, gradients pre-scaled)        16-byte aligned / one float off (the scalar path)

Every bit must be equal, through the by-value entry points and through fsr_adamw_step_ex with a constant schedule at the same rate.
A differing bit is a kernel bug: fsr_adamw.h names every rounding so that this holds.  MI355X only: the emulator's host build of
fsr_adamw_update uses the plain expressions and was never bit-equal to the device."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import optim_contract as C
from backend import L, ops, select

F32 = np.float32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adamw_bits.npz")
COUNTS, STEP0S, WDS = (1, 3, 5, 1025), (0, 9, 999), (0.0, 0.01)
CASES = list(itertools.product(COUNTS, STEP0S, WDS, (False, True), (0, 1)))     # count, step0, wd, scaled, offset
LR, B1, B2, EPS, GSCALE, LOSS_SCALE, CALLS = 1e-4, 0.9, 0.999, 1e-8, 0.5, 1024.0, 3


def in_key(count, step0):
    return "in_c%d_t%d_" % (count, step0)


def out_key(count, step0, wd, scaled, offset):
    return "out_c%d_t%d_wd%d_%s_o%d_" % (count, step0, int(wd != 0.0), "scaled" if scaled else "plain", offset)


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


def replay(dev, inputs, wd, scaled, offset, entry):
    """CALLS consecutive steps from `inputs` = (p, g, m, v, step0); entry "value": fsr_adamw_step / _scaled at LR, "block":
    fsr_adamw_step_ex with a constant schedule at LR.  Returns p', m', v' and the step counter as CPU tensors."""
    p, g, m, v, step0 = inputs
    lib = L.lib()
    gd = _dev(g * F32(LOSS_SCALE) if scaled else g, dev, offset)
    pd, md, vd = (_dev(x, dev, offset) for x in (p, m, v))
    assert all(t.data_ptr() % 16 == 4 * offset for t in (pd, gd, md, vd))
    step = torch.tensor([float(step0)]).to(dev)
    state = torch.tensor([LOSS_SCALE, 0.0, 0.0, 0.0]).to(dev) if scaled else None
    sched = torch.from_numpy(C.block("constant", LR)).to(dev)
    arena = (pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr())
    for _ in range(CALLS):
        if entry == "block":
            L.check(lib.fsr_adamw_step_ex(*arena, None, pd.numel(), sched.data_ptr(), B1, B2, EPS, wd, step.data_ptr(), GSCALE,
                                          None if state is None else state.data_ptr(), 0.0, ops._stream()), "fsr_adamw_step_ex")
        elif scaled:
            L.check(lib.fsr_adamw_step_scaled(*arena, pd.numel(), LR, B1, B2, EPS, wd, step.data_ptr(), GSCALE, state.data_ptr(),
                                              ops._stream()), "fsr_adamw_step_scaled")
        else:
            L.check(lib.fsr_adamw_step(*arena, pd.numel(), LR, B1, B2, EPS, wd, step.data_ptr(), GSCALE, ops._stream()), "fsr_adamw_step")
    return pd.cpu(), md.cpu(), vd.cpu(), step.cpu()


@functools.lru_cache(maxsize=1)
def _fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("count,step0,wd,scaled,offset", CASES,
                         ids=["c%d-t%d-wd%g-%s-o%d" % (c, t, w, "scaled" if s else "plain", o) for c, t, w, s, o in CASES])
@pytest.mark.parametrize("entry", ("value", "block"))
def test_three_steps_equal_the_recorded_bits(entry, count, step0, wd, scaled, offset):
    dev = select("hip")
    fx = _fixture()
    inputs = tuple(fx[in_key(count, step0) + k] for k in "pgmv") + (step0,)
    got = replay(dev, inputs, wd, scaled, offset, entry)
    for name, t in zip(("p", "m", "v", "step"), got):
        _same("%s after %d calls" % (name, CALLS), t, fx[out_key(count, step0, wd, scaled, offset) + name])
    assert float(got[3]) == step0 + CALLS
