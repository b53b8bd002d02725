"""Host side of the long-run support: LRSchedule against torch's schedulers, the block layout, the validation errors,
the optimizer's and the loader's state round trips (kernels on the host emulator; nothing here needs a GPU).

LRSchedule.lr_at(e) is the rate of the update applied at clock e (e updates before it).  torch's schedulers say the same thing as
"param_groups[0]['lr'] after e calls of scheduler.step()": MultiStepLR and CosineAnnealingLR agree with the contract to rounding.  The
warm-up val (e + 1) / W is LinearLR(start_factor=1 / W, total_iters=W - 1) chained in front.  Where torch and the contract differ, the
contract wins:
  * chained with CosineAnnealingLR and eta_min > 0, torch applies both schedulers' RECURSIVE forms, so the warm-up factor scales
    lr - eta_min and eta_min differently from step to step; the contract scales the whole cosine value.  With eta_min = 0 both are the
    same product, which is what is compared; the eta_min > 0 case is compared with the formula itself;
  * past T_max torch's cosine comes back up (it is periodic), the contract stays at min_lr: compared up to T_max only, asserted beyond;
  * LinearLR needs total_iters >= 1, so W = 1 (a factor of 1 at e = 0: no warm-up at all) has no torch counterpart.
"""
import math
import warnings

import numpy as np
import pytest
import torch

import optim_contract as C
from backend import L, select

STEPS = 40


def _torch_rates(make, base=1e-3, steps=STEPS):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base)
    sched = make(opt)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(steps):
            out.append(opt.param_groups[0]["lr"])
            p.grad = torch.zeros(1)
            opt.step()
            sched.step()
    return out


def _chain(opt, W, then):
    S = torch.optim.lr_scheduler
    return S.ChainedScheduler([S.LinearLR(opt, start_factor=1.0 / W, total_iters=W - 1), then(opt)])


def _assert_rates(schedule, want):
    got = [schedule.lr_at(e) for e in range(len(want))]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("W", (0, 2, 5))
def test_multistep_against_torch(pkg, W):
    S = torch.optim.lr_scheduler
    ms = lambda o: S.MultiStepLR(o, milestones=[3, 10, 11, 30], gamma=0.3)      # noqa: E731
    want = _torch_rates(ms if W == 0 else (lambda o: _chain(o, W, ms)))
    _assert_rates(pkg.LRSchedule("multistep", base_lr=1e-3, milestones=(3, 10, 11, 30), gamma=0.3, warmup=W), want)


@pytest.mark.parametrize("W,eta_min", [(0, 0.0), (0, 1e-5), (4, 0.0)])
def test_cosine_against_torch(pkg, W, eta_min):
    S = torch.optim.lr_scheduler
    cos = lambda o: S.CosineAnnealingLR(o, T_max=STEPS, eta_min=eta_min)        # noqa: E731
    want = _torch_rates(cos if W == 0 else (lambda o: _chain(o, W, cos)))
    sch = pkg.LRSchedule("cosine", base_lr=1e-3, total=STEPS, min_lr=eta_min, warmup=W)
    _assert_rates(sch, want)
    assert sch.lr_at(STEPS) == pytest.approx(eta_min, abs=1e-18) and sch.lr_at(3 * STEPS) == sch.lr_at(STEPS)


def test_cosine_warmup_with_a_floor_follows_the_contract(pkg):
    """The case torch's chaining computes differently (module docstring): the contract's formula, and the device block's restatement."""
    sch = pkg.LRSchedule("cosine", base_lr=1e-3, total=20, min_lr=1e-5, warmup=4)
    w = sch.words().numpy()
    for e in range(30):
        val = 1e-5 + 0.5 * (1e-3 - 1e-5) * (1.0 + math.cos(math.pi * min(e, 20) / 20))
        assert sch.lr_at(e) == pytest.approx(val * (e + 1) / 4 if e < 4 else val, rel=1e-14)
        assert C.lr64(w, e) == pytest.approx(sch.lr_at(e), rel=2e-7)        # the block holds float32 words


def test_constant_and_ema_only(pkg):
    sch = pkg.LRSchedule(base_lr=2e-4)
    assert [sch.lr_at(e) for e in (0, 1, 10 ** 6)] == [2e-4] * 3
    assert pkg.LRSchedule(base_lr=2e-4, warmup=2).lr_at(0) == 1e-4


def test_words_layout(pkg):
    sch = pkg.LRSchedule("multistep", base_lr=1e-4, warmup=3, milestones=(2, 3, 7), gamma=0.5, min_lr=1e-6)
    w = sch.words()
    assert w.dtype == torch.float32 and w.shape == (32,)
    assert np.array_equal(w.numpy(), C.block("multistep", 1e-4, warmup=3, milestones=(2, 3, 7), gamma=0.5, min_lr=1e-6))
    assert w[C.VALUES + 3] == np.float32(np.float64(1e-4) * 0.5 ** 3) and float(w[C.NB]) == 3 and not w[C.VALUES + 4:].any()
    w = pkg.LRSchedule("cosine", base_lr=1e-4, total=1000, min_lr=1e-6, milestones=(5,)).words()
    assert np.array_equal(w.numpy(), C.block("cosine", 1e-4, total=1000, min_lr=1e-6))      # milestones belong to multistep only
    w = pkg.LRSchedule("multistep", base_lr=1.0, milestones=tuple(range(1, 9)), gamma=0.1).words()
    assert float(w[C.NB]) == 8 and w[C.VALUES + 8] == np.float32(1e-8) and not w[C.VALUES + 9:].any()


@pytest.mark.parametrize("kw", [dict(kind="linear"), dict(kind="multistep", milestones=tuple(range(1, 10))), dict(kind="multistep", milestones=(3, 3)),
                                dict(kind="multistep", milestones=(5, 2)), dict(kind="multistep", milestones=(0, 2)),
                                dict(kind="multistep", milestones=(1.5,)), dict(gamma=0.0), dict(gamma=1.5), dict(kind="cosine"),
                                dict(kind="cosine", total=0), dict(min_lr=-1e-6), dict(min_lr=1.0), dict(warmup=-1), dict(warmup=1.5)],
                         ids=lambda k: ",".join("%s=%s" % kv for kv in k.items()))
def test_validation_errors(pkg, kw):
    with pytest.raises(ValueError, match="LRSchedule"):
        pkg.LRSchedule(**dict(dict(base_lr=1e-3), **kw))


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(5, 4, 3, 3, generator=g)), torch.nn.Parameter(torch.randn(7, generator=g)),
            torch.nn.Parameter(torch.randn(1, generator=g))]


def _run(opt, ps, steps, seed):
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        opt.zero_grad()
        for p in ps:
            p.grad.add_(torch.randn(p.shape, generator=g))
        opt.step()


def test_arena_adamw_defaults_allocate_nothing_and_use_the_old_entry_points(pkg):
    select("emu")
    ps = _params(0)
    opt = pkg.ArenaAdamW(ps, lr=1e-3)
    assert opt.schedule is None and opt._sched is None and opt.ema is None
    _run(opt, ps, 1, 1)
    assert L.lib().fsr_last_kernel() == b"adamw_kernel"
    opt.scale_state = torch.tensor([1024.0, 0.0, 0.0, 0.0])
    _run(opt, ps, 1, 1)
    assert L.lib().fsr_last_kernel() == b"adamw_scaled_kernel"
    assert set(opt.state_dict()) == {"state", "param_groups", "fsr_loss_scale_state"}
    with pytest.raises(L.FsrError):
        opt.lr_used()
    with pytest.raises(L.FsrError):
        opt.ema_views()


def test_schedule_and_ema_follow_torch_and_the_contract(pkg):
    """ArenaAdamW(schedule, ema_decay) on the emulator against torch.optim.AdamW + MultiStepLR and a float64 EMA of torch's parameters."""
    select("emu")
    ps, ref = _params(0), _params(0)
    opt = pkg.ArenaAdamW(ps, lr=1e-3, schedule=pkg.LRSchedule("multistep", base_lr=1e-3, milestones=(2, 3), gamma=0.5), ema_decay=0.9)
    ropt = torch.optim.AdamW(ref, lr=1e-3)
    rsch = torch.optim.lr_scheduler.MultiStepLR(ropt, [2, 3], 0.5)
    ema = [r.detach().double().clone() for r in ref]
    g = torch.Generator().manual_seed(4)
    for it in range(5):
        opt.zero_grad()
        for p, r in zip(ps, ref):
            gr = torch.randn(p.shape, generator=g)
            p.grad.add_(gr)
            r.grad = gr.clone()
        opt.step()
        assert L.lib().fsr_last_kernel() == b"adamw_ex_kernel<ema,plain,x4>"
        assert opt.lr_used() == np.float32(ropt.param_groups[0]["lr"]) and opt.schedule_clock() == it + 1
        ropt.step()
        rsch.step()
        ema = [e + (r.detach().double() - e) * (1.0 - float(np.float32(0.9))) for e, r in zip(ema, ref)]
    for p, r, e, v in zip(ps, ref, ema, opt.ema_views()):
        assert (p.detach() - r.detach()).abs().max() < 1e-6
        assert v.shape == p.shape and (v.double() - e).abs().max() < 1e-6
    opt.reset_ema()
    assert torch.equal(opt.ema, opt.flat_param)


def test_set_lr_rewrites_a_constant_schedule_only(pkg):
    select("emu")
    ps = _params(0)
    opt = pkg.ArenaAdamW(ps, lr=1e-3, ema_decay=0.5)          # ema_decay alone: a constant schedule at lr
    assert opt.schedule.kind == "constant" and opt.schedule.base_lr == 1e-3
    _run(opt, ps, 2, 1)
    opt.set_lr(1e-5)
    _run(opt, ps, 1, 2)
    assert opt.lr_used() == np.float32(1e-5) and opt.schedule_clock() == 3 and opt.param_groups[0]["lr"] == 1e-5
    assert np.array_equal(opt._sched.numpy()[[C.BASE, C.VALUES]], np.float32([1e-5, 1e-5]))
    opt.set_schedule(pkg.LRSchedule("cosine", base_lr=1e-3, total=10))
    assert opt.schedule_clock() == 0
    with pytest.raises(L.FsrError, match="cosine"):
        opt.set_lr(1e-4)


def test_state_dict_round_trip_restores_schedule_clock_and_ema_bit_for_bit(pkg):
    select("emu")
    sch = lambda: pkg.LRSchedule("cosine", base_lr=1e-3, total=9, min_lr=1e-5, warmup=2)       # noqa: E731
    pa, pb, pc = _params(0), _params(0), _params(5)
    A = pkg.ArenaAdamW(pa, lr=1e-3, schedule=sch(), ema_decay=0.75)
    B = pkg.ArenaAdamW(pb, lr=1e-3, schedule=sch(), ema_decay=0.75)
    _run(A, pa, 5, 1)
    _run(B, pb, 3, 1)
    sd = B.state_dict()
    assert sd["fsr_schedule"] == dict(kind="cosine", base_lr=1e-3, warmup=2, milestones=[], gamma=0.5, total=9, min_lr=1e-5, clock=3)
    assert sd["fsr_ema"].device.type == "cpu" and sd["fsr_ema"].shape == (B.flat_param.numel(),)
    # a reference-format loader takes the dict, extra keys and all
    ref = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in pb], lr=1e-3)
    ref.load_state_dict(sd)
    assert torch.equal(ref.state_dict()["state"][0]["exp_avg"], sd["state"][0]["exp_avg"])
    # a fresh optimizer built WITHOUT a schedule (other parameters, another rate) continues the run bit for bit
    Cc = pkg.ArenaAdamW(pc, lr=5e-2, ema_decay=0.75)
    Cc.flat_param.copy_(B.flat_param)
    Cc.load_state_dict(sd)
    assert Cc.schedule_clock() == 3 and Cc.schedule.args() == B.schedule.args() and torch.equal(Cc.ema, B.ema)
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        for p in pa:
            torch.randn(p.shape, generator=g)        # skip the three steps B already took
    for opt, ps in ((Cc, pc),):
        for _ in range(2):
            opt.zero_grad()
            for p in ps:
                p.grad.add_(torch.randn(p.shape, generator=g))
            opt.step()
    for name in ("flat_param", "exp_avg", "exp_avg_sq", "ema", "step_dev", "_sched"):
        assert torch.equal(getattr(Cc, name), getattr(A, name)), name
    short = pkg.ArenaAdamW(_params(0)[:2], lr=1e-3, ema_decay=0.75)
    with pytest.raises(L.FsrError, match="%d floats.*%d" % (B.ema.numel(), short.ema.numel())):
        short.load_state_dict(dict(sd, state={}))


def test_device_batch_loader_state_round_trip(pkg, tmp_path):
    """5 batches straight == 2 batches, state saved, a FRESH loader (another seed) restored, 3 batches -- degradation draws included."""
    dev = select("emu")
    g = torch.Generator().manual_seed(8)
    paths = []
    for i, (h, w) in enumerate(((40, 44), (37, 52))):
        paths.append(str(tmp_path / ("img%d.npy" % i)))
        np.save(paths[-1], torch.randint(0, 256, (3, h, w), generator=g).to(torch.uint8).numpy())
    ds = pkg.NumpyImagesDataset(paths, lr_image_size=8, scale_factor=4, device=dev)
    Deg = importlib_dataloader().Degradation

    def loader(seed, dseed):
        return pkg.DeviceBatchLoader(ds, 2, iterations=5, seed=seed, degradation=Deg(blur_prob=0.7, noise_prob=0.7, jpeg_prob=0.7, seed=dseed))

    straight = [tuple(t.clone() for t in b) for b in loader(3, 4)]
    first = loader(3, 4)
    head, it = [], iter(first)
    for _ in range(2):
        head.append(tuple(t.clone() for t in next(it)))
    state = first.state_dict()
    assert state["yielded"] == 2 and state["degradation"] is not None
    fresh = loader(99, 98)
    fresh.load_state_dict(state)
    tail = [tuple(t.clone() for t in b) for b in fresh]
    assert len(straight) == 5 and len(tail) == 3
    for a, b in zip(straight, head + tail):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert len(list(fresh)) == 5                                # the restored pass has ended; a new one starts over
    plain = pkg.DeviceBatchLoader(ds, 2, iterations=5, seed=3)
    with pytest.raises(ValueError, match="degradation"):
        plain.load_state_dict(state)


def importlib_dataloader():
    import importlib
    return importlib.import_module("fast-srgan_amd.dataloader")
