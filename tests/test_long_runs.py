"""Long training runs at the Trainer level: learning-rate schedules and the generator EMA under hipGraph replay,
set_lr under replay, bit-exact resume from state_N.pt, the EMA checkpoint and the untouched default path.

Trainers as tests/test_trainer.py builds them (nf 16 f32 on the host emulator, nf 32 on the MI355X; n_layers 1; VGG width_div 4 / 2;
batch 2; 16^2 -> 64^2).  Not asserted: bit equality of a graph-REPLAYED resumed run with Philox label noise -- whether captured and eager
draws consume the device generator identically has not been checked on hardware."""
import importlib
import os
import random
import shutil
import types
import warnings

import numpy as np
import pytest
import torch

from backend import L, select

GPU = pytest.mark.gpu


def ns(**k):
    return types.SimpleNamespace(**k)


def _cfg(device, cdt, nf=16, n_layers=1, **training):
    return ns(experiment=ns(name="t", seed=1234), generator=ns(n_filters=nf, n_layers=n_layers),
              discriminator=ns(n_filters=nf, n_layers=7),
              training=ns(**dict(dict(compiled=False, device=device, log_iter=1, checkpoint_iter=10 ** 9, generator_lr=1e-4,
                                      discriminator_lr=1e-4, batch_size=2, compute_dtype=cdt), **training)))


def _trainer(pkg, dev, cdt, nf=16, n_layers=1, width_div=4, **training):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        V = pkg.VGG19(compute_dtype=cdt, width_div=width_div, seed=1234)
        return pkg.Trainer(_cfg(str(dev), cdt, nf, n_layers, **training), perceptual_network=V)


def _gpu_trainer(pkg, dev, cdt, seed=21, **training):
    torch.manual_seed(seed)
    return _trainer(pkg, dev, cdt, nf=32, n_layers=1, width_div=4 if cdt == "f32" else 2, **training)      # (16-bit and x3: multiples of 32 channels)


def _batches(dev, seed, count):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).to(dev), (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).to(dev),
             [torch.rand(2, 1, 4, 4, generator=g).to(dev) for _ in range(3)]) for _ in range(count)]


def _opt_state(opt):
    out = {k: getattr(opt, k).detach().cpu().clone() for k in ("flat_param", "exp_avg", "exp_avg_sq", "step_dev")}
    if opt.ema is not None:
        out["ema"] = opt.ema.detach().cpu().clone()
    if opt.schedule is not None:
        out["clock"], out["lr_used"] = opt.schedule_clock(), opt.lr_used()
    return out


def _pt_files():
    """The checkpoint files of experiment "t" (a tensorboard writer, where installed, keeps its event files in the same directory)."""
    return sorted(f for f in os.listdir(os.path.join("runs", "t")) if f.endswith(".pt"))


def _assert_same_state(a, b, skip=()):
    assert set(a) == set(b)
    for k in a:
        if k not in skip:
            assert torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k], k


# ------------------------------------------------------------------------------------------------- schedule + EMA under replay
@GPU
@pytest.mark.parametrize("cdt", ["f32", "x3v", "f16"])
def test_graphed_replays_equal_eager_steps_with_schedule_and_ema(pkg, cdt):
    """tests/test_trainer.py::test_graphed_replays_equal_eager_steps with multistep milestones (3, 5), gamma 0.5 on both optimizers -- both
    fall inside the REPLAYED steps -- and ema_decay 0.9.  After two warm-up iterations and five replays the rate is base / 4: with the rate
    passed by value the replays would still run at the rate of the capture."""
    dev = select("hip")
    extra = dict(lr_schedule=ns(kind="multistep", milestones=[3, 5], gamma=0.5), ema_decay=0.9)
    data = _batches(dev, 5, 6)
    Te, Tg = _gpu_trainer(pkg, dev, cdt, **extra), _gpu_trainer(pkg, dev, cdt, **extra)
    assert torch.equal(Te.optim_generator.flat_param, Tg.optim_generator.flat_param)
    for T in (Te, Tg):
        T.install_schedules()
        T.optim_generator.reset_ema()
    eager_losses = []
    for lr, hr, nz in [data[0], data[0]] + data[1:]:
        eager_losses.append({k: float(v) for k, v in Te.train_step(lr, hr, nz).items()})
    Tg.capture_train_step(data[0][0], data[0][1], warmup=2, noise=data[0][2])
    graph_losses = []
    for lr, hr, nz in data[1:]:
        graph_losses.append({k: float(v) for k, v in Tg.graphed_train_step(lr, hr, nz).items()})
    torch.cuda.synchronize()
    assert graph_losses == eager_losses[2:]
    for oe, og in ((Te.optim_generator, Tg.optim_generator), (Te.optim_discriminator, Tg.optim_discriminator)):
        _assert_same_state(_opt_state(oe), _opt_state(og))
        assert og.schedule_clock() == 7 and float(og.step_dev) == 7.0
        assert og.lr_used() == float(np.float32(np.float64(1e-4) * 0.25))
    assert Tg.optim_generator.ema is not None and not torch.equal(Tg.optim_generator.ema, Tg.optim_generator.flat_param)
    if cdt in ("f16", "x3v"):
        assert Te.loss_scale_state() == Tg.loss_scale_state() and Tg.loss_scale_state()[1] == 0
    # the EMA generator reads the arena the replays wrote
    x = data[0][0]
    with torch.no_grad():
        assert torch.equal(Tg.generator_ema(x), Te.generator_ema(x))


@GPU
def test_set_lr_takes_effect_under_replay(pkg):
    """Capture, replay once, set_lr(base / 10), replay once: lr_used follows and the parameters equal an eager twin given the same rates."""
    dev = select("hip")
    extra = dict(lr_schedule=ns(kind="constant"))
    data = _batches(dev, 7, 3)
    Te, Tg = _gpu_trainer(pkg, dev, "f32", **extra), _gpu_trainer(pkg, dev, "f32", **extra)
    for T in (Te, Tg):
        T.install_schedules()
    Tg.capture_train_step(data[0][0], data[0][1], warmup=2, noise=data[0][2])
    Tg.graphed_train_step(*data[1])
    assert Tg.optim_generator.lr_used() == float(np.float32(1e-4))
    for opt in (Tg.optim_generator, Tg.optim_discriminator):
        opt.set_lr(1e-5)
    Tg.graphed_train_step(*data[2])
    for lr, hr, nz in (data[0], data[0], data[1]):
        Te.train_step(lr, hr, nz)
    for opt in (Te.optim_generator, Te.optim_discriminator):
        opt.set_lr(1e-5)
    Te.train_step(*data[2])
    torch.cuda.synchronize()
    for oe, og in ((Te.optim_generator, Tg.optim_generator), (Te.optim_discriminator, Tg.optim_discriminator)):
        assert og.lr_used() == float(np.float32(1e-5)) and og.schedule_clock() == 4
        _assert_same_state(_opt_state(oe), _opt_state(og))


# ------------------------------------------------------------------------------------------------- bit-exact resume
def _seed_all(v):
    torch.manual_seed(v)
    random.seed(v)
    np.random.seed(v % (2 ** 32))


def _loaders(pkg, dev, paths, seed, iterations):
    Deg = importlib.import_module("fast-srgan_amd.dataloader").Degradation
    ds = pkg.NumpyImagesDataset(paths, lr_image_size=16, scale_factor=4, device=dev)
    deg = lambda s: Deg(blur_prob=0.6, noise_prob=0.6, jpeg_prob=0.6, seed=s)       # noqa: E731
    return (pkg.DeviceBatchLoader(ds, 2, iterations, seed=seed, degradation=deg(seed + 1)),
            pkg.DeviceBatchLoader(ds, 2, seed=seed + 2, sequential=True, degradation=deg(seed + 3)))


def _resume_case(pkg, dev, cdt, tmp_path, monkeypatch):
    monkeypatch.setattr(pkg.Trainer, "fixed_lr_images", torch.tensor([]))
    monkeypatch.setattr(pkg.Trainer, "fixed_hr_images", torch.tensor([]))
    g = torch.Generator().manual_seed(2)
    paths = []
    for i, (h, w) in enumerate(((70, 80), (66, 91))):
        paths.append(str(tmp_path / ("img%d.npy" % i)))
        np.save(paths[-1], torch.randint(0, 256, (3, h, w), generator=g).to(torch.uint8).numpy())
    nf, wd = (16, 4) if dev.type == "cpu" else (32, 4 if cdt == "f32" else 2)
    extra = dict(hip_graph=False, iterations=4, checkpoint_iter=2, save_state=True, ema_decay=0.9,
                 lr_schedule=ns(kind="cosine", warmup=2, min_lr=1e-6))

    def final(T):
        out = {"g." + k: v for k, v in _opt_state(T.optim_generator).items()}
        out.update({"d." + k: v for k, v in _opt_state(T.optim_discriminator).items()})
        if T.loss_scale_state() is not None:
            out["loss_scale"] = T._scale_state.detach().cpu().clone()
        return out

    # run A: four iterations, checkpoints (and states) after 2 and 4
    dir_a, dir_b = tmp_path / "a", tmp_path / "b"
    os.makedirs(dir_a)
    monkeypatch.chdir(dir_a)
    _seed_all(31)
    Ta = _trainer(pkg, dev, cdt, nf=nf, width_div=wd, **extra)
    trn, val = _loaders(pkg, dev, paths, 5, 4)
    Ta.train(trn, val)
    A = final(Ta)
    assert A["g.clock"] == 4 and {"state_2.pt", "state_4.pt", "generator_ema_epoch_2.pt"} <= set(os.listdir(dir_a / "runs" / "t"))
    # run B: everything seeded differently, continues from A's state_2.pt (found by resume=auto) up to step 4
    os.makedirs(dir_b / "runs" / "t")
    shutil.copy(dir_a / "runs" / "t" / "state_2.pt", dir_b / "runs" / "t" / "state_2.pt")
    monkeypatch.chdir(dir_b)
    _seed_all(977)
    Tb = _trainer(pkg, dev, cdt, nf=nf, width_div=wd, resume="auto", **extra)
    assert not torch.equal(Tb.optim_generator.flat_param.cpu(), A["g.flat_param"])
    assert Tb.resume_file() == os.path.join("runs", "t", "state_2.pt")
    trn, val = _loaders(pkg, dev, paths, 4242, 4)
    Tb.pretrain(trn, val)                       # skipped on resume: would otherwise consume the loader
    Tb.train(trn, val)
    _assert_same_state(A, final(Tb), skip=("g.lr_used", "d.lr_used"))
    assert final(Tb)["g.lr_used"] == A["g.lr_used"]
    ema_a = torch.load(dir_a / "runs" / "t" / "generator_ema_epoch_4.pt", map_location="cpu")
    ema_b = torch.load(dir_b / "runs" / "t" / "generator_ema_epoch_4.pt", map_location="cpu")
    assert list(ema_a) == list(Ta.generator.state_dict()) == list(ema_b)
    assert all(torch.equal(ema_a[k], ema_b[k]) for k in ema_a)
    assert not os.path.exists(dir_b / "runs" / "t" / "generator_epoch_2.pt") and os.path.exists(dir_b / "runs" / "t" / "state_4.pt")
    # an explicit path works too, and a missing one is an error
    Tc = _trainer(pkg, dev, cdt, nf=nf, width_div=wd, resume=str(dir_a / "runs" / "t" / "state_4.pt"), **extra)
    assert Tc.resume_file().endswith("state_4.pt")
    with pytest.raises(FileNotFoundError):
        _trainer(pkg, dev, cdt, nf=nf, width_div=wd, resume=str(dir_a / "nothing.pt"), **extra).resume_file()


def test_bit_exact_resume_emulator_f32(pkg, tmp_path, monkeypatch):
    _resume_case(pkg, select("emu"), "f32", tmp_path, monkeypatch)


@GPU
@pytest.mark.parametrize("cdt", ["f32", "f16"])
def test_bit_exact_resume_gpu(pkg, tmp_path, monkeypatch, cdt):
    _resume_case(pkg, select("hip"), cdt, tmp_path, monkeypatch)


def test_resume_auto_without_a_state_starts_fresh_and_a_mismatched_state_is_refused(pkg, tmp_path, monkeypatch, capsys):
    dev = select("emu")
    monkeypatch.chdir(tmp_path)
    T = _trainer(pkg, dev, "f32", resume="auto", save_state=True)
    assert T.resume_file() is None and "starting fresh" in capsys.readouterr().out
    big = _trainer(pkg, dev, "f32", nf=32, save_state=True)
    big.save_checkpoints(1)
    path = os.path.join("runs", "t", "state_1.pt")
    n_big, n_small = big.optim_generator.flat_param.numel(), T.optim_generator.flat_param.numel()
    before = T.optim_generator.flat_param.clone()
    with pytest.raises(ValueError, match=r"generator arena of %d floats.*has %d" % (n_big, n_small)):
        T.load_state(path)
    assert torch.equal(T.optim_generator.flat_param, before)


# ------------------------------------------------------------------------------------------------- EMA checkpoint, defaults
def test_ema_checkpoint_loads_into_a_fresh_generator(pkg, tmp_path, monkeypatch):
    """generator_ema_epoch_N.pt has the generator's keys: loaded the way inference.load_generator loads a checkpoint, the fresh Generator's
    forward equals Trainer.generator_ema's (whose parameters are views of the optimizer's EMA arena)."""
    dev = select("emu")
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(3)
    T = _trainer(pkg, dev, "f32", ema_decay=0.9)
    opt = T.optim_generator
    assert [p.data_ptr() for p in T.generator_ema.parameters()] == [v.data_ptr() for v in opt.ema_views()]
    assert not list(T.generator_ema.buffers()) and not any(p.requires_grad for p in T.generator_ema.parameters())
    opt.flat_grad.copy_(torch.randn(opt.flat_grad.shape, generator=torch.Generator().manual_seed(1)) * 0.1)
    epoch = [p._fsr_epoch if hasattr(p, "_fsr_epoch") else 0 for p in T.generator_ema.parameters()]
    opt.step()
    assert L.lib().fsr_last_kernel().startswith(b"adamw_ex_kernel<ema,plain")
    assert all(p._fsr_epoch > e for p, e in zip(T.generator_ema.parameters(), epoch))       # cached filter packs re-pack
    assert not torch.equal(opt.ema, opt.flat_param)
    T.save_checkpoints(3)
    assert _pt_files() == sorted(["generator_epoch_3.pt", "discriminator_epoch_3.pt", "generator_optim_epoch_3.pt",
                            "discriminator_optim_epoch_3.pt", "generator_ema_epoch_3.pt"])
    inference = importlib.import_module("fast-srgan_amd.inference")
    fresh = inference.load_generator(T.config, os.path.join("runs", "t", "generator_ema_epoch_3.pt"), device=str(dev), compute_dtype="f32")
    x = torch.rand(1, 3, 16, 16, generator=torch.Generator().manual_seed(4)) * 2 - 1
    with torch.no_grad():
        got, want, raw = fresh(x), T.generator_ema(x), T.generator.eval()(x)
    assert torch.equal(got, want) and not torch.equal(got, raw)


def test_defaults_write_todays_files_and_issue_todays_launches(pkg, tmp_path, monkeypatch):
    dev = select("emu")
    monkeypatch.chdir(tmp_path)
    T = _trainer(pkg, dev, "f32")
    assert T.generator_ema is None and T.resume_file() is None
    for opt in (T.optim_generator, T.optim_discriminator):
        assert opt.schedule is None and opt._sched is None and opt.ema is None
        opt.step()
        assert L.lib().fsr_last_kernel() == b"adamw_kernel"
        assert set(opt.state_dict()) == {"state", "param_groups"}
    T.save_checkpoints(1)
    assert _pt_files() == sorted(["generator_epoch_1.pt", "discriminator_epoch_1.pt", "generator_optim_epoch_1.pt", "discriminator_optim_epoch_1.pt"])


def test_unknown_schedule_key_and_bad_values_are_refused(pkg):
    dev = select("emu")
    with pytest.raises(ValueError, match=r"unknown training.lr_schedule key\(s\) \['milestone'\]"):
        _trainer(pkg, dev, "f32", lr_schedule=ns(kind="multistep", milestone=[2]))
    with pytest.raises(ValueError, match="cosine"):
        _trainer(pkg, dev, "f32", lr_schedule=ns(kind="cosine"))                    # no training.iterations
    with pytest.raises(ValueError, match="ema_decay"):
        _trainer(pkg, dev, "f32", ema_decay=1.0)
