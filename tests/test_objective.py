"""The configurable training objective (training.loss.*): loss weights through the backward seeds, the pixel term
(ops.elem_loss on the generator's output and the HR batch), the least-squares adversarial term, the perceptual branch switched off.

The reference for every step is a torch-autograd restatement on the CPU (`restated_step`), built from the oracle's networks and
optimizer (oracle.srgan_cpu: generator_forward, discriminator_forward, vgg_forward, adamw_step) and the objective's own formulas.
Gates: losses 1e-3 relative (test_trainer.py); gradients through backend.check_grads with the f32 gates of test_modules.py
(t_tensor 1e-2, t_slope 1e-2, t_cos 0.9999) -- f16 and x3 / x3v: the train-step gates test_parity_bench.py uses for the mode.
The combined objective's weights are chosen on the reference so that each of its three terms carries at least 10 % of the norm of
the generator's gradient (asserted): a dropped or doubled term cannot pass the gradient gates."""
import importlib
import os
import types
import warnings

import pytest
import torch

from backend import BACKENDS, L, check_grads, ops, report, select
from oracle import srgan_cpu as O
from test_parity_bench import B32_X3_COS_D, B32_X3_COS_G, B32_X3_D_GRAD, B32_X3_G_GRAD, B32_X3_LOSS, B32_X3_SLOPE, CFG5_COS, CFG5_D_GRAD, \
    CFG5_G_GRAD, CFG5_LOSS, CFG5_SLOPE, STEP_NORM

trainer_mod = importlib.import_module("fast-srgan_amd.trainer")
GPU = pytest.mark.gpu
PIXEL_EPS = 1e-3
# Weights chosen on the CPU reference, per network size and adversarial term, so that each term's share of the norm of the generator's
# gradient is 0.5 .. 0.75 (the adversarial gradient per unit weight is ~40x the others' at these untrained networks, and larger with 32
# filters and with least squares); _check_step asserts the premise, >= 0.1 each
_CHARB = dict(pixel_kind="charbonnier", pixel_eps=PIXEL_EPS)
COMBINED = dict(_CHARB, adversarial=0.01, content=0.5, pixel=0.5)                       # 16 filters, BCE
COMBINED_LSGAN = dict(_CHARB, adversarial=0.004, content=0.5, pixel=0.5, gan="lsgan")   # 16 filters, least squares
COMBINED_32 = dict(_CHARB, adversarial=0.005, content=0.5, pixel=0.25)                  # 32 filters (f16), BCE
# 64 filters, 8 crops of 48x48 (x3, x3v), BCE: the adversarial share is 0.20, twice the premise's 10 % and no more -- the x3 error of a
# step enters through the discriminator branch (see test_combined_objective_16bit_and_x3_modes)
COMBINED_X3 = dict(_CHARB, adversarial=0.012, content=0.5, pixel=0.25)
SHAPE = (2, 16)             # the tiny trainer's batch: 2 crops of 16x16 -> 64x64
SHAPE_X3 = (8, 48)          # the x3 / x3v gradient case: see its docstring
SPELLED_OUT = dict(adversarial=0.05, content=0.5, pixel=0, gan="bce", pretrain_kind="smooth_l1")


def ns(**k):
    return types.SimpleNamespace(**k)


def _cfg(device, cdt, nf=16, loss=None, **training):
    t = ns(compiled=False, device=device, log_iter=1, checkpoint_iter=10 ** 9, generator_lr=1e-4, discriminator_lr=1e-4, batch_size=2,
           compute_dtype=cdt, **training)
    if loss is not None:
        t.loss = ns(**loss)
    return ns(experiment=ns(name="t", seed=1234), generator=ns(n_filters=nf, n_layers=1), discriminator=ns(n_filters=nf, n_layers=7), training=t)


def _sizes(cdt):
    """(n_filters, VGG width divisor): the tiny trainer of test_trainer.py; 16-bit and x3 tensors carry multiples of 32 channels, and
    x3 / x3v run at 64 filters, the width at which the x3 train-step gates of test_parity_bench.py were measured."""
    return {"f32": (16, 4), "f16": (32, 2)}.get(cdt, (64, 2))


def _trainer(pkg, dev, cdt, loss=None, perceptual="vgg", **training):
    nf, wd = _sizes(cdt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        V = pkg.VGG19(compute_dtype=cdt, width_div=wd, seed=1234) if perceptual == "vgg" else perceptual
        return pkg.Trainer(_cfg(str(dev), cdt, nf, loss, **training), perceptual_network=V)


def _batch(seed=3, dev=None, shape=SHAPE):
    n, s = shape
    g = torch.Generator().manual_seed(seed)
    lr, hr = torch.rand(n, 3, s, s, generator=g) * 2 - 1, torch.rand(n, 3, 4 * s, 4 * s, generator=g) * 2 - 1
    noise = [torch.rand(n, 1, s // 4, s // 4, generator=g) for _ in range(3)]
    if dev is not None:
        return lr.to(dev), hr.to(dev), [t.to(dev) for t in noise]
    return lr, hr, noise


# ------------------------------------------------------------------------------------------------- the reference
def elem64(kind, a, b, eps=PIXEL_EPS):
    d = a - b
    if kind == "l1":
        return d.abs().mean()
    if kind == "smooth_l1":
        return O.smooth_l1(a, b)
    if kind == "charbonnier":
        return (d * d + eps * eps).sqrt().mean()
    return (d * d).mean()


def restated_step(g_sd, d_sd, v_sd, lr, hr, noise, loss=None, grads_out=None, term_norms=None):
    """One iteration under training.loss = `loss` in torch autograd on the CPU: the structure of oracle.train_step (trainer.py:171-196)
    with the objective's formulas.  g_sd / d_sd are updated in place; returns the losses train_step returns."""
    obj = dict(trainer_mod._LOSS_DEFAULTS, **(loss or {}))
    gan = O.bce_with_logits if obj["gan"] == "bce" else (lambda x, t: ((x - t) ** 2).mean())
    dp = {k: v.detach().clone().requires_grad_(True) for k, v in d_sd.items()}
    with torch.no_grad():
        sr = O.generator_forward(g_sd, lr)
    loss_real = gan(O.discriminator_forward(dp, hr), 0.3 * noise[0] + 0.8)
    loss_fake = gan(O.discriminator_forward(dp, sr), 0.3 * noise[1])
    grads = torch.autograd.grad(0.5 * loss_real + 0.5 * loss_fake, list(dp.values()))
    if grads_out is not None:
        grads_out.update({"d." + k: g.detach().clone() for k, g in zip(dp, grads)})
    O.adamw_step(d_sd, dict(zip(dp, grads)), {}, lr=1e-4)
    gp = {k: v.detach().clone().requires_grad_(True) for k, v in g_sd.items()}
    sr = O.generator_forward(gp, lr)
    zero = torch.zeros(())
    terms = {}      # name -> (weight, unweighted value)
    if obj["adversarial"] > 0:
        terms["adversarial"] = (obj["adversarial"], gan(O.discriminator_forward(d_sd, sr), 0.3 * noise[2] + 0.7))
    if obj["content"] > 0:
        terms["content"] = (obj["content"], O.smooth_l1(O.vgg_forward(v_sd, sr), O.vgg_forward(v_sd, hr)))
    if obj["pixel"] > 0:
        terms["pixel"] = (obj["pixel"], elem64(obj["pixel_kind"], sr, hr, obj["pixel_eps"]))
    per_term = {k: torch.autograd.grad(w * v, list(gp.values()), retain_graph=True) for k, (w, v) in terms.items()}
    grads = [sum(gs) for gs in zip(*per_term.values())]
    if term_norms is not None:
        total = torch.cat([g.reshape(-1) for g in grads]).norm()
        term_norms.update({k: float(torch.cat([g.reshape(-1) for g in gs]).norm() / total) for k, gs in per_term.items()})
    if grads_out is not None:
        grads_out.update({"g." + k: g.detach().clone() for k, g in zip(gp, grads)})
    O.adamw_step(g_sd, dict(zip(gp, grads)), {}, lr=1e-4)
    out = {"loss_real": loss_real.detach(), "loss_fake": loss_fake.detach(),
           "adv_loss": 1e-1 * terms["adversarial"][1].detach() if "adversarial" in terms else zero,
           "content_loss": terms["content"][1].detach() if "content" in terms else zero}
    if "pixel" in terms:
        out["pixel_loss"] = terms["pixel"][1].detach()
    return out


_REFERENCE = {}


def _reference(cdt, loss_key, loss, shape=SHAPE):
    """The restated step for the trainer of `cdt` seeded with 9: computed once per (sizes, objective, batch shape) and shared, never
    modified."""
    nf, wd = _sizes(cdt)
    key = (nf, wd, loss_key, shape)
    if key not in _REFERENCE:
        pkg = importlib.import_module("fast-srgan_amd")
        torch.manual_seed(9)
        G = pkg.Generator(ns(n_filters=nf, n_layers=1), compute_dtype="f32")
        D = pkg.Discriminator(ns(n_filters=nf, n_layers=7), compute_dtype="f32")
        g_sd = {k: v.detach().clone() for k, v in G.state_dict().items()}
        d_sd = {k: v.detach().clone() for k, v in D.state_dict().items()}
        init = ({k: v.clone() for k, v in g_sd.items()}, {k: v.clone() for k, v in d_sd.items()})
        grads, norms = {}, {}
        lr, hr, noise = _batch(shape=shape)
        losses = restated_step(g_sd, d_sd, O.vgg_standin_state_dict(1234, wd), lr, hr, noise, loss, grads, norms)
        _REFERENCE[key] = dict(init=init, losses=losses, grads=grads, norms=norms, g_sd=g_sd, d_sd=d_sd)
    return _REFERENCE[key]


def _seeded_trainer(pkg, dev, cdt, loss, R, **kw):
    T = _trainer(pkg, dev, cdt, loss, **kw)
    T.generator.load_state_dict(R["init"][0])
    T.discriminator.load_state_dict(R["init"][1])
    return T


GATES = {   # mode -> (loss gate, [(which gradients, check_grads gates)]), laid out as the cited tests lay them out
    "f32": (1e-3, [("d", dict(t_tensor=1e-2, t_slope=1e-2, t_cos=0.9999)), ("g", dict(t_tensor=1e-2, t_slope=1e-2, t_cos=0.9999))]),
    # test_parity_bench.py, f16 train steps: D and G tensors, slopes and norm ratios each, the cosine over both networks together
    "f16": (CFG5_LOSS, [("d", dict(t_tensor=CFG5_D_GRAD, t_slope=CFG5_SLOPE, t_norm=STEP_NORM)),
                        ("g", dict(t_tensor=CFG5_G_GRAD, t_slope=CFG5_SLOPE, t_norm=STEP_NORM)),
                        ("dg", dict(t_tensor=CFG5_G_GRAD, t_slope=CFG5_SLOPE, t_cos=CFG5_COS))]),
    # test_parity_bench.py, x3 / x3v train steps: a cosine per network
    "x3": (B32_X3_LOSS, [("d", dict(t_tensor=B32_X3_D_GRAD, t_slope=B32_X3_SLOPE, t_cos=B32_X3_COS_D, t_norm=STEP_NORM)),
                         ("g", dict(t_tensor=B32_X3_G_GRAD, t_slope=B32_X3_SLOPE, t_cos=B32_X3_COS_G, t_norm=STEP_NORM))]),
}
GATES["x3v"] = GATES["x3"]


def _check_step(tag, pkg, dev, cdt, loss_key, loss, shape=SHAPE, **kw):
    """One train_step of the seeded trainer against the shared restatement: the returned key set, every loss, and the gradients the
    step left in .grad (divided by the loss scale), through check_grads."""
    R = _reference(cdt, loss_key, loss, shape)
    if loss_key.startswith("combined"):
        for k, share in R["norms"].items():
            report("objective.premise.%s.share.%s" % (tag, k), share)
        assert set(R["norms"]) == {"adversarial", "content", "pixel"} and min(R["norms"].values()) >= 0.1, \
            "premise: every term carries at least 10 %% of the generator gradient's norm, got %s" % (R["norms"],)
    T = _seeded_trainer(pkg, dev, cdt, loss, R, **kw)
    scale = T.loss_scale_state()[0] if T.loss_scale_state() is not None else T.loss_scale
    got = T.train_step(*_batch(dev=dev, shape=shape))
    assert set(got) == set(R["losses"]), (sorted(got), sorted(R["losses"]))
    loss_gate, grad_gates = GATES[cdt]
    for k, want in R["losses"].items():
        if float(want) == 0.0:
            assert float(got[k]) == 0.0, (k, float(got[k]))
            continue
        e = report("objective.%s.%s.%s" % (tag, dev.type, k), abs(float(got[k]) - float(want)) / abs(float(want)))
        print("objective %s %s: %s got %.9g want %.9g (rel %.3g, gate %g)" % (tag, dev.type, k, float(got[k]), float(want), e, loss_gate))
        assert e <= loss_gate, (k, float(got[k]), float(want))
    if T.loss_scale_state() is not None:
        assert T.loss_scale_state() == (scale, 0), "premise: no overflow, the gradients carry the scale the step began with"
    named = {"d": [("d." + k, p.grad / scale) for k, p in T.discriminator.named_parameters()],
             "g": [("g." + k, p.grad / scale) for k, p in T.generator.named_parameters()]}
    bad = []
    for which, gates in grad_gates:
        bad += check_grads("objective.%s.%s.grad.%s" % (tag, dev.type, which), sum((named[n] for n in which), []), R["grads"], **gates)
    assert not bad, bad
    return T, got


# ------------------------------------------------------------------------------------------------- emulator and GPU, f32
@pytest.mark.parametrize("backend", BACKENDS)
def test_spelled_out_defaults_equal_no_loss_node(pkg, backend):
    """training.loss with the defaults spelled out == no training.loss at all: torch.equal losses and parameters after a train step
    and after a pretrain step."""
    dev = select(backend)
    R = _reference("f32", "default", None)
    Ta, Tb = _seeded_trainer(pkg, dev, "f32", None, R), _seeded_trainer(pkg, dev, "f32", SPELLED_OUT, R)
    assert Ta.objective == Tb.objective and not Ta._objective_given and Tb._objective_given
    lr, hr, noise = _batch(dev=dev)
    for step in ("train", "pretrain"):
        if step == "train":
            la, lb = Ta.train_step(lr, hr, noise), Tb.train_step(lr, hr, noise)
            assert list(la) == list(lb) == ["loss_real", "loss_fake", "adv_loss", "content_loss"]
            assert all(torch.equal(la[k], lb[k]) for k in la), (step, la, lb)
        else:
            assert torch.equal(Ta.pretrain_step(lr, hr), Tb.pretrain_step(lr, hr))
        for oa, ob in ((Ta.optim_generator, Tb.optim_generator), (Ta.optim_discriminator, Tb.optim_discriminator)):
            assert torch.equal(oa.flat_param, ob.flat_param) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq), step


@pytest.mark.parametrize("backend", BACKENDS)
def test_combined_objective_vs_restatement(pkg, backend):
    """All three weights positive, a Charbonnier pixel term: losses and both networks' gradients against the restatement."""
    dev = select(backend)
    _check_step("combined.f32", pkg, dev, "f32", "combined", COMBINED)


@pytest.mark.parametrize("backend", BACKENDS)
def test_lsgan_objective_vs_restatement(pkg, backend):
    """The same step with gan=lsgan: least squares on the logits in all three places, same labels, same 0.5 / 0.5."""
    dev = select(backend)
    _check_step("lsgan.f32", pkg, dev, "f32", "combined_lsgan", COMBINED_LSGAN)
    R = _reference("f32", "combined_lsgan", COMBINED_LSGAN)
    assert abs(float(R["losses"]["loss_real"]) - float(_reference("f32", "combined", COMBINED)["losses"]["loss_real"])) > 1e-2, \
        "premise: the least-squares and the BCE discriminator losses differ"


@pytest.mark.parametrize("backend", BACKENDS)
def test_pretrain_kind_l1_vs_torch(pkg, backend):
    """pretrain_kind=l1: one pretrain step against torch.nn.L1Loss on the oracle's generator (the 1e-4 gate of
    test_pretrain_step_vs_oracle), parameters moved like the reference's."""
    dev = select(backend)
    R = _reference("f32", "default", None)
    T = _seeded_trainer(pkg, dev, "f32", dict(pretrain_kind="l1"), R)
    lr, hr, _ = _batch()
    got = T.pretrain_step(lr.to(dev), hr.to(dev))
    g_sd = {k: v.clone() for k, v in R["init"][0].items()}
    gp = {k: v.clone().requires_grad_(True) for k, v in g_sd.items()}
    want = torch.nn.L1Loss()(O.generator_forward(gp, lr), hr)
    O.adamw_step(g_sd, dict(zip(gp, torch.autograd.grad(want, list(gp.values())))), {}, lr=1e-4)
    want = want.detach()
    assert abs(float(got) - float(want)) <= 1e-4 * abs(float(want)), (float(got), float(want))
    assert abs(float(want) - float(O.smooth_l1(O.generator_forward(R["init"][0], lr), hr))) > 1e-2, "premise: L1 and smooth-L1 differ here"
    for k, p in T.generator.state_dict().items():
        assert (p.cpu() - g_sd[k]).abs().mean() <= 0.1 * 1e-4 + 1e-9, k


CONTENT_OFF = dict(adversarial=0.05, content=0, pixel=1.0, pixel_kind="l1")


class _NeverCalled(torch.nn.Module):
    def forward(self, *a, **k):
        raise AssertionError("the perceptual network was called although training.loss.content is 0")

    features_nhwc = forward


@pytest.mark.parametrize("backend", BACKENDS)
def test_content_off_never_touches_the_perceptual_network(pkg, backend, monkeypatch):
    """content=0: a perceptual network that raises when called is never called, Trainer(config) builds without constructing one (no
    VGG weights needed), content_loss is an exact 0 and the step matches the restatement."""
    dev = select(backend)
    T, got = _check_step("content_off.f32", pkg, dev, "f32", "content_off", CONTENT_OFF, perceptual=_NeverCalled())
    assert float(got["content_loss"]) == 0.0 and float(got["pixel_loss"]) > 0.0 and not T._streams
    monkeypatch.setattr(trainer_mod, "VGG19", lambda *a, **k: (_ for _ in ()).throw(AssertionError("VGG19 constructed")))
    T2 = pkg.Trainer(_cfg(str(dev), "f32", 16, CONTENT_OFF))
    assert T2.perceptual_network is None
    out = T2.train_step(*_batch(dev=dev))
    assert float(out["content_loss"]) == 0.0
    with pytest.raises(AssertionError, match="VGG19 constructed"):      # premise: the default objective does build one
        pkg.Trainer(_cfg(str(dev), "f32", 16))


# ------------------------------------------------------------------------------------------------- GPU only
@GPU
@pytest.mark.parametrize("cdt", ["f16", "x3", "x3v"])
def test_combined_objective_16bit_and_x3_modes(pkg, cdt):
    """The combined step in f16 (dynamic loss scale: the pixel seed follows it), x3 and x3v, at the mode's train-step gates.

    f16 runs the tiny trainer's batch at 32 filters.  x3 and x3v run 64 filters on 8 crops of 48x48 with an adversarial share of 0.20,
    for a reason that has nothing to do with the objective: test_parity_bench.py's x3 gates were measured at 32 crops of 96x96, and
    the PReLU-slope gate among them (0.02 of the largest slope gradient) is not one the x3 mode meets on a handful of pixels -- with
    the DEFAULT objective, the path of before, the MI355X gives 0.081 at 2 crops of 16x16, 0.034 at 4 of 32x32, 0.028 at 8 of 48x48 and
    0.023 at 8 of 64x64 (D cosine 0.99998 / 0.99992 / 0.99996 / 0.99998 against 0.9999).  That error comes in through the
    discriminator branch (x3 products flip LeakyReLU decisions there, test_modules.py) and is proportional to the adversarial term's
    share of the generator gradient: at 8 x 48x48, shares of 0.09 / 0.20 / 0.26 / 0.32 / 0.52 (the default) give 0.004 / 0.010 /
    0.014 / 0.017 / 0.028.  So the case takes 8 crops of 48x48 and an adversarial share of twice the premise's 10 %: large enough
    that such a share sits at half the slope gate, small enough for a test.  The reference step takes 2 to 4 s, once for both modes.
    Measured there: losses <= 1.8e-5 (gate 1e-3), D tensors <= 0.014 (0.04), G tensors <= 0.10 (0.25), slopes <= 0.010 / 0.011
    (0.02), cosines D 0.99996 (0.9999), G 0.9997 (0.99).  f16: losses <= 8.5e-4 (2e-3), D / G tensors <= 0.15 / 0.26 (0.5 / 0.75),
    slopes <= 0.034 (0.2), cosine over both networks 0.9954 (0.98)."""
    dev = select("hip")
    if cdt == "f16":
        T, _ = _check_step("combined.f16", pkg, dev, cdt, "combined", COMBINED_32)
    else:
        T, _ = _check_step("combined.%s" % cdt, pkg, dev, cdt, "combined_x3", COMBINED_X3, shape=SHAPE_X3)
    assert (T.loss_scale_state() is not None) == (cdt in ("f16", "x3v"))


def _replay_equals_eager(pkg, cdt, loss, perceptual="vgg"):
    dev = select("hip")

    def batches(seed, count):
        g = torch.Generator().manual_seed(seed)
        return [((torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).to(dev), (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).to(dev),
                 [torch.rand(2, 1, 4, 4, generator=g).to(dev) for _ in range(3)]) for _ in range(count)]

    data = batches(5, 5)
    torch.manual_seed(21)
    Te = _trainer(pkg, dev, cdt, loss, perceptual)
    torch.manual_seed(21)
    Tg = _trainer(pkg, dev, cdt, loss, perceptual)
    assert torch.equal(Te.optim_generator.flat_param, Tg.optim_generator.flat_param)
    # eager: the capture's two warm-up iterations see batch 0 twice, then batches 1..4
    eager = [{k: float(v) for k, v in Te.train_step(lr, hr, nz).items()} for lr, hr, nz in [data[0], data[0]] + data[1:]]
    Tg.capture_train_step(data[0][0], data[0][1], warmup=2, noise=data[0][2])
    graph = [{k: float(v) for k, v in Tg.graphed_train_step(lr, hr, nz).items()} for lr, hr, nz in data[1:]]
    torch.cuda.synchronize()
    assert graph == eager[2:]
    assert len({tuple(sorted(d.items())) for d in graph}) == len(graph)         # new batches, new weights: new losses
    for oe, og in ((Te.optim_generator, Tg.optim_generator), (Te.optim_discriminator, Tg.optim_discriminator)):
        assert torch.equal(oe.flat_param, og.flat_param) and torch.equal(oe.exp_avg_sq, og.exp_avg_sq)
        assert float(oe.step_dev) == float(og.step_dev) == 6.0
    if Te.loss_scale_state() is not None:
        assert Te.loss_scale_state() == Tg.loss_scale_state() and Tg.loss_scale_state()[1] == 0
    return graph


@GPU
@pytest.mark.parametrize("cdt", ["f32", "f16", "x3v"])
def test_graphed_replays_equal_eager_steps_with_the_combined_objective(pkg, cdt):
    """N replays of the captured iteration == N eager train_steps, bit for bit, with the pixel node and three seeds in the graph (the
    f16 and x3v seeds are products with the device-side loss scale, made inside the captured graph)."""
    graph = _replay_equals_eager(pkg, cdt, COMBINED_LSGAN if cdt == "f32" else COMBINED_32)   # (bit equality: any weights do)
    assert all(set(g) == {"loss_real", "loss_fake", "adv_loss", "content_loss", "pixel_loss"} for g in graph)


@GPU
def test_content_off_captured_form_replays(pkg):
    """content=0 under capture: no side stream is forked, every phase ends joined, and the replays equal the eager steps."""
    graph = _replay_equals_eager(pkg, "x3v", CONTENT_OFF, perceptual=_NeverCalled())
    assert all(g["content_loss"] == 0.0 and g["pixel_loss"] > 0.0 for g in graph)


# ------------------------------------------------------------------------------------------------- host logic, no device
def test_objective_settings_are_validated(pkg):
    select("emu")
    with pytest.raises(ValueError, match=r"unknown training\.loss key.*colour.*known: adversarial, content, pixel, pixel_kind, pixel_eps, gan, pretrain_kind"):
        pkg.Trainer(_cfg("cpu", "f32", 16, dict(colour=1.0)), perceptual_network=_NeverCalled())
    for bad in (dict(pixel=-1.0), dict(adversarial=float("nan")), dict(content=float("inf")), dict(content=-0.5),
                dict(adversarial=0, content=0, pixel=0), dict(adversarial=0.0, content=0.0),
                dict(pixel_kind="huber"), dict(gan="ragan"), dict(pretrain_kind="bce"), dict(pixel_eps=0.0), dict(pixel_eps=float("nan")),
                dict(pixel="much")):
        with pytest.raises(ValueError, match=r"training\.loss"):
            pkg.Trainer(_cfg("cpu", "f32", 16, bad), perceptual_network=_NeverCalled())
    T = pkg.Trainer(_cfg("cpu", "f32", 16, dict(content=0, pixel=1.0)), perceptual_network=None)     # weights of 0 are fine while one is left
    assert T.objective == dict(trainer_mod._LOSS_DEFAULTS, content=0.0, pixel=1.0) and T.perceptual_network is None
    cfg = pkg.load_config(None, ["training.loss.pixel=0.01", "training.loss.pixel_kind=charbonnier", "training.loss.gan=lsgan"])
    assert vars(cfg.training.loss) == {"pixel": 0.01, "pixel_kind": "charbonnier", "gan": "lsgan"}
    assert trainer_mod._objective_settings(cfg)[0] == dict(trainer_mod._LOSS_DEFAULTS, pixel=0.01, pixel_kind="charbonnier", gan="lsgan")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert not hasattr(pkg.load_config(os.path.join(root, "configs", "config.yaml")).training, "loss")      # override-only keys


def test_returned_keys_with_and_without_a_pixel_weight(pkg):
    """The four keys of the reference, plus pixel_loss exactly when its weight is positive; Trainer.train logs it.  (One 8x8 sample:
    this is about the keys.)"""
    dev = select("emu")
    g = torch.Generator().manual_seed(4)
    lr, hr = torch.rand(1, 3, 8, 8, generator=g) * 2 - 1, torch.rand(1, 3, 32, 32, generator=g) * 2 - 1
    noise = [torch.rand(1, 1, 2, 2, generator=g) for _ in range(3)]
    base = ["loss_real", "loss_fake", "adv_loss", "content_loss"]
    for loss, keys in ((dict(pixel=0.0), base), (dict(adversarial=0, pixel=0.5), base + ["pixel_loss"])):
        T = _trainer(pkg, dev, "f32", loss)
        out = T.train_step(lr, hr, noise)
        assert list(out) == keys, (loss, list(out))
    assert float(out["adv_loss"]) == 0.0 and float(out["pixel_loss"]) > 0.0       # adversarial=0: D(sr) is not evaluated for G at all
    # Trainer.train's logging: Loss/Generator/Pixel beside the four others (one eager iteration, metrics and images stubbed out)
    T.writer = trainer_mod._NullWriter()
    T._calculate_metrics_over_dataset = lambda *a, **k: None
    saved, trainer_mod.Trainer.fixed_lr_images = trainer_mod.Trainer.fixed_lr_images, torch.zeros(1, 1)
    try:
        T.train([(lr, hr)], [])
    finally:
        trainer_mod.Trainer.fixed_lr_images = saved
    assert {"Loss/Generator/Pixel", "Loss/Generator/Content", "Loss/Generator/Adversarial"} <= set(T.writer.scalars)


def _load_quietly(T, path):
    """load_state's return value, with no warning about the objective raised."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        step = T.load_state(path)
    assert not [w for w in caught if "objective" in str(w.message)], [str(w.message) for w in caught]
    return step


def test_state_file_records_the_objective_and_warns_on_a_mismatch(pkg, tmp_path, monkeypatch):
    dev = select("emu")
    monkeypatch.chdir(tmp_path)
    loss = dict(pixel=0.01, pixel_kind="charbonnier")
    T = _trainer(pkg, dev, "f32", loss, save_state=True)
    T.save_checkpoints(7)
    path = os.path.join("runs", "t", "state_7.pt")
    assert torch.load(path)["objective"] == dict(trainer_mod._LOSS_DEFAULTS, pixel=0.01, pixel_kind="charbonnier")
    assert _load_quietly(_trainer(pkg, dev, "f32", loss), path) == 7       # the same objective: silent
    with pytest.warns(UserWarning, match=r"another training objective.*pixel: 0\.01 -> 0\.0"):
        assert _trainer(pkg, dev, "f32").load_state(path) == 7
    with pytest.warns(UserWarning, match=r"gan: 'bce' -> 'lsgan'"):
        _trainer(pkg, dev, "f32", dict(loss, gan="lsgan")).load_state(path)
    # a default run's file has no entry, loads as before, and a configured objective is told apart from it
    T0 = _trainer(pkg, dev, "f32", save_state=True)
    T0.save_checkpoints(8)
    path0 = os.path.join("runs", "t", "state_8.pt")
    assert "objective" not in torch.load(path0)
    assert _load_quietly(_trainer(pkg, dev, "f32"), path0) == 8
    assert _load_quietly(_trainer(pkg, dev, "f32", SPELLED_OUT), path0) == 8
    with pytest.warns(UserWarning, match="another training objective"):
        _trainer(pkg, dev, "f32", loss).load_state(path0)
