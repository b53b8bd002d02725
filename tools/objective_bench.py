"""What the configurable training objective costs on the device.

    python tools/objective_bench.py [--batch 32] [--rounds 15] [--inner 10] [--dtypes f16,x3v] [--out profiles/objective_bench.txt]

At bench.py's workload (8 residual blocks, 64 filters, 96 -> 384, batch 32, random weights, synthetic batch), one captured iteration
per candidate, replayed as a hipGraph:
  (a) the default objective (no training.loss node: the path bench.py times);
  (b) training.loss.pixel=0.01 (ESRGAN's weight; L1);
  (c) training.loss.content=0 training.loss.pixel=1 (a PSNR-oriented fine-tune: no perceptual branch).
The candidates are INTERLEAVED: every round times each of them once, in turn (device events around `inner` replays), so clock and
thermal drift fall on all of them alike; the figure is the median over the rounds, the spread the 10th to 90th percentile.
Then the two new kernels alone, at the tensors of the pixel term -- the generator's output as the (N,3,H,W) view of an NHWC buffer
against a planar batch -- in us and TB/s of the bytes the algorithm needs (forward: two reads; backward: two reads and a write),
beside fsr_smooth_l1_fwd / _bwd on contiguous copies of the same tensors.  (b) - (a) is printed against the sum of the two kernels'
own times.  Nothing is gated on any of it."""
import argparse
import importlib
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("fast-srgan_amd")
ops = importlib.import_module("fast-srgan_amd.ops")
L = importlib.import_module("fast-srgan_amd._lib")
ns = types.SimpleNamespace

CANDIDATES = (("(a) default objective", None),
              ("(b) pixel=0.01", dict(pixel=0.01)),
              ("(c) content=0 pixel=1", dict(content=0, pixel=1.0)))


def make_trainer(batch, dtype, device, loss):
    t = ns(compiled=False, device=device, log_iter=10 ** 9, checkpoint_iter=10 ** 9, generator_lr=1e-4, discriminator_lr=1e-4,
           batch_size=batch, compute_dtype=dtype)
    if loss is not None:
        t.loss = ns(**loss)
    cfg = ns(experiment=ns(name="objective_bench", seed=1234), generator=ns(n_filters=64, n_layers=8, n_upsample=2),
             discriminator=ns(n_filters=64, n_layers=7), training=t)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(1234)
        V = pkg.VGG19(compute_dtype=dtype, seed=1234) if (loss or {}).get("content", 0.5) > 0 else None
        return pkg.Trainer(cfg, perceptual_network=V)


def timed(cands, rounds, inner):
    """us per call of every (name, fn), interleaved round by round."""
    for _, fn in cands:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in cands]
    for _ in range(rounds):
        for k, (_, fn) in enumerate(cands):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / inner)
    return times


def row(label, t, extra=""):
    return "%-44s %10.1f [%9.1f .. %9.1f]%s" % (label, np.median(t), np.percentile(t, 10), np.percentile(t, 90), extra)


def kernels_alone(batch, size, device, rounds, inner):
    """The element-wise kernels on the pixel term's tensors: (label, times, bytes) rows."""
    lib = L.lib()
    g = torch.Generator().manual_seed(0)
    sr = (torch.rand(batch, size, size, 3, generator=g) * 2 - 1).to(device).permute(0, 3, 1, 2)       # NCHW view of an NHWC buffer
    hr = (torch.rand(batch, 3, size, size, generator=g) * 2 - 1).to(device)                            # planar
    sr_c, da_c = sr.contiguous(), torch.empty_like(hr)
    da = torch.empty_strided(sr.shape, sr.stride(), dtype=torch.float32, device=device)
    loss, gs = torch.zeros(1, device=device), torch.ones(1, device=device)
    scr = ops._workspace(max(lib.fsr_elem_loss_scratch(), lib.fsr_loss_scratch()), device)
    count, st = sr.numel(), ops._stream()

    def fwd(code):
        return lambda: L.check(lib.fsr_elem_loss_fwd(code, 1e-3, sr.data_ptr(), *sr.stride(), hr.data_ptr(), *hr.stride(), *sr.shape,
                                                     loss.data_ptr(), scr.data_ptr(), st), "fsr_elem_loss_fwd")

    def bwd(code):
        return lambda: L.check(lib.fsr_elem_loss_bwd(code, 1e-3, sr.data_ptr(), *sr.stride(), hr.data_ptr(), *hr.stride(), gs.data_ptr(),
                                                     da.data_ptr(), *sr.shape, st), "fsr_elem_loss_bwd")

    cands = []
    for name, code in (("l1", L.LOSS_L1), ("charbonnier", L.LOSS_CHARBONNIER), ("mse", L.LOSS_MSE), ("smooth_l1", L.LOSS_SMOOTH_L1)):
        cands.append(("fsr_elem_loss_fwd %s (NHWC view vs planar)" % name, fwd(code), 2))
        cands.append(("fsr_elem_loss_bwd %s (NHWC view vs planar)" % name, bwd(code), 3))
    cands.append(("fsr_smooth_l1_fwd (contiguous copies)", lambda: L.check(lib.fsr_smooth_l1_fwd(
        L.FSR_F32, sr_c.data_ptr(), hr.data_ptr(), loss.data_ptr(), scr.data_ptr(), count, st), "fsr_smooth_l1_fwd"), 2))
    cands.append(("fsr_smooth_l1_bwd (contiguous copies)", lambda: L.check(lib.fsr_smooth_l1_bwd(
        L.FSR_F32, sr_c.data_ptr(), hr.data_ptr(), gs.data_ptr(), da_c.data_ptr(), count, st), "fsr_smooth_l1_bwd"), 3))
    cands.append(("  sr.contiguous() (what SmoothL1Fn pays first)", lambda: sr.contiguous(), 2))
    times = timed([(n, f) for n, f, _ in cands], rounds, inner)
    return [(n, t, passes * count * 4) for (n, _, passes), t in zip(cands, times)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lr", type=int, default=96, help="LR crop edge (HR = 4x)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="replays per timed interval")
    ap.add_argument("--dtypes", default="f16,x3v")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objective_bench.txt"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("objective_bench: needs the GPU (no fallback, nothing is measured without one)")
    dev = "cuda:0"
    lines = ["# tools/objective_bench.py --batch %d --lr %d --rounds %d --inner %d on %s" % (a.batch, a.lr, a.rounds, a.inner, torch.cuda.get_device_name(0)),
             "# us per call: median over the rounds [p10 .. p90]; candidates interleaved round by round",
             "# training step: 8 blocks / 64 filters, %d -> %d, batch %d, one hipGraph replay per step" % (a.lr, 4 * a.lr, a.batch)]
    g = torch.Generator().manual_seed(1)
    lr = (torch.rand(a.batch, 3, a.lr, a.lr, generator=g) * 2 - 1).to(dev)
    hr = (torch.rand(a.batch, 3, 4 * a.lr, 4 * a.lr, generator=g) * 2 - 1).to(dev)
    kern = kernels_alone(a.batch, 4 * a.lr, torch.device(dev), a.rounds, 50)
    by_name = {n: float(np.median(t)) for n, t, _ in kern}
    pair = by_name["fsr_elem_loss_fwd l1 (NHWC view vs planar)"] + by_name["fsr_elem_loss_bwd l1 (NHWC view vs planar)"]
    for dtype in a.dtypes.split(","):
        trainers = [make_trainer(a.batch, dtype, dev, loss) for _, loss in CANDIDATES]
        for T in trainers:
            T.capture_train_step(lr, hr)
        cands = [(name, (lambda T=T: T.graphed_train_step(lr, hr))) for (name, _), T in zip(CANDIDATES, trainers)]
        times = timed(cands, a.rounds, a.inner)
        med = [float(np.median(t)) for t in times]
        for (name, _), t in zip(cands, times):
            lines.append(row("%-5s %s" % (dtype, name), t, "   %8.2f img/s" % (a.batch / (np.median(t) * 1e-6))))
        lines.append("%-44s %10.1f   (the two L1 kernels alone: %.1f us)" % ("%-5s (b) - (a)" % dtype, med[1] - med[0], pair))
        lines.append("%-44s %10.3f" % ("%-5s (c) / (a)" % dtype, med[2] / med[0]))
        del trainers, cands
        torch.cuda.empty_cache()
    lines.append("# the kernels alone, float32 [%d,3,%d,%d]: us per launch and TB/s of the bytes the algorithm needs" % (a.batch, 4 * a.lr, 4 * a.lr))
    for name, t, nbytes in kern:
        lines.append(row(name, t, "   %6.2f TB/s" % (nbytes / (np.median(t) * 1e-6) / 1e12)))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
