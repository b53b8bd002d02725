"""Device time of the AdamW step with and without the device-side schedule and the fused EMA.

    python tools/optim_bench.py [--rounds 30] [--inner 10] [--against OTHER/libfsr_hip.so] [--out profiles/optim_bench.txt]

At the generator's and the discriminator's real arena sizes (read from freshly built default networks): fsr_adamw_step (the rate by
value, what every default run calls: the yardstick), fsr_adamw_step_scaled (the same under the fp16 loss scale), fsr_adamw_step_ex with
a constant schedule (the same kernel with the rate read from the block), that through pointers one float off their allocations (the
scalar path), and with the EMA.  Each from its own device events around --inner calls.  The candidates
are INTERLEAVED: every round times each of them once, in turn, so clock and thermal drift fall on all of them alike; the figure is the
median over the rounds, the spread the 10th to 90th percentile.  --against: the two by-value legs of another build of the library
(an A/B of the default path's launches) join the same rounds.  Nothing is gated on it."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = importlib.import_module("fast-srgan_amd._lib")
ops = importlib.import_module("fast-srgan_amd.ops")
optim = importlib.import_module("fast-srgan_amd.optim")
model = importlib.import_module("fast-srgan_amd.model")
config = importlib.import_module("fast-srgan_amd.config")

HP = (0.9, 0.999, 1e-8, 0.01)


def arena_sizes():
    cfg = config.load_config(None)
    g = model.Generator(config=cfg.generator, compute_dtype="f32")
    d = model.Discriminator(config=cfg.discriminator, compute_dtype="f32")
    return [("generator", sum(p.numel() for p in g.parameters())), ("discriminator", sum(p.numel() for p in d.parameters()))]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed interval")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.txt"))
    ap.add_argument("--against", default=None, help="another build of libfsr_hip.so: its by-value legs are interleaved with this build's")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    lib = L.lib()
    other = L._bind(a.against) if a.against else None
    lines = ["# tools/optim_bench.py --rounds %d --inner %d on %s" % (a.rounds, a.inner, torch.cuda.get_device_name(0)),
             "# us per call: median over the rounds [p10 .. p90]; candidates interleaved round by round; MB = bytes read + written; each call",
             "# includes its one-thread tick launch",
             "%-14s %10s %-38s %9s %19s %8s %8s" % ("arena", "floats", "call", "us", "[p10 .. p90]", "MB", "GB/s")]
    for name, n in arena_sizes():
        gen = torch.Generator().manual_seed(0)
        buf = {k: torch.zeros(n + 1, device=dev) for k in "pgmve"}
        buf["p"][:] = (torch.randn(n + 1, generator=gen) * 1e-2).to(dev)
        buf["g"][:] = (torch.randn(n + 1, generator=gen) * 1e-2).to(dev)
        buf["e"].copy_(buf["p"])
        step = torch.zeros(1, device=dev)
        sched = optim.LRSchedule("constant", base_lr=1e-4).words().to(dev)

        state = torch.tensor([1024.0, 0.0, 0.0, 0.0], device=dev)

        def by_value(scaled=False, lib=lib):
            p, g, m, v = (buf[k][:n].data_ptr() for k in "pgmv")
            if scaled:
                L.check(lib.fsr_adamw_step_scaled(p, g, m, v, n, 1e-4, *HP, step.data_ptr(), 1.0, state.data_ptr(), ops._stream()),
                        "fsr_adamw_step_scaled")
            else:
                L.check(lib.fsr_adamw_step(p, g, m, v, n, 1e-4, *HP, step.data_ptr(), 1.0, ops._stream()), "fsr_adamw_step")

        def ex(off=0, ema=False):
            p, g, m, v, e = (buf[k][off:off + n].data_ptr() for k in "pgmve")
            L.check(lib.fsr_adamw_step_ex(p, g, m, v, e if ema else None, n, sched.data_ptr(), *HP, step.data_ptr(), 1.0, None, 0.999,
                                          ops._stream()), "fsr_adamw_step_ex")

        cands = [("fsr_adamw_step", by_value, 28), ("fsr_adamw_step_scaled", lambda: by_value(True), 28),
                 ("fsr_adamw_step_ex constant, x4", ex, 28), ("fsr_adamw_step_ex constant, x1", lambda: ex(1), 28),
                 ("fsr_adamw_step_ex constant + EMA, x4", lambda: ex(0, True), 36)]
        if other is not None:
            cands += [("--against: fsr_adamw_step", lambda: by_value(False, other), 28),
                      ("--against: fsr_adamw_step_scaled", lambda: by_value(True, other), 28)]
        for _, fn, _ in cands:                          # warm-up: code objects
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in cands]
        for _ in range(a.rounds):
            for k, (_, fn, _) in enumerate(cands):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.inner)
        for (call, _, bpe), t in zip(cands, times):
            med = float(np.median(t))
            lines.append("%-14s %10d %-38s %9.2f [%7.2f .. %7.2f] %8.2f %8.0f" % (name, n, call, med, np.percentile(t, 10), np.percentile(t, 90),
                                                                                 bpe * n / 1e6, bpe * n / 1e3 / med))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
