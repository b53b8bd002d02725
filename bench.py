"""Benchmark of the Fast-SRGAN hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is one full GAN training iteration (/root/reference/trainer.py:171-196: D step + G step with the VGG
perceptual loss and both AdamW updates) over one synthetic batch that is already resident in HBM
(BASELINE.json configs[2]: 8 residual blocks / 64 filters, batch 32 per GPU, 96x96 -> 384x384, random-init weights,
kaiming-normal VGG19 stand-in).  `value` is timed in the x3v mode -- Generator and Discriminator in x3 (split-bf16 operands, three
bf16 MFMAs per product, f32 accumulation), the FROZEN perceptual network in fp16: the FASTEST mode whose outputs and four losses sit
inside north_star's 1e-3 relative fp32 tolerance (round-5 verdict, item 1b) --; pure x3, the 16-bit modes
(`--dtype f16` / `bf16`) and exact f32 are labelled legs.  N > 1 shards by batch (weak scaling): one process per GPU, two RCCL
gradient all-reduces per step; `python bench.py --gpus N` without a launcher re-executes itself under torch.distributed.run.

A plain run measures the headline only: it sets up, warms up, times --steps steps, writes --dump-outputs if given and prints the
result line (the contract keys, `config`, `timed_region_s`).  --full adds everything else below -- the sustained leg, the all-reduce
cost, the rooflines (instrumented iterations of their own), the other compute modes, cfg5, inference, the data pipeline, the CPU
baseline -- and bench_detail.json; the --no-* switches leave single legs out of a --full run.

--dump-outputs DIR writes what the timed path computed in its last timed step, as float32 DIR/<name>.npy: the four losses it returned
(loss_real, loss_fake, adv_loss, content_loss) and the weights its two AdamW updates left (generator.npy, discriminator.npy: every
floating-point state_dict tensor, flattened, in state_dict order; 22 MB for cfg3).  Weights, inputs and label noise are seeded, so
runs with the same arguments compute from the same numbers.

Rank 0 prints ONE LEAN JSON line on stdout (lean_line(): 3 KB, hard limit 6 KB -- a consumer may keep only the last 8 KB of stdout,
and round 5's 25 KB line did not parse there); with --full it also writes the FULL object to bench_detail.json (--detail PATH; the
default is given in --help).  The --full line carries the contract keys, the dominant kernel's `roofline` (with `traffic`),
`cpu_baseline`, and one scalar per leg.

Keys of the full object (bench_detail.json; DESIGN.md section 4 describes each):
  roofline      the DOMINANT kernel of the iteration (the kernel symbol with the largest share of its time): algorithmic FLOPs per
                launch / its average launch duration from HIP events on the launch stream of an instrumented single-stream step,
                against the dense MFMA peak of ITS arithmetic (kernel_peak: x3 launches 2500 / 3, fp16 / bf16 2500, f32 157.3 TFLOP/s);
                `traffic` = HBM bytes per launch of that kernel from the rocprofv3 PMC passes recorded in
                profiles/conv_traffic[_x3|_x3v].json (null when that file does not belong to the kernel sources being run);
                `family` = ALL conv forward + data-gradient launches together; `kernels` = every configuration against both roofs;
  x3_mode, f16_mode, bf16_mode, f32_mode
                the same iteration in the other compute modes, each with the SAME --steps / --warmup and its own `roofline`;
  sustained     >= --sustained-seconds of back-to-back steps of the headline mode with the shader clock sampled from sysfs;
  cpu_baseline  the oracle's CPU restatement of the same iteration AND of generator inference at 90x160 / 180x320 (BASELINE.md
                section 3), on FSR_CPU_THREADS (default 16: the fastest of profiles/r06_cpu_threads.txt) host threads (N=1, rank 0);
  cfg5          (default N = 1 run) BASELINE configs[4]: 12 residual blocks, three pixel-shuffle stages, 128x128 -> 1024x1024, fp16
                MFMA with the dynamic loss scale, batch 4 on this GPU, >= 100 steps and >= 3 s of hipGraph replays, its own roofline;
  allreduce     (a process group exists) ms per step the main stream spends in the two RCCL gradient exchanges, per exchange and
                as the maximum over ranks;
  inference     generator-only FPS at 90x160 and 180x320 (BASELINE.json configs[1]), batch 1 and batch 32, every leg >=
                --inference-seconds with the clock sampled, in the headline's generator mode (x3) and under `modes` in fp16, bf16 and
                exact f32, each with the `roofline` of its forward's dominant kernel; plus the end-to-end rate of the uint8 frame
                pipeline in fp16 (host bytes -> H2D -> G -> uint8 epilogue -> D2H): median of three warm passes.
"""
import argparse
import contextlib
import hashlib
import importlib
import json
import os
import socket
import subprocess
import sys
import time
import types
import warnings

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "f16": 2500.0, "f32": 157.3,   # /opt/skills/guides/MI355X_MICROARCH.md, dense
                    "x3": 2500.0 / 3}   # x3: three bf16 MFMAs per algorithmic MAC (hi*hi + lo*hi + hi*lo): the bf16 peak over 3


def kernel_peak(kernel_name, mode):
    """MFMA peak of ONE kernel launch: by the arithmetic its name carries (fsr_last_kernel: "<x3,...>", "<f16,...>", ...) -- the x3v
    mode mixes x3 launches (Generator, Discriminator) with fp16 ones (VGG19) --, else by the mode."""
    for dt in ("x3", "f16", "bf16", "f32"):
        if "<%s," % dt in kernel_name or "<%s>" % dt in kernel_name or ",%s>" % dt in kernel_name:
            return MFMA_PEAK_TFLOPS[dt]
    return MFMA_PEAK_TFLOPS[{"x3v": "x3"}.get(mode, mode)]
HBM_PEAK_GBS = 8000.0    # same guide: HBM3E ~8 TB/s
NOMINAL_SCLK_MHZ = 2400.0   # the boost clock MI355X's dense peaks are quoted at
LDS_FED_CEILING_TFLOPS = {"bf16": 1740.0, "f16": 1740.0}   # measured: profiles/r03_ubench_lds_mfma32.txt (32x32x16, 4+2 reads per 8 MFMAs, 8 waves per CU)
STEP_GFLOP_PER_IMAGE = 686.71                         # BASELINE.md section 2, as the REFERENCE graph executes it
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "conv_traffic.json")            # bf16; the x3 passes: conv_traffic_x3.json


MODE_DESCRIBED = {
    "x3v": "x3v (Generator and Discriminator in x3 -- split bf16, three bf16 MFMAs per product --, the frozen VGG19 perceptual network in fp16 "
           "under the dynamic loss scale)",
    "x3": "x3 (split bf16: hi + lo 16-bit planes, x_hi*w_hi + x_lo*w_hi + x_hi*w_lo on v_mfma_f32_32x32x16_bf16, f32 accumulate)",
    "f16": "f16 (v_mfma_f32_32x32x16_f16, f32 accumulate, device-side dynamic loss scale: the default 16-bit training mode)",
    "bf16": "bf16 (v_mfma_f32_32x32x16_bf16; rounds 1-4 timed `value` in this mode)",
    "f32": "f32 (v_mfma_f32_16x16x4_f32, exact fmaf chains)"}
MODE_MEETS = {
    "x3v": "all four losses within 1e-3 relative fp32 (content loss, the one quantity the fp16 network produces: 1.9e-4; the others as "
           "x3) and every generator output as x3 (the generator IS x3); parameter gradients at pure x3's distance from float64; the perceptual "
           "gradient itself is fp16-quality (11.8 % rel-L2 from fp32's, x3: 0.45 %) (tests/test_parity_bench.py [x3v] / [f16] cases, DESIGN.md 2c)",
    "x3": "forward outputs and all four losses within 1e-3 relative fp32 (measured 0 .. 7e-5: tests/test_x3.py, tests/test_parity_bench.py "
          "[x3] cases); parameter gradients are NOT at the f32 mode's gates: vs float64 the G network sits at 1.3x, the D network at "
          "2.8x the float32 oracle's own distance (DESIGN.md 2b)",
    "f16": "no: outside 1e-3 (gradients 0.15-0.5 rel-L2 per tensor); held to the operator-level and convergence gates (tests/test_convergence.py)",
    "bf16": "no: outside 1e-3 (content loss 1.7e-3, SR max |error| 3.3e-2); held to the operator-level and convergence gates like fp16",
    "f32": "1e-3 relative fp32, outputs, losses AND gradients (tests/test_parity_bench.py, tests/test_trainer.py)"}
PRECISION_NOTE = {
    "x3v": "`value` is timed in the x3v mode: Generator and Discriminator in x3 (split-bf16 operands, three bf16 MFMAs per product), the "
           "FROZEN perceptual network in fp16 -- the fastest mode whose outputs and four losses all meet north_star's 1e-3 relative "
           "fp32 (content loss 1.9e-4, others <= 2e-5). legs.x3 = every network in x3; legs.f16 / legs.bf16 are outside the tolerance; "
           "legs.f32 is exact-f32 MFMA",
    "x3": "`value` is timed in the x3 mode: the FASTEST mode whose outputs and losses meet north_star's 1e-3 relative fp32 "
          "(split-bf16 operands, three bf16 MFMAs per product, f32 accumulate; roofline peak = 2500/3 TFLOP/s). "
          "legs.f16 / legs.bf16 are 16-bit modes outside the tolerance; legs.f32 is exact-f32 MFMA",
    "f16": "`value` is timed in fp16 (outside north_star's 1e-3: a labelled 16-bit run; x3 is the credited mode)",
    "bf16": "`value` is timed in bf16 (outside north_star's 1e-3: a labelled 16-bit run; x3 is the credited mode)",
    "f32": "`value` is timed in exact-f32 MFMA (the reference's own arithmetic)"}


def ns(**k):
    return types.SimpleNamespace(**k)


WORKLOADS = {
    # BASELINE.json configs[2] (and [3] per GPU): the headline metric
    "cfg3": dict(n_layers=8, n_upsample=2, lr=96, batch=32, gflop_ref=686.71, dtype="x3v",
                 name="BASELINE configs[2]: full GAN training step, 8 residual blocks / 64 filters, 96x96->384x384",
                 metric="SR train-step images/sec (96->384 4x, full GAN step: G+D+VGG perceptual loss)"),
    # BASELINE.json configs[4]: 12 blocks, three pixel-shuffle stages, 128 -> 1024, fp16 MFMA (the dtype that config names)
    "cfg5": dict(n_layers=12, n_upsample=3, lr=128, batch=4, gflop_ref=None, dtype="f16",
                 name="BASELINE configs[4]: full GAN training step, 12 residual blocks / 64 filters, three pixel-shuffle stages, 128x128->1024x1024",
                 metric="SR train-step images/sec (128->1024 8x, full GAN step: G+D+VGG perceptual loss)"),
}


def make_config(batch, dtype, device, wl=None):
    wl = wl or WORKLOADS["cfg3"]
    return ns(experiment=ns(name="bench", seed=1234), generator=ns(n_filters=64, n_layers=wl["n_layers"], n_upsample=wl["n_upsample"]),
              discriminator=ns(n_filters=64, n_layers=7),
              training=ns(compiled=False, device=device, log_iter=10 ** 9, checkpoint_iter=10 ** 9, generator_lr=1e-4,
                          discriminator_lr=1e-4, batch_size=batch, compute_dtype=dtype))


def kernel_sources_hash():
    """sha256 over the kernel sources: ties profiles/conv_traffic.json (PMC passes) to the code being benchmarked."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "fast-srgan_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


class ClockSampler:
    """Samples the shader clock of one GPU from sysfs (pp_dpm_sclk: the line marked '*') on a background thread.
    The card is found by the HIP device's PCI address; returns None fields when sysfs is not readable."""

    def __init__(self, device_index, period=0.02):
        import glob
        import threading
        self.path = None
        self.samples = []
        self.period = period
        self._stop = threading.Event()
        self._thread = None
        try:
            pr = torch.cuda.get_device_properties(device_index)
            want = "%04x:%02x:%02x" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
            for f in glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"):
                if want in os.path.realpath(os.path.dirname(f)):
                    self.path = f
                    break
        except Exception:  # noqa: BLE001 -- the clock is a report, never a requirement
            self.path = None

    def _read(self):
        try:
            for line in open(self.path).read().splitlines():
                if line.rstrip().endswith("*"):
                    return float(line.split(":")[1].lower().replace("mhz", "").replace("*", "").strip())
        except (OSError, ValueError, IndexError):
            return None
        return None

    def __enter__(self):
        import threading
        if self.path is not None:
            def loop():
                while not self._stop.is_set():
                    v = self._read()
                    if v is not None:
                        self.samples.append(v)
                    self._stop.wait(self.period)
            self._thread = threading.Thread(target=loop, daemon=True)
            self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        if self._thread is not None:
            self._thread.join()
        return False

    def summary(self):
        if not self.samples:
            return {"sclk_mhz_mean": None, "source": "pp_dpm_sclk not readable for this GPU"}
        xs = self.samples
        return {"sclk_mhz_mean": round(sum(xs) / len(xs), 1), "sclk_mhz_min": min(xs), "sclk_mhz_max": max(xs), "samples": len(xs),
                "source": self.path}


def conv_profile(ops, fn):
    """Runs fn() with every convolution launch bracketed by HIP events on the launch stream.
    Returns the records (ms, flops, algorithmic bytes, kernel name, kind)."""
    rec = []
    ops.PROFILE_CONV = rec
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ops.PROFILE_CONV = None
    return [(r[0].elapsed_time(r[1]), r[2], r[3], r[4], r[5]) for r in rec]


def cpu_baseline():
    """The oracle (CPU restatement of trainer.py:171-196, fp32, torch CPU kernels) on a bounded sample of the same
    workload: full-size networks, 96 -> 384, batch 4 (BASELINE configs[0]), 1 warm-up + 3 timed iterations."""
    from oracle import srgan_cpu as O
    pkg = importlib.import_module("fast-srgan_amd")
    torch.manual_seed(0)
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    # thread count: the fastest of a sweep on the MI355X box's host (profiles/r06_cpu_threads.txt, tools/cpu_threads.py: 16 threads
    # 0.90 images/s, 32 0.73, 64 0.42, 128 0.16, all 256 0.012 -- oneDNN's convolutions at batch 4 thrash beyond a few dozen threads);
    # FSR_CPU_THREADS overrides.  `cores` in the line is what was used, `host_cores` what the box has
    cores = max(1, min(avail, int(os.environ.get("FSR_CPU_THREADS", "16"))))
    torch.set_num_threads(cores)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        G = pkg.Generator(ns(n_filters=64, n_layers=8))
        Dm = pkg.Discriminator(ns(n_filters=64, n_layers=7))
    g_sd = {k: v.detach().clone() for k, v in G.state_dict().items()}
    d_sd = {k: v.detach().clone() for k, v in Dm.state_dict().items()}
    v_sd = O.vgg_standin_state_dict(1234, 1)
    b = 4
    lr, hr = torch.rand(b, 3, 96, 96) * 2 - 1, torch.rand(b, 3, 384, 384) * 2 - 1
    noise = [torch.rand(b, 1, 24, 24) for _ in range(3)]
    gs, ds = {}, {}
    O.train_step(g_sd, d_sd, v_sd, lr, hr, noise, gs, ds)
    t0 = time.perf_counter()
    iters = 2
    for _ in range(iters):
        O.train_step(g_sd, d_sd, v_sd, lr, hr, noise, gs, ds)
    dt = (time.perf_counter() - t0) / iters
    out = {"value": round(b / dt, 4), "unit": "images/s", "cores": cores, "host_cores": os.cpu_count(), "kind": "port",
           "sample": "oracle/srgan_cpu.train_step (full GAN iteration, fp32, torch CPU), batch %d, 96->384, "
                     "1 warm-up + %d timed iterations, %.2f s each; generator inference: oracle.generator_forward, batch 1, "
                     "1 warm-up + 3 timed frames per size" % (b, iters, dt)}
    # BASELINE.md section 3 / configs[0]: "inference + one G/D step" -- the CPU figure beside the GPU inference FPS
    with torch.no_grad():
        for name, (h, w) in (("90x160", (90, 160)), ("180x320", (180, 320))):
            x = torch.rand(1, 3, h, w) * 2 - 1
            O.generator_forward(g_sd, x)
            t0 = time.perf_counter()
            for _ in range(3):
                O.generator_forward(g_sd, x)
            out["inference_fps_%s" % name] = round(3 / (time.perf_counter() - t0), 3)
    return out


def respawn_under_launcher(args):
    """`python bench.py --gpus N` (N > 1) without RANK/WORLD_SIZE: run the same command under torch.distributed.run, one
    process per GPU, and relay rank 0's JSON line."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def time_steps(step_fn, lr, hr, steps, warmup, world, device):
    def barrier():
        if world > 1:
            torch.distributed.barrier()

    for _ in range(warmup):
        step_fn(lr, hr)
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        last = step_fn(lr, hr)
    torch.cuda.synchronize()
    barrier()
    elapsed = time.perf_counter() - t0
    time_steps.last = last              # what the final timed step returned (--dump-outputs)
    per_rank = [elapsed]
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        allt = [torch.zeros_like(t) for _ in range(world)]
        torch.distributed.all_gather(allt, t)
        per_rank = [float(x.item()) for x in allt]
        elapsed = max(per_rank)
    time_steps.per_rank = per_rank      # (rank 0 reports min / max over ranks next to the MAX the contract asks for)
    return elapsed


def build_step(pkg, trainer, lr, hr, use_graph):
    """(step function, launch description)."""
    if use_graph:
        try:
            trainer.capture_train_step(lr, hr)
            n = len(trainer._graphs)
            return trainer.graphed_train_step, ("hipGraph replay" if n == 1 else "%d phase hipGraphs + 2 RCCL all-reduces" % n)
        except Exception as exc:  # noqa: BLE001 -- fall back to eager launches and say so in the JSON line
            print("bench: hipGraph capture failed (%s: %s); running eager" % (type(exc).__name__, exc), file=sys.stderr)
            torch.cuda.synchronize()
    return trainer.train_step, "eager"


def measure_roofline(trainer, ops, lr, hr, dtype, ms_per_step, B):
    """One instrumented single-stream iteration (outside any timed region): every convolution launch bracketed by HIP events on
    its launch stream.  (Single-stream: with the perceptual branch and the weight gradients on their own streams, kernels of
    several streams share the GPU and an event pair around one launch would also time its neighbours.)
    Returns (roofline dict, executed GFLOP per image)."""
    args = types.SimpleNamespace(dtype=dtype)
    side, wstream = trainer.use_side_stream, ops.USE_WGRAD_STREAM
    trainer.use_side_stream = False
    ops.USE_WGRAD_STREAM = False
    trainer.train_step(lr, hr)
    rec = conv_profile(ops, lambda: trainer.train_step(lr, hr))
    trainer.use_side_stream, ops.USE_WGRAD_STREAM = side, wstream
    conv = [r for r in rec if r[4] in ("fwd", "dgrad")]
    wgr = [r for r in rec if r[4] == "wgrad"]
    launches = len(conv)
    conv_ms, conv_flops, conv_bytes = sum(r[0] for r in conv), sum(r[1] for r in conv), sum(r[2] for r in conv)
    achieved = conv_flops / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
    # fraction of the family's time an ideal machine would need: sum(flops_i / peak_i) / sum(t_i) -- for a one-dtype mode simply
    # achieved / peak, for x3v (x3 and fp16 launches side by side) the only meaningful aggregate
    fam_frac = sum(r[1] / (kernel_peak(r[3], args.dtype) * 1e12) for r in conv) / (conv_ms * 1e-3) if conv_ms > 0 else 0.0
    by_kernel = {}
    for ms, fl, by, name, _ in conv:
        e = by_kernel.setdefault(name, [0, 0.0, 0.0, 0.0])
        e[0] += 1
        e[1] += ms
        e[2] += fl
        e[3] += by
    dom_name, dom = max(by_kernel.items(), key=lambda kv: kv[1][1]) if by_kernel else ("?", [0, 1.0, 0.0, 0.0])
    dom_tf = dom[2] / (dom[1] * 1e-3) / 1e12 if dom[1] > 0 else 0.0
    peak = kernel_peak(dom_name, args.dtype)
    # HBM traffic from the PMC passes recorded for exactly these kernel sources (tools/pmc_traffic.py): the dominant kernel's own
    # dispatches, and the whole family
    traffic = fam_traffic = None
    traffic_src = "no PMC record for these kernel sources (profiles/conv_traffic.json)"
    traffic_file = TRAFFIC_FILE if args.dtype not in ("x3", "x3v") else TRAFFIC_FILE.replace(".json", "_%s.json" % args.dtype)
    if os.path.exists(traffic_file):
        try:
            t = json.load(open(traffic_file))
            if t.get("kernel_sources_sha16") == kernel_sources_hash() and t.get("dtype") == args.dtype and t.get("batch") == B:
                fam_traffic = t["bytes_per_launch"]
                # rocprofv3 prints every template argument (conv_tall3's trailing STATS flag: ",false>" / ",true>"), the library's
                # own kernel note (fsr_last_kernel) prints "<...>" / "<...,stats>"
                per = {k.replace(",false>", ">").replace(",true>", ",stats>"): v for k, v in t.get("per_kernel", {}).items()}
                traffic = per.get(dom_name, {}).get("bytes_per_dispatch")
                traffic_src = ("rocprofv3 --pmc FETCH_SIZE (x2, gfx950 correction) + WRITE_SIZE over one iteration (%s), "
                               "recorded in profiles/%s for kernel sources %s" % (t.get("files", "?"), os.path.basename(traffic_file), t["kernel_sources_sha16"]))
            else:
                traffic_src = "profiles/conv_traffic.json was recorded for other kernel sources / another workload: not quoted"
        except (OSError, ValueError, KeyError):
            pass
    # `roofline` = the DOMINANT kernel (the single kernel symbol with the largest share of the iteration); `family` = all conv
    # forward + data-gradient launches together; `kernels` = every configuration of the family against both roofs
    roofline = {"bound": "mfma", "kernel": dom_name,
                "achieved": round(dom_tf, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(dom_tf / peak, 4),
                "traffic": traffic, "traffic_source": traffic_src,
                "algorithmic_bytes_per_launch": round(dom[3] / max(dom[0], 1)), "launches_per_step": dom[0],
                "avg_launch_us": round(dom[1] * 1e3 / max(dom[0], 1), 2),
                "algorithmic_gflop_per_launch": round(dom[2] / max(dom[0], 1) / 1e9, 3),
                "share_of_step_time": round(dom[1] / ms_per_step, 3),
                # what a bare loop whose operands pass through LDS reaches with the dominant kernel's wave tile (128 px x 64
                # channels of v_mfma_f32_32x32x16, two waves per SIMD): tools/ubench/lds_mfma32.hip, profiles/r03_ubench_lds_mfma32.txt
                "lds_fed_mfma_ceiling": {"tflops": LDS_FED_CEILING_TFLOPS.get(args.dtype), "frac": (round(dom_tf / LDS_FED_CEILING_TFLOPS[args.dtype], 4)
                                                                                                if args.dtype in LDS_FED_CEILING_TFLOPS else None)},
                "family": {"kernel": "3x3 convolution forward + data-gradient launches (conv_igemm_kernel / conv64 persistent kernels / first-layer kernels)",
                           "achieved": round(achieved, 2), "frac": round(fam_frac, 4), "traffic": fam_traffic,
                           "algorithmic_bytes_per_launch": round(conv_bytes / max(launches, 1)), "launches_per_step": launches,
                           "avg_launch_us": round(conv_ms * 1e3 / max(launches, 1), 2),
                           "algorithmic_gflop_per_launch": round(conv_flops / max(launches, 1) / 1e9, 3),
                           "share_of_step_time": round(conv_ms / ms_per_step, 3)},
                "kernels": [{"kernel": k, "launches_per_step": v[0], "ms_per_step": round(v[1], 3),
                             "tflops": round(v[2] / (v[1] * 1e-3) / 1e12, 1), "mfma_frac": round(v[2] / (v[1] * 1e-3) / 1e12 / kernel_peak(k, args.dtype), 3),
                             "algorithmic_gb_per_s": round(v[3] / (v[1] * 1e-3) / 1e9, 1), "hbm_frac": round(v[3] / (v[1] * 1e-3) / 1e9 / HBM_PEAK_GBS, 3)}
                            for k, v in sorted(by_kernel.items(), key=lambda kv: -kv[1][1])[:10] if v[1] > 0],
                "weight_gradient": {"launches_per_step": len(wgr), "achieved": round(sum(r[1] for r in wgr) / max(sum(r[0] for r in wgr), 1e-9) / 1e9, 2),
                                    "unit": "TFLOP/s", "ms_per_step": round(sum(r[0] for r in wgr), 3)}}
    return roofline, sum(r[1] for r in rec) / B / 1e9


LEAN_LIMIT = 6000      # bytes: the driver's record keeps the last 8 KB of stdout (round 5's 25 KB line did not parse there)
_CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                  "dtype", "data")
_ROOFLINE_KEYS = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch",
                  "algorithmic_gflop_per_launch", "launches_per_step", "avg_launch_us", "share_of_step_time", "peak_note")
_CPU_KEYS = ("value", "unit", "cores", "host_cores", "kind", "sample", "inference_fps_90x160", "inference_fps_180x320")


def lean_line(full):
    """The ONE stdout line: the contract keys, `config`, the dominant kernel's `roofline` (scalars only, with `traffic`),
    `cpu_baseline` and ONE scalar per leg; everything else stays in bench_detail.json.  Optional keys are dropped, least
    important first, until the line is under LEAN_LIMIT bytes (tests/test_tools.py runs this on canned numbers)."""
    def clip(text, n):
        text = str(text)
        return text if len(text) <= n else text[:n - 3] + "..."

    line = {k: full[k] for k in _CONTRACT_KEYS if k in full}
    line["data"] = clip(line.get("data", "synthetic"), 120)
    cfg = dict(full.get("config", {}))
    prec = cfg.pop("precision", None)
    line["config"] = {k: (clip(v, 140) if isinstance(v, str) else v) for k, v in cfg.items()}
    roof = full.get("roofline") or {}
    if roof:            # (a plain run measures no roofline)
        line["roofline"] = {k: roof[k] for k in _ROOFLINE_KEYS if k in roof}
        line["roofline"].setdefault("traffic", None)
    fam = roof.get("family") or {}
    if fam:
        line["roofline"]["family_frac"] = fam.get("frac")
    if "cpu_baseline" in full:
        cb = full["cpu_baseline"]
        line["cpu_baseline"] = {k: (clip(cb[k], 200) if isinstance(cb[k], str) else cb[k]) for k in _CPU_KEYS if k in cb}
    legs = {full.get("dtype", "?"): full.get("value")}
    fracs = {full.get("dtype", "?"): roof.get("frac")}
    for dt in ("x3v", "x3", "f16", "bf16", "f32"):
        leg = full.get(dt + "_mode")
        if leg:
            legs[dt] = leg.get("value")
            fracs[dt] = (leg.get("roofline") or {}).get("frac")
    line["legs_images_per_s"] = legs
    line["legs_dominant_kernel_frac"] = fracs
    if full.get("sustained"):
        line["sustained_images_per_s"] = full["sustained"].get("value")
    if (full.get("clock") or {}).get("sclk_mhz_mean"):
        line["sclk_mhz_mean"] = full["clock"]["sclk_mhz_mean"]
    for k in ("step_tflops_executed", "step_gflop_executed_per_image", "timed_region_s"):
        if k in full:
            line[k] = full[k]
    if full.get("cfg5"):
        c5 = full["cfg5"]
        line["cfg5"] = {"images_per_s": c5.get("value"), "dtype": c5.get("dtype"), "per_gpu_batch": c5.get("per_gpu_batch"),
                        "ms_per_step": c5.get("ms_per_step"), "roofline_frac": (c5.get("roofline") or {}).get("frac")}
    inf = full.get("inference")
    if inf:
        sizes = ("90x160_b1", "90x160_b32", "180x320_b1", "180x320_b32")
        per = {inf.get("dtype", "?"): inf}
        per.update(inf.get("modes") or {})
        line["inference_fps"] = {m: {k: v.get("fps_" + k) for k in sizes if "fps_" + k in v} for m, v in per.items()}
        line["inference_fps"]["e2e_%s" % inf.get("e2e_dtype", "?")] = {k[len("e2e_fps_"):]: v for k, v in inf.items() if k.startswith("e2e_fps_")}
    if full.get("allreduce"):
        ar = full["allreduce"]
        line["allreduce"] = {k: ar[k] for k in ("ms_in_allreduce", "ms_in_allreduce_max_over_ranks", "per_exchange_ms", "bytes") if k in ar}
    if full.get("ms_per_step_ranks"):
        line["ms_per_step_ranks"] = full["ms_per_step_ranks"]
    if (full.get("data_pipeline") or {}).get("crops_per_s"):
        line["data_pipeline_crops_per_s"] = full["data_pipeline"]["crops_per_s"]
    if prec:
        line["precision"] = clip(prec, 420)
    if "detail_file" in full:
        line["detail_file"] = full["detail_file"]
    text = json.dumps(line)
    for k in ("precision", "data_pipeline_crops_per_s", "ms_per_step_ranks", "legs_dominant_kernel_frac", "inference_fps", "cfg5", "allreduce"):
        if len(text) <= LEAN_LIMIT:
            break
        line.pop(k, None)
        text = json.dumps(line)
    assert len(text) <= LEAN_LIMIT, "bench: the lean line is %d bytes" % len(text)
    return text


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(directory, losses, trainer):
    """--dump-outputs: the losses the last timed step returned and the Generator / Discriminator weights it left, as float32
    <directory>/<name>.npy (the module docstring lists the files)."""
    import numpy as np
    arrays = {k: v.detach().float().cpu().numpy() for k, v in losses.items()}
    for name, net in (("generator", trainer.generator), ("discriminator", trainer.discriminator)):
        arrays[name] = torch.cat([v.detach().float().reshape(-1) for v in net.state_dict().values() if v.is_floating_point()]).cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, "bench: the outputs are %d bytes" % total
    os.makedirs(directory, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed steps (default 200: > 5 s of bf16 work, so the clock has settled)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (default: 32 for cfg3, 4 for cfg5)")
    ap.add_argument("--workload", default="cfg3", choices=sorted(WORKLOADS), help="cfg3 = the headline metric; cfg5 = BASELINE configs[4]")
    ap.add_argument("--dtype", default=None, choices=["bf16", "f16", "f32", "x3", "x3v"],
                    help="default: the workload's (cfg3: x3v = x3 Generator / Discriminator + fp16 perceptual network, the fastest mode inside "
                         "north_star's 1e-3 on every output and loss; cfg5: f16, the dtype BASELINE configs[4] names)")
    ap.add_argument("--no-cfg5", action="store_true", help="skip the BASELINE configs[4] leg of the default N = 1 line")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-inference", action="store_true")
    ap.add_argument("--no-f32", action="store_true", help="skip the exact-f32 (reference precision) leg")
    ap.add_argument("--no-x3", action="store_true", help="skip the x3 leg (when --dtype is not x3)")
    ap.add_argument("--no-f16", action="store_true", help="skip the fp16 leg (the default 16-bit training mode; outside 1e-3)")
    ap.add_argument("--no-bf16", action="store_true", help="skip the bf16 leg (the headline dtype of rounds 1-4, BASELINE configs[1]'s dtype)")
    ap.add_argument("--inference-seconds", type=float, default=1.5, help="minimum timed region of every model-only inference leg")
    ap.add_argument("--inference-dtypes", default="x3,f16,bf16,f32", help="compute modes of the inference legs (the first one fills the top-level keys)")
    ap.add_argument("--sustained-seconds", type=float, default=5.0, help="length of the sustained leg of the headline mode (0: none)")
    ap.add_argument("--detail", default=None, help="where the FULL object goes (default: gpurun_out/bench_detail.json when gpurun_out/ exists, else ./bench_detail.json)")
    ap.add_argument("--no-sustained", action="store_true", help="skip the >= 5 s sustained legs that follow a short timed region")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of hipGraph replays")
    ap.add_argument("--full", action="store_true", help="every leg besides the headline (sustained, all-reduce cost, rooflines, the other compute "
                                                        "modes, cfg5, inference, data pipeline, CPU baseline) and bench_detail.json")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's losses and the G / D weights it left to DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:       # a plain run measures the headline only
        args.no_sustained = args.no_cfg5 = args.no_cpu_baseline = args.no_inference = True
        args.no_f32 = args.no_x3 = args.no_f16 = args.no_bf16 = True

    # FSR_BENCH_FORCE_SPAWN=1 takes the launcher path for N = 1 as well (tests: the self-spawn logic on a one-GPU box)
    if (args.gpus > 1 or os.environ.get("FSR_BENCH_FORCE_SPAWN") == "1") and "WORLD_SIZE" not in os.environ:
        raise SystemExit(respawn_under_launcher(args))

    pkg = importlib.import_module("fast-srgan_amd")
    ops = importlib.import_module("fast-srgan_amd.ops")
    dist_mod = importlib.import_module("fast-srgan_amd.distributed")
    rank, world, local_rank = dist_mod.init_from_env()
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no GPU visible)")
    torch.cuda.set_device(local_rank)
    device = "cuda:%d" % local_rank
    pkg._lib.lib()  # fail loudly if the HIP extension is missing
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))

    wl = WORKLOADS[args.workload]
    if args.batch is None:
        args.batch = wl["batch"]
    if args.dtype is None:
        args.dtype = wl["dtype"]
    if args.workload != "cfg3":
        args.no_inference = args.no_f32 = args.no_x3 = args.no_f16 = args.no_bf16 = args.no_cpu_baseline = args.no_cfg5 = True     # those legs belong to the headline workload
    torch.manual_seed(1234)
    trainer = pkg.Trainer(make_config(args.batch, args.dtype, device, wl), perceptual_network=pkg.VGG19(compute_dtype=args.dtype, seed=1234))
    torch.manual_seed(100 + rank)
    B = args.batch
    hr_size = wl["lr"] * 2 ** wl["n_upsample"]
    lr = torch.rand(B, 3, wl["lr"], wl["lr"], device=device) * 2 - 1
    hr = torch.rand(B, 3, hr_size, hr_size, device=device) * 2 - 1

    step_fn, launch = build_step(pkg, trainer, lr, hr, not args.no_graph)
    with (ClockSampler(local_rank) if args.full else contextlib.nullcontext()) as clk:
        elapsed = time_steps(step_fn, lr, hr, args.steps, args.warmup, world, device)
    per_rank = list(time_steps.per_rank)
    ms_per_step = elapsed / args.steps * 1e3
    value = world * B * args.steps / elapsed
    if rank == 0 and args.dump_outputs:     # before anything else steps the trainer
        dump_outputs(args.dump_outputs, time_steps.last, trainer)

    def sustained_leg(fn, ms_guess, nominal_batch):
        """>= --sustained-seconds of back-to-back steps with the shader clock sampled: what the rate settles at."""
        n = max(20, int(args.sustained_seconds * 1e3 / max(ms_guess, 1e-3)) + 1)
        with ClockSampler(local_rank) as c:
            el = time_steps(fn, lr, hr, n, 2, world, device)
        return {"value": round(world * nominal_batch * n / el, 3), "unit": "images/s", "steps": n, "seconds": round(el, 2),
                "ms_per_step": round(el / n * 1e3, 3), "clock": c.summary()}

    sustained = None
    if not args.no_sustained and args.sustained_seconds > 0 and elapsed < args.sustained_seconds:
        sustained = sustained_leg(step_fn, ms_per_step, B)

    # N > 1 (or a 1-rank RCCL world): what the two gradient exchanges cost a step, outside the timed region -- HIP events from
    # the moment the main stream hands a gradient arena to RCCL to the moment it may continue (distributed.GradSync.record)
    allreduce = None
    if dist_mod.is_distributed() and args.full:
        dist_mod.GradSync.record = []
        n_ar = 10
        for _ in range(n_ar):
            step_fn(lr, hr)
        torch.cuda.synchronize()
        rec, dist_mod.GradSync.record = dist_mod.GradSync.record, None
        per = {}
        for tag, e0, e1 in rec:
            per[tag] = per.get(tag, 0.0) + e0.elapsed_time(e1)
        allreduce = {"ms_in_allreduce": round(sum(per.values()) / n_ar, 4),
                     "per_exchange_ms": {k: round(v / n_ar, 4) for k, v in per.items()},
                     "bytes": {"discriminator": trainer.optim_discriminator.flat_grad.numel() * 4, "generator": trainer.optim_generator.flat_grad.numel() * 4},
                     "steps": n_ar, "rank": rank,
                     "what": "HIP events on the main stream around each exchange (start of the RCCL all-reduce -> the stream may continue); "
                             "under phase graphs nothing overlaps an exchange, so this is its exposed cost"}
        if world > 1:   # the slowest rank's figure is the one that matters
            t = torch.tensor([allreduce["ms_in_allreduce"]], device=device, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            allreduce["ms_in_allreduce_max_over_ranks"] = round(float(t.item()), 4)

    out = {"metric": wl["metric"],
           "value": round(value, 3), "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": args.dtype, "data": "synthetic (uniform [-1,1) LR/HR tensors resident in HBM; random-init G/D, kaiming-normal VGG19 stand-in)",
           "config": {"workload": wl["name"],
                      "per_gpu_batch": B, "global_batch": B * world, "parallelism": "dp%d" % world,
                      "collectives": ("rccl world %d" % torch.distributed.get_world_size()) if dist_mod.is_distributed() else "none",
                      "rccl_world_size": torch.distributed.get_world_size() if dist_mod.is_distributed() else 1,
                      "launch": launch,
                      "precision": PRECISION_NOTE[args.dtype]},
           "timed_region_s": round(elapsed, 3),
           "ms_per_step_ranks": {"min": round(min(per_rank) / args.steps * 1e3, 3), "max": round(max(per_rank) / args.steps * 1e3, 3)}}
    if args.full:
        roofline, executed_gflop_per_image = measure_roofline(trainer, ops, lr, hr, args.dtype, ms_per_step, B)
        out.update({"clock": clk.summary(),
                    "step_gflop_executed_per_image": round(executed_gflop_per_image, 2),
                    "step_tflops_executed": round(value * executed_gflop_per_image / 1e3, 2),
                    "step_gflop_reference_graph_per_image": wl["gflop_ref"],
                    "roofline": roofline})

    # `peak` is the dense MFMA figure at the 2.4 GHz boost clock; under a dense kernel the part runs power-limited well
    # below it (sysfs pp_dpm_sclk sampled over the timed region), and with memory traffic lower still
    # (profiles/r03_wgrad_ablation.txt).  Reported beside `frac`, never instead of it.
    sclk = (out.get("clock") or {}).get("sclk_mhz_mean")
    if sclk:
        pk = roofline["peak"] * sclk / NOMINAL_SCLK_MHZ
        roofline["at_measured_clock"] = {"sclk_mhz_mean": sclk, "nominal_sclk_mhz": NOMINAL_SCLK_MHZ, "peak": round(pk, 1),
                                         "frac": round(roofline["achieved"] / pk, 4),
                                         "note": "clock = mean over the timed iterations (all kernels), not the dominant kernel alone"}
    if sustained is not None:
        out["sustained"] = sustained
    if allreduce is not None:
        out["allreduce"] = allreduce
    def precision_leg(dt, described, meets):
        """The same iteration in another compute mode, timed with the SAME --steps / --warmup, with its own roofline, clock and
        (after a short timed region) sustained leg."""
        torch.manual_seed(1234)
        t2 = pkg.Trainer(make_config(B, dt, device, wl), perceptual_network=pkg.VGG19(compute_dtype=dt, seed=1234))
        fn2, launch2 = build_step(pkg, t2, lr, hr, not args.no_graph)
        with ClockSampler(local_rank) as clk2:
            el = time_steps(fn2, lr, hr, args.steps, args.warmup, 1, device)
        ms2 = el / args.steps * 1e3
        roof2, gflop2 = measure_roofline(t2, ops, lr, hr, dt, ms2, B)
        roof2.pop("lds_fed_mfma_ceiling", None)
        leg = {"value": round(B * args.steps / el, 3), "unit": "images/s", "ms_per_step": round(ms2, 2), "steps": args.steps,
               "warmup": args.warmup, "timed_region_s": round(el, 3), "launch": launch2, "dtype": described,
               "meets_north_star_tolerance": meets,
               "step_tflops_executed": round(B * args.steps / el * gflop2 / 1e3, 2), "clock": clk2.summary(), "roofline": roof2}
        del t2, fn2
        torch.cuda.empty_cache()
        return leg

    # the other compute modes, each timed with the SAME --steps / --warmup and its own roofline
    del step_fn
    for dt, skip in (("x3v", args.no_x3), ("x3", args.no_x3), ("f16", args.no_f16), ("bf16", args.no_bf16), ("f32", args.no_f32)):
        if rank == 0 and world == 1 and not skip and dt != args.dtype and args.workload == "cfg3":
            out[dt + "_mode"] = precision_leg(dt, MODE_DESCRIBED[dt], MODE_MEETS[dt])
            if abs(out[dt + "_mode"]["roofline"]["peak"] - MFMA_PEAK_TFLOPS["x3"]) < 1e-6:
                out[dt + "_mode"]["roofline"]["peak_note"] = "2500 / 3 TFLOP/s: three bf16 MFMAs per algorithmic multiply-add"
    if args.full and abs(roofline["peak"] - MFMA_PEAK_TFLOPS["x3"]) < 1e-6:
        roofline["peak_note"] = "2500 / 3 TFLOP/s: three bf16 MFMAs per algorithmic multiply-add"

    if rank == 0 and world == 1 and not args.no_cfg5:
        # BASELINE configs[4] as a measured configuration (round-3 verdict): 12 blocks, three pixel-shuffle stages, 128 -> 1024,
        # fp16 MFMA with the dynamic loss scale, batch 4 on one GPU (configs[4] names 8 GPUs: weak scaling repeats this per GPU),
        # >= 100 steps and >= 5 s timed, hipGraph replay, its own roofline
        w5 = WORKLOADS["cfg5"]
        b5, dt5 = w5["batch"], w5["dtype"]
        torch.manual_seed(1234)
        t5 = pkg.Trainer(make_config(b5, dt5, device, w5), perceptual_network=pkg.VGG19(compute_dtype=dt5, seed=1234))
        hr5 = w5["lr"] * 2 ** w5["n_upsample"]
        lr_5 = torch.rand(b5, 3, w5["lr"], w5["lr"], device=device) * 2 - 1
        hr_5 = torch.rand(b5, 3, hr5, hr5, device=device) * 2 - 1
        fn5, launch5 = build_step(pkg, t5, lr_5, hr_5, not args.no_graph)
        el = time_steps(fn5, lr_5, hr_5, 10, 3, 1, device)                      # a first estimate of the step time
        n5 = max(100, int(3000.0 / (el / 10 * 1e3)) + 1)
        with ClockSampler(local_rank) as clk5:
            el = time_steps(fn5, lr_5, hr_5, n5, 2, 1, device)
        ms5 = el / n5 * 1e3
        roof5, gflop5 = measure_roofline(t5, ops, lr_5, hr_5, dt5, ms5, b5)
        for k in ("traffic", "traffic_source", "family", "lds_fed_mfma_ceiling"):
            roof5.pop(k, None)
        roof5["kernels"] = roof5["kernels"][:5]
        scale5 = t5.loss_scale_state()
        out["cfg5"] = {"metric": w5["metric"], "workload": w5["name"], "value": round(b5 * n5 / el, 3), "unit": "images/s",
                       "per_gpu_batch": b5, "n_gpus": 1, "dtype": dt5, "steps": n5, "timed_region_s": round(el, 3), "ms_per_step": round(ms5, 3),
                       "launch": launch5, "clock": clk5.summary(), "step_gflop_executed_per_image": round(gflop5, 2),
                       "step_tflops_executed": round(b5 * n5 / el * gflop5 / 1e3, 2),
                       "loss_scale": {"final": scale5[0], "skipped_iterations": scale5[1]} if scale5 else None,
                       "parity": "tests/test_parity_bench.py::test_train_step_cfg5_three_stage_generator_f16, ::test_generator_cfg5_full_size_vs_oracle",
                       "roofline": roof5}
        del t5, fn5, lr_5, hr_5
        torch.cuda.empty_cache()

    if rank == 0 and not args.no_inference:
        import numpy as np
        gen_sd = {k: v.detach().clone() for k, v in trainer.generator.state_dict().items()}
        modes = [m for m in args.inference_dtypes.split(",") if m]
        inf_dt = {"x3v": "x3"}.get(args.dtype, args.dtype)      # (x3v differs from x3 in the perceptual network only: the generator is x3)
        if inf_dt not in modes:
            modes = [inf_dt] + modes
        if world > 1:       # the other ranks wait at the final barrier meanwhile: the default mode only
            modes = [inf_dt]

        def model_only(dt):
            """Generator-only FPS in compute mode dt: every leg one hipGraph launch per call, >= --inference-seconds timed with the
            shader clock sampled; plus the roofline of the forward's dominant kernel at 180x320, batch 32 (HIP events around
            every convolution launch of one eager forward)."""
            legs = {"dtype": dt}
            Gm = trainer.generator.eval() if dt == inf_dt else pkg.Generator(ns(n_filters=64, n_layers=wl["n_layers"], n_upsample=wl["n_upsample"]),
                                                                                  compute_dtype=dt).to(device).eval()
            if dt != inf_dt:
                Gm.load_state_dict(gen_sd)
            launch_kind = "hipGraph replay"
            for name, (h, w) in (("90x160", (90, 160)), ("180x320", (180, 320))):
                for bsz in (1, 32):
                    x = torch.rand(bsz, 3, h, w, device=device) * 2 - 1
                    run = Gm
                    try:   # one hipGraph launch per frame/batch (batch-1 eager inference is host-launch bound)
                        run = pkg.GraphedGenerator(Gm, x)
                    except Exception as exc:  # noqa: BLE001
                        print("bench: inference graph capture failed (%s); eager" % exc, file=sys.stderr)
                        launch_kind = "eager"
                    for _ in range(3):
                        run(x)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(5):
                        run(x)
                    torch.cuda.synchronize()
                    est = (time.perf_counter() - t0) / 5
                    iters = max(10, int(args.inference_seconds / max(est, 1e-6)) + 1)
                    with ClockSampler(local_rank) as c:
                        t0 = time.perf_counter()
                        for _ in range(iters):
                            run(x)
                        torch.cuda.synchronize()
                        el = time.perf_counter() - t0
                    key = "%s_b%d" % (name, bsz)
                    legs["fps_" + key] = round(bsz * iters / el, 2)
                    legs.setdefault("timed", {})[key] = {"calls": iters, "seconds": round(el, 2), "sclk_mhz_mean": c.summary().get("sclk_mhz_mean")}
                    del run
            legs["launch"] = launch_kind
            x = torch.rand(32, 3, 180, 320, device=device) * 2 - 1
            Gm(x)
            rec = [r for r in conv_profile(ops, lambda: Gm(x)) if r[4] == "fwd"]
            by = {}
            for ms, fl, byts, kname, _ in rec:
                e = by.setdefault(kname, [0, 0.0, 0.0, 0.0])
                e[0] += 1; e[1] += ms; e[2] += fl; e[3] += byts
            if by:
                dom_name, dom = max(by.items(), key=lambda kv: kv[1][1])
                peak = MFMA_PEAK_TFLOPS[dt]
                tf = dom[2] / (dom[1] * 1e-3) / 1e12
                conv_ms = sum(v[1] for v in by.values())
                fps = legs["fps_180x320_b32"]
                legs["roofline"] = {"bound": "mfma", "kernel": dom_name, "achieved": round(tf, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                                    "frac": round(tf / peak, 4), "launches_per_forward": dom[0], "avg_launch_us": round(dom[1] * 1e3 / dom[0], 2),
                                    "algorithmic_gflop_per_launch": round(dom[2] / dom[0] / 1e9, 3),
                                    "algorithmic_bytes_per_launch": round(dom[3] / dom[0]), "hbm_frac": round(dom[3] / (dom[1] * 1e-3) / 1e9 / HBM_PEAK_GBS, 3),
                                    "share_of_conv_time": round(dom[1] / conv_ms, 3),
                                    "workload": "generator forward at 180x320, batch 32 (one eager forward, HIP events per convolution launch)",
                                    "whole_forward": {"gflop_per_frame": round(sum(v[2] for v in by.values()) / 32 / 1e9, 2),
                                                      "tflops_at_fps_180x320_b32": round(fps * sum(v[2] for v in by.values()) / 32 / 1e12, 1),
                                                      "frac": round(fps * sum(v[2] for v in by.values()) / 32 / 1e12 / peak, 4)},
                                    "kernels": [{"kernel": k, "launches": v[0], "ms": round(v[1], 3), "tflops": round(v[2] / (v[1] * 1e-3) / 1e12, 1),
                                                 "mfma_frac": round(v[2] / (v[1] * 1e-3) / 1e12 / peak, 3), "hbm_frac": round(v[3] / (v[1] * 1e-3) / 1e9 / HBM_PEAK_GBS, 3)}
                                                for k, v in sorted(by.items(), key=lambda kv: -kv[1][1])[:6]],
                                    "rocprofv3_summary": "profiles/r06_inference_kernel_stats_%s.csv" % dt}
            if dt != inf_dt:
                del Gm
            torch.cuda.empty_cache()
            return legs

        with torch.no_grad():
            per_mode = {m: model_only(m) for m in modes}
        inf = dict(per_mode[modes[0]])          # top level: the first mode (`dtype` beside the figures says which)
        inf["modes"] = {m: per_mode[m] for m in modes[1:]}
        inf["modes_note"] = ("top level = the mode `dtype` names (default x3: the fast mode inside north_star's 1e-3, measured 6e-5 .. 7e-5 at "
                             "these sizes, tests/test_parity_bench.py); f32 = exact-f32 MFMA; bf16 = BASELINE configs[1]'s dtype (mean |error| "
                             "2.9e-3 on (-1,1) images; fp16: an eighth of that)")
        e2e_dt = args.dtype if args.dtype in ("f16", "bf16") else "f16"       # the frame pipeline ships in fp16 (inference.py's default)
        with torch.no_grad():
            if e2e_dt == args.dtype:
                G = trainer.generator.eval()
            else:
                G = pkg.Generator(ns(n_filters=64, n_layers=wl["n_layers"], n_upsample=wl["n_upsample"]), compute_dtype=e2e_dt).to(device).eval()
                G.load_state_dict(gen_sd)
            # end to end: uint8 frames in host memory -> H2D -> generator (uint8 head epilogue) -> D2H -> host arrays
            rng = np.random.default_rng(0)

            def e2e_rate(pipe, frames, passes=3):
                """frames per second of `passes` timed passes over `frames`, each pass timed on its own: median, min, max (the
                single 4-pass figure of earlier rounds moved 3x between boxes -- host-side: the first pass after a pipeline is built
                pays pinned-buffer page faults and graph instantiation, and a box's host threads are not always idle)."""
                for _ in pipe.run(frames[:2 * pipe.batch]):
                    pass
                for _ in pipe.run(frames):          # one full untimed pass: every staging slot and plan is warm
                    pass
                rates = []
                for _ in range(passes):
                    t0, count = time.perf_counter(), 0
                    for _y in pipe.run(frames):
                        count += 1
                    rates.append(count / (time.perf_counter() - t0))
                rates.sort()
                return round(rates[len(rates) // 2], 2), {"min": round(rates[0], 2), "max": round(rates[-1], 2), "passes": passes, "frames_per_pass": len(frames)}

            inf["e2e_spread"] = {}
            for name, (h, w) in (("90x160", (90, 160)), ("180x320", (180, 320))):
                for bsz in (1, 8):
                    frames = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(64 if bsz == 1 else 128)]
                    pipe = pkg.InferencePipeline(G, device, batch=bsz, depth=2)
                    key = "e2e_fps_%s_b%d" % (name, bsz)
                    inf[key], inf["e2e_spread"][key] = e2e_rate(pipe, frames)
            pipe = pkg.InferencePipeline(G, device, batch=8, depth=3, copy=False)     # zero-copy hand-off of the pinned results
            inf["e2e_fps_180x320_b8_zero_copy"], inf["e2e_spread"]["e2e_fps_180x320_b8_zero_copy"] = e2e_rate(pipe, frames)
            inf["e2e_dtype"] = e2e_dt
            inf["e2e"] = "InferencePipeline: pinned uint8 frames -> H2D -> hipGraph(u8->[-1,1], G, uint8 head) -> D2H -> numpy, depth 2"
        out["inference"] = inf
        # device crop pipeline (dataloader.py:24-38 replacement): 96 -> 384 crops cut from a resident uint8 pool
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            rng = np.random.default_rng(0)
            paths = []
            for i in range(4):
                path = os.path.join(td, "img%d.npy" % i)
                np.save(path, rng.integers(0, 256, size=(3, 1356 + 8 * i, 2040), dtype=np.uint8))   # DIV2K-sized
                paths.append(path)
            ds = pkg.NumpyImagesDataset(paths, lr_image_size=96, scale_factor=4, device=device)
            for _ in pkg.DeviceBatchLoader(ds, B, 2, seed=1):
                pass
            torch.cuda.synchronize()
            iters = 20
            t0 = time.perf_counter()
            for _ in pkg.DeviceBatchLoader(ds, B, iters, seed=2):
                pass
            torch.cuda.synchronize()
            out["data_pipeline"] = {"crops_per_s": round(B * iters / (time.perf_counter() - t0), 1),
                                    "what": "NumpyImagesDataset + DeviceBatchLoader: uint8 pool resident in HBM -> (lr, hr) float batches"}
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline()
    if world > 1:
        torch.distributed.barrier()
    if rank == 0 and args.full:
        detail = args.detail or os.path.join(ROOT, "gpurun_out" if os.path.isdir(os.path.join(ROOT, "gpurun_out")) else "", "bench_detail.json")
        try:
            with open(detail, "w") as f:
                json.dump(out, f, indent=1)
            out["detail_file"] = os.path.relpath(detail, ROOT)
        except OSError as exc:
            print("bench: could not write %s (%s)" % (detail, exc), file=sys.stderr)
    if rank == 0:
        print(lean_line(out), flush=True)
    if dist_mod.is_distributed():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
