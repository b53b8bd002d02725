"""Timing of the first-layer (3-channel) kernels of csrc/conv_c3.hip through the C ABI, at the shapes of the x3v iteration:
the D neck (batch 64, 3 -> 64 @384^2, bias + LeakyReLU), the G neck (batch 32, PReLU + pre-activation copy), the G head's data
gradient (the forward kernel on the NHWC-strided gradient image, transposed filter) and the three weight gradients (the G head's
with the roles swapped).  hipGraph-timed like tools/conv_bench.py; the rate is over the 64-channel tensor(s) a launch writes or
reads.  FSR_HIP_LIB selects the library (tools/build_variant.sh builds, ablation builds -DFSR_ABLC3=n included).
Usage on the GPU box: python tools/c3_bench.py [--dtypes x3,f16] [--tag NAME]"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
L = importlib.import_module("fast-srgan_amd._lib")
ops = importlib.import_module("fast-srgan_amd.ops")
from conv_bench import timeit  # noqa: E402

H = W = 384
ONE, ZERO = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="x3,f16")
    ap.add_argument("--tag", default=os.path.basename(L.LIB_PATH))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = L.lib()
    for cdn in args.dtypes.split(","):
        cd = ops.Compute(cdn)
        esz = 4 if cd.x3 else torch.empty((), dtype=cd.torch_dtype).element_size()
        wt = torch.randn(64, 3, 3, 3, device=dev) * 0.1
        wh = torch.randn(3, 64, 3, 3, device=dev) * 0.1
        bias = torch.randn(64, device=dev)
        slope = torch.tensor([0.25], device=dev)
        wpk, wpk_t = ops.packed_filter(cd, wt, ops.PACK_C3, 32), ops.packed_filter(cd, wh, ops.PACK_C3T, 32)
        for name, n in (("D neck b64", 64), ("G neck b32", 32), ("G head b32", 32)):
            head = name.startswith("G head")
            prelu = name.startswith("G neck")
            if head:      # the 3-channel gradient image is NHWC, viewed as (N, 3, H, W)
                img = torch.randn(n, H, W, 3, device=dev)
                strides = (H * W * 3, 1, W * 3, 3)
            else:
                img = torch.randn(n, 3, H, W, device=dev)
                strides = tuple(img.stride())
            out = ops._empty((n, H, W, 64), cd.torch_dtype, dev)
            pre = ops._empty_like(out) if prelu else None
            act = L.ACT_NONE if head else (L.ACT_PRELU if prelu else L.ACT_LEAKY)

            def fwd():
                L.check(lib.fsr_conv3x3_c3_fwd(cd.code, img.data_ptr(), *strides, n, H, W, *ONE, *ZERO, (wpk_t if head else wpk).data_ptr(),
                                               None if head else bias.data_ptr(), act, 0.2, ops._p(slope if prelu else None), 64, out.data_ptr(),
                                               ops._p(pre), None, ops._stream()), "fsr_conv3x3_c3_fwd")

            dz = ops.to_storage(cd, torch.randn(n, H, W, 64, device=dev))
            if cd.x3:
                dz = ops._aligned(dz)
            dw = torch.zeros((3, 64, 3, 3) if head else (64, 3, 3, 3), device=dev)
            db = None if head else torch.zeros(64, device=dev)
            ws = ops._workspace(lib.fsr_conv3x3_c3_wgrad_workspace(n, H, W, 64), dev)

            def wgrad():
                L.check(lib.fsr_conv3x3_c3_wgrad(cd.code, img.data_ptr(), *strides, n, H, W, *ONE, *ZERO, dz.data_ptr(), 64, dw.data_ptr(),
                                                 ops._p(db), ws.data_ptr(), 1 if head else 0, ops._stream()), "fsr_conv3x3_c3_wgrad")

            tensor = n * H * W * 64 * esz
            tf = timeit(fwd)
            tw = timeit(wgrad)        # (with its reduce kernel)
            print("%-14s %-4s %-11s fwd %7.1f us %5.2f TB/s | wgrad %7.1f us %5.2f TB/s" % (
                args.tag, cdn, name, tf * 1e3, tensor * (2 if prelu else 1) / tf / 1e9, tw * 1e3, tensor / tw / 1e9), flush=True)


if __name__ == "__main__":
    main()
