"""Timing of the first-layer (3-channel) kernels of csrc/conv_c3.hip through the C ABI, at the shapes of the x3v iteration:
the D neck (batch 64, 3 -> 64 @384^2, bias + LeakyReLU), the G neck (batch 32, PReLU + pre-activation copy), the G head's data
gradient (the forward kernel on the NHWC-strided gradient image, transposed filter) and the three weight gradients (the G head's
with the roles swapped).  hipGraph-timed like tools/conv_bench.py; the rate is over the 64-channel tensor(s) a launch writes or
reads.  FSR_HIP_LIB selects the library (tools/build_variant.sh builds, ablation builds -DFSR_ABLC3=n included).
--rows 16,32,64,auto times the forward at every strip height (FSR_C3_ROWS; auto = unset, the host's rule), --gneck96 adds the
G neck at the shape the iteration runs it at (96^2, batch 32: the "G neck b32" row is 384^2, a shape the step never uses),
--fwd-only skips the weight gradients, --s2d3 adds the discriminator's block-0 stride-2 data gradient (64 -> 64, dx 384^2,
batch 64 and 32) gated by the saved neck output and by its sign bits.
Usage on the GPU box: python tools/c3_bench.py [--dtypes x3,f16] [--tag NAME] [--rows ...] [--gneck96] [--fwd-only] [--s2d3]"""
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

ONE, ZERO = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="x3,f16")
    ap.add_argument("--tag", default=os.path.basename(L.LIB_PATH))
    ap.add_argument("--rows", default="auto")
    ap.add_argument("--gneck96", action="store_true")
    ap.add_argument("--fwd-only", action="store_true")
    ap.add_argument("--s2d3", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = L.lib()
    rows_list = args.rows.split(",")
    shapes = [("D neck b64", 64, 384), ("G neck b32", 32, 384), ("G head b32", 32, 384)] + ([("G neck 96^2", 32, 96)] if args.gneck96 else [])
    for cdn in args.dtypes.split(","):
        cd = ops.Compute(cdn)
        esz = 4 if cd.x3 else torch.empty((), dtype=cd.torch_dtype).element_size()
        wt = torch.randn(64, 3, 3, 3, device=dev) * 0.1
        wh = torch.randn(3, 64, 3, 3, device=dev) * 0.1
        bias = torch.randn(64, device=dev)
        slope = torch.tensor([0.25], device=dev)
        wpk, wpk_t = ops.packed_filter(cd, wt, ops.PACK_C3, 32), ops.packed_filter(cd, wh, ops.PACK_C3T, 32)
        for name, n, H in shapes:
            W = H
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

            dz = ops.to_storage(cd, torch.randn(n, H, W, 64, device=dev)) if not args.fwd_only else out
            if cd.x3:
                dz = ops._aligned(dz)
            dw = torch.zeros((3, 64, 3, 3) if head else (64, 3, 3, 3), device=dev)
            db = None if head else torch.zeros(64, device=dev)
            ws = ops._workspace(lib.fsr_conv3x3_c3_wgrad_workspace(n, H, W, 64), dev)

            def wgrad():
                L.check(lib.fsr_conv3x3_c3_wgrad(cd.code, img.data_ptr(), *strides, n, H, W, *ONE, *ZERO, dz.data_ptr(), 64, dw.data_ptr(),
                                                 ops._p(db), ws.data_ptr(), 1 if head else 0, ops._stream()), "fsr_conv3x3_c3_wgrad")

            tensor = n * H * W * 64 * esz
            for rows in rows_list:
                if rows == "auto":
                    os.environ.pop("FSR_C3_ROWS", None)
                else:
                    os.environ["FSR_C3_ROWS"] = rows       # (read by the library at every call)
                tag = args.tag if rows_list == ["auto"] else "%s/%s" % (args.tag, rows)
                tf = timeit(fwd)
                if args.fwd_only:
                    print("%-14s %-4s %-11s fwd %7.1f us %5.2f TB/s" % (tag, cdn, name, tf * 1e3, tensor * (2 if prelu else 1) / tf / 1e9), flush=True)
                    continue
                tw = timeit(wgrad)        # (with its reduce kernel)
                print("%-14s %-4s %-11s fwd %7.1f us %5.2f TB/s | wgrad %7.1f us %5.2f TB/s" % (
                    tag, cdn, name, tf * 1e3, tensor * (2 if prelu else 1) / tf / 1e9, tw * 1e3, tensor / tw / 1e9), flush=True)
            os.environ.pop("FSR_C3_ROWS", None)
        if args.s2d3 and (cd.x3 or cd.is16):
            s2d3_rows(args.tag, cd, cdn, esz, dev)


def s2d3_rows(tag, cd, cdn, esz, dev):
    """The discriminator's block-0 data gradient (conv_s2d3): dy 192^2 x 64 -> dx 384^2 x 64, LeakyReLU backward of the neck fused,
    the mask read as the saved neck output or as its sign bits.  TB/s over the gradient tensor written."""
    for n in (64, 32):
        dy = ops.to_storage(cd, torch.randn(n, 192, 192, 64, device=dev))
        y = ops.to_storage(cd, torch.randn(n, 384, 384, 64, device=dev))
        pos = (ops.from_storage(cd, y) > 0).view(n, 384, 384, 8, 8).to(torch.uint8)
        bits = (pos << torch.arange(8, device=dev, dtype=torch.uint8)).sum(-1, dtype=torch.uint8)
        del pos
        wpk = ops.packed_filter(cd, torch.randn(64, 64, 3, 3, device=dev) * 0.1, L.PACK_DGRAD, 64)
        for what, mask, isbits in (("tensor", y, False), ("bits", bits, True)):
            def run():
                ops.conv3x3_raw(cd, dy, wpk, 64, mode=L.CONV_DGRAD, out_hw=(384, 384), stride=2, dact_mask=mask, dact_slope=0.2, dact_bits=isbits)
            try:
                t = timeit(run)
                print("%-14s %-4s block-0 dgrad b%d, mask = %-6s %7.1f us %5.2f TB/s  %s" % (
                    tag, cdn, n, what, t * 1e3, n * 384 * 384 * 64 * esz / t / 1e9, ops._last_kernel()), flush=True)
            except L.FsrError as e:
                print("%-14s %-4s block-0 dgrad b%d, mask = %-6s not taken by this library (%s)" % (tag, cdn, n, what, str(e)[:60]), flush=True)
        del dy, y, bits


if __name__ == "__main__":
    main()
