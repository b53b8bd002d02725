"""Generator / Discriminator / VGG19 with the reference's nn.Module surface on MI355X kernels.

Drop-in for /root/reference/model.py: same class names, constructor arguments, submodule names and
therefore the same state_dict keys and shapes (the shipped models/model.pt loads unchanged), same
forward signatures ((N,3,H,W) float32 in; (N,3,4H,4W) / (N,1,H/16,W/16) float32 out).  The torch.nn
submodules are kept purely as PARAMETER CONTAINERS (and so that default initialisation draws the
same random numbers in the same order as the reference); their forward methods are never called.
All math runs through fast-srgan_amd.ops on NHWC activations in the module's compute dtype.

Extra constructor keyword (not in the reference): compute_dtype = "f16" (default since round 5; fp16 MFMA with
f32 accumulation, f32 parameters/statistics), "bf16" (bf16 MFMA), "x3" (split-bf16 operands, three bf16
MFMAs per product: the fast mode inside the reference's 1e-3 fp32 tolerance on outputs and losses), "f32" (exact-f32 MFMA),
or "x3v" (round 6: the x3 mode for the TRAINED networks -- Generator, Discriminator -- and fp16 for the FROZEN perceptual
network, whose only product is the content loss: that loss stays within 2e-4 of the fp32 reference's, the gradients are as far
from float64 as pure x3's, and the iteration is 31 % faster; `split_compute_dtype`).
"""
import os
import warnings

import torch

from . import _lib as L
from . import ops

_DEFAULT_DTYPE = os.environ.get("FSR_COMPUTE_DTYPE", "f16")


def split_compute_dtype(name):
    """(dtype of the trained networks, dtype of the frozen perceptual network) of a compute-mode name.  Every mode but "x3v" uses
    one dtype for both; "x3v" = x3 for Generator / Discriminator, fp16 for VGG19 (its backward then runs under the Trainer's
    dynamic loss scale, like the fp16 mode's)."""
    if name == "x3v":
        return "x3", "f16"
    return name, name


class UpSamplingBlock(torch.nn.Module):
    """model.py:26-40: conv 3x3 C->4C (bias) -> PixelShuffle(2) -> PReLU, one fused kernel here."""

    def __init__(self, config):
        super().__init__()
        self.conv = torch.nn.Conv2d(config.n_filters, config.n_filters * 4, kernel_size=3, padding=1)
        self.phase_shift = torch.nn.PixelShuffle(upscale_factor=2)
        self.relu = torch.nn.PReLU()


class ResidualBlock(torch.nn.Module):
    """model.py:43-69."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = torch.nn.InstanceNorm2d(out_channels)
        self.relu1 = torch.nn.PReLU()
        self.conv2 = torch.nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = torch.nn.InstanceNorm2d(out_channels)


class Generator(torch.nn.Module):
    """model.py:72-117.  `config.n_upsample` (default 2, i.e. 4x) is an extension for BASELINE cfg #5."""

    def __init__(self, config, compute_dtype=None):
        super().__init__()
        nf = config.n_filters
        self.compute = ops.Compute(split_compute_dtype(compute_dtype or _DEFAULT_DTYPE)[0])
        if nf % self.compute.cpad:
            raise ValueError("n_filters=%d must be a multiple of %d in %s mode" % (nf, self.compute.cpad, self.compute.name))
        self.neck = torch.nn.Sequential(torch.nn.Conv2d(3, nf, kernel_size=3, padding=1), torch.nn.PReLU())
        self.stem = torch.nn.Sequential(*[ResidualBlock(nf, nf) for _ in range(config.n_layers)])
        self.bottleneck = torch.nn.Sequential(
            torch.nn.Conv2d(nf, nf, kernel_size=3, padding=1, bias=False), torch.nn.InstanceNorm2d(nf))
        self.upsampling = torch.nn.Sequential(*[UpSamplingBlock(config) for _ in range(getattr(config, "n_upsample", 2))])
        self.head = torch.nn.Sequential(torch.nn.Conv2d(nf, 3, kernel_size=3, padding=1), torch.nn.Tanh())
        cd = self.compute
        self._cfg_neck = ops.ConvCfg(cd, act=L.ACT_PRELU, image_in=True)
        self._cfg_in = ops.ConvCfg(cd, stats=True)
        # first convolution of a residual block: also hands out aliases of its input for the skip connection(s), whose
        # gradients its data-gradient launch adds in the epilogue (no autograd accumulation kernels on the block inputs)
        self._cfg_in_skip = ops.ConvCfg(cd, stats=True, n_alias=1)
        self._cfg_in_skip2 = ops.ConvCfg(cd, stats=True, n_alias=2)
        self._cfg_up = ops.ConvCfg(cd, act=L.ACT_PRELU, pixel_shuffle=True)
        self._cfg_head = ops.ConvCfg(cd, tanh_head=True)
        self._cfg_head_u8 = ops.ConvCfg(cd, tanh_head=True, u8_head=True)
        self._cfg_head_i420 = {}      # (matrix code, full range, nv12) -> ConvCfg of the I420 / NV12 head

    def _native_size(self, h, w, out_size):
        """True when out_size (None or (out_h, out_w)) is the size the network produces for an h x w input."""
        if out_size is None:
            return True
        s = 2 ** len(self.upsampling)
        oh, ow = out_size
        if int(oh) != oh or int(ow) != ow or oh <= 0 or ow <= 0:
            raise ValueError("out_size must be (out_h, out_w) of positive integers, got %r" % (out_size,))
        return (int(oh), int(ow)) == (s * h, s * w)

    def forward_u8(self, frames, out_size=None, bands=None, ensemble=False):
        """Inference on raw frames (inference.py:47-57 without the host round trips): (N,H,W,3) uint8 in, (N,4H,4W,3) uint8
        out.  The [-1,1] mapping (:48) is one small kernel in front of the neck; the head's epilogue applies :53-56
        ((y+1)/2 * 255, truncating cast) and stores bytes -- a 720p frame leaves the device as 2.8 MB instead of 11 MB of
        floats.
        out_size = (out_h, out_w): frames of that size instead -- the float head output goes through one fused kernel, the
        antialiased bicubic resize with the same truncating cast (ops.resample_image).  None or the native size:
        the head's own epilogue, as before.
        bands = R: the tail runs in row bands of R core rows (`_tail_banded`): the same bytes, and batches up to
        max_batch(h, w, bands=True).
        ensemble = True: the self-ensemble ("+") frames -- the mean of the float head outputs of the 8 flipped / transposed inputs,
        each brought back to the frame's orientation, through the same cast (`_ensemble`)."""
        with torch.no_grad():
            if ensemble:
                native = self._native_size(frames.shape[1], frames.shape[2], out_size)
                mean = self._ensemble(frames, "u8" if native else "f32", bands)
                return mean if native else ops.resample_image(mean.permute(0, 2, 3, 1), int(out_size[0]), int(out_size[1]), "u8")
            if self._native_size(frames.shape[1], frames.shape[2], out_size):
                return self._forward(ops.u8_to_image(frames), self._cfg_head_u8, bands)
            t = self._forward(ops.u8_to_image(frames), self._cfg_head, bands)
            return ops.resample_image(t.permute(0, 2, 3, 1), int(out_size[0]), int(out_size[1]), "u8")

    def max_batch(self, h, w, bands=False):
        """Largest batch of h x w frames the convolution kernels can index: every launcher refuses tensors of 2^31 or more elements,
        and the largest activation of a batch holds n * h * w * n_filters * 4 ** n_upsample of them (the output of the last
        up-sampling convolution, before its pixel shuffle; with no up-sampling block, the neck's output).  0: a single frame is too large.
        bands=True: the limit of a forward with `bands` set.  That tensor then only ever exists one group of row
        bands at a time, and the largest whole-frame tensors are the input of the last up-sampling convolution
        (n * h * w * n_filters * 4 ** (n_upsample - 1)) and the float head output (n * h * w * 3 * 4 ** n_upsample).  With no
        up-sampling block there is no tail to band and the limit is the same."""
        nf, u = self.neck[0].out_channels, len(self.upsampling)
        per = nf * 4 ** u
        if bands and u >= 1:
            per = max(nf * 4 ** (u - 1), 3 * 4 ** u)
        return (2 ** 31 - 1) // (int(h) * int(w) * per)

    def _head_i420(self, matrix, full_range, nv12=False):
        """ConvCfg of the head whose epilogue stores 8-bit I420 planes (nv12: the NV12 payload) in (matrix, full_range), made on first
        use."""
        key = (ops.yuv_matrix_code(matrix), int(full_range), int(bool(nv12)))
        cfg = self._cfg_head_i420.get(key)
        if cfg is None:
            cfg = self._cfg_head_i420[key] = ops.ConvCfg(self.compute, tanh_head=True, i420_head=key)
        return cfg

    def forward_yuv(self, frames, h, w, chroma="420", out_chroma=None, siting=None, matrix="bt601", full_range=False, out_matrix=None,
                    out_full_range=None, out_size=None, depth=8, out_depth=None, bands=None, layout="planar", out_layout=None):
        """Video inference on planar YUV frames: (N, bytes) uint8 payloads of h x w (odd sizes legal) in, (N, bytes) uint8 payloads of
        (s h) x (s w) out, s = 2 ** n_upsample.  `chroma` in, `out_chroma` out ("420", "422" or "444", independent of each other;
        out_chroma defaults to chroma): payloads are ops.yuv_frame_bytes(h, w, chroma, depth) bytes in and
        ops.yuv_frame_bytes(out_h, out_w, out_chroma, out_depth) out.  The input is decoded on the device (matrix "bt601" / "bt709",
        limited or full range, chroma `siting` "jpeg" or "mpeg2"; None: "mpeg2" for 4:2:2 input, what Y4M's C422 declares, "jpeg" for
        4:2:0; 4:4:4 has none) into the generator's [-1, 1] RGB; the float tanh output is encoded to Y, Cb, Cr planes (4:2:0: C420jpeg
        siting) in the output pair (out_matrix, out_full_range), which defaults to the input's.  The colour contract is DESIGN.md §6c.
        depth / out_depth (8..16; out_depth defaults to depth): bits per sample of the input / output payloads -- above 8 a sample is 2
        bytes, little-endian (Y4M's C420p<depth> and its kin).  The two are independent (8 -> 10 keeps the precision of the float head
        that 8-bit codes throw away).
        out_size = (out_h, out_w): payloads of that size instead (both even for "420", an even width for "422", any extents for "444").
        Routes: 8-bit "420" output at the native size (out_size None or that size) is the head's own I420 epilogue.  Anything else is the
        float head followed by ops.image_to_yuv at the native size, or by one fused kernel that resizes (antialiased bicubic) and encodes
        (ops.resample_image) -- "444" on a 4:2:0 source keeps the chroma the head has computed.
        bands = R: the tail in row bands of R core rows, as forward_u8's; the encode / resize kernels run on the whole frame after it.
        layout / out_layout ("planar" or "nv12", independent of each other; out_layout defaults to layout): "nv12" is the semi-planar
        payload of 4:2:0 frames -- Y, then one plane of (Cb, Cr) pairs; NV12 at depth 8, P010 / P012 / P016 above.  The
        routes are the same: the head's epilogue stores the NV12 payload itself (FSR_OUT_NV12), the encode and resize kernels have
        their semi-planar forms."""
        ops.chroma_code(chroma)
        out_chroma = chroma if out_chroma is None else out_chroma
        ops.chroma_code(out_chroma)
        out_layout = layout if out_layout is None else out_layout
        ops.layout_code(layout, chroma)
        ops.layout_code(out_layout, out_chroma)
        depth = ops.check_depth(depth)
        out_depth = depth if out_depth is None else ops.check_depth(out_depth)
        out_matrix = out_matrix or matrix
        out_full = bool(full_range if out_full_range is None else out_full_range)
        native = self._native_size(h, w, out_size)
        epilogue = out_chroma == "420" and native and out_depth == 8
        cfg = self._head_i420(out_matrix, out_full, out_layout == "nv12") if epilogue else self._cfg_head
        with torch.no_grad():
            y = self._forward(ops.yuv_to_image(frames, h, w, chroma, siting, matrix, full_range, depth, layout), cfg, bands)
            if epilogue:
                return y
            t = y.permute(0, 2, 3, 1)
            if native:
                return ops.image_to_yuv(t, out_chroma, out_matrix, out_full, out_depth, out_layout)
            return ops.resample_image(t, int(out_size[0]), int(out_size[1]), "i420", out_matrix, out_full, out_depth, out_chroma, out_layout)

    def forward_yuv420(self, frames, h, w, siting="jpeg", matrix="bt601", full_range=False, out_matrix=None, out_full_range=None,
                       out_size=None, depth=8, out_depth=None, bands=None):
        """forward_yuv for I420 payloads in and out."""
        return self.forward_yuv(frames, h, w, "420", "420", siting, matrix, full_range, out_matrix, out_full_range, out_size, depth, out_depth,
                                bands)

    def forward(self, x, bands=None, ensemble=False):
        """bands = R (inference only: raises while gradients are enabled): the tail in row bands of R core rows.
        ensemble = True (inference only, likewise): the self-ensemble mean of the 8 members' float outputs."""
        if ensemble:
            return self._ensemble(x.permute(0, 2, 3, 1).contiguous(), "f32", bands)
        return self._forward(x, self._cfg_head, bands)

    def _ensemble(self, frames, kind, bands=None):
        """Self-ensemble of (N,H,W,3) frames, uint8 or float32 NHWC in [-1,1]: per orientation group (codes 0..3 keep
        H x W, codes 4..7 are W x H) one member-input launch (ops.dihedral_members), the float head on the 4N members -- in chunks of
        whole members when 4N exceeds max_batch; InstanceNorm statistics are per image, so the chunking changes no bit -- and one
        accumulate launch per chunk (ops.dihedral_accumulate), which adds the outputs through the inverse transforms in code order.
        kind "u8": uint8 (N,sH,sW,3); "f32": the float32 (N,3,sH,sW) view of an NHWC buffer."""
        if torch.is_grad_enabled():
            raise L.FsrError("ensemble: self-ensemble inference has no gradient; call it under torch.no_grad()")
        n, h, w, _ = frames.shape
        s = 2 ** len(self.upsampling)
        per = min(4, self.max_batch(h, w, bands is not None) // n)      # members per forward (max_batch is symmetric in h and w)
        if per < 1:
            raise ValueError("ensemble: a batch of %d frames of %dx%d is too large for the convolution kernels (max_batch = %d)"
                             % (n, w, h, self.max_batch(h, w, bands is not None)))
        acc = torch.empty((n, s * h, s * w, 3), dtype=torch.float32, device=frames.device)
        out = None
        for g0 in (0, 4):
            x = ops.dihedral_members(frames, g0, g0 + 3)
            for k0 in range(g0, g0 + 4, per):
                k1 = min(k0 + per, g0 + 4) - 1
                y = self._forward(x[(k0 - g0) * n:(k1 - g0 + 1) * n], self._cfg_head, bands)
                out = ops.dihedral_accumulate(y.permute(0, 2, 3, 1), k0, k1, acc, kind)
        return out

    def _forward(self, x, cfg_head, bands=None):
        m = self._body(x)
        if bands is None or not len(self.upsampling):      # (no up-sampling block: there is no tail to band)
            return self._tail(m, cfg_head)
        return self._tail_banded(m, cfg_head, bands)

    def _tail(self, m, cfg_head):
        """The last up-sampling block and the head on m = `_body`'s output: local 3x3 arithmetic, no statistic."""
        for up in list(self.upsampling)[-1:]:
            m, _ = ops.conv3x3(m, up.conv.weight, up.conv.bias, up.relu.weight, self._cfg_up)
        out, _ = ops.conv3x3(m, self.head[0].weight, self.head[0].bias, None, cfg_head)                # :117
        return out

    def _tail_banded(self, m, cfg_head, bands):
        """`_tail` in row bands: the windows of ops.tail_windows over the rows of m, of all images, gathered into
        groups of G windows, each group run through `_tail` as a batch of its own, and the core rows of every result copied to
        their place in the whole output.  The output of the last up-sampling convolution -- the largest tensor of a forward --
        exists one group at a time; G is the largest group the convolution kernels index."""
        R = int(bands)
        if isinstance(bands, bool) or R != bands or R < 1:
            raise ValueError("bands must be None or the number of core rows per band (an integer >= 1), got %r" % (bands,))
        if torch.is_grad_enabled():
            raise L.FsrError("bands: the banded tail is inference-only (it has no gradient); call it under torch.no_grad()")
        n, H2, W2, c = m.shape
        wins = ops.tail_windows(H2, R)
        if len(wins) == 1:
            return self._tail(m, cfg_head)
        Hw, total = R + 2 * ops.TAIL_HALO, n * len(wins)
        cup = self.upsampling[-1].conv.out_channels
        G = min(total, 65535, (2 ** 31 - 1) // (Hw * W2 * max(cup, 12)))
        if G < 1:
            raise ValueError("bands=%d: one window of %d x %d is too large for the convolution kernels; use fewer rows" % (R, Hw, W2))
        es, oh, ow = m.element_size(), 2 * H2, 2 * W2
        if cfg_head.i420_head:      # (N, bytes) uint8: the Y plane, then Cb and Cr at a quarter of its size each
            out = torch.empty((n, oh * ow * 3 // 2), dtype=torch.uint8, device=m.device)
            # (row bytes, output rows per row of m, plane offset in a window's payload, plane offset in a frame's)
            planes = [(ow, 2, 0, 0), (W2, 1, 4 * Hw * W2, oh * ow), (W2, 1, 5 * Hw * W2, oh * ow + H2 * W2)]
            if cfg_head.i420_head[2]:       # NV12 (`_head_i420`'s key): one chroma plane of ow bytes per row (Cb, Cr pairs)
                planes = [(ow, 2, 0, 0), (ow, 1, 4 * Hw * W2, oh * ow)]
            src_pitch, dst_pitch = 6 * Hw * W2, oh * ow * 3 // 2
        else:                       # (N, 4H, 4W, 3) uint8 or float32
            out = torch.empty((n, oh, ow, 3), dtype=torch.uint8 if cfg_head.u8_head else torch.float32, device=m.device)
            row = ow * 3 * out.element_size()
            planes = [(row, 2, 0, 0)]
            src_pitch, dst_pitch = 2 * Hw * row, oh * row
        group = ops._empty((G, Hw, W2, c), m.dtype, m.device)
        for first in range(0, total, G):
            g = min(G, total - first)
            win = group[:g]
            ops.copy_rows(m, win, H2 * W2 * c * es, Hw * W2 * c * es, W2 * c * es, first, g, H2, R)
            y = self._tail(win, cfg_head)
            y = y if (cfg_head.i420_head or cfg_head.u8_head) else y.permute(0, 2, 3, 1)      # the float head's NHWC buffer
            for row, mul, src_off, dst_off in planes:
                ops.copy_rows(y, out, src_pitch, dst_pitch, row, first, g, H2, R, mul, True, src_off, dst_off)
        return out if (cfg_head.i420_head or cfg_head.u8_head) else out.permute(0, 3, 1, 2)

    def _body(self, x):
        """Everything in front of the last up-sampling block: the whole-frame part (InstanceNorm statistics are per image)."""
        cd = self.compute
        r, _ = ops.conv3x3(x, self.neck[0].weight, self.neck[0].bias, self.neck[1].weight, self._cfg_neck)  # :113
        y = r
        training = torch.is_grad_enabled()
        for k, blk in enumerate(self.stem):                                                             # :114
            if training:
                # block 0's input r also feeds the long skip of :115: two aliases
                t, st, *skip = ops.conv3x3(y, blk.conv1.weight, None, None, self._cfg_in_skip2 if k == 0 else self._cfg_in_skip)
            else:
                t, st = ops.conv3x3(y, blk.conv1.weight, None, None, self._cfg_in)
                skip = [y, y]
            if k == 0:
                r = skip[1]
            t = ops.instnorm_act(t, st, None, blk.relu1.weight, cd, L.ACT_PRELU)
            u, st = ops.conv3x3(t, blk.conv2.weight, None, None, self._cfg_in)
            y = ops.instnorm_act(u, st, skip[0], None, cd)
        u, st = ops.conv3x3(y, self.bottleneck[0].weight, None, None, self._cfg_in)                      # :115
        y = ops.instnorm_act(u, st, r, None, cd)
        for up in list(self.upsampling)[:-1]:                                                              # :116
            y, _ = ops.conv3x3(y, up.conv.weight, up.conv.bias, up.relu.weight, self._cfg_up)
        return y


class GraphedGenerator:
    """Inference replay of a Generator at one fixed input shape as a single hipGraph launch.

    At batch 1 a 720p frame is ~45 kernels of 10-30 us each, so eager inference is bound by host launch overhead;
    one graph launch per frame removes it.  `gg = GraphedGenerator(model, example)`; `y = gg(x)` copies x into the
    static input, replays, and returns the static output tensor (clone it if it must outlive the next call)."""

    def __init__(self, model, example, warmup=2):
        self.model = model.eval()
        self.x = example.detach().clone()
        with torch.no_grad():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(warmup):
                    self.model(self.x)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.y = self.model(self.x)

    def __call__(self, x):
        self.x.copy_(x, non_blocking=True)
        self.graph.replay()
        return self.y


class SimpleBlock(torch.nn.Module):
    """model.py:120-136 (LeakyReLU with the default slope 0.01)."""

    def __init__(self, in_channels, out_channels, stride):
        super().__init__()
        self.conv = torch.nn.Conv2d(in_channels, out_channels, kernel_size=3, padding=1, stride=stride, bias=False)
        self.bn = torch.nn.InstanceNorm2d(out_channels)
        self.act = torch.nn.LeakyReLU()
        self.stride = stride


class Discriminator(torch.nn.Module):
    """model.py:139-193.  config.n_layers is accepted and ignored, as in the reference."""

    def __init__(self, config, compute_dtype=None):
        super().__init__()
        self.config = config
        nf = config.n_filters
        self.compute = ops.Compute(split_compute_dtype(compute_dtype or _DEFAULT_DTYPE)[0])
        if nf % self.compute.cpad:
            raise ValueError("n_filters=%d must be a multiple of %d in %s mode" % (nf, self.compute.cpad, self.compute.name))
        self.neck = torch.nn.Sequential(torch.nn.Conv2d(3, nf, kernel_size=3, padding=1), torch.nn.LeakyReLU(negative_slope=0.2))
        self.stem = torch.nn.Sequential(
            SimpleBlock(nf, nf, 2), SimpleBlock(nf, nf * 2, 1), SimpleBlock(nf * 2, nf * 2, 2),
            SimpleBlock(nf * 2, nf * 4, 1), SimpleBlock(nf * 4, nf * 4, 2), SimpleBlock(nf * 4, nf * 8, 1),
            SimpleBlock(nf * 8, nf * 8, 2),
            torch.nn.Conv2d(nf * 8, 1, kernel_size=1, padding=0, stride=1))
        cd = self.compute
        # the neck's LeakyReLU(0.2) backward is applied by stem.0's data-gradient epilogue (mask = the neck output it
        # saved as its input); the neck then only needs the column sums of that gradient for its bias
        self._cfg_neck = ops.ConvCfg(cd, act=L.ACT_LEAKY, slope=0.2, image_in=True, act_bwd_by_consumer=True, emit_signs=True)
        self._cfg_s = {1: ops.ConvCfg(cd, stride=1, stats=True), 2: ops.ConvCfg(cd, stride=2, stats=True)}
        self._cfg_s0 = ops.ConvCfg(cd, stride=2, stats=True, input_act_bwd=0.2)

    def forward(self, x):
        cd = self.compute
        y, _ = ops.conv3x3(x, self.neck[0].weight, self.neck[0].bias, None, self._cfg_neck)
        for i, blk in enumerate(list(self.stem)[:7]):
            u, st = ops.conv3x3(y, blk.conv.weight, None, None, self._cfg_s0 if i == 0 else self._cfg_s[blk.stride])
            y = ops.instnorm_act(u, st, None, None, cd, L.ACT_LEAKY, 0.01)
        return ops.conv1x1_to_logits(y, self.stem[7].weight, self.stem[7].bias, cd)


_VGG_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"]


class VGG19(torch.nn.Module):
    """model.py:5-23: ImageNet normalisation + torchvision vgg19.features[:34], frozen.

    torchvision is not a dependency: the feature stack is rebuilt with the same module indices (state_dict
    keys vgg.{0,2,5,...,32}.{weight,bias} + buffers mean/std).  Pretrained weights: pass `weights=` a path
    to torchvision's vgg19 checkpoint (keys features.N.*) or set FSR_VGG19_WEIGHTS; when torchvision is
    installed and has the ImageNet file cached, it is used as the reference does (model.py:8).  WITHOUT ImageNet
    weights the constructor RAISES: a perceptual loss against random features trains a silently different model.
    The random stand-in (torchvision's weights=None initialisation, kaiming-normal fan_out) is an explicit opt-in
    for tests and benchmarks: `seed=` or `allow_random=True`.
    """

    def __init__(self, weights=None, compute_dtype=None, width_div=1, seed=None, allow_random=False):
        super().__init__()
        self.compute = ops.Compute(split_compute_dtype(compute_dtype or _DEFAULT_DTYPE)[1])
        layers, cin = [], 3
        for v in _VGG_CFG:
            if v == "M":
                layers.append(torch.nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [torch.nn.Conv2d(cin, v // width_div, kernel_size=3, padding=1), torch.nn.ReLU(inplace=True)]
                cin = v // width_div
        self.vgg = torch.nn.Sequential(*layers)[:34]
        path = weights or os.environ.get("FSR_VGG19_WEIGHTS")
        if path:
            sd = torch.load(path, map_location="cpu")
            self.vgg.load_state_dict({k[len("features."):]: v for k, v in sd.items()
                                      if k.startswith("features.") and int(k.split(".")[1]) < 34})
        elif seed is not None or allow_random:
            if seed is None:
                warnings.warn("VGG19: random kaiming-normal stand-in instead of the ImageNet weights (allow_random=True)")
            gen = torch.Generator().manual_seed(1234 if seed is None else seed)
            for m in self.vgg:
                if isinstance(m, torch.nn.Conv2d):
                    with torch.no_grad():
                        std = (2.0 / (m.out_channels * 9)) ** 0.5
                        m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * std)
                        m.bias.zero_()
        else:
            try:        # what the reference does (model.py:8); needs torchvision and its cached / downloadable checkpoint
                from torchvision.models.vgg import VGG19_Weights, vgg19
                tv = vgg19(weights=VGG19_Weights.IMAGENET1K_V1).features[:34]
                self.vgg.load_state_dict(tv.state_dict())
            except Exception as exc:
                raise L.FsrError(
                    "VGG19: no ImageNet weights. Pass weights=<torchvision vgg19 checkpoint>, set FSR_VGG19_WEIGHTS or the "
                    "config key training.vgg19_weights; the reference uses vgg19(IMAGENET1K_V1) (model.py:8) and a random "
                    "feature network would silently train a different model. For tests / benchmarks opt in to the random "
                    "stand-in with VGG19(seed=...) or training.allow_random_vgg=true. (torchvision: %s)" % (exc,)) from exc
        for param in self.vgg.parameters():
            param.requires_grad = False
        self.register_buffer("mean", torch.tensor([0.485, 0.456, 0.406], requires_grad=False).view(1, 3, 1, 1))
        self.register_buffer("std", torch.tensor([0.229, 0.224, 0.225], requires_grad=False).view(1, 3, 1, 1))
        mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
        cd = self.compute
        # (x+1)/2 then (x-mean)/std  ==  x * 1/(2 std) + (0.5-mean)/std, fused into the first conv's input load
        scale, shift = tuple(0.5 / s for s in std), tuple((0.5 - m) / s for m, s in zip(mean, std))
        # Backward plan (the stack is frozen, so no bias gradients exist): every conv's ReLU backward is applied
        # by its CONSUMER -- the next conv's data-gradient epilogue (mask = its own saved input) or the pool's
        # backward -- instead of a separate elementwise pass; only the last conv handles its own.
        mods = list(self.vgg)
        convs = [i for i, m in enumerate(mods) if isinstance(m, torch.nn.Conv2d)]
        self._plan = []
        for k, i in enumerate(convs):
            prev_is_relu = k > 0 and isinstance(mods[i - 1], torch.nn.ReLU)
            nxt = mods[i + 2] if i + 2 < len(mods) else None
            self._plan.append((i, ops.ConvCfg(cd, act=L.ACT_RELU, image_in=(k == 0), in_scale=scale if k == 0 else (1.0, 1.0, 1.0),
                                              in_shift=shift if k == 0 else (0.0, 0.0, 0.0),
                                              input_act_bwd=0.0 if prev_is_relu else None,
                                              act_bwd_by_consumer=nxt is not None),
                               isinstance(nxt, torch.nn.MaxPool2d)))

    @property
    def _plan_pooled(self):
        plan = getattr(self, "_plan_pooled_cache", None)
        if plan is None:
            plan = {k: ops.ConvCfg(self.compute, act=L.ACT_RELU, pool_after=True) for k, (_, _, pool) in enumerate(self._plan) if pool}
            self._plan_pooled_cache = plan
        return plan

    def features_nhwc(self, x):
        y = x
        # no gradient wanted (the target features of trainer.py:191, inference): conv + ReLU + MaxPool2d as ONE kernel in the
        # 16-bit modes -- the full-resolution tensor, which only the pool's backward would read, is never written
        fuse_pool = (not torch.is_grad_enabled()) and self.compute.name != "f32"
        for k, (i, cfg, pool_after) in enumerate(self._plan):
            m = self.vgg[i]
            if pool_after and fuse_pool and not cfg.image_in and y.shape[1] % 2 == 0 and y.shape[2] % 2 == 0:
                y, _ = ops.conv3x3(y, m.weight, m.bias, None, self._plan_pooled[k])
                continue
            y, _ = ops.conv3x3(y, m.weight, m.bias, None, cfg)
            if pool_after:
                y = ops.maxpool2(y, self.compute, relu_mask=True)
        return y

    def forward(self, x):
        """(N,3,H,W) in [-1,1] -> (N,512,H/16,W/16) feature VALUES (model.py:20-23).  In the x3 mode the kernels' output is a
        float32 container of bf16 hi / lo planes: it is decoded here (and the cotangent re-encoded on the way back), so
        callers of V(x) never see the container; the trainer's loss kernels take features_nhwc() directly."""
        return ops.values(self.compute, self.features_nhwc(x)).permute(0, 3, 1, 2)
