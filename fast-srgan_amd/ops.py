"""Operators of the Fast-SRGAN hot path: torch.autograd.Functions over the C ABI of libfsr_hip.so.

Layout contract: activations are NHWC tensors (N,H,W,C) in the compute dtype
(torch.bfloat16 for FSR_BF16, torch.float32 for FSR_F32) with C a multiple of CPAD (32 / 16);
3-channel images enter and leave as float32 NCHW-shaped tensors of any strides.  Every kernel is
enqueued on torch's current stream; nothing here synchronises, allocates pinned memory or falls
back to a torch implementation of the math.
"""
import ctypes
import math
import os
import weakref

import numpy as np
import torch

from . import _lib as L

_DT = {"f32": (L.FSR_F32, torch.float32, 16), "bf16": (L.FSR_BF16, torch.bfloat16, 32), "f16": (L.FSR_F16, torch.float16, 32),
       "x3": (L.FSR_X3, torch.float32, 32)}


class Compute:
    """Compute mode of a module: 'bf16' / 'f16' (16-bit MFMA, f32 accumulate; f16 = BASELINE configs[4]), 'f32' (exact-f32
    MFMA, the parity mode) or 'x3' (split bf16: every value is the pair hi = bf16(v), lo = bf16(v - hi), every product three
    bf16 MFMAs into one f32 accumulator -- the fast mode inside the reference's fp32 tolerance).

    An x3 activation lives in a float32 tensor of its logical shape (same bytes: per pixel and 32-channel group 64 bytes of
    hi, then 64 bytes of lo; include/fsr_hip.h).  The container is NOT float data: torch arithmetic on it is meaningless, only
    copies (cat along the batch, clone, slicing whole pixels) are legal -- x3_encode / x3_decode convert."""

    def __init__(self, name="f16"):
        if name not in _DT:
            raise ValueError("compute dtype must be 'bf16', 'f16', 'x3' or 'f32', got %r" % (name,))
        self.name = name
        self.code, self.torch_dtype, self.cpad = _DT[name]
        self.x3 = name == "x3"
        # packed filters: the MFMA operand type; an x3 pack holds 2 x K bf16 elements per row ([w_hi | w_lo] per 32 channels)
        self.pack_dtype = torch.bfloat16 if self.x3 else self.torch_dtype
        self.pack_kmul = 2 if self.x3 else 1
        self.is16 = name in ("bf16", "f16")     # plain 16-bit storage: the kernels that exist for those modes only

    def pad(self, c):
        return (c + self.cpad - 1) // self.cpad * self.cpad


def _empty(shape, dtype, device):
    """Activation storage.  x3 kernels address hi / lo halves through 128-byte blocks of the tensor: the GPU allocator hands out
    512-byte aligned blocks, the CPU allocator of the emulated test runs only 64-byte aligned ones."""
    if torch.device(device).type != "cpu":
        return torch.empty(shape, dtype=dtype, device=device)
    n = 1
    for d in shape:
        n *= d
    es = torch.empty((), dtype=dtype).element_size()
    flat = torch.empty(n + 128 // es, dtype=dtype, device=device)
    off = (-flat.data_ptr() % 128) // es
    return flat[off:off + n].view(shape)


def _empty_like(t):
    return _empty(tuple(t.shape), t.dtype, t.device)


def _aligned(t):
    """t, or a 128-byte aligned copy of it (CPU tensors of the emulated runs only)."""
    if t is None or t.is_cuda or t.data_ptr() % 128 == 0:
        return t
    out = _empty_like(t)
    out.copy_(t)
    return out


def x3_encode(x):
    """float32 (..., C) tensor, C % 32 == 0 -> its x3 storage form (a float32 tensor of the same shape; see Compute)."""
    if x.dtype != torch.float32 or x.shape[-1] % 32:
        raise ValueError("x3_encode expects a float32 tensor with a multiple of 32 channels, got %s %s" % (x.dtype, tuple(x.shape)))
    x = x.contiguous()
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    g = x.shape[-1] // 32
    pair = torch.stack([hi.view(*x.shape[:-1], g, 32), lo.view(*x.shape[:-1], g, 32)], dim=-2)     # (..., g, 2, 32) bf16
    out = _empty(tuple(x.shape), torch.float32, x.device)
    out.view(torch.bfloat16).view(*x.shape[:-1], g, 2, 32).copy_(pair)
    return out


def x3_decode(t):
    """x3 storage (float32 container, (..., C)) -> the float32 values hi + lo."""
    t = t.contiguous()
    g = t.shape[-1] // 32
    pair = t.view(torch.bfloat16).view(*t.shape[:-1], g, 2, 32).float()
    return (pair[..., 0, :] + pair[..., 1, :]).reshape(t.shape)


def to_storage(cd, x):
    """float32 NHWC values -> the storage tensor of compute mode `cd` (tests, module boundaries)."""
    return x3_encode(x.float()) if cd.x3 else x.to(cd.torch_dtype)


def from_storage(cd, t):
    """storage tensor of compute mode `cd` -> float32 values."""
    return x3_decode(t) if cd.x3 else t.float()


class _StorageBoundaryFn(torch.autograd.Function):
    """Storage tensor of a compute mode -> float32 VALUES, differentiable: the backward re-encodes the cotangent.  The boundary
    every public forward() crosses before handing a tensor to arbitrary torch code -- an x3 activation is a float32 CONTAINER of
    interleaved bf16 hi / lo planes, and any torch arithmetic on it (autograd accumulation, .float(), a channel-wise cat)
    would be silent garbage (round-5 advisor, model.py:279)."""

    @staticmethod
    def forward(ctx, cd, t):
        ctx.cd = cd
        return from_storage(cd, t)

    @staticmethod
    def backward(ctx, g):
        return None, to_storage(ctx.cd, g.contiguous())


def values(cd, t):
    """float32 values of a storage tensor, with the cotangent routed back in storage form (module boundaries)."""
    return _StorageBoundaryFn.apply(cd, t) if cd.x3 else t


def add(cd, a, b):
    """a + b of two activation tensors (fsr_add): what autograd's accumulation would do, legal for x3 containers."""
    _check_dev(a, b)
    a, b = _aligned(a.contiguous()), _aligned(b.contiguous())
    out = _empty_like(a)
    L.check(L.lib().fsr_add(cd.code, _p(a), _p(b), _p(out), a.numel(), _stream()), "fsr_add")
    return out


def _stream():
    if L.is_emulation():
        return None
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _check_dev(*ts):
    for t in ts:
        if t is not None and not L.is_emulation() and not t.is_cuda:
            raise L.FsrError("fast-srgan_amd operators run on the GPU only (got a %s tensor); there is no CPU path" % t.device)


# ---------------------------------------------------------------------------------- packed filters
_pack_cache = {}   # id(weight) -> (weakref to the weight, {(mode, dtype, k_pad): (version, packed tensor)})


PACK_C3 = "c3"   # packed_filter mode of the first-layer (image-input) kernels
PACK_C3T = "c3t"  # ... of the head conv's data gradient run as a first-layer forward (transposed, tap-flipped filter)


class FilterSpec:
    """A filter handed to conv3x3_raw as (weight, pack mode, k_pad) instead of a packed tensor: the launch then asks the
    library which pack layout the kernel it will dispatch reads (fsr_conv3x3_pack_block: the standard [9][rows][K] image or
    the stage-contiguous one of the 128..512-channel kernels) and packs -- cached per weight version -- accordingly."""

    __slots__ = ("weight", "mode", "k_pad")

    def __init__(self, weight, mode, k_pad):
        self.weight, self.mode, self.k_pad = weight, mode, k_pad


def packed_filter(cd, weight, mode, k_pad, lin=0):
    """[9][rows_pad][k_pad] image of an OIHW float weight (fsr_pack_conv3x3), cached per weight OBJECT and version.
    lin = 64 / 128: the stage-contiguous layout of that channel-block size instead (fsr_pack_conv3x3_lin).

    Entries die with the weight (weak reference), so a recycled id()/address can never serve a stale filter.

    The image of a (weight, mode, dtype, k_pad) lives in ONE buffer for the lifetime of the weight: a newer weight
    version is re-packed IN PLACE.  A captured hipGraph therefore bakes in addresses that stay valid, and the re-pack
    launches it contains (the optimizer step inside the graph bumps the version, so the next use re-packs) refresh
    exactly the memory the next replay reads -- no replay can see the filters of capture time."""
    ver = (weight._version, getattr(weight, "_fsr_epoch", 0), weight.data_ptr())
    slot = _pack_cache.get(id(weight))
    if slot is None or slot[0]() is not weight:
        wid = id(weight)
        slot = (weakref.ref(weight, lambda _r, wid=wid: _pack_cache.pop(wid, None)), {})
        _pack_cache[wid] = slot
    key = (mode, cd.code, k_pad, lin)
    hit = slot[1].get(key)
    if hit is not None and hit[0] == ver:
        return hit[1]
    cout, cin = weight.shape[0], weight.shape[1]
    fwd = mode in (L.PACK_FWD, L.PACK_FWD_PS)
    rows = cout if fwd else cin
    rows_pad = (rows + 15) // 16 * 16
    w = weight.detach()
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.float().contiguous()
    _check_dev(w)
    if mode == PACK_C3T:
        numel = ((cin + 15) // 16 * 16) * 32
    elif mode == PACK_C3:
        numel = ((cout + 15) // 16 * 16) * 32
    else:
        numel = 9 * (rows if lin else rows_pad) * k_pad * cd.pack_kmul
    out = hit[1] if (hit is not None and hit[1].device == w.device) else None
    if out is None:
        # (x3: the first-layer kernels compute in exact f32 on x3 storage, their filter image is float)
        out = torch.empty(numel, dtype=torch.float32 if (cd.x3 and mode in (PACK_C3, PACK_C3T)) else cd.pack_dtype, device=w.device)
    if lin:
        if k_pad != (cin if fwd else cout) or mode in (PACK_C3, PACK_C3T):
            raise L.FsrError("the stage-contiguous filter pack has no padding")
        L.check(L.lib().fsr_pack_conv3x3_lin(cd.code, mode, _p(w), cout, cin, lin, _p(out), _stream()), "fsr_pack_conv3x3_lin")
    elif mode == PACK_C3:     # first-layer kernels: [rows_pad][32]
        L.check(L.lib().fsr_pack_conv3x3_c3(cd.code, _p(w), cout, _p(out), 0, _stream()), "fsr_pack_conv3x3_c3")
    elif mode == PACK_C3T:  # head conv [3][cin][3][3]: rows = its input channels
        L.check(L.lib().fsr_pack_conv3x3_c3(cd.code, _p(w), cin, _p(out), 1, _stream()), "fsr_pack_conv3x3_c3")
    else:
        L.check(L.lib().fsr_pack_conv3x3(cd.code, mode, _p(w), cout, cin, k_pad, _p(out), _stream()), "fsr_pack_conv3x3")
    slot[1][key] = (ver, out)
    return out


_ws = {}
_const = {}


class ZeroPool:
    """Per-iteration arena of zero-initialised float32 scratch (InstanceNorm statistics, reduction outputs, bias /
    PReLU gradients, loss accumulators): ONE memset per iteration instead of ~160 tiny fill kernels.  `reset()` at the
    start of an iteration re-zeroes the arena and rewinds it; tensors carved from it live until the next reset."""

    def __init__(self, device, nfloats=4 << 20):
        self.buf = torch.zeros(nfloats, dtype=torch.float32, device=device)
        self.off = 0
        self.active = False

    def reset(self):
        if self.off:
            self.buf[:self.off].zero_()
        self.off = 0

    def take(self, shape):
        n = 1
        for d in shape:
            n *= d
        n4 = (n + 3) // 4 * 4          # keep 16-byte alignment for vector loads
        if self.off + n4 > self.buf.numel():
            return None
        t = self.buf[self.off:self.off + n].view(shape)
        self.off += n4
        return t


_zero_pool = {}


def zero_pool_reset(device):
    """Called by the Trainer at the start of every iteration (creates the arena on first use)."""
    key = str(device)
    pool = _zero_pool.get(key)
    if pool is None:
        pool = _zero_pool[key] = ZeroPool(device)
    pool.reset()
    pool.active = True


def zero_pool_end(device):
    """End of the iteration: later allocations (inference, metrics, captured inference graphs) must get their own
    zero-filled memory -- the arena is only re-zeroed by the next `zero_pool_reset`."""
    pool = _zero_pool.get(str(device))
    if pool is not None:
        pool.active = False


def _zeros(shape, device):
    pool = _zero_pool.get(str(device))
    if pool is not None and pool.active:
        t = pool.take(tuple(shape))
        if t is not None:
            return t
    return torch.zeros(shape, dtype=torch.float32, device=device)


def _assigned(shape, device):
    """float32 scratch for a result the kernels ASSIGN (the order-fixed second-level reduce overwrites it): from the
    iteration's arena when one is open, else uninitialised -- inference then launches no fill kernel per statistics tensor."""
    pool = _zero_pool.get(str(device))
    if pool is not None and pool.active:
        t = pool.take(tuple(shape))
        if t is not None:
            return t
    return torch.empty(shape, dtype=torch.float32, device=device)


def _const_vec(values, device):
    """Small float constant vector on `device`, uploaded once (no host-to-device copies inside captured steps)."""
    key = (tuple(values), str(device))
    t = _const.get(key)
    if t is None:
        t = torch.tensor(values, dtype=torch.float32, device=device)
        _const[key] = t
    return t

USE_LIN_PACK = os.environ.get("FSR_PACK_LIN", "1") != "0"   # A/B switch: 0 = every launch reads the standard filter pack
# A/B switch: 0 = activation-gradient masks are always the saved tensors.  Only conv_s2d3 reads the packed bits, so switching
# that kernel off (FSR_S2D3=0) switches the bits off with it instead of leaving a mask no kernel takes
USE_SIGN_BITS = os.environ.get("FSR_SIGN_BITS", "1") != "0" and os.environ.get("FSR_S2D3", "1") != "0"
_pack_block_memo = {}     # (descriptor fields, optional-tensor mask) -> block size: the dispatch is deterministic per shape
_DISPATCH_ENV = ("FSR_PERSIST_CUS", "FSR_T3_ROWS", "FSR_S2D3", "FSR_T3N_G3", "FSR_CONV_STAGE", "FSR_CONV64_S2FWD",
                 "FSR_PACK_LIN")   # every switch the conv dispatch reads (csrc: getenv) + the Python-side ones
USE_POOL_ARGMAX = os.environ.get("FSR_POOL_ARGMAX", "1") != "0"   # A/B switch: 0 = the pool backward re-reads its input and output
USE_C3_KERNELS = True   # tests flip this to compare the first-layer kernels with the padded-tensor path

# bench.py sets this to a list to collect (start_event, end_event, algorithmic_flops, algorithmic_bytes, kernel name, kind)
# per convolution launch; kind is "fwd", "dgrad" or "wgrad"
PROFILE_CONV = None


def _last_kernel():
    name = L.lib().fsr_last_kernel()
    return name.decode() if name else "?"


_ws_retired = []    # outgrown scratch buffers that a captured hipGraph may still address: never freed
_capture_seen = {}  # (device, stream) -> the current buffer was handed out during a stream capture


def _workspace(nbytes, device):
    """Scratch (split-K partials of the weight gradients, per-workgroup partials of the reductions), one buffer per
    (device, stream): launches on different streams may overlap; on one stream a producer and the kernel that finishes
    its partials are enqueued back to back by the same C-ABI call, so the next call may reuse the buffer."""
    key = (str(device), _stream())
    buf = _ws.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        if buf is not None:
            # a captured hipGraph may have baked this address in: keep the buffer alive only in that case (a buffer that no
            # capture can have seen is simply dropped, so a run of growing requests does not pile up)
            if _capture_seen.get(key):
                _ws_retired.append(buf)
            # geometric growth (O(log) reallocations, not one per larger request), capped: doubling below 64 MB, +25 % above --
            # a retired generation stays pinned for as long as a captured graph may address it, so large split-K workspaces
            # must not double their way to hundreds of MB each
            old = buf.numel() * 4
            nbytes = max(nbytes, 2 * old if old < (64 << 20) else old + old // 4)
        buf = torch.empty((max(nbytes, 1 << 20) + 3) // 4, dtype=torch.float32, device=device)
        _ws[key] = buf
        _capture_seen[key] = False
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        _capture_seen[key] = True
    return buf


# ---------------------------------------------------------------------------------- weight gradients on their own stream
# A weight gradient depends only on (x, dz) and nothing downstream depends on it before the optimizer step, so it can run
# beside the data-gradient chain instead of inside it.  `wgrad_stream_begin(device)` (the trainer, per iteration) turns
# this on; Conv3x3Fn.backward then launches its weight gradient on the side stream after an event of the producing
# stream, and `wgrad_stream_join()` makes the current stream wait for all of them (before gradients are reduced / used).
# The tensors a queued launch reads are kept referenced until the join, so the caching allocator cannot hand their
# memory to later work on the producing stream.
#
# Layers of ONE shape (the generator's 64 -> 64 stem: 17 of them, model.py:62-80) are additionally DEFERRED while the
# trainer's iteration is open: backward only queues (x, dz, arena) and the join launches the whole group as one
# fsr_conv3x3_wgrad_grouped call -- the layers share one launch's workgroups (15 slabs each instead of 256), so the
# split-K partials shrink 17x and 17 reduce launches become one.
_wgrad_state = {"stream": None, "active": False, "refs": [], "group": False, "pending": {}}
USE_WGRAD_STREAM = os.environ.get("FSR_WGRAD_STREAM", "1") != "0"
USE_WGRAD_GROUP = os.environ.get("FSR_WGRAD_GROUP", "1") != "0"
WGRAD_GROUP_MAX = 32


def wgrad_stream_begin(device):
    _wgrad_state["group"] = USE_WGRAD_GROUP
    if not USE_WGRAD_STREAM or L.is_emulation() or not torch.cuda.is_available():
        return
    if _wgrad_state["stream"] is None:
        _wgrad_state["stream"] = torch.cuda.Stream(device=device)
    _wgrad_state["active"] = True


def _wgrad_defer(cd, xin, dz, cout, cin, cfg, arena):
    """Queue a weight gradient for the grouped launch; False if this layer is not of the groupable class."""
    st = _wgrad_state
    if not st["group"] or cfg.stride != 1 or cfg.pixel_shuffle or cd.x3:
        return False
    if not (cout == cin == 64 and xin.shape[3] == 64 and dz.shape[3] == 64):
        return False
    st["pending"].setdefault((cd.code, tuple(xin.shape), str(xin.device)), []).append((cd, xin, dz, arena))
    return True


def _wgrad_flush():
    st = _wgrad_state
    pending, st["pending"] = st["pending"], {}
    lib = L.lib()
    for (_code, shape, _dev), items in pending.items():
        for i0 in range(0, len(items), WGRAD_GROUP_MAX):
            grp = items[i0:i0 + WGRAD_GROUP_MAX]
            cd, x0, dz0, _ = grp[0]
            if len(grp) == 1:
                with _on_wgrad_stream(x0, dz0):
                    conv3x3_wgrad_raw(cd, x0, dz0, 64, 64, 1, out=grp[0][3])
                continue
            n, ih, iw, _c = shape
            d = L.WgradDesc(cd.code, n, ih, iw, 64, 64, ih, iw, 64, 64, 1, 0)
            need = lib.fsr_conv3x3_wgrad_grouped_workspace(ctypes.byref(d), len(grp))
            if need == 0:
                L.check(-2, "fsr_conv3x3_wgrad_grouped_workspace")
            arr = ctypes.c_void_p * len(grp)
            xs, dys, dws = arr(*[_p(g[1]) for g in grp]), arr(*[_p(g[2]) for g in grp]), arr(*[_p(g[3]) for g in grp])
            with _on_wgrad_stream(*[t for g in grp for t in (g[1], g[2])]):
                prof = PROFILE_CONV
                if prof is not None:
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record()
                L.check(lib.fsr_conv3x3_wgrad_grouped(ctypes.byref(d), len(grp), xs, dys, dws, _p(_workspace(need, x0.device)),
                                                      _stream()), "fsr_conv3x3_wgrad_grouped")
                if prof is not None:
                    ev1.record()
                    nbytes = len(grp) * (2 * x0.numel() * x0.element_size() + 64 * 64 * 9 * 4)
                    prof.append((ev0, ev1, len(grp) * 2.0 * n * ih * iw * 64 * 64 * 9, nbytes, "conv_wgrad_kernel", "wgrad"))


def wgrad_stream_join():
    st = _wgrad_state
    if st["pending"]:
        _wgrad_flush()
    if st["active"] and st["refs"]:
        torch.cuda.current_stream().wait_stream(st["stream"])
    st["refs"] = []


def wgrad_stream_end():
    # an iteration that ran to its optimizer steps has joined (and flushed) already; what is still queued here belongs to an
    # iteration that raised: drop it instead of launching on its tensors
    _wgrad_state["pending"] = {}
    wgrad_stream_join()
    _wgrad_state["active"] = False
    _wgrad_state["group"] = False


class _on_wgrad_stream:
    """with _on_wgrad_stream(tensors): the body's launches go to the weight-gradient stream (if active), ordered after
    everything queued so far on the current stream."""

    def __init__(self, *tensors):
        self.tensors = tensors
        self.ctx = None

    def __enter__(self):
        st = _wgrad_state
        if st["active"] and self.tensors[0].is_cuda:
            st["stream"].wait_stream(torch.cuda.current_stream())
            st["refs"].append(self.tensors)
            self.ctx = torch.cuda.stream(st["stream"])
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


# ---------------------------------------------------------------------------------- raw launches
def conv3x3_raw(cd, x, wpk, cout, *, mode=L.CONV_FWD, out_hw=None, stride=1, bias=None, act=L.ACT_NONE, slope=0.0,
                prelu=None, oscale=None, pixel_shuffle=False, in_pixel_shuffled=False, out_f32=False, want_stats=False,
                want_preact=False, alg_k=None, dact_mask=None, dact_slope=0.0, out_u8=False, pool2=False, dact_add=False, dact_bits=False,
                out_i420=None):
    """One fsr_conv3x3 launch.  x: (N,IH,IW,Cin) [or its depth-to-space form when in_pixel_shuffled].
    out_u8 (tanh heads): the output is the finished uint8 HWC image of inference.py:53-56.
    out_i420 = (matrix, full_range) (3-channel tanh heads, even output extents): the output is (N, OH*OW*3/2) uint8, the I420
    planes of the RGB frame per image (FSR_OUT_I420).  A third element that is true -- (matrix, full_range, 1) --
    asks for the semi-planar payload instead (FSR_OUT_NV12): the same bytes, Cb and Cr interleaved in one plane.
    pool2 (no-grad passes): the output is MaxPool2d(2,2) of the activated result; the full-resolution tensor is never written.
    dact_add: `dact_mask` is ADDED to the result (the gradient of a skip connection) instead of gating it.
    dact_bits: `dact_mask` is the packed sign-bit tensor (N,OH,OW,Cout/8) uint8 of the producing layer's output (stride-2 data gradients)."""
    _check_dev(x)
    if cd.x3:
        x, dact_mask = _aligned(x), (_aligned(dact_mask) if (dact_mask is not None and not dact_bits) else dact_mask)
    n = x.shape[0]
    if in_pixel_shuffled:
        ih, iw, cin = x.shape[1] // 2, x.shape[2] // 2, x.shape[3] * 4
    else:
        ih, iw, cin = x.shape[1], x.shape[2], x.shape[3]
    if mode == L.CONV_FWD:
        oh, ow = (ih - 1) // stride + 1, (iw - 1) // stride + 1
    else:
        oh, ow = out_hw
    odt = torch.uint8 if (out_u8 or out_i420) else (torch.float32 if out_f32 else cd.torch_dtype)
    oshape = (n, 2 * oh, 2 * ow, cout // 4) if pixel_shuffle else ((n, oh // 2, ow // 2, cout) if pool2 else (n, oh, ow, cout))
    if out_i420:
        oshape = (n, oh * ow * 3 // 2)
    out = _empty(oshape, odt, x.device)
    pre = _empty(oshape, odt, x.device) if want_preact else None
    stats = _assigned((n, cout, 2), x.device) if want_stats else None
    okind = (L.OUT_NV12 if len(out_i420) > 2 and out_i420[2] else L.OUT_I420) if out_i420 else (L.OUT_U8 if out_u8 else int(out_f32))
    yuv = out_i420 or (0, 0)
    d = L.ConvDesc(cd.code, mode, n, ih, iw, cin, oh, ow, cout, stride, act, float(slope), int(pixel_shuffle),
                   int(in_pixel_shuffled), okind, int(pool2), 2 if dact_bits else int(bool(dact_add)), 0, int(yuv[0]), int(yuv[1]))
    if isinstance(wpk, FilterSpec):     # pack in the layout the kernel this launch dispatches reads
        opt = ((L.OPT_BIAS if bias is not None else 0) | (L.OPT_PRELU if prelu is not None else 0) | (L.OPT_OSCALE if oscale is not None else 0)
               | (L.OPT_MASK if dact_mask is not None else 0) | (L.OPT_PREACT if want_preact else 0) | (L.OPT_STATS if want_stats else 0))
        blk = 0
        if USE_LIN_PACK:
            # one ctypes call (a walk of the whole dispatch chain) per SHAPE, not per launch: eager paths (validation,
            # inference, f32 / x3 without graphs) otherwise pay it for every convolution
            # (the key carries everything the C-side dispatch reads besides the descriptor: the device -- its CU count sizes the
            # persistent grids --, the library in use and every dispatch switch of the environment; round-5 advisor)
            key = (tuple(getattr(d, f) for f, _ in d._fields_), opt, L.is_emulation(), str(x.device), L.LIB_PATH,
                   tuple(os.environ.get(v) for v in _DISPATCH_ENV))
            blk = _pack_block_memo.get(key)
            if blk is None:
                blk = L.lib().fsr_conv3x3_pack_block(ctypes.byref(d), opt)
                if blk < 0:
                    L.check(blk, "fsr_conv3x3_pack_block")
                _pack_block_memo[key] = blk
        d.pack_lin = blk
        wpk = packed_filter(cd, wpk.weight, wpk.mode, wpk.k_pad, lin=blk)
    scratch = _workspace(L.lib().fsr_conv3x3_scratch(ctypes.byref(d)), x.device) if want_stats else None
    prof = PROFILE_CONV
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    L.check(L.lib().fsr_conv3x3(ctypes.byref(d), _p(x), _p(wpk), _p(bias), _p(prelu), _p(oscale), _p(dact_mask),
                                float(dact_slope), _p(out), _p(pre), _p(stats), _p(scratch), _stream()), "fsr_conv3x3")
    if prof is not None:
        ev1.record()
        k = cin if alg_k is None else alg_k
        pix = oh * ow if mode == L.CONV_FWD else ih * iw      # dgrad: one MAC per forward MAC
        # every tensor the launch has to read or write once: input, output, filter, and the fused extras (activation-gradient
        # mask read, pre-activation copy written)
        nbytes = x.numel() * x.element_size() + out.numel() * out.element_size() + wpk.numel() * wpk.element_size()
        if dact_mask is not None:
            nbytes += dact_mask.numel() * dact_mask.element_size()
        if pre is not None:
            nbytes += pre.numel() * pre.element_size()
        prof.append((ev0, ev1, 2.0 * n * pix * cout * k * 9, nbytes, _last_kernel(), "fwd" if mode == L.CONV_FWD else "dgrad"))
    return out, pre, stats


def conv3x3_wgrad_raw(cd, x, dy, cout, cin, stride, dy_pixel_shuffled=False, out=None):
    """OIHW float weight gradient.  x (N,IH,IW,CinPad); dy (N,OH,OW,CoutPad) or its depth-to-space form."""
    if cd.x3:
        x, dy = _aligned(x), _aligned(dy)
    n, ih, iw, cin_pad = x.shape
    if dy_pixel_shuffled:
        oh, ow, cout_pad = dy.shape[1] // 2, dy.shape[2] // 2, dy.shape[3] * 4
    else:
        oh, ow, cout_pad = dy.shape[1], dy.shape[2], dy.shape[3]
    d = L.WgradDesc(cd.code, n, ih, iw, cin_pad, cin, oh, ow, cout_pad, cout, stride, int(dy_pixel_shuffled))
    need = L.lib().fsr_conv3x3_wgrad_workspace(ctypes.byref(d))
    if need == 0:
        L.check(-2, "fsr_conv3x3_wgrad_workspace")
    ws = _workspace(need, x.device)
    dw = out if out is not None else torch.zeros((cout, cin, 3, 3), dtype=torch.float32, device=x.device)
    prof = PROFILE_CONV
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    L.check(L.lib().fsr_conv3x3_wgrad(ctypes.byref(d), _p(x), _p(dy), _p(dw), _p(ws), _stream()), "fsr_conv3x3_wgrad")
    if prof is not None:
        ev1.record()
        nbytes = x.numel() * x.element_size() + dy.numel() * dy.element_size() + cout * cin * 9 * 4
        prof.append((ev0, ev1, 2.0 * n * oh * ow * cout * cin * 9, nbytes, "conv_wgrad_kernel", "wgrad"))
    return dw


def image_to_nhwc(cd, img, scale=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.0)):
    """(N,3,H,W) float32 of any strides -> zero-padded (N,H,W,CPAD) compute-dtype tensor."""
    _check_dev(img)
    if img.dtype != torch.float32:
        img = img.float()
    n, c, h, w = img.shape
    if c != 3:
        raise ValueError("expected a 3-channel image batch, got %s" % (tuple(img.shape),))
    out = _empty((n, h, w, cd.cpad), cd.torch_dtype, img.device)
    sn, sc, sh, sw = img.stride()
    L.check(L.lib().fsr_image_to_nhwc(cd.code, _p(img), sn, sc, sh, sw, n, h, w, scale[0], scale[1], scale[2], shift[0],
                                      shift[1], shift[2], _p(out), cd.cpad, _stream()), "fsr_image_to_nhwc")
    return out


# ---------------------------------------------------------------------------------- autograd: convolution
class ConvCfg:
    """Static description of one fused convolution (kept out of autograd's tensor arguments)."""

    def __init__(self, cd, *, stride=1, act=L.ACT_NONE, slope=0.0, pixel_shuffle=False, stats=False, image_in=False,
                 in_scale=(1.0, 1.0, 1.0), in_shift=(0.0, 0.0, 0.0), tanh_head=False, input_act_bwd=None,
                 act_bwd_by_consumer=False, u8_head=False, pool_after=False, n_alias=0, emit_signs=False, i420_head=None):
        # u8_head (inference only, with tanh_head): the head stores the finished uint8 HWC frame instead of float
        # i420_head = (matrix, full_range) (inference only, with tanh_head): the head stores the I420 planes of the frame;
        # (matrix, full_range, 1): the NV12 payload (one interleaved chroma plane)
        # input_act_bwd = slope: the data-gradient launch also applies the backward of the ReLU (0.0) / LeakyReLU
        #   that produced this conv's input (the mask is the saved input itself), so the tensor it returns is
        #   already the producer's pre-activation gradient;
        # act_bwd_by_consumer: the incoming gradient already went through this conv's own activation backward
        #   (its consumer -- a conv with input_act_bwd or a pool with relu_mask -- did it); a bias gradient, if
        #   needed, then costs one read pass (column sums) instead of the three passes of a separate act_bwd.
        self.input_act_bwd, self.act_bwd_by_consumer = input_act_bwd, act_bwd_by_consumer
        self.cd, self.stride, self.act, self.slope = cd, stride, act, slope
        self.pixel_shuffle, self.stats, self.image_in = pixel_shuffle, stats, image_in
        self.in_scale, self.in_shift, self.tanh_head = in_scale, in_shift, tanh_head
        self.u8_head = u8_head and tanh_head
        self.i420_head = i420_head if tanh_head else None
        # pool_after (no-grad passes only): the MaxPool2d(2,2) that follows this conv + ReLU is taken in the epilogue and
        # only the pooled tensor is stored (the full-resolution tensor is what a backward pass would need)
        self.pool_after = pool_after
        # n_alias (1 or 2): forward also returns that many ALIASES of its input for the caller's skip connections
        # (model.py:69, :115).  Their gradients come back to THIS function's backward, whose data-gradient launch adds the
        # first one in its epilogue (fsr_conv_desc.mask_is_addend): autograd has nothing left to accumulate on the block input.
        self.n_alias = n_alias
        # emit_signs (first-layer kernels, training, 16-bit and x3): the forward also writes the SIGN BITS of its output (N,H,W,Cout/8 uint8)
        # and hangs them on the output tensor (`_fsr_signs`); a stride-2 consumer with input_act_bwd then reads those -- a sixteenth
        # of the bytes -- as its activation-gradient mask instead of the tensor itself
        self.emit_signs = emit_signs


class Conv3x3Fn(torch.autograd.Function):
    """Conv2d(k=3,p=1) + bias + activation [+ PixelShuffle(2)] [+ InstanceNorm statistics].

    forward(x, weight, bias, prelu_weight, cfg) -> (out, stats)
      x      : NHWC activation, or (image_in) a float32 NCHW image batch of any strides
      out    : NHWC activation; (tanh_head) a float32 (N,3,H,W) view of the NHWC head output
      stats  : (N,Cout,2) float32 sums of the pre-activation, or an empty tensor
    """

    @staticmethod
    def forward(ctx, x, weight, bias, prelu, cfg, grad_on=True):
        # grad_on: torch.is_grad_enabled() at the call site (grad mode is always off INSIDE Function.forward, and
        # ctx.needs_input_grad reports the parameters' requires_grad even under no_grad): inference must not pay for the
        # tensors only a backward pass reads (the pre-activation copy of the PReLU layers)
        ctx.grad_on = grad_on
        cd = cfg.cd
        cout, cin = weight.shape[0], weight.shape[1]
        if (cfg.image_in and cfg.stride == 1 and cout % 16 == 0 and not (cfg.pixel_shuffle or cfg.stats or cfg.tanh_head)
                and USE_C3_KERNELS):
            return Conv3x3Fn._forward_c3(ctx, x, weight, bias, prelu, cfg)
        ctx.c3 = False
        # sign bits of the input (hung on it by the first-layer kernel that produced it): the stride-2 data gradient's mask
        ctx.in_signs = getattr(x, "_fsr_signs", None) if (cfg.input_act_bwd is not None and cfg.stride == 2 and (cd.is16 or cd.x3)) else None
        if cfg.image_in:
            xin = image_to_nhwc(cd, x, cfg.in_scale, cfg.in_shift)
        else:
            xin = x if x.is_contiguous() else x.contiguous()
            if xin.dtype != cd.torch_dtype:
                raise L.FsrError("activation dtype %s does not match the module's compute dtype %s" % (xin.dtype, cd.name))
        cin_pad = xin.shape[3]
        wpk = FilterSpec(weight, L.PACK_FWD_PS if cfg.pixel_shuffle else L.PACK_FWD, cin_pad)
        training = ctx.grad_on and any(ctx.needs_input_grad)
        if (cfg.u8_head or cfg.i420_head or cfg.pool_after) and training:
            raise L.FsrError("the uint8 / I420 head and fused max-pool epilogues are inference-only: they have no gradient")
        act = L.ACT_TANH if cfg.tanh_head else cfg.act
        want_pre = training and act == L.ACT_PRELU
        b32 = bias if bias is None or bias.dtype == torch.float32 else bias.float()
        out, pre, stats = conv3x3_raw(cd, xin, wpk, cout, stride=cfg.stride, bias=b32, act=act, slope=cfg.slope,
                                      prelu=prelu, pixel_shuffle=cfg.pixel_shuffle, out_f32=cfg.tanh_head,
                                      want_stats=cfg.stats, want_preact=want_pre, alg_k=cin, out_u8=cfg.u8_head,
                                      pool2=cfg.pool_after, out_i420=cfg.i420_head)
        ctx.cfg = cfg
        ctx.dims = (cout, cin, tuple(xin.shape))
        ctx.has_bias = bias is not None
        ctx.x_is_image = cfg.image_in
        saved_act = pre if want_pre else (out if act in (L.ACT_RELU, L.ACT_LEAKY, L.ACT_TANH) else None)
        ctx.save_for_backward(xin, weight, prelu, saved_act)
        if stats is None:
            stats = torch.empty(0, device=out.device)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)    # no zero-filled gradient tensor for the statistics output per backward call
        if cfg.u8_head or cfg.i420_head:
            return out, stats               # (N,H,W,3) uint8: already the frame layout inference.py:55 permutes to; I420: (N, bytes)
        if cfg.tanh_head:
            return out.permute(0, 3, 1, 2), stats
        if cfg.n_alias:
            if cfg.image_in or cfg.input_act_bwd is not None or cfg.pixel_shuffle or cfg.stride != 1:
                raise L.FsrError("skip aliases are for plain stride-1 convolutions on NHWC activations")
            return (out, stats) + tuple(xin.view_as(xin) for _ in range(cfg.n_alias))
        return out, stats

    @staticmethod
    def _forward_c3(ctx, x, weight, bias, prelu, cfg):
        """First layer straight from the (N,3,H,W) float image (fsr_conv3x3_c3_fwd): no padded NHWC copy."""
        cd = cfg.cd
        _check_dev(x)
        if x.dtype != torch.float32:
            x = x.float()
        n, c, h, w = x.shape
        if c != 3:
            raise ValueError("expected a 3-channel image batch, got %s" % (tuple(x.shape),))
        cout = weight.shape[0]
        wpk = packed_filter(cd, weight, PACK_C3, 32)
        training = ctx.grad_on and any(ctx.needs_input_grad)
        want_pre = training and cfg.act == L.ACT_PRELU
        b32 = bias if bias is None or bias.dtype == torch.float32 else bias.float()
        out = _empty((n, h, w, cout), cd.torch_dtype, x.device)
        pre = _empty_like(out) if want_pre else None
        signs = (torch.empty((n, h, w, cout // 8), dtype=torch.uint8, device=x.device)
                 if (cfg.emit_signs and USE_SIGN_BITS and training and (cd.is16 or cd.x3) and cout % 64 == 0) else None)
        sn, sc, sh, sw = x.stride()
        prof = PROFILE_CONV
        if prof is not None:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        L.check(L.lib().fsr_conv3x3_c3_fwd(cd.code, _p(x), sn, sc, sh, sw, n, h, w, *cfg.in_scale, *cfg.in_shift, _p(wpk),
                                           _p(b32), cfg.act, float(cfg.slope), _p(prelu), cout, _p(out), _p(pre), _p(signs), _stream()),
                "fsr_conv3x3_c3_fwd")
        if signs is not None:
            out._fsr_signs = signs
        if prof is not None:
            ev1.record()
            nbytes = x.numel() * 4 + out.numel() * out.element_size() * (2 if want_pre else 1) + wpk.numel() * wpk.element_size()
            prof.append((ev0, ev1, 2.0 * n * h * w * cout * 27, nbytes, "conv_c3_fwd_kernel", "fwd"))
        ctx.cfg = cfg
        ctx.c3 = True
        ctx.bias_param = bias
        ctx.dims = (cout, 3, (n, h, w, cd.cpad))
        ctx.has_bias = bias is not None
        ctx.x_is_image = True
        saved_act = pre if want_pre else (out if cfg.act in (L.ACT_RELU, L.ACT_LEAKY) else None)
        ctx.save_for_backward(x, weight, prelu, saved_act)
        stats = torch.empty(0, device=out.device)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)    # no zero-filled gradient tensor for the statistics output per backward call
        return out, stats

    @staticmethod
    def backward(ctx, g, _gstats, *g_alias):
        skips = [t for t in g_alias if t is not None]
        if g is None:       # (gradients are not materialised: only the statistics output -- or only a skip alias -- was used)
            dx = None
            for t in skips:
                dx = t if dx is None else add(ctx.cfg.cd, dx, t)
            return dx, None, None, None, None, None
        cfg, cd = ctx.cfg, ctx.cfg.cd
        xin, weight, prelu, saved = ctx.saved_tensors
        cout, cin, xshape = ctx.dims
        n, ih, iw, cin_pad = xshape
        lib, st = L.lib(), _stream()
        dbias = _zeros((cout,), xin.device) if ctx.has_bias else None
        dprelu = None
        act = L.ACT_TANH if cfg.tanh_head else cfg.act
        if cfg.tanh_head and USE_C3_KERNELS and cout == 3 and cin_pad % 16 == 0 and cin == cin_pad:
            return Conv3x3Fn._backward_head_c3(ctx, g)
        if cfg.tanh_head:
            # g: (N,3,H,W) float of any strides; saved: head output (N,H,W,3) float
            if g.dtype != torch.float32:
                g = g.float()
            _, _, h, w = g.shape
            dz = _empty((n, h, w, cd.cpad), cd.torch_dtype, xin.device)
            sn, sc, sh, sw = g.stride()
            L.check(lib.fsr_tanh_bwd_to_nhwc(cd.code, _p(g), sn, sc, sh, sw, _p(saved), n, h, w, _p(dz), cd.cpad, _p(dbias),
                                             _p(_workspace(lib.fsr_tanh_bwd_scratch(), xin.device)), st), "fsr_tanh_bwd_to_nhwc")
        else:
            g = g if g.is_contiguous() else g.contiguous()
            if cd.x3:
                g, saved = _aligned(g), _aligned(saved)
            # first-layer kernels with arena gradients: the weight-gradient launch also produces the bias gradient (a column
            # of ones in its padded K dimension), straight into the bias' arena slice
            bias_arena = getattr(getattr(ctx, "bias_param", None), "_fsr_grad", None) if ctx.c3 else None
            fused_dbias = (bias_arena is not None and cfg.act_bwd_by_consumer and ctx.needs_input_grad[1] and ctx.needs_input_grad[2]
                           and getattr(weight, "_fsr_grad", None) is not None)
            if cfg.act_bwd_by_consumer:
                dz = g          # already multiplied by this layer's act'() in the consumer's data-gradient epilogue
                if ctx.has_bias and ctx.needs_input_grad[2] and not fused_dbias:    # bias gradient: column sums of dz, one read pass
                    _, h, w, c = g.shape
                    scr = _workspace(lib.fsr_act_bwd_scratch(n, h, w, c, int(cfg.pixel_shuffle)), xin.device)
                    L.check(lib.fsr_act_bwd(cd.code, _p(g), None, L.ACT_NONE, 0.0, None, None, _p(dbias), None, _p(scr), n, h, w,
                                            c, int(cfg.pixel_shuffle), st), "fsr_act_bwd")
            elif act != L.ACT_NONE or ctx.has_bias:
                if act == L.ACT_PRELU:
                    dprelu = _zeros((1,), xin.device)
                dz = _empty_like(g)
                _, h, w, c = g.shape
                scr = _workspace(lib.fsr_act_bwd_scratch(n, h, w, c, int(cfg.pixel_shuffle)), xin.device)
                L.check(lib.fsr_act_bwd(cd.code, _p(g), _p(saved), act, float(cfg.slope), _p(prelu), _p(dz), _p(dbias),
                                        _p(dprelu), _p(scr), n, h, w, c, int(cfg.pixel_shuffle), st), "fsr_act_bwd")
            else:
                dz = g
        dx = None
        if ctx.needs_input_grad[0]:
            if ctx.x_is_image:
                wpk = packed_filter(cd, weight, L.PACK_DGRAD, dz.shape[3] * (4 if cfg.pixel_shuffle else 1))
                osc = _const_vec(cfg.in_scale, xin.device) if tuple(cfg.in_scale) != (1.0, 1.0, 1.0) else None
                dx, _, _ = conv3x3_raw(cd, dz, wpk, 3, mode=L.CONV_DGRAD, out_hw=(ih, iw), stride=cfg.stride, oscale=osc,
                                       out_f32=True, in_pixel_shuffled=cfg.pixel_shuffle, alg_k=cout)
                dx = dx.permute(0, 3, 1, 2)
            else:
                kpad = dz.shape[3] * (4 if cfg.pixel_shuffle else 1)
                wpk = FilterSpec(weight, L.PACK_DGRAD_PS if cfg.pixel_shuffle else L.PACK_DGRAD, kpad)
                mask = xin if cfg.input_act_bwd is not None else None
                bits = getattr(ctx, "in_signs", None) if (mask is not None and cin_pad % 64 == 0) else None
                if bits is not None:
                    mask = bits
                addend = None
                if skips:       # dL/dx = conv_dgrad(dz) + dL/d(skip): the first skip gradient rides in the launch's epilogue
                    addend = skips[0] if skips[0].is_contiguous() else skips[0].contiguous()
                dx, _, _ = conv3x3_raw(cd, dz, wpk, cin_pad, mode=L.CONV_DGRAD, out_hw=(ih, iw), stride=cfg.stride,
                                       in_pixel_shuffled=cfg.pixel_shuffle, alg_k=cout, dact_mask=addend if addend is not None else mask,
                                       dact_slope=cfg.input_act_bwd or 0.0, dact_add=addend is not None,
                                       dact_bits=(bits is not None and addend is None))
                for t in skips[1:]:
                    dx = add(cd, dx, t)
        dw = None
        if ctx.needs_input_grad[1]:
            arena = getattr(weight, "_fsr_grad", None)  # optim.ArenaAdamW: accumulate in place, hand autograd nothing

            def launch_wgrad():
                if ctx.c3:      # xin is the float image itself
                    out = arena if arena is not None else torch.zeros((cout, 3, 3, 3), dtype=torch.float32, device=xin.device)
                    need = lib.fsr_conv3x3_c3_wgrad_workspace(n, ih, iw, cout)
                    sn, sc, sh, sw = xin.stride()
                    L.check(lib.fsr_conv3x3_c3_wgrad(cd.code, _p(xin), sn, sc, sh, sw, n, ih, iw, *cfg.in_scale, *cfg.in_shift,
                                                     _p(dz), cout, _p(out), _p(bias_arena) if fused_dbias else None,
                                                     _p(_workspace(need, xin.device)), 0, _stream()),
                            "fsr_conv3x3_c3_wgrad")
                    return out
                return conv3x3_wgrad_raw(cd, xin, dz, cout, cin, cfg.stride, dy_pixel_shuffled=cfg.pixel_shuffle, out=arena)

            if arena is not None:   # nothing downstream reads the arena before the optimizer: own stream (see above)
                if ctx.c3 or not _wgrad_defer(cd, xin, dz, cout, cin, cfg, arena):
                    with _on_wgrad_stream(xin, dz):
                        launch_wgrad()
            else:
                dw = launch_wgrad()
            if arena is not None:
                dw = None
        db = dbias if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        if not cfg.tanh_head and ctx.c3 and fused_dbias:
            db = None       # accumulated in the arena by the weight-gradient launch
        dp = dprelu if (dprelu is not None and ctx.needs_input_grad[3]) else None
        return dx, dw, db, dp, None, None


def _head_backward_c3(ctx, g):
    """Backward of the head Conv2d(nf -> 3) + Tanh (model.py:102-110) on the first-layer kernels: dz = g (1 - y^2) is written
    as a 3-channel float image; the data gradient is the 3 -> nf convolution of that image with the transposed, tap-flipped
    filter (fsr_conv3x3_c3_fwd), the weight gradient the first-layer weight gradient with the roles of image and gradient
    swapped.  (The generic path pads dz to 32 channels: 10x the bytes for 3 channels of data.)"""
    cfg, cd = ctx.cfg, ctx.cfg.cd
    xin, weight, _prelu, saved = ctx.saved_tensors
    cout, cin, xshape = ctx.dims
    n, ih, iw, cin_pad = xshape
    lib, st = L.lib(), _stream()
    if g.dtype != torch.float32:
        g = g.float()
    if cd.x3:
        xin = _aligned(xin)
    dbias = _zeros((cout,), xin.device) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
    dz_img = torch.empty((n, ih, iw, 3), dtype=torch.float32, device=xin.device)
    sn, sc, sh, sw = g.stride()
    L.check(lib.fsr_tanh_bwd_image(_p(g), sn, sc, sh, sw, _p(saved), n, ih, iw, _p(dz_img), _p(dbias),
                                   _p(_workspace(lib.fsr_tanh_bwd_scratch(), xin.device)), st), "fsr_tanh_bwd_image")
    img_strides = (ih * iw * 3, 1, iw * 3, 3)     # the NHWC float image viewed as (N,3,H,W)
    one, zero = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    dx = None
    if ctx.needs_input_grad[0]:
        wpk = packed_filter(cd, weight, PACK_C3T, 32)
        dx = _empty((n, ih, iw, cin_pad), cd.torch_dtype, xin.device)
        prof = PROFILE_CONV
        if prof is not None:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        L.check(lib.fsr_conv3x3_c3_fwd(cd.code, _p(dz_img), *img_strides, n, ih, iw, *one, *zero, _p(wpk), None, L.ACT_NONE, 0.0, None,
                                       cin_pad, _p(dx), None, None, st), "fsr_conv3x3_c3_fwd")
        if prof is not None:
            ev1.record()
            prof.append((ev0, ev1, 2.0 * n * ih * iw * cin * 27, dz_img.numel() * 4 + dx.numel() * dx.element_size(), "conv_c3_fwd_kernel", "dgrad"))
    dw = None
    if ctx.needs_input_grad[1]:
        arena = getattr(weight, "_fsr_grad", None)

        def launch():
            out = arena if arena is not None else torch.zeros((cout, cin, 3, 3), dtype=torch.float32, device=xin.device)
            need = lib.fsr_conv3x3_c3_wgrad_workspace(n, ih, iw, cin_pad)
            L.check(lib.fsr_conv3x3_c3_wgrad(cd.code, _p(dz_img), *img_strides, n, ih, iw, *one, *zero, _p(xin), cin_pad, _p(out), None,
                                             _p(_workspace(need, xin.device)), 1, _stream()), "fsr_conv3x3_c3_wgrad")
            return out

        if arena is not None:
            with _on_wgrad_stream(xin, dz_img):
                launch()
        else:
            dw = launch()
    return dx, dw, dbias, None, None, None


Conv3x3Fn._backward_head_c3 = staticmethod(_head_backward_c3)


def conv3x3(x, weight, bias, prelu, cfg):
    return Conv3x3Fn.apply(x, weight, bias, prelu, cfg, torch.is_grad_enabled())


# ---------------------------------------------------------------------------------- autograd: InstanceNorm + act + residual
class InstNormActFn(torch.autograd.Function):
    """out = act(InstanceNorm(x)) + res, from the raw conv output and the statistics its epilogue made."""

    @staticmethod
    def forward(ctx, x, stats, res, prelu, cd, act, slope):
        _check_dev(x)
        n, h, w, c = x.shape
        if res is not None and not res.is_contiguous():
            res = res.contiguous()
        if cd.x3:
            x, res = _aligned(x), _aligned(res)
        out = _empty_like(x)
        L.check(L.lib().fsr_instnorm_act_fwd(cd.code, _p(x), _p(stats), _p(res), act, float(slope), _p(prelu), _p(out), n,
                                             h * w, c, _stream()), "fsr_instnorm_act_fwd")
        ctx.meta = (cd, act, slope, res is not None)
        ctx.save_for_backward(x, stats, prelu)
        return out

    @staticmethod
    def backward(ctx, g):
        cd, act, slope, has_res = ctx.meta
        x, stats, prelu = ctx.saved_tensors
        n, h, w, c = x.shape
        g = g if g.is_contiguous() else g.contiguous()
        if cd.x3:
            g = _aligned(g)
        lib, st = L.lib(), _stream()
        sums = _zeros((n, c, 2), x.device)
        dprelu = _zeros((1,), x.device) if act == L.ACT_PRELU else None
        scr = _workspace(lib.fsr_instnorm_act_bwd_scratch(n, h * w, c), x.device)
        L.check(lib.fsr_instnorm_act_bwd_reduce(cd.code, _p(g), _p(x), _p(stats), act, float(slope), _p(prelu), _p(sums),
                                                _p(dprelu), _p(scr), n, h * w, c, st), "fsr_instnorm_act_bwd_reduce")
        dx = _empty_like(x)
        L.check(lib.fsr_instnorm_act_bwd_apply(cd.code, _p(g), _p(x), _p(stats), _p(sums), act, float(slope), _p(prelu),
                                               _p(dx), n, h * w, c, st), "fsr_instnorm_act_bwd_apply")
        return dx, None, (g if has_res else None), dprelu, None, None, None


def instnorm_act(x, stats, res, prelu, cd, act=L.ACT_NONE, slope=0.0):
    return InstNormActFn.apply(x, stats, res, prelu, cd, act, slope)


# ---------------------------------------------------------------------------------- autograd: MaxPool2d(2,2)
class MaxPool2Fn(torch.autograd.Function):
    """relu_mask: backward also applies the backward of the ReLU that produced x (see ConvCfg.act_bwd_by_consumer).
    With gradients enabled the forward also writes one arg-max byte per pooled element (position of the maximum + its sign);
    the backward pass reads the pooled gradient and those bytes -- not the full-resolution input and the pooled output."""

    @staticmethod
    def forward(ctx, x, cd, relu_mask=False, grad_on=True):
        _check_dev(x)
        n, h, w, c = x.shape
        if cd.x3:
            x = _aligned(x)
        y = _empty((n, h // 2, w // 2, c), x.dtype, x.device)
        idx = torch.empty((n, h // 2, w // 2, c), dtype=torch.uint8, device=x.device) if (grad_on and USE_POOL_ARGMAX) else None
        L.check(L.lib().fsr_maxpool2_fwd(cd.code, _p(x), _p(y), _p(idx), n, h, w, c, _stream()), "fsr_maxpool2_fwd")
        ctx.cd, ctx.relu_mask, ctx.xshape = cd, relu_mask, tuple(x.shape)
        ctx.by_idx = idx is not None
        if idx is not None:
            ctx.save_for_backward(idx)
        else:
            ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, g):
        n, h, w, c = ctx.xshape
        g = g if g.is_contiguous() else g.contiguous()
        if ctx.cd.x3:
            g = _aligned(g)
        dx = _empty((n, h, w, c), g.dtype, g.device)
        if ctx.by_idx:
            (idx,) = ctx.saved_tensors
            L.check(L.lib().fsr_maxpool2_bwd_argmax(ctx.cd.code, _p(g), _p(idx), _p(dx), n, h, w, c, int(ctx.relu_mask), _stream()),
                    "fsr_maxpool2_bwd_argmax")
        else:
            x, y = ctx.saved_tensors
            L.check(L.lib().fsr_maxpool2_bwd(ctx.cd.code, _p(g), _p(x), _p(y), _p(dx), n, h, w, c, int(ctx.relu_mask), _stream()),
                    "fsr_maxpool2_bwd")
        return dx, None, None, None


def maxpool2(x, cd, relu_mask=False):
    return MaxPool2Fn.apply(x, cd, relu_mask, torch.is_grad_enabled())


# ---------------------------------------------------------------------------------- autograd: Conv2d(C -> 1, k=1)
class Conv1x1ToLogitsFn(torch.autograd.Function):
    """x (N,H,W,C) -> float32 logits (N,1,H,W) (model.py:184-186)."""

    @staticmethod
    def forward(ctx, x, weight, bias, cd):
        _check_dev(x)
        n, h, w, c = x.shape
        x = x if x.is_contiguous() else x.contiguous()
        if cd.x3:
            x = _aligned(x)
        wv = weight.detach().reshape(-1)
        logits = torch.empty((n, 1, h, w), dtype=torch.float32, device=x.device)
        L.check(L.lib().fsr_conv1x1_c1_fwd(cd.code, _p(x), _p(wv), _p(bias), _p(logits), n * h * w, c, _stream()),
                "fsr_conv1x1_c1_fwd")
        ctx.cd = cd
        ctx.save_for_backward(x, weight)
        return logits

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        n, h, w, c = x.shape
        g = g.contiguous().float()
        dx = _empty_like(x) if ctx.needs_input_grad[0] else None
        dw = _zeros(tuple(weight.shape), x.device)
        db = _zeros((1,), x.device)
        scr = _workspace(L.lib().fsr_conv1x1_c1_bwd_scratch(c), x.device)
        L.check(L.lib().fsr_conv1x1_c1_bwd(ctx.cd.code, _p(g), _p(x), _p(weight.detach().reshape(-1)), _p(dx), _p(dw), _p(db),
                                           _p(scr), n * h * w, c, _stream()), "fsr_conv1x1_c1_bwd")
        return dx, dw, db, None


def conv1x1_to_logits(x, weight, bias, cd):
    return Conv1x1ToLogitsFn.apply(x, weight, bias, cd)


# ---------------------------------------------------------------------------------- autograd: losses
class BCEWithLogitsFn(torch.autograd.Function):
    """torch.nn.BCEWithLogitsLoss() (mean) on float32 logits/targets (trainer.py:41)."""

    @staticmethod
    def forward(ctx, x, t):
        _check_dev(x, t)
        x = x.contiguous().float()
        t = t.contiguous().float()
        loss = _zeros((1,), x.device).view(())
        scr = _workspace(L.lib().fsr_loss_scratch(), x.device)
        L.check(L.lib().fsr_bce_logits_fwd(_p(x), _p(t), _p(loss), _p(scr), x.numel(), _stream()), "fsr_bce_logits_fwd")
        ctx.save_for_backward(x, t)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, t = ctx.saved_tensors
        g = g.contiguous().float()
        dx = torch.empty_like(x)
        L.check(L.lib().fsr_bce_logits_bwd(_p(x), _p(t), _p(g), _p(dx), x.numel(), _stream()), "fsr_bce_logits_bwd")
        return dx, None


def _is_dense(t):
    """True when t's elements tile its storage without gaps or overlap (e.g. a permuted contiguous tensor)."""
    pairs = sorted((st, sz) for st, sz in zip(t.stride(), t.shape) if sz > 1)
    expect = 1
    for st, sz in pairs:
        if st != expect:
            return False
        expect *= sz
    return True


class SmoothL1Fn(torch.autograd.Function):
    """torch.nn.SmoothL1Loss() (beta 1, mean) (trainer.py:43); the second argument is the target."""

    @staticmethod
    def forward(ctx, a, b, x3=False):
        _check_dev(a, b)
        if a.dtype != b.dtype or a.shape != b.shape:
            raise L.FsrError("SmoothL1: operands must share dtype and shape")
        if not (a.stride() == b.stride() and _is_dense(a)):  # elementwise: any shared dense layout will do
            a, b = a.contiguous(), b.contiguous()
        code = {torch.bfloat16: L.FSR_BF16, torch.float16: L.FSR_F16, torch.float32: L.FSR_F32}.get(a.dtype)
        if code is None:
            raise L.FsrError("SmoothL1: unsupported dtype %s" % a.dtype)
        if x3:      # x3 containers are float32 tensors: the caller says what they hold
            if a.dtype != torch.float32:
                raise L.FsrError("SmoothL1: x3 operands live in float32 containers")
            code = L.FSR_X3
            a, b = _aligned(a), _aligned(b)
        loss = _zeros((1,), a.device).view(())
        scr = _workspace(L.lib().fsr_loss_scratch(), a.device)
        L.check(L.lib().fsr_smooth_l1_fwd(code, _p(a), _p(b), _p(loss), _p(scr), a.numel(), _stream()), "fsr_smooth_l1_fwd")
        ctx.code = code
        ctx.save_for_backward(a, b)
        return loss

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous().float()
        da = _empty_like(a) if ctx.code == L.FSR_X3 else torch.empty_like(a)
        L.check(L.lib().fsr_smooth_l1_bwd(ctx.code, _p(a), _p(b), _p(g), _p(da), a.numel(), _stream()), "fsr_smooth_l1_bwd")
        return da, None, None


ELEM_LOSS_KINDS = {"l1": L.LOSS_L1, "smooth_l1": L.LOSS_SMOOTH_L1, "charbonnier": L.LOSS_CHARBONNIER, "mse": L.LOSS_MSE}


def _elem_loss_check(a, b, kind, eps):
    """The operand and parameter checks of elem_loss; returns (kind code, eps as a float)."""
    code = ELEM_LOSS_KINDS.get(kind)
    if code is None:
        raise ValueError("elem_loss: unknown kind %r (known: %s)" % (kind, ", ".join(ELEM_LOSS_KINDS)))
    eps = float(eps)
    if code == L.LOSS_CHARBONNIER and not (0.0 < eps < float("inf")):
        raise ValueError("elem_loss: Charbonnier's eps must be positive and finite, got %r" % (eps,))
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise L.FsrError("elem_loss: operands must be float32 (the head stores and the loaders hand out float32), got %s and %s"
                         % (a.dtype, b.dtype))
    if a.dim() != 4 or a.shape != b.shape:
        raise L.FsrError("elem_loss: operands must be two (N,C,H,W) tensors of one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if b.requires_grad:
        raise L.FsrError("elem_loss: the second operand is the target and gets no gradient, but it requires one")
    return code, eps


class ElemLossFn(torch.autograd.Function):
    """mean psi(a - b) over two float32 (N,C,H,W) tensors of ANY strides, psi by `code` (fsr_elem_loss_fwd / _bwd); b is the target."""

    @staticmethod
    def forward(ctx, a, b, code, eps):
        _check_dev(a, b)
        loss = _zeros((1,), a.device).view(())
        scr = _workspace(L.lib().fsr_elem_loss_scratch(), a.device)
        L.check(L.lib().fsr_elem_loss_fwd(code, eps, _p(a), *a.stride(), _p(b), *b.stride(), *a.shape, _p(loss), _p(scr), _stream()),
                "fsr_elem_loss_fwd")
        ctx.code, ctx.eps = code, eps
        ctx.save_for_backward(a, b)
        return loss

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous().float()
        da = torch.empty_strided(a.shape, a.stride(), dtype=torch.float32, device=a.device)
        L.check(L.lib().fsr_elem_loss_bwd(ctx.code, ctx.eps, _p(a), *a.stride(), _p(b), *b.stride(), _p(g), _p(da), *a.shape, _stream()),
                "fsr_elem_loss_bwd")
        return da, None, None, None


def elem_loss(a, b, kind="l1", eps=1e-3):
    """Mean element-wise loss between float32 (N,C,H,W) tensors, each read through its own strides (no copies): kind = l1, smooth_l1
    (beta 1), charbonnier (sqrt(d^2 + eps^2); 1e-3 is LapSRN's eps) or mse.  b is the target: it must not require a gradient."""
    code, eps = _elem_loss_check(a, b, kind, eps)
    return ElemLossFn.apply(a, b, code, eps)


def bce_with_logits(x, t):
    return BCEWithLogitsFn.apply(x, t)


def smooth_l1(a, b, cd=None):
    """cd: the compute mode of activation operands (needed for x3, whose containers are float32 tensors); images: None."""
    return SmoothL1Fn.apply(a, b, bool(cd is not None and cd.x3))


# ---------------------------------------------------------------------------------- validation metrics
def ssim_sse(a, b):
    """Per-image (sum of the SSIM map, sum of squared errors) of two (N,3,H,W) float32 batches in [-1,1], any strides
    (fsr_ssim_sse; torchmetrics' SSIM / PSNR defaults on (1+x)/2, trainer.py:46-69).  Returns a float32 (N,2) tensor."""
    _check_dev(a, b)
    if a.shape != b.shape or a.dim() != 4 or a.shape[1] != 3:
        raise ValueError("ssim_sse expects two (N,3,H,W) batches of one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    a = a if a.dtype == torch.float32 else a.float()
    b = b if b.dtype == torch.float32 else b.float()
    n, _, h, w = a.shape
    out = torch.empty((n, 2), dtype=torch.float32, device=a.device)
    scr = _workspace(L.lib().fsr_ssim_sse_scratch(n, h, w), a.device)
    L.check(L.lib().fsr_ssim_sse(_p(a), *a.stride(), _p(b), *b.stride(), n, h, w, _p(out), _p(scr), _stream()), "fsr_ssim_sse")
    return out


QUALITY_CHANNELS = {"y": (L.QUALITY_Y, 1), "rgb": (L.QUALITY_RGB, 3)}     # name -> (fsr_quality_u8 code, channels)


def quality_u8(a, b, shave=0, channel="y"):
    """Per-image (sum of the SSIM map, sum of squared errors), in code units 0..255, of two (N,H,W,3) uint8 batches with a border
    of `shave` pixels left out (fsr_quality_u8).  channel "y": BT.601 studio luma; "rgb": the three channels.
    Each tensor has unit stride on its last axis and stride 3 on W; row and image strides are free, so a [:, :H, :W] slice of
    larger frames is read in place.  Returns a float32 (N,2) tensor; with (eh, ew) the shaved extent and C the channel count,
    PSNR = 10 log10(255^2 C eh ew / sse) and SSIM = ssim_sum / (C (eh - 10)(ew - 10))."""
    _check_dev(a, b)
    if channel not in QUALITY_CHANNELS:
        raise ValueError("quality_u8 channel must be one of %s, got %r" % (sorted(QUALITY_CHANNELS), channel))
    for t in (a, b):
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
            raise ValueError("quality_u8 expects (N,H,W,3) uint8 tensors, got %s %s" % (t.dtype, tuple(t.shape)))
    if a.shape != b.shape:
        raise ValueError("quality_u8 expects two batches of one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    n, h, w, _ = a.shape
    shave = int(shave)
    if not 1 <= n <= 65535:
        raise ValueError("quality_u8 takes 1 .. 65535 images per call, got shape %s" % (tuple(a.shape),))
    if shave < 0 or min(h, w) - 2 * shave < 11:
        raise ValueError("quality_u8: shave %d of shape %s leaves no region of at least 11x11" % (shave, tuple(a.shape)))
    for t in (a, b):
        if t.stride(3) != 1 or t.stride(2) != 3 or t.stride(1) < 3 * w or (n > 1 and t.stride(0) < 0):
            raise ValueError("quality_u8 needs strides (*, >= 3 W, 3, 1), got %s for shape %s" % (t.stride(), tuple(t.shape)))
    code = QUALITY_CHANNELS[channel][0]
    out = torch.empty((n, 2), dtype=torch.float32, device=a.device)
    scr = _workspace(L.lib().fsr_quality_u8_scratch(n, h, w, shave, code), a.device)
    L.check(L.lib().fsr_quality_u8(_p(a), a.stride(0), a.stride(1), _p(b), b.stride(0), b.stride(1), n, h, w, shave, code,
                                   _p(out), _p(scr), _stream()), "fsr_quality_u8")
    return out


def u8_to_image(frames):
    """(N,H,W,3) uint8 frames -> float32 (N,3,H,W) VIEW in [-1,1] (x / 127.5 - 1, inference.py:48) of an NHWC buffer: the
    first-layer kernels read it in place through its strides."""
    _check_dev(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError("u8_to_image expects a contiguous (N,H,W,3) uint8 tensor")
    img = torch.empty(frames.shape, dtype=torch.float32, device=frames.device)
    L.check(L.lib().fsr_u8_to_image(_p(frames), _p(img), frames.numel(), _stream()), "fsr_u8_to_image")
    return img.permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------- the eight symmetries of the rectangle
DIHEDRAL_INVERSE = (0, 1, 2, 3, 4, 6, 5, 7)      # D_inv[k](D_k(x)) == x: codes 5 and 6 are each other's inverse
ENSEMBLE_KINDS = {"f32": L.OUT_F32, "u8": L.OUT_U8}
PROFILE_DIHEDRAL = None   # a list: every dihedral launch appends (what, start event, end event) -- tools/ensemble_bench.py


def _check_codes(k0, k1, who):
    for k in (k0, k1):
        if isinstance(k, bool) or int(k) != k or not 0 <= k <= 7:
            raise ValueError("%s: a transform code is an integer in 0..7, got %r" % (who, k))
    if k0 > k1 or (k0 >> 2) != (k1 >> 2):
        raise ValueError("%s: codes k0..k1 must lie in one orientation group (0..3 or 4..7), got %d..%d" % (who, k0, k1))
    return int(k0), int(k1)


def _profiled_dihedral(what, call):
    prof = PROFILE_DIHEDRAL
    if prof is None:
        return call()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    call()
    ev1.record()
    prof.append((what, ev0, ev1))


def dihedral_members(frames, k0=0, k1=3):
    """The self-ensemble inputs of members k0..k1 (one orientation group: codes 0..3 or 4..7) of (N,H,W,3) frames -- uint8, or the
    contiguous float32 NHWC buffer behind u8_to_image's view.  Returns the float32 ((k1-k0+1) N, 3, H, W) VIEW of an NHWC buffer for
    codes 0..3, (..., 3, W, H) for codes 4..7, member-major: image (k - k0) N + i is D_k of frame i, and for uint8 frames equals
    D_k(u8_to_image(frames)) bit for bit (fsr_dihedral_members)."""
    _check_dev(frames)
    k0, k1 = _check_codes(k0, k1, "dihedral_members")
    if frames.dtype not in (torch.uint8, torch.float32) or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError("dihedral_members expects a contiguous (N,H,W,3) uint8 or float32 tensor, got %s %s" % (frames.dtype, tuple(frames.shape)))
    n, h, w, _ = frames.shape
    oh, ow = (h, w) if k0 < 4 else (w, h)
    out = torch.empty(((k1 - k0 + 1) * n, oh, ow, 3), dtype=torch.float32, device=frames.device)
    _profiled_dihedral("members", lambda: L.check(L.lib().fsr_dihedral_members(
        _p(frames), int(frames.dtype == torch.uint8), n, h, w, k0, k1, _p(out), _stream()), "fsr_dihedral_members"))
    return out.permute(0, 3, 1, 2)


def dihedral_accumulate(y_nhwc, k0, k1, acc, kind="f32"):
    """Adds the float head outputs of members k0..k1 onto the self-ensemble sum (fsr_dihedral_accumulate).  y_nhwc: contiguous float32
    ((k1-k0+1) N, OH, OW, 3) for codes 0..3, (..., OW, OH, 3) for codes 4..7, member-major; acc: contiguous float32 (N, OH, OW, 3), the
    running sum -- assigned by the call with k0 == 0, continued by the others, in code order.  The call with k1 == 7 leaves acc alone
    and returns the mean instead: kind "f32" the float32 (N,3,OH,OW) view of an NHWC buffer, 0.125 * sum; kind "u8" the uint8
    (N,OH,OW,3) frames by the truncating cast of forward_u8.  Other calls return None."""
    _check_dev(y_nhwc, acc)
    k0, k1 = _check_codes(k0, k1, "dihedral_accumulate")
    if kind not in ENSEMBLE_KINDS:
        raise ValueError("dihedral_accumulate kind must be one of %s, got %r" % (sorted(ENSEMBLE_KINDS), kind))
    if acc.dtype != torch.float32 or acc.dim() != 4 or acc.shape[3] != 3 or not acc.is_contiguous():
        raise ValueError("dihedral_accumulate expects a contiguous float32 (N,OH,OW,3) accumulator, got %s %s" % (acc.dtype, tuple(acc.shape)))
    n, oh, ow, _ = acc.shape
    want = ((k1 - k0 + 1) * n,) + ((oh, ow) if k0 < 4 else (ow, oh)) + (3,)
    if y_nhwc.dtype != torch.float32 or tuple(y_nhwc.shape) != want or not y_nhwc.is_contiguous():
        raise ValueError("dihedral_accumulate: members %d..%d of a %s sum are a contiguous float32 %s tensor, got %s %s"
                         % (k0, k1, tuple(acc.shape), want, y_nhwc.dtype, tuple(y_nhwc.shape)))
    out = None
    if k1 == 7:
        out = torch.empty((n, oh, ow, 3), dtype=torch.float32 if kind == "f32" else torch.uint8, device=acc.device)
    _profiled_dihedral("accumulate", lambda: L.check(L.lib().fsr_dihedral_accumulate(
        _p(y_nhwc), n, oh, ow, k0, k1, _p(acc), None if out is None else _p(out), ENSEMBLE_KINDS[kind], _stream()), "fsr_dihedral_accumulate"))
    if out is None:
        return None
    return out.permute(0, 3, 1, 2) if kind == "f32" else out


# ---------------------------------------------------------------------------------- row bands of the generator's tail
TAIL_HALO = 2        # rows of the last up-sampling convolution's input discarded at each window edge that is not the frame's


def tail_windows(H2, R):
    """Windows of `R + 4` rows that cover a frame of H2 rows: [(start, core_lo, core_hi)].  Window k owns the core rows
    [k R, min((k + 1) R, H2)) and starts at clamp(k R - 2, 0, H2 - (R + 4)), so a window edge either is the frame's edge or lies
    2 rows outside the core.  H2 <= R + 4: the one window (0, 0, H2), the whole frame."""
    H2, R = int(H2), int(R)
    if H2 < 1 or R < 1:
        raise ValueError("tail_windows: H2 and R must be positive, got %d and %d" % (H2, R))
    Hw = R + 2 * TAIL_HALO
    if H2 <= Hw:
        return [(0, 0, H2)]
    return [(max(0, min(lo - TAIL_HALO, H2 - Hw)), lo, min(lo + R, H2)) for lo in range(0, H2, R)]


def copy_rows(src, dst, src_pitch, dst_pitch, row_bytes, first, count, H2, R, mul=1, scatter=False, src_offset=0, dst_offset=0):
    """fsr_copy_rows on two contiguous tensors, taken as bytes: gathers the windows first .. first + count - 1 of tail_windows(H2, R)
    (numbered image * windows + k over all images) from the frames in `src` into the group images of `dst`, or (scatter) copies the
    `mul` rows per core row of each window in `src` to their place in the frames of `dst`.  Pitches: bytes between consecutive images;
    offsets: bytes added to the bases (the planes of a planar payload).  Both extents are checked here -- the kernel cannot."""
    _check_dev(src, dst)
    if not (src.is_contiguous() and dst.is_contiguous()):
        raise ValueError("copy_rows expects contiguous tensors")
    H2, R, mul, first, count = int(H2), int(R), int(mul), int(first), int(count)
    Hw = R + 2 * TAIL_HALO
    if R >= 1 and H2 >= Hw and mul >= 1 and first >= 0 and count >= 1 and row_bytes >= 1:
        nwin = (H2 + R - 1) // R
        last_img = (first + count - 1) // nwin
        frame_end = last_img * (dst_pitch if scatter else src_pitch) + H2 * mul * row_bytes
        group_end = (count - 1) * (src_pitch if scatter else dst_pitch) + Hw * mul * row_bytes
        src_end, dst_end = (group_end, frame_end) if scatter else (frame_end, group_end)
        if (src_offset < 0 or dst_offset < 0 or src_offset + src_end > src.numel() * src.element_size()
                or dst_offset + dst_end > dst.numel() * dst.element_size()):
            raise ValueError("copy_rows: the windows %d..%d reach beyond a tensor (%d / %d bytes needed, %d / %d given)"
                             % (first, first + count - 1, src_offset + src_end, dst_offset + dst_end,
                                src.numel() * src.element_size(), dst.numel() * dst.element_size()))
    L.check(L.lib().fsr_copy_rows(src.data_ptr() + src_offset, int(src_pitch), dst.data_ptr() + dst_offset, int(dst_pitch), int(row_bytes),
                                  first, count, H2, Hw, R, mul, int(bool(scatter)), _stream()), "fsr_copy_rows")


def check_depth(depth, lo=8):
    """The sample depth as an int, refused outside lo..16."""
    if isinstance(depth, bool) or int(depth) != depth or not lo <= depth <= 16:
        raise ValueError("sample depth must be an integer in %d..16, got %r" % (lo, depth))
    return int(depth)


# ---------------------------------------------------------------------------------- planar YUV in and out
YUV_MATRICES = {"bt601": L.YUV_BT601, "bt709": L.YUV_BT709}
CHROMA_SITINGS = {"jpeg": L.SITING_JPEG, "mpeg2": L.SITING_MPEG2}
CHROMAS = {"420": L.CHROMA_420, "422": L.CHROMA_422, "444": L.CHROMA_444}
_YUV_NAMES = {"420": ("i420_to_image", "image_to_i420", "I420"), "422": ("yuv_to_image", "image_to_yuv", "4:2:2"),
              "444": ("yuv_to_image", "image_to_yuv", "4:4:4")}      # what the messages call the decode, the encode and the frames


def yuv_matrix_code(matrix):
    if matrix not in YUV_MATRICES:
        raise ValueError("colour matrix must be one of %s, got %r" % (sorted(YUV_MATRICES), matrix))
    return YUV_MATRICES[matrix]


def chroma_code(chroma):
    if chroma not in CHROMAS:
        raise ValueError("chroma subsampling must be one of %s, got %r" % (sorted(CHROMAS), chroma))
    return CHROMAS[chroma]


YUV_LAYOUTS = {"planar": L.LAYOUT_PLANAR, "nv12": L.LAYOUT_NV12}


def layout_code(layout, chroma="420"):
    """The payload layout's code.  "nv12" (semi-planar: Y, then one plane of (Cb, Cr) pairs; above 8 bits the code sits in the HIGH
    bits of its 16-bit word -- NV12, P010, P012, P016) exists for chroma "420" only."""
    if layout not in YUV_LAYOUTS:
        raise ValueError("payload layout must be one of %s, got %r" % (sorted(YUV_LAYOUTS), layout))
    if layout == "nv12" and chroma != "420":
        raise ValueError("layout \"nv12\" (semi-planar) is for chroma \"420\" only, got chroma %r" % (chroma,))
    return YUV_LAYOUTS[layout]


def _check_yuv_extents(chroma, h, w):
    """The output extents a subsampling can hold: even ones for "420", an even width for "422", any for "444"."""
    if chroma == "420" and (h % 2 or w % 2):
        raise ValueError("I420 output needs even output extents, got %d x %d" % (h, w))
    if chroma == "422" and w % 2:
        raise ValueError("4:2:2 output needs an even output width, got %d" % w)


def yuv_frame_bytes(h, w, chroma="420", depth=8, layout="planar"):
    """Bytes of one planar YUV payload at h x w: the Y plane, then Cb and Cr of ceil(h/2) x ceil(w/2) ("420"), h x ceil(w/2) ("422")
    or h x w ("444") each -- one byte per sample at depth 8, two (little-endian, the value in the low `depth` bits: Y4M's C420p<depth>
    and its kin) at depths 9..16.  layout "nv12" ("420" only): the same samples with Cb and Cr interleaved in one plane, so the same
    count."""
    chroma_code(chroma)
    layout_code(layout, chroma)
    ch, cw = (h + 1) // 2 if chroma == "420" else h, w if chroma == "444" else (w + 1) // 2
    return (h * w + 2 * ch * cw) * (2 if check_depth(depth) > 8 else 1)


def yuv_to_image(frames, h, w, chroma="420", siting=None, matrix="bt601", full_range=False, depth=8, layout="planar"):
    """(N, yuv_frame_bytes(h, w, chroma, depth)) uint8 planar YUV payloads -> float32 (N,3,H,W) VIEW in [-1,1] of an NHWC buffer (2 c - 1
    of the decoded RGB; fsr_yuv_to_image), the layout u8_to_image returns.  depth 9..16: payloads of 16-bit samples,
    still a uint8 tensor.  "420": chroma upsampled bilinearly at `siting` "jpeg" (centred, the default) or "mpeg2" (co-sited
    horizontally).  "422": chroma interpolated horizontally only, linearly with edge clamp, at "mpeg2" (co-sited with the even luma
    columns: what Y4M's C422 means, and the default) or "jpeg".  "444": no interpolation, `siting` is ignored.
    layout "nv12" ("420" only; fsr_yuv_to_image_ex): semi-planar payloads -- NV12 at depth 8, P010 / P012 / P016 above,
    whose low 16 - depth bits are ignored."""
    code = chroma_code(chroma)
    lcode = layout_code(layout, chroma)
    _check_dev(frames)
    depth = check_depth(depth)
    if siting is None or chroma == "444":
        siting = "mpeg2" if chroma == "422" else "jpeg"
    if siting not in CHROMA_SITINGS:
        raise ValueError("chroma siting must be one of %s, got %r" % (sorted(CHROMA_SITINGS), siting))
    fb = yuv_frame_bytes(h, w, chroma, depth)
    if (frames.dtype != torch.uint8 or frames.dim() != 2 or frames.shape[1] != fb or not frames.is_contiguous()):
        raise ValueError("%s expects a contiguous (N, %d) uint8 tensor of %dx%d %d-bit %s frames, got %s %s"
                         % (_YUV_NAMES[chroma][0], fb, w, h, depth, _YUV_NAMES[chroma][2], frames.dtype, tuple(frames.shape)))
    n = frames.shape[0]
    img = torch.empty((n, h, w, 3), dtype=torch.float32, device=frames.device)
    prof = PROFILE_YUV
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    if lcode != L.LAYOUT_PLANAR:
        L.check(L.lib().fsr_yuv_to_image_ex(_p(frames), _p(img), n, h, w, code, lcode, CHROMA_SITINGS[siting], yuv_matrix_code(matrix),
                                            int(bool(full_range)), depth, _stream()), "fsr_yuv_to_image_ex")
    else:
        L.check(L.lib().fsr_yuv_to_image(_p(frames), _p(img), n, h, w, code, CHROMA_SITINGS[siting], yuv_matrix_code(matrix),
                                         int(bool(full_range)), depth, _stream()), "fsr_yuv_to_image")
    if prof is not None:
        ev1.record()
        prof.append(("decode", chroma, ev0, ev1, img.numel() * 4 + frames.numel()))
    return img.permute(0, 3, 1, 2)


def image_to_yuv(t_nhwc, chroma="420", matrix="bt601", full_range=False, depth=8, layout="planar"):
    """The planar YUV encode of DESIGN.md §6c on its own (fsr_image_to_yuv): contiguous float32 (N,H,W,3) tanh output -> uint8
    (N, yuv_frame_bytes(H, W, chroma, depth)) payloads, depth 8..16 -- for "420" what the head's FSR_OUT_I420 epilogue computes, at any
    depth.  "420" needs even H and W; "422" an even W (chroma co-sited with the even luma columns); "444" takes any extents.
    layout "nv12" ("420" only; fsr_image_to_yuv_ex): the same codes as a semi-planar payload -- NV12 at depth 8, P010 /
    P012 / P016 above (the code in the high bits, the low 16 - depth bits zero)."""
    code = chroma_code(chroma)
    lcode = layout_code(layout, chroma)
    _check_dev(t_nhwc)
    depth = check_depth(depth)
    if t_nhwc.dtype != torch.float32 or t_nhwc.dim() != 4 or t_nhwc.shape[3] != 3 or not t_nhwc.is_contiguous():
        raise ValueError("%s expects a contiguous float32 (N,H,W,3) tensor, got %s %s" % (_YUV_NAMES[chroma][1], t_nhwc.dtype, tuple(t_nhwc.shape)))
    n, h, w, _ = t_nhwc.shape
    _check_yuv_extents(chroma, h, w)
    out = torch.empty((n, yuv_frame_bytes(h, w, chroma, depth)), dtype=torch.uint8, device=t_nhwc.device)
    prof = PROFILE_YUV
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    if lcode != L.LAYOUT_PLANAR:
        L.check(L.lib().fsr_image_to_yuv_ex(_p(t_nhwc), n, h, w, code, lcode, yuv_matrix_code(matrix), int(bool(full_range)), depth, _p(out),
                                            _stream()), "fsr_image_to_yuv_ex")
    else:
        L.check(L.lib().fsr_image_to_yuv(_p(t_nhwc), n, h, w, code, yuv_matrix_code(matrix), int(bool(full_range)), depth, _p(out), _stream()),
                "fsr_image_to_yuv")
    if prof is not None:
        ev1.record()
        prof.append(("encode", chroma, ev0, ev1, t_nhwc.numel() * 4 + out.numel()))
    return out


PROFILE_YUV = None        # a list: every decode / encode launch appends (what, chroma, start event, end event, algorithmic bytes) -- tools/video_bench.py


# 4:2:0 under its own names
def i420_frame_bytes(h, w, depth=8):
    return yuv_frame_bytes(h, w, "420", depth)


def i420_to_image(frames, h, w, siting="jpeg", matrix="bt601", full_range=False, depth=8):
    return yuv_to_image(frames, h, w, "420", siting, matrix, full_range, depth)


def image_to_i420(t_nhwc, matrix="bt601", full_range=False, depth=8):
    return image_to_yuv(t_nhwc, "420", matrix, full_range, depth)


# ---------------------------------------------------------------------------------- arbitrary output size
_aa_taps_cache = {}   # (in_size, out_size, device) -> (weights (out, k) float32, start (out,) int32, count (out,) int32, k)
RESAMPLE_KINDS = {"f32": L.OUT_F32, "u8": L.OUT_U8, "i420": L.OUT_I420}


def aa_taps(in_size, out_size, device):
    """Device tensors of dataloader.aa_bicubic_taps(in_size, out_size): the normalised float32 taps of the antialiased bicubic
    (torch's upsample_bicubic2d_aa) of one axis, in either direction.  Cached per (in, out, device); a table is built and
    uploaded on first use, which must lie OUTSIDE graph capture (InferencePipeline's warm-up call sees to it)."""
    from .dataloader import aa_bicubic_taps
    key = (int(in_size), int(out_size), str(torch.device(device)))
    hit = _aa_taps_cache.get(key)
    if hit is None:
        if key[0] <= 0 or key[1] <= 0:
            raise ValueError("aa_taps needs positive sizes, got %d -> %d" % key[:2])
        start, count, w, k = aa_bicubic_taps(key[0], key[1])
        hit = _aa_taps_cache[key] = (torch.from_numpy(w).to(device), torch.from_numpy(start).to(device),
                                     torch.from_numpy(count).to(device), int(k))
    return hit


def resample_image(t_nhwc, out_h, out_w, kind="f32", matrix="bt601", full_range=False, depth=8, chroma="420", layout="planar"):
    """Antialiased bicubic resize of a head output to out_h x out_w, fused with the output conversion (fsr_resample_image;
    DESIGN.md §6d).  t_nhwc: contiguous float32 (N,H,W,3) tanh output (the NHWC buffer behind Generator.forward's view).
      kind "f32" : float32 (N,3,out_h,out_w) VIEW of an NHWC buffer, 2 v - 1 of the resized c = (t + 1) / 2 -- what
                   F.interpolate(t, mode="bicubic", antialias=True, align_corners=False) returns;
      kind "u8"  : uint8 (N,out_h,out_w,3), (unsigned char)(clamp(v, 0, 1) * 255): forward_u8's bytes at another size;
      kind "i420": uint8 (N, yuv_frame_bytes(out_h, out_w, chroma, depth)), the planes of image_to_yuv for clamp(v, 0, 1) in (matrix,
                   full_range) (fsr_resample_image_yuv): "420" needs even extents, "422" an even out_w, "444" takes any; depth 9..16:
                   16-bit samples.  layout "nv12" (chroma "420" only): image_to_yuv's semi-planar payload (fsr_resample_image_yuv_ex).
                   The other kinds take chroma "420", depth 8 and layout "planar" only."""
    _check_dev(t_nhwc)
    depth = check_depth(depth)
    ccode = chroma_code(chroma)
    lcode = layout_code(layout, chroma)
    if layout != "planar" and kind != "i420":
        raise ValueError("resample_image: layout %r is for kind \"i420\" only, got kind %r" % (layout, kind))
    if chroma != "420" and kind != "i420":
        raise ValueError("resample_image: chroma %r is for kind \"i420\" only" % (chroma,))
    if depth != 8 and kind != "i420":
        raise ValueError("resample_image: depth %d is for kind \"i420\" only" % depth)
    if kind not in RESAMPLE_KINDS:
        raise ValueError("resample_image kind must be one of %s, got %r" % (sorted(RESAMPLE_KINDS), kind))
    if t_nhwc.dtype != torch.float32 or t_nhwc.dim() != 4 or t_nhwc.shape[3] != 3 or not t_nhwc.is_contiguous():
        raise ValueError("resample_image expects a contiguous float32 (N,H,W,3) tensor, got %s %s" % (t_nhwc.dtype, tuple(t_nhwc.shape)))
    out_h, out_w = int(out_h), int(out_w)
    if out_h <= 0 or out_w <= 0:
        raise ValueError("resample_image needs a positive output size, got %d x %d" % (out_h, out_w))
    mcode = yuv_matrix_code(matrix) if kind == "i420" else 0
    if kind == "i420":
        _check_yuv_extents(chroma, out_h, out_w)
    n, h, w, _ = t_nhwc.shape
    wy, ymin, ysize, ky = aa_taps(h, out_h, t_nhwc.device)
    wx, xmin, xsize, kx = aa_taps(w, out_w, t_nhwc.device)
    if kind == "f32":
        out = torch.empty((n, out_h, out_w, 3), dtype=torch.float32, device=t_nhwc.device)
    elif kind == "u8":
        out = torch.empty((n, out_h, out_w, 3), dtype=torch.uint8, device=t_nhwc.device)
    else:
        out = torch.empty((n, yuv_frame_bytes(out_h, out_w, chroma, depth)), dtype=torch.uint8, device=t_nhwc.device)
    prof = PROFILE_RESAMPLE
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    taps = (_p(wy), _p(ymin), _p(ysize), ky, _p(wx), _p(xmin), _p(xsize), kx)
    if kind == "i420" and lcode != L.LAYOUT_PLANAR:
        L.check(L.lib().fsr_resample_image_yuv_ex(_p(t_nhwc), n, h, w, out_h, out_w, *taps, ccode, lcode, mcode, int(bool(full_range)), depth,
                                                  _p(out), _stream()), "fsr_resample_image_yuv_ex")
    elif kind == "i420":
        L.check(L.lib().fsr_resample_image_yuv(_p(t_nhwc), n, h, w, out_h, out_w, *taps, ccode, mcode, int(bool(full_range)), depth, _p(out),
                                               _stream()), "fsr_resample_image_yuv")
    else:
        L.check(L.lib().fsr_resample_image(_p(t_nhwc), n, h, w, out_h, out_w, *taps, RESAMPLE_KINDS[kind], mcode, int(bool(full_range)), _p(out),
                                           _stream()), "fsr_resample_image")
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, t_nhwc.numel() * 4 + out.numel() * out.element_size()))
    return out.permute(0, 3, 1, 2) if kind == "f32" else out


PROFILE_RESAMPLE = None   # a list: every resample_image launch appends (start event, end event, algorithmic bytes) -- tools/video_bench.py


# ------------------------------------------------------------------ training degradations (csrc/degrade.hip)
BLUR_SIGMA_MAX, NOISE_SIGMA_MAX = 3.0, 25.0
JPEG_SUBSAMPLINGS = ("420", "444")
DEGRADE_WORDS = L.BLUR_TAPS + 5      # 4-byte words per sample: the taps, the radius, the noise sigma, two seed words, the quality


def gaussian_taps(sigma):
    """(radius, float32 taps j = -r..r) of the blur contract: r = min(ceil(3 sigma), 9), exp(-j^2 / 2 sigma^2) normalised in float64 on
    the host and cast to float32 -- the device never calls exp.  sigma = 0: the identity (r = 0)."""
    sigma = float(sigma)
    if not 0.0 <= sigma <= BLUR_SIGMA_MAX:
        raise ValueError("blur sigma must lie in [0, %g] (0 = off), got %r" % (BLUR_SIGMA_MAX, sigma))
    if sigma == 0.0:
        return 0, np.ones(1, dtype=np.float32)
    r = min(int(math.ceil(3.0 * sigma)), L.BLUR_MAX_RADIUS)
    j = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(j * j) / (2.0 * sigma * sigma))
    return r, (w / w.sum()).astype(np.float32)


def _per_sample(v, n, what):
    if isinstance(v, torch.Tensor):
        v = v.tolist()
    v = list(v)
    if len(v) != n:
        raise ValueError("%s: expected %d per-sample values, got %d" % (what, n, len(v)))
    return v


def degrade_words(n, blur_sigma=None, noise_sigma=None, seeds=None, quality=None):
    """The per-sample parameters of both degradation entry points as ONE int32 array of DEGRADE_WORDS * n words, so that they travel in a
    single host-to-device copy: [taps: 19 n float32][radii: n int32][noise sigma: n float32][seeds: 2 n uint32][quality: n int32].
    A stage that is not given stays "off" (radius 0, sigma 0, quality 0).  Ranges are checked here: the C entry points only see pointers."""
    T = L.BLUR_TAPS
    words = np.zeros(DEGRADE_WORDS * n, dtype=np.int32)
    if blur_sigma is not None:
        taps = words[:T * n].view(np.float32).reshape(n, T)
        for i, s in enumerate(_per_sample(blur_sigma, n, "blur_sigma")):
            r, t = gaussian_taps(s)
            taps[i, :2 * r + 1] = t
            words[T * n + i] = r
    if noise_sigma is not None:
        sig = [float(s) for s in _per_sample(noise_sigma, n, "noise_sigma")]
        if any(not 0.0 <= s <= NOISE_SIGMA_MAX for s in sig):
            raise ValueError("noise sigma must lie in [0, %g] code units (0 = off), got %r" % (NOISE_SIGMA_MAX, sig))
        words[(T + 1) * n:(T + 2) * n].view(np.float32)[:] = sig
        if seeds is None:
            raise ValueError("noise needs one (s0, s1) pair of 32-bit seed words per sample")
        sd = np.array(_per_sample(seeds, n, "seeds"), dtype=np.int64).reshape(n, 2)
        if sd.min() < 0 or sd.max() > 0xffffffff:
            raise ValueError("seed words must be unsigned 32-bit integers")
        words[(T + 2) * n:(T + 4) * n].view(np.uint32)[:] = sd.reshape(-1).astype(np.uint32)
    if quality is not None:
        q = [int(v) for v in _per_sample(quality, n, "quality")]
        if any(not 0 <= v <= 100 for v in q):
            raise ValueError("JPEG quality must lie in 0..100 (0 = off), got %r" % (q,))
        words[(T + 4) * n:] = q
    return words


def upload_words(words, device):
    """One pinned, non-blocking host-to-device copy of a small parameter array; nothing waits for the device."""
    host = torch.from_numpy(words)
    if torch.device(device).type == "cuda":
        host = host.pin_memory()
    return host.to(device, non_blocking=True)


def _check_degrade_input(x, who):
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
        raise ValueError("%s expects a contiguous float32 (N,3,H,W) tensor, got %s %s" % (who, x.dtype, tuple(x.shape)))
    if x.requires_grad:
        raise ValueError("%s has no autograd: it is a data-path operator, detach the input" % who)
    _check_dev(x)


def degrade_blur_noise_dev(x, dev_words, blur=True, noise=True):
    """fsr_degrade_blur_noise with the parameters already on the device (`dev_words`: degrade_words(...) uploaded).  blur=False is the
    noise-only launch, noise=False the blur alone; the launches depend on these two flags only, never on the values drawn."""
    _check_degrade_input(x, "degrade_blur_noise")
    if not (blur or noise):
        raise ValueError("degrade_blur_noise: neither blur nor noise asked for")
    n, _, h, w = x.shape
    if dev_words.dtype != torch.int32 or dev_words.numel() != DEGRADE_WORDS * n or dev_words.device != x.device:
        raise ValueError("degrade_blur_noise: dev_words must hold %d int32 words on %s" % (DEGRADE_WORDS * n, x.device))
    base, T = dev_words.data_ptr(), L.BLUR_TAPS
    out = torch.empty_like(x)
    tmp = torch.empty_like(x) if blur else None
    L.check(L.lib().fsr_degrade_blur_noise(_p(x), _p(out), _p(tmp), n, h, w, base if blur else None, base + 4 * T * n if blur else None,
                                           base + 4 * (T + 1) * n if noise else None, base + 4 * (T + 2) * n if noise else None, _stream()),
            "fsr_degrade_blur_noise")
    return out


def jpeg_roundtrip_dev(x, dev_words, subsampling="420"):
    """fsr_jpeg_roundtrip with the qualities already on the device (the last n words of `dev_words`)."""
    _check_degrade_input(x, "jpeg_roundtrip")
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError("jpeg_roundtrip: subsampling must be one of %s, got %r" % (JPEG_SUBSAMPLINGS, subsampling))
    n, _, h, w = x.shape
    if dev_words.dtype != torch.int32 or dev_words.numel() != DEGRADE_WORDS * n or dev_words.device != x.device:
        raise ValueError("jpeg_roundtrip: dev_words must hold %d int32 words on %s" % (DEGRADE_WORDS * n, x.device))
    out = torch.empty_like(x)
    L.check(L.lib().fsr_jpeg_roundtrip(_p(x), _p(out), n, h, w, dev_words.data_ptr() + 4 * (L.BLUR_TAPS + 4) * n, chroma_code(subsampling),
                                       _stream()), "fsr_jpeg_roundtrip")
    return out


def jpeg_quality_dev(x, dev_quality, subsampling="420"):
    """fsr_jpeg_roundtrip with a block of its own for the qualities (int32 [N] on the device): the second round's JPEG."""
    _check_degrade_input(x, "jpeg_roundtrip")
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError("jpeg_roundtrip: subsampling must be one of %s, got %r" % (JPEG_SUBSAMPLINGS, subsampling))
    n, _, h, w = x.shape
    if dev_quality.dtype != torch.int32 or dev_quality.numel() != n or dev_quality.device != x.device or not dev_quality.is_contiguous():
        raise ValueError("jpeg_roundtrip: dev_quality must hold %d contiguous int32 words on %s" % (n, x.device))
    out = torch.empty_like(x)
    L.check(L.lib().fsr_jpeg_roundtrip(_p(x), _p(out), n, h, w, dev_quality.data_ptr(), chroma_code(subsampling), _stream()), "fsr_jpeg_roundtrip")
    return out


def degrade_blur_noise(x, blur_sigma, noise_sigma, seeds):
    """Gaussian blur, then additive Gaussian noise, on a float32 (N,3,H,W) batch in [-1,1].  Per sample (sequences or
    tensors of length N): blur_sigma in LR pixels, 0 < sigma <= 3; noise_sigma in 8-bit code units, 0 < sigma <= 25; seeds, one (s0, s1)
    pair of 32-bit words that names the sample's noise field.  0 switches a stage off for a sample (it is copied); None switches it off
    for the call (noise only: one launch; blur only: two).  No autograd."""
    _check_degrade_input(x, "degrade_blur_noise")
    words = degrade_words(x.shape[0], blur_sigma=blur_sigma, noise_sigma=noise_sigma, seeds=seeds)
    return degrade_blur_noise_dev(x, upload_words(words, x.device), blur=blur_sigma is not None, noise=noise_sigma is not None)


def jpeg_roundtrip(x, quality, subsampling="420"):
    """What a baseline JPEG encode + decode does to a float32 (N,3,H,W) batch in [-1,1], without the entropy coder:
    per-sample integer quality 1..100 (libjpeg's table scaling; 0 copies the sample), subsampling "420" or "444".  No autograd."""
    _check_degrade_input(x, "jpeg_roundtrip")
    return jpeg_roundtrip_dev(x, upload_words(degrade_words(x.shape[0], quality=quality), x.device), subsampling)


# ------------------------------------------------------------------ per-sample 2-D filter (csrc/degrade.hip)
FILTER2D_WORDS = L.FILTER2D_TAPS + 1     # 4-byte words per sample: the K x K taps (packed, row-major) and the radius


def filter2d_words(n, kernels):
    """The per-sample parameters of fsr_filter2d as ONE int32 array of FILTER2D_WORDS * n words for a single host-to-device copy:
    [taps: 441 n float32][radii: n int32].  `kernels`: n entries, each a square 2-D array of odd size K <= 21 (cast to float32 as it
    is: dataloader.kernel_bank normalises in float64) or None for "off" (radius 0: the sample is copied)."""
    T = L.FILTER2D_TAPS
    kernels = _per_sample(kernels, n, "kernels")
    words = np.zeros(FILTER2D_WORDS * n, dtype=np.int32)
    taps = words[:T * n].view(np.float32).reshape(n, T)
    for i, k in enumerate(kernels):
        if k is None:
            continue
        k = np.asarray(k)
        if k.ndim != 2 or k.shape[0] != k.shape[1] or k.shape[0] % 2 != 1 or k.shape[0] > 2 * L.FILTER2D_MAX_RADIUS + 1:
            raise ValueError("filter2d: kernel %d must be square with an odd size of at most %d, got shape %s"
                             % (i, 2 * L.FILTER2D_MAX_RADIUS + 1, k.shape))
        if not np.isfinite(k).all():
            raise ValueError("filter2d: kernel %d holds a value that is not finite" % i)
        taps[i, :k.size] = k.reshape(-1)
        words[T * n + i] = k.shape[0] // 2
    return words


def filter2d_dev(x, dev_words):
    """fsr_filter2d with the parameters already on the device (`dev_words`: filter2d_words(...) uploaded, or a view of a larger block).
    One launch whatever the radii are; a sample of radius 0 leaves it as a copy."""
    _check_degrade_input(x, "filter2d")
    n, _, h, w = x.shape
    if dev_words.dtype != torch.int32 or dev_words.numel() != FILTER2D_WORDS * n or dev_words.device != x.device or not dev_words.is_contiguous():
        raise ValueError("filter2d: dev_words must hold %d contiguous int32 words on %s" % (FILTER2D_WORDS * n, x.device))
    base = dev_words.data_ptr()
    out = torch.empty_like(x)
    L.check(L.lib().fsr_filter2d(_p(x), _p(out), n, h, w, base, base + 4 * L.FILTER2D_TAPS * n, _stream()), "fsr_filter2d")
    return out


def filter2d(x, kernels):
    """A K x K filter per sample on a float32 (N,3,H,W) batch: out[n,c,y,x] = sum_dy sum_dx k_n[dy + r, dx + r] *
    in[n, c, clamp(y + dy), clamp(x + dx)] -- correlation, clamped borders, float32 accumulation, dy outer and dx inner.  `kernels`: one
    square array of odd size K <= 21 per sample, or None to copy that sample.  No autograd."""
    _check_degrade_input(x, "filter2d")
    return filter2d_dev(x, upload_words(filter2d_words(x.shape[0], kernels), x.device))


# ------------------------------------------------------------------ resize with a tap table per sample (csrc/degrade.hip)
class ResizeTables:
    """F tap tables per axis for fsr_resize_select, on the device: `x_tables` / `y_tables` are lists of (xmin, xsize, w, kmax) in the
    layout of dataloader.aa_bicubic_taps (one entry per filter, every table of an axis for the same output size); the rows are padded
    to the widest kmax.  Checked here, since the C entry point only sees pointers: xmin >= 0, 1 <= xsize <= kmax, xmin + xsize <= the
    input size."""

    def __init__(self, x_tables, y_tables, in_h, in_w, device):
        if len(x_tables) != len(y_tables) or not x_tables:
            raise ValueError("ResizeTables: one table per filter and axis, at least one filter")
        self.nf, self.in_h, self.in_w = len(x_tables), int(in_h), int(in_w)
        self.x, self.out_w, self.kx = self._pack(x_tables, self.in_w, device)
        self.y, self.out_h, self.ky = self._pack(y_tables, self.in_h, device)

    @staticmethod
    def _pack(tables, in_size, device):
        out = len(tables[0][0])
        kmax = max(int(t[3]) for t in tables)
        w = np.zeros((len(tables), out, kmax), dtype=np.float32)
        lo = np.zeros((len(tables), out), dtype=np.int32)
        sz = np.zeros((len(tables), out), dtype=np.int32)
        for f, (xmin, xsize, wt, k) in enumerate(tables):
            xmin, xsize, wt = np.asarray(xmin), np.asarray(xsize), np.asarray(wt, dtype=np.float32)
            if xmin.shape != (out,) or xsize.shape != (out,) or wt.shape != (out, int(k)):
                raise ValueError("ResizeTables: table %d does not have the layout of aa_bicubic_taps for %d outputs" % (f, out))
            if xmin.min() < 0 or xsize.min() < 1 or xsize.max() > k or (xmin + xsize).max() > in_size:
                raise ValueError("ResizeTables: table %d reads outside its %d input samples or its %d tap slots" % (f, in_size, k))
            w[f, :, :int(k)], lo[f], sz[f] = wt, xmin, xsize
        dev = tuple(torch.from_numpy(a).to(device) for a in (w, lo, sz))
        return dev, out, kmax


def resize_select_dev(x, tables, dev_sel):
    """fsr_resize_select with the table indices already on the device (int32 [N]): horizontal pass, then vertical pass."""
    _check_degrade_input(x, "resize_select")
    n, _, h, w = x.shape
    if (h, w) != (tables.in_h, tables.in_w) or tables.x[0].device != x.device:
        raise ValueError("resize_select: the tables were built for %dx%d inputs on %s, got %dx%d on %s"
                         % (tables.in_h, tables.in_w, tables.x[0].device, h, w, x.device))
    if dev_sel.dtype != torch.int32 or dev_sel.numel() != n or dev_sel.device != x.device or not dev_sel.is_contiguous():
        raise ValueError("resize_select: dev_sel must hold %d contiguous int32 table indices on %s" % (n, x.device))
    out = torch.empty((n, 3, tables.out_h, tables.out_w), dtype=torch.float32, device=x.device)
    tmp = torch.empty((n, 3, h, tables.out_w), dtype=torch.float32, device=x.device)
    (wx, xmin, xsize), (wy, ymin, ysize) = tables.x, tables.y
    L.check(L.lib().fsr_resize_select(_p(x), _p(out), _p(tmp), n, h, w, tables.out_h, tables.out_w, _p(wx), _p(xmin), _p(xsize), tables.kx,
                                      _p(wy), _p(ymin), _p(ysize), tables.ky, tables.nf, dev_sel.data_ptr(), _stream()), "fsr_resize_select")
    return out


def resize_select(x, tables, sel):
    """Resizes a float32 (N,3,H,W) batch with tap table sel[i] of `tables` (a ResizeTables) for sample i: separable, horizontal pass
    first, float32 accumulation in tap order.  An index outside 0 .. tables.nf - 1 is refused.  No autograd."""
    sel = [int(v) for v in _per_sample(sel, x.shape[0], "sel")]
    if any(not 0 <= v < tables.nf for v in sel):
        raise ValueError("resize_select: table indices must lie in 0..%d, got %r" % (tables.nf - 1, sel))
    return resize_select_dev(x, tables, upload_words(np.asarray(sel, dtype=np.int32), x.device))


# ------------------------------------------------------------------ noise kinds (csrc/degrade.hip)
SHOT_GAIN_MAX = 3.0
NOISE_KIND_WORDS = 4       # 4-byte words per sample: the strength, the flags, two seed words


def noise_kind_words(n, strength, flags, seeds):
    """The per-sample parameters of fsr_degrade_noise_kinds as ONE int32 array: [strength: n float32][flags: n int32][seeds: 2 n uint32].
    strength: the sigma in code units (0..25) of a Gaussian sample, the gain g (0..3) of a shot sample (flag L.NOISE_SHOT); 0 = off."""
    st = [float(s) for s in _per_sample(strength, n, "strength")]
    fl = [int(f) for f in _per_sample(flags, n, "flags")]
    if any(f & ~(L.NOISE_SHOT | L.NOISE_GREY) for f in fl):
        raise ValueError("noise flags are bits of NOISE_SHOT | NOISE_GREY, got %r" % (fl,))
    for s, f in zip(st, fl):
        top = SHOT_GAIN_MAX if f & L.NOISE_SHOT else NOISE_SIGMA_MAX
        if not 0.0 <= s <= top:
            raise ValueError("noise strength must lie in [0, %g] (%s; 0 = off), got %r" % (top, "shot gain" if f & L.NOISE_SHOT else "sigma", s))
    sd = np.array(_per_sample(seeds, n, "seeds"), dtype=np.int64).reshape(n, 2)
    if sd.min() < 0 or sd.max() > 0xffffffff:
        raise ValueError("seed words must be unsigned 32-bit integers")
    words = np.zeros(NOISE_KIND_WORDS * n, dtype=np.int32)
    words[:n].view(np.float32)[:] = st
    words[n:2 * n] = fl
    words[2 * n:].view(np.uint32)[:] = sd.reshape(-1).astype(np.uint32)
    return words


def degrade_noise_kinds_dev(x, dev_words):
    """fsr_degrade_noise_kinds with noise_kind_words(...) already on the device: one launch."""
    _check_degrade_input(x, "degrade_noise_kinds")
    n, _, h, w = x.shape
    if dev_words.dtype != torch.int32 or dev_words.numel() != NOISE_KIND_WORDS * n or dev_words.device != x.device or not dev_words.is_contiguous():
        raise ValueError("degrade_noise_kinds: dev_words must hold %d contiguous int32 words on %s" % (NOISE_KIND_WORDS * n, x.device))
    base = dev_words.data_ptr()
    out = torch.empty_like(x)
    L.check(L.lib().fsr_degrade_noise_kinds(_p(x), _p(out), n, h, w, base, base + 4 * n, base + 8 * n, _stream()), "fsr_degrade_noise_kinds")
    return out


def degrade_noise_kinds(x, strength, flags, seeds):
    """Additive noise of a kind per sample on a float32 (N,3,H,W) batch in [-1,1].  flags[i] = 0: Gaussian colour
    noise of sigma strength[i] code units, what degrade_blur_noise adds; L.NOISE_SHOT: shot noise in its normal approximation,
    x += z sqrt(g v) 2/255 with v the element's code and g = strength[i]; L.NOISE_GREY (may be combined): one z per pixel, shared by its
    three channels.  strength 0 copies the sample.  No autograd."""
    _check_degrade_input(x, "degrade_noise_kinds")
    return degrade_noise_kinds_dev(x, upload_words(noise_kind_words(x.shape[0], strength, flags, seeds), x.device))
