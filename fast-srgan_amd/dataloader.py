"""HR/LR crop pipeline on the device: drop-in for /root/reference/dataloader.py.

`NumpyImagesDataset(numpy_paths, lr_image_size, scale_factor)` keeps the reference's constructor, `__len__`
and `__getitem__ -> (lr (3,l,l), hr (3,l*s,l*s))` float32 in [-1,1] (dataloader.py:11-38) -- but the uint8
CHW arrays are uploaded once and stay resident in HBM, and the crop / float conversion / antialiased bicubic
down-scale / [-1,1] mapping run in two HIP kernels (csrc/data.hip) instead of 16 DataLoader worker processes.
`DeviceBatchLoader` draws whole batches that way (what train.py's RandomSampler(replacement=True) +
DataLoader pair does, train.py:69-113) and is what the Trainer iterates.
"""
import collections
import math
import random

import numpy as np
import torch

from . import _lib as L
from . import kernel_bank
from . import ops
from .ops import _p, _stream


def _cubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def aa_bicubic_taps(in_size, out_size):
    """Tap table of the antialiased bicubic down-scale (what v2.Resize(BICUBIC, antialias=True) computes for a
    float tensor, dataloader.py:15-19): support = 2*scale, center = scale*(i+.5), xmin = max(int(center-support+.5),0),
    xsize = min(int(center+support+.5), in) - xmin, w_j = cubic((j+xmin-center+.5)/scale), normalised in float32."""
    scale = in_size / out_size
    support = 2.0 * scale if scale >= 1.0 else 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    kmax = int(math.ceil(support)) * 2 + 1
    xmin = np.zeros(out_size, dtype=np.int32)
    xsize = np.zeros(out_size, dtype=np.int32)
    w = np.zeros((out_size, kmax), dtype=np.float32)
    for i in range(out_size):
        center = scale * (i + 0.5)
        lo = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - lo
        ws = np.array([_cubic((j + lo - center + 0.5) * inv) for j in range(n)], dtype=np.float32)
        w[i, :n] = ws / np.float32(ws.sum(dtype=np.float32))
        xmin[i], xsize[i] = lo, n
    return xmin, xsize, w, kmax


RESIZE_FILTERS = ("bicubic", "bilinear", "area")


def resize_taps(in_size, out_size, kind):
    """(xmin, xsize, w, kmax) of one down-scale filter in aa_bicubic_taps's layout.  "bicubic": aa_bicubic_taps itself; "bilinear": the
    antialiased triangle of support `scale` (F.interpolate(mode="bilinear", antialias=True)), built by the same window rule and normalised
    in float64; "area": the box over [floor(i scale), ceil((i + 1) scale)) (F.interpolate(mode="area"))."""
    if kind == "bicubic":
        return aa_bicubic_taps(in_size, out_size)
    scale = in_size / out_size
    xmin = np.zeros(out_size, dtype=np.int32)
    xsize = np.zeros(out_size, dtype=np.int32)
    if kind == "bilinear":
        support = scale if scale >= 1.0 else 1.0
        inv = 1.0 / scale if scale >= 1.0 else 1.0
        kmax = int(math.ceil(support)) * 2 + 1
        w = np.zeros((out_size, kmax), dtype=np.float32)
        for i in range(out_size):
            center = scale * (i + 0.5)
            lo = max(int(center - support + 0.5), 0)
            n = min(int(center + support + 0.5), in_size) - lo
            ws = np.array([max(0.0, 1.0 - abs((j + lo - center + 0.5) * inv)) for j in range(n)], dtype=np.float64)
            w[i, :n] = ws / ws.sum()
            xmin[i], xsize[i] = lo, n
        return xmin, xsize, w, kmax
    if kind == "area":
        kmax = int(math.ceil(scale)) + 1
        w = np.zeros((out_size, kmax), dtype=np.float32)
        for i in range(out_size):
            lo, hi = (i * in_size) // out_size, -((-(i + 1) * in_size) // out_size)
            w[i, :hi - lo] = 1.0 / (hi - lo)
            xmin[i], xsize[i] = lo, hi - lo
        return xmin, xsize, w, kmax
    raise ValueError("resize filter must be one of %s, got %r" % (", ".join(RESIZE_FILTERS), kind))


DegradeParams = collections.namedtuple("DegradeParams", "blur_sigma noise_sigma seeds quality")   # lists of n; 0 = the stage is off
# the high-order draws of a batch, lists of n: kernels as kernel_bank.draw's parameters or None; noise as (strength, flags)
HighOrderParams = collections.namedtuple("HighOrderParams", "kernel1 resize noise1 kernel2 noise2 seeds2 quality2 sinc_a sinc_b")


class DegradeParamsHO(DegradeParams):
    """DegradeParams of a Degradation with a high-order stage configured: the same four fields (and the same tuple), and the draws of
    the second stream in `.ho`."""
    ho = None


_BANK_KEYS = ("kernel_size", "kernel_kinds", "kernel_sigma", "kernel_beta_generalized", "kernel_beta_plateau", "sinc_prob")
SECOND_KEYS = ("kernel_prob",) + _BANK_KEYS + ("noise_prob", "noise_sigma", "noise_shot_prob", "noise_shot_gain", "noise_grey_prob",
                                               "jpeg_prob", "jpeg_quality")
HO_STREAM_MULTIPLIER = 0x9E3779B97F4A7C15     # odd: the second random stream's seed is seed * this mod 2^64


def _prob(name, v):
    v = float(v)
    if not 0.0 <= v <= 1.0:
        raise ValueError("Degradation: %s must be a probability, got %r" % (name, v))
    return v


def _range(name, v, top, integer=False):
    v = tuple((int if integer else float)(x) for x in v)
    if len(v) != 2 or not 0 < v[0] <= v[1] <= top:
        raise ValueError("Degradation: %s must be a (lo, hi) pair with 0 < lo <= hi <= %g, got %r" % (name, top, v))
    return v


class _Round:
    """The high-order stages of one blur -> noise -> JPEG round: probabilities, ranges and the kernel bank.  `bank`: the KernelBank
    keyword arguments (a subset of _BANK_KEYS).  The first round takes only the kernel and the noise-kind keys from here -- its blur,
    noise and JPEG settings are Degradation's own, first-order ones."""

    def __init__(self, prefix, bank, kernel_prob=0., noise_prob=0., noise_sigma=(1.0, 10.0), noise_shot_prob=0., noise_shot_gain=(0.05, 1.5),
                 noise_grey_prob=0., jpeg_prob=0., jpeg_quality=(30, 95)):
        self.bank = kernel_bank.KernelBank(**bank)
        self.kernel_prob, self.noise_prob = _prob(prefix + "kernel_prob", kernel_prob), _prob(prefix + "noise_prob", noise_prob)
        self.noise_shot_prob, self.noise_grey_prob = _prob(prefix + "noise_shot_prob", noise_shot_prob), _prob(prefix + "noise_grey_prob", noise_grey_prob)
        self.jpeg_prob = _prob(prefix + "jpeg_prob", jpeg_prob)
        self.noise_sigma = _range(prefix + "noise_sigma", noise_sigma, ops.NOISE_SIGMA_MAX)
        self.noise_shot_gain = _range(prefix + "noise_shot_gain", noise_shot_gain, ops.SHOT_GAIN_MAX)
        self.jpeg_quality = _range(prefix + "jpeg_quality", jpeg_quality, 100, integer=True)

    def draw_kernel(self, rng):
        on, params = rng.random() < self.kernel_prob, self.bank.draw(rng)
        return params if on else None

    def draw_kind(self, rng):
        """(shot decision, gain, grey decision): three variates, always."""
        return rng.random() < self.noise_shot_prob, rng.uniform(*self.noise_shot_gain), rng.random() < self.noise_grey_prob


def _noise_of(sigma, kind):
    """(strength, flags) of fsr_degrade_noise_kinds for a sample whose Gaussian sigma is `sigma` (0: the noise did not fire)."""
    shot, gain, grey = kind
    if sigma == 0:
        return 0.0, 0
    return (gain if shot else sigma), (L.NOISE_SHOT if shot else 0) | (L.NOISE_GREY if grey else 0)


class Degradation:
    """Random degradation of the LR batch on the device: LR = JPEG(blur(LR) + noise), each stage with its own probability and a
    strength drawn uniformly per sample (csrc/degrade.hip).  blur_sigma in LR pixels (0 < sigma <= 3), noise_sigma in
    8-bit code units (<= 25), jpeg_quality integers in 1..100.  The draws come from this object's OWN random.Random: the crop and index
    streams of DeviceBatchLoader do not move when it is switched on.

    The high-order model, all of it off by default: kernel_prob and the kernel_bank.KernelBank keys (kernel_size,
    kernel_kinds, kernel_sigma, kernel_beta_generalized, kernel_beta_plateau, sinc_prob) -- a K x K blur kernel per sample on the HR
    crop, in front of the down-scale; resize_filters, the draw weights of RESIZE_FILTERS for that down-scale; noise_shot_prob,
    noise_shot_gain, noise_grey_prob -- how often a sample's noise is shot noise of that gain (normal approximation) and grey;
    second, a dict of SECOND_KEYS -- a second blur -> noise -> JPEG round on lr; final_sinc_prob, final_sinc_size -- a sinc filter
    of an odd size drawn from that (lo, hi) range, in LR pixels, before or behind the last JPEG.  Their draws come from a SECOND
    random.Random of this object (rng2): the first stream does not move either."""

    def __init__(self, blur_sigma=(0.2, 2.0), blur_prob=0., noise_sigma=(1.0, 10.0), noise_prob=0., jpeg_quality=(30, 95), jpeg_prob=0.,
                 jpeg_subsampling="420", seed=0, kernel_prob=0., resize_filters=(1, 0, 0), noise_shot_prob=0., noise_shot_gain=(0.05, 1.5),
                 noise_grey_prob=0., second=None, final_sinc_prob=0., final_sinc_size=(7, 21), kernel_size=(7, 21),
                 kernel_kinds=(0.45, 0.25, 0.12, 0.03, 0.12, 0.03), kernel_sigma=(0.2, 3.0), kernel_beta_generalized=(0.5, 4.0),
                 kernel_beta_plateau=(1.0, 2.0), sinc_prob=0.):
        self.blur_sigma, self.noise_sigma = tuple(float(v) for v in blur_sigma), tuple(float(v) for v in noise_sigma)
        self.jpeg_quality = tuple(int(v) for v in jpeg_quality)
        self.blur_prob, self.noise_prob, self.jpeg_prob = float(blur_prob), float(noise_prob), float(jpeg_prob)
        self.jpeg_subsampling = str(jpeg_subsampling)
        for name, (lo, hi), top in (("blur_sigma", self.blur_sigma, ops.BLUR_SIGMA_MAX), ("noise_sigma", self.noise_sigma, ops.NOISE_SIGMA_MAX),
                                    ("jpeg_quality", self.jpeg_quality, 100)):
            if len(getattr(self, name)) != 2 or not 0 < lo <= hi <= top:
                raise ValueError("Degradation: %s must be a (lo, hi) pair with 0 < lo <= hi <= %g, got %r" % (name, top, getattr(self, name)))
        for name in ("blur_prob", "noise_prob", "jpeg_prob"):
            if not 0.0 <= getattr(self, name) <= 1.0:
                raise ValueError("Degradation: %s must be a probability, got %r" % (name, getattr(self, name)))
        if self.jpeg_subsampling not in ops.JPEG_SUBSAMPLINGS:
            raise ValueError("Degradation: jpeg_subsampling must be one of %s, got %r" % (ops.JPEG_SUBSAMPLINGS, jpeg_subsampling))
        self.seed = seed
        self.rng = random.Random(seed)
        # the high-order model: all of it off by default, its draws from a second stream
        bank = dict(kernel_size=kernel_size, kernel_kinds=kernel_kinds, kernel_sigma=kernel_sigma, kernel_beta_generalized=kernel_beta_generalized,
                    kernel_beta_plateau=kernel_beta_plateau, sinc_prob=sinc_prob)
        self.first = _Round("", bank, kernel_prob=kernel_prob, noise_shot_prob=noise_shot_prob, noise_shot_gain=noise_shot_gain,
                            noise_grey_prob=noise_grey_prob)
        second = dict(second or {})
        unknown = sorted(set(second) - set(SECOND_KEYS))
        if unknown:
            raise ValueError("Degradation: unknown key(s) %s of `second` (known: %s)" % (unknown, ", ".join(SECOND_KEYS)))
        self.second = _Round("second.", {k: second.pop(k) for k in _BANK_KEYS if k in second}, **second)
        lo, hi = (int(v) for v in final_sinc_size)
        self.final_sinc_sizes = [k for k in range(lo, hi + 1) if k % 2 == 1]
        if not self.final_sinc_sizes or self.final_sinc_sizes[0] < 1 or self.final_sinc_sizes[-1] > kernel_bank.MAX_SIZE:
            raise ValueError("Degradation: final_sinc_size must be a (lo, hi) pair holding an odd size in 1..%d, got %r"
                             % (kernel_bank.MAX_SIZE, final_sinc_size))
        self.final_sinc_size = (lo, hi)
        self.resize_filters = tuple(float(v) for v in resize_filters)
        if len(self.resize_filters) != len(RESIZE_FILTERS) or min(self.resize_filters) < 0 or not sum(self.resize_filters) > 0:
            raise ValueError("Degradation: resize_filters must hold %d non-negative weights (%s), not all 0, got %r"
                             % (len(RESIZE_FILTERS), ", ".join(RESIZE_FILTERS), resize_filters))
        self.final_sinc_prob = _prob("final_sinc_prob", final_sinc_prob)
        self.rng2 = random.Random((int(seed) * HO_STREAM_MULTIPLIER) & 0xffffffffffffffff)

    # which high-order launches a batch takes: a matter of the configuration alone
    hr_blur = property(lambda self: self.first.kernel_prob > 0)
    lr_from_hr = property(lambda self: self.hr_blur or self.resize_filters[1] > 0 or self.resize_filters[2] > 0)
    noise_kinds = property(lambda self: self.noise_prob > 0 and (self.first.noise_shot_prob > 0 or self.first.noise_grey_prob > 0))
    final_sinc = property(lambda self: self.final_sinc_prob > 0)

    @property
    def high_order(self):
        s = self.second
        return self.lr_from_hr or self.noise_kinds or s.kernel_prob > 0 or s.noise_prob > 0 or s.jpeg_prob > 0 or self.final_sinc

    @property
    def enabled(self):
        return self.blur_prob > 0 or self.noise_prob > 0 or self.jpeg_prob > 0 or self.high_order

    def draw(self, n):
        """Per-sample parameters of a batch of n.  Order per sample: blur decision, sigma, noise decision, sigma_n, two seed words, JPEG
        decision, q -- every draw is made whether or not its stage fires, so one stage's probability does not shift another's values."""
        p = DegradeParams([], [], [], [])
        rng = self.rng
        for _ in range(n):
            on, s = rng.random() < self.blur_prob, rng.uniform(*self.blur_sigma)
            p.blur_sigma.append(s if on else 0.0)
            on, s = rng.random() < self.noise_prob, rng.uniform(*self.noise_sigma)
            p.noise_sigma.append(s if on else 0.0)
            p.seeds.append((rng.getrandbits(32), rng.getrandbits(32)))
            on, q = rng.random() < self.jpeg_prob, rng.randint(*self.jpeg_quality)
            p.quality.append(q if on else 0)
        if not self.high_order:
            return p
        p = DegradeParamsHO(*p)
        p.ho = self.draw_high_order(p)
        return p

    def draw_high_order(self, p):
        """The high-order draws that go with the first-order parameters `p`, from the SECOND stream (the first one does not move when a
        new stage is switched on).  Per sample, always all of: kernel 1 (decision, nine bank variates), the resize filter, the noise
        kind (shot decision, gain, grey decision); second round: kernel 2, noise (decision, sigma, kind, two seed words), JPEG (decision,
        q); final sinc (decision, size, omega, the coin that puts it before or behind the last JPEG)."""
        rng, first, second = self.rng2, self.first, self.second
        ho = HighOrderParams([], [], [], [], [], [], [], [], [])
        sizes = self.final_sinc_sizes
        for i in range(len(p.quality)):
            ho.kernel1.append(first.draw_kernel(rng))
            u, pick, acc = rng.random() * sum(self.resize_filters), len(RESIZE_FILTERS) - 1, 0.0
            for f, wt in enumerate(self.resize_filters):
                acc += wt
                if u < acc:
                    pick = f
                    break
            ho.resize.append(pick)
            ho.noise1.append(_noise_of(p.noise_sigma[i], first.draw_kind(rng)))
            ho.kernel2.append(second.draw_kernel(rng))
            on, sg = rng.random() < second.noise_prob, rng.uniform(*second.noise_sigma)
            ho.noise2.append(_noise_of(sg if on else 0.0, second.draw_kind(rng)))
            ho.seeds2.append((rng.getrandbits(32), rng.getrandbits(32)))
            lo, hi = second.jpeg_quality                            # one variate each: randint / randrange would consume a varying number
            on, q = rng.random() < second.jpeg_prob, lo + int(rng.random() * (hi - lo + 1))
            ho.quality2.append(q if on else 0)
            on, size = rng.random() < self.final_sinc_prob, sizes[int(rng.random() * len(sizes))]
            sinc, before = kernel_bank.draw_sinc(rng, size), rng.random() < 0.5
            ho.sinc_a.append(sinc if on and before else None)
            ho.sinc_b.append(sinc if on and not before else None)
        return ho

    def _layout(self, n):
        """[(name, first word, words)] of the high-order block behind the DEGRADE_WORDS block: only the configured stages are there."""
        s, F, K = self.second, ops.FILTER2D_WORDS * n, ops.NOISE_KIND_WORDS * n
        parts = [("kernel1", F, self.hr_blur), ("resize", n, self.lr_from_hr), ("noise1", K, self.noise_kinds), ("kernel2", F, s.kernel_prob > 0),
                 ("noise2", K, s.noise_prob > 0), ("sinc_a", F, self.final_sinc), ("quality2", n, s.jpeg_prob > 0), ("sinc_b", F, self.final_sinc)]
        out, at = [], ops.DEGRADE_WORDS * n
        for name, size, on in parts:
            if on:
                out.append((name, at, size))
                at += size
        return out, at + (at & 1)                                   # an even count: the block travels as int64 words

    def words(self, params):
        """The parameters as the int32 words the kernels read (ops.degrade_words), ready for one host-to-device copy; with a high-order
        stage configured its words (tap tables, radii, table indices, strengths, flags, seeds, qualities) follow in the same array."""
        n = len(params.quality)
        base = ops.degrade_words(n, params.blur_sigma, params.noise_sigma, params.seeds, params.quality)
        if not self.high_order:
            return base
        ho = params.ho
        layout, total = self._layout(n)
        words = np.zeros(total, dtype=np.int32)
        words[:base.size] = base
        for name, at, size in layout:
            if name in ("kernel1", "kernel2", "sinc_a", "sinc_b"):
                part = ops.filter2d_words(n, [kernel_bank.build(k) for k in getattr(ho, name)])
            elif name == "resize":
                part = np.asarray(ho.resize, dtype=np.int32)
            elif name == "noise1":
                part = ops.noise_kind_words(n, [v[0] for v in ho.noise1], [v[1] for v in ho.noise1], params.seeds)
            elif name == "noise2":
                part = ops.noise_kind_words(n, [v[0] for v in ho.noise2], [v[1] for v in ho.noise2], ho.seeds2)
            else:
                part = np.asarray(ho.quality2, dtype=np.int32)
            words[at:at + size] = part
        return words

    def apply_high_order(self, lr, hr, params, tables, dev_words=None):
        """The whole order of a batch with a high-order stage configured: filter2d(k1) on hr -> resize_select -> lr
        (else the crop kernel's lr), the first-order blur -> noise (Gaussian or shot, colour or grey) -> JPEG, then the second round
        filter2d(k2) -> noise -> filter2d(sinc_a) -> JPEG -> filter2d(sinc_b).  `tables`: the ops.ResizeTables of the data set's three
        down-scale filters (only read when lr is made from hr).  The launches depend on the configuration alone."""
        n = lr.shape[0]
        if dev_words is None:
            dev_words = ops.upload_words(self.words(params), lr.device)
        base = dev_words[:ops.DEGRADE_WORDS * n]
        part = {name: dev_words[at:at + size] for name, at, size in self._layout(n)[0]}
        if self.lr_from_hr:
            src = ops.filter2d_dev(hr, part["kernel1"]) if self.hr_blur else hr
            lr = ops.resize_select_dev(src, tables, part["resize"])
        if self.noise_kinds:
            if self.blur_prob > 0:
                lr = ops.degrade_blur_noise_dev(lr, base, blur=True, noise=False)
            lr = ops.degrade_noise_kinds_dev(lr, part["noise1"])
        elif self.blur_prob > 0 or self.noise_prob > 0:
            lr = ops.degrade_blur_noise_dev(lr, base, blur=self.blur_prob > 0, noise=self.noise_prob > 0)
        if self.jpeg_prob > 0:
            lr = ops.jpeg_roundtrip_dev(lr, base, self.jpeg_subsampling)
        if "kernel2" in part:
            lr = ops.filter2d_dev(lr, part["kernel2"])
        if "noise2" in part:
            lr = ops.degrade_noise_kinds_dev(lr, part["noise2"])
        if "sinc_a" in part:
            lr = ops.filter2d_dev(lr, part["sinc_a"])
        if "quality2" in part:
            lr = ops.jpeg_quality_dev(lr, part["quality2"], self.jpeg_subsampling)
        if "sinc_b" in part:
            lr = ops.filter2d_dev(lr, part["sinc_b"])
        return lr

    def apply(self, lr, params, dev_words=None):
        """Runs the stages on lr (N,3,l,l): at most two launches for blur + noise, one for JPEG.  Which launches run depends on the
        probabilities alone, never on the draw: a sample whose stage did not fire is copied by the same launch.  `dev_words`:
        words(params) already on the device (the loader sends them with the batch descriptors); else one pinned, non-blocking copy is
        made here."""
        if dev_words is None:
            dev_words = ops.upload_words(self.words(params), lr.device)
        if self.blur_prob > 0 or self.noise_prob > 0:
            lr = ops.degrade_blur_noise_dev(lr, dev_words, blur=self.blur_prob > 0, noise=self.noise_prob > 0)
        if self.jpeg_prob > 0:
            lr = ops.jpeg_roundtrip_dev(lr, dev_words, self.jpeg_subsampling)
        return lr


class Augmentation:
    """Random flips and 90-degree rotations of the training crops on the device: with dihedral=True every sample gets
    one of the 8 transform codes of ops.DIHEDRAL_INVERSE's table, drawn uniformly, and hr / lr are cut from D_k(crop)
    (fsr_crop_resize_aug).  The draws come from this object's OWN random.Random: the index, crop and degradation streams of
    DeviceBatchLoader do not move when it is switched on."""

    def __init__(self, dihedral=True, seed=0):
        self.dihedral = bool(dihedral)
        self.seed = seed
        self.rng = random.Random(seed)

    @property
    def enabled(self):
        return self.dihedral

    def draw(self, n):
        """The transform codes of a batch of n samples."""
        return [self.rng.randrange(8) for _ in range(n)]


class NumpyImagesDataset(torch.utils.data.Dataset):
    def __init__(self, numpy_paths, lr_image_size, scale_factor, device="cuda"):
        self.numpy_paths = list(numpy_paths)
        self.lr_image_size = lr_image_size
        self.hr_image_size = lr_image_size * scale_factor
        self.scale_factor = scale_factor
        self.device = torch.device(device)
        self._images = [None] * len(self.numpy_paths)
        xmin, xsize, w, self._kmax = aa_bicubic_taps(self.hr_image_size, self.lr_image_size)
        self._xmin = torch.from_numpy(xmin).to(self.device)
        self._xsize = torch.from_numpy(xsize).to(self.device)
        self._w = torch.from_numpy(w).to(self.device)
        self._resize_tables = None

    def __len__(self):
        return len(self.numpy_paths)

    def resize_tables(self):
        """The ops.ResizeTables of RESIZE_FILTERS for hr -> lr, built on first use (fsr_resize_select)."""
        if self._resize_tables is None:
            tables = [resize_taps(self.hr_image_size, self.lr_image_size, kind) for kind in RESIZE_FILTERS]
            self._resize_tables = ops.ResizeTables(tables, tables, self.hr_image_size, self.hr_image_size, self.device)
        return self._resize_tables

    def _image(self, idx):
        img = self._images[idx]
        if img is None:
            arr = np.load(self.numpy_paths[idx], mmap_mode="r")       # uint8 (3,H,W), train.py:29-31
            if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[0] != 3:
                raise ValueError("%s: expected a uint8 (3,H,W) array" % self.numpy_paths[idx])
            img = torch.from_numpy(np.array(arr)).to(self.device)
            self._images[idx] = img
        return img

    def draw_crop(self, idx, rng=random):
        """dataloader.py:27-29: two inclusive randint draws, crop_h first."""
        _, h, w = self._image(idx).shape
        return rng.randint(0, h - self.hr_image_size), rng.randint(0, w - self.hr_image_size)

    def batch(self, indices, crops, degrade=None, xforms=None):
        """(lr, hr) float32 NCHW device batches for image `indices` cropped at `crops` [(y, x), ...].
        The per-sample descriptors (image pointer, height, width, crop origin) travel as ONE pinned, non-blocking
        host-to-device copy; nothing here waits for the device.
        degrade: a (Degradation, parameters it drew for this batch) pair -- lr then goes through its stages; the parameter
        words ride at the end of the same copy.
        xforms: one transform code 0..7 per sample -- hr and lr are then cut from D_k(crop) by fsr_crop_resize_aug, the
        codes riding in the same copy, and the degradation runs on that lr; None: fsr_crop_resize, as ever."""
        n = len(indices)
        imgs = [self._image(i) for i in indices]
        if xforms is not None:
            xforms = [int(k) for k in xforms]
            if len(xforms) != n or any(not 0 <= k <= 7 for k in xforms):
                raise ValueError("batch: xforms must hold one transform code in 0..7 per sample, got %r" % (xforms,))
        # [n int64 pointers][4 x n int32: heights, widths, crop_y, crop_x][n int32 transform codes, padded to an even count]
        # [degradation words]  (viewed as int64 words for one copy)
        words = degrade[0].words(degrade[1]) if degrade is not None else None
        extra = 0 if words is None else words.size // 2              # ops.DEGRADE_WORDS is even, a high-order block is padded
        xw = 0 if xforms is None else (n + 1) // 2
        desc = np.empty(3 * n + xw + extra, dtype=np.int64)
        desc[:n] = [im.data_ptr() for im in imgs]
        desc[n:3 * n].view(np.int32)[:] = ([im.shape[1] for im in imgs] + [im.shape[2] for im in imgs]
                                           + [c[0] for c in crops] + [c[1] for c in crops])
        if xw:
            desc[3 * n:3 * n + xw].view(np.int32)[:] = xforms + [0] * (2 * xw - n)
        if extra:
            desc[3 * n + xw:].view(np.int32)[:] = words
        host = torch.from_numpy(desc)
        if self.device.type == "cuda":
            host = host.pin_memory()
        dev_desc = host.to(self.device, non_blocking=True)
        meta = dev_desc[n:3 * n].view(torch.int32).view(4, n)
        hr, lr = self.hr_image_size, self.lr_image_size
        hr_out = torch.empty((n, 3, hr, hr), dtype=torch.float32, device=self.device)
        lr_out = torch.empty((n, 3, lr, lr), dtype=torch.float32, device=self.device)
        tmp = torch.empty((n, 3, hr, lr), dtype=torch.float32, device=self.device)
        if xforms is None:
            L.check(L.lib().fsr_crop_resize(_p(dev_desc), _p(meta[0]), _p(meta[1]), _p(meta[2]), _p(meta[3]), n, hr,
                                            self.scale_factor, _p(self._w), _p(self._xmin), _p(self._xsize), self._kmax,
                                            _p(hr_out), _p(lr_out), _p(tmp), _stream()), "fsr_crop_resize")
        else:
            codes = dev_desc[3 * n:3 * n + xw].view(torch.int32)
            L.check(L.lib().fsr_crop_resize_aug(_p(dev_desc), _p(meta[0]), _p(meta[1]), _p(meta[2]), _p(meta[3]), _p(codes), n, hr,
                                                self.scale_factor, _p(self._w), _p(self._xmin), _p(self._xsize), self._kmax,
                                                _p(hr_out), _p(lr_out), _p(tmp), _stream()), "fsr_crop_resize_aug")
        if degrade is not None and degrade[0].high_order:
            lr_out = degrade[0].apply_high_order(lr_out, hr_out, degrade[1], self.resize_tables() if degrade[0].lr_from_hr else None,
                                                 dev_desc[3 * n + xw:].view(torch.int32))
        elif degrade is not None:
            lr_out = degrade[0].apply(lr_out, degrade[1], dev_desc[3 * n + xw:].view(torch.int32))
        return lr_out, hr_out

    def __getitem__(self, idx):
        lr, hr = self.batch([idx], [self.draw_crop(idx)])
        return lr[0], hr[0]


class DeviceBatchLoader:
    """Iterable of device batches.

    Default (training, train.py:69-80,92-113): `iterations` batches whose image indices are drawn with replacement from a
    seeded torch.Generator (RandomSampler(replacement=True)), crops from a seeded `random.Random` (train.py:40-43 seeds
    python's RNG per worker).  sequential=True (validation, train.py:81-91: shuffle=False, drop_last=True): ONE pass over
    the data set in order, len(dataset) // batch_size batches, fresh random crops.  Under data parallelism each rank
    passes seed + rank.  degradation: a Degradation (with its own seed) applied to every lr batch; None, or one whose
    probabilities are all 0, leaves every batch and every launch as it is.  augmentation: an Augmentation (with its own seed) whose
    codes transform every crop before the down-scale and the degradation; None, or one with nothing switched on, likewise changes
    nothing -- the state dictionary included, which gains its "augmentation" entry only when one is set, and its
    "degradation_high_order" entry (the degradation's second stream) only when a high-order stage is configured.
    state_dict() / load_state_dict(): the three random streams and the batches already yielded -- a restored loader yields the
    REMAINING batches of the interrupted pass, the very ones the uninterrupted loader would have, and then stops."""

    def __init__(self, dataset, batch_size, iterations=None, seed=1234, sequential=False, degradation=None, augmentation=None):
        self.dataset, self.batch_size, self.sequential = dataset, batch_size, sequential
        self.degradation = degradation if degradation is not None and degradation.enabled else None
        self.augmentation = augmentation if augmentation is not None and augmentation.enabled else None
        self.iterations = len(dataset) // batch_size if sequential else iterations
        if self.iterations is None:
            raise ValueError("DeviceBatchLoader needs `iterations` unless sequential=True")
        if sequential and self.iterations == 0:
            # the reference's DataLoader(drop_last=True) behaves the same way (train.py:81-91), but silently: SSIM / PSNR are
            # then never logged and no fixed validation images exist
            import warnings
            warnings.warn("DeviceBatchLoader(sequential=True): %d images give no full batch of %d -- validation metrics and the "
                          "fixed validation images will be skipped (drop_last semantics of train.py:81-91)" % (len(dataset), batch_size))
        self.gen = torch.Generator().manual_seed(seed)
        self.rng = random.Random(seed)
        self._yielded, self._resume_at = 0, 0

    def __len__(self):
        return self.iterations

    def state_dict(self):
        sd = {"generator": self.gen.get_state(), "rng": self.rng.getstate(), "yielded": self._yielded,
              "degradation": None if self.degradation is None else self.degradation.rng.getstate()}
        if self.augmentation is not None:
            sd["augmentation"] = self.augmentation.rng.getstate()
        if self.degradation is not None and self.degradation.high_order:
            sd["degradation_high_order"] = self.degradation.rng2.getstate()
        return sd

    def load_state_dict(self, sd):
        if (sd["degradation"] is None) != (self.degradation is None):
            raise ValueError("DeviceBatchLoader.load_state_dict: the state was saved %s a degradation, this loader runs %s one"
                             % (("without", "with") if sd["degradation"] is None else ("with", "without")))
        if (sd.get("augmentation") is None) != (self.augmentation is None):
            raise ValueError("DeviceBatchLoader.load_state_dict: the state was saved %s an augmentation, this loader runs %s one"
                             % (("without", "with") if sd.get("augmentation") is None else ("with", "without")))
        high_order = self.degradation is not None and self.degradation.high_order
        if (sd.get("degradation_high_order") is None) == high_order:
            raise ValueError("DeviceBatchLoader.load_state_dict: the state was saved %s a high-order degradation stage, this loader runs %s one"
                             % (("with", "without") if not high_order else ("without", "with")))
        self.gen.set_state(sd["generator"])
        self.rng.setstate(sd["rng"])
        if high_order:
            self.degradation.rng2.setstate(sd["degradation_high_order"])
        if self.augmentation is not None:
            self.augmentation.rng.setstate(sd["augmentation"])
        if self.degradation is not None:
            self.degradation.rng.setstate(sd["degradation"])
        self._yielded = int(sd["yielded"])
        self._resume_at = self._yielded if self._yielded < self.iterations or not self.sequential else 0   # a finished validation pass starts over

    def __iter__(self):
        start, self._resume_at = self._resume_at, 0
        for it in range(start, self.iterations):
            self._yielded = it + 1
            if self.sequential:
                idx = list(range(it * self.batch_size, (it + 1) * self.batch_size))
            else:
                idx = torch.randint(len(self.dataset), (self.batch_size,), generator=self.gen).tolist()
            crops = [self.dataset.draw_crop(i, self.rng) for i in idx]
            degrade = None if self.degradation is None else (self.degradation, self.degradation.draw(len(idx)))
            if self.augmentation is not None:
                yield self.dataset.batch(idx, crops, degrade, self.augmentation.draw(len(idx)))
            elif degrade is None:
                yield self.dataset.batch(idx, crops)
            else:
                yield self.dataset.batch(idx, crops, degrade)
