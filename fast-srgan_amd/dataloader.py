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


DegradeParams = collections.namedtuple("DegradeParams", "blur_sigma noise_sigma seeds quality")   # lists of n; 0 = the stage is off


class Degradation:
    """Random degradation of the LR batch on the device: LR = JPEG(blur(LR) + noise), each stage with its own probability and a
    strength drawn uniformly per sample (csrc/degrade.hip).  blur_sigma in LR pixels (0 < sigma <= 3), noise_sigma in
    8-bit code units (<= 25), jpeg_quality integers in 1..100.  The draws come from this object's OWN random.Random: the crop and index
    streams of DeviceBatchLoader do not move when it is switched on."""

    def __init__(self, blur_sigma=(0.2, 2.0), blur_prob=0., noise_sigma=(1.0, 10.0), noise_prob=0., jpeg_quality=(30, 95), jpeg_prob=0.,
                 jpeg_subsampling="420", seed=0):
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

    @property
    def enabled(self):
        return self.blur_prob > 0 or self.noise_prob > 0 or self.jpeg_prob > 0

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
        return p

    def words(self, params):
        """The parameters as the int32 words the kernels read (ops.degrade_words), ready for one host-to-device copy."""
        return ops.degrade_words(len(params.quality), params.blur_sigma, params.noise_sigma, params.seeds, params.quality)

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

    def __len__(self):
        return len(self.numpy_paths)

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
        extra = 0 if words is None else words.size // 2              # ops.DEGRADE_WORDS is even
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
        if degrade is not None:
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
    nothing -- the state dictionary included, which gains its "augmentation" entry only when one is set.
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
        return sd

    def load_state_dict(self, sd):
        if (sd["degradation"] is None) != (self.degradation is None):
            raise ValueError("DeviceBatchLoader.load_state_dict: the state was saved %s a degradation, this loader runs %s one"
                             % (("without", "with") if sd["degradation"] is None else ("with", "without")))
        if (sd.get("augmentation") is None) != (self.augmentation is None):
            raise ValueError("DeviceBatchLoader.load_state_dict: the state was saved %s an augmentation, this loader runs %s one"
                             % (("without", "with") if sd.get("augmentation") is None else ("with", "without")))
        self.gen.set_state(sd["generator"])
        self.rng.setstate(sd["rng"])
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
