"""Flip / rotate training augmentation on the device: fsr_crop_resize_aug against the plain fsr_crop_resize on a
data set that holds the transformed images (built with numpy), bit for bit; and the loader's streams, state and configuration."""
import importlib
import random

import numpy as np
import pytest
import torch

from backend import BACKENDS, select
from yuv_contract import ns

dataloader = importlib.import_module("fast-srgan_amd.dataloader")
train = importlib.import_module("fast-srgan_amd.train")

LR, SCALE = 6, 4
HR = LR * SCALE
SIZES = [(40, 56), (31, 25)]           # two images of different sizes, one with odd extents


def D_np(img, k):
    """D_k of a (3,H,W) array."""
    if k & 1:
        img = img[:, :, ::-1]
    if k & 2:
        img = img[:, ::-1, :]
    if k & 4:
        img = img.transpose(0, 2, 1)
    return np.ascontiguousarray(img)


def D_crop(y, x, h, w, k):
    """Origin, in D_k(image), of the crop that is D_k of the HR x HR crop at (y, x) of an h x w image."""
    if k & 1:
        x = w - HR - x
    if k & 2:
        y = h - HR - y
    return (x, y) if k & 4 else (y, x)


def D_t(t, k):
    """D_k of an (N,3,H,W) tensor."""
    if k & 1:
        t = t.flip(3)
    if k & 2:
        t = t.flip(2)
    if k & 4:
        t = t.transpose(2, 3)
    return t.contiguous()


def _images(seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(3, h, w), dtype=np.uint8) for h, w in SIZES]


def _dataset(tmp_path, name, images, dev):
    paths = []
    for i, img in enumerate(images):
        paths.append(str(tmp_path / ("%s_%d.npy" % (name, i))))
        np.save(paths[-1], img)
    return dataloader.NumpyImagesDataset(paths, LR, SCALE, device=dev)


@pytest.mark.parametrize("backend", BACKENDS)
def test_augmented_crop_is_the_plain_crop_of_the_transformed_image(backend, tmp_path):
    dev = select(backend)
    images = _images(41)
    plain = _dataset(tmp_path, "plain", images, dev)
    # every image at its first corner, its last legal corner and one origin in between
    idx, crops = [], []
    for i, (h, w) in enumerate(SIZES):
        for c in ((0, 0), (h - HR, w - HR), ((h - HR) // 2, 1)):
            idx.append(i)
            crops.append(c)
    lr0, hr0 = plain.batch(idx, crops)
    assert lr0.shape == (len(idx), 3, LR, LR) and hr0.shape == (len(idx), 3, HR, HR)
    per_code = []
    for k in range(8):
        lr_k, hr_k = plain.batch(idx, crops, xforms=[k] * len(idx))
        moved = _dataset(tmp_path, "d%d" % k, [D_np(img, k) for img in images], dev)
        want_lr, want_hr = moved.batch(idx, [D_crop(y, x, *SIZES[i], k) for i, (y, x) in zip(idx, crops)])
        assert torch.equal(hr_k, want_hr), k
        assert torch.equal(lr_k, want_lr), k
        assert torch.equal(hr_k, D_t(hr0, k)), k
        per_code.append((lr_k, hr_k))
    # mixed codes within one batch: every sample is its own code's sample
    codes = [(3 * j + 5) % 8 for j in range(len(idx))]
    assert len(set(codes)) >= 5
    lr_m, hr_m = plain.batch(idx, crops, xforms=codes)
    for j, k in enumerate(codes):
        assert torch.equal(lr_m[j], per_code[k][0][j]) and torch.equal(hr_m[j], per_code[k][1][j]), (j, k)
    # the switch off, and the identity code: today's batches
    for xf in (None, [0] * len(idx)):
        lr_z, hr_z = plain.batch(idx, crops, xforms=xf)
        assert torch.equal(lr_z, lr0) and torch.equal(hr_z, hr0)
    for bad in ([0] * (len(idx) - 1), [8] + [0] * (len(idx) - 1), [-1] + [0] * (len(idx) - 1)):
        with pytest.raises(ValueError, match="xforms"):
            plain.batch(idx, crops, xforms=bad)


@pytest.mark.parametrize("backend", BACKENDS)
def test_augmentation_goes_in_front_of_the_degradation(backend, tmp_path):
    """Degradations run on the augmented lr: the batch equals the degradation applied to the augmented batch's lr, with the same words."""
    dev = select(backend)
    ds = _dataset(tmp_path, "deg", _images(42), dev)
    deg = dataloader.Degradation(blur_prob=1.0, seed=3)
    params = deg.draw(2)
    lr_a, hr_a = ds.batch([0, 1], [(1, 2), (3, 0)], xforms=[5, 2])
    lr_d, hr_d = ds.batch([0, 1], [(1, 2), (3, 0)], (deg, params), [5, 2])
    assert torch.equal(hr_d, hr_a)
    assert torch.equal(lr_d, deg.apply(lr_a.clone(), params)) and not torch.equal(lr_d, lr_a)


class _Recorder:
    """A data set that records what the loader asks for."""

    def __init__(self):
        self.calls = []

    def __len__(self):
        return 5

    def draw_crop(self, i, rng=random):
        return rng.randint(0, 10 + i), rng.randint(0, 20 + i)

    def batch(self, indices, crops, degrade=None, xforms=None):
        self.calls.append((list(indices), list(crops), None if degrade is None else degrade[1], xforms))
        return len(self.calls)


def test_augmentation_has_its_own_stream():
    a, b, c = _Recorder(), _Recorder(), _Recorder()
    list(dataloader.DeviceBatchLoader(a, 4, 64, seed=9))
    list(dataloader.DeviceBatchLoader(b, 4, 64, seed=9, augmentation=dataloader.Augmentation(seed=5)))
    deg = dataloader.Degradation(noise_prob=0.5, seed=4)
    list(dataloader.DeviceBatchLoader(c, 4, 64, seed=9, degradation=deg, augmentation=dataloader.Augmentation(seed=5)))
    assert [x[:2] for x in a.calls] == [x[:2] for x in b.calls] == [x[:2] for x in c.calls]      # indices and crops do not move
    assert all(x[3] is None and x[2] is None for x in a.calls)
    codes = [k for x in b.calls for k in x[3]]
    assert len(codes) == 256 and set(codes) == set(range(8))                                    # all 8 codes in 256 draws
    assert codes == [k for x in c.calls for k in x[3]]                                          # nor does the degradation move them
    d = _Recorder()
    list(dataloader.DeviceBatchLoader(d, 4, 64, seed=9, degradation=dataloader.Degradation(noise_prob=0.5, seed=4)))
    assert [x[2] for x in d.calls] == [x[2] for x in c.calls]                                   # and the reverse
    assert codes != [k for x in _codes_of(seed=6) for k in x]                                   # another seed, other codes
    off = dataloader.DeviceBatchLoader(_Recorder(), 4, 2, seed=9, augmentation=dataloader.Augmentation(dihedral=False))
    assert off.augmentation is None                                                             # nothing switched on: no augmentation


def _codes_of(seed):
    r = _Recorder()
    list(dataloader.DeviceBatchLoader(r, 4, 64, seed=9, augmentation=dataloader.Augmentation(seed=seed)))
    return [x[3] for x in r.calls]


@pytest.mark.parametrize("backend", BACKENDS)
def test_loader_state_round_trip(backend, tmp_path):
    dev = select(backend)
    ds = _dataset(tmp_path, "state", _images(43), dev)

    def make(aug=True):
        return dataloader.DeviceBatchLoader(ds, 3, 5, seed=11, augmentation=dataloader.Augmentation(seed=12) if aug else None)

    whole = list(make())
    first = make()
    it = iter(first)
    head = [next(it), next(it)]
    state = first.state_dict()
    assert sorted(state) == ["augmentation", "degradation", "generator", "rng", "yielded"]
    second = make()
    second.load_state_dict(state)
    rest = list(second)
    assert len(rest) == 3
    for (lr_a, hr_a), (lr_b, hr_b) in zip(whole, head + rest):
        assert torch.equal(lr_a, lr_b) and torch.equal(hr_a, hr_b)
    plain_state = make(aug=False).state_dict()
    assert sorted(plain_state) == ["degradation", "generator", "rng", "yielded"]                # today's keys exactly
    with pytest.raises(ValueError, match="saved with an augmentation"):
        make(aug=False).load_state_dict(state)
    with pytest.raises(ValueError, match="saved without an augmentation"):
        make().load_state_dict(plain_state)
    # the augmented pass is not the plain one (the codes are drawn), but its crops are
    plain = list(make(aug=False))
    assert any(not torch.equal(a[1], b[1]) for a, b in zip(whole, plain))


def _config(**augment):
    data = ns(lr_image_size=LR, scale_factor=SCALE)
    if augment:
        data.augment = ns(**augment)
    return ns(experiment=ns(seed=21), data=data, training=ns(batch_size=2, pretrain_iterations=3, iterations=4))


def test_train_builds_augmented_training_loaders_only():
    ds = _Recorder()
    val, pre, trn = train.build_loaders(_config(dihedral=True), ds)
    assert val.augmentation is None and val.sequential
    assert pre.augmentation is not None and trn.augmentation is not None
    assert pre.augmentation.seed != trn.augmentation.seed
    assert train.build_loaders(_config(dihedral=True), ds, rank=1)[2].augmentation.seed != trn.augmentation.seed
    for cfg in (_config(), _config(dihedral=False)):
        assert all(ld.augmentation is None for ld in train.build_loaders(cfg, ds))
    with pytest.raises(ValueError, match=r"unknown data\.augment key\(s\) \['foo'\]"):
        train.build_loaders(_config(dihedral=True, foo=1), ds)
    with pytest.raises(ValueError, match="true or false"):
        train.build_loaders(_config(dihedral=3), ds)


def test_config_override_reaches_the_loader_factory():
    config = importlib.import_module("fast-srgan_amd.config")
    cfg = config.load_config(None, ["data.augment.dihedral=true", "training.batch_size=2"])
    assert cfg.data.augment.dihedral is True
    assert train.make_augmentation(cfg, 5).dihedral and train.make_augmentation(config.load_config(None), 5) is None
    with pytest.raises(ValueError, match="unknown data.augment"):
        train.make_augmentation(config.load_config(None, ["data.augment.foo=1"]), 5)
