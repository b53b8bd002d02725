"""Self-ensemble inference: the member-input and accumulate kernels against torch index operations bit for bit,
the generator and pipeline routes against the composition a user would write in torch, equivariance within a derived bound, and
the argument checks of the new entry points.  Every reference is torch.flip / transpose and float32 adds, never the code under test."""
import numpy as np
import pytest
import torch

from backend import BACKENDS, L, ops, select
from yuv_contract import _shipped, _tiny

INVERSE = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 5, 7: 7}
# (n, h, w): odd sizes; one past a 32- and a 64-wide tile edge; single rows and columns
SHAPES = [(2, 5, 7), (1, 33, 65), (3, 1, 9), (1, 9, 1)]
GPU_SHAPE = (2, 70, 130)        # several tiles on both axes, partial ones at both edges


def _shapes(dev):
    return SHAPES + ([GPU_SHAPE] if dev.type == "cuda" else [])


def D(x, k):
    """D_k of an (N,H,W,C) tensor: flip W if k & 1, flip H if k & 2, then transpose H and W if k & 4."""
    if k & 1:
        x = x.flip(2)
    if k & 2:
        x = x.flip(1)
    if k & 4:
        x = x.transpose(1, 2)
    return x.contiguous()


def cast_u8(mean):
    """The project's cast: (unsigned char)(clamp((m + 1) / 2, 0, 1) * 255), truncating -- forward_u8's bytes for m in [-1, 1]."""
    return (((mean + 1.0) / 2.0).clamp(0.0, 1.0) * 255.0).to(torch.uint8)


def ref_mean(ys, inverse=INVERSE):
    """Sequential float32 sum in code order of the 8 member outputs (each (N,.,.,3)) through the inverse table, times 0.125."""
    s = D(ys[0], inverse[0])
    for k in range(1, 8):
        s = s + D(ys[k], inverse[k])
    return s * 0.125


def _frames(dev, n, h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)).to(dev)


def test_the_inverse_table_is_the_wrappers():
    assert tuple(INVERSE[k] for k in range(8)) == ops.DIHEDRAL_INVERSE
    x = torch.arange(2 * 3 * 5 * 3, dtype=torch.float32).reshape(2, 3, 5, 3)
    for k in range(8):
        assert torch.equal(D(D(x, k), INVERSE[k]), x)
    assert not torch.equal(D(D(x, 5), 5), x)            # 5 is not its own inverse


# ------------------------------------------------------------------------------------------------ 1. member input
@pytest.mark.parametrize("backend", BACKENDS)
def test_member_input_is_an_exact_permutation(backend):
    dev = select(backend)
    for n, h, w in _shapes(dev):
        u8 = _frames(dev, n, h, w, 31)
        img = ops.u8_to_image(u8).permute(0, 2, 3, 1)                      # the float NHWC buffer
        assert img.is_contiguous()
        for src in (u8, img):
            for g0 in (0, 4):
                got = ops.dihedral_members(src, g0, g0 + 3).permute(0, 2, 3, 1)
                assert got.is_contiguous() and got.dtype == torch.float32
                want = torch.cat([D(img, k) for k in range(g0, g0 + 4)])
                assert got.shape == want.shape and torch.equal(got, want), (n, h, w, src.dtype, g0)
            sub = ops.dihedral_members(src, 5, 6).permute(0, 2, 3, 1)       # a sub-range of the transposed group
            assert torch.equal(sub, torch.cat([D(img, 5), D(img, 6)])), (n, h, w, src.dtype)
            one = ops.dihedral_members(src, 2, 2).permute(0, 2, 3, 1)
            assert torch.equal(one, D(img, 2)), (n, h, w, src.dtype)


# ------------------------------------------------------------------------------------------------ 2. accumulate
def _accumulate(ys, n, per, kind):
    """The 8 members through ops.dihedral_accumulate, `per` members per launch."""
    acc = torch.full((n,) + tuple(ys[0].shape[1:]), float("nan"), dtype=torch.float32, device=ys[0].device)
    out = None
    for g0 in (0, 4):
        for k0 in range(g0, g0 + 4, per):
            out = ops.dihedral_accumulate(torch.cat(ys[k0:k0 + per]), k0, k0 + per - 1, acc, kind)
            assert (out is not None) == (k0 + per - 1 == 7)
    return out


@pytest.mark.parametrize("backend", BACKENDS)
def test_accumulate_is_the_sequential_sum_through_the_inverses(backend):
    dev = select(backend)
    g = torch.Generator().manual_seed(32)
    for n, h, w in _shapes(dev):
        ys = [(torch.rand((n, h, w, 3) if k < 4 else (n, w, h, 3), generator=g) * 2 - 1).to(dev) for k in range(8)]
        want = ref_mean(ys)
        # negative control: with the inverses of 5 and 6 swapped the reference is another image, so the comparison sees that bug
        swapped = dict(INVERSE)
        swapped[5], swapped[6] = 5, 6
        if h != w:
            assert not torch.equal(ref_mean(ys, swapped), want), (n, h, w)
        for per in (4, 2, 1):
            got = _accumulate(ys, n, per, "f32")
            assert got.shape == (n, 3, h, w) and got.permute(0, 2, 3, 1).is_contiguous()
            assert torch.equal(got.permute(0, 2, 3, 1), want), (n, h, w, per)
            got8 = _accumulate(ys, n, per, "u8")
            assert got8.dtype == torch.uint8 and torch.equal(got8, cast_u8(want)), (n, h, w, per)


@pytest.mark.parametrize("backend", BACKENDS)
def test_cast_reaches_both_ends(backend):
    """All members -1 or all +1: the mean is exact and the bytes are 0 and 255."""
    dev = select(backend)
    for v, byte in ((-1.0, 0), (1.0, 255)):
        ys = [torch.full((1, 3, 4, 3) if k < 4 else (1, 4, 3, 3), v, device=dev) for k in range(8)]
        assert bool((_accumulate(ys, 1, 4, "u8") == byte).all())


# ------------------------------------------------------------------------------------------------ 3. generator level
def _composition(G, u8):
    """What a user composes in torch: the two member batches at batch 4N through G.forward, the reference sum."""
    n = u8.shape[0]
    img = ops.u8_to_image(u8).permute(0, 2, 3, 1)
    ys = []
    for g0 in (0, 4):
        x = torch.cat([D(img, k) for k in range(g0, g0 + 4)]).permute(0, 3, 1, 2)
        y = G.forward(x).permute(0, 2, 3, 1)
        ys += [y[j * n:(j + 1) * n] for j in range(4)]
    return ref_mean(ys)


def _assert_generator_routes(G, dev, monkeypatch):
    u8 = _frames(dev, 2, 8, 12, 33)
    with torch.no_grad():
        want = _composition(G, u8)
        x = ops.u8_to_image(u8)
        got = G.forward(x, ensemble=True)
        assert got.shape == (2, 3, 32, 48) and torch.equal(got.permute(0, 2, 3, 1), want)
        assert torch.equal(G.forward(x.contiguous(), ensemble=True), got)                 # an NCHW-dense input too
        assert torch.equal(G.forward_u8(u8, ensemble=True), cast_u8(want))
        assert not torch.equal(G.forward_u8(u8, ensemble=True), G.forward_u8(u8))         # (it is another image than the plain one)
        # the tail in row bands: 16 (24 for the transposed group) rows of the tail's input in windows of 4 core rows
        assert len(ops.tail_windows(16, 4)) == 4 and len(ops.tail_windows(24, 4)) == 6
        assert torch.equal(G.forward_u8(u8, bands=4, ensemble=True), cast_u8(want))
        assert torch.equal(G.forward(x, bands=4, ensemble=True).permute(0, 2, 3, 1), want)
        # another output size: the float mean through the resampler
        assert torch.equal(G.forward_u8(u8, out_size=(30, 50), ensemble=True), ops.resample_image(want, 30, 50, "u8"))
        # members in chunks of 2N: InstanceNorm is per image, so the bytes do not change
        batches = []
        real = G._forward
        monkeypatch.setattr(G, "max_batch", lambda h, w, bands=False: 4)
        monkeypatch.setattr(G, "_forward", lambda x, cfg, bands=None: (batches.append(x.shape[0]), real(x, cfg, bands))[1])
        assert torch.equal(G.forward_u8(u8, ensemble=True), cast_u8(want))
        assert batches == [4, 4, 4, 4]
        monkeypatch.setattr(G, "max_batch", lambda h, w, bands=False: 1)
        with pytest.raises(ValueError, match="too large"):
            G.forward_u8(u8, ensemble=True)
    monkeypatch.undo()
    with torch.enable_grad(), pytest.raises(L.FsrError, match="no gradient"):
        G.forward(ops.u8_to_image(u8), ensemble=True)


@pytest.mark.parametrize("backend", BACKENDS)
def test_generator_ensemble_is_the_torch_composition_f32(pkg, backend, monkeypatch):
    dev = select(backend)
    _assert_generator_routes(_tiny(pkg, dev), dev, monkeypatch)


@pytest.mark.gpu
def test_generator_ensemble_is_the_torch_composition_f16_gpu(pkg, monkeypatch):
    dev = select("hip")
    _assert_generator_routes(_shipped(pkg, dev, "f16"), dev, monkeypatch)


# ------------------------------------------------------------------------------------------------ 4. equivariance
def _assert_equivariance(G, dev):
    """forward(D_k(x), ensemble) against D_k(forward(x, ensemble)): the 8 members of D_k(x) are the 8 members of x, so the two sides
    are float32 sums of the same 8 terms of magnitude <= 1 (tanh) in different orders.  Each sum is within 7 * 2^-24 * sum|y| <=
    7 * 2^-24 * 8 of exact; after the 0.125 the sides differ by at most 14 * 2^-24 = 8.4e-7.  Gate: 1e-6."""
    x = ops.u8_to_image(_frames(dev, 2 if dev.type == "cuda" else 1, 8, 12, 34))      # (the emulator is slow: one frame there)
    with torch.no_grad():
        # the premise: an image's output bits do not depend on its position in the batch
        x2 = torch.cat([x, x.flip(3)])
        assert torch.equal(G.forward(x2.flip(0)).flip(0), G.forward(x2))
        base = G.forward(x, ensemble=True).permute(0, 2, 3, 1)
        worst = 0.0
        for k in range(8):
            xk = D(x.permute(0, 2, 3, 1), k).permute(0, 3, 1, 2)
            got = G.forward(xk, ensemble=True).permute(0, 2, 3, 1)
            diff = float((got - D(base, k)).abs().max())
            print("equivariance k=%d max|diff| = %.3g" % (k, diff))
            worst = max(worst, diff)
            assert diff <= 1e-6, (k, diff)
    return worst


@pytest.mark.parametrize("backend", BACKENDS)
def test_ensemble_is_equivariant_f32(pkg, backend):
    dev = select(backend)
    _assert_equivariance(_tiny(pkg, dev), dev)


@pytest.mark.gpu
def test_ensemble_is_equivariant_f16_gpu(pkg):
    dev = select("hip")
    _assert_equivariance(_shipped(pkg, dev, "f16"), dev)


# ------------------------------------------------------------------------------------------------ 5. pipeline
def _mixed_frames(seed):
    rng = np.random.default_rng(seed)
    shapes = [(8, 12), (6, 5), (8, 12)]
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in shapes]


def _eager(G, dev, f):
    with torch.no_grad():
        return G.forward_u8(torch.from_numpy(f).unsqueeze(0).to(dev), ensemble=True)[0].cpu().numpy()


@pytest.mark.parametrize("backend", BACKENDS)
def test_pipeline_returns_the_ensemble_bytes(pkg, backend):
    dev = select(backend)
    G = _tiny(pkg, dev)
    frames = _mixed_frames(35)
    pipe = pkg.InferencePipeline(G, dev, batch=4, use_graph=False, ensemble=True)       # (fewer frames than a batch: the eager route)
    outs = pipe.run_mixed(frames)
    for f, y in zip(frames, outs):
        assert np.array_equal(y, _eager(G, dev, f)), f.shape
    same = [f for f in frames if f.shape[:2] == (8, 12)]
    for f, y in zip(same, pipe.run(same)):
        assert np.array_equal(y, _eager(G, dev, f))
    with pytest.raises(ValueError, match="RGB frames only"):
        pipe.run_yuv420([], 8, 12)


def test_pipeline_batch_accounts_for_the_members(pkg):
    from yuv_contract import ns
    G = pkg.Generator(ns(n_filters=64, n_layers=8), compute_dtype="f32")
    assert G.max_batch(360, 640) == 9 and G.max_batch(720, 1280) == 2
    plain, plus = pkg.InferencePipeline(G, "cpu", batch=8), pkg.InferencePipeline(G, "cpu", batch=8, ensemble=True)
    assert plain.ensemble is False and plus.ensemble is True
    assert plain._batch_for(360, 640) == 8 and plus._batch_for(360, 640) == 2        # 4 x 2 members stay below the kernels' 9
    assert plain._batch_for(720, 1280) == 2 and plus._batch_for(720, 1280) == 2      # below 4: forward_u8 chunks the members
    assert plus._batch_for(45, 80) == 8


@pytest.mark.gpu
def test_pipeline_ensemble_under_graph_gpu(pkg):
    dev = select("hip")
    G = _shipped(pkg, dev, "f16")
    rng = np.random.default_rng(36)
    frames = [rng.integers(0, 256, size=(8, 12, 3), dtype=np.uint8) for _ in range(5)]
    pipe = pkg.InferencePipeline(G, dev, batch=2, depth=1, ensemble=True)
    outs = list(pipe.run(frames))                     # two replays of one graph with different frames, then an eager tail
    (key, plan), = pipe._plans.items()
    assert key == (8, 12, "ensemble") and plan[0].graph is not None
    assert len(outs) == 5
    for f, y in zip(frames, outs):
        assert np.array_equal(y, _eager(G, dev, f))
    plain = pkg.InferencePipeline(G, dev, batch=2, depth=1)
    list(plain.run(frames[:2]))
    assert list(plain._plans) == [(8, 12)]            # the plain plan keeps its key


# ------------------------------------------------------------------------------------------------ 9. ABI
@pytest.mark.parametrize("backend", BACKENDS)
def test_entry_points_refuse_bad_arguments(backend):
    dev = select(backend)
    lib = L.lib()
    assert lib.fsr_version() == 16 == L.ABI_VERSION
    st = ops._stream()
    src = torch.zeros((2, 4, 5, 3), dtype=torch.uint8, device=dev)
    out = torch.full((8, 4, 5, 3), 7.0, device=dev)
    acc = torch.full((2, 4, 5, 3), 7.0, device=dev)
    s, o, a = src.data_ptr(), out.data_ptr(), acc.data_ptr()

    def members(src=s, u8=1, n=2, h=4, w=5, k0=0, k1=3, out=o):
        return lib.fsr_dihedral_members(src, u8, n, h, w, k0, k1, out, st)

    def accumulate(y=o, n=2, h=4, w=5, k0=0, k1=3, acc=a, out=None, kind=L.OUT_F32):
        return lib.fsr_dihedral_accumulate(y, n, h, w, k0, k1, acc, out, kind, st)

    for bad in (dict(src=None), dict(out=None), dict(n=0), dict(h=0), dict(w=-1), dict(k0=-1), dict(k1=8), dict(k0=4, k1=8),
                dict(k0=2, k1=1), dict(k0=3, k1=4), dict(n=65536)):
        assert members(**bad) < 0, bad
        assert lib.fsr_last_error(), bad
    for bad in (dict(y=None), dict(acc=None), dict(n=0), dict(h=-3), dict(w=0), dict(k0=-1), dict(k1=8), dict(k0=2, k1=5),
                dict(k0=4, k1=7, out=None), dict(k0=4, k1=7, out=a, kind=L.OUT_I420), dict(k0=4, k1=7, acc=None, out=a)):
        assert accumulate(**bad) < 0, bad
        assert lib.fsr_last_error(), bad
    # fsr_crop_resize_aug: its codes are device data (the wrapper checks them); pointers and sizes are checked like fsr_crop_resize's
    img = torch.zeros((3, 8, 8), dtype=torch.uint8, device=dev)
    ptrs = torch.tensor([img.data_ptr()], dtype=torch.int64, device=dev)
    ints = torch.zeros(8, dtype=torch.int32, device=dev)
    w = torch.zeros(64, device=dev)
    hr, lr, tmp = (torch.full((3 * 8 * 8,), 7.0, device=dev) for _ in range(3))
    good = [ptrs.data_ptr()] + [ints.data_ptr()] * 5 + [1, 8, 4, w.data_ptr(), ints.data_ptr(), ints.data_ptr(), 3,
                                                       hr.data_ptr(), lr.data_ptr(), tmp.data_ptr(), st]
    for i in (0, 5, 9, 13, 15):
        args = list(good)
        args[i] = None
        assert lib.fsr_crop_resize_aug(*args) < 0 and b"null" in lib.fsr_last_error(), i
    for i, v in ((6, 0), (7, 0), (7, -8), (8, 0), (8, 3)):
        args = list(good)
        args[i] = v
        assert lib.fsr_crop_resize_aug(*args) < 0 and b"bad sizes" in lib.fsr_last_error(), (i, v)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    for t in (out, acc, hr, lr, tmp):
        assert bool((t == 7.0).all())                                       # nothing was launched
    # the wrappers refuse the same before the library is called
    with pytest.raises(ValueError, match="0..7"):
        ops.dihedral_members(src, 0, 8)
    with pytest.raises(ValueError, match="one orientation group"):
        ops.dihedral_members(src, 3, 4)
    with pytest.raises(ValueError, match="members 0..3"):
        ops.dihedral_accumulate(out[:4], 0, 3, acc)
    assert members() == 0 and accumulate() == 0
