"""Self-ensemble through the evaluation tool and the command lines: Evaluator.run(ensemble=True) scores the bytes of
forward_u8(..., ensemble=True), evaluate.py adds a `<path>+` column, inference.py takes --self_ensemble."""
import importlib
import math

import numpy as np
import pytest
import torch

from backend import BACKENDS, ops, select
from yuv_contract import _tiny

evaluate = importlib.import_module("fast-srgan_amd.evaluate")
inference = importlib.import_module("fast-srgan_amd.inference")

SCALE = 4


def _write_hr(tmp_path):
    """Two tiny synthetic HR images of different shapes (smooth gradients plus noise), as the data set's uint8 (3,H,W) arrays."""
    rng = np.random.default_rng(51)
    paths = []
    for i, (h, w) in enumerate(((32, 40), (36, 32))):
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([4 * yy + 2 * xx, 200 - 3 * xx, 30 + 5 * yy], 0)
        img = np.clip(base + rng.integers(-20, 21, size=base.shape), 0, 255).astype(np.uint8)
        paths.append(str(tmp_path / ("hr%d.npy" % i)))
        np.save(paths[-1], img)
    return paths


@pytest.mark.parametrize("backend", BACKENDS)
def test_evaluator_scores_the_ensemble_bytes(pkg, backend, tmp_path):
    dev = select(backend)
    G = _tiny(pkg, dev)
    ev = evaluate.Evaluator(_write_hr(tmp_path), SCALE, device=dev, batch=2)
    res = ev.run(G, ensemble=True)
    plain = ev.run(G)
    assert len(ev.buckets) == 2
    for b in ev.buckets:
        with torch.no_grad():
            sr = G.forward_u8(b.lr, ensemble=True)
        q = ops.quality_u8(sr, b.hr, ev.shave, "y").cpu().double().numpy()
        eh, ew = b.H - 2 * ev.shave, b.W - 2 * ev.shave
        for j, i in enumerate(b.index):
            row = res["images"][i]
            assert row["psnr"] == 10.0 * math.log10(255.0 ** 2 * eh * ew / float(q[j, 1]))
            assert row["ssim"] == float(q[j, 0]) / ((eh - 10) * (ew - 10))
    assert res["psnr"] == float(np.mean([r["psnr"] for r in res["images"]]))
    assert [r["psnr"] for r in res["images"]] != [r["psnr"] for r in plain["images"]]      # another image than the plain run scores

    class _Plain:
        """A model whose forward_u8 has no `ensemble` argument (BicubicModel): a plain run never passes it."""

        def forward_u8(self, frames, bands=None):
            return G.forward_u8(frames, bands=bands)

    with torch.no_grad():
        assert ev.run(_Plain())["images"] == plain["images"]
    with pytest.raises(TypeError):
        ev.run(_Plain(), ensemble=True)


def test_evaluate_parser_and_table_have_the_plus_column():
    args = evaluate.parser.parse_args(["--hr_dir", "x", "--model", "a.pt", "b.pt", "--self_ensemble"])
    assert args.self_ensemble is True
    assert evaluate.parser.parse_args(["--hr_dir", "x"]).self_ensemble is False
    rows = [{"name": "img0", "psnr": 30.0, "ssim": 0.9}]
    columns = [dict(images=rows, psnr=30.0, ssim=0.9, name="a.pt"), dict(images=rows, psnr=30.5, ssim=0.91, name="a.pt+")]
    table = evaluate.format_table(["img0"], columns).splitlines()
    assert table[0].split() == ["a.pt", "a.pt+"]
    assert "30.5000 dB" in table[-1]


def test_evaluate_main_adds_a_plus_column_per_model(monkeypatch, tmp_path):
    """main() with the device parts replaced: every --model gets `<path>` and `<path>+`, the second from run(ensemble=True), and the
    setting is recorded in the JSON file."""
    import json
    calls = []

    class _Ev:
        names, shave, channel = ["img0"], 4, "y"

        def __init__(self, *a, **k):
            pass

        def run(self, model, bands="auto", band_rows=128, save_dir=None, ensemble=False):
            calls.append((model, ensemble))
            return {"images": [{"name": "img0", "psnr": 31.0 if ensemble else 30.0, "ssim": 0.9}], "psnr": 31.0 if ensemble else 30.0, "ssim": 0.9}

    monkeypatch.setattr(evaluate, "Evaluator", _Ev)
    monkeypatch.setattr(evaluate, "list_images", lambda d: ["img0.png"])
    monkeypatch.setattr(evaluate.torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(inference, "load_generator", lambda config, path, device, cd: path)
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path / "out.json")
    cols = evaluate.main(["--hr_dir", "x", "--model", "a.pt", "b.pt", "--self_ensemble", "--json", out])
    assert [c["name"] for c in cols] == ["a.pt", "a.pt+", "b.pt", "b.pt+"]
    assert calls == [("a.pt", False), ("a.pt", True), ("b.pt", False), ("b.pt", True)]
    assert json.load(open(out))["settings"]["self_ensemble"] is True
    calls.clear()
    cols = evaluate.main(["--hr_dir", "x", "--model", "a.pt", "--json", out])
    assert [c["name"] for c in cols] == ["a.pt"] and calls == [("a.pt", False)]
    assert json.load(open(out))["settings"]["self_ensemble"] is False


def test_inference_parser_takes_self_ensemble():
    base = ["--image_dir", "i", "--output_dir", "o"]
    assert inference.parser.parse_args(base + ["--self_ensemble"]).self_ensemble is True
    assert inference.parser.parse_args(base).self_ensemble is False
