"""main.py --augment resized-crop end to end on the MI355X: EfficientNet-B0 on Imagenet1000-shaped synthetic bytes trains
an epoch and evaluates with finite numbers, and under a fixed seed two runs hand the engine identical batches."""
import importlib.util
import math
import os

import pytest
import torch

import nbdt_path

pytestmark = pytest.mark.gpu

spec = importlib.util.spec_from_file_location("nbdt_main", os.path.join(nbdt_path.PKG_DIR, "main.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

ARGS = ("--dataset Imagenet1000 --arch efficientnet_b0 --loss SoftTreeSupLoss --hierarchy induced-efficientnet_b7b "
        "--augment resized-crop --synthetic 64 --image-size 64 --crop-size 64 --epochs 1 --batch-size 16 --lr 0.01").split()


def test_resized_crop_training_runs_and_repeats_its_batches(tmp_path, monkeypatch):
    """The batches are compared, not the trained weights: the EfficientNet step is not bit-reproducible outside
    deterministic mode."""
    monkeypatch.chdir(tmp_path)
    real_step = M.train_step
    runs = []

    def recording_step(engine, fast, xb, yb, lr, comm=None):
        runs[-1].append((xb.clone(), yb.clone()))
        return real_step(engine, fast, xb, yb, lr, comm=comm)

    monkeypatch.setattr(M, "train_step", recording_step)
    results = []
    for _ in range(2):
        runs.append([])
        results.append(M.main(ARGS))
    for acc, _ in results:
        assert 0.0 <= acc <= 100.0 and math.isfinite(acc)
    a, b = runs
    assert len(a) == len(b) == 4                      # 64 images in batches of 16
    for (xa, ya), (xb, yb) in zip(a, b):
        assert tuple(xa.shape) == (16, 3, 64, 64) and xa.dtype == torch.float32 and torch.isfinite(xa).all()
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
    assert not torch.equal(a[0][0], a[1][0])
    # another seed draws other crops (and other synthetic images)
    runs.append([])
    M.main(ARGS + ["--seed", "1"])
    assert not torch.equal(runs[2][0][0], a[0][0])


def test_float_data_files_are_refused(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    blob = {"train_x": torch.zeros(8, 3, 16, 16), "train_y": torch.zeros(8, dtype=torch.long),
            "test_x": torch.zeros(8, 3, 16, 16), "test_y": torch.zeros(8, dtype=torch.long)}
    torch.save(blob, "f.pt")
    with pytest.raises(SystemExit, match="uint8"):
        M.main("--dataset Imagenet1000 --arch efficientnet_b0 --augment resized-crop --data-file f.pt".split())
