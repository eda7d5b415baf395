"""main.py --augment end to end on the MI355X: a uint8 --data-file trained without and with the reference's crop + flip
(device-resident dataset, one launch per step), both well above chance; the augmented run repeatable to the bit; and the
refusal for Imagenet1000."""
import importlib.util
import math
import os
import shutil

import pytest
import torch

import nbdt_path

pytestmark = pytest.mark.gpu

spec = importlib.util.spec_from_file_location("nbdt_main", os.path.join(nbdt_path.PKG_DIR, "main.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

# ten well separated class colours; --synthetic's per-pixel prototypes would not do here: a 4-pixel shift decorrelates them
COLOURS = [(200, 60, 60), (60, 200, 60), (60, 60, 200), (200, 200, 60), (200, 60, 200), (60, 200, 200), (200, 200, 200),
           (60, 60, 60), (200, 130, 60), (60, 130, 200)]


def write_data_file(path, n_train=1024, n_test=256, size=32, seed=0):
    """A class signal that survives shifts and flips: a colour per class plus a low-frequency pattern (1-3 cosine periods
    across the image, symmetric about its centre line), under per-pixel noise of sigma 30."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(size, dtype=torch.float32)
    proto = torch.empty(10, 3, size, size)
    for c, rgb in enumerate(COLOURS):
        wave = 25.0 * torch.cos(2 * math.pi * (c % 3 + 1) * (t + 0.5) / size)[None, :] \
            + 15.0 * torch.cos(2 * math.pi * (c % 2 + 1) * (t + 0.5) / size)[:, None]
        proto[c] = torch.tensor(rgb, dtype=torch.float32).view(3, 1, 1) + wave[None]

    def make(n):
        y = torch.randint(0, 10, (n,), generator=g)
        x = proto[y] + 30.0 * torch.randn(n, 3, size, size, generator=g)
        return x.round().clamp(0, 255).to(torch.uint8), y
    tx, ty = make(n_train)
    vx, vy = make(n_test)
    torch.save({"train_x": tx, "train_y": ty, "test_x": vx, "test_y": vy}, path)


@pytest.fixture
def default_mode():
    from nbdt import ops
    yield
    ops.set_deterministic(False)         # --deterministic is a process-wide switch


def test_augmented_training_runs_learns_and_repeats(tmp_path, monkeypatch, default_mode):
    monkeypatch.chdir(tmp_path)
    write_data_file("data.pt")
    common = ("--arch ResNet18 --dataset CIFAR10 --batch-size 64 --data-file data.pt --lr 0.05 --epochs 7 "
              "--loss SoftTreeSupLoss --deterministic").split()
    ck = "checkpoint/ckpt-CIFAR10-ResNet18-lr0.05-induced-ResNet18-SoftTreeSupLoss.pth"
    acc_none, _ = M.main(common + ["--augment", "none"])
    assert os.path.exists(ck)
    shutil.move("checkpoint", "checkpoint_none")
    acc_a, _ = M.main(common + ["--augment", "reference"])
    shutil.move("checkpoint", "checkpoint_a")
    acc_b, _ = M.main(common + ["--augment", "reference"])
    print(f"accuracy after 7 epochs: --augment none {acc_none:.2f} %, --augment reference {acc_a:.2f} % / {acc_b:.2f} %")
    # repeatable: the same accuracy and a bit-identical checkpoint
    assert acc_a == acc_b
    a, b = torch.load("checkpoint_a/" + os.path.basename(ck), map_location="cpu"), torch.load(ck, map_location="cpu")
    assert a["acc"] == b["acc"] and a["epoch"] == b["epoch"] and set(a["net"]) == set(b["net"])
    for k in a["net"]:
        assert torch.equal(a["net"][k], b["net"][k]), k
    # the augmentation changed what was trained on
    n = torch.load("checkpoint_none/" + os.path.basename(ck), map_location="cpu")
    assert any(not torch.equal(n["net"][k], a["net"][k]) for k in a["net"])
    # 10 classes: both well above chance (the bar of tests/test_main_gpu.py)
    assert acc_none > 25.0
    assert acc_a > 25.0


def test_augmented_evaluation_equals_the_host_path(tmp_path, monkeypatch):
    """--eval of one checkpoint: the device-resident test split (gather + normalise in the kernel) scores exactly what the
    host-normalised split scores -- the evaluation transform is the same bits."""
    monkeypatch.chdir(tmp_path)
    write_data_file("data.pt", n_test=250)
    common = ("--arch ResNet18 --dataset CIFAR10 --batch-size 64 --data-file data.pt --lr 0.05 --epochs 4").split()
    M.main(common)
    acc_host, _ = M.main(common + ["--resume", "--eval"])
    acc_dev, _ = M.main(common + ["--resume", "--eval", "--augment", "reference"])
    assert acc_host == acc_dev and acc_host > 25.0        # (a model that learnt something: not a constant prediction)


def test_synthetic_float_data_trains_with_augmentation(tmp_path, monkeypatch):
    """--synthetic is float: taken as normalised, cropped and flipped with the (0 - mean)/std fill.  Runs and stays finite."""
    monkeypatch.chdir(tmp_path)
    acc, _ = M.main("--arch ResNet18 --dataset CIFAR10 --batch-size 64 --synthetic 256 --lr 0.05 --epochs 2 "
                    "--augment reference".split())
    assert 0.0 <= acc <= 100.0 and math.isfinite(acc)


def test_imagenet1000_is_refused():
    with pytest.raises(SystemExit, match="RandomResizedCrop"):
        M.main("--dataset Imagenet1000 --arch ResNet18 --augment reference --synthetic 64".split())
