"""main.py with --label-smoothing, --mixup-alpha and --cutmix-alpha end to end on the MI355X: the run trains (a finite
loss) and repeats to the bit."""
import glob
import importlib.util
import math
import os
import re
import shutil

import pytest
import torch

import nbdt_path

pytestmark = pytest.mark.gpu

spec = importlib.util.spec_from_file_location("nbdt_main", os.path.join(nbdt_path.PKG_DIR, "main.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)


@pytest.fixture
def default_mode():
    from nbdt import ops
    yield
    ops.set_deterministic(False)         # --deterministic is a process-wide switch


def test_smoothed_mixed_training_runs_and_repeats(tmp_path, monkeypatch, capsys, default_mode):
    monkeypatch.chdir(tmp_path)
    argv = ("--arch ResNet18 --dataset CIFAR10 --synthetic 256 --batch-size 64 --epochs 1 --loss SoftTreeSupLoss "
            "--label-smoothing 0.1 --mixup-alpha 0.2 --cutmix-alpha 1.0 --deterministic").split()
    runs = []
    for tag in "ab":
        M.main(argv)
        losses = [float(v) for v in re.findall(r"^Loss: ([-+.\w]+)", capsys.readouterr().out, flags=re.M)]
        assert len(losses) == 2 and all(math.isfinite(v) for v in losses), losses      # the training and the test loss
        (ck,) = glob.glob("checkpoint/*.pth")
        runs.append((losses, torch.load(ck, map_location="cpu")))
        shutil.move("checkpoint", "checkpoint_" + tag)
    (la, a), (lb, b) = runs
    assert la == lb
    assert a["acc"] == b["acc"] and set(a["net"]) == set(b["net"])
    for k in a["net"]:
        assert torch.isfinite(a["net"][k].float()).all(), k
        assert torch.equal(a["net"][k], b["net"][k]), k
