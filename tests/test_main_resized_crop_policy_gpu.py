"""main.py --augment resized-crop-policy end to end on the MI355X: ResNet18 trains one short epoch on a uint8 file with
RandAugment and random erasing on the 32 x 32 crop, through nbdt_resized_crop_policy_batch, and evaluates through the plain
resized-crop launch."""
import importlib.util
import math
import os
import re

import pytest
import torch

import nbdt_path

pytestmark = pytest.mark.gpu

spec = importlib.util.spec_from_file_location("nbdt_main", os.path.join(nbdt_path.PKG_DIR, "main.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)


def test_main_trains_with_a_policy_on_the_resized_crop(tmp_path, monkeypatch, capsys):
    from nbdt import ops
    monkeypatch.chdir(tmp_path)
    g = torch.Generator().manual_seed(0)
    blob = {"train_x": torch.randint(0, 256, (64, 3, 40, 40), dtype=torch.uint8, generator=g),
            "train_y": torch.randint(0, 1000, (64,), generator=g),
            "test_x": torch.randint(0, 256, (64, 3, 40, 40), dtype=torch.uint8, generator=g),
            "test_y": torch.randint(0, 1000, (64,), generator=g)}
    torch.save(blob, "data.pt")
    calls = {"policy": 0, "plain": 0}
    policy_batch, plain_batch = ops.resized_crop_policy_batch, ops.resized_crop_batch

    def count(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped
    monkeypatch.setattr(ops, "resized_crop_policy_batch", count("policy", policy_batch))
    monkeypatch.setattr(ops, "resized_crop_batch", count("plain", plain_batch))
    acc, _ = M.main(("--arch ResNet18 --dataset Imagenet1000 --batch-size 32 --data-file data.pt --lr 0.05 --epochs 1 "
                     "--augment resized-crop-policy --crop-size 32 --auto-augment ra --random-erase 0.1").split())
    assert 0.0 <= acc <= 100.0 and math.isfinite(acc)
    assert calls["policy"] == 2 and calls["plain"] >= 1             # two training steps; evaluation stays plain
    out = capsys.readouterr().out
    assert "ra: RandAugment, 2 operations at magnitude 9" in out and "nbdt_resized_crop_policy_batch" in out
    assert "--random-erase 0.1" in out and "32 x 32 crop" in out
    losses = [float(v) for v in re.findall(r"Loss: (\S+) \(2 steps", out)]   # the epoch's mean training loss
    assert len(losses) == 1 and math.isfinite(losses[0]), out
