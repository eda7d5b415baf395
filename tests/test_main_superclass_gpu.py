"""main.py's zero-shot superclass evaluation and training on a label subset, end to end on the MI355X: a CIFAR10
classifier evaluated on a synthetic TinyImagenet200-labelled split against "animal" / "vehicle", and two epochs of
training from which two labels are excluded."""
import importlib.util
import os
import re
import warnings

import pytest
import torch

import nbdt_path

pytestmark = pytest.mark.gpu

spec = importlib.util.spec_from_file_location("nbdt_main_superclass", os.path.join(nbdt_path.PKG_DIR, "main.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

from nbdt import superclass as S  # noqa: E402
from nbdt.data import label_subset  # noqa: E402
from nbdt.tree import get_wnids  # noqa: E402
from nbdt.utils import dataset_to_default_path_wnids  # noqa: E402

SUPERS = ["n00015388", "n04524313"]
EVAL = ("--arch ResNet18 --dataset CIFAR10 --dataset-test TinyImagenet200 --hierarchy induced-ResNet18 --synthetic 256 "
        "--eval --disable-test-eval --superclass-wnids").split() + SUPERS


@pytest.mark.parametrize("name, printed", [("SuperclassNBDT", "Superclass-NBDT"), ("Superclass", "Superclass")])
def test_zero_shot_superclass_evaluation(tmp_path, monkeypatch, capsys, name, printed):
    monkeypatch.chdir(tmp_path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)          # the lossy graph fallback says so; test_superclass.py checks it
        acc, analyzer_acc = M.main(EVAL + ["--analysis", name])
        mapping, _ = S.Superclass.build_mapping(get_wnids(dataset_to_default_path_wnids("TinyImagenet200")), SUPERS)
    out = capsys.readouterr().out
    args = M.parse_args(EVAL + ["--analysis", name])
    labels, _ = M.synthetic_test_labels(args.seed, 200, max(256 // 4, args.batch_size))
    expected = int((mapping[labels] >= 0).sum())
    line = re.search(r"\[%s\] Accuracy: ([0-9.]+)%% \((\d+) of (\d+) " % re.escape(printed), out)
    assert line, out
    correct, total = int(line.group(2)), int(line.group(3))
    assert 0 < expected < labels.numel() and total == expected and 0 <= correct <= total
    assert abs(analyzer_acc - 100.0 * correct / total) < 1e-9 and float(line.group(1)) == round(analyzer_acc, 2)
    assert "Testing with dataset TinyImagenet200 and 200 classes" in out and "--disable-test-eval" in out
    assert acc == 0.0 and not os.path.exists("checkpoint")     # nothing evaluated the backbone, nothing was saved


@pytest.mark.parametrize("augment", ["none", "reference"])
def test_excluded_labels_never_reach_the_loss(tmp_path, monkeypatch, augment):
    monkeypatch.chdir(tmp_path)
    argv = ("--arch ResNet18 --dataset CIFAR10 --batch-size 64 --synthetic 256 --lr 0.05 --epochs 2 --exclude-labels 0 1 "
            "--augment " + augment).split()
    args = M.parse_args(argv)
    train_y = M.load_data(args, 10, "cpu")[1]
    kept = label_subset(train_y, 10, exclude_labels=[0, 1], seed=args.seed)
    allowed = set(kept.tolist())
    assert 150 < len(allowed) < 256 and all(int(train_y[i]) > 1 for i in allowed)
    plans, seen = [], []
    real_plan, real_step = M.ndist.epoch_indices, M.train_step

    def plan_spy(*a, **k):
        plans.append(real_plan(*a, **k))
        return plans[-1]

    def step_spy(engine, fast, xb, yb, *a, **k):
        seen.append(yb)                                        # device tensors: looked at after the run
        return real_step(engine, fast, xb, yb, *a, **k)

    monkeypatch.setattr(M.ndist, "epoch_indices", plan_spy)
    monkeypatch.setattr(M, "train_step", step_spy)
    M.main(argv)
    assert len(plans) == 2 and all(p.shape == (len(allowed) // 64, 64) for p in plans)
    for p in plans:
        flat = p.reshape(-1).tolist()
        assert set(flat) <= allowed and len(set(flat)) == len(flat)
    assert not torch.equal(plans[0], plans[1])
    assert len(seen) == 2 * (len(allowed) // 64)
    labels = torch.cat([y.cpu() for y in seen])
    assert int(labels.min()) >= 2 and torch.equal(labels, train_y[torch.cat([p.reshape(-1) for p in plans])])


def test_training_with_the_backbone_evaluation_disabled_checkpoints_on_the_analyzer(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    argv = ("--arch ResNet18 --dataset CIFAR10 --dataset-test TinyImagenet200 --hierarchy induced-ResNet18 --batch-size 64 "
            "--synthetic 256 --lr 0.05 --epochs 2 --disable-test-eval --analysis Superclass --superclass-wnids").split() + SUPERS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        acc, analyzer_acc = M.main(argv)
    out = capsys.readouterr().out
    files = os.listdir("checkpoint")
    assert acc == 0.0 and len(files) == 1 and "Saving to" in out and "(Superclass)" in out
    saved = torch.load(os.path.join("checkpoint", files[0]), map_location="cpu")
    scores = [float(v) for v in re.findall(r"\| Superclass: ([0-9.]+)%", out)]
    assert len(scores) == 2 and 0.0 < saved["acc"] <= 100.0 and abs(saved["acc"] - max(scores)) < 1e-3
    assert abs(scores[-1] - analyzer_acc) < 1e-3
