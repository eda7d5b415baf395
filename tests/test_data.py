"""Host side of the device-resident datasets (no GPU): the draw of nbdt_augment_batch as nbdt.data.draw_params restates
it -- deterministic, a function of the dataset index and not of its position, in range, uniform over its cells, different
from epoch to epoch --, the argument checks of the C entry, which run before any HIP call, and main.py's --augment flag."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import nbdt_path
from nbdt import _C
from nbdt import data as D

spec = importlib.util.spec_from_file_location("nbdt_main", os.path.join(nbdt_path.PKG_DIR, "main.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

CASES = [(pad, n, seed, epoch) for pad, n in ((4, 50_000), (8, 100_000)) for seed in (0, 1, 2) for epoch in (0, 1, 199)]


def test_dataset_stats_are_the_reference_transforms():
    assert D.DATASET_STATS["CIFAR10"] == {"mean": M.CIFAR_MEAN, "std": M.CIFAR_STD, "pad": 4}
    assert D.DATASET_STATS["CIFAR100"] == D.DATASET_STATS["CIFAR10"]
    assert D.DATASET_STATS["TinyImagenet200"] == {"mean": (0.4802, 0.4481, 0.3975), "std": (0.2302, 0.2265, 0.2262),
                                                  "pad": 8}
    assert "Imagenet1000" not in D.DATASET_STATS


def test_draw_is_deterministic_and_a_function_of_the_index_only():
    rng = np.random.default_rng(0)
    idx = rng.integers(0, 50_000, size=777)
    a = D.draw_params(3, 5, idx, 4)
    b = D.draw_params(3, 5, idx.copy(), 4)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    # position, batch size and container do not matter: a permuted / split / repeated batch draws the same per index
    p = rng.permutation(idx.size)
    for u, v in zip(a, D.draw_params(3, 5, idx[p], 4)):
        assert np.array_equal(u[p], v)
    for u, v in zip(a, D.draw_params(3, 5, torch.from_numpy(idx[:100]), 4)):
        assert np.array_equal(u[:100], v)
    for u, v in zip(D.draw_params(3, 5, [7, 7, 7, 11], 4), D.draw_params(3, 5, [11, 7], 4)):
        assert u[0] == u[1] == u[2] == v[1] and u[3] == v[0]
    # ... and the index does
    dy, dx, fl = D.draw_params(3, 5, np.arange(1000), 4)
    assert len(set(zip(dy.tolist(), dx.tolist(), fl.tolist()))) > 100
    # the seed and the epoch are part of the key
    assert any(not np.array_equal(u, v) for u, v in zip(a, D.draw_params(4, 5, idx, 4)))
    assert any(not np.array_equal(u, v) for u, v in zip(a, D.draw_params(3, 6, idx, 4)))


@pytest.mark.parametrize("pad", [0, 1, 4, 8, D.MAX_PAD])
def test_draw_stays_in_range_and_reaches_every_value(pad):
    dy, dx, fl = D.draw_params(0, 0, np.arange(200_000), pad)
    for d in (dy, dx):
        assert d.min() == 0 and d.max() == 2 * pad and np.unique(d).size == 2 * pad + 1
    assert set(np.unique(fl).tolist()) == {0, 1}
    with pytest.raises(ValueError):
        D.draw_params(0, 0, [0], D.MAX_PAD + 1)
    with pytest.raises(ValueError):
        D.draw_params(0, 0, [0], -1)


@pytest.mark.parametrize("pad,n,seed,epoch", CASES)
def test_draw_is_uniform_over_its_cells(pad, n, seed, epoch):
    """Chi-square of the (2*pad+1)^2 * 2 cells (dy, dx, flip) over the dataset indices 0..n-1: p > 1e-3 in each of the
    18 cases (the smallest is 0.032)."""
    from scipy import stats
    span = 2 * pad + 1
    dy, dx, fl = D.draw_params(seed, epoch, np.arange(n), pad)
    cell = (dy * span + dx) * 2 + fl
    counts = np.bincount(cell, minlength=span * span * 2)
    assert counts.size == span * span * 2 and counts.min() > 0          # every value of the range occurs
    p = stats.chisquare(counts).pvalue
    print(f"pad {pad} n {n} seed {seed} epoch {epoch}: p = {p:.4f}")
    assert p > 1e-3


@pytest.mark.parametrize("pad,n", [(4, 50_000), (8, 100_000)])
def test_consecutive_epochs_draw_independently(pad, n):
    """Two epochs give a sample the same (dy, dx, flip) with probability 1 / cells when the draws are independent.  The
    count of coincidences over n samples is binomial: it must lie within 5 standard deviations of n / cells (a fixed
    generator either does or does not; 5 sigma leaves a false alarm to 1 in 1.7 million such generators)."""
    cells = (2 * pad + 1) ** 2 * 2
    for seed in (0, 1, 2):
        for e0, e1 in ((0, 1), (1, 2), (198, 199)):
            a = D.draw_params(seed, e0, np.arange(n), pad)
            b = D.draw_params(seed, e1, np.arange(n), pad)
            same = int(np.sum((a[0] == b[0]) & (a[1] == b[1]) & (a[2] == b[2])))
            q = 1.0 / cells
            sigma = (n * q * (1 - q)) ** 0.5
            print(f"pad {pad} seed {seed} epochs {e0},{e1}: {same} coincide, {n * q:.1f} +- {sigma:.1f} expected")
            assert abs(same - n * q) < 5 * sigma


def _call(**over):
    """nbdt_augment_batch with plausible arguments, `over` replacing some.  The pointers are never dereferenced: every
    case here is refused before the first HIP call."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    a = dict(src=p, dtype=_C.NBDT_U8, labels_src=p, index=p, B=4, N=16, H=32, W=32, pad=4, flip=1, mean=f3, std=f3, fill=f3,
             seed=0, epoch=0, params_in=None, out=p, labels_out=p, params_out=None, stream=None)
    a.update(over)
    lib = _C.lib()
    rc = lib.nbdt_augment_batch(a["src"], a["dtype"], a["labels_src"], a["index"], a["B"], a["N"], a["H"], a["W"], a["pad"],
                                a["flip"], a["mean"], a["std"], a["fill"], a["seed"], a["epoch"], a["params_in"], a["out"],
                                a["labels_out"], a["params_out"], a["stream"])
    return rc, lib.nbdt_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(src=None), "null"), (dict(labels_src=None), "null"), (dict(index=None), "null"), (dict(out=None), "null"),
    (dict(labels_out=None), "null"),
    (dict(mean=None), "mean"), (dict(std=None), "mean"), (dict(dtype=_C.NBDT_F32, fill=None), "fill"),
    (dict(B=0), "empty batch"), (dict(B=-3), "empty batch"), (dict(N=0), "empty dataset"),
    (dict(pad=_C.NBDT_AUGMENT_MAX_PAD + 1), "pad"), (dict(pad=-1), "pad"),
    (dict(dtype=_C.NBDT_BF16), "uint8"), (dict(dtype=7), "uint8"),
    (dict(flip=2), "flip"), (dict(H=0), "image sides"), (dict(W=5000), "image sides"),
    (dict(std=(ctypes.c_float * 3)(1.0, 0.0, 1.0)), "non-zero"),
])
def test_entry_rejects_bad_arguments_before_any_hip_call(over, word):
    assert _C.lib().nbdt_version() >= 110
    rc, msg = _call(**over)
    assert rc == -1 and word in msg, (rc, msg)


def test_pad_bound_admits_the_reference_paddings():
    assert _C.NBDT_AUGMENT_MAX_PAD >= 8 and D.MAX_PAD == _C.NBDT_AUGMENT_MAX_PAD
    text = open(os.path.join(nbdt_path.ROOT, "include", "nbdt_hip.h")).read()
    assert f"#define NBDT_AUGMENT_MAX_PAD {_C.NBDT_AUGMENT_MAX_PAD}\n" in text
    assert f"#define NBDT_U8 {_C.NBDT_U8} " in text


def test_device_dataset_refuses_the_cpu():
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    y = torch.zeros(4, dtype=torch.long)
    with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
        D.DeviceDataset(x, y, (0.5,) * 3, (0.5,) * 3, 2, device="cpu")


def test_main_accepts_the_augment_flag():
    p = M.build_parser()
    assert p.parse_args([]).augment == "none"
    assert p.parse_args(["--augment", "reference"]).augment == "reference"
    assert p.parse_args(["--augment", "none"]).augment == "none"
    with pytest.raises(SystemExit):
        p.parse_args(["--augment", "torchvision"])


def test_main_refuses_to_augment_imagenet1000():
    with pytest.raises(SystemExit, match="RandomResizedCrop"):
        M.main(["--dataset", "Imagenet1000", "--arch", "ResNet18", "--augment", "reference", "--synthetic", "8"])


def test_load_data_keeps_uint8_only_when_asked(tmp_path):
    """--augment none normalises a uint8 file on the host exactly as before; --augment reference hands the bytes on."""
    g = torch.Generator().manual_seed(0)
    blob = {"train_x": torch.randint(0, 256, (6, 3, 8, 8), dtype=torch.uint8, generator=g), "train_y": torch.arange(6),
            "test_x": torch.randint(0, 256, (2, 3, 8, 8), dtype=torch.uint8, generator=g), "test_y": torch.arange(2)}
    torch.save(blob, tmp_path / "d.pt")
    args = M.build_parser().parse_args(["--data-file", str(tmp_path / "d.pt")])
    tx, ty, vx, vy = M.load_data(args, 10, "cpu")
    assert tx.dtype == torch.float32
    want = (blob["train_x"].float().div(255.0) - torch.tensor(M.CIFAR_MEAN).view(1, 3, 1, 1)) / torch.tensor(M.CIFAR_STD).view(1, 3, 1, 1)
    assert torch.equal(tx, want)
    rx, ry, _, _ = M.load_data(args, 10, "cpu", raw=True)
    assert rx.dtype == torch.uint8 and torch.equal(rx, blob["train_x"]) and torch.equal(ry, ty)
