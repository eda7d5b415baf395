"""nbdt_augment_batch / nbdt.data.DeviceDataset on the MI355X against the reference's transform restated in plain torch
on the CPU: torch.nn.functional.pad of the uint8 tensor, a slice, flip(-1), .float().div(255).sub(mean).div(std), fed the
(dy, dx, flip) the kernel reports.  Every comparison is torch.equal: nothing is rounded or reordered, so there is no
tolerance."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nbdt_path
from nbdt import data as D

pytestmark = pytest.mark.gpu

CIFAR = D.DATASET_STATS["CIFAR10"]
TINY = D.DATASET_STATS["TinyImagenet200"]


def restate(x_u8, y, index, params, mean, std, pad):
    """RandomCrop(size, padding=pad) -> RandomHorizontalFlip -> ToTensor -> Normalize with given draws, on the CPU."""
    mean = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
    H, W = x_u8.shape[2:]
    out = []
    for i, (dy, dx, fl) in zip(index.tolist(), params.tolist()):
        img = F.pad(x_u8[i], (pad, pad, pad, pad))              # byte 0, before conversion
        img = img[:, dy:dy + H, dx:dx + W]
        if fl:
            img = img.flip(-1)
        out.append(img.float().div(255).sub(mean).div(std))
    return torch.stack(out), y[index]


def make(n, H, W, classes=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, 3, H, W), dtype=torch.uint8, generator=g),
            torch.randint(0, classes, (n,), generator=g))


@pytest.mark.parametrize("size,stats", [(32, CIFAR), (64, TINY)])
def test_every_crop_offset_and_flip_equals_the_cpu_restatement(size, stats):
    pad = stats["pad"]
    span = 2 * pad + 1
    combos = [(dy, dx, fl) for dy in range(span) for dx in range(span) for fl in (0, 1)]
    assert len(combos) == {4: 162, 8: 578}[pad]
    x, y = make(53, size, size, seed=pad)
    ds = D.DeviceDataset(x, y, stats["mean"], stats["std"], pad)
    g = torch.Generator().manual_seed(1)
    index = torch.randint(0, 53, (len(combos),), generator=g)
    params = torch.tensor(combos, dtype=torch.int8)
    img, tgt, used = ds.batch(index, params=params, return_params=True)
    assert torch.equal(used.cpu(), params)
    want, want_y = restate(x, y, index, params, stats["mean"], stats["std"], pad)
    assert torch.equal(img.cpu(), want) and torch.equal(tgt.cpu(), want_y)
    # a padded pixel is (0 - mean) / std, not 0: the top-left pixel of the (0, 0, no flip) crop lies in the padding
    assert combos[0] == (0, 0, 0)
    pix = (torch.zeros(3) - torch.tensor(stats["mean"])) / torch.tensor(stats["std"])
    assert torch.equal(img[0, :, 0, 0].cpu(), pix) and bool((pix != 0).all())


@pytest.mark.parametrize("B", [1, 37, 512])
@pytest.mark.parametrize("n,H,W,pad", [(1009, 32, 32, 4), (211, 64, 64, 8), (157, 24, 40, 3), (61, 9, 7, 2)])
def test_generated_draws_equal_draw_params_and_the_restatement(B, n, H, W, pad):
    """params_in null: the kernel's own draws are draw_params(seed, epoch, index, pad) and the images follow them.
    Indices repeat; N is prime; two cases are not square, one of them with a width no 16-byte store fits."""
    x, y = make(n, H, W, seed=n)
    ds = D.DeviceDataset(x, y, CIFAR["mean"], CIFAR["std"], pad)
    g = torch.Generator().manual_seed(B)
    index = torch.randint(0, n, (B,), generator=g)
    if B > 2:
        index[1] = index[0]
        index[-1] = index[0]
    for seed, epoch in ((0, 0), (5, 199)):
        img, tgt, used = ds.batch(index, epoch=epoch, seed=seed, return_params=True)
        dy, dx, fl = D.draw_params(seed, epoch, index, pad)
        want_p = torch.from_numpy(np.stack([dy, dx, fl], axis=1)).to(torch.int8)
        assert torch.equal(used.cpu(), want_p)
        want, want_y = restate(x, y, index, want_p, CIFAR["mean"], CIFAR["std"], pad)
        assert torch.equal(img.cpu(), want) and torch.equal(tgt.cpu(), want_y)
    # a device index takes the same path
    img2, tgt2 = ds.batch(index.cuda(), epoch=199, seed=5)
    assert torch.equal(img2, img) and torch.equal(tgt2, tgt)


def test_a_batch_is_the_concatenation_of_its_halves():
    x, y = make(307, 32, 32)
    ds = D.DeviceDataset(x, y, CIFAR["mean"], CIFAR["std"], 4)
    g = torch.Generator().manual_seed(2)
    a, b = torch.randint(0, 307, (100,), generator=g), torch.randint(0, 307, (28,), generator=g)
    whole = ds.batch(torch.cat([a, b]), epoch=3, seed=9, return_params=True)
    pa, pb = ds.batch(a, epoch=3, seed=9, return_params=True), ds.batch(b, epoch=3, seed=9, return_params=True)
    for w, u, v in zip(whole, pa, pb):
        assert torch.equal(w, torch.cat([u, v]))
    other = ds.batch(torch.cat([a, b]), epoch=4, seed=9, return_params=True)
    assert not torch.equal(other[2], whole[2])                  # the epoch is part of the draw
    assert whole[0].data_ptr() != other[0].data_ptr()           # and every call hands out its own tensors


def test_flip_off_and_pad_zero():
    x, y = make(64, 32, 32)
    index = torch.arange(64)
    noflip = D.DeviceDataset(x, y, CIFAR["mean"], CIFAR["std"], 4, flip=False)
    _, _, used = noflip.batch(index, return_params=True)
    assert int(used[:, 2].sum()) == 0 and int(used[:, :2].max()) > 0
    nopad = D.DeviceDataset(x, y, CIFAR["mean"], CIFAR["std"], 0)
    img, _, used = nopad.batch(index, return_params=True)
    assert int(used[:, :2].abs().sum()) == 0 and 0 < int(used[:, 2].sum()) < 64
    want, _ = restate(x, y, index, used.cpu(), CIFAR["mean"], CIFAR["std"], 0)
    assert torch.equal(img.cpu(), want)


def test_evaluation_transform_equals_main_py_host_normalisation(tmp_path):
    spec = importlib.util.spec_from_file_location("nbdt_main", os.path.join(nbdt_path.PKG_DIR, "main.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    x, y = make(203, 32, 32)
    torch.save({"train_x": x, "train_y": y, "test_x": x[:10], "test_y": y[:10]}, tmp_path / "d.pt")
    args = M.build_parser().parse_args(["--data-file", str(tmp_path / "d.pt")])
    host_x, host_y, _, _ = M.load_data(args, 10, "cpu")          # the uint8 branch: .float().div_(255), (x - mean) / std
    ds = D.DeviceDataset(x, y, CIFAR["mean"], CIFAR["std"], CIFAR["pad"])
    for lo in (0, 100, 200):
        index = torch.arange(lo, min(lo + 100, 203))
        img, tgt, used = ds.batch(index.cuda(), train=False, return_params=True)
        assert int(used.abs().sum()) == 0
        assert torch.equal(img.cpu(), host_x[index]) and torch.equal(tgt.cpu(), host_y[index])


@pytest.mark.parametrize("size,stats", [(32, CIFAR), (64, TINY)])
def test_a_normalised_fp32_source_gives_the_batches_of_its_uint8_original(size, stats):
    x, y = make(101, size, size)
    mean = torch.tensor(stats["mean"]).view(1, 3, 1, 1)
    std = torch.tensor(stats["std"]).view(1, 3, 1, 1)
    xf = x.float().div(255).sub(mean).div(std)
    a = D.DeviceDataset(x, y, stats["mean"], stats["std"], stats["pad"])
    b = D.DeviceDataset(xf, y, stats["mean"], stats["std"], stats["pad"])         # default fill: (0 - mean) / std
    g = torch.Generator().manual_seed(3)
    index = torch.randint(0, 101, (150,), generator=g)
    for train in (True, False):
        ra = a.batch(index, epoch=7, seed=1, train=train, return_params=True)
        rb = b.batch(index, epoch=7, seed=1, train=train, return_params=True)
        for u, v in zip(ra, rb):
            assert torch.equal(u, v)
    # an explicit fill is what the padding holds
    c = D.DeviceDataset(xf, y, stats["mean"], stats["std"], stats["pad"], fill=(1.5, -2.0, 0.25))
    params = torch.zeros(1, 3, dtype=torch.int8)
    img, _ = c.batch([0], params=params)
    assert img[0, :, 0, 0].tolist() == [1.5, -2.0, 0.25]


def test_large_images_take_the_global_read_path():
    """3 * H * W above the LDS staging limit (ImageNet-sized uint8 images): same values from guarded global reads."""
    x, y = make(5, 136, 132)
    ds = D.DeviceDataset(x, y, TINY["mean"], TINY["std"], 8)
    index = torch.tensor([4, 0, 4, 2])
    img, tgt, used = ds.batch(index, epoch=1, seed=2, return_params=True)
    want, want_y = restate(x, y, index, used.cpu(), TINY["mean"], TINY["std"], 8)
    assert torch.equal(img.cpu(), want) and torch.equal(tgt.cpu(), want_y)


def test_index_and_params_checks():
    x, y = make(50, 32, 32)
    ds = D.DeviceDataset(x, y, CIFAR["mean"], CIFAR["std"], 4)
    for bad in ([0, 50], [-1, 3]):
        with pytest.raises(IndexError):
            ds.batch(bad)
    with pytest.raises(ValueError):
        ds.batch(torch.tensor([0.5]))
    for bad in ([[9, 0, 0]], [[0, -1, 0]], [[0, 0, 2]]):
        with pytest.raises(ValueError):
            ds.batch([1], params=torch.tensor(bad, dtype=torch.int8))
    with pytest.raises(ValueError):
        ds.batch([1], params=torch.zeros(1, 3, dtype=torch.int8), train=False)
    # device params cannot be checked on the host: the kernel clamps them into range and reports what it used
    wild = torch.tensor([[100, -7, 5], [-128, 127, -1]], dtype=torch.int8).cuda()
    index = torch.tensor([3, 4])
    img, _, used = ds.batch(index, params=wild, return_params=True)
    assert used.cpu().tolist() == [[8, 0, 1], [0, 8, 1]]
    want, _ = restate(x, y, index, used.cpu(), CIFAR["mean"], CIFAR["std"], 4)
    assert torch.equal(img.cpu(), want)


def test_an_out_of_range_device_index_gives_a_zero_image_and_label_minus_one():
    """Guards the guard.  Nothing is provoked: the kernel never forms an address from such an index."""
    x, y = make(97, 32, 32)
    ds = D.DeviceDataset(x, y, CIFAR["mean"], CIFAR["std"], 4)
    index = torch.tensor([5, 96, 97, 0, -1, 2 ** 40, 13, -2 ** 62])
    img, tgt, used = ds.batch(index.cuda(), epoch=2, seed=4, return_params=True)
    ok = torch.tensor([0, 1, 3, 6])
    bad = torch.tensor([2, 4, 5, 7])
    assert tgt.cpu()[bad].tolist() == [-1] * 4
    assert int(img[bad.cuda()].abs().sum()) == 0 and int(used[bad.cuda()].abs().sum()) == 0
    want, want_y = restate(x, y, index[ok], used.cpu()[ok], CIFAR["mean"], CIFAR["std"], 4)
    assert torch.equal(img.cpu()[ok], want) and torch.equal(tgt.cpu()[ok], want_y)
    dy, dx, fl = D.draw_params(4, 2, index[ok], 4)
    assert used.cpu()[ok].tolist() == np.stack([dy, dx, fl], axis=1).tolist()


def test_an_engine_trains_on_device_dataset_batches():
    """The output handed to an engine trains: a few steps of the smoke-sized WRN on one augmented batch per step, the
    loss finite and falling, as engine.smoke() asserts."""
    import torch.nn as nn
    from nbdt.engine import WRNEngine, train_step
    from nbdt.loss import SoftTreeSupLoss
    eng = WRNEngine(num_classes=10, blocks=10, width_factor=2, device="cuda:0", seed=0)
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")
    g = torch.Generator().manual_seed(0)
    y = torch.randint(0, 10, (8,), generator=g)
    x = torch.randn(8, 3, 32, 32, generator=g)
    ds = D.DeviceDataset(x, y, CIFAR["mean"], CIFAR["std"], CIFAR["pad"], device="cuda:0")
    index = torch.arange(8, device="cuda:0")
    params = torch.tensor([[4, 4, 0]] * 8, dtype=torch.int8).cuda()   # the centre crop: one fixed batch, like smoke()
    img, tgt = ds.batch(index, params=params)
    assert torch.equal(img.cpu(), x) and torch.equal(tgt.cpu(), y)
    l0 = train_step(eng, crit, img, tgt, lr=0.05).item()
    for _ in range(5):
        img, tgt = ds.batch(index, params=params)
        l1 = train_step(eng, crit, img, tgt, lr=0.05).item()
    assert math.isfinite(l0) and math.isfinite(l1) and l1 < l0, (l0, l1)
    # and on freshly drawn crops the step stays finite
    for epoch in range(3):
        img, tgt = ds.batch(index, epoch=epoch, seed=1)
        assert math.isfinite(train_step(eng, crit, img, tgt, lr=0.05).item())
