"""nbdt_policy_batch / nbdt.data.DeviceDataset(policy=, erase_prob=) on the MI355X against the recipe restated on the CPU:
zero-padded crop, flip, nbdt.data.policy_reference (Pillow's rules, checked against Pillow in tests/test_policy.py),
.float().div(255).sub(mean).div(std), the erase rectangle set to 0.0.  Every comparison is of the fp32 bit patterns: nothing
is rounded or reordered, so there is no tolerance."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import nbdt_path
from nbdt import _C
from nbdt import data as D

pytestmark = pytest.mark.gpu

CIFAR = D.DATASET_STATS["CIFAR10"]
NOP = (0, 0, 0, 0, 0, 0, 0)          # Identity, no erase
_MAGNITUDE_FREE = (0, 12, 13)        # Identity, AutoContrast, Equalize: bin and sign do not matter


def fixtures(H, W, seed=0):
    """A random, a low-contrast (40..199), a four-level and a constant image."""
    rng = np.random.default_rng(1000 * H + W + seed)
    const = np.empty((3, H, W), dtype=np.uint8)
    const[0], const[1], const[2] = 7, 128, 255
    return np.stack([rng.integers(0, 256, (3, H, W), dtype=np.uint8), rng.integers(40, 200, (3, H, W), dtype=np.uint8),
                     (rng.integers(0, 4, (3, H, W)) * 60 + 20).astype(np.uint8), const])


def bits_equal(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def restate(x_u8, index, crop, policy, mean, std, pad, cache=None):
    """The recipe on the CPU for samples `index` of x_u8 (numpy [N,3,H,W]) under crop = [(dy, dx, flip)] and policy =
    [(op, bin, sign, top, left, h, w)]: fp32 [B,3,H,W].  cache: the bytes of a (sample, crop, op, magnitude) seen before."""
    cache = {} if cache is None else cache
    H, W = x_u8.shape[2:]
    out = np.empty((len(index), 3, H, W), dtype=np.uint8)
    for j, (i, (dy, dx, fl), p) in enumerate(zip(index, crop, policy)):
        op, b, sg = int(p[0]), int(p[1]), int(p[2])
        if op in _MAGNITUDE_FREE:
            b, sg = 0, 0
        elif op not in D.POLICY_SIGNED:
            sg = 0
        key = (int(i), int(dy), int(dx), int(fl), op, b, sg)
        if key not in cache:
            img = np.pad(x_u8[i], ((0, 0), (pad, pad), (pad, pad)))[:, dy:dy + H, dx:dx + W]        # byte 0, before conversion
            if fl:
                img = img[:, :, ::-1]
            cache[key] = D.policy_reference(np.ascontiguousarray(img), op, b, sg)
        out[j] = cache[key]
    mean = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    f = torch.from_numpy(out).float().div(255).sub(mean).div(std)
    for j, p in enumerate(policy):
        t, l, h, w = (int(v) for v in p[3:])
        f[j, :, t:t + h, l:l + w] = 0.0
    return f


def dataset(x_u8, pad, **kw):
    x = torch.from_numpy(x_u8)
    y = torch.arange(x.shape[0]) % 10
    return D.DeviceDataset(x, y, CIFAR["mean"], CIFAR["std"], pad, **kw), y


@pytest.mark.parametrize("H,W", [(32, 32), (64, 64), (24, 40), (9, 7)])
def test_every_op_bin_and_sign_in_one_launch_equals_the_restatement(H, W):
    """Explicit policy_params covering every (op, bin, sign) on every fixture, centre crop, no flip: one launch, bit-equal.
    9 x 7 takes the scalar load and store paths, 24 x 40 is not square (Rotate's +-90 is then the general path)."""
    pad = 4
    x = fixtures(H, W)
    ds, y = dataset(x, pad)
    combos = [(i, op, b, sg) for i in range(len(x)) for op in range(14) for b in range(31) for sg in (0, 1)]
    index = torch.tensor([c[0] for c in combos])
    policy = torch.tensor([(op, b, sg, 0, 0, 0, 0) for _, op, b, sg in combos], dtype=torch.int32)
    crop = torch.tensor([[pad, pad, 0]] * len(combos), dtype=torch.int8)
    img, tgt, used = ds.batch(index, params=crop, policy_params=policy, return_policy_params=True)
    assert torch.equal(used.cpu(), policy) and torch.equal(tgt.cpu(), y[index])
    want = restate(x, index.tolist(), crop.tolist(), policy.tolist(), CIFAR["mean"], CIFAR["std"], pad, cache={})
    if not bits_equal(img, want):
        bad = (img.cpu() != want).flatten(1).any(1).nonzero().flatten().tolist()
        raise AssertionError(f"{len(bad)} samples differ, first (fixture, op, bin, sign): {[combos[j] for j in bad[:8]]}")


def test_autocontrast_luts_for_every_range():
    """AutoContrast's fp64 scale = 255 / (hi - lo) and int(v * scale + offset) for every hi - lo in 1..255 at a few lo:
    9 x 7 images that contain both extremes (and every value between them when there is room)."""
    rng = np.random.default_rng(11)
    imgs = []
    for d in range(1, 256):
        for lo in sorted({0, 1, (255 - d) // 2, 255 - d}):
            v = rng.integers(lo, lo + d + 1, (3, 63))
            v[:, :min(d + 1, 63)] = lo + np.linspace(0, d, min(d + 1, 63)).round().astype(np.int64)
            v[:, 0], v[:, 1] = lo, lo + d
            imgs.append(rng.permuted(v, axis=1).reshape(3, 9, 7).astype(np.uint8))
    x = np.stack(imgs)
    ds, _ = dataset(x, 2)
    B = len(x)
    policy = torch.tensor([(12, 0, 0, 0, 0, 0, 0)] * B, dtype=torch.int32)
    crop = torch.tensor([[2, 2, 0]] * B, dtype=torch.int8)
    img, _ = ds.batch(torch.arange(B), params=crop, policy_params=policy)
    want = restate(x, range(B), crop.tolist(), policy.tolist(), CIFAR["mean"], CIFAR["std"], 2)
    assert bits_equal(img, want)
    assert not bits_equal(img, restate(x, range(B), crop.tolist(), [NOP] * B, CIFAR["mean"], CIFAR["std"], 2))


@pytest.mark.parametrize("H,W,pad", [(32, 32, 4), (24, 40, 3), (9, 7, 2)])
def test_random_crops_and_flips_compose_with_random_ops(H, W, pad):
    """The op sees the cropped and flipped image, padding included: crop, then flip, then policy_reference."""
    rng = np.random.default_rng(H)
    x = np.concatenate([fixtures(H, W), fixtures(H, W, seed=1)])
    ds, y = dataset(x, pad)
    B = 600
    index = rng.integers(0, len(x), B)
    crop = np.stack([rng.integers(0, 2 * pad + 1, B), rng.integers(0, 2 * pad + 1, B), rng.integers(0, 2, B)], axis=1)
    policy = np.stack([rng.integers(0, 14, B), rng.integers(0, 31, B), rng.integers(0, 2, B)] + [np.zeros(B, np.int64)] * 4,
                      axis=1)
    img, tgt = ds.batch(torch.from_numpy(index), params=torch.from_numpy(crop).to(torch.int8),
                        policy_params=torch.from_numpy(policy))              # int64 host params are accepted
    want = restate(x, index.tolist(), crop.tolist(), policy.tolist(), CIFAR["mean"], CIFAR["std"], pad)
    assert bits_equal(img, want) and torch.equal(tgt.cpu(), y[index])
    assert sorted(set(policy[:, 0].tolist())) == list(range(14)) and crop[:, 2].min() == 0 and crop[:, 2].max() == 1


@pytest.mark.parametrize("B", [1, 37, 512])
@pytest.mark.parametrize("n,H,W,pad", [(211, 32, 32, 4), (61, 9, 7, 2)])
def test_generated_draws_equal_draw_policy_params_and_the_restatement(B, n, H, W, pad):
    """No params given: the kernel's own draws are draw_params and draw_policy_params of (seed, epoch, index), and the images
    follow them.  Indices repeat; N is prime."""
    rng = np.random.default_rng(n)
    x = rng.integers(0, 256, (n, 3, H, W), dtype=np.uint8)
    ds, y = dataset(x, pad, policy="ta_wide", erase_prob=0.5)
    index = torch.from_numpy(rng.integers(0, n, B))
    if B > 2:
        index[1] = index[0]
        index[-1] = index[0]
    for seed, epoch in ((0, 0), (5, 199)):
        img, tgt, cused, pused = ds.batch(index, epoch=epoch, seed=seed, return_params=True, return_policy_params=True)
        want_c = np.stack(D.draw_params(seed, epoch, index, pad), axis=1)
        want_p = np.stack(D.draw_policy_params(seed, epoch, index, H, W, erase_prob=0.5), axis=1)
        assert torch.equal(cused.cpu().long(), torch.from_numpy(want_c))
        assert pused.dtype == torch.int32 and torch.equal(pused.cpu().long(), torch.from_numpy(want_p))
        want = restate(x, index.tolist(), want_c.tolist(), want_p.tolist(), CIFAR["mean"], CIFAR["std"], pad)
        assert bits_equal(img, want) and torch.equal(tgt.cpu(), y[index])
    if B == 512:
        assert len(set(want_p[:, 0].tolist())) == 14 and 0.3 < float(np.mean(want_p[:, 5] > 0)) < 0.7
    # a device index takes the same path; erase_prob = 0 with the policy on draws the same ops and erases nothing
    img2, _ = ds.batch(index.cuda(), epoch=199, seed=5)
    assert bits_equal(img2, img)
    ds0, _ = dataset(x, pad, policy="ta_wide")
    _, _, p0 = ds0.batch(index, epoch=199, seed=5, return_policy_params=True)
    assert torch.equal(p0[:, :3], pused[:, :3]) and not p0[:, 3:].any()
    # erase only: every op is Identity
    dse, _ = dataset(x, pad, erase_prob=0.5)
    _, _, pe = dse.batch(index, epoch=199, seed=5, return_policy_params=True)
    assert not pe[:, :3].any() and torch.equal(pe[:, 3:], pused[:, 3:])


@pytest.mark.parametrize("H,W,pad", [(32, 32, 4), (64, 64, 8), (9, 7, 2)])
def test_identity_through_the_policy_kernel_is_nbdt_augment_batch(H, W, pad):
    rng = np.random.default_rng(W)
    x = rng.integers(0, 256, (97, 3, H, W), dtype=np.uint8)
    ds, _ = dataset(x, pad)
    index = torch.from_numpy(rng.integers(0, 97, 300))
    plain = ds.batch(index, epoch=2, seed=3, return_params=True)
    ident = ds.batch(index, epoch=2, seed=3, return_params=True, policy_params=torch.tensor([NOP] * 300, dtype=torch.int32))
    for u, v in zip(plain, ident):
        assert torch.equal(u, v)
    assert bits_equal(plain[0], ident[0])
    # evaluation never applies a policy: the same launch and bits as a dataset without one
    dsp, _ = dataset(x, pad, policy="ta_wide", erase_prob=1.0)
    assert bits_equal(dsp.batch(index, train=False)[0], ds.batch(index, train=False)[0])
    assert not dsp.batch(index, train=False, return_policy_params=True)[2].any()
    with pytest.raises(ValueError, match="train=False"):
        dsp.batch(index, train=False, policy_params=torch.tensor([NOP] * 300, dtype=torch.int32))


@pytest.mark.parametrize("H,W", [(32, 32), (9, 7)])
def test_erased_pixels_are_zero_and_all_others_untouched(H, W):
    pad = 2
    rng = np.random.default_rng(H + 1)
    x = rng.integers(1, 256, (16, 3, H, W), dtype=np.uint8)
    ds, _ = dataset(x, pad)
    rects = [(0, 0, 1, 1), (H - 1, W - 1, 1, 1), (3, 2, 1, 1), (0, 0, H - 1, W - 1), (1, 1, H - 1, W - 1), (0, 1, H - 1, W - 1),
             (1, 0, H - 1, W - 1), (0, 2, 3, W - 2), (2, 0, H - 2, 3), (H - 2, 0, 2, W - 1), (0, W - 2, H - 1, 2), (2, 1, 4, 3),
             (0, 0, 0, 0), (3, 3, 0, 2), (3, 3, 2, 0)]
    B = len(rects)
    ops_ = rng.integers(0, 14, B)
    policy = torch.tensor([(int(o), 9, 1) + r for o, r in zip(ops_, rects)], dtype=torch.int32)
    clean = policy.clone()
    clean[:, 3:] = 0
    crop = torch.from_numpy(np.stack([rng.integers(0, 2 * pad + 1, B), rng.integers(0, 2 * pad + 1, B),
                                      rng.integers(0, 2, B)], axis=1)).to(torch.int8)
    index = torch.arange(B)
    base, _ = ds.batch(index, params=crop, policy_params=clean)
    img, _, used = ds.batch(index, params=crop, policy_params=policy, return_policy_params=True)
    base, img = base.cpu(), img.cpu()
    for j, (t, l, h, w) in enumerate(rects):
        inside = torch.zeros(3, H, W, dtype=torch.bool)
        inside[:, t:t + h, l:l + w] = True
        assert int(inside.sum()) == 3 * h * w
        z = img[j][inside]
        assert not z.any() and not torch.signbit(z).any(), rects[j]                # exactly +0.0f
        assert torch.equal(img[j][~inside].view(torch.int32), base[j][~inside].view(torch.int32)), rects[j]
        assert used[j, 3:].tolist() == (list(rects[j]) if h and w else [0, 0, 0, 0])
    assert bool((base != 0).all())            # (no pixel normalises to 0: the zeros above are the erase's)
    want = restate(x, range(B), crop.tolist(), policy.tolist(), CIFAR["mean"], CIFAR["std"], pad)
    assert bits_equal(img, want)


def test_a_shard_returns_the_whole_datasets_batch_for_the_indices_it_owns():
    rng = np.random.default_rng(4)
    x = rng.integers(0, 256, (101, 3, 32, 32), dtype=np.uint8)
    kw = dict(policy="ta_wide", erase_prob=0.5)
    whole, _ = dataset(x, 4, **kw)
    part, _ = dataset(x, 4, shard=(1, 3), **kw)
    lo, hi = D.shard_range(101, 1, 3)
    assert tuple(part.shard_range) == (lo, hi) == (33, 67) and len(part) == 34
    index = torch.from_numpy(rng.integers(lo, hi, 200))
    a = whole.batch(index, epoch=7, seed=1, return_params=True, return_policy_params=True)
    b = part.batch(index, epoch=7, seed=1, return_params=True, return_policy_params=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert bits_equal(a[0], b[0])
    with pytest.raises(ValueError, match="shard owns"):
        part.batch(torch.tensor([lo - 1]))
    # a device index outside the shard: a zero image, label -1, zero params
    img, tgt, cu, pu = part.batch(torch.tensor([lo, lo - 1, hi, hi - 1], device="cuda"), return_params=True,
                                  return_policy_params=True)
    assert tgt.tolist()[1:3] == [-1, -1] and tgt.tolist()[0] >= 0 and tgt.tolist()[3] >= 0
    assert not img[1:3].any() and not cu[1:3].any() and not pu[1:3].any() and bool(img[0].any()) and bool(img[3].any())


def test_a_device_index_outside_the_dataset_gives_a_zero_image_and_label_minus_one():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (50, 3, 32, 32), dtype=np.uint8)
    ds, y = dataset(x, 4, policy="ta_wide", erase_prob=1.0)
    index = torch.tensor([3, 50, -1, 2 ** 40, -2 ** 62, 49, 2 ** 63 - 1], device="cuda")
    img, tgt, cu, pu = ds.batch(index, return_params=True, return_policy_params=True)
    assert tgt.tolist() == [int(y[3]), -1, -1, -1, -1, int(y[49]), -1]
    for j in (1, 2, 3, 4, 6):
        assert not img[j].any() and not cu[j].any() and not pu[j].any()
    good = ds.batch(torch.tensor([3, 49]))[0]
    assert bits_equal(img[[0, 5]], good)
    with pytest.raises(IndexError):
        ds.batch(torch.tensor([3, 50]))


def test_refusals_come_before_any_launch(monkeypatch):
    from nbdt import ops

    def no_launch(*a, **k):
        raise AssertionError("a launch was attempted")
    y = torch.zeros(4, dtype=torch.long)
    xf = torch.zeros(4, 3, 32, 32)
    xbig = torch.zeros(4, 3, 129, 128, dtype=torch.uint8)
    for bad in (xf, xbig):
        for kw in (dict(policy="ta_wide"), dict(erase_prob=0.1)):
            with pytest.raises(ValueError, match="uint8 dataset|at most 49152"):
                D.DeviceDataset(bad, y, CIFAR["mean"], CIFAR["std"], 4, **kw)
    for kw in (dict(policy="rand_augment"), dict(erase_prob=1.5), dict(erase_prob=float("nan")),
               dict(erase_prob=0.1, erase_scale=(0.5, 0.2)), dict(erase_prob=0.1, erase_ratio=(0.0, 1.0))):
        with pytest.raises(ValueError):
            D.DeviceDataset(torch.zeros(4, 3, 32, 32, dtype=torch.uint8), y, CIFAR["mean"], CIFAR["std"], 4, **kw)
    monkeypatch.setattr(ops, "policy_batch", no_launch)
    monkeypatch.setattr(ops, "augment_batch", no_launch)
    index = torch.arange(4)
    for ds in (D.DeviceDataset(xf, y, CIFAR["mean"], CIFAR["std"], 4), D.DeviceDataset(xbig, y, CIFAR["mean"], CIFAR["std"], 4)):
        with pytest.raises(ValueError, match="uint8 dataset|at most 49152"):          # plain datasets, policy_params given
            ds.batch(index, policy_params=torch.tensor([NOP] * 4, dtype=torch.int32))
    ds = D.DeviceDataset(torch.zeros(4, 3, 32, 32, dtype=torch.uint8), y, CIFAR["mean"], CIFAR["std"], 4, policy="ta_wide")
    for row in ((14, 0, 0, 0, 0, 0, 0), (-1, 0, 0, 0, 0, 0, 0), (0, 31, 0, 0, 0, 0, 0), (0, -1, 0, 0, 0, 0, 0),
                (0, 0, 2, 0, 0, 0, 0), (0, 0, -1, 0, 0, 0, 0), (0, 0, 0, -1, 0, 1, 1), (0, 0, 0, 0, -1, 1, 1),
                (0, 0, 0, 30, 0, 3, 1), (0, 0, 0, 0, 30, 1, 3), (0, 0, 0, 0, 0, -1, 1), (0, 0, 0, 0, 0, 1, 33)):
        with pytest.raises(ValueError, match="policy_params outside"):
            ds.batch(index, policy_params=torch.tensor([NOP, row, NOP, NOP], dtype=torch.int32))
    for bad in (torch.zeros(4, 6, dtype=torch.int32), torch.zeros(3, 7, dtype=torch.int32), torch.zeros(4, 7)):
        with pytest.raises(ValueError, match="integer"):
            ds.batch(index, policy_params=bad)
    # the C entry refuses the same sources by itself
    out, lab = torch.empty(4, 3, 32, 32, device="cuda"), torch.empty(4, dtype=torch.int64, device="cuda")
    monkeypatch.undo()
    with pytest.raises(_C.NBDTHipError, match="uint8"):
        ops.policy_batch(xf.cuda(), y.cuda(), index.cuda(), out, lab, 4, True, CIFAR["mean"], CIFAR["std"])
    with pytest.raises(_C.NBDTHipError, match="49152"):
        ops.policy_batch(xbig.cuda(), y.cuda(), index.cuda(), torch.empty(4, 3, 129, 128, device="cuda"), lab, 4, True,
                         CIFAR["mean"], CIFAR["std"])
    # ... and policy_in without the table its operations would index
    x8 = torch.zeros(4, 3, 32, 32, dtype=torch.uint8, device="cuda")
    rows = torch.tensor([NOP, (5, 15, 0, 0, 0, 0, 0), NOP, NOP], dtype=torch.int32, device="cuda")
    with pytest.raises(_C.NBDTHipError, match="policy table"):
        ops.policy_batch(x8, y.cuda(), index.cuda(), out, lab, 4, True, CIFAR["mean"], CIFAR["std"], policy=False,
                         policy_table=None, policy_in=rows)


def test_device_policy_params_are_clamped_not_trusted():
    """policy_params on the device cannot be checked on the host: the kernel clamps them, and reports what it used."""
    rng = np.random.default_rng(6)
    x = rng.integers(0, 256, (8, 3, 32, 32), dtype=np.uint8)
    ds, _ = dataset(x, 4)
    wild = torch.tensor([(99, 99, 7, -5, -5, 99, 99), (-3, -3, -1, 40, 40, 5, 5), (5, 15, 0, 31, 31, 2 ** 30, 2 ** 30),
                         (2 ** 31 - 1, -2 ** 31, 1, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31)], dtype=torch.int32)
    crop = torch.tensor([[4, 4, 0]] * 4, dtype=torch.int8)
    img, _, used = ds.batch(torch.arange(4), params=crop, policy_params=wild.cuda(), return_policy_params=True)
    assert used.tolist() == [[13, 30, 1, 0, 0, 32, 32], [0, 0, 1, 31, 31, 1, 1], [5, 15, 0, 31, 31, 1, 1],
                             [13, 0, 1, 0, 0, 0, 0]]
    want = restate(x, range(4), crop.tolist(), used.tolist(), CIFAR["mean"], CIFAR["std"], 4)
    assert bits_equal(img, want) and not img[0].any()


def test_a_batch_is_the_concatenation_of_its_halves():
    rng = np.random.default_rng(7)
    x = rng.integers(0, 256, (307, 3, 32, 32), dtype=np.uint8)
    ds, _ = dataset(x, 4, policy="ta_wide", erase_prob=0.25)
    a, b = torch.from_numpy(rng.integers(0, 307, 100)), torch.from_numpy(rng.integers(0, 307, 28))
    kw = dict(epoch=3, seed=9, return_params=True, return_policy_params=True)
    whole, pa, pb = ds.batch(torch.cat([a, b]), **kw), ds.batch(a, **kw), ds.batch(b, **kw)
    for w, u, v in zip(whole, pa, pb):
        assert torch.equal(w, torch.cat([u, v]))
    assert bits_equal(whole[0], torch.cat([pa[0], pb[0]]))
    again = ds.batch(torch.cat([a, b]), **kw)
    assert bits_equal(whole[0], again[0]) and whole[0].data_ptr() != again[0].data_ptr()      # the launch repeats to the bit
    other = ds.batch(torch.cat([a, b]), epoch=4, seed=9, return_policy_params=True)
    assert not torch.equal(other[2], whole[3])                  # the epoch is part of the draw


def test_an_engine_trains_on_policy_batches_and_repeats_to_the_bit():
    import torch.nn as nn
    from nbdt import ops
    from nbdt.engine import WRNEngine, train_step
    from nbdt.loss import SoftTreeSupLoss
    rng = np.random.default_rng(8)
    x = rng.integers(0, 256, (64, 3, 32, 32), dtype=np.uint8)
    ds, _ = dataset(x, 4, policy="ta_wide", erase_prob=0.25, device="cuda:0")
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")
    ops.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            eng = WRNEngine(num_classes=10, blocks=10, width_factor=2, device="cuda:0", seed=0)
            losses = []
            for step in range(3):
                img, tgt = ds.batch(torch.arange(8 * step, 8 * step + 8), epoch=step, seed=1)
                losses.append(train_step(eng, crit, img, tgt, lr=0.05))
            runs.append(torch.stack(losses).cpu())
    finally:
        ops.set_deterministic(False)
    assert all(math.isfinite(v) for v in runs[0].tolist()), runs[0]
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), runs


def test_main_trains_with_the_policy_and_random_erasing(tmp_path, monkeypatch):
    from nbdt import ops
    spec = importlib.util.spec_from_file_location("nbdt_main", os.path.join(nbdt_path.PKG_DIR, "main.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    monkeypatch.chdir(tmp_path)
    g = torch.Generator().manual_seed(0)
    blob = {"train_x": torch.randint(0, 256, (128, 3, 32, 32), dtype=torch.uint8, generator=g),
            "train_y": torch.randint(0, 10, (128,), generator=g),
            "test_x": torch.randint(0, 256, (64, 3, 32, 32), dtype=torch.uint8, generator=g),
            "test_y": torch.randint(0, 10, (64,), generator=g)}
    torch.save(blob, "data.pt")
    calls = {"policy": 0, "plain": 0}
    policy_batch, augment_batch = ops.policy_batch, ops.augment_batch

    def count_policy(*a, **k):
        calls["policy"] += 1
        assert k["policy"] is True and k["erase_prob"] == 0.25
        return policy_batch(*a, **k)

    def count_plain(*a, **k):
        calls["plain"] += 1
        return augment_batch(*a, **k)
    monkeypatch.setattr(ops, "policy_batch", count_policy)
    monkeypatch.setattr(ops, "augment_batch", count_plain)
    acc, _ = M.main("--arch ResNet18 --dataset CIFAR10 --batch-size 64 --data-file data.pt --lr 0.05 --epochs 1 "
                    "--augment reference --auto-augment ta_wide --random-erase 0.25".split())
    assert 0.0 <= acc <= 100.0 and math.isfinite(acc)
    assert calls["policy"] == 2 and calls["plain"] >= 1       # two training steps through the policy kernel; evaluation plain
    # a float data file is refused by name
    torch.save({k: (v.float() if k.endswith("_x") else v) for k, v in blob.items()}, "float.pt")
    with pytest.raises(SystemExit, match="uint8"):
        M.main("--arch ResNet18 --dataset CIFAR10 --batch-size 64 --data-file float.pt --epochs 1 --augment reference "
               "--random-erase 0.25".split())
