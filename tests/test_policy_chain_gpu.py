"""nbdt_policy_chain_batch / nbdt.data.DeviceDataset(policy="ra" | "cifar10" | [sub-policies]) on the MI355X against the
recipe restated on the CPU: zero-padded crop, flip, nbdt.data.chain_reference (Pillow's rules per op, checked against Pillow
in tests/test_policy_chain.py), .float().div(255).sub(mean).div(std), the erase rectangle set to 0.0.  Every comparison is of
the fp32 bit patterns: nothing is rounded or reordered, so there is no tolerance."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import nbdt_path
from nbdt import _C
from nbdt import data as D

pytestmark = pytest.mark.gpu

CIFAR = D.DATASET_STATS["CIFAR10"]
K = D.CHAIN_MAX_OPS
STATS = (8, 12, 13)                   # Contrast, AutoContrast, Equalize: the ops that need per-image statistics
GEOMETRIC = (1, 2, 3, 4, 5)
USER = [[("Rotate", 1.0, 3), ("Invert", 0.0, None)], [("Equalize", 0.0, None), ("Solarize", 1.0, 9), ("Color", 1.0, 4)]]


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


def restate(x_u8, index, crop, chains, erase, table, pad, mean=CIFAR["mean"], std=CIFAR["std"]):
    """The recipe on the CPU for samples `index` of x_u8 (numpy [N,3,H,W]) under crop = [(dy, dx, flip)], chains =
    [[(op, bin, sign)] * 4] and erase = [(top, left, h, w)]: fp32 [B,3,H,W]."""
    H, W = x_u8.shape[2:]
    out = np.empty((len(index), 3, H, W), dtype=np.uint8)
    for j, (i, (dy, dx, fl), chain) in enumerate(zip(index, crop, chains)):
        img = np.pad(x_u8[i], ((0, 0), (pad, pad), (pad, pad)))[:, dy:dy + H, dx:dx + W]        # byte 0, before conversion
        if fl:
            img = img[:, :, ::-1]
        out[j] = D.chain_reference(np.ascontiguousarray(img), [s for s in chain if s[0] != 0], table)
    mean = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    f = torch.from_numpy(out).float().div(255).sub(mean).div(std)
    for j, (t, l, h, w) in enumerate(erase):
        f[j, :, t:t + h, l:l + w] = 0.0
    return f


def dataset(x_u8, pad, **kw):
    x = torch.from_numpy(x_u8)
    y = torch.arange(x.shape[0]) % 10
    return D.DeviceDataset(x, y, CIFAR["mean"], CIFAR["std"], pad, **kw), y


def differing(img, want, labels):
    bad = (img.cpu().view(torch.int32) != want.view(torch.int32)).flatten(1).any(1).nonzero().flatten().tolist()
    return f"{len(bad)} samples differ, first: {[labels[j] for j in bad[:8]]}"


def centre(B, pad):
    return torch.tensor([[pad, pad, 0]] * B, dtype=torch.int8)


def launch(ds, x, index, chains, pad, crop=None, erase=None, table=None):
    """One launch with explicit chains (and crops, and rectangles), and its restatement."""
    B = len(index)
    crop = centre(B, pad) if crop is None else crop
    erase = torch.zeros(B, 4, dtype=torch.int32) if erase is None else erase
    chains = torch.as_tensor(np.asarray(chains), dtype=torch.int32)
    img, tgt, cused, eused = ds.batch(torch.as_tensor(index), params=crop, chain_params=chains, erase_params=erase,
                                      return_chain_params=True, return_erase_params=True)
    assert torch.equal(cused.cpu(), chains) and torch.equal(eused.cpu(), erase)
    table = D.chain_table(ds.policy, *x.shape[2:]) if table is None else table
    return img, tgt, restate(x, list(index), crop.tolist(), chains.tolist(), erase.tolist(), table, pad)


@pytest.mark.parametrize("H,W", [(32, 32), (9, 7)])
def test_chains_of_one_cover_every_op_bin_and_sign(H, W):
    """Every (op, bin, sign) of the ra table on every fixture as a chain of length 1, the op in slot j % 4: one launch,
    bit-equal.  9 x 7 takes the scalar load path and the unpacked store paths."""
    pad = 4
    x = fixtures(H, W)
    ds, y = dataset(x, pad, policy="ra")
    combos = [(i, op, b, sg) for i in range(len(x)) for op in range(15) for b in range(31) for sg in (0, 1)]
    chains = np.zeros((len(combos), K, 3), dtype=np.int64)
    for j, (_, op, b, sg) in enumerate(combos):
        chains[j, j % K] = (op, b, sg)
    index = [c[0] for c in combos]
    img, tgt, want = launch(ds, x, index, chains, pad)
    assert torch.equal(tgt.cpu(), y[index])
    assert bits_equal(img, want), differing(img, want, combos)


@pytest.mark.parametrize("H,W,pad", [(32, 32, 4), (9, 7, 2), (24, 40, 3)])
def test_a_chain_of_one_on_trivial_augments_table_is_nbdt_policy_batch(H, W, pad):
    """The same op, crop and rectangle through both kernels, on a table built with TrivialAugmentWide's ranges: the same
    bits.  (The statistics, the op's pixel rule and the output pass are shared code; this pins that they stay so.)"""
    from nbdt import ops
    rng = np.random.default_rng(H * W)
    x = np.concatenate([fixtures(H, W), fixtures(H, W, seed=1)])
    plain, y = dataset(x, pad)
    B = 14 * 31 * 2
    index = torch.from_numpy(rng.integers(0, len(x), B))
    crop = torch.from_numpy(np.stack([rng.integers(0, 2 * pad + 1, B), rng.integers(0, 2 * pad + 1, B),
                                      rng.integers(0, 2, B)], axis=1)).to(torch.int8)
    top, left = rng.integers(0, H, B), rng.integers(0, W, B)
    rect = np.stack([top, left, rng.integers(0, H - top + 1), rng.integers(0, W - left + 1)], axis=1)
    rect[(rect[:, 2] == 0) | (rect[:, 3] == 0)] = 0
    one = np.array([(op, b, sg) for op in range(14) for b in range(31) for sg in (0, 1)])
    policy = torch.from_numpy(np.concatenate([one, rect], axis=1)).to(torch.int32)
    want, wtgt = plain.batch(index, params=crop, policy_params=policy)
    chains = np.zeros((B, K, 3), dtype=np.int32)
    chains[np.arange(B), np.arange(B) % K] = one
    table = torch.from_numpy(D.chain_table("ta_wide", H, W).copy()).cuda()
    img = torch.empty_like(want)
    tgt = torch.empty_like(wtgt)
    ops.policy_chain_batch(plain.x, plain.y, index.cuda(), img, tgt, pad, True, plain.mean, plain.std, table, 31, num_ops=1,
                           params_in=crop.cuda(), chain_in=torch.from_numpy(chains).cuda(),
                           erase_in=torch.from_numpy(rect).to(torch.int32).cuda())
    assert torch.equal(tgt, wtgt) and bits_equal(img, want), differing(img, want.cpu(), policy.tolist())


@pytest.mark.parametrize("policy,n", [("ra", 31), ("cifar10", 10)])
@pytest.mark.parametrize("H,W", [(32, 32), (24, 40)])
def test_all_225_ordered_pairs_in_one_launch(H, W, policy, n):
    """Every ordered pair of the 15 ops on every fixture, bins and signs at random, the pair in two of the four slots.  The
    pairs among Contrast, AutoContrast and Equalize (Equalize -> Equalize included) need their statistics collected twice:
    a stale histogram or a missing barrier shows here."""
    pad = 4
    rng = np.random.default_rng(n)
    x = fixtures(H, W)
    ds, _ = dataset(x, pad, policy=policy)
    combos = [(i, p, q) for i in range(len(x)) for p in range(15) for q in range(15)]
    chains = np.zeros((len(combos), K, 3), dtype=np.int64)
    for j, (_, p, q) in enumerate(combos):
        a, b = sorted(rng.choice(K, 2, replace=False).tolist())
        chains[j, a] = (p, rng.integers(0, n), rng.integers(0, 2))
        chains[j, b] = (q, rng.integers(0, n), rng.integers(0, 2))
    img, _, want = launch(ds, x, [c[0] for c in combos], chains, pad)
    assert bits_equal(img, want), differing(img, want, combos)
    both = [j for j, (_, p, q) in enumerate(combos) if p in STATS and q in STATS]
    assert len(both) == 9 * len(x)
    # on some fixture Equalize twice is not Equalize once: the second histogram has work of its own
    twice = [j for j in both if combos[j][1:] == (13, 13)]
    once = restate(x, range(len(x)), [(pad, pad, 0)] * len(x), [[(13, 0, 0)]] * len(x), [(0, 0, 0, 0)] * len(x),
                   D.chain_table(policy, H, W), pad)
    assert [combos[j][0] for j in twice] == list(range(len(x))) and not bits_equal(want[twice], once)


@pytest.mark.parametrize("length", [3, 4])
def test_random_chains_with_identities_and_geometry_before_statistics(length):
    """64 images per group at 32 x 32, random crops, flips and rectangles: random chains of `length` ops; the same with an
    Identity forced into each position in turn; all-Identity; and a geometric op followed by Sharpness, AutoContrast and
    Equalize, whose statistics then include the zero fill."""
    H = W = 32
    pad = 4
    rng = np.random.default_rng(length)
    x = np.concatenate([fixtures(H, W), fixtures(H, W, seed=1)])
    ds, _ = dataset(x, pad, policy="ra")

    def random_chain():
        c = np.zeros((K, 3), dtype=np.int64)
        c[:length] = np.stack([rng.integers(1, 15, length), rng.integers(0, 31, length), rng.integers(0, 2, length)], axis=1)
        return c
    chains = [random_chain() for _ in range(64)]
    for pos in range(length):
        for _ in range(64 // length):
            c = random_chain()
            c[pos] = 0
            chains.append(c)
    chains += [np.zeros((K, 3), dtype=np.int64)] * 8
    for g in GEOMETRIC:
        for follow in (9, 12, 13):
            for _ in range(4):
                c = random_chain()
                c[0] = (g, rng.integers(10, 31), rng.integers(0, 2))
                c[1, 0] = follow
                chains.append(c)
    chains = np.stack(chains)
    B = len(chains)
    index = rng.integers(0, len(x), B)
    crop = torch.from_numpy(np.stack([rng.integers(0, 2 * pad + 1, B), rng.integers(0, 2 * pad + 1, B),
                                      rng.integers(0, 2, B)], axis=1)).to(torch.int8)
    top, left = rng.integers(0, H, B), rng.integers(0, W, B)
    rect = np.stack([top, left, rng.integers(0, H - top + 1), rng.integers(0, W - left + 1)], axis=1)
    rect[(rect[:, 2] == 0) | (rect[:, 3] == 0) | (rng.random(B) < 0.5)] = 0
    img, _, want = launch(ds, x, index.tolist(), chains, pad, crop=crop, erase=torch.from_numpy(rect).to(torch.int32))
    assert bits_equal(img, want), differing(img, want, chains.tolist())
    # all-Identity is the plain crop / flip / normalise launch
    ident = slice(64 + (64 // length) * length, 64 + (64 // length) * length + 8)
    plain, _ = dataset(x, pad)
    base, _ = plain.batch(torch.from_numpy(index[ident]), params=crop[ident])
    for j, (t, l, h, w) in enumerate(rect[ident].tolist()):
        base[j, :, t:t + h, l:l + w] = 0.0
    assert bits_equal(img[ident], base)


@pytest.mark.parametrize("B", [1, 37, 512])
@pytest.mark.parametrize("kw", [dict(policy="ra", policy_ops=1, policy_magnitude=0), dict(policy="ra"),
                                dict(policy="ra", policy_ops=3, policy_magnitude=30),
                                dict(policy="ra", policy_ops=4, policy_magnitude=15), dict(policy="cifar10"), dict(policy=USER)],
                         ids=["ra-1-0", "ra-2-9", "ra-3-30", "ra-4-15", "cifar10", "user"])
def test_generated_draws_equal_draw_chain_params_and_the_restatement(B, kw):
    """No params given: the kernel's own draws are draw_params, draw_chain_params and the erase rectangle of
    draw_policy_params of (seed, epoch, index), and the images follow them.  Indices repeat; N is prime."""
    n, H, W, pad = 211, 32, 32, 4
    rng = np.random.default_rng(n)
    x = rng.integers(0, 256, (n, 3, H, W), dtype=np.uint8)
    ds, y = dataset(x, pad, erase_prob=0.5, **kw)
    index = torch.from_numpy(rng.integers(0, n, B))
    if B > 2:
        index[1] = index[0]
        index[-1] = index[0]
    table = D.chain_table(kw["policy"], H, W)
    for seed, epoch in ((0, 0), (5, 199)):
        img, tgt, cused, chused, eused = ds.batch(index, epoch=epoch, seed=seed, return_params=True,
                                                  return_chain_params=True, return_erase_params=True)
        want_c = np.stack(D.draw_params(seed, epoch, index, pad), axis=1)
        want_ch = D.draw_chain_params(seed, epoch, index, kw["policy"], kw.get("policy_ops", 2), kw.get("policy_magnitude", 9))
        want_e = np.stack(D.draw_policy_params(seed, epoch, index, H, W, erase_prob=0.5)[3:], axis=1)
        assert torch.equal(cused.cpu().long(), torch.from_numpy(want_c))
        assert chused.dtype == torch.int32 and torch.equal(chused.cpu().long(), torch.from_numpy(want_ch))
        assert eused.dtype == torch.int32 and torch.equal(eused.cpu().long(), torch.from_numpy(want_e))
        want = restate(x, index.tolist(), want_c.tolist(), want_ch.tolist(), want_e.tolist(), table, pad)
        assert bits_equal(img, want) and torch.equal(tgt.cpu(), y[index])
    if B == 512 and kw["policy"] == "ra":
        assert len(set(want_ch[:, 0, 0].tolist())) == 14 and 0.3 < float(np.mean(want_e[:, 2] > 0)) < 0.7
    if kw["policy"] is USER:             # p = 1 always, p = 0 never
        assert set(map(tuple, want_ch[:, :, 0].tolist())) <= {(5, 0, 0, 0), (0, 11, 7, 0)}
    img2, _ = ds.batch(index.cuda(), epoch=199, seed=5)          # a device index takes the same path
    assert bits_equal(img2, img)


def test_crop_and_erase_are_those_of_the_ta_wide_path():
    rng = np.random.default_rng(12)
    x = rng.integers(0, 256, (97, 3, 32, 32), dtype=np.uint8)
    index = torch.from_numpy(rng.integers(0, 97, 300))
    ta, _ = dataset(x, 4, policy="ta_wide", erase_prob=0.5)
    _, _, cta, pta = ta.batch(index, epoch=7, seed=3, return_params=True, return_policy_params=True)
    for kw in (dict(policy="ra"), dict(policy="ra", policy_ops=4, policy_magnitude=30), dict(policy="cifar10")):
        ds, _ = dataset(x, 4, erase_prob=0.5, **kw)
        _, _, c, e = ds.batch(index, epoch=7, seed=3, return_params=True, return_erase_params=True)
        assert torch.equal(c, cta) and torch.equal(e, pta[:, 3:]) and bool((e[:, 2] > 0).any())
    # evaluation never applies a policy: the plain launch and its bits
    plain, _ = dataset(x, 4)
    assert bits_equal(ds.batch(index, train=False)[0], plain.batch(index, train=False)[0])
    assert not ds.batch(index, train=False, return_chain_params=True)[2].any()


def test_a_shard_and_indices_outside_it():
    rng = np.random.default_rng(4)
    x = rng.integers(0, 256, (101, 3, 32, 32), dtype=np.uint8)
    kw = dict(policy="cifar10", erase_prob=0.5)
    whole, _ = dataset(x, 4, **kw)
    part, _ = dataset(x, 4, shard=(1, 3), **kw)
    lo, hi = D.shard_range(101, 1, 3)
    assert tuple(part.shard_range) == (lo, hi) == (33, 67) and len(part) == 34
    index = torch.from_numpy(rng.integers(lo, hi, 200))
    ret = dict(return_params=True, return_chain_params=True, return_erase_params=True)
    a = whole.batch(index, epoch=7, seed=1, **ret)
    b = part.batch(index, epoch=7, seed=1, **ret)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert bits_equal(a[0], b[0]) and bool(a[3].any())
    with pytest.raises(ValueError, match="shard owns"):
        part.batch(torch.tensor([lo - 1]))
    # a device index outside the shard, or outside the dataset: a zero image, label -1, zero params
    img, tgt, cu, ch, er = part.batch(torch.tensor([lo, lo - 1, hi, hi - 1], device="cuda"), **ret)
    assert tgt.tolist()[1:3] == [-1, -1] and tgt.tolist()[0] >= 0 and tgt.tolist()[3] >= 0
    assert not img[1:3].any() and not cu[1:3].any() and not ch[1:3].any() and not er[1:3].any()
    assert bool(img[0].any()) and bool(img[3].any())
    ra, y = dataset(x, 4, policy="ra", policy_ops=4, erase_prob=1.0)
    index = torch.tensor([3, 101, -1, 2 ** 40, -2 ** 62, 100, 2 ** 63 - 1], device="cuda")
    img, tgt, cu, ch, er = ra.batch(index, **ret)
    assert tgt.tolist() == [int(y[3]), -1, -1, -1, -1, int(y[100]), -1]
    for j in (1, 2, 3, 4, 6):
        assert not img[j].any() and not cu[j].any() and not ch[j].any() and not er[j].any()
    assert bits_equal(img[[0, 5]], ra.batch(torch.tensor([3, 100]))[0])
    with pytest.raises(IndexError):
        ra.batch(torch.tensor([3, 101]))


@pytest.mark.parametrize("policy,n", [("ra", 31), ("cifar10", 10)])
def test_device_chain_params_are_clamped_not_trusted(policy, n):
    """chain_params and erase_params on the device cannot be checked on the host: the kernel clamps them, reports what it
    used, and the image is the reference's on the clamped values."""
    rng = np.random.default_rng(6)
    x = rng.integers(0, 256, (8, 3, 32, 32), dtype=np.uint8)
    ds, _ = dataset(x, 4, policy=policy)
    big, small = 2 ** 31 - 1, -2 ** 31
    wild = torch.tensor([[(99, -5, 2 ** 30), (13, 99, -1), (-3, 5, 0), (15, n, 7)],
                         [(big, big, big), (small, small, small), (14, small, 1), (8, big, small)],
                         [(5, 3, 0), (0, 0, 0), (16, 0, 0), (9, n - 1, 1)]], dtype=torch.int32)
    rect = torch.tensor([(-5, -5, 99, 99), (40, 40, 5, 5), (big, small, big, small)], dtype=torch.int32)
    crop = centre(3, 4)
    img, _, used, eused = ds.batch(torch.arange(3), params=crop, chain_params=wild.cuda(), erase_params=rect.cuda(),
                                   return_chain_params=True, return_erase_params=True)
    assert used.tolist() == [[[14, 0, 1], [13, n - 1, 1], [0, 5, 0], [14, n - 1, 1]],
                             [[14, n - 1, 1], [0, 0, 1], [14, 0, 1], [8, n - 1, 1]],
                             [[5, 3, 0], [0, 0, 0], [14, 0, 0], [9, n - 1, 1]]]
    assert eused.tolist() == [[0, 0, 32, 32], [31, 31, 1, 1], [0, 0, 0, 0]]
    want = restate(x, range(3), crop.tolist(), used.tolist(), eused.tolist(), D.chain_table(policy, 32, 32), 4)
    assert bits_equal(img, want) and not img[0].any()
    # the same values on the host are refused before any launch
    for bad in (wild, wild.clamp(0, 14), torch.zeros(3, 3, 3, dtype=torch.int32), torch.zeros(3, K, 3)):
        with pytest.raises(ValueError, match="chain_params"):
            ds.batch(torch.arange(3), chain_params=bad)
    for bad in (rect, torch.tensor([(0, 0, 33, 1)] * 3), torch.zeros(3, 5, dtype=torch.int32)):
        with pytest.raises(ValueError, match="erase_params"):
            ds.batch(torch.arange(3), erase_params=bad)
    plain, _ = dataset(x, 4, policy="ta_wide")
    with pytest.raises(ValueError, match="chain_params"):
        plain.batch(torch.arange(3), chain_params=torch.zeros(3, K, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="policy_params"):
        ds.batch(torch.arange(3), policy_params=torch.zeros(3, 7, dtype=torch.int32))


@pytest.mark.parametrize("kw", [dict(policy="ra", policy_ops=4, policy_magnitude=20), dict(policy="cifar10")], ids=["ra", "cifar10"])
def test_a_batch_is_the_concatenation_of_its_halves_and_repeats_to_the_bit(kw):
    rng = np.random.default_rng(7)
    x = rng.integers(0, 256, (307, 3, 32, 32), dtype=np.uint8)
    ds, _ = dataset(x, 4, erase_prob=0.25, **kw)
    a, b = torch.from_numpy(rng.integers(0, 307, 100)), torch.from_numpy(rng.integers(0, 307, 28))
    ret = dict(epoch=3, seed=9, return_params=True, return_chain_params=True, return_erase_params=True)
    whole, pa, pb = ds.batch(torch.cat([a, b]), **ret), ds.batch(a, **ret), ds.batch(b, **ret)
    for w, u, v in zip(whole, pa, pb):
        assert torch.equal(w, torch.cat([u, v]))
    assert bits_equal(whole[0], torch.cat([pa[0], pb[0]]))
    again = ds.batch(torch.cat([a, b]), **ret)
    assert bits_equal(whole[0], again[0]) and whole[0].data_ptr() != again[0].data_ptr()      # the launch repeats to the bit
    other = ds.batch(torch.cat([a, b]), epoch=4, seed=9, return_chain_params=True)
    assert not torch.equal(other[2], whole[3])                  # the epoch is part of the draw


def test_the_c_entry_refuses_float_and_large_sources_by_itself():
    from nbdt import ops
    y = torch.zeros(4, dtype=torch.long)
    for bad in (torch.zeros(4, 3, 32, 32), torch.zeros(4, 3, 129, 128, dtype=torch.uint8)):
        for policy in ("ra", "cifar10"):
            with pytest.raises(ValueError, match="uint8 dataset|at most 49152"):
                D.DeviceDataset(bad, y, CIFAR["mean"], CIFAR["std"], 4, policy=policy)
    table = torch.from_numpy(D.chain_table("ra", 32, 32).copy()).cuda()
    out, lab = torch.empty(4, 3, 32, 32, device="cuda"), torch.empty(4, dtype=torch.int64, device="cuda")
    with pytest.raises(_C.NBDTHipError, match="uint8"):
        ops.policy_chain_batch(torch.zeros(4, 3, 32, 32).cuda(), y.cuda(), torch.arange(4).cuda(), out, lab, 4, True,
                               CIFAR["mean"], CIFAR["std"], table, 31, num_ops=2, magnitude=9)
    with pytest.raises(_C.NBDTHipError, match="49152"):
        ops.policy_chain_batch(torch.zeros(4, 3, 129, 128, dtype=torch.uint8).cuda(), y.cuda(), torch.arange(4).cuda(),
                               torch.empty(4, 3, 129, 128, device="cuda"), lab, 4, True, CIFAR["mean"], CIFAR["std"], table,
                               31, num_ops=2, magnitude=9)


def test_the_largest_image_the_kernel_takes():
    """128 x 128: both tiles fill 96 KB of LDS, past the 64 KB that needs no attribute."""
    x = fixtures(128, 128)[:2]
    ds, _ = dataset(x, 4, policy="ra")
    chains = [[(5, 30, 0), (13, 0, 0), (9, 25, 1), (12, 0, 0)], [(13, 0, 0), (13, 0, 0), (2, 30, 1), (8, 30, 0)]]
    img, _, want = launch(ds, x, [0, 1], chains, 4)
    assert bits_equal(img, want)


@pytest.mark.parametrize("kw", [dict(policy="ra"), dict(policy="cifar10")], ids=["ra", "cifar10"])
def test_an_engine_trains_on_chain_batches_and_repeats_to_the_bit(kw):
    import torch.nn as nn
    from nbdt import ops
    from nbdt.engine import WRNEngine, train_step
    from nbdt.loss import SoftTreeSupLoss
    rng = np.random.default_rng(8)
    x = rng.integers(0, 256, (64, 3, 32, 32), dtype=np.uint8)
    ds, _ = dataset(x, 4, erase_prob=0.25, device="cuda:0", **kw)
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


@pytest.mark.parametrize("flags,word", [("--auto-augment ra --ra-num-ops 3 --ra-magnitude 12",
                                         "ra: RandAugment, 3 operations at magnitude 12"),
                                        ("--auto-augment cifar10", "cifar10: AutoAugment, 25 sub-policies")], ids=["ra", "cifar10"])
def test_main_trains_with_a_policy_chain(tmp_path, monkeypatch, capsys, flags, word):
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
    calls = {"chain": 0, "single": 0, "plain": 0}
    chain_batch, policy_batch, augment_batch = ops.policy_chain_batch, ops.policy_batch, ops.augment_batch

    def count(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped
    monkeypatch.setattr(ops, "policy_chain_batch", count("chain", chain_batch))
    monkeypatch.setattr(ops, "policy_batch", count("single", policy_batch))
    monkeypatch.setattr(ops, "augment_batch", count("plain", augment_batch))
    acc, _ = M.main(("--arch ResNet18 --dataset CIFAR10 --batch-size 64 --data-file data.pt --lr 0.05 --epochs 1 "
                     "--augment reference --random-erase 0.25 " + flags).split())
    assert 0.0 <= acc <= 100.0 and math.isfinite(acc)
    assert calls == {"chain": 2, "single": 0, "plain": calls["plain"]} and calls["plain"] >= 1     # evaluation stays plain
    out = capsys.readouterr().out
    assert word in out                                                      # the log names the policy
    losses = [float(v) for v in re.findall(r"Loss: (\S+) \(2 steps", out)]   # the epoch's mean training loss
    assert len(losses) == 1 and math.isfinite(losses[0]), out
