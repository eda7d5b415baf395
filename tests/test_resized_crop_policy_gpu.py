"""nbdt_resized_crop_policy_batch / nbdt.data.ResizedCropDataset(policy=, erase_prob=) on the MI355X against
nbdt.data.resized_crop_policy_reference: PIL's crop-and-resize, the flip, Pillow's rules per operation (both checked against
Pillow in tests/test_resample.py, tests/test_policy_chain.py and tests/test_resized_crop_policy.py),
.float().div(255).sub(mean).div(std), the erase rectangle set to 0.0.  Every comparison is of the fp32 bit patterns
(np.array_equal on the int32 view): nothing is rounded or reordered, so there is no tolerance."""
import numpy as np
import pytest
import torch

from nbdt import data as D

pytestmark = pytest.mark.gpu

STATS = D.RESIZED_CROP_STATS["Imagenet1000"]
MEAN, STD = STATS["mean"], STATS["std"]
K = D.CHAIN_MAX_OPS
RET = dict(return_params=True, return_chain_params=True, return_erase_params=True)


def images(n, H, W, seed=0):
    """A smooth ramp plus seeded noise per image (AutoContrast and Equalize have work to do), one of them constant."""
    rng = np.random.default_rng(1000 * H + W + seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, 3, H, W), dtype=np.uint8)
    for i in range(n):
        ramp = np.stack([30 + 170 * x / W + 5 * i, 210 - 150 * y / H, 50 + 140 * (x + y) / (H + W)])
        out[i] = np.clip(np.rint(ramp) + rng.integers(-12, 13, ramp.shape), 20, 235)
    out[n - 1, 0], out[n - 1, 1], out[n - 1, 2] = 7, 128, 255
    return out


def dataset(x_u8, size, **kw):
    x = torch.from_numpy(x_u8)
    y = (torch.arange(x.shape[0]) * 7) % 1000
    return D.ResizedCropDataset(x, y, MEAN, STD, size=size, **kw), y


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def restate(x_u8, index, boxes, chains, erase, table, size):
    """The reference for samples `index` under boxes = [(top, left, h, w, flip)], chains = [[(op, bin, sign)] * 4] and
    erase = [(top, left, h, w)]: fp32 [B,3,size,size]."""
    return torch.stack([D.resized_crop_policy_reference(x_u8[i], b[:4], b[4], size, c, table, e, MEAN, STD)
                        for i, b, c, e in zip(index, boxes, chains, erase)])


def differing(img, want, labels):
    bad = (bits(img) != bits(want)).reshape(len(labels), -1).any(1).nonzero()[0].tolist()
    return f"{len(bad)} samples differ, first: {[labels[j] for j in bad[:8]]}"


def random_boxes(rng, B, H, W):
    top, left = rng.integers(0, H, B), rng.integers(0, W, B)
    return np.stack([top, left, rng.integers(1, H - top + 1), rng.integers(1, W - left + 1), rng.integers(0, 2, B)], axis=1)


def random_rects(rng, B, S):
    top, left = rng.integers(0, S, B), rng.integers(0, S, B)
    rect = np.stack([top, left, rng.integers(0, S - top + 1), rng.integers(0, S - left + 1)], axis=1)
    rect[(rect[:, 2] == 0) | (rect[:, 3] == 0)] = 0
    return rect


def launch(ds, x, index, boxes, chains, rects, table):
    """One batch with everything given, the parameters it reports, and its restatement."""
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32)
    img, tgt, used, cused, eused = ds.batch(torch.as_tensor(index), params=i32(boxes), chain_params=i32(chains),
                                            erase_params=i32(rects), **RET)
    assert np.array_equal(used.cpu().numpy(), boxes) and np.array_equal(cused.cpu().numpy(), chains)
    assert np.array_equal(eused.cpu().numpy(), rects)
    return img, tgt, restate(x, index, np.asarray(boxes).tolist(), np.asarray(chains).tolist(),
                             np.asarray(rects).tolist(), table, ds.size)


def test_every_operation_and_sign_at_22_on_the_scalar_store_path():
    """40 x 36 -> 22, B = 30: S % 4 != 0 and 3 * S * S % 16 != 0, so bytes and floats are stored one by one.  All 15
    operations under both signs, the operation in slot j % 4, given boxes (the whole image and a 1 x 1 box among them) and
    given erase rectangles."""
    H, W, S = 40, 36, 22
    assert S % 4 and (3 * S * S) % 16
    rng = np.random.default_rng(22)
    x = images(6, H, W)
    ds, y = dataset(x, S, policy="ra")
    combos = [(op, sg) for op in range(15) for sg in (0, 1)]
    chains = np.zeros((30, K, 3), dtype=np.int64)
    for j, (op, sg) in enumerate(combos):
        chains[j, j % K] = (op, rng.integers(1, 31), sg)
    index = rng.integers(0, 6, 30)
    boxes = random_boxes(rng, 30, H, W)
    boxes[0], boxes[1], boxes[2] = (0, 0, H, W, 0), (17, 5, 1, 1, 1), (0, 0, H, W, 1)
    rects = random_rects(rng, 30, S)
    rects[::3] = 0
    img, tgt, want = launch(ds, x, index, boxes, chains, rects, D.chain_table("ra", S, S))
    assert torch.equal(tgt.cpu(), y[index])
    assert np.array_equal(bits(img), bits(want)), differing(img, want, combos)


def test_randaugment_drawn_at_24_on_the_vector_path():
    """48 x 40 -> 24, B = 32: policy="ra" with four operations, everything drawn.  The parameters returned are those of
    draw_resized_crop_params, draw_chain_params and draw_policy_params(H = W = 24), the image is the reference under them,
    and a second call returns the same bits."""
    H, W, S, n = 48, 40, 24, 13
    rng = np.random.default_rng(24)
    x = images(n, H, W)
    ds, y = dataset(x, S, policy="ra", policy_ops=4, policy_magnitude=17, erase_prob=0.5)
    index = torch.from_numpy(rng.integers(0, n, 32))
    index[1] = index[0]
    table = D.chain_table("ra", S, S)
    for seed, epoch in ((0, 0), (5, 199)):
        img, tgt, used, cused, eused = ds.batch(index, epoch=epoch, seed=seed, **RET)
        want_b = np.stack(D.draw_resized_crop_params(seed, epoch, index, H, W, STATS["scale"], STATS["ratio"]), axis=1)
        want_c = D.draw_chain_params(seed, epoch, index, "ra", 4, 17)
        want_e = np.stack(D.draw_policy_params(seed, epoch, index, S, S, erase_prob=0.5)[3:], axis=1)
        assert used.dtype == torch.int32 and np.array_equal(used.cpu().numpy(), want_b)
        assert cused.dtype == torch.int32 and np.array_equal(cused.cpu().numpy(), want_c)
        assert eused.dtype == torch.int32 and np.array_equal(eused.cpu().numpy(), want_e)
        want = restate(x, index.tolist(), want_b.tolist(), want_c.tolist(), want_e.tolist(), table, S)
        assert np.array_equal(bits(img), bits(want)), differing(img, want, want_c.tolist())
        assert torch.equal(tgt.cpu(), y[index])
    assert (want_c[:, :, 0] != 0).all(axis=1).any() and 0 < int((want_e[:, 2] > 0).sum()) < 32
    again = ds.batch(index.cuda(), epoch=199, seed=5)[0]           # a device index takes the same path
    assert np.array_equal(bits(again), bits(img)) and again.data_ptr() != img.data_ptr()


def test_every_operation_and_two_chains_at_144_where_lds_tiles_would_not_fit():
    """160 x 176 -> 144 (62208 bytes per tile, past the 49152 of the padded-crop kernels), 24 samples in batches of 8: all
    15 single operations, the two four-slot chains of the golden under both tables' bins, and chains that collect
    statistics twice."""
    H, W, S = 160, 176, 144
    assert 3 * S * S > D.POLICY_MAX_BYTES
    rng = np.random.default_rng(144)
    x = images(4, H, W)
    ds, _ = dataset(x, S, policy="ra")
    op = D.CHAIN_OPS.index
    chains = np.zeros((24, K, 3), dtype=np.int64)
    for j in range(15):
        chains[j, (j + 1) % K] = (j, 30 if j % 2 else 21, j % 3 == 0)
    chains[15, :3] = [(op("Rotate"), 20, 1), (op("Equalize"), 0, 0), (op("Color"), 20, 0)]
    chains[16] = [(op("ShearX"), 20, 0), (op("Contrast"), 20, 1), (op("Sharpness"), 20, 0), (op("AutoContrast"), 0, 0)]
    chains[17] = [(op("Equalize"), 0, 0), (op("Equalize"), 0, 0), (op("Contrast"), 30, 0), (op("Contrast"), 30, 1)]
    chains[18] = [(op("TranslateX"), 30, 1), (op("AutoContrast"), 0, 0), (op("ShearY"), 30, 0), (op("Equalize"), 0, 0)]
    chains[19] = [(op("Sharpness"), 30, 0), (0, 0, 0), (op("Sharpness"), 30, 1), (op("Invert"), 0, 0)]
    for j in range(20, 24):
        chains[j] = np.stack([rng.integers(1, 15, K), rng.integers(0, 31, K), rng.integers(0, 2, K)], axis=1)
    index = rng.integers(0, 4, 24)
    boxes = random_boxes(rng, 24, H, W)
    boxes[:4] = [(0, 0, H, W, 0), (0, 0, H, W, 1), (3, 9, 150, 160, 1), (40, 30, 100, 144, 0)]
    boxes[15:19, 2:4] = np.maximum(boxes[15:19, 2:4], 60)
    boxes[15:19, :2] = np.minimum(boxes[15:19, :2], 90)
    rects = random_rects(rng, 24, S)
    rects[::2] = 0
    table = D.chain_table("ra", S, S)
    for lo in (0, 8, 16):
        sl = slice(lo, lo + 8)
        img, _, want = launch(ds, x, index[sl], boxes[sl], chains[sl], rects[sl], table)
        assert np.array_equal(bits(img), bits(want)), differing(img, want, chains[sl].tolist())


def test_the_imagenet_policy_with_erasing_at_224():
    """256 x 256 -> 224, B = 4: the real shape.  AutoAugment's ImageNet policy and erase_prob = 1, drawn; the image is
    compared under the parameters the launch returns, which are the host's restatement of the draw."""
    H = W = 256
    S = 224
    x = images(5, H, W)
    ds, y = dataset(x, S, policy="imagenet", erase_prob=1.0)
    index = torch.tensor([3, 0, 4, 1])
    img, tgt, used, cused, eused = ds.batch(index, epoch=2, seed=11, **RET)
    want_c, which = D.draw_chain_params(11, 2, index, "imagenet", return_subpolicy=True)
    assert np.array_equal(cused.cpu().numpy(), want_c) and bool(cused.any())
    assert np.array_equal(used.cpu().numpy(),
                          np.stack(D.draw_resized_crop_params(11, 2, index, H, W, STATS["scale"], STATS["ratio"]), axis=1))
    assert np.array_equal(eused.cpu().numpy(), np.stack(D.draw_policy_params(11, 2, index, S, S, erase_prob=1.0)[3:], axis=1))
    assert bool((eused[:, 2] > 0).all()) and torch.equal(tgt.cpu(), y[index])
    want = restate(x, index.tolist(), used.tolist(), cused.tolist(), eused.tolist(), D.chain_table("cifar10", S, S), S)
    assert tuple(img.shape) == (4, 3, S, S) and np.array_equal(bits(img), bits(want)), differing(img, want, want_c.tolist())
    for j, (t, l, h, w) in enumerate(eused.tolist()):
        assert not img[j, :, t:t + h, l:l + w].any()


def test_ta_wide_is_the_single_op_draw_in_slot_0():
    H, W, S, n = 48, 40, 24, 13
    x = images(n, H, W)
    ds, _ = dataset(x, S, policy="ta_wide", erase_prob=0.25)
    index = torch.arange(64) % n
    img, _, used, cused, eused = ds.batch(index, epoch=3, seed=2, **RET)
    op, b, sg, *rect = D.draw_policy_params(2, 3, index, S, S, erase_prob=0.25)
    assert np.array_equal(cused[:, 0].cpu().numpy(), np.stack([op, b, sg], axis=1)) and not cused[:, 1:].any()
    assert np.array_equal(eused.cpu().numpy(), np.stack(rect, axis=1))
    assert len(set(op[:n].tolist())) > 4 and int(b.max()) > 20
    want = restate(x, index.tolist(), used.tolist(), cused.tolist(), eused.tolist(), D.chain_table("ta_wide", S, S), S)
    assert np.array_equal(bits(img), bits(want)), differing(img, want, cused.tolist())


def test_without_a_policy_nothing_changes_and_evaluation_ignores_it():
    H, W, S, n = 48, 40, 24, 13
    x = images(n, H, W)
    index = torch.arange(40) % n
    old, _ = dataset(x, S)
    explicit, _ = dataset(x, S, policy=None, erase_prob=0.0)
    a = old.batch(index, epoch=4, seed=1, return_params=True)
    b = explicit.batch(index, epoch=4, seed=1, return_params=True)
    assert np.array_equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    plain = explicit.batch(index, epoch=4, seed=1, return_chain_params=True, return_erase_params=True)
    assert len(plain) == 4 and not plain[2].any() and not plain[3].any()
    # the box and the flip of a sample do not depend on the policy
    for kw in (dict(policy="ra"), dict(policy="imagenet", erase_prob=0.5), dict(policy="ta_wide"), dict(erase_prob=1.0)):
        ds, _ = dataset(x, S, **kw)
        got = ds.batch(index, epoch=4, seed=1, return_params=True)
        assert torch.equal(got[2], a[2]) and torch.equal(got[1], a[1]) and not np.array_equal(bits(got[0]), bits(a[0]))
        # train=False never applies a policy or an erase: the evaluation launch and its bits
        assert np.array_equal(bits(ds.batch(index, train=False)[0]), bits(old.batch(index, train=False)[0]))
        assert not ds.batch(index, train=False, return_chain_params=True)[2].any()
        with pytest.raises(ValueError, match="train=False"):
            ds.batch(index, train=False, erase_params=torch.zeros(40, 4, dtype=torch.int32))
    # the erase alone is the plain batch with the rectangle zeroed
    img, _, eused = ds.batch(index, epoch=4, seed=1, return_erase_params=True)
    want = a[0].clone()
    for j, (t, l, h, w) in enumerate(eused.tolist()):
        want[j, :, t:t + h, l:l + w] = 0.0
    assert np.array_equal(bits(img), bits(want)) and bool((eused[:, 2] > 0).any())
    with pytest.raises(ValueError, match="chain_params"):
        ds.batch(index, chain_params=torch.zeros(40, K, 3, dtype=torch.int32))


def test_a_shard_and_indices_outside_it():
    H, W, S, n = 48, 40, 24, 21
    rng = np.random.default_rng(7)
    x = images(n, H, W)
    kw = dict(policy="imagenet", erase_prob=0.5)
    whole, y = dataset(x, S, **kw)
    part, _ = dataset(x, S, shard=(1, 2), **kw)
    lo, hi = D.shard_range(n, 1, 2)
    assert tuple(part.shard_range) == (lo, hi) == (10, 21) and len(part) == 11
    index = torch.from_numpy(rng.integers(lo, hi, 48))
    a = whole.batch(index, epoch=7, seed=1, **RET)
    b = part.batch(index, epoch=7, seed=1, **RET)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert np.array_equal(bits(a[0]), bits(b[0])) and bool(a[3].any())
    with pytest.raises(ValueError, match="shard owns"):
        part.batch(torch.tensor([lo - 1]))
    # a device index outside the shard, or outside the dataset: a zero image, label -1, zero params
    img, tgt, used, cused, eused = part.batch(torch.tensor([lo, lo - 1, hi, hi - 1], device="cuda"), **RET)
    assert tgt.tolist()[1:3] == [-1, -1] and tgt.tolist()[0] >= 0 and tgt.tolist()[3] >= 0
    assert not img[1:3].any() and not used[1:3].any() and not cused[1:3].any() and not eused[1:3].any()
    assert bool(img[0].any()) and bool(img[3].any())
    index = torch.tensor([3, n, -1, 2 ** 40, -2 ** 62, n - 1, 2 ** 63 - 1], device="cuda")
    img, tgt, used, cused, eused = whole.batch(index, **RET)
    assert tgt.tolist() == [int(y[3]), -1, -1, -1, -1, int(y[n - 1]), -1]
    for j in (1, 2, 3, 4, 6):
        assert not img[j].any() and not used[j].any() and not cused[j].any() and not eused[j].any()
    assert np.array_equal(bits(img[[0, 5]]), bits(whole.batch(torch.tensor([3, n - 1]))[0]))
    with pytest.raises(IndexError):
        whole.batch(torch.tensor([3, n]))


@pytest.mark.parametrize("policy,n", [("ra", 31), ("imagenet", 10)])
def test_device_chain_params_are_clamped_not_trusted(policy, n):
    """chain_params and erase_params on the device cannot be checked on the host: the kernel clamps them as the header
    states, reports what it used, and the image is the reference's on the clamped values."""
    H, W, S = 48, 40, 24
    x = images(4, H, W)
    ds, _ = dataset(x, S, policy=policy)
    big, small = 2 ** 31 - 1, -2 ** 31
    wild = torch.tensor([[(99, -1, 2 ** 30), (13, 99, -1), (-3, 5, 0), (15, n, 7)],
                         [(big, big, big), (small, small, small), (14, small, 1), (8, big, small)],
                         [(5, 3, 0), (0, 0, 0), (16, 0, 0), (9, n - 1, 1)]], dtype=torch.int32)
    rect = torch.tensor([(-5, -5, 99, 99), (40, 40, 5, 5), (big, small, big, small)], dtype=torch.int32)
    boxes = torch.tensor([(0, 0, H, W, 0), (5, 5, 30, 30, 1), (10, 2, 20, 35, 0)], dtype=torch.int32)
    img, _, used, eused = ds.batch(torch.arange(3), params=boxes, chain_params=wild.cuda(), erase_params=rect.cuda(),
                                   return_chain_params=True, return_erase_params=True)
    assert used.tolist() == [[[14, 0, 1], [13, n - 1, 1], [0, 5, 0], [14, n - 1, 1]],
                             [[14, n - 1, 1], [0, 0, 1], [14, 0, 1], [8, n - 1, 1]],
                             [[5, 3, 0], [0, 0, 0], [14, 0, 0], [9, n - 1, 1]]]
    assert eused.tolist() == [[0, 0, S, S], [S - 1, S - 1, 1, 1], [0, 0, 0, 0]]
    table = D.chain_table("ra" if policy == "ra" else "cifar10", S, S)
    want = restate(x, range(3), boxes.tolist(), used.tolist(), eused.tolist(), table, S)
    assert np.array_equal(bits(img), bits(want)) and not img[0].any()
    # the same values on the host are refused before any launch
    for bad in (wild, wild.clamp(0, 14), torch.zeros(3, 3, 3, dtype=torch.int32), torch.zeros(3, K, 3)):
        with pytest.raises(ValueError, match="chain_params"):
            ds.batch(torch.arange(3), chain_params=bad)
    for bad in (rect, torch.tensor([(0, 0, S + 1, 1)] * 3), torch.zeros(3, 5, dtype=torch.int32)):
        with pytest.raises(ValueError, match="erase_params"):
            ds.batch(torch.arange(3), erase_params=bad)
