"""nbdt_resized_crop_batch / nbdt.data.ResizedCropDataset on the MI355X: the pixels against PIL's committed bytes and
against nbdt.data.resample_reference, normalised with torch on the CPU in the kernel's operation order (bit for bit); the
boxes the kernel draws against nbdt.data.draw_resized_crop_params (exactly); per-index purity; the guards."""
import os

import numpy as np
import pytest
import torch

import nbdt_path
from nbdt import _C, ops
from nbdt import data as D

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(nbdt_path.ROOT, "tests", "golden", "resized_crop_pil.npz")
MEAN, STD = D.RESIZED_CROP_STATS["Imagenet1000"]["mean"], D.RESIZED_CROP_STATS["Imagenet1000"]["std"]


def normalise(u8, flip=None):
    """[B,3,h,w] uint8 (numpy) -> what the kernel writes: flip, then (u / 255 - mean) / std, three fp32 operations on the
    CPU."""
    x = torch.from_numpy(np.ascontiguousarray(u8))
    if flip is not None:
        x = torch.where(torch.as_tensor(flip).bool().view(-1, 1, 1, 1), x.flip(3), x)
    return x.float().div(255.0).sub(torch.tensor(MEAN).view(1, 3, 1, 1)).div(torch.tensor(STD).view(1, 3, 1, 1))


def run(ds, index, resize, window, out_size, params):
    """The C entry through nbdt.ops with explicit geometry (the dataset class fixes a square output)."""
    B = len(index)
    index = torch.as_tensor(index, dtype=torch.int64).to(ds.device)
    img = torch.full((B, 3) + tuple(out_size), float("nan"), device=ds.device)
    tgt = torch.full((B,), -7, dtype=torch.int64, device=ds.device)
    used = torch.full((B, 5), -7, dtype=torch.int32, device=ds.device)
    ops.resized_crop_batch(ds.x, ds.y, index, img, tgt, resize, window, True, MEAN, STD, scale=ds.scale, ratio=ds.ratio,
                           ratio_table=ds._table, params_in=None if params is None else params.to(ds.device),
                           params_out=used)
    torch.cuda.synchronize()
    return img.cpu(), tgt.cpu(), used.cpu()


def dataset(x, size=32, **kw):
    x = torch.as_tensor(x)
    return D.ResizedCropDataset(x, torch.arange(100, 100 + x.shape[0]), MEAN, STD, size=size, **kw)


@pytest.mark.parametrize("name", ["a", "b"])
def test_given_boxes_equal_the_pil_goldens_bit_for_bit(name):
    """Every (image, box, size) of the fixture, unflipped and flipped; 27- and 5-wide outputs take the unvectorised store."""
    g = np.load(GOLDEN)
    imgs, boxes = g[f"img_{name}"], g[f"boxes_{name}"]
    ds = dataset(imgs)
    n, nb = len(imgs), len(boxes)
    index = np.repeat(np.arange(n), nb)
    for si, size in enumerate(g["sizes"]):
        size = tuple(int(v) for v in size)
        want_u8 = g[f"out_{name}_{si}"].reshape((n * nb, 3) + size)
        for flip in (0, 1, None):
            fl = np.arange(n * nb) % 2 if flip is None else np.full(n * nb, flip)
            params = torch.from_numpy(np.concatenate([np.tile(boxes, (n, 1)), fl[:, None]], axis=1).astype(np.int32))
            img, tgt, used = run(ds, index, size, (0, 0), size, params)
            assert torch.equal(img, normalise(want_u8, fl)), (name, size, flip)
            assert torch.equal(tgt, torch.from_numpy(100 + index)) and torch.equal(used, params)


@pytest.mark.parametrize("name", ["a", "b"])
def test_224_outputs_and_windows_of_them(name):
    g = np.load(GOLDEN)
    imgs = g[f"img_{name}"]
    ds = dataset(imgs)
    which, boxes, want = g[f"big_{name}_img"], g[f"big_{name}_boxes"], g[f"big_{name}_out"]
    index = np.repeat(which, len(boxes))
    params = torch.from_numpy(np.concatenate([np.tile(boxes, (len(which), 1)), np.zeros((len(index), 1))], axis=1).astype(np.int32))
    want = want.reshape((-1, 3, 224, 224))
    img, _, _ = run(ds, index, (224, 224), (0, 0), (224, 224), params)
    assert torch.equal(img, normalise(want))
    params[:, 4] = 1
    for top, left, h, w in ((0, 0, 224, 224), (16, 16, 192, 192), (3, 50, 100, 61), (223, 0, 1, 224), (200, 219, 24, 5)):
        img, _, _ = run(ds, index, (224, 224), (top, left), (h, w), params)
        assert torch.equal(img, normalise(want[:, :, top:top + h, left:left + w], np.ones(len(index)))), (top, left, h, w)


@pytest.mark.parametrize("name", ["a", "b"])
def test_evaluation_transform_equals_the_resize_center_crop_golden(name):
    g = np.load(GOLDEN)
    imgs = g[f"img_{name}"]
    ds = dataset(imgs, size=int(g["eval_size"]), resize=int(g["eval_resize"]))
    img, tgt = ds.batch(np.arange(len(imgs)), train=False)
    assert torch.equal(img.cpu(), normalise(g[f"eval_{name}"]))
    assert torch.equal(tgt.cpu(), torch.arange(100, 100 + len(imgs)))
    with pytest.raises(ValueError, match="train=False"):
        ds.batch([0], train=False, params=torch.zeros(1, 5, dtype=torch.int32))


@pytest.mark.parametrize("H,W,size", [(1024, 4096, 224), (512, 512, 224), (300, 1100, 64)])
def test_wide_sources_equal_the_numpy_restatement(H, W, size):
    """1024 x 4096 takes the kernel that stages nothing, for training and for evaluation; 512 x 512 and 300 x 1100 the LDS kernel with narrow bands."""
    rows = ops.resized_crop_band_rows(H, W, (size, size), (0, 0), (size, size))
    assert (rows == 0) == (W == 4096)
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (3, 3, H, W), dtype=np.uint8)
    ds = dataset(x, size=size)
    boxes = [(0, 0, H, W, 0), (H // 3, W // 5, H // 2, W // 2, 1), (H - 7, W - 200, 7, 200, 0), (1, 3, H - 2, 5, 1)]
    index = np.array([0, 1, 2, 1])
    params = torch.tensor(boxes, dtype=torch.int32)
    img, tgt, used = ds.batch(index, params=params, return_params=True)
    want = np.stack([D.resample_reference(x[i], b[:4], (size, size)) for i, b in zip(index, boxes)])
    assert torch.equal(img.cpu(), normalise(want, [b[4] for b in boxes]))
    assert torch.equal(used.cpu(), params) and torch.equal(tgt.cpu(), torch.from_numpy(100 + index))
    # the evaluation window of the same source
    assert (ops.resized_crop_band_rows(H, W, ds.eval_resize, ds.eval_window, (size, size)) == 0) == (W == 4096)
    img, _ = ds.batch(index, train=False)
    want = np.stack([D.resample_reference(x[i], (0, 0, H, W), ds.eval_resize, ds.eval_window + (size, size)) for i in index])
    assert torch.equal(img.cpu(), normalise(want))


@pytest.mark.parametrize("H,W", [(64, 64), (96, 80)])
def test_kernel_drawn_boxes_equal_the_numpy_restatement(H, W):
    n = 4096
    ds = dataset(torch.zeros(n, 3, H, W, dtype=torch.uint8), size=8)
    index = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    for seed, epoch in ((0, 0), (0, 1), (3, 199), (2 ** 40 + 5, 17)):
        _, _, used = ds.batch(index.to(ds.device), epoch=epoch, seed=seed, return_params=True)
        want = np.stack(D.draw_resized_crop_params(seed, epoch, index, H, W, ds.scale, ds.ratio), axis=1)
        assert np.array_equal(used.cpu().numpy().astype(np.int64), want), (H, W, seed, epoch)
    # other ranges, with the table that goes with them; a ratio range this image cannot hold exercises the fallback
    for scale, ratio in (((0.25, 0.5), (0.5, 2.0)), ((0.9, 1.0), (3.0, 4.0)), ((0.9, 1.0), (0.2, 0.25))):
        ds2 = dataset(torch.zeros(n, 3, H, W, dtype=torch.uint8), size=8, scale=scale, ratio=ratio)
        _, _, used = ds2.batch(index, epoch=4, seed=9, return_params=True)
        *want, which = D.draw_resized_crop_params(9, 4, index, H, W, scale, ratio, return_attempt=True)
        assert np.array_equal(used.cpu().numpy().astype(np.int64), np.stack(want, axis=1)), (scale, ratio)
        if ratio[0] >= 3.0 or ratio[1] <= 0.25:
            assert np.mean(which == _C.NBDT_RESIZED_CROP_ATTEMPTS) > 0.5


def test_training_batch_is_a_function_of_the_index_only_and_matches_its_own_boxes():
    rng = np.random.default_rng(11)
    x = rng.integers(0, 256, (40, 3, 96, 80), dtype=np.uint8)
    ds = dataset(x, size=48)
    index = torch.from_numpy(rng.integers(0, 40, 64))
    img, tgt, used = ds.batch(index, epoch=3, seed=5, return_params=True)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(0))
    img_p, tgt_p = ds.batch(index[perm].to(ds.device), epoch=3, seed=5)
    assert torch.equal(img_p, img[perm.to(ds.device)]) and torch.equal(tgt_p, tgt[perm.to(ds.device)])
    half, _ = ds.batch(index[:32], epoch=3, seed=5)
    assert torch.equal(half, img[:32])
    other, _ = ds.batch(index, epoch=4, seed=5)
    assert not torch.equal(other, img)
    # the pixels are the drawn boxes resampled: drawn and given boxes take the same path
    used = used.cpu()
    want = np.stack([D.resample_reference(x[i], b[:4], (48, 48)) for i, b in zip(index.tolist(), used.tolist())])
    assert torch.equal(img.cpu(), normalise(want, used[:, 4].numpy()))
    again, _ = ds.batch(index, params=used)
    assert torch.equal(again, img)
    assert img.data_ptr() != again.data_ptr()            # freshly allocated outputs


def test_guards():
    rng = np.random.default_rng(2)
    x = rng.integers(0, 256, (5, 3, 40, 56), dtype=np.uint8)
    ds = dataset(x, size=16)
    for bad in ([5], [-1], [0, 1, 99]):
        with pytest.raises(IndexError):
            ds.batch(bad)
    # a device index cannot be checked on the host: a zero image, target -1, zero params
    index = torch.tensor([0, 5, -1, 4, 2 ** 40], device=ds.device)
    img, tgt, used = ds.batch(index, return_params=True)
    assert tgt.tolist() == [100, -1, -1, 104, -1]
    for b in (1, 2, 4):
        assert torch.count_nonzero(img[b]) == 0 and used[b].tolist() == [0] * 5
    assert torch.isfinite(img).all() and torch.count_nonzero(img[0]) > 0
    # host params are range-checked ...
    for bad in ([0, 0, 41, 56, 0], [-1, 0, 4, 4, 0], [0, 53, 4, 4, 0], [0, 0, 0, 4, 0], [0, 0, 4, 4, 2]):
        with pytest.raises(ValueError, match="params"):
            ds.batch([0], params=torch.tensor([bad], dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        ds.batch([0], params=torch.zeros(1, 5, dtype=torch.int64))
    # ... device params are clamped into the image by the kernel: the result is the clamped box resampled
    hostile = [[-5, -9, 1000, 1000, 7], [39, 55, 2 ** 30, 2 ** 30, 0], [1000, 1000, 3, 3, -1], [10, 20, 0, -4, 0],
               [-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 1]]
    clamped = [[0, 0, 40, 56, 1], [39, 55, 1, 1, 0], [39, 55, 1, 1, 1], [10, 20, 1, 1, 0], [0, 55, 1, 1, 1]]
    index = np.array([0, 1, 2, 3, 4])
    img, _, used = ds.batch(index, params=torch.tensor(hostile, dtype=torch.int32).to(ds.device), return_params=True)
    assert used.tolist() == clamped
    want = np.stack([D.resample_reference(x[i], b[:4], (16, 16)) for i, b in zip(index, clamped)])
    assert torch.equal(img.cpu(), normalise(want, [b[4] for b in clamped]))
    # fp32 sources are refused, by the class and by the entry
    with pytest.raises(ValueError, match="uint8"):
        D.ResizedCropDataset(torch.zeros(2, 3, 8, 8), torch.zeros(2, dtype=torch.long), MEAN, STD, size=8)
    xf = torch.zeros(2, 3, 8, 8, device=ds.device)
    with pytest.raises(_C.NBDTHipError, match="uint8"):
        ops.resized_crop_batch(xf, ds.y, torch.zeros(1, dtype=torch.long, device=ds.device),
                               torch.empty(1, 3, 8, 8, device=ds.device), torch.empty(1, dtype=torch.long, device=ds.device),
                               (8, 8), (0, 0), False, MEAN, STD, params_in=torch.zeros(1, 5, dtype=torch.int32, device=ds.device))


def test_unaligned_dataset_views_take_the_checked_byte_path():
    """A dataset whose storage does not start on a 16-byte boundary, and whose first and last rows sit at the ends of the
    allocation's used range: the staging loop's whole-chunk loads stay inside [src, src + N*3*H*W), the rest goes byte
    by byte."""
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, (2, 3, 33, 47), dtype=np.uint8)
    ds = dataset(x, size=24)
    flat = torch.empty(x.size + 64, dtype=torch.uint8, device=ds.device)
    for off in (1, 7, 16, 37):
        view = flat[off:off + x.size].view(2, 3, 33, 47)
        view.copy_(torch.from_numpy(x))
        ds.x = view
        boxes = [(0, 0, 33, 47, 0), (30, 40, 3, 7, 1), (0, 0, 2, 3, 0), (31, 0, 2, 47, 1)]
        index = np.array([0, 1, 0, 1])
        img, _ = ds.batch(index, params=torch.tensor(boxes, dtype=torch.int32))
        want = np.stack([D.resample_reference(x[i], b[:4], (24, 24)) for i, b in zip(index, boxes)])
        assert torch.equal(img.cpu(), normalise(want, [b[4] for b in boxes])), off
