"""Device-resident datasets: the reference's training transform as one HIP launch per step.

The reference builds every training batch through ``RandomCrop(size, padding) -> RandomHorizontalFlip -> ToTensor ->
Normalize`` in DataLoader workers (nbdt/data/cifar.py:11-21, nbdt/data/imagenet.py:37-48).  Here the whole dataset sits in
device memory (CIFAR as uint8 is 150 MB, TinyImagenet200 1.2 GB) and ``nbdt_augment_batch`` (csrc/augment.hip) gathers a
batch by index, crops, flips, scales and normalises it into the fp32 NCHW tensor the engines take.  No CPU fallback:
``draw_params`` is the only part that runs without a GPU, and it computes no pixel.
"""
import numpy as np
import torch

from nbdt import _C, ops

# mean, std, pad of the reference's transform_train (nbdt/data/cifar.py:14-19, nbdt/data/imagenet.py:41-46)
DATASET_STATS = {
    "CIFAR10": {"mean": (0.4914, 0.4822, 0.4465), "std": (0.2023, 0.1994, 0.2010), "pad": 4},
    "CIFAR100": {"mean": (0.4914, 0.4822, 0.4465), "std": (0.2023, 0.1994, 0.2010), "pad": 4},
    "TinyImagenet200": {"mean": (0.4802, 0.4481, 0.3975), "std": (0.2302, 0.2265, 0.2262), "pad": 8},
}

MAX_PAD = _C.NBDT_AUGMENT_MAX_PAD
_M64 = (1 << 64) - 1


def _mix64(x):
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def draw_params(seed, epoch, index, pad):
    """The generator of nbdt_augment_batch (include/nbdt_hip.h), restated with numpy: (dy, dx, flip) int64 arrays shaped
    like `index`.  A pure function of (seed, epoch, dataset index, pad): not of the position in the batch, the batch size
    or the rank.  dy, dx in [0, 2*pad], flip in {0, 1}."""
    if not 0 <= int(pad) <= MAX_PAD:
        raise ValueError(f"pad must be 0..{MAX_PAD}, got {pad}")
    if isinstance(index, torch.Tensor):
        index = index.cpu().numpy()
    idx = np.asarray(index).astype(np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        key = _mix64(np.asarray([(int(seed) * 0x9E3779B97F4A7C15 + int(epoch)) & _M64], dtype=np.uint64))[0]
        r = _mix64(key ^ (idx * np.uint64(0xD1342543DE82EF95)))
    span = np.uint64(2 * int(pad) + 1)
    m24 = np.uint64(0xFFFFFF)
    dy = ((r & m24) * span) >> np.uint64(24)
    dx = (((r >> np.uint64(24)) & m24) * span) >> np.uint64(24)
    flip = r >> np.uint64(63)
    return dy.astype(np.int64), dx.astype(np.int64), flip.astype(np.int64)


class DeviceDataset:
    """A dataset held on the device, batched by `nbdt_augment_batch`.

    x: uint8 or fp32 ``[N,3,H,W]``; y: integer ``[N]``; both are moved to `device` once.  A uint8 `x` is scaled by 1/255
    and normalised with `mean` / `std` in the kernel, its padding is byte 0 before conversion (so a padded pixel is
    ``(0 - mean)/std``).  An fp32 `x` is taken as already normalised and copied; its padded pixels get `fill`, by default
    ``(0 - mean)/std`` -- a file normalised with the dataset's statistics then yields the same batches as its uint8
    original.  pad: pixels of zero padding before the random ``H x W`` crop; flip: random horizontal flip.
    """

    def __init__(self, x, y, mean, std, pad, flip=True, fill=None, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise _C.NBDTHipError(f"DeviceDataset lives on an MI355X, not on {device} (no CPU fallback)")
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"x must be uint8 or fp32 [N,3,H,W], got {x.dtype} {tuple(x.shape)}")
        if y.dim() != 1 or y.shape[0] != x.shape[0] or y.is_floating_point():
            raise ValueError(f"y must be integer [N] with N = {x.shape[0]}, got {y.dtype} {tuple(y.shape)}")
        if not 0 <= int(pad) <= MAX_PAD:
            raise ValueError(f"pad must be 0..{MAX_PAD}, got {pad}")
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("mean and std have one entry per channel (3)")
        self.mean = tuple(float(m) for m in mean)
        self.std = tuple(float(s) for s in std)
        if fill is None:       # (0 - mean) / std in fp32, the kernel's value of a padded uint8 pixel
            fill = ((torch.zeros(3) - torch.tensor(self.mean)) / torch.tensor(self.std)).tolist()
        self.fill = tuple(float(f) for f in fill)
        self.pad, self.flip = int(pad), bool(flip)
        self.x = x.to(device).contiguous()
        self.y = y.to(device=device, dtype=torch.int64).contiguous()
        self.device = self.x.device

    def __len__(self):
        return self.x.shape[0]

    @property
    def shape(self):
        return self.x.shape

    def batch(self, index, epoch=0, seed=0, train=True, params=None, return_params=False):
        """(img fp32 [B,3,H,W], targets int64 [B][, params int8 [B,3]]) for the samples `index`, in ONE launch on torch's
        current stream.

        index: a host sequence / array / CPU tensor is range-checked (IndexError) and copied; a device tensor goes straight
        to the kernel, which writes a zero image with target -1 for an index outside [0, N).  train=False is the evaluation
        transform (no crop, no flip).  params: int8 [B,3] of (dy, dx, flip) replaces the generator; a CPU tensor is
        range-checked and copied.  Without it the draw is ``draw_params(seed, epoch, index, pad)``.

        Every call returns freshly allocated tensors (torch's caching allocator): train_step is asynchronous and the engine
        keeps `img` until the stem's weight gradient, so nothing handed out is ever overwritten by a later call."""
        n = len(self)
        if not isinstance(index, torch.Tensor):
            index = torch.as_tensor(np.asarray(index))
        if index.dim() != 1 or index.is_floating_point() or index.shape[0] == 0:
            raise ValueError(f"index must be a non-empty integer vector, got {index.dtype} {tuple(index.shape)}")
        if not index.is_cuda:
            if int(index.min()) < 0 or int(index.max()) >= n:
                raise IndexError(f"index outside [0, {n}): min {int(index.min())}, max {int(index.max())}")
            index = index.to(self.device, non_blocking=True)
        _C.require_gpu(index, "DeviceDataset.batch")
        index = index.to(dtype=torch.int64).contiguous()
        pad, flip = (self.pad, self.flip) if train else (0, False)
        B = index.shape[0]
        if params is not None:
            if not train:
                raise ValueError("params replace the training draw; train=False has none")
            if tuple(params.shape) != (B, 3) or params.dtype != torch.int8:
                raise ValueError(f"params must be int8 [{B},3], got {params.dtype} {tuple(params.shape)}")
            if not params.is_cuda:
                lo, hi = params.min(dim=0).values, params.max(dim=0).values
                if int(lo.min()) < 0 or int(hi[0]) > 2 * pad or int(hi[1]) > 2 * pad or int(hi[2]) > 1:
                    raise ValueError(f"params outside dy, dx in [0, {2 * pad}], flip in {{0, 1}}")
                params = params.to(self.device, non_blocking=True)
            _C.require_gpu(params, "DeviceDataset.batch")
            params = params.contiguous()
        img = torch.empty((B,) + tuple(self.x.shape[1:]), dtype=torch.float32, device=self.device)
        targets = torch.empty((B,), dtype=torch.int64, device=self.device)
        used = torch.empty((B, 3), dtype=torch.int8, device=self.device) if return_params else None
        ops.augment_batch(self.x, self.y, index, img, targets, pad, flip, mean=self.mean, std=self.std, fill=self.fill,
                          seed=seed, epoch=epoch, params_in=params, params_out=used)
        return (img, targets, used) if return_params else (img, targets)
