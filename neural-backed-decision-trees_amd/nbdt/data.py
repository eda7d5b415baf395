"""Device-resident datasets: the reference's training transforms as one HIP launch per step.

The reference builds every training batch through ``RandomCrop(size, padding) -> RandomHorizontalFlip -> ToTensor ->
Normalize`` in DataLoader workers (nbdt/data/cifar.py:11-21, nbdt/data/imagenet.py:37-48).  Here the whole dataset sits in
device memory (CIFAR as uint8 is 150 MB, TinyImagenet200 1.2 GB) and ``nbdt_augment_batch`` (csrc/augment.hip) gathers a
batch by index, crops, flips, scales and normalises it into the fp32 NCHW tensor the engines take.  No CPU fallback:
``draw_params`` is the only part that runs without a GPU, and it computes no pixel.

ImageNet trains with a different family (nbdt/data/imagenet.py:152-172): ``RandomResizedCrop(224) -> RandomHorizontalFlip
-> ToTensor -> Normalize``, evaluated with ``Resize(256) -> CenterCrop(224)``.  ``ResizedCropDataset`` is its device-side
form, ``nbdt_resized_crop_batch`` (csrc/resample.hip): the crop box is drawn in the kernel (``draw_resized_crop_params``
restates the draw) and resampled with PIL's bilinear filter, byte for byte (``resample_reference`` restates the pixels; it
is documentation and test infrastructure, never called on the training path).

``DeviceDataset(policy="ra" | "cifar10" | [sub-policies])`` chains up to four such operations per image (RandAugment,
AutoAugment) in one launch of ``nbdt_policy_chain_batch`` (``draw_chain_params``, ``chain_reference``, ``chain_table``).
``DeviceDataset(policy="ta_wide", erase_prob=p)`` adds an augmentation policy to the padded-crop family without leaving the
one launch: ``nbdt_policy_batch`` (csrc/policy.hip) applies one TrivialAugmentWide operation to the cropped and flipped
bytes, with Pillow's pixel rules, before the normalisation, and torchvision's RandomErasing after it
(``draw_policy_params`` restates the draw, ``policy_reference`` the pixels; like ``resample_reference`` it is never called on
the training path).

``ResizedCropDataset(policy=, erase_prob=)`` has the same policies and the erase on the ``size x size`` crop:
``nbdt_resized_crop_policy_batch`` (csrc/resample.hip) resamples to bytes and runs the chain between two global-memory tiles
per image, since a 224 x 224 crop fits no LDS tile (``resized_crop_policy_reference`` restates the pixels).

Both classes take ``shard=(rank, world)``: the rank then keeps only its contiguous part ``shard_range(N, rank, world)`` of
the dataset on its GPU (ImageNet at 256 x 256 is 252 GB whole, 31.5 GB per rank at 8 ranks) and ``batch`` still takes
indices into the whole dataset.  The kernels draw from that index and gather from ``index - lo``
(``nbdt_augment_batch_sharded`` / ``nbdt_resized_crop_batch_sharded``), so a sample's augmentation does not depend on
which rank holds it.
"""
import functools
import math

import numpy as np
import torch

from nbdt import _C, ops

# mean, std, pad of the reference's transform_train (nbdt/data/cifar.py:14-19, nbdt/data/imagenet.py:41-46)
DATASET_STATS = {
    "CIFAR10": {"mean": (0.4914, 0.4822, 0.4465), "std": (0.2023, 0.1994, 0.2010), "pad": 4},
    "CIFAR100": {"mean": (0.4914, 0.4822, 0.4465), "std": (0.2023, 0.1994, 0.2010), "pad": 4},
    "TinyImagenet200": {"mean": (0.4802, 0.4481, 0.3975), "std": (0.2302, 0.2265, 0.2262), "pad": 8},
}

# the resized-crop family: statistics, output side, evaluation resize and the draw's ranges of the reference's
# transform_train / transform_val (nbdt/data/imagenet.py:152-172; scale and ratio are torchvision's defaults)
RESIZED_CROP_STATS = {
    "Imagenet1000": {"mean": (0.485, 0.456, 0.406), "std": (0.229, 0.224, 0.225), "size": 224, "resize": 256,
                     "scale": (0.08, 1.0), "ratio": (3.0 / 4.0, 4.0 / 3.0)},
}

MAX_PAD = _C.NBDT_AUGMENT_MAX_PAD
MAX_SIDE = 4096                      # nbdt_resized_crop_batch: image and resized sides
RESIZED_CROP_POLICY_MAX_SIDE = _C.NBDT_RESIZED_CROP_POLICY_MAX_SIDE      # nbdt_resized_crop_policy_batch: the crop's side
_M64 = (1 << 64) - 1


def shard_range(n, rank, world):
    """[lo, hi) of the n samples that rank `rank` of `world` owns: ``lo = rank * n // world``, ``hi = (rank + 1) * n //
    world``.  The ranges are contiguous, tile [0, n) in rank order and their sizes differ by at most one; with n < world
    some are empty.  THE rule: the datasets, the sampler (nbdt.dist.epoch_indices) and main.py's evaluation all use it."""
    n, rank, world = int(n), int(rank), int(world)
    if n < 0 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"need n >= 0 and 0 <= rank < world, got n {n}, rank {rank}, world {world}")
    return rank * n // world, (rank + 1) * n // world


def label_subset(labels, num_classes, probability_labels=None, include_labels=None, exclude_labels=None,
                 include_classes=None, classes=None, seed=0):
    """The samples the reference's label-subset datasets keep (nbdt/data/custom.py: ResampleLabels / IncludeLabels /
    ExcludeLabels / IncludeClasses), as an ascending int64 tensor of indices into `labels`.

    Its rule (build_index_mapping): ``random.seed(seed)``, one ``random.random()`` draw per sample in dataset order, and
    the sample is kept when the draw is below ``p[label]``.  ``probability_labels`` is p -- a scalar or a one-element list
    broadcasts, any other length must be num_classes; include / exclude are the p of ones and zeros (a draw is always
    below 1 and never below 0); ``include_classes`` names entries of ``classes``.  Exactly one of the four selects.  The
    labels keep their num_classes-way numbering: a training loop indexes the dataset through the result."""
    import random
    given = [k for k, v in (("probability_labels", probability_labels), ("include_labels", include_labels),
                            ("exclude_labels", exclude_labels), ("include_classes", include_classes)) if v is not None]
    if len(given) != 1:
        raise ValueError(f"label_subset takes exactly one of probability_labels, include_labels, exclude_labels and "
                         f"include_classes, got {given or 'none'}")
    k = int(num_classes)
    if include_classes is not None:
        if classes is None:
            raise ValueError("include_classes needs the dataset's class names (classes=)")
        names = list(classes)
        include_labels = [names.index(c) for c in include_classes]
    if exclude_labels is not None:
        include_labels = set(range(k)) - set(int(c) for c in exclude_labels)
    if include_labels is not None:
        keep = set(int(c) for c in include_labels)
        p = [int(c in keep) for c in range(k)]
    else:
        p = probability_labels
        if not isinstance(p, (tuple, list)):
            p = [p] * k
        elif len(p) == 1:
            p = list(p) * k
        if len(p) != k:
            raise ValueError(f"Length of probabilities vector {len(p)} must equal that of the dataset classes {k}.")
    if isinstance(labels, torch.Tensor):
        labels = labels.cpu().numpy()
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    if labels.size and (int(labels.min()) < 0 or int(labels.max()) >= k):
        raise ValueError(f"labels must lie in [0, {k}), got min {int(labels.min())}, max {int(labels.max())}")
    rng = random.Random(seed)          # random.seed(seed) + random.random(), without touching the global generator
    kept = [i for i, label in enumerate(labels.tolist()) if rng.random() < p[label]]
    if not kept:
        raise ValueError("the label subset is empty: no sample of the dataset was kept")
    return torch.tensor(kept, dtype=torch.int64)


def _place(name, x, y, shard, device):
    """(x, y on the device, (lo, hi), N): the whole of the N samples, or with shard = (rank, world) only the rank's
    range of them -- sliced on the host, so the rest of `x` (a memory-mapped file, say) is never read or copied."""
    n = x.shape[0]
    lo, hi = 0, n
    if shard is not None:
        if len(shard) != 2:
            raise ValueError(f"shard must be (rank, world), got {shard!r}")
        lo, hi = shard_range(n, shard[0], shard[1])
        if hi <= lo:
            raise ValueError(f"{name}: rank {int(shard[0])} of {int(shard[1])} owns none of the {n} samples (an empty "
                             f"shard [{lo}, {hi})); use at most {n} ranks")
        x, y = x[lo:hi], y[lo:hi]
    return x.to(device).contiguous(), y.to(device=device, dtype=torch.int64).contiguous(), (lo, hi), n


def _check_host_index(index, span, sharded):
    """A host index tensor against the range the dataset holds: IndexError for a whole dataset (as ever), ValueError naming
    the owned range for a shard."""
    lo, hi = span
    imin, imax = int(index.min()), int(index.max())
    if imin < lo or imax >= hi:
        if sharded:
            raise ValueError(f"index outside the range this shard owns, [{lo}, {hi}): min {imin}, max {imax} (batch takes "
                             "global dataset indices; another rank holds the rest)")
        raise IndexError(f"index outside [0, {hi}): min {imin}, max {imax}")


_mix64 = ops._mix64


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


def _check_policy_source(x):
    """The policy kernel works on bytes staged in LDS: refuse anything else on the host, before any launch."""
    if x.dtype != torch.uint8:
        raise ValueError(f"the augmentation policy and random erasing work on a uint8 dataset, got {x.dtype} (an fp32 "
                         "dataset is already normalised: there are no bytes left to posterize or equalize)")
    if 3 * x.shape[2] * x.shape[3] > POLICY_MAX_BYTES:
        raise ValueError(f"the augmentation policy and random erasing take images of at most {POLICY_MAX_BYTES} bytes "
                         f"(128 x 128 x 3), got {tuple(x.shape[1:])}")


def _check_policy(policy, policy_ops, policy_magnitude):
    """The `policy` setting of both dataset classes, checked on the host: (sub-policies int32 [P,4,3] or None, policy_ops,
    policy_magnitude)."""
    subs = None
    if isinstance(policy, (list, tuple)) or policy in ("cifar10", "imagenet"):
        subs = subpolicy_array(policy)
    elif policy == "ra":
        policy_ops, policy_magnitude = _check_ra(policy_ops, policy_magnitude)
    elif policy not in (None, "ta_wide"):
        raise ValueError("policy must be None, 'ta_wide', 'ra', 'cifar10', 'imagenet' or a list of sub-policies, got "
                         f"{policy!r}")
    return subs, policy_ops, policy_magnitude


def _device_rows(v, name, shape, rule, args, device, who, dtype=None):
    """An integer parameter tensor of `shape` for a batch launch, on the device: a host tensor is checked with
    ``rule(rows as int64, *args)`` -- (the rows that are in range, the range in words for the ValueError) -- and copied, a
    device tensor goes to the kernel, which clamps it.  dtype None: any integer type, handed on as int32; a dtype: exactly
    that one, handed on as it is."""
    if not isinstance(v, torch.Tensor):
        v = torch.as_tensor(np.asarray(v))
    wrong = v.is_floating_point() or v.dtype == torch.bool if dtype is None else v.dtype != dtype
    if tuple(v.shape) != shape or wrong:
        kind = "integer" if dtype is None else str(dtype).replace("torch.", "")
        raise ValueError(f"{name} must be {kind} {list(shape)}, got {v.dtype} {tuple(v.shape)}")
    if not v.is_cuda:
        ok, what = rule(v.long(), *args)
        if not bool(ok.all()):
            raise ValueError(f"{name} outside {what}")
        v = v.to(device, non_blocking=True)
    _C.require_gpu(v, who)
    want = dtype or torch.int32
    return v if v.dtype == want and v.is_contiguous() else v.to(dtype=want).contiguous()


# the rules of _device_rows: module-level, so that a batch call builds no closure
def _crop_rule(p, pad):
    return ((p >= 0).all(dim=1) & (p[:, 0] <= 2 * pad) & (p[:, 1] <= 2 * pad) & (p[:, 2] <= 1),
            f"dy, dx in [0, {2 * pad}], flip in {{0, 1}}")


def _box_rule(p, H, W):
    return ((p[:, 0] >= 0) & (p[:, 1] >= 0) & (p[:, 2] >= 1) & (p[:, 3] >= 1) & (p[:, 0] + p[:, 2] <= H)
            & (p[:, 1] + p[:, 3] <= W) & (p[:, 4] >= 0) & (p[:, 4] <= 1),
            f"the {H} x {W} image (top, left >= 0, h, w >= 1, top + h <= H, left + w <= W) or flip outside {{0, 1}}")


def _policy_rule(p, H, W):
    return ((p[:, 0] >= 0) & (p[:, 0] < len(POLICY_OPS)) & (p[:, 1] >= 0) & (p[:, 1] < POLICY_BINS) & (p[:, 2] >= 0)
            & (p[:, 2] <= 1) & (p[:, 3:] >= 0).all(dim=1) & (p[:, 3] + p[:, 5] <= H) & (p[:, 4] + p[:, 6] <= W),
            f"op in [0, {len(POLICY_OPS) - 1}], bin in [0, {POLICY_BINS - 1}], sign in {{0, 1}} or an erase rectangle outside "
            f"the {H} x {W} image")


def _chain_rule(p, nbins):
    return ((p[..., 0] >= 0) & (p[..., 0] < len(CHAIN_OPS)) & (p[..., 1] >= 0) & (p[..., 1] < nbins) & (p[..., 2] >= 0)
            & (p[..., 2] <= 1), f"op in [0, {len(CHAIN_OPS) - 1}], bin in [0, {nbins - 1}], sign in {{0, 1}}")


def _erase_rule(p, H, W):
    return (p >= 0).all(dim=1) & (p[:, 0] + p[:, 2] <= H) & (p[:, 1] + p[:, 3] <= W), f"the {H} x {W} image"


def _chain_rows(chain_params, erase_params, B, nbins, H, W, device, who):
    """chain_params [B,4,3] and erase_params [B,4] (either may be None) through ``_device_rows``."""
    if chain_params is not None:
        chain_params = _device_rows(chain_params, "chain_params", (B, CHAIN_MAX_OPS, 3), _chain_rule, (nbins,), device, who)
    if erase_params is not None:
        erase_params = _device_rows(erase_params, "erase_params", (B, 4), _erase_rule, (H, W), device, who)
    return chain_params, erase_params


class _DeviceBatches:
    """What DeviceDataset and ResizedCropDataset share: the settings and their checks, the placement of (a shard of) the
    samples, the index of a batch, the device copies of the policies' tables and the tuple a batch returns.  The geometry,
    `batch` and the routing between launches are each class's own."""

    def __init__(self, x, y, mean, std, flip, device, policy, erase_prob, erase_scale, erase_ratio, policy_ops,
                 policy_magnitude, dtypes):
        """The settings, checked; `_hold` (after the subclass's own checks) moves the samples."""
        who = type(self).__name__
        self._who = who + ".batch"
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _C.NBDTHipError(f"{who} lives on an MI355X, not on {self.device} (no CPU fallback)")
        # int32 [P,4,3] on the host when the policy is a list of sub-policies (AutoAugment), else None
        self._subpolicies, policy_ops, policy_magnitude = _check_policy(policy, policy_ops, policy_magnitude)
        self.policy = policy
        self.policy_ops, self.policy_magnitude = policy_ops, policy_magnitude
        self.erase_prob = _check_erase(erase_prob, erase_scale, erase_ratio)
        self.erase_scale = tuple(float(v) for v in erase_scale)
        self.erase_ratio = tuple(float(v) for v in erase_ratio)
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype not in dtypes:
            kinds = " or ".join({torch.uint8: "uint8", torch.float32: "fp32"}[d] for d in dtypes)
            raise ValueError(f"x must be {kinds} [N,3,H,W], got {x.dtype} {tuple(x.shape)}")
        if y.dim() != 1 or y.shape[0] != x.shape[0] or y.is_floating_point():
            raise ValueError(f"y must be integer [N] with N = {x.shape[0]}, got {y.dtype} {tuple(y.shape)}")
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("mean and std have one entry per channel (3)")
        self.mean = tuple(float(m) for m in mean)
        self.std = tuple(float(s) for s in std)
        self.flip = bool(flip)
        self._tables_on_device = {}       # the policies' tables, each built and copied by the first batch that needs it

    def _hold(self, x, y, shard):
        self.sharded = shard is not None
        self.x, self.y, self.shard_range, self.global_size = _place(type(self).__name__, x, y, shard, self.device)
        self.device = self.x.device       # (with its index)

    def __len__(self):
        return self.x.shape[0]

    @property
    def shape(self):
        return self.x.shape

    def _index(self, index):
        """`index` as a contiguous int64 device vector; a host one is range-checked first."""
        if not isinstance(index, torch.Tensor):
            index = torch.as_tensor(np.asarray(index))
        if index.dim() != 1 or index.is_floating_point() or index.shape[0] == 0:
            raise ValueError(f"index must be a non-empty integer vector, got {index.dtype} {tuple(index.shape)}")
        if not index.is_cuda:
            _check_host_index(index, self.shard_range, self.sharded)
            index = index.to(self.device, non_blocking=True)
        _C.require_gpu(index, self._who)
        return index if index.dtype == torch.int64 and index.is_contiguous() else index.to(dtype=torch.int64).contiguous()

    def _table_on_device(self, name, build, *args):
        """The host table ``build(*args)`` on the device; built once."""
        t = self._tables_on_device.get(name)
        if t is None:
            t = self._tables_on_device[name] = torch.from_numpy(build(*args).copy()).to(self.device)
        return t

    def _chain_tables(self, name, H, W):
        """(chain table of ``chain_table(name, H, W)`` or None without a name, sub-policies or None, erase ratio table)."""
        return (None if name is None else self._table_on_device("chain", chain_table, name, H, W),
                None if self._subpolicies is None else self._table_on_device("subpolicies", np.asarray, self._subpolicies),
                self._table_on_device("erase ratios", ratio_table, self.erase_ratio))

    def _used(self, *shape):
        """An int32 tensor for a launch to report what it used in."""
        return torch.empty(shape, dtype=torch.int32, device=self.device)

    def _extras(self, *extras):
        """The optional returns after (img, targets[, params]): each is (wanted, what a launch wrote or None, its shape), in
        the documented order; a wanted one that no launch wrote is zeros -- nothing was applied: Identity, no erase."""
        return tuple(torch.zeros(shape, dtype=torch.int32, device=self.device) if t is None else t
                     for wanted, t, shape in extras if wanted)


class DeviceDataset(_DeviceBatches):
    """A dataset held on the device, batched by `nbdt_augment_batch`.

    x: uint8 or fp32 ``[N,3,H,W]``; y: integer ``[N]``; both are moved to `device` once.  A uint8 `x` is scaled by 1/255
    and normalised with `mean` / `std` in the kernel, its padding is byte 0 before conversion (so a padded pixel is
    ``(0 - mean)/std``).  An fp32 `x` is taken as already normalised and copied; its padded pixels get `fill`, by default
    ``(0 - mean)/std`` -- a file normalised with the dataset's statistics then yields the same batches as its uint8
    original.  pad: pixels of zero padding before the random ``H x W`` crop; flip: random horizontal flip.

    policy="ra": RandAugment -- `policy_ops` (1..4) operations per training sample, each uniform among POLICY_OPS at bin
    `policy_magnitude` (0..30) with a random sign; policy="cifar10", "imagenet" or a list of sub-policies
    (``subpolicy_array``'s form): AutoAugment -- one sub-policy per sample, each of its slots applied with its probability.  Both run the whole chain in
    ``nbdt_policy_chain_batch``, one launch per batch, with the crop, flip and erase rectangle of every other setting.

    policy="ta_wide": every training sample gets one TrivialAugmentWide operation (POLICY_OPS, 31 magnitude bins) between the
    flip and the normalisation; erase_prob > 0: torchvision's RandomErasing(p, erase_scale, erase_ratio, value=0) after the
    normalisation.  Both need a uint8 `x` of at most 49152 bytes per image and run in ``nbdt_policy_batch``, still one launch
    per batch (csrc/policy.hip); the crop and the flip of a sample are the same with and without them.

    shard=(rank, world): only the samples ``shard_range(N, rank, world)`` are moved to the device.  ``shape[0]`` and
    ``len()`` are then the number held, ``global_size`` is N, ``shard_range`` the owned [lo, hi); ``batch`` keeps taking
    indices into the whole dataset and returns, for an index it owns, the very batch the unsharded dataset returns.
    """

    def __init__(self, x, y, mean, std, pad, flip=True, fill=None, device="cuda", shard=None, policy=None, erase_prob=0.0,
                 erase_scale=(0.02, 0.33), erase_ratio=(0.3, 3.3), policy_ops=2, policy_magnitude=9):
        super().__init__(x, y, mean, std, flip, device, policy, erase_prob, erase_scale, erase_ratio, policy_ops,
                         policy_magnitude, (torch.uint8, torch.float32))
        self.chain = policy is not None and policy != "ta_wide"       # RandAugment / AutoAugment: nbdt_policy_chain_batch
        if not 0 <= int(pad) <= MAX_PAD:
            raise ValueError(f"pad must be 0..{MAX_PAD}, got {pad}")
        if fill is None:       # (0 - mean) / std in fp32, the kernel's value of a padded uint8 pixel
            fill = ((torch.zeros(3) - torch.tensor(self.mean)) / torch.tensor(self.std)).tolist()
        self.fill = tuple(float(f) for f in fill)
        self.pad = int(pad)
        if policy is not None or self.erase_prob > 0.0:
            _check_policy_source(x)
        self._hold(x, y, shard)

    def batch(self, index, epoch=0, seed=0, train=True, params=None, return_params=False, policy_params=None,
              return_policy_params=False, chain_params=None, return_chain_params=False, erase_params=None,
              return_erase_params=False):
        """(img fp32 [B,3,H,W], targets int64 [B][, params int8 [B,3]]) for the samples `index`, in ONE launch on torch's
        current stream.

        index: a host sequence / array / CPU tensor is range-checked (IndexError; ValueError naming the owned range for a
        shard) and copied; a device tensor goes straight to the kernel, which writes a zero image with target -1 for an
        index outside [0, N), or outside the owned range of a shard.  train=False is the evaluation transform (no crop, no
        flip).  params: int8 [B,3] of (dy, dx, flip) replaces the generator; a CPU tensor is
        range-checked and copied.  Without it the draw is ``draw_params(seed, epoch, index, pad)``.

        With ``policy="ta_wide"`` or ``erase_prob > 0`` (or policy_params) a training batch is ONE launch of
        nbdt_policy_batch instead: the same crop and flip, then one TrivialAugmentWide operation on the bytes, the
        normalisation, then the erase rectangle set to 0.0.  policy_params: integer [B,7] of (op, bin, sign, top, left, h,
        w) replaces that draw (h = w = 0: no erase); a CPU tensor is range-checked and copied, a device tensor is clamped by
        the kernel.  Without it the draw is ``draw_policy_params(seed, epoch, index, H, W, erase_prob, erase_scale,
        erase_ratio)`` (every op is Identity when policy is None).  return_policy_params appends the int32 [B,7] used.
        train=False never applies a policy.  With neither setting nor argument the launch is nbdt_augment_batch, untouched.

        With ``policy="ra"``, ``"cifar10"`` or a list of sub-policies a training batch is ONE launch of
        nbdt_policy_chain_batch: the same crop, flip and erase rectangle, and between flip and normalisation the chain of
        up to four operations ``draw_chain_params(seed, epoch, index, policy, policy_ops, policy_magnitude)`` draws.
        chain_params: integer [B,4,3] of (op, bin, sign) per slot (op indexes CHAIN_OPS, Identity for an unused slot)
        replaces that draw; erase_params: integer [B,4] of (top, left, h, w) replaces the erase draw; a CPU tensor is
        range-checked and copied, a device tensor is clamped by the kernel.  return_chain_params / return_erase_params
        append the int32 [B,4,3] / [B,4] used, in that order, after the other returns.  These four arguments belong to
        the chain policies (policy_params / return_policy_params to None and "ta_wide"): the other kind is a ValueError.

        Every call returns freshly allocated tensors (torch's caching allocator): train_step is asynchronous and the engine
        keeps `img` until the stem's weight gradient, so nothing handed out is ever overwritten by a later call."""
        who = self._who
        index = self._index(index)
        pad, flip = (self.pad, self.flip) if train else (0, False)
        B, H, W = index.shape[0], self.x.shape[2], self.x.shape[3]
        if params is not None:
            if not train:
                raise ValueError("params replace the training draw; train=False has none")
            params = _device_rows(params, "params", (B, 3), _crop_rule, (pad,), self.device, who, dtype=torch.int8)
        if policy_params is not None:
            if not train:
                raise ValueError("policy_params replace the training draw; train=False has none")
            _check_policy_source(self.x)
            policy_params = _device_rows(policy_params, "policy_params", (B, 7), _policy_rule, (H, W), self.device, who)
        chain_args = chain_params is not None or erase_params is not None or return_chain_params or return_erase_params
        if chain_args and not self.chain:
            raise ValueError("chain_params / erase_params and their returns belong to policy='ra', 'cifar10' or a list of "
                             f"sub-policies; this dataset has policy={self.policy!r} (use policy_params)")
        if self.chain and (policy_params is not None or return_policy_params):
            raise ValueError(f"policy_params belong to policy=None or 'ta_wide'; policy={self.policy!r} takes chain_params "
                             "and erase_params")
        if not train and (chain_params is not None or erase_params is not None):
            raise ValueError("chain_params / erase_params replace the training draw; train=False has none")
        img = torch.empty((B,) + tuple(self.x.shape[1:]), dtype=torch.float32, device=self.device)
        targets = torch.empty((B,), dtype=torch.int64, device=self.device)
        used = torch.empty((B, 3), dtype=torch.int8, device=self.device) if return_params else None
        base = self.shard_range[0] if self.sharded else None
        pused = cused = eused = None
        if self.chain and train:
            table, subs, ratios = self._chain_tables("ra" if self.policy == "ra" else "cifar10", H, W)
            nbins = table.shape[1]
            chain_params, erase_params = _chain_rows(chain_params, erase_params, B, nbins, H, W, self.device, who)
            cused = self._used(B, CHAIN_MAX_OPS, 3) if return_chain_params else None
            eused = self._used(B, 4) if return_erase_params else None
            ops.policy_chain_batch(self.x, self.y, index, img, targets, pad, flip, self.mean, self.std, table, nbins,
                                   num_ops=self.policy_ops, magnitude=self.policy_magnitude, subpolicies=subs,
                                   ratio_table=ratios, seed=seed, epoch=epoch, params_in=params, chain_in=chain_params,
                                   erase_in=erase_params, params_out=used, chain_out=cused, erase_out=eused, index_base=base,
                                   erase_prob=self.erase_prob, erase_scale=self.erase_scale, erase_ratio=self.erase_ratio)
        elif train and (self.policy is not None or self.erase_prob > 0.0 or policy_params is not None):
            table = self._table_on_device("policy", policy_table, H, W)
            pused = self._used(B, 7) if return_policy_params else None
            ops.policy_batch(self.x, self.y, index, img, targets, pad, flip, self.mean, self.std,
                             policy=self.policy is not None, policy_table=table,
                             ratio_table=self._table_on_device("erase ratios", ratio_table, self.erase_ratio), seed=seed,
                             epoch=epoch, params_in=params, policy_in=policy_params, params_out=used, policy_out=pused,
                             index_base=base, erase_prob=self.erase_prob, erase_scale=self.erase_scale,
                             erase_ratio=self.erase_ratio)
        else:
            ops.augment_batch(self.x, self.y, index, img, targets, pad, flip, mean=self.mean, std=self.std, fill=self.fill,
                              seed=seed, epoch=epoch, params_in=params, params_out=used, index_base=base)
        out = (img, targets, used) if return_params else (img, targets)
        if return_policy_params or return_chain_params or return_erase_params:
            out += self._extras((return_policy_params, pused, (B, 7)), (return_chain_params, cused, (B, CHAIN_MAX_OPS, 3)),
                                (return_erase_params, eused, (B, 4)))
        return out


# ----------------------------------------------------------------------------------------------------------------------
# the resized-crop family (nbdt_resized_crop_batch)

@functools.lru_cache(maxsize=8)
def _ratio_table(lo, hi):
    t = np.exp(np.linspace(math.log(lo), math.log(hi), _C.NBDT_RESIZED_CROP_RATIOS))
    t[0], t[-1] = lo, hi
    t.setflags(write=False)
    return t


def ratio_table(ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """The fp64 aspect ratios the draw chooses from: NBDT_RESIZED_CROP_RATIOS log-spaced values from ratio[0] to ratio[1].
    torchvision draws ``exp(uniform(log lo, log hi))``; exp is not correctly rounded on the host or the device, so the law is
    quantised to this table, which both sides index with random bits."""
    return _ratio_table(float(ratio[0]), float(ratio[1]))


def _check_ranges(scale, ratio):
    if len(scale) != 2 or not 0.0 < scale[0] <= scale[1] <= 1.0:
        raise ValueError(f"scale must satisfy 0 < lo <= hi <= 1, got {tuple(scale)}")
    if len(ratio) != 2 or not 1.0 / 64.0 <= ratio[0] <= ratio[1] <= 64.0:
        raise ValueError(f"ratio must satisfy 1/64 <= lo <= hi <= 64, got {tuple(ratio)}")


def _round_sqrt(v):
    """round-half-to-even of sqrt(v), decided by exact comparisons (c*c and (c + 1/2)**2 are exact in fp64 here), so it
    does not depend on how sqrt itself is rounded."""
    c = np.sqrt(v).astype(np.int64)
    c = c - ((c * c).astype(np.float64) > v)
    c = c + (((c + 1) * (c + 1)).astype(np.float64) <= v)
    half = (c.astype(np.float64) + 0.5) * (c.astype(np.float64) + 0.5)
    return c + (v > half) + ((v == half) & ((c & 1) == 1))


def draw_resized_crop_params(seed, epoch, index, H, W, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0),
                             return_attempt=False):
    """The generator of nbdt_resized_crop_batch (include/nbdt_hip.h), restated with numpy: (top, left, h, w, flip) int64
    arrays shaped like `index`.  torchvision's RandomResizedCrop.get_params: up to 10 attempts of (area fraction uniform
    in `scale`, aspect ratio from ``ratio_table(ratio)``, w = round(sqrt(area * r)), h = round(sqrt(area / r)), accepted if
    it fits, position uniform), else the centre crop with the ratio clamped.  A pure function of (seed, epoch, dataset
    index, H, W, scale, ratio).  return_attempt: also the attempt that was accepted, NBDT_RESIZED_CROP_ATTEMPTS for the
    fallback."""
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"image sides must be 1..{MAX_SIDE}, got {H} x {W}")
    _check_ranges(scale, ratio)
    s0, s1, r0, r1 = float(scale[0]), float(scale[1]), float(ratio[0]), float(ratio[1])
    table = ratio_table(ratio)
    if isinstance(index, torch.Tensor):
        index = index.cpu().numpy()
    idx = np.asarray(index).astype(np.int64).astype(np.uint64)
    u64 = np.uint64
    m24, golden = u64(0xFFFFFF), 0x9E3779B97F4A7C15
    attempts = _C.NBDT_RESIZED_CROP_ATTEMPTS
    with np.errstate(over="ignore"):
        key = _mix64(np.asarray([(int(seed) * golden + int(epoch)) & _M64], dtype=np.uint64))[0]
        base = _mix64(key ^ (idx * u64(0xD1342543DE82EF95)))
        flip = (base >> u64(63)).astype(np.int64)
        # the fallback first; accepted attempts overwrite it, the earliest one last
        h = np.full(idx.shape, H, dtype=np.int64)
        w = np.full(idx.shape, W, dtype=np.int64)
        if W / H < r0:
            h[...] = min(max(int(np.rint(W / r0)), 1), H)
        elif W / H > r1:
            w[...] = min(max(int(np.rint(H * r1)), 1), W)
        top, left = (H - h) // 2, (W - w) // 2
        which = np.full(idx.shape, attempts, dtype=np.int64)
        for t in reversed(range(attempts)):
            ra = _mix64(base + u64(((2 * t + 1) * golden) & _M64))
            rb = _mix64(base + u64(((2 * t + 2) * golden) & _M64))
            u = (ra >> u64(11)).astype(np.float64) * 2.0 ** -53
            target = float(H * W) * (s0 + u * (s1 - s0))
            r = table[(rb & u64(_C.NBDT_RESIZED_CROP_RATIOS - 1)).astype(np.int64)]
            cw, ch = _round_sqrt(target * r), _round_sqrt(target / r)
            ok = (cw > 0) & (cw <= W) & (ch > 0) & (ch <= H)
            ct = (((rb >> u64(12)) & m24) * np.clip(H - ch + 1, 0, None).astype(np.uint64)) >> u64(24)
            cl = (((rb >> u64(36)) & m24) * np.clip(W - cw + 1, 0, None).astype(np.uint64)) >> u64(24)
            top, left = np.where(ok, ct.astype(np.int64), top), np.where(ok, cl.astype(np.int64), left)
            h, w, which = np.where(ok, ch, h), np.where(ok, cw, w), np.where(ok, t, which)
    out = (top, left, h, w, flip)
    return out + (which,) if return_attempt else out


def _axis_coefficients(in_size, out_size, first, count):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for the bilinear (triangle) filter: for output pixels
    [first, first + count) of an axis of `in_size` pixels resampled to `out_size`, a list of (xmin, int64 coefficients)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support, ss = 1.0 * filterscale, 1.0 / filterscale
    taps = []
    for xx in range(first, first + count):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        x = np.arange(xmin, xmax, dtype=np.float64)
        v = np.abs((x - center + 0.5) * ss)
        k = np.where(v < 1.0, 1.0 - v, 0.0)
        ww = 0.0
        for kk in k:              # summed in tap order, as PIL does
            ww += kk
        if ww != 0.0:
            k = k / ww
        taps.append((xmin, (0.5 + k * float(1 << 22)).astype(np.int64)))
    return taps


def resample_reference(img_u8, box, out_size, window=None):
    """``PIL.Image.fromarray(img).crop(box).resize(out_size, BILINEAR)`` restated with numpy for one uint8 ``[3,H,W]`` image
    (an array or a CPU tensor); returns a uint8 array.  box: (top, left, h, w) inside the image; out_size: (rs_h, rs_w);
    window: (top, left, h, w) inside the resized image, the part that is returned (default: all of it).

    PIL's arithmetic for an 8-bit image: triangle filter with support max(1, in/out) per axis, clipped at the box,
    coefficients in fp64, normalised, rounded to 22-bit fixed point; horizontal pass, rounded and clipped to uint8; vertical
    pass over those uint8 values, rounded and clipped to uint8.  What nbdt_resized_crop_batch computes before it flips and
    normalises.  Test infrastructure and documentation: it must not be called on the training path."""
    if isinstance(img_u8, torch.Tensor):
        img_u8 = img_u8.cpu().numpy()
    img = np.asarray(img_u8)
    if img.ndim != 3 or img.shape[0] != 3 or img.dtype != np.uint8:
        raise ValueError(f"img must be uint8 [3,H,W], got {img.dtype} {img.shape}")
    top, left, h, w = (int(v) for v in box)
    if not (0 <= top and 0 <= left and h >= 1 and w >= 1 and top + h <= img.shape[1] and left + w <= img.shape[2]):
        raise ValueError(f"box {tuple(box)} is not inside the {img.shape[1]} x {img.shape[2]} image")
    rs_h, rs_w = (int(v) for v in out_size)
    wt, wl, wh, ww_ = (0, 0, rs_h, rs_w) if window is None else (int(v) for v in window)
    if not (0 <= wt and 0 <= wl and wh >= 1 and ww_ >= 1 and wt + wh <= rs_h and wl + ww_ <= rs_w):
        raise ValueError(f"window {tuple(window)} is not inside the {rs_h} x {rs_w} resized image")
    src = img[:, top:top + h, left:left + w].astype(np.int64)
    half = 1 << 21
    horiz = np.empty((3, h, ww_), dtype=np.int64)
    for j, (xmin, k) in enumerate(_axis_coefficients(w, rs_w, wl, ww_)):
        horiz[:, :, j] = np.clip((half + (src[:, :, xmin:xmin + len(k)] * k).sum(axis=2)) >> 22, 0, 255)
    out = np.empty((3, wh, ww_), dtype=np.int64)
    for i, (ymin, k) in enumerate(_axis_coefficients(h, rs_h, wt, wh)):
        out[:, i, :] = np.clip((half + (horiz[:, ymin:ymin + len(k), :] * k[None, :, None]).sum(axis=1)) >> 22, 0, 255)
    return out.astype(np.uint8)


def resize_center_crop_geometry(H, W, size, resize):
    """torchvision's ``Resize(resize) -> CenterCrop(size)`` on an H x W image as (resized (rs_h, rs_w), window (top, left)):
    the short side becomes `resize`, the long side ``int(resize * long / short)``, and the crop starts at
    ``int(round((side - size) / 2))``."""
    H, W, size, resize = int(H), int(W), int(size), int(resize)
    if W <= H:
        rs_h, rs_w = int(resize * H / W), resize
    else:
        rs_h, rs_w = resize, int(resize * W / H)
    if size > min(rs_h, rs_w):
        raise ValueError(f"the {size} x {size} crop does not fit the resized {rs_h} x {rs_w} image")
    return (rs_h, rs_w), (int(round((rs_h - size) / 2.0)), int(round((rs_w - size) / 2.0)))


class ResizedCropDataset(_DeviceBatches):
    """A uint8 dataset held on the device, batched by `nbdt_resized_crop_batch`: the reference's ImageNet transforms.

    x: uint8 ``[N,3,H,W]`` (any fixed H x W up to 4096: ImageNet stored at 256 x 256, a downsampled ImageNet); y: integer
    ``[N]``; both are moved to `device` once.  Training batches are ``RandomResizedCrop(size, scale, ratio) ->
    RandomHorizontalFlip -> ToTensor -> Normalize(mean, std)``; evaluation batches are ``Resize(resize) -> CenterCrop(size)
    -> ToTensor -> Normalize`` (resize defaults to size + 32, as in the reference).  The resampling is PIL's bilinear filter.

    policy / erase_prob / erase_scale / erase_ratio / policy_ops / policy_magnitude: DeviceDataset's settings, here on the
    ``size x size`` crop (at most 512 x 512): policy="ta_wide" (one TrivialAugmentWide operation), "ra" (RandAugment),
    "cifar10" / "imagenet" / a list of sub-policies (AutoAugment) apply a chain of up to four operations to the resized and
    flipped bytes, before the normalisation; erase_prob > 0 is torchvision's RandomErasing(value=0) after it.  Such a
    training batch is ``nbdt_resized_crop_policy_batch`` (two launches, no host read-back); the magnitude tables are built
    for the crop (translations (150/331) * size, Rotate about its centre), and a sample's box and flip are the same with and
    without a policy.  With policy=None and erase_prob == 0 nothing changes: one launch, the same bits.

    shard=(rank, world): as for DeviceDataset -- only ``shard_range(N, rank, world)`` is held, ``batch`` takes indices into
    the whole dataset; ``global_size`` and ``shard_range`` say what is where.
    """

    def __init__(self, x, y, mean, std, size=224, resize=None, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip=True,
                 device="cuda", shard=None, policy=None, erase_prob=0.0, erase_scale=(0.02, 0.33), erase_ratio=(0.3, 3.3),
                 policy_ops=2, policy_magnitude=9):
        super().__init__(x, y, mean, std, flip, device, policy, erase_prob, erase_scale, erase_ratio, policy_ops,
                         policy_magnitude, (torch.uint8,))
        self.chain = policy is not None          # every policy is a chain here: nbdt_resized_crop_policy_batch
        if not (1 <= x.shape[2] <= MAX_SIDE and 1 <= x.shape[3] <= MAX_SIDE):
            raise ValueError(f"image sides must be 1..{MAX_SIDE}, got {tuple(x.shape[2:])}")
        _check_ranges(scale, ratio)
        self.size = int(size)
        self.resize = self.size + 32 if resize is None else int(resize)
        if not 1 <= self.size <= self.resize <= MAX_SIDE:
            raise ValueError(f"need 1 <= size <= resize <= {MAX_SIDE}, got size {size}, resize {self.resize}")
        if (policy is not None or self.erase_prob > 0.0) and self.size > RESIZED_CROP_POLICY_MAX_SIDE:
            raise ValueError(f"the augmentation policy and random erasing take crops of at most "
                             f"{RESIZED_CROP_POLICY_MAX_SIDE} x {RESIZED_CROP_POLICY_MAX_SIDE}, got size {self.size}")
        self.scale = tuple(float(v) for v in scale)
        self.ratio = tuple(float(v) for v in ratio)
        self.eval_resize, self.eval_window = resize_center_crop_geometry(x.shape[2], x.shape[3], self.size, self.resize)
        if max(self.eval_resize) > MAX_SIDE:
            raise ValueError(f"the evaluation resize {self.eval_resize} exceeds {MAX_SIDE}")
        self._hold(x, y, shard)
        self._table = torch.from_numpy(ratio_table(self.ratio).copy()).to(self.device)
        self._whole = torch.empty((0, 5), dtype=torch.int32, device=self.device)     # evaluation boxes, grown on demand

    def _whole_image(self, B):
        if self._whole.shape[0] < B:
            row = torch.tensor([0, 0, self.x.shape[2], self.x.shape[3], 0], dtype=torch.int32)
            self._whole = row.repeat(B, 1).to(self.device)
        return self._whole[:B]

    def batch(self, index, epoch=0, seed=0, train=True, params=None, return_params=False, chain_params=None,
              return_chain_params=False, erase_params=None, return_erase_params=False):
        """(img fp32 [B,3,size,size], targets int64 [B][, params int32 [B,5]]) for the samples `index`, in ONE launch on
        torch's current stream.

        index: a host sequence / array / CPU tensor is range-checked (IndexError; ValueError naming the owned range for a
        shard) and copied; a device tensor goes straight to the kernel, which writes a zero image with target -1 for an
        index outside [0, N), or outside the owned range of a shard.  train=False is the evaluation transform (the whole
        image resized so that its short side is `resize`, the central size x size of it, no flip).
        params: int32 [B,5] of (top, left, h, w, flip) replaces the generator; a CPU tensor is range-checked and copied, a
        device tensor is clamped into the image by the kernel.  Without it the draw is
        ``draw_resized_crop_params(seed, epoch, index, H, W, scale, ratio)``.

        With a policy or ``erase_prob > 0`` a training batch is nbdt_resized_crop_policy_batch instead (two launches, two
        uint8 staging buffers from torch's caching allocator, stream-ordered): the same box and flip, then the chain
        ``draw_chain_params(seed, epoch, index, policy, policy_ops, policy_magnitude)`` draws -- for "ta_wide" one slot,
        (op, bin, sign) of ``draw_policy_params`` -- then the normalisation, then the erase rectangle of
        ``draw_policy_params(seed, epoch, index, size, size, erase_prob, erase_scale, erase_ratio)`` set to 0.0.
        chain_params (integer [B,4,3] of (op, bin, sign), needs a policy) and erase_params (integer [B,4] of (top, left, h,
        w)) replace those draws; a CPU tensor is range-checked and copied, a device tensor is clamped by the kernel.
        return_chain_params / return_erase_params append the int32 [B,4,3] / [B,4] used, in that order.  train=False
        never applies a policy or an erase.

        Every call returns freshly allocated tensors, as DeviceDataset.batch does."""
        who = self._who
        index = self._index(index)
        B, H, W, S = index.shape[0], self.x.shape[2], self.x.shape[3], self.size
        if params is not None:
            if not train:
                raise ValueError("params replace the training draw; train=False has none")
            params = _device_rows(params, "params", (B, 5), _box_rule, (H, W), self.device, who, dtype=torch.int32)
        if chain_params is not None and not self.chain:
            raise ValueError("chain_params belong to policy='ta_wide', 'ra', 'cifar10', 'imagenet' or a list of "
                             f"sub-policies; this dataset has policy={self.policy!r}")
        if not train and (chain_params is not None or erase_params is not None):
            raise ValueError("chain_params / erase_params replace the training draw; train=False has none")
        with_policy = train and (self.chain or self.erase_prob > 0.0 or erase_params is not None)
        if with_policy and S > RESIZED_CROP_POLICY_MAX_SIDE:
            raise ValueError(f"the augmentation policy and random erasing take crops of at most "
                             f"{RESIZED_CROP_POLICY_MAX_SIDE} x {RESIZED_CROP_POLICY_MAX_SIDE}, got size {S}")
        img = torch.empty((B, 3, S, S), dtype=torch.float32, device=self.device)
        targets = torch.empty((B,), dtype=torch.int64, device=self.device)
        used = self._used(B, 5) if return_params else None
        base = self.shard_range[0] if self.sharded else None
        cused = eused = None
        if not with_policy:
            if train:
                resize, window = (S, S), (0, 0)
            else:
                resize, window, params = self.eval_resize, self.eval_window, self._whole_image(B)
            ops.resized_crop_batch(self.x, self.y, index, img, targets, resize, window, self.flip and train, self.mean,
                                   self.std, scale=self.scale, ratio=self.ratio, ratio_table=self._table, seed=seed,
                                   epoch=epoch, params_in=params, params_out=used, index_base=base)
        else:
            # the erase alone: no operation reads a table; AutoAugment's sub-policies share "cifar10"'s ten bins
            name = self.policy if self.policy in (None, "ra", "ta_wide") else "cifar10"
            table, subs, ratios = self._chain_tables(name, S, S)
            nbins = 1 if table is None else table.shape[1]
            chain_params, erase_params = _chain_rows(chain_params, erase_params, B, nbins, S, S, self.device, who)
            cused = self._used(B, CHAIN_MAX_OPS, 3) if return_chain_params else None
            eused = self._used(B, 4) if return_erase_params else None
            # the chain's two tiles per image: scratch of this call (the caching allocator reuses it in stream order)
            stage_a = torch.empty((B, 3, S, S), dtype=torch.uint8, device=self.device)
            stage_b = torch.empty((B, 3, S, S), dtype=torch.uint8, device=self.device)
            ra = self.policy == "ra"
            ops.resized_crop_policy_batch(self.x, self.y, index, img, targets, self.flip, self.mean, self.std, stage_a, stage_b,
                                          scale=self.scale, ratio=self.ratio, ratio_table=self._table, table=table, nbins=nbins,
                                          num_ops=self.policy_ops if ra else 0, magnitude=self.policy_magnitude if ra else 0,
                                          subpolicies=subs, ta_wide=self.policy == "ta_wide", erase_prob=self.erase_prob,
                                          erase_scale=self.erase_scale, erase_ratio=self.erase_ratio,
                                          erase_ratio_table=ratios, seed=seed, epoch=epoch, params_in=params,
                                          chain_in=chain_params, erase_in=erase_params, params_out=used, chain_out=cused,
                                          erase_out=eused, index_base=base)
        out = (img, targets, used) if return_params else (img, targets)
        if return_chain_params or return_erase_params:
            out += self._extras((return_chain_params, cused, (B, CHAIN_MAX_OPS, 3)), (return_erase_params, eused, (B, 4)))
        return out


def resized_crop_policy_reference(img_u8, box, flip, size, chain, table, erase, mean, std):
    """One training sample of ``ResizedCropDataset(policy=, erase_prob=)`` restated on the CPU: fp32 ``[3,size,size]`` (a
    tensor).  It composes ``resample_reference(img_u8, box, (size, size))``, the horizontal flip, ``chain_reference`` under
    `chain` (a sequence of (op, bin, sign); Identity slots may be left in) and `table` (``chain_table(..., size, size)``),
    torch's CPU ``x.float().div(255).sub(mean).div(std)``, and the rectangle `erase` = (top, left, h, w) set to 0.0.  What
    nbdt_resized_crop_policy_batch computes.  Test infrastructure and documentation: it must not be called on the training
    path."""
    size = int(size)
    out = resample_reference(img_u8, box, (size, size))
    if flip:
        out = out[:, :, ::-1]
    out = chain_reference(np.ascontiguousarray(out), chain, table)
    mean = torch.tensor([float(m) for m in mean], dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor([float(s) for s in std], dtype=torch.float32).view(3, 1, 1)
    f = torch.from_numpy(np.ascontiguousarray(out)).float().div(255).sub(mean).div(std)
    t, l, h, w = (int(v) for v in erase)
    if not (0 <= t and 0 <= l and h >= 0 and w >= 0 and t + h <= size and l + w <= size):
        raise ValueError(f"erase {tuple(erase)} is not inside the {size} x {size} crop")
    f[:, t:t + h, l:l + w] = 0.0
    return f


# ---------------------------------------------------------------------------------------------------------------------
# TrivialAugmentWide and random erasing (nbdt_policy_batch, csrc/policy.hip): one of 14 operations per image at one of 31
# magnitudes, on the cropped and flipped uint8 image, with Pillow's pixel rules; then torchvision's RandomErasing(value=0)
# on the normalised output.  DeviceDataset(policy="ta_wide", erase_prob=p) switches them on.

POLICY_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
              "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")        # the kernel's order
POLICY_BINS = _C.NBDT_POLICY_BINS
POLICY_SIGNED = frozenset(range(1, 10))           # ShearX .. Sharpness draw a sign, the others ignore it
POLICY_MAX_BYTES = 49152                          # 3*H*W of a dataset the policy kernel takes (NBDT_AUGMENT_LDS_BYTES)
ERASE_SCALE, ERASE_RATIO = (0.02, 0.33), (0.3, 3.3)          # torchvision's RandomErasing defaults
_OP = {name: i for i, name in enumerate(POLICY_OPS)}
_K_POLICY, _K_ERASE = 0xA0761D6478BD642F, 0xE7037ED1A0B428DB     # odd: the policy's and the erase's hash of the index


def _fix(v):
    """Pillow's FIX(): 16.16 fixed point, floor(v * 65536 + 0.5) for a negative argument, truncation otherwise."""
    v = v * 65536.0 + 0.5
    return int(math.floor(v)) if v < 0.0 else int(v)


def _affine_fixed(a):
    """The six int32 of Pillow's nearest-neighbour affine transform for the fp64 matrix a[0..5] (affine_fixed): output pixel
    (x, y) reads source ((a2 + a0*x + a1*y) >> 16, (a5 + a3*x + a4*y) >> 16), returned in the order a0 .. a5."""
    return [_fix(a[0]), _fix(a[1]), _fix(a[2] + a[0] * 0.5 + a[1] * 0.5),
            _fix(a[3]), _fix(a[4]), _fix(a[5] + a[3] * 0.5 + a[4] * 0.5)]


def _rotate_fixed(angle, H, W):
    """Image.rotate(angle, NEAREST) as the six fixed-point coefficients: Pillow's matrix (entries rounded to 15 decimals,
    centre (W/2, H/2)) for the general case; angle 0 and, on a square image, the quarter turns are exact copies /
    transposes, which the same form expresses exactly."""
    angle = angle % 360.0
    if angle == 0.0:
        return _affine_fixed([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    if H == W and angle == 90.0:        # Transpose.ROTATE_90: out[y][x] = in[x][W-1-y]
        return [0, -65536, ((W - 1) << 16) + 32768, 65536, 0, 32768]
    if H == W and angle == 270.0:       # Transpose.ROTATE_270: out[y][x] = in[H-1-x][y]
        return [0, 65536, 32768, -65536, 0, ((H - 1) << 16) + 32768]
    cx, cy = W / 2, H / 2
    r = -math.radians(angle)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return _affine_fixed(m)


def _magnitude_table(nops, n, shear, tx, ty, rotate, enhance, posterize_steps, H, W):
    """int32 [nops, n, 2, 6]: per (op, bin, sign) the magnitude hi * b / (n - 1), formed in fp64, in the form the kernels
    consume.  shear, rotate (degrees), enhance: the `hi` of those ops; tx, ty: of TranslateX / TranslateY in pixels;
    Posterize drops round(b / ((n - 1) / posterize_steps)) bits.  Rows past Equalize (Invert) have no magnitude."""
    t = np.zeros((nops, n, 2, 6), dtype=np.int32)
    for b in range(n):
        for sg in (0, 1):
            s = -1.0 if sg else 1.0
            m = s * shear * b / (n - 1)
            t[_OP["ShearX"], b, sg] = _affine_fixed([1.0, m, 0.0, 0.0, 1.0, 0.0])
            t[_OP["ShearY"], b, sg] = _affine_fixed([1.0, 0.0, 0.0, m, 1.0, 0.0])
            px, py = int(s) * int(tx * b / (n - 1)), int(s) * int(ty * b / (n - 1))
            t[_OP["TranslateX"], b, sg] = [65536, 0, 32768 - px * 65536, 0, 65536, 32768]
            t[_OP["TranslateY"], b, sg] = [65536, 0, 32768, 0, 65536, 32768 - py * 65536]
            t[_OP["Rotate"], b, sg] = _rotate_fixed(s * rotate * b / (n - 1), H, W)
            factor = np.array([1 + s * enhance * b / (n - 1)], dtype=np.float64).astype(np.float32).view(np.int32)[0]
            for name in ("Brightness", "Color", "Contrast", "Sharpness"):
                t[_OP[name], b, sg, 0] = factor
            bits = 8 - round(b / ((n - 1) / posterize_steps))
            t[_OP["Posterize"], b, sg, 0] = 0xFF & ~((1 << (8 - bits)) - 1)
            t[_OP["Solarize"], b, sg, 0] = math.ceil(255 - 255 * b / (n - 1))      # v < threshold  <=>  v < ceil(threshold)
    t.setflags(write=False)
    return t


# TrivialAugmentWide's ranges over 31 bins
_TA_WIDE = dict(n=31, shear=0.99, tx=32, ty=32, rotate=135, enhance=0.99, posterize_steps=6)


@functools.lru_cache(maxsize=8)
def _policy_table(H, W):
    return _magnitude_table(len(POLICY_OPS), H=H, W=W, **_TA_WIDE)


def policy_table(H, W):
    """The int32 ``[14, 31, 2, 6]`` table nbdt_policy_batch reads for an H x W dataset: per (op, bin, sign) the magnitude in
    the form the kernel consumes, formed here in fp64 so that the device does no trigonometry and no rounding of its own.
    Geometric ops (ShearX/Y, TranslateX/Y, Rotate): Pillow's six 16.16 fixed-point affine coefficients a0 .. a5.
    Brightness / Color / Contrast / Sharpness: word 0 is the bits of float32(1 + s * 0.99 * b / 30).  Posterize: word 0 is
    the byte mask.  Solarize: word 0 is ceil(255 - 255 * b / 30).  The other words, and the other ops' rows, are 0."""
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"image sides must be 1..{MAX_SIDE}, got {H} x {W}")
    return _policy_table(H, W)


def _check_erase(erase_prob, erase_scale, erase_ratio):
    p = float(erase_prob)
    if not 0.0 <= p <= 1.0:            # (NaN fails both comparisons)
        raise ValueError(f"erase_prob must be in [0, 1], got {erase_prob}")
    _check_ranges(erase_scale, erase_ratio)
    return p


def draw_policy_params(seed, epoch, index, H, W, erase_prob=0.0, erase_scale=ERASE_SCALE, erase_ratio=ERASE_RATIO):
    """The policy and erase draw of nbdt_policy_batch (include/nbdt_hip.h), restated with numpy: (op, bin, sign, top, left,
    h, w) int64 arrays shaped like `index`; h = w = 0 means no erase.  A pure function of (seed, epoch, dataset index) and
    the settings; the crop and flip of the same sample stay ``draw_params``.

    TrivialAugmentWide: op uniform in 0..13 (POLICY_OPS), bin uniform in 0..30, sign in {0, 1} (1: negative magnitude).
    RandomErasing: applied when a uniform [0, 1) draw is below erase_prob; then up to 10 attempts of (area fraction
    uniform in erase_scale, aspect ratio from ``ratio_table(erase_ratio)``, h = round(sqrt(area * r)),
    w = round(sqrt(area / r)), accepted if h < H and w < W, position uniform); nothing is erased if none is accepted."""
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"image sides must be 1..{MAX_SIDE}, got {H} x {W}")
    p = _check_erase(erase_prob, erase_scale, erase_ratio)
    s0, s1 = float(erase_scale[0]), float(erase_scale[1])
    table = ratio_table(erase_ratio)
    if isinstance(index, torch.Tensor):
        index = index.cpu().numpy()
    idx = np.asarray(index).astype(np.int64).astype(np.uint64)
    u64 = np.uint64
    m24, golden = u64(0xFFFFFF), 0x9E3779B97F4A7C15
    with np.errstate(over="ignore"):
        key = _mix64(np.asarray([(int(seed) * golden + int(epoch)) & _M64], dtype=np.uint64))[0]
        rp = _mix64(key ^ (idx * u64(_K_POLICY)))
        re = _mix64(key ^ (idx * u64(_K_ERASE)))
        op = (((rp & m24) * u64(len(POLICY_OPS))) >> u64(24)).astype(np.int64)
        bin_ = ((((rp >> u64(24)) & m24) * u64(POLICY_BINS)) >> u64(24)).astype(np.int64)
        sign = (rp >> u64(63)).astype(np.int64)
        top, left = np.zeros(idx.shape, dtype=np.int64), np.zeros(idx.shape, dtype=np.int64)
        h, w = np.zeros(idx.shape, dtype=np.int64), np.zeros(idx.shape, dtype=np.int64)
        apply = (re >> u64(11)).astype(np.float64) * 2.0 ** -53 < p
        for t in reversed(range(_C.NBDT_RESIZED_CROP_ATTEMPTS)):      # the earliest accepted attempt is written last
            ra = _mix64(re + u64(((2 * t + 1) * golden) & _M64))
            rb = _mix64(re + u64(((2 * t + 2) * golden) & _M64))
            u = (ra >> u64(11)).astype(np.float64) * 2.0 ** -53
            target = float(H * W) * (s0 + u * (s1 - s0))
            r = table[(rb & u64(_C.NBDT_RESIZED_CROP_RATIOS - 1)).astype(np.int64)]
            ch, cw = _round_sqrt(target * r), _round_sqrt(target / r)
            ok = apply & (ch < H) & (cw < W)
            ct = (((rb >> u64(12)) & m24) * np.clip(H - ch + 1, 0, None).astype(np.uint64)) >> u64(24)
            cl = (((rb >> u64(36)) & m24) * np.clip(W - cw + 1, 0, None).astype(np.uint64)) >> u64(24)
            top, left = np.where(ok, ct.astype(np.int64), top), np.where(ok, cl.astype(np.int64), left)
            h, w = np.where(ok, ch, h), np.where(ok, cw, w)
    empty = (h == 0) | (w == 0)                  # an accepted rectangle with a side that rounded to 0 erases nothing
    zero = np.zeros_like(h)
    return (op, bin_, sign, np.where(empty, zero, top), np.where(empty, zero, left), np.where(empty, zero, h),
            np.where(empty, zero, w))


def _grey(img):
    i = img.astype(np.int64)
    return (19595 * i[0] + 38470 * i[1] + 7471 * i[2] + 32768) >> 16


def _blend(deg, img, factor):
    """Pillow's Image.blend(degenerate, image, factor) on 8-bit data: fp32 d + a * (x - d), a separate multiply and add,
    then 0 at or below 0, 255 at or above 255, else truncated."""
    a = np.float32(factor)
    d, x = deg.astype(np.float32), img.astype(np.float32)
    t = d + a * (x - d)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def policy_reference(img_u8_chw, op, bin, sign):
    """One TrivialAugmentWide operation on one uint8 ``[3,H,W]`` image (an array or a CPU tensor), restated with numpy from
    Pillow's rules (include/nbdt_hip.h lists them); returns a uint8 array.  op: an index into POLICY_OPS or a name; bin:
    0..30; sign: 0 or 1 (1: negative magnitude; ignored by the unsigned ops).  What nbdt_policy_batch computes between the
    flip and the normalisation.  Test infrastructure and documentation: it must not be called on the training path."""
    if isinstance(img_u8_chw, torch.Tensor):
        img_u8_chw = img_u8_chw.cpu().numpy()
    img = np.asarray(img_u8_chw)
    if img.ndim != 3 or img.shape[0] != 3 or img.dtype != np.uint8:
        raise ValueError(f"img must be uint8 [3,H,W], got {img.dtype} {img.shape}")
    op = _OP[op] if isinstance(op, str) else int(op)
    b, sg = int(bin), int(sign)
    if not (0 <= op < len(POLICY_OPS) and 0 <= b < POLICY_BINS and sg in (0, 1)):
        raise ValueError(f"need op in 0..{len(POLICY_OPS) - 1}, bin in 0..{POLICY_BINS - 1}, sign in {{0, 1}}; got "
                         f"({op}, {b}, {sg})")
    _, H, W = img.shape
    return _apply_op(img, POLICY_OPS[op], policy_table(H, W)[op, b, sg].astype(np.int64))


def _apply_op(img, name, row):
    """Operation `name` on a uint8 [3,H,W] array under the six int64 words `row` of its magnitude table."""
    _, H, W = img.shape
    if name == "Identity":
        return img.copy()
    if name == "Invert":
        return (255 - img).astype(np.uint8)
    if name in ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"):
        y, x = np.mgrid[0:H, 0:W].astype(np.int64)
        sx = (row[2] + row[0] * x + row[1] * y) >> 16
        sy = (row[5] + row[3] * x + row[4] * y) >> 16
        inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        out = img[:, np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)]
        return np.where(inside[None], out, 0).astype(np.uint8)
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        factor = np.array([row[0]], dtype=np.int32).view(np.float32)[0]
        if name == "Brightness":
            deg = np.zeros_like(img)
        elif name == "Color":
            deg = np.broadcast_to(_grey(img)[None], img.shape)
        elif name == "Contrast":
            g = _grey(img)
            deg = np.full_like(img, int(float(g.sum()) / g.size + 0.5))
        else:       # ImageFilter.SMOOTH: (1 1 1; 1 5 1; 1 1 1) / 13, the one-pixel border copied
            i = img.astype(np.int64)
            deg = i.copy()
            if H >= 3 and W >= 3:
                s = 4 * i[:, 1:-1, 1:-1]
                for dy in (0, 1, 2):
                    for dx in (0, 1, 2):
                        s = s + i[:, dy:H - 2 + dy, dx:W - 2 + dx]
                deg[:, 1:-1, 1:-1] = (2 * s + 13) // 26              # trunc(s / 13 + 0.5)
        return _blend(deg, img, factor)
    if name == "Posterize":
        return img & np.uint8(row[0])
    if name == "Solarize":
        return np.where(img.astype(np.int64) < row[0], img, 255 - img).astype(np.uint8)
    out = img.copy()
    for c in range(3):
        ch = img[c]
        hist = np.bincount(ch.ravel(), minlength=256).astype(np.int64)
        lo, hi = int(ch.min()), int(ch.max())
        if hi <= lo:
            continue
        if name == "AutoContrast":
            scale = 255.0 / (hi - lo)
            offset = -lo * scale
            lut = np.clip((np.arange(256, dtype=np.float64) * scale + offset).astype(np.int64), 0, 255)
        else:       # Equalize
            step = (int(hist.sum()) - int(hist[hi])) // 255
            if step == 0:
                continue
            before = np.concatenate([[0], np.cumsum(hist)[:-1]])
            lut = np.minimum(255, (step // 2 + before) // step)
        out[c] = lut[ch].astype(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# RandAugment and AutoAugment (nbdt_policy_chain_batch, csrc/policy.hip): a chain of up to four operations per image, each
# under the pixel rules above, plus Invert.  DeviceDataset(policy="ra" | "cifar10" | <list of sub-policies>).

CHAIN_OPS = POLICY_OPS + ("Invert",)
CHAIN_MAX_OPS = _C.NBDT_CHAIN_MAX_OPS
CHAIN_SIGNED = POLICY_SIGNED
_CHAIN_NO_MAGNITUDE = frozenset(("Identity", "AutoContrast", "Equalize", "Invert"))
_CHAIN_OP = {name: i for i, name in enumerate(CHAIN_OPS)}
_K_CHAIN = 0x8EBC6AF09C88C6E3           # odd: the chain's hash of the index
RA_BINS, AA_BINS = 31, 10               # torchvision's RandAugment(num_magnitude_bins=31), AutoAugment's 10
# torchvision's _augmentation_space of RandAugment and AutoAugment; the translations are fractions of the image side
_RA_RANGES = dict(shear=0.3, rotate=30.0, enhance=0.9, posterize_steps=4)
_TRANSLATE = 150.0 / 331.0

# AutoAugment's CIFAR-10 policy (Cubuk et al. 2019, as torchvision lists it): 25 sub-policies of two (op, p, bin) slots
CIFAR10_POLICY = (
    (("Invert", 0.1, None), ("Contrast", 0.2, 6)), (("Rotate", 0.7, 2), ("TranslateX", 0.3, 9)),
    (("Sharpness", 0.8, 1), ("Sharpness", 0.9, 3)), (("ShearY", 0.5, 8), ("TranslateY", 0.7, 9)),
    (("AutoContrast", 0.5, None), ("Equalize", 0.9, None)), (("ShearY", 0.2, 7), ("Posterize", 0.3, 7)),
    (("Color", 0.4, 3), ("Brightness", 0.6, 7)), (("Sharpness", 0.3, 9), ("Brightness", 0.7, 9)),
    (("Equalize", 0.6, None), ("Equalize", 0.5, None)), (("Contrast", 0.6, 7), ("Sharpness", 0.6, 5)),
    (("Color", 0.7, 7), ("TranslateX", 0.5, 8)), (("Equalize", 0.3, None), ("AutoContrast", 0.4, None)),
    (("TranslateY", 0.4, 3), ("Sharpness", 0.2, 6)), (("Brightness", 0.9, 6), ("Color", 0.2, 8)),
    (("Solarize", 0.5, 2), ("Invert", 0.0, None)), (("Equalize", 0.2, None), ("AutoContrast", 0.6, None)),
    (("Equalize", 0.2, None), ("Equalize", 0.6, None)), (("Color", 0.9, 9), ("Equalize", 0.6, None)),
    (("AutoContrast", 0.8, None), ("Solarize", 0.2, 8)), (("Brightness", 0.1, 3), ("Color", 0.7, 0)),
    (("Solarize", 0.4, 5), ("AutoContrast", 0.9, None)), (("TranslateY", 0.9, 9), ("TranslateY", 0.7, 9)),
    (("AutoContrast", 0.9, None), ("Solarize", 0.8, 3)), (("Equalize", 0.8, None), ("Invert", 0.1, None)),
    (("TranslateY", 0.7, 9), ("AutoContrast", 0.9, None)),
)

# AutoAugment's ImageNet policy: 25 sub-policies in the order torchvision lists them.  Written down from memory; no copy of
# torchvision or of the paper's table was at hand to check it against (DESIGN.md section 20 says so too).
IMAGENET_POLICY = (
    (("Posterize", 0.4, 8), ("Rotate", 0.6, 9)), (("Solarize", 0.6, 5), ("AutoContrast", 0.6, None)),
    (("Equalize", 0.8, None), ("Equalize", 0.6, None)), (("Posterize", 0.6, 7), ("Posterize", 0.6, 6)),
    (("Equalize", 0.4, None), ("Solarize", 0.2, 4)), (("Equalize", 0.4, None), ("Rotate", 0.8, 8)),
    (("Solarize", 0.6, 3), ("Equalize", 0.6, None)), (("Posterize", 0.8, 5), ("Equalize", 1.0, None)),
    (("Rotate", 0.2, 3), ("Solarize", 0.6, 8)), (("Equalize", 0.6, None), ("Posterize", 0.4, 6)),
    (("Rotate", 0.8, 8), ("Color", 0.4, 0)), (("Rotate", 0.4, 9), ("Equalize", 0.6, None)),
    (("Equalize", 0.0, None), ("Equalize", 0.8, None)), (("Invert", 0.6, None), ("Equalize", 1.0, None)),
    (("Color", 0.6, 4), ("Contrast", 1.0, 8)), (("Rotate", 0.8, 8), ("Color", 1.0, 2)),
    (("Color", 0.8, 8), ("Solarize", 0.8, 7)), (("Sharpness", 0.4, 7), ("Invert", 0.6, None)),
    (("ShearX", 0.6, 5), ("Equalize", 1.0, None)), (("Color", 0.4, 0), ("Equalize", 0.6, None)),
    (("Equalize", 0.4, None), ("Solarize", 0.2, 4)), (("Solarize", 0.6, 5), ("AutoContrast", 0.6, None)),
    (("Invert", 0.6, None), ("Equalize", 1.0, None)), (("Color", 0.6, 4), ("Contrast", 1.0, 8)),
    (("Equalize", 0.8, None), ("Equalize", 0.6, None)),
)
_NAMED_POLICIES = {"cifar10": CIFAR10_POLICY, "imagenet": IMAGENET_POLICY}


def subpolicy_array(policy):
    """The int32 ``[P, 4, 3]`` of (op, q = round(p * 2^24), bin) nbdt_policy_chain_batch reads for ``"cifar10"``,
    ``"imagenet"`` or a list of sub-policies, each a sequence of 1..4 slots ``(op name, p, bin)`` with bin None (or 0) for an
    op without a magnitude; an unused slot is (0, 0, 0).  ValueError naming the slot for an unknown op, p outside [0, 1], a
    bin outside 0..9 or a sub-policy without slots or with more than four."""
    subs = _NAMED_POLICIES.get(policy, policy) if isinstance(policy, str) else policy
    if isinstance(subs, str) or not isinstance(subs, (list, tuple)) or not 1 <= len(subs) <= _C.NBDT_CHAIN_MAX_SUBPOLICIES:
        raise ValueError(f"a policy is 'cifar10', 'imagenet' or a list of 1..{_C.NBDT_CHAIN_MAX_SUBPOLICIES} sub-policies, "
                         f"got {policy!r}")
    out = np.zeros((len(subs), CHAIN_MAX_OPS, 3), dtype=np.int32)
    for i, sub in enumerate(subs):
        if not isinstance(sub, (list, tuple)) or not 1 <= len(sub) <= CHAIN_MAX_OPS:
            raise ValueError(f"sub-policy {i} must have 1..{CHAIN_MAX_OPS} slots (op, p, bin), got {sub!r}")
        for k, slot in enumerate(sub):
            where = f"sub-policy {i} slot {k} {slot!r}"
            if not isinstance(slot, (list, tuple)) or len(slot) != 3:
                raise ValueError(f"{where}: a slot is (op name, p, bin)")
            name, p, b = slot
            if name not in _CHAIN_OP:
                raise ValueError(f"{where}: unknown op {name!r} (one of {', '.join(CHAIN_OPS)})")
            try:
                p = float(p)
            except (TypeError, ValueError):
                p = float("nan")
            if not 0.0 <= p <= 1.0:
                raise ValueError(f"{where}: p must be in [0, 1]")
            b = 0 if b is None else b
            if not isinstance(b, (int, np.integer)) or isinstance(b, bool) or not 0 <= b < AA_BINS:
                raise ValueError(f"{where}: bin must be an integer in 0..{AA_BINS - 1} (None for an op without a magnitude)")
            if name in _CHAIN_NO_MAGNITUDE:
                b = 0
            out[i, k] = (_CHAIN_OP[name], round(p * 2 ** 24), int(b))
    return out


def _chain_bins(policy):
    if isinstance(policy, str) and policy in ("ra", "ta_wide"):
        return RA_BINS
    if isinstance(policy, str) and policy not in _NAMED_POLICIES:
        raise ValueError(f"policy must be 'ra', 'cifar10', 'imagenet', 'ta_wide' or a list of sub-policies, got {policy!r}")
    return AA_BINS


@functools.lru_cache(maxsize=16)
def _chain_table(n, ta_wide, H, W):
    if ta_wide:
        return _magnitude_table(len(CHAIN_OPS), H=H, W=W, **_TA_WIDE)
    return _magnitude_table(len(CHAIN_OPS), n, tx=_TRANSLATE * W, ty=_TRANSLATE * H, H=H, W=W, **_RA_RANGES)


def chain_table(policy, H, W):
    """The int32 ``[15, n, 2, 6]`` table nbdt_policy_chain_batch reads for an H x W dataset, rows in the form of
    ``policy_table``.  policy "ra": RandAugment's space over n = 31 bins; "cifar10" or a list of sub-policies:
    AutoAugment's over n = 10; each magnitude is hi * b / (n - 1) in fp64 with hi = 0.3 (shear), (150 / 331) * side
    (translation, truncated to whole pixels), 30 degrees, 0.9 (the four enhancements), Posterize to
    8 - round(b / ((n - 1) / 4)) bits, Solarize below 255 - 255 * b / (n - 1).  "ta_wide": TrivialAugmentWide's ranges
    (``policy_table``'s rows, and Invert's) -- a chain of one op on it is nbdt_policy_batch.  A table belongs to a space of
    magnitudes, not to a list of sub-policies: AutoAugment's ImageNet policy reads the table "cifar10" names, and
    ``chain_table("imagenet", ...)`` is a ValueError saying so."""
    if isinstance(policy, str) and policy == "imagenet":
        raise ValueError("AutoAugment has one magnitude space for all its policies: the table of policy 'imagenet' is "
                         "chain_table('cifar10', H, W)")
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"image sides must be 1..{MAX_SIDE}, got {H} x {W}")
    return _chain_table(_chain_bins(policy), isinstance(policy, str) and policy == "ta_wide", H, W)


def _check_ra(num_ops, magnitude):
    if not (isinstance(num_ops, (int, np.integer)) and 1 <= num_ops <= CHAIN_MAX_OPS):
        raise ValueError(f"RandAugment's num_ops must be 1..{CHAIN_MAX_OPS}, got {num_ops!r}")
    if not (isinstance(magnitude, (int, np.integer)) and 0 <= magnitude < RA_BINS):
        raise ValueError(f"RandAugment's magnitude must be 0..{RA_BINS - 1}, got {magnitude!r}")
    return int(num_ops), int(magnitude)


def draw_chain_params(seed, epoch, index, policy="ra", num_ops=2, magnitude=9, return_subpolicy=False):
    """The chain's draw of nbdt_policy_chain_batch (include/nbdt_hip.h), restated with numpy: int64 ``[B, 4, 3]`` of (op,
    bin, sign) per slot, sign 1 meaning a negative magnitude; a skipped or unused slot is Identity (0, 0, 0).  A pure
    function of (seed, epoch, dataset index) and the settings; the crop, the flip and the erase rectangle of the same
    sample stay ``draw_params`` and ``draw_policy_params``.

    policy "ra": each of `num_ops` slots gets an op uniform in 0..13, bin `magnitude` and a fresh sign.  "cifar10" or a
    list of sub-policies: one sub-policy uniformly; its slot (op, p, bin) is applied when a 24-bit uniform is below
    round(p * 2^24), with a fresh sign.  return_subpolicy appends the int64 [B] sub-policy chosen (0 for "ra")."""
    if isinstance(index, torch.Tensor):
        index = index.cpu().numpy()
    idx = np.asarray(index).astype(np.int64).astype(np.uint64).reshape(-1)
    u64 = np.uint64
    m24, golden = u64(0xFFFFFF), 0x9E3779B97F4A7C15
    out = np.zeros((idx.shape[0], CHAIN_MAX_OPS, 3), dtype=np.int64)
    if isinstance(policy, str) and policy == "ra":
        num_ops, magnitude = _check_ra(num_ops, magnitude)
        subs = None
    else:
        subs = subpolicy_array(policy).astype(np.int64)
    with np.errstate(over="ignore"):
        key = _mix64(np.asarray([(int(seed) * golden + int(epoch)) & _M64], dtype=np.uint64))[0]
        rc = _mix64(key ^ (idx * u64(_K_CHAIN)))
        which = np.zeros(idx.shape, dtype=np.int64) if subs is None else \
            (((rc & m24) * u64(len(subs))) >> u64(24)).astype(np.int64)
        for k in range(CHAIN_MAX_OPS if subs is not None else num_ops):
            rs = _mix64(rc + u64(((k + 1) * golden) & _M64))
            bit = (rs >> u64(63)).astype(np.int64)
            if subs is None:
                out[:, k, 0] = (((rs & m24) * u64(len(POLICY_OPS))) >> u64(24)).astype(np.int64)
                out[:, k, 1] = magnitude
                out[:, k, 2] = bit
            else:
                slot = subs[which, k]                               # [B, 3] (op, q, bin)
                applied = (rs & m24).astype(np.int64) < slot[:, 1]
                out[:, k, 0] = np.where(applied, slot[:, 0], 0)
                out[:, k, 1] = np.where(applied, slot[:, 2], 0)
                out[:, k, 2] = np.where(applied, 1 - bit, 0)
    return (out, which) if return_subpolicy else out


def chain_reference(img_u8_chw, chain, table):
    """The operations `chain` -- a sequence of (op, bin, sign), op an index into CHAIN_OPS or a name -- applied one after
    the other to one uint8 ``[3,H,W]`` image under the magnitudes of `table` (``chain_table``), each by the rules
    ``policy_reference`` restates from Pillow, Invert being 255 - v; returns a uint8 array.  What nbdt_policy_chain_batch
    computes between the flip and the normalisation.  Test infrastructure and documentation: it must not be called on the
    training path."""
    if isinstance(img_u8_chw, torch.Tensor):
        img_u8_chw = img_u8_chw.cpu().numpy()
    img = np.asarray(img_u8_chw)
    if img.ndim != 3 or img.shape[0] != 3 or img.dtype != np.uint8:
        raise ValueError(f"img must be uint8 [3,H,W], got {img.dtype} {img.shape}")
    table = np.asarray(table)
    if table.ndim != 4 or table.shape[0] != len(CHAIN_OPS) or table.shape[2:] != (2, 6):
        raise ValueError(f"table must be [15, n, 2, 6] (chain_table), got {table.shape}")
    out = img.copy()
    for slot in chain:
        op, b, sg = slot
        op = _CHAIN_OP[op] if isinstance(op, str) else int(op)
        b, sg = int(b), int(sg)
        if not (0 <= op < len(CHAIN_OPS) and 0 <= b < table.shape[1] and sg in (0, 1)):
            raise ValueError(f"need op in 0..{len(CHAIN_OPS) - 1}, bin in 0..{table.shape[1] - 1}, sign in {{0, 1}}; got "
                             f"({op}, {b}, {sg})")
        out = _apply_op(np.ascontiguousarray(out), CHAIN_OPS[op], table[op, b, sg].astype(np.int64))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# MixUp / CutMix (torchvision.transforms.v2.MixUp / CutMix; the soft-label transforms of the reference's ImageNet example):
# one draw per step on the host, one launch (nbdt_mix_batch, csrc/mix.hip) for the images and the probability targets.

def draw_mix(seed, epoch, step, H, W, mixup_alpha=0.0, cutmix_alpha=0.0):
    """The mixing of one training step, or None when both alphas are 0: a dict with ``mode`` ("mixup" | "cutmix"),
    ``lam`` (the draw, Beta(alpha, alpha), one per batch), ``box`` = (y1, y2, x1, x2) and ``lam_t``, the weight of a
    sample's own label.  A pure function of its arguments (numpy's default_rng([seed, epoch, step])), so every rank of a
    run draws the same mixing without talking to the others.

    MixUp: an empty box, lam_t = lam.  CutMix, as in torchvision: the box's centre is uniform over the pixels, its half
    sides are int(0.5*sqrt(1 - lam)*H) and int(0.5*sqrt(1 - lam)*W), it is clipped to the image and
    lam_t = 1 - area / (H*W).  With both alphas > 0 one fair coin per step picks the mode."""
    mixup_alpha, cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
    if mixup_alpha < 0 or cutmix_alpha < 0:
        raise ValueError(f"mixup_alpha and cutmix_alpha must be >= 0, got {mixup_alpha}, {cutmix_alpha}")
    if mixup_alpha == 0 and cutmix_alpha == 0:
        return None
    H, W = int(H), int(W)
    rng = np.random.default_rng([int(seed), int(epoch), int(step)])
    if mixup_alpha > 0 and cutmix_alpha > 0:
        cut = bool(rng.integers(2))
    else:
        cut = cutmix_alpha > 0
    alpha = cutmix_alpha if cut else mixup_alpha
    lam = float(rng.beta(alpha, alpha))
    if not cut:
        return {"mode": "mixup", "lam": lam, "box": (0, 0, 0, 0), "lam_t": lam}
    r_y, r_x = int(rng.integers(H)), int(rng.integers(W))
    r = 0.5 * math.sqrt(1.0 - lam)
    half_h, half_w = int(r * H), int(r * W)
    y1, y2 = max(r_y - half_h, 0), min(r_y + half_h, H)
    x1, x2 = max(r_x - half_w, 0), min(r_x + half_w, W)
    return {"mode": "cutmix", "lam": lam, "box": (y1, y2, x1, x2), "lam_t": 1.0 - (y2 - y1) * (x2 - x1) / float(H * W)}


def mix_batch(img, targets, num_classes, draw):
    """(mixed images [B,3,H,W], probability targets [B, num_classes] fp32) of a training batch under ``draw``
    (draw_mix): every sample is paired with its predecessor in the batch (the batch rolled by one).  One launch, freshly
    allocated outputs; ``img`` and ``targets`` are left as they are."""
    out = torch.empty_like(img)
    tgt = torch.empty((img.shape[0], int(num_classes)), dtype=torch.float32, device=img.device)
    if draw["mode"] == "cutmix":
        ops.mix_batch(img, targets, out, tgt, lam=1.0, box=draw["box"], lam_t=draw["lam_t"])
    else:
        ops.mix_batch(img, targets, out, tgt, lam=draw["lam"], box=(0, 0, 0, 0), lam_t=draw["lam_t"])
    return out, tgt
