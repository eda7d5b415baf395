"""What tests/test_upsampled_xent.py and tests/test_upsampled_xent_gpu.py share: a numpy transcription of the bilinear
interpolation contract of csrc/upsample_taps.h (torch's, ATen UpSample.h, in fp32), the shape pairs of the two files,
seeded inputs, and the yardstick -- torch's own composition F.cross_entropy(F.interpolate(...)) in float64 on the CPU
with autograd."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
IGNORE = 255

# (in, out) per axis: every tap clamped; integer scale; non-integer scale; one axis only; a larger integer scale
PAIRS = (((1, 1), (3, 5)), ((3, 4), (12, 16)), ((5, 7), (17, 23)), ((2, 3), (2, 9)), ((8, 8), (32, 32)))
AXES = tuple(sorted({(i, o) for (h, w), (H, W) in PAIRS for i, o in ((h, H), (w, W))} | {(7, 7)}))
# the stand-alone cases of the GPU file: (index into PAIRS, classes, align_corners) x KINDS
CASES = [(pair, C, ac) for pair in range(4) for C in (5, 40) for ac in (False, True)] + [(2, 19, False), (2, 19, True)]
KINDS = ("plain", "smoothing", "weight")


def scale_of(n_in, n_out, align_corners):
    if align_corners:
        return F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    return F32(n_in) / F32(n_out)


def taps(n_in, n_out, align_corners, dst):
    """(i0, i1, l0, l1) of one destination index, every operation a single fp32 rounding."""
    scale = scale_of(n_in, n_out, align_corners)
    if align_corners:
        src = F32(scale * F32(dst))
    else:
        src = F32(F32(scale * F32(F32(dst) + F32(0.5))) - F32(0.5))
        if src < 0:
            src = F32(0)
    i0 = int(src)
    i1 = i0 + (1 if i0 < n_in - 1 else 0)
    l1 = F32(src - F32(i0))
    return i0, i1, F32(F32(1) - l1), l1


def matrix(n_in, n_out, align_corners, taps_fn=taps):
    """A [n_out, n_in] float64: row dst holds the weights destination dst takes from every source index (the clamped
    borders, i0 == i1, add up)."""
    A = np.zeros((n_out, n_in), dtype=np.float64)
    for d in range(n_out):
        i0, i1, l0, l1 = taps_fn(n_in, n_out, align_corners, d)
        A[d, i0] += float(l0)
        A[d, i1] += float(l1)
    return A


def torch_matrix(n_in, n_out, align_corners):
    """The same matrix from F.interpolate of an identity basis in float64 (one axis: a [n_in, 1, n_in, 1] batch)."""
    eye = torch.eye(n_in, dtype=torch.float64).view(n_in, 1, n_in, 1)
    out = F.interpolate(eye, size=(n_out, 1), mode="bilinear", align_corners=align_corners)
    return out.view(n_in, n_out).t().contiguous().numpy()


# ------------------------------------------------------------------------------------------------ inputs, yardstick

def logits(N, C, h, w, seed, sliced=False):
    """2 * randn; sliced: a channel-sliced view of a tensor two channels wider."""
    g = torch.Generator().manual_seed(seed)
    if sliced:
        return (2.0 * torch.randn(N, C + 2, h, w, generator=g))[:, 1:C + 1]
    return 2.0 * torch.randn(N, C, h, w, generator=g)


def on_device(x, device):
    """A channel-sliced view moved as the view it is: the wider tensor goes to the device, then the slice is taken."""
    if x._base is None:
        return x.to(device)
    return x._base.to(device)[:, 1:1 + x.shape[1]]


def targets(N, C, H, W, seed, ignored_image=None):
    """Class indices with 30 % ignored labels and pixel 0 valid; ignored_image: one image with no valid pixel."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (N, H, W), generator=g)
    y[torch.rand(y.shape, generator=g) < 0.3] = IGNORE
    y.view(-1)[0] = 0
    if ignored_image is not None:
        y[ignored_image] = IGNORE
    return y


def class_weights(C, seed):
    return 0.5 + 1.5 * torch.rand(C, generator=torch.Generator().manual_seed(seed))


def composition(x, y, align_corners, weight=None, smoothing=0.0, ignore=IGNORE, dtype=torch.float64):
    """(loss, dloss/dx) of torch's composition on the CPU in `dtype`, by autograd."""
    x = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    up = x if tuple(x.shape[2:]) == tuple(y.shape[1:]) else F.interpolate(x, size=tuple(y.shape[1:]), mode="bilinear",
                                                                          align_corners=align_corners)
    loss = F.cross_entropy(up, y.cpu(), None if weight is None else weight.cpu().to(dtype), ignore_index=ignore,
                           label_smoothing=smoothing)
    loss.backward()
    return loss.item(), x.grad.numpy()


def gather_form(x, y, align_corners, taps_fn, weight=None, smoothing=0.0, ignore=IGNORE):
    """(loss, dloss/dx) in float64 the way the kernels are laid out, from the taps of `taps_fn` alone: v = Ay x Ax^T per
    plane, f = coef * softmax(v) - t' at the valid pixels, dx = Ay^T f Ax over the divisor.  With the library's taps this
    is the adjoint of the library's own interpolation matrix applied to a float64 f."""
    x = x.detach().cpu().double().numpy()
    y = y.cpu().numpy()
    N, C, h, w = x.shape
    H, W = y.shape[1:]
    Ay, Ax = matrix(h, H, align_corners, taps_fn), matrix(w, W, align_corners, taps_fn)
    v = np.einsum("Yi,ncij,Xj->ncYX", Ay, x, Ax)
    valid = y != ignore
    yc = np.where(valid, y, 0)
    onehot = (np.arange(C)[None, :, None, None] == yc[:, None]).astype(np.float64)
    coef = np.ones(y.shape) if weight is None else weight.double().numpy()[yc]
    tprime = (1.0 - smoothing) * coef[:, None] * onehot + smoothing / C
    m = v.max(axis=1, keepdims=True)
    lse = np.log(np.exp(v - m).sum(axis=1, keepdims=True)) + m
    rows = coef * lse[:, 0] - (tprime * v).sum(axis=1)
    divisor = (coef * valid).sum()
    f = (coef[:, None] * np.exp(v - lse) - tprime) * valid[:, None]
    dx = np.einsum("Yi,ncYX,Xj->ncij", Ay, f, Ax) / divisor
    return (rows * valid).sum() / divisor, dx


@functools.lru_cache(maxsize=None)
def standalone_case(pair, C, align_corners, kind):
    """One case of the stand-alone criterion, computed once and shared: (x [2, C, h, w] a channel-sliced view, y whose
    second image is ignored altogether in the odd pairs, weight or None, smoothing, float64 loss, float64 dx)."""
    (h, w), (H, W) = PAIRS[pair]
    seed = 1000 * pair + 10 * C + int(align_corners)
    x = logits(2, C, h, w, seed, sliced=True)
    y = targets(2, C, H, W, seed + 1, ignored_image=1 if pair % 2 else None)
    weight = class_weights(C, seed + 2) if kind == "weight" else None
    smoothing = 0.1 if kind == "smoothing" else 0.0
    loss, dx = composition(x, y, align_corners, weight, smoothing)
    return x, y, weight, smoothing, loss, dx
