"""nbdt_mix_batch on the MI355X against plain torch on the CPU, bit for bit: MixUp is
x.mul(lam32).add(x.roll(1, 0).mul(oml32)), CutMix is slice assignment from the rolled batch, and the targets are
onehot.mul(lam_t32).add(onehot.roll(1, 0).mul(omlt32))."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from nbdt import _C, ops  # noqa: E402
from nbdt import data as D  # noqa: E402

DEV = "cuda:0"
# W % 4 == 0 (8 x 8, 32 x 20, 32 x 32) takes the 16-byte kernel on torch's aligned allocations -- 32 x 20 with box edges
# that are no multiple of 4, so the box cuts through a group of four; W % 4 != 0 (8 x 6, 32 x 30) takes the scalar kernel
SHAPES = [(8, 8), (32, 20), (32, 32), (8, 6), (32, 30)]


def f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def make(B, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, H, W, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    return x, y


def target_reference(y, C, lam_t):
    onehot = torch.nn.functional.one_hot(y, C).float()
    return onehot.mul(f32(lam_t)).add(onehot.roll(1, 0).mul(f32(1.0 - float(lam_t))))


def run(x, y, C, draw):
    out, tgt = D.mix_batch(x.to(DEV), y.to(DEV), C, draw)
    return out.cpu(), tgt.cpu()


@pytest.mark.parametrize("C", [10, 1000])
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("B", [1, 5, 64])
def test_mixup(B, H, W, C):
    x, y = make(B, H, W, C, B + H + W + C)
    for lam in (0.3, 0.9371, 1.0, 0.0):
        out, tgt = run(x, y, C, {"mode": "mixup", "lam": lam, "box": (0, 0, 0, 0), "lam_t": lam})
        want = x.mul(f32(lam)).add(x.roll(1, 0).mul(f32(1.0 - lam)))
        assert torch.equal(out, want), lam
        assert torch.equal(tgt, target_reference(y, C, lam)), lam


def boxes(H, W):
    return {"empty": (3, 3, 2, 6), "empty-x": (1, 5, 4, 4), "whole": (0, H, 0, W), "top-left": (0, 3, 0, 5),
            "bottom-right": (H - 3, H, W - 5, W), "left": (2, H - 1, 0, 3), "right": (1, 4, W - 2, W),
            "top": (0, 2, 1, W - 1), "bottom": (H - 1, H, 3, W - 2), "inner-odd": (2, 6, 1, min(7, W)),
            "one-pixel": (4, 5, 5, 6)}


@pytest.mark.parametrize("C", [10, 1000])
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("B", [1, 5, 64])
def test_cutmix(B, H, W, C):
    x, y = make(B, H, W, C, 2 * B + H + W + C)
    if B > 1:
        y[1] = y[0]                                  # a partner with the same label: its row is lam_t + (1 - lam_t)
    for name, (y1, y2, x1, x2) in boxes(H, W).items():
        lam_t = 1.0 - (y2 - y1) * (x2 - x1) / float(H * W)
        out, tgt = run(x, y, C, {"mode": "cutmix", "lam": 0.5, "box": (y1, y2, x1, x2), "lam_t": lam_t})
        want = x.clone()
        want[:, :, y1:y2, x1:x2] = x.roll(1, 0)[:, :, y1:y2, x1:x2]
        assert torch.equal(out, want), name
        assert torch.equal(tgt, target_reference(y, C, lam_t)), name


def test_drawn_mixing_matches_torch():
    """The whole path main.py takes: draw_mix -> mix_batch, both modes."""
    x, y = make(16, 32, 32, 10, 3)
    modes = set()
    for step in range(8):
        draw = D.draw_mix(0, 1, step, 32, 32, 0.2, 1.0)
        modes.add(draw["mode"])
        out, tgt = run(x, y, 10, draw)
        if draw["mode"] == "mixup":
            want = x.mul(f32(draw["lam"])).add(x.roll(1, 0).mul(f32(1.0 - draw["lam"])))
        else:
            y1, y2, x1, x2 = draw["box"]
            want = x.clone()
            want[:, :, y1:y2, x1:x2] = x.roll(1, 0)[:, :, y1:y2, x1:x2]
        assert torch.equal(out, want) and torch.equal(tgt, target_reference(y, 10, draw["lam_t"]))
        np.testing.assert_allclose(tgt.sum(1).numpy(), 1.0, atol=1e-6)
    assert modes == {"mixup", "cutmix"}


@pytest.mark.parametrize("H,W", [(8, 8), (32, 20)])
def test_pointers_off_16_bytes_take_the_scalar_kernel(H, W):
    """x and out as contiguous views one float into their buffers: W % 4 == 0, but the pointers do not allow 16-byte
    accesses, so the launch falls back to single elements.  Same results, bit for bit."""
    x, y = make(5, H, W, 10, 77)
    n = x.numel()
    src = torch.empty(n + 1, device=DEV)[1:].view_as(x).copy_(x.to(DEV))
    out = torch.empty(n + 1, device=DEV)[1:].view_as(x)
    tgt = torch.empty(5, 10, device=DEV)
    assert src.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4 and src.is_contiguous() and out.is_contiguous()
    yd = y.to(DEV)
    ops.mix_batch(src, yd, out, tgt, lam=0.3, lam_t=0.3)
    assert torch.equal(out.cpu(), x.mul(f32(0.3)).add(x.roll(1, 0).mul(f32(1.0 - 0.3))))
    assert torch.equal(tgt.cpu(), target_reference(y, 10, 0.3))
    box = (1, H - 2, 3, W - 2)
    lam_t = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / float(H * W)
    ops.mix_batch(src, yd, out, tgt, lam=1.0, box=box, lam_t=lam_t)
    want = x.clone()
    want[:, :, box[0]:box[1], box[2]:box[3]] = x.roll(1, 0)[:, :, box[0]:box[1], box[2]:box[3]]
    assert torch.equal(out.cpu(), want) and torch.equal(tgt.cpu(), target_reference(y, 10, lam_t))
    # only one of the two off 16 bytes: still the scalar kernel
    aligned = torch.empty_like(x, device=DEV)
    ops.mix_batch(src, yd, aligned, tgt, lam=1.0, box=box, lam_t=lam_t)
    assert torch.equal(aligned.cpu(), want)


def test_a_label_outside_the_classes_gives_nan_rows_and_an_intact_batch():
    """The -1 a shard hands out for an index it does not own: every target row built from it (its own and the row of
    the sample it is the partner of) is NaN, the other rows and every image are what they would be anyway."""
    x, y = make(6, 8, 8, 10, 9)
    good_out, good_tgt = run(x, y, 10, {"mode": "mixup", "lam": 0.25, "box": (0, 0, 0, 0), "lam_t": 0.25})
    for bad in (-1, 10, 2 ** 40):
        yb = y.clone()
        yb[2] = bad
        out, tgt = run(x, yb, 10, {"mode": "mixup", "lam": 0.25, "box": (0, 0, 0, 0), "lam_t": 0.25})
        assert torch.equal(out, good_out)
        assert torch.isnan(tgt[2]).all() and torch.isnan(tgt[3]).all()
        keep = [0, 1, 4, 5]
        assert torch.equal(tgt[keep], good_tgt[keep])


def test_refusals():
    x, y = make(4, 8, 8, 10, 1)
    xd, yd = x.to(DEV), y.to(DEV)
    tgt = torch.empty(4, 10, device=DEV)
    with pytest.raises(_C.NBDTHipError, match="overlap"):
        ops.mix_batch(xd, yd, xd, tgt, lam=0.5, lam_t=0.5)
    buf = torch.empty(2 * xd.numel(), device=DEV)
    src = buf[:xd.numel()].view_as(xd).copy_(xd)
    with pytest.raises(_C.NBDTHipError, match="overlap"):           # shifted by one image: still overlapping
        ops.mix_batch(src, yd, buf[3 * 64:3 * 64 + xd.numel()].view_as(xd), tgt, lam=0.5, lam_t=0.5)
    for bad_tgt in (xd.view(-1)[:40].view(4, 10), buf[xd.numel():xd.numel() + 40].view(4, 10)):      # tgt inside x / inside out
        with pytest.raises(_C.NBDTHipError, match="tgt must not overlap"):
            ops.mix_batch(xd, yd, buf[xd.numel():].view_as(xd), bad_tgt, lam=0.5, lam_t=0.5)
    with pytest.raises(_C.NBDTHipError, match="box"):
        ops.mix_batch(xd, yd, torch.empty_like(xd), tgt, lam=1.0, box=(0, 9, 0, 4), lam_t=0.5)
    with pytest.raises(_C.NBDTHipError, match="contiguous device tensors"):
        ops.mix_batch(xd, yd.int(), torch.empty_like(xd), tgt, lam=0.5, lam_t=0.5)
    with pytest.raises(_C.NBDTHipError, match="contiguous device tensors"):
        ops.mix_batch(xd.double(), yd, torch.empty_like(xd), tgt, lam=0.5, lam_t=0.5)
