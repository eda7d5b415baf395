"""Per-op cases of the grouped 3x3 convolution (csrc/conv_group.hip), their integer and random inputs with CPU references,
and a host restatement of the weight expansion -- shared by tests/test_resnext.py (host) and tests/test_conv_group_gpu.py.

The smallest shapes that can still go wrong: every cg the kernels take at width 64 (two 32-channel blocks: block indexing)
and cg = 4 at width 128 (32 groups, four blocks); 3 images; grids of 8 x 8, 7 x 7 (49 pixels per image: partial waves,
pixel runs that cross rows and images), 14 x 14, and stride 2 from 16 -> 8 and 14 -> 7.

Integer inputs: activations and gradients in [-2, 2], weights in {-1, 0, 1}.  A forward / data-gradient value is a sum of
at most 9 * cg products of magnitude <= 2, a weight gradient a sum over at most 588 pixels of products of magnitude <= 4;
integer_case() ASSERTS that every reference magnitude is <= 256, so each is a bf16 number (and an fp32 one), every partial
sum is exact in fp32 in any order, and no rounding mode or summation order can hide an error: the comparison is bit for bit."""
import numpy as np
import torch
import torch.nn.functional as F

B = 3
CONFIGS = [(64, 4), (64, 8), (64, 16), (64, 32), (128, 4)]            # (width, cg)
GRIDS = [(8, 8, 1), (7, 7, 1), (14, 14, 1), (16, 16, 2), (14, 14, 2)]  # (H, W of the input, stride)
CASES = [(width, cg, H, W, s) for width, cg in CONFIGS for H, W, s in GRIDS]
EXACT_MAX = 256


def case_id(case):
    width, cg, H, W, s = case
    return f"w{width}cg{cg}_{H}x{W}s{s}"


# ------------------------------------------------------------------------------------------------------------------------
# layouts

def master_of(w_oihw):
    """torchvision's grouped weight [width, cg, 3, 3] -> the project's master [width][9][cg] ([cout][taps][cin in group])."""
    width, cg = w_oihw.shape[:2]
    return w_oihw.permute(0, 2, 3, 1).reshape(width, 9, cg).contiguous()


def dense_block_diagonal(master):
    """numpy [width][9][width]: the dense conv that equals the grouped one -- master on the group diagonal, zeros elsewhere."""
    m = np.asarray(master)
    width, _, cg = m.shape
    d = np.zeros((width, 9, width), dtype=m.dtype)
    for co in range(width):
        g0 = co // cg * cg
        d[co, :, g0:g0 + cg] = m[co]
    return d


def expand_host(master):
    """Host restatement of nbdt_conv_group_weight_prep, written as the kernel is indexed (element by element of a block):
    (wf [width/32][32 co][9][32 ci], wd [width/32][32 ci][9][32 co]) as numpy arrays of master's dtype."""
    m = np.asarray(master)
    width, _, cg = m.shape
    nb = width // 32
    wf = np.zeros((nb, 32, 9, 32), dtype=m.dtype)
    wd = np.zeros((nb, 32, 9, 32), dtype=m.dtype)
    for n in range(nb):
        for r in range(32):
            for c in range(32):
                if r // cg != c // cg:
                    continue
                for t in range(9):
                    wf[n, r, t, c] = m[n * 32 + r, t, c % cg]            # wf[co = r][t][ci = c]
                    wd[n, r, t, c] = m[n * 32 + c, 8 - t, r % cg]        # wd[ci = r][t][co = c] = w[co][8 - t][ci]
    return wf, wd


# ------------------------------------------------------------------------------------------------------------------------
# references (NCHW on the CPU)

def refs(x, w_oihw, gy, stride, groups, dtype):
    """F.conv2d(groups=), torch.nn.grad.conv2d_input and conv2d_weight in `dtype`: forward [B,width,Ho,Wo], data gradient
    [B,width,H,W], weight gradient as the master [width][9][cg]."""
    x, w, g = x.to(dtype), w_oihw.to(dtype), gy.to(dtype)
    fwd = F.conv2d(x, w, None, stride, 1, 1, groups)
    gx = torch.nn.grad.conv2d_input(x.shape, w, g, stride, 1, 1, groups)
    dw = torch.nn.grad.conv2d_weight(x, w.shape, g, stride, 1, 1, groups)
    return fwd, gx, master_of(dw)


_INT, _REAL = {}, {}


def integer_case(case):
    """Integer inputs (float32 tensors holding integers) and their exact references, built once and never modified:
    x [B,width,H,W], gy [B,width,Ho,Wo], w [width,cg,3,3], dw0 (what dw holds before the call, [width][9][cg]);
    fwd, gx, dw (without dw0)."""
    if case not in _INT:
        width, cg, H, W, s = case
        gen = torch.Generator().manual_seed(97 * width + 13 * cg + 5 * H + s)
        ints = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).float()      # noqa: E731
        c = dict(x=ints(-2, 2, B, width, H, W), gy=ints(-2, 2, B, width, H // s, W // s), w=ints(-1, 1, width, cg, 3, 3),
                 dw0=ints(-4, 4, width, 9, cg))
        fwd, gx, dw = refs(c["x"], c["w"], c["gy"], s, width // cg, torch.float64)
        for name, t in (("fwd", fwd), ("gx", gx), ("dw", dw + c["dw0"].double())):
            assert torch.equal(t, t.round()) and t.abs().max().item() <= EXACT_MAX, (case, name, t.abs().max().item())
        f32 = refs(c["x"], c["w"], c["gy"], s, width // cg, torch.float32)
        assert all(torch.equal(a.double(), b) for a, b in zip(f32, (fwd, gx, dw)))       # fp32 equals fp64
        c.update(fwd=fwd.float(), gx=gx.float(), dw=dw.float())
        _INT[case] = c
    return _INT[case]


def real_case(case):
    """Random inputs rounded to bf16 (activations and gradients N(0, 1), weights N(0, 1 / (9 cg))) and the fp32 references
    on those rounded values; built once."""
    if case not in _REAL:
        width, cg, H, W, s = case
        gen = torch.Generator().manual_seed(31 * width + 7 * cg + 3 * H + s)
        rnd = lambda *shape: torch.randn(shape, generator=gen)      # noqa: E731
        bf = lambda t: t.to(torch.bfloat16).float()                  # noqa: E731
        c = dict(x=bf(rnd(B, width, H, W)), gy=bf(rnd(B, width, H // s, W // s)), w=bf(rnd(width, cg, 3, 3) / (9 * cg) ** 0.5))
        fwd, gx, dw = refs(c["x"], c["w"], c["gy"], s, width // cg, torch.float32)
        c.update(fwd=fwd, gx=gx, dw=dw)
        _REAL[case] = c
    return _REAL[case]
