"""The convolutions ResNetEngine and BottleneckEngine launch at 32x32 input, as per-op test cases, and the inputs the
per-op tests run them on (tests/test_conv_resnet_cases.py on the host, tests/test_conv_resnet_shapes_gpu.py on the GPU).

Integer inputs: activations in [-2, 2], a residual / accumulate base in [-8, 8], weights in {-1, 0, 1}.  The weights are
sparse by construction: every 32 x 32 (cout block, cin slice) block of every tap holds n non-zeros on n distinct rows
and n distinct columns; the row sets of the blocks along a cout row are consecutive windows of the 32 residues (and the
column sets along a cin column likewise), so a cout row holds at most ceil(taps * cin/32 * n / 32) non-zeros and a cin
column at most ceil(taps * cout/32 * n / 32).  n is the largest count that keeps both at MAX_NNZ = 124 or below:
sum |x||w| + |base| <= 2 * 124 + 8 = 256, and every integer up to 256 is a bf16.  Signs and the row / column pairing
inside a block are random."""
import torch
import torch.nn.functional as F

import nbdt_path

nbdt_path.add()
from nbdt import ops  # noqa: E402

X_MAX, BASE_MAX, MAX_NNZ = 2, 8, 124

# B, H, W (input), cin, cout, k, stride.  B: the smallest batch at which the forward, data-gradient and weight-gradient
# launches take the kernels they take at 128 images (the dense 3x3 rules look at the tile count; the K-split weight
# gradient needs 4096 pixels) and the output holds one full 256-pixel tile -- min_batch() below, pinned by
# tests/test_conv_resnet_cases.py.
RESNET_CASES = [
    # ResNetEngine (BasicBlock), and the same dense 3x3 convs in BottleneckEngine
    (4, 32, 32, 64, 64, 3, 1),
    (16, 16, 16, 128, 128, 3, 1),
    (64, 8, 8, 256, 256, 3, 1),
    (16, 4, 4, 512, 512, 3, 1),       # one half tile x 4 cout tiles, 144 K steps: the automatic K split; nine-tap wgrad_dma
    (1, 32, 32, 64, 128, 3, 2),
    (4, 16, 16, 128, 256, 3, 2),
    (16, 8, 8, 256, 512, 3, 2),
    (1, 32, 32, 64, 128, 1, 2),
    (4, 16, 16, 128, 256, 1, 2),
    (16, 8, 8, 256, 512, 1, 2),
    # BottleneckEngine: 1x1 convs
    (1, 32, 32, 64, 64, 1, 1),
    (1, 32, 32, 64, 256, 1, 1),
    (1, 32, 32, 256, 64, 1, 1),
    (1, 32, 32, 256, 128, 1, 1),
    (1, 16, 16, 128, 512, 1, 1),
    (1, 16, 16, 512, 128, 1, 1),
    (1, 16, 16, 512, 256, 1, 1),
    (4, 8, 8, 256, 1024, 1, 1),
    (4, 8, 8, 1024, 256, 1, 1),
    (4, 8, 8, 1024, 512, 1, 1),
    (16, 4, 4, 512, 2048, 1, 1),
    (16, 4, 4, 2048, 512, 1, 1),
    # ... strided 3x3 convs
    (1, 32, 32, 128, 128, 3, 2),
    (4, 16, 16, 256, 256, 3, 2),
    (16, 8, 8, 512, 512, 3, 2),
    # ... strided 1x1 shortcuts
    (1, 32, 32, 256, 512, 1, 2),
    (4, 16, 16, 512, 1024, 1, 2),
    (16, 8, 8, 1024, 2048, 1, 2),
]


def case_id(case):
    B, H, W, cin, cout, k, stride = case
    return f"{cin}to{cout}_k{k}s{stride}_{H}x{W}_b{B}"


def dense3x3(case):
    return case[5] == 3 and case[6] == 1


def pointwise(case):
    return case[5] == 1 and case[6] == 1


# ------------------------------------------------------------------------------------------------------------------------
# which kernels a case takes

PP512, HALF = 2, 4          # ops.CONV_FORMS
TILED = 0x1000              # any non-zero "address": the plan never dereferences it


def force_wide(case):
    """desc.wide_tile of the forward / data-gradient launch, or None for engine.Conv's own.  At 128 images the 32x32 stage
    has 256 tiles of 512 pixels and takes the 512-pixel ping-pong kernel, which needs 192 of them: forced (wide_tile = 2)."""
    return 2 if dense3x3(case) and case[1] * case[2] >= 1024 else None


def descs(case, B=None, tiles=(TILED, TILED), force=True):
    """(forward, [data gradient], [accumulating data gradient], weight gradient) descriptors as engine.Conv plans them: the
    DMA-ordered weight tiles `tiles` = (forward, data gradient) on the dense 3x3 launches, wide_tile 1 / 0 -- or, with
    `force`, force_wide()'s."""
    _, H, W, cin, cout, k, stride = case
    B = case[0] if B is None else B
    args = (B, H, W, cin, cout, k, stride)
    plain = None if (k == 1 and stride == 2) else ops.conv_dgrad_descs(*args, accumulate=False)
    plan = (ops.conv_fwd_desc(*args), plain, ops.conv_dgrad_descs(*args, accumulate=True), ops.conv_wgrad_desc(*args))
    if dense3x3(case):
        wide = force_wide(case) if force else None
        plan[0].w_tiled = tiles[0]
        for ds in plan[1:3]:
            ds[0].w_tiled = tiles[1]
        if wide is not None:
            for d in (plan[0], plan[1][0], plan[2][0]):
                d.wide_tile = wide
    return plan


def host_plan(case, B, force=True):
    """What the launch rules say for batch B, without a GPU: (form, ksplit) of the forward and of the data gradient, and
    whether the weight gradient is the 8-wave dense 3x3 kernel."""
    fwd, plain, acc, wg = descs(case, B, force=force)
    return (ops.conv_plan(fwd), ops.conv_plan(acc[0]), ops.conv_wgrad_blocks(wg) > 0)


def min_batch(case):
    _, H, W, _, _, _, stride = case
    want = host_plan(case, 128, force=False)
    for B in range(1, 129):
        if B * (H // stride) * (W // stride) >= 256 and host_plan(case, B) == want:
            return B
    raise AssertionError(case)


def kernel_names(case):
    """(forward, data gradient, weight gradient) kernel names of the engine's launches at 128 images."""
    _, H, W, _, _, k, stride = case
    if dense3x3(case):
        conv = ("conv3x3_pp_kernel" if H * W >= 1024 else "conv3x3_pp_kernel/half" if H * W >= 64
                else "conv3x3_pp_kernel/half/ksplit")
        return conv, conv, "conv_wgrad_ks_kernel" if H >= 8 else "conv_wgrad_dma_kernel"
    dgrad = "conv_igemm_dma_multi_kernel" if (k == 3 and stride == 2) else "conv_igemm_dma_kernel"
    return "conv_igemm_dma_kernel", dgrad, "conv_wgrad_dma_kernel"


def conv_key(d):
    """What the case-table test compares of a conv descriptor: (cin, cout, ntaps, strided, gh, gw)."""
    return (d.cin, d.cout, d.ntaps, d.in_ws != d.cin or d.out_ws != d.cout, d.gh, d.gw)


def wgrad_key(d):
    return (d.cin, d.cout, d.ntaps, d.x_ws != d.cin, d.gh, d.gw)


def table_keys():
    """(conv descriptor keys, weight-gradient descriptor keys) of every launch of every case."""
    conv, wgrad = set(), set()
    for case in RESNET_CASES:
        fwd, plain, acc, wg = descs(case)
        conv.update(conv_key(d) for d in [fwd] + (plain or []) + acc)
        wgrad.add(wgrad_key(wg))
    return conv, wgrad


# ------------------------------------------------------------------------------------------------------------------------
# integer inputs and their exact references

def _nonzeros_per_block(taps, cin, cout):
    blocks = taps * max(cin, cout) // 32
    n = 32
    while (blocks * n + 31) // 32 > MAX_NNZ:
        n -= 1
    return n


def sparse_weights(cout, cin, taps, gen):
    """[cout][taps][cin] in {-1, 0, 1} (int64); see the module docstring."""
    n = _nonzeros_per_block(taps, cin, cout)
    ncb, nsb = cout // 32, cin // 32
    w = torch.zeros(cout, taps, cin, dtype=torch.int64)
    j = torch.arange(n)
    row_off = torch.randint(0, 32, (ncb,), generator=gen)
    col_off = torch.randint(0, 32, (nsb,), generator=gen)
    for cb in range(ncb):
        for t in range(taps):
            for sb in range(nsb):
                rows = (n * (t * nsb + sb) + j + row_off[cb]) % 32
                cols = ((n * (t * ncb + cb) + j + col_off[sb]) % 32)[torch.randperm(n, generator=gen)]
                sign = torch.randint(0, 2, (n,), generator=gen) * 2 - 1
                w[cb * 32 + rows, t, sb * 32 + cols] = sign
    return w


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _exact(t):
    """A float64 tensor of integers as int64.  The CPU convolutions below run in float64, which holds every partial sum of
    these inputs exactly (all far below 2^53): they ARE the int64 convolutions, at BLAS speed."""
    r = t.round()
    assert torch.equal(r, t) and t.abs().max().item() < 2.0 ** 52
    return r.to(torch.int64)


def conv_refs(x, w_oihw, gy, stride):
    """float64 forward [B,Ho,Wo,cout], data gradient [B,H,W,cin] and weight gradient [cout][taps][cin] of NHWC x / gy."""
    cout, cin, k, _ = w_oihw.shape
    x64, w64, g64 = _nchw(x).double(), w_oihw.double(), _nchw(gy).double()
    fwd = _nhwc(F.conv2d(x64, w64, None, stride, k // 2))
    dgrad = _nhwc(F.conv_transpose2d(g64, w64, None, stride, k // 2, output_padding=stride - 1))
    dw = torch.nn.grad.conv2d_weight(x64, w64.shape, g64, stride, k // 2)
    return fwd, dgrad, dw.permute(0, 2, 3, 1).reshape(cout, k * k, cin).contiguous()


def oihw(w_int, k):
    cout, _, cin = w_int.shape
    return w_int.view(cout, k, k, cin).permute(0, 3, 1, 2)


_INT = {}


def integer_case(case):
    """Integer inputs and int64 references of one case, built once and shared (never modified):
    x [B,H,W,cin], gy / res [B,Ho,Wo,cout], base [B,H,W,cin], w [cout][taps][cin]; fwd, dgrad, dw."""
    if case not in _INT:
        B, H, W, cin, cout, k, stride = case
        Ho, Wo = H // stride, W // stride
        gen = torch.Generator().manual_seed(1000 * cin + cout + 7 * k + stride)
        ints = lambda lim, *shape: torch.randint(-lim, lim + 1, shape, generator=gen)      # noqa: E731
        c = dict(x=ints(X_MAX, B, H, W, cin), gy=ints(X_MAX, B, Ho, Wo, cout), res=ints(BASE_MAX, B, Ho, Wo, cout),
                 base=ints(BASE_MAX, B, H, W, cin), w=sparse_weights(cout, cin, k * k, gen))
        fwd, dgrad, dw = conv_refs(c["x"], oihw(c["w"], k), c["gy"], stride)
        c.update(fwd=_exact(fwd), dgrad=_exact(dgrad), dw=_exact(dw))
        _INT[case] = c
    return _INT[case]
