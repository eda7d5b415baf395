"""The inputs of tests/test_conv_resnet_shapes_gpu.py, checked on the host: the integer inputs of every case make every
result exactly representable (so the GPU tests may ask for the reference bit for bit), every 32-channel block of the
weights takes part, and the batches of the case table are the smallest that take the engines' kernels."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resnet_conv_cases as C  # noqa: E402

IDS = [C.case_id(c) for c in C.RESNET_CASES]


@pytest.mark.parametrize("case", C.RESNET_CASES, ids=IDS)
def test_integer_inputs_keep_every_result_exact(case):
    B, H, W, cin, cout, k, stride = case
    c = C.integer_case(case)
    x, gy, w = c["x"], c["gy"], c["w"]
    assert x.abs().max() <= 2 and gy.abs().max() <= 2 and set(w.unique().tolist()) == {-1, 0, 1}
    # every (cout block, cin slice) block of every tap holds a non-zero: no 32-channel K slice, tap or cout block of any
    # kernel multiplies zeros only
    blocks = w.abs().view(cout // 32, 32, k * k, cin // 32, 32).sum((1, 4))
    assert blocks.min().item() >= 1
    # sum |x||w| + |base| <= 256 for every output of the forward (+ residual) and of the data gradient (+ accumulate
    # base): every partial sum in any order is an integer of at most 256 in magnitude, exact in fp32 and in bf16
    fwd_abs, dgrad_abs, _ = C.conv_refs(x.abs(), C.oihw(w.abs(), k), gy.abs(), stride)
    assert (C._exact(fwd_abs) + c["res"].abs()).max().item() <= 256
    assert (C._exact(dgrad_abs) + c["base"].abs()).max().item() <= 256
    assert c["fwd"].abs().max().item() >= 4 and c["dgrad"].abs().max().item() >= 4     # (not a degenerate case)
    # statistics epilogue: per-channel sums and sums of squares of the output are integers below 2^24 (exact in fp32,
    # whatever the order of the partial sums: each is bounded by sum v^2)
    assert (c["fwd"] ** 2).sum((0, 1, 2)).max().item() < 2 ** 24
    # weight gradient: sum |x||gy| over the pixels, twice (the second launch adds)
    Ho, Wo = H // stride, W // stride
    assert 2 * 4 * B * Ho * Wo < 2 ** 24
    assert c["dw"].abs().max().item() > 8


def test_float64_references_are_the_int64_convolutions():
    """The references are computed in float64 (exact for these integers); one small case against torch's int64 conv2d."""
    case = (1, 32, 32, 64, 128, 3, 2)
    c = C.integer_case(case)
    ref = F.conv2d(c["x"].permute(0, 3, 1, 2), C.oihw(c["w"], 3), None, 2, 1).permute(0, 2, 3, 1)
    assert ref.dtype == torch.int64 and torch.equal(ref, c["fwd"])


@pytest.mark.parametrize("case", C.RESNET_CASES, ids=IDS)
def test_batches_are_the_smallest_that_take_the_kernels_of_128_images(case):
    """nbdt_conv_plan / nbdt_conv_wgrad_blocks (host arithmetic): at the table's batch the forward and the data gradient
    take the form and K split they take at 128 images (the 32x32 stage: forced onto 512-pixel tiles), and the weight
    gradient the same kernel family; no smaller batch with a full 256-pixel output tile does."""
    assert C.host_plan(case, case[0]) == C.host_plan(case, 128, force=False)
    assert C.min_batch(case) == case[0]
    fwd, dgrad, wgrad = C.kernel_names(case)
    (form, ks), (dform, dks), taps = C.host_plan(case, case[0])
    names = {(C.PP512, 1): "conv3x3_pp_kernel", (C.HALF, 1): "conv3x3_pp_kernel/half", (C.HALF, 4): "conv3x3_pp_kernel/half/ksplit",
             (0, 1): "conv_igemm_dma_kernel"}
    assert names[(form, ks)] == fwd
    assert names[(dform, dks)] == (dgrad if dgrad != "conv_igemm_dma_multi_kernel" else "conv_igemm_dma_kernel")
    assert taps == (wgrad == "conv_wgrad_ks_kernel")


def test_table_lists_each_conv_once_and_the_engines_widths():
    assert len(set(c[1:] for c in C.RESNET_CASES)) == len(C.RESNET_CASES)
    convs = {(cin, cout, k, s, H) for _, H, _, cin, cout, k, s in C.RESNET_CASES}
    # ResNetEngine: stage widths 64 .. 512 on 32x32 .. 4x4, a strided 3x3 and a strided 1x1 shortcut between stages
    for i, (c, h) in enumerate(((64, 32), (128, 16), (256, 8), (512, 4))):
        assert (c, c, 3, 1, h) in convs
        if i:
            assert (c // 2, c, 3, 2, 2 * h) in convs and (c // 2, c, 1, 2, 2 * h) in convs
    # BottleneckEngine: per stage 1x1 (in -> planes, 4 planes -> planes), 3x3 (stride of the stage), 1x1 (planes -> 4 planes)
    cin, h = 64, 32
    for planes, stride in ((64, 1), (128, 2), (256, 2), (512, 2)):
        ho = h // stride
        assert (cin, planes, 1, 1, h) in convs and (planes, planes, 3, stride, h) in convs
        assert (planes, 4 * planes, 1, 1, ho) in convs and (4 * planes, planes, 1, 1, ho) in convs
        assert (cin, 4 * planes, 1, stride, h) in convs and (planes, planes, 3, 1, ho) in convs
        cin, h = 4 * planes, ho
