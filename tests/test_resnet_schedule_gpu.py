"""The launch schedule of ResNetEngine and BottleneckEngine, pinned launch by launch.

The two engines share one residual-block protocol: which launch writes which buffer, on which stream, in which order --
the buffers a side-stream weight gradient reads alternate between consecutive blocks, the shortcut's data gradient
accumulates into the block-input gradient AFTER conv1's plain one, an identity shortcut writes its gradient straight
into it.  This file records every nbdt.ops entry point the engines call over a forward and a backward and compares each
block's slice of that trace with the lists below, written out by hand from forward() / backward() as they stood when each
engine carried its own copy of the protocol (the file passed against that code unchanged).

One recorded launch is (op, buffer, extra):
  buffer  the name (first element of its engine._bufs key) of the launch's output -- for the BatchNorm statistics
          launches, whose outputs are [C] vectors, of the tensor they reduce; for weight gradients the parameter's name;
  extra   conv_igemm / conv_pw / conv_igemm_multi / conv_igemm_bnbwd: desc.accumulate; conv_igemm_affine: (act, residual);
          bn_apply: (relu, residual); bn_bwd: g_resid; bn_bwd_fused: cus > 0; conv_wgrad: cu_budget > 0; else None.
Whether the launch ran on the engine's side stream is recorded beside it and asserted for the whole trace: every weight
gradient and nothing else in the two-stream state, nothing after set_overlap(False)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from nbdt import ops  # noqa: E402
from nbdt import engine as E  # noqa: E402
from _launch_trace import Recorder  # noqa: E402

DEV = "cuda:0"
SMALL = (2, 1, 1, 1)
ASSERTED = ("l1b0", "l1b1", "l2b0")


def _inputs(B):
    g = torch.Generator().manual_seed(41)
    return torch.randn(B, 3, 32, 32, generator=g).to(DEV), (0.01 * torch.randn(B, 10, generator=g)).to(DEV)


def _train(eng, B):
    x, gz = _inputs(B)
    eng.zero_grad()
    with Recorder(eng) as fwd:
        eng.forward(x, training=True)
    with Recorder(eng) as bwd:
        eng.backward(gz)
    torch.cuda.synchronize()
    return fwd, bwd


def _eval(eng, B):
    with Recorder(eng) as rec:
        eng.forward(_inputs(B)[0], training=False)
    torch.cuda.synchronize()
    return rec


def _forward_slices(eng, rec, first):
    """{block key: (start, end)} of a forward trace: from the launch that writes `key + first` to the one that writes
    key.out; the slices must tile the trace between the stem's three launches and the head's two."""
    out = [t[1] for t in rec.trace]
    sl, at = {}, 3 if first == ".t1" else 2
    for blk in eng.blocks:
        k = blk["key"]
        start, end = out.index(k + first), out.index(k + ".out") + 1
        assert start == at, (k, start, at)
        sl[k], at = (start, end), end
    assert at == len(out) - 2
    return sl


def _backward_slices(eng, rec):
    """{block key: (start, end)} of a backward trace: a block starts at the BatchNorm backward that reads its key.out and
    ends where the next one starts (the last one at the stem's BatchNorm backward into gt0)."""
    starts = {}
    for blk in eng.blocks:
        k = blk["key"]
        hits = [i for i, (t, r) in enumerate(zip(rec.trace, rec.reads)) if t[0] == "bn_bwd" and k + ".out" in r]
        assert len(hits) == 1, (k, hits)
        starts[k] = hits[0]
    order = [b["key"] for b in reversed(eng.blocks)]
    bounds = [starts[k] for k in order] + [[t[1] for t in rec.trace].index("gt0")]
    assert bounds == sorted(bounds) and bounds[0] == 2 and bounds[-1] == len(rec.trace) - 2
    return {k: (bounds[i], bounds[i + 1]) for i, k in enumerate(order)}


def _check_blocks(rec, slices, want):
    for k in ASSERTED:
        a, b = slices[k]
        assert rec.trace[a:b] == want[k], (k, rec.trace[a:b])


def _check_streams(rec, two_streams):
    for t, side in zip(rec.trace, rec.side):
        assert side == (two_streams and t[0] == "conv_wgrad"), t


def _check_rotation(eng, rec, slices):
    """What a side-stream weight gradient of one block reads, no main-stream launch of the next block (or, after the
    last block, of the stem) writes: the main stream waits only for what the side stream was given one block ago."""
    order = [b["key"] for b in reversed(eng.blocks)]
    spans = [slices[k] for k in order] + [(slices[order[-1]][1], len(rec.trace))]
    n_side = 0
    for (a, b), (c, d) in zip(spans, spans[1:]):
        read = set().union(*(rec.reads[i] for i in range(a, b) if rec.side[i]))
        n_side += sum(rec.side[a:b])
        written = {rec.trace[i][1] for i in range(c, d) if not rec.side[i]}
        assert not read & written, (read & written, rec.trace[a:b], rec.trace[c:d])
    return n_side


STEM_FWD = [("stem_conv", "t0", None), ("bn_stats", "t0", None), ("bn_apply", "a0", (True, None))]
STEM_EVAL = [("stem_conv", "t0", None), ("bn_apply", "a0", (True, None))]
HEAD_FWD = [("bn_relu_pool", "pooled", None), ("linear_fwd", "z", None)]
STEM_BWD = [("bn_bwd", "gt0", None), ("stem_wgrad", "conv1.weight", None)]


def _head_bwd(feat_c):
    return [("linear_bwd", "gpool", None), ("pool_bn_bwd_apply", f"g_out{feat_c}", None)]


# ---------------------------------------------------------------------------------------------------------------------
# ResNetEngine((2, 1, 1, 1)), 32 images of 32x32.  Backward visits l4b0, l3b0, l2b0, l1b1, l1b0 with par = 0, 1, 0, 1, 0.

R_FWD = {
    "l1b0": [("conv_igemm", "l1b0.t1", False), ("bn_finalize", "l1b0.t1", None), ("bn_apply", "l1b0.a1", (True, None)),
             ("conv_igemm", "l1b0.t2", False), ("bn_finalize", "l1b0.t2", None), ("bn_apply", "l1b0.out", (True, "a0"))],
    "l1b1": [("conv_igemm", "l1b1.t1", False), ("bn_finalize", "l1b1.t1", None), ("bn_apply", "l1b1.a1", (True, None)),
             ("conv_igemm", "l1b1.t2", False), ("bn_finalize", "l1b1.t2", None),
             ("bn_apply", "l1b1.out", (True, "l1b0.out"))],
    "l2b0": [("conv_igemm", "l2b0.t1", False), ("bn_finalize", "l2b0.t1", None), ("bn_apply", "l2b0.a1", (True, None)),
             ("conv_igemm", "l2b0.t2", False), ("bn_finalize", "l2b0.t2", None),
             ("conv_igemm", "l2b0.ts", False), ("bn_finalize", "l2b0.ts", None), ("bn_apply", "sc128", (False, None)),
             ("bn_apply", "l2b0.out", (True, "sc128"))],
}
R_EVAL = {
    "l1b0": [("conv_igemm_affine", "l1b0.a1", (1, None)), ("conv_igemm_affine", "l1b0.out", (1, "a0"))],
    "l1b1": [("conv_igemm_affine", "l1b1.a1", (1, None)), ("conv_igemm_affine", "l1b1.out", (1, "l1b0.out"))],
    "l2b0": [("conv_igemm_affine", "l2b0.a1", (1, None)), ("conv_igemm_affine", "sc128", (0, None)),
             ("conv_igemm_affine", "l2b0.out", (1, "sc128"))],
}
# the (conv2, bn1) pair in its three forms, then the block around it
R_PAIR = {
    "shared": {
        "l1b0": [("conv_igemm_bnbwd", "ga1_64", False), ("conv_wgrad", "layer1.0.conv2.weight", True),
                 ("bn_bwd_fused", "gt1_64_0", True)],
        "l1b1": [("conv_igemm_bnbwd", "ga1_64", False), ("conv_wgrad", "layer1.1.conv2.weight", True),
                 ("bn_bwd_fused", "gt1_64_1", True)],
        "l2b0": [("conv_igemm_bnbwd", "ga1_128", False), ("conv_wgrad", "layer2.0.conv2.weight", True),
                 ("bn_bwd_fused", "gt1_128_0", True)],
    },
    "fused": {
        "l1b0": [("conv_wgrad", "layer1.0.conv2.weight", False), ("conv_igemm_bnbwd", "ga1_64", False),
                 ("bn_bwd_fused", "gt1_64_0", False)],
        "l1b1": [("conv_wgrad", "layer1.1.conv2.weight", False), ("conv_igemm_bnbwd", "ga1_64", False),
                 ("bn_bwd_fused", "gt1_64_1", False)],
        "l2b0": [("conv_wgrad", "layer2.0.conv2.weight", False), ("conv_igemm_bnbwd", "ga1_128", False),
                 ("bn_bwd_fused", "gt1_128_0", False)],
    },
    "plain": {
        "l1b0": [("conv_wgrad", "layer1.0.conv2.weight", False), ("conv_igemm", "ga1_64", False),
                 ("bn_bwd", "gt1_64_0", None)],
        "l1b1": [("conv_wgrad", "layer1.1.conv2.weight", False), ("conv_igemm", "ga1_64", False),
                 ("bn_bwd", "gt1_64_1", None)],
        "l2b0": [("conv_wgrad", "layer2.0.conv2.weight", False), ("conv_igemm", "ga1_128", False),
                 ("bn_bwd", "gt1_128_0", None)],
    },
}


def _r_bwd(form):
    p = R_PAIR[form]
    return {
        # identity blocks: bn2's backward writes the masked gradient into the block-input gradient, conv1's data gradient
        # accumulates onto it
        "l1b0": [("bn_bwd", "gt2_64_0", "g_in64_32_1")] + p["l1b0"]
                + [("conv_wgrad", "layer1.0.conv1.weight", False), ("conv_igemm", "g_in64_32_1", True)],
        "l1b1": [("bn_bwd", "gt2_64_1", "g_in64_32_0")] + p["l1b1"]
                + [("conv_wgrad", "layer1.1.conv1.weight", False), ("conv_igemm", "g_in64_32_0", True)],
        # strided shortcut: conv1's (four parity classes, one grid) plain data gradient first, the shortcut's accumulates
        "l2b0": [("bn_bwd", "gt2_128_0", "gsc_128")] + p["l2b0"]
                + [("conv_wgrad", "layer2.0.conv1.weight", False), ("conv_igemm_multi", "g_in64_32_1", False),
                   ("bn_bwd", "gts_128_0", None), ("conv_wgrad", "layer2.0.shortcut.0.weight", False),
                   ("conv_igemm", "g_in64_32_1", True)],
    }


@pytest.fixture(scope="module")
def resnet():
    return E.ResNetEngine(num_classes=10, num_blocks=SMALL, device=DEV, seed=0)


def _check_train(eng, B, want_fwd, want_bwd, two_streams):
    fwd, bwd = _train(eng, B)
    fs = _forward_slices(eng, fwd, ".t1")
    assert fwd.trace[:3] == STEM_FWD and fwd.trace[-2:] == HEAD_FWD
    _check_blocks(fwd, fs, want_fwd)
    _check_streams(fwd, False)
    bs = _backward_slices(eng, bwd)
    assert bwd.trace[:2] == _head_bwd(eng.feat_c) and bwd.trace[-2:] == STEM_BWD
    _check_blocks(bwd, bs, want_bwd)
    _check_streams(bwd, two_streams)
    n_side = _check_rotation(eng, bwd, bs)
    assert n_side == (sum(t[0] == "conv_wgrad" for t in bwd.trace) if two_streams else 0)
    return bwd


def test_resnet_training_step_two_streams(resnet):
    form = "shared" if ops.cu_topology_is_mi355x(resnet.device) else "fused"
    bwd = _check_train(resnet, 32, R_FWD, _r_bwd(form), True)
    assert sum(t[0] == "conv_wgrad" for t in bwd.trace) == 2 * 5 + 3


def test_resnet_training_step_one_stream(resnet):
    resnet.set_overlap(False)
    try:
        _check_train(resnet, 32, R_FWD, _r_bwd("fused"), False)
    finally:
        resnet.set_overlap(True)


def test_resnet_training_step_without_fused_bn1_backward(resnet):
    resnet.fuse_bn1_bwd = False
    try:
        _check_train(resnet, 32, R_FWD, _r_bwd("plain"), True)
    finally:
        resnet.fuse_bn1_bwd = True


def _check_eval(eng, B, want, per_block):
    rec = _eval(eng, B)
    assert rec.trace[:2] == STEM_EVAL and rec.trace[-2:] == HEAD_FWD
    sl = _forward_slices(eng, rec, ".a1")
    _check_blocks(rec, sl, want)
    _check_streams(rec, False)
    for blk in eng.blocks:
        a, b = sl[blk["key"]]
        assert all(t[0] == "conv_igemm_affine" for t in rec.trace[a:b])
        assert b - a == per_block + (blk["sconv"] is not None)


def test_resnet_eval_forward(resnet):
    _check_eval(resnet, 32, R_EVAL, 2)


# ---------------------------------------------------------------------------------------------------------------------
# BottleneckEngine((2, 1, 1, 1)), 8 images of 32x32: l1b0 has a stride-1 conv shortcut, l1b1 an identity one, l2b0 a strided
# one.  Stride-1 1x1 data gradients run on conv_pw; statistics launches below 1024 input channels stay on conv_igemm.

B_FWD = {
    "l1b0": [("conv_igemm", "l1b0.t1", False), ("bn_finalize", "l1b0.t1", None), ("bn_apply", "l1b0.a1", (True, None)),
             ("conv_igemm", "l1b0.t2", False), ("bn_finalize", "l1b0.t2", None), ("bn_apply", "l1b0.a2", (True, None)),
             ("conv_igemm", "l1b0.t3", False), ("bn_finalize", "l1b0.t3", None),
             ("conv_igemm", "l1b0.ts", False), ("bn_finalize", "l1b0.ts", None), ("bn_apply", "sc256", (False, None)),
             ("bn_apply", "l1b0.out", (True, "sc256"))],
    "l1b1": [("conv_igemm", "l1b1.t1", False), ("bn_finalize", "l1b1.t1", None), ("bn_apply", "l1b1.a1", (True, None)),
             ("conv_igemm", "l1b1.t2", False), ("bn_finalize", "l1b1.t2", None), ("bn_apply", "l1b1.a2", (True, None)),
             ("conv_igemm", "l1b1.t3", False), ("bn_finalize", "l1b1.t3", None),
             ("bn_apply", "l1b1.out", (True, "l1b0.out"))],
    "l2b0": [("conv_igemm", "l2b0.t1", False), ("bn_finalize", "l2b0.t1", None), ("bn_apply", "l2b0.a1", (True, None)),
             ("conv_igemm", "l2b0.t2", False), ("bn_finalize", "l2b0.t2", None), ("bn_apply", "l2b0.a2", (True, None)),
             ("conv_igemm", "l2b0.t3", False), ("bn_finalize", "l2b0.t3", None),
             ("conv_igemm", "l2b0.ts", False), ("bn_finalize", "l2b0.ts", None), ("bn_apply", "sc512", (False, None)),
             ("bn_apply", "l2b0.out", (True, "sc512"))],
}
B_EVAL = {
    "l1b0": [("conv_igemm_affine", "l1b0.a1", (1, None)), ("conv_igemm_affine", "l1b0.a2", (1, None)),
             ("conv_igemm_affine", "sc256", (0, None)), ("conv_igemm_affine", "l1b0.out", (1, "sc256"))],
    "l1b1": [("conv_igemm_affine", "l1b1.a1", (1, None)), ("conv_igemm_affine", "l1b1.a2", (1, None)),
             ("conv_igemm_affine", "l1b1.out", (1, "l1b0.out"))],
    "l2b0": [("conv_igemm_affine", "l2b0.a1", (1, None)), ("conv_igemm_affine", "l2b0.a2", (1, None)),
             ("conv_igemm_affine", "sc512", (0, None)), ("conv_igemm_affine", "l2b0.out", (1, "sc512"))],
}
# every (conv, previous bn) pair in the plain form: weight gradient, data gradient, BatchNorm backward
B_BWD = {
    "l1b0": [("bn_bwd", "gt3_256_0", "gsc_256"),
             ("conv_wgrad", "layer1.0.conv3.weight", False), ("conv_pw", "ga2_64", False), ("bn_bwd", "gt2_64_0", None),
             ("conv_wgrad", "layer1.0.conv2.weight", False), ("conv_igemm", "ga1_64", False), ("bn_bwd", "gt1_64_0", None),
             ("conv_wgrad", "layer1.0.conv1.weight", False), ("conv_pw", "g_in64_32_1", False),
             ("bn_bwd", "gts_256_0", None), ("conv_wgrad", "layer1.0.shortcut.0.weight", False),
             ("conv_pw", "g_in64_32_1", True)],
    "l1b1": [("bn_bwd", "gt3_256_1", "g_in256_32_0"),
             ("conv_wgrad", "layer1.1.conv3.weight", False), ("conv_pw", "ga2_64", False), ("bn_bwd", "gt2_64_1", None),
             ("conv_wgrad", "layer1.1.conv2.weight", False), ("conv_igemm", "ga1_64", False), ("bn_bwd", "gt1_64_1", None),
             ("conv_wgrad", "layer1.1.conv1.weight", False), ("conv_pw", "g_in256_32_0", True)],
    "l2b0": [("bn_bwd", "gt3_512_0", "gsc_512"),
             ("conv_wgrad", "layer2.0.conv3.weight", False), ("conv_pw", "ga2_128", False), ("bn_bwd", "gt2_128_0", None),
             ("conv_wgrad", "layer2.0.conv2.weight", False), ("conv_igemm_multi", "ga1_128", False),
             ("bn_bwd", "gt1_128_0", None),
             ("conv_wgrad", "layer2.0.conv1.weight", False), ("conv_pw", "g_in256_32_1", False),
             ("bn_bwd", "gts_512_0", None), ("conv_wgrad", "layer2.0.shortcut.0.weight", False),
             ("conv_igemm", "g_in256_32_1", True)],
}


@pytest.fixture(scope="module")
def bottleneck():
    return E.BottleneckEngine(num_classes=10, num_blocks=SMALL, device=DEV, seed=0)


def test_bottleneck_training_step_two_streams(bottleneck):
    assert bottleneck.fuse_bn1_bwd            # ... and every pair is in the plain form all the same
    bwd = _check_train(bottleneck, 8, B_FWD, B_BWD, True)
    assert sum(t[0] == "conv_wgrad" for t in bwd.trace) == 3 * 5 + 4
    assert not any(t[0] in ("conv_igemm_bnbwd", "bn_bwd_fused") for t in bwd.trace)


def test_bottleneck_training_step_one_stream(bottleneck):
    bottleneck.set_overlap(False)
    try:
        _check_train(bottleneck, 8, B_FWD, B_BWD, False)
    finally:
        bottleneck.set_overlap(True)


def test_bottleneck_eval_forward(bottleneck):
    _check_eval(bottleneck, 8, B_EVAL, 3)


# ---------------------------------------------------------------------------------------------------------------------
# Parameter layout: (name, offset in the flat buffers, internal shape), in creation order -- the seeded generator is drawn
# from in this order and every offset follows from it.

R_ENTRIES = [
    ("conv1.weight", 0, (64, 3, 3, 3)), ("bn1.weight", 1728, (64,)), ("bn1.bias", 1792, (64,)),
    ("layer1.0.conv1.weight", 1856, (64, 9, 64)), ("layer1.0.bn1.weight", 38720, (64,)), ("layer1.0.bn1.bias", 38784, (64,)),
    ("layer1.0.conv2.weight", 38848, (64, 9, 64)), ("layer1.0.bn2.weight", 75712, (64,)), ("layer1.0.bn2.bias", 75776, (64,)),
    ("layer1.1.conv1.weight", 75840, (64, 9, 64)), ("layer1.1.bn1.weight", 112704, (64,)), ("layer1.1.bn1.bias", 112768, (64,)),
    ("layer1.1.conv2.weight", 112832, (64, 9, 64)), ("layer1.1.bn2.weight", 149696, (64,)),
    ("layer1.1.bn2.bias", 149760, (64,)), ("layer2.0.conv1.weight", 149824, (128, 9, 64)),
    ("layer2.0.bn1.weight", 223552, (128,)), ("layer2.0.bn1.bias", 223680, (128,)),
    ("layer2.0.conv2.weight", 223808, (128, 9, 128)), ("layer2.0.bn2.weight", 371264, (128,)),
    ("layer2.0.bn2.bias", 371392, (128,)), ("layer2.0.shortcut.0.weight", 371520, (128, 1, 64)),
    ("layer2.0.shortcut.1.weight", 379712, (128,)), ("layer2.0.shortcut.1.bias", 379840, (128,)),
    ("layer3.0.conv1.weight", 379968, (256, 9, 128)), ("layer3.0.bn1.weight", 674880, (256,)),
    ("layer3.0.bn1.bias", 675136, (256,)), ("layer3.0.conv2.weight", 675392, (256, 9, 256)),
    ("layer3.0.bn2.weight", 1265216, (256,)), ("layer3.0.bn2.bias", 1265472, (256,)),
    ("layer3.0.shortcut.0.weight", 1265728, (256, 1, 128)), ("layer3.0.shortcut.1.weight", 1298496, (256,)),
    ("layer3.0.shortcut.1.bias", 1298752, (256,)), ("layer4.0.conv1.weight", 1299008, (512, 9, 256)),
    ("layer4.0.bn1.weight", 2478656, (512,)), ("layer4.0.bn1.bias", 2479168, (512,)),
    ("layer4.0.conv2.weight", 2479680, (512, 9, 512)), ("layer4.0.bn2.weight", 4838976, (512,)),
    ("layer4.0.bn2.bias", 4839488, (512,)), ("layer4.0.shortcut.0.weight", 4840000, (512, 1, 256)),
    ("layer4.0.shortcut.1.weight", 4971072, (512,)), ("layer4.0.shortcut.1.bias", 4971584, (512,)),
    ("linear.weight", 4972096, (10, 512)), ("linear.bias", 4977216, (10,)),
]
B_ENTRIES = [
    ("conv1.weight", 0, (64, 3, 3, 3)), ("bn1.weight", 1728, (64,)), ("bn1.bias", 1792, (64,)),
    ("layer1.0.conv1.weight", 1856, (64, 1, 64)), ("layer1.0.bn1.weight", 5952, (64,)), ("layer1.0.bn1.bias", 6016, (64,)),
    ("layer1.0.conv2.weight", 6080, (64, 9, 64)), ("layer1.0.bn2.weight", 42944, (64,)), ("layer1.0.bn2.bias", 43008, (64,)),
    ("layer1.0.conv3.weight", 43072, (256, 1, 64)), ("layer1.0.bn3.weight", 59456, (256,)),
    ("layer1.0.bn3.bias", 59712, (256,)), ("layer1.0.shortcut.0.weight", 59968, (256, 1, 64)),
    ("layer1.0.shortcut.1.weight", 76352, (256,)), ("layer1.0.shortcut.1.bias", 76608, (256,)),
    ("layer1.1.conv1.weight", 76864, (64, 1, 256)), ("layer1.1.bn1.weight", 93248, (64,)), ("layer1.1.bn1.bias", 93312, (64,)),
    ("layer1.1.conv2.weight", 93376, (64, 9, 64)), ("layer1.1.bn2.weight", 130240, (64,)), ("layer1.1.bn2.bias", 130304, (64,)),
    ("layer1.1.conv3.weight", 130368, (256, 1, 64)), ("layer1.1.bn3.weight", 146752, (256,)),
    ("layer1.1.bn3.bias", 147008, (256,)), ("layer2.0.conv1.weight", 147264, (128, 1, 256)),
    ("layer2.0.bn1.weight", 180032, (128,)), ("layer2.0.bn1.bias", 180160, (128,)),
    ("layer2.0.conv2.weight", 180288, (128, 9, 128)), ("layer2.0.bn2.weight", 327744, (128,)),
    ("layer2.0.bn2.bias", 327872, (128,)), ("layer2.0.conv3.weight", 328000, (512, 1, 128)),
    ("layer2.0.bn3.weight", 393536, (512,)), ("layer2.0.bn3.bias", 394048, (512,)),
    ("layer2.0.shortcut.0.weight", 394560, (512, 1, 256)), ("layer2.0.shortcut.1.weight", 525632, (512,)),
    ("layer2.0.shortcut.1.bias", 526144, (512,)), ("layer3.0.conv1.weight", 526656, (256, 1, 512)),
    ("layer3.0.bn1.weight", 657728, (256,)), ("layer3.0.bn1.bias", 657984, (256,)),
    ("layer3.0.conv2.weight", 658240, (256, 9, 256)), ("layer3.0.bn2.weight", 1248064, (256,)),
    ("layer3.0.bn2.bias", 1248320, (256,)), ("layer3.0.conv3.weight", 1248576, (1024, 1, 256)),
    ("layer3.0.bn3.weight", 1510720, (1024,)), ("layer3.0.bn3.bias", 1511744, (1024,)),
    ("layer3.0.shortcut.0.weight", 1512768, (1024, 1, 512)), ("layer3.0.shortcut.1.weight", 2037056, (1024,)),
    ("layer3.0.shortcut.1.bias", 2038080, (1024,)), ("layer4.0.conv1.weight", 2039104, (512, 1, 1024)),
    ("layer4.0.bn1.weight", 2563392, (512,)), ("layer4.0.bn1.bias", 2563904, (512,)),
    ("layer4.0.conv2.weight", 2564416, (512, 9, 512)), ("layer4.0.bn2.weight", 4923712, (512,)),
    ("layer4.0.bn2.bias", 4924224, (512,)), ("layer4.0.conv3.weight", 4924736, (2048, 1, 512)),
    ("layer4.0.bn3.weight", 5973312, (2048,)), ("layer4.0.bn3.bias", 5975360, (2048,)),
    ("layer4.0.shortcut.0.weight", 5977408, (2048, 1, 1024)), ("layer4.0.shortcut.1.weight", 8074560, (2048,)),
    ("layer4.0.shortcut.1.bias", 8076608, (2048,)), ("linear.weight", 8078656, (10, 2048)), ("linear.bias", 8099136, (10,)),
]


def test_parameter_layout(resnet, bottleneck):
    for eng, want in ((resnet, R_ENTRIES), (bottleneck, B_ENTRIES)):
        assert [(n, off, shape) for n, (off, shape) in eng.store.entries.items()] == want
