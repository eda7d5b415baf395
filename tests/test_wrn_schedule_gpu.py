"""The launch schedule of WRNEngine, pinned launch by launch (the recorder of tests/_launch_trace.py).

WRNEngine(blocks=16, width_factor=2) on 16 images of 32x32: two units per stage, so every stage has one shape-changing
unit (on the slice-list kernel in training mode) and one dense unit -- the only ones that reach the shared, fused and
plain forms of the (conv1, bn1) pair.  One forward and one backward run under the recorder in the four backward forms
and, for two of them, on one stream; the slices of units s1u1 (stride-1 shortcut conv), s1u2 (dense) and s2u1 (strided)
are compared with the lists below, written out by hand from forward() / backward() as they stood when WRNEngine spelled
the (conv, preceding BatchNorm) pair out in _conv2_backward and _conv1_backward (the file passed against that code
unchanged).  At this size the conv2 + shortcut slice list would fall back to 256-pixel tiles, so every shape-changing
unit takes the dense conv2 with a separate shortcut launch; conv1 of the strided units and the data gradients of all
shape-changing units are slice lists ("ConvSeg").

Whether a launch ran on the engine's side stream is asserted for the whole trace: every weight gradient and nothing
else with two streams, nothing after set_overlap(False)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from nbdt import ops  # noqa: E402
from nbdt import engine as E  # noqa: E402
from _launch_trace import Recorder  # noqa: E402

DEV = "cuda:0"
B = 16
ASSERTED = ("s1u1", "s1u2", "s2u1")
W = {  # unit -> (conv1, conv2, shortcut conv) parameter names
    "s1u1": ("features.stage1.unit1.body.conv1.conv.weight", "features.stage1.unit1.body.conv2.conv.weight",
             "features.stage1.unit1.identity_conv.weight"),
    "s1u2": ("features.stage1.unit2.body.conv1.conv.weight", "features.stage1.unit2.body.conv2.conv.weight", None),
    "s2u1": ("features.stage2.unit1.body.conv1.conv.weight", "features.stage2.unit1.body.conv2.conv.weight",
             "features.stage2.unit1.identity_conv.weight"),
}


def _fwd(stats):
    """stats: the statistics launch of a tensor whose producer can leave partial sums ("bn_finalize": it did)."""
    return {
        "s1u1": [("bn_stats", "x0", None), ("bn_apply", "s1u1.a1", (True, None)),
                 ("conv_igemm", "s1u1.t", False), (stats, "s1u1.t", None), ("bn_apply", "s1u1.a2", (True, None)),
                 ("conv_igemm", "idn32", False), ("conv_igemm", "s1u1.out", False)],
        "s1u2": [(stats, "s1u1.out", None), ("bn_apply", "s1u2.a1", (True, None)),
                 ("conv_igemm", "s1u2.t", False), (stats, "s1u2.t", None), ("bn_apply", "s1u2.a2", (True, None)),
                 ("conv_igemm", "s1u2.out", False)],
        "s2u1": [(stats, "s1u2.out", None), ("bn_apply_s2d", "s2u1.a1", True),
                 ("ConvSeg", "s2u1.t", None), (stats, "s2u1.t", None), ("bn_apply", "s2u1.a2", (True, None)),
                 ("conv_igemm", "idn64", False), ("conv_igemm", "s2u1.out", False)],
    }


# Backward visits s3u2, s3u1, s2u2, s2u1, s1u2, s1u1 (i = 0 .. 5): gt alternates with i & 1, the unit's input gradient
# rotates with (i + 1) % 3, and a unit's output gradient is the previous unit's input gradient.
GT = {"s1u1": "gt_32_1", "s1u2": "gt_32_0", "s2u1": "gt_64_1"}
GA2 = {"s1u1": "ga2_32", "s1u2": "ga2_32", "s2u1": "ga2_64"}
G_OUT = {"s1u1": "g_in32_32_2", "s1u2": "g_in32_32_1", "s2u1": "g_in64_16_0"}
G_IN = {"s1u1": "g_in32_32_0", "s1u2": "g_in32_32_2", "s2u1": "g_in32_32_1"}
GA1 = "ga1_32_32"


def _pair(form, w, ga, gt, gx_add=None):
    """The (conv, preceding BatchNorm) pair of the dense kernels in its four forms."""
    if form == "split":
        return [("conv_igemm", ga, False), ("conv_wgrad", w, True), ("bn_bwd_cus", gt, gx_add)]
    if form == "shared":
        return [("conv_igemm_bnbwd", ga, False), ("conv_wgrad", w, True), ("bn_bwd_fused", gt, True)]
    if form == "fused":
        return [("conv_wgrad", w, False), ("conv_igemm_bnbwd", ga, False), ("bn_bwd_fused", gt, False)]
    return [("conv_wgrad", w, False), ("conv_igemm", ga, False), ("bn_bwd", gt, None)]


def _bwd(form):
    want = {}
    for k in ASSERTED:
        c1, c2, sc = W[k]
        want[k] = _pair(form, c2, GA2[k], GT[k])
        if sc is None:      # dense unit: the unit's output gradient joins bn1's backward
            want[k] += _pair(form, c1, GA1, G_IN[k], gx_add=G_OUT[k])
        elif form == "split" and k == "s2u1":
            # strided slice-list unit: both data gradients in one launch, conv1's weight gradient budgeted beside bn1's
            # confined backward, the shortcut's on all CUs
            want[k] += [("ConvSeg", GA1, None), ("conv_wgrad", c1, True), ("conv_wgrad", sc, False),
                        ("bn_bwd_cus", G_IN[k], None)]
        else:
            want[k] += [("conv_wgrad", c1, False), ("conv_wgrad", sc, False), ("ConvSeg", GA1, None),
                        ("bn_bwd", G_IN[k], None)]
    return want


@pytest.fixture(scope="module")
def wrn():
    eng = E.WRNEngine(num_classes=10, blocks=16, width_factor=2, device=DEV, seed=0)
    assert [u["key"] for u in eng.units] == ["s1u1", "s1u2", "s2u1", "s2u2", "s3u1", "s3u2"]
    return eng


def _train(eng):
    g = torch.Generator().manual_seed(41)
    x, gz = torch.randn(B, 3, 32, 32, generator=g).to(DEV), (0.01 * torch.randn(B, 10, generator=g)).to(DEV)
    eng.zero_grad()
    with Recorder(eng) as fwd:
        eng.forward(x, training=True)
    with Recorder(eng) as bwd:
        eng.backward(gz)
    torch.cuda.synchronize()
    return fwd, bwd


def _forward_slices(eng, rec):
    """{unit key: (start, end)}: a unit ends at the launch that writes key.out; the slices tile the trace between the
    stem conv and the head's three launches."""
    out = [t[1] for t in rec.trace]
    sl, at = {}, 1
    for u in eng.units:
        end = out.index(u["key"] + ".out") + 1
        sl[u["key"]], at = (at, end), end
    assert at == len(out) - 3
    return sl


def _backward_slices(eng, rec):
    """{unit key: (start, end)}: a unit starts at conv2's data gradient into ga2 (or, in the forms that issue conv2's
    weight gradient first, at that weight gradient) and ends where the next one starts, the last at the stem's."""
    starts = []
    for i, t in enumerate(rec.trace):
        if t[1].startswith("ga2_"):
            starts.append(i - 1 if rec.trace[i - 1][0] == "conv_wgrad" else i)
    order = [u["key"] for u in reversed(eng.units)]
    assert len(starts) == len(order) and starts[0] == 2
    bounds = starts + [len(rec.trace) - 1]
    return {k: (bounds[i], bounds[i + 1]) for i, k in enumerate(order)}


def _check(eng, stats, form, two_streams):
    fwd, bwd = _train(eng)
    assert fwd.trace[0] == ("stem_conv", "x0", None)
    assert fwd.trace[-3:] == [(stats, "s3u2.out", None), ("bn_relu_pool", "pooled", None), ("linear_fwd", "z", None)]
    fs, want = _forward_slices(eng, fwd), _fwd(stats)
    for k in ASSERTED:
        assert fwd.trace[slice(*fs[k])] == want[k], (k, fwd.trace[slice(*fs[k])])
    assert not any(fwd.side)
    assert bwd.trace[:2] == [("linear_bwd", "gpool", None), ("pool_bn_bwd", "g_out128", None)]
    assert bwd.trace[-1] == ("stem_wgrad", "features.init_block.weight", None)
    bs, want = _backward_slices(eng, bwd), _bwd(form)
    for k in ASSERTED:
        assert bwd.trace[slice(*bs[k])] == want[k], (k, bwd.trace[slice(*bs[k])])
    for t, side in zip(bwd.trace, bwd.side):
        assert side == (two_streams and t[0] == "conv_wgrad"), t
    # what a side-stream weight gradient of one unit reads, no main-stream launch of the next unit writes
    order = [u["key"] for u in reversed(eng.units)]
    spans = [bs[k] for k in order] + [(len(bwd.trace) - 1, len(bwd.trace))]
    for (a, b), (c, d) in zip(spans, spans[1:]):
        read = set().union(*(bwd.reads[i] for i in range(a, b) if bwd.side[i]))
        written = {bwd.trace[i][1] for i in range(c, d) if not bwd.side[i]}
        assert not read & written, (read & written, bwd.trace[a:b], bwd.trace[c:d])


def _shared(eng, form):
    """The CU split is MI355X's (256 CUs, 8 XCDs): elsewhere set_cu_share() leaves the sharing off."""
    return form if ops.cu_topology_is_mi355x(eng.device) else "fused"


def test_split_schedule(wrn):
    wrn.set_cu_share(47.0, calibrate=False)
    _check(wrn, "bn_finalize", _shared(wrn, "split"), True)


def test_split_schedule_on_one_stream_is_the_plain_one(wrn):
    wrn.set_cu_share(47.0, calibrate=False)
    wrn.set_overlap(False)
    try:
        _check(wrn, "bn_finalize", _shared(wrn, "plain"), False)
    finally:
        wrn.set_overlap(True)


def test_fused_schedule_with_sharing(wrn):
    wrn.set_cu_share(47.0, calibrate=False, split_reduce=False)
    _check(wrn, "bn_finalize", _shared(wrn, "shared"), True)


def test_fused_schedule(wrn):
    wrn.set_cu_share(None)
    _check(wrn, "bn_finalize", "fused", True)


def test_fused_schedule_on_one_stream(wrn):
    wrn.set_cu_share(None)
    wrn.set_overlap(False)
    try:
        _check(wrn, "bn_finalize", "fused", False)
    finally:
        wrn.set_overlap(True)


def test_plain_schedule_without_fused_statistics(wrn):
    wrn.set_cu_share(47.0, calibrate=False)
    wrn.fuse_stats = False
    try:
        _check(wrn, "bn_stats", "plain", True)
    finally:
        wrn.fuse_stats = True
