"""EfficientNet-B1..B7 and the TF-padded b0b..b7b (host side): the configuration table against the published sizes,
state_dict names against the test module's PyTorch restatement, the padding rule, the C ABI of the padded strided
convolutions and their refusals (no device call: the pointers are null), the model registry."""
import math
import os

import pytest
import torch

import nbdt_path
from nbdt import _C, models, ops
from nbdt.engine_effnet import B0_STAGES, efficientnet_config, efficientnet_layout

from _effnet_family_ref import EfficientNetRef, same_pad

# version: (parameters at 1000 classes, units, stem, final, widest expanded, widest SE squeeze) -- the published sizes
TABLE = {
    "b0": (5288548, 16, 32, 1280, 1152, 48), "b1": (7794184, 23, 32, 1280, 1920, 80),
    "b2": (9109994, 23, 32, 1408, 2112, 88), "b3": (12233232, 26, 40, 1536, 2304, 96),
    "b4": (19341616, 32, 48, 1792, 2688, 112), "b5": (30389784, 39, 48, 2048, 3072, 128),
    "b6": (43040704, 45, 56, 2304, 3456, 144), "b7": (66347960, 55, 64, 2560, 3840, 160),
}
NATIVE = {"b0": (224, 0.2), "b1": (240, 0.2), "b2": (260, 0.3), "b3": (300, 0.3), "b4": (380, 0.4), "b5": (456, 0.4),
          "b6": (528, 0.5), "b7": (600, 0.5)}
NEW_FUNCTIONS = ["nbdt_dwconv_fwd_pad", "nbdt_dwconv_bwd_data_pad", "nbdt_dwconv_bwd_weight_pad", "nbdt_stem_conv_pad",
                 "nbdt_stem_wgrad_pad", "nbdt_ref_dwconv_fwd_pad", "nbdt_ref_dwconv_bwd_data_pad",
                 "nbdt_ref_dwconv_bwd_weight_pad", "nbdt_ref_stem_conv_pad", "nbdt_ref_stem_wgrad_pad"]


@pytest.mark.parametrize("version", sorted(TABLE))
def test_configuration_gives_the_published_sizes(version):
    params, units, stem, final, widest, squeeze = TABLE[version]
    c = efficientnet_config(version)
    assert sum(len(sp) for _, sp in c["stages"]) == units
    assert (c["init_channels"], c["final_channels"]) == (stem, final)
    assert (c["in_size"], c["dropout_rate"]) == NATIVE[version]
    assert sum(math.prod(shape) for _, shape in efficientnet_layout(c, 1000)) == params
    cin, wide, sq = c["init_channels"], 0, 0
    for _, specs in c["stages"]:
        for cout, k, exp in specs:
            wide, sq, cin = max(wide, cin * exp), max(sq, cin * exp // (4 * exp)), cout
    assert (wide, sq) == (widest, squeeze)
    assert len(c["stages"]) == 5 and [s for s, _ in c["stages"]] == [1, 2, 2, 2, 2]
    assert units <= _C.NBDT_SD_MAX_UNITS and squeeze <= 256 and stem <= 72      # limits of the kernels
    assert c["bn_eps"] == 1e-5 and c["tf_mode"] is False
    # the `b` twin: eps and padding mode, nothing else
    t = efficientnet_config(version, tf_mode=True)
    assert t["bn_eps"] == 1e-3 and t["tf_mode"] is True
    assert {k: v for k, v in t.items() if k not in ("bn_eps", "tf_mode")} == \
           {k: v for k, v in c.items() if k not in ("bn_eps", "tf_mode")}


def test_b0_configuration_is_the_engine_default():
    assert efficientnet_config("b0")["stages"] == B0_STAGES
    with pytest.raises(ValueError, match="unknown EfficientNet version"):
        efficientnet_config("b8")


@pytest.mark.parametrize("version,tf_mode", [("b2", False), ("b5", True)])
def test_state_dict_names_and_shapes_follow_from_the_configuration(version, tf_mode):
    config = efficientnet_config(version, tf_mode)
    ref = EfficientNetRef(config, num_classes=1000)
    want = [(n, tuple(p.shape)) for n, p in ref.named_parameters()]
    assert efficientnet_layout(config, 1000) == want
    assert sum(p.numel() for p in ref.parameters()) == TABLE[version][0]
    assert all(m.eps == config["bn_eps"] for m in ref.modules() if isinstance(m, torch.nn.BatchNorm2d))
    for name in ("features.stage3.unit1.conv1.conv.weight", "features.stage5.unit1.conv1.conv.weight"):   # grad_buckets
        assert name in dict(want)


def test_padding_rule():
    assert [ops.conv_padding(h, k, 2, same=True) for k, h in ((3, 8), (5, 8), (3, 15), (5, 15))] == \
           [(0, 1), (1, 2), (1, 1), (2, 2)]
    for k in (3, 5):
        for h in (7, 8, 15, 16):
            assert ops.conv_padding(h, k, 1, same=True) == ops.conv_padding(h, k, 1) == (k // 2, k // 2)
            assert ops.conv_padding(h, k, 2) == (k // 2, k // 2)
            assert ops.conv_out_size(h, 2) == (h + 1) // 2 and ops.conv_out_size(h, 1) == h
            # the restatement's F.pad agrees
            x = torch.zeros(1, 1, h, h)
            lo, hi = ops.conv_padding(h, k, 2, same=True)
            assert same_pad(x, k, 2).shape[2] == h + lo + hi
            assert (h + lo + hi - k) // 2 + 1 == ops.conv_out_size(h, 2)
    # the chains of the issue: native side -> stem -> stride-2 stages
    for side, chain in ((240, [120, 60, 30, 15, 8]), (260, [130, 65, 33, 17, 9]), (300, [150, 75, 38, 19, 10]),
                        (456, [228, 114, 57, 29, 15]), (600, [300, 150, 75, 38, 19])):
        got, h = [], side
        for _ in chain:
            h = ops.conv_out_size(h, 2)
            got.append(h)
        assert got == chain


def test_new_functions_are_declared_bound_and_exported():
    text = open(os.path.join(nbdt_path.ROOT, "include", "nbdt_hip.h")).read()
    assert "padded strided convolutions (nbdt_version() >= 126)" in text
    section = text.split("padded strided convolutions (nbdt_version() >= 126)")[1]
    exported = set(_C.exported_symbols())
    for fn in NEW_FUNCTIONS:
        assert f"int {fn}(" in section and fn in _C.SIGNATURES and fn in exported, fn
    assert _C.lib().nbdt_version() >= 126


def _refused(rc, what):
    assert rc == -1, what                    # NBDT_EINVAL
    msg = _C.lib().nbdt_last_error()
    assert msg, what
    return msg


@pytest.mark.parametrize("fn", NEW_FUNCTIONS)
def test_bad_geometry_is_refused_before_any_device_call(fn):
    """pad_lo outside [0, k / 2], k not 3 or 5, stride not 1 or 2, non-positive extents: NBDT_EINVAL with a message, from
    null device pointers (a call that got as far as a launch would fault or report a HIP error instead)."""
    f = getattr(_C.lib(), fn)
    stem, tail = "stem" in fn, (None, None, None) if fn == "nbdt_dwconv_fwd_pad" else (None, None)

    def call(B=2, H=9, W=9, C=32, k=3, stride=2, pt=1, pl=1):
        if stem:        # (img, w, B, H, W, cout_real, cpad, stride, pad_top, pad_left, out, stream)
            return f(None, None, B, H, W, 32, C, stride, pt, pl, *tail)
        return f(None, None, B, H, W, C, k, stride, pt, pl, *tail)

    assert b"padding" in _refused(call(pt=2), "pad_top > k / 2")
    assert b"padding" in _refused(call(pl=-1), "pad_left < 0")
    assert b"stride" in _refused(call(stride=3), "stride 3")
    assert b"stride" in _refused(call(stride=0), "stride 0")
    assert b"empty" in _refused(call(H=0), "H = 0")
    assert b"empty" in _refused(call(W=-4), "W < 0")
    assert b"empty" in _refused(call(B=0), "B = 0")
    assert b"stride 1" in _refused(call(stride=1, pt=0, pl=0), "stride 1 with SAME-style padding")
    if not stem:
        assert b"3 or 5" in _refused(call(k=7, pt=3, pl=3), "k = 7")
        assert b"3 or 5" in _refused(call(k=4), "k = 4")
        assert b"padding" in _refused(call(k=5, pt=3, pl=2), "pad_top > 2 at k = 5")
    _refused(call(), "null tensors")         # a good geometry still refuses null pointers


def test_registry_holds_the_family():
    names = [f"efficientnet_b{i}{s}" for s in ("", "b") for i in range(8)]
    choices = models.get_model_choices()
    assert len(set(choices)) == len(choices)
    for n in names:
        assert n in choices and n in models.__all__
        f = getattr(models, n)
        assert hasattr(f.engine_cls, "set_stochastic_depth") and f.__name__ == n
    for old in ("ResNet18", "wrn28_10_cifar10", "resnet50", "resnext50_32x4d", "efficientnet_b0"):
        assert old in choices
    assert len(choices) == 19 + 15
    assert models.efficientnet_b7b.config == efficientnet_config("b7", True)
    assert models.efficientnet_b3.config["in_size"] == 300
