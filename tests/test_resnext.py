"""ResNeXt and wide ResNets without a GPU: the restatement (tests/_resnext_ref.py) has torchvision's parameter counts, names
and shapes; the public surface names the four architectures; every grouped-convolution entry validates its arguments
before any device work; and a host restatement of the weight expansion is the dense block-diagonal matrix."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import nbdt_path

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_group_cases as G  # noqa: E402
import _resnext_ref as R  # noqa: E402
from nbdt import _C, models  # noqa: E402

NAMES = sorted(R.ARCHS)
ENTRIES = ("nbdt_conv_group_weight_prep", "nbdt_conv_group_weight_prep_batched", "nbdt_conv_group_fwd",
           "nbdt_conv_group_dgrad", "nbdt_conv_group_wgrad", "nbdt_ref_conv_group_fwd", "nbdt_ref_conv_group_dgrad",
           "nbdt_ref_conv_group_wgrad")


@pytest.mark.parametrize("name", NAMES)
def test_parameter_counts_are_torchvisions(name):
    with torch.device("meta"):         # shapes only: wide_resnet101_2 is 127 M parameters
        net = R.make(name)
    assert sum(p.numel() for p in net.parameters()) == R.PARAMS[name]


def test_state_dict_names_and_shapes():
    with torch.device("meta"):
        sx = {k: tuple(v.shape) for k, v in R.make("resnext50_32x4d").state_dict().items()}
        sw = {k: tuple(v.shape) for k, v in R.make("wide_resnet50_2").state_dict().items()}
        net = R.make("resnext50_32x4d")
    assert sx["layer1.0.conv2.weight"] == (128, 4, 3, 3) and sx["layer4.0.conv2.weight"] == (1024, 32, 3, 3)
    assert sw["layer4.2.conv2.weight"] == (1024, 1024, 3, 3) and sw["layer4.2.conv3.weight"] == (2048, 1024, 1, 1)
    assert sx["layer1.0.conv1.weight"] == (128, 64, 1, 1) and sx["layer1.0.conv3.weight"] == (256, 128, 1, 1)
    assert sx["layer2.0.downsample.0.weight"] == (512, 256, 1, 1) and sx["fc.weight"] == (1000, 2048)
    assert set(sx) == set(sw)          # one name pattern: conv1, bn1, layerN.M.conv{1,2,3} / bnK, downsample.0/1, fc
    for key in sx:
        assert key.split(".")[0] in ("conv1", "bn1", "layer1", "layer2", "layer3", "layer4", "fc"), key
    # the stride sits on conv2 (v1.5), and conv2 is the grouped one
    blk = net.layer3[0]
    assert blk.conv1.stride == (1, 1) and blk.conv2.stride == (2, 2) and blk.conv3.stride == (1, 1)
    assert blk.conv2.groups == 32 and blk.conv1.groups == 1 and net.layer3[1].conv2.stride == (1, 1)


def test_public_surface_names_the_four_architectures():
    assert set(NAMES) <= set(models.get_model_choices())
    assert "resnext101_32x8d" not in models.get_model_choices() and not hasattr(models, "resnext101_32x8d")
    spec = importlib.util.spec_from_file_location("nbdt_main_rx", os.path.join(nbdt_path.PKG_DIR, "main.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    for name in NAMES:
        a = M.build_parser().parse_args(f"--arch {name} --hierarchy induced-efficientnet_b7b --loss SoftTreeSupLoss".split())
        assert a.arch == name
        with pytest.raises(NotImplementedError):
            getattr(models, name)(pretrained=True)


def test_cabi_declares_the_grouped_entries():
    assert set(ENTRIES) <= set(_C.SIGNATURES)
    assert _C.lib().nbdt_version() >= 125
    assert set(ENTRIES) <= set(_C.exported_symbols())


# ------------------------------------------------------------------------------------------------------------------------
# refusals: fake non-null pointers, never dereferenced -- every refusal comes before the first HIP call

P = _C.c_void_p
GOOD = dict(B=2, H=8, W=8, width=64, cg=8, stride=1)


def _call(entry, null=None, **over):
    a = dict(GOOD, **over)
    ptrs = [None if null == i else P(0x1000 * (i + 1)) for i in range(3)]
    geo = [a["B"], a["H"], a["W"], a["width"], a["cg"], a["stride"]]
    lib = _C.lib()
    if entry == "nbdt_conv_group_fwd":
        rc = lib.nbdt_conv_group_fwd(*ptrs, *geo, None, None, 0, None)
    elif entry.endswith("dgrad"):
        rc = getattr(lib, entry)(*ptrs, *geo, a.get("accumulate", 0), None)
    else:
        rc = getattr(lib, entry)(*ptrs, *geo, None)
    return rc, lib.nbdt_last_error()


LAUNCHES = [e for e in ENTRIES if "weight_prep" not in e]
BAD = {"width % 32": (dict(width=48), b"multiple of 32"), "cg = 64": (dict(width=128, cg=64), b"4, 8, 16 or 32"),
       "cg = 12": (dict(width=96, cg=12), b"4, 8, 16 or 32"), "cg = 2": (dict(cg=2), b"4, 8, 16 or 32"),
       "stride 3": (dict(stride=3), b"stride is 1 or 2"), "stride 0": (dict(stride=0), b"stride is 1 or 2"),
       "odd side at stride 2": (dict(H=7, W=7, stride=2), b"even input sides"),
       "odd width at stride 2": (dict(H=8, W=7, stride=2), b"even input sides"),
       "empty batch": (dict(B=0), b"empty batch")}


@pytest.mark.parametrize("entry", LAUNCHES)
def test_every_launch_refuses_bad_arguments_without_a_gpu(entry):
    for what, (over, msg) in BAD.items():
        rc, err = _call(entry, **over)
        assert rc == -1 and msg in err, (entry, what, rc, err)
    for i in range(3):
        rc, err = _call(entry, null=i)
        assert rc == -1 and b"null argument" in err, (entry, i, rc, err)
    if entry.endswith("dgrad"):
        rc, err = _call(entry, accumulate=1)
        assert rc == -1 and b"no accumulate form" in err, (entry, rc, err)


def test_eval_epilogue_and_weight_prep_refusals():
    lib = _C.lib()
    geo = [2, 8, 8, 64, 8, 1]
    a, b, c = P(0x1000), P(0x2000), P(0x3000)
    assert lib.nbdt_conv_group_fwd(a, b, c, *geo, P(0x4000), None, 1, None) == -1      # scale without shift
    assert b"come together" in lib.nbdt_last_error()
    assert lib.nbdt_conv_group_fwd(a, b, c, *geo, None, None, 1, None) == -1           # an activation without the affine
    assert b"act" in lib.nbdt_last_error()
    assert lib.nbdt_conv_group_fwd(a, b, c, *geo, P(0x4000), P(0x5000), 7, None) == -1
    assert lib.nbdt_conv_group_weight_prep(None, 64, 8, b, c, None) == -1 and b"null argument" in lib.nbdt_last_error()
    assert lib.nbdt_conv_group_weight_prep(a, 64, 8, None, None, None) == -1 and b"null argument" in lib.nbdt_last_error()
    assert lib.nbdt_conv_group_weight_prep(a, 48, 8, b, c, None) == -1 and b"multiple of 32" in lib.nbdt_last_error()
    assert lib.nbdt_conv_group_weight_prep(a, 128, 64, b, c, None) == -1 and b"4, 8, 16 or 32" in lib.nbdt_last_error()
    assert lib.nbdt_conv_group_weight_prep_batched(a, None, 1, 2, b, c, None) == -1
    assert lib.nbdt_conv_group_weight_prep_batched(a, b, 0, 2, c, c, None) == -1 and b"layer table" in lib.nbdt_last_error()


# ------------------------------------------------------------------------------------------------------------------------
# the weight expansion

@pytest.mark.parametrize("width,cg", G.CONFIGS + [(32, 32), (96, 8)])
def test_host_expansion_is_the_dense_block_diagonal_matrix(width, cg):
    rng = np.random.default_rng(width + cg)
    master = rng.integers(1, 100, size=(width, 9, cg)).astype(np.float32)      # no zero entry: zeros below are structural
    dense = G.dense_block_diagonal(master)
    wf, wd = G.expand_host(master)
    assert wf.shape == wd.shape == (width // 32, 32, 9, 32)
    covered = np.zeros_like(dense, dtype=bool)
    for n in range(width // 32):
        sl = slice(32 * n, 32 * n + 32)
        assert np.array_equal(wf[n], dense[sl, :, sl])
        covered[sl, :, sl] = True
        # the data-gradient copy: transposed, taps reversed
        assert np.array_equal(wd[n], wf[n][:, ::-1, :].transpose(2, 1, 0))
        # explicit zeros off the group diagonal, none on it
        same = (np.arange(32)[:, None] // cg) == (np.arange(32)[None, :] // cg)
        assert np.array_equal(wf[n] != 0, np.broadcast_to(same[:, None, :], (32, 9, 32)))
    assert not dense[~covered].any()        # nothing of the dense matrix lies outside the 32 x 32 diagonal blocks
    assert (dense != 0).sum() == width * 9 * cg


def test_integer_fixtures_are_exactly_representable():
    """Every expected value of every per-op case is an integer of magnitude <= 256 (integer_case asserts it, and that fp32
    equals fp64 on the CPU); the figures the bound leaves room for are printed."""
    worst = {"fwd": 0, "gx": 0, "dw": 0}
    for case in G.CASES:
        c = G.integer_case(case)
        for k in worst:
            worst[k] = max(worst[k], int(c[k].abs().max().item()))
    print("largest |expected| over the cases:", worst)
    assert max(worst.values()) <= G.EXACT_MAX
