"""ImageNet-style ResNets without a GPU: the restatement tests/_imagenet_resnet_ref.py against torchvision's published
parameter counts and shapes, argument validation of the three new C entries, the factory names and the driver's flags."""
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

import nbdt_path

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _imagenet_resnet_ref as R  # noqa: E402

from nbdt import _C, models  # noqa: E402

# torchvision.models.resnet*, 1000 classes (the model cards' "num_params")
PARAMS = {"resnet18": 11689512, "resnet34": 21797672, "resnet50": 25557032, "resnet101": 44549160, "resnet152": 60192808}


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_restatement_has_torchvisions_parameter_count(name):
    net = R.make(name)
    assert sum(p.numel() for p in net.parameters()) == PARAMS[name]
    sd = net.state_dict()
    assert tuple(sd["conv1.weight"].shape) == (64, 3, 7, 7)
    assert "fc.weight" in sd and "fc.bias" in sd and tuple(sd["fc.weight"].shape)[0] == 1000
    assert "layer1.0.bn1.running_mean" in sd and "layer4.0.downsample.1.weight" in sd
    # torchvision's names and nothing else: conv1, bn1, layerN.M.{convK, bnK, downsample.0/1}, fc
    pat = re.compile(r"^(conv1\.weight|bn1\.\w+|fc\.(weight|bias)|layer[1-4]\.\d+\.(conv[123]\.weight|bn[123]\.\w+|"
                     r"downsample\.0\.weight|downsample\.1\.\w+))$")
    assert all(pat.match(k) for k in sd), [k for k in sd if not pat.match(k)][:5]


def test_restatement_shapes_and_v1_5_stride():
    r18, r50 = R.make("resnet18"), R.make("resnet50")
    assert tuple(r18.state_dict()["layer2.0.downsample.0.weight"].shape) == (128, 64, 1, 1)
    assert tuple(r50.state_dict()["layer2.0.downsample.0.weight"].shape) == (512, 256, 1, 1)
    assert "layer1.0.downsample.0.weight" not in r18.state_dict() and "layer1.0.downsample.0.weight" in r50.state_dict()
    blk = r50.layer2[0]
    assert blk.conv1.stride == (1, 1) and blk.conv2.stride == (2, 2) and blk.conv3.stride == (1, 1)      # v1.5
    assert tuple(r50.state_dict()["layer4.2.conv3.weight"].shape) == (2048, 512, 1, 1)
    small = R.make("resnet50", 10, num_blocks=(1, 1, 1, 1), zero_init_residual=True)
    assert small.layer3[0].bn3.weight.abs().sum().item() == 0 and small.layer3[0].bn2.weight.min().item() == 1
    with torch.no_grad():
        assert tuple(small(torch.randn(2, 3, 64, 64)).shape) == (2, 10)
        assert tuple(F.max_pool2d(small.stem(torch.randn(1, 3, 64, 64)), 3, 2, 1).shape) == (1, 64, 16, 16)


def test_new_entries_validate_their_arguments_without_a_gpu():
    """null pointers, odd H, C % 8 != 0, cpad < 3*k*k and even k: NBDT_EINVAL and a message, before any HIP call."""
    lib = _C.lib()
    assert lib.nbdt_version() >= 115
    p = 4096            # any non-null "pointer": a refused call never dereferences it
    BF = _C.NBDT_BF16

    def refused(rc, text):
        assert rc == -1
        assert text in lib.nbdt_last_error(), lib.nbdt_last_error()

    # nbdt_stem_patches(img, B, H, W, k, stride, cpad, dtype, out, stream)
    refused(lib.nbdt_stem_patches(None, 1, 32, 32, 7, 2, 160, BF, p, None), b"null")
    refused(lib.nbdt_stem_patches(p, 1, 32, 32, 7, 2, 160, BF, None, None), b"null")
    refused(lib.nbdt_stem_patches(p, 1, 32, 32, 7, 2, 128, BF, p, None), b"cpad")            # 128 < 147
    refused(lib.nbdt_stem_patches(p, 1, 32, 32, 7, 2, 152, BF, p, None), b"cpad")            # not a multiple of 32
    refused(lib.nbdt_stem_patches(p, 1, 32, 32, 6, 2, 160, BF, p, None), b"odd")             # even k
    refused(lib.nbdt_stem_patches(p, 1, 32, 32, 9, 2, 256, BF, p, None), b"at most 7")
    refused(lib.nbdt_stem_patches(p, 1, 33, 32, 7, 2, 160, BF, p, None), b"divisible")       # no clamp
    refused(lib.nbdt_stem_patches(p, 1, 32, 32, 7, 3, 160, BF, p, None), b"stride")
    refused(lib.nbdt_stem_patches(p, 1, 32, 32, 7, 2, 160, _C.NBDT_F16, p, None), b"bf16")
    refused(lib.nbdt_stem_patches(p, 0, 32, 32, 7, 2, 160, BF, p, None), b"empty")
    # nbdt_maxpool3x3s2_fwd(x, dtype, B, H, W, C, y, idx, stream)
    refused(lib.nbdt_maxpool3x3s2_fwd(None, BF, 1, 8, 8, 64, p, None, None), b"null")
    refused(lib.nbdt_maxpool3x3s2_fwd(p, BF, 1, 8, 8, 64, None, None, None), b"null")
    refused(lib.nbdt_maxpool3x3s2_fwd(p, BF, 1, 7, 8, 64, p, None, None), b"even")
    refused(lib.nbdt_maxpool3x3s2_fwd(p, BF, 1, 8, 9, 64, p, None, None), b"even")
    refused(lib.nbdt_maxpool3x3s2_fwd(p, BF, 1, 8, 8, 60, p, None, None), b"multiple of 8")
    refused(lib.nbdt_maxpool3x3s2_fwd(p, _C.NBDT_U8, 1, 8, 8, 64, p, None, None), b"bf16")
    # nbdt_maxpool3x3s2_bwd(gy, idx, dtype, B, H, W, C, gx, stream)
    refused(lib.nbdt_maxpool3x3s2_bwd(None, p, BF, 1, 8, 8, 64, p, None), b"null")
    refused(lib.nbdt_maxpool3x3s2_bwd(p, None, BF, 1, 8, 8, 64, p, None), b"null")           # the backward needs the positions
    refused(lib.nbdt_maxpool3x3s2_bwd(p, p, BF, 1, 8, 8, 64, None, None), b"null")
    refused(lib.nbdt_maxpool3x3s2_bwd(p, p, BF, 1, 9, 8, 64, p, None), b"even")
    refused(lib.nbdt_maxpool3x3s2_bwd(p, p, BF, 1, 8, 8, 12, p, None), b"multiple of 8")


def test_factories_and_driver_flags():
    names = ("resnet18", "resnet34", "resnet50", "resnet101", "resnet152")
    assert all(n in models.get_model_choices() for n in names)
    assert all(n in models.get_model_choices() for n in ("ResNet18", "ResNet50", "efficientnet_b0"))     # ... beside the old ones
    for n in names:
        with pytest.raises(NotImplementedError, match="pretrained"):
            getattr(models, n)(pretrained=True)
    sys.path.insert(0, nbdt_path.PKG_DIR)
    import main
    args = main.build_parser().parse_args("--arch resnet18 --weight-decay 1e-4".split())
    assert args.arch == "resnet18" and args.weight_decay == 1e-4
    assert main.build_parser().parse_args([]).weight_decay == 5e-4


def test_imagenet_engines_refuse_the_cpu():
    from nbdt import engine as E
    assert issubclass(E.ImageNetResNetEngine, E.ResNetEngine) and issubclass(E.ImageNetBottleneckEngine, E.BottleneckEngine)
    assert E.ImageNetResNetEngine.classifier_names == ("fc.weight", "fc.bias") and E.ImageNetResNetEngine.res_share is None
    assert E.ResNetEngine.classifier_names == ("linear.weight", "linear.bias") and E.ResNetEngine.res_share is not None
    with pytest.raises(RuntimeError):
        E.ImageNetResNetEngine(device="cpu")
