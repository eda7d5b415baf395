"""Bottleneck ResNets without a GPU: the fp32 restatement (tests/_bottleneck_ref.py) is the reference's ResNet50
(golden recorded by tests/golden/make_bottleneck_golden.py), the public surface names the three architectures, and
nbdt_conv_pw validates its arguments before any device work."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import nbdt_oracle as O
import nbdt_path

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bottleneck_ref as R  # noqa: E402
from nbdt import _C, models, ops  # noqa: E402


def test_restatement_is_the_reference_resnet50(golden_dir, pkg_dir):
    """Same seed -> the same parameters under the same state-dict names in the same order, the same train-mode logits,
    the same SoftTreeSupLoss (numpy oracle on these logits), per-parameter gradient norms and running statistics."""
    g = np.load(os.path.join(golden_dir, "backbone_resnet50_cifar10.npz"))
    torch.manual_seed(int(g["seed"]))
    net = R.ResNet50(num_classes=10)
    net.train()
    sd = net.state_dict()
    assert list(sd.keys()) == list(g["keys"])
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    np.testing.assert_allclose(sums, g["param_sums"], rtol=1e-6, atol=1e-9)
    x, y = torch.from_numpy(g["x"]), g["y"]
    z = net(x)
    np.testing.assert_allclose(z.detach().numpy(), g["logits"], rtol=1e-5, atol=1e-5)
    otree = O.OracleTree(*O.default_paths("CIFAR10", "induced-ResNet18", pkg_dir))
    loss, dz = O.soft_tree_sup_loss(otree, z.detach().numpy(), y)
    assert abs(loss - float(g["loss"])) <= 1e-6 * abs(float(g["loss"])), (loss, float(g["loss"]))
    z.backward(torch.from_numpy(dz))
    assert [n for n, _ in net.named_parameters()] == list(g["grad_names"])
    gn = np.array([float(p.grad.double().norm()) for _, p in net.named_parameters()])
    np.testing.assert_allclose(gn, g["grad_norms"], rtol=1e-4, atol=1e-7)
    sd = net.state_dict()
    np.testing.assert_allclose(sd["bn1.running_mean"].numpy(), g["bn1_running_mean"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(sd["layer4.2.bn3.running_var"].numpy(), g["last_running_var"], rtol=1e-6, atol=1e-6)


def test_public_surface_names_the_bottleneck_resnets():
    choices = models.get_model_choices()
    assert {"ResNet50", "ResNet101", "ResNet152"} <= set(choices)
    spec = importlib.util.spec_from_file_location("nbdt_main_bn", os.path.join(nbdt_path.PKG_DIR, "main.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    a = M.build_parser().parse_args("--arch ResNet50 --hierarchy induced-ResNet18 --loss SoftTreeSupLoss".split())
    assert a.arch == "ResNet50"
    with pytest.raises(NotImplementedError):
        models.ResNet50(pretrained=True)


def test_cabi_declares_the_pointwise_entry():
    assert "nbdt_conv_pw" in _C.SIGNATURES
    assert _C.lib().nbdt_version() >= 113
    assert "nbdt_conv_pw" in set(_C.exported_symbols())


def _refused(desc, in_=1, w=1, out=1, partials=None):
    """nbdt_conv_pw on fake non-null pointers (never dereferenced: every refusal comes before the first launch)."""
    lib = _C.lib()
    P = _C.c_void_p
    rc = lib.nbdt_conv_pw(desc, P(0x1000) if in_ else None, P(0x2000) if w else None, P(0x3000) if out else None,
                          P(0x4000) if partials else None, None)
    return rc, lib.nbdt_last_error()


def test_pointwise_entry_refuses_without_a_gpu():
    EINVAL = -1
    cases = {
        "stride-2 1x1": _refused(ops.conv_fwd_desc(2, 8, 8, 64, 128, 1, 2)),
        "stride-2 1x1 data gradient": _refused(ops.conv_dgrad_descs(2, 8, 8, 64, 128, 1, 2, accumulate=True)[0]),
        "nine taps": _refused(ops.conv_fwd_desc(2, 8, 8, 64, 64, 3, 1)),
        "null in": _refused(ops.conv_fwd_desc(2, 8, 8, 64, 64, 1, 1), in_=0),
        "null w": _refused(ops.conv_fwd_desc(2, 8, 8, 64, 64, 1, 1), w=0),
        "null out": _refused(ops.conv_fwd_desc(2, 8, 8, 64, 64, 1, 1), out=0),
        "statistics with accumulate": _refused(ops.conv_dgrad_descs(2, 8, 8, 64, 64, 1, 1, accumulate=True)[0], partials=1),
    }
    d = ops.conv_fwd_desc(2, 8, 8, 64, 64, 1, 1)
    d.cin, d.in_ws = 48, 48
    cases["cin = 48"] = _refused(d)
    for what, (rc, msg) in cases.items():
        assert rc == EINVAL and len(msg) > 0, (what, rc, msg)
    assert b"null argument" in cases["null in"][1]
    assert b"multiple of 32" in cases["cin = 48"][1]
    assert b"one tap" in cases["nine taps"][1]
    assert b"stride-1" in cases["stride-2 1x1"][1]
    assert b"plain outputs" in cases["statistics with accumulate"][1]
