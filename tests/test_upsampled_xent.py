"""Cross-entropy on bilinearly upsampled logits, without a GPU: the interpolation contract (nbdt_upsample_taps /
nbdt_upsample_footprint run on the host), the refusals of nbdt_upsampled_xent ahead of any HIP call, the header and the
bindings, UpsampledCrossEntropyLoss on CPU tensors, and the dispatch decisions as pure host functions."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from nbdt import _C
from nbdt import loss as L

import _upsampled_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = (False, True)


# ------------------------------------------------------------------------------------ 1. taps and footprint

@pytest.mark.parametrize("ac", FLAGS)
@pytest.mark.parametrize("axis", U.AXES)
def test_taps_are_the_numpy_transcription_bit_for_bit(axis, ac):
    n_in, n_out = axis
    for d in range(n_out):
        i0, i1, l0, l1 = _C.upsample_taps(n_in, n_out, ac, d)
        r0, r1, m0, m1 = U.taps(n_in, n_out, ac, d)
        assert (i0, i1) == (r0, r1), (axis, ac, d)
        assert np.float32(l0).tobytes() == m0.tobytes() and np.float32(l1).tobytes() == m1.tobytes(), (axis, ac, d)
        assert 0 <= i0 <= i1 <= n_in - 1


@pytest.mark.parametrize("ac", FLAGS)
@pytest.mark.parametrize("axis", U.AXES)
def test_taps_against_torch_in_float64(axis, ac):
    """F.interpolate's linear map, from an identity basis in float64: 1e-6 per weight (fp32 rounding of the source index;
    6e-7 observed)."""
    n_in, n_out = axis
    A = U.matrix(n_in, n_out, ac, _C.upsample_taps)
    worst = np.abs(A - U.torch_matrix(n_in, n_out, ac)).max()
    print(f"{axis} align_corners={ac}: worst weight difference {worst:.2e}")
    assert worst <= 1e-6


@pytest.mark.parametrize("ac", FLAGS)
@pytest.mark.parametrize("axis", U.AXES)
def test_weights_of_a_destination_sum_to_one(axis, ac):
    n_in, n_out = axis
    for d in range(n_out):
        _, _, l0, l1 = _C.upsample_taps(n_in, n_out, ac, d)
        assert abs(float(np.float32(l0) + np.float32(l1)) - 1.0) <= 2 * np.finfo(np.float32).eps


@pytest.mark.parametrize("ac", FLAGS)
@pytest.mark.parametrize("axis", U.AXES)
def test_footprint_covers_every_tap_and_stays_narrow(axis, ac):
    n_in, n_out = axis
    A = U.matrix(n_in, n_out, ac, _C.upsample_taps)
    for i in range(n_in):
        lo, hi = _C.upsample_footprint(n_in, n_out, ac, i)
        assert 0 <= lo <= hi <= n_out - 1
        nonzero = np.nonzero(A[:, i])[0]
        assert nonzero.size and lo <= nonzero.min() and nonzero.max() <= hi, (axis, ac, i, lo, hi)
        assert hi - lo + 1 <= 2 * math.ceil(n_out / n_in) + 2, (axis, ac, i, lo, hi)


def test_taps_and_footprint_refuse_bad_arguments():
    lib = _C.lib()
    i, f = ctypes.c_int(), ctypes.c_float()
    bi, bf = ctypes.byref(i), ctypes.byref(f)
    assert lib.nbdt_upsample_taps(4, 8, 0, 8, bi, bi, bf, bf) == -1           # dst outside [0, out)
    assert lib.nbdt_upsample_taps(0, 8, 0, 0, bi, bi, bf, bf) == -1
    assert lib.nbdt_upsample_taps(4, 8, 0, 0, None, bi, bf, bf) == -1
    assert lib.nbdt_upsample_taps(4, (1 << 22) + 1, 0, 0, bi, bi, bf, bf) == -1
    assert lib.nbdt_upsample_footprint(8, 4, 0, 0, bi, bi) == -1              # downsampling
    assert lib.nbdt_upsample_footprint(4, 8, 0, 4, bi, bi) == -1              # source index outside [0, in)
    assert lib.nbdt_upsample_footprint(4, 8, 0, 0, None, bi) == -1


# ------------------------------------------------------------------------------------ 2. the entry's refusals

GOOD = dict(x=0x1000, xtype=0, N=2, C=5, h=3, w=4, xi=60, xc=12, y=0x2000, H=12, W=16, ac=0, ignore=255, weight=None,
            smoothing=0.0, grad_scale=1.0, workspace=0x3000, loss=0x4000, gx=0x5000)


def call(**changes):
    """nbdt_upsampled_xent on made-up addresses: a refusal returns before anything is dereferenced or launched."""
    a = dict(GOOD, **changes)
    rc = _C.lib().nbdt_upsampled_xent(a["x"], a["xtype"], a["N"], a["C"], a["h"], a["w"], a["xi"], a["xc"], a["y"], a["H"],
                                      a["W"], a["ac"], a["ignore"], a["weight"], a["smoothing"], a["grad_scale"],
                                      a["workspace"], a["loss"], a["gx"], None)
    return rc, _C.lib().nbdt_last_error().decode()


@pytest.mark.parametrize("changes, message", [
    (dict(x=None), "null buffer"), (dict(y=None), "null buffer"), (dict(workspace=None), "null buffer"),
    (dict(loss=None), "null buffer"), (dict(gx=None), "null buffer"),
    (dict(gx=0x1000), "aliased"), (dict(workspace=0x5000), "aliased"), (dict(loss=0x3000), "aliased"),
    (dict(weight=0x5000), "alias"),
    (dict(xtype=3), "dtype"), (dict(N=0), "empty"), (dict(C=0), "empty"),
    (dict(H=2), "downsampling"), (dict(W=3), "downsampling"),
    (dict(N=2, H=1 << 15, W=1 << 15), "2^31"), (dict(N=1 << 20, H=64, W=32), "2^31"),
    (dict(W=(1 << 22) + 1, N=1, H=3), "2^22"),
    (dict(C=4 * 65535 + 1, xi=(4 * 65535 + 1) * 12), "classes"),
    (dict(xc=11), "stride"), (dict(xi=59), "stride"),
    (dict(smoothing=1.0), "smoothing"), (dict(smoothing=-0.1), "smoothing"), (dict(smoothing=float("nan")), "smoothing"),
    (dict(weight=0x6000, smoothing=0.1), "not fused"),
    (dict(grad_scale=float("nan")), "grad_scale"),
])
def test_entry_refuses_before_any_device_call(changes, message):
    """NBDT_EINVAL (-1), never NBDT_EHIP: this process has no device, so any HIP call would have failed as such."""
    rc, err = call(**changes)
    assert rc == -1, (rc, err)
    assert message in err, err


def test_workspace_size():
    lib = _C.lib()
    assert lib.nbdt_upsampled_xent_workspace_floats(2, 17, 23) == 4 + 2 * 2 * 7 + 2 * 2 * 391    # 7 waves per image
    assert lib.nbdt_upsampled_xent_workspace_floats(0, 17, 23) == 4
    assert lib.nbdt_upsampled_xent_workspace_floats(2, 1 << 15, 1 << 15) == 4                     # refused by the entry


# ------------------------------------------------------------------------------------ 3. header and bindings

def test_header_bindings_and_version():
    with open(os.path.join(ROOT, "include", "nbdt_hip.h")) as f:
        header = f.read()
    names = ("nbdt_upsample_taps", "nbdt_upsample_footprint", "nbdt_upsampled_xent_workspace_floats",
             "nbdt_upsampled_xent")
    for name in names:
        assert re.search(r"\b(int|int64_t) " + name + r"\(", header), name
        assert name in _C.SIGNATURES and name in _C.exported_symbols(), name
    assert "nbdt_version() >= 133" in header
    limits = header[header.index("Size limits"):header.index("#ifndef NBDT_HIP_H")]
    assert "nbdt_upsampled_xent" in limits and "2^22" in limits
    assert _C.lib().nbdt_version() >= 133
    assert "UpsampledCrossEntropyLoss" in L.__all__


# ------------------------------------------------------------------------------------ 4. the module on CPU tensors

@pytest.mark.parametrize("ac", FLAGS)
@pytest.mark.parametrize("kind", ["plain", "smoothing", "weight", "weight+smoothing"])
def test_module_on_cpu_is_the_torch_composition(kind, ac):
    C, (h, w), (H, W) = 5, (5, 7), (17, 23)
    x = U.logits(2, C, h, w, 3).requires_grad_(True)
    y = U.targets(2, C, H, W, 4)
    weight = U.class_weights(C, 5) if "weight" in kind else None
    eps = 0.1 if "smoothing" in kind else 0.0
    crit = L.UpsampledCrossEntropyLoss(weight=weight, ignore_index=U.IGNORE, label_smoothing=eps, align_corners=ac)
    assert crit.route(x, y) == "composed"
    loss = crit(x, y)
    ref_x = x.detach().clone().requires_grad_(True)
    ref = F.cross_entropy(F.interpolate(ref_x, size=(H, W), mode="bilinear", align_corners=ac), y, weight,
                          ignore_index=U.IGNORE, label_smoothing=eps)
    assert torch.equal(loss, ref)
    loss.backward()
    ref.backward()
    assert torch.equal(x.grad, ref_x.grad)
    # targets at the logits' size: no interpolation at all
    same = U.targets(2, C, h, w, 6)
    assert torch.equal(crit(x, same), F.cross_entropy(x, same, weight, ignore_index=U.IGNORE, label_smoothing=eps))
    assert crit.route(x, same) == ("plain" if weight is None else "composed")


@pytest.mark.parametrize("kind", U.KINDS)
def test_fp32_composition_is_within_the_bounds(kind):
    """The bounds of tests/test_upsampled_xent_gpu.py (loss 1e-5 relative, gradient 1e-6 absolute against float64) are
    attainable in fp32: torch's own fp32 composition on the CPU keeps them on every case of that file."""
    worst = [0.0, 0.0]
    for pair, C, ac in U.CASES:
        x, y, weight, eps, ref_loss, ref_dx = U.standalone_case(pair, C, ac, kind)
        loss, dx = U.composition(x, y, ac, weight, eps, dtype=torch.float32)
        worst = [max(worst[0], abs(loss - ref_loss) / abs(ref_loss)), max(worst[1], np.abs(dx - ref_dx).max())]
        # the gather form on the library's taps is the same function (float64): what the adjoint test compares with
        g_loss, g_dx = U.gather_form(x, y, ac, _C.upsample_taps, weight, eps)
        assert abs(g_loss - ref_loss) <= 1e-6 * abs(ref_loss) and np.abs(g_dx - ref_dx).max() <= 1e-7
    print(f"{kind}: fp32 composition against float64: loss rel {worst[0]:.2e}, gradient abs {worst[1]:.2e}")
    assert worst[0] <= 1e-5 and worst[1] <= 1e-6


def test_module_state_and_repr():
    crit = L.UpsampledCrossEntropyLoss(weight=[1.0, 2.0], ignore_index=7, align_corners=True)
    assert "weight" in dict(crit.named_buffers()) and crit.weight.dtype == torch.float32
    assert crit.ignore_index == 7 and crit.align_corners is True and crit.label_smoothing == 0.0
    assert "align_corners=True" in repr(crit)
    assert L.UpsampledCrossEntropyLoss().weight is None


# ------------------------------------------------------------------------------------ 5. dispatch as host functions

f32, i64 = torch.float32, torch.int64


def test_criterion_route_is_a_host_function():
    route = L.upsampled_xent_route
    assert route(True, (2, 5, 3, 4), f32, (2, 12, 16), i64, False, 0.0) == "fused"
    assert route(True, (2, 5, 3, 4), torch.bfloat16, (2, 12, 16), i64, True, 0.0) == "fused"
    assert route(True, (2, 5, 3, 4), f32, (2, 12, 16), i64, False, 0.1) == "fused"
    assert route(True, (2, 5, 3, 4), f32, (2, 3, 4), i64, True, 0.0) == "fused"              # same size, class weights
    assert route(True, (2, 5, 3, 4), f32, (2, 3, 4), i64, False, 0.0) == "plain"
    assert route(False, (2, 5, 3, 4), f32, (2, 3, 4), i64, False, 0.0) == "plain"
    assert route(False, (2, 5, 3, 4), f32, (2, 12, 16), i64, False, 0.0) == "composed"       # CPU tensors
    assert route(True, (2, 5, 3, 4), f32, (2, 12, 16), i64, True, 0.1) == "composed"         # weights with smoothing
    assert route(True, (2, 5, 12, 16), f32, (2, 3, 4), i64, False, 0.0) == "composed"        # downsampling
    assert route(True, (2, 5, 3, 4), f32, (2, 2, 16), i64, False, 0.0) == "composed"         # one axis shrinks
    assert route(True, (2, 5, 3, 4), torch.float64, (2, 12, 16), i64, False, 0.0) == "composed"
    assert route(True, (2, 5, 3, 4), f32, (2, 12, 16), f32, False, 0.0) == "composed"        # not class indices
    assert route(True, (2, 5, 3, 4), f32, (2, 5, 12, 16), f32, False, 0.0) == "composed"     # probability targets
    assert route(True, (2, 5, 3, 4), f32, (3, 12, 16), i64, False, 0.0) == "composed"
    assert route(True, (2, 5, 3, 4), f32, (2, 1 << 15, 1 << 15), i64, False, 0.0) == "composed"   # N*H*W = 2^31
    assert route(True, (2, 5, 3, 4), f32, (1, 3, (1 << 22) + 1), i64, False, 0.0) == "composed"


class Subclass(L.UpsampledCrossEntropyLoss):
    """The same criterion under another type: SoftSegTreeSupLoss composes it through autograd."""


def test_seg_criterion_route_is_a_host_function():
    route = L.seg_criterion_route
    up = L.UpsampledCrossEntropyLoss(ignore_index=255)
    lo, full, same = (2, 20, 9, 11), (2, 36, 44), (2, 9, 11)
    assert route(up, lo, f32, full, i64) == ("upsampled",)
    assert route(up, lo, torch.float16, full, i64) == ("upsampled",)
    assert route(L.UpsampledCrossEntropyLoss(ignore_index=255, label_smoothing=0.1), lo, f32, full, i64) == ("upsampled",)
    assert route(L.UpsampledCrossEntropyLoss(weight=torch.ones(20)), lo, f32, full, i64) == ("upsampled",)
    assert route(L.UpsampledCrossEntropyLoss(weight=torch.ones(20)), lo, f32, same, i64) == ("upsampled",)
    # targets at the logits' size and no weights: today's single fused call, with the criterion's settings
    assert route(up, lo, f32, same, i64) == ("pixel", 255, 0.0)
    assert route(L.UpsampledCrossEntropyLoss(ignore_index=3, label_smoothing=0.2), lo, f32, same, i64) == ("pixel", 3, 0.2)
    # what the kernels refuse, and any other type, composes
    assert route(Subclass(ignore_index=255), lo, f32, full, i64) == ("composed",)
    assert route(L.UpsampledCrossEntropyLoss(weight=torch.ones(20), label_smoothing=0.1), lo, f32, full, i64) == ("composed",)
    assert route(up, full[:1] + (20,) + full[1:], f32, same, i64) == ("composed",)                      # downsampling
    assert route(up, lo, f32, full, f32) == ("composed",)
    assert route(nn.MSELoss(), lo, f32, same, i64) == ("composed",)
    # nn.CrossEntropyLoss keeps the route it had
    assert route(nn.CrossEntropyLoss(ignore_index=255), lo, f32, same, i64) == ("pixel", 255, 0.0)
    assert route(nn.CrossEntropyLoss(label_smoothing=0.1), lo, f32, same, i64) == ("pixel", -100, 0.1)
    assert route(nn.CrossEntropyLoss(weight=torch.ones(20)), lo, f32, same, i64) == ("composed",)
    assert route(nn.CrossEntropyLoss(ignore_index=255), lo, f32, (2, 20, 9, 11), f32) == ("composed",)
