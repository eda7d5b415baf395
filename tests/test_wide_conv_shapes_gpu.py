"""The dense 3x3 entries at the widths the wide ResNets add (wide_resnet50_2 / 101_2: conv2 at 128 .. 1024 channels): the
integer-exact method and the helpers of tests/_resnet_conv_cases.py at 1024 -> 1024 on 8 x 8 and 7 x 7 grids, stride 2
from 16 -> 8 at 1024, and 512 -> 512 at 14 x 14 -- forward, data gradient (plain and accumulating) and weight gradient equal
the int64 convolution bit for bit on whichever kernel the launch rules pick (a plan that refuses a shape falls back to the
first-generation kernel inside the entry).  No kernel is new here: the table of tests/_resnet_conv_cases.py stops at 512."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resnet_conv_cases as C  # noqa: E402
import test_conv_resnet_shapes_gpu as S  # noqa: E402

from nbdt import ops  # noqa: E402

DEV = S.DEV
# B, H, W (input), cin, cout, k, stride: a few hundred output pixels each (more than one 256-pixel tile where the grid allows)
WIDE_CASES = [(5, 8, 8, 1024, 1024, 3, 1), (3, 7, 7, 1024, 1024, 3, 1), (5, 16, 16, 1024, 1024, 3, 2),
              (2, 14, 14, 512, 512, 3, 1)]
cases = pytest.mark.parametrize("case", WIDE_CASES, ids=[C.case_id(c) for c in WIDE_CASES])

_DEVC = {}


def _dev(case):
    if case not in _DEVC:
        c = C.integer_case(case)
        _DEVC[case] = dict(c, xp=S._padded_from(c["x"]), gp=S._padded_from(c["gy"]), wts=S._Weights(case, c["w"]))
    return _DEVC[case]


@cases
def test_wide_forward_is_exact(case):
    B, H, W, cin, cout, k, stride = case
    c = _dev(case)
    out = S._sentinel_out(B, H // stride, W // stride, cout)
    ops.conv_igemm(c["wts"].descs()[0], c["xp"], c["wts"].wb, out)
    print(C.case_id(case), "forward on", ops.last_igemm_kernel())
    assert S._equal_int(ops.interior(out), c["fwd"]) and S._halo_untouched(out)


@cases
def test_wide_data_gradient_is_exact(case):
    B, H, W, cin, cout, k, stride = case
    c = _dev(case)
    wts = c["wts"]
    _, plain, acc, _ = wts.descs()
    for descs, base in ((plain, None), (acc, c["base"])):
        ref = c["dgrad"] if base is None else c["dgrad"] + base
        gx = ops.padded(B, H, W, cin, DEV) if base is None else S._padded_from(base)
        if len(descs) > 1:
            ops.conv_igemm_multi(descs, c["gp"], wts.wd, gx)
        else:
            ops.conv_igemm(descs[0], c["gp"], wts.wd, gx)
        print(C.case_id(case), "data gradient on", ops.last_igemm_kernel())
        assert S._equal_int(ops.interior(gx), ref), base is not None
        S._check_border_zero(gx)


@cases
def test_wide_weight_gradient_is_exact(case):
    B, H, W, cin, cout, k, stride = case
    c = _dev(case)
    dw = torch.zeros(cout, k * k, cin, dtype=torch.float32, device=DEV)
    wg = c["wts"].descs()[3]
    ops.conv_wgrad(wg, c["xp"], c["gp"], dw)
    print(C.case_id(case), "weight gradient on", ops.last_wgrad_kernel())
    assert S._equal_int(dw, c["dw"])
    ops.conv_wgrad(wg, c["xp"], c["gp"], dw)
    assert S._equal_int(dw, 2 * c["dw"])
