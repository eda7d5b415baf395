"""Stochastic depth, host side (no GPU): the probability / scale tables, the numpy restatement of the draw
(nbdt.ops.draw_stochastic_depth -- tests/test_stochastic_depth_gpu.py holds the kernel to it bit for bit) and main.py's
--stochastic-depth flag."""
import importlib.util
import math
import os

import numpy as np
import pytest

import nbdt_path
from nbdt import ops
from nbdt.engine_effnet import B0_STAGES

spec = importlib.util.spec_from_file_location("nbdt_main", os.path.join(nbdt_path.PKG_DIR, "main.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

RESIDUAL = (2, 4, 6, 7, 9, 10, 12, 13, 14)        # s2u2, s3u2, s4u2, s4u3, s4u5, s4u6, s5u2, s5u3, s5u4


def _b0_flags():
    """cin == cout and stride == 1, from the stage table the engine is built from."""
    flags, cin = [], 32
    for stage_stride, specs in B0_STAGES:
        for j, (cout, _, _) in enumerate(specs):
            flags.append(cin == cout and (stage_stride if j == 0 else 1) == 1)
            cin = cout
    return flags


def test_probability_tables_follow_the_linear_rule():
    flags = _b0_flags()
    assert len(flags) == 16 and tuple(i for i, f in enumerate(flags) if f) == RESIDUAL
    prob, scale = ops.stochastic_depth_probs(0.2, 16, flags)
    assert prob.dtype == np.float32 and scale.dtype == np.float32 and prob.shape == scale.shape == (16,)
    for i in range(16):
        if i in RESIDUAL:
            assert prob[i] == np.float32(0.2 * i / 16)
        else:
            assert prob[i] == 0 and scale[i] == 1
    assert (scale == (1.0 / (1.0 - prob.astype(np.float64))).astype(np.float32)).all()
    assert prob[14] == np.float32(0.175)
    p0, s0 = ops.stochastic_depth_probs(0.0, 16, flags)
    assert (p0 == 0).all() and (s0 == 1).all()
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.stochastic_depth_probs(bad, 16, flags)
    with pytest.raises(ValueError):
        ops.stochastic_depth_probs(0.2, 16, flags[:15])


def test_draw_is_a_pure_function_with_the_right_statistics():
    prob, scale = ops.stochastic_depth_probs(0.2, 16, _b0_flags())
    B = 4096
    t = ops.draw_stochastic_depth(3, 0, 0, prob, scale, B)
    assert t.dtype == np.float32 and t.shape == (16, B)
    assert (t == ops.draw_stochastic_depth(3, 0, 0, prob, scale, B)).all()
    # a function of (unit, image), not of the batch size: a smaller batch is a prefix
    assert (ops.draw_stochastic_depth(3, 0, 0, prob, scale, 7) == t[:, :7]).all()
    for other in ((4, 0, 0), (3, 1, 0), (3, 0, 1), (3, 0, 2 ** 31), (3, 0, 2 ** 40)):
        assert (ops.draw_stochastic_depth(*other, prob, scale, B) != t).any(), other
    for i in range(16):
        if i in RESIDUAL:
            assert np.isin(t[i], (np.float32(0), scale[i])).all()
        else:
            assert (t[i] == 1).all()
    # kept fraction of the unit with p = 0.175 over 64 counters: within 4 binomial standard deviations of 0.825
    kept = sum(int((ops.draw_stochastic_depth(3, 0, c, prob, scale, B)[14] != 0).sum()) for c in range(64))
    n, p = 64 * B, 1.0 - float(prob[14])
    assert abs(kept / n - p) <= 4.0 * math.sqrt(p * (1.0 - p) / n), (kept / n, p)
    # images of one unit and units of one image are not copies of each other
    assert len({t[i].tobytes() for i in RESIDUAL}) == len(RESIDUAL)


def test_main_accepts_the_flag_for_efficientnet_only(capsys):
    a = M.parse_args("--arch efficientnet_b0 --dataset CIFAR10 --stochastic-depth 0.2".split())
    assert a.stochastic_depth == 0.2
    assert M.parse_args("--arch efficientnet_b0 --dataset CIFAR10".split()).stochastic_depth == 0
    assert M.parse_args("--arch ResNet18 --dataset CIFAR10".split()).stochastic_depth == 0
    assert M.parse_args("--arch ResNet18 --stochastic-depth 0".split()).stochastic_depth == 0
    with pytest.raises(SystemExit):
        M.parse_args("--arch ResNet18 --dataset CIFAR10 --stochastic-depth 0.2".split())
    assert "--stochastic-depth" in capsys.readouterr().err
    for bad in ("1.0", "-0.1"):
        with pytest.raises(SystemExit):
            M.parse_args(["--arch", "efficientnet_b0", "--stochastic-depth", bad])
        assert "--stochastic-depth" in capsys.readouterr().err
