"""Host side of the LARS path (no GPU): the float64 reference's self-check, ParamStore.segments, the per-step learning-rate
schedule ``lr_at`` of the driver, the refusals of nbdt_lars_create and the driver's new flags."""
import math

import numpy as np
import pytest
import torch

import nbdt_path  # noqa: F401  (tests/conftest.py put the package on sys.path)
from nbdt import _C, ops
from nbdt.engine import LarsConfig, ParamStore

import _lars_ref as R
import main as driver


def check_segment_table(store, weight_decay):
    """What every ParamStore.segments table must satisfy (also applied to a real engine's store by the GPU tests)."""
    rows = store.segments(weight_decay)
    names = store.segment_names()
    assert len(rows) == len(store.entries) == len(names) and sorted(names) == sorted(store.entries)
    end = 0
    for name, (off, length, wd, adapt) in zip(names, rows):
        e_off, shape = store.entries[name]
        assert off == e_off and length == math.prod(shape) and length > 0, name       # the entry itself, gaps excluded
        assert off % 4 == 0 and off >= end, name                                       # sorted, disjoint, 16-byte aligned
        end = off + length
        if len(shape) <= 1:
            assert (wd, adapt) == (0.0, 0), name
        else:
            assert (wd, adapt) == (weight_decay, 1), name
    assert end <= store.n
    flipped = store.segments(weight_decay, exclude_1d=False)
    assert [(o, l) for o, l, _, _ in flipped] == [(o, l) for o, l, _, _ in rows]
    assert all((wd, adapt) == (weight_decay, 1) for _, _, wd, adapt in flipped)
    return rows


def test_reference_with_no_adaptation_is_torch_sgd_with_weight_decay():
    gen = torch.Generator().manual_seed(3)
    n, wd, lr, mom = 257, 5e-4, 0.1, 0.9
    p0, b0 = torch.randn(n, generator=gen, dtype=torch.float64), torch.randn(n, generator=gen, dtype=torch.float64)
    ref = R.LarsRef(p0, b0, [(0, 100, wd, 0), (100, 157, wd, 0)], mom)
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([q], lr=lr, momentum=mom, weight_decay=wd)
    opt.state[q]["momentum_buffer"] = b0.clone()
    for _ in range(4):
        g = torch.randn(n, generator=gen, dtype=torch.float64)
        assert ref.step(g, lr, trust=1e-3, eps=1e-8) == [1.0, 1.0]
        q.grad = g.clone()
        opt.step()
        assert (ref.param - q.detach()).abs().max().item() <= 1e-12
        assert (ref.buf - opt.state[q]["momentum_buffer"]).abs().max().item() <= 1e-12


def test_reference_ratio_is_the_published_formula():
    p, g = np.full(16, 2.0), np.full(16, 1.0)
    assert R.trust_ratio(p, g, 0.5, 1, 0.25, 0.0, 1.0) == 0.25          # wn 8, gn 4: 0.25 * 8 / (4 + 4)
    assert R.trust_ratio(p, 0 * g, 0.5, 1, 0.25, 0.0, 1.0) == 1.0       # degenerate norms: no adaptation
    assert R.trust_ratio(0 * p, g, 0.5, 1, 0.25, 0.0, 1.0) == 1.0
    assert R.trust_ratio(p, g, 0.5, 0, 0.25, 0.0, 1.0) == 1.0
    assert R.trust_ratio(p, g, 0.0, 1, 1.0, 0.0, 0.5) == 4.0            # grad_scale enters the gradient norm


def test_param_store_segments_on_a_hand_made_store():
    s = ParamStore("cpu")
    s.add("conv.weight", (32, 9, 32), lambda v: v.normal_())
    s.add("bn.weight", (32,), lambda v: v.fill_(1.0))
    s.add("bn.bias", (32,), lambda v: v.zero_())
    s.add("fc.weight", (10, 13), lambda v: v.normal_())       # 130 elements: a 6-element alignment gap follows
    s.add("fc.bias", (10,), lambda v: v.zero_())              # ... and the tail after this one
    rows = check_segment_table(s, 5e-4)
    assert rows == [(0, 9216, 5e-4, 1), (9216, 32, 0.0, 0), (9248, 32, 0.0, 0), (9280, 130, 5e-4, 1), (9416, 10, 0.0, 0)]
    assert s.segment_names() == ["conv.weight", "bn.weight", "bn.bias", "fc.weight", "fc.bias"]
    assert s.n == 9432


def test_lars_config_defaults():
    assert LarsConfig() == (1e-3, 1e-8, True) and LarsConfig(0.02).exclude_1d is True


def test_create_refuses_bad_tables_without_a_gpu():
    assert _C.lib().nbdt_version() >= 117
    good = [(0, 10, 0.0, 1), (12, 5, 0.0, 1)]
    for rows, n, what in [
            ([], 64, "empty"),
            ([(12, 5, 0.0, 1), (0, 10, 0.0, 1)], 64, "sorted"),
            ([(0, 10, 0.0, 1), (8, 5, 0.0, 1)], 64, "overlap"),
            ([(0, 10, 0.0, 1), (14, 5, 0.0, 1)], 64, "multiples of 4"),
            ([(0, 10, 0.0, 1), (60, 5, 0.0, 1)], 64, "out of range"),
            ([(0, 10, 0.0, 1), (64, 1, 0.0, 1)], 64, "out of range"),
            ([(0, 0, 0.0, 1)], 64, "positive"),
            (good, 0, "empty arena")]:
        with pytest.raises(_C.NBDTHipError, match=what):
            ops.LarsPlan(n, rows)
    # null pointers are refused before anything is read
    assert _C.lib().nbdt_lars_create(64, None, None, None, None, 1, None) == -1
    assert _C.lib().nbdt_lars_step(None, None, None, None, 0.1, 0.9, 1e-3, 0.0, 1.0, None, 0, None) == -1
    assert b"null plan" in _C.lib().nbdt_last_error()
    assert _C.lib().nbdt_lars_destroy(None) == 0 and not _C.lib().nbdt_lars_ratios(None)


def test_lr_at_multistep_without_warmup_is_multistep_lr():
    epochs, spe = 200, 7
    for epoch in range(epochs):
        want = driver.multistep_lr(0.1, epoch, epochs)
        for step in (epoch * spe, epoch * spe + spe - 1):
            assert driver.lr_at(0.1, step, spe, epochs, "multistep", 0.0) == want        # the same float


@pytest.mark.parametrize("schedule", ["cosine", "poly", "multistep"])
def test_lr_at_warmup_and_decay(schedule):
    base, spe, epochs, W = 0.4, 10, 6, 1.5
    t_w, T = 15, 60
    lr = [driver.lr_at(base, s, spe, epochs, schedule, W) for s in range(T + 1)]
    assert lr[0] == base / t_w and lr[t_w - 1] == base                       # warm-up: base / T_w ... base
    assert all(a < b for a, b in zip(lr[:t_w - 1], lr[1:t_w]))
    assert lr[t_w] == base                                                   # the decay starts at base on step T_w
    assert all(a >= b for a, b in zip(lr[t_w:-1], lr[t_w + 1:]))             # non-increasing afterwards
    if schedule == "multistep":
        assert lr[T - 1] == driver.multistep_lr(base, epochs - 1, epochs)
        return
    assert lr[T] == pytest.approx(0.0, abs=1e-17) and lr[T - 1] > 0.0        # 0 on step T; the last used step is T - 1
    t = (T - 1 - t_w) / (T - t_w)
    want = 0.5 * base * (1 + math.cos(math.pi * t)) if schedule == "cosine" else base * (1 - t) ** 2
    assert lr[T - 1] == pytest.approx(want, rel=1e-12)
    # no warm-up: the first step already decays from base
    assert driver.lr_at(base, 0, spe, epochs, schedule, 0.0) == base


def test_driver_defaults_select_sgd_and_multistep():
    a = driver.build_parser().parse_args([])
    assert (a.optimizer, a.lr_schedule, a.warmup_epochs) == ("sgd", "multistep", 0.0)
    assert (a.lars_trust, a.lars_eps, a.lars_adapt_1d) == (1e-3, 1e-8, False)
    b = driver.parse_args("--optimizer lars --lr-schedule poly --warmup-epochs 2.5 --lars-trust 0.02 --lars-adapt-1d".split())
    assert (b.optimizer, b.lr_schedule, b.warmup_epochs, b.lars_trust, b.lars_adapt_1d) == ("lars", "poly", 2.5, 0.02, True)
    with pytest.raises(SystemExit):
        driver.parse_args(["--warmup-epochs", "-1"])
    with pytest.raises(SystemExit):
        driver.parse_args(["--optimizer", "lamb"])
