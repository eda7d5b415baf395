"""Host side of gradient clipping and accumulation (no GPU): the numpy restatement of include/nbdt_hip.h
(tests/_clip_ref.py) against torch.nn.utils.clip_grad_norm_ in float64, the C-ABI table, every refusal that needs no
device, the driver's flags, ClipConfig and train_step's argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import nbdt_path
from nbdt import _C, ops
from nbdt import engine as E
from nbdt.engine import ClipConfig, train_step

import _clip_ref as C
import main as driver

EINVAL = -1
SHAPES = [(3, 5, 7), (64,), (17, 3), (1,), (2, 2, 2, 2), (129,), (10, 13)]      # 7 ragged tensors, 496 elements


def ragged_grads(seed, scale=1.0):
    """The 7 tensors as fp32, every magnitude in [2^-6, 4] * scale: nothing denormal, nothing that cancels in a norm."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in SHAPES:
        mag = torch.empty(s).uniform_(2.0 ** -6, 4.0, generator=g)
        sign = torch.randint(0, 2, s, generator=g).float() * 2 - 1
        out.append((mag * sign * scale).float())
    flat = torch.cat([t.reshape(-1) for t in out])
    assert flat.numel() == 496 and 2.0 ** -6 * scale <= float(flat.abs().min()) and float(flat.abs().max()) <= 4.0 * scale
    return out, flat.numpy().copy()


def torch_clip64(tensors, max_norm):
    params = [torch.nn.Parameter(torch.zeros_like(t, dtype=torch.float64)) for t in tensors]
    for p, t in zip(params, tensors):
        p.grad = t.double().clone()
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    return float(total), torch.cat([p.grad.reshape(-1) for p in params]).numpy()


# ------------------------------------------------------------------------------------------------ restatement vs torch
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_matches_clip_grad_norm_in_float64(seed):
    """With grad_scale = 1 both compute min(1, max_norm / (norm + 1e-6)) g; the restatement in fp32, torch in fp64, so they
    differ by the restatement's roundings, u = 2^-24 each.  norm: the cast of S, the root, the multiply by |1| -- three
    (the fp64 sum's own error, 496 x 2^-53, is far below) -- so 2^-22 relative.  Clipped gradient: those three, the add
    of 1e-6f (with the constant's own rounding, which acts on 1e-6 of a norm above 1), the division and the element's
    multiply: at most six, so 2^-21 relative, per element (no element is near zero: asserted by the fixture)."""
    tensors, flat = ragged_grads(seed)
    want_norm, want_g = torch_clip64(tensors, 1.5)
    assert want_norm > 10.0                                              # so it does clip, by a factor well below 1
    got_g, rec = C.clip(flat, 1.0, 1.5)
    assert rec["clipped"] == 1 and rec["steps"] == 1 and rec["total_clipped"] == 1 and rec["nonfinite"] == 0
    err_n = abs(float(rec["norm"]) - want_norm) / want_norm
    err_g = np.max(np.abs(got_g.astype(np.float64) - want_g) / np.abs(want_g))
    print(f"seed {seed}: norm {float(rec['norm']):.6f}, relative error {err_n:.3e} (bound {2.0 ** -22:.3e}); "
          f"gradient {err_g:.3e} (bound {2.0 ** -21:.3e})")
    assert err_n <= 2.0 ** -22
    assert err_g <= 2.0 ** -21
    assert got_g.dtype == np.float32 and rec["coef"] < 1.0


def test_grad_scale_enters_the_norm_only():
    """norm = |grad_scale| * r: the sign does not matter, and g is scaled by coef alone (the optimizer applies grad_scale)."""
    _, flat = ragged_grads(3)
    a, ra = C.clip(flat, 0.25, 1.5)
    b, rb = C.clip(flat, -0.25, 1.5)
    assert ra == rb and np.array_equal(C.bits(a), C.bits(b))
    assert ra["norm"] == np.float32(0.25) * C.norm_of(flat, 1.0)          # a power of two: exact
    assert np.array_equal(C.bits(a), C.bits(flat * ra["coef"]))


def test_an_unclipped_step_leaves_the_bits():
    tensors, flat = ragged_grads(4, scale=2.0 ** -10)
    want_norm, want_g = torch_clip64(tensors, 1.5)
    assert want_norm < 1.0
    got, rec = C.clip(flat, 1.0, 1.5)
    assert np.array_equal(C.bits(got), C.bits(flat)) and np.array_equal(want_g, flat.astype(np.float64))
    assert rec["coef"] == 1.0 and rec["clipped"] == 0 and rec["steps"] == 1 and rec["total_clipped"] == 0
    # exactly at the bound the quotient is below 1 by the 1e-6: that step IS clipped, as torch's is
    three_four = np.array([3.0, 4.0, 0.0, 0.0], dtype=np.float32)
    _, rec = C.clip(three_four, 1.0, 5.0)
    assert rec["norm"] == 5.0 and rec["clipped"] == 1 and rec["coef"] == np.float32(5.0) / (np.float32(5.0) + C.EPS)


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_a_non_finite_gradient_is_counted_and_left_alone(bad):
    _, flat = ragged_grads(5)
    flat[200] = bad
    rec = C.new_record()
    C.clip(np.ones(4, dtype=np.float32), 1.0, 1.0, rec)                  # a clipped step first: the counters go on
    got, rec = C.clip(flat, 1.0, 1.5, rec)
    assert np.array_equal(C.bits(got), C.bits(flat))
    assert not np.isfinite(rec["norm"]) and rec["coef"] == 1.0
    assert (rec["clipped"], rec["steps"], rec["nonfinite"], rec["total_clipped"]) == (0, 2, 1, 1)
    # a sum that overflows fp32 although every element is finite is non-finite too
    big = np.full(8, 3.0e38, dtype=np.float32)
    got, rec = C.clip(big, 1.0, 1.0)
    assert np.isinf(rec["norm"]) and rec["nonfinite"] == 1 and np.array_equal(got, big)


# ------------------------------------------------------------------------------------------------ C-ABI
ENTRIES = (("nbdt_clip_create", 2), ("nbdt_clip_destroy", 1), ("nbdt_clip_norm", 5), ("nbdt_clip_apply", 3),
           ("nbdt_clip_record", 1), ("nbdt_clip_record_to_host", 3))


def test_header_ctypes_table_and_version_agree():
    lib = _C.lib()
    assert lib.nbdt_version() >= 121
    text = open(os.path.join(nbdt_path.ROOT, "include", "nbdt_hip.h")).read()
    assert "gradient clipping (nbdt_version() >= 121)" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    exported = set(_C.exported_symbols())
    for name, n_args in ENTRIES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert m and len(m.group(1).split(",")) == n_args == len(_C.SIGNATURES[name][1]), name
        assert name in exported, name
    assert ctypes.sizeof(ops.ClipRecord) == 32
    assert [f[0] for f in ops.ClipRecord._fields_] == ["norm", "coef", "clipped", "steps", "nonfinite", "total_clipped",
                                                       "reserved"]
    from nbdt import _build
    assert _build.FLAGS["clip.hip"] == _build.FLAGS["lars.hip"] == _build.FLAGS["adaptive.hip"]
    assert "clip.hip" in _build.sources()


def test_entries_refuse_bad_arguments_without_a_gpu():
    """The scalars are checked first, then g, then the plan: with host memory standing in and no plan nothing is launched,
    and every refusal names its reason."""
    lib = _C.lib()
    nan, inf = float("nan"), float("inf")
    buf = torch.zeros(64)
    assert buf.data_ptr() % 16 == 0
    G = ctypes.c_void_p(buf.data_ptr())
    off = ctypes.c_void_p(buf.data_ptr() + 4)

    def norm(g=G, gs=1.0, m=1.0, plan=None):
        return lib.nbdt_clip_norm(plan, g, gs, m, None)

    for kwargs, what in [(dict(m=0.0), b"max_norm"), (dict(m=-1.0), b"max_norm"), (dict(m=nan), b"max_norm"),
                         (dict(m=inf), b"max_norm"), (dict(gs=nan), b"grad_scale"), (dict(gs=inf), b"grad_scale"),
                         (dict(gs=-inf), b"grad_scale"), (dict(g=None), b"null gradient"), (dict(g=off), b"16-byte aligned"),
                         (dict(), b"null plan")]:
        assert norm(**kwargs) == EINVAL and what in lib.nbdt_last_error(), (kwargs, lib.nbdt_last_error())
    for g, what in [(None, b"null gradient"), (off, b"16-byte aligned"), (G, b"null plan")]:
        assert lib.nbdt_clip_apply(None, g, None) == EINVAL and what in lib.nbdt_last_error(), lib.nbdt_last_error()
    assert lib.nbdt_clip_create(64, None) == EINVAL and b"null plan pointer" in lib.nbdt_last_error()
    handle = ctypes.c_void_p()
    for n in (0, -4):
        assert lib.nbdt_clip_create(n, ctypes.byref(handle)) == EINVAL and not handle.value
        assert b"empty arena" in lib.nbdt_last_error()
    out = (ctypes.c_char * 32)()
    assert lib.nbdt_clip_record_to_host(None, out, None) == EINVAL and lib.nbdt_clip_record_to_host(None, None, None) == EINVAL
    assert lib.nbdt_clip_destroy(None) == 0 and lib.nbdt_clip_record(None) is None
    with pytest.raises(_C.NBDTHipError, match="empty arena"):
        ops.ClipPlan(0)
    # the Python layer refuses host tensors, other lengths and other types before it reaches the library
    plan = object.__new__(ops.ClipPlan)
    plan.n, plan.handle, plan.device = 64, None, None
    with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
        plan.norm(buf, 1.0, 1.0)
    with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
        plan.apply(buf)


# ------------------------------------------------------------------------------------------------ flags
def test_driver_flags_defaults_and_refusals():
    a = driver.parse_args([])
    assert (a.accum_steps, a.clip_grad_norm) == (1, None)
    b = driver.parse_args("--accum-steps 16 --clip-grad-norm 2.5 --batch-size 4096".split())
    assert (b.accum_steps, b.clip_grad_norm, b.batch_size) == (16, 2.5, 4096)
    for bad in ("--clip-grad-norm 0", "--clip-grad-norm -1", "--clip-grad-norm nan", "--clip-grad-norm inf",
                "--accum-steps 0", "--accum-steps -2", "--accum-steps 1.5"):
        with pytest.raises(SystemExit):
            driver.parse_args(bad.split())


# ------------------------------------------------------------------------------------------------ train_step's arguments
def test_clip_config():
    c = ClipConfig(2.0)
    assert c == (2.0,) and c.max_norm == 2.0 and ClipConfig(max_norm=0.5).max_norm == 0.5 and c._fields == ("max_norm",)
    with pytest.raises(TypeError):
        ClipConfig()                                                    # no default: clipping is asked for with a bound
    assert E.ClipConfig is ClipConfig


class _StubEngine:
    """Counts what train_step calls: every refusal below must come before the first of them."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def record(*a, **k):
            self.calls.append(name)
            raise AssertionError(f"train_step reached engine.{name}")
        return record


def test_train_step_refuses_before_any_launch():
    img, y = torch.zeros(10, 3, 8, 8), torch.zeros(10, dtype=torch.long)
    for kwargs, exc, what in [(dict(micro_batches=4), ValueError, "does not split"),
                              (dict(micro_batches=3), ValueError, "does not split"),
                              (dict(micro_batches=0), ValueError, "micro_batches"),
                              (dict(micro_batches=-2), ValueError, "micro_batches"),
                              (dict(micro_batches=2.5), ValueError, "micro_batches"),
                              (dict(clip=1.0), TypeError, "ClipConfig"),
                              (dict(clip=(1.0,)), TypeError, "ClipConfig")]:
        eng = _StubEngine()
        with pytest.raises(exc, match=what):
            train_step(eng, None, img, y, 0.1, **kwargs)
        assert eng.calls == [], kwargs
    eng = _StubEngine()
    with pytest.raises(AssertionError, match="zero_grad"):              # a good split goes on to the engine
        train_step(eng, None, img, y, 0.1, micro_batches=5, clip=ClipConfig(1.0))
    assert eng.calls == ["zero_grad"]


def test_clip_grad_norm_refuses_a_bad_bound_on_the_host():
    eng = object.__new__(E._Engine)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_norm"):
            eng.clip_grad_norm(bad)
    eng._clip_plan = None
    with pytest.raises(RuntimeError, match="no clip_grad_norm yet"):
        eng.clip_stats()
