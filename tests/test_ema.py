"""Host side of the weight EMA (no GPU): the decay ramp, the restatement's own arithmetic, every refusal of nbdt_ema_* through
the loaded library, the driver's flags and its checkpoint plumbing with a stub engine."""
import ctypes
import math

import pytest
import torch

import nbdt_path  # noqa: F401  (tests/conftest.py put the package on sys.path)
from nbdt import _C, ops
from nbdt.engine import _Engine

import _ema_ref as R
import main as driver

EINVAL = -1


# ------------------------------------------------------------------------------------------------ the ramp
def test_decay_ramp_values():
    d = 0.9999
    for at in (_Engine.ema_decay_at, R.decay_at):
        assert at(0, d, True) == 0.1                                   # (1 + 0) / (10 + 0)
        assert at(1, d, True) == 2.0 / 11.0
        assert at(89989, d, True) == 89990.0 / 89999.0 < d             # the last step of the ramp ...
        assert at(89990, d, True) == d                                 # ... (1 + t) / (10 + t) = 0.9999 exactly at t = 89990
        assert at(89991, d, True) == d and at(10 ** 9, d, True) == d   # and beyond
        for t in (0, 1, 89990, 10 ** 9):
            assert at(t, d, False) == d                                # no warm-up: the decay as given
    assert _Engine.ema_decay_at(0) == 0.1 and _Engine.ema_decay_at(10 ** 7) == 0.9999      # the defaults
    # non-decreasing in t
    vals = [_Engine.ema_decay_at(t, d, True) for t in range(0, 100000, 997)]
    assert all(a <= b for a, b in zip(vals, vals[1:]))


def test_one_minus_decay_is_rounded_once_to_fp32():
    for d in (0.9999, 0.1, 2.0 / 11.0, 0.99):
        omd = R.omd32(d)
        assert omd == ctypes.c_float(1.0 - d).value                    # what the binding hands the kernel
        assert abs(omd - (1.0 - d)) <= 2.0 ** -24 * (1.0 - d)
    assert R.omd32(0.9999) != 1.0 - 0.9999                             # (the double is not an fp32 value)


def test_restatement_is_three_roundings():
    p = torch.tensor([1.0, 3.0, 1.0 + 2.0 ** -23, 0.0], dtype=torch.float32)
    e = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float32)
    omd = R.omd32(0.9)                                                 # float32(0.1)
    f = lambda v: torch.tensor(v, dtype=torch.float64).to(torch.float32).item()   # noqa: E731
    want = [f(ev + f(omd * f(pv - ev))) for pv, ev in zip(p.tolist(), e.tolist())]
    p0 = p.clone()
    assert R.update_(e, p, omd).tolist() == want and torch.equal(p, p0)
    # omd = 1 is what the sequence yields, not a copy: e + (p - e) is not p when the subtraction rounds
    p, e = torch.tensor([2.0 ** -30], dtype=torch.float32), torch.tensor([1.0], dtype=torch.float32)
    assert R.update_(e.clone(), p, 1.0).item() == f(1.0 + f(2.0 ** -30 - 1.0)) == 0.0 != p.item()
    assert R.update_(e.clone(), p, 0.0).item() == e.item()
    assert R.mirror(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])).tolist() == [1.0, 1.0 + 2.0 ** -6]   # ties to even


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_without_a_gpu():
    lib = _C.lib()
    assert lib.nbdt_version() >= 118
    a, b = torch.zeros(64), torch.zeros(64)                      # host memory stands in: nothing is launched
    m = torch.zeros(64, dtype=torch.bfloat16)
    table = torch.zeros(3, dtype=torch.int64)
    P, E, M, T = a.data_ptr(), b.data_ptr(), m.data_ptr(), table.data_ptr()
    assert P % 16 == 0 and E % 16 == 0 and M % 8 == 0 and T % 8 == 0
    nan = float("nan")
    v = ctypes.c_void_p

    def refused(rc, what):
        assert rc == EINVAL, what
        assert lib.nbdt_last_error(), what

    for p, e, n, omd, what in [
            (None, E, 64, 0.1, "p NULL"), (P, None, 64, 0.1, "ema NULL"),
            (P, E, 0, 0.1, "n = 0"), (P, E, -4, 0.1, "n < 0"), (P, E, 6, 0.1, "n % 4"),
            (P + 4, E, 32, 0.1, "p misaligned"), (P, E + 8, 32, 0.1, "ema misaligned"),
            (P, P, 64, 0.1, "p == ema"),
            (P, E, 64, -0.125, "omd < 0"), (P, E, 64, 1.5, "omd > 1"), (P, E, 64, nan, "omd NaN")]:
        refused(lib.nbdt_ema_update(v(p), v(e), n, omd, None), "update: " + what)
    for p, e, mb, n, what in [
            (None, E, M, 64, "p NULL"), (P, None, M, 64, "ema NULL"),
            (P, E, M, 0, "n = 0"), (P, E, M, -4, "n < 0"), (P, E, None, 6, "n % 4"),
            (P + 4, E, None, 32, "p misaligned"), (P, E + 8, None, 32, "ema misaligned"),
            (P, E, M + 4, 32, "mirror misaligned"), (P, P, None, 64, "p == ema")]:
        refused(lib.nbdt_ema_swap(v(p), v(e), v(mb), n, None), "swap: " + what)
    for t, rows, omd, what in [(None, 1, 0.1, "table NULL"), (T, 0, 0.1, "no rows"), (T, -1, 0.1, "rows < 0"),
                               (T, 1, -0.125, "omd < 0"), (T, 1, 1.5, "omd > 1"), (T, 1, nan, "omd NaN")]:
        refused(lib.nbdt_ema_update_multi(v(t), rows, omd, None), "update_multi: " + what)
    for t, rows, what in [(None, 1, "table NULL"), (T, 0, "no rows"), (T, -1, "rows < 0")]:
        refused(lib.nbdt_ema_swap_multi(v(t), rows, None), "swap_multi: " + what)
    assert b"empty ema table" in lib.nbdt_last_error()


def test_python_bindings_refuse_host_tensors_and_bad_tables():
    a, b = torch.zeros(64), torch.zeros(64)
    with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
        ops.ema_update(a, b, 0.1)
    with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
        ops.ema_swap(a, b)
    for pairs, what in [([], "empty"), ([(a, torch.zeros(32))], "multiples of 32"), ([(a[:48], b[:48])], "multiples of 32"),
                        ([(a, a)], "own shadow"), ([(a, b.double())], "fp32"), ([(a[1:33], b[:32])], "16-byte")]:
        with pytest.raises(_C.NBDTHipError, match=what):
            ops.EmaTable(pairs, "cpu")
    t = ops.EmaTable([(a, b), (a[:32], b[32:])], "cpu")              # a good table builds without a GPU ...
    assert t.n_rows == 2 and t.table.tolist() == [[a.data_ptr(), b.data_ptr(), 64], [a.data_ptr(), b.data_ptr() + 128, 32]]
    with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):    # ... and launches nothing on the host
        t.update(0.1)
    with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
        t.swap()


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_flags():
    a = driver.build_parser().parse_args([])
    assert (a.ema_decay, a.ema_steps, a.no_ema_warmup, a.use_ema) == (None, 1, False, False)
    b = driver.parse_args("--ema-decay 0.999 --ema-steps 4 --no-ema-warmup".split())
    assert (b.ema_decay, b.ema_steps, b.no_ema_warmup, b.use_ema) == (0.999, 4, True, False)
    c = driver.parse_args("--eval --resume --use-ema".split())
    assert c.use_ema and c.ema_decay is None
    for bad in (["--use-ema"], ["--use-ema", "--resume"], ["--use-ema", "--ema-decay", "0.99"], ["--use-ema", "--eval"],
                ["--ema-decay", "1.0"], ["--ema-decay", "0"], ["--ema-decay", "-0.5"], ["--ema-steps", "0"]):
        with pytest.raises(SystemExit):
            driver.parse_args(bad)


class _StubEngine:
    """What the driver's checkpoint helpers touch of an engine."""

    def __init__(self):
        self.avg = {"w": torch.tensor([1.0, 2.0]), "bn.num_batches_tracked": torch.tensor(3)}
        self.ema_updates = 7
        self.loaded = None

    def ema_state_dict(self):
        return {k: v.clone() for k, v in self.avg.items()}

    def load_ema_state_dict(self, sd):
        self.loaded = dict(sd)


def test_checkpoint_key_plumbing_with_a_stub_engine():
    eng = _StubEngine()
    fields = driver.ema_checkpoint_fields(eng, 91.5)
    assert sorted(fields) == ["acc_ema", "ema_updates", "net_ema"]
    assert fields["acc_ema"] == 91.5 and fields["ema_updates"] == 7
    assert sorted(fields["net_ema"]) == sorted(eng.avg) and torch.equal(fields["net_ema"]["w"], eng.avg["w"])
    assert all(not v.is_cuda for v in fields["net_ema"].values())
    ckpt = {"net": {"w": torch.tensor([5.0, 6.0]), "bn.num_batches_tracked": torch.tensor(9)}, "acc": 90.0, "epoch": 4}
    ckpt.update(fields)
    # --resume: the average and the count come back ...
    fresh = _StubEngine()
    fresh.ema_updates = 0
    assert driver.restore_ema(fresh, ckpt, ckpt["net"]) is True
    assert fresh.ema_updates == 7 and torch.equal(fresh.loaded["w"], eng.avg["w"])
    # ... with the `module.` prefix coerced like the weights'
    pre = dict(ckpt, net_ema={"module." + k: v for k, v in ckpt["net_ema"].items()})
    assert driver.restore_ema(fresh, pre, ckpt["net"]) and sorted(fresh.loaded) == sorted(eng.avg)
    # ... and a checkpoint without them leaves the engine alone (the average starts from the loaded weights)
    plain = _StubEngine()
    assert driver.restore_ema(plain, {"net": ckpt["net"], "acc": 1.0, "epoch": 0}, ckpt["net"]) is False
    assert plain.loaded is None and plain.ema_updates == 7
    # --use-ema picks net_ema as the weights to evaluate, and says so clearly when there are none
    assert driver.eval_state_of(ckpt, False) is ckpt
    picked = driver.eval_state_of(ckpt, True, "x.pth")
    assert list(picked) == ["net"] and picked["net"] is ckpt["net_ema"]
    with pytest.raises(SystemExit, match="x.pth holds no averaged weights"):
        driver.eval_state_of({"net": ckpt["net"]}, True, "x.pth")
    assert math.isclose(fields["acc_ema"], 91.5)
