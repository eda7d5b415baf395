"""Host side of the AdamW / RMSprop path (no GPU): the fp32 restatement of include/nbdt_hip.h against the fp64 oracle
(tests/_adaptive_ref.py), the driver's ``exp`` schedule and new flags, the C-ABI table, and every refusal that needs no
device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import nbdt_path
from nbdt import _C, ops
from nbdt.engine import AdamWConfig, ParamStore, RMSpropConfig

import _adaptive_ref as A
import _lars_ref as R
import main as driver

EINVAL = -1
U = 2.0 ** -24                         # unit roundoff of fp32

# the hyper-parameters of the ragged case, here and on the GPU (tests/test_adaptive_gpu.py): grad_scale 0.5 and eps large
# enough that its place in the formula (inside or outside the root, before or after the bias correction) shows
HP = {
    "adamw": dict(lr=0.01, betas=(0.9, 0.999), eps=1e-4),
    "rmsprop": dict(lr=0.01, alpha=0.99, eps=1e-3, momentum=0.9),
    "rmsprop_mu0": dict(lr=0.01, alpha=0.99, eps=1e-3, momentum=0.0),
    "rmsprop_tf": dict(lr=0.01, alpha=0.9, eps=1e-3, momentum=0.9),
}
GS = 0.5


def kind_of(name):
    return "rmsprop" if name == "rmsprop_mu0" else name


def ragged(name, item=ops.ARENA_OPT_ITEM):
    """(n, rows (offset, length, decay), p0, s1_0, s2_0, grads) of tests/_lars_ref.ragged_case for optimizer `name`."""
    n, segments, p0, b0, grads = R.ragged_case(item)
    rows = [(o, l, wd) for o, l, wd, _ in segments]
    s1, s2 = A.start_state(kind_of(name), n, rows, b0)
    return n, rows, p0, s1, s2, grads


def run_fp32(name, n, rows, p0, s1, s2, grads):
    hp = HP[name]
    ref = A.Fp32Ref(p0, s1, s2, rows)
    for t, g in enumerate(grads, 1):
        if name == "adamw":
            ref.adamw(g, hp["lr"], hp["betas"], hp["eps"], t, GS)
        else:
            ref.rmsprop(g, hp["lr"], hp["alpha"], hp["eps"], hp["momentum"], name == "rmsprop_tf", GS)
    return ref


# ------------------------------------------------------------------------------------------------ restatement vs oracle
@pytest.mark.parametrize("name", list(HP))
def test_fp32_restatement_matches_the_fp64_oracle(name):
    """Three steps on the ragged table.  Both references get the same fp32 arguments, so they differ by rounding alone,
    u = 2^-24 per fp32 operation.  With the bounds asserted below -- |p| <= P = 4, |grad_scale g| <= 3 so that
    |gs| <= G = 3 + wd_max P, every oracle step <= STEP = 0.5, the states within M and S, the root a >= A_MIN -- and T = 3
    steps, each error is (roundings on the path) x u x (the magnitude they act on), summed over the steps:

      mean square (v, sq): sums of non-negative terms, no cancellation: (3 roundings + twice the relative error of gs,
        itself 3 u G / |gs| at worst, i.e. 6 u G |gs| <= 6 u G^2 absolute) per step: T u (4 S + 8 G^2).
      AdamW m: two products and a sum of terms below max(M, G): T u 4 max(M, G).
      AdamW p: p k (two roundings on |p| <= P) and the difference (one more), plus the update ss (m / d): its factors have
        relative errors of a few u each (m through its own recurrence -- m and sqrt(v) shrink together with the gradients,
        so the quotient stays conditioned --, d through half of v's, ss and c2 one each), 16 roundings in all on a
        quantity bounded by the step: T u (4 P + 32 STEP), the 32 a factor 2 over the count for second-order terms.
      RMSprop quotient q = gs / a: gs = grad_scale g + wd p CAN cancel, so its error is absolute, 3 u G, and divides by
        a >= A_MIN; a's relative error is half of sq's plus two roundings, acting on |q| <= G / A_MIN: 20 u G / A_MIN.
      RMSprop buf: q's error (times lr in TensorFlow's form) and two roundings on |buf| <= M per step:
        T u (20 G / A_MIN [x lr] + 2 M);  p: T u 2 P plus lr (torch) or 1 (TensorFlow) times the buffer's error per step.
    Nothing here was fitted to what the restatement gives."""
    n, rows, p0, s1, s2, grads = ragged(name)
    hp, kind = HP[name], kind_of(name)
    T, P, STEP, M, S = len(grads), 4.0, 0.5, 16.0, 2.0
    G = 3.0 + max(wd for _, _, wd in rows) * P
    A_MIN = {"adamw": None, "rmsprop": 0.45, "rmsprop_tf": 0.8}[kind]
    inside = torch.zeros(n, dtype=torch.bool)
    for o, l, _ in rows:
        inside[o:o + l] = True
    okw = {k: v for k, v in hp.items() if k != "lr"}
    oracle = A.Fp64Oracle(kind, p0, s1, s2, rows, **okw)
    assert all(float(GS * g[inside].abs().max()) <= 3.0 for g in grads)
    for g in grads:
        assert oracle.step(g, hp["lr"], GS) <= STEP                       # the oracle's own step stays bounded
        assert oracle.p[inside].abs().max().item() <= P
        assert oracle.s1[inside].abs().max().item() <= M and oracle.s2[inside].abs().max().item() <= S
        if A_MIN is not None:
            assert oracle.s2[inside].min().item() >= A_MIN ** 2
    ref = run_fp32(name, n, rows, p0, s1, s2, grads)
    tol_s2 = T * U * (4 * S + 8 * G * G)
    if kind == "adamw":
        tol_s1, tol_p = T * U * 4 * max(M, G), T * U * (4 * P + 32 * STEP)
    else:
        lr_in = hp["lr"] if kind == "rmsprop_tf" else 1.0
        tol_s1 = T * U * (20 * G / A_MIN * lr_in + 2 * M)
        tol_p = T * U * 2 * P + T * tol_s1 * (1.0 if kind == "rmsprop_tf" else hp["lr"])
    got = {k: torch.from_numpy(v).double() for k, v in (("p", ref.p), ("s1", ref.s1), ("s2", ref.s2))}
    want = {"p": oracle.p, "s1": oracle.s1, "s2": oracle.s2}
    for key, tol in (("p", tol_p), ("s1", tol_s1), ("s2", tol_s2)):
        err = (got[key] - want[key]).abs()
        print(f"{name} {key}: max error {err[inside].max().item():.3e}, bound {tol:.3e}")
        assert err[inside].max().item() <= tol, (name, key)
        assert torch.equal(got[key][~inside], torch.full((int((~inside).sum()),), 7.0, dtype=torch.float64)), key
    assert not torch.equal(got["p"][inside], p0.double()[inside])           # ... and it did move
    if name == "rmsprop_mu0":                                              # no momentum: the buffer is not touched
        assert np.array_equal(ref.s1, s1.numpy())


def test_eps_sits_where_each_formula_puts_it():
    """One element, exact values: torch's RMSprop adds eps to the root, TensorFlow's adds it under the root; AdamW adds it
    after the bias correction."""
    one = lambda x: torch.tensor([x, 0.0, 0.0, 0.0])   # noqa: E731
    rows = [(0, 1, 0.0)]
    r = A.Fp32Ref(one(1.0), one(0.0), one(0.0), rows)
    r.rmsprop(one(2.0), 0.5, 0.75, 1.0, 0.0, tf=False)                 # sq = 0.25 * 4 = 1, a = 1 + 1 = 2, p = 1 - 0.5 * (2 / 2)
    assert (r.p[0], r.s2[0], r.s1[0]) == (0.5, 1.0, 0.0)
    r = A.Fp32Ref(one(1.0), one(0.0), one(1.0), rows)
    r.rmsprop(one(2.0), 0.5, 0.75, 0.75, 0.5, tf=True)                 # sq = 1 + 0.25 * 3 = 1.75, a = sqrt(2.5)
    a = np.sqrt(np.float32(2.5))
    assert r.s2[0] == 1.75 and r.s1[0] == np.float32(0.5) * (np.float32(2.0) / a) and r.p[0] == np.float32(1.0) - r.s1[0]
    r = A.Fp32Ref(one(1.0), one(0.0), one(0.0), rows)
    r.adamw(one(2.0), 0.5, (0.5, 0.75), 1.0, 1)                        # m = 1, v = 1, c2 = 0.5, d = 1 / 0.5 + 1 = 3, ss = 1
    assert (r.s1[0], r.s2[0]) == (1.0, 1.0) and r.p[0] == np.float32(1.0) - np.float32(1.0) / np.float32(3.0)
    assert (r.p[1:] == 0).all()                                         # outside the row: untouched
    c = A.host_scalars(0.5, 0.5, 0.75, 0.75, 2)
    assert (c["omb1"], c["omb2"], c["oma"], c["ss"]) == (0.5, 0.25, 0.25, np.float32(0.5 / 0.75))
    assert c["c2"] == np.float32(np.sqrt(1.0 - 0.5625))


# ------------------------------------------------------------------------------------------------ schedule
def test_lr_at_exp_is_step_lr_stepped_once_per_optimizer_step():
    """StepLR multiplies the running learning rate by gamma at every boundary; lr_at evaluates base * gamma^k.  After k
    decays the two products differ by at most k roundings of a double: 1e-12 relative is far above that for k <= 30."""
    base, spe, epochs, G, E = 0.256, 5, 14, 0.97, 2.4
    every = 12                                                            # round(2.4 * 5)
    q = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([q], lr=base)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=every, gamma=G)
    for step in range(spe * epochs):
        want = opt.param_groups[0]["lr"]
        got = driver.lr_at(base, step, spe, epochs, "exp", 0.0, G, E)
        assert got == pytest.approx(want, rel=1e-12), step
        assert got == base * G ** (step // every)
        opt.step()
        sched.step()
    # after warm-up the staircase starts at base on step T_w
    t_w = 8                                                               # round(1.5 * 5) = 8 (banker's rounding of 7.5)
    lr = [driver.lr_at(base, s, spe, epochs, "exp", 1.5, G, E) for s in range(40)]
    assert lr[0] == base / t_w and lr[t_w - 1] == base and lr[t_w] == base
    assert lr[t_w + every - 1] == base and lr[t_w + every] == base * G and lr[t_w + 2 * every] == base * G ** 2
    # defaults: 0.97 every 2.4 epochs; a period shorter than one step is one step
    assert driver.lr_at(1.0, 24, 10, 9, "exp") == 0.97 and driver.lr_at(1.0, 23, 10, 9, "exp") == 1.0
    assert driver.lr_at(1.0, 3, 1, 9, "exp", 0.0, 0.5, 0.01) == 0.125


def test_the_three_existing_schedules_are_unchanged():
    import math
    base, spe, epochs, W = 0.4, 10, 6, 1.5
    t_w, total = 15, 60
    for step in range(total):
        for sched in ("multistep", "cosine", "poly"):
            got = driver.lr_at(base, step, spe, epochs, sched, W)
            assert got == driver.lr_at(base, step, spe, epochs, sched, W, 0.5, 1.0)       # the new arguments do not enter
            if step < t_w:
                want = base * (step + 1) / t_w
            elif sched == "multistep":
                want = driver.multistep_lr(base, step // spe, epochs)
            else:
                t = (step - t_w) / float(total - t_w)
                want = 0.5 * base * (1.0 + math.cos(math.pi * t)) if sched == "cosine" else base * (1.0 - t) ** 2
            assert got == want, (sched, step)                                             # the same float
    with pytest.raises(ValueError):
        driver.lr_at(base, 20, spe, epochs, "linear", 0.0)


# ------------------------------------------------------------------------------------------------ flags
def test_driver_flags_defaults_and_refusals():
    a = driver.parse_args([])
    assert (a.optimizer, a.lr_schedule) == ("sgd", "multistep")
    assert (a.adam_betas, a.opt_eps, a.rmsprop_alpha, a.rmsprop_tf, a.opt_decay_1d) == ((0.9, 0.999), 1e-8, 0.99, False, False)
    assert (a.lr_decay_rate, a.lr_decay_epochs) == (0.97, 2.4)
    b = driver.parse_args("--optimizer adamw --adam-betas 0.8 0.99 --opt-eps 1e-6 --opt-decay-1d".split())
    assert (b.optimizer, b.adam_betas, b.opt_eps, b.opt_decay_1d) == ("adamw", (0.8, 0.99), 1e-6, True)
    c = driver.parse_args("--optimizer rmsprop --rmsprop-tf --lr-schedule exp --lr-decay-rate 0.9 --lr-decay-epochs 1".split())
    assert (c.rmsprop_tf, c.opt_eps, c.rmsprop_alpha, c.lr_schedule, c.lr_decay_rate, c.lr_decay_epochs) == \
        (True, 1e-3, 0.9, "exp", 0.9, 1.0)
    d = driver.parse_args("--optimizer rmsprop --rmsprop-tf --opt-eps 0.01 --rmsprop-alpha 0.95".split())
    assert (d.opt_eps, d.rmsprop_alpha) == (0.01, 0.95)
    e = driver.parse_args("--optimizer rmsprop".split())
    assert (e.opt_eps, e.rmsprop_alpha) == (1e-8, 0.99)
    for bad in ("--optimizer lamb", "--optimizer adam", "--optimizer sgd --rmsprop-tf", "--optimizer adamw --rmsprop-tf",
                "--adam-betas 0.9 1.0", "--adam-betas -0.1 0.9", "--adam-betas 0.9", "--rmsprop-alpha 1.0",
                "--rmsprop-alpha -0.5", "--opt-eps -1e-8", "--opt-eps nan", "--opt-eps inf", "--lr-decay-rate 0",
                "--lr-decay-rate 1.5", "--lr-decay-rate nan", "--lr-decay-epochs 0", "--lr-decay-epochs -2",
                "--lr-decay-epochs inf", "--lr-schedule step"):
        with pytest.raises(SystemExit):
            driver.parse_args(bad.split())


def test_configs_and_the_second_state_arena():
    assert AdamWConfig() == ((0.9, 0.999), 1e-8, True) and RMSpropConfig() == (0.99, 1e-8, False, True)
    assert RMSpropConfig(0.9, 1e-3, True).exclude_1d is True
    s = ParamStore("cpu")
    s.add("conv.weight", (32, 9, 32), lambda v: v.normal_())
    s.add("fc.weight", (10, 13), lambda v: v.normal_())                # 130 elements: a 6-element gap follows
    s.add("fc.bias", (10,), lambda v: v.zero_())
    assert s.sq is None
    s.finalize()
    assert s.sq is None                                                 # SGD and LARS users never allocate it
    s.init_sq()
    assert s.sq.shape == s.flat.shape and int(torch.count_nonzero(s.sq)) == 0
    first = s.sq
    s.init_sq(ones=True)
    assert s.sq is first                                                # re-initialised in place
    inside = torch.zeros(s.flat.numel(), dtype=torch.bool)
    for o, l, _, _ in s.segments(0.0):
        inside[o:o + l] = True
    assert torch.equal(s.sq, inside.float()) and int((~inside).sum()) > 0
    s.init_sq()
    assert int(torch.count_nonzero(s.sq)) == 0


# ------------------------------------------------------------------------------------------------ C-ABI
def test_header_ctypes_table_and_version_agree():
    lib = _C.lib()
    assert lib.nbdt_version() >= 120
    text = open(os.path.join(nbdt_path.ROOT, "include", "nbdt_hip.h")).read()
    assert "AdamW and RMSprop (nbdt_version() >= 120)" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    exported = set(_C.exported_symbols())
    for name, n_args in (("nbdt_arena_opt_create", 6), ("nbdt_arena_opt_destroy", 1), ("nbdt_arena_opt_n", 1),
                         ("nbdt_adamw_step", 14), ("nbdt_rmsprop_step", 14)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert m and len(m.group(1).split(",")) == n_args == len(_C.SIGNATURES[name][1]), name
        assert name in exported, name
    assert ops.ARENA_OPT_ITEM == 512
    src = open(os.path.join(nbdt_path.PKG_DIR, "csrc", "adaptive.hip")).read()
    assert re.search(r"constexpr int kItem = %d;" % ops.ARENA_OPT_ITEM, src)


def test_create_refuses_bad_tables_without_a_gpu():
    for rows, n, what in [
            ([], 64, "empty"),
            ([(12, 5, 0.0), (0, 10, 0.0)], 64, "sorted"),
            ([(0, 10, 0.0), (8, 5, 0.0)], 64, "overlap"),
            ([(0, 10, 0.0), (14, 5, 0.0)], 64, "multiples of 4"),
            ([(0, 10, 0.0), (60, 5, 0.0)], 64, "out of range"),
            ([(0, 10, 0.0), (64, 1, 0.0)], 64, "out of range"),
            ([(0, 0, 0.0)], 64, "positive"),
            ([(0, 10, -0.5)], 64, "weight decays"),
            ([(0, 10, float("nan"))], 64, "weight decays"),
            ([(0, 10, 0.0), (12, 5, 0.0)], 0, "empty arena")]:
        with pytest.raises(_C.NBDTHipError, match=what):
            ops.ArenaOptPlan(n, rows)
    lib = _C.lib()
    assert lib.nbdt_arena_opt_create(64, None, None, None, 1, None) == EINVAL
    handle = ctypes.c_void_p()
    assert lib.nbdt_arena_opt_create(64, None, None, None, 1, ctypes.byref(handle)) == EINVAL and not handle.value
    assert b"null segment table" in lib.nbdt_last_error()
    assert lib.nbdt_arena_opt_destroy(None) == 0 and lib.nbdt_arena_opt_n(None) == 0


def test_step_entries_refuse_bad_arguments_without_a_gpu():
    """The scalars are checked first, then the plan, then the pointers: with host memory standing in and no plan nothing
    is launched, and every refusal names its reason."""
    lib = _C.lib()
    nan, inf = float("nan"), float("inf")
    bufs = [torch.zeros(64) for _ in range(4)]
    P, Gp, S1, S2 = (ctypes.c_void_p(b.data_ptr()) for b in bufs)

    def adamw(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, t=1, gs=1.0, plan=None):
        return lib.nbdt_adamw_step(plan, P, Gp, S1, S2, lr, b1, b2, eps, t, gs, None, 0, None)

    def rmsprop(lr=1e-3, alpha=0.99, eps=1e-8, mu=0.9, tf=0, gs=1.0, plan=None):
        return lib.nbdt_rmsprop_step(plan, P, Gp, S2, S1, lr, alpha, eps, mu, tf, gs, None, 0, None)

    for kwargs, what in [(dict(t=0), b"step count"), (dict(t=-3), b"step count"), (dict(b1=1.0), b"betas"),
                         (dict(b1=-0.1), b"betas"), (dict(b2=1.0), b"betas"), (dict(b2=nan), b"betas"),
                         (dict(eps=-1e-8), b"eps"), (dict(eps=nan), b"eps"), (dict(lr=nan), b"finite"),
                         (dict(lr=inf), b"finite"), (dict(gs=inf), b"finite"), (dict(), b"null plan")]:
        assert adamw(**kwargs) == EINVAL and what in lib.nbdt_last_error(), (kwargs, lib.nbdt_last_error())
    for tf in (0, 1):
        for kwargs, what in [(dict(alpha=1.0), b"alpha"), (dict(alpha=-0.5), b"alpha"), (dict(alpha=nan), b"alpha"),
                             (dict(mu=1.0), b"momentum"), (dict(mu=-0.1), b"momentum"), (dict(eps=-1.0), b"eps"),
                             (dict(eps=nan), b"eps"), (dict(lr=-inf), b"finite"), (dict(lr=nan), b"finite"),
                             (dict(gs=nan), b"finite"), (dict(), b"null plan")]:
            assert rmsprop(tf=tf, **kwargs) == EINVAL and what in lib.nbdt_last_error(), (tf, kwargs)
    # the Python layer refuses host tensors before it reaches the library
    plan = object.__new__(ops.ArenaOptPlan)
    plan.n, plan.handle = 64, None
    with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
        plan.adamw(*bufs, 1e-3, (0.9, 0.999), 1e-8, 1)
    with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
        plan.rmsprop(*bufs, 1e-3, 0.99, 1e-8, 0.9)
