"""Host side of the augmentation policy (no GPU): nbdt.data.policy_reference against Pillow's bytes (the committed golden,
and Pillow itself when it imports), the draw of nbdt_policy_batch as nbdt.data.draw_policy_params restates it, the
argument checks of the C entry, which run before any HIP call, and main.py's --auto-augment / --random-erase."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import nbdt_path
from nbdt import _C
from nbdt import data as D

spec = importlib.util.spec_from_file_location("nbdt_main", os.path.join(nbdt_path.PKG_DIR, "main.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

GOLDEN = os.path.join(nbdt_path.ROOT, "tests", "golden", "policy_pil.npz")
SEED = 0            # test_every_op_and_every_bin_occurs: chosen on the CPU so that the condition holds


# ------------------------------------------------------------------------------------------------------------ pixels

def test_policy_ops_are_trivial_augment_wides_in_kernel_order():
    assert D.POLICY_OPS == ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color",
                            "Contrast", "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
    assert len(D.POLICY_OPS) == _C.NBDT_POLICY_OPS == 14 and D.POLICY_BINS == _C.NBDT_POLICY_BINS == 31
    assert sorted(D.POLICY_SIGNED) == list(range(1, 10))


def test_policy_reference_equals_the_pillow_golden_byte_for_byte():
    g = np.load(GOLDEN)
    assert str(g["pil_version"])          # the fixture says which Pillow made it
    assert tuple(g["ops"].tolist()) == D.POLICY_OPS and g["bins"].tolist() == [0, 1, 7, 15, 20, 29, 30]
    shapes = {"random": (32, 32), "low": (24, 40), "const": (16, 16)}
    checked = 0
    for name, (H, W) in shapes.items():
        img, want = g[f"img_{name}"], g[f"out_{name}"]
        assert img.shape == (3, H, W) and want.shape == (14, 7, 2, 3, H, W)
        for oi, op in enumerate(D.POLICY_OPS):
            for bi, b in enumerate(g["bins"].tolist()):
                for sg in (0, 1):
                    got = D.policy_reference(img, oi, b, sg)
                    assert got.dtype == np.uint8 and np.array_equal(got, want[oi, bi, sg]), (name, op, b, sg)
                    checked += 1
    assert checked == 3 * 14 * 7 * 2
    low, const = g["img_low"], g["img_const"]
    assert low.min() == 40 and low.max() == 199                    # AutoContrast and Equalize have work to do ...
    assert not np.array_equal(g["out_low"][12, 0, 0], low) and not np.array_equal(g["out_low"][13, 0, 0], low)
    assert all(len(np.unique(const[c])) == 1 for c in range(3))    # ... and nothing to do on a constant image
    assert np.array_equal(g["out_const"][12, 0, 0], const) and np.array_equal(g["out_const"][13, 0, 0], const)


def test_policy_reference_equals_pillow_live():
    """All 31 bins and both signs of every op against the installed Pillow, on random, low-contrast, four-level and
    constant images, square and not, with odd sides."""
    pytest.importorskip("PIL.Image")
    spec = importlib.util.spec_from_file_location("make_policy_golden",
                                                  os.path.join(nbdt_path.ROOT, "tests", "golden", "make_policy_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    rng = np.random.default_rng(3)
    imgs = []
    for H, W in ((32, 32), (64, 64), (24, 40), (9, 7)):
        imgs += [rng.integers(0, 256, (3, H, W), dtype=np.uint8), rng.integers(100, 140, (3, H, W), dtype=np.uint8),
                 (rng.integers(0, 4, (3, H, W)) * 60 + 20).astype(np.uint8), np.full((3, H, W), 77, dtype=np.uint8)]
    for img in imgs:
        for oi, op in enumerate(D.POLICY_OPS):
            for b in range(D.POLICY_BINS):
                for sg in (0, 1):
                    assert np.array_equal(D.policy_reference(img, oi, b, sg), mk.pil_op(img, op, b, sg)), \
                        (img.shape, op, b, sg)


def test_policy_reference_special_cases_and_argument_checks():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (3, 12, 12), dtype=np.uint8)
    for oi in range(14):             # bin 0 is the identity, but for the two ops without a magnitude and for Solarize
        if D.POLICY_OPS[oi] not in ("AutoContrast", "Equalize", "Solarize"):
            assert np.array_equal(D.policy_reference(img, oi, 0, 0), img), D.POLICY_OPS[oi]
    assert np.array_equal(D.policy_reference(img, "Solarize", 0, 0), np.where(img == 255, 0, img))    # threshold 255
    assert np.array_equal(D.policy_reference(img, "Rotate", 20, 0), np.rot90(img, 1, axes=(1, 2)))      # +90: transpose
    assert np.array_equal(D.policy_reference(img, "Rotate", 20, 1), np.rot90(img, -1, axes=(1, 2)))
    assert not D.policy_reference(img, "TranslateX", 15, 0).any()                                        # 16 px > 12 wide
    t = D.policy_reference(img, "TranslateY", 3, 1)                                                   # 3 px up
    assert np.array_equal(t[:, :9], img[:, 3:]) and not t[:, 9:].any()
    assert np.array_equal(D.policy_reference(img, "Posterize", 30, 0), img & 0xC0)                       # 2 bits
    assert np.array_equal(D.policy_reference(img, "Solarize", 30, 0), 255 - img)                         # threshold 0
    assert np.array_equal(D.policy_reference(torch.from_numpy(img), "Solarize", 30, 1), 255 - img)       # sign ignored
    for bad in (dict(op=14), dict(op=-1), dict(bin=31), dict(bin=-1), dict(sign=2)):
        kw = dict(op=1, bin=3, sign=0)
        kw.update(bad)
        with pytest.raises(ValueError, match="op in"):
            D.policy_reference(img, **kw)
    with pytest.raises(ValueError, match="uint8"):
        D.policy_reference(img.astype(np.float32), 0, 0, 0)
    with pytest.raises(KeyError):
        D.policy_reference(img, "Cutout", 0, 0)


def test_policy_table_layout():
    t = D.policy_table(32, 32)
    assert t.shape == (14, 31, 2, 6) and t.dtype == np.int32 and not t.flags.writeable
    assert not t[0].any() and not t[12].any() and not t[13].any()
    assert t[1, 0, 0].tolist() == [65536, 0, 32768, 0, 65536, 32768]                  # the identity in 16.16
    assert t[3, 30, 0].tolist() == [65536, 0, 32768 - 32 * 65536, 0, 65536, 32768]    # 32 px to the right
    f = t[6, :, :, 0].copy().view(np.float32)
    assert f[0, 0] == 1.0 and f[30, 0] == np.float32(1.99) and f[30, 1] == np.float32(1 - 0.99)
    assert t[10, :, 0, 0].tolist() == [0xFF & ~((1 << round(b / 5)) - 1) for b in range(31)]
    assert t[11, 0, 0, 0] == 255 and t[11, 30, 0, 0] == 0 and t[11, 1, 0, 0] == 247      # ceil(246.5)
    assert not np.array_equal(D.policy_table(24, 40)[5], t[5])       # the rotation's centre depends on the geometry
    assert np.array_equal(D.policy_table(24, 40)[:5], t[:5])
    with pytest.raises(ValueError):
        D.policy_table(0, 32)


# -------------------------------------------------------------------------------------------------------------- draw

def test_the_crop_and_flip_part_of_the_draw_is_draw_params():
    """The policy adds words to the draw, it does not touch the crop's: draw_params is unchanged (its own tests pin its
    values), and the policy words come from other multipliers of the index, so they are not a function of (dy, dx, flip)."""
    idx = np.arange(5000)
    dy, dx, fl = D.draw_params(3, 5, idx, 4)
    op, b, sg, *_ = D.draw_policy_params(3, 5, idx, 32, 32)
    same_crop = (dy == dy[0]) & (dx == dx[0]) & (fl == fl[0])
    assert same_crop.sum() > 10 and len(set(zip(op[same_crop].tolist(), b[same_crop].tolist()))) > 10


def test_policy_draw_is_deterministic_and_a_function_of_the_index_only():
    rng = np.random.default_rng(0)
    idx = rng.integers(0, 50_000, size=777)
    kw = dict(erase_prob=0.5)
    a = D.draw_policy_params(3, 5, idx, 32, 32, **kw)
    assert len(a) == 7
    for u, v in zip(a, D.draw_policy_params(3, 5, idx.copy(), 32, 32, **kw)):
        assert u.dtype == np.int64 and np.array_equal(u, v)
    p = rng.permutation(idx.size)           # a permuted batch gives permuted draws
    for u, v in zip(a, D.draw_policy_params(3, 5, idx[p], 32, 32, **kw)):
        assert np.array_equal(u[p], v)
    for u, v in zip(a, D.draw_policy_params(3, 5, torch.from_numpy(idx[:100]), 32, 32, **kw)):
        assert np.array_equal(u[:100], v)
    for u, v in zip(D.draw_policy_params(3, 5, [7, 7, 7, 11], 32, 32, **kw), D.draw_policy_params(3, 5, [11, 7], 32, 32, **kw)):
        assert u[0] == u[1] == u[2] == v[1] and u[3] == v[0]
    assert any(not np.array_equal(u, v) for u, v in zip(a, D.draw_policy_params(4, 5, idx, 32, 32, **kw)))
    assert any(not np.array_equal(u, v) for u, v in zip(a, D.draw_policy_params(3, 6, idx, 32, 32, **kw)))
    # the erase settings do not move the policy's words
    for u, v in zip(a[:3], D.draw_policy_params(3, 5, idx, 32, 32)):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("H,W", [(32, 32), (64, 64), (24, 40), (9, 7)])
def test_drawn_fields_lie_in_range_and_rectangles_inside_the_image(H, W):
    n = 20_000
    op, b, sg, top, left, h, w = D.draw_policy_params(1, 2, np.arange(n), H, W, erase_prob=1.0)
    assert op.min() == 0 and op.max() == 13 and b.min() == 0 and b.max() == 30 and set(np.unique(sg).tolist()) == {0, 1}
    assert top.min() >= 0 and left.min() >= 0 and h.min() >= 0 and w.min() >= 0
    assert h.max() < H and w.max() < W and (top + h).max() <= H and (left + w).max() <= W
    erased = (h > 0) & (w > 0)
    assert np.all((h > 0) == (w > 0)) and erased.mean() > 0.95         # p = 1: nearly every sample finds a rectangle
    assert not (top[~erased].any() or left[~erased].any())
    # h = round(sqrt(A r)), w = round(sqrt(A / r)) with A in [0.02, 0.33] H W and r in [0.3, 3.3]: each side within 1/2
    ha, wa = h[erased].astype(np.float64), w[erased].astype(np.float64)
    assert np.all((ha + 0.5) * (wa + 0.5) >= 0.02 * H * W) and np.all((ha - 0.5) * (wa - 0.5) <= 0.33 * H * W)
    assert np.all((ha + 0.5) / (wa - 0.5) >= 0.3) and np.all((ha - 0.5) / (wa + 0.5) <= 3.3)
    assert top[erased].min() == 0 and left[erased].min() == 0
    assert (top + h)[erased].max() == H and (left + w)[erased].max() == W        # positions reach both borders


def test_erase_probability():
    n = 40_000
    none = D.draw_policy_params(0, 0, np.arange(n), 32, 32, erase_prob=0.0)
    assert not any(v.any() for v in none[3:])                  # erase_prob = 0 gives none
    for p in (0.1, 0.25):
        *_, h, w = D.draw_policy_params(0, 0, np.arange(n), 32, 32, erase_prob=p)
        share = float(np.mean((h > 0) & (w > 0)))
        assert abs(share - p) < 5 * (p * (1 - p) / n) ** 0.5, (p, share)     # binomial, 5 sigma (every 32 x 32 attempt fits)
    for bad in (dict(erase_prob=-0.1), dict(erase_prob=1.5), dict(erase_prob=float("nan")),
                dict(erase_prob=0.5, erase_scale=(0.0, 0.3)), dict(erase_prob=0.5, erase_scale=(0.5, 0.4)),
                dict(erase_prob=0.5, erase_ratio=(3.0, 0.3)), dict(erase_prob=0.5, erase_ratio=(0.001, 1.0))):
        with pytest.raises(ValueError):
            D.draw_policy_params(0, 0, [0], 32, 32, **bad)
    with pytest.raises(ValueError):
        D.draw_policy_params(0, 0, [0], 0, 32)


def test_every_op_and_every_bin_occurs_among_4096_draws():
    op, b, sg, *_ = D.draw_policy_params(SEED, 0, np.arange(4096), 32, 32)
    assert sorted(set(op.tolist())) == list(range(14)) and sorted(set(b.tolist())) == list(range(31))
    assert abs(int(sg.sum()) - 2048) < 5 * 32                      # binomial, 5 sigma
    counts = np.bincount(op, minlength=14)
    assert counts.min() > 4096 / 14 - 5 * (4096 / 14) ** 0.5 and counts.max() < 4096 / 14 + 5 * (4096 / 14) ** 0.5


# ------------------------------------------------------------------------------------------------------------- C entry

def _call(sharded=False, **over):
    """nbdt_policy_batch with plausible arguments, `over` replacing some.  The pointers are never dereferenced: every case
    here is refused before the first HIP call."""
    f3 = ctypes.c_float * 3
    d2 = ctypes.c_double * 2
    P = ctypes.c_void_p
    a = dict(src=P(16), dtype=_C.NBDT_U8, labels_src=P(16), index=P(16), base=0, B=4, N=8, H=32, W=32, pad=4, flip=1,
             mean=f3(0.5, 0.5, 0.5), std=f3(0.25, 0.25, 0.25), policy=_C.NBDT_POLICY_TA_WIDE, table=P(16), erase_prob=0.25,
             scale=d2(0.02, 0.33), ratio=d2(0.3, 3.3), ratios=P(16), seed=0, epoch=0, params_in=None, policy_in=None,
             out=P(16), labels_out=P(16), params_out=None, policy_out=None)
    a.update(over)
    lib = _C.lib()
    head = (a["src"], a["dtype"], a["labels_src"], a["index"])
    tail = (a["B"], a["N"], a["H"], a["W"], a["pad"], a["flip"], a["mean"], a["std"], a["policy"], a["table"],
            a["erase_prob"], a["scale"], a["ratio"], a["ratios"], a["seed"], a["epoch"], a["params_in"], a["policy_in"],
            a["out"], a["labels_out"], a["params_out"], a["policy_out"], None)
    if sharded:
        rc = lib.nbdt_policy_batch_sharded(*head, a["base"], *tail)
    else:
        rc = lib.nbdt_policy_batch(*head, *tail)
    return rc, lib.nbdt_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(src=None), "null"), (dict(out=None), "null"), (dict(labels_out=None), "null"), (dict(index=None), "null"),
    (dict(dtype=_C.NBDT_F32), "uint8"), (dict(dtype=_C.NBDT_BF16), "uint8"),
    (dict(B=0), "batch"), (dict(N=0), "empty dataset"), (dict(H=0), "sides"), (dict(W=4097), "sides"),
    (dict(H=129, W=128), "49152"), (dict(H=4096, W=4096), "49152"),
    (dict(pad=-1), "pad"), (dict(pad=33), "pad"), (dict(flip=2), "flip"), (dict(mean=None), "mean"),
    (dict(std=(ctypes.c_float * 3)(0.5, 0.0, 0.5)), "non-zero"),
    (dict(policy=2), "policy"), (dict(policy=-1), "policy"), (dict(table=None), "policy table"),
    (dict(table=None, policy=_C.NBDT_POLICY_NONE, policy_in=ctypes.c_void_p(16)), "policy table"),
    (dict(erase_prob=-0.5), "erase_prob"), (dict(erase_prob=1.5), "erase_prob"), (dict(erase_prob=float("nan")), "erase_prob"),
    (dict(ratios=None), "ratio table"), (dict(scale=None), "ratio table"), (dict(ratio=None), "ratio table"),
    (dict(scale=(ctypes.c_double * 2)(0.0, 0.3)), "erase_scale"), (dict(scale=(ctypes.c_double * 2)(0.5, 1.5)), "erase_scale"),
    (dict(ratio=(ctypes.c_double * 2)(2.0, 1.0)), "erase_ratio"), (dict(ratio=(ctypes.c_double * 2)(0.001, 1.0)), "erase_ratio"),
])
def test_entry_refuses_bad_arguments_before_any_device_work(over, word):
    for sharded in (False, True):
        rc, msg = _call(sharded=sharded, **over)
        assert rc == -1 and word in msg, (rc, msg)


def test_sharded_entry_checks_its_base():
    for base in (-1, 2 ** 63 - 4):
        rc, msg = _call(sharded=True, base=base, H=0)          # (H = 0 would be refused next: no launch either way)
        assert rc == -1 and "index_base" in msg, (rc, msg)


def test_symbols_version_and_constants_are_in_step_with_the_header():
    assert _C.lib().nbdt_version() >= 119
    assert {"nbdt_policy_batch", "nbdt_policy_batch_sharded"} <= set(_C.exported_symbols())
    text = open(os.path.join(nbdt_path.ROOT, "include", "nbdt_hip.h")).read()
    for name in ("nbdt_policy_batch", "nbdt_policy_batch_sharded"):
        assert name in _C.SIGNATURES and f"int {name}(" in text
    assert f"#define NBDT_POLICY_OPS {_C.NBDT_POLICY_OPS}\n" in text
    assert f"#define NBDT_POLICY_BINS {_C.NBDT_POLICY_BINS}\n" in text
    assert f"#define NBDT_POLICY_TA_WIDE {_C.NBDT_POLICY_TA_WIDE}\n" in text
    # the draw's multipliers are the header's
    assert f"{D._K_POLICY:#018X}".replace("0X", "0x") in text and f"{D._K_ERASE:#018X}".replace("0X", "0x") in text
    assert D._K_POLICY % 2 == 1 and D._K_ERASE % 2 == 1 and D.POLICY_MAX_BYTES == 49152


# ------------------------------------------------------------------------------------------------ dataset and main.py

def test_device_dataset_with_a_policy_still_refuses_the_cpu():
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    y = torch.zeros(4, dtype=torch.long)
    with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
        D.DeviceDataset(x, y, (0.5,) * 3, (0.5,) * 3, 2, device="cpu", policy="ta_wide", erase_prob=0.1)


def test_main_flags_and_their_refusals():
    p = M.build_parser()
    a = p.parse_args([])
    assert a.auto_augment == "none" and a.random_erase == 0.0
    a = p.parse_args(["--auto-augment", "ta_wide", "--random-erase", "0.1"])
    assert a.auto_augment == "ta_wide" and a.random_erase == 0.1
    with pytest.raises(SystemExit):
        p.parse_args(["--auto-augment", "rand"])
    ok = ["--augment", "reference", "--data-file", "x.pt"]
    assert M.parse_args(ok + ["--auto-augment", "ta_wide", "--random-erase", "0.25"]).random_erase == 0.25
    for bad in (["--auto-augment", "ta_wide"],                                            # --augment none
                ["--random-erase", "0.1"],
                ["--augment", "reference", "--synthetic", "8", "--auto-augment", "ta_wide"],      # no --data-file
                ["--augment", "resized-crop", "--data-file", "x.pt", "--auto-augment", "ta_wide"],
                ["--augment", "resized-crop", "--data-file", "x.pt", "--random-erase", "0.1"],
                ok + ["--random-erase", "1.5"], ok + ["--random-erase", "-0.1"]):
        with pytest.raises(SystemExit):
            M.parse_args(bad)


def test_main_names_the_resized_crop_path_as_not_built(capsys):
    with pytest.raises(SystemExit):
        M.parse_args(["--augment", "resized-crop", "--data-file", "x.pt", "--auto-augment", "ta_wide"])
    assert "resized-crop is not built" in capsys.readouterr().err
