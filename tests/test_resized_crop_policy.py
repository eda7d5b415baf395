"""Host side of the policy chains on the resized-crop path (no GPU): nbdt.data.resized_crop_policy_reference against
Pillow's ``crop -> resize(BILINEAR) -> FLIP_LEFT_RIGHT -> the operations`` (the committed golden), AutoAugment's ImageNet
policy, the argument checks of nbdt_resized_crop_policy_batch, which run before any HIP call, and main.py's
``--augment resized-crop-policy``."""
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

GOLDEN = os.path.join(nbdt_path.ROOT, "tests", "golden", "resized_crop_policy_pil.npz")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
LARGEST_GOLDEN = 564410


def normalised(u8):
    mean = torch.tensor(MEAN, dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).view(3, 1, 1)
    return torch.from_numpy(np.ascontiguousarray(u8)).float().div(255).sub(mean).div(std)


def same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ pixels

def test_the_golden_is_small_and_says_where_it_came_from():
    assert os.path.getsize(GOLDEN) <= LARGEST_GOLDEN
    g = np.load(GOLDEN)
    assert str(g["pil_version"]) and tuple(g["ops"].tolist()) == D.CHAIN_OPS
    assert g["img_small"].shape == (3, 40, 36) and int(g["side_small"]) == 22
    assert g["img_large"].shape == (3, 160, 176) and int(g["side_large"]) == 144
    assert 3 * 144 * 144 > D.POLICY_MAX_BYTES                        # above what the padded-crop kernels take
    for name in ("small", "large"):                                   # AutoContrast and Equalize have work to do
        p = g[f"plain_{name}"]
        assert p.min() > 0 and p.max() < 255 and len(np.unique(p)) > 100


def test_reference_reproduces_pillow_at_22():
    """40 x 36 -> 22: all 15 operations, both signs, bins {0, middle, last} of RandAugment's and AutoAugment's tables."""
    g = np.load(GOLDEN)
    img, box, S = g["img_small"], tuple(g["box_small"].tolist()), int(g["side_small"])
    none = (0, 0, 0, 0)
    assert same(D.resized_crop_policy_reference(img, box, 1, S, [], D.chain_table("ra", S, S), none, MEAN, STD),
                normalised(g["plain_small"]))
    checked = 0
    for policy, n in (("ra", 31), ("cifar10", 10)):
        table = D.chain_table(policy, S, S)
        bins, single = g[f"bins_{n}"].tolist(), g[f"single_small_{n}"]
        assert bins == [0, n // 2, n - 1] and single.shape == (15, 3, 2, 3, S, S)
        for oi in range(15):
            for bi, b in enumerate(bins):
                for sg in (0, 1):
                    got = D.resized_crop_policy_reference(img, box, 1, S, [(oi, b, sg)], table, none, MEAN, STD)
                    assert got.dtype == torch.float32 and same(got, normalised(single[oi, bi, sg])), (policy, oi, b, sg)
                    checked += 1
    assert checked == 15 * 3 * 2 * 2
    assert not np.array_equal(single[12, 0, 0], g["plain_small"]) and not np.array_equal(single[13, 0, 0], g["plain_small"])


def test_reference_reproduces_pillow_at_144():
    """160 x 176 -> 144, past the old 49152-byte limit: the operations whose arithmetic scales with the side, and two chains."""
    g = np.load(GOLDEN)
    img, box, S = g["img_large"], tuple(g["box_large"].tolist()), int(g["side_large"])
    none = (0, 0, 0, 0)
    tables = {31: D.chain_table("ra", S, S), 10: D.chain_table("cifar10", S, S)}
    ops = g["large_ops"].tolist()
    assert ops == ["Rotate", "TranslateX", "ShearY", "Contrast", "Equalize", "Sharpness"]
    checked = 0
    for n in (31, 10):
        bins, single = g[f"bins_{n}"].tolist(), g[f"single_large_{n}"]
        assert bins == [0, n // 2, n - 1] and single.shape == (len(ops), 3, 2, 3, S, S)
        for oi, op in enumerate(ops):
            for bi, b in enumerate(bins):
                for sg in (0, 1):
                    got = D.resized_crop_policy_reference(img, box, 1, S, [(op, b, sg)], tables[n], none, MEAN, STD)
                    assert same(got, normalised(single[oi, bi, sg])), (op, n, b, sg)
                    checked += 1
    assert checked == 6 * 3 * 2 * 2
    plain = g["plain_large"]
    assert not np.array_equal(single[4, 0, 0], plain)                    # Equalize has work to do
    assert not np.array_equal(single[0, 2, 0], single[0, 2, 1])          # the two signs of a rotation differ
    chains = ((("Rotate", 1), ("Equalize", 0), ("Color", 0)),
              (("ShearX", 0), ("Contrast", 1), ("Sharpness", 0), ("AutoContrast", 0)))
    for n, b in ((31, 20), (10, 7)):
        for k, chain in enumerate(chains):
            got = D.resized_crop_policy_reference(img, box, 1, S, [(op, b, sg) for op, sg in chain], tables[n], none,
                                                  MEAN, STD)
            assert same(got, normalised(g[f"chain{k}_{n}"])), (n, k)
    # the translation follows the crop's side: int(150/331 * 144) = 65 pixels at the last bin
    assert (32768 - int(tables[31][3, 30, 0, 2])) // 65536 == int(150 / 331 * 144) == 65


def test_reference_order_flip_and_erase():
    g = np.load(GOLDEN)
    img, S = g["img_small"], 22
    table = D.chain_table("ra", S, S)
    box = (0, 0, 40, 36)
    plain = D.resample_reference(img, box, (S, S))
    a = D.resized_crop_policy_reference(img, box, 0, S, [(0, 0, 0)] * 4, table, (0, 0, 0, 0), MEAN, STD)
    assert same(a, normalised(plain))
    b = D.resized_crop_policy_reference(torch.from_numpy(img), box, 1, S, [], table, (0, 0, 0, 0), MEAN, STD)
    assert same(b, normalised(plain[:, :, ::-1]))
    # the flip comes before the chain (a shear is not symmetric), the erase after the normalisation (0.0, not (0 - mean) / std)
    c = D.resized_crop_policy_reference(img, box, 1, S, [("ShearX", 30, 0)], table, (2, 3, 5, 7), MEAN, STD)
    want = normalised(D.chain_reference(np.ascontiguousarray(plain[:, :, ::-1]), [("ShearX", 30, 0)], table))
    assert not c[:, 2:7, 3:10].any() and bool((want[:, 2:7, 3:10] != 0).all())
    want[:, 2:7, 3:10] = 0.0
    assert same(c, want)
    with pytest.raises(ValueError, match="erase"):
        D.resized_crop_policy_reference(img, box, 0, S, [], table, (20, 0, 3, 1), MEAN, STD)


# ------------------------------------------------------------------------------------------------------------ policies

def test_subpolicy_array_of_the_imagenet_policy():
    a = D.subpolicy_array("imagenet")
    assert a.shape == (25, 4, 3) and a.dtype == np.int32 and not a[:, 2:].any()
    assert len(D.IMAGENET_POLICY) == 25 and all(len(s) == 2 for s in D.IMAGENET_POLICY)
    op = D.CHAIN_OPS.index
    q = lambda p: round(p * 2 ** 24)
    assert a[0].tolist()[:2] == [[op("Posterize"), q(0.4), 8], [op("Rotate"), q(0.6), 9]]
    assert a[12].tolist()[:2] == [[op("Equalize"), 0, 0], [op("Equalize"), q(0.8), 0]]
    assert a[14].tolist()[:2] == [[op("Color"), q(0.6), 4], [op("Contrast"), 2 ** 24, 8]]
    assert a[18].tolist()[:2] == [[op("ShearX"), q(0.6), 5], [op("Equalize"), 2 ** 24, 0]]
    assert np.array_equal(a[24], a[2]) and np.array_equal(a[20], a[4]) and np.array_equal(a[21], a[1])
    assert D._chain_bins("imagenet") == D.AA_BINS == 10
    c, which = D.draw_chain_params(1, 2, np.arange(5000), "imagenet", return_subpolicy=True)
    assert which.min() == 0 and which.max() == 24 and not c[:, 2:].any() and c[:, :2, 1].max() == 9
    assert not np.array_equal(c, D.draw_chain_params(1, 2, np.arange(5000), "cifar10"))


def test_dataset_checks_its_policy_settings_before_the_device():
    x, y = torch.zeros(4, 3, 8, 8, dtype=torch.uint8), torch.zeros(4, dtype=torch.long)
    mk = lambda **kw: D.ResizedCropDataset(x, y, MEAN, STD, size=8, device="cuda", **kw)
    for kw in (dict(policy_ops=0), dict(policy_ops=5), dict(policy_magnitude=31), dict(policy_magnitude=-1)):
        with pytest.raises(ValueError, match="RandAugment"):
            mk(policy="ra", **kw)
    with pytest.raises(ValueError, match="policy must be"):
        mk(policy="rand")
    with pytest.raises(ValueError, match="sub-policy 0 slot 0"):
        mk(policy=[[("Cutout", 0.5, 3)]])
    with pytest.raises(ValueError, match="erase_prob"):
        mk(erase_prob=1.5)
    with pytest.raises(ValueError, match="scale must satisfy"):
        mk(erase_prob=0.5, erase_scale=(0.0, 0.3))
    big = torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    for kw in (dict(policy="ra"), dict(erase_prob=0.1)):
        with pytest.raises(ValueError, match="at most 512 x 512"):
            D.ResizedCropDataset(big, y[:1], MEAN, STD, size=513, resize=600, device="cuda", **kw)
    for policy in ("ta_wide", "ra", "imagenet"):
        with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
            D.ResizedCropDataset(x, y, MEAN, STD, size=8, device="cpu", policy=policy)


# ------------------------------------------------------------------------------------------------------------- C entry

def _call(sharded=False, **over):
    """nbdt_resized_crop_policy_batch with plausible arguments, `over` replacing some.  The pointers are never
    dereferenced: every case here is refused before the first HIP call."""
    f3, d2, P = ctypes.c_float * 3, ctypes.c_double * 2, ctypes.c_void_p
    a = dict(src=P(16), dtype=_C.NBDT_U8, labels_src=P(16), index=P(16), base=0, B=4, N=8, H=256, W=256, S=224, flip=1,
             mean=f3(0.5, 0.5, 0.5), std=f3(0.25, 0.25, 0.25), scale=d2(0.08, 1.0), ratio=d2(0.75, 4 / 3), ratios=P(16),
             mode=_C.NBDT_CHAIN_RAND, nbins=31, table=P(16), num_ops=2, magnitude=9, subs=None, P=0, erase_prob=0.25,
             erase_scale=d2(0.02, 0.33), erase_ratio=d2(0.3, 3.3), erase_ratios=P(16), seed=0, epoch=0, params_in=None,
             chain_in=None, erase_in=None, stage_a=P(16), stage_b=P(32), out=P(16), labels_out=P(16), params_out=None,
             chain_out=None, erase_out=None)
    a.update(over)
    lib = _C.lib()
    head = (a["src"], a["dtype"], a["labels_src"], a["index"])
    tail = (a["B"], a["N"], a["H"], a["W"], a["S"], a["flip"], a["mean"], a["std"], a["scale"], a["ratio"], a["ratios"],
            a["mode"], a["nbins"], a["table"], a["num_ops"], a["magnitude"], a["subs"], a["P"], a["erase_prob"],
            a["erase_scale"], a["erase_ratio"], a["erase_ratios"], a["seed"], a["epoch"], a["params_in"], a["chain_in"],
            a["erase_in"], a["stage_a"], a["stage_b"], a["out"], a["labels_out"], a["params_out"], a["chain_out"],
            a["erase_out"], None)
    if sharded:
        rc = lib.nbdt_resized_crop_policy_batch_sharded(*head, a["base"], *tail)
    else:
        rc = lib.nbdt_resized_crop_policy_batch(*head, *tail)
    return rc, lib.nbdt_last_error().decode()


SUB = dict(mode=_C.NBDT_CHAIN_SUBPOLICY, nbins=10, subs=ctypes.c_void_p(16), P=25)
TA = dict(mode=_C.NBDT_CHAIN_TA_WIDE, nbins=31)


@pytest.mark.parametrize("over,word", [
    (dict(src=None), "null"), (dict(out=None), "null"), (dict(labels_out=None), "null"), (dict(index=None), "null"),
    (dict(stage_a=None), "staging"), (dict(stage_b=None), "staging"), (dict(stage_b=ctypes.c_void_p(16)), "distinct"),
    (dict(stage_a=ctypes.c_void_p(24)), "16-byte aligned"),
    (dict(table=None), "table"), (dict(num_ops=0, table=None, chain_in=ctypes.c_void_p(16)), "table"),
    (dict(SUB, subs=None), "null"), (dict(SUB, table=None), "table"), (dict(TA, table=None), "table"),
    (dict(S=0), "512"), (dict(S=513), "512"), (dict(S=4096), "overflow"), (dict(H=64, W=64, S=1024), "32 bits"),
    (dict(nbins=0), "nbins"), (dict(nbins=32), "nbins"), (dict(TA, nbins=10), "nbins must be 31"),
    (dict(num_ops=-1), "num_ops"), (dict(num_ops=5), "num_ops"),
    (dict(magnitude=31), "magnitude"), (dict(magnitude=-1), "magnitude"), (dict(nbins=10, magnitude=10), "magnitude"),
    (dict(SUB, P=0), "sub-policies"), (dict(SUB, P=1025), "sub-policies"),
    (dict(mode=3), "mode"), (dict(mode=-1), "mode"),
    (dict(dtype=_C.NBDT_F32), "uint8"), (dict(H=0), "image sides"), (dict(W=4097), "image sides"),
    (dict(erase_prob=float("nan")), "erase_prob"), (dict(erase_prob=1.5), "erase_prob"),
    (dict(B=0), "batch"), (dict(N=0), "empty dataset"), (dict(flip=2), "flip"),
    (dict(ratios=None), "ratio table"), (dict(erase_ratios=None), "ratio table"),
    (dict(erase_scale=(ctypes.c_double * 2)(0.0, 0.3)), "erase_scale"), (dict(scale=(ctypes.c_double * 2)(0.0, 0.3)), "scale"),
])
def test_entry_refuses_bad_arguments_before_any_device_work(over, word):
    for sharded in (False, True):
        rc, msg = _call(sharded=sharded, **over)
        assert rc == -1 and word in msg, (rc, msg)


def test_sharded_entry_checks_its_base():
    for base in (-1, 2 ** 63 - 4):
        rc, msg = _call(sharded=True, base=base, H=0)          # (H = 0 would be refused next: no launch either way)
        assert rc == -1 and "index_base" in msg, (rc, msg)


def test_the_padded_crop_entry_keeps_refusing_the_new_mode():
    f3, d2, P = ctypes.c_float * 3, ctypes.c_double * 2, ctypes.c_void_p
    rc = _C.lib().nbdt_policy_chain_batch(P(16), _C.NBDT_U8, P(16), P(16), 4, 8, 32, 32, 4, 1, f3(0.5, 0.5, 0.5),
                                          f3(0.25, 0.25, 0.25), _C.NBDT_CHAIN_TA_WIDE, 31, P(16), 2, 9, None, 0, 0.0, None,
                                          None, None, 0, 0, None, None, None, P(16), P(16), None, None, None, None)
    assert rc == -1 and "mode" in _C.lib().nbdt_last_error().decode()


def test_symbols_version_and_constants_are_in_step_with_the_header():
    assert _C.lib().nbdt_version() >= 124
    names = ("nbdt_resized_crop_policy_batch", "nbdt_resized_crop_policy_batch_sharded")
    assert set(names) <= set(_C.exported_symbols())
    text = open(os.path.join(nbdt_path.ROOT, "include", "nbdt_hip.h")).read()
    assert "resized-crop policy (nbdt_version() >= 124)" in text
    for name in names:
        assert name in _C.SIGNATURES and f"int {name}(" in text
    for name in ("NBDT_CHAIN_TA_WIDE", "NBDT_RESIZED_CROP_POLICY_MAX_SIDE"):
        assert f"#define {name} {getattr(_C, name)}\n" in text
    assert _C.NBDT_CHAIN_TA_WIDE == 2 and _C.NBDT_RESIZED_CROP_POLICY_MAX_SIDE == D.RESIZED_CROP_POLICY_MAX_SIDE == 512
    assert f"{D._K_POLICY:#018X}".replace("0X", "0x") in text.split("resized-crop policy (nbdt_version() >= 124)")[1]


def test_both_translation_units_keep_ieee_arithmetic():
    from nbdt import _build
    want = ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]
    assert _build.FLAGS["resample.hip"] == want and _build.FLAGS["policy.hip"] == want
    for name in ("resample.hip", "policy.hip"):
        assert '#include "policy_ops.h"' in open(os.path.join(_build.CSRC, name)).read()


# ------------------------------------------------------------------------------------------------------------ main.py

def test_main_accepts_the_new_augment_value():
    ok = ["--augment", "resized-crop-policy", "--data-file", "x.pt", "--dataset", "Imagenet1000"]
    assert M.parse_args(ok).augment == "resized-crop-policy"
    for policy in ("ta_wide", "ra", "cifar10", "imagenet"):
        a = M.parse_args(ok + ["--auto-augment", policy])
        assert (a.augment, a.auto_augment, a.random_erase) == ("resized-crop-policy", policy, 0.0)
        assert M.resized_crop_family(a)
    a = M.parse_args(ok + ["--random-erase", "0.1"])
    assert a.random_erase == 0.1 and a.auto_augment == "none"
    a = M.parse_args(ok + ["--auto-augment", "ra", "--ra-num-ops", "3", "--ra-magnitude", "14", "--random-erase", "0.25",
                           "--crop-size", "64", "--shard-data"])
    assert (a.ra_num_ops, a.ra_magnitude, a.random_erase, a.crop_size, a.shard_data) == (3, 14, 0.25, 64, True)
    assert M.parse_args(["--augment", "reference", "--data-file", "x.pt", "--auto-augment", "imagenet"]).auto_augment \
        == "imagenet"
    assert M.resized_crop_family(M.parse_args(["--augment", "resized-crop"]))
    assert not M.resized_crop_family(M.parse_args(["--augment", "reference"]))
    for bad in (["--ra-num-ops", "5"], ["--ra-magnitude", "31"], ["--random-erase", "1.5"]):
        with pytest.raises(SystemExit):
            M.parse_args(ok + ["--auto-augment", "ra"] + bad)


def test_main_refuses_the_new_value_without_a_data_file(capsys):
    for extra in ([], ["--synthetic", "8"], ["--auto-augment", "ra"], ["--random-erase", "0.1"]):
        with pytest.raises(SystemExit):
            M.parse_args(["--augment", "resized-crop-policy"] + extra)
        assert "--data-file" in capsys.readouterr().err


def test_the_old_refusal_still_fires_and_points_at_the_new_value(capsys):
    for extra in (["--auto-augment", "ra"], ["--auto-augment", "imagenet"], ["--random-erase", "0.1"]):
        with pytest.raises(SystemExit):
            M.parse_args(["--augment", "resized-crop", "--data-file", "x.pt"] + extra)
        err = capsys.readouterr().err
        assert "resized-crop is not built" in err and "--augment resized-crop-policy" in err
