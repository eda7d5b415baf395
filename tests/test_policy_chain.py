"""Host side of the policy chains -- RandAugment and AutoAugment (no GPU): nbdt.data.chain_reference against Pillow's bytes
(the committed golden, and Pillow itself when it imports), chain_table's magnitudes, the draw of nbdt_policy_chain_batch as
nbdt.data.draw_chain_params restates it, the argument checks of the C entry, which run before any HIP call, main.py's
--auto-augment ra / cifar10 and DeviceDataset's host-side validation."""
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

GOLDEN = os.path.join(nbdt_path.ROOT, "tests", "golden", "policy_chain_pil.npz")
SEED = 0            # the counting tests: checked on the CPU that the six-sigma conditions hold for this seed
N_COUNT = 200_000


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_policy_chain_golden", os.path.join(nbdt_path.ROOT, "tests", "golden", "make_policy_chain_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


# ------------------------------------------------------------------------------------------------------------ pixels

def test_chain_ops_are_the_policy_ops_and_invert():
    assert D.CHAIN_OPS == D.POLICY_OPS + ("Invert",) and len(D.CHAIN_OPS) == _C.NBDT_CHAIN_OPS == 15
    assert len(D.POLICY_OPS) == _C.NBDT_POLICY_OPS == 14 and D.CHAIN_MAX_OPS == _C.NBDT_CHAIN_MAX_OPS == 4
    assert len(D.CIFAR10_POLICY) == 25 and all(len(s) == 2 for s in D.CIFAR10_POLICY)


def test_chain_reference_equals_the_pillow_golden_byte_for_byte():
    g = np.load(GOLDEN)
    assert str(g["pil_version"]) and tuple(g["ops"].tolist()) == D.CHAIN_OPS
    checked = 0
    for name, (H, W) in {"random": (9, 7), "low": (18, 16)}.items():
        img = g[f"img_{name}"]
        assert img.shape == (3, H, W)
        for policy, n, pair_bin in (("ra", 31, 9), ("cifar10", 10, 7)):
            table = D.chain_table(policy, H, W)
            bins, single, pairs = g[f"bins_{name}_{n}"].tolist(), g[f"single_{name}_{n}"], g[f"pairs_{name}_{n}"]
            assert single.shape == (15, len(bins), 2, 3, H, W) and pairs.shape == (15, 15, 3, H, W)
            assert bins == (list(range(n)) if name == "random" else bins)
            for oi in range(15):
                for bi, b in enumerate(bins):
                    for sg in (0, 1):
                        got = D.chain_reference(img, [(oi, b, sg)], table)
                        assert got.dtype == np.uint8 and np.array_equal(got, single[oi, bi, sg]), (name, policy, oi, b, sg)
                        checked += 1
                for oj in range(15):
                    got = D.chain_reference(img, [(oi, pair_bin, 0), (D.CHAIN_OPS[oj], pair_bin, 1)], table)
                    assert np.array_equal(got, pairs[oi, oj]), (name, policy, oi, oj)
                    checked += 1
    assert checked == 15 * 2 * (31 + 10 + 5 + 3) + 4 * 225
    low = g["img_low"]
    assert low.min() == 40 and low.max() == 199                    # AutoContrast and Equalize have work to do
    assert not np.array_equal(g["single_low_31"][12, 0, 0], low) and not np.array_equal(g["single_low_31"][13, 0, 0], low)
    assert np.array_equal(g["single_low_31"][14, 0, 0], 255 - low)


def _fixtures(H, W, rng):
    return [rng.integers(0, 256, (3, H, W), dtype=np.uint8), rng.integers(100, 140, (3, H, W), dtype=np.uint8),
            (rng.integers(0, 4, (3, H, W)) * 60 + 20).astype(np.uint8), np.full((3, H, W), 77, dtype=np.uint8)]


def test_chain_reference_equals_pillow_live():
    """Every op x every bin x both signs under the ra (n = 31) and the cifar10 (n = 10) table, and all 15 x 15 ordered
    pairs at one bin as two successive Pillow calls, on random, low-contrast, four-level and constant images at 32 x 32,
    24 x 40 and 9 x 7: zero differing bytes."""
    pytest.importorskip("PIL.Image")
    mk = _generator()
    rng = np.random.default_rng(3)
    for H, W in ((32, 32), (24, 40), (9, 7)):
        for policy, n in (("ra", 31), ("cifar10", 10)):
            table = D.chain_table(policy, H, W)
            for img in _fixtures(H, W, rng):
                for oi, op in enumerate(D.CHAIN_OPS):
                    for b in range(n):
                        for sg in (0, 1):
                            assert np.array_equal(D.chain_reference(img, [(oi, b, sg)], table),
                                                  mk.pil_chain(img, [(op, b, sg)], n)), (img.shape, policy, op, b, sg)
                b = n // 3
                for p in D.CHAIN_OPS:
                    for q in D.CHAIN_OPS:
                        assert np.array_equal(D.chain_reference(img, [(p, b, 0), (q, b, 1)], table),
                                              mk.pil_chain(img, [(p, b, 0), (q, b, 1)], n)), (img.shape, policy, p, q)


def test_chain_reference_composes_and_checks_its_arguments():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (3, 20, 20), dtype=np.uint8)           # (Equalize needs more than 255 pixels a channel)
    table = D.chain_table("ra", 20, 20)
    assert np.array_equal(D.chain_reference(img, [], table), img)
    assert np.array_equal(D.chain_reference(img, [(0, 0, 0)] * 4, table), img)
    assert np.array_equal(D.chain_reference(img, [("Invert", 0, 0)], table), 255 - img)
    assert np.array_equal(D.chain_reference(torch.from_numpy(img), [("Invert", 0, 0), (14, 3, 1)], table), img)
    one = D.chain_reference(img, [("Rotate", 30, 0)], table)
    two = D.chain_reference(img, [("Rotate", 30, 0), ("Equalize", 0, 0)], table)
    assert np.array_equal(two, D.chain_reference(one, [("Equalize", 0, 0)], table)) and not np.array_equal(one, two)
    # the order matters: the zero fill of a geometric op changes the statistics of what follows
    assert not np.array_equal(two, D.chain_reference(img, [("Equalize", 0, 0), ("Rotate", 30, 0)], table))
    for bad in ([(15, 0, 0)], [(-1, 0, 0)], [(1, 31, 0)], [(1, -1, 0)], [(1, 0, 2)]):
        with pytest.raises(ValueError, match="op in"):
            D.chain_reference(img, bad, table)
    with pytest.raises(ValueError, match="op in"):
        D.chain_reference(img, [(1, 10, 0)], D.chain_table("cifar10", 20, 20))          # bin 10 of 10
    with pytest.raises(ValueError, match="uint8"):
        D.chain_reference(img.astype(np.float32), [], table)
    with pytest.raises(ValueError, match="table"):
        D.chain_reference(img, [], D.policy_table(20, 20))
    with pytest.raises(KeyError):
        D.chain_reference(img, [("Cutout", 0, 0)], table)


def test_chain_table():
    ra, aa = D.chain_table("ra", 32, 32), D.chain_table("cifar10", 32, 32)
    assert ra.shape == (15, 31, 2, 6) and aa.shape == (15, 10, 2, 6) and ra.dtype == aa.dtype == np.int32
    assert not ra.flags.writeable and not ra[0].any() and not ra[12:].any() and not aa[12:].any()
    # TrivialAugment's ranges give policy_table's rows (and an Invert row without a magnitude)
    for H, W in ((32, 32), (24, 40), (9, 7)):
        ta = D.chain_table("ta_wide", H, W)
        assert ta.shape == (15, 31, 2, 6) and np.array_equal(ta[:14], D.policy_table(H, W)) and not ta[14].any()
    px = lambda t, op, b, sg, word: (32768 - int(t[op, b, sg, word])) // 65536
    assert px(ra, 3, 9, 0, 2) == 4 and px(ra, 3, 9, 1, 2) == -4                  # int((150/331) * 32 * 9/30) = 4
    assert px(aa, 3, 9, 0, 2) == 14 and px(aa, 4, 9, 0, 5) == 14                 # int((150/331) * 32) = 14
    wide = D.chain_table("ra", 24, 40)
    assert px(wide, 3, 30, 0, 2) == int(150 / 331 * 40) == 18 and px(wide, 4, 30, 0, 5) == int(150 / 331 * 24) == 10
    f = ra[6, :, :, 0].copy().view(np.float32)
    assert f[0, 0] == 1.0 and f[30, 0] == np.float32(1.9) and f[30, 1] == np.float32(1 - 0.9)
    assert all(np.array_equal(ra[6, :, :, 0], ra[k, :, :, 0]) for k in (7, 8, 9))
    assert ra[10, :, 0, 0].tolist() == [0xFF & ~((1 << round(b / 7.5)) - 1) for b in range(31)]
    assert aa[10, :, 0, 0].tolist() == [0xFF & ~((1 << round(b / 2.25)) - 1) for b in range(10)]
    assert ra[11, 0, 0, 0] == 255 and ra[11, 30, 0, 0] == 0 and aa[11, 9, 0, 0] == 0 and aa[11, 2, 0, 0] == 199      # ceil(198.33)
    assert ra[1, 30, 0].tolist() == [65536, D._fix(0.3), D._fix(0.5 + 0.5 * 0.3), 0, 65536, 32768]
    assert np.array_equal(D.chain_table([[("Rotate", 0.5, 3)]], 32, 32), aa)        # a user list: AutoAugment's bins
    for bad in ("rand", "imagenet"):
        with pytest.raises(ValueError):
            D.chain_table(bad, 32, 32)
    with pytest.raises(ValueError):
        D.chain_table("ra", 0, 32)


def test_subpolicy_array_of_the_cifar10_policy():
    a = D.subpolicy_array("cifar10")
    assert a.shape == (25, 4, 3) and a.dtype == np.int32 and not a[:, 2:].any()
    op = D.CHAIN_OPS.index
    assert a[0].tolist()[:2] == [[op("Invert"), round(0.1 * 2 ** 24), 0], [op("Contrast"), round(0.2 * 2 ** 24), 6]]
    assert a[1].tolist()[:2] == [[op("Rotate"), round(0.7 * 2 ** 24), 2], [op("TranslateX"), round(0.3 * 2 ** 24), 9]]
    assert a[14].tolist()[:2] == [[op("Solarize"), 2 ** 23, 2], [op("Invert"), 0, 0]]
    assert a[21].tolist()[:2] == [[op("TranslateY"), round(0.9 * 2 ** 24), 9], [op("TranslateY"), round(0.7 * 2 ** 24), 9]]
    assert a[24].tolist()[:2] == [[op("TranslateY"), round(0.7 * 2 ** 24), 9], [op("AutoContrast"), round(0.9 * 2 ** 24), 0]]
    names = [[D.CHAIN_OPS[s[0]] for s in sub[:2]] for sub in a.tolist()]
    assert names[4] == ["AutoContrast", "Equalize"] and names[8] == ["Equalize", "Equalize"] and names[19] == ["Brightness", "Color"]
    assert a[:, :2, 2].max() == 9 and a[:, :2, 1].max() == round(0.9 * 2 ** 24)
    assert D.subpolicy_array([[("Equalize", 1, None)]])[0, 0].tolist() == [13, 2 ** 24, 0]


@pytest.mark.parametrize("policy,word", [
    ([[("Rotate", 0.5, 3)], [("Cutout", 0.5, 3)]], "sub-policy 1 slot 0"),
    ([[("Rotate", 0.5, 3), ("Color", 1.5, 3)]], "sub-policy 0 slot 1"),
    ([[("Rotate", 0.5, 3), ("Color", -0.1, 3)]], "sub-policy 0 slot 1"),
    ([[("Rotate", float("nan"), 3)]], "sub-policy 0 slot 0"),
    ([[("Rotate", 0.5, 10)]], "sub-policy 0 slot 0"),
    ([[("Rotate", 0.5, -1)]], "sub-policy 0 slot 0"),
    ([[("Rotate", 0.5, 2.5)]], "sub-policy 0 slot 0"),
    ([[("Rotate", 0.5)]], "sub-policy 0 slot 0"),
    ([[("Rotate", 0.5, 3)], []], "sub-policy 1"),
    ([[("Rotate", 0.5, 3)] * 5], "sub-policy 0"),
    ([], "sub-policies"),
])
def test_a_bad_list_of_subpolicies_is_a_value_error_naming_the_slot(policy, word):
    x, y = torch.zeros(4, 3, 8, 8, dtype=torch.uint8), torch.zeros(4, dtype=torch.long)
    with pytest.raises(ValueError, match=word):
        D.subpolicy_array(policy)
    with pytest.raises(ValueError, match=word):           # (validated before the device is touched)
        D.DeviceDataset(x, y, (0.5,) * 3, (0.5,) * 3, 2, device="cuda", policy=policy)


def test_device_dataset_checks_the_randaugment_settings_and_still_refuses_the_cpu():
    x, y = torch.zeros(4, 3, 8, 8, dtype=torch.uint8), torch.zeros(4, dtype=torch.long)
    for kw in (dict(policy_ops=0), dict(policy_ops=5), dict(policy_magnitude=31), dict(policy_magnitude=-1),
               dict(policy_ops=2.0)):
        with pytest.raises(ValueError, match="RandAugment"):
            D.DeviceDataset(x, y, (0.5,) * 3, (0.5,) * 3, 2, device="cuda", policy="ra", **kw)
    with pytest.raises(ValueError, match="policy must be"):
        D.DeviceDataset(x, y, (0.5,) * 3, (0.5,) * 3, 2, device="cuda", policy="rand")
    for policy in ("ra", "cifar10", [[("Invert", 1.0, None)]]):
        with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
            D.DeviceDataset(x, y, (0.5,) * 3, (0.5,) * 3, 2, device="cpu", policy=policy)


# -------------------------------------------------------------------------------------------------------------- draw

USER = [[("Rotate", 1.0, 3), ("Invert", 0.0, None)], [("Equalize", 0.0, None), ("Solarize", 1.0, 9), ("Color", 0.5, 4)]]
SETTINGS = [dict(policy="ra"), dict(policy="ra", num_ops=1, magnitude=0), dict(policy="ra", num_ops=4, magnitude=30),
            dict(policy="cifar10"), dict(policy=USER)]


@pytest.mark.parametrize("kw", SETTINGS)
def test_chain_draw_is_a_pure_function_of_the_index(kw):
    rng = np.random.default_rng(0)
    idx = rng.integers(0, 50_000, size=777)
    a = D.draw_chain_params(3, 5, idx, **kw)
    assert a.shape == (777, 4, 3) and a.dtype == np.int64
    assert np.array_equal(a, D.draw_chain_params(3, 5, idx.copy(), **kw))
    assert np.array_equal(a, np.concatenate([D.draw_chain_params(3, 5, idx[:300], **kw),
                                             D.draw_chain_params(3, 5, idx[300:], **kw)]))       # halves concatenate
    p = rng.permutation(idx.size)                                                                   # any batch order
    assert np.array_equal(a[p], D.draw_chain_params(3, 5, idx[p], **kw))
    assert np.array_equal(a[:100], D.draw_chain_params(3, 5, torch.from_numpy(idx[:100]), **kw))
    b = D.draw_chain_params(3, 5, [7, 7, 11], **kw)
    assert np.array_equal(b[0], b[1]) and np.array_equal(b[[2, 0]], D.draw_chain_params(3, 5, [11, 7], **kw))
    assert not np.array_equal(a, D.draw_chain_params(4, 5, idx, **kw))
    assert not np.array_equal(a, D.draw_chain_params(3, 6, idx, **kw))


@pytest.mark.parametrize("N,Mg", [(1, 0), (2, 9), (3, 30), (4, 15)])
def test_randaugment_draw_fields(N, Mg):
    c, which = D.draw_chain_params(1, 2, np.arange(20_000), "ra", N, Mg, return_subpolicy=True)
    assert not which.any()
    assert c[:, :N, 0].min() == 0 and c[:, :N, 0].max() == 13                  # Invert is not in RandAugment's space
    assert np.all(c[:, :N, 1] == Mg) and set(np.unique(c[:, :N, 2]).tolist()) == {0, 1}
    assert not c[:, N:].any()                                                  # exactly N slots, the rest is padding
    # the slots of one sample are independent draws
    if N >= 2:
        assert 0.04 < float(np.mean(c[:, 0, 0] == c[:, 1, 0])) < 0.11           # 1/14
    for bad in (dict(num_ops=0), dict(num_ops=5), dict(magnitude=31), dict(magnitude=-1)):
        with pytest.raises(ValueError, match="RandAugment"):
            D.draw_chain_params(0, 0, [0], "ra", **bad)


def test_cifar10_draw_fields():
    c, which = D.draw_chain_params(1, 2, np.arange(20_000), "cifar10", return_subpolicy=True)
    assert which.min() == 0 and which.max() == 24 and not c[:, 2:].any()
    subs = D.subpolicy_array("cifar10")
    applied = c[:, :2, 0] != 0
    want = subs[which][:, :2]
    assert np.array_equal(c[:, :2, 0][applied], want[:, :, 0][applied])         # an applied slot is the sub-policy's
    assert np.array_equal(c[:, :2, 1][applied], want[:, :, 2][applied])
    assert not c[:, :2, 1:][~applied].any()                                     # a skipped one is Identity (0, 0, 0)
    assert set(np.unique(c[:, :2, 2][applied]).tolist()) == {0, 1}


def _within(count, n, p, sigmas=6.0):
    return abs(count - n * p) <= sigmas * (n * p * (1 - p)) ** 0.5


def test_randaugment_frequencies_over_200000_indices():
    c = D.draw_chain_params(SEED, 0, np.arange(N_COUNT), "ra", 4, 9)
    for k in range(4):
        counts = np.bincount(c[:, k, 0], minlength=14)
        assert counts.shape == (14,) and all(_within(int(v), N_COUNT, 1 / 14) for v in counts), (k, counts)
        assert _within(int(c[:, k, 2].sum()), N_COUNT, 0.5), k


def test_subpolicy_frequencies_over_200000_indices():
    c, which = D.draw_chain_params(SEED, 0, np.arange(N_COUNT), "cifar10", return_subpolicy=True)
    counts = np.bincount(which, minlength=25)
    assert counts.shape == (25,) and all(_within(int(v), N_COUNT, 1 / 25) for v in counts), counts
    for i, sub in enumerate(D.CIFAR10_POLICY):
        own = c[which == i]
        for k, (name, p, _) in enumerate(sub):
            applied = int((own[:, k, 0] == D.CHAIN_OPS.index(name)).sum())
            assert applied == int((own[:, k, 0] != 0).sum())
            assert _within(applied, len(own), p), (i, k, name, p, applied, len(own))
            if p == 0.0:
                assert applied == 0
            neg = int(own[own[:, k, 0] != 0][:, k, 2].sum())
            assert _within(neg, applied, 0.5), (i, k, neg, applied)
    assert int((c[which == 14][:, 1, 0] != 0).sum()) == 0              # Invert .0 is never applied


def test_probability_zero_never_applies_and_one_always():
    c, which = D.draw_chain_params(SEED, 1, np.arange(N_COUNT), USER, return_subpolicy=True)
    assert _within(int((which == 0).sum()), N_COUNT, 0.5)
    a, b = c[which == 0], c[which == 1]
    assert np.all(a[:, 0, 0] == 5) and np.all(a[:, 0, 1] == 3) and not a[:, 1:].any()               # p = 1 / p = 0
    assert not b[:, 0].any() and np.all(b[:, 1, 0] == 11) and np.all(b[:, 1, 1] == 9) and not b[:, 3].any()
    assert _within(int((b[:, 2, 0] == 7).sum()), len(b), 0.5) and set(np.unique(b[:, 2, 0]).tolist()) == {0, 7}


def test_the_chain_leaves_the_crop_and_the_erase_draw_alone():
    """draw_params and the erase rectangles of draw_policy_params are what they were (their own tests pin their values);
    the chain's words come from another multiplier of the index, so they are not a function of either."""
    idx = np.arange(5000)
    # values recorded from the parent commit's draw_params / draw_policy_params
    dy, dx, fl = D.draw_params(3, 5, idx[:6], 4)
    assert (dy.tolist(), dx.tolist(), fl.tolist()) == PINNED_CROP
    *_, top, left, h, w = D.draw_policy_params(3, 5, idx[:6], 32, 32, erase_prob=1.0)
    assert (top.tolist(), left.tolist(), h.tolist(), w.tolist()) == PINNED_ERASE
    dy, dx, fl = D.draw_params(3, 5, idx, 4)
    op, *_ = D.draw_policy_params(3, 5, idx, 32, 32)
    c = D.draw_chain_params(3, 5, idx, "ra", 2, 9)
    same_crop = (dy == dy[0]) & (dx == dx[0]) & (fl == fl[0])
    assert same_crop.sum() > 10 and len(set(map(tuple, c[same_crop][:, :2, 0].tolist()))) > 10
    assert 0.03 < float(np.mean(c[:, 0, 0] == op)) < 0.12              # not TrivialAugment's op either (1/14 by chance)
    assert D._K_CHAIN % 2 == 1 and D._K_CHAIN not in (D._K_POLICY, D._K_ERASE, 0xD1342543DE82EF95)


PINNED_CROP = ([7, 8, 7, 4, 1, 7], [3, 0, 5, 0, 7, 2], [0, 0, 0, 0, 1, 1])
PINNED_ERASE = ([9, 18, 13, 6, 1, 12], [14, 11, 12, 10, 0, 7], [10, 13, 10, 25, 13, 13], [11, 5, 5, 12, 20, 7])


# ------------------------------------------------------------------------------------------------------------- C entry

def _call(sharded=False, **over):
    """nbdt_policy_chain_batch with plausible arguments, `over` replacing some.  The pointers are never dereferenced: every
    case here is refused before the first HIP call."""
    f3 = ctypes.c_float * 3
    d2 = ctypes.c_double * 2
    P = ctypes.c_void_p
    a = dict(src=P(16), dtype=_C.NBDT_U8, labels_src=P(16), index=P(16), base=0, B=4, N=8, H=32, W=32, pad=4, flip=1,
             mean=f3(0.5, 0.5, 0.5), std=f3(0.25, 0.25, 0.25), mode=_C.NBDT_CHAIN_RAND, nbins=31, table=P(16), num_ops=2,
             magnitude=9, subs=None, P=0, erase_prob=0.25, scale=d2(0.02, 0.33), ratio=d2(0.3, 3.3), ratios=P(16), seed=0,
             epoch=0, params_in=None, chain_in=None, erase_in=None, out=P(16), labels_out=P(16), params_out=None,
             chain_out=None, erase_out=None)
    a.update(over)
    lib = _C.lib()
    head = (a["src"], a["dtype"], a["labels_src"], a["index"])
    tail = (a["B"], a["N"], a["H"], a["W"], a["pad"], a["flip"], a["mean"], a["std"], a["mode"], a["nbins"], a["table"],
            a["num_ops"], a["magnitude"], a["subs"], a["P"], a["erase_prob"], a["scale"], a["ratio"], a["ratios"], a["seed"],
            a["epoch"], a["params_in"], a["chain_in"], a["erase_in"], a["out"], a["labels_out"], a["params_out"],
            a["chain_out"], a["erase_out"], None)
    if sharded:
        rc = lib.nbdt_policy_chain_batch_sharded(*head, a["base"], *tail)
    else:
        rc = lib.nbdt_policy_chain_batch(*head, *tail)
    return rc, lib.nbdt_last_error().decode()


SUB = dict(mode=_C.NBDT_CHAIN_SUBPOLICY, nbins=10, subs=ctypes.c_void_p(16), P=25)


@pytest.mark.parametrize("over,word", [
    (dict(src=None), "null"), (dict(out=None), "null"), (dict(labels_out=None), "null"), (dict(index=None), "null"),
    (dict(labels_src=None), "null"), (dict(table=None), "null"), (dict(SUB, subs=None), "null"),
    (dict(nbins=0), "nbins"), (dict(nbins=32), "nbins"), (dict(SUB, nbins=0), "nbins"),
    (dict(num_ops=0), "num_ops"), (dict(num_ops=5), "num_ops"),
    (dict(magnitude=31), "magnitude"), (dict(magnitude=-1), "magnitude"), (dict(nbins=10, magnitude=10), "magnitude"),
    (dict(SUB, P=0), "sub-policies"), (dict(SUB, P=1025), "sub-policies"),
    (dict(mode=2), "mode"), (dict(mode=-1), "mode"),
    (dict(dtype=_C.NBDT_F32), "uint8"), (dict(H=129, W=128), "49152"), (dict(H=4096, W=4096), "49152"),
    (dict(erase_prob=float("nan")), "erase_prob"), (dict(erase_prob=1.5), "erase_prob"),
    (dict(B=0), "batch"), (dict(N=0), "empty dataset"), (dict(pad=33), "pad"), (dict(flip=2), "flip"),
    (dict(ratios=None), "ratio table"), (dict(scale=(ctypes.c_double * 2)(0.0, 0.3)), "erase_scale"),
])
def test_entry_refuses_bad_arguments_before_any_device_work(over, word):
    for sharded in (False, True):
        rc, msg = _call(sharded=sharded, **over)
        assert rc == -1 and word in msg, (rc, msg)


def test_sharded_entry_checks_its_base():
    for base in (-1, 2 ** 63 - 4):
        rc, msg = _call(sharded=True, base=base, H=0)          # (H = 0 would be refused next: no launch either way)
        assert rc == -1 and "index_base" in msg, (rc, msg)


def test_the_single_op_entry_keeps_refusing_a_third_policy():
    f3, P = ctypes.c_float * 3, ctypes.c_void_p
    rc = _C.lib().nbdt_policy_batch(P(16), _C.NBDT_U8, P(16), P(16), 4, 8, 32, 32, 4, 1, f3(0.5, 0.5, 0.5),
                                    f3(0.25, 0.25, 0.25), 2, P(16), 0.0, None, None, None, 0, 0, None, None, P(16), P(16),
                                    None, None, None)
    assert rc == -1 and "policy" in _C.lib().nbdt_last_error().decode()


def test_symbols_version_and_constants_are_in_step_with_the_header():
    assert _C.lib().nbdt_version() >= 123
    assert {"nbdt_policy_chain_batch", "nbdt_policy_chain_batch_sharded"} <= set(_C.exported_symbols())
    text = open(os.path.join(nbdt_path.ROOT, "include", "nbdt_hip.h")).read()
    assert "policy chains (nbdt_version() >= 123)" in text
    for name in ("nbdt_policy_chain_batch", "nbdt_policy_chain_batch_sharded"):
        assert name in _C.SIGNATURES and f"int {name}(" in text
    for name in ("NBDT_CHAIN_OPS", "NBDT_CHAIN_MAX_OPS", "NBDT_CHAIN_MAX_BINS", "NBDT_CHAIN_MAX_SUBPOLICIES", "NBDT_CHAIN_RAND",
                 "NBDT_CHAIN_SUBPOLICY", "NBDT_POLICY_OPS", "NBDT_POLICY_BINS"):
        assert f"#define {name} {getattr(_C, name)}\n" in text
    assert _C.NBDT_CHAIN_OPS == 15 and _C.NBDT_POLICY_OPS == 14 and _C.NBDT_CHAIN_MAX_OPS == 4
    assert f"{D._K_CHAIN:#018X}".replace("0X", "0x") in text            # the draw's multiplier is the header's
    assert D.RA_BINS == _C.NBDT_CHAIN_MAX_BINS == 31 and D.AA_BINS == 10


# ------------------------------------------------------------------------------------------------------------ main.py

def test_main_flags_and_their_refusals():
    p = M.build_parser()
    a = p.parse_args([])
    assert a.auto_augment == "none" and a.ra_num_ops == 2 and a.ra_magnitude == 9
    for choice in ("ta_wide", "ra", "cifar10"):
        assert p.parse_args(["--auto-augment", choice]).auto_augment == choice
    with pytest.raises(SystemExit):
        p.parse_args(["--auto-augment", "rand"])
    ok = ["--augment", "reference", "--data-file", "x.pt"]
    a = M.parse_args(ok + ["--auto-augment", "ra", "--ra-num-ops", "3", "--ra-magnitude", "14", "--random-erase", "0.25"])
    assert (a.auto_augment, a.ra_num_ops, a.ra_magnitude, a.random_erase) == ("ra", 3, 14, 0.25)
    assert M.parse_args(ok + ["--auto-augment", "ra", "--ra-num-ops", "4", "--ra-magnitude", "30"]).ra_magnitude == 30
    assert M.parse_args(ok + ["--auto-augment", "ra", "--ra-num-ops", "1", "--ra-magnitude", "0"]).ra_num_ops == 1
    assert M.parse_args(ok + ["--auto-augment", "cifar10"]).auto_augment == "cifar10"
    for policy in ("ra", "cifar10"):
        for bad in (["--auto-augment", policy],                                                       # --augment none
                    ["--augment", "reference", "--synthetic", "8", "--auto-augment", policy],         # no --data-file
                    ["--augment", "resized-crop", "--data-file", "x.pt", "--auto-augment", policy]):
            with pytest.raises(SystemExit):
                M.parse_args(bad)
    for bad in (["--ra-num-ops", "5"], ["--ra-num-ops", "0"], ["--ra-magnitude", "31"], ["--ra-magnitude", "-1"]):
        with pytest.raises(SystemExit):
            M.parse_args(ok + ["--auto-augment", "ra"] + bad)


def test_main_names_the_resized_crop_path_as_not_built(capsys):
    with pytest.raises(SystemExit):
        M.parse_args(["--augment", "resized-crop", "--data-file", "x.pt", "--auto-augment", "ra"])
    assert "resized-crop is not built" in capsys.readouterr().err
