"""Host side of the resized-crop datasets (no GPU): nbdt.data.resample_reference against PIL's bytes (committed goldens,
and PIL itself when it imports), the draw of nbdt_resized_crop_batch as nbdt.data.draw_resized_crop_params restates it,
the argument checks of the C entry, which run before any HIP call, and main.py's --augment resized-crop."""
import ctypes
import importlib.util
import math
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

GOLDEN = os.path.join(nbdt_path.ROOT, "tests", "golden", "resized_crop_pil.npz")


def test_resized_crop_stats_are_the_reference_transforms():
    assert D.RESIZED_CROP_STATS == {"Imagenet1000": {"mean": (0.485, 0.456, 0.406), "std": (0.229, 0.224, 0.225),
                                                     "size": 224, "resize": 256, "scale": (0.08, 1.0),
                                                     "ratio": (3 / 4, 4 / 3)}}
    assert sorted(D.DATASET_STATS) == ["CIFAR10", "CIFAR100", "TinyImagenet200"]


# ------------------------------------------------------------------------------------------------------------ pixels

def test_resample_reference_equals_the_pil_goldens_byte_for_byte():
    g = np.load(GOLDEN)
    assert str(g["pil_version"])          # the fixture says which PIL made it
    checked = 0
    for name in ("a", "b"):
        imgs, boxes = g[f"img_{name}"], g[f"boxes_{name}"]
        for si, size in enumerate(g["sizes"]):
            want = g[f"out_{name}_{si}"]
            assert want.shape == (len(imgs), len(boxes), 3, size[0], size[1])
            for i, img in enumerate(imgs):
                for k, box in enumerate(boxes):
                    got = D.resample_reference(img, box, size)
                    assert got.dtype == np.uint8 and np.array_equal(got, want[i, k]), (name, i, box.tolist(), size.tolist())
                    checked += 1
        for u, i in enumerate(g[f"big_{name}_img"]):
            for k, box in enumerate(g[f"big_{name}_boxes"]):
                assert np.array_equal(D.resample_reference(imgs[i], box, (224, 224)), g[f"big_{name}_out"][u, k])
                checked += 1
    assert checked == (4 + 2) * 12 * 4 + 3


def test_resample_reference_window_is_resize_then_center_crop():
    """The evaluation transform: box = the whole image, resized so that the short side is 40, the central 32 x 32 written.
    The window of resample_reference equals PIL's resize + crop, and equals slicing its own full result."""
    g = np.load(GOLDEN)
    resize, size = int(g["eval_resize"]), int(g["eval_size"])
    for name in ("a", "b"):
        for i, img in enumerate(g[f"img_{name}"]):
            H, W = img.shape[1:]
            rs, (top, left) = D.resize_center_crop_geometry(H, W, size, resize)
            got = D.resample_reference(img, (0, 0, H, W), rs, window=(top, left, size, size))
            assert np.array_equal(got, g[f"eval_{name}"][i]), (name, i)
            full = D.resample_reference(img, (0, 0, H, W), rs)
            assert np.array_equal(got, full[:, top:top + size, left:left + size])
    assert D.resize_center_crop_geometry(96, 80, 32, 40) == ((48, 40), (8, 4))
    assert D.resize_center_crop_geometry(256, 256, 224, 256) == ((256, 256), (16, 16))
    assert D.resize_center_crop_geometry(375, 500, 224, 256) == ((256, 341), (16, 58))     # int(256 * 500 / 375), round(58.5)


def test_resample_reference_equals_pil_live():
    """A seeded sweep of random (image size, box, output size) against the installed PIL, byte for byte."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for it in range(300):
        H, W = (int(v) for v in rng.integers(1, 90, 2))
        if it % 10 == 0:
            H, W = int(rng.integers(200, 520)), int(rng.integers(200, 520))       # the shapes that matter: shrink to 224
        img = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        t, l = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        oh, ow = ((224, 224) if it % 10 == 0 else (int(v) for v in rng.integers(1, 70, 2)))
        pil = Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)), "RGB")
        want = np.asarray(pil.crop((l, t, l + w, t + h)).resize((ow, oh), Image.BILINEAR)).transpose(2, 0, 1)
        got = D.resample_reference(img, (t, l, h, w), (oh, ow))
        assert np.array_equal(got, want), (H, W, (t, l, h, w), (oh, ow))


def test_resample_reference_checks_its_arguments():
    img = np.zeros((3, 8, 8), dtype=np.uint8)
    for box in ((0, 0, 9, 8), (-1, 0, 4, 4), (0, 5, 4, 4), (0, 0, 0, 4)):
        with pytest.raises(ValueError, match="box"):
            D.resample_reference(img, box, (4, 4))
    with pytest.raises(ValueError, match="window"):
        D.resample_reference(img, (0, 0, 8, 8), (4, 4), window=(1, 1, 4, 4))
    with pytest.raises(ValueError, match="uint8"):
        D.resample_reference(img.astype(np.float32), (0, 0, 8, 8), (4, 4))


# -------------------------------------------------------------------------------------------------------------- draw

def test_resized_crop_draw_is_deterministic_and_a_function_of_the_index_only():
    rng = np.random.default_rng(0)
    idx = rng.integers(0, 1_281_167, size=777)
    a = D.draw_resized_crop_params(3, 5, idx, 256, 256)
    b = D.draw_resized_crop_params(3, 5, idx.copy(), 256, 256)
    assert len(a) == 5
    for u, v in zip(a, b):
        assert u.dtype == np.int64 and np.array_equal(u, v)
    # position, batch size and container do not matter: a permuted / split / repeated batch draws the same per index
    p = rng.permutation(idx.size)
    for u, v in zip(a, D.draw_resized_crop_params(3, 5, idx[p], 256, 256)):
        assert np.array_equal(u[p], v)
    for u, v in zip(a, D.draw_resized_crop_params(3, 5, torch.from_numpy(idx[:100]), 256, 256)):
        assert np.array_equal(u[:100], v)
    for u, v in zip(D.draw_resized_crop_params(3, 5, [7, 7, 7, 11], 96, 80), D.draw_resized_crop_params(3, 5, [11, 7], 96, 80)):
        assert u[0] == u[1] == u[2] == v[1] and u[3] == v[0]
    # ... and the index does
    boxes = D.draw_resized_crop_params(3, 5, np.arange(1000), 256, 256)
    assert len(set(zip(*(v.tolist() for v in boxes)))) > 900
    # the seed and the epoch are part of the key
    assert any(not np.array_equal(u, v) for u, v in zip(a, D.draw_resized_crop_params(4, 5, idx, 256, 256)))
    assert any(not np.array_equal(u, v) for u, v in zip(a, D.draw_resized_crop_params(3, 6, idx, 256, 256)))


@pytest.mark.parametrize("H,W", [(64, 64), (256, 256), (96, 80), (160, 213), (375, 500), (32, 200), (300, 40)])
def test_drawn_boxes_lie_inside_the_image_and_inside_the_scale_and_ratio_ranges(H, W):
    """Every box is inside the image.  An accepted box came from w = round(sqrt(A r)), h = round(sqrt(A / r)) with the area
    A in [0.08, 1] W H and r in [3/4, 4/3]; round() moves each side by at most 1/2, so the unrounded sides lie in
    [w - 1/2, w + 1/2] x [h - 1/2, h + 1/2]: their product interval must meet the area range and their quotient interval the
    ratio range.  That slack and no more."""
    n = 50_000
    top, left, h, w, flip, which = D.draw_resized_crop_params(1, 2, np.arange(n), H, W, return_attempt=True)
    assert top.min() >= 0 and left.min() >= 0 and h.min() >= 1 and w.min() >= 1
    assert (top + h).max() <= H and (left + w).max() <= W
    ok = which < _C.NBDT_RESIZED_CROP_ATTEMPTS
    wa, ha = w[ok].astype(np.float64), h[ok].astype(np.float64)
    assert np.all((wa + 0.5) * (ha + 0.5) >= 0.08 * W * H) and np.all((wa - 0.5) * (ha - 0.5) <= 1.0 * W * H)
    assert np.all((wa + 0.5) / (ha - 0.5) >= 3 / 4) and np.all((wa - 0.5) / (ha + 0.5) <= 4 / 3)
    # the fallback is torchvision's: the centre crop with the ratio clamped
    fb = ~ok
    if W / H < 3 / 4:
        want = (W, int(round(W / (3 / 4))))
    elif W / H > 4 / 3:
        want = (int(round(H * (4 / 3))), H)
    else:
        want = (W, H)
    assert np.all(w[fb] == want[0]) and np.all(h[fb] == want[1])
    assert np.all(top[fb] == (H - want[1]) // 2) and np.all(left[fb] == (W - want[0]) // 2)
    # positions reach both borders, the flip is balanced (binomial, 5 sigma)
    assert top[ok].min() == 0 and left[ok].min() == 0 and (top + h)[ok].max() == H and (left + w)[ok].max() == W
    assert abs(int(flip.sum()) - n / 2) < 5 * (n / 4) ** 0.5
    assert set(np.unique(flip).tolist()) == {0, 1}


def test_fallback_is_rare_on_a_square_image():
    """On a square image an attempt is rejected when the box is wider or taller than the image: before rounding, when
    A max(r, 1/r) > W H.  With A / (W H) uniform in [0.08, 1] and log r uniform in [-L, L], L = log(4/3), that has probability
    (1 - (1 - exp(-L)) / L) / 0.92 = 0.1424; rounding w, h to integers only admits more.  Ten independent attempts all fail
    with probability 0.1424^10 = 3.4e-9.

    Measured with this restatement over n = 200 000 indices of a 256 x 256 dataset (seed 0, epoch 0): first attempt
    rejected 0.1383, fallback boxes 0 (share 0.0).  Asserted: the first-attempt share is at most 0.1424 plus five binomial
    standard deviations (sqrt(p (1 - p) / n) = 0.00078), and at most one fallback box among the n: their count is
    binomial with mean n * 3.4e-9 = 7e-4, so two or more have probability 2.4e-7."""
    n = 200_000
    *_, which = D.draw_resized_crop_params(0, 0, np.arange(n), 256, 256, return_attempt=True)
    rejected_first = float(np.mean(which > 0))
    fallback = int(np.sum(which == _C.NBDT_RESIZED_CROP_ATTEMPTS))
    p = (1 - (1 - math.exp(-math.log(4 / 3))) / math.log(4 / 3)) / 0.92
    sigma = (p * (1 - p) / n) ** 0.5
    print(f"first attempt rejected {rejected_first:.4f} (law {p:.4f} +- {sigma:.5f}), fallback boxes {fallback} of {n} "
          f"(share {fallback / n:.2e})")
    assert rejected_first <= p + 5 * sigma
    assert fallback <= 1


def test_consecutive_epochs_and_seeds_draw_different_boxes():
    n = 20_000
    a = D.draw_resized_crop_params(0, 0, np.arange(n), 256, 256)
    for seed, epoch in ((0, 1), (1, 0), (0, 199)):
        b = D.draw_resized_crop_params(seed, epoch, np.arange(n), 256, 256)
        same = int(np.sum(np.all([u == v for u, v in zip(a, b)], axis=0)))
        print(f"seed {seed} epoch {epoch}: {same} of {n} boxes coincide with seed 0 epoch 0")
        assert same < n // 1000       # thousands of (top, left, h, w) combinations per sample: coincidences are rare


def test_ratio_table_and_range_checks():
    t = D.ratio_table((3 / 4, 4 / 3))
    assert t.shape == (_C.NBDT_RESIZED_CROP_RATIOS,) and t.dtype == np.float64
    assert t[0] == 3 / 4 and t[-1] == 4 / 3 and np.all(np.diff(t) > 0)
    assert abs(float(np.mean(np.log(t)))) < 1e-12          # log-uniform: symmetric about ratio 1
    for bad in (dict(scale=(0.0, 1.0)), dict(scale=(0.5, 0.4)), dict(scale=(0.5, 1.5)), dict(ratio=(2.0, 1.0)),
                dict(ratio=(0.001, 1.0))):
        with pytest.raises(ValueError):
            D.draw_resized_crop_params(0, 0, [0], 64, 64, **bad)
    with pytest.raises(ValueError):
        D.draw_resized_crop_params(0, 0, [0], 0, 64)
    with pytest.raises(ValueError):
        D.draw_resized_crop_params(0, 0, [0], 64, D.MAX_SIDE + 1)


# ------------------------------------------------------------------------------------------------------------- C entry

def _call(**over):
    """nbdt_resized_crop_batch with plausible arguments, `over` replacing some.  The pointers are never dereferenced: every
    case here is refused before the first HIP call."""
    f3 = ctypes.c_float * 3
    d2 = ctypes.c_double * 2
    a = dict(src=ctypes.c_void_p(16), dtype=_C.NBDT_U8, labels_src=ctypes.c_void_p(16), index=ctypes.c_void_p(16), B=4, N=8,
             H=64, W=64, rs_h=32, rs_w=32, win_top=0, win_left=0, out_h=32, out_w=32, flip=1, mean=f3(0.5, 0.5, 0.5),
             std=f3(0.25, 0.25, 0.25), scale=d2(0.08, 1.0), ratio=d2(0.75, 4 / 3), table=ctypes.c_void_p(16), seed=0, epoch=0,
             params_in=None, out=ctypes.c_void_p(16), labels_out=ctypes.c_void_p(16), params_out=None)
    a.update(over)
    lib = _C.lib()
    rc = lib.nbdt_resized_crop_batch(a["src"], a["dtype"], a["labels_src"], a["index"], a["B"], a["N"], a["H"], a["W"],
                                     a["rs_h"], a["rs_w"], a["win_top"], a["win_left"], a["out_h"], a["out_w"], a["flip"],
                                     a["mean"], a["std"], a["scale"], a["ratio"], a["table"], a["seed"], a["epoch"],
                                     a["params_in"], a["out"], a["labels_out"], a["params_out"], None)
    return rc, lib.nbdt_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(src=None), "null"), (dict(out=None), "null"), (dict(labels_out=None), "null"),
    (dict(dtype=_C.NBDT_F32), "uint8"), (dict(dtype=_C.NBDT_BF16), "uint8"),
    (dict(B=0), "batch"), (dict(N=0), "empty dataset"), (dict(H=0), "sides"), (dict(W=4097), "sides"),
    (dict(rs_h=0), "resized"), (dict(rs_w=4097), "resized"), (dict(out_h=0), "window"),
    (dict(win_top=1), "window"), (dict(win_left=-1), "window"), (dict(out_w=33), "window"),
    (dict(flip=2), "flip"), (dict(mean=None), "mean"), (dict(std=(ctypes.c_float * 3)(0.5, 0.0, 0.5)), "non-zero"),
    (dict(table=None), "ratio table"), (dict(scale=None), "ratio table"),
    (dict(scale=(ctypes.c_double * 2)(0.0, 1.0)), "scale"), (dict(scale=(ctypes.c_double * 2)(0.5, 1.5)), "scale"),
    (dict(ratio=(ctypes.c_double * 2)(2.0, 1.0)), "ratio"),
])
def test_entry_refuses_bad_arguments_before_any_device_work(over, word):
    rc, msg = _call(**over)
    assert rc == -1 and word in msg, (rc, msg)


def test_version_and_constants_are_in_step_with_the_header():
    assert _C.lib().nbdt_version() >= 111
    text = open(os.path.join(nbdt_path.ROOT, "include", "nbdt_hip.h")).read()
    assert f"#define NBDT_RESIZED_CROP_RATIOS {_C.NBDT_RESIZED_CROP_RATIOS}\n" in text
    assert f"#define NBDT_RESIZED_CROP_ATTEMPTS {_C.NBDT_RESIZED_CROP_ATTEMPTS}\n" in text


def test_band_plan_is_host_only_and_keeps_the_shapes_that_matter_in_lds():
    """nbdt_resized_crop_band_rows: the ImageNet shapes (source side 64 to 512, output 224, training and evaluation) are
    staged in LDS; a 4096-wide source is not; a refused geometry raises."""
    from nbdt import ops
    for side in (64, 96, 160, 256, 320, 512):
        assert ops.resized_crop_band_rows(side, side, (224, 224), (0, 0), (224, 224)) >= 1, side
        rs, win = D.resize_center_crop_geometry(side, side, 224, 256)
        assert ops.resized_crop_band_rows(side, side, rs, win, (224, 224)) >= 1, side
    assert ops.resized_crop_band_rows(256, 256, (224, 224), (0, 0), (224, 224)) >= 8
    assert ops.resized_crop_band_rows(24, 4096, (224, 224), (0, 0), (224, 224)) == 0
    with pytest.raises(_C.NBDTHipError, match="window"):
        ops.resized_crop_band_rows(64, 64, (32, 32), (1, 0), (32, 32))


# ------------------------------------------------------------------------------------------------ dataset and main.py

def test_resized_crop_dataset_refuses_the_cpu():
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    y = torch.zeros(4, dtype=torch.long)
    with pytest.raises(_C.NBDTHipError, match="no CPU fallback"):
        D.ResizedCropDataset(x, y, (0.5,) * 3, (0.5,) * 3, size=8, device="cpu")


def test_main_accepts_the_resized_crop_flag():
    p = M.build_parser()
    assert p.parse_args(["--augment", "resized-crop"]).augment == "resized-crop"
    assert p.parse_args(["--augment", "resized-crop"]).crop_size == 0
    assert p.parse_args(["--augment", "resized-crop", "--crop-size", "64"]).crop_size == 64
    assert p.parse_args([]).augment == "none"
    with pytest.raises(SystemExit):
        p.parse_args(["--augment", "torchvision"])


@pytest.mark.parametrize("dataset", ["CIFAR10", "CIFAR100", "TinyImagenet200"])
def test_main_refuses_the_resized_crop_for_the_padded_crop_datasets(dataset):
    with pytest.raises(SystemExit, match="resized-crop"):
        M.main(["--dataset", dataset, "--arch", "ResNet18", "--augment", "resized-crop", "--synthetic", "8"])


def test_main_still_refuses_the_padded_crop_for_imagenet1000_and_names_the_other_mode():
    with pytest.raises(SystemExit, match="RandomResizedCrop") as e:
        M.main(["--dataset", "Imagenet1000", "--arch", "ResNet18", "--augment", "reference", "--synthetic", "8"])
    assert "--augment resized-crop" in str(e.value)


def test_synthetic_data_for_the_resized_crop_is_uint8():
    args = M.build_parser().parse_args(["--dataset", "Imagenet1000", "--augment", "resized-crop", "--synthetic", "12",
                                        "--image-size", "16", "--batch-size", "4"])
    tx, ty, vx, vy = M.load_data(args, 1000, "cpu", raw=True)
    assert tx.dtype == torch.uint8 and tuple(tx.shape) == (12, 3, 16, 16) and vx.dtype == torch.uint8
    assert 30.0 < float(tx.float().std()) < 80.0 and 100.0 < float(tx.float().mean()) < 156.0     # greys around 128
    args = M.build_parser().parse_args(["--synthetic", "12", "--image-size", "16", "--batch-size", "4"])
    assert M.load_data(args, 10, "cpu")[0].dtype == torch.float32            # the other modes keep their float noise
