"""MixUp / CutMix without a GPU: the draw (nbdt.data.draw_mix) and the host-side argument checks of nbdt_mix_batch."""
import ctypes

import numpy as np
import pytest

from nbdt import _C
from nbdt import data as D


def test_no_alphas_no_mixing():
    assert D.draw_mix(0, 0, 0, 32, 32) is None
    assert D.draw_mix(3, 1, 2, 32, 32, 0.0, 0.0) is None
    with pytest.raises(ValueError):
        D.draw_mix(0, 0, 0, 32, 32, -1.0, 0.0)


def test_draw_is_a_pure_function_of_its_arguments():
    a = [D.draw_mix(7, e, s, 32, 48, 0.2, 1.0) for e in range(3) for s in range(20)]
    np.random.default_rng(0).random(1000)               # nobody else's generator state matters
    np.random.seed(123)
    b = [D.draw_mix(7, e, s, 32, 48, 0.2, 1.0) for e in range(3) for s in range(20)]
    assert a == b
    assert len({d["lam"] for d in a}) == len(a)         # every (epoch, step) draws its own
    assert D.draw_mix(8, 0, 0, 32, 48, 0.2, 1.0) != a[0]


@pytest.mark.parametrize("H,W", [(32, 32), (8, 8), (32, 20), (224, 224), (1, 7)])
def test_cutmix_boxes_stay_inside_and_lam_t_matches_the_area(H, W):
    empty = 0
    for step in range(300):
        d = D.draw_mix(1, 0, step, H, W, 0.0, 1.0)
        assert d["mode"] == "cutmix" and 0.0 <= d["lam"] <= 1.0
        y1, y2, x1, x2 = d["box"]
        assert 0 <= y1 <= y2 <= H and 0 <= x1 <= x2 <= W
        assert y2 - y1 <= 2 * int(0.5 * np.sqrt(1.0 - d["lam"]) * H) and x2 - x1 <= 2 * int(0.5 * np.sqrt(1.0 - d["lam"]) * W)
        assert d["lam_t"] == 1.0 - (y2 - y1) * (x2 - x1) / float(H * W)
        empty += (y2 - y1) * (x2 - x1) == 0
    assert empty < 300 or H * W < 16


def test_mixup_has_no_box_and_keeps_lam():
    for step in range(50):
        d = D.draw_mix(1, 2, step, 32, 32, 0.4, 0.0)
        assert d["mode"] == "mixup" and d["box"] == (0, 0, 0, 0) and d["lam_t"] == d["lam"] and 0.0 <= d["lam"] <= 1.0


def test_mode_selection():
    assert {D.draw_mix(0, 0, s, 32, 32, 0.2, 0.0)["mode"] for s in range(200)} == {"mixup"}
    assert {D.draw_mix(0, 0, s, 32, 32, 0.0, 0.2)["mode"] for s in range(200)} == {"cutmix"}
    assert {D.draw_mix(0, 0, s, 32, 32, 0.2, 1.0)["mode"] for s in range(200)} == {"mixup", "cutmix"}


@pytest.mark.parametrize("alpha", [1.0, 0.2])
def test_lam_is_beta_distributed_around_a_half(alpha):
    """Beta(a, a) has mean 1/2 and variance 1/(4(2a+1)): the standard error of the mean of 2000 draws is 0.0065 (a = 1)
    and 0.0094 (a = 0.2), so 0.05 is more than five of them."""
    lam = np.array([D.draw_mix(5, 0, s, 32, 32, alpha, 0.0)["lam"] for s in range(2000)])
    assert abs(lam.mean() - 0.5) < 0.05
    assert lam.min() >= 0.0 and lam.max() <= 1.0
    if alpha < 1:           # Beta(0.2, 0.2) piles up at the ends, Beta(1, 1) is flat
        assert (np.abs(lam - 0.5) > 0.4).mean() > 0.4


def _call(**over):
    a = dict(x=ctypes.c_void_p(4096), y=ctypes.c_void_p(64), B=4, H=8, W=8, lam=1.0, oml=0.0, y1=0, y2=0, x1=0, x2=0,
             lam_t=1.0, oml_t=0.0, out=ctypes.c_void_p(1 << 20), tgt=ctypes.c_void_p(1 << 21), C=10)
    a.update(over)
    lib = _C.lib()
    rc = lib.nbdt_mix_batch(a["x"], a["y"], a["B"], a["H"], a["W"], a["lam"], a["oml"], a["y1"], a["y2"], a["x1"], a["x2"],
                            a["lam_t"], a["oml_t"], a["out"], a["tgt"], a["C"], None)
    return rc, lib.nbdt_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(x=None), "null"), (dict(tgt=None), "null"), (dict(B=0), "empty batch"), (dict(H=0), "image sides"),
    (dict(W=5000), "image sides"), (dict(C=0), "classes"), (dict(y1=3, y2=2), "box"), (dict(y2=9), "box"),
    (dict(x1=-1, x2=4), "box"), (dict(x2=9), "box"),
    (dict(out=ctypes.c_void_p(4096)), "overlap"), (dict(out=ctypes.c_void_p(4096 + 4 * 8 * 8 * 3 * 4 - 4)), "overlap"),
    (dict(tgt=ctypes.c_void_p(4096 + 64)), "tgt must not overlap"), (dict(tgt=ctypes.c_void_p((1 << 20) + 8)), "tgt must not overlap"),
    (dict(lam=0.5, oml=0.5, y2=4, x2=4), "CutMix"),
])
def test_entry_rejects_bad_arguments_before_any_hip_call(over, word):
    """Every refusal is decided on the host from the arguments alone (the pointers here are never dereferenced)."""
    rc, msg = _call(**over)
    assert rc == -1 and word in msg, (rc, msg)
