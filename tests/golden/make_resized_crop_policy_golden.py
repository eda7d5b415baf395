"""Writes tests/golden/resized_crop_policy_pil.npz: what Pillow computes for ``crop -> resize(BILINEAR) -> FLIP_LEFT_RIGHT ->
the operations of a policy chain as successive Pillow calls`` on two seeded uint8 images, one resized to 22 x 22 and one to
144 x 144 (3 * 144 * 144 = 62208 bytes: above the 49152 the padded-crop kernels take).
nbdt.data.resized_crop_policy_reference and nbdt_resized_crop_policy_batch must reproduce these bytes.  Needs Pillow (and
numpy to write the file); the Pillow version is recorded in the file.

    python tests/golden/make_resized_crop_policy_golden.py

The operations and their magnitudes are make_policy_chain_golden.py's ``pil_op`` (hi * b / (n - 1) in double over n = 31
bins for RandAugment, n = 10 for AutoAugment), applied to the S x S crop: translations are (150/331) * S, Rotate turns
about the crop's centre.
"""
import importlib.util
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resized_crop_policy_pil.npz")
_spec = importlib.util.spec_from_file_location("make_policy_chain_golden", os.path.join(HERE, "make_policy_chain_golden.py"))
_chain = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_chain)
OPS, pil_image, pil_op = _chain.OPS, _chain.pil_image, _chain.pil_op

BINS = {31: (0, 15, 30), 10: (0, 5, 9)}                  # first, middle, last
# name: (H, W of the source, side S of the crop, box (top, left, h, w)); both are flipped
CASES = {"small": (40, 36, 22, (3, 2, 33, 30)), "large": (160, 176, 144, (4, 9, 150, 161))}
LARGE_OPS = ("Rotate", "TranslateX", "ShearY", "Contrast", "Equalize", "Sharpness")      # arithmetic that scales with the side
LARGE_CHAINS = ((("Rotate", 1), ("Equalize", 0), ("Color", 0)),                           # (op, sign); every op at one bin
                (("ShearX", 0), ("Contrast", 1), ("Sharpness", 0), ("AutoContrast", 0)))
LARGE_CHAIN_BIN = {31: 20, 10: 7}


def fixture(H, W, seed, patch=None):
    """A smooth ramp per channel (along x, along y, along the diagonal; 40..200) plus seeded noise, so that AutoContrast and
    Equalize have work to do.  patch = (top, left, h, w): the noise is confined to that rectangle -- the 144 x 144 results
    then compress to some 6 KB each, and all 72 of them fit a file that has to stay below 564410 bytes."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ramp = np.stack([40 + 150 * x / W, 200 - 150 * y / H, 60 + 100 * (x + y) / (H + W)])
    noise = rng.integers(-10, 11, ramp.shape)
    if patch is not None:
        t, l, h, w = patch
        keep = np.zeros(ramp.shape, dtype=bool)
        keep[:, t:t + h, l:l + w] = True
        noise = np.where(keep, noise, 0)
    return np.clip(np.rint(ramp) + noise, 30, 220).astype(np.uint8)


def resized_crop(img, box, S):
    """crop -> resize(BILINEAR) -> FLIP_LEFT_RIGHT of a uint8 [3,H,W] array, as a PIL image."""
    top, left, h, w = box
    im = pil_image(img).crop((left, top, left + w, top + h)).resize((S, S), Image.BILINEAR)
    return im.transpose(Image.FLIP_LEFT_RIGHT)


def apply(im, chain, n):
    for name, b, sign in chain:
        im = pil_op(im, name, b, sign, n)
    return np.asarray(im).transpose(2, 0, 1)


def main():
    blob = {"pil_version": np.array(PIL.__version__), "ops": np.array(OPS), "large_ops": np.array(LARGE_OPS)}
    for name, (H, W, S, box) in CASES.items():
        img = fixture(H, W, 20261020 + S, patch=(40, 60, 24, 32) if name == "large" else None)
        blob[f"img_{name}"], blob[f"box_{name}"], blob[f"side_{name}"] = img, np.array(box), np.array(S)
        base = resized_crop(img, box, S)
        blob[f"plain_{name}"] = np.asarray(base).transpose(2, 0, 1)
        ops = OPS if name == "small" else LARGE_OPS
        for n in (31, 10):
            blob[f"bins_{n}"] = np.array(BINS[n])
            blob[f"single_{name}_{n}"] = np.stack([np.stack([np.stack([apply(base, [(op, b, sg)], n) for sg in (0, 1)])
                                                             for b in BINS[n]]) for op in ops])      # [ops, 3, 2, 3, S, S]
            if name == "large":
                for k, chain in enumerate(LARGE_CHAINS):
                    blob[f"chain{k}_{n}"] = apply(base, [(op, LARGE_CHAIN_BIN[n], sg) for op, sg in chain], n)
    np.savez_compressed(OUT, **blob)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
