"""Writes tests/golden/policy_pil.npz: what Pillow computes for each of TrivialAugmentWide's 14 operations on three small
seeded uint8 images.  nbdt.data.policy_reference and nbdt_policy_batch must reproduce these bytes.  Needs Pillow (and numpy
to write the file); the Pillow version is recorded in the file.

    python tests/golden/make_policy_golden.py

The magnitudes are formed in double exactly as include/nbdt_hip.h states them (TrivialAugmentWide's ranges over 31 bins);
the calls are the ones torchvision makes on PIL images, with fill 0 and nearest-neighbour geometry.
"""
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageOps

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "policy_pil.npz")
OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
       "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
BINS = (0, 1, 7, 15, 20, 29, 30)


def pil_image(img):
    return Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)), "RGB")


def pil_op(img, name, b, sign):
    """One operation by Pillow on a uint8 [3,H,W] array; sign: 0 (+) or 1 (-)."""
    im = pil_image(img)
    s = -1.0 if sign else 1.0
    m = s * 0.99 * b / 30
    if name == "Identity":
        out = im.copy()
    elif name == "ShearX":
        out = im.transform(im.size, Image.AFFINE, [1, m, 0, 0, 1, 0], Image.NEAREST, fillcolor=0)
    elif name == "ShearY":
        out = im.transform(im.size, Image.AFFINE, [1, 0, 0, m, 1, 0], Image.NEAREST, fillcolor=0)
    elif name == "TranslateX":
        out = im.transform(im.size, Image.AFFINE, [1, 0, -int(s) * int(32 * b / 30), 0, 1, 0], Image.NEAREST, fillcolor=0)
    elif name == "TranslateY":
        out = im.transform(im.size, Image.AFFINE, [1, 0, 0, 0, 1, -int(s) * int(32 * b / 30)], Image.NEAREST, fillcolor=0)
    elif name == "Rotate":
        out = im.rotate(s * 135 * b / 30, Image.NEAREST, fillcolor=0)
    elif name in ("Brightness", "Color", "Contrast", "Sharpness"):
        out = getattr(ImageEnhance, name)(im).enhance(1 + m)
    elif name == "Posterize":
        out = ImageOps.posterize(im, 8 - round(b / 5))
    elif name == "Solarize":
        out = ImageOps.solarize(im, 255 - 255 * b / 30)
    elif name == "AutoContrast":
        out = ImageOps.autocontrast(im)
    else:
        out = ImageOps.equalize(im)
    return np.asarray(out).transpose(2, 0, 1)


def fixtures():
    """A random 32 x 32 image; a low-contrast 24 x 40 image (40..199: AutoContrast and Equalize have work to do; a smooth
    ramp plus a few levels of noise, so that the file stays small); a constant 16 x 16 image (hi <= lo, one histogram bin)."""
    rng = np.random.default_rng(20241019)
    y, x = np.mgrid[0:24, 0:40]
    ramp = np.stack([40 + 3 * x + 2 * y, 199 - 4 * x - (y // 2), 60 + 5 * y + (x % 7)])
    low = np.clip(ramp + rng.integers(-6, 7, ramp.shape), 40, 199).astype(np.uint8)
    low[0, 0, 0], low[0, 0, 1], low[1, 0, 0], low[1, 0, 1], low[2, 0, 0], low[2, 0, 1] = 40, 199, 40, 199, 40, 199
    const = np.empty((3, 16, 16), dtype=np.uint8)
    const[0], const[1], const[2] = 7, 128, 255
    return {"random": rng.integers(0, 256, (3, 32, 32), dtype=np.uint8), "low": low, "const": const}


def main():
    blob = {"pil_version": np.array(PIL.__version__), "ops": np.array(OPS), "bins": np.array(BINS)}
    for name, img in fixtures().items():
        blob[f"img_{name}"] = img
        blob[f"out_{name}"] = np.stack([np.stack([np.stack([pil_op(img, op, b, sg) for sg in (0, 1)]) for b in BINS])
                                        for op in OPS])           # [14, 7, 2, 3, H, W]
    np.savez_compressed(OUT, **blob)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
