"""Writes tests/golden/policy_chain_pil.npz: what Pillow computes for the 15 operations of the policy chains (RandAugment,
AutoAugment) under their magnitude tables, and for all 225 ordered pairs of them applied as two successive Pillow calls, on
two small seeded uint8 images.  nbdt.data.chain_reference and nbdt_policy_chain_batch must reproduce these bytes.  Needs
Pillow (and numpy to write the file); the Pillow version is recorded in the file.

    python tests/golden/make_policy_chain_golden.py

The magnitudes are formed in double exactly as include/nbdt_hip.h states them (hi * b / (n - 1) over n = 31 bins for
RandAugment, n = 10 for AutoAugment); the calls are the ones torchvision makes on PIL images, with fill 0 and
nearest-neighbour geometry.
"""
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageOps

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "policy_chain_pil.npz")
OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
       "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize", "Invert")
LOW_BINS = {31: (0, 1, 9, 15, 30), 10: (0, 5, 9)}       # the bins kept for the larger fixture
PAIR_BIN = {31: 9, 10: 7}                                # all pairs: first op at sign 0, second at sign 1


def pil_image(img):
    return Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)), "RGB")


def pil_op(im, name, b, sign, n):
    """One operation by Pillow on a PIL image at bin b of n; sign: 0 (+) or 1 (-)."""
    s = -1.0 if sign else 1.0
    W, H = im.size
    if name == "Identity":
        return im.copy()
    if name == "ShearX":
        return im.transform(im.size, Image.AFFINE, [1, s * 0.3 * b / (n - 1), 0, 0, 1, 0], Image.NEAREST, fillcolor=0)
    if name == "ShearY":
        return im.transform(im.size, Image.AFFINE, [1, 0, 0, s * 0.3 * b / (n - 1), 1, 0], Image.NEAREST, fillcolor=0)
    if name == "TranslateX":
        t = int(s) * int(150.0 / 331.0 * W * b / (n - 1))
        return im.transform(im.size, Image.AFFINE, [1, 0, -t, 0, 1, 0], Image.NEAREST, fillcolor=0)
    if name == "TranslateY":
        t = int(s) * int(150.0 / 331.0 * H * b / (n - 1))
        return im.transform(im.size, Image.AFFINE, [1, 0, 0, 0, 1, -t], Image.NEAREST, fillcolor=0)
    if name == "Rotate":
        return im.rotate(s * 30.0 * b / (n - 1), Image.NEAREST, fillcolor=0)
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        return getattr(ImageEnhance, name)(im).enhance(1 + s * 0.9 * b / (n - 1))
    if name == "Posterize":
        return ImageOps.posterize(im, 8 - round(b / ((n - 1) / 4)))
    if name == "Solarize":
        return ImageOps.solarize(im, 255 - 255 * b / (n - 1))
    if name == "AutoContrast":
        return ImageOps.autocontrast(im)
    if name == "Equalize":
        return ImageOps.equalize(im)
    if name == "Invert":
        return ImageOps.invert(im)
    raise KeyError(name)


def pil_chain(img, chain, n):
    """The operations chain = [(name, bin, sign), ...] as successive Pillow calls on a uint8 [3,H,W] array."""
    im = pil_image(img)
    for name, b, sign in chain:
        im = pil_op(im, name, b, sign, n)
    return np.asarray(im).transpose(2, 0, 1)


def fixtures():
    """A random 9 x 7 image (every bin of every op is kept for it) and a low-contrast 18 x 16 image (40..199: AutoContrast
    and, with more than 255 pixels a channel, Equalize have work to do)."""
    rng = np.random.default_rng(20261020)
    y, x = np.mgrid[0:18, 0:16]
    ramp = np.stack([40 + 6 * x + 4 * y, 199 - 7 * x - 2 * y, 60 + 7 * y + (x % 4)])
    low = np.clip(ramp + rng.integers(-6, 7, ramp.shape), 40, 199).astype(np.uint8)
    low[:, 0, 0], low[:, 0, 1] = 40, 199
    return {"random": rng.integers(0, 256, (3, 9, 7), dtype=np.uint8), "low": low}


def main():
    blob = {"pil_version": np.array(PIL.__version__), "ops": np.array(OPS)}
    for name, img in fixtures().items():
        blob[f"img_{name}"] = img
        for n in (31, 10):
            bins = tuple(range(n)) if name == "random" else LOW_BINS[n]
            blob[f"bins_{name}_{n}"] = np.array(bins)
            blob[f"single_{name}_{n}"] = np.stack([np.stack([np.stack([pil_chain(img, [(op, b, sg)], n) for sg in (0, 1)])
                                                             for b in bins]) for op in OPS])      # [15, bins, 2, 3, H, W]
            blob[f"pairs_{name}_{n}"] = np.stack([np.stack([pil_chain(img, [(p, PAIR_BIN[n], 0), (q, PAIR_BIN[n], 1)], n)
                                                            for q in OPS]) for p in OPS])           # [15, 15, 3, H, W]
    np.savez_compressed(OUT, **blob)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
