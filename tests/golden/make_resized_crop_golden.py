"""Writes tests/golden/resized_crop_pil.npz: what PIL computes for ``crop(box).resize(size, BILINEAR)`` and for
``Resize(40) -> CenterCrop(32)`` on small seeded uint8 images.  nbdt.data.resample_reference and nbdt_resized_crop_batch
must reproduce these bytes.  Needs Pillow (and numpy to write the file); the PIL version is recorded in the file.

    python tests/golden/make_resized_crop_golden.py
"""
import os

import numpy as np
import PIL
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resized_crop_pil.npz")
SIZES = [(16, 16), (32, 32), (20, 27), (7, 5)]        # (out_h, out_w): even and odd widths
EVAL_RESIZE, EVAL_SIZE = 40, 32


def boxes_for(H, W):
    """(top, left, h, w): strong and mild shrink, identity, 2x and 4x enlargement for the 32 x 32 output, one-pixel-wide
    and one-pixel-tall boxes, the full image, boxes touching each border."""
    return [(0, 0, H, W), (0, 0, 40, 44), (5, 7, 32, 32), (10, 3, 16, 16), (H - 8, W - 8, 8, 8), (3, 10, 20, 1),
            (H - 1, 0, 1, W), (0, 0, 20, 30), (H - 20, W - 30, 20, 30), (0, W - 9, H, 9), (H - 11, 0, 11, W),
            (17, 23, 29, 13)]


def gradient(H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    planes = [255.0 * x / (W - 1), 255.0 * y / (H - 1), 127.5 + 127.5 * np.sin(0.2 * x) * np.cos(0.15 * y)]
    return np.stack(planes).round().astype(np.uint8)


def pil_image(img):
    return Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)), "RGB")


def crop_resize(img, box, size):
    t, l, h, w = box
    out = pil_image(img).crop((l, t, l + w, t + h)).resize((size[1], size[0]), Image.BILINEAR)
    return np.asarray(out).transpose(2, 0, 1)


def resize_center_crop(img, resize, size):
    """torchvision's Resize(resize) + CenterCrop(size) on a PIL image"""
    H, W = img.shape[1:]
    rs_h, rs_w = (int(resize * H / W), resize) if W <= H else (resize, int(resize * W / H))
    top, left = int(round((rs_h - size) / 2.0)), int(round((rs_w - size) / 2.0))
    out = pil_image(img).resize((rs_w, rs_h), Image.BILINEAR).crop((left, top, left + size, top + size))
    return np.asarray(out).transpose(2, 0, 1)


def main():
    rng = np.random.default_rng(20240607)
    sets = {"a": np.concatenate([rng.integers(0, 256, (3, 3, 64, 64), dtype=np.uint8), gradient(64, 64)[None]]),
            "b": rng.integers(0, 256, (2, 3, 96, 80), dtype=np.uint8)}
    big = {"a": ([3], [(0, 0, 64, 64), (16, 8, 24, 30)]), "b": ([0], [(20, 10, 40, 50)])}     # 224 x 224 outputs
    blob = {"pil_version": np.array(PIL.__version__), "sizes": np.array(SIZES), "eval_resize": np.array(EVAL_RESIZE),
            "eval_size": np.array(EVAL_SIZE)}
    for name, imgs in sets.items():
        boxes = boxes_for(*imgs.shape[2:])
        blob[f"img_{name}"] = imgs
        blob[f"boxes_{name}"] = np.array(boxes)
        for si, size in enumerate(SIZES):
            blob[f"out_{name}_{si}"] = np.stack([np.stack([crop_resize(im, b, size) for b in boxes]) for im in imgs])
        which, bboxes = big[name]
        blob[f"big_{name}_img"] = np.array(which)
        blob[f"big_{name}_boxes"] = np.array(bboxes)
        blob[f"big_{name}_out"] = np.stack([np.stack([crop_resize(imgs[i], b, (224, 224)) for b in bboxes]) for i in which])
        blob[f"eval_{name}"] = np.stack([resize_center_crop(im, EVAL_RESIZE, EVAL_SIZE) for im in imgs])
    np.savez_compressed(OUT, **blob)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, PIL {PIL.__version__}")


if __name__ == "__main__":
    main()
