"""Wall time per call of the segmentation entries (csrc/rules_pixel.h, one lane per pixel) against the only alternative
the row kernels offer: coerce [N,C,H,W] -> [N*H*W, C], the row kernel, uncoerce -- the permutes included.

  python scratch/seg_rules.py [OUT.txt] [SHAPES]        (needs an MI355X; profiles/seg_rules.txt is its output)

Shapes: 8 x 19 x 512 x 1024 (Cityscapes-like, on a synthetic 19-class binary hierarchy: the reference has no Cityscapes
wnid list) and 8 x 150 x 512 x 512 (ADE20K, tests/golden/seg_hierarchies), fp32 and bf16 logits.  SHAPES = "city", "ade"
or "city,ade" (default).  Per call: a host clock around `iters` calls that end in a device synchronise, after a warm-up;
windows of the two paths alternate, the median of 5 and [min, max] are printed.  Bytes are counted from the shapes -- what
the algorithm must move: read z (and gP / y), write P / gz / the labels -- so GB/s and the share of the 8.0 TB/s HBM peak
are algorithmic, not counters.  The two paths are compared on the timed tensors before they are timed."""
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nbdt_path  # noqa: E402

nbdt_path.add()
import _tree_shapes as S  # noqa: E402
from nbdt import _C  # noqa: E402
from nbdt.tree import Tree  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12
IGNORE = 255


def coerce(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def uncoerce(rows, shape):
    N, _, H, W = shape
    return rows.view(N, H, W, rows.shape[1]).permute(0, 3, 1, 2).contiguous()


def entries(handle, z, gP, y):
    """name -> (pixel call, coerced call, algorithmic bytes)."""
    N, C, H, W = z.shape
    px, e = N * H * W, z.element_size()
    yr = y.view(-1)

    def rows_loss():
        loss, g = _C.soft_tree_loss(handle, coerce(z), yr, 1.0, 10.0)
        return loss, uncoerce(g, z.shape)

    def rows_hard():
        pred, onehot, _ = _C.hard_forward(handle, coerce(z))
        return pred.view(N, H, W), uncoerce(onehot, z.shape)

    return {
        "soft_forward": (lambda: _C.seg_soft_forward(handle, z),
                         lambda: uncoerce(_C.soft_forward(handle, coerce(z)), z.shape), px * C * (e + 4)),
        "soft_backward": (lambda: _C.seg_soft_backward(handle, z, gP),
                          lambda: uncoerce(_C.soft_backward(handle, coerce(z), coerce(gP)), z.shape), px * C * (e + 8)),
        "soft_tree_loss": (lambda: _C.seg_soft_tree_loss(handle, z, y, IGNORE, 1.0, 10.0), rows_loss,
                           px * (C * (e + 4) + 8)),
        "hard_forward": (lambda: _C.seg_hard_forward(handle, z), rows_hard, px * (C * (e + 4) + 8)),
        "hard_predict": (lambda: _C.seg_hard_forward(handle, z, want_onehot=False)[0],
                         lambda: _C.hard_forward(handle, coerce(z), want_onehot=False)[0].view(N, H, W), px * (C * e + 8)),
    }


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def time_pair(a, b):
    """Median, min, max of 5 alternating windows of each, in us per call."""
    iters = []
    for fn in (a, b):
        for _ in range(2):
            fn()
        once = window(fn, 1)
        iters.append(max(5, min(500, int(0.25e6 / max(once, 1.0)))))
    wa, wb = [], []
    for _ in range(5):
        wa.append(window(a, iters[0]))
        wb.append(window(b, iters[1]))
    wa.sort()
    wb.sort()
    return (wa[2], wa[0], wa[-1], iters[0]), (wb[2], wb[0], wb[-1], iters[1])


def agree(name, p, r):
    """The two paths on the timed tensors: integers equal, floats by their largest absolute difference."""
    p = p if isinstance(p, tuple) else (p,)
    r = r if isinstance(r, tuple) else (r,)
    out = []
    for a, b in zip(p, r):
        if a is None:
            continue
        if a.dtype == torch.int64:
            out.append("labels equal" if torch.equal(a, b) else f"LABELS DIFFER at {(a != b).sum().item()} pixels")
        else:
            out.append(f"max |diff| {(a.float() - b.float()).abs().max().item():.2e}")
    return ", ".join(out)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    which = (sys.argv[2] if len(sys.argv) > 2 else "city,ade").split(",")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    assert torch.cuda.is_available(), "needs an MI355X"
    tmp = tempfile.mkdtemp()
    pg, pw, leaves = S.kary(tmp, 19, 2)
    gold = os.path.join(ROOT, "tests", "golden", "seg_hierarchies")
    shapes = {"city": ("kary19_2 (Cityscapes-like)", Tree(None, path_graph=pg, path_wnids=pw, classes=leaves), (8, 19, 512, 1024)),
              "ade": ("ADE20K induced-HRNet-w48",
                      Tree("ADE20K", path_graph=os.path.join(gold, "ADE20K-graph-induced-HRNet-w48.json"),
                           path_wnids=os.path.join(gold, "ADE20K-wnids.txt")), (8, 150, 512, 512))}
    props = torch.cuda.get_device_properties(0)
    say(f"segmentation rules, pixel kernels against coerce -> row kernel -> uncoerce, {props.name} "
        f"({props.multi_processor_count} CUs)")
    say("us = median of 5 alternating windows [min, max] x calls per window; GB/s and % of the 8.0 TB/s HBM peak by "
        "algorithmic bytes")
    for key in which:
        name, tree, shape = shapes[key]
        flat = tree.flat
        handle = tree.device_handle(0)
        fan = int((flat.node_off[1:] - flat.node_off[:-1]).max())
        say()
        say(f"{name}: {' x '.join(map(str, shape))}; C {flat.num_classes}, N {flat.num_inodes}, R {flat.num_slots}, "
            f"L {len(flat.slot_cls)}, F {fan}; LDS per wave {(flat.num_slots + fan) * 256 / 1024:.1f} KB")
        g = torch.Generator().manual_seed(7)
        z32 = 3.0 * torch.randn(shape, generator=g)
        gP = torch.randn(shape, generator=g).to(DEV)
        y = torch.randint(0, shape[1], (shape[0], shape[2], shape[3]), generator=g).to(DEV)
        for dtype in (torch.float32, torch.bfloat16):
            z = z32.to(DEV).to(dtype)
            for entry, (pixel, rows, nbytes) in entries(handle, z, gP, y).items():
                p = pixel()
                path = _C.last_rules_path()
                same = agree(entry, p, rows())
                del p
                tp, tr = time_pair(pixel, rows)
                for label, (med, lo, hi, iters), pth in (("pixel", tp, path), ("coerced", tr, "rows")):
                    say(f"  {str(dtype)[6:]:8s} {entry:15s} {label:8s} {pth:6s} {med:10.1f} us [{lo:.1f}, {hi:.1f}] x{iters:<4d}"
                        f" {nbytes / 1e9:6.3f} GB {nbytes / med / 1e3:8.1f} GB/s {100 * nbytes / (med * 1e-6) / HBM_PEAK:5.1f} %")
                say(f"  {'':8s} {entry:15s} pixel is {tr[0] / tp[0]:.2f}x the coerced path "
                    f"(windows do{'' if tp[2] < tr[1] else ' NOT'} separate); {same}")
            del z
        del gP, y
        torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
