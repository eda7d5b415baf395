"""Wall time per call of the segmentation evaluation launch (csrc/seg_stats.h) against what a user composes from the
entries that were there before it.

  python scratch/seg_stats.py [OUT.txt] [SHAPES]        (needs an MI355X; profiles/seg_stats.txt is its output)

Shapes and hierarchies as scratch/seg_rules.py: 8 x 19 x 512 x 1024 (Cityscapes-like, synthetic 19-class binary
hierarchy) and 8 x 150 x 512 x 512 (ADE20K), fp32 and bf16 logits.  Labels: a blocky map (constant 16 x 16 tiles, 10 % of
the tiles ignored) -- what real label maps give the key aggregation -- and, as the adversarial case, uniformly random
labels with 10 % of the pixels ignored.  Logits: noise plus 4.0 on the label's class at 80 % of the tiles, so the three
predictions are blocky too where the labels are.

Timed, in the same process and in alternating windows (median of 5, [min, max]):
  fused      nbdt_seg_stats_accumulate with totals + the three confusion matrices
  fused+     the same plus node_counts and first_error_depth
  composed   seg_hard_forward(want_onehot=False) + seg_soft_forward + two argmax(1) + masking + three bincounts
  rules      the first two calls of `composed` alone: hard predict + soft forward
The fused counters are compared with the composed ones on the timed tensors before anything is timed."""
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
from nbdt import _C, ops  # noqa: E402
from nbdt.tree import Tree  # noqa: E402

DEV = "cuda:0"
IGNORE = 255
TILE = 16


def labels(kind, shape, gen):
    N, C, H, W = shape
    if kind == "blocky":
        tiles = torch.randint(0, C, (N, H // TILE, W // TILE), generator=gen)
        tiles[torch.rand(tiles.shape, generator=gen) < 0.1] = IGNORE
        return tiles.repeat_interleave(TILE, 1).repeat_interleave(TILE, 2).contiguous()
    y = torch.randint(0, C, (N, H, W), generator=gen)
    y[torch.rand(y.shape, generator=gen) < 0.1] = IGNORE
    return y


def logits(y, shape, gen):
    """Noise, plus 4.0 on the label's class where a coarse coin says so (per 16 x 16 tile)."""
    N, C, H, W = shape
    z = torch.randn(shape, generator=gen)
    keep = (torch.rand((N, H // TILE, W // TILE), generator=gen) < 0.8).repeat_interleave(TILE, 1).repeat_interleave(TILE, 2)
    cls = torch.where(y == IGNORE, torch.zeros_like(y), y)
    z.scatter_add_(1, cls.unsqueeze(1), (4.0 * keep).unsqueeze(1).to(z.dtype))
    return z


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def time_all(fns):
    """name -> (median, min, max, calls per window) of 5 alternating windows, in us per call."""
    iters = {}
    for name, fn in fns.items():
        for _ in range(2):
            fn()
        iters[name] = max(3, min(200, int(0.1e6 / max(window(fn, 1), 1.0))))
    seen = {name: [] for name in fns}
    for _ in range(5):
        for name, fn in fns.items():
            seen[name].append(window(fn, iters[name]))
    return {name: (sorted(w)[2], min(w), max(w), iters[name]) for name, w in seen.items()}


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
    say(f"segmentation evaluation: the fused launch against the composition of the existing entries, {props.name} "
        f"({props.multi_processor_count} CUs)")
    say("us = median of 5 alternating windows [min, max] x calls per window")
    for key in which:
        name, tree, shape = shapes[key]
        flat = tree.flat
        handle = tree.device_handle(0)
        C = flat.num_classes
        sizes = ops.tree_stats_sizes(handle)
        say()
        say(f"{name}: {' x '.join(map(str, shape))}; C {C}, N {flat.num_inodes}, R {flat.num_slots}; LDS per block "
            f"{_C.seg_stats_lds_bytes(flat) / 1024:.1f} KB")
        for kind in ("blocky", "random"):
            gen = torch.Generator().manual_seed(7)
            y_host = labels(kind, shape, gen)
            z32 = logits(y_host, shape, gen)
            y = y_host.to(DEV)
            for dtype in (torch.float32, torch.bfloat16):
                z = z32.to(DEV).to(dtype)
                small = {f: torch.zeros(sizes[f], dtype=torch.int64, device=DEV)
                         for f in ("totals", "confusion_net", "confusion_hard", "confusion_soft")}
                full = {f: torch.zeros(sizes[f], dtype=torch.int64, device=DEV) for f in ops.SEG_STATS_FIELDS}

                def rules():
                    return _C.seg_hard_forward(handle, z, want_onehot=False)[0], _C.seg_soft_forward(handle, z)

                def composed():
                    hard, P = rules()
                    valid = y != IGNORE
                    row = y[valid] * C
                    return [torch.bincount(row + p[valid], minlength=C * C) for p in (z.argmax(1), hard, P.argmax(1))]

                fns = {"fused": lambda: ops.seg_stats_accumulate(handle, z, y, IGNORE, small),
                       "fused+": lambda: ops.seg_stats_accumulate(handle, z, y, IGNORE, full),
                       "composed": composed, "rules": rules}
                fns["fused"]()
                assert _C.last_rules_path() == "pixel"
                ref = composed()
                agree = all(torch.equal(small["confusion_" + k], r) for k, r in zip(("net", "hard", "soft"), ref))
                del ref
                t = time_all(fns)
                for label in fns:
                    med, lo, hi, iters = t[label]
                    say(f"  {kind:7s} {str(dtype)[6:]:8s} {label:9s} {med:10.1f} us [{lo:.1f}, {hi:.1f}] x{iters}")
                apart = t["fused"][2] < t["rules"][1]
                say(f"  {kind:7s} {str(dtype)[6:]:8s} fused is {t['rules'][0] / t['fused'][0]:.2f}x `rules` (windows do"
                    f"{'' if apart else ' NOT'} separate) and {t['composed'][0] / t['fused'][0]:.2f}x `composed`; fused+ costs "
                    f"{t['fused+'][0] / t['fused'][0]:.2f}x fused; counters {'equal' if agree else 'DIFFER from'} the composition")
                del z, small, full
                torch.cuda.empty_cache()
            del y
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
