"""Wall time per launch of the tree-rule kernels at 256 samples, LDS form against global-row form (csrc/rules_global.h).

  python scratch/large_hierarchy_rules.py [OUT.txt]        (needs an MI355X; profiles/large_hierarchy_rules.txt is its output)

Shapes: kary(2560 | 8192 | 21841, 2) in automatic mode (global rows), the shipped ImageNet-1000 hierarchy and kary(2048, 2)
in both modes.  Per launch: a host clock around `iters` launches that end in a device synchronise, after a warm-up; the
median of 5 such windows.  Bytes per sample are counted from the shapes: `ext` is what the algorithm must move (read z,
write P / gz), `row` the floats the global form writes to and reads from its workspace row (the LDS form keeps them on chip).
GB/s = (ext + row) * samples / time for the global form, ext * samples / time for the LDS form."""
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
SAMPLES = 256
# what bounds a launch, by the path it took.  None of these comes from counters: see DESIGN.md section 23
BOUND = {"global": "hypothesis: the CU's L1 request rate (two lane-private 4-byte loads per chain element)",
         "lds": "latency of the ordered LDS chains (DESIGN.md 4.4)",
         "lds-unstaged": "hypothesis: one dependent global index load and LDS read per chain element, nothing in flight"}


def traffic(flat, entry):
    """(ext, row) floats per sample."""
    C, N, R = flat.num_classes, flat.num_inodes, flat.num_slots
    Ls = int(flat.slot_off[R])
    if entry == "soft_forward":          # zs, ss, ps written; slot gather, softmax (ss, ps), path gather read
        return 2 * C, (C + 2 * R) + (Ls + 3 * R + Ls)
    if entry == "soft_tree_loss":        # + pq, gx written twice, G and dL/ds over ss; two more gathers; three class passes
        return 2 * C + 1, (3 * C + 2 * R + 2 * C + 2 * R) + (4 * Ls + 5 * R + 7 * C)
    if entry == "hard_forward":          # zs, ss, the two per-node arrays; slot gather, argmax, the walk
        return C + 1, (C + R + 2 * N) + (Ls + R)
    if entry == "hard_tree_loss":        # zs, ss, ds, gx; slot gather, three passes over zs, path gather, gx
        return 2 * C + 1, (2 * C + 2 * R) + (2 * Ls + 4 * C)
    raise KeyError(entry)


def workspace_bytes(flat, cus):
    C, N, R = flat.num_classes, flat.num_inodes, flat.num_slots
    row = (C + 2 * R + max(2 * C, 2 * N) + 3) & ~3
    used = min(SAMPLES, cus) * row * 4                   # one row per block, one block per CU
    floats = used // 4
    alloc = (16 << 20) * 4 if floats < (16 << 20) else (floats + floats // 4) * 4      # det_rows: >= 64 MB, then 25 % headroom
    return used, row * 4, alloc


def per_launch_us(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    once = time.perf_counter() - t0
    iters = max(20, min(2000, int(0.3 / max(once, 1e-6))))
    windows = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / iters * 1e6)
    windows.sort()
    return windows[2], windows[0], windows[-1], iters


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "large_hierarchy_rules.txt")
    assert torch.cuda.is_available(), "needs an MI355X"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = [f"tree-rule kernels, {SAMPLES} samples, fp32 logits 3*randn, {torch.cuda.get_device_name(0)} ({cus} CUs)",
             "us = median of 5 windows [min, max]; ext / row = bytes per sample the algorithm moves / the global row costs", ""]
    tmp = tempfile.mkdtemp()
    cases = [("kary2560_2", ("kary", (2560, 2)), ("auto",)), ("kary8192_2", ("kary", (8192, 2)), ("auto",)),
             ("kary21841_2", ("kary", (21841, 2)), ("auto",)), ("Imagenet1000 induced-efficientnet_b7b", None, ("auto", "global")),
             ("kary2048_2", ("kary", (2048, 2)), ("auto", "global"))]
    for name, gen, modes in cases:
        t0 = time.perf_counter()
        if gen is None:
            tree = Tree("Imagenet1000", hierarchy="induced-efficientnet_b7b")
        else:
            pg, pw, leaves = S.GENERATORS[gen[0]](tmp, *gen[1])
            tree = Tree(None, path_graph=pg, path_wnids=pw, classes=leaves)
        t_tree = time.perf_counter() - t0
        t0 = time.perf_counter()
        handle = tree.device_handle(0)
        t_create = time.perf_counter() - t0
        flat = tree.flat
        C, N, R = flat.num_classes, flat.num_inodes, flat.num_slots
        ws, row, alloc = workspace_bytes(flat, cus)
        lines.append(f"{name}: C {C}, N {N}, R {R}, L {int(flat.slot_off[R])}; host: Tree {t_tree:.2f} s, nbdt_tree_create "
                     f"{t_create * 1e3:.1f} ms; global rows: {row / 1024:.0f} KB per row, {ws / 2 ** 20:.1f} MB at {SAMPLES} samples "
                     f"(workspace allocation {alloc / 2 ** 20:.0f} MB)")
        g = torch.Generator().manual_seed(C)
        z = (torch.randn(SAMPLES, C, generator=g) * 3).to(DEV)
        y = torch.randint(0, C, (SAMPLES,), generator=g).to(DEV)
        launches = {"soft_forward": lambda: _C.soft_forward(handle, z),
                    "soft_tree_loss": lambda: _C.soft_tree_loss(handle, z, y, 1.0, 1.0),
                    "hard_forward": lambda: _C.hard_forward(handle, z, want_onehot=False),
                    "hard_tree_loss": lambda: _C.hard_tree_loss(handle, z, y, 1.0, 2.0 / N)}
        for mode in modes:
            ops.set_rules_path(mode)
            try:
                for entry, fn in launches.items():
                    us, lo, hi, iters = per_launch_us(fn)
                    path = _C.last_rules_path()
                    ext, rowf = traffic(flat, entry)
                    moved = (ext + (rowf if path == "global" else 0)) * 4
                    lines.append(f"  {mode:6s} {entry:15s} {path:12s} {us:9.1f} us [{lo:.1f}, {hi:.1f}] x{iters:<5d} ext {ext * 4:7d} B"
                                 f"  row {rowf * 4 if path == 'global' else 0:8d} B  {moved * SAMPLES / us / 1e3:7.1f} GB/s  | {BOUND[path]}")
            finally:
                ops.set_rules_path("auto")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
