"""Synthetic hierarchies for the tree-rule kernels, and a restatement of the paths csrc/rules.hip takes on them.

The control flow of csrc/rules.hip is chosen by the shape of the hierarchy (C classes, N inner nodes, R child slots,
L = sum of leaf depths), not by the batch.  The generators here write a graph JSON and a wnid list that both
``nbdt.tree.Tree(None, path_graph=..., path_wnids=..., classes=...)`` and ``nbdt_oracle.OracleTree`` load;
``describe(flat)`` says which of the file's paths a ``FlatTree`` reaches, so that tests/test_tree_shapes.py can assert
that every fixture still reaches the cell it was built for, without a GPU.

``describe`` is copied from csrc/rules.hip BY HAND.  A change to any of these has to be repeated here:

  pick_tps ...................... ``static int pick_tps(int C, int R)``
  Gather U, nr, left ............ ``struct Gather``: ``U``, ``S`` and ``issue()`` (``cnt``, ``nr``, ``left``), lane g_tid = 0
  chunks, schedule rows ......... ``build_slot_schedule`` (stable sort by length, chunks of 64, least-loaded wave first)
  peel .......................... ``long_chain``: ``peel = (4 - ((a >> 2) & 3)) & 3`` for the chains of 16 or more
                                  elements that ``chains`` sends there; the address is the stage row of each kernel
  joint_of ...................... ``joint_of<TPS>()``
  tree_lds_ints, block ints ..... ``tree_lds_ints``, ``stats_small_ints``, ``stats_block_ints``
  staged ........................ ``NBDT_DISPATCH_RULES_EX`` with ``kLdsBytes``, ``kStagePad`` and the BASE_FLOATS every
                                  ``NBDT_DISPATCH_RULES`` call passes (``front_floats`` below: also the offset of ``stage``
                                  inside a sample's LDS row in the kernel of that entry point)
  fused head .................... ``launch_head`` and the NBDT_HEAD ladder of ``nbdt_head_soft_tree_loss``
"""
import json
import os

import numpy as np

LDS_BYTES = 160 * 1024      # kLdsBytes
STAGE_PAD = 4               # kStagePad
BLOCK = 256                 # kBlock


# ------------------------------------------------------------------------------------------------------------
# generators: (directory, sizes) -> (path_graph, path_wnids, leaves)

def _write(directory, name, inner, leaves, links):
    pg, pw = os.path.join(str(directory), f"{name}.json"), os.path.join(str(directory), f"{name}.txt")
    with open(pg, "w") as f:
        json.dump({"directed": True, "multigraph": False, "graph": {},
                   "nodes": [{"id": w} for w in inner + leaves], "links": links}, f)
    with open(pw, "w") as f:
        f.write("\n".join(leaves) + "\n")
    return pg, pw, leaves


def caterpillar(tmp_path, C):
    """Every inner node keeps one leaf and hands the rest down: depth C-1, sum of leaf depths ~ C*C/2."""
    leaves = [f"f{i:08d}" for i in range(C)]
    inner = [f"n{i:08d}" for i in range(C - 1)]
    links = []
    for i in range(C - 1):
        links.append({"source": inner[i], "target": leaves[i]})
        links.append({"source": inner[i], "target": inner[i + 1] if i + 1 < C - 1 else leaves[C - 1]})
    return _write(tmp_path, f"cat{C}", inner, leaves, links)


def star(tmp_path, C):
    """One inner node with C leaf children: N = 1, R = L = C, fan-out C."""
    leaves = [f"f{i:08d}" for i in range(C)]
    root = "n00000000"
    return _write(tmp_path, f"star{C}", [root], leaves, [{"source": root, "target": w} for w in leaves])


def kary(tmp_path, C, k):
    """A complete k-ary tree built bottom-up over the C leaves: consecutive groups of k become one parent, level by level
    (the last group of a level may be smaller; a group of one is handed up as it is).  The root sorts first."""
    leaves = [f"f{i:08d}" for i in range(C)]
    levels, level = [], list(leaves)
    while len(level) > 1:
        groups = [level[i:i + k] for i in range(0, len(level), k)]
        levels.append(groups)
        level = [None] * len(groups)        # named below, once the number of levels is known
        for i, g in enumerate(groups):
            level[i] = (len(levels) - 1, i) if len(g) > 1 else g[0]
    top = len(levels) - 1
    name = lambda w: w if isinstance(w, str) else f"n{top - w[0]:02d}{w[1]:06d}"
    inner, links = [], []
    for li in range(top, -1, -1):
        for i, g in enumerate(levels[li]):
            if len(g) == 1:
                continue
            inner.append(name((li, i)))
            links.extend({"source": name((li, i)), "target": name(w)} for w in g)
    return _write(tmp_path, f"kary{C}_{k}", inner, leaves, links)


GENERATORS = {"caterpillar": caterpillar, "star": star, "kary": kary}

# name -> (generator, arguments): the fixtures of tests/test_tree_shapes.py and tests/test_rules_shapes_gpu.py
SHAPES = {
    "cat33": ("caterpillar", (33,)), "cat34": ("caterpillar", (34,)), "cat120": ("caterpillar", (120,)),
    "cat200": ("caterpillar", (200,)), "cat257": ("caterpillar", (257,)), "cat258": ("caterpillar", (258,)),
    "cat264": ("caterpillar", (264,)), "cat280": ("caterpillar", (280,)),
    "star64": ("star", (64,)), "star65": ("star", (65,)), "star300": ("star", (300,)), "star513": ("star", (513,)),
    "kary243_3": ("kary", (243, 3)), "kary600_70": ("kary", (600, 70)),
}
RAMP = 8.0          # height of the logit ramp of a caterpillar (see logits_for): enough down to depth 279


def build(name, directory):
    gen, args = SHAPES[name]
    return GENERATORS[gen](directory, *args)


def logits_for(name, B, C, seed=None):
    """Seeded fp32 logits [B, C] that keep every path probability of the shape a normal fp32 number.

    A caterpillar multiplies up to C-1 factors: with plain 3*randn the deep classes underflow to exact zeros from depth
    ~120 on, and a kernel returning zeros would pass.  ``0.5*randn + 8*i/C`` makes the walk prefer to go on, so the deep
    products stay above 1e-30 (asserted with the oracle in tests/test_tree_shapes.py).  Stars and k-ary trees are
    shallow: 3*randn."""
    import torch
    gen = torch.Generator().manual_seed(C + 1000 * B if seed is None else seed)
    z = torch.randn(B, C, generator=gen)
    if SHAPES[name][0] == "caterpillar":
        return z * 0.5 + RAMP * torch.arange(C, dtype=torch.float32) / C
    return z * 3


# ------------------------------------------------------------------------------------------------------------
# the host-side choices of csrc/rules.hip

def pick_tps(C, R):
    return 64 if (C <= 64 and R <= 64) else 256 if (C <= 512 and R <= 512) else 1024


def block_of(tps):
    return max(tps, BLOCK)


def joint_of(tps):
    return 2 if tps == 256 else 1


def slot_schedule(slot_off, lanes):
    """build_slot_schedule: ([3][rows * lanes] int array, rows, chunks)."""
    R = len(slot_off) - 1
    length = lambda s: int(slot_off[s + 1] - slot_off[s])
    order = sorted(range(R), key=lambda s: -length(s))            # sorted() is stable, like std::stable_sort
    waves, chunks = lanes // 64, (R + 63) // 64
    mine, load = [[] for _ in range(waves)], [0] * waves
    for c in range(chunks):
        w = min(range(waves), key=lambda i: (load[i], i))         # the first least-loaded wave
        mine[w].append(c)
        load[w] += 64 + 8 * length(order[c * 64])
    rows = max(len(m) for m in mine)
    n = rows * lanes
    out = np.full((3, n), -1, dtype=np.int64)
    for w in range(waves):
        for k, c in enumerate(mine[w]):
            for l in range(64):
                i = c * 64 + l
                if i >= R:
                    break
                at, s = k * lanes + w * 64 + l, order[i]
                out[:, at] = (s, slot_off[s], slot_off[s + 1])
    return out, rows, chunks


def max_depth(flat):
    """nbdt_tree_create: inner nodes on the longest walk from the root."""
    depth, changed = [1] * flat.num_inodes, True
    while changed:                                                 # relax until stable, like the C loop
        changed = False
        for n in range(flat.num_inodes):
            for s in range(flat.node_off[n], flat.node_off[n + 1]):
                nx = int(flat.slot_next[s])
                if nx >= 0 and depth[n] < depth[nx] + 1:
                    depth[n] = depth[nx] + 1
                    changed = True
    return depth[flat.root]


def tree_lds_ints(C, N, R, sched_len, nxt):
    return ((N + 1) + (R + 1) + (C + 1) + 3 * sched_len + (R if nxt else 0) + 3) & ~3


def stats_block_ints(N, depth):
    small = (5 * N + 4 + depth + 1 + 1) & ~1
    return (small + 4 * N + 3) & ~3


def front_floats(entry, C, N, R):
    """BASE_FLOATS of the entry point's NBDT_DISPATCH_RULES call = offset of `stage` in a sample's LDS row."""
    return {"soft_forward": C + 2 * R, "node_outputs": C + 2 * R, "soft_backward": 2 * C + 2 * R,
            "soft_tree_loss": 3 * C + 2 * R + 16, "hard_tree_loss": 2 * C + 2 * R + 16,
            "hard_forward": C + R + 8 + 2 * N, "tree_stats": C + 2 * R + 2 * N + 32}[entry]


ENTRY_POINTS = ("soft_forward", "node_outputs", "soft_backward", "soft_tree_loss", "hard_tree_loss", "hard_forward",
                "tree_stats")       # soft_tree_loss: both soft_loss_kernel and soft_target_loss_kernel (one row layout)


def _fits(tl_ints, spb, floats):
    return (tl_ints + spb * floats + STAGE_PAD) * 4 <= LDS_BYTES


def head_launch(d, K):
    """launch_head through the NBDT_HEAD ladder: (samples per block, staged) of the launch that is made, None when the
    entry point refuses (TPS 1024, or nothing fits)."""
    if d["tps"] > 256:
        return None
    tl = tree_lds_ints(d["C"], d["N"], d["R"], d["sched_len"], False)
    floats = K + 3 * d["C"] + 2 * d["R"] + 16
    for spb in ((8, 4, 1) if d["tps"] == 64 else (4, 2, 1)):
        if _fits(tl, spb, floats + d["L"]):
            return spb, True
        if _fits(tl, spb, floats):
            return spb, False
    return None


def _peels(tl_ints, spb, front, stride, starts):
    """long_chain's peel for chains starting at float `b` of the stage row of every sample group of a block (the dynamic
    LDS starts 16-byte aligned and tl_ints is a multiple of 4)."""
    return {(-(tl_ints + g * stride + front + int(b))) % 4 for g in range(spb) for b in starts}


def describe(flat):
    """The paths of csrc/rules.hip a FlatTree reaches (see the module docstring for the lines restated)."""
    C, N, R = flat.num_classes, flat.num_inodes, flat.num_slots
    L = int(flat.slot_off[R])
    tps = pick_tps(C, R)
    spb = block_of(tps) // tps
    U = 4 if tps > 256 else 8
    cnt = (L + tps - 1) // tps if L > 0 else 0                     # lane 0 of Gather::issue, both index arrays have L
    nr = cnt // U
    left = cnt - nr * U
    sched, rows, chunks = slot_schedule(flat.slot_off, tps)
    sched_len = rows * tps
    depth = max_depth(flat)
    d = {"C": C, "N": N, "R": R, "L": L, "tps": tps, "spb": spb, "joint": joint_of(tps), "U": U, "nr": nr, "left": left,
         "trailing_block": nr % 2 == 1, "pipelined_trips": nr // 2,
         "chunks": chunks, "rows": rows, "sched_len": sched_len, "max_depth": depth,
         "max_fanout": int(np.diff(flat.node_off).max()),
         "binary_nodes": int((np.diff(flat.node_off) == 2).sum()),
         "longest_slot": int(np.diff(flat.slot_off).max()), "longest_path": int(np.diff(flat.cls_off).max())}
    staged, slot_peels, path_peels = {}, {}, {}
    long_slots = [b for b, e in zip(flat.slot_off[:-1], flat.slot_off[1:]) if e - b >= 16]
    long_paths = [b for b, e in zip(flat.cls_off[:-1], flat.cls_off[1:]) if e - b >= 16]
    for entry in ENTRY_POINTS:
        tl = tree_lds_ints(C, N, R, sched_len, entry == "hard_forward")
        if entry == "tree_stats":
            tl += stats_block_ints(N, depth)
        front = front_floats(entry, C, N, R)
        staged[entry] = _fits(tl, spb, front + L)
        if not staged[entry] and not _fits(tl, spb, front):
            staged[entry] = None                                   # "hierarchy too large for LDS"
        if staged[entry]:                                          # the unstaged chains never reach long_chain
            slot_peels[entry] = _peels(tl, spb, front, front + L, long_slots)
            path_peels[entry] = _peels(tl, spb, front, front + L, long_paths)
        else:
            slot_peels[entry], path_peels[entry] = set(), set()
    d["staged"], d["slot_peels"], d["path_peels"] = staged, slot_peels, path_peels
    # hard_forward, node_outputs: no class -> slots chains (next_idx is null)
    for entry in ("hard_forward", "node_outputs"):
        path_peels[entry] = set()
    return d
