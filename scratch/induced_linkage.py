"""Writes profiles/induced_linkage.txt: nbdt_linkage (csrc/linkage.hip) on synthetic fp32 classifier matrices, its two
launches timed separately (torch.profiler's kernel records; HIP events around the call for the sum), the sklearn backend
on the same box where it imports, launch B's time per chain step next to the time ONE workgroup needs to stream a row
of the same matrix (probes/row_stream_probe, when it has been built), and -- once -- a tree induced at 21,841 x 2048
loaded and run through the large-hierarchy rules kernels.

  python scratch/induced_linkage.py [--out profiles/induced_linkage.txt] [--skip-host-above N]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbdt_path  # noqa: E402

nbdt_path.add()
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nbdt import _C  # noqa: E402
from nbdt import graph as G  # noqa: E402

DEV = "cuda:0"
SHAPES = [(1000, 1280), (1000, 2048), (10450, 2048), (21841, 2048)]
PROBE = os.path.join(nbdt_path.ROOT, "probes", "row_stream_probe")


def centers(n, d):
    g = torch.Generator().manual_seed(n + d)
    return torch.randn(n, d, generator=g).to(DEV)


class Run:
    """The buffers of one nbdt_linkage call, made once so that the timed region is the two launches."""

    def __init__(self, x, method="ward", metric="euclidean"):
        self.x, (self.n, self.d) = x, x.shape
        self.nbytes = G.linkage_workspace_bytes(self.n)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=DEV)
        self.merges = torch.empty((self.n - 1, 2), dtype=torch.int32, device=DEV)
        self.heights = torch.empty(self.n - 1, dtype=torch.float64, device=DEV)
        self.sizes = torch.empty(self.n - 1, dtype=torch.int32, device=DEV)
        self.method, self.metric = _C.NBDT_LINKAGE[method], _C.NBDT_METRIC[metric]

    def __call__(self):
        _C.check(_C.lib().nbdt_linkage(_C.ptr(self.x), self.n, self.d, self.method, self.metric, _C.ptr(self.ws),
                                       self.nbytes, _C.ptr(self.merges), _C.ptr(self.heights), _C.ptr(self.sizes),
                                       _C.stream_of(self.x)))

    def steps(self):
        """chain steps of the last run: the first int32 of the chain array (behind D and size[n])."""
        off = 8 * self.n * self.n + 4 * self.n
        return int(self.ws[off:off + 4].view(torch.int32).item())


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def kernel_ms(fn):
    """(launch A ms, launch B ms) from the profiler's kernel records, or None where it records none."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        us = getattr(ev, "device_time_total", None)
        if us is None:
            us = getattr(ev, "cuda_time_total", 0.0)
        for tag in ("pairwise_kernel", "chain_kernel"):
            if tag in ev.key:
                out[tag] = out.get(tag, 0.0) + us / 1e3
    return (out["pairwise_kernel"], out["chain_kernel"]) if len(out) == 2 else None


def row_stream_us(n):
    if not os.path.exists(PROBE):
        return None
    r = subprocess.run([PROBE, str(n)], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        return None
    return float(r.stdout.split("us_per_row")[1].split()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(nbdt_path.ROOT, "profiles", "induced_linkage.txt"))
    ap.add_argument("--skip-host-above", type=int, default=10450, help="no sklearn run for more rows than this")
    args = ap.parse_args()
    lines = [f"nbdt_linkage (ward, euclidean) on synthetic fp32 centres (torch.randn), {torch.cuda.get_device_name(0)} "
             f"({torch.cuda.get_device_properties(0).multi_processor_count} CUs)",
             "launch A = pairwise_kernel (all CUs), launch B = chain_kernel (one workgroup of 1024 lanes); ms per launch from "
             "the profiler's kernel records, 'call' = HIP events around nbdt_linkage (second of two runs); 'end to end' = "
             "linkage_children(backend=\"device\") with allocation, read-back and host labelling", ""]

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    try:
        import sklearn  # noqa: F401
        have_sklearn = True
    except ImportError:
        have_sklearn = False
    last = None
    for n, d in SHAPES:
        x = centers(n, d)
        run = Run(x)
        run()
        torch.cuda.synchronize()                      # first run: code object load, page faults of a fresh workspace
        call = event_ms(run)
        split = kernel_ms(run)
        steps = run.steps()
        finished = int(run.sizes.min().item()) >= 2 and int(run.sizes.max().item()) == n
        row_bytes = 12 * n                            # 8 n of D, 4 n of size[]
        emit(f"{n} x {d}: workspace {run.nbytes / 2**20:.1f} MiB, {steps} chain steps ({steps / n:.2f} n), "
             f"{n - 1} merges, finished {finished}")
        if split:
            a_ms, b_ms = split
            flops = 3.0 * d * n * (n + 64) / 2            # subtract, multiply, add per feature and pair, upper tiles
            emit(f"  launch A {a_ms:10.3f} ms   ({flops / a_ms / 1e9:.1f} fp64 Tflop/s, {8 * n * n / a_ms / 1e6:.1f} GB/s of D written)")
            emit(f"  launch B {b_ms:10.3f} ms   ({1e3 * b_ms / steps:.2f} us per chain step, {1e3 * b_ms / (n - 1):.2f} us per merge; "
                 f"a scan reads {row_bytes} B: {row_bytes * steps / b_ms / 1e6:.1f} GB/s if scans were all)")
        else:
            emit("  (no kernel records from the profiler: launches not split)")
        emit(f"  call     {call:10.3f} ms")
        del run
        t0 = time.perf_counter()
        children, heights = G.linkage_children(x, backend="device")
        emit(f"  end to end (device)  {1e3 * (time.perf_counter() - t0):10.1f} ms")
        stream = row_stream_us(n)
        if stream is not None and split:
            emit(f"  one workgroup streams a {row_bytes} B row (8 n + 4 n, random rows of an [n][n] fp64 matrix) in "
                 f"{stream:.2f} us: a chain step is {1e3 * split[1] / steps / stream:.2f} x that")
        if have_sklearn and n <= args.skip_host_above:
            xc = x.cpu()
            t0 = time.perf_counter()
            want, _ = G.linkage_children(xc, backend="sklearn")
            host = time.perf_counter() - t0
            emit(f"  sklearn backend      {1e3 * host:10.1f} ms   children equal: {bool(np.array_equal(want, children))}")
        elif have_sklearn:
            emit("  sklearn backend      not run at this size")
        else:
            emit("  sklearn backend      not importable on this box")
        emit()
        last = (x, children)
        torch.cuda.empty_cache()

    # once: the 21,841-class tree loads and runs through the large-hierarchy rules kernels
    x, _ = last
    n = x.shape[0]
    from nbdt.tree import Tree
    with tempfile.TemporaryDirectory() as tmp:
        wnids = [f"n{i:08d}" for i in range(n)]
        path_wnids, path_graph = os.path.join(tmp, "wnids.txt"), os.path.join(tmp, "graph-induced-synthetic.json")
        with open(path_wnids, "w") as f:
            f.write("\n".join(wnids))
        t0 = time.perf_counter()
        graph = G.build_induced_graph(wnids, state_dict={"linear.weight": x}, dataset="synthetic", backend="device")
        G.write_graph(graph, path_graph)
        t_graph = time.perf_counter() - t0
        t0 = time.perf_counter()
        tree = Tree(None, path_graph=path_graph, path_wnids=path_wnids, classes=wnids)
        t_tree = time.perf_counter() - t0
        handle = tree.device_handle(0)
        z = torch.randn(64, n, device=DEV) * 3
        y = torch.randint(0, n, (64,), device=DEV)
        P = _C.soft_forward(handle, z)
        path = _C.last_rules_path()
        loss, gz = _C.soft_tree_loss(handle, z, y, 1.0, 1.0)
        pred = _C.hard_forward(handle, z, want_onehot=False)[0]
        torch.cuda.synchronize()
        depth = handle.max_depth
        emit(f"tree induced on the device at {n} x {x.shape[1]}: build_induced_graph + write_graph {t_graph:.2f} s, Tree {t_tree:.2f} s, "
             f"{len(tree.inodes)} inner nodes, depth {depth}; rules path '{path}': soft_forward row sums in "
             f"[{P.sum(1).min().item():.6f}, {P.sum(1).max().item():.6f}], soft_tree_loss {loss.item():.4f} "
             f"(gradient finite: {bool(torch.isfinite(gz).all())}), hard_forward classes in [{int(pred.min())}, {int(pred.max())}]")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
