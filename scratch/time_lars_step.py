"""engine.sgd_step and engine.lars_step alone on WRN-28-10 (36.5 M parameters), in one process: each the median of 20
event-bracketed calls after 3 warm-up calls, three interleaved rounds; then the bare launches without the derived-weight
refresh (ops.sgd_step, LarsPlan.step) and LarsPlan.step on a table with every adapt = 0, which has no norm items -- fold +
update only, so the difference to the full plan is the partial-sums launch and its kernel boundary.  An engine without
lars_step (the parent commit) reports the SGD figures alone.  profiles/lars_step.txt."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbdt_path  # noqa: E402

nbdt_path.add()
import torch  # noqa: E402
from nbdt import ops  # noqa: E402
from nbdt.engine import WRNEngine  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "run"
eng = WRNEngine(num_classes=10, blocks=28, width_factor=10, device="cuda:0", seed=0)
eng.store.grad.normal_(0, 1e-3)
s = eng.store
n = s.flat.numel()


def timed(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


def line(label, row):
    return f"{tag} {label}: " + "  ".join(f"{k} median {v[0]:.1f} us min {v[1]:.1f} us" for k, v in row.items())


out = [f"{tag}: WRN-28-10 arena n = {n} fp32 elements; SGD pass 26 n = {26 * n / 1e6:.1f} MB, LARS 34 n = {34 * n / 1e6:.1f} MB"]
has_lars = hasattr(eng, "lars_step")
for r in range(3):
    row = {"sgd_step": timed(lambda: eng.sgd_step(1e-6, zero_grad=True))}
    if has_lars:
        row["lars_step"] = timed(lambda: eng.lars_step(1e-6, zero_grad=True))
    out.append(line(f"round {r}", row))
raw = {"sgd launch": timed(lambda: ops.sgd_step(s.flat, s.grad, s.mom, 1e-6, 0.9, 5e-4, 1.0, s.bf16, zero_grad=True))}
if has_lars:
    args = (s.flat, s.grad, s.mom, 1e-6, 0.9, 1e-3, 1e-8, 1.0, s.bf16)
    plan = ops.LarsPlan(n, s.segments(5e-4, True), device=eng.device)
    flat = ops.LarsPlan(n, [(o, l, w, 0) for o, l, w, _ in s.segments(5e-4, True)], device=eng.device)
    raw["lars launches"] = timed(lambda: plan.step(*args, zero_grad=True))
    raw["lars fold + update only"] = timed(lambda: flat.step(*args, zero_grad=True))
out.append(line("launches alone", raw))
print("\n".join(out))
