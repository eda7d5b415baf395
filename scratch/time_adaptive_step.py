"""engine.sgd_step, engine.adamw_step and engine.rmsprop_step alone on WRN-28-10 (36.5 M parameters), in one process: each
the median of 20 event-bracketed calls after 3 warm-up calls, three interleaved rounds; then the bare launches without the
derived-weight refresh (ops.sgd_step, ArenaOptPlan.adamw / .rmsprop in its three forms) with the bytes each moves and the
rate that gives.  A fresh engine per adaptive optimizer: the state arenas belong to one optimizer at a time.
profiles/adaptive_step.txt."""
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


def line(label, row, bytes_per=None):
    parts = []
    for k, v in row.items():
        rate = f" ({bytes_per[k] * n / v[0] / 1e6:.2f} TB/s)" if bytes_per else ""
        parts.append(f"{k} median {v[0]:.1f} us min {v[1]:.1f} us{rate}")
    return f"{tag} {label}: " + "  ".join(parts)


out = [f"{tag}: WRN-28-10 arena n = {n} fp32 elements; SGD pass 26 n = {26 * n / 1e6:.1f} MB, AdamW / RMSprop with momentum "
       f"34 n = {34 * n / 1e6:.1f} MB, RMSprop without momentum 26 n"]
# engine level: the SGD rounds first (store.mom is theirs), then AdamW, a reset, RMSprop
rows = [{} for _ in range(3)]
for r in range(3):
    rows[r]["sgd_step"] = timed(lambda: eng.sgd_step(1e-6, zero_grad=True))
eng.reset_optimizer_state()
for r in range(3):
    rows[r]["adamw_step"] = timed(lambda: eng.adamw_step(1e-6, zero_grad=True))
eng.reset_optimizer_state()
for r in range(3):
    rows[r]["rmsprop_step (tf)"] = timed(lambda: eng.rmsprop_step(1e-6, 0.9, 1e-3, 0.9, 1e-5, tf=True, zero_grad=True))
for r in range(3):        # once more, interleaved, so that drift over the process shows
    rows[r]["sgd_step again"] = timed(lambda: eng.sgd_step(1e-6, zero_grad=True))
for r in range(3):
    out.append(line(f"round {r}", rows[r]))
# the launches alone, interleaved round by round
plan = ops.ArenaOptPlan(n, s.segments(5e-4, True), device=eng.device)
s.init_sq()
s.mom.zero_()
calls = {
    "sgd launch": (26, lambda: ops.sgd_step(s.flat, s.grad, s.mom, 1e-6, 0.9, 5e-4, 1.0, s.bf16, zero_grad=True)),
    "adamw launch": (34, lambda: plan.adamw(s.flat, s.grad, s.mom, s.sq, 1e-6, (0.9, 0.999), 1e-8, 10, 1.0, s.bf16,
                                            zero_grad=True)),
    "rmsprop launch": (34, lambda: plan.rmsprop(s.flat, s.grad, s.sq, s.mom, 1e-6, 0.99, 1e-8, 0.9, False, 1.0, s.bf16,
                                                zero_grad=True)),
    "rmsprop tf launch": (34, lambda: plan.rmsprop(s.flat, s.grad, s.sq, s.mom, 1e-6, 0.9, 1e-3, 0.9, True, 1.0, s.bf16,
                                                   zero_grad=True)),
    "rmsprop mu=0 launch": (26, lambda: plan.rmsprop(s.flat, s.grad, s.sq, None, 1e-6, 0.99, 1e-8, 0.0, False, 1.0, s.bf16,
                                                     zero_grad=True)),
}
for r in range(2):
    out.append(line(f"launches alone, round {r}", {k: timed(fn) for k, (_, fn) in calls.items()},
                    {k: b for k, (b, _) in calls.items()}))
print("\n".join(out))
