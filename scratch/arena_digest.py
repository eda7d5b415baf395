"""SHA-256 digests of what the arena passes leave behind, for comparing two commits bit for bit (run this file at both
and diff the output; profiles/arena_refactor_digests.txt).  Bare launches, three steps each on the ragged tables of the
LARS and adaptive tests: ops.sgd_step, LarsPlan.step (with the ratios), ArenaOptPlan.adamw and the three rmsprop forms,
ClipPlan.norm + apply (with the record), ema_update / ema_swap -- p, every state arena, the mirror and g.  Then, in
deterministic mode, store.flat and store.mom after three train_steps of the smoke() WRN, once per optimizer config."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nbdt_path  # noqa: E402

nbdt_path.add()
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
from nbdt import ops  # noqa: E402
from nbdt.engine import AdamWConfig, ClipConfig, LarsConfig, RMSpropConfig, WRNEngine, train_step  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402

import _adaptive_ref as A  # noqa: E402
import _lars_ref as R  # noqa: E402

DEV = "cuda:0"


def show(tag, **tensors):
    torch.cuda.synchronize()
    for name, t in tensors.items():
        if t is not None:
            raw = t.detach().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()
            print(f"{tag}.{name} {hashlib.sha256(raw).hexdigest()}")


def mirror_of(n):
    return torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)


# ---- the LARS tests' table: SGD over the whole arena, LARS, clipping, EMA
n, segments, p0, b0, grads = R.ragged_case(ops.LARS_ITEM)
p, buf, g, mirror = p0.to(DEV), b0.to(DEV), torch.empty(n, device=DEV), mirror_of(n)
for gk in grads:
    g.copy_(gk)
    ops.sgd_step(p, g, buf, 0.02, 0.9, 5e-4, 0.5, mirror, zero_grad=True)
show("sgd", p=p, buf=buf, mirror=mirror, g=g)

p, buf, mirror = p0.to(DEV), b0.to(DEV), mirror_of(n)
plan = ops.LarsPlan(n, segments, device=DEV)
for gk in grads:
    g.copy_(gk)
    plan.step(p, g, buf, 0.02, 0.9, 0.5, 1e-8, 0.5, mirror, zero_grad=True)
show("lars", p=p, buf=buf, mirror=mirror, g=g, ratios=plan.ratios())

clip = ops.ClipPlan(n, device=DEV)
for k, (gk, max_norm) in enumerate(zip(grads, (1.0, 1e6, 3.0))):      # clipped, not clipped, clipped
    g.copy_(gk)
    clip.norm(g, 0.5, max_norm)
    clip.apply(g)
    show(f"clip.step{k}", g=g, record=clip.record())

p, ema, mirror = p0.to(DEV), b0.to(DEV), mirror_of(n)
for _ in range(3):
    ops.ema_update(p, ema, 0.01)
show("ema.update", p=p, ema=ema)
ops.ema_swap(p, ema, mirror)
show("ema.swap", p=p, ema=ema, mirror=mirror)

# ---- the adaptive tests' table
n, rows, p0, b0, grads = A.ragged_table(ops.ARENA_OPT_ITEM)
plan = ops.ArenaOptPlan(n, rows, device=DEV)
for name in ("adamw", "rmsprop", "rmsprop_mu0", "rmsprop_tf"):
    s1_0, s2_0 = A.start_state("rmsprop" if name == "rmsprop_mu0" else name, n, rows, b0)
    p, s1, s2, g, mirror = p0.to(DEV), s1_0.to(DEV), s2_0.to(DEV), torch.empty(n, device=DEV), mirror_of(n)
    for t, gk in enumerate(grads, 1):
        g.copy_(gk)
        if name == "adamw":
            plan.adamw(p, g, s1, s2, 0.01, (0.9, 0.999), 1e-4, t, 0.5, mirror, zero_grad=True)
        elif name == "rmsprop_mu0":
            plan.rmsprop(p, g, s2, None, 0.01, 0.99, 1e-3, 0.0, False, 0.5, mirror, zero_grad=True)
        else:
            plan.rmsprop(p, g, s2, s1, 0.01, 0.9 if name == "rmsprop_tf" else 0.99, 1e-3, 0.9, name == "rmsprop_tf", 0.5,
                         mirror, zero_grad=True)
    show(name, p=p, s1=s1, s2=s2, mirror=mirror, g=g)

# ---- train_step of the smoke() WRN, deterministic mode
ops.set_deterministic(True)
crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")
gen = torch.Generator().manual_seed(0)
img = torch.randn(8, 3, 32, 32, generator=gen).to(DEV)
y = torch.randint(0, 10, (8,), generator=gen).to(DEV)
for name, lr, kwargs in (("sgd", 0.05, {}),
                         ("sgd_clip", 0.05, dict(clip=ClipConfig(1.0))),
                         ("lars", 0.2, dict(lars=LarsConfig(0.02))),
                         ("adamw", 1e-3, dict(optim=AdamWConfig())),
                         ("rmsprop", 1e-3, dict(optim=RMSpropConfig())),
                         ("rmsprop_tf", 1e-3, dict(optim=RMSpropConfig(0.9, 1e-3, True)))):
    eng = WRNEngine(num_classes=10, blocks=10, width_factor=2, device=DEV, seed=0)
    for _ in range(3):
        loss = train_step(eng, crit, img, y, lr=lr, **kwargs)
    eng.join_side_stream()
    show(f"train_step.{name}", flat=eng.store.flat, mom=eng.store.mom, sq=eng.store.sq, loss=loss)
