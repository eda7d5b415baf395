"""SHA-256 digests of what the BatchNorm protocol computes, for comparing two commits bit for bit (run this file at both
and diff the output; profiles/bn_protocol_digests.txt).  Deterministic mode throughout (nbdt_set_deterministic): same
launches + same inputs => same bits.

Engines: logits, loss, the flat gradient and the running statistics after each of two training steps (forward, tree loss,
backward, SGD) of
  WRN-16-2, 16 x 32x32: split, fused-with-sharing, fused and plain (fuse_stats off) backward forms, two streams and one;
  ResNet18 with num_blocks (2, 1, 1, 1), 8 x 32x32: two streams, one stream, fuse_bn1_bwd off;
  the Bottleneck (2, 1, 1, 1) of tests/test_resnet_schedule_gpu.py, 8 x 32x32: two streams;
  EfficientNet-B0, 4 x 64x64, stochastic depth 0 and 0.2: two streams and one.
Entries: every nbdt_bn_* / nbdt_bn_act_* / nbdt_dwconv_* entry point that sums into the 32 slots, on 2 x 8x8 tensors of
C = 64 (40 channels padded) and C = 320."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbdt_path  # noqa: E402

nbdt_path.add()
import torch  # noqa: E402
from torch import nn  # noqa: E402
from nbdt import engine as E  # noqa: E402
from nbdt import ops  # noqa: E402
from nbdt.engine_effnet import EfficientNetEngine  # noqa: E402
from nbdt.loss import SoftTreeSupLoss  # noqa: E402

DEV = "cuda:0"


def digest(tag, t):
    torch.cuda.synchronize()
    raw = t.detach().float().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
    print(f"{tag} {hashlib.sha256(raw).hexdigest()}", flush=True)


def steps(tag, eng, B, size, crit):
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, 3, size, size, generator=g).to(DEV)
    y = torch.randint(0, 10, (B,), generator=g).to(DEV)
    for step in range(2):
        eng.zero_grad()
        z = eng.forward(x, training=True)
        loss, gz = crit.loss_and_grad(z, y)
        eng.backward(gz)
        digest(f"{tag}.step{step}.logits", z)
        digest(f"{tag}.step{step}.loss", loss)
        digest(f"{tag}.step{step}.grad", eng.store.grad)
        eng.sgd_step(0.05, momentum=0.9, weight_decay=5e-4)
        digest(f"{tag}.step{step}.running", torch.cat([b.reshape(-1).float().to(DEV) for b in eng.named_buffers().values()]))


def engines():
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")
    settings = (("split", lambda e: e.set_cu_share(47.0, calibrate=False)),
                ("shared", lambda e: e.set_cu_share(47.0, calibrate=False, split_reduce=False)),
                ("fused", lambda e: e.set_cu_share(None)),
                ("plain", lambda e: (e.set_cu_share(47.0, calibrate=False), setattr(e, "fuse_stats", False))))
    for name, setup in settings:
        for overlap in (True, False):
            eng = E.WRNEngine(num_classes=10, blocks=16, width_factor=2, device=DEV, seed=5)
            setup(eng)
            eng.set_overlap(overlap)
            steps(f"wrn16_2.{name}.{'two' if overlap else 'one'}_stream", eng, 16, 32, crit)
    for name, setup in (("two_streams", lambda e: None), ("one_stream", lambda e: e.set_overlap(False)),
                        ("no_fused_bn1_bwd", lambda e: setattr(e, "fuse_bn1_bwd", False))):
        eng = E.ResNetEngine(num_classes=10, num_blocks=(2, 1, 1, 1), device=DEV, seed=5)
        setup(eng)
        steps(f"resnet_2111.{name}", eng, 8, 32, crit)
    steps("bottleneck_2111.two_streams", E.BottleneckEngine(num_classes=10, num_blocks=(2, 1, 1, 1), device=DEV, seed=5),
          8, 32, crit)
    for sd in (0.0, 0.2):
        for overlap in (True, False):
            eng = EfficientNetEngine(num_classes=10, device=DEV, seed=5, stochastic_depth_prob=sd)
            eng.set_overlap(overlap)
            steps(f"effnet_b0.sd{sd}.{'two' if overlap else 'one'}_stream", eng, 4, 64, crit)


def entries():
    B, H, W = 2, 8, 8
    for C in (64, 320):
        g = torch.Generator().manual_seed(C)

        def act(scale=1.0):
            t = ops.padded(B, H, W, C, DEV, torch.bfloat16)
            ops.interior(t).copy_((scale * torch.randn(B, H, W, C, generator=g)).to(torch.bfloat16))
            return t

        def vec(n=C, lo=None):
            v = torch.randn(n, generator=g)
            return (v.abs() + lo if lo is not None else v).to(DEV)

        x, gy = act(), act(0.1)
        mean, rstd, gamma, beta = vec(), vec(lo=0.5), vec(lo=0.5), vec()
        scratch = torch.zeros(ops.BN_SLOTS * 2 * C, device=DEV)
        pair = (torch.zeros_like(scratch), torch.zeros_like(scratch))
        dsum = torch.zeros(2 * C, device=DEV)
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        gx = ops.padded(B, H, W, C, DEV, torch.bfloat16)
        tag = f"entry.C{C}"

        def out(name, *extra):
            for n, t in (("gx", gx), ("dsum", dsum), ("dgamma", dg), ("dbeta", db), ("slots", scratch)) + extra:
                digest(f"{tag}.{name}.{n}", t)

        m, r = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        ops.bn_stats(x, scratch, m, r, rm, rv)
        out("bn_stats", ("mean", m), ("rstd", r), ("running_mean", rm), ("running_var", rv))
        ops.bn_bwd(gy, None, x, mean, rstd, gamma, scratch, dsum, dg, db, gx, relu=True, beta=beta)
        out("bn_bwd_relu")
        ops.bn_bwd(gy, None, x, mean, rstd, gamma, scratch, dsum, dg, db, gx, relu=False, gx_add=gy)
        out("bn_bwd_linear")
        ops.bn_bwd_cus(gy, x, mean, rstd, gamma, beta, scratch, dsum, dg, db, gx, 24)
        out("bn_bwd_reduce_cus")
        ops.bn_bwd_cus(gy, x, mean, rstd, gamma, beta, pair, dsum, dg, db, gx, 24, gx_add=gy)
        out("bn_bwd_cus", ("slots0", pair[0]), ("slots1", pair[1]))
        ops.bn_bwd_cus(gy, x, mean, rstd, gamma, beta, pair[::-1], dsum, dg, db, gx, 24)
        out("bn_bwd_cus_swapped", ("slots0", pair[0]), ("slots1", pair[1]))
        gpooled = (0.1 * torch.randn(B, C, generator=g)).to(DEV)
        ops.pool_bn_bwd(gpooled, x, mean, rstd, gamma, beta, scratch, dsum, dg, db, gx)
        out("pool_bn_bwd")
        gate, rows = torch.rand(B, C, generator=g).to(DEV), torch.tensor([0.0, 1.25], device=DEV)
        ops.bn_act_bwd(gy, x, mean, rstd, gamma, beta, scratch, dsum, dg, db, gx)
        out("bn_act_bwd")
        ops.bn_act_bwd(gy, x, mean, rstd, gamma, beta, scratch, dsum, dg, db, gx, gate=gate, gpool=gpooled, gx_add=gy)
        out("bn_act_bwd_se")
        ops.bn_act_bwd(None, x, mean, rstd, gamma, beta, scratch, dsum, dg, db, gx, gpool=gpooled)
        out("bn_act_bwd_pool")
        ops.bn_act_bwd(gy, x, mean, rstd, gamma, beta, scratch, dsum, dg, db, gx, act=ops.ACT_NONE, row_scale=rows)
        out("bn_act_bwd_rows")
        for k in (3, 5):
            w = torch.randn(k * k, C, generator=g).to(DEV)
            for stride in (1, 2):
                y = ops.padded(B, H // stride, W // stride, C, DEV, torch.bfloat16)
                ops.dwconv_fwd(x, w, y, k, stride, bn_scratch=scratch)
                digest(f"{tag}.dwconv_fwd_k{k}s{stride}.y", y)
                digest(f"{tag}.dwconv_fwd_k{k}s{stride}.slots", scratch)
                ops.bn_stats(y, scratch, m, r, rm, rv, slots_filled=True)
                out(f"dwconv_fwd_k{k}s{stride}.bn_stats", ("mean", m), ("rstd", r), ("running_var", rv))
            ops.dwconv_bwd_data_bn(gy, w, gx, k, x, mean, rstd, gamma, beta, scratch)
            digest(f"{tag}.dwconv_bwd_data_bn_k{k}.gx", gx)
            digest(f"{tag}.dwconv_bwd_data_bn_k{k}.slots", scratch)
            ops.bn_act_bwd_apply(gx, x, mean, rstd, gamma, beta, scratch, dsum, dg, db, gx)
            out(f"dwconv_bwd_data_bn_k{k}.bn_act_bwd_apply")


ops.set_deterministic(True)
entries()
engines()
ops.set_deterministic(False)
# the atomic path on the same entry shapes is not bit-stable between runs; tests/test_bn_exact_gpu.py and
# tests/test_effnet_gpu.py cover it bit for bit on exactly representable fixtures
