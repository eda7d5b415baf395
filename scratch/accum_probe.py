"""Does every engine family's backward ADD to store.grad?  Two backward passes without a zero between them against twice
one pass (deterministic mode), per named parameter."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbdt_path
nbdt_path.add()
import torch
from nbdt import ops
from nbdt import engine as E
from nbdt.engine_effnet import EfficientNetEngine

ops.set_deterministic(True)
dev = "cuda:0"


class CE:
    def loss_and_grad(self, z, y, grad_scale=1.0):
        zz = z.detach().float().clone().requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(zz, y)
        loss.backward()
        return loss.detach(), zz.grad.to(z.dtype).contiguous()


cases = [("WRN", lambda: E.WRNEngine(10, 10, 2, device=dev, seed=1), 32, 10),
         ("ResNet18", lambda: E.ResNetEngine(10, device=dev, seed=1), 32, 10),
         ("Bottleneck50", lambda: E.BottleneckEngine(10, device=dev, seed=1), 32, 10),
         ("ImageNetResNet18", lambda: E.ImageNetResNetEngine(10, (2, 2, 2, 2), device=dev, seed=1), 64, 10),
         ("ImageNetBottleneck50", lambda: E.ImageNetBottleneckEngine(10, (3, 4, 6, 3), device=dev, seed=1), 64, 10),
         ("EfficientNetB0", lambda: EfficientNetEngine(num_classes=10, dropout_rate=0.0, device=dev, seed=1), 32, 10)]
crit = CE()
for name, make, size, classes in cases:
    eng = make()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(8, 3, size, size, generator=g).to(dev)
    y = torch.randint(0, classes, (8,), generator=g).to(dev)

    def once():
        z = eng.forward(x, training=True)
        _, gz = crit.loss_and_grad(z, y)
        eng.backward(gz)
        eng.join_side_stream()
        torch.cuda.synchronize()

    eng.zero_grad(); once()
    one = {k: v.detach().double().cpu() for k, v in eng.named_params("grad").items()}
    eng.zero_grad(); once(); once()
    two = {k: v.detach().double().cpu() for k, v in eng.named_params("grad").items()}
    worst, worst_name = 0.0, None
    for k in one:
        s = one[k].abs().max().item()
        if s == 0:
            continue
        e = ((two[k] - 2 * one[k]).abs().max().item()) / (2 * s)
        if e > worst:
            worst, worst_name = e, k
    print(f"{name}: {len(one)} tensors, worst |two passes - 2 x one| / max|2 x one| = {worst:.3e} ({worst_name})", flush=True)
