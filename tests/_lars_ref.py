"""float64 reference of the LARS step (nbdt_lars_step, include/nbdt_hip.h) for tests/test_lars*.py.

Per segment (offset, length, weight_decay, adapt) the two norms and the trust ratio are computed with numpy; the update is
``torch.optim.SGD(momentum, weight_decay=0)`` applied to the gradient ``ratio * (grad_scale * g + wd * p)``, which is the
form apex's ``LARC(clip=False)`` gives a wrapped ``optim.SGD``.  Elements outside every segment get a zero gradient and a
zero momentum buffer here and therefore never move; the tests check them on the device side (sentinels)."""
import numpy as np
import torch


def trust_ratio(p, g, weight_decay, adapt, trust, eps, grad_scale):
    """ratio of one segment from float64 numpy vectors."""
    if not adapt:
        return 1.0
    wn = float(np.sqrt(np.sum(p * p)))
    gs = grad_scale * g
    gn = float(np.sqrt(np.sum(gs * gs)))
    if not (wn > 0.0 and gn > 0.0):
        return 1.0
    return trust * wn / (gn + weight_decay * wn + eps)


class LarsRef:
    """p, buf: flat tensors (any float dtype, copied to float64); segments: rows (offset, length, weight_decay, adapt)."""

    def __init__(self, p, buf, segments, momentum):
        self.segments = [(int(o), int(l), float(w), int(a)) for o, l, w, a in segments]
        self.inside = torch.zeros(p.numel(), dtype=torch.bool)
        for o, l, _, _ in self.segments:
            self.inside[o:o + l] = True
        self.p = torch.nn.Parameter(p.detach().cpu().double().clone())
        self.opt = torch.optim.SGD([self.p], lr=1.0, momentum=momentum, weight_decay=0.0)
        b = buf.detach().cpu().double().clone()
        b[~self.inside] = 0.0
        self.opt.state[self.p]["momentum_buffer"] = b

    def step(self, g, lr, trust, eps, grad_scale=1.0):
        """One step on the gradient g (flat, any float dtype).  Returns the list of trust ratios."""
        g = g.detach().cpu().double().numpy()
        p = self.p.detach().numpy()
        d = np.zeros_like(p)
        ratios = []
        for o, l, wd, adapt in self.segments:
            r = trust_ratio(p[o:o + l], g[o:o + l], wd, adapt, trust, eps, grad_scale)
            d[o:o + l] = r * (grad_scale * g[o:o + l] + wd * p[o:o + l])
            ratios.append(r)
        self.p.grad = torch.from_numpy(d)
        for group in self.opt.param_groups:
            group["lr"] = lr
        self.opt.step()
        return ratios

    @property
    def param(self):
        return self.p.detach()

    @property
    def buf(self):
        return self.opt.state[self.p]["momentum_buffer"]


def ragged_case(item, seed=0):
    """The ragged table of the GPU tests: lengths 1, 3, 4, 5, 8, 1000 and one segment of more than three blocks' worth of
    elements (a block of csrc/lars.hip reduces 4 * item), gaps of 4-11 elements between the rows and after the last one,
    one adapt = 0 row, a different decay per row.  Returns (n, segments, p, buf, [g of step 0, 1, 2]) as float32 tensors:
    sentinel 7.0 in the gaps of p and buf, random gradients everywhere (the gaps' must not be read)."""
    lengths = [1, 3, 4, 5, 8, 1000, 3 * 4 * item + item + 5]
    segments, off = [], 0
    for i, l in enumerate(lengths):
        segments.append((off, l, 1e-3 * (i + 1), 0 if i == 4 else 1))
        off = (off + l + 4 + 4 * (i % 2) + 3) // 4 * 4
    n = off
    gen = torch.Generator().manual_seed(seed)
    p = torch.full((n,), 7.0)
    buf = torch.full((n,), 7.0)
    for o, l, _, _ in segments:
        p[o:o + l] = 0.5 * torch.randn(l, generator=gen)
        buf[o:o + l] = 0.1 * torch.randn(l, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(3)]
    return n, segments, p, buf, grads
