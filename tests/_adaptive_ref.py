"""Two references of nbdt_adamw_step / nbdt_rmsprop_step (include/nbdt_hip.h) for tests/test_adaptive*.py.

``Fp32Ref`` restates the header in numpy float32: one array operation per IEEE operation, so one rounding each, the host
scalars formed in double from the fp32 arguments and rounded once.  The kernels are compared with it bit for bit.

``Fp64Oracle`` is ``torch.optim.AdamW`` / ``torch.optim.RMSprop`` on double tensors, one parameter (and one param group,
for its decay) per segment, ``grad_scale`` applied to the gradient; TensorFlow's RMSprop is written out from its formula,
because no library here has it.  The restatement is compared with it to a derived tolerance.

Both take segment rows (offset, length, weight_decay[, ...]) and leave everything outside the segments alone."""
import math

import numpy as np
import torch

f32 = np.float32


def host_scalars(lr, beta1, beta2, alpha, t):
    """The derived fp32 scalars as the header forms them: double arithmetic on the fp32 arguments, one rounding."""
    lr, b1, b2, a = (float(f32(x)) for x in (lr, beta1, beta2, alpha))
    return dict(omb1=f32(1.0 - b1), omb2=f32(1.0 - b2), oma=f32(1.0 - a),
                ss=f32(lr / (1.0 - math.pow(b1, float(t)))), c2=f32(math.sqrt(1.0 - math.pow(b2, float(t)))))


class Fp32Ref:
    """p, s1 (m / momentum buffer), s2 (v / mean square): float32 numpy copies of flat tensors."""

    def __init__(self, p, s1, s2, segments):
        self.segments = [(int(r[0]), int(r[1]), float(r[2])) for r in segments]
        self.p, self.s1, self.s2 = (np.array(x.detach().cpu().numpy(), dtype=f32, copy=True) for x in (p, s1, s2))

    def adamw(self, g, lr, betas, eps, t, grad_scale=1.0):
        g = g.detach().cpu().numpy().astype(f32)
        c = host_scalars(lr, betas[0], betas[1], 0.0, t)
        lr, b1, b2, eps, gsc = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps), f32(grad_scale)
        for o, l, wd in self.segments:
            s = slice(o, o + l)
            gs = gsc * g[s]
            k = f32(1.0) - lr * f32(wd)
            p1 = self.p[s] * k
            m = b1 * self.s1[s] + c["omb1"] * gs
            v = b2 * self.s2[s] + (c["omb2"] * gs) * gs
            d = np.sqrt(v) / c["c2"] + eps
            self.p[s], self.s1[s], self.s2[s] = p1 - c["ss"] * (m / d), m, v
        for x in (self.p, self.s1, self.s2):
            assert x.dtype == f32

    def rmsprop(self, g, lr, alpha, eps, momentum, tf=False, grad_scale=1.0):
        g = g.detach().cpu().numpy().astype(f32)
        oma = host_scalars(lr, 0.0, 0.0, alpha, 1)["oma"]
        lr, alpha, eps, mu, gsc = f32(lr), f32(alpha), f32(eps), f32(momentum), f32(grad_scale)
        for o, l, wd in self.segments:
            s = slice(o, o + l)
            p, buf, sq = self.p[s], self.s1[s], self.s2[s]
            gs = gsc * g[s]
            gs = gs + f32(wd) * p
            if tf:
                sq = sq + oma * (gs * gs - sq)
                a = np.sqrt(sq + eps)
                buf = mu * buf + lr * (gs / a)
                p = p - buf
            else:
                sq = alpha * sq + (oma * gs) * gs
                a = np.sqrt(sq) + eps
                if mu != 0:
                    buf = mu * buf + gs / a
                    p = p - lr * buf
                else:                      # the buffer is neither read nor written
                    p = p - lr * (gs / a)
            self.p[s], self.s1[s], self.s2[s] = p, buf, sq
        for x in (self.p, self.s1, self.s2):
            assert x.dtype == f32


class Fp64Oracle:
    """kind: "adamw" | "rmsprop" | "rmsprop_tf".  hp: betas / alpha, eps, momentum as the fp32 values the kernel is
    given (float(np.float32(x))), so that the two references differ by rounding alone."""

    def __init__(self, kind, p, s1, s2, segments, **hp):
        self.kind, self.hp = kind, {k: (tuple(float(f32(b)) for b in v) if isinstance(v, tuple) else float(f32(v)))
                                    for k, v in hp.items()}
        self.segments = [(int(r[0]), int(r[1]), float(f32(r[2]))) for r in segments]
        self.p, self.s1, self.s2 = (x.detach().cpu().double().clone() for x in (p, s1, s2))
        self.t = 0
        if kind == "rmsprop_tf":
            return
        self.params = [torch.nn.Parameter(self.p[o:o + l].clone()) for o, l, _ in self.segments]
        groups = [{"params": [q], "weight_decay": wd} for q, (_, _, wd) in zip(self.params, self.segments)]
        if kind == "adamw":
            self.opt = torch.optim.AdamW(groups, lr=1.0, betas=self.hp["betas"], eps=self.hp["eps"], amsgrad=False)
        else:
            self.opt = torch.optim.RMSprop(groups, lr=1.0, alpha=self.hp["alpha"], eps=self.hp["eps"],
                                           momentum=self.hp["momentum"], centered=False)
        for q, (o, l, _) in zip(self.params, self.segments):     # the state the arenas start with
            st = self.opt.state[q]
            st["step"] = torch.tensor(0.0)
            if kind == "adamw":
                st["exp_avg"], st["exp_avg_sq"] = self.s1[o:o + l].clone(), self.s2[o:o + l].clone()
            else:
                st["square_avg"] = self.s2[o:o + l].clone()
                if self.hp["momentum"] > 0:
                    st["momentum_buffer"] = self.s1[o:o + l].clone()

    def step(self, g, lr, grad_scale=1.0):
        """One step on the flat gradient g.  Returns the largest |change of p|."""
        lr, gsc = float(f32(lr)), float(f32(grad_scale))
        g = g.detach().cpu().double()
        before = self.p.clone()
        self.t += 1
        if self.kind == "rmsprop_tf":
            a_, eps, mu = self.hp["alpha"], self.hp["eps"], self.hp["momentum"]
            for o, l, wd in self.segments:
                s = slice(o, o + l)
                gs = gsc * g[s] + wd * self.p[s]
                self.s2[s] = self.s2[s] + (1.0 - a_) * (gs * gs - self.s2[s])
                self.s1[s] = mu * self.s1[s] + lr * gs / torch.sqrt(self.s2[s] + eps)
                self.p[s] = self.p[s] - self.s1[s]
        else:
            for group in self.opt.param_groups:
                group["lr"] = lr
            for q, (o, l, _) in zip(self.params, self.segments):
                q.grad = gsc * g[o:o + l]
            self.opt.step()
            for q, (o, l, _) in zip(self.params, self.segments):
                st = self.opt.state[q]
                self.p[o:o + l] = q.detach()
                if self.kind == "adamw":
                    self.s1[o:o + l], self.s2[o:o + l] = st["exp_avg"], st["exp_avg_sq"]
                else:
                    self.s2[o:o + l] = st["square_avg"]
                    if self.hp["momentum"] > 0:
                        self.s1[o:o + l] = st["momentum_buffer"]
        return (self.p - before).abs().max().item()


def mirror(p):
    """bf16(p), round to nearest even: what the step writes into the bf16 mirror."""
    return torch.as_tensor(p).to(torch.bfloat16)


def ragged_table(item, seed=0):
    """The ragged table of the GPU tests: lengths 1, 3, 4, 5, 8, 1000 and one segment of 2 * item + 5 elements (three
    items, the last one with a scalar tail), gaps of 4-11 elements between the rows and after the last one, a different
    decay per row.  Returns (n, rows (offset, length, decay), p, buf, [g of step 0, 1, 2]) as float32 tensors: sentinel
    7.0 in the gaps of p and buf, random gradients everywhere (the gaps' must not be read)."""
    lengths = [1, 3, 4, 5, 8, 1000, 2 * item + 5]
    rows, off = [], 0
    for i, l in enumerate(lengths):
        rows.append((off, l, 1e-3 * (i + 1)))
        off = (off + l + 4 + 4 * (i % 2) + 3) // 4 * 4
    n = off
    gen = torch.Generator().manual_seed(seed)
    p, buf = torch.full((n,), 7.0), torch.full((n,), 7.0)
    for o, l, _ in rows:
        p[o:o + l] = 0.5 * torch.randn(l, generator=gen)
        buf[o:o + l] = 0.1 * torch.randn(l, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(3)]
    return n, rows, p, buf, grads


def start_state(kind, n, segments, buf):
    """(s1, s2) the tests start an arena with: sentinel 7.0 outside the segments; inside, AdamW starts m = v = 0 (its own
    start: with another m the first bias-corrected step is not bounded by lr), torch's RMSprop the given buffer and a
    mean square of 0.25 (a start at 0 makes the first step lr * sign(gs) / sqrt(1 - alpha), which no tolerance can follow
    through gs = 0), TensorFlow's the given buffer and 1."""
    s1, s2 = buf.clone().float(), torch.full((n,), 7.0)
    for r in segments:
        o, l = int(r[0]), int(r[1])
        s2[o:o + l] = {"adamw": 0.0, "rmsprop": 0.25, "rmsprop_tf": 1.0}[kind]
        if kind == "adamw":
            s1[o:o + l] = 0.0
    return s1, s2
