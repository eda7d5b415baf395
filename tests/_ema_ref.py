"""The weight EMA restated in torch on the CPU, one rounding per operation: what csrc/ema.hip must reproduce bit for bit.

    e <- e + omd * (p - e)   as   e.add_((p - e).mul_(omd))   -- a subtract, a multiply, then an add, each rounded to fp32
    mirror = p.to(torch.bfloat16)                               -- round to nearest even
    d(t) = min(decay, (1 + t) / (10 + t))  (warm-up)  or  decay;  omd = float32(1 - d)

Never ``add_(..., alpha=)`` or ``lerp_``: either may evaluate a fused multiply-add.
"""
import torch


def decay_at(t, decay=0.9999, warmup=True):
    """The decay of the update that follows t earlier ones, in double."""
    return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)


def omd32(decay):
    """float32(1 - decay) as a Python float (exactly representable in fp32)."""
    return torch.tensor(1.0 - float(decay), dtype=torch.float64).to(torch.float32).item()


def update_(e, p, omd):
    """In place on e (CPU, fp32); p is left alone.  omd: a Python float that is an fp32 value (omd32)."""
    assert e.dtype == p.dtype == torch.float32 and not e.is_cuda and not p.is_cuda
    assert torch.tensor(omd, dtype=torch.float32).item() == omd, "omd must already be an fp32 value"
    t = p - e
    t.mul_(omd)
    return e.add_(t)


def mirror(p):
    return p.to(torch.bfloat16)


def fold_(avg, live, omd):
    """One update of a whole state dict `avg` (CPU tensors) towards `live`: floating-point entries by update_, integer
    ones (num_batches_tracked) take the live value."""
    assert set(avg) == set(live)
    for k, v in live.items():
        v = v.detach().cpu()
        if v.is_floating_point():
            update_(avg[k], v.contiguous(), omd)
        else:
            avg[k] = v.clone()
    return avg
