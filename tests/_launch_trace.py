"""Recording the launches an engine makes: every nbdt.ops entry point named in SPEC is wrapped by attribute while a
Recorder is active (the engines call them as ops.<name> at call time).  Shared by the schedule tests.

One recorded launch is (op, buffer, extra):
  buffer  the name (first element of its engine._bufs key) of the launch's output -- for the BatchNorm statistics
          launches, whose outputs are [C] vectors, of the tensor they reduce; for weight gradients the parameter's name;
  extra   conv_igemm / conv_pw / conv_igemm_multi / conv_igemm_bnbwd: desc.accumulate; conv_igemm_affine: (act, residual);
          bn_apply: (relu, residual); bn_bwd: g_resid; bn_bwd_fused: cus > 0; bn_bwd_cus: gx_add; bn_apply_s2d: relu;
          conv_wgrad: cu_budget > 0; else None.
"ConvSeg" is a launch of a slice list (ops.ConvSeg.__call__, wrapped on the class)."""
import inspect

import torch

from nbdt import ops


def _acc(a):
    d = a["descs"][0] if "descs" in a else a["desc"]
    return bool(d.accumulate)


# op -> (the argument that names the launch, extra(bound arguments))
SPEC = {
    "stem_conv": ("out", None),
    "conv_igemm": ("out", _acc),
    "conv_pw": ("out", _acc),
    "conv_igemm_multi": ("out", _acc),
    "conv_igemm_bnbwd": ("out", _acc),
    "conv_igemm_affine": ("out", lambda a: (a["act"], a["residual"])),
    "bn_stats": ("x", None),
    "bn_finalize": ("x", None),
    "bn_apply": ("y", lambda a: (bool(a["relu"]), a["residual"])),
    "bn_apply_s2d": ("y", lambda a: bool(a["relu"])),
    "bn_bwd": ("gx", lambda a: a["g_resid"]),
    "bn_bwd_fused": ("gx", lambda a: a["cus"] > 0),
    "bn_bwd_cus": ("gx", lambda a: a["gx_add"]),
    "conv_wgrad": ("dw", lambda a: a["cu_budget"] > 0),
    "pool_bn_bwd": ("gx", None),
    "pool_bn_bwd_apply": ("gx", None),
    "stem_wgrad": ("dw", None),
    "bn_relu_pool": ("pooled", None),
    "linear_fwd": ("z", None),
    "linear_bwd": ("gx", None),
    "ConvSeg": ("out", None),
}


def _holder(op):
    """(object, attribute) the entry point `op` is looked up on at call time."""
    return (ops.ConvSeg, "__call__") if op == "ConvSeg" else (ops, op)


class Recorder:
    """Wraps the SPEC entry points of nbdt.ops while active.  `trace`: [(op, buffer, extra)]; `side`: [bool] and `reads`:
    [names of the engine buffers the launch was given besides its output], index for index."""

    def __init__(self, eng):
        self.eng, self.raw, self.real, self.depth = eng, [], {}, 0

    def _wrap(self, op):
        real = self.real[op]
        sig = inspect.signature(real)
        key, extra = SPEC[op]

        def f(*a, **k):
            if self.depth == 0:
                b = sig.bind(*a, **k)
                b.apply_defaults()
                args = b.arguments
                side = torch.cuda.current_stream(self.eng.device) == self.eng._side
                others = [v for n, v in args.items() if n != key and isinstance(v, torch.Tensor)]
                if op == "ConvSeg":
                    others += list(args["ins"])       # (a slice list's input tensors)
                self.raw.append((op, args[key], side, extra(args) if extra else None, others))
            self.depth += 1
            try:
                return real(*a, **k)
            finally:
                self.depth -= 1
        return f

    def __enter__(self):
        for op in SPEC:
            obj, attr = _holder(op)
            self.real[op] = getattr(obj, attr)
            setattr(obj, attr, self._wrap(op))
        return self

    def __exit__(self, *exc):
        for op, real in self.real.items():
            setattr(*_holder(op), real)
        eng = self.eng
        names = {t.data_ptr(): k[0] for k, t in eng._bufs.items()}
        grad0 = eng.store.grad.data_ptr()
        params = {grad0 + 4 * off: name for name, (off, _) in eng.store.entries.items()}

        def name(v, table):
            return table.get(v.data_ptr()) if isinstance(v, torch.Tensor) else v

        self.trace, self.side, self.reads = [], [], []
        for op, out, side, extra, others in self.raw:
            out = name(out, params if op in ("conv_wgrad", "stem_wgrad") else names)
            assert out is not None, f"{op}: output is neither an engine buffer nor a parameter gradient"
            if isinstance(extra, tuple):
                extra = tuple(name(v, names) for v in extra)
            self.trace.append((op, out, name(extra, names)))
            self.side.append(side)
            self.reads.append({names[t.data_ptr()] for t in others if t.data_ptr() in names})
