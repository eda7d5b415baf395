"""EfficientNet execution engine: B0 (SURVEY.md row A4 / BASELINE config 5) and, scaled by ``efficientnet_config``, B1 .. B7
and the TF-padded b0b .. b7b, at any image side >= 32.

Restates pytorchcv's ``efficientnet_b0`` .. ``efficientnet_b7b`` (the models the reference re-exports at
nbdt/models/__init__.py:3 and names in README.md:141-151) as a fixed launch sequence over the HIP
kernels: 1x1 expand / project convolutions are the implicit-GEMM kernels (csrc/conv_dma.hip) with the
following BatchNorm's statistics fused into their epilogue; depthwise convolutions, BatchNorm + swish,
squeeze-and-excitation and dropout are the streaming kernels of csrc/effnet.hip.  State-dict names and
logical shapes follow pytorchcv (``features.stageS.unitU.{conv1,conv2,se,conv3}``,
``features.final_block``, ``output.fc``).

Per MBConv unit the forward keeps only raw conv outputs + the tensors the next conv must read
(e_raw, e_act, d_raw, d_se, p_raw, out); the swish / SE-scaled activations needed by the backward are
recomputed from the raw outputs inside the backward kernels.
"""
import math

import torch

from nbdt import ops
from nbdt.engine import _Engine, _pad32, side_stream

# (stage stride, [(out_channels, kernel, expansion), ...]) -- pytorchcv get_efficientnet(version="b0")
B0_STAGES = [
    (1, [(16, 3, 1)]),
    (2, [(24, 3, 6), (24, 3, 6)]),
    (2, [(40, 5, 6), (40, 5, 6)]),
    (2, [(80, 3, 6)] * 3 + [(112, 5, 6)] * 3),
    (2, [(192, 5, 6)] * 4 + [(320, 3, 6)]),
]
ACT = ops.ACT_SWISH

# pytorchcv get_efficientnet: the B0 groups, and per version (width factor, depth factor, native input size, dropout rate)
_BASE_LAYERS = [1, 2, 2, 3, 3, 4, 1]
_BASE_CHANNELS = [16, 24, 40, 80, 112, 192, 320]
_BASE_EXPANSION = [1, 6, 6, 6, 6, 6, 6]
_BASE_KERNEL = [3, 3, 5, 3, 5, 5, 3]
_BASE_STRIDE = [1, 2, 2, 2, 1, 2, 1]          # of a group's first unit
EFFNET_SCALING = {
    "b0": (1.0, 1.0, 224, 0.2), "b1": (1.0, 1.1, 240, 0.2), "b2": (1.1, 1.2, 260, 0.3), "b3": (1.2, 1.4, 300, 0.3),
    "b4": (1.4, 1.8, 380, 0.4), "b5": (1.6, 2.2, 456, 0.4), "b6": (1.8, 2.6, 528, 0.5), "b7": (2.0, 3.1, 600, 0.5),
}


def round_channels(c, divisor=8):
    """pytorchcv round_channels: the nearest multiple of 8, never more than 10 % below c."""
    r = max(int(c + divisor / 2.0) // divisor * divisor, divisor)
    if float(r) < 0.9 * c:
        r += divisor
    return r


def efficientnet_config(version, tf_mode=False):
    """What EfficientNetEngine needs to build pytorchcv's efficientnet_<version> (tf_mode: the `b` names, e.g. b7b):
    {"stages": in the shape of B0_STAGES, "init_channels", "final_channels", "dropout_rate", "in_size", "bn_eps",
    "tf_mode"}.  Depth scales a group's unit count by ceil, width its channels by round_channels (the final block only when
    width > 1); a group whose first unit has stride 1 continues the previous stage (except the first), which fixes the
    stage / unit numbers and so the state_dict keys.  tf_mode changes the padding rule (ops.conv_padding(same=True)) and the
    BatchNorm eps (1e-3 instead of 1e-5), nothing else."""
    if version not in EFFNET_SCALING:
        raise ValueError(f"unknown EfficientNet version {version!r}: one of {sorted(EFFNET_SCALING)}")
    width, depth, in_size, dropout = EFFNET_SCALING[version]
    stages = []
    for n, c, e, k, s in zip(_BASE_LAYERS, _BASE_CHANNELS, _BASE_EXPANSION, _BASE_KERNEL, _BASE_STRIDE):
        units = [(round_channels(c * width), k, e)] * int(math.ceil(n * depth))
        if s != 1 or not stages:
            stages.append((s, units))
        else:
            stages[-1] = (stages[-1][0], stages[-1][1] + units)
    return {"stages": stages, "init_channels": round_channels(32 * width),
            "final_channels": round_channels(1280 * width) if width > 1.0 else 1280, "dropout_rate": dropout,
            "in_size": in_size, "bn_eps": 1e-3 if tf_mode else 1e-5, "tf_mode": bool(tf_mode)}


def efficientnet_layout(config, num_classes=1000):
    """[(state_dict key, logical shape)] of the parameters of the model `config` describes, in pytorchcv's module order
    -- derived from the configuration alone (no device): what an engine built from it exposes, and what a checkpoint
    of pytorchcv's model holds.  BatchNorm contributes .weight and .bias (buffers are not listed)."""
    out = []

    def conv(name, cout, cin, k):
        out.append((name + ".conv.weight", (cout, cin, k, k)))
        out.extend([(name + ".bn.weight", (cout,)), (name + ".bn.bias", (cout,))])

    def se(name, c, mid):
        out.extend([(name + ".conv1.weight", (mid, c, 1, 1)), (name + ".conv1.bias", (mid,)),
                    (name + ".conv2.weight", (c, mid, 1, 1)), (name + ".conv2.bias", (c,))])

    cin = config["init_channels"]
    conv("features.init_block.conv", cin, 3, 3)
    for i, (_, specs) in enumerate(config["stages"]):
        for j, (cout, k, exp) in enumerate(specs):
            pre, mid = f"features.stage{i + 1}.unit{j + 1}.", cin * exp
            if i == 0:
                conv(pre + "dw_conv", mid, 1, k)
                se(pre + "se", mid, mid // 4)
                conv(pre + "pw_conv", cout, mid, 1)
            else:
                conv(pre + "conv1", mid, cin, 1)
                conv(pre + "conv2", mid, 1, k)
                se(pre + "se", mid, mid // (4 * exp))
                conv(pre + "conv3", cout, mid, 1)
            cin = cout
    out.append(("features.final_block.conv.weight", (config["final_channels"], cin, 1, 1)))
    out.extend([("features.final_block.bn.weight", (config["final_channels"],)),
                ("features.final_block.bn.bias", (config["final_channels"],))])
    out.extend([("output.fc.weight", (num_classes, config["final_channels"])), ("output.fc.bias", (num_classes,))])
    return out


class DepthwiseConv:
    """groups=C Conv2d(k, stride, padding=k//2), bias-free; master weights fp32 [k*k][Cpad]."""

    def __init__(self, store, name, c_real, k, stride, gen, same=False):
        self.store, self.name, self.c_real, self.k, self.stride = store, name, c_real, k, stride
        self.same = same            # TF "SAME" padding (ops.conv_padding) instead of the symmetric k // 2
        self.C = _pad32(c_real)
        bound = math.sqrt(2.0) * math.sqrt(3.0 / (k * k))   # kaiming_uniform_(a=0), fan_in = k*k

        def init(v):
            v.zero_()
            v[:, :c_real].uniform_(-bound, bound, generator=gen)

        store.add(name, (k * k, self.C), init)
        self.side_stream = None     # the engine's second stream for weight gradients, or None: the caller's

    def logical(self, buf):
        v = self.store._view(buf, self.name).view(self.k, self.k, self.C)
        return v[:, :, :self.c_real].permute(2, 0, 1).unsqueeze(1)      # [C, 1, k, k]

    def pad(self, hw):
        """None: the launches without a padding argument (padding k // 2, extents the stride divides -- every B0 layer at
        a multiple of 32); else (top, left) for the input extents hw."""
        h, w = hw
        if self.stride == 1 or (not self.same and h % 2 == 0 and w % 2 == 0):
            return None
        return (ops.conv_padding(h, self.k, self.stride, self.same)[0],
                ops.conv_padding(w, self.k, self.stride, self.same)[0])

    def forward(self, x, y, bn_scratch=None):
        ops.dwconv_fwd(x, self.store.p(self.name), y, self.k, self.stride, bn_scratch,
                       pad=self.pad((x.shape[1] - 2, x.shape[2] - 2)))

    def backward_data(self, gy, gx, bn=None, bn_x=None):
        """bn/bn_x: `gx` is dL/d(swish(bn(bn_x))) -- also leave that BatchNorm's backward sums in its owner's slots
        (stride 1 only; follow with bn.act_backward_apply)."""
        if bn is not None:
            assert self.stride == 1
            bn.dwconv_backward_data(gy, self.store.p(self.name), gx, self.k, bn_x)
            return
        ops.dwconv_bwd_data(gy, self.store.p(self.name), gx, self.k, self.stride,
                            pad=self.pad((gx.shape[1] - 2, gx.shape[2] - 2)))

    def backward_weight(self, x, gy, also):
        """also: a further launch that only feeds the optimizer (the SE block's parameter gradients), issued behind the
        weight gradient on the same stream -- one cross-stream dependency for both."""
        side = self.side_stream
        pad = self.pad((x.shape[1] - 2, x.shape[2] - 2))
        if side is None:
            ops.dwconv_bwd_weight(x, gy, self.store.g(self.name), self.k, self.stride, pad=pad)
            also()
            return
        side.wait_stream(torch.cuda.current_stream(x.device))     # second stream: see WRNEngine
        with torch.cuda.stream(side):
            ops.dwconv_bwd_weight(x, gy, self.store.g(self.name), self.k, self.stride, pad=pad)
            also()


class SqueezeExcite:
    """pytorchcv SEBlock: two biased 1x1 convs on the pooled vector (swish, sigmoid)."""

    def __init__(self, store, name, c_real, mid, gen):
        self.store, self.name, self.c_real, self.mid = store, name, c_real, mid
        b1 = math.sqrt(2.0) * math.sqrt(3.0 / c_real)
        b2 = math.sqrt(2.0) * math.sqrt(3.0 / mid)
        store.add(name + ".conv1.weight", (mid, c_real), lambda v: v.uniform_(-b1, b1, generator=gen))
        store.add(name + ".conv1.bias", (mid,), lambda v: v.zero_())
        store.add(name + ".conv2.weight", (c_real, mid), lambda v: v.uniform_(-b2, b2, generator=gen))
        store.add(name + ".conv2.bias", (c_real,), lambda v: v.zero_())

    def views(self, buf):
        s, n = self.store, self.name
        return {
            n + ".conv1.weight": s._view(buf, n + ".conv1.weight").view(self.mid, self.c_real, 1, 1),
            n + ".conv1.bias": s._view(buf, n + ".conv1.bias"),
            n + ".conv2.weight": s._view(buf, n + ".conv2.weight").view(self.c_real, self.mid, 1, 1),
            n + ".conv2.bias": s._view(buf, n + ".conv2.bias"),
        }

    def forward(self, pooled, pre1, gate):
        p = self.store.p
        ops.se_gate_fwd(pooled, p(self.name + ".conv1.weight"), p(self.name + ".conv1.bias"),
                        p(self.name + ".conv2.weight"), p(self.name + ".conv2.bias"), pre1, gate, self.c_real)

    def backward(self, dgate, gate, pre1, pooled, dpre2, dpre1, gpool):
        """The data part only; returns the launch of the parameter gradients for the caller to place (they read
        dpre2 / dpre1 / pre1 / pooled and feed nothing but the optimizer)."""
        p, g = self.store.p, self.store.g
        grads = (g(self.name + ".conv1.weight"), g(self.name + ".conv1.bias"), g(self.name + ".conv2.weight"),
                 g(self.name + ".conv2.bias"))
        ops.se_gate_bwd(dgate, gate, pre1, pooled, p(self.name + ".conv1.weight"), p(self.name + ".conv2.weight"),
                        dpre2, dpre1, gpool, None, None, None, None, self.c_real)
        return lambda: ops.se_param_grad(dpre2, dpre1, pre1, pooled, *grads, self.c_real)


class EfficientNetEngine(_Engine):
    def __init__(self, num_classes=1000, dropout_rate=0.2, stages=B0_STAGES, init_channels=32,
                 final_channels=1280, device="cuda", seed=0, stochastic_depth_prob=0.0, bn_eps=1e-5, tf_mode=False):
        """stages / init_channels / final_channels / dropout_rate / bn_eps / tf_mode: efficientnet_config(version,
        tf_mode) names them all (EfficientNetEngine.from_config); the defaults are B0."""
        super().__init__(device, seed)
        self.num_classes, self.dropout_rate = num_classes, float(dropout_rate)
        self.bn_eps, self.tf_mode = float(bn_eps), bool(tf_mode)
        if len(stages) != 5 or len(stages[2][1]) < 1 or sum(len(sp) for _, sp in stages) > ops._C.NBDT_SD_MAX_UNITS:
            raise ValueError("EfficientNetEngine takes five stages and at most %d units" % ops._C.NBDT_SD_MAX_UNITS)
        gen = self.gen
        self.stem_c = init_channels
        b0 = math.sqrt(2.0) * math.sqrt(3.0 / 27)
        self.store.add("features.init_block.conv.conv.weight", (init_channels, 3, 3, 3),
                       lambda v: v.uniform_(-b0, b0, generator=gen))
        self.bn0 = self.bn("features.init_block.conv.bn", init_channels)
        self.units, self.dws, self.ses = [], [], []
        cin = init_channels
        for i, (stage_stride, specs) in enumerate(stages):
            for j, (cout, k, exp) in enumerate(specs):
                stride = stage_stride if j == 0 else 1
                pre = f"features.stage{i + 1}.unit{j + 1}."
                mid = cin * exp
                u = {"cin": cin, "cout": cout, "mid": mid, "k": k, "stride": stride, "exp": exp,
                     "key": f"s{i + 1}u{j + 1}", "stage": i + 1, "residual": cin == cout and stride == 1,
                     "index": len(self.units)}
                if i == 0:   # EffiDwsConvUnit: depthwise -> SE -> pointwise
                    u["conv1"] = u["bn1"] = None
                    u["dw"] = DepthwiseConv(self.store, pre + "dw_conv.conv.weight", mid, k, stride, gen, self.tf_mode)
                    u["bn2"] = self.bn(pre + "dw_conv.bn", mid)
                    u["se"] = SqueezeExcite(self.store, pre + "se", mid, mid // 4, gen)
                    u["conv3"] = self.conv(pre + "pw_conv.conv.weight", mid, cout, 1, 1)
                    u["bn3"] = self.bn(pre + "pw_conv.bn", cout)
                else:        # EffiInvResUnit: expand -> depthwise -> SE -> project
                    u["conv1"] = self.conv(pre + "conv1.conv.weight", cin, mid, 1, 1)
                    u["bn1"] = self.bn(pre + "conv1.bn", mid)
                    u["dw"] = DepthwiseConv(self.store, pre + "conv2.conv.weight", mid, k, stride, gen, self.tf_mode)
                    u["bn2"] = self.bn(pre + "conv2.bn", mid)
                    u["se"] = SqueezeExcite(self.store, pre + "se", mid, mid // (exp * 4), gen)
                    u["conv3"] = self.conv(pre + "conv3.conv.weight", mid, cout, 1, 1)
                    u["bn3"] = self.bn(pre + "conv3.bn", cout)
                self.dws.append(u["dw"])
                self.ses.append(u["se"])
                self.units.append(u)
                cin = cout
        self.final_conv = self.conv("features.final_block.conv.weight", cin, final_channels, 1, 1)
        self.final_bn = self.bn("features.final_block.bn", final_channels)
        self.feat_c = final_channels
        kb = 1.0 / math.sqrt(final_channels)
        self.store.add("output.fc.weight", (num_classes, final_channels), lambda v: v.uniform_(-kb, kb, generator=gen))
        self.store.add("output.fc.bias", (num_classes,), lambda v: v.uniform_(-kb, kb, generator=gen))
        self.finalize()
        self._step = 0
        self.dropout_seed = seed
        self._se_sums_dirty = set()    # ids of the one-pass SE sums a backward has summed into and not yet re-zeroed
        self._side = side_stream(self.device)     # weight gradients on the process's second stream (see WRNEngine)
        for c in self.convs + self.dws:
            c.side_stream = self._side
        self.sd_seed = seed            # stochastic depth: the draw hashes (sd_seed, sd_stream, sd_counter, unit, image)
        self.sd_counter = 0            # the counter the NEXT training forward draws with; not saved: a resumed run restarts it
        self._sd_rows = None           # the [units, B] table the last forward drew (None: it drew none) -- what backward reads
        self.set_stochastic_depth(stochastic_depth_prob)

    @classmethod
    def from_config(cls, config, **kwargs):
        """An engine from efficientnet_config(version, tf_mode); keywords override (dropout_rate, num_classes, ...)."""
        args = {k: config[k] for k in ("stages", "init_channels", "final_channels", "dropout_rate", "bn_eps", "tf_mode")}
        args.update(kwargs)
        return cls(**args)

    def _stem_pad(self, H, W):
        """(top, left) of the 3x3/2 stem, or None for the launch without a padding argument (see DepthwiseConv.pad)."""
        if not self.tf_mode and H % 2 == 0 and W % 2 == 0:
            return None
        return (ops.conv_padding(H, 3, 2, self.tf_mode)[0], ops.conv_padding(W, 3, 2, self.tf_mode)[0])

    def _add(self, a, b, out):
        """out = a + b on padded tensors of one shape, as the BatchNorm + residual pass with the identity transform
        (x * 1 + 0 is exact): the skip gradient of a stage-1 unit, which has no expand convolution to accumulate it."""
        C = a.shape[3]
        if ("ident", C) not in self._bufs:
            self._bufs[("ident", C)] = (torch.zeros(C, device=self.device), torch.ones(C, device=self.device))
        zero, one = self._bufs[("ident", C)]
        ops.bn_act_apply(a, zero, one, one, zero, out, act=ops.ACT_NONE, residual=b)

    def set_stochastic_depth(self, prob, stream=0):
        """torchvision's StochasticDepth(p, mode="row") on every unit with a skip connection: in training, image b of unit
        i (0-based over ALL units) loses its branch with probability prob * i / len(units) and keeps it scaled by
        1 / (1 - p_i) otherwise; evaluation never changes.  0 <= prob < 1, 0 switches it off.  stream: an id mixed into
        the draw (main.py passes the rank, so the ranks of a data-parallel run drop different images)."""
        flags = [u["residual"] for u in self.units]
        self._sd_prob, self._sd_scale = ops.stochastic_depth_probs(prob, len(flags), flags)     # raises outside [0, 1)
        self.stochastic_depth_prob, self.sd_stream = float(prob), int(stream)

    # ------------------------------------------------------------------ reference-named views
    def extra_param_views(self, buf):
        out = {
            "features.init_block.conv.conv.weight":
                self.store._view(buf, "features.init_block.conv.conv.weight").permute(0, 3, 1, 2),
            "output.fc.weight": self.store._view(buf, "output.fc.weight"),
            "output.fc.bias": self.store._view(buf, "output.fc.bias"),
        }
        for d in self.dws:
            out[d.name] = d.logical(buf)
        for s in self.ses:
            out.update(s.views(buf))
        return out

    def grad_buckets(self):
        """Flat-gradient ranges in the order backward completes them: [stage5..classifier], [stage3..4],
        [stem..stage2]."""
        ent = self.store.entries
        s3 = ent["features.stage3.unit1.conv1.conv.weight"][0]
        s5 = ent["features.stage5.unit1.conv1.conv.weight"][0]
        return [(s5, self.store.grad.numel()), (s3, s5), (0, s3)]

    bucket_units = ("s5u1", "s3u1")

    def _vec(self, key, B, n):
        return self._tensor(key, (B, n))

    def algorithmic_bytes(self, B, size):
        """HBM bytes one training step of THIS schedule has to move if every pass reads each of its input tensors once and
        writes each output once (bf16 activations / gradients, padded channel counts; weights, statistics and the [B, C]
        vectors of the SE branch are noise and left out).  What bench.py prices EfficientNet-B0 against: round 4 used
        2 x the resident buffers (12.6 GB at 128 x 224 x 224), which ignores that backward re-reads every stored
        activation and that several passes read two tensors -- the PMC counters said 36 GB.  Per unit, with X / E / D / O
        the unit's input, expanded (before the depthwise conv), depthwise-output and output tensors:
          forward   expand conv X + E | BatchNorm + swish 2E | depthwise E + D | squeeze D | scale 2D | project D + O |
                    BatchNorm (+ skip) 2O (+ X)
          backward  bn3 5O | project weight gradient D + O, data gradient O + D | dL/dgate + bn2's sums 2D (one pass) |
                    bn2 + SE elementwise 3D | depthwise
                    weight gradient E + D, data gradient + bn1 sums D + 2E | bn1 elementwise 3E | expand weight gradient
                    X + E, data gradient E + X (+ X when it accumulates onto the skip gradient)"""
        h = w = ops.conv_out_size(size, 2)
        e = lambda hh, ww, c: 2 * B * hh * ww * _pad32(c)       # bytes of one bf16 tensor
        stem = e(h, w, self.stem_c)
        total = 12 * B * size * size + 2 * stem + 2 * stem      # image in, stem conv out, BatchNorm + swish (read + write)
        total += 5 * stem + 12 * B * size * size + stem         # backward of that BatchNorm, stem weight gradient
        for u in self.units:
            s = u["stride"]
            ho, wo = ops.conv_out_size(h, s), ops.conv_out_size(w, s)
            X, O = e(h, w, u["cin"]), e(ho, wo, u["cout"])
            E, D = e(h, w, u["mid"]), e(ho, wo, u["mid"])
            res = X if u["residual"] else 0
            if u["conv1"] is not None:
                fwd = (X + E) + 2 * E + (E + D) + D + 2 * D + (D + O) + 2 * O + res
                bwd = 5 * O + (D + O) + (O + D) + 2 * D + 3 * D + (E + D) + (D + 2 * E) + 3 * E + (X + E) + (E + X) + res
            else:       # stage 1: depthwise on the unit's input, no expand conv
                fwd = (X + D) + D + 2 * D + (D + O) + 2 * O + res
                bwd = 5 * O + (D + O) + (O + D) + 2 * D + 3 * D + (X + D) + (D + X) + 3 * res   # (+ the skip gradient's add)
            total += fwd + bwd
            h, w = ho, wo
        F, L = e(h, w, self.feat_c), e(h, w, self.units[-1]["cout"])
        total += (L + F) + F                                    # final conv, BatchNorm + swish + pool (reads only)
        total += 4 * F + F + (L + F) + (F + L)                  # its backward (pool form: no gradient tensor read), conv grads
        return int(total)

    # ------------------------------------------------------------------ forward
    def forward(self, img, training=None):
        training = self.training if training is None else training
        if img.shape[2] < 32 or img.shape[3] < 32:
            raise ValueError("EfficientNet input sides must be at least 32")
        img = self._input(img)
        B, _, H, W = img.shape
        fuse = training and self.fuse_stats
        h, w = ops.conv_out_size(H, 2), ops.conv_out_size(W, 2)
        c0 = _pad32(self.stem_c)
        t0 = self.buf("t0", B, h, w, c0)
        x = self.buf("a0", B, h, w, c0)
        ops.stem_conv(img, self.store.p("features.init_block.conv.conv.weight"), t0, self.stem_c, stride=2,
                      pad=self._stem_pad(H, W))
        self.bn0.stats(t0, training)
        self.bn0.act_apply(t0, x, act=ACT)
        self._sd_rows = None
        if training and self.stochastic_depth_prob > 0.0:
            # ONE launch draws every unit's per-image factors; a unit's row rides in the residual add it already makes
            # and in bn3's backward.  Like _mask, the table is what this forward's backward reads.
            self._sd_rows = self._tensor("sd_rows", (len(self.units), B))
            ops.stochastic_depth_draw(self._sd_rows, self._sd_prob, self._sd_scale, self.sd_seed, self.sd_stream,
                                      self.sd_counter)
            self.sd_counter += 1
        for u in self.units:
            k, s = u["key"], u["stride"]
            cin, mid, cout = _pad32(u["cin"]), _pad32(u["mid"]), _pad32(u["cout"])
            ho, wo = ops.conv_out_size(h, s), ops.conv_out_size(w, s)
            if u["conv1"] is not None:
                e_raw = self.buf(k + ".e_raw", B, h, w, mid)
                e_act = self.buf(k + ".e_act", B, h, w, mid)
                if not training and self.fuse_eval:   # expand conv + BN + swish in one launch
                    u["conv1"].forward_affine(x, e_act, u["bn1"], act=2)
                else:
                    u["conv1"].forward(x, e_raw, bn_scratch=self.partials(e_raw) if fuse else None)
                    u["bn1"].stats(e_raw, training, fused=fuse)
                    u["bn1"].act_apply(e_raw, e_act, act=ACT)
            else:
                e_act = x
            d_raw = self.buf(k + ".d_raw", B, ho, wo, mid)
            d_se = self.buf(k + ".d_se", B, ho, wo, mid)
            bn = u["bn2"]
            if fuse:   # the depthwise kernel leaves sum / sum-of-squares in the BN slots: fold only
                u["dw"].forward(e_act, d_raw, bn_scratch=self.scratch(bn.C))
                bn.stats(d_raw, training, slots_filled=True)
            else:
                u["dw"].forward(e_act, d_raw)
                bn.stats(d_raw, training)
            pooled, gate = self._vec(k + ".pooled", B, mid), self._vec(k + ".gate", B, mid)
            pre1 = self._vec(k + ".pre1", B, u["se"].mid)
            bn.act_pool(d_raw, pooled, act=ACT)
            u["se"].forward(pooled, pre1, gate)
            bn.act_apply(d_raw, d_se, act=ACT, gate=gate)
            p_raw = self.buf(k + ".p_raw", B, ho, wo, cout)
            out = self.buf(k + ".out", B, ho, wo, cout)
            if not training and self.fuse_eval:       # project conv + BN (+ skip) in one launch
                u["conv3"].forward_affine(d_se, out, u["bn3"], act=0, residual=x if u["residual"] else None)
            else:
                u["conv3"].forward(d_se, p_raw, bn_scratch=self.partials(p_raw) if fuse else None)
                bn = u["bn3"]
                bn.stats(p_raw, training, fused=fuse)
                if u["residual"] and self._sd_rows is not None:
                    bn.act_apply(p_raw, out, act=ops.ACT_NONE, residual=x, row_scale=self._sd_rows[u["index"]])
                else:
                    bn.act_apply(p_raw, out, act=ops.ACT_NONE, residual=x if u["residual"] else None)
            u["x_in"], u["hw_in"] = x, (h, w)
            x, h, w = out, ho, wo
        self._x_last, self._hw = x, (h, w)
        f_raw = self.buf("f_raw", B, h, w, self.feat_c)
        self.final_conv.forward(x, f_raw, bn_scratch=self.partials(f_raw) if fuse else None)
        self.final_bn.stats(f_raw, training, fused=fuse)
        self._pooled = self._vec("pooled", B, self.feat_c)
        self.final_bn.act_pool(f_raw, self._pooled, act=ACT)
        feat = self._pooled
        self._dropped = training and self.dropout_rate > 0.0
        if self._dropped:
            if ("mask", B) not in self._bufs:
                self._bufs[("mask", B)] = torch.empty((B, self.feat_c), dtype=torch.uint8, device=self.device)
            self._mask = self._bufs[("mask", B)]
            feat = self._vec("dropped", B, self.feat_c)
            self._step += 1
            ops.dropout_fwd(self._pooled, self.dropout_rate, self.dropout_seed * 1000003 + self._step, self._mask,
                            feat)
        self._feat = feat
        z = self._vec("z", B, self.num_classes)
        ops.linear_fwd(feat, self.store.p("output.fc.weight"), self.store.p("output.fc.bias"), z)
        return z

    # ------------------------------------------------------------------ backward
    def backward(self, gz, comm=None):
        self._begin_backward(comm)
        B, st = self._B, self.store
        gz = gz.contiguous()
        gfeat = self._vec("gfeat", B, self.feat_c)
        ops.linear_bwd(self._feat, st.p("output.fc.weight"), gz, gfeat, st.g("output.fc.weight"),
                       st.g("output.fc.bias"))
        if self._dropped:
            gpooled = self._vec("gpooled", B, self.feat_c)
            ops.dropout_bwd(gfeat, self.dropout_rate, self._mask, gpooled)
        else:
            gpooled = gfeat
        h, w = self._hw
        f_raw = self.buf("f_raw", B, h, w, self.feat_c)
        gf = self.buf("g_f", B, h, w, self.feat_c)
        self.final_bn.act_backward(None, f_raw, gf, act=ACT, gpool=gpooled)
        self.final_conv.backward_weight(self._x_last, gf)
        g = self.buf(f"g_{self._x_last.shape[3]}_{h}", B, h, w, self._x_last.shape[3])
        self.final_conv.backward_data(gf, g)
        for i, u in self._units_backward(self.units, comm):
            # the three buffers a weight gradient reads (gp, gd, ge) alternate between consecutive units, so that a unit
            # never overwrites what the previous unit's weight gradients may still be reading (checked bit for bit
            # against one stream with private buffers: tests/test_effnet_gpu.py)
            par = i & 1
            k, s = u["key"], u["stride"]
            cin, mid, cout = _pad32(u["cin"]), _pad32(u["mid"]), _pad32(u["cout"])
            ho, wo = h, w
            hi, wi = u["hw_in"]
            tag = ("@" + k) if self.debug_keep else ""
            p_raw = self.buf(k + ".p_raw", B, ho, wo, cout)
            d_raw = self.buf(k + ".d_raw", B, ho, wo, mid)
            d_se = self.buf(k + ".d_se", B, ho, wo, mid)
            gp = self.buf(f"gp_{cout}_{ho}_{par}{tag}", B, ho, wo, cout)
            gd = self.buf(f"gd_{mid}_{ho}_{par}{tag}", B, ho, wo, mid)
            bn = u["bn3"]
            if u["residual"] and self._sd_rows is not None:
                # out = x_in + r[b] * bn3(p_raw): the branch gradient is g * r[b]; g itself stays the skip gradient
                bn.act_backward(g, p_raw, gp, act=ops.ACT_NONE, row_scale=self._sd_rows[u["index"]])
            else:
                bn.act_backward(g, p_raw, gp, act=ops.ACT_NONE)
            u["conv3"].backward_weight(d_se, gp)
            u["conv3"].backward_data(gp, gd)
            # squeeze-and-excitation + BatchNorm/swish of the depthwise output (gd rewritten in place)
            bn = u["bn2"]
            gpool = self._vec(f"gpool{tag}", B, mid)
            gate = self._vec(k + ".gate", B, mid)
            one_pass = gd.dtype == torch.bfloat16 and not ops.is_deterministic()
            if one_pass:
                # dL/dgate AND what bn2's backward sums are linear in, in one pass over (gd, d_raw): the reduction pass
                # of bn_act_bwd (a second read of both tensors) becomes a [B, C]-sized fold once gpool exists
                sums = self._zeroed(f"se_sums{tag}", (5, B, mid))     # zero on entry, re-zeroed by its last reader
                if id(sums) in self._se_sums_dirty:   # a backward that stopped between the two calls (an exception, an
                    sums.zero_()                      # interrupt) left its sums behind: never accumulate on top of them
                self._se_sums_dirty.add(id(sums))
                bn.act_se_sums(gd, d_raw, sums, act=ACT)
                dgate = sums[0]
            else:
                dgate = self._vec(f"dgate{tag}", B, mid)
                bn.act_pool(d_raw, dgate, act=ACT, mul=gd, scale=1.0)
            # the SE block's parameter gradients go behind the depthwise weight gradient on the second stream (their
            # workspaces alternate between consecutive units like the gradient buffers)
            se_params = u["se"].backward(dgate, gate, self._vec(k + ".pre1", B, u["se"].mid),
                                         self._vec(k + ".pooled", B, mid), self._vec(f"dpre2_{par}{tag}", B, mid),
                                         self._vec(f"dpre1_{par}{tag}", B, u["se"].mid), gpool)
            if one_pass:
                bn.act_se_backward_apply(gd, gate, gpool, sums, d_raw, gd, act=ACT)
                self._se_sums_dirty.discard(id(sums))
            else:
                bn.act_backward(gd, d_raw, gd, act=ACT, gate=gate, gpool=gpool)
            x_in = u["x_in"]
            if u["conv1"] is not None:
                e_raw = self.buf(k + ".e_raw", B, hi, wi, mid)
                e_act = self.buf(k + ".e_act", B, hi, wi, mid)
                ge = self.buf(f"ge_{mid}_{hi}_{par}{tag}", B, hi, wi, mid)
                u["dw"].backward_weight(e_act, gd, also=se_params)
                bn = u["bn1"]
                if u["dw"].stride == 1:
                    # the depthwise data gradient's epilogue leaves bn1's backward sums in the slots: no reduction
                    # pass over ge and e_raw (5.5 % of a step), e_raw is read once there
                    u["dw"].backward_data(gd, ge, bn=bn, bn_x=e_raw)
                    bn.act_backward_apply(ge, e_raw, ge, act=ACT)
                else:
                    u["dw"].backward_data(gd, ge)
                    bn.act_backward(ge, e_raw, ge, act=ACT)
                u["conv1"].backward_weight(x_in, ge)
                if u["residual"]:
                    # out = bn3(...) + x_in: the unit-output gradient g is also the skip gradient ->
                    # accumulate the expand conv's data gradient into it in place
                    u["conv1"].backward_data(ge, g, accumulate=True)
                    g_in = g
                else:
                    g_in = self.buf(f"g_{cin}_{hi}{tag}", B, hi, wi, cin)
                    u["conv1"].backward_data(ge, g_in)
            else:
                # (a unit with a skip still needs g after the data gradient is written: never the buffer g lives in)
                skip = f"_s{par}" if u["residual"] else ""
                g_in = self.buf(f"g_{cin}_{hi}{skip}{tag}", B, hi, wi, cin)
                u["dw"].backward_weight(x_in, gd, also=se_params)
                u["dw"].backward_data(gd, g_in)
                if u["residual"]:      # (B1 and up: stage 1 has a second unit, 16 -> 16 channels) the skip gradient
                    self._add(g_in, g, g_in)
            u["dbg"] = {"g_out": g, "g_in": g_in, "gp": gp, "gd": gd}
            g, h, w = g_in, hi, wi
        t0 = self.buf("t0", B, h, w, _pad32(self.stem_c))
        self.bn0.act_backward(g, t0, g, act=ACT)
        ops.stem_wgrad(self._img, g, st.g("features.init_block.conv.conv.weight"), self.stem_c, stride=2,
                       pad=self._stem_pad(self._img.shape[2], self._img.shape[3]))
        self._end_backward(comm)
