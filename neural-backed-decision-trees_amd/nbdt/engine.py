"""Backbone execution engine: explicit forward/backward/SGD over hand-written HIP kernels.

This replaces the autograd graph of stock aten/cuDNN ops the reference builds per step
(main.py:233-239 around nbdt/models/resnet.py:136-149 / pytorchcv CIFARWRN.forward) with a fixed,
pre-planned launch sequence:

  * every parameter lives in ONE flat fp32 buffer (``ParamStore``) with a flat gradient buffer, a
    flat momentum buffer and a flat bf16 mirror -- SGD is one kernel, gradient all-reduce is a few
    large buckets, and the bf16 weights the convs read are refreshed by the SGD kernel itself;
  * activations are padded NHWC bf16 buffers allocated once per batch size and kept resident
    (288 GB of HBM: nothing is recomputed or freed inside a step);
  * forward records nothing: backward is the hand-written mirror sequence.

Python here only sequences C-ABI launches on the current HIP stream (capturable in a hipGraph via
torch.cuda.CUDAGraph); there is no CPU or PyTorch-op fallback for any tensor op on the path.
"""
import collections
import contextlib
import math

import torch

from nbdt import _C, ops

ALIGN = 8  # elements: keeps every parameter 16-byte aligned in the bf16 mirror

_SIDE_STREAMS = {}


def side_stream(device):
    """THE second HIP stream of this process on `device` (weight gradients, derived-weight builds): created once and
    shared by every engine.  Streams created later in a process land on the main stream's hardware queue in about one
    of four tries (measured in round 3; seen again in round 6 as one 20 ms engine in ten in scripts that build several
    engines) -- there the two-stream schedule serialises and a WRN-28-10 step takes 19-20 ms instead of 16.5.  One engine
    steps at a time, so sharing the stream costs nothing."""
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _SIDE_STREAMS[key]


def _pad32(c):
    return (c + 31) // 32 * 32


# train_step(..., lars=LarsConfig(...)): the optimizer pass is engine.lars_step instead of engine.sgd_step
LarsConfig = collections.namedtuple("LarsConfig", ("trust", "eps", "exclude_1d"), defaults=(1e-3, 1e-8, True))
# train_step(..., optim=AdamWConfig(...) | RMSpropConfig(...)): engine.adamw_step / engine.rmsprop_step; lr, weight_decay and
# (RMSprop) momentum are train_step's own arguments.  RMSpropConfig(tf=True) is TensorFlow's form, with its defaults given
# explicitly by the caller (alpha 0.9, eps 1e-3 in the EfficientNet recipe).
AdamWConfig = collections.namedtuple("AdamWConfig", ("betas", "eps", "exclude_1d"), defaults=((0.9, 0.999), 1e-8, True))
RMSpropConfig = collections.namedtuple("RMSpropConfig", ("alpha", "eps", "tf", "exclude_1d"),
                                       defaults=(0.99, 1e-8, False, True))
# train_step(..., clip=ClipConfig(max_norm)): engine.clip_grad_norm between the last backward and the optimizer pass
ClipConfig = collections.namedtuple("ClipConfig", ("max_norm",))

_EMA_SWAPPED = ("%s: the averaged weights are swapped in (ema_swap / ema_weights); stepping or averaging would train into "
                "the average -- swap back first")


class ParamStore:
    """Flat parameter / gradient / momentum / bf16-mirror buffers + named views."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.entries = {}   # name -> (offset, internal_shape)
        self.inits = []     # (name, fn(view))
        self.n = 0
        self.flat = self.grad = self.mom = self.bf16 = None
        self.ema = None     # the moving average of flat (or, while _Engine.ema_swapped, the live weights): ema_enable
        self.sq = None      # second optimizer state (AdamW's v, RMSprop's mean square): init_sq, at the first adaptive step
        self._views = {}    # (which buffer, name) -> (view, the buffer it was made of)

    def add(self, name, shape, init):
        assert self.flat is None and name not in self.entries
        numel = 1
        for s in shape:
            numel *= s
        self.entries[name] = (self.n, tuple(shape))
        self.inits.append((name, init))
        self.n += (numel + ALIGN - 1) // ALIGN * ALIGN

    def finalize(self):
        n = (self.n + 3) // 4 * 4
        host = torch.zeros(n, dtype=torch.float32)
        for name, init in self.inits:
            off, shape = self.entries[name]
            numel = math.prod(shape)
            init(host[off:off + numel].view(shape))
        self.flat = host.to(self.device)
        self.grad = torch.zeros_like(self.flat)
        self.mom = torch.zeros_like(self.flat)
        self.bf16 = self.flat.to(torch.bfloat16)

    def _view(self, buf, name):
        off, shape = self.entries[name]
        return buf[off:off + math.prod(shape)].view(shape)

    def _cached(self, which, buf, name):
        # the flat buffers are allocated once (finalize) and only ever written in place: a named view is made once.  (ResNet18
        # on CIFAR10 at 128 images is bound by the host's launch path: 9,000 slice + view calls per 50 steps were 10 % of it.)
        hit = self._views.get((which, name))
        if hit is not None and hit[1] is buf:          # (a replaced flat buffer -- nobody does that today -- is a miss)
            return hit[0]
        v = self._view(buf, name)
        self._views[(which, name)] = (v, buf)
        return v

    def p(self, name):
        return self._cached(0, self.flat, name)

    def g(self, name):
        return self._cached(1, self.grad, name)

    def pb(self, name):
        return self._cached(2, self.bf16, name)

    def refresh_bf16(self):
        self.bf16.copy_(self.flat)   # plumbing: only after load_state_dict, not on the step path

    def zero_grad(self):
        self.grad.zero_()            # one memset node

    def init_sq(self, ones=False):
        """(Re-)initialise the second state arena, allocating it at first use (SGD and LARS runs never pay for it): zeros, or
        with `ones` 1 inside every segment (TensorFlow's RMSprop starts its mean square there) and 0 in the gaps."""
        if self.sq is None:
            self.sq = torch.zeros_like(self.flat)
        else:
            self.sq.zero_()
        if ones:
            for off, length, _, _ in self.segments(0.0):
                self.sq[off:off + length].fill_(1.0)

    def segments(self, weight_decay, exclude_1d=True):
        """The segment table of a layer-wise optimizer (ops.LarsPlan): one row (offset, length, weight_decay, adapt) per
        entry, in offset order.  The length is the product of the INTERNAL shape: the zero padding inside an entry adds
        nothing to either norm and stays zero under the update; the alignment gaps between entries and the tail belong to
        no row.  exclude_1d: one-dimensional entries (BatchNorm gamma / beta, biases) are neither decayed nor adapted,
        the published recipe; False gives every entry adapt = 1 and the decay."""
        rows = []
        for name, (off, shape) in sorted(self.entries.items(), key=lambda kv: kv[1][0]):
            plain = exclude_1d and len(shape) <= 1
            rows.append((off, math.prod(shape), 0.0 if plain else float(weight_decay), 0 if plain else 1))
        return rows

    def segment_names(self):
        """Entry names in the row order of segments()."""
        return [name for name, _ in sorted(self.entries.items(), key=lambda kv: kv[1][0])]


class Conv:
    """3x3 / 1x1 convolution (bias-free) with forward, data-gradient and weight-gradient launches."""

    def __init__(self, store, name, cin_real, cout_real, k, stride, gen, init="kaiming_a0", fan_taps=None):
        self.store, self.name = store, name
        self.cin_real, self.cout_real, self.k, self.stride = cin_real, cout_real, k, stride
        self.cin, self.cout = _pad32(cin_real), _pad32(cout_real)
        self.taps = k * k
        fan_in = cin_real * k * k
        std = None
        if init == "kaiming_a0":       # pytorchcv: init.kaiming_uniform_(w)  (a = 0)
            bound = math.sqrt(2.0) * math.sqrt(3.0 / fan_in)
        elif init == "kaiming_normal_fan_out":   # torchvision: kaiming_normal_(w, mode="fan_out", nonlinearity="relu");
            std = math.sqrt(2.0 / (cout_real * (fan_taps or k * k)))      # fan_taps: the taps a patch conv stands for
        else:                          # nn.Conv2d default: kaiming_uniform_(w, a=sqrt(5))
            bound = 1.0 / math.sqrt(fan_in)

        def init(v):
            v.zero_()
            if std is not None:
                v[:cout_real, :, :cin_real].normal_(0.0, std, generator=gen)
            else:
                v[:cout_real, :, :cin_real].uniform_(-bound, bound, generator=gen)

        store.add(name, (self.cout, self.taps, self.cin), init)
        self._plans = {}
        self.wd = None
        self.wt_fwd = self.wt_dgrad = None   # DMA-ordered weight tiles (dense 3x3 / stride 1: _Engine.finalize)
        self.side_stream = None              # the engine's second stream for weight gradients, or None: the caller's
        self.pointwise = False               # stride-1 1x1 launches go to ops.conv_pw (BottleneckEngine.pointwise)

    fused_stats = True     # forward(bn_scratch=...) leaves the next BatchNorm's partial sums (ResNetEngine.forward asks)

    def logical(self, buf):
        """[cout_real, cin_real, k, k] view (OIHW semantics, channels_last memory) of a flat buffer."""
        v = self.store._view(buf, self.name).view(self.cout, self.k, self.k, self.cin)
        return v[:self.cout_real, :, :, :self.cin_real].permute(0, 3, 1, 2)

    def plan(self, B, Hi, Wi):
        key = (B, Hi, Wi)
        if key not in self._plans:
            self._plans[key] = self._make_plan(B, Hi, Wi)
        return self._plans[key]

    def _make_plan(self, B, Hi, Wi):
        p = self._raw_plan(B, Hi, Wi)
        if self.wt_fwd is not None:      # dense 3x3 / stride 1: DMA-ordered weight tiles
            p[0].w_tiled = self.wt_fwd.data_ptr()
            for descs in (p[1], p[2]):
                if descs is not None and len(descs) == 1:
                    descs[0].w_tiled = self.wt_dgrad.data_ptr()
        return p

    def _raw_plan(self, B, Hi, Wi):
        """(forward desc, dgrad descs, accumulating dgrad descs, wgrad desc) for one input geometry."""
        args = (B, Hi, Wi, self.cin, self.cout, self.k, self.stride)
        plain_dgrad = None if (self.k == 1 and self.stride == 2) else ops.conv_dgrad_descs(*args, accumulate=False)
        plan = (ops.conv_fwd_desc(*args), plain_dgrad, ops.conv_dgrad_descs(*args, accumulate=True),
                ops.conv_wgrad_desc(*args))
        # what the launch timers count as a launch's flops: the layer's REAL channels, not the 32-padded ones the kernels
        # multiply (16 -> 32 for WRN's first unit): fwd / wgrad (cin, cout), dgrad (cout, cin) -- ops.desc_flops
        for d in (plan[0], plan[3]):
            d.flop_channels = (self.cin_real, self.cout_real)
        for descs in (plan[1], plan[2]):
            for d in descs or ():
                d.flop_channels = (self.cout_real, self.cin_real)
        return plan

    def numel(self):
        return self.cout * self.taps * self.cin

    def _w_for(self, x):
        """Forward weights in the storage type of the activations: the bf16 mirror, or (verification-only fp32
        reference mode) the fp32 master itself."""
        return self.store.p(self.name) if x.dtype == torch.float32 else self.store.pb(self.name)

    def _wd_for(self, g):
        """Data-gradient weights [cin][taps][cout], tap order reversed: the bf16 copy weight_prep built, or an fp32
        one (reference mode; plumbing on parameters, rebuilt by refresh_derived_weights)."""
        return self.wd32 if g.dtype == torch.float32 else self.wd

    # Shapes that stay on nbdt_conv_igemm (form 0) although the conv is pointwise: STATISTICS launches (the training
    # forward) with fewer than this many input channels.  The pointwise kernel's statistics pass (the first-generation
    # kernel's summation order, so that both leave the same bits) costs 3-5 us per launch; measured at 128 images
    # (profiles/bottleneck_pw_ab.txt) it is 5-51 % slower there for cin <= 512 and 10-24 % faster for cin >= 1024.
    # Plain and accumulating launches (every data gradient) are faster on every shape and have no exception.
    PW_STATS_MIN_CIN = 1024

    def _pw(self):
        """This conv's forward and data gradient run on the pointwise GEMM kernel (ops.conv_pw): stride-1 1x1 convs of an
        engine that asked for it.  The only routing point ("Pointwise convolutions")."""
        return self.pointwise and self.k == 1 and self.stride == 1

    def forward(self, x, out, residual=None, bn_scratch=None):
        B, Hp, Wp, _ = x.shape
        if self._pw() and residual is None and (bn_scratch is None or self.cin >= self.PW_STATS_MIN_CIN):
            ops.conv_pw(self.plan(B, Hp - 2, Wp - 2)[0], x, self._w_for(x), out, bn_scratch)
            return
        ops.conv_igemm(self.plan(B, Hp - 2, Wp - 2)[0], x, self._w_for(x), out, residual, bn_scratch)

    def forward_affine(self, x, out, bn, act=1, residual=None):
        """Inference: conv + eval-mode BatchNorm `bn` (folded to scale/shift) + activation [+ residual] in one
        launch (act: 0 none, 1 ReLU, 2 swish)."""
        B, Hp, Wp, _ = x.shape
        scale, shift = bn.eval_affine()
        ops.conv_igemm_affine(self.plan(B, Hp - 2, Wp - 2)[0], x, self.store.pb(self.name), out, scale, shift, act,
                              residual)

    def backward_data(self, gout, gin, accumulate=False, bn=None, bn_x=None, partials=None):
        """bn/bn_x/partials: `gin` is dL/d(relu(bn(bn_x))) -- also emit that BatchNorm's backward sums
        (single-launch stride-1 dgrads only)."""
        B, Hp, Wp, _ = gin.shape
        plan = self.plan(B, Hp - 2, Wp - 2)
        descs = plan[2] if accumulate else plan[1]
        if bn is not None:
            assert len(descs) == 1 and not accumulate
            ops.conv_igemm_bnbwd(descs[0], gout, self.wd, gin, bn_x, bn.mean, bn.rstd, bn.gamma, bn.beta, partials)
            return
        if len(descs) > 1:      # strided 3x3: four parity classes, one grid
            ops.conv_igemm_multi(descs, gout, self._wd_for(gout), gin)
            return
        for d in descs:
            if self._pw():
                ops.conv_pw(d, gout, self._wd_for(gout), gin)
            else:
                ops.conv_igemm(d, gout, self._wd_for(gout), gin)

    def s2d_plan(self, B, Hi, Wi):
        """(forward desc [1x1 only], wgrad desc) of this stride-2 conv over the space-to-depth copy of its input."""
        key = ("s2d", B, Hi, Wi)
        if key not in self._plans:
            fwd = ops.conv_fwd_desc_s2d_1x1(B, Hi, Wi, self.cin, self.cout) if self.k == 1 else None
            wg = ops.conv_wgrad_desc_s2d(B, Hi, Wi, self.cin, self.cout, self.k)
            for d in (fwd, wg):
                if d is not None:
                    d.flop_channels = (self.cin_real, self.cout_real)
            self._plans[key] = (fwd, wg)
        return self._plans[key]

    def forward_s2d(self, xs, out, Hi, Wi):
        ops.conv_igemm(self.s2d_plan(xs.shape[0], Hi, Wi)[0], xs, self._w_for(xs), out)

    def backward_weight_s2d(self, xs, gout, Hi, Wi, cu_budget=0):
        self._wgrad(self.s2d_plan(xs.shape[0], Hi, Wi)[1], xs, gout, cu_budget)

    def backward_weight(self, x, gout, cu_budget=0):
        """cu_budget: CUs this launch is sized for when it runs on the second stream (0 = all of them): the caller
        is about to launch an HBM-bound pass on the main stream that should get the remaining CUs."""
        B, Hp, Wp, _ = x.shape
        self._wgrad(self.plan(B, Hp - 2, Wp - 2)[3], x, gout, cu_budget)

    def _wgrad(self, desc, x, gout, cu_budget):
        side = self.side_stream
        if side is None:
            ops.conv_wgrad(desc, x, gout, self.store.g(self.name), cu_budget)
            return
        # the weight gradient only feeds the optimizer, so it runs on a second stream next to the
        # data-gradient chain (see WRNEngine.backward for the buffer-reuse ordering)
        side.wait_stream(torch.cuda.current_stream(x.device))
        with torch.cuda.stream(side):
            ops.conv_wgrad(desc, x, gout, self.store.g(self.name), cu_budget)


class GroupedConv:
    """Grouped 3x3 convolution (bias-free) of a ResNeXt bottleneck: cin == cout == width, cg = width / groups channels per
    group with cg in ops.GROUP_CG -- width / 32 block-diagonal 32 x 32 convolutions (csrc/conv_group.hip).  The four
    launches the block walker calls; NOT in _Engine.convs (whose batched tables assume dense [cout][taps][cin] masters):
    _Engine.gconvs, with its own derived-weight tables (_Engine.finalize / refresh_derived_weights).

    Master parameter [width][9][cg] (project order [cout][taps][cin in group]); init is torchvision's
    kaiming_normal_(mode="fan_out") of the [width, cg, 3, 3] weight, whose fan_out is width * 9 (torch takes it from the
    tensor's shape: the group count does not enter)."""

    k, taps = 3, 9
    fused_stats = False    # no statistics epilogue: the following BatchNorm takes its separate bn.stats pass
    pointwise = False

    def __init__(self, store, name, width, groups, stride, gen):
        cg = width // groups if groups > 0 else 0
        if groups <= 0 or width % groups or width % 32 or cg not in ops.GROUP_CG:
            raise ValueError(f"{name}: a grouped 3x3 conv takes width % 32 == 0 and width / groups in {ops.GROUP_CG}, got "
                             f"width {width}, groups {groups} (cg = 64, as in resnext101_32x8d, is not supported)")
        self.store, self.name = store, name
        self.cin_real = self.cout_real = self.cin = self.cout = self.width = width
        self.groups, self.cg, self.stride = groups, cg, stride
        std = math.sqrt(2.0 / (width * 9))
        store.add(name, (width, 9, cg), lambda v: v.normal_(0.0, std, generator=gen))
        self.wf = self.wd = None             # expanded bf16 blocks [width/32][32][9][32]: views of the engine's flat buffers
        self.side_stream = None

    def logical(self, buf):
        """[width, cg, 3, 3] view (OIHW semantics: torchvision's shape of a grouped weight) of a flat buffer."""
        return self.store._view(buf, self.name).view(self.width, 3, 3, self.cg).permute(0, 3, 1, 2)

    def numel(self):
        return self.width * 9 * 32

    def _master_or(self, t, blocks):
        """fp32 tensors (verification-only reference mode) take the fp32 master itself, bf16 ones the expanded blocks."""
        return self.store.p(self.name) if t.dtype == torch.float32 else blocks

    def forward(self, x, out, residual=None, bn_scratch=None):
        assert residual is None and bn_scratch is None, "the grouped conv has no residual operand and no statistics epilogue"
        ops.conv_group_fwd(x, self._master_or(x, self.wf), out, self.cg, self.stride)

    def forward_affine(self, x, out, bn, act=1, residual=None):
        assert residual is None, "the grouped conv has no residual operand"
        scale, shift = bn.eval_affine()
        ops.conv_group_fwd(x, self.wf, out, self.cg, self.stride, scale, shift, act)

    def backward_data(self, gout, gin, accumulate=False):
        ops.conv_group_dgrad(gout, self._master_or(gout, self.wd), gin, self.cg, self.stride, accumulate)

    def backward_weight(self, x, gout, cu_budget=0):
        """On the engine's second stream, as Conv._wgrad (cu_budget: ignored, the launch is not a one-block-per-CU kernel)."""
        side = self.side_stream
        if side is None:
            ops.conv_group_wgrad(x, gout, self.store.g(self.name), self.cg, self.stride)
            return
        side.wait_stream(torch.cuda.current_stream(x.device))
        with torch.cuda.stream(side):
            ops.conv_group_wgrad(x, gout, self.store.g(self.name), self.cg, self.stride)


class PatchConv(Conv):
    """A k x k convolution of the 3-colour image as the 1x1 convolution of its patch tensor (ops.stem_patches): cin_real =
    3 * k * k channels in (r, s, ci) order.  Always on nbdt_conv_igemm, whatever the engine routes its pointwise convs to."""

    def __init__(self, store, name, cout_real, patch_k, gen, init):
        super().__init__(store, name, 3 * patch_k * patch_k, cout_real, 1, 1, gen, init, fan_taps=patch_k * patch_k)
        self.patch_k = patch_k

    def _pw(self):
        return False

    def logical(self, buf):
        """[cout_real, 3, k, k] view (OIHW semantics) of a flat buffer: the row's first 3*k*k entries are (r, s, ci)."""
        k = self.patch_k
        v = self.store._view(buf, self.name)[:self.cout_real, 0, :self.cin_real]
        return v.view(self.cout_real, k, k, 3).permute(0, 3, 1, 2)


class SegOp:
    """A slice-list launch (ops.ConvSeg, csrc/conv_seg.hip) together with its DMA-ordered weight tiles.  `sources` returns
    the bf16 weight matrices the tiles are built from (views of the engine's flat bf16 mirror / data-gradient copies) and
    `sources32` their fp32 twins for the verification-only reference mode; `on_side`: the sources are the data-gradient
    copies the engine builds on its second stream, so the tiles are built there too."""

    def __init__(self, plan, sources, sources32, on_side):
        self.plan, self.sources, self.sources32, self.on_side = plan, sources, sources32, on_side
        self.tiles = None

    def retile(self):
        self.tiles = self.plan.tile_weights(self.sources(), out=self.tiles)

    def __call__(self, ins, out, bn_scratch=None):
        if ins[0].dtype == torch.float32:
            self.plan(ins, self.sources32(), out, bn_scratch=bn_scratch)
        else:
            self.plan(ins, self.tiles, out, bn_scratch=bn_scratch)


class BatchNorm:
    def __init__(self, store, name, c_real, scratch_owner, gamma=1.0, eps=ops.BN_EPS):
        self.store, self.name, self.c_real = store, name, c_real
        self.eps = float(eps)          # one value for the batch statistics, the evaluation transform and eval_affine
        self.C = _pad32(c_real)
        store.add(name + ".weight", (self.C,), lambda v: v.fill_(gamma))
        store.add(name + ".bias", (self.C,), lambda v: v.zero_())
        dev = store.device
        self.running_mean = torch.zeros(self.C, device=dev)
        self.running_var = torch.ones(self.C, device=dev)
        self.num_batches_tracked = 0   # host counter (state_dict compat); no launch on the step path
        self.mean = torch.empty(self.C, device=dev)
        self.rstd = torch.empty(self.C, device=dev)
        self.dsum = torch.empty(2 * self.C, device=dev)
        self.owner = scratch_owner
        self._affine = None            # cached (scale, shift) of the eval-mode transform

    def eval_affine(self):
        """scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale: two [C] vectors computed
        once per parameter / running-statistics version (plumbing on parameters, not on the data path)."""
        if self._affine is None:
            scale = self.gamma * torch.rsqrt(self.running_var + self.eps)
            self._affine = (scale.contiguous(), (self.beta - self.running_mean * scale).contiguous())
        return self._affine

    @property
    def gamma(self):
        return self.store.p(self.name + ".weight")

    @property
    def beta(self):
        return self.store.p(self.name + ".bias")

    def stats(self, x, training, fused=False, slots_filled=False):
        """fused=True: the producing conv's epilogue already wrote per-tile partial sums (fold only).
        slots_filled=True: the producing kernel (a depthwise conv given the owner's scratch) left the sums in the slots."""
        if training:
            self._affine = None        # running statistics are about to change
            if fused:
                ops.bn_finalize(x, self.owner.partials(x), self.mean, self.rstd, self.running_mean,
                                self.running_var, eps=self.eps)
            elif slots_filled:
                ops.bn_stats(x, self.owner.scratch(self.C), self.mean, self.rstd, self.running_mean,
                             self.running_var, eps=self.eps, slots_filled=True)
            else:
                ops.bn_stats(x, self.owner.scratch(self.C), self.mean, self.rstd, self.running_mean,
                             self.running_var, eps=self.eps)
            self.num_batches_tracked += 1
        else:  # eval: running statistics (two [C]-sized plumbing ops, not on the training path)
            self.mean.copy_(self.running_mean)
            torch.rsqrt(self.running_var + self.eps, out=self.rstd)

    def apply(self, x, y, relu=True, residual=None):
        ops.bn_apply(x, self.mean, self.rstd, self.gamma, self.beta, y, relu=relu, residual=residual)

    def apply_s2d(self, x, y, relu=True):
        """apply() written as the space-to-depth copy the stride-2 convs of a shape-changing unit read."""
        ops.bn_apply_s2d(x, self.mean, self.rstd, self.gamma, self.beta, y, relu=relu)

    def backward_fused(self, gy, x, gx, partials, gx_add=None, cus=0):
        """Backward of relu(bn(x)) when the dgrad that produced gy already wrote the reduction partials.
        cus > 0: the elementwise pass is confined to that many CUs (a weight gradient runs on the others)."""
        ops.bn_bwd_fused(gy, x, self.mean, self.rstd, self.gamma, self.beta, partials, self.dsum,
                         self.store.g(self.name + ".weight"), self.store.g(self.name + ".bias"), gx, gx_add=gx_add,
                         cus=cus)

    def backward_cus(self, gy, x, gx, cus, gx_add=None):
        """Backward of relu(bn(x)) entirely on `cus` CUs: sums and elementwise pass, the fold of the sums in the latter's
        prologue (no dgrad-epilogue partials), summed into the owner's slot pair of this channel count."""
        ops.bn_bwd_cus(gy, x, self.mean, self.rstd, self.gamma, self.beta, self.owner.slot_pair(self.C), self.dsum,
                       self.store.g(self.name + ".weight"), self.store.g(self.name + ".bias"), gx, cus, gx_add=gx_add)

    def backward(self, gy, y, x, gx, relu=True, gx_add=None, g_resid=None):
        """y=None: recompute the ReLU mask from x (valid when apply() had no residual)."""
        ops.bn_bwd(gy, y, x, self.mean, self.rstd, self.gamma, self.owner.scratch(self.C), self.dsum,
                   self.store.g(self.name + ".weight"), self.store.g(self.name + ".bias"), gx, relu=relu,
                   gx_add=gx_add, g_resid=g_resid, beta=self.beta)

    def pool_backward(self, gpooled, x, gx):
        """Backward of mean_hw relu(bn(x)) from dL/dpooled [B, C]."""
        ops.pool_bn_bwd(gpooled, x, self.mean, self.rstd, self.gamma, self.beta, self.owner.scratch(self.C), self.dsum,
                        self.store.g(self.name + ".weight"), self.store.g(self.name + ".bias"), gx)

    # ---- the activation family (csrc/effnet.hip): act(bn(x)) with a squeeze-and-excitation gate, a residual, a per-image
    # row scale.  Each method is its nbdt.ops entry with this BatchNorm's vectors, the owner's scratch and the two
    # gradient views filled in; row_scale is handed on only when there is one (the call without it is the plain entry's).
    def act_apply(self, x, y, act=ops.ACT_SWISH, gate=None, residual=None, row_scale=None):
        if row_scale is not None:
            ops.bn_act_apply(x, self.mean, self.rstd, self.gamma, self.beta, y, act=act, gate=gate, residual=residual,
                             row_scale=row_scale)
        else:
            ops.bn_act_apply(x, self.mean, self.rstd, self.gamma, self.beta, y, act=act, gate=gate, residual=residual)

    def act_pool(self, x, out, act=ops.ACT_SWISH, mul=None, scale=None):
        ops.bn_act_pool(x, self.mean, self.rstd, self.gamma, self.beta, out, act=act, mul=mul, scale=scale)

    def act_backward(self, gu, x, gx, act=ops.ACT_SWISH, gate=None, gpool=None, gx_add=None, row_scale=None):
        if row_scale is not None:
            ops.bn_act_bwd(gu, x, self.mean, self.rstd, self.gamma, self.beta, self.owner.scratch(self.C), self.dsum,
                           self.store.g(self.name + ".weight"), self.store.g(self.name + ".bias"), gx, act=act,
                           gate=gate, gpool=gpool, gx_add=gx_add, row_scale=row_scale)
        else:
            ops.bn_act_bwd(gu, x, self.mean, self.rstd, self.gamma, self.beta, self.owner.scratch(self.C), self.dsum,
                           self.store.g(self.name + ".weight"), self.store.g(self.name + ".bias"), gx, act=act,
                           gate=gate, gpool=gpool, gx_add=gx_add)

    def act_backward_apply(self, gu, x, gx, act=ops.ACT_SWISH, gx_add=None):
        """act_backward without its reduction pass: the producing kernel filled the owner's slots."""
        ops.bn_act_bwd_apply(gu, x, self.mean, self.rstd, self.gamma, self.beta, self.owner.scratch(self.C), self.dsum,
                             self.store.g(self.name + ".weight"), self.store.g(self.name + ".bias"), gx, act=act,
                             gx_add=gx_add)

    def dwconv_backward_data(self, gy, w, gx, k, x):
        """ops.dwconv_bwd_data_bn: the stride-1 depthwise data gradient gx = dL/d(swish(bn(x))), which also leaves this
        BatchNorm's backward sums in the owner's slots (DepthwiseConv.backward_data(bn=...); act_backward_apply follows)."""
        ops.dwconv_bwd_data_bn(gy, w, gx, k, x, self.mean, self.rstd, self.gamma, self.beta, self.owner.scratch(self.C))

    def act_se_sums(self, gu, x, sums, act=ops.ACT_SWISH):
        ops.bn_act_se_sums(gu, x, self.mean, self.rstd, self.gamma, self.beta, sums, act=act)

    def act_se_backward_apply(self, gu, gate, gpool, sums, x, gx, act=ops.ACT_SWISH):
        ops.bn_act_se_bwd_apply(gu, gate, gpool, sums, x, self.mean, self.rstd, self.gamma, self.beta, self.dsum,
                                self.store.g(self.name + ".weight"), self.store.g(self.name + ".bias"), gx, act=act)


class _Engine:
    """Shared machinery: parameter store, scratch, activation buffers, optimizer."""

    def __init__(self, device, seed):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the NBDT backbone engine runs on MI355X only (no CPU fallback)")
        self.store = ParamStore(self.device)
        self.gen = torch.Generator().manual_seed(seed)
        self._scratch = None
        self._bufs = {}
        self.convs, self.bns = [], []
        self.gconvs = []          # GroupedConv: not in convs (finalize's dense tables); own tables, same refresh points
        self.training = True
        self.act_dtype = torch.bfloat16   # storage of activations / activation gradients (fp32: set_reference_fp32)
        self.debug_keep = False   # tests: give every unit its own gradient buffers (no reuse)
        self.debug_share_serial = False   # tests: the CU-sharing schedule's exact launches (CU counts, budgets) on ONE stream
        self.fuse_stats = True    # BN sums come out of the producing conv's epilogue (no stats pass)
        self.fuse_eval = True     # inference: eval-mode BN + activation folded into the conv epilogue
        self.share_bn2_tensors, self.share_bn1_tensors = 5, 6   # tensor passes of the confined BatchNorm backward (CU plan)
        self.fuse_bn1_bwd = True  # ResNet basic block: bn1's backward sums in conv2's data-gradient epilogue (A/B)
        self._side = None         # second stream for weight gradients (WRNEngine turns it on)
        self._cu_share = None     # set_cu_share(): BatchNorm-backward passes beside weight gradients on disjoint CUs
        self._share_join = False
        self._share_split = (False, 250.0)
        self._share_calibrated = True
        self.cu_share_report = None
        self._overlap = True
        self._seg_ops = {}        # slice-list launches (SegOp) by (unit, role, geometry)
        self._seg_skip = set()    # ... and the keys whose fused conv2 + shortcut launch is not taken (_seg_conv2_sc)
        self.share_stage_us = {}  # output-grid pixels (ho * wo) -> split_target_us of that stage (absent: set_cu_share's)
        self._slot_pairs = {}     # channel count -> [buffer 0, buffer 1, dirty index] (slot_pair)
        self._slot_arena, self._slot_arena_pairs = None, 0    # the one buffer every slot pair lives in (reset_slot_pairs)
        self._partials = None     # conv-epilogue BatchNorm partial sums (partials)
        self._reserved_now = 0    # CUs the MFMA launches currently leave to in-flight all-reduces (_reserve_for)
        self._grad_is_zero = False   # the flat gradient buffer is known to be zero (sgd_step(zero_grad=True))
        self._plans = {}          # (ops.LarsPlan | ops.ArenaOptPlan, weight_decay, exclude_1d) -> that plan (optimizer_step)
        self._lars_last = None    # the plan of the last lars_step (last_trust_ratios)
        self._opt_owner = None    # "adamw" | "rmsprop" | "rmsprop_tf": whose state store.mom and store.sq hold
        self.opt_steps = 0        # adaptive steps since the state was (re-)initialised: AdamW's t
        self._clip_plan = None    # ops.ClipPlan over store.grad (clip_grad_norm), made at first use
        self.ema_swapped = False  # ema_swap(): the arena holds the average, store.ema the live weights; no optimizer step then
        self.ema_updates = 0      # ema_update() calls since ema_enable (the t of ema_decay_at)
        self._ema_table = None    # ops.EmaTable over (running statistic, its shadow) of every BatchNorm
        self._B = None            # batch of the last forward()

    def seg_op(self, key, build, sources, sources32, on_side=False):
        """The SegOp `key` (created, and its weights tiled, at first use: a new batch size or image size)."""
        op = self._seg_ops.get(key)
        if op is None:
            op = SegOp(build(), sources, sources32, on_side)
            if self.act_dtype != torch.float32:
                if on_side and self._side is not None and self._overlap:
                    self._side.wait_stream(torch.cuda.current_stream(self.device))
                    with torch.cuda.stream(self._side):
                        op.retile()
                    torch.cuda.current_stream(self.device).wait_stream(self._side)
                else:
                    op.retile()
            self._seg_ops[key] = op
        return op

    def _retile_seg(self, on_side):
        if self.act_dtype == torch.float32:
            return
        for op in self._seg_ops.values():
            if op.on_side == on_side:
                op.retile()

    def s2d_buf(self, key, B, H, W, C):
        k = (key, "s2d", B, H, W, C)
        if k not in self._bufs:
            self._bufs[k] = ops.s2d_buffer(B, H, W, C, self.device, self.act_dtype)
        return self._bufs[k]

    def scratch(self, C):
        need = ops.BN_SLOTS * 2 * C
        if self._scratch is None or self._scratch.numel() < need:
            # zero on entry is the C-ABI contract; the fold kernels re-zero what they read
            self._scratch = torch.zeros(max(need, ops.BN_SLOTS * 2 * 2048), device=self.device)
        return self._scratch

    def slot_pair(self, C):
        """(slots, slots_other) for ops.bn_bwd_cus' two-launch form: two 32-slot buffers PER CHANNEL COUNT that swap roles
        at every call (the pass leaves the one it summed into dirty and zeroes the other one -- for ITS channel count, hence
        one pair per C).  Every user is a launch on the caller's stream, in program order.  The kernel's contract is
        "`slots` is zero on entry": a step makes an ODD number of calls per channel count (2n-1 for a WRN stage), so the
        pair does not return to its starting state by itself -- backward() calls reset_slot_pairs() first, which makes
        every step (and every captured graph of one) start from (zero, zero) whatever ran before it."""
        pairs = self._slot_pairs
        if C not in pairs:
            n = ops.BN_SLOTS * 2 * C
            # [buffer 0, buffer 1, index of the buffer the LAST call summed into (dirty), or -1: both are zero]
            pairs[C] = [torch.zeros(n, device=self.device), torch.zeros(n, device=self.device), -1]
        pair = pairs[C]
        use = 0 if pair[2] != 0 else 1          # sum into the buffer the last call zeroed
        pair[2] = use
        return pair[use], pair[use ^ 1]

    def reset_slot_pairs(self):
        """Zero the one dirty buffer of every slot pair (a stream-ordered fill on the caller's stream) so that the next
        slot_pair() call finds (zero, zero).  Called at the top of backward(): a hipGraph of a step bakes the pointers
        in, and without this replay k+1's first call per channel count summed into what replay k's last call left."""
        pairs = self._slot_pairs
        if not pairs:
            return
        if self._slot_arena_pairs != len(pairs):
            # (re)pack every pair into ONE zeroed arena, so that a step pays one fill launch for all channel counts instead of
            # one each (three per WRN-28-10 step: 15 us + their launch gaps between forward and backward).  Only when a new
            # channel count appeared -- the first backward of a shape; GraphedStep's warm-up steps come before its capture.
            arena = torch.zeros(sum(2 * p[0].numel() for p in pairs.values()), device=self.device)
            off = 0
            for p in pairs.values():
                n = p[0].numel()
                p[0], p[1], p[2] = arena[off:off + n], arena[off + n:off + 2 * n], -1
                off += 2 * n
            self._slot_arena, self._slot_arena_pairs = arena, len(pairs)
            return
        if any(p[2] >= 0 for p in pairs.values()):
            self._slot_arena.zero_()
            for p in pairs.values():
                p[2] = -1

    def partials(self, out):
        """Workspace for the conv-epilogue BN partial sums of a padded [B,H+2,W+2,C] output."""
        B, Hp, Wp, C = out.shape
        need = ((B * (Hp - 2) * (Wp - 2) + 255) // 256) * 2 * C
        if self._partials is None or self._partials.numel() < need:
            self._partials = torch.empty(need, device=self.device)
        return self._partials

    def buf(self, key, B, H, W, C):
        k = (key, B, H, W, C)
        if k not in self._bufs:
            self._bufs[k] = ops.padded(B, H, W, C, self.device, self.act_dtype)
        return self._bufs[k]

    def conv(self, name, cin, cout, k, stride, init="kaiming_a0"):
        c = Conv(self.store, name, cin, cout, k, stride, self.gen, init)
        if self._side is not None:
            c.side_stream = self._side
        self.convs.append(c)
        return c

    def grouped_conv(self, name, width, groups, stride):
        c = GroupedConv(self.store, name, width, groups, stride, self.gen)
        if self._side is not None:
            c.side_stream = self._side
        self.gconvs.append(c)
        return c

    def set_reference_fp32(self, on=True):
        """VERIFICATION ONLY.  Switch the storage of every activation / activation-gradient buffer to fp32: nbdt.ops then
        routes each launch on such a buffer to the plain fp32 kernel of the same meaning (csrc/ref_fp32.hip) while this
        engine keeps doing exactly what it does in production -- the same forward() / backward() code, launch order,
        two streams, events, rotating buffers, fused-statistics and CU-sharing protocol.  With fp32 storage a whole
        training step must agree with the fp32 oracle to ~1e-5; with bf16 storage the same path agrees to a gradient
        cosine of ~0.9 (mask flips from 1-ulp roundings).  The difference between the two is storage precision and
        nothing else -- that is the statement tests/test_reference_fp32_gpu.py makes.  Slow (one thread per output);
        small models and batches only.  Inference fusion (conv + folded BatchNorm) has no fp32 twin: eval-mode
        forwards run unfused."""
        self.join_side_stream()
        self.act_dtype = torch.float32 if on else torch.bfloat16
        self.fuse_eval = not on
        self._bufs = {}
        self._seg_ops = {}
        self._seg_skip = set()
        for c in self.convs:
            c._plans = {}
        self._share_calibrated = True        # (a timing decision between two schedules of the SLOW kernels means nothing)
        self.refresh_derived_weights()

    def set_overlap(self, on):
        """Turn the second (weight-gradient) stream on/off at run time; off = every launch on the caller's stream,
        so a kernel's event-bracketed duration is its own (bench.py's roofline pass)."""
        self.join_side_stream()
        for c in self.convs + self.gconvs + list(getattr(self, "dws", [])):
            c.side_stream = self._side if on else None
        self._overlap = bool(on)

    def set_cu_share(self, gbps_per_cu=47.0, target_us=200.0, min_cus=16, max_cus=128, join=False, calibrate=True,
                     split_reduce=True, split_target_us=190.0):
        """Run the BatchNorm-backward pass of every fused WRN unit BESIDE the weight gradient of the same conv, on
        disjoint CUs (gbps_per_cu=None: off -- weight gradients next to the data gradients, every pass on all CUs).
        WRNEngine turns this on at construction (calibrated, see below), so main.py / HipBackbone users and bench.py
        run the same schedule.

        Why it pays (probes/cu_share_probe.hip, profiles/r02_cu_share_probe.txt): the pass is HBM-bound and HBM needs
        few CUs -- one CU streams ~47 GB/s, 64 CUs 3.0 TB/s, all 256 5.6 TB/s -- while the MFMA-bound weight gradient
        loses LESS than its share of CUs when it gives some up, because the chip is power-limited (192 CUs deliver
        83 % of the 256-CU matrix rate, and a streaming kernel on the other 64 does not slow them).  The two kernels
        can never share a CU (a weight-gradient block takes its whole register file), so the split is by CU: the pass
        runs as n persistent one-per-CU blocks (nbdt_bn_bwd_apply_cus), the weight gradient is sized for the rest
        (nbdt_wgrad_desc.cu_budget).  n = bytes of the pass / (gbps_per_cu x target_us), clamped to
        [min_cus, max_cus] and then set by the weight gradient's actual block count per XCD (ops.plan_cu_share).
        split_reduce: the BatchNorm-backward SUMS move there too -- the data gradients run with their plain epilogue
        (the fused one reads the BatchNorm input in an HBM burst while the matrix pipes wait: 240 instead of 190 us
        per stage-1 launch) and the confined work becomes reduce + fold + apply (nbdt_bn_bwd_reduce_cus +
        nbdt_bn_bwd_apply_cus: 5-6 tensor passes instead of 3-4, so n is larger: split_target_us).  Same-box A/B at
        512 images: 19.25 ms per step without sharing, 18.45 with the fused sums, 17.55 with the split
        (profiles/r03_split_cu_share_ab.txt).
        join: wait for the weight gradient before the next data gradient (bounds the cost of an unbalanced pair to
        max(pass, weight gradient); measured 1 % slower when the pairs are balanced, so off by default).
        calibrate: calibrate_cu_share() runs before the first backward() at a new setting (or when the caller invokes
        it): it times the conv2 half of one stage-1 unit in the default order and in the order that would be used, on
        the engine's own buffers, and keeps the sharing only if it is faster -- e.g. not when the two streams were
        mapped to one hardware queue and cannot overlap at all, where a pass confined to 50 CUs costs 35 % of a step.
        Only the second stream the engine was created with is used: streams created later wrapped onto the main
        stream's hardware queue in one of four tries (measured), never the first one.
        The CU arithmetic is MI355X's (256 CUs = 8 XCDs x 32): on any other device the sharing stays off."""
        self.join_side_stream()
        self.cu_share_report = None
        self._share_join = bool(join)
        self._share_split = bool(split_reduce), float(split_target_us)
        if gbps_per_cu is not None and not ops.cu_topology_is_mi355x(self.device):
            self._cu_share = None
            self._share_calibrated = True
            self.cu_share_report = {"enabled": False, "reason": "not a 256-CU / 8-XCD device: the CU split is MI355X's"}
            return
        self._cu_share = None if gbps_per_cu is None else (float(gbps_per_cu), float(target_us),
                                                           max(8, int(min_cus)), int(max_cus))
        self._share_calibrated = not calibrate

    def _split_us(self, out):
        """Time budget of the confined reduce + apply of a stage, from a padded [B, H+2, W+2, C] tensor on its output grid:
        share_stage_us[H * W] (or set_cu_share's split_target_us), quoted at 512 images -- the weight gradient beside the pass lasts in proportion
        to the batch, so the pass's budget does too and the CU split does not depend on the batch (a 256-image shard with
        512-image microseconds gave its passes half the CUs: 10.6 instead of 9.3 ms per step)."""
        B, Hp, Wp, _ = out.shape
        return self.share_stage_us.get((Hp - 2) * (Wp - 2), self._share_split[1]) * (B / 512.0)

    def _pair_backward(self, conv, bn, form, g, a, t, ga, gt, share=None, tensors=0, gx_add=None):
        """Backward of a (conv, preceding BatchNorm) pair: g = dL/d(conv output) -> gt = dL/dt [+ gx_add], where the conv
        read a = relu(bn(t)) and ga = dL/da is the buffer between the two.  The order of these launches is the
        cross-stream protocol (weight gradients go to the second stream, see Conv._wgrad); every engine's pairs run here.
          "split"  data gradient with its plain epilogue; the weight gradient AFTER it, sized for 256 - n CUs; the whole
                   BatchNorm backward (sums, fold, elementwise pass) on n CUs beside it (needs `share`);
          "fused"  the data gradient's epilogue also emits bn's backward sums.  Without `share` the weight gradient is
                   issued first and the elementwise pass runs on all CUs; with it the weight gradient follows the data
                   gradient with a CU budget and the pass is confined to n CUs;
          "plain"  weight gradient, data gradient with its plain epilogue, the sums in a pass of their own on all CUs.
        share: None, or (gbps_per_cu, target_us, min_cus, max_cus) for ops.plan_cu_share, with `tensors` the tensor
        passes of the confined work over ga's elements."""
        if form == "plain":
            conv.backward_weight(a, g)
            conv.backward_data(g, ga)
            bn.backward(ga, None, t, gt, relu=True, gx_add=gx_add)   # mask recomputed from t: a not re-read
            return
        fused = form == "fused"
        assert fused or share is not None, "the split form is a CU-sharing form"
        partials = self.partials(t) if fused else None
        if fused and share is None:
            conv.backward_weight(a, g)
        conv.backward_data(g, ga, bn=bn if fused else None, bn_x=t if fused else None, partials=partials)
        n = 0
        if share is not None:
            B, Hp, Wp, C = ga.shape
            budget, n = ops.plan_cu_share(conv.plan(B, Hp - 2, Wp - 2)[3], B * (Hp - 2) * (Wp - 2) * C, tensors, *share)
            conv.backward_weight(a, g, cu_budget=budget)
        if fused:
            bn.backward_fused(ga, t, gt, partials, gx_add=gx_add, cus=n)
        else:
            bn.backward_cus(ga, t, gt, n, gx_add=gx_add)

    def _calibration_unit(self):
        """The unit whose conv2 pair the calibration times (subclasses with CU sharing override)."""
        return None

    def calibrate_cu_share(self, comm=None):
        """Decide whether the CU-sharing schedule set by set_cu_share() is kept on THIS box: time the conv2 half of one
        widest-tensor unit -- data gradient, BatchNorm backward, weight gradient, exactly the launches backward()
        would make -- in the default order and in the sharing order that is configured (split or fused sums), each
        4 times on the engine's own buffers (about 3 ms, once), and keep the sharing only if it is at least 6 %
        faster (the pair-to-step fit in the code below).  Needs a training-mode forward() at the batch size that will be trained (it uses that forward's
        activations and BatchNorm statistics); backward() calls it before its first launch when a new setting has not
        been calibrated yet.  It synchronises with the host, so it must not run inside a hipGraph capture (GraphedStep
        warms up, and thereby calibrates, before it captures).
        comm (a GradComm of more than one rank): every rank measures, rank 0's decision is broadcast and adopted by
        all, so the ranks of a data-parallel job never run different schedules (the slowest would set the pace)."""
        self._share_calibrated = True
        if self._cu_share is None:
            return self.cu_share_report
        if ops.is_deterministic():
            # The keep/discard decision is a TIMING measurement, and the two schedules sum the BatchNorm-backward
            # reductions in different orders: a run-to-run different decision would break "same launches + same
            # inputs => same bits".  Deterministic mode therefore pins the configured schedule and measures nothing.
            self.cu_share_report = {"enabled": True, "decided_by": "deterministic mode (schedule pinned, not timed)"}
            return self.cu_share_report
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("calibrate_cu_share() synchronises with the host: call it (or run one eager step) "
                               "before capturing the step in a hipGraph")
        u = self._calibration_unit()
        if u is None or self._side is None or self._B is None:
            self._cu_share = None
            self.cu_share_report = {"enabled": False, "reason": "no unit / second stream / forward to calibrate on"}
            return self.cu_share_report
        B = self._B
        k, cout = u["key"], _pad32(u["cout"])
        x_out = u["x_out"]
        h, w = x_out.shape[1] - 2, x_out.shape[2] - 2
        conv, bn = u["conv2"], u["bn2"]
        a2, t = self.buf(k + ".a2", B, h, w, cout), self.buf(k + ".t", B, h, w, cout)
        ga2, gt = self.buf(f"ga2_{cout}", B, h, w, cout), self.buf(f"gt_{cout}_0", B, h, w, cout)
        g = self.buf(f"g_in{cout}_{h}_0", B, h, w, cout)      # backward() rewrites all three before it reads them
        # (plumbing: a one-off fill so the MFMAs see real data -- from a private generator: the caller's global
        # RNG stream is not advanced by a calibration)
        ops.interior(g).normal_(0.0, 1e-3, generator=torch.Generator(device=self.device).manual_seed(0x5eed))
        split, split_us = self._share_split[0], self._split_us(t)
        elements = B * h * w * cout
        gbps, us, lo, hi_cus = self._cu_share
        desc = conv.plan(B, h, w)[3]
        budget, n = ops.plan_cu_share(desc, elements, 5 if split else 3, gbps, split_us if split else us, lo, hi_cus)
        main = torch.cuda.current_stream(self.device)
        dw = torch.zeros_like(self.store.g(conv.name))
        dsum = torch.empty(2 * bn.C, device=self.device)
        dg, db = torch.zeros(bn.C, device=self.device), torch.zeros(bn.C, device=self.device)
        partials = self.partials(t)
        plan = conv.plan(B, h, w)
        d_plain = plan[1][0]

        def dgrad(fused):
            if fused:
                ops.conv_igemm_bnbwd(d_plain, g, conv.wd, ga2, t, bn.mean, bn.rstd, bn.gamma, bn.beta, partials)
            else:
                ops.conv_igemm(d_plain, g, conv.wd, ga2)

        def wgrad_side(cu_budget):
            self._side.wait_stream(main)
            with torch.cuda.stream(self._side):
                ops.conv_wgrad(desc, a2, g, dw, cu_budget)

        def default_order():        # what backward() does with set_cu_share(None)
            wgrad_side(0)
            dgrad(True)
            ops.bn_bwd_fused(ga2, t, bn.mean, bn.rstd, bn.gamma, bn.beta, partials, dsum, dg, db, gt)
            main.wait_stream(self._side)

        def sharing_order():
            dgrad(not split)
            wgrad_side(budget)
            if split:
                ops.bn_bwd_cus(ga2, t, bn.mean, bn.rstd, bn.gamma, bn.beta, self.slot_pair(bn.C), dsum, dg, db, gt, n)
            else:
                ops.bn_bwd_fused(ga2, t, bn.mean, bn.rstd, bn.gamma, bn.beta, partials, dsum, dg, db, gt, cus=n)
            main.wait_stream(self._side)

        def best_us(fn):
            best = float("inf")
            for _ in range(4):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(main)
                fn()
                e1.record(main)
                e1.synchronize()
                best = min(best, e0.elapsed_time(e1) * 1e3)
            return best

        t_default, t_share = best_us(default_order), best_us(sharing_order)
        # The isolated pair overstates what the whole step gains: in the default order a weight gradient already hides
        # under the NEXT data gradient, which one pair cannot show.  Measured on WRN-28-10 (scratch/share_by_batch.py;
        # round 4, after the epilogue statistics stopped costing the default order's data gradients 40 us each:
        # profiles/r04_share_by_batch.txt): pair 4.7 % SLOWER -> step 10 % slower (128 images); pair 8-10 % faster ->
        # step +2.7 ... +3.7 % (256); 18 % -> +5.7 % (384); 29 % -> +12.7 % (512) -- break-even near 5 %, so the
        # sharing is kept from 6 % up (round 3's data put the break-even at 8 %).
        keep = t_share < 0.94 * t_default
        decided_by = "this rank"
        if comm is not None and comm.world_size > 1:
            keep = comm.broadcast_flag(keep, self.device)
            decided_by = "rank 0 (broadcast)"
        self.cu_share_report = {"pass_cus": n, "wgrad_cu_budget": budget, "default_order_us": round(t_default, 1),
                                "sharing_order_us": round(t_share, 1), "enabled": bool(keep), "decided_by": decided_by,
                                "timed": f"conv2 half of unit {k} (data gradient + BatchNorm backward + weight "
                                         f"gradient) at batch {B}",
                                "bn_sums": "beside the weight gradient (nbdt_bn_bwd_reduce_cus)" if split
                                           else "data-gradient epilogue"}
        if not keep:
            self._cu_share = None
        return self.cu_share_report

    def _reserve_for(self, comm):
        """While gradient buckets are in flight the collective's kernels hold `comm.reserved_cus` CUs (one RCCL block
        per channel): the one-block-per-CU MFMA launches that follow are sized for the rest (ops.set_reserved_cus), so
        none of their persistent blocks waits for a CU an all-reduce block holds.  comm=None: back to the whole chip."""
        n = int(getattr(comm, "reserved_cus", 0) or 0) if comm is not None else 0
        if n != self._reserved_now:
            ops.set_reserved_cus(n)
            self._reserved_now = n

    def join_side_stream(self):
        """Order every weight-gradient launch issued on the side stream before what follows on the main one."""
        if self._side is not None:
            torch.cuda.current_stream(self.device).wait_stream(self._side)

    # ---- what every engine's forward() / backward() does around its own launches
    bucket_units = ()   # keys of the units after whose backward grad_buckets()[0] and [1] are complete

    def _input(self, img):
        """The image as contiguous fp32, remembered with its batch size for backward()."""
        if img.dtype != torch.float32 or not img.is_contiguous():
            img = img.float().contiguous()
        self._img, self._B = img, img.shape[0]
        return img

    def _pool_head(self, x, mean, rstd, gamma, beta, head):
        """Global pooling of relu(bn(x)) into [B, feat_c], then the classifier (head=False: the pooled features)."""
        B = self._B
        self._pooled = self._tensor("pooled", (B, self.feat_c))
        ops.bn_relu_pool(x, mean, rstd, gamma, beta, self._pooled)
        if not head:
            return self._pooled
        z = self._tensor("z", (B, self.num_classes))
        w, b = self.classifier_names
        ops.linear_fwd(self._pooled, self.store.p(w), self.store.p(b), z)
        return z

    def _head_backward(self, gz, gpooled):
        """dL/dpooled: `gpooled` after forward(head=False) (the fused head kernel already accumulated the classifier's
        gradients), else the classifier's backward from gz = dL/dz."""
        if gpooled is not None:
            return gpooled
        gz = gz.contiguous()
        gpool = self._tensor("gpool", (self._B, self.feat_c))
        w, b = self.classifier_names
        ops.linear_bwd(self._pooled, self.store.p(w), gz, gpool, self.store.g(w), self.store.g(b))
        return gpool

    def _begin_backward(self, comm):
        self._grad_is_zero = False   # this call accumulates into the gradient buffer
        self.join_side_stream()      # dgrad weight copies (built on the second stream after the last update)
        if self._cu_share is not None and not self._share_calibrated:
            self.calibrate_cu_share(comm)      # once per set_cu_share(): keep the sharing only if it is faster here
        self.reset_slot_pairs()      # the confined BatchNorm backward's slot buffers start every step from (zero, zero)

    def _units_backward(self, units, comm):
        """(i, unit) for `units` in reverse order, with the cross-stream protocol around each unit's launches.

        Gradient buffers are shared between units, and a weight gradient still running on the side stream may be reading
        what a later unit is about to overwrite.  Joining the side stream at the top of every unit would order that, but
        it makes the main stream wait for the weight gradient issued LAST (~70 us of a 1 ms WRN unit with 96 CUs idle:
        0.95 ms of launch gaps per backward in profiles/r03_split_*two_streams*).  Instead the main stream waits for
        everything the side stream had been given ONE UNIT AGO (an event recorded at the top of the previous unit), and
        each engine rotates the buffers a weight gradient reads so that unit i never writes what unit i - 1's may still
        be reading (i is the unit's position in this order).  After each unit named in `bucket_units` the side stream is
        joined and that unit's gradient bucket is all-reduced (comm: a GradComm, or None)."""
        main = torch.cuda.current_stream(self.device)
        two_streams = self._side is not None and self._overlap
        if two_streams:      # (also forks the side stream into a hipGraph capture before its first event is recorded)
            self._side.wait_stream(main)
        buckets = self.grad_buckets() if comm is not None else None
        side_mark = None
        for i, u in enumerate(reversed(units)):
            if two_streams:
                if side_mark is not None:
                    main.wait_event(side_mark)
                side_mark = torch.cuda.Event()
                side_mark.record(self._side)
            yield i, u
            if comm is not None and u["key"] in self.bucket_units:
                self.join_side_stream()
                comm.reduce_range(self.store.grad, *buckets[self.bucket_units.index(u["key"])])
                self._reserve_for(comm)

    def _end_backward(self, comm):
        self.join_side_stream()      # every gradient is complete on the caller's stream when backward returns
        if comm is not None:
            comm.reduce_range(self.store.grad, *self.grad_buckets()[2])
            comm.finish(self.store.grad)
            self._reserve_for(None)

    bn_eps = ops.BN_EPS        # an engine whose BatchNorms use another eps sets it before it builds them

    def bn(self, name, c, gamma=1.0):
        b = BatchNorm(self.store, name, c, self, gamma, eps=self.bn_eps)
        self.bns.append(b)
        return b

    def finalize(self):
        self.store.finalize()
        # one flat buffer for every conv's data-gradient weight copy + the layer table of the batched
        # transpose kernel (one launch per optimizer step instead of one per layer)
        total = sum(c.numel() for c in self.convs)
        self._wd_flat = torch.empty(total, dtype=torch.bfloat16, device=self.device)
        rows, off, tiles = [], 0, 0
        for c in self.convs:
            rows.append([self.store.entries[c.name][0], off, c.cout, c.taps, c.cin, tiles])
            c.wd = self._wd_flat[off:off + c.numel()].view(c.cin, c.taps, c.cout)
            off += c.numel()
            tiles += c.taps * ((c.cout + 63) // 64) * (c.cin // 32)
        # nbdt_weight_prep_batched takes at most 64 layers per launch: one launch up to there (ResNet50: 53 convs), one per 64
        # layers beyond (the 101-layer nets: 71 .. 155), each with its own first-tile numbering
        self._wd_chunks = []
        for i in range(0, len(rows), self.WD_CHUNK):
            part = rows[i:i + self.WD_CHUNK]
            end = rows[i + self.WD_CHUNK][5] if i + self.WD_CHUNK < len(rows) else tiles
            table = torch.tensor([r[:5] + [r[5] - part[0][5]] for r in part], dtype=torch.int64, device=self.device)
            self._wd_chunks.append((table, len(part), end - part[0][5]))
        # DMA-ordered weight tiles for the dense 3x3 / stride-1 kernel (forward weights from the bf16 mirror, data-
        # gradient weights from the transposed copy): one 1-KiB LDS-DMA instruction then reads one contiguous KiB
        dense = [c for c in self.convs if c.k == 3 and c.stride == 1]
        self._wt_n = len(dense)
        if dense:
            n_el = sum(c.numel() for c in dense)
            self._wt_fwd = torch.empty(n_el, dtype=torch.bfloat16, device=self.device)
            self._wt_dgrad = torch.empty(n_el, dtype=torch.bfloat16, device=self.device)
            frows, drows, off, tf, td = [], [], 0, 0, 0

            def ntile(r):
                r32 = r // 32
                return 5 if r32 % 5 == 0 else 4 if r32 % 4 == 0 else 2 if r32 % 2 == 0 else 1

            wd_off = {}
            o = 0
            for c in self.convs:
                wd_off[c.name] = o
                o += c.numel()
            for c in dense:
                frows.append([self.store.entries[c.name][0], off, c.cout, c.cin, tf])
                drows.append([wd_off[c.name], off, c.cin, c.cout, td])
                c.wt_fwd = self._wt_fwd[off:off + c.numel()]
                c.wt_dgrad = self._wt_dgrad[off:off + c.numel()]
                off += c.numel()
                tf += (c.cout // (32 * ntile(c.cout))) * (c.cin // 32) * 9
                td += (c.cin // (32 * ntile(c.cin))) * (c.cout // 32) * 9
            self._wt_ftable = torch.tensor(frows, dtype=torch.int64, device=self.device)
            self._wt_dtable = torch.tensor(drows, dtype=torch.int64, device=self.device)
            self._wt_ftotal, self._wt_dtotal = tf, td
        # grouped 3x3 convs: the expanded block-diagonal forward / data-gradient blocks of all of them, one table
        if self.gconvs:
            n_el = sum(c.numel() for c in self.gconvs)
            self._gw_fwd = torch.empty(n_el, dtype=torch.bfloat16, device=self.device)
            self._gw_dgrad = torch.empty(n_el, dtype=torch.bfloat16, device=self.device)
            rows, off, first = [], 0, 0
            for c in self.gconvs:
                rows.append([self.store.entries[c.name][0], off, c.width, c.cg, first])
                c.wf = self._gw_fwd[off:off + c.numel()]
                c.wd = self._gw_dgrad[off:off + c.numel()]
                off += c.numel()
                first += c.width // 32
            self._gw_table = torch.tensor(rows, dtype=torch.int64, device=self.device)
            self._gw_total = first
        self.refresh_derived_weights()

    WD_CHUNK = 64     # layers per nbdt_weight_prep_batched launch (the entry's limit)

    def _prep_dgrad_copies(self):
        for table, n, tiles in self._wd_chunks:
            ops.weight_prep_batched(self.store.flat, table, n, tiles, self._wd_flat)

    def _prep_grouped(self, dgrad):
        """The grouped convs' forward blocks (needed by the very next forward: caller's stream) or data-gradient blocks
        (wherever the dense data-gradient copies are built)."""
        if self.gconvs:
            ops.conv_group_weight_prep_batched(self.store.flat, self._gw_table, len(self.gconvs), self._gw_total,
                                               wf_flat=None if dgrad else self._gw_fwd,
                                               wd_flat=self._gw_dgrad if dgrad else None)

    def refresh_derived_weights(self):
        for b in self.bns:             # gamma / beta may have changed: drop the folded eval transforms
            b._affine = None
        if self.act_dtype == torch.float32:      # reference mode: fp32 data-gradient weights (plumbing on parameters)
            for c in self.convs:
                c.wd32 = self.store.p(c.name).flip(1).permute(2, 1, 0).contiguous()
        if self._wt_n:     # forward tiles are needed by the very next forward: caller's stream
            ops.weight_tile_batched(self.store.bf16, self._wt_ftable, self._wt_n, self._wt_ftotal, self._wt_fwd)
        self._retile_seg(False)
        self._prep_grouped(False)
        if self._side is None or not self._overlap:
            self._prep_dgrad_copies()
            if self._wt_n:
                ops.weight_tile_batched(self._wd_flat, self._wt_dtable, self._wt_n, self._wt_dtotal, self._wt_dgrad)
            self._retile_seg(True)
            self._prep_grouped(True)
            return
        # the transposed copies are only read by data-gradient launches: build them on the second stream while
        # the next forward runs (backward() joins the stream before its first dgrad)
        self._side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self._side):
            self._prep_dgrad_copies()
            if self._wt_n:
                ops.weight_tile_batched(self._wd_flat, self._wt_dtable, self._wt_n, self._wt_dtotal, self._wt_dgrad)
            self._retile_seg(True)
            self._prep_grouped(True)

    def optimizer_step(self, lr, momentum, weight_decay, config=None, grad_scale=1.0, zero_grad=False):
        """The optimizer pass over every parameter + refresh of bf16 / dgrad weights: what sgd_step (config None),
        lars_step (a LarsConfig), adamw_step (an AdamWConfig) and rmsprop_step (an RMSpropConfig) wrap and train_step
        calls.  No host synchronisation.  zero_grad: the same pass leaves the gradient buffer zeroed, and the next
        zero_grad() is then free (the separate 146 MB fill took 108 us per WRN-28-10 step; train_step asks for it)."""
        adaptive = isinstance(config, (AdamWConfig, RMSpropConfig))
        what = ("sgd_step" if config is None else "adamw_step" if isinstance(config, AdamWConfig) else
                "rmsprop_step" if adaptive else "lars_step")
        if self.ema_swapped:
            raise RuntimeError(_EMA_SWAPPED % what)
        s = self.store
        if adaptive:
            owner = "adamw" if what == "adamw_step" else "rmsprop_tf" if config.tf else "rmsprop"
            if self._opt_owner not in (None, owner):
                raise RuntimeError(f"{what}: store.mom and store.sq hold the state of {self._opt_owner}; call "
                                   "reset_optimizer_state() before changing the optimizer")
            if self._opt_owner is None:      # the second state arena at first use
                s.init_sq(ones=owner == "rmsprop_tf")
                self._opt_owner = owner
        self.join_side_stream()
        if config is None:
            ops.sgd_step(s.flat, s.grad, s.mom, lr, momentum, weight_decay, grad_scale, s.bf16, zero_grad=zero_grad)
        else:
            cls, wd, rule = ops.ArenaOptPlan if adaptive else ops.LarsPlan, float(weight_decay), bool(config.exclude_1d)
            plan = self._plans.get((cls, wd, rule))
            if plan is None:         # host tables built and copied to the device once per (pass, decay, rule)
                plan = self._plans[cls, wd, rule] = cls(s.flat.numel(), s.segments(wd, rule), device=self.device)
            if not adaptive:
                plan.step(s.flat, s.grad, s.mom, lr, momentum, config.trust, config.eps, grad_scale, s.bf16,
                          zero_grad=zero_grad)
                self._lars_last = plan
            else:
                self.opt_steps += 1
                if what == "adamw_step":
                    plan.adamw(s.flat, s.grad, s.mom, s.sq, lr, config.betas, config.eps, self.opt_steps, grad_scale,
                               s.bf16, zero_grad=zero_grad)
                else:
                    plan.rmsprop(s.flat, s.grad, s.sq, s.mom, lr, config.alpha, config.eps, momentum, config.tf,
                                 grad_scale, s.bf16, zero_grad=zero_grad)
        self._grad_is_zero = bool(zero_grad)
        self.refresh_derived_weights()

    def sgd_step(self, lr, momentum=0.9, weight_decay=5e-4, grad_scale=1.0, zero_grad=False):
        """optim.SGD step over every parameter (main.py:207); zero_grad as in optimizer_step."""
        self.optimizer_step(lr, momentum, weight_decay, None, grad_scale, zero_grad)

    def lars_step(self, lr, momentum=0.9, weight_decay=5e-4, trust=1e-3, eps=1e-8, grad_scale=1.0, zero_grad=False,
                  exclude_1d=True):
        """LARS step over every parameter (You et al. 2017: SGD with momentum on ratio * (g + wd * p), the ratio per
        ParamStore entry; nbdt_lars_step).  Three launches whatever the number of parameters.  exclude_1d: BatchNorm
        parameters and biases take plain SGD steps without decay."""
        self.optimizer_step(lr, momentum, weight_decay, LarsConfig(trust, eps, exclude_1d), grad_scale, zero_grad)

    def adamw_step(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0, zero_grad=False,
                   exclude_1d=True):
        """torch.optim.AdamW step over every parameter (decoupled decay per ParamStore entry, no amsgrad; nbdt_adamw_step).
        One launch.  m lives in store.mom, v in store.sq (allocated at the first adaptive step); the bias corrections
        take opt_steps.  exclude_1d: BatchNorm parameters and biases are not decayed.  A step after sgd_step / lars_step
        on the same engine wants reset_optimizer_state() first: store.mom then still holds their momentum."""
        self.optimizer_step(lr, None, weight_decay, AdamWConfig(betas, eps, exclude_1d), grad_scale, zero_grad)

    def rmsprop_step(self, lr, alpha=0.99, eps=1e-8, momentum=0.9, weight_decay=5e-4, tf=False, grad_scale=1.0,
                     zero_grad=False, exclude_1d=True):
        """torch.optim.RMSprop step (not centered; the decay enters the gradient) or, with tf, TensorFlow's -- eps inside
        the root, lr inside the momentum buffer, the mean square started at 1: the form EfficientNet was trained with
        (alpha 0.9, momentum 0.9, eps 1e-3) -- over every parameter (nbdt_rmsprop_step).  One launch.  The buffer lives
        in store.mom, the mean square in store.sq."""
        self.optimizer_step(lr, momentum, weight_decay, RMSpropConfig(alpha, eps, tf, exclude_1d), grad_scale, zero_grad)

    def clip_grad_norm(self, max_norm, grad_scale=1.0):
        """torch.nn.utils.clip_grad_norm_ over every parameter's gradient, on the device: the global norm of grad_scale *
        store.grad (nbdt_clip_norm, two launches) and, only where it exceeds max_norm, one scaling pass over store.grad
        (nbdt_clip_apply).  No host synchronisation: the coefficient stays in the plan's device record (clip_stats reads
        it).  Runs between backward() and the optimizer step, which takes the same grad_scale."""
        if not (math.isfinite(max_norm) and max_norm > 0.0):
            raise ValueError(f"clip_grad_norm: max_norm must be finite and > 0, got {max_norm}")
        self.join_side_stream()      # weight gradients still running on the second stream write store.grad
        g = self.store.grad
        if self._clip_plan is None:
            self._clip_plan = ops.ClipPlan(g.numel(), device=self.device)
        self._clip_plan.norm(g, grad_scale, max_norm)
        self._clip_plan.apply(g)

    def clip_stats(self):
        """{norm, coef, clipped, steps, nonfinite, total_clipped} of the clip_grad_norm calls so far: the last call's norm
        and coefficient, the counts over all of them.  Copies from the device and waits for it: for logging and tests."""
        if self._clip_plan is None:
            raise RuntimeError("clip_stats: no clip_grad_norm yet")
        return self._clip_plan.to_host()

    def calibrate_pending(self, comm):
        """Run the CU-sharing calibration now if the next backward() would: a caller whose first backward must not reduce
        gradients (train_step's leading micro-batches) still hands the calibration its communicator, so every rank adopts
        rank 0's schedule."""
        if self._cu_share is not None and not self._share_calibrated:
            self.join_side_stream()
            self.calibrate_cu_share(comm)

    def reset_optimizer_state(self):
        """Forget every optimizer's state: store.mom and store.sq (if it exists) zeroed, opt_steps = 0; the next adaptive
        step owns the state and gives store.sq its own start (ones inside the segments for TensorFlow's RMSprop).
        Required between two different adaptive optimizers on one engine."""
        self.join_side_stream()
        self.store.mom.zero_()
        if self.store.sq is not None:
            self.store.sq.zero_()
        self._opt_owner = None
        self.opt_steps = 0

    def last_trust_ratios(self):
        """ParamStore entry name -> trust ratio of the last lars_step (1 for entries it did not adapt).  Copies from the
        device and waits for it: for logging and tests, not for the step path."""
        if self._lars_last is None:
            raise RuntimeError("last_trust_ratios: no lars_step yet")
        return dict(zip(self.store.segment_names(), self._lars_last.ratios().tolist()))

    # ---- exponential moving average of the weights
    def ema_enable(self, decay=0.9999, warmup=True):
        """Start averaging: the shadow of the parameter arena (store.ema) and ONE flat shadow of every BatchNorm's running
        statistics begin as copies of the live values, ema_updates = 0.  Calling it again re-initialises the average.
        decay, warmup: what ema_update hands to ema_decay_at."""
        if self.ema_swapped:
            raise RuntimeError("ema_enable: the average is swapped into the weights (ema_swap / ema_weights); swap back first")
        s = self.store
        s.ema = s.flat.clone()
        self._ema_stats = torch.empty(sum(2 * b.C for b in self.bns), dtype=torch.float32, device=self.device)
        pairs, off = [], 0
        for b in self.bns:
            for live in (b.running_mean, b.running_var):
                shadow = self._ema_stats[off:off + b.C]
                shadow.copy_(live)
                pairs.append((live, shadow))
                off += b.C
        self._ema_table = ops.EmaTable(pairs, self.device) if pairs else None
        self._ema_nbt = [b.num_batches_tracked for b in self.bns]    # host ints: the counters as of the last update
        self.ema_decay, self.ema_warmup, self.ema_updates = float(decay), bool(warmup), 0

    @staticmethod
    def ema_decay_at(t, decay=0.9999, warmup=True):
        """The decay of the update that follows t earlier ones, in double: min(decay, (1 + t) / (10 + t)) with warm-up (the
        ramp of tf.train.ExponentialMovingAverage(num_updates=) and timm's ModelEmaV3), else `decay`.  Host only.  The
        kernel takes float32(1 - d)."""
        return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)

    def _ema_require(self, what):
        if self.store.ema is None:
            raise RuntimeError(f"{what}: no average is kept (call ema_enable first)")

    def ema_update(self):
        """e += (1 - d) * (p - e) over the parameter arena and over every running statistic, d = ema_decay_at(ema_updates):
        two launches on the current stream, no host synchronisation.  They only read the live values, so nothing the
        second stream still does with them has to be waited for.  The caller issues it after train_step / a GraphedStep."""
        self._ema_require("ema_update")
        if self.ema_swapped:
            raise RuntimeError(_EMA_SWAPPED % "ema_update")
        omd = 1.0 - self.ema_decay_at(self.ema_updates, self.ema_decay, self.ema_warmup)   # (ctypes rounds it to fp32)
        ops.ema_update(self.store.flat, self.store.ema, omd)
        if self._ema_table is not None:
            self._ema_table.update(omd)
        self._ema_nbt = [b.num_batches_tracked for b in self.bns]
        self.ema_updates += 1

    def ema_swap(self):
        """Exchange the live weights and running statistics with their averages IN PLACE (the facade's parameters, the
        named views and BatchNorm.running_mean / running_var alias the live tensors), write the bf16 mirror of what the
        arena now holds in the same pass, exchange the host counters, and rebuild every derived weight copy.  Flips
        ema_swapped; while it is set, the optimizer steps and ema_update raise."""
        self._ema_require("ema_swap")
        self.join_side_stream()          # the second stream may still be reading flat (the transposed copies)
        s = self.store
        ops.ema_swap(s.flat, s.ema, s.bf16)
        if self._ema_table is not None:
            self._ema_table.swap()
        live = [b.num_batches_tracked for b in self.bns]
        for b, k in zip(self.bns, self._ema_nbt):
            b.num_batches_tracked = k
        self._ema_nbt = live
        self.ema_swapped = not self.ema_swapped
        self.refresh_derived_weights()

    @contextlib.contextmanager
    def ema_weights(self):
        """with engine.ema_weights(): forward() / the facade evaluate the averaged weights; swapped back on exit, also when
        the body raises."""
        self.ema_swap()
        try:
            yield self
        finally:
            self.ema_swap()

    def _ema_stat_views(self):
        out, off = {}, 0
        for b, k in zip(self.bns, self._ema_nbt):
            out[b.name + ".running_mean"] = self._ema_stats[off:off + b.c_real]
            out[b.name + ".running_var"] = self._ema_stats[off + b.C:off + b.C + b.c_real]
            out[b.name + ".num_batches_tracked"] = torch.tensor(k, dtype=torch.long)
            off += 2 * b.C
        return out

    def ema_state_dict(self):
        """The average under state_dict()'s keys and logical shapes, whichever side it currently lives on."""
        self._ema_require("ema_state_dict")
        if self.ema_swapped:
            return self.state_dict()
        out = {k: v.detach().clone().contiguous() for k, v in self.named_params("ema").items()}
        out.update({k: v.detach().clone() for k, v in self._ema_stat_views().items()})
        return out

    def load_ema_state_dict(self, sd):
        """Copy a reference-named state dict into the average, whichever side it currently lives on."""
        self._ema_require("load_ema_state_dict")
        if self.ema_swapped:
            return self.load_state_dict(sd)
        params, bufs = self.named_params("ema"), self._ema_stat_views()
        missing = {m for m in (set(params) | set(bufs)) - set(sd) if not m.endswith("num_batches_tracked")}
        if missing:
            raise KeyError(f"state dict is missing {sorted(missing)[:5]} ...")
        for name, view in list(params.items()) + list(bufs.items()):
            if not name.endswith("num_batches_tracked"):
                view.copy_(sd[name].to(self.device))
        self._ema_nbt = [int(sd.get(b.name + ".num_batches_tracked", k)) for b, k in zip(self.bns, self._ema_nbt)]

    def zero_grad(self):
        if not self._grad_is_zero:
            self.store.zero_grad()
        self._grad_is_zero = False       # whatever runs next may accumulate into it

    # ---- logical (reference-named) parameter / buffer views for state_dict compatibility
    def extra_param_views(self, buf):
        """name -> view for parameters that are not Conv/BatchNorm objects (stem, classifier)."""
        return {}

    def named_params(self, which="flat"):
        buf = {"flat": self.store.flat, "grad": self.store.grad, "bf16": self.store.bf16, "ema": self.store.ema}[which]
        out = dict(self.extra_param_views(buf))
        for c in self.convs + self.gconvs:
            out[c.name] = c.logical(buf)
        for b in self.bns:
            out[b.name + ".weight"] = self.store._view(buf, b.name + ".weight")[:b.c_real]
            out[b.name + ".bias"] = self.store._view(buf, b.name + ".bias")[:b.c_real]
        return out

    def named_buffers(self):
        out = {}
        for b in self.bns:
            out[b.name + ".running_mean"] = b.running_mean[:b.c_real]
            out[b.name + ".running_var"] = b.running_var[:b.c_real]
            out[b.name + ".num_batches_tracked"] = torch.tensor(b.num_batches_tracked, dtype=torch.long)
        return out

    def load_state_dict(self, sd):
        """Copy a reference-named state dict (fp32 tensors, any device) into the engine."""
        params, bufs = self.named_params("flat"), self.named_buffers()
        missing = {m for m in (set(params) | set(bufs)) - set(sd) if not m.endswith("num_batches_tracked")}
        if missing:
            raise KeyError(f"state dict is missing {sorted(missing)[:5]} ...")
        for name, view in list(params.items()) + list(bufs.items()):
            if name in sd and not name.endswith("num_batches_tracked"):
                view.copy_(sd[name].to(self.device))
        for b in self.bns:
            if b.name + ".num_batches_tracked" in sd:
                b.num_batches_tracked = int(sd[b.name + ".num_batches_tracked"])
        self.store.refresh_bf16()
        self.refresh_derived_weights()

    def state_dict(self):
        out = {k: v.detach().clone().contiguous() for k, v in self.named_params("flat").items()}
        out.update({k: v.detach().clone() for k, v in self.named_buffers().items()})
        return out

    def _tensor(self, key, shape):
        k = (key,) + tuple(shape)
        if k not in self._bufs:
            self._bufs[k] = torch.empty(shape, dtype=torch.float32, device=self.device)
        return self._bufs[k]

    def _zeroed(self, key, shape):
        """fp32 accumulator under the zero-on-entry / re-zeroed-by-the-last-reader contract (like the BatchNorm slots)."""
        k = (key, "zeroed") + tuple(shape)
        if k not in self._bufs:
            self._bufs[k] = torch.zeros(shape, dtype=torch.float32, device=self.device)
        return self._bufs[k]


class WRNEngine(_Engine):
    """Pre-activation WideResNet (pytorchcv ``CIFARWRN``: wrn28_10_cifar10/100, reference
    nbdt/models/wideresnet.py:1-5).  State-dict names follow pytorchcv."""

    def __init__(self, num_classes=10, blocks=28, width_factor=10, in_size=(32, 32), device="cuda", seed=0):
        super().__init__(device, seed)
        assert (blocks - 4) % 6 == 0
        self.num_classes = num_classes
        self.in_size = in_size
        layers = [(blocks - 4) // 6] * 3
        widths = [16 * width_factor, 32 * width_factor, 64 * width_factor]
        self.stem_c = 16
        self.stem_cpad = _pad32(16)
        gen = self.gen
        bound = math.sqrt(2.0) * math.sqrt(3.0 / 27)
        self.store.add("features.init_block.weight", (self.stem_c, 3, 3, 3),
                       lambda v: v.uniform_(-bound, bound, generator=gen))
        self.units = []
        cin = 16
        for i, (n, cout) in enumerate(zip(layers, widths)):
            for j in range(n):
                stride = 2 if (j == 0 and i != 0) else 1
                pre = f"features.stage{i + 1}.unit{j + 1}."
                u = {
                    "bn1": self.bn(pre + "body.conv1.bn", cin),
                    "conv1": self.conv(pre + "body.conv1.conv.weight", cin, cout, 3, stride),
                    "bn2": self.bn(pre + "body.conv2.bn", cout),
                    "conv2": self.conv(pre + "body.conv2.conv.weight", cout, cout, 3, 1),
                    "idconv": (self.conv(pre + "identity_conv.weight", cin, cout, 1, stride)
                               if (cin != cout or stride != 1) else None),
                    "cin": cin, "cout": cout, "stride": stride, "key": f"s{i + 1}u{j + 1}",
                    "seg": False,    # forward(): this unit ran on the slice-list kernel (training mode, shortcut conv)
                }
                self.units.append(u)
                cin = cout
        self.feat_c = cin
        self.post_bn = self.bn("features.post_activ.bn", cin)
        kb = 1.0 / math.sqrt(cin)   # nn.Linear default init
        self.store.add("output.weight", (num_classes, cin), lambda v: v.uniform_(-kb, kb, generator=gen))
        self.store.add("output.bias", (num_classes,), lambda v: v.uniform_(-kb, kb, generator=gen))
        self.finalize()
        self._img = None
        # Weight gradients on a second HIP stream: a wgrad block (55 KB LDS, 4 waves) and a 256-pixel igemm block
        # (76 KB, 4 waves) fit on one CU together, and the two kernels stall on different things, so running
        # conv.wgrad next to the dgrad / BatchNorm-backward chain instead of in front of it is worth 3.9 % of the
        # step (21.62 -> 20.80 ms, same-box A/B; engine.set_overlap(False) restores the single-stream order).
        self._side = side_stream(self.device)     # engine.set_overlap(False) puts everything back
        for c in self.convs:                                   # on the caller's stream (profiling passes)
            c.side_stream = self._side
        # BatchNorm-backward passes beside the weight gradients on disjoint CUs: on by default, kept only if the
        # calibration before the first backward() finds it faster on this box (set_cu_share(None) turns it off)
        self.set_cu_share(47.0)
        # per stage (output-grid pixels -> split_target_us, quoted at 512 images): the 32x32 and 16x16 stages are bound by the
        # main stream's chain (data gradient, then the confined reduce + apply), the 8x8 stage by its MFMA work.  With plain
        # loads in the passes the chain-bound stages wanted more CUs (170 / 150 us: 104-120 / 72); with the nontemporal loads
        # of round 6 the passes are faster and 190 / 170 us (96-112 / 56-72 CUs) is best again -- the value of the per-stage
        # table is now the batch scaling (_split_us) and a place to retune (profiles/r06_stage_target_ab.txt, sections 1-5)
        self.share_stage_us = {1024: 190.0, 256: 170.0}

    # ---- the shape-changing units on the slice-list kernel (csrc/conv_seg.hip)
    def _seg_conv1(self, u, B, h, w):
        """stride-2 conv1 forward over the space-to-depth a1."""
        c = u["conv1"]
        return self.seg_op((u["key"], "conv1", B, h, w), lambda: ops.seg_fwd_s2(B, h, w, c.cin, c.cout),
                           lambda: [self.store.pb(c.name).view(c.cout, 9 * c.cin)],
                           lambda: [self.store.p(c.name).view(c.cout, 9 * c.cin)])

    def _seg_conv2_sc(self, u, B, ho, wo):
        """conv2 + shortcut in one launch (the residual add disappears into the K loop); None where the plan would fall
        back to 256-pixel half tiles (8x8 grids cannot hold three halo buffers of a 512-pixel tile: the dense kernel + a
        separate 1x1 launch are faster there)."""
        c2, ci = u["conv2"], u["idconv"]
        key = (u["key"], "conv2sc", B, ho, wo)
        if key in self._seg_ops:
            return self._seg_ops[key]
        if key in self._seg_skip:
            return None
        try:
            plan = ops.seg_conv3x3_plus_1x1(B, ho, wo, c2.cin, c2.cout, ci.cin, (4 if u["stride"] == 2 else 1) * ci.cin)
        except _C.NBDTHipError:
            plan = None
        if plan is None or plan.tile != 512:
            self._seg_skip.add(key)
            return None
        return self.seg_op(key, lambda: plan,
                           lambda: [self.store.pb(c2.name).view(c2.cout, 9 * c2.cin), self.store.pb(ci.name).view(ci.cout, ci.cin)],
                           lambda: [self.store.p(c2.name).view(c2.cout, 9 * c2.cin), self.store.p(ci.name).view(ci.cout, ci.cin)])

    def _seg_dgrad(self, u, B, hi, wi):
        """dL/d(a1) = conv1's data gradient (four parity classes when strided) + the shortcut's, one launch."""
        c1, ci = u["conv1"], u["idconv"]
        if u["stride"] == 2:
            build = lambda: ops.seg_dgrad_s2(B, hi, wi, c1.cin, c1.cout, shortcut=True)
        else:
            build = lambda: ops.seg_dgrad3x3_plus_1x1(B, hi, wi, c1.cin, c1.cout)
        return self.seg_op((u["key"], "dgrad", B, hi, wi), build,
                           lambda: [c1.wd.view(c1.cin, 9 * c1.cout), ci.wd.view(ci.cin, ci.cout)],
                           lambda: [c1.wd32.view(c1.cin, 9 * c1.cout), ci.wd32.view(ci.cin, ci.cout)], on_side=True)

    def _calibration_unit(self):
        for u in self.units:      # a widest-tensor unit without a shape change: both of its convs are dense 3x3
            if u["idconv"] is None and u["cout"] == self.units[0]["cout"]:
                return u
        return None

    # ------------------------------------------------------------------ forward / backward
    classifier_names = ("output.weight", "output.bias")

    def forward(self, img, training=None, head=True):
        """head=False: stop at the pooled features [B, feat_c] (fp32) -- the caller runs the classifier inside the
        fused head + loss kernel (train_step) and hands dL/dpooled to backward(gpooled=...)."""
        training = self.training if training is None else training
        img = self._input(img)
        B, _, H, W = img.shape
        x = self.buf("x0", B, H, W, self.stem_cpad)
        ops.stem_conv(img, self.store.p("features.init_block.weight"), x, self.stem_c)
        h, w = H, W
        x_has_stats = False   # the stem kernel does not produce BN sums
        for u in self.units:
            k, s = u["key"], u["stride"]
            cin, cout = _pad32(u["cin"]), _pad32(u["cout"])
            ho, wo = h // s, w // s
            t = self.buf(k + ".t", B, ho, wo, cout)
            a2 = self.buf(k + ".a2", B, ho, wo, cout)
            out = self.buf(k + ".out", B, ho, wo, cout)
            fuse = training and self.fuse_stats
            u["bn1"].stats(x, training, fused=fuse and x_has_stats)
            # Shape-changing units in training mode (round 6, csrc/conv_seg.hip): the pre-activation of a stride-2 unit is
            # written as its space-to-depth copy -- its only readers are conv1, the shortcut and their weight gradients,
            # all stride 2 -- conv1 runs as a slice list over it, and conv2 takes the shortcut as one more term of its K
            # loop (no shortcut launch, no residual read in the epilogue).
            seg = training and u["idconv"] is not None
            u["seg"] = seg
            if seg and s == 2:
                a1 = self.s2d_buf(k + ".a1", B, h, w, cin)
                u["bn1"].apply_s2d(x, a1, relu=True)
            else:
                a1 = self.buf(k + ".a1", B, h, w, cin)
                u["bn1"].apply(x, a1, relu=True)
            if not training and self.fuse_eval:   # conv1 + bn2 + ReLU in one launch (t is never materialised)
                u["conv1"].forward_affine(a1, a2, u["bn2"], act=1)
            else:
                if seg and s == 2:
                    self._seg_conv1(u, B, h, w)([a1], t, bn_scratch=self.partials(t) if fuse else None)
                else:
                    u["conv1"].forward(a1, t, bn_scratch=self.partials(t) if fuse else None)
                u["bn2"].stats(t, training, fused=fuse)
                u["bn2"].apply(t, a2, relu=True)
            both = self._seg_conv2_sc(u, B, ho, wo) if seg else None
            if both is not None:
                both([a2, a1], out, bn_scratch=self.partials(out) if fuse else None)
            else:
                if u["idconv"] is not None:
                    idn = self.buf(f"idn{cout}", B, ho, wo, cout)
                    if seg and s == 2:
                        u["idconv"].forward_s2d(a1, idn, h, w)
                    else:
                        u["idconv"].forward(a1, idn)
                    res = idn
                else:
                    res = x
                u["conv2"].forward(a2, out, residual=res, bn_scratch=self.partials(out) if fuse else None)
            x_has_stats = True
            u["x_in"], u["x_out"] = x, out
            x, h, w = out, ho, wo
        self._x_last, self._hw = x, (h, w)
        pb = self.post_bn
        pb.stats(x, training, fused=training and self.fuse_stats)
        return self._pool_head(x, pb.mean, pb.rstd, pb.gamma, pb.beta, head)

    def grad_buckets(self):
        """(lo, hi) ranges of the flat gradient buffer in the order backward completes them:
        [stage3 .. classifier], [stage2], [stem .. stage1]."""
        ent = self.store.entries
        s2 = ent["features.stage2.unit1.body.conv1.bn.weight"][0]
        s3 = ent["features.stage3.unit1.body.conv1.bn.weight"][0]
        return [(s3, self.store.grad.numel()), (s2, s3), (0, s2)]

    bucket_units = ("s3u1", "s2u1")

    def backward(self, gz, comm=None, gpooled=None):
        """Accumulates d(loss)/d(params) into the flat gradient buffer given gz = dloss/dz [B, classes] -- or, after
        forward(head=False), given gpooled = dloss/dpooled [B, feat_c] (the fused head kernel already accumulated the
        classifier's gradients).  With a GradComm, each stage's gradient bucket is all-reduced as soon as it is
        complete."""
        self._begin_backward(comm)
        B, st = self._B, self.store
        gpool = self._head_backward(gz, gpooled)
        h, w = self._hw
        C = _pad32(self.feat_c)
        g = self.buf(f"g_out{C}", B, h, w, C)
        self.post_bn.pool_backward(gpool, self._x_last, g)
        form, share = self._backward_form()
        for i, u in self._units_backward(self.units, comm):
            # The buffers a weight gradient of unit i - 1 can still be reading (see _units_backward) are not the ones unit
            # i writes: conv1's reads `gt`, which alternates between two buffers, conv2's the unit's output gradient (the
            # previous unit's g_in), which rotates through three.  (tests/test_engine_gpu.py::
            # test_deterministic_mode_makes_the_schedules_bit_comparable: this gives the same bits as one stream with
            # private buffers.)
            k, s = u["key"], u["stride"]
            cin, cout = _pad32(u["cin"]), _pad32(u["cout"])
            hi, wi = h * s, w * s
            a1 = self.s2d_buf(k + ".a1", B, hi, wi, cin) if (u["seg"] and s == 2) else self.buf(k + ".a1", B, hi, wi, cin)
            t = self.buf(k + ".t", B, h, w, cout)
            a2 = self.buf(k + ".a2", B, h, w, cout)
            tag = ("@" + k) if self.debug_keep else ""
            ga2 = self.buf(f"ga2_{cout}{tag}", B, h, w, cout)
            gt = self.buf(f"gt_{cout}_{i & 1}{tag}", B, h, w, cout)
            ga1 = self.buf(f"ga1_{cin}_{hi}{tag}", B, hi, wi, cin)
            # the unit's input gradient must not alias its output gradient `g` (nor, see above, the one before that)
            g_in = self.buf(f"g_in{cin}_{hi}_{(i + 1) % 3}{tag}", B, hi, wi, cin)
            u["dbg"] = {"g_out": g, "ga2": ga2, "gt": gt, "ga1": ga1, "g_in": g_in}
            numbers = self._pair_share(form, gt) if share else None
            self._conv2_backward(u, form, numbers, g, a2, t, ga2, gt)
            if u["seg"]:
                self._seg_conv1_backward(u, form, g, a1, gt, ga1, g_in)
            else:
                self._conv1_backward(u, form, numbers, g, a1, gt, ga1, g_in)
            g, h, w = g_in, hi, wi
        ops.stem_wgrad(self._img, g, st.g("features.init_block.weight"), self.stem_c)
        self._end_backward(comm)

    def _backward_form(self):
        """(form, share) of this backward's units.  share: each weight gradient is issued AFTER the data gradient of its
        conv and sized for 256 - n CUs, and the BatchNorm-backward pass that follows on the main stream is confined to n
        CUs, so the HBM-bound pass and the MFMA-bound kernel run at the same time on disjoint CUs (set_cu_share).  form:
          "split"  shared, and the BatchNorm-backward sums move out of the data gradient's epilogue (which reads the
                   BatchNorm input in an HBM burst while the matrix pipes wait) into the confined pass;
          "fused"  the sums come out of the data gradient's epilogue; the elementwise pass is confined when shared;
          "plain"  data gradients with their plain epilogue, the sums in a pass of their own on all CUs: fuse_stats off,
                   and the one-stream mode of the split schedule (profiling passes, bench.py's roofline pass: the same
                   MFMA kernels as the timed step, back to back)."""
        two_streams = self._side is not None and self._overlap
        share = self._cu_share is not None and self.fuse_stats and (two_streams or self.debug_share_serial)
        if share and self._share_split[0]:
            return "split", True
        if self.fuse_stats and not (self._cu_share is not None and self._share_split[0]):
            return "fused", share
        return "plain", False

    def _pair_share(self, form, gt):
        """ops.plan_cu_share's numbers for the pairs of one unit: the split form's time budget is its stage's."""
        if form != "split":
            return self._cu_share
        gbps, _, lo, hi = self._cu_share
        return gbps, self._split_us(gt), lo, hi

    def _conv2_backward(self, u, form, share, g, a2, t, ga2, gt):
        """conv2 and bn2 of one unit: dL/d(out) `g` -> dL/dt `gt`."""
        self._pair_backward(u["conv2"], u["bn2"], form, g, a2, t, ga2, gt, share=share,
                            tensors=self.share_bn2_tensors if form == "split" else 3)
        if share is not None and self._share_join:
            # The next data gradient is one persistent block per CU with a fixed share of the tiles: blocks that found
            # their CU still held by the weight gradient would start late and finish late, and the delay would push the
            # next weight gradient under the next data gradient, and so on (measured: 19.1 -> 26 ms per step with the
            # passes slightly too fast for the weight gradients).  Waiting here makes an unbalanced pair cost
            # max(pass, weight gradient), never more.
            self.join_side_stream()

    def _conv1_backward(self, u, form, share, g, a1, gt, ga1, g_in):
        """conv1, the shortcut conv (if any) and bn1 of a unit on the dense kernels: dL/dt `gt` and dL/d(out) `g` ->
        dL/d(x_in) `g_in`.  The shared and fused forms are for units without a shortcut conv."""
        conv, bn, x_in = u["conv1"], u["bn1"], u["x_in"]
        if u["idconv"] is None:
            self._pair_backward(conv, bn, form, gt, a1, x_in, ga1, g_in, share=share,
                                tensors=self.share_bn1_tensors if form == "split" else 4, gx_add=g)
            return
        conv.backward_weight(a1, gt)
        conv.backward_data(gt, ga1)
        u["idconv"].backward_weight(a1, g)
        u["idconv"].backward_data(g, ga1, accumulate=True)
        bn.backward(ga1, None, x_in, g_in, relu=True)

    def _seg_conv1_backward(self, u, form, g, a1, gt, ga1, g_in):
        """conv1, shortcut and bn1 of a slice-list unit: the two data gradients in one launch (strided: the four parity
        classes, the shortcut's gradient one more term of the even/even class); both weight gradients read the same a1."""
        c1, ci, bn, x_in, s = u["conv1"], u["idconv"], u["bn1"], u["x_in"], u["stride"]
        B, Hp, Wp, C = ga1.shape
        hi, wi = Hp - 2, Wp - 2
        if form == "split" and s == 2:
            # the CU-sharing order of the dense units: data gradient on the whole chip, then conv1's weight gradient
            # sized for 256 - n CUs beside bn1's backward on n (the unit's input gradient is bn1's alone: conv1 and the
            # shortcut both read relu(bn1(x)))
            self._seg_dgrad(u, B, hi, wi)([gt, g], ga1)
            gbps, _, lo, hi_cus = self._cu_share
            budget, n1 = ops.plan_cu_share(c1.s2d_plan(B, hi, wi)[1], B * hi * wi * C, self.share_bn2_tensors, gbps,
                                           self._split_us(gt), lo, hi_cus)
            c1.backward_weight_s2d(a1, gt, hi, wi, cu_budget=budget)
            ci.backward_weight_s2d(a1, g, hi, wi)
            bn.backward_cus(ga1, x_in, g_in, n1)
            return
        if s == 2:
            c1.backward_weight_s2d(a1, gt, hi, wi)
            ci.backward_weight_s2d(a1, g, hi, wi)
        else:
            c1.backward_weight(a1, gt)
            ci.backward_weight(a1, g)
        self._seg_dgrad(u, B, hi, wi)([gt, g], ga1)
        bn.backward(ga1, None, x_in, g_in, relu=True)
    # ------------------------------------------------------------------ reference-named views
    def extra_param_views(self, buf):
        return {
            "features.init_block.weight": self.store._view(buf, "features.init_block.weight").permute(0, 3, 1, 2),
            "output.weight": self.store._view(buf, "output.weight"),
            "output.bias": self.store._view(buf, "output.bias"),
        }


class ResNetEngine(_Engine):
    """CIFAR-style ResNet of the reference (nbdt/models/resnet.py:42-74 BasicBlock, :115-149 ResNet,
    :171-179 ResNet18): 3x3 stem, 4 stages of post-activation BasicBlocks, global average pool,
    ``linear``.  State-dict names are the reference's (conv1, bn1, layerN.M.*, shortcut.0/1, linear).

    A residual block is data: a chain of main stages (conv, bn) -- two for a BasicBlock, three for a Bottleneck
    (BottleneckEngine) -- plus an optional shortcut (sconv, sbn).  ``_block_stages`` is the recipe; forward() and
    backward() walk whatever chain it made, so the cross-stream buffer protocol below exists once.  A new block type
    overrides ``_block_stages``; a new stem overrides ``_make_stem`` and ``_stem_forward`` / ``_stem_backward``
    (_TorchvisionFront: the ImageNet-style nets)."""

    # (GB/s per CU, time budget of bn1's confined pass at 128 images in us, min CUs, max CUs) or None: see backward()
    res_share = (47.0, 15.0, 16, 128)

    def __init__(self, num_classes=10, num_blocks=(2, 2, 2, 2), device="cuda", seed=0):
        super().__init__(device, seed)
        self.num_classes = num_classes
        gen = self.gen
        self.stem_c = 64
        self._make_stem()
        self.blocks = []
        cin = 64
        # Parameters are created in the reference's module order -- per block conv1, bn1, conv2, bn2, [conv3, bn3], then
        # shortcut.0, shortcut.1: the seeded generator is drawn from in creation order and every offset in the flat
        # buffers follows from it, so reordering these calls changes the initial weights and every checkpoint's layout.
        for i, (planes, stride0, n) in enumerate(zip((64, 128, 256, 512), (1, 2, 2, 2), num_blocks)):
            for j in range(n):
                stride = stride0 if j == 0 else 1
                pre, k = f"layer{i + 1}.{j}.", f"l{i + 1}b{j}"
                stages = self._block_stages(pre, cin, planes, stride)
                cout = stages[-1][0].cout_real
                short = stride != 1 or cin != cout
                blk = {
                    "sconv": self.conv(f"{pre}{self.shortcut_name}.0.weight", cin, cout, 1, stride, init=self.conv_init) if short else None,
                    "sbn": self.bn(f"{pre}{self.shortcut_name}.1", cout) if short else None,
                    "cin": cin, "cout": cout, "stride": stride, "key": k,
                }
                # what forward() / backward() iterate, resolved once (the small configurations run at the host's launch
                # rate): per stage m its conv, bn, channels and the keys of its raw output t, its activation a and their
                # gradients gt (alternating: the key lacks its parity) and ga
                head, pairs = [], []
                for m, (conv, bn, fusable) in enumerate(stages, 1):
                    blk[f"conv{m}"], blk[f"bn{m}"] = conv, bn
                    c = conv.cout_real
                    if m > 1:               # backward's pair: conv m with stage m - 1
                        pairs.append((conv, fusable) + prev)
                    if m < len(stages):
                        head.append((conv, bn, c, f"{k}.t{m}", f"{k}.a{m}"))
                        prev = (bn, c, f"{k}.t{m}", f"{k}.a{m}", f"gt{m}_{c}_", f"ga{m}_{c}")
                blk["head"], blk["last"] = tuple(head), (conv, bn, f"{k}.t{m}", f"gt{m}_{c}_")
                blk["pairs"] = tuple(reversed(pairs))
                self.blocks.append(blk)
                cin = cout
        self.feat_c = cin
        kb = 1.0 / math.sqrt(cin)          # nn.Linear's default
        w, b = self.classifier_names
        self.store.add(w, (num_classes, cin), lambda v: v.uniform_(-kb, kb, generator=gen))
        self.store.add(b, (num_classes,), lambda v: v.uniform_(-kb, kb, generator=gen))
        self.finalize()
        self._side = side_stream(self.device)     # weight gradients on a second stream (see WRNEngine)
        for c in self.convs + self.gconvs:
            c.side_stream = self._side
        dev = self.device
        # identity "BN" for the plain average-pool head (features are already post-ReLU)
        self._id_mean = torch.zeros(cin, device=dev)
        self._id_rstd = torch.ones(cin, device=dev)
        self._id_gamma = torch.ones(cin, device=dev)
        self._id_beta = torch.zeros(cin, device=dev)
        self._id_dsum = torch.zeros(2 * cin, device=dev)

    shortcut_name = "shortcut"      # the projection shortcut's module name (torchvision: downsample)
    conv_init = "torch_default"     # Conv's init of every block conv
    block_convs = 2                 # main-chain stages of a block
    zero_init_residual = False      # gamma of each block's last BatchNorm starts at 0 (torchvision's keyword)

    def _make_stem(self):
        """Create the stem's parameters (first in the store): conv1 [64][3][3][3] (co, r, s, ci), bn1."""
        gen = self.gen
        b0 = 1.0 / math.sqrt(27)
        self.store.add("conv1.weight", (64, 3, 3, 3), lambda v: v.uniform_(-b0, b0, generator=gen))
        self.bn0 = self.bn("bn1", 64)

    def _block_stages(self, pre, cin, planes, stride):
        """The main chain of one block as [(conv, bn, fusable)], created in order.  BasicBlock: 3x3 (stride s) -> 3x3.
        fusable: backward() may take the (this conv, previous stage's bn) pair in its fused / CU-sharing forms --
        measured for this block's (conv2, bn1) only."""
        return [self._stage(pre, 1, cin, planes, 3, stride), self._stage(pre, 2, planes, planes, 3, 1, fusable=True)]

    def _stage(self, pre, m, cin, cout, k, stride, fusable=False, groups=1):
        gamma = 0.0 if self.zero_init_residual and m == self.block_convs else 1.0
        if groups > 1:       # (a ResNeXt conv2: cin == cout, 3x3)
            assert cin == cout and k == 3
            conv = self.grouped_conv(f"{pre}conv{m}.weight", cout, groups, stride)
        else:
            conv = self.conv(f"{pre}conv{m}.weight", cin, cout, k, stride, init=self.conv_init)
        return (conv, self.bn(f"{pre}bn{m}", cout, gamma), fusable)

    def extra_param_views(self, buf):
        w, b = self.classifier_names
        return {
            "conv1.weight": self.store._view(buf, "conv1.weight").permute(0, 3, 1, 2),
            w: self.store._view(buf, w),
            b: self.store._view(buf, b),
        }

    def grad_buckets(self):
        ent = self.store.entries
        l3 = ent["layer3.0.conv1.weight"][0]
        l2 = ent["layer2.0.conv1.weight"][0]
        return [(l3, self.store.grad.numel()), (l2, l3), (0, l2)]

    bucket_units = ("l3b0", "l2b0")

    classifier_names = ("linear.weight", "linear.bias")

    def _stem_forward(self, img, training):
        """conv1 -> bn1 -> ReLU; returns the first block's input."""
        B, _, H, W = img.shape
        t0 = self.buf("t0", B, H, W, 64)
        x = self.buf("a0", B, H, W, 64)
        ops.stem_conv(img, self.store.p("conv1.weight"), t0, 64)
        self.bn0.stats(t0, training)
        self.bn0.apply(t0, x, relu=True)
        return x

    def _stem_backward(self, g):
        """From g = dL/d(first block's input): bn1's backward and conv1's weight gradient."""
        B, Hp, Wp, _ = g.shape
        gt0 = self.buf("gt0", B, Hp - 2, Wp - 2, 64)
        self.bn0.backward(g, None, self.buf("t0", B, Hp - 2, Wp - 2, 64), gt0, relu=True)
        ops.stem_wgrad(self._img, gt0, self.store.g("conv1.weight"), 64)

    def forward(self, img, training=None, head=True):
        training = self.training if training is None else training
        img = self._input(img)
        B = self._B
        x = self._stem_forward(img, training)
        h, w = x.shape[1] - 2, x.shape[2] - 2
        fuse = training and self.fuse_stats
        affine = not training and self.fuse_eval
        for blk in self.blocks:
            k, cout, sconv = blk["key"], blk["cout"], blk["sconv"]
            y = x
            if affine:
                # inference: every Conv-BN(-ReLU)(+shortcut) group of the block is ONE launch
                for conv, bn, c, _, ak in blk["head"]:
                    h, w = h // conv.stride, w // conv.stride
                    a = self.buf(ak, B, h, w, c)
                    conv.forward_affine(y, a, bn, act=1)
                    y = a
                conv, bn, _, _ = blk["last"]
                h, w = h // conv.stride, w // conv.stride
                res = x
                if sconv is not None:
                    res = self.buf(f"sc{cout}", B, h, w, cout)
                    sconv.forward_affine(x, res, blk["sbn"], act=0)
                out = self.buf(k + ".out", B, h, w, cout)
                conv.forward_affine(y, out, bn, act=1, residual=res)
                blk["x_in"] = x
                x = out
                continue
            for conv, bn, c, tk, ak in blk["head"]:
                h, w = h // conv.stride, w // conv.stride
                t = self.buf(tk, B, h, w, c)              # raw conv outputs: only the training path keeps them
                f = fuse and conv.fused_stats             # (a grouped conv has no statistics epilogue: separate pass)
                conv.forward(y, t, bn_scratch=self.partials(t) if f else None)
                bn.stats(t, training, fused=f)
                y = self.buf(ak, B, h, w, c)
                bn.apply(t, y, relu=True)
            conv, bn, tk, _ = blk["last"]
            h, w = h // conv.stride, w // conv.stride
            t = self.buf(tk, B, h, w, cout)
            conv.forward(y, t, bn_scratch=self.partials(t) if fuse else None)
            bn.stats(t, training, fused=fuse)
            res = x
            if sconv is not None:
                ts = self.buf(k + ".ts", B, h, w, cout)
                res = self.buf(f"sc{cout}", B, h, w, cout)
                sconv.forward(x, ts, bn_scratch=self.partials(ts) if fuse else None)
                blk["sbn"].stats(ts, training, fused=fuse)
                blk["sbn"].apply(ts, res, relu=False)
            out = self.buf(k + ".out", B, h, w, cout)
            bn.apply(t, out, relu=True, residual=res)
            blk["x_in"] = x
            x = out
        self._x_last, self._hw = x, (h, w)
        return self._pool_head(x, self._id_mean, self._id_rstd, self._id_gamma, self._id_beta, head)

    def backward(self, gz, comm=None, gpooled=None):
        self._begin_backward(comm)
        B = self._B
        gpool = self._head_backward(gz, gpooled)
        h, w = self._hw
        g = self.buf(f"g_out{self.feat_c}", B, h, w, self.feat_c)
        # plain avg-pool backward: identity BN with zero batch sums (the x>0 mask it applies is the
        # same mask the following ReLU backward applies anyway)
        ops.pool_bn_bwd_apply(gpool, self._x_last, self._id_mean, self._id_rstd, self._id_gamma, self._id_beta,
                              self._id_dsum, g)
        two_streams = self._side is not None and self._overlap
        # how a fusable (conv, previous bn) pair runs -- the same for every block of a step:
        # fused: the conv's data gradient is dL/d(relu(bn(t))): its epilogue also emits that bn's backward sums (as in
        #   WRNEngine's fused order), so the gradient is not re-read for them -- one HBM-bound pass fewer per block
        # share: CU sharing as in WRNEngine (fused-sums form): the conv's weight gradient is issued AFTER its data gradient,
        #   sized for 256 - n CUs, and the bn's elementwise pass that follows on this stream is confined to n CUs -- in the
        #   plain order the pass's blocks waited for the weight gradient's to leave their CUs (bn_bwd_fold_partials: 42 us
        #   in the trace for 5 us of work, profiles/r06_c4_step_dump_before.txt)
        fused = self.fuse_bn1_bwd and self.act_dtype == torch.bfloat16
        share = (fused and self.res_share is not None and (two_streams or self.debug_share_serial)
                 and ops.cu_topology_is_mi355x(self.device))
        form = "fused" if fused else "plain"
        numbers = None
        if share:
            gbps, us, lo, hi_cus = self.res_share
            numbers = (gbps, us * B / 128.0, lo, hi_cus)
        for i, blk in self._units_backward(self.blocks, comm):
            # the buffers a weight gradient reads (every gt / gts) alternate between consecutive blocks, and so does
            # the block's input gradient: the block in flight never overwrites what the previous one's may be reading
            k, s, cin, cout, sconv = blk["key"], blk["stride"], blk["cin"], blk["cout"], blk["sconv"]
            hi, wi = h * s, w * s
            tag = ("@" + k) if self.debug_keep else ""
            par = i & 1
            g_in = self.buf(f"g_in{cin}_{hi}_{par ^ 1}{tag}", B, hi, wi, cin)
            x_in = blk["x_in"]
            _, bn, tk, gtk = blk["last"]
            gt = self.buf(f"{gtk}{par}{tag}", B, h, w, cout)
            if sconv is not None:
                gsc = g_resid = self.buf(f"gsc_{cout}{tag}", B, h, w, cout)
                gts = self.buf(f"gts_{cout}_{par}{tag}", B, h, w, cout)
            else:
                g_resid = g_in      # identity shortcut: the masked gradient IS part of the block-input gradient
            bn.backward(g, self.buf(k + ".out", B, h, w, cout), self.buf(tk, B, h, w, cout), gt, relu=True, g_resid=g_resid)
            hh, ww = h, w
            for conv, fusable, bn, c, tk, ak, gtk, gak in blk["pairs"]:     # conv m with stage m - 1, m = n ... 2
                hh, ww = hh * conv.stride, ww * conv.stride
                t, a = self.buf(tk, B, hh, ww, c), self.buf(ak, B, hh, ww, c)
                ga = self.buf(gak + tag, B, hh, ww, c)
                gt_prev = self.buf(f"{gtk}{par}{tag}", B, hh, ww, c)
                self._pair_backward(conv, bn, form if fusable else "plain", gt, a, t, ga, gt_prev, share=numbers,
                                    tensors=3)
                gt = gt_prev
            conv1 = blk["conv1"]
            conv1.backward_weight(x_in, gt)
            if sconv is not None:
                conv1.backward_data(gt, g_in)
                blk["sbn"].backward(gsc, None, self.buf(k + ".ts", B, h, w, cout), gts, relu=False)
                sconv.backward_weight(x_in, gts)
                sconv.backward_data(gts, g_in, accumulate=True)      # after conv1's plain one
            else:
                conv1.backward_data(gt, g_in, accumulate=True)
            blk["dbg"] = {"g_out": g, "g_in": g_in}
            g, h, w = g_in, hi, wi
        self._stem_backward(g)
        self._end_backward(comm)


class BottleneckEngine(ResNetEngine):
    """CIFAR-style Bottleneck ResNet of the reference (nbdt/models/resnet.py:77-112 Bottleneck, expansion 4; :193-223
    ResNet50 / 101 / 152): ResNetEngine -- its stem, stage widths, head, gradient buckets, forward() and backward() -- with
    blocks of 1x1 -> 3x3 (stride s) -> 1x1 (x 4).  State-dict names are the reference's (layerN.M.conv1/bn1/conv2/bn2/
    conv3/bn3, shortcut.0/1, linear); parameters are created in the reference's module order.

    While ``pointwise`` is true the stride-1 1x1 convolutions -- conv1, conv3 and layer1.0's shortcut -- run on the
    pointwise GEMM kernel (csrc/conv_pw.hip): every data gradient, the eval-mode unfused forward, and the training
    forward (a statistics launch) from Conv.PW_STATS_MIN_CIN = 1024 input channels on.  Training forwards with fewer
    input channels -- 25 of ResNet50's 33 -- stay on nbdt_conv_igemm, where they are faster (Conv.PW_STATS_MIN_CIN says
    why).  Both kernels leave the same bits, statistics included, so the routing is not a numerical event.
    ``engine.pointwise = False`` sends every launch through nbdt_conv_igemm (the A/B, and a test handle).  3x3 convs,
    strided shortcuts and every weight gradient take the kernels they take in ResNetEngine."""

    expansion = 4
    block_convs = 3

    # No CU sharing: ResNetEngine confines bn1's backward pass beside conv2's weight gradient with a plan measured for
    # BasicBlocks; nothing has been measured for these blocks, so every launch gets the whole chip.
    res_share = None

    def __init__(self, num_classes=10, num_blocks=(3, 4, 6, 3), device="cuda", seed=0, groups=1, width_per_group=64):
        self.groups, self.width_per_group = int(groups), int(width_per_group)
        if self.groups < 1 or self.width_per_group < 1:
            raise ValueError(f"groups and width_per_group are positive, got {groups} and {width_per_group}")
        super().__init__(num_classes, num_blocks, device, seed)
        self.pointwise = True

    def _block_stages(self, pre, cin, planes, stride):
        """1x1 (cin -> width) -> 3x3 (stride s) -> 1x1 (-> 4 planes), width = planes * width_per_group / 64 * groups as in
        torchvision's Bottleneck: planes with the defaults, 2 planes for the wide ResNets (dense convs, the entries every
        other 3x3 takes), and for a ResNeXt (groups > 1) conv2 is a GroupedConv.  Every pair's backward in the plain form
        (nothing else has been measured for these blocks)."""
        width = int(planes * self.width_per_group / 64) * self.groups
        return [self._stage(pre, 1, cin, width, 1, 1), self._stage(pre, 2, width, width, 3, stride, groups=self.groups),
                self._stage(pre, 3, width, self.expansion * planes, 1, 1)]

    @property
    def pointwise(self):
        return self._pointwise

    @pointwise.setter
    def pointwise(self, on):
        self._pointwise = bool(on)
        for c in self.convs:
            c.pointwise = self._pointwise


class _TorchvisionFront:
    """What torchvision.models.resnet puts around the four stages, for ResNetEngine and BottleneckEngine alike (mixed in
    ahead of them): the 7x7 / 2 stem, BatchNorm, ReLU and MaxPool2d(3, 2, 1) in front, ``fc`` behind, torchvision's module
    names (conv1, bn1, layerN.M.conv{1,2,3} / bnK, downsample.0/1, fc) and its initialisation.

    No new convolution kernel: ops.stem_patches gathers the 7x7 patches (147 -> 160 channels) and ``conv1`` is a 1x1
    convolution over them -- forward with fused statistics, the eval-mode conv + affine launch and the weight gradient are
    the launches every other conv takes; the patch tensor is kept for the weight gradient.  BatchNorm and ReLU are bn1's
    usual passes, the pool is its own op (ops.maxpool_fwd / maxpool_bwd, window positions kept as uint8 in training).

    The stages see H/4 x W/4, H/8, H/16 and H/32 pixels, so H and W must be multiples of 32.  Stage widths that are powers
    of two (128 x 128 or 256 x 256 images) take the kernels the CIFAR trunks take; 224 x 224 (56 / 28 / 14 / 7) takes the
    generic implicit-GEMM and weight-gradient kernels for its dense 3x3 convs ("ImageNet-style ResNets")."""

    shortcut_name = "downsample"
    conv_init = "kaiming_normal_fan_out"
    classifier_names = ("fc.weight", "fc.bias")
    res_share = None        # the CU-sharing plan was measured on CIFAR grids: nothing is assumed to carry over
    PATCH_K = 7

    def __init__(self, num_classes=1000, num_blocks=None, zero_init_residual=False, device="cuda", seed=0, **block_kw):
        """block_kw: what the block engine behind this front takes besides (BottleneckEngine: groups, width_per_group)."""
        self.zero_init_residual = bool(zero_init_residual)
        if num_blocks is not None:
            block_kw["num_blocks"] = num_blocks
        super().__init__(num_classes=num_classes, device=device, seed=seed, **block_kw)

    def _make_stem(self):
        self.conv0 = PatchConv(self.store, "conv1.weight", 64, self.PATCH_K, self.gen, self.conv_init)
        self.convs.append(self.conv0)
        self.bn0 = self.bn("bn1", 64)

    def extra_param_views(self, buf):
        w, b = self.classifier_names          # (conv1.weight is a Conv: PatchConv.logical)
        return {w: self.store._view(buf, w), b: self.store._view(buf, b)}

    def _stem_forward(self, img, training):
        """patches -> conv1 (+ statistics) -> bn1 + ReLU -> max-pool; returns layer1's input."""
        B, _, H, W = img.shape
        if H % 32 or W % 32:
            raise ValueError(f"ImageNet-style ResNets take images whose sides are multiples of 32, got {H} x {W}")
        h, w = H // 2, W // 2
        patches = self.buf("patches", B, h, w, self.conv0.cin)
        a = self.buf("a0", B, h, w, 64)
        x = self.buf("p0", B, h // 2, w // 2, 64)
        ops.stem_patches(img, patches, self.PATCH_K, 2)
        if not training and self.fuse_eval:
            self.conv0.forward_affine(patches, a, self.bn0, act=1)
            ops.maxpool_fwd(a, x, None)
            return x
        t0 = self.buf("t0", B, h, w, 64)
        fuse = training and self.fuse_stats
        self.conv0.forward(patches, t0, bn_scratch=self.partials(t0) if fuse else None)
        self.bn0.stats(t0, training, fused=fuse)
        self.bn0.apply(t0, a, relu=True)
        ops.maxpool_fwd(a, x, self._pool_idx(B, h // 2, w // 2) if training else None)
        return x

    def _pool_idx(self, B, h, w):
        k = ("pool_idx", B, h, w)
        if k not in self._bufs:
            self._bufs[k] = torch.empty((B, h, w, 64), dtype=torch.uint8, device=self.device)
        return self._bufs[k]

    def _stem_backward(self, g):
        """From g = dL/d(layer1's input): the pool's backward, bn1's backward and conv1's weight gradient."""
        B, Hp, Wp, _ = g.shape
        h, w = 2 * (Hp - 2), 2 * (Wp - 2)
        ga = self.buf("ga0", B, h, w, 64)
        gt0 = self.buf("gt0", B, h, w, 64)
        ops.maxpool_bwd(g, self._pool_idx(B, Hp - 2, Wp - 2), ga)
        self.bn0.backward(ga, None, self.buf("t0", B, h, w, 64), gt0, relu=True)
        self.conv0.backward_weight(self.buf("patches", B, h, w, self.conv0.cin), gt0)


class ImageNetResNetEngine(_TorchvisionFront, ResNetEngine):
    """torchvision's resnet18 / resnet34 (BasicBlocks; the reference's ImageNet recipe takes them from torchvision.models
    through nbdt/models/__init__.py): ResNetEngine's stages between _TorchvisionFront's stem and head."""


class ImageNetBottleneckEngine(_TorchvisionFront, BottleneckEngine):
    """torchvision's resnet50 / 101 / 152 (Bottleneck v1.5: the stride is on the 3x3 conv, as in BottleneckEngine), and with
    torchvision's ``groups`` / ``width_per_group`` keywords its resnext50_32x4d / resnext101_64x4d (groups = 32 / 64,
    width_per_group = 4: conv2 is a GroupedConv) and wide_resnet50_2 / wide_resnet101_2 (width_per_group = 128: dense convs
    at twice the width).  With the defaults nothing differs from before the keywords existed."""


def _loss_backward(engine, criterion, img, targets, comm, fused_head, calibrate_with=None):
    """forward, loss and backward of one (micro-)batch on the head path its targets and the criterion select; the
    gradients are ADDED to store.grad, all-reduced if comm is given.  Returns the loss (device scalar).
    calibrate_with: the communicator of a step whose backward HERE does not reduce (a leading micro-batch).  A pending
    CU-sharing calibration broadcasts rank 0's decision, so it runs with that communicator, after the forward it needs
    and before backward() would run it without one."""
    names = getattr(engine, "classifier_names", None)
    gpool = None
    if targets.is_floating_point():
        z = engine.forward(img, training=True)
        loss, gz = criterion.soft_target_loss_and_grad(z, targets)
    elif (fused_head and names is not None and hasattr(criterion, "can_fuse_head")
            and criterion.can_fuse_head(engine.num_classes)):
        # classifier + rules + loss + their backward in ONE launch (nbdt_head_soft_tree_loss): logits stay on chip
        pooled = engine.forward(img, training=True, head=False)
        st = engine.store
        loss, gpool, _ = criterion.head_loss_and_grad(pooled, st.p(names[0]), st.p(names[1]), targets,
                                                      grad_weight=st.g(names[0]), grad_bias=st.g(names[1]))
    else:
        z = engine.forward(img, training=True)
        loss, gz = criterion.loss_and_grad(z, targets)
    if calibrate_with is not None and comm is None:
        engine.calibrate_pending(calibrate_with)
    if gpool is not None:
        engine.backward(None, comm=comm, gpooled=gpool)
    else:
        engine.backward(gz, comm=comm)
    return loss


def train_step(engine, criterion, img, targets, lr, momentum=0.9, weight_decay=5e-4, comm=None, fused_head=True,
               zero_grad=True, lars=None, optim=None, clip=None, micro_batches=1):
    """One full training step (main.py:233-239): zero_grad, forward, SoftTreeSupLoss fwd+bwd (one fused
    kernel -- with the classifier's forward and backward inside it when the criterion and the head's width allow,
    fused_head=False keeps linear -> loss -> linear-backward as three launches), backward, [gradient all-reduce],
    SGD.  Returns the loss tensor (device scalar).  zero_grad=False leaves the step's gradient in the flat gradient
    buffer instead of having the SGD kernel clear it for the next step (tests that compare gradients).
    Floating-point targets are probability rows [B, C] (MixUp / CutMix, nbdt.data.mix_batch): they skip the fused head
    and go through criterion.soft_target_loss_and_grad, still one loss launch.
    lars: a LarsConfig (trust, eps, exclude_1d) makes the optimizer pass engine.lars_step; the 1 / world_size of a
    data-parallel step enters its norms, so every rank computes the same trust ratios from the same reduced gradient.
    optim: an AdamWConfig or RMSpropConfig makes it engine.adamw_step / engine.rmsprop_step with this call's lr,
    weight_decay and (RMSprop) momentum; not together with lars.
    micro_batches=K > 1: gradient accumulation.  img / targets are cut into K equal chunks along dim 0 (B % K != 0
    raises); the gradient buffer is zeroed once, every chunk runs forward + loss + backward into it -- each with its own
    BatchNorm statistics and its own update of the running ones, as K PyTorch forward passes would -- only the last
    chunk's backward all-reduces, and the optimizer takes grad_scale = 1 / (K * world_size): the step of the mean loss
    over all K chunks.  Returns the mean of the chunk losses.
    clip: a ClipConfig(max_norm) runs engine.clip_grad_norm(max_norm, grad_scale) on the complete (accumulated, reduced)
    gradient before the optimizer pass, whichever it is.  With the defaults of both the launches are what they were."""
    if lars is not None and optim is not None:
        raise ValueError("train_step: lars= and optim= both name the optimizer pass; pass one of them")
    if optim is not None and not isinstance(optim, (AdamWConfig, RMSpropConfig)):
        raise TypeError(f"train_step: optim must be an AdamWConfig or an RMSpropConfig, got {type(optim).__name__}")
    if clip is not None and not isinstance(clip, ClipConfig):
        raise TypeError(f"train_step: clip must be a ClipConfig, got {type(clip).__name__}")
    K = int(micro_batches)
    if K != micro_batches or K < 1:
        raise ValueError(f"train_step: micro_batches must be an integer >= 1, got {micro_batches!r}")
    if img.shape[0] % K or targets.shape[0] != img.shape[0]:
        raise ValueError(f"train_step: a batch of {img.shape[0]} images ({targets.shape[0]} targets) does not split into "
                         f"{K} equal micro-batches")
    engine.zero_grad()
    if K == 1:
        loss = _loss_backward(engine, criterion, img, targets, comm, fused_head)
    else:
        # (chunks along dim 0 of contiguous tensors are contiguous views: nothing is copied)
        total = None
        for k, (x, y) in enumerate(zip(img.chunk(K), targets.chunk(K))):
            last = k == K - 1
            loss_k = _loss_backward(engine, criterion, x, y, comm if last else None, fused_head, calibrate_with=comm)
            total = loss_k.clone() if total is None else total.add_(loss_k)
        loss = total.div_(K)
    scale = 1.0 / (K * (comm.world_size if comm is not None else 1))
    if clip is not None:
        engine.clip_grad_norm(clip.max_norm, grad_scale=scale)
    engine.optimizer_step(lr, momentum, weight_decay, lars if lars is not None else optim, grad_scale=scale,
                          zero_grad=zero_grad)
    return loss


class GraphedStep:
    """One training step captured in a hipGraph (torch.cuda.CUDAGraph drives hipStreamBeginCapture on the
    stream every C-ABI launch already uses) and replayed with one host call.

    The step is a fixed sequence of ~130 (ResNet18) to ~700 (EfficientNet-B0) launches with no host
    synchronisation, so it captures as is.  Measured on MI355X (scratch/bench_graph.py, profiles/r04_graph.txt):
    replay is 4-8 % SLOWER than eager launching for every configuration tried (ResNet18 B=128: 3.35 vs 3.13 ms;
    WRN-28-10 B=512: 18.42 vs 17.40 ms; in round 2, before the two-stream schedule, the two were equal at 21.8 ms) --
    the ctypes launch path costs ~5 us per kernel and the CPU stays ahead of the GPU (2.2 ms of enqueue for a 17 ms
    step), while the graph serialises the cross-stream edges the eager schedule overlaps.  So this is latency insurance
    for slower hosts, not a speed-up, and bench.py does not use it.  The learning rate and the dropout
    seed are kernel arguments baked into the graph: build one GraphedStep per learning rate, and do not use it
    for models with dropout or stochastic depth (its counter is such an argument too).  A per-step learning rate is such a baked argument too, so a GraphedStep cannot be used with
    learning-rate warm-up or a per-iteration decay (main.py --warmup-epochs, --lr-schedule cosine | poly).  So are the loss weights and the device pointers of the hierarchy: a replay after
    ``criterion.set_epoch`` changed the weights (--tswe / --xwe schedules) or after the hierarchy was re-induced
    (SoftTreeLoss) raises instead of silently using the captured ones; the captured tree handle is kept alive
    by this object.  Gradient all-reduce (RCCL) is not captured: single-GPU steps only."""

    def __init__(self, engine, criterion, img, targets, lr, momentum=0.9, weight_decay=5e-4, warmup=2):
        if getattr(engine, "dropout_rate", 0.0) > 0.0:
            raise ValueError("the dropout seed is a kernel argument: a captured step would repeat one mask")
        if getattr(engine, "stochastic_depth_prob", 0.0) > 0.0:
            raise ValueError("the stochastic depth counter is a kernel argument: a captured step would repeat one draw")
        if targets.is_floating_point():
            raise ValueError("GraphedStep captures class-index targets only; probability targets go through train_step")
        self.engine, self.criterion = engine, criterion
        self.img = img.clone()
        self.targets = targets.clone()
        # Warm up and capture on ONE explicit stream: the library's per-(device, stream) workspaces -- K-split
        # weight-gradient copies, stem weight-gradient rows, split-K partials and tickets -- cannot be allocated inside a
        # capture, so a launch that meets its stream for the first time there silently takes its fallback form (atomics, no
        # split).  torch.cuda.graph() without stream= captures on a private stream the warm-up never ran on.
        self._stream = torch.cuda.Stream(device=self.img.device)
        self._stream.wait_stream(torch.cuda.current_stream(self.img.device))
        with torch.cuda.stream(self._stream):
            for _ in range(warmup):     # allocate every buffer and workspace, set kernel attributes, warm the allocator
                train_step(engine, criterion, self.img, self.targets, lr, momentum, weight_decay)
        torch.cuda.synchronize()
        self._captured = self._criterion_state()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self._stream):
            self.loss = train_step(engine, criterion, self.img, self.targets, lr, momentum, weight_decay)
            engine.join_side_stream()     # a capture must end with every forked stream joined

    def _criterion_state(self):
        """(loss weights, tree handle) the captured launches were built with; holding the handle keeps its device
        memory alive even if the Tree drops it."""
        c = self.criterion
        weights = tuple(float(w) for w in c.current_weights()) if hasattr(c, "current_weights") else None
        tree = getattr(c, "tree", None)
        handle = tree.device_handle(self.img.device.index) if tree is not None else None
        return weights, handle

    def __call__(self, img, targets):
        weights, handle = self._criterion_state()
        if weights != self._captured[0] or handle is not self._captured[1]:
            raise RuntimeError("GraphedStep: the criterion's weights or hierarchy changed since capture; "
                               "build a new GraphedStep (they are baked into the captured launches)")
        self.img.copy_(img, non_blocking=True)
        self.targets.copy_(targets, non_blocking=True)
        # the captured step holds no gradient fill when it was captured after a step whose SGD pass left the buffer
        # zeroed (zero_grad() was free then): anything eager that accumulated since must be cleared here, not summed in
        if not self.engine._grad_is_zero:
            self.engine.store.zero_grad()
        self.graph.replay()
        self.engine._grad_is_zero = True     # the replayed SGD pass zeroed it again
        return self.loss


def smoke():
    """Tiny forward+backward+step of the flagship backbone on cuda:0 (called by __graft_entry__)."""
    import torch.nn as nn
    from nbdt.loss import SoftTreeSupLoss
    eng = WRNEngine(num_classes=10, blocks=10, width_factor=2, device="cuda:0", seed=0)
    crit = SoftTreeSupLoss(dataset="CIFAR10", criterion=nn.CrossEntropyLoss(), hierarchy="induced-wrn28_10_cifar10")
    g = torch.Generator().manual_seed(0)
    img = torch.randn(8, 3, 32, 32, generator=g).cuda()
    y = torch.randint(0, 10, (8,), generator=g).cuda()
    l0 = train_step(eng, crit, img, y, lr=0.05).item()
    for _ in range(5):
        l1 = train_step(eng, crit, img, y, lr=0.05).item()
    assert math.isfinite(l0) and math.isfinite(l1) and l1 < l0, (l0, l1)
    print(f"smoke ok: WRN-10-2 SoftTreeSupLoss train steps on cuda:0, loss {l0:.4f} -> {l1:.4f}")
