"""fp32 PyTorch restatement of pytorchcv's EfficientNet family (efficientnet_b0 .. b7 and the TF-padded b0b .. b7b),
parametrised by nbdt.engine_effnet.efficientnet_config: plain nn.Conv2d / F.pad / nn.BatchNorm2d, pytorchcv's module
names (so the state_dict keys are the checkpoint's), nothing from the package under test but the configuration table.
oracle/torch_models.py holds only a hard-coded B0; this is the scaled family's comparator."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def same_pad(x, k, stride):
    """TensorFlow "SAME" padding of an NCHW tensor for a k-tap, stride-s convolution that then runs with padding 0."""
    h, w = x.shape[2:]
    ph = max((-(-h // stride) - 1) * stride + k - h, 0)
    pw = max((-(-w // stride) - 1) * stride + k - w, 0)
    return F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))


_EMULATE = [False]


class emulate_bf16:
    """Inside this context the restatement rounds to bf16 wherever the engine stores bf16: raw convolution outputs, stored
    activations (after BatchNorm + swish, the SE scaling, the residual add), the weights of the 1x1 convolutions, and the
    gradients of the same tensors on the way back.  Everything else stays fp32: what is left between this and the plain
    fp32 run is what bf16 STORAGE costs at a given shape, whatever kernels compute it."""

    def __enter__(self):
        _EMULATE[0] = True

    def __exit__(self, *exc):
        _EMULATE[0] = False


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).float()

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).float()


def _q(x):
    return _Round.apply(x) if _EMULATE[0] else x


class ConvBlock(nn.Module):
    """pytorchcv ConvBlock: conv (bias-free) -> bn -> optional swish; tf_mode pads SAME in front of an unpadded conv."""

    def __init__(self, cin, cout, k, stride, groups, eps, act, tf_mode):
        super().__init__()
        self.k, self.stride, self.tf_mode = k, stride, tf_mode
        self.conv = nn.Conv2d(cin, cout, k, stride, 0 if tf_mode else k // 2, groups=groups, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=eps)
        self.act = act

    def forward(self, x):
        if self.tf_mode:
            x = same_pad(x, self.k, self.stride)
        if _EMULATE[0] and self.k == 1:
            x = F.conv2d(x, self.conv.weight.to(torch.bfloat16).float() + (self.conv.weight - self.conv.weight.detach()))
        else:
            x = self.conv(x)
        x = self.bn(_q(x))
        return x * torch.sigmoid(x) if self.act else x


class SEBlock(nn.Module):
    def __init__(self, c, mid):
        super().__init__()
        self.conv1 = nn.Conv2d(c, mid, 1, bias=True)
        self.conv2 = nn.Conv2d(mid, c, 1, bias=True)

    def forward(self, x):
        w = x.mean((2, 3), keepdim=True)
        w = self.conv1(w)
        w = self.conv2(w * torch.sigmoid(w))
        return _q(x * torch.sigmoid(w))


class DwsUnit(nn.Module):          # pytorchcv EffiDwsConvUnit
    def __init__(self, cin, cout, k, stride, eps, tf_mode):
        super().__init__()
        self.residual = cin == cout and stride == 1
        self.dw_conv = ConvBlock(cin, cin, k, stride, cin, eps, True, tf_mode)
        self.se = SEBlock(cin, cin // 4)
        self.pw_conv = ConvBlock(cin, cout, 1, 1, 1, eps, False, tf_mode)

    def forward(self, x):
        y = self.pw_conv(self.se(self.dw_conv(x)))
        return _q(y + x if self.residual else y)


class InvResUnit(nn.Module):       # pytorchcv EffiInvResUnit
    def __init__(self, cin, cout, k, stride, exp, eps, tf_mode):
        super().__init__()
        self.residual = cin == cout and stride == 1
        mid = cin * exp
        self.conv1 = ConvBlock(cin, mid, 1, 1, 1, eps, True, tf_mode)
        self.conv2 = ConvBlock(mid, mid, k, stride, mid, eps, True, tf_mode)
        self.se = SEBlock(mid, mid // (4 * exp))
        self.conv3 = ConvBlock(mid, cout, 1, 1, 1, eps, False, tf_mode)

    def forward(self, x):
        y = self.conv3(self.se(self.conv2(_q(self.conv1(x)))))
        return _q(y + x if self.residual else y)


class _Named(nn.Module):
    def forward(self, x):
        for m in self.children():
            x = m(x)
        return x


class EfficientNetRef(nn.Module):
    def __init__(self, config, num_classes=1000, dropout_rate=None):
        super().__init__()
        eps, tf = config["bn_eps"], config["tf_mode"]
        self.features = _Named()
        init = _Named()
        init.add_module("conv", ConvBlock(3, config["init_channels"], 3, 2, 1, eps, True, tf))
        self.features.add_module("init_block", init)
        cin = config["init_channels"]
        for i, (stage_stride, specs) in enumerate(config["stages"]):
            stage = _Named()
            for j, (cout, k, exp) in enumerate(specs):
                stride = stage_stride if j == 0 else 1
                unit = DwsUnit(cin, cout, k, stride, eps, tf) if i == 0 else InvResUnit(cin, cout, k, stride, exp, eps, tf)
                stage.add_module(f"unit{j + 1}", unit)
                cin = cout
            self.features.add_module(f"stage{i + 1}", stage)
        self.features.add_module("final_block", ConvBlock(cin, config["final_channels"], 1, 1, 1, eps, True, tf))
        self.output = nn.Module()
        self.dropout_rate = config["dropout_rate"] if dropout_rate is None else dropout_rate
        self.output.add_module("fc", nn.Linear(config["final_channels"], num_classes))

    def forward(self, x):
        x = self.features(x).mean((2, 3))
        if self.dropout_rate > 0:
            x = F.dropout(x, self.dropout_rate, self.training)
        return self.output.fc(x)
