"""Host-side launch helpers for the backbone kernels of libnbdt_hip.so.

Everything here is plumbing: tensor allocation (PyTorch caching allocator), tap-table construction
for the implicit-GEMM kernel and raw-pointer hand-off through ctypes.  No arithmetic on the data
path happens in Python/PyTorch.

Activation layout: padded NHWC bf16 ``[B][H+2][W+2][C]`` with a zero one-pixel border (kernels only
ever write interiors, so the border stays zero for the lifetime of the buffer).
Weight layout: ``[cout][taps][cin]`` (fp32 master and bf16 copy); the data-gradient kernel reads
the transposed, tap-reversed copy ``[cin][taps][cout]`` produced by ``weight_prep``.
"""
import contextlib
import ctypes

import numpy as np
import torch

from nbdt import _C
from nbdt._C import ConvDesc, WgradDesc, check, lib, ptr

BN_SLOTS = 32
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def set_deterministic(on):
    """Process-wide: every cross-block reduction of the ResNet / WideResNet path in a fixed order instead of fp32
    atomics (nbdt_set_deterministic in include/nbdt_hip.h) -- same launches + same inputs => same bits, like the
    reference's CPU path.  Slower; for parity runs and debugging."""
    check(lib().nbdt_set_deterministic(1 if on else 0))


def is_deterministic():
    return bool(lib().nbdt_get_deterministic())


RULES_PATHS = ("auto", "global")


def set_rules_path(name):
    """Process-wide: "auto" (default) = the tree rules and losses keep a sample's row in LDS wherever it fits and take
    the global-row kernels only for hierarchies too large for that; "global" = the global-row kernels for every
    hierarchy, for tests and measurements (nbdt_set_rules_path in include/nbdt_hip.h)."""
    if name not in RULES_PATHS:
        raise ValueError(f"unknown rules path {name!r}: expected one of {RULES_PATHS}")
    check(lib().nbdt_set_rules_path(RULES_PATHS.index(name)))


def rules_path():
    return RULES_PATHS[lib().nbdt_get_rules_path()]


def set_wgrad_store_epilogue(on):
    """K-split weight gradient: 1 (default) = plain stores into per-split copies + a fold pass, 0 = fp32 atomics into dw
    (nbdt_set_wgrad_store_epilogue in include/nbdt_hip.h)."""
    check(lib().nbdt_set_wgrad_store_epilogue(1 if on else 0))


def wgrad_store_epilogue():
    return bool(lib().nbdt_get_wgrad_store_epilogue())


def set_reserved_cus(n):
    """CUs the one-block-per-CU MFMA kernels leave free for a collective's kernels (nbdt_set_reserved_cus)."""
    check(lib().nbdt_set_reserved_cus(int(n)))


def reserved_cus():
    return int(lib().nbdt_get_reserved_cus())


def set_stream_nt_min_bytes(n):
    """Tensors of at least n bytes take the nontemporal-load BatchNorm passes (nbdt_set_stream_nt_min_bytes)."""
    check(lib().nbdt_set_stream_nt_min_bytes(int(n)))


def stream_nt_min_bytes():
    return int(lib().nbdt_get_stream_nt_min_bytes())


def last_stream_nt():
    """Whether the calling thread's last NT-selecting BatchNorm launch took the nontemporal form (None: none yet)."""
    v = int(lib().nbdt_debug_last_stream_nt())
    return None if v < 0 else bool(v)


def padded(B, H, W, C, device, dtype=torch.bfloat16):
    """Zero-initialised padded NHWC activation buffer: bf16 (the product path), or fp32 for the engines'
    verification-only reference mode (see _ref below)."""
    return torch.zeros((B, H + 2, W + 2, C), dtype=dtype, device=device)


def _no_ref(t, what):
    if t.dtype == torch.float32:
        raise RuntimeError(f"fp32 reference mode has no twin of {what}")


def _ref(t):
    """fp32 padded tensors select the verification-only kernels of csrc/ref_fp32.hip (engine.set_reference_fp32): same
    operator, same descriptors, fp32 storage.  The product path never creates an fp32 activation buffer."""
    return t.dtype == torch.float32


def interior(t):
    """[B, H, W, C] view of the interior of a padded buffer."""
    return t[:, 1:-1, 1:-1, :]


_DEV_INDEX = {}


def stream_ptr(device):
    """Raw handle of torch's CURRENT stream on `device` (what every launch goes to).  torch._C._cuda_getCurrentRawStream is the
    one C call behind torch.cuda.current_stream(...).cuda_stream without the Stream object and the device-index resolution
    around it: a quarter of the host time of a ResNet18 / CIFAR10 step, which is bound by the launch path."""
    idx = _DEV_INDEX.get(device)
    if idx is None:
        d = torch.device(device)
        idx = _DEV_INDEX[device] = d.index if d.index is not None else torch.cuda.current_device()
    return ctypes.c_void_p(_raw_stream(idx))


def _raw_stream_public(idx):
    return torch.cuda.current_stream(idx).cuda_stream


# (a private binding: present in every torch this repo has met, but do not depend on it)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", _raw_stream_public)


def _fill(desc_arr, values):
    for i, v in enumerate(values):
        desc_arr[i] = int(v)


# ------------------------------------------------------------------------------------------------
# tap tables

def conv_fwd_desc(B, Hi, Wi, cin, cout, k, stride):
    """Conv2d(k in {1,3}, padding=k//2, stride) forward: in [B,Hi,Wi,cin] -> out [B,Hi/s,Wi/s,cout]."""
    assert k in (1, 3) and Hi % stride == 0 and Wi % stride == 0
    Ho, Wo = Hi // stride, Wi // stride
    d = ConvDesc()
    d.B, d.gh, d.gw, d.cin, d.cout = B, Ho, Wo, cin, cout
    rowi = (Wi + 2) * cin
    if k == 3:
        d.ntaps = d.w_ntaps = 9
        _fill(d.tap_off, [r * rowi + s * cin for r in range(3) for s in range(3)])
        _fill(d.w_tap, range(9))
        d.in_base = 0
    else:
        d.ntaps = d.w_ntaps = 1
        d.tap_off[0] = 0
        d.w_tap[0] = 0
        d.in_base = rowi + cin
    d.in_bs, d.in_hs, d.in_ws = (Hi + 2) * rowi, stride * rowi, stride * cin
    rowo = (Wo + 2) * cout
    d.out_bs, d.out_hs, d.out_ws, d.out_base = (Ho + 2) * rowo, rowo, cout, rowo + cout
    d.accumulate = 0
    d.wide_tile = 1      # forward launches run alone on the GPU (data gradients share it with weight gradients)
    return d


def conv_dgrad_descs(B, Hi, Wi, cin, cout, k, stride, accumulate=False):
    """Data gradient of the conv above: g_out [B,Ho,Wo,cout] -> g_in [B,Hi,Wi,cin].

    Returns a list of launches (1 for stride 1; 4 output-parity classes for a strided 3x3).  The
    weight operand is the tap-reversed transposed copy ``wd[cin][taps][cout]``.
    """
    assert k in (1, 3) and stride in (1, 2)
    Ho, Wo = Hi // stride, Wi // stride
    rowg = (Wo + 2) * cout          # gradient (kernel input) row, channels = cout
    rowx = (Wi + 2) * cin           # g_in (kernel output) row, channels = cin
    out = []
    if k == 1:
        d = ConvDesc()
        d.B, d.gh, d.gw, d.cin, d.cout = B, Ho, Wo, cout, cin
        d.ntaps = d.w_ntaps = 1
        d.tap_off[0] = 0
        d.w_tap[0] = 0
        d.in_bs, d.in_hs, d.in_ws, d.in_base = (Ho + 2) * rowg, rowg, cout, rowg + cout
        d.out_bs, d.out_hs, d.out_ws, d.out_base = (Hi + 2) * rowx, stride * rowx, stride * cin, rowx + cin
        d.accumulate = 1 if accumulate else 0
        if stride == 2 and not accumulate:
            raise ValueError("a strided 1x1 dgrad only touches every other pixel: use accumulate=True "
                             "into a fully written buffer")
        return [d]
    if stride == 1:
        d = ConvDesc()
        d.B, d.gh, d.gw, d.cin, d.cout = B, Hi, Wi, cout, cin
        d.ntaps = d.w_ntaps = 9
        _fill(d.tap_off, [r * rowg + s * cout for r in range(3) for s in range(3)])
        _fill(d.w_tap, range(9))     # wd is already tap-reversed
        d.in_bs, d.in_hs, d.in_ws, d.in_base = (Ho + 2) * rowg, rowg, cout, 0
        d.out_bs, d.out_hs, d.out_ws, d.out_base = (Hi + 2) * rowx, rowx, cin, rowx + cin
        d.accumulate = 1 if accumulate else 0
        return [d]
    # stride 2, 3x3: padded input row hp = 2*ho + r.  hp odd (=2i+1): r=1, ho=i.
    # hp even (=2i+2): r=0 -> ho=i+1 ; r=2 -> ho=i.  Same for columns.  g rows are padded (+1).
    taps_1d = {1: [(1, 1)], 0: [(0, 2), (2, 1)]}   # parity -> [(r, padded g row shift)]
    for ph in (1, 0):
        for pw in (1, 0):
            d = ConvDesc()
            d.B, d.gh, d.gw, d.cin, d.cout = B, Ho, Wo, cout, cin
            taps = [(r, sr, s, sc) for (r, sr) in taps_1d[ph] for (s, sc) in taps_1d[pw]]
            d.ntaps, d.w_ntaps = len(taps), 9
            _fill(d.tap_off, [sr * rowg + sc * cout for (_, sr, _, sc) in taps])
            _fill(d.w_tap, [8 - (3 * r + s) for (r, _, s, _) in taps])
            d.in_bs, d.in_hs, d.in_ws, d.in_base = (Ho + 2) * rowg, rowg, cout, 0
            hp0, wp0 = (1 if ph else 2), (1 if pw else 2)
            d.out_bs, d.out_hs, d.out_ws = (Hi + 2) * rowx, 2 * rowx, 2 * cin
            d.out_base = hp0 * rowx + wp0 * cin
            d.accumulate = 1 if accumulate else 0
            out.append(d)
    return out


CONV_FORMS = {0: "conv_igemm_dma", 1: "4-wave 256-pixel", 2: "ping-pong 512-pixel", 3: "ping-pong 512-pixel, padded pitch",
              4: "ping-pong 256-pixel half tiles"}


def conv_plan(desc):
    """(form, ksplit) a launch of this descriptor would take -- host only (nbdt_conv_plan in include/nbdt_hip.h)."""
    form, ks = ctypes.c_int32(0), ctypes.c_int32(0)
    check(lib().nbdt_conv_plan(ctypes.byref(desc), ctypes.byref(form), ctypes.byref(ks)))
    return form.value, ks.value


def conv_wgrad_desc(B, Hi, Wi, cin, cout, k, stride):
    Ho, Wo = Hi // stride, Wi // stride
    d = WgradDesc()
    d.B, d.gh, d.gw, d.cin, d.cout = B, Ho, Wo, cin, cout
    rowi = (Wi + 2) * cin
    if k == 3:
        d.ntaps = d.w_ntaps = 9
        _fill(d.tap_off, [r * rowi + s * cin for r in range(3) for s in range(3)])
        _fill(d.w_tap, range(9))
        d.x_base = 0
    else:
        d.ntaps = d.w_ntaps = 1
        d.tap_off[0] = 0
        d.w_tap[0] = 0
        d.x_base = rowi + cin
    d.x_bs, d.x_hs, d.x_ws = (Hi + 2) * rowi, stride * rowi, stride * cin
    rowo = (Wo + 2) * cout
    d.g_bs, d.g_hs, d.g_ws, d.g_base = (Ho + 2) * rowo, rowo, cout, rowo + cout
    return d


# ------------------------------------------------------------------------------------------------
# optional per-launch timing of the MFMA kernels with HIP events on the launch stream (bench.py)

class KernelTimer:
    """Brackets every conv_igemm / conv_wgrad launch with HIP events on the stream the kernel is
    launched on (torch's current stream) and accumulates algorithmic flops per kernel family."""

    def __init__(self, only=None):
        self.items = []   # (kind, flops, start_event, end_event)
        self.only = only  # restrict to these kinds (None: all)
        self.kernels = {}  # device kernel name (nbdt_debug_last_igemm / _wgrad) -> launches bracketed

    def wants(self, kind):
        return self.only is None or kind in self.only

    def bracket(self, kind, flops, device):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        self.items.append((kind, flops, s, e))
        return s, e

    def count(self, kernel_name):
        self.kernels[kernel_name] = self.kernels.get(kernel_name, 0) + 1

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for kind, flops, s, e in self.items:
            d = out.setdefault(kind, {"launches": 0, "flops": 0.0, "ms": 0.0})
            d["launches"] += 1
            d["flops"] += flops
            d["ms"] += s.elapsed_time(e)
        for d in out.values():
            d["avg_us"] = 1e3 * d["ms"] / max(d["launches"], 1)
            d["tflops"] = d["flops"] / (d["ms"] * 1e-3) / 1e12 if d["ms"] > 0 else 0.0
        return out


_timer = None


def set_timer(t):
    global _timer
    _timer = t


# ------------------------------------------------------------------------------------------------
# launches

def conv_igemm(desc, inp, w_bf16, out, residual=None, bn_scratch=None):
    """bn_scratch: also accumulate the output's per-channel sum / sum-of-squares for the next BatchNorm."""
    if _ref(inp):
        check(lib().nbdt_ref_conv(ctypes.byref(desc), ptr(inp), ptr(w_bf16), ptr(out), ptr(residual),
                                  stream_ptr(inp.device)))
        if bn_scratch is not None:      # the epilogue's statistics: row 0 of the partial table, folded by bn_finalize
            B, H, W, C = _dims(out)
            check(lib().nbdt_ref_bn_stats(ptr(out), B, H, W, C, BN_EPS, BN_MOMENTUM, None, None, None, None,
                                          ptr(bn_scratch), stream_ptr(inp.device)))
        return
    ev = None
    if _timer is not None and _timer.wants("conv_igemm"):
        flops = desc_flops(desc)
        ev = _timer.bracket("conv_igemm", flops, inp.device)
        ev[0].record()
    if bn_scratch is None:
        check(lib().nbdt_conv_igemm(ctypes.byref(desc), ptr(inp), ptr(w_bf16), ptr(out), ptr(residual),
                                    stream_ptr(inp.device)))
    else:
        check(lib().nbdt_conv_igemm_stats(ctypes.byref(desc), ptr(inp), ptr(w_bf16), ptr(out), ptr(residual),
                                          ptr(bn_scratch), stream_ptr(inp.device)))
    if ev is not None:
        ev[1].record()
        _timer.count(last_igemm_kernel_full())


def conv_pw(desc, inp, w_bf16, out, bn_scratch=None):
    """Stride-1 1x1 convolution (forward or data gradient) on the pointwise GEMM kernel (nbdt_conv_pw, csrc/conv_pw.hip);
    bn_scratch as in conv_igemm.  fp32 tensors (the engines' reference mode) go to the fp32 reference kernel."""
    if _ref(inp):
        conv_igemm(desc, inp, w_bf16, out, None, bn_scratch)
        return
    ev = None
    if _timer is not None and _timer.wants("conv_igemm"):
        flops = desc_flops(desc)
        ev = _timer.bracket("conv_igemm", flops, inp.device)
        ev[0].record()
    check(lib().nbdt_conv_pw(ctypes.byref(desc), ptr(inp), ptr(w_bf16), ptr(out), ptr(bn_scratch),
                             stream_ptr(inp.device)))
    if ev is not None:
        ev[1].record()
        _timer.count(last_igemm_kernel_full())


def desc_flops(desc):
    """Algorithmic flops of one conv / data-gradient / weight-gradient launch: 2 x pixels x taps x cin x cout with the
    layer's REAL channel counts when the engine attached them (desc.flop_channels; the kernels multiply channels padded
    to 32 -- WRN's first unit 16 -> 32 -- and round 4's roofline counted those, +0.5 %), else the descriptor's own."""
    cin, cout = getattr(desc, "flop_channels", (desc.cin, desc.cout))
    return 2.0 * desc.B * desc.gh * desc.gw * desc.ntaps * cin * cout


def conv_igemm_multi(descs, inp, w_bf16, out):
    """The launches of `descs` (<= 4, same operands: the parity classes of a strided 3x3 data gradient) in one grid."""
    if _ref(inp):
        for d in descs:
            check(lib().nbdt_ref_conv(ctypes.byref(d), ptr(inp), ptr(w_bf16), ptr(out), None, stream_ptr(inp.device)))
        return
    arr = (ConvDesc * len(descs))(*descs)
    ev = None
    if _timer is not None and _timer.wants("conv_igemm"):
        flops = sum(desc_flops(d) for d in descs)
        ev = _timer.bracket("conv_igemm", flops, inp.device)
        ev[0].record()
    check(lib().nbdt_conv_igemm_multi(arr, len(descs), ptr(inp), ptr(w_bf16), ptr(out), stream_ptr(inp.device)))
    if ev is not None:
        ev[1].record()
        _timer.count(last_igemm_kernel_full())


def conv_igemm_bnbwd(desc, inp, w_bf16, out, bn_x, mean, rstd, gamma, beta, partials):
    """dgrad launch that also produces the BatchNorm-backward sums of (out, bn_x) as per-tile partials."""
    _no_ref(inp, "conv_igemm_bnbwd (fused BatchNorm-backward sums): use the split or the unfused schedule")
    ev = None
    if _timer is not None and _timer.wants("conv_igemm"):
        flops = desc_flops(desc)
        ev = _timer.bracket("conv_igemm", flops, inp.device)
        ev[0].record()
    check(lib().nbdt_conv_igemm_bnbwd(ctypes.byref(desc), ptr(inp), ptr(w_bf16), ptr(out), ptr(bn_x), ptr(mean),
                                      ptr(rstd), ptr(gamma), ptr(beta), ptr(partials), stream_ptr(inp.device)))
    if ev is not None:
        ev[1].record()
        _timer.count(last_igemm_kernel_full())


def conv_igemm_affine(desc, inp, w_bf16, out, scale, shift, act=1, residual=None):
    """Inference launch: out = act(conv * scale[c] + shift[c] [+ residual]) (act: 0 none, 1 ReLU, 2 swish)."""
    _no_ref(inp, "conv_igemm_affine (folded eval-mode BatchNorm): engine.fuse_eval is off in reference mode")
    check(lib().nbdt_conv_igemm_affine(ctypes.byref(desc), ptr(inp), ptr(w_bf16), ptr(out), ptr(residual),
                                       ptr(scale), ptr(shift), act, stream_ptr(inp.device)))


def bn_bwd_fused(gy, x, mean, rstd, gamma, beta, partials, dsum, dgamma, dbeta, gx, gx_add=None, cus=0):
    """BatchNorm(+ReLU) backward when the producing dgrad already left the reduction partials.
    cus > 0: the apply pass runs on that many CUs only (nbdt_bn_bwd_apply_cus) -- the caller has a weight gradient
    with cu_budget = 256 - cus in flight on another stream."""
    _no_ref(x, "bn_bwd_fused: use the split or the unfused schedule")
    B, H, W, C = _dims(x)
    st = stream_ptr(x.device)
    check(lib().nbdt_bn_bwd_fold(B, H, W, C, ptr(partials), ptr(dsum), ptr(dgamma), ptr(dbeta), st))
    if cus > 0:
        check(lib().nbdt_bn_bwd_apply_cus(ptr(gy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(dsum),
                                          ptr(gx_add), B, H, W, C, ptr(gx), int(cus), st))
        return
    check(lib().nbdt_bn_bwd_apply(ptr(gy), None, ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta),
                                  ptr(dsum), ptr(gx_add), 1, B, H, W, C, ptr(gx), None, st))


def bn_bwd_cus(gy, x, mean, rstd, gamma, beta, scratch, dsum, dgamma, dbeta, gx, cus, gx_add=None):
    """Whole BatchNorm(+ReLU) backward -- sums, fold, elementwise pass -- on `cus` CUs (no partials from a dgrad
    epilogue needed).  scratch: one zeroed 32-slot buffer (nbdt_bn_bwd_reduce_cus + nbdt_bn_bwd_apply_cus, three
    launches), or a PAIR (slots, slots_other) of them: nbdt_bn_bwd_cus, two launches -- the fold runs in the prologue of
    the elementwise pass; `slots` is left dirty and `slots_other` zeroed, so the caller swaps them for the next call."""
    B, H, W, C = _dims(x)
    st = stream_ptr(x.device)
    if _ref(x):
        check(lib().nbdt_ref_bn_bwd(ptr(gy), None, None, ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), 1,
                                    ptr(gx_add), B, H, W, C, 1, ptr(dsum), ptr(dgamma), ptr(dbeta), ptr(gx), None, st))
        return
    if isinstance(scratch, (tuple, list)):
        slots, other = scratch
        check(lib().nbdt_bn_bwd_cus(ptr(gy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(gx_add), B, H, W,
                                    C, ptr(slots), ptr(other), ptr(dsum), ptr(dgamma), ptr(dbeta), ptr(gx), int(cus),
                                    st))
        return
    check(lib().nbdt_bn_bwd_reduce_cus(ptr(gy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), B, H, W, C,
                                       ptr(scratch), ptr(dsum), ptr(dgamma), ptr(dbeta), int(cus), st))
    check(lib().nbdt_bn_bwd_apply_cus(ptr(gy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(dsum),
                                      ptr(gx_add), B, H, W, C, ptr(gx), int(cus), st))


def conv_wgrad(desc, x, gy, dw, cu_budget=0):
    """cu_budget: size the launch for that many CUs (0 = all) -- see nbdt_wgrad_desc.cu_budget."""
    desc.cu_budget = int(cu_budget)
    if _ref(x):
        check(lib().nbdt_ref_wgrad(ctypes.byref(desc), ptr(x), ptr(gy), ptr(dw), stream_ptr(x.device)))
        return
    ev = None
    if _timer is not None and _timer.wants("conv_wgrad"):
        flops = desc_flops(desc)
        ev = _timer.bracket("conv_wgrad", flops, x.device)
        ev[0].record()
    check(lib().nbdt_conv_wgrad(ctypes.byref(desc), ptr(x), ptr(gy), ptr(dw), stream_ptr(x.device)))
    if ev is not None:
        ev[1].record()


def conv_wgrad_blocks(desc, cu_budget=0):
    """Thread blocks (= CUs, for the 8-wave kernel) the weight-gradient launch of `desc` will use with that budget;
    0 when the launch is not one of the CU-budgeted dense 3x3 kernels."""
    desc.cu_budget = int(cu_budget)
    return int(lib().nbdt_conv_wgrad_blocks(ctypes.byref(desc)))


MI355X_CUS, MI355X_XCDS = 256, 8


def cu_topology_is_mi355x(device):
    """The CU-sharing arithmetic below is MI355X's: 256 CUs in 8 XCDs of 32, thread blocks dealt to the XCDs
    round-robin.  Anything else (MI300X: 304 CUs, 38 per XCD) gets no sharing rather than a wrong split."""
    props = torch.cuda.get_device_properties(device)
    return props.multi_processor_count == MI355X_CUS and "gfx950" in getattr(props, "gcnArchName", "gfx950")


def plan_cu_share(desc, elements, tensors, gbps_per_cu, target_us, min_cus, max_cus):
    """(CU budget of the weight gradient of `desc`, CUs of the HBM-bound pass of `tensors` tensors of `elements` bf16
    that runs beside it).  n = bytes / (gbps_per_cu x target_us), clamped to [max(8, min_cus), max_cus]; then the XCD
    rule: thread blocks go to the 8 XCDs round-robin by block index, per kernel -- the weight gradient's blocks (a
    whole number of pixel splits per (cout, cin) tile: 205 for a budget of 208, 160 for 232 with 80 tiles) put
    ceil(blocks / 8) on each XCD, so the pass may take 32 minus that on EACH.  One block more on any XCD waits for a
    weight-gradient block to finish there and the pass takes as long as both (measured: 19.1 -> 27 ms per step
    whenever the dispatch order fell that way).  A budget whose blocks would leave the pass less than one CU per XCD
    is lowered by 8 until they do, so the pass never gets 0 CUs.  Host arithmetic only."""
    held = (reserved_cus() + MI355X_XCDS - 1) // MI355X_XCDS      # per XCD: CUs a collective's kernels hold right now
    per_xcd = MI355X_CUS // MI355X_XCDS - held
    cus = per_xcd * MI355X_XCDS                                    # what the pair has to share
    n = int(round(elements * 2 * tensors / (gbps_per_cu * 1e9 * target_us * 1e-6)))
    n = max(max(8, int(min_cus)), min(int(max_cus), n))
    n = min(n, cus - MI355X_XCDS)
    while True:
        blocks = conv_wgrad_blocks(desc, cus - n)
        if not 0 < blocks <= cus - n:             # not the one-block-per-CU kernel (small problems): the model's n
            return cus - n, n
        free = MI355X_XCDS * (per_xcd - (blocks + MI355X_XCDS - 1) // MI355X_XCDS)
        if free >= MI355X_XCDS or n + MI355X_XCDS > cus - MI355X_XCDS:
            return cus - n, max(free, MI355X_XCDS)
        n += MI355X_XCDS


def weight_prep(w_fp32, cout, taps, cin, w_bf16=None, wd_bf16=None):
    check(lib().nbdt_weight_prep(ptr(w_fp32), cout, taps, cin, ptr(w_bf16), ptr(wd_bf16),
                                 stream_ptr(w_fp32.device)))


def weight_tile_batched(src_bf16, table, n, total, dst_bf16):
    check(lib().nbdt_weight_tile_batched(ptr(src_bf16), ptr(table), n, total, ptr(dst_bf16),
                                         stream_ptr(src_bf16.device)))


def weight_tiles(w_bf16):
    """One [rows][9][k] bf16 weight matrix (forward weights, or the transposed data-gradient copy) re-stored as the
    DMA-ordered tiles the dense 3x3 kernels read (desc.w_tiled): the single-matrix form of weight_tile_batched."""
    rows, taps, k = w_bf16.shape
    assert taps == 9 and rows % 32 == 0 and k % 32 == 0
    r32 = rows // 32
    nt = 5 if r32 % 5 == 0 else 4 if r32 % 4 == 0 else 2 if r32 % 2 == 0 else 1
    total = (rows // (32 * nt)) * (k // 32) * 9
    table = torch.tensor([[0, 0, rows, k, 0]], dtype=torch.int64, device=w_bf16.device)
    dst = torch.empty(rows * 9 * k, dtype=torch.bfloat16, device=w_bf16.device)
    weight_tile_batched(w_bf16.contiguous(), table, 1, total, dst)
    return dst


def last_igemm_kernel():
    """Name of the device kernel this thread's last conv_igemm* call launched (tests assert on it)."""
    return lib().nbdt_debug_last_igemm().decode()


def last_igemm_kernel_full():
    """... with its template arguments, as rocprofv3 prints the device kernel (bench.py's traffic guard)."""
    return lib().nbdt_debug_last_igemm_full().decode()


def last_wgrad_kernel():
    return lib().nbdt_debug_last_wgrad().decode()


def weight_prep_batched(flat, table, n_layers, total, wd_flat):
    check(lib().nbdt_weight_prep_batched(ptr(flat), ptr(table), n_layers, total, ptr(wd_flat),
                                         stream_ptr(flat.device)))


def _dims(t):
    B, Hp, Wp, C = t.shape
    return B, Hp - 2, Wp - 2, C


# ------------------------------------------------------------------------------------------------
# grouped 3x3 convolution (csrc/conv_group.hip): B, H, W below are always the conv's INPUT batch and sides

GROUP_CG = (4, 8, 16, 32)      # channels per group the kernels take (each divides the 32-channel MFMA block)


def conv_group_weight_prep(w_fp32, width, cg, wf_bf16=None, wd_bf16=None):
    """fp32 master [width][9][cg] -> block-diagonal bf16 blocks: forward wf[width/32][32][9][32] and / or the transposed,
    tap-reversed data-gradient blocks wd (nbdt_conv_group_weight_prep)."""
    check(lib().nbdt_conv_group_weight_prep(ptr(w_fp32), width, cg, ptr(wf_bf16), ptr(wd_bf16),
                                            stream_ptr(w_fp32.device)))


def conv_group_weight_prep_batched(flat, table, n_layers, total_blocks, wf_flat=None, wd_flat=None):
    check(lib().nbdt_conv_group_weight_prep_batched(ptr(flat), ptr(table), n_layers, total_blocks, ptr(wf_flat),
                                                    ptr(wd_flat), stream_ptr(flat.device)))


def conv_group_fwd(x, w, out, cg, stride, scale=None, shift=None, act=0):
    """out = conv3x3(x, groups = width / cg).  bf16 tensors: w = the expanded forward blocks; scale / shift / act: the eval
    epilogue act(acc * scale[c] + shift[c]).  fp32 tensors (the engines' reference mode): w = the fp32 master."""
    B, H, W, C = _dims(x)
    st = stream_ptr(x.device)
    if _ref(x):
        if scale is not None:
            _no_ref(x, "conv_group_fwd's eval epilogue: engine.fuse_eval is off in reference mode")
        check(lib().nbdt_ref_conv_group_fwd(ptr(x), ptr(w), ptr(out), B, H, W, C, cg, stride, st))
        return
    check(lib().nbdt_conv_group_fwd(ptr(x), ptr(w), ptr(out), B, H, W, C, cg, stride, ptr(scale), ptr(shift), act, st))


def conv_group_dgrad(gout, w, gin, cg, stride, accumulate=False):
    """gin = data gradient of conv_group_fwd.  bf16: w = the expanded data-gradient blocks; fp32: the fp32 master.  The
    entry has no accumulate form and refuses the request."""
    B, H, W, C = _dims(gin)
    st = stream_ptr(gin.device)
    fn = lib().nbdt_ref_conv_group_dgrad if _ref(gout) else lib().nbdt_conv_group_dgrad
    check(fn(ptr(gout), ptr(w), ptr(gin), B, H, W, C, cg, stride, 1 if accumulate else 0, st))


def conv_group_wgrad(x, gout, dw, cg, stride):
    """dw[width][9][cg] fp32 += the pixel sum, in a fixed order (no atomics)."""
    B, H, W, C = _dims(x)
    fn = lib().nbdt_ref_conv_group_wgrad if _ref(x) else lib().nbdt_conv_group_wgrad
    check(fn(ptr(x), ptr(gout), ptr(dw), B, H, W, C, cg, stride, stream_ptr(x.device)))


def bn_stats(x, scratch, save_mean, save_rstd, running_mean=None, running_var=None,
             eps=BN_EPS, momentum=BN_MOMENTUM, slots_filled=False):
    """slots_filled: the producing kernel already accumulated the sums into `scratch` (fold only)."""
    B, H, W, C = _dims(x)
    if _ref(x):
        check(lib().nbdt_ref_bn_stats(ptr(x), B, H, W, C, eps, momentum, ptr(running_mean), ptr(running_var),
                                      ptr(save_mean), ptr(save_rstd), None, stream_ptr(x.device)))
        return
    check(lib().nbdt_bn_stats(None if slots_filled else ptr(x), B, H, W, C, eps, momentum, ptr(running_mean), ptr(running_var),
                              ptr(scratch), ptr(save_mean), ptr(save_rstd), stream_ptr(x.device)))


def bn_finalize(x, scratch, save_mean, save_rstd, running_mean=None, running_var=None,
                eps=BN_EPS, momentum=BN_MOMENTUM):
    """Fold sums that a conv epilogue already left in `scratch` (conv_igemm(..., bn_scratch=scratch))."""
    B, H, W, C = _dims(x)
    check(lib().nbdt_bn_finalize(B, H, W, C, eps, momentum, ptr(running_mean), ptr(running_var), ptr(scratch),
                                 ptr(save_mean), ptr(save_rstd), stream_ptr(x.device)))


def bn_apply(x, mean, rstd, gamma, beta, y, relu=True, residual=None):
    B, H, W, C = _dims(x)
    if _ref(x):
        check(lib().nbdt_ref_bn_apply(ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(residual),
                                      1 if relu else 0, B, H, W, C, ptr(y), stream_ptr(x.device)))
        return
    check(lib().nbdt_bn_apply(ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(residual),
                              1 if relu else 0, B, H, W, C, ptr(y), stream_ptr(x.device)))


def bn_bwd(gy, y, x, mean, rstd, gamma, scratch, dsum, dgamma, dbeta, gx, relu=True, gx_add=None,
           g_resid=None, beta=None):
    """y=None (allowed when the forward had no residual): the ReLU mask is recomputed from x/gamma/beta."""
    B, H, W, C = _dims(x)
    st = stream_ptr(x.device)
    r = 1 if relu else 0
    if _ref(x):
        check(lib().nbdt_ref_bn_bwd(ptr(gy), None, ptr(y), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), r,
                                    ptr(gx_add), B, H, W, C, 1, ptr(dsum), ptr(dgamma), ptr(dbeta), ptr(gx), ptr(g_resid),
                                    st))
        return
    check(lib().nbdt_bn_bwd_reduce(ptr(gy), ptr(y), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), r,
                                   B, H, W, C, ptr(scratch), ptr(dsum), ptr(dgamma), ptr(dbeta), st))
    check(lib().nbdt_bn_bwd_apply(ptr(gy), ptr(y), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta),
                                  ptr(dsum), ptr(gx_add), r, B, H, W, C, ptr(gx), ptr(g_resid), st))


def bn_relu_pool(x, mean, rstd, gamma, beta, pooled):
    B, H, W, C = _dims(x)
    if _ref(x):
        check(lib().nbdt_ref_bn_relu_pool(ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), B, H, W, C, ptr(pooled),
                                          stream_ptr(x.device)))
        return
    check(lib().nbdt_bn_relu_pool(ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), B, H, W, C,
                                  ptr(pooled), stream_ptr(x.device)))


def pool_bn_bwd(gpooled, x, mean, rstd, gamma, beta, scratch, dsum, dgamma, dbeta, gx):
    B, H, W, C = _dims(x)
    st = stream_ptr(x.device)
    if _ref(x):
        check(lib().nbdt_ref_bn_bwd(None, ptr(gpooled), None, ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), 1,
                                    None, B, H, W, C, 1, ptr(dsum), ptr(dgamma), ptr(dbeta), ptr(gx), None, st))
        return
    check(lib().nbdt_pool_bn_bwd_reduce(ptr(gpooled), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta),
                                        B, H, W, C, ptr(scratch), ptr(dsum), ptr(dgamma), ptr(dbeta), st))
    check(lib().nbdt_pool_bn_bwd_apply(ptr(gpooled), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta),
                                       ptr(dsum), B, H, W, C, ptr(gx), st))


def pool_bn_bwd_apply(gpooled, x, mean, rstd, gamma, beta, dsum, gx):
    """Elementwise pass of the pooled head's backward alone, with the caller's sums (ResNetEngine: a plain average pool
    is an identity BatchNorm with zero batch sums)."""
    B, H, W, C = _dims(x)
    st = stream_ptr(x.device)
    if _ref(x):
        check(lib().nbdt_ref_bn_bwd(None, ptr(gpooled), None, ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), 1,
                                    None, B, H, W, C, 0, ptr(dsum), None, None, ptr(gx), None, st))
        return
    check(lib().nbdt_pool_bn_bwd_apply(ptr(gpooled), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(dsum),
                                       B, H, W, C, ptr(gx), st))


def conv_out_size(h, stride):
    """Output extent of a strided convolution of this package: ceil(h / stride), for both padding rules."""
    return -(-int(h) // int(stride))


def conv_padding(h, k, stride, same=False):
    """(low, high) zero padding of one axis of a k-tap convolution with conv_out_size(h, stride) outputs.  same=False:
    PyTorch's symmetric padding=k // 2.  same=True: TensorFlow's "SAME" rule, total = max((out - 1) * stride + k - h, 0)
    with the odd pixel on the high side; it differs from the symmetric rule only for stride 2 on an even extent
    (k = 3: (0, 1), k = 5: (1, 2))."""
    if not same or stride == 1:
        return k // 2, k // 2
    total = max((conv_out_size(h, stride) - 1) * stride + k - int(h), 0)
    return total // 2, total - total // 2


def _check_out(x_hw, y, stride):
    want = (conv_out_size(x_hw[0], stride) + 2, conv_out_size(x_hw[1], stride) + 2)
    if tuple(y.shape[1:3]) != want:
        raise ValueError(f"output tensor is {tuple(y.shape[1:3])} with its border, the convolution writes {want}")


def stem_conv(img, w, out, cout_real, stride=1, pad=None):
    """pad: None = padding 1 on extents the stride divides; (top, left) = the low-side padding of
    nbdt_stem_conv_pad, any extents."""
    B, _, H, W = img.shape
    if pad is not None:
        _check_out((H, W), out, stride)
        fn = lib().nbdt_ref_stem_conv_pad if _ref(out) else lib().nbdt_stem_conv_pad
        check(fn(ptr(img), ptr(w), B, H, W, cout_real, out.shape[3], stride, int(pad[0]), int(pad[1]), ptr(out),
                 stream_ptr(img.device)))
        return
    if _ref(out):
        check(lib().nbdt_ref_stem_conv(ptr(img), ptr(w), B, H, W, cout_real, out.shape[3], stride, ptr(out),
                                       stream_ptr(img.device)))
        return
    check(lib().nbdt_stem_conv(ptr(img), ptr(w), B, H, W, cout_real, out.shape[3], stride, ptr(out),
                               stream_ptr(img.device)))


def stem_wgrad(img, gy, dw, cout_real, stride=1, pad=None):
    B, _, H, W = img.shape
    if pad is not None:
        _check_out((H, W), gy, stride)
        fn = lib().nbdt_ref_stem_wgrad_pad if _ref(gy) else lib().nbdt_stem_wgrad_pad
        check(fn(ptr(img), ptr(gy), B, H, W, cout_real, gy.shape[3], stride, int(pad[0]), int(pad[1]), ptr(dw),
                 stream_ptr(img.device)))
        return
    if _ref(gy):
        check(lib().nbdt_ref_stem_wgrad(ptr(img), ptr(gy), B, H, W, cout_real, gy.shape[3], stride, ptr(dw),
                                        stream_ptr(img.device)))
        return
    check(lib().nbdt_stem_wgrad(ptr(img), ptr(gy), B, H, W, cout_real, gy.shape[3], stride, ptr(dw),
                                stream_ptr(img.device)))


def _storage(t):
    return _C.NBDT_F32 if t.dtype == torch.float32 else _C.NBDT_BF16


def stem_patches(img, out, k=7, stride=2):
    """nbdt_stem_patches: fp32 NCHW img [B,3,H,W] -> the interior of the padded NHWC patch tensor out
    [B, H/stride+2, W/stride+2, cpad], channel (r*k + s)*3 + ci, zeros from 3*k*k on; out is bf16 or (reference mode) fp32.
    The k x k / stride / pad k/2 convolution is the 1x1 convolution of `out` (conv_igemm, conv_wgrad)."""
    B, _, H, W = img.shape
    check(lib().nbdt_stem_patches(ptr(img), B, H, W, int(k), int(stride), out.shape[3], _storage(out), ptr(out),
                                  stream_ptr(img.device)))


def maxpool_fwd(x, y, idx=None):
    """nbdt_maxpool3x3s2_fwd: MaxPool2d(3, 2, 1) of padded x [B,H+2,W+2,C] into padded y [B,H/2+2,W/2+2,C]; idx (training):
    uint8 [B,H/2,W/2,C], the winner's window position 3*dy + dx."""
    B, H, W, C = _dims(x)
    check(lib().nbdt_maxpool3x3s2_fwd(ptr(x), _storage(x), B, H, W, C, ptr(y), ptr(idx), stream_ptr(x.device)))


def maxpool_bwd(gy, idx, gx):
    """nbdt_maxpool3x3s2_bwd: gx [B,H+2,W+2,C] (every interior element written) from gy [B,H/2+2,W/2+2,C] and the forward's
    idx; a gather with an fp32 sum in a fixed order, no atomics."""
    B, H, W, C = _dims(gx)
    check(lib().nbdt_maxpool3x3s2_bwd(ptr(gy), ptr(idx), _storage(gy), B, H, W, C, ptr(gx), stream_ptr(gx.device)))


# the batch launches of the data path (augment.hip, policy.hip, resample.hip): their small converters and their one call
_M64 = (1 << 64) - 1


def _f3(v):
    return None if v is None else (ctypes.c_float * 3)(*[float(a) for a in v])


def _d2(v):
    return None if v is None else (ctypes.c_double * 2)(*[float(a) for a in v])


def _batch_call(plain, sharded, src, labels_src, index, index_base, tail):
    """The plain entry, or with index_base its _sharded twin (index_base goes in after `index`)."""
    dtype = _C.NBDT_U8 if src.dtype == torch.uint8 else _C.NBDT_F32
    if index_base is None:
        check(plain(ptr(src), dtype, ptr(labels_src), ptr(index), *tail))
    else:
        check(sharded(ptr(src), dtype, ptr(labels_src), ptr(index), int(index_base), *tail))


def augment_batch(src, labels_src, index, out, labels_out, pad, flip, mean=None, std=None, fill=None, seed=0, epoch=0,
                  params_in=None, params_out=None, index_base=None):
    """nbdt_augment_batch: out[B,3,H,W] fp32, labels_out[B] <- gather + zero-padded random crop + flip (+ /255 and normalise
    for a uint8 `src`) of src[N,3,H,W] at `index` (int64 [B], device).  mean / std / fill: three host floats each.
    index_base (nbdt_augment_batch_sharded): `src` holds the samples [index_base, index_base + N) of the dataset `index`
    names; the draw uses `index`, the gather `index - index_base`."""
    N, _, H, W = src.shape
    tail = (index.shape[0], N, H, W, int(pad), 1 if flip else 0, _f3(mean), _f3(std), _f3(fill), int(seed) & _M64,
            int(epoch) & _M64, ptr(params_in), ptr(out), ptr(labels_out), ptr(params_out), stream_ptr(src.device))
    _batch_call(lib().nbdt_augment_batch, lib().nbdt_augment_batch_sharded, src, labels_src, index, index_base, tail)


def policy_batch(src, labels_src, index, out, labels_out, pad, flip, mean, std, policy=False, policy_table=None,
                 erase_prob=0.0, erase_scale=None, erase_ratio=None, ratio_table=None, seed=0, epoch=0, params_in=None,
                 policy_in=None, params_out=None, policy_out=None, index_base=None):
    """nbdt_policy_batch: augment_batch for a uint8 `src` of at most 49152 bytes per image, with one TrivialAugmentWide
    operation per image between the flip and the normalisation (policy=True; policy_table: int32 [14,31,2,6], device) and
    RandomErasing(value=0) after it (erase_prob; erase_scale / erase_ratio: two host floats each; ratio_table: fp64 [4096],
    device).  policy_in / policy_out: int32 [B,7] (op, bin, sign, top, left, h, w), device; policy_in replaces the policy
    and erase draw.  index_base: nbdt_policy_batch_sharded, as for augment_batch."""
    N, _, H, W = src.shape
    tail = (index.shape[0], N, H, W, int(pad), 1 if flip else 0, _f3(mean), _f3(std),
            _C.NBDT_POLICY_TA_WIDE if policy else _C.NBDT_POLICY_NONE, ptr(policy_table), float(erase_prob), _d2(erase_scale),
            _d2(erase_ratio), ptr(ratio_table), int(seed) & _M64, int(epoch) & _M64, ptr(params_in), ptr(policy_in),
            ptr(out), ptr(labels_out), ptr(params_out), ptr(policy_out), stream_ptr(src.device))
    _batch_call(lib().nbdt_policy_batch, lib().nbdt_policy_batch_sharded, src, labels_src, index, index_base, tail)


def policy_chain_batch(src, labels_src, index, out, labels_out, pad, flip, mean, std, table, nbins, num_ops=0, magnitude=0,
                       subpolicies=None, erase_prob=0.0, erase_scale=None, erase_ratio=None, ratio_table=None, seed=0,
                       epoch=0, params_in=None, chain_in=None, erase_in=None, params_out=None, chain_out=None,
                       erase_out=None, index_base=None):
    """nbdt_policy_chain_batch: policy_batch with a chain of up to four operations per image (RandAugment, AutoAugment).
    table: int32 [15, nbins, 2, 6], device.  subpolicies: int32 [P,4,3] of (op, round(p * 2^24), bin), device -- given:
    NBDT_CHAIN_SUBPOLICY; None: NBDT_CHAIN_RAND with num_ops slots at bin `magnitude`.  chain_in / chain_out: int32 [B,4,3]
    (op, bin, sign), erase_in / erase_out: int32 [B,4] (top, left, h, w), device; the *_in replace the draws.
    index_base: nbdt_policy_chain_batch_sharded, as for augment_batch."""
    N, _, H, W = src.shape
    mode = _C.NBDT_CHAIN_RAND if subpolicies is None else _C.NBDT_CHAIN_SUBPOLICY
    tail = (index.shape[0], N, H, W, int(pad), 1 if flip else 0, _f3(mean), _f3(std), mode, int(nbins), ptr(table),
            int(num_ops), int(magnitude), ptr(subpolicies), 0 if subpolicies is None else subpolicies.shape[0],
            float(erase_prob), _d2(erase_scale), _d2(erase_ratio), ptr(ratio_table), int(seed) & _M64,
            int(epoch) & _M64, ptr(params_in), ptr(chain_in), ptr(erase_in), ptr(out), ptr(labels_out), ptr(params_out),
            ptr(chain_out), ptr(erase_out), stream_ptr(src.device))
    _batch_call(lib().nbdt_policy_chain_batch, lib().nbdt_policy_chain_batch_sharded, src, labels_src, index, index_base, tail)


def mix_batch(x, y, out, tgt, lam=1.0, box=(0, 0, 0, 0), lam_t=1.0):
    """nbdt_mix_batch: MixUp / CutMix of the fp32 batch x [B,3,H,W] (labels y, int64 [B]) with itself rolled by one, into
    out [B,3,H,W] (not x) and the probability targets tgt [B,C] fp32.  MixUp: lam, an empty box, lam_t = lam.  CutMix:
    lam = 1, box = (y1, y2, x1, x2) taken from the partner, lam_t = 1 - box area / (H*W).  lam and 1 - lam (formed in double, as torchvision
    forms it) are each rounded to fp32 once, which is what torch does with a Python scalar next to a float32 tensor."""
    B, ch, H, W = x.shape
    ok = lambda t, dt: t.is_cuda and t.dtype == dt and t.is_contiguous() and t.device == x.device
    if ch != 3 or not (ok(x, torch.float32) and ok(out, torch.float32) and ok(tgt, torch.float32) and ok(y, torch.int64)):
        raise _C.NBDTHipError("mix_batch takes contiguous device tensors: fp32 x / out [B,3,H,W], int64 y [B], fp32 tgt [B,C]")
    if tuple(out.shape) != tuple(x.shape) or tuple(y.shape) != (B,) or tgt.dim() != 2 or tgt.shape[0] != B:
        raise _C.NBDTHipError(f"mix_batch: x {tuple(x.shape)}, out {tuple(out.shape)}, y {tuple(y.shape)}, tgt {tuple(tgt.shape)}")
    lam, lam_t = float(lam), float(lam_t)
    check(lib().nbdt_mix_batch(ptr(x), ptr(y), B, H, W, lam, 1.0 - lam, int(box[0]), int(box[1]), int(box[2]), int(box[3]),
                               lam_t, 1.0 - lam_t, ptr(out), ptr(tgt), tgt.shape[1], stream_ptr(x.device)))


def resized_crop_batch(src, labels_src, index, out, labels_out, resize, window, flip, mean, std, scale=None, ratio=None,
                       ratio_table=None, seed=0, epoch=0, params_in=None, params_out=None, index_base=None):
    """nbdt_resized_crop_batch: out[B,3,out_h,out_w] fp32, labels_out[B] <- gather + crop box + PIL-bilinear resample to
    `resize` = (rs_h, rs_w), of which `window` = (top, left) + out's size is written, + flip + /255 + normalise of the uint8
    src[N,3,H,W] at `index` (int64 [B], device).  The boxes are params_in (int32 [B,5]: top, left, h, w, flip) or drawn
    from (seed, epoch, index) with `scale`, `ratio` (two host floats each) and `ratio_table` (fp64 [4096], device).
    index_base (nbdt_resized_crop_batch_sharded): `src` holds the samples [index_base, index_base + N) of the dataset
    `index` names; the draw uses `index`, the gather `index - index_base`."""
    N, _, H, W = src.shape
    tail = (index.shape[0], N, H, W, int(resize[0]), int(resize[1]), int(window[0]), int(window[1]), out.shape[2],
            out.shape[3], 1 if flip else 0, _f3(mean), _f3(std), _d2(scale), _d2(ratio), ptr(ratio_table),
            int(seed) & _M64, int(epoch) & _M64, ptr(params_in), ptr(out), ptr(labels_out), ptr(params_out),
            stream_ptr(src.device))
    _batch_call(lib().nbdt_resized_crop_batch, lib().nbdt_resized_crop_batch_sharded, src, labels_src, index, index_base, tail)


def resized_crop_policy_batch(src, labels_src, index, out, labels_out, flip, mean, std, stage_a, stage_b, scale=None,
                              ratio=None, ratio_table=None, table=None, nbins=1, num_ops=0, magnitude=0, subpolicies=None,
                              ta_wide=False, erase_prob=0.0, erase_scale=None, erase_ratio=None, erase_ratio_table=None,
                              seed=0, epoch=0, params_in=None, chain_in=None, erase_in=None, params_out=None,
                              chain_out=None, erase_out=None, index_base=None):
    """nbdt_resized_crop_policy_batch: resized_crop_batch's training transform to out[B,3,S,S] (S = out.shape[2]) with a
    chain of up to four operations on the S x S bytes between the flip and the normalisation, and RandomErasing(value=0)
    after it.  Two launches on the current stream; stage_a / stage_b: uint8 [B,3,S,S] scratch, device.  table: int32
    [15, nbins, 2, 6] built for S x S, device.  subpolicies given: NBDT_CHAIN_SUBPOLICY; ta_wide: NBDT_CHAIN_TA_WIDE (one
    slot, policy_batch's draw); else NBDT_CHAIN_RAND with num_ops (0..4; 0: the erase only) slots at bin `magnitude`.
    params_in / params_out: int32 [B,5] as resized_crop_batch; chain_in / chain_out: int32 [B,4,3]; erase_in / erase_out:
    int32 [B,4]; the *_in replace the draws.  index_base: the _sharded entry, as for resized_crop_batch."""
    N, _, H, W = src.shape
    if out.shape[2] != out.shape[3] or tuple(stage_a.shape) != tuple(out.shape) or tuple(stage_b.shape) != tuple(out.shape) \
            or stage_a.dtype != torch.uint8 or stage_b.dtype != torch.uint8:
        raise _C.NBDTHipError(f"resized_crop_policy_batch: out must be [B,3,S,S] and both staging buffers uint8 of that "
                              f"shape, got out {tuple(out.shape)}, stage_a {stage_a.dtype} {tuple(stage_a.shape)}, stage_b "
                              f"{stage_b.dtype} {tuple(stage_b.shape)}")
    if subpolicies is not None:
        mode = _C.NBDT_CHAIN_SUBPOLICY
    else:
        mode = _C.NBDT_CHAIN_TA_WIDE if ta_wide else _C.NBDT_CHAIN_RAND
    tail = (index.shape[0], N, H, W, out.shape[2], 1 if flip else 0, _f3(mean), _f3(std), _d2(scale), _d2(ratio),
            ptr(ratio_table), mode, int(nbins), ptr(table), int(num_ops), int(magnitude), ptr(subpolicies),
            0 if subpolicies is None else subpolicies.shape[0], float(erase_prob), _d2(erase_scale), _d2(erase_ratio),
            ptr(erase_ratio_table), int(seed) & _M64, int(epoch) & _M64, ptr(params_in), ptr(chain_in), ptr(erase_in),
            ptr(stage_a), ptr(stage_b), ptr(out), ptr(labels_out), ptr(params_out), ptr(chain_out), ptr(erase_out),
            stream_ptr(src.device))
    _batch_call(lib().nbdt_resized_crop_policy_batch, lib().nbdt_resized_crop_policy_batch_sharded, src, labels_src, index,
                index_base, tail)


def resized_crop_band_rows(H, W, resize, window, out_size):
    """nbdt_resized_crop_band_rows (host only): output rows per block of the LDS-staged kernel, 0 = the global-memory
    kernel runs for this geometry."""
    rows = lib().nbdt_resized_crop_band_rows(int(H), int(W), int(resize[0]), int(resize[1]), int(window[0]), int(window[1]),
                                             int(out_size[0]), int(out_size[1]))
    if rows < 0:
        check(rows)
    return rows


def linear_fwd(x, w, b, z):
    B, K = x.shape
    N = w.shape[0]
    check(lib().nbdt_linear_fwd(ptr(x), ptr(w), ptr(b), B, K, N, ptr(z), stream_ptr(x.device)))


def linear_bwd(x, w, gz, gx, gw, gb):
    B, K = x.shape
    N = w.shape[0]
    check(lib().nbdt_linear_bwd(ptr(x), ptr(w), ptr(gz), B, K, N, ptr(gx), ptr(gw), ptr(gb),
                                stream_ptr(x.device)))


STATS_FIELDS = _C.TreeStats.FIELDS
ENTROPY_ONE = 1 << 32      # node_entropy sums are integers in units of 2^-32


def tree_stats_sizes(handle):
    """Element counts of the int64 counters of nbdt_tree_stats, by field name, for one hierarchy handle."""
    C, N = handle.flat.num_classes, handle.flat.num_inodes
    return {"totals": 4, "confusion_net": C * C, "confusion_hard": C * C, "confusion_soft": C * C,
            "node_counts": N * 5, "node_entropy": N * 2, "first_error_depth": handle.max_depth + 1}


def tree_stats_accumulate(handle, z, y, stats=None, scores=None):
    """One launch of nbdt_tree_stats_accumulate: ADDS the statistics of the batch (logits z [B, C], labels y [B]) to the
    int64 device tensors in ``stats`` (a dict by nbdt_tree_stats field name; a missing or None entry is not computed)
    and WRITES the per-sample scores into ``scores`` (fp32 [B, 3], optional).  Enqueues only: no host synchronisation."""
    _C.require_gpu(z, "tree_stats_accumulate")
    z, B, ld = _C._rows(z, handle)
    block = _C.TreeStats()
    sizes = tree_stats_sizes(handle)
    for name, t in (stats or {}).items():
        if name not in sizes:
            raise _C.NBDTHipError(f"unknown statistic {name!r}; nbdt_tree_stats has {', '.join(STATS_FIELDS)}")
        if t is None:
            continue
        if t.dtype != torch.int64 or t.device != z.device or not t.is_contiguous() or t.numel() != sizes[name]:
            raise _C.NBDTHipError(f"{name}: expected a contiguous int64 tensor of {sizes[name]} elements on {z.device}, "
                                  f"got {t.dtype} {tuple(t.shape)} on {t.device}")
        setattr(block, name, t.data_ptr())
    if y is not None:
        if y.is_floating_point() or y.dim() != 1 or y.shape[0] != B:
            raise _C.NBDTHipError(f"tree_stats_accumulate takes class-index labels [B], got {y.dtype} {tuple(y.shape)}")
        y = y.to(device=z.device, dtype=torch.int64).contiguous()
    if scores is not None and (scores.dtype != torch.float32 or scores.device != z.device or not scores.is_contiguous()
                               or tuple(scores.shape) != (B, 3)):
        raise _C.NBDTHipError(f"scores: expected a contiguous fp32 [{B}, 3] tensor on {z.device}")
    check(lib().nbdt_tree_stats_accumulate(handle.h, ptr(z), _C.ztype_of(z), B, ld, ptr(y), ctypes.byref(block),
                                           ptr(scores), _C.stream_of(z)))


seg_stats_dispatch = _C.seg_stats_dispatch
SEG_STATS_FIELDS = tuple(f for f in STATS_FIELDS if f != "node_entropy")


def seg_stats_accumulate(handle, z, y, ignore_index, stats=None, want_pred=False):
    """Segmentation evaluation of one batch: ADDS the statistics of logits z [N, C, H, W] against labels y [N, H, W] to
    the int64 device tensors in ``stats`` (a dict by nbdt_tree_stats field name without node_entropy; a missing or None
    entry is not computed).  A pixel whose label is ``ignore_index`` or outside [0, C) counts nowhere.  ONE launch of
    nbdt_seg_stats_accumulate for contiguous planes; channels_last memory and hierarchies beyond the pixel limit go
    through nbdt_tree_stats_accumulate on the [N*H*W, C] rows (seg_stats_dispatch).  Enqueues only: no host
    synchronisation.  want_pred: returns (pred_net, pred_hard, pred_soft), int64 [N, H, W] each, else None."""
    _C.require_gpu(z, "seg_stats_accumulate")
    how = seg_stats_dispatch(tuple(z.shape), tuple(z.stride()), z.dtype, handle.flat)
    N, C, H, W = z.shape
    sizes = tree_stats_sizes(handle)
    block = _C.TreeStats()
    wanted = {}
    for name, t in (stats or {}).items():
        if name not in SEG_STATS_FIELDS:
            raise _C.NBDTHipError(f"unknown segmentation statistic {name!r}; there are {', '.join(SEG_STATS_FIELDS)}")
        if t is None:
            continue
        if t.dtype != torch.int64 or t.device != z.device or not t.is_contiguous() or t.numel() != sizes[name]:
            raise _C.NBDTHipError(f"{name}: expected a contiguous int64 tensor of {sizes[name]} elements on {z.device}, "
                                  f"got {t.dtype} {tuple(t.shape)} on {t.device}")
        setattr(block, name, t.data_ptr())
        wanted[name] = t
    if y is not None:
        if y.is_floating_point() or tuple(y.shape) != (N, H, W):
            raise _C.NBDTHipError(f"segmentation targets must be class indices [N, H, W] = {(N, H, W)}, got {y.dtype} "
                                  f"{tuple(y.shape)}")
        y = y.to(device=z.device, dtype=torch.int64).contiguous()
    elif wanted:
        raise _C.NBDTHipError("seg_stats_accumulate: statistics against the labels need the labels")
    if not wanted and not want_pred:
        return None
    if how in ("rows", "coerced"):
        zl = z if how == "rows" else z.contiguous(memory_format=torch.channels_last)
        rows = zl.permute(0, 2, 3, 1).reshape(-1, C)
        if wanted:
            labels = y.reshape(-1)
            labels = torch.where(labels == int(ignore_index), torch.full_like(labels, -1), labels)   # a copy
            tree_stats_accumulate(handle, rows, labels, wanted)
        if not want_pred:
            return None
        pred_hard = _C.hard_forward(handle, rows, want_onehot=False)[0]
        P = _C.soft_forward(handle, rows)                         # (single-parent hierarchies, like SoftSegNBDT)
        return tuple(p.view(N, H, W) for p in (rows.float().argmax(1), pred_hard, P.argmax(1)))
    zz = z.contiguous() if how == "contiguous" else z
    n, HW, zi, zc = _C._seg_geom(zz)
    preds = tuple(torch.empty((N, H, W), dtype=torch.int64, device=z.device) for _ in range(3)) if want_pred \
        else (None, None, None)
    check(lib().nbdt_seg_stats_accumulate(handle.h, ptr(zz), _C.ztype_of(zz), n, HW, zi, zc, ptr(y), int(ignore_index),
                                          ctypes.byref(block), ptr(preds[0]), ptr(preds[1]), ptr(preds[2]),
                                          _C.stream_of(zz)))
    return preds if want_pred else None


def sgd_step(p, g, buf, lr, momentum, weight_decay, grad_scale=1.0, p_bf16=None, zero_grad=False):
    """zero_grad: the same pass leaves g zeroed (the next step's zero_grad())."""
    check(lib().nbdt_sgd_step(ptr(p), ptr(g), ptr(buf), p.numel(), lr, momentum, weight_decay, grad_scale,
                              ptr(p_bf16), 1 if zero_grad else 0, stream_ptr(p.device)))


def _check_fp32(what, n, p, named):
    """Every (tensor, name) of `named` that is not None: contiguous fp32, n elements, on p's device."""
    for t, name in named:
        if t is None:
            continue
        if t.dtype != torch.float32 or t.numel() != n or t.device != p.device or not t.is_contiguous():
            raise _C.NBDTHipError(f"{what}: {name} must be a contiguous fp32 tensor of {n} elements on {p.device}")


def _check_mirror(what, n, p, p_bf16):
    if p_bf16 is not None and (p_bf16.dtype != torch.bfloat16 or p_bf16.numel() != n or p_bf16.device != p.device
                               or not p_bf16.is_contiguous()):
        raise _C.NBDTHipError(f"{what}: the mirror must be a contiguous bf16 tensor of {n} elements on {p.device}")


class _ArenaPlan:
    """What the plans over a flat arena of n fp32 elements share (csrc/arena.h has the library's half): the segment rows
    as ctypes columns, the create call with `device` current -- the table is checked on the host first (a bad one raises
    without a GPU), a good one puts the plan's tables and workspace on `device` once -- the tensor checks of a step, and
    the destroy call when the plan goes.  A subclass names its entry points and the ctypes type of each row column."""
    _CREATE = _DESTROY = None
    _COLUMNS = ()

    def __init__(self, n, rows, device):
        self.n = int(n)
        self.device = torch.device(device) if device is not None else None
        self.handle = ctypes.c_void_p()
        args = [self.n]
        if self._COLUMNS:
            k = len(rows)
            self.n_seg, self.segments = k, rows
            args += [(ct * max(k, 1))(*[r[i] for r in rows]) for i, ct in enumerate(self._COLUMNS)] + [k]
        on_device = self.device is not None and self.device.type == "cuda"
        with torch.cuda.device(self.device) if on_device else contextlib.nullcontext():
            check(getattr(lib(), self._CREATE)(*args, ctypes.byref(self.handle)))

    def _check(self, what, p, named, p_bf16):
        _C.require_gpu(p, what)
        _check_fp32(what, self.n, p, named)
        _check_mirror(what, self.n, p, p_bf16)

    def __del__(self):
        try:
            h = getattr(self, "handle", None)
            if h is not None and h.value:
                getattr(lib(), self._DESTROY)(h)
                self.handle = None
        except Exception:      # (interpreter shutdown: modules may already be gone)
            pass


LARS_ITEM = 4096      # elements one wave of csrc/lars.hip reduces / updates (kItem); a block is four waves


class LarsPlan(_ArenaPlan):
    """A plan of nbdt_lars_*: `segments` = rows (offset, length, weight_decay, adapt) over a flat arena of n fp32 elements
    (sorted, disjoint, offsets multiples of 4: ParamStore.segments)."""
    _CREATE, _DESTROY = "nbdt_lars_create", "nbdt_lars_destroy"
    _COLUMNS = (ctypes.c_int64, ctypes.c_int64, ctypes.c_float, ctypes.c_int32)

    def __init__(self, n, segments, device=None):
        super().__init__(n, [(int(o), int(l), float(w), int(bool(a))) for o, l, w, a in segments], device)

    def step(self, p, g, buf, lr, momentum, trust, eps, grad_scale=1.0, p_bf16=None, zero_grad=False):
        """Three launches on p's current stream; no host synchronisation."""
        self._check("lars_step", p, ((p, "p"), (g, "g"), (buf, "buf")), p_bf16)
        check(lib().nbdt_lars_step(self.handle, ptr(p), ptr(g), ptr(buf), lr, momentum, trust, eps, grad_scale,
                                   ptr(p_bf16), 1 if zero_grad else 0, stream_ptr(p.device)))

    def ratios(self):
        """ratio[n_seg] of the last step as a host tensor (1 before the first step).  Synchronises: not for the step path."""
        out = torch.empty(self.n_seg, dtype=torch.float32)
        with torch.cuda.device(self.device):
            check(lib().nbdt_lars_ratios_to_host(self.handle, ctypes.cast(out.data_ptr(), ctypes.POINTER(ctypes.c_float)),
                                                 stream_ptr(self.device)))
        return out


ARENA_OPT_ITEM = 512      # elements one wave of csrc/adaptive.hip updates (kItem); a block is four waves


class ArenaOptPlan(_ArenaPlan):
    """A plan of nbdt_adamw_step / nbdt_rmsprop_step: `segments` = rows (offset, length, weight_decay) over a flat arena of n
    fp32 elements (sorted, disjoint, offsets multiples of 4; a fourth column, as ParamStore.segments has, is ignored).
    Every step is one launch on p's current stream, no host synchronisation."""
    _CREATE, _DESTROY = "nbdt_arena_opt_create", "nbdt_arena_opt_destroy"
    _COLUMNS = (ctypes.c_int64, ctypes.c_int64, ctypes.c_float)

    def __init__(self, n, segments, device=None):
        super().__init__(n, [(int(r[0]), int(r[1]), float(r[2])) for r in segments], device)

    def adamw(self, p, g, m, v, lr, betas, eps, t, grad_scale=1.0, p_bf16=None, zero_grad=False):
        """torch.optim.AdamW's step number t >= 1 (the decay of each row decoupled, no amsgrad)."""
        self._check("adamw_step", p, ((p, "p"), (g, "g"), (m, "m"), (v, "v")), p_bf16)
        check(lib().nbdt_adamw_step(self.handle, ptr(p), ptr(g), ptr(m), ptr(v), lr, betas[0], betas[1], eps, int(t),
                                    grad_scale, ptr(p_bf16), 1 if zero_grad else 0, stream_ptr(p.device)))

    def rmsprop(self, p, g, sq, buf, lr, alpha, eps, momentum, tf=False, grad_scale=1.0, p_bf16=None, zero_grad=False):
        """torch.optim.RMSprop's step (not centered), or with tf TensorFlow's: eps inside the root, lr inside the buffer, sq
        started at 1 by the caller.  buf may be None for the torch form with momentum 0, which does not touch it."""
        self._check("rmsprop_step", p, ((p, "p"), (g, "g"), (sq, "sq"), (buf, "buf")), p_bf16)
        check(lib().nbdt_rmsprop_step(self.handle, ptr(p), ptr(g), ptr(sq), ptr(buf), lr, alpha, eps, momentum,
                                      1 if tf else 0, grad_scale, ptr(p_bf16), 1 if zero_grad else 0,
                                      stream_ptr(p.device)))


class ClipRecord(ctypes.Structure):      # nbdt_clip_*'s 32-byte record
    _fields_ = [("norm", ctypes.c_float), ("coef", ctypes.c_float), ("clipped", ctypes.c_int32), ("steps", ctypes.c_int32),
                ("nonfinite", ctypes.c_int32), ("total_clipped", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]


class ClipPlan(_ArenaPlan):
    """A plan of nbdt_clip_*: global-norm clipping of a flat fp32 gradient arena of n elements on `device`, which gets the
    fp64 partials and the 32-byte record once, here.  norm() is two launches and apply() one on g's current stream, no
    host synchronisation; to_host() is the one place that waits."""
    _CREATE, _DESTROY = "nbdt_clip_create", "nbdt_clip_destroy"

    def __init__(self, n, device=None):
        super().__init__(n, None, device)

    def _check(self, what, g):
        _C.require_gpu(g, what)
        if g.dtype != torch.float32 or g.numel() != self.n or not g.is_contiguous():
            raise _C.NBDTHipError(f"{what}: g must be a contiguous fp32 tensor of {self.n} elements, got {g.dtype} x {g.numel()}")
        if self.device is not None and g.device != self.device:
            raise _C.NBDTHipError(f"{what}: g is on {g.device}, the plan on {self.device}")

    def norm(self, g, grad_scale, max_norm):
        """The record after this call holds norm = |grad_scale| * ||g||_2 and coef = min(1, max_norm / (norm + 1e-6))."""
        self._check("clip_norm", g)
        check(lib().nbdt_clip_norm(self.handle, ptr(g), grad_scale, max_norm, stream_ptr(g.device)))

    def apply(self, g):
        """g *= coef of the record when that is below 1; nothing is read or written otherwise."""
        self._check("clip_apply", g)
        check(lib().nbdt_clip_apply(self.handle, ptr(g), stream_ptr(g.device)))

    def record(self):
        """The device record as an int32[8] tensor view (norm and coef are its first two words, as fp32 bits); owned by the
        plan, valid while it lives.  Reading it in a kernel on the issuing stream costs no synchronisation."""
        addr = lib().nbdt_clip_record(self.handle)
        if not addr:
            raise _C.NBDTHipError("clip_record: no plan")
        iface = {"shape": (8,), "typestr": "<i4", "data": (int(addr), False), "version": 2, "strides": None}
        holder = type("_ClipRecordView", (), {"__cuda_array_interface__": iface})()
        return torch.as_tensor(holder, device=self.device)

    def to_host(self):
        """{norm, coef, clipped, steps, nonfinite, total_clipped} as the last norm() left them.  Synchronises."""
        out = ClipRecord()
        with torch.cuda.device(self.device):
            check(lib().nbdt_clip_record_to_host(self.handle, ctypes.byref(out), stream_ptr(self.device)))
        return {k: getattr(out, k) for k, _ in ClipRecord._fields_[:6]}


def _ema_pair(p, ema, what):
    _C.require_gpu(p, what)
    _check_fp32(what, p.numel(), p, ((p, "p"), (ema, "ema")))


def ema_update(p, ema, one_minus_decay):
    """ema += one_minus_decay * (p - ema) as a subtract, a multiply and an add per element (nbdt_ema_update): one launch on
    p's current stream, p only read."""
    _ema_pair(p, ema, "ema_update")
    check(lib().nbdt_ema_update(ptr(p), ptr(ema), p.numel(), one_minus_decay, stream_ptr(p.device)))


def ema_swap(p, ema, p_bf16=None):
    """p and ema exchange their values in place; p_bf16 (optional) becomes the bf16 mirror of the new p (nbdt_ema_swap)."""
    _ema_pair(p, ema, "ema_swap")
    _check_mirror("ema_swap", p.numel(), p, p_bf16)
    check(lib().nbdt_ema_swap(ptr(p), ptr(ema), ptr(p_bf16), p.numel(), stream_ptr(p.device)))


class EmaTable:
    """The device table of nbdt_ema_update_multi / nbdt_ema_swap_multi: `pairs` = (live, shadow) fp32 tensors of equal
    length, a positive multiple of 32 elements each (the BatchNorm running statistics and their views of one flat shadow).
    The rows are checked here, on the host (the library sees only a device pointer), and copied to `device` once; the
    table keeps the tensors alive, whose addresses it holds."""

    def __init__(self, pairs, device):
        self.pairs = [(a, b) for a, b in pairs]
        self.device = torch.device(device)
        rows = []
        for live, shadow in self.pairs:
            for t in (live, shadow):
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != live.device:
                    raise _C.NBDTHipError("EmaTable: rows are pairs of contiguous fp32 tensors on one device")
                if t.data_ptr() % 16:
                    raise _C.NBDTHipError("EmaTable: tensors must be 16-byte aligned")
            n = live.numel()
            if shadow.numel() != n or n <= 0 or n % 32:
                raise _C.NBDTHipError(f"EmaTable: row lengths must be equal positive multiples of 32, got {n} / {shadow.numel()}")
            if live.data_ptr() == shadow.data_ptr():
                raise _C.NBDTHipError("EmaTable: a tensor cannot be its own shadow")
            rows.append([live.data_ptr(), shadow.data_ptr(), n])
        self.n_rows = len(rows)
        if not rows:
            raise _C.NBDTHipError("EmaTable: empty table")
        self.table = torch.tensor(rows, dtype=torch.int64).to(self.device)

    def update(self, one_minus_decay):
        _C.require_gpu(self.table, "EmaTable.update")
        check(lib().nbdt_ema_update_multi(ptr(self.table), self.n_rows, one_minus_decay, stream_ptr(self.device)))

    def swap(self):
        _C.require_gpu(self.table, "EmaTable.swap")
        check(lib().nbdt_ema_swap_multi(ptr(self.table), self.n_rows, stream_ptr(self.device)))


# ------------------------------------------------------------------------------------------------
# MBConv pieces (EfficientNet-B0, csrc/effnet.hip)

ACT_NONE, ACT_RELU, ACT_SWISH = 0, 1, 2


def bn_act_apply(x, mean, rstd, gamma, beta, y, act=ACT_SWISH, gate=None, residual=None, row_scale=None):
    """row_scale (fp32 [B], device; stochastic depth): y = residual + row_scale[b] * act(bn(x)) through
    nbdt_bn_act_apply_rows, which needs a residual and refuses a gate.  None: the call made without it."""
    B, H, W, C = _dims(x)
    if row_scale is not None:
        _check_rows(row_scale, B, x.device)
        fn = lib().nbdt_ref_bn_act_apply_rows if _ref(x) else lib().nbdt_bn_act_apply_rows
        check(fn(ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), act, ptr(gate), ptr(residual), ptr(row_scale), B, H,
                 W, C, ptr(y), stream_ptr(x.device)))
        return
    if _ref(x):
        check(lib().nbdt_ref_bn_act_apply(ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), act, ptr(gate),
                                          ptr(residual), B, H, W, C, ptr(y), stream_ptr(x.device)))
        return
    check(lib().nbdt_bn_act_apply(ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), act, ptr(gate),
                                  ptr(residual), B, H, W, C, ptr(y), stream_ptr(x.device)))


def bn_act_pool(x, mean, rstd, gamma, beta, out, act=ACT_SWISH, mul=None, scale=None):
    B, H, W, C = _dims(x)
    scale = 1.0 / (H * W) if scale is None else scale
    if _ref(x):
        check(lib().nbdt_ref_bn_act_pool(ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), act, ptr(mul), scale,
                                         B, H, W, C, ptr(out), stream_ptr(x.device)))
        return
    check(lib().nbdt_bn_act_pool(ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), act, ptr(mul), scale,
                                 B, H, W, C, ptr(out), stream_ptr(x.device)))


def bn_act_bwd(gu, x, mean, rstd, gamma, beta, scratch, dsum, dgamma, dbeta, gx, act=ACT_SWISH, gate=None,
               gpool=None, gx_add=None, row_scale=None):
    """row_scale (fp32 [B], device; stochastic depth): the gradient entering the activation is gu * row_scale[b], through
    nbdt_bn_act_bwd_rows -- the plain form only (gu given, no gate, no gpool).  None: the call made without it."""
    B, H, W, C = _dims(x)
    if row_scale is not None:
        _check_rows(row_scale, B, x.device)
        head = (ptr(gu), ptr(row_scale), ptr(gate), ptr(gpool), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), act,
                ptr(gx_add), B, H, W, C)
        tail = (ptr(dsum), ptr(dgamma), ptr(dbeta), ptr(gx), stream_ptr(x.device))
        if _ref(x):
            check(lib().nbdt_ref_bn_act_bwd_rows(*head, *tail))
        else:
            check(lib().nbdt_bn_act_bwd_rows(*head, ptr(scratch), *tail))
        return
    if _ref(x):
        check(lib().nbdt_ref_bn_act_bwd(ptr(gu), ptr(gate), ptr(gpool), ptr(x), ptr(mean), ptr(rstd), ptr(gamma),
                                        ptr(beta), act, ptr(gx_add), B, H, W, C, ptr(dsum), ptr(dgamma), ptr(dbeta),
                                        ptr(gx), stream_ptr(x.device)))
        return
    check(lib().nbdt_bn_act_bwd(ptr(gu), ptr(gate), ptr(gpool), ptr(x), ptr(mean), ptr(rstd), ptr(gamma),
                                ptr(beta), act, ptr(gx_add), B, H, W, C, ptr(scratch), ptr(dsum), ptr(dgamma),
                                ptr(dbeta), ptr(gx), stream_ptr(x.device)))


def _check_rows(row_scale, B, device):
    if not (row_scale.is_cuda and row_scale.device == device and row_scale.dtype == torch.float32 and
            row_scale.is_contiguous() and tuple(row_scale.shape) == (B,)):
        raise _C.NBDTHipError(f"row_scale must be a contiguous fp32 [{B}] tensor on {device}, got {row_scale.dtype} "
                              f"{tuple(row_scale.shape)} on {row_scale.device}")


def stochastic_depth_probs(P, n_units, residual_flags):
    """The host tables of nbdt_stochastic_depth_draw for torchvision's linear rule: unit i of n_units (0-based over ALL
    units) drops with p_i = P * i / n_units where residual_flags[i], never elsewhere.  Returns (prob, scale), numpy fp32
    [n_units]: prob = float32(p_i) is what the kernel compares its uniform with, scale = float32(1 / (1 - prob)), formed in
    double from that fp32 prob and rounded once; (0, 1) for a unit without a skip."""
    P = float(P)
    if not 0.0 <= P < 1.0:
        raise ValueError(f"the stochastic depth probability must be in [0, 1), got {P}")
    flags = [bool(f) for f in residual_flags]
    if len(flags) != int(n_units) or not 0 < len(flags) <= _C.NBDT_SD_MAX_UNITS:
        raise ValueError(f"residual_flags must name each of the {n_units} units (at most {_C.NBDT_SD_MAX_UNITS})")
    prob = np.asarray([P * i / len(flags) if f else 0.0 for i, f in enumerate(flags)], dtype=np.float64).astype(np.float32)
    scale = (1.0 / (1.0 - prob.astype(np.float64))).astype(np.float32)
    return prob, scale


def _sd_host(v, what):
    a = np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
    if a.dtype != np.float32 or a.ndim != 1:
        raise ValueError(f"{what} must be a one-dimensional fp32 host table, got {a.dtype} {a.shape}")
    return a


def stochastic_depth_draw(table, prob, scale, seed, stream, counter):
    """nbdt_stochastic_depth_draw: ONE launch writes table [U, B] fp32 (device) = 0 where image b of unit i is dropped,
    scale[i] where it is kept.  prob / scale: the host tables of stochastic_depth_probs; `stream` is the draw's stream
    id (a rank), not a HIP stream."""
    prob, scale = _sd_host(prob, "prob"), _sd_host(scale, "scale")
    _C.require_gpu(table, "stochastic_depth_draw")
    U, B = table.shape
    if table.dtype != torch.float32 or not table.is_contiguous() or prob.shape != (U,) or scale.shape != (U,):
        raise _C.NBDTHipError(f"stochastic_depth_draw: table must be contiguous fp32 [U, B] with prob / scale of length U, "
                              f"got {table.dtype} {tuple(table.shape)}, prob {prob.shape}, scale {scale.shape}")
    mask = (1 << 64) - 1
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    check(lib().nbdt_stochastic_depth_draw(int(seed) & mask, int(stream) & mask, int(counter) & mask, fp(prob), fp(scale),
                                           U, B, ptr(table), stream_ptr(table.device)))


def _mix64(x):      # splitmix64's finaliser (csrc/effnet.hip, csrc/policy_ops.h mix64); nbdt/data.py's draws use this one
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def draw_stochastic_depth(seed, stream, counter, prob, scale, B):
    """The generator of nbdt_stochastic_depth_draw (include/nbdt_hip.h), restated with numpy: the fp32 [U, B] table, bit
    for bit.  A pure function of (seed, stream, counter, unit, image)."""
    prob, scale = _sd_host(prob, "prob"), _sd_host(scale, "scale")
    U = prob.shape[0]
    u64 = np.uint64
    golden, k = 0x9E3779B97F4A7C15, u64(0xD1342543DE82EF95)
    with np.errstate(over="ignore"):
        key = _mix64(np.asarray([(int(seed) * golden + int(counter)) & _M64], dtype=u64))
        key = _mix64(key ^ (u64(int(stream) & _M64) * k))[0]
        elem = (np.arange(U, dtype=u64)[:, None] << u64(32)) | np.arange(int(B), dtype=u64)[None, :]
        r = _mix64(key ^ (elem * k))
    u = (r >> u64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.where(u < prob[:, None], np.float32(0.0), scale[:, None]).astype(np.float32)


def dwconv_fwd(x, w, y, k, stride, bn_scratch=None, pad=None):
    """bn_scratch: the 32-slot BN scratch; the kernel adds sum(y), sum(y^2) (fold with bn_stats(None, ...)).
    pad: None = padding k // 2 on extents the stride divides; (top, left) = the low-side padding of nbdt_dwconv_fwd_pad
    (conv_padding), any extents, y holding conv_out_size rows and columns."""
    B, H, W, C = _dims(x)
    if pad is not None:
        _check_out((H, W), y, stride)
        if _ref(x):
            check(lib().nbdt_ref_dwconv_fwd_pad(ptr(x), ptr(w), B, H, W, C, k, stride, int(pad[0]), int(pad[1]), ptr(y),
                                                stream_ptr(x.device)))
            return
        check(lib().nbdt_dwconv_fwd_pad(ptr(x), ptr(w), B, H, W, C, k, stride, int(pad[0]), int(pad[1]), ptr(y),
                                        ptr(bn_scratch), stream_ptr(x.device)))
        return
    if _ref(x):    # (no statistics from the fp32 twin: bn_stats re-reads the tensor in reference mode)
        check(lib().nbdt_ref_dwconv_fwd(ptr(x), ptr(w), B, H, W, C, k, stride, ptr(y), stream_ptr(x.device)))
        return
    check(lib().nbdt_dwconv_fwd(ptr(x), ptr(w), B, H, W, C, k, stride, ptr(y), ptr(bn_scratch),
                                stream_ptr(x.device)))


def dwconv_bwd_data(gy, w, gx, k, stride, pad=None):
    B, H, W, C = _dims(gx)
    if pad is not None:
        _check_out((H, W), gy, stride)
        fn = lib().nbdt_ref_dwconv_bwd_data_pad if _ref(gx) else lib().nbdt_dwconv_bwd_data_pad
        check(fn(ptr(gy), ptr(w), B, H, W, C, k, stride, int(pad[0]), int(pad[1]), ptr(gx), stream_ptr(gx.device)))
        return
    if _ref(gx):
        check(lib().nbdt_ref_dwconv_bwd_data(ptr(gy), ptr(w), B, H, W, C, k, stride, ptr(gx), stream_ptr(gx.device)))
        return
    check(lib().nbdt_dwconv_bwd_data(ptr(gy), ptr(w), B, H, W, C, k, stride, ptr(gx), stream_ptr(gx.device)))


def dwconv_bwd_data_bn(gy, w, gx, k, bn_x, mean, rstd, gamma, beta, scratch):
    """Stride-1 depthwise data gradient + the backward sums of the BatchNorm + swish that produced its input (into the
    32-slot scratch); follow with bn_act_bwd_apply."""
    B, H, W, C = _dims(gx)
    if _ref(gx):   # the plain data gradient; the sums are recomputed by bn_act_bwd_apply's reference form
        check(lib().nbdt_ref_dwconv_bwd_data(ptr(gy), ptr(w), B, H, W, C, k, 1, ptr(gx), stream_ptr(gx.device)))
        return
    check(lib().nbdt_dwconv_bwd_data_bn(ptr(gy), ptr(w), B, H, W, C, k, ptr(gx), ptr(bn_x), ptr(mean), ptr(rstd),
                                        ptr(gamma), ptr(beta), ptr(scratch), stream_ptr(gx.device)))


def bn_act_bwd_apply(gu, x, mean, rstd, gamma, beta, scratch, dsum, dgamma, dbeta, gx, act=ACT_SWISH, gx_add=None):
    """bn_act_bwd without its reduction pass (the producing kernel filled the slots)."""
    B, H, W, C = _dims(x)
    if _ref(x):    # reference mode: sums + elementwise pass (dwconv_bwd_data_bn's twin left no sums)
        check(lib().nbdt_ref_bn_act_bwd(ptr(gu), None, None, ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), act,
                                        ptr(gx_add), B, H, W, C, ptr(dsum), ptr(dgamma), ptr(dbeta), ptr(gx),
                                        stream_ptr(x.device)))
        return
    check(lib().nbdt_bn_act_bwd_apply(ptr(gu), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), act, ptr(gx_add),
                                      B, H, W, C, ptr(scratch), ptr(dsum), ptr(dgamma), ptr(dbeta), ptr(gx),
                                      stream_ptr(x.device)))


def bn_act_se_sums(gu, x, mean, rstd, gamma, beta, sums, act=ACT_SWISH):
    """One pass over (gu, x): sums[5][B][C] = dL/dgate and the four per-(image, channel) sums the BatchNorm backward of the
    SE-scaled activation is linear in (include/nbdt_hip.h: nbdt_bn_act_se_sums).  bf16 production path only."""
    B, H, W, C = _dims(x)
    check(lib().nbdt_bn_act_se_sums(ptr(gu), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), act, B, H, W, C,
                                    ptr(sums), stream_ptr(x.device)))


def bn_act_se_bwd_apply(gu, gate, gpool, sums, x, mean, rstd, gamma, beta, dsum, dgamma, dbeta, gx, act=ACT_SWISH):
    """Fold bn_act_se_sums' sums with gate / gpool into the BatchNorm-backward sums, then bn_act_bwd's elementwise pass."""
    B, H, W, C = _dims(x)
    check(lib().nbdt_bn_act_se_bwd_apply(ptr(gu), ptr(gate), ptr(gpool), ptr(sums), ptr(x), ptr(mean), ptr(rstd),
                                         ptr(gamma), ptr(beta), act, B, H, W, C, ptr(dsum), ptr(dgamma), ptr(dbeta),
                                         ptr(gx), stream_ptr(x.device)))


def dwconv_bwd_weight(x, gy, dw, k, stride, pad=None):
    B, H, W, C = _dims(x)
    if pad is not None:
        _check_out((H, W), gy, stride)
        fn = lib().nbdt_ref_dwconv_bwd_weight_pad if _ref(x) else lib().nbdt_dwconv_bwd_weight_pad
        check(fn(ptr(x), ptr(gy), B, H, W, C, k, stride, int(pad[0]), int(pad[1]), ptr(dw), stream_ptr(x.device)))
        return
    if _ref(x):
        check(lib().nbdt_ref_dwconv_bwd_weight(ptr(x), ptr(gy), B, H, W, C, k, stride, ptr(dw), stream_ptr(x.device)))
        return
    check(lib().nbdt_dwconv_bwd_weight(ptr(x), ptr(gy), B, H, W, C, k, stride, ptr(dw), stream_ptr(x.device)))


def se_gate_fwd(pooled, w1, b1, w2, b2, pre1, gate, c_real):
    B, C = pooled.shape
    check(lib().nbdt_se_gate_fwd(ptr(pooled), ptr(w1), ptr(b1), ptr(w2), ptr(b2), B, C, c_real, w1.shape[0],
                                 ptr(pre1), ptr(gate), stream_ptr(pooled.device)))


def se_gate_bwd(dgate, gate, pre1, pooled, w1, w2, dpre2, dpre1, gpool, dw1, db1, dw2, db2, c_real):
    """dw1 = db1 = dw2 = db2 = None: the data part only (follow with se_param_grad, on any stream ordered after this)."""
    B, C = pooled.shape
    check(lib().nbdt_se_gate_bwd(ptr(dgate), ptr(gate), ptr(pre1), ptr(pooled), ptr(w1), ptr(w2), B, C, c_real,
                                 w1.shape[0], ptr(dpre2), ptr(dpre1), ptr(gpool), ptr(dw1), ptr(db1), ptr(dw2),
                                 ptr(db2), stream_ptr(pooled.device)))


def se_param_grad(dpre2, dpre1, pre1, pooled, dw1, db1, dw2, db2, c_real):
    B, C = pooled.shape
    check(lib().nbdt_se_param_grad(ptr(dpre2), ptr(dpre1), ptr(pre1), ptr(pooled), B, C, c_real, dw1.shape[0],
                                   ptr(dw1), ptr(db1), ptr(dw2), ptr(db2), stream_ptr(pooled.device)))


def dropout_fwd(x, p, seed, mask, y):
    check(lib().nbdt_dropout_fwd(ptr(x), x.numel(), p, seed & 0xffffffff, ptr(mask), ptr(y), stream_ptr(x.device)))


def dropout_bwd(gy, p, mask, gx):
    check(lib().nbdt_dropout_bwd(ptr(gy), gy.numel(), p, ptr(mask), ptr(gx), stream_ptr(gy.device)))


# ------------------------------------------------------------------------------------------------
# slice-list convolutions (csrc/conv_seg.hip): the shape-changing units' convs as sums of stride-1 tap-subset convs

class ConvSeg:
    """A plan of nbdt_conv_seg_*: `classes` = [{"slices": [(tensor, ch0, [halo taps 3R+S], w_matrix, [w_off per tap])],
    "out": (bs, hs, ws, base)}], over input tensors [B][gh+2][gw+2][pix_strides[i]] and weight matrices
    [cout][w_row_strides[j]].  Host-side object; the device tables appear at the first launch."""

    def __init__(self, B, gh, gw, cout, pix_strides, w_row_strides, classes, tile=0, nbuf=0, flops=None):
        d = _C.ConvSegDesc()
        d.B, d.gh, d.gw, d.cout = B, gh, gw, cout
        d.ntensors, d.nmatrices, d.nclasses = len(pix_strides), len(w_row_strides), len(classes)
        _fill(d.pix_stride, pix_strides)
        _fill(d.w_row_stride, w_row_strides)
        d.tile, d.nbuf = tile, nbuf
        self._keep = []
        for c, k in enumerate(classes):
            arr = (_C.ConvSegSlice * len(k["slices"]))()
            for s, (tensor, ch0, taps, wm, woffs) in enumerate(k["slices"]):
                arr[s].tensor, arr[s].ch0, arr[s].ntaps, arr[s].w_matrix = tensor, ch0, len(taps), wm
                _fill(arr[s].tap, taps)
                _fill(arr[s].w_off, woffs)
            self._keep.append(arr)
            d.cls[c].nslices = len(k["slices"])
            d.cls[c].slices = ctypes.cast(arr, ctypes.POINTER(_C.ConvSegSlice))
            d.cls[c].out_bs, d.cls[c].out_hs, d.cls[c].out_ws, d.cls[c].out_base = k["out"]
        self.desc, self.classes = d, classes
        self.handle = ctypes.c_void_p()
        check(lib().nbdt_conv_seg_create(ctypes.byref(d), ctypes.byref(self.handle)))
        tile_, nbuf_, rounds = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        steps = (ctypes.c_int32 * 4)()
        wel = ctypes.c_int64()
        check(lib().nbdt_conv_seg_info(self.handle, ctypes.byref(tile_), ctypes.byref(nbuf_), steps, ctypes.byref(rounds),
                                       ctypes.byref(wel)))
        self.tile, self.nbuf, self.max_rounds, self.w_tile_elems = tile_.value, nbuf_.value, rounds.value, wel.value
        self.nsteps = list(steps)[:len(classes)]
        # algorithmic flops of a launch (the launch timers): 2 x pixels x cout x 32 per K step unless the caller knows better
        self.flops = float(flops) if flops is not None else 2.0 * B * gh * gw * cout * 32 * sum(self.nsteps)

    def steps(self, cls):
        """(records [n][8] int32, prologue slices) of class `cls` -- host copy, no device work."""
        import numpy as np
        n = self.nsteps[cls]
        buf = (ctypes.c_int32 * (8 * n))()
        npro = ctypes.c_int32()
        rc = lib().nbdt_conv_seg_steps(self.handle, cls, buf, n, ctypes.byref(npro))
        if rc < 0:
            check(rc)
        return np.frombuffer(buf, dtype=np.int32).reshape(n, 8).copy(), npro.value

    def tile_weights(self, ws, out=None):
        """ws: the bf16 weight matrices -> the DMA-ordered tile buffer the launches read."""
        dev = ws[0].device
        if out is None:
            out = torch.empty(self.w_tile_elems, dtype=torch.bfloat16, device=dev)
        arr = (ctypes.c_void_p * len(ws))(*[w.data_ptr() for w in ws])
        check(lib().nbdt_conv_seg_tile_weights(self.handle, arr, ptr(out), stream_ptr(dev)))
        return out

    def __call__(self, ins, w, out, residual=None, bn_scratch=None):
        """w: the tile buffer (bf16 path) or, for fp32 tensors (verification-only reference mode), the list of fp32
        weight matrices in their plain layout."""
        dev = ins[0].device
        arr = (ctypes.c_void_p * len(ins))(*[t.data_ptr() for t in ins])
        if _ref(ins[0]):
            warr = (ctypes.c_void_p * len(w))(*[t.data_ptr() for t in w])
            check(lib().nbdt_ref_conv_seg(self.handle, arr, warr, ptr(out), ptr(residual), stream_ptr(dev)))
            if bn_scratch is not None:
                B, H, W, C = _dims(out)
                check(lib().nbdt_ref_bn_stats(ptr(out), B, H, W, C, BN_EPS, BN_MOMENTUM, None, None, None, None,
                                              ptr(bn_scratch), stream_ptr(dev)))
            return
        ev = None
        if _timer is not None and _timer.wants("conv_igemm"):
            ev = _timer.bracket("conv_igemm", self.flops, dev)
            ev[0].record()
        check(lib().nbdt_conv_seg(self.handle, arr, ptr(w), ptr(out), ptr(residual), ptr(bn_scratch), stream_ptr(dev)))
        if ev is not None:
            ev[1].record()
            _timer.count(last_igemm_kernel_full())

    def __del__(self):
        try:
            h = getattr(self, "handle", None)
            if h is not None and h.value:
                lib().nbdt_conv_seg_destroy(h)
                self.handle = None
        except Exception:      # (interpreter shutdown: modules may already be gone)
            pass


def _plain_out(H, W, C):
    row = (W + 2) * C
    return ((H + 2) * row, row, C, row + C)


# 1-D phase tables of a stride-2 3x3 / pad-1 conv.  Forward over the space-to-depth input: phase p (row parity of the
# input) holds kernel rows r with halo row R (input row y + R - 1 of the half-resolution grid): out(y) reads
# in(2y + r - 1).  Data gradient: output parity p (of the unpadded input row) gets kernel rows r from gradient row u + R - 1.
S2_FWD = {0: [(1, 1)], 1: [(0, 0), (2, 1)]}
S2_BWD = {0: [(1, 1)], 1: [(0, 2), (2, 1)]}


def _interleave(major, minor):
    """`minor` slices spread evenly among `major` ones (never first: the first slice is every tile's prologue)."""
    if not minor:
        return list(major)
    out, j = [], 0
    for i, s in enumerate(major):
        out.append(s)
        while j < len(minor) and (j + 1) * len(major) <= (i + 1) * len(minor):
            out.append(minor[j])
            j += 1
    out.extend(minor[j:])
    return out


def seg_fwd_s2(B, Hi, Wi, cin, cout, tile=0, nbuf=0, order=(3, 0, 1, 2)):
    """Conv2d(3x3, stride 2, pad 1) forward over the space-to-depth copy [B][Hi/2+2][Wi/2+2][4 cin] of its input
    (bn_apply_s2d); weight matrix 0 = the forward weights [cout][9][cin].  order: phases (2 p + q) per 32-channel chunk."""
    Ho, Wo = Hi // 2, Wi // 2
    slices = []
    for kc in range(cin // 32):
        for ph in order:
            p, q = ph >> 1, ph & 1
            taps = [(3 * R + S, 3 * r + s) for (r, R) in S2_FWD[p] for (s, S) in S2_FWD[q]]
            slices.append((0, ph * cin + kc * 32, [t for t, _ in taps], 0, [w * cin + kc * 32 for _, w in taps]))
    return ConvSeg(B, Ho, Wo, cout, [4 * cin], [9 * cin], [{"slices": slices, "out": _plain_out(Ho, Wo, cout)}],
                   tile=tile, nbuf=nbuf, flops=2.0 * B * Ho * Wo * 9 * cin * cout)


def seg_conv3x3_plus_1x1(B, H, W, cin, cout, cin_sc, sc_pix_stride, tile=0, nbuf=0):
    """conv3x3(stride 1)(x) + conv1x1(s): tensor 0 = x [..][cin], tensor 1 = s with `sc_pix_stride` channels per pixel of
    which the first cin_sc are the shortcut's input (the plain tensor, or phase (0,0) of a space-to-depth copy: a 1x1
    stride-2 conv); matrices: [cout][9][cin], [cout][cin_sc]."""
    major = [(0, kc * 32, list(range(9)), 0, [t * cin + kc * 32 for t in range(9)]) for kc in range(cin // 32)]
    minor = [(1, kc * 32, [4], 1, [kc * 32]) for kc in range(cin_sc // 32)]
    return ConvSeg(B, H, W, cout, [cin, sc_pix_stride], [9 * cin, cin_sc],
                   [{"slices": _interleave(major, minor), "out": _plain_out(H, W, cout)}], tile=tile, nbuf=nbuf,
                   flops=2.0 * B * H * W * cout * (9 * cin + cin_sc))


def seg_dgrad_s2(B, Hi, Wi, cin, cout, shortcut=False, tile=0, nbuf=0):
    """Data gradient of Conv2d(cin -> cout, 3x3, stride 2, pad 1) [+ of the 1x1 stride-2 shortcut next to it]: tensor 0 =
    dL/d(conv output) [B][Hi/2+2][Wi/2+2][cout] (tensor 1 = dL/d(shortcut output), same shape); output dL/d(input)
    [B][Hi+2][Wi+2][cin], every interior pixel written once (four parity classes); matrices: the transposed tap-reversed
    copy wd [cin][9][cout] (weight_prep), and the shortcut's [cin][cout]."""
    Ho, Wo = Hi // 2, Wi // 2
    rowx = (Wi + 2) * cin
    classes = []
    for ph in (1, 0):
        for pw in (1, 0):
            taps = [(3 * R + S, 8 - (3 * r + s)) for (r, R) in S2_BWD[ph] for (s, S) in S2_BWD[pw]]
            major = [(0, kc * 32, [t for t, _ in taps], 0, [w * cout + kc * 32 for _, w in taps])
                     for kc in range(cout // 32)]
            minor = [(1, kc * 32, [4], 1, [kc * 32]) for kc in range(cout // 32)] if (shortcut and ph == 0 and pw == 0) else []
            classes.append({"slices": _interleave(major, minor),
                            "out": ((Hi + 2) * rowx, 2 * rowx, 2 * cin, (ph + 1) * rowx + (pw + 1) * cin)})
    return ConvSeg(B, Ho, Wo, cin, [cout, cout] if shortcut else [cout], [9 * cout, cout] if shortcut else [9 * cout],
                   classes, tile=tile, nbuf=nbuf, flops=2.0 * B * Ho * Wo * cin * cout * (9 + (1 if shortcut else 0)))


def seg_dgrad3x3_plus_1x1(B, H, W, cin, cout, tile=0, nbuf=0):
    """Data gradient of conv3x3(cin -> cout, stride 1) plus that of the 1x1 shortcut beside it (stride 1): tensors
    dL/d(conv output), dL/d(shortcut output) [B][H+2][W+2][cout]; matrices wd [cin][9][cout], wd_sc [cin][cout]."""
    major = [(0, kc * 32, list(range(9)), 0, [t * cout + kc * 32 for t in range(9)]) for kc in range(cout // 32)]
    minor = [(1, kc * 32, [4], 1, [kc * 32]) for kc in range(cout // 32)]
    return ConvSeg(B, H, W, cin, [cout, cout], [9 * cout, cout],
                   [{"slices": _interleave(major, minor), "out": _plain_out(H, W, cin)}], tile=tile, nbuf=nbuf,
                   flops=2.0 * B * H * W * cin * cout * 10)


def bn_apply_s2d(x, mean, rstd, gamma, beta, y, relu=True):
    """y = [relu](bn(x)) as the space-to-depth copy [B][H/2+2][W/2+2][4C] (nbdt_bn_apply_s2d)."""
    B, H, W, C = _dims(x)
    fn = lib().nbdt_ref_bn_apply_s2d if _ref(x) else lib().nbdt_bn_apply_s2d
    check(fn(ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), 1 if relu else 0, B, H, W, C, ptr(y),
             stream_ptr(x.device)))


def s2d_buffer(B, H, W, C, device, dtype=torch.bfloat16):
    """Zero-initialised space-to-depth activation buffer [B][H/2+2][W/2+2][4C] for an [H, W, C] tensor."""
    return torch.zeros((B, H // 2 + 2, W // 2 + 2, 4 * C), dtype=dtype, device=device)


def conv_wgrad_desc_s2d(B, Hi, Wi, cin, cout, k):
    """Weight gradient of Conv2d(k in {1,3}, stride 2, pad k//2) when its input is stored as the space-to-depth copy
    [B][Hi/2+2][Wi/2+2][4 cin] (bn_apply_s2d): tap (r, s) reads phase (r != 1, s != 1) at half-resolution pixel
    (y + (r == 0 ? -1 : 0), x + ...) -- every tap a unit-stride pixel walk of 4 cin-element pixels."""
    Ho, Wo = Hi // 2, Wi // 2
    d = WgradDesc()
    d.B, d.gh, d.gw, d.cin, d.cout = B, Ho, Wo, cin, cout
    row2 = (Wo + 2) * 4 * cin
    if k == 3:
        d.ntaps = d.w_ntaps = 9
        offs = []
        for r in range(3):
            for s in range(3):
                p, q = int(r != 1), int(s != 1)
                dy, dx = (-1 if r == 0 else 0), (-1 if s == 0 else 0)
                offs.append((1 + dy) * row2 + (1 + dx) * 4 * cin + (2 * p + q) * cin)
        _fill(d.tap_off, offs)
        _fill(d.w_tap, range(9))
        d.x_base = 0
    else:
        d.ntaps = d.w_ntaps = 1
        d.tap_off[0] = 0
        d.w_tap[0] = 0
        d.x_base = row2 + 4 * cin
    d.x_bs, d.x_hs, d.x_ws = (Ho + 2) * row2, row2, 4 * cin
    rowo = (Wo + 2) * cout
    d.g_bs, d.g_hs, d.g_ws, d.g_base = (Ho + 2) * rowo, rowo, cout, rowo + cout
    return d


def conv_fwd_desc_s2d_1x1(B, Hi, Wi, cin, cout):
    """Conv2d(1x1, stride 2) forward over the space-to-depth copy of its input: phase (0, 0), unit-stride pixels."""
    Ho, Wo = Hi // 2, Wi // 2
    d = ConvDesc()
    d.B, d.gh, d.gw, d.cin, d.cout = B, Ho, Wo, cin, cout
    row2 = (Wo + 2) * 4 * cin
    d.ntaps = d.w_ntaps = 1
    d.tap_off[0] = 0
    d.w_tap[0] = 0
    d.in_bs, d.in_hs, d.in_ws, d.in_base = (Ho + 2) * row2, row2, 4 * cin, row2 + 4 * cin
    rowo = (Wo + 2) * cout
    d.out_bs, d.out_hs, d.out_ws, d.out_base = (Ho + 2) * rowo, rowo, cout, rowo + cout
    d.accumulate = 0
    d.wide_tile = 1
    return d
