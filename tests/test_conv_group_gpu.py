"""Per-op parity of the grouped 3x3 convolution (csrc/conv_group.hip) on the MI355X, over tests/_conv_group_cases.py:

  * the device weight expansion is the host restatement, bit for bit, single and batched;
  * integer inputs: forward and data gradient (bf16) and the weight gradient (fp32, onto a non-zero dw) equal
    F.conv2d(groups=) / conv2d_input / conv2d_weight on the CPU bit for bit; the ring of every output keeps a sentinel;
    two runs of each entry leave identical bits;
  * the same integer inputs through the dense entries (nbdt_conv_igemm, its data gradient, nbdt_conv_wgrad) with the dense
    block-diagonal [width][9][width] weight: equal bit for bit (the weight gradient on the diagonal sub-blocks);
  * random bf16-rounded inputs against fp32 F.conv2d with the per-op criteria of tests/test_conv_resnet_shapes_gpu.py
    (|a - b| <= 2^-7 max(|a|, |b|) + 1e-4; weight gradient rtol 2e-3, atol 2e-3 mean|ref|), the eval epilogue included;
  * the fp32-storage twins to the bounds tests/test_reference_fp32_gpu.py holds fp32 storage to (activations 1e-4 of the
    scale, weight gradients 1e-3 relative L2)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_group_cases as G  # noqa: E402
from _conv_group_cases import B, CASES  # noqa: E402

from nbdt import ops  # noqa: E402

DEV = "cuda:0"
SENTINEL = 1.5          # exactly representable in bf16
cases = pytest.mark.parametrize("case", CASES, ids=[G.case_id(c) for c in CASES])


def _padded(t_nchw, dtype=torch.bfloat16, halo=0.0):
    """Padded NHWC device buffer with interior t ([B,C,H,W] on the host) and `halo` in the ring."""
    b, c, h, w = t_nchw.shape
    p = torch.full((b, h + 2, w + 2, c), halo, dtype=dtype, device=DEV)
    ops.interior(p).copy_(t_nchw.permute(0, 2, 3, 1).to(dtype).to(DEV))
    return p


def _sentinel(b, h, w, c, dtype=torch.bfloat16):
    return torch.full((b, h + 2, w + 2, c), SENTINEL, dtype=dtype, device=DEV)


def _ring_untouched(p):
    ring = torch.ones(p.shape[:3], dtype=torch.bool, device=p.device)
    ring[:, 1:-1, 1:-1] = False
    return torch.equal(p[ring], torch.full_like(p[ring], SENTINEL))


def _nchw(p):
    return ops.interior(p).permute(0, 3, 1, 2)


def _bits_equal(got, ref):
    """A device tensor equals a CPU float32 reference whose values are numbers of the device tensor's type: same bits."""
    return torch.equal(got.cpu(), ref.to(got.dtype))


def _expanded(w_oihw):
    """(master on the device, wf, wd) of a [width, cg, 3, 3] weight."""
    master = G.master_of(w_oihw).float().to(DEV)
    width, _, cg = master.shape
    wf = torch.empty(width // 32, 32, 9, 32, dtype=torch.bfloat16, device=DEV)
    wd = torch.empty_like(wf)
    ops.conv_group_weight_prep(master, width, cg, wf, wd)
    return master, wf, wd


_DEVC = {}


def _dev(kind, case):
    """Device copies of a case's inputs (built once, never written)."""
    if (kind, case) not in _DEVC:
        c = G.integer_case(case) if kind == "int" else G.real_case(case)
        master, wf, wd = _expanded(c["w"])
        _DEVC[kind, case] = dict(c, xp=_padded(c["x"]), gp=_padded(c["gy"]), master=master, wf=wf, wd=wd)
    return _DEVC[kind, case]


# ------------------------------------------------------------------------------------------------------------------------
# weight expansion

@pytest.mark.parametrize("width,cg", G.CONFIGS)
def test_device_expansion_is_the_host_restatement(width, cg):
    g = torch.Generator().manual_seed(width + cg)
    master = torch.randn(width, 9, cg, generator=g)
    hf, hd = G.expand_host(master.numpy())
    wf = torch.full((width // 32, 32, 9, 32), SENTINEL, dtype=torch.bfloat16, device=DEV)
    wd = torch.full_like(wf, SENTINEL)
    ops.conv_group_weight_prep(master.to(DEV), width, cg, wf, wd)
    assert torch.equal(wf.cpu(), torch.from_numpy(hf).to(torch.bfloat16))       # (torch rounds to nearest even too)
    assert torch.equal(wd.cpu(), torch.from_numpy(hd).to(torch.bfloat16))
    only = torch.full_like(wf, SENTINEL)
    ops.conv_group_weight_prep(master.to(DEV), width, cg, None, only)
    assert torch.equal(only, wd)


def test_batched_expansion_equals_the_single_launches():
    g = torch.Generator().manual_seed(3)
    layers = [(64, 8), (128, 4), (32, 32), (96, 16)]
    masters = [torch.randn(w, 9, cg, generator=g) for w, cg in layers]
    pad = 8                                   # masters at aligned, non-adjacent offsets of a flat arena
    flat, rows, src, dst, first = [], [], 0, 0, 0
    for (w, cg), m in zip(layers, masters):
        flat += [m.flatten(), torch.full((pad,), float("nan"))]
        rows.append([src, dst, w, cg, first])
        src += m.numel() + pad
        dst += w * 9 * 32
        first += w // 32
    flat = torch.cat(flat).to(DEV)
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    wf = torch.full((dst,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    wd = torch.full_like(wf, SENTINEL)
    ops.conv_group_weight_prep_batched(flat, table, len(layers), first, wf, wd)
    for (w, cg), m, row in zip(layers, masters, rows):
        _, sf, sd = _expanded(m.view(w, 3, 3, cg).permute(0, 3, 1, 2))
        assert torch.equal(wf[row[1]:row[1] + sf.numel()], sf.flatten()), (w, cg)
        assert torch.equal(wd[row[1]:row[1] + sd.numel()], sd.flatten()), (w, cg)


# ------------------------------------------------------------------------------------------------------------------------
# integer inputs: bit for bit

@cases
def test_integer_forward_is_exact(case):
    width, cg, H, W, s = case
    c = _dev("int", case)
    outs = []
    for _ in range(2):
        out = _sentinel(B, H // s, W // s, width)
        ops.conv_group_fwd(c["xp"], c["wf"], out, cg, s)
        outs.append(out)
    assert _bits_equal(_nchw(outs[0]), c["fwd"]) and _ring_untouched(outs[0])
    assert torch.equal(outs[0], outs[1])


@cases
def test_integer_data_gradient_is_exact(case):
    width, cg, H, W, s = case
    c = _dev("int", case)
    outs = []
    for _ in range(2):
        gx = _sentinel(B, H, W, width)
        ops.conv_group_dgrad(c["gp"], c["wd"], gx, cg, s)
        outs.append(gx)
    assert _bits_equal(_nchw(outs[0]), c["gx"]) and _ring_untouched(outs[0])
    assert torch.equal(outs[0], outs[1])


@cases
def test_integer_weight_gradient_adds_onto_dw_exactly(case):
    width, cg, H, W, s = case
    c = _dev("int", case)
    outs = []
    for _ in range(2):
        dw = c["dw0"].clone().to(DEV)                 # non-zero on entry: the fold adds onto what .grad holds
        ops.conv_group_wgrad(c["xp"], c["gp"], dw, cg, s)
        outs.append(dw)
    assert _bits_equal(outs[0], c["dw"] + c["dw0"])
    assert torch.equal(outs[0], outs[1])
    ops.conv_group_wgrad(c["xp"], c["gp"], outs[1], cg, s)
    assert _bits_equal(outs[1], 2 * c["dw"] + c["dw0"])


def test_data_gradient_refuses_an_accumulate_request():
    c = _dev("int", CASES[0])
    width, cg, H, W, s = CASES[0]
    with pytest.raises(RuntimeError, match="no accumulate form"):
        ops.conv_group_dgrad(c["gp"], c["wd"], _sentinel(B, H, W, width), cg, s, accumulate=True)


# ------------------------------------------------------------------------------------------------------------------------
# the dense entries on the dense block-diagonal weight, on the device

@cases
def test_integer_results_equal_the_dense_entries_bit_for_bit(case):
    width, cg, H, W, s = case
    c = _dev("int", case)
    Ho, Wo = H // s, W // s
    dense = torch.from_numpy(G.dense_block_diagonal(G.master_of(c["w"]).numpy())).float().to(DEV)      # [width][9][width]
    wb = torch.empty(width, 9, width, dtype=torch.bfloat16, device=DEV)
    wdd = torch.empty_like(wb)
    ops.weight_prep(dense, width, 9, width, wb, wdd)
    args = (B, H, W, width, width, 3, s)
    ours, theirs = ops.padded(B, Ho, Wo, width, DEV), ops.padded(B, Ho, Wo, width, DEV)
    ops.conv_group_fwd(c["xp"], c["wf"], ours, cg, s)
    ops.conv_igemm(ops.conv_fwd_desc(*args), c["xp"], wb, theirs)
    assert torch.equal(ours, theirs)
    ours, theirs = ops.padded(B, H, W, width, DEV), ops.padded(B, H, W, width, DEV)
    ops.conv_group_dgrad(c["gp"], c["wd"], ours, cg, s)
    descs = ops.conv_dgrad_descs(*args, accumulate=False)
    if len(descs) > 1:
        ops.conv_igemm_multi(descs, c["gp"], wdd, theirs)
    else:
        ops.conv_igemm(descs[0], c["gp"], wdd, theirs)
    assert torch.equal(ours, theirs)
    dw = torch.zeros(width, 9, cg, device=DEV)
    dwd = torch.zeros(width, 9, width, device=DEV)
    ops.conv_group_wgrad(c["xp"], c["gp"], dw, cg, s)
    ops.conv_wgrad(ops.conv_wgrad_desc(*args), c["xp"], c["gp"], dwd)
    co = torch.arange(width, device=DEV)
    cols = (co // cg * cg)[:, None] + torch.arange(cg, device=DEV)[None, :]                       # [width][cg]
    diag = dwd.gather(2, cols[:, None, :].expand(width, 9, cg))
    assert torch.equal(dw, diag)


# ------------------------------------------------------------------------------------------------------------------------
# random bf16-rounded inputs against fp32 F.conv2d

def _close(got, ref, what):
    a, b = got.float().cpu(), ref.float()
    bad = (a - b).abs() > 2.0 ** -7 * torch.maximum(a.abs(), b.abs()) + 1e-4
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {(a - b).abs().max():.4g}"


@cases
def test_real_forward_and_eval_epilogue(case):
    width, cg, H, W, s = case
    c = _dev("real", case)
    out = _sentinel(B, H // s, W // s, width)
    ops.conv_group_fwd(c["xp"], c["wf"], out, cg, s)
    _close(_nchw(out), c["fwd"], "forward")
    assert _ring_untouched(out)
    g = torch.Generator().manual_seed(width + cg)
    scale, shift = torch.rand(width, generator=g) + 0.5, torch.randn(width, generator=g) * 0.3
    affine = c["fwd"] * scale[None, :, None, None] + shift[None, :, None, None]
    for act, fn in ((0, lambda t: t), (1, torch.relu), (2, lambda t: t * torch.sigmoid(t))):
        out = _sentinel(B, H // s, W // s, width)
        ops.conv_group_fwd(c["xp"], c["wf"], out, cg, s, scale.to(DEV), shift.to(DEV), act)
        _close(_nchw(out), fn(affine), f"eval epilogue, act {act}")
        assert _ring_untouched(out)


@cases
def test_real_data_gradient(case):
    width, cg, H, W, s = case
    c = _dev("real", case)
    gx = _sentinel(B, H, W, width)
    ops.conv_group_dgrad(c["gp"], c["wd"], gx, cg, s)
    _close(_nchw(gx), c["gx"], "data gradient")
    assert _ring_untouched(gx)


@cases
def test_real_weight_gradient(case):
    width, cg, H, W, s = case
    c = _dev("real", case)
    dw = torch.zeros(width, 9, cg, device=DEV)
    ops.conv_group_wgrad(c["xp"], c["gp"], dw, cg, s)
    ref = c["dw"].double().numpy()
    np.testing.assert_allclose(dw.cpu().double().numpy(), ref, rtol=2e-3, atol=2e-3 * np.abs(ref).mean())


# ------------------------------------------------------------------------------------------------------------------------
# the fp32-storage twins

@cases
def test_fp32_twins(case):
    width, cg, H, W, s = case
    c = G.real_case(case)
    g = torch.Generator().manual_seed(11)
    x, gy = torch.randn(c["x"].shape, generator=g), torch.randn(c["gy"].shape, generator=g)       # not bf16-rounded
    w = torch.randn(c["w"].shape, generator=g) / (9 * cg) ** 0.5
    fwd, gx, dw = G.refs(x, w, gy, s, width // cg, torch.float64)
    master = G.master_of(w).to(DEV)
    xp, gp = _padded(x, torch.float32), _padded(gy, torch.float32)
    out = _sentinel(B, H // s, W // s, width, torch.float32)
    ops.conv_group_fwd(xp, master, out, cg, s)
    assert (_nchw(out).double().cpu() - fwd).abs().max().item() < 1e-4 * fwd.abs().max().item() and _ring_untouched(out)
    gin = _sentinel(B, H, W, width, torch.float32)
    ops.conv_group_dgrad(gp, master, gin, cg, s)
    assert (_nchw(gin).double().cpu() - gx).abs().max().item() < 1e-4 * gx.abs().max().item() and _ring_untouched(gin)
    with pytest.raises(RuntimeError, match="no accumulate form"):
        ops.conv_group_dgrad(gp, master, gin, cg, s, accumulate=True)
    base = torch.randn(width, 9, cg, generator=g)
    got = base.clone().to(DEV)
    ops.conv_group_wgrad(xp, gp, got, cg, s)
    err = (got.double().cpu() - base.double() - dw).norm().item() / dw.norm().item()
    assert err < 1e-3, err
