"""Every tensor entry point refuses a tensor AT its documented 32-bit offset limit with NBDT_EINVAL and a message that
names the quantity -- before any HIP call, so it can be shown on a box without a GPU, with pointers that lead nowhere --
and the table of tests/_offset_limit_cases.py is consistent in plain Python integers.

The calls take dummy pointers.  They must never reach a device: the module skips itself where one is present (there
tests/test_offset_limits_gpu.py runs the shapes just below the limits for real)."""
import ctypes

import pytest

from nbdt import _C, ops

import _offset_limit_cases as L

NBDT_EINVAL, NBDT_EHIP = -1, -2

if _C.lib().nbdt_device_count() > 0:
    pytest.skip("a GPU is present: these calls hand dummy pointers to the entry points and must never reach a device "
                "(the refusals are host code; they are tested on a box without a GPU)", allow_module_level=True)

_HOST = ctypes.create_string_buffer(4096 + 16)
_BASE = (ctypes.addressof(_HOST) + 15) & ~15


def P(i=0):
    """A non-null, 16-byte-aligned pointer (distinct per i); never dereferenced by a call that is refused."""
    return ctypes.c_void_p(_BASE + 256 * i)


N = None


def _err():
    return _C.lib().nbdt_last_error().decode()


def _bhwc_call(entry, B, H, W, C):
    lib = _C.lib()
    calls = {
        "nbdt_bn_stats": lambda: lib.nbdt_bn_stats(P(), B, H, W, C, 1e-5, 0.1, N, N, P(1), P(2), P(3), N),
        "nbdt_bn_apply": lambda: lib.nbdt_bn_apply(P(), P(1), P(2), P(3), P(4), N, 1, B, H, W, C, P(5), N),
        "nbdt_bn_bwd_reduce": lambda: lib.nbdt_bn_bwd_reduce(P(), N, P(1), P(2), P(3), P(4), P(5), 1, B, H, W, C, P(6), P(7),
                                                             N, N, N),
        "nbdt_bn_bwd_apply": lambda: lib.nbdt_bn_bwd_apply(P(), N, P(1), P(2), P(3), P(4), P(5), P(6), N, 1, B, H, W, C,
                                                           P(7), N, N),
        "nbdt_bn_relu_pool": lambda: lib.nbdt_bn_relu_pool(P(), P(1), P(2), P(3), P(4), B, H, W, C, P(5), N),
        "nbdt_bn_act_apply": lambda: lib.nbdt_bn_act_apply(P(), P(1), P(2), P(3), P(4), 2, N, N, B, H, W, C, P(5), N),
        "nbdt_bn_act_pool": lambda: lib.nbdt_bn_act_pool(P(), P(1), P(2), P(3), P(4), 2, N, 1.0, B, H, W, C, P(5), N),
        "nbdt_bn_act_bwd": lambda: lib.nbdt_bn_act_bwd(P(), N, N, P(1), P(2), P(3), P(4), P(5), 2, N, B, H, W, C, P(6), P(7),
                                                       P(8), P(9), P(10), N),
        "nbdt_dwconv_fwd": lambda: lib.nbdt_dwconv_fwd(P(), P(1), B, H, W, C, 3, 1, P(2), N, N),
        "nbdt_dwconv_bwd_data": lambda: lib.nbdt_dwconv_bwd_data(P(), P(1), B, H, W, C, 5, 2, P(2), N),
        "nbdt_dwconv_bwd_weight": lambda: lib.nbdt_dwconv_bwd_weight(P(), P(1), B, H, W, C, 3, 2, P(2), N),
    }
    return calls[entry]()


def _call(entry, kind, shape):
    """One call of `entry` on `shape` with dummy operands: the return code (the message is in nbdt_last_error)."""
    lib = _C.lib()
    if kind.startswith("conv_"):
        descs = L.conv_descs(kind, shape)
        d = ctypes.byref(descs[0])
        if entry == "nbdt_conv_plan":
            form, ks = ctypes.c_int32(-7), ctypes.c_int32(-7)
            return lib.nbdt_conv_plan(d, ctypes.byref(form), ctypes.byref(ks))
        if entry == "nbdt_conv_igemm":
            return lib.nbdt_conv_igemm(d, P(), P(1), P(2), N, N)
        if entry == "nbdt_conv_igemm_stats":
            return lib.nbdt_conv_igemm_stats(d, P(), P(1), P(2), N, P(3), N)
        if entry == "nbdt_conv_igemm_affine":
            return lib.nbdt_conv_igemm_affine(d, P(), P(1), P(2), N, P(3), P(4), 1, N)
        if entry == "nbdt_conv_igemm_bnbwd":
            return lib.nbdt_conv_igemm_bnbwd(d, P(), P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8), N)
        if entry == "nbdt_conv_igemm_multi":
            arr = (_C.ConvDesc * len(descs))(*descs)
            return lib.nbdt_conv_igemm_multi(arr, len(descs), P(), P(1), P(2), N)
        if entry == "nbdt_conv_pw":
            return lib.nbdt_conv_pw(d, P(), P(1), P(2), N, N)
    if kind in ("wgrad_x", "wgrad_g", "wgrad_w"):
        return lib.nbdt_conv_wgrad(ctypes.byref(ops.conv_wgrad_desc(*shape)), P(), P(1), P(2), N)
    if kind in ("seg_fwd_s2", "seg_fwd_s2_in"):
        try:                    # (ops.ConvSeg builds the slice tables and raises "libnbdt_hip error <rc>: <message>")
            ops.seg_fwd_s2(*shape)
        except _C.NBDTHipError as e:
            return int(str(e).split("error ")[1].split(":")[0])
        return 0
    if kind == "bhwc":
        return _bhwc_call(entry, *shape)
    if kind == "s2d":
        B, H, W, C = shape
        return lib.nbdt_bn_apply_s2d(P(), P(1), P(2), P(3), P(4), 1, B, H, W, C, P(5), N)
    if kind == "stem":
        B, H, W = shape
        return lib.nbdt_stem_wgrad(P(), P(1), B, H, W, 16, 32, 1, P(2), N)
    if kind == "stem_grid":
        B, H, W = shape
        return lib.nbdt_stem_conv(P(), P(1), B, H, W, 16, 32, 1, P(2), N)
    if kind == "stem_pad":
        B, H, W = shape
        if entry == "nbdt_stem_conv_pad":
            return lib.nbdt_stem_conv_pad(P(), P(1), B, H, W, 16, 32, 1, 1, 1, P(2), N)
        return lib.nbdt_stem_wgrad_pad(P(), P(1), B, H, W, 16, 32, 1, 1, 1, P(2), N)
    if kind == "group":
        B, H, W, width = shape
        if entry == "nbdt_conv_group_fwd":
            return lib.nbdt_conv_group_fwd(P(), P(1), P(2), B, H, W, width, 8, 1, N, N, 0, N)
        if entry == "nbdt_conv_group_dgrad":
            return lib.nbdt_conv_group_dgrad(P(), P(1), P(2), B, H, W, width, 8, 1, 0, N)
        if entry == "nbdt_conv_group_wgrad":
            return lib.nbdt_conv_group_wgrad(P(), P(1), P(2), B, H, W, width, 8, 1, N)
    raise KeyError((entry, kind))


AT = [(r[0], e) for r in L.ROWS for e in r[1]]


@pytest.mark.parametrize("rid,entry", AT, ids=["%s-%s" % a for a in AT])
def test_at_the_limit_is_refused_before_any_hip_call(rid, entry):
    _, _, kind, at, _, quantity, _ = L.row(rid)
    rc = _call(entry, kind, at)
    msg = _err()
    print(f"{entry} at {at}: rc {rc}, '{msg}'")
    assert rc == NBDT_EINVAL and rc != NBDT_EHIP, (rc, msg)
    assert quantity in msg, msg


HOST_ONLY = [(r[0], e) for r in L.ROWS for e in r[1] if e in ("nbdt_conv_plan", "nbdt_conv_seg_create")]


@pytest.mark.parametrize("rid,entry", HOST_ONLY, ids=["%s-%s" % a for a in HOST_ONLY])
def test_just_below_the_limit_is_accepted_by_the_host_only_entries(rid, entry):
    """nbdt_conv_plan and nbdt_conv_seg_create do no device work: the BELOW shape passes every check."""
    _, _, kind, _, below, _, _ = L.row(rid)
    assert _call(entry, kind, below) == 0, _err()


def test_plan_names_the_kernels_the_gpu_cases_take():
    """The 32x32 cases take the 8-wave halo kernel on 512-pixel tiles (with DMA-ordered weights) -- the input one with
    4 294 623 232 bytes of input, 344 064 short of where the halo kernels' byte offsets end --, the 30x30 and 1x1 ones
    conv_igemm_dma: the kernels tests/test_offset_limits_gpu.py asserts by name."""
    for rid, form in (("conv_out_3x3_halo", 2), ("conv_in_3x3_halo", 2), ("conv_out_3x3", 0), ("conv_in_3x3", 0),
                      ("conv_out_1x1", 0)):
        d = L.conv_descs("conv_fwd", L.row(rid)[4])[0]
        d.w_tiled = 16            # any non-null value: nbdt_conv_plan only asks whether tiles are there
        assert ops.conv_plan(d)[0] == form, rid


@pytest.mark.parametrize("r", L.ROWS, ids=[r[0] for r in L.ROWS])
def test_table_arithmetic(r):
    rid, _, kind, at, below, quantity, limit = r
    hi, lo = L.largest_offset(kind, at, quantity), L.largest_offset(kind, below, quantity)
    assert lo < limit <= hi, (rid, lo, limit, hi)
    assert at[0] - below[0] == 1 or kind in ("conv_weights", "wgrad_w")           # the smallest step: one image


@pytest.mark.parametrize("case", L.GPU_CASES, ids=[c[0] for c in L.GPU_CASES])
def test_gpu_case_footprints(case):
    cid, rid, tensors = case
    assert L.footprint(case) <= L.FOOTPRINT_MAX, (cid, L.footprint(case) / L.GIB)
    if rid is None:           # a 64-bit path: its first tensor passes 2^32 bytes
        assert tensors[0][1] * tensors[0][2] > (1 << 32), cid
        return
    _, _, kind, _, below, quantity, limit = L.row(rid)
    # the case's first tensor is the one at the limit: within one image of it, and it crosses 2^31 BYTES half way
    name, n, size = tensors[0]
    assert limit - 34 * 34 * 256 <= n < limit and n * size > (1 << 31), (cid, name, n)
