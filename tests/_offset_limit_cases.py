"""Shapes at and just below the 32-bit offset limits of the tensor entry points ("Size limits of the tensor
entry points"): one table for tests/test_offset_limits.py (host: every AT shape is refused with NBDT_EINVAL before any
HIP call, and the table's own arithmetic holds in Python integers) and tests/test_offset_limits_gpu.py (GPU: the BELOW
shape computes the right answer inside a guarded arena).

A row is  (id, entries, kind, at, below, quantity, limit):
  entries    C-ABI symbols that share the guard
  kind       how `at` / `below` are read (see largest_offset and the callers in the two test modules)
  quantity   what nbdt_last_error() must name
  limit      the documented bound: largest_offset(at) >= limit > largest_offset(below)

Every limit here is 2^31 ELEMENTS of a signed 32-bit element offset unless the row says otherwise.  The smallest step
below is one image fewer (the alignment rules of the descriptors do not bind at these shapes); the images are 30x30, which
pad to 32x32, so that a 256-channel image is exactly 2^18 elements and 8192 of them are exactly 2^31."""
from nbdt import ops

LIMIT = 1 << 31
GIB = 1 << 30
FRONT_MARGIN, BACK_MARGIN = 4 * GIB, 64 << 20        # around every arena of the GPU tests
FOOTPRINT_MAX = 16 * GIB

S = 30                       # image side: (S + 2)^2 = 1024 padded pixels
B_AT, B_BELOW = 8192, 8191   # 8192 * 1024 * 256 = 2^31
WIDE, NARROW = 256, 32
HALO_AT, HALO_BELOW = 7257, 7256   # 32x32 images (34x34 padded) of 256 channels

# (B, Hi, Wi, cin, cout, k, stride): forward descriptors unless the kind says otherwise
_F = lambda B, cin, cout, k=3, stride=1, side=S: (B, side, side, cin, cout, k, stride)      # noqa: E731

ROWS = [
    # ---- nbdt_conv_igemm family (csrc/conv.hip: check_desc)
    ("conv_out_3x3", ("nbdt_conv_igemm", "nbdt_conv_igemm_stats", "nbdt_conv_igemm_affine", "nbdt_conv_igemm_bnbwd",
                      "nbdt_conv_plan"), "conv_fwd", _F(B_AT, NARROW, WIDE), _F(B_BELOW, NARROW, WIDE),
     "output elements", LIMIT),
    ("conv_out_1x1", ("nbdt_conv_igemm", "nbdt_conv_plan"), "conv_fwd", _F(B_AT, NARROW, WIDE, 1), _F(B_BELOW, NARROW, WIDE, 1),
     "output elements", LIMIT),
    ("conv_in_3x3", ("nbdt_conv_igemm", "nbdt_conv_plan"), "conv_fwd", _F(B_AT, WIDE, NARROW), _F(B_BELOW, WIDE, NARROW),
     "input elements", LIMIT),
    # (no LDS-resident halo tile fits a 30-wide image -- tiles are whole rows or whole images -- so the 30x30 rows take
    #  conv_igemm_dma; the halo kernels get 32x32 images: 34 * 34 * 256 = 295936 elements per padded image, 7257 of them
    #  pass 2^31, and 7256 of them as an INPUT are 4 294 623 232 bytes: just inside the kernels' 32-bit byte lane offsets)
    ("conv_out_3x3_halo", ("nbdt_conv_igemm", "nbdt_conv_plan"), "conv_fwd", _F(HALO_AT, NARROW, WIDE, side=32),
     _F(HALO_BELOW, NARROW, WIDE, side=32), "output elements", LIMIT),
    ("conv_in_3x3_halo", ("nbdt_conv_igemm", "nbdt_conv_plan"), "conv_fwd", _F(HALO_AT, WIDE, NARROW, side=32),
     _F(HALO_BELOW, WIDE, NARROW, side=32), "input elements", LIMIT),
    ("conv_dgrad_accumulate", ("nbdt_conv_igemm",), "conv_dgrad_acc", _F(B_AT, WIDE, NARROW), _F(B_BELOW, WIDE, NARROW),
     "output elements", LIMIT),
    ("conv_dgrad_strided_multi", ("nbdt_conv_igemm_multi",), "conv_dgrad_multi", _F(B_AT, WIDE, NARROW, 3, 2),
     _F(B_BELOW, WIDE, NARROW, 3, 2), "output elements", LIMIT),
    ("conv_weights", ("nbdt_conv_igemm", "nbdt_conv_plan"), "conv_weights", (2, 2, 2, 15456, 15456, 3, 1),
     (2, 2, 2, 15456, 15424, 3, 1), "weight elements", LIMIT),
    # ---- nbdt_conv_wgrad (csrc/wgrad.hip)
    ("wgrad_x_3x3", ("nbdt_conv_wgrad",), "wgrad_x", _F(B_AT, WIDE, NARROW), _F(B_BELOW, WIDE, NARROW), "input elements", LIMIT),
    # (the all-nine-taps kernels stage 32 or 64 pixels of a row: 30-wide images take conv_wgrad_dma_kernel, 32-wide ones
    #  the 8-wave kernel, whose 32-bit byte lane offsets 7256 images of 34 x 34 x 256 just fit)
    ("wgrad_x_3x3_taps", ("nbdt_conv_wgrad",), "wgrad_x", _F(HALO_AT, WIDE, NARROW, side=32), _F(HALO_BELOW, WIDE, NARROW, side=32),
     "input elements", LIMIT),
    ("wgrad_gy_3x3", ("nbdt_conv_wgrad",), "wgrad_g", _F(B_AT, NARROW, WIDE), _F(B_BELOW, NARROW, WIDE),
     "output-gradient elements", LIMIT),
    ("wgrad_x_1x1", ("nbdt_conv_wgrad",), "wgrad_x", _F(B_AT, WIDE, NARROW, 1), _F(B_BELOW, WIDE, NARROW, 1),
     "input elements", LIMIT),
    ("wgrad_gy_strided", ("nbdt_conv_wgrad",), "wgrad_g", _F(B_AT, NARROW, WIDE, 3, 2, 2 * S), _F(B_BELOW, NARROW, WIDE, 3, 2, 2 * S),
     "output-gradient elements", LIMIT),
    ("wgrad_weights", ("nbdt_conv_wgrad",), "wgrad_w", (2, 2, 2, 15456, 15456, 3, 1), (2, 2, 2, 15456, 15424, 3, 1),
     "weight-gradient elements", LIMIT),
    # ---- nbdt_conv_pw (csrc/conv_pw.hip)
    ("conv_pw_out", ("nbdt_conv_pw",), "conv_fwd", _F(B_AT, NARROW, WIDE, 1), _F(B_BELOW, NARROW, WIDE, 1), "output elements", LIMIT),
    ("conv_pw_in", ("nbdt_conv_pw",), "conv_fwd", _F(B_AT, WIDE, NARROW, 1), _F(B_BELOW, WIDE, NARROW, 1), "input elements", LIMIT),
    # ---- nbdt_conv_seg_create (csrc/conv_seg.hip): the stride-2 forward over the space-to-depth input
    # (its tiles are whole rows of the output grid: 32x32 outputs, 34 * 34 * 256 = 295936 elements per padded image)
    ("conv_seg_out", ("nbdt_conv_seg_create",), "seg_fwd_s2", (7257, 64, 64, NARROW, WIDE), (7256, 64, 64, NARROW, WIDE),
     "output elements", LIMIT),
    # (input BYTES of the space-to-depth copy: 34 * 34 * 512 * 2 = 1 183 744 per image, unsigned 32-bit byte lane offsets)
    ("conv_seg_in", ("nbdt_conv_seg_create",), "seg_fwd_s2_in", (3629, 64, 64, 128, NARROW), (3628, 64, 64, 128, NARROW),
     "input tensor beyond 32-bit byte offsets", 1 << 32),
    # ---- padded NHWC streaming kernels (csrc/bn_sums.h: check_shape / check_shape_wide)
    ("bn_tensor", ("nbdt_bn_stats", "nbdt_bn_apply", "nbdt_bn_bwd_reduce", "nbdt_bn_bwd_apply", "nbdt_bn_relu_pool",
                   "nbdt_bn_act_apply", "nbdt_bn_act_pool", "nbdt_bn_act_bwd", "nbdt_dwconv_fwd", "nbdt_dwconv_bwd_data",
                   "nbdt_dwconv_bwd_weight"), "bhwc", (B_AT, S, S, WIDE), (B_BELOW, S, S, WIDE), "padded tensor elements", LIMIT),
    ("bn_s2d_out", ("nbdt_bn_apply_s2d",), "s2d", (29128, 2, 2, 2048), (29127, 2, 2, 2048),
     "space-to-depth output elements", LIMIT),
    # (the GPU case: 30x30x256 images, whose copy [B][17][17][1024] has 295936 elements per image where the input has 2^18)
    ("bn_s2d_out_30", ("nbdt_bn_apply_s2d",), "s2d", (HALO_AT, S, S, WIDE), (HALO_BELOW, S, S, WIDE),
     "space-to-depth output elements", LIMIT),
    # ---- nbdt_stem_wgrad (csrc/misc.hip): a 32-bit PIXEL index that overshoots by up to 64 * (tiles per block + 1)
    ("stem_wgrad_pixels", ("nbdt_stem_wgrad",), "stem", (2093056, 32, 32), (2093055, 32, 32), "output pixels",
     LIMIT - (1 << 22)),
    # ---- nbdt_stem_conv: 64-bit addresses, one block per 256 output pixels and at most 2^31 - 1 blocks
    ("stem_conv_grid", ("nbdt_stem_conv",), "stem_grid", (1 << 21, 512, 512), ((1 << 21) - 1, 512, 512), "output pixels",
     256 * (LIMIT - 1) + 1),
    # ---- the asymmetric-padding stem entries: check_stem_pad's own, stricter bound
    ("stem_pad_pixels", ("nbdt_stem_conv_pad", "nbdt_stem_wgrad_pad"), "stem_pad", (1 << 15, 32, 32), ((1 << 15) - 1, 32, 32),
     "image batch too large", 1 << 25),
    # ---- grouped conv (csrc/conv_group.hip): 64-bit addresses, a 32-bit index of PADDED pixels
    ("conv_group_pixels", ("nbdt_conv_group_fwd", "nbdt_conv_group_dgrad", "nbdt_conv_group_wgrad"), "group",
     (2 * 1024 * 1024, S, S, 32), (2 * 1024 * 1024 - 1, S, S, 32), "pixel grid", LIMIT),
]


def row(rid):
    return next(r for r in ROWS if r[0] == rid)


def conv_descs(kind, shape):
    """The nbdt_conv_desc list of a conv row (host only: ctypes structures)."""
    B, H, W, cin, cout, k, stride = shape
    if kind in ("conv_fwd", "conv_weights"):
        return [ops.conv_fwd_desc(B, H, W, cin, cout, k, stride)]
    if kind in ("conv_dgrad_acc", "conv_dgrad_multi"):
        return ops.conv_dgrad_descs(B, H, W, cin, cout, k, stride, accumulate=True)
    raise KeyError(kind)


def _conv_extents(d):
    taps = max([d.tap_off[t] for t in range(d.ntaps)] + [0])
    return {"output elements": d.B * d.out_bs + d.out_base, "input elements": d.B * d.in_bs + d.in_base + taps,
            "weight elements": d.cout * d.w_ntaps * d.cin}


def largest_offset(kind, shape, quantity):
    """The bound quantity of a row's shape in plain Python integers: what the guard compares with `limit`."""
    if kind.startswith("conv_"):
        return max(_conv_extents(d)[quantity] for d in conv_descs(kind, shape))
    if kind == "wgrad_w":
        d = ops.conv_wgrad_desc(*shape)
        return d.cout * d.w_ntaps * d.cin
    if kind == "seg_fwd_s2_in":
        B, H, W, cin, _ = shape
        return B * (H // 2 + 2) * (W // 2 + 2) * 4 * cin * 2
    if kind in ("wgrad_x", "wgrad_g"):
        d = ops.conv_wgrad_desc(*shape)
        taps = max([d.tap_off[t] for t in range(d.ntaps)] + [0])
        return d.B * d.x_bs + d.x_base + taps if kind == "wgrad_x" else d.B * d.g_bs + d.g_base
    if kind == "seg_fwd_s2":
        B, H, W, cin, cout = shape
        row_o = (W // 2 + 2) * cout
        return B * (H // 2 + 2) * row_o + row_o + cout
    if kind == "bhwc":
        B, H, W, C = shape
        return B * (H + 2) * (W + 2) * C
    if kind == "s2d":
        B, H, W, C = shape
        return B * (H // 2 + 2) * (W // 2 + 2) * 4 * C
    if kind in ("stem", "stem_grid", "stem_pad"):
        B, H, W = shape
        return B * H * W
    if kind == "group":
        B, H, W, _ = shape
        return B * (H + 2) * (W + 2)
    raise KeyError(kind)


# ------------------------------------------------------------------------------------------------------------------------
# GPU cases: (id, row id, the big tensors as (name, elements, bytes per element)) -- everything inside one arena of
# FRONT_MARGIN + tensors + BACK_MARGIN bytes.  A case's small operands (weights, per-channel vectors, sums) are not listed.

def _padded(B, C, side=S):
    return B * (side + 2) * (side + 2) * C


GPU_CASES = [
    ("conv_fwd_halo_residual_stats", "conv_out_3x3_halo", [("out", _padded(HALO_BELOW, WIDE, 32), 2),
                                                           ("res", _padded(HALO_BELOW, WIDE, 32), 2),
                                                           ("in", _padded(HALO_BELOW, NARROW, 32), 2)]),
    ("conv_fwd_halo_input", "conv_in_3x3_halo", [("in", _padded(HALO_BELOW, WIDE, 32), 2), ("out", _padded(HALO_BELOW, NARROW, 32), 2)]),
    ("conv_fwd_dma_3x3", "conv_out_3x3", [("out", _padded(B_BELOW, WIDE), 2), ("res", _padded(B_BELOW, WIDE), 2),
                                          ("in", _padded(B_BELOW, NARROW), 2)]),
    ("conv_fwd_dma_1x1", "conv_out_1x1", [("out", _padded(B_BELOW, WIDE), 2), ("in", _padded(B_BELOW, NARROW), 2)]),
    ("conv_fwd_dma_input", "conv_in_3x3", [("in", _padded(B_BELOW, WIDE), 2), ("out", _padded(B_BELOW, NARROW), 2)]),
    ("conv_dgrad_accumulate", "conv_dgrad_accumulate", [("gx", _padded(B_BELOW, WIDE), 2), ("gy", _padded(B_BELOW, NARROW), 2)]),
    ("wgrad_x_3x3_taps", "wgrad_x_3x3_taps", [("x", _padded(HALO_BELOW, WIDE, 32), 2), ("gy", _padded(HALO_BELOW, NARROW, 32), 2)]),
    ("wgrad_x_3x3", "wgrad_x_3x3", [("x", _padded(B_BELOW, WIDE), 2), ("gy", _padded(B_BELOW, NARROW), 2)]),
    ("wgrad_gy_1x1", "wgrad_gy_3x3", [("gy", _padded(B_BELOW, WIDE), 2), ("x", _padded(B_BELOW, NARROW), 2)]),
    ("conv_pw_fwd", "conv_pw_out", [("out", _padded(B_BELOW, WIDE), 2), ("in", _padded(B_BELOW, NARROW), 2)]),
    ("bn_stats_apply", "bn_tensor", [("y", _padded(B_BELOW, WIDE), 2), ("x", _padded(B_BELOW, WIDE), 2)]),
    ("bn_bwd_reduce", "bn_tensor", [("gy", _padded(B_BELOW, WIDE), 2), ("x", _padded(B_BELOW, WIDE), 2)]),
    ("bn_act_apply_pool", "bn_tensor", [("y", _padded(B_BELOW, WIDE), 2), ("x", _padded(B_BELOW, WIDE), 2)]),
    ("bn_act_bwd_pooled", "bn_tensor", [("gx", _padded(B_BELOW, WIDE), 2), ("x", _padded(B_BELOW, WIDE), 2)]),
    ("dwconv", "bn_tensor", [("y", _padded(B_BELOW, WIDE), 2), ("x", _padded(B_BELOW, WIDE), 2)]),
]


GPU_CASES += [
    ("conv_seg_fwd", "conv_seg_out", [("out", _padded(HALO_BELOW, WIDE, 32), 2), ("in", HALO_BELOW * 34 * 34 * 4 * NARROW, 2)]),
    ("bn_s2d", "bn_s2d_out_30", [("y", HALO_BELOW * 17 * 17 * 4 * WIDE, 2), ("x", _padded(HALO_BELOW, WIDE), 2)]),
]

# 64-bit paths ("none" in DESIGN.md's table): tensors past 2^32 bytes, no row above
DATA_N, DATA_SIDE = 350000, 64                   # uint8 [N, 3, 64, 64]: 4 300 800 000 bytes
MIX_B, MIX_SIDE = 87400, 64                      # fp32 [B, 3, 64, 64]: 4 295 884 800 bytes each way
GROUP_B = 8200                                   # bf16 [8200, 32, 32, 256]: 2 149 580 800 elements, past 2^31
DROPOUT_N = 1680000 * 1280                       # fp32 [1 680 000, 1280]: 2 150 400 000 elements, x and y ONE tensor
SEG_N, SEG_C, SEG_SIDE = 3496, 150, 64           # bf16 [3496, 150, 64, 64]: 2 147 942 400 elements
SEG_FIRST, SEG_EVERY = 7, 32                     # the view z[7::32]: 110 images, the last one image 3495
GPU_CASES += [
    ("conv_group", None, [("x", _padded(GROUP_B, WIDE), 2), ("y", _padded(GROUP_B, WIDE), 2)]),
    ("dropout", None, [("x", DROPOUT_N, 4), ("mask", DROPOUT_N, 1)]),
    ("seg_rules", None, [("z", SEG_N * SEG_C * SEG_SIDE * SEG_SIDE, 2)]),
    ("resident_dataset", None, [("src", DATA_N * 3 * DATA_SIDE * DATA_SIDE, 1)]),
    ("mix_batch", None, [("out", MIX_B * 3 * MIX_SIDE * MIX_SIDE, 4), ("x", MIX_B * 3 * MIX_SIDE * MIX_SIDE, 4)]),
]


def gpu_case(cid):
    return next(c for c in GPU_CASES if c[0] == cid)


def footprint(case):
    return FRONT_MARGIN + sum(-(-n * size // 256) * 256 for _, n, size in case[2]) + BACK_MARGIN
