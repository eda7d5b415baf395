// Cross-entropy on bilinearly upsampled logits, on gfx950: CE(up(x), y) and its gradient from the LOW-resolution tensor
// x [N, C, h, w] and the FULL-resolution labels y [N, H, W], for
//   F.cross_entropy(F.interpolate(x, size=(H, W), mode="bilinear", align_corners=ac), y, weight, ignore_index,
//                   reduction="mean", label_smoothing=eps)
// the criterion of segmentation backbones that emit logits at 1/4 of the label resolution (HRNet and its like).  No
// tensor of N*C*H*W elements is ever formed and there is no floating-point atomic: torch's composition materialises
// up(x), its log-softmax and both gradients at full resolution, and its bilinear backward scatters with atomics.
//
// Three launches, no host read-back:
//   upx_fwd_kernel   one lane per full-resolution pixel, a wave on 64 consecutive pixels of a row-major [H, W] plane (so
//                    neighbouring lanes share their low-resolution taps).  The classes are walked in ascending order,
//                    kUpU at a time with their 4 * kUpU loads in flight: v_c = up(x)[c] (up_lerp on four taps), once for
//                    the maximum and the target sum, once for the exponential sum.  The lane leaves lse and its label
//                    (-1: ignored) in an [N, H, W] workspace and adds its row loss and divisor term to per-wave
//                    partials by a fixed butterfly.
//   upx_fold_kernel  one block adds the partials in block order: loss = sum / divisor; the divisor stays in the
//                    workspace for the backward.  The same bits on every run.
//   upx_bwd_kernel   GATHER form: one lane per low-resolution pixel (i, j), kUpBwdC classes per block (grid.y walks the
//                    class chunks).  gx[n, c, i, j] = grad_scale / divisor * sum over the footprint (Y, X) of
//                    wy(Y, i) * wx(X, j) * f_c(Y, X), f_c = coef * exp(v_c - lse) - t'_c, ascending Y then ascending X,
//                    ignored pixels skipped.  Upsampling (H >= h, W >= w) means a pixel whose taps touch (i, j) reads
//                    only the 3 x 3 neighbourhood of (i, j): nine loads per class up front, then arithmetic.  v_c is
//                    recomputed by up_lerp on the same four taps in the same operand order as the forward, so
//                    exp(v - lse) is the forward's softmax.  Everything that does not depend on the class (taps,
//                    weights, lse, label) is worked out once per (Y, X) and shared by the chunk's classes.
//
// Criterion.  coef = weight[y] with class weights, 1 without (T = sum_c t'_c = 1);  t'_c = (1 - eps) * coef * 1[c == y] + eps / C
//   row = coef * lse - sum_c t'_c v_c;   divisor = sum of coef over the valid pixels (their count without weights)
// weight together with eps > 0 is refused (torch weighs the smoothing term per class; the Python layer composes it).  A
// label outside [0, C) that is not ignore_index gives a NaN loss; no valid pixel gives 0 / 0 = NaN and a zero gradient.
#include "common.h"
#include "upsample_taps.h"

#include <algorithm>

using namespace nbdt;

namespace {

struct LoadF32 { static __device__ __forceinline__ float at(const void* p, int64_t i) { return ((const float*)p)[i]; } };
struct LoadBF16 { static __device__ __forceinline__ float at(const void* p, int64_t i) { return bf16_to_f32(((const bf16_t*)p)[i]); } };
struct LoadF16 { static __device__ __forceinline__ float at(const void* p, int64_t i) { return __half2float(((const __half*)p)[i]); } };

constexpr int kUpLanes = 64;
constexpr int kUpU = 8;        // classes per load block of the forward: 4 * kUpU loads in flight per lane
constexpr int kUpBwdC = 4;     // classes per block of the backward: 9 * kUpBwdC neighbourhood values in registers
constexpr int kFoldBlock = 256;
constexpr int64_t kUpMaxExtent = 1 << 22;  // dst + 0.5f is exact and src keeps a fraction bit

struct UpGeom {
  int C, h, w, H, W, ac;
  float sy, sx;          // up_scale of the two axes
  int64_t hw, HW;        // pixels of a low- / full-resolution plane
  int64_t lchunks, chunks;  // blocks per image of the backward / the forward
  int64_t xi, xc;        // image and channel stride of x, in elements
};

// workspace: [0] divisor, [4 ..) loss partials, divisor partials (one each per forward block), lse [N*HW], label [N*HW]
struct UpWorkspace {
  float *hdr, *ploss, *pdiv, *lse;
  int* lab;
};

__host__ __device__ inline UpWorkspace carve(float* ws, int64_t nblk, int64_t npix) {
  UpWorkspace u;
  u.hdr = ws;
  u.ploss = ws + 4;
  u.pdiv = u.ploss + nblk;
  u.lse = u.pdiv + nblk;
  u.lab = (int*)(u.lse + npix);
  return u;
}

template <typename LD>
__global__ __launch_bounds__(kUpLanes) void upx_fwd_kernel(UpGeom g, const void* __restrict__ x,
                                                           const int64_t* __restrict__ y, int64_t ignore,
                                                           const float* __restrict__ wgt, float eps, UpWorkspace u) {
  const int lane = threadIdx.x;
  const int64_t blk = blockIdx.x;
  const int64_t img = blk / g.chunks;
  const int64_t pix = (blk - img * g.chunks) * kUpLanes + lane;
  const bool active = pix < g.HW;
  const int64_t pc = active ? pix : g.HW - 1;  // tail lanes read the last pixel
  const int64_t at = img * g.HW + pc;
  const int64_t yy = y[at];
  const bool valid = active && yy != ignore;
  if (__ballot(valid) == 0) {  // nothing to learn from these 64 pixels
    if (active) {
      u.lab[at] = -1;
      u.lse[at] = 0.f;
    }
    if (lane == 0) {
      u.ploss[blk] = 0.f;
      u.pdiv[blk] = 0.f;
    }
    return;
  }
  const int Y = (int)(pc / g.W), X = (int)(pc - (int64_t)Y * g.W);
  const UpTap ty = up_taps(g.h, g.sy, g.ac, Y), tx = up_taps(g.w, g.sx, g.ac, X);
  const int64_t base = img * g.xi;
  const int64_t o00 = base + (int64_t)ty.i0 * g.w + tx.i0, o01 = base + (int64_t)ty.i0 * g.w + tx.i1;
  const int64_t o10 = base + (int64_t)ty.i1 * g.w + tx.i0, o11 = base + (int64_t)ty.i1 * g.w + tx.i1;
  const bool inrange = yy >= 0 && yy < g.C;
  const float nanv = __uint_as_float(0x7fc00000u);
  const float coef = wgt ? (inrange ? wgt[inrange ? yy : 0] : nanv) : 1.f;
  const float uni = eps / (float)g.C, hit = (1.f - eps) * coef;

  float m = -INFINITY, tz = 0.f;
  for (int c0 = 0; c0 < g.C; c0 += kUpU) {
    float a[kUpU], b[kUpU], c[kUpU], d[kUpU];
#pragma unroll
    for (int k = 0; k < kUpU; ++k) {
      const int64_t oc = (int64_t)min(c0 + k, g.C - 1) * g.xc;
      a[k] = LD::at(x, o00 + oc);
      b[k] = LD::at(x, o01 + oc);
      c[k] = LD::at(x, o10 + oc);
      d[k] = LD::at(x, o11 + oc);
    }
#pragma unroll
    for (int k = 0; k < kUpU; ++k)
      if (c0 + k < g.C) {
        const float v = up_lerp(ty.l0, ty.l1, tx.l0, tx.l1, a[k], b[k], c[k], d[k]);
        const float ts = ((c0 + k == yy) ? hit : 0.f) + uni;
        m = fmaxf(m, v);
        tz += ts * v;
      }
  }
  float s = 0.f;
  for (int c0 = 0; c0 < g.C; c0 += kUpU) {
    float a[kUpU], b[kUpU], c[kUpU], d[kUpU];
#pragma unroll
    for (int k = 0; k < kUpU; ++k) {
      const int64_t oc = (int64_t)min(c0 + k, g.C - 1) * g.xc;
      a[k] = LD::at(x, o00 + oc);
      b[k] = LD::at(x, o01 + oc);
      c[k] = LD::at(x, o10 + oc);
      d[k] = LD::at(x, o11 + oc);
    }
#pragma unroll
    for (int k = 0; k < kUpU; ++k)
      if (c0 + k < g.C) s += expf(up_lerp(ty.l0, ty.l1, tx.l0, tx.l1, a[k], b[k], c[k], d[k]) - m);
  }
  const float lse = logf(s) + m;
  float row = 0.f, div = 0.f;
  if (valid) {
    row = inrange ? coef * lse - tz : nanv;  // loud: NaN loss
    div = inrange ? coef : 0.f;
  }
  if (active) {
    // a stray label keeps its pixel in the backward with a NaN lse: the gradient around it is NaN, as the loss is
    u.lab[at] = valid ? (inrange ? (int)yy : g.C) : -1;
    u.lse[at] = (valid && !inrange) ? nanv : lse;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    row += __shfl_xor(row, o, 64);
    div += __shfl_xor(div, o, 64);
  }
  if (lane == 0) {
    u.ploss[blk] = row;
    u.pdiv[blk] = div;
  }
}

// loss = (ploss[0] + ploss[1] + ...) / (pdiv[0] + pdiv[1] + ...): a thread adds its partials in ascending order, the
// threads are added in ascending order.  The divisor is summed in double: without class weights its terms are counts of
// at most 64, so the count is exact up to the entry's 2^31 pixels.  No valid pixel gives 0 / 0 = NaN, as torch's mean does.
__global__ __launch_bounds__(kFoldBlock) void upx_fold_kernel(UpWorkspace u, int64_t n, float* __restrict__ loss) {
  __shared__ float rl[kFoldBlock];
  __shared__ double rd[kFoldBlock];
  float acc = 0.f;
  double dv = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kFoldBlock) {
    acc = acc + u.ploss[i];
    dv = dv + (double)u.pdiv[i];
  }
  rl[threadIdx.x] = acc;
  rd[threadIdx.x] = dv;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    double d = 0.0;
    for (int i = 0; i < kFoldBlock; ++i) {
      tot = tot + rl[i];
      d = d + rd[i];
    }
    const float divisor = (float)d;
    u.hdr[0] = divisor;
    loss[0] = tot / divisor;
  }
}

template <typename LD>
__global__ __launch_bounds__(kUpLanes) void upx_bwd_kernel(UpGeom g, const void* __restrict__ x,
                                                           const float* __restrict__ wgt, float eps, float grad_scale,
                                                           UpWorkspace u, float* __restrict__ gx) {
  const int lane = threadIdx.x;
  const int64_t blk = blockIdx.x;
  const int64_t img = blk / g.lchunks;
  const int64_t p = (blk - img * g.lchunks) * kUpLanes + lane;
  const bool active = p < g.hw;
  const int64_t pc = active ? p : g.hw - 1;
  const int i = (int)(pc / g.w), j = (int)(pc - (int64_t)i * g.w);
  const int c0 = blockIdx.y * kUpBwdC;

  // the 3 x 3 neighbourhood of (i, j) for each class of the chunk; a clamped row / column is never selected below
  const int r[3] = {max(i - 1, 0), i, min(i + 1, g.h - 1)}, q[3] = {max(j - 1, 0), j, min(j + 1, g.w - 1)};
  float nb[kUpBwdC][3][3];
#pragma unroll
  for (int k = 0; k < kUpBwdC; ++k) {
    const int64_t oc = img * g.xi + (int64_t)min(c0 + k, g.C - 1) * g.xc;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) nb[k][a][b] = LD::at(x, oc + (int64_t)r[a] * g.w + q[b]);
  }
  int ylo, yhi, xlo, xhi;
  up_footprint(g.h, g.H, g.sy, g.ac, i, &ylo, &yhi);
  up_footprint(g.w, g.W, g.sx, g.ac, j, &xlo, &xhi);
  const float uni = eps / (float)g.C;
  const float nanv = __uint_as_float(0x7fc00000u);
  float acc[kUpBwdC];
#pragma unroll
  for (int k = 0; k < kUpBwdC; ++k) acc[k] = 0.f;

  for (int Y = ylo; Y <= yhi; ++Y) {
    const UpTap ty = up_taps(g.h, g.sy, g.ac, Y);
    const float wy = up_weight(ty, i);
    if (wy == 0.f) continue;  // from here on i0 is i - 1 or i, and i1 is i0 or i0 + 1
    const int ry0 = ty.i0 - (i - 1), ry1 = ty.i1 - (i - 1);
    float top[kUpBwdC][3], bot[kUpBwdC][3];
#pragma unroll
    for (int k = 0; k < kUpBwdC; ++k)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        top[k][b] = ry0 == 0 ? nb[k][0][b] : nb[k][1][b];
        bot[k][b] = ry1 == 0 ? nb[k][0][b] : (ry1 == 1 ? nb[k][1][b] : nb[k][2][b]);
      }
    const int64_t rowat = img * g.HW + (int64_t)Y * g.W;
    for (int X = xlo; X <= xhi; ++X) {
      const UpTap tx = up_taps(g.w, g.sx, g.ac, X);
      const float wx = up_weight(tx, j);
      if (wx == 0.f) continue;
      const int lab = u.lab[rowat + X];
      if (lab < 0) continue;  // ignored
      const float lse = u.lse[rowat + X];
      const float coef = wgt ? (lab < g.C ? wgt[lab < g.C ? lab : 0] : nanv) : 1.f;
      const float hit = (1.f - eps) * coef;
      const float ww = wy * wx;
      const int cx0 = tx.i0 - (j - 1), cx1 = tx.i1 - (j - 1);
#pragma unroll
      for (int k = 0; k < kUpBwdC; ++k) {
        const float a = cx0 == 0 ? top[k][0] : top[k][1];
        const float b = cx1 == 0 ? top[k][0] : (cx1 == 1 ? top[k][1] : top[k][2]);
        const float c = cx0 == 0 ? bot[k][0] : bot[k][1];
        const float d = cx1 == 0 ? bot[k][0] : (cx1 == 1 ? bot[k][1] : bot[k][2]);
        const float v = up_lerp(ty.l0, ty.l1, tx.l0, tx.l1, a, b, c, d);
        const float f = coef * expf(v - lse) - (((c0 + k == lab) ? hit : 0.f) + uni);
        acc[k] = acc[k] + ww * f;
      }
    }
  }
  const float divisor = u.hdr[0];
  const float scale = divisor > 0.f ? grad_scale / divisor : 0.f;  // no valid pixel: a zero gradient
  if (active) {
    float* G = gx + (img * g.C + c0) * g.hw + p;
#pragma unroll
    for (int k = 0; k < kUpBwdC; ++k)
      if (c0 + k < g.C) G[(int64_t)k * g.hw] = acc[k] * scale;
  }
}

int64_t fwd_blocks(int64_t N, int64_t H, int64_t W) { return N * ((H * W + kUpLanes - 1) / kUpLanes); }

}  // namespace

extern "C" int nbdt_upsample_taps(int in, int out, int align_corners, int dst, int* i0, int* i1, float* l0, float* l1) {
  NBDT_REQUIRE(i0 && i1 && l0 && l1, "null output");
  NBDT_REQUIRE(in >= 1 && out >= 1 && dst >= 0 && dst < out, "bad axis sizes / destination index");
  NBDT_REQUIRE(in <= kUpMaxExtent && out <= kUpMaxExtent, "axis longer than 2^22 samples");
  const UpTap t = up_taps(in, up_scale(in, out, align_corners != 0), align_corners != 0, dst);
  *i0 = t.i0; *i1 = t.i1; *l0 = t.l0; *l1 = t.l1;
  return NBDT_OK;
}

extern "C" int nbdt_upsample_footprint(int in, int out, int align_corners, int i, int* lo, int* hi) {
  NBDT_REQUIRE(lo && hi, "null output");
  NBDT_REQUIRE(in >= 1 && out >= in && i >= 0 && i < in, "bad axis sizes / source index (out >= in: upsampling only)");
  NBDT_REQUIRE(in <= kUpMaxExtent && out <= kUpMaxExtent, "axis longer than 2^22 samples");
  up_footprint(in, out, up_scale(in, out, align_corners != 0), align_corners != 0, i, lo, hi);
  return NBDT_OK;
}

extern "C" int64_t nbdt_upsampled_xent_workspace_floats(int64_t N, int64_t H, int64_t W) {
  if (N <= 0 || H <= 0 || W <= 0 || H > kUpMaxExtent || W > kUpMaxExtent || N > ((1ll << 31) - 1) / (H * W)) return 4;
  return 4 + 2 * fwd_blocks(N, H, W) + 2 * N * H * W;
}

extern "C" int nbdt_upsampled_xent(const void* x, int xtype, int64_t N, int64_t C, int64_t h, int64_t w, int64_t xi,
                                   int64_t xc, const int64_t* y, int64_t H, int64_t W, int align_corners,
                                   int64_t ignore_index, const float* weight, float smoothing, float grad_scale,
                                   float* workspace, float* loss, float* gx, void* stream) {
  NBDT_REQUIRE(x && y && workspace && loss && gx, "null buffer");
  NBDT_REQUIRE((const void*)gx != x && (const void*)gx != (const void*)y && gx != workspace && gx != loss &&
                   (const void*)workspace != x && (const void*)workspace != (const void*)y && workspace != loss &&
                   (const void*)loss != x && (const void*)loss != (const void*)y && (const void*)x != (const void*)y,
               "aliased buffers");
  NBDT_REQUIRE(weight == nullptr || ((const void*)weight != (const void*)gx && weight != workspace && weight != loss),
               "class weights alias an output");
  NBDT_REQUIRE(xtype == NBDT_F32 || xtype == NBDT_BF16 || xtype == NBDT_F16, "unsupported logits dtype");
  NBDT_REQUIRE(N > 0 && C > 0 && h > 0 && w > 0, "empty tensor has no mean loss");
  NBDT_REQUIRE(H >= h && W >= w, "downsampling: the backward's 3 x 3 neighbourhood holds for H >= h and W >= w only");
  NBDT_REQUIRE(H <= kUpMaxExtent && W <= kUpMaxExtent, "H and W must stay within 2^22 (the source index is fp32)");
  NBDT_REQUIRE(N <= ((1ll << 31) - 1) / (H * W), "pixels: N * H * W must stay below 2^31");
  NBDT_REQUIRE(C <= (int64_t)kUpBwdC * 65535, "more than 262,140 classes (the backward walks them in grid.y)");
  NBDT_REQUIRE(xc >= h * w && xi >= (C - 1) * xc + h * w, "bad channel / image stride (planes must not overlap)");
  NBDT_REQUIRE(smoothing >= 0.f && smoothing < 1.f, "label smoothing must be in [0, 1)");
  NBDT_REQUIRE(weight == nullptr || smoothing == 0.f, "class weights together with label smoothing are not fused");
  NBDT_REQUIRE(grad_scale == grad_scale, "grad_scale is NaN");

  UpGeom g;
  g.C = (int)C; g.h = (int)h; g.w = (int)w; g.H = (int)H; g.W = (int)W; g.ac = align_corners != 0;
  g.sy = up_scale(g.h, g.H, g.ac);
  g.sx = up_scale(g.w, g.W, g.ac);
  g.hw = h * w; g.HW = H * W;
  g.lchunks = (g.hw + kUpLanes - 1) / kUpLanes;
  g.chunks = (g.HW + kUpLanes - 1) / kUpLanes;
  g.xi = xi; g.xc = xc;
  const int64_t nblk = N * g.chunks;  // < 2^31: N * HW is
  const UpWorkspace u = carve(workspace, nblk, N * g.HW);
  hipStream_t st = (hipStream_t)stream;
  const dim3 fgrid((unsigned)nblk), bgrid((unsigned)(N * g.lchunks), (unsigned)((C + kUpBwdC - 1) / kUpBwdC));

#define NBDT_UPX_LAUNCH(LD)                                                                                          \
  do {                                                                                                               \
    hipLaunchKernelGGL(upx_fwd_kernel<LD>, fgrid, dim3(kUpLanes), 0, st, g, x, y, ignore_index, weight, smoothing, u); \
    NBDT_LAUNCH_CHECK();                                                                                             \
    hipLaunchKernelGGL(upx_fold_kernel, dim3(1), dim3(kFoldBlock), 0, st, u, nblk, loss);                            \
    NBDT_LAUNCH_CHECK();                                                                                             \
    hipLaunchKernelGGL(upx_bwd_kernel<LD>, bgrid, dim3(kUpLanes), 0, st, g, x, weight, smoothing, grad_scale, u, gx); \
    NBDT_LAUNCH_CHECK();                                                                                             \
  } while (0)
  if (xtype == NBDT_F32) NBDT_UPX_LAUNCH(LoadF32);
  else if (xtype == NBDT_BF16) NBDT_UPX_LAUNCH(LoadBF16);
  else NBDT_UPX_LAUNCH(LoadF16);
#undef NBDT_UPX_LAUNCH
  return NBDT_OK;
}
