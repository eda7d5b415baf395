// Grouped 3x3 convolution of a ResNeXt bottleneck (torchvision.models.resnet.Bottleneck.conv2 with groups > 1): forward,
// data gradient, weight gradient, the weight expansion they read, and fp32-storage twins (gfx950 only).
//
// The block-diagonal argument.  cin == cout == width, width % 32 == 0, and cg = width / groups is 4, 8, 16 or 32 -- it
// divides 32, so a group never straddles a 32-channel boundary and output channels [32 n, 32 n + 32) depend on input
// channels [32 n, 32 n + 32) only.  The grouped conv is width / 32 INDEPENDENT dense 32 -> 32 convolutions whose 32 x 9 x 32
// weight block is block-diagonal (32 / cg diagonal cg x cg sub-blocks, zeros elsewhere), and a 32 x 32 block is one
// v_mfma_f32_32x32x16_bf16 tile: one wave, 32 pixels x 32 channels, ONE accumulator, 9 taps x 2 MFMAs.  The zeros are
// multiplied (8x the useful flops at cg = 4): per pixel and channel block 18,432 flop against 64 B in + 64 B out.
//
// Tensors are the project's padded NHWC [B][H+2][W+2][width] with a zero ring; only interior pixels are written, the
// ring of an input is read as the convolution's zero padding (every tap address lies inside the padded tensor, so no
// tap is predicated), pixel counts that are no multiple of 32 repeat the last pixel in the idle lanes and skip its store.
//
//   nbdt_conv_group_weight_prep[_batched]   fp32 master [width][9][cg] -> bf16 blocks wf[width/32][32 co][9][32 ci] with
//                                           explicit zeros off the group diagonal, and wd[width/32][32 ci][9][32 co], taps
//                                           reversed: wd[n][ci][t][co] = wf[n][co][8 - t][ci] (as nbdt_weight_prep's copy)
//   nbdt_conv_group_fwd / _dgrad            conv_group_kernel: plain __global__ C++, no LDS, no inline assembly.  A wave
//                                           keeps the 18 weight fragments of its channel block in registers and walks
//                                           32-pixel chunks; per tap it reads 2 x 16 B per lane straight from memory (the
//                                           9x tap re-reads are L1 / L2 hits).  The 4 waves of a workgroup are 2 chunks x 2
//                                           ADJACENT channel blocks, so together they use every 128-byte line whole.
//                                           MFMA "transposed" (A = weights, B = pixels): a lane ends with 16 channels of
//                                           ONE pixel; the two lane halves swap 8 bytes so that each stores 16 contiguous
//                                           bytes.  fp32 accumulation in tap order, one round-to-nearest-even at the store.
//                                           Stride 1: the data gradient IS the forward kernel over wd.  Stride 2: gather
//                                           form over the four input-parity classes, a chunk lies in one class and runs
//                                           the 4 / 2 / 2 / 1 taps its parity allows.  No accumulate form.
//   nbdt_conv_group_wgrad                   conv_group_wgrad_kernel: k = pixels, so both operands are read ACROSS
//                                           pixels: each wave copies its 32-pixel x 32-channel tiles (gy once, x per tap)
//                                           into a wave-private LDS tile with 16-byte accesses and reads the fragments back
//                                           transposed, two bytes at a time.  Nine accumulators (one per tap) per wave;
//                                           a wave owns pixel split s of S (chunks s, s + S, ...: a fixed order), stores the
//                                           diagonal cg x cg sub-blocks of its sums to row s of a per-stream workspace
//                                           with plain stores -- products off the diagonal are never stored -- and det_fold
//                                           adds the S rows onto dw in row order.  No atomics: two runs leave the same bits.
//   nbdt_ref_conv_group_{fwd,dgrad,wgrad}   one thread per output, direct loops over the fp32 master (csrc/ref_fp32.hip's style)
#include "common.h"

using namespace nbdt;

namespace {

typedef __attribute__((ext_vector_type(8))) short g_bf16x8;
typedef __attribute__((ext_vector_type(16))) float g_f32x16;

struct GroupGeom {
  int B, Hi, Wi, Ho, Wo, C;  // the conv's input / output sides, C = width
  int nblk;                  // C / 32
  int M;                     // pixels a launch enumerates (per parity class for the strided data gradient)
  int cpc;                   // 32-pixel chunks per parity class
  int nchunks;               // all chunks
};

constexpr int MODE_S1 = 0;       // stride-1 gather: forward and data gradient (over wd)
constexpr int MODE_FWD_S2 = 1;   // stride-2 forward
constexpr int MODE_DGRAD_S2 = 2; // stride-2 data gradient, gather form over input-parity classes

__device__ __forceinline__ float group_act(float v, int act) {
  if (act == NBDT_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == NBDT_ACT_SWISH) return v / (1.f + __expf(-v));
  return v;
}

template <int MODE, bool AFFINE>
__global__ __launch_bounds__(256) void conv_group_kernel(const bf16_t* __restrict__ in, const bf16_t* __restrict__ wexp,
                                                         bf16_t* __restrict__ out, GroupGeom g,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         int act) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int blk = blockIdx.y * 2 + (wave & 1);
  if (blk >= g.nblk) return;       // (an odd number of channel blocks; no barrier follows)
  const int r = lane & 31, h = lane >> 5;
  // A operand of k-step s, tap t: wexp[blk][row r][t][16 s + 8 h .. + 7]
  g_bf16x8 wf[9][2];
  const bf16_t* wb = wexp + ((size_t)blk * 32 + r) * 288 + 8 * h;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    wf[t][0] = *(const g_bf16x8*)(wb + t * 32);
    wf[t][1] = *(const g_bf16x8*)(wb + t * 32 + 16);
  }
  float sc[16], sh[16];
  if (AFFINE) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 a = *(const float4*)(scale + blk * 32 + 8 * q + 4 * h);
      const float4 b = *(const float4*)(shift + blk * 32 + 8 * q + 4 * h);
      sc[4 * q] = a.x; sc[4 * q + 1] = a.y; sc[4 * q + 2] = a.z; sc[4 * q + 3] = a.w;
      sh[4 * q] = b.x; sh[4 * q + 1] = b.y; sh[4 * q + 2] = b.z; sh[4 * q + 3] = b.w;
    }
  }
  constexpr int S = MODE == MODE_FWD_S2 ? 2 : 1;
  // the tensor the taps read: the conv's input (forward), or for a data gradient the output gradient
  const int in_ph = (MODE == MODE_DGRAD_S2 ? g.Ho : g.Hi) + 2, in_pw = (MODE == MODE_DGRAD_S2 ? g.Wo : g.Wi) + 2;
  const int out_ph = (MODE == MODE_DGRAD_S2 ? g.Hi : g.Ho) + 2, out_pw = (MODE == MODE_DGRAD_S2 ? g.Wi : g.Wo) + 2;
  for (int chunk = blockIdx.x * 2 + (wave >> 1); chunk < g.nchunks; chunk += gridDim.x * 2) {
    int cls = 0, local = chunk;
    if (MODE == MODE_DGRAD_S2) {
      cls = chunk / g.cpc;
      local = chunk - cls * g.cpc;
    }
    const int py = cls >> 1, px = cls & 1;
    const int p = local * 32 + r;
    const bool live = p < g.M;
    const int pc = live ? p : g.M - 1;
    const int x = pc % g.Wo, t2 = pc / g.Wo, y = t2 % g.Ho, b = t2 / g.Ho;     // (MODE_S1: Ho == Hi, Wo == Wi)
    g_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int tr = 0; tr < 3; ++tr) {
      // stride-2 data gradient: input row iy = 2 y + py takes tap row tr of wd from output row (iy - 1 + tr) / 2 when that
      // is whole; as a padded row index: (iy + 1 + tr) / 2
      if (MODE == MODE_DGRAD_S2 && ((py + 1 + tr) & 1)) continue;      // wave-uniform
      const int row = MODE == MODE_DGRAD_S2 ? y + ((py + 1 + tr) >> 1) : y * S + tr;
#pragma unroll
      for (int ts = 0; ts < 3; ++ts) {
        if (MODE == MODE_DGRAD_S2 && ((px + 1 + ts) & 1)) continue;
        const int col = MODE == MODE_DGRAD_S2 ? x + ((px + 1 + ts) >> 1) : x * S + ts;
        const bf16_t* ip = in + (((size_t)b * in_ph + row) * in_pw + col) * g.C + blk * 32 + 8 * h;
        const g_bf16x8 p0 = *(const g_bf16x8*)ip, p1 = *(const g_bf16x8*)(ip + 16);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[3 * tr + ts][0], p0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[3 * tr + ts][1], p1, acc, 0, 0, 0);
      }
    }
    // acc[i] is channel (i & 3) + 8 (i >> 2) + 4 h of pixel r: quad q = i >> 2 holds channels 8 q + 4 h .. + 3
    unsigned pk[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = acc[4 * q + j];
        if (AFFINE) v[j] = group_act(v[j] * sc[4 * q + j] + sh[4 * q + j], act);
      }
      pk[q][0] = pack_bf16x2(v[0], v[1]);
      pk[q][1] = pack_bf16x2(v[2], v[3]);
    }
    const int oy = MODE == MODE_DGRAD_S2 ? 2 * y + py + 1 : y + 1, ox = MODE == MODE_DGRAD_S2 ? 2 * x + px + 1 : x + 1;
    bf16_t* op = out + (((size_t)b * out_ph + oy) * out_pw + ox) * g.C + blk * 32;
#pragma unroll
    for (int q0 = 0; q0 < 4; q0 += 2) {
      // half 0 keeps quad q0 and takes half 1's (channels 8 q0 .. + 7); half 1 keeps quad q0 + 1 and takes half 0's
      const unsigned s0 = h ? pk[q0][0] : pk[q0 + 1][0], s1 = h ? pk[q0][1] : pk[q0 + 1][1];
      const unsigned r0 = __shfl_xor(s0, 32, 64), r1 = __shfl_xor(s1, 32, 64);
      u32x4_t v;
      if (h == 0) { v[0] = pk[q0][0]; v[1] = pk[q0][1]; v[2] = r0; v[3] = r1; }
      else { v[0] = r0; v[1] = r1; v[2] = pk[q0 + 1][0]; v[3] = pk[q0 + 1][1]; }
      if (live) *(u32x4_t*)(op + 8 * (q0 + h)) = v;
    }
  }
}

// ---- weight gradient
constexpr int WG_PITCH = 80;                  // bytes per pixel row of an LDS tile: 64 of data; the two lane halves of a
constexpr int WG_TILE = 32 * WG_PITCH;        // transposed read (8 rows apart) then meet different banks

__device__ __forceinline__ void wave_lds_order() {
  // LDS instructions of one wave execute in order; this keeps the compiler from moving accesses across the hand-over
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// element [16 s + 8 h + j][c] of a [32 pixels][32 channels] tile, j = 0 .. 7: the MFMA operand with k = pixel
__device__ __forceinline__ g_bf16x8 tile_column(const unsigned char* tile, int s, int h, int c) {
  g_bf16x8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = *(const short*)(tile + (16 * s + 8 * h + j) * WG_PITCH + 2 * c);
  return f;
}

template <int STRIDE>
__global__ __launch_bounds__(256, 2) void conv_group_wgrad_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ gy,
                                                                  float* __restrict__ part, GroupGeom g, int cg, int splits) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[4][2][WG_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int blk = blockIdx.y * 2 + (wave & 1);
  const int split = blockIdx.x * 2 + (wave >> 1);
  if (blk >= g.nblk || split >= splits) return;      // (no block-wide barrier follows)
  unsigned char* gt = lds[wave][0];
  unsigned char* xt = lds[wave][1];
  const int r = lane & 31, h = lane >> 5;
  const int piece = lane & 3;                        // 16-byte piece of a pixel's 64-byte channel segment
  g_f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  const u32x4_t zero = {0u, 0u, 0u, 0u};
  for (int chunk = split; chunk < g.nchunks; chunk += splits) {
    const bf16_t* xb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pl = 16 * i + (lane >> 2);
      const int p = chunk * 32 + pl;
      const bool live = p < g.M;
      const int pc = live ? p : g.M - 1;
      const int px = pc % g.Wo, t2 = pc / g.Wo, py = t2 % g.Ho, b = t2 / g.Ho;
      const bf16_t* gp = gy + (((size_t)b * (g.Ho + 2) + py + 1) * (g.Wo + 2) + px + 1) * g.C + blk * 32 + 8 * piece;
      // pixels past the end add nothing: their gradient is zero (x re-reads the last pixel)
      *(u32x4_t*)(gt + pl * WG_PITCH + 16 * piece) = live ? *(const u32x4_t*)gp : zero;
      xb[i] = x + (((size_t)b * (g.Hi + 2) + py * STRIDE) * (g.Wi + 2) + px * STRIDE) * g.C + blk * 32 + 8 * piece;
    }
    wave_lds_order();
    const g_bf16x8 a0 = tile_column(gt, 0, h, r), a1 = tile_column(gt, 1, h, r);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const size_t tap = ((size_t)(t / 3) * (g.Wi + 2) + (t % 3)) * g.C;
#pragma unroll
      for (int i = 0; i < 2; ++i)
        *(u32x4_t*)(xt + (16 * i + (lane >> 2)) * WG_PITCH + 16 * piece) = *(const u32x4_t*)(xb[i] + tap);
      wave_lds_order();
      const g_bf16x8 b0 = tile_column(xt, 0, h, r), b1 = tile_column(xt, 1, h, r);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[t], 0, 0, 0);
      wave_lds_order();
    }
  }
  // acc[t][i]: cout (i & 3) + 8 (i >> 2) + 4 h (row), cin r (column) of the block; only the group diagonal is kept
  float* dst = part + (size_t)split * g.C * 9 * cg;
  const int ci_group = r / cg, ci_in = r - ci_group * cg;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = (i & 3) + 8 * (i >> 2) + 4 * h;
      if (co / cg == ci_group) dst[((size_t)(blk * 32 + co) * 9 + t) * cg + ci_in] = acc[t][i];
    }
}

// ---- weight expansion: one workgroup per 32-channel block
struct PrepRow {
  long long src, dst;     // element offsets of the master in `flat` and of the layer's blocks in wf / wd
  int width, cg;
  long long first;        // index of the layer's first block among all blocks of the launch
};

__global__ __launch_bounds__(256) void conv_group_prep_kernel(const float* __restrict__ flat, const long long* __restrict__ table,
                                                              int n, PrepRow one, bf16_t* __restrict__ wf,
                                                              bf16_t* __restrict__ wd) {
  PrepRow row = one;
  if (table != nullptr) {     // rows {src, dst, width, cg, first block}, first ascending
    int l = 0;
    while (l + 1 < n && table[(l + 1) * 5 + 4] <= (long long)blockIdx.x) ++l;
    row.src = table[l * 5];
    row.dst = table[l * 5 + 1];
    row.width = (int)table[l * 5 + 2];
    row.cg = (int)table[l * 5 + 3];
    row.first = table[l * 5 + 4];
  }
  const int blk = (int)((long long)blockIdx.x - row.first);
  if (blk < 0 || blk >= row.width / 32) return;
  const int cg = row.cg;
  const float* w = flat + row.src + (size_t)blk * 32 * 9 * cg;     // [32 co][9][cg]
  const size_t base = (size_t)row.dst + (size_t)blk * 9216;
  for (int e = threadIdx.x; e < 9216; e += 256) {
    const int c = e & 31, t = (e >> 5) % 9, rw = e / 288;
    const bool diag = rw / cg == c / cg;
    if (wf != nullptr)        // wf[co = rw][t][ci = c]
      wf[base + e] = diag ? f32_to_bf16(w[((size_t)rw * 9 + t) * cg + c % cg]) : (bf16_t)0;
    if (wd != nullptr)        // wd[ci = rw][t][co = c] = w[co][8 - t][ci]
      wd[base + e] = diag ? f32_to_bf16(w[((size_t)c * 9 + (8 - t)) * cg + rw % cg]) : (bf16_t)0;
  }
}

// ---- fp32-storage twins: one thread per output, direct loops over the master [width][9][cg]
__global__ __launch_bounds__(256) void ref_group_fwd_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                            float* __restrict__ out, GroupGeom g, int cg, int stride,
                                                            long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int co = (int)(idx % g.C);
  long long m = idx / g.C;
  const int x = (int)(m % g.Wo);
  m /= g.Wo;
  const int y = (int)(m % g.Ho), b = (int)(m / g.Ho);
  const int c0 = co / cg * cg;
  float acc = 0.f;
  for (int t = 0; t < 9; ++t) {
    const float* a = in + (((size_t)b * (g.Hi + 2) + y * stride + t / 3) * (g.Wi + 2) + x * stride + t % 3) * g.C + c0;
    const float* k = w + ((size_t)co * 9 + t) * cg;
    float s = 0.f;
    for (int c = 0; c < cg; ++c) s += a[c] * k[c];
    acc += s;
  }
  out[(((size_t)b * (g.Ho + 2) + y + 1) * (g.Wo + 2) + x + 1) * g.C + co] = acc;
}

__global__ __launch_bounds__(256) void ref_group_dgrad_kernel(const float* __restrict__ gy, const float* __restrict__ w,
                                                              float* __restrict__ gx, GroupGeom g, int cg, int stride,
                                                              long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ci = (int)(idx % g.C);
  long long m = idx / g.C;
  const int ix = (int)(m % g.Wi);
  m /= g.Wi;
  const int iy = (int)(m % g.Hi), b = (int)(m / g.Hi);
  const int c0 = ci / cg * cg, cl = ci - c0;
  float acc = 0.f;
  for (int t = 0; t < 9; ++t) {
    const int ny = iy + 1 - t / 3, nx = ix + 1 - t % 3;      // stride * (output position)
    if (ny < 0 || nx < 0 || ny % stride || nx % stride) continue;
    const int oy = ny / stride, ox = nx / stride;
    if (oy >= g.Ho || ox >= g.Wo) continue;
    const float* a = gy + (((size_t)b * (g.Ho + 2) + oy + 1) * (g.Wo + 2) + ox + 1) * g.C + c0;
    float s = 0.f;
    for (int c = 0; c < cg; ++c) s += a[c] * w[((size_t)(c0 + c) * 9 + t) * cg + cl];
    acc += s;
  }
  gx[(((size_t)b * (g.Hi + 2) + iy + 1) * (g.Wi + 2) + ix + 1) * g.C + ci] = acc;
}

__global__ __launch_bounds__(256) void ref_group_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                              float* __restrict__ dw, GroupGeom g, int cg, int stride,
                                                              long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int cl = (int)(idx % cg), t = (int)((idx / cg) % 9), co = (int)(idx / (9 * cg));
  const int ci = co / cg * cg + cl;
  double s = 0.0;
  for (int b = 0; b < g.B; ++b)
    for (int y = 0; y < g.Ho; ++y)
      for (int xx = 0; xx < g.Wo; ++xx)
        s += (double)gy[(((size_t)b * (g.Ho + 2) + y + 1) * (g.Wo + 2) + xx + 1) * g.C + co] *
             (double)x[(((size_t)b * (g.Hi + 2) + y * stride + t / 3) * (g.Wi + 2) + xx * stride + t % 3) * g.C + ci];
  dw[idx] += (float)s;
}

inline GroupGeom group_geom(int B, int H, int W, int width, int stride) {
  GroupGeom g;
  g.B = B; g.Hi = H; g.Wi = W; g.Ho = H / stride; g.Wo = W / stride; g.C = width;
  g.nblk = width / 32;
  g.M = B * g.Ho * g.Wo;
  g.cpc = (g.M + 31) / 32;
  g.nchunks = g.cpc;
  return g;
}

// workgroups along the pixel axis: two chunks each, about four workgroups per CU over both axes (a wave re-uses its
// weight fragments for every chunk it walks)
inline dim3 group_grid(const GroupGeom& g) {
  const int gy = (g.nblk + 1) / 2;
  int gx = (g.nchunks + 1) / 2;
  const int cap = 1024 / gy > 0 ? 1024 / gy : 1;
  gx = gx < cap ? gx : cap;
  return dim3((unsigned)gx, (unsigned)gy);
}

}  // namespace

#define NBDT_GROUP_ARGS()                                                                                            \
  NBDT_REQUIRE(width > 0 && width % 32 == 0, "width must be a multiple of 32");                                      \
  NBDT_REQUIRE(cg == 4 || cg == 8 || cg == 16 || cg == 32,                                                            \
               "channels per group must be 4, 8, 16 or 32 (cg = 64, resnext101_32x8d's layer4, is not supported)");   \
  NBDT_REQUIRE(stride == 1 || stride == 2, "stride is 1 or 2");                                                       \
  NBDT_REQUIRE(B > 0 && H > 0 && W > 0, "empty batch or image");                                                      \
  NBDT_REQUIRE(H <= 16384 && W <= 16384 && width <= 65536, "oversized tensor");                                       \
  NBDT_REQUIRE(stride == 1 || (H % 2 == 0 && W % 2 == 0), "a stride-2 conv takes even input sides");                  \
  NBDT_REQUIRE((int64_t)B * (H + 2) * (W + 2) < (1ll << 31), "pixel grid too large")

extern "C" int nbdt_conv_group_weight_prep(const float* w, int32_t width, int32_t cg, void* wf_bf16, void* wd_bf16,
                                           void* stream) {
  NBDT_REQUIRE(w && (wf_bf16 || wd_bf16), "null argument");
  NBDT_REQUIRE(width > 0 && width % 32 == 0 && width <= 65536, "width must be a multiple of 32");
  NBDT_REQUIRE(cg == 4 || cg == 8 || cg == 16 || cg == 32,
               "channels per group must be 4, 8, 16 or 32 (cg = 64, resnext101_32x8d's layer4, is not supported)");
  PrepRow one{0, 0, width, cg, 0};
  hipLaunchKernelGGL(conv_group_prep_kernel, dim3((unsigned)(width / 32)), dim3(256), 0, (hipStream_t)stream, w,
                     (const long long*)nullptr, 1, one, (bf16_t*)wf_bf16, (bf16_t*)wd_bf16);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_conv_group_weight_prep_batched(const float* flat, const int64_t* table, int32_t n_layers,
                                                   int64_t total_blocks, void* wf_flat, void* wd_flat, void* stream) {
  NBDT_REQUIRE(flat && table && (wf_flat || wd_flat), "null argument");
  NBDT_REQUIRE(n_layers > 0 && total_blocks > 0 && total_blocks < (1ll << 31), "empty or oversized layer table");
  PrepRow one{0, 0, 0, 4, 0};
  hipLaunchKernelGGL(conv_group_prep_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, flat,
                     (const long long*)table, n_layers, one, (bf16_t*)wf_flat, (bf16_t*)wd_flat);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_conv_group_fwd(const void* in, const void* wf, void* out, int32_t B, int32_t H, int32_t W, int32_t width,
                                   int32_t cg, int32_t stride, const float* scale, const float* shift, int32_t act,
                                   void* stream) {
  NBDT_REQUIRE(in && wf && out, "null argument");
  NBDT_GROUP_ARGS();
  NBDT_REQUIRE((scale == nullptr) == (shift == nullptr), "scale and shift come together");
  NBDT_REQUIRE(act == NBDT_ACT_NONE || ((act == NBDT_ACT_RELU || act == NBDT_ACT_SWISH) && scale != nullptr),
               "act is NBDT_ACT_NONE, or RELU / SWISH together with scale and shift");
  const GroupGeom g = group_geom(B, H, W, width, stride);
  const dim3 grid = group_grid(g);
  hipStream_t st = (hipStream_t)stream;
  const bf16_t *i = (const bf16_t*)in, *w = (const bf16_t*)wf;
  bf16_t* o = (bf16_t*)out;
  if (stride == 1) {
    if (scale) hipLaunchKernelGGL((conv_group_kernel<MODE_S1, true>), grid, dim3(256), 0, st, i, w, o, g, scale, shift, act);
    else hipLaunchKernelGGL((conv_group_kernel<MODE_S1, false>), grid, dim3(256), 0, st, i, w, o, g, scale, shift, act);
  } else {
    if (scale) hipLaunchKernelGGL((conv_group_kernel<MODE_FWD_S2, true>), grid, dim3(256), 0, st, i, w, o, g, scale, shift, act);
    else hipLaunchKernelGGL((conv_group_kernel<MODE_FWD_S2, false>), grid, dim3(256), 0, st, i, w, o, g, scale, shift, act);
  }
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_conv_group_dgrad(const void* gout, const void* wd, void* gin, int32_t B, int32_t H, int32_t W,
                                     int32_t width, int32_t cg, int32_t stride, int32_t accumulate, void* stream) {
  NBDT_REQUIRE(gout && wd && gin, "null argument");
  NBDT_GROUP_ARGS();
  NBDT_REQUIRE(accumulate == 0, "the grouped data gradient has no accumulate form");
  hipStream_t st = (hipStream_t)stream;
  const bf16_t *i = (const bf16_t*)gout, *w = (const bf16_t*)wd;
  bf16_t* o = (bf16_t*)gin;
  if (stride == 1) {
    const GroupGeom g = group_geom(B, H, W, width, 1);
    hipLaunchKernelGGL((conv_group_kernel<MODE_S1, false>), group_grid(g), dim3(256), 0, st, i, w, o, g,
                       (const float*)nullptr, (const float*)nullptr, 0);
  } else {
    GroupGeom g = group_geom(B, H, W, width, 2);      // M: the pixels of one input-parity class = the output pixels
    g.nchunks = 4 * g.cpc;
    hipLaunchKernelGGL((conv_group_kernel<MODE_DGRAD_S2, false>), group_grid(g), dim3(256), 0, st, i, w, o, g,
                       (const float*)nullptr, (const float*)nullptr, 0);
  }
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_conv_group_wgrad(const void* x, const void* gout, float* dw, int32_t B, int32_t H, int32_t W,
                                     int32_t width, int32_t cg, int32_t stride, void* stream) {
  NBDT_REQUIRE(x && gout && dw, "null argument");
  NBDT_GROUP_ARGS();
  const GroupGeom g = group_geom(B, H, W, width, stride);
  // pixel splits: about 2048 waves in all (1024 at cg = 32, whose rows are the largest), never more than chunks
  int splits = (cg == 32 ? 1024 : 2048) / g.nblk;
  splits = splits < 1 ? 1 : splits > g.nchunks ? g.nchunks : splits;
  const size_t n = (size_t)width * 9 * cg;
  hipStream_t st = (hipStream_t)stream;
  float* rows = det_rows(st, (size_t)splits * n);
  if (rows == nullptr) return fail(NBDT_ENOMEM, "nbdt_conv_group_wgrad: no workspace for the per-split sums: %s", det_rows_why());
  const dim3 grid((unsigned)((splits + 1) / 2), (unsigned)((g.nblk + 1) / 2));
  if (stride == 1)
    hipLaunchKernelGGL(conv_group_wgrad_kernel<1>, grid, dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)gout, rows, g, cg, splits);
  else
    hipLaunchKernelGGL(conv_group_wgrad_kernel<2>, grid, dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)gout, rows, g, cg, splits);
  NBDT_LAUNCH_CHECK();
  return det_fold(st, rows, splits, n, dw);       // dw += row 0 + row 1 + ...: onto whatever .grad already holds
}

extern "C" int nbdt_ref_conv_group_fwd(const float* in, const float* w, float* out, int32_t B, int32_t H, int32_t W,
                                       int32_t width, int32_t cg, int32_t stride, void* stream) {
  NBDT_REQUIRE(in && w && out, "null argument");
  NBDT_GROUP_ARGS();
  const GroupGeom g = group_geom(B, H, W, width, stride);
  const long long total = (long long)g.M * width;
  NBDT_REQUIRE((total + 255) / 256 <= 0x7fffffffll, "too many elements for one launch");
  hipLaunchKernelGGL(ref_group_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, w,
                     out, g, cg, stride, total);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_ref_conv_group_dgrad(const float* gout, const float* w, float* gin, int32_t B, int32_t H, int32_t W,
                                         int32_t width, int32_t cg, int32_t stride, int32_t accumulate, void* stream) {
  NBDT_REQUIRE(gout && w && gin, "null argument");
  NBDT_GROUP_ARGS();
  NBDT_REQUIRE(accumulate == 0, "the grouped data gradient has no accumulate form");
  const GroupGeom g = group_geom(B, H, W, width, stride);
  const long long total = (long long)B * H * W * width;
  NBDT_REQUIRE((total + 255) / 256 <= 0x7fffffffll, "too many elements for one launch");
  hipLaunchKernelGGL(ref_group_dgrad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gout,
                     w, gin, g, cg, stride, total);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_ref_conv_group_wgrad(const float* x, const float* gout, float* dw, int32_t B, int32_t H, int32_t W,
                                         int32_t width, int32_t cg, int32_t stride, void* stream) {
  NBDT_REQUIRE(x && gout && dw, "null argument");
  NBDT_GROUP_ARGS();
  const GroupGeom g = group_geom(B, H, W, width, stride);
  const long long total = (long long)width * 9 * cg;
  hipLaunchKernelGGL(ref_group_wgrad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                     gout, dw, g, cg, stride, total);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}
