// ImageNet-style batch assembly on the device: gather by index + RandomResizedCrop(size) + RandomHorizontalFlip + ToTensor +
// Normalize for training, Resize(size + 32) + CenterCrop(size) + ToTensor + Normalize for evaluation (reference
// nbdt/data/imagenet.py:152-172), in ONE launch, from a uint8 dataset that lives in device memory, into the fp32 NCHW tensor
// the stem kernels of misc.hip read.  The second transform family next to augment.hip's padded crop.
//
// The resampling is PIL's bilinear filter as Image.resize applies it to an 8-bit image (what torchvision's transforms call
// on a PIL image): per axis a triangle filter whose support is max(1, in / out) source pixels, coefficients computed in
// fp64, normalised to sum 1 and rounded to 22-bit fixed point; the horizontal pass first, rounded and clipped to uint8;
// then the vertical pass over those uint8 values, rounded and clipped to uint8.  The filter's support is clipped at the
// crop box, not at the image: torchvision crops, then resizes.  Everything after the coefficients is integer arithmetic,
// so the result is the bytes PIL produces; nbdt/data.py resample_reference restates it in numpy.
//
// int32 accumulators: the coefficients of one output pixel are non-negative and sum to 2^22 before rounding, each rounding
// adds at most 1/2, and an axis has at most 2 * 4096 + 1 taps, so an accumulator stays below
// 2^21 + 255 * (2^22 + 4097) < 2^31.
//
// Two kernels.  resized_crop_lds: one block per (image, band of output rows); the source rows the band needs go to LDS
// with 16-byte loads, the horizontal pass writes a uint8 tile in LDS, the vertical pass reads that tile and a lane writes
// four consecutive x with one 16-byte store.  The band height is chosen on the host so that the worst box (the whole
// image) fits 64 KB.  resized_crop_global: a source too wide for that; one lane per output pixel, coefficients recomputed
// per tap, every source byte a global read.  Slow, and the same bytes.
//
// nbdt_resized_crop_policy_batch (further down) adds an augmentation policy and random erasing to the training transform:
// both kernels have a byte-output mode (template parameter BYTES) that writes the resized and flipped uint8 image to a
// staging buffer, and resized_crop_policy_kernel runs the chain of policy_ops.h's operations on it, one block per image,
// between two tiles in global memory, normalises and erases.  The float mode is the code it was.
//
// Built with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (nbdt/_build.py), like augment.hip: the fp64
// coefficient arithmetic is a sequence of single IEEE operations, and (u / 255 - mean) / std is the three fp32 operations
// of torch's CPU x.float().div(255).sub(mean).div(std).
#include "common.h"
#include "policy_ops.h"

using namespace nbdt;
using namespace nbdt::pol;      // mix64, pick3, round_sqrt: the draws' arithmetic is the policies'

#define NBDT_RESAMPLE_LDS_BYTES 65536
#define NBDT_RESAMPLE_PRECISION 22

namespace {

struct RcArgs {
  const unsigned char* src;
  const long long* labels_src;
  const long long* index;
  long long index_base;        // src / labels_src hold the samples [index_base, index_base + N) of the dataset index[] names
  long long N;
  int H, W;
  int rs_h, rs_w;              // the box is resampled to rs_h x rs_w ...
  int win_top, win_left;       // ... of which the window (win_top, win_left, out_h, out_w) is written
  int out_h, out_w;
  int flip_on;
  float mean[3], std[3];
  double s0, s1, r0, r1;       // scale and ratio ranges of the draw
  const double* ratio_table;   // NBDT_RESIZED_CROP_RATIOS log-spaced aspect ratios (device)
  unsigned long long key;
  const int* params_in;
  float* out;
  unsigned char* out_u8;       // the byte-output mode (BYTES): the resized, flipped uint8 image instead of `out`
  long long* labels_out;
  int* params_out;
  // LDS kernel only: band height, taps per axis, source rows per band, pitches
  int band, kx, ky, srows, spitch, opitch;
};

// torchvision's RandomResizedCrop.get_params with the project's counter hash (include/nbdt_hip.h, nbdt/data.py
// draw_resized_crop_params)
__device__ inline void draw_box(const RcArgs& a, unsigned long long base, int& top, int& left, int& h, int& w) {
  const int H = a.H, W = a.W;
  const double area = (double)((long long)H * W);
  for (int t = 0; t < NBDT_RESIZED_CROP_ATTEMPTS; ++t) {
    const unsigned long long ra = mix64(base + (unsigned long long)(2 * t + 1) * 0x9E3779B97F4A7C15ull);
    const unsigned long long rb = mix64(base + (unsigned long long)(2 * t + 2) * 0x9E3779B97F4A7C15ull);
    const double u = (double)(ra >> 11) * 0x1p-53;
    const double target = area * (a.s0 + u * (a.s1 - a.s0));
    const double rt = a.ratio_table[rb & (NBDT_RESIZED_CROP_RATIOS - 1)];
    const int cw = round_sqrt(target * rt), ch = round_sqrt(target / rt);
    if (cw > 0 && cw <= W && ch > 0 && ch <= H) {
      w = cw;
      h = ch;
      top = (int)((((rb >> 12) & 0xFFFFFFull) * (unsigned long long)(H - ch + 1)) >> 24);
      left = (int)((((rb >> 36) & 0xFFFFFFull) * (unsigned long long)(W - cw + 1)) >> 24);
      return;
    }
  }
  const double in_ratio = (double)W / (double)H;      // the fallback: a centre crop with the ratio clamped
  w = W;
  h = H;
  if (in_ratio < a.r0) h = (int)rint((double)W / a.r0);
  else if (in_ratio > a.r1) w = (int)rint((double)H * a.r1);
  h = h < 1 ? 1 : (h > H ? H : h);
  w = w < 1 ? 1 : (w > W ? W : w);
  top = (H - h) / 2;
  left = (W - w) / 2;
}

// (top, left, h, w, flip) of the block's sample: drawn, or params_in clamped into the image
__device__ inline void sample_params(const RcArgs& a, int b, long long gidx, int* p) {
  int top, left, h, w, fl;
  if (a.params_in) {
    const int* q = a.params_in + (size_t)b * 5;
    top = q[0]; left = q[1]; h = q[2]; w = q[3]; fl = q[4] != 0;
    top = top < 0 ? 0 : (top > a.H - 1 ? a.H - 1 : top);
    left = left < 0 ? 0 : (left > a.W - 1 ? a.W - 1 : left);
    h = h < 1 ? 1 : (h > a.H - top ? a.H - top : h);
    w = w < 1 ? 1 : (w > a.W - left ? a.W - left : w);
  } else {
    const unsigned long long base = mix64(a.key ^ ((unsigned long long)gidx * 0xD1342543DE82EF95ull));
    draw_box(a, base, top, left, h, w);
    fl = a.flip_on ? (int)(base >> 63) : 0;
  }
  p[0] = top; p[1] = left; p[2] = h; p[3] = w; p[4] = fl;
}

// One axis of PIL's precompute_coeffs for a source of `in` pixels resampled to `out`
struct Axis {
  double scale, support, ss;
  __device__ Axis(int in, int out) {
    scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    support = fs;            // the triangle filter's support is 1
    ss = 1.0 / fs;
  }
  // taps [xmin, xmin + cnt) of output pixel xx, and the sum ww of their weights
  __device__ void bounds(int xx, int in, int& xmin, int& cnt, double& center, double& ww) const {
    center = ((double)xx + 0.5) * scale;
    xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    cnt = xmax - xmin;
    ww = 0.0;
    for (int t = 0; t < cnt; ++t) ww += weight(t + xmin, center);
  }
  __device__ double weight(int x, double center) const {
    double v = ((double)x - center + 0.5) * ss;
    if (v < 0.0) v = -v;
    return v < 1.0 ? 1.0 - v : 0.0;
  }
  __device__ int coef(int x, double center, double ww) const {      // normalised, 22-bit fixed point
    double k = weight(x, center);
    if (ww != 0.0) k /= ww;
    return (int)(0.5 + k * (double)(1 << NBDT_RESAMPLE_PRECISION));
  }
};

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> NBDT_RESAMPLE_PRECISION;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ void write_header(const RcArgs& a, int b, bool valid, unsigned long long idx, const int* p) {
  a.labels_out[b] = valid ? a.labels_src[idx] : -1ll;
  if (a.params_out)
    for (int k = 0; k < 5; ++k) a.params_out[(size_t)b * 5 + k] = valid ? p[k] : 0;
}

// grid (bands, B).  Every address is formed only after its index has been checked: idx against [0, N), the box against the
// image (sample_params), taps against the box (Axis::bounds), LDS rows against a.srows.  idx is index[b] - index_base mod
// 2^64, compared unsigned (nbdt_resized_crop_batch_sharded; base 0 is the whole dataset): the draw hashes index[b], rows
// and labels are read at idx.
// BYTES: the byte-output mode of nbdt_resized_crop_policy_batch -- the same boxes and resampling, the uint8 result to
// a.out_u8 [B,3,out_h,out_w] (four packed bytes per lane where out_w % 4 == 0; the host has checked the alignment) and
// nothing to a.out; an invalid sample's tile is left as it is, nobody reads it.
template <bool BYTES>
__global__ __launch_bounds__(256) void resized_crop_lds(const RcArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int hdr[8];
  const int tid = threadIdx.x, b = blockIdx.y, y0 = blockIdx.x * a.band;
  const int rows = min(a.band, a.out_h - y0);
  const long long gidx = a.index[b];               // the dataset's index: what the draw hashes
  const unsigned long long idx = (unsigned long long)gidx - (unsigned long long)a.index_base;    // the row held here
  const bool valid = idx < (unsigned long long)a.N;
  const size_t n_out = (size_t)a.out_h * a.out_w;
  float* o = a.out + (size_t)b * 3 * n_out;
  if (!valid) {      // (block-uniform) a zero image, label -1, no source address formed
    if (tid == 0 && blockIdx.x == 0) write_header(a, b, false, idx, hdr);
    if (BYTES) return;
    for (int it = tid; it < 3 * rows * a.out_w; it += 256) {
      const int cy = it / a.out_w, x = it - cy * a.out_w;
      const int c = cy / rows, y = cy - c * rows;
      o[(size_t)c * n_out + (size_t)(y0 + y) * a.out_w + x] = 0.f;
    }
    return;
  }
  if (tid == 0) {
    sample_params(a, b, gidx, hdr);
    if (blockIdx.x == 0) write_header(a, b, true, idx, hdr);
  }
  __syncthreads();
  const int top = hdr[0], left = hdr[1], bh = hdr[2], bw = hdr[3], fl = hdr[4];

  int* cx = (int*)lds;                         // [out_w][kx] horizontal coefficients
  int* xb = cx + a.out_w * a.kx;               // [out_w] xmin | cnt << 16
  int* cyv = xb + a.out_w;                     // [band][ky] vertical coefficients
  int* yb = cyv + a.band * a.ky;               // [band] ymin | cnt << 16, then [2] first source row, row count
  unsigned char* srcs = (unsigned char*)(((uintptr_t)(yb + a.band + 2) + 15) & ~(uintptr_t)15);   // [3][srows][spitch]
  unsigned char* hts = srcs + (size_t)3 * a.srows * a.spitch;                                      // [3][srows][opitch]

  {  // coefficients: one lane per output column, one per output row of the band
    const Axis ax(bw, a.rs_w), ay(bh, a.rs_h);
    for (int j = tid; j < a.out_w; j += 256) {
      int xmin, cnt;
      double center, ww;
      ax.bounds(a.win_left + j, bw, xmin, cnt, center, ww);
      cnt = cnt < 0 ? 0 : (cnt > a.kx ? a.kx : cnt);
      for (int t = 0; t < cnt; ++t) cx[j * a.kx + t] = ax.coef(t + xmin, center, ww);
      xb[j] = xmin | (cnt << 16);
    }
    for (int y = tid; y < rows; y += 256) {
      int ymin, cnt;
      double center, ww;
      ay.bounds(a.win_top + y0 + y, bh, ymin, cnt, center, ww);
      cnt = cnt < 0 ? 0 : (cnt > a.ky ? a.ky : cnt);
      for (int t = 0; t < cnt; ++t) cyv[y * a.ky + t] = ay.coef(t + ymin, center, ww);
      yb[y] = ymin | (cnt << 16);
    }
  }
  __syncthreads();
  // the source rows of the band: [ys0, ys0 + nrows) of the box (ymin is non-decreasing in y)
  const int ys0 = yb[0] & 0xFFFF;
  int nrows = (yb[rows - 1] & 0xFFFF) + (yb[rows - 1] >> 16) - ys0;
  nrows = nrows > a.srows ? a.srows : nrows;      // cannot exceed it (host: resample_plan); never index past the tile

  // stage: 16-byte loads of the aligned chunks that cover each row's [left, left + bw)
  const unsigned char* img = a.src + (size_t)idx * 3 * a.H * a.W;
  const uintptr_t lo = (uintptr_t)a.src, hi = lo + (size_t)a.N * 3 * a.H * a.W;
  const int nchunk = a.spitch >> 4;
  for (int it = tid; it < 3 * nrows * nchunk; it += 256) {
    const int cr = it / nchunk, k = it - cr * nchunk;
    const int c = cr / nrows, r = cr - c * nrows;
    const uintptr_t g = (uintptr_t)(img + ((size_t)c * a.H + top + ys0 + r) * a.W + left);
    const uintptr_t ga = (g & ~(uintptr_t)15) + ((uintptr_t)k << 4);
    if (ga >= g + bw) continue;                 // past the row's last byte
    u32x4_t v;
    if (ga >= lo && ga + 16 <= hi) {
      v = *(const u32x4_t*)ga;                  // inside the dataset: neighbouring bytes are read and not used
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {             // the dataset's first or last bytes: byte by byte, each one checked
        unsigned word = 0;
#pragma unroll
        for (int k8 = 0; k8 < 4; ++k8) {
          const uintptr_t p = ga + 4 * q + k8;
          const unsigned byte = (p >= lo && p < hi) ? *(const unsigned char*)p : 0u;
          word |= byte << (8 * k8);
        }
        v[q] = word;
      }
    }
    *(u32x4_t*)(srcs + ((size_t)c * a.srows + r) * a.spitch + (k << 4)) = v;
  }
  __syncthreads();
  // horizontal pass: uint8 tile [3][nrows][out_w]
  for (int it = tid; it < 3 * nrows * a.out_w; it += 256) {
    const int cr = it / a.out_w, j = it - cr * a.out_w;
    const int c = cr / nrows, r = cr - c * nrows;
    const int shift = (int)((uintptr_t)(img + ((size_t)c * a.H + top + ys0 + r) * a.W + left) & 15);
    const unsigned char* s = srcs + ((size_t)c * a.srows + r) * a.spitch + shift;
    const int xmin = xb[j] & 0xFFFF, cnt = xb[j] >> 16;
    int acc = 1 << (NBDT_RESAMPLE_PRECISION - 1);
    for (int t = 0; t < cnt; ++t) acc += (int)s[xmin + t] * cx[j * a.kx + t];
    hts[((size_t)c * a.srows + r) * a.opitch + j] = (unsigned char)clip8(acc);
  }
  __syncthreads();
  // vertical pass + flip + normalise: four consecutive x per lane
  const int G = (a.out_w + 3) >> 2;
  const int vec_out = (a.out_w % 4 == 0 && (uintptr_t)a.out % 16 == 0) ? 1 : 0;
  for (int it = tid; it < 3 * rows * G; it += 256) {
    const int cy = it / G, g = it - cy * G;
    const int c = cy / rows, y = cy - c * rows;
    const int ymin = (yb[y] & 0xFFFF) - ys0, cnt = yb[y] >> 16;
    const float mean = pick3(a.mean, c), sd = pick3(a.std, c);
    float v[4];
    unsigned u8[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = g * 4 + k;
      const int j = x < a.out_w ? (fl ? a.out_w - 1 - x : x) : 0;
      int acc = 1 << (NBDT_RESAMPLE_PRECISION - 1);
      for (int t = 0; t < cnt; ++t) {
        const int r = ymin + t;
        const int u = r < nrows ? hts[((size_t)c * a.srows + r) * a.opitch + j] : 0;
        acc += u * cyv[y * a.ky + t];
      }
      u8[k] = (unsigned)clip8(acc);
      v[k] = ((float)clip8(acc) / 255.0f - mean) / sd;
    }
    if (BYTES) {
      unsigned char* d8 = a.out_u8 + (size_t)b * 3 * n_out + (size_t)c * n_out + (size_t)(y0 + y) * a.out_w + g * 4;
      if ((a.out_w & 3) == 0) {
        *(unsigned*)d8 = u8[0] | (u8[1] << 8) | (u8[2] << 16) | (u8[3] << 24);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (g * 4 + k < a.out_w) d8[k] = (unsigned char)u8[k];
      }
      continue;
    }
    float* dst = o + (size_t)c * n_out + (size_t)(y0 + y) * a.out_w + g * 4;
    if (vec_out) {
      *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (g * 4 + k < a.out_w) dst[k] = v[k];
    }
  }
}

// grid (ceil(3 * out_h * out_w / 256), B): one lane per output pixel, nothing staged
template <bool BYTES>
__global__ __launch_bounds__(256) void resized_crop_global(const RcArgs a) {
  __shared__ int hdr[8];
  const int tid = threadIdx.x, b = blockIdx.y;
  const long long gidx = a.index[b];               // the dataset's index: what the draw hashes
  const unsigned long long idx = (unsigned long long)gidx - (unsigned long long)a.index_base;    // the row held here
  const bool valid = idx < (unsigned long long)a.N;
  const int n_out = a.out_h * a.out_w;
  const int e = blockIdx.x * 256 + tid;
  float* o = a.out + (size_t)b * 3 * n_out;
  if (!valid) {
    if (tid == 0 && blockIdx.x == 0) write_header(a, b, false, idx, hdr);
    if (!BYTES && e < 3 * n_out) o[e] = 0.f;
    return;
  }
  if (tid == 0) {
    sample_params(a, b, gidx, hdr);
    if (blockIdx.x == 0) write_header(a, b, true, idx, hdr);
  }
  __syncthreads();
  if (e >= 3 * n_out) return;
  const int top = hdr[0], left = hdr[1], bh = hdr[2], bw = hdr[3], fl = hdr[4];
  const int c = e / n_out, yx = e - c * n_out;
  const int y = yx / a.out_w, x = yx - y * a.out_w;
  const int j = fl ? a.out_w - 1 - x : x;
  const Axis ax(bw, a.rs_w), ay(bh, a.rs_h);
  int xmin, xcnt, ymin, ycnt;
  double xc, xww, yc, yww;
  ax.bounds(a.win_left + j, bw, xmin, xcnt, xc, xww);
  ay.bounds(a.win_top + y, bh, ymin, ycnt, yc, yww);
  const unsigned char* plane = a.src + ((size_t)idx * 3 + c) * a.H * a.W;
  int acc = 1 << (NBDT_RESAMPLE_PRECISION - 1);
  for (int ty = 0; ty < ycnt; ++ty) {
    const unsigned char* s = plane + (size_t)(top + ymin + ty) * a.W + left + xmin;
    int hacc = 1 << (NBDT_RESAMPLE_PRECISION - 1);
    for (int tx = 0; tx < xcnt; ++tx) hacc += (int)s[tx] * ax.coef(xmin + tx, xc, xww);
    acc += clip8(hacc) * ay.coef(ymin + ty, yc, yww);
  }
  if (BYTES) a.out_u8[(size_t)b * 3 * n_out + e] = (unsigned char)clip8(acc);
  else o[e] = ((float)clip8(acc) / 255.0f - pick3(a.mean, c)) / pick3(a.std, c);
}

// ---- the policy chain and the erase on the resized crop (nbdt_resized_crop_policy_batch's second launch).  One block per
// image.  The chain ping-pongs between the image's tile of the staging buffer A (what the byte-output mode above wrote) and
// its tile of B, both in GLOBAL memory: 3 * S * S bytes are 150 KB at S = 224 and two of them fit no LDS.  A tile is
// written and re-read by this block alone, on one CU, so __syncthreads() (workgroup scope) is all the ordering the passes
// need; plain loads and stores, so the tile stays in that CU's L1 and the XCD's L2.  Only the statistics live in LDS.  The
// loop is the one policy_chain_kernel (policy.hip) runs, run_chain, and the rules are the same functions (policy_ops.h): an
// Identity slot costs no pass, statistics are collected again on the tile an operation reads, the last non-Identity
// operation is evaluated inside the output pass.  The chain is block-uniform, so every barrier is.
struct RcpArgs {
  const long long* index;
  long long index_base, N;
  int S;
  float mean[3], std[3];
  unsigned long long key;
  unsigned char* A;                  // uint8 [B,3,S,S]: the resized and flipped image, then scratch
  unsigned char* Bt;                 // uint8 [B,3,S,S]: scratch
  ChainSpec c;                       // the chain and the erase (policy_ops.h); the table is built for S x S
  int vec_out;                       // S % 4 == 0 and `out` 16-byte aligned (the tiles always are when S % 4 == 0)
  float* out;
};

// Lanes per image.  Measured at 512 images of 224 x 224 (two blocks per CU; profiles/resized_crop_policy_launch.txt): 256
// lanes 1150 - 1200 us per call, 512 lanes 861 - 890, 1024 lanes 848 - 897 -- a pass is a stream of dependent byte loads
// that wants waves to hide behind, and at 73 VGPRs two blocks of 16 waves still share a CU.  512 and 1024 tie at this batch
// within the spread of the rounds; 1024 was ahead in every fixed-chain timing (1 - 3 %) and is the wider one when a
// smaller batch leaves a block per CU or fewer.  Reading a point operation's four bytes with one load (WORD) instead of
// four: 850 - 890 against 899 - 925 us, and 685 against 961 us for four Brightness passes.
constexpr int kPolicyBlock = 1024;

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void resized_crop_policy_kernel(const RcpArgs a) {
  __shared__ unsigned hist[kStatWords];      // [3][256] histogram, then prefix sums, then the LUT; then stat[8]
  __shared__ double ac[6];                   // [3][2] AutoContrast's (scale, offset)
  const int b = blockIdx.x, tid = threadIdx.x;
  const int S = a.S, n = 3 * S * S;
  const long long gidx = a.index[b];               // the dataset's index: what the draws hash
  const unsigned long long idx = (unsigned long long)gidx - (unsigned long long)a.index_base;
  const bool valid = idx < (unsigned long long)a.N;
  float* o = a.out + (size_t)b * n;

  // ---- the sample's chain and rectangle (block-uniform; every lane computes them)
  int et, el, eh, ew;
  unsigned long long chain;
  chain_params(a.c, a.key, gidx, b, S, S, valid, chain, et, el, eh, ew);
  if (tid == 0) store_chain_params(a.c, b, chain, et, el, eh, ew);   // (the label and the box are the first launch's)
  if (!valid) {      // (block-uniform) an index the host could not check: a zero image, no tile read
    for (int i = tid; i < n; i += BLOCK) o[i] = 0.f;
    return;
  }
  unsigned char* cur = a.A + (size_t)b * n;
  unsigned char* oth = a.Bt + (size_t)b * n;
  if ((S & 3) == 0)
    run_chain<BLOCK, true>(a.c, chain, cur, oth, hist, ac, S, S, a.mean, a.std, a.vec_out, o, et, el, eh, ew, tid);
  else
    run_chain<BLOCK, false>(a.c, chain, cur, oth, hist, ac, S, S, a.mean, a.std, a.vec_out, o, et, el, eh, ew, tid);
}

// taps of one axis for the widest box (the whole side): PIL's ksize
int axis_taps(int in, int out) {
  double s = (double)in / (double)out;
  if (s < 1.0) s = 1.0;
  return (int)ceil(s) * 2 + 1;
}

// LDS bytes of resized_crop_lds for a band of `band` output rows, and the tile geometry; the source rows a band can need:
// its first tap is at least center0 - support - 1/2, its last below center0 + (band - 1) * scale + support + 1/2, so
// at most (band + 1) * max(1, H / rs_h) + 1 rows, rounded up
size_t lds_bytes(int H, int W, int rs_h, int rs_w, int out_w, int band, RcArgs* a) {
  double sy = (double)H / (double)rs_h;
  if (sy < 1.0) sy = 1.0;
  const int kx = axis_taps(W, rs_w), ky = axis_taps(H, rs_h);
  int srows = (int)floor((band + 1) * sy) + 2;
  if (srows > H) srows = H;
  const int spitch = ((W + 15) / 16 + 1) * 16, opitch = (out_w + 3) & ~3;
  if (a) { a->band = band; a->kx = kx; a->ky = ky; a->srows = srows; a->spitch = spitch; a->opitch = opitch; }
  return (size_t)4 * ((size_t)out_w * kx + out_w + (size_t)band * ky + band + 2) + 16 + (size_t)3 * srows * (spitch + opitch);
}

// the largest band of 16, 8, 4, 2, 1 output rows that fits; 0: no band fits, the global kernel runs
int plan_band(int H, int W, int rs_h, int rs_w, int out_h, int out_w, RcArgs* a) {
  for (int band = 16; band >= 1; band >>= 1) {
    if (band > 1 && band >= 2 * out_h) continue;
    if (lds_bytes(H, W, rs_h, rs_w, out_w, band, a) <= NBDT_RESAMPLE_LDS_BYTES) return band;
  }
  return 0;
}

int check_geometry(int32_t H, int32_t W, int32_t rs_h, int32_t rs_w, int32_t win_top, int32_t win_left, int32_t out_h,
                   int32_t out_w) {
  NBDT_REQUIRE(H > 0 && W > 0 && H <= 4096 && W <= 4096, "image sides must be 1..4096");
  NBDT_REQUIRE(rs_h > 0 && rs_w > 0 && rs_h <= 4096 && rs_w <= 4096, "resized sides must be 1..4096");
  NBDT_REQUIRE(out_h > 0 && out_w > 0, "empty output window");
  NBDT_REQUIRE(win_top >= 0 && win_left >= 0 && win_top <= rs_h - out_h && win_left <= rs_w - out_w,
               "the output window must lie inside the resized image");
  return NBDT_OK;
}

}  // namespace

extern "C" int nbdt_resized_crop_band_rows(int32_t H, int32_t W, int32_t rs_h, int32_t rs_w, int32_t win_top,
                                           int32_t win_left, int32_t out_h, int32_t out_w) {
  if (check_geometry(H, W, rs_h, rs_w, win_top, win_left, out_h, out_w) != NBDT_OK) return -1;
  return plan_band(H, W, rs_h, rs_w, out_h, out_w, nullptr);
}

// the arguments of both entries, checked before the first device call, into `a` (out / out_u8 are the caller's)
static int fill_args(RcArgs& a, const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index,
                     int64_t index_base, int32_t B, int64_t N, int32_t H, int32_t W, int32_t rs_h, int32_t rs_w,
                     int32_t win_top, int32_t win_left, int32_t out_h, int32_t out_w, int32_t flip, const float* mean,
                     const float* std, const double* scale, const double* ratio, const double* ratio_table, uint64_t seed,
                     uint64_t epoch, const int32_t* params_in, const void* out, int64_t* labels_out, int32_t* params_out) {
  NBDT_REQUIRE(src && labels_src && index && out && labels_out, "null argument");
  NBDT_REQUIRE(N <= 0 || (index_base >= 0 && index_base <= INT64_MAX - N),
               "index_base must be >= 0 and index_base + N must fit int64");
  NBDT_REQUIRE(src_dtype == NBDT_U8, "the resized crop takes a uint8 dataset (NBDT_U8)");
  NBDT_REQUIRE(B > 0 && B <= 65535, "batch must be 1..65535");
  NBDT_REQUIRE(N > 0, "empty dataset");
  if (int rc = check_geometry(H, W, rs_h, rs_w, win_top, win_left, out_h, out_w)) return rc;
  NBDT_REQUIRE(flip == 0 || flip == 1, "flip is 0 or 1");
  NBDT_REQUIRE(mean && std, "a uint8 dataset needs mean[3] and std[3]");
  NBDT_REQUIRE(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "std must be non-zero");
  if (!params_in) {
    NBDT_REQUIRE(scale && ratio && ratio_table, "the draw needs scale[2], ratio[2] and the ratio table");
    NBDT_REQUIRE(scale[0] > 0.0 && scale[0] <= scale[1] && scale[1] <= 1.0, "scale must satisfy 0 < lo <= hi <= 1");
    NBDT_REQUIRE(ratio[0] > 0.0 && ratio[0] <= ratio[1] && ratio[1] <= 64.0 && ratio[0] >= 1.0 / 64.0,
                 "ratio must satisfy 1/64 <= lo <= hi <= 64");
    a.s0 = scale[0]; a.s1 = scale[1]; a.r0 = ratio[0]; a.r1 = ratio[1];
    a.ratio_table = ratio_table;
  }
  a.src = (const unsigned char*)src;
  a.labels_src = (const long long*)labels_src;
  a.index = (const long long*)index;
  a.index_base = index_base;
  a.N = N; a.H = H; a.W = W;
  a.rs_h = rs_h; a.rs_w = rs_w; a.win_top = win_top; a.win_left = win_left; a.out_h = out_h; a.out_w = out_w;
  a.flip_on = flip;
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.std[c] = std[c]; }
  a.key = mix64((unsigned long long)seed * 0x9E3779B97F4A7C15ull + (unsigned long long)epoch);
  a.params_in = (const int*)params_in;
  a.labels_out = (long long*)labels_out;
  a.params_out = (int*)params_out;
  return NBDT_OK;
}

// the resampling launch: the LDS kernel with the largest band that fits, else the global-memory kernel
template <bool BYTES>
static void launch_resample(RcArgs& a, int32_t B, hipStream_t s) {
  const int band = plan_band(a.H, a.W, a.rs_h, a.rs_w, a.out_h, a.out_w, &a);
  if (band > 0) {
    const size_t bytes = lds_bytes(a.H, a.W, a.rs_h, a.rs_w, a.out_w, band, nullptr);
    hipLaunchKernelGGL(resized_crop_lds<BYTES>, dim3((a.out_h + band - 1) / band, B), dim3(256), bytes, s, a);
  } else {
    const long long blocks = ((long long)3 * a.out_h * a.out_w + 255) / 256;
    hipLaunchKernelGGL(resized_crop_global<BYTES>, dim3((unsigned)blocks, B), dim3(256), 0, s, a);
  }
}

extern "C" int nbdt_resized_crop_batch_sharded(const void* src, int32_t src_dtype, const int64_t* labels_src,
                                               const int64_t* index, int64_t index_base, int32_t B, int64_t N, int32_t H,
                                               int32_t W, int32_t rs_h, int32_t rs_w, int32_t win_top, int32_t win_left,
                                               int32_t out_h, int32_t out_w, int32_t flip, const float* mean,
                                               const float* std, const double* scale, const double* ratio,
                                               const double* ratio_table, uint64_t seed, uint64_t epoch,
                                               const int32_t* params_in, float* out, int64_t* labels_out,
                                               int32_t* params_out, void* stream) {
  RcArgs a = {};
  if (int rc = fill_args(a, src, src_dtype, labels_src, index, index_base, B, N, H, W, rs_h, rs_w, win_top, win_left, out_h,
                         out_w, flip, mean, std, scale, ratio, ratio_table, seed, epoch, params_in, out, labels_out,
                         params_out))
    return rc;
  a.out = out;
  launch_resample<false>(a, B, (hipStream_t)stream);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

// ---- the policy chain and the erase on the resized crop: the byte-output resampling into stage_a, then
// resized_crop_policy_kernel, both on the caller's stream
extern "C" int nbdt_resized_crop_policy_batch_sharded(
    const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index, int64_t index_base, int32_t B,
    int64_t N, int32_t H, int32_t W, int32_t S, int32_t flip, const float* mean, const float* std, const double* scale,
    const double* ratio, const double* ratio_table, int32_t mode, int32_t nbins, const int32_t* table, int32_t num_ops,
    int32_t magnitude, const int32_t* subpolicies, int32_t P, double erase_prob, const double* erase_scale,
    const double* erase_ratio, const double* erase_ratio_table, uint64_t seed, uint64_t epoch, const int32_t* params_in,
    const int32_t* chain_in, const int32_t* erase_in, void* stage_a, void* stage_b, float* out, int64_t* labels_out,
    int32_t* params_out, int32_t* chain_out, int32_t* erase_out, void* stream) {
  NBDT_REQUIRE(S >= 1 && S <= NBDT_RESIZED_CROP_POLICY_MAX_SIDE,
               "the crop side S must be 1..NBDT_RESIZED_CROP_POLICY_MAX_SIDE (512): Contrast's grey sum and its rounding "
               "(2*sum + S*S) / (2*S*S) are formed in 32 bits, which a 4096 x 4096 crop would overflow");
  RcArgs a = {};
  if (int rc = fill_args(a, src, src_dtype, labels_src, index, index_base, B, N, H, W, S, S, 0, 0, S, S, flip, mean, std,
                         scale, ratio, ratio_table, seed, epoch, params_in, out, labels_out, params_out))
    return rc;
  NBDT_REQUIRE(stage_a && stage_b && stage_a != stage_b, "null argument: the chain needs two distinct staging buffers");
  NBDT_REQUIRE((uintptr_t)stage_a % 16 == 0 && (uintptr_t)stage_b % 16 == 0, "the staging buffers must be 16-byte aligned");
  RcpArgs p = {};
  if (int rc = check_chain(p.c, mode, nbins, table, num_ops, magnitude, subpolicies, P, chain_in, true, true)) return rc;
  if (int rc = check_erase(p.c, erase_prob, erase_scale, erase_ratio, erase_ratio_table, !erase_in)) return rc;
  a.out_u8 = (unsigned char*)stage_a;
  p.index = a.index; p.index_base = index_base; p.N = N;
  p.S = S;
  for (int c = 0; c < 3; ++c) { p.mean[c] = mean[c]; p.std[c] = std[c]; }
  p.key = a.key;
  p.A = (unsigned char*)stage_a;
  p.Bt = (unsigned char*)stage_b;
  p.c.erase_in = erase_in;
  p.vec_out = (S % 4 == 0 && (uintptr_t)out % 16 == 0) ? 1 : 0;
  p.out = out;
  p.c.chain_out = chain_out; p.c.erase_out = erase_out;
  hipStream_t s = (hipStream_t)stream;
  launch_resample<true>(a, B, s);
  NBDT_LAUNCH_CHECK();
  hipLaunchKernelGGL(resized_crop_policy_kernel<kPolicyBlock>, dim3(B), dim3(kPolicyBlock), 0, s, p);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_resized_crop_policy_batch(
    const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index, int32_t B, int64_t N, int32_t H,
    int32_t W, int32_t S, int32_t flip, const float* mean, const float* std, const double* scale, const double* ratio,
    const double* ratio_table, int32_t mode, int32_t nbins, const int32_t* table, int32_t num_ops, int32_t magnitude,
    const int32_t* subpolicies, int32_t P, double erase_prob, const double* erase_scale, const double* erase_ratio,
    const double* erase_ratio_table, uint64_t seed, uint64_t epoch, const int32_t* params_in, const int32_t* chain_in,
    const int32_t* erase_in, void* stage_a, void* stage_b, float* out, int64_t* labels_out, int32_t* params_out,
    int32_t* chain_out, int32_t* erase_out, void* stream) {
  return nbdt_resized_crop_policy_batch_sharded(src, src_dtype, labels_src, index, 0, B, N, H, W, S, flip, mean, std, scale,
                                                ratio, ratio_table, mode, nbins, table, num_ops, magnitude, subpolicies, P,
                                                erase_prob, erase_scale, erase_ratio, erase_ratio_table, seed, epoch,
                                                params_in, chain_in, erase_in, stage_a, stage_b, out, labels_out, params_out,
                                                chain_out, erase_out, stream);
}

// the whole dataset is the shard at base 0: the same kernels, the same bits
extern "C" int nbdt_resized_crop_batch(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index,
                                       int32_t B, int64_t N, int32_t H, int32_t W, int32_t rs_h, int32_t rs_w,
                                       int32_t win_top, int32_t win_left, int32_t out_h, int32_t out_w, int32_t flip,
                                       const float* mean, const float* std, const double* scale, const double* ratio,
                                       const double* ratio_table, uint64_t seed, uint64_t epoch, const int32_t* params_in,
                                       float* out, int64_t* labels_out, int32_t* params_out, void* stream) {
  return nbdt_resized_crop_batch_sharded(src, src_dtype, labels_src, index, 0, B, N, H, W, rs_h, rs_w, win_top, win_left,
                                         out_h, out_w, flip, mean, std, scale, ratio, ratio_table, seed, epoch, params_in,
                                         out, labels_out, params_out, stream);
}
