// Training-batch assembly with an augmentation policy, on the device: gather by index + RandomCrop(size, padding) +
// RandomHorizontalFlip + ONE TrivialAugmentWide operation on the uint8 image + ToTensor + Normalize + RandomErasing(value=0)
// in ONE launch, from a uint8 dataset that lives in device memory, into the fp32 NCHW tensor the stem kernels read.  The
// recipe of the TrivialAugment paper's CIFAR setup and of torchvision's ResNet reference (ta_wide + RandomErasing); the
// pixel rules are Pillow's, byte for byte (include/nbdt_hip.h states them, nbdt/data.py policy_reference restates them).
//
// One block per image.  The image's 3*H*W source bytes go to LDS with 16-byte loads (as in augment.hip); the cropped and
// flipped image is written to a second LDS tile T, which is what every operation reads: a geometric op is a gather from T
// through Pillow's 16.16 fixed-point affine coefficients, a colour op blends T with a degenerate image formed from T, the
// three histogram ops need per-image statistics first (the grey sum, per-channel min / max, per-channel 256-bin
// histogram), which one pass over T collects with INTEGER wave reductions and LDS atomics -- sums, minima and maxima of
// integers do not depend on the order, so the launch is bit-reproducible as it stands.  A lane then forms four consecutive x
// of one output row, applies the erase rectangle and the normalisation and writes one 16-byte store.
//
// The magnitudes come from a table the host builds in fp64 (nbdt/data.py policy_table): six int32 per (op, bin, sign), so
// there is no trigonometry and no magnitude arithmetic on the device.  Every value read from device memory (index, params,
// table) is clamped or bounds-checked before an address is formed from it.
//
// Built with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (nbdt/_build.py): the blend d + a * (x - d) is a
// separate fp32 multiply and add (Pillow's C), AutoContrast's v * scale + offset a separate fp64 multiply and add
// (Python's), and the normalisation is augment.hip's three IEEE operations.
#include "common.h"

using namespace nbdt;

// 3*H*W of the images this kernel takes: both tiles and the statistics stay far below the 160 KB of LDS
#define NBDT_AUGMENT_LDS_BYTES 49152

namespace {

enum {
  OP_IDENTITY, OP_SHEAR_X, OP_SHEAR_Y, OP_TRANSLATE_X, OP_TRANSLATE_Y, OP_ROTATE, OP_BRIGHTNESS, OP_COLOR, OP_CONTRAST,
  OP_SHARPNESS, OP_POSTERIZE, OP_SOLARIZE, OP_AUTOCONTRAST, OP_EQUALIZE
};

struct PolArgs {
  const unsigned char* src;
  const long long* labels_src;
  const long long* index;
  long long index_base, N;
  int H, W, pad, flip_on, policy_on;
  float mean[3], std[3];
  unsigned long long key;
  const signed char* params_in;      // int8 [B,3] (dy, dx, flip): replaces the crop / flip draw
  const int* policy_in;              // int32 [B,7] (op, bin, sign, top, left, h, w): replaces the policy and erase draw
  const int* table;                  // int32 [NBDT_POLICY_OPS][NBDT_POLICY_BINS][2][6] (device)
  double erase_p, s0, s1;            // erase probability and area-fraction range
  const double* ratio_table;         // NBDT_RESIZED_CROP_RATIOS log-spaced aspect ratios (device)
  int vec_in, vec_out;
  float* out;
  long long* labels_out;
  signed char* params_out;
  int* policy_out;
};

// the draw (include/nbdt_hip.h, nbdt/data.py): splitmix64's finaliser
__host__ __device__ inline unsigned long long mix64(unsigned long long x) {
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ float pick3(const float* v, int c) { return c == 0 ? v[0] : (c == 1 ? v[1] : v[2]); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// round-half-to-even of sqrt(v), 0 < v <= 2^30, decided by exact comparisons (resample.hip's): the result does not depend
// on how sqrt() itself is rounded
__device__ inline int round_sqrt(double v) {
  long long c = (long long)sqrt(v);
  if ((double)(c * c) > v) --c;
  if ((double)((c + 1) * (c + 1)) <= v) ++c;
  const double half = ((double)c + 0.5) * ((double)c + 0.5);
  if (v > half) return (int)c + 1;
  if (v < half) return (int)c;
  return (int)(c + (c & 1));
}

// torchvision's RandomErasing.get_params with the project's counter hash (nbdt/data.py draw_policy_params): the first
// attempt with h < H and w < W is taken; a side that rounded to 0 erases nothing
__device__ inline void draw_erase(const PolArgs& a, unsigned long long re, int& top, int& left, int& h, int& w) {
  top = left = h = w = 0;
  if (!((double)(re >> 11) * 0x1p-53 < a.erase_p)) return;
  const int H = a.H, W = a.W;
  const double area = (double)(H * W);
  for (int t = 0; t < NBDT_RESIZED_CROP_ATTEMPTS; ++t) {
    const unsigned long long ra = mix64(re + (unsigned long long)(2 * t + 1) * 0x9E3779B97F4A7C15ull);
    const unsigned long long rb = mix64(re + (unsigned long long)(2 * t + 2) * 0x9E3779B97F4A7C15ull);
    const double u = (double)(ra >> 11) * 0x1p-53;
    const double target = area * (a.s0 + u * (a.s1 - a.s0));
    const double rt = a.ratio_table[rb & (NBDT_RESIZED_CROP_RATIOS - 1)];
    const int ch = round_sqrt(target * rt), cw = round_sqrt(target / rt);
    if (ch < H && cw < W) {
      if (ch > 0 && cw > 0) {
        h = ch;
        w = cw;
        top = (int)((((rb >> 12) & 0xFFFFFFull) * (unsigned long long)(H - ch + 1)) >> 24);
        left = (int)((((rb >> 36) & 0xFFFFFFull) * (unsigned long long)(W - cw + 1)) >> 24);
      }
      return;
    }
  }
}

// integer reductions over the 64 lanes of a wave (every lane gets the result): order-independent, like the LDS atomics
// that combine the four waves
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
  return v;
}
__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = (unsigned)__shfl_xor((int)v, o);
    v = t < v ? t : v;
  }
  return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = (unsigned)__shfl_xor((int)v, o);
    v = t > v ? t : v;
  }
  return v;
}

__device__ __forceinline__ unsigned grey_of(unsigned r, unsigned g, unsigned b) {
  return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16;
}

// Pillow's Image.blend on 8-bit data: fp32, a separate multiply and add
__device__ __forceinline__ unsigned blend(unsigned d, unsigned x, float a) {
  const float fd = (float)d;
  const float t = fd + a * ((float)x - fd);
  return t <= 0.f ? 0u : (t >= 255.f ? 255u : (unsigned)(int)t);
}

// what an operation needs beyond the tile, block-uniform
struct OpCtx {
  int op;
  unsigned a[6];        // the table row: affine coefficients | factor bits | mask | threshold
  float factor;
  unsigned mean;        // Contrast: the grey mean
};

// the byte of output pixel (c, y, x) under the operation; T is the cropped and flipped image, lut the equalisation tables
// [3][256], ac AutoContrast's (scale, offset) per channel -- scale 0 for a channel that stays as it is
__device__ __forceinline__ unsigned op_pixel(const OpCtx& k, const unsigned char* T, const unsigned* lut, const double* ac,
                                              int H, int W, int c, int y, int x) {
  const int HW = H * W, p = y * W + x;
  switch (k.op) {
    case OP_SHEAR_X: case OP_SHEAR_Y: case OP_TRANSLATE_X: case OP_TRANSLATE_Y: case OP_ROTATE: {
      // (unsigned arithmetic: whatever the table holds wraps instead of overflowing; the result is bounds-checked)
      const int sx = (int)(k.a[2] + k.a[0] * (unsigned)x + k.a[1] * (unsigned)y) >> 16;
      const int sy = (int)(k.a[5] + k.a[3] * (unsigned)x + k.a[4] * (unsigned)y) >> 16;
      return (sx >= 0 && sx < W && sy >= 0 && sy < H) ? T[(c * H + sy) * W + sx] : 0u;
    }
    case OP_BRIGHTNESS: return blend(0u, T[c * HW + p], k.factor);
    case OP_COLOR: return blend(grey_of(T[p], T[HW + p], T[2 * HW + p]), T[c * HW + p], k.factor);
    case OP_CONTRAST: return blend(k.mean, T[c * HW + p], k.factor);
    case OP_SHARPNESS: {
      const unsigned char* q = T + c * HW + p;
      const unsigned v = q[0];
      if (x == 0 || y == 0 || x == W - 1 || y == H - 1) return v;        // ImageFilter.SMOOTH copies the border
      const unsigned s = q[-W - 1] + q[-W] + q[-W + 1] + q[-1] + 5u * v + q[1] + q[W - 1] + q[W] + q[W + 1];
      return blend((2u * s + 13u) / 26u, v, k.factor);                    // trunc(s / 13 + 0.5)
    }
    case OP_POSTERIZE: return T[c * HW + p] & k.a[0] & 0xFFu;
    case OP_SOLARIZE: {
      const int v = T[c * HW + p];
      return (unsigned)(v < (int)k.a[0] ? v : 255 - v);
    }
    case OP_AUTOCONTRAST: {
      const unsigned v = T[c * HW + p];
      const double scale = ac[2 * c], offset = ac[2 * c + 1];
      if (scale == 0.0) return v;          // hi <= lo
      return (unsigned)clampi((int)((double)v * scale + offset), 0, 255);
    }
    case OP_EQUALIZE: return lut[c * 256 + T[c * HW + p]] & 0xFFu;
    default: return T[c * HW + p];
  }
}

__global__ __launch_bounds__(256) void policy_kernel(const PolArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int H = a.H, W = a.W, pad = a.pad, HW = H * W, n = 3 * HW;
  const int npad = (n + 15) & ~15;
  unsigned char* S = lds;                                   // [3][H][W] the source image
  unsigned char* T = lds + npad;                            // [3][H][W] cropped and flipped
  unsigned* hist = (unsigned*)(lds + 2 * npad);             // [3][256] histogram, then prefix sums, then the LUT
  unsigned* stat = hist + 768;                              // [0] grey sum, [1..3] channel minima, [4..6] maxima
  double* ac = (double*)(stat + 8);                         // [3][2] AutoContrast's (scale, offset)
  const long long gidx = a.index[b];               // the dataset's index: what the draw hashes
  const unsigned long long idx = (unsigned long long)gidx - (unsigned long long)a.index_base;      // the row held here
  const bool valid = idx < (unsigned long long)a.N;
  float* o = a.out + (size_t)b * n;

  // ---- the sample's parameters (block-uniform; every lane computes them)
  int dy = 0, dx = 0, fl = 0, op = 0, bin = 0, sg = 0, et = 0, el = 0, eh = 0, ew = 0;
  if (valid) {
    if (a.params_in) {
      dy = clampi(a.params_in[b * 3], 0, 2 * pad);
      dx = clampi(a.params_in[b * 3 + 1], 0, 2 * pad);
      fl = a.params_in[b * 3 + 2] != 0;
    } else {
      const unsigned long long r = mix64(a.key ^ ((unsigned long long)gidx * 0xD1342543DE82EF95ull));
      const unsigned span = 2u * (unsigned)pad + 1u;
      dy = (int)((((unsigned)r & 0xFFFFFFu) * span) >> 24);
      dx = (int)((((unsigned)(r >> 24) & 0xFFFFFFu) * span) >> 24);
      fl = a.flip_on ? (int)(r >> 63) : 0;
    }
    if (a.policy_in) {
      const int* q = a.policy_in + (size_t)b * 7;
      op = clampi(q[0], 0, NBDT_POLICY_OPS - 1);
      bin = clampi(q[1], 0, NBDT_POLICY_BINS - 1);
      sg = q[2] != 0;
      et = clampi(q[3], 0, H - 1);
      el = clampi(q[4], 0, W - 1);
      eh = clampi(q[5], 0, H - et);
      ew = clampi(q[6], 0, W - el);
      if (eh == 0 || ew == 0) et = el = eh = ew = 0;
    } else {
      if (a.policy_on) {
        const unsigned long long rp = mix64(a.key ^ ((unsigned long long)gidx * 0xA0761D6478BD642Full));
        op = (int)((((unsigned)rp & 0xFFFFFFu) * (unsigned)NBDT_POLICY_OPS) >> 24);
        bin = (int)((((unsigned)(rp >> 24) & 0xFFFFFFu) * (unsigned)NBDT_POLICY_BINS) >> 24);
        sg = (int)(rp >> 63);
      }
      draw_erase(a, mix64(a.key ^ ((unsigned long long)gidx * 0xE7037ED1A0B428DBull)), et, el, eh, ew);
    }
  }
  if (tid == 0) {
    a.labels_out[b] = valid ? a.labels_src[idx] : -1ll;
    if (a.params_out) {
      a.params_out[b * 3] = (signed char)dy;
      a.params_out[b * 3 + 1] = (signed char)dx;
      a.params_out[b * 3 + 2] = (signed char)fl;
    }
    if (a.policy_out) {
      int* q = a.policy_out + (size_t)b * 7;
      q[0] = op; q[1] = bin; q[2] = sg; q[3] = et; q[4] = el; q[5] = eh; q[6] = ew;
    }
  }
  if (!valid) {      // (block-uniform) an index the host could not check: a zero image, label -1, no source address formed
    for (int i = tid; i < n; i += 256) o[i] = 0.f;
    return;
  }

  // ---- stage the source, then crop and flip it into T
  const unsigned char* s8 = a.src + (size_t)idx * n;
  if (a.vec_in)
    for (int i = tid; i < (n >> 4); i += 256) ((u32x4_t*)S)[i] = ((const u32x4_t*)s8)[i];
  else
    for (int i = tid; i < n; i += 256) S[i] = s8[i];
  for (int i = tid; i < 776; i += 256) hist[i] = (i >= 769 && i <= 771) ? 255u : 0u;
  __syncthreads();
  const int G = (W + 3) >> 2;            // groups of four x per row
  const int items = 3 * H * G;
  for (int it = tid; it < items; it += 256) {
    const int row = it / G, g = it - row * G;     // row = c * H + y
    const int c = row / H, y = row - c * H;
    const int sy = y + dy - pad;
    const bool yin = sy >= 0 && sy < H;
    unsigned u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = g * 4 + j;
      const int sx = (fl ? W - 1 - x : x) + dx - pad;
      u[j] = (yin && x < W && sx >= 0 && sx < W) ? S[(c * H + sy) * W + sx] : 0u;
    }
    unsigned char* dst = T + row * W + g * 4;
    if ((W & 3) == 0) {                  // (T and the row pitch are multiples of four bytes)
      *(unsigned*)dst = u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (g * 4 + j < W) dst[j] = (unsigned char)u[j];
    }
  }
  __syncthreads();

  // ---- the operation's constants and per-image statistics (op is block-uniform: so is every barrier below)
  OpCtx k = {};
  k.op = op;
  {
    const int* row = a.table ? a.table + (size_t)(((op * NBDT_POLICY_BINS + bin) * 2 + sg) * 6) : nullptr;
#pragma unroll
    for (int i = 0; i < 6; ++i) k.a[i] = row ? (unsigned)row[i] : 0u;
    k.factor = __uint_as_float(k.a[0]);
  }
  if (op == OP_CONTRAST) {
    unsigned sum = 0;
    for (int p = tid; p < HW; p += 256) sum += grey_of(T[p], T[HW + p], T[2 * HW + p]);
    sum = wave_sum(sum);
    if ((tid & 63) == 0) atomicAdd(&stat[0], sum);            // at most 255 * 16384: no overflow
    __syncthreads();
    k.mean = (2u * stat[0] + (unsigned)HW) / (2u * (unsigned)HW);         // int(sum / HW + 0.5)
  } else if (op == OP_AUTOCONTRAST || op == OP_EQUALIZE) {
    for (int c = 0; c < 3; ++c) {
      unsigned lo = 255u, hi = 0u;
      for (int p = tid; p < HW; p += 256) {
        const unsigned v = T[c * HW + p];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
        if (op == OP_EQUALIZE) atomicAdd(&hist[c * 256 + v], 1u);
      }
      lo = wave_min(lo);
      hi = wave_max(hi);
      if ((tid & 63) == 0) {             // one atomic per wave and address, not 64 contending ones
        atomicMin(&stat[1 + c], lo);
        atomicMax(&stat[4 + c], hi);
      }
    }
    __syncthreads();
    if (op == OP_AUTOCONTRAST) {
      if (tid < 3) {
        const int lo = (int)stat[1 + tid], hi = (int)stat[4 + tid];
        const double scale = hi > lo ? 255.0 / (double)(hi - lo) : 0.0;
        ac[2 * tid] = scale;
        ac[2 * tid + 1] = -(double)lo * scale;
      }
      __syncthreads();
    } else {
      // ImageOps.equalize: lut[i] = min(255, (step / 2 + sum of h[j], j < i) / step), step = (H*W - h[last non-empty]) / 255
      unsigned own[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) own[c] = hist[c * 256 + tid];
      for (int off = 1; off < 256; off <<= 1) {            // inclusive prefix sums, all three channels at once
        unsigned add[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) add[c] = tid >= off ? hist[c * 256 + tid - off] : 0u;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) hist[c * 256 + tid] += add[c];
        __syncthreads();
      }
      unsigned lutv[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        lutv[c] = (unsigned)tid;
        const int lo = (int)stat[1 + c], hi = (int)stat[4 + c];
        if (hi > lo) {                    // (then hi >= 1) more than one non-empty bin
          const unsigned last = hist[c * 256 + hi] - hist[c * 256 + hi - 1];
          const unsigned step = ((unsigned)HW - last) / 255u;
          if (step != 0u) {
            const unsigned q = (step / 2u + hist[c * 256 + tid] - own[c]) / step;
            lutv[c] = q > 255u ? 255u : q;
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 3; ++c) hist[c * 256 + tid] = lutv[c];
      __syncthreads();
    }
  }

  // ---- the output: four consecutive x of one row per lane
  for (int it = tid; it < items; it += 256) {
    const int row = it / G, g = it - row * G;     // row = c * H + y
    const int c = row / H, y = row - c * H;
    const float mean = pick3(a.mean, c), sd = pick3(a.std, c);
    const bool yer = y >= et && y < et + eh;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = g * 4 + j;
      v[j] = 0.f;
      if (x < W && !(yer && x >= el && x < el + ew)) {
        const unsigned u = op_pixel(k, T, hist, ac, H, W, c, y, x);
        v[j] = ((float)u / 255.0f - mean) / sd;
      }
    }
    float* dst = o + (size_t)row * W + g * 4;
    if (a.vec_out) {
      *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (g * 4 + j < W) dst[j] = v[j];
    }
  }
}

}  // namespace

extern "C" int nbdt_policy_batch_sharded(const void* src, int32_t src_dtype, const int64_t* labels_src,
                                         const int64_t* index, int64_t index_base, int32_t B, int64_t N, int32_t H,
                                         int32_t W, int32_t pad, int32_t flip, const float* mean, const float* std,
                                         int32_t policy, const int32_t* policy_table, double erase_prob,
                                         const double* erase_scale, const double* erase_ratio, const double* ratio_table,
                                         uint64_t seed, uint64_t epoch, const int8_t* params_in, const int32_t* policy_in,
                                         float* out, int64_t* labels_out, int8_t* params_out, int32_t* policy_out,
                                         void* stream) {
  NBDT_REQUIRE(src && labels_src && index && out && labels_out, "null argument");
  NBDT_REQUIRE(N <= 0 || (index_base >= 0 && index_base <= INT64_MAX - N),
               "index_base must be >= 0 and index_base + N must fit int64");
  NBDT_REQUIRE(src_dtype == NBDT_U8, "the policy works on bytes: the dataset must be uint8 (NBDT_U8)");
  NBDT_REQUIRE(B > 0, "empty batch");
  NBDT_REQUIRE(N > 0, "empty dataset");
  NBDT_REQUIRE(H > 0 && W > 0 && H <= 4096 && W <= 4096, "image sides must be 1..4096");
  NBDT_REQUIRE((long long)H * W * 3 <= NBDT_AUGMENT_LDS_BYTES,
               "the policy kernel stages the image in LDS: 3*H*W must be at most 49152 bytes (128 x 128)");
  NBDT_REQUIRE(pad >= 0 && pad <= NBDT_AUGMENT_MAX_PAD, "pad must be 0..NBDT_AUGMENT_MAX_PAD");
  NBDT_REQUIRE(flip == 0 || flip == 1, "flip is 0 or 1");
  NBDT_REQUIRE(mean && std, "a uint8 dataset needs mean[3] and std[3]");
  NBDT_REQUIRE(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "std must be non-zero");
  NBDT_REQUIRE(policy == NBDT_POLICY_NONE || policy == NBDT_POLICY_TA_WIDE, "policy is NBDT_POLICY_NONE or NBDT_POLICY_TA_WIDE");
  NBDT_REQUIRE(policy_table || (policy == NBDT_POLICY_NONE && !policy_in),
               "a policy (or policy_in) needs the policy table");
  NBDT_REQUIRE(erase_prob >= 0.0 && erase_prob <= 1.0, "erase_prob must be in [0, 1]");       // (NaN fails both)
  PolArgs a = {};
  if (erase_prob > 0.0 && !policy_in) {
    NBDT_REQUIRE(erase_scale && erase_ratio && ratio_table,
                 "the erase draw needs erase_scale[2], erase_ratio[2] and the ratio table");
    NBDT_REQUIRE(erase_scale[0] > 0.0 && erase_scale[0] <= erase_scale[1] && erase_scale[1] <= 1.0,
                 "erase_scale must satisfy 0 < lo <= hi <= 1");
    NBDT_REQUIRE(erase_ratio[0] >= 1.0 / 64.0 && erase_ratio[0] <= erase_ratio[1] && erase_ratio[1] <= 64.0,
                 "erase_ratio must satisfy 1/64 <= lo <= hi <= 64");
    a.erase_p = erase_prob;
    a.s0 = erase_scale[0];
    a.s1 = erase_scale[1];
    a.ratio_table = ratio_table;
  }
  a.src = (const unsigned char*)src;
  a.labels_src = (const long long*)labels_src;
  a.index = (const long long*)index;
  a.index_base = index_base;
  a.N = N;
  a.H = H; a.W = W; a.pad = pad; a.flip_on = flip; a.policy_on = policy == NBDT_POLICY_TA_WIDE;
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.std[c] = std[c]; }
  a.key = mix64((unsigned long long)seed * 0x9E3779B97F4A7C15ull + (unsigned long long)epoch);
  a.params_in = (const signed char*)params_in;
  a.policy_in = policy_in;
  a.table = policy_table;
  const int n = 3 * H * W;
  a.vec_in = (n % 16 == 0 && (uintptr_t)src % 16 == 0) ? 1 : 0;
  a.vec_out = (W % 4 == 0 && (uintptr_t)out % 16 == 0) ? 1 : 0;
  a.out = out;
  a.labels_out = (long long*)labels_out;
  a.params_out = (signed char*)params_out;
  a.policy_out = policy_out;
  const size_t shmem = (size_t)2 * ((n + 15) & ~15) + 776 * sizeof(unsigned) + 6 * sizeof(double);
  static DeviceAttr site;
  if (shmem > 65536 && site.need(shmem)) {      // (up to 64 KB needs no attribute)
    NBDT_ATTR_CHECK(site, hipFuncSetAttribute(reinterpret_cast<const void*>(&policy_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    site.done(shmem);
  }
  hipLaunchKernelGGL(policy_kernel, dim3(B), dim3(256), shmem, (hipStream_t)stream, a);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

// the whole dataset is the shard at base 0: the same kernel, the same bits
extern "C" int nbdt_policy_batch(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index,
                                 int32_t B, int64_t N, int32_t H, int32_t W, int32_t pad, int32_t flip, const float* mean,
                                 const float* std, int32_t policy, const int32_t* policy_table, double erase_prob,
                                 const double* erase_scale, const double* erase_ratio, const double* ratio_table,
                                 uint64_t seed, uint64_t epoch, const int8_t* params_in, const int32_t* policy_in,
                                 float* out, int64_t* labels_out, int8_t* params_out, int32_t* policy_out, void* stream) {
  return nbdt_policy_batch_sharded(src, src_dtype, labels_src, index, 0, B, N, H, W, pad, flip, mean, std, policy,
                                   policy_table, erase_prob, erase_scale, erase_ratio, ratio_table, seed, epoch, params_in,
                                   policy_in, out, labels_out, params_out, policy_out, stream);
}
