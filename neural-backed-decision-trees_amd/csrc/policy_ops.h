// The rules of the augmentation policies, shared by the kernels that apply them: policy.hip (the padded-crop path, both
// tiles in LDS, 256 lanes) and resample.hip (the resized-crop path, both tiles in global memory, a wider block).  The draw
// of the chain and of the erase rectangle, the per-image statistics, the per-pixel rule of each of the 15 operations, the
// byte pass from one tile into the other, the normalising output pass, the loop that runs a chain through them (run_chain),
// a sample's parameters (ChainSpec, chain_params, store_chain_params) and the host checks that fill them.  Pillow's pixel
// rules, byte for byte (include/nbdt_hip.h states them, nbdt/data.py policy_reference / chain_reference restate them).
//
// A tile is a plain `unsigned char*`: after inlining the compiler knows whether it is LDS or global.  BLOCK is the number of
// lanes of the block (a multiple of 64, at least 256: Equalize's prefix sums give every bin a lane).  Every statistic is an
// integer sum, minimum or maximum, so neither BLOCK nor the order of the lanes changes a bit of the result.
//
// Both translation units are built with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (nbdt/_build.py): the
// blend d + a * (x - d) is a separate fp32 multiply and add (Pillow's C), AutoContrast's v * scale + offset a separate fp64
// multiply and add (Python's), and the normalisation is augment.hip's three IEEE operations.
#pragma once
#include "common.h"

namespace nbdt {
namespace pol {

enum {
  OP_IDENTITY, OP_SHEAR_X, OP_SHEAR_Y, OP_TRANSLATE_X, OP_TRANSLATE_Y, OP_ROTATE, OP_BRIGHTNESS, OP_COLOR, OP_CONTRAST,
  OP_SHARPNESS, OP_POSTERIZE, OP_SOLARIZE, OP_AUTOCONTRAST, OP_EQUALIZE,
  OP_INVERT          // the policy chains' 15th operation (NBDT_CHAIN_OPS): policy_kernel clamps its op to 0..13
};

// words of the per-image statistics: hist[3][256], then stat[8] = grey sum, three minima, three maxima, one spare
constexpr int kStatWords = 776;

// the draw (include/nbdt_hip.h, nbdt/data.py): splitmix64's finaliser
__host__ __device__ inline unsigned long long mix64(unsigned long long x) {
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ float pick3(const float* v, int c) { return c == 0 ? v[0] : (c == 1 ? v[1] : v[2]); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// round-half-to-even of sqrt(v), 0 < v <= 2^30 (4096^2 pixels x ratio 64), decided by exact comparisons: c * c and
// (c + 1/2)^2 are exact in fp64 for c < 2^25, so the result does not depend on how sqrt() itself is rounded
__device__ inline int round_sqrt(double v) {
  long long c = (long long)sqrt(v);
  if ((double)(c * c) > v) --c;
  if ((double)((c + 1) * (c + 1)) <= v) ++c;
  const double half = ((double)c + 0.5) * ((double)c + 0.5);
  if (v > half) return (int)c + 1;
  if (v < half) return (int)c;
  return (int)(c + (c & 1));
}

// what the erase draw needs beyond the image's sides
struct EraseDraw {
  double p, s0, s1;                  // erase probability and area-fraction range
  const double* ratio_table;         // NBDT_RESIZED_CROP_RATIOS log-spaced aspect ratios (device)
};

// torchvision's RandomErasing.get_params with the project's counter hash (nbdt/data.py draw_policy_params): the first
// attempt with h < H and w < W is taken; a side that rounded to 0 erases nothing
__device__ inline void draw_erase(const EraseDraw& e, int H, int W, unsigned long long re, int& top, int& left, int& h,
                                  int& w) {
  top = left = h = w = 0;
  if (!((double)(re >> 11) * 0x1p-53 < e.p)) return;
  const double area = (double)(H * W);
  for (int t = 0; t < NBDT_RESIZED_CROP_ATTEMPTS; ++t) {
    const unsigned long long ra = mix64(re + (unsigned long long)(2 * t + 1) * 0x9E3779B97F4A7C15ull);
    const unsigned long long rb = mix64(re + (unsigned long long)(2 * t + 2) * 0x9E3779B97F4A7C15ull);
    const double u = (double)(ra >> 11) * 0x1p-53;
    const double target = area * (e.s0 + u * (e.s1 - e.s0));
    const double rt = e.ratio_table[rb & (NBDT_RESIZED_CROP_RATIOS - 1)];
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

// the erase rectangle of sample `gidx`: its own word of the hash, the same under every policy setting
__device__ __forceinline__ unsigned long long erase_word(unsigned long long key, long long gidx) {
  return mix64(key ^ ((unsigned long long)gidx * 0xE7037ED1A0B428DBull));
}

// a rectangle read from device memory (top, left, h, w), clamped into the image; an empty one is all zeros
__device__ __forceinline__ void clamp_erase(const int* q, int H, int W, int& et, int& el, int& eh, int& ew) {
  et = clampi(q[0], 0, H - 1);
  el = clampi(q[1], 0, W - 1);
  eh = clampi(q[2], 0, H - et);
  ew = clampi(q[3], 0, W - el);
  if (eh == 0 || ew == 0) et = el = eh = ew = 0;
}

// integer reductions over the 64 lanes of a wave (every lane gets the result): order-independent, like the LDS atomics
// that combine the waves
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

// an operation whose output byte depends on the input byte at the same place and channel only (Identity included)
__device__ __forceinline__ bool op_is_point(int op) {
  return op == OP_IDENTITY || op == OP_BRIGHTNESS || op == OP_CONTRAST || op >= OP_POSTERIZE;
}

// the byte a point operation makes of the byte v of channel c; lut the equalisation tables [3][256], ac AutoContrast's
// (scale, offset) per channel -- scale 0 for a channel that stays as it is
__device__ __forceinline__ unsigned op_value(const OpCtx& k, const unsigned* lut, const double* ac, int c, unsigned v) {
  switch (k.op) {
    case OP_BRIGHTNESS: return blend(0u, v, k.factor);
    case OP_CONTRAST: return blend(k.mean, v, k.factor);
    case OP_POSTERIZE: return v & k.a[0] & 0xFFu;
    case OP_SOLARIZE: return (unsigned)((int)v < (int)k.a[0] ? (int)v : 255 - (int)v);
    case OP_AUTOCONTRAST: {
      const double scale = ac[2 * c], offset = ac[2 * c + 1];
      if (scale == 0.0) return v;          // hi <= lo
      return (unsigned)clampi((int)((double)v * scale + offset), 0, 255);
    }
    case OP_EQUALIZE: return lut[c * 256 + v] & 0xFFu;
    case OP_INVERT: return 255u - v;
    default: return v;
  }
}

// the byte of output pixel (c, y, x) under the operation; T is the image so far
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
    case OP_COLOR: return blend(grey_of(T[p], T[HW + p], T[2 * HW + p]), T[c * HW + p], k.factor);
    case OP_SHARPNESS: {
      const unsigned char* q = T + c * HW + p;
      const unsigned v = q[0];
      if (x == 0 || y == 0 || x == W - 1 || y == H - 1) return v;        // ImageFilter.SMOOTH copies the border
      const unsigned s = q[-W - 1] + q[-W] + q[-W + 1] + q[-1] + 5u * v + q[1] + q[W - 1] + q[W] + q[W + 1];
      return blend((2u * s + 13u) / 26u, v, k.factor);                    // trunc(s / 13 + 0.5)
    }
    default: return op_value(k, lut, ac, c, T[c * HW + p]);
  }
}

// hist / stat back to their initial values (zeros, minima 255); the caller puts a barrier on both sides
template <int BLOCK>
__device__ __forceinline__ void reset_statistics(unsigned* hist, int tid) {
  for (int i = tid; i < kStatWords; i += BLOCK) hist[i] = (i >= 769 && i <= 771) ? 255u : 0u;
}

// the per-image statistics an operation needs, collected over the tile T (block-uniform in k.op: so is every barrier):
// Contrast's grey mean into k.mean, AutoContrast's (scale, offset) into ac, Equalize's tables into hist.  hist / stat
// (= hist + 768) must hold their initial values and a barrier must lie between that and this call.  The grey sum and its
// rounding are formed in 32 bits: 2 * 255 * HW + HW < 2^32 needs HW <= 8.4e6; the entries hold HW far below it.
template <int BLOCK>
__device__ __forceinline__ void op_statistics(OpCtx& k, const unsigned char* T, unsigned* hist, unsigned* stat, double* ac,
                                               int HW, int tid) {
  static_assert(BLOCK >= 256 && BLOCK % 64 == 0, "every histogram bin needs a lane; whole waves");
  const int op = k.op;
  if (op == OP_CONTRAST) {
    unsigned sum = 0;
    for (int p = tid; p < HW; p += BLOCK) sum += grey_of(T[p], T[HW + p], T[2 * HW + p]);
    sum = wave_sum(sum);
    if ((tid & 63) == 0) atomicAdd(&stat[0], sum);
    __syncthreads();
    k.mean = (2u * stat[0] + (unsigned)HW) / (2u * (unsigned)HW);         // int(sum / HW + 0.5)
  } else if (op == OP_AUTOCONTRAST || op == OP_EQUALIZE) {
    for (int c = 0; c < 3; ++c) {
      unsigned lo = 255u, hi = 0u;
      for (int p = tid; p < HW; p += BLOCK) {
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
      const bool bin = BLOCK == 256 || tid < 256;          // the lanes that own a bin; the barriers are everybody's
      const int t = bin ? tid : 0;
      unsigned own[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) own[c] = hist[c * 256 + t];
      for (int off = 1; off < 256; off <<= 1) {            // inclusive prefix sums, all three channels at once
        unsigned add[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) add[c] = t >= off ? hist[c * 256 + t - off] : 0u;
        __syncthreads();
        if (bin) {
#pragma unroll
          for (int c = 0; c < 3; ++c) hist[c * 256 + t] += add[c];
        }
        __syncthreads();
      }
      unsigned lutv[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        lutv[c] = (unsigned)t;
        const int lo = (int)stat[1 + c], hi = (int)stat[4 + c];
        if (hi > lo) {                    // (then hi >= 1) more than one non-empty bin
          const unsigned last = hist[c * 256 + hi] - hist[c * 256 + hi - 1];
          const unsigned step = ((unsigned)HW - last) / 255u;
          if (step != 0u) {
            const unsigned q = (step / 2u + hist[c * 256 + t] - own[c]) / step;
            lutv[c] = q > 255u ? 255u : q;
          }
        }
      }
      __syncthreads();
      if (bin) {
#pragma unroll
        for (int c = 0; c < 3; ++c) hist[c * 256 + t] = lutv[c];
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ bool op_needs_statistics(int op) {
  return op == OP_CONTRAST || op == OP_AUTOCONTRAST || op == OP_EQUALIZE;
}

// ---- the chain: 16 bits per slot, op | bin << 4 | sign << 9 (all zero: Identity)
__device__ __forceinline__ unsigned long long pack_slot(int op, int bin, int sg) {
  return (unsigned long long)(unsigned)(op | (bin << 4) | (sg << 9));
}

__device__ __forceinline__ void load_op(OpCtx& k, const int* table, int nbins, int op, int bin, int sg) {
  const int* row = table + (size_t)(((op * nbins + bin) * 2 + sg) * 6);
  k.op = op;
#pragma unroll
  for (int i = 0; i < 6; ++i) k.a[i] = (unsigned)row[i];
  k.factor = __uint_as_float(k.a[0]);
  k.mean = 0u;
}

// slot s of a packed chain into k (the slot is a run-time shift); returns its op
__device__ __forceinline__ int load_slot(OpCtx& k, const int* table, int nbins, unsigned long long chain, int s) {
  const unsigned w = (unsigned)(chain >> (16 * s));
  const int op = (int)(w & 15u);
  if (op != OP_IDENTITY) load_op(k, table, nbins, op, (int)((w >> 4) & 31u), (int)((w >> 9) & 1u));
  return op;
}

// the last slot that is not Identity, -1 if there is none
__device__ __forceinline__ int last_slot(unsigned long long chain) {
  int last = -1;
#pragma unroll
  for (int s = 0; s < NBDT_CHAIN_MAX_OPS; ++s)
    if ((chain >> (16 * s)) & 15ull) last = s;
  return last;
}

// a chain read from device memory, int32 [NBDT_CHAIN_MAX_OPS][3] (op, bin, sign): clamped, never trusted
__device__ __forceinline__ unsigned long long clamp_chain(const int* q, int nbins) {
  unsigned long long chain = 0;
#pragma unroll
  for (int s = 0; s < NBDT_CHAIN_MAX_OPS; ++s) {
    chain |= pack_slot(clampi(q[3 * s], 0, NBDT_CHAIN_OPS - 1), clampi(q[3 * s + 1], 0, nbins - 1), q[3 * s + 2] != 0)
             << (16 * s);
  }
  return chain;
}

__device__ __forceinline__ void store_chain(int* q, unsigned long long chain) {
#pragma unroll
  for (int s = 0; s < NBDT_CHAIN_MAX_OPS; ++s) {
    const unsigned w = (unsigned)(chain >> (16 * s));
    q[3 * s] = (int)(w & 15u); q[3 * s + 1] = (int)((w >> 4) & 31u); q[3 * s + 2] = (int)((w >> 9) & 1u);
  }
}

// the chain's draw for sample `gidx` (include/nbdt_hip.h, nbdt/data.py draw_chain_params / draw_policy_params).
// NBDT_CHAIN_RAND: num_ops slots, each an op of RandAugment's space at bin `magnitude` with a fresh sign.
// NBDT_CHAIN_SUBPOLICY: one of the P sub-policies int32 [P][NBDT_CHAIN_MAX_OPS][3] (op, q, bin), device memory: clamped.
// NBDT_CHAIN_TA_WIDE: one slot, nbdt_policy_batch's (op, bin, sign) -- the callers hold nbins at NBDT_POLICY_BINS for it.
__device__ __forceinline__ unsigned long long draw_chain(unsigned long long key, long long gidx, int mode, int nbins,
                                                         int num_ops, int magnitude, const int* subpolicies, int P) {
  unsigned long long chain = 0;
  if (mode == NBDT_CHAIN_TA_WIDE) {
    const unsigned long long rp = mix64(key ^ ((unsigned long long)gidx * 0xA0761D6478BD642Full));
    return pack_slot((int)((((unsigned)rp & 0xFFFFFFu) * (unsigned)NBDT_POLICY_OPS) >> 24),
                     (int)((((unsigned)(rp >> 24) & 0xFFFFFFu) * (unsigned)NBDT_POLICY_BINS) >> 24), (int)(rp >> 63));
  }
  const unsigned long long rc = mix64(key ^ ((unsigned long long)gidx * 0x8EBC6AF09C88C6E3ull));
  const int* sub = nullptr;
  int slots = num_ops;
  if (mode == NBDT_CHAIN_SUBPOLICY) {
    sub = subpolicies + (size_t)(((rc & 0xFFFFFFull) * (unsigned long long)P) >> 24) * (NBDT_CHAIN_MAX_OPS * 3);
    slots = NBDT_CHAIN_MAX_OPS;
  }
#pragma unroll
  for (int s = 0; s < NBDT_CHAIN_MAX_OPS; ++s) {
    if (s >= slots) continue;
    const unsigned long long rs = mix64(rc + (unsigned long long)(s + 1) * 0x9E3779B97F4A7C15ull);
    if (sub) {
      // applied when the 24-bit uniform lies below q = round(p * 2^24); negative magnitude when the sign bit is 0
      if ((int)((unsigned)rs & 0xFFFFFFu) < clampi(sub[3 * s + 1], 0, 1 << 24))
        chain |= pack_slot(clampi(sub[3 * s], 0, NBDT_CHAIN_OPS - 1), clampi(sub[3 * s + 2], 0, nbins - 1),
                           (int)(rs >> 63) ^ 1) << (16 * s);
    } else {          // (Invert is not in RandAugment's space)
      chain |= pack_slot((int)((((unsigned)rs & 0xFFFFFFu) * (unsigned)NBDT_POLICY_OPS) >> 24), magnitude,
                         (int)(rs >> 63)) << (16 * s);
    }
  }
  return chain;
}

// ---- what a chain launch needs beyond its tiles: how a sample's chain and erase rectangle are drawn or read, and where
// what was used is reported.  The host checks below fill it; ChainArgs (policy.hip) and RcpArgs (resample.hip) embed it.
struct ChainSpec {
  int mode, nbins, num_ops, magnitude, P;
  const int* table;                  // int32 [NBDT_CHAIN_OPS][nbins][2][6] (device); [NBDT_POLICY_OPS][31][2][6] indexes alike
  const int* subpolicies;            // int32 [P][NBDT_CHAIN_MAX_OPS][3] (op, q, bin), device: clamped by draw_chain
  const int* chain_in;               // int32 [B][NBDT_CHAIN_MAX_OPS][3] (op, bin, sign): replaces the chain's draw
  const int* erase_in;               // int32 [B][4] (top, left, h, w): replaces the erase draw
  int* chain_out;
  int* erase_out;
  EraseDraw erase;                   // erase probability, area-fraction range and the aspect-ratio table
};

// the chain and the erase rectangle of sample b (dataset index gidx) of an H x W image: read from device memory and
// clamped, or drawn; an invalid index gets the chain of none and no rectangle.  Block-uniform; every lane computes it.
__device__ __forceinline__ void chain_params(const ChainSpec& c, unsigned long long key, long long gidx, int b, int H, int W,
                                               bool valid, unsigned long long& chain, int& et, int& el, int& eh, int& ew) {
  chain = 0;                         // 16 bits per slot: op | bin << 4 | sign << 9 (all zero: Identity)
  et = el = eh = ew = 0;
  if (!valid) return;
  if (c.chain_in)
    chain = clamp_chain(c.chain_in + (size_t)b * (NBDT_CHAIN_MAX_OPS * 3), c.nbins);
  else
    chain = draw_chain(key, gidx, c.mode, c.nbins, c.num_ops, c.magnitude, c.subpolicies, c.P);
  if (c.erase_in)
    clamp_erase(c.erase_in + (size_t)b * 4, H, W, et, el, eh, ew);
  else
    draw_erase(c.erase, H, W, erase_word(key, gidx), et, el, eh, ew);
}

// what sample b used, into the outputs that were asked for (one lane calls this)
__device__ __forceinline__ void store_chain_params(const ChainSpec& c, int b, unsigned long long chain, int et, int el, int eh,
                                              int ew) {
  if (c.chain_out) store_chain(c.chain_out + (size_t)b * (NBDT_CHAIN_MAX_OPS * 3), chain);
  if (c.erase_out) {
    int* q = c.erase_out + (size_t)b * 4;
    q[0] = et; q[1] = el; q[2] = eh; q[3] = ew;
  }
}

// the mode and its arguments into c, as both chain entries check them.  zero_ops: NBDT_CHAIN_RAND may have no slot (the
// erase alone), and then, without chain_in, no table; ta_wide: NBDT_CHAIN_TA_WIDE is a mode of this entry.
inline int check_chain(ChainSpec& c, int32_t mode, int32_t nbins, const int32_t* table, int32_t num_ops, int32_t magnitude,
                       const int32_t* subpolicies, int32_t P, const int32_t* chain_in, bool zero_ops, bool ta_wide) {
  if (ta_wide)
    NBDT_REQUIRE(mode == NBDT_CHAIN_RAND || mode == NBDT_CHAIN_SUBPOLICY || mode == NBDT_CHAIN_TA_WIDE,
                 "mode is NBDT_CHAIN_RAND, NBDT_CHAIN_SUBPOLICY or NBDT_CHAIN_TA_WIDE");
  else
    NBDT_REQUIRE(mode == NBDT_CHAIN_RAND || mode == NBDT_CHAIN_SUBPOLICY, "mode is NBDT_CHAIN_RAND or NBDT_CHAIN_SUBPOLICY");
  NBDT_REQUIRE(nbins >= 1 && nbins <= NBDT_CHAIN_MAX_BINS, "nbins must be 1..NBDT_CHAIN_MAX_BINS");
  if (!zero_ops) NBDT_REQUIRE(table, "null argument: the chain needs its magnitude table");      // (each entry's own order)
  if (mode == NBDT_CHAIN_RAND) {
    if (zero_ops)
      NBDT_REQUIRE(num_ops >= 0 && num_ops <= NBDT_CHAIN_MAX_OPS, "num_ops must be 0..NBDT_CHAIN_MAX_OPS");
    else
      NBDT_REQUIRE(num_ops >= 1 && num_ops <= NBDT_CHAIN_MAX_OPS, "num_ops must be 1..NBDT_CHAIN_MAX_OPS");
    NBDT_REQUIRE(magnitude >= 0 && magnitude < nbins, "magnitude must be a bin: 0 <= magnitude < nbins");
    c.num_ops = num_ops;
    c.magnitude = magnitude;
  } else if (mode == NBDT_CHAIN_SUBPOLICY) {
    NBDT_REQUIRE(subpolicies, "null argument: NBDT_CHAIN_SUBPOLICY needs the sub-policies");
    NBDT_REQUIRE(P >= 1 && P <= NBDT_CHAIN_MAX_SUBPOLICIES, "P (the number of sub-policies) must be 1..NBDT_CHAIN_MAX_SUBPOLICIES");
    c.subpolicies = subpolicies;
    c.P = P;
  } else {
    NBDT_REQUIRE(nbins == NBDT_POLICY_BINS, "NBDT_CHAIN_TA_WIDE draws among NBDT_POLICY_BINS bins: nbins must be 31");
  }
  if (zero_ops)
    NBDT_REQUIRE(table || (mode == NBDT_CHAIN_RAND && num_ops == 0 && !chain_in),
                 "null argument: the chain needs its magnitude table");
  c.mode = mode;
  c.nbins = nbins;
  c.table = table;
  c.chain_in = chain_in;
  return NBDT_OK;
}

// erase_prob, and what the erase draw needs when it is made (`drawn`: no rectangle is given), into c.erase
inline int check_erase(ChainSpec& c, double erase_prob, const double* erase_scale, const double* erase_ratio,
                       const double* ratio_table, bool drawn) {
  NBDT_REQUIRE(erase_prob >= 0.0 && erase_prob <= 1.0, "erase_prob must be in [0, 1]");       // (NaN fails both)
  if (erase_prob > 0.0 && drawn) {
    NBDT_REQUIRE(erase_scale && erase_ratio && ratio_table,
                 "the erase draw needs erase_scale[2], erase_ratio[2] and the ratio table");
    NBDT_REQUIRE(erase_scale[0] > 0.0 && erase_scale[0] <= erase_scale[1] && erase_scale[1] <= 1.0,
                 "erase_scale must satisfy 0 < lo <= hi <= 1");
    NBDT_REQUIRE(erase_ratio[0] >= 1.0 / 64.0 && erase_ratio[0] <= erase_ratio[1] && erase_ratio[1] <= 64.0,
                 "erase_ratio must satisfy 1/64 <= lo <= hi <= 64");
    c.erase.p = erase_prob;
    c.erase.s0 = erase_scale[0];
    c.erase.s1 = erase_scale[1];
    c.erase.ratio_table = ratio_table;
  }
  return NBDT_OK;
}

// ---- the two passes over a tile; four consecutive x of one row per lane.  WORD: the tiles and the row pitch are
// multiples of four bytes (the caller has checked it) and a point operation reads its four bytes with one load.

// operation k on the tile `cur` into the tile `oth`
template <int BLOCK, bool WORD>
__device__ __forceinline__ void byte_pass(const OpCtx& k, const unsigned char* cur, unsigned char* oth, const unsigned* hist,
                                           const double* ac, int H, int W, int tid) {
  const int G = (W + 3) >> 2;            // groups of four x per row
  const int items = 3 * H * G;
  const bool point = WORD && op_is_point(k.op);
  for (int it = tid; it < items; it += BLOCK) {
    const int row = it / G, g = it - row * G;     // row = c * H + y
    const int c = row / H, y = row - c * H;
    unsigned u[4];
    if (point) {
      const unsigned w = *(const unsigned*)(cur + row * W + g * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] = op_value(k, hist, ac, c, (w >> (8 * j)) & 0xFFu);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = g * 4 + j;
        u[j] = x < W ? op_pixel(k, cur, hist, ac, H, W, c, y, x) : 0u;
      }
    }
    unsigned char* dst = oth + row * W + g * 4;
    if ((W & 3) == 0) {                  // (both tiles and the row pitch are multiples of four bytes)
      *(unsigned*)dst = u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (g * 4 + j < W) dst[j] = (unsigned char)u[j];
    }
  }
}

// the output: operation k on the tile T, /255 and the normalisation, the erase rectangle set to 0.0; one 16-byte store per
// lane with vec_out (W % 4 == 0 and an aligned `o`)
template <int BLOCK, bool WORD>
__device__ __forceinline__ void output_pass(const float* mean3, const float* std3, int H, int W, int vec_out, const OpCtx& k,
                                             const unsigned char* T, const unsigned* hist, const double* ac, float* o, int et,
                                             int el, int eh, int ew, int tid) {
  const int G = (W + 3) >> 2;
  const int items = 3 * H * G;
  const bool point = WORD && op_is_point(k.op);
  for (int it = tid; it < items; it += BLOCK) {
    const int row = it / G, g = it - row * G;     // row = c * H + y
    const int c = row / H, y = row - c * H;
    const float mean = pick3(mean3, c), sd = pick3(std3, c);
    const bool yer = y >= et && y < et + eh;
    unsigned w = 0;
    if (point) w = *(const unsigned*)(T + row * W + g * 4);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = g * 4 + j;
      v[j] = 0.f;
      if (x < W && !(yer && x >= el && x < el + ew)) {
        const unsigned u = point ? op_value(k, hist, ac, c, (w >> (8 * j)) & 0xFFu) : op_pixel(k, T, hist, ac, H, W, c, y, x);
        v[j] = ((float)u / 255.0f - mean) / sd;
      }
    }
    float* dst = o + (size_t)row * W + g * 4;
    if (vec_out) {
      *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (g * 4 + j < W) dst[j] = v[j];
    }
  }
}

// ---- the chain on two tiles, then the output.  `cur` holds the image so far, `oth` is free: every non-Identity slot but
// the last is a byte pass from `cur` into `oth`, the last is evaluated inside the normalising output pass, and the
// statistics an operation needs are collected again on the tile it reads.  The chain is block-uniform, so every barrier is.
// A tile is written and re-read by this block alone, so __syncthreads() (workgroup scope) orders global tiles as it does
// LDS ones.  hist: kStatWords words of LDS, ac: six doubles of LDS.
template <int BLOCK, bool WORD>
__device__ __forceinline__ void run_chain(const ChainSpec& c, unsigned long long chain, unsigned char* cur,
                                           unsigned char* oth, unsigned* hist, double* ac, int H, int W, const float* mean,
                                           const float* std, int vec_out, float* o, int et, int el, int eh, int ew, int tid) {
  unsigned* stat = hist + 768;
  const int last = last_slot(chain);
  OpCtx k = {};            // all slots Identity: the output is read straight from `cur`
  for (int s = 0; s <= last; ++s) {             // (one copy of the passes, not four: the slot is a run-time shift)
    const int op = load_slot(k, c.table, c.nbins, chain, s);
    if (op == OP_IDENTITY) continue;            // costs nothing: no pass, no barrier
    if (op_needs_statistics(op)) {
      // the statistics of an earlier operation are stale: start again, a barrier on both sides (the first one also keeps
      // this slot's writes behind every read of the previous LUT)
      __syncthreads();
      reset_statistics<BLOCK>(hist, tid);
      __syncthreads();
      op_statistics<BLOCK>(k, cur, hist, stat, ac, H * W, tid);
    }
    if (s == last) break;
    byte_pass<BLOCK, WORD>(k, cur, oth, hist, ac, H, W, tid);
    __syncthreads();       // the pass's stores before the next pass's loads, its loads before the next pass's stores
    unsigned char* t = cur;
    cur = oth;
    oth = t;
  }
  output_pass<BLOCK, WORD>(mean, std, H, W, vec_out, k, cur, hist, ac, o, et, el, eh, ew, tid);
}

}  // namespace pol
}  // namespace nbdt
