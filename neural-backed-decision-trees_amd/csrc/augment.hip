// Training-batch assembly on the device: gather by index + RandomCrop(size, padding) + RandomHorizontalFlip + ToTensor +
// Normalize (reference nbdt/data/cifar.py:11-21, nbdt/data/imagenet.py:37-48) in ONE launch, from a dataset that lives in
// device memory, into the fp32 NCHW tensor the stem kernels of misc.hip read.
//
// Pure data movement: 1 byte in, 4 bytes out per element.  One block per image; the image's 3*H*W source bytes -- one
// contiguous run, 3 KB for CIFAR, 12 KB for TinyImagenet -- go to LDS with 16-byte loads, then a lane produces four
// consecutive x of one output row from LDS (the shifted, possibly reversed byte reads are LDS reads, not unaligned global
// byte loads) and writes one 16-byte store.  Plain stores: the stem reads the tensor back at once.
//
// Built with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (nbdt/_build.py): the three fp32 operations
// (u / 255 - mean) / std are IEEE operations in this order, the bits of torch's CPU x.float().div(255).sub(mean).div(std).
#include "common.h"

using namespace nbdt;

// uint8 images of up to this many bytes are staged in LDS (128 x 128 x 3); larger ones are read from global memory
#define NBDT_AUGMENT_LDS_BYTES 49152

namespace {

struct AugStats {
  float mean[3], std[3], fill[3];
};

// the draw (include/nbdt_hip.h, nbdt/data.py draw_params): splitmix64's finaliser
__host__ __device__ inline unsigned long long mix64(unsigned long long x) {
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ float pick3(const float* v, int c) { return c == 0 ? v[0] : (c == 1 ? v[1] : v[2]); }

// U8: uint8 source, normalised here; else fp32 source, copied.  LDS: the source image is staged in LDS (uint8 images of at
// most NBDT_AUGMENT_LDS_BYTES); else every element is a guarded global read (fp32 sources, ImageNet-sized uint8 images).
// Every address is formed only after its index has been checked: idx against [0, N), (sy, sx) against the image, and
// (dy, dx) are clamped to [0, 2 * pad] whatever params_in holds.
//
// A shard (nbdt_augment_batch_sharded): src / labels_src hold the N samples [index_base, index_base + N) of a larger
// dataset and index[] holds that dataset's indices.  The draw hashes index[b] itself, the gather reads row
// index[b] - index_base: a sample gets the crop it gets from the whole dataset.  The difference is taken mod 2^64 and
// compared unsigned, so no index, however far outside the shard, passes as a row of it (the entry bounds index_base).
template <bool U8, bool LDS>
__global__ __launch_bounds__(256) void augment_kernel(const void* __restrict__ src, const long long* __restrict__ labels_src,
                                                      const long long* __restrict__ index, long long index_base,
                                                      long long N, int H, int W,
                                                      int pad, int flip_on, AugStats st, unsigned long long key,
                                                      const signed char* __restrict__ params_in, int vec_in, int vec_out,
                                                      float* __restrict__ out, long long* __restrict__ labels_out,
                                                      signed char* __restrict__ params_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tile[];  // [3][H][W] (LDS only)
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = 3 * H * W;
  const long long gidx = index[b];                 // the dataset's index: what the draw hashes
  const unsigned long long idx = (unsigned long long)gidx - (unsigned long long)index_base;      // the row held here
  const bool valid = idx < (unsigned long long)N;
  float* o = out + (size_t)b * n;
  int dy = 0, dx = 0, fl = 0;
  if (valid) {
    if (params_in) {
      dy = params_in[b * 3];
      dx = params_in[b * 3 + 1];
      fl = params_in[b * 3 + 2] != 0;
      dy = dy < 0 ? 0 : (dy > 2 * pad ? 2 * pad : dy);
      dx = dx < 0 ? 0 : (dx > 2 * pad ? 2 * pad : dx);
    } else {
      const unsigned long long r = mix64(key ^ ((unsigned long long)gidx * 0xD1342543DE82EF95ull));
      const unsigned span = 2u * (unsigned)pad + 1u;
      dy = (int)((((unsigned)r & 0xFFFFFFu) * span) >> 24);
      dx = (int)((((unsigned)(r >> 24) & 0xFFFFFFu) * span) >> 24);
      fl = flip_on ? (int)(r >> 63) : 0;
    }
  }
  if (tid == 0) {
    labels_out[b] = valid ? labels_src[idx] : -1ll;
    if (params_out) {
      params_out[b * 3] = (signed char)dy;
      params_out[b * 3 + 1] = (signed char)dx;
      params_out[b * 3 + 2] = (signed char)fl;
    }
  }
  if (!valid) {      // (block-uniform) an index the host could not check: a zero image, label -1, no source address formed
    for (int i = tid; i < n; i += 256) o[i] = 0.f;
    return;
  }
  const unsigned char* s8 = (const unsigned char*)src + (size_t)idx * n;
  const float* s32 = (const float*)src + (size_t)idx * n;
  if (LDS) {
    if (vec_in)
      for (int i = tid; i < (n >> 4); i += 256) ((u32x4_t*)tile)[i] = ((const u32x4_t*)s8)[i];
    else
      for (int i = tid; i < n; i += 256) tile[i] = s8[i];
    __syncthreads();
  }
  const int G = (W + 3) >> 2;            // groups of four x per row
  const int items = 3 * H * G;
  for (int it = tid; it < items; it += 256) {
    const int row = it / G, g = it - row * G;     // row = c * H + y
    const int c = row / H, y = row - c * H;
    const int sy = y + dy - pad;
    const bool yin = sy >= 0 && sy < H;
    const float mean = pick3(st.mean, c), sd = pick3(st.std, c), fill = pick3(st.fill, c);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = g * 4 + k;
      const int xs = fl ? W - 1 - x : x;
      const int sx = xs + dx - pad;
      const bool in = yin && x < W && sx >= 0 && sx < W;
      const int off = (c * H + sy) * W + sx;
      if (U8) {
        unsigned u = 0;
        if (in) u = LDS ? tile[off] : s8[off];
        v[k] = ((float)u / 255.0f - mean) / sd;
      } else {
        v[k] = in ? s32[off] : fill;
      }
    }
    float* dst = o + (size_t)row * W + g * 4;
    if (vec_out) {
      *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (g * 4 + k < W) dst[k] = v[k];
    }
  }
}

}  // namespace

extern "C" int nbdt_augment_batch_sharded(const void* src, int32_t src_dtype, const int64_t* labels_src,
                                          const int64_t* index, int64_t index_base, int32_t B, int64_t N, int32_t H,
                                          int32_t W, int32_t pad, int32_t flip, const float* mean, const float* std,
                                          const float* fill, uint64_t seed, uint64_t epoch, const int8_t* params_in,
                                          float* out, int64_t* labels_out, int8_t* params_out, void* stream) {
  NBDT_REQUIRE(src && labels_src && index && out && labels_out, "null argument");
  NBDT_REQUIRE(N <= 0 || (index_base >= 0 && index_base <= INT64_MAX - N),
               "index_base must be >= 0 and index_base + N must fit int64");
  NBDT_REQUIRE(src_dtype == NBDT_U8 || src_dtype == NBDT_F32, "the dataset is uint8 (NBDT_U8) or fp32 (NBDT_F32)");
  NBDT_REQUIRE(B > 0, "empty batch");
  NBDT_REQUIRE(N > 0, "empty dataset");
  NBDT_REQUIRE(H > 0 && W > 0 && H <= 4096 && W <= 4096, "image sides must be 1..4096");
  NBDT_REQUIRE(pad >= 0 && pad <= NBDT_AUGMENT_MAX_PAD, "pad must be 0..NBDT_AUGMENT_MAX_PAD");
  NBDT_REQUIRE(flip == 0 || flip == 1, "flip is 0 or 1");
  AugStats st = {};
  if (src_dtype == NBDT_U8) {
    NBDT_REQUIRE(mean && std, "a uint8 dataset needs mean[3] and std[3]");
    NBDT_REQUIRE(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "std must be non-zero");
    for (int c = 0; c < 3; ++c) { st.mean[c] = mean[c]; st.std[c] = std[c]; }
  } else {
    NBDT_REQUIRE(fill, "an fp32 dataset needs fill[3]");
    for (int c = 0; c < 3; ++c) st.fill[c] = fill[c];
  }
  const unsigned long long key = mix64((unsigned long long)seed * 0x9E3779B97F4A7C15ull + (unsigned long long)epoch);
  const int n = 3 * H * W;
  const int vec_out = (W % 4 == 0 && (uintptr_t)out % 16 == 0) ? 1 : 0;
  const long long* ls = (const long long*)labels_src;
  const long long* ix = (const long long*)index;
  long long* lo = (long long*)labels_out;
  const signed char* pin = (const signed char*)params_in;
  signed char* pout = (signed char*)params_out;
  hipStream_t s = (hipStream_t)stream;
  if (src_dtype == NBDT_F32) {
    hipLaunchKernelGGL((augment_kernel<false, false>), dim3(B), dim3(256), 0, s, src, ls, ix, (long long)index_base,
                       (long long)N, H, W, pad, flip, st, key, pin, 0, vec_out, out, lo, pout);
  } else if (n <= NBDT_AUGMENT_LDS_BYTES) {
    const int vec_in = (n % 16 == 0 && (uintptr_t)src % 16 == 0) ? 1 : 0;
    hipLaunchKernelGGL((augment_kernel<true, true>), dim3(B), dim3(256), (size_t)((n + 15) & ~15), s, src, ls, ix,
                       (long long)index_base, (long long)N, H, W, pad, flip, st, key, pin, vec_in, vec_out, out, lo, pout);
  } else {
    hipLaunchKernelGGL((augment_kernel<true, false>), dim3(B), dim3(256), 0, s, src, ls, ix, (long long)index_base,
                       (long long)N, H, W, pad, flip, st, key, pin, 0, vec_out, out, lo, pout);
  }
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

// the whole dataset is the shard at base 0: the same kernels, the same bits
extern "C" int nbdt_augment_batch(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index,
                                  int32_t B, int64_t N, int32_t H, int32_t W, int32_t pad, int32_t flip,
                                  const float* mean, const float* std, const float* fill, uint64_t seed, uint64_t epoch,
                                  const int8_t* params_in, float* out, int64_t* labels_out, int8_t* params_out,
                                  void* stream) {
  return nbdt_augment_batch_sharded(src, src_dtype, labels_src, index, 0, B, N, H, W, pad, flip, mean, std, fill, seed,
                                    epoch, params_in, out, labels_out, params_out, stream);
}
