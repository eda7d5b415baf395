// The front of an ImageNet-style ResNet (torchvision.models.resnet: Conv2d(3, 64, 7, 2, 3) -> BatchNorm -> ReLU ->
// MaxPool2d(3, 2, 1)) as two small data-movement ops around launches the library already has:
//
//   nbdt_stem_patches       fp32 NCHW image -> padded NHWC patch tensor [B][Ho+2][Wo+2][cpad], channel (r*k + s)*3 + ci:
//                           the k x k / stride / pad k/2 convolution over 3 colours is then a 1x1 convolution over
//                           3*k*k (147 -> 160) channels, i.e. nbdt_conv_igemm / nbdt_conv_wgrad as they are
//   nbdt_maxpool3x3s2_fwd   padded NHWC -> padded NHWC, optionally with the winner's window position per output element
//   nbdt_maxpool3x3s2_bwd   the gather that undoes it: every input element sums the (at most four) windows that chose it
//
// All three are HBM-bound, one thread per 8 channels of one pixel, 16-byte accesses on the NHWC side, no LDS, no atomics.
// Storage is bf16 (product) or fp32 (the engines' verification-only reference mode): one template, no arithmetic differs
// because there is none besides the fp32 sum of the backward.  Every index is checked against the image before an address
// is formed from it; the zero ring of the padded tensors is neither read nor written.
#include "common.h"

using namespace nbdt;

namespace {

// 8 consecutive channels of a padded NHWC tensor as fp32
template <typename T>
__device__ __forceinline__ void load8(const T* p, float* f);
template <>
__device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float* f) {
  unpack8(*(const u32x4_t*)p, f);
}
template <>
__device__ __forceinline__ void load8<float>(const float* p, float* f) {
  const float4 a = ((const float4*)p)[0], b = ((const float4*)p)[1];
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
template <typename T>
__device__ __forceinline__ void store8(T* p, const float* f);
template <>
__device__ __forceinline__ void store8<bf16_t>(bf16_t* p, const float* f) {
  *(u32x4_t*)p = pack8(f);       // round-to-nearest-even, NaN preserved (common.h)
}
template <>
__device__ __forceinline__ void store8<float>(float* p, const float* f) {
  ((float4*)p)[0] = make_float4(f[0], f[1], f[2], f[3]);
  ((float4*)p)[1] = make_float4(f[4], f[5], f[6], f[7]);
}

// thread t -> (pixel, 8-channel group): groups fastest, so a wave writes consecutive 16-byte pieces
template <typename T>
__global__ __launch_bounds__(256) void stem_patches_kernel(const float* __restrict__ img, int B, int H, int W, int Ho, int Wo,
                                                           int k, int stride, int cpad, T* __restrict__ out) {
  const int groups = cpad >> 3;
  const long long total = (long long)B * Ho * Wo * groups;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int g = (int)(t % groups);
  long long p = t / groups;
  const int ox = (int)(p % Wo);
  p /= Wo;
  const int oy = (int)(p % Ho);
  const int b = (int)(p / Ho);
  const int pad = k >> 1, nreal = 3 * k * k;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = g * 8 + j;
    float val = 0.f;
    if (c < nreal) {
      const int tap = c / 3, ci = c - tap * 3;
      const int r = tap / k, s = tap - r * k;
      const int iy = oy * stride - pad + r, ix = ox * stride - pad + s;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) val = img[(((size_t)b * 3 + ci) * H + iy) * W + ix];
    }
    v[j] = val;
  }
  store8<T>(out + (((size_t)b * (Ho + 2) + oy + 1) * (Wo + 2) + ox + 1) * cpad + g * 8, v);
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ x, int B, int H, int W, int C,
                                                          T* __restrict__ y, unsigned char* __restrict__ idx) {
  const int Ho = H >> 1, Wo = W >> 1, groups = C >> 3;
  const long long total = (long long)B * Ho * Wo * groups;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int g = (int)(t % groups);
  long long p = t / groups;
  const int ox = (int)(p % Wo);
  p /= Wo;
  const int oy = (int)(p % Ho);
  const int b = (int)(p / Ho);
  // torch's max_pool2d: start from -inf at the first position inside the image, take a later one when it is greater or NaN
  float best[8];
  unsigned pos[8];
  const unsigned first = (oy == 0 ? 3u : 0u) + (ox == 0 ? 1u : 0u);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    best[j] = -INFINITY;
    pos[j] = first;
  }
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int iy = 2 * oy - 1 + dy;
    if (iy < 0 || iy >= H) continue;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int ix = 2 * ox - 1 + dx;
      if (ix < 0 || ix >= W) continue;
      float v[8];
      load8<T>(x + (((size_t)b * (H + 2) + iy + 1) * (W + 2) + ix + 1) * C + g * 8, v);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (v[j] > best[j] || v[j] != v[j]) {
          best[j] = v[j];
          pos[j] = 3u * dy + dx;
        }
    }
  }
  store8<T>(y + (((size_t)b * (Ho + 2) + oy + 1) * (Wo + 2) + ox + 1) * C + g * 8, best);   // (a maximum of T values: exact)
  if (idx) {
    uint2 w;
    w.x = pos[0] | (pos[1] << 8) | (pos[2] << 16) | (pos[3] << 24);
    w.y = pos[4] | (pos[5] << 8) | (pos[6] << 16) | (pos[7] << 24);
    *(uint2*)(idx + (((size_t)b * Ho + oy) * Wo + ox) * C + g * 8) = w;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ gy, const unsigned char* __restrict__ idx,
                                                          int B, int H, int W, int C, T* __restrict__ gx) {
  const int Ho = H >> 1, Wo = W >> 1, groups = C >> 3;
  const long long total = (long long)B * H * W * groups;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int g = (int)(t % groups);
  long long p = t / groups;
  const int ix = (int)(p % W);
  p /= W;
  const int iy = (int)(p % H);
  const int b = (int)(p / H);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  // windows that contain (iy, ix): oy = iy / 2 and, for odd iy, iy / 2 + 1 (if there is such a row); the same in x.
  // Fixed order (oy ascending, then ox), fp32 sum, one rounding.
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int oy = (iy >> 1) + a;
    if ((a == 1 && !(iy & 1)) || oy >= Ho) continue;
    const int dy = iy - (2 * oy - 1);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int ox = (ix >> 1) + c;
      if ((c == 1 && !(ix & 1)) || ox >= Wo) continue;
      const unsigned me = 3u * (unsigned)dy + (unsigned)(ix - (2 * ox - 1));
      const uint2 w = *(const uint2*)(idx + (((size_t)b * Ho + oy) * Wo + ox) * C + g * 8);
      float v[8];
      load8<T>(gy + (((size_t)b * (Ho + 2) + oy + 1) * (Wo + 2) + ox + 1) * C + g * 8, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned chosen = ((j < 4 ? w.x : w.y) >> (8 * (j & 3))) & 0xffu;
        if (chosen == me) acc[j] += v[j];
      }
    }
  }
  store8<T>(gx + (((size_t)b * (H + 2) + iy + 1) * (W + 2) + ix + 1) * C + g * 8, acc);
}

// blocks of 256 threads for `total` threads, or -1 when the grid would not fit
inline long long blocks_for(long long total) {
  const long long n = (total + 255) / 256;
  return n <= 0x7fffffffll ? n : -1;
}

}  // namespace

extern "C" int nbdt_stem_patches(const float* img, int32_t B, int32_t H, int32_t W, int32_t k, int32_t stride,
                                 int32_t cpad, int32_t dtype, void* out, void* stream) {
  NBDT_REQUIRE(img && out, "null argument");
  NBDT_REQUIRE(dtype == NBDT_BF16 || dtype == NBDT_F32, "the patch tensor is bf16 (NBDT_BF16) or fp32 (NBDT_F32)");
  NBDT_REQUIRE(B > 0 && H > 0 && W > 0 && H <= 16384 && W <= 16384, "empty or oversized image batch");
  NBDT_REQUIRE(k >= 1 && k <= 7 && (k & 1) == 1, "kernel size must be odd and at most 7");
  NBDT_REQUIRE(stride == 1 || stride == 2, "stride is 1 or 2");
  NBDT_REQUIRE(H % stride == 0 && W % stride == 0, "image sides must be divisible by the stride");
  NBDT_REQUIRE(cpad > 0 && cpad % 32 == 0 && cpad >= 3 * k * k, "cpad must be a multiple of 32 and at least 3*k*k");
  NBDT_REQUIRE(cpad <= 4096, "cpad is at most 4096");
  const int Ho = H / stride, Wo = W / stride;
  const long long nb = blocks_for((long long)B * Ho * Wo * (cpad / 8));
  NBDT_REQUIRE(nb > 0, "too many elements for one launch");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == NBDT_BF16)
    hipLaunchKernelGGL(stem_patches_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, s, img, B, H, W, Ho, Wo, k, stride,
                       cpad, (bf16_t*)out);
  else
    hipLaunchKernelGGL(stem_patches_kernel<float>, dim3((unsigned)nb), dim3(256), 0, s, img, B, H, W, Ho, Wo, k, stride,
                       cpad, (float*)out);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

#define NBDT_POOL_ARGS()                                                                                   \
  NBDT_REQUIRE(dtype == NBDT_BF16 || dtype == NBDT_F32, "storage is bf16 (NBDT_BF16) or fp32 (NBDT_F32)"); \
  NBDT_REQUIRE(B > 0 && H > 0 && W > 0 && H <= 16384 && W <= 16384, "empty or oversized tensor");          \
  NBDT_REQUIRE(H % 2 == 0 && W % 2 == 0, "H and W must be even");                                          \
  NBDT_REQUIRE(C > 0 && C % 8 == 0 && C <= 65536, "C must be a multiple of 8")

extern "C" int nbdt_maxpool3x3s2_fwd(const void* x, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C, void* y,
                                     uint8_t* idx, void* stream) {
  NBDT_REQUIRE(x && y, "null argument");
  NBDT_POOL_ARGS();
  const long long nb = blocks_for((long long)B * (H / 2) * (W / 2) * (C / 8));
  NBDT_REQUIRE(nb > 0, "too many elements for one launch");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == NBDT_BF16)
    hipLaunchKernelGGL(maxpool_fwd_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, s, (const bf16_t*)x, B, H, W, C,
                       (bf16_t*)y, (unsigned char*)idx);
  else
    hipLaunchKernelGGL(maxpool_fwd_kernel<float>, dim3((unsigned)nb), dim3(256), 0, s, (const float*)x, B, H, W, C,
                       (float*)y, (unsigned char*)idx);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_maxpool3x3s2_bwd(const void* gy, const uint8_t* idx, int32_t dtype, int32_t B, int32_t H, int32_t W,
                                     int32_t C, void* gx, void* stream) {
  NBDT_REQUIRE(gy && idx && gx, "null argument");
  NBDT_POOL_ARGS();
  const long long nb = blocks_for((long long)B * H * W * (C / 8));
  NBDT_REQUIRE(nb > 0, "too many elements for one launch");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == NBDT_BF16)
    hipLaunchKernelGGL(maxpool_bwd_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, s, (const bf16_t*)gy,
                       (const unsigned char*)idx, B, H, W, C, (bf16_t*)gx);
  else
    hipLaunchKernelGGL(maxpool_bwd_kernel<float>, dim3((unsigned)nb), dim3(256), 0, s, (const float*)gy,
                       (const unsigned char*)idx, B, H, W, C, (float*)gx);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}
