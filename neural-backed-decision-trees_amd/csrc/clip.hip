// Gradient clipping by global norm (torch.nn.utils.clip_grad_norm_, torchvision's --clip-grad-norm) over the flat gradient
// arena of nbdt.engine.ParamStore, on gfx950.
//
//   S = sum_i (double)g_i (double)g_i;  norm = |gscale| sqrtf((float)S);  coef = max_norm / (norm + 1e-6f)
//   coef < 1:  g_i = g_i * coef        else (and for a non-finite norm): g is not touched
//
// Three launches per step, no host synchronisation, no floating-point atomics, no last-block-done counter:
//   1. clip_partials_kernel  clip_blocks(n) blocks (at most kMaxBlocks, 8 per CU), each the owner of ONE contiguous
//                            chunk of 16-byte groups; thread t takes groups t, t + 256, ... of the chunk into four fp64
//                            accumulators (one per component; a product of two floats is exact in fp64, so each step is
//                            one rounding), the last block's first n % 4 lanes take the scalar tail, waves fold with the
//                            xor butterfly, the block's four wave sums are added in wave order, and one fp64 partial per
//                            block goes to the plan's workspace.
//   2. clip_fold_kernel      ONE block: thread t sums partials t, t + 256, ... in increasing index, the same butterfly
//                            and wave-order sum, then thread 0 forms norm and coef -- five fp32 operations, the root and
//                            the division IEEE-correct (-fhip-fp32-correctly-rounded-divide-sqrt) -- and updates the
//                            32-byte record with plain loads and stores (it is the only writer).
//   3. clip_apply_kernel     the partition of launch 1; every wave reads coef from the record and returns at once when
//                            it is 1, else g_i *= coef with 16-byte accesses and the same scalar tail.
// Which thread sums what, in which order, is fixed by n alone: the same g gives the same record bits on every run, with
// nbdt_set_deterministic on or off.  The fp64 work of launch 1 is one convert and one fused multiply-add per element
// beside a 4-byte read; whether that or the bytes bound the pass is a measurement.
#include "arena.h"

#include <math.h>

namespace nbdt {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;     // 8 blocks of 4 waves on each of 256 CUs
constexpr int kGroupsPerBlockMin = 4 * kThreads;   // below 16 KiB a block is not worth its launch slot

struct ClipRecord {                  // include/nbdt_hip.h: 32 bytes
  float norm, coef;
  int clipped, steps, nonfinite, total_clipped;
  int reserved[2];
};
static_assert(sizeof(ClipRecord) == 32, "the clip record is 32 bytes by ABI");

struct ClipPlan : ArenaPlan {        // the blob: the record, then the partials
  using ArenaPlan::ArenaPlan;
  int blocks = 0;
  ClipRecord* rec = nullptr;
  double* part = nullptr;
};

// blocks and 16-byte groups per block: a function of n alone
inline int clip_blocks(long long n) {
  const long long n4 = n >> 2;
  long long b = (n4 + kGroupsPerBlockMin - 1) / kGroupsPerBlockMin;
  if (b < 1) b = 1;
  if (b > kMaxBlocks) b = kMaxBlocks;
  return (int)b;
}
inline long long clip_chunk(long long n, int blocks) { return ((n >> 2) + blocks - 1) / blocks; }

// the block's sum in thread 0: butterfly per wave, then wave 0 + wave 1 + wave 2 + wave 3 in that order
__device__ __forceinline__ double block_sum(double v, double* lds) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__global__ __launch_bounds__(kThreads) void clip_partials_kernel(const float* __restrict__ g, long long n, long long chunk,
                                                                 double* __restrict__ part) {
  __shared__ double lds[kThreads / 64];
  const long long n4 = n >> 2;
  const long long begin = (long long)blockIdx.x * chunk;
  long long end = begin + chunk;
  if (end > n4) end = n4;
  const float4* g4 = (const float4*)g;
  double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
#pragma unroll 8
  for (long long i = begin + threadIdx.x; i < end; i += kThreads) {
    const float4 v = g4[i];
    const double x = (double)v.x, y = (double)v.y, z = (double)v.z, w = (double)v.w;
    sx = fma(x, x, sx);              // x * x is exact in fp64: the fused form rounds once, as the separate add would
    sy = fma(y, y, sy);
    sz = fma(z, z, sz);
    sw = fma(w, w, sw);
  }
  double s = (sx + sy) + (sz + sw);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x < (unsigned)(n & 3)) {   // the arena's last n % 4 elements
    const double t = (double)g[(n4 << 2) + threadIdx.x];
    s = fma(t, t, s);
  }
  s = block_sum(s, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void clip_fold_kernel(const double* __restrict__ part, int n_part, float gscale,
                                                             float max_norm, ClipRecord* rec) {
  __shared__ double lds[kThreads / 64];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_part; i += kThreads) s += part[i];
  s = block_sum(s, lds);
  if (threadIdx.x != 0) return;
  const float s32 = (float)s;
  const float r = sqrtf(s32);
  const float norm = fabsf(gscale) * r;
  const float den = norm + 1e-6f;
  float coef = max_norm / den;
  ClipRecord c = *rec;
  c.steps += 1;
  c.clipped = 0;
  if ((__float_as_uint(norm) & 0x7f800000u) == 0x7f800000u) {   // inf or NaN: the step is counted and left alone
    coef = 1.f;
    c.nonfinite += 1;
  } else if (coef < 1.f) {
    c.clipped = 1;
    c.total_clipped += 1;
  } else {
    coef = 1.f;
  }
  c.norm = norm;
  c.coef = coef;
  *rec = c;
}

__global__ __launch_bounds__(kThreads) void clip_apply_kernel(float* __restrict__ g, long long n, long long chunk,
                                                              const ClipRecord* __restrict__ rec) {
  const float coef = rec->coef;      // one address for the whole grid: block-uniform
  if (coef == 1.0f) return;          // not clipped: nothing is read or written
  const long long n4 = n >> 2;
  const long long begin = (long long)blockIdx.x * chunk;
  long long end = begin + chunk;
  if (end > n4) end = n4;
  float4* g4 = (float4*)g;
#pragma unroll 4
  for (long long i = begin + threadIdx.x; i < end; i += kThreads) {
    float4 v = g4[i];
    v.x *= coef; v.y *= coef; v.z *= coef; v.w *= coef;
    g4[i] = v;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x < (unsigned)(n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    g[i] = g[i] * coef;
  }
}

int clip_check(void* plan, const float* g) {
  NBDT_REQUIRE(g, "null gradient arena");
  NBDT_REQUIRE(((uintptr_t)g % 16) == 0, "the gradient arena must be 16-byte aligned");
  NBDT_REQUIRE(plan, "null plan");
  int dev = 0;
  NBDT_HIP_CHECK(hipGetDevice(&dev));
  NBDT_REQUIRE(dev == ((ClipPlan*)plan)->blob.device, "the plan's workspace lives on another device");
  return NBDT_OK;
}

}  // namespace
}  // namespace nbdt

using nbdt::ClipPlan;
using nbdt::ClipRecord;

extern "C" int nbdt_clip_create(int64_t n, void** plan) {
  NBDT_REQUIRE(plan, "null plan pointer");
  *plan = nullptr;
  NBDT_REQUIRE(n > 0, "empty arena");
  ClipPlan* P = new ClipPlan(n, sizeof(ClipRecord) + (size_t)nbdt::kMaxBlocks * sizeof(double));
  P->blocks = nbdt::clip_blocks(n);
  const ClipRecord start = {0.f, 1.f, 0, 0, 0, 0, {0, 0}};   // read before the first step: nothing clipped
  P->rec = (ClipRecord*)P->blob.put(0, &start, sizeof(start));
  P->part = (double*)(P->blob.base + sizeof(ClipRecord));
  return nbdt::finish_plan(P, "nbdt_clip_create: device workspace", plan);
}

extern "C" int nbdt_clip_destroy(void* plan) {
  delete (ClipPlan*)plan;
  return NBDT_OK;
}

extern "C" int nbdt_clip_norm(void* plan, const float* g, float grad_scale, float max_norm, void* stream) {
  NBDT_REQUIRE(isfinite(max_norm) && max_norm > 0.f, "max_norm must be finite and > 0");
  NBDT_REQUIRE(isfinite(grad_scale), "grad_scale must be finite");
  if (int rc = nbdt::clip_check(plan, g)) return rc;
  ClipPlan* P = (ClipPlan*)plan;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(nbdt::clip_partials_kernel, dim3((unsigned)P->blocks), dim3(nbdt::kThreads), 0, st, g, P->n,
                     nbdt::clip_chunk(P->n, P->blocks), P->part);
  NBDT_LAUNCH_CHECK();
  hipLaunchKernelGGL(nbdt::clip_fold_kernel, dim3(1), dim3(nbdt::kThreads), 0, st, P->part, P->blocks, grad_scale,
                     max_norm, P->rec);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_clip_apply(void* plan, float* g, void* stream) {
  if (int rc = nbdt::clip_check(plan, g)) return rc;
  ClipPlan* P = (ClipPlan*)plan;
  hipLaunchKernelGGL(nbdt::clip_apply_kernel, dim3((unsigned)P->blocks), dim3(nbdt::kThreads), 0, (hipStream_t)stream, g,
                     P->n, nbdt::clip_chunk(P->n, P->blocks), P->rec);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" const void* nbdt_clip_record(void* plan) { return plan ? ((ClipPlan*)plan)->rec : nullptr; }

extern "C" int nbdt_clip_record_to_host(void* plan, void* out32, void* stream) {
  NBDT_REQUIRE(plan && out32, "null argument");
  ClipPlan* P = (ClipPlan*)plan;
  NBDT_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  NBDT_HIP_CHECK(hipMemcpy(out32, P->rec, sizeof(ClipRecord), hipMemcpyDeviceToHost));
  return NBDT_OK;
}
