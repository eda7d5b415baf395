// Exponential moving average (EMA) of the weights over the flat parameter arena of nbdt.engine.ParamStore, and the in-place
// exchange of the live values with the average, on gfx950.
//
//   update, per element:  t = p - e;  e = e + one_minus_decay * t        (three roundings: subtract, multiply, add)
//   swap, per element:    (p, e) = (e, p);  mirror = bf16(new p)          (round to nearest even, as sgd_kernel writes it)
//
// Both are one streaming pass with 16-byte accesses: a block takes kChunk consecutive float4 and every thread kUnroll of
// them, 256 float4 apart, all loads of a thread issued before its first store.  An element is read and written by one
// thread only, there are no atomics and nothing crosses a block: the bits depend on the inputs alone.  The arena's
// alignment gaps and in-entry padding are zero in both buffers and the formula keeps them zero (0 - 0 = 0, omd * 0 = 0,
// 0 + 0 = 0), so neither pass needs a segment table.  Plain loads and stores: the shadow and the arena are read again
// by the next update, nothing here is a one-off stream (DESIGN.md section 13 has the measurement).
// The _multi forms do the same for many small tensors (the BatchNorm running statistics, [C] each) in ONE launch: a device
// table of rows (live pointer, shadow pointer, length), one block per row.
// Built with -ffp-contract=off: e + omd * t must not become a fused multiply-add, the tests compare bits with
// e.add_((p - e).mul_(omd)) on the host.
#include "common.h"

namespace nbdt {
namespace {

constexpr int kUnroll = 4;                  // float4 per thread
constexpr int kChunk = 256 * kUnroll;       // float4 per block

__device__ __forceinline__ float4 ema_of(const float4 p, const float4 e, const float omd) {
  float4 t, o;
  t.x = p.x - e.x; t.y = p.y - e.y; t.z = p.z - e.z; t.w = p.w - e.w;
  t.x = omd * t.x; t.y = omd * t.y; t.z = omd * t.z; t.w = omd * t.w;
  o.x = e.x + t.x; o.y = e.y + t.y; o.z = e.z + t.z; o.w = e.w + t.w;
  return o;
}

__global__ __launch_bounds__(256) void ema_update_kernel(const float4* __restrict__ p, float4* __restrict__ e,
                                                         long long n4, float omd) {
  const long long base = (long long)blockIdx.x * kChunk + threadIdx.x;
  float4 pv[kUnroll], ev[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const long long i = base + u * 256;
    if (i < n4) {
      pv[u] = p[i];
      ev[u] = e[i];
    }
  }
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const long long i = base + u * 256;
    if (i < n4) e[i] = ema_of(pv[u], ev[u], omd);
  }
}

__global__ __launch_bounds__(256) void ema_swap_kernel(float4* __restrict__ p, float4* __restrict__ e,
                                                       uint2* __restrict__ pb, long long n4) {
  const long long base = (long long)blockIdx.x * kChunk + threadIdx.x;
  float4 pv[kUnroll], ev[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const long long i = base + u * 256;
    if (i < n4) {
      pv[u] = p[i];
      ev[u] = e[i];
    }
  }
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const long long i = base + u * 256;
    if (i < n4) {
      p[i] = ev[u];
      e[i] = pv[u];
      if (pb) pb[i] = bf16x4_of(ev[u]);
    }
  }
}

// one block per table row (live, shadow, length); lengths are multiples of 32 elements, so a row is whole float4s
__global__ __launch_bounds__(256) void ema_update_multi_kernel(const long long* __restrict__ table, float omd) {
  const long long* row = table + 3 * (long long)blockIdx.x;
  const float4* p = (const float4*)row[0];
  float4* e = (float4*)row[1];
  const long long n4 = row[2] >> 2;
  for (long long i = threadIdx.x; i < n4; i += 256) e[i] = ema_of(p[i], e[i], omd);
}

__global__ __launch_bounds__(256) void ema_swap_multi_kernel(const long long* __restrict__ table) {
  const long long* row = table + 3 * (long long)blockIdx.x;
  float4* p = (float4*)row[0];
  float4* e = (float4*)row[1];
  const long long n4 = row[2] >> 2;
  for (long long i = threadIdx.x; i < n4; i += 256) {
    const float4 pv = p[i], ev = e[i];
    p[i] = ev;
    e[i] = pv;
  }
}

inline bool decay_ok(float omd) { return omd >= 0.f && omd <= 1.f; }      // (false for NaN)

}  // namespace
}  // namespace nbdt

extern "C" int nbdt_ema_update(const float* p, float* ema, int64_t n, float one_minus_decay, void* stream) {
  NBDT_REQUIRE(p && ema, "null ema buffer");
  NBDT_REQUIRE(n > 0 && n % 4 == 0, "ema: the element count must be a positive multiple of 4");
  NBDT_REQUIRE(((uintptr_t)p % 16) == 0 && ((uintptr_t)ema % 16) == 0, "ema buffers must be 16-byte aligned");
  NBDT_REQUIRE(p != ema, "ema: the shadow is the live buffer");
  NBDT_REQUIRE(nbdt::decay_ok(one_minus_decay), "ema: one_minus_decay must be in [0, 1]");
  const long long n4 = n >> 2;
  const long long blocks = (n4 + nbdt::kChunk - 1) / nbdt::kChunk;
  NBDT_REQUIRE(blocks <= 0x7fffffffLL, "ema: arena too large");
  hipLaunchKernelGGL(nbdt::ema_update_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)p,
                     (float4*)ema, n4, one_minus_decay);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_ema_swap(float* p, float* ema, void* p_bf16, int64_t n, void* stream) {
  NBDT_REQUIRE(p && ema, "null ema buffer");
  NBDT_REQUIRE(n > 0 && n % 4 == 0, "ema: the element count must be a positive multiple of 4");
  NBDT_REQUIRE(((uintptr_t)p % 16) == 0 && ((uintptr_t)ema % 16) == 0, "ema buffers must be 16-byte aligned");
  NBDT_REQUIRE(((uintptr_t)p_bf16 % 8) == 0, "the bf16 mirror must be 8-byte aligned");
  NBDT_REQUIRE(p != ema, "ema: the shadow is the live buffer");
  const long long n4 = n >> 2;
  const long long blocks = (n4 + nbdt::kChunk - 1) / nbdt::kChunk;
  NBDT_REQUIRE(blocks <= 0x7fffffffLL, "ema: arena too large");
  hipLaunchKernelGGL(nbdt::ema_swap_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float4*)p,
                     (float4*)ema, (uint2*)p_bf16, n4);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_ema_update_multi(const int64_t* table, int32_t n_rows, float one_minus_decay, void* stream) {
  NBDT_REQUIRE(table, "null ema table");
  NBDT_REQUIRE(n_rows > 0, "empty ema table");
  NBDT_REQUIRE(((uintptr_t)table % 8) == 0, "the ema table must be 8-byte aligned");
  NBDT_REQUIRE(nbdt::decay_ok(one_minus_decay), "ema: one_minus_decay must be in [0, 1]");
  hipLaunchKernelGGL(nbdt::ema_update_multi_kernel, dim3((unsigned)n_rows), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)table, one_minus_decay);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_ema_swap_multi(const int64_t* table, int32_t n_rows, void* stream) {
  NBDT_REQUIRE(table, "null ema table");
  NBDT_REQUIRE(n_rows > 0, "empty ema table");
  NBDT_REQUIRE(((uintptr_t)table % 8) == 0, "the ema table must be 8-byte aligned");
  hipLaunchKernelGGL(nbdt::ema_swap_multi_kernel, dim3((unsigned)n_rows), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)table);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}
