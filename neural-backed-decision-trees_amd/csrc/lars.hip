// LARS (layer-wise adaptive rate scaling, You et al. 2017; apex LARC(clip=False) around optim.SGD) over the flat
// parameter arena of nbdt.engine.ParamStore, on gfx950.
//
//   per segment s:  gn = sqrt(sum (gscale g_i)^2),  wn = sqrt(sum p_i^2)
//                   ratio_s = trust wn / (gn + wd_s wn + eps)   if adapt_s and wn > 0 and gn > 0, else 1
//   per element:    u = ratio_s (gscale g_i + wd_s p_i);  buf_i = momentum buf_i + u;  p_i -= lr buf_i;  mirror_i = bf16(p_i)
//
// Three launches per step, no host synchronisation, no floating-point atomics:
//   1. lars_partials_kernel  one WAVE per item of the norm table -- (segment, start, <= kItem elements) -- writes the two
//                            fp32 partial sums of squares of its item to the plan's workspace.  A 3.7 M-element weight is
//                            900 items over 225 blocks; a 64-element weight is one wave, next to three other tensors' waves
//                            in its block.  Segments with adapt = 0 have no items (their ratio is 1 whatever the norms are).
//   2. lars_fold_kernel      one wave per segment sums that segment's partials -- lane l takes partials l, l + 64, ..., then
//                            the xor butterfly -- and writes ratio[s].  The one sqrt pair and the one division per segment
//                            are IEEE-correct (this file is built with -fhip-fp32-correctly-rounded-divide-sqrt).
//   3. lars_update_kernel    one wave per item of the update table (every segment, in items of <= kItem elements, plus the
//                            gaps between segments as items that only zero the gradient): the streaming pass sgd_kernel is,
//                            16-byte accesses, a scalar tail for length % 4.
// Which wave sums which elements, and in which order, is fixed by the tables, which are fixed by the segment list: the
// step gives the same bits on every run, with nbdt_set_deterministic on or off.  Built with -ffp-contract=off: the
// element update is the four roundings of the formula above, which is what the exact-fixture test evaluates on the host.
#include "common.h"

#include <vector>

namespace nbdt {
namespace {

constexpr int kItem = 4096;          // elements per wave item: 16 iterations of 64 lanes x 16 bytes
constexpr int kWavesPerBlock = 4;

struct LarsItem {
  long long start;   // first element (a multiple of 4 for segment items; anything for gap items)
  int len;           // 1..kItem
  int seg;           // segment index, or -1: a gap (only ever zeroed in g)
};
struct LarsSeg {
  float wd;
  int adapt;
  int first, count;  // this segment's partial sums: part[first .. first + count)
};

struct LarsPlan {
  long long n = 0;
  int n_seg = 0, n_norm = 0, n_upd = 0, device = 0;
  void* blob = nullptr;              // one allocation: the three tables, the partials and the ratios
  LarsItem *norm = nullptr, *upd = nullptr;
  LarsSeg* seg = nullptr;
  float2* part = nullptr;
  float* ratio = nullptr;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void lars_partials_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                            const LarsItem* __restrict__ items, int n_items, float gscale,
                                                            float2* __restrict__ part) {
  const int item = blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (item >= n_items) return;
  const int lane = threadIdx.x & 63;
  const LarsItem it = items[item];
  const float4* p4 = (const float4*)(p + it.start);
  const float4* g4 = (const float4*)(g + it.start);
  const int n4 = it.len >> 2;
  float4 sw = {0.f, 0.f, 0.f, 0.f}, sg = {0.f, 0.f, 0.f, 0.f};
  for (int i = lane; i < n4; i += 64) {
    const float4 pv = p4[i];
    float4 gv = g4[i];
    gv.x *= gscale; gv.y *= gscale; gv.z *= gscale; gv.w *= gscale;
    sw.x += pv.x * pv.x; sw.y += pv.y * pv.y; sw.z += pv.z * pv.z; sw.w += pv.w * pv.w;
    sg.x += gv.x * gv.x; sg.y += gv.y * gv.y; sg.z += gv.z * gv.z; sg.w += gv.w * gv.w;
  }
  float w = (sw.x + sw.y) + (sw.z + sw.w), q = (sg.x + sg.y) + (sg.z + sg.w);
  if (lane < (it.len & 3)) {         // the segment's last item: length % 4 elements
    const long long i = it.start + ((long long)n4 << 2) + lane;
    const float pv = p[i], gv = gscale * g[i];
    w += pv * pv;
    q += gv * gv;
  }
  w = wave_sum(w);
  q = wave_sum(q);
  if (lane == 0) part[item] = float2{w, q};
}

__global__ __launch_bounds__(256) void lars_fold_kernel(const LarsSeg* __restrict__ segs, int n_seg,
                                                        const float2* __restrict__ part, float trust, float eps,
                                                        float* __restrict__ ratio) {
  const int s = blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (s >= n_seg) return;
  const int lane = threadIdx.x & 63;
  const LarsSeg sg = segs[s];
  float r = 1.f;
  if (sg.adapt) {
    float w = 0.f, q = 0.f;
    for (int i = lane; i < sg.count; i += 64) {
      const float2 v = part[sg.first + i];
      w += v.x;
      q += v.y;
    }
    const float wn = sqrtf(wave_sum(w)), gn = sqrtf(wave_sum(q));
    if (wn > 0.f && gn > 0.f) r = (trust * wn) / ((gn + sg.wd * wn) + eps);
  }
  if (lane == 0) ratio[s] = r;
}

__global__ __launch_bounds__(256) void lars_update_kernel(float* __restrict__ p, float* __restrict__ g,
                                                          float* __restrict__ buf, const LarsItem* __restrict__ items,
                                                          int n_items, const LarsSeg* __restrict__ segs,
                                                          const float* __restrict__ ratio, float lr, float momentum,
                                                          float gscale, bf16_t* __restrict__ pb, int zero_g) {
  const int item = blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (item >= n_items) return;
  const int lane = threadIdx.x & 63;
  const LarsItem it = items[item];
  if (it.seg < 0) {                  // a gap between segments, or the arena's tail: nothing but g is touched
    if (zero_g)
      for (int i = lane; i < it.len; i += 64) g[it.start + i] = 0.f;
    return;
  }
  const float r = ratio[it.seg], wd = segs[it.seg].wd;
  float4* p4 = (float4*)(p + it.start);
  float4* g4 = (float4*)(g + it.start);
  float4* b4 = (float4*)(buf + it.start);
  uint2* pb2 = pb ? (uint2*)(pb + it.start) : nullptr;
  const int n4 = it.len >> 2;
  for (int i = lane; i < n4; i += 64) {
    float4 pv = p4[i];
    const float4 gv = g4[i];
    float4 bv = b4[i];
    bv.x = momentum * bv.x + r * (gscale * gv.x + wd * pv.x);
    bv.y = momentum * bv.y + r * (gscale * gv.y + wd * pv.y);
    bv.z = momentum * bv.z + r * (gscale * gv.z + wd * pv.z);
    bv.w = momentum * bv.w + r * (gscale * gv.w + wd * pv.w);
    pv.x -= lr * bv.x; pv.y -= lr * bv.y; pv.z -= lr * bv.z; pv.w -= lr * bv.w;
    b4[i] = bv;
    p4[i] = pv;
    if (zero_g) g4[i] = float4{0.f, 0.f, 0.f, 0.f};
    if (pb2) {
      uint2 o;
      o.x = pack_bf16x2(pv.x, pv.y);
      o.y = pack_bf16x2(pv.z, pv.w);
      pb2[i] = o;
    }
  }
  if (lane < (it.len & 3)) {         // tail (length % 4) of the segment's last item
    const long long i = it.start + ((long long)n4 << 2) + lane;
    const float b = momentum * buf[i] + r * (gscale * g[i] + wd * p[i]);
    const float pn = p[i] - lr * b;
    buf[i] = b;
    p[i] = pn;
    if (zero_g) g[i] = 0.f;
    if (pb) pb[i] = f32_to_bf16(pn);
  }
}

void push_items(std::vector<LarsItem>& v, long long start, long long len, int seg) {
  for (long long o = 0; o < len; o += kItem) {
    const long long l = len - o < kItem ? len - o : kItem;
    v.push_back(LarsItem{start + o, (int)l, seg});
  }
}

}  // namespace
}  // namespace nbdt

using nbdt::LarsItem;
using nbdt::LarsPlan;
using nbdt::LarsSeg;

extern "C" int nbdt_lars_create(int64_t n, const int64_t* offsets, const int64_t* lengths, const float* weight_decays,
                                const int32_t* adapt, int32_t n_seg, void** plan) {
  NBDT_REQUIRE(plan, "null plan pointer");
  *plan = nullptr;
  NBDT_REQUIRE(offsets && lengths && weight_decays && adapt, "null segment table");
  NBDT_REQUIRE(n_seg > 0, "empty segment table");
  NBDT_REQUIRE(n > 0, "empty arena");
  long long end = 0;                 // end of the previous row
  for (int s = 0; s < n_seg; ++s) {
    NBDT_REQUIRE(lengths[s] > 0, "segment lengths must be positive");
    NBDT_REQUIRE(offsets[s] >= 0 && offsets[s] % 4 == 0, "segment offsets must be multiples of 4 elements");
    if (s > 0) NBDT_REQUIRE(offsets[s] >= offsets[s - 1], "segment rows must be sorted by offset");
    NBDT_REQUIRE(offsets[s] >= end, "segment rows overlap");
    NBDT_REQUIRE(lengths[s] <= n && offsets[s] <= n - lengths[s], "segment runs out of range");
    end = offsets[s] + lengths[s];
  }
  // block -> (segment, range) tables, built once: the norm items of the adaptive segments, and the update items of
  // every segment with the gaps (which zero_grad clears) between them
  std::vector<LarsItem> norm, upd;
  std::vector<LarsSeg> segs((size_t)n_seg);
  end = 0;
  for (int s = 0; s < n_seg; ++s) {
    if (offsets[s] > end) nbdt::push_items(upd, end, offsets[s] - end, -1);
    nbdt::push_items(upd, offsets[s], lengths[s], s);
    const int first = (int)norm.size();
    if (adapt[s]) nbdt::push_items(norm, offsets[s], lengths[s], s);
    segs[(size_t)s] = LarsSeg{weight_decays[s], adapt[s] ? 1 : 0, first, (int)norm.size() - first};
    end = offsets[s] + lengths[s];
  }
  if (n > end) nbdt::push_items(upd, end, n - end, -1);
  NBDT_REQUIRE(upd.size() < (size_t)1 << 30, "arena too large");

  auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
  const size_t o_norm = 0;
  const size_t o_upd = o_norm + up16(norm.size() * sizeof(LarsItem));
  const size_t o_seg = o_upd + up16(upd.size() * sizeof(LarsItem));
  const size_t o_part = o_seg + up16(segs.size() * sizeof(LarsSeg));
  const size_t o_ratio = o_part + up16((norm.size() + 1) * sizeof(float2));
  const size_t total = o_ratio + up16(segs.size() * sizeof(float));
  LarsPlan* P = new LarsPlan();
  P->n = n;
  P->n_seg = n_seg;
  P->n_norm = (int)norm.size();
  P->n_upd = (int)upd.size();
  hipError_t e = hipGetDevice(&P->device);
  if (e == hipSuccess) e = hipMalloc(&P->blob, total);
  char* base = (char*)P->blob;
  if (e == hipSuccess && !norm.empty())
    e = hipMemcpy(base + o_norm, norm.data(), norm.size() * sizeof(LarsItem), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(base + o_upd, upd.data(), upd.size() * sizeof(LarsItem), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(base + o_seg, segs.data(), segs.size() * sizeof(LarsSeg), hipMemcpyHostToDevice);
  if (e == hipSuccess) {             // ratios read before the first step: 1
    std::vector<float> ones(segs.size(), 1.f);
    e = hipMemcpy(base + o_ratio, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    if (P->blob) (void)hipFree(P->blob);
    delete P;
    return nbdt::fail(NBDT_EHIP, "%s: %s", "nbdt_lars_create: device tables", hipGetErrorString(e));
  }
  P->norm = (LarsItem*)(base + o_norm);
  P->upd = (LarsItem*)(base + o_upd);
  P->seg = (LarsSeg*)(base + o_seg);
  P->part = (float2*)(base + o_part);
  P->ratio = (float*)(base + o_ratio);
  *plan = P;
  return NBDT_OK;
}

extern "C" int nbdt_lars_destroy(void* plan) {
  if (!plan) return NBDT_OK;
  LarsPlan* P = (LarsPlan*)plan;
  if (P->blob) (void)hipFree(P->blob);
  delete P;
  return NBDT_OK;
}

extern "C" const float* nbdt_lars_ratios(void* plan) {
  return plan ? ((LarsPlan*)plan)->ratio : nullptr;
}

extern "C" int nbdt_lars_ratios_to_host(void* plan, float* out, void* stream) {
  NBDT_REQUIRE(plan && out, "null argument");
  LarsPlan* P = (LarsPlan*)plan;
  NBDT_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  NBDT_HIP_CHECK(hipMemcpy(out, P->ratio, (size_t)P->n_seg * sizeof(float), hipMemcpyDeviceToHost));
  return NBDT_OK;
}

extern "C" int nbdt_lars_step(void* plan, float* p, float* g, float* buf, float lr, float momentum, float trust,
                              float eps, float grad_scale, void* p_bf16, int32_t zero_grad, void* stream) {
  NBDT_REQUIRE(plan, "null plan");
  NBDT_REQUIRE(p && g && buf, "bad lars arguments");
  NBDT_REQUIRE(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)buf % 16) == 0,
               "flat buffers must be 16-byte aligned");
  NBDT_REQUIRE(((uintptr_t)p_bf16 % 8) == 0, "the bf16 mirror must be 8-byte aligned");
  LarsPlan* P = (LarsPlan*)plan;
  int dev = 0;
  NBDT_HIP_CHECK(hipGetDevice(&dev));
  NBDT_REQUIRE(dev == P->device, "the plan's tables live on another device");
  hipStream_t st = (hipStream_t)stream;
  const int w = nbdt::kWavesPerBlock;
  if (P->n_norm > 0) {
    hipLaunchKernelGGL(nbdt::lars_partials_kernel, dim3((unsigned)((P->n_norm + w - 1) / w)), dim3(256), 0, st, p, g,
                       P->norm, P->n_norm, grad_scale, P->part);
    NBDT_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(nbdt::lars_fold_kernel, dim3((unsigned)((P->n_seg + w - 1) / w)), dim3(256), 0, st, P->seg, P->n_seg,
                     P->part, trust, eps, P->ratio);
  NBDT_LAUNCH_CHECK();
  hipLaunchKernelGGL(nbdt::lars_update_kernel, dim3((unsigned)((P->n_upd + w - 1) / w)), dim3(256), 0, st, p, g, buf,
                     P->upd, P->n_upd, P->seg, P->ratio, lr, momentum, grad_scale, (nbdt::bf16_t*)p_bf16,
                     zero_grad ? 1 : 0);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}
