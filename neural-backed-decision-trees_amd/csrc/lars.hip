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
//   3. lars_update_kernel    one wave per item of the update table: arena.h's streaming pass (arena_update) over one
//                            state arena, with LarsUpdate below as its element arithmetic.
// This file's own: the two norm kernels, the norm table (the items of the adaptive segments alone), the per-segment
// record and the element update.  The table check, the item record and the update table, the streaming pass, the step
// entry's checks and the plan's device memory are arena.h's.
// Which wave sums which elements, and in which order, is fixed by the tables, which are fixed by the segment list: the
// step gives the same bits on every run, with nbdt_set_deterministic on or off.  Built with -ffp-contract=off: the
// element update is the four roundings of the formula above, which is what the exact-fixture test evaluates on the host.
#include "arena.h"

namespace nbdt {
namespace {

constexpr int kItem = 4096;          // elements per wave item: 16 iterations of 64 lanes x 16 bytes

struct LarsSeg {
  float wd;
  int adapt;
  int first, count;  // this segment's partial sums: part[first .. first + count)
};

struct LarsPlan : ArenaPlan {        // the blob: the three tables, the partials and the ratios
  using ArenaPlan::ArenaPlan;
  int n_seg = 0, n_norm = 0, n_upd = 0;
  ArenaItem *norm = nullptr, *upd = nullptr;
  LarsSeg* seg = nullptr;
  float2* part = nullptr;
  float* ratio = nullptr;
};

__global__ __launch_bounds__(256) void lars_partials_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                            const ArenaItem* __restrict__ items, int n_items, float gscale,
                                                            float2* __restrict__ part) {
  const int item = blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (item >= n_items) return;
  const int lane = threadIdx.x & 63;
  const ArenaItem it = items[item];
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

struct LarsUpdate {                  // arena.h's functor contract; a: the momentum buffer
  static constexpr int kStates = 1;
  struct Params {
    const float* ratio;
    float lr, momentum, gscale;
  };
  float r, wd, lr, momentum, gscale;
  __device__ LarsUpdate(const Params& c, const ArenaItem& it)
      : r(c.ratio[it.seg]), wd(it.wd), lr(c.lr), momentum(c.momentum), gscale(c.gscale) {}
  __device__ __forceinline__ void operator()(float& p, float g, float& a, float&) const {
    a = momentum * a + r * (gscale * g + wd * p);
    p -= lr * a;
  }
};

__global__ __launch_bounds__(256) void lars_update_kernel(float* __restrict__ p, float* __restrict__ g,
                                                          float* __restrict__ buf, const ArenaItem* __restrict__ items,
                                                          int n_items, LarsUpdate::Params c, bf16_t* __restrict__ pb,
                                                          int zero_g) {
  arena_update<LarsUpdate>(p, g, buf, nullptr, items, n_items, c, pb, zero_g);
}

}  // namespace
}  // namespace nbdt

using nbdt::ArenaItem;
using nbdt::LarsPlan;
using nbdt::LarsSeg;

extern "C" int nbdt_lars_create(int64_t n, const int64_t* offsets, const int64_t* lengths, const float* weight_decays,
                                const int32_t* adapt, int32_t n_seg, void** plan) {
  if (int rc = nbdt::check_segment_table(n, offsets, lengths, weight_decays && adapt, n_seg, plan,
                                         [](int) { return NBDT_OK; }))
    return rc;
  // wave -> (segment, range) tables, built once: the update items of every segment with the gaps (which zero_grad
  // clears) between them, and the norm items of the adaptive segments
  std::vector<ArenaItem> norm, upd;
  std::vector<LarsSeg> segs((size_t)n_seg);
  if (int rc = nbdt::update_items(upd, nbdt::kItem, n, offsets, lengths, weight_decays, n_seg)) return rc;
  for (int s = 0; s < n_seg; ++s) {
    const int first = (int)norm.size();
    if (adapt[s]) nbdt::push_items(norm, nbdt::kItem, offsets[s], lengths[s], s, weight_decays[s]);
    segs[(size_t)s] = LarsSeg{weight_decays[s], adapt[s] ? 1 : 0, first, (int)norm.size() - first};
  }
  auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
  const size_t o_upd = up16(norm.size() * sizeof(ArenaItem));
  const size_t o_seg = o_upd + up16(upd.size() * sizeof(ArenaItem));
  const size_t o_part = o_seg + up16(segs.size() * sizeof(LarsSeg));
  const size_t o_ratio = o_part + up16((norm.size() + 1) * sizeof(float2));
  LarsPlan* P = new LarsPlan(n, o_ratio + up16(segs.size() * sizeof(float)));
  P->n_seg = n_seg;
  P->n_norm = (int)norm.size();
  P->n_upd = (int)upd.size();
  P->norm = P->blob.put(0, norm);
  P->upd = P->blob.put(o_upd, upd);
  P->seg = P->blob.put(o_seg, segs);
  P->part = (float2*)(P->blob.base + o_part);
  P->ratio = P->blob.put(o_ratio, std::vector<float>(segs.size(), 1.f));   // ratios read before the first step: 1
  return nbdt::finish_plan(P, "nbdt_lars_create: device tables", plan);
}

extern "C" int nbdt_lars_destroy(void* plan) {
  delete (LarsPlan*)plan;
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
  LarsPlan* P = (LarsPlan*)plan;
  if (int rc = nbdt::check_step(P, p, g, buf, nullptr, 1, p_bf16, false)) return rc;
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
                     P->upd, P->n_upd, nbdt::LarsUpdate::Params{P->ratio, lr, momentum, grad_scale},
                     (nbdt::bf16_t*)p_bf16, zero_grad ? 1 : 0);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

