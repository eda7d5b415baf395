// AdamW (torch.optim.AdamW, no amsgrad) and RMSprop (torch.optim.RMSprop, not centered; and TensorFlow's form, the one
// EfficientNet was trained with) over the flat parameter arena of nbdt.engine.ParamStore, on gfx950.
//
// One launch per step: one WAVE per item of the plan's table -- (start, <= kItem elements, the segment's decay), the
// gaps between segments and the tail as items that only zero the gradient -- the streaming pass sgd_kernel and
// lars_update_kernel are, with two state arenas instead of one: 16-byte accesses, a scalar tail for length % 4, the
// bf16 mirror and the zeroed gradient written in the same pass.  34 bytes per element with momentum (read p, g and two
// states, write p, two states, the mirror and g), against 26 of the SGD pass.  Nothing crosses a lane, so where the
// items are cut does not change a bit, and neither does nbdt_set_deterministic.
//
// The item size is a measurement (WRN-28-10 arena, 36.5 M elements, AdamW launch alone, one MI355X): 4096 elements per
// wave, lars.hip's size, 290 us; 2048 295; 1024 286; 512 266 on one box and 221 on a faster one, where 256 gave 213-222
// and the SGD pass 164.  Short items keep the waves that run together on neighbouring memory and leave no long last
// round; the 24-byte item record per 512 elements is 0.14 % of the traffic.  DESIGN.md section 15.
//
// Built with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt: every element update is the sequence of single
// IEEE fp32 operations include/nbdt_hip.h writes out, which tests/_adaptive_ref.py restates on the host bit for bit.
// One square root and one division per element (AdamW: two), expanded to their correctly rounded sequences: 50 to 60
// VALU instructions per element in the ISA, no scratch, 47-57 VGPRs.  Whether that leaves the pass bound by its 34
// bytes is a measurement: DESIGN.md section 15.
#include "common.h"

#include <math.h>

#include <vector>

namespace nbdt {
namespace {

constexpr int kItem = 512;           // elements per wave item: 2 iterations of 64 lanes x 16 bytes (measured: above)
constexpr int kWavesPerBlock = 4;

struct OptItem {
  long long start;   // first element (a multiple of 4 for segment items; anything for gap items)
  int len;           // 1..kItem
  int seg;           // segment index, or -1: a gap (only ever zeroed in g)
  float wd;          // the segment's weight decay
  int pad;
};

struct OptPlan {
  long long n = 0;
  int n_items = 0, device = 0;
  OptItem* items = nullptr;          // device
};

enum Mode { kAdamW = 0, kRmsprop = 1, kRmspropPlain = 2, kRmspropTf = 3 };   // Plain: momentum == 0, no buffer

struct OptScalars {   // fp32 values as include/nbdt_hip.h forms them
  float lr, gscale, eps;
  float b1, omb1, b2, omb2, ss, c2;  // AdamW
  float alpha, oma, mu;              // RMSprop
};

// One element.  s1: m (AdamW) or the momentum buffer; s2: v or the mean square.  k: 1 - lr wd of the segment (AdamW).
template <int MODE>
__device__ __forceinline__ void update(float& p, float g, float& s1, float& s2, const OptScalars& c, float wd, float k) {
  float gs = c.gscale * g;
  if (MODE == kAdamW) {
    const float p1 = p * k;
    s1 = c.b1 * s1 + c.omb1 * gs;
    s2 = c.b2 * s2 + (c.omb2 * gs) * gs;
    const float d = sqrtf(s2) / c.c2 + c.eps;
    p = p1 - c.ss * (s1 / d);
  } else if (MODE == kRmspropTf) {
    gs = gs + wd * p;
    s2 = s2 + c.oma * (gs * gs - s2);
    const float a = sqrtf(s2 + c.eps);
    s1 = c.mu * s1 + c.lr * (gs / a);
    p = p - s1;
  } else {
    gs = gs + wd * p;
    s2 = c.alpha * s2 + (c.oma * gs) * gs;
    const float a = sqrtf(s2) + c.eps;
    if (MODE == kRmsprop) {
      s1 = c.mu * s1 + gs / a;
      p = p - c.lr * s1;
    } else {
      p = p - c.lr * (gs / a);
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void arena_opt_kernel(float* __restrict__ p, float* __restrict__ g,
                                                        float* __restrict__ s1, float* __restrict__ s2,
                                                        const OptItem* __restrict__ items, int n_items, OptScalars c,
                                                        bf16_t* __restrict__ pb, int zero_g) {
  constexpr bool kS1 = MODE != kRmspropPlain;      // the first state arena takes part
  const int item = blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (item >= n_items) return;
  const int lane = threadIdx.x & 63;
  const OptItem it = items[item];
  if (it.seg < 0) {                  // a gap between segments, or the arena's tail: nothing but g is touched
    if (zero_g)
      for (int i = lane; i < it.len; i += 64) g[it.start + i] = 0.f;
    return;
  }
  const float wd = it.wd, k = 1.f - c.lr * wd;
  float4* p4 = (float4*)(p + it.start);
  float4* g4 = (float4*)(g + it.start);
  float4* a4 = kS1 ? (float4*)(s1 + it.start) : nullptr;
  float4* b4 = (float4*)(s2 + it.start);
  uint2* pb2 = pb ? (uint2*)(pb + it.start) : nullptr;
  const int n4 = it.len >> 2;
  for (int i = lane; i < n4; i += 64) {
    float4 pv = p4[i];
    const float4 gv = g4[i];
    float4 av = {0.f, 0.f, 0.f, 0.f};
    if (kS1) av = a4[i];
    float4 bv = b4[i];
    update<MODE>(pv.x, gv.x, av.x, bv.x, c, wd, k);
    update<MODE>(pv.y, gv.y, av.y, bv.y, c, wd, k);
    update<MODE>(pv.z, gv.z, av.z, bv.z, c, wd, k);
    update<MODE>(pv.w, gv.w, av.w, bv.w, c, wd, k);
    if (kS1) a4[i] = av;
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
    float pv = p[i], av = kS1 ? s1[i] : 0.f, bv = s2[i];
    update<MODE>(pv, g[i], av, bv, c, wd, k);
    if (kS1) s1[i] = av;
    s2[i] = bv;
    p[i] = pv;
    if (zero_g) g[i] = 0.f;
    if (pb) pb[i] = f32_to_bf16(pv);
  }
}

void push_items(std::vector<OptItem>& v, long long start, long long len, int seg, float wd) {
  for (long long o = 0; o < len; o += kItem) {
    const long long l = len - o < kItem ? len - o : kItem;
    v.push_back(OptItem{start + o, (int)l, seg, wd, 0});
  }
}

bool unit_interval(float x) { return x >= 0.f && x < 1.f; }    // false for NaN

template <int MODE>
void launch(const OptPlan* P, float* p, float* g, float* s1, float* s2, const OptScalars& c, void* pb, int zero_g,
            hipStream_t st) {
  const int w = kWavesPerBlock;
  hipLaunchKernelGGL(arena_opt_kernel<MODE>, dim3((unsigned)((P->n_items + w - 1) / w)), dim3(256), 0, st, p, g, s1, s2,
                     P->items, P->n_items, c, (bf16_t*)pb, zero_g);
}

}  // namespace
}  // namespace nbdt

using nbdt::OptItem;
using nbdt::OptPlan;
using nbdt::OptScalars;

extern "C" int nbdt_arena_opt_create(int64_t n, const int64_t* offsets, const int64_t* lengths,
                                     const float* weight_decays, int32_t n_seg, void** plan) {
  NBDT_REQUIRE(plan, "null plan pointer");
  *plan = nullptr;
  NBDT_REQUIRE(offsets && lengths && weight_decays, "null segment table");
  NBDT_REQUIRE(n_seg > 0, "empty segment table");
  NBDT_REQUIRE(n > 0, "empty arena");
  long long end = 0;                 // end of the previous row
  for (int s = 0; s < n_seg; ++s) {
    NBDT_REQUIRE(lengths[s] > 0, "segment lengths must be positive");
    NBDT_REQUIRE(offsets[s] >= 0 && offsets[s] % 4 == 0, "segment offsets must be multiples of 4 elements");
    if (s > 0) NBDT_REQUIRE(offsets[s] >= offsets[s - 1], "segment rows must be sorted by offset");
    NBDT_REQUIRE(offsets[s] >= end, "segment rows overlap");
    NBDT_REQUIRE(lengths[s] <= n && offsets[s] <= n - lengths[s], "segment runs out of range");
    NBDT_REQUIRE(weight_decays[s] >= 0.f && weight_decays[s] <= 3.0e38f, "weight decays must be finite and >= 0");
    end = offsets[s] + lengths[s];
  }
  std::vector<OptItem> items;
  end = 0;
  for (int s = 0; s < n_seg; ++s) {
    if (offsets[s] > end) nbdt::push_items(items, end, offsets[s] - end, -1, 0.f);
    nbdt::push_items(items, offsets[s], lengths[s], s, weight_decays[s]);
    end = offsets[s] + lengths[s];
  }
  if (n > end) nbdt::push_items(items, end, n - end, -1, 0.f);
  NBDT_REQUIRE(items.size() < (size_t)1 << 30, "arena too large");

  OptPlan* P = new OptPlan();
  P->n = n;
  P->n_items = (int)items.size();
  hipError_t e = hipGetDevice(&P->device);
  if (e == hipSuccess) e = hipMalloc((void**)&P->items, items.size() * sizeof(OptItem));
  if (e == hipSuccess) e = hipMemcpy(P->items, items.data(), items.size() * sizeof(OptItem), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (P->items) (void)hipFree(P->items);
    delete P;
    return nbdt::fail(NBDT_EHIP, "%s: %s", "nbdt_arena_opt_create: device table", hipGetErrorString(e));
  }
  *plan = P;
  return NBDT_OK;
}

extern "C" int nbdt_arena_opt_destroy(void* plan) {
  if (!plan) return NBDT_OK;
  OptPlan* P = (OptPlan*)plan;
  if (P->items) (void)hipFree(P->items);
  delete P;
  return NBDT_OK;
}

extern "C" int64_t nbdt_arena_opt_n(void* plan) { return plan ? ((OptPlan*)plan)->n : 0; }

// what both steps check after their own scalars: the plan, the pointers, the device
static int arena_opt_check(void* plan, const float* p, const float* g, const float* s1, bool need_s1, const float* s2,
                           const void* pb) {
  NBDT_REQUIRE(plan, "null plan");
  NBDT_REQUIRE(p && g && s2 && (s1 || !need_s1), "null flat buffer");
  NBDT_REQUIRE(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)s1 % 16) == 0 &&
                   ((uintptr_t)s2 % 16) == 0,
               "flat buffers must be 16-byte aligned");
  NBDT_REQUIRE(((uintptr_t)pb % 8) == 0, "the bf16 mirror must be 8-byte aligned");
  NBDT_REQUIRE(p != g && p != s2 && g != s2 && s1 != p && s1 != g && s1 != s2, "flat buffers must be distinct");
  int dev = 0;
  NBDT_HIP_CHECK(hipGetDevice(&dev));
  NBDT_REQUIRE(dev == ((OptPlan*)plan)->device, "the plan's tables live on another device");
  return NBDT_OK;
}

extern "C" int nbdt_adamw_step(void* plan, float* p, float* g, float* m, float* v, float lr, float beta1, float beta2,
                               float eps, int64_t t, float grad_scale, void* p_bf16, int32_t zero_grad, void* stream) {
  NBDT_REQUIRE(t >= 1, "the step count t starts at 1");
  NBDT_REQUIRE(nbdt::unit_interval(beta1) && nbdt::unit_interval(beta2), "betas must be in [0, 1)");
  NBDT_REQUIRE(eps >= 0.f, "eps must be >= 0");
  NBDT_REQUIRE(isfinite(lr) && isfinite(grad_scale), "lr and grad_scale must be finite");
  if (int rc = arena_opt_check(plan, p, g, m, true, v, p_bf16)) return rc;
  OptScalars c = {};
  c.lr = lr;
  c.gscale = grad_scale;
  c.eps = eps;
  c.b1 = beta1;
  c.b2 = beta2;
  c.omb1 = (float)(1.0 - (double)beta1);
  c.omb2 = (float)(1.0 - (double)beta2);
  c.ss = (float)((double)lr / (1.0 - pow((double)beta1, (double)t)));
  c.c2 = (float)sqrt(1.0 - pow((double)beta2, (double)t));
  nbdt::launch<nbdt::kAdamW>((OptPlan*)plan, p, g, m, v, c, p_bf16, zero_grad ? 1 : 0, (hipStream_t)stream);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_rmsprop_step(void* plan, float* p, float* g, float* sq, float* buf, float lr, float alpha, float eps,
                                 float momentum, int32_t tf, float grad_scale, void* p_bf16, int32_t zero_grad,
                                 void* stream) {
  NBDT_REQUIRE(nbdt::unit_interval(alpha) && nbdt::unit_interval(momentum), "alpha and momentum must be in [0, 1)");
  NBDT_REQUIRE(eps >= 0.f, "eps must be >= 0");
  NBDT_REQUIRE(isfinite(lr) && isfinite(grad_scale), "lr and grad_scale must be finite");
  const bool plain = !tf && momentum == 0.f;       // torch's form without momentum keeps no buffer
  if (int rc = arena_opt_check(plan, p, g, plain ? nullptr : buf, !plain, sq, p_bf16)) return rc;
  OptScalars c = {};
  c.lr = lr;
  c.gscale = grad_scale;
  c.eps = eps;
  c.alpha = alpha;
  c.oma = (float)(1.0 - (double)alpha);
  c.mu = momentum;
  OptPlan* P = (OptPlan*)plan;
  const int z = zero_grad ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (tf) nbdt::launch<nbdt::kRmspropTf>(P, p, g, buf, sq, c, p_bf16, z, st);
  else if (plain) nbdt::launch<nbdt::kRmspropPlain>(P, p, g, nullptr, sq, c, p_bf16, z, st);
  else nbdt::launch<nbdt::kRmsprop>(P, p, g, buf, sq, c, p_bf16, z, st);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}
