// AdamW (torch.optim.AdamW, no amsgrad) and RMSprop (torch.optim.RMSprop, not centered; and TensorFlow's form, the one
// EfficientNet was trained with) over the flat parameter arena of nbdt.engine.ParamStore, on gfx950.
//
// One launch per step: arena.h's streaming pass (arena_update: one WAVE per item of the plan's update table) over two
// state arenas, or one for RMSprop without momentum.  34 bytes per element with momentum (read p, g and two states,
// write p, two states, the mirror and g), against 26 of the SGD pass.  Nothing crosses a lane, so where the items are
// cut does not change a bit, and neither does nbdt_set_deterministic.
// This file's own: the item size, the element updates of the four modes, the scalars each step entry checks and forms,
// and the refusal of a negative or non-finite decay.  The table check, the item record and the table, the streaming
// pass, the step entries' pointer checks and the plan's device memory are arena.h's.
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
#include "arena.h"

#include <math.h>

namespace nbdt {
namespace {

constexpr int kItem = 512;           // elements per wave item: 2 iterations of 64 lanes x 16 bytes (measured: above)

struct OptPlan : ArenaPlan {         // the blob: the update table
  using ArenaPlan::ArenaPlan;
  int n_items = 0;
  ArenaItem* items = nullptr;
};

enum Mode { kAdamW = 0, kRmsprop = 1, kRmspropPlain = 2, kRmspropTf = 3 };   // Plain: momentum == 0, no buffer

struct OptScalars {   // fp32 values as include/nbdt_hip.h forms them
  float lr, gscale, eps;
  float b1, omb1, b2, omb2, ss, c2;  // AdamW
  float alpha, oma, mu;              // RMSprop
};

// arena.h's functor contract.  s1: m (AdamW) or the momentum buffer; s2: v or the mean square, which for Plain is the
// one state arena.  k: 1 - lr wd of the segment (AdamW), formed once per item.
template <int MODE>
struct OptUpdate {
  static constexpr int kStates = MODE == kRmspropPlain ? 1 : 2;
  typedef OptScalars Params;
  const OptScalars& c;
  const float wd, k;
  __device__ OptUpdate(const OptScalars& c_, const ArenaItem& it) : c(c_), wd(it.wd), k(1.f - c_.lr * it.wd) {}
  __device__ __forceinline__ void operator()(float& p, float g, float& s1, float& b) const {
    float& s2 = kStates == 2 ? b : s1;
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
};

template <int MODE>
__global__ __launch_bounds__(256) void arena_opt_kernel(float* __restrict__ p, float* __restrict__ g,
                                                        float* __restrict__ s0, float* __restrict__ s1,
                                                        const ArenaItem* __restrict__ items, int n_items, OptScalars c,
                                                        bf16_t* __restrict__ pb, int zero_g) {
  arena_update<OptUpdate<MODE>>(p, g, s0, s1, items, n_items, c, pb, zero_g);
}

bool unit_interval(float x) { return x >= 0.f && x < 1.f; }    // false for NaN

// s0, s1: the state arenas in the functor's order (Plain: the mean square, nothing)
template <int MODE>
void launch(const OptPlan* P, float* p, float* g, float* s0, float* s1, const OptScalars& c, void* pb, int zero_g,
            hipStream_t st) {
  const int w = kWavesPerBlock;
  hipLaunchKernelGGL(arena_opt_kernel<MODE>, dim3((unsigned)((P->n_items + w - 1) / w)), dim3(256), 0, st, p, g, s0, s1,
                     P->items, P->n_items, c, (bf16_t*)pb, zero_g);
}

}  // namespace
}  // namespace nbdt

using nbdt::OptPlan;
using nbdt::OptScalars;

extern "C" int nbdt_arena_opt_create(int64_t n, const int64_t* offsets, const int64_t* lengths,
                                     const float* weight_decays, int32_t n_seg, void** plan) {
  if (int rc = nbdt::check_segment_table(n, offsets, lengths, weight_decays != nullptr, n_seg, plan, [&](int s) {
        NBDT_REQUIRE(weight_decays[s] >= 0.f && weight_decays[s] <= 3.0e38f, "weight decays must be finite and >= 0");
        return NBDT_OK;
      }))
    return rc;
  std::vector<nbdt::ArenaItem> items;
  if (int rc = nbdt::update_items(items, nbdt::kItem, n, offsets, lengths, weight_decays, n_seg)) return rc;
  OptPlan* P = new OptPlan(n, items.size() * sizeof(nbdt::ArenaItem));
  P->n_items = (int)items.size();
  P->items = P->blob.put(0, items);
  return nbdt::finish_plan(P, "nbdt_arena_opt_create: device table", plan);
}

extern "C" int nbdt_arena_opt_destroy(void* plan) {
  delete (OptPlan*)plan;
  return NBDT_OK;
}

extern "C" int64_t nbdt_arena_opt_n(void* plan) { return plan ? ((OptPlan*)plan)->n : 0; }

extern "C" int nbdt_adamw_step(void* plan, float* p, float* g, float* m, float* v, float lr, float beta1, float beta2,
                               float eps, int64_t t, float grad_scale, void* p_bf16, int32_t zero_grad, void* stream) {
  NBDT_REQUIRE(t >= 1, "the step count t starts at 1");
  NBDT_REQUIRE(nbdt::unit_interval(beta1) && nbdt::unit_interval(beta2), "betas must be in [0, 1)");
  NBDT_REQUIRE(eps >= 0.f, "eps must be >= 0");
  NBDT_REQUIRE(isfinite(lr) && isfinite(grad_scale), "lr and grad_scale must be finite");
  if (int rc = nbdt::check_step((OptPlan*)plan, p, g, m, v, 2, p_bf16, true)) return rc;
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
  OptPlan* P = (OptPlan*)plan;
  if (int rc = plain ? nbdt::check_step(P, p, g, sq, nullptr, 1, p_bf16, true)
                     : nbdt::check_step(P, p, g, buf, sq, 2, p_bf16, true))
    return rc;
  OptScalars c = {};
  c.lr = lr;
  c.gscale = grad_scale;
  c.eps = eps;
  c.alpha = alpha;
  c.oma = (float)(1.0 - (double)alpha);
  c.mu = momentum;
  const int z = zero_grad ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (tf) nbdt::launch<nbdt::kRmspropTf>(P, p, g, buf, sq, c, p_bf16, z, st);
  else if (plain) nbdt::launch<nbdt::kRmspropPlain>(P, p, g, sq, nullptr, c, p_bf16, z, st);
  else nbdt::launch<nbdt::kRmsprop>(P, p, g, buf, sq, c, p_bf16, z, st);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

