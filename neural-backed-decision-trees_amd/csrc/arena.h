// What the optimizer passes over the flat parameter arena of nbdt.engine.ParamStore share (lars.hip, adaptive.hip; the
// device blob also clip.hip): the check of a segment table, the wave-item table cut from it, the streaming update every
// wave runs over its item, the check of a step entry's arguments and the owner of a plan's device memory.  Internal:
// nothing here is exported, and each including file's own flags (nbdt/_build.py) govern its instantiations.
//
// The update functor F of arena_update<F>:
//   static constexpr int kStates      state arenas that take part beside p and g: 0, 1 or 2
//   F(params, item)                   on the device, once per wave item: the wave-uniform scalars of the item's segment
//   void operator()(float& p, float g, float& a, float& b) const
//                                     ONE element: p and the states a (arena 0), b (arena 1) updated in place; a state
//                                     beyond kStates is a dummy.  The sequence of fp32 operations written here is the
//                                     arithmetic of the pass, for the float4 body and the scalar tail alike.
#pragma once
#include "common.h"

#include <vector>

namespace nbdt {
namespace {

constexpr int kWavesPerBlock = 4;

struct ArenaItem {
  long long start;   // first element (a multiple of 4 for segment items; anything for gap items)
  int len;           // 1..item size
  int seg;           // segment index, or -1: a gap (only ever zeroed in g)
  float wd;          // the segment's weight decay
  int pad;
};

// ---------------------------------------------------------------------------------------------------------- host
// What every *_create checks before it reads the table: rows sorted by offset, disjoint, offsets multiples of 4, inside
// [0, n).  columns: the caller's own columns (decays, adapt flags) are there.  row_check(s): a refusal of the caller's
// own for row s, made after the shared ones of that row.
template <class RowCheck>
int check_segment_table(int64_t n, const int64_t* offsets, const int64_t* lengths, bool columns, int32_t n_seg,
                        void** plan, RowCheck row_check) {
  NBDT_REQUIRE(plan, "null plan pointer");
  *plan = nullptr;
  NBDT_REQUIRE(offsets && lengths && columns, "null segment table");
  NBDT_REQUIRE(n_seg > 0, "empty segment table");
  NBDT_REQUIRE(n > 0, "empty arena");
  long long end = 0;                 // end of the previous row
  for (int s = 0; s < n_seg; ++s) {
    NBDT_REQUIRE(lengths[s] > 0, "segment lengths must be positive");
    NBDT_REQUIRE(offsets[s] >= 0 && offsets[s] % 4 == 0, "segment offsets must be multiples of 4 elements");
    if (s > 0) NBDT_REQUIRE(offsets[s] >= offsets[s - 1], "segment rows must be sorted by offset");
    NBDT_REQUIRE(offsets[s] >= end, "segment rows overlap");
    NBDT_REQUIRE(lengths[s] <= n && offsets[s] <= n - lengths[s], "segment runs out of range");
    if (int rc = row_check(s)) return rc;
    end = offsets[s] + lengths[s];
  }
  return NBDT_OK;
}

// [start, start + len) in items of at most `item` elements
inline void push_items(std::vector<ArenaItem>& v, int item, long long start, long long len, int seg, float wd) {
  for (long long o = 0; o < len; o += item) {
    const long long l = len - o < item ? len - o : item;
    v.push_back(ArenaItem{start + o, (int)l, seg, wd, 0});
  }
}

// the update table of a checked segment table: every segment in offset order, and the gaps between the segments and
// the arena's tail as items that only zero the gradient
inline int update_items(std::vector<ArenaItem>& v, int item, int64_t n, const int64_t* offsets, const int64_t* lengths,
                        const float* weight_decays, int32_t n_seg) {
  long long end = 0;
  for (int s = 0; s < n_seg; ++s) {
    if (offsets[s] > end) push_items(v, item, end, offsets[s] - end, -1, 0.f);
    push_items(v, item, offsets[s], lengths[s], s, weight_decays[s]);
    end = offsets[s] + lengths[s];
  }
  if (n > end) push_items(v, item, end, n - end, -1, 0.f);
  NBDT_REQUIRE(v.size() < (size_t)1 << 30, "arena too large");
  return NBDT_OK;
}

// A plan's one device allocation, on the device that is current when the plan is made.  The first failing call stays in
// err and turns the later ones into no-ops; the memory goes with the plan.
struct DeviceBlob {
  char* base = nullptr;
  int device = 0;
  hipError_t err;
  explicit DeviceBlob(size_t bytes) {
    err = hipGetDevice(&device);
    if (err == hipSuccess) err = hipMalloc((void**)&base, bytes);
  }
  DeviceBlob(const DeviceBlob&) = delete;
  DeviceBlob& operator=(const DeviceBlob&) = delete;
  ~DeviceBlob() {
    if (base) (void)hipFree(base);
  }
  // `bytes` of host memory to base + off; returns that device address
  void* put(size_t off, const void* src, size_t bytes) {
    if (err == hipSuccess && bytes) err = hipMemcpy(base + off, src, bytes, hipMemcpyHostToDevice);
    return base + off;
  }
  template <class T>
  T* put(size_t off, const std::vector<T>& v) { return (T*)put(off, v.data(), v.size() * sizeof(T)); }
};

struct ArenaPlan {                   // what every plan over the arena starts with
  long long n;
  DeviceBlob blob;
  ArenaPlan(long long n_, size_t bytes) : n(n_), blob(bytes) {}
};

// the end of a *_create: the plan when its blob was filled, else the HIP error under `what` and no plan
template <class Plan>
int finish_plan(Plan* P, const char* what, void** out) {
  const hipError_t e = P->blob.err;
  if (e != hipSuccess) {
    delete P;
    return fail(NBDT_EHIP, "%s: %s", what, hipGetErrorString(e));
  }
  *out = P;
  return NBDT_OK;
}

// What a step entry checks after its own scalars: the plan, the fp32 arenas (n_states of a, b take part), the mirror,
// and with `distinct` that no two arenas are one; then the plan's device.
inline int check_step(const ArenaPlan* plan, const float* p, const float* g, const float* a, const float* b,
                      int n_states, const void* pb, bool distinct) {
  NBDT_REQUIRE(plan, "null plan");
  NBDT_REQUIRE(p && g && (a || n_states < 1) && (b || n_states < 2), "null flat buffer");
  NBDT_REQUIRE(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)a % 16) == 0 &&
                   ((uintptr_t)b % 16) == 0,
               "flat buffers must be 16-byte aligned");
  NBDT_REQUIRE(((uintptr_t)pb % 8) == 0, "the bf16 mirror must be 8-byte aligned");
  if (distinct)
    NBDT_REQUIRE(p != g && p != a && p != b && g != a && g != b && a != b, "flat buffers must be distinct");
  int dev = 0;
  NBDT_HIP_CHECK(hipGetDevice(&dev));
  NBDT_REQUIRE(dev == plan->blob.device, "the plan's tables live on another device");
  return NBDT_OK;
}

// -------------------------------------------------------------------------------------------------------- device
// One WAVE per item: 16-byte accesses with every arena loaded before the first store, the bf16 mirror and the zeroed
// gradient written in the same pass, a scalar tail for length % 4 (the last item of a segment).  s0 / s1: the state
// arenas, read and written only below F::kStates.  Nothing crosses a lane.
template <class F>
__device__ __forceinline__ void arena_update(float* __restrict__ p, float* __restrict__ g, float* __restrict__ s0,
                                             float* __restrict__ s1, const ArenaItem* __restrict__ items, int n_items,
                                             const typename F::Params& c, bf16_t* __restrict__ pb, int zero_g) {
  constexpr bool kA = F::kStates >= 1, kB = F::kStates >= 2;
  const int item = blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (item >= n_items) return;
  const int lane = threadIdx.x & 63;
  const ArenaItem it = items[item];
  if (it.seg < 0) {                  // a gap between segments, or the arena's tail: nothing but g is touched
    if (zero_g)
      for (int i = lane; i < it.len; i += 64) g[it.start + i] = 0.f;
    return;
  }
  const F f(c, it);
  float4* p4 = (float4*)(p + it.start);
  float4* g4 = (float4*)(g + it.start);
  float4* a4 = kA ? (float4*)(s0 + it.start) : nullptr;
  float4* b4 = kB ? (float4*)(s1 + it.start) : nullptr;
  uint2* pb2 = pb ? (uint2*)(pb + it.start) : nullptr;
  const int n4 = it.len >> 2;
  for (int i = lane; i < n4; i += 64) {
    float4 pv = p4[i];
    const float4 gv = g4[i];
    float4 av = {0.f, 0.f, 0.f, 0.f}, bv = {0.f, 0.f, 0.f, 0.f};
    if (kA) av = a4[i];
    if (kB) bv = b4[i];
    f(pv.x, gv.x, av.x, bv.x);
    f(pv.y, gv.y, av.y, bv.y);
    f(pv.z, gv.z, av.z, bv.z);
    f(pv.w, gv.w, av.w, bv.w);
    if (kA) a4[i] = av;
    if (kB) b4[i] = bv;
    p4[i] = pv;
    if (zero_g) g4[i] = float4{0.f, 0.f, 0.f, 0.f};
    if (pb2) pb2[i] = bf16x4_of(pv);
  }
  if (lane < (it.len & 3)) {         // tail (length % 4) of the segment's last item
    const long long i = it.start + ((long long)n4 << 2) + lane;
    float pv = p[i], av = kA ? s0[i] : 0.f, bv = kB ? s1[i] : 0.f;
    f(pv, g[i], av, bv);
    if (kA) s0[i] = av;
    if (kB) s1[i] = bv;
    p[i] = pv;
    if (zero_g) g[i] = 0.f;
    if (pb) pb[i] = f32_to_bf16(pv);
  }
}

}  // namespace
}  // namespace nbdt
