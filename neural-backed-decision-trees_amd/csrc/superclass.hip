// Zero-shot superclass evaluation and ad-hoc class groupings on gfx950.
//
// Replaces, for a grouping of the classifier's classes that no hierarchy node stands for,
//   get_node_logits(new_to_old_classes=...) ... nbdt/model.py:84-99     (one gather + mean per group)
//   Superclass.forward / _update_batch ........ nbdt/analysis.py:510-535 (boolean-mask compaction, a -100 fill of a
//                                               copy of the logits, max, a .item() per batch)
//   SuperclassNBDT.forward .................... nbdt/analysis.py:545-559
// by one launch per call and no host read-back: nbdt_superclass_accumulate adds one batch into int64 counters on the
// device, as nbdt_tree_stats_accumulate does for the tree diagnostics.
//
// Layout.  One block of kBlock lanes owns one sample at a time (a grid-stride loop over the batch).  The group means
// are ordered fp32 chains, which cannot be split, but their indirection can: the flattened member list (all groups end
// to end, nbdt_groups::group_cls) is walked in chunks of kChunk entries; every lane gathers z[group_cls[j]] into an LDS
// staging row (coalesced index reads), then lane g folds the part of group g that lies in the chunk, contiguous LDS.
// Groups are taken kBlock at a time, so a lane carries one accumulator in a register whatever G is.  Nothing is sized
// by C, G or the member count: the staging row is 8 KB of static LDS and there is NO size limit (C = 21,841 runs as
// C = 10 does).  With G = 2 two lanes of the block fold while the others wait at the barrier; the launch is bounded by
// the longest chain (members of the largest group x one dependent LDS read + add), not by bandwidth.
//
// Arithmetic contract (oracle/nbdt_oracle.py, rules.hip): a group's logit is the sequential fp32 sum of its members in
// the LISTED order, starting from 0.0f, then one IEEE division by the member count (0 / 0 = NaN for an empty group);
// bf16 / fp16 inputs are widened exactly.  The maximum is torch's: a NaN is the largest value, and among equal values
// the lowest index wins.  The backward term of group g is gs / n_g (one division), the terms of a class are added in
// ascending group index starting from 0.0f.  No floating-point atomics anywhere: the only atomics add integers.
// Compiled with -ffp-contract=off and correctly rounded division.  Every row offset (b * ldz, b * G, b * C) is 64-bit.
#include "common.h"

#include <algorithm>
#include <vector>

using namespace nbdt;

struct nbdt_groups {
  int device, cus;
  int C, G, L;           // classes, groups, members of all groups together
  int32_t* d_all;        // one allocation
  const int32_t *group_off, *group_cls;   // [G+1], [L]: members of group g in the listed order
  const int32_t *cls_off, *cls_grp;       // [C+1], [L]: groups holding class c, ascending
};

namespace {

struct GroupView {
  int C, G, L;
  const int32_t *group_off, *group_cls, *cls_off, *cls_grp;
};

GroupView view_of(const nbdt_groups* g) {
  GroupView v;
  v.C = g->C; v.G = g->G; v.L = g->L;
  v.group_off = g->group_off; v.group_cls = g->group_cls; v.cls_off = g->cls_off; v.cls_grp = g->cls_grp;
  return v;
}

struct LoadF32 { static __device__ __forceinline__ float at(const void* p, int64_t i) { return ((const float*)p)[i]; } };
struct LoadBF16 { static __device__ __forceinline__ float at(const void* p, int64_t i) { return bf16_to_f32(((const bf16_t*)p)[i]); } };
struct LoadF16 { static __device__ __forceinline__ float at(const void* p, int64_t i) { return __half2float(((const __half*)p)[i]); } };

constexpr int kBlock = 256;
constexpr int kChunk = 2048;     // floats of the staging row
constexpr int kNone = 0x7fffffff;

// torch's max over a row: NaN is the largest value, the lowest index wins among equals
struct Best {
  float v;
  int i;
};
__device__ __forceinline__ bool beats(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an != bn) return an;
  if (!an && av != bv) return av > bv;
  return ai < bi;
}
__device__ __forceinline__ void take(Best& b, float v, int i) {
  if (beats(v, i, b.v, b.i)) { b.v = v; b.i = i; }
}

// the block's best in every lane.  red: 2 * (kBlock / 64) words of LDS.
__device__ __forceinline__ Best block_best(Best b, float* red_v, int* red_i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(b.v, o, 64);
    const int oi = __shfl_xor(b.i, o, 64);
    take(b, ov, oi);
  }
  __syncthreads();               // (the previous sample's readers are done with red)
  if ((threadIdx.x & 63) == 0) { red_v[threadIdx.x >> 6] = b.v; red_i[threadIdx.x >> 6] = b.i; }
  __syncthreads();
  Best r = {red_v[0], red_i[0]};
#pragma unroll
  for (int w = 1; w < kBlock / 64; ++w) take(r, red_v[w], red_i[w]);
  return r;
}

// The means of groups [g0, g0 + kBlock) of one sample: lane l returns group g0 + l's (anything when g0 + l >= G).
// Every lane of the block must call it.  zrow: element offset of the sample's row.
template <typename LD>
__device__ __forceinline__ float group_means(const GroupView& t, const void* z, int64_t zrow, int g0, float* stage) {
  const int g = g0 + (int)threadIdx.x;
  const int gend = min(g0 + kBlock, t.G);
  const int lo = g < t.G ? t.group_off[g] : 0, hi = g < t.G ? t.group_off[g + 1] : 0;
  const int first = t.group_off[g0], last = t.group_off[gend];     // block-uniform
  float acc = 0.f;
  for (int k0 = first; k0 < last; k0 += kChunk) {
    const int k1 = min(k0 + kChunk, last);
    __syncthreads();             // the previous chunk's chains are done with the row
    for (int j = k0 + (int)threadIdx.x; j < k1; j += kBlock) stage[j - k0] = LD::at(z, zrow + t.group_cls[j]);
    __syncthreads();
    const int a = max(lo, k0), b = min(hi, k1);
    // the adds are one dependent chain, the LDS reads are not: eight reads in flight per eight adds, same order
    int j = a;
    for (; j + 8 <= b; j += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = stage[j - k0 + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; j < b; ++j) acc += stage[j - k0];
  }
  return acc / (float)(hi - lo);
}

template <typename LD>
__global__ __launch_bounds__(kBlock) void group_logits_kernel(GroupView t, const void* z, int64_t B, int64_t ldz,
                                                              float* __restrict__ out) {
  __shared__ float stage[kChunk];
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x)
    for (int g0 = 0; g0 < t.G; g0 += kBlock) {
      const float m = group_means<LD>(t, z, b * ldz, g0, stage);
      if (g0 + (int)threadIdx.x < t.G) out[b * t.G + g0 + threadIdx.x] = m;
    }
}

// gz[b][c] = sum over the groups g holding c, ascending g, of gs[b][g] / n_g.  One lane per element, every element written.
__global__ __launch_bounds__(kBlock) void group_logits_bwd_kernel(GroupView t, const float* __restrict__ gs, int64_t B,
                                                                  float* __restrict__ gz) {
  const int64_t n = B * t.C;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int64_t b = i / t.C;
    const int c = (int)(i - b * t.C);
    float acc = 0.f;
    for (int j = t.cls_off[c]; j < t.cls_off[c + 1]; ++j) {
      const int g = t.cls_grp[j];
      acc += gs[b * t.G + g] / (float)(t.group_off[g + 1] - t.group_off[g]);
    }
    gz[i] = acc;
  }
}

template <typename LD, int MODE>
__global__ __launch_bounds__(kBlock) void superclass_kernel(GroupView t, const void* z, int64_t B, int64_t ldz,
                                                            const int64_t* __restrict__ y,
                                                            const int32_t* __restrict__ map_target, int C_test,
                                                            const int32_t* __restrict__ map_pred,
                                                            unsigned long long* totals, unsigned long long* confusion,
                                                            int64_t* __restrict__ pred) {
  __shared__ float stage[kChunk];
  __shared__ float red_v[kBlock / 64];
  __shared__ int red_i[kBlock / 64];
  unsigned long long seen = 0, right = 0;      // lane 0's: the block's share of totals
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t zrow = b * ldz;
    Best best = {-INFINITY, kNone};
    if (MODE == NBDT_SUPER_MASKED) {
      // the reference writes -100 over the unmapped columns of a copy, then takes the row's max
      for (int c = threadIdx.x; c < t.C; c += kBlock) take(best, map_pred[c] < 0 ? -100.0f : LD::at(z, zrow + c), c);
    } else {
      for (int g0 = 0; g0 < t.G; g0 += kBlock) {
        const float m = group_means<LD>(t, z, zrow, g0, stage);
        if (g0 + (int)threadIdx.x < t.G) take(best, m, g0 + (int)threadIdx.x);
      }
    }
    best = block_best(best, red_v, red_i);
    if (threadIdx.x == 0) {
      int p = best.i == kNone ? 0 : best.i;
      if (MODE == NBDT_SUPER_MASKED) p = map_pred[p];
      if (pred) pred[b] = p;
      const int64_t label = y[b];
      const int tg = (label >= 0 && label < C_test) ? map_target[label] : -1;
      if (tg >= 0 && tg < t.G) {
        ++seen;
        right += p == tg;
        if (confusion && p >= 0 && p < t.G) atomicAdd(confusion + (int64_t)tg * t.G + p, 1ull);
      }
    }
  }
  if (threadIdx.x == 0 && seen) {
    atomicAdd(totals, seen);
    if (right) atomicAdd(totals + 1, right);
  }
}

unsigned sample_grid(const nbdt_groups* g, int64_t B) {
  return (unsigned)std::min<int64_t>(B, 8 * (int64_t)std::max(g->cus, 1));
}

int check_rows(const nbdt_groups* g, const void* z, int ztype, int64_t B, int64_t ldz) {
  NBDT_REQUIRE(g != nullptr, "null grouping handle");
  NBDT_REQUIRE(z != nullptr || B == 0, "null logits");
  NBDT_REQUIRE(ztype == NBDT_F32 || ztype == NBDT_BF16 || ztype == NBDT_F16, "unsupported logits dtype");
  NBDT_REQUIRE(B >= 0 && ldz >= g->C, "bad batch / row stride");
  return NBDT_OK;
}

}  // namespace

extern "C" int nbdt_groups_create(int device, int C, int G, const int32_t* group_off, const int32_t* group_cls,
                                  nbdt_groups** out) {
  NBDT_REQUIRE(out && group_off, "null argument");
  NBDT_REQUIRE(C > 0 && G > 0, "bad grouping sizes");
  NBDT_REQUIRE(group_off[0] == 0, "group_off must start at 0");
  for (int g = 0; g < G; ++g) NBDT_REQUIRE(group_off[g + 1] >= group_off[g], "group_off must not decrease");
  const int L = group_off[G];
  NBDT_REQUIRE(L == 0 || group_cls != nullptr, "null member list");
  // the transposed map, and the two refusals: a class index outside [0, C), a class twice within one group
  std::vector<int32_t> count(C + 1, 0), seen_in(C, -1);
  for (int g = 0; g < G; ++g)
    for (int j = group_off[g]; j < group_off[g + 1]; ++j) {
      const int c = group_cls[j];
      if (c < 0 || c >= C) {
        snprintf(g_err, sizeof(g_err), "group %d lists class index %d, outside [0, %d)", g, c, C);
        return NBDT_EINVAL;
      }
      if (seen_in[c] == g) {
        snprintf(g_err, sizeof(g_err), "group %d lists class %d twice", g, c);
        return NBDT_EINVAL;
      }
      seen_in[c] = g;
      ++count[c + 1];
    }
  std::vector<int32_t> cls_off(C + 1, 0), cls_grp((size_t)std::max(L, 1));
  for (int c = 0; c < C; ++c) cls_off[c + 1] = cls_off[c] + count[c + 1];
  std::vector<int32_t> fill(cls_off.begin(), cls_off.end() - 1);
  for (int g = 0; g < G; ++g)      // ascending g, so every class's list comes out ascending
    for (int j = group_off[g]; j < group_off[g + 1]; ++j) cls_grp[fill[group_cls[j]]++] = g;

  int prev = 0;
  NBDT_HIP_CHECK(hipGetDevice(&prev));
  NBDT_HIP_CHECK(hipSetDevice(device));
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 1;
  nbdt_groups* h = new nbdt_groups();
  h->device = device; h->cus = cus; h->C = C; h->G = G; h->L = L;
  const size_t n_ints = (size_t)(G + 1) + (size_t)(C + 1) + 2 * (size_t)L;
  hipError_t e = hipMalloc((void**)&h->d_all, n_ints * sizeof(int32_t));
  if (e != hipSuccess) {
    delete h;
    (void)hipSetDevice(prev);
    return nbdt::fail(NBDT_ENOMEM, "hipMalloc(groups): %s", hipGetErrorString(e));
  }
  std::vector<int32_t> host(n_ints);
  size_t o = 0;
  auto put = [&](const int32_t* src, size_t n, const int32_t** dst) {
    if (n) memcpy(host.data() + o, src, n * sizeof(int32_t));
    *dst = h->d_all + o;
    o += n;
  };
  put(group_off, G + 1, &h->group_off);
  put(group_cls, L, &h->group_cls);
  put(cls_off.data(), C + 1, &h->cls_off);
  put(cls_grp.data(), L, &h->cls_grp);
  e = hipMemcpy(h->d_all, host.data(), n_ints * sizeof(int32_t), hipMemcpyHostToDevice);
  (void)hipSetDevice(prev);
  if (e != hipSuccess) {
    (void)hipFree(h->d_all);
    delete h;
    return nbdt::fail(NBDT_EHIP, "hipMemcpy(groups): %s", hipGetErrorString(e));
  }
  *out = h;
  return NBDT_OK;
}

extern "C" int nbdt_groups_destroy(nbdt_groups* g) {
  if (!g) return NBDT_OK;
  (void)hipFree(g->d_all);
  delete g;
  return NBDT_OK;
}

extern "C" int nbdt_group_logits(const nbdt_groups* g, const void* z, int ztype, int64_t B, int64_t ldz, float* out,
                                 void* stream) {
  int rc = check_rows(g, z, ztype, B, ldz);
  if (rc) return rc;
  if (B == 0) return NBDT_OK;
  NBDT_REQUIRE(out != nullptr, "null output");
  const GroupView v = view_of(g);
  const dim3 grid(sample_grid(g, B)), block(kBlock);
  hipStream_t st = (hipStream_t)stream;
  if (ztype == NBDT_F32) hipLaunchKernelGGL(group_logits_kernel<LoadF32>, grid, block, 0, st, v, z, B, ldz, out);
  else if (ztype == NBDT_BF16) hipLaunchKernelGGL(group_logits_kernel<LoadBF16>, grid, block, 0, st, v, z, B, ldz, out);
  else hipLaunchKernelGGL(group_logits_kernel<LoadF16>, grid, block, 0, st, v, z, B, ldz, out);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_group_logits_backward(const nbdt_groups* g, const float* gs, int64_t B, float* gz, void* stream) {
  NBDT_REQUIRE(g != nullptr, "null grouping handle");
  NBDT_REQUIRE(B >= 0, "bad batch");
  if (B == 0) return NBDT_OK;
  NBDT_REQUIRE(gs && gz, "null gradient buffer");
  const int64_t n = B * g->C;
  const int64_t blocks = std::min<int64_t>((n + kBlock - 1) / kBlock, 64 * (int64_t)std::max(g->cus, 1));
  hipLaunchKernelGGL(group_logits_bwd_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, view_of(g),
                     gs, B, gz);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_superclass_accumulate(const nbdt_groups* g, const void* z, int ztype, int64_t B, int64_t ldz,
                                          const int64_t* y, const int32_t* map_target, int32_t C_test,
                                          const int32_t* map_pred, int32_t mode, int64_t* totals, int64_t* confusion,
                                          int64_t* pred, void* stream) {
  int rc = check_rows(g, z, ztype, B, ldz);
  if (rc) return rc;
  NBDT_REQUIRE(mode == NBDT_SUPER_MASKED || mode == NBDT_SUPER_GROUP_MEAN, "mode must be NBDT_SUPER_MASKED or NBDT_SUPER_GROUP_MEAN");
  NBDT_REQUIRE(C_test > 0 && map_target != nullptr, "the target mapping is required");
  NBDT_REQUIRE(mode != NBDT_SUPER_MASKED || map_pred != nullptr, "the masked mode needs map_pred");
  NBDT_REQUIRE(totals != nullptr, "null totals");
  if (B == 0) return NBDT_OK;
  NBDT_REQUIRE(y != nullptr, "null labels");
  const GroupView v = view_of(g);
  const dim3 grid(sample_grid(g, B)), block(kBlock);
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* tot = (unsigned long long*)totals;
  unsigned long long* conf = (unsigned long long*)confusion;
#define NBDT_SUPER_LAUNCH(LD)                                                                                       \
  do {                                                                                                              \
    if (mode == NBDT_SUPER_MASKED)                                                                                  \
      hipLaunchKernelGGL((superclass_kernel<LD, NBDT_SUPER_MASKED>), grid, block, 0, st, v, z, B, ldz, y,           \
                         map_target, (int)C_test, map_pred, tot, conf, pred);                                       \
    else                                                                                                            \
      hipLaunchKernelGGL((superclass_kernel<LD, NBDT_SUPER_GROUP_MEAN>), grid, block, 0, st, v, z, B, ldz, y,       \
                         map_target, (int)C_test, map_pred, tot, conf, pred);                                       \
  } while (0)
  if (ztype == NBDT_F32) NBDT_SUPER_LAUNCH(LoadF32);
  else if (ztype == NBDT_BF16) NBDT_SUPER_LAUNCH(LoadBF16);
  else NBDT_SUPER_LAUNCH(LoadF16);
#undef NBDT_SUPER_LAUNCH
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}
