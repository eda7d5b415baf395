// Per-channel reduction plumbing of the BatchNorm kernels, shared by bn.hip and effnet.hip (built with the same flags):
// the 32 replicated slot accumulators, their deterministic-mode twin, the block fold in front of them and the backward
// finalize kernel behind them.  The zero-on-entry slot contract, the row-per-block deterministic mode and the fixed fold
// orders below are what the bit-exact tests rest on; this is their only copy.  Everything has internal linkage (the
// library is not built with relocatable device code, and both translation units instantiate the finalize kernel).
#pragma once
#include "common.h"

namespace nbdt {
namespace {

constexpr int kSlots = NBDT_BN_SLOTS;

// a padded NHWC tensor of C channels the streaming kernels can walk: 8-channel chunks, at most 256 of them per block
int check_shape(int B, int H, int W, int C) {
  NBDT_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "empty tensor");
  NBDT_REQUIRE(C % 8 == 0 && C / 8 <= 256, "C must be a multiple of 8 and <= 2048");
  NBDT_REQUIRE((long long)B * (H + 2) * (W + 2) * C < (1ll << 31), "padded tensor elements: B * (H+2) * (W+2) * C must stay below 2^31 (32-bit element offsets)");
  return NBDT_OK;
}

// the same without the 256-chunk limit: for entry points whose kernels index channels by a grid dimension, or that launch
// the streaming kernels once per channel range (effnet.hip: chan_slices)
int check_shape_wide(int B, int H, int W, int C) {
  NBDT_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "empty tensor");
  NBDT_REQUIRE(C % 8 == 0, "C must be a multiple of 8");
  NBDT_REQUIRE((long long)B * (H + 2) * (W + 2) * C < (1ll << 31), "padded tensor elements: B * (H+2) * (W+2) * C must stay below 2^31 (32-bit element offsets)");
  return NBDT_OK;
}

// fold NQ*8 per-thread partials over the PY pixel rows of the block and hand every sum to `sink(q, channel, value)`.
// lds: [PY][c8][NQ*8] floats.  Output o = q * (c8*8) + channel goes to thread o % (c8*PY): CONSECUTIVE THREADS HOLD
// CONSECUTIVE CHANNELS, so the sinks' global atomics are one contiguous 256-byte run per wave (thread (cx, py) folding
// element e = py, py+PY, ... of ITS chunk put a wave's lanes 32 bytes apart -- 64 sectors per atomic instruction once
// c8 >= 64; that, not the arithmetic, was most of the time of every statistics / weight-gradient kernel of effnet.hip on
// the narrow late layers: profiles/r04_dw_wgrad.txt).  Each sum is its PY partials in ascending row order.
template <int NQ, typename Sink>
__device__ __forceinline__ void block_fold(float (&acc)[NQ][8], int cx, int py, int c8, int PY, float* lds,
                                           Sink sink) {
  float* mine = lds + ((size_t)py * c8 + cx) * (NQ * 8);
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int i = 0; i < 8; ++i) mine[q * 8 + i] = acc[q][i];
  __syncthreads();
  const int nch = c8 * 8, nthr = c8 * PY;
  for (int o = py * c8 + cx; o < NQ * nch; o += nthr) {
    const int q = o / nch, c = o - q * nch;
    const float* src = lds + (size_t)(c >> 3) * (NQ * 8) + q * 8 + (c & 7);
    float s = 0.f;
    for (int r = 0; r < PY; ++r) s += src[(size_t)r * c8 * (NQ * 8)];
    sink(q, c, s);
  }
}

// The slot sink: sum q of channel c of a block's fold goes to scratch[slot][q][c], slot = the block's linear index &
// slot_mask.  slot_mask = kSlots - 1: the 32 replicated accumulators (several blocks add to one slot, in whatever order
// they finish -- no same-address pile-up); slot_mask = ~0 (deterministic mode): `scratch` is a zeroed row per BLOCK,
// every address receives exactly one add, and det_fold() sums the rows in block order.
template <int NQ>
__device__ __forceinline__ void slot_add(float* scratch, unsigned slot, int C, int q, int c, float s) {
  atomicAdd(scratch + ((size_t)slot * NQ + q) * C + c, s);
}

// Backward sums out of the slots: dsum[0][c] = sum g', dsum[1][c] = sum g'*xhat (slots in ascending order), added to
// dbeta / dgamma; leaves the 32 slots zeroed for the next user.
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(float* __restrict__ scratch, int C,
                                                              float* __restrict__ dsum,
                                                              float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta) {
  for (int c = blockIdx.x * 256 + threadIdx.x; c < C; c += gridDim.x * 256) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll 8
    for (int k = 0; k < kSlots; ++k) {
      s0 += scratch[((size_t)k * 2 + 0) * C + c];
      s1 += scratch[((size_t)k * 2 + 1) * C + c];
    }
#pragma unroll 8
    for (int k = 0; k < kSlots; ++k) {
      scratch[((size_t)k * 2 + 0) * C + c] = 0.f;
      scratch[((size_t)k * 2 + 1) * C + c] = 0.f;
    }
    dsum[c] = s0;
    dsum[C + c] = s1;
    if (dbeta) dbeta[c] += s0;
    if (dgamma) dgamma[c] += s1;
  }
}

// Where a reduction kernel of `grid` blocks adds its per-block sums of n = 2*C floats.  Normally the caller's 32-slot
// scratch; in deterministic mode (nbdt_set_deterministic) a zeroed library-owned row per block -- each address then
// receives exactly one atomic add -- that slot_finish() sums in block order into slot 0 of the caller's scratch, so
// the finalize kernels (which fold the 32 slots in a fixed order anyway) need no second form.
struct SlotTarget {
  float* ptr;
  unsigned mask;
  bool det;
};
int slot_target(hipStream_t st, float* scratch, int grid, size_t n, SlotTarget* t) {
  t->ptr = scratch; t->mask = kSlots - 1; t->det = false;
  if (!deterministic()) return NBDT_OK;
  float* rows = det_rows(st, (size_t)grid * n);
  if (!rows) return nbdt::fail(NBDT_ENOMEM, "deterministic mode: %s (%s)", "no workspace for the per-block rows", nbdt::det_rows_why());
  NBDT_HIP_CHECK(hipMemsetAsync(rows, 0, (size_t)grid * n * sizeof(float), st));
  t->ptr = rows; t->mask = ~0u; t->det = true;
  return NBDT_OK;
}
int slot_finish(hipStream_t st, const SlotTarget& t, int grid, size_t n, float* scratch) {
  return t.det ? det_fold(st, t.ptr, grid, n, scratch) : NBDT_OK;
}

}  // namespace
}  // namespace nbdt
