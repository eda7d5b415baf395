// Training-batch assembly with an augmentation policy, on the device: gather by index + RandomCrop(size, padding) +
// RandomHorizontalFlip + ONE TrivialAugmentWide operation on the uint8 image + ToTensor + Normalize + RandomErasing(value=0)
// in ONE launch, from a uint8 dataset that lives in device memory, into the fp32 NCHW tensor the stem kernels read.  The
// recipe of the TrivialAugment paper's CIFAR setup and of torchvision's ResNet reference (ta_wide + RandomErasing); the
// pixel rules are Pillow's, byte for byte (include/nbdt_hip.h states them, nbdt/data.py policy_reference restates them).
//
// One block per image.  The image's 3*H*W source bytes go to LDS with 16-byte loads (as in augment.hip); the cropped and
// flipped image is written to a second LDS tile T, which is what every operation reads: a geometric op is a gather from T
// through Pillow's 16.16 fixed-point affine coefficients, a colour op blends T with a degenerate image formed from T, the
// three histogram ops need per-image statistics first (the grey sum, per-channel min / max, per-channel 256-bin
// histogram), which one pass over T collects with INTEGER wave reductions and LDS atomics -- sums, minima and maxima of
// integers do not depend on the order, so the launch is bit-reproducible as it stands.  A lane then forms four consecutive x
// of one output row, applies the erase rectangle and the normalisation and writes one 16-byte store.
//
// The magnitudes come from a table the host builds in fp64 (nbdt/data.py policy_table): six int32 per (op, bin, sign), so
// there is no trigonometry and no magnitude arithmetic on the device.  Every value read from device memory (index, params,
// table) is clamped or bounds-checked before an address is formed from it.
//
// policy_chain_kernel (RandAugment, AutoAugment; further down) is the same launch with a chain of up to four operations:
// the staging, the statistics, the per-pixel rules and the output pass are the functions policy_kernel is made of, and after
// the crop the source tile is the chain's second buffer, so the LDS budget is the same.
//
// Built with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (nbdt/_build.py): the blend d + a * (x - d) is a
// separate fp32 multiply and add (Pillow's C), AutoContrast's v * scale + offset a separate fp64 multiply and add
// (Python's), and the normalisation is augment.hip's three IEEE operations.
//
// The rules themselves -- the draws, the statistics, the per-pixel operations, the byte pass and the output pass -- live in
// policy_ops.h, which the resized-crop path (resample.hip) shares; here they run on LDS tiles with 256 lanes.
#include "common.h"
#include "policy_ops.h"

using namespace nbdt;
using namespace nbdt::pol;

// 3*H*W of the images this kernel takes: both tiles and the statistics stay far below the 160 KB of LDS
#define NBDT_AUGMENT_LDS_BYTES 49152

namespace {

struct PolArgs {
  const unsigned char* src;
  const long long* labels_src;
  const long long* index;
  long long index_base, N;
  int H, W, pad, flip_on, policy_on;
  float mean[3], std[3];
  unsigned long long key;
  const signed char* params_in;      // int8 [B,3] (dy, dx, flip): replaces the crop / flip draw
  const int* policy_in;              // int32 [B,7] (op, bin, sign, top, left, h, w): replaces the policy and erase draw
  const int* table;                  // int32 [NBDT_POLICY_OPS][NBDT_POLICY_BINS][2][6] (device)
  EraseDraw erase;                   // erase probability, area-fraction range and the aspect-ratio table
  int vec_in, vec_out;
  float* out;
  long long* labels_out;
  signed char* params_out;
  int* policy_out;
};

// the crop / flip of sample b (nbdt_augment_batch's draw, or params_in clamped)
__device__ __forceinline__ void draw_crop(const PolArgs& a, int b, long long gidx, int& dy, int& dx, int& fl) {
  const int pad = a.pad;
  if (a.params_in) {
    dy = clampi(a.params_in[b * 3], 0, 2 * pad);
    dx = clampi(a.params_in[b * 3 + 1], 0, 2 * pad);
    fl = a.params_in[b * 3 + 2] != 0;
  } else {
    const unsigned long long r = mix64(a.key ^ ((unsigned long long)gidx * 0xD1342543DE82EF95ull));
    const unsigned span = 2u * (unsigned)pad + 1u;
    dy = (int)((((unsigned)r & 0xFFFFFFu) * span) >> 24);
    dx = (int)((((unsigned)(r >> 24) & 0xFFFFFFu) * span) >> 24);
    fl = a.flip_on ? (int)(r >> 63) : 0;
  }
}

// the image's bytes s8 into S, a barrier, the zero-padded crop and the flip into T (four packed bytes per lane where the
// row pitch allows), a barrier
__device__ __forceinline__ void stage_and_crop(const PolArgs& a, const unsigned char* s8, unsigned char* S, unsigned char* T,
                                                int dy, int dx, int fl, int tid) {
  const int H = a.H, W = a.W, pad = a.pad, n = 3 * H * W;
  if (a.vec_in)
    for (int i = tid; i < (n >> 4); i += 256) ((u32x4_t*)S)[i] = ((const u32x4_t*)s8)[i];
  else
    for (int i = tid; i < n; i += 256) S[i] = s8[i];
  __syncthreads();
  const int G = (W + 3) >> 2;            // groups of four x per row
  const int items = 3 * H * G;
  for (int it = tid; it < items; it += 256) {
    const int row = it / G, g = it - row * G;     // row = c * H + y
    const int c = row / H, y = row - c * H;
    const int sy = y + dy - pad;
    const bool yin = sy >= 0 && sy < H;
    unsigned u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = g * 4 + j;
      const int sx = (fl ? W - 1 - x : x) + dx - pad;
      u[j] = (yin && x < W && sx >= 0 && sx < W) ? S[(c * H + sy) * W + sx] : 0u;
    }
    unsigned char* dst = T + row * W + g * 4;
    if ((W & 3) == 0) {                  // (T and the row pitch are multiples of four bytes)
      *(unsigned*)dst = u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (g * 4 + j < W) dst[j] = (unsigned char)u[j];
    }
  }
  __syncthreads();
}

// the output pass on an LDS tile (byte reads: an LDS word read buys nothing here)
__device__ __forceinline__ void write_output(const PolArgs& a, const OpCtx& k, const unsigned char* T, const unsigned* hist,
                                              const double* ac, float* o, int et, int el, int eh, int ew, int tid) {
  output_pass<256, false>(a.mean, a.std, a.H, a.W, a.vec_out, k, T, hist, ac, o, et, el, eh, ew, tid);
}

__global__ __launch_bounds__(256) void policy_kernel(const PolArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int H = a.H, W = a.W, HW = H * W, n = 3 * HW;
  const int npad = (n + 15) & ~15;
  unsigned char* S = lds;                                   // [3][H][W] the source image
  unsigned char* T = lds + npad;                            // [3][H][W] cropped and flipped
  unsigned* hist = (unsigned*)(lds + 2 * npad);             // [3][256] histogram, then prefix sums, then the LUT
  unsigned* stat = hist + 768;                              // [0] grey sum, [1..3] channel minima, [4..6] maxima
  double* ac = (double*)(stat + 8);                         // [3][2] AutoContrast's (scale, offset)
  const long long gidx = a.index[b];               // the dataset's index: what the draw hashes
  const unsigned long long idx = (unsigned long long)gidx - (unsigned long long)a.index_base;      // the row held here
  const bool valid = idx < (unsigned long long)a.N;
  float* o = a.out + (size_t)b * n;

  // ---- the sample's parameters (block-uniform; every lane computes them)
  int dy = 0, dx = 0, fl = 0, op = 0, bin = 0, sg = 0, et = 0, el = 0, eh = 0, ew = 0;
  if (valid) {
    draw_crop(a, b, gidx, dy, dx, fl);
    if (a.policy_in) {
      const int* q = a.policy_in + (size_t)b * 7;
      op = clampi(q[0], 0, NBDT_POLICY_OPS - 1);
      bin = clampi(q[1], 0, NBDT_POLICY_BINS - 1);
      sg = q[2] != 0;
      clamp_erase(q + 3, H, W, et, el, eh, ew);
    } else {
      if (a.policy_on) {
        const unsigned long long rp = mix64(a.key ^ ((unsigned long long)gidx * 0xA0761D6478BD642Full));
        op = (int)((((unsigned)rp & 0xFFFFFFu) * (unsigned)NBDT_POLICY_OPS) >> 24);
        bin = (int)((((unsigned)(rp >> 24) & 0xFFFFFFu) * (unsigned)NBDT_POLICY_BINS) >> 24);
        sg = (int)(rp >> 63);
      }
      draw_erase(a.erase, H, W, erase_word(a.key, gidx), et, el, eh, ew);
    }
  }
  if (tid == 0) {
    a.labels_out[b] = valid ? a.labels_src[idx] : -1ll;
    if (a.params_out) {
      a.params_out[b * 3] = (signed char)dy;
      a.params_out[b * 3 + 1] = (signed char)dx;
      a.params_out[b * 3 + 2] = (signed char)fl;
    }
    if (a.policy_out) {
      int* q = a.policy_out + (size_t)b * 7;
      q[0] = op; q[1] = bin; q[2] = sg; q[3] = et; q[4] = el; q[5] = eh; q[6] = ew;
    }
  }
  if (!valid) {      // (block-uniform) an index the host could not check: a zero image, label -1, no source address formed
    for (int i = tid; i < n; i += 256) o[i] = 0.f;
    return;
  }

  // ---- stage the source, then crop and flip it into T
  reset_statistics<256>(hist, tid);
  stage_and_crop(a, a.src + (size_t)idx * n, S, T, dy, dx, fl, tid);

  // ---- the operation's constants and per-image statistics (op is block-uniform: so is every barrier below)
  OpCtx k = {};
  k.op = op;
  {
    const int* row = a.table ? a.table + (size_t)(((op * NBDT_POLICY_BINS + bin) * 2 + sg) * 6) : nullptr;
#pragma unroll
    for (int i = 0; i < 6; ++i) k.a[i] = row ? (unsigned)row[i] : 0u;
    k.factor = __uint_as_float(k.a[0]);
  }
  op_statistics<256>(k, T, hist, stat, ac, HW, tid);

  write_output(a, k, T, hist, ac, o, et, el, eh, ew, tid);
}

// ---- policy chains: RandAugment and AutoAugment, up to NBDT_CHAIN_MAX_OPS operations per image in the same one launch.
// After the crop the source tile S is free, so the chain ping-pongs between the two tiles: every non-Identity slot but the
// last is a byte pass from the current tile into the other one, the last is evaluated inside the normalising output pass as
// in policy_kernel, and the statistics an operation needs are collected again on the tile it reads.  The chain is
// block-uniform, so every barrier below is.
struct ChainArgs {
  PolArgs p;                         // (policy_on, policy_in, policy_out unused; table is [NBDT_CHAIN_OPS][nbins][2][6])
  int mode, nbins, num_ops, magnitude, P;
  const int* subpolicies;            // int32 [P][NBDT_CHAIN_MAX_OPS][3] (op, q, bin), device: clamped here
  const int* chain_in;               // int32 [B][NBDT_CHAIN_MAX_OPS][3] (op, bin, sign): replaces the chain's draw
  const int* erase_in;               // int32 [B][4] (top, left, h, w): replaces the erase draw
  int* chain_out;
  int* erase_out;
};

__global__ __launch_bounds__(256) void policy_chain_kernel(const ChainArgs ca) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const PolArgs& a = ca.p;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int H = a.H, W = a.W, HW = H * W, n = 3 * HW;
  const int npad = (n + 15) & ~15;
  unsigned char* S = lds;                                   // [3][H][W] the source image, then the chain's other tile
  unsigned char* T = lds + npad;                            // [3][H][W] cropped and flipped
  unsigned* hist = (unsigned*)(lds + 2 * npad);             // [3][256] histogram, then prefix sums, then the LUT
  unsigned* stat = hist + 768;                              // [0] grey sum, [1..3] channel minima, [4..6] maxima
  double* ac = (double*)(stat + 8);                         // [3][2] AutoContrast's (scale, offset)
  const long long gidx = a.index[b];
  const unsigned long long idx = (unsigned long long)gidx - (unsigned long long)a.index_base;
  const bool valid = idx < (unsigned long long)a.N;
  float* o = a.out + (size_t)b * n;

  // ---- the sample's parameters (block-uniform; every lane computes them)
  int dy = 0, dx = 0, fl = 0, et = 0, el = 0, eh = 0, ew = 0;
  unsigned long long chain = 0;      // 16 bits per slot: op | bin << 4 | sign << 9 (all zero: Identity)
  if (valid) {
    draw_crop(a, b, gidx, dy, dx, fl);
    if (ca.chain_in)
      chain = clamp_chain(ca.chain_in + (size_t)b * (NBDT_CHAIN_MAX_OPS * 3), ca.nbins);
    else
      chain = draw_chain(a.key, gidx, ca.mode, ca.nbins, ca.num_ops, ca.magnitude, ca.subpolicies, ca.P);
    if (ca.erase_in)
      clamp_erase(ca.erase_in + (size_t)b * 4, H, W, et, el, eh, ew);
    else
      draw_erase(a.erase, H, W, erase_word(a.key, gidx), et, el, eh, ew);
  }
  if (tid == 0) {
    a.labels_out[b] = valid ? a.labels_src[idx] : -1ll;
    if (a.params_out) {
      a.params_out[b * 3] = (signed char)dy;
      a.params_out[b * 3 + 1] = (signed char)dx;
      a.params_out[b * 3 + 2] = (signed char)fl;
    }
    if (ca.chain_out) store_chain(ca.chain_out + (size_t)b * (NBDT_CHAIN_MAX_OPS * 3), chain);
    if (ca.erase_out) {
      int* q = ca.erase_out + (size_t)b * 4;
      q[0] = et; q[1] = el; q[2] = eh; q[3] = ew;
    }
  }
  if (!valid) {      // (block-uniform) an index the host could not check: a zero image, label -1, no source address formed
    for (int i = tid; i < n; i += 256) o[i] = 0.f;
    return;
  }

  stage_and_crop(a, a.src + (size_t)idx * n, S, T, dy, dx, fl, tid);

  // ---- the chain: `cur` holds the image so far, `oth` is free
  const int last = last_slot(chain);
  unsigned char* cur = T;
  unsigned char* oth = S;
  OpCtx k = {};            // all slots Identity: the output is read straight from T
  for (int s = 0; s <= last; ++s) {             // (one copy of the passes, not four: the slot is a run-time shift)
    const int op = load_slot(k, a.table, ca.nbins, chain, s);
    if (op == OP_IDENTITY) continue;            // costs nothing: no pass, no barrier
    if (op_needs_statistics(op)) {
      // the statistics of an earlier operation are stale: start again, a barrier on both sides (the first one also keeps
      // this slot's writes behind every read of the previous LUT)
      __syncthreads();
      reset_statistics<256>(hist, tid);
      __syncthreads();
      op_statistics<256>(k, cur, hist, stat, ac, HW, tid);
    }
    if (s == last) break;
    byte_pass<256, false>(k, cur, oth, hist, ac, H, W, tid);
    __syncthreads();
    unsigned char* t = cur;
    cur = oth;
    oth = t;
  }
  write_output(a, k, cur, hist, ac, o, et, el, eh, ew, tid);
}

}  // namespace

// the arguments both entries share, checked before the first device call
static int check_source(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index,
                        int64_t index_base, int32_t B, int64_t N, int32_t H, int32_t W, int32_t pad, int32_t flip,
                        const float* mean, const float* std, const float* out, const int64_t* labels_out) {
  NBDT_REQUIRE(src && labels_src && index && out && labels_out, "null argument");
  NBDT_REQUIRE(N <= 0 || (index_base >= 0 && index_base <= INT64_MAX - N),
               "index_base must be >= 0 and index_base + N must fit int64");
  NBDT_REQUIRE(src_dtype == NBDT_U8, "the policy works on bytes: the dataset must be uint8 (NBDT_U8)");
  NBDT_REQUIRE(B > 0, "empty batch");
  NBDT_REQUIRE(N > 0, "empty dataset");
  NBDT_REQUIRE(H > 0 && W > 0 && H <= 4096 && W <= 4096, "image sides must be 1..4096");
  NBDT_REQUIRE((long long)H * W * 3 <= NBDT_AUGMENT_LDS_BYTES,
               "the policy kernel stages the image in LDS: 3*H*W must be at most 49152 bytes (128 x 128)");
  NBDT_REQUIRE(pad >= 0 && pad <= NBDT_AUGMENT_MAX_PAD, "pad must be 0..NBDT_AUGMENT_MAX_PAD");
  NBDT_REQUIRE(flip == 0 || flip == 1, "flip is 0 or 1");
  NBDT_REQUIRE(mean && std, "a uint8 dataset needs mean[3] and std[3]");
  NBDT_REQUIRE(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "std must be non-zero");
  return NBDT_OK;
}

// erase_prob, and what the erase draw needs when it is made (`drawn`: no rectangle is given)
static int check_erase(PolArgs& a, double erase_prob, const double* erase_scale, const double* erase_ratio,
                       const double* ratio_table, bool drawn) {
  NBDT_REQUIRE(erase_prob >= 0.0 && erase_prob <= 1.0, "erase_prob must be in [0, 1]");       // (NaN fails both)
  if (erase_prob > 0.0 && drawn) {
    NBDT_REQUIRE(erase_scale && erase_ratio && ratio_table,
                 "the erase draw needs erase_scale[2], erase_ratio[2] and the ratio table");
    NBDT_REQUIRE(erase_scale[0] > 0.0 && erase_scale[0] <= erase_scale[1] && erase_scale[1] <= 1.0,
                 "erase_scale must satisfy 0 < lo <= hi <= 1");
    NBDT_REQUIRE(erase_ratio[0] >= 1.0 / 64.0 && erase_ratio[0] <= erase_ratio[1] && erase_ratio[1] <= 64.0,
                 "erase_ratio must satisfy 1/64 <= lo <= hi <= 64");
    a.erase.p = erase_prob;
    a.erase.s0 = erase_scale[0];
    a.erase.s1 = erase_scale[1];
    a.erase.ratio_table = ratio_table;
  }
  return NBDT_OK;
}

static void fill_source(PolArgs& a, const void* src, const int64_t* labels_src, const int64_t* index, int64_t index_base,
                        int64_t N, int32_t H, int32_t W, int32_t pad, int32_t flip, const float* mean, const float* std,
                        uint64_t seed, uint64_t epoch, const int8_t* params_in, const int32_t* table, float* out,
                        int64_t* labels_out, int8_t* params_out) {
  a.src = (const unsigned char*)src;
  a.labels_src = (const long long*)labels_src;
  a.index = (const long long*)index;
  a.index_base = index_base;
  a.N = N;
  a.H = H; a.W = W; a.pad = pad; a.flip_on = flip;
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.std[c] = std[c]; }
  a.key = mix64((unsigned long long)seed * 0x9E3779B97F4A7C15ull + (unsigned long long)epoch);
  a.params_in = (const signed char*)params_in;
  a.table = table;
  const int n = 3 * H * W;
  a.vec_in = (n % 16 == 0 && (uintptr_t)src % 16 == 0) ? 1 : 0;
  a.vec_out = (W % 4 == 0 && (uintptr_t)out % 16 == 0) ? 1 : 0;
  a.out = out;
  a.labels_out = (long long*)labels_out;
  a.params_out = (signed char*)params_out;
}

// both tiles, the histograms and statistics, AutoContrast's three (scale, offset)
static size_t policy_lds_bytes(int H, int W) {
  return (size_t)2 * ((3 * H * W + 15) & ~15) + 776 * sizeof(unsigned) + 6 * sizeof(double);
}

extern "C" int nbdt_policy_batch_sharded(const void* src, int32_t src_dtype, const int64_t* labels_src,
                                         const int64_t* index, int64_t index_base, int32_t B, int64_t N, int32_t H,
                                         int32_t W, int32_t pad, int32_t flip, const float* mean, const float* std,
                                         int32_t policy, const int32_t* policy_table, double erase_prob,
                                         const double* erase_scale, const double* erase_ratio, const double* ratio_table,
                                         uint64_t seed, uint64_t epoch, const int8_t* params_in, const int32_t* policy_in,
                                         float* out, int64_t* labels_out, int8_t* params_out, int32_t* policy_out,
                                         void* stream) {
  if (int rc = check_source(src, src_dtype, labels_src, index, index_base, B, N, H, W, pad, flip, mean, std, out, labels_out))
    return rc;
  NBDT_REQUIRE(policy == NBDT_POLICY_NONE || policy == NBDT_POLICY_TA_WIDE, "policy is NBDT_POLICY_NONE or NBDT_POLICY_TA_WIDE");
  NBDT_REQUIRE(policy_table || (policy == NBDT_POLICY_NONE && !policy_in),
               "a policy (or policy_in) needs the policy table");
  PolArgs a = {};
  if (int rc = check_erase(a, erase_prob, erase_scale, erase_ratio, ratio_table, !policy_in)) return rc;
  fill_source(a, src, labels_src, index, index_base, N, H, W, pad, flip, mean, std, seed, epoch, params_in, policy_table, out,
              labels_out, params_out);
  a.policy_on = policy == NBDT_POLICY_TA_WIDE;
  a.policy_in = policy_in;
  a.policy_out = policy_out;
  const size_t shmem = policy_lds_bytes(H, W);
  static DeviceAttr site;
  if (shmem > 65536 && site.need(shmem)) {      // (up to 64 KB needs no attribute)
    NBDT_ATTR_CHECK(site, hipFuncSetAttribute(reinterpret_cast<const void*>(&policy_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    site.done(shmem);
  }
  hipLaunchKernelGGL(policy_kernel, dim3(B), dim3(256), shmem, (hipStream_t)stream, a);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

// the whole dataset is the shard at base 0: the same kernel, the same bits
extern "C" int nbdt_policy_batch(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index,
                                 int32_t B, int64_t N, int32_t H, int32_t W, int32_t pad, int32_t flip, const float* mean,
                                 const float* std, int32_t policy, const int32_t* policy_table, double erase_prob,
                                 const double* erase_scale, const double* erase_ratio, const double* ratio_table,
                                 uint64_t seed, uint64_t epoch, const int8_t* params_in, const int32_t* policy_in,
                                 float* out, int64_t* labels_out, int8_t* params_out, int32_t* policy_out, void* stream) {
  return nbdt_policy_batch_sharded(src, src_dtype, labels_src, index, 0, B, N, H, W, pad, flip, mean, std, policy,
                                   policy_table, erase_prob, erase_scale, erase_ratio, ratio_table, seed, epoch, params_in,
                                   policy_in, out, labels_out, params_out, policy_out, stream);
}

// ---- policy chains (RandAugment, AutoAugment): the same staging, LDS budget and refusals, policy_chain_kernel
extern "C" int nbdt_policy_chain_batch_sharded(const void* src, int32_t src_dtype, const int64_t* labels_src,
                                               const int64_t* index, int64_t index_base, int32_t B, int64_t N, int32_t H,
                                               int32_t W, int32_t pad, int32_t flip, const float* mean, const float* std,
                                               int32_t mode, int32_t nbins, const int32_t* table, int32_t num_ops,
                                               int32_t magnitude, const int32_t* subpolicies, int32_t P, double erase_prob,
                                               const double* erase_scale, const double* erase_ratio,
                                               const double* ratio_table, uint64_t seed, uint64_t epoch,
                                               const int8_t* params_in, const int32_t* chain_in, const int32_t* erase_in,
                                               float* out, int64_t* labels_out, int8_t* params_out, int32_t* chain_out,
                                               int32_t* erase_out, void* stream) {
  if (int rc = check_source(src, src_dtype, labels_src, index, index_base, B, N, H, W, pad, flip, mean, std, out, labels_out))
    return rc;
  NBDT_REQUIRE(mode == NBDT_CHAIN_RAND || mode == NBDT_CHAIN_SUBPOLICY, "mode is NBDT_CHAIN_RAND or NBDT_CHAIN_SUBPOLICY");
  NBDT_REQUIRE(nbins >= 1 && nbins <= NBDT_CHAIN_MAX_BINS, "nbins must be 1..NBDT_CHAIN_MAX_BINS");
  NBDT_REQUIRE(table, "null argument: the chain needs its magnitude table");
  ChainArgs ca = {};
  if (mode == NBDT_CHAIN_RAND) {
    NBDT_REQUIRE(num_ops >= 1 && num_ops <= NBDT_CHAIN_MAX_OPS, "num_ops must be 1..NBDT_CHAIN_MAX_OPS");
    NBDT_REQUIRE(magnitude >= 0 && magnitude < nbins, "magnitude must be a bin: 0 <= magnitude < nbins");
    ca.num_ops = num_ops;
    ca.magnitude = magnitude;
  } else {
    NBDT_REQUIRE(subpolicies, "null argument: NBDT_CHAIN_SUBPOLICY needs the sub-policies");
    NBDT_REQUIRE(P >= 1 && P <= NBDT_CHAIN_MAX_SUBPOLICIES, "P (the number of sub-policies) must be 1..NBDT_CHAIN_MAX_SUBPOLICIES");
    ca.subpolicies = subpolicies;
    ca.P = P;
  }
  if (int rc = check_erase(ca.p, erase_prob, erase_scale, erase_ratio, ratio_table, !erase_in)) return rc;
  fill_source(ca.p, src, labels_src, index, index_base, N, H, W, pad, flip, mean, std, seed, epoch, params_in, table, out,
              labels_out, params_out);
  ca.mode = mode;
  ca.nbins = nbins;
  ca.chain_in = chain_in;
  ca.erase_in = erase_in;
  ca.chain_out = chain_out;
  ca.erase_out = erase_out;
  const size_t shmem = policy_lds_bytes(H, W);
  static DeviceAttr site;
  if (shmem > 65536 && site.need(shmem)) {      // (up to 64 KB needs no attribute)
    NBDT_ATTR_CHECK(site, hipFuncSetAttribute(reinterpret_cast<const void*>(&policy_chain_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    site.done(shmem);
  }
  hipLaunchKernelGGL(policy_chain_kernel, dim3(B), dim3(256), shmem, (hipStream_t)stream, ca);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_policy_chain_batch(const void* src, int32_t src_dtype, const int64_t* labels_src, const int64_t* index,
                                       int32_t B, int64_t N, int32_t H, int32_t W, int32_t pad, int32_t flip,
                                       const float* mean, const float* std, int32_t mode, int32_t nbins,
                                       const int32_t* table, int32_t num_ops, int32_t magnitude, const int32_t* subpolicies,
                                       int32_t P, double erase_prob, const double* erase_scale, const double* erase_ratio,
                                       const double* ratio_table, uint64_t seed, uint64_t epoch, const int8_t* params_in,
                                       const int32_t* chain_in, const int32_t* erase_in, float* out, int64_t* labels_out,
                                       int8_t* params_out, int32_t* chain_out, int32_t* erase_out, void* stream) {
  return nbdt_policy_chain_batch_sharded(src, src_dtype, labels_src, index, 0, B, N, H, W, pad, flip, mean, std, mode, nbins,
                                         table, num_ops, magnitude, subpolicies, P, erase_prob, erase_scale, erase_ratio,
                                         ratio_table, seed, epoch, params_in, chain_in, erase_in, out, labels_out, params_out,
                                         chain_out, erase_out, stream);
}
