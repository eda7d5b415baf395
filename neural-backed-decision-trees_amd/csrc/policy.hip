// Training-batch assembly with an augmentation policy, on the device: gather by index + RandomCrop(size, padding) +
// RandomHorizontalFlip + a chain of up to NBDT_CHAIN_MAX_OPS operations on the uint8 image + ToTensor + Normalize +
// RandomErasing(value=0) in ONE launch, from a uint8 dataset that lives in device memory, into the fp32 NCHW tensor the stem
// kernels read.  nbdt_policy_batch is the chain of one TrivialAugmentWide operation (or of none: the erase alone), the
// recipe of the TrivialAugment paper's CIFAR setup and of torchvision's ResNet reference; nbdt_policy_chain_batch is
// RandAugment and AutoAugment, policy_kernel and policy_chain_kernel.  Pillow's pixel rules, byte for byte (include/nbdt_hip.h states them, nbdt/data.py policy_reference / chain_reference restate them).
//
// One block per image.  The image's 3*H*W source bytes go to LDS with 16-byte loads (as in augment.hip); the cropped and
// flipped image is written to a second LDS tile T, which is what an operation reads: a geometric op is a gather from T
// through Pillow's 16.16 fixed-point affine coefficients, a colour op blends T with a degenerate image formed from T, the
// three histogram ops need per-image statistics first (the grey sum, per-channel min / max, per-channel 256-bin
// histogram), which one pass over T collects with INTEGER wave reductions and LDS atomics -- sums, minima and maxima of
// integers do not depend on the order, so the launch is bit-reproducible as it stands.  After the crop the source tile S is
// free, so a chain ping-pongs between the two tiles (policy_ops.h run_chain) and the LDS budget does not grow with it.  For
// the last operation a lane forms four consecutive x of one output row, applies the erase rectangle and the normalisation
// and writes one 16-byte store.
//
// The magnitudes come from a table the host builds in fp64 (nbdt/data.py policy_table, chain_table): six int32 per (op,
// bin, sign), so there is no trigonometry and no magnitude arithmetic on the device.  Every value read from device memory
// (index, params, table) is clamped or bounds-checked before an address is formed from it.
//
// Built with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (nbdt/_build.py): the blend d + a * (x - d) is a
// separate fp32 multiply and add (Pillow's C), AutoContrast's v * scale + offset a separate fp64 multiply and add
// (Python's), and the normalisation is augment.hip's three IEEE operations.
//
// The rules themselves -- the draws, the statistics, the per-pixel operations, the two passes and the loop over the chain --
// live in policy_ops.h, which the resized-crop path (resample.hip) shares; here they run on LDS tiles with 256 lanes.
#include "common.h"
#include "policy_ops.h"

using namespace nbdt;
using namespace nbdt::pol;

// 3*H*W of the images this kernel takes: both tiles and the statistics stay far below the 160 KB of LDS
#define NBDT_AUGMENT_LDS_BYTES 49152

namespace {

struct ChainArgs {
  const unsigned char* src;
  const long long* labels_src;
  const long long* index;
  long long index_base, N;
  int H, W, pad, flip_on;
  float mean[3], std[3];
  unsigned long long key;
  const signed char* params_in;      // int8 [B,3] (dy, dx, flip): replaces the crop / flip draw
  ChainSpec c;                       // the chain and the erase: their draw, their table, what replaces and reports them
  const int* policy_in;              // int32 [B,7], policy_kernel only: replaces the policy and erase draw
  int* policy_out;                   // int32 [B,7], policy_kernel only
  int vec_in, vec_out;
  float* out;
  long long* labels_out;
  signed char* params_out;
};

// the crop / flip of sample b (nbdt_augment_batch's draw, or params_in clamped)
__device__ __forceinline__ void draw_crop(const ChainArgs& a, int b, long long gidx, int& dy, int& dx, int& fl) {
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
__device__ __forceinline__ void stage_and_crop(const ChainArgs& a, const unsigned char* s8, unsigned char* S,
                                                unsigned char* T, int dy, int dx, int fl, int tid) {
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

// what both kernels begin with: the block's LDS, the sample's row and its crop / flip (block-uniform; every lane computes it)
struct Sample {
  unsigned char* S;        // [3][H][W] the source image, then the chain's other tile
  unsigned char* T;        // [3][H][W] cropped and flipped
  unsigned* hist;          // [3][256] histogram, then prefix sums, then the LUT; then stat[8]
  double* ac;              // [3][2] AutoContrast's (scale, offset)
  long long gidx;          // the dataset's index: what the draws hash
  unsigned long long idx;  // the row held here
  bool valid;
  int n, dy, dx, fl;
  float* o;
  __device__ __forceinline__ Sample(const ChainArgs& a, unsigned char* lds, int b) {
    n = 3 * a.H * a.W;
    const int npad = (n + 15) & ~15;
    S = lds;
    T = lds + npad;
    hist = (unsigned*)(lds + 2 * npad);
    ac = (double*)(hist + kStatWords);
    gidx = a.index[b];
    idx = (unsigned long long)gidx - (unsigned long long)a.index_base;
    valid = idx < (unsigned long long)a.N;
    o = a.out + (size_t)b * n;
    dy = dx = fl = 0;
    if (valid) draw_crop(a, b, gidx, dy, dx, fl);
  }
  // the label and the crop used (one lane calls this)
  __device__ __forceinline__ void store(const ChainArgs& a, int b) const {
    a.labels_out[b] = valid ? a.labels_src[idx] : -1ll;
    if (a.params_out) {
      a.params_out[b * 3] = (signed char)dy;
      a.params_out[b * 3 + 1] = (signed char)dx;
      a.params_out[b * 3 + 2] = (signed char)fl;
    }
  }
  // (block-uniform) an index the host could not check: a zero image, label -1, no source address formed
  __device__ __forceinline__ void zero_image(int tid) const {
    for (int i = tid; i < n; i += 256) o[i] = 0.f;
  }
};

// nbdt_policy_batch: ONE operation per image, in this entry's own [B,7] rows (op, bin, sign, top, left, h, w).  The
// statistics are reset before the staging's barriers and the operation goes straight to the output pass: measured against
// the chain kernel below (profiles/data_path_refactor_ab.txt).  Byte reads (WORD = false): an LDS word read buys nothing here.
__global__ __launch_bounds__(256) void policy_kernel(const ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int H = a.H, W = a.W;
  const Sample s(a, lds, b);
  int op = 0, bin = 0, sg = 0, et = 0, el = 0, eh = 0, ew = 0;
  if (s.valid && a.policy_in) {      // (Invert stays out of reach of this entry)
    const int* q = a.policy_in + (size_t)b * 7;
    op = clampi(q[0], 0, NBDT_POLICY_OPS - 1);
    bin = clampi(q[1], 0, NBDT_POLICY_BINS - 1);
    sg = q[2] != 0;
    clamp_erase(q + 3, H, W, et, el, eh, ew);
  } else {
    unsigned long long chain;        // one slot (NBDT_CHAIN_TA_WIDE) or none
    chain_params(a.c, a.key, s.gidx, b, H, W, s.valid, chain, et, el, eh, ew);
    op = (int)(chain & 15u); bin = (int)((chain >> 4) & 31u); sg = (int)((chain >> 9) & 1u);
  }
  if (tid == 0) {
    s.store(a, b);
    if (a.policy_out) {
      int* q = a.policy_out + (size_t)b * 7;
      q[0] = op; q[1] = bin; q[2] = sg; q[3] = et; q[4] = el; q[5] = eh; q[6] = ew;
    }
  }
  if (!s.valid) {
    s.zero_image(tid);
    return;
  }

  // ---- stage the source, then crop and flip it into T
  reset_statistics<256>(s.hist, tid);
  stage_and_crop(a, a.src + (size_t)s.idx * s.n, s.S, s.T, s.dy, s.dx, s.fl, tid);

  // ---- the operation's constants and per-image statistics (op is block-uniform: so is every barrier below)
  OpCtx k = {};
  k.op = op;
  {
    const int* row = a.c.table ? a.c.table + (size_t)(((op * NBDT_POLICY_BINS + bin) * 2 + sg) * 6) : nullptr;
#pragma unroll
    for (int i = 0; i < 6; ++i) k.a[i] = row ? (unsigned)row[i] : 0u;
    k.factor = __uint_as_float(k.a[0]);
  }
  op_statistics<256>(k, s.T, s.hist, s.hist + 768, s.ac, H * W, tid);
  output_pass<256, false>(a.mean, a.std, H, W, a.vec_out, k, s.T, s.hist, s.ac, s.o, et, el, eh, ew, tid);
}

// nbdt_policy_chain_batch (RandAugment, AutoAugment): up to NBDT_CHAIN_MAX_OPS operations per image; after the crop the
// source tile S is the chain's other tile (policy_ops.h run_chain)
__global__ __launch_bounds__(256) void policy_chain_kernel(const ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int H = a.H, W = a.W;
  const Sample s(a, lds, b);
  int et, el, eh, ew;
  unsigned long long chain;
  chain_params(a.c, a.key, s.gidx, b, H, W, s.valid, chain, et, el, eh, ew);
  if (tid == 0) {
    s.store(a, b);
    store_chain_params(a.c, b, chain, et, el, eh, ew);
  }
  if (!s.valid) {
    s.zero_image(tid);
    return;
  }
  stage_and_crop(a, a.src + (size_t)s.idx * s.n, s.S, s.T, s.dy, s.dx, s.fl, tid);
  run_chain<256, false>(a.c, chain, s.T, s.S, s.hist, s.ac, H, W, a.mean, a.std, a.vec_out, s.o, et, el, eh, ew, tid);
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

// both tiles, the histograms and statistics, AutoContrast's three (scale, offset)
static size_t policy_lds_bytes(int H, int W) {
  return (size_t)2 * ((3 * H * W + 15) & ~15) + 776 * sizeof(unsigned) + 6 * sizeof(double);
}

// the checked source into `a` (a.c is the entry's), then the launch of `kernel` (`site`: its own)
static int launch(void (*kernel)(const ChainArgs), DeviceAttr& site, ChainArgs& a, const void* src,
                  const int64_t* labels_src, const int64_t* index, int64_t index_base, int32_t B, int64_t N, int32_t H,
                  int32_t W, int32_t pad, int32_t flip, const float* mean, const float* std, uint64_t seed, uint64_t epoch,
                  const int8_t* params_in, float* out, int64_t* labels_out, int8_t* params_out, void* stream) {
  a.src = (const unsigned char*)src;
  a.labels_src = (const long long*)labels_src;
  a.index = (const long long*)index;
  a.index_base = index_base;
  a.N = N;
  a.H = H; a.W = W; a.pad = pad; a.flip_on = flip;
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.std[c] = std[c]; }
  a.key = mix64((unsigned long long)seed * 0x9E3779B97F4A7C15ull + (unsigned long long)epoch);
  a.params_in = (const signed char*)params_in;
  const int n = 3 * H * W;
  a.vec_in = (n % 16 == 0 && (uintptr_t)src % 16 == 0) ? 1 : 0;
  a.vec_out = (W % 4 == 0 && (uintptr_t)out % 16 == 0) ? 1 : 0;
  a.out = out;
  a.labels_out = (long long*)labels_out;
  a.params_out = (signed char*)params_out;
  const size_t shmem = policy_lds_bytes(H, W);
  if (shmem > 65536 && site.need(shmem)) {      // (up to 64 KB needs no attribute)
    NBDT_ATTR_CHECK(site, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    site.done(shmem);
  }
  hipLaunchKernelGGL(kernel, dim3(B), dim3(256), shmem, (hipStream_t)stream, a);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

// TrivialAugmentWide is drawn as the chain of one slot among NBDT_POLICY_BINS bins, no policy as the chain of none
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
  ChainArgs a = {};
  if (int rc = check_erase(a.c, erase_prob, erase_scale, erase_ratio, ratio_table, !policy_in)) return rc;
  a.c.mode = policy == NBDT_POLICY_TA_WIDE ? NBDT_CHAIN_TA_WIDE : NBDT_CHAIN_RAND;      // (RAND with num_ops 0: none)
  a.c.nbins = NBDT_POLICY_BINS;
  a.c.table = policy_table;
  a.policy_in = policy_in;
  a.policy_out = policy_out;
  static DeviceAttr site;
  return launch(policy_kernel, site, a, src, labels_src, index, index_base, B, N, H, W, pad, flip, mean, std, seed, epoch, params_in, out,
                labels_out, params_out, stream);
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

// ---- policy chains (RandAugment, AutoAugment): the same source checks, the same launch
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
  ChainArgs a = {};
  if (int rc = check_chain(a.c, mode, nbins, table, num_ops, magnitude, subpolicies, P, chain_in, false, false)) return rc;
  if (int rc = check_erase(a.c, erase_prob, erase_scale, erase_ratio, ratio_table, !erase_in)) return rc;
  a.c.erase_in = erase_in;
  a.c.chain_out = chain_out;
  a.c.erase_out = erase_out;
  static DeviceAttr site;
  return launch(policy_chain_kernel, site, a, src, labels_src, index, index_base, B, N, H, W, pad, flip, mean, std, seed, epoch, params_in, out,
                labels_out, params_out, stream);
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
