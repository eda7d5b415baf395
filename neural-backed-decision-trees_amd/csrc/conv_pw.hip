// Pointwise convolution: a stride-1 1x1 conv over padded NHWC tensors as a plain GEMM (gfx950 only).
//
// Replaces nn.Conv2d(kernel_size=1) of the reference's Bottleneck (nbdt/models/resnet.py:82, 88-90) -- conv1 and conv3
// of every block, forward and data gradient:
//
//     out[pix(m)][n] (+)= sum_c in[pix(m)][c] * w[n][c]          m over the B*gh*gw INTERIOR pixels
//
// Both operands are K-contiguous (pixels x cin against w[cout][1][cin]; for the data gradient pixels x cout against
// wd[cin][1][cout]), so one kernel serves both, with no halo, no taps and 16-byte LDS-DMA pieces along the channel axis.
// The halo ring of `in` is never read (pixel rows past M re-read the last interior pixel) and the halo ring of `out` is
// never written.
//
// Tile and K loop.  A block is 8 waves (512 threads) on a 256-pixel x BN-channel output tile, BN = 32 * NT; wave w owns
// pixels [32 w, 32 w + 32) x all BN channels: acc[NT] tiles of v_mfma_f32_32x32x16_bf16, issued "transposed" (A operand =
// weights, B operand = pixels) like the other conv kernels, so a lane holds 4 consecutive couts of ONE pixel per
// accumulator quad and the shared epilogue (conv_common.h: LDS transposition, 16-byte write-through stores, per-tile
// BatchNorm partial sums without atomics) applies unchanged with NWV = 8, MW = 1.  K advances in 32-channel steps through a
// 3-stage LDS ring filled by global_load_lds_dwordx4 (the protocol of conv_dma.hip: counted s_waitcnt vmcnt(N), one raw
// s_barrier per step, the DMA of step t + 2 issued right behind the barrier that frees its slot); tiles are [row][32 k]
// with the 16-byte chunk XOR-swizzled on the SOURCE address and on the fragment read.  fp32 accumulation over all of K in
// ascending order, one rounding to bf16 at the store (`accumulate`: out is read as the epilogue's residual, added in
// fp32, rounded once).
//
// Against conv_igemm_dma_kernel (4 waves, 64 pixels per wave) on the same launch: twice the waves per CU behind the same
// LDS (two 512-thread blocks per CU, 16 waves, for NT <= 4; NT = 5 takes 89-104 KB of LDS and up to 148 VGPRs: one) -- the wide early layers (64 -> 256 at 32x32: 2 K steps, 84 MB for 4.3
// GFLOP) are all prologue and epilogue, and what hides their latency is the other waves -- and a cout tile chosen per
// LAUNCH: the widest of NT = 5 / 4 / 3 / 2 / 1 that still gives every CU a block, else the narrowest (stage 4 of a
// ResNet50 at 128 images is 8 pixel tiles: 2048 -> 512 runs 64 blocks of 64 couts where the first-generation kernel ran
// 32 of 128).  NT = 1 is not taken by a statistics launch unless cout / 32 has no other divisor.
//
// Statistics.  The shared epilogue runs without its statistics mode; the per-tile sums are taken from the transposed bf16
// tile in LDS in a pass of this kernel's own, in the summation order of nbdt_conv_igemm_stats (see there): outputs AND
// partial sums of the two entries are bit-identical for every cout that is a multiple of 64 (a single 32-channel cout
// tile of that entry adds with LDS atomics, in no fixed order), plain stores, no atomics.
//
// The statistics pass costs 3-9 us per launch (2-byte LDS reads, one chain per thread), which the shared epilogue's own
// statistics mode (8 waves x 32 pixels: another order, last-bit different sums) does not: with fewer than 1024 input
// channels a statistics launch is slower than nbdt_conv_igemm_stats, and nbdt.engine.Conv keeps those there
// (Conv.PW_STATS_MIN_CIN; DESIGN.md section 4.2b has both variants' times).
//
// Not built: persistent blocks with a resident weight tile, a K split for the few-tile shapes, and a statistics pass
// that keeps the order at the shared epilogue's cost (the chain handed from wave 2 w4 to wave 2 w4 + 1 inside its row walk).
//
// Out of scope: no residual operand (the block's add is in bn3.apply, as for BasicBlock); no eval-affine epilogue and no
// fused BatchNorm-backward epilogue (inference keeps nbdt_conv_igemm_affine; conv3's data gradient is followed by the
// plain BatchNorm backward); strided 1x1 shortcuts and their gradients stay on nbdt_conv_igemm.
#include "conv_common.h"

namespace {

constexpr int PW_WAVES = 8;

// weight DMA instructions (16 rows x 64 B each) are handed out as ids {(w + 4) % 8, + 8, ..}: the fewest any wave issues
constexpr int pw_min_w_dma(int w_instr) {
  int best = 1 << 30;
  for (int w = 0; w < PW_WAVES; ++w) {
    int n = 0;
    for (int id = (w + 4) & 7; id < w_instr; id += PW_WAVES) ++n;
    best = n < best ? n : best;
  }
  return best;
}

// statistics pass: (channel, wave pair) items per block, and where their partial sums are parked -- in the waves' transposition
// regions once everybody has read them (one trip), else (NT = 5: 640 items for 512 threads) behind the epilogue's LDS
template <int NT>
constexpr int pw_stat_trips() { return (32 * NT * 4 + 64 * PW_WAVES - 1) / (64 * PW_WAVES); }
template <int NT>
constexpr int pw_stat_scratch() { return pw_stat_trips<NT>() > 1 ? 32 * NT * 4 * 3 * 8 : 0; }   // NT = 5: 3 chains per item

template <int NT>
constexpr int pw_lds_bytes() {
  constexpr int ring = NSTAGE * (BM * BK * 2 + 32 * NT * BK * 2);
  constexpr int epi = conv_epilogue_lds_bytes<NT, PW_WAVES>() + pw_stat_scratch<NT>();
  return ring > epi ? ring : epi;
}

}  // namespace

template <int NT, bool HAS_RES, int STATS>
__global__ __launch_bounds__(64 * PW_WAVES, 2) void conv_pw_kernel(nbdt::ConvDmaParams p) {
  constexpr int BN = 32 * NT;
  constexpr int A_BYTES = BM * BK * 2;  // 16 KiB
  constexpr int W_BYTES = BN * BK * 2;
  constexpr int STAGE = A_BYTES + W_BYTES;
  constexpr int A_IPW = A_BYTES / 1024 / PW_WAVES;            // 2 pixel instructions per wave and stage
  constexpr int W_INSTR = W_BYTES / 1024;
  constexpr int W_IPW = (W_INSTR + PW_WAVES - 1) / PW_WAVES;
  constexpr int MINPW = A_IPW + pw_min_w_dma(W_INSTR);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int bid = blockIdx.x;
  const int item = (bid & 7) * p.per_xcd + (bid >> 3);        // each XCD walks a contiguous range of items
  if (item >= p.m_blocks * p.n_blocks) return;
  const int m_blk = item / p.n_blocks;                        // cout tiles of one pixel tile are neighbours: one L2
  const int n_blk = item - m_blk * p.n_blocks;
  const int m0 = m_blk * BM;
  const int n0 = n_blk * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const nbdt_conv_desc& d = p.d;
  const int cin = __builtin_amdgcn_readfirstlane(d.cin);
  const int nk = cin >> 5;
  const bf16_t* in_base = p.in;
  const bf16_t* w_base = p.w;

  // ---- DMA slot tables (fixed per block): LDS position (row, cpos) receives data chunk cpos ^ swz(row)
  const int cpos = lane & 3;
  int a_src[A_IPW];
#pragma unroll
  for (int k = 0; k < A_IPW; ++k) {
    const int row = (wave + PW_WAVES * k) * 16 + (lane >> 2);
    int m = m0 + row;
    m = m < p.M ? m : p.M - 1;        // rows past M: the last interior pixel again (never stored)
    a_src[k] = pix_offset(m, d.gh, d.gw, d.in_bs, d.in_hs, d.in_ws, d.in_base) + d.tap_off[0] +
               ((cpos ^ ((row >> 2) & 3)) << 3);
  }
  int w_src[W_IPW];
#pragma unroll
  for (int k = 0; k < W_IPW; ++k) {
    const int id = ((wave + 4) & 7) + PW_WAVES * k;
    int row = id * 16 + (lane >> 2);
    row = row < BN ? row : BN - 1;
    w_src[k] = (n0 + row) * cin + ((cpos ^ ((row >> 2) & 3)) << 3);
  }
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;

  auto issue = [&](int slot, int kc) {
    const unsigned dst0 = lds_base + slot * STAGE;
#pragma unroll
    for (int k = 0; k < A_IPW; ++k)
      glds16(in_base + (a_src[k] + kc * BK), __builtin_amdgcn_readfirstlane(dst0 + (wave + PW_WAVES * k) * 1024));
#pragma unroll
    for (int k = 0; k < W_IPW; ++k) {
      const int id = ((wave + 4) & 7) + PW_WAVES * k;
      if (id < W_INSTR) {  // wave-uniform
        glds16(w_base + (w_src[k] + kc * BK), __builtin_amdgcn_readfirstlane(dst0 + A_BYTES + id * 1024));
      }
    }
  };

  f32x16 acc[NT][1];
#pragma unroll
  for (int tn = 0; tn < NT; ++tn)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[tn][0][r] = 0.f;

  const int frag_row = lane & 31;
  const int frag_half = lane >> 5;

  auto compute = [&](int slot) {
    const unsigned char* As = smem + slot * STAGE;
    const unsigned char* Ws = As + A_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = 2 * ks + frag_half;
      const bf16x8 pf = *(const bf16x8*)(As + lds_off(wave * 32 + frag_row, c));
#pragma unroll
      for (int tn = 0; tn < NT; ++tn) {
        const bf16x8 wf = *(const bf16x8*)(Ws + lds_off(tn * 32 + frag_row, c));
        acc[tn][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, pf, acc[tn][0], 0, 0, 0);
      }
    }
  };

  // ---- pipeline over the 32-channel K steps, ascending
  issue(0, 0);
  if (nk > 1) issue(1, 1);
  int slot = 0;
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) {
      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(MINPW) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();     // step t has landed for every wave; everybody is done reading step t - 1's slot
    asm volatile("" ::: "memory");
    if (t + 2 < nk) {
      int s2 = slot + 2;
      s2 = s2 >= NSTAGE ? s2 - NSTAGE : s2;
      issue(s2, t + 2);
    }
    compute(slot);
    slot = slot + 1 == NSTAGE ? 0 : slot + 1;
  }

  static_assert(conv_epilogue_lds_bytes<NT, PW_WAVES>() + pw_stat_scratch<NT>() <= pw_lds_bytes<NT>(), "epilogue does not fit");
  conv_epilogue<NT, HAS_RES, 0, PW_WAVES, 1>(acc, p, epi_lds_packed<NT, PW_WAVES>(smem, wave), m0, n0, m_blk, wave, lane,
                                             tid);
  if (STATS == 1) {
    // Per-channel sum / sum of squares of the tile's bf16 outputs, read back from the waves' transposition regions and
    // added IN THE ORDER nbdt_conv_igemm_stats ADDS THEM for this cout, so that the two entries leave the same bits (a
    // 1-ulp difference in a BatchNorm mean is enough to decorrelate the small gradients of a 50-layer net at random
    // initialisation: switching a launch between the kernels must not be a numerical event).  That kernel's wave w4 owns
    // pixels 64 w4 .. 64 w4 + 63 as two 32-row fragments (here: waves 2 w4 and 2 w4 + 1); its lane (w4, rl) runs ONE chain
    // over rows rl, rl + RL, .. of the first fragment and then of the second, RL = 64 / (cout tile / 8) of ITS cout tile
    // (160 / 128 / 96 / 64 / 32 wide by divisibility of cout); the block then adds the 4 RL chains in (w4, rl) order.
    constexpr int PITCH = 2 * BN + 16, REGION = 32 * PITCH;
    constexpr int TRIPS = pw_stat_trips<NT>();
    // (nt_o: the cout-tile ladder of conv_igemm_dma in conv_dma.hip -- keep the two in step;
    //  tests/test_conv_pw_gpu.py compares the partial sums of the two entries bit for bit)
    const int nt32 = d.cout >> 5;
    const int nt_o = nt32 % 5 == 0 ? 5 : nt32 % 4 == 0 ? 4 : nt32 % 3 == 0 ? 3 : nt32 % 2 == 0 ? 2 : 1;
    const int rl_o = __builtin_amdgcn_readfirstlane(16 / nt_o);
    float* scratch = (float*)(smem + (TRIPS > 1 ? conv_epilogue_lds_bytes<NT, PW_WAVES>() : 0));
    __syncthreads();          // every wave's [32 rows][BN] bf16 tile is in its region
    float p1[TRIPS][16], p2[TRIPS][16];
#pragma unroll
    for (int trip = 0; trip < TRIPS; ++trip) {
      const int item = tid + trip * 64 * PW_WAVES;
      const int c = item % BN, w4 = item / BN;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float a1 = 0.f, a2 = 0.f;
        if (r < rl_o && w4 < 4) {
#pragma unroll
          for (int tm = 0; tm < 2; ++tm) {
            const unsigned char* rg = smem + (2 * w4 + tm) * REGION + c * 2;
            const int mbase = m0 + (2 * w4 + tm) * 32;
            for (int row = r; row < 32; row += rl_o) {
              const float f = __uint_as_float((unsigned)(*(const unsigned short*)(rg + row * PITCH)) << 16);
              const float v = f * (mbase + row < p.M ? 1.f : 0.f);
              a1 += v;
              a2 += v * v;
            }
          }
        }
        p1[trip][r] = a1;
        p2[trip][r] = a2;
      }
    }
    if (TRIPS == 1) __syncthreads();      // the chains live in registers; the regions may now be overwritten
#pragma unroll
    for (int trip = 0; trip < TRIPS; ++trip) {
      const int item = tid + trip * 64 * PW_WAVES;
      if (item < BN * 4) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (r < rl_o) {
            scratch[(item * rl_o + r) * 2 + 0] = p1[trip][r];
            scratch[(item * rl_o + r) * 2 + 1] = p2[trip][r];
          }
      }
    }
    __syncthreads();
    float* part = p.stats + (size_t)m_blk * 2 * d.cout;
    for (int i = tid; i < 2 * BN; i += 64 * PW_WAVES) {
      const int which = i / BN, c = i - which * BN;
      float sum = 0.f;
      for (int w4 = 0; w4 < 4; ++w4)
        for (int r = 0; r < rl_o; ++r) sum += scratch[((w4 * BN + c) * rl_o + r) * 2 + which];
      part[(size_t)which * d.cout + n0 + c] = sum;
    }
  }
}

namespace nbdt {

template <int NT>
static int launch_pw(ConvDmaParams& p, hipStream_t st) {
  constexpr int BN = 32 * NT;
  p.n_blocks = p.d.cout / BN;
  p.m_blocks = (p.M + BM - 1) / BM;
  const int items = p.m_blocks * p.n_blocks;
  p.per_xcd = (items + 7) / 8;
  const size_t shmem = (size_t)pw_lds_bytes<NT>();
  static DeviceAttr site;     // one per NT instantiation
  if (site.need(shmem)) {
#define NBDT_ATTR(R, S)                                                                                  \
  NBDT_ATTR_CHECK(site, hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_pw_kernel<NT, R, S>),    \
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem))
    NBDT_ATTR(false, 0); NBDT_ATTR(true, 0); NBDT_ATTR(false, 1);
#undef NBDT_ATTR
    site.done(shmem);
  }
  const dim3 grid(p.per_xcd * 8), blk(64 * PW_WAVES);
#define NBDT_GO(R, S)                                                                                              \
  do {                                                                                                              \
    snprintf(g_last_igemm_full, sizeof(g_last_igemm_full), "conv_pw_kernel<%d, %s, %d>", NT, R ? "true" : "false", S); \
    hipLaunchKernelGGL((conv_pw_kernel<NT, R, S>), grid, blk, shmem, st, p);                                       \
  } while (0)
  if (p.stats != nullptr) NBDT_GO(false, 1);
  else if (p.res != nullptr) NBDT_GO(true, 0);
  else NBDT_GO(false, 0);
#undef NBDT_GO
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

// cout tile of a launch: the widest of 5 / 4 / 3 / 2 / 1 (x 32 channels, dividing cout) that gives each of the 256 CUs a
// block, else the narrowest; a statistics launch takes NT = 1 only when nothing else divides cout / 32
static int pw_cout_tile(int M, int cout, bool stats) {
  const int nt32 = cout / 32, m_blocks = (M + BM - 1) / BM;
  int narrowest = 0;
  for (int nt = 5; nt >= 1; --nt) {
    if (nt32 % nt != 0) continue;
    if (nt == 1 && stats && narrowest != 0) break;
    if ((long long)m_blocks * (nt32 / nt) >= 256) return nt;
    narrowest = nt;
  }
  return narrowest;
}

}  // namespace nbdt

extern "C" int nbdt_conv_pw(const nbdt_conv_desc* d, const void* in, const void* w, void* out, float* bn_partials,
                            void* stream) {
  NBDT_REQUIRE(d && in && w && out, "null argument");
  NBDT_REQUIRE(d->cin > 0 && d->cin % 32 == 0, "cin must be a multiple of 32");
  NBDT_REQUIRE(d->cout > 0 && d->cout % 32 == 0, "cout must be a multiple of 32");
  NBDT_REQUIRE(d->ntaps == 1 && d->w_ntaps == 1 && d->w_tap[0] == 0, "a pointwise launch has one tap");
  NBDT_REQUIRE(d->in_ws == d->cin && d->out_ws == d->cout,
               "stride-1 1x1 convolutions over dense pixels only (strided ones go to nbdt_conv_igemm)");
  NBDT_REQUIRE(d->B > 0 && d->gh > 0 && d->gw > 0, "empty pixel grid");
  NBDT_REQUIRE(d->in_base >= 0 && d->out_base >= 0 && d->in_hs > 0 && d->out_hs > 0 && d->in_bs > 0 && d->out_bs > 0 &&
               d->tap_off[0] >= 0, "negative pixel offsets");
  NBDT_REQUIRE((d->in_base % 8) == 0 && (d->in_hs % 8) == 0 && (d->in_bs % 8) == 0 && (d->tap_off[0] % 8) == 0,
               "input pixel offsets must be 16-byte aligned");
  NBDT_REQUIRE((d->out_base % 8) == 0 && (d->out_hs % 8) == 0 && (d->out_bs % 8) == 0,
               "output pixel offsets must be 16-byte aligned");
  NBDT_REQUIRE(d->accumulate == 0 || d->accumulate == 1, "accumulate is 0 or 1");
  NBDT_REQUIRE(!(bn_partials != nullptr && d->accumulate), "fused statistics are for plain outputs");
  const int64_t M64 = (int64_t)d->B * d->gh * d->gw;
  NBDT_REQUIRE(M64 < (1ll << 31), "pixel grid too large");
  {   // signed 32-bit ELEMENT offsets: a_src[] here, row_off[] in the shared epilogue (conv_common.h), w_src[]
    const int64_t out_last = (int64_t)(d->B - 1) * d->out_bs + (int64_t)(d->gh - 1) * d->out_hs +
                             (int64_t)(d->gw - 1) * d->out_ws + d->cout;
    const int64_t in_last = (int64_t)(d->B - 1) * d->in_bs + (int64_t)(d->gh - 1) * d->in_hs +
                            (int64_t)(d->gw - 1) * d->in_ws + d->cin;
    const int64_t out_all = (int64_t)d->B * d->out_bs, in_all = (int64_t)d->B * d->in_bs;
    // (B * bs bounds every pixel of a padded NHWC map, base included; the last pixel's own end covers any other map)
    NBDT_REQUIRE((in_all > in_last + d->in_base ? in_all : in_last + d->in_base) + d->tap_off[0] < (1ll << 31),
                 "input elements: B * in_bs + tap_off must stay below 2^31 (32-bit element offsets)");
    NBDT_REQUIRE((out_all > out_last + d->out_base ? out_all : out_last + d->out_base) < (1ll << 31),
                 "output elements: B * out_bs must stay below 2^31 (32-bit element offsets)");
    NBDT_REQUIRE((int64_t)d->cin * d->cout < (1ll << 31), "weight elements: cin * cout must stay below 2^31");
  }
  nbdt::ConvDmaParams p{};
  p.d = *d;
  p.in = (const bf16_t*)in;
  p.w = (const bf16_t*)w;
  p.out = (bf16_t*)out;
  p.res = d->accumulate ? (const bf16_t*)out : nullptr;
  p.stats = bn_partials;
  p.M = (int)M64;
  const int nt = nbdt::pw_cout_tile(p.M, d->cout, bn_partials != nullptr);
  nbdt::g_last_igemm = "conv_pw_kernel";
  hipStream_t st = (hipStream_t)stream;
  switch (nt) {
    case 5: return nbdt::launch_pw<5>(p, st);
    case 4: return nbdt::launch_pw<4>(p, st);
    case 3: return nbdt::launch_pw<3>(p, st);
    case 2: return nbdt::launch_pw<2>(p, st);
    default: return nbdt::launch_pw<1>(p, st);
  }
}
