// The rules layer on NCHW logits (segmentation: SegNBDT / SoftSegTreeSupLoss), included at the end of rules.hip.
//
// The reference coerces [N,C,H,W] to [N*H*W, C] rows, runs the row rules and permutes back (nbdt/model.py:376-399,
// nbdt/loss.py:318-327).  On the row kernels above that gives every pixel a group of at least 64 lanes for a few dozen
// classes, and costs four permute passes.  Here ONE LANE OWNS ONE PIXEL and a wave owns 64 consecutive pixels of one
// image: a class plane is contiguous over pixels, so every class read is one coalesced wave-wide load, and the hierarchy
// is the same for every lane, so walking it is scalar work and the soft path has no divergence at all.
//
// Per-pixel state that is indexed dynamically cannot live in registers; it is R + F rows of LDS laid out [row][64 lanes]
// (lane l touches bank l: no conflicts, and no barrier anywhere -- a lane only ever reads what it wrote):
//   S [R rows]  child logits, overwritten by the child probabilities, overwritten by dL/ds over the slot's leaf count
//   T [F rows]  the G sums of the node being differentiated (F = the largest fan-out; 2 for a binary hierarchy)
// Everything indexed by class stays in global memory: z is re-read through L1/L2 where an ordered chain needs it (L
// coalesced loads per pixel in place of C), and the backward keeps P, then P*g, then the path sums in the gz plane it is
// about to overwrite (a lane reads back only its own stores).  Staging the C logits in LDS as well would cost C more
// rows; at ADE20K (C 150, R 298) that is 115 KB per wave against 77 KB, one wave per CU against two, and the loads it
// saves are L2 hits.  DESIGN.md 25 has the numbers.
//
// An ordered chain cannot be split, but its loads can run ahead: flat_chains walks a CSR map in blocks of kPixU
// elements, issues a block's loads together, one block ahead of the fold, and folds them in order, closing a segment
// where the map's own words say so (a first version read the offset arrays with scalar loads: one exposed scalar-cache
// round trip per element, 13.3 ms for the ADE20K forward against 13.6 ms on the coerced path; profiles/seg_rules.txt).
// The arithmetic is rules.hip's contract: sequential fp32 sums in ascending class order and one IEEE
// division; first maximum; path product 1.0f * p(node_1) * p(node_2) ... in inode order -- so child logits, node
// decisions and hard predictions are bit-equal to the row kernels' on the coerced tensor.  The cross-entropy sums run
// sequentially in a lane here and as a butterfly over lanes there, so losses and gradients agree to rounding only.
//
// Limit of this form: R + F <= kPixMaxRows = 640 (160 KB of LDS / 256 B per row).  F <= R, so 2R <= 640 always fits.

constexpr int kPixLanes = 64;
constexpr int kPixU = 32;         // loads in flight per lane in a chain (LDS bounds the occupancy, registers are plentiful)
constexpr int kPixMaxRows = 640;  // kLdsBytes / (kPixLanes * sizeof(float))

struct PixGeom {
  int64_t HW, chunks;  // pixels per plane, blocks per image
  int64_t zi, zc;      // image and channel stride of z, in elements
  const int32_t *pslot, *pcls;  // the two CSR maps as packed words (flat_chains)
  int binary;                   // every inner node has two children: node n owns slots 2n, 2n + 1
};

#define NBDT_PIX_PROLOGUE                                                              \
  extern __shared__ __attribute__((aligned(16))) float lds[];                          \
  const int lane = threadIdx.x;                                                        \
  const int64_t blk = blockIdx.x;                                                      \
  const int64_t img = blk / g.chunks;                                                  \
  const int64_t pix = (blk - img * g.chunks) * kPixLanes + lane;                       \
  const bool active = pix < g.HW;                                                      \
  const int64_t pc = active ? pix : g.HW - 1; /* tail lanes read the last pixel */     \
  const int64_t zbase = img * g.zi + pc;                                               \
  float* S = lds + lane;                                                               \
  float* T = S + (size_t)t.R * kPixLanes;                                              \
  (void)T; (void)zbase

// A CSR map as the pixel kernels walk it (built by nbdt_tree_create): one word per element, in order --
// bits 0..15 the index (class of a slot's leaf / slot on a class's path), bit 31 set on the last element of its segment
// (slot / class), bit 30 on the last element of the last slot of an inner node.  The words are read 32 at a time by a
// vector load (lane u holds element u of the block) and handed out by v_readlane, so the bookkeeping is scalar and no
// scalar memory load sits in front of a chain element.
constexpr unsigned kPixEnd = 0x80000000u, kPixNodeEnd = 0x40000000u;

// acc = OP(...OP(OP(init, load(i_0)), load(i_1))..., load(i_last)) for every segment of a packed map of L elements, in
// order; done(segment, acc, elements, last word) at its end.  The loads of block b + 1 are issued before block b is
// folded, and the words of block b + 2 before that.
template <typename OP, typename LOAD, typename DONE>
__device__ __forceinline__ void flat_chains(const int32_t* __restrict__ packed, int L, float init, int lane, LOAD load,
                                            DONE done) {
  const int nb = (L + kPixU - 1) / kPixU;
  auto words = [&](int b) { return packed[min(min(b, nb - 1) * kPixU + (lane & (kPixU - 1)), L - 1)]; };
  int seg = 0, cnt = 0;
  float acc = init;
  auto issue = [&](float (&x)[kPixU], int w) {
#pragma unroll
    for (int u = 0; u < kPixU; ++u) x[u] = load(__builtin_amdgcn_readlane(w, u) & 0xffff);
  };
  auto fold = [&](const float (&x)[kPixU], int wv, int b) {  // a block past the end (the last one again) folds nothing
#pragma unroll
    for (int u = 0; u < kPixU; ++u) {
      if (b * kPixU + u < L) {
        const unsigned w = (unsigned)__builtin_amdgcn_readlane(wv, u);
        acc = OP::ap(acc, x[u]);
        ++cnt;
        if (w & kPixEnd) {
          done(seg, acc, cnt, w);
          acc = init;
          cnt = 0;
          ++seg;
        }
      }
    }
  };
  // two register blocks take turns, so a fold waits for its own block only (a copy between them waited for both)
  float xa[kPixU], xb[kPixU];
  int w0 = words(0), w1 = words(1);
  issue(xa, w0);
  for (int b = 0; b < nb; b += 2) {
    issue(xb, w1);
    const int w2 = words(b + 2);
    fold(xa, w0, b);
    issue(xa, w2);
    const int w3 = words(b + 3);
    fold(xb, w1, b + 1);
    w0 = w2;
    w1 = w3;
  }
}

// S[s] = mean of the class logits under child s (nbdt/model.py:94-99)
template <typename LD>
__device__ __forceinline__ void pix_node_logits(const TreeView& t, const PixGeom& g, const void* __restrict__ z,
                                                int64_t zbase, int lane, float* S) {
  flat_chains<ChainAdd>(
      g.pslot, t.L, 0.f, lane, [&](int c) { return LD::at(z, zbase + (int64_t)c * g.zc); },
      [&](int s, float acc, int cnt, unsigned) { S[s * kPixLanes] = acc / (float)cnt; });
}

__device__ __forceinline__ void pix_softmax2(float s0, float s1, float& p0, float& p1) {
  const float m = fmaxf(s0, s1);
  const float e0 = expf(s0 - m), e1 = expf(s1 - m);
  float sum = 0.f;
  sum = sum + e0;
  sum = sum + e1;
  p0 = e0 / sum;
  p1 = e1 / sum;
}

// S[b..e) <- softmax(S[b..e)) for every inner node (nbdt/model.py:114): node_softmax's operations.  In a binary
// hierarchy node n owns slots 2n and 2n + 1: four nodes go together, so their LDS round trips and divisions overlap.
__device__ __forceinline__ void pix_node_softmax(const TreeView& t, const PixGeom& g, float* S) {
  int n = 0;
  if (g.binary)
    for (; n + 4 <= t.N; n += 4) {
      float s[8], p[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) s[k] = S[(2 * n + k) * kPixLanes];
#pragma unroll
      for (int k = 0; k < 8; k += 2) pix_softmax2(s[k], s[k + 1], p[k], p[k + 1]);
#pragma unroll
      for (int k = 0; k < 8; ++k) S[(2 * n + k) * kPixLanes] = p[k];
    }
  for (; n < t.N; ++n) {
    const int b = t.node_off[n], e = t.node_off[n + 1];
    if (e - b == 2) {
      float p0, p1;
      pix_softmax2(S[b * kPixLanes], S[(b + 1) * kPixLanes], p0, p1);
      S[b * kPixLanes] = p0;
      S[(b + 1) * kPixLanes] = p1;
      continue;
    }
    float m = S[b * kPixLanes];
    for (int s = b + 1; s < e; ++s) m = fmaxf(m, S[s * kPixLanes]);
    float sum = 0.f;
    for (int s = b; s < e; ++s) {
      const float ex = expf(S[s * kPixLanes] - m);
      S[s * kPixLanes] = ex;
      sum = sum + ex;
    }
    for (int s = b; s < e; ++s) S[s * kPixLanes] = S[s * kPixLanes] / sum;
  }
}

// tree_backward's operations: with pq(c) = P[c] * dL/dP[c], G[s] = ordered sum of pq over the leaves of slot s; per node
// tot = sum of its G, dL/ds = G[s] - p[s] * tot; S[s] <- dL/ds over the slot's leaf count (what each leaf receives).
// A binary node keeps its two sums and leaf counts in registers; any other fan-out parks the sums in T.
template <typename LOAD>
__device__ __forceinline__ void pix_tree_backward(const TreeView& t, const PixGeom& g, int lane, float* S, float* T,
                                                  LOAD pq) {
  int first = 0, cnt_prev = 0;  // first slot of the node being summed; leaf count of the slot before this one
  float g_prev = 0.f;
  flat_chains<ChainAdd>(g.pslot, t.L, 0.f, lane, pq, [&](int s, float acc, int cnt, unsigned w) {
    if ((w & kPixNodeEnd) && s == first + 1) {
      float tot = 0.f;
      tot = tot + g_prev;
      tot = tot + acc;
      const float d0 = g_prev - S[first * kPixLanes] * tot, d1 = acc - S[s * kPixLanes] * tot;
      S[first * kPixLanes] = d0 / (float)cnt_prev;
      S[s * kPixLanes] = d1 / (float)cnt;
      first = s + 1;
      return;
    }
    T[(s - first) * kPixLanes] = acc;
    g_prev = acc;
    cnt_prev = cnt;
    if (w & kPixNodeEnd) {
      float tot = 0.f;
      for (int k = first; k <= s; ++k) tot = tot + T[(k - first) * kPixLanes];
      for (int k = first; k <= s; ++k) {
        const float ds = T[(k - first) * kPixLanes] - S[k * kPixLanes] * tot;
        S[k * kPixLanes] = ds / (float)(t.slot_off[k + 1] - t.slot_off[k]);
      }
      first = s + 1;
    }
  });
}

template <typename LD>
__global__ __launch_bounds__(kPixLanes) void pix_soft_fwd_kernel(TreeView t, PixGeom g, const void* __restrict__ z,
                                                                 float* P) {
  NBDT_PIX_PROLOGUE;
  pix_node_logits<LD>(t, g, z, zbase, lane, S);
  pix_node_softmax(t, g, S);
  float* Pp = P + img * t.C * g.HW + pc;
  flat_chains<ChainMul>(
      g.pcls, t.L, 1.0f, lane, [&](int s) { return S[s * kPixLanes]; },
      [&](int c, float acc, int, unsigned) {
        if (active) Pp[(int64_t)c * g.HW] = acc;
      });
}

template <typename LD>
__global__ __launch_bounds__(kPixLanes) void pix_soft_bwd_kernel(TreeView t, PixGeom g, const void* __restrict__ z,
                                                                 const float* gP, float* gz) {
  NBDT_PIX_PROLOGUE;
  pix_node_logits<LD>(t, g, z, zbase, lane, S);
  pix_node_softmax(t, g, S);
  float* G = gz + img * t.C * g.HW + pc;  // this pixel's gz column: P, then P * gP, then the result
  const float* gp = gP + img * t.C * g.HW + pc;
  flat_chains<ChainMul>(
      g.pcls, t.L, 1.0f, lane, [&](int s) { return S[s * kPixLanes]; },
      [&](int c, float acc, int, unsigned) {
        if (active) G[(int64_t)c * g.HW] = acc;
      });
  for (int c0 = 0; c0 < t.C; c0 += kPixU) {
    float p[kPixU], q[kPixU];
#pragma unroll
    for (int u = 0; u < kPixU; ++u) {
      const int64_t o = (int64_t)min(c0 + u, t.C - 1) * g.HW;
      p[u] = G[o];
      q[u] = gp[o];
    }
#pragma unroll
    for (int u = 0; u < kPixU; ++u)
      if (c0 + u < t.C && active) G[(int64_t)(c0 + u) * g.HW] = p[u] * q[u];
  }
  pix_tree_backward(t, g, lane, S, T, [&](int c) { return G[(int64_t)c * g.HW]; });
  flat_chains<ChainAdd>(
      g.pcls, t.L, 0.f, lane, [&](int s) { return S[s * kPixLanes]; },
      [&](int c, float acc, int, unsigned) {
        if (active) G[(int64_t)c * g.HW] = acc;
      });
}

// SoftSegTreeSupLoss forward + backward for nn.CrossEntropyLoss(ignore_index = I, label_smoothing = eps), mean over the
// pixels with y != I (their number is *n_valid, counted by pix_count_kernel in front of this launch):
//   t'_c = (1 - eps) * 1[c == y] + eps / C,  T = sum_c t'_c
//   row  = w_x * (T * lse(z) - sum_c t'_c z_c) + w_t * (T * lse(P) - sum_c t'_c P_c)      (soft_loss_from_lds_logits, SOFT)
//   gz   = grad_scale / n_valid * ( w_x * (T * softmax(z) - t') + J^T w_t * (T * softmax(P) - t') ),  0 where y == I.
// The wave's row losses are summed by a butterfly into partial[block]; pix_fold_kernel adds the partials in block order.
template <typename LD>
__global__ __launch_bounds__(kPixLanes) void pix_soft_loss_kernel(TreeView t, PixGeom g, const void* __restrict__ z,
                                                                  const int64_t* __restrict__ y, int64_t ignore,
                                                                  float eps, float w_x, float w_t, float grad_scale,
                                                                  const int* __restrict__ n_valid, float* partial,
                                                                  float* gz) {
  NBDT_PIX_PROLOGUE;
  const int64_t yy = y[img * g.HW + pc];
  const bool valid = active && yy != ignore;
  float* G = gz + img * t.C * g.HW + pc;  // this pixel's gz column: P, then P * dL/dP, then the path sums, then the result
  if (__ballot(valid) == 0) {               // nothing to learn from these 64 pixels
    if (active)
      for (int c = 0; c < t.C; ++c) G[(int64_t)c * g.HW] = 0.f;
    if (lane == 0) partial[blk] = 0.f;
    return;
  }
  const float scale = grad_scale / (float)n_valid[0];
  pix_node_logits<LD>(t, g, z, zbase, lane, S);
  pix_node_softmax(t, g, S);
  flat_chains<ChainMul>(
      g.pcls, t.L, 1.0f, lane, [&](int s) { return S[s * kPixLanes]; },
      [&](int c, float acc, int, unsigned) {
        if (active) G[(int64_t)c * g.HW] = acc;
      });

  const float uni = eps / (float)t.C;
  float mz = -INFINITY, mp = -INFINITY, st = 0.f, stz = 0.f, stp = 0.f;
  for (int c0 = 0; c0 < t.C; c0 += kPixU) {
    float zc[kPixU], p[kPixU];
#pragma unroll
    for (int u = 0; u < kPixU; ++u) {
      const int c = min(c0 + u, t.C - 1);
      zc[u] = LD::at(z, zbase + (int64_t)c * g.zc);
      p[u] = G[(int64_t)c * g.HW];
    }
#pragma unroll
    for (int u = 0; u < kPixU; ++u)
      if (c0 + u < t.C) {
        const float ts = (1.f - eps) * ((c0 + u == yy) ? 1.f : 0.f) + uni;
        mz = fmaxf(mz, zc[u]);
        mp = fmaxf(mp, p[u]);
        st += ts;
        stz += ts * zc[u];
        stp += ts * p[u];
      }
  }
  float sz = 0.f, sp = 0.f;
  for (int c0 = 0; c0 < t.C; c0 += kPixU) {
    float zc[kPixU], p[kPixU];
#pragma unroll
    for (int u = 0; u < kPixU; ++u) {
      const int c = min(c0 + u, t.C - 1);
      zc[u] = LD::at(z, zbase + (int64_t)c * g.zc);
      p[u] = G[(int64_t)c * g.HW];
    }
#pragma unroll
    for (int u = 0; u < kPixU; ++u)
      if (c0 + u < t.C) {
        sz += expf(zc[u] - mz);
        sp += expf(p[u] - mp);
      }
  }
  for (int c0 = 0; c0 < t.C; c0 += kPixU) {
    float p[kPixU];
#pragma unroll
    for (int u = 0; u < kPixU; ++u) p[u] = G[(int64_t)min(c0 + u, t.C - 1) * g.HW];
#pragma unroll
    for (int u = 0; u < kPixU; ++u)
      if (c0 + u < t.C) {
        const float ts = (1.f - eps) * ((c0 + u == yy) ? 1.f : 0.f) + uni;
        const float gp = (st * (expf(p[u] - mp) / sp) - ts) * (w_t * scale);
        if (active) G[(int64_t)(c0 + u) * g.HW] = p[u] * gp;
      }
  }
  float row = 0.f;
  if (valid)
    row = (yy >= 0 && yy < t.C) ? w_x * (st * (logf(sz) + mz) - stz) + w_t * (st * (logf(sp) + mp) - stp)
                                : __uint_as_float(0x7fc00000u);  // loud: NaN loss
  pix_tree_backward(t, g, lane, S, T, [&](int c) { return G[(int64_t)c * g.HW]; });
  flat_chains<ChainAdd>(
      g.pcls, t.L, 0.f, lane, [&](int s) { return S[s * kPixLanes]; },
      [&](int c, float acc, int, unsigned) {
        if (active) G[(int64_t)c * g.HW] = acc;
      });
  for (int c0 = 0; c0 < t.C; c0 += kPixU) {
    float zc[kPixU], d[kPixU];
#pragma unroll
    for (int u = 0; u < kPixU; ++u) {
      const int c = min(c0 + u, t.C - 1);
      zc[u] = LD::at(z, zbase + (int64_t)c * g.zc);
      d[u] = G[(int64_t)c * g.HW];
    }
#pragma unroll
    for (int u = 0; u < kPixU; ++u)
      if (c0 + u < t.C) {
        const float ts = (1.f - eps) * ((c0 + u == yy) ? 1.f : 0.f) + uni;
        const float gx = (st * (expf(zc[u] - mz) / sz) - ts) * (w_x * scale);
        if (active) G[(int64_t)(c0 + u) * g.HW] = valid ? gx + d[u] : 0.f;
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) row += __shfl_xor(row, o, 64);
  if (lane == 0) partial[blk] = row;
}

// *n_valid += the number of targets that are not `ignore` (integer adds: any order gives the same count)
__global__ __launch_bounds__(kBlock) void pix_count_kernel(const int64_t* __restrict__ y, int64_t n, int64_t ignore,
                                                           int* n_valid) {
  int mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    mine += y[i] != ignore;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_valid, mine);
}

// loss = (partial[0] + partial[1] + ...) / n_valid: a thread adds its partials in ascending order, the 256 threads are
// added in ascending order -- the same bits on every run.  No valid pixel gives 0 / 0 = NaN, as torch's mean does.
__global__ __launch_bounds__(kBlock) void pix_fold_kernel(const float* __restrict__ partial, int64_t n,
                                                          const int* __restrict__ n_valid, float* __restrict__ loss) {
  __shared__ float red[kBlock];
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) acc = acc + partial[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int i = 0; i < kBlock; ++i) tot = tot + red[i];
    loss[0] = tot / (float)n_valid[0];
  }
}

// Greedy root-to-leaf walk per pixel (nbdt/model.py:145-192): the lanes of a wave part ways here, so a lane reads its
// node's offsets itself; the first maximum wins.
template <typename LD>
__global__ __launch_bounds__(kPixLanes) void pix_hard_fwd_kernel(TreeView t, PixGeom g, const void* __restrict__ z,
                                                                 int64_t* __restrict__ pred,
                                                                 float* __restrict__ onehot) {
  NBDT_PIX_PROLOGUE;
  pix_node_logits<LD>(t, g, z, zbase, lane, S);
  int n = t.root, cls = -1;
  for (int d = 0; d < t.max_depth; ++d) {
    const int b = t.node_off[n], e = t.node_off[n + 1];
    int best = b;
    float top = S[b * kPixLanes];
    for (int s = b + 1; s < e; ++s) {
      const float v = S[s * kPixLanes];
      if (v > top) { top = v; best = s; }
    }
    const int nx = t.slot_next[best];
    if (nx < 0) {
      cls = -nx - 1;
      break;
    }
    n = nx;
  }
  if (!active) return;
  pred[img * g.HW + pix] = cls;
  if (onehot) {
    float* O = onehot + img * t.C * g.HW + pix;
    for (int c = 0; c < t.C; ++c) O[(int64_t)c * g.HW] = (c == cls) ? 1.f : 0.f;
  }
}

// ------------------------------------------------------------------------------------------
// host side

static int pix_rows(const nbdt_tree* t) { return t->R + t->max_fan; }

extern "C" int nbdt_seg_pixel_fits(const nbdt_tree* t) { return t != nullptr && t->pix_ok && pix_rows(t) <= kPixMaxRows; }

extern "C" int64_t nbdt_seg_loss_workspace_floats(int64_t N, int64_t HW) {
  if (N <= 0 || HW <= 0) return 4;
  return 4 + N * ((HW + kPixLanes - 1) / kPixLanes);
}

static int pix_check(const nbdt_tree* t, const void* z, int ztype, int64_t N, int64_t HW, int64_t zi, int64_t zc,
                     PixGeom* g, unsigned* grid) {
  NBDT_REQUIRE(t != nullptr, "null tree handle");
  NBDT_REQUIRE(z != nullptr || N == 0, "null logits");
  NBDT_REQUIRE(ztype == NBDT_F32 || ztype == NBDT_BF16 || ztype == NBDT_F16, "unsupported logits dtype");
  NBDT_REQUIRE(N >= 0 && HW > 0, "bad image count / plane size");
  NBDT_REQUIRE(zc >= HW && zi >= (int64_t)(t->C - 1) * zc + HW, "bad channel / image stride (planes must not overlap)");
  NBDT_REQUIRE(t->pix_ok && pix_rows(t) <= kPixMaxRows,
               "hierarchy beyond the pixel form (child slots + largest fan-out > 640): run the row kernels on the "
               "coerced [N*H*W, C] tensor");
  g->HW = HW; g->chunks = (HW + kPixLanes - 1) / kPixLanes; g->zi = zi; g->zc = zc;
  g->pslot = t->pix_slot; g->pcls = t->pix_cls; g->binary = t->binary;
  NBDT_REQUIRE(N == 0 || g->chunks <= (int64_t)0x7fffffff / N, "more than 2^31 blocks of 64 pixels");
  *grid = (unsigned)(N * g->chunks);
  return NBDT_OK;
}

#define NBDT_PIX_LAUNCH(KERNEL, ...)                                                                          \
  do {                                                                                                        \
    const size_t shmem = (size_t)pix_rows(t) * kPixLanes * sizeof(float);                                     \
    hipStream_t st = (hipStream_t)stream;                                                                     \
    int lrc;                                                                                                  \
    if (ztype == NBDT_F32) lrc = launch_rules(KERNEL<LoadF32>, grid, kPixLanes, shmem, st, __VA_ARGS__);      \
    else if (ztype == NBDT_BF16) lrc = launch_rules(KERNEL<LoadBF16>, grid, kPixLanes, shmem, st, __VA_ARGS__); \
    else lrc = launch_rules(KERNEL<LoadF16>, grid, kPixLanes, shmem, st, __VA_ARGS__);                        \
    if (lrc) return lrc;                                                                                      \
    g_last_rules_path = 4;                                                                                    \
  } while (0)

extern "C" int nbdt_seg_soft_forward(const nbdt_tree* t, const void* z, int ztype, int64_t N, int64_t HW, int64_t zi,
                                     int64_t zc, float* P, void* stream) {
  PixGeom g;
  unsigned grid = 0;
  int rc = pix_check(t, z, ztype, N, HW, zi, zc, &g, &grid);
  if (rc) return rc;
  if (N == 0) return NBDT_OK;
  NBDT_REQUIRE(P != nullptr, "null output");
  TreeView v = view_of(t);
  NBDT_PIX_LAUNCH(pix_soft_fwd_kernel, v, g, z, P);
  return NBDT_OK;
}

extern "C" int nbdt_seg_soft_backward(const nbdt_tree* t, const void* z, int ztype, int64_t N, int64_t HW, int64_t zi,
                                      int64_t zc, const float* gP, float* gz, void* stream) {
  PixGeom g;
  unsigned grid = 0;
  int rc = pix_check(t, z, ztype, N, HW, zi, zc, &g, &grid);
  if (rc) return rc;
  if (N == 0) return NBDT_OK;
  NBDT_REQUIRE(gP != nullptr && gz != nullptr && (const void*)gz != z && gz != gP, "null or aliased gradient buffer");
  TreeView v = view_of(t);
  NBDT_PIX_LAUNCH(pix_soft_bwd_kernel, v, g, z, gP, gz);
  return NBDT_OK;
}

extern "C" int nbdt_seg_soft_tree_loss(const nbdt_tree* t, const void* z, int ztype, int64_t N, int64_t HW, int64_t zi,
                                       int64_t zc, const int64_t* y, int64_t ignore_index, float smoothing,
                                       float w_xent, float w_tree, float grad_scale, float* workspace, float* loss,
                                       float* gz, void* stream) {
  PixGeom g;
  unsigned grid = 0;
  int rc = pix_check(t, z, ztype, N, HW, zi, zc, &g, &grid);
  if (rc) return rc;
  NBDT_REQUIRE(N > 0, "empty batch has no mean loss");
  NBDT_REQUIRE(y && workspace && loss && gz && (const void*)gz != z, "null or aliased buffer");
  NBDT_REQUIRE(smoothing >= 0.f && smoothing < 1.f, "label smoothing must be in [0, 1)");
  // (addresses are 64-bit throughout; the count of valid pixels -- pix_count_kernel, the loss's divisor -- is an int)
  NBDT_REQUIRE(HW < (1ll << 31) && N <= ((1ll << 31) - 1) / HW, "pixels: N * HW must stay below 2^31 (the valid-pixel count is a 32-bit integer)");
  TreeView v = view_of(t);
  int* n_valid = (int*)workspace;
  float* partial = workspace + 4;
  NBDT_HIP_CHECK(hipMemsetAsync(n_valid, 0, sizeof(int), (hipStream_t)stream));
  const int64_t ny = N * HW;
  const unsigned cgrid = (unsigned)std::min<int64_t>((ny + kBlock - 1) / kBlock, 4 * (int64_t)std::max(t->cus, 1));
  hipLaunchKernelGGL(pix_count_kernel, dim3(cgrid), dim3(kBlock), 0, (hipStream_t)stream, y, ny, ignore_index, n_valid);
  NBDT_LAUNCH_CHECK();
  NBDT_PIX_LAUNCH(pix_soft_loss_kernel, v, g, z, y, ignore_index, smoothing, w_xent, w_tree, grad_scale,
                  (const int*)n_valid, partial, gz);
  hipLaunchKernelGGL(pix_fold_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const float*)partial,
                     (int64_t)grid, (const int*)n_valid, loss);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}

extern "C" int nbdt_seg_hard_forward(const nbdt_tree* t, const void* z, int ztype, int64_t N, int64_t HW, int64_t zi,
                                     int64_t zc, int64_t* pred, float* onehot, void* stream) {
  PixGeom g;
  unsigned grid = 0;
  int rc = pix_check(t, z, ztype, N, HW, zi, zc, &g, &grid);
  if (rc) return rc;
  if (N == 0) return NBDT_OK;
  NBDT_REQUIRE(pred != nullptr, "null pred");
  TreeView v = view_of(t);
  NBDT_PIX_LAUNCH(pix_hard_fwd_kernel, v, g, z, pred, onehot);
  return NBDT_OK;
}
