// The per-sample rules kernels of rules.hip for hierarchies whose sample row does not fit LDS (included by rules.hip,
// after the LDS kernels: TreeView, the Load* types, the group_* reductions and the chain operators are theirs).
//
// One block of kGlobalBlock lanes owns one row of the library's per-(device, stream) workspace and strides over the
// samples, so the workspace is bounded by the grid (one block per CU), not by the batch:
//   row = [ zs: C | ss: R | ps: R | pq: C | gx: C ]     floats; the hard walk keeps [best_of: N | next_of: N] ints in
//                                                       place of pq / gx (global_row_floats)
// The row is written and read by its own block only; phases are separated by block barriers (a barrier orders the
// block's global stores before its later loads: both go through the CU's vector L1, and the row pointers are plain,
// never __restrict__ or const, so no load of a row is hoisted over a barrier or sent through the scalar cache).
// The hierarchy's arrays are read from global memory; they are shared by every block and stay in L2.
//
// The arithmetic contract is the LDS form's: a child logit is one lane's ordered chain over ascending class index (its
// loads run a block of 16 ahead of the adds, the indices one block further), a path product one lane's ordered chain in
// inode order, argmax takes the first maximum.  What differs is the order of sums the contract leaves open, and only for
// inner nodes with more than kWideFan children: their maximum, softmax denominator, entropy and gradient total are
// folded by the whole block (strided partial sums, then the fixed tree of group_sum), where the LDS form has one lane
// walk the children.  Nothing is summed with atomics and nothing depends on which block took a sample, so a sample's
// bits depend neither on the batch nor on the run.
#pragma once

constexpr int kGlobalBlock = 1024;  // lanes of a block = lanes of a sample
constexpr int kWideFan = 64;        // an inner node with more children is folded by the whole block

struct GlobalRows {
  float* rows;           // [grid][row_floats]
  size_t row_floats;
  const int32_t* wide;   // inner nodes with more than kWideFan children, ascending
  int n_wide;
};

struct GRow { float *zs, *ss, *ps, *pq, *gx; };

__device__ __forceinline__ GRow global_row(const TreeView& t, const GlobalRows& g) {
  GRow r;
  r.zs = g.rows + (size_t)blockIdx.x * g.row_floats;
  r.ss = r.zs + t.C;
  r.ps = r.ss + t.R;
  r.pq = r.ps + t.R;
  r.gx = r.pq + t.C;
  return r;
}

// acc = OP(...OP(OP(acc, src[idx[b]]), src[idx[b + 1]])..., src[idx[e - 1]]) in exactly that order
template <typename OP>
__device__ __forceinline__ float global_chain(const int32_t* __restrict__ idx, int b, int e, float* src, float acc) {
  constexpr int U = 16;
  int j = b;
  if (j + U <= e) {
    int i[U];
#pragma unroll
    for (int u = 0; u < U; ++u) i[u] = idx[j + u];
    for (; j + U <= e; j += U) {
      float x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) x[u] = src[i[u]];
      const int jn = (j + 2 * U <= e) ? j + U : j;  // past the last whole block: reload this one, never used
#pragma unroll
      for (int u = 0; u < U; ++u) i[u] = idx[jn + u];
#pragma unroll
      for (int u = 0; u < U; ++u) acc = OP::ap(acc, x[u]);
    }
  }
  for (; j < e; ++j) acc = OP::ap(acc, src[idx[j]]);
  return acc;
}

// phase 0: logits row -> zs (fp32)
template <typename LD>
__device__ __forceinline__ void global_load(const TreeView& t, const void* z, int64_t row_off, float* zs) {
  for (int c = threadIdx.x; c < t.C; c += kGlobalBlock) zs[c] = LD::at(z, row_off + c);
  __syncthreads();
}

// out[s] = ordered sum over the leaves of slot s of src[class] (divided by the leaf count when MEAN): one lane per slot
template <bool MEAN>
__device__ __forceinline__ void global_slot_sums(const TreeView& t, float* src, float* out) {
  for (int s = threadIdx.x; s < t.R; s += kGlobalBlock) {
    const int b = t.slot_off[s], e = t.slot_off[s + 1];
    const float acc = global_chain<ChainAdd>(t.slot_cls, b, e, src, 0.f);
    out[s] = MEAN ? acc / (float)(e - b) : acc;
  }
  __syncthreads();
}

// the first maximum of ss[b, e), by the whole block; every lane returns the same slot
__device__ __forceinline__ int global_wide_argmax(float* ss, int b, int e, float* red) {
  float v = -INFINITY;
  int i = 0x7fffffff;
  for (int s = b + (int)threadIdx.x; s < e; s += kGlobalBlock) {
    const float x = ss[s];
    if (x > v) { v = x; i = s; }
  }
  group_argmax<kGlobalBlock>(v, i, red, threadIdx.x);
  // The one-lane rule starts from the first child and moves on `x > best`: a NaN there is never beaten, and neither is
  // -inf when nothing compares greater.  Both keep the first child here too.
  const float first = ss[b];
  return (first != first || i == 0x7fffffff) ? b : i;
}

// per-node softmax (node_softmax of the LDS form; wide nodes by the whole block)
__device__ __forceinline__ void global_node_softmax(const TreeView& t, const GlobalRows& g, float* ss, float* ps, float* red) {
  for (int n = threadIdx.x; n < t.N; n += kGlobalBlock) {
    const int b = t.node_off[n], e = t.node_off[n + 1];
    if (e - b > kWideFan) continue;
    float m = ss[b];
    for (int s = b + 1; s < e; ++s) m = fmaxf(m, ss[s]);
    float sum = 0.f;
    for (int s = b; s < e; ++s) {
      const float ex = expf(ss[s] - m);
      ps[s] = ex;
      sum = sum + ex;
    }
    for (int s = b; s < e; ++s) ps[s] = ps[s] / sum;
  }
  for (int w = 0; w < g.n_wide; ++w) {
    const int n = g.wide[w];
    const int b = t.node_off[n], e = t.node_off[n + 1];
    float m = -INFINITY;
    for (int s = b + (int)threadIdx.x; s < e; s += kGlobalBlock) m = fmaxf(m, ss[s]);
    m = group_max<kGlobalBlock>(m, red, threadIdx.x);
    float sum = 0.f;
    for (int s = b + (int)threadIdx.x; s < e; s += kGlobalBlock) sum += expf(ss[s] - m);
    sum = group_sum<kGlobalBlock>(sum, red, threadIdx.x);
    for (int s = b + (int)threadIdx.x; s < e; s += kGlobalBlock) ps[s] = expf(ss[s] - m) / sum;
  }
  __syncthreads();
}

// node_entropy of a wide node's probabilities, by the whole block
__device__ __forceinline__ float global_wide_entropy(float* ps, int b, int e, float* red) {
  const float eps = 1.1920928955078125e-07f;
  float tot = 0.f;
  for (int s = b + (int)threadIdx.x; s < e; s += kGlobalBlock) tot += ps[s];
  tot = group_sum<kGlobalBlock>(tot, red, threadIdx.x);
  float h = 0.f;
  for (int s = b + (int)threadIdx.x; s < e; s += kGlobalBlock) {
    const float p = ps[s] / tot;
    h += p * logf(fminf(fmaxf(p, eps), 1.0f - eps));
  }
  return -group_sum<kGlobalBlock>(h, red, threadIdx.x);
}

// tree_backward of the LDS form: pq holds P*g per class; ss becomes G, then dL/ds over the slot's leaf count
__device__ __forceinline__ void global_tree_backward(const TreeView& t, const GlobalRows& g, float* ss, float* ps, float* pq,
                                                     float* red) {
  global_slot_sums<false>(t, pq, ss);
  for (int n = threadIdx.x; n < t.N; n += kGlobalBlock) {
    const int b = t.node_off[n], e = t.node_off[n + 1];
    if (e - b > kWideFan) continue;
    float tot = 0.f;
    for (int s = b; s < e; ++s) tot = tot + ss[s];
    for (int s = b; s < e; ++s) {
      const float ds = ss[s] - ps[s] * tot;
      ss[s] = ds / (float)(t.slot_off[s + 1] - t.slot_off[s]);
    }
  }
  for (int w = 0; w < g.n_wide; ++w) {
    const int n = g.wide[w];
    const int b = t.node_off[n], e = t.node_off[n + 1];
    float tot = 0.f;
    for (int s = b + (int)threadIdx.x; s < e; s += kGlobalBlock) tot += ss[s];
    tot = group_sum<kGlobalBlock>(tot, red, threadIdx.x);  // its barriers sit between the reads above and the writes below
    for (int s = b + (int)threadIdx.x; s < e; s += kGlobalBlock) {
      const float ds = ss[s] - ps[s] * tot;
      ss[s] = ds / (float)(t.slot_off[s + 1] - t.slot_off[s]);
    }
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------
// kernels: grid <= one block per CU, block b takes samples b, b + grid, ...

template <typename LD>
__global__ __launch_bounds__(kGlobalBlock) void global_soft_fwd_kernel(TreeView t, GlobalRows g, const void* z, int64_t B,
                                                                       int64_t ldz, float* __restrict__ P) {
  __shared__ float red[64];
  const GRow r = global_row(t, g);
  for (int64_t sample = blockIdx.x; sample < B; sample += gridDim.x) {
    global_load<LD>(t, z, sample * ldz, r.zs);
    global_slot_sums<true>(t, r.zs, r.ss);
    global_node_softmax(t, g, r.ss, r.ps, red);
    for (int c = threadIdx.x; c < t.C; c += kGlobalBlock)
      P[sample * t.C + c] = global_chain<ChainMul>(t.cls_slot, t.cls_off[c], t.cls_off[c + 1], r.ps, 1.0f);
    __syncthreads();  // the row is rewritten by the next sample
  }
}

template <typename LD>
__global__ __launch_bounds__(kGlobalBlock) void global_soft_bwd_kernel(TreeView t, GlobalRows g, const void* z, int64_t B,
                                                                       int64_t ldz, const float* __restrict__ gP,
                                                                       float* __restrict__ gz) {
  __shared__ float red[64];
  const GRow r = global_row(t, g);
  for (int64_t sample = blockIdx.x; sample < B; sample += gridDim.x) {
    global_load<LD>(t, z, sample * ldz, r.zs);
    global_slot_sums<true>(t, r.zs, r.ss);
    global_node_softmax(t, g, r.ss, r.ps, red);
    for (int c = threadIdx.x; c < t.C; c += kGlobalBlock) {
      const float p = global_chain<ChainMul>(t.cls_slot, t.cls_off[c], t.cls_off[c + 1], r.ps, 1.0f);
      r.pq[c] = p * gP[sample * t.C + c];
    }
    __syncthreads();
    global_tree_backward(t, g, r.ss, r.ps, r.pq, red);
    for (int c = threadIdx.x; c < t.C; c += kGlobalBlock)
      gz[sample * t.C + c] = global_chain<ChainAdd>(t.cls_slot, t.cls_off[c], t.cls_off[c + 1], r.ss, 0.f);
    __syncthreads();
  }
}

// soft_loss_kernel (SOFT = false) and soft_target_loss_kernel (SOFT = true): the operations of
// soft_loss_from_lds_logits, lane tid owning classes tid, tid + kGlobalBlock, ... in every class loop
template <typename LD, bool SOFT>
__device__ __forceinline__ void global_soft_loss(const TreeView& t, const GlobalRows& g, const void* z, int64_t B, int64_t ldz,
                                                 const int64_t* __restrict__ y, const float* __restrict__ tprob,
                                                 int64_t ldt, float eps, float w_x, float w_t, float scale,
                                                 float* __restrict__ row_loss, float* __restrict__ gz, float* red) {
  const GRow r = global_row(t, g);
  const int tid = threadIdx.x;
  for (int64_t sample = blockIdx.x; sample < B; sample += gridDim.x) {
    global_load<LD>(t, z, sample * ldz, r.zs);
    global_slot_sums<true>(t, r.zs, r.ss);
    global_node_softmax(t, g, r.ss, r.ps, red);
    const float* trow = (SOFT && tprob) ? tprob + sample * ldt : nullptr;
    float mz = -INFINITY, mp = -INFINITY;
    float st = 0.f, stz = 0.f, stp = 0.f;
    const float uni = SOFT ? eps / (float)t.C : 0.f;
    int64_t ys = -1;
    if (SOFT && !trow) ys = y[sample];
    for (int c = tid; c < t.C; c += kGlobalBlock) {
      const float p = global_chain<ChainMul>(t.cls_slot, t.cls_off[c], t.cls_off[c + 1], r.ps, 1.0f);
      const float zc = r.zs[c];
      r.pq[c] = p;
      mp = fmaxf(mp, p);
      mz = fmaxf(mz, zc);
      if (SOFT) {
        const float tc = trow ? trow[c] : ((c == ys) ? 1.f : 0.f);
        const float ts = (1.f - eps) * tc + uni;
        r.gx[c] = ts;
        st += ts;
        stz += ts * zc;
        stp += ts * p;
      }
    }
    mz = group_max<kGlobalBlock>(mz, red, tid);
    mp = group_max<kGlobalBlock>(mp, red, tid);
    float sz = 0.f, sp = 0.f;
    for (int c = tid; c < t.C; c += kGlobalBlock) {
      sz += expf(r.zs[c] - mz);
      sp += expf(r.pq[c] - mp);
    }
    sz = group_sum<kGlobalBlock>(sz, red, tid);
    sp = group_sum<kGlobalBlock>(sp, red, tid);
    if (SOFT) {
      st = group_sum<kGlobalBlock>(st, red, tid);
      stz = group_sum<kGlobalBlock>(stz, red, tid);
      stp = group_sum<kGlobalBlock>(stp, red, tid);
      for (int c = tid; c < t.C; c += kGlobalBlock) {
        const float ts = r.gx[c];
        const float p = r.pq[c];
        r.gx[c] = (st * (expf(r.zs[c] - mz) / sz) - ts) * (w_x * scale);
        const float gp = (st * (expf(p - mp) / sp) - ts) * (w_t * scale);
        r.pq[c] = p * gp;
      }
      if (tid == 0) {
        const bool valid = trow || (ys >= 0 && ys < t.C);
        row_loss[sample] = valid ? w_x * (st * (logf(sz) + mz) - stz) + w_t * (st * (logf(sp) + mp) - stp)
                                 : __uint_as_float(0x7fc00000u);  // loud: NaN loss
      }
    } else {
      const int64_t yy = y[sample];
      const bool valid = yy >= 0 && yy < t.C;
      for (int c = tid; c < t.C; c += kGlobalBlock) {
        const float hot = (c == yy) ? 1.f : 0.f;
        const float p = r.pq[c];
        const float zc = r.zs[c];
        if (c == yy) row_loss[sample] = w_x * ((logf(sz) + mz) - zc) + w_t * ((logf(sp) + mp) - p);
        r.gx[c] = (expf(zc - mz) / sz - hot) * (w_x * scale);
        const float gp = (expf(p - mp) / sp - hot) * (w_t * scale);
        r.pq[c] = p * gp;
      }
      if (!valid && tid == 0) row_loss[sample] = __uint_as_float(0x7fc00000u);  // loud: NaN loss
    }
    __syncthreads();
    global_tree_backward(t, g, r.ss, r.ps, r.pq, red);
    for (int c = tid; c < t.C; c += kGlobalBlock)
      gz[sample * t.C + c] = r.gx[c] + global_chain<ChainAdd>(t.cls_slot, t.cls_off[c], t.cls_off[c + 1], r.ss, 0.f);
    __syncthreads();
  }
}

template <typename LD>
__global__ __launch_bounds__(kGlobalBlock) void global_soft_loss_kernel(TreeView t, GlobalRows g, const void* z, int64_t B,
                                                                        int64_t ldz, const int64_t* __restrict__ y,
                                                                        float w_x, float w_t, float scale,
                                                                        float* __restrict__ row_loss,
                                                                        float* __restrict__ gz) {
  __shared__ float red[64];
  global_soft_loss<LD, false>(t, g, z, B, ldz, y, nullptr, 0, 0.f, w_x, w_t, scale, row_loss, gz, red);
}

template <typename LD>
__global__ __launch_bounds__(kGlobalBlock) void global_soft_target_loss_kernel(TreeView t, GlobalRows g, const void* z,
                                                                               int64_t B, int64_t ldz,
                                                                               const int64_t* __restrict__ y,
                                                                               const float* __restrict__ tprob, int64_t ldt,
                                                                               float eps, float w_x, float w_t, float scale,
                                                                               float* __restrict__ row_loss,
                                                                               float* __restrict__ gz) {
  __shared__ float red[64];
  global_soft_loss<LD, true>(t, g, z, B, ldz, y, tprob, ldt, eps, w_x, w_t, scale, row_loss, gz, red);
}

// node owning slot s: last n with node_off[n] <= s
__device__ __forceinline__ int global_node_of_slot(const TreeView& t, int s) {
  int lo = 0, hi = t.N - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.node_off[mid] <= s) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// hard_loss_kernel: ds (the per-slot gradient terms) lives in the row's ps
template <typename LD>
__global__ __launch_bounds__(kGlobalBlock) void global_hard_loss_kernel(TreeView t, GlobalRows g, const void* z, int64_t B,
                                                                        int64_t ldz, const int64_t* __restrict__ y,
                                                                        float eps, float w_x, float w_h, float scale,
                                                                        float* __restrict__ row_loss,
                                                                        float* __restrict__ gz) {
  __shared__ float red[64];
  const GRow r = global_row(t, g);
  float* ss = r.ss;
  float* ds = r.ps;
  const int tid = threadIdx.x;
  const bool smooth = eps != 0.f;
  for (int64_t sample = blockIdx.x; sample < B; sample += gridDim.x) {
    global_load<LD>(t, z, sample * ldz, r.zs);
    global_slot_sums<true>(t, r.zs, ss);
    for (int s = tid; s < t.R; s += kGlobalBlock) ds[s] = 0.f;
    __syncthreads();

    const int64_t yy = y[sample];
    const bool valid = yy >= 0 && yy < t.C;  // the same for every lane: a sample is the whole block's
    float tree_rows = 0.f;
    if (valid) {
      const int pb = t.cls_off[yy], pe = t.cls_off[yy + 1];
      for (int j = pb + tid; j < pe; j += kGlobalBlock) {
        const int s = t.cls_slot[j];
        const int n = global_node_of_slot(t, s);
        const int b = t.node_off[n], e = t.node_off[n + 1];
        if (e - b > kWideFan) continue;                        // below, by the whole block
        if (j > pb && t.cls_slot[j - 1] >= b) continue;        // same node, later child: not the first
        float m = ss[b];
        for (int q = b + 1; q < e; ++q) m = fmaxf(m, ss[q]);
        float sum = 0.f;
        for (int q = b; q < e; ++q) sum = sum + expf(ss[q] - m);
        if (smooth) {
          const float uni = eps / (float)(e - b);
          float sl = 0.f;
          for (int q = b; q < e; ++q) sl = sl + ss[q];
          tree_rows += ((logf(sum) + m) - (1.f - eps) * ss[s]) - uni * sl;
          for (int q = b; q < e; ++q)
            ds[q] = (expf(ss[q] - m) / sum - ((q == s ? 1.f - eps : 0.f) + uni)) * (w_h * scale) /
                    (float)(t.slot_off[q + 1] - t.slot_off[q]);
          continue;
        }
        tree_rows += (logf(sum) + m) - ss[s];
        for (int q = b; q < e; ++q)
          ds[q] = (expf(ss[q] - m) / sum - (q == s ? 1.f : 0.f)) * (w_h * scale) /
                  (float)(t.slot_off[q + 1] - t.slot_off[q]);
      }
      for (int w = 0; w < g.n_wide; ++w) {
        const int n = g.wide[w];
        const int b = t.node_off[n], e = t.node_off[n + 1];
        int lo = pb, hi = pe;  // the label's first slot at or behind b (its slots ascend)
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (t.cls_slot[mid] < b) lo = mid + 1; else hi = mid;
        }
        if (lo >= pe) continue;
        const int s = t.cls_slot[lo];
        if (s >= e) continue;  // the label is not under this node
        float m = -INFINITY;
        for (int q = b + tid; q < e; q += kGlobalBlock) m = fmaxf(m, ss[q]);
        m = group_max<kGlobalBlock>(m, red, tid);
        float sum = 0.f, sl = 0.f;
        for (int q = b + tid; q < e; q += kGlobalBlock) {
          sum += expf(ss[q] - m);
          sl += ss[q];
        }
        sum = group_sum<kGlobalBlock>(sum, red, tid);
        const float uni = eps / (float)(e - b);
        if (smooth) sl = group_sum<kGlobalBlock>(sl, red, tid);
        if (tid == 0)
          tree_rows += smooth ? ((logf(sum) + m) - (1.f - eps) * ss[s]) - uni * sl : (logf(sum) + m) - ss[s];
        for (int q = b + tid; q < e; q += kGlobalBlock) {
          const float hot = smooth ? ((q == s ? 1.f - eps : 0.f) + uni) : (q == s ? 1.f : 0.f);
          ds[q] = (expf(ss[q] - m) / sum - hot) * (w_h * scale) / (float)(t.slot_off[q + 1] - t.slot_off[q]);
        }
      }
    }
    tree_rows = group_sum<kGlobalBlock>(tree_rows, red, tid);

    float mz = -INFINITY;
    for (int c = tid; c < t.C; c += kGlobalBlock) mz = fmaxf(mz, r.zs[c]);
    mz = group_max<kGlobalBlock>(mz, red, tid);
    float sz = 0.f;
    for (int c = tid; c < t.C; c += kGlobalBlock) sz += expf(r.zs[c] - mz);
    sz = group_sum<kGlobalBlock>(sz, red, tid);
    float sumz = 0.f;
    if (smooth) {
      for (int c = tid; c < t.C; c += kGlobalBlock) sumz += r.zs[c];
      sumz = group_sum<kGlobalBlock>(sumz, red, tid);
    }
    const float uni = eps / (float)t.C;
    for (int c = tid; c < t.C; c += kGlobalBlock) {
      const float zc = r.zs[c];
      if (smooth) {
        if (c == yy) row_loss[sample] = w_x * (((logf(sz) + mz) - (1.f - eps) * zc) - uni * sumz) + w_h * tree_rows;
        r.gx[c] = (expf(zc - mz) / sz - ((c == yy ? 1.f - eps : 0.f) + uni)) * (w_x * scale);
        continue;
      }
      const float hot = (c == yy) ? 1.f : 0.f;
      if (c == yy) row_loss[sample] = w_x * ((logf(sz) + mz) - zc) + w_h * tree_rows;
      r.gx[c] = (expf(zc - mz) / sz - hot) * (w_x * scale);
    }
    if (!valid && tid == 0) row_loss[sample] = __uint_as_float(0x7fc00000u);  // loud: NaN loss
    __syncthreads();
    for (int c = tid; c < t.C; c += kGlobalBlock)
      gz[sample * t.C + c] = r.gx[c] + global_chain<ChainAdd>(t.cls_slot, t.cls_off[c], t.cls_off[c + 1], ds, 0.f);
    __syncthreads();
  }
}

// hard_fwd_kernel: every node decides in parallel, lane 0 walks.  A wide node's decision probability and entropy are
// folded by the whole block before the walk and wait in ps[b], ps[b + 1] (ps is otherwise unused here).
template <typename LD>
__global__ __launch_bounds__(kGlobalBlock) void global_hard_fwd_kernel(TreeView t, GlobalRows g, const void* z, int64_t B,
                                                                       int64_t ldz, int64_t* __restrict__ pred,
                                                                       float* __restrict__ onehot,
                                                                       int32_t* __restrict__ path_node,
                                                                       int32_t* __restrict__ path_child,
                                                                       float* __restrict__ path_prob,
                                                                       float* __restrict__ path_entropy) {
  __shared__ float red[64];
  __shared__ int res;
  const GRow r = global_row(t, g);
  float* ss = r.ss;
  float* ws = r.ps;
  int* best_of = (int*)r.pq;
  int* next_of = best_of + t.N;
  const int tid = threadIdx.x;
  const bool want = path_node != nullptr;
  for (int64_t sample = blockIdx.x; sample < B; sample += gridDim.x) {
    global_load<LD>(t, z, sample * ldz, r.zs);
    global_slot_sums<true>(t, r.zs, ss);
    for (int n = tid; n < t.N; n += kGlobalBlock) {
      const int b = t.node_off[n], e = t.node_off[n + 1];
      if (e - b > kWideFan) continue;
      int best = b;
      float bv = ss[b];
      for (int s = b + 1; s < e; ++s) {
        const float x = ss[s];
        if (x > bv) { bv = x; best = s; }  // first maximum wins (torch.max, model.py:113)
      }
      best_of[n] = best;
      next_of[n] = t.slot_next[best];
    }
    for (int w = 0; w < g.n_wide; ++w) {
      const int n = g.wide[w];
      const int b = t.node_off[n], e = t.node_off[n + 1];
      const int best = global_wide_argmax(ss, b, e, red);
      if (tid == 0) { best_of[n] = best; next_of[n] = t.slot_next[best]; }
      if (want) {
        const float eps = 1.1920928955078125e-07f;
        const float m = ss[best];
        float sum = 0.f;
        for (int s = b + tid; s < e; s += kGlobalBlock) sum += expf(ss[s] - m);
        sum = group_sum<kGlobalBlock>(sum, red, tid);
        float tot = 0.f;
        for (int s = b + tid; s < e; s += kGlobalBlock) tot += expf(ss[s] - m) / sum;
        tot = group_sum<kGlobalBlock>(tot, red, tid);
        float h = 0.f;
        for (int s = b + tid; s < e; s += kGlobalBlock) {
          const float p = (expf(ss[s] - m) / sum) / tot;
          h += p * logf(fminf(fmaxf(p, eps), 1.0f - eps));
        }
        h = group_sum<kGlobalBlock>(h, red, tid);
        if (tid == 0) { ws[b] = expf(ss[best] - m) / sum; ws[b + 1] = -h; }
      }
    }
    __syncthreads();
    if (tid == 0) {
      int n = t.root, cls = -1;
      int d = 0;
      for (; d < t.max_depth; ++d) {
        const int best = best_of[n];
        if (want) {
          const int b = t.node_off[n], e = t.node_off[n + 1];
          float prob, ent;
          if (e - b > kWideFan) {
            prob = ws[b];
            ent = ws[b + 1];
          } else {
            const float m = ss[best];
            float sum = 0.f;
            for (int s = b; s < e; ++s) sum = sum + expf(ss[s] - m);
            const float eps = 1.1920928955078125e-07f;
            float tot = 0.f;
            for (int s = b; s < e; ++s) tot = tot + expf(ss[s] - m) / sum;
            float h = 0.f;
            for (int s = b; s < e; ++s) {
              const float p = (expf(ss[s] - m) / sum) / tot;
              h = h + p * logf(fminf(fmaxf(p, eps), 1.0f - eps));
            }
            prob = expf(ss[best] - m) / sum;
            ent = -h;
          }
          const int64_t o = sample * t.max_depth + d;
          path_node[o] = n;
          path_child[o] = best - b;
          path_prob[o] = prob;
          path_entropy[o] = ent;
        }
        const int nx = next_of[n];
        if (nx >= 0) {
          n = nx;
        } else {
          cls = -nx - 1;
          ++d;
          break;
        }
      }
      if (want)
        for (; d < t.max_depth; ++d) {
          const int64_t o = sample * t.max_depth + d;
          path_node[o] = -1; path_child[o] = -1; path_prob[o] = 0.f; path_entropy[o] = 0.f;
        }
      pred[sample] = cls;
      res = cls;
    }
    __syncthreads();
    if (onehot != nullptr) {
      const int cls = res;
      for (int c = tid; c < t.C; c += kGlobalBlock) onehot[sample * t.C + c] = (c == cls) ? 1.f : 0.f;
    }
    __syncthreads();  // res and the row are rewritten by the next sample
  }
}

template <typename LD>
__global__ __launch_bounds__(kGlobalBlock) void global_node_outputs_kernel(TreeView t, GlobalRows g, const void* z, int64_t B,
                                                                           int64_t ldz, float* __restrict__ logits,
                                                                           float* __restrict__ probs,
                                                                           int64_t* __restrict__ preds,
                                                                           float* __restrict__ entropy) {
  __shared__ float red[64];
  const GRow r = global_row(t, g);
  float* ss = r.ss;
  float* ps = r.ps;
  const int tid = threadIdx.x;
  const bool want_probs = probs != nullptr || entropy != nullptr;
  for (int64_t sample = blockIdx.x; sample < B; sample += gridDim.x) {
    global_load<LD>(t, z, sample * ldz, r.zs);
    global_slot_sums<true>(t, r.zs, ss);
    if (want_probs) global_node_softmax(t, g, ss, ps, red);
    for (int s = tid; s < t.R; s += kGlobalBlock) {
      if (logits) logits[sample * t.R + s] = ss[s];
      if (probs) probs[sample * t.R + s] = ps[s];
    }
    for (int n = tid; n < t.N; n += kGlobalBlock) {
      const int b = t.node_off[n], e = t.node_off[n + 1];
      if (e - b > kWideFan) continue;
      if (preds) {
        int best = b;
        float bv = ss[b];
        for (int s = b + 1; s < e; ++s) {
          const float x = ss[s];
          if (x > bv) { bv = x; best = s; }
        }
        preds[sample * t.N + n] = best - b;
      }
      if (entropy) entropy[sample * t.N + n] = node_entropy(ps, b, e);
    }
    for (int w = 0; w < g.n_wide; ++w) {
      const int n = g.wide[w];
      const int b = t.node_off[n], e = t.node_off[n + 1];
      if (preds) {
        const int best = global_wide_argmax(ss, b, e, red);
        if (tid == 0) preds[sample * t.N + n] = best - b;
      }
      if (entropy) {
        const float h = global_wide_entropy(ps, b, e, red);
        if (tid == 0) entropy[sample * t.N + n] = h;
      }
    }
    __syncthreads();
  }
}
