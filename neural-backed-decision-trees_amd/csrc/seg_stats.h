// Segmentation evaluation (nbdt_seg_stats_accumulate), included at the end of rules.hip behind rules_pixel.h: the
// per-pixel twin of tree_stats_kernel on the layout of the pixel kernels.
//
// One lane owns one pixel, a wave owns 64 consecutive pixels of one image, a block is ONE wave.  pix_node_logits runs
// once into the [row][64] LDS rows; the hard walk reads the child logits there (pix_hard_fwd_kernel's rule), then
// pix_node_softmax overwrites them with the child probabilities and the soft path product runs over the packed
// class -> slots map in pix_soft_fwd_kernel's order (1.0f * p(node_1) * p(node_2) ...), keeping only the running maximum
// and its class: no probability goes to memory, and the soft argmax is argmax of what nbdt_seg_soft_forward writes, bit
// for bit.  The backbone's argmax is one more pass over the C planes (L2 hits).  The first maximum wins everywhere.
//
// Counters.  The grid is persistent (a block strides over the 64-pixel chunks), so that what a block counts can wait in
// its LDS -- [5N node counters][4 totals][max_depth + 1 first-error depths], ints behind the rows -- and reach the
// caller's int64 counters once, when the block is done, zeros skipped.  With one wave per block the totals need no
// atomics at all (lane 0 adds ballot counts); the node counters and the depth histogram take LDS atomics, because two
// lanes may sit on one node.  The confusion matrices are C * C int64 each and stay in global memory, but a wave does
// not pay one atomic per pixel: its 64 pixels are neighbours in an image row, so real label and prediction maps give
// it a handful of distinct (label, prediction) pairs, and wave_add_keys lets the first lane of every distinct key add
// the number of lanes that hold it.  Every sum is an integer sum: the counters do not depend on the order of the
// atomics, the size of the grid or the way a pass is cut into calls.
//
// The label's path comes from the class -> slots map in global memory (a lane reads its own label's list; the lists
// are ascending, which nbdt_tree_create checks, so the children of one node that hold the class are neighbours).
// Nothing per node is kept per pixel: the hard walk looks the node's argmax up in the label's list as it goes.
//
// Limit: the rows of the pixel form plus the block's counters within 160 KB of LDS (nbdt_seg_stats_fits).

constexpr int kSegStatsBlocksPerCU = 16;  // one-wave blocks per CU: what the kernel's 126-127 VGPRs keep resident (4 per SIMD); fewer where LDS admits fewer

struct SegStatsArgs {
  const int64_t* y;
  int64_t ignore;
  int64_t *totals, *conf_net, *conf_hard, *conf_soft, *node_counts, *first_error;
  int64_t *pred_net, *pred_hard, *pred_soft;
  int64_t total_chunks;  // N * g.chunks
  int rows;              // LDS rows in front of the counters (pix_rows)
};

// conf[key] += the number of lanes that hold `key`, for every distinct key among the lanes with `ok`: one add per
// distinct key of the wave.  The loop is uniform (it runs on ballot masks) and only counts; the first lane of every key
// then adds its count, all of them in ONE atomic instruction (a first version issued one single-lane atomic per key
// from inside the loop: 64 distinct keys cost 64 trips through the memory pipeline; DESIGN.md 28 has both timings).
__device__ __forceinline__ void wave_add_keys(int64_t* conf, bool ok, unsigned key, int lane) {
  unsigned long long live = __ballot(ok);
  int mine = 0;  // on the first lane of a key: the number of lanes that hold it
  while (live) {
    const int leader = __ffsll((long long)live) - 1;
    const unsigned k = (unsigned)__builtin_amdgcn_readlane((int)key, leader);
    const unsigned long long same = __ballot(ok && key == k);
    if (lane == leader) mine = __popcll(same);
    live &= ~same;
  }
  if (mine != 0) add_i64(conf + key, mine);
}

// first maximum of S[b..e)
__device__ __forceinline__ int pix_best_slot(const float* S, int b, int e) {
  int best = b;
  float top = S[b * kPixLanes];
  for (int s = b + 1; s < e; ++s) {
    const float v = S[s * kPixLanes];
    if (v > top) { top = v; best = s; }
  }
  return best;
}

template <typename LD>
__global__ __launch_bounds__(kPixLanes) void pix_stats_kernel(TreeView t, PixGeom g, const void* __restrict__ z,
                                                              SegStatsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x;
  float* S = lds + lane;
  int* cnt = (int*)(lds + (size_t)a.rows * kPixLanes);
  int* tot = cnt + 5 * t.N;
  int* fed = tot + 4;
  const int nsmall = stats_small_ints(t.N, t.max_depth);
  for (int i = lane; i < nsmall; i += kPixLanes) cnt[i] = 0;
  __syncthreads();
  const bool want_pred = a.pred_net != nullptr || a.pred_hard != nullptr || a.pred_soft != nullptr;
  const bool want_net = a.totals != nullptr || a.conf_net != nullptr || a.pred_net != nullptr;
  const bool want_soft = a.totals != nullptr || a.conf_soft != nullptr || a.pred_soft != nullptr;
  const bool want_path = a.node_counts != nullptr || a.first_error != nullptr;

  for (int64_t q = blockIdx.x; q < a.total_chunks; q += gridDim.x) {
    const int64_t img = q / g.chunks;
    const int64_t pix = (q - img * g.chunks) * kPixLanes + lane;
    const bool active = pix < g.HW;
    const int64_t pc = active ? pix : g.HW - 1;  // tail lanes read the last pixel
    const int64_t zbase = img * g.zi + pc;
    int64_t yy = -1;
    if (a.y != nullptr) yy = a.y[img * g.HW + pc];
    const bool valid = active && yy != a.ignore && yy >= 0 && yy < t.C;
    const unsigned long long vmask = __ballot(valid);
    if (vmask == 0 && !want_pred) continue;  // nothing to count in these 64 pixels

    pix_node_logits<LD>(t, g, z, zbase, lane, S);

    // the label's path: every child slot that holds the label, the children of one node side by side
    int pb = 0, pe = 0;
    if (valid && want_path) { pb = t.cls_off[yy]; pe = t.cls_off[yy + 1]; }
    if (a.node_counts != nullptr)
      for (int j = pb; j < pe;) {
        const int s = t.cls_slot[j];
        int n = s >> 1;
        if (!g.binary) {  // node owning slot s: last n with node_off[n] <= s
          int lo = 0, hi = t.N - 1;
          while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (t.node_off[mid] <= s) lo = mid; else hi = mid - 1;
          }
          n = lo;
        }
        const int b = t.node_off[n], e = t.node_off[n + 1];
        const int best = pix_best_slot(S, b, e);
        bool right = false;
        for (; j < pe; ++j) {
          const int s2 = t.cls_slot[j];
          if (s2 >= e) break;
          right = right || s2 == best;
        }
        lds_count(cnt + 5 * n);
        if (right) lds_count(cnt + 5 * n + 1);
      }

    // the hard walk (pix_hard_fwd_kernel); on the way, whether the node is on the label's path and sends it on
    int hard_cls = -1, first_err = t.max_depth;
    {
      int n = t.root;
      for (int d = 0; d < t.max_depth; ++d) {
        const int b = t.node_off[n], e = t.node_off[n + 1];
        const int best = pix_best_slot(S, b, e);
        if (valid && want_path) {
          int lo = pb, hi = pe;  // first slot of the label's list that is not in front of this node
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (t.cls_slot[mid] < b) lo = mid + 1; else hi = mid;
          }
          bool on_path = false, right = false;
          for (int j = lo; j < pe; ++j) {
            const int s2 = t.cls_slot[j];
            if (s2 >= e) break;
            on_path = true;
            right = right || s2 == best;
          }
          if (a.node_counts != nullptr) {
            lds_count(cnt + 5 * n + 2);
            if (on_path) lds_count(cnt + 5 * n + 3);
            if (right) lds_count(cnt + 5 * n + 4);
          }
          if (first_err == t.max_depth && !right) first_err = d;
        }
        const int nx = t.slot_next[best];
        if (nx < 0) { hard_cls = -nx - 1; break; }
        n = nx;
      }
    }

    // the backbone's own prediction: one pass over the C planes
    float vz = -INFINITY;
    int iz = 0x7fffffff;
    if (want_net)
      for (int c0 = 0; c0 < t.C; c0 += kPixU) {
        float x[kPixU];
#pragma unroll
        for (int u = 0; u < kPixU; ++u) x[u] = LD::at(z, zbase + (int64_t)min(c0 + u, t.C - 1) * g.zc);
#pragma unroll
        for (int u = 0; u < kPixU; ++u)
          if (c0 + u < t.C && x[u] > vz) { vz = x[u]; iz = c0 + u; }
      }

    // the soft rules: pix_soft_fwd_kernel's product, of which only the running maximum is kept
    float vp = -INFINITY;
    int ip = 0x7fffffff;
    if (want_soft) {
      pix_node_softmax(t, g, S);
      flat_chains<ChainMul>(
          g.pcls, t.L, 1.0f, lane, [&](int s) { return S[s * kPixLanes]; },
          [&](int c, float acc, int, unsigned) {
            if (acc > vp) { vp = acc; ip = c; }
          });
    }

    if (vmask != 0) {
      if (a.totals != nullptr) {
        const int n_net = __popcll(__ballot(valid && iz == yy)), n_hard = __popcll(__ballot(valid && hard_cls == yy)),
                  n_soft = __popcll(__ballot(valid && ip == yy));
        if (lane == 0) {
          tot[0] += __popcll(vmask);
          tot[1] += n_net;
          tot[2] += n_hard;
          tot[3] += n_soft;
        }
      }
      if (a.first_error != nullptr && valid) lds_count(fed + first_err);
      const unsigned row = (unsigned)yy * (unsigned)t.C;  // C < 65536 (pix_ok): label * C + prediction fits 32 bits
      if (a.conf_net != nullptr) wave_add_keys(a.conf_net, valid && iz >= 0 && iz < t.C, row + (unsigned)iz, lane);
      if (a.conf_hard != nullptr)
        wave_add_keys(a.conf_hard, valid && hard_cls >= 0 && hard_cls < t.C, row + (unsigned)hard_cls, lane);
      if (a.conf_soft != nullptr) wave_add_keys(a.conf_soft, valid && ip >= 0 && ip < t.C, row + (unsigned)ip, lane);
    }
    if (active) {
      const int64_t o = img * g.HW + pix;
      if (a.pred_net != nullptr) a.pred_net[o] = iz;
      if (a.pred_hard != nullptr) a.pred_hard[o] = hard_cls;
      if (a.pred_soft != nullptr) a.pred_soft[o] = ip;
    }
  }

  // one flush per block; untouched counters cost nothing
  __syncthreads();
  if (a.node_counts != nullptr)
    for (int i = lane; i < 5 * t.N; i += kPixLanes)
      if (cnt[i] != 0) add_i64(a.node_counts + i, cnt[i]);
  if (a.totals != nullptr && lane < 4 && tot[lane] != 0) add_i64(a.totals + lane, tot[lane]);
  if (a.first_error != nullptr)
    for (int i = lane; i <= t.max_depth; i += kPixLanes)
      if (fed[i] != 0) add_i64(a.first_error + i, fed[i]);
}

// ------------------------------------------------------------------------------------------
// host side

static size_t seg_stats_lds_bytes(const nbdt_tree* t) {
  return (size_t)pix_rows(t) * kPixLanes * sizeof(float) + (size_t)stats_small_ints(t->N, t->max_depth) * sizeof(int);
}

extern "C" int nbdt_seg_stats_fits(const nbdt_tree* t) {
  return nbdt_seg_pixel_fits(t) && seg_stats_lds_bytes(t) <= kLdsBytes;
}

// blocks of the persistent grid (process-wide; 0 = one per resident wave slot): lets a test make a block stride
static std::atomic<int> g_seg_stats_max_blocks{0};

extern "C" int nbdt_set_seg_stats_max_blocks(int blocks) {
  NBDT_REQUIRE(blocks >= 0, "the block cap must be 0 (automatic) or positive");
  g_seg_stats_max_blocks.store(blocks, std::memory_order_relaxed);
  return NBDT_OK;
}
extern "C" int nbdt_get_seg_stats_max_blocks(void) { return g_seg_stats_max_blocks.load(std::memory_order_relaxed); }

extern "C" int nbdt_seg_stats_accumulate(const nbdt_tree* t, const void* z, int ztype, int64_t N, int64_t HW, int64_t zi,
                                         int64_t zc, const int64_t* y, int64_t ignore_index,
                                         const nbdt_tree_stats* stats, int64_t* pred_net, int64_t* pred_hard,
                                         int64_t* pred_soft, void* stream) {
  SegStatsArgs a = {};
  if (stats) {
    NBDT_REQUIRE(stats->node_entropy == nullptr,
                 "node_entropy is not part of the segmentation statistics: leave it NULL");
    a.totals = stats->totals; a.conf_net = stats->confusion_net; a.conf_hard = stats->confusion_hard;
    a.conf_soft = stats->confusion_soft; a.node_counts = stats->node_counts; a.first_error = stats->first_error_depth;
  }
  const bool counted = a.totals || a.conf_net || a.conf_hard || a.conf_soft || a.node_counts || a.first_error;
  NBDT_REQUIRE(!counted || y != nullptr, "statistics against the labels need the labels");
  NBDT_REQUIRE(counted || pred_net || pred_hard || pred_soft, "nothing requested: every statistic and prediction is NULL");
  // (a block counts in 32-bit LDS counters, whatever the grid)
  NBDT_REQUIRE(N <= 0 || HW <= 0 || (HW < (1ll << 31) && N <= ((1ll << 31) - 1) / HW),
               "pixels: N * HW must stay below 2^31 (a block's counters are 32-bit integers)");
  PixGeom g;
  unsigned chunks = 0;
  int rc = pix_check(t, z, ztype, N, HW, zi, zc, &g, &chunks);
  if (rc) return rc;
  NBDT_REQUIRE(seg_stats_lds_bytes(t) <= kLdsBytes,
               "hierarchy beyond the segmentation statistics (the pixel rows plus the block's counters exceed 160 KB "
               "of LDS): run nbdt_tree_stats_accumulate on the coerced [N*H*W, C] tensor");
  if (N == 0) return NBDT_OK;
  a.y = y; a.ignore = ignore_index;
  a.pred_net = pred_net; a.pred_hard = pred_hard; a.pred_soft = pred_soft;
  a.total_chunks = (int64_t)chunks;
  a.rows = pix_rows(t);
  const size_t shmem = seg_stats_lds_bytes(t);
  const size_t per_cu = std::max<size_t>(1, std::min<size_t>(kSegStatsBlocksPerCU, kLdsBytes / shmem));
  int64_t blocks = (int64_t)per_cu * std::max(t->cus, 1);
  const int cap = g_seg_stats_max_blocks.load(std::memory_order_relaxed);
  if (cap > 0) blocks = std::min<int64_t>(blocks, cap);
  const unsigned grid = (unsigned)std::min<int64_t>(blocks, a.total_chunks);
  TreeView v = view_of(t);
  hipStream_t st = (hipStream_t)stream;
  int lrc;
  if (ztype == NBDT_F32) lrc = launch_rules(pix_stats_kernel<LoadF32>, grid, kPixLanes, shmem, st, v, g, z, a);
  else if (ztype == NBDT_BF16) lrc = launch_rules(pix_stats_kernel<LoadBF16>, grid, kPixLanes, shmem, st, v, g, z, a);
  else lrc = launch_rules(pix_stats_kernel<LoadF16>, grid, kPixLanes, shmem, st, v, g, z, a);
  if (lrc) return lrc;
  g_last_rules_path = 4;
  return NBDT_OK;
}
