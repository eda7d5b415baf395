// Agglomerative clustering of the classifier's rows on gfx950: what nbdt.graph.build_induced_graph needs from
// scipy.cluster.hierarchy.linkage / sklearn's AgglomerativeClustering, in two launches.  All arithmetic is fp64.
//
//   A  pairwise_kernel   D[i][j] = metric(centers[i], centers[j]) for all pairs, the full symmetric [n][n] matrix with
//                        +inf on the diagonal.  One 64 x 64 tile of pairs per workgroup (upper triangle of tiles, each
//                        stores its transpose too), rows staged through LDS in chunks of 32 features, a 4 x 4 block of
//                        pairs per lane, one fp64 accumulator per pair, features summed in index order.
//   B  chain_kernel      the nearest-neighbour chain (Murtagh) in ONE workgroup of 1024 lanes: no grid barrier, nothing
//                        waits on another block.  The chain top x scans its row for the nearest active cluster; with a
//                        previous element p the minimum starts at D[x][p] and is replaced only by a strictly smaller
//                        value, so a reciprocal pair is found in finitely many steps whatever the ties.  A merge keeps
//                        the larger index, retires the smaller and rewrites row and column of the kept cluster by the
//                        Lance-Williams rule on distances.  size[], the chain and D live in the workspace, only the 16
//                        per-wave reduction slots are in LDS: n is bounded by memory, not by LDS.
//
// The minimum of a scan is the smallest value and among equal values the lowest index (lane loop ascending, then a
// butterfly over a total order), so two runs give the same bits.  The merges come out in chain order; the host sorts
// them by height (stable) and labels them (nbdt/graph.py).
// Built with -ffp-contract=off: the sums and the Lance-Williams formulas are the separate IEEE operations that
// tests/_linkage_ref.py restates in numpy.
#include "common.h"

#include <math.h>

namespace nbdt {
namespace {

constexpr int kTile = 64;            // pairs tile: kTile rows x kTile columns per workgroup
constexpr int kChunk = 32;           // features staged per trip
constexpr int kLd = kTile + 4;       // LDS row stride in floats (16-byte aligned rows)
constexpr int kLanes = 1024;         // launch B: one workgroup
constexpr int kWaves = kLanes / 64;
constexpr int kNone = 0x7fffffff;
constexpr int kScanUnroll = 4;       // independent loads in flight per lane (8, 16, 22 measured: no faster)

template <int METRIC>
__global__ __launch_bounds__(256) void pairwise_kernel(const float* __restrict__ c, int n, int d, double* __restrict__ D) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;                               // the transpose of tile (bj, bi) covers it
  __shared__ __attribute__((aligned(16))) float As[kChunk][kLd];
  __shared__ __attribute__((aligned(16))) float Bs[kChunk][kLd];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int row0 = bi * kTile, col0 = bj * kTile;
  double acc[4][4], na[4], nb[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    na[u] = 0.0;
    nb[u] = 0.0;
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
  }
  for (int k0 = 0; k0 < d; k0 += kChunk) {
    for (int e = tid; e < kTile * kChunk; e += 256) {    // rows past n and features past d are staged as zeros
      const int r = e / kChunk, kk = e % kChunk, k = k0 + kk;
      const int ga = row0 + r, gb = col0 + r;
      As[kk][r] = (ga < n && k < d) ? c[(long long)ga * d + k] : 0.f;
      Bs[kk][r] = (gb < n && k < d) ? c[(long long)gb * d + k] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < kChunk; ++kk) {
      const float4 a4 = *(const float4*)&As[kk][ti * 4];
      const float4 b4 = *(const float4*)&Bs[kk][tj * 4];
      const double a[4] = {(double)a4.x, (double)a4.y, (double)a4.z, (double)a4.w};
      const double b[4] = {(double)b4.x, (double)b4.y, (double)b4.z, (double)b4.w};
      if (METRIC == NBDT_METRIC_COSINE) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          na[u] += a[u] * a[u];
          nb[u] += b[u] * b[u];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          if (METRIC == NBDT_METRIC_EUCLIDEAN) {
            const double t = a[u] - b[v];
            acc[u][v] += t * t;
          } else if (METRIC == NBDT_METRIC_MANHATTAN) {
            acc[u][v] += fabs(a[u] - b[v]);
          } else {
            acc[u][v] += a[u] * b[v];
          }
        }
    }
    __syncthreads();
  }
  const double inf = __builtin_huge_val();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = row0 + ti * 4 + u;
    if (i >= n) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = col0 + tj * 4 + v;
      if (j >= n) continue;
      double r;
      if (METRIC == NBDT_METRIC_EUCLIDEAN) {
        r = sqrt(acc[u][v]);
      } else if (METRIC == NBDT_METRIC_MANHATTAN) {
        r = acc[u][v];
      } else {                                        // scipy's pdist: the cosine clipped to [-1, 1]
        double cs = acc[u][v] / (sqrt(na[u]) * sqrt(nb[v]));
        if (fabs(cs) > 1.0) cs = copysign(1.0, cs);
        r = 1.0 - cs;
      }
      if (i == j) r = inf;
      D[(long long)i * n + j] = r;
      if (bi != bj) D[(long long)j * n + i] = r;
    }
  }
}

// (ov, oi) comes before (bv, bi): a found entry before none, then the smaller value, then the lower index
__device__ __forceinline__ bool comes_first(double ov, int oi, double bv, int bi) {
  return oi != kNone && (bi == kNone || ov < bv || (ov == bv && oi < bi));
}

template <int METHOD>
__device__ __forceinline__ double lance_williams(double dak, double dbk, double dab, double na, double nb, double nk) {
  if (METHOD == NBDT_LINKAGE_WARD)
    return sqrt((((na + nk) * (dak * dak) + (nb + nk) * (dbk * dbk)) - nk * (dab * dab)) / ((na + nb) + nk));
  if (METHOD == NBDT_LINKAGE_COMPLETE) return dak > dbk ? dak : dbk;
  if (METHOD == NBDT_LINKAGE_SINGLE) return dak < dbk ? dak : dbk;
  return (na * dak + nb * dbk) / (na + nb);
}

template <int METHOD>
__global__ __launch_bounds__(kLanes) void chain_kernel(double* D, int* size, int* chain, int n, int* merges,
                                                      double* heights, int* sizes) {
  __shared__ double slot_v[2][kWaves];
  __shared__ int slot_i[2][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = tid; k < n; k += kLanes) size[k] = 1;
  __syncthreads();
  // everything below is uniform over the workgroup: every lane keeps the same chain state in registers
  int len = 0, merged = 0, lowest = 0, x = -1, p = -1;
  // a step pushes or pops two, and n - 1 merges end the loop: at most 3n steps.  The bound is what ends the loop
  // should a NaN ever break the order the argument rests on; unwritten merges then get size 0 (below).
  const int max_steps = 4 * n + 16;
  int step = 0;
  for (; merged < n - 1 && step < max_steps; ++step) {
    if (len == 0) {
      while (lowest < n - 1 && size[lowest] == 0) ++lowest;
      x = lowest;
      p = -1;
      len = 1;
      if (tid == 0) chain[0] = x;
    }
    const double* row = D + (long long)x * n;
    double bv = __builtin_huge_val();
    int bi = kNone;
    for (int k0 = tid; k0 < n; k0 += kLanes * kScanUnroll) {
      double v[kScanUnroll];
      int s[kScanUnroll];
#pragma unroll
      for (int u = 0; u < kScanUnroll; ++u) {
        const int k = k0 + u * kLanes;
        const bool in = k < n;
        s[u] = in ? size[k] : 0;
        v[u] = in ? row[k] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kScanUnroll; ++u) {
        const int k = k0 + u * kLanes;
        if (s[u] > 0 && k != x && (bi == kNone || v[u] < bv)) {
          bv = v[u];
          bi = k;
        }
      }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const double ov = __shfl_xor(bv, m, 64);
      const int oi = __shfl_xor(bi, m, 64);
      if (comes_first(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    const int par = step & 1;                  // two sets of slots: one barrier per step is enough
    if (lane == 0) {
      slot_v[par][wave] = bv;
      slot_i[par][wave] = bi;
    }
    __syncthreads();
    bv = slot_v[par][lane & (kWaves - 1)];
    bi = slot_i[par][lane & (kWaves - 1)];
#pragma unroll
    for (int m = 1; m < kWaves; m <<= 1) {
      const double ov = __shfl_xor(bv, m, 64);
      const int oi = __shfl_xor(bi, m, 64);
      if (comes_first(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    int y = bi;
    double dmin = bv;
    if (p >= 0) {
      const double dp = row[p];
      if (!(bv < dp)) {                               // the previous element keeps a tie
        y = p;
        dmin = dp;
      }
    }
    if (y == kNone) break;                            // no other active cluster: cannot happen while merged < n - 1
    if (y != p) {                                     // grow the chain
      if (len >= n) break;                            // chain elements are distinct active clusters: cannot happen
      if (tid == 0) chain[len] = y;
      ++len;
      p = x;
      x = y;
      continue;
    }
    // x and p are each other's nearest neighbours: merge them into the larger index
    const int a = x < y ? x : y, b = x < y ? y : x;
    const int sa = size[a], sb = size[b];
    const double* ra = D + (long long)a * n;
    double* rb = D + (long long)b * n;
    for (int k = tid; k < n; k += kLanes) {
      const int sk = size[k];
      if (sk > 0 && k != a && k != b) {
        const double nd = lance_williams<METHOD>(ra[k], rb[k], dmin, (double)sa, (double)sb, (double)sk);
        rb[k] = nd;
        D[(long long)k * n + b] = nd;
      }
    }
    __syncthreads();                                  // every lane has read size[a], size[b]
    if (tid == 0) {
      size[a] = 0;
      size[b] = sa + sb;
      merges[2 * merged] = a;
      merges[2 * merged + 1] = b;
      heights[merged] = dmin;
      sizes[merged] = sa + sb;
    }
    ++merged;
    len -= 2;
    if (len >= 1) x = chain[len - 1];
    p = len >= 2 ? chain[len - 2] : -1;
    __syncthreads();                                  // the new sizes, row and column before the next scan
  }
  for (int m = merged + tid; m < n - 1; m += kLanes) sizes[m] = 0;     // an unfinished run is visible to the host
  if (tid == 0) chain[0] = step;                                       // the chain is done with: steps taken, for profiles
}

constexpr int64_t kMaxN = 1 << 20, kMaxD = 1 << 24;

inline int64_t workspace_bytes_of(int64_t n) {
  const int64_t ints = ((2 * n * 4 + 255) / 256) * 256;       // size[n], chain[n]
  return n * n * 8 + ints;
}

}  // namespace
}  // namespace nbdt

extern "C" int nbdt_linkage_workspace_bytes(int64_t n, int64_t* bytes) {
  NBDT_REQUIRE(bytes, "null bytes pointer");
  NBDT_REQUIRE(n >= 2 && n <= nbdt::kMaxN, "linkage: n must be in [2, 2^20]");
  *bytes = nbdt::workspace_bytes_of(n);
  return NBDT_OK;
}

extern "C" int nbdt_linkage(const float* centers, int64_t n, int64_t d, int32_t method, int32_t metric, void* workspace,
                            int64_t workspace_bytes, int32_t* merges_out, double* heights_out, int32_t* sizes_out,
                            void* stream) {
  using namespace nbdt;
  NBDT_REQUIRE(centers && workspace && merges_out && heights_out && sizes_out, "linkage: null pointer");
  NBDT_REQUIRE(n >= 2 && n <= kMaxN, "linkage: n must be in [2, 2^20]");
  NBDT_REQUIRE(d >= 1 && d <= kMaxD, "linkage: d must be in [1, 2^24]");
  NBDT_REQUIRE(method >= NBDT_LINKAGE_WARD && method <= NBDT_LINKAGE_AVERAGE, "linkage: unknown linkage");
  NBDT_REQUIRE(metric >= NBDT_METRIC_EUCLIDEAN && metric <= NBDT_METRIC_COSINE, "linkage: unknown metric");
  NBDT_REQUIRE(method != NBDT_LINKAGE_WARD || metric == NBDT_METRIC_EUCLIDEAN, "linkage: ward takes the euclidean metric only");
  NBDT_REQUIRE(workspace_bytes >= workspace_bytes_of(n), "linkage: workspace too small (nbdt_linkage_workspace_bytes)");
  NBDT_REQUIRE(((uintptr_t)workspace % 8) == 0 && ((uintptr_t)heights_out % 8) == 0 && ((uintptr_t)centers % 4) == 0 &&
                   ((uintptr_t)merges_out % 4) == 0 && ((uintptr_t)sizes_out % 4) == 0,
               "linkage: misaligned pointer");
  double* D = (double*)workspace;
  int* size = (int*)(D + n * n);
  int* chain = size + n;
  const int tiles = (int)((n + kTile - 1) / kTile);
  const dim3 grid((unsigned)tiles, (unsigned)tiles);
  hipStream_t s = (hipStream_t)stream;
  const int ni = (int)n, di = (int)d;
  switch (metric) {
    case NBDT_METRIC_EUCLIDEAN:
      hipLaunchKernelGGL(pairwise_kernel<NBDT_METRIC_EUCLIDEAN>, grid, dim3(256), 0, s, centers, ni, di, D);
      break;
    case NBDT_METRIC_MANHATTAN:
      hipLaunchKernelGGL(pairwise_kernel<NBDT_METRIC_MANHATTAN>, grid, dim3(256), 0, s, centers, ni, di, D);
      break;
    default:
      hipLaunchKernelGGL(pairwise_kernel<NBDT_METRIC_COSINE>, grid, dim3(256), 0, s, centers, ni, di, D);
  }
  NBDT_LAUNCH_CHECK();
  switch (method) {
    case NBDT_LINKAGE_WARD:
      hipLaunchKernelGGL(chain_kernel<NBDT_LINKAGE_WARD>, dim3(1), dim3(kLanes), 0, s, D, size, chain, ni, merges_out,
                         heights_out, sizes_out);
      break;
    case NBDT_LINKAGE_COMPLETE:
      hipLaunchKernelGGL(chain_kernel<NBDT_LINKAGE_COMPLETE>, dim3(1), dim3(kLanes), 0, s, D, size, chain, ni, merges_out,
                         heights_out, sizes_out);
      break;
    case NBDT_LINKAGE_SINGLE:
      hipLaunchKernelGGL(chain_kernel<NBDT_LINKAGE_SINGLE>, dim3(1), dim3(kLanes), 0, s, D, size, chain, ni, merges_out,
                         heights_out, sizes_out);
      break;
    default:
      hipLaunchKernelGGL(chain_kernel<NBDT_LINKAGE_AVERAGE>, dim3(1), dim3(kLanes), 0, s, D, size, chain, ni, merges_out,
                         heights_out, sizes_out);
  }
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}
