// How long does ONE workgroup of 1024 lanes need to stream one row of an [n][n] fp64 matrix plus an int32 [n] array?
// The yardstick for a chain step of csrc/linkage.hip's chain_kernel (scratch/induced_linkage.py quotes it).  (gfx950)
//   hipcc --offload-arch=gfx950 -O3 -o row_stream_probe row_stream_probe.hip && ./row_stream_probe 21841
// The kernel reads `rows` rows, far apart, one after the other: four independent 8-byte loads and four 4-byte loads in
// flight per lane (the scan's shape), a running minimum so that nothing is dropped, and a workgroup barrier after every
// row, because in the chain the next row is known only when the scan of this one is done.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(e)                                                                   \
  do {                                                                             \
    hipError_t _e = (e);                                                           \
    if (_e != hipSuccess) {                                                        \
      fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(_e));                      \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

__global__ __launch_bounds__(1024) void stream_rows(const double* D, const int* size, int n, int rows, double* sink) {
  double best = __builtin_huge_val();
  for (int r = 0; r < rows; ++r) {
    const int x = (int)(((long long)r * 7919 + 13) % n);
    const double* row = D + (long long)x * n;
    for (int k0 = threadIdx.x; k0 < n; k0 += 4096) {
      double v[4];
      int s[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = k0 + u * 1024;
        s[u] = k < n ? size[k] : 0;
        v[u] = k < n ? row[k] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (s[u] > 0 && v[u] < best) best = v[u];
    }
    __syncthreads();
  }
  if (best < 0.0) sink[threadIdx.x] = best;      // never true: the matrix holds ones
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 21841;
  const int rows = argc > 2 ? atoi(argv[2]) : 4000;
  if (n < 2 || n > (1 << 20) || rows < 1) {
    fprintf(stderr, "usage: row_stream_probe n [rows]\n");
    return 2;
  }
  double *D, *sink;
  int* size;
  CHECK(hipMalloc(&D, (size_t)n * n * 8));
  CHECK(hipMalloc(&size, (size_t)n * 4));
  CHECK(hipMalloc(&sink, 1024 * 8));
  CHECK(hipMemset(D, 0x3f, (size_t)n * n * 8));          // 0x3f3f... is a positive finite double
  CHECK(hipMemset(size, 0x01, (size_t)n * 4));
  hipEvent_t t0, t1;
  CHECK(hipEventCreate(&t0));
  CHECK(hipEventCreate(&t1));
  float best_ms = 1e30f;
  for (int rep = 0; rep < 4; ++rep) {                     // the first repetition warms up
    CHECK(hipEventRecord(t0, 0));
    hipLaunchKernelGGL(stream_rows, dim3(1), dim3(1024), 0, 0, D, size, n, rows, sink);
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(t1, 0));
    CHECK(hipEventSynchronize(t1));
    float ms;
    CHECK(hipEventElapsedTime(&ms, t0, t1));
    if (rep > 0 && ms < best_ms) best_ms = ms;
  }
  const double us = 1e3 * best_ms / rows;
  printf("n %d rows %d row_bytes %lld us_per_row %.3f GBps %.1f\n", n, rows, 12LL * n, us, 12.0 * n / us / 1e3);
  CHECK(hipFree(D));
  CHECK(hipFree(size));
  CHECK(hipFree(sink));
  return 0;
}
