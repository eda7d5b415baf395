// MixUp / CutMix of a training batch on the device (torchvision.transforms.v2.MixUp / CutMix; the soft-label transforms
// the reference's ImageNet example applies under Classy Vision), with the probability targets that go with it, in ONE
// launch: nbdt_mix_batch (include/nbdt_hip.h).
//
// Pure data movement: per output element two 4-byte reads (the sample and its partner, the batch rolled by one) and one
// 4-byte write, so the launch is bound by 3 * B*3*H*W*4 bytes of HBM traffic.  A lane handles four consecutive x of one
// row with 16-byte loads and one 16-byte store when W % 4 == 0 and the pointers allow, single elements otherwise.  The
// [B, C] target rows are written by the same grid after its image share.  No atomics, no LDS.
//
// Built with -ffp-contract=off (nbdt/_build.py): x*lam + x_partner*one_minus_lam is two IEEE multiplies and one add, the
// bits of torch's x.mul(lam).add(x.roll(1, 0).mul(one_minus_lam)); the target rows likewise.
#include "common.h"

#include <algorithm>

using namespace nbdt;

namespace {

struct MixBox {
  int y1, y2, x1, x2;
};

// V = 4: items are float4 groups (W % 4 == 0, so a group never crosses a row); V = 1: single elements.
// blend = 0 (lam == 1 and one_minus_lam == 0: CutMix, or a MixUp draw of exactly 1): outside the box the sample is copied,
// not formed as x*1 + partner*0 -- the same bits for a finite partner; an inf / NaN partner pixel leaves x, where the
// product form would give NaN.
template <int V>
__global__ __launch_bounds__(256) void mix_kernel(const float* __restrict__ x, const long long* __restrict__ y, int B,
                                                  int H, int W, float lam, float oml, int blend, MixBox box, float lam_t,
                                                  float oml_t, float* __restrict__ out, float* __restrict__ tgt, int C) {
  const int G = W / V;                               // items per row
  const long long per_img = 3ll * H * G;             // items per image
  const long long items = (long long)B * per_img;
  const long long stride = (long long)gridDim.x * 256;
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < items; it += stride) {
    const long long b = it / per_img;
    const long long r = it - b * per_img;            // item within the image
    const int row = (int)(r / G), g = (int)(r - (long long)row * G);
    const int yy = row % H, x0 = g * V;
    const long long pb = b == 0 ? B - 1 : b - 1;     // roll(1, 0): out[b] pairs x[b] with x[b - 1]
    const bool yin = yy >= box.y1 && yy < box.y2;
    const long long off = r * V;
    const float* xs = x + b * per_img * V + off;
    const float* xp = x + pb * per_img * V + off;
    float* o = out + b * per_img * V + off;
    if (V == 4) {
      const float4 a = *(const float4*)xs, p = *(const float4*)xp;
      const float av[4] = {a.x, a.y, a.z, a.w}, pv[4] = {p.x, p.y, p.z, p.w};
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = yin && x0 + k >= box.x1 && x0 + k < box.x2;
        const float m = blend ? av[k] * lam + pv[k] * oml : av[k];
        v[k] = in ? pv[k] : m;
      }
      *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      const float a = *xs, p = *xp;
      const bool in = yin && x0 >= box.x1 && x0 < box.x2;
      const float m = blend ? a * lam + p * oml : a;
      *o = in ? p : m;
    }
  }
  // target rows: onehot(y_b)*lam_t + onehot(y_partner)*oml_t.  The labels are only compared, never used as an index; a
  // row built from a label outside [0, C) is all NaN (the loss kernels then report a NaN loss).
  const long long telems = (long long)B * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < telems; i += stride) {
    const long long b = i / C;
    const int c = (int)(i - b * C);
    const long long ya = y[b], yp = y[b == 0 ? B - 1 : b - 1];
    const bool valid = ya >= 0 && ya < C && yp >= 0 && yp < C;
    const float ha = (c == ya) ? 1.f : 0.f, hp = (c == yp) ? 1.f : 0.f;
    tgt[i] = valid ? ha * lam_t + hp * oml_t : __uint_as_float(0x7fc00000u);
  }
}

}  // namespace

extern "C" int nbdt_mix_batch(const float* x, const int64_t* y, int32_t B, int32_t H, int32_t W, float lam,
                              float one_minus_lam, int32_t y1, int32_t y2, int32_t x1, int32_t x2, float lam_t,
                              float one_minus_lam_t, float* out, float* tgt, int32_t C, void* stream) {
  NBDT_REQUIRE(x && y && out && tgt, "null argument");
  NBDT_REQUIRE(B > 0, "empty batch");
  NBDT_REQUIRE(H > 0 && W > 0 && H <= 4096 && W <= 4096, "image sides must be 1..4096");
  NBDT_REQUIRE(C > 0, "no classes");
  NBDT_REQUIRE(0 <= y1 && y1 <= y2 && y2 <= H && 0 <= x1 && x1 <= x2 && x2 <= W, "the box must lie inside the image");
  const size_t n = (size_t)B * 3 * H * W;
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
  NBDT_REQUIRE(oa + n * sizeof(float) <= xa || xa + n * sizeof(float) <= oa,
               "out must not overlap x: a sample is read again as its neighbour's partner");
  const uintptr_t ta = (uintptr_t)tgt;
  const size_t tbytes = (size_t)B * C * sizeof(float);
  NBDT_REQUIRE((ta + tbytes <= xa || xa + n * sizeof(float) <= ta) && (ta + tbytes <= oa || oa + n * sizeof(float) <= ta),
               "tgt must not overlap x or out");
  const bool empty = y1 == y2 || x1 == x2;
  NBDT_REQUIRE(empty || (lam == 1.f && one_minus_lam == 0.f), "a box (CutMix) goes with lam = 1, one_minus_lam = 0");
  const int blend = !(lam == 1.f && one_minus_lam == 0.f);
  const MixBox box = {y1, y2, x1, x2};
  const bool vec = W % 4 == 0 && xa % 16 == 0 && oa % 16 == 0;
  const size_t items = vec ? n / 4 : n;
  const size_t work = items > (size_t)B * C ? items : (size_t)B * C;
  // four items per lane: enough blocks to fill the device on a CIFAR batch, few enough to keep the index arithmetic off the
  // critical path on an ImageNet one
  const unsigned grid = (unsigned)std::min<size_t>((work + 1023) / 1024, (size_t)1 << 20);   // the loops stride over the rest
  const long long* yl = (const long long*)y;
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(mix_kernel<4>, dim3(grid), dim3(256), 0, s, x, yl, B, H, W, lam, one_minus_lam, blend, box, lam_t,
                       one_minus_lam_t, out, tgt, C);
  else
    hipLaunchKernelGGL(mix_kernel<1>, dim3(grid), dim3(256), 0, s, x, yl, B, H, W, lam, one_minus_lam, blend, box, lam_t,
                       one_minus_lam_t, out, tgt, C);
  NBDT_LAUNCH_CHECK();
  return NBDT_OK;
}
