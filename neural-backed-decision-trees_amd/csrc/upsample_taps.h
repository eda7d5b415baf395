// The bilinear interpolation contract of upsampled_xent.hip: torch's (ATen UpSample.h, area_pixel_compute_scale /
// area_pixel_compute_source_index / compute_source_index_and_lambda), restated in fp32 for one axis with `in` source
// and `out` destination samples.  ONE definition for every kernel and for the host entries nbdt_upsample_taps /
// nbdt_upsample_footprint, so the forward, the backward and the tests cannot drift apart.  Compiled with
// -ffp-contract=off: every multiply and add below is a single rounding.
//   align_corners = 0:  scale = (float)in / (float)out;                    src = max(scale * (dst + 0.5f) - 0.5f, 0)
//   align_corners = 1:  scale = out > 1 ? (float)(in - 1) / (out - 1) : 0; src = scale * dst
//   taps:  i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1
//   value: ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)
// The scale is worked out ONCE on the host (up_scale) and handed to the kernels, so host and device divide nowhere twice.
#pragma once

namespace nbdt {

struct UpTap {
  int i0, i1;
  float l0, l1;
};

inline float up_scale(int in, int out, int align_corners) {
  if (align_corners) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  return (float)in / (float)out;
}

__host__ __device__ __forceinline__ UpTap up_taps(int in, float scale, int align_corners, int dst) {
  float src;
  if (align_corners) {
    src = scale * (float)dst;
  } else {
    src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
  }
  UpTap t;
  t.i0 = (int)src;
  if (t.i0 > in - 1) t.i0 = in - 1;  // never taken within the entries' extent limit; keeps every address in bounds beyond it
  t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
  t.l1 = src - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

__host__ __device__ __forceinline__ float up_lerp(float ly0, float ly1, float lx0, float lx1, float a, float b, float c,
                                                  float d) {
  return ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d);
}

// what destination `dst` takes from source index i: the clamped borders (i0 == i1) add up by construction
__host__ __device__ __forceinline__ float up_weight(const UpTap& t, int i) {
  return (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f);
}

// [lo, hi]: every destination that takes a nonzero weight from source index i.  Its taps name i when i - 1 <= i0(dst) <= i;
// src, and with it i0, never decreases with dst (a product with a positive constant and a sum are monotone in fp32 too),
// so those destinations are a range; a closed-form guess is walked to its ends with up_taps itself, which makes the range
// exact for the arithmetic above whatever the rounding of the guess.  Never short; an inner destination of weight 0 stays.
__host__ __device__ __forceinline__ void up_footprint(int in, int out, float scale, int align_corners, int i, int* lo,
                                                      int* hi) {
  if (!(scale > 0.f)) {  // in == 1 with align_corners: every destination reads source 0
    *lo = 0;
    *hi = out - 1;
    return;
  }
  const float off = align_corners ? 0.f : 0.5f;
  const float last = (float)(out - 1);
  float a = ((float)(i - 1) + off) / scale - off, b = ((float)(i + 1) + off) / scale - off;
  int l = (int)(a < 0.f ? 0.f : (a > last ? last : a));
  int h = (int)(b < 0.f ? 0.f : (b > last ? last : b));
  while (l > 0 && up_taps(in, scale, align_corners, l - 1).i0 >= i - 1) --l;
  while (l < out - 1 && up_taps(in, scale, align_corners, l).i0 < i - 1) ++l;
  while (h < out - 1 && up_taps(in, scale, align_corners, h + 1).i0 <= i) ++h;
  while (h > 0 && up_taps(in, scale, align_corners, h).i0 > i) --h;
  // a tap that names i with weight exactly 0 (l1 == 0 at an end of the range) contributes nothing: leave it out
  while (l < h && up_weight(up_taps(in, scale, align_corners, l), i) == 0.f) ++l;
  while (h > l && up_weight(up_taps(in, scale, align_corners, h), i) == 0.f) --h;
  *lo = l;
  *hi = h;
}

}  // namespace nbdt
