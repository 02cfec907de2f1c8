// What loss.hip (the training losses) and predict.hip (the evaluator's prediction kernels) both build on:
// the geometry of an align_corners upsample, torch-CPU's bilinear taps, the softmax and first-max argmax of
// one pixel, and the host's geometry check and class-count dispatch.  Internal to csrc/.
#pragma once
#include <math.h>
#include <cmath>

#include "msl_internal.h"

// No FMA contraction in a file that includes this: torch-CPU rounds s*o before subtracting floor(s*o), and
// the bilinear taps are exact fma(x0, w0, x1*w1) patterns written out explicitly below.
#pragma clang fp contract(off)

namespace msl {

constexpr int kMaxC = 32;

struct Geo {
  int C, Hi, Wi, Ho, Wo;
  float sh, sw;  // align_corners scales (in-1)/(out-1) in fp32, as torch computes them
};

struct Lin {
  int i0, i1;
  float w0, w1;
};

// area_pixel_compute_source_index + guard_index_and_lambda (align_corners=True)
__device__ __forceinline__ Lin lin(int o, float s, int n) {
  const float real = s * (float)o;
  int i0 = (int)floorf(real);
  i0 = min(i0, n - 1);
  const float lam = fminf(fmaxf(real - (float)i0, 0.f), 1.f);
  Lin r;
  r.i0 = i0;
  r.i1 = i0 + (i0 < n - 1 ? 1 : 0);
  r.w0 = 1.f - lam;
  r.w1 = lam;
  return r;
}

__device__ __forceinline__ float bilerp(const float* __restrict__ plane, int Wi, const Lin& ly,
                                        const Lin& lx) {
  const float* r0 = plane + ly.i0 * Wi;
  const float* r1 = plane + ly.i1 * Wi;
  const float t0 = __fmaf_rn(r0[lx.i0], lx.w0, __fmul_rn(r0[lx.i1], lx.w1));
  const float t1 = __fmaf_rn(r1[lx.i0], lx.w0, __fmul_rn(r1[lx.i1], lx.w1));
  return __fmaf_rn(t0, ly.w0, __fmul_rn(t1, ly.w1));
}

template <int CM>
__device__ __forceinline__ void up_logits(const float* __restrict__ L, const Geo& g, const Lin& ly,
                                          const Lin& lx, float (&v)[CM]) {
  const int hw = g.Hi * g.Wi;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < g.C) v[c] = bilerp(L + c * hw, g.Wi, ly, lx);
}

// softmax over C (max, exp(x - max), sequential sum, divide) + first-max argmax of p
template <int CM>
__device__ __forceinline__ void softmax(const float (&v)[CM], int C, float (&p)[CM], float& mx,
                                        float& sum) {
  mx = v[0];
#pragma unroll
  for (int c = 1; c < CM; ++c)
    if (c < C) mx = fmaxf(mx, v[c]);
  sum = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) {
      p[c] = expf(v[c] - mx);
      sum += p[c];
    }
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) p[c] = p[c] / sum;
}

template <int CM>
__device__ __forceinline__ int argmax_first(const float (&p)[CM], int C, float& best) {
  best = p[0];
  int a = 0;
#pragma unroll
  for (int c = 1; c < CM; ++c)
    if (c < C && p[c] > best) {
      best = p[c];
      a = c;
    }
  return a;
}

// ---------------------------------------------------------------- host helpers
static bool geo_ok(int c, int hi, int wi, int ho, int wo) {
  return c >= 1 && c <= kMaxC && hi >= 1 && wi >= 1 && ho >= 1 && wo >= 1 &&
         (long long)ho * wo < (1LL << 31);
}

static Geo make_geo(int c, int hi, int wi, int ho, int wo) {
  Geo g;
  g.C = c;
  g.Hi = hi;
  g.Wi = wi;
  g.Ho = ho;
  g.Wo = wo;
  g.sh = ho > 1 ? (float)(hi - 1) / (float)(ho - 1) : 0.f;
  g.sw = wo > 1 ? (float)(wi - 1) / (float)(wo - 1) : 0.f;
  return g;
}

#define MSL_DISPATCH_C(C, CM, ...)      \
  do {                                  \
    if ((C) == 19) {                    \
      constexpr int CM = 19;            \
      __VA_ARGS__;                      \
    } else if ((C) == 16) {             \
      constexpr int CM = 16;            \
      __VA_ARGS__;                      \
    } else if ((C) == 13) {             \
      constexpr int CM = 13;            \
      __VA_ARGS__;                      \
    } else {                            \
      constexpr int CM = kMaxC;         \
      __VA_ARGS__;                      \
    }                                   \
  } while (0)

}  // namespace msl
