// The memory-bound half of the AdaIN style pass (the reference's utils/style_transform.py over
// tools/net.py: a VGG-19 encoder to relu4_1, adaptive instance normalisation, a mirrored decoder);
// its 3x3 convs are msl_dconv_fwd.  One image per call, [C][H][W] fp32.
//
// The padded grid.  The reference pads every 3x3 conv by reflection (ReflectionPad2d(1)); msl_dconv_fwd is
// a "same" conv with zero padding.  So a stage's input is materialised WITH its reflected border, as
// [C][H+2][W+2], and the conv runs over that whole grid: an interior output (rows 1..H, columns 1..W)
// reads the grid's own cells only, i.e. the reflected image; a border output also reads the conv's zero
// padding, is finite, and is never read.  Every kernel here reads either a plain [C][H][W] tensor or the
// interior of such a grid (x_grid = 1: row pitch W+2, plane (H+2)(W+2), first cell one row and one column
// in), and the ones that feed a conv write a whole grid.
//
// Access width: one dword per lane.  A grid row starts (W+2)*4*row + 4 bytes into its plane, so neither
// the interior of a row nor, for odd W, the row itself is 8- or 16-byte aligned, and the reflected border
// cells break any wider pattern at both ends; consecutive lanes take consecutive cells of a row (256 B
// per wave instruction, fully coalesced).
//
// No FMA contraction in this file: the outputs are compared bit for bit with torch's own fp32 sequences
// (mul, then add, each rounded); the few fused operations are written as fmaf.
#include "msl_internal.h"

#pragma clang fp contract(off)

namespace msl {

constexpr int kStyleThreads = 256;
constexpr int kStatsBatch = 8;                                      // values a thread reduces in registers at a time
constexpr int kStatsIters = 4;                                      // batches per thread
constexpr int kStatsChunk = kStyleThreads * kStatsBatch * kStatsIters;  // pixels of a channel per block (8192)

// torch's ReLU (clamp_min(0)): a negative becomes +0, -0.0 and NaN pass
__device__ __forceinline__ float relu_t(float v) { return v < 0.f ? 0.f : v; }

// reflect-by-one of a grid coordinate g in [0, n+1] onto [0, n): 0 -> 1, n+1 -> n-2
__device__ __forceinline__ int reflect1(int g, int n) { return g == 0 ? 1 : (g == n + 1 ? n - 2 : g - 1); }

struct StyleSrc {
  const float* x;   // first interior cell of channel 0
  int pitch;        // floats between rows
  long long plane;  // floats between channels
};

static inline StyleSrc style_src(const float* x, int x_grid, int h, int w) {
  if (x_grid) return {x + (w + 2) + 1, w + 2, (long long)(h + 2) * (w + 2)};
  return {x, w, (long long)h * w};
}

// y[cpad][ho+2][wo+2] = reflect_pad1(resample(act(a_c * x + b_c))), one thread per cell of y
template <int RESAMPLE>  // 0 none, 1 2x2 stride-2 ceil-mode max-pool, 2 nearest x2
__global__ void __launch_bounds__(kStyleThreads) k_style_pad(StyleSrc s, int c, int h, int w, int ho, int wo, int act,
                                                             const float* __restrict__ a, const float* __restrict__ b,
                                                             float* __restrict__ y, int total) {
  const int i = blockIdx.x * kStyleThreads + threadIdx.x;
  if (i >= total) return;
  const int gw = wo + 2, gh = ho + 2;
  const int col = i % gw, t = i / gw;
  const int row = t % gh, ch = t / gh;
  if (ch >= c) {  // the channels a caller pads cin with
    y[i] = 0.f;
    return;
  }
  const int oy = reflect1(row, ho), ox = reflect1(col, wo);
  const float* p = s.x + ch * s.plane;
  const bool affine = a != nullptr;
  const float ac = affine ? a[ch] : 1.f, bc = affine ? b[ch] : 0.f;
  auto f = [&](float v) {
    if (act == 2) v = relu_t(v);
    if (affine) v = v * ac + bc;
    if (act == 1) v = relu_t(v);
    return v;
  };
  float r;
  if (RESAMPLE == 0) {
    r = f(p[(long long)oy * s.pitch + ox]);
  } else if (RESAMPLE == 2) {
    r = f(p[(long long)(oy >> 1) * s.pitch + (ox >> 1)]);
  } else {
    // torch's max-pool scan: row-major over the window clipped to the input, the first of equals stays
    r = -INFINITY;
    const int y1 = min(2 * oy + 2, h), x1 = min(2 * ox + 2, w);
    for (int yy = 2 * oy; yy < y1; ++yy)
      for (int xx = 2 * ox; xx < x1; ++xx) {
        const float v = f(p[(long long)yy * s.pitch + xx]);
        if (v > r || v != v) r = v;
      }
  }
  y[i] = r;
}

// y[cpad][h+2][w+2] = reflect_pad1(W1 * (img / 255 or img) + b1): the encoder's leading 1x1 conv 3 -> 3 as a
// per-pixel affine; img is uint8 HWC RGB (torchvision's ToTensor: a true division by 255) or float [3][H][W]
__global__ void __launch_bounds__(kStyleThreads) k_style_input(const uint8_t* __restrict__ u8,
                                                               const float* __restrict__ f32, int h, int w,
                                                               const float* __restrict__ w1,
                                                               const float* __restrict__ b1, float* __restrict__ y,
                                                               int cpad, int plane_total) {
  const int i = blockIdx.x * kStyleThreads + threadIdx.x;
  if (i >= plane_total) return;
  const int gw = w + 2;
  const int col = i % gw, row = i / gw;
  const int sy = reflect1(row, h), sx = reflect1(col, w);
  const long long px = (long long)sy * w + sx;
  float v[3];
  if (u8) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = __fdiv_rn((float)u8[px * 3 + k], 255.f);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = f32[(long long)k * h * w + px];
  }
#pragma unroll
  for (int o = 0; o < 3; ++o)
    y[(long long)o * plane_total + i] = fmaf(w1[3 * o + 2], v[2], fmaf(w1[3 * o + 1], v[1], fmaf(w1[3 * o], v[0], b1[o])));
  for (int o = 3; o < cpad; ++o) y[(long long)o * plane_total + i] = 0.f;
}

// torch's `nearest` source index (F.interpolate's default mode): min((int)floorf(dst * scale), n - 1) with
// scale = (float)in / (float)out formed by the host; one fp32 multiply, rounded, then the floor (no FMA:
// contraction is off in this file).  Not dst * in / out in integers: 24 -> 74 and 56 -> 46 differ.
__device__ __forceinline__ int nearest_t(int dst, float scale, int n) {
  const int s = (int)floorf((float)dst * scale);
  return s < n - 1 ? s : n - 1;
}

struct Window {
  int x0, y0, cw, ch;  // the window of the source image
  float sx, sy;        // cw / w and ch / h
};

// k_style_input reading a window of the image magnified to h x w by torch's nearest rule: the reference's
// F.interpolate(crop, size) ahead of the style network (cropTrans, rectification), never materialised.
// iw is the image's row length, ihw its plane.
__global__ void __launch_bounds__(kStyleThreads) k_style_input_window(const uint8_t* __restrict__ u8,
                                                                      const float* __restrict__ f32, int iw,
                                                                      long long ihw, Window win, int h, int w,
                                                                      const float* __restrict__ w1,
                                                                      const float* __restrict__ b1,
                                                                      float* __restrict__ y, int cpad,
                                                                      int plane_total) {
  const int i = blockIdx.x * kStyleThreads + threadIdx.x;
  if (i >= plane_total) return;
  const int gw = w + 2;
  const int col = i % gw, row = i / gw;
  const int sy = win.y0 + nearest_t(reflect1(row, h), win.sy, win.ch);
  const int sx = win.x0 + nearest_t(reflect1(col, w), win.sx, win.cw);
  const long long px = (long long)sy * iw + sx;
  float v[3];
  if (u8) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = __fdiv_rn((float)u8[px * 3 + k], 255.f);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = f32[k * ihw + px];
  }
#pragma unroll
  for (int o = 0; o < 3; ++o)
    y[(long long)o * plane_total + i] = fmaf(w1[3 * o + 2], v[2], fmaf(w1[3 * o + 1], v[1], fmaf(w1[3 * o], v[0], b1[o])));
  for (int o = 3; o < cpad; ++o) y[(long long)o * plane_total + i] = 0.f;
}

// ------------------------------------------------------------------------------------------ statistics
// (count, mean, M2 = sum of squared deviations from that mean) of a set of values; two sets merge by Chan
// et al.'s update, which never forms a difference of large sums: a channel with mean 1000 and spread 0.01
// keeps its variance.  The merge order is fixed by the indices alone (no atomics): the result is
// deterministic.
struct Moments {
  float n, mean, m2;
};

__device__ __forceinline__ Moments merge(Moments p, Moments q) {
  if (q.n == 0.f) return p;
  if (p.n == 0.f) return q;
  const float n = p.n + q.n;
  const float d = q.mean - p.mean;
  const float f = __fdiv_rn(q.n, n);
  Moments r;
  r.n = n;
  r.mean = p.mean + d * f;
  r.m2 = p.m2 + q.m2 + (d * d) * (p.n * f);
  return r;
}

__device__ __forceinline__ Moments shfl_down_m(Moments m, int o) {
  return {__shfl_down(m.n, o, 64), __shfl_down(m.mean, o, 64), __shfl_down(m.m2, o, 64)};
}

// lane 0 of the wave gets the merge of its 64 lanes
__device__ __forceinline__ Moments wave_merge(Moments m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = merge(m, shfl_down_m(m, o));
  return m;
}

// thread 0 of the block gets the merge of every thread's moments (waves through LDS, in wave order)
template <int THREADS>
__device__ __forceinline__ Moments block_merge(Moments m) {
  __shared__ Moments part[THREADS / 64];
  m = wave_merge(m);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = part[0];
#pragma unroll
    for (int k = 1; k < THREADS / 64; ++k) m = merge(m, part[k]);
  }
  return m;
}

__device__ __forceinline__ void stats_store(Moments m, float pivot, float* stats, int c, int ch) {
  stats[ch] = pivot + m.mean;
  stats[c + ch] = __fdiv_rn(m.m2, m.n - 1.f);  // torch's unbiased variance
}

// The values are reduced as differences from the channel's pivot, its first pixel (the same in every block):
// the moments of v - pivot are the moments of v with the mean moved, and a channel whose spread is small
// beside its mean (1000 +- 0.01) is reduced at the precision of the spread, not of the mean.
__device__ __forceinline__ float stats_pivot(const float* p, int relu) { return relu ? relu_t(p[0]) : p[0]; }

// stage 1: block (chunk, channel) reduces kStatsChunk pixels: each thread takes kStatsBatch lane-strided
// values at a time, reduces them in registers in two passes (their mean, then the deviations from it and
// their squares: the corrected two-pass sum, which cancels the rounding of that mean) and merges the batch
// into its running moments.  One chunk per channel: the result itself.
__global__ void __launch_bounds__(kStyleThreads) k_style_stats(StyleSrc s, int c, int w, int hw, int relu,
                                                               float* __restrict__ stats,
                                                               Moments* __restrict__ partial, int nchunk) {
  const int ch = blockIdx.y;
  const float* p = s.x + ch * s.plane;
  const float pivot = stats_pivot(p, relu);
  const int base = blockIdx.x * kStatsChunk;
  Moments acc = {0.f, 0.f, 0.f};
  for (int it = 0; it < kStatsIters; ++it) {
    float v[kStatsBatch];
    int k = 0;
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < kStatsBatch; ++j) {
      const int px = base + (it * kStatsBatch + j) * kStyleThreads + threadIdx.x;
      v[j] = 0.f;
      if (px < hw) {
        const int row = px / w, col = px - row * w;
        const float t = p[(long long)row * s.pitch + col];
        v[j] = (relu ? relu_t(t) : t) - pivot;
        sum += v[j];
        ++k;
      }
    }
    if (k == 0) break;  // the pixels of later batches lie further on
    const float n = (float)k, m0 = __fdiv_rn(sum, n);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < kStatsBatch; ++j) {
      const float d = v[j] - m0;
      if (j < k) {  // a thread's valid values are its first k
        s1 += d;
        s2 += d * d;
      }
    }
    const float corr = __fdiv_rn(s1, n);
    acc = merge(acc, Moments{n, m0 + corr, fmaxf(s2 - s1 * corr, 0.f)});
  }
  acc = block_merge<kStyleThreads>(acc);
  if (threadIdx.x == 0) {
    if (nchunk == 1)
      stats_store(acc, pivot, stats, c, ch);
    else
      partial[(long long)ch * nchunk + blockIdx.x] = acc;
  }
}

// stage 2 (channels of more than one chunk): one wave per channel merges the chunks' moments
__global__ void __launch_bounds__(64) k_style_stats_merge(StyleSrc s, int relu, const Moments* __restrict__ partial,
                                                          int nchunk, int c, float* __restrict__ stats) {
  const int ch = blockIdx.x;
  Moments acc = {0.f, 0.f, 0.f};
  for (int k = threadIdx.x; k < nchunk; k += 64) acc = merge(acc, partial[(long long)ch * nchunk + k]);
  acc = wave_merge(acc);
  if (threadIdx.x == 0) stats_store(acc, stats_pivot(s.x + ch * s.plane, relu), stats, c, ch);
}

// ------------------------------------------------------------------------------------------ AdaIN
constexpr int kStyleMaxStyles = 16;
struct StyleWeights {
  float w[kStyleMaxStyles];
};

// a = alpha * (sum_i w_i ss_i) / sc + (1 - alpha),  b = alpha * (sum_i w_i ms_i - mc * (sum_i w_i ss_i) / sc),
// s = sqrt(var + eps): alpha * t + (1 - alpha) of the reference with the per-channel scalars folded.
// alpha = 0: a = 0 * ratio + 1 = 1 and b = 0 * (...) = 0 exactly (ratio is finite: sc >= sqrt(eps) > 0).
__global__ void __launch_bounds__(64) k_style_adain_coef(const float* __restrict__ cs, const float* __restrict__ ss,
                                                         StyleWeights wt, int nstyle, int c, float alpha, float eps,
                                                         float* __restrict__ a, float* __restrict__ b) {
  const int ch = blockIdx.x * 64 + threadIdx.x;
  if (ch >= c) return;
  const float mc = cs[ch], sc = __fsqrt_rn(cs[c + ch] + eps);
  float sstd = 0.f, smean = 0.f;
  for (int i = 0; i < nstyle; ++i) {
    const float* st = ss + (long long)i * 2 * c;
    sstd += wt.w[i] * __fsqrt_rn(st[c + ch] + eps);
    smean += wt.w[i] * st[ch];
  }
  const float ratio = __fdiv_rn(sstd, sc);
  a[ch] = alpha * ratio + (1.f - alpha);
  // a zero offset is stored as -0.0, the identity of IEEE addition: v + -0.0 is v for every v, -0.0 included
  const float off = alpha * (smean - mc * ratio);
  b[ch] = off == 0.f ? -0.f : off;
}

// ------------------------------------------------------------------------------------------ output
// q = clamp(x * 255 + 0.5, 0, 255) as torch computes it (mul, add, clamp_min, clamp_max, each on its own);
// rgb[h][w][3] = uint8(q) (torchvision's save_image), seg[3][h][w] = q of B, G, R minus the channel's mean
// (the reference's Trainer.seg_transform), either or both
__global__ void __launch_bounds__(kStyleThreads) k_style_output(StyleSrc s, int w, int hw, uint8_t* __restrict__ rgb,
                                                                float* __restrict__ seg, float mean_b, float mean_g,
                                                                float mean_r) {
  const int px = blockIdx.x * kStyleThreads + threadIdx.x;
  if (px >= hw) return;
  const int row = px / w, col = px - row * w;
  float q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float v = s.x[k * s.plane + (long long)row * s.pitch + col] * 255.f;
    v = v + 0.5f;
    v = v < 0.f ? 0.f : v;
    q[k] = v > 255.f ? 255.f : v;
  }
  if (rgb) {
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[(long long)px * 3 + k] = (uint8_t)q[k];
  }
  if (seg) {
    seg[px] = q[2] - mean_b;
    seg[(long long)hw + px] = q[1] - mean_g;
    seg[2ll * hw + px] = q[0] - mean_r;
  }
}

// One axis of k_style_output_resampled: a destination coordinate d (absolute, inside the window) to a row
// or column of the decoder's map.
//   one map  (full == 0): l = d - d0, the window's own coordinate, over `mid` cells;
//   two maps (full  > 0): l = nearest(d: full -> dest) - off, the cell of the stitched map of `full` cells
//                         this image holds `mid` of, from `off` on; outside [0, mid) the pixel is another
//                         image's and is left alone;
// then nearest(l: n -> mid), n the decoder map's size.
struct AxisMap {
  int d0, mid, full, off, n;
  float s_in, s_out;  // n / mid, full / dest
};

__device__ __forceinline__ int axis_src(const AxisMap& a, int d) {
  const int l = a.full ? nearest_t(d, a.s_out, a.full) - a.off : d - a.d0;
  if (l < 0 || l >= a.mid) return -1;
  return nearest_t(l, a.s_in, a.n);
}

// k_style_output's seg output gathered through torch's nearest maps into the window (ax.d0, ay.d0, dw, dh)
// of seg[3][hd][wd]: the quantisation is pointwise, so it commutes with the gather and the values are
// those of interpolate -> mul, add, clamp -> minus mean -> B, G, R.
__global__ void __launch_bounds__(kStyleThreads) k_style_output_resampled(StyleSrc s, AxisMap ay, AxisMap ax, int dw,
                                                                          int npx, float* __restrict__ seg, int wd,
                                                                          long long dplane, float mean_b,
                                                                          float mean_g, float mean_r) {
  const int i = blockIdx.x * kStyleThreads + threadIdx.x;
  if (i >= npx) return;
  const int r = i / dw, c = i - r * dw;
  const int dy = ay.d0 + r, dx = ax.d0 + c;
  const int sy = axis_src(ay, dy), sx = axis_src(ax, dx);
  if (sy < 0 || sx < 0) return;
  float q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float v = s.x[k * s.plane + (long long)sy * s.pitch + sx] * 255.f;
    v = v + 0.5f;
    v = v < 0.f ? 0.f : v;
    q[k] = v > 255.f ? 255.f : v;
  }
  const long long o = (long long)dy * wd + dx;
  seg[o] = q[2] - mean_b;
  seg[dplane + o] = q[1] - mean_g;
  seg[2 * dplane + o] = q[0] - mean_r;
}

// out[ho][wo] = in[nearest][nearest]: F.interpolate of the reference's float label map, on the int64 map
__global__ void __launch_bounds__(kStyleThreads) k_label_resize_nearest(const long long* __restrict__ in, int h, int w,
                                                                        long long* __restrict__ out, int wo, int npx,
                                                                        float sy, float sx) {
  const int i = blockIdx.x * kStyleThreads + threadIdx.x;
  if (i >= npx) return;
  const int r = i / wo, c = i - r * wo;
  out[i] = in[(long long)nearest_t(r, sy, h) * w + nearest_t(c, sx, w)];
}

// every index a kernel forms from these counts stays below 2^31
static inline bool fits_i32(long long v) { return v > 0 && v <= 0x7fffffffLL; }

// torch's scale of a nearest map from `in` to `out` cells: compute_scales_value<float>
static inline float nearest_scale(int in, int out) { return (float)in / (float)out; }

}  // namespace msl

using namespace msl;

extern "C" {

int msl_style_max_styles(void) { return kStyleMaxStyles; }

int msl_style_pad(const float* x, int x_grid, int c, int h, int w, int act, int resample, const float* a,
                  const float* b, float* y, int cpad, msl_stream_t stream) {
  if (!x || !y || c < 1 || cpad < c || (unsigned)act > 2u || (unsigned)resample > 2u || (unsigned)x_grid > 1u ||
      (a == nullptr) != (b == nullptr))
    return MSL_ERR_ARG;
  if (h < 1 || w < 1) return MSL_ERR_ARG;
  const long long ho = resample == 1 ? (h + 1LL) / 2 : (resample == 2 ? 2LL * h : h);
  const long long wo = resample == 1 ? (w + 1LL) / 2 : (resample == 2 ? 2LL * w : w);
  if (h < 2 || w < 2 || ho < 2 || wo < 2) return MSL_ERR_SHAPE;  // reflection needs two rows and two columns
  const long long total = (long long)cpad * (ho + 2) * (wo + 2);
  if (!fits_i32(total) || !fits_i32((long long)c * (h + 2LL) * (w + 2LL))) return MSL_ERR_ARG;
  const StyleSrc s = style_src(x, x_grid, h, w);
  const dim3 grid((unsigned)cdiv(total, kStyleThreads)), block(kStyleThreads);
  if (resample == 0)
    MSL_LAUNCH(k_style_pad<0>, grid, block, 0, as_stream(stream), s, c, h, w, (int)ho, (int)wo, act, a, b, y, (int)total);
  else if (resample == 1)
    MSL_LAUNCH(k_style_pad<1>, grid, block, 0, as_stream(stream), s, c, h, w, (int)ho, (int)wo, act, a, b, y, (int)total);
  else
    MSL_LAUNCH(k_style_pad<2>, grid, block, 0, as_stream(stream), s, c, h, w, (int)ho, (int)wo, act, a, b, y, (int)total);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_style_input(const uint8_t* rgb_u8, const float* chw_f32, int h, int w, const float* w1, const float* b1,
                    float* y, int cpad, msl_stream_t stream) {
  if ((rgb_u8 == nullptr) == (chw_f32 == nullptr) || !w1 || !b1 || !y || cpad < 3 || h < 1 || w < 1)
    return MSL_ERR_ARG;
  if (h < 2 || w < 2) return MSL_ERR_SHAPE;
  const long long plane = (h + 2LL) * (w + 2LL);
  if (!fits_i32(plane * cpad)) return MSL_ERR_ARG;
  MSL_LAUNCH(k_style_input, dim3((unsigned)cdiv(plane, kStyleThreads)), dim3(kStyleThreads), 0, as_stream(stream),
             rgb_u8, chw_f32, h, w, w1, b1, y, cpad, (int)plane);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_style_input_window(const uint8_t* rgb_u8, const float* chw_f32, int ih, int iw, int x0, int y0, int cw,
                           int ch, int h, int w, const float* w1, const float* b1, float* y, int cpad,
                           msl_stream_t stream) {
  if ((rgb_u8 == nullptr) == (chw_f32 == nullptr) || !w1 || !b1 || !y || cpad < 3 || h < 1 || w < 1 || ih < 1 ||
      iw < 1 || x0 < 0 || y0 < 0 || cw < 1 || ch < 1 || (long long)x0 + cw > iw || (long long)y0 + ch > ih)
    return MSL_ERR_ARG;
  if (h < 2 || w < 2) return MSL_ERR_SHAPE;
  const long long plane = (h + 2LL) * (w + 2LL);
  if (!fits_i32(plane * cpad) || !fits_i32(3LL * ih * iw)) return MSL_ERR_ARG;
  const Window win = {x0, y0, cw, ch, nearest_scale(cw, w), nearest_scale(ch, h)};
  MSL_LAUNCH(k_style_input_window, dim3((unsigned)cdiv(plane, kStyleThreads)), dim3(kStyleThreads), 0,
             as_stream(stream), rgb_u8, chw_f32, iw, (long long)ih * iw, win, h, w, w1, b1, y, cpad, (int)plane);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

size_t msl_style_stats_workspace(int c, int h, int w) {
  if (c < 1 || h < 1 || w < 1) return 0;
  const long long nchunk = ((long long)h * w + kStatsChunk - 1) / kStatsChunk;
  return nchunk > 1 ? (size_t)c * (size_t)nchunk * sizeof(Moments) : 0;
}

int msl_style_stats(const float* x, int x_grid, int c, int h, int w, int relu, float* stats, void* ws,
                    size_t ws_bytes, msl_stream_t stream) {
  if (!x || !stats || c < 1 || h < 1 || w < 1 || (unsigned)x_grid > 1u || (unsigned)relu > 1u) return MSL_ERR_ARG;
  const long long hw = (long long)h * w;
  if (hw < 2) return MSL_ERR_SHAPE;  // torch's unbiased variance of one value is NaN
  if (!fits_i32((long long)c * (h + 2LL) * (w + 2LL)) || c > 65535) return MSL_ERR_ARG;
  const int nchunk = cdiv(hw, kStatsChunk);
  const size_t need = msl_style_stats_workspace(c, h, w);
  if (need && (!ws || ws_bytes < need)) return MSL_ERR_WORKSPACE;
  Moments* partial = reinterpret_cast<Moments*>(ws);
  const StyleSrc s = style_src(x, x_grid, h, w);
  MSL_LAUNCH(k_style_stats, dim3((unsigned)nchunk, (unsigned)c), dim3(kStyleThreads), 0, as_stream(stream), s, c, w,
             (int)hw, relu, stats, partial, nchunk);
  MSL_CHECK_LAUNCH();
  if (nchunk > 1) {
    MSL_LAUNCH(k_style_stats_merge, dim3((unsigned)c), dim3(64), 0, as_stream(stream), s, relu,
               (const Moments*)partial, nchunk, c, stats);
    MSL_CHECK_LAUNCH();
  }
  return MSL_OK;
}

int msl_style_adain_coef(const float* content_stats, const float* style_stats, const float* weights, int nstyle,
                         int c, float alpha, float eps, float* a, float* b, msl_stream_t stream) {
  if (!content_stats || !style_stats || !weights || !a || !b || c < 1 || nstyle < 1 || nstyle > kStyleMaxStyles ||
      !(alpha >= 0.f && alpha <= 1.f) || !(eps >= 0.f))
    return MSL_ERR_ARG;
  StyleWeights wt = {};
  for (int i = 0; i < nstyle; ++i) wt.w[i] = weights[i];
  MSL_LAUNCH(k_style_adain_coef, dim3((unsigned)cdiv(c, 64)), dim3(64), 0, as_stream(stream), content_stats,
             style_stats, wt, nstyle, c, alpha, eps, a, b);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_style_output(const float* x, int x_grid, int h, int w, uint8_t* rgb_u8, float* seg_bgr, float mean_b,
                     float mean_g, float mean_r, msl_stream_t stream) {
  if (!x || (!rgb_u8 && !seg_bgr) || h < 1 || w < 1 || (unsigned)x_grid > 1u) return MSL_ERR_ARG;
  const long long hw = (long long)h * w;
  if (!fits_i32(3 * (h + 2LL) * (w + 2LL))) return MSL_ERR_ARG;
  MSL_LAUNCH(k_style_output, dim3((unsigned)cdiv(hw, kStyleThreads)), dim3(kStyleThreads), 0, as_stream(stream),
             style_src(x, x_grid, h, w), w, (int)hw, rgb_u8, seg_bgr, mean_b, mean_g, mean_r);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_style_output_resampled(const float* x, int x_grid, int h, int w, int mid_h, int mid_w, int full_h, int full_w,
                               int off_y, int off_x, float* seg_bgr, int hd, int wd, int dx0, int dy0, int dw, int dh,
                               float mean_b, float mean_g, float mean_r, msl_stream_t stream) {
  if (!x || !seg_bgr || h < 1 || w < 1 || (unsigned)x_grid > 1u || mid_h < 1 || mid_w < 1 || hd < 1 || wd < 1 ||
      dx0 < 0 || dy0 < 0 || dw < 1 || dh < 1 || (long long)dx0 + dw > wd || (long long)dy0 + dh > hd)
    return MSL_ERR_ARG;
  const bool two = full_h != 0 || full_w != 0;
  if (two) {
    if (full_h < 1 || full_w < 1 || off_y < 0 || off_x < 0 || (long long)off_y + mid_h > full_h ||
        (long long)off_x + mid_w > full_w)
      return MSL_ERR_ARG;
  } else if (mid_h != dh || mid_w != dw || off_y != 0 || off_x != 0) {
    return MSL_ERR_ARG;
  }
  if (!fits_i32(3 * (h + 2LL) * (w + 2LL)) || !fits_i32(3LL * hd * wd)) return MSL_ERR_ARG;
  const AxisMap ay = {dy0, mid_h, full_h, off_y, h, nearest_scale(h, mid_h), two ? nearest_scale(full_h, hd) : 0.f};
  const AxisMap ax = {dx0, mid_w, full_w, off_x, w, nearest_scale(w, mid_w), two ? nearest_scale(full_w, wd) : 0.f};
  const long long npx = (long long)dw * dh;
  MSL_LAUNCH(k_style_output_resampled, dim3((unsigned)cdiv(npx, kStyleThreads)), dim3(kStyleThreads), 0,
             as_stream(stream), style_src(x, x_grid, h, w), ay, ax, dw, (int)npx, seg_bgr, wd, (long long)hd * wd,
             mean_b, mean_g, mean_r);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_label_resize_nearest(const long long* label, int h, int w, long long* out, int ho, int wo,
                             msl_stream_t stream) {
  if (!label || !out || h < 1 || w < 1 || ho < 1 || wo < 1) return MSL_ERR_ARG;
  const long long npx = (long long)ho * wo;
  if (!fits_i32(npx) || !fits_i32((long long)h * w)) return MSL_ERR_ARG;
  MSL_LAUNCH(k_label_resize_nearest, dim3((unsigned)cdiv(npx, kStyleThreads)), dim3(kStyleThreads), 0,
             as_stream(stream), label, h, w, out, wo, (int)npx, nearest_scale(h, ho), nearest_scale(w, wo));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

}  // extern "C"
