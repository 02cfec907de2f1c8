// Pillow-exact image resampling on the device (HBM-bound byte work): what the reference loaders do
// between the decoded PNG and _img_transform / _mask_transform, on the host, in Pillow
//   img.transpose(FLIP_LEFT_RIGHT); img.crop(...); img.resize(size, Image.BICUBIC)
//   mask.transpose(...);            mask.crop(...); mask.resize(size, Image.NEAREST)
//                                              datasets/cityscapes_Dataset.py:173-243
// Pillow's 8-bit resampling is integer arithmetic on tables computed once per (in, out) size on the
// host (utils/resample.py builds them): per output index a first tap, a tap count and 22-bit fixed
// point coefficients.  One pass over an axis is
//     out = clamp((2^21 + sum_k pixel[first + k] * coeff[k]) >> 22, 0, 255)      (int32, arithmetic shift)
// and a resize is the horizontal pass into a uint8 image followed by the vertical pass on that; an
// axis whose size does not change gets no pass.  The same sums here, so every byte equals Pillow's.
// The last pass can write BGR - mean fp32 planes directly (preprocess.hip's __fsub_rn form), so on
// the training path the resized uint8 image never reaches memory.
//
// Mirror and crop are addressing only: the crop (x0, y0, cw, ch) is in the coordinates of the
// mirrored image, crop column x is source column  mirror ? sw - 1 - (x0 + x) : x0 + x.
#include "msl_internal.h"

namespace msl {

constexpr int kBits = 22;           // Pillow's PRECISION_BITS for 8-bit images
constexpr int kRound = 1 << (kBits - 1);
constexpr int kTile = 256;          // output pixels of one block of the horizontal pass
constexpr int kMaxTaps = 64;
constexpr int kMaxDim = 65535;

__device__ __forceinline__ int clamp8(int acc) { return min(max(acc >> kBits, 0), 255); }

// the three bytes of one output pixel -> the requested outputs (uint8 HWC and / or fp32 BGR - mean planes)
__device__ __forceinline__ void put_pixel(int r, int g, int b, int y, int x, int ow, long long plane,
                                          uint8_t* __restrict__ out_u8, float* __restrict__ out_f32, float mb,
                                          float mg, float mr) {
  const long long p = (long long)y * ow + x;
  if (out_u8) {
    uint8_t* o = out_u8 + p * 3;
    o[0] = (uint8_t)r;
    o[1] = (uint8_t)g;
    o[2] = (uint8_t)b;
  }
  if (out_f32) {
    out_f32[p] = __fsub_rn((float)b, mb);
    out_f32[plane + p] = __fsub_rn((float)g, mg);
    out_f32[2 * plane + p] = __fsub_rn((float)r, mr);
  }
}

// Horizontal pass.  Block (bx, y) = kTile consecutive output pixels of crop row y.  The source bytes
// those outputs read - one contiguous run of the source row, [lo, hi) in crop columns - are staged in
// LDS with aligned dword loads; each thread then sums its taps from LDS.  `tab` is [2 + ks][ow]: row 0
// the first tap, row 1 the tap count, rows 2.. the coefficients, so a wave's table loads are contiguous.
// first / taps are clamped to the crop and to the staged run, so a table that disagrees with the bounds
// the host validated still cannot read outside the source row.
__global__ void __launch_bounds__(kTile) k_resize_h(const uint8_t* __restrict__ src, int sw, int x0, int y0, int cw,
                                                    int mirror, const int32_t* __restrict__ tab, int ks, int ow,
                                                    int oh, int span_cap, uint8_t* __restrict__ out_u8,
                                                    float* __restrict__ out_f32, float mb, float mg, float mr) {
  extern __shared__ uint32_t seg[];
  __shared__ int s_lo, s_hi;
  const int y = blockIdx.y;
  const int x = blockIdx.x * kTile + threadIdx.x;
  if (threadIdx.x == 0) {
    s_lo = cw;
    s_hi = 0;
  }
  __syncthreads();
  int first = 0, taps = 0;
  const int32_t* col = tab + x;  // this output's column of the table
  if (x < ow) {
    first = min(max(col[0], 0), cw);
    taps = min(max(col[ow], 0), min(ks, cw - first));
  }
  // the block's run: a reduction per wave, then one LDS atomic per wave
  int lo_w = taps > 0 ? first : cw, hi_w = taps > 0 ? first + taps : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo_w = min(lo_w, __shfl_xor(lo_w, o, 64));
    hi_w = max(hi_w, __shfl_xor(hi_w, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&s_lo, lo_w);
    atomicMax(&s_hi, hi_w);
  }
  __syncthreads();
  const int lo = s_lo;
  const int hi = min(s_hi, lo + span_cap);
  if (hi > lo) {
    // source columns of crop columns [lo, hi): ascending in memory either way
    const int c0 = mirror ? sw - (x0 + hi) : x0 + lo;
    const uint8_t* p = src + ((long long)(y0 + y) * sw + c0) * 3;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const int off = (int)(a & 3);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a - off);
    const int nd = (off + (hi - lo) * 3 + 3) >> 2;
    for (int i = threadIdx.x; i < nd; i += kTile) seg[i] = q[i];
    __syncthreads();
    if (x < ow) {
      const uint8_t* sb = reinterpret_cast<const uint8_t*>(seg) + off;
      const int n = min(taps, hi - first);
      int r = kRound, g = kRound, b = kRound;
      for (int k = 0; k < n; ++k) {
        const int c = first + k;
        const uint8_t* px = sb + (mirror ? hi - 1 - c : c - lo) * 3;
        const int w = col[(long long)(2 + k) * ow];
        r += px[0] * w;
        g += px[1] * w;
        b += px[2] * w;
      }
      put_pixel(clamp8(r), clamp8(g), clamp8(b), y, x, ow, (long long)oh * ow, out_u8, out_f32, mb, mg, mr);
    }
  } else if (x < ow) {
    put_pixel(0, 0, 0, y, x, ow, (long long)oh * ow, out_u8, out_f32, mb, mg, mr);
  }
}

// Vertical pass (TAB) or plain crop + mirror copy (!TAB): thread = one output pixel of output row
// blockIdx.y, coalesced along x; the row's taps are uniform over the block (scalar loads; `tab` is
// [2 + ks][oh], as in k_resize_h).  `in_h` is the number of rows the table may address from row y0 on.
template <bool TAB>
__global__ void __launch_bounds__(256) k_resize_v(const uint8_t* __restrict__ src, int sw, int x0, int y0, int in_h,
                                                  int mirror, const int32_t* __restrict__ tab, int ks, int ow, int oh,
                                                  uint8_t* __restrict__ out_u8, float* __restrict__ out_f32, float mb,
                                                  float mg, float mr) {
  const int y = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= ow) return;
  const int col = mirror ? sw - 1 - (x0 + x) : x0 + x;
  int r, g, b;
  if (TAB) {
    const int32_t* row = tab + y;  // this output row's column of the table
    const int first = min(max(row[0], 0), in_h);
    const int taps = min(max(row[oh], 0), min(ks, in_h - first));
    const uint8_t* p = src + ((long long)(y0 + first) * sw + col) * 3;
    r = g = b = kRound;
    for (int k = 0; k < taps; ++k, p += (long long)sw * 3) {
      const int w = row[(long long)(2 + k) * oh];
      r += p[0] * w;
      g += p[1] * w;
      b += p[2] * w;
    }
    r = clamp8(r);
    g = clamp8(g);
    b = clamp8(b);
  } else {
    const uint8_t* p = src + ((long long)(y0 + y) * sw + col) * 3;
    r = p[0];
    g = p[1];
    b = p[2];
  }
  put_pixel(r, g, b, y, x, ow, (long long)oh * ow, out_u8, out_f32, mb, mg, mr);
}

// NEAREST on an id map: a gather through the two index tables (NULL = identity), the trainId table in
// LDS.  Indices are clamped to the crop.
__global__ void __launch_bounds__(256) k_resize_nearest(const uint8_t* __restrict__ ids, int sw, int x0, int y0,
                                                        int cw, int ch, int mirror, const int32_t* __restrict__ xtab,
                                                        const int32_t* __restrict__ ytab, int ow,
                                                        const int32_t* __restrict__ lut, uint8_t* __restrict__ out_u8,
                                                        int64_t* __restrict__ out_i64) {
  __shared__ int32_t t[256];
  if (out_i64) t[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const int y = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= ow) return;
  const int sx = xtab ? min(max(xtab[x], 0), cw - 1) : x;
  const int sy = ytab ? min(max(ytab[y], 0), ch - 1) : y;
  const int col = mirror ? sw - 1 - (x0 + sx) : x0 + sx;
  const uint8_t id = ids[(long long)(y0 + sy) * sw + col];
  const long long p = (long long)y * ow + x;
  if (out_u8) out_u8[p] = id;
  if (out_i64) out_i64[p] = t[id];
}

// host check of a table's (first, taps) pairs against the axis they address; the widest run of source
// columns one kTile-wide block of outputs reads goes to *span (the horizontal pass's LDS size)
static bool bounds_ok(const int32_t* b, int n_out, int ks, int in_size, int* span) {
  int widest = 0;
  for (int t0 = 0; t0 < n_out; t0 += kTile) {
    int lo = in_size, hi = 0;
    for (int i = t0; i < std::min(n_out, t0 + kTile); ++i) {
      const long long first = b[2 * i], taps = b[2 * i + 1];
      if (first < 0 || taps < 0 || taps > ks || first + taps > in_size) return false;
      if (taps > 0) {
        lo = std::min<int>(lo, (int)first);
        hi = std::max<int>(hi, (int)(first + taps));
      }
    }
    widest = std::max(widest, hi - lo);
  }
  *span = widest;
  return true;
}

static bool crop_ok(int sh, int sw, int x0, int y0, int cw, int ch, int ow, int oh) {
  return sh >= 1 && sw >= 1 && sh <= kMaxDim && sw <= kMaxDim && x0 >= 0 && y0 >= 0 && cw >= 1 && ch >= 1 &&
         (long long)x0 + cw <= sw && (long long)y0 + ch <= sh && ow >= 1 && oh >= 1 && ow <= kMaxDim && oh <= kMaxDim;
}

}  // namespace msl

using namespace msl;

extern "C" {

size_t msl_resize_workspace(int ch, int ow) {
  if (ch < 1 || ow < 1) return 0;
  return (size_t)ch * (size_t)ow * 3;
}

int msl_resize_bicubic_rgb(const uint8_t* src, int sh, int sw, int x0, int y0, int cw, int ch, int mirror,
                           const int32_t* xb, const int32_t* xk, int xks, const int32_t* yb, const int32_t* yk,
                           int yks, int ow, int oh, uint8_t* out_u8, float* out_f32, float mean_b, float mean_g,
                           float mean_r, void* ws, size_t ws_bytes, msl_stream_t stream) {
  if (!src || (!out_u8 && !out_f32) || !crop_ok(sh, sw, x0, y0, cw, ch, ow, oh)) return MSL_ERR_ARG;
  const bool hpass = xb || xk, vpass = yb || yk;
  int span = 0, unused = 0;
  if (hpass) {
    if (!xb || !xk || xks < 1 || xks > kMaxTaps || !bounds_ok(xb, ow, xks, cw, &span)) return MSL_ERR_ARG;
  } else if (ow != cw) {
    return MSL_ERR_ARG;
  }
  if (vpass) {
    if (!yb || !yk || yks < 1 || yks > kMaxTaps || !bounds_ok(yb, oh, yks, ch, &unused)) return MSL_ERR_ARG;
  } else if (oh != ch) {
    return MSL_ERR_ARG;
  }
  if (hpass && vpass && (!ws || ws_bytes < msl_resize_workspace(ch, ow))) return MSL_ERR_ARG;
  const size_t lds = ((size_t)span * 3 + 3 + 3) / 4 * 4;  // the run, its dword misalignment, rounded up
  if (lds > 60 * 1024) return MSL_ERR_ARG;
  const hipStream_t st = as_stream(stream);
  const int m = mirror ? 1 : 0;
  if (hpass) {
    // rows of the crop -> (ch, ow): the intermediate when a vertical pass follows, else the outputs
    uint8_t* h_u8 = vpass ? static_cast<uint8_t*>(ws) : out_u8;
    float* h_f32 = vpass ? nullptr : out_f32;
    MSL_LAUNCH(k_resize_h, dim3(cdiv(ow, kTile), ch), dim3(kTile), lds, st, src, sw, x0, y0, cw, m, xk, xks, ow, ch,
               span, h_u8, h_f32, mean_b, mean_g, mean_r);
    if (vpass)
      MSL_LAUNCH(k_resize_v<true>, dim3(cdiv(ow, 256), oh), dim3(256), 0, st, static_cast<const uint8_t*>(ws), ow, 0,
                 0, ch, 0, yk, yks, ow, oh, out_u8, out_f32, mean_b, mean_g, mean_r);
  } else if (vpass) {
    MSL_LAUNCH(k_resize_v<true>, dim3(cdiv(ow, 256), oh), dim3(256), 0, st, src, sw, x0, y0, ch, m, yk, yks, ow, oh,
               out_u8, out_f32, mean_b, mean_g, mean_r);
  } else {
    MSL_LAUNCH(k_resize_v<false>, dim3(cdiv(ow, 256), oh), dim3(256), 0, st, src, sw, x0, y0, ch, m, nullptr, 0, ow,
               oh, out_u8, out_f32, mean_b, mean_g, mean_r);
  }
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_resize_nearest_label(const uint8_t* ids, int sh, int sw, int x0, int y0, int cw, int ch, int mirror,
                             const int32_t* xtab, const int32_t* ytab, int ow, int oh, const int32_t* lut256,
                             uint8_t* out_u8, int64_t* out_i64, msl_stream_t stream) {
  if (!ids || (!out_u8 && !out_i64) || (out_i64 && !lut256) || !crop_ok(sh, sw, x0, y0, cw, ch, ow, oh))
    return MSL_ERR_ARG;
  if ((!xtab && ow != cw) || (!ytab && oh != ch)) return MSL_ERR_ARG;
  MSL_LAUNCH(k_resize_nearest, dim3(cdiv(ow, 256), oh), dim3(256), 0, as_stream(stream), ids, sw, x0, y0, cw, ch,
             mirror ? 1 : 0, xtab, ytab, ow, lut256, out_u8, out_i64);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

}  // extern "C"
