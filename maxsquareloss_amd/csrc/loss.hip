// Fused segmentation losses + bilinear upsampling on gfx950 (HBM/VALU-bound).
//
// Replaces, on the hot path of one UDA iteration (solve_gta5.py:178-235):
//   F.interpolate(.., align_corners=True)              deeplab_multi.py:124,128
//   F.softmax(pred, dim=1)                             solve_gta5.py:182-183
//   MaxSquareloss / IW_MaxSquareloss                   utils/loss.py:69-119
//   nn.CrossEntropyLoss(ignore_index=-1)               train_source.py:128
//   multi-level self-produced guidance label + CE      solve_gta5.py:206-213
//   softCrossEntropy / IWsoftCrossEntropy (MinEnt)     utils/loss.py:17-67
//   hard pseudo-label + CE (self-training)             solve_gta5.py:185-199
//
// The losses read the LOW-resolution logits [C][Hi][Wi] (0.6 MB, L2 resident)
// and re-interpolate every hi-res pixel on the fly with torch-CPU's exact
// rounding (t = fma(x0, w0, x1*w1) per axis, width first), so the 40 MB hi-res
// logits are never re-read.  Forward: one pass, per-block partial records,
// deterministic finalize.  Backward: the loss/softmax gradient of a hi-res row
// is formed in LDS and folded straight into the low-res gradient with the
// transposed (separable) interpolation weights: rows -> T[C][Ho][Wi] ->
// d logits[C][Hi][Wi], a fixed-order gather (no atomics).
#include "loss_common.h"  // the pieces shared with predict.hip; no FMA contraction in this file either

namespace msl {

enum LossKind { K_CE = 0, K_MS = 1, K_IW = 2, K_MULTI = 3, K_UPS = 4, K_ENT = 5, K_IWENT = 6, K_HARD = 7 };

constexpr int kStats = 64;       // floats in a stats record
constexpr int kFwdBlocks = 1024; // partial records per forward pass

// label2 of the multi-level guidance (solve_gta5.py:207-212)
template <int CM>
__device__ __forceinline__ int multi_label(const float (&P)[CM], const float (&P2)[CM], int C,
                                           float thr) {
  float m1, m2;
  argmax_first(P, C, m1);
  argmax_first(P2, C, m2);
  if (!(m1 > thr || m2 > thr)) return -1;
  float best = (P[0] + P2[0]) / 2.f;
  int a = 0;
#pragma unroll
  for (int c = 1; c < CM; ++c)
    if (c < C) {
      const float pc = (P[c] + P2[c]) / 2.f;
      if (pc > best) {
        best = pc;
        a = c;
      }
    }
  return a;
}

// label of the hard target mode (solve_gta5.py:185-197): argmax p where max p > thr, else -1
template <int CM>
__device__ __forceinline__ int hard_label(const float (&p)[CM], int C, float thr) {
  float best;
  const int a = argmax_first<CM>(p, C, best);
  return best > thr ? a : -1;
}

// log_softmax as (v_c - max) - log(sum) (never log(p_c): p_c may round to 0) and the pixel's
// entropy H = sum_c (-lp_c) * p_c in ascending c, shared by the forward and the backward
template <int CM>
__device__ __forceinline__ float log_softmax_entropy(const float (&v)[CM], const float (&p)[CM],
                                                     int C, float mx, float sum, float (&lp)[CM]) {
  const float ls = logf(sum);
  float h = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) {
      lp[c] = (v[c] - mx) - ls;
      h += -lp[c] * p[c];
    }
  return h;
}

// Block-wide sum of one float (256 threads) -> returned to all threads.
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------- forward
// Partial record layout per block (floats):
//   CE / MULTI: [0] = sum of -log p[y], [1] = n_valid
//   MS:         [0] = sum p^2
//   IW:         [0..C) = per-class sum of sum_k p_k^2 (by argmax class), [C..2C) = per-class count
//   ENT:        [0] = sum of -lp * p (the pixel entropies)
//   IWENT:      [0..C) = per-class sum of the pixel entropy (by the LOGITS' argmax class,
//               loss.py:54), [C..2C) = per-class count
//   HARD:       [0] = sum of -lp[y], [1] = n_valid (y = hard_label)
template <int KIND, int CM>
__global__ void __launch_bounds__(256) k_loss_fwd(const float* __restrict__ L1,
                                                   const float* __restrict__ L2,
                                                   const int64_t* __restrict__ labels, Geo g,
                                                   float thr, float* __restrict__ part, int rec) {
  __shared__ float red[4];
  const int npx = g.Ho * g.Wo;
  float a0 = 0.f, a1 = 0.f;
  float cs[CM], cn[CM];
#pragma unroll
  for (int c = 0; c < CM; ++c) cs[c] = cn[c] = 0.f;

  for (int px = blockIdx.x * 256 + threadIdx.x; px < npx; px += gridDim.x * 256) {
    const int oy = px / g.Wo, ox = px - oy * g.Wo;
    const Lin ly = lin(oy, g.sh, g.Hi), lx = lin(ox, g.sw, g.Wi);
    float v[CM], p[CM], mx, sum;
    up_logits<CM>(L1, g, ly, lx, v);
    softmax<CM>(v, g.C, p, mx, sum);
    if (KIND == K_CE) {
      const int y = (int)labels[px];
      if (y >= 0 && y < g.C) {
        float vy = v[0];
#pragma unroll
        for (int c = 1; c < CM; ++c)
          if (c == y) vy = v[c];
        a0 += -((vy - mx) - logf(sum));
        a1 += 1.f;
      }
    } else if (KIND == K_MS) {
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < g.C) a0 += p[c] * p[c];
    } else if (KIND == K_IW) {
      float best;
      const int am = argmax_first<CM>(p, g.C, best);
      float s2 = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < g.C) s2 += p[c] * p[c];
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c == am) {
          cs[c] += s2;
          cn[c] += 1.f;
        }
    } else if (KIND == K_MULTI) {
      float v2[CM], P[CM], mx2, sum2;
      up_logits<CM>(L2, g, ly, lx, v2);
      softmax<CM>(v2, g.C, P, mx2, sum2);
      const int y = multi_label<CM>(P, p, g.C, thr);
      if (y >= 0) {
        float vy = v[0];
#pragma unroll
        for (int c = 1; c < CM; ++c)
          if (c == y) vy = v[c];
        a0 += -((vy - mx) - logf(sum));
        a1 += 1.f;
      }
    } else if (KIND == K_ENT) {
      float lp[CM];
      a0 += log_softmax_entropy<CM>(v, p, g.C, mx, sum, lp);
    } else if (KIND == K_IWENT) {
      float lp[CM], best;
      const float h = log_softmax_entropy<CM>(v, p, g.C, mx, sum, lp);
      const int am = argmax_first<CM>(v, g.C, best);
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c == am) {
          cs[c] += h;
          cn[c] += 1.f;
        }
    } else if (KIND == K_HARD) {
      const int y = hard_label<CM>(p, g.C, thr);
      if (y >= 0) {
        float vy = v[0];
#pragma unroll
        for (int c = 1; c < CM; ++c)
          if (c == y) vy = v[c];
        a0 += -((vy - mx) - logf(sum));
        a1 += 1.f;
      }
    }
  }
  float* rp = part + (long long)blockIdx.x * rec;
  if (KIND == K_IW || KIND == K_IWENT) {
    for (int c = 0; c < g.C; ++c) {
      float s = 0.f, n = 0.f;
#pragma unroll
      for (int k = 0; k < CM; ++k)
        if (k == c) {
          s = cs[k];
          n = cn[k];
        }
      s = block_sum(s, red);
      n = block_sum(n, red);
      if (threadIdx.x == 0) {
        rp[c] = s;
        rp[g.C + c] = n;
      }
    }
  } else {
    const float s0 = block_sum(a0, red);
    const float s1 = block_sum(a1, red);
    if (threadIdx.x == 0) {
      rp[0] = s0;
      rp[1] = s1;
    }
  }
}

// Deterministic finalize: one block sums the partial records in fixed order.
// stats: [0] loss, [1] n_valid (CE/MULTI/HARD) or H*W (MS/IW/ENT/IWENT), [2..2+C) class weights
// (IW/IWENT)
template <int KIND>
__global__ void __launch_bounds__(256) k_loss_finalize(const float* __restrict__ part, int nblk,
                                                        int rec, int C, int npx, float ratio,
                                                        float* __restrict__ out,
                                                        float* __restrict__ stats,
                                                        int32_t* __restrict__ hist,
                                                        float* __restrict__ weights) {
  __shared__ double sred[256];
  const int nvals = (KIND == K_IW || KIND == K_IWENT) ? 2 * C : 2;
  __shared__ double vals[2 * kMaxC];
  for (int j = 0; j < nvals; ++j) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) s += (double)part[(long long)b * rec + j];
    sred[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (threadIdx.x < w) sred[threadIdx.x] += sred[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) vals[j] = sred[0];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  for (int k = 0; k < kStats; ++k) stats[k] = 0.f;
  if (KIND == K_CE || KIND == K_MULTI || KIND == K_HARD) {
    const float n = (float)vals[1];
    const float loss = (float)(vals[0] / vals[1]);  // 0/0 -> nan, as the reference (quirk Q8)
    out[0] = loss;
    stats[0] = loss;
    stats[1] = n;
  } else if (KIND == K_MS) {
    const float loss = (float)(-vals[0] / (2.0 * (double)C * (double)npx));
    out[0] = loss;
    stats[0] = loss;
    stats[1] = (float)npx;
  } else if (KIND == K_ENT) {
    const float loss = (float)(vals[0] / ((double)C * (double)npx));  // loss.py:33, no factor 1/2
    out[0] = loss;
    stats[0] = loss;
    stats[1] = (float)npx;
  } else if (KIND == K_IW || KIND == K_IWENT) {
    // weight = 1 / max(hist^r * (sum hist)^(1-r), 1)   (loss.py:61, :95), fp32 as the reference
    float tot = 0.f;
    for (int c = 0; c < C; ++c) tot += (float)vals[C + c];
    const float tp = powf(tot, 1.f - ratio);
    double l = 0.0;
    for (int c = 0; c < C; ++c) {
      const float h = (float)vals[C + c];
      const float w = 1.f / fmaxf(powf(h, ratio) * tp, 1.f);
      stats[2 + c] = w;
      if (weights) weights[c] = w;
      if (hist) hist[c] = (int32_t)vals[C + c];
      l += (double)w * vals[c];
    }
    const float loss = KIND == K_IW ? (float)(-l / (double)C) : (float)(l / (double)C);
    out[0] = loss;
    stats[0] = loss;
    stats[1] = (float)npx;
  }
}

// ---------------------------------------------------------------- backward
// Per-pixel hi-res gradient g[c] = dL/d logit_hi[c] for the loss KIND.
struct BwdScal {
  float a;  // CE/MULTI/HARD: gout / n_valid ; MS/ENT: -gout / (C*H*W) ; IW: -2*gout / C ; IWENT: -gout / C
};

template <int KIND, int CM>
__device__ __forceinline__ void pixel_grad(const float* __restrict__ L1, const float* __restrict__ L2,
                                           const int64_t* __restrict__ labels,
                                           const float* __restrict__ gin_hi, const Geo& g,
                                           const float* __restrict__ stats, float thr, float sc,
                                           int oy, int ox, const Lin& ly, float (&gr)[CM]) {
  if (KIND == K_UPS) {
    const long long hw = (long long)g.Ho * g.Wo;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < g.C) gr[c] = gin_hi[c * hw + (long long)oy * g.Wo + ox];
    return;
  }
  const Lin lx = lin(ox, g.sw, g.Wi);
  float v[CM], p[CM], mx, sum;
  up_logits<CM>(L1, g, ly, lx, v);
  softmax<CM>(v, g.C, p, mx, sum);
  if (KIND == K_CE || KIND == K_MULTI || KIND == K_HARD) {
    int y;
    if (KIND == K_CE) {
      y = (int)labels[(long long)oy * g.Wo + ox];
      if (y >= g.C) y = -1;
    } else if (KIND == K_HARD) {
      y = hard_label<CM>(p, g.C, thr);
    } else {
      float v2[CM], P[CM], mx2, sum2;
      up_logits<CM>(L2, g, ly, lx, v2);
      softmax<CM>(v2, g.C, P, mx2, sum2);
      y = multi_label<CM>(P, p, g.C, thr);
    }
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < g.C) gr[c] = y < 0 ? 0.f : sc * (p[c] - (c == y ? 1.f : 0.f));
  } else if (KIND == K_ENT || KIND == K_IWENT) {
    // d/dv_c sum_k -lp_k p_k = -p_c (lp_c + H): the target softmax is not detached (loss.py:33)
    float lp[CM];
    const float h = log_softmax_entropy<CM>(v, p, g.C, mx, sum, lp);
    float a = sc;
    if (KIND == K_IWENT) {
      float best;
      const int am = argmax_first<CM>(v, g.C, best);
      float w = stats[2];
#pragma unroll
      for (int c = 1; c < CM; ++c)
        if (c == am) w = stats[2 + c];
      a = sc * w;
    }
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < g.C) gr[c] = a * p[c] * (lp[c] + h);
  } else {
    float s2 = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < g.C) s2 += p[c] * p[c];
    float a = sc;
    if (KIND == K_IW) {
      float best;
      const int am = argmax_first<CM>(p, g.C, best);
      float w = stats[2];
#pragma unroll
      for (int c = 1; c < CM; ++c)
        if (c == am) w = stats[2 + c];
      a = sc * w;
    }
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < g.C) gr[c] = a * p[c] * (p[c] - s2);
  }
}

// first ox with i0(ox) >= t (i0 is monotone in ox), searched in [lo, hi)
__device__ __forceinline__ int lb_ox(int t, int lo, int hi, const Geo& g) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (lin(mid, g.sw, g.Wi).i0 >= t) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// Block (oy, j): hi-res row oy, low-res columns ix in [ixa, ixb) (chunk j of gridDim.y).  The
// pixels that feed those columns, ox with i0(ox) in [ixa - 1, ixb), get their gradient G[c][ox]
// in LDS, then T[c][oy][ix] = sum_ox Wx[ox][ix] G[c][ox] in ascending ox (fp64).  Chunks of ~33
// columns (~280 pixels) instead of a whole row per block: 4x the blocks at a quarter of the LDS,
// so the latency-bound per-pixel softmax has 3-4x the waves in flight (r01: 130 us per loss).
// A pixel on a chunk border is computed by both neighbours: the same value, so T is unchanged.
template <int KIND, int CM>
__global__ void __launch_bounds__(256) k_bwd_rows(const float* __restrict__ L1,
                                                   const float* __restrict__ L2,
                                                   const int64_t* __restrict__ labels,
                                                   const float* __restrict__ gin_hi, Geo g, float thr,
                                                   const float* __restrict__ stats,
                                                   const float* __restrict__ gout,
                                                   float* __restrict__ T, int wmax) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* G = sm;                               // [C][wmax]
  float* wx0 = G + g.C * wmax;                 // [wmax]
  float* wx1 = wx0 + wmax;                     // [wmax]
  int* ix0 = reinterpret_cast<int*>(wx1 + wmax);  // [wmax]

  const int oy = blockIdx.x;
  const int nch = gridDim.y, per = (g.Wi + nch - 1) / nch;
  const int ixa = blockIdx.y * per, ixb = min(g.Wi, ixa + per);
  if (ixa >= ixb) return;
  const int ox_lo = lb_ox(ixa - 1, 0, g.Wo, g);
  const int ox_hi = ixb >= g.Wi ? g.Wo : lb_ox(ixb, ox_lo, g.Wo, g);
  const int nw = ox_hi - ox_lo;  // <= wmax (host bound)
  const Lin ly = lin(oy, g.sh, g.Hi);
  float sc = 0.f;
  if (KIND == K_CE || KIND == K_MULTI || KIND == K_HARD) sc = gout[0] / stats[1];
  else if (KIND == K_MS || KIND == K_ENT) sc = -gout[0] / ((float)g.C * stats[1]);
  else if (KIND == K_IW) sc = -2.f * gout[0] / (float)g.C;
  else if (KIND == K_IWENT) sc = -gout[0] / (float)g.C;

  for (int k = threadIdx.x; k < nw; k += 256) {
    const int ox = ox_lo + k;
    const Lin lx = lin(ox, g.sw, g.Wi);
    wx0[k] = lx.w0;
    wx1[k] = lx.w1;
    ix0[k] = lx.i0;
    float gr[CM];
    pixel_grad<KIND, CM>(L1, L2, labels, gin_hi, g, stats, thr, sc, oy, ox, ly, gr);
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < g.C) G[c * wmax + k] = gr[c];
  }
  __syncthreads();
  auto bnd = [&](int t) {  // first chunk pixel with i0 >= t (t in [ixa - 1, ixb])
    int lo = 0, hi = nw;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ix0[mid] >= t) hi = mid;
      else lo = mid + 1;
    }
    return lo;
  };
  const long long plane = (long long)g.Ho * g.Wi;
  const int ncol = ixb - ixa;
  for (int e = threadIdx.x; e < g.C * ncol; e += 256) {
    const int c = e / ncol, ix = ixa + (e - c * ncol);
    const int beg = bnd(ix > 0 ? ix - 1 : 0), end = ix + 1 <= g.Wi - 1 ? bnd(ix + 1) : nw;
    const float* Gc = G + c * wmax;
    double s = 0.0;  // ~2*Wo/Wi terms; fp64 keeps the gather at fp32-rounding accuracy
    for (int k = beg; k < end; ++k) {
      const int i0 = ix0[k];
      const int i1 = i0 + (i0 < g.Wi - 1 ? 1 : 0);
      float w = 0.f;
      if (i0 == ix) w += wx0[k];
      if (i1 == ix) w += wx1[k];
      s += (double)w * (double)Gc[k];
    }
    T[c * plane + (long long)oy * g.Wi + ix] = (float)s;
  }
}

// dlow[c][iy][ix] = sum_oy Wy[oy][iy] T[c][oy][ix]
__global__ void __launch_bounds__(256) k_bwd_cols(const float* __restrict__ T, Geo g,
                                                   float* __restrict__ dlow) {
  const int n = g.C * g.Hi * g.Wi;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
    const int ix = e % g.Wi;
    const int r = e / g.Wi;
    const int iy = r % g.Hi;
    const int c = r / g.Hi;
    // oy range: i0(oy) in {iy-1, iy}
    auto lb = [&](int target) {
      int lo = 0, hi = g.Ho;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lin(mid, g.sh, g.Hi).i0 >= target) hi = mid;
        else lo = mid + 1;
      }
      return lo;
    };
    const int beg = lb(iy > 0 ? iy - 1 : 0), end = lb(iy + 1);
    const float* Tc = T + (long long)c * g.Ho * g.Wi + ix;
    double s = 0.0;
    for (int oy = beg; oy < end; ++oy) {
      const Lin ly = lin(oy, g.sh, g.Hi);
      float w = 0.f;
      if (ly.i0 == iy) w += ly.w0;
      if (ly.i1 == iy) w += ly.w1;
      s += (double)w * (double)Tc[(long long)oy * g.Wi];
    }
    dlow[e] = (float)s;
  }
}

// ---------------------------------------------------------------- upsample forward
__global__ void __launch_bounds__(256) k_upsample_fwd(const float* __restrict__ in, Geo g,
                                                       float* __restrict__ out) {
  const unsigned wq = (g.Wo + 3) / 4;
  const unsigned n = (unsigned)g.C * g.Ho * wq;  // < 2^31 (msl_upsample_fwd checks): 32-bit decode
  const long long hwo = (long long)g.Ho * g.Wo;
  const bool vec = (g.Wo & 3) == 0;
  for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < n; e += gridDim.x * 256u) {
    const int q = (int)(e % wq);
    const unsigned r = e / wq;
    const int oy = (int)(r % (unsigned)g.Ho);
    const int c = (int)(r / (unsigned)g.Ho);
    const Lin ly = lin(oy, g.sh, g.Hi);
    const float* plane = in + (long long)c * g.Hi * g.Wi;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ox = min(q * 4 + k, g.Wo - 1);
      v[k] = bilerp(plane, g.Wi, ly, lin(ox, g.sw, g.Wi));
    }
    float* o = out + (long long)c * hwo + (long long)oy * g.Wo + q * 4;
    if (vec) {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (q * 4 + k < g.Wo) o[k] = v[k];
    }
  }
}

// torch-CPU's other bilinear form.  Where ho + wo <= 128 its CPU kernel does not interpolate per axis:
// it rounds the four weight products and sums the taps as fma chains starting from the (y0, x1) tap:
//   w_ab = ly.w_a * lx.w_b;   r = w01 * v01;   r = fma(w00, v00, r);   r = fma(w10, v10, r);   r = fma(w11, v11, r)
// (the scalar form its fewer-than-a-vector channel counts take: images and masks).  One output per thread:
// at most 64 x 64 pixels of at most kResizeMaxC planes.
constexpr int kResizeMaxC = 4;
__global__ void __launch_bounds__(256) k_resize_four(const float* __restrict__ in, Geo g,
                                                      float* __restrict__ out) {
  const int n = g.C * g.Ho * g.Wo;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
    const int ox = e % g.Wo, r = e / g.Wo;
    const int oy = r % g.Ho, c = r / g.Ho;
    const Lin ly = lin(oy, g.sh, g.Hi), lx = lin(ox, g.sw, g.Wi);
    const float* r0 = in + ((long long)c * g.Hi + ly.i0) * g.Wi;
    const float* r1 = in + ((long long)c * g.Hi + ly.i1) * g.Wi;
    float acc = __fmul_rn(__fmul_rn(ly.w0, lx.w1), r0[lx.i1]);
    acc = __fmaf_rn(__fmul_rn(ly.w0, lx.w0), r0[lx.i0], acc);
    acc = __fmaf_rn(__fmul_rn(ly.w1, lx.w0), r1[lx.i0], acc);
    acc = __fmaf_rn(__fmul_rn(ly.w1, lx.w1), r1[lx.i1], acc);
    out[e] = acc;
  }
}

// ---------------------------------------------------------------- prob-input losses
// record: [0] sum p^2 (MS) | IW: [0..C) class sums, [C..2C) class counts
template <int IW, int CM>
__global__ void __launch_bounds__(256) k_prob_fwd(const float* __restrict__ prob,
                                                   const int64_t* __restrict__ label, int C, int hw,
                                                   float* __restrict__ part, int rec) {
  __shared__ float red[4];
  float a0 = 0.f;
  float cs[CM], cn[CM];
#pragma unroll
  for (int c = 0; c < CM; ++c) cs[c] = cn[c] = 0.f;
  for (int px = blockIdx.x * 256 + threadIdx.x; px < hw; px += gridDim.x * 256) {
    float p[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) p[c] = prob[(long long)c * hw + px];
    float s2 = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) s2 += p[c] * p[c];
    if (!IW) {
      a0 += s2;
    } else {
      float best;
      const int am = argmax_first<CM>(p, C, best);
      const int lb = label ? (int)label[px] : am;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        if (c == am) cs[c] += s2;
        if (c == lb) cn[c] += 1.f;
      }
    }
  }
  float* rp = part + (long long)blockIdx.x * rec;
  if (IW) {
    for (int c = 0; c < C; ++c) {
      float s = 0.f, n = 0.f;
#pragma unroll
      for (int k = 0; k < CM; ++k)
        if (k == c) {
          s = cs[k];
          n = cn[k];
        }
      s = block_sum(s, red);
      n = block_sum(n, red);
      if (threadIdx.x == 0) {
        rp[c] = s;
        rp[C + c] = n;
      }
    }
  } else {
    const float s = block_sum(a0, red);
    if (threadIdx.x == 0) rp[0] = s;
  }
}

template <int IW, int CM>
__global__ void __launch_bounds__(256) k_prob_bwd(const float* __restrict__ prob, int C, int hw,
                                                   const float* __restrict__ weights,
                                                   const float* __restrict__ gout,
                                                   float* __restrict__ dprob) {
  const float g = gout[0];
  for (int px = blockIdx.x * 256 + threadIdx.x; px < hw; px += gridDim.x * 256) {
    float p[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) p[c] = prob[(long long)c * hw + px];
    float a;
    if (IW) {
      float best;
      const int am = argmax_first<CM>(p, C, best);
      a = -2.f * g * weights[am] / (float)C;
    } else {
      a = -g / ((float)C * (float)hw);
    }
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) dprob[(long long)c * hw + px] = a * p[c];
  }
}

// ---------------------------------------------------------------- soft cross-entropy, explicit tensors
// softCrossEntropy / IWsoftCrossEntropy (loss.py:17-67) on hi-res logits x[C][hw] and an explicit
// target distribution t[C][hw]; m = (t != ignore) per element.
// record: plain: [0] = sum m * (-lp * t), [1] = sum m | IW: [0..C) per-class sums of the pixel's
// sum_c m * (-lp * t) (by the logits' argmax class), [C..2C) class counts
template <int CM>
__device__ __forceinline__ void load_px(const float* __restrict__ x, int C, int hw, int px,
                                        float (&v)[CM]) {
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) v[c] = x[(long long)c * hw + px];
}

template <int IW, int CM>
__global__ void __launch_bounds__(256) k_soft_fwd(const float* __restrict__ x,
                                                   const float* __restrict__ t, int C, int hw,
                                                   float ignore, float* __restrict__ part, int rec) {
  __shared__ float red[4];
  float a0 = 0.f, a1 = 0.f;
  float cs[CM], cn[CM];
#pragma unroll
  for (int c = 0; c < CM; ++c) cs[c] = cn[c] = 0.f;
  for (int px = blockIdx.x * 256 + threadIdx.x; px < hw; px += gridDim.x * 256) {
    float v[CM], tt[CM], p[CM], mx, sum;
    load_px<CM>(x, C, hw, px, v);
    load_px<CM>(t, C, hw, px, tt);
    softmax<CM>(v, C, p, mx, sum);
    const float ls = logf(sum);
    float s = 0.f, n = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C && tt[c] != ignore) {
        s += -((v[c] - mx) - ls) * tt[c];
        n += 1.f;
      }
    if (!IW) {
      a0 += s;
      a1 += n;
    } else {
      float best;
      const int am = argmax_first<CM>(v, C, best);
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c == am) {
          cs[c] += s;
          cn[c] += 1.f;
        }
    }
  }
  float* rp = part + (long long)blockIdx.x * rec;
  if (IW) {
    for (int c = 0; c < C; ++c) {
      float s = 0.f, n = 0.f;
#pragma unroll
      for (int k = 0; k < CM; ++k)
        if (k == c) {
          s = cs[k];
          n = cn[k];
        }
      s = block_sum(s, red);
      n = block_sum(n, red);
      if (threadIdx.x == 0) {
        rp[c] = s;
        rp[C + c] = n;
      }
    }
  } else {
    const float s0 = block_sum(a0, red);
    const float s1 = block_sum(a1, red);
    if (threadIdx.x == 0) {
      rp[0] = s0;
      rp[1] = s1;
    }
  }
}

// dx_c = a * (p_c * S - m_c t_c), S = sum_k m_k t_k; dt_c = -a * m_c * lp_c; a = gout / n (plain;
// 0 when no element is kept: the reference's mean over nothing has a zero gradient) or
// gout * w[argmax x] / C (IW).  dx / dt nullable.
template <int IW, int CM>
__global__ void __launch_bounds__(256) k_soft_bwd(const float* __restrict__ x,
                                                   const float* __restrict__ t, int C, int hw,
                                                   float ignore, const float* __restrict__ stats,
                                                   const float* __restrict__ gout,
                                                   float* __restrict__ dx, float* __restrict__ dt) {
  const float g = gout[0];
  for (int px = blockIdx.x * 256 + threadIdx.x; px < hw; px += gridDim.x * 256) {
    float v[CM], tt[CM], p[CM], mx, sum;
    load_px<CM>(x, C, hw, px, v);
    load_px<CM>(t, C, hw, px, tt);
    softmax<CM>(v, C, p, mx, sum);
    const float ls = logf(sum);
    float a;
    if (IW) {
      float best;
      const int am = argmax_first<CM>(v, C, best);
      a = g * stats[2 + am] / (float)C;
    } else {
      a = stats[1] > 0.f ? g / stats[1] : 0.f;
    }
    float S = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C && tt[c] != ignore) S += tt[c];
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) {
        const bool m = tt[c] != ignore;
        if (dx) dx[(long long)c * hw + px] = a * (p[c] * S - (m ? tt[c] : 0.f));
        if (dt) dt[(long long)c * hw + px] = m ? -a * ((v[c] - mx) - ls) : 0.f;
      }
  }
}

// ---------------------------------------------------------------- label inspection
// The per-pixel decisions the fused losses take internally, written out: arg[px] = first-max
// argmax of softmax(up(L1)) (the IW histogram's class, loss.py:84-86), label2[px] = the
// multi-level guidance label with P = softmax(up(L2)), P2 = softmax(up(L1)) (solve_gta5.py:
// 206-212; -1 = ignored).  Same device functions as k_loss_fwd / pixel_grad.
template <int CM>
__global__ void __launch_bounds__(256) k_loss_labels(const float* __restrict__ L1,
                                                      const float* __restrict__ L2, Geo g,
                                                      float thr, int32_t* __restrict__ arg,
                                                      int32_t* __restrict__ label2) {
  const int npx = g.Ho * g.Wo;
  for (int px = blockIdx.x * 256 + threadIdx.x; px < npx; px += gridDim.x * 256) {
    const int oy = px / g.Wo, ox = px - oy * g.Wo;
    const Lin ly = lin(oy, g.sh, g.Hi), lx = lin(ox, g.sw, g.Wi);
    float v[CM], p[CM], mx, sum;
    up_logits<CM>(L1, g, ly, lx, v);
    softmax<CM>(v, g.C, p, mx, sum);
    if (arg) {
      float best;
      arg[px] = argmax_first<CM>(p, g.C, best);
    }
    if (label2) {
      float v2[CM], P[CM], mx2, sum2;
      up_logits<CM>(L2, g, ly, lx, v2);
      softmax<CM>(v2, g.C, P, mx2, sum2);
      label2[px] = multi_label<CM>(P, p, g.C, thr);
    }
  }
}

// The decisions of the hard / IW-entropy kinds: label[px] = hard_label of softmax(up(L1)) (-1 =
// ignored), arg[px] = first-max argmax of the upsampled LOGITS (IWsoftCrossEntropy's histogram
// class, loss.py:54).  Same device functions as k_loss_fwd / pixel_grad.
template <int CM>
__global__ void __launch_bounds__(256) k_pseudo_labels(const float* __restrict__ L1, Geo g,
                                                        float thr, int32_t* __restrict__ label,
                                                        int32_t* __restrict__ arg) {
  const int npx = g.Ho * g.Wo;
  for (int px = blockIdx.x * 256 + threadIdx.x; px < npx; px += gridDim.x * 256) {
    const int oy = px / g.Wo, ox = px - oy * g.Wo;
    const Lin ly = lin(oy, g.sh, g.Hi), lx = lin(ox, g.sw, g.Wi);
    float v[CM];
    up_logits<CM>(L1, g, ly, lx, v);
    if (arg) {
      float best;
      arg[px] = argmax_first<CM>(v, g.C, best);
    }
    if (label) {
      float p[CM], mx, sum;
      softmax<CM>(v, g.C, p, mx, sum);
      label[px] = hard_label<CM>(p, g.C, thr);
    }
  }
}

// ---------------------------------------------------------------- host helpers
static int rec_len(int C) { return 2 * C > 2 ? 2 * C : 2; }

// partial records + one trailing stats record (used by the prob-input forms)
static size_t part_bytes(int C) {
  return align_up(((size_t)kFwdBlocks * rec_len(C) + kStats) * 4, 256);
}

static size_t t_bytes(int c, int ho, int wi) { return align_up((size_t)c * ho * wi * 4, 256); }

// k_bwd_rows: column chunks per hi-res row, and the widest pixel range a chunk can need: the
// pixels whose i0 is one of the chunk's columns or the one before, at most ceil(1/sw) + 1 per
// column (sw = (Wi-1)/(Wo-1), fp32 as torch computes it), clamped to the row
static int rows_chunks(const Geo& g) { return std::max(1, std::min(8, g.Wi / 32)); }
static int rows_per(const Geo& g) { return (g.Wi + rows_chunks(g) - 1) / rows_chunks(g); }  // k_bwd_rows' `per`
static int rows_wmax(const Geo& g) {
  const int per = rows_per(g);
  if (g.Wi < 2 || !(g.sw > 0.f)) return g.Wo;
  const long long each = (long long)std::ceil(1.0 / (double)g.sw) + 2;
  return (int)std::min<long long>(g.Wo, (per + 1) * each);
}
static size_t rows_lds(const Geo& g) { return (size_t)rows_wmax(g) * (g.C * 4 + 12); }

constexpr size_t kRowsLdsDefault = 64 * 1024;  // dynamic LDS a kernel gets without opting in
constexpr size_t kRowsLdsMax = 160 * 1024;     // a gfx950 workgroup's LDS

// A grid-stride launch of 256-thread blocks over n items under a block cap: the blocks, and the
// trips of the kernel's loop a thread of the first block makes.
struct Flat {
  int blocks, trips;
};
static Flat flat_launch(long long n, int cap) {
  Flat f;
  f.blocks = (int)std::min<long long>((n + 255) / 256, cap);
  f.trips = (int)((n + (long long)f.blocks * 256 - 1) / ((long long)f.blocks * 256));
  return f;
}
constexpr int kColsBlocks = 2048;     // k_bwd_cols
constexpr int kFlatBwdBlocks = 4096;  // k_prob_bwd, k_soft_bwd, k_loss_labels, k_pseudo_labels
constexpr int kUpsampleBlocks = 8192; // k_upsample_fwd
constexpr int kResizeFourMax = 128;   // msl_resize_bilinear: ho + wo up to here take k_resize_four

// What a call of this file does with its geometry, computed once: every launch below reads its
// grid, its LDS and its refusals from one of these records and msl_loss_plan reports the same
// record, so the two cannot drift.  Pointer checks stay with the entry points.
struct LossPlan {
  int status;
  Flat fwd;        // the forward kernel (k_loss_fwd, k_prob_fwd, k_soft_fwd, k_upsample_fwd, k_resize_four,
                   // the label kernels) or the flat backward (k_prob_bwd, k_soft_bwd)
  int chunks, per, wmax;  // k_bwd_rows
  size_t lds;
  bool optin;      // lds above the default: hipFuncSetAttribute before the launch
  Flat cols;       // k_bwd_cols
  bool vec;        // k_upsample_fwd stores float4 (the kernel's own test of Wo)
  bool four;       // msl_resize_bilinear runs k_resize_four, else msl_upsample_fwd's launch
  size_t ws_need;
};

static bool upsample_vec(int wo) { return (wo & 3) == 0; }

static LossPlan refused(LossPlan pl, int status) {
  pl.status = status;
  return pl;
}

// k_loss_fwd + k_loss_finalize
static LossPlan up_fwd_plan(int c, int hi, int wi, int ho, int wo, size_t ws_bytes) {
  LossPlan pl = {};
  if (!geo_ok(c, hi, wi, ho, wo)) return refused(pl, MSL_ERR_ARG);
  pl.ws_need = part_bytes(c);
  if (ws_bytes < pl.ws_need) return refused(pl, MSL_ERR_WORKSPACE);
  pl.fwd = flat_launch((long long)ho * wo, kFwdBlocks);
  return pl;
}

// k_bwd_rows + k_bwd_cols (the losses and msl_upsample_bwd)
static LossPlan up_bwd_plan(int c, int hi, int wi, int ho, int wo, size_t ws_bytes) {
  LossPlan pl = {};
  if (!geo_ok(c, hi, wi, ho, wo)) return refused(pl, MSL_ERR_ARG);
  pl.ws_need = t_bytes(c, ho, wi);
  if (ws_bytes < pl.ws_need) return refused(pl, MSL_ERR_WORKSPACE);
  const Geo g = make_geo(c, hi, wi, ho, wo);
  pl.chunks = rows_chunks(g);
  pl.per = rows_per(g);
  pl.wmax = rows_wmax(g);
  pl.lds = rows_lds(g);
  pl.optin = pl.lds > kRowsLdsDefault;
  if (pl.lds > kRowsLdsMax) return refused(pl, MSL_ERR_SHAPE);
  pl.cols = flat_launch((long long)c * hi * wi, kColsBlocks);
  return pl;
}

// k_loss_labels / k_pseudo_labels
static LossPlan labels_plan(int c, int hi, int wi, int ho, int wo) {
  LossPlan pl = {};
  if (!geo_ok(c, hi, wi, ho, wo)) return refused(pl, MSL_ERR_ARG);
  pl.fwd = flat_launch((long long)ho * wo, kFlatBwdBlocks);
  return pl;
}

// k_upsample_fwd; max_c: kResizeMaxC through msl_resize_bilinear, else no limit
static LossPlan upsample_fwd_plan(int c, int hi, int wi, int ho, int wo, int max_c = 0) {
  LossPlan pl = {};
  if (c < 1 || (max_c && c > max_c) || hi < 1 || wi < 1 || ho < 1 || wo < 1 || (long long)c * ho * wo >= (1LL << 31))
    return refused(pl, MSL_ERR_ARG);
  pl.fwd = flat_launch((long long)c * ho * ((wo + 3) / 4), kUpsampleBlocks);
  pl.vec = upsample_vec(wo);
  return pl;
}

// msl_resize_bilinear: k_resize_four (one output per thread) or msl_upsample_fwd's launch
static LossPlan resize_plan(int c, int hi, int wi, int ho, int wo) {
  LossPlan pl = upsample_fwd_plan(c, hi, wi, ho, wo, kResizeMaxC);
  if (pl.status != MSL_OK || (long long)ho + wo > kResizeFourMax) return pl;
  pl.four = true;
  pl.vec = false;
  pl.fwd.blocks = cdiv((long long)c * ho * wo, 256);
  pl.fwd.trips = 1;
  return pl;
}

// the prob and soft forms on [C][hw]: the forward (partial records, then a finalize) and the backward
static LossPlan flat_fwd_plan(int c, int hw, size_t ws_bytes) {
  LossPlan pl = {};
  if (c < 1 || c > kMaxC || hw < 1) return refused(pl, MSL_ERR_ARG);
  pl.ws_need = part_bytes(c);
  if (ws_bytes < pl.ws_need) return refused(pl, MSL_ERR_WORKSPACE);
  pl.fwd = flat_launch(hw, kFwdBlocks);
  return pl;
}

static LossPlan flat_bwd_plan(int c, int hw) {
  LossPlan pl = {};
  if (c < 1 || c > kMaxC || hw < 1) return refused(pl, MSL_ERR_ARG);
  pl.fwd = flat_launch(hw, kFlatBwdBlocks);
  return pl;
}

template <int KIND>
static int loss_fwd(const float* L1, const float* L2, const int64_t* labels, int c, int hi, int wi,
                    int ho, int wo, float thr, float ratio, float* out, float* stats,
                    int32_t* hist, float* weights, void* ws, size_t ws_bytes, msl_stream_t s) {
  if (!L1 || !out || !stats) return MSL_ERR_ARG;
  const LossPlan pl = up_fwd_plan(c, hi, wi, ho, wo, ws_bytes);
  if (pl.status != MSL_OK) return pl.status;
  const Geo g = make_geo(c, hi, wi, ho, wo);
  hipStream_t st = as_stream(s);
  float* part = (float*)ws;
  const int rec = rec_len(c);
  const int nblk = pl.fwd.blocks;
  MSL_DISPATCH_C(c, CM,
                 MSL_LAUNCH((k_loss_fwd<KIND, CM>), dim3(nblk), dim3(256), 0, st, L1, L2,
                                    labels, g, thr, part, rec));
  MSL_CHECK_LAUNCH();
  MSL_LAUNCH((k_loss_finalize<KIND>), dim3(1), dim3(256), 0, st, part, nblk, rec, c,
                     ho * wo, ratio, out, stats, hist, weights);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

template <int KIND>
static int loss_bwd(const float* L1, const float* L2, const int64_t* labels, const float* gin_hi,
                    int c, int hi, int wi, int ho, int wo, float thr, const float* stats,
                    const float* gout, float* dlow, void* ws, size_t ws_bytes, msl_stream_t s) {
  if (!dlow) return MSL_ERR_ARG;
  const LossPlan pl = up_bwd_plan(c, hi, wi, ho, wo, ws_bytes);
  if (pl.status != MSL_OK) return pl.status;
  const Geo g = make_geo(c, hi, wi, ho, wo);
  const size_t lds = pl.lds;
  hipStream_t st = as_stream(s);
  float* T = (float*)ws;
  MSL_DISPATCH_C(c, CM, {
    constexpr auto kern = k_bwd_rows<KIND, CM>;
    if (pl.optin) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    MSL_LAUNCH(kern, dim3(ho, pl.chunks), dim3(256), lds, st, L1, L2, labels, gin_hi, g, thr,
                       stats, gout, T, pl.wmax);
  });
  MSL_CHECK_LAUNCH();
  MSL_LAUNCH(k_bwd_cols, dim3(pl.cols.blocks), dim3(256), 0, st,
                     (const float*)T, g, dlow);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

template <int IW>
static int soft_fwd(const float* inputs, const float* target, int c, int hw, float ignore,
                    float ratio, float* out, float* stats, int32_t* hist, float* weights,
                    void* ws, size_t ws_bytes, msl_stream_t stream) {
  if (!inputs || !target || !out || !stats) return MSL_ERR_ARG;
  const LossPlan pl = flat_fwd_plan(c, hw, ws_bytes);
  if (pl.status != MSL_OK) return pl.status;
  hipStream_t st = as_stream(stream);
  const int nblk = pl.fwd.blocks;
  const int rec = rec_len(c);
  float* part = (float*)ws;
  MSL_DISPATCH_C(c, CM,
                 MSL_LAUNCH((k_soft_fwd<IW, CM>), dim3(nblk), dim3(256), 0, st, inputs, target,
                                    c, hw, ignore, part, rec));
  MSL_CHECK_LAUNCH();
  // plain: sum / count, nan when nothing is kept (the CE finalize); IW: sum_c w_c * sums_c / C
  MSL_LAUNCH((k_loss_finalize<IW ? K_IWENT : K_CE>), dim3(1), dim3(256), 0, st,
                     (const float*)part, nblk, rec, c, hw, ratio, out, stats, hist, weights);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

template <int IW>
static int soft_bwd(const float* inputs, const float* target, int c, int hw, float ignore,
                    const float* stats, const float* gout, float* dinputs, float* dtarget,
                    msl_stream_t stream) {
  if (!inputs || !target || !stats || !gout) return MSL_ERR_ARG;
  const LossPlan pl = flat_bwd_plan(c, hw);
  if (pl.status != MSL_OK) return pl.status;
  if (!dinputs && !dtarget) return MSL_OK;
  MSL_DISPATCH_C(c, CM,
                 MSL_LAUNCH((k_soft_bwd<IW, CM>), dim3(pl.fwd.blocks),
                                    dim3(256), 0, as_stream(stream), inputs, target, c, hw,
                                    ignore, stats, gout, dinputs, dtarget));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

}  // namespace msl

using namespace msl;

extern "C" {

size_t msl_loss_workspace(int c, int hi, int wi, int ho, int wo) {
  if (!geo_ok(c, hi, wi, ho, wo)) return 0;
  return std::max(part_bytes(c), t_bytes(c, ho, wi));
}

int msl_loss_stats_elems(void) { return kStats; }

int msl_upsample_fwd(const float* in, float* out, int c, int hi, int wi, int ho, int wo,
                     msl_stream_t stream) {
  if (!in || !out) return MSL_ERR_ARG;
  const LossPlan pl = upsample_fwd_plan(c, hi, wi, ho, wo);
  if (pl.status != MSL_OK) return pl.status;
  const Geo g = make_geo(c, hi, wi, ho, wo);
  MSL_LAUNCH(k_upsample_fwd, dim3(pl.fwd.blocks), dim3(256), 0, as_stream(stream), in, g, out);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_resize_bilinear(const float* in, float* out, int c, int hi, int wi, int ho, int wo,
                        msl_stream_t stream) {
  if (!in || !out) return MSL_ERR_ARG;
  const LossPlan pl = resize_plan(c, hi, wi, ho, wo);
  if (pl.status != MSL_OK) return pl.status;
  if (!pl.four) return msl_upsample_fwd(in, out, c, hi, wi, ho, wo, stream);
  const Geo g = make_geo(c, hi, wi, ho, wo);
  MSL_LAUNCH(k_resize_four, dim3(pl.fwd.blocks), dim3(256), 0, as_stream(stream), in, g, out);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

size_t msl_upsample_bwd_workspace(int c, int hi, int wi, int ho, int wo) {
  return t_bytes(c, ho, wi);
}

int msl_upsample_bwd(const float* gout, float* gin, int c, int hi, int wi, int ho, int wo,
                     void* ws, size_t ws_bytes, msl_stream_t stream) {
  if (!gout || c < 1 || c > kMaxC) return MSL_ERR_ARG;
  return loss_bwd<K_UPS>(nullptr, nullptr, nullptr, gout, c, hi, wi, ho, wo, 0.f, nullptr,
                         nullptr, gin, ws, ws_bytes, stream);
}

int msl_ce_up_fwd(const float* logits, const int64_t* labels, int c, int hi, int wi, int ho,
                  int wo, float* out, float* stats, void* ws, size_t ws_bytes,
                  msl_stream_t stream) {
  if (!labels) return MSL_ERR_ARG;
  return loss_fwd<K_CE>(logits, nullptr, labels, c, hi, wi, ho, wo, 0.f, 0.f, out, stats, nullptr,
                        nullptr, ws, ws_bytes, stream);
}

int msl_ce_up_bwd(const float* logits, const int64_t* labels, int c, int hi, int wi, int ho,
                  int wo, const float* stats, const float* gout, float* dlogits, void* ws,
                  size_t ws_bytes, msl_stream_t stream) {
  if (!logits || !labels || !stats || !gout) return MSL_ERR_ARG;
  return loss_bwd<K_CE>(logits, nullptr, labels, nullptr, c, hi, wi, ho, wo, 0.f, stats, gout,
                        dlogits, ws, ws_bytes, stream);
}

int msl_maxsquare_up_fwd(const float* logits, int c, int hi, int wi, int ho, int wo, float* out,
                         float* stats, void* ws, size_t ws_bytes, msl_stream_t stream) {
  return loss_fwd<K_MS>(logits, nullptr, nullptr, c, hi, wi, ho, wo, 0.f, 0.f, out, stats,
                        nullptr, nullptr, ws, ws_bytes, stream);
}

int msl_maxsquare_up_bwd(const float* logits, int c, int hi, int wi, int ho, int wo,
                         const float* stats, const float* gout, float* dlogits, void* ws,
                         size_t ws_bytes, msl_stream_t stream) {
  if (!logits || !stats || !gout) return MSL_ERR_ARG;
  return loss_bwd<K_MS>(logits, nullptr, nullptr, nullptr, c, hi, wi, ho, wo, 0.f, stats, gout,
                        dlogits, ws, ws_bytes, stream);
}

int msl_iw_maxsquare_up_fwd(const float* logits, int c, int hi, int wi, int ho, int wo,
                            float ratio, float* out, float* stats, int32_t* hist,
                            float* weights, void* ws, size_t ws_bytes, msl_stream_t stream) {
  return loss_fwd<K_IW>(logits, nullptr, nullptr, c, hi, wi, ho, wo, 0.f, ratio, out, stats, hist,
                        weights, ws, ws_bytes, stream);
}

int msl_iw_maxsquare_up_bwd(const float* logits, int c, int hi, int wi, int ho, int wo,
                            const float* stats, const float* gout, float* dlogits, void* ws,
                            size_t ws_bytes, msl_stream_t stream) {
  if (!logits || !stats || !gout) return MSL_ERR_ARG;
  return loss_bwd<K_IW>(logits, nullptr, nullptr, nullptr, c, hi, wi, ho, wo, 0.f, stats, gout,
                        dlogits, ws, ws_bytes, stream);
}

int msl_multi_ce_up_fwd(const float* logits1, const float* logits2, int c, int hi, int wi,
                        int ho, int wo, float thr, float* out, float* stats, void* ws,
                        size_t ws_bytes, msl_stream_t stream) {
  if (!logits2) return MSL_ERR_ARG;
  return loss_fwd<K_MULTI>(logits1, logits2, nullptr, c, hi, wi, ho, wo, thr, 0.f, out, stats,
                           nullptr, nullptr, ws, ws_bytes, stream);
}

int msl_multi_ce_up_bwd(const float* logits1, const float* logits2, int c, int hi, int wi,
                        int ho, int wo, float thr, const float* stats, const float* gout,
                        float* dlogits1, void* ws, size_t ws_bytes, msl_stream_t stream) {
  if (!logits1 || !logits2 || !stats || !gout) return MSL_ERR_ARG;
  return loss_bwd<K_MULTI>(logits1, logits2, nullptr, nullptr, c, hi, wi, ho, wo, thr, stats,
                           gout, dlogits1, ws, ws_bytes, stream);
}

int msl_loss_labels_up(const float* logits1, const float* logits2, int c, int hi, int wi, int ho,
                       int wo, float thr, int32_t* argmax1, int32_t* label2, msl_stream_t stream) {
  const LossPlan pl = labels_plan(c, hi, wi, ho, wo);
  if (pl.status != MSL_OK || !logits1 || (label2 && !logits2)) return MSL_ERR_ARG;
  if (!argmax1 && !label2) return MSL_OK;
  const Geo g = make_geo(c, hi, wi, ho, wo);
  const int nblk = pl.fwd.blocks;
  MSL_DISPATCH_C(c, CM,
                 MSL_LAUNCH((k_loss_labels<CM>), dim3(nblk), dim3(256), 0, as_stream(stream),
                                    logits1, logits2, g, thr, argmax1, label2));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_entropy_up_fwd(const float* logits, int c, int hi, int wi, int ho, int wo, float* out,
                       float* stats, void* ws, size_t ws_bytes, msl_stream_t stream) {
  return loss_fwd<K_ENT>(logits, nullptr, nullptr, c, hi, wi, ho, wo, 0.f, 0.f, out, stats,
                         nullptr, nullptr, ws, ws_bytes, stream);
}

int msl_entropy_up_bwd(const float* logits, int c, int hi, int wi, int ho, int wo,
                       const float* stats, const float* gout, float* dlogits, void* ws,
                       size_t ws_bytes, msl_stream_t stream) {
  if (!logits || !stats || !gout) return MSL_ERR_ARG;
  return loss_bwd<K_ENT>(logits, nullptr, nullptr, nullptr, c, hi, wi, ho, wo, 0.f, stats, gout,
                         dlogits, ws, ws_bytes, stream);
}

int msl_iw_entropy_up_fwd(const float* logits, int c, int hi, int wi, int ho, int wo, float ratio,
                          float* out, float* stats, int32_t* hist, float* weights, void* ws,
                          size_t ws_bytes, msl_stream_t stream) {
  return loss_fwd<K_IWENT>(logits, nullptr, nullptr, c, hi, wi, ho, wo, 0.f, ratio, out, stats,
                           hist, weights, ws, ws_bytes, stream);
}

int msl_iw_entropy_up_bwd(const float* logits, int c, int hi, int wi, int ho, int wo,
                          const float* stats, const float* gout, float* dlogits, void* ws,
                          size_t ws_bytes, msl_stream_t stream) {
  if (!logits || !stats || !gout) return MSL_ERR_ARG;
  return loss_bwd<K_IWENT>(logits, nullptr, nullptr, nullptr, c, hi, wi, ho, wo, 0.f, stats,
                           gout, dlogits, ws, ws_bytes, stream);
}

int msl_hard_ce_up_fwd(const float* logits, int c, int hi, int wi, int ho, int wo, float thr,
                       float* out, float* stats, void* ws, size_t ws_bytes,
                       msl_stream_t stream) {
  return loss_fwd<K_HARD>(logits, nullptr, nullptr, c, hi, wi, ho, wo, thr, 0.f, out, stats,
                          nullptr, nullptr, ws, ws_bytes, stream);
}

int msl_hard_ce_up_bwd(const float* logits, int c, int hi, int wi, int ho, int wo, float thr,
                       const float* stats, const float* gout, float* dlogits, void* ws,
                       size_t ws_bytes, msl_stream_t stream) {
  if (!logits || !stats || !gout) return MSL_ERR_ARG;
  return loss_bwd<K_HARD>(logits, nullptr, nullptr, nullptr, c, hi, wi, ho, wo, thr, stats, gout,
                          dlogits, ws, ws_bytes, stream);
}

int msl_pseudo_labels_up(const float* logits, int c, int hi, int wi, int ho, int wo, float thr,
                         int32_t* label, int32_t* argmax_logits, msl_stream_t stream) {
  const LossPlan pl = labels_plan(c, hi, wi, ho, wo);
  if (pl.status != MSL_OK || !logits) return MSL_ERR_ARG;
  if (!label && !argmax_logits) return MSL_OK;
  const Geo g = make_geo(c, hi, wi, ho, wo);
  const int nblk = pl.fwd.blocks;
  MSL_DISPATCH_C(c, CM,
                 MSL_LAUNCH((k_pseudo_labels<CM>), dim3(nblk), dim3(256), 0, as_stream(stream),
                                    logits, g, thr, label, argmax_logits));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_soft_ce_fwd(const float* inputs, const float* target, int c, int hw, float ignore,
                    float* out, float* stats, void* ws, size_t ws_bytes, msl_stream_t stream) {
  return soft_fwd<0>(inputs, target, c, hw, ignore, 0.f, out, stats, nullptr, nullptr, ws,
                     ws_bytes, stream);
}

int msl_soft_ce_bwd(const float* inputs, const float* target, int c, int hw, float ignore,
                    const float* stats, const float* gout, float* dinputs, float* dtarget,
                    msl_stream_t stream) {
  return soft_bwd<0>(inputs, target, c, hw, ignore, stats, gout, dinputs, dtarget, stream);
}

int msl_iw_soft_ce_fwd(const float* inputs, const float* target, int c, int hw, float ignore,
                       float ratio, float* out, float* stats, int32_t* hist, float* weights,
                       void* ws, size_t ws_bytes, msl_stream_t stream) {
  return soft_fwd<1>(inputs, target, c, hw, ignore, ratio, out, stats, hist, weights, ws,
                     ws_bytes, stream);
}

int msl_iw_soft_ce_bwd(const float* inputs, const float* target, int c, int hw, float ignore,
                       const float* stats, const float* gout, float* dinputs, float* dtarget,
                       msl_stream_t stream) {
  return soft_bwd<1>(inputs, target, c, hw, ignore, stats, gout, dinputs, dtarget, stream);
}

int msl_maxsquare_prob_fwd(const float* prob, int c, int hw, float* out, void* ws,
                           size_t ws_bytes, msl_stream_t stream) {
  if (!prob || !out) return MSL_ERR_ARG;
  const LossPlan pl = flat_fwd_plan(c, hw, ws_bytes);
  if (pl.status != MSL_OK) return pl.status;
  hipStream_t st = as_stream(stream);
  const int nblk = pl.fwd.blocks;
  const int rec = rec_len(c);
  float* part = (float*)ws;
  MSL_DISPATCH_C(c, CM,
                 MSL_LAUNCH((k_prob_fwd<0, CM>), dim3(nblk), dim3(256), 0, st, prob,
                                    (const int64_t*)nullptr, c, hw, part, rec));
  MSL_CHECK_LAUNCH();
  // MS finalize: -sum / (2*C*hw); stats scratch lives after the partials
  float* stats = part + (size_t)nblk * rec;
  MSL_LAUNCH((k_loss_finalize<K_MS>), dim3(1), dim3(256), 0, st, (const float*)part, nblk,
                     rec, c, hw, 0.f, out, stats, (int32_t*)nullptr, (float*)nullptr);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_maxsquare_prob_bwd(const float* prob, int c, int hw, const float* gout, float* dprob,
                           msl_stream_t stream) {
  if (!prob || !gout || !dprob) return MSL_ERR_ARG;
  const LossPlan pl = flat_bwd_plan(c, hw);
  if (pl.status != MSL_OK) return pl.status;
  MSL_DISPATCH_C(c, CM,
                 MSL_LAUNCH((k_prob_bwd<0, CM>), dim3(pl.fwd.blocks),
                                    dim3(256), 0, as_stream(stream), prob, c, hw,
                                    (const float*)nullptr, gout, dprob));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_iw_maxsquare_prob_fwd(const float* prob, const int64_t* label, int c, int hw,
                              float ratio, float* out, int32_t* hist, float* weights, void* ws,
                              size_t ws_bytes, msl_stream_t stream) {
  if (!prob || !out || !weights) return MSL_ERR_ARG;
  const LossPlan pl = flat_fwd_plan(c, hw, ws_bytes);
  if (pl.status != MSL_OK) return pl.status;
  hipStream_t st = as_stream(stream);
  const int nblk = pl.fwd.blocks;
  const int rec = rec_len(c);
  float* part = (float*)ws;
  MSL_DISPATCH_C(c, CM,
                 MSL_LAUNCH((k_prob_fwd<1, CM>), dim3(nblk), dim3(256), 0, st, prob, label,
                                    c, hw, part, rec));
  MSL_CHECK_LAUNCH();
  float* stats = part + (size_t)nblk * rec;
  MSL_LAUNCH((k_loss_finalize<K_IW>), dim3(1), dim3(256), 0, st, (const float*)part, nblk,
                     rec, c, hw, ratio, out, stats, hist, weights);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_iw_maxsquare_prob_bwd(const float* prob, int c, int hw, const float* weights,
                              const float* gout, float* dprob, msl_stream_t stream) {
  if (!prob || !weights || !gout || !dprob) return MSL_ERR_ARG;
  const LossPlan pl = flat_bwd_plan(c, hw);
  if (pl.status != MSL_OK) return pl.status;
  MSL_DISPATCH_C(c, CM,
                 MSL_LAUNCH((k_prob_bwd<1, CM>), dim3(pl.fwd.blocks),
                                    dim3(256), 0, as_stream(stream), prob, c, hw, weights, gout,
                                    dprob));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_loss_plan(int family, int c, int hi, int wi, int ho, int wo, size_t ws_bytes, msl_loss_plan_info* out) {
  if (!out || family < MSL_LOSS_UP_FWD || family > MSL_LOSS_LABELS) return MSL_ERR_ARG;
  const long long hw = (long long)ho * wo;  // the flat families' pixel count
  const bool flat = family >= MSL_LOSS_PROB_FWD && family <= MSL_LOSS_SOFT_BWD;
  LossPlan pl = {};
  if (flat && (ho < 1 || wo < 1 || hw >= (1LL << 31))) pl.status = MSL_ERR_ARG;
  else if (family == MSL_LOSS_UP_FWD) pl = up_fwd_plan(c, hi, wi, ho, wo, ws_bytes);
  else if (family == MSL_LOSS_UP_BWD || family == MSL_LOSS_UPSAMPLE_BWD) pl = up_bwd_plan(c, hi, wi, ho, wo, ws_bytes);
  else if (family == MSL_LOSS_UPSAMPLE_FWD) pl = upsample_fwd_plan(c, hi, wi, ho, wo);
  else if (family == MSL_LOSS_RESIZE) pl = resize_plan(c, hi, wi, ho, wo);
  else if (family == MSL_LOSS_LABELS) pl = labels_plan(c, hi, wi, ho, wo);
  else if (family == MSL_LOSS_PROB_FWD || family == MSL_LOSS_SOFT_FWD) pl = flat_fwd_plan(c, (int)hw, ws_bytes);
  else pl = flat_bwd_plan(c, (int)hw);
  *out = msl_loss_plan_info{};
  out->status = pl.status;
  out->ws_required = (long long)pl.ws_need;
  // a refused backward still says why: the chunks and the LDS it would have needed
  out->rows_chunks = pl.chunks;
  out->per = pl.per;
  out->rows_wmax = pl.wmax;
  out->lds_bytes = (long long)pl.lds;
  out->lds_optin = pl.optin;
  if (pl.status != MSL_OK) return MSL_OK;
  const bool by_class = family != MSL_LOSS_UPSAMPLE_FWD && family != MSL_LOSS_RESIZE;
  if (by_class) MSL_DISPATCH_C(c, CM, out->cm = CM);  // the instantiation the launch's own dispatch picks
  out->fwd_blocks = pl.fwd.blocks;
  out->fwd_trips = pl.fwd.trips;
  out->cols_blocks = pl.cols.blocks;
  out->cols_trips = pl.cols.trips;
  out->vec = pl.vec;
  out->four_tap = pl.four;
  return MSL_OK;
}

}  // extern "C"
