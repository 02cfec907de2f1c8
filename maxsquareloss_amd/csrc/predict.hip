// The evaluator's prediction kernels on gfx950: the class of every hi-res pixel straight from the
// low-resolution logits, fused with the confusion matrix and, optionally, written out as images.
//
//   msl_predict_up / msl_predict_images          tools/evaluate.py:114-141 (single scale, optional flip)
//   msl_predict_rectify                          tools/train_source.py:353-381 (Trainer.rectification)
//   msl_predict_tta / msl_predict_tta_images     multi-scale / mirror fusion over an entry table
//   msl_colorize                                 datasets/cityscapes_Dataset.py:352-377 (decode_labels)
//   msl_confidence_hist / msl_class_thresholds / msl_pseudo_classwise
//                                                class-balanced pseudo-label thresholds (--threshold_mode class)
//
// Where the class of a pixel comes from is a *source* (UpSource, RectifySource, TtaSource): it yields the
// class of (oy, ox) and, for the image maps and the confidence bodies, the winning probability.  What is
// done with the classes is a *body*: predict_classes (a class per thread-pixel, the optional int32 map) or
// predict_images (four pixels of a row per thread, the uint8 maps); both count the (label, class) pairs in
// the one confusion tile.  predict_confidence counts (class, confidence bin) pairs instead of writing, and
// predict_classwise writes the pseudo-label under a threshold per class.  A __global__ kernel is a source
// handed to a body.
#include "loss_common.h"  // the pieces shared with loss.hip; no FMA contraction in this file either

namespace msl {

// ---------------------------------------------------------------- the pixel's class: three sources
// np.argmax over the classes (k_confusion's rule, eval.hip): the lowest index wins a tie and a NaN
// counts as the maximum, so the first NaN is the answer.  Equal to argmax_first when no value is NaN.
template <int CM>
__device__ __forceinline__ int argmax_np(const float (&v)[CM], int C) {
  float best = v[0];
  int a = 0;
  bool open = !(best != best);
#pragma unroll
  for (int c = 1; c < CM; ++c)
    if (c < C && open) {
      if (v[c] != v[c]) {
        a = c;
        open = false;
      } else if (v[c] > best) {
        best = v[c];
        a = c;
      }
    }
  return a;
}

constexpr int kPredictBlocks = 1024;  // grid cap of every k_predict_* kernel (grid-stride beyond it)

// The evaluator's per-pixel decision (tools/evaluate.py:114-141).  FLIP = 0: v = up(L) at (ly, ox), the
// class is np.argmax of v.  FLIP = 1: p = (softmax(up(L))[y][x] + softmax(up(Lf))[y][Wo-1-x]) / 2, Lf the
// logits of the mirrored image (the reference flips its probabilities back after upsampling), the class
// is np.argmax of p; v is scratch.
template <int FLIP, int CM>
__device__ __forceinline__ int pixel_class(const float* __restrict__ L, const float* __restrict__ Lf,
                                           const Geo& g, const Lin& ly, int ox, float (&v)[CM],
                                           float (&p)[CM]) {
  const Lin lx = lin(ox, g.sw, g.Wi);
  up_logits<CM>(L, g, ly, lx, v);
  if (FLIP) {
    float q[CM], mx, sum;
    softmax<CM>(v, g.C, p, mx, sum);
    up_logits<CM>(Lf, g, ly, lin(g.Wo - 1 - ox, g.sw, g.Wi), v);
    softmax<CM>(v, g.C, q, mx, sum);
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < g.C) p[c] = (p[c] + q[c]) / 2.f;
    return argmax_np<CM>(p, g.C);
  }
  return argmax_np<CM>(v, g.C);
}

// A source: classify() is the class of (oy, ox); top() - after classify(), image bodies only - the
// probability of argmax_first's winner; quad_row() the row index predict_images hands to classify().  The
// body declares one pixel's registers, two arrays of kCM floats, per pixel and hands them to both: what a
// source keeps in them between classify() and top() is its own business, and one it does not touch costs
// nothing.  Sources and bodies take their arguments by value: the compiler then sees the kernel's own
// arguments, as it did when each kernel spelled its loop out.

// Single scale: pixel_class.  The winning probability is argmax_first's over p: softmax(up(L)) without
// flip (formed here, on demand), the averaged p pixel_class left with it.
template <int FLIP, int CM>
struct UpSource {
  const float* L;
  const float* Lf;
  const Geo g;
  static constexpr int kCM = CM;
  __device__ __forceinline__ int classify(int oy, int ox, float (&v)[CM], float (&p)[CM]) const {
    const Lin ly = lin(oy, g.sh, g.Hi);
    return pixel_class<FLIP, CM>(L, Lf, g, ly, ox, v, p);
  }
  __device__ __forceinline__ float top(float (&v)[CM], float (&p)[CM]) const {
    if (!FLIP) {
      float mx, sum;
      softmax<CM>(v, g.C, p, mx, sum);
    }
    float top;
    argmax_first<CM>(p, g.C, top);
    return top;
  }
  // the row's taps are the same for the four pixels of a quad, but hoisted out of its loop they are 2 * CM
  // row pointers held in VGPRs across it (168 VGPRs at C = 19 against k_predict_up's 45): recompute them
  // per pixel from a row index the compiler cannot see through
  __device__ __forceinline__ int quad_row(int oy) const {
    int oyj = oy;
    asm volatile("" : "+v"(oyj));
    return oyj;
  }
};

// Single scale without flip, then the reference's Trainer.rectification (tools/train_source.py:353-381)
// with both of its crops: inside rows [segy0, segy0 + Ho/2) the pixel (y, x) also has a prediction from
// crop k = x / (Wo/2), the half-size window magnified, stylised and forwarded on its own, at
// (2 (y - segy0), 2 (x - k Wo/2)) of its upsampled logits (the reference's nearest x1/2 of that map is
// [::2, ::2]).  The crop's class replaces the pixel's where its winning logit is strictly greater
// (numpy's >: a NaN on either side keeps the class).  v is reused for the crop: one pixel's registers.
template <int CM>
struct RectifySource {
  const float* L;
  const float* L0;
  const float* L1;
  const Geo g;
  int segy0, hh, hw;  // the band's first row; its height Ho/2 and a crop's width Wo/2
  static constexpr int kCM = CM;
  __device__ __forceinline__ int classify(int oy, int ox, float (&v)[CM], float (&)[CM]) const {
    up_logits<CM>(L, g, lin(oy, g.sh, g.Hi), lin(ox, g.sw, g.Wi), v);
    int best = argmax_np<CM>(v, g.C);
    if (oy >= segy0 && oy < segy0 + hh) {
      float m = v[0];  // the value at the class: the maximum, or the first NaN (np.amax)
#pragma unroll
      for (int c = 1; c < CM; ++c)
        if (c == best) m = v[c];
      const int k = ox >= hw ? 1 : 0;
      const int yy = 2 * (oy - segy0), xx = 2 * (ox - k * hw);
      up_logits<CM>(k ? L1 : L0, g, lin(yy, g.sh, g.Hi), lin(xx, g.sw, g.Wi), v);
      const int nb = argmax_np<CM>(v, g.C);
      float nm = v[0];
#pragma unroll
      for (int c = 1; c < CM; ++c)
        if (c == nb) nm = v[c];
      if (nm > m) best = nb;
    }
    return best;
  }
};

// One low-resolution prediction of the image: the head output at some input scale, of the image
// (mirror 0) or of its horizontal mirror (mirror 1).  sh / sw are make_geo's scales to the output size.
struct TtaEntry {
  const float* L;  // [C][Hi][Wi]
  int Hi, Wi;
  float sh, sw;
  int mirror, pad;
};

constexpr int kTtaMax = 16;

// The table of a call, a kernel argument by value (512 bytes of the kernarg segment: a captured graph
// holds its own copy).  The entry index is uniform and the entry is read where it lies: no scratch copy.
struct TtaTable {
  TtaEntry e[kTtaMax];
};

// acc = sum over the entries, in their order, of softmax(up(L_k)) at (oy, ox) - at (oy, Wo-1-ox) of a
// mirrored entry, whose probabilities the reference flips back after upsampling - and the class
// np.argmax of acc.  0 + p is p, so two entries (L, 0), (Lf, 1) give pixel_class<1>'s p + q: the same
// class, and acc / 2 its averaged probability.  One entry at a time (unroll 1): the registers are acc and
// one entry's v, p.
template <int CM>
__device__ __forceinline__ int tta_class(const TtaTable& t, int n, int C, int Wo, int oy, int ox,
                                         float (&acc)[CM]) {
#pragma unroll
  for (int c = 0; c < CM; ++c) acc[c] = 0.f;
#pragma unroll 1
  for (int k = 0; k < n; ++k) {
    const TtaEntry e = t.e[k];
    const Geo g = {C, e.Hi, e.Wi, 0, Wo, e.sh, e.sw};  // up_logits reads C, Hi, Wi
    const Lin ly = lin(oy, e.sh, e.Hi);
    const Lin lx = lin(e.mirror ? Wo - 1 - ox : ox, e.sw, e.Wi);
    float v[CM], p[CM], mx, sum;
    up_logits<CM>(e.L, g, ly, lx, v);
    softmax<CM>(v, C, p, mx, sum);
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) acc[c] = acc[c] + p[c];
  }
  return argmax_np<CM>(acc, C);
}

// An entry table: tta_class.  The winning probability is acc at its first maximum divided by n (exact for
// n = 2: UpSource<1>'s averaged p).
template <int CM>
struct TtaSource {
  const TtaTable& t;
  int n, C, Wo;
  static constexpr int kCM = CM;
  __device__ __forceinline__ int classify(int oy, int ox, float (&acc)[CM], float (&)[CM]) const {
    return tta_class<CM>(t, n, C, Wo, oy, ox, acc);
  }
  __device__ __forceinline__ float top(float (&acc)[CM], float (&)[CM]) const {
    float top;
    argmax_first<CM>(acc, C, top);
    return top / (float)n;
  }
  __device__ __forceinline__ int quad_row(int oy) const { return oy; }
};

// ---------------------------------------------------------------- the confusion tile
// The (gt, class) cells of the confusion matrix (utils/eval.py:109-115), k_confusion's histogram: per-block
// LDS counts h[cc = C*C], integer atomics on the uint64 matrix - exact in any order.  Zero, a barrier of the
// caller's (the image body shares it with its table loads), count per pixel, flush.
__device__ __forceinline__ void tile_zero(unsigned int* h, int cc) {
  for (int i = threadIdx.x; i < cc; i += 256) h[i] = 0u;
}

__device__ __forceinline__ void tile_count(unsigned int* h, const long long* __restrict__ label, int px,
                                           int C, int best) {
  const long long y = label[px];
  if (y >= 0 && y < C) atomicAdd(&h[(int)y * C + best], 1u);
}

__device__ __forceinline__ void tile_flush(const unsigned int* h, int cc, unsigned long long* __restrict__ cm) {
  __syncthreads();
  for (int i = threadIdx.x; i < cc; i += 256)
    if (h[i]) atomicAdd(&cm[i], (unsigned long long)h[i]);
}

// ---------------------------------------------------------------- body: a class per pixel
// The class of every pixel of Ho x Wo, one pixel per thread and trip.  label / cm and arg are nullable
// (the host requires one of them).
template <class Source>
__device__ __forceinline__ void predict_classes(const Source src, int C, int Ho, int Wo,
                                                const long long* __restrict__ label,
                                                unsigned long long* __restrict__ cm,
                                                int32_t* __restrict__ arg) {
  __shared__ unsigned int h[kMaxC * kMaxC];
  const int cc = C * C;
  if (cm) {
    tile_zero(h, cc);
    __syncthreads();
  }
  const long long npx = (long long)Ho * Wo;  // < 2^31 (geo_ok); the stride may step past it
  for (long long pp = blockIdx.x * 256LL + threadIdx.x; pp < npx; pp += (long long)gridDim.x * 256) {
    const int px = (int)pp;
    const int oy = px / Wo, ox = px - oy * Wo;
    float v[Source::kCM], p[Source::kCM];
    const int best = src.classify(oy, ox, v, p);
    if (arg) arg[px] = best;
    if (cm) tile_count(h, label, px, C, best);
  }
  if (cm) tile_flush(h, cc, cm);
}

// ---------------------------------------------------------------- body: prediction images
struct ImgOut {
  uint8_t* cls;     // [Ho*Wo]   the class (predict_classes' arg as a byte)
  uint8_t* ids;     // [Ho*Wo]   id_lut[class]
  uint8_t* color;   // [Ho*Wo*3] palette[class], HWC
  uint8_t* conf;    // [Ho*Wo*3] shade[bucket of the winning probability][class], black below 0.5
  uint8_t* pseudo;  // [Ho*Wo]   class where the winning probability > thr, else 255
};

__device__ __forceinline__ unsigned int rgb24(const uint8_t* __restrict__ t, int i) {
  return (unsigned int)t[3 * i] | ((unsigned int)t[3 * i + 1] << 8) | ((unsigned int)t[3 * i + 2] << 16);
}

// four 24-bit pixels -> the three dwords of their 12 bytes
__device__ __forceinline__ void store_rgb4(uint8_t* __restrict__ out, long long quad, unsigned int a,
                                           unsigned int b, unsigned int c, unsigned int d) {
  unsigned int* o = reinterpret_cast<unsigned int*>(out) + 3 * quad;
  o[0] = a | (b << 24);
  o[1] = (b >> 8) | (c << 16);
  o[2] = (c >> 16) | (d << 8);
}

__device__ __forceinline__ void store_rgb1(uint8_t* __restrict__ out, long long px, unsigned int a) {
  out[3 * px] = (uint8_t)a;
  out[3 * px + 1] = (uint8_t)(a >> 8);
  out[3 * px + 2] = (uint8_t)(a >> 16);
}

// The source's decision written as images.  A thread takes four consecutive pixels of one row (a
// quad), one after the other (the registers are those of one pixel), and keeps their bytes in
// registers: with VEC (Wo % 4 == 0 and dword-aligned outputs, so quad q is bytes [4q, 4q+4) of a byte
// map and [12q, 12q+12) of an RGB map) it stores one dword per byte map and three per RGB map; without,
// rows are not dword-aligned, the last quad of a row is partial and every pixel stores its own bytes.
// The tables sit in LDS as one dword per entry.  The winning probability is the source's top() and the
// pseudo-label decision hard_label's: the class where top > thr.
template <class Source>
__device__ __forceinline__ void predict_images(const Source src, int C, int Ho, int Wo,
                                               const long long* __restrict__ label,
                                               unsigned long long* __restrict__ cm, float thr,
                                               const uint8_t* __restrict__ id_lut,
                                               const uint8_t* __restrict__ palette,
                                               const uint8_t* __restrict__ shade, const ImgOut o, int vec) {
  __shared__ unsigned int h[kMaxC * kMaxC];
  __shared__ unsigned int t_pal[kMaxC], t_id[kMaxC], t_shade[4 * kMaxC];
  const int cc = C * C;
  if (cm) tile_zero(h, cc);
  if ((int)threadIdx.x < C) {
    t_pal[threadIdx.x] = palette ? rgb24(palette, threadIdx.x) : 0u;
    t_id[threadIdx.x] = id_lut ? id_lut[threadIdx.x] : 0u;
  }
  if ((int)threadIdx.x < 4 * C) t_shade[threadIdx.x] = shade ? rgb24(shade, threadIdx.x) : 0u;
  __syncthreads();
  const bool want_p = o.conf || o.pseudo;
  const int nq = (Wo + 3) >> 2;                   // quads per row
  const long long nquad = (long long)Ho * nq;     // < 2^31 (geo_ok)
  for (long long qq = blockIdx.x * 256LL + threadIdx.x; qq < nquad; qq += (long long)gridDim.x * 256) {
    const int q = (int)qq;
    const int oy = q / nq, ox0 = (q - oy * nq) << 2;
    const int row = oy * Wo;
    unsigned int w_cls = 0u, w_ids = 0u, w_ps = 0u;
    unsigned int c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u, f0 = 0u, f1 = 0u, f2 = 0u, f3 = 0u;
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      const int ox = ox0 + j;
      if (ox >= Wo) break;  // never with vec
      float v[Source::kCM], p[Source::kCM];
      const int best = src.classify(src.quad_row(oy), ox, v, p);
      const int px = row + ox;
      if (cm) tile_count(h, label, px, C, best);
      unsigned int ps = 255u, cf = 0u;
      if (want_p) {
        const float top = src.top(v, p);
        if (top > thr) ps = (unsigned int)best;
        const int bucket = top > 0.9f ? 0 : top > 0.8f ? 1 : top > 0.7f ? 2 : top > 0.5f ? 3 : -1;
        if (bucket >= 0) cf = t_shade[bucket * C + best];
      }
      const unsigned int col = t_pal[best], id = t_id[best];
      if (vec) {
        const int sh = 8 * j;
        w_cls |= (unsigned int)best << sh;
        w_ids |= id << sh;
        w_ps |= ps << sh;
        c0 = j == 0 ? col : c0;
        c1 = j == 1 ? col : c1;
        c2 = j == 2 ? col : c2;
        c3 = j == 3 ? col : c3;
        f0 = j == 0 ? cf : f0;
        f1 = j == 1 ? cf : f1;
        f2 = j == 2 ? cf : f2;
        f3 = j == 3 ? cf : f3;
      } else {
        if (o.cls) o.cls[px] = (uint8_t)best;
        if (o.ids) o.ids[px] = (uint8_t)id;
        if (o.pseudo) o.pseudo[px] = (uint8_t)ps;
        if (o.color) store_rgb1(o.color, px, col);
        if (o.conf) store_rgb1(o.conf, px, cf);
      }
    }
    if (vec) {  // row + ox0 == 4 * q
      if (o.cls) reinterpret_cast<unsigned int*>(o.cls)[q] = w_cls;
      if (o.ids) reinterpret_cast<unsigned int*>(o.ids)[q] = w_ids;
      if (o.pseudo) reinterpret_cast<unsigned int*>(o.pseudo)[q] = w_ps;
      if (o.color) store_rgb4(o.color, q, c0, c1, c2, c3);
      if (o.conf) store_rgb4(o.conf, q, f0, f1, f2, f3);
    }
  }
  if (cm) tile_flush(h, cc, cm);
}

// ---------------------------------------------------------------- body: the confidence histogram
// One add of a wave's (class, bin) keys into the block's LDS tile; key < 0 adds nothing.  On a real target
// image most pixels of a wave are road or sky in the top bin: 64 lanes on one LDS word serialise.  So the
// wave first merges: twice, the lowest pending lane's key is broadcast, the lanes that hold it are counted
// with a ballot and that lane adds the count once.  What is still pending after the two rounds - the
// spread-out rest - adds 1 per lane.  Every lane of the wave calls this, converged.
constexpr int kMergeRounds = 2;
__device__ __forceinline__ void tile_add_merged(unsigned int* h, int key) {
  const int lane = threadIdx.x & 63;
  bool pending = key >= 0;
#pragma unroll
  for (int r = 0; r < kMergeRounds; ++r) {
    const unsigned long long act = __ballot(pending);
    if (act == 0ull) break;  // wave-uniform
    const int lead = __ffsll((long long)act) - 1;
    const int k0 = __shfl(key, lead, 64);
    const bool hit = pending && key == k0;
    const unsigned long long m = __ballot(hit);
    if (lane == lead) atomicAdd(&h[k0], (unsigned int)__popcll(m));
    pending = pending && !hit;
  }
  if (pending) atomicAdd(&h[key], 1u);
}

// hist[class][bin of the source's top()] += 1 over the pixels of Ho x Wo, one pixel per thread and trip
// (neighbouring lanes hold neighbouring pixels: what the merge above feeds on).  The tile h[C * bins] is
// the launch's dynamic LDS; a NaN pixel (top != top) is not counted.  The trip count is the wave's, so the
// merge's ballots see every lane.
template <class Source>
__device__ __forceinline__ void predict_confidence(const Source src, int C, int Ho, int Wo, int bins,
                                                   unsigned long long* __restrict__ hist) {
  extern __shared__ unsigned int h_conf[];
  const int cells = C * bins;
  tile_zero(h_conf, cells);
  __syncthreads();
  const long long npx = (long long)Ho * Wo;  // < 2^31 (geo_ok)
  const long long stride = (long long)gridDim.x * 256;
  const long long wave0 = blockIdx.x * 256LL + (threadIdx.x & ~63);  // the wave's first pixel of trip 0
  const float fb = (float)bins;
  for (long long base = wave0; base < npx; base += stride) {
    const long long pp = base + (threadIdx.x & 63);
    int key = -1;
    if (pp < npx) {
      const int px = (int)pp;
      const int oy = px / Wo, ox = px - oy * Wo;
      float v[Source::kCM], p[Source::kCM];
      const int best = src.classify(oy, ox, v, p);
      const float top = src.top(v, p);
      if (!(top != top)) {
        const int b = max(0, min(bins - 1, (int)(top * fb)));
        key = best * bins + b;
      }
    }
    tile_add_merged(h_conf, key);
  }
  tile_flush(h_conf, cells, hist);
}

// ---------------------------------------------------------------- body: per-class pseudo-labels
// predict_images' pseudo map with a threshold per class, read from device memory (a captured launch
// picks up new values): label[px] = top > thr[class] ? class : -1 as int64, pseudo[px] the same with 255
// for -1.  The quad layout and alignment rule of predict_images for the byte map; the thresholds sit in LDS.
template <class Source>
__device__ __forceinline__ void predict_classwise(const Source src, int C, int Ho, int Wo,
                                                  const float* __restrict__ thr, long long* __restrict__ label,
                                                  uint8_t* __restrict__ pseudo, int vec) {
  __shared__ float t_thr[kMaxC];
  if ((int)threadIdx.x < C) t_thr[threadIdx.x] = thr[threadIdx.x];
  __syncthreads();
  const int nq = (Wo + 3) >> 2;                // quads per row
  const long long nquad = (long long)Ho * nq;  // < 2^31 (geo_ok)
  for (long long qq = blockIdx.x * 256LL + threadIdx.x; qq < nquad; qq += (long long)gridDim.x * 256) {
    const int q = (int)qq;
    const int oy = q / nq, ox0 = (q - oy * nq) << 2;
    const int row = oy * Wo;
    unsigned int w_ps = 0u;
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      const int ox = ox0 + j;
      if (ox >= Wo) break;  // never with vec
      float v[Source::kCM], p[Source::kCM];
      const int best = src.classify(src.quad_row(oy), ox, v, p);
      const float top = src.top(v, p);
      const bool keep = top > t_thr[best];  // strict; false for a NaN
      const int px = row + ox;
      if (label) label[px] = keep ? (long long)best : -1LL;
      const unsigned int ps = keep ? (unsigned int)best : 255u;
      if (vec)
        w_ps |= ps << (8 * j);
      else if (pseudo)
        pseudo[px] = (uint8_t)ps;
    }
    if (vec && pseudo) reinterpret_cast<unsigned int*>(pseudo)[q] = w_ps;  // row + ox0 == 4 * q
  }
}

// ---------------------------------------------------------------- class-balanced thresholds
// Suffix sums over the 64 lanes of a wave: lane l receives the sum of x over lanes >= l.
__device__ __forceinline__ unsigned long long wave_suffix_sum(unsigned long long x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long t = __shfl_down(x, o, 64);
    if (lane + o < 64) x += t;
  }
  return x;
}

// One threshold per class from its own confidence histogram (CBST / BDL): the largest bin edge q = b* / bins
// that still keeps `portion` of the class's pixels at or above it, capped at thr_max.  One block; a wave per
// class, lane l holding the bins [l * per, (l + 1) * per).  All integer sums: exact.
__global__ void __launch_bounds__(256) k_class_thresholds(const unsigned long long* __restrict__ hist, int C, int bins,
                                                          double portion, float thr_max, float* __restrict__ thr,
                                                          unsigned long long* __restrict__ kept) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = bins >> 6 > 0 ? bins >> 6 : 1;  // bins is a power of two >= 16
  const int lo = lane * per, hi = min(bins, lo + per);  // lo >= bins: an idle lane (bins < 64)
  for (int k = wave; k < C; k += 4) {
    const unsigned long long* hk = hist + (long long)k * bins;
    unsigned long long s = 0ull;
    for (int b = lo; b < hi; ++b) s += hk[b];
    const unsigned long long suf = wave_suffix_sum(s);  // bins >= lo
    const unsigned long long n = __shfl(suf, 0, 64);
    const unsigned long long need = (unsigned long long)ceil(portion * (double)n);
    int bstar = bins;  // need == 0: q = 1
    if (need > 0ull) {
      const unsigned long long ok = __ballot(suf >= need);  // a prefix of the lanes: suf falls with the lane
      bstar = 0;                                            // need > n (n above 2^53 only): keep everything
      if (ok) {
        const int owner = 63 - __clzll((long long)ok);  // the last lane whose suffix still reaches need
        int mine = 0;
        if (lane == owner) {
          unsigned long long run = suf - s;  // the bins above this lane's
          for (int b = hi - 1; b >= lo; --b) {
            run += hk[b];
            if (run >= need) {
              mine = b;
              break;
            }
          }
        }
        bstar = __shfl(mine, owner, 64);
      }
    }
    const float q = (float)bstar / (float)bins;
    const float t = n == 0ull ? thr_max : fminf(thr_max, q);
    if (lane == 0) thr[k] = t;
    if (kept) {
      const int b0 = (int)(t * (float)bins);  // floor: t >= 0
      unsigned long long ks = 0ull;
      for (int b = max(lo, b0); b < hi; ++b) ks += hk[b];
      ks = wave_suffix_sum(ks);
      if (lane == 0) kept[k] = ks;
    }
  }
}

// ---------------------------------------------------------------- the kernels: a source and a body
template <int FLIP, int CM>
__global__ void __launch_bounds__(256) k_confidence_hist(const float* __restrict__ L, const float* __restrict__ Lf,
                                                          Geo g, int bins, unsigned long long* __restrict__ hist) {
  predict_confidence(UpSource<FLIP, CM>{L, Lf, g}, g.C, g.Ho, g.Wo, bins, hist);
}

template <int CM>
__global__ void __launch_bounds__(256) k_confidence_hist_tta(TtaTable t, int n, int C, int Ho, int Wo, int bins,
                                                              unsigned long long* __restrict__ hist) {
  predict_confidence(TtaSource<CM>{t, n, C, Wo}, C, Ho, Wo, bins, hist);
}

template <int FLIP, int CM>
__global__ void __launch_bounds__(256) k_pseudo_classwise(const float* __restrict__ L, const float* __restrict__ Lf,
                                                           Geo g, const float* __restrict__ thr,
                                                           long long* __restrict__ label, uint8_t* __restrict__ pseudo,
                                                           int vec) {
  predict_classwise(UpSource<FLIP, CM>{L, Lf, g}, g.C, g.Ho, g.Wo, thr, label, pseudo, vec);
}

template <int CM>
__global__ void __launch_bounds__(256) k_pseudo_classwise_tta(TtaTable t, int n, int C, int Ho, int Wo,
                                                               const float* __restrict__ thr,
                                                               long long* __restrict__ label,
                                                               uint8_t* __restrict__ pseudo, int vec) {
  predict_classwise(TtaSource<CM>{t, n, C, Wo}, C, Ho, Wo, thr, label, pseudo, vec);
}

template <int FLIP, int CM>
__global__ void __launch_bounds__(256) k_predict_up(const float* __restrict__ L, const float* __restrict__ Lf, Geo g,
                                                     const long long* __restrict__ label,
                                                     unsigned long long* __restrict__ cm, int32_t* __restrict__ arg) {
  predict_classes(UpSource<FLIP, CM>{L, Lf, g}, g.C, g.Ho, g.Wo, label, cm, arg);
}

template <int CM>
__global__ void __launch_bounds__(256) k_predict_rectify(const float* __restrict__ L, const float* __restrict__ L0,
                                                          const float* __restrict__ L1, Geo g, int segy0,
                                                          const long long* __restrict__ label,
                                                          unsigned long long* __restrict__ cm,
                                                          int32_t* __restrict__ arg) {
  predict_classes(RectifySource<CM>{L, L0, L1, g, segy0, g.Ho >> 1, g.Wo >> 1}, g.C, g.Ho, g.Wo, label, cm, arg);
}

template <int CM>
__global__ void __launch_bounds__(256) k_predict_tta(TtaTable t, int n, int C, int Ho, int Wo,
                                                      const long long* __restrict__ label,
                                                      unsigned long long* __restrict__ cm, int32_t* __restrict__ arg) {
  predict_classes(TtaSource<CM>{t, n, C, Wo}, C, Ho, Wo, label, cm, arg);
}

template <int FLIP, int CM>
__global__ void __launch_bounds__(256) k_predict_images(const float* __restrict__ L, const float* __restrict__ Lf,
                                                         Geo g, const long long* __restrict__ label,
                                                         unsigned long long* __restrict__ cm, float thr,
                                                         const uint8_t* __restrict__ id_lut,
                                                         const uint8_t* __restrict__ palette,
                                                         const uint8_t* __restrict__ shade, ImgOut o, int vec) {
  predict_images(UpSource<FLIP, CM>{L, Lf, g}, g.C, g.Ho, g.Wo, label, cm, thr, id_lut, palette, shade, o, vec);
}

template <int CM>
__global__ void __launch_bounds__(256) k_predict_tta_images(TtaTable t, int n, int C, int Ho, int Wo,
                                                             const long long* __restrict__ label,
                                                             unsigned long long* __restrict__ cm, float thr,
                                                             const uint8_t* __restrict__ id_lut,
                                                             const uint8_t* __restrict__ palette,
                                                             const uint8_t* __restrict__ shade, ImgOut o, int vec) {
  predict_images(TtaSource<CM>{t, n, C, Wo}, C, Ho, Wo, label, cm, thr, id_lut, palette, shade, o, vec);
}

// decode_labels (datasets/cityscapes_Dataset.py:352-377) on the device: out[px] = palette[cls[px]], black
// outside [0, C).  A thread takes four pixels: three dword stores with VEC (dword-aligned out), else
// bytes; the last quad may be partial.
constexpr int kColorizeMaxC = 256;
template <typename T>
__global__ void __launch_bounds__(256) k_colorize(const T* __restrict__ cls, long long npx,
                                                   const uint8_t* __restrict__ palette, int C,
                                                   uint8_t* __restrict__ out, int vec) {
  __shared__ unsigned int t_pal[kColorizeMaxC];
  for (int i = threadIdx.x; i < C; i += 256) t_pal[i] = rgb24(palette, i);
  __syncthreads();
  const long long nquad = (npx + 3) >> 2;
  for (long long q = blockIdx.x * 256LL + threadIdx.x; q < nquad; q += (long long)gridDim.x * 256) {
    unsigned int col[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long px = 4 * q + j;
      col[j] = 0u;
      if (px < npx) {
        const long long k = (long long)cls[px];
        if (k >= 0 && k < C) col[j] = t_pal[(int)k];
      }
    }
    if (vec && 4 * q + 3 < npx) {
      store_rgb4(out, q, col[0], col[1], col[2], col[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * q + j < npx) store_rgb1(out, 4 * q + j, col[j]);
    }
  }
}

// ---------------------------------------------------------------- the failure maps of one image
// Per-image analysis (the reference's tools/analysis.py:208-227): the label, the prediction and the input of an
// image whose MIoU fell below the threshold, as RGB maps, plus an error map.  Whether to write at all was
// decided on the device by msl_image_metrics (eval.hip): with `state` every thread reads state[1] first and
// returns on 0 before any other load or store; otherwise the maps go to slot state[2] of the ring.  The
// four-pixels-per-thread layout of predict_images: with VEC a float4 per input plane, a dword of classes and
// three dwords per RGB map, without it every pixel loads and stores its own.
struct MapsOut {
  uint8_t* label;  // [H*W*3] palette[label], black outside [0, C)  (decode_labels)
  uint8_t* pred;   // [H*W*3] palette[cls]
  uint8_t* input;  // [H*W*3] the uint8 RGB image the network input was made from  (recover_input)
  uint8_t* error;  // [H*W*3] black where unlabelled, the dimmed input where right, palette[cls] where wrong
};

// one byte of utils/images.py:recover_input: clamp(rint(x + mean), 0, 255), round half to even, NaN -> 0
__device__ __forceinline__ unsigned int input_byte(float x, float m) {
  const float v = rintf(x + m);
  return v >= 0.f ? (unsigned int)fminf(v, 255.f) : 0u;
}

__global__ void __launch_bounds__(256) k_analysis_maps(const float* __restrict__ x, const float* __restrict__ mean,
                                                       const long long* __restrict__ label,
                                                       const uint8_t* __restrict__ cls,
                                                       const uint8_t* __restrict__ palette, int C, int H, int W,
                                                       const int* __restrict__ state, long long slot_stride,
                                                       MapsOut o, int vec) {
  long long off = 0;
  if (state) {
    if (state[1] == 0) return;  // the device-side gate: uniform over the grid
    off = (long long)state[2] * slot_stride;
  }
  __shared__ unsigned int t_pal[kMaxC];
  if ((int)threadIdx.x < C) t_pal[threadIdx.x] = palette ? rgb24(palette, threadIdx.x) : 0u;
  __syncthreads();
  uint8_t* const o_label = o.label ? o.label + off : nullptr;
  uint8_t* const o_pred = o.pred ? o.pred + off : nullptr;
  uint8_t* const o_input = o.input ? o.input + off : nullptr;
  uint8_t* const o_error = o.error ? o.error + off : nullptr;
  // what the requested maps read (the host checked that it is there): nothing else is loaded or looked up
  const bool want_in = o.input || o.error, want_lab = o.label || o.error, want_cls = o.pred || o.error;
  float m[3] = {0.f, 0.f, 0.f};
  if (want_in) {
    m[0] = mean[0];
    m[1] = mean[1];
    m[2] = mean[2];
  }
  const long long plane = (long long)H * W;    // < 2^31 (the host checks)
  const int nq = (W + 3) >> 2;                 // quads per row
  const long long nquad = (long long)H * nq;
  for (long long qq = blockIdx.x * 256LL + threadIdx.x; qq < nquad; qq += (long long)gridDim.x * 256) {
    const int oy = (int)(qq / nq), ox0 = (int)(qq - (long long)oy * nq) << 2;
    const long long px0 = (long long)oy * W + ox0;
    const int n = vec ? 4 : min(4, W - ox0);
    float xv[3][4];
    unsigned int cw = 0u;
    if (vec) {  // px0 == 4 * qq
      if (want_in) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float4 f = *reinterpret_cast<const float4*>(x + k * plane + px0);
          xv[k][0] = f.x;
          xv[k][1] = f.y;
          xv[k][2] = f.z;
          xv[k][3] = f.w;
        }
      }
      if (want_cls) cw = *reinterpret_cast<const unsigned int*>(cls + px0);
    }
    unsigned int lc[4], pc[4], ic[4], ec[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lc[j] = pc[j] = ic[j] = ec[j] = 0u;
      if (j < n) {
        const long long px = px0 + j;
        unsigned int cb = (cw >> (8 * j)) & 255u;
        if (!vec) {
          if (want_cls) cb = cls[px];
          if (want_in) {
            xv[0][j] = x[px];
            xv[1][j] = x[plane + px];
            xv[2][j] = x[2 * plane + px];
          }
        }
        const long long y = want_lab ? label[px] : -1;
        const bool valid = y >= 0 && y < C;
        lc[j] = valid ? t_pal[(int)y] : 0u;
        if (want_cls) pc[j] = (int)cb < C ? t_pal[cb] : 0u;
        if (want_in)  // RGB = channels 2, 1, 0 of the BGR input
          ic[j] = input_byte(xv[2][j], m[2]) | (input_byte(xv[1][j], m[1]) << 8) | (input_byte(xv[0][j], m[0]) << 16);
        if (o.error) ec[j] = !valid ? 0u : (long long)cb == y ? (ic[j] >> 1) & 0x7f7f7fu : pc[j];
      }
    }
    if (vec) {
      if (o_label) store_rgb4(o_label, qq, lc[0], lc[1], lc[2], lc[3]);
      if (o_pred) store_rgb4(o_pred, qq, pc[0], pc[1], pc[2], pc[3]);
      if (o_input) store_rgb4(o_input, qq, ic[0], ic[1], ic[2], ic[3]);
      if (o_error) store_rgb4(o_error, qq, ec[0], ec[1], ec[2], ec[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < n) {
          if (o_label) store_rgb1(o_label, px0 + j, lc[j]);
          if (o_pred) store_rgb1(o_pred, px0 + j, pc[j]);
          if (o_input) store_rgb1(o_input, px0 + j, ic[j]);
          if (o_error) store_rgb1(o_error, px0 + j, ec[j]);
        }
    }
  }
}

// ---------------------------------------------------------------- host helpers
// What a call computes into: label and confusion go together, and there is a matrix or an output.
static bool sinks_ok(const long long* label, const unsigned long long* confusion, bool any_out) {
  return (label == nullptr) == (confusion == nullptr) && (confusion || any_out);
}

// ... and every image map that reads a table has its table
static bool image_sinks_ok(const long long* label, const unsigned long long* confusion, const ImgOut& o,
                           const uint8_t* id_lut, const uint8_t* palette, const uint8_t* shade) {
  const bool any_out = o.cls || o.ids || o.color || o.conf || o.pseudo;
  return sinks_ok(label, confusion, any_out) && !(o.ids && !id_lut) && !(o.color && !palette) &&
         !(o.conf && !shade);
}

static bool dword_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// predict_images' VEC: whole quads per row and every map (a null one too) on a dword
static int image_vec(const ImgOut& o, int wo) {
  return wo % 4 == 0 && dword_aligned(o.cls) && dword_aligned(o.ids) && dword_aligned(o.color) &&
         dword_aligned(o.conf) && dword_aligned(o.pseudo);
}

static int class_blocks(int ho, int wo) { return std::min(kPredictBlocks, cdiv((long long)ho * wo, 256)); }
static int image_blocks(int ho, int wo) {
  return std::min(kPredictBlocks, cdiv((long long)ho * cdiv(wo, 4), 256));
}

// predict_confidence: a power-of-two bin count (b / bins is then exact in fp32) whose tile fits 64 KB of LDS
constexpr int kHistMaxCells = 16384;
static bool hist_ok(int c, int bins) {
  return bins >= 16 && bins <= 1024 && (bins & (bins - 1)) == 0 && c >= 1 && c * bins <= kHistMaxCells;
}
// one pixel per thread and trip, two trips until the grid cap binds: the zero and flush of the tile are paid once
// per 512 pixels.  Measured at 1024 x 512 (profiles/pseudo_thresholds_times.txt): more pixels per block merge more
// per flush but leave compute units idle - 2048 per block takes 1.4x to 1.7x the time of 1024, 512 takes 0.8x to 1.0x
static int hist_blocks(int ho, int wo) { return std::min(kPredictBlocks, cdiv((long long)ho * wo, 512)); }

// the caller's entries -> the kernel's table; each entry's scales are make_geo's for its own size
static bool make_tta(const msl_tta_entry* entries, int n, int c, int ho, int wo, TtaTable* t) {
  if (!entries || n < 1 || n > kTtaMax) return false;
  *t = TtaTable{};
  for (int k = 0; k < n; ++k) {
    const msl_tta_entry& e = entries[k];
    if (!e.logits || !geo_ok(c, e.hi, e.wi, ho, wo) || (e.mirror != 0 && e.mirror != 1)) return false;
    const Geo g = make_geo(c, e.hi, e.wi, ho, wo);
    t->e[k] = {e.logits, e.hi, e.wi, g.sh, g.sw, e.mirror, 0};
  }
  return true;
}

}  // namespace msl

using namespace msl;

extern "C" {

int msl_predict_up(const float* logits, const float* logits_flip, int c, int hi, int wi, int ho, int wo,
                   const long long* label, unsigned long long* confusion, int32_t* argmax_out,
                   msl_stream_t stream) {
  if (!geo_ok(c, hi, wi, ho, wo) || !logits || !sinks_ok(label, confusion, argmax_out)) return MSL_ERR_ARG;
  const Geo g = make_geo(c, hi, wi, ho, wo);
  const int nblk = class_blocks(ho, wo);
  hipStream_t st = as_stream(stream);
  if (logits_flip)
    MSL_DISPATCH_C(c, CM,
                   MSL_LAUNCH((k_predict_up<1, CM>), dim3(nblk), dim3(256), 0, st, logits, logits_flip,
                              g, label, confusion, argmax_out));
  else
    MSL_DISPATCH_C(c, CM,
                   MSL_LAUNCH((k_predict_up<0, CM>), dim3(nblk), dim3(256), 0, st, logits, logits_flip,
                              g, label, confusion, argmax_out));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_predict_rectify(const float* base, const float* crop0, const float* crop1, int c, int hi, int wi, int ho,
                        int wo, int segy0, const long long* label, unsigned long long* confusion,
                        int32_t* argmax_out, msl_stream_t stream) {
  if (!geo_ok(c, hi, wi, ho, wo) || !base || !crop0 || !crop1 || !sinks_ok(label, confusion, argmax_out) ||
      (ho & 1) || (wo & 1) || segy0 < 0 || segy0 > ho / 2)
    return MSL_ERR_ARG;
  const Geo g = make_geo(c, hi, wi, ho, wo);
  MSL_DISPATCH_C(c, CM,
                 MSL_LAUNCH((k_predict_rectify<CM>), dim3(class_blocks(ho, wo)), dim3(256), 0, as_stream(stream),
                            base, crop0, crop1, g, segy0, label, confusion, argmax_out));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_predict_images(const float* logits, const float* logits_flip, int c, int hi, int wi, int ho, int wo,
                       const long long* label, unsigned long long* confusion, float thr,
                       const uint8_t* id_lut, const uint8_t* palette, const uint8_t* shade,
                       uint8_t* class_out, uint8_t* ids_out, uint8_t* color_out, uint8_t* conf_out,
                       uint8_t* pseudo_out, msl_stream_t stream) {
  const ImgOut o = {class_out, ids_out, color_out, conf_out, pseudo_out};
  if (!geo_ok(c, hi, wi, ho, wo) || !logits || !image_sinks_ok(label, confusion, o, id_lut, palette, shade))
    return MSL_ERR_ARG;
  const Geo g = make_geo(c, hi, wi, ho, wo);
  const int vec = image_vec(o, wo);
  const int nblk = image_blocks(ho, wo);
  hipStream_t st = as_stream(stream);
  if (logits_flip)
    MSL_DISPATCH_C(c, CM,
                   MSL_LAUNCH((k_predict_images<1, CM>), dim3(nblk), dim3(256), 0, st, logits, logits_flip,
                              g, label, confusion, thr, id_lut, palette, shade, o, vec));
  else
    MSL_DISPATCH_C(c, CM,
                   MSL_LAUNCH((k_predict_images<0, CM>), dim3(nblk), dim3(256), 0, st, logits, logits_flip,
                              g, label, confusion, thr, id_lut, palette, shade, o, vec));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_predict_tta_max_entries(void) { return kTtaMax; }

int msl_predict_tta(const msl_tta_entry* entries, int n, int c, int ho, int wo, const long long* label,
                    unsigned long long* confusion, int32_t* argmax_out, msl_stream_t stream) {
  TtaTable t;
  if (!geo_ok(c, 1, 1, ho, wo) || !make_tta(entries, n, c, ho, wo, &t) ||
      !sinks_ok(label, confusion, argmax_out))
    return MSL_ERR_ARG;
  MSL_DISPATCH_C(c, CM,
                 MSL_LAUNCH((k_predict_tta<CM>), dim3(class_blocks(ho, wo)), dim3(256), 0, as_stream(stream), t,
                            n, c, ho, wo, label, confusion, argmax_out));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_predict_tta_images(const msl_tta_entry* entries, int n, int c, int ho, int wo, const long long* label,
                           unsigned long long* confusion, float thr, const uint8_t* id_lut,
                           const uint8_t* palette, const uint8_t* shade, uint8_t* class_out, uint8_t* ids_out,
                           uint8_t* color_out, uint8_t* conf_out, uint8_t* pseudo_out, msl_stream_t stream) {
  TtaTable t;
  const ImgOut o = {class_out, ids_out, color_out, conf_out, pseudo_out};
  if (!geo_ok(c, 1, 1, ho, wo) || !make_tta(entries, n, c, ho, wo, &t) ||
      !image_sinks_ok(label, confusion, o, id_lut, palette, shade))
    return MSL_ERR_ARG;
  const int vec = image_vec(o, wo);
  MSL_DISPATCH_C(c, CM,
                 MSL_LAUNCH((k_predict_tta_images<CM>), dim3(image_blocks(ho, wo)), dim3(256), 0,
                            as_stream(stream), t, n, c, ho, wo, label, confusion, thr, id_lut, palette, shade, o,
                            vec));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_confidence_hist(const float* logits, const float* logits_flip, int c, int hi, int wi, int ho, int wo,
                        int bins, unsigned long long* hist, msl_stream_t stream) {
  if (!geo_ok(c, hi, wi, ho, wo) || !logits || !hist || !hist_ok(c, bins)) return MSL_ERR_ARG;
  const Geo g = make_geo(c, hi, wi, ho, wo);
  const int nblk = hist_blocks(ho, wo);
  const size_t lds = (size_t)c * bins * sizeof(unsigned int);
  hipStream_t st = as_stream(stream);
  if (logits_flip)
    MSL_DISPATCH_C(c, CM,
                   MSL_LAUNCH((k_confidence_hist<1, CM>), dim3(nblk), dim3(256), lds, st, logits, logits_flip, g,
                              bins, hist));
  else
    MSL_DISPATCH_C(c, CM,
                   MSL_LAUNCH((k_confidence_hist<0, CM>), dim3(nblk), dim3(256), lds, st, logits, logits_flip, g,
                              bins, hist));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_confidence_hist_tta(const msl_tta_entry* entries, int n, int c, int ho, int wo, int bins,
                            unsigned long long* hist, msl_stream_t stream) {
  TtaTable t;
  if (!geo_ok(c, 1, 1, ho, wo) || !make_tta(entries, n, c, ho, wo, &t) || !hist || !hist_ok(c, bins))
    return MSL_ERR_ARG;
  const size_t lds = (size_t)c * bins * sizeof(unsigned int);
  MSL_DISPATCH_C(c, CM,
                 MSL_LAUNCH((k_confidence_hist_tta<CM>), dim3(hist_blocks(ho, wo)), dim3(256), lds,
                            as_stream(stream), t, n, c, ho, wo, bins, hist));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_class_thresholds(const unsigned long long* hist, int c, int bins, double portion, float thr_max,
                         float* thr, unsigned long long* kept, msl_stream_t stream) {
  if (!hist || !thr || c < 1 || c > kMaxC || !hist_ok(c, bins) || !(portion >= 0.0 && portion <= 1.0) ||
      !(thr_max > 0.f && thr_max <= 1.f))
    return MSL_ERR_ARG;
  MSL_LAUNCH(k_class_thresholds, dim3(1), dim3(256), 0, as_stream(stream), hist, c, bins, portion, thr_max, thr,
             kept);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_pseudo_classwise(const float* logits, const float* logits_flip, int c, int hi, int wi, int ho, int wo,
                         const float* thr, long long* label, uint8_t* pseudo, msl_stream_t stream) {
  if (!geo_ok(c, hi, wi, ho, wo) || !logits || !thr || !(label || pseudo)) return MSL_ERR_ARG;
  const Geo g = make_geo(c, hi, wi, ho, wo);
  const int vec = wo % 4 == 0 && dword_aligned(pseudo);
  const int nblk = image_blocks(ho, wo);
  hipStream_t st = as_stream(stream);
  if (logits_flip)
    MSL_DISPATCH_C(c, CM,
                   MSL_LAUNCH((k_pseudo_classwise<1, CM>), dim3(nblk), dim3(256), 0, st, logits, logits_flip, g,
                              thr, label, pseudo, vec));
  else
    MSL_DISPATCH_C(c, CM,
                   MSL_LAUNCH((k_pseudo_classwise<0, CM>), dim3(nblk), dim3(256), 0, st, logits, logits_flip, g,
                              thr, label, pseudo, vec));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_pseudo_classwise_tta(const msl_tta_entry* entries, int n, int c, int ho, int wo, const float* thr,
                             long long* label, uint8_t* pseudo, msl_stream_t stream) {
  TtaTable t;
  if (!geo_ok(c, 1, 1, ho, wo) || !make_tta(entries, n, c, ho, wo, &t) || !thr || !(label || pseudo))
    return MSL_ERR_ARG;
  const int vec = wo % 4 == 0 && dword_aligned(pseudo);
  MSL_DISPATCH_C(c, CM,
                 MSL_LAUNCH((k_pseudo_classwise_tta<CM>), dim3(image_blocks(ho, wo)), dim3(256), 0,
                            as_stream(stream), t, n, c, ho, wo, thr, label, pseudo, vec));
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_colorize(const void* cls, int is_int64, long long npx, const uint8_t* palette, int c, uint8_t* out,
                 msl_stream_t stream) {
  if (!cls || !palette || !out || npx < 0 || c < 1 || c > kColorizeMaxC || (is_int64 != 0 && is_int64 != 1))
    return MSL_ERR_ARG;
  if (npx == 0) return MSL_OK;
  const int vec = dword_aligned(out);
  const int nblk = (int)std::min<long long>(4096, (npx + 1023) / 1024);
  hipStream_t st = as_stream(stream);
  if (is_int64)
    MSL_LAUNCH((k_colorize<long long>), dim3(nblk), dim3(256), 0, st, (const long long*)cls, npx, palette, c,
               out, vec);
  else
    MSL_LAUNCH((k_colorize<int32_t>), dim3(nblk), dim3(256), 0, st, (const int32_t*)cls, npx, palette, c, out,
               vec);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_analysis_maps(const float* x, const float* mean, const long long* label, const uint8_t* cls,
                      const uint8_t* palette, int c, int h, int w, const int* state, long long slot_stride,
                      uint8_t* label_out, uint8_t* pred_out, uint8_t* input_out, uint8_t* error_out,
                      msl_stream_t stream) {
  const MapsOut o = {label_out, pred_out, input_out, error_out};
  if (!(label_out || pred_out || input_out || error_out) || c < 1 || c > kMaxC || h < 1 || w < 1 ||
      (long long)h * w >= (1LL << 31) || slot_stride < 0)
    return MSL_ERR_ARG;
  // what each map reads
  if (((label_out || error_out) && !label) || ((input_out || error_out) && (!x || !mean)) ||
      ((pred_out || error_out) && !cls) || ((label_out || pred_out || error_out) && !palette))
    return MSL_ERR_ARG;
  const int vec = w % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15u) == 0 && dword_aligned(cls) &&
                  dword_aligned(label_out) && dword_aligned(pred_out) && dword_aligned(input_out) &&
                  dword_aligned(error_out) && slot_stride % 4 == 0;
  MSL_LAUNCH(k_analysis_maps, dim3(image_blocks(h, w)), dim3(256), 0, as_stream(stream), x, mean, label, cls,
             palette, c, h, w, state, slot_stride, o, vec);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

}  // extern "C"
