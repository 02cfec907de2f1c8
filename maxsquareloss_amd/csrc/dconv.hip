// Dilated 3x3 (stride 1, padding = dilation) and pointwise convolutions as implicit GEMMs on the
// gfx950 matrix cores: this file is their host half (packs, call records, plans, launches, the C entry
// points); the GEMM kernels are in dconv_kernels.h.  Replaces the cuDNN/oneDNN convolutions of
//   - Bottleneck.conv2 in layer3 (d=2) and layer4 (d=4)   deeplab_multi.py:17-18, 82-83
//   - the live ASPP branches conv_d6 + conv_d12 (+bias)    deeplab_multi.py:51-66, 84-85
//   - every 1x1 conv and, through im2col (stem.hip), the stem
// forward, data gradient and weight gradient.
//
// Layout: activations are [C][P] fp32 with P = H*W (N = 1, NCHW).  The pixel
// axis is tiled linearly (not in 2-D blocks): 65x129 maps do not tile in 2-D
// without ~20 % waste, while 128-pixel linear tiles waste < 1 %.  A dilated tap
// is then a constant shift of the linear pixel index plus a per-pixel validity
// test (row wrap / image border), evaluated once per K-step per thread.
//
// GEMM mapping (one mapping, several matrix-core forms: exact-f32 v_mfma_f32_32x32x2_f32, bf16, the
// fp32-accurate bf16x6 and f16x3 splits, fp16 - chosen per call by plan_fwd / plan_wgrad below):
//   forward / dgrad:  C[m][p] = sum_k A[k][m] * B[k][p]
//       k = ((branch*9 + tap)*ncb + cb)*16 + ci_local  (one tap, 16 channels per K-step;
//       tap-major, so the shifted-pixel offsets change only every ncb K-steps)
//       A = packed weights [Kp][lda] (m contiguous; dgrad: transposed + tap-flipped)
//       B = image[cb*16 + ci_local][p + shift(tap)]  (zero outside the image)
//   wgrad (one GEMM per tap, batched over grid.z):
//       dW[m][n][tap] = sum_p dY[m][p] * X[n][p + shift(tap)]   (K = pixels)
// The forward form runs stream-K over persistent workgroups (pieces of split tiles summed by
// k_sk_reduce in a fixed order).  The exact-f32 and bf16 kernels stage both operands through LDS
// ([k][m] / [k][n]: every MFMA operand read is a conflict-free ds_read_b32 of 32 consecutive floats);
// the split forms read their weights from planes split at pack time and, for the 3x3 shapes, the image
// operand straight to registers (BD) or pre-split (BP).  Only an odd K-step count with M <= 32 still
// runs the split-K tile kernel, its fp32 slabs summed by k_reduce_slabs.
#include "dconv_kernels.h"

namespace msl {

// out[i] = (acc ? out[i] : 0) + sum_s ws[s*n + i] (+ sum_b bias[b*M + i/bias_div])
__global__ void __launch_bounds__(256) k_reduce_slabs(const float* __restrict__ ws, int S, long long n,
                                                       float* __restrict__ out, int accumulate,
                                                       const float* __restrict__ bias, int nbias,
                                                       int bias_M, int bias_div) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    float v = ws[i];
    for (int s = 1; s < S; ++s) v += ws[(long long)s * n + i];
    if (bias) {
      const int m = (int)(i / bias_div);
      float bsum = bias[m];
      for (int b = 1; b < nbias; ++b) bsum += bias[b * bias_M + m];
      v += bsum;
    }
    out[i] = accumulate ? out[i] + v : v;
  }
}

// msl_launch_guard_probe's kernel: out[t] = t (a 256-thread bound, like most of the library's kernels)
__global__ void __launch_bounds__(256) k_guard_probe(float* __restrict__ out) { out[threadIdx.x] = (float)threadIdx.x; }

// dbias[b][m] (=|+=) sum_p dy[m][p], same value for every branch b.
__global__ void __launch_bounds__(256) k_bias_grad(const float* __restrict__ dy, int P,
                                                    float* __restrict__ db, int M, int nbranch,
                                                    int accumulate) {
  const int m = blockIdx.x;
  float s = 0.f;
  for (int p = threadIdx.x; p < P; p += 256) s += dy[(long long)m * P + p];
  s = wave_sum(s);
  __shared__ float part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float tot = (part[0] + part[1]) + (part[2] + part[3]);
    for (int b = 0; b < nbranch; ++b) db[b * M + m] = accumulate ? db[b * M + m] + tot : tot;
  }
}

// Packed operand for the forward-form GEMM.
//   for_dgrad = 0: image = x (cin channels),  m = co: P[k][co] = W[co][ci][t]
//   for_dgrad = 1: image = dy (cout channels), m = ci: P[k][ci] = W[co][ci][8 - t]
// k = ((b*taps + t)*ncb + cb)*16 + c_local with c = cb*16 + c_local (image channel); taps = 9
// for the 3x3 convs, 1 for the pointwise ones.
__global__ void __launch_bounds__(256) k_pack(const float* __restrict__ w, long long branch_stride,
                                               int cin, int cout, int for_dgrad, int ncb, int lda,
                                               int taps, long long total, float* __restrict__ out) {
  const int cimg = for_dgrad ? cout : cin;
  const int mreal = for_dgrad ? cin : cout;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int m = (int)(e % lda);
    const long long k = e / lda;
    const int cl = (int)(k % kCB);
    const long long q = k / kCB;
    const int cb = (int)(q % ncb);
    const long long q2 = q / ncb;
    const int t = (int)(q2 % taps);
    const int b = (int)(q2 / taps);
    const int c = cb * kCB + cl;
    float v = 0.f;
    if (c < cimg && m < mreal) {
      const float* wb = w + (long long)b * branch_stride;
      if (!for_dgrad)
        v = wb[((long long)m * cin + c) * taps + t];
      else
        v = wb[((long long)c * cin + m) * taps + (taps - 1 - t)];
    }
    out[e] = v;
  }
}

// The same pack through LDS, with the bf16x6 planes split in the same launch: one block per
// (16-row m chunk, channel block cb, branch) - 256 blocks for a 256x256 conv.  Both weight
// layouts read as contiguous runs (fwd: W[m][cb*16..+16][taps] = 16*taps floats per m; dgrad:
// W[c][m0..m0+16][taps] = 16*taps floats per c), the tile is transposed in LDS, and the writes
// are 64-B fp32 row segments and 256-B plane runs.  k_pack's per-element gather (a 36-B or
// cin*36-B lane stride) took 6 us for a 256x256x9 weight; the split was a second 4.6-us launch.
// (64-row chunks: 64 blocks for that weight, 24 us - too few workgroups.)
constexpr int kPackTileM = 16;

// One (16-row m chunk, 16-channel block, branch) block of the pack + split; s = the block's LDS tile.
template <int TAPS>
__device__ __forceinline__ void pack_split_block(const float* __restrict__ w, long long branch_stride, int cin,
                                                 int cout, int for_dgrad, int ncb, int lda, int split,
                                                 float* __restrict__ out, __bf16* __restrict__ planes, int mx,
                                                 int cb, int b, float (*s)[kPackTileM + 1],
                                                 float* __restrict__ tail = nullptr) {
  const int m0 = mx * kPackTileM;
  const int cimg = for_dgrad ? cout : cin;
  const int mreal = for_dgrad ? cin : cout;
  const float* wb = w + (long long)b * branch_stride;
  constexpr int N = kCB * TAPS * kPackTileM;
  for (int i = threadIdx.x; i < N; i += 256) {
    int ml, cl, tm;  // tm = memory tap
    if (!for_dgrad) {  // i = (ml*16 + cl)*TAPS + tm: W[m][c][tm] contiguous over (cl, tm)
      tm = i % TAPS;
      cl = (i / TAPS) % kCB;
      ml = i / (TAPS * kCB);
    } else {  // i = (cl*16 + ml)*TAPS + tm: W[c][m][tm] contiguous over (ml, tm)
      tm = i % TAPS;
      ml = (i / TAPS) % kPackTileM;
      cl = i / (TAPS * kPackTileM);
    }
    const int m = m0 + ml, c = cb * kCB + cl;
    float v = 0.f;
    if (m < mreal && c < cimg)
      v = for_dgrad ? wb[((long long)c * cin + m) * TAPS + tm] : wb[((long long)m * cin + c) * TAPS + tm];
    const int t = for_dgrad ? TAPS - 1 - tm : tm;
    s[cl * TAPS + t][ml] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < N; i += 256) {  // i = (t*16 + cl)*16 + ml
    const int ml = i % kPackTileM, cl = (i / kPackTileM) % kCB, t = i / (kPackTileM * kCB);
    const long long k = ((long long)(b * TAPS + t) * ncb + cb) * kCB + cl;
    out[k * lda + m0 + ml] = s[cl * TAPS + t][ml];
  }
  if (!split) return;
  if (tail) {  // f16x3: two fp16 planes of W * sA; {sA, 1/sA} written by k_pack_scale* before this launch
    const float sc = tail[kNPart];
    f16x8* pl = reinterpret_cast<f16x8*>(planes);
    for (int i = threadIdx.x; i < TAPS * 2 * kPackTileM; i += 256) {
      const int ml = i % kPackTileM, h = (i / kPackTileM) & 1, t = i / (2 * kPackTileM);
      const long long ks = (long long)(b * TAPS + t) * ncb + cb;
      Split2h sp;
#pragma unroll
      for (int j = 0; j < 8; ++j) split2h_set(sp, j, s[(8 * h + j) * TAPS + t][ml] * sc);
      const long long row = ((ks * 2) * 2 + h) * lda + m0 + ml;  // plane 0
      pl[row] = sp.hi;
      pl[row + 2LL * lda] = sp.lo;
    }
    return;
  }
  bf16x8* pl = reinterpret_cast<bf16x8*>(planes);
  for (int i = threadIdx.x; i < TAPS * 2 * kPackTileM; i += 256) {  // i = (t*2 + h)*16 + ml
    const int ml = i % kPackTileM, h = (i / kPackTileM) & 1, t = i / (2 * kPackTileM);
    const long long ks = (long long)(b * TAPS + t) * ncb + cb;
    Split3 sp;
#pragma unroll
    for (int j = 0; j < 8; ++j) split3_set(sp, j, s[(8 * h + j) * TAPS + t][ml]);
    const long long row = ((ks * 3) * 2 + h) * lda + m0 + ml;  // plane 0 (k_split_pack layout)
    pl[row] = sp.hi;
    pl[row + 2LL * lda] = sp.mid;
    pl[row + 4LL * lda] = sp.lo;
  }
}

template <int TAPS>
__global__ void __launch_bounds__(256) k_pack_split(const float* __restrict__ w, long long branch_stride,
                                                    int cin, int cout, int for_dgrad, int ncb, int lda,
                                                    int split, float* __restrict__ out,
                                                    __bf16* __restrict__ planes, float* __restrict__ tail) {
  __shared__ float s[kCB * TAPS][kPackTileM + 1];  // [cl*TAPS + t][ml], t = packed tap index
  pack_split_block<TAPS>(w, branch_stride, cin, cout, for_dgrad, ncb, lda, split, out, planes, blockIdx.x,
                         blockIdx.y, blockIdx.z, s, tail);
}

// Packed-buffer tail (after the fp32 pack and its planes): the f16x3 form's kNPart absmax
// partials of the weights, then {sA, 1/sA}.
constexpr long long kPackTail = 320;
__host__ __device__ inline long long pack_tail_offset(long long f32_elems) { return f32_elems * 5 / 2; }

// f16x3 weight absmax of every job (grid = (kNPart, njobs)) into each job's pack tail
template <int TAPS>
__global__ void __launch_bounds__(256) k_absmax_jobs(const msl_pack_job* __restrict__ jobs) {
  const msl_pack_job jb = jobs[blockIdx.y];
  const int cimg = jb.for_dgrad ? jb.cout : jb.cin;
  const int m = jb.for_dgrad ? jb.cin : jb.cout;
  const long long f32 = (long long)jb.nbranch * ((cimg + kCB - 1) / kCB) * TAPS * kCB * ((m + kPackPad - 1) / kPackPad * kPackPad);
  absmax_block(jb.w, (long long)jb.cout * jb.cin * TAPS, jb.branch_stride, jb.nbranch, blockIdx.x,
               jb.packed + pack_tail_offset(f32) + blockIdx.x);
}

// {sA, 1/sA} of a pack from its kNPart weight absmax partials, once per pack (the pack blocks read
// sA: every one of them reducing the 256 partials itself read 4x its own 1-KB tile - 0.44 ms per
// step for the ~170k blocks of the step's packs, r03)
__device__ __forceinline__ void pack_scale(float* __restrict__ tail) {
  float inv;
  const float sc = pow2_scale(partials_max(tail, kNPart, threadIdx.x & 63), inv);
  if (threadIdx.x == 0) {
    tail[kNPart] = sc;
    tail[kNPart + 1] = inv;
  }
}
__global__ void __launch_bounds__(64) k_pack_scale(float* __restrict__ tail) { pack_scale(tail); }
template <int TAPS>
__global__ void __launch_bounds__(64) k_pack_scale_jobs(const msl_pack_job* __restrict__ jobs) {
  const msl_pack_job jb = jobs[blockIdx.x];
  const int cimg = jb.for_dgrad ? jb.cout : jb.cin;
  const int m = jb.for_dgrad ? jb.cin : jb.cout;
  const long long f32 = (long long)jb.nbranch * ((cimg + kCB - 1) / kCB) * TAPS * kCB * ((m + kPackPad - 1) / kPackPad * kPackPad);
  pack_scale(jb.packed + pack_tail_offset(f32));
}

// (m chunk, channel block) tiles per block of the batched pack: a pointwise tile is only 256 floats
// (one per thread), and the ~300k one-tile blocks of a step's pointwise packs took 288 us (r03)
template <int TAPS>
constexpr int kPackSub() { return TAPS == 1 ? 8 : 1; }

// Every weight pack of a step in one launch (per tap count): block b runs block b - start[j] of
// job j (start[] ascending, start[njobs] = the total), each job exactly as msl_*_pack would.
template <int TAPS>
__global__ void __launch_bounds__(256) k_pack_split_many(const msl_pack_job* __restrict__ jobs,
                                                         const long long* __restrict__ start, int njobs, int h3) {
  __shared__ float s[kCB * TAPS][kPackTileM + 1];
  const long long b = blockIdx.x;
  int lo = 0, hi = njobs - 1;  // the last job with start <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const msl_pack_job jb = jobs[lo];
  const int cimg = jb.for_dgrad ? jb.cout : jb.cin;
  const int m = jb.for_dgrad ? jb.cin : jb.cout;
  const int lda = (m + kPackPad - 1) / kPackPad * kPackPad;
  const int ncb = (cimg + kCB - 1) / kCB;
  const int nmx = lda / kPackTileM;
  const long long tiles = (long long)nmx * ncb * jb.nbranch;
  const long long f32 = (long long)jb.nbranch * ncb * TAPS * kCB * lda;
  constexpr int SUB = kPackSub<TAPS>();
#pragma unroll 1
  for (int sub = 0; sub < SUB; ++sub) {
    const long long local = (b - start[lo]) * SUB + sub;
    if (local >= tiles) break;  // block-uniform
    if (sub) __syncthreads();   // the previous tile's LDS reads are done
    const int mx = (int)(local % nmx);
    const long long rest = local / nmx;
    const int cb = (int)(rest % ncb), br = (int)(rest / ncb);
    pack_split_block<TAPS>(jb.w, jb.branch_stride, jb.cin, jb.cout, jb.for_dgrad, ncb, lda, m > 64 || h3, jb.packed,
                           reinterpret_cast<__bf16*>(jb.packed + f32), mx, cb, br, s,
                           h3 ? jb.packed + pack_tail_offset(f32) : nullptr);
  }
}

// ---------------------------------------------------------------- the calls
// The geometry of a conv call: nbranch dilated 3x3 branches over nimg images of h x w stacked along the
// pixel axis (P = nimg * h * w), or one unshifted tap (dilation 0) over p flat pixels
struct ConvGeom {
  int nbranch, taps, h, w, nimg, dil0, dil1;
};
static ConvGeom geom_3x3(int nbranch, int h, int w, int nimg, int dil0, int dil1) {
  return {nbranch, 9, h, w, nimg, dil0, dil1};
}
static ConvGeom geom_1x1(int p) { return {1, 1, 1, p, 1, 0, 0}; }

// One forward-form GEMM (a forward or a data gradient): out[M][P] (=|+=) W . img
struct FwdCall {
  ConvGeom g;
  const float* img;     // [cimg][P]: x (cin channels) forward, dy (cout channels) for a data gradient
  const float* packed;  // the weights packed for this orientation (pack())
  const float* bias;    // [nbranch][M] or null
  float* out;           // [M][P]
  int M, cimg;
  int accum;            // out += the result (the fused residual-gradient sum)
  const float* img_part;  // the caller's absmax partials of img (null: reduced here where the form scales)
  int img_npart;
  // with accum: out = mask(res) + the result (FwdArgs::accres, msl_pconv_dgrad_resmask*)
  const float* res;
  const unsigned long long* res_mask;
  int res_nimg;
};

// One weight gradient: dw[nbranch][cout][cin][taps] (=|+=) dy . x^T over the P pixels
struct WgradCall {
  ConvGeom g;
  const float* x;
  const float* dy;
  float* dw;
  float* dbias;  // [nbranch][cout] or null
  int cin, cout, accumulate;
  // the caller's per-row absmax partials of x / dy (null: reduced here where the form scales)
  const float* x_part;
  int x_npart;
  const float* dy_part;
  int dy_npart;
};

static bool bad_dims(int nbranch, int cin, int cout, int h, int w, int nimg = 1) {
  return nbranch < 1 || nbranch > 2 || cin < 1 || cout < 1 || h < 1 || w < 1 || nimg < 1 ||
         (long long)nimg * h * w > (1LL << 30);
}
static bool bad_geom(const ConvGeom& g, int cin, int cout) {
  return bad_dims(g.nbranch, cin, cout, g.h, g.w, g.nimg) ||
         (g.taps == 9 && (g.dil0 < 1 || (g.nbranch == 2 && g.dil1 < 1)));
}
static bool bad_parts(const float* p, int n) { return p && n < 1; }

// The argument checks of every forward-form / weight-gradient entry point (MSL_ERR_ARG)
static bool bad_fwd(const FwdCall& c) {
  return bad_geom(c.g, c.cimg, c.M) || !c.img || !c.packed || !c.out || bad_parts(c.img_part, c.img_npart) ||
         (c.res && (!c.accum || !c.res_mask || c.res_nimg < 1 || (c.g.nimg * c.g.h * c.g.w) % c.res_nimg != 0));
}
static bool bad_wgrad(const WgradCall& c) {
  return bad_geom(c.g, c.cin, c.cout) || !c.x || !c.dy || !c.dw || bad_parts(c.x_part, c.x_npart) ||
         bad_parts(c.dy_part, c.dy_npart);
}

// ---------------------------------------------------------------- forward form: the plan
// Forward form (fwd and dgrad) runs stream-K (k_igemm_fwd_sk): 128-pixel tiles of 128, 64 or
// 32 rows (by M: the ASPP forward has 19 classes), up to 512 persistent workgroups (2 per CU), so
// every CU gets the same number of MFMA stages whatever the tile count.  The split-K tile kernel
// remains for an odd K-step count with M <= 32.
constexpr int kSkBN = 128, kSkNW = 512;
// The call's forms (msl_forms, r05: per call, no process state): sk_hybrid = the forward-form
// schedule (1: data-parallel rounds + stream-K remainder when the tiles outnumber the workers,
// SkArgs; 0: pure stream-K); f32_form = the matrix-core form of the fp32 entry points: kMathF32 runs
// v_mfma_f32_32x32x2_f32 (an exact fmaf chain), kMathX6 the three-way bf16 split on the BF16
// matrix cores (fp32-accurate, dconv_kernels.h; layer3 fwd 78 vs 102 us in the step, err vs fp64
// 4e-8 vs 6e-8 relative to sum|terms|), kMathH3P the scaled two-way fp16 split (three fp16
// MFMAs per slice; dconv_kernels.h Split2h); packs are form-specific.
static_assert(kMathF32 == 0 && kMathX6 == 2 && kMathH3P == 5, "msl_forms.f32_form values");

// How the image operand reaches the MFMAs: staged through LDS; straight to registers (BD: dword pieces
// of the shifted 3x3 rows, split in the loop); or pre-split once for the whole GEMM by k_split_img (BP)
enum { kBLds = 0, kBDirect = 1, kBPre = 2 };

// One instantiation of the stream-K kernel: the template arguments of k_igemm_fwd_sk / k_igemm_fwd_sk2
struct SkForm {
  int bm, G, stages, wm, wn;  // tile rows, K-steps per LDS stage, stages, wave layout
  bool pw;                    // pointwise B rows (dwordx4 pieces)
  int mt;                     // the kernel's math (kMathF32, kMathBf16, kMathX6P, kMathH3P, kMathH1P)
  bool acc;                   // the accumulate epilogue
  int bform;                  // kBLds / kBDirect / kBPre
};
static bool operator==(const SkForm& a, const SkForm& b) {
  return a.bm == b.bm && a.G == b.G && a.stages == b.stages && a.wm == b.wm && a.wn == b.wn && a.pw == b.pw &&
         a.mt == b.mt && a.acc == b.acc && a.bform == b.bform;
}

struct FwdPlan {
  bool sk;      // stream-K (form, sched); else the split-K tile kernel k_igemm_fwd (S slabs of kps K-steps)
  SkForm form;
  int tiles_m, tiles_n, ksteps, kps, S;
  SkArgs sched;  // tiles, stages per tile, tdp / gm / NW / T (no pointers)
  bool reduce;   // k_sk_reduce<form.bm> follows over the split tiles
};

// r06: f16x3 pointwise GEMMs with M a multiple of 256 from kPw256MinM on 256 x 128 tiles, 1 x 4 waves (each 256 rows
// x 32 pixels, its A fragments streamed row block by row block): the image operand read once per 256 rows.  Same box
// (profiles/r06_wide_tiles_ab.txt): 512 -> 2048 fwd 109 vs 118 us, 2048 -> 512 dgrad 120 vs 128; at M = 1024 even,
// at M <= 512 slower (fewer tiles than workers: 1024 -> 256 fwd 54 vs 48, 2048 -> 512 fwd 129 vs 107).  A 384-row
// tile for the ASPP heads (M = 342: the operand read once instead of three times) needs 192 accumulator registers
// per lane and spilled 96-188 VGPRs at one or two waves per SIMD: not built.
constexpr int kPw256MinM = 2048;
static int wide_rows(int taps, int M) { return taps == 1 && M % 256 == 0 && M >= kPw256MinM ? 256 : 0; }

static int pad_to(int v, int a) { return (v + a - 1) / a * a; }

static int choose_split(int tiles, int ksteps, int min_steps) {
  const int target = 512;  // 256 CUs x 2 resident workgroups
  if (tiles >= 384) return 1;
  int S = (target + tiles - 1) / tiles;
  S = std::max(1, std::min(S, ksteps / min_steps));
  return S;
}

// The f16x3 / fp16 forward-form GEMMs that read their image operand pre-split (k_split_img, BP form):
// the 3x3 ones with M >= 512: the split pass is shared by 4 row blocks and 9 taps (layer4 fwd 162 vs 174 us,
// dgrad 172 vs 185; loses where the pass is a large share: pointwise 39 vs 31 us, layer2 34 vs 31, ASPP
// 144 vs 135 - profiles/r03_bp_ab.txt); fp16 math (one plane: a quarter of the loads' instructions, half
// their bytes) from M >= 128 (r05)
static bool bp_form(int taps, int M, bool h1) { return taps == 9 && (M >= 512 || (h1 && M >= 128)); }

// The stream-K schedule of tiles_m x tiles_n tiles of KS stages over at most nw_max workers.
// At least as many tiles as workers: whole rounds of tiles data-parallel, stream-K over the rest
// (SkArgs); fewer: pure stream-K.  Every stream-K worker must own at least one iteration: the piece
// count of a tile is the number of workgroups its iteration range touches.
static SkArgs plan_sk(int tiles_m, int tiles_n, int KS, int nw_max, int hybrid) {
  SkArgs sk{};
  sk.tiles_m = tiles_m;
  sk.tiles_n = tiles_n;
  sk.KS = KS;
  const long long tiles = (long long)tiles_m * tiles_n;
  sk.tdp = (hybrid && tiles >= nw_max) ? (int)(tiles / nw_max * nw_max) : 0;
  // Tile order (r04): m fastest when whole rounds of tiles run data-parallel (hybrid): one XCD's
  // workers then hold every m-block of a few pixel blocks, so each image block is fetched once and
  // re-read from that L2 (same box: 256 -> 1024 fwd 42.7 vs 49.8 us, 2048 -> 512 dgrad 127 vs 141,
  // layer4 fwd 214 vs 226; profiles/r04_tile_order_ab.txt).  n fastest for pure stream-K: a worker's
  // range there is under one tile, the m-blocks of a pixel block run at staggered K offsets and get no
  // L2 reuse, and the shared weights of n fastest win (ASPP fwd, M = 342 over 128 K-steps: 134 vs
  // 101 us m fastest; layer3 fwd 79 vs 77.7; profiles/r04_aspp_tile_order.txt).
  sk.gm = sk.tdp > 0 ? tiles_m : 1;
  const long long T = (tiles - sk.tdp) * KS;
  sk.NW = (int)std::min<long long>(nw_max, T);
  // the remainder after data-parallel rounds (e.g. 16 tiles x 16 K-steps of a 256 -> 1024 pointwise
  // GEMM): at one or two K-steps per worker every worker writes a whole 64-KB piece for almost no
  // work; at least kSkMinIt K-steps each (512 -> 2048 fwd 75.9 vs 82.2 us, 2048 -> 512 dgrad 85.6 vs
  // 90.0)
  constexpr long long kSkMinIt = 8;
  if (sk.tdp > 0) sk.NW = (int)std::max<long long>(1, std::min<long long>(sk.NW, T / kSkMinIt));
  sk.T = (int)T;
  return sk;
}

// Every form decision of a forward-form call; `math` = the entry point's (kMathF32 / kMathX6 / kMathH3P: the
// fp32 entry points' f32_form; kMathBf16; kMathH1P = fp16).  No launches, no pointers.
static FwdPlan plan_fwd(int math, int nbranch, int taps, int cimg, int M, int P, int accum, int dil0,
                        const msl_forms* forms) {
  FwdPlan pl{};
  const bool f16 = math == kMathH3P || math == kMathH1P;
  const int groups = nbranch * cdiv(cimg, kCB) * taps;  // K-steps: one tap, 16 channels each
  const int bm = M > 64 ? 128 : (M > 32 ? 64 : 32);
  pl.ksteps = groups;
  pl.tiles_n = cdiv(P, kSkBN);
  pl.sk = groups % 2 == 0 || bm > 32;
  if (!pl.sk) {  // k_igemm_fwd<64, 128, 16, 2, 2>: exact f32 in every math, S slabs summed by k_reduce_slabs
    pl.tiles_m = cdiv(M, 64);
    const int S = choose_split(pl.tiles_m * pl.tiles_n, groups, 4);
    pl.kps = cdiv(groups, S);
    pl.S = cdiv(groups, pl.kps);
    return pl;
  }
  // exact-f32 / bf16 MFMA, both operands through LDS: two K-steps per stage where the count is even, 2 x 2
  // waves (1 x 4 on the 32-row tiles); also the 64- and 32-row tiles of the x6 form (no gain measured there)
  SkForm& f = pl.form;
  f.bm = bm;
  f.G = groups % 2 == 0 ? 2 : 1;
  f.stages = f.G == 2 ? 2 : 3;
  f.wm = bm == 32 ? 1 : 2;
  f.wn = bm == 32 ? 4 : 2;
  f.mt = math == kMathBf16 ? kMathBf16 : kMathF32;
  f.acc = accum != 0;
  if (math == kMathX6 && bm == 128) {
    // one K-step per stage, four stages deep (r01 tuning harness, layer3: 87 us vs 115 with two K-steps
    // per stage), the weights from the bf16 planes that pack() split once (M > 64 <=> 128-row tiles)
    f.G = 1;
    f.stages = 4;
    f.mt = kMathX6P;
  } else if (f16) {
    // f16x3 / fp16 (which reads the f16x3 packs' hi planes): one K-step per stage, four stages, the weights
    // from the fp16 planes.  Waves 1 x 4 (each 128 rows x 32 pixels): every wave splits only its own B columns
    // (2 x 2 waves split each column twice); step 40.5 vs 40.9 ms on one box (profiles/r02_f16x3_waves.txt)
    f.G = 1;
    f.stages = 4;
    f.wm = 1;
    f.wn = 4;
    f.mt = math;
    // the image operand straight to registers (BD form) for the shifted 3x3 rows (dword pieces); the pointwise
    // rows keep their two dwordx4 LDS-DMA pieces per wave and K-step (BD loses there: 256 -> 1024 fwd 32.7 vs
    // 31.0 us, 2048 -> 512 82.7 vs 75.1; layer3 3x3 fwd 52.4 vs 55.0, layer4 172 vs 190;
    // profiles/r03_fwd_forms_ab.txt).  Full 16-channel blocks only: the stem's 147-row im2col operand keeps
    // the LDS form
    const bool bd = cimg % kCB == 0;
    if (bm <= 64) {
      // r03: M <= 64 (the 19-class ASPP forward, layer1's 64-channel 3x3 and 256 -> 64 convs, the 64-channel
      // data gradients, the stem's 147 -> 64) on 64-row tiles of the same kernel, pointwise too (one unshifted
      // tap), instead of exact-f32 32 / 64-row tiles: 3 fp16 MFMAs per 16-deep slice at 64 rows cost 2.7x less
      // matrix time than 8 f32 MFMAs at 32 rows.  r04: the fp16 math too (fwd_sk_body AHALF).  The only
      // accumulating BD form: the pointwise M <= 64 data gradients
      f.bm = 64;
      f.bform = bd ? kBDirect : kBLds;
    } else if (taps == 1 && dil0 == 0) {
      // pointwise: B rows are unshifted, so they move as dwordx4 (4 pixels per lane: 2 DMAs per wave and
      // K-step instead of 8 dword ones): 1-4 us per call on the wide 1x1 GEMMs (profiles/r02_f16x3_pw_dma.txt)
      f.pw = true;
      if (math == kMathH3P && wide_rows(taps, M)) {
        f.bm = 256;
        f.stages = 3;
      } else if (math == kMathH1P && groups % 2 == 0) {
        // fp16 (r04): two K-steps per LDS stage, three stages (72 KB, two workgroups per CU): one barrier per
        // 8 MFMAs per wave instead of 4 (f16x3's two planes would need 96 KB)
        f.G = 2;
        f.stages = 3;
      }
    } else if (!f.acc) {  // (no 3x3 call accumulates; no 128-row accumulating 3x3 form - LDS, BD or BP - is built)
      f.bform = bp_form(taps, M, math == kMathH1P) ? kBPre : bd ? kBDirect : kBLds;
    }
  }
  pl.tiles_m = cdiv(M, f.bm);
  pl.kps = groups / f.G;  // stages per tile
  pl.S = 1;
  pl.sched = plan_sk(pl.tiles_m, pl.tiles_n, pl.kps, kSkNW, forms_of(forms).sk_hybrid);
  pl.reduce = pl.sched.T > 0;
  return pl;
}

// Workspace of a forward-form call: the stream-K pieces, NW x 2 x BM*BN floats (summed by k_sk_reduce; no
// flags or other state survive a call), then (the BP form) the image operand's fp16 planes, then (f16x3)
// the image's kNPart absmax partials at the end of the caller's workspace.  Independent of the call's
// forms and math (they come with the call, not with the query): the pieces sized for the largest tile the
// shape can get (64 rows at M <= 64, the 256-row pointwise tiles twice the 128-row pieces - r05's 256 /
// 384-row attempt kept the 128-row size, and its pieces ran past the workspace into the partials behind
// them), and a 3x3 GEMM with 128 <= M < 512 reserves the image planes that only the fp16 math's BP form
// reads (cimg x P x 4 bytes, e.g. ~17 MB at layer2's pair shape): conservative, accepted.
// The stem / pointwise calls reserve no planes.
constexpr size_t kPartBytes = kNPart * sizeof(float);
static size_t fwd_piece_bytes(int taps, int M) {
  return align_up((size_t)kSkNW * 2 * std::max(wide_rows(taps, M), M > 64 ? 128 : 64) * kSkBN * sizeof(float), 256);
}
static size_t img_planes_bytes(int cimg, int P) { return align_up((size_t)cdiv(cimg, kCB) * kCB * P * 4, 256); }
static size_t fwd_ws_bytes(const FwdPlan& pl, int taps, int cimg, int M, int P) {
  if (pl.sk) return fwd_piece_bytes(taps, M) + (bp_form(taps, M, true) ? img_planes_bytes(cimg, P) : 0) + kPartBytes;
  return (pl.S > 1 ? (size_t)pl.S * M * P * sizeof(float) : 0) + kPartBytes;
}
static size_t fwd_query_bytes(int nbranch, int taps, int cimg, int M, int P) {
  return fwd_ws_bytes(plan_fwd(kMathF32, nbranch, taps, cimg, M, P, 0, taps == 9, nullptr), taps, cimg, M, P);
}
static float* ws_partials(void* ws, size_t ws_bytes, int k) {  // k-th partials block from the end
  return reinterpret_cast<float*>((char*)ws + ((ws_bytes - (size_t)k * kPartBytes) & ~(size_t)15));
}

// ---------------------------------------------------------------- forward form: the kernels
// Every instantiation of the stream-K kernel, keyed by its own template arguments, with its launch bound
// (MSL_LAUNCH_ENTRY).  k_igemm_fwd_sk2 is the same kernel held to two waves per SIMD (the f16 forms).  Only rows
// that a call through some entry point launches are built (tests/test_conv_forms.py); a plan whose form has no row
// here is MSL_ERR_SHAPE: an accumulate epilogue in the bf16 math (its entry points take no accumulate flag) or on a
// 128-row tile that is not pointwise (no 3x3 call accumulates).
struct SkKernel {
  SkForm form;
  void (*fn)(FwdArgs, SkArgs);
  std::atomic<int> bound{0};
};
#define MSL_SK(BM, G, ST, WM, WN, MT, ACC) \
  {{BM, G, ST, WM, WN, false, MT, ACC, kBLds}, k_igemm_fwd_sk<BM, kSkBN, G, ST, WM, WN, false, MT, ACC>}
#define MSL_SK_BOTH(BM, G, ST, WM, WN, MT) MSL_SK(BM, G, ST, WM, WN, MT, false), MSL_SK(BM, G, ST, WM, WN, MT, true)
#define MSL_SK2(BM, G, ST, PW, MT, ACC, BF)  \
  {{BM, G, ST, 1, 4, PW, MT, ACC, BF},       \
   k_igemm_fwd_sk2<BM, kSkBN, G, ST, 1, 4, PW, MT, ACC, (BF) != kBLds, (BF) == kBPre>}
#define MSL_SK2_BOTH(BM, G, ST, PW, MT, BF) MSL_SK2(BM, G, ST, PW, MT, false, BF), MSL_SK2(BM, G, ST, PW, MT, true, BF)
// the f16x3 / fp16 rows they share: 64-row tiles (LDS and BD), 128-row 3x3 tiles in every operand form, pointwise
#define MSL_SK2_F16(MT)                                                                                      \
  MSL_SK2_BOTH(64, 1, 4, false, MT, kBLds), MSL_SK2_BOTH(64, 1, 4, false, MT, kBDirect),                      \
  MSL_SK2(128, 1, 4, false, MT, false, kBLds), MSL_SK2(128, 1, 4, false, MT, false, kBDirect),                \
  MSL_SK2(128, 1, 4, false, MT, false, kBPre), MSL_SK2_BOTH(128, 1, 4, true, MT, kBLds)
static SkKernel kSkKernels[] = {
    MSL_SK_BOTH(128, 2, 2, 2, 2, kMathF32), MSL_SK_BOTH(128, 1, 3, 2, 2, kMathF32),
    MSL_SK_BOTH(64, 2, 2, 2, 2, kMathF32), MSL_SK_BOTH(64, 1, 3, 2, 2, kMathF32),
    MSL_SK_BOTH(32, 2, 2, 1, 4, kMathF32),
    MSL_SK(128, 2, 2, 2, 2, kMathBf16, false), MSL_SK(128, 1, 3, 2, 2, kMathBf16, false),
    MSL_SK(64, 2, 2, 2, 2, kMathBf16, false), MSL_SK(64, 1, 3, 2, 2, kMathBf16, false),
    MSL_SK(32, 2, 2, 1, 4, kMathBf16, false),
    MSL_SK_BOTH(128, 1, 4, 2, 2, kMathX6P),
    MSL_SK2_F16(kMathH3P), MSL_SK2_BOTH(256, 1, 3, true, kMathH3P, kBLds),
    MSL_SK2_F16(kMathH1P), MSL_SK2_BOTH(128, 2, 3, true, kMathH1P, kBLds),
};
#undef MSL_SK2_F16
#undef MSL_SK2_BOTH
#undef MSL_SK2
#undef MSL_SK_BOTH
#undef MSL_SK

static SkKernel* sk_kernel(const SkForm& f) {
  for (SkKernel& k : kSkKernels)
    if (k.form == f) return &k;
  return nullptr;
}

// The shapes a planned call refuses (MSL_ERR_SHAPE), for launch_fwd_form and the plan query
// (msl_conv_fwd_plan) alike: the split-K tile kernel (odd K-step count, M <= 32) has no bf16 form and no
// accumulate epilogue; the stream-K kernels index in 32 bits (the bound of 128-row tiles, for the 256-row
// ones too), and a form without a row in kSkKernels is not built.
static int fwd_refusal(int math, const FwdPlan& pl, int cimg, int M, int P, int accum) {
  if (!pl.sk) return (math == kMathBf16 || accum) ? MSL_ERR_SHAPE : MSL_OK;
  const long long lda = pad_to(M, kPackPad);
  if ((long long)cdiv(M, std::min(pl.form.bm, 128)) * pl.tiles_n * pl.kps * kSkNW >= (1LL << 31) ||
      (long long)cimg * P >= (1LL << 29) || (long long)pl.ksteps * kCB * lda >= (1LL << 29))
    return MSL_ERR_SHAPE;
  return sk_kernel(pl.form) ? MSL_OK : MSL_ERR_SHAPE;
}

// Plan, then launch in this order: k_absmax, k_split_img, the GEMM, k_sk_reduce
static int launch_fwd_form(int math, const FwdCall& c, const msl_forms* forms, void* ws, size_t ws_bytes,
                           hipStream_t st) {
  const ConvGeom& g = c.g;
  const int P = g.nimg * g.h * g.w;
  const FwdPlan pl = plan_fwd(math, g.nbranch, g.taps, c.cimg, c.M, P, c.accum, g.dil0, forms);
  if (ws_bytes < fwd_ws_bytes(pl, g.taps, c.cimg, c.M, P)) return MSL_ERR_WORKSPACE;
  if (const int refused = fwd_refusal(math, pl, c.cimg, c.M, P, c.accum)) return refused;
  FwdArgs a{};
  a.A = c.packed;
  a.B = c.img;
  a.C = c.out;
  a.bias = c.bias;
  a.nbias = g.nbranch;  // (read with a bias only)
  a.M = c.M;
  a.lda = pad_to(c.M, kPackPad);
  a.H = g.h;
  a.W = g.w;
  a.P = P;
  a.cimg = c.cimg;
  a.ncb = cdiv(c.cimg, kCB);
  a.dil0 = g.dil0;
  a.dil1 = g.dil1;
  a.ksteps = pl.ksteps;
  a.kps = pl.kps;
  a.taps = g.taps;
  a.slab = (long long)c.M * P;
  a.accum = c.accum;
  a.accres = c.res;
  a.accmask = c.res_mask;
  a.accni = c.res_nimg;
  const dim3 block(256);
  if (!pl.sk) {
    if (pl.S > 1) {
      a.C = (float*)ws;
      a.bias = nullptr;
    }
    MSL_LAUNCH((k_igemm_fwd<64, 128, 16, 2, 2>), dim3(pl.tiles_n, pl.tiles_m, pl.S), block, 0, st, a);
    MSL_CHECK_LAUNCH();
    if (pl.S > 1) {
      const long long n = (long long)c.M * P;
      const int blocks = (int)std::min<long long>(cdiv(n, 256), 4096);
      MSL_LAUNCH(k_reduce_slabs, dim3(blocks), block, 0, st, (const float*)ws, pl.S, n, c.out, 0, c.bias, a.nbias, c.M,
                 P);
      MSL_CHECK_LAUNCH();
    }
    return MSL_OK;
  }
  const SkForm& f = pl.form;
  SkKernel* k = sk_kernel(f);
  SkArgs sk = pl.sched;
  sk.part = (float*)ws;
  const long long tiles = (long long)pl.tiles_m * pl.tiles_n;
  const dim3 grid(sk.tdp > 0 ? kSkNW : sk.NW), rgrid(f.bm * kSkBN / 1024, (unsigned)(tiles - sk.tdp));
  const bool f16 = f.mt == kMathH3P || f.mt == kMathH1P;
  if (f16 || f.mt == kMathX6P) {  // the weights' planes, behind the fp32 part of the pack
    const long long f32 = (long long)pl.ksteps * kCB * a.lda;
    a.Ax6 = reinterpret_cast<const __bf16*>(c.packed + f32);
    if (f16) a.ascale = c.packed + pack_tail_offset(f32) + kNPart;  // the pack's {sA, 1/sA}
  }
  if (f16) {  // the image's absmax partials: the caller's (msl_absmax_partials, a BN kernel) or k_absmax's
    a.bpart = c.img_part;
    a.bnpart = c.img_npart;
    if (!c.img_part) {
      float* part = ws_partials(ws, ws_bytes, 1);
      MSL_LAUNCH(k_absmax, dim3(kNPart), block, 0, st, c.img, (long long)c.cimg * P, 0LL, 1, part);
      MSL_CHECK_LAUNCH();
      a.bpart = part;
      a.bnpart = kNPart;
    }
  }
  if (f.bform == kBPre) {  // the image's fp16 planes, behind the pieces
    f16x8* planes = reinterpret_cast<f16x8*>((char*)ws + fwd_piece_bytes(g.taps, c.M));
    const long long n = (long long)a.ncb * 2 * P;
    const dim3 sgrid((unsigned)std::min<long long>(cdiv(n, 256), 8192));
    if (f.mt == kMathH1P)
      MSL_LAUNCH(k_split_img<1>, sgrid, block, 0, st, c.img, c.cimg, a.ncb, P, a.bpart, a.bnpart, planes);
    else
      MSL_LAUNCH(k_split_img<2>, sgrid, block, 0, st, c.img, c.cimg, a.ncb, P, a.bpart, a.bnpart, planes);
    MSL_CHECK_LAUNCH();
    a.Bx6 = planes;
  }
  MSL_LAUNCH_ENTRY(k->fn, k->bound, grid, block, 0, st, a, sk);
  MSL_CHECK_LAUNCH();
  if (pl.reduce) {
    switch (f.bm) {
      case 32: MSL_LAUNCH((k_sk_reduce<32, kSkBN>), rgrid, block, 0, st, a, sk); break;
      case 64: MSL_LAUNCH((k_sk_reduce<64, kSkBN>), rgrid, block, 0, st, a, sk); break;
      case 128: MSL_LAUNCH((k_sk_reduce<128, kSkBN>), rgrid, block, 0, st, a, sk); break;
      default: MSL_LAUNCH((k_sk_reduce<256, kSkBN>), rgrid, block, 0, st, a, sk); break;
    }
    MSL_CHECK_LAUNCH();
  }
  return MSL_OK;
}

// Weight gradient: stream-K over (tile, 64-pixel stage) (k_wgrad_sk + k_wsk_reduce).  Tiles by
// shape (the r01 tuning harness, profiles/r01_tune_wsk*.txt): 128x128 at one workgroup per CU for the
// 512-channel layer4 convs, 64x64 at two per CU below, 32-row tiles for the 19-class ASPP.
struct WgradPlan {
  int bm, bn, nw, tiles_m, tiles_n, ntap, KS, slots;
  bool rx6;        // k_wgrad_x6 (register-staged bf16x6, dY pre-split) with 16-pixel K-steps
  int lda;         // rx6: dY plane row length
  int nchunk, kchunk;  // rx6: chunked split-K (items = tiles x nchunk, kchunk K-steps each)
  long long T;
};

// k_wgrad_x6 with chunked split-K: the chunk count whose (tile, chunk) items fill whole rounds of
// 512 resident workgroups best, at least 8 K-steps per item.  Returns the fill (0 if none).
static double plan_chunks(long long ntiles, int KS, int& nchunk, int& kchunk) {
  double best = 0.0;
  nchunk = kchunk = 0;
  for (int C = 1; C <= KS && ntiles * C <= 4096; ++C) {
    const int L = cdiv(KS, C);
    if (L < 8) break;
    const int Ce = cdiv(KS, L);
    const long long items = ntiles * Ce;
    const double eff = (double)items / (double)(cdiv(items, 512LL) * 512);
    if (eff > best + 0.01) {
      best = eff;
      nchunk = Ce;
      kchunk = L;
    }
  }
  return best;
}

static WgradPlan plan_wgrad(int nbranch, int taps, int cin, int cout, int P, bool x6 = false, int w = 0) {
  WgradPlan pl;
  pl.rx6 = false;
  pl.lda = 0;
  pl.nchunk = 0;
  pl.kchunk = 0;
  int bk = kWskBK;
  const int ntap = nbranch * taps;
  int nchunk = 0, kchunk = 0;
  const bool rx6_ok = x6 && cout >= 128 && cin >= 128 && w >= 16;
  const double fill = rx6_ok ? plan_chunks((long long)cdiv(cout, 128) * cdiv(cin, 128) * ntap, cdiv(P, kWx6BK),
                                           nchunk, kchunk) : 0.0;
  if (rx6_ok && (fill >= 0.75 || (cout >= 256 && cin >= 256))) {
    // x6, >= 128 channels: k_wgrad_x6 (dY split once, 16-pixel K-steps, two workgroups per CU),
    // chunked split-K when its items fill the resident slots (layer3 77.6 us, layer4 274,
    // layer2 38.8; stream-K 86.5 / 306 / 44.1; k_wgrad_sk 110 / 395 / 41.0 -
    // profiles/r02_wgrad_x6.txt), else stream-K over 512 workers
    pl.bm = 128; pl.bn = 128; pl.nw = 512;
    pl.rx6 = true;
    pl.lda = pad_to(cout, kPackPad);
    bk = kWx6BK;
    if (fill >= 0.75) {
      pl.nchunk = nchunk;
      pl.kchunk = kchunk;
    }
  } else if (x6 && cout >= 128 && cin >= 128) {
    pl.bm = 128; pl.bn = 128; pl.nw = 256;
  } else if (cout <= 32) {
    pl.bm = 32; pl.bn = 128; pl.nw = 256;
  } else if (cout >= 512 && cin >= 512) {
    pl.bm = 128; pl.bn = 128; pl.nw = 256;
  } else {
    // layers 1-2 (<= 128 channels): 256 workers, fewer pieces per tile for the reduce (layer2
    // 41.5 vs 44.3 us, layer1 44.1 vs 47.7; profiles/r01_tune_wsks.txt)
    pl.bm = 64; pl.bn = 64; pl.nw = (cout <= 128 && cin <= 128) ? 256 : 512;
  }
  pl.tiles_m = cdiv(cout, pl.bm);
  pl.tiles_n = cdiv(cin, pl.bn);
  pl.ntap = ntap;
  pl.KS = cdiv(P, bk);
  pl.T = (long long)pl.tiles_m * pl.tiles_n * pl.ntap * pl.KS;
  pl.nw = (int)std::min<long long>(pl.nw, pl.T);
  // tiles a worker range can touch: its length (<= ceil(T/NW) stages) starting anywhere in a tile
  pl.slots = (int)((cdiv(pl.T, (long long)pl.nw) + pl.KS - 2) / pl.KS + 1);
  if (pl.nchunk > 0) {  // one piece per (tile, chunk) item
    pl.nw = (int)((long long)pl.tiles_m * pl.tiles_n * pl.ntap * pl.nchunk);
    pl.slots = 1;
  }
  return pl;
}

static size_t wgrad_piece_bytes(const WgradPlan& pl) { return (size_t)pl.nw * pl.slots * pl.bm * pl.bn * sizeof(float); }
// (+ two K-steps: k_wgrad_x6's loads one stage ahead read up to K-step KS + 1, unused)
static size_t wgrad_planes_bytes(const WgradPlan& pl) { return pl.rx6 ? (size_t)(pl.KS + 2) * 6 * pl.lda * 16 : 0; }

// ---------------------------------------------------------------- shared by 3x3 and pointwise
// A packed operand is the fp32 K-major pack [ksteps*16][lda] followed by its bf16x6 planes
// [ks][plane][k half][lda][8] (k_split_pack; 1.5x the fp32 bytes).  The planes are written by
// pack() when M > 64 - the 128-row tiles of the x6 form, the only reader - so the split runs
// once per weight update instead of once per conv call.
static long long packed_f32_elems(int nbranch, int taps, int cin, int cout, int for_dgrad) {
  const int cimg = for_dgrad ? cout : cin;
  const int m = for_dgrad ? cin : cout;
  return (long long)nbranch * cdiv(cimg, kCB) * taps * kCB * pad_to(m, kPackPad);
}

static long long packed_elems(int nbranch, int taps, int cin, int cout, int for_dgrad) {
  return pack_tail_offset(packed_f32_elems(nbranch, taps, cin, cout, for_dgrad)) + kPackTail;
}

// forms.pack_form: 1 = k_pack_split, 0 = k_pack + k_split_pack
static int pack(const float* w, long long branch_stride, int nbranch, int taps, int cin, int cout,
                int for_dgrad, float* packed, const msl_forms* forms, hipStream_t st) {
  if (forms_bad(forms)) return MSL_ERR_ARG;
  const int cimg = for_dgrad ? cout : cin;
  const int m = for_dgrad ? cin : cout;
  const long long total = packed_f32_elems(nbranch, taps, cin, cout, for_dgrad);
  const int lda = pad_to(m, kPackPad);
  const int ncb = cdiv(cimg, kCB);
  __bf16* planes = reinterpret_cast<__bf16*>(packed + total);
  // f16x3: fp16 planes for every M (the <= 64-row 3x3 / ASPP tiles run f16x3 too since r03)
  const bool h3 = forms_of(forms).f32_form == kMathH3P;
  float* tail = h3 ? packed + pack_tail_offset(total) : nullptr;
  // M <= 64 has no planes to split, and its 128-row padding is mostly zeros, which k_pack's
  // fully coalesced rows write faster (ASPP fwd 2048 -> 19: 5.2 vs 9.5 us)
  if (!h3 && (forms_of(forms).pack_form == 0 || m <= 64)) {  // element-wise gather, then a separate split
    const int blocks = (int)std::min<long long>(cdiv(total, 256), 8192);
    MSL_LAUNCH(k_pack, dim3(blocks), dim3(256), 0, st, w, branch_stride, cin, cout, for_dgrad,
                       ncb, lda, taps, total, packed);
    MSL_CHECK_LAUNCH();
    if (m > 64) {
      const int ksteps = nbranch * ncb * taps;
      MSL_LAUNCH(k_split_pack, dim3((int)std::min<long long>(cdiv(total, 256), 4096)), dim3(256),
                         0, st, packed, ksteps, lda, planes);
      MSL_CHECK_LAUNCH();
    }
    return MSL_OK;
  }
  // lda is a multiple of kPackPad (128): the m chunks tile it exactly, zero rows included
  static_assert(kPackPad % kPackTileM == 0, "pack tiles must cover lda");
  const dim3 grid(lda / kPackTileM, ncb, nbranch);
  const int split = m > 64 || h3;
  if (taps != 9 && taps != 1) return MSL_ERR_ARG;
  if (h3) {
    MSL_LAUNCH(k_absmax, dim3(kNPart), dim3(256), 0, st, w, (long long)cout * cin * taps, branch_stride,
                       nbranch, tail);
    MSL_CHECK_LAUNCH();
    MSL_LAUNCH(k_pack_scale, dim3(1), dim3(64), 0, st, tail);
    MSL_CHECK_LAUNCH();
  }
  if (taps == 9)
    MSL_LAUNCH(k_pack_split<9>, grid, dim3(256), 0, st, w, branch_stride, cin, cout, for_dgrad, ncb,
                       lda, split, packed, planes, tail);
  else
    MSL_LAUNCH(k_pack_split<1>, grid, dim3(256), 0, st, w, branch_stride, cin, cout, for_dgrad, ncb,
                       lda, split, packed, planes, tail);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

// Pointwise weight gradients with more output than input channels run with the operands swapped
// (WskArgs::trans): k_wgrad_x6 pre-splits the operand with fewer rows - the image instead of dY
// (256 -> 1024: a 256-row split instead of a 1024-row one, ~10 vs ~20 us) - and the reduce writes
// the dW^T tiles transposed.
static bool wgrad_swaps(int nbranch, int taps, int cin, int cout) { return nbranch == 1 && taps == 1 && cout > cin; }
// k_wgrad_x6's piece reduce in the [m][n] orientation: waves per 64 outputs (1 = k_wsk_reduce's single chain)
constexpr int kWskSplit = 4, kWskSplitMinPieces = 16;

static size_t wgrad_core_bytes(int nbranch, int taps, int cin, int cout, int P, int w) {
  // large enough for either fp32 form and orientation: pieces, then (k_wgrad_x6) the split planes
  size_t b = 0;
  for (int x6 = 0; x6 < 2; ++x6)
    for (int sw = 0; sw < 2; ++sw) {
      WgradPlan pl = sw ? plan_wgrad(nbranch, taps, cout, cin, P, x6 != 0, w)
                        : plan_wgrad(nbranch, taps, cin, cout, P, x6 != 0, w);
      b = std::max(b, wgrad_piece_bytes(pl) + wgrad_planes_bytes(pl));
    }
  return align_up(b, 16);
}

static size_t wgrad_ws_bytes(int nbranch, int taps, int cin, int cout, int P, int w) {
  // + (f16x3) both operands' per-row absmax partials when the caller passes none
  return wgrad_core_bytes(nbranch, taps, cin, cout, P, w) + align_up((size_t)(cin + cout) * 4, 16) + 16;
}

// ---- the choices of a weight-gradient call, shared by the launch (launch_wgrad) and the query
// (msl_conv_wgrad_plan): the math family's fp32-accurate split forms, the plan with its operand swap,
// the math each GEMM kernel is instantiated with, the piece reduce, the refusal and the scale mode.
constexpr bool wgrad_f16(int mt) { return mt == kMathH3P || mt == kMathH1P; }
constexpr bool wgrad_x6l(int mt) { return mt == kMathX6 || wgrad_f16(mt); }
// the math of the GEMM kernel a plan of math family `mt` launches: k_wgrad_x6 runs the family's split (fp16:
// its planes), k_wgrad_sk has no f16 form (x6 on its 128-row tile), and the split forms run only on 128x128
// tiles (plan_wgrad): exact f32 on the 64- and 32-row ones
constexpr int wgrad_gemm_math(int mt, bool rx6, int bm) {
  if (rx6) return wgrad_f16(mt) ? mt : kMathX6;
  if (bm == 128) return wgrad_f16(mt) ? kMathX6 : mt;
  return wgrad_x6l(mt) ? kMathF32 : mt;
}

// The plan of the call; trans: it runs with the operands swapped (the plan is then of (cout, cin))
static WgradPlan plan_wgrad_call(int mt, int nbranch, int taps, int cin, int cout, int P, int w, bool has_dbias,
                                 bool& trans) {
  const bool x6l = wgrad_x6l(mt);
  WgradPlan pl = plan_wgrad(nbranch, taps, cin, cout, P, x6l, w);
  trans = false;
  if (x6l && wgrad_swaps(nbranch, taps, cin, cout) && !has_dbias) {
    WgradPlan ps = plan_wgrad(nbranch, taps, cout, cin, P, true, w);
    if (ps.rx6) {  // dW^T = image . dY^T: M = cin (pre-split), N = cout
      pl = ps;
      trans = true;
    }
  }
  return pl;
}

// cin / cout as the plan sees them (after a swap): 32-bit index arithmetic, float pixel-row division in the kernel
static int wgrad_refusal(const WgradPlan& pl, int cin, int cout, int P) {
  if (pl.T * pl.nw >= (1LL << 31) || (long long)pl.nw * pl.slots * pl.bm * pl.bn * 4 >= (1LL << 31) ||
      (long long)std::max(cin, cout) * P >= (1LL << 29) || (long long)P + kWskBK >= (1LL << 22))
    return MSL_ERR_SHAPE;
  return MSL_OK;
}

enum WgradReduce { kWrSk32, kWrSk64, kWrWide64, kWrSk128, kWrSplit128 };
static unsigned wgrad_rgrid_x(const WgradPlan& pl, int taps) { return (unsigned)cdiv((long long)pl.bm * pl.bn / 4 * taps, 256); }
static unsigned wgrad_rgrid_y(const WgradPlan& pl, int nbranch) { return (unsigned)(pl.tiles_m * pl.tiles_n * nbranch); }
static WgradReduce wgrad_reduce(const WgradPlan& pl, int nbranch, int taps) {
  const long long ntiles = (long long)pl.tiles_m * pl.tiles_n * pl.ntap;
  // r06, k_wgrad_x6: S waves per 64 outputs, each summing every S-th piece (k_wsk_reduce_split), where a tile has >= 16
  // pieces (the 16- and 9-tile layer3 1x1 / layer2 3x3 gradients: 32-56 chunks; at 8 pieces, 512 -> 2048, it lost 4 us)
  const long long x6_pieces = pl.nchunk > 0 ? pl.nchunk : cdiv((long long)pl.nw, ntiles);
  // 64 x 64, few tiles with many pieces each (the 33k-px 1x1 gradients: 4 tiles x ~128 pieces): 8 threads per
  // output float4 (k_wsk_reduce_wide) instead of one serial chain of every piece
  const long long sk_pieces = cdiv((long long)pl.nw, std::max(1LL, pl.T / pl.KS));  // per (tile, tap)
  if (pl.rx6 && kWskSplit > 1 && x6_pieces >= kWskSplitMinPieces) return kWrSplit128;
  if (pl.bm == 128) return kWrSk128;
  if (pl.bm == 64 && (long long)wgrad_rgrid_x(pl, taps) * wgrad_rgrid_y(pl, nbranch) < 256 && sk_pieces >= 16)
    return kWrWide64;
  return pl.bm == 64 ? kWrSk64 : kWrSk32;
}

// one scale per row when both operands come with one maximum per row (M, N as the plan sees them)
static int wgrad_rowscale(int anpart, int M, int bnpart, int N) { return (anpart == M && bnpart == N) ? 1 : 0; }

template <int MT>
static int launch_wgrad(WgradCall c, void* ws, size_t ws_bytes, hipStream_t st) {
  const ConvGeom& g = c.g;
  const int P = g.nimg * g.h * g.w, taps = g.taps, nbranch = g.nbranch;
  constexpr bool F16 = wgrad_f16(MT);
  constexpr int MX = wgrad_gemm_math(MT, true, 128);  // k_wgrad_x6's
  if (ws_bytes < wgrad_ws_bytes(nbranch, taps, c.cin, c.cout, P, g.w)) return MSL_ERR_WORKSPACE;
  bool trans = false;
  const WgradPlan pl = plan_wgrad_call(MT, nbranch, taps, c.cin, c.cout, P, g.w, c.dbias != nullptr, trans);
  if (trans) {
    std::swap(c.x, c.dy);
    std::swap(c.x_part, c.dy_part);
    std::swap(c.x_npart, c.dy_npart);
    std::swap(c.cin, c.cout);
  }
  const int cin = c.cin, cout = c.cout;
  if (const int refused = wgrad_refusal(pl, cin, cout, P)) return refused;
  WskArgs a{};
  a.dy = c.dy;
  a.x = c.x;
  a.dw = c.dw;
  a.part = (float*)ws;
  a.M = cout;
  a.N = cin;
  a.H = g.h;
  a.W = g.w;
  a.P = P;
  a.dil0 = g.dil0;
  a.dil1 = g.dil1;
  a.taps = taps;
  a.accumulate = c.accumulate;
  a.slots = pl.slots;
  a.invW = 1.0f / (float)g.w;
  a.invH = 1.0f / (float)g.h;
  a.tiles_m = pl.tiles_m;
  a.tiles_n = pl.tiles_n;
  a.KS = pl.KS;
  a.NW = pl.nw;
  a.T = (int)pl.T;
  a.cbranch = (long long)cout * cin * taps;
  a.lda = pl.lda;
  a.nchunk = pl.nchunk;
  a.kchunk = pl.kchunk;
  a.ntiles = pl.tiles_m * pl.tiles_n * pl.ntap;
  a.trans = trans ? 1 : 0;
  const dim3 grid(pl.nw), block(256);
  const dim3 rgrid(wgrad_rgrid_x(pl, taps), wgrad_rgrid_y(pl, nbranch)), rblock(256);
  // the GEMM
  if (pl.rx6) {
    bf16x8* planes = reinterpret_cast<bf16x8*>((char*)ws + wgrad_piece_bytes(pl));
    a.dyx6 = planes;
    if constexpr (F16) {  // both operands' per-row absmax partials for the per-row scaled split
      // the caller's partials are one maximum per row (msl_absmax_partials, the BN kernels' per-
      // channel outputs); none given: reduce them here (after a swap the operands traded places)
      float* rp = reinterpret_cast<float*>((char*)ws + wgrad_core_bytes(nbranch, taps, cin, cout, P, g.w));
      a.apart = c.dy_part;
      a.anpart = c.dy_npart;
      if (!a.apart) {
        MSL_TRY(absmax_rows(c.dy, cout, P, rp, st));
        a.apart = rp;
        a.anpart = cout;
      }
      a.bpart = c.x_part;
      a.bnpart = c.x_npart;
      if (!a.bpart) {
        float* r2 = rp + align_up((size_t)cout, 4);
        MSL_TRY(absmax_rows(c.x, cin, P, r2, st));
        a.bpart = r2;
        a.bnpart = cin;
      }
      a.rowscale = wgrad_rowscale(a.anpart, cout, a.bnpart, cin);
    }
    MSL_LAUNCH(k_split_rows<MX>, dim3(pl.lda / kSplitRowsR, cdiv(pl.KS, 16)), block, 0, st, c.dy, cout, P, pl.KS,
               pl.lda, planes, a.apart, a.anpart, a.rowscale);
    MSL_CHECK_LAUNCH();
    MSL_LAUNCH(k_wgrad_x6<MX>, grid, block, 0, st, a);
  } else if (pl.bm == 128) {
    MSL_LAUNCH((k_wgrad_sk<128, 128, 2, 2, 2, wgrad_gemm_math(MT, false, 128)>), grid, block, 0, st, a);
  } else if (pl.bm == 64) {
    MSL_LAUNCH((k_wgrad_sk<64, 64, 2, 2, 2, wgrad_gemm_math(MT, false, 64)>), grid, block, 0, st, a);
  } else {
    MSL_LAUNCH((k_wgrad_sk<32, 128, 2, 1, 4, wgrad_gemm_math(MT, false, 32)>), grid, block, 0, st, a);
  }
  MSL_CHECK_LAUNCH();
  // the piece reduce
  switch (wgrad_reduce(pl, nbranch, taps)) {
    case kWrSplit128:
      MSL_LAUNCH((k_wsk_reduce_split<128, 128, kWskSplit>), dim3(cdiv(128LL * 128 / 4 * taps, 64), rgrid.y),
                 dim3(64 * kWskSplit), 0, st, a);
      break;
    case kWrSk128: MSL_LAUNCH((k_wsk_reduce<128, 128>), rgrid, rblock, 0, st, a); break;
    case kWrWide64:
      MSL_LAUNCH((k_wsk_reduce_wide<64, 64, 8>), dim3(cdiv((long long)64 * 64 / 4 * taps, 32), rgrid.y), rblock, 0, st, a);
      break;
    case kWrSk64: MSL_LAUNCH((k_wsk_reduce<64, 64>), rgrid, rblock, 0, st, a); break;
    case kWrSk32: MSL_LAUNCH((k_wsk_reduce<32, 128>), rgrid, rblock, 0, st, a); break;
  }
  MSL_CHECK_LAUNCH();
  if (c.dbias) {
    MSL_LAUNCH(k_bias_grad, dim3(cout), block, 0, st, c.dy, P, c.dbias, cout, nbranch, c.accumulate);
    MSL_CHECK_LAUNCH();
  }
  return MSL_OK;
}

// ---------------------------------------------------------------- the entry points' families
// Every conv entry point builds its call record and ends here.  fp32: the kernels of the call's f32_form,
// any valid forms; bf16: bf16 MFMA; fp16: BASELINE config 5's fp16 MFMA path on the f16x3 machinery - each
// operand tensor scaled by its power of two and rounded to fp16 once (the weights at pack time: the f16x3
// packs' hi planes, so the forms must name the f16x3 fp32 form, the default), one v_mfma_f32_32x32x16_f16
// per 16-deep slice, fp32 sums, the result unscaled exactly; its 64- / 32-row weight-gradient tiles run
// exact f32 MFMA.
enum Family { kFamF32, kFamBf16, kFamF16 };

// the family's math (plan_fwd), or -1 for forms it cannot run (MSL_ERR_ARG)
static int family_math(Family fam, const msl_forms* forms) {
  if (forms_bad(forms)) return -1;
  const int form = forms_of(forms).f32_form;
  if (fam == kFamF16) return form == kMathH3P ? kMathH1P : -1;
  return fam == kFamBf16 ? kMathBf16 : form;
}

static int run_fwd(Family fam, const FwdCall& c, const msl_forms* forms, void* ws, size_t ws_bytes,
                   msl_stream_t stream) {
  const int math = family_math(fam, forms);
  if (math < 0 || bad_fwd(c)) return MSL_ERR_ARG;
  return launch_fwd_form(math, c, forms, ws, ws_bytes, as_stream(stream));
}

static int run_wgrad(Family fam, const WgradCall& c, const msl_forms* forms, void* ws, size_t ws_bytes,
                     msl_stream_t stream) {
  const int math = family_math(fam, forms);
  if (math < 0 || bad_wgrad(c)) return MSL_ERR_ARG;
  hipStream_t st = as_stream(stream);
  switch (math) {
    case kMathH1P: return launch_wgrad<kMathH1P>(c, ws, ws_bytes, st);
    case kMathBf16: return launch_wgrad<kMathBf16>(c, ws, ws_bytes, st);
    case kMathH3P: return launch_wgrad<kMathH3P>(c, ws, ws_bytes, st);
    case kMathX6: return launch_wgrad<kMathX6>(c, ws, ws_bytes, st);
    default: return launch_wgrad<kMathF32>(c, ws, ws_bytes, st);
  }
}

// The three operations behind the entry points, each in every family and geometry
static int conv_fwd(Family fam, const ConvGeom& g, const float* x, const float* packed, const float* bias, float* y,
                    int cin, int cout, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream,
                    const float* x_part, int x_npart) {
  FwdCall c{};
  c.g = g;
  c.img = x;
  c.cimg = cin;
  c.packed = packed;
  c.bias = bias;
  c.out = y;
  c.M = cout;
  c.img_part = x_part;
  c.img_npart = x_npart;
  c.res_nimg = 1;
  return run_fwd(fam, c, forms, ws, ws_bytes, stream);
}

// res = null: dx (=|+=) W^T dy; else dx = mask(res) + W^T dy
static int conv_dgrad(Family fam, const ConvGeom& g, const float* dy, const float* packed_dgrad, float* dx, int cin,
                      int cout, int accumulate, const float* res, const unsigned long long* res_mask, int res_nimg,
                      const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream, const float* dy_part,
                      int dy_npart) {
  FwdCall c{};
  c.g = g;
  c.img = dy;
  c.cimg = cout;
  c.packed = packed_dgrad;
  c.out = dx;
  c.M = cin;
  c.accum = accumulate ? 1 : 0;
  c.img_part = dy_part;
  c.img_npart = dy_npart;
  c.res = res;
  c.res_mask = res_mask;
  c.res_nimg = res_nimg;
  return run_fwd(fam, c, forms, ws, ws_bytes, stream);
}

static int conv_wgrad(Family fam, const ConvGeom& g, const float* x, const float* dy, float* dw, float* dbias, int cin,
                      int cout, int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream,
                      const float* x_part, int x_npart, const float* dy_part, int dy_npart) {
  WgradCall c{};
  c.g = g;
  c.x = x;
  c.dy = dy;
  c.dw = dw;
  c.dbias = dbias;
  c.cin = cin;
  c.cout = cout;
  c.accumulate = accumulate;
  c.x_part = x_part;
  c.x_npart = x_npart;
  c.dy_part = dy_part;
  c.dy_npart = dy_npart;
  return run_wgrad(fam, c, forms, ws, ws_bytes, stream);
}

}  // namespace msl

using namespace msl;

extern "C" {

int msl_abi_version(void) { return MSL_ABI_VERSION; }

int msl_forms_default(msl_forms* out) {
  if (!out) return MSL_ERR_ARG;
  *out = kDefaultForms;
  return MSL_OK;
}

int msl_forms_check(const msl_forms* forms) { return forms_bad(forms) ? MSL_ERR_ARG : MSL_OK; }

int msl_launch_guard_probe(int threads, float* out, msl_stream_t stream) {
  if (threads < 1 || !out) return MSL_ERR_ARG;
  MSL_LAUNCH(k_guard_probe, dim3(1), dim3(threads), 0, as_stream(stream), out);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

const char* msl_status_string(int status) {
  switch (status) {
    case MSL_OK: return "ok";
    case MSL_ERR_SHAPE: return "invalid shape";
    case MSL_ERR_WORKSPACE: return "workspace too small";
    case MSL_ERR_ARG: return "invalid argument";
    case MSL_ERR_LAUNCH: return "block exceeds the kernel's launch bounds";
    default: return status > 0 ? hipGetErrorString((hipError_t)status) : "unknown error";
  }
}

// ------------------------------------------------------------------ packs, workspaces, queries
long long msl_dconv_packed_elems(int nbranch, int cin, int cout, int for_dgrad) {
  return packed_elems(nbranch, 9, cin, cout, for_dgrad);
}

int msl_dconv_pack(const float* w, long long branch_stride, int nbranch, int cin, int cout,
                   int for_dgrad, float* packed, const msl_forms* forms, msl_stream_t stream) {
  if (bad_dims(nbranch, cin, cout, 1, 1) || !w || !packed) return MSL_ERR_ARG;
  return pack(w, branch_stride, nbranch, 9, cin, cout, for_dgrad, packed, forms, as_stream(stream));
}

long long msl_conv_pack_blocks(int nbranch, int taps, int cin, int cout, int for_dgrad) {
  if (bad_dims(nbranch, cin, cout, 1, 1) || (taps != 1 && taps != 9)) return -1;
  const int cimg = for_dgrad ? cout : cin;
  const int m = for_dgrad ? cin : cout;
  const long long tiles = (long long)(pad_to(m, kPackPad) / kPackTileM) * cdiv(cimg, kCB) * nbranch;
  return taps == 1 ? cdiv(tiles, (long long)kPackSub<1>()) : tiles;  // blocks of msl_conv_pack_many
}

int msl_conv_pack_many(const msl_pack_job* jobs, const long long* block_start, int njobs, int taps,
                       long long total_blocks, const msl_forms* forms, msl_stream_t stream) {
  if (!jobs || !block_start || njobs < 1 || total_blocks < 1 || total_blocks >= (1LL << 31) ||
      (taps != 1 && taps != 9) || forms_bad(forms))
    return MSL_ERR_ARG;
  hipStream_t st = as_stream(stream);
  const int h3 = forms_of(forms).f32_form == kMathH3P;
  if (h3) {  // the weights' absmax partials first (jobs with M > 64: the split packs)
    if (taps == 9)
      MSL_LAUNCH(k_absmax_jobs<9>, dim3(kNPart, (unsigned)njobs), dim3(256), 0, st, jobs);
    else
      MSL_LAUNCH(k_absmax_jobs<1>, dim3(kNPart, (unsigned)njobs), dim3(256), 0, st, jobs);
    MSL_CHECK_LAUNCH();
    if (taps == 9)
      MSL_LAUNCH(k_pack_scale_jobs<9>, dim3((unsigned)njobs), dim3(64), 0, st, jobs);
    else
      MSL_LAUNCH(k_pack_scale_jobs<1>, dim3((unsigned)njobs), dim3(64), 0, st, jobs);
    MSL_CHECK_LAUNCH();
  }
  if (taps == 9)
    MSL_LAUNCH(k_pack_split_many<9>, dim3((unsigned)total_blocks), dim3(256), 0, st, jobs, block_start, njobs,
                       h3);
  else
    MSL_LAUNCH(k_pack_split_many<1>, dim3((unsigned)total_blocks), dim3(256), 0, st, jobs, block_start, njobs,
                       h3);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

// A pointwise conv is the 3x3 GEMM with one unshifted tap (dilation 0) over the flat pixel axis.
long long msl_pconv_packed_elems(int cin, int cout, int for_dgrad) {
  return packed_elems(1, 1, cin, cout, for_dgrad);
}

int msl_pconv_pack(const float* w, int cin, int cout, int for_dgrad, float* packed, const msl_forms* forms,
                   msl_stream_t stream) {
  if (bad_dims(1, cin, cout, 1, 1) || !w || !packed) return MSL_ERR_ARG;
  return pack(w, 0, 1, 1, cin, cout, for_dgrad, packed, forms, as_stream(stream));
}

size_t msl_dconv_fwd_workspace(int nbranch, int cin, int cout, int h, int w, int nimg) {
  if (bad_dims(nbranch, cin, cout, h, w, nimg)) return 0;
  return fwd_query_bytes(nbranch, 9, cin, cout, nimg * h * w);
}

size_t msl_dconv_dgrad_workspace(int nbranch, int cin, int cout, int h, int w, int nimg) {
  if (bad_dims(nbranch, cin, cout, h, w, nimg)) return 0;
  return fwd_query_bytes(nbranch, 9, cout, cin, nimg * h * w);
}

size_t msl_dconv_wgrad_workspace(int nbranch, int cin, int cout, int h, int w, int nimg) {
  if (bad_dims(nbranch, cin, cout, h, w, nimg)) return 0;
  return wgrad_ws_bytes(nbranch, 9, cin, cout, nimg * h * w, w);
}

size_t msl_pconv_fwd_workspace(int cin, int cout, int p) {
  if (bad_dims(1, cin, cout, 1, p)) return 0;
  return fwd_query_bytes(1, 1, cin, cout, p);
}

size_t msl_pconv_dgrad_workspace(int cin, int cout, int p) {
  if (bad_dims(1, cin, cout, 1, p)) return 0;
  return fwd_query_bytes(1, 1, cout, cin, p);
}

size_t msl_pconv_wgrad_workspace(int cin, int cout, int p) {
  if (bad_dims(1, cin, cout, 1, p)) return 0;
  return wgrad_ws_bytes(1, 1, cin, cout, p, p);
}

int msl_conv_wgrad_split(int nbranch, int taps, int cin, int cout, int h, int w, int nimg) {
  if (bad_dims(nbranch, cin, cout, h, w, nimg) || (taps != 1 && taps != 9)) return MSL_ERR_ARG;
  const int P = nimg * h * w;
  const int wr = taps == 1 ? P : w;  // a pointwise call passes one flat row (msl_pconv_wgrad*)
  if (wgrad_swaps(nbranch, taps, cin, cout) && plan_wgrad(nbranch, taps, cout, cin, P, true, wr).rx6) return 1;
  return plan_wgrad(nbranch, taps, cin, cout, P, true, wr).rx6 ? 1 : 0;
}

int msl_conv_fwd_form_count(void) { return (int)(sizeof(kSkKernels) / sizeof(kSkKernels[0])); }

int msl_conv_fwd_form_describe(int row, msl_conv_form* out) {
  if (row < 0 || row >= msl_conv_fwd_form_count() || !out) return MSL_ERR_ARG;
  const SkForm& f = kSkKernels[row].form;
  *out = {f.bm, f.G, f.stages, f.wm, f.wn, f.pw ? 1 : 0, f.mt, f.acc ? 1 : 0, f.bform};
  return MSL_OK;
}

int msl_conv_fwd_plan(int family, int nbranch, int taps, int cimg, int M, int P, int accumulate, int dil0,
                      const msl_forms* forms, msl_conv_fwd_plan_info* out) {
  if (family < kFamF32 || family > kFamF16 || !out) return MSL_ERR_ARG;
  const int math = family_math((Family)family, forms);
  // the geometries of the entry points: 3x3 with a dilation (one or two branches), one unshifted pointwise tap
  if (math < 0 || bad_dims(nbranch, cimg, M, 1, 1) || P < 1 || P > (1 << 30) ||
      !((taps == 9 && dil0 >= 1) || (taps == 1 && dil0 == 0 && nbranch == 1)))
    return MSL_ERR_ARG;
  const int accum = accumulate ? 1 : 0;
  const FwdPlan pl = plan_fwd(math, nbranch, taps, cimg, M, P, accum, dil0, forms);
  msl_conv_fwd_plan_info info{};
  info.row = -1;
  info.stream_k = pl.sk ? 1 : 0;
  info.math = kMathF32;  // the split-K tile kernel is exact f32 in every family
  info.tiles_m = pl.tiles_m;
  info.tiles_n = pl.tiles_n;
  info.ksteps = pl.ksteps;
  info.kps = pl.kps;
  info.S = pl.S;
  info.reduce = pl.sk ? (pl.reduce ? 1 : 0) : (pl.S > 1 ? 1 : 0);
  info.status = fwd_refusal(math, pl, cimg, M, P, accum);
  if (pl.sk) {
    if (SkKernel* k = sk_kernel(pl.form)) info.row = (int)(k - kSkKernels);
    info.math = pl.form.mt;
    info.tdp = pl.sched.tdp;
    info.NW = pl.sched.NW;
    info.T = pl.sched.T;
    info.split_img = pl.form.bform == kBPre ? 1 : 0;
  }
  *out = info;
  return MSL_OK;
}

int msl_conv_wgrad_plan(int family, int nbranch, int taps, int cin, int cout, int h, int w, int nimg, int has_dbias,
                        int x_npart, int dy_npart, const msl_forms* forms, msl_conv_wgrad_plan_info* out) {
  if (family < kFamF32 || family > kFamF16 || !out) return MSL_ERR_ARG;
  const int math = family_math((Family)family, forms);
  // the geometries of the entry points: 3x3 (one or two branches, with or without dbias), pointwise (neither)
  if (math < 0 || bad_dims(nbranch, cin, cout, h, w, nimg) || x_npart < 0 || dy_npart < 0 ||
      !(taps == 9 || (taps == 1 && nbranch == 1 && !has_dbias)))
    return MSL_ERR_ARG;
  const int P = nimg * h * w;
  const int wr = taps == 1 ? P : w;  // a pointwise call passes one flat row (geom_1x1)
  bool trans = false;
  const WgradPlan pl = plan_wgrad_call(math, nbranch, taps, cin, cout, P, wr, has_dbias != 0, trans);
  if (trans) {
    std::swap(cin, cout);
    std::swap(x_npart, dy_npart);
  }
  msl_conv_wgrad_plan_info info{};
  info.gemm = pl.rx6 ? 1 : 0;
  info.bm = pl.bm;
  info.bn = pl.bn;
  info.math = wgrad_gemm_math(math, pl.rx6, pl.bm);
  info.split_rows = pl.rx6 ? 1 : 0;
  info.reduce = (int)wgrad_reduce(pl, nbranch, taps);
  info.trans = trans ? 1 : 0;
  info.tiles_m = pl.tiles_m;
  info.tiles_n = pl.tiles_n;
  info.ntap = pl.ntap;
  info.KS = pl.KS;
  info.bk = pl.rx6 ? kWx6BK : kWskBK;
  info.NW = pl.nw;
  info.T = (int)pl.T;
  info.slots = pl.slots;
  info.nchunk = pl.nchunk;
  info.kchunk = pl.kchunk;
  info.swizzle = (pl.nw & 7) ? 0 : 1;
  info.status = wgrad_refusal(pl, cin, cout, P);
  // the longest run of K-steps of one tile in one worker's range, as the kernels cut them (sk_start)
  long long run = 0;
  if (pl.nchunk > 0) {
    run = std::min(pl.KS, pl.kchunk);
  } else if (info.status == MSL_OK) {
    for (long long wk = 0; wk < pl.nw; ++wk) {
      const long long b = wk * pl.T / pl.nw, e = (wk + 1) * pl.T / pl.nw;
      if (e - b >= 2LL * pl.KS - 1) run = pl.KS;  // holds a whole tile
      for (long long it = b; it < e && run < pl.KS;) {
        const long long k_a = it % pl.KS, nst = std::min<long long>(pl.KS - k_a, e - it);
        run = std::max(run, nst);
        it += nst;
      }
    }
  }
  info.max_run = (int)run;
  info.mask_tab = pl.rx6 && run + 3 <= kWxMaskTab ? 1 : 0;
  if (pl.rx6 && wgrad_f16(math))  // counts none given: one per row, reduced by the call
    info.rowscale = wgrad_rowscale(dy_npart ? dy_npart : cout, cout, x_npart ? x_npart : cin, cin);
  *out = info;
  return MSL_OK;
}

int msl_absmax_partials(const float* x, int rows, int row_len, float* part, msl_stream_t stream) {
  if (!x || !part || rows < 1 || row_len < 1) return MSL_ERR_ARG;
  return absmax_rows(x, rows, row_len, part, as_stream(stream));
}

// ------------------------------------------------------------------ fp32 math
// The _sc entry points take the operands' absmax partials ((pointer, count), NULL = computed where the
// form needs them); the plain ones are the same calls without partials.
int msl_dconv_fwd_sc(const float* x, const float* packed, const float* bias, float* y, int nbranch,
                     int cin, int cout, int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws,
                     size_t ws_bytes, msl_stream_t stream, const float* x_part, int x_npart) {
  return conv_fwd(kFamF32, geom_3x3(nbranch, h, w, nimg, dil0, dil1), x, packed, bias, y, cin, cout, forms, ws,
                  ws_bytes, stream, x_part, x_npart);
}

int msl_dconv_dgrad_sc(const float* dy, const float* packed_dgrad, float* dx, int nbranch, int cin,
                       int cout, int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws,
                       size_t ws_bytes, msl_stream_t stream, const float* dy_part, int dy_npart) {
  return conv_dgrad(kFamF32, geom_3x3(nbranch, h, w, nimg, dil0, dil1), dy, packed_dgrad, dx, cin, cout, 0, nullptr,
                    nullptr, 1, forms, ws, ws_bytes, stream, dy_part, dy_npart);
}

int msl_dconv_wgrad_sc(const float* x, const float* dy, float* dw, float* dbias, int nbranch, int cin,
                       int cout, int h, int w, int nimg, int dil0, int dil1, int accumulate, const msl_forms* forms, void* ws,
                       size_t ws_bytes, msl_stream_t stream, const float* x_part, int x_npart,
                       const float* dy_part, int dy_npart) {
  return conv_wgrad(kFamF32, geom_3x3(nbranch, h, w, nimg, dil0, dil1), x, dy, dw, dbias, cin, cout, accumulate,
                    forms, ws, ws_bytes, stream, x_part, x_npart, dy_part, dy_npart);
}

int msl_pconv_fwd_sc(const float* x, const float* packed, float* y, int cin, int cout, int p,
                     const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream, const float* x_part,
                     int x_npart) {
  return conv_fwd(kFamF32, geom_1x1(p), x, packed, nullptr, y, cin, cout, forms, ws, ws_bytes, stream, x_part,
                  x_npart);
}

int msl_pconv_dgrad_acc_sc(const float* dy, const float* packed_dgrad, float* dx, int cin, int cout, int p,
                           int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream,
                           const float* dy_part, int dy_npart) {
  return conv_dgrad(kFamF32, geom_1x1(p), dy, packed_dgrad, dx, cin, cout, accumulate, nullptr, nullptr, 1, forms,
                    ws, ws_bytes, stream, dy_part, dy_npart);
}

int msl_pconv_dgrad_resmask_sc(const float* dy, const float* packed_dgrad, float* dx, int cin, int cout, int p,
                               const float* res, const unsigned long long* res_mask, int nimg, const msl_forms* forms,
                               void* ws, size_t ws_bytes, msl_stream_t stream, const float* dy_part, int dy_npart) {
  if (!res) return MSL_ERR_ARG;
  return conv_dgrad(kFamF32, geom_1x1(p), dy, packed_dgrad, dx, cin, cout, 1, res, res_mask, nimg, forms, ws,
                    ws_bytes, stream, dy_part, dy_npart);
}

int msl_pconv_wgrad_sc(const float* x, const float* dy, float* dw, int cin, int cout, int p,
                       int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream, const float* x_part,
                       int x_npart, const float* dy_part, int dy_npart) {
  return conv_wgrad(kFamF32, geom_1x1(p), x, dy, dw, nullptr, cin, cout, accumulate, forms, ws, ws_bytes, stream,
                    x_part, x_npart, dy_part, dy_npart);
}

int msl_dconv_fwd(const float* x, const float* packed, const float* bias, float* y, int nbranch,
                  int cin, int cout, int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws,
                  size_t ws_bytes, msl_stream_t stream) {
  return msl_dconv_fwd_sc(x, packed, bias, y, nbranch, cin, cout, h, w, nimg, dil0, dil1, forms, ws, ws_bytes, stream,
                          nullptr, 0);
}

int msl_dconv_dgrad(const float* dy, const float* packed_dgrad, float* dx, int nbranch, int cin,
                    int cout, int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws,
                    size_t ws_bytes, msl_stream_t stream) {
  return msl_dconv_dgrad_sc(dy, packed_dgrad, dx, nbranch, cin, cout, h, w, nimg, dil0, dil1, forms, ws, ws_bytes,
                            stream, nullptr, 0);
}

int msl_dconv_wgrad(const float* x, const float* dy, float* dw, float* dbias, int nbranch, int cin,
                    int cout, int h, int w, int nimg, int dil0, int dil1, int accumulate, const msl_forms* forms, void* ws,
                    size_t ws_bytes, msl_stream_t stream) {
  return msl_dconv_wgrad_sc(x, dy, dw, dbias, nbranch, cin, cout, h, w, nimg, dil0, dil1, accumulate, forms, ws,
                            ws_bytes, stream, nullptr, 0, nullptr, 0);
}

int msl_pconv_fwd(const float* x, const float* packed, float* y, int cin, int cout, int p,
                  const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream) {
  return msl_pconv_fwd_sc(x, packed, y, cin, cout, p, forms, ws, ws_bytes, stream, nullptr, 0);
}

int msl_pconv_dgrad_acc(const float* dy, const float* packed_dgrad, float* dx, int cin, int cout, int p,
                        int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream) {
  return msl_pconv_dgrad_acc_sc(dy, packed_dgrad, dx, cin, cout, p, accumulate, forms, ws, ws_bytes, stream, nullptr,
                                0);
}

int msl_pconv_dgrad(const float* dy, const float* packed_dgrad, float* dx, int cin, int cout, int p,
                    const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream) {
  return msl_pconv_dgrad_acc(dy, packed_dgrad, dx, cin, cout, p, 0, forms, ws, ws_bytes, stream);
}

int msl_pconv_wgrad(const float* x, const float* dy, float* dw, int cin, int cout, int p,
                    int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream) {
  return msl_pconv_wgrad_sc(x, dy, dw, cin, cout, p, accumulate, forms, ws, ws_bytes, stream, nullptr, 0, nullptr, 0);
}

// ------------------------------------------------------------------ bf16 math
// Same operands, workspaces and results layout; products in bf16 (RNE from the fp32 operands),
// sums in fp32 (BASELINE config 5's fp16/bf16 MFMA path).  No partials, no accumulate epilogue.
int msl_dconv_fwd_bf16(const float* x, const float* packed, const float* bias, float* y, int nbranch,
                  int cin, int cout, int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws,
                  size_t ws_bytes, msl_stream_t stream) {
  return conv_fwd(kFamBf16, geom_3x3(nbranch, h, w, nimg, dil0, dil1), x, packed, bias, y, cin, cout, forms, ws,
                  ws_bytes, stream, nullptr, 0);
}

int msl_dconv_dgrad_bf16(const float* dy, const float* packed_dgrad, float* dx, int nbranch, int cin,
                    int cout, int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws,
                    size_t ws_bytes, msl_stream_t stream) {
  return conv_dgrad(kFamBf16, geom_3x3(nbranch, h, w, nimg, dil0, dil1), dy, packed_dgrad, dx, cin, cout, 0, nullptr,
                    nullptr, 1, forms, ws, ws_bytes, stream, nullptr, 0);
}

int msl_dconv_wgrad_bf16(const float* x, const float* dy, float* dw, float* dbias, int nbranch, int cin,
                    int cout, int h, int w, int nimg, int dil0, int dil1, int accumulate, const msl_forms* forms, void* ws,
                    size_t ws_bytes, msl_stream_t stream) {
  return conv_wgrad(kFamBf16, geom_3x3(nbranch, h, w, nimg, dil0, dil1), x, dy, dw, dbias, cin, cout, accumulate,
                    forms, ws, ws_bytes, stream, nullptr, 0, nullptr, 0);
}

int msl_pconv_fwd_bf16(const float* x, const float* packed, float* y, int cin, int cout, int p,
                  const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream) {
  return conv_fwd(kFamBf16, geom_1x1(p), x, packed, nullptr, y, cin, cout, forms, ws, ws_bytes, stream, nullptr, 0);
}

int msl_pconv_dgrad_bf16(const float* dy, const float* packed_dgrad, float* dx, int cin, int cout, int p,
                    const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream) {
  return conv_dgrad(kFamBf16, geom_1x1(p), dy, packed_dgrad, dx, cin, cout, 0, nullptr, nullptr, 1, forms, ws,
                    ws_bytes, stream, nullptr, 0);
}

int msl_pconv_wgrad_bf16(const float* x, const float* dy, float* dw, int cin, int cout, int p,
                    int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream) {
  return conv_wgrad(kFamBf16, geom_1x1(p), x, dy, dw, nullptr, cin, cout, accumulate, forms, ws, ws_bytes, stream,
                    nullptr, 0, nullptr, 0);
}

// ------------------------------------------------------------------ fp16 math
// Partials as in the _sc entry points.
int msl_dconv_fwd_f16(const float* x, const float* packed, const float* bias, float* y, int nbranch, int cin,
                      int cout, int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws, size_t ws_bytes,
                      msl_stream_t stream, const float* x_part, int x_npart) {
  return conv_fwd(kFamF16, geom_3x3(nbranch, h, w, nimg, dil0, dil1), x, packed, bias, y, cin, cout, forms, ws,
                  ws_bytes, stream, x_part, x_npart);
}

int msl_dconv_dgrad_f16(const float* dy, const float* packed_dgrad, float* dx, int nbranch, int cin, int cout,
                        int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws, size_t ws_bytes,
                        msl_stream_t stream, const float* dy_part, int dy_npart) {
  return conv_dgrad(kFamF16, geom_3x3(nbranch, h, w, nimg, dil0, dil1), dy, packed_dgrad, dx, cin, cout, 0, nullptr,
                    nullptr, 1, forms, ws, ws_bytes, stream, dy_part, dy_npart);
}

int msl_dconv_wgrad_f16(const float* x, const float* dy, float* dw, float* dbias, int nbranch, int cin, int cout,
                        int h, int w, int nimg, int dil0, int dil1, int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes,
                        msl_stream_t stream, const float* x_part, int x_npart, const float* dy_part, int dy_npart) {
  return conv_wgrad(kFamF16, geom_3x3(nbranch, h, w, nimg, dil0, dil1), x, dy, dw, dbias, cin, cout, accumulate,
                    forms, ws, ws_bytes, stream, x_part, x_npart, dy_part, dy_npart);
}

int msl_pconv_fwd_f16(const float* x, const float* packed, float* y, int cin, int cout, int p, const msl_forms* forms,
                      void* ws, size_t ws_bytes, msl_stream_t stream, const float* x_part, int x_npart) {
  return conv_fwd(kFamF16, geom_1x1(p), x, packed, nullptr, y, cin, cout, forms, ws, ws_bytes, stream, x_part,
                  x_npart);
}

int msl_pconv_dgrad_f16(const float* dy, const float* packed_dgrad, float* dx, int cin, int cout, int p,
                        int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream,
                        const float* dy_part, int dy_npart) {
  return conv_dgrad(kFamF16, geom_1x1(p), dy, packed_dgrad, dx, cin, cout, accumulate, nullptr, nullptr, 1, forms,
                    ws, ws_bytes, stream, dy_part, dy_npart);
}

int msl_pconv_dgrad_resmask_f16(const float* dy, const float* packed_dgrad, float* dx, int cin, int cout, int p,
                                const float* res, const unsigned long long* res_mask, int nimg, const msl_forms* forms,
                                void* ws, size_t ws_bytes, msl_stream_t stream, const float* dy_part, int dy_npart) {
  if (!res) return MSL_ERR_ARG;
  return conv_dgrad(kFamF16, geom_1x1(p), dy, packed_dgrad, dx, cin, cout, 1, res, res_mask, nimg, forms, ws,
                    ws_bytes, stream, dy_part, dy_npart);
}

int msl_pconv_wgrad_f16(const float* x, const float* dy, float* dw, int cin, int cout, int p, int accumulate, const msl_forms* forms,
                        void* ws, size_t ws_bytes, msl_stream_t stream, const float* x_part, int x_npart,
                        const float* dy_part, int dy_npart) {
  return conv_wgrad(kFamF16, geom_1x1(p), x, dy, dw, nullptr, cin, cout, accumulate, forms, ws, ws_bytes, stream,
                    x_part, x_npart, dy_part, dy_npart);
}

}  // extern "C"
