// Baseline JPEG decode (msl_jpeg_*, include/msl_hip.h): the host entry points over jpeg_host.h, and the device
// half - everything after the Huffman decode - as two launches, byte-exact against libjpeg-turbo's defaults
// (JDCT_ISLOW, fancy upsampling), that is against Pillow.
//
// Launch 1, k_jpeg_idct: 8 threads per 8x8 block, 32 blocks per workgroup.  Thread r of a block loads row r of the
// block's coefficients as one 16-byte load (a wave reads 1 KiB of consecutive coefficients) and the same row
// of the quantisation table, multiplies, and the block is transposed through the wave's own LDS so that thread
// c runs jidctint.c's column pass on column c; transposed back, thread r runs the row pass on row r and stores
// its 8 clamped bytes at once into the component's plane of whole blocks.  A block never leaves its wave, so
// the three hand-overs need the wave's own ordering only (wave_sync), no barrier.
//
// Accumulator width.  jidctint.c's passes are sums and products, one DESCALE at the end of each: computed
// in uint32_t they are exact modulo 2^32, so the result is libjpeg's whenever the value a DESCALE shifts fits
// int32, whatever the intermediates did.  Each such value is sum_k m_k in_k over the pass's 8 inputs with
// |m_k| <= 11363 (the largest multiplier of the flow graph, FIX(sqrt(2) cos(pi/16))), plus the rounding term:
//   column pass:  11363 * sum|x| + 2^10 < 2^31        for a column of dequantised values with sum|x| < 188 000;
//   row pass:     its inputs are |ws| <= 11363 * sum_column|x| / 2^11 + 1, so 11363 * sum_row|ws| + 2^17 < 2^31
//                 for a block with sum|x| < 34 000.
// A block an encoder made from 8-bit samples has sum|F| <= 8 * sqrt(sum F^2) = 8 * sqrt(64 * 128^2) = 8192 for its
// true DCT F (the DCT is orthonormal), and a quantised coefficient that is not zero has |x| <= 2 |F|: sum|x| <=
// 16 384, quality 100 on 0/255 noise included - half the bound.  Beyond it (a corrupt stream) the arithmetic
// wraps modulo 2^32, the same in utils/jpeg.py's restatement: defined, and no longer libjpeg's (whose SIMD and
// C paths differ from each other there).  coefficient * table entry is int16 * uint16: it fits int32.
//
// Launch 2, k_jpeg_rgb: a thread makes 4 consecutive pixels of the flat [height * width] raster - 12 bytes, three
// dword stores, 768 consecutive bytes per wave whatever the width - from the planes: Y as it is, the chroma
// sample by libjpeg-turbo's rule for the file's sampling (jdsample.c), the colour by jdcolor.c's fixed point.
// Only samples inside the component's true size ceil(W h / hmax) x ceil(H v / vmax) enter a filter.
#include "jpeg_host.h"
#include "msl_internal.h"

namespace msl {

constexpr int kIdctThreads = 256;
constexpr int kIdctBlocks = kIdctThreads / 8;  // 8x8 blocks per workgroup
constexpr int kTilePitch = 72;                 // ints per block in LDS: 64 + 8, so a wave's 8 blocks spread over the banks
constexpr int kRgbThreads = 256;
constexpr int kRgbPixels = 4;                  // per thread
constexpr size_t kPlaneAlign = 256;

__device__ __forceinline__ void jpeg_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// jidctint.c's 1-D pass (CONST_BITS 13), modulo 2^32; out[k] = DESCALE(., SH)
template <int SH>
__device__ __forceinline__ void idct8(const int32_t* in, int32_t* out) {
  using u = uint32_t;
  const u i0 = in[0], i1 = in[1], i2 = in[2], i3 = in[3], i4 = in[4], i5 = in[5], i6 = in[6], i7 = in[7];
  u z1 = (i2 + i6) * 4433u;
  const u t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u;
  const u t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
  const u t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  u a0 = i7, a1 = i5, a2 = i3, a3 = i1;
  z1 = a0 + a3;
  u z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const u z5 = (z3 + z4) * 9633u;
  a0 *= 2446u;
  a1 *= 16819u;
  a2 *= 25172u;
  a3 *= 12299u;
  z1 = 0u - z1 * 7373u;
  z2 = 0u - z2 * 20995u;
  z3 = z5 - z3 * 16069u;
  z4 = z5 - z4 * 3196u;
  a0 += z1 + z3;
  a1 += z2 + z4;
  a2 += z2 + z3;
  a3 += z1 + z4;
  constexpr u half = 1u << (SH - 1);
  out[0] = (int32_t)(t10 + a3 + half) >> SH;
  out[7] = (int32_t)(t10 - a3 + half) >> SH;
  out[1] = (int32_t)(t11 + a2 + half) >> SH;
  out[6] = (int32_t)(t11 - a2 + half) >> SH;
  out[2] = (int32_t)(t12 + a1 + half) >> SH;
  out[5] = (int32_t)(t12 - a1 + half) >> SH;
  out[3] = (int32_t)(t13 + a0 + half) >> SH;
  out[4] = (int32_t)(t13 - a0 + half) >> SH;
}

struct IdctArgs {
  int end[3];       // one past the last global block index of each component
  int blocks_w[3];
  int tq[3];
  uint32_t plane[3];  // byte offset of the component's plane in the workspace
  int total;
};

__global__ void __launch_bounds__(kIdctThreads) k_jpeg_idct(const int16_t* __restrict__ coef,
                                                            const uint16_t* __restrict__ quant, IdctArgs a,
                                                            uint8_t* __restrict__ planes) {
  __shared__ __attribute__((aligned(16))) int32_t tile[kIdctBlocks * kTilePitch];
  const int r = threadIdx.x & 7, bl = threadIdx.x >> 3;
  const int g = blockIdx.x * kIdctBlocks + bl;
  const bool live = g < a.total;
  const int gg = live ? g : a.total - 1;  // a lane past the last block works on the last one and stores nothing
  const int c = (gg >= a.end[0]) + (gg >= a.end[1]);
  const int local = gg - (c == 0 ? 0 : a.end[c - 1]);
  const int bw = a.blocks_w[c];
  const int brow = local / bw, bcol = local - brow * bw;
  int32_t* mine = tile + bl * kTilePitch;

  const uint4 raw = *reinterpret_cast<const uint4*>(coef + (size_t)gg * 64 + r * 8);
  const uint4 qv = *reinterpret_cast<const uint4*>(quant + a.tq[c] * 64 + r * 8);
  const uint32_t rw[4] = {raw.x, raw.y, raw.z, raw.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
  int32_t v[8], o[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[2 * j] = (int32_t)(int16_t)(rw[j] & 0xffffu) * (int32_t)(qw[j] & 0xffffu);
    v[2 * j + 1] = (int32_t)(int16_t)(rw[j] >> 16) * (int32_t)(qw[j] >> 16);
  }
  *reinterpret_cast<int4*>(mine + r * 8) = make_int4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<int4*>(mine + r * 8 + 4) = make_int4(v[4], v[5], v[6], v[7]);
  jpeg_wave_sync();  // the block's 8 rows are in the tile
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = mine[k * 8 + r];
  idct8<11>(v, o);   // column r (CONST_BITS - PASS1_BITS)
  jpeg_wave_sync();  // every column has left the tile
#pragma unroll
  for (int k = 0; k < 8; ++k) mine[k * 8 + r] = o[k];
  jpeg_wave_sync();
  const int4 lo = *reinterpret_cast<const int4*>(mine + r * 8), hi = *reinterpret_cast<const int4*>(mine + r * 8 + 4);
  v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w, v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
  idct8<18>(v, o);  // row r (CONST_BITS + PASS1_BITS + 3)
  uint32_t w0 = 0, w1 = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w0 |= (uint32_t)min(max(o[k] + 128, 0), 255) << (8 * k);
    w1 |= (uint32_t)min(max(o[k + 4] + 128, 0), 255) << (8 * k);
  }
  if (live)
    *reinterpret_cast<uint2*>(planes + a.plane[c] + ((size_t)brow * 8 + r) * ((size_t)bw * 8) + (size_t)bcol * 8) =
        make_uint2(w0, w1);
}

struct RgbArgs {
  int w, h, ncomp;
  int hs, vs;         // luma sampling = the chroma planes' subsampling
  int cw, ch;         // true size of a chroma plane
  int fancy;          // libjpeg selects the fancy upsamplers only for cw > 2
  uint32_t plane[3];
  int pitch[3];
  int aligned;        // rgb is dword aligned
};

// the chroma sample of pixel (x, y) from plane p (jdsample.c: fullsize, h2v1 / h2v2 box, h2v1_fancy, h2v2_fancy)
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int pitch, const RgbArgs& a, int x, int y) {
  if (a.hs == 1) return p[(size_t)y * pitch + x];
  const int i = x >> 1;
  if (!a.fancy) return p[(size_t)(a.vs == 2 ? y >> 1 : y) * pitch + i];
  const int im = max(i - 1, 0), ip = min(i + 1, a.cw - 1);
  if (a.vs == 1) {
    const uint8_t* row = p + (size_t)y * pitch;
    const int s = row[i];
    if (x & 1) return i == a.cw - 1 ? s : (3 * s + row[ip] + 2) >> 2;
    return i == 0 ? s : (3 * s + row[im] + 1) >> 2;
  }
  const int ir = y >> 1;
  const uint8_t* near = p + (size_t)ir * pitch;
  const uint8_t* far = p + (size_t)((y & 1) ? min(ir + 1, a.ch - 1) : max(ir - 1, 0)) * pitch;
  const int cs = 3 * near[i] + far[i];
  if (x & 1) return i == a.cw - 1 ? (4 * cs + 7) >> 4 : (3 * cs + 3 * near[ip] + far[ip] + 7) >> 4;
  return i == 0 ? (4 * cs + 8) >> 4 : (3 * cs + 3 * near[im] + far[im] + 8) >> 4;
}

__device__ __forceinline__ uint32_t clamp255(int v) { return (uint32_t)min(max(v, 0), 255); }

__global__ void __launch_bounds__(kRgbThreads) k_jpeg_rgb(const uint8_t* __restrict__ planes, RgbArgs a,
                                                          uint8_t* __restrict__ rgb, uint32_t npix) {
  const uint32_t p0 = (blockIdx.x * (uint32_t)kRgbThreads + threadIdx.x) * kRgbPixels;
  if (p0 >= npix) return;
  int y = (int)(p0 / (uint32_t)a.w), x = (int)(p0 - (uint32_t)y * (uint32_t)a.w);
  const int n = (int)min((uint32_t)kRgbPixels, npix - p0);
  uint32_t px[kRgbPixels];  // R | G << 8 | B << 16
#pragma unroll
  for (int j = 0; j < kRgbPixels; ++j) {
    px[j] = 0;
    if (j < n) {
      const int Y = planes[a.plane[0] + (size_t)y * a.pitch[0] + x];
      if (a.ncomp == 1) {
        px[j] = (uint32_t)Y * 0x010101u;
      } else {
        const int cb = chroma_at(planes + a.plane[1], a.pitch[1], a, x, y) - 128;
        const int cr = chroma_at(planes + a.plane[2], a.pitch[2], a, x, y) - 128;
        // jdcolor.c: FIX(1.402) = 91881, FIX(1.772) = 116130, FIX(0.34414) = 22554, FIX(0.71414) = 46802, ONE_HALF = 32768
        const int R = Y + ((91881 * cr + 32768) >> 16);
        const int B = Y + ((116130 * cb + 32768) >> 16);
        const int G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
        px[j] = clamp255(R) | clamp255(G) << 8 | clamp255(B) << 16;
      }
      if (++x == a.w) {
        x = 0;
        ++y;
      }
    }
  }
  uint8_t* out = rgb + (size_t)p0 * 3;
  if (n == kRgbPixels && a.aligned) {
    uint32_t* o = reinterpret_cast<uint32_t*>(out);
    o[0] = px[0] | px[1] << 24;
    o[1] = px[1] >> 8 | px[2] << 16;
    o[2] = px[2] >> 16 | px[3] << 8;
  } else {
#pragma unroll
    for (int j = 0; j < kRgbPixels; ++j) {
      if (j < n) {
        out[3 * j] = (uint8_t)px[j];
        out[3 * j + 1] = (uint8_t)(px[j] >> 8);
        out[3 * j + 2] = (uint8_t)(px[j] >> 16);
      }
    }
  }
}

static size_t plane_bytes(const msl_jpeg_comp& c) {
  return align_up((size_t)c.blocks_w * 8 * (size_t)c.blocks_h * 8, kPlaneAlign);
}

}  // namespace msl

using namespace msl;

extern "C" {

int msl_jpeg_info(const uint8_t* file, size_t n, msl_jpeg_header* header) { return jpeg::info(file, n, header); }

size_t msl_jpeg_coef_elems(const msl_jpeg_header* header) {
  return header && jpeg::check_header(*header) == MSL_OK ? jpeg::coef_elems(*header) : 0;
}

int msl_jpeg_entropy_decode(const uint8_t* file, size_t n, msl_jpeg_header* header, int16_t* coef, size_t coef_elems,
                            uint16_t* quant) {
  return jpeg::entropy_decode(file, n, header, coef, coef_elems, quant);
}

size_t msl_jpeg_workspace(const msl_jpeg_header* header) {
  if (!header || jpeg::check_header(*header) != MSL_OK) return 0;
  size_t b = 0;
  for (int c = 0; c < header->ncomp; ++c) b += plane_bytes(header->comp[c]);
  return b;
}

int msl_jpeg_tile_blocks(void) { return kIdctBlocks; }
int msl_jpeg_tile_pixels(void) { return kRgbThreads * kRgbPixels; }

int msl_jpeg_reconstruct(const int16_t* coef, const uint16_t* quant, const msl_jpeg_header* header, uint8_t* rgb,
                         void* ws, size_t ws_bytes, msl_stream_t stream) {
  if (!coef || !quant || !header || !rgb || !ws) return MSL_ERR_ARG;
  if (jpeg::check_header(*header) != MSL_OK) return MSL_ERR_ARG;
  if (((uintptr_t)coef & 15) || ((uintptr_t)quant & 15) || ((uintptr_t)ws & 15)) return MSL_ERR_ARG;
  const msl_jpeg_header& h = *header;
  if (ws_bytes < msl_jpeg_workspace(header)) return MSL_ERR_ARG;
  if ((long long)h.width * h.height > (1ll << 28)) return MSL_ERR_SHAPE;
  IdctArgs ia = {};
  RgbArgs ra = {};
  size_t off = 0;
  long long blocks = 0;
  for (int c = 0; c < 3; ++c) {
    if (c < h.ncomp) {
      blocks += (long long)h.comp[c].blocks_w * h.comp[c].blocks_h;
      ia.blocks_w[c] = h.comp[c].blocks_w;
      ia.tq[c] = h.comp[c].tq;
      ia.plane[c] = ra.plane[c] = (uint32_t)off;
      ra.pitch[c] = h.comp[c].blocks_w * 8;
      off += plane_bytes(h.comp[c]);
    } else {
      ia.blocks_w[c] = 1;
    }
    ia.end[c] = (int)blocks;
  }
  if (blocks > (1ll << 24) || off > 0xffffffffull) return MSL_ERR_SHAPE;  // (2^28 pixels: at most 3 * 2^22 blocks and a little)
  ia.total = (int)blocks;
  ra.w = h.width;
  ra.h = h.height;
  ra.ncomp = h.ncomp;
  ra.hs = h.hmax;
  ra.vs = h.vmax;
  ra.cw = (h.width + h.hmax - 1) / h.hmax;
  ra.ch = (h.height + h.vmax - 1) / h.vmax;
  ra.fancy = ra.cw > 2;
  ra.aligned = ((uintptr_t)rgb & 3) == 0;
  const uint32_t npix = (uint32_t)h.width * (uint32_t)h.height;
  uint8_t* planes = static_cast<uint8_t*>(ws);
  MSL_LAUNCH(k_jpeg_idct, dim3(cdiv(blocks, kIdctBlocks)), dim3(kIdctThreads), 0, as_stream(stream), coef, quant, ia,
             planes);
  MSL_CHECK_LAUNCH();
  MSL_LAUNCH(k_jpeg_rgb, dim3(cdiv(npix, kRgbThreads * kRgbPixels)), dim3(kRgbThreads), 0, as_stream(stream),
             (const uint8_t*)planes, ra, rgb, npix);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

}  // extern "C"
