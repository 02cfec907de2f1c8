// PNG unfilter of one byte lane on the device (msl_png_unfilter_lane, include/msl_hip.h): the step between
// the host's inflate of a SYNTHIA label PNG and resize_label (datasets/synthia_Dataset.py).
//
// Filter types 1..4 make pixel x of row r depend on a = (r, x-1), b = (r-1, x), c = (r-1, x-1): serial
// along a row, serial down the rows.  The anti-diagonals are independent, so ONE workgroup runs a skewed
// wavefront, thread = row: at step t row r reconstructs pixel t - r; a is the thread's own last result,
// b what the row above produced one step earlier, c last step's b.  One byte per step moves from each
// row to the next:
//   - inside a wave it is a DPP shift of the whole wave by one lane (wave_shr:1), no LDS;
//   - between waves, wave k runs kLag = 2 blocks of kS = 64 steps behind wave k-1.  After a block the last
//     lane of a wave holds its row's kS results in registers and writes them to a ring in LDS at once; the
//     next wave reads them a block later, one per lane, and feeds them to its lane 0 by the opposite shift.
//     One __syncthreads() per kS steps orders that hand-over, not one per step.
// Images taller than the workgroup (kPngBand = 1024 rows) run as successive bands; the first row of a band reads
// the previous band's last OUTPUT row back from global memory, after a __syncthreads() (whose workgroup
// release / acquire makes one wave's stores visible to the others of the block).
//
// Loads and stores are staged through a per-wave LDS tile so that global memory sees rows, not columns:
// per block a wave reads, for each of its 64 rows, the 64 filtered bytes that row will use (64 lanes = 64
// consecutive pixels of one row); each thread then takes its own row out of the tile as 16 dwords, runs the
// kS steps in registers, puts 16 dwords of results into a second tile, and the wave writes them out row by
// row the same way.  The loads of the NEXT block ride inside the kS steps, one row per step, each stored to
// the input tile kAhead steps after it was issued, so their latency passes under the chain.  The tile rows are
// padded to 68 B so the dword accesses spread over the banks.  The tiles are private to their wave: between
// its phases only the wave's own lanes have to agree (wave_sync: LDS operations of one wave execute in order).
//
// Every trip count (bands, blocks per band, kS steps, 64 rows) and every barrier depends on (h, w) only:
// no data-dependent loop, no flag in memory, one workgroup.  Pixels outside [0, w) and rows outside
// [0, h) are never addressed: loads are clamped into the image and zeroed, stores predicated.
#include <type_traits>

#include "msl_internal.h"

namespace msl {

constexpr int kPngWaves = 16;               // waves of the workgroup
constexpr int kPngBand = 64 * kPngWaves;    // rows per band = threads
constexpr int kS = 64;                      // steps per block = bytes per hand-over
constexpr int kLag = 2;                     // blocks wave k runs behind wave k-1
constexpr int kPitch = 68;                  // bytes per tile row (64 + one dword of padding)
constexpr int kRing = 256;                  // ring bytes per wave boundary (a power of two >= 3 * kS)
constexpr int kDppWaveShl1 = 0x130, kDppWaveShr1 = 0x138;  // DPP controls: the whole wave one lane down / up

// orders the LDS accesses of this wave's lanes among themselves (no instruction: one wave's LDS
// operations execute in order; the compiler must not move them across)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int kTileBytes = 64 * kPitch;
constexpr size_t kPngLds = (size_t)kPngWaves * (2 * kTileBytes + kRing);  // above 64 KiB: dynamic, opted into at launch

__global__ void __launch_bounds__(kPngBand) k_png_unfilter_lane(const uint8_t* __restrict__ scan, int h, int w,
                                                                int bpp, int lane_b, size_t row_stride,
                                                                uint8_t* out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int L = threadIdx.x & 63;
  const int k = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // the wave: uniform, so row bases are scalar
  uint8_t* tin = lds + (size_t)k * kTileBytes;                // this wave's filtered bytes of a block, [row][lane]
  uint8_t* tout = lds + (size_t)(kPngWaves + k) * kTileBytes;  // its results of a block, the same layout
  // ring(k): what wave k-1 hands to wave k, pixel x of its last row at byte (x + 63) % kRing
  auto ring = [&](int wave) { return lds + (size_t)2 * kPngWaves * kTileBytes + (size_t)wave * kRing; };
  const int J = (w + 63 + kS - 1) / kS;  // blocks a wave needs: local steps 0 .. w - 1 + 63

  for (int band0 = 0; band0 < h; band0 += kPngBand) {
    const int rows = min(h - band0, kPngBand);
    const int nw = (rows + 63) >> 6;  // waves with rows in this band
    const int G = J + kLag * (nw - 1);
    const int row0 = band0 + k * 64;
    int ft = row0 + L < h ? scan[(size_t)(row0 + L) * row_stride] : 0;
    if (ft > 4) ft = 0;
    // the predictor without a branch: ((a & m_a) + (b & m_b)) >> half is 0, a, b, (a + b) >> 1 for types 0..3
    const int m_a = (ft == 1 || ft == 3) ? 0xff : 0, m_b = (ft == 2 || ft == 3) ? 0xff : 0, half = ft == 3 ? 1 : 0;
    const bool paeth = ft == 4;
    int cur = 0, bprev = 0;  // this row's last result (a) and last step's b (c)
    int pre_top = 0;         // band's first wave: the output row above the band, lane = pixel 64 j + lane

    // Row i of block j as the wave loads it: lane = pixel 64 j - i + lane.  A uniform row base and a 32-bit lane
    // offset, both clamped into the image; a lane outside it loads a byte it does not use and stores 0.
    // (r0 = row0, made opaque once per block: what the 64 rows derive from it is scalar work of a few
    // instructions each, and kept across blocks it would cost some 250 scalar registers)
    int r0 = row0;
    auto row_base = [&](int i) { return scan + (size_t)min(r0 + i, h - 1) * row_stride + 1 + lane_b; };
    auto load_at = [&](const uint8_t* base, int j, int i) -> int {
      return base[(uint32_t)__umul24(min(max(kS * j - i + L, 0), w - 1), bpp)];  // both factors under 2^16
    };
    auto load_row = [&](int j, int i) -> int { return load_at(row_base(i), j, i); };
    auto put_row = [&](int j, int i, int v) {
      const int x = kS * j - i + L;
      tin[i * kPitch + L] = (r0 + i < h && (unsigned)x < (unsigned)w) ? (uint8_t)v : (uint8_t)0;
    };
    auto load_top = [&](int j) {
      if (k == 0 && band0 > 0) pre_top = (out + (size_t)(band0 - 1) * w)[(uint32_t)min(kS * j + L, w - 1)];
    };
    // a wave's first block of a band: nothing to hide the loads behind
    auto fill = [&](int j) {
      for (int i0 = 0; i0 < 64; i0 += 16) {
        int v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = load_row(j, i0 + i);
#pragma unroll
        for (int i = 0; i < 16; ++i) put_row(j, i0 + i, v[i]);
      }
      load_top(j);
    };
    auto active = [&](int g) { return k < nw && g - kLag * k >= 0 && g - kLag * k < J; };  // wave-uniform
    auto run_block = [&](int j, auto with_next) {
      constexpr bool kNext = decltype(with_next)::value;
      int top = kS * j + L < w ? pre_top : 0;  // lane s: the row above this wave's first row, pixel 64 j + s
      if (k > 0) top = ring(k)[(kS * j + L + 63) & (kRing - 1)];
      wave_sync();  // the block's bytes are in the tile
      uint32_t d[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) d[q] = *reinterpret_cast<const uint32_t*>(tin + L * kPitch + 4 * q);
      wave_sync();  // every row has left the tile: the next block's bytes may come in, kAhead steps after their loads
      if (kNext) load_top(j + 1);
      constexpr int kAhead = kPngWaves > 8 ? 8 : 16;  // steps between a row's load and its store to the tile
      int ld[kAhead];
      uint32_t acc = 0;
      const uint8_t* base = row_base(0);
      // No range test per step: a pixel left of the row (x < 0) has f = 0 from the tile and a = b = c = 0, so
      // every filter gives 0, the neighbour the first pixel needs; what is computed right of the row (x >= w)
      // is only ever read by pixels right of the row, and never stored.
#pragma unroll
      for (int s = 0; s < kS; ++s) {
        if (kNext) {
          if (s >= kAhead) put_row(j + 1, s - kAhead, ld[s % kAhead]);
          ld[s % kAhead] = load_at(base, j + 1, s);
          base += r0 + s + 1 < h ? row_stride : 0;  // the next row's base, clamped like row_base
        }
        const int f = (d[s >> 2] >> (8 * (s & 3))) & 0xff;
        // b: the row above, one lane up; lane 0 keeps `top`, its own row above.  Then the next pixel of that row
        // moves to lane 0 (off the chain; what the last lane keeps never gets there within the block)
        const int b = __builtin_amdgcn_update_dpp(top, cur, kDppWaveShr1, 0xf, 0xf, false);
        top = __builtin_amdgcn_update_dpp(top, top, kDppWaveShl1, 0xf, 0xf, false);
        const int a = cur, c = bprev;
        // Paeth: p = a + b - c; the nearest of a, b, c to p, ties in that order: pa = |b - c|, pb = |a - c|,
        // pc = |a + b - 2 c|, each one v_sad_u16 on operands under 2^16
        const uint32_t pa = __builtin_amdgcn_sad_u16(b, c, 0), pb = __builtin_amdgcn_sad_u16(a, c, 0),
                       pc = __builtin_amdgcn_sad_u16(a + b, 2 * c, 0);
        const int pp = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
        const int lin = ((a & m_a) + (b & m_b)) >> half;
        cur = (f + (paeth ? pp : lin)) & 0xff;
        bprev = b;
        acc = __builtin_amdgcn_alignbyte((uint32_t)cur, acc, 1);  // results enter at the top byte: 4 steps fill a dword
        if ((s & 3) == 3) d[s >> 2] = acc;
      }
      if (kNext) {
#pragma unroll
        for (int s = kS; s < kS + kAhead; ++s) put_row(j + 1, s - kAhead, ld[s % kAhead]);
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) *reinterpret_cast<uint32_t*>(tout + L * kPitch + 4 * q) = d[q];
      // the last lane's d[] is its row's pixels 64 j - 63 .. 64 j: ring bytes 64 j .. 64 j + 63
      if (L == 63 && k + 1 < nw) {
        uint32_t* hand = reinterpret_cast<uint32_t*>(ring(k + 1) + ((kS * j) & (kRing - 1)));
#pragma unroll
        for (int q = 0; q < 16; ++q) hand[q] = d[q];
      }
    };
    if (active(0)) fill(0);

    for (int g = 0; g < G; ++g) {
      const int j = g - kLag * k;
      const bool on = active(g), next = active(g + 1);
      asm volatile("" : "+s"(r0));
      if (on) {
        // two copies of the block, with and without the next block's loads riding in it: a test per step would
        // cut the steps into basic blocks, and the loads' counted waits do not survive those
        if (next)
          run_block(j, std::true_type{});
        else
          run_block(j, std::false_type{});
      } else if (next) {
        fill(j + 1);
      }
      __syncthreads();  // the hand-over (and, for this wave, results in the tile before they are read by row)
      if (on) {
#pragma unroll 16
        for (int i = 0; i < 64; ++i) {
          const int r = r0 + i, x = kS * j - i + L;
          if (r < h && x >= 0 && x < w) (out + (size_t)r * w)[(uint32_t)x] = tout[i * kPitch + L];
        }
      }
    }
    __syncthreads();  // the band's last output row is read by the next band's first wave
  }
}

}  // namespace msl

using namespace msl;

extern "C" {

int msl_png_unfilter_band_rows(void) { return kPngBand; }

int msl_png_unfilter_lane(const uint8_t* scan, int h, int w, int bpp, int lane, size_t row_stride, uint8_t* out,
                          msl_stream_t stream) {
  if (!scan || !out || h < 1 || w < 1 || h > 65535 || w > 65535 || bpp < 1 || bpp > 8 || lane < 0 || lane >= bpp ||
      row_stride < 1 + (size_t)w * bpp)
    return MSL_ERR_ARG;
  // two tiles per wave pass the 64 KiB a kernel gets unasked (of the CU's 160 KiB): opt in, once per process
  static std::atomic<int> opted{0};
  if (!opted.load(std::memory_order_acquire)) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_png_unfilter_lane),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPngLds);
    if (e != hipSuccess) return (int)e;
    opted.store(1, std::memory_order_release);
  }
  MSL_LAUNCH(k_png_unfilter_lane, dim3(1), dim3(kPngBand), kPngLds, as_stream(stream), scan, h, w, bpp, lane, row_stride,
             out);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

}  // extern "C"
