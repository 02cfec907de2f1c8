// Training-time evaluation: the argmax of the upsampled prediction and the
// class confusion matrix, on device.  The reference copies the 19 x H x W fp32 prediction and the
// label to the host every iteration, takes np.argmax over classes and bins
// num_class * gt + pred with np.bincount (tools/train_source.py:280-283, utils/eval.py:109-115).
//
// One thread per pixel: first-max argmax over the C class planes (np.argmax's tie rule: the
// lowest index wins; a NaN logit is taken as the maximum, as numpy does), then the (gt, pred)
// cell of a per-block LDS histogram; each block adds its non-zero cells to the int64 matrix
// with integer atomics.  Counts are order-independent, so the result is exact and deterministic.
#include "msl_internal.h"

// No FMA contraction in this file: k_image_metrics' fp64 scores are compared with numpy's, where every
// operation is rounded on its own (k_confusion has no floating-point arithmetic).
#pragma clang fp contract(off)

namespace msl {

constexpr int kEvalMaxClasses = 64;  // LDS histogram of C*C ints

__global__ void __launch_bounds__(256) k_confusion(const float* __restrict__ pred,
                                                   const long long* __restrict__ label, int C, long long P,
                                                   unsigned long long* __restrict__ cm,
                                                   int* __restrict__ argmax_out) {
  __shared__ unsigned int h[kEvalMaxClasses * kEvalMaxClasses];
  for (int i = threadIdx.x; i < C * C; i += 256) h[i] = 0u;
  __syncthreads();
  for (long long p = blockIdx.x * 256LL + threadIdx.x; p < P; p += (long long)gridDim.x * 256) {
    int best = 0;
    float bv = pred[p];
    if (!(bv != bv)) {  // a NaN at class 0 is the answer already
      for (int c = 1; c < C; ++c) {
        const float v = pred[(long long)c * P + p];
        if (v != v) { best = c; break; }
        if (v > bv) { bv = v; best = c; }
      }
    }
    if (argmax_out) argmax_out[p] = best;
    const long long g = label[p];
    if (g >= 0 && g < C) atomicAdd(&h[(int)g * C + best], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * C; i += 256)
    if (h[i]) atomicAdd(&cm[i], (unsigned long long)h[i]);
}

// ---------------------------------------------------------------- one image's scores, on the device
// Per-image analysis (the reference's tools/analysis.py: Eval.add_batch, val_info, Eval.reset per image):
// the four scores of utils/eval.py:Eval from the matrix the image's prediction launch just filled, the
// save / don't-save decision against the threshold, and the hand-over to the whole-set matrix - one block,
// nothing crosses to the host.  The row, column and diagonal sums are exact uint64 sums converted to fp64
// once; every fp64 operation after that is rounded on its own (no contraction, IEEE divides), so a
// per-class ratio is numpy's bit for bit; the nan-means and FWIoU are summed by one thread in class order.
constexpr int kMetricsMaxC = 32;
constexpr int kMetricsHead = 9;  // PA, MPA, MIoU, FWIoU, MPA_13, MIoU_13, FWIoU_13, pixels, selected
__constant__ int k16to13[13] = {0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};  // synthia_set_16_to_13

__global__ void __launch_bounds__(256) k_image_metrics(unsigned long long* __restrict__ image_cm,
                                                       unsigned long long* __restrict__ total_cm, int C,
                                                       double threshold, double* __restrict__ rows, int capacity,
                                                       int* __restrict__ state) {
  __shared__ unsigned long long s_r[kMetricsMaxC], s_d[kMetricsMaxC];
  __shared__ double s_w[kMetricsMaxC], s_acc[kMetricsMaxC], s_iou[kMetricsMaxC];
  const int t = threadIdx.x;
  if (t < C) {
    unsigned long long r = 0ull, c = 0ull;
    for (int j = 0; j < C; ++j) {
      r += image_cm[t * C + j];
      c += image_cm[j * C + t];
    }
    const unsigned long long d = image_cm[t * C + t];
    const double rd = (double)r, cd = (double)c, dd = (double)d;
    s_r[t] = r;
    s_d[t] = d;
    s_w[t] = rd;
    s_acc[t] = dd / rd;              // 0/0 = NaN: an absent class
    s_iou[t] = dd / (rd + cd - dd);  // numpy's order
  }
  __syncthreads();  // every cell of image_cm has been read
  if (t == 0) {
    const int cursor = state[0];
    const int slot = (int)((unsigned int)cursor % (unsigned int)capacity);  // in [0, capacity) whatever state held
    double* row = rows + (long long)slot * (kMetricsHead + C);
    unsigned long long total = 0ull, trace = 0ull;
    for (int k = 0; k < C; ++k) {
      total += s_r[k];
      trace += s_d[k];
    }
    const double tot = (double)total;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double sa = 0.0, si = 0.0, sf = 0.0;
    int na = 0, ni = 0;
    for (int k = 0; k < C; ++k) {
      const double a = s_acc[k], u = s_iou[k];
      if (a == a) { sa += a; ++na; }
      if (u == u) { si += u; ++ni; sf += s_w[k] * u; }
      row[kMetricsHead + k] = u;
    }
    const double mpa = na ? sa / (double)na : nan, miou = ni ? si / (double)ni : nan;
    double mpa13 = nan, miou13 = nan, fw13 = nan;
    if (C == 16) {
      double sa3 = 0.0, si3 = 0.0, sf3 = 0.0;
      int na3 = 0, ni3 = 0;
      for (int j = 0; j < 13; ++j) {
        const int k = k16to13[j];
        const double a = s_acc[k], u = s_iou[k];
        if (a == a) { sa3 += a; ++na3; }
        if (u == u) { si3 += u; ++ni3; sf3 += s_w[k] * u; }
      }
      mpa13 = na3 ? sa3 / (double)na3 : nan;
      miou13 = ni3 ? si3 / (double)ni3 : nan;
      fw13 = sf3 / tot;
    }
    const double m = C == 16 ? miou13 : miou;  // val_info's MIoU
    const int selected = m < threshold ? 1 : 0;  // strict; a NaN is not selected
    row[0] = total ? (double)trace / tot : 0.0;
    row[1] = mpa;
    row[2] = miou;
    row[3] = sf / tot;
    row[4] = mpa13;
    row[5] = miou13;
    row[6] = fw13;
    row[7] = tot;
    row[8] = (double)selected;
    state[0] = cursor + 1;
    state[1] = selected;
    state[2] = slot;
  }
  for (int i = t; i < C * C; i += 256) {
    total_cm[i] += image_cm[i];
    image_cm[i] = 0ull;
  }
}

}  // namespace msl

using namespace msl;

extern "C" {

int msl_image_metrics(unsigned long long* image_cm, unsigned long long* total_cm, int c, double threshold,
                      double* rows, int capacity, int* state, msl_stream_t stream) {
  if (!image_cm || !total_cm || !rows || !state || c < 1 || c > kMetricsMaxC || capacity < 1) return MSL_ERR_ARG;
  MSL_LAUNCH(k_image_metrics, dim3(1), dim3(256), 0, as_stream(stream), image_cm, total_cm, c, threshold, rows,
             capacity, state);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

int msl_confusion_accumulate(const float* pred, const long long* label, int c, long long p,
                             unsigned long long* confusion, int* argmax_out, msl_stream_t stream) {
  if (!pred || !label || !confusion || c < 1 || c > kEvalMaxClasses || p < 1) return MSL_ERR_ARG;
  const int blocks = (int)std::min<long long>((p + 255) / 256, 2048);
  MSL_LAUNCH(k_confusion, dim3(blocks), dim3(256), 0, as_stream(stream), pred, label, c, p,
                     confusion, argmax_out);
  MSL_CHECK_LAUNCH();
  return MSL_OK;
}

}  // extern "C"
