// One-launch Adam step over every parameter of the model (HBM-bound: read p, g, m, v; write p,
// m, v), reproducing torch.optim.Adam's single-tensor loop (amsgrad=False, maximize=False, L2
// weight decay) as the reference drives it (train_source.py:145-146):
//
//   for each entry of optim_parameters()  (deeplab_multi.py:132-171), duplicates included (Q2)
//       step += 1
//       d  = g + wd * p                         (grad.add(param, alpha=wd) -> fma)
//       m  = m + (1-b1) * (d - m)               (exp_avg.lerp_(d, 1-b1))
//       v  = v * b2 + ((1-b2) * d) * d          (exp_avg_sq.mul_(b2).addcmul_(d, d, value=1-b2))
//       p  = p + (-(lr / (1-b1^step)) * m) / (sqrt(v) / sqrt(1-b2^step) + eps)
//
// The k entries of a parameter listed k times share m, v and step and run one after the other on
// one element, so one thread applies the k updates in registers, as k_sgd does.
//
// The step counter lives in device memory (an fp32 scalar per entry, as torch stores
// state['step']), so a replayed hipGraph advances it without the host.  It is read and advanced by
// k_adam_coef alone - one thread per entry, launched before the element kernel on the same stream
// - which also evaluates, in fp64 as torch does on the host, the two scalars each of the entry's
// updates needs and rounds them to fp32 into a small table.  k_adam reads that table and never the
// counter: no block of the element kernel can see a counter another block has advanced, and pow
// stays out of the element loop.
#include "msl_internal.h"

namespace msl {

constexpr int kAdamBlockElems = 4096;  // the block plan is msl_sgd_plan's (msl_sgd_block_elems)
constexpr int kAdamMaxMult = 4;        // rows of an entry's coefficient table

__global__ void __launch_bounds__(64) k_adam_coef(const msl_adam_entry* __restrict__ entries, int n_entries,
                                                   float lr0, float lr1, const float* __restrict__ lr_dev,
                                                   double b1, double b2, float* __restrict__ coef) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_entries) return;
  const msl_adam_entry e = entries[i];
  const int mult = e.mult < kAdamMaxMult ? e.mult : kAdamMaxMult;
  const double lr = lr_dev ? lr_dev[e.group ? 1 : 0] : (e.group ? lr1 : lr0);
  const float step = *e.step;
  float* c = coef + (size_t)i * kAdamMaxMult * 2;
  for (int r = 0; r < kAdamMaxMult; ++r) {
    float step_size = 0.f, bc2_sqrt = 1.f;
    if (r < mult) {
      const double t = (double)step + (r + 1);
      step_size = (float)(lr / (1.0 - pow(b1, t)));
      bc2_sqrt = (float)sqrt(1.0 - pow(b2, t));
    }
    c[2 * r] = step_size;
    c[2 * r + 1] = bc2_sqrt;
  }
  *e.step = step + (float)(mult > 0 ? mult : 0);
}

// one Adam update of one element, every product and sum rounded on its own as torch-CPU's tensor
// ops round them (lerp_, mul_, addcmul_, sqrt, div, add_, addcdiv_): hipcc's -ffp-contract=fast
// would fuse them into fmas, under contract(off) it does not.  sqrt and / are correctly rounded.
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float d, float om_b1, float b2,
                                            float om_b2, float eps, float neg_step_size, float bc2_sqrt) {
#pragma clang fp contract(off)
  m = m + om_b1 * (d - m);
  v = v * b2 + (om_b2 * d) * d;
  const float denom = __fdiv_rn(__fsqrt_rn(v), bc2_sqrt) + eps;
  p = p + __fdiv_rn(neg_step_size * m, denom);
}

__global__ void __launch_bounds__(256) k_adam(const msl_adam_entry* __restrict__ entries,
                                               const int32_t* __restrict__ block_entry,
                                               const long long* __restrict__ block_offset,
                                               const float* __restrict__ coef, float om_b1, float b2,
                                               float om_b2, float eps, float wd, float gscale) {
  const int ei = block_entry[blockIdx.x];
  const msl_adam_entry e = entries[ei];
  const long long base = block_offset[blockIdx.x];
  const long long end = base + kAdamBlockElems < e.numel ? base + kAdamBlockElems : e.numel;
  const int mult = e.mult < kAdamMaxMult ? e.mult : kAdamMaxMult;
  // the entry's coefficients (uniform over the block): -lr/(1-b1^t), sqrt(1-b2^t) for its mult updates
  float nss[kAdamMaxMult], bcs[kAdamMaxMult];
#pragma unroll
  for (int r = 0; r < kAdamMaxMult; ++r) {
    nss[r] = -coef[((size_t)ei * kAdamMaxMult + r) * 2];
    bcs[r] = coef[((size_t)ei * kAdamMaxMult + r) * 2 + 1];
  }
  for (long long i = base + threadIdx.x; i < end; i += 256) {
    float p = e.param[i];
    const float g = gscale == 1.f ? e.grad[i] : e.grad[i] * gscale;
    float m = e.exp_avg[i];
    float v = e.exp_avg_sq[i];
#pragma unroll
    for (int r = 0; r < kAdamMaxMult; ++r) {
      if (r < mult) {
        const float d = wd != 0.f ? __fmaf_rn(p, wd, g) : g;
        adam_update(p, m, v, d, om_b1, b2, om_b2, eps, nss[r], bcs[r]);
      }
    }
    e.param[i] = p;
    e.exp_avg[i] = m;
    e.exp_avg_sq[i] = v;
  }
}

static int adam_launch(const msl_adam_entry* entries, int n_entries, const int32_t* block_entry,
                       const long long* block_offset, long long n_blocks, float lr0, float lr1,
                       const float* lr_dev, double beta1, double beta2, double eps, float weight_decay,
                       float grad_scale, float* coef, msl_stream_t stream) {
  if (n_entries > 0) {
    MSL_LAUNCH(k_adam_coef, dim3((unsigned)cdiv(n_entries, 64)), dim3(64), 0, as_stream(stream), entries,
               n_entries, lr0, lr1, lr_dev, beta1, beta2, coef);
    MSL_CHECK_LAUNCH();
  }
  if (n_blocks > 0) {
    // 1-b1, b2, 1-b2 and eps are formed in double and rounded to fp32 once, as torch rounds the
    // Python doubles it hands to the fp32 tensor ops
    MSL_LAUNCH(k_adam, dim3((unsigned)n_blocks), dim3(256), 0, as_stream(stream), entries, block_entry,
               block_offset, (const float*)coef, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
               (float)eps, weight_decay, grad_scale);
    MSL_CHECK_LAUNCH();
  }
  return MSL_OK;
}

static bool adam_args_ok(const msl_adam_entry* entries, int n_entries, const int32_t* block_entry,
                         const long long* block_offset, long long n_blocks, double beta1, double beta2,
                         double eps, const float* coef) {
  return entries && block_entry && block_offset && coef && n_entries >= 0 && n_blocks >= 0 &&
         n_blocks <= 0x7fffffff && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0;
}

}  // namespace msl

using namespace msl;

extern "C" {

int msl_adam_max_mult(void) { return kAdamMaxMult; }

size_t msl_adam_coef_bytes(int n_entries) {
  return n_entries > 0 ? (size_t)n_entries * kAdamMaxMult * 2 * sizeof(float) : 0;
}

int msl_adam_step(const msl_adam_entry* entries, int n_entries, const int32_t* block_entry,
                  const long long* block_offset, long long n_blocks, float lr0, float lr1, double beta1,
                  double beta2, double eps, float weight_decay, float grad_scale, float* coef,
                  msl_stream_t stream) {
  if (!adam_args_ok(entries, n_entries, block_entry, block_offset, n_blocks, beta1, beta2, eps, coef))
    return MSL_ERR_ARG;
  return adam_launch(entries, n_entries, block_entry, block_offset, n_blocks, lr0, lr1, nullptr, beta1,
                     beta2, eps, weight_decay, grad_scale, coef, stream);
}

int msl_adam_step_lr_dev(const msl_adam_entry* entries, int n_entries, const int32_t* block_entry,
                         const long long* block_offset, long long n_blocks, const float* lr_dev,
                         double beta1, double beta2, double eps, float weight_decay, float grad_scale,
                         float* coef, msl_stream_t stream) {
  if (!lr_dev ||
      !adam_args_ok(entries, n_entries, block_entry, block_offset, n_blocks, beta1, beta2, eps, coef))
    return MSL_ERR_ARG;
  return adam_launch(entries, n_entries, block_entry, block_offset, n_blocks, 0.f, 0.f, lr_dev, beta1,
                     beta2, eps, weight_decay, grad_scale, coef, stream);
}

}  // extern "C"
