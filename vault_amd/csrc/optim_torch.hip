// torch.optim.AdamW arithmetic for the fused train step (optim_clip.hip's adamw_grouped_kernel and optim_ema.hip's
// adamw_ema_kernel are the transformers-4.48 form and stay as they are).
//   vault_adamw_step_torch: the grouped AdamW, with or without the weight average, in the form a current HF Trainer steps
//     ("adamw_torch"): the weights decay BEFORE the update (p <- p (1 - lr wd)), the bias correction is always on, and eps is
//     added to the CORRECTED root (sqrt(v) / sqrt(1 - b2^t) + eps), not to the raw one.  Same streams as the siblings: 4 loads
//     (p, g, m, v), up to 5 stores (p, m, v, the gradient's zero, the 16-bit shadow) - 34 B per parameter, 42 with the average.
//     The betas arrive as f32, and 1 - 0.999f is 216 f32 roundoffs from 0.001 (0.999f lies 1.3e-8 above 0.999): the second
//     moment would sit 1.3e-5 from torch's, against bias corrections the caller computed in double precision.  The host takes
//     1 - beta from the shortest decimal that rounds to the f32 it was given (short_decimal) and hands the kernel both factors.
#include <math.h>

#include "common.h"
#include "../../include/vault_hip.h"

namespace {

__device__ __forceinline__ bool same_bits4(f32x4 a, f32x4 b) {
  const u32x4 x = __builtin_bit_cast(u32x4, a), y = __builtin_bit_cast(u32x4, b);
  return x[0] == y[0] && x[1] == y[1] && x[2] == y[2] && x[3] == y[3];
}

template <bool EMA>
__global__ __launch_bounds__(256) void adamw_torch_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, h16* __restrict__ pb, float* __restrict__ ema,
                                                          long long n4, const uint8_t* __restrict__ gmap,
                                                          const float* __restrict__ table, int n_groups, float lr_factor,
                                                          float inv_bc1, float inv_sqrt_bc2, float b1, float omb1, float b2,
                                                          float omb2, float eps, float gscale,
                                                          const float* __restrict__ coef, float omd,
                                                          int zero_grad, const uint8_t* __restrict__ zmask) {
  H16_SATURATE();
  // (bias-corrected step size, decay factor 1 - lr x weight decay) per group; a map byte without a group reads NaNs (loud)
  // instead of stray LDS
  __shared__ float2 tab[256];
  {
    const int t = threadIdx.x;
    float2 e = {__builtin_nanf(""), __builtin_nanf("")};
    if (t < n_groups) {
      const float lr = lr_factor * table[2 * t];
      e = {lr * inv_bc1, 1.f - lr * table[2 * t + 1]};
    }
    tab[t] = e;
  }
  const float gs = coef ? gscale * coef[0] : gscale;
  __syncthreads();
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256ll) {
    const float2 sw = tab[gmap[i >> 4]];
    const float step_size = sw.x, decay = sw.y;
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    f32x4 gv = reinterpret_cast<f32x4*>(g)[i];
    f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
    f32x4 ev = pv;
    if (EMA) ev = reinterpret_cast<f32x4*>(ema)[i];
    // idle elements (g = m = v = 0 in a group that does not decay) keep p, m, v, the shadow and the gradient as the sibling
    // kernels do; the average still moves towards p unless it already holds p's bits (then fmaf(d, 0, e) = e: nothing to store)
    if (decay == 1.f) {
      bool idle = true;
#pragma unroll
      for (int e = 0; e < 4; ++e) idle = idle && gv[e] == 0.f && mv[e] == 0.f && vv[e] == 0.f;
      if (idle) {
        if (EMA && !same_bits4(pv, ev)) {
#pragma unroll
          for (int e = 0; e < 4; ++e) ev[e] = __builtin_fmaf(omd, pv[e] - ev[e], ev[e]);
          reinterpret_cast<f32x4*>(ema)[i] = ev;
        }
        continue;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ge = gv[e] * gs;
      if (decay != 1.f) pv[e] = pv[e] * decay;
      mv[e] = mv[e] * b1 + omb1 * ge;
      vv[e] = vv[e] * b2 + omb2 * ge * ge;
      pv[e] = pv[e] - step_size * (mv[e] / (sqrtf(vv[e]) * inv_sqrt_bc2 + eps));
      if (EMA) ev[e] = __builtin_fmaf(omd, pv[e] - ev[e], ev[e]);
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    if (EMA) reinterpret_cast<f32x4*>(ema)[i] = ev;
    if (zero_grad && (zmask == nullptr || zmask[i >> 4])) reinterpret_cast<f32x4*>(g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (pb) {
      uint2 w = {pack_h16x2(pv[0], pv[1]), pack_h16x2(pv[2], pv[3])};
      reinterpret_cast<uint2*>(pb)[i] = w;
    }
  }
}

// The double a caller most likely rounded to get the f32 x: the shortest decimal (1 to 9 digits behind the point) that rounds
// to x, or x itself when none does.  0.999f -> 0.999, so that 1 - beta2 is 0.001 to double precision.
double short_decimal(float x) {
  for (double s = 10.0; s <= 1e9; s *= 10.0) {
    const double r = nearbyint((double)x * s) / s;
    if ((float)r == x) return r;
  }
  return (double)x;
}

}  // namespace

extern "C" int vault_adamw_step_torch(float* p, float* g, float* m, float* v, void* p_bf16, float* ema, long long n,
                                      const unsigned char* group_map, const float* group_table, int n_groups,
                                      float lr_factor, float beta1, float beta2, float eps, float inv_bias_corr1,
                                      float inv_sqrt_bias_corr2, float grad_scale, const float* coef, float one_minus_decay,
                                      int zero_grad, const unsigned char* zero_mask, void* stream) {
  // (the comparisons are written so that a NaN fails them)
  if (!p || !g || !m || !v || !group_map || !group_table || n <= 0 || (n & 3) || (zero_mask && (n & 63)) ||
      n_groups < 1 || n_groups > 256 || !(inv_bias_corr1 >= 1.f) || !(inv_sqrt_bias_corr2 >= 1.f) || p == ema ||
      (ema && !(one_minus_decay > 0.f && one_minus_decay <= 1.f)))
    return VAULT_EINVAL;
  const long long n4 = n / 4;
  const int blocks = (int)((n4 + 255) / 256 > 8192 ? 8192 : (n4 + 255) / 256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  h16* pb = reinterpret_cast<h16*>(p_bf16);
  const float omb1 = (float)(1.0 - short_decimal(beta1)), omb2 = (float)(1.0 - short_decimal(beta2));
  if (ema)
    hipLaunchKernelGGL(adamw_torch_kernel<true>, dim3(blocks), dim3(256), 0, s, p, g, m, v, pb, ema, n4, group_map,
                       group_table, n_groups, lr_factor, inv_bias_corr1, inv_sqrt_bias_corr2, beta1, omb1, beta2, omb2, eps,
                       grad_scale, coef, one_minus_decay, zero_grad, zero_mask);
  else
    hipLaunchKernelGGL(adamw_torch_kernel<false>, dim3(blocks), dim3(256), 0, s, p, g, m, v, pb, ema, n4, group_map,
                       group_table, n_groups, lr_factor, inv_bias_corr1, inv_sqrt_bias_corr2, beta1, omb1, beta2, omb2, eps,
                       grad_scale, coef, one_minus_decay, zero_grad, zero_mask);
  return (int)hipGetLastError();
}
