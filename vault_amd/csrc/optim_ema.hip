// Exponential moving average (EMA) of the weights for the fused train step (optim_clip.hip's adamw_grouped_kernel is the form
// without an average and stays as it is).
//   vault_adamw_step_ema: adamw_grouped_kernel with one more stream.  After the element's AdamW update,
//     e <- fmaf(one_minus_decay, p_new - e, e) in f32: where p_new == e the average keeps its bits.  5 loads (p, g, m, v, e),
//     up to 6 stores (p, m, v, e, the gradient's zero, the 16-bit shadow): 42 B per parameter against the grouped kernel's 34.
//   vault_ema_swap: p <-> e in place and the 16-bit shadow of the new p, 18 B per parameter.  Two calls restore every bit.
#include "common.h"
#include "../../include/vault_hip.h"

namespace {

__device__ __forceinline__ bool same_bits4(f32x4 a, f32x4 b) {
  const u32x4 x = __builtin_bit_cast(u32x4, a), y = __builtin_bit_cast(u32x4, b);
  return x[0] == y[0] && x[1] == y[1] && x[2] == y[2] && x[3] == y[3];
}

__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, h16* __restrict__ pb, float* __restrict__ ema,
                                                        long long n4, const uint8_t* __restrict__ gmap,
                                                        const float* __restrict__ table, int n_groups, float lr_factor,
                                                        float bias_corr, float b1, float b2, float eps, float gscale,
                                                        const float* __restrict__ coef, float omd, int zero_grad,
                                                        const uint8_t* __restrict__ zmask) {
  H16_SATURATE();
  // (step size, lr x weight decay) per group, as adamw_grouped_kernel builds it
  __shared__ float2 tab[256];
  {
    const int t = threadIdx.x;
    float2 e = {__builtin_nanf(""), __builtin_nanf("")};
    if (t < n_groups) {
      const float lr = lr_factor * table[2 * t];
      e = {lr * bias_corr, lr * table[2 * t + 1]};
    }
    tab[t] = e;
  }
  const float gs = coef ? gscale * coef[0] : gscale;
  __syncthreads();
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256ll) {
    const float2 sw = tab[gmap[i >> 4]];
    const float step_size = sw.x, lr_wd = sw.y;
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    f32x4 gv = reinterpret_cast<f32x4*>(g)[i];
    f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
    f32x4 ev = reinterpret_cast<f32x4*>(ema)[i];
    // idle elements (g = m = v = 0 in a group without weight decay) keep p, m, v, the shadow and the gradient as the sibling
    // kernels do; the average still moves towards p unless it already holds p's bits (then fmaf(d, 0, e) = e: nothing to store)
    if (lr_wd == 0.f) {
      bool idle = true;
#pragma unroll
      for (int e = 0; e < 4; ++e) idle = idle && gv[e] == 0.f && mv[e] == 0.f && vv[e] == 0.f;
      if (idle) {
        if (same_bits4(pv, ev)) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) ev[e] = __builtin_fmaf(omd, pv[e] - ev[e], ev[e]);
        reinterpret_cast<f32x4*>(ema)[i] = ev;
        continue;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ge = gv[e] * gs;
      mv[e] = mv[e] * b1 + (1.f - b1) * ge;
      vv[e] = vv[e] * b2 + (1.f - b2) * ge * ge;
      pv[e] = pv[e] - step_size * (mv[e] / (sqrtf(vv[e]) + eps));
      if (lr_wd != 0.f) pv[e] = pv[e] - lr_wd * pv[e];
      ev[e] = __builtin_fmaf(omd, pv[e] - ev[e], ev[e]);
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    reinterpret_cast<f32x4*>(ema)[i] = ev;
    if (zero_grad && (zmask == nullptr || zmask[i >> 4])) reinterpret_cast<f32x4*>(g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (pb) {
      uint2 w = {pack_h16x2(pv[0], pv[1]), pack_h16x2(pv[2], pv[3])};
      reinterpret_cast<uint2*>(pb)[i] = w;
    }
  }
}

__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ ema, h16* __restrict__ pb,
                                                       long long n4) {
  H16_SATURATE();
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256ll) {
    const f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 ev = reinterpret_cast<f32x4*>(ema)[i];
    reinterpret_cast<f32x4*>(p)[i] = ev;
    reinterpret_cast<f32x4*>(ema)[i] = pv;
    if (pb) {
      uint2 w = {pack_h16x2(ev[0], ev[1]), pack_h16x2(ev[2], ev[3])};
      reinterpret_cast<uint2*>(pb)[i] = w;
    }
  }
}

}  // namespace

extern "C" int vault_adamw_step_ema(float* p, float* g, float* m, float* v, void* p_bf16, float* ema, long long n,
                                    const unsigned char* group_map, const float* group_table, int n_groups,
                                    float lr_factor, float beta1, float beta2, float eps, float bias_corr_factor,
                                    float grad_scale, const float* coef, float one_minus_decay, int zero_grad,
                                    const unsigned char* zero_mask, void* stream) {
  if (!p || !g || !m || !v || !ema || !group_map || !group_table || n <= 0 || (n & 3) || (zero_mask && (n & 63)) ||
      n_groups < 1 || n_groups > 256 || !(one_minus_decay > 0.f && one_minus_decay <= 1.f))
    return VAULT_EINVAL;
  const long long n4 = n / 4;
  const int blocks = (int)((n4 + 255) / 256 > 8192 ? 8192 : (n4 + 255) / 256);
  hipLaunchKernelGGL(adamw_ema_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p, g, m, v,
                     reinterpret_cast<h16*>(p_bf16), ema, n4, group_map, group_table, n_groups, lr_factor, bias_corr_factor,
                     beta1, beta2, eps, grad_scale, coef, one_minus_decay, zero_grad, zero_mask);
  return (int)hipGetLastError();
}

extern "C" int vault_ema_swap(float* p, float* ema, void* p_bf16, long long n, void* stream) {
  if (!p || !ema || p == ema || n <= 0 || (n & 3)) return VAULT_EINVAL;
  const long long n4 = n / 4;
  const int blocks = (int)((n4 + 255) / 256 > 8192 ? 8192 : (n4 + 255) / 256);
  hipLaunchKernelGGL(ema_swap_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p, ema,
                     reinterpret_cast<h16*>(p_bf16), n4);
  return (int)hipGetLastError();
}
