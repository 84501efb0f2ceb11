// Global gradient-norm clipping and parameter groups for the fused AdamW of the train step (optim.hip's adamw_kernel is the
// one-group, unclipped form and stays as it is).
//   vault_grad_norm: sum of g^2 over the flat gradient in two launches - a fixed grid of grid-stride f32x4 loads, f64
//     accumulation per lane, one partial per block (no atomics), then one block that sums the partials in a fixed order -
//     so that a buffer gives the same bits on every run and every data-parallel rank.  It leaves the norm and the
//     clip_grad_norm_ factor in device memory for the optimizer to read: nothing goes back to the host.
//   vault_adamw_step_grouped: adamw_kernel with a (lr, weight_decay) pair per 64-element group, a schedule multiplier and
//     the clip factor read from the device.
#include <math.h>

#include "common.h"
#include "../../include/vault_hip.h"

namespace {

constexpr int NORM_BLOCKS = VAULT_GRAD_NORM_PARTIALS;    // 8 blocks of 4 waves per CU: one full-occupancy round

__device__ __forceinline__ double sq4(f32x4 a, double acc) {
#pragma unroll
  for (int e = 0; e < 4; ++e) acc = fma((double)a[e], (double)a[e], acc);
  return acc;
}

// Sum of the 256 threads' values in a fixed order: butterfly inside each wave, then the four waves in index order.
__device__ __forceinline__ double block_sum(double x, double* ws) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = x;
  __syncthreads();
  return (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

__global__ __launch_bounds__(256) void sqnorm_partials_kernel(const float* __restrict__ g, long long n4,
                                                              double* __restrict__ partials) {
  __shared__ double ws[4];
  const f32x4* G = reinterpret_cast<const f32x4*>(g);
  const long long stride = (long long)gridDim.x * 256ll;
  long long i = blockIdx.x * 256ll + threadIdx.x;
  double acc = 0.0;
  // four 16-byte loads in flight per lane, then the tail one at a time (the split depends on n and the grid only)
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const f32x4 a = G[i], b = G[i + stride], c = G[i + 2 * stride], d = G[i + 3 * stride];
    acc = sq4(d, sq4(c, sq4(b, sq4(a, acc))));
  }
  for (; i < n4; i += stride) acc = sq4(G[i], acc);
  const double s = block_sum(acc, ws);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void norm_finish_kernel(const double* __restrict__ partials, int nparts,
                                                          float* __restrict__ out, float max_norm, float unscale) {
  __shared__ double ws[4];
  double acc = 0.0;
  for (int k = threadIdx.x; k < nparts; k += 256) acc += partials[k];
  const double s = block_sum(acc, ws);
  if (threadIdx.x == 0) {
    const float norm = (float)(sqrt(s) * fabs((double)unscale));
    // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1) in f32, the division as torch's Tensor.__rdiv__
    // does it (reciprocal, then the product) - a NaN norm gives a NaN factor (the comparison is false), an infinite one 0
    const float c = (1.f / (norm + 1e-6f)) * max_norm;
    out[0] = norm;
    out[1] = c > 1.f ? 1.f : c;
  }
}

__global__ __launch_bounds__(256) void adamw_grouped_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, h16* __restrict__ pb, long long n4,
                                                            const uint8_t* __restrict__ gmap, const float* __restrict__ table,
                                                            int n_groups, float lr_factor, float bias_corr, float b1, float b2,
                                                            float eps, float gscale, const float* __restrict__ coef,
                                                            int zero_grad, const uint8_t* __restrict__ zmask) {
  H16_SATURATE();
  // (step size, lr x weight decay) per group; a map byte without a group reads NaNs (loud) instead of stray LDS
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
    // adamw_kernel's idle elements (g = m = v = 0: untouched embedding rows keep their bits), decided per group: only a
    // group without weight decay may skip them
    if (lr_wd == 0.f) {
      bool idle = true;
#pragma unroll
      for (int e = 0; e < 4; ++e) idle = idle && gv[e] == 0.f && mv[e] == 0.f && vv[e] == 0.f;
      if (idle) continue;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ge = gv[e] * gs;
      mv[e] = mv[e] * b1 + (1.f - b1) * ge;
      vv[e] = vv[e] * b2 + (1.f - b2) * ge * ge;
      pv[e] = pv[e] - step_size * (mv[e] / (sqrtf(vv[e]) + eps));
      if (lr_wd != 0.f) pv[e] = pv[e] - lr_wd * pv[e];
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    if (zero_grad && (zmask == nullptr || zmask[i >> 4])) reinterpret_cast<f32x4*>(g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (pb) {
      uint2 w = {pack_h16x2(pv[0], pv[1]), pack_h16x2(pv[2], pv[3])};
      reinterpret_cast<uint2*>(pb)[i] = w;
    }
  }
}

}  // namespace

extern "C" int vault_grad_norm(const float* g, long long n, double* partials, float* out2, float max_norm, float unscale,
                               void* stream) {
  if (!g || !partials || !out2 || n <= 0 || (n & 3) || !(max_norm > 0.f)) return VAULT_EINVAL;
  const long long n4 = n / 4;
  const int blocks = (int)((n4 + 255) / 256 > NORM_BLOCKS ? NORM_BLOCKS : (n4 + 255) / 256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sqnorm_partials_kernel, dim3(blocks), dim3(256), 0, s, g, n4, partials);
  hipLaunchKernelGGL(norm_finish_kernel, dim3(1), dim3(256), 0, s, partials, blocks, out2, max_norm, unscale);
  return (int)hipGetLastError();
}

extern "C" int vault_adamw_step_grouped(float* p, float* g, float* m, float* v, void* p_bf16, long long n,
                                        const unsigned char* group_map, const float* group_table, int n_groups,
                                        float lr_factor, float beta1, float beta2, float eps, float bias_corr_factor,
                                        float grad_scale, const float* coef, int zero_grad, const unsigned char* zero_mask,
                                        void* stream) {
  if (!p || !g || !m || !v || !group_map || !group_table || n <= 0 || (n & 3) || (zero_mask && (n & 63)) ||
      n_groups < 1 || n_groups > 256)
    return VAULT_EINVAL;
  const long long n4 = n / 4;
  const int blocks = (int)((n4 + 255) / 256 > 8192 ? 8192 : (n4 + 255) / 256);
  hipLaunchKernelGGL(adamw_grouped_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p, g, m, v,
                     reinterpret_cast<h16*>(p_bf16), n4, group_map, group_table, n_groups, lr_factor, bias_corr_factor,
                     beta1, beta2, eps, grad_scale, coef, zero_grad, zero_mask);
  return (int)hipGetLastError();
}
