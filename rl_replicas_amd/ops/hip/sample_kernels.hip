// Action-sampling kernels for the rollout hot loop.
//
// The reference samples actions through torch.distributions on the
// host path (stochastic_policy.py:26-41): exp(log_std) + randn + mul +
// add (+ clamp) is 4-5 kernels per sampler step.  Here the sample is
// ONE kernel: counter-based Philox4x32-10 RNG (stateless, seeded from
// the run seed + a per-call offset -> bitwise reproducible, replay-safe
// under hipGraph capture) with Box-Muller for normals.
#include "common.h"
#include "philox.h"
#include "rollout_steps.h"

// actions = mean + exp(log_std) * z, with optional clip to [-limit, limit]
// (limit < 0 disables clipping; noise_scale overrides sigma when >= 0,
// which implements the _NoisedPolicy deterministic-actor case)
__global__ __launch_bounds__(256) void gaussian_sample_kernel(
    const float* __restrict__ mean, const float* __restrict__ log_std,
    float* __restrict__ out, int B, int D, uint64_t seed, uint64_t offset,
    float noise_scale, float limit,
    const unsigned long long* __restrict__ offset_ptr) {
  // offset_ptr: optional device counter added to `offset` -- lets a
  // hipGraph replay draw fresh randomness (the by-value offset is
  // frozen at capture; the counter advances via counter_add_kernel)
  if (offset_ptr) offset += *offset_ptr;
  const int total = B * D;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    out[i] = gaussian_sample_elem(mean[i], log_std, i % D, seed, offset,
                                  (uint32_t)i, noise_scale, limit);
  }
}

// categorical sample: inverse-CDF over softmax(logits) per row
// (offset_ptr: optional device counter, as in gaussian_sample_kernel)
__global__ __launch_bounds__(256) void categorical_sample_kernel(
    const float* __restrict__ logits, int64_t* __restrict__ out, int B, int N,
    uint64_t seed, uint64_t offset,
    const unsigned long long* __restrict__ offset_ptr) {
  if (offset_ptr) offset += *offset_ptr;
  for (int row = blockIdx.x * 256 + threadIdx.x; row < B; row += gridDim.x * 256)
    out[row] = categorical_sample_row(logits + (long)row * N, N, seed, offset,
                                      (uint32_t)row);
}

// uniform actions in [low, high] (RandomPolicy over a Box with one bound
// pair): element i = row * A + d is keyed by (seed, offset, i)
// (offset_ptr: optional device counter, as in gaussian_sample_kernel)
__global__ __launch_bounds__(256) void uniform_sample_kernel(
    float* __restrict__ out, int total, float low, float high, uint64_t seed,
    uint64_t offset, const unsigned long long* __restrict__ offset_ptr) {
  if (offset_ptr) offset += *offset_ptr;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256)
    out[i] = uniform_sample_elem(low, high, seed, offset, (uint32_t)i);
}
