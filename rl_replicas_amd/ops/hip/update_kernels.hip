// Multi-tensor parameter-update kernels: fused Adam and fused Polyak.
//
// The reference updates parameters through torch.optim.Adam and a
// per-parameter Python Polyak loop (utils.py:47-57); at this model
// scale those cost one-plus kernel launch per tensor.  Here the whole
// update is ONE launch (plus a one-block step-counter bump for Adam):
// the tensor table travels by value in the kernarg segment, and the
// grid is 2-D — tensors x element chunks — so the 65K-element tensors
// of the off-policy nets update across many CUs instead of one
// workgroup (one-block-per-tensor measured 114 us; chunked ~10 us).
//
// The step counters are read (s+1) by every block and bumped by a
// separate single-block kernel AFTER the update — concurrent blocks
// must all see the same pre-update count.
#include "common.h"

#define MT_CHUNK 8192  // elements per (tensor, chunk) block

__global__ __launch_bounds__(256) void fused_adam_kernel(AdamArgs a) {
  // device-side gate: a captured loop can disable later updates without
  // host control flow (PPO's KL early stop runs entirely on device)
  if (a.gate && *a.gate == 0.f) return;
  const int t = blockIdx.x;
  if (t >= a.n_tensors) return;
  const int n = a.numel[t];
  const int c0 = blockIdx.y * MT_CHUNK;
  if (c0 >= n) return;
  const int c1 = min(c0 + MT_CHUNK, n);
  const float s = a.step[t][0] + 1.f + a.step_delta;
  const float bc1 = 1.f - __powf(a.beta1, s);
  const float bc2 = 1.f - __powf(a.beta2, s);

  float* p = a.p[t];
  float* g = a.g[t];
  float* m = a.m[t];
  float* v = a.v[t];
  for (int i = c0 + threadIdx.x; i < c1; i += 256) {
    float grad = g[i];
    if (a.weight_decay != 0.f) grad += a.weight_decay * p[i];
    float mi = a.beta1 * m[i] + (1.f - a.beta1) * grad;
    float vi = a.beta2 * v[i] + (1.f - a.beta2) * grad * grad;
    m[i] = mi;
    v[i] = vi;
    const float mhat = mi / bc1;
    const float vhat = vi / bc2;
    p[i] -= a.lr * mhat / (sqrtf(vhat) + a.eps);
  }
}

// bump every tensor's step counter once per optimizer step (launched
// after fused_adam_kernel on the same stream)
__global__ void adam_step_bump_kernel(AdamArgs a) {
  if (a.gate && *a.gate == 0.f) return;
  const int t = threadIdx.x;
  if (t < a.n_tensors) a.step[t][0] += a.step_delta;  // 1.0 for a plain step
}

// bump by a DEVICE scalar (captured gated loops: the executed-iteration
// count is only known on device)
__global__ void adam_step_bump_dev_kernel(AdamArgs a,
                                          const float* __restrict__ amount) {
  const int t = threadIdx.x;
  if (t < a.n_tensors) a.step[t][0] += *amount;
}

// One-thread bookkeeping for the captured PPO policy loop's device-side
// KL early stop: while the gate is open, record the KL and iteration
// count; close the gate when the KL crosses the threshold.  Replaces a
// ~6-torch-op chain per captured iteration.  (The mega policy iteration
// applies the same rule to its per-block pending-KL partials inside the
// reduce+Adam kernel, mlp_kernels.hip; this kernel serves the epilogue
// and the non-mega path.)
__global__ void ppo_gate_update_kernel(float* gate, const float* kl,
                                       float* kl_final, float* iters_done,
                                       float thr) {
  if (*gate != 0.f) {
    *kl_final = *kl;
    *iters_done += 1.f;
    if (*kl > thr) *gate = 0.f;
  }
}

// The tail of the captured PPO epoch in one launch, replacing
// ppo_gate_update_kernel, adam_step_bump_dev_kernel, adam_step_bump_kernel,
// value_loss_finalize_rows and the per-tensor old-policy copies.  Workgroups
// [0, ceil(rows / 4)) finalize the value-loss rows (one wave per row), the
// next one does the bookkeeping, and one workgroup per parameter tensor
// copies the policy into the old policy: a plain load and store, so every
// bit pattern (-0.0f, NaN payloads) arrives as it is.  The bookkeeping is
// the three small kernels' arithmetic in their order on one thread, the step
// bumps on thread t of the same workgroup; it then hands the host its copy
// of the executed-update count and leaves gate = 1, iters_done = 0 behind,
// which is what the next replay's first iteration expects.
__global__ __launch_bounds__(256) void ppo_epoch_epilogue(PPOEpilogueArgs a) {
  const int row_blocks = (a.rows + 3) / 4;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  if (b < row_blocks) {
    const int r = b * 4 + (tid >> 6);
    if (r >= a.rows) return;  // wave-uniform
    value_loss_row_sum(a.partials, a.losses, r, a.fb, a.row_stride, tid & 63);
    return;
  }
  if (b == row_blocks) {
    __shared__ float s_done;
    if (tid == 0) {
      if (*a.gate != 0.f) {
        *a.kl_final = *a.kl;
        *a.iters_done += 1.f;
        if (*a.kl > a.thr) *a.gate = 0.f;
      }
      s_done = *a.iters_done;
    }
    __syncthreads();
    const float done = s_done;
    if (tid < a.n_pol_steps) a.pol_step[tid][0] += done;
    if (tid < a.n_val_steps) a.val_step[tid][0] += a.val_bump;
    if (tid == 0) {
      *a.iters_out = done;
      *a.iters_done = 0.f;
      *a.gate = 1.f;
    }
    return;
  }
  const int t = b - row_blocks - 1;
  if (t >= a.n_sync) return;
  const float* s = a.src[t];
  float* d = a.dst[t];
  for (int i = tid; i < a.numel[t]; i += 256) d[i] = s[i];
}

__global__ __launch_bounds__(256) void fused_polyak_kernel(PolyakArgs a) {
  const int t = blockIdx.x;
  if (t >= a.n_tensors) return;
  const int n = a.numel[t];
  const int c0 = blockIdx.y * MT_CHUNK;
  if (c0 >= n) return;
  const int c1 = min(c0 + MT_CHUNK, n);
  const float* s = a.src[t];
  float* d = a.dst[t];
  const float rho = a.rho, one_m = 1.f - a.rho;
  for (int i = c0 + threadIdx.x; i < c1; i += 256) {
    d[i] = rho * d[i] + one_m * s[i];
  }
}
