// Persistent CartPole rollout kernel: the whole epoch's steps x (policy
// forward -> categorical action sample -> CartPole transition with
// per-instance termination, truncation and autoreset) in ONE launch.
//
// No instance reads another's state, so a workgroup owns 16 instances for
// the whole epoch.  The net's weight image, the biases and the fp32
// observation tile stay in LDS; the fp64 env state and the elapsed counter
// of row r live in the registers of thread r; the logits never leave the
// chip.  The only synchronisation is the workgroup barrier.
//
// Results are byte-identical to the multi-kernel body (mlp_forward ->
// categorical_sample -> cartpole_env_step): the net stage and the per-row
// arithmetic are the shared code of rollout_steps.h and every Philox draw
// uses the same (seed, offset, row).  LDS: the observation tile + 2
// activation tiles and the net (net_lds_floats, common.h).
#include "common.h"
#include "philox.h"
#include "rollout_steps.h"

template <int NT>
__global__ __launch_bounds__(NT) void cartpole_rollout_fused_f32(CartPoleRolloutArgs a) {
  constexpr int LDSW = ROLLOUT_LDSW;
  constexpr int ROWS = ROLLOUT_ROWS;
  extern __shared__ float smem[];
  float* const st = smem;
  float* const buf0 = st + ROWS * LDSW;
  float* const buf1 = buf0 + ROWS * LDSW;
  float* const wl = buf1 + ROWS * LDSW;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int row0 = blockIdx.x * ROWS;
  const int N = a.N, steps = a.steps;
  const int n_act = a.dims[a.n_layers];
  const uint64_t ctr = *a.ctr;  // read once; the bump is a later graph node

  // ---- prologue: weights, biases -> LDS ---------------------------------
  const NetStage net = net_stage<NT, false>(a, wl, tid);
  for (int idx = tid; idx < ROWS * LDSW; idx += NT) st[idx] = 0.f;
  __syncthreads();

  // thread r < 16 owns instance row0 + r: fp64 state and elapsed in
  // registers from the env's carry tensors or the epoch-reset draw
  const int row = row0 + tid;
  const bool owner = tid < ROWS && row < N;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int el = 0;
  if (owner) {
    if (a.start_with_reset) {
      cartpole_reset_draw(a.env_seed, (uint64_t)steps + ctr, (uint32_t)row, s);
    } else {
      #pragma unroll
      for (int k = 0; k < 4; ++k) s[k] = a.state[(long)row * 4 + k];
      el = a.elapsed[row];
    }
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v = (float)s[k];
      a.obs_full[(long)row * 4 + k] = v;
      st[tid * LDSW + k] = v;
    }
  }
  __syncthreads();

  for (int t = 0; t < steps; ++t) {
    // ---- policy forward on the LDS-resident observation tile -----------
    const float* const logits =
        net_forward<NT, LDSW, false>(a, st, buf0, buf1, wl, net.bl, wave, lane);

    // ---- sample + env transition: thread r on its own row --------------
    if (owner) {
      const uint64_t off = (uint64_t)t + ctr;
      const int action = categorical_sample_row(logits + tid * LDSW, n_act,
                                                a.policy_seed, off, (uint32_t)row);
      float fin[4], ob[4];
      const bool d = cartpole_env_row(s, &el, action, a.max_steps, a.env_seed, off,
                                      (uint32_t)row, fin, ob);
      const long tr = (long)t * N + row;
      #pragma unroll
      for (int k = 0; k < 4; ++k) {
        a.obs_full[((long)(t + 1) * N + row) * 4 + k] = ob[k];
        a.final_obs[tr * 4 + k] = fin[k];
        st[tid * LDSW + k] = ob[k];
      }
      a.act_buf[tr] = action;
      a.rew_buf[tr] = 1.f;
      a.done_buf[tr] = d ? 1 : 0;
    }
    __syncthreads();
  }

  // ---- epilogue: live state back to the env's carry tensors -------------
  if (owner) {
    #pragma unroll
    for (int k = 0; k < 4; ++k) a.state[(long)row * 4 + k] = s[k];
    a.elapsed[row] = el;
  }
}

// 4 waves per workgroup: one 16-column output tile each at width 64
void launch_cartpole_rollout_fused(const CartPoleRolloutArgs& a, hipStream_t stream) {
  const dim3 g((a.N + ROLLOUT_ROWS - 1) / ROLLOUT_ROWS);
  const size_t lds = net_lds_floats(3, a.dims, a.n_layers) * sizeof(float);
  hipLaunchKernelGGL((cartpole_rollout_fused_f32<256>), g, dim3(256), lds, stream, a);
}
