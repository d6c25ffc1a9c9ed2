// Persistent Pendulum rollout kernel: the whole epoch's steps x (policy
// forward -> Gaussian action sample -> Pendulum transition with lockstep
// autoreset on the host-known cut steps) in ONE launch.
//
// No instance reads another's state, so a workgroup owns 16 instances for
// the whole epoch.  The net's weight image, the biases and the fp32
// observation tile stay in LDS; the fp64 env state of row r lives in the
// registers of thread r; the mean never leaves the chip.  The only
// synchronisation is the workgroup barrier.
//
// Results are byte-identical to the multi-kernel body (mlp_forward ->
// gaussian_sample -> pendulum_env_step): the net stage and the per-row
// arithmetic are the shared code of rollout_steps.h and every Philox draw
// uses the same (seed, offset, row).  LDS: the observation tile + 2
// activation tiles and the net (net_lds_floats, common.h).
#include "common.h"
#include "philox.h"
#include "rollout_steps.h"

template <int NT>
__global__ __launch_bounds__(NT) void pendulum_rollout_fused_f32(PendulumRolloutArgs a) {
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
  const uint64_t ctr = *a.ctr;  // read once; the bump is a later graph node

  // ---- prologue: weights, biases -> LDS ---------------------------------
  const NetStage net = net_stage<NT, false>(a, wl, tid);
  for (int idx = tid; idx < ROWS * LDSW; idx += NT) st[idx] = 0.f;
  __syncthreads();

  // thread r < 16 owns instance row0 + r: fp64 state in registers from the
  // env's carry tensor or the epoch-reset draw
  const int row = row0 + tid;
  const bool owner = tid < ROWS && row < N;
  double s[2] = {0.0, 0.0};
  if (owner) {
    if (a.start_with_reset) {
      pendulum_reset_draw(a.env_seed, (uint64_t)steps + ctr, (uint32_t)row, s);
    } else {
      s[0] = a.state[(long)row * 2];
      s[1] = a.state[(long)row * 2 + 1];
    }
    float ob[3];
    pendulum_obs(s, ob);
    #pragma unroll
    for (int k = 0; k < 3; ++k) {
      a.obs_full[(long)row * 3 + k] = ob[k];
      st[tid * LDSW + k] = ob[k];
    }
  }
  __syncthreads();

  for (int t = 0; t < steps; ++t) {
    // ---- policy forward on the LDS-resident observation tile -----------
    // column 0 of the output tile
    const float* const mean =
        net_forward<NT, LDSW, false>(a, st, buf0, buf1, wl, net.bl, wave, lane);

    // lockstep truncation: the host's cut list says whether step t resets
    const int slot = cut_slot(a.cut_step, a.n_cuts, t);
    const int do_reset = slot >= 0;

    // ---- sample + env transition: thread r on its own row --------------
    if (owner) {
      const uint64_t off = (uint64_t)t + ctr;
      // A == 1: the element index of gaussian_sample_kernel is the row
      const float action = gaussian_sample_elem(mean[tid * LDSW], a.log_std, 0,
                                                a.policy_seed, off, (uint32_t)row,
                                                -1.f, -1.f);
      float fin[3], ob[3], rew;
      pendulum_env_row(s, action, do_reset, a.env_seed, off, (uint32_t)row, fin, ob,
                       &rew);
      const long tr = (long)t * N + row;
      #pragma unroll
      for (int k = 0; k < 3; ++k) {
        a.obs_full[((long)(t + 1) * N + row) * 3 + k] = ob[k];
        st[tid * LDSW + k] = ob[k];
      }
      if (do_reset) {
        #pragma unroll
        for (int k = 0; k < 3; ++k)
          a.cut_final[((long)slot * N + row) * 3 + k] = fin[k];
      }
      a.act_buf[tr] = action;
      a.rew_buf[tr] = rew;
    }
    __syncthreads();
  }

  // ---- epilogue: live state back to the env's carry tensor --------------
  if (owner) {
    a.state[(long)row * 2] = s[0];
    a.state[(long)row * 2 + 1] = s[1];
  }
}

// 4 waves per workgroup: one 16-column output tile each at width 64
void launch_pendulum_rollout_fused(const PendulumRolloutArgs& a, hipStream_t stream) {
  const dim3 g((a.N + ROLLOUT_ROWS - 1) / ROLLOUT_ROWS);
  const size_t lds = net_lds_floats(3, a.dims, a.n_layers) * sizeof(float);
  hipLaunchKernelGGL((pendulum_rollout_fused_f32<256>), g, dim3(256), lds, stream, a);
}
