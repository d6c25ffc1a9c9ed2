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
// gaussian_sample -> pendulum_env_step): the per-row arithmetic is the
// shared code of rollout_steps.h and every Philox draw uses the same
// (seed, offset, row).
#include "common.h"
#include "philox.h"
#include "rollout_steps.h"

// LDS image (floats): the observation tile + 2 activation tiles, the padded
// whole-net weight image ([out][in + 1] per layer), biases.
__host__ __device__ inline int pendulum_rollout_lds_floats(const int* dims,
                                                           int n_layers) {
  int n = 3 * ROLLOUT_ROWS * ROLLOUT_LDSW;
  for (int l = 0; l < n_layers; ++l) n += dims[l + 1] * (dims[l] + 1) + dims[l + 1];
  return n;
}

template <int NT>
__global__ __launch_bounds__(NT) void pendulum_rollout_fused_f32(PendulumRolloutArgs a) {
  constexpr int LDSW = ROLLOUT_LDSW;
  constexpr int ROWS = ROLLOUT_ROWS;
  constexpr int NW = NT / 64;
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
  int woff = 0;
  for (int l = 0; l < a.n_layers; ++l) {
    const int in_d = a.dims[l], out_d = a.dims[l + 1];
    for (int idx = tid; idx < out_d * in_d; idx += NT) {
      const int r = idx / in_d, c = idx % in_d;
      wl[woff + r * (in_d + 1) + c] = a.w[l][idx];
    }
    woff += out_d * (in_d + 1);
  }
  float* const bl = wl + woff;
  int boff = 0;
  for (int l = 0; l < a.n_layers; ++l) {
    for (int idx = tid; idx < a.dims[l + 1]; idx += NT) bl[boff + idx] = a.b[l][idx];
    boff += a.dims[l + 1];
  }
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

  const int i16 = lane & 15;
  const int k4 = lane >> 4;
  for (int t = 0; t < steps; ++t) {
    // ---- policy forward on the LDS-resident observation tile -----------
    const float* buf_in = st;
    int wo = 0, bo = 0;
    for (int l = 0; l < a.n_layers; ++l) {
      const int in_d = a.dims[l], out_d = a.dims[l + 1];
      float* const buf_out = (l & 1) ? buf1 : buf0;
      for (int jt = wave * 16; jt < out_d; jt += 16 * NW) {
        const int j = jt + i16;
        const bool jok = j < out_d;
        const f32x4 acc = mlp_fwd_tile_lds<LDSW, false>(buf_in, wl + wo, in_d + 1,
                                                        in_d, i16, k4, j, jok);
        mlp_fwd_tile_epilogue<LDSW>(acc, bl + bo, a.acts[l], j, jok, 0, lane, buf_out);
      }
      __syncthreads();
      buf_in = buf_out;
      wo += out_d * (in_d + 1);
      bo += out_d;
    }
    const float* const mean = buf_in;  // [ROWS][LDSW], column 0; never in HBM

    // lockstep truncation: the host's cut list says whether step t resets
    int slot = -1;
    for (int c = 0; c < a.n_cuts; ++c)
      if (a.cut_step[c] == t) slot = c;
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

size_t pendulum_rollout_fused_lds_bytes(const int* dims, int n_layers) {
  return (size_t)pendulum_rollout_lds_floats(dims, n_layers) * sizeof(float);
}

// 4 waves per workgroup: one 16-column output tile each at width 64
void launch_pendulum_rollout_fused(const PendulumRolloutArgs& a, hipStream_t stream) {
  const dim3 g((a.N + ROLLOUT_ROWS - 1) / ROLLOUT_ROWS);
  const size_t lds = pendulum_rollout_fused_lds_bytes(a.dims, a.n_layers);
  hipLaunchKernelGGL((pendulum_rollout_fused_f32<256>), g, dim3(256), lds, stream, a);
}
