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
// categorical_sample -> cartpole_env_step): the per-row arithmetic is the
// shared code of rollout_steps.h and every Philox draw uses the same
// (seed, offset, row).
#include "common.h"
#include "philox.h"
#include "rollout_steps.h"

// LDS image (floats): the observation tile + 2 activation tiles, the padded
// whole-net weight image ([out][in + 1] per layer), biases.
__host__ __device__ inline int cartpole_rollout_lds_floats(const int* dims,
                                                           int n_layers) {
  int n = 3 * ROLLOUT_ROWS * ROLLOUT_LDSW;
  for (int l = 0; l < n_layers; ++l) n += dims[l + 1] * (dims[l] + 1) + dims[l + 1];
  return n;
}

template <int NT>
__global__ __launch_bounds__(NT) void cartpole_rollout_fused_f32(CartPoleRolloutArgs a) {
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
  const int n_act = a.dims[a.n_layers];
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
    const float* const logits = buf_in;  // [ROWS][LDSW], never written to HBM

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

size_t cartpole_rollout_fused_lds_bytes(const int* dims, int n_layers) {
  return (size_t)cartpole_rollout_lds_floats(dims, n_layers) * sizeof(float);
}

// 4 waves per workgroup: one 16-column output tile each at width 64
void launch_cartpole_rollout_fused(const CartPoleRolloutArgs& a, hipStream_t stream) {
  const dim3 g((a.N + ROLLOUT_ROWS - 1) / ROLLOUT_ROWS);
  const size_t lds = cartpole_rollout_fused_lds_bytes(a.dims, a.n_layers);
  hipLaunchKernelGGL((cartpole_rollout_fused_f32<256>), g, dim3(256), lds, stream, a);
}
