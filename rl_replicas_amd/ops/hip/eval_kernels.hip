// Persistent policy evaluation: whole episodes, from the init draw to their
// end, in ONE launch, with nothing written per step.
//
//   pendulum_eval_fused_f32  horizon x (forward -> action -> Pendulum step);
//                            the action is the net's output (deterministic
//                            actor) or a Gaussian sample around it
//   cartpole_eval_fused_f32  up to horizon x (forward -> categorical sample
//                            -> CartPole step) with per-row termination; a
//                            finished row is frozen, and the step loop ends
//                            when no row of the workgroup is live
//   episode_reduce_kernel    the reduction that closes the multi-kernel body:
//                            first-episode return and length of each row of
//                            a [steps, N] reward / done buffer
//
// A workgroup owns 16 episodes for their whole life, as in the persistent
// rollout and collect kernels: the fp64 env state of row r, its return
// (double) and its length live in the registers of thread r, the fp32
// observation tile in LDS.  The only synchronisation is the workgroup
// barrier; there are no atomics.  Per row the kernels write the return, the
// length and the init state.
//
// Weight regimes are those of pendulum_collect_kernels.hip: narrow (every
// width <= MLP_NARROW_WIDTH) keeps the padded whole-net weight image in LDS,
// wide (Pendulum only, up to MLP_MAX_WIDTH) reads weights from global memory.
// LDS: the observation tile + 2 activation tiles and the net (net_lds_floats,
// common.h).
//
// Results are byte-identical to the multi-kernel body (env reset, then
// mlp_forward -> [gaussian_sample | categorical_sample] -> env step per
// step, then episode_reduce): the net stage and the per-row arithmetic are
// the shared code of rollout_steps.h and every Philox draw uses the same
// (seed, offset, row).
#include "common.h"
#include "philox.h"
#include "rollout_steps.h"

template <int NT, bool WIDE>
__global__ __launch_bounds__(NT) void pendulum_eval_fused_f32(PendulumEvalArgs a) {
  constexpr int LDSW = WIDE ? ROLLOUT_WIDE_LDSW : ROLLOUT_LDSW;
  constexpr int ROWS = ROLLOUT_ROWS;
  extern __shared__ float smem[];
  float* const st = smem;
  float* const buf0 = st + ROWS * LDSW;
  float* const buf1 = buf0 + ROWS * LDSW;
  float* const wl = buf1 + ROWS * LDSW;  // narrow only

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int N = a.N, horizon = a.horizon;
  // read once; the bumps are later graph nodes
  const uint64_t ctr = *a.ctr;
  const uint64_t reset_ctr = *a.reset_ctr;

  const NetStage net = net_stage<NT, WIDE>(a, wl, tid);
  for (int idx = tid; idx < ROWS * LDSW; idx += NT) st[idx] = 0.f;
  __syncthreads();

  // thread r < 16 owns episode row0 + r: fp64 state in registers from the
  // init draw
  const int row = blockIdx.x * ROWS + tid;
  const bool owner = tid < ROWS && row < N;
  double s[2] = {0.0, 0.0};
  double ret = 0.0;
  if (owner) {
    pendulum_reset_draw(a.env_seed, reset_ctr, (uint32_t)row, s);
    a.init_state[(long)row * 2] = s[0];
    a.init_state[(long)row * 2 + 1] = s[1];
    float ob[3];
    pendulum_obs(s, ob);
    #pragma unroll
    for (int k = 0; k < 3; ++k) st[tid * LDSW + k] = ob[k];
  }
  __syncthreads();

  for (int t = 0; t < horizon; ++t) {
    const float* const mean =
        net_forward<NT, LDSW, WIDE>(a, st, buf0, buf1, wl, net.bl, wave, lane);

    // ---- action + env transition: thread r on its own row --------------
    if (owner) {
      float action = mean[tid * LDSW];
      if (a.mode == EVAL_GAUSSIAN)  // A == 1: the sample kernel's element is the row
        action = gaussian_sample_elem(action, a.log_std, 0, a.policy_seed,
                                      (uint64_t)t + ctr, (uint32_t)row, -1.f, -1.f);
      float rew, ob[3];
      pendulum_row_step(s, action, &rew);
      pendulum_obs(s, ob);
      ret += (double)rew;
      #pragma unroll
      for (int k = 0; k < 3; ++k) st[tid * LDSW + k] = ob[k];
    }
    __syncthreads();
  }

  if (owner) {
    a.returns[row] = ret;
    a.lengths[row] = horizon;
  }
}

template <int NT>
__global__ __launch_bounds__(NT) void cartpole_eval_fused_f32(CartPoleEvalArgs a) {
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
  const int N = a.N, horizon = a.horizon;
  const int n_act = a.dims[a.n_layers];
  // read once; the bumps are later graph nodes
  const uint64_t ctr = *a.ctr;
  const uint64_t reset_ctr = *a.reset_ctr;

  const NetStage net = net_stage<NT, false>(a, wl, tid);
  for (int idx = tid; idx < ROWS * LDSW; idx += NT) st[idx] = 0.f;
  __syncthreads();

  // thread r < 16 owns episode row0 + r: fp64 state, return and length in
  // registers
  const int row = blockIdx.x * ROWS + tid;
  const bool owner = tid < ROWS && row < N;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  double ret = 0.0;
  int len = 0;
  bool alive = owner;
  if (owner) {
    cartpole_reset_draw(a.env_seed, reset_ctr, (uint32_t)row, s);
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
      a.init_state[(long)row * 4 + k] = s[k];
      st[tid * LDSW + k] = (float)s[k];
    }
  }
  __syncthreads();

  for (int t = 0; t < horizon; ++t) {
    const float* const logits =
        net_forward<NT, LDSW, false>(a, st, buf0, buf1, wl, net.bl, wave, lane);

    // ---- sample + env transition: thread r on its own live row ---------
    // a finished row samples nothing, steps nothing and adds nothing; its
    // tile row keeps the last observation it acted on
    if (alive) {
      const int action = categorical_sample_row(logits + tid * LDSW, n_act, a.policy_seed,
                                                (uint64_t)t + ctr, (uint32_t)row);
      const bool terminated = cartpole_row_step(s, action);
      ret += (double)1.f;
      len += 1;
      alive = !terminated && len < horizon;
      if (alive) {
        #pragma unroll
        for (int k = 0; k < 4; ++k) st[tid * LDSW + k] = (float)s[k];
      }
    }
    // the step's trailing barrier and the workgroup-uniform exit test in
    // one: every thread gets the same answer, so all leave together
    if (!__syncthreads_or(alive ? 1 : 0)) break;
  }

  if (owner) {
    a.returns[row] = ret;
    a.lengths[row] = len;
  }
}

// first-episode return and length of each row: steps 0 up to and including
// the first done step, or all `steps` without a done buffer.  One thread
// per row; the same sequential fp32 -> double sum as the persistent kernels.
__global__ __launch_bounds__(256) void episode_reduce_kernel(
    const float* __restrict__ rew_buf, const unsigned char* __restrict__ done_buf,
    double* __restrict__ returns, int* __restrict__ lengths, int N, int steps) {
  for (int row = blockIdx.x * 256 + threadIdx.x; row < N; row += gridDim.x * 256) {
    double ret = 0.0;
    int len = 0;
    for (int t = 0; t < steps; ++t) {
      ret += (double)rew_buf[(long)t * N + row];
      len += 1;
      if (done_buf && done_buf[(long)t * N + row]) break;
    }
    returns[row] = ret;
    lengths[row] = len;
  }
}

// Narrow: 4 waves, one 16-column tile each at width 64.  Wide: `wide_threads`
// is 256 (each wave loops over four tiles of a 256-wide layer) or 1024 (one
// tile per wave); the caller has checked it.
void launch_pendulum_eval_fused(const PendulumEvalArgs& a, int wide_threads,
                                hipStream_t stream) {
  const dim3 g((a.N + ROLLOUT_ROWS - 1) / ROLLOUT_ROWS);
  const size_t lds = net_lds_floats(3, a.dims, a.n_layers) * sizeof(float);
  if (!net_is_wide(a.dims, a.n_layers))
    hipLaunchKernelGGL((pendulum_eval_fused_f32<256, false>), g, dim3(256), lds, stream, a);
  else if (wide_threads == 1024)
    hipLaunchKernelGGL((pendulum_eval_fused_f32<1024, true>), g, dim3(1024), lds, stream, a);
  else
    hipLaunchKernelGGL((pendulum_eval_fused_f32<256, true>), g, dim3(256), lds, stream, a);
}

// narrow only (the caller has checked every width)
void launch_cartpole_eval_fused(const CartPoleEvalArgs& a, hipStream_t stream) {
  const dim3 g((a.N + ROLLOUT_ROWS - 1) / ROLLOUT_ROWS);
  const size_t lds = net_lds_floats(3, a.dims, a.n_layers) * sizeof(float);
  hipLaunchKernelGGL((cartpole_eval_fused_f32<256>), g, dim3(256), lds, stream, a);
}
