// GPU-resident synthetic-environment kernels (envs/device.py fast path).
//
// One rollout step of the synthetic MuJoCo-shaped envs
// (synthetic.py:72-78) is
//     s' = tanh(s A + clip(a) B + sigma * eps)
//     r  = <s', w> - 0.1 |clip(a)|^2
// which the eager torch path issues as ~10 tiny kernels.  Here it is
// ONE launch: one wavefront per env instance computes the row's GEMV
// columns, the tanh epilogue, the Philox dynamics noise, the reward
// reduction, and (on lockstep horizon boundaries) the autoreset init
// state — N x O is a few thousand elements, so this regime is pure
// launch-latency: fewer launches IS the optimization.
//
// CartPole-v1 (DeviceCartPoleEnv) has its own step/reset kernels below:
// fp64 state, one thread per instance, per-instance termination,
// truncation and autoreset.  Pendulum-v1 (DevicePendulumEnv) follows: fp64
// state, one thread per instance, lockstep truncation decided by the host.
#include "common.h"
#include "philox.h"
#include "rollout_steps.h"

// grid = N blocks of 64 threads (one wave per env row).
// s_out: next live state (post-autoreset when do_reset).
// final_out: true successor state (pre-reset; GAE bootstrap).  May
// alias s_out when do_reset == 0.
__global__ __launch_bounds__(64) void synthetic_env_step_kernel(
    const float* __restrict__ state, const float* __restrict__ actions,
    const float* __restrict__ A, const float* __restrict__ Bm,
    const float* __restrict__ w, float* __restrict__ s_out,
    float* __restrict__ final_out, float* __restrict__ reward, int N, int O,
    int Adim, float sigma, uint64_t seed, uint64_t offset, int do_reset,
    const unsigned long long* __restrict__ offset_ptr) {
  if (offset_ptr) offset += *offset_ptr;  // hipGraph-replay RNG advance
  const int row = blockIdx.x;
  if (row >= N) return;
  const float* s = state + (long)row * O;
  const float* a = actions + (long)row * Adim;
  const int o = threadIdx.x;

  // the row arithmetic is shared with the persistent rollout kernel
  float out_o, s_next, rsum;
  synthetic_env_row(s, a, A, Bm, w, row, o, O, Adim, sigma, seed, offset,
                    do_reset, &out_o, &s_next, &rsum);
  if (o < O) final_out[(long)row * O + o] = out_o;
  if (o == 0) reward[row] = rsum;
  if (o < O) s_out[(long)row * O + o] = s_next;
}

// fresh init states: s = 0.1 * eps  (SyntheticEnv._init_state)
__global__ __launch_bounds__(256) void synthetic_env_reset_kernel(
    float* __restrict__ s_out, int total, uint64_t seed, uint64_t offset,
    const unsigned long long* __restrict__ offset_ptr) {
  if (offset_ptr) offset += *offset_ptr;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256)
    s_out[i] = 0.1f * philox_normal(seed, offset, (uint32_t)i);
}

// CartPole-v1 with per-instance termination and autoreset: one thread per
// instance.  state fp64 [N,4] and elapsed int32 [N] are updated in place;
// obs is the post-autoreset observation, final_obs the true successor.
__global__ __launch_bounds__(256) void cartpole_env_step_kernel(
    double* __restrict__ state, int* __restrict__ elapsed,
    const int64_t* __restrict__ actions, float* __restrict__ obs,
    float* __restrict__ final_obs, float* __restrict__ reward,
    uint8_t* __restrict__ done, int N, int max_steps, uint64_t seed,
    uint64_t offset, const unsigned long long* __restrict__ offset_ptr) {
  if (offset_ptr) offset += *offset_ptr;
  for (int row = blockIdx.x * 256 + threadIdx.x; row < N; row += gridDim.x * 256) {
    double s[4];
    #pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = state[(long)row * 4 + k];
    int el = elapsed[row];
    float fin[4], ob[4];
    const bool d = cartpole_env_row(s, &el, (int)actions[row], max_steps, seed,
                                    offset, (uint32_t)row, fin, ob);
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
      state[(long)row * 4 + k] = s[k];
      obs[(long)row * 4 + k] = ob[k];
      final_obs[(long)row * 4 + k] = fin[k];
    }
    elapsed[row] = el;
    reward[row] = 1.f;
    done[row] = d ? 1 : 0;
  }
}

// fresh CartPole states for all N instances
__global__ __launch_bounds__(256) void cartpole_env_reset_kernel(
    double* __restrict__ state, int* __restrict__ elapsed, float* __restrict__ obs,
    int N, uint64_t seed, uint64_t offset,
    const unsigned long long* __restrict__ offset_ptr) {
  if (offset_ptr) offset += *offset_ptr;
  for (int row = blockIdx.x * 256 + threadIdx.x; row < N; row += gridDim.x * 256) {
    double s[4];
    cartpole_reset_draw(seed, offset, (uint32_t)row, s);
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
      state[(long)row * 4 + k] = s[k];
      obs[(long)row * 4 + k] = (float)s[k];
    }
    elapsed[row] = 0;
  }
}

// Pendulum-v1, lockstep (no early termination; the host knows the truncation
// step and passes do_reset): one thread per instance.  state fp64 [N,2] is
// updated in place; obs is the post-autoreset observation, final_obs the
// true successor, reward the cost of the pre-step state.
__global__ __launch_bounds__(256) void pendulum_env_step_kernel(
    double* __restrict__ state, const float* __restrict__ actions,
    float* __restrict__ obs, float* __restrict__ final_obs,
    float* __restrict__ reward, int N, int do_reset, uint64_t seed,
    uint64_t offset, const unsigned long long* __restrict__ offset_ptr) {
  if (offset_ptr) offset += *offset_ptr;
  for (int row = blockIdx.x * 256 + threadIdx.x; row < N; row += gridDim.x * 256) {
    double s[2] = {state[(long)row * 2], state[(long)row * 2 + 1]};
    float fin[3], ob[3], r;
    pendulum_env_row(s, actions[row], do_reset, seed, offset, (uint32_t)row, fin,
                     ob, &r);
    state[(long)row * 2] = s[0];
    state[(long)row * 2 + 1] = s[1];
    #pragma unroll
    for (int k = 0; k < 3; ++k) {
      obs[(long)row * 3 + k] = ob[k];
      final_obs[(long)row * 3 + k] = fin[k];
    }
    reward[row] = r;
  }
}

// fresh Pendulum states for all N instances (draw != 0), or only the
// observation of the states as they stand (draw == 0)
__global__ __launch_bounds__(256) void pendulum_env_reset_kernel(
    double* __restrict__ state, float* __restrict__ obs, int N, int draw,
    uint64_t seed, uint64_t offset,
    const unsigned long long* __restrict__ offset_ptr) {
  if (offset_ptr) offset += *offset_ptr;
  for (int row = blockIdx.x * 256 + threadIdx.x; row < N; row += gridDim.x * 256) {
    double s[2];
    if (draw) {
      pendulum_reset_draw(seed, offset, (uint32_t)row, s);
      state[(long)row * 2] = s[0];
      state[(long)row * 2 + 1] = s[1];
    } else {
      s[0] = state[(long)row * 2];
      s[1] = state[(long)row * 2 + 1];
    }
    float ob[3];
    pendulum_obs(s, ob);
    #pragma unroll
    for (int k = 0; k < 3; ++k) obs[(long)row * 3 + k] = ob[k];
  }
}

// advance a device RNG counter (graph-replayable: one bump per epoch)
__global__ void counter_add_kernel(unsigned long long* ctr,
                                   unsigned long long delta) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *ctr += delta;
}
