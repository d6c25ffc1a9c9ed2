// Persistent PPO rollout kernel: the whole epoch's steps x (policy forward
// -> Gaussian action sample -> synthetic env transition) in ONE launch.
//
// The three-kernel rollout is a chain of 3 * steps dependent launches that
// each do a few microseconds of work (13 workgroups of forward, 1200
// sampled elements, a 17x17 GEMV per row at the bench shape).  No env
// instance ever reads another's state, so a workgroup can own 16 env rows
// for the whole epoch: the net's weight image, the env matrices and the
// live state tile stay in LDS, the policy mean never leaves the chip, and
// the only synchronisation is the workgroup barrier.  Nothing here waits
// on another workgroup.
//
// Results are byte-identical to the three-kernel path: the net stage and
// the per-row arithmetic are the shared code of rollout_steps.h (sizing:
// rollout_fused_lds_floats, common.h), the env part keeps the
// one-wave-per-row lane mapping (same reduction tree), and every Philox
// draw uses the same (seed, offset, element index).
#include "common.h"
#include "philox.h"
#include "rollout_steps.h"

template <int NT>
__global__ __launch_bounds__(NT) void ppo_rollout_fused_f32(RolloutFusedArgs a) {
  constexpr int LDSW = ROLLOUT_LDSW;
  constexpr int ROWS = ROLLOUT_ROWS;
  constexpr int NW = NT / 64;
  extern __shared__ float smem[];
  float* const st0 = smem;
  float* const st1 = st0 + ROWS * LDSW;
  float* const buf0 = st1 + ROWS * LDSW;
  float* const buf1 = buf0 + ROWS * LDSW;
  float* const actt = buf1 + ROWS * LDSW;
  float* const wl = actt + ROWS * LDSW;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int row0 = blockIdx.x * ROWS;
  const int N = a.N, O = a.O, A = a.A, steps = a.steps;
  const uint64_t ctr = *a.ctr;  // read once; the bump is a later graph node

  // ---- prologue: weights, biases, log_std, env matrices -> LDS ----------
  const NetStage net = net_stage<NT, false>(a, wl, tid);
  float* const lstd = net.end;
  float* const eA = lstd + A;
  float* const eB = eA + O * O;
  float* const ew = eB + A * O;
  for (int idx = tid; idx < A; idx += NT) lstd[idx] = a.log_std[idx];
  for (int idx = tid; idx < O * O; idx += NT) eA[idx] = a.envA[idx];
  for (int idx = tid; idx < A * O; idx += NT) eB[idx] = a.envB[idx];
  for (int idx = tid; idx < O; idx += NT) ew[idx] = a.envw[idx];

  // starting state of this workgroup's rows -> LDS and obs_full[0]:
  // lockstep reset draw (synthetic_env_reset_kernel's stream) or the carry
  // slot obs_full[steps], which this workgroup alone overwrites later
  const float* const carry = a.obs_full + (long)steps * N * O;
  for (int idx = tid; idx < ROWS * LDSW; idx += NT) {
    const int r = idx / LDSW, o = idx % LDSW;
    const int row = row0 + r;
    float v = 0.f;
    if (row < N && o < O) {
      const int i = row * O + o;
      v = a.start_with_reset
              ? 0.1f * philox_normal(a.env_seed, (uint64_t)(2 * steps) + ctr, (uint32_t)i)
              : carry[i];
      a.obs_full[i] = v;
    }
    st0[idx] = v;
    st1[idx] = 0.f;
  }
  __syncthreads();

  for (int t = 0; t < steps; ++t) {
    const float* const st = (t & 1) ? st1 : st0;
    float* const st_next = (t & 1) ? st0 : st1;

    // ---- policy forward on the LDS-resident state tile -----------------
    const float* const mean =
        net_forward<NT, LDSW, false>(a, st, buf0, buf1, wl, net.bl, wave, lane);

    // ---- action sample: a = mean + exp(log_std) * z --------------------
    float* const act_t = a.act_buf + (long)t * N * A;
    for (int idx = tid; idx < ROWS * A; idx += NT) {
      const int r = idx / A, d = idx % A;
      const int row = row0 + r;
      if (row < N) {
        const int i = row * A + d;
        const float av = gaussian_sample_elem(mean[r * LDSW + d], lstd, d,
                                              a.policy_seed, (uint64_t)t + ctr,
                                              (uint32_t)i, -1.f, -1.f);
        actt[r * LDSW + d] = av;
        act_t[i] = av;
      }
    }
    __syncthreads();

    // ---- env transition: one wave per row ------------------------------
    const int slot = cut_slot(a.cut_step, a.n_cuts, t);
    const int do_reset = slot >= 0;
    float* const obs_next = a.obs_full + (long)(t + 1) * N * O;
    for (int r = wave; r < ROWS; r += NW) {
      const int row = row0 + r;
      if (row >= N) break;  // wave-uniform; no barrier inside this loop
      float out_o, s_next, rsum;
      synthetic_env_row(st + r * LDSW, actt + r * LDSW, eA, eB, ew, row, lane, O,
                        A, a.sigma, a.env_seed, (uint64_t)(2 * t) + ctr, do_reset,
                        &out_o, &s_next, &rsum);
      if (lane < O) {
        if (do_reset) a.cut_final[((long)slot * N + row) * O + lane] = out_o;
        obs_next[(long)row * O + lane] = s_next;
        st_next[r * LDSW + lane] = s_next;
      }
      if (lane == 0) a.rew_buf[(long)t * N + row] = rsum;
    }
    __syncthreads();
  }
}

// 16 waves per workgroup: one env row per wave in the transition part
void launch_ppo_rollout_fused(const RolloutFusedArgs& a, hipStream_t stream) {
  const dim3 g((a.N + ROLLOUT_ROWS - 1) / ROLLOUT_ROWS);
  const size_t lds = rollout_fused_lds_floats(a.dims, a.n_layers, a.O, a.A) * sizeof(float);
  hipLaunchKernelGGL((ppo_rollout_fused_f32<1024>), g, dim3(1024), lds, stream, a);
}
