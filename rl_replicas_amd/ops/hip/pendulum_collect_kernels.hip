// Persistent Pendulum replay collection: the whole epoch's steps x
// (behaviour action -> Pendulum transition with lockstep autoreset on the
// host-known cut steps -> replay-ring write) in ONE launch, for the two
// behaviour policies of an off-policy epoch:
//
//   COLLECT_NOISED   actor forward, then mean + noise_scale * z clipped to
//                    +-limit (utils._NoisedPolicy over a DeterministicPolicy)
//   COLLECT_UNIFORM  uniform in [low, high] (RandomPolicy); no net is read
//
// A workgroup owns 16 instances for the whole epoch, as in
// pendulum_rollout_kernels.hip: the fp64 env state of row r lives in the
// registers of thread r, the fp32 observation tile in LDS.  Every transition
// goes straight to its ring slot (write + row * steps + t) % cap, the
// instance-major order ReplayBuffer._add_flat_tensors produces, so no
// staging buffer and no second copy exist.
//
// Two weight regimes, chosen on the host by mlp_forward's own rule
// (net_is_wide, common.h; the stage itself is net_stage / net_forward of
// rollout_steps.h, LDS sized by net_lds_floats with 3 tiles):
//   narrow (every width <= MLP_NARROW_WIDTH): the padded whole-net weight
//          image in LDS, tiles from mlp_fwd_tile_lds;
//   wide   (up to MLP_MAX_WIDTH): activations ping-pong between two
//          [16][MLP_MAX_WIDTH + 4] LDS tiles, weights read from global
//          memory (L2-resident across steps), tiles from mlp_fwd_tile_wide,
//          the K loop of mlp_layer_fwd_wide_f32.
//
// Results are byte-identical to the multi-kernel body (mlp_forward ->
// gaussian_sample | uniform_sample -> pendulum_env_step, then
// replay_scatter): the net stage and the per-row arithmetic are the shared code of
// rollout_steps.h and every Philox draw uses the same (seed, offset, row).
#include "common.h"
#include "philox.h"
#include "rollout_steps.h"

template <int NT, bool WIDE>
__global__ __launch_bounds__(NT) void pendulum_collect_fused_f32(PendulumCollectArgs a) {
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
  const int row0 = blockIdx.x * ROWS;
  const int N = a.N, steps = a.steps;
  const uint64_t ctr = *a.ctr;  // read once; the bump is a later graph node
  // read once and reduced: whatever the scalar holds, slots stay in the ring
  const unsigned long long cap = a.ring.cap;
  const unsigned long long write = (unsigned long long)*a.ring.write % cap;

  // ---- prologue: (narrow) weights, biases -> LDS ------------------------
  const NetStage net = net_stage<NT, WIDE>(a, wl, tid);
  for (int idx = tid; idx < ROWS * LDSW; idx += NT) st[idx] = 0.f;
  __syncthreads();

  // thread r < 16 owns instance row0 + r: fp64 state in registers from the
  // env's carry tensor or the epoch-reset draw
  const int row = row0 + tid;
  const bool owner = tid < ROWS && row < N;
  double s[2] = {0.0, 0.0};
  float cur[3] = {0.f, 0.f, 0.f};  // the observation the next action sees
  if (owner) {
    if (a.start_with_reset) {
      pendulum_reset_draw(a.env_seed, (uint64_t)steps + ctr, (uint32_t)row, s);
    } else {
      s[0] = a.state[(long)row * 2];
      s[1] = a.state[(long)row * 2 + 1];
    }
    pendulum_obs(s, cur);
    #pragma unroll
    for (int k = 0; k < 3; ++k) st[tid * LDSW + k] = cur[k];
  }
  __syncthreads();

  float seg_acc = 0.f;  // this row's reward sum of the running segment
  for (int t = 0; t < steps; ++t) {
    // ---- actor forward on the LDS-resident observation tile ------------
    // column 0 of the output tile (unread in uniform mode: no layers)
    const float* const mean =
        net_forward<NT, LDSW, WIDE>(a, st, buf0, buf1, wl, net.bl, wave, lane);

    // lockstep truncation: the host's cut list says whether step t resets
    const int cslot = cut_slot(a.cut_step, a.n_cuts, t);
    const int do_reset = cslot >= 0;

    // ---- action + env transition + ring write: thread r on its own row --
    if (owner) {
      const uint64_t off = (uint64_t)t + ctr;
      // A == 1: the element index of the sample kernels is the row
      float action;
      if (a.mode == COLLECT_UNIFORM)
        action = uniform_sample_elem(a.low, a.high, a.action_seed, off, (uint32_t)row);
      else  // noise_scale >= 0 (host-checked): log_std is never read
        action = gaussian_sample_elem(mean[tid * LDSW], nullptr, 0, a.action_seed, off,
                                      (uint32_t)row, a.noise_scale, a.limit);
      float fin[3], ob[3], rew;
      pendulum_env_row(s, action, do_reset, a.env_seed, off, (uint32_t)row, fin, ob,
                       &rew);
      const unsigned long long slot = ring_slot(write, cap, row, steps, t);
      #pragma unroll
      for (int k = 0; k < 3; ++k) {
        a.ring.obs[slot * 3 + k] = cur[k];
        a.ring.nxt[slot * 3 + k] = fin[k];  // the true successor, pre-reset
        cur[k] = ob[k];
        st[tid * LDSW + k] = ob[k];
      }
      a.ring.act[slot] = action;
      a.ring.rew[slot] = rew;
      a.ring.dn[slot] = do_reset ? 1.f : 0.f;
      seg_acc += rew;
      if (do_reset) {
        a.seg_returns[(long)row * a.n_segs + cslot] = seg_acc;
        seg_acc = 0.f;
      }
    }
    __syncthreads();
  }

  // ---- epilogue: the open segment, live state back to the env's carry ---
  if (owner) {
    if (a.n_segs > a.n_cuts) a.seg_returns[(long)row * a.n_segs + a.n_cuts] = seg_acc;
    a.state[(long)row * 2] = s[0];
    a.state[(long)row * 2 + 1] = s[1];
    #pragma unroll
    for (int k = 0; k < 3; ++k) a.last_obs[(long)row * 3 + k] = cur[k];
  }
}

// Narrow: 4 waves, one 16-column tile each at width 64.  Wide: `wide_threads`
// is 256 (each wave loops over four tiles of a 256-wide layer) or 1024 (one
// tile per wave); the caller has checked it.
void launch_pendulum_collect_fused(const PendulumCollectArgs& a, int wide_threads,
                                   hipStream_t stream) {
  const dim3 g((a.N + ROLLOUT_ROWS - 1) / ROLLOUT_ROWS);
  const size_t lds = net_lds_floats(3, a.dims, a.n_layers) * sizeof(float);
  if (!net_is_wide(a.dims, a.n_layers))
    hipLaunchKernelGGL((pendulum_collect_fused_f32<256, false>), g, dim3(256), lds,
                       stream, a);
  else if (wide_threads == 1024)
    hipLaunchKernelGGL((pendulum_collect_fused_f32<1024, true>), g, dim3(1024), lds,
                       stream, a);
  else
    hipLaunchKernelGGL((pendulum_collect_fused_f32<256, true>), g, dim3(256), lds,
                       stream, a);
}
