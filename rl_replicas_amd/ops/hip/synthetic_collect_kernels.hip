// Persistent replay collection on the synthetic envs: the whole epoch's
// steps x (behaviour action -> synthetic transition with lockstep autoreset
// on the host-known cut steps -> replay-ring write) in ONE launch, for the
// two behaviour policies of an off-policy epoch (the modes of
// pendulum_collect_kernels.hip):
//
//   COLLECT_NOISED   actor forward, then per element mean + noise_scale * z
//                    clipped to +-limit
//   COLLECT_UNIFORM  uniform in [low, high] per element; no net is read
//
// A workgroup owns 16 env rows for the whole epoch, as in
// rollout_fused_kernels.hip: the live state tile ping-pongs between two LDS
// tiles, the env matrices stay in LDS, and the transition keeps the
// one-wave-per-row mapping of synthetic_env_step_kernel (lane o owns state
// column o, the same reward reduction tree).  Every transition goes straight
// to its ring slot (write + row * steps + t) % cap, the instance-major order
// ReplayBuffer._add_flat_tensors produces; nothing is staged.
//
// The two weight regimes are those of pendulum_collect_fused_f32 (net_stage /
// net_forward of rollout_steps.h, chosen on the host by net_is_wide; LDS
// sized by synthetic_collect_lds_floats, common.h).
//
// Philox streams (GraphedRollout's layout): action element (row, d) of step
// t at (action_seed, t + ctr, row * A + d), dynamics noise at 2t + ctr and
// the autoreset draw at 2t + 1 + ctr (env_seed, row * O + o), the epoch reset
// at 2 * steps + ctr.  Results are byte-identical to the multi-kernel body
// (mlp_forward -> gaussian_sample | uniform_sample -> synthetic_env_step,
// then replay_scatter).
#include "common.h"
#include "philox.h"
#include "rollout_steps.h"

template <int NT, bool WIDE>
__global__ __launch_bounds__(NT) void synthetic_collect_fused_f32(SyntheticCollectArgs a) {
  constexpr int LDSW = WIDE ? ROLLOUT_WIDE_LDSW : ROLLOUT_LDSW;
  constexpr int ROWS = ROLLOUT_ROWS;
  constexpr int NW = NT / 64;
  constexpr int RPW = ROWS / NW;  // env rows per wave in the transition part
  static_assert(ROWS % NW == 0, "a wave owns a whole number of rows");
  extern __shared__ float smem[];
  float* const st0 = smem;
  float* const st1 = st0 + ROWS * LDSW;
  float* const buf0 = st1 + ROWS * LDSW;
  float* const buf1 = buf0 + ROWS * LDSW;
  float* const actt = buf1 + ROWS * LDSW;
  float* const wl = actt + ROWS * LDSW;  // narrow only

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int row0 = blockIdx.x * ROWS;
  const int N = a.N, O = a.O, A = a.A, steps = a.steps;
  const uint64_t ctr = *a.ctr;  // read once; the bump is a later graph node
  // read once and reduced: whatever the scalar holds, slots stay in the ring
  const unsigned long long cap = a.ring.cap;
  const unsigned long long write = (unsigned long long)*a.ring.write % cap;

  // ---- prologue: (narrow) weights, biases, then env matrices -> LDS ------
  const NetStage net = net_stage<NT, WIDE>(a, wl, tid);
  float* const eA = net.end;
  float* const eB = eA + O * O;
  float* const ew = eB + A * O;
  for (int idx = tid; idx < O * O; idx += NT) eA[idx] = a.envA[idx];
  for (int idx = tid; idx < A * O; idx += NT) eB[idx] = a.envB[idx];
  for (int idx = tid; idx < O; idx += NT) ew[idx] = a.envw[idx];

  // starting state of this workgroup's rows: the lockstep reset draw
  // (synthetic_env_reset_kernel's stream) or the carry, which this workgroup
  // alone overwrites in the epilogue
  for (int idx = tid; idx < ROWS * LDSW; idx += NT) {
    const int r = idx / LDSW, o = idx % LDSW;
    const int row = row0 + r;
    float v = 0.f;
    if (row < N && o < O) {
      const int i = row * O + o;
      v = a.start_with_reset
              ? 0.1f * philox_normal(a.env_seed, (uint64_t)(2 * steps) + ctr, (uint32_t)i)
              : a.carry[i];
    }
    st0[idx] = v;
    st1[idx] = 0.f;
    actt[idx] = 0.f;
  }
  __syncthreads();

  float seg_acc[RPW];  // reward sums of the running segment (lane 0)
  #pragma unroll
  for (int ri = 0; ri < RPW; ++ri) seg_acc[ri] = 0.f;

  for (int t = 0; t < steps; ++t) {
    const float* const st = (t & 1) ? st1 : st0;
    float* const st_next = (t & 1) ? st0 : st1;

    // ---- actor forward on the LDS-resident state tile -------------------
    // (unread in uniform mode: no layers)
    const float* const mean =
        net_forward<NT, LDSW, WIDE>(a, st, buf0, buf1, wl, net.bl, wave, lane);

    // ---- behaviour action, element (row, d) -> LDS tile and ring ---------
    const uint64_t aoff = (uint64_t)t + ctr;
    for (int idx = tid; idx < ROWS * A; idx += NT) {
      const int r = idx / A, d = idx % A;
      const int row = row0 + r;
      if (row < N) {
        const uint32_t i = (uint32_t)(row * A + d);
        float av;
        if (a.mode == COLLECT_UNIFORM)
          av = uniform_sample_elem(a.low, a.high, a.action_seed, aoff, i);
        else  // noise_scale >= 0 (host-checked): log_std is never read
          av = gaussian_sample_elem(mean[r * LDSW + d], nullptr, 0, a.action_seed, aoff,
                                    i, a.noise_scale, a.limit);
        actt[r * LDSW + d] = av;
        a.ring.act[ring_slot(write, cap, row, steps, t) * A + d] = av;
      }
    }
    __syncthreads();

    // lockstep truncation: the host's cut list says whether step t resets
    const int cslot = cut_slot(a.cut_step, a.n_cuts, t);
    const int do_reset = cslot >= 0;

    // ---- env transition + ring write: one wave per row -------------------
    #pragma unroll
    for (int ri = 0; ri < RPW; ++ri) {
      const int r = wave + ri * NW;
      const int row = row0 + r;
      if (row < N) {  // wave-uniform; no barrier inside this loop
        float out_o, s_next, rsum;
        synthetic_env_row(st + r * LDSW, actt + r * LDSW, eA, eB, ew, row, lane, O, A,
                          a.sigma, a.env_seed, (uint64_t)(2 * t) + ctr, do_reset,
                          &out_o, &s_next, &rsum);
        const unsigned long long slot = ring_slot(write, cap, row, steps, t);
        if (lane < O) {
          a.ring.obs[slot * O + lane] = st[r * LDSW + lane];  // what the action saw
          a.ring.nxt[slot * O + lane] = out_o;  // the true successor, pre-reset
          st_next[r * LDSW + lane] = s_next;
        }
        if (lane == 0) {
          a.ring.rew[slot] = rsum;
          a.ring.dn[slot] = do_reset ? 1.f : 0.f;
          seg_acc[ri] += rsum;
          if (do_reset) {
            a.seg_returns[(long)row * a.n_segs + cslot] = seg_acc[ri];
            seg_acc[ri] = 0.f;
          }
        }
      }
    }
    __syncthreads();
  }

  // ---- epilogue: the open segment, live state back to the carry ----------
  const float* const live = (steps & 1) ? st1 : st0;
  #pragma unroll
  for (int ri = 0; ri < RPW; ++ri) {
    const int r = wave + ri * NW;
    const int row = row0 + r;
    if (row < N) {
      if (lane == 0 && a.n_segs > a.n_cuts)
        a.seg_returns[(long)row * a.n_segs + a.n_cuts] = seg_acc[ri];
      if (lane < O) a.carry[(long)row * O + lane] = live[r * LDSW + lane];
    }
  }
}

// Narrow: 4 waves, one 16-column tile each at width 64, four env rows per
// wave.  Wide: `wide_threads` is 256 or 1024 (one tile and one env row per
// wave); the caller has checked it.
void launch_synthetic_collect_fused(const SyntheticCollectArgs& a, int wide_threads,
                                    hipStream_t stream) {
  const dim3 g((a.N + ROLLOUT_ROWS - 1) / ROLLOUT_ROWS);
  const size_t lds =
      synthetic_collect_lds_floats(a.dims, a.n_layers, a.O, a.A) * sizeof(float);
  if (!net_is_wide(a.dims, a.n_layers))
    hipLaunchKernelGGL((synthetic_collect_fused_f32<256, false>), g, dim3(256), lds,
                       stream, a);
  else if (wide_threads == 1024)
    hipLaunchKernelGGL((synthetic_collect_fused_f32<1024, true>), g, dim3(1024), lds,
                       stream, a);
  else
    hipLaunchKernelGGL((synthetic_collect_fused_f32<256, true>), g, dim3(256), lds,
                       stream, a);
}
