// One pass over a PPO epoch's rows, ahead of the captured update graph.
//
//   ppo_ingest_rows_f32  per 16-row tile of the T step rows + E bootstrap
//                        rows: value net, current policy and old policy on
//                        the LDS-resident tile; V(s) of every row, the old
//                        policy's log-prob and the current policy's log-prob
//                        of the step rows; and the copy of the epoch's
//                        observations, actions, rewards, episode offsets and
//                        done flags into the graph's capture-stable buffers
//
// It replaces, per epoch: the cat of observations and bootstrap observations,
// three mlp_forward launches that each read the same rows from HBM, two
// gaussian_logp launches and the copies into the graph's buffers.  It is the
// only kernel of the epoch's train side that sees per-epoch addresses.
//
// Rows < T come from `obs`, rows >= T from `last_obs[row - T]`; a tile may
// hold both kinds, and rows past T + E are zero and never written.  The three
// padded weight images stay in LDS for the launch (narrow nets only; the host
// checks ppo_ingest_lds_floats against the LDS budget).
//
// Results are byte-identical to mlp_forward + gaussian_logp: the net stage is
// the shared code of rollout_steps.h (net_stage / net_forward), the log-prob
// row is gaussian_logp_row of the same header.
#include "common.h"
#include "rollout_steps.h"

template <int NT>
__global__ __launch_bounds__(NT) void ppo_ingest_rows_f32(PPOIngestArgs a) {
  constexpr int LDSW = ROLLOUT_LDSW;
  constexpr int ROWS = ROLLOUT_ROWS;
  extern __shared__ float smem[];
  float* const st = smem;
  float* const buf0 = st + ROWS * LDSW;
  float* const buf1 = buf0 + ROWS * LDSW;
  float* const wl_val = buf1 + ROWS * LDSW;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int T = a.T, E = a.E, O = a.O, A = a.A;
  const int row0 = blockIdx.x * ROWS;

  const NetStage val = net_stage<NT, false>(a.val, wl_val, tid);
  float* const wl_pol = val.end;
  const NetStage pol = net_stage<NT, false>(a.pol, wl_pol, tid);
  float* const wl_old = pol.end;
  const NetStage old = net_stage<NT, false>(a.old, wl_old, tid);
  float* const sigma = old.end;      // [A] of the current policy
  float* const sigma_old = sigma + A;  // [A] of the old policy

  // the row tile, and the step rows' observations on their way through
  for (int idx = tid; idx < ROWS * O; idx += NT) {
    const int r = idx / O, c = idx % O;
    const int row = row0 + r;
    float v = 0.f;
    if (row < T) {
      v = a.obs[(long)row * O + c];
      a.obs_out[(long)row * O + c] = v;
    } else if (row < T + E) {
      v = a.last_obs[(long)(row - T) * O + c];
    }
    st[r * LDSW + c] = v;
  }
  for (int idx = tid; idx < ROWS * A; idx += NT) {
    const int row = row0 + idx / A;
    if (row < T) a.act_out[(long)row * A + idx % A] = a.actions[(long)row * A + idx % A];
  }
  // rewards, offsets and done flags pass through; the grid has at least
  // T + E threads, so the first workgroups cover them in one sweep
  for (int i = blockIdx.x * NT + tid; i < T; i += gridDim.x * NT) a.rew_out[i] = a.rewards[i];
  for (int i = blockIdx.x * NT + tid; i <= E; i += gridDim.x * NT) a.off_out[i] = a.offsets[i];
  for (int i = blockIdx.x * NT + tid; i < E; i += gridDim.x * NT) a.dones_out[i] = a.dones[i];
  for (int d = tid; d < A; d += NT) {
    sigma[d] = __expf(a.log_std[d]);
    sigma_old[d] = __expf(a.old_log_std[d]);
  }
  __syncthreads();

  // thread r < 16 owns row0 + r once a forward has left its output tile
  const int row = row0 + tid;
  const bool owner = tid < ROWS;

  const float* out =
      net_forward<NT, LDSW, false>(a.val, st, buf0, buf1, wl_val, val.bl, wave, lane);
  if (owner && row < T + E) a.values_all[row] = out[tid * LDSW];
  __syncthreads();  // the next forward writes the tile just read

  out = net_forward<NT, LDSW, false>(a.pol, st, buf0, buf1, wl_pol, pol.bl, wave, lane);
  if (owner && row < T)
    a.logp_now[row] = gaussian_logp_row(a.actions, (long)row * A, out, tid * LDSW, sigma,
                                        gaussian_logp_base(a.log_std, A), A);
  __syncthreads();

  out = net_forward<NT, LDSW, false>(a.old, st, buf0, buf1, wl_old, old.bl, wave, lane);
  if (owner && row < T)
    a.old_logp[row] = gaussian_logp_row(a.actions, (long)row * A, out, tid * LDSW,
                                        sigma_old, gaussian_logp_base(a.old_log_std, A), A);
}

// one workgroup of 4 waves per 16-row tile, one 16-column tile per wave at
// width 64 (the caller has checked every width and the LDS budget)
void launch_ppo_ingest_rows(const PPOIngestArgs& a, hipStream_t stream) {
  const dim3 g((a.T + a.E + ROLLOUT_ROWS - 1) / ROLLOUT_ROWS);
  const size_t lds = ppo_ingest_lds_floats(a.val.dims, a.val.n_layers, a.pol.dims,
                                           a.pol.n_layers) * sizeof(float);
  hipLaunchKernelGGL((ppo_ingest_rows_f32<256>), g, dim3(256), lds, stream, a);
}
