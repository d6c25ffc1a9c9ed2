// Off-policy (DDPG/TD3) hot-loop kernels.
//
// The reference's 50-iteration train loop (ddpg.py:195-253,
// td3.py:214-263) does per iteration: numpy minibatch gather + 5x
// from_numpy, a target chain (randn + clamp + add + clamp + two target-Q
// forwards + min + r+gamma(1-d)q), two critic MSE steps and a delayed
// actor step.  On MI355X the whole loop is device-resident; these
// kernels cover the three pieces the fused-MLP/loss/Adam kernels don't:
//
//   replay_gather_kernel  one kernel draws the minibatch indices
//                         (counter-based Philox -> graph-replay safe)
//                         and gathers obs|act (pre-concatenated as the
//                         critic input), next_obs, rewards, dones from
//                         the HBM ring -- replaces randint + 5
//                         index_selects + torch.cat
//   td3_smooth_kernel     target-policy smoothing: clamp(a +
//                         clamp(scale*z, +-clip), +-limit) in one pass
//   q_target_min2_kernel  min-twin bootstrap target
//
// and the collection side of a device-env epoch (replay_scatter_kernel,
// ring_advance_kernel, at the end of this file).
//
// The first three read their RNG offset through an optional device counter so
// a hipGraph replay of the whole train loop draws fresh randomness
// (same pattern as sample_kernels.hip).
#include "common.h"
#include "philox.h"
#include "rollout_steps.h"

// out = clamp(a + clamp(scale * z, -clip, clip), -limit, limit)
// (reference td3.py:325-341)
__global__ __launch_bounds__(256) void td3_smooth_kernel(
    const float* __restrict__ a, float* __restrict__ out, int total,
    uint64_t seed, uint64_t offset, float scale, float clip, float limit,
    const unsigned long long* __restrict__ offset_ptr) {
  if (offset_ptr) offset += *offset_ptr;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total;
       i += gridDim.x * 256) {
    float eps = scale * philox_normal(seed, offset, (uint32_t)i);
    eps = fminf(fmaxf(eps, -clip), clip);
    float v = a[i] + eps;
    out[i] = fminf(fmaxf(v, -limit), limit);
  }
}

// out = r + gamma * (1 - d) * min(q1, q2)   (reference td3.py:335-341)
__global__ __launch_bounds__(256) void q_target_min2_kernel(
    const float* __restrict__ r, const float* __restrict__ d,
    const float* __restrict__ q1, const float* __restrict__ q2,
    float* __restrict__ out, float gamma, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    out[i] = r[i] + gamma * (1.f - d[i]) * fminf(q1[i], q2[i]);
  }
}

// Minibatch gather from the HBM replay ring (replay_buffer.py).
// Row i's index is Philox-keyed by (seed, offset, i) modulo the CURRENT
// buffer size, which is read from a device scalar so one captured graph
// keeps sampling correctly as the ring fills between epochs.  Each row
// writes:
//   qin[i]      = [obs(idx) | act(idx)]   (critic input, pre-concatenated)
//   obs_out[i]  = obs(idx)                (actor input, contiguous)
//   nxt_out[i]  = next_obs(idx)
//   rew_out[i], dn_out[i]
__global__ __launch_bounds__(256) void replay_gather_kernel(
    ReplayGatherArgs a) {
  uint64_t offset = a.offset;
  if (a.offset_ptr) offset += *a.offset_ptr;
  const uint32_t size = (uint32_t)*a.size;
  const int row_elems = 2 * a.O + a.A + 2;
  const long total = (long)a.B * row_elems;
  for (long t = blockIdx.x * 256 + threadIdx.x; t < total;
       t += (long)gridDim.x * 256) {
    const int row = (int)(t / row_elems);
    const int e = (int)(t % row_elems);
    uint32_t r4[4];
    philox4(a.seed, offset, (uint32_t)row, r4);
    const long idx = (long)(r4[0] % size);
    if (e < a.O) {
      const float v = a.obs[idx * a.O + e];
      a.qin[(long)row * (a.O + a.A) + e] = v;
      a.obs_out[(long)row * a.O + e] = v;
    } else if (e < a.O + a.A) {
      const int c = e - a.O;
      a.qin[(long)row * (a.O + a.A) + a.O + c] = a.act[idx * a.A + c];
    } else if (e < 2 * a.O + a.A) {
      const int c = e - a.O - a.A;
      a.nxt_out[(long)row * a.O + c] = a.nxt[idx * a.O + c];
    } else if (e == 2 * a.O + a.A) {
      a.rew_out[row] = a.rew[idx];
    } else {
      a.dn_out[row] = a.dn[idx];
    }
  }
}

// Ring write of one captured collect epoch (the multi-kernel bodies of
// ops/fused_rollout.py::GraphedPendulumCollect / GraphedSyntheticCollect):
// the epoch's buffers go to the slots (write + row * steps + t) % cap, the
// slots, values and segment sums of the persistent collect kernels, for any
// O = ring.O and A = ring.A.  Cut steps store the pre-reset successor from
// cut_final and done = 1.  Two passes over disjoint outputs: the O + O + A
// row elements of every transition, one thread each; then one thread per
// instance walks its rewards in step order (the segment sums' order).
__global__ __launch_bounds__(256) void replay_scatter_kernel(ReplayScatterArgs a) {
  const unsigned long long cap = a.ring.cap;
  const unsigned long long write = (unsigned long long)*a.ring.write % cap;
  const int N = a.N, steps = a.steps, O = a.ring.O, A = a.ring.A;
  const int row_elems = 2 * O + A;
  const long total = (long)N * steps * row_elems;
  for (long i = blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int e = (int)(i % row_elems);
    const long rt = i / row_elems;
    const int t = (int)(rt % steps), row = (int)(rt / steps);
    const unsigned long long slot = ring_slot(write, cap, row, steps, t);
    if (e < O) {
      a.ring.obs[slot * O + e] = a.obs_full[((long)t * N + row) * O + e];
    } else if (e < 2 * O) {
      const int k = e - O;
      int cslot = a.cut_slot[t];
      if (cslot >= a.n_cuts) cslot = -1;  // device data: never past cut_final
      a.ring.nxt[slot * O + k] = cslot >= 0
                                     ? a.cut_final[((long)cslot * N + row) * O + k]
                                     : a.obs_full[((long)(t + 1) * N + row) * O + k];
    } else {
      const int d = e - 2 * O;
      a.ring.act[slot * A + d] = a.act_buf[((long)t * N + row) * A + d];
    }
  }
  for (int row = blockIdx.x * 256 + threadIdx.x; row < N; row += gridDim.x * 256) {
    float seg_acc = 0.f;
    int cslot = -1;
    for (int t = 0; t < steps; ++t) {
      cslot = a.cut_slot[t];
      if (cslot >= a.n_cuts) cslot = -1;
      const unsigned long long slot = ring_slot(write, cap, row, steps, t);
      const float rew = a.rew_buf[(long)t * N + row];
      a.ring.rew[slot] = rew;
      a.ring.dn[slot] = cslot >= 0 ? 1.f : 0.f;
      seg_acc += rew;
      if (cslot >= 0) {
        a.seg_returns[(long)row * a.n_segs + cslot] = seg_acc;
        seg_acc = 0.f;
      }
    }
    // the open segment (the last step is no cut)
    if (cslot < 0) a.seg_returns[(long)row * a.n_segs + a.n_segs - 1] = seg_acc;
  }
}

// the ring's device scalars after n transitions were written:
// write = (write + n) % cap, size = min(size + n, cap); one thread
__global__ void ring_advance_kernel(long long* write, long long* size,
                                    unsigned long long n, unsigned long long cap) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const unsigned long long w = (unsigned long long)*write % cap;
    *write = (long long)((w + n) % cap);
    const unsigned long long sz = *size < 0 ? 0ull : (unsigned long long)*size;
    *size = (long long)(sz + n < cap ? sz + n : cap);
  }
}
