// Per-row arithmetic of one rollout step, shared by the stand-alone
// kernels (fused_mlp_fwd_f32_t, mlp_layer_fwd_wide_f32, the gaussian /
// categorical / uniform sample kernels, the synthetic / cartpole / pendulum
// env step and reset kernels, replay_scatter_kernel) and the persistent
// kernels (rollout_fused_kernels.hip, cartpole_rollout_kernels.hip,
// pendulum_rollout_kernels.hip, pendulum_collect_kernels.hip,
// synthetic_collect_kernels.hip, eval_kernels.hip, ppo_ingest_kernels.hip).  Every caller inlines the SAME expressions in the SAME
// order, so both routes produce the same bytes; the operands may live in
// global memory or in LDS.
//
// The persistent kernels also share their net stage from here: net_stage
// (weight image -> LDS), net_forward (the per-step forward) and cut_slot.
// It has ONE definition so that a fix cannot reach some of them only.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"
#include "philox.h"

// One 16x16 output tile of a Linear layer from LDS-resident operands:
// activations buf_in[row][LDSW], weights wl[out][wrow] (padded image).
// Lane (i = lane & 15, k = lane >> 4) feeds A[arow][k0 + k] and
// W[j][k0 + k]; the k0 order is the accumulation order.
template <int LDSW, bool BF16>
DEV_INLINE f32x4 mlp_fwd_tile_lds(const float* buf_in, const float* wl, int wrow,
                                  int in_d, int arow, int k, int j, bool jok) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if constexpr (BF16) {
    // bf16 compute: v_mfma_f32_16x16x32_bf16, fp32 accumulate;
    // fragments built from the fp32 LDS images with RNE converts
    for (int k0 = 0; k0 < in_d; k0 += 32) {
      bf16x8 af, bf;
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int kk = k0 + k * 8 + e;
        af[e] = f32_to_bf16((kk < in_d) ? buf_in[arow * LDSW + kk] : 0.f);
        bf[e] = f32_to_bf16((jok && kk < in_d) ? wl[j * wrow + kk] : 0.f);
      }
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc, 0, 0, 0);
    }
  } else {
    for (int k0 = 0; k0 < in_d; k0 += 4) {
      const int kk = k0 + k;
      float a = (kk < in_d) ? buf_in[arow * LDSW + kk] : 0.f;
      float bv = (jok && kk < in_d) ? wl[j * wrow + kk] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0);
    }
  }
  return acc;
}

// bias + activation epilogue of one output tile into buf_out[row][LDSW]
// (C/D map: col = lane & 15, row = (lane >> 4) * 4 + r)
template <int LDSW>
DEV_INLINE void mlp_fwd_tile_epilogue(f32x4 acc, const float* B, int act, int j,
                                      bool jok, int wr0, int lane, float* buf_out) {
  if (jok) {
    const float bias = B[j];
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wr0 + (lane >> 4) * 4 + r;
      buf_out[row * LDSW + j] = act_apply(act, acc[r] + bias);
    }
  }
}

// One 16x16 output tile of a wide Linear layer (in_d up to MLP_MAX_WIDTH):
// activations from the LDS tile xt[16][LDSW], the weight row wrow[in_d] of
// output column j from global memory.  Lane (i = lane & 15, k = lane >> 4).
// The accumulation order is fixed: two chains over the 8-wide K blocks, the
// single 4-block and the ragged tail on the first chain, then acc += acc2.
// Shared by mlp_layer_fwd_wide_f32 and net_forward's wide regime.
template <int LDSW>
DEV_INLINE f32x4 mlp_fwd_tile_wide(const float* xt, const float* wrow, int in_d,
                                   int i, int k, bool jok) {
  const int in4 = in_d & ~3;
  const int in8 = in_d & ~7;
  // two independent accumulator chains double the MFMA/load ILP
  // (the K chain is otherwise a serial dependent sequence)
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < in8; k0 += 8) {
    float bv0 = 0.f, bv1 = 0.f;
    if (jok) {
      // every lane of a 16-lane group reads its K element of the
      // broadcast W chunk (4x fewer load instructions than scalar)
      bv0 = wrow[k0 + k];
      bv1 = wrow[k0 + 4 + k];
    }
    const float a0 = xt[i * LDSW + k0 + k];
    const float a1 = xt[i * LDSW + k0 + 4 + k];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv0, acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv1, acc2, 0, 0, 0);
  }
  for (int k0 = in8; k0 < in4; k0 += 4) {
    float bv = jok ? wrow[k0 + k] : 0.f;
    const float a = xt[i * LDSW + k0 + k];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0);
  }
  if (in4 < in_d) {  // ragged K tail
    const int kk = in4 + k;
    float a = (kk < in_d) ? xt[i * LDSW + kk] : 0.f;
    float bv = (jok && kk < in_d) ? wrow[kk] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0);
  }
  acc[0] += acc2[0]; acc[1] += acc2[1]; acc[2] += acc2[2]; acc[3] += acc2[3];
  return acc;
}

// ---- the net stage of the persistent kernels ------------------------------
// A workgroup of NT threads runs the net on a 16-row LDS tile every step.
// Narrow nets (net_is_wide false) keep the padded weight image and the biases
// in LDS from `wl` on, sized by net_lds_floats; wide nets read both from
// global memory.

// where net_stage left the biases, and the first free LDS float after them
struct NetStage {
  const float* bl;  // LDS bias image, layers back to back (nullptr when wide)
  float* end;
};

// prologue: (narrow) weights [out][in + 1] per layer, then biases -> LDS at
// wl.  The caller's barrier makes them visible.
template <int NT, bool WIDE>
DEV_INLINE NetStage net_stage(const NetArgs& a, float* wl, int tid) {
  if constexpr (WIDE) return {nullptr, wl};
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
  return {bl, bl + boff};
}

// the net's forward on the LDS-resident tile st[ROWS][LDSW], activations
// ping-ponging between buf0 and buf1; every thread of the workgroup calls it
// (it ends each layer with a barrier).  Returns the output tile [ROWS][LDSW],
// which never reaches HBM: buf0 or buf1 by the layer count, st without layers.
template <int NT, int LDSW, bool WIDE>
DEV_INLINE const float* net_forward(const NetArgs& a, const float* st, float* buf0,
                                    float* buf1, const float* wl, const float* bl,
                                    int wave, int lane) {
  constexpr int NW = NT / 64;
  const int i16 = lane & 15;
  const int k4 = lane >> 4;
  const float* buf_in = st;
  int wo = 0, bo = 0;
  for (int l = 0; l < a.n_layers; ++l) {
    const int in_d = a.dims[l], out_d = a.dims[l + 1];
    float* const buf_out = (l & 1) ? buf1 : buf0;
    for (int jt = wave * 16; jt < out_d; jt += 16 * NW) {
      const int j = jt + i16;
      const bool jok = j < out_d;
      if constexpr (WIDE) {
        const f32x4 acc = mlp_fwd_tile_wide<LDSW>(buf_in, a.w[l] + (long)j * in_d,
                                                  in_d, i16, k4, jok);
        mlp_fwd_tile_epilogue<LDSW>(acc, a.b[l], a.acts[l], j, jok, 0, lane, buf_out);
      } else {
        const f32x4 acc = mlp_fwd_tile_lds<LDSW, false>(buf_in, wl + wo, in_d + 1,
                                                        in_d, i16, k4, j, jok);
        mlp_fwd_tile_epilogue<LDSW>(acc, bl + bo, a.acts[l], j, jok, 0, lane, buf_out);
      }
    }
    __syncthreads();
    buf_in = buf_out;
    wo += out_d * (in_d + 1);
    bo += out_d;
  }
  return buf_in;
}

// lockstep truncation: the slot of step t in the host's ascending cut list,
// -1 when t is no cut
DEV_INLINE int cut_slot(const int* cut_step, int n_cuts, int t) {
  int slot = -1;
  for (int c = 0; c < n_cuts; ++c)
    if (cut_step[c] == t) slot = c;
  return slot;
}

// Diagonal-Gaussian log-prob of one row (gaussian_logp_kernel, loss_kernels.hip,
// and ppo_ingest_rows_f32, ppo_ingest_kernels.hip): the caller tabulates
// sigma[d] = __expf(log_std[d]) and the row-independent base once, then every
// row sums its squared z in d order.
DEV_INLINE float gaussian_logp_base(const float* log_std, int D) {
  float b = 0.f;
  for (int d = 0; d < D; ++d) b += log_std[d];
  return b + 0.5f * (float)D * LOG_2PI;
}

// The row's actions start at actions[aoff], its means at mean[moff].
DEV_INLINE float gaussian_logp_row(const float* __restrict__ actions, long aoff,
                                   const float* __restrict__ mean, long moff,
                                   const float* sigma, float base, int D) {
  float q = 0.f;
  for (int d = 0; d < D; ++d) {
    const float z = (actions[aoff + d] - mean[moff + d]) / sigma[d];
    q += z * z;
  }
  return -0.5f * q - base;
}

// one uniform action element in [low, high], keyed by (seed, offset, i)
DEV_INLINE float uniform_sample_elem(float low, float high, uint64_t seed,
                                     uint64_t offset, uint32_t i) {
  uint32_t r[4];
  philox4(seed, offset, i, r);
  return low + (high - low) * u32_to_open_unit(r[0]);
}

// slot of transition (row, t) of an epoch written instance-major from ring
// position `write` (already reduced modulo cap)
DEV_INLINE unsigned long long ring_slot(unsigned long long write,
                                        unsigned long long cap, int row, int steps,
                                        int t) {
  return (write + (unsigned long long)row * (unsigned long long)steps +
          (unsigned long long)t) % cap;
}

// one action element: mean + exp(log_std[d]) * z, z keyed by
// (seed, offset, i); noise_scale >= 0 overrides sigma, limit >= 0 clips
DEV_INLINE float gaussian_sample_elem(float mean, const float* log_std, int d,
                                      uint64_t seed, uint64_t offset, uint32_t i,
                                      float noise_scale, float limit) {
  uint32_t r[4];
  philox4(seed, offset, i, r);
  float z0, z1;
  box_muller(r[0], r[1], &z0, &z1);
  const float sigma = noise_scale >= 0.f ? noise_scale : __expf(log_std[d]);
  float a = mean + sigma * z0;
  if (limit >= 0.f) a = fminf(fmaxf(a, -limit), limit);
  return a;
}

// one env row on one wave: lane o owns state column o.
//   out_o  : true successor state element (pre-reset)
//   s_next : next live state element (autoreset draw when do_reset)
//   rsum   : the row's reward (valid on lane 0)
// All 64 lanes of the wave must call it (wave_reduce_sum).
DEV_INLINE void synthetic_env_row(const float* s, const float* a, const float* A,
                                  const float* Bm, const float* w, int row, int o,
                                  int O, int Adim, float sigma, uint64_t seed,
                                  uint64_t offset, int do_reset, float* out_o_p,
                                  float* s_next_p, float* rsum_p) {
  float r_part = 0.f;
  float out_o = 0.f;
  if (o < O) {
    float acc = 0.f;
    for (int k = 0; k < O; ++k) acc += s[k] * A[k * O + o];
    for (int j = 0; j < Adim; ++j) {
      const float aj = fminf(fmaxf(a[j], -1.f), 1.f);
      acc += aj * Bm[j * O + o];
    }
    if (sigma > 0.f)
      acc += sigma * philox_normal(seed, offset, (uint32_t)(row * O + o));
    out_o = tanhf(acc);
    r_part = out_o * w[o];
  }
  if (o == 0) {
    float pen = 0.f;
    for (int j = 0; j < Adim; ++j) {
      const float aj = fminf(fmaxf(a[j], -1.f), 1.f);
      pen += aj * aj;
    }
    r_part -= 0.1f * pen;
  }
  *rsum_p = wave_reduce_sum(r_part);
  float s_next = out_o;
  if (o < O && do_reset) {
    // offset+1 is the autoreset noise stream (host bumps the counter by 2
    // on reset steps so streams never collide)
    s_next = 0.1f * philox_normal(seed, offset + 1, (uint32_t)(row * O + o));
  }
  *out_o_p = out_o;
  *s_next_p = s_next;
}

// one categorical action: inverse CDF over softmax(logits[0..n)) on the
// uniform keyed by (seed, offset, row)
DEV_INLINE int categorical_sample_row(const float* lg, int n, uint64_t seed,
                                      uint64_t offset, uint32_t row) {
  float m = lg[0];
  for (int j = 1; j < n; ++j) m = fmaxf(m, lg[j]);
  float z = 0.f;
  for (int j = 0; j < n; ++j) z += __expf(lg[j] - m);
  uint32_t r[4];
  philox4(seed, offset, row, r);
  const float u = u32_to_open_unit(r[0]) * z;
  float acc = 0.f;
  int pick = n - 1;
  for (int j = 0; j < n; ++j) {
    acc += __expf(lg[j] - m);
    if (u <= acc) { pick = j; break; }
  }
  return pick;
}

// CartPole-v1 (envs/classic.py::CartPoleEnv._step_b): one Euler step of
// s = (x, x_dot, theta, theta_dot) in fp64, the host env's constants and
// expression order, no contraction.  Returns terminated.
DEV_INLINE bool cartpole_row_step(double s[4], int action) {
#pragma clang fp contract(off)
  constexpr double GRAVITY = 9.8;
  constexpr double MASSPOLE = 0.1;
  constexpr double TOTAL_MASS = 1.0 + 0.1;
  constexpr double LENGTH = 0.5;
  constexpr double POLEMASS_LENGTH = 0.1 * 0.5;
  constexpr double FORCE_MAG = 10.0;
  constexpr double TAU = 0.02;
  constexpr double THETA_THRESHOLD = 24.0 * 3.141592653589793 / 360.0;
  constexpr double X_THRESHOLD = 2.4;
  double x = s[0], x_dot = s[1], theta = s[2], theta_dot = s[3];
  const double force = action == 1 ? FORCE_MAG : -FORCE_MAG;
  const double costheta = cos(theta);
  const double sintheta = sin(theta);
  const double temp =
      (force + POLEMASS_LENGTH * (theta_dot * theta_dot) * sintheta) / TOTAL_MASS;
  const double thetaacc =
      (GRAVITY * sintheta - costheta * temp) /
      (LENGTH * (4.0 / 3.0 - MASSPOLE * (costheta * costheta) / TOTAL_MASS));
  const double xacc = temp - POLEMASS_LENGTH * thetaacc * costheta / TOTAL_MASS;
  x = x + TAU * x_dot;
  x_dot = x_dot + TAU * xacc;
  theta = theta + TAU * theta_dot;
  theta_dot = theta_dot + TAU * thetaacc;
  s[0] = x; s[1] = x_dot; s[2] = theta; s[3] = theta_dot;
  return fabs(x) > X_THRESHOLD || fabs(theta) > THETA_THRESHOLD;
}

// CartPole init state: four uniforms strictly inside (-0.05, 0.05) from ONE
// Philox call keyed by (seed, offset, row)
DEV_INLINE void cartpole_reset_draw(uint64_t seed, uint64_t offset, uint32_t row,
                                    double out[4]) {
#pragma clang fp contract(off)
  uint32_t r[4];
  philox4(seed, offset, row, r);
  #pragma unroll
  for (int k = 0; k < 4; ++k)
    out[k] = -0.05 + 0.1 * (((double)r[k] + 0.5) * (1.0 / 4294967296.0));
}

// one whole env row of VectorEnv.step semantics: Euler step, termination,
// truncation (max_steps <= 0: none), autoreset.  s/elapsed are updated in
// place to the next LIVE state; fin is the true successor observation,
// obs the post-autoreset one.  Returns done.
DEV_INLINE bool cartpole_env_row(double s[4], int* elapsed, int action,
                                 int max_steps, uint64_t seed, uint64_t offset,
                                 uint32_t row, float fin[4], float obs[4]) {
  const bool terminated = cartpole_row_step(s, action);
  const int el = *elapsed + 1;
  const bool truncated = max_steps > 0 && el >= max_steps && !terminated;
  const bool done = terminated || truncated;
  #pragma unroll
  for (int k = 0; k < 4; ++k) fin[k] = (float)s[k];
  if (done) cartpole_reset_draw(seed, offset, row, s);
  *elapsed = done ? 0 : el;
  #pragma unroll
  for (int k = 0; k < 4; ++k) obs[k] = (float)s[k];
  return done;
}

// Pendulum-v1 (envs/classic.py::PendulumEnv._step_b): one step of
// s = (theta, theta_dot) in fp64, the host env's constants and expression
// order, no contraction.  *reward = (float)(-costs) of the PRE-step state.
DEV_INLINE void pendulum_row_step(double s[2], float action, float* reward) {
#pragma clang fp contract(off)
  constexpr double PI = 3.141592653589793;
  constexpr double TWO_PI = 2.0 * 3.141592653589793;
  constexpr double MAX_SPEED = 8.0;
  constexpr double MAX_TORQUE = 2.0;
  constexpr double DT = 0.05;
  const double th = s[0], thdot = s[1];
  const double u = fmin(fmax((double)action, -MAX_TORQUE), MAX_TORQUE);
  // numpy's %: the result takes the sign of the (positive) divisor
  double ang = fmod(th + PI, TWO_PI);
  if (ang < 0.0) ang = ang + TWO_PI;
  ang = ang - PI;
  const double costs = ang * ang + 0.1 * (thdot * thdot) + 0.001 * (u * u);
  double newthdot = thdot + (15.0 * sin(th) + 3.0 * u) * DT;
  newthdot = fmin(fmax(newthdot, -MAX_SPEED), MAX_SPEED);
  const double newth = th + newthdot * DT;
  s[0] = newth; s[1] = newthdot;
  *reward = (float)(-costs);
}

// Pendulum init state: theta strictly inside (-pi, pi), theta_dot strictly
// inside (-1, 1), from ONE Philox call keyed by (seed, offset, row)
DEV_INLINE void pendulum_reset_draw(uint64_t seed, uint64_t offset, uint32_t row,
                                    double out[2]) {
#pragma clang fp contract(off)
  constexpr double PI = 3.141592653589793;
  uint32_t r[4];
  philox4(seed, offset, row, r);
  out[0] = -PI + (2.0 * PI) * (((double)r[0] + 0.5) * (1.0 / 4294967296.0));
  out[1] = -1.0 + 2.0 * (((double)r[1] + 0.5) * (1.0 / 4294967296.0));
}

// observation (cos theta, sin theta, theta_dot) in fp32
DEV_INLINE void pendulum_obs(const double s[2], float o[3]) {
  o[0] = (float)cos(s[0]);
  o[1] = (float)sin(s[0]);
  o[2] = (float)s[1];
}

// one whole env row of the lockstep step: transition, then (do_reset) the
// autoreset draw.  s is updated in place to the next LIVE state; fin is the
// true successor observation, obs the post-autoreset one.
DEV_INLINE void pendulum_env_row(double s[2], float action, int do_reset,
                                 uint64_t seed, uint64_t offset, uint32_t row,
                                 float fin[3], float obs[3], float* reward) {
  pendulum_row_step(s, action, reward);
  pendulum_obs(s, fin);
  if (do_reset) {
    pendulum_reset_draw(seed, offset, row, s);
    pendulum_obs(s, obs);
  } else {
    #pragma unroll
    for (int k = 0; k < 3; ++k) obs[k] = fin[k];
  }
}
