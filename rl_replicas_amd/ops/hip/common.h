// Shared device helpers for the rl_replicas_amd CDNA4 (gfx950) kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define WAVE 64
#define DEV_INLINE __device__ __forceinline__

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __hip_bfloat16 bf16_t;
// bf16 MFMA fragment: 8 elements per lane (v_mfma_f32_16x16x32_bf16)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

DEV_INLINE __bf16 f32_to_bf16(float v) {
  return (__bf16)v;  // hardware RNE conversion on gfx950
}

// activation codes shared with python (ops/fused_mlp.py)
#define ACT_IDENTITY 0
#define ACT_TANH 1
#define ACT_RELU 2

DEV_INLINE float act_apply(int code, float x) {
  switch (code) {
    case ACT_TANH: return tanhf(x);
    case ACT_RELU: return x > 0.f ? x : 0.f;
    default: return x;
  }
}

// derivative of the activation expressed through the POST-activation y
// (tanh' = 1 - y^2, relu' = y > 0), so backward only needs saved outputs
DEV_INLINE float act_grad_from_y(int code, float y) {
  switch (code) {
    case ACT_TANH: return 1.f - y * y;
    case ACT_RELU: return y > 0.f ? 1.f : 0.f;
    default: return 1.f;
  }
}

// PPO/VPG gradient coefficient wrt logp for one row (caller scales by
// 1/B):  mode 0 = VPG (-A), mode 1 = PPO clipped surrogate.  Gradient
// semantics replicate torch exactly (min-tie 0.5/0.5, clamp-inclusive).
#define LOG_2PI 1.8378770664093453f
DEV_INLINE float dlogp_coeff(int mode, float logp, float old_logp, float adv,
                             float clip, float* loss_out) {
  if (mode == 0) {
    *loss_out = -logp * adv;
    return -adv;
  }
  const float ratio = __expf(logp - old_logp);
  const float lo = 1.f - clip, hi = 1.f + clip;
  const float rc = fminf(fmaxf(ratio, lo), hi);
  const float s1 = ratio * adv;
  const float s2 = rc * adv;
  *loss_out = -fminf(s1, s2);
  const float g1 = (s1 < s2) ? 1.f : (s1 == s2 ? 0.5f : 0.f);
  const float inclip = (ratio >= lo && ratio <= hi) ? 1.f : 0.f;
  return -(g1 * s1 + (1.f - g1) * inclip * s1);
}

// log-sum-exp of one row of n logits (max-shifted).  The one definition:
// the categorical loss kernels (loss_kernels.hip) and the categorical-PPO
// seed of the fused iteration (mlp_kernels.hip) both take logp from it.
DEV_INLINE float row_lse(const float* logits, int n) {
  float m = logits[0];
  for (int j = 1; j < n; ++j) m = fmaxf(m, logits[j]);
  float s = 0.f;
  for (int j = 0; j < n; ++j) s += __expf(logits[j] - m);
  return m + __logf(s);
}

// wave-level f32 sum (64 lanes)
DEV_INLINE float wave_reduce_sum(float v) {
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// One row of the deferred value-loss finalize on one wave
// (value_loss_finalize_rows, loss_kernels.hip, and ppo_epoch_epilogue,
// update_kernels.hip): the wave loads 64 partials per coalesced access and
// every lane then adds them lane by lane (v_readlane), in the serial order
// from 0.f of loss_partials_finalize.  All 64 lanes must call it.
DEV_INLINE void value_loss_row_sum(const float* __restrict__ partials,
                                   float* __restrict__ scalars, int r, int fb,
                                   int row_stride, int lane) {
  const float* row = partials + (long)r * row_stride;
  float s = 0.f;
  for (int p0 = 0; p0 < fb; p0 += 64) {
    const int v = p0 + lane < fb ? __float_as_int(row[p0 + lane]) : 0;
    const int n = min(64, fb - p0);  // pads are never added
    for (int p = 0; p < n; ++p)
      s += __int_as_float(__builtin_amdgcn_readlane(v, p));
  }
  if (lane == 0) scalars[r] = s;
}

// Fused-MLP static limits.  Python reads them from the extension
// (fused_mlp_limits); ops/fused_mlp.py keeps MAX_LAYERS / MAX_WIDTH for
// hosts without it, and a GPU test holds the two equal.
#define MLP_MAX_LAYERS 5
#define MLP_MAX_WIDTH 256
// widest layer of the kernels that keep a whole net's padded weight image
// in LDS beside [rows][MLP_NARROW_WIDTH + 4] activation tiles
#define MLP_NARROW_WIDTH 64
// dynamic-LDS budget per workgroup of those kernels and of the persistent
// rollout kernel: 100 of the CU's 160 KiB
#define MLP_LDS_BUDGET ((size_t)100 * 1024)
#define GAUSS_MAX_D 512  // Gaussian loss kernels' LDS sigma table bound

// kernel-argument block for the fused MLP kernels (passed by value)
struct MLPArgs {
  const float* w[MLP_MAX_LAYERS];
  const float* b[MLP_MAX_LAYERS];
  float* h[MLP_MAX_LAYERS];  // saved post-activation outputs (h[L-1] = final out)
  int dims[MLP_MAX_LAYERS + 1];
  int acts[MLP_MAX_LAYERS];
  int n_layers;
  int batch;
};

// whole-net fused-backward argument block (mlp_kernels.hip)
struct MLPBwdArgs {
  const float* w[MLP_MAX_LAYERS];
  const float* h[MLP_MAX_LAYERS];  // post-activations; h[L-1] = final out
  const float* b[MLP_MAX_LAYERS];  // biases (DO_FWD mode only)
  int dims[MLP_MAX_LAYERS + 1];
  int acts[MLP_MAX_LAYERS];
  int n_layers;
  int batch;
  long ws_stride;
  int layer_off[MLP_MAX_LAYERS];  // flat elem offset of each layer's partials
};

// all-layer gradient-reduction argument block (mlp_kernels.hip).
// workspace layout: ws[partial][flat-elem] with the layers' (od*id+od)
// segments concatenated in layer order inside each partial row.
struct ReduceAllArgs {
  const float* ws;            // [n_blocks][stride]
  long stride;                // flat elems per partial row (grand total)
  float* dw[MLP_MAX_LAYERS];
  float* db[MLP_MAX_LAYERS];
  int total[MLP_MAX_LAYERS];  // od*id + od per layer
  int wsize[MLP_MAX_LAYERS];  // od*id (split point)
  int n_layers;
  int n_blocks;
};

// multi-tensor update argument blocks (update_kernels.hip / bindings.hip)
#define MT_MAX_TENSORS 16

struct AdamArgs {
  float* p[MT_MAX_TENSORS];
  float* g[MT_MAX_TENSORS];
  float* m[MT_MAX_TENSORS];
  float* v[MT_MAX_TENSORS];
  float* step[MT_MAX_TENSORS];  // scalar step counters (fp32, torch-compatible)
  int numel[MT_MAX_TENSORS];
  int n_tensors;
  float lr, beta1, beta2, eps, weight_decay;
  // added to step[t] when computing bias correction (captured value loop
  // bakes per-iteration deltas so ONE bump per graph suffices); also the
  // bump amount for adam_step_bump_kernel
  float step_delta;
  // optional device gate: update and bump are skipped while *gate == 0
  // (captured PPO policy loop: KL early stop without host control flow)
  const float* gate;
};

struct PolyakArgs {
  const float* src[MT_MAX_TENSORS];
  float* dst[MT_MAX_TENSORS];
  int numel[MT_MAX_TENSORS];
  int n_tensors;
  float rho;
};

// merged gradient-reduce + Adam update (mlp_kernels.hip): consumes the
// backward stage-1 workspace and applies the optimizer in the SAME
// kernel — no dw/db round trip through HBM, one fewer dependent launch
// per optimizer step in the captured loops
struct ReduceAdamArgs {
  const float* ws;  // [n_blocks][stride] partials
  long stride;
  float* pw[MLP_MAX_LAYERS];
  float* pb[MLP_MAX_LAYERS];
  float* mw[MLP_MAX_LAYERS];
  float* mb[MLP_MAX_LAYERS];
  float* vw[MLP_MAX_LAYERS];
  float* vb[MLP_MAX_LAYERS];
  const float* step;  // shared pre-bump step counter (params step in lockstep)
  int total[MLP_MAX_LAYERS];
  int wsize[MLP_MAX_LAYERS];
  int n_layers, n_blocks;
  float lr, beta1, beta2, eps, weight_decay, step_delta;
  const float* gate;  // optional: skip entirely while *gate == 0
  // optional PPO gate bookkeeping (kl_partials != nullptr; needs gate):
  // the kernel sums the fused iteration kernel's per-block pending-KL /
  // loss partials itself, applies the KL early-stop rule and gates its
  // own Adam update on the result (reduce_adam_gate_closed, mlp_kernels.hip)
  const float* kl_partials;    // [n_blocks]
  const float* loss_partials;  // [n_blocks]
  float* gate_rw;              // == gate, writable (workgroup 0 only)
  float* kl_final;
  float* iters_done;
  float* loss_out;
  float inv_b, thr;
  int first_iter;
};

// Gaussian-PPO seed for the DO_FWD fused backward (mlp_kernels.hip):
// when `actions` is non-null the dZ seed of the last (identity-head)
// layer is the PPO clipped-surrogate gradient computed from the
// LDS-resident forward output, and the kernel additionally emits
// per-block loss partials, pending-KL partials, and dlog_std partials
// (written into the stage-1 workspace at dls_off as a pseudo-layer).
// kind == SEED_CATEGORICAL: the head tile holds N = dims[L] logits per row,
// `actions` is [B] (class index as fp32), the dZ seed is the clipped
// surrogate's gradient through the row softmax, and there is no pseudo-
// layer (log_std / dls_off unused).  The host picks the kernel
// instantiation from `kind`; the Gaussian one never reads it.
#define SEED_GAUSSIAN 0
#define SEED_CATEGORICAL 1
struct GaussSeedArgs {
  const float* actions;   // [B, D]; nullptr -> plain dy/mse seed
  const float* old_logp;  // [B]
  const float* adv;       // [B]
  const float* log_std;   // [D]
  float* kl_partials;     // [n_blocks]
  int dls_off;            // flat ws offset of the dlog_std pseudo-layer
  float clip;
  int kind;               // SEED_GAUSSIAN | SEED_CATEGORICAL
  // optional: the whole kernel returns at once while *skip_gate == 0 (a
  // gate-frozen policy iteration; its partials are never read then)
  const float* skip_gate;
};

// twin PPO update launch (mlp_bwd_fused_twin_f32): the PPO policy half
// (Gaussian or categorical seed, gauss.kind) and the value-MSE half of one
// update iteration, each with its own net, workspace and partials; both
// read the same x.  ~0.5 KB by value.
struct MLPBwdTwinArgs {
  MLPBwdArgs pol;
  GaussSeedArgs gauss;
  float* pol_ws;
  float* pol_loss_partials;  // [n_blocks]
  MLPBwdArgs val;
  float* val_ws;
  const float* returns;      // [B]
  float* val_loss_partials;  // [n_blocks] (the caller's deferred-loss row)
  const float* x;            // [B, dims[0]] of both nets
};

// The persistent kernels (rollout, collect, evaluation): one workgroup
// carries ROLLOUT_ROWS env rows through a whole epoch or episode.
#define ROLLOUT_ROWS 16
#define ROLLOUT_MAX_WIDTH 64  // widest layer / obs dim (one wave per env row)
#define ROLLOUT_LDSW (ROLLOUT_MAX_WIDTH + 4)  // LDS row stride of the 16-row tiles
#define ROLLOUT_MAX_CUTS 16   // lockstep truncation cuts per captured epoch
// LDS row stride of the wide regime's 16-row activation tiles
#define ROLLOUT_WIDE_LDSW (MLP_MAX_WIDTH + 4)

// the net every persistent kernel's argument block starts with
struct NetArgs {
  const float* w[MLP_MAX_LAYERS];
  const float* b[MLP_MAX_LAYERS];
  int dims[MLP_MAX_LAYERS + 1];
  int acts[MLP_MAX_LAYERS];
  int n_layers;
};

// The persistent kernels' weight regime, by mlp_forward's own rule: narrow
// (every width <= MLP_NARROW_WIDTH) keeps the padded whole-net weight image
// in LDS, wide reads the weights from global memory.
__host__ __device__ inline bool net_is_wide(const int* dims, int n_layers) {
  for (int l = 0; l <= n_layers; ++l)
    if (dims[l] > MLP_NARROW_WIDTH) return true;
  return false;
}

// LDS floats of a persistent kernel's net stage: `tiles` 16-row tiles;
// narrow nets add the padded weight image ([out][in + 1] per layer) and the
// biases.  Host sizing, launchers and *_lds_bytes all take it from here.
__host__ __device__ inline long net_lds_floats(int tiles, const int* dims,
                                               int n_layers) {
  if (net_is_wide(dims, n_layers)) return (long)tiles * ROLLOUT_ROWS * ROLLOUT_WIDE_LDSW;
  long n = (long)tiles * ROLLOUT_ROWS * ROLLOUT_LDSW;
  for (int l = 0; l < n_layers; ++l) n += dims[l + 1] * (dims[l] + 1) + dims[l + 1];
  return n;
}

// persistent rollout kernel (rollout_fused_kernels.hip): one workgroup
// carries ROLLOUT_ROWS env rows through all `steps` iterations of
// forward -> Gaussian sample -> synthetic env transition.
struct RolloutFusedArgs : NetArgs {
  const float* log_std;  // [A]
  const float* envA;     // [O, O]
  const float* envB;     // [A, O]
  const float* envw;     // [O]
  float* obs_full;       // [steps + 1, N, O]; slot `steps` is the carry
  float* act_buf;        // [steps, N, A]
  float* rew_buf;        // [steps, N]
  float* cut_final;      // [n_cuts, N, O] pre-reset successors, cut order
  const unsigned long long* ctr;  // device RNG counter (read once)
  int cut_step[ROLLOUT_MAX_CUTS];  // ascending
  int n_cuts;
  int N, O, A, steps;
  int start_with_reset;  // 1: Philox reset; 0: continue from the carry slot
  float sigma;           // env dynamics noise
  uint64_t policy_seed, env_seed;
};

// its LDS floats: 2 state tiles (step ping-pong) + 2 activation tiles + 1
// action tile and the net, then log_std and env A/B/w
__host__ __device__ inline long rollout_fused_lds_floats(const int* dims, int n_layers,
                                                         int O, int A) {
  return net_lds_floats(5, dims, n_layers) + A + O * O + A * O + O;
}

// persistent CartPole rollout kernel (cartpole_rollout_kernels.hip): one
// workgroup carries ROLLOUT_ROWS instances through all `steps` iterations
// of forward -> categorical sample -> Euler step / termination / autoreset.
struct CartPoleRolloutArgs : NetArgs {  // dims[0] == 4 (obs), dims[L] == n_act
  double* state;           // [N, 4] env carry (read unless start_with_reset)
  int* elapsed;            // [N]    env carry
  float* obs_full;         // [steps + 1, N, 4]
  float* final_obs;        // [steps, N, 4] true successors
  long long* act_buf;      // [steps, N]
  float* rew_buf;          // [steps, N]
  unsigned char* done_buf; // [steps, N]
  const unsigned long long* ctr;  // device RNG counter (read once)
  int N, steps, max_steps;
  int start_with_reset;
  uint64_t policy_seed, env_seed;
};

// persistent Pendulum rollout kernel (pendulum_rollout_kernels.hip): one
// workgroup carries ROLLOUT_ROWS instances through all `steps` iterations
// of forward -> Gaussian sample -> transition / lockstep autoreset.
struct PendulumRolloutArgs : NetArgs {  // dims[0] == 3 (obs), dims[L] == 1 (torque)
  const float* log_std;    // [1]
  double* state;           // [N, 2] env carry (read unless start_with_reset)
  float* obs_full;         // [steps + 1, N, 3]
  float* act_buf;          // [steps, N, 1]
  float* rew_buf;          // [steps, N]
  float* cut_final;        // [n_cuts, N, 3] pre-reset successors, cut order
  const unsigned long long* ctr;  // device RNG counter (read once)
  int cut_step[ROLLOUT_MAX_CUTS];  // ascending
  int n_cuts;
  int N, steps;
  int start_with_reset;
  uint64_t policy_seed, env_seed;
};

// The replay ring as the collect kernels see it (replay_buffer.py): the five
// storage tensors, the capacity, and the write position held on the device.
// Kernels reduce *write modulo cap before use, so no value of the scalar
// can index outside the storage.
struct ReplayRing {
  float* obs;   // [cap, O]
  float* act;   // [cap, A]
  float* rew;   // [cap]
  float* nxt;   // [cap, O]
  float* dn;    // [cap]
  const long long* write;  // device scalar: next slot to write
  unsigned long long cap;
  int O, A;     // floats per slot of obs / nxt and of act (Pendulum: 3, 1)
};

// persistent Pendulum replay collection (pendulum_collect_kernels.hip): one
// workgroup carries ROLLOUT_ROWS instances through all `steps` iterations of
// behaviour action -> transition / lockstep autoreset -> ring write.
#define COLLECT_NOISED 0   // actor forward + clipped Gaussian noise
#define COLLECT_UNIFORM 1  // uniform in [low, high]; no net is read
// dims[0] == 3 (obs), dims[L] == 1 (torque); n_layers == 0 in uniform mode
struct PendulumCollectArgs : NetArgs {
  double* state;           // [N, 2] env carry (read unless start_with_reset)
  ReplayRing ring;
  float* seg_returns;      // [N, n_segs] per-row segment reward sums
  float* last_obs;         // [N, 3] observation of the carry after the epoch
  const unsigned long long* ctr;  // device RNG counter (read once)
  int cut_step[ROLLOUT_MAX_CUTS];  // ascending
  int n_cuts, n_segs;
  int N, steps;
  int start_with_reset;
  int mode;                // COLLECT_NOISED | COLLECT_UNIFORM
  float noise_scale, limit;  // noised mode
  float low, high;           // uniform mode
  uint64_t action_seed, env_seed;
};

// persistent replay collection on the synthetic envs
// (synthetic_collect_kernels.hip): one workgroup carries ROLLOUT_ROWS rows
// through all `steps` iterations of behaviour action -> synthetic transition
// / lockstep autoreset -> ring write.  dims[0] == O, dims[L] == A;
// n_layers == 0 in uniform mode.  O == ring.O, A == ring.A.
struct SyntheticCollectArgs : NetArgs {
  const float* envA;       // [O, O]
  const float* envB;       // [A, O]
  const float* envw;       // [O]
  float* carry;            // [N, O] live state (read unless start_with_reset)
  ReplayRing ring;
  float* seg_returns;      // [N, n_segs] per-row segment reward sums
  const unsigned long long* ctr;  // device RNG counter (read once)
  int cut_step[ROLLOUT_MAX_CUTS];  // ascending
  int n_cuts, n_segs;
  int N, O, A, steps;
  int start_with_reset;
  int mode;                // COLLECT_NOISED | COLLECT_UNIFORM
  float noise_scale, limit;  // noised mode
  float low, high;           // uniform mode
  float sigma;               // env dynamics noise
  uint64_t action_seed, env_seed;
};

// its LDS floats: 2 state tiles (step ping-pong) + 2 activation tiles + 1
// action tile and the net, then env A/B/w.  The launcher, the binding's
// budget check and the Python gate all size from here.
__host__ __device__ inline long synthetic_collect_lds_floats(const int* dims,
                                                             int n_layers, int O,
                                                             int A) {
  return net_lds_floats(5, dims, n_layers) + O * O + A * O + O;
}

// persistent policy evaluation (eval_kernels.hip): one workgroup carries
// ROLLOUT_ROWS episodes from their init draw to their end and writes only
// the per-episode return, length and init state.
#define EVAL_DETERMINISTIC 0  // action = the net's output (DeterministicPolicy)
#define EVAL_GAUSSIAN 1       // action = mean + exp(log_std) * z
struct PendulumEvalArgs : NetArgs {  // dims[0] == 3 (obs), dims[L] == 1 (torque)
  const float* log_std;    // [1]; Gaussian mode only
  double* returns;         // [N] fp32 step rewards summed in step order
  int* lengths;            // [N] == horizon
  double* init_state;      // [N, 2]
  const unsigned long long* ctr;        // action-stream counter (read once)
  const unsigned long long* reset_ctr;  // init-draw counter (read once)
  int N, horizon;
  int mode;                // EVAL_DETERMINISTIC | EVAL_GAUSSIAN
  uint64_t policy_seed, env_seed;
};

struct CartPoleEvalArgs : NetArgs {  // dims[0] == 4 (obs), dims[L] == n_act
  double* returns;         // [N] == length (reward 1 per step)
  int* lengths;            // [N] in [1, horizon]
  double* init_state;      // [N, 4]
  const unsigned long long* ctr;        // action-stream counter (read once)
  const unsigned long long* reset_ctr;  // init-draw counter (read once)
  int N, horizon;
  uint64_t policy_seed, env_seed;
};

// one pass over a PPO epoch's rows (ppo_ingest_kernels.hip): a workgroup owns
// ROLLOUT_ROWS of the T step rows + E bootstrap rows, runs the value net, the
// current policy and the old policy on its LDS tile and copies the epoch's
// tensors into the update graph's capture-stable buffers.  Narrow nets only.
struct PPOIngestArgs {
  NetArgs val, pol, old;     // old has the shape of pol
  const float* obs;          // [T, O]
  const float* last_obs;     // [E, O]
  const float* actions;      // [T, A]
  const float* rewards;      // [T]
  const int* offsets;        // [E + 1]
  const int* dones;          // [E]
  const float* log_std;      // [A] of pol
  const float* old_log_std;  // [A] of old
  float* obs_out;            // [T, O]
  float* act_out;            // [T, A]
  float* rew_out;            // [T]
  int* off_out;              // [E + 1]
  int* dones_out;            // [E]
  float* values_all;         // [T + E]
  float* old_logp;           // [T]
  float* logp_now;           // [T]
  int T, E, O, A;
};

// its LDS floats: the row tile + 2 activation tiles, three net images and
// the two sigma tables
__host__ __device__ inline long ppo_ingest_lds_floats(const int* vdims, int vl,
                                                      const int* pdims, int pl) {
  return net_lds_floats(3, vdims, vl) + 2 * net_lds_floats(0, pdims, pl) +
         2 * pdims[pl];
}

// the tail of the captured PPO epoch (ppo_epoch_epilogue, update_kernels.hip):
// the flushed KL's gate bookkeeping, both optimizers' step bumps, the deferred
// value-loss rows and the old-policy sync, then the gate left open again
struct PPOEpilogueArgs {
  float* gate;               // left at 1 for the next replay
  const float* kl;           // the last executed iteration's pending KL
  float* kl_final;
  float* iters_done;         // left at 0 for the next replay
  float* iters_out;          // the executed-update count, for the host
  float thr;
  float* pol_step[MT_MAX_TENSORS];  // += executed-update count
  float* val_step[MT_MAX_TENSORS];  // += val_bump
  int n_pol_steps, n_val_steps;
  float val_bump;
  const float* partials;     // [rows][row_stride], fb used per row
  float* losses;             // [rows]
  int rows, fb, row_stride;
  const float* src[MT_MAX_TENSORS];  // policy parameters ...
  float* dst[MT_MAX_TENSORS];        // ... copied to the old policy's
  int numel[MT_MAX_TENSORS];
  int n_sync;
};

// the multi-kernel body's ring write (offpolicy_kernels.hip): the buffers
// of steps x (action -> env step) into the same slots; O = ring.O, A = ring.A
struct ReplayScatterArgs {
  const float* obs_full;   // [steps + 1, N, O]
  const float* act_buf;    // [steps, N, A]
  const float* rew_buf;    // [steps, N]
  const float* cut_final;  // [n_cuts, N, O]
  const int* cut_slot;     // [steps]: index into cut_final, -1 off the cuts
  ReplayRing ring;
  float* seg_returns;      // [N, n_segs]
  int N, steps, n_cuts, n_segs;
};

// replay-ring minibatch gather (offpolicy_kernels.hip / bindings.hip)
struct ReplayGatherArgs {
  const float* obs;   // [cap, O] ring storage
  const float* act;   // [cap, A]
  const float* rew;   // [cap]
  const float* nxt;   // [cap, O]
  const float* dn;    // [cap]
  const long long* size;  // device scalar: current ring fill
  float* qin;      // [B, O+A]  critic input (obs|act)
  float* obs_out;  // [B, O]    actor input
  float* nxt_out;  // [B, O]
  float* rew_out;  // [B]
  float* dn_out;   // [B]
  int B, O, A;
  uint64_t seed, offset;
  const unsigned long long* offset_ptr;  // optional device RNG counter
};
