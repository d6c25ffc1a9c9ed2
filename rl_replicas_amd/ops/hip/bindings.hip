// PyTorch bindings for the rl_replicas_amd HIP/CDNA4 kernels.
//
// Built in-tree as rl_replicas_amd/_hip_ops*.so (setup.py,
// PYTORCH_ROCM_ARCH=gfx950).  All entry points run on the current
// torch HIP stream and validate device/dtype/contiguity up front so a
// misuse fails loudly instead of silently falling back.
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"

// kernel declarations (defined in the .hip translation units)
void launch_mlp_fwd(const MLPArgs& args, const float* x, int save_hidden,
                    int rows, int n_blocks, size_t lds_bytes, int compute_bf16,
                    hipStream_t stream);
void launch_mlp_bwd_layer(const float* dy, const float* y, const float* xin,
                          const float* W, float* dx, float* ws, long ws_stride,
                          int batch, int out_d, int in_d, int act, int rows,
                          int n_blocks, size_t lds_bytes, hipStream_t stream);
void launch_mlp_bwd_fused(const MLPBwdArgs& args, const float* x,
                          const float* dy, float* dx, float* ws,
                          const float* mse_returns, float* loss_partials,
                          size_t lds_bytes, int n_blocks, int compute_bf16,
                          hipStream_t stream, int do_fwd = 0,
                          GaussSeedArgs gargs = GaussSeedArgs{},
                          int need_dx = 1);
__global__ void mlp_grad_reduce_onepass_f32(ReduceAllArgs a);
void launch_mlp_grad_reduce_adam(const ReduceAdamArgs& a, long grand,
                                 hipStream_t stream);
void launch_mlp_bwd_fused_twin(const MLPBwdTwinArgs& a, size_t lds_bytes,
                               int n_blocks, hipStream_t stream);
void launch_mlp_bwd_fused_twin_shaped(const MLPBwdTwinArgs& a, int n_blocks,
                                      hipStream_t stream);
size_t mlp_bwd_fused_shaped_lds(int in_d);
bool mlp_reduce_adam_is_staged(int n_blocks, long grand);
void launch_mlp_grad_reduce_adam_twin(const ReduceAdamArgs& pol, long grand_pol,
                                      const ReduceAdamArgs& val, long grand_val,
                                      hipStream_t stream);
void launch_mlp_layer_fwd_wide(const float* x, const float* W, const float* B,
                               float* out, int batch, int in_d, int out_d,
                               int act, hipStream_t stream);
void launch_mlp_bwd_wide(const float* dy, const float* y, const float* xin,
                         const float* W, float* dx, float* ws, long ws_stride,
                         int batch, int out_d, int in_d, int act,
                         hipStream_t stream);
void launch_mlp_dgrad_wide(const float* dy, const float* y, const float* W,
                           float* dx, int batch, int out_d, int in_d, int act,
                           hipStream_t stream);
void launch_gaussian_loss(const float* mean, const float* actions,
                          const float* old_logp, const float* adv,
                          const float* log_std, float* dmean, float* c_buf,
                          float* partials, int B, int D, float clip, int mode,
                          int n_blocks, hipStream_t stream);
__global__ void loss_partials_finalize(const float* partials, float* dlog_std,
                                       float* scalars, int n_blocks, int D);
__global__ void gaussian_logp_kernel(const float* mean, const float* actions,
                                     const float* log_std, float* logp, int B,
                                     int D);
__global__ void gaussian_kl_kernel(const float* mean, const float* actions,
                                   const float* log_std, const float* old_logp,
                                   float* out, int B, int D);
__global__ void categorical_policy_loss_bwd(const float* logits,
                                            const float* actions,
                                            const float* old_logp,
                                            const float* adv, float* dlogits,
                                            float* partials, int B, int N,
                                            float clip, int mode);
__global__ void categorical_logp_kernel(const float* logits, const float* actions,
                                        float* logp, int B, int N);
__global__ void categorical_kl_kernel(const float* logits, const float* actions,
                                      const float* old_logp, float* out, int B,
                                      int N);
__global__ void value_loss_finalize_rows(const float* partials, float* scalars,
                                         int rows, int fb, int row_stride);
__global__ void value_mse_bwd_kernel(const float* v, const float* ret, float* dv,
                                     float* scalars, int B);
__global__ void gaussian_sample_kernel(const float* mean, const float* log_std,
                                       float* out, int B, int D, uint64_t seed,
                                       uint64_t offset, float noise_scale,
                                       float limit,
                                       const unsigned long long* offset_ptr);
__global__ void categorical_sample_kernel(const float* logits, int64_t* out,
                                          int B, int N, uint64_t seed,
                                          uint64_t offset,
                                          const unsigned long long* offset_ptr);
__global__ void cartpole_env_step_kernel(double* state, int* elapsed,
                                         const int64_t* actions, float* obs,
                                         float* final_obs, float* reward,
                                         uint8_t* done, int N, int max_steps,
                                         uint64_t seed, uint64_t offset,
                                         const unsigned long long* offset_ptr);
__global__ void cartpole_env_reset_kernel(double* state, int* elapsed, float* obs,
                                          int N, uint64_t seed, uint64_t offset,
                                          const unsigned long long* offset_ptr);
void launch_cartpole_rollout_fused(const CartPoleRolloutArgs& a, hipStream_t stream);
__global__ void pendulum_env_step_kernel(double* state, const float* actions,
                                         float* obs, float* final_obs,
                                         float* reward, int N, int do_reset,
                                         uint64_t seed, uint64_t offset,
                                         const unsigned long long* offset_ptr);
__global__ void pendulum_env_reset_kernel(double* state, float* obs, int N,
                                          int draw, uint64_t seed, uint64_t offset,
                                          const unsigned long long* offset_ptr);
void launch_pendulum_rollout_fused(const PendulumRolloutArgs& a, hipStream_t stream);
void launch_synthetic_collect_fused(const SyntheticCollectArgs& a, int wide_threads,
                                    hipStream_t stream);
void launch_pendulum_collect_fused(const PendulumCollectArgs& a, int wide_threads,
                                   hipStream_t stream);
void launch_pendulum_eval_fused(const PendulumEvalArgs& a, int wide_threads,
                                hipStream_t stream);
void launch_cartpole_eval_fused(const CartPoleEvalArgs& a, hipStream_t stream);
__global__ void episode_reduce_kernel(const float* rew_buf,
                                      const unsigned char* done_buf, double* returns,
                                      int* lengths, int N, int steps);
__global__ void uniform_sample_kernel(float* out, int total, float low, float high,
                                      uint64_t seed, uint64_t offset,
                                      const unsigned long long* offset_ptr);
__global__ void replay_scatter_kernel(ReplayScatterArgs a);
__global__ void ring_advance_kernel(long long* write, long long* size,
                                    unsigned long long n, unsigned long long cap);
__global__ void synthetic_env_step_kernel(const float* state, const float* actions,
                                          const float* A, const float* Bm,
                                          const float* w, float* s_out,
                                          float* final_out, float* reward, int N,
                                          int O, int Adim, float sigma,
                                          uint64_t seed, uint64_t offset,
                                          int do_reset,
                                          const unsigned long long* offset_ptr);
__global__ void synthetic_env_reset_kernel(float* s_out, int total,
                                           uint64_t seed, uint64_t offset,
                                           const unsigned long long* offset_ptr);
__global__ void counter_add_kernel(unsigned long long* ctr,
                                   unsigned long long delta);
void launch_ppo_rollout_fused(const RolloutFusedArgs& a, hipStream_t stream);
void launch_ppo_ingest_rows(const PPOIngestArgs& a, hipStream_t stream);
__global__ void ppo_epoch_epilogue(PPOEpilogueArgs a);
__global__ void segmented_gae_kernel(const float* rewards, const float* values,
                                     const float* last_values, const int* offsets,
                                     const int* dones, float* advantages,
                                     float* returns, float gamma, float lam);
__global__ void normalize_kernel(const float* x, float* y, int n);
__global__ void q_target_kernel(const float* r, const float* d, const float* qn,
                                float* out, float gamma, int n);
__global__ void td3_smooth_kernel(const float* a, float* out, int total,
                                  uint64_t seed, uint64_t offset, float scale,
                                  float clip, float limit,
                                  const unsigned long long* offset_ptr);
__global__ void q_target_min2_kernel(const float* r, const float* d,
                                     const float* q1, const float* q2,
                                     float* out, float gamma, int n);
__global__ void replay_gather_kernel(ReplayGatherArgs a);

__global__ void fused_adam_kernel(AdamArgs a);
__global__ void adam_step_bump_kernel(AdamArgs a);
__global__ void fused_polyak_kernel(PolyakArgs a);
__global__ void ppo_gate_update_kernel(float* gate, const float* kl,
                                       float* kl_final, float* iters_done,
                                       float thr);

namespace {

hipStream_t current_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_f32_gpu(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

#define HIP_OK(expr)                                                        \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ", hipGetErrorString(_e));    \
  } while (0)

// Backward tiles stay at 32 rows: 16-row tiles made stage-1 faster but
// DOUBLED the partial-row count, pushing the (latency-bound) reduce
// from 10.3 to 17.8 us — a measured net loss.  (The FORWARD still uses
// 16-row tiles below 8K rows; its cost has no reduce to pay.)
constexpr int BWD_FUSED_ROWS = 32;

// The one validated description of a net handed to a binding: layer widths
// and the flat layout of its gradient partials — the layers' (od*id + od)
// segments in layer order.  whole_w = floats of the padded whole-net LDS
// weight image ([out][in + 1] per layer).
struct NetLayout {
  int L = 0;
  int dims[MLP_MAX_LAYERS + 1] = {};
  int64_t totals[MLP_MAX_LAYERS] = {};
  int64_t layer_off[MLP_MAX_LAYERS] = {};
  int64_t grand = 0;
  size_t whole_w = 0;
  int max_width = 0;
};

// dims = [in, hidden..., out]; `reserve` keeps that many of the fixed
// argument-block slots free (the policy path's log_std pseudo-layer)
NetLayout net_layout(const std::vector<int64_t>& dims, int width_cap,
                     int reserve = 0) {
  NetLayout n;
  n.L = (int)dims.size() - 1;
  TORCH_CHECK(n.L >= 1 && n.L + reserve <= MLP_MAX_LAYERS,
              "unsupported layer count ", n.L, " (at most ",
              MLP_MAX_LAYERS - reserve, ")");
  for (int l = 0; l <= n.L; ++l) {
    TORCH_CHECK(dims[l] >= 1 && dims[l] <= width_cap, "layer width ", dims[l],
                " outside [1, ", width_cap, "]");
    n.dims[l] = (int)dims[l];
    n.max_width = std::max(n.max_width, n.dims[l]);
  }
  for (int l = 0; l < n.L; ++l) {
    n.totals[l] = (int64_t)n.dims[l + 1] * n.dims[l] + n.dims[l + 1];
    n.layer_off[l] = n.grand;
    n.grand += n.totals[l];
    n.whole_w += (size_t)n.dims[l + 1] * (n.dims[l] + 1);
  }
  return n;
}

// every check a binding makes of (input width, weights, biases, acts)
NetLayout net_layout(int64_t in_dim, const std::vector<torch::Tensor>& weights,
                     const std::vector<torch::Tensor>& biases,
                     const std::vector<int64_t>& acts, int width_cap,
                     int reserve = 0) {
  TORCH_CHECK(biases.size() == weights.size() && acts.size() == weights.size(),
              "weights/biases/acts length mismatch");
  std::vector<int64_t> dims{in_dim};
  for (size_t l = 0; l < weights.size(); ++l) {
    check_f32_gpu(weights[l], "weight");
    check_f32_gpu(biases[l], "bias");
    TORCH_CHECK(weights[l].dim() == 2 && weights[l].size(1) == dims[l],
                "weight shape mismatch at layer ", l);
    TORCH_CHECK(biases[l].numel() == weights[l].size(0),
                "bias shape mismatch at layer ", l);
    dims.push_back(weights[l].size(0));
  }
  return net_layout(dims, width_cap, reserve);
}

NetLayout net_layout(const torch::Tensor& x,
                     const std::vector<torch::Tensor>& weights,
                     const std::vector<torch::Tensor>& biases,
                     const std::vector<int64_t>& acts, int width_cap,
                     int reserve = 0) {
  check_f32_gpu(x, "x");
  TORCH_CHECK(x.dim() == 2, "x must be 2-D");
  return net_layout(x.size(1), weights, biases, acts, width_cap, reserve);
}

// the w/b/dims/acts/n_layers fields every net-carrying argument block has
template <class Args>
void fill_net(Args& a, const NetLayout& n,
              const std::vector<torch::Tensor>& weights,
              const std::vector<torch::Tensor>& biases,
              const std::vector<int64_t>& acts) {
  a.n_layers = n.L;
  a.dims[0] = n.dims[0];
  for (int l = 0; l < n.L; ++l) {
    a.w[l] = weights[l].data_ptr<float>();
    a.b[l] = biases[l].data_ptr<float>();
    a.dims[l + 1] = n.dims[l + 1];
    a.acts[l] = (int)acts[l];
  }
}

// saved activations of a backward: hidden[l] is layer l's output
// [batch, dims[l + 1]] for l < L - 1, final_out the last layer's
void check_saved(const NetLayout& n, int64_t batch,
                 const std::vector<torch::Tensor>& hidden,
                 const torch::Tensor& final_out) {
  TORCH_CHECK((int)hidden.size() == n.L - 1, "hidden must hold ", n.L - 1,
              " activations, got ", hidden.size());
  for (int l = 0; l < n.L; ++l) {
    const torch::Tensor& h = l == n.L - 1 ? final_out : hidden[l];
    check_f32_gpu(h, "saved activation");
    TORCH_CHECK(h.numel() == batch * n.dims[l + 1],
                "saved activation shape mismatch at layer ", l);
  }
}

// Adam state of one net for the merged reduce+Adam kernels: m/v ordered
// [weights..., biases...], shaped like the parameters
void check_adam_state(const std::vector<torch::Tensor>& weights,
                      const std::vector<torch::Tensor>& biases,
                      const std::vector<torch::Tensor>& m,
                      const std::vector<torch::Tensor>& v,
                      const torch::Tensor& step) {
  const size_t L = weights.size();
  TORCH_CHECK(m.size() == 2 * L && v.size() == 2 * L,
              "adam m/v must be [weights..., biases...] (2L tensors)");
  for (size_t i = 0; i < 2 * L; ++i) {
    const torch::Tensor& p = i < L ? weights[i] : biases[i - L];
    check_f32_gpu(m[i], "adam m");
    check_f32_gpu(v[i], "adam v");
    TORCH_CHECK(m[i].numel() == p.numel() && v[i].numel() == p.numel(),
                "adam state shape mismatch");
  }
  TORCH_CHECK(step.is_cuda() && step.scalar_type() == torch::kFloat32 &&
                  step.numel() == 1,
              "adam step must be a 1-element fp32 GPU tensor");
}

// dynamic LDS of the narrow forward (activation ping-pong) and per-layer
// backward (dZ + x) kernels: two row tiles + a padded weight image
size_t two_tile_lds(int rows, size_t image_floats) {
  return ((size_t)2 * rows * (MLP_NARROW_WIDTH + 4) + image_floats) * 4;
}

// dynamic LDS of the whole-net fused backward: 3 tiles (dZ ping-pong + x),
// plus one activation tile per layer when the forward runs in the kernel
size_t fused_bwd_lds(const NetLayout& n, bool fwd_in_kernel) {
  const size_t act_tiles = (size_t)(fwd_in_kernel ? 3 + n.L : 3);
  return (act_tiles * BWD_FUSED_ROWS * (MLP_NARROW_WIDTH + 4) + n.whole_w) * 4;
}

// whether the whole-net fused backward takes this net — the gate of
// mlp_backward, the check of the bindings that have no other kernel, and
// what fused_bwd_fits tells Python
bool fused_bwd_fits(const NetLayout& n, bool fwd_in_kernel) {
  return n.max_width <= MLP_NARROW_WIDTH &&
         fused_bwd_lds(n, fwd_in_kernel) <= MLP_LDS_BUDGET;
}

// whole-net fused-backward argument block with h[] unset (the in-kernel
// forward keeps activations in LDS); ws_stride = flat elems per partial row
MLPBwdArgs fill_bwd_args(const torch::Tensor& x,
                         const std::vector<torch::Tensor>& weights,
                         const std::vector<torch::Tensor>& biases,
                         const std::vector<int64_t>& acts,
                         const NetLayout& n, int64_t ws_stride) {
  MLPBwdArgs ba{};
  fill_net(ba, n, weights, biases, acts);
  ba.batch = (int)x.size(0);
  ba.ws_stride = ws_stride;
  for (int l = 0; l < n.L; ++l) ba.layer_off[l] = (int)n.layer_off[l];
  return ba;
}

// ... and with the saved activations of a separate forward
void set_saved(MLPBwdArgs& ba, const NetLayout& n,
               const std::vector<torch::Tensor>& hidden,
               const torch::Tensor& final_out) {
  for (int l = 0; l < n.L; ++l)
    ba.h[l] = (l == n.L - 1 ? final_out : hidden[l]).data_ptr<float>();
}

// gradient tensors of a backward and its [dx, dW..., db...] result
struct GradOut {
  std::vector<torch::Tensor> dws, dbs;
  GradOut(const NetLayout& n, const torch::TensorOptions& opts) {
    for (int l = 0; l < n.L; ++l) {
      dws.push_back(torch::empty({n.dims[l + 1], n.dims[l]}, opts));
      dbs.push_back(torch::empty({n.dims[l + 1]}, opts));
    }
  }
  std::vector<torch::Tensor> pack(const torch::Tensor& dx) const {
    std::vector<torch::Tensor> out{dx};
    out.insert(out.end(), dws.begin(), dws.end());
    out.insert(out.end(), dbs.begin(), dbs.end());
    return out;
  }
};

// one-pass deterministic reduction of the partial rows ws[n_blocks][grand]
// into the gradient tensors
void launch_reduce_all(const NetLayout& n, const float* ws, int n_blocks,
                       const GradOut& g, hipStream_t stream) {
  ReduceAllArgs ra{};
  ra.ws = ws;
  ra.stride = n.grand;
  ra.n_layers = n.L;
  ra.n_blocks = n_blocks;
  for (int l = 0; l < n.L; ++l) {
    ra.dw[l] = g.dws[l].data_ptr<float>();
    ra.db[l] = g.dbs[l].data_ptr<float>();
    ra.total[l] = (int)n.totals[l];
    ra.wsize[l] = n.dims[l + 1] * n.dims[l];
  }
  const int rb = (int)std::min<int64_t>(256, (n.grand + 63) / 64);
  hipLaunchKernelGGL(mlp_grad_reduce_onepass_f32, dim3(rb), dim3(256), 0,
                     stream, ra);
  HIP_OK(hipGetLastError());
}

// argument block of the merged reduce+Adam kernels for one net (m/v as
// check_adam_state admits them)
ReduceAdamArgs fill_reduce_adam(const std::vector<torch::Tensor>& weights,
                                const std::vector<torch::Tensor>& biases,
                                const NetLayout& n, const float* ws,
                                long stride, int n_blocks,
                                const std::vector<torch::Tensor>& m,
                                const std::vector<torch::Tensor>& v,
                                const torch::Tensor& step, double lr,
                                double beta1, double beta2, double eps,
                                double weight_decay, double step_delta,
                                const c10::optional<torch::Tensor>& gate) {
  const int L = n.L;
  ReduceAdamArgs ra{};
  ra.ws = ws;
  ra.stride = stride;
  ra.n_layers = L;
  ra.n_blocks = n_blocks;
  for (int l = 0; l < L; ++l) {
    ra.pw[l] = weights[l].data_ptr<float>();
    ra.pb[l] = biases[l].data_ptr<float>();
    ra.mw[l] = m[l].data_ptr<float>();
    ra.mb[l] = m[L + l].data_ptr<float>();
    ra.vw[l] = v[l].data_ptr<float>();
    ra.vb[l] = v[L + l].data_ptr<float>();
    ra.total[l] = (int)n.totals[l];
    ra.wsize[l] = n.dims[l + 1] * n.dims[l];
  }
  ra.step = step.data_ptr<float>();
  ra.lr = (float)lr;
  ra.beta1 = (float)beta1;
  ra.beta2 = (float)beta2;
  ra.eps = (float)eps;
  ra.weight_decay = (float)weight_decay;
  ra.step_delta = (float)step_delta;
  ra.gate = gate.has_value() ? gate->data_ptr<float>() : nullptr;
  return ra;
}

// merged reduce+Adam launch (optional fast path of mlp_backward /
// value_mlp_backward)
void launch_reduce_adam(const std::vector<torch::Tensor>& weights,
                        const std::vector<torch::Tensor>& biases,
                        const NetLayout& n, const float* ws, int n_blocks,
                        const std::vector<torch::Tensor>& m,
                        const std::vector<torch::Tensor>& v,
                        const torch::Tensor& step, double lr, double beta1,
                        double beta2, double eps, double weight_decay,
                        double step_delta,
                        const c10::optional<torch::Tensor>& gate,
                        hipStream_t stream) {
  const ReduceAdamArgs ra =
      fill_reduce_adam(weights, biases, n, ws, n.grand, n_blocks, m, v, step,
                       lr, beta1, beta2, eps, weight_decay, step_delta, gate);
  launch_mlp_grad_reduce_adam(ra, (long)n.grand, stream);
  HIP_OK(hipGetLastError());
}

// RL_REPLICAS_AMD_MLP_ROWS=16|32|64 (read once): forward row tile override
int env_mlp_rows() {
  static int env_rows = []() {
    const char* e = getenv("RL_REPLICAS_AMD_MLP_ROWS");
    const int r = e ? atoi(e) : 0;
    return (r == 16 || r == 32 || r == 64) ? r : 0;
  }();
  return env_rows;
}

// Row tile of the whole-net forward (narrow nets): 16 rows up to 8K rows
// (4000-row rollout -> 250 WGs; measured +2.4% over 32-row on the PPO
// bench — latency hiding beats weight-staging amortization until the chip
// is well past full), 32 beyond.  The override is ignored where its image
// would not fit the budget (64 rows on a five-layer 64-wide net); the
// default tile fits every net net_layout admits at MLP_NARROW_WIDTH.
int fwd_rows(int batch, size_t whole_w) {
  const int env_rows = env_mlp_rows();
  if (env_rows != 0 && two_tile_lds(env_rows, whole_w) <= MLP_LDS_BUDGET)
    return env_rows;
  return batch < 8192 ? 16 : 32;
}

// Row tile of the per-layer backward (instantiated at 32 and 64; its
// single-layer image always fits).  Wide nets: the 2D-grid kernels' 32.
int bwd_layer_rows(bool wide) {
  return (!wide && env_mlp_rows() == 64) ? 64 : 32;
}

}  // namespace

// ---------------------------------------------------------------------------
// fused MLP
// ---------------------------------------------------------------------------
std::vector<torch::Tensor> mlp_forward(torch::Tensor x,
                                       std::vector<torch::Tensor> weights,
                                       std::vector<torch::Tensor> biases,
                                       std::vector<int64_t> acts,
                                       bool save_hidden,
                                       int64_t compute_bf16) {
  const NetLayout net = net_layout(x, weights, biases, acts, MLP_MAX_WIDTH);
  const int L = net.L;
  // per-layer column-split kernels for wide nets at ANY batch: a whole-net
  // 256-wide kernel was measured SLOWER at minibatch scale (batch 100 ->
  // 4 WGs serializing 3 layers each, 800 vs 1232 env-steps/s on the TD3
  // bench) — concurrency across independent per-layer launches beats
  // fewer launches here
  const bool wide = net.max_width > MLP_NARROW_WIDTH;
  const int batch = (int)x.size(0);
  const int rows = fwd_rows(batch, net.whole_w);
  const size_t lds_bytes = two_tile_lds(rows, net.whole_w);
  TORCH_CHECK(wide || lds_bytes <= MLP_LDS_BUDGET,
              "net image exceeds the LDS budget");

  MLPArgs args{};
  fill_net(args, net, weights, biases, acts);
  args.batch = batch;

  auto opts = x.options();
  std::vector<torch::Tensor> outs;  // [final, h0..h_{L-2}]
  torch::Tensor final_out = torch::empty({x.size(0), net.dims[L]}, opts);
  outs.push_back(final_out);
  std::vector<torch::Tensor> inter;  // wide path needs intermediates always
  for (int l = 0; l < L - 1; ++l) {
    if (save_hidden || wide) {
      torch::Tensor h = torch::empty({x.size(0), net.dims[l + 1]}, opts);
      args.h[l] = h.data_ptr<float>();
      if (save_hidden) outs.push_back(h);
      else inter.push_back(h);
    } else {
      args.h[l] = nullptr;
    }
  }
  args.h[L - 1] = final_out.data_ptr<float>();

  if (batch > 0) {
    auto stream = current_stream();
    if (wide) {
      // per-layer 2D-grid kernels: column groups spread across blocks
      const float* cur = x.data_ptr<float>();
      for (int l = 0; l < L; ++l) {
        launch_mlp_layer_fwd_wide(cur, args.w[l], args.b[l], args.h[l], batch,
                                  args.dims[l], args.dims[l + 1], args.acts[l],
                                  stream);
        HIP_OK(hipGetLastError());
        cur = args.h[l];
      }
    } else {
      launch_mlp_fwd(args, x.data_ptr<float>(), save_hidden ? 1 : 0, rows,
                     (batch + rows - 1) / rows, lds_bytes, (int)compute_bf16,
                     stream);
      HIP_OK(hipGetLastError());
    }
  }
  return outs;
}

std::vector<torch::Tensor> mlp_backward(torch::Tensor grad_out, torch::Tensor x,
                                        std::vector<torch::Tensor> weights,
                                        std::vector<torch::Tensor> biases,
                                        std::vector<torch::Tensor> hidden,
                                        torch::Tensor final_out,
                                        std::vector<int64_t> acts,
                                        int64_t compute_bf16,
                                        c10::optional<std::vector<torch::Tensor>> adam_m,
                                        c10::optional<std::vector<torch::Tensor>> adam_v,
                                        c10::optional<torch::Tensor> adam_step,
                                        double lr, double beta1, double beta2,
                                        double eps, double weight_decay,
                                        double adam_step_delta,
                                        c10::optional<torch::Tensor> adam_gate,
                                        bool input_grad_only) {
  const bool fuse_adam = adam_m.has_value();
  const NetLayout net = net_layout(x, weights, biases, acts, MLP_MAX_WIDTH);
  const int L = net.L;
  const int batch = (int)x.size(0);
  check_f32_gpu(grad_out, "grad_out");
  TORCH_CHECK(grad_out.numel() == (int64_t)batch * net.dims[L],
              "grad_out shape mismatch");
  check_saved(net, batch, hidden, final_out);
  if (fuse_adam) {
    TORCH_CHECK(adam_v.has_value() && adam_step.has_value(),
                "adam_m needs adam_v and adam_step");
    check_adam_state(weights, biases, *adam_m, *adam_v, *adam_step);
  }
  auto opts = x.options();
  auto stream = current_stream();
  const int64_t grand = net.grand;
  // weight gradients: consumed on device (fused Adam), not wanted at all
  // (input_grad_only), or reduced into fresh tensors
  auto finish = [&](const torch::Tensor& dx, const torch::Tensor& ws,
                    int n_blocks) -> std::vector<torch::Tensor> {
    if (input_grad_only) return {dx};
    if (fuse_adam) {
      launch_reduce_adam(weights, biases, net, ws.data_ptr<float>(), n_blocks,
                         *adam_m, *adam_v, *adam_step, lr, beta1, beta2, eps,
                         weight_decay, adam_step_delta, adam_gate, stream);
      return {dx};
    }
    const GradOut g(net, opts);
    launch_reduce_all(net, ws.data_ptr<float>(), n_blocks, g, stream);
    return g.pack(dx);
  };

  // one workspace: [block][concatenated layer elems] (layer-blind stage-1).
  // Whole-net fused backward for narrow nets when the LDS image fits
  if (fused_bwd_fits(net, false)) {
    const int fb = (batch + BWD_FUSED_ROWS - 1) / BWD_FUSED_ROWS;
    torch::Tensor ws = torch::empty({(int64_t)fb, grand}, opts);
    MLPBwdArgs ba = fill_bwd_args(x, weights, biases, acts, net, grand);
    set_saved(ba, net, hidden, final_out);
    torch::Tensor dx = torch::empty({batch, x.size(1)}, opts);
    launch_mlp_bwd_fused(ba, x.data_ptr<float>(), grad_out.data_ptr<float>(),
                         dx.data_ptr<float>(), ws.data_ptr<float>(), nullptr,
                         nullptr, fused_bwd_lds(net, false), fb,
                         (int)compute_bf16, stream);
    HIP_OK(hipGetLastError());
    return finish(dx, ws, fb);
  }

  const bool wide = net.max_width > MLP_NARROW_WIDTH;
  const int rows = bwd_layer_rows(wide);
  const int n_blocks = (batch + rows - 1) / rows;
  torch::Tensor ws = torch::empty({(int64_t)n_blocks, grand}, opts);
  float* ws_ptr = ws.data_ptr<float>();

  torch::Tensor dy = grad_out;
  torch::Tensor dx;
  for (int l = L - 1; l >= 0; --l) {
    const int out_d = net.dims[l + 1];
    const int in_d = net.dims[l];
    torch::Tensor y = (l == L - 1) ? final_out : hidden[l];
    torch::Tensor xin = (l == 0) ? x : hidden[l - 1];
    float* ws_l = ws_ptr + (long)net.layer_off[l] * n_blocks;
    dx = torch::empty({batch, in_d}, opts);
    if (wide) {
      if (input_grad_only) {
        // dgrad chain only (e.g. actor step through a frozen critic:
        // the critic's weight grads would be discarded)
        launch_mlp_dgrad_wide(dy.data_ptr<float>(), y.data_ptr<float>(),
                              weights[l].data_ptr<float>(),
                              dx.data_ptr<float>(), batch, out_d, in_d,
                              (int)acts[l], stream);
      } else {
        // wide layer: 2D-grid dgrad + wgrad kernels
        launch_mlp_bwd_wide(dy.data_ptr<float>(), y.data_ptr<float>(),
                            xin.data_ptr<float>(), weights[l].data_ptr<float>(),
                            dx.data_ptr<float>(), ws_l, grand, batch, out_d,
                            in_d, (int)acts[l], stream);
      }
    } else {
      // merged dgrad + wgrad/bias partials in one kernel: dZ and x tiles
      // plus this layer's padded weight image
      const size_t lds_bytes =
          two_tile_lds(rows, (size_t)out_d * (in_d + 1));
      launch_mlp_bwd_layer(dy.data_ptr<float>(), y.data_ptr<float>(),
                           xin.data_ptr<float>(), weights[l].data_ptr<float>(),
                           dx.data_ptr<float>(), ws_l, grand, batch, out_d,
                           in_d, (int)acts[l], rows, n_blocks, lds_bytes,
                           stream);
    }
    HIP_OK(hipGetLastError());
    dy = dx;
  }
  return finish(dx, ws, n_blocks);
}

// ---------------------------------------------------------------------------
// fused losses (loss_kernels.hip)
// ---------------------------------------------------------------------------
std::vector<torch::Tensor> gaussian_policy_loss(torch::Tensor mean,
                                                torch::Tensor actions,
                                                torch::Tensor old_logp,
                                                torch::Tensor adv,
                                                torch::Tensor log_std,
                                                double clip, int64_t mode) {
  check_f32_gpu(mean, "mean");
  const int B = (int)mean.size(0);
  const int D = (int)mean.size(1);
  TORCH_CHECK(D >= 1 && D <= GAUSS_MAX_D, "action dim must be in [1, ",
              GAUSS_MAX_D, "] for the fused loss");
  auto opts = mean.options();
  auto dmean = torch::empty_like(mean);
  auto dlog_std = torch::empty({D}, opts);
  auto scalars = torch::empty({1}, opts);
  const int n_blocks = std::min(32, (B + 255) / 256);
  auto partials = torch::empty({n_blocks, D + 1}, opts);
  // generic-D kernel scratch (per-row dlogp coefficients)
  auto c_buf = D > 8 ? torch::empty({B}, opts) : torch::Tensor();
  const float* olp = mode == 1 ? old_logp.data_ptr<float>() : nullptr;
  auto stream = current_stream();
  launch_gaussian_loss(mean.data_ptr<float>(), actions.data_ptr<float>(), olp,
                       adv.data_ptr<float>(), log_std.data_ptr<float>(),
                       dmean.data_ptr<float>(),
                       D > 8 ? c_buf.data_ptr<float>() : nullptr,
                       partials.data_ptr<float>(), B,
                       D, (float)clip, (int)mode, n_blocks, stream);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(loss_partials_finalize, dim3(1), dim3(D + 1), 0, stream,
                     partials.data_ptr<float>(), dlog_std.data_ptr<float>(),
                     scalars.data_ptr<float>(), n_blocks, D);
  HIP_OK(hipGetLastError());
  return {dmean, dlog_std, scalars};
}

torch::Tensor gaussian_logp(torch::Tensor mean, torch::Tensor actions,
                            torch::Tensor log_std) {
  check_f32_gpu(mean, "mean");
  const int B = (int)mean.size(0);
  const int D = (int)mean.size(1);
  auto logp = torch::empty({B}, mean.options());
  hipLaunchKernelGGL(gaussian_logp_kernel, dim3(std::min(64, (B + 1023) / 1024)),
                     dim3(1024), 0, current_stream(), mean.data_ptr<float>(),
                     actions.data_ptr<float>(), log_std.data_ptr<float>(),
                     logp.data_ptr<float>(), B, D);
  HIP_OK(hipGetLastError());
  return logp;
}

torch::Tensor gaussian_kl(torch::Tensor mean, torch::Tensor actions,
                          torch::Tensor log_std, torch::Tensor old_logp) {
  check_f32_gpu(mean, "mean");
  const int B = (int)mean.size(0);
  const int D = (int)mean.size(1);
  auto out = torch::empty({1}, mean.options());
  hipLaunchKernelGGL(gaussian_kl_kernel, dim3(1), dim3(1024), 0, current_stream(),
                     mean.data_ptr<float>(), actions.data_ptr<float>(),
                     log_std.data_ptr<float>(), old_logp.data_ptr<float>(),
                     out.data_ptr<float>(), B, D);
  HIP_OK(hipGetLastError());
  return out;
}

std::vector<torch::Tensor> categorical_policy_loss(torch::Tensor logits,
                                                   torch::Tensor actions,
                                                   torch::Tensor old_logp,
                                                   torch::Tensor adv, double clip,
                                                   int64_t mode) {
  check_f32_gpu(logits, "logits");
  const int B = (int)logits.size(0);
  const int N = (int)logits.size(1);
  auto dlogits = torch::empty_like(logits);
  auto scalars = torch::empty({1}, logits.options());
  const int n_blocks = std::min(32, (B + 255) / 256);
  auto partials = torch::empty({n_blocks}, logits.options());
  const float* olp = mode == 1 ? old_logp.data_ptr<float>() : nullptr;
  auto stream = current_stream();
  hipLaunchKernelGGL(categorical_policy_loss_bwd, dim3(n_blocks), dim3(256), 0,
                     stream, logits.data_ptr<float>(),
                     actions.data_ptr<float>(), olp, adv.data_ptr<float>(),
                     dlogits.data_ptr<float>(), partials.data_ptr<float>(), B, N,
                     (float)clip, (int)mode);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(loss_partials_finalize, dim3(1), dim3(1), 0, stream,
                     partials.data_ptr<float>(), nullptr,
                     scalars.data_ptr<float>(), n_blocks, 0);
  HIP_OK(hipGetLastError());
  return {dlogits, scalars};
}

torch::Tensor categorical_logp(torch::Tensor logits, torch::Tensor actions) {
  check_f32_gpu(logits, "logits");
  const int B = (int)logits.size(0);
  const int N = (int)logits.size(1);
  auto logp = torch::empty({B}, logits.options());
  hipLaunchKernelGGL(categorical_logp_kernel, dim3(std::min(64, (B + 1023) / 1024)),
                     dim3(1024), 0, current_stream(), logits.data_ptr<float>(),
                     actions.data_ptr<float>(), logp.data_ptr<float>(), B, N);
  HIP_OK(hipGetLastError());
  return logp;
}

torch::Tensor categorical_kl(torch::Tensor logits, torch::Tensor actions,
                             torch::Tensor old_logp) {
  check_f32_gpu(logits, "logits");
  const int B = (int)logits.size(0);
  const int N = (int)logits.size(1);
  auto out = torch::empty({1}, logits.options());
  hipLaunchKernelGGL(categorical_kl_kernel, dim3(1), dim3(1024), 0,
                     current_stream(), logits.data_ptr<float>(),
                     actions.data_ptr<float>(), old_logp.data_ptr<float>(),
                     out.data_ptr<float>(), B, N);
  HIP_OK(hipGetLastError());
  return out;
}

std::vector<torch::Tensor> value_mse_loss(torch::Tensor v, torch::Tensor ret) {
  check_f32_gpu(v, "v");
  const int B = (int)v.numel();
  auto dv = torch::empty_like(v);
  auto scalars = torch::empty({1}, v.options());
  hipLaunchKernelGGL(value_mse_bwd_kernel, dim3(1), dim3(1024), 0,
                     current_stream(), v.data_ptr<float>(), ret.data_ptr<float>(),
                     dv.data_ptr<float>(), scalars.data_ptr<float>(), B);
  HIP_OK(hipGetLastError());
  return {dv, scalars};
}

// value-function backward with the MSE loss fused into the dZ seed:
// returns [dx, dW..., db..., loss_scalar].  Requires a narrow net with
// identity output (the ValueFunction case); falls back is the caller's
// job (value_supported gates on MLP shape).
std::vector<torch::Tensor> value_mlp_backward(torch::Tensor x,
                                              std::vector<torch::Tensor> weights,
                                              std::vector<torch::Tensor> biases,
                                              std::vector<torch::Tensor> hidden,
                                              torch::Tensor final_out,
                                              std::vector<int64_t> acts,
                                              torch::Tensor returns,
                                              int64_t compute_bf16,
                                              c10::optional<torch::Tensor> partials_out,
                                              c10::optional<std::vector<torch::Tensor>> adam_m,
                                              c10::optional<std::vector<torch::Tensor>> adam_v,
                                              c10::optional<torch::Tensor> adam_step,
                                              double lr, double beta1,
                                              double beta2, double eps,
                                              double weight_decay,
                                              double adam_step_delta,
                                              bool fwd_in_kernel) {
  const bool fuse_adam = adam_m.has_value();
  TORCH_CHECK(!fwd_in_kernel || compute_bf16 == 0,
              "fwd_in_kernel is fp32-only");
  const NetLayout net = net_layout(x, weights, biases, acts, MLP_NARROW_WIDTH);
  const int L = net.L;
  const int batch = (int)x.size(0);
  check_f32_gpu(returns, "returns");
  TORCH_CHECK(returns.numel() == batch, "returns must be [batch]");
  TORCH_CHECK(net.dims[L] == 1 && acts[L - 1] == 0,
              "value_mlp_backward needs a 1-output identity head");
  TORCH_CHECK(fused_bwd_fits(net, fwd_in_kernel),
              "net too large for fused value backward");
  // fwd_in_kernel: activations never exist in HBM — the kernel computes
  // them into LDS (hidden/final_out are ignored)
  if (!fwd_in_kernel) check_saved(net, batch, hidden, final_out);
  if (fuse_adam) {
    TORCH_CHECK(adam_v.has_value() && adam_step.has_value(),
                "adam_m needs adam_v and adam_step");
    check_adam_state(weights, biases, *adam_m, *adam_v, *adam_step);
  }
  const int fb = (batch + BWD_FUSED_ROWS - 1) / BWD_FUSED_ROWS;
  // partials_out: caller-owned slice -> finalize is deferred (the captured
  // value loop batches all iterations' finalizes into one kernel)
  const bool deferred = partials_out.has_value();
  if (deferred) {
    check_f32_gpu(*partials_out, "partials_out");
    TORCH_CHECK(partials_out->numel() >= fb, "partials_out too small");
  }
  auto opts = x.options();
  auto stream = current_stream();

  const int64_t grand = net.grand;
  torch::Tensor ws = torch::empty({(int64_t)fb, grand}, opts);
  torch::Tensor loss_partials = deferred ? *partials_out : torch::empty({fb}, opts);
  torch::Tensor scalars = torch::empty({1}, opts);
  const GradOut g(net, opts);
  MLPBwdArgs ba = fill_bwd_args(x, weights, biases, acts, net, grand);
  if (!fwd_in_kernel) set_saved(ba, net, hidden, final_out);
  // the fused-Adam mode consumes the gradient on device and nobody reads
  // the input gradient: skip computing it and return an empty dx slot
  torch::Tensor dx = fuse_adam ? torch::empty({0}, opts)
                               : torch::empty({batch, x.size(1)}, opts);
  launch_mlp_bwd_fused(ba, x.data_ptr<float>(), nullptr,
                       fuse_adam ? nullptr : dx.data_ptr<float>(),
                       ws.data_ptr<float>(), returns.data_ptr<float>(),
                       loss_partials.data_ptr<float>(),
                       fused_bwd_lds(net, fwd_in_kernel), fb,
                       (int)compute_bf16, stream, fwd_in_kernel ? 1 : 0,
                       GaussSeedArgs{}, fuse_adam ? 0 : 1);
  HIP_OK(hipGetLastError());

  if (fuse_adam) {
    launch_reduce_adam(weights, biases, net, ws.data_ptr<float>(), fb,
                       *adam_m, *adam_v, *adam_step, lr, beta1, beta2, eps,
                       weight_decay, adam_step_delta, c10::nullopt, stream);
  } else {
    launch_reduce_all(net, ws.data_ptr<float>(), fb, g, stream);
  }
  if (!deferred) {
    // loss = sum of the per-block partials (fixed order)
    hipLaunchKernelGGL(loss_partials_finalize, dim3(1), dim3(1), 0, stream,
                       loss_partials.data_ptr<float>(), nullptr,
                       scalars.data_ptr<float>(), fb, 0);
    HIP_OK(hipGetLastError());
  }

  std::vector<torch::Tensor> out = g.pack(dx);
  out.push_back(scalars);
  return out;
}

// ---------------------------------------------------------------------------
// segmented GAE
// ---------------------------------------------------------------------------
// one workgroup of 256 per episode
static void launch_segmented_gae(const float* rewards, const float* values,
                                 const float* last_values, const int* offsets,
                                 const int* dones, float* adv, float* ret, int n_eps,
                                 double gamma, double lam) {
  if (n_eps <= 0) return;
  hipLaunchKernelGGL(segmented_gae_kernel, dim3(n_eps), dim3(256), 0,
                     current_stream(), rewards, values, last_values, offsets, dones,
                     adv, ret, (float)gamma, (float)lam);
  HIP_OK(hipGetLastError());
}

std::vector<torch::Tensor> segmented_gae(torch::Tensor rewards, torch::Tensor values,
                                         torch::Tensor last_values,
                                         torch::Tensor offsets, torch::Tensor dones,
                                         double gamma, double lam) {
  check_f32_gpu(rewards, "rewards");
  check_f32_gpu(values, "values");
  check_f32_gpu(last_values, "last_values");
  TORCH_CHECK(offsets.scalar_type() == torch::kInt32 && offsets.is_cuda());
  TORCH_CHECK(dones.scalar_type() == torch::kInt32 && dones.is_cuda());
  const int n_eps = (int)last_values.size(0);
  auto adv = torch::empty_like(rewards);
  auto ret = torch::empty_like(rewards);
  launch_segmented_gae(rewards.data_ptr<float>(), values.data_ptr<float>(),
                       last_values.data_ptr<float>(), offsets.data_ptr<int>(),
                       dones.data_ptr<int>(), adv.data_ptr<float>(),
                       ret.data_ptr<float>(), n_eps, gamma, lam);
  return {adv, ret};
}

// the same launch into the caller's buffers (the captured PPO epoch):
// values_all = [values (T) | last_values (E)], as one forward leaves them
void segmented_gae_out(torch::Tensor rewards, torch::Tensor values_all,
                       torch::Tensor offsets, torch::Tensor dones, double gamma,
                       double lam, torch::Tensor adv, torch::Tensor ret) {
  check_f32_gpu(rewards, "rewards");
  check_f32_gpu(values_all, "values_all");
  check_f32_gpu(adv, "adv");
  check_f32_gpu(ret, "ret");
  const int64_t T = rewards.numel();
  const int64_t n_eps = values_all.numel() - T;
  TORCH_CHECK(n_eps >= 0 && adv.numel() == T && ret.numel() == T,
              "segmented_gae_out: rewards/adv/ret [T], values_all [T + E]");
  TORCH_CHECK(offsets.scalar_type() == torch::kInt32 && offsets.is_cuda() &&
                  offsets.is_contiguous() && offsets.numel() == n_eps + 1,
              "offsets must be a contiguous int32 GPU tensor [E + 1]");
  TORCH_CHECK(dones.scalar_type() == torch::kInt32 && dones.is_cuda() &&
                  dones.is_contiguous() && dones.numel() == n_eps,
              "dones must be a contiguous int32 GPU tensor [E]");
  launch_segmented_gae(rewards.data_ptr<float>(), values_all.data_ptr<float>(),
                       values_all.data_ptr<float>() + T, offsets.data_ptr<int>(),
                       dones.data_ptr<int>(), adv.data_ptr<float>(),
                       ret.data_ptr<float>(), (int)n_eps, gamma, lam);
}

static void launch_normalize(const torch::Tensor& x, torch::Tensor& y) {
  hipLaunchKernelGGL(normalize_kernel, dim3(1), dim3(1024), 0, current_stream(),
                     x.data_ptr<float>(), y.data_ptr<float>(), (int)x.numel());
  HIP_OK(hipGetLastError());
}

torch::Tensor normalize(torch::Tensor x) {
  check_f32_gpu(x, "x");
  auto y = torch::empty_like(x);
  launch_normalize(x, y);
  return y;
}

// the same launch into the caller's buffer (x and y distinct)
void normalize_out(torch::Tensor x, torch::Tensor y) {
  check_f32_gpu(x, "x");
  check_f32_gpu(y, "y");
  TORCH_CHECK(y.numel() == x.numel() && y.data_ptr() != x.data_ptr(),
              "normalize_out: y must be a second buffer of x's size");
  launch_normalize(x, y);
}

torch::Tensor q_target(torch::Tensor r, torch::Tensor d, torch::Tensor qn,
                       double gamma) {
  check_f32_gpu(r, "rewards");
  auto out = torch::empty_like(r);
  int n = (int)r.numel();
  hipLaunchKernelGGL(q_target_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     current_stream(), r.data_ptr<float>(), d.data_ptr<float>(),
                     qn.data_ptr<float>(), out.data_ptr<float>(), (float)gamma, n);
  HIP_OK(hipGetLastError());
  return out;
}

// ---------------------------------------------------------------------------
// fused updates
// ---------------------------------------------------------------------------
void fused_adam_(std::vector<torch::Tensor> params, std::vector<torch::Tensor> grads,
                 std::vector<torch::Tensor> exp_avgs,
                 std::vector<torch::Tensor> exp_avg_sqs,
                 std::vector<torch::Tensor> steps, double lr, double beta1,
                 double beta2, double eps, double weight_decay,
                 double step_delta, bool do_bump,
                 c10::optional<torch::Tensor> gate) {
  const float* gate_ptr = nullptr;
  if (gate.has_value()) {
    TORCH_CHECK(gate->scalar_type() == torch::kFloat32 && gate->is_cuda() &&
                    gate->numel() == 1,
                "gate must be a 1-element fp32 CUDA tensor");
    gate_ptr = gate->data_ptr<float>();
  }
  size_t n = params.size();
  for (size_t base = 0; base < n; base += MT_MAX_TENSORS) {
    AdamArgs a{};
    a.n_tensors = (int)std::min((size_t)MT_MAX_TENSORS, n - base);
    for (int i = 0; i < a.n_tensors; ++i) {
      size_t t = base + i;
      a.p[i] = params[t].data_ptr<float>();
      a.g[i] = grads[t].data_ptr<float>();
      a.m[i] = exp_avgs[t].data_ptr<float>();
      a.v[i] = exp_avg_sqs[t].data_ptr<float>();
      a.step[i] = steps[t].data_ptr<float>();
      a.numel[i] = (int)params[t].numel();
    }
    a.lr = (float)lr;
    a.beta1 = (float)beta1;
    a.beta2 = (float)beta2;
    a.eps = (float)eps;
    a.weight_decay = (float)weight_decay;
    a.step_delta = (float)step_delta;
    a.gate = gate_ptr;
    int max_chunks = 1;
    for (int i = 0; i < a.n_tensors; ++i)
      max_chunks = std::max(max_chunks, (a.numel[i] + 8191) / 8192);
    hipLaunchKernelGGL(fused_adam_kernel, dim3(a.n_tensors, max_chunks),
                       dim3(256), 0, current_stream(), a);
    HIP_OK(hipGetLastError());
    if (do_bump) {
      a.step_delta = 1.f;
      hipLaunchKernelGGL(adam_step_bump_kernel, dim3(1), dim3(MT_MAX_TENSORS), 0,
                         current_stream(), a);
      HIP_OK(hipGetLastError());
    }
  }
}

__global__ void adam_step_bump_dev_kernel(AdamArgs a, const float* amount);

// bump by a device scalar (captured gated policy loop)
void adam_bump_dev_(std::vector<torch::Tensor> steps, torch::Tensor amount) {
  size_t n = steps.size();
  for (size_t base = 0; base < n; base += MT_MAX_TENSORS) {
    AdamArgs a{};
    a.n_tensors = (int)std::min((size_t)MT_MAX_TENSORS, n - base);
    for (int i = 0; i < a.n_tensors; ++i)
      a.step[i] = steps[base + i].data_ptr<float>();
    hipLaunchKernelGGL(adam_step_bump_dev_kernel, dim3(1), dim3(MT_MAX_TENSORS),
                       0, current_stream(), a, amount.data_ptr<float>());
    HIP_OK(hipGetLastError());
  }
}

// bump-only entry (captured value loop: ONE bump of +num_iters per replay)
void adam_bump_(std::vector<torch::Tensor> steps, double amount) {
  size_t n = steps.size();
  for (size_t base = 0; base < n; base += MT_MAX_TENSORS) {
    AdamArgs a{};
    a.n_tensors = (int)std::min((size_t)MT_MAX_TENSORS, n - base);
    for (int i = 0; i < a.n_tensors; ++i)
      a.step[i] = steps[base + i].data_ptr<float>();
    a.step_delta = (float)amount;
    hipLaunchKernelGGL(adam_step_bump_kernel, dim3(1), dim3(MT_MAX_TENSORS), 0,
                       current_stream(), a);
    HIP_OK(hipGetLastError());
  }
}

// deferred value-loss finalize over all iterations at once
torch::Tensor value_loss_finalize(torch::Tensor partials, int64_t fb) {
  check_f32_gpu(partials, "partials");
  const int rows = (int)partials.size(0);
  const int stride = (int)partials.size(1);
  TORCH_CHECK((int)fb <= stride, "fb exceeds partials row stride");
  auto scalars = torch::empty({rows}, partials.options());
  // one wave per row, four rows per workgroup
  hipLaunchKernelGGL(value_loss_finalize_rows, dim3((rows + 3) / 4),
                     dim3(256), 0, current_stream(),
                     partials.data_ptr<float>(), scalars.data_ptr<float>(),
                     rows, (int)fb, stride);
  HIP_OK(hipGetLastError());
  return scalars;
}

// The captured PPO epoch's tail in one launch (ppo_epoch_epilogue,
// update_kernels.hip): ppo_gate_update_ on the flushed KL, adam_bump_dev_ of
// pol_steps by the executed-update count, adam_bump_ of val_steps by
// val_bump, value_loss_finalize of partials into losses, and src -> dst for
// every tensor of the old-policy sync.  iters_out receives the count the
// host reads; gate = 1 and iters_done = 0 are left for the next replay.
void ppo_epoch_epilogue_(torch::Tensor gate, torch::Tensor kl, torch::Tensor kl_final,
                         torch::Tensor iters_done, torch::Tensor iters_out,
                         double thr, std::vector<torch::Tensor> pol_steps,
                         std::vector<torch::Tensor> val_steps, double val_bump,
                         torch::Tensor partials, int64_t fb, torch::Tensor losses,
                         std::vector<torch::Tensor> srcs,
                         std::vector<torch::Tensor> dsts) {
  PPOEpilogueArgs a{};
  for (const torch::Tensor* t : {&gate, &kl, &kl_final, &iters_done, &iters_out}) {
    check_f32_gpu(*t, "gate/kl/kl_final/iters_done/iters_out");
    TORCH_CHECK(t->numel() >= 1, "gate bookkeeping scalars must not be empty");
  }
  TORCH_CHECK(gate.numel() == 1 && kl_final.numel() == 1 && iters_done.numel() == 1 &&
                  iters_out.numel() == 1,
              "gate bookkeeping scalars must have 1 element");
  a.gate = gate.data_ptr<float>();
  a.kl = kl.data_ptr<float>();
  a.kl_final = kl_final.data_ptr<float>();
  a.iters_done = iters_done.data_ptr<float>();
  a.iters_out = iters_out.data_ptr<float>();
  a.thr = (float)thr;
  TORCH_CHECK(pol_steps.size() <= MT_MAX_TENSORS && val_steps.size() <= MT_MAX_TENSORS &&
                  srcs.size() <= MT_MAX_TENSORS && srcs.size() == dsts.size(),
              "ppo_epoch_epilogue_: at most ", MT_MAX_TENSORS,
              " step counters per optimizer and synced tensors");
  auto fill_steps = [](const std::vector<torch::Tensor>& steps, float** out) {
    for (size_t i = 0; i < steps.size(); ++i) {
      TORCH_CHECK(steps[i].is_cuda() && steps[i].scalar_type() == torch::kFloat32 &&
                      steps[i].numel() == 1,
                  "adam step must be a 1-element fp32 GPU tensor");
      out[i] = steps[i].data_ptr<float>();
    }
  };
  fill_steps(pol_steps, a.pol_step);
  fill_steps(val_steps, a.val_step);
  a.n_pol_steps = (int)pol_steps.size();
  a.n_val_steps = (int)val_steps.size();
  a.val_bump = (float)val_bump;
  check_f32_gpu(partials, "partials");
  check_f32_gpu(losses, "losses");
  TORCH_CHECK(partials.dim() == 2, "partials must be [rows, stride]");
  a.rows = (int)partials.size(0);
  a.row_stride = (int)partials.size(1);
  a.fb = (int)fb;
  TORCH_CHECK(fb >= 0 && a.fb <= a.row_stride, "fb exceeds partials row stride");
  TORCH_CHECK(losses.numel() == a.rows, "losses must hold one element per row");
  a.partials = partials.data_ptr<float>();
  a.losses = losses.data_ptr<float>();
  a.n_sync = (int)srcs.size();
  for (int i = 0; i < a.n_sync; ++i) {
    check_f32_gpu(srcs[i], "sync source");
    check_f32_gpu(dsts[i], "sync destination");
    TORCH_CHECK(srcs[i].numel() == dsts[i].numel() &&
                    srcs[i].numel() < (1LL << 31),
                "sync source and destination differ in size");
    a.src[i] = srcs[i].data_ptr<float>();
    a.dst[i] = dsts[i].data_ptr<float>();
    a.numel[i] = (int)srcs[i].numel();
  }
  hipLaunchKernelGGL(ppo_epoch_epilogue, dim3((a.rows + 3) / 4 + 1 + a.n_sync),
                     dim3(256), 0, current_stream(), a);
  HIP_OK(hipGetLastError());
}

void fused_polyak_(std::vector<torch::Tensor> srcs, std::vector<torch::Tensor> dsts,
                   double rho) {
  size_t n = srcs.size();
  for (size_t base = 0; base < n; base += MT_MAX_TENSORS) {
    PolyakArgs a{};
    a.n_tensors = (int)std::min((size_t)MT_MAX_TENSORS, n - base);
    for (int i = 0; i < a.n_tensors; ++i) {
      size_t t = base + i;
      a.src[i] = srcs[t].data_ptr<float>();
      a.dst[i] = dsts[t].data_ptr<float>();
      a.numel[i] = (int)srcs[t].numel();
    }
    a.rho = (float)rho;
    int max_chunks = 1;
    for (int i = 0; i < a.n_tensors; ++i)
      max_chunks = std::max(max_chunks, (a.numel[i] + 8191) / 8192);
    hipLaunchKernelGGL(fused_polyak_kernel, dim3(a.n_tensors, max_chunks),
                       dim3(256), 0, current_stream(), a);
    HIP_OK(hipGetLastError());
  }
}

static const unsigned long long* ctr_ptr(const c10::optional<torch::Tensor>& t) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->scalar_type() == torch::kInt64 && t->is_cuda() && t->numel() == 1,
              "offset_ctr must be a 1-element int64 CUDA tensor");
  return reinterpret_cast<const unsigned long long*>(t->data_ptr<int64_t>());
}

torch::Tensor gaussian_sample(torch::Tensor mean, torch::Tensor log_std,
                              int64_t seed, int64_t offset, double noise_scale,
                              double limit,
                              c10::optional<torch::Tensor> offset_ctr,
                              c10::optional<torch::Tensor> out_opt) {
  check_f32_gpu(mean, "mean");
  const int B = (int)mean.size(0);
  const int D = (int)mean.size(1);
  auto out = out_opt.has_value() ? *out_opt : torch::empty_like(mean);
  const int total = B * D;
  hipLaunchKernelGGL(gaussian_sample_kernel,
                     dim3(std::min(256, (total + 255) / 256)), dim3(256), 0,
                     current_stream(), mean.data_ptr<float>(),
                     log_std.data_ptr<float>(), out.data_ptr<float>(), B, D,
                     (uint64_t)seed, (uint64_t)offset, (float)noise_scale,
                     (float)limit, ctr_ptr(offset_ctr));
  HIP_OK(hipGetLastError());
  return out;
}

torch::Tensor categorical_sample(torch::Tensor logits, int64_t seed,
                                 int64_t offset,
                                 c10::optional<torch::Tensor> offset_ctr,
                                 c10::optional<torch::Tensor> out_opt) {
  check_f32_gpu(logits, "logits");
  const int B = (int)logits.size(0);
  const int N = (int)logits.size(1);
  auto out = out_opt.has_value()
                 ? *out_opt
                 : torch::empty({B}, logits.options().dtype(torch::kInt64));
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() &&
                  out.scalar_type() == torch::kInt64 && out.numel() == B,
              "categorical_sample: out must be a contiguous int64 CUDA tensor [B]");
  hipLaunchKernelGGL(categorical_sample_kernel,
                     dim3(std::min(256, (B + 255) / 256)), dim3(256), 0,
                     current_stream(), logits.data_ptr<float>(),
                     out.data_ptr<int64_t>(), B, N, (uint64_t)seed,
                     (uint64_t)offset, ctr_ptr(offset_ctr));
  HIP_OK(hipGetLastError());
  return out;
}

// CartPole carry tensors: state fp64 [N,4], elapsed int32 [N]
static int check_cartpole_carry(const torch::Tensor& state,
                                const torch::Tensor& elapsed) {
  TORCH_CHECK(state.is_cuda() && state.is_contiguous() &&
                  state.scalar_type() == torch::kFloat64 && state.dim() == 2 &&
                  state.size(1) == 4,
              "state must be a contiguous float64 CUDA tensor [N, 4]");
  TORCH_CHECK(elapsed.is_cuda() && elapsed.is_contiguous() &&
                  elapsed.scalar_type() == torch::kInt32 &&
                  elapsed.numel() == state.size(0),
              "elapsed must be a contiguous int32 CUDA tensor [N]");
  return (int)state.size(0);
}

static void check_out(const torch::Tensor& t, torch::ScalarType dt, int64_t numel,
                      const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == dt &&
                  t.numel() == numel,
              name, ": wrong device, dtype, layout or size");
}

// ---- checks shared by the persistent rollout / collect / evaluation bindings
// the default per-workgroup dynamic-LDS limit (no opt-in attribute needed):
// the budget of the CartPole and Pendulum rollout and the evaluation kernels
#define DEFAULT_LDS_LIMIT (64 * 1024)

// dynamic LDS of a persistent kernel with the observation tile + 2 activation
// tiles beside the net (every one but the synthetic-env kernel)
static size_t persistent_lds_bytes(const NetLayout& n) {
  return (size_t)net_lds_floats(3, n.dims, n.L) * sizeof(float);
}

static size_t ppo_rollout_fused_lds_bytes(const NetLayout& n, int O, int A) {
  return (size_t)rollout_fused_lds_floats(n.dims, n.L, O, A) * sizeof(float);
}

// an epoch's step count or an evaluation's horizon
static int check_step_count(int64_t v, const char* name) {
  TORCH_CHECK(v >= 1 && v <= (1 << 24), name, " out of range");
  return (int)v;
}

static void check_net_device(const std::vector<torch::Tensor>& weights,
                             const std::vector<torch::Tensor>& biases,
                             const torch::Device& dev) {
  for (const auto& t : weights)
    TORCH_CHECK(t.device() == dev, "the net is on another device");
  for (const auto& t : biases)
    TORCH_CHECK(t.device() == dev, "the net is on another device");
}

// the lockstep cuts of an epoch of `steps` steps -> a.cut_step / a.n_cuts:
// at most ROLLOUT_MAX_CUTS step indices, strictly ascending (what
// lockstep_cuts of the samplers produces, and what makes slot j of the
// cut-indexed outputs belong to cuts[j] alone)
template <class Args>
static void fill_cuts(Args& a, const std::vector<int64_t>& cuts, int64_t steps,
                      const char* who) {
  TORCH_CHECK(cuts.size() <= ROLLOUT_MAX_CUTS, who, ": too many cuts");
  a.n_cuts = (int)cuts.size();
  for (int c = 0; c < a.n_cuts; ++c) {
    TORCH_CHECK(cuts[c] >= 0 && cuts[c] < steps, "cut step out of range");
    TORCH_CHECK(c == 0 || cuts[c] > cuts[c - 1], "cuts must be ascending");
    a.cut_step[c] = (int)cuts[c];
  }
}

// -> {obs, reward, done, final_obs}; state and elapsed are updated in place
std::vector<torch::Tensor> cartpole_env_step(
    torch::Tensor state, torch::Tensor elapsed, torch::Tensor actions,
    int64_t max_steps, int64_t seed, int64_t offset,
    c10::optional<torch::Tensor> offset_ctr, c10::optional<torch::Tensor> obs_opt,
    c10::optional<torch::Tensor> final_opt, c10::optional<torch::Tensor> reward_opt,
    c10::optional<torch::Tensor> done_opt) {
  const int N = check_cartpole_carry(state, elapsed);
  check_out(actions, torch::kInt64, N, "actions");
  const auto f32 = state.options().dtype(torch::kFloat32);
  auto obs = obs_opt.has_value() ? *obs_opt : torch::empty({N, 4}, f32);
  auto fin = final_opt.has_value() ? *final_opt : torch::empty({N, 4}, f32);
  auto reward = reward_opt.has_value() ? *reward_opt : torch::empty({N}, f32);
  auto done = done_opt.has_value()
                  ? *done_opt
                  : torch::empty({N}, state.options().dtype(torch::kUInt8));
  check_out(obs, torch::kFloat32, (int64_t)N * 4, "obs");
  check_out(fin, torch::kFloat32, (int64_t)N * 4, "final_obs");
  check_out(reward, torch::kFloat32, N, "reward");
  check_out(done, torch::kUInt8, N, "done");
  hipLaunchKernelGGL(cartpole_env_step_kernel,
                     dim3(std::min(256, (N + 255) / 256)), dim3(256), 0,
                     current_stream(), state.data_ptr<double>(),
                     elapsed.data_ptr<int>(), actions.data_ptr<int64_t>(),
                     obs.data_ptr<float>(), fin.data_ptr<float>(),
                     reward.data_ptr<float>(), done.data_ptr<uint8_t>(), N,
                     (int)max_steps, (uint64_t)seed, (uint64_t)offset,
                     ctr_ptr(offset_ctr));
  HIP_OK(hipGetLastError());
  return {obs, reward, done, fin};
}

torch::Tensor cartpole_env_reset(torch::Tensor state, torch::Tensor elapsed,
                                 int64_t seed, int64_t offset,
                                 c10::optional<torch::Tensor> offset_ctr,
                                 c10::optional<torch::Tensor> obs_opt) {
  const int N = check_cartpole_carry(state, elapsed);
  auto obs = obs_opt.has_value()
                 ? *obs_opt
                 : torch::empty({N, 4}, state.options().dtype(torch::kFloat32));
  check_out(obs, torch::kFloat32, (int64_t)N * 4, "obs");
  hipLaunchKernelGGL(cartpole_env_reset_kernel,
                     dim3(std::min(256, (N + 255) / 256)), dim3(256), 0,
                     current_stream(), state.data_ptr<double>(),
                     elapsed.data_ptr<int>(), obs.data_ptr<float>(), N,
                     (uint64_t)seed, (uint64_t)offset, ctr_ptr(offset_ctr));
  HIP_OK(hipGetLastError());
  return obs;
}

// Pendulum carry tensor: state fp64 [N,2]
static int check_pendulum_carry(const torch::Tensor& state) {
  TORCH_CHECK(state.is_cuda() && state.is_contiguous() &&
                  state.scalar_type() == torch::kFloat64 && state.dim() == 2 &&
                  state.size(1) == 2 && state.size(0) >= 1,
              "state must be a contiguous float64 CUDA tensor [N, 2]");
  return (int)state.size(0);
}

// -> {obs, reward, final_obs}; state is updated in place.  do_reset: the
// lockstep truncation step (every instance draws a fresh init state)
std::vector<torch::Tensor> pendulum_env_step(
    torch::Tensor state, torch::Tensor actions, bool do_reset, int64_t seed,
    int64_t offset, c10::optional<torch::Tensor> offset_ctr,
    c10::optional<torch::Tensor> obs_opt, c10::optional<torch::Tensor> final_opt,
    c10::optional<torch::Tensor> reward_opt) {
  const int N = check_pendulum_carry(state);
  check_out(actions, torch::kFloat32, N, "actions");
  if (obs_opt.has_value()) check_out(*obs_opt, torch::kFloat32, (int64_t)N * 3, "obs");
  if (final_opt.has_value())
    check_out(*final_opt, torch::kFloat32, (int64_t)N * 3, "final_obs");
  if (reward_opt.has_value()) check_out(*reward_opt, torch::kFloat32, N, "reward");
  const unsigned long long* ctr = ctr_ptr(offset_ctr);
  const auto f32 = state.options().dtype(torch::kFloat32);
  auto obs = obs_opt.has_value() ? *obs_opt : torch::empty({N, 3}, f32);
  auto fin = final_opt.has_value() ? *final_opt : torch::empty({N, 3}, f32);
  auto reward = reward_opt.has_value() ? *reward_opt : torch::empty({N}, f32);
  hipLaunchKernelGGL(pendulum_env_step_kernel,
                     dim3(std::min(256, (N + 255) / 256)), dim3(256), 0,
                     current_stream(), state.data_ptr<double>(),
                     actions.data_ptr<float>(), obs.data_ptr<float>(),
                     fin.data_ptr<float>(), reward.data_ptr<float>(), N,
                     do_reset ? 1 : 0, (uint64_t)seed, (uint64_t)offset, ctr);
  HIP_OK(hipGetLastError());
  return {obs, reward, fin};
}

// fresh init states into `state` (draw) or only the observation of the
// states as they stand (!draw); -> obs [N,3]
torch::Tensor pendulum_env_reset(torch::Tensor state, int64_t seed, int64_t offset,
                                 c10::optional<torch::Tensor> offset_ctr,
                                 c10::optional<torch::Tensor> obs_opt, bool draw) {
  const int N = check_pendulum_carry(state);
  if (obs_opt.has_value()) check_out(*obs_opt, torch::kFloat32, (int64_t)N * 3, "obs");
  const unsigned long long* ctr = ctr_ptr(offset_ctr);
  auto obs = obs_opt.has_value()
                 ? *obs_opt
                 : torch::empty({N, 3}, state.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(pendulum_env_reset_kernel,
                     dim3(std::min(256, (N + 255) / 256)), dim3(256), 0,
                     current_stream(), state.data_ptr<double>(),
                     obs.data_ptr<float>(), N, draw ? 1 : 0, (uint64_t)seed,
                     (uint64_t)offset, ctr);
  HIP_OK(hipGetLastError());
  return obs;
}

std::vector<torch::Tensor> synthetic_env_step(torch::Tensor state,
                                              torch::Tensor actions,
                                              torch::Tensor A, torch::Tensor B,
                                              torch::Tensor w, double sigma,
                                              int64_t seed, int64_t offset,
                                              bool do_reset,
                                              c10::optional<torch::Tensor> offset_ctr,
                                              c10::optional<torch::Tensor> s_out_opt,
                                              c10::optional<torch::Tensor> final_out_opt,
                                              c10::optional<torch::Tensor> reward_opt) {
  check_f32_gpu(state, "state");
  check_f32_gpu(actions, "actions");
  const int N = (int)state.size(0);
  const int O = (int)state.size(1);
  const int Adim = (int)actions.size(1);
  TORCH_CHECK(O <= 64, "synthetic_env_step: obs_dim must be <= 64 (one wave per row)");
  auto s_out = s_out_opt.has_value() ? *s_out_opt : torch::empty_like(state);
  auto final_out = final_out_opt.has_value() ? *final_out_opt
                   : (do_reset ? torch::empty_like(state) : s_out);
  auto reward = reward_opt.has_value() ? *reward_opt
                                       : torch::empty({N}, state.options());
  hipLaunchKernelGGL(synthetic_env_step_kernel, dim3(N), dim3(64), 0,
                     current_stream(), state.data_ptr<float>(),
                     actions.data_ptr<float>(), A.data_ptr<float>(),
                     B.data_ptr<float>(), w.data_ptr<float>(),
                     s_out.data_ptr<float>(), final_out.data_ptr<float>(),
                     reward.data_ptr<float>(), N, O, Adim, (float)sigma,
                     (uint64_t)seed, (uint64_t)offset, do_reset ? 1 : 0,
                     ctr_ptr(offset_ctr));
  HIP_OK(hipGetLastError());
  return {s_out, reward, final_out};
}

torch::Tensor synthetic_env_reset(int64_t num_envs, int64_t obs_dim,
                                  torch::Tensor like, int64_t seed,
                                  int64_t offset,
                                  c10::optional<torch::Tensor> offset_ctr,
                                  c10::optional<torch::Tensor> out_opt) {
  auto s_out = out_opt.has_value()
                   ? *out_opt
                   : torch::empty({num_envs, obs_dim}, like.options());
  const int total = (int)(num_envs * obs_dim);
  hipLaunchKernelGGL(synthetic_env_reset_kernel,
                     dim3(std::min(256, (total + 255) / 256)), dim3(256), 0,
                     current_stream(), s_out.data_ptr<float>(), total,
                     (uint64_t)seed, (uint64_t)offset, ctr_ptr(offset_ctr));
  HIP_OK(hipGetLastError());
  return s_out;
}

torch::Tensor td3_smooth(torch::Tensor a, int64_t seed, int64_t offset,
                         double scale, double clip, double limit,
                         c10::optional<torch::Tensor> offset_ctr) {
  check_f32_gpu(a, "actions");
  auto out = torch::empty_like(a);
  const int total = (int)a.numel();
  hipLaunchKernelGGL(td3_smooth_kernel,
                     dim3(std::min(256, (total + 255) / 256)), dim3(256), 0,
                     current_stream(), a.data_ptr<float>(),
                     out.data_ptr<float>(), total, (uint64_t)seed,
                     (uint64_t)offset, (float)scale, (float)clip,
                     (float)limit, ctr_ptr(offset_ctr));
  HIP_OK(hipGetLastError());
  return out;
}

torch::Tensor q_target_min2(torch::Tensor r, torch::Tensor d, torch::Tensor q1,
                            torch::Tensor q2, double gamma) {
  check_f32_gpu(r, "rewards");
  auto out = torch::empty_like(r);
  const int n = (int)r.numel();
  hipLaunchKernelGGL(q_target_min2_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     current_stream(), r.data_ptr<float>(), d.data_ptr<float>(),
                     q1.data_ptr<float>(), q2.data_ptr<float>(),
                     out.data_ptr<float>(), (float)gamma, n);
  HIP_OK(hipGetLastError());
  return out;
}

std::vector<torch::Tensor> replay_gather(torch::Tensor obs, torch::Tensor act,
                                         torch::Tensor rew, torch::Tensor nxt,
                                         torch::Tensor dn, torch::Tensor size_dev,
                                         int64_t B, int64_t seed, int64_t offset,
                                         c10::optional<torch::Tensor> offset_ctr) {
  check_f32_gpu(obs, "obs");
  check_f32_gpu(act, "act");
  check_f32_gpu(rew, "rew");
  check_f32_gpu(nxt, "nxt");
  check_f32_gpu(dn, "dn");
  TORCH_CHECK(size_dev.scalar_type() == torch::kInt64 && size_dev.is_cuda() &&
                  size_dev.numel() == 1,
              "size_dev must be a 1-element int64 CUDA tensor");
  ReplayGatherArgs a{};
  a.obs = obs.data_ptr<float>();
  a.act = act.data_ptr<float>();
  a.rew = rew.data_ptr<float>();
  a.nxt = nxt.data_ptr<float>();
  a.dn = dn.data_ptr<float>();
  a.size = reinterpret_cast<const long long*>(size_dev.data_ptr<int64_t>());
  a.B = (int)B;
  a.O = (int)obs.size(1);
  a.A = (int)act.size(1);
  auto qin = torch::empty({B, a.O + a.A}, obs.options());
  auto obs_out = torch::empty({B, a.O}, obs.options());
  auto nxt_out = torch::empty({B, a.O}, obs.options());
  auto rew_out = torch::empty({B}, obs.options());
  auto dn_out = torch::empty({B}, obs.options());
  a.qin = qin.data_ptr<float>();
  a.obs_out = obs_out.data_ptr<float>();
  a.nxt_out = nxt_out.data_ptr<float>();
  a.rew_out = rew_out.data_ptr<float>();
  a.dn_out = dn_out.data_ptr<float>();
  a.seed = (uint64_t)seed;
  a.offset = (uint64_t)offset;
  a.offset_ptr = ctr_ptr(offset_ctr);
  const long total = (long)a.B * (2 * a.O + a.A + 2);
  hipLaunchKernelGGL(replay_gather_kernel,
                     dim3((int)std::min<long>(512, (total + 255) / 256)),
                     dim3(256), 0, current_stream(), a);
  HIP_OK(hipGetLastError());
  return {qin, obs_out, nxt_out, rew_out, dn_out};
}

void ppo_gate_update_(torch::Tensor gate, torch::Tensor kl,
                      torch::Tensor kl_final, torch::Tensor iters_done,
                      double thr) {
  hipLaunchKernelGGL(ppo_gate_update_kernel, dim3(1), dim3(1), 0,
                     current_stream(), gate.data_ptr<float>(),
                     kl.data_ptr<float>(), kl_final.data_ptr<float>(),
                     iters_done.data_ptr<float>(), (float)thr);
  HIP_OK(hipGetLastError());
}

// ONE captured PPO policy iteration = 2 kernels:
//   1. DO_FWD fused kernel: forward (LDS activations) + pending-KL /
//      loss (/ dlog_std) partials + clipped-surrogate dZ seed + whole-net
//      backward stage-1 (no input gradient).  After the first iteration
//      it returns at once while the gate is closed: a frozen iteration
//      costs a launch, not a kernel.
//   2. merged reduce+Adam over net params AND log_std (pseudo-layer)
//      with the gate bookkeeping folded in: every workgroup sums the
//      pending-KL partials and closes the gate if the KL crossed
//      1.5*maxkl (so this iteration's update is skipped, like the
//      reference's break at ppo.py:176-181); workgroup 0 records gate,
//      kl_final, iters_done and the iteration-0 loss.
// Narrow fp32 identity-head policies only: Gaussian (the bench config) or
// categorical, which has no log_std and so no pseudo-layer — its seed is
// the row softmax over the head tile.  The returned tensor is the (empty)
// dx slot.
namespace {

// what tells the two policy kinds apart on the host: the seed kind and,
// for Gaussian, log_std with its Adam state (the pseudo-layer)
struct PolicySeed {
  int kind;  // SEED_GAUSSIAN | SEED_CATEGORICAL
  const torch::Tensor* log_std = nullptr;
  const torch::Tensor* ls_m = nullptr;
  const torch::Tensor* ls_v = nullptr;
  bool gaussian() const { return kind == SEED_GAUSSIAN; }
  // argument-block slots / workspace elements of the pseudo-layer
  int reserve() const { return gaussian() ? 1 : 0; }
  int64_t extra(int D) const { return gaussian() ? D : 0; }
};

// everything one PPO policy iteration launches with: the fused kernel's
// argument blocks, the reduce+Adam block (log_std pseudo-layer if any
// and gate bookkeeping included) and the buffers they point into
struct PolicyIterBlocks {
  MLPBwdArgs ba;
  GaussSeedArgs ga;
  ReduceAdamArgs ra;
  torch::Tensor ws, loss_partials, kl_partials;
  size_t fused_lds;
  int fb;
  int64_t grand_ls;
};

// every check of one PPO policy iteration's arguments
NetLayout check_policy_iter(
    const PolicySeed& seed, const torch::Tensor& x,
    const std::vector<torch::Tensor>& weights,
    const std::vector<torch::Tensor>& biases, const std::vector<int64_t>& acts,
    const torch::Tensor& actions, const torch::Tensor& old_logp,
    const torch::Tensor& advantages, const std::vector<torch::Tensor>& adam_m,
    const std::vector<torch::Tensor>& adam_v, const torch::Tensor& adam_step,
    const torch::Tensor& gate, const torch::Tensor& kl_final,
    const torch::Tensor& iters_done, const torch::Tensor& loss_out) {
  // Gaussian: one slot of the fixed argument arrays goes to the log_std
  // pseudo-layer
  const NetLayout net =
      net_layout(x, weights, biases, acts, MLP_NARROW_WIDTH, seed.reserve());
  const int64_t batch = x.size(0);
  const int D = net.dims[net.L];
  TORCH_CHECK(acts[net.L - 1] == 0, "needs an identity head");
  TORCH_CHECK(fused_bwd_fits(net, true), "net too large for the fused iter");
  check_f32_gpu(actions, "actions");
  check_f32_gpu(old_logp, "old_logp");
  check_f32_gpu(advantages, "advantages");
  // Gaussian actions are [batch, D]; categorical ones a class index per row
  TORCH_CHECK(actions.numel() == (seed.gaussian() ? batch * D : batch) &&
                  old_logp.numel() == batch && advantages.numel() == batch,
              "actions/old_logp/advantages must be [batch, D] (Gaussian) or "
              "[batch] (categorical) / [batch] / [batch]");
  if (seed.gaussian()) {
    for (const torch::Tensor* t : {seed.log_std, seed.ls_m, seed.ls_v}) {
      check_f32_gpu(*t, "log_std and its adam state");
      TORCH_CHECK(t->numel() == D, "log_std and its adam state must be [D]");
    }
  }
  check_adam_state(weights, biases, adam_m, adam_v, adam_step);
  for (const torch::Tensor* t : {&gate, &kl_final, &iters_done, &loss_out}) {
    check_f32_gpu(*t, "gate/kl_final/iters_done/loss_out");
    TORCH_CHECK(t->numel() == 1, "gate bookkeeping scalars must have 1 element");
  }
  return net;
}

PolicyIterBlocks build_policy_iter(
    const PolicySeed& seed, const NetLayout& net, const torch::Tensor& x,
    const std::vector<torch::Tensor>& weights,
    const std::vector<torch::Tensor>& biases, const std::vector<int64_t>& acts,
    const torch::Tensor& actions, const torch::Tensor& old_logp,
    const torch::Tensor& advantages, double clip,
    const std::vector<torch::Tensor>& adam_m,
    const std::vector<torch::Tensor>& adam_v, const torch::Tensor& adam_step,
    double lr,
    double beta1, double beta2, double eps, double weight_decay,
    double step_delta, const torch::Tensor& gate, const torch::Tensor& kl_final,
    const torch::Tensor& iters_done, double thr, const torch::Tensor& loss_out,
    bool first_iter) {
  const int L = net.L;
  const int batch = (int)x.size(0);
  const int D = net.dims[L];
  auto opts = x.options();

  PolicyIterBlocks pb;
  pb.grand_ls = net.grand + seed.extra(D);  // + dlog_std pseudo-layer
  pb.fused_lds = fused_bwd_lds(net, true);
  pb.fb = (batch + BWD_FUSED_ROWS - 1) / BWD_FUSED_ROWS;

  pb.ws = torch::empty({(int64_t)pb.fb, pb.grand_ls}, opts);
  pb.loss_partials = torch::empty({pb.fb}, opts);
  pb.kl_partials = torch::empty({pb.fb}, opts);

  pb.ba = fill_bwd_args(x, weights, biases, acts, net, pb.grand_ls);
  GaussSeedArgs& ga = pb.ga;
  ga = GaussSeedArgs{};
  ga.actions = actions.data_ptr<float>();
  ga.old_logp = old_logp.data_ptr<float>();
  ga.adv = advantages.data_ptr<float>();
  ga.kind = seed.kind;
  ga.log_std = seed.gaussian() ? seed.log_std->data_ptr<float>() : nullptr;
  ga.kl_partials = pb.kl_partials.data_ptr<float>();
  ga.dls_off = (int)net.grand;
  ga.clip = (float)clip;
  // a frozen iteration skips the fused kernel.  The first iteration never
  // gates and its loss partials are always read, so it always runs.
  ga.skip_gate = first_iter ? nullptr : gate.data_ptr<float>();

  ReduceAdamArgs& ra = pb.ra;
  ra = fill_reduce_adam(weights, biases, net, pb.ws.data_ptr<float>(),
                        pb.grand_ls, pb.fb, adam_m, adam_v, adam_step, lr,
                        beta1, beta2, eps, weight_decay, step_delta, gate);
  if (seed.gaussian()) {
    ra.n_layers = L + 1;
    // log_std pseudo-layer: bias-only (wsize 0)
    ra.pw[L] = nullptr;
    ra.pb[L] = seed.log_std->data_ptr<float>();
    ra.mw[L] = nullptr;
    ra.mb[L] = seed.ls_m->data_ptr<float>();
    ra.vw[L] = nullptr;
    ra.vb[L] = seed.ls_v->data_ptr<float>();
    ra.total[L] = D;
    ra.wsize[L] = 0;
  }
  // gate bookkeeping block: every workgroup derives the open/closed
  // decision itself from the partials, workgroup 0 records it
  ra.kl_partials = pb.kl_partials.data_ptr<float>();
  ra.loss_partials = pb.loss_partials.data_ptr<float>();
  ra.gate_rw = gate.data_ptr<float>();
  ra.kl_final = kl_final.data_ptr<float>();
  ra.iters_done = iters_done.data_ptr<float>();
  ra.loss_out = loss_out.data_ptr<float>();
  ra.inv_b = 1.f / (float)batch;
  ra.thr = (float)thr;
  ra.first_iter = first_iter ? 1 : 0;
  return pb;
}

// the policy iteration of either kind
torch::Tensor ppo_policy_iter(
    const PolicySeed& seed, const torch::Tensor& x,
    const std::vector<torch::Tensor>& weights,
    const std::vector<torch::Tensor>& biases, const std::vector<int64_t>& acts,
    const torch::Tensor& actions, const torch::Tensor& old_logp,
    const torch::Tensor& advantages, double clip,
    const std::vector<torch::Tensor>& adam_m,
    const std::vector<torch::Tensor>& adam_v, const torch::Tensor& adam_step,
    double lr, double beta1, double beta2, double eps, double weight_decay,
    double step_delta, const torch::Tensor& gate, const torch::Tensor& kl_final,
    const torch::Tensor& iters_done, double thr, const torch::Tensor& loss_out,
    bool first_iter) {
  const NetLayout net = check_policy_iter(
      seed, x, weights, biases, acts, actions, old_logp, advantages, adam_m,
      adam_v, adam_step, gate, kl_final, iters_done, loss_out);
  const PolicyIterBlocks pb = build_policy_iter(
      seed, net, x, weights, biases, acts, actions, old_logp, advantages, clip,
      adam_m, adam_v, adam_step, lr, beta1, beta2, eps, weight_decay,
      step_delta, gate, kl_final, iters_done, thr, loss_out, first_iter);
  auto stream = current_stream();
  // no input gradient: the update is fused, nobody reads dx
  launch_mlp_bwd_fused(pb.ba, x.data_ptr<float>(), nullptr, nullptr,
                       pb.ws.data_ptr<float>(), nullptr,
                       pb.loss_partials.data_ptr<float>(), pb.fused_lds, pb.fb,
                       0, stream, 1, pb.ga, 0);
  HIP_OK(hipGetLastError());
  launch_mlp_grad_reduce_adam(pb.ra, (long)pb.grand_ls, stream);
  HIP_OK(hipGetLastError());
  return torch::empty({0}, x.options());  // dx slot: never computed here
}

}  // namespace

torch::Tensor gaussian_ppo_policy_iter(
    torch::Tensor x, std::vector<torch::Tensor> weights,
    std::vector<torch::Tensor> biases, std::vector<int64_t> acts,
    torch::Tensor actions, torch::Tensor old_logp, torch::Tensor advantages,
    torch::Tensor log_std, double clip, std::vector<torch::Tensor> adam_m,
    std::vector<torch::Tensor> adam_v, torch::Tensor ls_m, torch::Tensor ls_v,
    torch::Tensor adam_step, double lr, double beta1, double beta2, double eps,
    double weight_decay, double step_delta, torch::Tensor gate,
    torch::Tensor kl_final, torch::Tensor iters_done, double thr,
    torch::Tensor loss_out, bool first_iter) {
  return ppo_policy_iter(
      PolicySeed{SEED_GAUSSIAN, &log_std, &ls_m, &ls_v}, x, weights, biases,
      acts, actions, old_logp, advantages, clip, adam_m, adam_v, adam_step, lr,
      beta1, beta2, eps, weight_decay, step_delta, gate, kl_final, iters_done,
      thr, loss_out, first_iter);
}

// gaussian_ppo_policy_iter for a categorical policy: no log_std, ls_m, ls_v;
// actions is float32 [batch] (class indices, as categorical_policy_loss
// takes them)
torch::Tensor categorical_ppo_policy_iter(
    torch::Tensor x, std::vector<torch::Tensor> weights,
    std::vector<torch::Tensor> biases, std::vector<int64_t> acts,
    torch::Tensor actions, torch::Tensor old_logp, torch::Tensor advantages,
    double clip, std::vector<torch::Tensor> adam_m,
    std::vector<torch::Tensor> adam_v, torch::Tensor adam_step, double lr,
    double beta1, double beta2, double eps, double weight_decay,
    double step_delta, torch::Tensor gate, torch::Tensor kl_final,
    torch::Tensor iters_done, double thr, torch::Tensor loss_out,
    bool first_iter) {
  return ppo_policy_iter(
      PolicySeed{SEED_CATEGORICAL}, x, weights, biases, acts, actions,
      old_logp, advantages, clip, adam_m, adam_v, adam_step, lr, beta1, beta2,
      eps, weight_decay, step_delta, gate, kl_final, iters_done, thr, loss_out,
      first_iter);
}

// The shape-specialised twin kernel (mlp_bwd_fused_twin_shaped_f32) covers
// 3-layer nets [in <= 64, 64, 32, out <= 16] on 32-row blocks; the value
// half has out == 1.  dims = [in, hidden..., out] of each net.
// RL_REPLICAS_AMD_TWIN_SHAPED=0 forces the generic twin kernel; the switch
// is read per call (a captured graph keeps what it was captured with).
static bool twin_shaped_net_ok(const std::vector<int64_t>& d, int64_t max_out) {
  return d.size() == 4 && d[0] >= 1 && d[0] <= 64 && d[1] == 64 &&
         d[2] == 32 && d[3] >= 1 && d[3] <= max_out;
}

bool ppo_twin_uses_shaped(std::vector<int64_t> p_dims,
                          std::vector<int64_t> v_dims, int64_t batch) {
  const char* e = getenv("RL_REPLICAS_AMD_TWIN_SHAPED");
  if (e != nullptr && e[0] == '0' && e[1] == '\0') return false;
  static_assert(BWD_FUSED_ROWS == 32, "the shaped twin kernel has 32-row blocks");
  return twin_shaped_net_ok(p_dims, 16) && twin_shaped_net_ok(v_dims, 1) &&
         p_dims[0] == v_dims[0];
}

static std::vector<int64_t> net_dims(const NetLayout& n) {
  return std::vector<int64_t>(n.dims, n.dims + n.L + 1);
}

// Policy iteration i and value iteration i of one PPO epoch in the SAME
// two launches (the two loops are independent: neither reads what the
// other writes):
//   1. twin fused kernel, grid (fb, 2): the policy half of
//      gaussian_ppo_policy_iter / categorical_ppo_policy_iter and the
//      fwd_in_kernel fused-Adam half of value_mlp_backward;
//   2. twin reduce+Adam: the policy's gated update with its bookkeeping
//      and the value net's ungated one.
// Arguments are those of the policy iteration binding, then the value net's
// (v_*).  v_partials_out is the caller's deferred loss-partials row.  Each
// net's result is bitwise what its own binding gives.  The shape-specialised
// kernel has the Gaussian seed only: categorical nets always take the
// generic twin kernel.
namespace {

void ppo_value_twin_iter(
    const PolicySeed& seed, const torch::Tensor& x,
    const std::vector<torch::Tensor>& weights,
    const std::vector<torch::Tensor>& biases, const std::vector<int64_t>& acts,
    const torch::Tensor& actions, const torch::Tensor& old_logp,
    const torch::Tensor& advantages, double clip,
    const std::vector<torch::Tensor>& adam_m,
    const std::vector<torch::Tensor>& adam_v, const torch::Tensor& adam_step,
    double lr, double beta1, double beta2, double eps, double weight_decay,
    double step_delta, const torch::Tensor& gate, const torch::Tensor& kl_final,
    const torch::Tensor& iters_done, double thr, const torch::Tensor& loss_out,
    bool first_iter, const torch::Tensor& v_x,
    const std::vector<torch::Tensor>& v_weights,
    const std::vector<torch::Tensor>& v_biases,
    const std::vector<int64_t>& v_acts, const torch::Tensor& returns,
    const torch::Tensor& v_partials_out,
    const std::vector<torch::Tensor>& v_adam_m,
    const std::vector<torch::Tensor>& v_adam_v,
    const torch::Tensor& v_adam_step, double v_lr, double v_beta1,
    double v_beta2, double v_eps, double v_weight_decay, double v_step_delta) {
  const NetLayout net = check_policy_iter(
      seed, x, weights, biases, acts, actions, old_logp, advantages, adam_m,
      adam_v, adam_step, gate, kl_final, iters_done, loss_out);
  TORCH_CHECK(v_x.data_ptr() == x.data_ptr() && v_x.sizes() == x.sizes(),
              "the twin iteration needs the same x for both nets");
  const NetLayout vnet =
      net_layout(x, v_weights, v_biases, v_acts, MLP_NARROW_WIDTH);
  const int fb = ((int)x.size(0) + BWD_FUSED_ROWS - 1) / BWD_FUSED_ROWS;
  check_f32_gpu(returns, "returns");
  TORCH_CHECK(returns.numel() == x.size(0), "returns must be [batch]");
  TORCH_CHECK(vnet.dims[vnet.L] == 1 && v_acts[vnet.L - 1] == 0,
              "the value half needs a 1-output identity head");
  TORCH_CHECK(fused_bwd_fits(vnet, true),
              "value net too large for the fused iter");
  check_adam_state(v_weights, v_biases, v_adam_m, v_adam_v, v_adam_step);
  check_f32_gpu(v_partials_out, "v_partials_out");
  TORCH_CHECK(v_partials_out.numel() >= fb, "v_partials_out too small");
  TORCH_CHECK(mlp_reduce_adam_is_staged(
                  fb, (long)(net.grand + seed.extra(net.dims[net.L]))) &&
                  mlp_reduce_adam_is_staged(fb, (long)vnet.grand),
              "the twin reduce needs both nets on the staged reduce");
  const bool shaped =
      seed.gaussian() &&
      ppo_twin_uses_shaped(net_dims(net), net_dims(vnet), x.size(0));
  TORCH_CHECK(!shaped || mlp_bwd_fused_shaped_lds(net.dims[0]) <= 80 * 1024,
              "shaped twin kernel over its LDS budget");

  const PolicyIterBlocks pb = build_policy_iter(
      seed, net, x, weights, biases, acts, actions, old_logp, advantages, clip,
      adam_m, adam_v, adam_step, lr, beta1, beta2, eps, weight_decay,
      step_delta, gate, kl_final, iters_done, thr, loss_out, first_iter);
  torch::Tensor v_ws = torch::empty({(int64_t)pb.fb, vnet.grand}, x.options());

  MLPBwdTwinArgs ta{};
  ta.pol = pb.ba;
  ta.gauss = pb.ga;
  ta.pol_ws = pb.ws.data_ptr<float>();
  ta.pol_loss_partials = pb.loss_partials.data_ptr<float>();
  ta.val = fill_bwd_args(x, v_weights, v_biases, v_acts, vnet, vnet.grand);
  ta.val_ws = v_ws.data_ptr<float>();
  ta.returns = returns.data_ptr<float>();
  ta.val_loss_partials = v_partials_out.data_ptr<float>();
  ta.x = x.data_ptr<float>();
  auto stream = current_stream();
  if (shaped) {
    launch_mlp_bwd_fused_twin_shaped(ta, pb.fb, stream);
  } else {
    launch_mlp_bwd_fused_twin(
        ta, std::max(pb.fused_lds, fused_bwd_lds(vnet, true)), pb.fb, stream);
  }
  HIP_OK(hipGetLastError());

  const ReduceAdamArgs vra = fill_reduce_adam(
      v_weights, v_biases, vnet, v_ws.data_ptr<float>(), vnet.grand, pb.fb,
      v_adam_m, v_adam_v, v_adam_step, v_lr, v_beta1, v_beta2, v_eps,
      v_weight_decay, v_step_delta, c10::nullopt);
  launch_mlp_grad_reduce_adam_twin(pb.ra, (long)pb.grand_ls, vra,
                                   (long)vnet.grand, stream);
  HIP_OK(hipGetLastError());
}

}  // namespace

void gaussian_ppo_value_twin_iter(
    torch::Tensor x, std::vector<torch::Tensor> weights,
    std::vector<torch::Tensor> biases, std::vector<int64_t> acts,
    torch::Tensor actions, torch::Tensor old_logp, torch::Tensor advantages,
    torch::Tensor log_std, double clip, std::vector<torch::Tensor> adam_m,
    std::vector<torch::Tensor> adam_v, torch::Tensor ls_m, torch::Tensor ls_v,
    torch::Tensor adam_step, double lr, double beta1, double beta2, double eps,
    double weight_decay, double step_delta, torch::Tensor gate,
    torch::Tensor kl_final, torch::Tensor iters_done, double thr,
    torch::Tensor loss_out, bool first_iter, torch::Tensor v_x,
    std::vector<torch::Tensor> v_weights, std::vector<torch::Tensor> v_biases,
    std::vector<int64_t> v_acts, torch::Tensor returns,
    torch::Tensor v_partials_out, std::vector<torch::Tensor> v_adam_m,
    std::vector<torch::Tensor> v_adam_v, torch::Tensor v_adam_step,
    double v_lr, double v_beta1, double v_beta2, double v_eps,
    double v_weight_decay, double v_step_delta) {
  ppo_value_twin_iter(
      PolicySeed{SEED_GAUSSIAN, &log_std, &ls_m, &ls_v}, x, weights, biases,
      acts, actions, old_logp, advantages, clip, adam_m, adam_v, adam_step, lr,
      beta1, beta2, eps, weight_decay, step_delta, gate, kl_final, iters_done,
      thr, loss_out, first_iter, v_x, v_weights, v_biases, v_acts, returns,
      v_partials_out, v_adam_m, v_adam_v, v_adam_step, v_lr, v_beta1, v_beta2,
      v_eps, v_weight_decay, v_step_delta);
}

void categorical_ppo_value_twin_iter(
    torch::Tensor x, std::vector<torch::Tensor> weights,
    std::vector<torch::Tensor> biases, std::vector<int64_t> acts,
    torch::Tensor actions, torch::Tensor old_logp, torch::Tensor advantages,
    double clip, std::vector<torch::Tensor> adam_m,
    std::vector<torch::Tensor> adam_v, torch::Tensor adam_step, double lr,
    double beta1, double beta2, double eps, double weight_decay,
    double step_delta, torch::Tensor gate, torch::Tensor kl_final,
    torch::Tensor iters_done, double thr, torch::Tensor loss_out,
    bool first_iter, torch::Tensor v_x, std::vector<torch::Tensor> v_weights,
    std::vector<torch::Tensor> v_biases, std::vector<int64_t> v_acts,
    torch::Tensor returns, torch::Tensor v_partials_out,
    std::vector<torch::Tensor> v_adam_m, std::vector<torch::Tensor> v_adam_v,
    torch::Tensor v_adam_step, double v_lr, double v_beta1, double v_beta2,
    double v_eps, double v_weight_decay, double v_step_delta) {
  ppo_value_twin_iter(
      PolicySeed{SEED_CATEGORICAL}, x, weights, biases, acts, actions,
      old_logp, advantages, clip, adam_m, adam_v, adam_step, lr, beta1, beta2,
      eps, weight_decay, step_delta, gate, kl_final, iters_done, thr, loss_out,
      first_iter, v_x, v_weights, v_biases, v_acts, returns, v_partials_out,
      v_adam_m, v_adam_v, v_adam_step, v_lr, v_beta1, v_beta2, v_eps,
      v_weight_decay, v_step_delta);
}

void counter_add_(torch::Tensor ctr, int64_t delta) {
  TORCH_CHECK(ctr.scalar_type() == torch::kInt64 && ctr.is_cuda() && ctr.numel() == 1,
              "ctr must be a 1-element int64 CUDA tensor");
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, current_stream(),
                     reinterpret_cast<unsigned long long*>(ctr.data_ptr<int64_t>()),
                     (unsigned long long)delta);
  HIP_OK(hipGetLastError());
}

// dims = [O, hidden..., A] of the policy net
int64_t ppo_rollout_fused_lds_bytes_py(std::vector<int64_t> dims, int64_t O,
                                       int64_t A) {
  const NetLayout n = net_layout(dims, ROLLOUT_MAX_WIDTH);
  return (int64_t)ppo_rollout_fused_lds_bytes(n, (int)O, (int)A);
}

// whole-epoch rollout in one launch (rollout_fused_kernels.hip): writes
// obs_full[0..steps], act_buf, rew_buf and cut_final[j] for cuts[j];
// reads the RNG counter, never advances it (counter_add_ follows)
void ppo_rollout_fused(std::vector<torch::Tensor> weights,
                       std::vector<torch::Tensor> biases,
                       std::vector<int64_t> acts, torch::Tensor log_std,
                       torch::Tensor envA, torch::Tensor envB, torch::Tensor envw,
                       double sigma, int64_t policy_seed, int64_t env_seed,
                       std::vector<int64_t> cuts, bool start_with_reset,
                       torch::Tensor ctr, torch::Tensor obs_full,
                       torch::Tensor act_buf, torch::Tensor rew_buf,
                       torch::Tensor cut_final) {
  check_f32_gpu(obs_full, "obs_full");
  check_f32_gpu(act_buf, "act_buf");
  check_f32_gpu(rew_buf, "rew_buf");
  check_f32_gpu(cut_final, "cut_final");
  check_f32_gpu(log_std, "log_std");
  check_f32_gpu(envA, "env A");
  check_f32_gpu(envB, "env B");
  check_f32_gpu(envw, "env w");
  TORCH_CHECK(obs_full.dim() == 3 && obs_full.size(0) >= 2, "obs_full must be [steps+1, N, O]");
  RolloutFusedArgs a{};
  a.steps = (int)obs_full.size(0) - 1;
  a.N = (int)obs_full.size(1);
  a.O = (int)obs_full.size(2);
  a.A = (int)log_std.numel();
  TORCH_CHECK(a.N >= 1 && a.O >= 1 && a.O <= ROLLOUT_MAX_WIDTH && a.A >= 1 &&
                  a.A <= ROLLOUT_MAX_WIDTH,
              "ppo_rollout_fused: obs/action dims must be in [1, ", ROLLOUT_MAX_WIDTH, "]");
  TORCH_CHECK(act_buf.dim() == 3 && act_buf.size(0) == a.steps &&
                  act_buf.size(1) == a.N && act_buf.size(2) == a.A,
              "act_buf must be [steps, N, A]");
  TORCH_CHECK(rew_buf.dim() == 2 && rew_buf.size(0) == a.steps && rew_buf.size(1) == a.N,
              "rew_buf must be [steps, N]");
  TORCH_CHECK(envA.dim() == 2 && envA.size(0) == a.O && envA.size(1) == a.O &&
                  envB.dim() == 2 && envB.size(0) == a.A && envB.size(1) == a.O &&
                  envw.numel() == a.O,
              "env matrices must be A[O,O], B[A,O], w[O]");
  const NetLayout net = net_layout(a.O, weights, biases, acts, ROLLOUT_MAX_WIDTH);
  fill_net(a, net, weights, biases, acts);
  const int L = net.L;
  TORCH_CHECK(a.dims[L] == a.A, "policy head width must equal the action dim");
  TORCH_CHECK(ppo_rollout_fused_lds_bytes(net, a.O, a.A) <= MLP_LDS_BUDGET,
              "ppo_rollout_fused: net + env image exceeds the LDS budget");
  fill_cuts(a, cuts, a.steps, "ppo_rollout_fused");
  TORCH_CHECK(cut_final.dim() == 3 && cut_final.size(0) >= std::max(a.n_cuts, 1) &&
                  cut_final.size(1) == a.N && cut_final.size(2) == a.O,
              "cut_final must be [n_cuts, N, O]");
  a.log_std = log_std.data_ptr<float>();
  a.envA = envA.data_ptr<float>();
  a.envB = envB.data_ptr<float>();
  a.envw = envw.data_ptr<float>();
  a.obs_full = obs_full.data_ptr<float>();
  a.act_buf = act_buf.data_ptr<float>();
  a.rew_buf = rew_buf.data_ptr<float>();
  a.cut_final = cut_final.data_ptr<float>();
  a.ctr = ctr_ptr(c10::optional<torch::Tensor>(ctr));
  a.start_with_reset = start_with_reset ? 1 : 0;
  a.sigma = (float)sigma;
  a.policy_seed = (uint64_t)policy_seed;
  a.env_seed = (uint64_t)env_seed;
  launch_ppo_rollout_fused(a, current_stream());
  HIP_OK(hipGetLastError());
}

// dims = [4, hidden..., n_act] of the policy net
int64_t cartpole_rollout_fused_lds_bytes_py(std::vector<int64_t> dims) {
  const NetLayout n = net_layout(dims, ROLLOUT_MAX_WIDTH);
  return (int64_t)persistent_lds_bytes(n);
}

// whole-epoch CartPole rollout in one launch (cartpole_rollout_kernels.hip):
// writes obs_full[0..steps], final_obs, act_buf, rew_buf, done_buf and the
// env carry; reads the RNG counter, never advances it (counter_add_ follows)
void cartpole_rollout_fused(std::vector<torch::Tensor> weights,
                            std::vector<torch::Tensor> biases,
                            std::vector<int64_t> acts, int64_t policy_seed,
                            int64_t env_seed, int64_t max_steps,
                            bool start_with_reset, torch::Tensor ctr,
                            torch::Tensor state, torch::Tensor elapsed,
                            torch::Tensor obs_full, torch::Tensor final_obs,
                            torch::Tensor act_buf, torch::Tensor rew_buf,
                            torch::Tensor done_buf) {
  const NetLayout net = net_layout(4, weights, biases, acts, ROLLOUT_MAX_WIDTH);
  CartPoleRolloutArgs a{};
  a.N = check_cartpole_carry(state, elapsed);
  check_f32_gpu(obs_full, "obs_full");
  TORCH_CHECK(obs_full.dim() == 3 && obs_full.size(0) >= 2 &&
                  obs_full.size(1) == a.N && obs_full.size(2) == 4,
              "obs_full must be [steps+1, N, 4]");
  a.steps = (int)obs_full.size(0) - 1;
  const int64_t SN = (int64_t)a.steps * a.N;
  check_out(final_obs, torch::kFloat32, SN * 4, "final_obs");
  check_out(act_buf, torch::kInt64, SN, "act_buf");
  check_out(rew_buf, torch::kFloat32, SN, "rew_buf");
  check_out(done_buf, torch::kUInt8, SN, "done_buf");
  fill_net(a, net, weights, biases, acts);
  TORCH_CHECK(persistent_lds_bytes(net) <= DEFAULT_LDS_LIMIT,
              "cartpole_rollout_fused: net image exceeds the LDS budget");
  a.state = state.data_ptr<double>();
  a.elapsed = elapsed.data_ptr<int>();
  a.obs_full = obs_full.data_ptr<float>();
  a.final_obs = final_obs.data_ptr<float>();
  a.act_buf = reinterpret_cast<long long*>(act_buf.data_ptr<int64_t>());
  a.rew_buf = rew_buf.data_ptr<float>();
  a.done_buf = done_buf.data_ptr<uint8_t>();
  a.ctr = ctr_ptr(c10::optional<torch::Tensor>(ctr));
  a.max_steps = (int)max_steps;
  a.start_with_reset = start_with_reset ? 1 : 0;
  a.policy_seed = (uint64_t)policy_seed;
  a.env_seed = (uint64_t)env_seed;
  launch_cartpole_rollout_fused(a, current_stream());
  HIP_OK(hipGetLastError());
}

// dims = [3, hidden..., 1] of the policy net
int64_t pendulum_rollout_fused_lds_bytes_py(std::vector<int64_t> dims) {
  const NetLayout n = net_layout(dims, ROLLOUT_MAX_WIDTH);
  return (int64_t)persistent_lds_bytes(n);
}

// whole-epoch Pendulum rollout in one launch (pendulum_rollout_kernels.hip):
// writes obs_full[0..steps], act_buf, rew_buf, cut_final[j] for cuts[j] and
// the env carry; reads the RNG counter, never advances it (counter_add_
// follows)
void pendulum_rollout_fused(std::vector<torch::Tensor> weights,
                            std::vector<torch::Tensor> biases,
                            std::vector<int64_t> acts, torch::Tensor log_std,
                            int64_t policy_seed, int64_t env_seed,
                            std::vector<int64_t> cuts, bool start_with_reset,
                            torch::Tensor ctr, torch::Tensor state,
                            torch::Tensor obs_full, torch::Tensor act_buf,
                            torch::Tensor rew_buf, torch::Tensor cut_final) {
  const NetLayout net = net_layout(3, weights, biases, acts, ROLLOUT_MAX_WIDTH);
  const int L = net.L;
  PendulumRolloutArgs a{};
  a.N = check_pendulum_carry(state);
  TORCH_CHECK(net.dims[L] == 1, "pendulum_rollout_fused: the policy head must be 1 wide");
  check_f32_gpu(log_std, "log_std");
  TORCH_CHECK(log_std.numel() == 1, "pendulum_rollout_fused: log_std must have 1 element");
  check_f32_gpu(obs_full, "obs_full");
  TORCH_CHECK(obs_full.dim() == 3 && obs_full.size(0) >= 2 &&
                  obs_full.size(1) == a.N && obs_full.size(2) == 3,
              "obs_full must be [steps+1, N, 3]");
  a.steps = (int)obs_full.size(0) - 1;
  const int64_t SN = (int64_t)a.steps * a.N;
  check_out(act_buf, torch::kFloat32, SN, "act_buf");
  check_out(rew_buf, torch::kFloat32, SN, "rew_buf");
  fill_cuts(a, cuts, a.steps, "pendulum_rollout_fused");
  check_f32_gpu(cut_final, "cut_final");
  TORCH_CHECK(cut_final.dim() == 3 && cut_final.size(0) >= std::max(a.n_cuts, 1) &&
                  cut_final.size(1) == a.N && cut_final.size(2) == 3,
              "cut_final must be [n_cuts, N, 3]");
  fill_net(a, net, weights, biases, acts);
  TORCH_CHECK(persistent_lds_bytes(net) <= DEFAULT_LDS_LIMIT,
              "pendulum_rollout_fused: net image exceeds the LDS budget");
  a.ctr = ctr_ptr(c10::optional<torch::Tensor>(ctr));
  a.log_std = log_std.data_ptr<float>();
  a.state = state.data_ptr<double>();
  a.obs_full = obs_full.data_ptr<float>();
  a.act_buf = act_buf.data_ptr<float>();
  a.rew_buf = rew_buf.data_ptr<float>();
  a.cut_final = cut_final.data_ptr<float>();
  a.start_with_reset = start_with_reset ? 1 : 0;
  a.policy_seed = (uint64_t)policy_seed;
  a.env_seed = (uint64_t)env_seed;
  launch_pendulum_rollout_fused(a, current_stream());
  HIP_OK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Replay collection: device-side ring writes
// ---------------------------------------------------------------------------
// The replay ring handed to a collect kernel: storage = [observations [cap,O],
// actions [cap,A], rewards [cap], next_observations [cap,O], dones [cap]],
// all contiguous fp32 on `dev`, both scalars 1-element int64 there, and room
// for the epoch's n transitions without a slot written twice.  O and A are
// the storage tensors' own floats per slot, which must be the caller's.
static ReplayRing check_ring(const std::vector<torch::Tensor>& storage,
                             const torch::Tensor& write_dev,
                             const torch::Tensor& size_dev, int64_t n,
                             const torch::Device& dev, int64_t O, int64_t A) {
  TORCH_CHECK(storage.size() == 5,
              "ring storage must be [obs, act, rew, next_obs, dones]");
  static const char* names[5] = {"ring observations", "ring actions", "ring rewards",
                                 "ring next_observations", "ring dones"};
  for (int i = 0; i < 5; ++i) {
    check_f32_gpu(storage[i], names[i]);
    TORCH_CHECK(storage[i].device() == dev, names[i], " is on another device");
    TORCH_CHECK(storage[i].dim() >= 1, names[i], " must have a slot dimension");
  }
  const int64_t cap = storage[2].numel();
  TORCH_CHECK(cap >= 1, "empty ring");
  const int64_t ring_O = storage[0].numel() / cap, ring_A = storage[1].numel() / cap;
  TORCH_CHECK(ring_O == O && ring_A == A, "the ring holds ", ring_O,
              "-wide observations and ", ring_A, "-wide actions, the epoch's are ", O,
              " and ", A, " wide");
  const int64_t per_slot[5] = {O, A, 1, O, 1};
  for (int i = 0; i < 5; ++i)
    TORCH_CHECK(storage[i].size(0) == cap && storage[i].numel() == cap * per_slot[i],
                names[i], " must hold ", per_slot[i], " floats per ring slot");
  for (const torch::Tensor* s : {&write_dev, &size_dev})
    TORCH_CHECK(s->scalar_type() == torch::kInt64 && s->is_cuda() &&
                    s->numel() == 1 && s->device() == dev,
                "ring scalars must be 1-element int64 tensors on the ring's device");
  TORCH_CHECK(n >= 1 && n <= cap, "an epoch of ", n,
              " transitions does not fit a ring of ", cap);
  ReplayRing r{};
  r.obs = storage[0].data_ptr<float>();
  r.act = storage[1].data_ptr<float>();
  r.rew = storage[2].data_ptr<float>();
  r.nxt = storage[3].data_ptr<float>();
  r.dn = storage[4].data_ptr<float>();
  r.write = reinterpret_cast<const long long*>(write_dev.data_ptr<int64_t>());
  r.cap = (unsigned long long)cap;
  r.O = (int)O;
  r.A = (int)A;
  return r;
}

// segments of a lockstep epoch: one per cut, plus the open one when the
// last step is no cut
static int epoch_segments(const std::vector<int64_t>& cuts, int64_t steps) {
  return (int)cuts.size() + ((cuts.empty() || cuts.back() != steps - 1) ? 1 : 0);
}

// dims = [3, hidden..., 1] of the actor
int64_t pendulum_collect_fused_lds_bytes_py(std::vector<int64_t> dims) {
  const NetLayout n = net_layout(dims, MLP_MAX_WIDTH);
  return (int64_t)persistent_lds_bytes(n);
}

// whole-epoch Pendulum replay collection in one launch
// (pendulum_collect_kernels.hip): writes the epoch's N * steps transitions
// into the ring at the device-held write position, seg_returns, last_obs and
// the env carry; reads the RNG counter and the ring scalars, never advances
// them (ring_advance_ and counter_add_ follow).  mode COLLECT_UNIFORM takes
// no net.  wide_threads: workgroup size of the wide regime, 256 or 1024.
void pendulum_collect_fused(std::vector<torch::Tensor> weights,
                            std::vector<torch::Tensor> biases,
                            std::vector<int64_t> acts, int64_t mode,
                            double noise_scale, double limit, double low,
                            double high, int64_t action_seed, int64_t env_seed,
                            std::vector<int64_t> cuts, bool start_with_reset,
                            torch::Tensor ctr, torch::Tensor state, int64_t steps,
                            std::vector<torch::Tensor> storage,
                            torch::Tensor write_dev, torch::Tensor size_dev,
                            torch::Tensor seg_returns, torch::Tensor last_obs,
                            int64_t wide_threads) {
  PendulumCollectArgs a{};
  a.N = check_pendulum_carry(state);
  a.steps = check_step_count(steps, "steps");
  a.ring = check_ring(storage, write_dev, size_dev, (int64_t)a.N * steps,
                      state.device(), 3, 1);
  TORCH_CHECK(mode == COLLECT_NOISED || mode == COLLECT_UNIFORM, "unknown mode");
  a.mode = (int)mode;
  NetLayout net;  // no layers in uniform mode
  if (mode == COLLECT_NOISED) {
    net = net_layout(3, weights, biases, acts, MLP_MAX_WIDTH);
    TORCH_CHECK(net.dims[net.L] == 1,
                "pendulum_collect_fused: the actor head must be 1 wide");
    check_net_device(weights, biases, state.device());
    TORCH_CHECK(noise_scale >= 0.0 && limit >= 0.0,
                "pendulum_collect_fused: noise_scale and limit must be >= 0");
    fill_net(a, net, weights, biases, acts);
  } else {
    TORCH_CHECK(weights.empty() && biases.empty() && acts.empty(),
                "pendulum_collect_fused: uniform mode takes no net");
    TORCH_CHECK(low <= high, "pendulum_collect_fused: low > high");
  }
  TORCH_CHECK(persistent_lds_bytes(net) <= MLP_LDS_BUDGET,
              "pendulum_collect_fused: net image exceeds the LDS budget");
  TORCH_CHECK(wide_threads == 256 || wide_threads == 1024,
              "pendulum_collect_fused: wide_threads must be 256 or 1024");
  fill_cuts(a, cuts, steps, "pendulum_collect_fused");
  a.n_segs = epoch_segments(cuts, steps);
  check_out(seg_returns, torch::kFloat32, (int64_t)a.N * a.n_segs, "seg_returns");
  check_out(last_obs, torch::kFloat32, (int64_t)a.N * 3, "last_obs");
  TORCH_CHECK(seg_returns.device() == state.device() &&
                  last_obs.device() == state.device(),
              "seg_returns / last_obs are on another device");
  a.ctr = ctr_ptr(c10::optional<torch::Tensor>(ctr));
  a.state = state.data_ptr<double>();
  a.seg_returns = seg_returns.data_ptr<float>();
  a.last_obs = last_obs.data_ptr<float>();
  a.start_with_reset = start_with_reset ? 1 : 0;
  a.noise_scale = (float)noise_scale;
  a.limit = (float)limit;
  a.low = (float)low;
  a.high = (float)high;
  a.action_seed = (uint64_t)action_seed;
  a.env_seed = (uint64_t)env_seed;
  launch_pendulum_collect_fused(a, (int)wide_threads, current_stream());
  HIP_OK(hipGetLastError());
}

static size_t synthetic_collect_lds_bytes(const NetLayout& n, int O, int A) {
  return (size_t)synthetic_collect_lds_floats(n.dims, n.L, O, A) * sizeof(float);
}

// dims = [O, hidden..., A] of the actor; empty for the uniform draw
int64_t synthetic_collect_fused_lds_bytes_py(std::vector<int64_t> dims, int64_t O,
                                             int64_t A) {
  TORCH_CHECK(O >= 1 && O <= ROLLOUT_MAX_WIDTH && A >= 1 && A <= ROLLOUT_MAX_WIDTH,
              "synthetic_collect_fused: obs/action dims must be in [1, ",
              ROLLOUT_MAX_WIDTH, "]");
  NetLayout n;
  if (!dims.empty()) n = net_layout(dims, MLP_MAX_WIDTH);
  return (int64_t)synthetic_collect_lds_bytes(n, (int)O, (int)A);
}

// whole-epoch replay collection on a synthetic env in one launch
// (synthetic_collect_kernels.hip): writes the epoch's N * steps transitions
// into the ring at the device-held write position, seg_returns and the carry
// [N, O]; reads the RNG counter and the ring scalars, never advances them
// (ring_advance_ and counter_add_ follow).  mode COLLECT_UNIFORM takes no
// net.  wide_threads: workgroup size of the wide regime, 256 or 1024.
void synthetic_collect_fused(std::vector<torch::Tensor> weights,
                             std::vector<torch::Tensor> biases,
                             std::vector<int64_t> acts, int64_t mode,
                             double noise_scale, double limit, double low,
                             double high, int64_t action_seed, int64_t env_seed,
                             torch::Tensor envA, torch::Tensor envB,
                             torch::Tensor envw, double sigma,
                             std::vector<int64_t> cuts, bool start_with_reset,
                             torch::Tensor ctr, torch::Tensor carry, int64_t steps,
                             std::vector<torch::Tensor> storage,
                             torch::Tensor write_dev, torch::Tensor size_dev,
                             torch::Tensor seg_returns, int64_t wide_threads) {
  check_f32_gpu(carry, "carry");
  check_f32_gpu(envA, "env A");
  check_f32_gpu(envB, "env B");
  check_f32_gpu(envw, "env w");
  TORCH_CHECK(carry.dim() == 2 && carry.size(0) >= 1, "carry must be [N, O]");
  TORCH_CHECK(envB.dim() == 2, "env B must be [A, O]");
  SyntheticCollectArgs a{};
  a.N = (int)carry.size(0);
  a.O = (int)carry.size(1);
  a.A = (int)envB.size(0);
  TORCH_CHECK(a.O >= 1 && a.O <= ROLLOUT_MAX_WIDTH && a.A >= 1 &&
                  a.A <= ROLLOUT_MAX_WIDTH,
              "synthetic_collect_fused: obs/action dims must be in [1, ",
              ROLLOUT_MAX_WIDTH, "]");
  TORCH_CHECK(envA.dim() == 2 && envA.size(0) == a.O && envA.size(1) == a.O &&
                  envB.size(1) == a.O && envw.dim() == 1 && envw.numel() == a.O,
              "env matrices must be A[O,O], B[A,O], w[O]");
  for (const torch::Tensor* t : {&envA, &envB, &envw})
    TORCH_CHECK(t->device() == carry.device(), "the env matrices are on another device");
  a.steps = check_step_count(steps, "steps");
  a.ring = check_ring(storage, write_dev, size_dev, (int64_t)a.N * steps,
                      carry.device(), a.O, a.A);
  TORCH_CHECK(mode == COLLECT_NOISED || mode == COLLECT_UNIFORM, "unknown mode");
  a.mode = (int)mode;
  NetLayout net;  // no layers in uniform mode
  if (mode == COLLECT_NOISED) {
    net = net_layout(a.O, weights, biases, acts, MLP_MAX_WIDTH);
    TORCH_CHECK(net.dims[net.L] == a.A,
                "synthetic_collect_fused: the actor head width must equal the action dim");
    check_net_device(weights, biases, carry.device());
    TORCH_CHECK(noise_scale >= 0.0 && limit >= 0.0,
                "synthetic_collect_fused: noise_scale and limit must be >= 0");
    fill_net(a, net, weights, biases, acts);
  } else {
    TORCH_CHECK(weights.empty() && biases.empty() && acts.empty(),
                "synthetic_collect_fused: uniform mode takes no net");
    TORCH_CHECK(low <= high, "synthetic_collect_fused: low > high");
  }
  TORCH_CHECK(synthetic_collect_lds_bytes(net, a.O, a.A) <= MLP_LDS_BUDGET,
              "synthetic_collect_fused: net + env image exceeds the LDS budget");
  TORCH_CHECK(wide_threads == 256 || wide_threads == 1024,
              "synthetic_collect_fused: wide_threads must be 256 or 1024");
  fill_cuts(a, cuts, steps, "synthetic_collect_fused");
  a.n_segs = epoch_segments(cuts, steps);
  check_out(seg_returns, torch::kFloat32, (int64_t)a.N * a.n_segs, "seg_returns");
  TORCH_CHECK(seg_returns.device() == carry.device(),
              "seg_returns is on another device");
  a.ctr = ctr_ptr(c10::optional<torch::Tensor>(ctr));
  a.envA = envA.data_ptr<float>();
  a.envB = envB.data_ptr<float>();
  a.envw = envw.data_ptr<float>();
  a.carry = carry.data_ptr<float>();
  a.seg_returns = seg_returns.data_ptr<float>();
  a.start_with_reset = start_with_reset ? 1 : 0;
  a.noise_scale = (float)noise_scale;
  a.limit = (float)limit;
  a.low = (float)low;
  a.high = (float)high;
  a.sigma = (float)sigma;
  a.action_seed = (uint64_t)action_seed;
  a.env_seed = (uint64_t)env_seed;
  launch_synthetic_collect_fused(a, (int)wide_threads, current_stream());
  HIP_OK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// one pass over a PPO epoch's rows (ppo_ingest_kernels.hip)
// ---------------------------------------------------------------------------
static size_t ppo_ingest_lds_bytes(const NetLayout& v, const NetLayout& p) {
  return (size_t)ppo_ingest_lds_floats(v.dims, v.L, p.dims, p.L) * sizeof(float);
}

// vdims / pdims = [obs, hidden..., 1] / [obs, hidden..., act_dim]
int64_t ppo_ingest_rows_lds_bytes_py(std::vector<int64_t> vdims,
                                     std::vector<int64_t> pdims) {
  return (int64_t)ppo_ingest_lds_bytes(net_layout(vdims, ROLLOUT_MAX_WIDTH),
                                       net_layout(pdims, ROLLOUT_MAX_WIDTH));
}

// Reads the epoch's tensors (observations [T, O], last_observations [E, O],
// actions [T, A], rewards [T], offsets int32 [E + 1], dones int32 [E]) once
// and writes the update graph's buffers: the copies obs_out / act_out /
// rew_out / off_out / dones_out, values_all [T + E] from the value net,
// logp_now [T] from the policy and old_logp [T] from the old policy (which
// has the policy's shape and activations).
void ppo_ingest_rows(torch::Tensor observations, torch::Tensor last_observations,
                     torch::Tensor actions, torch::Tensor rewards,
                     torch::Tensor offsets, torch::Tensor dones,
                     std::vector<torch::Tensor> vweights,
                     std::vector<torch::Tensor> vbiases, std::vector<int64_t> vacts,
                     std::vector<torch::Tensor> pweights,
                     std::vector<torch::Tensor> pbiases, std::vector<int64_t> pacts,
                     torch::Tensor log_std, std::vector<torch::Tensor> oweights,
                     std::vector<torch::Tensor> obiases, torch::Tensor old_log_std,
                     torch::Tensor obs_out, torch::Tensor act_out,
                     torch::Tensor rew_out, torch::Tensor off_out,
                     torch::Tensor dones_out, torch::Tensor values_all,
                     torch::Tensor old_logp, torch::Tensor logp_now) {
  PPOIngestArgs a{};
  const NetLayout pnet =
      net_layout(observations, pweights, pbiases, pacts, ROLLOUT_MAX_WIDTH);
  const NetLayout onet =
      net_layout(observations, oweights, obiases, pacts, ROLLOUT_MAX_WIDTH);
  const NetLayout vnet =
      net_layout(observations, vweights, vbiases, vacts, ROLLOUT_MAX_WIDTH);
  TORCH_CHECK(onet.L == pnet.L, "the old policy must have the policy's shape");
  for (int l = 0; l <= pnet.L; ++l)
    TORCH_CHECK(onet.dims[l] == pnet.dims[l], "the old policy must have the policy's shape");
  TORCH_CHECK(vnet.dims[vnet.L] == 1, "ppo_ingest_rows: the value head must be 1 wide");
  const torch::Device dev = observations.device();
  check_net_device(pweights, pbiases, dev);
  check_net_device(oweights, obiases, dev);
  check_net_device(vweights, vbiases, dev);
  TORCH_CHECK(ppo_ingest_lds_bytes(vnet, pnet) <= MLP_LDS_BUDGET,
              "ppo_ingest_rows: net images exceed the LDS budget");

  const int64_t T = observations.size(0), O = observations.size(1);
  const int64_t A = pnet.dims[pnet.L];
  check_f32_gpu(last_observations, "last_observations");
  TORCH_CHECK(last_observations.dim() == 2 && last_observations.size(1) == O,
              "last_observations must be [E, O]");
  const int64_t E = last_observations.size(0);
  TORCH_CHECK(T >= 1 && E >= 1 && T + E < (1LL << 24), "row count out of range");
  for (const torch::Tensor* t : {&actions, &rewards, &log_std, &old_log_std})
    check_f32_gpu(*t, "actions / rewards / log_std");
  TORCH_CHECK(actions.numel() == T * A && rewards.numel() == T,
              "actions must be [T, A] and rewards [T]");
  TORCH_CHECK(log_std.numel() == A && old_log_std.numel() == A, "log_std must be [A]");
  check_out(offsets, torch::kInt32, E + 1, "offsets");
  check_out(dones, torch::kInt32, E, "dones");
  check_out(obs_out, torch::kFloat32, T * O, "obs_out");
  check_out(act_out, torch::kFloat32, T * A, "act_out");
  check_out(rew_out, torch::kFloat32, T, "rew_out");
  check_out(off_out, torch::kInt32, E + 1, "off_out");
  check_out(dones_out, torch::kInt32, E, "dones_out");
  check_out(values_all, torch::kFloat32, T + E, "values_all");
  check_out(old_logp, torch::kFloat32, T, "old_logp");
  check_out(logp_now, torch::kFloat32, T, "logp_now");
  for (const torch::Tensor* t :
       {&last_observations, &actions, &rewards, &offsets, &dones, &log_std,
        &old_log_std, &obs_out, &act_out, &rew_out, &off_out, &dones_out,
        &values_all, &old_logp, &logp_now})
    TORCH_CHECK(t->device() == dev, "ppo_ingest_rows: tensors on different devices");

  fill_net(a.val, vnet, vweights, vbiases, vacts);
  fill_net(a.pol, pnet, pweights, pbiases, pacts);
  fill_net(a.old, onet, oweights, obiases, pacts);
  a.obs = observations.data_ptr<float>();
  a.last_obs = last_observations.data_ptr<float>();
  a.actions = actions.data_ptr<float>();
  a.rewards = rewards.data_ptr<float>();
  a.offsets = offsets.data_ptr<int>();
  a.dones = dones.data_ptr<int>();
  a.log_std = log_std.data_ptr<float>();
  a.old_log_std = old_log_std.data_ptr<float>();
  a.obs_out = obs_out.data_ptr<float>();
  a.act_out = act_out.data_ptr<float>();
  a.rew_out = rew_out.data_ptr<float>();
  a.off_out = off_out.data_ptr<int>();
  a.dones_out = dones_out.data_ptr<int>();
  a.values_all = values_all.data_ptr<float>();
  a.old_logp = old_logp.data_ptr<float>();
  a.logp_now = logp_now.data_ptr<float>();
  a.T = (int)T;
  a.E = (int)E;
  a.O = (int)O;
  a.A = (int)A;
  launch_ppo_ingest_rows(a, current_stream());
  HIP_OK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// GPU-resident policy evaluation (eval_kernels.hip)
// ---------------------------------------------------------------------------
// the per-episode outputs of an evaluation: returns fp64 [N], lengths int32
// [N], init_state fp64 [N, state_dim], all contiguous on one GPU.  -> N
static int check_eval_outputs(const torch::Tensor& returns,
                              const torch::Tensor& lengths,
                              const torch::Tensor& init_state, int state_dim) {
  TORCH_CHECK(returns.is_cuda() && returns.is_contiguous() &&
                  returns.scalar_type() == torch::kFloat64 && returns.dim() == 1 &&
                  returns.size(0) >= 1,
              "returns must be a contiguous float64 CUDA tensor [N]");
  const int64_t N = returns.size(0);
  TORCH_CHECK(N < (1LL << 24), "too many episodes");
  TORCH_CHECK(lengths.is_cuda() && lengths.is_contiguous() &&
                  lengths.scalar_type() == torch::kInt32 && lengths.dim() == 1 &&
                  lengths.size(0) == N,
              "lengths must be a contiguous int32 CUDA tensor [N]");
  TORCH_CHECK(init_state.is_cuda() && init_state.is_contiguous() &&
                  init_state.scalar_type() == torch::kFloat64 &&
                  init_state.dim() == 2 && init_state.size(0) == N &&
                  init_state.size(1) == state_dim,
              "init_state must be a contiguous float64 CUDA tensor [N, ", state_dim, "]");
  TORCH_CHECK(lengths.device() == returns.device() &&
                  init_state.device() == returns.device(),
              "returns / lengths / init_state are on different devices");
  return (int)N;
}

// the two device counters of an evaluation, on the outputs' device
static void check_eval_counters(const torch::Tensor& ctr, const torch::Tensor& reset_ctr,
                                const torch::Device& dev) {
  for (const torch::Tensor* c : {&ctr, &reset_ctr})
    TORCH_CHECK(c->scalar_type() == torch::kInt64 && c->is_cuda() && c->numel() == 1 &&
                    c->device() == dev,
                "ctr / reset_ctr must be 1-element int64 tensors on the outputs' device");
}

// dims = [3, hidden..., 1] of the policy net
int64_t pendulum_eval_fused_lds_bytes_py(std::vector<int64_t> dims) {
  const NetLayout n = net_layout(dims, MLP_MAX_WIDTH);
  return (int64_t)persistent_lds_bytes(n);
}

// dims = [4, hidden..., n_act] of the policy net
int64_t cartpole_eval_fused_lds_bytes_py(std::vector<int64_t> dims) {
  const NetLayout n = net_layout(dims, ROLLOUT_MAX_WIDTH);
  return (int64_t)persistent_lds_bytes(n);
}

// N whole Pendulum episodes of `horizon` steps in one launch
// (eval_kernels.hip): writes returns, lengths and init_state; reads both
// counters, never advances them (counter_add_ follows).  mode
// EVAL_DETERMINISTIC takes no log_std.  wide_threads: workgroup size of the
// wide regime, 256 or 1024.
void pendulum_eval_fused(std::vector<torch::Tensor> weights,
                         std::vector<torch::Tensor> biases,
                         std::vector<int64_t> acts, int64_t mode,
                         c10::optional<torch::Tensor> log_std, int64_t policy_seed,
                         int64_t env_seed, int64_t horizon, torch::Tensor ctr,
                         torch::Tensor reset_ctr, torch::Tensor returns,
                         torch::Tensor lengths, torch::Tensor init_state,
                         int64_t wide_threads) {
  PendulumEvalArgs a{};
  a.N = check_eval_outputs(returns, lengths, init_state, 2);
  check_eval_counters(ctr, reset_ctr, returns.device());
  a.horizon = check_step_count(horizon, "horizon");
  TORCH_CHECK(mode == EVAL_DETERMINISTIC || mode == EVAL_GAUSSIAN, "unknown mode");
  a.mode = (int)mode;
  const NetLayout net = net_layout(3, weights, biases, acts, MLP_MAX_WIDTH);
  TORCH_CHECK(net.dims[net.L] == 1, "pendulum_eval_fused: the policy head must be 1 wide");
  check_net_device(weights, biases, returns.device());
  if (mode == EVAL_GAUSSIAN) {
    TORCH_CHECK(log_std.has_value(), "pendulum_eval_fused: Gaussian mode needs log_std");
    check_f32_gpu(*log_std, "log_std");
    TORCH_CHECK(log_std->numel() == 1 && log_std->device() == returns.device(),
                "pendulum_eval_fused: log_std must have 1 element on the outputs' device");
    a.log_std = log_std->data_ptr<float>();
  }
  fill_net(a, net, weights, biases, acts);
  TORCH_CHECK(persistent_lds_bytes(net) <= DEFAULT_LDS_LIMIT,
              "pendulum_eval_fused: net image exceeds the LDS budget");
  TORCH_CHECK(wide_threads == 256 || wide_threads == 1024,
              "pendulum_eval_fused: wide_threads must be 256 or 1024");
  a.returns = returns.data_ptr<double>();
  a.lengths = lengths.data_ptr<int>();
  a.init_state = init_state.data_ptr<double>();
  a.ctr = ctr_ptr(c10::optional<torch::Tensor>(ctr));
  a.reset_ctr = ctr_ptr(c10::optional<torch::Tensor>(reset_ctr));
  a.policy_seed = (uint64_t)policy_seed;
  a.env_seed = (uint64_t)env_seed;
  launch_pendulum_eval_fused(a, (int)wide_threads, current_stream());
  HIP_OK(hipGetLastError());
}

// N whole CartPole episodes of at most `horizon` steps in one launch
// (eval_kernels.hip): writes returns, lengths and init_state; reads both
// counters, never advances them (counter_add_ follows).  Narrow nets only.
void cartpole_eval_fused(std::vector<torch::Tensor> weights,
                         std::vector<torch::Tensor> biases,
                         std::vector<int64_t> acts, int64_t policy_seed,
                         int64_t env_seed, int64_t horizon, torch::Tensor ctr,
                         torch::Tensor reset_ctr, torch::Tensor returns,
                         torch::Tensor lengths, torch::Tensor init_state) {
  CartPoleEvalArgs a{};
  a.N = check_eval_outputs(returns, lengths, init_state, 4);
  check_eval_counters(ctr, reset_ctr, returns.device());
  a.horizon = check_step_count(horizon, "horizon");
  const NetLayout net = net_layout(4, weights, biases, acts, ROLLOUT_MAX_WIDTH);
  check_net_device(weights, biases, returns.device());
  fill_net(a, net, weights, biases, acts);
  TORCH_CHECK(persistent_lds_bytes(net) <= DEFAULT_LDS_LIMIT,
              "cartpole_eval_fused: net image exceeds the LDS budget");
  a.returns = returns.data_ptr<double>();
  a.lengths = lengths.data_ptr<int>();
  a.init_state = init_state.data_ptr<double>();
  a.ctr = ctr_ptr(c10::optional<torch::Tensor>(ctr));
  a.reset_ctr = ctr_ptr(c10::optional<torch::Tensor>(reset_ctr));
  a.policy_seed = (uint64_t)policy_seed;
  a.env_seed = (uint64_t)env_seed;
  launch_cartpole_eval_fused(a, current_stream());
  HIP_OK(hipGetLastError());
}

// first-episode return (fp64) and length (int32) of each row of rew_buf
// [steps, N]: up to and including the first step done_buf [steps, N] (uint8)
// marks, or all steps without one
void episode_reduce(torch::Tensor rew_buf, c10::optional<torch::Tensor> done_buf,
                    torch::Tensor returns, torch::Tensor lengths) {
  check_f32_gpu(rew_buf, "rew_buf");
  TORCH_CHECK(rew_buf.dim() == 2 && rew_buf.size(0) >= 1 && rew_buf.size(1) >= 1 &&
                  rew_buf.size(0) <= (1 << 24) && rew_buf.size(1) < (1 << 24),
              "rew_buf must be [steps, N]");
  const int steps = (int)rew_buf.size(0);
  const int N = (int)rew_buf.size(1);
  const unsigned char* dn = nullptr;
  if (done_buf.has_value()) {
    check_out(*done_buf, torch::kUInt8, (int64_t)steps * N, "done_buf");
    TORCH_CHECK(done_buf->device() == rew_buf.device(), "episode_reduce: mixed devices");
    dn = done_buf->data_ptr<uint8_t>();
  }
  check_out(returns, torch::kFloat64, N, "returns");
  check_out(lengths, torch::kInt32, N, "lengths");
  TORCH_CHECK(returns.device() == rew_buf.device() && lengths.device() == rew_buf.device(),
              "episode_reduce: mixed devices");
  hipLaunchKernelGGL(episode_reduce_kernel, dim3(std::min(256, (N + 255) / 256)),
                     dim3(256), 0, current_stream(), rew_buf.data_ptr<float>(), dn,
                     returns.data_ptr<double>(), lengths.data_ptr<int>(), N, steps);
  HIP_OK(hipGetLastError());
}

// out[i] = low + (high - low) * u, u in (0, 1] keyed by (seed, offset, i)
void uniform_sample(torch::Tensor out, double low, double high, int64_t seed,
                    int64_t offset, c10::optional<torch::Tensor> offset_ctr) {
  check_f32_gpu(out, "out");
  TORCH_CHECK(low <= high, "uniform_sample: low > high");
  TORCH_CHECK(out.numel() < (1LL << 31), "uniform_sample: out too large");
  const int total = (int)out.numel();
  if (total == 0) return;
  hipLaunchKernelGGL(uniform_sample_kernel,
                     dim3(std::min(256, (total + 255) / 256)), dim3(256), 0,
                     current_stream(), out.data_ptr<float>(), total, (float)low,
                     (float)high, (uint64_t)seed, (uint64_t)offset,
                     ctr_ptr(offset_ctr));
  HIP_OK(hipGetLastError());
}

// the multi-kernel body's ring write: the epoch buffers of steps x (action
// -> env step) into the slots the persistent collect kernels write.  O and A
// come from obs_full and act_buf and must be the ring's.
// cut_slot [steps] int32: index into cut_final on cut steps, -1 elsewhere.
void replay_scatter(torch::Tensor obs_full, torch::Tensor act_buf,
                    torch::Tensor rew_buf, torch::Tensor cut_final,
                    torch::Tensor cut_slot, int64_t n_cuts,
                    std::vector<torch::Tensor> storage, torch::Tensor write_dev,
                    torch::Tensor size_dev, torch::Tensor seg_returns) {
  check_f32_gpu(obs_full, "obs_full");
  TORCH_CHECK(obs_full.dim() == 3 && obs_full.size(0) >= 2 && obs_full.size(1) >= 1 &&
                  obs_full.size(2) >= 1,
              "obs_full must be [steps+1, N, O]");
  TORCH_CHECK(act_buf.dim() == 3 && act_buf.size(2) >= 1, "act_buf must be [steps, N, A]");
  ReplayScatterArgs a{};
  a.steps = (int)obs_full.size(0) - 1;
  a.N = (int)obs_full.size(1);
  const int64_t O = obs_full.size(2), A = act_buf.size(2);
  const int64_t SN = (int64_t)a.steps * a.N;
  a.ring = check_ring(storage, write_dev, size_dev, SN, obs_full.device(), O, A);
  check_out(act_buf, torch::kFloat32, SN * A, "act_buf");
  check_out(rew_buf, torch::kFloat32, SN, "rew_buf");
  check_out(cut_slot, torch::kInt32, a.steps, "cut_slot");
  TORCH_CHECK(n_cuts >= 0 && n_cuts <= a.steps, "n_cuts out of range");
  a.n_cuts = (int)n_cuts;
  check_f32_gpu(cut_final, "cut_final");
  TORCH_CHECK(cut_final.dim() == 3 && cut_final.size(0) >= std::max(a.n_cuts, 1) &&
                  cut_final.size(1) == a.N && cut_final.size(2) == O,
              "cut_final must be [n_cuts, N, O]");
  check_f32_gpu(seg_returns, "seg_returns");
  TORCH_CHECK(seg_returns.dim() == 2 && seg_returns.size(0) == a.N &&
                  seg_returns.size(1) >= std::max(a.n_cuts, 1),
              "seg_returns must be [N, n_segs]");
  a.n_segs = (int)seg_returns.size(1);
  for (const torch::Tensor* t : {&act_buf, &rew_buf, &cut_slot, &cut_final, &seg_returns})
    TORCH_CHECK(t->device() == obs_full.device(), "replay_scatter: mixed devices");
  a.obs_full = obs_full.data_ptr<float>();
  a.act_buf = act_buf.data_ptr<float>();
  a.rew_buf = rew_buf.data_ptr<float>();
  a.cut_final = cut_final.data_ptr<float>();
  a.cut_slot = cut_slot.data_ptr<int>();
  a.seg_returns = seg_returns.data_ptr<float>();
  const int64_t elems = SN * (2 * O + A);
  hipLaunchKernelGGL(replay_scatter_kernel,
                     dim3((unsigned)std::min<int64_t>(256, (elems + 255) / 256)),
                     dim3(256), 0, current_stream(), a);
  HIP_OK(hipGetLastError());
}

// write = (write + n) % cap, size = min(size + n, cap) on the device
void ring_advance_(torch::Tensor write_dev, torch::Tensor size_dev, int64_t n,
                   int64_t cap) {
  for (const torch::Tensor* s : {&write_dev, &size_dev})
    TORCH_CHECK(s->scalar_type() == torch::kInt64 && s->is_cuda() && s->numel() == 1,
                "ring scalars must be 1-element int64 CUDA tensors");
  TORCH_CHECK(cap >= 1 && n >= 0 && n <= cap, "ring_advance_: n outside [0, cap]");
  hipLaunchKernelGGL(ring_advance_kernel, dim3(1), dim3(1), 0, current_stream(),
                     reinterpret_cast<long long*>(write_dev.data_ptr<int64_t>()),
                     reinterpret_cast<long long*>(size_dev.data_ptr<int64_t>()),
                     (unsigned long long)n, (unsigned long long)cap);
  HIP_OK(hipGetLastError());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("pendulum_eval_fused", &pendulum_eval_fused,
        "N whole Pendulum episodes in one persistent kernel (gfx950)",
        py::arg("weights"), py::arg("biases"), py::arg("acts"), py::arg("mode"),
        py::arg("log_std"), py::arg("policy_seed"), py::arg("env_seed"),
        py::arg("horizon"), py::arg("ctr"), py::arg("reset_ctr"),
        py::arg("returns"), py::arg("lengths"), py::arg("init_state"),
        py::arg("wide_threads"));
  m.def("pendulum_eval_fused_lds_bytes", &pendulum_eval_fused_lds_bytes_py,
        "dynamic LDS of pendulum_eval_fused for a net [3, ..., 1]");
  m.def("pendulum_eval_fused_limits",
        []() {
          return std::vector<int64_t>{MLP_MAX_LAYERS, MLP_MAX_WIDTH, DEFAULT_LDS_LIMIT};
        },
        "(max layers, max width, LDS budget in bytes) of pendulum_eval_fused");
  m.def("cartpole_eval_fused", &cartpole_eval_fused,
        "N whole CartPole episodes in one persistent kernel (gfx950)",
        py::arg("weights"), py::arg("biases"), py::arg("acts"),
        py::arg("policy_seed"), py::arg("env_seed"), py::arg("horizon"),
        py::arg("ctr"), py::arg("reset_ctr"), py::arg("returns"),
        py::arg("lengths"), py::arg("init_state"));
  m.def("cartpole_eval_fused_lds_bytes", &cartpole_eval_fused_lds_bytes_py,
        "dynamic LDS of cartpole_eval_fused for a net [4, ..., n_act]");
  m.def("cartpole_eval_fused_limits",
        []() {
          return std::vector<int64_t>{MLP_MAX_LAYERS, ROLLOUT_MAX_WIDTH,
                                      DEFAULT_LDS_LIMIT};
        },
        "(max layers, max width, LDS budget in bytes) of cartpole_eval_fused");
  m.def("episode_reduce", &episode_reduce,
        "first-episode return and length of each row of a reward buffer (gfx950)",
        py::arg("rew_buf"), py::arg("done_buf"), py::arg("returns"),
        py::arg("lengths"));
  m.def("pendulum_collect_fused", &pendulum_collect_fused,
        "whole-epoch Pendulum replay collection in one persistent kernel (gfx950)",
        py::arg("weights"), py::arg("biases"), py::arg("acts"), py::arg("mode"),
        py::arg("noise_scale"), py::arg("limit"), py::arg("low"), py::arg("high"),
        py::arg("action_seed"), py::arg("env_seed"), py::arg("cuts"),
        py::arg("start_with_reset"), py::arg("ctr"), py::arg("state"),
        py::arg("steps"), py::arg("storage"), py::arg("write_dev"),
        py::arg("size_dev"), py::arg("seg_returns"), py::arg("last_obs"),
        py::arg("wide_threads"));
  m.def("pendulum_collect_fused_lds_bytes", &pendulum_collect_fused_lds_bytes_py,
        "dynamic LDS of pendulum_collect_fused for an actor [3, ..., 1]");
  m.def("pendulum_collect_fused_limits",
        []() {
          return std::vector<int64_t>{MLP_MAX_LAYERS, MLP_MAX_WIDTH,
                                      ROLLOUT_MAX_CUTS, (int64_t)MLP_LDS_BUDGET};
        },
        "(max layers, max width, max cuts, LDS budget in bytes) of "
        "pendulum_collect_fused");
  m.def("synthetic_collect_fused", &synthetic_collect_fused,
        "whole-epoch synthetic-env replay collection in one persistent kernel (gfx950)",
        py::arg("weights"), py::arg("biases"), py::arg("acts"), py::arg("mode"),
        py::arg("noise_scale"), py::arg("limit"), py::arg("low"), py::arg("high"),
        py::arg("action_seed"), py::arg("env_seed"), py::arg("envA"),
        py::arg("envB"), py::arg("envw"), py::arg("sigma"), py::arg("cuts"),
        py::arg("start_with_reset"), py::arg("ctr"), py::arg("carry"),
        py::arg("steps"), py::arg("storage"), py::arg("write_dev"),
        py::arg("size_dev"), py::arg("seg_returns"), py::arg("wide_threads"));
  m.def("synthetic_collect_fused_lds_bytes", &synthetic_collect_fused_lds_bytes_py,
        "dynamic LDS of synthetic_collect_fused for an actor [O, ..., A] "
        "(empty dims: the uniform draw)");
  m.def("synthetic_collect_fused_limits",
        []() {
          return std::vector<int64_t>{MLP_MAX_LAYERS, MLP_MAX_WIDTH,
                                      ROLLOUT_MAX_CUTS, (int64_t)MLP_LDS_BUDGET};
        },
        "(max layers, max width, max cuts, LDS budget in bytes) of "
        "synthetic_collect_fused");
  m.def("uniform_sample", &uniform_sample,
        "Philox uniform actions in [low, high] (gfx950)", py::arg("out"),
        py::arg("low"), py::arg("high"), py::arg("seed"), py::arg("offset"),
        py::arg("offset_ctr") = py::none());
  m.def("replay_scatter", &replay_scatter,
        "ring write of one captured collect epoch's buffers (gfx950)",
        py::arg("obs_full"), py::arg("act_buf"), py::arg("rew_buf"),
        py::arg("cut_final"), py::arg("cut_slot"), py::arg("n_cuts"),
        py::arg("storage"), py::arg("write_dev"), py::arg("size_dev"),
        py::arg("seg_returns"));
  m.def("ring_advance_", &ring_advance_,
        "advance the replay ring's device write position and fill (gfx950)");
  m.def("pendulum_rollout_fused", &pendulum_rollout_fused,
        "whole-epoch Pendulum rollout in one persistent kernel (gfx950)",
        py::arg("weights"), py::arg("biases"), py::arg("acts"),
        py::arg("log_std"), py::arg("policy_seed"), py::arg("env_seed"),
        py::arg("cuts"), py::arg("start_with_reset"), py::arg("ctr"),
        py::arg("state"), py::arg("obs_full"), py::arg("act_buf"),
        py::arg("rew_buf"), py::arg("cut_final"));
  m.def("pendulum_rollout_fused_lds_bytes", &pendulum_rollout_fused_lds_bytes_py,
        "dynamic LDS of pendulum_rollout_fused for a net [3, ..., 1]");
  m.def("pendulum_rollout_fused_limits",
        []() {
          return std::vector<int64_t>{MLP_MAX_LAYERS, ROLLOUT_MAX_WIDTH,
                                      ROLLOUT_MAX_CUTS, DEFAULT_LDS_LIMIT};
        },
        "(max layers, max width, max cuts, LDS budget in bytes) of "
        "pendulum_rollout_fused");
  m.def("pendulum_env_step", &pendulum_env_step,
        "Pendulum transition + lockstep autoreset (gfx950)", py::arg("state"),
        py::arg("actions"), py::arg("do_reset"), py::arg("seed"),
        py::arg("offset"), py::arg("offset_ctr") = py::none(),
        py::arg("obs") = py::none(), py::arg("final_obs") = py::none(),
        py::arg("reward") = py::none());
  m.def("pendulum_env_reset", &pendulum_env_reset,
        "Pendulum init states, or (draw=False) the observation of `state`",
        py::arg("state"), py::arg("seed"), py::arg("offset"),
        py::arg("offset_ctr") = py::none(), py::arg("obs") = py::none(),
        py::arg("draw") = true);
  m.def("cartpole_rollout_fused", &cartpole_rollout_fused,
        "whole-epoch CartPole rollout in one persistent kernel (gfx950)",
        py::arg("weights"), py::arg("biases"), py::arg("acts"),
        py::arg("policy_seed"), py::arg("env_seed"), py::arg("max_steps"),
        py::arg("start_with_reset"), py::arg("ctr"), py::arg("state"),
        py::arg("elapsed"), py::arg("obs_full"), py::arg("final_obs"),
        py::arg("act_buf"), py::arg("rew_buf"), py::arg("done_buf"));
  m.def("cartpole_rollout_fused_lds_bytes", &cartpole_rollout_fused_lds_bytes_py,
        "dynamic LDS of cartpole_rollout_fused for a net [4, ..., n_act]");
  m.def("cartpole_rollout_fused_limits",
        []() {
          return std::vector<int64_t>{MLP_MAX_LAYERS, ROLLOUT_MAX_WIDTH,
                                      DEFAULT_LDS_LIMIT};
        },
        "(max layers, max width, LDS budget in bytes) of cartpole_rollout_fused");
  m.def("cartpole_env_step", &cartpole_env_step,
        "CartPole transition + termination + autoreset (gfx950)",
        py::arg("state"), py::arg("elapsed"), py::arg("actions"),
        py::arg("max_steps"), py::arg("seed"), py::arg("offset"),
        py::arg("offset_ctr") = py::none(), py::arg("obs") = py::none(),
        py::arg("final_obs") = py::none(), py::arg("reward") = py::none(),
        py::arg("done") = py::none());
  m.def("cartpole_env_reset", &cartpole_env_reset,
        "CartPole init states (gfx950)", py::arg("state"), py::arg("elapsed"),
        py::arg("seed"), py::arg("offset"), py::arg("offset_ctr") = py::none(),
        py::arg("obs") = py::none());
  m.def("ppo_rollout_fused", &ppo_rollout_fused,
        "whole-epoch PPO rollout in one persistent kernel (gfx950)",
        py::arg("weights"), py::arg("biases"), py::arg("acts"),
        py::arg("log_std"), py::arg("env_A"), py::arg("env_B"), py::arg("env_w"),
        py::arg("sigma"), py::arg("policy_seed"), py::arg("env_seed"),
        py::arg("cuts"), py::arg("start_with_reset"), py::arg("ctr"),
        py::arg("obs_full"), py::arg("act_buf"), py::arg("rew_buf"),
        py::arg("cut_final"));
  m.def("ppo_rollout_fused_lds_bytes", &ppo_rollout_fused_lds_bytes_py,
        "dynamic LDS of ppo_rollout_fused for a net [O, ..., A]");
  m.def("ppo_rollout_fused_limits",
        []() {
          return std::vector<int64_t>{MLP_MAX_LAYERS, ROLLOUT_MAX_WIDTH,
                                      ROLLOUT_MAX_CUTS, (int64_t)MLP_LDS_BUDGET};
        },
        "(max layers, max width / obs dim, max cuts, LDS budget in bytes) of "
        "ppo_rollout_fused");
  m.def("fused_mlp_limits",
        []() {
          return std::vector<int64_t>{MLP_MAX_LAYERS, MLP_MAX_WIDTH,
                                      MLP_NARROW_WIDTH, GAUSS_MAX_D};
        },
        "(max layers, max width, max width of the whole-net LDS-image "
        "kernels = max action dim of the fused policy iteration, max action "
        "dim of the Gaussian loss kernel)");
  m.def("fused_bwd_fits",
        [](std::vector<int64_t> dims, int64_t reserve) {
          try {
            const NetLayout n = net_layout(dims, MLP_MAX_WIDTH, (int)reserve);
            return std::vector<bool>{fused_bwd_fits(n, false),
                                     fused_bwd_fits(n, true)};
          } catch (const c10::Error&) {  // no net the bindings take at all
            return std::vector<bool>{false, false};
          }
        },
        "whether the whole-net fused backward takes a net [in, ..., out]: "
        "(with a separate forward, with the forward in the kernel); reserve "
        "= argument-block slots kept free (1 for the log_std pseudo-layer)",
        py::arg("dims"), py::arg("reserve") = 0);
  m.def("mlp_forward", &mlp_forward, "fused MLP forward (gfx950)",
        py::arg("x"), py::arg("weights"), py::arg("biases"), py::arg("acts"),
        py::arg("save_hidden"), py::arg("compute_bf16") = 0);
  m.def("mlp_backward", &mlp_backward, "fused MLP backward (gfx950)",
        py::arg("grad_out"), py::arg("x"), py::arg("weights"), py::arg("biases"),
        py::arg("hidden"), py::arg("final_out"), py::arg("acts"),
        py::arg("compute_bf16") = 0, py::arg("adam_m") = py::none(),
        py::arg("adam_v") = py::none(), py::arg("adam_step") = py::none(),
        py::arg("lr") = 0.0, py::arg("beta1") = 0.9, py::arg("beta2") = 0.999,
        py::arg("eps") = 1e-8, py::arg("weight_decay") = 0.0,
        py::arg("adam_step_delta") = 0.0, py::arg("adam_gate") = py::none(),
        py::arg("input_grad_only") = false);
  m.def("value_mlp_backward", &value_mlp_backward,
        "fused value-MSE whole-net backward (gfx950)", py::arg("x"),
        py::arg("weights"), py::arg("biases"), py::arg("hidden"),
        py::arg("final_out"), py::arg("acts"), py::arg("returns"),
        py::arg("compute_bf16") = 0, py::arg("partials_out") = py::none(),
        py::arg("adam_m") = py::none(), py::arg("adam_v") = py::none(),
        py::arg("adam_step") = py::none(), py::arg("lr") = 0.0,
        py::arg("beta1") = 0.9, py::arg("beta2") = 0.999,
        py::arg("eps") = 1e-8, py::arg("weight_decay") = 0.0,
        py::arg("adam_step_delta") = 0.0, py::arg("fwd_in_kernel") = false);
  m.def("value_loss_partials_blocks",
        [](int64_t batch) {
          return (batch + BWD_FUSED_ROWS - 1) / BWD_FUSED_ROWS;
        },
        "partials row length used by value_mlp_backward");
  m.def("value_loss_finalize", &value_loss_finalize,
        "batched deferred value-loss finalize (gfx950)");
  m.def("adam_bump_", &adam_bump_, "bump Adam step counters (gfx950)");
  m.def("adam_bump_dev_", &adam_bump_dev_,
        "bump Adam step counters by a device scalar (gfx950)");
  m.def("ppo_gate_update_", &ppo_gate_update_,
        "device-side KL early-stop gate bookkeeping (gfx950)");
  m.def("gaussian_ppo_policy_iter", &gaussian_ppo_policy_iter,
        "one 2-kernel Gaussian-PPO policy iteration (gfx950)");
  m.def("gaussian_ppo_value_twin_iter", &gaussian_ppo_value_twin_iter,
        "PPO policy + value iteration in one twin kernel pair (gfx950)");
  m.def("categorical_ppo_policy_iter", &categorical_ppo_policy_iter,
        "one 2-kernel categorical-PPO policy iteration (gfx950)");
  m.def("categorical_ppo_value_twin_iter", &categorical_ppo_value_twin_iter,
        "categorical-PPO policy + value iteration in one twin kernel pair "
        "(gfx950)");
  m.def("ppo_twin_uses_shaped", &ppo_twin_uses_shaped,
        "whether the twin iteration takes the [*,64,32,*] shaped kernel");
  m.def("reduce_adam_is_staged",
        [](int64_t n_blocks, int64_t grand) {
          return mlp_reduce_adam_is_staged((int)n_blocks, (long)grand);
        },
        "whether the reduce+Adam launch takes the LDS-staged kernel");
  m.def("segmented_gae", &segmented_gae, "segmented GAE+returns scan (gfx950)");
  m.def("normalize", &normalize, "fused mean/std normalize (gfx950)");
  m.def("segmented_gae_out", &segmented_gae_out,
        "segmented GAE+returns scan into the caller's buffers (gfx950)");
  m.def("normalize_out", &normalize_out,
        "fused mean/std normalize into the caller's buffer (gfx950)");
  m.def("ppo_ingest_rows", &ppo_ingest_rows,
        "one pass over a PPO epoch's rows: three forwards, two log-probs and "
        "the copies into the update graph's buffers (gfx950)");
  m.def("ppo_ingest_rows_lds_bytes", &ppo_ingest_rows_lds_bytes_py,
        "dynamic LDS of ppo_ingest_rows for (value dims, policy dims)");
  m.def("ppo_ingest_rows_limits",
        []() {
          return std::vector<int64_t>{ROLLOUT_MAX_WIDTH, (int64_t)MLP_LDS_BUDGET};
        },
        "(max width, LDS budget) of ppo_ingest_rows");
  m.def("ppo_epoch_epilogue_", &ppo_epoch_epilogue_,
        "the captured PPO epoch's tail in one launch (gfx950)");
  m.def("q_target", &q_target, "fused Q-learning target (gfx950)");
  m.def("td3_smooth", &td3_smooth,
        "TD3 target-policy smoothing: Philox noise + clip + limit (gfx950)",
        py::arg("a"), py::arg("seed"), py::arg("offset"), py::arg("scale"),
        py::arg("clip"), py::arg("limit"), py::arg("offset_ctr") = py::none());
  m.def("q_target_min2", &q_target_min2,
        "fused min-twin Q-learning target (gfx950)");
  m.def("replay_gather", &replay_gather,
        "one-kernel Philox minibatch gather from the HBM replay ring (gfx950)",
        py::arg("obs"), py::arg("act"), py::arg("rew"), py::arg("nxt"),
        py::arg("dn"), py::arg("size_dev"), py::arg("B"), py::arg("seed"),
        py::arg("offset"), py::arg("offset_ctr") = py::none());
  m.def("fused_adam_", &fused_adam_, "fused multi-tensor Adam (gfx950)",
        py::arg("params"), py::arg("grads"), py::arg("exp_avgs"),
        py::arg("exp_avg_sqs"), py::arg("steps"), py::arg("lr"),
        py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("weight_decay"), py::arg("step_delta") = 0.0,
        py::arg("do_bump") = true, py::arg("gate") = py::none());
  m.def("fused_polyak_", &fused_polyak_, "fused multi-tensor Polyak (gfx950)");
  m.def("gaussian_policy_loss", &gaussian_policy_loss,
        "fused Gaussian VPG/PPO loss fwd+bwd (gfx950)");
  m.def("gaussian_logp", &gaussian_logp, "Gaussian log-prob (gfx950)");
  m.def("gaussian_kl", &gaussian_kl, "approx KL for Gaussian policy (gfx950)");
  m.def("categorical_policy_loss", &categorical_policy_loss,
        "fused Categorical VPG/PPO loss fwd+bwd (gfx950)");
  m.def("categorical_logp", &categorical_logp, "Categorical log-prob (gfx950)");
  m.def("categorical_kl", &categorical_kl, "approx KL for Categorical policy (gfx950)");
  m.def("value_mse_loss", &value_mse_loss, "fused value MSE fwd+bwd (gfx950)");
  m.def("gaussian_sample", &gaussian_sample,
        "Philox Gaussian action sample (gfx950)", py::arg("mean"),
        py::arg("log_std"), py::arg("seed"), py::arg("offset"),
        py::arg("noise_scale"), py::arg("limit"),
        py::arg("offset_ctr") = py::none(), py::arg("out") = py::none());
  m.def("categorical_sample", &categorical_sample,
        "Philox categorical action sample (gfx950)", py::arg("logits"),
        py::arg("seed"), py::arg("offset"), py::arg("offset_ctr") = py::none(),
        py::arg("out") = py::none());
  m.def("synthetic_env_step", &synthetic_env_step,
        "fused synthetic-env transition + reward (gfx950)", py::arg("state"),
        py::arg("actions"), py::arg("A"), py::arg("B"), py::arg("w"),
        py::arg("sigma"), py::arg("seed"), py::arg("offset"),
        py::arg("do_reset"), py::arg("offset_ctr") = py::none(),
        py::arg("s_out") = py::none(), py::arg("final_out") = py::none(),
        py::arg("reward") = py::none());
  m.def("synthetic_env_reset", &synthetic_env_reset,
        "synthetic-env init states (gfx950)", py::arg("num_envs"),
        py::arg("obs_dim"), py::arg("like"), py::arg("seed"), py::arg("offset"),
        py::arg("offset_ctr") = py::none(), py::arg("out") = py::none());
  m.def("counter_add_", &counter_add_,
        "advance a device RNG counter (gfx950)");
}
