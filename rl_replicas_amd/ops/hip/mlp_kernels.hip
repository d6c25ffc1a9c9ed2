// Fused MLP forward/backward kernels for gfx950 (CDNA4).
//
// Replaces the reference's eager nn.Sequential forward + autograd
// backward (reference: src/rl_replicas/networks/mlp.py:29-41) for the
// tiny-MLP / launch-latency-bound regime this library lives in
// (SURVEY.md §7 "Tiny-tensor regime"): the whole multi-layer forward is
// ONE kernel launch; each workgroup owns a ROWS-row tile of the batch,
// ping-pongs layer activations between two padded LDS regions, and runs
// every Linear layer as MFMA tiles (v_mfma_f32_16x16x4_f32: exact fp32,
// guide §3) with bias+activation fused into the epilogue.
//
// Weight access is the latency hazard at these sizes (a scattered
// per-lane W read per MFMA serializes on L2 latency when the grid is
// small), so the narrow kernels (widths <= 64) stage weights through LDS:
// the ENTIRE net's weights (one layer's, in the per-layer backward) are
// staged once per block into a padded LDS image ([out][(in+1)] per layer
// -> odd row stride, bank-conflict-free for both W and W^T reads).  The
// host sizes the dynamic LDS and admits only nets whose image fits its
// budget; wider nets run the per-layer column-split kernels further down.
//
// Backward = ONE merged kernel per layer (dgrad + wgrad/bias partials
// sharing the staged dZ tile) + a TWO-STAGE deterministic partial
// reduction (split-K via workspace instead of atomics so every run is
// bitwise reproducible — SURVEY.md §4).  Workspace layout is
// [block][all-layer elems] so the first reduction stage is layer-blind.
#include <algorithm>

#include "common.h"
#include "rollout_steps.h"

// ---------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------
template <int LDSW>
DEV_INLINE void load_tile(const float* __restrict__ src, float* dst_lds,
                          int row0, int batch, int width, int tid, int rows) {
  for (int idx = tid; idx < rows * width; idx += 256) {
    int r = idx / width, c = idx % width;
    float v = 0.f;
    int row = row0 + r;
    if (row < batch) v = src[(long)row * width + c];
    dst_lds[r * LDSW + c] = v;
  }
}

template <int LDSW>
DEV_INLINE void store_tile(float* __restrict__ dst, const float* src_lds,
                           int row0, int batch, int width, int tid, int rows) {
  for (int idx = tid; idx < rows * width; idx += 256) {
    int r = idx / width, c = idx % width;
    int row = row0 + r;
    if (row < batch) dst[(long)row * width + c] = src_lds[r * LDSW + c];
  }
}

// stage W[rows0..rows0+nrows)[0..ncols) -> lds image with row stride
// (ncols+1) — whole-block cooperative, caller barriers
DEV_INLINE void stage_weights_block(const float* __restrict__ W, float* wlds,
                                    int nrows, int ncols, int tid) {
  for (int idx = tid; idx < nrows * ncols; idx += 256) {
    int r = idx / ncols, c = idx % ncols;
    wlds[r * (ncols + 1) + c] = W[(long)r * ncols + c];
  }
}

// ---------------------------------------------------------------------------
// fused forward
// ---------------------------------------------------------------------------
template <int ROWS, int MAXW, bool BF16 = false>
__global__ __launch_bounds__(256) void fused_mlp_fwd_f32_t(
    MLPArgs args, const float* __restrict__ x, int save_hidden) {
  constexpr int LDSW = MAXW + 4;
  constexpr int RT = ROWS / 16;        // row tiles per block
  constexpr int JT_STRIDE = 4 / RT;    // waves sharing one row tile
  extern __shared__ float smem[];
  float* const buf0 = smem;
  float* const buf1 = smem + ROWS * LDSW;
  float* wlds = smem + 2 * ROWS * LDSW;  // whole-net weight image
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int row0 = blockIdx.x * ROWS;
  const int wr0 = (wave % RT) * 16;
  const int jt0 = (wave / RT) * 16;

  load_tile<LDSW>(x, buf0, row0, args.batch, args.dims[0], tid, ROWS);
  int off = 0;
  for (int l = 0; l < args.n_layers; ++l) {
    stage_weights_block(args.w[l], wlds + off, args.dims[l + 1], args.dims[l], tid);
    off += args.dims[l + 1] * (args.dims[l] + 1);
  }
  __syncthreads();

  const int i = lane & 15;
  const int k = lane >> 4;
  int cur = 0;
  int woff = 0;
  for (int l = 0; l < args.n_layers; ++l) {
    const int in_d = args.dims[l];
    const int out_d = args.dims[l + 1];
    const float* B = args.b[l];
    const int act = args.acts[l];
    const int nxt = cur ^ 1;
    const float* buf_in = (cur == 0) ? buf0 : buf1;
    float* buf_out = (cur == 0) ? buf1 : buf0;
    const int wrow = in_d + 1;  // padded W row stride

    for (int jt = jt0; jt < out_d; jt += 16 * JT_STRIDE) {
      const int j = jt + i;
      const bool jok = j < out_d;
      // shared with the persistent rollout kernel (rollout_steps.h)
      const f32x4 acc = mlp_fwd_tile_lds<LDSW, BF16>(buf_in, wlds + woff, wrow,
                                                     in_d, wr0 + i, k, j, jok);
      mlp_fwd_tile_epilogue<LDSW>(acc, B, act, j, jok, wr0, lane, buf_out);
    }
    __syncthreads();

    const bool is_last = (l == args.n_layers - 1);
    if (is_last || save_hidden) {
      store_tile<LDSW>(args.h[l], buf_out, row0, args.batch, out_d, tid, ROWS);
    }
    cur = nxt;
    woff += out_d * wrow;
    // next layer writes bufs[cur^1] (fully consumed) and reads bufs[cur]
    // (fully written before the barrier above) -> one barrier per layer
  }
}

// ---------------------------------------------------------------------------
// merged backward layer: ONE kernel per layer computing
//   dZ = dY * act'(y)           (staged once in LDS)
//   dX = dZ @ W                 (row tiles, written to global)
//   dW_p = dZ^T @ X, db_p       (per-row-block partials to workspace)
// workspace layout: ws[block][layer-elems at layer_off]
// ---------------------------------------------------------------------------
template <int ROWS, int MAXW>
__global__ __launch_bounds__(256) void mlp_bwd_layer_f32_t(
    const float* __restrict__ dy, const float* __restrict__ y,
    const float* __restrict__ xin, const float* __restrict__ W,
    float* __restrict__ dx, float* __restrict__ workspace, long ws_stride,
    int batch, int out_d, int in_d, int act) {
  constexpr int LDSW = MAXW + 4;
  constexpr int RT = ROWS / 16;
  constexpr int JT_STRIDE = 4 / RT;
  extern __shared__ float smem[];
  float* dz = smem;
  float* xt = smem + ROWS * LDSW;
  float* wlds = smem + 2 * ROWS * LDSW;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int row0 = blockIdx.x * ROWS;
  const int wr0 = (wave % RT) * 16;
  const int jt0 = (wave / RT) * 16;
  // element-major workspace (ws[elem][block]): the latency-bound reduce
  // reads each element's partials CONTIGUOUSLY; writers scatter instead
  // (stores don't stall)
  float* wsp = workspace + blockIdx.x;
  const long WSN = gridDim.x;

  for (int idx = tid; idx < ROWS * out_d; idx += 256) {
    int r = idx / out_d, c = idx % out_d;
    int row = row0 + r;
    float v = 0.f;
    if (row < batch) {
      long g = (long)row * out_d + c;
      v = dy[g] * act_grad_from_y(act, y[g]);
    }
    dz[r * LDSW + c] = v;
  }
  load_tile<LDSW>(xin, xt, row0, batch, in_d, tid, ROWS);
  stage_weights_block(W, wlds, out_d, in_d, tid);
  __syncthreads();

  const int i = lane & 15;
  const int k = lane >> 4;
  const int wrow = in_d + 1;

  // ---- dgrad: dX[b][j] = sum_k dZ[b][k] W[k][j] ----
  for (int jt = jt0; jt < in_d; jt += 16 * JT_STRIDE) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int j = jt + i;
    const bool jok = j < in_d;
    for (int k0 = 0; k0 < out_d; k0 += 4) {
      const int kk = k0 + k;
      float a = (kk < out_d) ? dz[(wr0 + i) * LDSW + kk] : 0.f;
      float bv = (jok && kk < out_d) ? wlds[kk * wrow + j] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0);
    }
    if (jok) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + wr0 + (lane >> 4) * 4 + r;
        if (row < batch) dx[(long)row * in_d + jt + i] = acc[r];
      }
    }
  }

  // ---- wgrad partials: dW[i][j] = sum_r dZ[r][i] X[r][j], K = ROWS ----
  const int n_it = (out_d + 15) / 16;
  for (int it = wave; it < n_it; it += 4) {
    const int ii = it * 16 + i;
    for (int jt = 0; jt < in_d; jt += 16) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < ROWS; k0 += 4) {
        float a = (ii < out_d) ? dz[(k0 + k) * LDSW + ii] : 0.f;
        float bv = (jt + i < in_d) ? xt[(k0 + k) * LDSW + jt + i] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0);
      }
      const int col = jt + i;
      if (col < in_d) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int orow = it * 16 + (lane >> 4) * 4 + r;
          if (orow < out_d) wsp[((long)orow * in_d + col) * WSN] = acc[r];
        }
      }
    }
  }

  __syncthreads();
  for (int c = tid; c < out_d; c += 256) {
    float s = 0.f;
    #pragma unroll 4
    for (int r = 0; r < ROWS; ++r) s += dz[r * LDSW + c];
    wsp[((long)out_d * in_d + c) * WSN] = s;
  }
}

// ---------------------------------------------------------------------------
// whole-net fused backward (narrow nets): ONE kernel walks the layer
// chain backwards per 32-row block — dZ ping-pongs between two LDS
// tiles (the next layer's activation-grad is fused into the dgrad
// epilogue, read from the already-staged X tile), weights come from the
// whole-net LDS image, and wgrad/bias partials stream to the split-K
// workspace.  Replaces L per-layer launches with one.
// ---------------------------------------------------------------------------
// When mse_returns != nullptr the last layer's dZ is seeded directly
// from the value-MSE gradient 2*(v - ret)/B (final activation must be
// identity, out_d == 1 — the value-function case, ppo.py:283-287) and
// the per-block loss partial sum((v-ret)^2)/B goes to loss_partials.
// DO_FWD: the forward pass runs INSIDE this kernel (value-loop fast
// path): x is staged once, every layer's activations land in LDS
// (hlds) and never touch HBM; the MSE seed and the backward read them
// from LDS.  fp32 only; requires mse_returns.
// NEED_DX = false drops the layer-0 dgrad MFMA loop and the dx_out store
// (batch x in_dim floats): the fused-Adam callers never read the input
// gradient, so dx_out may be nullptr there.
//
// The body is a device function so that one launch can run it for two
// nets (mlp_bwd_fused_twin_f32 below).  `bx` is the workgroup's row block
// and `WSN` the block count of the element-major workspace — blockIdx.x
// and gridDim.x in the single-net kernel; `smem` is the dynamic LDS base.
template <int ROWS, bool BF16, bool DO_FWD, bool NEED_DX, bool CAT = false>
DEV_INLINE void mlp_bwd_fused_body(
    const MLPBwdArgs& args, const float* __restrict__ x,
    const float* __restrict__ dy, float* __restrict__ dx_out,
    float* __restrict__ workspace, const float* __restrict__ mse_returns,
    float* __restrict__ loss_partials, const GaussSeedArgs& gargs,
    float* smem, const int bx, const long WSN) {
  constexpr int MAXW = 64;
  constexpr int LDSW = MAXW + 4;
  constexpr int RT = ROWS / 16;
  constexpr int JT_STRIDE = 4 / RT;
  // gate-frozen PPO iteration: a no-op by definition.  The only reader of
  // this kernel's partials (the gated reduce+Adam kernel that follows)
  // tests the same gate before it touches them, and nothing between the
  // two launches reopens it.
  if (DO_FWD && gargs.skip_gate != nullptr && *gargs.skip_gate == 0.f) return;
  float* const dza = smem;
  float* const dzb = smem + ROWS * LDSW;
  float* const xt = smem + 2 * ROWS * LDSW;
  float* const wlds = smem + 3 * ROWS * LDSW;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int row0 = bx * ROWS;
  const int wr0 = (wave % RT) * 16;
  const int jt0 = (wave / RT) * 16;
  float* wsp = workspace + bx;  // element-major: ws[elem][block]
  const int L = args.n_layers;

  // whole-net padded W image + layer offsets
  int woffs[MLP_MAX_LAYERS];
  int wtotal = 0;
  {
    int off = 0;
    for (int l = 0; l < L; ++l) {
      woffs[l] = off;
      stage_weights_block(args.w[l], wlds + off, args.dims[l + 1], args.dims[l], tid);
      off += args.dims[l + 1] * (args.dims[l] + 1);
    }
    wtotal = off;
  }
  // DO_FWD: per-layer activations live here, [L][ROWS][LDSW]
  float* const hlds = wlds + wtotal;
  if constexpr (DO_FWD) {
    const int fi = lane & 15;
    load_tile<LDSW>(x, xt, row0, args.batch, args.dims[0], tid, ROWS);
    __syncthreads();  // weights + x staged
    const float* fin = xt;
    for (int l = 0; l < L; ++l) {
      const int in_d = args.dims[l];
      const int out_d = args.dims[l + 1];
      const int wrow = in_d + 1;
      const float* wl = wlds + woffs[l];
      float* hl = hlds + l * ROWS * LDSW;
      const int fk = lane >> 4;
      for (int jt = jt0; jt < out_d; jt += 16 * JT_STRIDE) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int j = jt + fi;
        const bool jok = j < out_d;
        for (int k0 = 0; k0 < in_d; k0 += 4) {
          const int kk = k0 + fk;
          float a = (kk < in_d) ? fin[(wr0 + fi) * LDSW + kk] : 0.f;
          float bv = (jok && kk < in_d) ? wl[j * wrow + kk] : 0.f;
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0);
        }
        if (jok) {
          const float bias = args.b[l][j];
          #pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int rr = wr0 + (lane >> 4) * 4 + r;
            hl[rr * LDSW + j] = act_apply(args.acts[l], acc[r] + bias);
          }
        }
      }
      __syncthreads();
      fin = hl;
    }
  }
  // Categorical-PPO seed (CAT instantiations, DO_FWD fp32): per-row
  // logp = logit[a] - lse from the LDS-resident head tile — what
  // categorical_policy_loss_bwd and categorical_kl_kernel compute per row
  // (loss_kernels.hip) — then loss + pending-KL partials and the softmax
  // dZ seed.  No pseudo-layer.
  if constexpr (CAT) {
    static_assert(DO_FWD && !BF16 && ROWS <= 64, "categorical seed: fp32 DO_FWD");
    const float* outl = hlds + (L - 1) * ROWS * LDSW;
    const int N = args.dims[L];
    __shared__ float cbuf[64];       // per-row dlogp coeff (ROWS <= 64)
    __shared__ float lbuf[64];       // per-row loss
    __shared__ float kbuf[64];       // per-row pending KL
    __shared__ float sbuf[64];       // per-row log-sum-exp
    __shared__ int abuf[64];         // per-row action index
    const float inv_b = 1.f / (float)args.batch;
    if (tid < ROWS) {
      const int row = row0 + tid;
      float lossr = 0.f, klr = 0.f, c = 0.f, lse = 0.f;
      int a = 0;
      if (row < args.batch) {
        const float* lg = outl + tid * LDSW;
        lse = row_lse(lg, N);
        // clamped: a corrupt action never indexes outside the head tile
        a = min(max((int)gargs.actions[row], 0), N - 1);
        const float logp = lg[a] - lse;
        klr = gargs.old_logp[row] - logp;
        float lr_;
        c = dlogp_coeff(1, logp, gargs.old_logp[row], gargs.adv[row],
                        gargs.clip, &lr_) * inv_b;
        lossr = lr_ * inv_b;
      }
      cbuf[tid] = c;
      lbuf[tid] = lossr;
      kbuf[tid] = klr;
      sbuf[tid] = lse;
      abuf[tid] = a;
    }
    __syncthreads();
    // dZ seed = dlogits (identity head); tail rows have c == 0
    for (int idx = tid; idx < ROWS * N; idx += 256) {
      const int r = idx / N, j = idx % N;
      float v = 0.f;
      if (row0 + r < args.batch) {
        const float p = __expf(outl[r * LDSW + j] - sbuf[r]);
        v = cbuf[r] * (((j == abuf[r]) ? 1.f : 0.f) - p);
      }
      dza[r * LDSW + j] = v;
    }
    // fixed row order: deterministic
    if (tid == 0) {
      float sl = 0.f, sk = 0.f;
      for (int r = 0; r < ROWS; ++r) {
        sl += lbuf[r];
        sk += kbuf[r];
      }
      loss_partials[bx] = sl;
      gargs.kl_partials[bx] = sk;
    }
  } else
  // Gaussian-PPO seed (DO_FWD only): loss + pending-KL + dlog_std
  // partials and the dmean dZ seed, all from the LDS-resident forward
  if (DO_FWD && gargs.actions != nullptr) {
    const float* outl = hlds + (L - 1) * ROWS * LDSW;
    const int D = args.dims[L];
    __shared__ float cbuf[64];       // per-row dlogp coeff (ROWS <= 64)
    __shared__ float lbuf[64];       // per-row loss
    __shared__ float kbuf[64];       // per-row pending KL
    const float inv_b = 1.f / (float)args.batch;
    if (tid < ROWS) {
      const int row = row0 + tid;
      float lossr = 0.f, klr = 0.f, c = 0.f;
      if (row < args.batch) {
        float base = 0.5f * (float)D * LOG_2PI;
        float q = 0.f;
        for (int d = 0; d < D; ++d) {
          const float ls = gargs.log_std[d];
          base += ls;
          const float sg = __expf(ls);
          const float diff =
              gargs.actions[(long)row * D + d] - outl[tid * LDSW + d];
          const float z = diff / sg;
          q += z * z;
        }
        const float logp = -0.5f * q - base;
        klr = gargs.old_logp[row] - logp;
        float lr_;
        c = dlogp_coeff(1, logp, gargs.old_logp[row], gargs.adv[row],
                        gargs.clip, &lr_) * inv_b;
        lossr = lr_ * inv_b;
      }
      cbuf[tid] = c;
      lbuf[tid] = lossr;
      kbuf[tid] = klr;
    }
    __syncthreads();
    // dZ seed = dmean (identity head)
    for (int idx = tid; idx < ROWS * D; idx += 256) {
      const int r = idx / D, d = idx % D;
      const int row = row0 + r;
      float v = 0.f;
      if (row < args.batch) {
        const float inv_s2 = __expf(-2.f * gargs.log_std[d]);
        const float diff =
            gargs.actions[(long)row * D + d] - outl[r * LDSW + d];
        v = cbuf[r] * diff * inv_s2;
      }
      dza[r * LDSW + d] = v;
    }
    // dlog_std partials -> ws pseudo-layer (fixed row order: deterministic)
    if (tid < D) {
      const float inv_s2 = __expf(-2.f * gargs.log_std[tid]);
      float acc = 0.f;
      for (int r = 0; r < ROWS; ++r) {
        const int row = row0 + r;
        if (row < args.batch) {
          const float diff =
              gargs.actions[(long)row * D + tid] - outl[r * LDSW + tid];
          acc += cbuf[r] * (diff * diff * inv_s2 - 1.f);
        }
      }
      wsp[(long)(gargs.dls_off + tid) * WSN] = acc;
    }
    if (tid == 0) {
      float sl = 0.f, sk = 0.f;
      for (int r = 0; r < ROWS; ++r) {
        sl += lbuf[r];
        sk += kbuf[r];
      }
      loss_partials[bx] = sl;
      gargs.kl_partials[bx] = sk;
    }
  } else
  // seed dZ for the last layer: dY * act'(final out), or the fused
  // value-MSE gradient when mse_returns is given
  {
    const int od = args.dims[L];
    const int act = args.acts[L - 1];
    const float* yl = args.h[L - 1];
    const float* yl_lds = hlds + (L - 1) * ROWS * LDSW;
    const float inv_b = 2.f / (float)args.batch;
    float loss_acc = 0.f;
    for (int idx = tid; idx < ROWS * od; idx += 256) {
      int r = idx / od, c = idx % od;
      int row = row0 + r;
      float v = 0.f;
      if (row < args.batch) {
        float yv;
        if constexpr (DO_FWD) {
          yv = yl_lds[r * LDSW + c];
        } else {
          yv = yl[(long)row * od + c];
        }
        if (mse_returns) {
          const float diff = yv - mse_returns[row];
          v = diff * inv_b;
          loss_acc += diff * diff;
        } else {
          v = dy[(long)row * od + c] * act_grad_from_y(act, yv);
        }
      }
      dza[r * LDSW + c] = v;
    }
    if (mse_returns) {
      // deterministic block loss partial (fixed wave order)
      loss_acc = wave_reduce_sum(loss_acc);
      __shared__ float lred[4];
      if ((tid & 63) == 0) lred[tid >> 6] = loss_acc;
      __syncthreads();
      if (tid == 0) {
        loss_partials[bx] =
            ((lred[0] + lred[1]) + (lred[2] + lred[3])) / (float)args.batch;
      }
    }
  }
  __syncthreads();

  const int i = lane & 15;
  const int k = lane >> 4;
  const float* dz_cur = dza;
  float* dz_nxt = dzb;

  for (int l = L - 1; l >= 0; --l) {
    const int in_d = args.dims[l];
    const int out_d = args.dims[l + 1];
    const int wrow = in_d + 1;
    const float* wl = wlds + woffs[l];

    // X_l (input activations of layer l; post-act of layer l-1):
    // DO_FWD reads them straight from the LDS-resident forward
    const float* xl;
    if constexpr (DO_FWD) {
      xl = (l == 0) ? xt : hlds + (l - 1) * ROWS * LDSW;
    } else {
      load_tile<LDSW>(l == 0 ? x : args.h[l - 1], xt, row0, args.batch, in_d, tid, ROWS);
      __syncthreads();
      xl = xt;
    }

    // ---- wgrad partials: dW[i][j] = sum_r dZ[r][i] X[r][j] ----
    // The (it, jt) output tiles are independent, so the flattened tile
    // list is dealt over the four waves (striding `it` alone left layers
    // with out_d <= 32 on one or two waves).  Each tile's MFMA chain is
    // unchanged.
    const int n_it = (out_d + 15) / 16;
    const int n_jt = (in_d + 15) / 16;
    float* lw = wsp + (long)args.layer_off[l] * WSN;
    for (int t = wave; t < n_it * n_jt; t += 4) {
      const int it = t / n_jt;
      const int ii = it * 16 + i;
      {
        const int jt = (t - it * n_jt) * 16;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if constexpr (BF16) {
          for (int k0 = 0; k0 < ROWS; k0 += 32) {
            bf16x8 af, bf;
            #pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int kk = k0 + k * 8 + e;
              af[e] = f32_to_bf16((kk < ROWS && ii < out_d) ? dz_cur[kk * LDSW + ii] : 0.f);
              bf[e] = f32_to_bf16((kk < ROWS && jt + i < in_d) ? xl[kk * LDSW + jt + i] : 0.f);
            }
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc, 0, 0, 0);
          }
        } else {
          for (int k0 = 0; k0 < ROWS; k0 += 4) {
            float a = (ii < out_d) ? dz_cur[(k0 + k) * LDSW + ii] : 0.f;
            float bv = (jt + i < in_d) ? xl[(k0 + k) * LDSW + jt + i] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0);
          }
        }
        const int col = jt + i;
        if (col < in_d) {
          #pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int orow = it * 16 + (lane >> 4) * 4 + r;
            if (orow < out_d) lw[((long)orow * in_d + col) * WSN] = acc[r];
          }
        }
      }
    }
    // bias partial: column c goes to thread 255 - c, i.e. to the last
    // wave, which holds the fewest wgrad tiles whenever the tile count is
    // no multiple of 4 (same serial row order per column)
    for (int c = 255 - tid; c < out_d; c += 256) {
      float s = 0.f;
      #pragma unroll 4
      for (int r = 0; r < ROWS; ++r) s += dz_cur[r * LDSW + c];
      lw[((long)out_d * in_d + c) * WSN] = s;
    }

    // ---- dgrad: dX[b][j] = sum_k dZ[b][k] W[k][j]; for l>0 the next
    // activation-grad is fused from the staged X tile ----
    if (!NEED_DX && l == 0) break;  // nobody reads the input gradient
    const int prev_act = l > 0 ? args.acts[l - 1] : ACT_IDENTITY;
    for (int jt = jt0; jt < in_d; jt += 16 * JT_STRIDE) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const int j = jt + i;
      const bool jok = j < in_d;
      if constexpr (BF16) {
        for (int k0 = 0; k0 < out_d; k0 += 32) {
          bf16x8 af, bf;
          #pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int kk = k0 + k * 8 + e;
            af[e] = f32_to_bf16((kk < out_d) ? dz_cur[(wr0 + i) * LDSW + kk] : 0.f);
            bf[e] = f32_to_bf16((jok && kk < out_d) ? wl[kk * wrow + j] : 0.f);
          }
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc, 0, 0, 0);
        }
      } else {
        for (int k0 = 0; k0 < out_d; k0 += 4) {
          const int kk = k0 + k;
          float a = (kk < out_d) ? dz_cur[(wr0 + i) * LDSW + kk] : 0.f;
          float bv = (jok && kk < out_d) ? wl[kk * wrow + j] : 0.f;
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0);
        }
      }
      if (jok) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = wr0 + (lane >> 4) * 4 + r;
          if (l > 0) {
            const float g = act_grad_from_y(prev_act, xl[row * LDSW + j]);
            dz_nxt[row * LDSW + j] = acc[r] * g;
          } else {
            const int grow = row0 + row;
            if (grow < args.batch) dx_out[(long)grow * in_d + j] = acc[r];
          }
        }
      }
    }
    __syncthreads();
    // swap dz ping-pong
    const float* t = dz_cur;
    dz_cur = dz_nxt;
    dz_nxt = (float*)t;
  }
}

template <int ROWS, bool BF16 = false, bool DO_FWD = false, bool NEED_DX = true,
          bool CAT = false>
__global__ __launch_bounds__(256) void mlp_bwd_fused_f32_t(
    MLPBwdArgs args, const float* __restrict__ x, const float* __restrict__ dy,
    float* __restrict__ dx_out, float* __restrict__ workspace,
    const float* __restrict__ mse_returns, float* __restrict__ loss_partials,
    GaussSeedArgs gargs = GaussSeedArgs{}) {
  extern __shared__ float smem[];
  mlp_bwd_fused_body<ROWS, BF16, DO_FWD, NEED_DX, CAT>(
      args, x, dy, dx_out, workspace, mse_returns, loss_partials, gargs, smem,
      blockIdx.x, gridDim.x);
}

// Twin launch of the PPO update: policy iteration i and value iteration i
// are independent, have the same batch and the same row tiling, and each
// alone fills half the chip, so one grid (fb, 2) runs both — blockIdx.y
// 0 is the PPO policy half (Gaussian seed, or the categorical one in the
// CAT instantiation), 1 the value-MSE half.  Each half is the
// single-net body on its own argument block, workspace and partials; the
// halves share nothing but x.  A gate-frozen policy half returns inside
// the body before its first barrier (blockIdx.y is workgroup-uniform).
template <int ROWS, bool CAT = false>
__global__ __launch_bounds__(256) void mlp_bwd_fused_twin_f32(MLPBwdTwinArgs a) {
  extern __shared__ float smem[];
  if (blockIdx.y == 0) {
    mlp_bwd_fused_body<ROWS, false, true, false, CAT>(
        a.pol, a.x, nullptr, nullptr, a.pol_ws, nullptr, a.pol_loss_partials,
        a.gauss, smem, blockIdx.x, gridDim.x);
  } else {
    mlp_bwd_fused_body<ROWS, false, true, false>(
        a.val, a.x, nullptr, nullptr, a.val_ws, a.returns, a.val_loss_partials,
        GaussSeedArgs{}, smem, blockIdx.x, gridDim.x);
  }
}

// ---------------------------------------------------------------------------
// shape-specialised twin iteration: 3-layer fp32 nets [in, H1, H2, out]
// with compile-time hidden widths (in <= 64 and out <= 16 stay runtime,
// wave-uniform trip counts).  Same arithmetic as mlp_bwd_fused_body<ROWS,
// false, true, false> — every MFMA accumulator sees the same operand
// values in the same k order, the seeds and the bias sums are the same
// expressions — so results are bitwise those of the generic body.  What
// changes is the schedule:
//   * every global load (all three weight matrices, biases, the x tile,
//     the per-row seed inputs) is issued at the top, before the first wait;
//   * the MFMA loops carry no per-lane predicate: the x tile, the head dZ
//     tile and the W images are zero-filled out to the padded k range, so a
//     padded k-step multiplies 0.0f by 0.0f exactly as the masked one did;
//   * a tile's LDS operands are all read ahead of its MFMA chain.
// LDS (floats): five [ROWS][68] tiles (dZ ping-pong, x, h0, h1), the head
// output [ROWS][20], the seed scratch, then the W images with row strides
// = 2 mod 32 (a 16-row x 2-k half-wave read then covers 32 distinct banks).
// ---------------------------------------------------------------------------
#define SHAPED_TS 68   // activation / dZ tile row stride
#define SHAPED_OS 20   // head-output tile row stride (out <= 16)
#define SHAPED_AS 17   // staged actions row stride
#define SHAPED_MAX_OUT 16

template <int ROWS, int H1, int H2>
struct ShapedLds {
  static constexpr int W1S = H1 + 2;
  static constexpr int W2S = H2 + 2;
  static constexpr int DZA = 0;
  static constexpr int DZB = DZA + ROWS * SHAPED_TS;
  static constexpr int XT = DZB + ROWS * SHAPED_TS;
  static constexpr int HID0 = XT + ROWS * SHAPED_TS;
  static constexpr int HID1 = HID0 + ROWS * SHAPED_TS;
  static constexpr int OUT = HID1 + ROWS * SHAPED_TS;
  static constexpr int CBUF = OUT + ROWS * SHAPED_OS;  // c / loss / kl per row
  static constexpr int LRED = CBUF + 3 * ROWS;
  static constexpr int ACT = LRED + 4;
  static constexpr int LSTD = ACT + ROWS * SHAPED_AS;
  static constexpr int W1 = LSTD + SHAPED_MAX_OUT;
  static constexpr int W2 = W1 + H2 * W1S;
  static constexpr int W0 = W2 + SHAPED_MAX_OUT * W2S;  // [H1][w0 stride], last
};

// W0 image row stride: >= roundup4(in) columns, = 2 mod 32
__host__ __device__ inline int shaped_w0_stride(int in_d) {
  return ((in_d + 3) & ~3) <= 32 ? 34 : 66;
}

size_t mlp_bwd_fused_shaped_lds(int in_d) {
  return (size_t)(ShapedLds<32, 64, 32>::W0 + 64 * shaped_w0_stride(in_d)) * 4;
}

// One MFMA chain of NK k-steps.  All
// LDS operands are read first (the scheduling barrier keeps the compiler
// from sinking the reads back between the MFMAs), so the chain pays one
// LDS latency and then counted waits.  ap/bp point at this lane's operand
// of k-step 0; astep/bstep are the float strides between k-steps.
template <int NK>
DEV_INLINE f32x4 shaped_chain1(const float* ap, int astep, const float* bp,
                               int bstep) {
  float a[NK], b[NK];
  #pragma unroll
  for (int s = 0; s < NK; ++s) {
    a[s] = ap[s * astep];
    b[s] = bp[s * bstep];
  }
  __builtin_amdgcn_sched_barrier(0);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  #pragma unroll
  for (int s = 0; s < NK; ++s)
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
  return acc;
}

// Two output tiles of one wave, one chain after the other.  (Interleaving
// the two chains' MFMAs behind one joint read phase was traced 0.3 us per
// launch slower at the bench shape and is not kept.)
template <int NK>
DEV_INLINE void shaped_chain2(const float* ap0, const float* ap1, int astep,
                              const float* bp0, const float* bp1, int bstep,
                              f32x4& acc0, f32x4& acc1) {
  acc0 = shaped_chain1<NK>(ap0, astep, bp0, bstep);
  __builtin_amdgcn_sched_barrier(0);
  acc1 = shaped_chain1<NK>(ap1, astep, bp1, bstep);
}

// bias partial of one layer: column c goes to thread 255 - c (as in the
// generic body), summed over the rows in serial order
template <int ROWS>
DEV_INLINE void shaped_bias_partial(const float* dz, int out_d, int tid,
                                    float* dst, const long WSN) {
  const int c = 255 - tid;
  if (c < out_d) {
    float s = 0.f;
    #pragma unroll
    for (int r = 0; r < ROWS; ++r) s += dz[r * SHAPED_TS + c];
    dst[(long)c * WSN] = s;
  }
}

template <int ROWS, int H1, int H2, bool GAUSS>
DEV_INLINE void mlp_bwd_fused_shaped_body(
    const MLPBwdArgs& args, const float* __restrict__ x,
    float* __restrict__ workspace, const float* __restrict__ mse_returns,
    float* __restrict__ loss_partials, const GaussSeedArgs& gargs, float* smem,
    const int bx, const long WSN) {
  static_assert(ROWS == 32 && H1 == 64 && H2 == 32,
                "wave -> tile maps below assume the <32, 64, 32> shape");
  using LY = ShapedLds<ROWS, H1, H2>;
  constexpr int TS = SHAPED_TS, OS = SHAPED_OS, AS = SHAPED_AS;
  constexpr int W1S = LY::W1S, W2S = LY::W2S;
  float* const dza = smem + LY::DZA;
  float* const dzb = smem + LY::DZB;
  float* const xt = smem + LY::XT;
  float* const h0 = smem + LY::HID0;
  float* const h1 = smem + LY::HID1;
  float* const h2 = smem + LY::OUT;
  float* const cbuf = smem + LY::CBUF;
  float* const lbuf = cbuf + ROWS;
  float* const kbuf = lbuf + ROWS;
  float* const lred = smem + LY::LRED;
  float* const actl = smem + LY::ACT;
  float* const lsl = smem + LY::LSTD;
  float* const w1l = smem + LY::W1;
  float* const w2l = smem + LY::W2;
  float* const w0l = smem + LY::W0;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int i = lane & 15;
  const int k = lane >> 4;
  const int row0 = bx * ROWS;
  const int wr0 = (wave & 1) * 16;   // this wave's row tile (fwd / dgrad)
  const int jt0 = (wave >> 1) * 16;  // and its first column tile
  const int batch = args.batch;
  const int in_d = args.dims[0];
  const int D = args.dims[3];
  const int in4 = (in_d + 3) & ~3;
  const int in16 = (in_d + 15) & ~15;
  const int w0s = shaped_w0_stride(in_d);
  const int act0 = args.acts[0], act1 = args.acts[1], act2 = args.acts[2];
  float* wsp = workspace + bx;  // element-major: ws[elem][block]

  // ---- every global load of the launch, issued back to back ----
  // W0 and the x tile are both [*, in_d] row-major and this block's x rows
  // are contiguous, so flat element idx = tid + 256 u serves both.
  const int n_w0 = H1 * in_d;
  const int n_x = ROWS * in_d;
  const int n_xv = min(ROWS, batch - row0) * in_d;  // rows >= batch read 0
  const float* const xg = x + (long)row0 * in_d;
  float gw0[16], gx[8], gw1[8], gw2[2];
  #pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int idx = tid + 256 * u;
    gw0[u] = idx < n_w0 ? args.w[0][idx] : 0.f;
  }
  #pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int idx = tid + 256 * u;
    gx[u] = idx < n_xv ? xg[idx] : 0.f;
  }
  #pragma unroll
  for (int u = 0; u < 8; ++u) gw1[u] = args.w[1][tid + 256 * u];  // H2*H1 = 2048
  #pragma unroll
  for (int u = 0; u < 2; ++u) {  // image rows >= D are zero
    const int idx = tid + 256 * u;
    gw2[u] = idx < D * H2 ? args.w[2][idx] : 0.f;
  }
  const float b0a = args.b[0][jt0 + i];
  const float b0b = args.b[0][jt0 + 32 + i];
  const float b1v = args.b[1][jt0 + i];
  const float b2v = i < D ? args.b[2][i] : 0.f;
  // seed inputs: thread tid < ROWS owns row tid; thread (ar, ad) owns
  // elements (ar, ad) and (ar + 16, ad) of the [ROWS][16] head tiles
  const int ar = tid >> 4, ad = tid & 15;
  float olp = 0.f, advv = 0.f, retv = 0.f, ga0 = 0.f, ga1 = 0.f, lsv = 0.f;
  if constexpr (GAUSS) {
    if (tid < ROWS && row0 + tid < batch) {
      olp = gargs.old_logp[row0 + tid];
      advv = gargs.adv[row0 + tid];
    }
    if (ad < D) {
      if (row0 + ar < batch) ga0 = gargs.actions[(long)(row0 + ar) * D + ad];
      if (row0 + ar + 16 < batch)
        ga1 = gargs.actions[(long)(row0 + ar + 16) * D + ad];
    }
    if (tid < D) lsv = gargs.log_std[tid];
  } else {
    if (tid < ROWS && row0 + tid < batch) retv = mse_returns[row0 + tid];
  }
  // gate-frozen PPO iteration: a no-op by definition (see the generic body)
  if (GAUSS && gargs.skip_gate != nullptr && *gargs.skip_gate == 0.f) return;

  // ---- stage to LDS ----
  {
    // (r, c) of idx = tid, then stepped by 256 elements without dividing
    int r = tid / in_d, c = tid - r * in_d;
    const int qs = 256 / in_d, rs = 256 - qs * in_d;
    #pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int idx = tid + 256 * u;
      if (idx < n_w0) w0l[r * w0s + c] = gw0[u];
      if (u < 8 && idx < n_x) xt[r * TS + c] = gx[u < 8 ? u : 0];
      c += rs;
      r += qs;
      if (c >= in_d) {
        c -= in_d;
        ++r;
      }
    }
    // zero pads: W0 columns [in_d, in4) and x columns [in_d, in16)
    if (tid < H1) {
      for (int cc = in_d; cc < in4; ++cc) w0l[tid * w0s + cc] = 0.f;
    } else if (tid < H1 + 4 * ROWS) {
      const int rr = (tid - H1) >> 2;
      for (int cc = in_d + ((tid - H1) & 3); cc < in16; cc += 4)
        xt[rr * TS + cc] = 0.f;
    }
    #pragma unroll
    for (int u = 0; u < 8; ++u)
      w1l[((tid >> 6) + 4 * u) * W1S + (tid & 63)] = gw1[u];
    #pragma unroll
    for (int u = 0; u < 2; ++u)
      w2l[((tid >> 5) + 8 * u) * W2S + (tid & 31)] = gw2[u];
    if constexpr (GAUSS) {
      actl[ar * AS + ad] = ga0;
      actl[(ar + 16) * AS + ad] = ga1;
      if (tid < SHAPED_MAX_OUT) lsl[tid] = lsv;
    }
  }
  __syncthreads();

  // ---- forward layer 0: two column tiles per wave ----
  {
    const int nk = in4 >> 2;
    const float* ap = xt + (wr0 + i) * TS + k;
    const float* bp0 = w0l + (jt0 + i) * w0s + k;
    const float* bp1 = bp0 + 32 * w0s;
    f32x4 acc0, acc1;
    // wave-uniform dispatch on the k-step count: straight-line chains
#define SHAPED_FWD0(N) \
  case N: shaped_chain2<N>(ap, ap, 4, bp0, bp1, 4, acc0, acc1); break;
    switch (nk) {
      SHAPED_FWD0(1) SHAPED_FWD0(2) SHAPED_FWD0(3) SHAPED_FWD0(4)
      SHAPED_FWD0(5) SHAPED_FWD0(6) SHAPED_FWD0(7) SHAPED_FWD0(8)
      SHAPED_FWD0(9) SHAPED_FWD0(10) SHAPED_FWD0(11) SHAPED_FWD0(12)
      SHAPED_FWD0(13) SHAPED_FWD0(14) SHAPED_FWD0(15)
      default: shaped_chain2<16>(ap, ap, 4, bp0, bp1, 4, acc0, acc1); break;
    }
#undef SHAPED_FWD0
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = wr0 + k * 4 + r;
      h0[rr * TS + jt0 + i] = act_apply(act0, acc0[r] + b0a);
      h0[rr * TS + jt0 + 32 + i] = act_apply(act0, acc1[r] + b0b);
    }
  }
  __syncthreads();
  // ---- forward layer 1: one tile per wave, K = H1 ----
  {
    const float* ap = h0 + (wr0 + i) * TS + k;
    const float* bp = w1l + (jt0 + i) * W1S + k;
    const f32x4 acc = shaped_chain1<H1 / 4>(ap, 4, bp, 4);
    #pragma unroll
    for (int r = 0; r < 4; ++r)
      h1[(wr0 + k * 4 + r) * TS + jt0 + i] = act_apply(act1, acc[r] + b1v);
  }
  __syncthreads();
  // ---- forward layer 2 (head, out <= 16: one column tile, waves 0-1) ----
  if (jt0 == 0) {
    const float* ap = h1 + (wr0 + i) * TS + k;
    const float* bp = w2l + i * W2S + k;
    const f32x4 acc = shaped_chain1<H2 / 4>(ap, 4, bp, 4);
    if (i < D) {
      #pragma unroll
      for (int r = 0; r < 4; ++r)
        h2[(wr0 + k * 4 + r) * OS + i] = act_apply(act2, acc[r] + b2v);
    }
  }
  __syncthreads();

  // ---- seed the head dZ tile [ROWS][16] (columns >= D are zero) ----
  if constexpr (GAUSS) {
    // Gaussian-PPO seed: loss + pending-KL + dlog_std partials and dmean
    const float inv_b = 1.f / (float)batch;
    if (tid < ROWS) {
      const int row = row0 + tid;
      float lossr = 0.f, klr = 0.f, c = 0.f;
      if (row < batch) {
        float base = 0.5f * (float)D * LOG_2PI;
        float q = 0.f;
        for (int d = 0; d < D; ++d) {
          const float ls = lsl[d];
          base += ls;
          const float sg = __expf(ls);
          const float diff = actl[tid * AS + d] - h2[tid * OS + d];
          const float z = diff / sg;
          q += z * z;
        }
        const float logp = -0.5f * q - base;
        klr = olp - logp;
        float lr_;
        c = dlogp_coeff(1, logp, olp, advv, gargs.clip, &lr_) * inv_b;
        lossr = lr_ * inv_b;
      }
      cbuf[tid] = c;
      lbuf[tid] = lossr;
      kbuf[tid] = klr;
    }
    __syncthreads();
    #pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = ar + 16 * h;
      float v = 0.f;
      if (ad < D && row0 + r < batch) {
        const float inv_s2 = __expf(-2.f * lsl[ad]);
        const float diff = actl[r * AS + ad] - h2[r * OS + ad];
        v = cbuf[r] * diff * inv_s2;
      }
      dza[r * TS + ad] = v;
    }
    // the two serial sums sit on waves that hold no head wgrad tile:
    // dlog_std partials -> ws pseudo-layer (fixed row order), wave 2
    if (tid >= 128 && tid - 128 < D) {
      const int d = tid - 128;
      const float inv_s2 = __expf(-2.f * lsl[d]);
      float acc = 0.f;
      for (int r = 0; r < ROWS; ++r) {
        if (row0 + r < batch) {
          const float diff = actl[r * AS + d] - h2[r * OS + d];
          acc += cbuf[r] * (diff * diff * inv_s2 - 1.f);
        }
      }
      wsp[(long)(gargs.dls_off + d) * WSN] = acc;
    }
    if (tid == 192) {  // wave 3
      float sl = 0.f, sk = 0.f;
      for (int r = 0; r < ROWS; ++r) {
        sl += lbuf[r];
        sk += kbuf[r];
      }
      loss_partials[bx] = sl;
      gargs.kl_partials[bx] = sk;
    }
  } else {
    // value-MSE seed (out == 1): dZ = 2 (v - ret) / B, block loss partial
    const float inv_b = 2.f / (float)batch;
    float loss_acc = 0.f;
    if (ad >= 1) {
      dza[ar * TS + ad] = 0.f;
      dza[(ar + 16) * TS + ad] = 0.f;
    }
    if (tid < ROWS) {
      float v = 0.f;
      if (row0 + tid < batch) {
        const float diff = h2[tid * OS] - retv;
        v = diff * inv_b;
        loss_acc += diff * diff;
      }
      dza[tid * TS] = v;
    }
    // deterministic block loss partial (fixed wave order)
    loss_acc = wave_reduce_sum(loss_acc);
    if (lane == 0) lred[wave] = loss_acc;
  }
  __syncthreads();
  if (!GAUSS && tid == 0) {
    loss_partials[bx] =
        ((lred[0] + lred[1]) + (lred[2] + lred[3])) / (float)batch;
  }

  // ---- layer 2 backward: wgrad (out x H2: tiles on waves 0-1), bias
  // partial, dgrad into dzb with tanh'/relu' of h1 fused ----
  {
    float* lw = wsp + (long)args.layer_off[2] * WSN;
    if (wave < 2) {
      const int jt = wave * 16;
      const f32x4 acc = shaped_chain1<ROWS / 4>(dza + k * TS + i, 4 * TS,
                                                h1 + k * TS + jt + i, 4 * TS);
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int orow = k * 4 + r;
        if (orow < D) lw[((long)orow * H2 + jt + i) * WSN] = acc[r];
      }
    }
    shaped_bias_partial<ROWS>(dza, D, tid, lw + (long)D * H2 * WSN, WSN);

    const int nk = (D + 3) >> 2;  // <= 4
    const int j = jt0 + i;
    const float* ap = dza + (wr0 + i) * TS + k;
    const float* bp = w2l + k * W2S + j;
    f32x4 acc;
    switch (nk) {
      case 1: acc = shaped_chain1<1>(ap, 4, bp, 4 * W2S); break;
      case 2: acc = shaped_chain1<2>(ap, 4, bp, 4 * W2S); break;
      case 3: acc = shaped_chain1<3>(ap, 4, bp, 4 * W2S); break;
      default: acc = shaped_chain1<4>(ap, 4, bp, 4 * W2S); break;
    }
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = wr0 + k * 4 + r;
      dzb[rr * TS + j] = acc[r] * act_grad_from_y(act1, h1[rr * TS + j]);
    }
  }
  __syncthreads();

  // ---- layer 1 backward: wgrad (H2 x H1: two tiles per wave sharing the
  // X operand), bias partial, dgrad (two column tiles) into dza ----
  {
    float* lw = wsp + (long)args.layer_off[1] * WSN;
    {
      const int jt = wave * 16;
      const float* bp = h0 + k * TS + jt + i;
      f32x4 acc0, acc1;
      shaped_chain2<ROWS / 4>(dzb + k * TS + i, dzb + k * TS + 16 + i, 4 * TS,
                              bp, bp, 4 * TS, acc0, acc1);
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int orow = k * 4 + r;
        lw[((long)orow * H1 + jt + i) * WSN] = acc0[r];
        lw[((long)(orow + 16) * H1 + jt + i) * WSN] = acc1[r];
      }
    }
    shaped_bias_partial<ROWS>(dzb, H2, tid, lw + (long)H2 * H1 * WSN, WSN);

    const int j = jt0 + i;
    const float* ap = dzb + (wr0 + i) * TS + k;
    const float* bp = w1l + k * W1S + j;
    f32x4 acc0, acc1;
    shaped_chain2<H2 / 4>(ap, ap, 4, bp, bp + 32, 4 * W1S, acc0, acc1);
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = wr0 + k * 4 + r;
      dza[rr * TS + j] = acc0[r] * act_grad_from_y(act0, h0[rr * TS + j]);
      dza[rr * TS + j + 32] =
          acc1[r] * act_grad_from_y(act0, h0[rr * TS + j + 32]);
    }
  }
  __syncthreads();

  // ---- layer 0 backward: wgrad only (H1 x in_d; nobody reads dX).  The
  // 4 * n_jt tiles are dealt over the waves as in the generic body, t =
  // wave + 4 m ----
  {
    float* lw = wsp + (long)args.layer_off[0] * WSN;
    const int n_jt = in16 >> 4;  // 1..4
    auto tile_it = [n_jt](int t) {
      return n_jt == 1 ? t : n_jt == 2 ? t >> 1 : n_jt == 3 ? t / 3 : t >> 2;
    };
    auto store = [&](const f32x4& acc, int it, int jt) {
      const int col = jt + i;
      if (col < in_d) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int orow = it * 16 + k * 4 + r;
          lw[((long)orow * in_d + col) * WSN] = acc[r];
        }
      }
    };
    for (int m = 0; m < n_jt; m += 2) {
      const int t0 = wave + 4 * m;
      const int it0 = tile_it(t0), jtA = (t0 - it0 * n_jt) * 16;
      if (m + 1 < n_jt) {
        const int t1 = t0 + 4;
        const int it1 = tile_it(t1), jtB = (t1 - it1 * n_jt) * 16;
        f32x4 acc0, acc1;
        shaped_chain2<ROWS / 4>(dza + k * TS + it0 * 16 + i,
                                dza + k * TS + it1 * 16 + i, 4 * TS,
                                xt + k * TS + jtA + i, xt + k * TS + jtB + i,
                                4 * TS, acc0, acc1);
        store(acc0, it0, jtA);
        store(acc1, it1, jtB);
      } else {
        const f32x4 acc =
            shaped_chain1<ROWS / 4>(dza + k * TS + it0 * 16 + i, 4 * TS,
                                    xt + k * TS + jtA + i, 4 * TS);
        store(acc, it0, jtA);
      }
    }
    shaped_bias_partial<ROWS>(dza, H1, tid, lw + (long)H1 * in_d * WSN, WSN);
  }
}

// The twin launch on the shaped body: grid (fb, 2), blockIdx.y 0 the
// Gaussian-PPO half, 1 the value-MSE half, same argument block, workspace
// layout and partials as mlp_bwd_fused_twin_f32<32>.
__global__ __launch_bounds__(256) void mlp_bwd_fused_twin_shaped_f32(
    MLPBwdTwinArgs a) {
  extern __shared__ float smem[];
  if (blockIdx.y == 0) {
    mlp_bwd_fused_shaped_body<32, 64, 32, true>(
        a.pol, a.x, a.pol_ws, nullptr, a.pol_loss_partials, a.gauss, smem,
        blockIdx.x, gridDim.x);
  } else {
    mlp_bwd_fused_shaped_body<32, 64, 32, false>(
        a.val, a.x, a.val_ws, a.returns, a.val_loss_partials, GaussSeedArgs{},
        smem, blockIdx.x, gridDim.x);
  }
}

// ---------------------------------------------------------------------------
// wide-net single-layer kernels: 2D grids (row blocks x 64-col groups).
// The fused multi-layer kernel keeps every output column of a row tile
// in one block, which leaves most of the chip idle for [*,256,256,*]
// nets at minibatch-sized inputs (DDPG/TD3's 100-row hot path); these
// per-layer kernels spread the column dimension across blocks instead.
// ---------------------------------------------------------------------------
template <int ROWS>
__global__ __launch_bounds__(256) void mlp_layer_fwd_wide_f32(
    const float* __restrict__ x, const float* __restrict__ W,
    const float* __restrict__ B, float* __restrict__ out, int batch, int in_d,
    int out_d, int act) {
  constexpr int LDSW = 256 + 4;
  extern __shared__ float smem[];  // x tile [ROWS][LDSW]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int row0 = blockIdx.x * ROWS;
  const int jt = blockIdx.y * 64 + wave * 16;  // one 16-col tile per wave

  load_tile<LDSW>(x, smem, row0, batch, in_d, tid, ROWS);
  __syncthreads();
  if (jt >= out_d) return;

  const int i = lane & 15;
  const int k = lane >> 4;
  const int j = jt + i;
  const bool jok = j < out_d;
  const float bias = jok ? B[j] : 0.f;
  const float* wrow = W + (long)j * in_d;
  for (int rt = 0; rt < ROWS; rt += 16) {
    // the K loop shared with the persistent collect kernel (rollout_steps.h)
    const f32x4 acc = mlp_fwd_tile_wide<LDSW>(smem + rt * LDSW, wrow, in_d, i, k, jok);
    if (jok) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + rt + (lane >> 4) * 4 + r;
        if (row < batch) out[(long)row * out_d + j] = act_apply(act, acc[r] + bias);
      }
    }
  }
}

DEV_INLINE void dgrad_wide_body(
    float* __restrict__ smem, const float* __restrict__ dy,
    const float* __restrict__ y, const float* __restrict__ W,
    float* __restrict__ dx, int batch, int out_d, int in_d, int act,
    int bx, int by, int ROWS) {
  constexpr int LDSW = 256 + 4;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int row0 = bx * ROWS;
  const int jt = by * 64 + wave * 16;  // over in_d

  for (int idx = tid; idx < ROWS * out_d; idx += 256) {
    int r = idx / out_d, c = idx % out_d;
    int row = row0 + r;
    float v = 0.f;
    if (row < batch) {
      long g = (long)row * out_d + c;
      v = dy[g] * act_grad_from_y(act, y[g]);
    }
    smem[r * LDSW + c] = v;
  }
  __syncthreads();
  if (jt >= in_d) return;

  const int i = lane & 15;
  const int k = lane >> 4;
  const int j = jt + i;
  const bool jok = j < in_d;
  const int od8 = out_d & ~7;
  for (int rt = 0; rt < ROWS; rt += 16) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < od8; k0 += 8) {
      const float a0 = smem[(rt + i) * LDSW + k0 + k];
      const float a1 = smem[(rt + i) * LDSW + k0 + 4 + k];
      float bv0 = jok ? W[(long)(k0 + k) * in_d + j] : 0.f;
      float bv1 = jok ? W[(long)(k0 + 4 + k) * in_d + j] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv0, acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv1, acc2, 0, 0, 0);
    }
    for (int k0 = od8; k0 < out_d; k0 += 4) {
      const int kk = k0 + k;
      float a = (kk < out_d) ? smem[(rt + i) * LDSW + kk] : 0.f;
      float bv = (jok && kk < out_d) ? W[(long)kk * in_d + j] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0);
    }
    acc[0] += acc2[0]; acc[1] += acc2[1]; acc[2] += acc2[2]; acc[3] += acc2[3];
    if (jok) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + rt + (lane >> 4) * 4 + r;
        if (row < batch) dx[(long)row * in_d + j] = acc[r];
      }
    }
  }
}

template <int ROWS>
__global__ __launch_bounds__(256) void mlp_dgrad_wide_f32(
    const float* __restrict__ dy, const float* __restrict__ y,
    const float* __restrict__ W, float* __restrict__ dx, int batch, int out_d,
    int in_d, int act) {
  extern __shared__ float smem[];
  dgrad_wide_body(smem, dy, y, W, dx, batch, out_d, in_d, act, blockIdx.x,
                  blockIdx.y, ROWS);
}

// wgrad + bias partials, columns of dW's out dimension split over
// blockIdx.y (disjoint writes into the same per-row-block partial row)
DEV_INLINE void wgrad_wide_body(
    float* __restrict__ smem, const float* __restrict__ dy,
    const float* __restrict__ y, const float* __restrict__ xin,
    float* __restrict__ workspace, long ws_stride, int batch, int out_d,
    int in_d, int act, int bx, int by, int ROWS) {
  constexpr int LDSW = 256 + 4;
  constexpr int DZW = 64 + 4;
  float* xt = smem;
  float* dz = smem + ROWS * LDSW;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int row0 = bx * ROWS;
  const int og0 = by * 64;  // out-col group
  float* wsp = workspace + bx;  // element-major: ws[elem][block]
  const long WSN = gridDim.x;

  load_tile<LDSW>(xin, xt, row0, batch, in_d, tid, ROWS);
  const int og_w = min(64, out_d - og0);
  for (int idx = tid; idx < ROWS * og_w; idx += 256) {
    int r = idx / og_w, c = idx % og_w;
    int row = row0 + r;
    float v = 0.f;
    if (row < batch) {
      long g = (long)row * out_d + og0 + c;
      v = dy[g] * act_grad_from_y(act, y[g]);
    }
    dz[r * DZW + c] = v;
  }
  __syncthreads();

  const int i = lane & 15;
  const int k = lane >> 4;
  const int ii = wave * 16 + i;       // dz slice col (out index og0+ii)
  const bool iok = og0 + ii < out_d;
  for (int jt = 0; jt < in_d; jt += 16) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < ROWS; k0 += 4) {
      float a = iok ? dz[(k0 + k) * DZW + ii] : 0.f;
      float bv = (jt + i < in_d) ? xt[(k0 + k) * LDSW + jt + i] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc, 0, 0, 0);
    }
    const int col = jt + i;
    if (col < in_d) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int orow = og0 + wave * 16 + (lane >> 4) * 4 + r;
        if (orow < out_d) wsp[((long)orow * in_d + col) * WSN] = acc[r];
      }
    }
  }

  __syncthreads();
  for (int c = tid; c < og_w; c += 256) {
    float s = 0.f;
    #pragma unroll 4
    for (int r = 0; r < ROWS; ++r) s += dz[r * DZW + c];
    wsp[((long)out_d * in_d + og0 + c) * WSN] = s;
  }
}

template <int ROWS>
__global__ __launch_bounds__(256) void mlp_wgrad_wide_f32(
    const float* __restrict__ dy, const float* __restrict__ y,
    const float* __restrict__ xin, float* __restrict__ workspace,
    long ws_stride, int batch, int out_d, int in_d, int act) {
  extern __shared__ float smem[];
  wgrad_wide_body(smem, dy, y, xin, workspace, ws_stride, batch, out_d, in_d,
                  act, blockIdx.x, blockIdx.y, ROWS);
}

// dgrad and wgrad of one layer are independent given dZ: one launch with
// blockIdx.z selecting the family doubles the resident block pool (the
// per-family grids are 16ish blocks at minibatch scale — far below the
// 256-CU chip) instead of serializing two launches on the stream
template <int ROWS>
__global__ __launch_bounds__(256) void mlp_bwd_wide_both_f32(
    const float* __restrict__ dy, const float* __restrict__ y,
    const float* __restrict__ xin, const float* __restrict__ W,
    float* __restrict__ dx, float* __restrict__ workspace, long ws_stride,
    int batch, int out_d, int in_d, int act) {
  extern __shared__ float smem[];
  if (blockIdx.z == 0) {
    if ((int)blockIdx.y * 64 < in_d)
      dgrad_wide_body(smem, dy, y, W, dx, batch, out_d, in_d, act, blockIdx.x,
                      blockIdx.y, ROWS);
  } else {
    if ((int)blockIdx.y * 64 < out_d)
      wgrad_wide_body(smem, dy, y, xin, workspace, ws_stride, batch, out_d,
                      in_d, act, blockIdx.x, blockIdx.y, ROWS);
  }
}

// host-side dispatch over the instantiations — called from bindings.hip so
// template symbols stay in this translation unit.  The whole-net backward
// runs 32-row blocks only (BWD_FUSED_ROWS, bindings.hip).
template <bool BF16, bool DO_FWD>
static void launch_mlp_bwd_fused_t(bool need_dx, const MLPBwdArgs& args,
                                   const float* x, const float* dy, float* dx,
                                   float* ws, const float* mse_returns,
                                   float* loss_partials, size_t lds_bytes,
                                   int n_blocks, hipStream_t stream,
                                   const GaussSeedArgs& gargs) {
  if (need_dx)
    hipLaunchKernelGGL((mlp_bwd_fused_f32_t<32, BF16, DO_FWD, true>),
                       dim3(n_blocks), dim3(256), lds_bytes, stream, args, x,
                       dy, dx, ws, mse_returns, loss_partials, gargs);
  else
    hipLaunchKernelGGL((mlp_bwd_fused_f32_t<32, BF16, DO_FWD, false>),
                       dim3(n_blocks), dim3(256), lds_bytes, stream, args, x,
                       dy, dx, ws, mse_returns, loss_partials, gargs);
}

// need_dx == 0: dx may be nullptr (the kernel neither computes nor stores
// the input gradient)
void launch_mlp_bwd_fused(const MLPBwdArgs& args, const float* x,
                          const float* dy, float* dx, float* ws,
                          const float* mse_returns, float* loss_partials,
                          size_t lds_bytes, int n_blocks, int compute_bf16,
                          hipStream_t stream, int do_fwd, GaussSeedArgs gargs,
                          int need_dx) {
  const bool ndx = need_dx != 0;
#define BWD_FUSED_ARGS \
  ndx, args, x, dy, dx, ws, mse_returns, loss_partials, lds_bytes, n_blocks, \
      stream, gargs
  // the in-kernel forward is fp32 only (host gates); the categorical seed
  // is an instantiation of its own, so the Gaussian / value code is
  // untouched by it
  if (do_fwd && gargs.kind == SEED_CATEGORICAL) {
    hipLaunchKernelGGL((mlp_bwd_fused_f32_t<32, false, true, false, true>),
                       dim3(n_blocks), dim3(256), lds_bytes, stream, args, x,
                       dy, dx, ws, mse_returns, loss_partials, gargs);
  } else if (do_fwd) launch_mlp_bwd_fused_t<false, true>(BWD_FUSED_ARGS);
  else if (compute_bf16) launch_mlp_bwd_fused_t<true, false>(BWD_FUSED_ARGS);
  else launch_mlp_bwd_fused_t<false, false>(BWD_FUSED_ARGS);
#undef BWD_FUSED_ARGS
}

// lds_bytes: the larger of the two halves' budgets; grid (n_blocks, 2)
void launch_mlp_bwd_fused_twin(const MLPBwdTwinArgs& a, size_t lds_bytes,
                               int n_blocks, hipStream_t stream) {
  if (a.gauss.kind == SEED_CATEGORICAL)
    hipLaunchKernelGGL((mlp_bwd_fused_twin_f32<32, true>), dim3(n_blocks, 2),
                       dim3(256), lds_bytes, stream, a);
  else
    hipLaunchKernelGGL((mlp_bwd_fused_twin_f32<32>), dim3(n_blocks, 2),
                       dim3(256), lds_bytes, stream, a);
}

// Both nets must be [in <= 64, 64, 32, out <= 16] fp32 on 32-row blocks
// (the caller checks); LDS is mlp_bwd_fused_shaped_lds(in).
void launch_mlp_bwd_fused_twin_shaped(const MLPBwdTwinArgs& a, int n_blocks,
                                      hipStream_t stream) {
  hipLaunchKernelGGL(mlp_bwd_fused_twin_shaped_f32, dim3(n_blocks, 2),
                     dim3(256), mlp_bwd_fused_shaped_lds(a.pol.dims[0]), stream,
                     a);
}

void launch_mlp_layer_fwd_wide(const float* x, const float* W, const float* B,
                               float* out, int batch, int in_d, int out_d,
                               int act, hipStream_t stream) {
  constexpr int ROWS = 32;
  dim3 g((batch + ROWS - 1) / ROWS, (out_d + 63) / 64), b(256);
  size_t lds = (size_t)ROWS * (256 + 4) * 4;
  hipLaunchKernelGGL((mlp_layer_fwd_wide_f32<ROWS>), g, b, lds, stream, x, W, B,
                     out, batch, in_d, out_d, act);
}

void launch_mlp_bwd_wide(const float* dy, const float* y, const float* xin,
                         const float* W, float* dx, float* ws, long ws_stride,
                         int batch, int out_d, int in_d, int act,
                         hipStream_t stream) {
  constexpr int ROWS = 32;
  const int rb = (batch + ROWS - 1) / ROWS;
  const int it = (in_d + 63) / 64, ot = (out_d + 63) / 64;
  const int yt = it > ot ? it : ot;
  size_t lds = (size_t)ROWS * (256 + 4 + 64 + 4) * 4;  // max of both bodies
  hipLaunchKernelGGL((mlp_bwd_wide_both_f32<ROWS>), dim3(rb, yt, 2), dim3(256),
                     lds, stream, dy, y, xin, W, dx, ws, ws_stride, batch,
                     out_d, in_d, act);
}

// dgrad chain only (input gradient without weight-grad partials) — the
// actor step's path through the frozen critic
void launch_mlp_dgrad_wide(const float* dy, const float* y, const float* W,
                           float* dx, int batch, int out_d, int in_d, int act,
                           hipStream_t stream) {
  constexpr int ROWS = 32;
  const int rb = (batch + ROWS - 1) / ROWS;
  size_t lds1 = (size_t)ROWS * (256 + 4) * 4;
  hipLaunchKernelGGL((mlp_dgrad_wide_f32<ROWS>), dim3(rb, (in_d + 63) / 64),
                     dim3(256), lds1, stream, dy, y, W, dx, batch, out_d, in_d,
                     act);
}

// narrow nets only (widths <= 64); rows in {16, 32, 64}
void launch_mlp_fwd(const MLPArgs& args, const float* x, int save_hidden,
                    int rows, int n_blocks, size_t lds_bytes, int compute_bf16,
                    hipStream_t stream) {
  dim3 g(n_blocks), b(256);
#define FWD_LAUNCH(ROWS, BF16)                                               \
  hipLaunchKernelGGL((fused_mlp_fwd_f32_t<ROWS, 64, BF16>), g, b, lds_bytes, \
                     stream, args, x, save_hidden)
  if (compute_bf16) {
    if (rows == 16) FWD_LAUNCH(16, true);
    else if (rows == 32) FWD_LAUNCH(32, true);
    else FWD_LAUNCH(64, true);
  } else {
    if (rows == 16) FWD_LAUNCH(16, false);
    else if (rows == 32) FWD_LAUNCH(32, false);
    else FWD_LAUNCH(64, false);
  }
#undef FWD_LAUNCH
}

// narrow nets only (widths <= 64); rows in {32, 64}
void launch_mlp_bwd_layer(const float* dy, const float* y, const float* xin,
                          const float* W, float* dx, float* ws, long ws_stride,
                          int batch, int out_d, int in_d, int act, int rows,
                          int n_blocks, size_t lds_bytes, hipStream_t stream) {
  dim3 g(n_blocks), b(256);
  if (rows == 32)
    hipLaunchKernelGGL((mlp_bwd_layer_f32_t<32, 64>), g, b, lds_bytes, stream,
                       dy, y, xin, W, dx, ws, ws_stride, batch, out_d, in_d, act);
  else
    hipLaunchKernelGGL((mlp_bwd_layer_f32_t<64, 64>), g, b, lds_bytes, stream,
                       dy, y, xin, W, dx, ws, ws_stride, batch, out_d, in_d, act);
}

// ---------------------------------------------------------------------------
// deterministic split-K partial reduction
// one-pass variant: 256 threads = 64 elements x 4 partial-quarters,
// combined through LDS in fixed order — one launch even at 125 partials
// reduce + Adam in one pass: identical fixed-order partial summation to
// mlp_grad_reduce_onepass_f32, but the summed gradient feeds the Adam
// update (same math as fused_adam_kernel) directly — no dw/db tensors.
// ---------------------------------------------------------------------------

// Gate prologue of the reduce+Adam kernels; returns true when this
// workgroup must leave its Adam slice untouched.  Without kl_partials it
// is the plain "skip while *gate == 0" test.  With them (the mega PPO
// policy iteration) EVERY workgroup redoes the one-thread bookkeeping of
// the former gate-reduce kernel — the per-block partials are staged
// through LDS and thread 0 adds them in block order, the same serial
// order as before — and gates its own slice on the result, so no kernel
// boundary is needed between the decision and the update.  Only
// workgroup 0 writes gate / kl_final / iters_done / loss_out.
//
// Workgroups of one launch may read the gate before or after workgroup 0
// closes it.  Both views lead to the same decision: workgroup 0 closes
// the gate only when kl > thr, and kl is a pure function of kl_partials
// (final before this launch starts), summed in the same order by every
// workgroup.  One that still sees the gate open therefore computes the
// same kl, finds kl > thr and skips its slice; one that already sees it
// closed skips its slice too.  Workgroup 0's own threads read the gate
// before the first barrier below and thread 0 writes it after that
// barrier, so its bookkeeping always acts on the value at entry.
DEV_INLINE bool reduce_adam_gate_closed(const ReduceAdamArgs& a, float* stage,
                                        const int wg) {
  const float g_in = a.gate ? *a.gate : 1.f;
  if (a.kl_partials == nullptr) return g_in == 0.f;
  const int tid = threadIdx.x;
  // closed on entry: nothing changes (the partials are stale then — the
  // fused iteration kernel returned at once).  The first iteration never
  // gates and always records its loss.
  if (!a.first_iter && g_in == 0.f) return true;
  if (a.first_iter && wg != 0) return g_in == 0.f;
  const float* part = a.first_iter ? a.loss_partials : a.kl_partials;
  float acc = 0.f;  // thread 0's running sum
  for (int base = 0; base < a.n_blocks; base += 256) {
    const int cnt = min(256, a.n_blocks - base);
    if (tid < cnt) stage[tid] = part[base + tid];
    __syncthreads();
    if (tid == 0) {
      for (int j = 0; j < cnt; ++j) acc += stage[j];
    }
    __syncthreads();
  }
  if (a.first_iter) {
    if (tid == 0) *a.loss_out = acc;  // no pending KL at iteration 0
    return g_in == 0.f;
  }
  if (tid == 0) {
    const float kl = acc * a.inv_b;
    const bool close = kl > a.thr;
    if (wg == 0) {
      *a.kl_final = kl;
      *a.iters_done += 1.f;
      if (close) *a.gate_rw = 0.f;
    }
    stage[0] = close ? 1.f : 0.f;
  }
  __syncthreads();
  const bool closed = stage[0] != 0.f;
  __syncthreads();  // the caller reuses stage
  return closed;
}

__global__ __launch_bounds__(256) void mlp_grad_reduce_adam_f32(ReduceAdamArgs a) {
  __shared__ float red[256];
  if (reduce_adam_gate_closed(a, red, blockIdx.x)) return;
  int grand = 0;
  int base[MLP_MAX_LAYERS];
  for (int l = 0; l < a.n_layers; ++l) {
    base[l] = grand;
    grand += a.total[l];
  }
  const float s0 = a.step[0] + 1.f + a.step_delta;
  const float bc1 = 1.f - __powf(a.beta1, s0);
  const float bc2 = 1.f - __powf(a.beta2, s0);
  const int e_local = threadIdx.x & 63;
  const int quarter = threadIdx.x >> 6;
  const int chunk = (a.n_blocks + 3) / 4;
  const int p0 = quarter * chunk;
  const int p1 = min(p0 + chunk, a.n_blocks);
  for (int g0 = blockIdx.x * 64; g0 < grand; g0 += gridDim.x * 64) {
    const int g = g0 + e_local;
    float s = 0.f;
    if (g < grand) {
      for (int p = p0; p < p1; ++p) s += a.ws[(long)g * a.n_blocks + p];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (quarter == 0 && g < grand) {
      float grad = (red[e_local] + red[64 + e_local]) +
                   (red[128 + e_local] + red[192 + e_local]);
      int l = 0;
      while (l + 1 < a.n_layers && g >= base[l + 1]) ++l;
      int idx = g - base[l];
      float *p, *m, *v;
      if (idx < a.wsize[l]) {
        p = a.pw[l]; m = a.mw[l]; v = a.vw[l];
      } else {
        idx -= a.wsize[l];
        p = a.pb[l]; m = a.mb[l]; v = a.vb[l];
      }
      if (a.weight_decay != 0.f) grad += a.weight_decay * p[idx];
      const float mi = a.beta1 * m[idx] + (1.f - a.beta1) * grad;
      const float vi = a.beta2 * v[idx] + (1.f - a.beta2) * grad * grad;
      m[idx] = mi;
      v[idx] = vi;
      p[idx] -= a.lr * (mi / bc1) / (sqrtf(vi / bc2) + a.eps);
    }
    __syncthreads();
  }
}

// LDS-staged reduce+Adam for small partial counts.  In the element-major
// workspace the partial rows of EPB consecutive elements are ONE
// contiguous run of EPB * n_blocks floats, so the workgroup copies that
// run into LDS with coalesced 16-byte loads (the direct kernel above has
// every lane walk its own row, 4 bytes at a time, n_blocks * 4 bytes away
// from its neighbour's) and sums from LDS.  EPB = 16 instead of 64
// elements per workgroup quadruples the grid (205 workgroups for the
// bench nets' 3265 elements instead of 52).  The arithmetic is the direct
// kernel's: four quarter sums, each sequential from 0.f over
// ceil(n_blocks/4) partials, combined as (q0+q1)+(q2+q3), then the same
// Adam expression; the old p/m/v values are fetched before the copy so
// their latency overlaps it.  Host side: dynamic LDS = EPB * n_blocks
// floats, grid = ceil(grand / EPB).
#define REDUCE_EPB 16
#define REDUCE_STAGED_MAX_LDS (48 * 1024)  // bytes: n_blocks <= 768 at EPB 16
#define REDUCE_STAGED_MAX_ELEMS 32768      // small nets only (grid = elems / 16)
// The body is a device function so that one launch can serve two nets
// (mlp_grad_reduce_adam_staged_twin_f32 below): `wg` is the workgroup's
// index within its own net, blockIdx.x in the single-net kernel.
DEV_INLINE void reduce_adam_staged_body(const ReduceAdamArgs& a, float* part,
                                        float* red, const int wg) {
  constexpr int EPB = REDUCE_EPB;
  if (reduce_adam_gate_closed(a, red, wg)) return;
  int grand = 0;
  int base[MLP_MAX_LAYERS];
  for (int l = 0; l < a.n_layers; ++l) {
    base[l] = grand;
    grand += a.total[l];
  }
  const float s0 = a.step[0] + 1.f + a.step_delta;
  const float bc1 = 1.f - __powf(a.beta1, s0);
  const float bc2 = 1.f - __powf(a.beta2, s0);
  const int tid = threadIdx.x;
  const int nb = a.n_blocks;
  const int g0 = wg * EPB;
  const int ne = min(EPB, grand - g0);  // elements of this workgroup (>= 1)

  // this thread's Adam slot (threads 0..ne-1): old values fetched early
  const int g = g0 + tid;
  float *p = nullptr, *m = nullptr, *v = nullptr;
  int idx = 0;
  float p_old = 0.f, m_old = 0.f, v_old = 0.f;
  if (tid < ne) {
    int l = 0;
    while (l + 1 < a.n_layers && g >= base[l + 1]) ++l;
    idx = g - base[l];
    if (idx < a.wsize[l]) {
      p = a.pw[l]; m = a.mw[l]; v = a.vw[l];
    } else {
      idx -= a.wsize[l];
      p = a.pb[l]; m = a.mb[l]; v = a.vb[l];
    }
    p_old = p[idx];
    m_old = m[idx];
    v_old = v[idx];
  }

  // coalesced copy of the run ws[g0 * nb, (g0 + ne) * nb): g0 is a
  // multiple of EPB = 16, so the run starts 16-byte aligned
  const int cnt = ne * nb;
  const float* src = a.ws + (long)g0 * nb;
  const int cnt4 = cnt >> 2;
  const float4* src4 = reinterpret_cast<const float4*>(src);
  float4* part4 = reinterpret_cast<float4*>(part);
  for (int i = tid; i < cnt4; i += 256) part4[i] = src4[i];
  for (int i = (cnt4 << 2) + tid; i < cnt; i += 256) part[i] = src[i];
  __syncthreads();

  const int e_local = tid % EPB;
  const int quarter = tid / EPB;
  if (quarter < 4) {
    const int chunk = (nb + 3) / 4;
    const int p0 = quarter * chunk;
    const int p1 = min(p0 + chunk, nb);
    float s = 0.f;
    if (e_local < ne) {
      for (int q = p0; q < p1; ++q) s += part[e_local * nb + q];
    }
    red[tid] = s;
  }
  __syncthreads();
  if (tid < ne) {
    float grad = (red[tid] + red[EPB + tid]) +
                 (red[2 * EPB + tid] + red[3 * EPB + tid]);
    if (a.weight_decay != 0.f) grad += a.weight_decay * p_old;
    const float mi = a.beta1 * m_old + (1.f - a.beta1) * grad;
    const float vi = a.beta2 * v_old + (1.f - a.beta2) * grad * grad;
    m[idx] = mi;
    v[idx] = vi;
    p[idx] = p_old - a.lr * (mi / bc1) / (sqrtf(vi / bc2) + a.eps);
  }
}

__global__ __launch_bounds__(256) void mlp_grad_reduce_adam_staged_f32(ReduceAdamArgs a) {
  extern __shared__ __align__(16) float part[];  // [EPB][n_blocks], as in ws
  __shared__ float red[256];
  reduce_adam_staged_body(a, part, red, blockIdx.x);
}

// Twin form for the PPO update: workgroups [0, pol_wgs) are the policy
// net's (log_std pseudo-layer and gate bookkeeping included), the rest the
// value net's (ungated), each with its index within its own net.  The
// argument written above reduce_adam_gate_closed carries over: only policy
// workgroups read the gate and only the policy's workgroup 0 writes it.
// One concatenated blockIdx.x range instead of a (max, 2) grid: every
// launched workgroup has work (215 + 205 for the bench nets, against 430
// with 10 of them empty).  Measured on MI355X the two forms tie: 33.47
// against 33.42 us per captured twin iteration at batch 4000.
__global__ __launch_bounds__(256) void mlp_grad_reduce_adam_staged_twin_f32(
    ReduceAdamArgs pol, ReduceAdamArgs val, int pol_wgs) {
  extern __shared__ __align__(16) float part[];  // [EPB][max n_blocks]
  __shared__ float red[256];
  const int bx = blockIdx.x;
  if (bx < pol_wgs) reduce_adam_staged_body(pol, part, red, bx);
  else reduce_adam_staged_body(val, part, red, bx - pol_wgs);
}

bool mlp_reduce_adam_is_staged(int n_blocks, long grand) {
  const size_t staged_lds = (size_t)REDUCE_EPB * n_blocks * sizeof(float);
  return staged_lds <= REDUCE_STAGED_MAX_LDS && grand <= REDUCE_STAGED_MAX_ELEMS;
}

// both nets must qualify for the staged reduce (the caller checks)
void launch_mlp_grad_reduce_adam_twin(const ReduceAdamArgs& pol, long grand_pol,
                                      const ReduceAdamArgs& val, long grand_val,
                                      hipStream_t stream) {
  const int nb = pol.n_blocks > val.n_blocks ? pol.n_blocks : val.n_blocks;
  const size_t staged_lds = (size_t)REDUCE_EPB * nb * sizeof(float);
  const int rb_pol = (int)((grand_pol + REDUCE_EPB - 1) / REDUCE_EPB);
  const int rb_val = (int)((grand_val + REDUCE_EPB - 1) / REDUCE_EPB);
  hipLaunchKernelGGL(mlp_grad_reduce_adam_staged_twin_f32,
                     dim3(rb_pol + rb_val), dim3(256), staged_lds, stream, pol,
                     val, rb_pol);
}

void launch_mlp_grad_reduce_adam(const ReduceAdamArgs& a, long grand,
                                 hipStream_t stream) {
  // staged: the partial rows of one workgroup fit a modest LDS slice and
  // the net is small (large nets keep the grid-strided direct kernel)
  const size_t staged_lds = (size_t)REDUCE_EPB * a.n_blocks * sizeof(float);
  if (mlp_reduce_adam_is_staged(a.n_blocks, grand)) {
    const int rb = (int)((grand + REDUCE_EPB - 1) / REDUCE_EPB);
    hipLaunchKernelGGL(mlp_grad_reduce_adam_staged_f32, dim3(rb), dim3(256),
                       staged_lds, stream, a);
    return;
  }
  const int rb = (int)std::min<long>(256, (grand + 63) / 64);
  hipLaunchKernelGGL(mlp_grad_reduce_adam_f32, dim3(rb), dim3(256), 0, stream,
                     a);
}

__global__ __launch_bounds__(256) void mlp_grad_reduce_onepass_f32(ReduceAllArgs a) {
  __shared__ float red[256];
  int grand = 0;
  int base[MLP_MAX_LAYERS];
  for (int l = 0; l < a.n_layers; ++l) {
    base[l] = grand;
    grand += a.total[l];
  }
  const int e_local = threadIdx.x & 63;
  const int quarter = threadIdx.x >> 6;
  const int chunk = (a.n_blocks + 3) / 4;
  const int p0 = quarter * chunk;
  const int p1 = min(p0 + chunk, a.n_blocks);
  for (int g0 = blockIdx.x * 64; g0 < grand; g0 += gridDim.x * 64) {
    const int g = g0 + e_local;
    float s = 0.f;
    if (g < grand) {
      for (int p = p0; p < p1; ++p) s += a.ws[(long)g * a.n_blocks + p];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (quarter == 0 && g < grand) {
      const float tot = (red[e_local] + red[64 + e_local]) +
                        (red[128 + e_local] + red[192 + e_local]);
      int l = 0;
      while (l + 1 < a.n_layers && g >= base[l + 1]) ++l;
      const int idx = g - base[l];
      if (idx < a.wsize[l]) a.dw[l][idx] = tot;
      else a.db[l][idx - a.wsize[l]] = tot;
    }
    __syncthreads();
  }
}
