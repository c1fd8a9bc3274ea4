// LLAL loss-prediction module (LossNet, pcdet/models/roi_heads/loss_net.py) as two launches forward and two backward
//
// replaces, per step: for each of the num_layer shared-FC latents a Conv1d(C -> 1, k=1) as a batched GEMM, BatchNorm1d(1) (mean, var,
// normalise, running-statistics update), ReLU, view, then cat + Linear — and the same chain backwards (~12 launches each way per
// layer). Sizes are small (R = frames * 128 rows of 256 channels), so every launch is latency-bound: what matters is their number.
//
//   forward  1: lossnet_dot_kernel      z[k][r] = <x_k[r, :], w_k>, one wave per (layer, row)
//            2: lossnet_head_kernel     one workgroup: BN statistics (train) or running statistics (eval), normalise, ReLU, per-frame
//                                       linear; running-statistics update
//   backward 1: lossnet_bwd_head_kernel one workgroup: d linear, d bias, ReLU mask, BN backward -> dz[k][r], d gamma, d beta
//            2: lossnet_bwd_x_kernel    d x_k = dz_k (x) w_k (elementwise blocks) and d w_k = sum_r dz_k[r] x_k[r, :] (column blocks,
//                                       16 row groups summed in a fixed order)
// All accumulation in f64, every sum in a fixed order, no atomics: bit-reproducible run to run.
#include "crb_common.h"
#include "../../include/crb_hip.h"

namespace {

constexpr int TPB = 1024;
constexpr int WAVES = TPB / 64;
constexpr int DX_ROWS = 8;         // rows of d x per elementwise block
constexpr int DW_COLS = 64;        // columns of d w per column block (one per lane)

// workspace (f64): z, xhat, act, dz (num_layer * R each) + mean / invstd per layer
struct LossNetWs {
  double* z;
  double* xhat;
  double* act;
  double* dz;
  double* stats;                   // [2k] mean, [2k + 1] inverse standard deviation
};

__host__ __device__ inline int64_t ws_doubles(int L, int64_t R) { return 4 * (int64_t)L * R + 2 * CRB_LOSSNET_MAX_LAYERS; }

__host__ __device__ inline LossNetWs carve(void* ws, int L, int64_t R) {
  double* p = (double*)ws;
  const int64_t n = (int64_t)L * R;
  return LossNetWs{p, p + n, p + 2 * n, p + 3 * n, p + 4 * n};
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// block-wide sum, the same fixed order on every call; every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) t += sh[w];
  return t;
}

__global__ void __launch_bounds__(TPB) lossnet_dot_kernel(CrbLossNetArgs a, int64_t R, LossNetWs ws) {
  const int k = blockIdx.y;
  const int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (r >= R) return;
  const int C = a.channels[k];
  const float* xr = a.x[k] + r * C;
  const float* w = a.w[k];
  double acc = 0.0;
  for (int c = crb_lane(); c < C; c += 64) acc = fma((double)xr[c], (double)w[c], acc);
  acc = wave_sum(acc);
  if (crb_lane() == 0) ws.z[k * R + r] = acc;
}

__global__ void __launch_bounds__(TPB) lossnet_head_kernel(CrbLossNetArgs a, int64_t R, const float* lin_w, const float* lin_b,
                                                           float* out, LossNetWs ws) {
  __shared__ double sh[WAVES];
  const int tid = threadIdx.x;
  const int L = a.num_layer, P = a.rows_per_frame;
  for (int k = 0; k < L; ++k) {
    const double* z = ws.z + k * R;
    double mean, invstd;
    if (a.training) {
      double s = 0.0;
      for (int64_t r = tid; r < R; r += TPB) s += z[r];
      mean = block_sum(s, sh) / (double)R;
      double q = 0.0;
      for (int64_t r = tid; r < R; r += TPB) {
        const double d = z[r] - mean;
        q = fma(d, d, q);
      }
      const double Q = block_sum(q, sh);
      invstd = 1.0 / sqrt(Q / (double)R + (double)a.eps);
      if (tid == 0) {
        // torch: running = (1 - momentum) * running + momentum * batch value, the variance unbiased
        const double m = (double)a.momentum;
        a.running_mean[k][0] = (float)((1.0 - m) * (double)a.running_mean[k][0] + m * mean);
        a.running_var[k][0] = (float)((1.0 - m) * (double)a.running_var[k][0] + m * (Q / (double)(R - 1)));
        a.num_batches_tracked[k][0] += 1;
      }
    } else {
      mean = (double)a.running_mean[k][0];
      invstd = 1.0 / sqrt((double)a.running_var[k][0] + (double)a.eps);
    }
    if (tid == 0) {
      ws.stats[2 * k] = mean;
      ws.stats[2 * k + 1] = invstd;
    }
    const double g = (double)a.gamma[k][0], b = (double)a.beta[k][0];
    for (int64_t r = tid; r < R; r += TPB) {
      const double xh = (z[r] - mean) * invstd;
      ws.xhat[k * R + r] = xh;
      ws.act[k * R + r] = fmax(fma(xh, g, b), 0.0);
    }
  }
  __syncthreads();
  // per-frame linear: wave per frame, columns k * P + j <- act[k][frame * P + j]
  const int lane = crb_lane();
  for (int f = tid >> 6; f < a.frames; f += WAVES) {
    double acc = 0.0;
    for (int k = 0; k < L; ++k) {
      const double* act = ws.act + k * R + (int64_t)f * P;
      for (int j = lane; j < P; j += 64) acc = fma(act[j], (double)lin_w[k * P + j], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) out[f] = (float)(acc + (double)lin_b[0]);
  }
}

__global__ void __launch_bounds__(TPB) lossnet_bwd_head_kernel(CrbLossNetArgs a, int64_t R, const float* lin_w, const float* d_out,
                                                               LossNetWs ws, float* d_gamma_beta, float* d_lin_w, float* d_lin_b) {
  __shared__ double sh[WAVES];
  const int tid = threadIdx.x;
  const int L = a.num_layer, P = a.rows_per_frame, F = a.frames;
  for (int col = tid; col < L * P; col += TPB) {
    const int k = col / P, j = col - k * P;
    double acc = 0.0;
    for (int f = 0; f < F; ++f) acc = fma((double)d_out[f], ws.act[k * R + (int64_t)f * P + j], acc);
    d_lin_w[col] = (float)acc;
  }
  if (tid == 0) {
    double acc = 0.0;
    for (int f = 0; f < F; ++f) acc += (double)d_out[f];
    d_lin_b[0] = (float)acc;
  }
  for (int k = 0; k < L; ++k) {
    const double* xhat = ws.xhat + k * R;
    const double* act = ws.act + k * R;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t r = tid; r < R; r += TPB) {
      const int64_t f = r / P;
      const double dy = act[r] > 0.0 ? (double)d_out[f] * (double)lin_w[k * P + (r - f * P)] : 0.0;
      s1 += dy;
      s2 = fma(dy, xhat[r], s2);
    }
    const double S1 = block_sum(s1, sh);
    const double S2 = block_sum(s2, sh);
    if (tid == 0) {
      d_gamma_beta[2 * k] = (float)S2;
      d_gamma_beta[2 * k + 1] = (float)S1;
    }
    const double scale = (double)a.gamma[k][0] * ws.stats[2 * k + 1];
    const double m1 = S1 / (double)R, m2 = S2 / (double)R;
    for (int64_t r = tid; r < R; r += TPB) {
      const int64_t f = r / P;
      const double dy = act[r] > 0.0 ? (double)d_out[f] * (double)lin_w[k * P + (r - f * P)] : 0.0;
      ws.dz[k * R + r] = a.training ? scale * (dy - m1 - xhat[r] * m2) : scale * dy;
    }
  }
}

// blockIdx.x < nx: rows [blockIdx.x * DX_ROWS, +DX_ROWS) of d x_k; blockIdx.x >= nx: columns [(blockIdx.x - nx) * DW_COLS, +DW_COLS)
// of d w_k, 16 contiguous row ranges (one per wave) summed in order
__global__ void __launch_bounds__(TPB) lossnet_bwd_x_kernel(CrbLossNetArgs a, int64_t R, int nx, LossNetWs ws, CrbLossNetGrads gr) {
  __shared__ double part[WAVES][DW_COLS];
  const int k = blockIdx.y;
  const int C = a.channels[k];
  const double* dz = ws.dz + k * R;
  const float* w = a.w[k];
  if ((int)blockIdx.x < nx) {
    float* dx = gr.d_x[k];
    if (dx == nullptr) return;
    const int64_t r0 = (int64_t)blockIdx.x * DX_ROWS;
    const int64_t rows = R - r0 < DX_ROWS ? R - r0 : DX_ROWS;
    for (int64_t i = threadIdx.x; i < rows * C; i += TPB) {
      const int64_t r = r0 + i / C;
      const int c = (int)(i % C);
      dx[r * C + c] = (float)(dz[r] * (double)w[c]);
    }
    return;
  }
  const int c0 = ((int)blockIdx.x - nx) * DW_COLS;
  if (c0 >= C) return;                                   // block-uniform
  const int lane = crb_lane(), wv = threadIdx.x >> 6;
  const int c = c0 + lane;
  const int64_t chunk = (R + WAVES - 1) / WAVES;
  const int64_t rb = (int64_t)wv * chunk;
  const int64_t re = rb + chunk < R ? rb + chunk : R;
  const float* x = a.x[k];
  double acc = 0.0;
  if (c < C)
    for (int64_t r = rb; r < re; ++r) acc = fma(dz[r], (double)x[r * C + c], acc);
  part[wv][lane] = acc;
  __syncthreads();
  if (wv == 0 && c < C) {
    double t = 0.0;
#pragma unroll
    for (int v = 0; v < WAVES; ++v) t += part[v][lane];
    gr.d_w[k][c] = (float)t;
  }
}

int check_args(const CrbLossNetArgs* a, int64_t* R) {
  if (!a || a->num_layer < 1 || a->num_layer > CRB_LOSSNET_MAX_LAYERS || a->rows_per_frame <= 0 || a->frames <= 0) return CRB_ERR_ARG;
  const int64_t rows = (int64_t)a->frames * a->rows_per_frame;
  if (a->training && rows < 2) return CRB_ERR_ARG;      // torch: "Expected more than 1 value per channel when training"
  for (int k = 0; k < a->num_layer; ++k) {
    if (a->channels[k] <= 0 || !a->x[k] || !a->w[k] || !a->gamma[k] || !a->beta[k] || !a->running_mean[k] || !a->running_var[k])
      return CRB_ERR_ARG;
    if (a->training && !a->num_batches_tracked[k]) return CRB_ERR_ARG;
    if (rows * a->channels[k] >= (1LL << 40)) return CRB_ERR_ARG;
  }
  if (rows / WAVES + 1 >= (1LL << 31)) return CRB_ERR_ARG;
  *R = rows;
  return CRB_OK;
}

}  // namespace

extern "C" int64_t crb_lossnet_workspace_bytes(int num_layer, int64_t rows) {
  if (num_layer < 1 || num_layer > CRB_LOSSNET_MAX_LAYERS || rows < 0) return 0;
  return ws_doubles(num_layer, rows) * (int64_t)sizeof(double);
}

extern "C" int crb_lossnet_forward(const CrbLossNetArgs* args, const float* lin_w, const float* lin_b, float* out, void* ws,
                                   int64_t ws_bytes, void* stream) {
  int64_t R = 0;
  const int rc = check_args(args, &R);
  if (rc != CRB_OK) return rc;
  if (!lin_w || !lin_b || !out) return CRB_ERR_ARG;
  if (!ws || ws_bytes < crb_lossnet_workspace_bytes(args->num_layer, R)) return CRB_ERR_WORKSPACE;
  const LossNetWs w = carve(ws, args->num_layer, R);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lossnet_dot_kernel, dim3(crb_cdiv(R, WAVES), args->num_layer), dim3(TPB), 0, s, *args, R, w);
  CRB_CHECK_LAUNCH();
  hipLaunchKernelGGL(lossnet_head_kernel, dim3(1), dim3(TPB), 0, s, *args, R, lin_w, lin_b, out, w);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_lossnet_backward(const CrbLossNetArgs* args, const float* lin_w, const float* d_out, void* ws, int64_t ws_bytes,
                                    const CrbLossNetGrads* grads, void* stream) {
  int64_t R = 0;
  const int rc = check_args(args, &R);
  if (rc != CRB_OK) return rc;
  if (!lin_w || !d_out || !grads || !grads->d_gamma_beta || !grads->d_lin_w || !grads->d_lin_b) return CRB_ERR_ARG;
  int cmax = 0;
  for (int k = 0; k < args->num_layer; ++k) {
    if (!grads->d_w[k]) return CRB_ERR_ARG;
    cmax = args->channels[k] > cmax ? args->channels[k] : cmax;
  }
  if (!ws || ws_bytes < crb_lossnet_workspace_bytes(args->num_layer, R)) return CRB_ERR_WORKSPACE;
  const LossNetWs w = carve(ws, args->num_layer, R);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lossnet_bwd_head_kernel, dim3(1), dim3(TPB), 0, s, *args, R, lin_w, d_out, w, grads->d_gamma_beta, grads->d_lin_w,
                     grads->d_lin_b);
  CRB_CHECK_LAUNCH();
  const int nx = crb_cdiv(R, DX_ROWS);
  hipLaunchKernelGGL(lossnet_bwd_x_kernel, dim3(nx + crb_cdiv(cmax, DW_COLS), args->num_layer), dim3(TPB), 0, s, *args, R, nx, w, *grads);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
