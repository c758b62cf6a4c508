// The initial state of a rollout (core.py:121-135) in one launch each way: the masked mean of the two frame-0 embeddings,
// init_proj (Linear-act-Linear), the prior head (Linear-act-Linear) and the categorical head.  Before: two elementwise launches,
// four 64-row GEMMs with their clears (15-20 us each: a chain of dependent k-steps on a handful of workgroups), the head's
// launch; the mirror of all that in the backward pass.
//
// One workgroup of 1024 threads per batch row; no workgroup waits for another.  The activations of a layer sit in LDS, the
// weights (550 KB at the base dims) stream from L2.
//
// Reduction orders (all fp32 fma chains; the bias is added last):
//   forward   y[n] = b[n] + sum_k W[n][k] x[k]: one wave per output row.  Lane l folds k = 4l .. 4l+3, 4l+256 .. in ascending
//             order into ONE accumulator (16-byte loads; rows that are not 16-byte aligned or K % 4 != 0: k = l, l+64, ..), the
//             64 lane sums meet in the DPP tree of wave_sum (scan_common.h).
//   backward  g[m] = sum_r W[r][m] y[r]: lanes run along m (coalesced rows).  The r range is cut into P = floor(1024 / M)
//             contiguous parts (at most R), each folded in ascending r by one thread; the P partial sums are added in ascending
//             part order.
// The categorical arithmetic is categorical.h's, shared with categorical_sample_*_kernel.
// Weight and bias gradients are NOT formed here: the backward kernel leaves their operands (d_logits, d_zp, g_deter, d_z1 and
// the forward's e, z1, deter0, zp) in HBM for the grouped weight-gradient GEMMs (linear.weight_grad).
#include "categorical.h"
#include "scan_common.h"

namespace mtrssm {

constexpr int kInitThreads = 1024;
constexpr int kInitMax = 1024;   // largest layer width (and K * C) whose activations fit the static LDS vectors
constexpr int kInitRows = 4;     // output rows a wave has in flight in the forward
// The four matrices together (2 MB).  A guess between two measured points, not a measured crossover: 550 KB (base dims, 64
// rows) is 87 us per step faster fused; 6 MB (Large dims, 32 rows) was not faster (16.76-16.81 against 16.74-16.75 ms per step,
// inside the noise) and is left to the GEMMs.  Nobody has timed a size in between.
constexpr int64_t kInitWeightFloats = 512 * 1024;

__device__ __forceinline__ float act_grad_in(float z, int act) {
  switch (act) {
    case MTRSSM_ACT_RELU: return z > 0.f ? 1.f : 0.f;
    case MTRSSM_ACT_ELU: return z > 0.f ? 1.f : expf(z);
    case MTRSSM_ACT_TANH: { const float t = tanhf(z); return 1.f - t * t; }
    default: return 1.f;
  }
}

// emit(n, bias[n] + sum_k W[n][k] x[k]) for n < N on lane 0 of the row's wave; x in LDS (16-byte aligned)
template <typename Emit>
__device__ __forceinline__ void rows_dot(const float* __restrict__ W, int ld, int N, int K, const float* x, const float* __restrict__ bias,
                                         Emit&& emit) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, waves = blockDim.x / kWave;
  const bool vec = (((uintptr_t)W & 15) == 0) && (ld & 3) == 0 && (K & 3) == 0;
  for (int n0 = wave * kInitRows; n0 < N; n0 += waves * kInitRows) {   // wave-uniform
    float acc[kInitRows];
    const float* row[kInitRows];
#pragma unroll
    for (int i = 0; i < kInitRows; ++i) {
      acc[i] = 0.f;
      row[i] = W + (size_t)(n0 + i < N ? n0 + i : N - 1) * ld;   // (clamped: a row past the end is summed and dropped)
    }
    if (vec) {
      for (int k = lane * 4; k < K; k += kWave * 4) {
        const float4 xv = *reinterpret_cast<const float4*>(x + k);
#pragma unroll
        for (int i = 0; i < kInitRows; ++i) {
          const float4 w = *reinterpret_cast<const float4*>(row[i] + k);
          acc[i] = fmaf(w.x, xv.x, acc[i]);
          acc[i] = fmaf(w.y, xv.y, acc[i]);
          acc[i] = fmaf(w.z, xv.z, acc[i]);
          acc[i] = fmaf(w.w, xv.w, acc[i]);
        }
      }
    } else {
      for (int k = lane; k < K; k += kWave) {
        const float xv = x[k];
#pragma unroll
        for (int i = 0; i < kInitRows; ++i) acc[i] = fmaf(row[i][k], xv, acc[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < kInitRows; ++i) {
      const float s = wave_sum(acc[i]);
      if (lane == 0 && n0 + i < N) emit(n0 + i, s + bias[n0 + i]);
    }
  }
}

// emit(m, sum_r W[r][m] y[r]) for m < M on thread m; y and part in LDS (part: kInitMax floats).  Ends with the caller's barrier.
template <typename Emit>
__device__ __forceinline__ void cols_dot(const float* __restrict__ W, int ld, int R, int M, const float* y, float* part, Emit&& emit) {
  const int tid = threadIdx.x;
  int P = (int)blockDim.x / M;
  if (P > R) P = R;
  const int per = (R + P - 1) / P;
  const int q = tid / M, m = tid - q * M;
  if (q < P) {
    const int r1 = (q + 1) * per < R ? (q + 1) * per : R;
    float acc = 0.f;
#pragma unroll 8
    for (int r = q * per; r < r1; ++r) acc = fmaf(W[(size_t)r * ld + m], y[r], acc);
    part[q * M + m] = acc;
  }
  __syncthreads();
  if (tid < M) {
    float s = part[tid];
    for (int i = 1; i < P; ++i) s += part[i * M + tid];
    emit(tid, s);
  }
}

// 0: both embeddings (mean), 1: audio only, 2: vision only
__device__ __forceinline__ int embed_mode(const MtrssmInitialState& p, int b) {
  if (!p.ea) return 2;
  if (!p.ev) return 1;
  if (!p.mask0) return 0;
  const bool a = p.mask0[2 * b] != 0, v = p.mask0[2 * b + 1] != 0;
  return a && v ? 0 : (a ? 1 : 2);
}

__global__ __launch_bounds__(kInitThreads) void initial_state_fwd_kernel(const MtrssmInitialState p) {
  __shared__ __attribute__((aligned(16))) float s_e[kInitMax], s_a[kInitMax], s_d[kInitMax], s_p[kInitMax], s_l[kInitMax];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int S = p.K * p.C;
  const int mode = embed_mode(p, b);
  const float* ea = p.ea ? p.ea + (size_t)b * p.ea_stride : nullptr;
  const float* ev = p.ev ? p.ev + (size_t)b * p.ev_stride : nullptr;
  for (int k = tid; k < p.E; k += blockDim.x) {
    const float v = mode == 0 ? (ea[k] + ev[k]) / 2.f : (mode == 1 ? ea[k] : ev[k]);
    s_e[k] = v;
    p.e[(size_t)b * p.E + k] = v;
  }
  __syncthreads();
  rows_dot(p.wi1, p.ld_wi1, p.cells, p.E, s_e, p.bi1, [&](int n, float v) {
    p.z1[(size_t)b * p.cells + n] = v;
    s_a[n] = act_fwd(v, p.act_i);
  });
  __syncthreads();
  rows_dot(p.wi2, p.ld_wi2, p.D, p.cells, s_a, p.bi2, [&](int n, float v) {
    p.deter0[(size_t)b * p.D + n] = v;
    s_d[n] = v;
  });
  __syncthreads();
  rows_dot(p.wp1, p.ld_wp1, p.H, p.D, s_d, p.bp1, [&](int n, float v) {
    p.zp[(size_t)b * p.H + n] = v;
    s_p[n] = act_fwd(v, p.act_p);
  });
  __syncthreads();
  rows_dot(p.wp2, p.ld_wp2, S, p.H, s_p, p.bp2, [&](int n, float v) { s_l[n] = v; });
  __syncthreads();
  if (tid < p.K) {
    const size_t at = ((size_t)b * p.K + tid) * p.C;
    categorical_sample_one(s_l + tid * p.C, p.u[(size_t)b * p.K + tid], p.C, p.logp + at, p.probs + at, p.stoch + at);
  }
}

__global__ __launch_bounds__(kInitThreads) void initial_state_bwd_kernel(const MtrssmInitialState p) {
  __shared__ __attribute__((aligned(16))) float s_gp[kInitMax], s_gl[kInitMax], s_dl[kInitMax], s_x[kInitMax], s_y[kInitMax], s_part[kInitMax];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int S = p.K * p.C;
  const bool has_gp = p.g_stoch0 || p.g_probs, has_gl = p.g_logp != nullptr;
  for (int i = tid; i < S; i += blockDim.x) {
    const size_t at = (size_t)b * S + i;
    s_gp[i] = (p.g_stoch0 ? p.g_stoch0[at] : 0.f) + (p.g_probs ? p.g_probs[at] : 0.f);
    s_gl[i] = has_gl ? p.g_logp[at] : 0.f;
  }
  __syncthreads();
  if (tid < p.K)
    categorical_grad_one(p.probs + ((size_t)b * p.K + tid) * p.C, has_gp ? s_gp + tid * p.C : nullptr, has_gl ? s_gl + tid * p.C : nullptr, p.C,
                         s_dl + tid * p.C);
  __syncthreads();
  for (int i = tid; i < S; i += blockDim.x) p.d_logits[(size_t)b * S + i] = s_dl[i];
  cols_dot(p.wp2, p.ld_wp2, S, p.H, s_dl, s_part, [&](int m, float s) {
    const float v = s * act_grad_in(p.zp[(size_t)b * p.H + m], p.act_p);
    p.d_zp[(size_t)b * p.H + m] = v;
    s_x[m] = v;
  });
  __syncthreads();
  cols_dot(p.wp1, p.ld_wp1, p.H, p.D, s_x, s_part, [&](int m, float s) {
    const float v = s + (p.g_deter0 ? p.g_deter0[(size_t)b * p.D + m] : 0.f);
    p.g_deter[(size_t)b * p.D + m] = v;
    s_y[m] = v;
  });
  __syncthreads();
  cols_dot(p.wi2, p.ld_wi2, p.D, p.cells, s_y, s_part, [&](int m, float s) {
    const float v = s * act_grad_in(p.z1[(size_t)b * p.cells + m], p.act_i);
    p.d_z1[(size_t)b * p.cells + m] = v;
    s_x[m] = v;
  });
  __syncthreads();
  const int mode = embed_mode(p, b);
  cols_dot(p.wi1, p.ld_wi1, p.cells, p.E, s_x, s_part, [&](int m, float s) {
    if (p.g_ea) p.g_ea[(size_t)b * p.E + m] = mode == 0 ? s / 2.f : (mode == 1 ? s : 0.f);
    if (p.g_ev) p.g_ev[(size_t)b * p.E + m] = mode == 0 ? s / 2.f : (mode == 2 ? s : 0.f);
  });
}

static const char* refusal(const MtrssmInitialState* p) {
  if (!p) return "null argument";
  if (p->depth_i != 1 || p->depth_p != 1) return "Linear-act-Linear stacks only (depth 1)";
  for (int a : {p->act_i, p->act_p})
    if (a < MTRSSM_ACT_IDENTITY || a > MTRSSM_ACT_TANH) return "unknown activation id";
  if (p->B <= 0 || p->E <= 0 || p->cells <= 0 || p->D <= 0 || p->H <= 0 || p->K <= 0 || p->C <= 0) return "non-positive extent";
  if (p->E > kInitMax || p->cells > kInitMax || p->D > kInitMax || p->H > kInitMax || p->K > kInitMax || p->C > kInitMax ||
      (int64_t)p->K * p->C > kInitMax)
    return "a layer is wider than 1024 (the activations of a layer sit in LDS)";
  // every workgroup streams ALL weights once: that pays while they are a small L2-resident set (550 KB at the base dims).  At
  // the Large dims (6 MB, 32 rows: 190 MB through the L2) the layer-by-layer GEMMs, which read each weight once, are faster.
  if ((int64_t)p->E * p->cells + (int64_t)p->cells * p->D + (int64_t)p->D * p->H + (int64_t)p->H * p->K * p->C > kInitWeightFloats)
    return "more than 2 MB of weights (every batch row's workgroup streams them all)";
  if (p->ld_wi1 < p->E || p->ld_wi2 < p->cells || p->ld_wp1 < p->D || p->ld_wp2 < p->H) return "a leading dimension is smaller than its row";
  return nullptr;
}

static bool common_pointers(const MtrssmInitialState* p) {
  return (p->ea || p->ev) && (!p->ea || p->ea_stride >= p->E) && (!p->ev || p->ev_stride >= p->E) && p->wi1 && p->bi1 && p->wi2 && p->bi2 &&
         p->wp1 && p->bp1 && p->wp2 && p->bp2;
}

static int finish(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("%s launch failed: %s", what, hipGetErrorString(e)); return MTRSSM_ELAUNCH; }
  return MTRSSM_OK;
}

int initial_state_supported(const MtrssmInitialState* p) { return refusal(p) == nullptr ? 1 : 0; }

int initial_state_fwd_launch(const MtrssmInitialState* p, hipStream_t stream) {
  if (const char* why = refusal(p)) { set_error("initial_state_fwd: %s", why); return MTRSSM_EINVAL; }
  if (!common_pointers(p) || !p->u || !p->e || !p->z1 || !p->deter0 || !p->zp || !p->logp || !p->probs || !p->stoch) {
    set_error("initial_state_fwd: null pointer (or an embedding row stride below E)");
    return MTRSSM_EINVAL;
  }
  set_last_kernel("mtrssm::initial_state_fwd_kernel");
  hipLaunchKernelGGL(initial_state_fwd_kernel, dim3((unsigned)p->B), dim3(kInitThreads), 0, stream, *p);
  return finish("initial_state_fwd");
}

int initial_state_bwd_launch(const MtrssmInitialState* p, hipStream_t stream) {
  if (const char* why = refusal(p)) { set_error("initial_state_bwd: %s", why); return MTRSSM_EINVAL; }
  if (!common_pointers(p) || !p->z1 || !p->zp || !p->probs || !p->d_logits || !p->d_zp || !p->g_deter || !p->d_z1) {
    set_error("initial_state_bwd: null pointer (or an embedding row stride below E)");
    return MTRSSM_EINVAL;
  }
  set_last_kernel("mtrssm::initial_state_bwd_kernel");
  hipLaunchKernelGGL(initial_state_bwd_kernel, dim3((unsigned)p->B), dim3(kInitThreads), 0, stream, *p);
  return finish("initial_state_bwd");
}

}  // namespace mtrssm
