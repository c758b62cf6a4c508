// The fit loop's per-step fold for gfx950: per-segment sum(g^2), sum(p^2) and non-finite counts over the flat
// gradient / parameter buffers, then the epoch accumulator's update, in two launches of one call.  Every product and sum is double,
// partial sums meet in an order fixed by numel and the segment table, there is no atomic and no exchange between the workgroups of a
// launch: two calls on the same buffers are bitwise equal.  Nothing the host passes by value changes from step to step (the step's
// weight is a device scalar, its index a word of the flag block), so the call may sit behind a replayed graph as it is.
#include "scan_common.h"

namespace mtrssm {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kChunk = 4096;  // floats of one segment a workgroup sums: four float4 of each buffer per lane
constexpr int kFinalThreads = 1024;
constexpr int kFinalWaves = kFinalThreads / kWave;

__device__ __forceinline__ double shfl_xor_d(double v, int mask) { return __shfl_xor(v, mask, kWave); }
__device__ __forceinline__ double wave_sum_d(double v) {  // (every lane active; every lane ends with the same bits)
  for (int m = 1; m < kWave; m <<= 1) v += shfl_xor_d(v, m);
  return v;
}
__device__ __forceinline__ int not_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ int64_t chunks_of(int64_t floats) { return (floats + kChunk - 1) / kChunk; }

// Workgroup c of the grid owns chunk c of the list "segment 0's chunks, segment 1's chunks, ...": its slot in `partial` is c.
// The grid is the host's upper bound numel / kChunk + G: a workgroup past the list's end leaves.
__global__ __launch_bounds__(kThreads) void fit_partial_kernel(const float* __restrict__ grad, const float* __restrict__ param,
                                                               const int64_t* __restrict__ offsets, int G, int64_t numel,
                                                               double* __restrict__ partial) {
  __shared__ double s_sum[kWaves][3];
  int64_t c = blockIdx.x, lo = 0, hi = 0;
  int seg = 0;
  for (; seg < G; ++seg) {  // (uniform: every lane walks the same G <= 32 entries)
    lo = offsets[seg];
    hi = offsets[seg + 1];
    const int64_t n = chunks_of(hi - lo);
    if (c < n) break;
    c -= n;
  }
  if (seg == G) return;
  hi = hi < numel ? hi : numel;  // (a table the host checked never needs this; a foreign one cannot read past the buffers)
  const int64_t base = lo + c * kChunk;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  double g2 = 0.0, p2 = 0.0;
  int bad = 0;
#pragma unroll
  for (int j = 0; j < kChunk / (4 * kThreads); ++j) {
    const int64_t at = base + 4 * ((int64_t)j * kThreads + threadIdx.x);
    if (at >= 0 && at + 4 <= hi) {
      const float4 g = *reinterpret_cast<const float4*>(grad + at);
      const float4 p = *reinterpret_cast<const float4*>(param + at);
      g2 += (double)g.x * (double)g.x;
      g2 += (double)g.y * (double)g.y;
      g2 += (double)g.z * (double)g.z;
      g2 += (double)g.w * (double)g.w;
      p2 += (double)p.x * (double)p.x;
      p2 += (double)p.y * (double)p.y;
      p2 += (double)p.z * (double)p.z;
      p2 += (double)p.w * (double)p.w;
      bad += not_finite(g.x) + not_finite(g.y) + not_finite(g.z) + not_finite(g.w);
    }
  }
  g2 = wave_sum_d(g2);
  p2 = wave_sum_d(p2);
  const double nb = wave_sum_d((double)bad);
  if (lane == 0) {
    s_sum[wave][0] = g2;
    s_sum[wave][1] = p2;
    s_sum[wave][2] = nb;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double v = 0.0;
    for (int w = 0; w < kWaves; ++w) v += s_sum[w][threadIdx.x];
    partial[3 * (int64_t)blockIdx.x + threadIdx.x] = v;
  }
}

// One workgroup: the chunks' partial sums per segment (lane t takes slots t, t + 1024, ..., then the waves' sums in ascending
// order), the groups' sums (ascending segments), and the accumulator's update by one lane.
__global__ __launch_bounds__(kFinalThreads) void fit_finish_kernel(const double* __restrict__ partial, const int64_t* __restrict__ offsets,
                                                                   const int32_t* __restrict__ group, int G, int64_t slots,
                                                                   const float* __restrict__ scalars,
                                                                   int K, float scalar_scale, float grad_scale, float clip_norm,
                                                                   const float* __restrict__ weight, double* __restrict__ sums,
                                                                   double* __restrict__ acc, int32_t* __restrict__ flags) {
  __shared__ double s_wave[kFinalWaves][3];
  __shared__ double s_seg[3][MTRSSM_FIT_MAX_SEGMENTS];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int64_t slot0 = 0;
  for (int seg = 0; seg < G; ++seg) {
    const int64_t n = chunks_of(offsets[seg + 1] - offsets[seg]);
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < n && slot0 + i < slots; i += kFinalThreads) {  // (slots: what the workspace holds)
#pragma unroll
      for (int q = 0; q < 3; ++q) v[q] += partial[3 * (slot0 + i) + q];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] = wave_sum_d(v[q]);
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 3; ++q) s_wave[wave][q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      double t = 0.0;
      for (int w = 0; w < kFinalWaves; ++w) t += s_wave[w][threadIdx.x];
      s_seg[threadIdx.x][seg] = t;
      sums[threadIdx.x * MTRSSM_FIT_MAX_SEGMENTS + seg] = t;
    }
    __syncthreads();
    slot0 += n;
  }
  if (threadIdx.x != 0) return;
  int32_t bad_segments = 0, bad_scalars = 0;
  double g2_all = 0.0, p2_all = 0.0;
  for (int seg = 0; seg < G; ++seg) {
    if (s_seg[2][seg] > 0.0) bad_segments |= (int32_t)(1u << seg);
    g2_all += s_seg[0][seg];
    p2_all += s_seg[1][seg];
  }
  double s[MTRSSM_FIT_MAX_SCALARS];
  for (int k = 0; k < K; ++k) {
    const float x = scalars[k];
    if (not_finite(x)) bad_scalars |= 1 << k;
    s[k] = (double)x * (double)scalar_scale;
  }
  const int32_t step = flags[MTRSSM_FIT_FLAG_STEP];
  flags[MTRSSM_FIT_FLAG_STEP] = step + 1;
  if (bad_segments || bad_scalars) {
    if (flags[MTRSSM_FIT_FLAG_BAD_STEPS] == 0) flags[MTRSSM_FIT_FLAG_FIRST_BAD] = step;
    flags[MTRSSM_FIT_FLAG_BAD_STEPS] += 1;
    flags[MTRSSM_FIT_FLAG_BAD_SEGMENTS] |= bad_segments;
    flags[MTRSSM_FIT_FLAG_BAD_SCALARS] |= bad_scalars;
    return;
  }
  const double w = (double)weight[0], scale = (double)grad_scale;
  acc[MTRSSM_FIT_ACC_WEIGHT] += w;
  acc[MTRSSM_FIT_ACC_STEPS] += 1.0;
  const double norm = sqrt(g2_all) * scale;
  if (clip_norm > 0.f && norm > (double)clip_norm) acc[MTRSSM_FIT_ACC_CLIPPED] += 1.0;
  acc[MTRSSM_FIT_ACC_GRAD_SUM] += norm;
  acc[MTRSSM_FIT_ACC_GRAD_MAX] = fmax(acc[MTRSSM_FIT_ACC_GRAD_MAX], norm);
  acc[MTRSSM_FIT_ACC_PARAM] = sqrt(p2_all);
  for (int k = 0; k < K; ++k) acc[MTRSSM_FIT_ACC_SCALARS + k] += w * s[k];
  for (int seg = 0; seg < G; ++seg) {
    if (group && group[seg] != seg) continue;  // (a later run of a name: summed into the name's first segment)
    double g2 = 0.0, p2 = 0.0;
    for (int t = seg; t < G; ++t) {
      if (t == seg || (group && group[t] == seg)) {
        g2 += s_seg[0][t];
        p2 += s_seg[1][t];
      }
    }
    double* a = acc + MTRSSM_FIT_ACC_SEGMENTS + 3 * seg;
    const double gn = sqrt(g2) * scale;
    a[0] += gn;
    a[1] = fmax(a[1], gn);
    a[2] = sqrt(p2);
  }
}

bool sizes_ok(const char* what, int64_t numel, int G) {
  if (numel <= 0 || (numel & 3) || G < 1 || G > MTRSSM_FIT_MAX_SEGMENTS) {
    set_error("%s: need numel > 0, a multiple of 4, and 1 <= G <= %d segments (got %lld, %d)", what, (long long)numel, MTRSSM_FIT_MAX_SEGMENTS, G);
    return false;
  }
  return true;
}

}  // namespace
}  // namespace mtrssm

using namespace mtrssm;
#define MTRSSM_API extern "C" __attribute__((visibility("default")))

MTRSSM_API int64_t mtrssm_fit_fold_workspace_bytes(int64_t numel, int32_t G, int64_t* chunk_floats) {
  if (!sizes_ok("fit_fold_workspace_bytes", numel, G)) return -1;
  if (chunk_floats) *chunk_floats = kChunk;
  return 8 * (3 * (int64_t)MTRSSM_FIT_MAX_SEGMENTS + 3 * ((numel + kChunk - 1) / kChunk + G));
}

MTRSSM_API int mtrssm_fit_fold(const float* grad, const float* param, int64_t numel, const int64_t* offsets, const int32_t* group, int32_t G,
                               const float* scalars, int32_t K, float scalar_scale, float grad_scale, float clip_norm, const float* weight,
                               double* acc, int32_t* flags, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!grad || !param || !offsets || !weight || !acc || !flags || !workspace || (K > 0 && !scalars)) {
    set_error("fit_fold: null pointer");
    return MTRSSM_EINVAL;
  }
  if (!sizes_ok("fit_fold", numel, G)) return MTRSSM_EINVAL;
  if (K < 0 || K > MTRSSM_FIT_MAX_SCALARS) { set_error("fit_fold: need 0 <= K <= %d scalars (got %d)", MTRSSM_FIT_MAX_SCALARS, K); return MTRSSM_EINVAL; }
  if (((uintptr_t)grad | (uintptr_t)param) & 15) { set_error("fit_fold: grad and param must be 16-byte aligned"); return MTRSSM_EINVAL; }
  if (((uintptr_t)offsets | (uintptr_t)acc | (uintptr_t)workspace) & 7 || ((uintptr_t)flags | (uintptr_t)group | (uintptr_t)scalars | (uintptr_t)weight) & 3) {
    set_error("fit_fold: offsets, acc and workspace must be 8-byte, flags, group, scalars and weight 4-byte aligned");
    return MTRSSM_EINVAL;
  }
  const int64_t need = mtrssm_fit_fold_workspace_bytes(numel, G, nullptr);
  if (workspace_bytes < need) {
    set_error("fit_fold: the workspace holds %lld bytes, mtrssm_fit_fold_workspace_bytes asks for %lld", (long long)workspace_bytes, (long long)need);
    return MTRSSM_EINVAL;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* sums = static_cast<double*>(workspace);
  double* partial = sums + 3 * MTRSSM_FIT_MAX_SEGMENTS;
  const int64_t blocks = (numel + kChunk - 1) / kChunk + G;
  set_last_kernel("mtrssm::fit_partial_kernel");
  hipLaunchKernelGGL(fit_partial_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, grad, param, offsets, (int)G, numel, partial);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    set_last_kernel("mtrssm::fit_finish_kernel");
    hipLaunchKernelGGL(fit_finish_kernel, dim3(1), dim3(kFinalThreads), 0, s, partial, offsets, group, (int)G, blocks, scalars, (int)K, scalar_scale, grad_scale,
                       clip_norm, weight, sums, acc, flags);
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    set_error("fit_fold launch failed: %s", hipGetErrorString(e));
    return MTRSSM_ELAUNCH;
  }
  return MTRSSM_OK;
}
