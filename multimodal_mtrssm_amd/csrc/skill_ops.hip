// Forecast skill for gfx950: the per-frame ensemble scores of S sampled reconstructions and the fold of
// the score planes into a table by horizon.  The scorer streams ((S + 1) * E * 4 bytes per frame, 16 B per lane coalesced; measured rates in 6h);
// both kernels reduce in a fixed order and use no float atomics, so their results are bitwise reproducible.
#include "scan_common.h"

namespace mtrssm {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxSamples = 16;
constexpr int kMaxPlanes = 64;

// sum_e 0.5 (x_e - y_e)^2 over one quad.  Not contracted: the score of a sample and the score of the ensemble mean go through
// the same roundings, so with S = 1 (ybar = y_0) they are bitwise equal.
__device__ __forceinline__ float half_sq(const float4 x, const float4 y) {
#pragma clang fp contract(off)
  const float a = x.x - y.x, b = x.y - y.y, c = x.z - y.z, d = x.w - y.w;
  return 0.5f * (a * a) + 0.5f * (b * b) + 0.5f * (c * c) + 0.5f * (d * d);
}

// ybar and the spread of one element: both left folds over s, as the rule states them
template <int S>
__device__ __forceinline__ float fold_elem(const float (&y)[S], float s_f, float& spread) {
#pragma clang fp contract(off)
  float sum = y[0];
#pragma unroll
  for (int s = 1; s < S; ++s) sum += y[s];
  const float ybar = sum / s_f;
  float var = (y[0] - ybar) * (y[0] - ybar);
#pragma unroll
  for (int s = 1; s < S; ++s) var += (y[s] - ybar) * (y[s] - ybar);
  spread += 0.5f * var / s_f;
  return ybar;
}

// One workgroup per frame (b, t), grid-stride over the frames.  A lane holds one quad of the target and the S quads of the
// samples at the same elements (S * 4 floats), so ybar and the spread need no second pass over memory.  Per frame S + 2 sums
// (se_0 .. se_{S-1}, ens, spread) are reduced: in-lane over the lane's quads in ascending order, the DPP tree inside a wave, the
// four waves in ascending order by thread 0.  A dead frame (t >= valid[b]) loads nothing and scores 0.
template <int S, bool TANH>
__global__ __launch_bounds__(kThreads) void ensemble_score_kernel(
    const float* __restrict__ pred, const float* __restrict__ target, const int32_t* __restrict__ valid, int64_t frames, int T, int64_t E4,
    float* __restrict__ mean, float* __restrict__ ens, float* __restrict__ best, float* __restrict__ spread, float* __restrict__ se_samples) {
  __shared__ float red[kWaves][S + 2];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const float s_f = (float)S;
  for (int64_t f = blockIdx.x; f < frames; f += gridDim.x) {
    const int64_t b = f / T;
    const int t = (int)(f - b * T);
    const int64_t row0 = (b * S) * T + t;  // frame of sample 0 in pred / se_samples; sample s is s * T frames further
    if (valid && t >= valid[b]) {          // (uniform over the workgroup)
      if (threadIdx.x == 0) {
        mean[f] = ens[f] = best[f] = spread[f] = 0.f;
        if (se_samples)
          for (int s = 0; s < S; ++s) se_samples[row0 + (int64_t)s * T] = 0.f;
      }
      continue;
    }
    const float4* x4 = reinterpret_cast<const float4*>(target) + f * E4;
    const float4* p4 = reinterpret_cast<const float4*>(pred) + row0 * E4;
    const int64_t sample_stride = (int64_t)T * E4;
    float se[S], a_ens = 0.f, a_spread = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s) se[s] = 0.f;
    for (int64_t i = threadIdx.x; i < E4; i += kThreads) {
      const float4 x = x4[i];
      float4 y[S];
#pragma unroll
      for (int s = 0; s < S; ++s) y[s] = p4[s * sample_stride + i];
      float yx[S], yy[S], yz[S], yw[S];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        if (TANH) { y[s].x = tanh_fast(y[s].x); y[s].y = tanh_fast(y[s].y); y[s].z = tanh_fast(y[s].z); y[s].w = tanh_fast(y[s].w); }
        se[s] += half_sq(x, y[s]);
        yx[s] = y[s].x; yy[s] = y[s].y; yz[s] = y[s].z; yw[s] = y[s].w;
      }
      float4 ybar;
      ybar.x = fold_elem<S>(yx, s_f, a_spread);
      ybar.y = fold_elem<S>(yy, s_f, a_spread);
      ybar.z = fold_elem<S>(yz, s_f, a_spread);
      ybar.w = fold_elem<S>(yw, s_f, a_spread);
      a_ens += half_sq(x, ybar);
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const float v = wave_sum(se[s]);
      if (lane == 0) red[wave][s] = v;
    }
    a_ens = wave_sum(a_ens);
    a_spread = wave_sum(a_spread);
    if (lane == 0) { red[wave][S] = a_ens; red[wave][S + 1] = a_spread; }
    __syncthreads();
    if (threadIdx.x == 0) {
      float tot[S + 2];
#pragma unroll
      for (int k = 0; k < S + 2; ++k) {
        float v = red[0][k];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v += red[w][k];
        tot[k] = v;
      }
      float sum = tot[0], low = tot[0];
#pragma unroll
      for (int s = 1; s < S; ++s) { sum += tot[s]; low = fminf(low, tot[s]); }
      mean[f] = sum / s_f;
      best[f] = low;
      ens[f] = tot[S];
      spread[f] = tot[S + 1];
      if (se_samples) {
#pragma unroll
        for (int s = 0; s < S; ++s) se_samples[row0 + (int64_t)s * T] = tot[s];
      }
    }
    __syncthreads();  // (red is written again by the next frame)
  }
}

// sums[p][h] += planes[p][b][t] over the live frames with horizon h, counts[h] += 1: one thread per (p, h), p = P the counts.
// With c_b = clamp(context[b], 1, T) and n_b = clamp(valid[b], 0, T), bin 0 takes the frames t < min(c_b, n_b) of a row and bin
// h >= 1 the one frame t = c_b + h - 1 when it is live.  A thread walks the rows in ascending b (bin 0: ascending t inside a
// row) and adds onto the value already in the buffer: a left fold, the same for every launch shape.
__global__ __launch_bounds__(kThreads) void horizon_table_kernel(const float* __restrict__ planes, int P, const int32_t* __restrict__ context,
                                                                 const int32_t* __restrict__ valid, int B, int T, float* __restrict__ sums,
                                                                 float* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (P + 1) * T) return;
  const int p = i / T, h = i - p * T;
  const float* plane = p < P ? planes + (int64_t)p * B * T : nullptr;
  float* dst = p < P ? sums + (int64_t)p * T + h : counts + h;
  float acc = *dst;
  for (int b = 0; b < B; ++b) {
    int c = context[b];
    c = c < 1 ? 1 : (c > T ? T : c);
    int n = valid ? valid[b] : T;
    n = n < 0 ? 0 : (n > T ? T : n);
    if (h == 0) {
      const int end = c < n ? c : n;
      for (int t = 0; t < end; ++t) acc += plane ? plane[(int64_t)b * T + t] : 1.f;
    } else {
      const int t = c + h - 1;
      if (t < n) acc += plane ? plane[(int64_t)b * T + t] : 1.f;
    }
  }
  *dst = acc;
}

template <int S>
void launch_score(bool tanh, int grid, hipStream_t s, const float* pred, const float* target, const int32_t* valid, int64_t frames, int T,
                  int64_t E4, float* mean, float* ens, float* best, float* spread, float* se_samples) {
  if (tanh)
    hipLaunchKernelGGL((ensemble_score_kernel<S, true>), dim3(grid), dim3(kThreads), 0, s, pred, target, valid, frames, T, E4, mean, ens, best,
                       spread, se_samples);
  else
    hipLaunchKernelGGL((ensemble_score_kernel<S, false>), dim3(grid), dim3(kThreads), 0, s, pred, target, valid, frames, T, E4, mean, ens, best,
                       spread, se_samples);
}

}  // namespace

int ensemble_score_launch(const float* pred, const float* target, const int32_t* valid, int64_t B, int64_t S, int64_t T, int64_t E, int act,
                          float* mean, float* ens, float* best, float* spread, float* se_samples, hipStream_t s) {
  if (!pred || !target || !mean || !ens || !best || !spread) { set_error("ensemble_score: null pointer"); return MTRSSM_EINVAL; }
  if (B <= 0 || T <= 0 || E <= 0) {
    set_error("ensemble_score: need B, T, E > 0 (got %lld %lld %lld)", (long long)B, (long long)T, (long long)E);
    return MTRSSM_EINVAL;
  }
  if (S < 1 || S > kMaxSamples) { set_error("ensemble_score: need 1 <= S <= %d samples (got %lld)", kMaxSamples, (long long)S); return MTRSSM_EINVAL; }
  if (E % 4) { set_error("ensemble_score: E must be a multiple of 4 (16-byte loads), got %lld", (long long)E); return MTRSSM_EINVAL; }
  if (act != MTRSSM_ACT_IDENTITY && act != MTRSSM_ACT_TANH) { set_error("ensemble_score: the fused output activation is Identity or Tanh (got %d)", act); return MTRSSM_EINVAL; }
  int64_t frames = 0, elems = 0;
  if (__builtin_mul_overflow(B, T, &frames) || frames >= (int64_t)1 << 31 || __builtin_mul_overflow(frames * S, E, &elems) ||
      elems >= (int64_t)1 << 60) {
    set_error("ensemble_score: B * T must stay below 2^31 frames and B * S * T * E below 2^60 elements (got %lld %lld %lld %lld)", (long long)B,
              (long long)S, (long long)T, (long long)E);
    return MTRSSM_EINVAL;
  }
  if (((uintptr_t)pred | (uintptr_t)target) & 15) { set_error("ensemble_score: pred/target must be 16-byte aligned"); return MTRSSM_EINVAL; }
  if (((uintptr_t)mean | (uintptr_t)ens | (uintptr_t)best | (uintptr_t)spread | (uintptr_t)se_samples | (uintptr_t)valid) & 3) {
    set_error("ensemble_score: the planes and valid must be 4-byte aligned");
    return MTRSSM_EINVAL;
  }
  const int grid = (int)(frames < 2048 ? frames : 2048);
  const bool tanh = act == MTRSSM_ACT_TANH;
  set_last_kernel("mtrssm::ensemble_score_kernel");
#define MTRSSM_SCORE(N) case N: launch_score<N>(tanh, grid, s, pred, target, valid, frames, (int)T, E / 4, mean, ens, best, spread, se_samples); break;
  switch ((int)S) {
    MTRSSM_SCORE(1) MTRSSM_SCORE(2) MTRSSM_SCORE(3) MTRSSM_SCORE(4) MTRSSM_SCORE(5) MTRSSM_SCORE(6) MTRSSM_SCORE(7) MTRSSM_SCORE(8)
    MTRSSM_SCORE(9) MTRSSM_SCORE(10) MTRSSM_SCORE(11) MTRSSM_SCORE(12) MTRSSM_SCORE(13) MTRSSM_SCORE(14) MTRSSM_SCORE(15) MTRSSM_SCORE(16)
    default: set_error("ensemble_score: no instance for S = %lld", (long long)S); return MTRSSM_EINVAL;
  }
#undef MTRSSM_SCORE
  return check_launch("ensemble_score");
}

int horizon_table_launch(const float* planes, int64_t P, const int32_t* context, const int32_t* valid, int64_t B, int64_t T, float* sums,
                         float* counts, hipStream_t s) {
  if (!planes || !context || !sums || !counts) { set_error("horizon_table: null pointer"); return MTRSSM_EINVAL; }
  if (P < 1 || P > kMaxPlanes || B <= 0 || T <= 0) {
    set_error("horizon_table: need 1 <= P <= %d and B, T > 0 (got %lld %lld %lld)", kMaxPlanes, (long long)P, (long long)B, (long long)T);
    return MTRSSM_EINVAL;
  }
  if (B >= (int64_t)1 << 24 || T >= (int64_t)1 << 24 || B * T >= (int64_t)1 << 24) {
    set_error("horizon_table: %lld x %lld frames (the fp32 counts are exact below 2^24)", (long long)B, (long long)T);
    return MTRSSM_EINVAL;
  }
  if (((uintptr_t)planes | (uintptr_t)context | (uintptr_t)valid | (uintptr_t)sums | (uintptr_t)counts) & 3) {
    set_error("horizon_table: buffers must be 4-byte aligned");
    return MTRSSM_EINVAL;
  }
  const int64_t threads = (P + 1) * T;
  set_last_kernel("mtrssm::horizon_table_kernel");
  hipLaunchKernelGGL(horizon_table_kernel, dim3((unsigned)((threads + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, planes, (int)P, context, valid,
                     (int)B, (int)T, sums, counts);
  return check_launch("horizon_table");
}

}  // namespace mtrssm
