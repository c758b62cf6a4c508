// Held-out likelihood for gfx950: the latent log-ratio of the classes a sampled posterior took, and the
// importance-weighted bound folded over time from S sampled trajectories per row.  Both kernels compute in double, reduce in a fixed
// order without atomics and round every output to fp32 once, so their results are bitwise reproducible.
#include "row_fold.h"
#include "scan_common.h"

namespace mtrssm {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxSamples = 16;
constexpr int kTile = 512;                            // floats of each input a wave stages in LDS
constexpr double kHalfLog2Pi = 0.9189385332046727;    // 0.5 * log(2 * pi)

// log p_k(c*) - log q_k(c*) of one categorical whose C logits lie at q / p (LDS), c* = the first c with stoch > 0.5 (0 when there
// is none).  Max, log-sum and the differences in double; bitwise-equal q and p give exactly 0.
__device__ __forceinline__ double cat_log_ratio(const float* q, const float* p, const float* stoch, int C) {
  double qm = q[0], pm = p[0];
  int cs = -1;
  for (int c = 0; c < C; ++c) {
    qm = fmax(qm, (double)q[c]);
    pm = fmax(pm, (double)p[c]);
    if (cs < 0 && stoch[c] > 0.5f) cs = c;
  }
  if (cs < 0) cs = 0;
  double qs = 0.0, ps = 0.0;
  for (int c = 0; c < C; ++c) {
    qs += exp((double)q[c] - qm);
    ps += exp((double)p[c] - pm);
  }
  return (((double)p[cs] - pm) - log(ps)) - (((double)q[cs] - qm) - log(qs));
}

// C <= kTile.  A wave stages a contiguous span of the three inputs in LDS with coalesced loads (lane i reads float i, i + 64, ...),
// then a lane owns one categorical of the span.  When a whole row fits (K * C <= kTile) the span is R consecutive rows
// (R * K <= 64 where K allows, so every lane has work) and lane r sums row r's K differences in ascending k; else the span is kc
// categoricals of ONE row and lane 0 carries the row's running sum across the spans, still in ascending k.  The trip counts
// depend on nothing but the launch's sizes, so the workgroup barriers are uniform.
__global__ __launch_bounds__(kThreads) void latent_log_ratio_kernel(const float* __restrict__ post, const float* __restrict__ prior,
                                                                    const float* __restrict__ stoch, int64_t rows, int K, int C, int R, int kc,
                                                                    int accumulate, float* __restrict__ out) {
  __shared__ float s_q[kWaves][kTile], s_p[kWaves][kTile], s_s[kWaves][kTile];
  __shared__ double s_d[kWaves][kTile];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t N = (int64_t)K * C;
  const int64_t groups = (rows + R - 1) / R;
  for (int64_t g0 = (int64_t)blockIdx.x * kWaves; g0 < groups; g0 += (int64_t)gridDim.x * kWaves) {
    const int64_t row0 = (g0 + wave) * R;
    const int nr = row0 >= rows ? 0 : (int)(rows - row0 < R ? rows - row0 : R);  // rows of this wave's span (0: nothing to do)
    double acc = 0.0;                                                             // (lane r: the running sum of row row0 + r)
    for (int k0 = 0; k0 < K; k0 += kc) {
      const int nk = K - k0 < kc ? K - k0 : kc;
      const int64_t base = row0 * N + (int64_t)k0 * C;
      const int n = nr * nk * C;  // (nr > 1 only with nk == K: the span is contiguous)
      for (int i = lane; i < n; i += kWave) {
        s_q[wave][i] = post[base + i];
        s_p[wave][i] = prior[base + i];
        s_s[wave][i] = stoch[base + i];
      }
      __syncthreads();
      for (int j = lane; j < nr * nk; j += kWave) s_d[wave][j] = cat_log_ratio(&s_q[wave][j * C], &s_p[wave][j * C], &s_s[wave][j * C], C);
      __syncthreads();
      if (lane < nr)
        for (int k = 0; k < nk; ++k) acc += s_d[wave][lane * nk + k];
      __syncthreads();  // (the next span overwrites the staging buffers)
    }
    if (lane < nr) out[row0 + lane] = accumulate ? (float)((double)out[row0 + lane] + acc) : (float)acc;
  }
}

__device__ __forceinline__ double shfl_xor_d(double v, int mask) { return __shfl_xor(v, mask, kWave); }

// C > kTile: a wave walks one row, categorical by categorical; the lanes stride the classes (coalesced) and meet in butterfly
// reductions of a fixed order.  Lane 0 carries the sum in ascending k.
__global__ __launch_bounds__(kThreads) void latent_log_ratio_long_kernel(const float* __restrict__ post, const float* __restrict__ prior,
                                                                         const float* __restrict__ stoch, int64_t rows, int K, int C,
                                                                         int accumulate, float* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int64_t row = (int64_t)blockIdx.x * kWaves + wave; row < rows; row += (int64_t)gridDim.x * kWaves) {  // (wave-uniform)
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      const int64_t base = (row * K + k) * (int64_t)C;
      float qm = -INFINITY, pm = -INFINITY;
      int cs = C;
      for (int c = lane; c < C; c += kWave) {
        qm = fmaxf(qm, post[base + c]);
        pm = fmaxf(pm, prior[base + c]);
        if (cs == C && stoch[base + c] > 0.5f) cs = c;
      }
      qm = wave_max(qm);
      pm = wave_max(pm);
      double qs = 0.0, ps = 0.0;
      for (int c = lane; c < C; c += kWave) {
        qs += exp((double)post[base + c] - (double)qm);
        ps += exp((double)prior[base + c] - (double)pm);
      }
      for (int m = 1; m < kWave; m <<= 1) {
        qs += shfl_xor_d(qs, m);
        ps += shfl_xor_d(ps, m);
        const int other = __shfl_xor(cs, m, kWave);
        cs = other < cs ? other : cs;
      }
      if (cs == C) cs = 0;
      acc += (((double)prior[base + cs] - (double)pm) - log(ps)) - (((double)post[base + cs] - (double)qm) - log(qs));
    }
    if (lane == 0) out[row] = accumulate ? (float)((double)out[row] + acc) : (float)acc;
  }
}

// (the sums and the max over a 16-lane DPP row, row_sum_d / row_max_d, are in row_fold.h: mtrssm_particle_fold uses them too)
// A 16-lane DPP row per batch row b (four per wave), lane s of it owns sample s and walks the frames serially, carrying
// cum[b][s] in a register; the lanes s >= S carry the neutral element of every reduction.  No lane leaves before the end: the DPP
// steps need the whole wave.  Lane 0 of a row writes the eight planes of a frame.
__global__ __launch_bounds__(kThreads) void iw_bound_kernel(const float* __restrict__ se_audio, const float* __restrict__ se_vision,
                                                            const float* __restrict__ log_ratio, const int32_t* __restrict__ valid, int B, int S,
                                                            int T, double const_audio, double const_vision, float* __restrict__ planes) {
  const int s = threadIdx.x & 15;
  const int b = (int)((blockIdx.x * (int64_t)kThreads + threadIdx.x) >> 4);
  const bool row = b < B, own = row && s < S;
  int n = 0;
  if (row) {
    n = valid ? valid[b] : T;
    n = n < 0 ? 0 : (n > T ? T : n);
  }
  const int64_t in0 = ((int64_t)(row ? b : 0) * S + (own ? s : 0)) * T;
  const int64_t plane = (int64_t)B * T, out0 = (int64_t)(row ? b : 0) * T;
  const double s_d = (double)S, log_s = log(s_d);
  double cum = 0.0, l_prev = 0.0, m_prev = 0.0;
  // the next frame's three inputs are requested before this frame's arithmetic: the loads' latency hides behind it
  float na = 0.f, nv = 0.f, nr = 0.f;
  if (own && 0 < n) {
    if (se_audio) na = se_audio[in0];
    if (se_vision) nv = se_vision[in0];
    if (log_ratio) nr = log_ratio[in0];
  }
  for (int t = 0; t < T; ++t) {
    const bool live = t < n;  // (uniform over the row of 16)
    const float fa = na, fv = nv, fr = nr;
    if (own && t + 1 < n) {
      if (se_audio) na = se_audio[in0 + t + 1];
      if (se_vision) nv = se_vision[in0 + t + 1];
      if (log_ratio) nr = log_ratio[in0 + t + 1];
    }
    double a = 0.0, v = 0.0, r = 0.0;
    if (own && live) {
      if (se_audio) a = -(double)fa - const_audio;
      if (se_vision) v = -(double)fv - const_vision;
      if (log_ratio) r = (double)fr;
    }
    cum += (a + v) + r;
    const double mx = row_max_d(own ? cum : -INFINITY);
    const double w = own ? exp(cum - mx) : 0.0;
    const double sum_w = row_sum_d(w), sum_w2 = row_sum_d(w * w), sum_cum = row_sum_d(own ? cum : 0.0);
    const double sum_a = row_sum_d(a), sum_v = row_sum_d(v), sum_r = row_sum_d(r);
    if (row && s == 0) {
      float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (live) {
        const double l_now = (mx + log(sum_w)) - log_s, m_now = sum_cum / s_d;
        o[0] = (float)(l_now - l_prev);
        o[1] = (float)(m_now - m_prev);
        o[2] = (float)(sum_a / s_d);
        o[3] = (float)(sum_v / s_d);
        o[4] = (float)(sum_r / s_d);
        o[5] = (float)((sum_w * sum_w) / sum_w2);
        o[6] = (float)l_now;
        o[7] = (float)m_now;
        l_prev = l_now;
        m_prev = m_now;
      }
#pragma unroll
      for (int p = 0; p < 8; ++p) planes[p * plane + out0 + t] = o[p];
    }
  }
}

}  // namespace

int latent_log_ratio_launch(const float* post_logits, const float* prior_logits, const float* stoch, int64_t rows, int64_t K, int64_t C,
                            int accumulate, float* out, hipStream_t s) {
  if (!post_logits || !prior_logits || !stoch || !out) { set_error("latent_log_ratio: null pointer"); return MTRSSM_EINVAL; }
  if (rows <= 0 || K <= 0 || C <= 0) {
    set_error("latent_log_ratio: need rows, K, C > 0 (got %lld %lld %lld)", (long long)rows, (long long)K, (long long)C);
    return MTRSSM_EINVAL;
  }
  int64_t width = 0, elems = 0;
  if (__builtin_mul_overflow(K, C, &width) || __builtin_mul_overflow(rows, width, &elems) || elems >= (int64_t)1 << 31) {
    set_error("latent_log_ratio: rows * K * C must stay below 2^31 (got %lld %lld %lld)", (long long)rows, (long long)K, (long long)C);
    return MTRSSM_EINVAL;
  }
  if (accumulate != 0 && accumulate != 1) { set_error("latent_log_ratio: accumulate is 0 or 1 (got %d)", accumulate); return MTRSSM_EINVAL; }
  if (((uintptr_t)post_logits | (uintptr_t)prior_logits | (uintptr_t)stoch | (uintptr_t)out) & 3) {
    set_error("latent_log_ratio: buffers must be 4-byte aligned");
    return MTRSSM_EINVAL;
  }
  if (C > kTile) {
    const int64_t blocks = (rows + kWaves - 1) / kWaves;
    set_last_kernel("mtrssm::latent_log_ratio_long_kernel");
    hipLaunchKernelGGL(latent_log_ratio_long_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kThreads), 0, s, post_logits, prior_logits,
                       stoch, rows, (int)K, (int)C, accumulate, out);
    return check_launch("latent_log_ratio");
  }
  int R = 1, kc = (int)K;
  if (width <= kTile) {  // whole rows: as many as fit the tile, and no more than give every lane a categorical
    const int fit = (int)(kTile / width), want = (int)((kWave + K - 1) / K);
    R = fit < want ? fit : want;
  } else {
    kc = kTile / (int)C;
  }
  const int64_t groups = (rows + R - 1) / R, blocks = (groups + kWaves - 1) / kWaves;
  set_last_kernel("mtrssm::latent_log_ratio_kernel");
  hipLaunchKernelGGL(latent_log_ratio_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kThreads), 0, s, post_logits, prior_logits, stoch,
                     rows, (int)K, (int)C, R, kc, accumulate, out);
  return check_launch("latent_log_ratio");
}

int iw_bound_launch(const float* se_audio, const float* se_vision, const float* log_ratio, const int32_t* valid, int64_t B, int64_t S, int64_t T,
                    int64_t event_audio, int64_t event_vision, float* planes, hipStream_t s) {
  if (!planes || (!se_audio && !se_vision && !log_ratio)) { set_error("iw_bound: null pointer (planes, or all three inputs)"); return MTRSSM_EINVAL; }
  if (B <= 0 || T <= 0 || (se_audio && event_audio <= 0) || (se_vision && event_vision <= 0)) {
    set_error("iw_bound: need B, T > 0 and an event size > 0 for every data term given (got %lld %lld %lld %lld)", (long long)B, (long long)T,
              (long long)event_audio, (long long)event_vision);
    return MTRSSM_EINVAL;
  }
  if (S < 1 || S > kMaxSamples) { set_error("iw_bound: need 1 <= S <= %d samples (got %lld)", kMaxSamples, (long long)S); return MTRSSM_EINVAL; }
  if (B >= (int64_t)1 << 24 || T >= (int64_t)1 << 24 || B * T >= (int64_t)1 << 24) {
    set_error("iw_bound: %lld x %lld frames (B * T must stay below 2^24)", (long long)B, (long long)T);
    return MTRSSM_EINVAL;
  }
  if (((uintptr_t)se_audio | (uintptr_t)se_vision | (uintptr_t)log_ratio | (uintptr_t)valid | (uintptr_t)planes) & 3) {
    set_error("iw_bound: buffers must be 4-byte aligned");
    return MTRSSM_EINVAL;
  }
  const int64_t blocks = (B * 16 + kThreads - 1) / kThreads;
  set_last_kernel("mtrssm::iw_bound_kernel");
  hipLaunchKernelGGL(iw_bound_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, se_audio, se_vision, log_ratio, valid, (int)B, (int)S, (int)T,
                     kHalfLog2Pi * (double)event_audio, kHalfLog2Pi * (double)event_vision, planes);
  return check_launch("iw_bound");
}

}  // namespace mtrssm
