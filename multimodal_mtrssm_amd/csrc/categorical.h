// The categorical head of the INITIAL state, one categorical per call: the device code shared by categorical_sample_*_kernel
// (train_ops.hip) and the fused initial-state kernels (init_state.hip), so that both give the same values to the bit.
#pragma once
#include <hip/hip_runtime.h>

namespace mtrssm {

// C logits `x` + one uniform -> log-probabilities, probabilities and the inverse-CDF one-hot sample; the classes are walked in
// order (the cumulative sum is an fp32 left fold, as torch's on the host; a draw ON a CDF edge goes to the next class).
__device__ __forceinline__ void categorical_sample_one(const float* x, float uu, int C, float* logp, float* probs, float* onehot) {
  float m = x[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
  float sum = 0.f;
  for (int c = 0; c < C; ++c) sum += expf(x[c] - m);
  // The log-probabilities reach |logp| > 8, where `(x - m) - logf(sum)` in fp32 is three roundings of up to half an ulp
  // (4.8e-7) each: the log-sum and the differences in double, one rounding at the end (a thread per categorical, once per
  // rollout: no cost).  Probabilities and the sample stay the fp32 left fold the scans and the host use.
  double dsum = 0.0;
  for (int c = 0; c < C; ++c) dsum += exp((double)x[c] - (double)m);
  const double ls = log(dsum);
  float acc = 0.f;
  int idx = 0;
  for (int c = 0; c < C; ++c) {
    const float p = expf(x[c] - m) / sum;
    probs[c] = p;
    logp[c] = (float)(((double)x[c] - (double)m) - ls);
    acc += p;
    if (c + 1 < C && acc <= uu) ++idx;
  }
  for (int c = 0; c < C; ++c) onehot[c] = c == idx ? 1.f : 0.f;
}

// d logits of the same head: through the probabilities (g_p: the straight-through sample's gradient plus any gradient of the
// probabilities themselves; may be null) and through the log-probabilities (g_l, may be null):
//   d x_c = p_c (g_p[c] - sum_j p_j g_p[j]) + g_l[c] - p_c sum_j g_l[j]
__device__ __forceinline__ void categorical_grad_one(const float* probs, const float* g_p, const float* g_l, int C, float* d_logits) {
  float dot = 0.f, sl = 0.f;
  for (int c = 0; c < C; ++c) {
    const float p = probs[c];
    if (g_p) dot += p * g_p[c];
    if (g_l) sl += g_l[c];
  }
  for (int c = 0; c < C; ++c) {
    const float p = probs[c];
    float d = 0.f;
    if (g_p) d += p * (g_p[c] - dot);
    if (g_l) d += g_l[c] - p * sl;
    d_logits[c] = d;
  }
}

}  // namespace mtrssm
