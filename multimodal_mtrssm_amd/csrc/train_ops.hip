// Streaming train-step ops for gfx950: fused Gaussian NLL (objective.py:7-23) and a flat fused
// AdamW with global-norm clipping (default.yaml:103-107,119).  All are HBM-bound: 16 B per lane
// coalesced accesses, grid-stride over <= 2048 workgroups, wave64 shuffle reductions, one atomic
// per workgroup.
#include "scan_common.h"
#include "categorical.h"

namespace mtrssm {

constexpr int kThreads = 256;

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x < kWave) {
    t = threadIdx.x < blockDim.x / kWave ? red[threadIdx.x] : 0.f;
    t = wave_sum(t);
  }
  return t;  // valid in wave 0
}

// tanh_fast (scan_common.h): libm's tanhf made the two NLL kernels VALU-bound (41 / 25 us for a 105 MB stream).
// out += scale * sum 0.5 (t - p)^2   (+ the constant on block 0)
template <bool TANH>
__global__ void nll_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, int64_t n,
                               float scale, float constant, float* __restrict__ out) {
  __shared__ float red[kThreads / kWave];
  const int64_t n4 = n / 4;
  const float4* p4 = reinterpret_cast<const float4*>(pred);
  const float4* t4 = reinterpret_cast<const float4*>(target);
  float acc = 0.f;
  auto term = [](float4 p, const float4 t) {
    if (TANH) { p.x = tanh_fast(p.x); p.y = tanh_fast(p.y); p.z = tanh_fast(p.z); p.w = tanh_fast(p.w); }
    const float a = t.x - p.x, b = t.y - p.y, c = t.z - p.z, d = t.w - p.w;
    return 0.5f * (a * a) + 0.5f * (b * b) + 0.5f * (c * c) + 0.5f * (d * d);
  };
  // four quads per thread and iteration in flight; few workgroups (the launch picks 512): every workgroup ends in ONE atomic
  // on the same word, ~25 ns each when they queue up (2048 of them were 40 us of a 41 us kernel)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const float4 pa = p4[i], pb = p4[i + stride], pc = p4[i + 2 * stride], pd = p4[i + 3 * stride];
    const float4 ta = t4[i], tb = t4[i + stride], tc = t4[i + 2 * stride], td = t4[i + 3 * stride];
    acc += (term(pa, ta) + term(pb, tb)) + (term(pc, tc) + term(pd, td));
  }
  for (; i < n4; i += stride) acc += term(p4[i], t4[i]);
  if (blockIdx.x == 0) {
    for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
      const float a = target[i] - (TANH ? tanh_fast(pred[i]) : pred[i]);
      acc += 0.5f * a * a;
    }
  }
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) atomicAdd(out, tot * scale + (blockIdx.x == 0 ? constant : 0.f));
}

// d/dz of 0.5 (t - act(z))^2 = (act(z) - t) act'(z); Tanh: act' = 1 - act^2
template <bool TANH>
__global__ void nll_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                               const float* __restrict__ g_out, int64_t n, float inv_frames, float* __restrict__ g_pred) {
  const float g = g_out[0] * inv_frames;
  const int64_t n4 = n / 4;
  const float4* p4 = reinterpret_cast<const float4*>(pred);
  const float4* t4 = reinterpret_cast<const float4*>(target);
  float4* o4 = reinterpret_cast<float4*>(g_pred);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 p = p4[i];
    const float4 t = t4[i];
    float4 d = make_float4(1.f, 1.f, 1.f, 1.f);
    if (TANH) {
      p.x = tanh_fast(p.x); p.y = tanh_fast(p.y); p.z = tanh_fast(p.z); p.w = tanh_fast(p.w);
      d = make_float4(1.f - p.x * p.x, 1.f - p.y * p.y, 1.f - p.z * p.z, 1.f - p.w * p.w);
    }
    o4[i] = make_float4(g * (p.x - t.x) * d.x, g * (p.y - t.y) * d.y, g * (p.z - t.z) * d.z, g * (p.w - t.w) * d.w);
  }
  if (blockIdx.x == 0)
    for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
      const float p = TANH ? tanh_fast(pred[i]) : pred[i];
      g_pred[i] = g * (p - target[i]) * (TANH ? 1.f - p * p : 1.f);
    }
}

// The NLL over the frames a modality is present in (core.py, missing modalities): an element of frame n counts when
// present[n] != 0, the sum is divided by the device scalar *count (0 -> the loss is 0).  *count need not be the number of
// present frames (a data-parallel rank: the global batch's / world); the constant 0.5 log(2 pi) per element belongs to the
// per-frame term and is divided by it too: constant * (present frames) / count.  An absent element is taken out with a select
// (forward: the difference before it is squared; backward: the finished product), so it may hold NaN or Inf, and with every
// frame present the arithmetic -- and the launch shape -- is nll_fwd_kernel's.
// EV4: event % 4 == 0, one frame per quad (one frame index per quad).  Frame indices are 32-bit divisions: the launchers
// take n < 2^31 elements only.
__device__ __forceinline__ bool frame_present(const float* __restrict__ present, uint32_t e, uint32_t event) {
  return present[e / event] != 0.f;
}

// the elements of the quad starting at element e0 that lie in absent frames set to 0 (a select: whatever they held, NaN included)
template <bool EV4>
__device__ __forceinline__ float4 masked_zero(const float* __restrict__ present, uint32_t e0, uint32_t event, float4 a) {
  if (EV4) {
    if (!frame_present(present, e0, event)) a = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    if (!frame_present(present, e0, event)) a.x = 0.f;
    if (!frame_present(present, e0 + 1, event)) a.y = 0.f;
    if (!frame_present(present, e0 + 2, event)) a.z = 0.f;
    if (!frame_present(present, e0 + 3, event)) a.w = 0.f;
  }
  return a;
}

template <bool EV4>
__device__ __forceinline__ float4 masked_diff(const float* __restrict__ present, uint32_t e0, uint32_t event, float4 t, float4 p) {
  return masked_zero<EV4>(present, e0, event, make_float4(t.x - p.x, t.y - p.y, t.z - p.z, t.w - p.w));
}

template <bool TANH, bool EV4>
__global__ void nll_masked_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ present,
                                      const float* __restrict__ count, int64_t n, int64_t event, float constant, float* __restrict__ out) {
  __shared__ float red[kThreads / kWave];
  const int64_t n4 = n / 4;
  const float4* p4 = reinterpret_cast<const float4*>(pred);
  const float4* t4 = reinterpret_cast<const float4*>(target);
  float acc = 0.f;
  auto term = [&](int64_t i, float4 p, const float4 t) {
    if (TANH) { p.x = tanh_fast(p.x); p.y = tanh_fast(p.y); p.z = tanh_fast(p.z); p.w = tanh_fast(p.w); }
    const float4 q = masked_diff<EV4>(present, (uint32_t)(4 * i), (uint32_t)event, t, p);
    const float a = q.x, b = q.y, c = q.z, d = q.w;
    return 0.5f * (a * a) + 0.5f * (b * b) + 0.5f * (c * c) + 0.5f * (d * d);
  };
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const float4 pa = p4[i], pb = p4[i + stride], pc = p4[i + 2 * stride], pd = p4[i + 3 * stride];
    const float4 ta = t4[i], tb = t4[i + stride], tc = t4[i + 2 * stride], td = t4[i + 3 * stride];
    acc += (term(i, pa, ta) + term(i + stride, pb, tb)) + (term(i + 2 * stride, pc, tc) + term(i + 3 * stride, pd, td));
  }
  for (; i < n4; i += stride) acc += term(i, p4[i], t4[i]);
  if (blockIdx.x == 0) {
    for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
      const float a = frame_present(present, (uint32_t)i, (uint32_t)event) ? target[i] - (TANH ? tanh_fast(pred[i]) : pred[i]) : 0.f;
      acc += 0.5f * a * a;
    }
  }
  const float tot = block_sum(acc, red);
  const float cnt = count[0];
  // the constant is a term of every PRESENT frame and is divided by *count like the rest: constant * sum(present) / count.
  // Block 0 counts the frames (whole numbers in fp32: exact below 2^24); with count = sum(present) the quotient is exactly 1.
  float share = 0.f;
  if (blockIdx.x == 0) {
    __syncthreads();  // `red` is read by wave 0 above
    float np = 0.f;
    for (int64_t f = threadIdx.x; f < n / event; f += blockDim.x) np += present[f] != 0.f ? 1.f : 0.f;
    share = block_sum(np, red) / cnt;
  }
  if (threadIdx.x == 0 && cnt > 0.f) atomicAdd(out, tot * (1.f / cnt) + (blockIdx.x == 0 ? constant * share : 0.f));
}

template <bool TANH, bool EV4>
__global__ void nll_masked_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ present,
                                      const float* __restrict__ count, const float* __restrict__ g_out, int64_t n, int64_t event,
                                      float* __restrict__ g_pred) {
  const float cnt = count[0];
  const float g = cnt > 0.f ? g_out[0] * (1.f / cnt) : 0.f;
  const int64_t n4 = n / 4;
  const float4* p4 = reinterpret_cast<const float4*>(pred);
  const float4* t4 = reinterpret_cast<const float4*>(target);
  float4* o4 = reinterpret_cast<float4*>(g_pred);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 p = p4[i];
    const float4 t = t4[i];
    float4 d = make_float4(1.f, 1.f, 1.f, 1.f);
    if (TANH) {
      p.x = tanh_fast(p.x); p.y = tanh_fast(p.y); p.z = tanh_fast(p.z); p.w = tanh_fast(p.w);
      d = make_float4(1.f - p.x * p.x, 1.f - p.y * p.y, 1.f - p.z * p.z, 1.f - p.w * p.w);
    }
    // absent elements are zeroed AFTER the product, as in the tail below: an absent frame's prediction may be anything (NaN: a
    // frame nobody computed), and 0 * (1 - tanh(NaN)^2) is NaN.  With every frame present this is nll_bwd_kernel's arithmetic.
    const float4 r = make_float4(g * (p.x - t.x) * d.x, g * (p.y - t.y) * d.y, g * (p.z - t.z) * d.z, g * (p.w - t.w) * d.w);
    o4[i] = masked_zero<EV4>(present, (uint32_t)(4 * i), (uint32_t)event, r);
  }
  if (blockIdx.x == 0)
    for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
      const float p = TANH ? tanh_fast(pred[i]) : pred[i];
      g_pred[i] = frame_present(present, (uint32_t)i, (uint32_t)event) ? g * (p - target[i]) * (TANH ? 1.f - p * p : 1.f) : 0.f;
    }
}

__global__ void sumsq_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ out) {
  __shared__ float red[kThreads / kWave];
  const int64_t n4 = n / 4;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = x4[i];
    acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  if (blockIdx.x == 0)
    for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) acc += x[i] * x[i];
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) atomicAdd(out, tot);
}

// torch.optim.AdamW semantics (decoupled decay, bias correction, eps outside the sqrt's bias term):
//   p *= 1 - lr*wd ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2
//   p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
// preceded by clip_grad_norm_: g *= min(1, clip / (||g|| + 1e-6)), and by grad_scale (e.g. 1/world).
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                             int64_t n, const float* __restrict__ sumsq, float clip, float gscale, float lr, float b1,
                             float b2, float eps, float wd, float bc1, float bc2_sqrt) {
  float coef = gscale;
  if (clip > 0.f && sumsq) {
    const float norm = sqrtf(sumsq[0]) * gscale;
    coef *= fminf(1.f, clip / (norm + 1e-6f));
  }
  const float step = lr / bc1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float gi = g[i] * coef;
    float pi = p[i] * (1.f - lr * wd);
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    pi -= step * mi / (sqrtf(vi) / bc2_sqrt + eps);
    p[i] = pi;
  }
}

// Graph-safe variant: the learning rate and the step count live in device memory (`state`: [0] lr, [1] steps taken,
// [2] 1 - b1^step, [3] sqrt(1 - b2^step)), so a captured train step replays with the right bias correction and sees a
// scheduler's new lr without re-capture.  `active` (one byte per element, may be null) marks the parameters that have ever
// received a gradient: torch.optim.AdamW skips parameters whose .grad is None (no decay, no moments) -- MMTRSSM's
// l_posterior and dummy transition (mmtrssm/mopoe_mmtrssm/core.py:143-151,188).
__global__ void sumsq_tick_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ out, float* __restrict__ state,
                                  const int* __restrict__ status, float b1, float b2) {
  __shared__ float red[kThreads / kWave];
  if (blockIdx.x == 0 && threadIdx.x == 0 && state && !(status && *status)) {  // one optimizer step = one launch of this kernel
    const float step = state[1] + 1.f;
    state[1] = step;
    state[2] = 1.f - powf(b1, step);
    state[3] = sqrtf(1.f - powf(b2, step));
  }
  const int64_t n4 = n / 4;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = x4[i];
    acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  if (blockIdx.x == 0)
    for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) acc += x[i] * x[i];
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) atomicAdd(out, tot);
}

__global__ void adamw_masked_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                    const unsigned char* __restrict__ active, int64_t n, const float* __restrict__ sumsq,
                                    const float* __restrict__ state, const int* __restrict__ status, float clip, float gscale, float b1,
                                    float b2, float eps, float wd) {
  // a cooperative scan kernel of this step gave up on an exchange (sticky status word of its workspace): its outputs, hence
  // these gradients, are invalid -- leave the parameters and the moments alone; the host raises at its next status poll
  if (status && *status) return;
  const float lr = state[0], bc1 = state[2], bc2_sqrt = state[3];
  float coef = gscale;
  if (clip > 0.f && sumsq) {
    const float norm = sqrtf(sumsq[0]) * gscale;
    coef *= fminf(1.f, clip / (norm + 1e-6f));
  }
  const float step = lr / bc1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (active && !active[i]) continue;
    const float gi = g[i] * coef;
    float pi = p[i] * (1.f - lr * wd);
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    pi -= step * mi / (sqrtf(vi) / bc2_sqrt + eps);
    p[i] = pi;
  }
}

__global__ void clear_words_kernel(unsigned* __restrict__ p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0u;
}

int clear_async(void* p, size_t bytes, hipStream_t stream) {
  if (!p || (bytes & 3) || ((uintptr_t)p & 3)) { set_error("clear_async: needs a 4-byte aligned buffer of a multiple of 4 bytes"); return MTRSSM_EINVAL; }
  const size_t n = bytes / 4;
  if (n == 0) return MTRSSM_OK;
  const size_t blocks = (n + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(clear_words_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(kThreads), 0, stream, static_cast<unsigned*>(p), n);
  return hipGetLastError() == hipSuccess ? MTRSSM_OK : MTRSSM_ELAUNCH;
}

static int grid_for(int64_t n) {
  int64_t g = (n + kThreads - 1) / kThreads;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

// ------------------------------------------------------------------------------------------------
// Categorical head of the INITIAL state (core.py:121-135; mmtrssm core.py:321-362): flat logits [rows][K * C] + one uniform per
// categorical -> log-probabilities, probabilities and the inverse-CDF one-hot sample, one thread per (row, categorical), the
// classes walked in order (the cumulative sum is a left fold, as torch's on the host).  Replaces a dozen eager launches per
// level (softmax, log_softmax, cumsum, compare, sum, one_hot, the straight-through add / sub).
// ------------------------------------------------------------------------------------------------
__global__ void categorical_sample_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ u, int64_t n, int C,
                                              float* __restrict__ logp, float* __restrict__ probs, float* __restrict__ onehot) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (row, categorical)
  if (i >= n) return;
  categorical_sample_one(logits + i * C, u[i], C, logp + i * C, probs + i * C, onehot + i * C);   // (categorical.h)
}

// d logits of the same head (categorical.h: categorical_grad_one); g_p and g_l may be null
__global__ void categorical_sample_bwd_kernel(const float* __restrict__ probs, const float* __restrict__ g_p, const float* __restrict__ g_l,
                                              int64_t n, int C, float* __restrict__ d_logits) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  categorical_grad_one(probs + i * C, g_p ? g_p + i * C : nullptr, g_l ? g_l + i * C : nullptr, C, d_logits + i * C);
}

int categorical_sample_fwd_launch(const float* logits, const float* u, int64_t rows, int K, int C, float* logp, float* probs, float* onehot,
                                  hipStream_t s) {
  if (!logits || !u || !logp || !probs || !onehot || rows <= 0 || K <= 0 || C <= 0) { set_error("categorical_sample_fwd: bad argument"); return MTRSSM_EINVAL; }
  const int64_t n = rows * K;
  set_last_kernel("mtrssm::categorical_sample_fwd_kernel");
  hipLaunchKernelGGL(categorical_sample_fwd_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, logits, u, n, C, logp, probs, onehot);
  return check_launch("categorical_sample_fwd");
}

int categorical_sample_bwd_launch(const float* probs, const float* g_p, const float* g_l, int64_t rows, int K, int C, float* d_logits,
                                  hipStream_t s) {
  if (!probs || !d_logits || rows <= 0 || K <= 0 || C <= 0) { set_error("categorical_sample_bwd: bad argument"); return MTRSSM_EINVAL; }
  const int64_t n = rows * K;
  set_last_kernel("mtrssm::categorical_sample_bwd_kernel");
  hipLaunchKernelGGL(categorical_sample_bwd_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, probs, g_p, g_l, n, C, d_logits);
  return check_launch("categorical_sample_bwd");
}

// ------------------------------------------------------------------------------------------------
// The scalar end of shared_step (core.py:187-221; mmtrssm core.py:563-606) in one launch each way, ONE kernel pair for every case:
//   recon = nll_a + nll_v;  kl_j = coeff_j * sum_live(kl_bt_j) / N  (j < nkl <= 2);  loss = recon + sum_j kl_j
// live / count null: every step is live and N = n.  Given (ragged batches): live[i] in {0, 1} and N = the
// device scalar *count (the global batch's live steps / world; 0 -> the term is 0).  Four scalar outputs (o_k1 may be null).
// SCHED (an ElboSchedule): free bits per (b, t), a beta warm-up read from the device scalar *step,
// per-modality reconstruction weights; beside the four scalars it writes beta and stats = { raw_0, raw_1, active_0, active_1 } from
//   s[3j .. 3j + 2] = sum_live clip_j, sum_live kl_j, #{live, not kl_j < free_j}.
// Without SCHED nothing is clipped (a negative entry counts as it is) and one sum per plane is kept, s[j] = sum_live kl_j.
// Every operation is rounded on its own (contraction is switched off in both kernels): schedule.py's torch rule reproduces beta and
// the gradient planes bit for bit.  The sums take block_sum's order (wave_sum, one partial per wave, wave_sum over the partials),
// all of them behind one barrier: the neutral schedule gives the unscheduled scalars bitwise, and with every step live and
// *count == n the counted scalars are the uncounted ones.
// Backward: g = { g_recon, g_kl_0, g_kl_1, g_loss } (any may be null = 0) -> g_nll_a, g_nll_v = g_recon + g_loss (times w_a, w_v);
//   g_kl_bt_j[i] = (g_kl_j + g_loss) * coeff_j (* the beta the forward stored) / N;  a step that is dead or below its threshold
//   gets an explicit zero.
// ------------------------------------------------------------------------------------------------
template <bool SCHED>
__global__ void elbo_fwd_kernel(const float* __restrict__ nll_a, const float* __restrict__ nll_v, const float* __restrict__ kl0,
                                const float* __restrict__ kl1, const float* __restrict__ live, const float* __restrict__ count,
                                const float* __restrict__ step, int64_t n, MtrssmElboSchedule p, float* __restrict__ o_recon,
                                float* __restrict__ o_k0, float* __restrict__ o_k1, float* __restrict__ o_loss, float* __restrict__ o_beta,
                                float* __restrict__ o_stats) {
#pragma clang fp contract(off)
  constexpr int K = SCHED ? 3 : 1;  // sums per KL plane
  __shared__ float red[2 * K][kThreads / kWave];
  float a[2 * K] = {};
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const bool on = !live || live[i] != 0.f;
    auto add = [&](float* acc, float x, float free) {
      if constexpr (SCHED) {
        const bool low = x < free;
        acc[0] += on ? (low ? free : x) : 0.f;
        acc[1] += on ? x : 0.f;
        acc[2] += on && !low ? 1.f : 0.f;
      } else {
        acc[0] += on ? x : 0.f;
      }
    };
    add(a, kl0[i], p.free0);
    if (kl1) add(a + K, kl1[i], p.free1);
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < 2 * K; ++k) {
    const float v = wave_sum(a[k]);
    if (lane == 0) red[k][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x >= kWave) return;
  float s[2 * K];
#pragma unroll
  for (int k = 0; k < 2 * K; ++k) s[k] = wave_sum(threadIdx.x < blockDim.x / kWave ? red[k][threadIdx.x] : 0.f);
  if (threadIdx.x == 0) {
    const float cnt = live ? count[0] : (float)n;
    const bool some = !live || cnt > 0.f;
    float beta = 1.f;
    if (SCHED && p.warmup > 0.f) {
      const float r = step[0] / p.warmup;
      beta = p.beta_start + (1.f - p.beta_start) * (r > 1.f ? 1.f : r);
    }
    auto term = [&](float sum, float c) {
      const float k = sum / cnt * c;
      return SCHED ? k * beta : k;
    };
    const float recon = SCHED ? p.w_a * nll_a[0] + p.w_v * nll_v[0] : nll_a[0] + nll_v[0];
    const float k0 = some ? term(s[0], p.c0) : 0.f, k1 = kl1 && some ? term(s[K], p.c1) : 0.f;
    o_recon[0] = recon; o_k0[0] = k0; if (o_k1) o_k1[0] = k1; o_loss[0] = recon + k0 + k1;
    if constexpr (SCHED) {
      o_beta[0] = beta;
      o_stats[0] = some ? s[1] / cnt * p.c0 : 0.f;
      o_stats[1] = kl1 && some ? s[4] / cnt * p.c1 : 0.f;
      o_stats[2] = some ? s[2] / cnt : 0.f;
      o_stats[3] = kl1 && some ? s[5] / cnt : 0.f;
    }
  }
}
template <bool SCHED>
__global__ void elbo_bwd_kernel(const float* __restrict__ g_recon, const float* __restrict__ g_k0, const float* __restrict__ g_k1,
                                const float* __restrict__ g_loss, const float* __restrict__ kl0, const float* __restrict__ kl1,
                                const float* __restrict__ live, const float* __restrict__ count, const float* __restrict__ beta, int64_t n,
                                MtrssmElboSchedule p, float* __restrict__ g_nll_a, float* __restrict__ g_nll_v, float* __restrict__ g_kl0,
                                float* __restrict__ g_kl1) {
#pragma clang fp contract(off)
  const float gl = g_loss ? g_loss[0] : 0.f;
  const float gn = (g_recon ? g_recon[0] : 0.f) + gl;
  const float cnt = live ? count[0] : (float)n;
  const bool some = !live || cnt > 0.f;
  auto plane = [&](const float* g, float c) {
    const float v = ((g ? g[0] : 0.f) + gl) * c;
    return (SCHED ? v * beta[0] : v) / cnt;
  };
  const float v0 = some ? plane(g_k0, p.c0) : 0.f, v1 = some ? plane(g_k1, p.c1) : 0.f;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) { g_nll_a[0] = SCHED ? p.w_a * gn : gn; g_nll_v[0] = SCHED ? p.w_v * gn : gn; }
  if (i < n) {
    const bool on = !live || live[i] != 0.f;
    g_kl0[i] = on && !(SCHED && kl0[i] < p.free0) ? v0 : 0.f;
    if (g_kl1) g_kl1[i] = on && !(SCHED && kl1[i] < p.free1) ? v1 : 0.f;
  }
}

// The six entry points' launchers: `sched` picks the instantiation (and asks for what only it reads), `what` is the entry's name.
static bool elbo_args_ok(const char* what, bool sched, const MtrssmElboSchedule& p, const float* live, const float* count) {
  if ((live == nullptr) != (count == nullptr)) { set_error("%s: live and count come together (both null: every step is live)", what); return false; }
  if (sched && (!(p.warmup >= 0.f) || !(p.warmup < 16777216.f))) { set_error("%s: warmup must lie in [0, 2^24), got %g", what, (double)p.warmup); return false; }
  return true;
}
static int elbo_fwd(const char* what, bool sched, const float* nll_a, const float* nll_v, const float* kl0, const float* kl1, const float* live,
                    const float* count, const float* step, int64_t n, MtrssmElboSchedule p, float* o_recon, float* o_k0, float* o_k1,
                    float* o_loss, float* o_beta, float* o_stats, hipStream_t s) {
  if (!nll_a || !nll_v || !kl0 || !o_recon || !o_k0 || !o_loss || (sched && (!o_beta || !o_stats)) || n <= 0) {
    set_error("%s: bad argument", what);
    return MTRSSM_EINVAL;
  }
  if (!elbo_args_ok(what, sched, p, live, count)) return MTRSSM_EINVAL;
  if (sched && p.warmup > 0.f && !step) { set_error("%s: a warm-up of %g steps needs the device scalar step (null)", what, (double)p.warmup); return MTRSSM_EINVAL; }
  set_last_kernel(sched ? "mtrssm::elbo_fwd_kernel<scheduled>" : "mtrssm::elbo_fwd_kernel<unscheduled>");
  hipLaunchKernelGGL(sched ? elbo_fwd_kernel<true> : elbo_fwd_kernel<false>, dim3(1), dim3(kThreads), 0, s, nll_a, nll_v, kl0, kl1, live, count,
                     step, n, p, o_recon, o_k0, o_k1, o_loss, o_beta, o_stats);
  return check_launch(what);
}
static int elbo_bwd(const char* what, bool sched, const float* g_recon, const float* g_k0, const float* g_k1, const float* g_loss, const float* kl0,
                    const float* kl1, const float* live, const float* count, const float* beta, int64_t n, MtrssmElboSchedule p,
                    float* g_nll_a, float* g_nll_v, float* g_kl0, float* g_kl1, hipStream_t s) {
  if (!g_nll_a || !g_nll_v || !g_kl0 || (sched && (!kl0 || !beta || (g_kl1 && !kl1))) || n <= 0) { set_error("%s: bad argument", what); return MTRSSM_EINVAL; }
  if (!elbo_args_ok(what, sched, p, live, count)) return MTRSSM_EINVAL;
  set_last_kernel(sched ? "mtrssm::elbo_bwd_kernel<scheduled>" : "mtrssm::elbo_bwd_kernel<unscheduled>");
  hipLaunchKernelGGL(sched ? elbo_bwd_kernel<true> : elbo_bwd_kernel<false>, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                     g_recon, g_k0, g_k1, g_loss, kl0, kl1, live, count, beta, n, p, g_nll_a, g_nll_v, g_kl0, g_kl1);
  return check_launch(what);
}

int elbo_combine_fwd_launch(const float* nll_a, const float* nll_v, const float* kl0, const float* kl1, int64_t n, float c0, float c1,
                            float* o_recon, float* o_k0, float* o_k1, float* o_loss, hipStream_t s) {
  return elbo_fwd("elbo_combine_fwd", false, nll_a, nll_v, kl0, kl1, nullptr, nullptr, nullptr, n, MtrssmElboSchedule{c0, c1}, o_recon, o_k0, o_k1,
                  o_loss, nullptr, nullptr, s);
}
int elbo_combine_bwd_launch(const float* g_recon, const float* g_k0, const float* g_k1, const float* g_loss, int64_t n, float c0, float c1,
                            float* g_nll_a, float* g_nll_v, float* g_kl0, float* g_kl1, hipStream_t s) {
  return elbo_bwd("elbo_combine_bwd", false, g_recon, g_k0, g_k1, g_loss, nullptr, nullptr, nullptr, nullptr, nullptr, n, MtrssmElboSchedule{c0, c1},
                  g_nll_a, g_nll_v, g_kl0, g_kl1, s);
}
int elbo_combine_counted_fwd_launch(const float* nll_a, const float* nll_v, const float* kl0, const float* kl1, const float* live,
                                    const float* count, int64_t n, float c0, float c1, float* o_recon, float* o_k0, float* o_k1, float* o_loss,
                                    hipStream_t s) {
  if (!live || !count) { set_error("elbo_combine_counted_fwd: bad argument"); return MTRSSM_EINVAL; }
  return elbo_fwd("elbo_combine_counted_fwd", false, nll_a, nll_v, kl0, kl1, live, count, nullptr, n, MtrssmElboSchedule{c0, c1}, o_recon, o_k0,
                  o_k1, o_loss, nullptr, nullptr, s);
}
int elbo_combine_counted_bwd_launch(const float* g_recon, const float* g_k0, const float* g_k1, const float* g_loss, const float* live,
                                    const float* count, int64_t n, float c0, float c1, float* g_nll_a, float* g_nll_v, float* g_kl0, float* g_kl1,
                                    hipStream_t s) {
  if (!live || !count) { set_error("elbo_combine_counted_bwd: bad argument"); return MTRSSM_EINVAL; }
  return elbo_bwd("elbo_combine_counted_bwd", false, g_recon, g_k0, g_k1, g_loss, nullptr, nullptr, live, count, nullptr, n,
                  MtrssmElboSchedule{c0, c1}, g_nll_a, g_nll_v, g_kl0, g_kl1, s);
}
int elbo_schedule_fwd_launch(const float* nll_a, const float* nll_v, const float* kl0, const float* kl1, const float* live, const float* count,
                             const float* step, int64_t n, MtrssmElboSchedule p, float* o_recon, float* o_k0, float* o_k1, float* o_loss,
                             float* o_beta, float* o_stats, hipStream_t s) {
  return elbo_fwd("elbo_schedule_fwd", true, nll_a, nll_v, kl0, kl1, live, count, step, n, p, o_recon, o_k0, o_k1, o_loss, o_beta, o_stats, s);
}
int elbo_schedule_bwd_launch(const float* g_recon, const float* g_k0, const float* g_k1, const float* g_loss, const float* kl0, const float* kl1,
                             const float* live, const float* count, const float* beta, int64_t n, MtrssmElboSchedule p, float* g_nll_a,
                             float* g_nll_v, float* g_kl0, float* g_kl1, hipStream_t s) {
  return elbo_bwd("elbo_schedule_bwd", true, g_recon, g_k0, g_k1, g_loss, kl0, kl1, live, count, beta, n, p, g_nll_a, g_nll_v, g_kl0, g_kl1, s);
}

int nll_fwd_launch(const float* pred, const float* target, int64_t frames, int64_t event, int act, float* out, hipStream_t s) {
  if (!pred || !target || !out || frames <= 0 || event <= 0) { set_error("gaussian_nll_fwd: bad argument"); return MTRSSM_EINVAL; }
  if (act != MTRSSM_ACT_IDENTITY && act != MTRSSM_ACT_TANH) { set_error("gaussian_nll: the fused output activation is Identity or Tanh (got %d)", act); return MTRSSM_EINVAL; }
  if (((uintptr_t)pred | (uintptr_t)target) & 15) { set_error("gaussian_nll_fwd: pred/target must be 16-byte aligned"); return MTRSSM_EINVAL; }
  if (int rc = clear_async(out, sizeof(float), s)) return rc;
  const int64_t n = frames * event;
  const float constant = 0.5f * 1.8378770664093453f * (float)event;  // 0.5 log(2 pi) per element
  const int sum_grid = grid_for(n / 4) < 512 ? grid_for(n / 4) : 512;
  set_last_kernel("mtrssm::nll_fwd_kernel");
  if (act == MTRSSM_ACT_TANH)
    hipLaunchKernelGGL(nll_fwd_kernel<true>, dim3(sum_grid), dim3(kThreads), 0, s, pred, target, n, 1.f / (float)frames, constant, out);
  else
    hipLaunchKernelGGL(nll_fwd_kernel<false>, dim3(sum_grid), dim3(kThreads), 0, s, pred, target, n, 1.f / (float)frames, constant, out);
  return check_launch("gaussian_nll_fwd");
}

int nll_bwd_launch(const float* pred, const float* target, const float* g_out, int64_t frames, int64_t event, int act, float* g_pred, hipStream_t s) {
  if (!pred || !target || !g_out || !g_pred || frames <= 0 || event <= 0) { set_error("gaussian_nll_bwd: bad argument"); return MTRSSM_EINVAL; }
  if (act != MTRSSM_ACT_IDENTITY && act != MTRSSM_ACT_TANH) { set_error("gaussian_nll: the fused output activation is Identity or Tanh (got %d)", act); return MTRSSM_EINVAL; }
  if (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)g_pred) & 15) { set_error("gaussian_nll_bwd: buffers must be 16-byte aligned"); return MTRSSM_EINVAL; }
  const int64_t n = frames * event;
  set_last_kernel("mtrssm::nll_bwd_kernel");
  if (act == MTRSSM_ACT_TANH)
    hipLaunchKernelGGL(nll_bwd_kernel<true>, dim3(grid_for(n / 4)), dim3(kThreads), 0, s, pred, target, g_out, n, 1.f / (float)frames, g_pred);
  else
    hipLaunchKernelGGL(nll_bwd_kernel<false>, dim3(grid_for(n / 4)), dim3(kThreads), 0, s, pred, target, g_out, n, 1.f / (float)frames, g_pred);
  return check_launch("gaussian_nll_bwd");
}

int nll_masked_fwd_launch(const float* pred, const float* target, const float* present, const float* count, int64_t frames,
                          int64_t event, int act, float* out, hipStream_t s) {
  if (!pred || !target || !present || !count || !out || frames <= 0 || event <= 0) {
    set_error("gaussian_nll_masked_fwd: bad argument");
    return MTRSSM_EINVAL;
  }
  if (act != MTRSSM_ACT_IDENTITY && act != MTRSSM_ACT_TANH) { set_error("gaussian_nll: the fused output activation is Identity or Tanh (got %d)", act); return MTRSSM_EINVAL; }
  if (((uintptr_t)pred | (uintptr_t)target) & 15) { set_error("gaussian_nll_masked_fwd: pred/target must be 16-byte aligned"); return MTRSSM_EINVAL; }
  const int64_t n = frames * event;
  if (n >= (int64_t)1 << 31) {
    set_error("gaussian_nll_masked_fwd: %lld elements (the frame index is 32-bit: < 2^31)", (long long)n);
    return MTRSSM_EINVAL;
  }
  if (int rc = clear_async(out, sizeof(float), s)) return rc;
  const float constant = 0.5f * 1.8378770664093453f * (float)event;  // as nll_fwd_launch
  const int sum_grid = grid_for(n / 4) < 512 ? grid_for(n / 4) : 512;
  const bool ev4 = event % 4 == 0, tanh = act == MTRSSM_ACT_TANH;
  set_last_kernel("mtrssm::nll_masked_fwd_kernel");
#define MTRSSM_NLLM_FWD(TV, EV) hipLaunchKernelGGL((nll_masked_fwd_kernel<TV, EV>), dim3(sum_grid), dim3(kThreads), 0, s, pred, target, present, count, n, event, constant, out)
  if (tanh) { if (ev4) MTRSSM_NLLM_FWD(true, true); else MTRSSM_NLLM_FWD(true, false); }
  else { if (ev4) MTRSSM_NLLM_FWD(false, true); else MTRSSM_NLLM_FWD(false, false); }
#undef MTRSSM_NLLM_FWD
  return check_launch("gaussian_nll_masked_fwd");
}

int nll_masked_bwd_launch(const float* pred, const float* target, const float* present, const float* count, const float* g_out,
                          int64_t frames, int64_t event, int act, float* g_pred, hipStream_t s) {
  if (!pred || !target || !present || !count || !g_out || !g_pred || frames <= 0 || event <= 0) {
    set_error("gaussian_nll_masked_bwd: bad argument");
    return MTRSSM_EINVAL;
  }
  if (act != MTRSSM_ACT_IDENTITY && act != MTRSSM_ACT_TANH) { set_error("gaussian_nll: the fused output activation is Identity or Tanh (got %d)", act); return MTRSSM_EINVAL; }
  if (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)g_pred) & 15) { set_error("gaussian_nll_masked_bwd: buffers must be 16-byte aligned"); return MTRSSM_EINVAL; }
  const int64_t n = frames * event;
  if (n >= (int64_t)1 << 31) {
    set_error("gaussian_nll_masked_bwd: %lld elements (the frame index is 32-bit: < 2^31)", (long long)n);
    return MTRSSM_EINVAL;
  }
  const bool ev4 = event % 4 == 0, tanh = act == MTRSSM_ACT_TANH;
  set_last_kernel("mtrssm::nll_masked_bwd_kernel");
#define MTRSSM_NLLM_BWD(TV, EV) hipLaunchKernelGGL((nll_masked_bwd_kernel<TV, EV>), dim3(grid_for(n / 4)), dim3(kThreads), 0, s, pred, target, present, count, g_out, n, event, g_pred)
  if (tanh) { if (ev4) MTRSSM_NLLM_BWD(true, true); else MTRSSM_NLLM_BWD(true, false); }
  else { if (ev4) MTRSSM_NLLM_BWD(false, true); else MTRSSM_NLLM_BWD(false, false); }
#undef MTRSSM_NLLM_BWD
  return check_launch("gaussian_nll_masked_bwd");
}

// ------------------------------------------------------------------------------------------------
// Step masks: uniforms, lengths and contexts -> everything a masked train step reads, no host involvement.  ONE kernel, three KINDs.
// Every (b, t) of the GLOBAL batch is visited (grid-stride); the rank's rows [row0, row0 + b_local) are written out, all rows are
// counted: wave shuffle + LDS reduction, then ONE vector atomic per workgroup and count.  The counts are whole numbers below
// 2^24 (checked by the launch), so the fp32 atomic sums are exact whatever order they arrive in.
// Modality dropout:
//   present_m(b, t) = u[b, t / span, m] >= p_m   (fp32 compare), m = 0 audio, 1 vision;
//   at t = 0 only, a row with neither present gets the modality with the larger u (tie: audio).
// kMaskDropout: that rule alone; codes, the two present planes, mask0; counts = {audio, vision}.
// kMaskRagged: row b of the global batch has valid[b] live steps (clamped into [0, T] here), step (b, t) is
//   live iff t < valid[b].  A modality is present iff the step is live AND (no dropout -- u == nullptr -- or the dropout rule says
//   so, its t = 0 fix-up applied BEFORE the AND).  Beside the dropout outputs: the `live` plane the counted ELBO epilogue reads,
//   last[r] = valid - 1 (-1: an empty row) for the carry's save, and a third count, the live steps.
// kMaskForecast: row b observes a context of c_b = lo + min(int(u_context[b] * float(n)), n - 1) frames,
//   n = hi - lo + 1 (ONE fp32 multiply, truncated), and runs open loop after it.  live as above (valid == nullptr: T), observed =
//   live AND t < c_b; a modality is SEEN iff the step is observed AND (no dropout or the dropout rule says present, fix-up BEFORE
//   the AND).  What is seen (codes, plane_a / plane_v, mask0) and what is reconstructed (plane_live, the target) are different
//   planes here; plane_obs is the KL's plane.  counts = {live, observed}.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dropout_present(const float* __restrict__ u, long b, int t, int span, int S, float p_audio, float p_vision,
                                                bool& a, bool& v) {
  const float2 uu = reinterpret_cast<const float2*>(u)[b * S + t / span];
  a = uu.x >= p_audio;
  v = uu.y >= p_vision;
  if (t == 0 && !a && !v) {
    a = uu.x >= uu.y;
    v = !a;
  }
}

enum { kMaskDropout, kMaskRagged, kMaskForecast };

template <int KIND>
__global__ __launch_bounds__(kThreads) void step_mask_kernel(
    const int* __restrict__ valid, const float* __restrict__ u, const float* __restrict__ u_context, float p_audio, float p_vision, int span,
    int T, int S, int lo, int n_bins, long b_global, long row0, long b_local, int* __restrict__ codes, float* __restrict__ plane_a,
    float* __restrict__ plane_v, float* __restrict__ plane_live, float* __restrict__ plane_obs, unsigned char* __restrict__ mask0,
    int* __restrict__ last, float* __restrict__ counts) {
  constexpr int NC = KIND == kMaskRagged ? 3 : 2;
  __shared__ float red[NC][kThreads / kWave];
  const long total = b_global * T;
  float cnt[NC] = {};
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / T;
    const int t = (int)(i - b * T);
    int n = T;
    if (KIND == kMaskRagged || (KIND == kMaskForecast && valid)) n = valid[b];
    n = n < 0 ? 0 : (n > T ? T : n);
    const bool on = KIND == kMaskDropout || t < n;
    bool obs = on;
    if constexpr (KIND == kMaskForecast) {
      const long long bin = (long long)(u_context[b] * (float)n_bins);  // (64-bit, then clamped: above 2^24 (float)n_bins may round up, to as much as 2^31)
      obs = on && t < lo + (int)(bin < n_bins - 1 ? bin : n_bins - 1);
    }
    bool a = true, v = true;
    if (KIND == kMaskDropout || u) dropout_present(u, b, t, span, S, p_audio, p_vision, a, v);
    a = a && obs;
    v = v && obs;
    if constexpr (KIND == kMaskForecast) {
      cnt[0] += on ? 1.f : 0.f;
      cnt[1] += obs ? 1.f : 0.f;
    } else {
      cnt[0] += a ? 1.f : 0.f;
      cnt[1] += v ? 1.f : 0.f;
      if constexpr (KIND == kMaskRagged) cnt[2] += on ? 1.f : 0.f;
    }
    const long r = b - row0;
    if (r >= 0 && r < b_local) {
      const long o = r * T + t;
      codes[o] = (a ? 1 : 0) | (v ? 2 : 0);
      plane_a[o] = a ? 1.f : 0.f;
      plane_v[o] = v ? 1.f : 0.f;
      if constexpr (KIND != kMaskDropout) plane_live[o] = on ? 1.f : 0.f;
      if constexpr (KIND == kMaskForecast) plane_obs[o] = obs ? 1.f : 0.f;
      if (t == 0) {
        mask0[2 * r] = a ? 1 : 0;
        mask0[2 * r + 1] = v ? 1 : 0;
        if constexpr (KIND != kMaskDropout) last[r] = n - 1;
      }
    }
  }
  float tot[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) tot[k] = block_sum(cnt[k], red[k]);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NC; ++k) atomicAdd(counts + k, tot[k]);
  }
}

// The three entry points' shared checks and launch; `what` is the entry's name, the caller has checked its own pointers.
static int step_mask_launch(const char* what, int kind, const int32_t* valid, const float* u, const float* u_context, int64_t b_global, int64_t T,
                            int64_t span, float p_audio, float p_vision, int64_t lo, int64_t hi, int64_t row0, int64_t b_local, int32_t* codes,
                            float* plane_a, float* plane_v, float* plane_live, float* plane_obs, unsigned char* mask0, int32_t* last,
                            float* counts, hipStream_t s) {
  if (b_global <= 0 || T <= 0 || span <= 0 || b_local <= 0 || row0 < 0 || row0 + b_local > b_global) {
    set_error("%s: need B_global, T, span, B_local > 0 and 0 <= row0 <= B_global - B_local (got %lld %lld %lld %lld %lld)", what,
              (long long)b_global, (long long)T, (long long)span, (long long)b_local, (long long)row0);
    return MTRSSM_EINVAL;
  }
  if (kind == kMaskForecast && (lo < 1 || hi < lo || hi >= (int64_t)1 << 31)) {
    set_error("%s: need 1 <= lo <= hi < 2^31 (got %lld, %lld)", what, (long long)lo, (long long)hi);
    return MTRSSM_EINVAL;
  }
  if (u && (!(p_audio >= 0.f && p_audio < 1.f) || !(p_vision >= 0.f && p_vision < 1.f))) {
    set_error("%s: probabilities must be in [0, 1) (got %g, %g)", what, (double)p_audio, (double)p_vision);
    return MTRSSM_EINVAL;
  }
  if (b_global * T >= (int64_t)1 << 24) {
    set_error("%s: %lld frames (the fp32 counts are exact below 2^24)", what, (long long)(b_global * T));
    return MTRSSM_EINVAL;
  }
  if (span >= (int64_t)1 << 31) { set_error("%s: span %lld does not fit 31 bits", what, (long long)span); return MTRSSM_EINVAL; }
  if (((uintptr_t)u & 7) || (((uintptr_t)valid | (uintptr_t)u_context) & 3)) {
    set_error("%s: the mask uniforms must be 8-byte, valid and u_context 4-byte aligned", what);
    return MTRSSM_EINVAL;
  }
  if (int rc = clear_async(counts, (kind == kMaskRagged ? 3 : 2) * sizeof(float), s)) return rc;
  const int grid = grid_for(b_global * T) < 64 ? grid_for(b_global * T) : 64;
  const auto kernel = kind == kMaskDropout ? step_mask_kernel<kMaskDropout> : kind == kMaskRagged ? step_mask_kernel<kMaskRagged> : step_mask_kernel<kMaskForecast>;
  set_last_kernel(kind == kMaskDropout ? "mtrssm::step_mask_kernel<dropout>" : kind == kMaskRagged ? "mtrssm::step_mask_kernel<ragged>" : "mtrssm::step_mask_kernel<forecast>");
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), 0, s, reinterpret_cast<const int*>(valid), u, u_context, p_audio, p_vision, (int)span,
                     (int)T, (int)((T + span - 1) / span), (int)lo, (int)(hi - lo + 1), (long)b_global, (long)row0, (long)b_local,
                     reinterpret_cast<int*>(codes), plane_a, plane_v, plane_live, plane_obs, mask0, reinterpret_cast<int*>(last), counts);
  return check_launch(what);
}

int modality_dropout_launch(const float* u, int64_t b_global, int64_t T, int64_t span, float p_audio, float p_vision, int64_t row0,
                            int64_t b_local, int32_t* codes, float* present_audio, float* present_vision, unsigned char* mask0,
                            float* counts, hipStream_t s) {
  if (!u || !codes || !present_audio || !present_vision || !mask0 || !counts) { set_error("modality_dropout: null pointer"); return MTRSSM_EINVAL; }
  return step_mask_launch("modality_dropout", kMaskDropout, nullptr, u, nullptr, b_global, T, span, p_audio, p_vision, 1, 1, row0, b_local, codes,
                          present_audio, present_vision, nullptr, nullptr, mask0, nullptr, counts, s);
}

int step_mask_ragged_launch(const int32_t* valid, const float* u, int64_t b_global, int64_t T, int64_t span, float p_audio, float p_vision,
                            int64_t row0, int64_t b_local, int32_t* codes, float* present_audio, float* present_vision, float* live,
                            unsigned char* mask0, int32_t* last, float* counts, hipStream_t s) {
  if (!valid || !codes || !present_audio || !present_vision || !live || !mask0 || !last || !counts) {
    set_error("step_mask_ragged: null pointer");
    return MTRSSM_EINVAL;
  }
  return step_mask_launch("step_mask_ragged", kMaskRagged, valid, u, nullptr, b_global, T, span, p_audio, p_vision, 1, 1, row0, b_local, codes,
                          present_audio, present_vision, live, nullptr, mask0, last, counts, s);
}

int step_mask_forecast_launch(const int32_t* valid, const float* u_mask, const float* u_context, int64_t b_global, int64_t T, int64_t span,
                              float p_audio, float p_vision, int64_t lo, int64_t hi, int64_t row0, int64_t b_local, int32_t* codes,
                              float* seen_audio, float* seen_vision, float* target, float* observed, unsigned char* mask0, int32_t* last,
                              float* counts, hipStream_t s) {
  if (!u_context || !codes || !seen_audio || !seen_vision || !target || !observed || !mask0 || !last || !counts) {
    set_error("step_mask_forecast: null pointer");
    return MTRSSM_EINVAL;
  }
  return step_mask_launch("step_mask_forecast", kMaskForecast, valid, u_mask, u_context, b_global, T, span, p_audio, p_vision, lo, hi, row0, b_local,
                          codes, seen_audio, seen_vision, target, observed, mask0, last, counts, s);
}

int sumsq_launch(const float* x, int64_t n, float* out, hipStream_t s) {
  if (!x || !out || n <= 0) { set_error("sumsq: bad argument"); return MTRSSM_EINVAL; }
  if ((uintptr_t)x & 15) { set_error("sumsq: x must be 16-byte aligned"); return MTRSSM_EINVAL; }
  if (int rc = clear_async(out, sizeof(float), s)) return rc;
  set_last_kernel("mtrssm::sumsq_kernel");
  hipLaunchKernelGGL(sumsq_kernel, dim3(grid_for(n / 4) < 512 ? grid_for(n / 4) : 512), dim3(kThreads), 0, s, x, n, out);  // one same-address atomic per workgroup
  return check_launch("sumsq");
}

int adamw_launch(float* p, const float* g, float* m, float* v, int64_t n, const float* sumsq, float clip, float gscale,
                 float lr, float b1, float b2, float eps, float wd, int step, hipStream_t s) {
  if (!p || !g || !m || !v || n <= 0 || step <= 0) { set_error("adamw_step: bad argument"); return MTRSSM_EINVAL; }
  const float bc1 = 1.f - powf(b1, (float)step);
  const float bc2_sqrt = sqrtf(1.f - powf(b2, (float)step));
  set_last_kernel("mtrssm::adamw_kernel");
  hipLaunchKernelGGL(adamw_kernel, dim3(grid_for(n)), dim3(kThreads), 0, s, p, g, m, v, n, sumsq, clip, gscale, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
  return check_launch("adamw_step");
}

int adamw_prepare_launch(const float* g, int64_t n, float* sumsq, float* state, const int* status, float b1, float b2, hipStream_t s) {
  if (!g || !sumsq || !state || n <= 0) { set_error("adamw_prepare: bad argument"); return MTRSSM_EINVAL; }
  if ((uintptr_t)g & 15) { set_error("adamw_prepare: grad must be 16-byte aligned"); return MTRSSM_EINVAL; }
  if (int rc = clear_async(sumsq, sizeof(float), s)) return rc;
  set_last_kernel("mtrssm::sumsq_tick_kernel");
  hipLaunchKernelGGL(sumsq_tick_kernel, dim3(grid_for(n / 4) < 512 ? grid_for(n / 4) : 512), dim3(kThreads), 0, s, g, n, sumsq, state, status, b1, b2);  // (as sumsq)
  return check_launch("adamw_prepare");
}

int adamw_apply_launch(float* p, const float* g, float* m, float* v, const unsigned char* active, int64_t n, const float* sumsq,
                       const float* state, const int* status, float clip, float gscale, float b1, float b2, float eps, float wd, hipStream_t s) {
  if (!p || !g || !m || !v || !state || n <= 0) { set_error("adamw_apply: bad argument"); return MTRSSM_EINVAL; }
  set_last_kernel("mtrssm::adamw_masked_kernel");
  hipLaunchKernelGGL(adamw_masked_kernel, dim3(grid_for(n)), dim3(kThreads), 0, s, p, g, m, v, active, n, sumsq, state, status, clip, gscale,
                     b1, b2, eps, wd);
  return check_launch("adamw_apply");
}

// ------------------------------------------------------------------------------------------------
// Conv weight gradients, end of backward: every conv weight gradient of the step was accumulated (fp32 atomics, 128-byte
// coalesced) in the kernels' packed layout [OPad][taps][IPad]; ONE launch adds them all into the flat gradient buffer in
// the parameter layout [O][I][KH][KW] and clears the packed buffers for the next step.  Replaces one strided torch add
// (AccumulateGrad) and one zero fill per conv weight (~80 of each per MoPoE-MRSSM train step).
// table: `count` rows of 8 int64 = { packed*, grad*, O, I, taps, IPad, 0, 0 }.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void unpack_conv_grads_kernel(const long* __restrict__ table) {
  const long* row = table + (long)blockIdx.y * 8;
  float* packed = reinterpret_cast<float*>(row[0]);
  float* grad = reinterpret_cast<float*>(row[1]);
  const long O = row[2], I = row[3], taps = row[4], ipad = row[5];
  const long total = O * taps * ipad;  // rows o >= O of the padded buffer are never written by the kernels
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long i = e % ipad, ot = e / ipad, tap = ot % taps, o = ot / taps;
    const float v = packed[e];
    if (v != 0.f) packed[e] = 0.f;
    if (i < I) grad[(o * I + i) * taps + tap] += v;
  }
}

int unpack_conv_grads_launch(const int64_t* table, int count, int blocks_per_entry, hipStream_t s) {
  if (!table || count <= 0 || blocks_per_entry <= 0) { set_error("unpack_conv_grads: bad argument"); return MTRSSM_EINVAL; }
  static_assert(sizeof(long) == sizeof(int64_t), "descriptor words are 64-bit");
  set_last_kernel("mtrssm::unpack_conv_grads_kernel");
  hipLaunchKernelGGL(unpack_conv_grads_kernel, dim3(blocks_per_entry, count), dim3(kThreads), 0, s, reinterpret_cast<const long*>(table));
  return check_launch("unpack_conv_grads");
}

// ------------------------------------------------------------------------------------------------
// Episode feed: one [B, T, E] input / target pair from the HBM-resident episode store.
//   target[b, t, :] = store[idx[b], t, :]            (TakeFirstN: t < T <= Tfull, transform.py:31-52)
//   input [b, t, :] = target + noise[b, t, :] * std  (GaussianNoise, transform.py:55-72: two roundings, mul then add)
// Replaces EpisodeDataset.__getitem__ + default collate of the 6-tuple StackDataset (dataset.py:84-112,
// mrssm/dataset.py:155-183).  One float4 per thread; rows are E floats, E % 4 == 0.  ONE kernel, three MODEs:
// kGatherFirst: the first T frames, as above.
// kGatherWindow: a WINDOW of each episode, target[b, t, :] = store[idx[b], start[b] + t, :].  start[b] is read on the device (a
//   replayed graph takes new windows without a host round trip), so the launcher cannot range-check it: the kernel clamps it into
//   [0, Tfull - T] and the host validates the starts where it makes them (dataset.py).  A start shifts a row by whole frames of E
//   floats, E % 4 == 0: every access stays a 16-byte one.  (Neither of these two modes clamps idx[b].)
// kGatherRagged: the window gather for episodes of different lengths: frame start[b] + t of episode idx[b] is
//   LIVE iff it lies before lengths[idx[b]]; a dead frame is exactly 0 in target and input (no noise added) and issues no load and
//   no generator work.  start[b] is clamped into [0, Tfull] (a chunk may hang over the end of the store: the length test keeps
//   every read inside it), lengths into [0, Tfull], idx[b] into [0, n_episodes).  valid_out[b] (optional) = clamp(length - start,
//   0, T), the row's live steps.
// The noise is the `noise` plane (null: input = target), or with SEEDED the generator below.
// ------------------------------------------------------------------------------------------------
// SEEDED: the standard normals are made in the kernel: the noise of a frame is a pure
// function of (key, epoch, episode, absolute frame, element), never stored, whatever row of whatever batch the frame lands in.
//   x[0..3] = Philox4x32-10(counter = (e4, frame, low 32 bits of episode, epoch), key = (key0, key1))
//   two Box-Muller pairs, (x0, x1) -> elements 4 e4 + 0, 1 and (x2, x3) -> elements 4 e4 + 2, 3:
//     u1 = ((xa >> 8) + 1) * 2^-24 in (0, 1], u2 = (xb >> 8) * 2^-24 in [0, 1), r = sqrtf(-2 logf(u1)), z = r cos(2 pi u2), r sin(2 pi u2)
// Philox as Salmon et al. (SC'11) define it: per round (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1,
// lo(M0 c0)), the key advancing by the Weyl constants between rounds.
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&out)[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

__device__ __forceinline__ void box_muller(unsigned xa, unsigned xb, float& z0, float& z1) {
#pragma clang fp contract(off)
  const float u1 = (float)((xa >> 8) + 1u) * 0x1p-24f;  // (0, 1]: 24-bit integers, exact in fp32
  const float u2 = (float)(xb >> 8) * 0x1p-24f;         // [0, 1)
  const float r = sqrtf(-2.f * logf(u1));
  float sn, cs;
  sincospif(2.f * u2, &sn, &cs);  // (2 u2 is exact: the argument reduction sees the 24-bit fraction itself)
  z0 = r * cs;
  z1 = r * sn;
}

enum { kGatherFirst, kGatherWindow, kGatherRagged };

template <int MODE, bool SEEDED>
__global__ __launch_bounds__(kThreads) void episode_gather_kernel(
    const float* __restrict__ store, const long* __restrict__ idx, const int* __restrict__ start, const int* __restrict__ lengths,
    const float* __restrict__ noise, unsigned key0, unsigned key1, unsigned epoch, long n_episodes, long B, long T, long Tfull, long E4,
    float std_, float* __restrict__ input, float* __restrict__ target, int* __restrict__ valid_out) {
#pragma clang fp contract(off)  // mul then add, each rounded (torch's `data + randn * std`): hipcc would contract to v_pk_fma_f32
  const long per_b = T * E4;
  const long total = B * per_b;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / per_b, r = i - b * per_b;  // r = t * E4 + e4
    long t = 0;
    if constexpr (MODE == kGatherRagged || SEEDED) t = r / E4;
    long ep = idx[b], s = 0;
    bool on = true;
    if constexpr (MODE == kGatherWindow) {
      const long last = Tfull - T;
      s = start[b];
      s = s < 0 ? 0 : (s > last ? last : s);
    }
    if constexpr (MODE == kGatherRagged) {
      s = start[b];
      s = s < 0 ? 0 : (s > Tfull ? Tfull : s);
      ep = ep < 0 ? 0 : (ep >= n_episodes ? n_episodes - 1 : ep);
      long len = lengths[ep];
      len = len < 0 ? 0 : (len > Tfull ? Tfull : len);
      on = s + t < len;  // (< Tfull: the read below stays inside the episode)
      if (valid_out && r == 0) {
        const long n = len - s;
        valid_out[b] = (int)(n < 0 ? 0 : (n > T ? T : n));
      }
    }
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on) x = reinterpret_cast<const float4*>(store)[(ep * Tfull + s) * E4 + r];
    if (target) reinterpret_cast<float4*>(target)[i] = x;
    if (input) {
      float4 y = x;
      if (on && (SEEDED || noise)) {
        float4 n;
        if constexpr (SEEDED) {
          unsigned w[4];
          philox4x32_10((unsigned)(r - t * E4), (unsigned)(s + t), (unsigned)ep, epoch, key0, key1, w);
          box_muller(w[0], w[1], n.x, n.y);
          box_muller(w[2], w[3], n.z, n.w);
        } else {
          n = reinterpret_cast<const float4*>(noise)[i];
        }
        const float px = n.x * std_, py = n.y * std_, pz = n.z * std_, pw = n.w * std_;  // plain expressions: the pragma
        y.x = x.x + px;                                                                  // above does not reach into the
        y.y = x.y + py;                                                                  // headers' __fmul_rn / __fadd_rn
        y.z = x.z + pz;
        y.w = x.w + pw;
      }
      reinterpret_cast<float4*>(input)[i] = y;
    }
  }
}

// The four entry points' shared checks and launch; `what` is the entry's name, the caller has checked which of start / lengths /
// valid_out it needs.  lengths given: ragged; else start given: windows; else the first T frames.
static int episode_gather(const char* what, bool seeded, const float* store, const int64_t* idx, const int32_t* start, const int32_t* lengths,
                          const float* noise, uint32_t key0, uint32_t key1, uint32_t epoch, int64_t n_episodes, int64_t B, int64_t T,
                          int64_t Tfull, int64_t E, float std_, float* input, float* target, int32_t* valid_out, hipStream_t s) {
  if (!store || !idx || (!input && !target) || n_episodes <= 0 || B <= 0 || T <= 0 || Tfull < T || E <= 0) {
    set_error("%s: bad argument (need 0 < T <= Tfull, B, E > 0, an output)", what);
    return MTRSSM_EINVAL;
  }
  if (E % 4) { set_error("%s: the event size %ld must be a multiple of 4 floats", what, (long)E); return MTRSSM_EINVAL; }
  if (seeded && E / 4 > 0xffffffffL) { set_error("%s: the event size %ld exceeds the 32-bit element counter", what, (long)E); return MTRSSM_EINVAL; }
  if (((uintptr_t)store | (uintptr_t)noise | (uintptr_t)input | (uintptr_t)target) & 15) {
    set_error("%s: buffers must be 16-byte aligned", what);
    return MTRSSM_EINVAL;
  }
  if (((uintptr_t)start | (uintptr_t)lengths | (uintptr_t)valid_out) & 3) {
    set_error("%s: start, lengths and valid_out must be 4-byte aligned", what);
    return MTRSSM_EINVAL;
  }
  const int mode = lengths ? kGatherRagged : (start ? kGatherWindow : kGatherFirst);
  static const struct {
    decltype(&episode_gather_kernel<kGatherFirst, false>) kernel;
    const char* name;
  } table[2][3] = {{{episode_gather_kernel<kGatherFirst, false>, "mtrssm::episode_gather_kernel<first>"},
                    {episode_gather_kernel<kGatherWindow, false>, "mtrssm::episode_gather_kernel<window>"},
                    {episode_gather_kernel<kGatherRagged, false>, "mtrssm::episode_gather_kernel<ragged>"}},
                   {{episode_gather_kernel<kGatherFirst, true>, "mtrssm::episode_gather_kernel<first, seeded>"},
                    {episode_gather_kernel<kGatherWindow, true>, "mtrssm::episode_gather_kernel<window, seeded>"},
                    {episode_gather_kernel<kGatherRagged, true>, "mtrssm::episode_gather_kernel<ragged, seeded>"}}};
  set_last_kernel(table[seeded][mode].name);
  hipLaunchKernelGGL(table[seeded][mode].kernel, dim3(grid_for(B * T * E / 4)), dim3(kThreads), 0, s, store, reinterpret_cast<const long*>(idx),
                     reinterpret_cast<const int*>(start), reinterpret_cast<const int*>(lengths), noise, key0, key1, epoch, (long)n_episodes,
                     (long)B, (long)T, (long)Tfull, (long)(E / 4), std_, input, target, reinterpret_cast<int*>(valid_out));
  return check_launch(what);
}

int episode_gather_launch(const float* store, const int64_t* idx, const float* noise, int64_t n_episodes, int64_t B, int64_t T,
                          int64_t Tfull, int64_t E, float std_, float* input, float* target, hipStream_t s) {
  return episode_gather("episode_gather", false, store, idx, nullptr, nullptr, noise, 0, 0, 0, n_episodes, B, T, Tfull, E, std_, input, target,
                        nullptr, s);
}

int episode_gather_window_launch(const float* store, const int64_t* idx, const int32_t* start, const float* noise, int64_t n_episodes,
                                 int64_t B, int64_t T, int64_t Tfull, int64_t E, float std_, float* input, float* target, hipStream_t s) {
  if (!start) { set_error("episode_gather_window: start is null (mtrssm_episode_gather reads the first T frames)"); return MTRSSM_EINVAL; }
  return episode_gather("episode_gather_window", false, store, idx, start, nullptr, noise, 0, 0, 0, n_episodes, B, T, Tfull, E, std_, input,
                        target, nullptr, s);
}

int episode_gather_ragged_launch(const float* store, const int64_t* idx, const int32_t* start, const int32_t* lengths, const float* noise,
                                 int64_t n_episodes, int64_t B, int64_t T, int64_t Tfull, int64_t E, float std_, float* input, float* target,
                                 int32_t* valid_out, hipStream_t s) {
  if (!start || !lengths) { set_error("episode_gather_ragged: start or lengths is null"); return MTRSSM_EINVAL; }
  return episode_gather("episode_gather_ragged", false, store, idx, start, lengths, noise, 0, 0, 0, n_episodes, B, T, Tfull, E, std_, input,
                        target, valid_out, s);
}

int episode_gather_seeded_launch(const float* store, const int64_t* idx, const int32_t* start, const int32_t* lengths, int32_t* valid_out,
                                 uint32_t key0, uint32_t key1, uint32_t epoch, int64_t n_episodes, int64_t B, int64_t T, int64_t Tfull,
                                 int64_t E, float std_, float* input, float* target, hipStream_t s) {
  if (lengths && !start) { set_error("episode_gather_seeded: lengths without start (a ragged batch needs its windows' starts)"); return MTRSSM_EINVAL; }
  if (valid_out && !lengths) { set_error("episode_gather_seeded: valid_out without lengths"); return MTRSSM_EINVAL; }
  return episode_gather("episode_gather_seeded", true, store, idx, start, lengths, nullptr, key0, key1, epoch, n_episodes, B, T, Tfull, E, std_,
                        input, target, valid_out, s);
}

// ------------------------------------------------------------------------------------------------
// AUGMENTED: the seeded gather with a seeded shift and band masks (include/mtrssm.h states the rule).  The
// shift (dy, dx) and the bands (r0, h, c0, w) are uniform per (row, frame), so the work is mapped one WORKGROUP per frame
// (blockIdx.x = b * T + t; no loop over frames, which kept twice the scalar registers live): lane j <= bands of the first wave makes Philox call j (call 0: the shift, call
// 1 + j: band j) and leaves four integers in LDS, a barrier, and every lane reads them back -- 1 + bands Philox calls per frame, none
// per float4.  Lane q then walks the frame's output quads q, q + 256, ...: quad q is pixels x0 .. x0 + 3 of row y of channel c, its source
// the four floats from column x0 - dx of row y - dy of the same channel.  A source row outside [0, H) reads nothing.  Inside, the
// source quad is covered by the aligned float4s at a = floor((x0 - dx) / 4) and a + 1 of that ROW (W % 4 == 0: every row begins on 16
// bytes); each is loaded only if it lies inside the row, stands for fill otherwise, and the second only when dx % 4 != 0 (uniform per
// frame).  So no access leaves the source row, whatever dx: a vacated pixel never sees the neighbouring row, channel or frame.
// Stores are whole float4s.  MODE as in episode_gather_kernel, with its clamps; the liveness of a frame is uniform per workgroup,
// so the barrier stands in uniform control flow.
// ------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(kThreads) void episode_gather_augmented_kernel(
    MtrssmFeedAugment aug, const float* __restrict__ store, const long* __restrict__ idx, const int* __restrict__ start,
    const int* __restrict__ lengths, unsigned key0, unsigned key1, unsigned akey0, unsigned akey1, unsigned epoch, long n_episodes,
    long T, long Tfull, int C, int H, int W, int noisy, float std_, float* __restrict__ input, float* __restrict__ target,
    int* __restrict__ valid_out) {
#pragma clang fp contract(off)  // mul then add, each rounded, as episode_gather_kernel
  __shared__ int4 prm[1 + MTRSSM_AUGMENT_MAX_BANDS];  // [0]: (dy, dx, -, -); [1 + j]: (r0, h, c0, w) of band j
  const unsigned W4 = (unsigned)W >> 2, E4 = (unsigned)(C * H) * W4;
  const float4 fill4 = make_float4(aug.fill, aug.fill, aug.fill, aug.fill);
  // Quad q = (c H + y) W4 + x4.  A lane's quads are q = threadIdx.x + 256 k: divisions give the lane's first quad and the step of 256
  // quads (the step's are scalar), and the quad loop walks (c, y, x4) by additions.
  const unsigned cy_first = threadIdx.x / W4, x4_first = threadIdx.x - cy_first * W4;
  const unsigned c_first = cy_first / (unsigned)H, y_first = cy_first - c_first * (unsigned)H;
  const unsigned step_cy = kThreads / W4, step_x = kThreads - step_cy * W4;
  const unsigned step_c = step_cy / (unsigned)H, step_y = step_cy - step_c * (unsigned)H;
  {
    const long fr = blockIdx.x;  // < B * T < 2^31 (the launcher's check)
    const long b = (unsigned)fr / (unsigned)T, t = fr - b * T;
    long ep = idx[b], s = 0;
    bool on = true;
    if constexpr (MODE == kGatherWindow) {
      const long last = Tfull - T;
      s = start[b];
      s = s < 0 ? 0 : (s > last ? last : s);
    }
    if constexpr (MODE == kGatherRagged) {
      s = start[b];
      s = s < 0 ? 0 : (s > Tfull ? Tfull : s);
      ep = ep < 0 ? 0 : (ep >= n_episodes ? n_episodes - 1 : ep);
      long len = lengths[ep];
      len = len < 0 ? 0 : (len > Tfull ? Tfull : len);
      on = s + t < len;  // (< Tfull: the reads below stay inside the episode)
      if (valid_out && t == 0 && threadIdx.x == 0) {
        const long n = len - s;
        valid_out[b] = (int)(n < 0 ? 0 : (n > T ? T : n));
      }
    }
    float4* const tgt = target ? reinterpret_cast<float4*>(target) + fr * E4 : nullptr;
    float4* const inp = input ? reinterpret_cast<float4*>(input) + fr * E4 : nullptr;
    if (!on) {  // a dead frame: zeros, no load, no generator work
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
      for (unsigned q = threadIdx.x; q < E4; q += kThreads) {
        if (tgt) tgt[q] = zero;
        if (inp) inp[q] = zero;
      }
      return;
    }
    const unsigned f = (unsigned)(s + t);
    if (threadIdx.x <= (unsigned)aug.bands) {
      const unsigned j = threadIdx.x;
      unsigned w[4];
      philox4x32_10(j, (j && aug.per_frame) ? f + 1u : 0u, (unsigned)ep, epoch, akey0, akey1, w);
      int4 p = make_int4(0, 0, 0, 0);
      if (j == 0) {
        p.x = (int)__umulhi(w[0], 2u * aug.sy + 1u) - aug.sy;  // dy
        p.y = (int)__umulhi(w[1], 2u * aug.sx + 1u) - aug.sx;  // dx
      } else {
        p.y = (int)__umulhi(w[0], (unsigned)aug.max_rows + 1u);  // h
        p.x = (int)__umulhi(w[1], (unsigned)(H - p.y) + 1u);     // r0
        p.w = (int)__umulhi(w[2], (unsigned)aug.max_cols + 1u);  // w
        p.z = (int)__umulhi(w[3], (unsigned)(W - p.w) + 1u);     // c0
      }
      prm[j] = p;
    }
    __syncthreads();
    const int dy = __builtin_amdgcn_readfirstlane(prm[0].x), dx = __builtin_amdgcn_readfirstlane(prm[0].y);
    const int sh = (-dx) & 3;  // the source quad begins `sh` floats into an aligned one (two's complement: right for dx > 0 too)
    const float4* const src = reinterpret_cast<const float4*>(store) + (ep * Tfull + (long)f) * E4;
    unsigned c = c_first, y = y_first, x4 = x4_first;
    for (unsigned q = threadIdx.x; q < E4; q += kThreads) {
      const unsigned x0 = x4 * 4u;
      const int ys = (int)y - dy;
      float4 x = fill4;
      if ((unsigned)ys < (unsigned)H) {
        const float4* const row = src + (c * (unsigned)H + (unsigned)ys) * W4;
        const int a = ((int)x0 - dx) >> 2;  // floor: the aligned quad that holds source column x0 - dx
        float4 lo = fill4, hi = fill4;
        if ((unsigned)a < W4) lo = row[a];
        if (sh && (unsigned)(a + 1) < W4) hi = row[a + 1];
        x = sh == 0 ? lo : (sh == 1 ? make_float4(lo.y, lo.z, lo.w, hi.x) : (sh == 2 ? make_float4(lo.z, lo.w, hi.x, hi.y)
                                                                                     : make_float4(lo.w, hi.x, hi.y, hi.z)));
      }
      if (tgt) tgt[q] = x;
      if (inp) {
        bool m0 = false, m1 = false, m2 = false, m3 = false;
        for (int j = 1; j <= aug.bands; ++j) {  // (a uniform trip count; band j is one broadcast 16-byte LDS read)
          const int4 p = prm[j];
          const bool rowm = y - (unsigned)p.x < (unsigned)p.y;  // r0 <= y < r0 + h in one unsigned test; h = 0 never holds
          m0 |= rowm | (x0 - (unsigned)p.z < (unsigned)p.w);
          m1 |= rowm | (x0 + 1u - (unsigned)p.z < (unsigned)p.w);
          m2 |= rowm | (x0 + 2u - (unsigned)p.z < (unsigned)p.w);
          m3 |= rowm | (x0 + 3u - (unsigned)p.z < (unsigned)p.w);
        }
        float4 v = make_float4(m0 ? aug.fill : x.x, m1 ? aug.fill : x.y, m2 ? aug.fill : x.z, m3 ? aug.fill : x.w);
        if (noisy) {
          unsigned w[4];
          float4 n;
          philox4x32_10(q, f, (unsigned)ep, epoch, key0, key1, w);
          box_muller(w[0], w[1], n.x, n.y);
          box_muller(w[2], w[3], n.z, n.w);
          const float px = n.x * std_, py = n.y * std_, pz = n.z * std_, pw = n.w * std_;
          v.x = v.x + px;
          v.y = v.y + py;
          v.z = v.z + pz;
          v.w = v.w + pw;
        }
        inp[q] = v;
      }
      // the lane's next quad, 256 further on: x4 < 2 W4 and y < 2 H before the corrections, one of each is enough
      x4 += step_x;
      const unsigned carry = x4 >= W4 ? 1u : 0u;
      x4 -= carry ? W4 : 0u;
      y += step_y + carry;
      c += step_c;
      if (y >= (unsigned)H) y -= (unsigned)H, ++c;
    }
  }
}

int episode_gather_augmented_launch(const MtrssmFeedAugment* aug, const float* store, const int64_t* idx, const int32_t* start,
                                    const int32_t* lengths, int32_t* valid_out, uint32_t key0, uint32_t key1, uint32_t akey0, uint32_t akey1,
                                    uint32_t epoch, int64_t n_episodes, int64_t B, int64_t T, int64_t Tfull, int64_t C, int64_t H, int64_t W,
                                    int32_t noisy, float std_, float* input, float* target, hipStream_t s) {
  const char* what = "episode_gather_augmented";
  if (!aug) { set_error("%s: aug is null", what); return MTRSSM_EINVAL; }
  if (lengths && !start) { set_error("%s: lengths without start (a ragged batch needs its windows' starts)", what); return MTRSSM_EINVAL; }
  if (valid_out && !lengths) { set_error("%s: valid_out without lengths", what); return MTRSSM_EINVAL; }
  if (!store || !idx || (!input && !target) || n_episodes <= 0 || B <= 0 || T <= 0 || Tfull < T || C <= 0 || H <= 0 || W <= 0) {
    set_error("%s: bad argument (need 0 < T <= Tfull, B, C, H, W > 0, an output)", what);
    return MTRSSM_EINVAL;
  }
  if (W % 4) { set_error("%s: the row length W = %ld must be a multiple of 4 floats", what, (long)W); return MTRSSM_EINVAL; }
  if (C > 0x7fffffffL || H > 0x7fffffffL || W > 0x7fffffffL || C * H > 0x7fffffffL / W) {
    set_error("%s: the event %ld x %ld x %ld exceeds 2^31 - 1 floats", what, (long)C, (long)H, (long)W);
    return MTRSSM_EINVAL;
  }
  if (aug->sy < 0 || aug->sy >= H || aug->sx < 0 || aug->sx >= W) {
    set_error("%s: the shift (%d, %d) must lie in [0, H) x [0, W) = [0, %ld) x [0, %ld)", what, aug->sy, aug->sx, (long)H, (long)W);
    return MTRSSM_EINVAL;
  }
  if (aug->bands < 0 || aug->bands > MTRSSM_AUGMENT_MAX_BANDS) {
    set_error("%s: bands = %d must lie in [0, %d]", what, aug->bands, MTRSSM_AUGMENT_MAX_BANDS);
    return MTRSSM_EINVAL;
  }
  if (aug->max_rows < 0 || aug->max_rows > H || aug->max_cols < 0 || aug->max_cols > W) {
    set_error("%s: max_rows = %d, max_cols = %d must lie in [0, H = %ld], [0, W = %ld]", what, aug->max_rows, aug->max_cols, (long)H, (long)W);
    return MTRSSM_EINVAL;
  }
  if ((aug->per_frame & ~1) || (noisy & ~1)) { set_error("%s: per_frame and noisy are 0 or 1", what); return MTRSSM_EINVAL; }
  if (!(aug->fill - aug->fill == 0.f)) { set_error("%s: fill must be finite", what); return MTRSSM_EINVAL; }
  if (((uintptr_t)store | (uintptr_t)input | (uintptr_t)target) & 15) { set_error("%s: buffers must be 16-byte aligned", what); return MTRSSM_EINVAL; }
  if (((uintptr_t)start | (uintptr_t)lengths | (uintptr_t)valid_out) & 3) {
    set_error("%s: start, lengths and valid_out must be 4-byte aligned", what);
    return MTRSSM_EINVAL;
  }
  const int mode = lengths ? kGatherRagged : (start ? kGatherWindow : kGatherFirst);
  static const struct {
    decltype(&episode_gather_augmented_kernel<kGatherFirst>) kernel;
    const char* name;
  } table[3] = {{episode_gather_augmented_kernel<kGatherFirst>, "mtrssm::episode_gather_augmented_kernel<first>"},
                {episode_gather_augmented_kernel<kGatherWindow>, "mtrssm::episode_gather_augmented_kernel<window>"},
                {episode_gather_augmented_kernel<kGatherRagged>, "mtrssm::episode_gather_augmented_kernel<ragged>"}};
  if (B > 0x7fffffffL / T) { set_error("%s: B * T = %ld x %ld exceeds 2^31 - 1 frames (one workgroup each)", what, (long)B, (long)T); return MTRSSM_EINVAL; }
  set_last_kernel(table[mode].name);
  hipLaunchKernelGGL(table[mode].kernel, dim3((unsigned)(B * T)), dim3(kThreads), 0, s, *aug, store,
                     reinterpret_cast<const long*>(idx), reinterpret_cast<const int*>(start), reinterpret_cast<const int*>(lengths), key0, key1, akey0,
                     akey1, epoch, (long)n_episodes, (long)T, (long)Tfull, (int)C, (int)H, (int)W, (int)noisy, std_, input, target,
                     reinterpret_cast<int*>(valid_out));
  return check_launch(what);
}

// ------------------------------------------------------------------------------------------------
// Carried state of truncated BPTT: up to MTRSSM_STATE_MAX row-major [B, width] tensors per launch, the
// table of pointers passed by value.  For entry k and row b:
//   dst[b, :] = (!reset || reset[b]) ? src[b * stride : +width] : (alt ? alt[b, :] : 0)
// select: src = the fresh initial state (rows `stride` floats apart: init_proj's halves are column slices), alt = the carry;
// its backward is the same launch with src = the incoming gradient and alt = null (a carried row passes no gradient on);
// save: reset = null, src = the scan's [B, T, width] output at t = T - 1 (stride T * width), dst = the carry.
// reset is read on the device: the launch sequence of a step is the same whether a row starts an episode or continues one.
// blockIdx.y = entry; 16-byte accesses for an entry whose width, stride and pointers allow them, 4-byte ones otherwise.
// ------------------------------------------------------------------------------------------------
struct StateRows {
  const float* src[MTRSSM_STATE_MAX];
  const float* alt[MTRSSM_STATE_MAX];
  float* dst[MTRSSM_STATE_MAX];
  long stride[MTRSSM_STATE_MAX];
  int width[MTRSSM_STATE_MAX];
  int vec[MTRSSM_STATE_MAX];
};

__device__ __forceinline__ void state_rows(const StateRows& t, const unsigned char* __restrict__ reset, long B) {
  const int k = blockIdx.y;
  const float* __restrict__ src = t.src[k];
  const float* __restrict__ alt = t.alt[k];
  float* __restrict__ dst = t.dst[k];
  const long stride = t.stride[k], w = t.width[k];
  if (t.vec[k]) {
    const long w4 = w / 4, total = B * w4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
      const long b = i / w4, q = i - b * w4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!reset || reset[b]) v = reinterpret_cast<const float4*>(src + b * stride)[q];
      else if (alt) v = reinterpret_cast<const float4*>(alt + b * w)[q];
      reinterpret_cast<float4*>(dst + b * w)[q] = v;
    }
  } else {
    const long total = B * w;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
      const long b = i / w, e = i - b * w;
      float v = 0.f;
      if (!reset || reset[b]) v = src[b * stride + e];
      else if (alt) v = alt[b * w + e];
      dst[b * w + e] = v;
    }
  }
}

__global__ __launch_bounds__(kThreads) void state_select_kernel(const StateRows t, const unsigned char* __restrict__ reset, long B) {
  state_rows(t, reset, B);
}
__global__ __launch_bounds__(kThreads) void state_save_kernel(const StateRows t, long B) { state_rows(t, nullptr, B); }

// save at a per-row step: dst[k][b, :] = src[k][b, last[b], :] for 0 <= last[b] < steps, else dst is left as
// it is (an empty row of a ragged batch keeps its carry).  src[k] is the [B, steps, width] base; same lanes as state_rows.
__global__ __launch_bounds__(kThreads) void state_save_at_kernel(const StateRows t, const int* __restrict__ last, long B, long steps) {
  const int k = blockIdx.y;
  const float* __restrict__ src = t.src[k];
  float* __restrict__ dst = t.dst[k];
  const long stride = t.stride[k], w = t.width[k];
  if (t.vec[k]) {
    const long w4 = w / 4, total = B * w4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
      const long b = i / w4, q = i - b * w4, at = last[b];
      if (at < 0 || at >= steps) continue;
      reinterpret_cast<float4*>(dst + b * w)[q] = reinterpret_cast<const float4*>(src + b * stride + at * w)[q];
    }
  } else {
    const long total = B * w;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
      const long b = i / w, e = i - b * w, at = last[b];
      if (at < 0 || at >= steps) continue;
      dst[b * w + e] = src[b * stride + at * w + e];
    }
  }
}

// fills `rows` from the caller's table; `steps` > 0: the save forms (src is [B, steps, width], read at t = steps - 1, or from its
// base when `base`: the kernel adds a per-row step)
static int state_rows_fill(const char* what, const MtrssmStateTable* table, int64_t B, int64_t steps, StateRows* rows, int* grid_x,
                           bool base = false) {
  if (!table || B <= 0) { set_error("%s: null table or B <= 0", what); return MTRSSM_EINVAL; }
  if (table->count <= 0 || table->count > MTRSSM_STATE_MAX) {
    set_error("%s: count %d outside 1 .. %d", what, (int)table->count, MTRSSM_STATE_MAX);
    return MTRSSM_EINVAL;
  }
  int64_t most = 0;
  for (int k = 0; k < MTRSSM_STATE_MAX; ++k) {
    rows->src[k] = rows->alt[k] = nullptr;
    rows->dst[k] = nullptr;
    rows->stride[k] = 0;
    rows->width[k] = rows->vec[k] = 0;
  }
  for (int k = 0; k < table->count; ++k) {
    const int64_t w = table->width[k];
    if (!table->src[k] || !table->dst[k] || w <= 0) { set_error("%s: entry %d has a null pointer or width <= 0", what, k); return MTRSSM_EINVAL; }
    int64_t stride = steps > 0 ? steps * w : table->src_stride[k];
    if (stride < w) { set_error("%s: entry %d has row stride %lld < width %lld", what, k, (long long)stride, (long long)w); return MTRSSM_EINVAL; }
    if (B * w >= (int64_t)1 << 31) { set_error("%s: entry %d has %lld elements (< 2^31)", what, k, (long long)(B * w)); return MTRSSM_EINVAL; }
    const float* src = steps > 0 && !base ? table->src[k] + (steps - 1) * w : table->src[k];
    const float* alt = steps > 0 ? nullptr : table->alt[k];
    if (((uintptr_t)src | (uintptr_t)alt | (uintptr_t)table->dst[k]) & 3) { set_error("%s: entry %d is not 4-byte aligned", what, k); return MTRSSM_EINVAL; }
    rows->src[k] = src;
    rows->alt[k] = alt;
    rows->dst[k] = table->dst[k];
    rows->stride[k] = (long)stride;
    rows->width[k] = (int)w;
    rows->vec[k] = (w % 4 == 0 && stride % 4 == 0 && !(((uintptr_t)src | (uintptr_t)alt | (uintptr_t)table->dst[k]) & 15)) ? 1 : 0;
    const int64_t items = rows->vec[k] ? B * (w / 4) : B * w;
    most = items > most ? items : most;
  }
  *grid_x = grid_for(most) < 64 ? grid_for(most) : 64;
  return MTRSSM_OK;
}

int state_select_launch(const MtrssmStateTable* table, const unsigned char* reset, int64_t B, hipStream_t s) {
  StateRows rows;
  int gx = 1;
  if (!reset) { set_error("state_select: reset is null"); return MTRSSM_EINVAL; }
  if (int rc = state_rows_fill("state_select", table, B, 0, &rows, &gx)) return rc;
  set_last_kernel("mtrssm::state_select_kernel");
  hipLaunchKernelGGL(state_select_kernel, dim3(gx, table->count), dim3(kThreads), 0, s, rows, reset, (long)B);
  return check_launch("state_select");
}

int state_save_launch(const MtrssmStateTable* table, int64_t B, int64_t steps, hipStream_t s) {
  StateRows rows;
  int gx = 1;
  if (steps <= 0) { set_error("state_save: steps must be positive (got %lld)", (long long)steps); return MTRSSM_EINVAL; }
  if (int rc = state_rows_fill("state_save", table, B, steps, &rows, &gx)) return rc;
  set_last_kernel("mtrssm::state_save_kernel");
  hipLaunchKernelGGL(state_save_kernel, dim3(gx, table->count), dim3(kThreads), 0, s, rows, (long)B);
  return check_launch("state_save");
}

int state_save_at_launch(const MtrssmStateTable* table, const int32_t* last, int64_t B, int64_t steps, hipStream_t s) {
  StateRows rows;
  int gx = 1;
  if (!last || ((uintptr_t)last & 3)) { set_error("state_save_at: last is null or not 4-byte aligned"); return MTRSSM_EINVAL; }
  if (steps <= 0) { set_error("state_save_at: steps must be positive (got %lld)", (long long)steps); return MTRSSM_EINVAL; }
  if (int rc = state_rows_fill("state_save_at", table, B, steps, &rows, &gx, true)) return rc;
  set_last_kernel("mtrssm::state_save_at_kernel");
  hipLaunchKernelGGL(state_save_at_kernel, dim3(gx, table->count), dim3(kThreads), 0, s, rows, reinterpret_cast<const int*>(last), (long)B,
                     (long)steps);
  return check_launch("state_save_at");
}

}  // namespace mtrssm
