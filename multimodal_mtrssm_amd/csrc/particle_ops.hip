// Particle-filter likelihood for gfx950: the fold of one time segment of S particles per row -- per-frame
// weights carried in double across segments, the resampling decision and the systematic resampling itself on the device -- and the
// gather of the particles' end-of-segment states by ancestor.  The fold computes in double, reduces in a fixed order without atomics
// and rounds every plane to fp32 once, so two calls agree bitwise; a row's result depends on that row only.
#include "row_fold.h"
#include "scan_common.h"

namespace mtrssm {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxParticles = 16;
constexpr double kHalfLog2Pi = 0.9189385332046727;  // 0.5 * log(2 * pi)

// The layout of iw_bound_kernel: a 16-lane DPP row per batch row b (four per wave), lane s of it owns particle s and walks the
// segment's frames serially with lw[b][s] in a register; the lanes s >= S carry the neutral element of every reduction and no lane
// leaves before the end (the DPP steps and the broadcasts need the whole wave).  Lane 0 of a row writes the eight planes of a frame.
// At the segment's last frame the prefix sums of the weights and the ancestors' counts are a walk in lane order: w_s is broadcast
// within the row in ascending s, so c_s is the left fold the float64 rule states, and lane i counts the c_s at or below its target.
__global__ __launch_bounds__(kThreads) void particle_fold_kernel(const float* __restrict__ se_audio, const float* __restrict__ se_vision,
                                                                 const float* __restrict__ log_ratio, const int32_t* __restrict__ valid,
                                                                 const float* __restrict__ u, int64_t u_stride, int t0, int B, int S, int c,
                                                                 double const_audio, double const_vision, double threshold, int last_segment,
                                                                 double* __restrict__ carry, float* __restrict__ planes,
                                                                 int32_t* __restrict__ ancestor) {
  const int s = threadIdx.x & 15;
  const int row_lane0 = (threadIdx.x & (kWave - 1)) & ~15;  // the wave's lane that holds particle 0 of this row
  const int b = (int)((blockIdx.x * (int64_t)kThreads + threadIdx.x) >> 4);
  const bool row = b < B, own = row && s < S;
  const int br = row ? b : 0;
  int n = 0;  // live frames of this segment: t0 + j is live iff j < n
  int64_t left = 0;  // valid[b] - t0: frames of the row from the segment's first on
  if (row) {
    left = valid ? (int64_t)(valid[b] < 0 ? 0 : valid[b]) - t0 : (int64_t)1 << 40;
    n = left < 0 ? 0 : (left > c ? c : (int)left);
  }
  const int64_t in0 = ((int64_t)br * S + (own ? s : 0)) * c;
  const int64_t plane = (int64_t)B * c, out0 = (int64_t)br * c;
  const double s_d = (double)S, log_s = log(s_d);
  double* __restrict__ cr = carry + (int64_t)br * (S + 2);
  double lw = own ? cr[s] : 0.0, base = cr[S], prev = cr[S + 1];
  const double u_row = (row && u && !last_segment) ? (double)u[(int64_t)b * u_stride] : 0.0;
  int anc = s;
  // the next frame's three inputs are requested before this frame's arithmetic: the loads' latency hides behind it
  float na = 0.f, nv = 0.f, nr = 0.f;
  if (own && 0 < n) {
    if (se_audio) na = se_audio[in0];
    if (se_vision) nv = se_vision[in0];
    if (log_ratio) nr = log_ratio[in0];
  }
  for (int j = 0; j < c; ++j) {
    const bool live = j < n;  // (uniform over the row of 16)
    const float fa = na, fv = nv, fr = nr;
    if (own && j + 1 < n) {
      if (se_audio) na = se_audio[in0 + j + 1];
      if (se_vision) nv = se_vision[in0 + j + 1];
      if (log_ratio) nr = log_ratio[in0 + j + 1];
    }
    double a = 0.0, v = 0.0, r = 0.0;
    if (own && live) {
      if (se_audio) a = -(double)fa - const_audio;
      if (se_vision) v = -(double)fv - const_vision;
      if (log_ratio) r = (double)fr;
    }
    const double l = (a + v) + r;
    lw += l;
    const double mx = row_max_d(own ? lw : -INFINITY);
    const double w = own ? exp(lw - mx) : 0.0;
    const double sum_w = row_sum_d(w), sum_w2 = row_sum_d(w * w), sum_l = row_sum_d(l);
    const double sum_a = row_sum_d(a), sum_v = row_sum_d(v), sum_r = row_sum_d(r);
    const double l_now = base + (mx + log(sum_w)) - log_s, ess = (sum_w * sum_w) / sum_w2;
    bool resample = false;
    if (j == c - 1 && !last_segment) {  // (uniform over the launch: every lane walks)
      double total = 0.0;
      for (int k = 0; k < S; ++k) total += __shfl(w, row_lane0 + k, kWave);
      const double target = ((u_row + (double)s) / s_d) * total;
      double prefix = 0.0;
      int count = 0;
      for (int k = 0; k < S; ++k) {
        prefix += __shfl(w, row_lane0 + k, kWave);
        count += prefix <= target ? 1 : 0;
      }
      resample = live && (int64_t)j + 1 < left && ess <= threshold * s_d;
      if (resample) anc = count < S - 1 ? count : S - 1;
    }
    if (row && s == 0) {
      float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (live) {
        o[0] = (float)(l_now - prev);
        o[1] = (float)(sum_l / s_d);
        o[2] = (float)(sum_a / s_d);
        o[3] = (float)(sum_v / s_d);
        o[4] = (float)(sum_r / s_d);
        o[5] = (float)ess;
        o[6] = resample ? 1.f : 0.f;
        o[7] = (float)l_now;
      }
#pragma unroll
      for (int p = 0; p < 8; ++p) planes[p * plane + out0 + j] = o[p];
    }
    if (live) prev = l_now;
    if (resample) {
      base = l_now;
      lw = 0.0;
    }
  }
  if (own) {
    cr[s] = lw;
    ancestor[(int64_t)b * S + s] = anc;
  }
  if (row && s == 0) {
    cr[S] = base;
    cr[S + 1] = prev;
  }
}

// dst[k][b * S + i, :] = src[k][(b * S + ancestor[b, i]) * stride + (steps - 1) * width : + width]; blockIdx.y = entry; 16-byte
// accesses for an entry whose width and pointers allow them, 4-byte ones otherwise.  An ancestor outside 0 .. S - 1 is clamped:
// nothing outside the row's S particles is ever read.
struct ParticleRows {
  const float* src[MTRSSM_STATE_MAX];  // at step steps - 1 of row 0
  float* dst[MTRSSM_STATE_MAX];
  long stride[MTRSSM_STATE_MAX];  // floats between the rows of src: steps * width
  int width[MTRSSM_STATE_MAX];
  int vec[MTRSSM_STATE_MAX];
};

__global__ __launch_bounds__(kThreads) void particle_gather_kernel(const ParticleRows t, const int32_t* __restrict__ ancestor, long rows, int S) {
  const int k = blockIdx.y;
  const float* __restrict__ src = t.src[k];
  float* __restrict__ dst = t.dst[k];
  const long stride = t.stride[k], w = t.width[k];
  const long per = t.vec[k] ? w / 4 : w, total = rows * per;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / per, q = i - r * per;
    int a = ancestor[r];
    a = a < 0 ? 0 : (a > S - 1 ? S - 1 : a);
    const long from = (r / S) * S + a;
    if (t.vec[k]) reinterpret_cast<float4*>(dst + r * w)[q] = reinterpret_cast<const float4*>(src + from * stride)[q];
    else dst[r * w + q] = src[from * stride + q];
  }
}

}  // namespace

int particle_fold_launch(const float* se_audio, const float* se_vision, const float* log_ratio, const int32_t* valid, const float* u,
                         int64_t u_stride, int64_t t0, int64_t B, int64_t S, int64_t c, int64_t event_audio, int64_t event_vision,
                         double threshold, int last_segment, double* carry, float* planes, int32_t* ancestor, hipStream_t s) {
  if (!carry || !planes || !ancestor || (!se_audio && !se_vision && !log_ratio)) {
    set_error("particle_fold: null pointer (carry, planes, ancestor, or all three inputs)");
    return MTRSSM_EINVAL;
  }
  if (last_segment != 0 && last_segment != 1) { set_error("particle_fold: last_segment is 0 or 1 (got %d)", last_segment); return MTRSSM_EINVAL; }
  if (!last_segment && (!u || u_stride < 1)) { set_error("particle_fold: a segment that may resample needs u and u_stride >= 1"); return MTRSSM_EINVAL; }
  if (B <= 0 || c <= 0 || t0 < 0 || (se_audio && event_audio <= 0) || (se_vision && event_vision <= 0)) {
    set_error("particle_fold: need B, c > 0, t0 >= 0 and an event size > 0 for every data term given (got %lld %lld %lld %lld %lld)", (long long)B,
              (long long)c, (long long)t0, (long long)event_audio, (long long)event_vision);
    return MTRSSM_EINVAL;
  }
  if (S < 1 || S > kMaxParticles) { set_error("particle_fold: need 1 <= S <= %d particles (got %lld)", kMaxParticles, (long long)S); return MTRSSM_EINVAL; }
  if (!(threshold >= 0.0 && threshold <= 1.0)) { set_error("particle_fold: need 0 <= threshold <= 1 (got %g)", threshold); return MTRSSM_EINVAL; }
  if (B >= (int64_t)1 << 24 || c >= (int64_t)1 << 24 || B * c >= (int64_t)1 << 24 || t0 >= (int64_t)1 << 30 || u_stride >= (int64_t)1 << 30) {
    set_error("particle_fold: %lld x %lld frames from %lld (B * c must stay below 2^24, t0 and u_stride below 2^30)", (long long)B, (long long)c,
              (long long)t0);
    return MTRSSM_EINVAL;
  }
  if ((((uintptr_t)se_audio | (uintptr_t)se_vision | (uintptr_t)log_ratio | (uintptr_t)valid | (uintptr_t)u | (uintptr_t)planes |
        (uintptr_t)ancestor) & 3) || ((uintptr_t)carry & 7)) {
    set_error("particle_fold: buffers must be 4-byte aligned, the carry 8-byte");
    return MTRSSM_EINVAL;
  }
  const int64_t blocks = (B * 16 + kThreads - 1) / kThreads;
  set_last_kernel("mtrssm::particle_fold_kernel");
  hipLaunchKernelGGL(particle_fold_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, se_audio, se_vision, log_ratio, valid, u, u_stride, (int)t0,
                     (int)B, (int)S, (int)c, kHalfLog2Pi * (double)event_audio, kHalfLog2Pi * (double)event_vision, threshold, last_segment, carry,
                     planes, ancestor);
  return check_launch("particle_fold");
}

int particle_gather_launch(const MtrssmStateTable* table, const int32_t* ancestor, int64_t B, int64_t S, int64_t steps, hipStream_t s) {
  if (!table || !ancestor || ((uintptr_t)ancestor & 3)) { set_error("particle_gather: null table, or ancestor null or not 4-byte aligned"); return MTRSSM_EINVAL; }
  if (B <= 0 || steps <= 0 || S < 1 || S > kMaxParticles) {
    set_error("particle_gather: need B, steps > 0 and 1 <= S <= %d (got %lld %lld %lld)", kMaxParticles, (long long)B, (long long)steps, (long long)S);
    return MTRSSM_EINVAL;
  }
  if (table->count <= 0 || table->count > MTRSSM_STATE_MAX) {
    set_error("particle_gather: count %d outside 1 .. %d", (int)table->count, MTRSSM_STATE_MAX);
    return MTRSSM_EINVAL;
  }
  const int64_t rows = B * S;
  ParticleRows pr;
  int64_t most = 0;
  for (int k = 0; k < MTRSSM_STATE_MAX; ++k) {
    pr.src[k] = nullptr;
    pr.dst[k] = nullptr;
    pr.stride[k] = 0;
    pr.width[k] = pr.vec[k] = 0;
  }
  for (int k = 0; k < table->count; ++k) {
    const int64_t w = table->width[k];
    if (!table->src[k] || !table->dst[k] || w <= 0) { set_error("particle_gather: entry %d has a null pointer or width <= 0", k); return MTRSSM_EINVAL; }
    if (table->src[k] == table->dst[k]) { set_error("particle_gather: entry %d gathers in place (src == dst)", k); return MTRSSM_EINVAL; }
    int64_t stride = 0, elems = 0;
    if (__builtin_mul_overflow(steps, w, &stride) || __builtin_mul_overflow(rows, stride, &elems) || elems >= (int64_t)1 << 31) {
      set_error("particle_gather: entry %d has B * S * steps * width >= 2^31", k);
      return MTRSSM_EINVAL;
    }
    const float* src = table->src[k] + (steps - 1) * w;
    if (((uintptr_t)src | (uintptr_t)table->dst[k]) & 3) { set_error("particle_gather: entry %d is not 4-byte aligned", k); return MTRSSM_EINVAL; }
    pr.src[k] = src;
    pr.dst[k] = table->dst[k];
    pr.stride[k] = (long)stride;
    pr.width[k] = (int)w;
    pr.vec[k] = (w % 4 == 0 && !(((uintptr_t)src | (uintptr_t)table->dst[k]) & 15)) ? 1 : 0;
    const int64_t items = pr.vec[k] ? rows * (w / 4) : rows * w;
    most = items > most ? items : most;
  }
  const int64_t want = (most + kThreads - 1) / kThreads;
  set_last_kernel("mtrssm::particle_gather_kernel");
  hipLaunchKernelGGL(particle_gather_kernel, dim3((unsigned)(want < 256 ? want : 256), table->count), dim3(kThreads), 0, s, pr, ancestor, (long)rows,
                     (int)S);
  return check_launch("particle_gather");
}

}  // namespace mtrssm
