// Generation coherence for gfx950: the two readers' logits of every copy-frame of a sampled rollout scored
// against the frame's label and against each other -- hits, agreement, the joint hit, the soft agreement sum_k pv_k pa_k and the
// (vision digit, audio digit) histogram -- in ONE pass over the logits plus a fixed-order fold by horizon.  Both kernels compute in
// double, add floating point without atomics in an order that depends on the shapes only (the histogram counts integers), so two
// calls agree bitwise; the planes are rounded to fp32 once.
#include "scan_common.h"

namespace mtrssm {

namespace {

constexpr int kRowThreads = 256;
constexpr int kFrames = 16;       // frames of a staged span: S * kFrames <= kRowThreads copy-frames, one per thread
constexpr int kMaxSamples = 16;
constexpr int kMaxGroups = 4;
constexpr int kClasses = 10;
constexpr int kBins = kClasses + 1;  // the ten digits and the failure bin
constexpr int kPlanes = 5;           // vision, audio, agree, joint, soft
constexpr int kPairCells = 2 * kBins * kBins;
constexpr int kFoldThreads = 256;
constexpr int kMaxBlocks = 1024;

// Scan row of copy (g, s) of row b: (b * G + g) * S + s; r = b * G + g names a row's group.  A group's block of the table:
// sums [5][T] by horizon, counts [T], pairs [2][11][11].  c = min(context, T).
struct CoherenceGeom {
  int B, G, S, T, c, blocks;
  int64_t GS;
};

__device__ __forceinline__ int row_length(const int32_t* __restrict__ valid, int b, int T) {
  if (!valid) return T;
  const int n = valid[b];
  return n < 0 ? 0 : (n > T ? T : n);
}

__device__ __forceinline__ bool frame_live(const int32_t* __restrict__ labels, const int32_t* __restrict__ valid, int b, int t, int T) {
  const int label = labels[(int64_t)b * T + t];
  return t < row_length(valid, b, T) && label >= 0 && label < kClasses;
}

// The lowest index among the largest of 10 logits and that maximum, in double; 10 when a logit is not finite.
__device__ __forceinline__ int first_max(const float* z, double* m) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < kClasses; ++k) ok = ok && __builtin_isfinite(z[k]);
  if (!ok) return kClasses;
  double mx = z[0];
  int d = 0;
#pragma unroll
  for (int k = 1; k < kClasses; ++k)
    if ((double)z[k] > mx) {
      mx = z[k];
      d = k;
    }
  *m = mx;
  return d;
}

// sum_k pv_k pa_k with p_k = exp(z_k - max) / (the left fold of exp(z_k - max) over ascending k); every product and sum is rounded
// on its own (no contraction), classes in ascending order.
__device__ __forceinline__ double soft_agreement(const float* zv, double mv, const float* za, double ma) {
#pragma clang fp contract(off)
  double ev[kClasses], ea[kClasses], sv = 0.0, sa = 0.0;
#pragma unroll
  for (int k = 0; k < kClasses; ++k) {
    ev[k] = exp((double)zv[k] - mv);
    ea[k] = exp((double)za[k] - ma);
    sv += ev[k];
    sa += ea[k];
  }
  double soft = 0.0;
#pragma unroll
  for (int k = 0; k < kClasses; ++k) soft += (ev[k] / sv) * (ea[k] / sa);
  return soft;
}

// One workgroup per group r = b * G + g of a row (grid-stride over r).  The S copies of (b, g) are S consecutive scan rows; a span of
// nt <= 16 frames of them -- S runs of nt * 10 consecutive floats per reader -- is staged in LDS with coalesced loads, then thread
// s * nt + f scores copy s of frame t0 + f in double and leaves its five values in LDS, and thread p * nt + f adds plane p's values of
// frame t0 + f over s = 0 .. S - 1 from +0: the frame sum u, which goes to the workspace, and u / S, rounded to fp32 once, to the plane.
// A dead frame is not scored: its u and its planes are exactly 0.  The (phase, dv, da) histogram of the workgroup's live copy-frames is
// counted in LDS as integers and written out as the workgroup's partial set.
__global__ __launch_bounds__(kRowThreads) void coherence_rows_kernel(const float* __restrict__ logits_v, const float* __restrict__ logits_a,
                                                                     const int32_t* __restrict__ labels, const int32_t* __restrict__ valid,
                                                                     const CoherenceGeom g, float* __restrict__ planes, double* __restrict__ u_ws,
                                                                     int32_t* __restrict__ pair_ws) {
  __shared__ float s_v[kMaxSamples * kFrames * kClasses], s_a[kMaxSamples * kFrames * kClasses];
  __shared__ double s_val[kPlanes][kFrames][kMaxSamples];
  __shared__ int32_t s_hist[kMaxGroups * kPairCells];
  const int tid = threadIdx.x;
  const int64_t R = (int64_t)g.B * g.G, plane = R * g.T;
  for (int i = tid; i < g.G * kPairCells; i += kRowThreads) s_hist[i] = 0;
  __syncthreads();
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const int b = (int)(r / g.G), group = (int)(r - (int64_t)b * g.G);
    const int64_t row0 = r * g.S;  // the first of the S scan rows
    for (int t0 = 0; t0 < g.T; t0 += kFrames) {
      const int nt = g.T - t0 < kFrames ? g.T - t0 : kFrames;
      const int run = nt * kClasses;
      for (int x = tid; x < g.S * run; x += kRowThreads) {
        const int s = x / run, j = x - s * run;
        const int64_t at = ((row0 + s) * g.T + t0) * kClasses + j;
        s_v[s * kFrames * kClasses + j] = logits_v[at];
        s_a[s * kFrames * kClasses + j] = logits_a[at];
      }
      __syncthreads();
      if (tid < g.S * nt) {
        const int s = tid / nt, f = tid - s * nt, t = t0 + f;
        double v[kPlanes] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (frame_live(labels, valid, b, t, g.T)) {
          const int label = labels[(int64_t)b * g.T + t];
          const float* zv = &s_v[(s * kFrames + f) * kClasses];
          const float* za = &s_a[(s * kFrames + f) * kClasses];
          double mv = 0.0, ma = 0.0;
          const int dv = first_max(zv, &mv), da = first_max(za, &ma);
          v[0] = dv == label ? 1.0 : 0.0;
          v[1] = da == label ? 1.0 : 0.0;
          v[2] = (dv == da && dv < kClasses) ? 1.0 : 0.0;
          v[3] = (dv == da && dv == label) ? 1.0 : 0.0;
          if (dv < kClasses && da < kClasses) v[4] = soft_agreement(zv, mv, za, ma);
          const int phase = t < g.c ? 0 : 1;
          atomicAdd(&s_hist[(group * 2 + phase) * kBins * kBins + dv * kBins + da], 1);  // (an integer count in LDS)
        }
#pragma unroll
        for (int p = 0; p < kPlanes; ++p) s_val[p][f][s] = v[p];
      }
      __syncthreads();
      if (tid < kPlanes * nt) {
        const int p = tid / nt, f = tid - p * nt;
        double u = 0.0;
        for (int s = 0; s < g.S; ++s) u += s_val[p][f][s];
        const int64_t at = p * plane + r * g.T + t0 + f;
        u_ws[at] = u;
        if (planes) planes[at] = (float)(u / (double)g.S);
      }
      __syncthreads();  // (the next span overwrites the staging buffers)
    }
  }
  __syncthreads();
  for (int i = tid; i < g.G * kPairCells; i += kRowThreads) pair_ws[(int64_t)blockIdx.x * g.G * kPairCells + i] = s_hist[i];
}

// One thread per cell of the table.  sums (g, p, h): a left fold from +0 over b ascending and, within a row, over t ascending of
// u[p][b * G + g][t] with h(t) = h -- bin 0 takes the c context frames of every row, bin h > 0 the frame c + h - 1 (dead frames, exactly
// +0, included: they change nothing).  counts: S times the live frames of the bin; pairs: the sum of the workgroups' integer partial
// sets.  Each result is added once onto what the cell holds (so a second call of the same step doubles a cell exactly).
__global__ __launch_bounds__(kFoldThreads) void coherence_fold_kernel(const double* __restrict__ u_ws, const int32_t* __restrict__ pair_ws,
                                                                      const int32_t* __restrict__ labels, const int32_t* __restrict__ valid,
                                                                      const CoherenceGeom g, double* __restrict__ table) {
  const int64_t cells = (int64_t)g.G * g.GS;
  const int64_t R = (int64_t)g.B * g.G, plane = R * g.T;
  for (int64_t x = (int64_t)blockIdx.x * kFoldThreads + threadIdx.x; x < cells; x += (int64_t)gridDim.x * kFoldThreads) {
    const int group = (int)(x / g.GS);
    const int64_t cell = x - (int64_t)group * g.GS;
    double v = 0.0;
    if (cell < (int64_t)kPlanes * g.T) {
      const int p = (int)(cell / g.T), h = (int)(cell - (int64_t)p * g.T);
      const int first = h == 0 ? 0 : g.c + h - 1, last = h == 0 ? g.c : g.c + h;  // the bin's frames [first, last)
      if (first < g.T)
        for (int b = 0; b < g.B; ++b) {
          const double* row = u_ws + p * plane + ((int64_t)b * g.G + group) * g.T;
#pragma unroll 4
          for (int t = first; t < last; ++t) v += row[t];
        }
    } else if (cell < (int64_t)(kPlanes + 1) * g.T) {
      const int h = (int)(cell - (int64_t)kPlanes * g.T);
      const int first = h == 0 ? 0 : g.c + h - 1, last = h == 0 ? g.c : g.c + h;
      long long total = 0;
      if (first < g.T)
        for (int b = 0; b < g.B; ++b)
          for (int t = first; t < last; ++t) total += frame_live(labels, valid, b, t, g.T) ? 1 : 0;
      v = (double)(total * g.S);
    } else {
      const int y = (int)(cell - (int64_t)(kPlanes + 1) * g.T);
      long long total = 0;
      for (int k = 0; k < g.blocks; ++k) total += pair_ws[((int64_t)k * g.G + group) * kPairCells + y];
      v = (double)total;
    }
    table[x] += v;
  }
}

int64_t round8(int64_t bytes) { return (bytes + 7) & ~(int64_t)7; }

// The geometry and the workspace's two regions (the frame sums u [5][B * G][T], the workgroups' pair counts), or false.
bool coherence_geometry(int64_t B, int64_t G, int64_t S, int64_t T, int64_t context, CoherenceGeom* g, int64_t* bytes_u, int64_t* bytes_pairs) {
  const int64_t big = (int64_t)1 << 24;
  if (B <= 0 || T <= 0 || S <= 0 || context <= 0 || G < 1 || G > kMaxGroups || S > kMaxSamples || B >= big || T >= big) return false;
  int64_t frames = 0;
  if (__builtin_mul_overflow(B * G * S, T, &frames) || frames >= big) return false;
  const int64_t rows = B * G;
  g->B = (int)B;
  g->G = (int)G;
  g->S = (int)S;
  g->T = (int)T;
  g->c = (int)(context < T ? context : T);
  g->blocks = (int)(rows < kMaxBlocks ? rows : kMaxBlocks);
  g->GS = (kPlanes + 1) * T + kPairCells;
  *bytes_u = kPlanes * rows * T * (int64_t)sizeof(double);
  *bytes_pairs = round8((int64_t)g->blocks * G * kPairCells * (int64_t)sizeof(int32_t));
  return true;
}

}  // namespace

int64_t coherence_fold_workspace_bytes(int64_t B, int64_t G, int64_t S, int64_t T) {
  CoherenceGeom g;
  int64_t a = 0, b = 0;
  if (!coherence_geometry(B, G, S, T, 1, &g, &a, &b)) return -1;
  return a + b;
}

int coherence_fold_launch(const float* logits_v, const float* logits_a, const int32_t* labels, const int32_t* valid, int64_t B, int64_t G, int64_t S,
                          int64_t T, int64_t context, float* planes, double* table, void* workspace, int64_t workspace_bytes, hipStream_t st) {
  if (!logits_v || !logits_a || !labels || !table || !workspace) { set_error("coherence_fold: null pointer"); return MTRSSM_EINVAL; }
  CoherenceGeom g;
  int64_t bytes_u = 0, bytes_pairs = 0;
  if (!coherence_geometry(B, G, S, T, context, &g, &bytes_u, &bytes_pairs)) {
    set_error("coherence_fold: need B, T, S, context > 0, 1 <= G <= 4, S <= 16 and B * G * S * T < 2^24 (got B %lld G %lld S %lld T %lld context %lld)",
              (long long)B, (long long)G, (long long)S, (long long)T, (long long)context);
    return MTRSSM_EINVAL;
  }
  if ((((uintptr_t)logits_v | (uintptr_t)logits_a | (uintptr_t)labels | (uintptr_t)valid | (uintptr_t)planes) & 3) ||
      (((uintptr_t)table | (uintptr_t)workspace) & 7)) {
    set_error("coherence_fold: buffers must be 4-byte aligned, the table and the workspace 8-byte");
    return MTRSSM_EINVAL;
  }
  if (workspace_bytes < bytes_u + bytes_pairs) {
    set_error("coherence_fold: the workspace has %lld bytes, mtrssm_coherence_fold_workspace_bytes asks for %lld", (long long)workspace_bytes,
              (long long)(bytes_u + bytes_pairs));
    return MTRSSM_EINVAL;
  }
  char* ws = static_cast<char*>(workspace);
  double* u_ws = reinterpret_cast<double*>(ws);
  int32_t* pair_ws = reinterpret_cast<int32_t*>(ws + bytes_u);
  const int64_t cells = (int64_t)g.G * g.GS;
  const int64_t fold_blocks = (cells + kFoldThreads - 1) / kFoldThreads;
  set_last_kernel("mtrssm::coherence_rows_kernel");
  hipLaunchKernelGGL(coherence_rows_kernel, dim3((unsigned)g.blocks), dim3(kRowThreads), 0, st, logits_v, logits_a, labels, valid, g, planes, u_ws,
                     pair_ws);
  hipLaunchKernelGGL(coherence_fold_kernel, dim3((unsigned)(fold_blocks < kMaxBlocks ? fold_blocks : kMaxBlocks)), dim3(kFoldThreads), 0, st, u_ws,
                     pair_ws, labels, valid, g, table);
  return check_launch("coherence_fold");
}

}  // namespace mtrssm
