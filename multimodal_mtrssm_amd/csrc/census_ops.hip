// Latent census for gfx950: per categorical of a posterior rollout the entropies, the KL to the prior, the
// KL from the row's first copy, the class counts, the aggregate posterior / prior and the frame-to-frame switches of the sampled
// class, in ONE pass over the scan's outputs plus a fixed-order fold.  Both kernels compute in double, use no atomics and add in an
// order that depends on the shapes only, so two calls agree bitwise; the planes are rounded to fp32 once.
#include "scan_common.h"

namespace mtrssm {

namespace {

constexpr int kRowThreads = kWave;  // one wave per scan row: its barriers cost nothing and a CU holds many rows
constexpr int kTile = 512;          // floats of each input a row stages in LDS per span
constexpr int kSpan = kWave;        // categoricals of a span: one per lane
constexpr int kPlanes = 5;          // post_entropy, prior_entropy, kl, cross, switches
constexpr int kFoldThreads = 256;
constexpr int kMaxBlocks = 4096;

// Scan row r = b * G + g.  PS = 3 K C + 5 K doubles per row partial: n, qsum, psum [K][C], then hq, hp, kl, cross, sw [K].
// A group's block of the table: the partial's PS cells, frames, pairs, the position sums [5][T], the live rows per position [T].
struct CensusGeom {
  int B, G, T, K, C;
  int kc, staged, single;
  int64_t KC, PS, GS;
};

__device__ __forceinline__ int row_length(const int32_t* __restrict__ valid, int b, int T) {
  if (!valid) return T;
  const int n = valid[b];
  return n < 0 ? 0 : (n > T ? T : n);
}

// Max and log-sum of one categorical's C logits, in double, classes in ascending order (as mtrssm_latent_log_ratio forms them).
__device__ __forceinline__ void cat_norm(const float* x, int C, double* m, double* l) {
  double mx = x[0];
  for (int c = 1; c < C; ++c) mx = fmax(mx, (double)x[c]);
  double s = 0.0;
  for (int c = 0; c < C; ++c) s += exp((double)x[c] - mx);
  *m = mx;
  *l = log(s);
}

// One wave per scan row; lane j owns categorical k0 + j of a span of kc <= 64 categoricals and walks the row's live frames in
// ascending t, so every accumulator of a row is a left fold over t that starts at +0.  staged (C <= kTile): the span's logits and
// sample (and the first copy's posterior when g > 0) are copied into LDS with coalesced loads (lane i reads float i, i + 64, ...);
// else a lane reads its categorical in place.  single (K <= 64 and K * C <= kTile): the row's partial and the previous classes stay
// in LDS until the row ends; else they live in the workspace and the owning lane updates them there.  Lane 0 adds a frame's
// per-categorical values in ascending k and writes the five planes, exactly 0 on a dead frame.  The trip counts depend on the
// launch's sizes and on valid[b] only (uniform over the wave).
__global__ __launch_bounds__(kRowThreads) void census_rows_kernel(const float* __restrict__ post, const float* __restrict__ prior,
                                                                  const float* __restrict__ stoch, const int32_t* __restrict__ valid,
                                                                  const CensusGeom g, float* __restrict__ planes, double* __restrict__ partials,
                                                                  int32_t* __restrict__ prev_ws) {
  __shared__ float s_q[kTile], s_p[kTile], s_s[kTile], s_q0[kTile];
  __shared__ double s_d[kPlanes][kSpan];
  __shared__ double s_part[3 * kTile + kPlanes * kSpan];
  __shared__ int32_t s_prev[kSpan];
  const int lane = threadIdx.x;
  const int64_t R = (int64_t)g.B * g.G, plane = R * g.T;
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const int b = (int)(r / g.G), copy = (int)(r - (int64_t)b * g.G);
    const int n = row_length(valid, b, g.T);
    double* part = partials + r * g.PS;
    double* acc = g.single ? s_part : part;
    int32_t* prev = g.single ? s_prev : prev_ws + r * g.K;
    for (int64_t i = lane; i < g.PS; i += kRowThreads) acc[i] = 0.0;
    __syncthreads();
    double* cls_n = acc;
    double* cls_q = acc + g.KC;
    double* cls_p = acc + 2 * g.KC;
    double* cat = acc + 3 * g.KC;
    for (int t = 0; t < n; ++t) {
      const int64_t frame = (r * g.T + t) * g.KC, frame0 = (((int64_t)b * g.G) * g.T + t) * g.KC;
      double sum[kPlanes] = {0.0, 0.0, 0.0, 0.0, 0.0};  // (lane 0: the frame's running sums in ascending k)
      for (int k0 = 0; k0 < g.K; k0 += g.kc) {
        const int nk = g.K - k0 < g.kc ? g.K - k0 : g.kc;
        const int64_t off = (int64_t)k0 * g.C;
        if (g.staged)
          for (int x = lane; x < nk * g.C; x += kRowThreads) {
            s_q[x] = post[frame + off + x];
            s_p[x] = prior[frame + off + x];
            s_s[x] = stoch[frame + off + x];
            if (copy > 0) s_q0[x] = post[frame0 + off + x];
          }
        __syncthreads();
        if (lane < nk) {
          const int k = k0 + lane;
          const int64_t at = off + (int64_t)lane * g.C;
          const float* q = g.staged ? &s_q[lane * g.C] : post + frame + at;
          const float* p = g.staged ? &s_p[lane * g.C] : prior + frame + at;
          const float* s = g.staged ? &s_s[lane * g.C] : stoch + frame + at;
          const float* q0 = g.staged ? &s_q0[lane * g.C] : post + frame0 + at;
          double qm, ql, pm, pl, q0m = 0.0, q0l = 0.0;
          cat_norm(q, g.C, &qm, &ql);
          cat_norm(p, g.C, &pm, &pl);
          if (copy > 0) cat_norm(q0, g.C, &q0m, &q0l);
          int star = -1;
          double qlq = 0.0, plp = 0.0, kl = 0.0, cross = 0.0;
          const int64_t cell = (int64_t)k * g.C;
          for (int c = 0; c < g.C; ++c) {
            const double lq = ((double)q[c] - qm) - ql, lp = ((double)p[c] - pm) - pl;
            const double qq = exp(lq), pp = exp(lp);
            if (star < 0 && s[c] > 0.5f) star = c;
            if (qq > 0.0) {
              qlq += qq * lq;
              kl += qq * (lq - lp);
            }
            if (pp > 0.0) plp += pp * lp;
            if (copy > 0) {
              const double lq0 = ((double)q0[c] - q0m) - q0l;
              const double qq0 = exp(lq0);
              if (qq0 > 0.0) cross += qq0 * (lq0 - lq);
            }
            cls_q[cell + c] += qq;
            cls_p[cell + c] += pp;
          }
          if (star < 0) star = 0;
          cls_n[cell + star] += 1.0;
          const double sw = (t >= 1 && star != prev[k]) ? 1.0 : 0.0;
          prev[k] = star;
          const double v[kPlanes] = {-qlq, -plp, kl, cross, sw};
#pragma unroll
          for (int i = 0; i < kPlanes; ++i) {
            cat[(int64_t)i * g.K + k] += v[i];
            s_d[i][lane] = v[i];
          }
        }
        __syncthreads();
        if (lane == 0)
          for (int j = 0; j < nk; ++j) {
#pragma unroll
            for (int i = 0; i < kPlanes; ++i) sum[i] += s_d[i][j];
          }
        __syncthreads();  // (the next span overwrites the staging buffers)
      }
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kPlanes; ++i) planes[i * plane + r * g.T + t] = (float)sum[i];
      }
    }
    for (int x = n * kPlanes + lane; x < g.T * kPlanes; x += kRowThreads) planes[(x % kPlanes) * plane + r * g.T + x / kPlanes] = 0.f;
    __syncthreads();
    if (g.single)
      for (int64_t i = lane; i < g.PS; i += kRowThreads) part[i] = s_part[i];
    __syncthreads();  // (the next row clears s_part)
  }
}

// One thread per cell of the table: the step's sum is a left fold from +0 over the rows' values in ascending b, added once onto what
// the cell holds (so a second call of the same step doubles a cell exactly).  The position sums read the fp32 planes back as doubles,
// dead frames (exactly 0) included; the three kinds of count are whole numbers.
__global__ __launch_bounds__(kFoldThreads) void census_fold_kernel(const double* __restrict__ partials, const float* __restrict__ planes,
                                                                   const int32_t* __restrict__ valid, const CensusGeom g,
                                                                   double* __restrict__ table) {
  const int64_t cells = (int64_t)g.G * g.GS;
  const int64_t R = (int64_t)g.B * g.G, plane = R * g.T;
  for (int64_t x = (int64_t)blockIdx.x * kFoldThreads + threadIdx.x; x < cells; x += (int64_t)gridDim.x * kFoldThreads) {
    const int copy = (int)(x / g.GS);
    const int64_t cell = x - (int64_t)copy * g.GS;
    double v = 0.0;
    if (cell < g.PS) {
      for (int b = 0; b < g.B; ++b) v += partials[((int64_t)b * g.G + copy) * g.PS + cell];
    } else if (cell < g.PS + 2) {
      const int pairs = (int)(cell - g.PS);  // 0 frames: n_b; 1 pairs: max(n_b - 1, 0)
      long long total = 0;
      for (int b = 0; b < g.B; ++b) {
        const int n = row_length(valid, b, g.T);
        total += pairs ? (n > 0 ? n - 1 : 0) : n;
      }
      v = (double)total;
    } else if (cell < g.PS + 2 + (int64_t)kPlanes * g.T) {
      const int64_t y = cell - (g.PS + 2);
      const int p = (int)(y / g.T), t = (int)(y - (int64_t)p * g.T);
      for (int b = 0; b < g.B; ++b) v += (double)planes[p * plane + ((int64_t)b * g.G + copy) * g.T + t];
    } else {
      const int t = (int)(cell - (g.PS + 2 + (int64_t)kPlanes * g.T));
      long long total = 0;
      for (int b = 0; b < g.B; ++b) total += t < row_length(valid, b, g.T) ? 1 : 0;
      v = (double)total;
    }
    table[x] += v;
  }
}

int64_t round8(int64_t bytes) { return (bytes + 7) & ~(int64_t)7; }

// The geometry and the workspace's three regions (row partials, planes for a call without them, previous classes), or false.
bool census_geometry(int64_t B, int64_t G, int64_t T, int64_t K, int64_t C, CensusGeom* g, int64_t* bytes_part, int64_t* bytes_planes,
                     int64_t* bytes_prev) {
  const int64_t big = (int64_t)1 << 24;
  if (B <= 0 || T <= 0 || K <= 0 || C <= 0 || G < 1 || G > 4 || B >= big || T >= big) return false;
  int64_t rows = B * G, frames = 0, width = 0, elems = 0;
  if (__builtin_mul_overflow(rows, T, &frames) || frames >= big) return false;
  if (__builtin_mul_overflow(K, C, &width) || __builtin_mul_overflow(frames, width, &elems) || elems >= (int64_t)1 << 31) return false;
  g->B = (int)B;
  g->G = (int)G;
  g->T = (int)T;
  g->K = (int)K;
  g->C = (int)C;
  g->KC = width;
  g->PS = 3 * width + kPlanes * K;
  g->GS = g->PS + 2 + (kPlanes + 1) * T;
  g->staged = C <= kTile ? 1 : 0;
  g->single = (K <= kSpan && width <= kTile) ? 1 : 0;
  int64_t kc = g->staged ? kTile / C : kSpan;
  kc = kc > kSpan ? kSpan : kc;
  g->kc = (int)(kc > K ? K : kc);
  *bytes_part = rows * g->PS * (int64_t)sizeof(double);
  *bytes_planes = round8(kPlanes * frames * (int64_t)sizeof(float));
  *bytes_prev = round8(rows * K * (int64_t)sizeof(int32_t));
  return true;
}

}  // namespace

int64_t latent_census_workspace_bytes(int64_t B, int64_t G, int64_t T, int64_t K, int64_t C) {
  CensusGeom g;
  int64_t a = 0, b = 0, c = 0;
  if (!census_geometry(B, G, T, K, C, &g, &a, &b, &c)) return -1;
  return a + b + c;
}

int latent_census_launch(const float* post_logits, const float* prior_logits, const float* stoch, const int32_t* valid, int64_t B, int64_t G,
                         int64_t T, int64_t K, int64_t C, float* planes, double* table, void* workspace, int64_t workspace_bytes, hipStream_t st) {
  if (!post_logits || !prior_logits || !stoch || !table || !workspace) { set_error("latent_census: null pointer"); return MTRSSM_EINVAL; }
  CensusGeom g;
  int64_t bytes_part = 0, bytes_planes = 0, bytes_prev = 0;
  if (!census_geometry(B, G, T, K, C, &g, &bytes_part, &bytes_planes, &bytes_prev)) {
    set_error("latent_census: need B, T, K, C > 0, 1 <= G <= 4, B * G * T < 2^24 and B * G * T * K * C < 2^31 (got B %lld G %lld T %lld K %lld C %lld)",
              (long long)B, (long long)G, (long long)T, (long long)K, (long long)C);
    return MTRSSM_EINVAL;
  }
  if ((((uintptr_t)post_logits | (uintptr_t)prior_logits | (uintptr_t)stoch | (uintptr_t)valid | (uintptr_t)planes) & 3) ||
      (((uintptr_t)table | (uintptr_t)workspace) & 7)) {
    set_error("latent_census: buffers must be 4-byte aligned, the table and the workspace 8-byte");
    return MTRSSM_EINVAL;
  }
  if (workspace_bytes < bytes_part + bytes_planes + bytes_prev) {
    set_error("latent_census: the workspace has %lld bytes, mtrssm_latent_census_workspace_bytes asks for %lld", (long long)workspace_bytes,
              (long long)(bytes_part + bytes_planes + bytes_prev));
    return MTRSSM_EINVAL;
  }
  char* ws = static_cast<char*>(workspace);
  double* partials = reinterpret_cast<double*>(ws);
  float* out = planes ? planes : reinterpret_cast<float*>(ws + bytes_part);
  int32_t* prev = reinterpret_cast<int32_t*>(ws + bytes_part + bytes_planes);
  const int64_t rows = B * G, cells = (int64_t)g.G * g.GS;
  const int64_t fold_blocks = (cells + kFoldThreads - 1) / kFoldThreads;
  set_last_kernel("mtrssm::census_rows_kernel");
  hipLaunchKernelGGL(census_rows_kernel, dim3((unsigned)(rows < kMaxBlocks ? rows : kMaxBlocks)), dim3(kRowThreads), 0, st, post_logits, prior_logits,
                     stoch, valid, g, out, partials, prev);
  hipLaunchKernelGGL(census_fold_kernel, dim3((unsigned)(fold_blocks < kMaxBlocks ? fold_blocks : kMaxBlocks)), dim3(kFoldThreads), 0, st, partials,
                     out, valid, g, table);
  return check_launch("latent_census");
}

}  // namespace mtrssm
