// Latent overshooting for gfx950: the gather of the posterior states an episode's overshoot rows start from
// (with their action windows), its backward, and the categorical KL between the closed-loop posterior at frame t0 + k and the prior
// rolled k steps open loop from the posterior at t0, with its backward.  The KL kernels compute in double, reduce in a fixed order
// without atomics and round every output to fp32 once, so two calls agree bitwise; a row's outputs depend on that row only.
#include "scan_common.h"

namespace mtrssm {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kTile = 512;        // floats of each input a wave stages in LDS
constexpr int kFoldThreads = 1024;
constexpr int kMaxBlocks = 4096;

// Starts t0_i = o + i * s for i < N; overshoot row r = b * N + i; step j (0-based) of a row targets frame t = t0_i + j + 1 and is
// the k = j + 1 step prior.  The rank holds the rows row0 .. row0 + b_local - 1 of the b_global rows `valid` describes.
struct OsGeom {
  int b_global, row0, b_local, T, N, s, o, D, K, C;
};

__device__ __forceinline__ int row_length(const int32_t* __restrict__ valid, int b, int T) {
  if (!valid) return T;
  const int n = valid[b];
  return n < 0 ? 0 : (n > T ? T : n);
}

// Max and log-sum of one categorical's C logits at q (posterior) and p (prior), in double, classes in ascending order.
struct CatStats {
  double qm, ql, pm, pl;
};

__device__ __forceinline__ CatStats cat_stats(const float* q, const float* p, int C) {
  double qm = q[0], pm = p[0];
  for (int c = 1; c < C; ++c) {
    qm = fmax(qm, (double)q[c]);
    pm = fmax(pm, (double)p[c]);
  }
  double qs = 0.0, ps = 0.0;
  for (int c = 0; c < C; ++c) {
    qs += exp((double)q[c] - qm);
    ps += exp((double)p[c] - pm);
  }
  return {qm, log(qs), pm, log(ps)};
}

// sum_c q_c (lq_c - lp_c); a class with q_c = 0 adds 0; bitwise-equal q and p give exactly 0.
__device__ __forceinline__ double cat_kl(const float* q, const float* p, int C, const CatStats& st) {
  double kl = 0.0;
  for (int c = 0; c < C; ++c) {
    const double lq = ((double)q[c] - st.qm) - st.ql, lp = ((double)p[c] - st.pm) - st.pl;
    const double qq = exp(lq);
    if (qq > 0.0) kl += qq * (lq - lp);
  }
  return kl;
}

// One wave per term (r, j).  With C <= kTile (staged) the wave copies a span of kc categoricals of both rows into LDS with coalesced
// loads (lane i reads float i, i + 64, ...), then a lane owns one categorical of the span and lane 0 adds the span's KLs in ascending
// order; with C > kTile a lane reads its categorical from memory.  The trip counts depend on nothing but the launch's sizes, so the
// workgroup barriers are uniform.  plane [rows * D] fp32 and terms [rows * D] double are exactly 0 on a dead term.
__global__ __launch_bounds__(kThreads) void overshoot_kl_fwd_kernel(const float* __restrict__ post, const float* __restrict__ os,
                                                                    const int32_t* __restrict__ valid, const OsGeom g, int kc, int staged,
                                                                    float* __restrict__ plane, double* __restrict__ terms) {
  __shared__ float s_q[kWaves][kTile], s_p[kWaves][kTile];
  __shared__ double s_d[kWaves][kTile];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t S = (int64_t)g.K * g.C;
  const int64_t items = (int64_t)g.b_local * g.N * g.D;
  for (int64_t it0 = (int64_t)blockIdx.x * kWaves; it0 < items; it0 += (int64_t)gridDim.x * kWaves) {
    const int64_t item = it0 + wave;
    const bool in = item < items;
    const int64_t r = in ? item / g.D : 0;
    const int j = in ? (int)(item - r * g.D) : 0;
    const int bl = (int)(r / g.N), i = (int)(r - (int64_t)bl * g.N);
    const int64_t t = (int64_t)g.o + (int64_t)i * g.s + j + 1;
    const bool live = in && t < row_length(valid, g.row0 + bl, g.T);  // (wave-uniform; a live t is below T)
    double acc = 0.0;                                                   // (lane 0: the term's running sum)
    for (int k0 = 0; k0 < g.K; k0 += kc) {
      const int nk = g.K - k0 < kc ? g.K - k0 : kc;
      const float* qg = post + (live ? ((int64_t)bl * g.T + t) * S + (int64_t)k0 * g.C : 0);
      const float* pg = os + (live ? item * S + (int64_t)k0 * g.C : 0);
      if (staged && live)
        for (int x = lane; x < nk * g.C; x += kWave) {
          s_q[wave][x] = qg[x];
          s_p[wave][x] = pg[x];
        }
      __syncthreads();
      if (live)
        for (int c = lane; c < nk; c += kWave) {
          const float* q = staged ? &s_q[wave][c * g.C] : qg + (int64_t)c * g.C;
          const float* p = staged ? &s_p[wave][c * g.C] : pg + (int64_t)c * g.C;
          s_d[wave][c] = cat_kl(q, p, g.C, cat_stats(q, p, g.C));
        }
      __syncthreads();
      if (live && lane == 0)
        for (int c = 0; c < nk; ++c) acc += s_d[wave][c];
      __syncthreads();  // (the next span overwrites the staging buffers)
    }
    if (in && lane == 0) {
      plane[item] = live ? (float)acc : 0.f;
      terms[item] = live ? acc : 0.0;
    }
  }
}

// The fixed-order fold of one launch's terms: ONE workgroup; thread x owns a run of consecutive rows, adds it in ascending order,
// and the runs meet in a tree whose shape depends on nothing.  table [2][D]: per k the sum and the count of the rank's live terms;
// count: the live terms with k >= 2 of ALL b_global rows; term: the rank's sum over its live k >= 2 terms / max(count, 1).
__global__ __launch_bounds__(kFoldThreads) void overshoot_kl_fold_kernel(const double* __restrict__ terms, const int32_t* __restrict__ valid,
                                                                         const OsGeom g, double* __restrict__ table, float* __restrict__ count,
                                                                         float* __restrict__ term) {
  __shared__ double s_sum[kFoldThreads];
  __shared__ long long s_n[kFoldThreads];
  const int x = threadIdx.x;
  long long mine = 0;
  const int64_t starts = (int64_t)g.b_global * g.N;
  for (int64_t idx = x; idx < starts; idx += kFoldThreads) {
    const int b = (int)(idx / g.N), i = (int)(idx - (int64_t)b * g.N);
    int64_t m = (int64_t)row_length(valid, b, g.T) - 1 - ((int64_t)g.o + (int64_t)i * g.s);  // distances k with t0 + k < length
    m = m > g.D ? g.D : m;
    mine += m >= 2 ? m - 1 : 0;
  }
  s_n[x] = mine;
  __syncthreads();
  for (int w = kFoldThreads / 2; w > 0; w >>= 1) {
    if (x < w) s_n[x] += s_n[x + w];
    __syncthreads();
  }
  const long long total_n = s_n[0];
  __syncthreads();
  const int64_t rows = (int64_t)g.b_local * g.N;
  const int64_t run = (rows + kFoldThreads - 1) / kFoldThreads;
  const int64_t r0 = x * run < rows ? x * run : rows, r1 = r0 + run < rows ? r0 + run : rows;
  double total = 0.0;  // (thread 0: the k >= 2 sums in ascending k)
  for (int j = 0; j < g.D; ++j) {
    double sum = 0.0;
    long long n = 0;
    for (int64_t r = r0; r < r1; ++r) {
      const int bl = (int)(r / g.N), i = (int)(r - (int64_t)bl * g.N);
      const int64_t t = (int64_t)g.o + (int64_t)i * g.s + j + 1;
      if (t < row_length(valid, g.row0 + bl, g.T)) {
        sum += terms[r * g.D + j];
        ++n;
      }
    }
    s_sum[x] = sum;
    s_n[x] = n;
    __syncthreads();
    for (int w = kFoldThreads / 2; w > 0; w >>= 1) {
      if (x < w) {
        s_sum[x] += s_sum[x + w];
        s_n[x] += s_n[x + w];
      }
      __syncthreads();
    }
    if (x == 0) {
      table[j] = s_sum[0];
      table[g.D + j] = (double)s_n[0];
      if (j >= 1) total += s_sum[0];
    }
    __syncthreads();
  }
  if (x == 0) {
    count[0] = (float)total_n;
    term[0] = (float)(total / (total_n > 1 ? (double)total_n : 1.0));
  }
}

// The first blocks_os workgroups write g_os, a wave per term (r, j): scale * w_prior * (p - q) on a live k >= 2 term, 0 elsewhere.
// The others (launched only when g_post is given) write g_post, a wave per frame (b, t): the sum over the rows that target the frame,
// k = 2 .. D in ascending order, of scale * w_post * q_c ((lq_c - lp_c) - kl_cat), accumulated in double (staged) and rounded once.
// scale = g_term / max(count, 1), both read from device memory.  Staging and barriers as in the forward kernel.
__global__ __launch_bounds__(kThreads) void overshoot_kl_bwd_kernel(const float* __restrict__ post, const float* __restrict__ os,
                                                                    const int32_t* __restrict__ valid, const OsGeom g, int kc, int staged,
                                                                    const float* __restrict__ g_term, const float* __restrict__ count,
                                                                    double w_prior, double w_post, int blocks_os, float* __restrict__ g_os,
                                                                    float* __restrict__ g_post) {
  __shared__ float s_q[kWaves][kTile], s_p[kWaves][kTile];
  __shared__ double s_a[kWaves][kTile];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t S = (int64_t)g.K * g.C;
  const double cnt = (double)count[0];
  const double scale = (double)g_term[0] / (cnt > 1.0 ? cnt : 1.0);
  if ((int)blockIdx.x < blocks_os) {
    const int64_t items = (int64_t)g.b_local * g.N * g.D;
    for (int64_t it0 = (int64_t)blockIdx.x * kWaves; it0 < items; it0 += (int64_t)blocks_os * kWaves) {
      const int64_t item = it0 + wave;
      const bool in = item < items;
      const int64_t r = in ? item / g.D : 0;
      const int j = in ? (int)(item - r * g.D) : 0;
      const int bl = (int)(r / g.N), i = (int)(r - (int64_t)bl * g.N);
      const int64_t t = (int64_t)g.o + (int64_t)i * g.s + j + 1;
      const bool live = in && j >= 1 && t < row_length(valid, g.row0 + bl, g.T);
      const double f = scale * w_prior;
      for (int k0 = 0; k0 < g.K; k0 += kc) {
        const int nk = g.K - k0 < kc ? g.K - k0 : kc;
        const float* qg = post + (live ? ((int64_t)bl * g.T + t) * S + (int64_t)k0 * g.C : 0);
        const float* pg = os + (live ? item * S + (int64_t)k0 * g.C : 0);
        float* out = g_os + (in ? item * S + (int64_t)k0 * g.C : 0);
        if (staged && live)
          for (int x = lane; x < nk * g.C; x += kWave) {
            s_q[wave][x] = qg[x];
            s_p[wave][x] = pg[x];
          }
        __syncthreads();
        if (live)
          for (int c0 = lane; c0 < nk; c0 += kWave) {
            const float* q = staged ? &s_q[wave][c0 * g.C] : qg + (int64_t)c0 * g.C;
            const float* p = staged ? &s_p[wave][c0 * g.C] : pg + (int64_t)c0 * g.C;
            float* d = staged ? &s_p[wave][c0 * g.C] : out + (int64_t)c0 * g.C;  // (staged: over the lane's own categorical)
            const CatStats st = cat_stats(q, p, g.C);
            for (int c = 0; c < g.C; ++c) {
              const double qq = exp(((double)q[c] - st.qm) - st.ql), pp = exp(((double)p[c] - st.pm) - st.pl);
              d[c] = (float)(f * (pp - qq));
            }
          }
        __syncthreads();
        if (in && (staged || !live))
          for (int x = lane; x < nk * g.C; x += kWave) out[x] = live ? s_p[wave][x] : 0.f;
        __syncthreads();
      }
    }
    return;  // (uniform over the workgroup)
  }
  const int blocks_post = (int)gridDim.x - blocks_os;
  const int64_t frames = (int64_t)g.b_local * g.T;
  const double f = scale * w_post;
  for (int64_t it0 = (int64_t)((int)blockIdx.x - blocks_os) * kWaves; it0 < frames; it0 += (int64_t)blocks_post * kWaves) {
    const int64_t frame = it0 + wave;
    const bool in = frame < frames;
    const int bl = in ? (int)(frame / g.T) : 0, t = in ? (int)(frame - (int64_t)bl * g.T) : 0;
    const bool live = in && t < row_length(valid, g.row0 + bl, g.T);
    for (int k0 = 0; k0 < g.K; k0 += kc) {
      const int nk = g.K - k0 < kc ? g.K - k0 : kc;
      const float* qg = post + (in ? frame * S + (int64_t)k0 * g.C : 0);
      float* out = g_post + (in ? frame * S + (int64_t)k0 * g.C : 0);
      if (in)
        for (int x = lane; x < nk * g.C; x += kWave) {
          if (staged) {
            s_a[wave][x] = 0.0;
            if (live) s_q[wave][x] = qg[x];
          } else {
            out[x] = 0.f;
          }
        }
      __syncthreads();
      for (int k = 2; k <= g.D; ++k) {  // (uniform trip count)
        const int t0 = t - k;
        const bool hit = live && t0 >= g.o && (t0 - g.o) % g.s == 0 && (t0 - g.o) / g.s < g.N;
        const int64_t r = hit ? (int64_t)bl * g.N + (t0 - g.o) / g.s : 0;
        const float* pg = os + (hit ? (r * g.D + (k - 1)) * S + (int64_t)k0 * g.C : 0);
        if (staged && hit)
          for (int x = lane; x < nk * g.C; x += kWave) s_p[wave][x] = pg[x];
        __syncthreads();
        if (hit)
          for (int c0 = lane; c0 < nk; c0 += kWave) {
            const float* q = staged ? &s_q[wave][c0 * g.C] : qg + (int64_t)c0 * g.C;
            const float* p = staged ? &s_p[wave][c0 * g.C] : pg + (int64_t)c0 * g.C;
            const CatStats st = cat_stats(q, p, g.C);
            const double kl = cat_kl(q, p, g.C, st);
            for (int c = 0; c < g.C; ++c) {
              const double lq = ((double)q[c] - st.qm) - st.ql, lp = ((double)p[c] - st.pm) - st.pl;
              const double qq = exp(lq);
              const double add = qq > 0.0 ? f * qq * ((lq - lp) - kl) : 0.0;
              if (staged) s_a[wave][c0 * g.C + c] += add;
              else out[(int64_t)c0 * g.C + c] = (float)((double)out[(int64_t)c0 * g.C + c] + add);
            }
          }
        __syncthreads();
      }
      if (in && staged)
        for (int x = lane; x < nk * g.C; x += kWave) out[x] = (float)s_a[wave][x];
      __syncthreads();
    }
  }
}

// One launch for all tensors of a state and the action windows.  blockIdx.y = entry k < count: dst[k][b * N + i, :] =
// src[k][b, t0_i, :]; blockIdx.y = count: windows[b * N + i, j, :] = actions[b, t0_i + 1 + j, :], zeros past the last frame.
// 16-byte accesses for an entry whose width and pointers allow them, 4-byte ones otherwise.
struct OsRows {
  const float* src[MTRSSM_STATE_MAX + 1];
  float* dst[MTRSSM_STATE_MAX + 1];
  int width[MTRSSM_STATE_MAX + 1];
  int vec[MTRSSM_STATE_MAX + 1];
};

__global__ __launch_bounds__(kThreads) void overshoot_gather_kernel(const OsRows t, int count, long B, long T, long N, long s, long o, long D) {
  const int k = blockIdx.y;
  const float* __restrict__ src = t.src[k];
  float* __restrict__ dst = t.dst[k];
  const long w = t.width[k], per = t.vec[k] ? w / 4 : w;
  const long steps = k == count ? D : 1, total = B * N * steps * per;
  for (long x = (long)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (long)gridDim.x * blockDim.x) {
    const long q = x % per, row = x / per;  // row = r * steps + j
    const long r = row / steps, j = row - r * steps;
    const long b = r / N, i = r - b * N;
    const long from = o + i * s + (k == count ? 1 + j : 0);
    const bool have = from < T;
    if (t.vec[k]) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (have) v = reinterpret_cast<const float4*>(src + (b * T + from) * w)[q];
      reinterpret_cast<float4*>(dst + row * w)[q] = v;
    } else {
      dst[row * w + q] = have ? src[(b * T + from) * w + q] : 0.f;
    }
  }
}

// The gather's backward for the state tensors: g_src[k][b, t, :] = g_dst[k][b * N + i, :] where t = o + i * s with i < N, 0 elsewhere;
// every element of g_src is written exactly once.  (src = g_dst, dst = g_src in the table.)
__global__ __launch_bounds__(kThreads) void overshoot_scatter_kernel(const OsRows t, long B, long T, long N, long s, long o) {
  const int k = blockIdx.y;
  const float* __restrict__ src = t.src[k];
  float* __restrict__ dst = t.dst[k];
  const long w = t.width[k], per = t.vec[k] ? w / 4 : w;
  const long total = B * T * per;
  for (long x = (long)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (long)gridDim.x * blockDim.x) {
    const long q = x % per, frame = x / per;
    const long b = frame / T, tt = frame - b * T;
    const long rel = tt - o;
    const bool start = rel >= 0 && rel % s == 0 && rel / s < N;
    const long r = start ? b * N + rel / s : 0;
    if (t.vec[k]) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (start) v = reinterpret_cast<const float4*>(src + r * w)[q];
      reinterpret_cast<float4*>(dst + frame * w)[q] = v;
    } else {
      dst[frame * w + q] = start ? src[r * w + q] : 0.f;
    }
  }
}

// T >= 2, s >= 1, 0 <= o <= T - 2, N = (T - 2 - o) / s + 1, D >= 2: every start lies in [0, T - 2].
int check_starts(const char* what, int64_t B, int64_t T, int64_t N, int64_t s, int64_t o, int64_t D) {
  const int64_t big = (int64_t)1 << 24;
  if (B <= 0 || B >= big || T < 2 || T >= big || s < 1 || s >= big || o < 0 || o > T - 2 || D < 2 || D >= big || N != (T - 2 - o) / s + 1) {
    set_error("%s: need 0 < B < 2^24, 2 <= T < 2^24, 1 <= s, 0 <= o <= T - 2, 2 <= D < 2^24 and N = (T - 2 - o) / s + 1 "
              "(got B %lld T %lld N %lld s %lld o %lld D %lld)", what, (long long)B, (long long)T, (long long)N, (long long)s, (long long)o, (long long)D);
    return MTRSSM_EINVAL;
  }
  return MTRSSM_OK;
}

// The entries of `table` as the kernels take them; `big[k]` elements of the [B, T, W] side and `small[k]` of the [B * N, W] side
// must stay below 2^31.  swap: src is the [B * N, W] side (the scatter).
int fill_rows(const char* what, const MtrssmStateTable* table, int64_t B, int64_t T, int64_t N, bool swap, OsRows* rows, int64_t* most) {
  if (!table) { set_error("%s: null table", what); return MTRSSM_EINVAL; }
  if (table->count <= 0 || table->count > MTRSSM_STATE_MAX) {
    set_error("%s: count %d outside 1 .. %d", what, (int)table->count, MTRSSM_STATE_MAX);
    return MTRSSM_EINVAL;
  }
  for (int k = 0; k <= MTRSSM_STATE_MAX; ++k) {
    rows->src[k] = nullptr;
    rows->dst[k] = nullptr;
    rows->width[k] = rows->vec[k] = 0;
  }
  for (int k = 0; k < table->count; ++k) {
    const int64_t w = table->width[k];
    if (!table->src[k] || !table->dst[k] || w <= 0) { set_error("%s: entry %d has a null pointer or width <= 0", what, k); return MTRSSM_EINVAL; }
    if (table->src[k] == table->dst[k]) { set_error("%s: entry %d works in place (src == dst)", what, k); return MTRSSM_EINVAL; }
    int64_t frames = 0, elems = 0;
    if (__builtin_mul_overflow(B, T > N ? T : N, &frames) || __builtin_mul_overflow(frames, w, &elems) || elems >= (int64_t)1 << 31) {
      set_error("%s: entry %d has B * max(T, N) * width >= 2^31", what, k);
      return MTRSSM_EINVAL;
    }
    if (((uintptr_t)table->src[k] | (uintptr_t)table->dst[k]) & 3) { set_error("%s: entry %d is not 4-byte aligned", what, k); return MTRSSM_EINVAL; }
    rows->src[k] = table->src[k];
    rows->dst[k] = table->dst[k];
    rows->width[k] = (int)w;
    rows->vec[k] = (w % 4 == 0 && !(((uintptr_t)table->src[k] | (uintptr_t)table->dst[k]) & 15)) ? 1 : 0;
    const int64_t items = B * (swap ? T : N) * (rows->vec[k] ? w / 4 : w);
    *most = items > *most ? items : *most;
  }
  return MTRSSM_OK;
}

int kl_geometry(const char* what, int64_t b_global, int64_t row0, int64_t b_local, int64_t T, int64_t N, int64_t s, int64_t o, int64_t D,
                int64_t K, int64_t C, OsGeom* g, int* kc, int* staged) {
  const int rc = check_starts(what, b_local, T, N, s, o, D);
  if (rc != MTRSSM_OK) return rc;
  if (b_global <= 0 || b_global >= (int64_t)1 << 24 || row0 < 0 || row0 + b_local > b_global) {
    set_error("%s: the rank's rows %lld .. %lld must lie inside the %lld global rows (below 2^24)", what, (long long)row0,
              (long long)(row0 + b_local - 1), (long long)b_global);
    return MTRSSM_EINVAL;
  }
  if (K <= 0 || C <= 0) { set_error("%s: need K, C > 0 (got %lld %lld)", what, (long long)K, (long long)C); return MTRSSM_EINVAL; }
  int64_t width = 0, rows = 0, steps = 0, a = 0, b = 0, c = 0;
  if (__builtin_mul_overflow(K, C, &width) || __builtin_mul_overflow(b_local, N, &rows) || __builtin_mul_overflow(rows, D, &steps) ||
      __builtin_mul_overflow(steps, width, &a) || __builtin_mul_overflow(b_local * T, width, &b) || __builtin_mul_overflow(b_global, N, &c) ||
      a >= (int64_t)1 << 31 || b >= (int64_t)1 << 31 || c >= (int64_t)1 << 31) {
    set_error("%s: B * N * D * K * C, B * T * K * C and B_global * N must stay below 2^31", what);
    return MTRSSM_EINVAL;
  }
  *g = OsGeom{(int)b_global, (int)row0, (int)b_local, (int)T, (int)N, (int)s, (int)o, (int)D, (int)K, (int)C};
  *staged = C <= kTile ? 1 : 0;
  *kc = *staged ? (int)(kTile / C) : kWave;
  if (*kc > K) *kc = (int)K;
  return MTRSSM_OK;
}

int blocks_for(int64_t items) {
  const int64_t want = (items + kWaves - 1) / kWaves;
  return (int)(want < kMaxBlocks ? (want < 1 ? 1 : want) : kMaxBlocks);
}

}  // namespace

int overshoot_gather_launch(const MtrssmStateTable* table, const float* actions, float* windows, int64_t B, int64_t T, int64_t N, int64_t s,
                            int64_t o, int64_t D, int64_t A, hipStream_t st) {
  int rc = check_starts("overshoot_gather", B, T, N, s, o, D);
  if (rc != MTRSSM_OK) return rc;
  if (!actions || !windows || A <= 0 || (((uintptr_t)actions | (uintptr_t)windows) & 3) || (const float*)windows == actions) {
    set_error("overshoot_gather: actions / windows null, aliased or not 4-byte aligned, or A <= 0");
    return MTRSSM_EINVAL;
  }
  int64_t rows = B * N, a = 0, b = 0;
  if (__builtin_mul_overflow(rows * D, A, &a) || __builtin_mul_overflow(B * T, A, &b) || a >= (int64_t)1 << 31 || b >= (int64_t)1 << 31) {
    set_error("overshoot_gather: B * N * D * A and B * T * A must stay below 2^31");
    return MTRSSM_EINVAL;
  }
  OsRows pr;
  int64_t most = 0;
  rc = fill_rows("overshoot_gather", table, B, T, N, false, &pr, &most);
  if (rc != MTRSSM_OK) return rc;
  const int k = table->count;
  pr.src[k] = actions;
  pr.dst[k] = windows;
  pr.width[k] = (int)A;
  pr.vec[k] = (A % 4 == 0 && !(((uintptr_t)actions | (uintptr_t)windows) & 15)) ? 1 : 0;
  const int64_t items = rows * D * (pr.vec[k] ? A / 4 : A);
  most = items > most ? items : most;
  const int64_t want = (most + kThreads - 1) / kThreads;
  set_last_kernel("mtrssm::overshoot_gather_kernel");
  hipLaunchKernelGGL(overshoot_gather_kernel, dim3((unsigned)(want < 256 ? want : 256), k + 1), dim3(kThreads), 0, st, pr, k, (long)B, (long)T,
                     (long)N, (long)s, (long)o, (long)D);
  return check_launch("overshoot_gather");
}

int overshoot_scatter_launch(const MtrssmStateTable* table, int64_t B, int64_t T, int64_t N, int64_t s, int64_t o, hipStream_t st) {
  int rc = check_starts("overshoot_scatter", B, T, N, s, o, 2);
  if (rc != MTRSSM_OK) return rc;
  OsRows pr;
  int64_t most = 0;
  rc = fill_rows("overshoot_scatter", table, B, T, N, true, &pr, &most);
  if (rc != MTRSSM_OK) return rc;
  const int64_t want = (most + kThreads - 1) / kThreads;
  set_last_kernel("mtrssm::overshoot_scatter_kernel");
  hipLaunchKernelGGL(overshoot_scatter_kernel, dim3((unsigned)(want < 256 ? want : 256), table->count), dim3(kThreads), 0, st, pr, (long)B, (long)T,
                     (long)N, (long)s, (long)o);
  return check_launch("overshoot_scatter");
}

int64_t overshoot_kl_workspace_bytes(int64_t b_local, int64_t N, int64_t D) {
  int64_t rows = 0, terms = 0;
  if (b_local <= 0 || N <= 0 || D < 2 || __builtin_mul_overflow(b_local, N, &rows) || __builtin_mul_overflow(rows, D, &terms) ||
      terms >= (int64_t)1 << 31)
    return -1;
  return terms * (int64_t)sizeof(double);
}

int overshoot_kl_fwd_launch(const float* post_logits, const float* os_logits, const int32_t* valid, int64_t b_global, int64_t row0,
                            int64_t b_local, int64_t T, int64_t N, int64_t s, int64_t o, int64_t D, int64_t K, int64_t C, float* plane,
                            double* table, float* count, float* term, void* workspace, int64_t workspace_bytes, hipStream_t st) {
  if (!post_logits || !os_logits || !plane || !table || !count || !term || !workspace) { set_error("overshoot_kl_fwd: null pointer"); return MTRSSM_EINVAL; }
  OsGeom g;
  int kc = 0, staged = 0;
  const int rc = kl_geometry("overshoot_kl_fwd", b_global, row0, b_local, T, N, s, o, D, K, C, &g, &kc, &staged);
  if (rc != MTRSSM_OK) return rc;
  if ((((uintptr_t)post_logits | (uintptr_t)os_logits | (uintptr_t)valid | (uintptr_t)plane | (uintptr_t)count | (uintptr_t)term) & 3) ||
      (((uintptr_t)table | (uintptr_t)workspace) & 7)) {
    set_error("overshoot_kl_fwd: buffers must be 4-byte aligned, the table and the workspace 8-byte");
    return MTRSSM_EINVAL;
  }
  if (workspace_bytes < overshoot_kl_workspace_bytes(b_local, N, D)) {
    set_error("overshoot_kl_fwd: the workspace has %lld bytes, mtrssm_overshoot_kl_workspace_bytes asks for %lld", (long long)workspace_bytes,
              (long long)overshoot_kl_workspace_bytes(b_local, N, D));
    return MTRSSM_EINVAL;
  }
  double* terms = static_cast<double*>(workspace);
  set_last_kernel("mtrssm::overshoot_kl_fwd_kernel");
  hipLaunchKernelGGL(overshoot_kl_fwd_kernel, dim3((unsigned)blocks_for(b_local * N * D)), dim3(kThreads), 0, st, post_logits, os_logits, valid, g, kc,
                     staged, plane, terms);
  hipLaunchKernelGGL(overshoot_kl_fold_kernel, dim3(1), dim3(kFoldThreads), 0, st, terms, valid, g, table, count, term);
  return check_launch("overshoot_kl_fwd");
}

int overshoot_kl_bwd_launch(const float* post_logits, const float* os_logits, const int32_t* valid, const float* g_term, const float* count,
                            int64_t b_global, int64_t row0, int64_t b_local, int64_t T, int64_t N, int64_t s, int64_t o, int64_t D, int64_t K,
                            int64_t C, float w_prior, float w_post, float* g_os_logits, float* g_post_logits, hipStream_t st) {
  if (!post_logits || !os_logits || !g_term || !count || !g_os_logits) { set_error("overshoot_kl_bwd: null pointer"); return MTRSSM_EINVAL; }
  OsGeom g;
  int kc = 0, staged = 0;
  const int rc = kl_geometry("overshoot_kl_bwd", b_global, row0, b_local, T, N, s, o, D, K, C, &g, &kc, &staged);
  if (rc != MTRSSM_OK) return rc;
  if (!(w_prior >= 0.f) || !(w_post >= 0.f) || (w_post == 0.f) != (g_post_logits == nullptr)) {
    set_error("overshoot_kl_bwd: need w_prior, w_post >= 0 and g_post_logits exactly when w_post > 0 (got %g %g)", (double)w_prior, (double)w_post);
    return MTRSSM_EINVAL;
  }
  if (((uintptr_t)post_logits | (uintptr_t)os_logits | (uintptr_t)valid | (uintptr_t)g_term | (uintptr_t)count | (uintptr_t)g_os_logits |
       (uintptr_t)g_post_logits) & 3) {
    set_error("overshoot_kl_bwd: buffers must be 4-byte aligned");
    return MTRSSM_EINVAL;
  }
  if (g_os_logits == os_logits || g_os_logits == post_logits || g_post_logits == post_logits || g_post_logits == os_logits ||
      g_post_logits == g_os_logits) {
    set_error("overshoot_kl_bwd: a gradient buffer aliases an input or the other gradient");
    return MTRSSM_EINVAL;
  }
  const int blocks_os = blocks_for(b_local * N * D), blocks_post = g_post_logits ? blocks_for(b_local * T) : 0;
  set_last_kernel("mtrssm::overshoot_kl_bwd_kernel");
  hipLaunchKernelGGL(overshoot_kl_bwd_kernel, dim3((unsigned)(blocks_os + blocks_post)), dim3(kThreads), 0, st, post_logits, os_logits, valid, g, kc,
                     staged, g_term, count, (double)w_prior, (double)w_post, blocks_os, g_os_logits, g_post_logits);
  return check_launch("overshoot_kl_bwd");
}

}  // namespace mtrssm
