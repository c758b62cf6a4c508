// Linear word probes on latent features for gfx950: one fused step of G multinomial-logistic classifiers over
// N feature rows -- logits, log-softmax loss, arg-max and the weight / bias gradients -- in one pass over the features.  A tile of 16
// rows is staged in LDS once and serves both contractions on v_mfma_f32_16x16x4_f32 (fp32 operands, fp32 accumulation: a k-ordered
// fmaf chain); logits and probabilities live in registers and LDS only.  Workgroup partials go to the workspace and a second small
// kernel adds them in a fixed order (no atomics); the grid depends on the shapes alone, so two calls agree bitwise.
#include "scan_common.h"

namespace mtrssm {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kRows = 16;          // rows of a tile: the M (logits) / K (gradient) extent of four 16x16x4 MFMAs
constexpr int kClasses = 16;       // classes are padded to the MFMA's 16-wide tile
constexpr int kPad = kClasses + 1; // row stride of the small LDS arrays
constexpr int kMaxF = 2048;        // 16 rows of F floats must fit the CU's LDS, a wave's share of W and dW its registers
constexpr int kMaxPartials = 256;  // workgroups (= partial sets) per group at most
constexpr int kMinTiles = 2;       // tiles a workgroup walks at least (when there are that many)

using f32x4 = __attribute__((ext_vector_type(4))) float;

struct ProbeArgs {
  const float* x;
  int64_t ld, col0;
  const int32_t* labels;
  const float* weight;
  const float* bias;
  int N, C, F, stride, P, tiles_per;
  float* part;        // [G][P][C * F + C]
  double* stat_part;  // [G][P][3]
  float* nll;
  float* hit;
  int32_t* pred;
};

// The partial sets of one group: P workgroups of tiles_per consecutive 16-row tiles each.  A function of N alone.
__host__ __device__ inline void probe_split(int64_t N, int* P, int* tiles_per) {
  const int64_t tiles = (N + kRows - 1) / kRows;
  int64_t per = (tiles + kMaxPartials - 1) / kMaxPartials;
  if (per < kMinTiles) per = kMinTiles;
  if (per > tiles) per = tiles;
  *tiles_per = (int)per;
  *P = (int)((tiles + per - 1) / per);
}

// LDS row stride of the staged tile: >= F rounded up to 16 (the gradient's last 16-column tile stays inside the row) and = 17 mod 32,
// which spreads both operand patterns (16 rows x 4 columns for the logits, 4 rows x 16 columns for the gradient) over the banks.
inline int probe_stride(int F) {
  int s = (F + 15) / 16 * 16;
  while (s % 32 != 17) ++s;
  return s;
}

// Reductions over a 16-lane DPP row (every lane of the row gets the result, bitwise the same: each step combines two values that the
// partner lane combines in the other order).  All 64 lanes must be active.
template <int CTRL>
__device__ __forceinline__ int dpp_move(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) { return __int_as_float(dpp_move<CTRL>(__float_as_int(v))); }
#define MTRSSM_PROBE_ROW_REDUCE(name, type, op)                  \
  __device__ __forceinline__ type name(type v) {                 \
    v = op(v, dpp_move<0xB1>(v));  /* quad_perm [1, 0, 3, 2] */  \
    v = op(v, dpp_move<0x4E>(v));  /* quad_perm [2, 3, 0, 1] */  \
    v = op(v, dpp_move<0x141>(v)); /* row_half_mirror */         \
    v = op(v, dpp_move<0x140>(v)); /* row_mirror */              \
    return v;                                                    \
  }
__device__ __forceinline__ float op_add(float a, float b) { return a + b; }
__device__ __forceinline__ int op_min(int a, int b) { return a < b ? a : b; }
MTRSSM_PROBE_ROW_REDUCE(row_max, float, fmaxf)
MTRSSM_PROBE_ROW_REDUCE(row_sum, float, op_add)
MTRSSM_PROBE_ROW_REDUCE(row_min, int, op_min)
#undef MTRSSM_PROBE_ROW_REDUCE

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// Workgroup (p, g) walks its tiles of group g.  TPW: 16-column gradient tiles a wave owns at most (tile j * 4 + wave), and a quarter
// of the k-steps (4 features each) it owns of the logits (step j * 4 + wave), so F <= 64 * TPW.
//   stage     wave w copies rows 4w .. 4w + 3 of the tile through registers (coalesced; a dead or out-of-range row is not read, its
//             LDS row is 0)
//   logits    every wave multiplies all 16 rows by ITS k-steps of W (held in registers as the B operand), the four partial tiles
//             meet in LDS and thread (row, class) adds them in a fixed order
//   softmax   across the 16 lanes of a row (butterflies); loss, arg-max (lowest index), p - onehot -> LDS
//   gradient  dW[class][f] += sum_rows d[row][class] x[row][f]: A = d (4 rows per MFMA), B = the staged tile, accumulators in
//             registers over all of the workgroup's tiles
template <int TPW, bool GRAD>
__global__ __launch_bounds__(kThreads, TPW <= 4 ? 3 : 1) void linear_probe_kernel(ProbeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [kRows][stride]
  __shared__ float s_z[kWaves][kRows][kPad];
  __shared__ float s_d[kRows][kPad];
  __shared__ double s_stat[kRows][3];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int lrow = lane & 15, lgrp = lane >> 4;
  const int g = blockIdx.y, p = blockIdx.x;
  const int N = a.N, C = a.C, F = a.F, stride = a.stride;
  const int nsteps = (F + 3) >> 2, ntiles = (F + 15) >> 4;
  const int row = tid >> 4, cls = tid & 15;  // the (row, class) this thread owns in the softmax

  // this wave's k-steps of W as the logits' B operand: B[k = lane >> 4][class = lane & 15]
  float wreg[4 * TPW];
  const float* wg = a.weight + (int64_t)g * C * F;
#pragma unroll
  for (int j = 0; j < 4 * TPW; ++j) {
    const int f = 4 * (4 * j + wave) + lgrp;
    wreg[j] = (lrow < C && f < F) ? wg[(int64_t)lrow * F + f] : 0.f;
  }
  const float bias = cls < C ? a.bias[g * C + cls] : 0.f;
  for (int i = tid; i < kRows * (stride - F); i += kThreads) xs[(i / (stride - F)) * stride + F + i % (stride - F)] = 0.f;  // the rows' padding

  const int tiles = (N + kRows - 1) / kRows;
  const int t0 = p * a.tiles_per, t1 = t0 + a.tiles_per < tiles ? t0 + a.tiles_per : tiles;
  double sum_nll = 0.0, sum_hit = 0.0, sum_live = 0.0;
  float g_b = 0.f;
  f32x4 acc[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Staging goes through registers: all of a lane's loads of a tile (its wave's 4 rows, TPW floats of each) are in flight together.
  // kPrefetch: the NEXT tile is requested right after the barrier that publishes this one, so its latency hides behind the MFMAs;
  // at large F the registers go to W and dW instead and the rows are fetched one at a time.
  constexpr bool kPrefetch = TPW <= 4;
  constexpr int kHeld = kPrefetch ? kRows / kWaves : 1;
  float held[kHeld][TPW];
  // A lane carries the label of row 4 * wave + (lane >> 4) of a tile: its own row in the softmax, and (read across the wave) the four
  // rows its wave stages.  Labels run two tiles ahead of the arithmetic, the features one, so no load is waited for where it is issued.
  auto load_label = [&](int t) {
    const int n = t * kRows + wave * (kRows / kWaves) + lgrp;
    return (t < t1 && n < N) ? a.labels[n] : -1;
  };
  auto fetch = [&](int t, int r, int lab_lane, float (&v)[TPW]) {
    const int n = t * kRows + wave * (kRows / kWaves) + r;
    const int lab = __builtin_amdgcn_readlane(lab_lane, 16 * r);
    const bool live = lab >= 0 && lab < C;  // (wave-uniform)
    const float* src = a.x + ((int64_t)g * N + (live ? n : 0)) * a.ld + a.col0;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      const int f = lane + kWave * i;
      v[i] = (live && f < F) ? src[f] : 0.f;
    }
  };
  auto put = [&](int r, const float (&v)[TPW]) {
    float* dst = xs + (wave * (kRows / kWaves) + r) * stride;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      const int f = lane + kWave * i;
      if (f < F) dst[f] = v[i];
    }
  };
  int lab_cur = load_label(t0), lab_next = load_label(t0 + 1);
  if (kPrefetch && t0 < t1) {
#pragma unroll
    for (int r = 0; r < kHeld; ++r) fetch(t0, r, lab_cur, held[r]);
  }

  for (int t = t0; t < t1; ++t) {
    const int n0 = t * kRows;
    if (kPrefetch) {
#pragma unroll
      for (int r = 0; r < kHeld; ++r) put(r, held[r]);
    } else {
#pragma unroll 1
      for (int r = 0; r < kRows / kWaves; ++r) {
        fetch(t, r, lab_cur, held[0]);
        put(r, held[0]);
      }
    }
    __syncthreads();
    if (kPrefetch && t + 1 < t1) {
#pragma unroll
      for (int r = 0; r < kHeld; ++r) fetch(t + 1, r, lab_next, held[r]);
    }
    const int lab_after = load_label(t + 2);

    // logits: A[row = lane & 15][k = lane >> 4] from LDS, two accumulators so that consecutive MFMAs are independent
    f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
    const float* xa = xs + lrow * stride + lgrp;
#pragma unroll
    for (int j = 0; j < 4 * TPW; ++j) {
      const int s = 4 * j + wave;
      if (s < nsteps) {
        if (j & 1) z1 = mfma4(xa[4 * s], wreg[j], z1);
        else z0 = mfma4(xa[4 * s], wreg[j], z0);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s_z[wave][lgrp * 4 + i][lrow] = z0[i] + z1[i];  // D[row = (lane >> 4) * 4 + i][class = lane & 15]
    __syncthreads();

    const int n = n0 + row;
    const int lab = lab_cur;
    const bool live = lab >= 0 && lab < C;
    lab_cur = lab_next;
    lab_next = lab_after;
    float z = ((s_z[0][row][cls] + s_z[1][row][cls]) + (s_z[2][row][cls] + s_z[3][row][cls])) + bias;
    if (cls >= C) z = -INFINITY;
    const float m = row_max(z);
    const int best = row_min((z == m && cls < C) ? cls : kClasses);
    const float e = expf(z - m);
    const float se = row_sum(e);
    const float z_label = __shfl(z, live ? lab : 0, kClasses);
    const float nll = (m + logf(se)) - z_label;
    const float d = live ? e / se - (cls == lab ? 1.f : 0.f) : 0.f;
    if (cls == 0 && n < N) {
      const int64_t o = (int64_t)g * N + n;
      if (a.nll) a.nll[o] = live ? nll : 0.f;
      if (a.hit) a.hit[o] = live && best == lab ? 1.f : 0.f;
      if (a.pred) a.pred[o] = live ? best : -1;
      if (live) {
        sum_nll += (double)nll;
        sum_hit += best == lab ? 1.0 : 0.0;
        sum_live += 1.0;
      }
    }
    if (GRAD) {
      s_d[row][cls] = d;
      g_b += d;
      __syncthreads();
#pragma unroll 1
      for (int k = 0; k < 4; ++k) {  // (not unrolled: four operand loads in flight at a time keep the registers for a third wave)
        const float da = s_d[4 * k + lgrp][lrow];                   // A[class = lane & 15][k = row = lane >> 4]
        const float* xb = xs + (4 * k + lgrp) * stride + lrow;      // B[k = row = lane >> 4][f = lane & 15]
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
          const int tile = 4 * j + wave;
          if (tile < ntiles) acc[j] = mfma4(da, xb[16 * tile], acc[j]);
        }
      }
      __syncthreads();  // (the next tile overwrites xs and s_d)
    }
  }

  const int64_t slot = (int64_t)g * a.P + p;
  if (GRAD) {
    float* out = a.part + slot * ((int64_t)C * F + C);
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const int f = 16 * (4 * j + wave) + lrow;
      if (4 * j + wave < ntiles && f < F) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (lgrp * 4 + i < C) out[(int64_t)(lgrp * 4 + i) * F + f] = acc[j][i];  // D[class = (lane >> 4) * 4 + i][f]
      }
    }
    s_d[row][cls] = g_b;
  }
  if (cls == 0) {
    s_stat[row][0] = sum_nll;
    s_stat[row][1] = sum_hit;
    s_stat[row][2] = sum_live;
  }
  __syncthreads();
  if (GRAD && tid < C) {
    float total = 0.f;
    for (int r = 0; r < kRows; ++r) total += s_d[r][tid];
    a.part[slot * ((int64_t)C * F + C) + (int64_t)C * F + tid] = total;
  }
  if (tid < 3) {
    double total = 0.0;
    for (int r = 0; r < kRows; ++r) total += s_stat[r][tid];
    a.stat_part[slot * 3 + tid] = total;
  }
}

constexpr int kRedElems = 32;                     // gradient elements a reducer workgroup owns (128 contiguous bytes per partial set)
constexpr int kRedChunks = kThreads / kRedElems;  // runs of partial sets added side by side

// Element e of group g's gradient = its P partials added in a FIXED order: kRedChunks consecutive runs of partial sets, each added
// in ascending p by one thread (eight loads in flight, the adds in order), then the runs' sums in ascending order (normalize: divided
// by max(count, 1)).  The three stats sums: partial set p goes to slot p of an LDS array, which is folded in halves (slot i += slot
// i + h, h = 128 .. 1), in double -- a tree whose shape is fixed, so the sum depends on the values alone.  The first workgroup writes them.
__global__ __launch_bounds__(kThreads) void linear_probe_reduce_kernel(const float* __restrict__ part, const double* __restrict__ stat_part, int P,
                                                                       int C, int F, int normalize, float* __restrict__ g_weight,
                                                                       float* __restrict__ g_bias, float* __restrict__ stats) {
  static_assert(kMaxPartials <= kThreads, "one thread per partial set in the stats tree");
  __shared__ float s_run[kRedChunks][kRedElems];
  __shared__ double s_st[kThreads][3];
  const int tid = threadIdx.x, g = blockIdx.y, lane = tid % kRedElems, run = tid / kRedElems;
  const int64_t E = (int64_t)C * F + C, e = (int64_t)blockIdx.x * kRedElems + lane;
  const double* sp = stat_part + ((int64_t)g * P + tid) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) s_st[tid][k] = tid < P ? sp[k] : 0.0;
  float total = 0.f;
  if (g_weight && e < E) {
    const int per = (P + kRedChunks - 1) / kRedChunks;
    const int p0 = run * per, p1 = p0 + per < P ? p0 + per : P;
    const float* src = part + (int64_t)g * P * E + e;
    int p = p0;
    for (; p + 8 <= p1; p += 8) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = src[(int64_t)(p + i) * E];
#pragma unroll
      for (int i = 0; i < 8; ++i) total += v[i];
    }
    for (; p < p1; ++p) total += src[(int64_t)p * E];
  }
  s_run[run][lane] = total;
  __syncthreads();
  for (int h = kThreads / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s_st[tid][k] += s_st[tid + h][k];
    }
    __syncthreads();
  }
  const double live = s_st[0][2];
  if (blockIdx.x == 0 && tid < 3) stats[g * 3 + tid] = (float)s_st[0][tid];
  if (!g_weight || run != 0 || e >= E) return;
  total = s_run[0][lane];
#pragma unroll
  for (int r = 1; r < kRedChunks; ++r) total += s_run[r][lane];
  if (normalize) total /= (float)(live > 1.0 ? live : 1.0);
  if (e < (int64_t)C * F) g_weight[(int64_t)g * C * F + e] = total;
  else g_bias[(int64_t)g * C + (e - (int64_t)C * F)] = total;
}

bool sizes_ok(int64_t G, int64_t N, int64_t C, int64_t F) {
  return G >= 1 && N >= 1 && N < ((int64_t)1 << 24) && C >= 2 && C <= kClasses && F >= 1 && F <= kMaxF && G < ((int64_t)1 << 31);
}

int64_t workspace_bytes(int64_t G, int64_t N, int64_t C, int64_t F) {
  int P = 0, per = 0;
  probe_split(N, &P, &per);
  return G * P * (3 * (int64_t)sizeof(double) + (C * F + C) * (int64_t)sizeof(float));
}

template <int TPW, bool GRAD>
int launch(const ProbeArgs& a, int64_t G, hipStream_t s) {
  const size_t lds = (size_t)kRows * a.stride * sizeof(float);
  auto* fn = linear_probe_kernel<TPW, GRAD>;
  if (lds > 32768) {  // (static LDS comes on top: stay clear of the 64 KiB a kernel gets without asking)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { set_error("linear_probe_step: hipFuncSetAttribute(max dynamic LDS=%zu): %s", lds, hipGetErrorString(e)); return MTRSSM_ELAUNCH; }
  }
  hipLaunchKernelGGL(fn, dim3((unsigned)a.P, (unsigned)G), dim3(kThreads), lds, s, a);
  return MTRSSM_OK;
}

}  // namespace

int64_t linear_probe_workspace_bytes(int64_t G, int64_t N, int64_t C, int64_t F) {
  if (!sizes_ok(G, N, C, F)) {
    set_error("linear_probe_workspace_bytes: need G >= 1, 1 <= N < 2^24, 2 <= C <= %d, 1 <= F <= %d (got %lld %lld %lld %lld)", kClasses, kMaxF,
              (long long)G, (long long)N, (long long)C, (long long)F);
    return MTRSSM_EINVAL;
  }
  return workspace_bytes(G, N, C, F);
}

int linear_probe_step_launch(const float* x, int64_t ld, int64_t col0, const int32_t* labels, const float* weight, const float* bias, int64_t G,
                             int64_t N, int64_t C, int64_t F, int normalize, float* g_weight, float* g_bias, float* stats, float* nll, float* hit,
                             int32_t* pred, void* workspace, int64_t workspace_bytes_given, hipStream_t s) {
  if (!x || !labels || !weight || !bias || !stats || !workspace) { set_error("linear_probe_step: null pointer"); return MTRSSM_EINVAL; }
  if ((g_weight == nullptr) != (g_bias == nullptr)) {
    set_error("linear_probe_step: give g_weight and g_bias, or neither (evaluation only)");
    return MTRSSM_EINVAL;
  }
  if (!sizes_ok(G, N, C, F)) {
    set_error("linear_probe_step: need G >= 1, 1 <= N < 2^24, 2 <= C <= %d, 1 <= F <= %d (got %lld %lld %lld %lld)", kClasses, kMaxF, (long long)G,
              (long long)N, (long long)C, (long long)F);
    return MTRSSM_EINVAL;
  }
  int64_t rows = 0, elems = 0;
  if (col0 < 0 || ld < 1 || col0 > ld - F || __builtin_mul_overflow(G, N, &rows) || __builtin_mul_overflow(rows, ld, &elems) ||
      elems >= (int64_t)1 << 31) {
    set_error("linear_probe_step: need 0 <= col0, col0 + F <= ld and G * N * ld < 2^31 (got col0 %lld F %lld ld %lld G %lld N %lld)", (long long)col0,
              (long long)F, (long long)ld, (long long)G, (long long)N);
    return MTRSSM_EINVAL;
  }
  if (normalize != 0 && normalize != 1) { set_error("linear_probe_step: normalize is 0 or 1 (got %d)", normalize); return MTRSSM_EINVAL; }
  const int64_t need = workspace_bytes(G, N, C, F);
  if (workspace_bytes_given < need) {
    set_error("linear_probe_step: the workspace holds %lld bytes, %lld are needed", (long long)workspace_bytes_given, (long long)need);
    return MTRSSM_EINVAL;
  }
  if ((((uintptr_t)x | (uintptr_t)labels | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)g_weight | (uintptr_t)g_bias | (uintptr_t)stats |
        (uintptr_t)nll | (uintptr_t)hit | (uintptr_t)pred) & 3) || ((uintptr_t)workspace & 7)) {
    set_error("linear_probe_step: buffers must be 4-byte aligned, the workspace 8-byte aligned");
    return MTRSSM_EINVAL;
  }
  ProbeArgs a;
  a.x = x; a.ld = ld; a.col0 = col0; a.labels = labels; a.weight = weight; a.bias = bias;
  a.N = (int)N; a.C = (int)C; a.F = (int)F; a.stride = probe_stride((int)F);
  probe_split(N, &a.P, &a.tiles_per);
  a.stat_part = static_cast<double*>(workspace);
  a.part = reinterpret_cast<float*>(a.stat_part + G * a.P * 3);
  a.nll = nll; a.hit = hit; a.pred = pred;
  const bool grad = g_weight != nullptr;
  int rc;
  if (F <= 256) rc = grad ? launch<4, true>(a, G, s) : launch<4, false>(a, G, s);
  else if (F <= 1280) rc = grad ? launch<20, true>(a, G, s) : launch<20, false>(a, G, s);
  else rc = grad ? launch<32, true>(a, G, s) : launch<32, false>(a, G, s);
  if (rc != MTRSSM_OK) return rc;
  set_last_kernel(grad ? "mtrssm::linear_probe_kernel<grad>" : "mtrssm::linear_probe_kernel<eval>");
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("linear_probe_step launch failed: %s", hipGetErrorString(e)); return MTRSSM_ELAUNCH; }
  const int64_t E = C * F + C;
  hipLaunchKernelGGL(linear_probe_reduce_kernel, dim3((unsigned)(grad ? (E + kRedElems - 1) / kRedElems : 1), (unsigned)G), dim3(kThreads), 0, s, a.part,
                     a.stat_part, a.P, (int)C, (int)F, normalize, g_weight, g_bias, stats);
  e = hipGetLastError();
  if (e != hipSuccess) { set_error("linear_probe_step reduce launch failed: %s", hipGetErrorString(e)); return MTRSSM_ELAUNCH; }
  return MTRSSM_OK;
}

}  // namespace mtrssm
