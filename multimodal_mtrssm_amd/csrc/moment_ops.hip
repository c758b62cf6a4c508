// Feature moments by bin for gfx950: per bin j the count, the sum and the full second-moment matrix of the fp32
// feature rows x[n] with bin[n] == j, accumulated in double onto a table.  Two launches, no atomics, no double copy of the features
// and no gather per bin; every product x_ni * x_nj is formed in double (exact: 24 + 24 bits) on v_mfma_f64_16x16x4_f64, the
// contraction runs over rows, and the order of addition depends on (N, D, J) alone, so two calls agree bitwise.
#include "scan_common.h"

namespace mtrssm {

namespace {

constexpr int kTileDim = 16;     // a tile of the second moment: one MFMA accumulator
constexpr int kTileCells = 256;  // doubles a wave writes per tile and bin
constexpr int kSteps = 8;        // MFMA steps (of 4 rows) whose operands a lane holds at a time
constexpr int kSlices = 16;      // row slices: every (tile, slice) pair is one wave
constexpr int kFoldThreads = 256;
constexpr int kMaxD = 256, kMaxJ = 16;

typedef double double4_t __attribute__((ext_vector_type(4)));

// DT = ceil(D / 16) tile strips; the tiles of a slice are the P = DT (DT + 1) / 2 pairs (it <= jt) of the second moment, in
// ascending (it, jt), then DT "sum tiles" whose A operand is a row of ones.  S slices of `rows` rows each.
struct MomentGeom {
  int64_t N, ldx;
  int D, J, DT, P, S;
  int64_t rows;
};

__host__ __device__ __forceinline__ int pair_index(int it, int jt, int DT) { return it * DT - it * (it - 1) / 2 + (jt - it); }

// One wave per (tile, slice).  Lane l feeds the MFMA of rows n0 .. n0 + 3 with A = x[n0 + (l >> 4)][i0 + (l & 15)] and
// B = x[n0 + (l >> 4)][j0 + (l & 15)]: it loads exactly the two floats it feeds (16 consecutive floats of a row per 16 lanes), so
// no LDS stage is needed -- the operands of kSteps steps are loaded ahead into registers while the previous kSteps are multiplied.
// Bins by masking: for bin j both operands of a lane whose row is in another bin are 0, so a row adds to its own bin only (a NaN
// row stays in its bin); a bin none of the step's four rows has is skipped, which changes nothing (it would add exact zeros).
// A row past the slice and a bin outside [0, J) count as bin -1; nothing out of bounds is touched (see the loads below).
// The f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg.  A sum tile (tile >= P) has A = 1 in row 0: row 0 of its result is
// the column sums of strip jt; its first wave (jt = 0) also counts the rows per bin.
template <int JMAX>
__global__ __launch_bounds__(kWave) void moment_tiles_kernel(const float* __restrict__ x, const int32_t* __restrict__ bin, const MomentGeom g,
                                                             double* __restrict__ partials, double* __restrict__ counts) {
  const int lane = threadIdx.x, sub = lane >> 4, col = lane & 15;
  const int tile = blockIdx.x, slice = blockIdx.y;
  const bool ones = tile >= g.P;
  int it = 0, jt = 0;
  if (ones) {
    jt = tile - g.P;
  } else {
    int rest = tile;
    while (rest >= g.DT - it) {
      rest -= g.DT - it;
      ++it;
    }
    jt = it + rest;
  }
  const int ca = it * kTileDim + col, cb = jt * kTileDim + col;
  const bool in_a = ca < g.D, in_b = cb < g.D;
  const int64_t n_begin = (int64_t)slice * g.rows;
  const int64_t n_end = n_begin + g.rows < g.N ? n_begin + g.rows : g.N;

  double4_t acc[JMAX];
  int cnt[JMAX];
#pragma unroll
  for (int j = 0; j < JMAX; ++j) {
    acc[j] = double4_t{0.0, 0.0, 0.0, 0.0};
    cnt[j] = 0;
  }

  float va[kSteps], vb[kSteps], na[kSteps], nb[kSteps];
  int vbin[kSteps], nbin[kSteps];
  const unsigned stride = 4u * (unsigned)g.ldx, bins = (unsigned)g.J;  // (N * ldx < 2^31: a live row's offsets fit 32 bits)
  // Every load is unconditional and its value is used as it comes, so a batch's loads are all in flight together.  A dead row
  // reads the slice's last row and gets bin -1 (the bin mask drops it); a column past D reads column 0 and only fills cells of the
  // tile with a row or column index >= D, which the fold never reads (a cell of an MFMA result depends on its own row of A and
  // column of B alone).  Both addresses are in bounds.
  const int64_t n_last = n_end - 1;
  const unsigned at_last = (unsigned)n_last * (unsigned)g.ldx, cca = in_a ? ca : 0, ccb = in_b ? cb : 0;
  const float one = col == 0 ? 1.f : 0.f;
  auto load = [&](int64_t c0, float* a, float* b, int* bn) {
    const int64_t n0 = c0 + sub;
    const unsigned base = (unsigned)n0 * (unsigned)g.ldx;
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
      const int64_t n = n0 + 4 * k;
      const bool live = n < n_end;
      const unsigned at = live ? base + k * stride : at_last;
      const int v = bin[live ? n : n_last];
      bn[k] = ((unsigned)v < bins ? v : -1) | (live ? 0 : -1);
      a[k] = ones ? one : x[at + cca];
      b[k] = x[at + ccb];
    }
  };
  if (n_begin < n_end) load(n_begin, va, vb, vbin);
  for (int64_t c0 = n_begin; c0 < n_end; c0 += 4 * kSteps) {
    const bool more = c0 + 4 * kSteps < n_end;
    if (more) load(c0 + 4 * kSteps, na, nb, nbin);
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
      const double a = (double)va[k], b = (double)vb[k];
      const int mine = vbin[k];
#pragma unroll
      for (int j = 0; j < JMAX; ++j) {
        const bool hit = mine == j;
        const unsigned long long any = __ballot(hit);
        if (any) {
          acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(hit ? a : 0.0, hit ? b : 0.0, acc[j], 0, 0, 0);
          cnt[j] += __popcll(any & 0x0001000100010001ull);  // (lane 0 of each of the step's four rows)
        }
      }
    }
    if (more) {
#pragma unroll
      for (int k = 0; k < kSteps; ++k) {
        va[k] = na[k];
        vb[k] = nb[k];
        vbin[k] = nbin[k];
      }
    }
  }

  const int tiles = g.P + g.DT;
#pragma unroll
  for (int j = 0; j < JMAX; ++j) {
    if (j < g.J) {
      double* out = partials + (((int64_t)slice * g.J + j) * tiles + tile) * kTileCells;
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(sub + 4 * r) * kTileDim + col] = acc[j][r];
      if (tile == g.P && lane == 0) counts[(int64_t)slice * g.J + j] = (double)cnt[j];
    }
  }
}

// One thread per cell of the table [J][1 + D + D * D]: the call's sum is a left fold from +0 over the slices in ascending order,
// added once onto what the cell holds.  Cell (i, j) of the second moment with tile(i) > tile(j) reads the mirrored cell of tile
// (tile(j), tile(i)), and inside a diagonal tile the cell with i > j reads (j, i): both triangles are the same doubles.
__global__ __launch_bounds__(kFoldThreads) void moment_fold_kernel(const double* __restrict__ partials, const double* __restrict__ counts,
                                                                   const MomentGeom g, double* __restrict__ table) {
  const int64_t per = 1 + (int64_t)g.D + (int64_t)g.D * g.D, cells = per * g.J;
  const int tiles = g.P + g.DT;
  for (int64_t c = (int64_t)blockIdx.x * kFoldThreads + threadIdx.x; c < cells; c += (int64_t)gridDim.x * kFoldThreads) {
    const int j = (int)(c / per);
    const int64_t cell = c - (int64_t)j * per;
    double v = 0.0;
    if (cell == 0) {
      for (int s = 0; s < g.S; ++s) v += counts[(int64_t)s * g.J + j];
    } else {
      int tile, at;
      if (cell <= g.D) {
        const int i = (int)(cell - 1);
        tile = g.P + i / kTileDim;
        at = i % kTileDim;  // (row 0 of the sum tile)
      } else {
        const int64_t y = cell - 1 - g.D;
        int r = (int)(y / g.D), q = (int)(y - (int64_t)r * g.D);
        if (r > q) {
          const int keep = r;
          r = q;
          q = keep;
        }
        tile = pair_index(r / kTileDim, q / kTileDim, g.DT);
        at = (r % kTileDim) * kTileDim + q % kTileDim;
      }
      for (int s = 0; s < g.S; ++s) v += partials[(((int64_t)s * g.J + j) * tiles + tile) * kTileCells + at];
    }
    table[c] += v;
  }
}

bool moment_geometry(int64_t N, int64_t ldx, int D, int J, MomentGeom* g) {
  if (N < 1 || N >= (int64_t)1 << 31 || D < 1 || D > kMaxD || J < 1 || J > kMaxJ) return false;
  g->N = N;
  g->ldx = ldx;
  g->D = D;
  g->J = J;
  g->DT = (D + kTileDim - 1) / kTileDim;
  g->P = g->DT * (g->DT + 1) / 2;
  const int64_t groups = (N + 4 * kSteps - 1) / (4 * kSteps);
  g->S = (int)(groups < kSlices ? groups : kSlices);
  g->rows = (N + g->S - 1) / g->S;
  return true;
}

int64_t moment_bytes(const MomentGeom& g) { return (int64_t)sizeof(double) * g.S * g.J * ((int64_t)(g.P + g.DT) * kTileCells + 1); }

template <int JMAX>
void launch_tiles(const float* x, const int32_t* bin, const MomentGeom& g, double* partials, double* counts, hipStream_t st) {
  hipLaunchKernelGGL(moment_tiles_kernel<JMAX>, dim3((unsigned)(g.P + g.DT), (unsigned)g.S), dim3(kWave), 0, st, x, bin, g, partials, counts);
}

}  // namespace

int64_t feature_moments_workspace_bytes(int64_t N, int D, int J) {
  MomentGeom g;
  if (!moment_geometry(N, D, D, J, &g)) return -1;
  return moment_bytes(g);
}

int feature_moments_launch(const float* x, int64_t ldx, const int32_t* bin, int64_t N, int D, int J, double* table, void* workspace,
                           int64_t workspace_bytes, hipStream_t st) {
  if (!x || !bin || !table || !workspace) { set_error("feature_moments: null pointer"); return MTRSSM_EINVAL; }
  MomentGeom g;
  int64_t elems = 0;
  if (!moment_geometry(N, ldx, D, J, &g) || ldx < 1 || __builtin_mul_overflow(N, ldx, &elems) || elems >= (int64_t)1 << 31) {
    set_error("feature_moments: need N >= 1, 1 <= D <= 256, 1 <= J <= 16 and N * ldx < 2^31 (got N %lld D %d J %d ldx %lld)", (long long)N, D, J,
              (long long)ldx);
    return MTRSSM_EINVAL;
  }
  if (ldx < D) {
    set_error("feature_moments: ldx %lld is smaller than D %d", (long long)ldx, D);
    return MTRSSM_EINVAL;
  }
  if ((((uintptr_t)x | (uintptr_t)bin) & 3) || (((uintptr_t)table | (uintptr_t)workspace) & 7)) {
    set_error("feature_moments: x and bin must be 4-byte aligned, the table and the workspace 8-byte");
    return MTRSSM_EINVAL;
  }
  const int64_t need = moment_bytes(g);
  if (workspace_bytes < need) {
    set_error("feature_moments: the workspace has %lld bytes, mtrssm_feature_moments_workspace_bytes asks for %lld", (long long)workspace_bytes,
              (long long)need);
    return MTRSSM_EINVAL;
  }
  double* partials = static_cast<double*>(workspace);
  double* counts = partials + (int64_t)g.S * g.J * (g.P + g.DT) * kTileCells;
  set_last_kernel("mtrssm::moment_tiles_kernel");
  if (J <= 1) launch_tiles<1>(x, bin, g, partials, counts, st);
  else if (J <= 2) launch_tiles<2>(x, bin, g, partials, counts, st);
  else if (J <= 4) launch_tiles<4>(x, bin, g, partials, counts, st);
  else if (J <= 8) launch_tiles<8>(x, bin, g, partials, counts, st);
  else launch_tiles<16>(x, bin, g, partials, counts, st);
  const int64_t cells = (int64_t)J * (1 + (int64_t)D + (int64_t)D * D);
  const int64_t blocks = (cells + kFoldThreads - 1) / kFoldThreads;
  hipLaunchKernelGGL(moment_fold_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kFoldThreads), 0, st, partials, counts, g, table);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("feature_moments launch failed: %s", hipGetErrorString(e));
    return MTRSSM_ELAUNCH;
  }
  return MTRSSM_OK;
}

}  // namespace mtrssm
