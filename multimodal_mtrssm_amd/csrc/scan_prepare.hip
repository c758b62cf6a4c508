// The weight layouts of the cooperative MRSSM scans (mrssm_cluster.hip, mrssm_wide.hip) in ONE launch: the three transposes
//   w1s_t [S][H]  = w1[:, A:]^T,   whh_t [D][3D] = whh^T,   wh1_t [D][3H] = [w3 ; wa1[:, :D] ; wv1[:, :D]]^T
// and the fused GRU input path
//   wf_t [H][3D],  wf_t[k][j] = sum_h W2[h][k] W_ih[j][h]          bf [3D],  bf[j] = sum_h b2[h] W_ih[j][h] + b_ih[j]
// straight from the raw parameters (each with its leading dimension: they are views of a flat parameter buffer) into one
// caller-owned buffer.  The parameters change every optimizer step, so this runs every step: before, it was three torch copies,
// a cat and two latency-bound GEMMs (six launches, 52 us at the base dims, for half a megabyte of output).
//
// One grid of independent 32 x 32 tiles, 256 threads each; no workgroup waits for another.  A transpose tile goes through a
// padded LDS tile (coalesced reads along the source row, coalesced writes along the destination row) and is exact.  A product
// tile walks h in ascending order, 64 at a time (the next chunk's loads are in flight while the current one is summed): every
// output element is ONE fp32 fma chain acc = fma(W2[h][k], W_ih[j][h], acc) over h = 0 .. H-1 starting from zero -- the
// arithmetic of mtrssm_gemm when it does not split its reduction.  b2 rides along as row k = H of the left operand, so bf is the
// same chain, with b_ih[j] added last.
#include "scan_common.h"

namespace mtrssm {

constexpr int kPrepTile = 32;    // output tile edge
constexpr int kPrepChunk = 64;   // h values per staged chunk of a product tile
constexpr int kPrepThreads = 256;
constexpr int kPrepSegs = 5;
constexpr int kPrepAlign = 64;   // floats: every output starts on a 256-byte boundary of the buffer

// dst[c * ld_dst + col_off + r] = src[r * ld_src + c]   for r < rows, c < cols
struct PrepSeg {
  const float* src;
  float* dst;
  int rows, cols, ld_src, ld_dst, col_off, tiles_c;
};

struct PrepArgs {
  PrepSeg seg[kPrepSegs];
  int first[kPrepSegs + 2];   // first block of every segment, then of the product, then the grid size
  const float *w2, *b2, *wih, *bih;
  float *wf_t, *bf;
  int H, D3, ld_w2, ld_wih, tiles_j;
};

__device__ __forceinline__ void transpose_tile(const PrepSeg& s, int tile, float (*t)[kPrepTile + 1]) {
  const int r0 = (tile / s.tiles_c) * kPrepTile, c0 = (tile % s.tiles_c) * kPrepTile;
  const int tx = threadIdx.x & (kPrepTile - 1), ty = threadIdx.x / kPrepTile;   // ty: 0 .. 7
#pragma unroll
  for (int i = 0; i < kPrepTile; i += kPrepThreads / kPrepTile) {
    const int r = r0 + ty + i, c = c0 + tx;
    if (r < s.rows && c < s.cols) t[ty + i][tx] = s.src[(size_t)r * s.ld_src + c];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kPrepTile; i += kPrepThreads / kPrepTile) {
    const int c = c0 + ty + i, r = r0 + tx;
    if (r < s.rows && c < s.cols) s.dst[(size_t)c * s.ld_dst + s.col_off + r] = t[tx][ty + i];
  }
}

__global__ __launch_bounds__(kPrepThreads) void scan_prepare_kernel(const PrepArgs p) {
  __shared__ float a_s[kPrepChunk][kPrepTile];          // [h][k]: W2 (row k = H: b2)
  __shared__ float b_s[kPrepTile][kPrepChunk + 1];      // [j][h]: W_ih
  const int block = blockIdx.x;
  if (block < p.first[kPrepSegs]) {
    int s = 0;
    while (block >= p.first[s + 1]) ++s;
    transpose_tile(p.seg[s], block - p.first[s], reinterpret_cast<float(*)[kPrepTile + 1]>(&b_s[0][0]));
    return;
  }
  const int tile = block - p.first[kPrepSegs];
  const int k0 = (tile / p.tiles_j) * kPrepTile, j0 = (tile % p.tiles_j) * kPrepTile;
  const int tid = threadIdx.x;
  const int H = p.H;
  // staging: W2 rows are read along k (32 lanes per row, 8 rows per pass), W_ih rows along h (64 lanes per row, 4 rows per pass)
  const int ak = tid & (kPrepTile - 1), ah = tid / kPrepTile;
  const int bh = tid & (kPrepChunk - 1), bj = tid / kPrepChunk;
  float ra[8], rb[8];
  auto load = [&](int h0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int h = h0 + ah + 8 * i, k = k0 + ak;
      float v = 0.f;
      if (h < H) {
        if (k < H) v = p.w2[(size_t)h * p.ld_w2 + k];
        else if (k == H) v = p.b2[h];
      }
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = j0 + bj + 4 * i, h = h0 + bh;
      rb[i] = (j < p.D3 && h < H) ? p.wih[(size_t)j * p.ld_wih + h] : 0.f;
    }
  };
  // compute: lanes run along j (coalesced stores of wf_t rows), every thread holds four k rows
  const int tj = tid & (kPrepTile - 1), tk = tid / kPrepTile;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  load(0);
  for (int h0 = 0; h0 < H; h0 += kPrepChunk) {
#pragma unroll
    for (int i = 0; i < 8; ++i) a_s[ah + 8 * i][ak] = ra[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) b_s[bj + 4 * i][bh] = rb[i];
    __syncthreads();
    if (h0 + kPrepChunk < H) load(h0 + kPrepChunk);
    const int hn = H - h0 < kPrepChunk ? H - h0 : kPrepChunk;
    for (int h = 0; h < hn; ++h) {
      const float b = b_s[tj][h];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = fmaf(a_s[h][tk + 8 * i], b, acc[i]);
    }
    __syncthreads();
  }
  const int j = j0 + tj;
  if (j >= p.D3) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = k0 + tk + 8 * i;
    if (k < H) p.wf_t[(size_t)k * p.D3 + j] = acc[i];
    else if (k == H) p.bf[j] = acc[i] + p.bih[j];
  }
}

static int64_t round_up(int64_t n) { return (n + kPrepAlign - 1) / kPrepAlign * kPrepAlign; }

// Offsets (in floats) of w1s_t, whh_t, wh1_t, wf_t, bf inside the buffer; returns the buffer's size in floats, 0 for bad dims.
int64_t mrssm_scan_prepare_layout(int D, int H, int S, int64_t* offsets) {
  if (D <= 0 || H <= 0 || S <= 0 || D > (1 << 14) || H > (1 << 14) || S > (1 << 14)) return 0;
  const int64_t sizes[5] = {(int64_t)S * H, (int64_t)D * 3 * D, (int64_t)D * 3 * H, (int64_t)H * 3 * D, (int64_t)3 * D};
  int64_t at = 0;
  for (int i = 0; i < 5; ++i) {
    if (offsets) offsets[i] = at;
    at += round_up(sizes[i]);
  }
  return at;
}

int mrssm_scan_prepare_launch(const MtrssmScanPrepare* q, hipStream_t stream) {
  if (!q || !q->w1 || !q->whh || !q->w3 || !q->wa1 || !q->wv1 || !q->out) { set_error("mrssm_scan_prepare: null pointer"); return MTRSSM_EINVAL; }
  if (q->product && (!q->w2 || !q->b2 || !q->wih || !q->bih)) { set_error("mrssm_scan_prepare: the fused input path needs w2, b2, wih, bih (null)"); return MTRSSM_EINVAL; }
  int64_t off[5];
  const int64_t need = mrssm_scan_prepare_layout(q->D, q->H, q->S, off);
  if (need == 0 || q->A < 0) { set_error("mrssm_scan_prepare: need 0 < D, H, S <= 16384 and A >= 0 (got %d %d %d %d)", q->D, q->H, q->S, q->A); return MTRSSM_EINVAL; }
  if (q->out_floats < need) { set_error("mrssm_scan_prepare: the buffer holds %lld floats, the layouts take %lld", (long long)q->out_floats, (long long)need); return MTRSSM_EINVAL; }
  const int D = q->D, H = q->H, S = q->S;
  if (q->ld_w1 < q->A + S || q->ld_whh < D || q->ld_w3 < D || q->ld_wa1 < D || q->ld_wv1 < D || (q->product && (q->ld_w2 < H || q->ld_wih < H))) {
    set_error("mrssm_scan_prepare: a leading dimension is smaller than the row it is read along");
    return MTRSSM_EINVAL;
  }
  PrepArgs p;
  auto tiles = [](int n) { return (n + kPrepTile - 1) / kPrepTile; };
  auto seg = [&](int i, const float* src, float* dst, int rows, int cols, int ld_src, int ld_dst, int col_off) {
    p.seg[i] = PrepSeg{src, dst, rows, cols, ld_src, ld_dst, col_off, tiles(cols)};
    p.first[i + 1] = p.first[i] + tiles(rows) * tiles(cols);
  };
  p.first[0] = 0;
  seg(0, q->w1 + q->A, q->out + off[0], H, S, q->ld_w1, H, 0);
  seg(1, q->whh, q->out + off[1], 3 * D, D, q->ld_whh, 3 * D, 0);
  seg(2, q->w3, q->out + off[2], H, D, q->ld_w3, 3 * H, 0);
  seg(3, q->wa1, q->out + off[2], H, D, q->ld_wa1, 3 * H, H);
  seg(4, q->wv1, q->out + off[2], H, D, q->ld_wv1, 3 * H, 2 * H);
  p.w2 = q->w2; p.b2 = q->b2; p.wih = q->wih; p.bih = q->bih;
  p.wf_t = q->out + off[3]; p.bf = q->out + off[4];
  p.H = H; p.D3 = 3 * D; p.ld_w2 = q->ld_w2; p.ld_wih = q->ld_wih; p.tiles_j = tiles(3 * D);
  p.first[kPrepSegs + 1] = p.first[kPrepSegs] + (q->product ? tiles(H + 1) * p.tiles_j : 0);   // (+ 1: the b2 row)
  set_last_kernel("mtrssm::scan_prepare_kernel");
  hipLaunchKernelGGL(scan_prepare_kernel, dim3((unsigned)p.first[kPrepSegs + 1]), dim3(kPrepThreads), 0, stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("mrssm_scan_prepare launch failed: %s", hipGetErrorString(e)); return MTRSSM_ELAUNCH; }
  return MTRSSM_OK;
}

}  // namespace mtrssm
