// Digit reader for gfx950: the inference path of the small CNN that reads a digit off a predicted vision
// frame -- conv 1->32, ReLU, pool, conv 32->64, ReLU, pool as ONE launch (digit_features_kernel), the 128->10 head with its
// arg-max (digit_head_kernel) and the (word, digit) count table (word_counts_kernel).  fc1 (4096->128) runs on mtrssm_gemm.
//
// digit_features_kernel: persistent workgroups of four waves (one per SIMD, 512 registers per lane) walk the frames.  A frame's
// 4 KB are requested one frame ahead; activation, denormalisation and clamp are applied while the frame is written into a haloed
// 34 x 34 fp32 image in LDS.  conv1 runs on the VALU (K = 9): thread = one pooled pixel, its 4 x 4 input patch in registers, per
// channel the four conv outputs of the pool window, their maximum, + bias, ReLU, split into two bf16 pieces and written into the
// haloed channel-innermost image [piece][18 x 18 positions][32 channels] (80-byte rows: conv_resident.h's layout).  conv2 is an
// implicit GEMM on v_mfma_f32_32x32x16_bf16: M = 64 output channels (two tiles), N = 256 pixels, K = 288 = 9 taps x 2 blocks of
// 16 channels; wave = (channel tile, half of the pooled rows).  A wave's four accumulators are the four members of the 2 x 2 pool
// window: column il of accumulator q = (dy, dx) is conv2's pixel (2 py + dy, 2 px + dx) of pooled pixel il = (py, px), so the
// second pool is a maximum over the SAME register of four accumulators and a lane's 16 results are 16 channels of one pooled
// pixel -- stored as 128-byte runs in the view(-1, 4096) order.  The 16 image positions (dy + ty, dx + tx) a lane needs are
// read once per channel block (32 ds_read_b128) and serve all 36 (window member, tap) pairs.  The A operands (both pieces of
// 32 output channels x 288) stay in registers for the whole launch.  Arithmetic: bf16x2 -- p0 q0 + p0 q1 + p1 q0, fp32 sums.
// The same kernel with TAPE set is the training forward (section 6m, mtrssm_digit_features_train): identical features, plus one byte
// per pooled unit naming the window member that held the maximum; csrc/digit_train.hip has the backward that reads it.
#include "scan_common.h"

namespace mtrssm {

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

constexpr int kThreads = 256;
constexpr int kPix = 1024;             // 32 x 32 input pixels
constexpr int kC1 = 32, kC2 = 64;      // channels after conv1 / conv2
constexpr int kFeat = kC2 * 64;        // 4096
constexpr int kTape = kC1 * 256 + kFeat;  // bytes of a frame's tape: conv1's pooled units, then conv2's in the feature order
constexpr int kXW = 34;                // haloed input row
constexpr int kPW = 18;                // haloed pooled row
constexpr int kRowB = kC1 * 2 + 16;    // bytes per image row: one position, 32 bf16 channels, padded to an odd number of 16-byte slots
constexpr int kImgB = kPW * kPW * kRowB;  // one piece: 25 920 bytes
constexpr int kW1Row = 12;             // conv1 weights in LDS: [32][9 taps, bias, 2 pad]
constexpr int kClasses = 10, kHidden = 128, kBins = 11;

__device__ __forceinline__ void split2(float x, unsigned short& hi, unsigned short& lo) {
  const __bf16 h = (__bf16)x;
  hi = __builtin_bit_cast(unsigned short, h);
  const __bf16 l = (__bf16)(x - (float)h);  // (the difference is exact in fp32)
  lo = __builtin_bit_cast(unsigned short, l);
}

// TAPE (the training forward, section 6m): the same arithmetic, plus one byte per pooled unit -- the member 2 dy + dx of its 2 x 2
// window that holds the maximum (the first among equal maxima: a strict > over members 0 .. 3), 4 when max + bias <= 0.
template <bool TANH, bool TAPE>
__global__ __launch_bounds__(kThreads, 1) void digit_features_kernel(const float* __restrict__ pred, int64_t frames,
                                                                     const int32_t* __restrict__ select, int N,
                                                                     const float* __restrict__ w1, const float* __restrict__ b1,
                                                                     const float* __restrict__ w2, const float* __restrict__ b2,
                                                                     float* __restrict__ features, unsigned char* __restrict__ tape) {
  __shared__ __attribute__((aligned(16))) float xin[kXW * kXW];
  __shared__ __attribute__((aligned(16))) float w1s[kC1 * kW1Row];
  __shared__ __attribute__((aligned(16))) unsigned char img[2 * kImgB];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kl = lane >> 5, il = lane & 31;
  const int ct = wave & 1, ph = wave >> 1;

  // ---- once per workgroup: zero the images (the halos stay zero), conv1's weights, this wave's conv2 A operands
  for (int i = tid; i < kXW * kXW; i += kThreads) xin[i] = 0.f;
  for (int o = tid * 16; o < 2 * kImgB; o += kThreads * 16) *reinterpret_cast<u32x4*>(img + o) = u32x4{0u, 0u, 0u, 0u};
  for (int i = tid; i < kC1 * kW1Row; i += kThreads) {
    const int c = i / kW1Row, j = i - c * kW1Row;
    w1s[i] = j < 9 ? w1[c * 9 + j] : (j == 9 ? b1[c] : 0.f);
  }
  // a[t][cb][piece]: row = output channel ct * 32 + il, k = input channels cb * 16 + 8 * kl + (0 .. 7) at tap t
  bf16x8 a[9][2][2];
  {
    const float* wrow = w2 + (size_t)(ct * 32 + il) * kC1 * 9;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        unsigned hi[4], lo[4];
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
          unsigned short h0, l0, h1, l1;
          const int ci = cb * 16 + 8 * kl + 2 * e2;
          split2(wrow[ci * 9 + t], h0, l0);
          split2(wrow[(ci + 1) * 9 + t], h1, l1);
          hi[e2] = (unsigned)h0 | ((unsigned)h1 << 16);
          lo[e2] = (unsigned)l0 | ((unsigned)l1 << 16);
        }
        a[t][cb][0] = __builtin_bit_cast(bf16x8, u32x4{hi[0], hi[1], hi[2], hi[3]});
        a[t][cb][1] = __builtin_bit_cast(bf16x8, u32x4{lo[0], lo[1], lo[2], lo[3]});
      }
  }
  // this lane's 16 accumulator rows are output channels cbase + (r & 3) + 8 * (r >> 2)
  const int cbase = ct * 32 + 4 * kl;
  float bv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) bv[r] = b2[cbase + (r & 3) + 8 * (r >> 2)];

  // staging: thread = four consecutive pixels of row tid / 8
  const int sy = tid >> 3, sx = (tid & 7) * 4;
  // conv1: thread = pooled pixel (py1, px1) of the 16 x 16 plane
  const int py1 = tid >> 4, px1 = tid & 15;
  // conv2: lane il = pooled pixel (py2, px2) of the 8 x 8 plane; byte offset of image position (2 py2, 2 px2), channel 8 * kl
  const int py2 = 4 * ph + (il >> 3), px2 = il & 7;
  const unsigned char* bbase = img + ((2 * py2) * kPW + 2 * px2) * kRowB + kl * 16;

  auto frame_of = [&](int n, bool& bad) -> const float4* {
    int64_t src = select ? (int64_t)select[n] : (int64_t)n;
    bad = src < 0 || src >= frames;
    if (bad) src = 0;  // (nothing out of bounds is read; the frame's features are NaN)
    return reinterpret_cast<const float4*>(pred + src * kPix) + tid;
  };
  int n = blockIdx.x;
  bool bad = false, bad_next = false;
  float4 cur = float4{0.f, 0.f, 0.f, 0.f}, nxt = cur;
  if (n < N) cur = *frame_of(n, bad);
  __syncthreads();  // zero fill and weights are in place

  for (; n < N; n += gridDim.x) {
    const int nn = n + (int)gridDim.x;
    if (nn < N) nxt = *frame_of(nn, bad_next);  // in flight under this frame's two convolutions
    {
      float v[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float y = v[j];
        if (TANH) y = tanh_fast(y);
        y = (y + 1.f) * 0.5f;
        y = y < 0.f ? 0.f : y;  // (a NaN goes through both selects)
        y = y > 1.f ? 1.f : y;
        xin[(sy + 1) * kXW + sx + 1 + j] = y;
      }
    }
    __syncthreads();  // the input image is complete; every wave is done with the previous frame's pooled image
    // ---- conv1 + bias + ReLU + 2 x 2 max pool -> bf16 pieces, eight channels per 16-byte store
    {
      float p[4][4];
#pragma unroll
      for (int dy = 0; dy < 4; ++dy)
#pragma unroll
        for (int dx = 0; dx < 4; ++dx) p[dy][dx] = xin[(2 * py1 + dy) * kXW + 2 * px1 + dx];
      unsigned char* dst = img + ((py1 + 1) * kPW + px1 + 1) * kRowB;
#pragma unroll
      for (int c8 = 0; c8 < 4; ++c8) {
        unsigned hi[4], lo[4];
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
          unsigned short h[2], l[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int c = c8 * 8 + e2 * 2 + u;
            const float4 wa = *reinterpret_cast<const float4*>(w1s + c * kW1Row);
            const float4 wb = *reinterpret_cast<const float4*>(w1s + c * kW1Row + 4);
            const float4 wc = *reinterpret_cast<const float4*>(w1s + c * kW1Row + 8);
            const float w[9] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w, wc.x};
            float best = 0.f;
            int arg = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int dy = q >> 1, dx = q & 1;
              float s = 0.f;
#pragma unroll
              for (int t = 0; t < 9; ++t) s = fmaf(w[t], p[dy + t / 3][dx + t % 3], s);
              if (TAPE && q > 0 && s > best) arg = q;
              best = q == 0 ? s : fmaxf(best, s);
            }
            best += wc.y;  // bias
            if (TAPE) tape[(size_t)n * kTape + c * 256 + tid] = (unsigned char)(best <= 0.f ? 4 : arg);
            best = best > 0.f ? best : 0.f;
            split2(best, h[u], l[u]);
          }
          hi[e2] = (unsigned)h[0] | ((unsigned)h[1] << 16);
          lo[e2] = (unsigned)l[0] | ((unsigned)l[1] << 16);
        }
        *reinterpret_cast<u32x4*>(dst + c8 * 16) = u32x4{hi[0], hi[1], hi[2], hi[3]};
        *reinterpret_cast<u32x4*>(dst + kImgB + c8 * 16) = u32x4{lo[0], lo[1], lo[2], lo[3]};
      }
    }
    __syncthreads();  // the pooled image is complete; every wave is done with the input image
    // ---- conv2: four accumulators = the four members of the pool window
    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      bf16x8 fr[16][2];
#pragma unroll
      for (int pa = 0; pa < 4; ++pa)
#pragma unroll
        for (int pb = 0; pb < 4; ++pb)
#pragma unroll
          for (int s = 0; s < 2; ++s)
            fr[pa * 4 + pb][s] = *reinterpret_cast<const bf16x8*>(bbase + s * kImgB + (pa * kPW + pb) * kRowB + cb * 32);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int ty = t / 3, tx = t % 3;
#pragma unroll
        for (int prod = 0; prod < 3; ++prod) {  // p0 q1, p1 q0, p0 q0: the small terms first
          const int sa = prod == 1 ? 1 : 0, sb = prod == 0 ? 1 : 0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int pidx = ((q >> 1) + ty) * 4 + (q & 1) + tx;
            acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[t][cb][sa], fr[pidx][sb], acc[q], 0, 0, 0);
          }
        }
      }
    }
    // ---- + bias, ReLU, the second pool across the accumulators, features in the view(-1, 64 * 8 * 8) order
    {
      float* out = features + (size_t)n * kFeat + cbase * 64 + ph * 32 + il;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = fmaxf(fmaxf(acc[0][r], acc[1][r]), fmaxf(acc[2][r], acc[3][r])) + bv[r];
        if (TAPE) {  // the four members are this lane's four accumulators: compares only
          int arg = 0;
          float best = acc[0][r];
#pragma unroll
          for (int q = 1; q < 4; ++q)
            if (acc[q][r] > best) { best = acc[q][r]; arg = q; }
          tape[(size_t)n * kTape + kC1 * 256 + (cbase + (r & 3) + 8 * (r >> 2)) * 64 + ph * 32 + il] = (unsigned char)(v <= 0.f ? 4 : arg);
        }
        v = v > 0.f ? v : 0.f;
        if (bad) v = __builtin_nanf("");
        out[((r & 3) + 8 * (r >> 2)) * 64] = v;
      }
    }
    cur = nxt;
    bad = bad_next;
  }
}

// logits = W2 relu?(h) + b2 for one frame per wave: lane l multiplies h[l], h[l + 64] into the ten rows, ten wave sums in a fixed
// order; digit = the lowest index among the maxima.  A frame that digit_features could not read (select[n] outside [0, frames):
// the ReLU behind fc1 has swallowed its NaN features) or whose logits hold a NaN gets NaN logits and digit 10, the failure bin.
__global__ __launch_bounds__(kThreads) void digit_head_kernel(const float* __restrict__ hidden, const float* __restrict__ w,
                                                              const float* __restrict__ b, int N, const int32_t* __restrict__ select,
                                                              int64_t frames, int32_t* __restrict__ digit, float* __restrict__ logits) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (n >= N) return;  // wave-uniform; no barrier in this kernel
  const bool unread = select && (select[n] < 0 || (int64_t)select[n] >= frames);
  const float h0 = hidden[(size_t)n * kHidden + lane], h1 = hidden[(size_t)n * kHidden + 64 + lane];
  float best = 0.f;
  int arg = 0;
  bool nan = false;
#pragma unroll
  for (int k = 0; k < kClasses; ++k) {
    float v = fmaf(w[k * kHidden + 64 + lane], h1, w[k * kHidden + lane] * h0);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);  // (a butterfly: every lane holds the same sum)
    v += b[k];
    if (unread) v = __builtin_nanf("");
    if (logits && lane == 0) logits[(size_t)n * kClasses + k] = v;
    nan = nan || v != v;
    if (k == 0 || v > best) { best = v; arg = k; }
  }
  if (lane == 0) digit[n] = nan ? kClasses : arg;
}

// counts[w][d] += #{n : word[n] == w, digit[n] == d}: ONE workgroup counts into an integer histogram in LDS (integer adds
// commute exactly: the order of the atomics does not show), then one thread per cell adds its whole number onto the value
// already in the table.  No float atomics, nothing shared between workgroups: two runs agree bitwise.
constexpr int kCountThreads = 1024;
__global__ __launch_bounds__(kCountThreads) void word_counts_kernel(const int32_t* __restrict__ word, const int32_t* __restrict__ digit, int N,
                                                                    float* __restrict__ counts) {
  __shared__ int hist[kClasses * kBins];
  if (threadIdx.x < kClasses * kBins) hist[threadIdx.x] = 0;
  __syncthreads();
  for (int n = threadIdx.x; n < N; n += kCountThreads) {
    const int w = word[n], d = digit[n];
    if (w >= 0 && w < kClasses && d >= 0 && d < kBins) atomicAdd(&hist[w * kBins + d], 1);
  }
  __syncthreads();
  if (threadIdx.x < kClasses * kBins) counts[threadIdx.x] += (float)hist[threadIdx.x];
}

int cu_count() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cus = n;
  }
  return cus > 0 ? cus : 256;
}

}  // namespace

namespace {
int digit_features_any(const float* pred, int64_t frames, const int32_t* select, int64_t N, int act, const float* w1, const float* b1,
                       const float* w2, const float* b2, float* features, unsigned char* tape, hipStream_t s);
}

int digit_features_launch(const float* pred, int64_t frames, const int32_t* select, int64_t N, int act, const float* w1, const float* b1,
                          const float* w2, const float* b2, float* features, hipStream_t s) {
  return digit_features_any(pred, frames, select, N, act, w1, b1, w2, b2, features, nullptr, s);
}

int digit_features_train_launch(const float* pred, int64_t frames, const int32_t* select, int64_t N, int act, const float* w1, const float* b1,
                                const float* w2, const float* b2, float* features, unsigned char* tape, hipStream_t s) {
  if (!tape) { set_error("digit_features_train: null tape"); return MTRSSM_EINVAL; }
  return digit_features_any(pred, frames, select, N, act, w1, b1, w2, b2, features, tape, s);
}

namespace {
int digit_features_any(const float* pred, int64_t frames, const int32_t* select, int64_t N, int act, const float* w1, const float* b1,
                       const float* w2, const float* b2, float* features, unsigned char* tape, hipStream_t s) {
  if (!pred || !w1 || !b1 || !w2 || !b2 || !features) { set_error("digit_features: null pointer"); return MTRSSM_EINVAL; }
  if (frames <= 0 || N <= 0 || frames >= (int64_t)1 << 31 || N >= (int64_t)1 << 31) {
    set_error("digit_features: need 0 < frames, N < 2^31 (got %lld %lld)", (long long)frames, (long long)N);
    return MTRSSM_EINVAL;
  }
  if (!select && N > frames) {
    set_error("digit_features: without select frame n is read for output n, but N = %lld > frames = %lld", (long long)N, (long long)frames);
    return MTRSSM_EINVAL;
  }
  if (act != MTRSSM_ACT_IDENTITY && act != MTRSSM_ACT_TANH) { set_error("digit_features: the fused output activation is Identity or Tanh (got %d)", act); return MTRSSM_EINVAL; }
  if (((uintptr_t)pred | (uintptr_t)features) & 15) { set_error("digit_features: pred / features must be 16-byte aligned"); return MTRSSM_EINVAL; }
  if (((uintptr_t)select | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 | (uintptr_t)b2) & 3) {
    set_error("digit_features: select and the weights must be 4-byte aligned");
    return MTRSSM_EINVAL;
  }
  const int cus = cu_count();
  const int grid = (int)(N < cus ? N : cus);
#define MTRSSM_DIGIT_FEATURES(TANH, TAPE)                                                                                              \
  do {                                                                                                                                \
    set_last_kernel("mtrssm::digit_features_kernel<" #TANH ", " #TAPE ">");                                                           \
    hipLaunchKernelGGL((digit_features_kernel<TANH, TAPE>), dim3(grid), dim3(kThreads), 0, s, pred, frames, select, (int)N, w1, b1, w2, \
                       b2, features, tape);                                                                                           \
  } while (0)
  if (act == MTRSSM_ACT_TANH) {
    if (tape) MTRSSM_DIGIT_FEATURES(true, true);
    else MTRSSM_DIGIT_FEATURES(true, false);
  } else {
    if (tape) MTRSSM_DIGIT_FEATURES(false, true);
    else MTRSSM_DIGIT_FEATURES(false, false);
  }
#undef MTRSSM_DIGIT_FEATURES
  return check_launch("digit_features");
}
}  // namespace

int digit_head_launch(const float* hidden, const float* w, const float* b, int64_t N, const int32_t* select, int64_t frames, int32_t* digit,
                      float* logits, hipStream_t s) {
  if (!hidden || !w || !b || !digit) { set_error("digit_head: null pointer"); return MTRSSM_EINVAL; }
  if (N <= 0 || N >= (int64_t)1 << 31) { set_error("digit_head: need 0 < N < 2^31 (got %lld)", (long long)N); return MTRSSM_EINVAL; }
  if (select && frames <= 0) { set_error("digit_head: select needs the number of frames it indexes (got %lld)", (long long)frames); return MTRSSM_EINVAL; }
  if (((uintptr_t)hidden | (uintptr_t)w | (uintptr_t)b | (uintptr_t)digit | (uintptr_t)logits | (uintptr_t)select) & 3) {
    set_error("digit_head: buffers must be 4-byte aligned");
    return MTRSSM_EINVAL;
  }
  const int per = kThreads / 64;
  set_last_kernel("mtrssm::digit_head_kernel");
  hipLaunchKernelGGL(digit_head_kernel, dim3((unsigned)((N + per - 1) / per)), dim3(kThreads), 0, s, hidden, w, b, (int)N, select, frames, digit, logits);
  return check_launch("digit_head");
}

int word_counts_launch(const int32_t* word, const int32_t* digit, int64_t N, float* counts, hipStream_t s) {
  if (!word || !digit || !counts) { set_error("word_counts: null pointer"); return MTRSSM_EINVAL; }
  if (N <= 0 || N >= (int64_t)1 << 24) {
    set_error("word_counts: need 0 < N < 2^24 frames (the fp32 counts are exact below 2^24), got %lld", (long long)N);
    return MTRSSM_EINVAL;
  }
  if (((uintptr_t)word | (uintptr_t)digit | (uintptr_t)counts) & 3) { set_error("word_counts: buffers must be 4-byte aligned"); return MTRSSM_EINVAL; }
  set_last_kernel("mtrssm::word_counts_kernel");
  hipLaunchKernelGGL(word_counts_kernel, dim3(1), dim3(kCountThreads), 0, s, word, digit, (int)N, counts);
  return check_launch("word_counts");
}

}  // namespace mtrssm
