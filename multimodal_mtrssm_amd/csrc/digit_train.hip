// Training the digit reader for gfx950: the trunk's backward and the head in training mode.  The training
// forward is digit_ops.hip's fused trunk with its TAPE parameter set: one byte per pooled unit (conv1's [32][16][16], then conv2's
// [64][8][8] in the feature order) naming the member 2 dy + dx of the 2 x 2 window that held the maximum, 4 for a dead unit.
//
// digit_trunk_bwd_kernel: persistent workgroups of four waves walk the live frames (labels[n] in 0 .. 9; a dead frame is skipped by the
// whole workgroup and never read).  Per frame HBM gives the frame, its g_features row and its tape row, nothing else:
//   1. the frame is staged as in the forward (activation, denormalisation, clamp, haloed 34 x 34 fp32); conv2's tape and the g_features
//      row become the sparse g_c2 as 4096 (value, position) pairs -- a pooled unit passes its gradient to ONE conv2 pixel, so g_c2 has
//      at most 64 entries per channel out of 256 and is never made dense;
//   2. p1 = pool(relu(conv1(x))) again on the VALU: the forward's 9-term fma chains, the member picked by the tape, as a haloed fp32
//      image [18 x 18 positions][32 channels] (rows of 33 floats: lanes that differ in position or in channel meet no bank twice);
//   3. dW2[co][ci][tap] += g p1[ci][position + tap] over the entries of channel co: wave = 16 output channels, lane = (input channel,
//      half of the entries), 144 accumulators per lane that live in registers across all of the workgroup's frames;
//   4. g_p1[ci][position + tap] += W2[co][ci][tap] g: thread = (input channel, 4 x 4 block of conv2 pixels), the 6 x 6 positions the
//      block reaches summed in registers over the 64 output channels, then added into a haloed fp32 image in four rounds by block
//      parity (blocks of one parity share no position; the rounds have one order; no LDS atomics: ds_add_f32 measured ~200 cycles
//      per wave instruction here); the halo of the image takes what falls over the edge;
//   5. conv1's backward: thread = (channel, 32 pooled pixels), g_p1 routed by conv1's tape to one of the four pixels of the window,
//      dW1[c][tap] += g x[pixel + tap], db1 += g; db2 is the sum of the entries.
// Every workgroup stores ONE partial set at the end; digit_trunk_reduce_kernel adds the sets in ascending order (no atomics between
// workgroups: two calls agree bitwise).  All arithmetic is fp32 on exact operands: the tape removes three quarters of the terms of
// the dense products, which is what a bf16x2 MFMA form would have to win back (section 6m has the count).
//
// digit_head_train_kernel: one wave per frame as digit_head_kernel; dropout's keep-mask is a pure function of (seed, step, global row,
// unit) -- word j & 3 of Philox4x32-10((j >> 2, row, step, 0), key) -- so nothing is stored and any sharding of the rows draws the
// same mask.  Workgroup partial sums of g_fc2.weight / g_fc2.bias / the stats meet in digit_head_reduce_kernel in a fixed order.
#include "scan_common.h"

namespace mtrssm {

namespace {

using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

constexpr int kThreads = 256;
constexpr int kPix = 1024;
constexpr int kC1 = 32, kC2 = 64;
constexpr int kFeat = kC2 * 64;            // 4096
constexpr int kTape1 = kC1 * 256;          // 8192
constexpr int kTape = kTape1 + kFeat;      // 12288 bytes per frame
constexpr int kXW = 34, kPW = 18;
constexpr int kPos = kPW * kPW;            // 324 haloed positions of the pooled plane
constexpr int kPS = 33;                    // floats per position: 32 channels + 1
constexpr int kW1Row = 12;                 // conv1 weights in LDS: [32][9 taps, bias, 2 pad]
constexpr int kClasses = 10, kHidden = 128;

// one workgroup's partial set, in floats: dW2 [64][32][9], db2 [64], then conv1's [8 pixel groups][32][9 taps + bias]
constexpr int kSetW2 = kC2 * kC1 * 9;      // 18432
constexpr int kSetB2 = kSetW2 + kC2;       // 18496
constexpr int kSet = kSetB2 + 8 * kC1 * 10;  // 21056
constexpr int kTrunkOut = kSetB2 + kC1 * 9 + kC1;  // 18816 gradient elements

// LDS of the trunk backward, in bytes
constexpr int kOffW1 = kXW * kXW * 4;                  // 4624
constexpr int kOffP1 = kOffW1 + kC1 * kW1Row * 4;      // 6160
constexpr int kOffGp = kOffP1 + kPos * kPS * 4;        // 48928
constexpr int kOffGq = kOffGp + kPos * kPS * 4;        // 91696
constexpr int kOffBq = kOffGq + kFeat * 4;             // 108080
constexpr int kOffT1 = kOffBq + kFeat * 2;             // 116272
constexpr int kTrunkLds = kOffT1 + kTape1;             // 124464
static_assert(kOffGq % 16 == 0 && kOffT1 % 16 == 0 && kTrunkLds <= 160 * 1024, "LDS layout");

template <bool TANH>
__global__ __launch_bounds__(kThreads, 1) void digit_trunk_bwd_kernel(const float* __restrict__ pred, int64_t frames,
                                                                      const int32_t* __restrict__ select, int N,
                                                                      const unsigned char* __restrict__ tape,
                                                                      const float* __restrict__ gfeat, const int32_t* __restrict__ labels,
                                                                      const float* __restrict__ w1, const float* __restrict__ b1,
                                                                      const float* __restrict__ w2, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dtb_lds[];
  float* xin = reinterpret_cast<float*>(dtb_lds);
  float* w1s = reinterpret_cast<float*>(dtb_lds + kOffW1);
  float* p1s = reinterpret_cast<float*>(dtb_lds + kOffP1);
  float* gp1 = reinterpret_cast<float*>(dtb_lds + kOffGp);
  float* gq = reinterpret_cast<float*>(dtb_lds + kOffGq);
  unsigned short* bq = reinterpret_cast<unsigned short*>(dtb_lds + kOffBq);
  unsigned char* t1s = dtb_lds + kOffT1;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- once per workgroup: zero the two haloed images (their halos stay zero), conv1's weights
  for (int i = tid; i < kXW * kXW; i += kThreads) xin[i] = 0.f;
  for (int i = tid; i < kPos * kPS; i += kThreads) p1s[i] = 0.f;
  for (int i = tid; i < kC1 * kW1Row; i += kThreads) {
    const int c = i / kW1Row, j = i - c * kW1Row;
    w1s[i] = j < 9 ? w1[c * 9 + j] : (j == 9 ? b1[c] : 0.f);
  }

  float a2[16][9];  // dW2 of output channels 16 wave + k, input channel lane & 31, over this lane's half of the entries
#pragma unroll
  for (int k = 0; k < 16; ++k)
#pragma unroll
    for (int t = 0; t < 9; ++t) a2[k][t] = 0.f;
  float a1[9], ab1 = 0.f, ab2 = 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) a1[t] = 0.f;

  const int sy = tid >> 3, sx = (tid & 7) * 4;      // staging: four consecutive pixels of row tid / 8
  const int py1 = tid >> 4, px1 = tid & 15;         // conv1 again: thread = pooled pixel
  const int ci2 = lane & 31, half = lane >> 5;      // dW2
  const int c1 = tid & 31, grp = tid >> 5;          // conv1's backward

  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    const int label = labels[n];
    if (label < 0 || label >= kClasses) continue;  // dead: the whole workgroup passes by, nothing of the frame is read
    const int64_t src = select ? (int64_t)select[n] : (int64_t)n;
    if (src < 0 || src >= frames) continue;        // (an index outside the decode has nothing to read: it adds nothing either)
    __syncthreads();  // every wave is done with the previous frame's images, entries and tape
    {
      const float4 cur = *(reinterpret_cast<const float4*>(pred + src * kPix) + tid);
      float v[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float y = v[j];
        if (TANH) y = tanh_fast(y);
        y = (y + 1.f) * 0.5f;
        y = y < 0.f ? 0.f : y;
        y = y > 1.f ? 1.f : y;
        xin[(sy + 1) * kXW + sx + 1 + j] = y;
      }
    }
    {
      const unsigned char* trow = tape + (size_t)n * kTape;
      const u32x4* t16 = reinterpret_cast<const u32x4*>(trow);
      for (int i = tid; i < kTape1 / 16; i += kThreads) reinterpret_cast<u32x4*>(t1s)[i] = t16[i];
      const float* grow = gfeat + (size_t)n * kFeat;
#pragma unroll 4
      for (int k = 0; k < kFeat / kThreads; ++k) {
        const int e = tid + kThreads * k;
        const int code = trow[kTape1 + e];
        const float g = grow[e];
        const int u = e & 63;
        const int y = 2 * (u >> 3) + ((code >> 1) & 1), x = 2 * (u & 7) + (code & 1);
        const bool dead = code >= 4;
        gq[e] = dead ? 0.f : g;
        bq[e] = (unsigned short)(dead ? 0 : (y * kPW + x) | (code << 12));  // position, and the member in bits 12, 13
      }
      for (int i = tid; i < kPos * kPS; i += kThreads) gp1[i] = 0.f;
    }
    __syncthreads();  // the input image, the tape and the entries are in place
    // ---- p1 again: the forward's fma chains, the member the tape names
    {
      float p[4][4];
#pragma unroll
      for (int dy = 0; dy < 4; ++dy)
#pragma unroll
        for (int dx = 0; dx < 4; ++dx) p[dy][dx] = xin[(2 * py1 + dy) * kXW + 2 * px1 + dx];
      float* dst = p1s + ((py1 + 1) * kPW + px1 + 1) * kPS;
#pragma unroll 4
      for (int c = 0; c < kC1; ++c) {
        const float4 wa = *reinterpret_cast<const float4*>(w1s + c * kW1Row);
        const float4 wb = *reinterpret_cast<const float4*>(w1s + c * kW1Row + 4);
        const float4 wc = *reinterpret_cast<const float4*>(w1s + c * kW1Row + 8);
        const float w[9] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w, wc.x};
        const int code = t1s[c * 256 + tid];
        float val = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int dy = q >> 1, dx = q & 1;
          float s = 0.f;
#pragma unroll
          for (int t = 0; t < 9; ++t) s = fmaf(w[t], p[dy + t / 3][dx + t % 3], s);
          val = code == q ? s : val;
        }
        val += wc.y;  // bias
        dst[c] = code >= 4 ? 0.f : val;
      }
    }
    __syncthreads();  // p1 is complete
    // ---- dW2: this wave's 16 output channels, this lane's input channel and half of the entries
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int e0 = (wave * 16 + k) * 64 + half;
#pragma unroll 4
      for (int i = 0; i < 32; ++i) {
        const float g = gq[e0 + 2 * i];
        const float* pp = p1s + (int)(bq[e0 + 2 * i] & 0xfff) * kPS + ci2;
#pragma unroll
        for (int t = 0; t < 9; ++t) a2[k][t] = fmaf(g, pp[((t / 3) * kPW + t % 3) * kPS], a2[k][t]);
      }
    }
    // db2: the sum of a channel's entries (rotated start: one bank per lane)
    if (tid < kC2) {
#pragma unroll 8
      for (int u = 0; u < 64; ++u) ab2 += gq[tid * 64 + ((u + tid) & 63)];
    }
    // ---- g_p1: thread = (input channel, 4 x 4 block of conv2 pixels = 2 x 2 pooled units).  The block's gradients reach the 6 x 6
    // positions around it, which the thread sums in registers over all 64 output channels; the member a unit's gradient sits at is
    // data, so each of the four candidates takes its nine taps with the value or with 0.  Neighbouring blocks share their rims: the
    // blocks add their sums into the image in four rounds by the parity of (block row, block column) -- blocks of one parity lie
    // 8 apart and touch nothing in common, and the rounds have one order
    for (int pass = 0; pass < 2; ++pass) {
      const int ci = (tid >> 4) + 16 * pass, ba = (tid >> 2) & 3, bb = tid & 3;
      float fp[6][6];
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) fp[r][c] = 0.f;
      const float* wcol = w2 + (size_t)ci * 9;
      float wn[9];  // the next output channel's nine weights are in flight under this one's 144 fmas
#pragma unroll
      for (int t = 0; t < 9; ++t) wn[t] = wcol[t];
#pragma unroll 1
      for (int co = 0; co < kC2; ++co) {
        float w[9];
        const int cn = co + 1 < kC2 ? co + 1 : co;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          w[t] = wn[t];
          wn[t] = wcol[(size_t)cn * kC1 * 9 + t];
        }
#pragma unroll
        for (int uy = 0; uy < 2; ++uy)
#pragma unroll
          for (int ux = 0; ux < 2; ++ux) {
            const int e = co * 64 + (2 * ba + uy) * 8 + 2 * bb + ux;
            const float g = gq[e];
            const int m = bq[e] >> 12;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float gm = m == q ? g : 0.f;
#pragma unroll
              for (int t = 0; t < 9; ++t) fp[2 * uy + (q >> 1) + t / 3][2 * ux + (q & 1) + t % 3] = fmaf(gm, w[t], fp[2 * uy + (q >> 1) + t / 3][2 * ux + (q & 1) + t % 3]);
            }
          }
      }
      float* gp = gp1 + ((4 * ba) * kPW + 4 * bb) * kPS + ci;
#pragma unroll
      for (int round = 0; round < 4; ++round) {
        if (((ba & 1) * 2 + (bb & 1)) == round) {
#pragma unroll
          for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) gp[(r * kPW + c) * kPS] += fp[r][c];
        }
        __syncthreads();
      }
    }
    // ---- conv1's backward: thread = (channel, 32 pooled pixels); the tape routes g_p1 to one pixel of the window
#pragma unroll 2
    for (int i = 0; i < 32; ++i) {
      const int pix = grp * 32 + i, py = pix >> 4, px = pix & 15;
      const int code = t1s[c1 * 256 + pix];
      float g = gp1[((py + 1) * kPW + px + 1) * kPS + c1];
      g = code >= 4 ? 0.f : g;
      const float* xp = xin + (2 * py + ((code >> 1) & 1)) * kXW + 2 * px + (code & 1);
#pragma unroll
      for (int t = 0; t < 9; ++t) a1[t] = fmaf(g, xp[(t / 3) * kXW + t % 3], a1[t]);
      ab1 += g;
    }
  }

  // ---- one partial set per workgroup
  float* set = part + (size_t)blockIdx.x * kSet;
#pragma unroll
  for (int k = 0; k < 16; ++k)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float v = a2[k][t] + __shfl_xor(a2[k][t], 32, 64);
      if (half == 0) set[((wave * 16 + k) * kC1 + ci2) * 9 + t] = v;
    }
  if (tid < kC2) set[kSetW2 + tid] = ab2;
#pragma unroll
  for (int t = 0; t < 9; ++t) set[kSetB2 + (grp * kC1 + c1) * 10 + t] = a1[t];
  set[kSetB2 + (grp * kC1 + c1) * 10 + 9] = ab1;
}

// gradient element e = the sum of its entries in the S partial sets, in ascending order (conv1's also over the 8 pixel groups)
__global__ __launch_bounds__(kThreads) void digit_trunk_reduce_kernel(const float* __restrict__ part, int S, int accumulate,
                                                                      float* __restrict__ gw1, float* __restrict__ gb1,
                                                                      float* __restrict__ gw2, float* __restrict__ gb2) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= kTrunkOut) return;
  float total = 0.f;
  float* dst;
  if (e < kSetB2) {
    for (int s = 0; s < S; ++s) total += part[(size_t)s * kSet + e];
    dst = e < kSetW2 ? gw2 + e : gb2 + (e - kSetW2);
  } else {
    const int f = e - kSetB2;
    const int c = f < kC1 * 9 ? f / 9 : f - kC1 * 9, t = f < kC1 * 9 ? f - c * 9 : 9;
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int g = 0; g < 8; ++g) total += part[(size_t)s * kSet + kSetB2 + (g * kC1 + c) * 10 + t];
    dst = f < kC1 * 9 ? gw1 + f : gb1 + c;
  }
  *dst = accumulate ? *dst + total : total;
}

// ---- the head in training mode --------------------------------------------------------------------------------------------------------
constexpr int kHeadSet = kClasses * kHidden + kClasses + 3;  // g_fc2.weight, g_fc2.bias, (sum nll, sum hit, live count)

// Philox4x32-10 (Salmon et al., SC'11), as train_ops.hip's feed noise and dataset.philox4x32_10 state it
__device__ __forceinline__ unsigned philox_word(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, int word) {
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
  return word == 0 ? c0 : (word == 1 ? c1 : (word == 2 ? c2 : c3));
}

__global__ __launch_bounds__(kThreads) void digit_head_train_kernel(const float* __restrict__ hidden, const float* __restrict__ w,
                                                                    const float* __restrict__ b, const int32_t* __restrict__ labels,
                                                                    const int32_t* __restrict__ rows, int N, unsigned row0, unsigned step, unsigned key0, unsigned key1, float p,
                                                                    int normalize, float* __restrict__ nll_out, int32_t* __restrict__ pred_out,
                                                                    float* __restrict__ g_hidden, float* __restrict__ part) {
  __shared__ float red[kThreads / 64][kHeadSet];
  __shared__ int cnt[kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float inv_count = 1.f;
  if (normalize) {  // the mean loss's gradient needs the batch's live count before the first frame: every workgroup counts
    int c = 0;
    for (int n = tid; n < N; n += kThreads) c += (labels[n] >= 0 && labels[n] < kClasses) ? 1 : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
    if (lane == 0) cnt[wave] = c;
    __syncthreads();
    const int total = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    inv_count = 1.f / (float)(total > 1 ? total : 1);
  }
  const float keep_scale = 1.f / (1.f - p);
  float gw0[kClasses], gw1[kClasses], gb[kClasses], s_nll = 0.f, s_hit = 0.f, s_cnt = 0.f;
#pragma unroll
  for (int k = 0; k < kClasses; ++k) gw0[k] = gw1[k] = gb[k] = 0.f;

  for (int n = blockIdx.x * (kThreads / 64) + wave; n < N; n += gridDim.x * (kThreads / 64)) {  // wave-uniform; no barrier inside
    const int label = labels[n];
    float* grow = g_hidden + (size_t)n * kHidden;
    if (label < 0 || label >= kClasses) {
      grow[lane] = 0.f;
      grow[64 + lane] = 0.f;
      if (lane == 0) {
        if (nll_out) nll_out[n] = 0.f;
        if (pred_out) pred_out[n] = -1;
      }
      continue;
    }
    const float h0 = hidden[(size_t)n * kHidden + lane], h1 = hidden[(size_t)n * kHidden + 64 + lane];
    float m0 = 1.f, m1 = 1.f;
    if (p > 0.f) {
      const unsigned row = row0 + (rows ? (unsigned)rows[n] : (unsigned)n);
      const unsigned x0 = philox_word((unsigned)lane >> 2, row, step, 0u, key0, key1, lane & 3);
      const unsigned x1 = philox_word((unsigned)(lane + 64) >> 2, row, step, 0u, key0, key1, lane & 3);
      m0 = (float)(x0 >> 8) * 0x1p-24f >= p ? keep_scale : 0.f;
      m1 = (float)(x1 >> 8) * 0x1p-24f >= p ? keep_scale : 0.f;
    }
    const float d0 = h0 * m0, d1 = h1 * m1;
    float z[kClasses], best = 0.f;
    int arg = 0;
#pragma unroll
    for (int k = 0; k < kClasses; ++k) {
      float v = fmaf(w[k * kHidden + 64 + lane], d1, w[k * kHidden + lane] * d0);
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
      v += b[k];
      z[k] = v;
      if (k == 0 || v > best) { best = v; arg = k; }
    }
    float sum = 0.f, zl = 0.f, ex[kClasses];
#pragma unroll
    for (int k = 0; k < kClasses; ++k) {
      ex[k] = expf(z[k] - best);
      sum += ex[k];
      zl = k == label ? z[k] : zl;
    }
    const float nll = best + logf(sum) - zl;
    float gh0 = 0.f, gh1 = 0.f;
#pragma unroll
    for (int k = 0; k < kClasses; ++k) {
      float d = ex[k] / sum - (k == label ? 1.f : 0.f);
      if (normalize) d *= inv_count;
      gh0 = fmaf(w[k * kHidden + lane], d, gh0);
      gh1 = fmaf(w[k * kHidden + 64 + lane], d, gh1);
      gw0[k] = fmaf(d, d0, gw0[k]);
      gw1[k] = fmaf(d, d1, gw1[k]);
      gb[k] += d;
    }
    grow[lane] = h0 > 0.f ? gh0 * m0 : 0.f;
    grow[64 + lane] = h1 > 0.f ? gh1 * m1 : 0.f;
    s_nll += nll;
    s_hit += arg == label ? 1.f : 0.f;
    s_cnt += 1.f;
    if (lane == 0) {
      if (nll_out) nll_out[n] = nll;
      if (pred_out) pred_out[n] = arg;
    }
  }
#pragma unroll
  for (int k = 0; k < kClasses; ++k) {
    red[wave][k * kHidden + lane] = gw0[k];
    red[wave][k * kHidden + 64 + lane] = gw1[k];
    if (lane == 0) red[wave][kClasses * kHidden + k] = gb[k];
  }
  if (lane == 0) {
    red[wave][kHeadSet - 3] = s_nll;
    red[wave][kHeadSet - 2] = s_hit;
    red[wave][kHeadSet - 1] = s_cnt;
  }
  __syncthreads();
  for (int e = tid; e < kHeadSet; e += kThreads) part[(size_t)blockIdx.x * kHeadSet + e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
}

__global__ __launch_bounds__(kThreads) void digit_head_reduce_kernel(const float* __restrict__ part, int S, int accumulate,
                                                                     float* __restrict__ g_w, float* __restrict__ g_b, float* __restrict__ stats) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= kHeadSet) return;
  if (e >= kHeadSet - 3) {  // the stats in double: whole numbers stay whole
    double total = 0.0;
    for (int s = 0; s < S; ++s) total += (double)part[(size_t)s * kHeadSet + e];
    stats[e - (kHeadSet - 3)] = (float)total;
    return;
  }
  float total = 0.f;
  for (int s = 0; s < S; ++s) total += part[(size_t)s * kHeadSet + e];
  float* dst = e < kClasses * kHidden ? g_w + e : g_b + (e - kClasses * kHidden);
  *dst = accumulate ? *dst + total : total;
}

int cu_count() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cus = n;
  }
  return cus > 0 ? cus : 256;
}

int trunk_grid(int64_t N) { const int cus = cu_count(); return (int)(N < cus ? N : cus); }
int head_grid(int64_t N) {
  const int64_t groups = (N + kThreads / 64 - 1) / (kThreads / 64);
  const int cus = cu_count();
  return (int)(groups < cus ? groups : cus);
}

}  // namespace

int64_t digit_trunk_bwd_workspace_bytes(int64_t N) {
  if (N <= 0 || N >= (int64_t)1 << 31) { set_error("digit_trunk_bwd_workspace_bytes: need 0 < N < 2^31 (got %lld)", (long long)N); return MTRSSM_EINVAL; }
  return (int64_t)trunk_grid(N) * kSet * (int64_t)sizeof(float);
}

int digit_trunk_bwd_launch(const float* pred, int64_t frames, const int32_t* select, int64_t N, int act, const unsigned char* tape,
                           const float* g_features, const int32_t* labels, const float* w1, const float* b1, const float* w2, float* g_w1,
                           float* g_b1, float* g_w2, float* g_b2, int accumulate, void* workspace, int64_t workspace_bytes, hipStream_t s) {
  if (!pred || !tape || !g_features || !labels || !w1 || !b1 || !w2 || !g_w1 || !g_b1 || !g_w2 || !g_b2 || !workspace) {
    set_error("digit_trunk_bwd: null pointer");
    return MTRSSM_EINVAL;
  }
  if (frames <= 0 || N <= 0 || frames >= (int64_t)1 << 31 || N >= (int64_t)1 << 31) {
    set_error("digit_trunk_bwd: need 0 < frames, N < 2^31 (got %lld %lld)", (long long)frames, (long long)N);
    return MTRSSM_EINVAL;
  }
  if (!select && N > frames) {
    set_error("digit_trunk_bwd: without select frame n is read for row n, but N = %lld > frames = %lld", (long long)N, (long long)frames);
    return MTRSSM_EINVAL;
  }
  if (act != MTRSSM_ACT_IDENTITY && act != MTRSSM_ACT_TANH) { set_error("digit_trunk_bwd: the fused activation is Identity or Tanh (got %d)", act); return MTRSSM_EINVAL; }
  if (accumulate != 0 && accumulate != 1) { set_error("digit_trunk_bwd: accumulate is 0 or 1 (got %d)", accumulate); return MTRSSM_EINVAL; }
  if (((uintptr_t)pred | (uintptr_t)tape | (uintptr_t)g_features | (uintptr_t)workspace) & 15) {
    set_error("digit_trunk_bwd: pred / tape / g_features / workspace must be 16-byte aligned");
    return MTRSSM_EINVAL;
  }
  if (((uintptr_t)select | (uintptr_t)labels | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 | (uintptr_t)g_w1 | (uintptr_t)g_b1 | (uintptr_t)g_w2 |
       (uintptr_t)g_b2) & 3) {
    set_error("digit_trunk_bwd: select, labels, the weights and the gradients must be 4-byte aligned");
    return MTRSSM_EINVAL;
  }
  const int grid = trunk_grid(N);
  if (workspace_bytes < (int64_t)grid * kSet * (int64_t)sizeof(float)) {
    set_error("digit_trunk_bwd: workspace of %lld bytes, need %lld", (long long)workspace_bytes, (long long)grid * kSet * (long long)sizeof(float));
    return MTRSSM_EINVAL;
  }
  float* part = static_cast<float*>(workspace);
  auto launch = [&](auto* fn, const char* name) -> int {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, kTrunkLds);
    if (e != hipSuccess) { set_error("digit_trunk_bwd: hipFuncSetAttribute(max dynamic LDS=%d): %s", kTrunkLds, hipGetErrorString(e)); return MTRSSM_ELAUNCH; }
    set_last_kernel(name);
    hipLaunchKernelGGL(fn, dim3(grid), dim3(kThreads), kTrunkLds, s, pred, frames, select, (int)N, tape, g_features, labels, w1, b1, w2, part);
    return check_launch("digit_trunk_bwd");
  };
  const int rc = act == MTRSSM_ACT_TANH ? launch(digit_trunk_bwd_kernel<true>, "mtrssm::digit_trunk_bwd_kernel<true>")
                                        : launch(digit_trunk_bwd_kernel<false>, "mtrssm::digit_trunk_bwd_kernel<false>");
  if (rc != MTRSSM_OK) return rc;
  hipLaunchKernelGGL(digit_trunk_reduce_kernel, dim3((kTrunkOut + kThreads - 1) / kThreads), dim3(kThreads), 0, s, part, grid, accumulate, g_w1, g_b1,
                     g_w2, g_b2);
  return check_launch("digit_trunk_reduce");
}

int64_t digit_head_train_workspace_bytes(int64_t N) {
  if (N <= 0 || N >= (int64_t)1 << 31) { set_error("digit_head_train_workspace_bytes: need 0 < N < 2^31 (got %lld)", (long long)N); return MTRSSM_EINVAL; }
  return (int64_t)head_grid(N) * kHeadSet * (int64_t)sizeof(float);
}

int digit_head_train_launch(const float* hidden, const float* w, const float* b, const int32_t* labels, const int32_t* rows, int64_t N, int64_t row0,
                            int64_t step,
                            uint32_t key0, uint32_t key1, float p, int normalize, float* nll, int32_t* pred, float* stats, float* g_hidden,
                            float* g_w, float* g_b, int accumulate, void* workspace, int64_t workspace_bytes, hipStream_t s) {
  if (!hidden || !w || !b || !labels || !stats || !g_hidden || !g_w || !g_b || !workspace) { set_error("digit_head_train: null pointer"); return MTRSSM_EINVAL; }
  if (N <= 0 || N >= (int64_t)1 << 31) { set_error("digit_head_train: need 0 < N < 2^31 (got %lld)", (long long)N); return MTRSSM_EINVAL; }
  if (row0 < 0 || row0 + N > (int64_t)1 << 32 || step < 0 || step >= (int64_t)1 << 32) {
    set_error("digit_head_train: rows [row0, row0 + N) and step are 32-bit counter words (got %lld %lld)", (long long)row0, (long long)step);
    return MTRSSM_EINVAL;
  }
  if (!(p >= 0.f && p < 1.f)) { set_error("digit_head_train: the dropout rate lies in [0, 1) (got %g)", (double)p); return MTRSSM_EINVAL; }
  if ((normalize != 0 && normalize != 1) || (accumulate != 0 && accumulate != 1)) {
    set_error("digit_head_train: normalize and accumulate are 0 or 1 (got %d %d)", normalize, accumulate);
    return MTRSSM_EINVAL;
  }
  if (((uintptr_t)hidden | (uintptr_t)w | (uintptr_t)b | (uintptr_t)labels | (uintptr_t)rows | (uintptr_t)nll | (uintptr_t)pred | (uintptr_t)stats | (uintptr_t)g_hidden |
       (uintptr_t)g_w | (uintptr_t)g_b | (uintptr_t)workspace) & 3) {
    set_error("digit_head_train: buffers must be 4-byte aligned");
    return MTRSSM_EINVAL;
  }
  const int grid = head_grid(N);
  if (workspace_bytes < (int64_t)grid * kHeadSet * (int64_t)sizeof(float)) {
    set_error("digit_head_train: workspace of %lld bytes, need %lld", (long long)workspace_bytes, (long long)grid * kHeadSet * (long long)sizeof(float));
    return MTRSSM_EINVAL;
  }
  float* part = static_cast<float*>(workspace);
  set_last_kernel("mtrssm::digit_head_train_kernel");
  hipLaunchKernelGGL(digit_head_train_kernel, dim3(grid), dim3(kThreads), 0, s, hidden, w, b, labels, rows, (int)N, (unsigned)row0, (unsigned)step, key0, key1,
                     p, normalize, nll, pred, g_hidden, part);
  int rc = check_launch("digit_head_train");
  if (rc != MTRSSM_OK) return rc;
  hipLaunchKernelGGL(digit_head_reduce_kernel, dim3((kHeadSet + kThreads - 1) / kThreads), dim3(kThreads), 0, s, part, grid, accumulate, g_w, g_b, stats);
  return check_launch("digit_head_reduce");
}

}  // namespace mtrssm
