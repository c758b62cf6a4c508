// The encoders' strided stem in ONE pass per frame (default.yaml:31-60): Conv2d(k 3, s 2, p 1) x 3 with channels
// (frame + 2 coordinate planes) -> 8 -> 16 -> 32 on 4096-position frames (64 x 64 or 128 x 32), bf16x2 arithmetic.  Included by
// conv.hip after conv_s2_band.h.
//
// All three layers are HBM-bound by two orders of magnitude and frame-local; as three launches they write y1 and y2 and read
// them straight back (315 MB per step at B T = 3200 per modality).  Here a persistent workgroup (512 threads, one per CU) walks
// frames; per frame it reads the 16 KB frame once and writes y1, y2, y3 once (the backward pass needs all three), the
// activated bf16 pieces of y1 and y2 stay in LDS:
//   * frame image F: one 16-byte row per (source row, y1 column ox) = the three x-taps of the stride-2 window, both pieces:
//       [p0 f(2 ox - 1), p0 f(2 ox), p0 f(2 ox + 1), 0, p1 (the same three), 0]   (33 KB; image row 0 = the zero row above the frame)
//     so that the three source rows of a window are three k-quarters of ONE v_mfma_f32_16x16x32_bf16 (lane group = ty, the
//     fourth has zero weights).  With A = [a0, 0, a0, 0] that MFMA forms a0 b0 + a0 b1, a second one with A = [a1, 0, 0, 0]
//     forms a1 b0: the three products of the bf16x2 mode in 2 MFMAs of 16 cycles per 16 pixels (the band kernel: 15 of 32
//     cycles per 32 pixels, 5 of every 8 k-slots zero).
//   * the two coordinate planes are frame-independent: their contribution (and the bias) is the accumulators' START value,
//     formed once per workgroup in fp32 from the packed fp32 weights and kept in registers (a wave owns the same 8 units of 16
//     pixels in every frame: 32 registers).  The band kernel re-requested and re-converted the planes for every tile.
//   * y1 is stored from the accumulators; the same values, activated and split once, are written as the image conv2 reads:
//     conv3x3s2_band_kernel<8, 0>'s layout ([piece][row][parity-de-interleaved column] 16-byte rows) for the whole frame.
//   * conv2 keeps that kernel's k-blocks (tap 2 kb + kl, 8 channels), product order and start value: y2 is bit-identical to
//     its y2 given the same y1.  One 32-pixel unit per wave.
//   * y2's activated pieces go to a 16-channel image [piece][channel half][haloed position]; conv3 is 5 k-steps (two taps of 16
//     channels each) x 3 products of v_mfma_f32_16x16x32_bf16 per (16-pixel unit, 16-channel row tile): 8 jobs = one per wave.
//   * the next frame is requested right after this one's conversion and flies under the three products; three barriers per
//     frame (F, y1 image, y2 image are separate buffers: conv3 of a frame overlaps the next frame's conversion in other waves).
// conv1's and conv2's weights are A operands in registers for the whole launch, conv3's a per-lane table in LDS.
#pragma once
#include <type_traits>

namespace mtrssm {

struct StemProblem {
  const float* src;           // [N][1][Hs][Ws], Hs * Ws == 4096
  const float* coords;        // [2][Hs][Ws]
  const float* wp1;           // layer 1 packed fp32 [32][9][16] (the coordinate channels' weights are read from here)
  const unsigned short* wq1;  // packed bf16 pieces [2][32][9][16] of the three layers
  const unsigned short* wq2;
  const unsigned short* wq3;
  const float* b1;            // biases or null
  const float* b2;
  const float* b3;
  float* y1;                  // [N][8][Hs/2][Ws/2]
  float* y2;                  // [N][16][Hs/4][Ws/4]
  float* y3;                  // [N][32][Hs/8][Ws/8]
  int N, Ws, act, nx;
};

constexpr int kStemThreads = 512;
constexpr int kStemPlane = 4096;
constexpr int kStemF = 65 * 32 * 16;        // (Hs + 1) * (Ws / 2) rows: 33280 (64 x 64) / 33024 (128 x 32)
constexpr int kStemY1 = 2 * 65 * 18 * 16;   // 2 pieces x (Hs / 2 + 1) x (Ws / 2 + 2) rows: 35904 (64 x 64) / 37440 (128 x 32)
constexpr int kStemY2 = 4 * 298 * 16;       // 2 pieces x 2 halves x ((Hs / 4 + 1) (Ws / 4 + 1) + 1) rows: 289 + 1 / 297 + 1 positions
constexpr int kStemImg = kStemF + kStemY1 + kStemY2;
constexpr int kStemA3 = 2 * 10 * 64 * 16;   // conv3's A operands: [row tile][k-step][piece][lane] 16-byte rows
constexpr int kStemLds = kStemImg + kStemA3;

__global__ __launch_bounds__(kStemThreads, 1) void encoder_stem_kernel(const StemProblem pa, const StemProblem pb) {
  const bool second = blockIdx.x >= (unsigned)pa.nx;  // workgroup-uniform
  // (every field is selected by itself: a reference to "second ? pb : pa" can make the compiler copy both structs to scratch)
#define MTRSSM_PICK(f) (second ? pb.f : pa.f)
  const float* __restrict__ src = MTRSSM_PICK(src);
  const float* __restrict__ coords = MTRSSM_PICK(coords);
  const float* __restrict__ wp1 = MTRSSM_PICK(wp1);
  const unsigned short* __restrict__ wq1 = MTRSSM_PICK(wq1);
  const unsigned short* __restrict__ wq2 = MTRSSM_PICK(wq2);
  const unsigned short* __restrict__ wq3 = MTRSSM_PICK(wq3);
  const float* __restrict__ b1 = MTRSSM_PICK(b1);
  const float* __restrict__ b2 = MTRSSM_PICK(b2);
  const float* __restrict__ b3 = MTRSSM_PICK(b3);
  float* __restrict__ y1 = MTRSSM_PICK(y1);
  float* __restrict__ y2 = MTRSSM_PICK(y2);
  float* __restrict__ y3 = MTRSSM_PICK(y3);
  const int N = MTRSSM_PICK(N), Ws = MTRSSM_PICK(Ws), act = MTRSSM_PICK(act), nwg = MTRSSM_PICK(nx);
#undef MTRSSM_PICK
  const int wg = second ? (int)blockIdx.x - pa.nx : (int)blockIdx.x;
  const int wsh = 31 - __builtin_clz(Ws);                   // host: Ws in {32, 64}, Hs = 4096 / Ws
  const int Hs = kStemPlane >> wsh;
  const int W1 = Ws >> 1, q1 = wsh - 1, H1 = Hs >> 1;       // y1: 1024 pixels
  const int W2 = Ws >> 2, q2 = wsh - 2, H2 = Hs >> 2;       // y2: 256
  const int W3 = Ws >> 3, q3 = wsh - 3;                     // y3: 64
  const int RP1 = (2 * W2 + 2) * 16, IMG1 = (H1 + 1) * RP1; // y1 image: band_row_bytes(W2), H1 + 1 rows per piece
  const int PW2 = W2 + 1, HALF2 = ((H2 + 1) * PW2 + 1) * 16, IMG2 = 2 * HALF2;  // y2 image: zero row above, zero column left
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4, il = lane & 31, kl = lane >> 5;
  if (wg >= N) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char stem_lds[];
  unsigned char* const F = stem_lds;
  unsigned char* const Y1 = stem_lds + kStemF;
  unsigned char* const Y2 = stem_lds + kStemF + kStemY1;
  unsigned char* const A3 = stem_lds + kStemImg;
  using f32x4v = __attribute__((ext_vector_type(4))) float;
  constexpr size_t PIECE = (size_t)32 * 9 * 16;             // host: every layer packs to CoutPad == 32, Cpad == 16

  // conv1's A operands (16 x 16 x 32): row l16 = output channel (rows 8 .. 15 are zero padding), lane group g = window row ty
  bf16x8 a1m, a1s;
  {
    const int ty = g < 3 ? g : 0;
    u16x8 m = u16x8{0, 0, 0, 0, 0, 0, 0, 0}, s = m;
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
      const size_t o = ((size_t)l16 * 9 + ty * 3 + tx) * 16;  // input channel 0 = the frame
      const unsigned short h0 = wq1[o], h1 = wq1[PIECE + o];
      m[tx] = g < 3 ? h0 : (unsigned short)0;
      m[4 + tx] = m[tx];
      s[tx] = g < 3 ? h1 : (unsigned short)0;
    }
    a1m = __builtin_bit_cast(bf16x8, m);
    a1s = __builtin_bit_cast(bf16x8, s);
  }
  // conv2's: exactly conv3x3s2_band_kernel<8, 0>'s (row il, k-block kb = tap 2 kb + kl x channels 0..7)
  bf16x8 a2[5][2];
#pragma unroll
  for (int kb = 0; kb < 5; ++kb) {
    const int tap = 2 * kb + kl;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      u32x4 v = u32x4{0u, 0u, 0u, 0u};
      if (tap < 9) v = *reinterpret_cast<const u32x4*>(wq2 + s * PIECE + ((size_t)il * 9 + tap) * 16);
      a2[kb][s] = __builtin_bit_cast(bf16x8, v);
    }
  }
  // conv3's (16 x 16 x 32): row l16 of row tile ct = output channel 16 ct + l16; k-step ss = taps 2 ss and 2 ss + 1 of 16 channels:
  // lane group g has tap 2 ss + (g >> 1), channels 8 (g & 1) .. + 7
  const int u3 = wave & 3, ct = wave >> 2;
  // (kept in LDS, read once per frame: with them in registers conv1's eight accumulators do not fit beside the other weights)
  unsigned char* const a3 = A3 + ((size_t)ct * 10 * 64 + lane) * 16;
  if (u3 == 0) {
#pragma unroll
    for (int ss = 0; ss < 5; ++ss) {
      const int tap = 2 * ss + (g >> 1);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (tap < 9) v = *reinterpret_cast<const u32x4*>(wq3 + s * PIECE + ((size_t)(16 * ct + l16) * 9 + tap) * 16 + 8 * (g & 1));
        *reinterpret_cast<u32x4*>(a3 + (2 * ss + s) * 64 * 16) = v;
      }
    }
  }
  for (int o = tid * 16; o < kStemImg; o += kStemThreads * 16) *reinterpret_cast<u32x4*>(stem_lds + o) = u32x4{0u, 0u, 0u, 0u};

  // conv1: this wave's eight 16-pixel units of every frame, pixel j = 128 wave + 16 i + l16 -> (oy, ox); the lane's accumulator
  // rows are channels 4 g + r: lane groups 2 and 3 hold padding rows, so after the products lanes 32 .. 63 take over units
  // 4 .. 7 from lanes 0 .. 31 (one cross-lane read per value) and every lane activates, splits and stores: merged unit i of a lane is unit
  // i + 4 hi, its channels 4 gc + r
  const int hi = g >> 1, gc = g & 1;
  // pixel j = j0 + 16 i: (oy, ox) = (oy0 + doy(i), ox0 + dox(i)) with wave-uniform steps (16 i has no bits below 16 <= W1)
  const int j0 = 128 * wave + l16, oy0 = j0 >> q1, ox0 = j0 & (W1 - 1);
  auto doy = [&](int i) { return (16 * i) >> q1; };
  auto dox = [&](int i) { return (16 * i) & (W1 - 1); };
  const unsigned fa0 = (unsigned)(((2 * oy0 + (g < 3 ? g : 2)) * W1 + ox0) * 16);   // F row of the lane's k-quarter
  auto fa = [&](int i) { return fa0 + (unsigned)((2 * doy(i) * W1 + dox(i)) * 16); };
  const int ic0 = ox0 + 1;  // y1 image column (0 = the zero column left of the plane); dox is even: the parity is the lane's
  const unsigned ya0 = (unsigned)((1 + oy0) * RP1 + ((ic0 & 1) ? W2 + 1 + (ic0 >> 1) : (ic0 >> 1)) * 16 + 8 * gc);
  auto ya = [&](int i) { return ya0 + (unsigned)(doy(i) * RP1 + (dox(i) >> 1) * 16); };
  f32x4v sv[8];            // start value: bias + the coordinate planes' contribution (fp32, frame-independent)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int oy = oy0 + doy(i), ox = ox0 + dox(i);
#pragma unroll
    for (int r = 0; r < 4; ++r) sv[i][r] = b1 ? b1[(4 * g + r) & 7] : 0.f;
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
      const int sy = 2 * oy - 1 + t / 3, sx = 2 * ox - 1 + t % 3;
      const bool in = sy >= 0 && sy < Hs && sx >= 0 && sx < Ws;
      const int so = in ? sy * Ws + sx : 0;  // (unconditional requests from a valid address, selected afterwards)
      const float c0 = in ? coords[so] : 0.f, c1 = in ? coords[kStemPlane + so] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* w = wp1 + ((size_t)((4 * g + r) & 7) * 9 + t) * 16;
        sv[i][r] = fmaf(w[2], c1, fmaf(w[1], c0, sv[i][r]));
      }
    }
  }
  // conv2: this wave's 32-pixel unit, pixel j = 32 wave + il (band kernel: baddr / opix with the whole frame as one band)
  unsigned ba2[5];
  const int j2 = 32 * wave + il, oy2 = j2 >> q2, ox2 = j2 & (W2 - 1);
#pragma unroll
  for (int kb = 0; kb < 5; ++kb) {
    const int tap = 2 * kb + kl < 9 ? 2 * kb + kl : 8, ty = tap / 3, tx = tap - 3 * ty;
    const int slot = (tx & 1) ? W2 + 1 + ox2 : ox2 + (tx >> 1);
    ba2[kb] = (unsigned)((2 * oy2 + ty) * RP1 + slot * 16);
  }
  const unsigned yb = (unsigned)(((oy2 + 1) * PW2 + ox2 + 1) * 16 + 8 * kl);  // y2 image row of the pixel (channel half 0, piece 0)
  float bv2[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) bv2[r] = b2 ? b2[4 * kl + (r & 3) + 8 * (r >> 2)] : 0.f;
  // conv3: job (unit u3, row tile ct), pixel j = 16 u3 + l16; tap (ty, tx) reads y2 (2 oy - 1 + ty, 2 ox - 1 + tx) = image (2 oy + ty, 2 ox + tx)
  const int j3 = 16 * u3 + l16, oy3 = j3 >> q3, ox3 = j3 & (W3 - 1);
  unsigned ba3[5];
#pragma unroll
  for (int ss = 0; ss < 5; ++ss) {
    const int tap = 2 * ss + (g >> 1) < 9 ? 2 * ss + (g >> 1) : 8, ty = tap / 3, tx = tap - 3 * ty;
    ba3[ss] = (unsigned)((g & 1) * HALF2 + ((2 * oy3 + ty) * PW2 + 2 * ox3 + tx) * 16);
  }
  f32x4v bv3;
#pragma unroll
  for (int r = 0; r < 4; ++r) bv3[r] = b3 ? b3[16 * ct + 4 * g + r] : 0.f;

  band_f4 pv[2];  // the frame: two groups of four positions per thread
  auto request = [&](int n) {
    const float* f = src + (size_t)n * kStemPlane;
#pragma unroll
    for (int k = 0; k < 2; ++k) pv[k] = *reinterpret_cast<const band_f4*>(f + (tid + kStemThreads * k) * 4);
  };
  auto stage = [&]() {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int p = (tid + kStemThreads * k) * 4, r = p >> wsh, x = p & (Ws - 1);
      const band_f4 v = pv[k];
      float left = __shfl_up(v[3], 1);  // f(x - 1): the neighbour's last position (lane 0 of a wave starts a row)
      if (x == 0) left = 0.f;
      unsigned short hl[2], h[4][2];
      split_bf16<2>(left, hl);
#pragma unroll
      for (int e = 0; e < 4; ++e) split_bf16<2>(v[e], h[e]);
      const u16x8 qa = u16x8{hl[0], h[0][0], h[1][0], 0, hl[1], h[0][1], h[1][1], 0};
      const u16x8 qb = u16x8{h[1][0], h[2][0], h[3][0], 0, h[1][1], h[2][1], h[3][1], 0};
      unsigned char* d = F + ((r + 1) * W1 + (x >> 1)) * 16;
      *reinterpret_cast<u16x8*>(d) = qa;
      *reinterpret_cast<u16x8*>(d + 16) = qb;
    }
  };

  auto frame = [&](int n, auto mode_tag) {
    constexpr int MODE = decltype(mode_tag)::value;
    auto activate = [&](float v) { return MODE == 1 ? elu_fast(v) : act_fwd(v, act); };
    {  // conv1
      f32x4v acc[8];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {  // four independent chains at a time
        bf16x8 b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = *reinterpret_cast<const bf16x8*>(F + fa(4 * hh + i));
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[4 * hh + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1s, b[i], sv[4 * hh + i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[4 * hh + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1m, b[i], acc[4 * hh + i], 0, 0, 0);
      }
      float* o = y1 + (size_t)n * (8 * 1024) + (size_t)(4 * gc) * 1024 + j0 + 64 * hi;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned short h[4][2];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float up = __shfl(acc[i + 4][r], lane & 31);
          const float v = hi ? up : acc[i][r];  // lanes 0 .. 31: unit i, lanes 32 .. 63: unit i + 4 of lane - 32
          o[r * 1024 + 16 * i] = v;
          split_bf16<2>(activate(v), h[r]);
        }
        unsigned char* d = Y1 + (hi ? ya(i + 4) : ya(i));
        *reinterpret_cast<uint2*>(d) = make_uint2((unsigned)h[0][0] | ((unsigned)h[1][0] << 16), (unsigned)h[2][0] | ((unsigned)h[3][0] << 16));
        *reinterpret_cast<uint2*>(d + IMG1) = make_uint2((unsigned)h[0][1] | ((unsigned)h[1][1] << 16), (unsigned)h[2][1] | ((unsigned)h[3][1] << 16));
      }
    }
    lds_barrier();  // the y1 image is complete
    {  // conv2
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = r < 8 ? bv2[r] : 0.f;
#pragma unroll
      for (int kb = 0; kb < 5; ++kb) {
        const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(Y1 + ba2[kb]);
        const bf16x8 b1q = *reinterpret_cast<const bf16x8*>(Y1 + ba2[kb] + IMG1);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2[kb][0], b1q, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2[kb][1], b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2[kb][0], b0, acc, 0, 0, 0);
      }
      float* o = y2 + (size_t)n * (16 * 256) + (size_t)(4 * kl) * 256 + j2;
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        unsigned short h[4][2];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          o[(8 * hf + r) * 256] = acc[4 * hf + r];
          split_bf16<2>(activate(acc[4 * hf + r]), h[r]);
        }
        unsigned char* d = Y2 + hf * HALF2 + yb;
        *reinterpret_cast<uint2*>(d) = make_uint2((unsigned)h[0][0] | ((unsigned)h[1][0] << 16), (unsigned)h[2][0] | ((unsigned)h[3][0] << 16));
        *reinterpret_cast<uint2*>(d + IMG2) = make_uint2((unsigned)h[0][1] | ((unsigned)h[1][1] << 16), (unsigned)h[2][1] | ((unsigned)h[3][1] << 16));
      }
    }
    lds_barrier();  // the y2 image is complete
    {  // conv3
      f32x4v acc = bv3;
#pragma unroll
      for (int ss = 0; ss < 5; ++ss) {
        const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(Y2 + ba3[ss]);
        const bf16x8 b1q = *reinterpret_cast<const bf16x8*>(Y2 + ba3[ss] + IMG2);
        const bf16x8 w0 = *reinterpret_cast<const bf16x8*>(a3 + (2 * ss) * 64 * 16);
        const bf16x8 w1 = *reinterpret_cast<const bf16x8*>(a3 + (2 * ss + 1) * 64 * 16);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, b1q, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, b0, acc, 0, 0, 0);
      }
      float* o = y3 + (size_t)n * (32 * 64) + (size_t)(16 * ct + 4 * g) * 64 + j3;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r * 64] = acc[r];
    }
  };

  // The requests stay unconditional (past the last frame they repeat it) so that the wait before a conversion is counted.
  // Buffer reuse: F is rewritten after the barrier that ends conv1, the y1 image after the one that ends conv2, the y2 image
  // after the one that follows the next conversion -- each a barrier every wave passes after its last read.
  const int last = wg + ((N - 1 - wg) / nwg) * nwg;  // this workgroup's last frame
  request(wg);
  __syncthreads();  // the zero fill
  for (int n = wg; n < N; n += nwg) {
    stage();
    const int nx = n + nwg;
    request(nx < last ? nx : last);
    lds_barrier();  // F is complete
    if (act == MTRSSM_ACT_ELU) frame(n, std::integral_constant<int, 1>{});
    else frame(n, std::integral_constant<int, 2>{});
  }
}

}  // namespace mtrssm
