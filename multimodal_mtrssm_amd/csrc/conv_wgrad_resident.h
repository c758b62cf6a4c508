// Staged weight-gradient kernels (included by conv.hip after conv_split.h and conv_wgrad_stage.h, which holds the pieces they
// share and the one body that sums their partial sets): a workgroup per CU owns a run of frames, loads
// every frame of both operands once, converts it once, keeps it in LDS for the MFMAs and leaves ONE partial set for a
// reduce kernel.  In this file: the 3x3 / stride 1 layers of the residual stacks (first, with the reasoning), their 1x1
// layers, the encoders' three 3x3 / stride-2 convolutions and the decoders' three k = 4 / stride-2 transposed convolutions.
//
// Weight gradient of the 3x3 / stride 1 / pad 1 layers of the residual stacks on 64-pixel planes (8x8 vision, 16x4 audio)
// with BOTH operands staged once per frame.
//
//   dW[co][ty][tx][ci] = sum over frames n and pixels (y, x) of  a[n][co][y][x] * act(src)[n][ci][y + ty - 1][x + tx - 1]
//
// The register-direct kernel (conv_split.h: conv3x3_weight_grad_split_kernel) lets every lane load, activate and split its
// own operands: each src element is fetched 2 (co tiles) x 3 (window rows) times by 16-byte loads that touch 32 cache lines
// per instruction and is converted as often, each `a` element twice -- the kernel is VALU-bound (about 75 % of its issue
// slots are conversions), and ~60 us of every launch pass after its loop (9.4 M fp32 atomics of the tiles, and -- the larger
// part, see profiles/round2_notes.md -- the bias sums every workgroup adds to the same 64 addresses).  Here a workgroup
// owns a run of frames and
//   * loads every frame of `src` and of `a` ONCE, coalesced (consecutive lanes = consecutive 16 bytes), activates / splits
//     it once and writes it to LDS: `a` as a plain [co][pixel] bf16 image, src as a channel-major image with a zero halo
//     row between consecutive planes: a row tap (ty) is a 16-byte read at row offset ty, the column taps (tx) are funnel
//     shifts of that fragment in registers -- a lane's 8 pixels are whole plane rows, so the shifted row needs no
//     neighbour (three column-shifted copies in LDS instead made the LDS pipe the bottleneck: 2300 of its cycles per
//     frame against 3456 of MFMA work, and the two did not overlap);
//   * double-buffers those images: frame n + 1 is converted (VALU + ds_write_b64) while the MFMAs of frame n run, its
//     raw values requested a whole frame ahead, so no HBM latency is exposed;
//   * gives each wave nine accumulator tiles chosen so that it reads two image rows instead of three: the two waves of a
//     ci tile hold {co tile 0: taps 0-4, co tile 1: taps 0-3} and {co tile 1: taps 4-8, co tile 0: taps 5-8};
//   * writes its partial tiles with plain 16-byte stores, in accumulator order, to a scratch slice of its own (`part`),
//     summed and scattered into dwp by wgrad_reduce_batch_kernel (layout WgRedRes) right behind it in the stream: no atomics, run-to-run
//     deterministic.  With part == NULL (no scratch: first call inside a stream capture, or MTRSSM_WGRAD_PARTIALS=0) the
//     tiles leave by fp32 atomics in the dwp layout [co][tap][Cpad], as in the other kernels.
// One barrier per frame.
//
// LDS images: src piece [C][H + 1 rows][W] bf16 -- row 0 of every plane is the zero halo, shared with the plane above (the
// image ends with one more zero row); `a` piece [64][64 pixels + 8].  Both pitches are an odd number of 16-byte
// (W = 4: 8-byte, reads are two ds_read_b64 halves) slots, so the 32 channels one read covers fall on different banks.
#pragma once

namespace mtrssm {

template <int W>
__host__ __device__ constexpr int wgres_pitch() { return (64 / W + 1) * 2 * W; }  // 144 (W = 8), 136 (W = 4)
constexpr int kWgresAPitch = 144;  // bytes per co row of the `a` image: 64 bf16 + 16
template <int SPLIT, int C, int W>
__host__ __device__ constexpr int wgres_xbuf_bytes() { return SPLIT * C * wgres_pitch<W>() + 16; }
template <int SPLIT>
__host__ __device__ constexpr int wgres_abuf_bytes() { return SPLIT * 64 * kWgresAPitch; }
template <int SPLIT, int C, int W>
__host__ __device__ constexpr int wgres_lds_bytes() { return 2 * (wgres_xbuf_bytes<SPLIT, C, W>() + wgres_abuf_bytes<SPLIT>()); }
// floats of one workgroup's partial tile set: its waves' nine 32x32 tiles
__host__ __device__ constexpr int wgres_tile_floats(int c) { return 2 * (c / 32) * 9 * 1024; }
// ... followed by the workgroup's 64 bias-gradient sums (256 workgroups adding to the same 64 addresses took 10-25 us)
__host__ __device__ constexpr int wgres_set_floats(int c) { return wgres_tile_floats(c) + 64; }
constexpr int kWg1x1SetFloats = 8 * 1024 + 64;  // conv1x1_wgrad_staged_kernel: 8 waves x one tile, + 64 bias sums

// One problem's work of one workgroup: bx of the problem's nbx x blocks (its run of frames_per_wg frames), co group blockIdx.y.
// The kernels below are wrappers: one problem per grid, or two (audio and vision planes) side by side in one grid.
template <int SPLIT, int C, int W>
__device__ __forceinline__ void conv3x3_wgrad_resident_body(
    const int N, const int Cout, const int cpad, const int act, const int pre_act, const float* __restrict__ a, const float* __restrict__ src, float* __restrict__ dwp,
    float* __restrict__ part, float* __restrict__ dbias, const int frames_per_wg, const int bx, const int nbx) {
  static_assert(SPLIT == 1 || SPLIT == 2, "one or two bf16 pieces");
  constexpr int NW = 2 * (C / 32), NT = 64 * NW;
  constexpr int RB = 2 * W;  // bytes per image row
  constexpr int PITCH = wgres_pitch<W>(), COPYB = C * PITCH, XBUFB = wgres_xbuf_bytes<SPLIT, C, W>();
  constexpr int APIECEB = 64 * kWgresAPitch, ABUFB = wgres_abuf_bytes<SPLIT>();
  constexpr int XI = 4, AI = 1024 / NT;  // float4 items per thread and frame: src (C * 16 = 4 NT), a (64 co * 16)
  extern __shared__ __attribute__((aligned(16))) unsigned char wgres_lds[];
  unsigned char* const lds = wgres_lds;           // [src image 0][src image 1][a image 0][a image 1]
  unsigned char* const lds_a = wgres_lds + 2 * XBUFB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int il = lane & 31, kl = lane >> 5;
  const int tci = wave >> 1, half = wave & 1;
  const int n0 = bx * frames_per_wg;
  const int n1 = n0 + frames_per_wg < N ? n0 + frames_per_wg : N;
  if (n0 >= n1) return;  // whole workgroup
  const int nlast = n1 - 1;
  const int cob = blockIdx.y * 64;
  // development aid (tools/wgrad_probe.py): cycle stamps of workgroup 0 and of the middle workgroup
  unsigned long long* const prof = (tid == 0 && blockIdx.y == 0 && g_res_prof) ? (bx == 0 ? g_res_prof + 32 : (bx == nbx / 2 ? g_res_prof + 40 : nullptr)) : nullptr;
  if (prof) prof[0] = __builtin_readcyclecounter();

  const bool act_elu = act == MTRSSM_ACT_ELU, act_relu = act == MTRSSM_ACT_RELU, pre = pre_act != 0;
  const WgActSel act_sel{act_elu, act_relu, pre};

  // ---- zero everything once: the halo rows are never written again
  for (int o = tid * 16; o < wgres_lds_bytes<SPLIT, C, W>(); o += NT * 16) *reinterpret_cast<uint4*>(lds + o) = make_uint4(0u, 0u, 0u, 0u);

  // ---- staging: item j of a thread = float4 number tid + NT * j of the frame (of the workgroup's 64 co of it for `a`):
  // 4 consecutive pixels of channel (tid >> 4) + j * NT / 16
  const float4* const xsrc = reinterpret_cast<const float4*>(src) + tid;
  const float4* const asrc = reinterpret_cast<const float4*>(a + (size_t)cob * 64) + tid;
  const size_t xfr = (size_t)C * 16, afr = (size_t)Cout * 16;  // float4 per frame
  const int xi = tid & 15;
  const int xrow = (xi * 4) / W, xcol = (xi * 4) % W;
  const unsigned wofs = (unsigned)((tid >> 4) * PITCH + (xrow + 1) * RB + xcol * 2);
  const unsigned wofs_a = (unsigned)((tid >> 4) * kWgresAPitch + xi * 8);
  auto stage_x = [&](const float4 v, const int j, const unsigned bufoff) __attribute__((always_inline)) {
    unsigned d0[SPLIT], d1[SPLIT];
    wg_split_pair<SPLIT>(act_sel(v.x), act_sel(v.y), d0);
    wg_split_pair<SPLIT>(act_sel(v.z), act_sel(v.w), d1);
#pragma unroll
    for (int p = 0; p < SPLIT; ++p)
      *reinterpret_cast<uint2*>(lds + bufoff + wofs + (unsigned)(j * (NT / 16) * PITCH) + (unsigned)(p * COPYB)) = make_uint2(d0[p], d1[p]);
  };
  float bsum[AI];  // bias gradient: this thread's share of channel (tid >> 4) + j * NT / 16
#pragma unroll
  for (int j = 0; j < AI; ++j) bsum[j] = 0.f;
  auto stage_a = [&](const float4 v, const int j, const unsigned bufoff, const float keep) __attribute__((always_inline)) {
    bsum[j] += keep * ((v.x + v.y) + (v.z + v.w));
    unsigned d0[SPLIT], d1[SPLIT];
    wg_split_pair<SPLIT>(v.x, v.y, d0);
    wg_split_pair<SPLIT>(v.z, v.w, d1);
#pragma unroll
    for (int p = 0; p < SPLIT; ++p)
      *reinterpret_cast<uint2*>(lds_a + bufoff + wofs_a + (unsigned)(j * (NT / 16) * kWgresAPitch) + (unsigned)(p * APIECEB)) = make_uint2(d0[p], d1[p]);
  };

  // ---- the wave's tiles.  Its B operands come from TWO image rows per k-step, the outer one (ty = 0 for half 0, ty = 2
  // for half 1) and the centre one (ty = 1); the column taps are funnel shifts of those rows in registers (a lane's 8
  // pixels are whole plane rows, so a shifted row needs no neighbour).  Five B slots:
  //   0: outer row, tx = 0    1: outer, tx = 1    2: outer, tx = 2    3: centre, tx = (half 0: 0, half 1: 2)    4: centre, tx = 1
  // nine accumulators = (coA, slots 0-4) and (coB, slots 0-3); coA = co tile `half`: half 0 holds {co 0: taps 0-4, co 1: taps
  // 0-3}, half 1 {co 1: taps 6 7 8 5 4, co 0: taps 6 7 8 5}.
  const int coA = half, coB = half ^ 1;  // 32-channel tile of the co group
  const int tyo = half ? 2 : 0;
  const unsigned lane_b = (unsigned)((tci * 32 + il) * PITCH + kl * 16);
  const unsigned lane_a0 = (unsigned)((coA * 32 + il) * kWgresAPitch + kl * 16), lane_a1 = (unsigned)((coB * 32 + il) * kWgresAPitch + kl * 16);
  // W = 8: a fragment is one 16-byte row, rows ty apart are 16 bytes apart.  W = 4: a fragment is two 8-byte rows starting
  // at row ty: the outer one is 16-byte aligned, the centre one straddles -- it is put together from the outer fragment and
  // one more 8-byte row (`ext`).
  const unsigned outer_off = lane_b + (unsigned)(tyo * RB);
  const unsigned ext_off = lane_b + (W == 8 ? 16u : (half ? 8u : 16u));

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  u32x4 qa[2][2][SPLIT];  // [set][co tile][piece]
  u32x4 ro[2][SPLIT], rc[2][SPLIT];  // [set][piece]: outer row fragment; centre row fragment (W = 4: .xy = the extra row)
  auto operands = [&](const int q, const int set, const unsigned xoff, const unsigned aoff) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < SPLIT; ++p) {
      qa[set][0][p] = *reinterpret_cast<const u32x4*>(lds_a + aoff + lane_a0 + (unsigned)(p * APIECEB + q * 32));
      qa[set][1][p] = *reinterpret_cast<const u32x4*>(lds_a + aoff + lane_a1 + (unsigned)(p * APIECEB + q * 32));
      ro[set][p] = *reinterpret_cast<const u32x4*>(lds + xoff + outer_off + (unsigned)(p * COPYB + q * 32));
      if (W == 8) {
        rc[set][p] = *reinterpret_cast<const u32x4*>(lds + xoff + ext_off + (unsigned)(p * COPYB + q * 32));
      } else {
        const uint2 e = *reinterpret_cast<const uint2*>(lds + xoff + ext_off + (unsigned)(p * COPYB + q * 32));
        rc[set][p] = u32x4{e.x, e.y, 0u, 0u};
      }
    }
  };
  constexpr int FR = W == 8 ? 1 : 2;  // image rows per fragment
  auto shr1 = [](const u32x4 f) __attribute__((always_inline)) { return wg_rows_shift_in_front<FR>(f); };  // pixel x <- x - 1
  auto shl1 = [](const u32x4 f) __attribute__((always_inline)) { return wg_rows_shift_behind<FR>(f); };    // pixel x <- x + 1
  auto mfmas = [&](const int set) __attribute__((always_inline)) {
    u32x4 qb[5][SPLIT];
#pragma unroll
    for (int p = 0; p < SPLIT; ++p) {
      const u32x4 o = ro[set][p];
      u32x4 c = rc[set][p];
      if (W == 4) c = half ? u32x4{c.x, c.y, o.x, o.y} : u32x4{o.z, o.w, c.x, c.y};
      const u32x4 cl = shl1(c), cr = shr1(c);
      qb[0][p] = shr1(o);
      qb[1][p] = o;
      qb[2][p] = shl1(o);
      qb[3][p] = half ? cl : cr;
      qb[4][p] = c;
    }
    // product-major: consecutive MFMAs go to different accumulator tiles, so none waits for its predecessor
#pragma unroll
    for (int ord = SPLIT - 1; ord >= 0; --ord)
#pragma unroll
      for (int sa = 0; sa <= ord; ++sa)
#pragma unroll
        for (int j = 0; j < 9; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, qa[set][j < 5 ? 0 : 1][sa]),
                                                           __builtin_bit_cast(bf16x8, qb[j < 5 ? j : j - 5][ord - sa]), acc[j], 0, 0, 0);
  };

  // ---- raw frames: two register sets.  Set s is requested early in a frame and staged under the NEXT one, so every use
  // is at least three k-steps behind its request, and the requests of a frame follow its first staged item: whatever
  // counter value the compiler waits for there, nothing younger than a frame is in flight.
  // The requests are inline asm: the compiler sinks its own loads to their uses, a frame later (and then waits for them
  // there).  As volatile asm they keep their place among the LDS operations; raw_wait is the matching counter wait.
  constexpr int NI = XI + AI;
  wg_f32x4 raw[2][NI];  // [set][x items, a items]
  auto raw_load = [&](const int rs, const int n) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      const float4* const ptr = it < XI ? xsrc + (size_t)n * xfr + NT * it : asrc + (size_t)n * afr + NT * (it - XI);
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(raw[rs][it]) : "v"(ptr));
    }
  };
  auto raw_wait = [&](const int rs) __attribute__((always_inline)) { wg_raw_wait<0>(raw[rs]); };  // every request so far has landed
  auto stage = [&](const int rs, const int it, const unsigned xo, const unsigned ao, const float keep) __attribute__((always_inline)) {
    const float4 v = make_float4(raw[rs][it].x, raw[rs][it].y, raw[rs][it].z, raw[rs][it].w);
    if (it < XI) stage_x(v, it, xo); else stage_a(v, it - XI, ao, keep);
  };
  // staging order within a frame: x0 a0 x1 a1 x2 a2 x3 a3 [a4 ...]; item number of the k-th staged one
  auto item_of = [](const int k) __attribute__((always_inline)) { return k < 8 ? ((k & 1) ? XI + (k >> 1) : (k >> 1)) : XI + k - 4; };

  // ---- prologue: frame n0 staged into images 0, frame n0 + 1 requested into set 1
  raw_load(0, n0);
  raw_wait(0);
  raw_load(1, n0 + 1 < nlast ? n0 + 1 : nlast);
  lds_barrier();  // the zeroes are in place
#pragma unroll
  for (int k = 0; k < NI; ++k) stage(0, k, 0u, 0u, 1.f);
  lds_barrier();  // images 0 complete
  operands(0, 0, 0u, 0u);
  if (prof) prof[1] = __builtin_readcyclecounter();

  // One frame: par = parity of the frame within the workgroup's run (a literal at the call sites: image offsets and raw
  // sets are compile-time).  Images par hold frame n; raw set par ^ 1 holds frame n + 1, staged into images par ^ 1 under
  // k-steps 0-2; raw set par is free and receives frame n + 2.
  auto frame = [&](const int n, const int par) __attribute__((always_inline)) {
    const unsigned xoff = par ? (unsigned)XBUFB : 0u, xoth = (unsigned)XBUFB - xoff;
    const unsigned aoff = par ? (unsigned)ABUFB : 0u, aoth = (unsigned)ABUFB - aoff;
    const float keep = n + 1 < n1 ? 1.f : 0.f;  // the frame staged under the last one is a duplicate: keep it out of the bias sum
    const int nn2 = n + 2 < nlast ? n + 2 : nlast;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int set = q & 1;
      // operands of the NEXT k-step first: their LDS latency passes under this step's MFMAs
      if (q < 3) {
        operands(q + 1, set ^ 1, xoff, aoff);
      } else {
        lds_barrier();  // every wave has read these images and written the other ones
        operands(0, set ^ 1, xoth, aoth);
      }
      mfmas(set);
      if (q < 3) {
#pragma unroll
        for (int k = q * NI / 3; k < (q + 1) * NI / 3; ++k) {
          if (k == 0) raw_wait(par ^ 1);  // requested a frame ago, nothing younger in flight
          stage(par ^ 1, item_of(k), xoth, aoth, keep);
          if (k == 0) raw_load(par, nn2);
        }
      }
      // the fragment shifts, the staging and the next operands in the MFMAs' shadow: after every MFMA up to five VALU /
      // transcendental instructions, after every other one an LDS access (left to itself the scheduler issues the MFMAs in
      // runs: 5400 instead of 4600 cycles per frame, 6400 instead of 4900 on the 4-wide planes)
#pragma unroll
      for (int i = 0; i < 9 * (SPLIT == 2 ? 3 : 1); ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x402, 5, 0);
        if ((i & 1) == 0) __builtin_amdgcn_sched_group_barrier(0x080, 1, 0);
      }
    }
  };
#pragma unroll 1
  for (int n = n0; n < n1; n += 2) {
    frame(n, 0);
    if (n + 1 < n1) frame(n + 1, 1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped requests of the last frame
  if (prof) prof[2] = __builtin_readcyclecounter();

  if (part) {
    // accumulator order: float4 number ((wave * 9 + j) * 4 + r / 4) * 64 + lane of this workgroup's set -- every store
    // instruction writes 1 KiB in a row (WgRedRes::scatter maps it back to dwp)
    float4* const ps = reinterpret_cast<float4*>(part) + ((size_t)blockIdx.y * nbx + bx) * (wgres_set_floats(C) / 4) + (size_t)wave * (9 * 4 * 64) + lane;
#pragma unroll
    for (int j = 0; j < 9; ++j) wg_store_tile(ps + j * 256, acc[j]);
  } else {
    const int ci = tci * 32 + il;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int k = j < 5 ? j : j - 5;
      const int tap = k < 3 ? tyo * 3 + k : (k == 3 ? (half ? 5 : 3) : 4);
      const int cot = cob + (j < 5 ? coA : coB) * 32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wg_tile_row(r, kl, cot);
        atomicAdd(&dwp[((size_t)row * 9 + tap) * cpad + ci], acc[j][r]);
      }
    }
  }
  if (dbias != nullptr) {
#pragma unroll
    for (int j = 0; j < AI; ++j) {  // the 16 lanes of a DPP row share a channel
      const float v = wg_row16_sum(bsum[j]);
      if (xi == 0) {
        const int ch = (tid >> 4) + j * (NT / 16);
        if (part) part[((size_t)blockIdx.y * nbx + bx) * wgres_set_floats(C) + wgres_tile_floats(C) + ch] = v;
        else atomicAdd(&dbias[cob + ch], v);
      }
    }
  }
  if (prof) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    prof[3] = __builtin_readcyclecounter();
  }
}

template <int SPLIT, int C, int W>
__global__ __launch_bounds__(64 * 2 * (C / 32), 1) void conv3x3_wgrad_resident_kernel(
    const MtrssmConvGeom g, const float* __restrict__ a, const float* __restrict__ src, float* __restrict__ dwp,
    float* __restrict__ part, float* __restrict__ dbias, const int frames_per_wg) {
  conv3x3_wgrad_resident_body<SPLIT, C, W>(g.N, g.Cout, g.Cpad, g.act, g.pre_act, a, src, dwp, part, dbias, frames_per_wg, (int)blockIdx.x, (int)gridDim.x);
}

// Two problems of the same C and Cout in ONE grid (the audio and the vision stack's layer: WA- and WB-wide planes): x blocks
// 0 .. pa.xblocks - 1 run problem a, the rest problem b; every workgroup's run is twice as long as in two launches of their
// own, and the fixed part of a launch (ramp, zeroing the images, the first frame's round trip, the partial-set store, the
// drain) is paid once.  Half as many workgroups per problem = half as many partial sets.  The choice is uniform per workgroup:
// no barrier sits under a divergent branch.  Dynamic LDS: the larger of the two wgres_lds_bytes.
struct WgresProblem {
  const float* a;
  const float* src;
  float* dwp;
  float* part;    // this problem's partial sets [cogroups][xblocks] (NULL: fp32 atomics into dwp / dbias)
  float* dbias;
  int N, Cout, cpad, act, pre_act;  // of the problem's geometry
  int frames_per_wg, xblocks;
};
template <int SPLIT, int C, int WA, int WB>
__global__ __launch_bounds__(64 * 2 * (C / 32), 1) void conv3x3_wgrad_pair_resident_kernel(const WgresProblem pa, const WgresProblem pb) {
  const int bx = (int)blockIdx.x;
  if (bx < pa.xblocks) conv3x3_wgrad_resident_body<SPLIT, C, WA>(pa.N, pa.Cout, pa.cpad, pa.act, pa.pre_act, pa.a, pa.src, pa.dwp, pa.part, pa.dbias, pa.frames_per_wg, bx, pa.xblocks);
  else conv3x3_wgrad_resident_body<SPLIT, C, WB>(pb.N, pb.Cout, pb.cpad, pb.act, pb.pre_act, pb.a, pb.src, pb.dwp, pb.part, pb.dbias, pb.frames_per_wg, bx - pa.xblocks, pb.xblocks);
}

// Partial sets of conv3x3_wgrad_resident_body (and its pair form): float4 f = ((wave * 9 + j) * 4 + gq) * 64 + lane, then the
// 64 bias sums of the co group (16 float4 of the bias block's 32).
template <int C>
struct WgRedRes {
  static constexpr int NL = 32, NG = 8, U = 4, KS = 1, SET4 = wgres_set_floats(C) / 4, TILE4 = wgres_tile_floats(C) / 4;
  static_assert(TILE4 % NL == 0, "whole blocks");  // host: grid.x * 32 == TILE4 (+ 32: the bias block)
  static __device__ __forceinline__ WgRedCol column(const int f, const int by) {
    return {(size_t)f, 0, f >= TILE4 ? by * 64 + 4 * (f - TILE4) : -1, f >= SET4};
  }
  // rows cot + 8 gq + 4 kl + {0..3}, tap, ci (the kernel's tile assignment)
  static __device__ __forceinline__ void scatter(const int f, const int by, const float4 v, const int cpad, float* __restrict__ dwp) {
    const int lane = f & 63, gq = (f >> 6) & 3, wj = f >> 8, j = wj % 9, wave = wj / 9;
    const int il = lane & 31, kl = lane >> 5, tci = wave >> 1, half = wave & 1;
    const int k = j < 5 ? j : j - 5, tap = k < 3 ? (half ? 6 : 0) + k : (k == 3 ? (half ? 5 : 3) : 4);
    const int row = by * 64 + (j < 5 ? half : half ^ 1) * 32 + 8 * gq + 4 * kl;
    wg_red_add_rows(dwp + ((size_t)row * 9 + tap) * cpad + tci * 32 + il, (size_t)9 * cpad, v);
  }
};

// ------------------------------------------------------------------------------------------------
// Weight gradient of the 1x1 layers of the residual stacks on 64-pixel planes (64 -> 64 in the encoders, 128 -> 64 in the
// decoders), operands staged once per frame as in conv3x3_wgrad_resident_kernel:
//   dW[co][ci] = sum over frames n and pixels p of  a[n][co][p] * act(src)[n][ci][p]
// The register-direct kernel (conv_split.h: conv1x1_weight_grad_split_kernel) converts every `a` element once per ci tile
// and every src element once per co tile (2x - 4x) on one wave per SIMD, and a single wave issues a VALU instruction every
// ~5 cycles (tools/micro/mfma_shadow.hip): it is conversion-bound at about half the HBM rate.  Here a workgroup of EIGHT
// waves (two per SIMD issue twice the VALU instructions per cycle) owns a run of frames; every thread loads, activates
// and splits its share of each frame exactly once (coalesced 16-byte loads, requested TWO frames ahead through three
// register sets: one frame in flight per CU does not cover the HBM latency at this rate) and writes it to
// double-buffered [channel][64 pixels + 8] bf16 images; the MFMA work is small (6 or 12 per wave and frame): wave w holds
// tile w % NTILE and, with four tiles, half of the k-steps of every frame.  One barrier per frame; partial tiles stored
// (32 KiB per workgroup) and summed by wgrad_reduce_batch_kernel (layout WgRed1x1), or by fp32 atomics when part == NULL.
// ------------------------------------------------------------------------------------------------
template <int SPLIT, int C>
__host__ __device__ constexpr int wg1x1_lds_bytes() { return 2 * SPLIT * (64 + C) * kWgresAPitch; }

template <int SPLIT, int C>
__global__ __launch_bounds__(512, 1) void conv1x1_wgrad_staged_kernel(
    const MtrssmConvGeom g, const float* __restrict__ a, const float* __restrict__ src, float* __restrict__ dwp,
    float* __restrict__ part, float* __restrict__ dbias, const int frames_per_wg) {
  static_assert(SPLIT == 1 || SPLIT == 2, "one or two bf16 pieces");
  static_assert(C == 64 || C == 128, "input channels");
  constexpr int NT = 512, P = kWgresAPitch;
  constexpr int XI = C * 16 / NT, AI = 2, NI = XI + AI;  // float4 items per thread and frame: src, a (64 co * 16)
  constexpr int NTILE = 2 * (C / 32), KS = 8 / NTILE;    // tiles per co group; waves per tile (each 4 / KS k-steps of a frame)
  constexpr int APB = 64 * P, XPB = C * P;               // bytes of one piece of the a / src image
  constexpr int BUFB = SPLIT * (APB + XPB);              // one buffer: [a pieces][src pieces]
  extern __shared__ __attribute__((aligned(16))) unsigned char wg1_lds[];
  unsigned char* const lds = wg1_lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int il = lane & 31, kl = lane >> 5;
  const int tile = wave % NTILE, kpart = wave / NTILE;
  const int tco = tile & 1, tci = tile >> 1;
  const int n0 = blockIdx.x * frames_per_wg;
  const int n1 = n0 + frames_per_wg < g.N ? n0 + frames_per_wg : g.N;
  if (n0 >= n1) return;  // whole workgroup
  const int nlast = n1 - 1;
  const int cob = blockIdx.y * 64;
  unsigned long long* const prof = (tid == 0 && blockIdx.y == 0 && g_res_prof) ? (blockIdx.x == 0 ? g_res_prof + 32 : (blockIdx.x == gridDim.x / 2 ? g_res_prof + 40 : nullptr)) : nullptr;
  if (prof) prof[0] = __builtin_readcyclecounter();

  const bool act_elu = g.act == MTRSSM_ACT_ELU, act_relu = g.act == MTRSSM_ACT_RELU, pre = g.pre_act != 0;
  const WgActSel act_sel{act_elu, act_relu, pre};

  // staging: item j = float4 number tid + 512 j of the frame: 4 consecutive pixels of channel (tid >> 4) + 32 j
  const float4* const xsrc = reinterpret_cast<const float4*>(src) + tid;
  const float4* const asrc = reinterpret_cast<const float4*>(a + (size_t)cob * 64) + tid;
  const size_t xfr = (size_t)C * 16, afr = (size_t)g.Cout * 16;  // float4 per frame
  const unsigned wofs = (unsigned)((tid >> 4) * P + (tid & 15) * 8);
  float bsum[AI];
#pragma unroll
  for (int j = 0; j < AI; ++j) bsum[j] = 0.f;
  wg_f32x4 raw[3][NI];  // [set][a items, x items]
  auto raw_load = [&](const int rs, const int n) __attribute__((always_inline)) { wg_raw_load<NT, AI, XI>(raw[rs], asrc, afr, xsrc, xfr, n); };
  auto raw_wait = [&](const int rs) __attribute__((always_inline)) { wg_raw_wait<2 * NI>(raw[rs]); };  // the two younger sets may still be in flight
  auto stage = [&](const int rs, const unsigned bufoff) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      const wg_f32x4 v = raw[rs][it];
      unsigned d0[SPLIT], d1[SPLIT];
      if (it < AI) {
        bsum[it] += (v.x + v.y) + (v.z + v.w);
        wg_split_pair<SPLIT>(v.x, v.y, d0);
        wg_split_pair<SPLIT>(v.z, v.w, d1);
      } else {
        wg_split_pair<SPLIT>(act_sel(v.x), act_sel(v.y), d0);
        wg_split_pair<SPLIT>(act_sel(v.z), act_sel(v.w), d1);
      }
      const unsigned base = it < AI ? (unsigned)(it * 32 * P) : (unsigned)(SPLIT * APB + (it - AI) * 32 * P);
      const unsigned piece = it < AI ? (unsigned)APB : (unsigned)XPB;
#pragma unroll
      for (int p = 0; p < SPLIT; ++p) *reinterpret_cast<uint2*>(lds + bufoff + base + wofs + p * piece) = make_uint2(d0[p], d1[p]);
    }
  };

  const unsigned lane_a = (unsigned)((tco * 32 + il) * P + kl * 16);
  const unsigned lane_b = (unsigned)(SPLIT * APB + (tci * 32 + il) * P + kl * 16);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  raw_load(0, n0);
  raw_load(1, n0 + 1 < nlast ? n0 + 1 : nlast);
  if (prof) prof[1] = __builtin_readcyclecounter();
  // One frame: rs = (n - n0) % 3 and par = (n - n0) & 1 are literals at the call sites.
  auto frame = [&](const int n, const int rs, const int par) __attribute__((always_inline)) {
    const unsigned bufoff = par ? (unsigned)BUFB : 0u;
    raw_load((rs + 2) % 3, n + 2 < nlast ? n + 2 : nlast);  // its set held frame n - 1, staged a frame ago
    raw_wait(rs);
    stage(rs, bufoff);
    lds_barrier();  // images par complete; every wave is done reading images par ^ 1 (frame n - 1)
#pragma unroll
    for (int qq = 0; qq < 4 / KS; ++qq) {
      const int q = kpart * (4 / KS) + qq;
      u32x4 qa[SPLIT], qb[SPLIT];
#pragma unroll
      for (int p = 0; p < SPLIT; ++p) {
        qa[p] = *reinterpret_cast<const u32x4*>(lds + bufoff + lane_a + (unsigned)(p * APB) + (unsigned)(q * 32));
        qb[p] = *reinterpret_cast<const u32x4*>(lds + bufoff + lane_b + (unsigned)(p * XPB) + (unsigned)(q * 32));
      }
      wg_mfma_pieces<SPLIT>(acc, qa, qb);
    }
  };
#pragma unroll 1
  for (int n = n0; n < n1; n += 6) {
    frame(n, 0, 0);
    if (n + 1 < n1) frame(n + 1, 1, 1);
    if (n + 2 < n1) frame(n + 2, 2, 0);
    if (n + 3 < n1) frame(n + 3, 0, 1);
    if (n + 4 < n1) frame(n + 4, 1, 0);
    if (n + 5 < n1) frame(n + 5, 2, 1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped requests of the last frames
  if (prof) prof[2] = __builtin_readcyclecounter();

  if (part) {
    // one tile per wave, accumulator order: float4 number (wave * 4 + r / 4) * 64 + lane of this workgroup's set (2048 atomic
    // adders per address took 9-27 us of a 41 us launch; wgrad_reduce_batch_kernel sums the sets behind this kernel)
    float4* const ps = reinterpret_cast<float4*>(part) + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (kWg1x1SetFloats / 4) + (size_t)wave * 256 + lane;
    wg_store_tile(ps, acc);
  } else {
    const int ci = tci * 32 + il;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wg_tile_row(r, kl, cob + tco * 32);
      atomicAdd(&dwp[(size_t)row * g.Cpad + ci], acc[r]);
    }
  }
  if (dbias != nullptr) {
#pragma unroll
    for (int j = 0; j < AI; ++j) {  // the 16 lanes of a DPP row share a channel
      const float v = wg_row16_sum(bsum[j]);
      if ((tid & 15) == 0) {
        const int ch = (tid >> 4) + j * 32;
        if (part) part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kWg1x1SetFloats + 8 * 1024 + ch] = v;
        else atomicAdd(&dbias[cob + ch], v);
      }
    }
  }
  if (prof) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    prof[3] = __builtin_readcyclecounter();
  }
}

// Partial tiles of conv1x1_wgrad_staged_kernel and conv1x1_bwd_fused_body (a set = [8 waves][256] float4, accumulator order,
// then 64 bias sums); a workgroup's waves w and w + NTILE hold the same tile (k-halves): 8 / NTILE x S slices per tile.
template <int C>
struct WgRed1x1 {
  static constexpr int NTILE = 2 * (C / 32), TILE4 = 256;
  static constexpr int NL = 32, NG = 8, U = 4, KS = 8 / NTILE, SET4 = kWg1x1SetFloats / 4;  // host: grid.x * 32 == NTILE * 256 (+ 32)
  static __device__ __forceinline__ WgRedCol column(const int f, const int by) {
    const int fb = f - NTILE * TILE4;  // >= 0: the bias block, 16 float4 of it in use
    return {(size_t)(fb >= 0 ? 8 * TILE4 + fb : f), NTILE * TILE4, fb >= 0 ? by * 64 + 4 * fb : -1, fb >= 16};
  }
  static __device__ __forceinline__ void scatter(const int f, const int by, const float4 v, const int cpad, float* __restrict__ dwp) {
    const int tile = f / TILE4, ft = f - tile * TILE4;
    const int lane = ft & 63, gq = ft >> 6, il = lane & 31, kl = lane >> 5;
    const int tco = tile & 1, tci = tile >> 1;
    wg_red_add_rows(dwp + (size_t)(by * 64 + tco * 32 + 8 * gq + 4 * kl) * cpad + tci * 32 + il, (size_t)cpad, v);
  }
};

// ------------------------------------------------------------------------------------------------
// The WHOLE backward of a residual block's 1x1 layer (C = 128 or 64 mid channels -> 64, 64-pixel planes, two bf16 pieces) in
// one pass over g_y (`a`) and h (`src`):
//   g_h[n][m][p] = (sum_o W1[o][m] g_y[n][o][p]) * act'(h[n][m][p])     dW1[o][m] = sum g_y[n][o][p] act(h)[n][m][p]     db1[o] = sum g_y
// conv1x1_stream_kernel<64, C, false> followed by conv1x1_wgrad_staged_kernel<2, C> streams both tensors twice (8 / 5 units
// of one 64-channel tensor per block pair); this is conv1x1_wgrad_staged_kernel<2, C> -- same staging, same tiles, same
// partial sets and bias sums, so the same reduce -- with the backward-data product added from the frame it has in LDS
// (5 / 3 units).  Its B operand wants k = output channel, lane = pixel: the staging threads also write a PIXEL-major image of
// g_y's pieces ([pixel][64 channels + 8], 18 KB per buffer), a fragment is one 16-byte read.  A operands: wave w owns the
// 32-channel tile w >> 1 of g_h for the pixel half w & 1 (C = 64: waves 4 - 7 repeat the products of waves 0 - 3 and do not
// store), its rows of W1^T in 32 registers for the whole launch.  Products per k-block in conv1x1_stream_kernel's order
// (a0 bl, a1 bh, a0 bh), k-blocks in channel order, the same pieces: g_h is bit-identical to that kernel's.  act'(h) comes
// from the fp32 h in accumulator layout, requested a frame ahead (an L2 hit: the workgroup has just loaded the frame).
// Counter waits: every load of the loop is inline asm in a fixed order -- frame n issues [act' operand of n + 1][raw set
// n + 2] -- and a wait names the number of LOADS issued behind the one it needs (loads return in order among themselves;
// the g_h stores share the counter, return in an order of their own and can only make a wait longer).
// ------------------------------------------------------------------------------------------------
template <int C>
__host__ __device__ constexpr int bwd1x1_lds_bytes() { return wg1x1_lds_bytes<2, C>() + 2 * 2 * 64 * kWgresAPitch; }

// One problem's work of workgroup bx (its run of frames_per_wg frames); `act` and `cpad` are the geometry's.
template <int C>
__device__ __forceinline__ void conv1x1_bwd_fused_body(
    const int N, const int act, const int cpad, const float* __restrict__ a, const float* __restrict__ src,
    const unsigned short* __restrict__ wq, float* __restrict__ gh, float* __restrict__ dwp, float* __restrict__ part,
    float* __restrict__ dbias, const int frames_per_wg, const int bx) {
  static_assert(C == 64 || C == 128, "mid channels");
  constexpr int SPLIT = 2, NT = 512, P = kWgresAPitch;
  constexpr int XI = C * 16 / NT, AI = 2, NI = XI + AI;  // float4 items per thread and frame: src (h), a (g_y: 64 co * 16)
  constexpr int NTILE = 2 * (C / 32), KS = 8 / NTILE;
  constexpr int APB = 64 * P, XPB = C * P;
  constexpr int BUFB = SPLIT * (APB + XPB);              // one buffer: [a pieces][src pieces]
  constexpr int PMB = 64 * P, PMBUF = SPLIT * PMB;       // pixel-major g_y image: one piece, one buffer
  constexpr int PM0 = 2 * BUFB;                          // [buffer 0][buffer 1][pixel-major 0][pixel-major 1]
  extern __shared__ __attribute__((aligned(16))) unsigned char bw1_lds[];
  unsigned char* const lds = bw1_lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int il = lane & 31, kl = lane >> 5;
  const int tile = wave % NTILE, kpart = wave / NTILE;
  const int tco = tile & 1, tci = tile >> 1;
  const int n0 = bx * frames_per_wg;
  const int n1 = n0 + frames_per_wg < N ? n0 + frames_per_wg : N;
  if (n0 >= n1) return;  // whole workgroup
  const int nlast = n1 - 1;

  const bool act_elu = act == MTRSSM_ACT_ELU, act_relu = act == MTRSSM_ACT_RELU;
  auto act_sel = [&](float x) __attribute__((always_inline)) {
    float e = __expf(x) - 1.f;
    asm volatile("" : "+v"(e));  // computed unconditionally: the compiler would branch around the exponential
    const float neg = act_elu ? e : (act_relu ? 0.f : x);
    return x > 0.f ? x : neg;
  };

  // backward-data job of this wave: g_h channels bct * 32 .. + 31, pixels bhalf * 32 .. + 31
  const int bct = (wave >> 1) % (C / 32), bhalf = wave & 1;
  const bool bstore = C == 128 || wave < 4;
  u32x4 wa[4][2];  // [k-block][piece]: row bct * 32 + il of W1^T, output channels cb * 16 + 8 kl .. + 7
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) {
      wa[cb][sp] = *reinterpret_cast<const u32x4*>(wq + (size_t)sp * (C * 64) + (size_t)(bct * 32 + il) * 64 + cb * 16 + 8 * kl);
      asm volatile("" : "+v"(wa[cb][sp]));  // landed here: no compiler-made wait for them inside the loop
    }

  const float4* const xsrc = reinterpret_cast<const float4*>(src) + tid;
  const float4* const asrc = reinterpret_cast<const float4*>(a) + tid;
  constexpr size_t xfr = (size_t)C * 16, afr = (size_t)64 * 16;  // float4 per frame
  const unsigned wofs = (unsigned)((tid >> 4) * P + (tid & 15) * 8);
  const unsigned pofs = (unsigned)(PM0 + 4 * (tid & 15) * P + (tid >> 4) * 2);  // pixel 4 (tid & 15), channel tid >> 4
  float bsum[AI];
#pragma unroll
  for (int j = 0; j < AI; ++j) bsum[j] = 0.f;
  wg_f32x4 raw[3][NI];  // [set][a items, x items]
  auto raw_load = [&](const int rs, const int n) __attribute__((always_inline)) { wg_raw_load<NT, AI, XI>(raw[rs], asrc, afr, xsrc, xfr, n); };
  auto raw_wait = [&](const int rs) __attribute__((always_inline)) { wg_raw_wait<2 * NI + 2 * 16>(raw[rs]); };  // loads behind this set: 2 raw sets + 2 act' sets
  // act' operand: h in accumulator layout (row (r & 3) + 8 (r >> 2) + 4 kl of the wave's channel tile, this lane's pixel)
  const float* const hop = src + (size_t)(bct * 32 + 4 * kl) * 64 + bhalf * 32 + il;
  float* const ghp = gh + (size_t)(bct * 32 + 4 * kl) * 64 + bhalf * 32 + il;
  float opv[2][16];
  auto op_load = [&](const int os, const int n) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* const ptr = hop + (size_t)n * (C * 64) + ((r & 3) + 8 * (r >> 2)) * 64;
      asm volatile("global_load_dword %0, %1, off" : "=v"(opv[os][r]) : "v"(ptr));
    }
  };
  auto op_wait = [&](const int os) __attribute__((always_inline)) {  // loads behind this set: 2 raw sets + 1 act' set
#define MTRSSM_OPV(os_, b_) "+v"(opv[os_][b_]), "+v"(opv[os_][b_ + 1]), "+v"(opv[os_][b_ + 2]), "+v"(opv[os_][b_ + 3]), "+v"(opv[os_][b_ + 4]), \
                            "+v"(opv[os_][b_ + 5]), "+v"(opv[os_][b_ + 6]), "+v"(opv[os_][b_ + 7])
    asm volatile("s_waitcnt vmcnt(%8)" : MTRSSM_OPV(os, 0) : "n"(2 * NI + 16));
    asm volatile("" : MTRSSM_OPV(os, 8));  // (volatile: stays behind the wait)
#undef MTRSSM_OPV
  };
  auto stage = [&](const int rs, const unsigned bufoff, const unsigned pmoff) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      const wg_f32x4 v = raw[rs][it];
      unsigned d0[SPLIT], d1[SPLIT];
      if (it < AI) {
        bsum[it] += (v.x + v.y) + (v.z + v.w);
        wg_split_pair<SPLIT>(v.x, v.y, d0);
        wg_split_pair<SPLIT>(v.z, v.w, d1);
#pragma unroll
        for (int p = 0; p < SPLIT; ++p) {  // the pixel-major copy: channel (tid >> 4) + 32 it of pixels 4 (tid & 15) .. + 3
          unsigned char* const q = lds + pmoff + pofs + (unsigned)(it * 64 + p * PMB);
          *reinterpret_cast<unsigned short*>(q) = (unsigned short)(d0[p] & 0xffffu);
          *reinterpret_cast<unsigned short*>(q + P) = (unsigned short)(d0[p] >> 16);
          *reinterpret_cast<unsigned short*>(q + 2 * P) = (unsigned short)(d1[p] & 0xffffu);
          *reinterpret_cast<unsigned short*>(q + 3 * P) = (unsigned short)(d1[p] >> 16);
        }
      } else {
        wg_split_pair<SPLIT>(act_sel(v.x), act_sel(v.y), d0);
        wg_split_pair<SPLIT>(act_sel(v.z), act_sel(v.w), d1);
      }
      const unsigned base = it < AI ? (unsigned)(it * 32 * P) : (unsigned)(SPLIT * APB + (it - AI) * 32 * P);
      const unsigned piece = it < AI ? (unsigned)APB : (unsigned)XPB;
#pragma unroll
      for (int p = 0; p < SPLIT; ++p) *reinterpret_cast<uint2*>(lds + bufoff + base + wofs + p * piece) = make_uint2(d0[p], d1[p]);
    }
  };

  const unsigned lane_a = (unsigned)((tco * 32 + il) * P + kl * 16);
  const unsigned lane_b = (unsigned)(SPLIT * APB + (tci * 32 + il) * P + kl * 16);
  const unsigned lane_p = (unsigned)(PM0 + (bhalf * 32 + il) * P + kl * 16);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  raw_load(0, n0);
  op_load(0, n0);
  raw_load(1, n0 + 1 < nlast ? n0 + 1 : nlast);
  // One frame: rs = (n - n0) % 3 and par = (n - n0) & 1 are literals at the call sites.
  auto frame = [&](const int n, const int rs, const int par) __attribute__((always_inline)) {
    const unsigned bufoff = par ? (unsigned)BUFB : 0u, pmoff = par ? (unsigned)PMBUF : 0u;
    op_load(par ^ 1, n + 1 < nlast ? n + 1 : nlast);        // its set held frame n - 1's, used a frame ago
    raw_load((rs + 2) % 3, n + 2 < nlast ? n + 2 : nlast);  // its set held frame n - 1, staged a frame ago
    raw_wait(rs);
    stage(rs, bufoff, pmoff);
    lds_barrier();  // images par complete; every wave is done reading images par ^ 1 (frame n - 1)
#pragma unroll
    for (int qq = 0; qq < 4 / KS; ++qq) {
      const int q = kpart * (4 / KS) + qq;
      u32x4 qa[SPLIT], qb[SPLIT];
#pragma unroll
      for (int p = 0; p < SPLIT; ++p) {
        qa[p] = *reinterpret_cast<const u32x4*>(lds + bufoff + lane_a + (unsigned)(p * APB) + (unsigned)(q * 32));
        qb[p] = *reinterpret_cast<const u32x4*>(lds + bufoff + lane_b + (unsigned)(p * XPB) + (unsigned)(q * 32));
      }
      wg_mfma_pieces<SPLIT>(acc, qa, qb);
    }
    // backward-data: 4 k-blocks of 16 output channels x 3 products
    f32x16 accb;
#pragma unroll
    for (int r = 0; r < 16; ++r) accb[r] = 0.f;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const bf16x8 bh = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(lds + pmoff + lane_p + (unsigned)(cb * 32)));
      const bf16x8 bl = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(lds + pmoff + lane_p + (unsigned)(PMB + cb * 32)));
      accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wa[cb][0]), bl, accb, 0, 0, 0);
      accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wa[cb][1]), bh, accb, 0, 0, 0);
      accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wa[cb][0]), bh, accb, 0, 0, 0);
    }
    op_wait(par);
    if (bstore) {  // wave-uniform
      float* const o = ghp + (size_t)n * (C * 64);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float x = opv[par][r];
        const float e = __expf(x);
        const float neg = act_elu ? e : (act_relu ? 0.f : 1.f);
        o[((r & 3) + 8 * (r >> 2)) * 64] = accb[r] * (x > 0.f ? 1.f : neg);
      }
    }
  };
#pragma unroll 1
  for (int n = n0; n < n1; n += 6) {
    frame(n, 0, 0);
    if (n + 1 < n1) frame(n + 1, 1, 1);
    if (n + 2 < n1) frame(n + 2, 2, 0);
    if (n + 3 < n1) frame(n + 3, 0, 1);
    if (n + 4 < n1) frame(n + 4, 1, 0);
    if (n + 5 < n1) frame(n + 5, 2, 1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped requests of the last frames

  if (part) {  // the partial set of conv1x1_wgrad_staged_kernel: layout WgRed1x1 of the reduce
    float4* const ps = reinterpret_cast<float4*>(part) + (size_t)bx * (kWg1x1SetFloats / 4) + (size_t)wave * 256 + lane;
    wg_store_tile(ps, acc);
  } else {
    const int ci = tci * 32 + il;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = tco * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
      atomicAdd(&dwp[(size_t)row * cpad + ci], acc[r]);
    }
  }
  if (dbias != nullptr) {
#pragma unroll
    for (int j = 0; j < AI; ++j) {  // the 16 lanes of a DPP row share a channel
      const float v = wg_row16_sum(bsum[j]);
      if ((tid & 15) == 0) {
        const int ch = (tid >> 4) + j * 32;
        if (part) part[(size_t)bx * kWg1x1SetFloats + 8 * 1024 + ch] = v;
        else atomicAdd(&dbias[ch], v);
      }
    }
  }
}

template <int C>
__global__ __launch_bounds__(512, 1) void conv1x1_bwd_fused_kernel(
    const MtrssmConvGeom g, const float* __restrict__ a, const float* __restrict__ src, const unsigned short* __restrict__ wq,
    float* __restrict__ gh, float* __restrict__ dwp, float* __restrict__ part, float* __restrict__ dbias, const int frames_per_wg) {
  conv1x1_bwd_fused_body<C>(g.N, g.act, g.Cpad, a, src, wq, gh, dwp, part, dbias, frames_per_wg, (int)blockIdx.x);
}

// Two problems of the same C in ONE grid (the audio and the vision stack's block; the kernel does not depend on the plane's
// shape): workgroups 0 .. pa.xblocks - 1 run problem a, the rest problem b.  The problem is picked by scalar selects and the
// body instantiated once; each frame's g_h is computed as in a launch of its own, bit for bit.
struct Bwd1x1Problem {
  const float* a;
  const float* src;
  const unsigned short* wq;
  float* gh;
  float* dwp;
  float* part;    // this problem's partial sets [xblocks] (NULL: fp32 atomics into dwp / dbias)
  float* dbias;
  int N, act, cpad, frames_per_wg, xblocks;
};
template <int C>
__global__ __launch_bounds__(512, 1) void conv1x1_bwd_fused_pair_kernel(const Bwd1x1Problem pa, const Bwd1x1Problem pb) {
  const bool first = (int)blockIdx.x < pa.xblocks;  // workgroup-uniform
  conv1x1_bwd_fused_body<C>(first ? pa.N : pb.N, first ? pa.act : pb.act, first ? pa.cpad : pb.cpad, first ? pa.a : pb.a,
                            first ? pa.src : pb.src, first ? pa.wq : pb.wq, first ? pa.gh : pb.gh, first ? pa.dwp : pb.dwp,
                            first ? pa.part : pb.part, first ? pa.dbias : pb.dbias, first ? pa.frames_per_wg : pb.frames_per_wg,
                            first ? (int)blockIdx.x : (int)blockIdx.x - pa.xblocks);
}

// ------------------------------------------------------------------------------------------------
// Weight gradient of the second encoder layer (3x3 / stride 2 / pad 1, 8 -> 16 channels, 256-pixel output planes: 16x16
// vision, 32x8 audio), staged like the kernels above:
//   dW[co][ky][kx][ci] = sum over frames n and output pixels (oy, ox) of  a[n][co][oy][ox] * act(src)[n][ci][2 oy + ky - 1][2 ox + kx - 1]
// The patch-staged kernel (conv_split.h: conv_weight_grad_split_kernel<1, 2>) gathers its patches by 4-byte loads and runs
// at 0.13 of the HBM rate (235-246 us for 157 MB).  Here every frame of `a` (16 x 256) and of src (8 x 2Ho x 2Wo) is loaded
// once with coalesced 16-byte loads (eight waves, requests two frames ahead through three register sets), converted once and
// written to LDS; src DE-INTERLEAVED by column parity (even / odd image, one zero halo row on top of every plane), so that the
// 8 consecutive output pixels of a lane's B fragment are 8 consecutive elements: kx = 1 reads the even image at ox, kx = 2 the
// odd image at ox, kx = 0 the odd image at ox - 1 = a funnel shift of the kx = 2 fragment with one more element in front.
// MFMA columns are (tap, ci) pairs, 72 of them in three 32-column tiles; rows are the 16 co (the upper half of the 32-row
// tile is unused).  Wave w: column tile w & 3 (3: staging only), k-steps (w >> 2) * 8 .. + 8 of the frame's 16.  Partial set:
// float4 number (w * 2 + r / 4) * 64 + lane, r < 8, + 16 bias sums.
// ------------------------------------------------------------------------------------------------
constexpr int kWgS2SetFloats = 8 * 2 * 64 * 4 + 16;
template <int WO>
__host__ __device__ constexpr int wgs2_cip() { return (((256 / WO * 2 + 1) * (2 * WO)) / 16 | 1) * 16; }  // bytes per channel of one src image: odd in 16-byte slots
template <int SPLIT, int WO>
__host__ __device__ constexpr int wgs2_lds_bytes() { return 2 * SPLIT * (2 * 8 * wgs2_cip<WO>() + 16 * 528); }

template <int SPLIT, int WO>
__global__ __launch_bounds__(512, 1) void conv3x3s2_wgrad_staged_kernel(
    const MtrssmConvGeom g, const float* __restrict__ a, const float* __restrict__ src, float* __restrict__ dwp,
    float* __restrict__ part, float* __restrict__ dbias, const int frames_per_wg) {
  static_assert(SPLIT == 1 || SPLIT == 2, "one or two bf16 pieces");
  static_assert(WO == 16 || WO == 8, "output plane 16x16 or 32x8");
  constexpr int NT = 512, C = 8, CO = 16, HO = 256 / WO, HS = 2 * HO, WS = 2 * WO;
  constexpr int ROWB = WS;                 // bytes per row of one parity image: WS / 2 bf16
  constexpr int CIP = wgs2_cip<WO>();      // bytes per channel: (HS + 1) rows, padded
  constexpr int XCOPY = C * CIP;           // one parity image of one piece
  constexpr int AP = 528, APB = CO * AP;   // `a` image: [co][256 pixels + 8] bf16
  constexpr int BUFB = SPLIT * (2 * XCOPY + APB);  // one buffer: [piece][even image][odd image] then [piece][a image]
  constexpr int XI = C * HS * WS / 4 / NT, AI = CO * 256 / 4 / NT, NI = XI + AI;  // 4 + 2 float4 items per thread and frame
  extern __shared__ __attribute__((aligned(16))) unsigned char wgs2_lds[];
  unsigned char* const lds = wgs2_lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int il = lane & 31, kl = lane >> 5;
  const int ct = wave & 3, kh = wave >> 2;
  const int n0 = blockIdx.x * frames_per_wg;
  const int n1 = n0 + frames_per_wg < g.N ? n0 + frames_per_wg : g.N;
  if (n0 >= n1) return;  // whole workgroup
  const int nlast = n1 - 1;

  const bool act_elu = g.act == MTRSSM_ACT_ELU, act_relu = g.act == MTRSSM_ACT_RELU, pre = g.pre_act != 0;
  const WgActSel act_sel{act_elu, act_relu, pre};

  // zero both buffers once: the halo rows are never written again
  for (int o = tid * 16; o < 2 * BUFB; o += NT * 16) *reinterpret_cast<uint4*>(lds + o) = make_uint4(0u, 0u, 0u, 0u);

  // staging: src item j = float4 number tid + 512 j of the frame = 4 consecutive columns c0 .. c0 + 3 of one row of one
  // channel; `a` item j = 4 consecutive pixels of channel tid / 64 + 8 j
  const float4* const xsrc = reinterpret_cast<const float4*>(src) + tid;
  const float4* const asrc = reinterpret_cast<const float4*>(a) + tid;
  constexpr size_t xfr = (size_t)C * HS * WS / 4, afr = (size_t)CO * 256 / 4;  // float4 per frame
  float bsum[AI];
#pragma unroll
  for (int j = 0; j < AI; ++j) bsum[j] = 0.f;
  wg_f32x4 raw[3][NI];  // [set][a items, src items]
  auto raw_load = [&](const int rs, const int n) __attribute__((always_inline)) { wg_raw_load<NT, AI, XI>(raw[rs], asrc, afr, xsrc, xfr, n); };
  auto raw_wait = [&](const int rs) __attribute__((always_inline)) { wg_raw_wait<2 * NI>(raw[rs]); };  // the two younger sets may still be in flight
  auto stage = [&](const int rs, const unsigned bufoff) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      const wg_f32x4 v = raw[rs][it];
      if (it < AI) {
        bsum[it] += (v.x + v.y) + (v.z + v.w);
        unsigned d0[SPLIT], d1[SPLIT];
        wg_split_pair<SPLIT>(v.x, v.y, d0);
        wg_split_pair<SPLIT>(v.z, v.w, d1);
        const int f = tid + NT * it;  // co = f / 64, pixel = 4 (f % 64)
        const unsigned o = bufoff + (unsigned)(SPLIT * 2 * XCOPY) + (unsigned)((f >> 6) * AP + (f & 63) * 8);
#pragma unroll
        for (int p = 0; p < SPLIT; ++p) *reinterpret_cast<uint2*>(lds + o + p * APB) = make_uint2(d0[p], d1[p]);
      } else {
        unsigned de[SPLIT], dd[SPLIT];  // even columns (c0, c0 + 2), odd columns (c0 + 1, c0 + 3)
        wg_split_pair<SPLIT>(act_sel(v.x), act_sel(v.z), de);
        wg_split_pair<SPLIT>(act_sel(v.y), act_sel(v.w), dd);
        const int f = tid + NT * (it - AI);
        const int ci = f / (HS * WS / 4), rem = f - ci * (HS * WS / 4), row = rem / (WS / 4), c4 = rem - row * (WS / 4);
        const unsigned o = bufoff + (unsigned)(ci * CIP + (row + 1) * ROWB + c4 * 4);  // columns c0 / 2, c0 / 2 + 1 of the parity images
#pragma unroll
        for (int p = 0; p < SPLIT; ++p) {
          *reinterpret_cast<unsigned*>(lds + o + p * 2 * XCOPY) = de[p];
          *reinterpret_cast<unsigned*>(lds + o + p * 2 * XCOPY + XCOPY) = dd[p];
        }
      }
    }
  };

  // the lane's column of the tile: (tap, ci); columns 72 .. 95 of tile 2 are padding (computed on tap 8, never stored)
  const int col = ct * 32 + il, colc = col < 72 ? col : 71;
  const int tap = colc >> 3, ci = colc & 7, ky = tap / 3, kx = tap - 3 * ky;
  // k-step s covers output pixels 16 s .. 16 s + 15, this lane 8 of them: WO = 16: row s, columns 8 kl ..; WO = 8: row 2 s + kl
  const unsigned lane_b = (unsigned)((kx == 1 ? 0 : XCOPY) + ci * CIP + ky * ROWB + (WO == 16 ? kl * 16 : kl * 2 * ROWB));
  constexpr unsigned kStepB = WO == 16 ? 2 * ROWB : 4 * ROWB;
  const unsigned lane_a = (unsigned)(SPLIT * 2 * XCOPY + (il & 15) * AP + kl * 16);
  const bool shifted = kx == 0;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  raw_load(0, n0);
  raw_load(1, n0 + 1 < nlast ? n0 + 1 : nlast);
  lds_barrier();  // the zeroes are in place
  // One frame: rs = (n - n0) % 3 and par = (n - n0) & 1 are literals at the call sites.
  auto frame = [&](const int n, const int rs, const int par) __attribute__((always_inline)) {
    const unsigned bufoff = par ? (unsigned)BUFB : 0u;
    raw_load((rs + 2) % 3, n + 2 < nlast ? n + 2 : nlast);  // its set held frame n - 1, staged a frame ago
    raw_wait(rs);
    stage(rs, bufoff);
    lds_barrier();  // images par complete; every wave is done reading images par ^ 1 (frame n - 1)
    if (ct < 3) {
#pragma unroll
      for (int ss = 0; ss < 8; ++ss) {
        const int s = kh * 8 + ss;
        u32x4 qa[SPLIT], qb[SPLIT];
#pragma unroll
        for (int p = 0; p < SPLIT; ++p) {
          qa[p] = *reinterpret_cast<const u32x4*>(lds + bufoff + lane_a + (unsigned)(p * APB) + (unsigned)(s * 32));
          const unsigned bo = bufoff + lane_b + (unsigned)(p * 2 * XCOPY) + (unsigned)s * kStepB;
          const u32x4 f = *reinterpret_cast<const u32x4*>(lds + bo);
          // kx = 0: the odd image one element to the left; the element in front of the fragment is the last one of the
          // row's first half (WO = 16, second half) or the zero left of the row
          unsigned prev = 0u;
          if (WO == 16) prev = kl ? (unsigned)*reinterpret_cast<const unsigned short*>(lds + bo - 2) : 0u;
          const u32x4 sh = wg_shift_in_front(f, prev);
          qb[p] = shifted ? sh : f;
        }
#pragma unroll
        for (int ord = SPLIT - 1; ord >= 0; --ord)
#pragma unroll
          for (int sa = 0; sa <= ord; ++sa)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, qa[sa]), __builtin_bit_cast(bf16x8, qb[ord - sa]), acc, 0, 0, 0);
      }
    }
  };
#pragma unroll 1
  for (int n = n0; n < n1; n += 6) {
    frame(n, 0, 0);
    if (n + 1 < n1) frame(n + 1, 1, 1);
    if (n + 2 < n1) frame(n + 2, 2, 0);
    if (n + 3 < n1) frame(n + 3, 0, 1);
    if (n + 4 < n1) frame(n + 4, 1, 0);
    if (n + 5 < n1) frame(n + 5, 2, 1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped requests of the last frames

  if (part) {
    float* const set = part + (size_t)blockIdx.x * kWgS2SetFloats;
    float4* const ps = reinterpret_cast<float4*>(set) + (size_t)wave * 128 + lane;
    ps[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);   // rows 4 kl + 0 .. 3
    ps[64] = make_float4(acc[4], acc[5], acc[6], acc[7]);  // rows 8 + 4 kl + 0 .. 3
    if (dbias != nullptr) {
#pragma unroll
      for (int j = 0; j < AI; ++j) {  // a wave's 64 lanes share channel wave + 8 j
        const float v = wave_sum(bsum[j]);
        if (lane == 0) set[8 * 2 * 64 * 4 + wave + 8 * j] = v;
      }
    }
  } else {
    if (ct < 3 && col < 72) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int row = wg_tile_row(r, kl);
        atomicAdd(&dwp[((size_t)row * 9 + tap) * g.Cpad + ci], acc[r]);
      }
    }
    if (dbias != nullptr) {
#pragma unroll
      for (int j = 0; j < AI; ++j) {
        const float v = wave_sum(bsum[j]);
        if (lane == 0) atomicAdd(&dbias[wave + 8 * j], v);
      }
    }
  }
}

// Partial sets of conv3x3s2_wgrad_staged_kernel: 72 columns x 16 rows, two k-halves per workgroup (waves ct and ct + 4).
// float4 f = (ct * 2 + half) * 64 + lane of the three column tiles: 384 (48 blocks), then 4 bias float4.
struct WgRedS2 {
  static constexpr int NL = 8, NG = 32, U = 2, KS = 2, SET4 = kWgS2SetFloats / 4;
  static __device__ __forceinline__ WgRedCol column(const int f, const int by) {
    return {(size_t)(f >= 384 ? 8 * 128 + (f - 384) : f), 4 * 128, f >= 384 ? 4 * (f - 384) : -1, f >= 388};
  }
  static __device__ __forceinline__ void scatter(const int f, const int by, const float4 v, const int cpad, float* __restrict__ dwp) {
    const int ct = f >> 7, rem = f & 127, half = rem >> 6, lane = rem & 63, il = lane & 31, kl = lane >> 5;
    const int col = ct * 32 + il;
    if (col < 72) wg_red_add_rows(dwp + ((size_t)(8 * half + 4 * kl) * 9 + (col >> 3)) * cpad + (col & 7), (size_t)9 * cpad, v);
  }
};

// ------------------------------------------------------------------------------------------------
// Weight gradient of the decoders' second ConvTranspose2d (k = 4, stride 2, pad 1, 32 -> 16 channels; input planes of 256
// pixels: 16x16 vision, 32x8 audio), the same recipe with the roles the transposed layer gives the operands:
//   dW[ci][ky][kx][co] = sum over frames n and INPUT pixels (y, x) of  act(a)[n][ci][y][x] * src[n][co][2 y - 1 + ky][2 x - 1 + kx]
// `a` is the layer input (32 channels, activated here), src the output gradient (16 channels, 2H x 2W, raw).  src is
// de-interleaved by column parity with a zero halo row above AND below every plane: kx = 0 reads the odd image at x - 1
// (funnel shift with the element in front), kx = 1 the even image at x, kx = 2 the odd image at x, kx = 3 the even image
// at x + 1 (funnel shift the other way with the element behind).  MFMA columns are (tap, co) pairs: 16 x 16 = 256 = one
// 32-column tile per wave; rows are the 32 ci.  One image buffer (102 KB: two barriers per frame), raw frames (96 KB per
// frame and workgroup) requested two frames ahead.  Partial set: float4 number (w * 4 + r / 4) * 64 + lane, + 16 bias sums.
// The layer's bias gradient is the per-channel sum of src, which this kernel streams anyway: with dsrcbias != NULL every
// thread adds up its src items while staging (item j of a thread is channel tid / 256 + 2 j: four waves per channel, met
// in LDS) and the workgroup's 16 sums travel with its partial set -- a separate channel-sum launch re-read the tensor.
// ------------------------------------------------------------------------------------------------
constexpr int kWgT4TileFloats = 8 * 4 * 64 * 4;
constexpr int kWgT4SetFloats = kWgT4TileFloats + 16;
template <int WO>
__host__ __device__ constexpr int wgt4_cip() { return (((256 / WO * 2 + 2) * (2 * WO)) / 16 | 1) * 16; }
template <int SPLIT, int WO>
__host__ __device__ constexpr int wgt4_lds_bytes() { return SPLIT * (2 * 16 * wgt4_cip<WO>() + 32 * 528); }

template <int SPLIT, int WO>
__global__ __launch_bounds__(512, 1) void convt4s2_wgrad_staged_kernel(
    const MtrssmConvGeom g, const float* __restrict__ a, const float* __restrict__ src, const int pre_act_a, float* __restrict__ dwp,
    float* __restrict__ part, float* __restrict__ dsrcbias, const int frames_per_wg) {
  static_assert(SPLIT == 1 || SPLIT == 2, "one or two bf16 pieces");
  static_assert(WO == 16 || WO == 8, "input plane 16x16 or 32x8");
  constexpr int NT = 512, C = 16, CO = 32, HO = 256 / WO, HS = 2 * HO, WS = 2 * WO;
  constexpr int ROWB = WS;                 // bytes per row of one parity image: WS / 2 bf16
  constexpr int CIP = wgt4_cip<WO>();      // bytes per channel: (HS + 2) rows, padded
  constexpr int XCOPY = C * CIP;           // one parity image of one piece
  constexpr int AP = 528, APB = CO * AP;   // `a` image: [ci][256 pixels + 8] bf16
  constexpr int XI = C * HS * WS / 4 / NT, AI = CO * 256 / 4 / NT, NI = XI + AI;  // 8 + 4 float4 items per thread and frame
  extern __shared__ __attribute__((aligned(16))) unsigned char wgt4_lds[];
  unsigned char* const lds = wgt4_lds;     // [piece][even image][odd image] then [piece][a image]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int il = lane & 31, kl = lane >> 5;
  const int n0 = blockIdx.x * frames_per_wg;
  const int n1 = n0 + frames_per_wg < g.N ? n0 + frames_per_wg : g.N;
  if (n0 >= n1) return;  // whole workgroup
  const int nlast = n1 - 1;

  const bool act_elu = g.act == MTRSSM_ACT_ELU, act_relu = g.act == MTRSSM_ACT_RELU, pre = pre_act_a != 0;
  const WgActSel act_sel{act_elu, act_relu, pre};

  // zero the buffer once: the halo rows are never written again
  for (int o = tid * 16; o < wgt4_lds_bytes<SPLIT, WO>(); o += NT * 16) *reinterpret_cast<uint4*>(lds + o) = make_uint4(0u, 0u, 0u, 0u);

  const float4* const xsrc = reinterpret_cast<const float4*>(src) + tid;
  const float4* const asrc = reinterpret_cast<const float4*>(a) + tid;
  constexpr size_t xfr = (size_t)C * HS * WS / 4, afr = (size_t)CO * 256 / 4;  // float4 per frame
  static_assert(HS * WS / 4 == 256 && XI == 8, "src item j of a thread is channel tid / 256 + 2 j");
  float bsum[XI];
#pragma unroll
  for (int j = 0; j < XI; ++j) bsum[j] = 0.f;
  wg_f32x4 raw[3][NI];  // [set][a items, src items]
  auto raw_load = [&](const int rs, const int n) __attribute__((always_inline)) { wg_raw_load<NT, AI, XI>(raw[rs], asrc, afr, xsrc, xfr, n); };
  auto raw_wait = [&](const int rs) __attribute__((always_inline)) { wg_raw_wait<2 * NI>(raw[rs]); };  // the two younger sets may still be in flight
  auto stage = [&](const int rs) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      const wg_f32x4 v = raw[rs][it];
      if (it < AI) {
        unsigned d0[SPLIT], d1[SPLIT];
        wg_split_pair<SPLIT>(act_sel(v.x), act_sel(v.y), d0);
        wg_split_pair<SPLIT>(act_sel(v.z), act_sel(v.w), d1);
        const int f = tid + NT * it;  // ci = f / 64, pixel = 4 (f % 64)
        const unsigned o = (unsigned)(SPLIT * 2 * XCOPY) + (unsigned)((f >> 6) * AP + (f & 63) * 8);
#pragma unroll
        for (int p = 0; p < SPLIT; ++p) *reinterpret_cast<uint2*>(lds + o + p * APB) = make_uint2(d0[p], d1[p]);
      } else {
        unsigned de[SPLIT], dd[SPLIT];  // even columns (c0, c0 + 2), odd columns (c0 + 1, c0 + 3)
        bsum[it - AI] += (v.x + v.y) + (v.z + v.w);
        wg_split_pair<SPLIT>(v.x, v.z, de);
        wg_split_pair<SPLIT>(v.y, v.w, dd);
        const int f = tid + NT * (it - AI);
        const int co = f / (HS * WS / 4), rem = f - co * (HS * WS / 4), row = rem / (WS / 4), c4 = rem - row * (WS / 4);
        const unsigned o = (unsigned)(co * CIP + (row + 1) * ROWB + c4 * 4);
#pragma unroll
        for (int p = 0; p < SPLIT; ++p) {
          *reinterpret_cast<unsigned*>(lds + o + p * 2 * XCOPY) = de[p];
          *reinterpret_cast<unsigned*>(lds + o + p * 2 * XCOPY + XCOPY) = dd[p];
        }
      }
    }
  };

  // the lane's column: (tap, co) = (col >> 4, col & 15)
  const int col = wave * 32 + il;
  const int tap = col >> 4, co = col & 15, ky = tap >> 2, kx = tap & 3;
  const bool odd = kx == 0 || kx == 2;
  // k-step s covers input pixels 16 s .. 16 s + 15, this lane 8 of them: WO = 16: row s, columns 8 kl ..; WO = 8: row 2 s + kl
  const unsigned lane_b = (unsigned)((odd ? XCOPY : 0) + co * CIP + ky * ROWB + (WO == 16 ? kl * 16 : kl * 2 * ROWB));
  constexpr unsigned kStepB = WO == 16 ? 2 * ROWB : 4 * ROWB;
  const unsigned lane_a = (unsigned)(SPLIT * 2 * XCOPY + il * AP + kl * 16);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  raw_load(0, n0);
  raw_load(1, n0 + 1 < nlast ? n0 + 1 : nlast);
  auto frame = [&](const int n, const int rs) __attribute__((always_inline)) {  // rs = (n - n0) % 3, a literal at the call sites
    raw_load((rs + 2) % 3, n + 2 < nlast ? n + 2 : nlast);  // its set held frame n - 1, staged a frame ago
    raw_wait(rs);
    lds_barrier();  // every wave is done reading the previous frame's images (first frame: the zeroes are in place)
    stage(rs);
    lds_barrier();  // images complete
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      u32x4 qa[SPLIT], qb[SPLIT];
#pragma unroll
      for (int p = 0; p < SPLIT; ++p) {
        qa[p] = *reinterpret_cast<const u32x4*>(lds + lane_a + (unsigned)(p * APB) + (unsigned)(s * 32));
        const unsigned bo = lane_b + (unsigned)(p * 2 * XCOPY) + (unsigned)s * kStepB;
        const u32x4 f = *reinterpret_cast<const u32x4*>(lds + bo);
        // the element in front of / behind the fragment: the neighbouring half of the row (WO = 16) or the zero beyond it
        unsigned prev = 0u, next = 0u;
        if (WO == 16) {
          prev = kl ? (unsigned)*reinterpret_cast<const unsigned short*>(lds + bo - 2) : 0u;
          next = kl ? 0u : (unsigned)*reinterpret_cast<const unsigned short*>(lds + bo + 16);
        }
        const u32x4 shr = u32x4{(f.x << 16) | prev, __builtin_amdgcn_alignbit(f.y, f.x, 16), __builtin_amdgcn_alignbit(f.z, f.y, 16), __builtin_amdgcn_alignbit(f.w, f.z, 16)};
        const u32x4 shl = u32x4{__builtin_amdgcn_alignbit(f.y, f.x, 16), __builtin_amdgcn_alignbit(f.z, f.y, 16), __builtin_amdgcn_alignbit(f.w, f.z, 16), (f.w >> 16) | (next << 16)};
        qb[p] = kx == 0 ? shr : (kx == 3 ? shl : f);
      }
      wg_mfma_pieces<SPLIT>(acc, qa, qb);
    }
  };
#pragma unroll 1
  for (int n = n0; n < n1; n += 3) {
    frame(n, 0);
    if (n + 1 < n1) frame(n + 1, 1);
    if (n + 2 < n1) frame(n + 2, 2);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped requests of the last frames

  float* const bred = reinterpret_cast<float*>(lds);  // [item][wave]
  if (dsrcbias != nullptr) {
    lds_barrier();  // the images are dead
#pragma unroll
    for (int j = 0; j < XI; ++j) {
      const float v = wave_sum(bsum[j]);
      if (lane == 0) bred[j * 8 + wave] = v;
    }
    lds_barrier();
  }
  if (part) {
    float4* const ps = reinterpret_cast<float4*>(part) + (size_t)blockIdx.x * (kWgT4SetFloats / 4) + (size_t)wave * 256 + lane;
    wg_store_tile(ps, acc);
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wg_tile_row(r, kl);
      atomicAdd(&dwp[((size_t)row * 16 + tap) * g.Cpad + co], acc[r]);
    }
  }
  if (dsrcbias != nullptr && tid < 16) {
    const int j = tid >> 1, w0 = 4 * (tid & 1);  // channel tid = w0 / 4 + 2 j
    const float v = (bred[j * 8 + w0] + bred[j * 8 + w0 + 1]) + (bred[j * 8 + w0 + 2] + bred[j * 8 + w0 + 3]);
    if (part) part[(size_t)blockIdx.x * kWgT4SetFloats + kWgT4TileFloats + tid] = v;
    else atomicAdd(&dsrcbias[tid], v);
  }
}

// Partial sets of convt4s2_wgrad_staged_kernel into dwp / dbias (the sums of src): float4 f = (wave * 4 + gq) * 64 + lane,
// then 4 bias float4 (host: grid.x * 8 == TILE4, + 8).
struct WgRedT4 {
  static constexpr int NL = 8, NG = 32, U = 4, KS = 1, SET4 = kWgT4SetFloats / 4, TILE4 = kWgT4TileFloats / 4;
  static __device__ __forceinline__ WgRedCol column(const int f, const int by) {
    return {(size_t)f, 0, f >= TILE4 ? 4 * (f - TILE4) : -1, f >= SET4};
  }
  static __device__ __forceinline__ void scatter(const int f, const int by, const float4 v, const int cpad, float* __restrict__ dwp) {
    const int lane = f & 63, gq = (f >> 6) & 3, wave = f >> 8, il = lane & 31, kl = lane >> 5;
    const int col = wave * 32 + il, tap = col >> 4, co = col & 15, row = 8 * gq + 4 * kl;
    wg_red_add_rows(dwp + ((size_t)row * 16 + tap) * cpad + co, (size_t)16 * cpad, v);
  }
};

// ------------------------------------------------------------------------------------------------
// ... and of the decoders' FIRST ConvTranspose2d (k = 4, stride 2, pad 1, 64 -> 32 channels; input planes of 64 pixels: 8x8
// vision, 16x4 audio).  32 src channels per tap make every 32-column tile ONE tap with lane = src channel, so the column
// shift is wave-uniform: wave w holds taps 2 w (odd image: kx = 0 shifted by one with a zero in front, kx = 2 as it stands)
// and 2 w + 1 (even image: kx = 1 as it stands, kx = 3 shifted the other way) for both 32-row tiles of the 64 ci = four
// accumulator tiles.  A lane's 8 pixels are one whole row (8x8) or two whole rows (16x4: two 8-byte reads two image rows
// apart), so no neighbour element is needed.  Partial set: float4 number ((w * 4 + tile) * 4 + r / 4) * 64 + lane,
// tile = 2 (row tile) + (tap & 1), + 32 bias sums (dsrcbias != NULL: the per-channel sums of src, added up while staging; src
// item j of a thread is channel wave + 8 j, so a wave sum is a workgroup sum).
// ------------------------------------------------------------------------------------------------
constexpr int kWgT4bTileFloats = 8 * 4 * 4 * 64 * 4;
constexpr int kWgT4bSetFloats = kWgT4bTileFloats + 32;
template <int WO>
__host__ __device__ constexpr int wgt4b_cip() { return (((64 / WO * 2 + 2) * (2 * WO)) / 16 | 1) * 16; }
template <int SPLIT, int WO>
__host__ __device__ constexpr int wgt4b_lds_bytes() { return SPLIT * (2 * 32 * wgt4b_cip<WO>() + 64 * kWgresAPitch); }

template <int SPLIT, int WO>
__global__ __launch_bounds__(512, 1) void convt4s2b_wgrad_staged_kernel(
    const MtrssmConvGeom g, const float* __restrict__ a, const float* __restrict__ src, const int pre_act_a, float* __restrict__ dwp,
    float* __restrict__ part, float* __restrict__ dsrcbias, const int frames_per_wg) {
  static_assert(SPLIT == 1 || SPLIT == 2, "one or two bf16 pieces");
  static_assert(WO == 8 || WO == 4, "input plane 8x8 or 16x4");
  constexpr int NT = 512, C = 32, CO = 64, HO = 64 / WO, HS = 2 * HO, WS = 2 * WO;
  constexpr int ROWB = WS;                 // bytes per row of one parity image: WS / 2 bf16
  constexpr int CIP = wgt4b_cip<WO>();     // bytes per channel: (HS + 2) rows, padded
  constexpr int XCOPY = C * CIP;           // one parity image of one piece
  constexpr int AP = kWgresAPitch, APB = CO * AP;  // `a` image: [ci][64 pixels + 8] bf16
  constexpr int XI = C * HS * WS / 4 / NT, AI = CO * 64 / 4 / NT, NI = XI + AI;  // 4 + 2 float4 items per thread and frame
  extern __shared__ __attribute__((aligned(16))) unsigned char wgt4b_lds[];
  unsigned char* const lds = wgt4b_lds;    // [piece][even image][odd image] then [piece][a image]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int il = lane & 31, kl = lane >> 5;
  const int n0 = blockIdx.x * frames_per_wg;
  const int n1 = n0 + frames_per_wg < g.N ? n0 + frames_per_wg : g.N;
  if (n0 >= n1) return;  // whole workgroup
  const int nlast = n1 - 1;

  const bool act_elu = g.act == MTRSSM_ACT_ELU, act_relu = g.act == MTRSSM_ACT_RELU, pre = pre_act_a != 0;
  const WgActSel act_sel{act_elu, act_relu, pre};

  for (int o = tid * 16; o < wgt4b_lds_bytes<SPLIT, WO>(); o += NT * 16) *reinterpret_cast<uint4*>(lds + o) = make_uint4(0u, 0u, 0u, 0u);

  const float4* const xsrc = reinterpret_cast<const float4*>(src) + tid;
  const float4* const asrc = reinterpret_cast<const float4*>(a) + tid;
  constexpr size_t xfr = (size_t)C * HS * WS / 4, afr = (size_t)CO * 64 / 4;  // float4 per frame
  static_assert(HS * WS / 4 == 64 && XI == 4, "src item j of a thread is channel wave + 8 j");
  float bsum[XI];
#pragma unroll
  for (int j = 0; j < XI; ++j) bsum[j] = 0.f;
  wg_f32x4 raw[3][NI];  // [set][a items, src items]
  auto raw_load = [&](const int rs, const int n) __attribute__((always_inline)) { wg_raw_load<NT, AI, XI>(raw[rs], asrc, afr, xsrc, xfr, n); };
  auto raw_wait = [&](const int rs) __attribute__((always_inline)) { wg_raw_wait<2 * NI>(raw[rs]); };  // the two younger sets may still be in flight
  auto stage = [&](const int rs) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      const wg_f32x4 v = raw[rs][it];
      if (it < AI) {
        unsigned d0[SPLIT], d1[SPLIT];
        wg_split_pair<SPLIT>(act_sel(v.x), act_sel(v.y), d0);
        wg_split_pair<SPLIT>(act_sel(v.z), act_sel(v.w), d1);
        const int f = tid + NT * it;  // ci = f / 16, pixel = 4 (f % 16)
        const unsigned o = (unsigned)(SPLIT * 2 * XCOPY) + (unsigned)((f >> 4) * AP + (f & 15) * 8);
#pragma unroll
        for (int p = 0; p < SPLIT; ++p) *reinterpret_cast<uint2*>(lds + o + p * APB) = make_uint2(d0[p], d1[p]);
      } else {
        unsigned de[SPLIT], dd[SPLIT];  // even columns (c0, c0 + 2), odd columns (c0 + 1, c0 + 3)
        bsum[it - AI] += (v.x + v.y) + (v.z + v.w);
        wg_split_pair<SPLIT>(v.x, v.z, de);
        wg_split_pair<SPLIT>(v.y, v.w, dd);
        const int f = tid + NT * (it - AI);
        const int co = f / (HS * WS / 4), rem = f - co * (HS * WS / 4), row = rem / (WS / 4), c4 = rem - row * (WS / 4);
        const unsigned o = (unsigned)(co * CIP + (row + 1) * ROWB + c4 * 4);
#pragma unroll
        for (int p = 0; p < SPLIT; ++p) {
          *reinterpret_cast<unsigned*>(lds + o + p * 2 * XCOPY) = de[p];
          *reinterpret_cast<unsigned*>(lds + o + p * 2 * XCOPY + XCOPY) = dd[p];
        }
      }
    }
  };

  // taps 2 w (odd image) and 2 w + 1 (even image): ky = w >> 1 for both, kx = 2 (w & 1) and 2 (w & 1) + 1; lane = src channel
  const int ky = wave >> 1;
  const bool hi = (wave & 1) != 0;  // kx in {2, 3}: the odd-image tap as it stands, the even-image tap shifted towards x + 1
  // k-step s covers input pixels 16 s .. 16 s + 15, this lane 8 of them: WO = 8: row 2 s + kl; WO = 4: rows 4 s + 2 kl, + 1
  const unsigned lane_b = (unsigned)(il * CIP + ky * ROWB + kl * (WO == 8 ? 2 * ROWB : 4 * ROWB));
  constexpr unsigned kStepB = WO == 8 ? 4 * ROWB : 8 * ROWB;
  const unsigned lane_a = (unsigned)(SPLIT * 2 * XCOPY + il * AP + kl * 16);
  f32x16 acc[4];  // [row tile * 2 + (tap & 1)]
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  constexpr int FR = WO == 8 ? 1 : 2;  // image rows per fragment
  auto shr1 = [](const u32x4 f) __attribute__((always_inline)) { return wg_rows_shift_in_front<FR>(f); };  // element x <- x - 1
  auto shl1 = [](const u32x4 f) __attribute__((always_inline)) { return wg_rows_shift_behind<FR>(f); };    // element x <- x + 1
  auto read_frag = [&](const unsigned off) __attribute__((always_inline)) {
    if (WO == 8) return *reinterpret_cast<const u32x4*>(lds + off);
    const uint2 r0 = *reinterpret_cast<const uint2*>(lds + off), r1 = *reinterpret_cast<const uint2*>(lds + off + 2 * ROWB);
    return u32x4{r0.x, r0.y, r1.x, r1.y};
  };

  raw_load(0, n0);
  raw_load(1, n0 + 1 < nlast ? n0 + 1 : nlast);
  auto frame = [&](const int n, const int rs) __attribute__((always_inline)) {  // rs = (n - n0) % 3, a literal at the call sites
    raw_load((rs + 2) % 3, n + 2 < nlast ? n + 2 : nlast);  // its set held frame n - 1, staged a frame ago
    raw_wait(rs);
    lds_barrier();  // every wave is done reading the previous frame's images (first frame: the zeroes are in place)
    stage(rs);
    lds_barrier();  // images complete
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      u32x4 qa[2][SPLIT], qb[2][SPLIT];
#pragma unroll
      for (int p = 0; p < SPLIT; ++p) {
        qa[0][p] = *reinterpret_cast<const u32x4*>(lds + lane_a + (unsigned)(p * APB) + (unsigned)(s * 32));
        qa[1][p] = *reinterpret_cast<const u32x4*>(lds + lane_a + (unsigned)(32 * AP + p * APB) + (unsigned)(s * 32));
        const unsigned bo = lane_b + (unsigned)(p * 2 * XCOPY) + (unsigned)s * kStepB;
        const u32x4 fe = read_frag(bo), fo = read_frag(bo + XCOPY);
        const u32x4 fos = shr1(fo), fes = shl1(fe);
        qb[0][p] = hi ? fo : fos;   // tap 2 w: kx = 2 : kx = 0
        qb[1][p] = hi ? fes : fe;   // tap 2 w + 1: kx = 3 : kx = 1
      }
#pragma unroll
      for (int ord = SPLIT - 1; ord >= 0; --ord)
#pragma unroll
        for (int sa = 0; sa <= ord; ++sa)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, qa[t >> 1][sa]), __builtin_bit_cast(bf16x8, qb[t & 1][ord - sa]), acc[t], 0, 0, 0);
    }
  };
#pragma unroll 1
  for (int n = n0; n < n1; n += 3) {
    frame(n, 0);
    if (n + 1 < n1) frame(n + 1, 1);
    if (n + 2 < n1) frame(n + 2, 2);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped requests of the last frames

  if (part) {
    float4* const ps = reinterpret_cast<float4*>(part) + (size_t)blockIdx.x * (kWgT4bSetFloats / 4) + (size_t)wave * 1024 + lane;
#pragma unroll
    for (int t = 0; t < 4; ++t) wg_store_tile(ps + t * 256, acc[t]);
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wg_tile_row(r, kl, (t >> 1) * 32);
        atomicAdd(&dwp[((size_t)row * 16 + 2 * wave + (t & 1)) * g.Cpad + il], acc[t][r]);
      }
  }
  if (dsrcbias != nullptr) {
#pragma unroll
    for (int j = 0; j < XI; ++j) {
      const float v = wave_sum(bsum[j]);
      if (lane == 0) {
        if (part) part[(size_t)blockIdx.x * kWgT4bSetFloats + kWgT4bTileFloats + wave + 8 * j] = v;
        else atomicAdd(&dsrcbias[wave + 8 * j], v);
      }
    }
  }
}

// Partial sets of convt4s2b_wgrad_staged_kernel into dwp / dbias (the sums of src): float4 f = ((wave * 4 + t) * 4 + gq) * 64
// + lane, then the bias block's 8 float4, all in use (host: grid.x * 8 == TILE4, + 8).
struct WgRedT4b {
  static constexpr int NL = 8, NG = 32, U = 4, KS = 1, SET4 = kWgT4bSetFloats / 4, TILE4 = kWgT4bTileFloats / 4;
  static __device__ __forceinline__ WgRedCol column(const int f, const int by) {
    return {(size_t)f, 0, f >= TILE4 ? 4 * (f - TILE4) : -1, false};
  }
  static __device__ __forceinline__ void scatter(const int f, const int by, const float4 v, const int cpad, float* __restrict__ dwp) {
    const int lane = f & 63, gq = (f >> 6) & 3, t = (f >> 8) & 3, wave = f >> 10, il = lane & 31, kl = lane >> 5;
    const int tap = 2 * wave + (t & 1), row = (t >> 1) * 32 + 8 * gq + 4 * kl;
    wg_red_add_rows(dwp + ((size_t)row * 16 + tap) * cpad + il, (size_t)16 * cpad, v);
  }
};

// ------------------------------------------------------------------------------------------------
// Weight gradient of the FIRST encoder layer (3x3 / stride 2 / pad 1; one frame channel + two frame-independent
// coordinate channels -> 8; 1024-pixel output planes: 32x32 vision, 64x16 audio), the recipe of
// conv3x3s2_wgrad_staged_kernel on a thin layer:
//   dW[co][ky][kx][c] = sum over frames n and output pixels of  a[n][co][oy][ox] * act(src ++ coords)[n][c][2 oy + ky - 1][2 ox + kx - 1]
// 27 (tap, channel) columns = one MFMA tile with 8 of its 32 rows used; all eight waves hold that tile for eight of the
// frame's 64 k-steps each (the reduce kernel adds the eight).  The coordinate channels are staged once per workgroup.
// Partial set: float4 number w * 64 + lane (rows 4 kl .. + 3 of column il), + 8 bias sums.
// ------------------------------------------------------------------------------------------------
constexpr int kWgThinSetFloats = 8 * 64 * 4 + 8;
template <int WO>
__host__ __device__ constexpr int wgthin_cip() { return (((1024 / WO * 2 + 1) * (2 * WO)) / 16 | 1) * 16; }
template <int SPLIT, int WO>
__host__ __device__ constexpr int wgthin_lds_bytes() { return SPLIT * (2 * 3 * wgthin_cip<WO>() + 8 * 2064) + 128; }

template <int SPLIT, int WO>
__global__ __launch_bounds__(512, 1) void conv3x3s2_thin_wgrad_staged_kernel(
    const MtrssmConvGeom g, const float* __restrict__ a, const float* __restrict__ src, const float* __restrict__ coords,
    float* __restrict__ dwp, float* __restrict__ part, float* __restrict__ dbias, const int frames_per_wg) {
  static_assert(SPLIT == 1 || SPLIT == 2, "one or two bf16 pieces");
  static_assert(WO == 32 || WO == 16, "output plane 32x32 or 64x16");
  constexpr int NT = 512, CH = 3, CO = 8, HO = 1024 / WO, HS = 2 * HO, WS = 2 * WO;
  constexpr int ROWB = WS;                 // bytes per row of one parity image: WS / 2 bf16
  constexpr int CIP = wgthin_cip<WO>();    // bytes per channel: (HS + 1) rows, padded
  constexpr int XCOPY = CH * CIP;          // one parity image of one piece: [frame channel, coordinate y, coordinate x]
  constexpr int AP = 2064, APB = CO * AP;  // `a` image: [co][1024 pixels + 8] bf16
  constexpr int XI = HS * WS / 4 / NT, AI = CO * 1024 / 4 / NT, NI = XI + AI;  // 2 + 4 float4 items per thread and frame
  constexpr int LDSB = SPLIT * (2 * XCOPY + APB);
  extern __shared__ __attribute__((aligned(16))) unsigned char wgthin_lds[];
  unsigned char* const lds = wgthin_lds;   // [piece][even image][odd image], [piece][a image], 32 floats of bias scratch
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int il = lane & 31, kl = lane >> 5;
  const int n0 = blockIdx.x * frames_per_wg;
  const int n1 = n0 + frames_per_wg < g.N ? n0 + frames_per_wg : g.N;
  if (n0 >= n1) return;  // whole workgroup
  const int nlast = n1 - 1;

  const bool act_elu = g.act == MTRSSM_ACT_ELU, act_relu = g.act == MTRSSM_ACT_RELU, pre = g.pre_act != 0;
  const WgActSel act_sel{act_elu, act_relu, pre};

  for (int o = tid * 16; o < wgthin_lds_bytes<SPLIT, WO>(); o += NT * 16) *reinterpret_cast<uint4*>(lds + o) = make_uint4(0u, 0u, 0u, 0u);

  // a src / coordinate float4 = 4 consecutive columns c0 .. c0 + 3 of one row: even columns to the even image, odd to the odd one
  auto stage_src = [&](const float4 v, const int ch, const int f) __attribute__((always_inline)) {
    unsigned de[SPLIT], dd[SPLIT];
    wg_split_pair<SPLIT>(act_sel(v.x), act_sel(v.z), de);
    wg_split_pair<SPLIT>(act_sel(v.y), act_sel(v.w), dd);
    const int row = f / (WS / 4), c4 = f - row * (WS / 4);
    const unsigned o = (unsigned)(ch * CIP + (row + 1) * ROWB + c4 * 4);
#pragma unroll
    for (int p = 0; p < SPLIT; ++p) {
      *reinterpret_cast<unsigned*>(lds + o + p * 2 * XCOPY) = de[p];
      *reinterpret_cast<unsigned*>(lds + o + p * 2 * XCOPY + XCOPY) = dd[p];
    }
  };

  const float4* const xsrc = reinterpret_cast<const float4*>(src) + tid;
  const float4* const asrc = reinterpret_cast<const float4*>(a) + tid;
  constexpr size_t xfr = (size_t)HS * WS / 4, afr = (size_t)CO * 1024 / 4;  // float4 per frame
  float bsum[AI];
#pragma unroll
  for (int j = 0; j < AI; ++j) bsum[j] = 0.f;
  wg_f32x4 raw[3][NI];  // [set][a items, src items]
  auto raw_load = [&](const int rs, const int n) __attribute__((always_inline)) { wg_raw_load<NT, AI, XI>(raw[rs], asrc, afr, xsrc, xfr, n); };
  auto raw_wait = [&](const int rs) __attribute__((always_inline)) { wg_raw_wait<2 * NI>(raw[rs]); };  // the two younger sets may still be in flight
  auto stage = [&](const int rs) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      const wg_f32x4 v = raw[rs][it];
      if (it < AI) {
        bsum[it] += (v.x + v.y) + (v.z + v.w);
        unsigned d0[SPLIT], d1[SPLIT];
        wg_split_pair<SPLIT>(v.x, v.y, d0);
        wg_split_pair<SPLIT>(v.z, v.w, d1);
        const int f = tid + NT * it;  // co = f / 256, pixel = 4 (f % 256)
        const unsigned o = (unsigned)(SPLIT * 2 * XCOPY) + (unsigned)((f >> 8) * AP + (f & 255) * 8);
#pragma unroll
        for (int p = 0; p < SPLIT; ++p) *reinterpret_cast<uint2*>(lds + o + p * APB) = make_uint2(d0[p], d1[p]);
      } else {
        stage_src(make_float4(v.x, v.y, v.z, v.w), 0, tid + NT * (it - AI));
      }
    }
  };

  // the lane's column: (tap, channel) = (il / 3, il % 3); lanes 27 .. 31 are padding (computed on column 26, never stored)
  const int colc = il < 27 ? il : 26;
  const int tap = colc / 3, ch = colc - 3 * tap, ky = tap / 3, kx = tap - 3 * ky;
  const unsigned lane_b = (unsigned)((kx == 1 ? 0 : XCOPY) + ch * CIP + ky * ROWB + kl * 16);
  const unsigned lane_a = (unsigned)(SPLIT * 2 * XCOPY + (il & 7) * AP + kl * 16);
  const bool shifted = kx == 0;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  raw_load(0, n0);
  raw_load(1, n0 + 1 < nlast ? n0 + 1 : nlast);
  lds_barrier();  // the zeroes are in place
  // the coordinate channels, once: 2 x HS x WS floats = 4 float4 per thread
#pragma unroll
  for (int j = 0; j < 2 * XI; ++j) {
    const int f = tid + NT * j;  // channel f / (HS WS / 4)
    stage_src(reinterpret_cast<const float4*>(coords)[f], 1 + f / (HS * WS / 4), f % (HS * WS / 4));
  }
  auto frame = [&](const int n, const int rs) __attribute__((always_inline)) {  // rs = (n - n0) % 3, a literal at the call sites
    raw_load((rs + 2) % 3, n + 2 < nlast ? n + 2 : nlast);  // its set held frame n - 1, staged a frame ago
    raw_wait(rs);
    lds_barrier();  // every wave is done reading the previous frame's images
    stage(rs);
    lds_barrier();  // images complete
#pragma unroll
    for (int ss = 0; ss < 8; ++ss) {
      const int s = wave * 8 + ss;  // k-step: output pixels 16 s .. 16 s + 15; WO = 32: row s / 2, half s & 1; WO = 16: row s
      const unsigned soff = WO == 32 ? (unsigned)((s >> 1) * 2 * ROWB + (s & 1) * 32) : (unsigned)(s * 2 * ROWB);
      const bool has_prev = WO == 32 ? ((s & 1) | kl) != 0 : kl != 0;
      u32x4 qa[SPLIT], qb[SPLIT];
#pragma unroll
      for (int p = 0; p < SPLIT; ++p) {
        qa[p] = *reinterpret_cast<const u32x4*>(lds + lane_a + (unsigned)(p * APB) + (unsigned)(s * 32));
        const unsigned bo = lane_b + (unsigned)(p * 2 * XCOPY) + soff;
        const u32x4 f = *reinterpret_cast<const u32x4*>(lds + bo);
        const unsigned prev = has_prev ? (unsigned)*reinterpret_cast<const unsigned short*>(lds + bo - 2) : 0u;
        const u32x4 sh = wg_shift_in_front(f, prev);
        qb[p] = shifted ? sh : f;
      }
#pragma unroll
      for (int ord = SPLIT - 1; ord >= 0; --ord)
#pragma unroll
        for (int sa = 0; sa <= ord; ++sa)
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, qa[sa]), __builtin_bit_cast(bf16x8, qb[ord - sa]), acc, 0, 0, 0);
    }
  };
#pragma unroll 1
  for (int n = n0; n < n1; n += 3) {
    frame(n, 0);
    if (n + 1 < n1) frame(n + 1, 1);
    if (n + 2 < n1) frame(n + 2, 2);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped requests of the last frames

  // bias sums: `a` item j of this thread belongs to channel tid / 256 + 2 j: four waves per channel, met in LDS
  float* const bred = reinterpret_cast<float*>(lds + LDSB);  // [item][wave]
  if (dbias != nullptr) {
    lds_barrier();  // the images are dead
#pragma unroll
    for (int j = 0; j < AI; ++j) {
      const float v = wave_sum(bsum[j]);
      if (lane == 0) bred[j * 8 + wave] = v;
    }
    lds_barrier();
  }
  if (part) {
    float* const set = part + (size_t)blockIdx.x * kWgThinSetFloats;
    reinterpret_cast<float4*>(set)[wave * 64 + lane] = make_float4(acc[0], acc[1], acc[2], acc[3]);  // rows 4 kl + 0 .. 3
    if (dbias != nullptr && tid < 8) {
      const int j = tid >> 1, w0 = 4 * (tid & 1);  // channel tid = w0 / 4 + 2 j
      set[8 * 64 * 4 + tid] = (bred[j * 8 + w0] + bred[j * 8 + w0 + 1]) + (bred[j * 8 + w0 + 2] + bred[j * 8 + w0 + 3]);
    }
  } else {
    if (il < 27) {
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(&dwp[((size_t)(4 * kl + r) * 9 + tap) * g.Cpad + ch], acc[r]);
    }
    if (dbias != nullptr && tid < 8) {
      const int j = tid >> 1, w0 = 4 * (tid & 1);
      atomicAdd(&dbias[tid], (bred[j * 8 + w0] + bred[j * 8 + w0 + 1]) + (bred[j * 8 + w0 + 2] + bred[j * 8 + w0 + 3]));
    }
  }
}

// Partial sets of conv3x3s2_thin_wgrad_staged_kernel: one tile, eight k-parts (waves) per workgroup.  float4 f = the lane's
// (64 of them: 8 blocks), then the bias block (2 float4 in use).
struct WgRedThin {
  static constexpr int NL = 8, NG = 32, U = 2, KS = 8, SET4 = kWgThinSetFloats / 4;
  static __device__ __forceinline__ WgRedCol column(const int f, const int by) {
    return {(size_t)(f >= 64 ? 8 * 64 + (f - 64) : f), 64, f >= 64 ? 4 * (f - 64) : -1, f >= 66};
  }
  static __device__ __forceinline__ void scatter(const int f, const int by, const float4 v, const int cpad, float* __restrict__ dwp) {
    const int il = f & 31, kl = f >> 5, tap = il / 3, ch = il - 3 * tap;
    if (il < 27) wg_red_add_rows(dwp + ((size_t)(4 * kl) * 9 + tap) * cpad + ch, (size_t)9 * cpad, v);
  }
};

// ------------------------------------------------------------------------------------------------
// Weight gradient of the decoders' LAST ConvTranspose2d (k = 4, stride 2, pad 1, 16 -> 1 channel; input planes of 1024
// pixels: 32x32 vision, 64x16 audio): convt4s2_wgrad_staged_kernel on a thin layer.  `a` is the layer input (16 channels,
// activated here), src the one-channel output gradient; 16 (tap) columns and 16 rows = a quarter of one MFMA tile, held by
// all eight waves for eight of the frame's 64 k-steps each.  Partial set: float4 number (w * 2 + r / 4) * 64 + lane, r < 8,
// + 8 bias sums (dsrcbias != NULL: every wave's sum of the one src channel, added up while staging).
// ------------------------------------------------------------------------------------------------
constexpr int kWgThinTTileFloats = 8 * 2 * 64 * 4;
constexpr int kWgThinTSetFloats = kWgThinTTileFloats + 8;
template <int WO>
__host__ __device__ constexpr int wgthint_cip() { return (((1024 / WO * 2 + 2) * (2 * WO)) / 16 | 1) * 16; }
template <int SPLIT, int WO>
__host__ __device__ constexpr int wgthint_lds_bytes() { return SPLIT * (2 * wgthint_cip<WO>() + 16 * 2064); }

template <int SPLIT, int WO>
__global__ __launch_bounds__(512, 1) void convt4s2_thin_wgrad_staged_kernel(
    const MtrssmConvGeom g, const float* __restrict__ a, const float* __restrict__ src, const int pre_act_a, float* __restrict__ dwp,
    float* __restrict__ part, float* __restrict__ dsrcbias, const int frames_per_wg) {
  static_assert(SPLIT == 1 || SPLIT == 2, "one or two bf16 pieces");
  static_assert(WO == 32 || WO == 16, "input plane 32x32 or 64x16");
  constexpr int NT = 512, CO = 16, HO = 1024 / WO, HS = 2 * HO, WS = 2 * WO;
  constexpr int ROWB = WS;                  // bytes per row of one parity image: WS / 2 bf16
  constexpr int XCOPY = wgthint_cip<WO>();  // one parity image of one piece: (HS + 2) rows, padded
  constexpr int AP = 2064, APB = CO * AP;   // `a` image: [ci][1024 pixels + 8] bf16
  constexpr int XI = HS * WS / 4 / NT, AI = CO * 1024 / 4 / NT, NI = XI + AI;  // 2 + 8 float4 items per thread and frame
  extern __shared__ __attribute__((aligned(16))) unsigned char wgthint_lds[];
  unsigned char* const lds = wgthint_lds;   // [piece][even image][odd image] then [piece][a image]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int il = lane & 31, kl = lane >> 5;
  const int n0 = blockIdx.x * frames_per_wg;
  const int n1 = n0 + frames_per_wg < g.N ? n0 + frames_per_wg : g.N;
  if (n0 >= n1) return;  // whole workgroup
  const int nlast = n1 - 1;

  const bool act_elu = g.act == MTRSSM_ACT_ELU, act_relu = g.act == MTRSSM_ACT_RELU, pre = pre_act_a != 0;
  const WgActSel act_sel{act_elu, act_relu, pre};

  for (int o = tid * 16; o < wgthint_lds_bytes<SPLIT, WO>(); o += NT * 16) *reinterpret_cast<uint4*>(lds + o) = make_uint4(0u, 0u, 0u, 0u);

  const float4* const xsrc = reinterpret_cast<const float4*>(src) + tid;
  const float4* const asrc = reinterpret_cast<const float4*>(a) + tid;
  constexpr size_t xfr = (size_t)HS * WS / 4, afr = (size_t)CO * 1024 / 4;  // float4 per frame
  float bsum = 0.f;  // this thread's share of the one src channel
  wg_f32x4 raw[3][NI];  // [set][a items, src items]
  auto raw_load = [&](const int rs, const int n) __attribute__((always_inline)) { wg_raw_load<NT, AI, XI>(raw[rs], asrc, afr, xsrc, xfr, n); };
  auto raw_wait = [&](const int rs) __attribute__((always_inline)) { wg_raw_wait<2 * NI>(raw[rs]); };  // the two younger sets may still be in flight
  auto stage = [&](const int rs) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      const wg_f32x4 v = raw[rs][it];
      if (it < AI) {
        unsigned d0[SPLIT], d1[SPLIT];
        wg_split_pair<SPLIT>(act_sel(v.x), act_sel(v.y), d0);
        wg_split_pair<SPLIT>(act_sel(v.z), act_sel(v.w), d1);
        const int f = tid + NT * it;  // ci = f / 256, pixel = 4 (f % 256)
        const unsigned o = (unsigned)(SPLIT * 2 * XCOPY) + (unsigned)((f >> 8) * AP + (f & 255) * 8);
#pragma unroll
        for (int p = 0; p < SPLIT; ++p) *reinterpret_cast<uint2*>(lds + o + p * APB) = make_uint2(d0[p], d1[p]);
      } else {
        unsigned de[SPLIT], dd[SPLIT];  // even columns (c0, c0 + 2), odd columns (c0 + 1, c0 + 3)
        bsum += (v.x + v.y) + (v.z + v.w);
        wg_split_pair<SPLIT>(v.x, v.z, de);
        wg_split_pair<SPLIT>(v.y, v.w, dd);
        const int f = tid + NT * (it - AI);
        const int row = f / (WS / 4), c4 = f - row * (WS / 4);
        const unsigned o = (unsigned)((row + 1) * ROWB + c4 * 4);
#pragma unroll
        for (int p = 0; p < SPLIT; ++p) {
          *reinterpret_cast<unsigned*>(lds + o + p * 2 * XCOPY) = de[p];
          *reinterpret_cast<unsigned*>(lds + o + p * 2 * XCOPY + XCOPY) = dd[p];
        }
      }
    }
  };

  // the lane's column = tap il & 15 (lanes 16 .. 31 repeat the columns, never stored)
  const int tap = il & 15, ky = tap >> 2, kx = tap & 3;
  const bool odd = kx == 0 || kx == 2;
  const unsigned lane_b = (unsigned)((odd ? XCOPY : 0) + ky * ROWB + kl * 16);
  const unsigned lane_a = (unsigned)(SPLIT * 2 * XCOPY + (il & 15) * AP + kl * 16);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  raw_load(0, n0);
  raw_load(1, n0 + 1 < nlast ? n0 + 1 : nlast);
  auto frame = [&](const int n, const int rs) __attribute__((always_inline)) {  // rs = (n - n0) % 3, a literal at the call sites
    raw_load((rs + 2) % 3, n + 2 < nlast ? n + 2 : nlast);  // its set held frame n - 1, staged a frame ago
    raw_wait(rs);
    lds_barrier();  // every wave is done reading the previous frame's images (first frame: the zeroes are in place)
    stage(rs);
    lds_barrier();  // images complete
#pragma unroll
    for (int ss = 0; ss < 8; ++ss) {
      const int s = wave * 8 + ss;  // k-step: input pixels 16 s .. 16 s + 15; WO = 32: row s / 2, half s & 1; WO = 16: row s
      const unsigned soff = WO == 32 ? (unsigned)((s >> 1) * 2 * ROWB + (s & 1) * 32) : (unsigned)(s * 2 * ROWB);
      const bool has_prev = WO == 32 ? ((s & 1) | kl) != 0 : kl != 0;
      const bool has_next = WO == 32 ? ((s & 1) & kl) == 0 : kl == 0;
      u32x4 qa[SPLIT], qb[SPLIT];
#pragma unroll
      for (int p = 0; p < SPLIT; ++p) {
        qa[p] = *reinterpret_cast<const u32x4*>(lds + lane_a + (unsigned)(p * APB) + (unsigned)(s * 32));
        const unsigned bo = lane_b + (unsigned)(p * 2 * XCOPY) + soff;
        const u32x4 f = *reinterpret_cast<const u32x4*>(lds + bo);
        const unsigned prev = has_prev ? (unsigned)*reinterpret_cast<const unsigned short*>(lds + bo - 2) : 0u;
        const unsigned next = has_next ? (unsigned)*reinterpret_cast<const unsigned short*>(lds + bo + 16) : 0u;
        const u32x4 shr = u32x4{(f.x << 16) | prev, __builtin_amdgcn_alignbit(f.y, f.x, 16), __builtin_amdgcn_alignbit(f.z, f.y, 16), __builtin_amdgcn_alignbit(f.w, f.z, 16)};
        const u32x4 shl = u32x4{__builtin_amdgcn_alignbit(f.y, f.x, 16), __builtin_amdgcn_alignbit(f.z, f.y, 16), __builtin_amdgcn_alignbit(f.w, f.z, 16), (f.w >> 16) | (next << 16)};
        qb[p] = kx == 0 ? shr : (kx == 3 ? shl : f);
      }
      wg_mfma_pieces<SPLIT>(acc, qa, qb);
    }
  };
#pragma unroll 1
  for (int n = n0; n < n1; n += 3) {
    frame(n, 0);
    if (n + 1 < n1) frame(n + 1, 1);
    if (n + 2 < n1) frame(n + 2, 2);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped requests of the last frames

  if (part) {
    float4* const ps = reinterpret_cast<float4*>(part) + (size_t)blockIdx.x * (kWgThinTSetFloats / 4) + (size_t)wave * 128 + lane;
    ps[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);   // rows 4 kl + 0 .. 3
    ps[64] = make_float4(acc[4], acc[5], acc[6], acc[7]);  // rows 8 + 4 kl + 0 .. 3
  } else if (il < 16) {
#pragma unroll
    for (int r = 0; r < 8; ++r) atomicAdd(&dwp[((size_t)wg_tile_row(r, kl) * 16 + tap) * g.Cpad], acc[r]);
  }
  if (dsrcbias != nullptr) {
    const float v = wave_sum(bsum);
    if (lane == 0) {
      if (part) part[(size_t)blockIdx.x * kWgThinTSetFloats + kWgThinTTileFloats + wave] = v;
      else atomicAdd(&dsrcbias[0], v);
    }
  }
}

// Partial sets of convt4s2_thin_wgrad_staged_kernel into dwp: one tile, eight k-parts (waves) per workgroup; float4 f = half *
// 64 + lane, 128 of them (host: 16 blocks).  Its bias is ONE word: block 16 (launched when dbias != NULL) is
// wgrad_reduce_thint_bias below, not a column of this layout.
struct WgRedThinT {
  static constexpr int NL = 8, NG = 32, U = 2, KS = 8, SET4 = kWgThinTSetFloats / 4;
  static __device__ __forceinline__ WgRedCol column(const int f, const int by) { return {(size_t)f, 128, -1, false}; }
  static __device__ __forceinline__ void scatter(const int f, const int by, const float4 v, const int cpad, float* __restrict__ dwp) {
    const int half = f >> 6, lane = f & 63, il = lane & 31, kl = lane >> 5;
    if (il < 16) wg_red_add_rows(dwp + ((size_t)(8 * half + 4 * kl) * 16 + il) * cpad, (size_t)16 * cpad, v);
  }
};
// the 8 S wave sums of src (one float per wave behind every set's tile) into dbias[0]
__device__ __forceinline__ void wgrad_reduce_thint_bias(float4* const red /* [32][8] */, const float4* __restrict__ part, const int S, float* __restrict__ dbias) {
  constexpr int NL = 8, NG = 32;
  const int li = threadIdx.x & (NL - 1), sg = threadIdx.x / NL;
  const float* const pb = reinterpret_cast<const float*>(part) + kWgThinTTileFloats + li;  // wave li of every workgroup
  float t = 0.f;
  for (int s = sg; s < S; s += NG) t += pb[(size_t)s * kWgThinTSetFloats];
  red[sg * NL + li].x = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = 0.f;
    for (int k = 0; k < NG * NL; ++k) v += red[k].x;
    dbias[0] += v;
  }
}

// ------------------------------------------------------------------------------------------------
// ... and of the THIRD encoder layer (3x3 / stride 2 / pad 1, 16 -> 32 channels, 64-pixel output planes: 8x8 vision, 16x4
// audio): 144 (tap, ci) columns in five 32-column tiles (waves 0 - 4, the rest only stage), all 32 rows, four k-steps per
// frame.  A lane's 8 output pixels are one whole row (8x8) or two whole rows (16x4: two 8-byte reads two image rows apart),
// so kx = 0 is a funnel shift with zeros.  Partial set: float4 number (w * 4 + r / 4) * 64 + lane, + 32 bias sums.
// ------------------------------------------------------------------------------------------------
constexpr int kWgS2cSetFloats = 8 * 4 * 64 * 4 + 32;
template <int SPLIT>
__host__ __device__ constexpr int wgs2c_lds_bytes() { return SPLIT * (2 * 16 * 272 + 32 * kWgresAPitch); }

template <int SPLIT, int WO>
__global__ __launch_bounds__(512, 1) void conv3x3s2c_wgrad_staged_kernel(
    const MtrssmConvGeom g, const float* __restrict__ a, const float* __restrict__ src, float* __restrict__ dwp,
    float* __restrict__ part, float* __restrict__ dbias, const int frames_per_wg) {
  static_assert(SPLIT == 1 || SPLIT == 2, "one or two bf16 pieces");
  static_assert(WO == 8 || WO == 4, "output plane 8x8 or 16x4");
  constexpr int NT = 512, C = 16, CO = 32, HO = 64 / WO, HS = 2 * HO, WS = 2 * WO;
  constexpr int ROWB = WS;                 // bytes per row of one parity image: WS / 2 bf16
  constexpr int CIP = 272;                 // bytes per channel: (HS + 1) rows (272 / 264 bytes), an odd number of 16-byte slots
  static_assert((HS + 1) * ROWB <= CIP, "channel pitch");
  constexpr int XCOPY = C * CIP;           // one parity image of one piece
  constexpr int AP = kWgresAPitch, APB = CO * AP;  // `a` image: [co][64 pixels + 8] bf16
  constexpr int XI = C * HS * WS / 4 / NT, AI = CO * 64 / 4 / NT, NI = XI + AI;  // 2 + 1 float4 items per thread and frame
  extern __shared__ __attribute__((aligned(16))) unsigned char wgs2c_lds[];
  unsigned char* const lds = wgs2c_lds;    // [piece][even image][odd image] then [piece][a image]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int il = lane & 31, kl = lane >> 5;
  const int n0 = blockIdx.x * frames_per_wg;
  const int n1 = n0 + frames_per_wg < g.N ? n0 + frames_per_wg : g.N;
  if (n0 >= n1) return;  // whole workgroup
  const int nlast = n1 - 1;

  const bool act_elu = g.act == MTRSSM_ACT_ELU, act_relu = g.act == MTRSSM_ACT_RELU, pre = g.pre_act != 0;
  const WgActSel act_sel{act_elu, act_relu, pre};

  for (int o = tid * 16; o < wgs2c_lds_bytes<SPLIT>(); o += NT * 16) *reinterpret_cast<uint4*>(lds + o) = make_uint4(0u, 0u, 0u, 0u);

  const float4* const xsrc = reinterpret_cast<const float4*>(src) + tid;
  const float4* const asrc = reinterpret_cast<const float4*>(a) + tid;
  constexpr size_t xfr = (size_t)C * HS * WS / 4, afr = (size_t)CO * 64 / 4;  // float4 per frame
  float bsum = 0.f;  // this thread's share of channel tid / 16
  wg_f32x4 raw[3][NI];  // [set][a item, src items]
  auto raw_load = [&](const int rs, const int n) __attribute__((always_inline)) { wg_raw_load<NT, AI, XI>(raw[rs], asrc, afr, xsrc, xfr, n); };
  auto raw_wait = [&](const int rs) __attribute__((always_inline)) { wg_raw_wait<2 * NI>(raw[rs]); };  // the two younger sets may still be in flight
  auto stage = [&](const int rs) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      const wg_f32x4 v = raw[rs][it];
      if (it < AI) {
        bsum += (v.x + v.y) + (v.z + v.w);
        unsigned d0[SPLIT], d1[SPLIT];
        wg_split_pair<SPLIT>(v.x, v.y, d0);
        wg_split_pair<SPLIT>(v.z, v.w, d1);
        const unsigned o = (unsigned)(SPLIT * 2 * XCOPY) + (unsigned)((tid >> 4) * AP + (tid & 15) * 8);
#pragma unroll
        for (int p = 0; p < SPLIT; ++p) *reinterpret_cast<uint2*>(lds + o + p * APB) = make_uint2(d0[p], d1[p]);
      } else {
        unsigned de[SPLIT], dd[SPLIT];  // even columns (c0, c0 + 2), odd columns (c0 + 1, c0 + 3)
        wg_split_pair<SPLIT>(act_sel(v.x), act_sel(v.z), de);
        wg_split_pair<SPLIT>(act_sel(v.y), act_sel(v.w), dd);
        const int f = tid + NT * (it - AI);
        const int ci = f / (HS * WS / 4), rem = f - ci * (HS * WS / 4), row = rem / (WS / 4), c4 = rem - row * (WS / 4);
        const unsigned o = (unsigned)(ci * CIP + (row + 1) * ROWB + c4 * 4);
#pragma unroll
        for (int p = 0; p < SPLIT; ++p) {
          *reinterpret_cast<unsigned*>(lds + o + p * 2 * XCOPY) = de[p];
          *reinterpret_cast<unsigned*>(lds + o + p * 2 * XCOPY + XCOPY) = dd[p];
        }
      }
    }
  };

  // the lane's column: (tap, ci) = (col >> 4, col & 15); columns 144 .. 159 of tile 4 are padding (computed on column 143)
  const int col = wave * 32 + il, colc = col < 144 ? col : 143;
  const int tap = colc >> 4, ci = colc & 15, ky = tap / 3, kx = tap - 3 * ky;
  // k-step s covers output pixels 16 s .. 16 s + 15, this lane 8 of them: WO = 8: row 2 s + kl; WO = 4: rows 4 s + 2 kl, + 1
  const unsigned lane_b = (unsigned)((kx == 1 ? 0 : XCOPY) + ci * CIP + ky * ROWB + kl * (WO == 8 ? 2 * ROWB : 4 * ROWB));
  constexpr unsigned kStepB = WO == 8 ? 4 * ROWB : 8 * ROWB;
  const unsigned lane_a = (unsigned)(SPLIT * 2 * XCOPY + il * AP + kl * 16);
  const bool shifted = kx == 0;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  raw_load(0, n0);
  raw_load(1, n0 + 1 < nlast ? n0 + 1 : nlast);
  auto frame = [&](const int n, const int rs) __attribute__((always_inline)) {  // rs = (n - n0) % 3, a literal at the call sites
    raw_load((rs + 2) % 3, n + 2 < nlast ? n + 2 : nlast);  // its set held frame n - 1, staged a frame ago
    raw_wait(rs);
    lds_barrier();  // every wave is done reading the previous frame's images (first frame: the zeroes are in place)
    stage(rs);
    lds_barrier();  // images complete
    if (wave < 5) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        u32x4 qa[SPLIT], qb[SPLIT];
#pragma unroll
        for (int p = 0; p < SPLIT; ++p) {
          qa[p] = *reinterpret_cast<const u32x4*>(lds + lane_a + (unsigned)(p * APB) + (unsigned)(s * 32));
          const unsigned bo = lane_b + (unsigned)(p * 2 * XCOPY) + (unsigned)s * kStepB;
          u32x4 f;
          if (WO == 8) {
            f = *reinterpret_cast<const u32x4*>(lds + bo);
          } else {
            const uint2 r0 = *reinterpret_cast<const uint2*>(lds + bo), r1 = *reinterpret_cast<const uint2*>(lds + bo + 2 * ROWB);
            f = u32x4{r0.x, r0.y, r1.x, r1.y};
          }
          const u32x4 sh = wg_rows_shift_in_front<WO == 8 ? 1 : 2>(f);
          qb[p] = shifted ? sh : f;
        }
#pragma unroll
        for (int ord = SPLIT - 1; ord >= 0; --ord)
#pragma unroll
          for (int sa = 0; sa <= ord; ++sa)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, qa[sa]), __builtin_bit_cast(bf16x8, qb[ord - sa]), acc, 0, 0, 0);
      }
    }
  };
#pragma unroll 1
  for (int n = n0; n < n1; n += 3) {
    frame(n, 0);
    if (n + 1 < n1) frame(n + 1, 1);
    if (n + 2 < n1) frame(n + 2, 2);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped requests of the last frames

  const float bv = wg_row16_sum(bsum);  // the 16 lanes of a DPP row share channel tid / 16
  if (part) {
    float* const set = part + (size_t)blockIdx.x * kWgS2cSetFloats;
    if (wave < 5) {
      float4* const ps = reinterpret_cast<float4*>(set) + (size_t)wave * 256 + lane;
      wg_store_tile(ps, acc);
    }
    if (dbias != nullptr && (tid & 15) == 0) set[8 * 4 * 64 * 4 + (tid >> 4)] = bv;
  } else {
    if (wave < 5 && col < 144) {
#pragma unroll
      for (int r = 0; r < 16; ++r) atomicAdd(&dwp[((size_t)wg_tile_row(r, kl) * 9 + tap) * g.Cpad + ci], acc[r]);
    }
    if (dbias != nullptr && (tid & 15) == 0) atomicAdd(&dbias[tid >> 4], bv);
  }
}

// Partial sets of conv3x3s2c_wgrad_staged_kernel: float4 f = (wave * 4 + gq) * 64 + lane of the five column tiles: 1280 (160
// blocks), then the bias block's 8 float4, all in use.
struct WgRedS2c {
  static constexpr int NL = 8, NG = 32, U = 4, KS = 1, SET4 = kWgS2cSetFloats / 4;
  static __device__ __forceinline__ WgRedCol column(const int f, const int by) {
    return {(size_t)(f >= 1280 ? 8 * 256 + (f - 1280) : f), 0, f >= 1280 ? 4 * (f - 1280) : -1, false};
  }
  static __device__ __forceinline__ void scatter(const int f, const int by, const float4 v, const int cpad, float* __restrict__ dwp) {
    const int lane = f & 63, gq = (f >> 6) & 3, wave = f >> 8, il = lane & 31, kl = lane >> 5;
    const int col = wave * 32 + il, tap = col >> 4, ci = col & 15, row = 8 * gq + 4 * kl;
    if (col < 144) wg_red_add_rows(dwp + ((size_t)row * 9 + tap) * cpad + ci, (size_t)9 * cpad, v);
  }
};

}  // namespace mtrssm
