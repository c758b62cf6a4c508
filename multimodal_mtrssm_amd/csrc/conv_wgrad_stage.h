// Pieces the staged weight-gradient kernels of conv_wgrad_resident.h share (included by conv.hip behind conv_split.h): the
// activation select, raw register sets requested ahead and their counter wait, the ordered piece products, funnel shifts,
// the 32-row tile's rows and store -- and the sum of their partial sets, written once for every set layout.  What is per
// layer (LDS image geometry, column-to-tap mapping, which operand is activated) stays in the kernels.
//
// A helper here is used by a kernel only where the kernel's machine code stays what it was with the text written out in
// place (profiles/wgrad_staged_refactor_notes.md, section 2): the schedules of these kernels move with the order of the IR
// they are built from.  That is why the helpers take their operands the way the kernels' own lambdas captured them (by
// reference), why a few kernels keep a piece of their own (named at the helper), and why the run of frames and the unrolled
// frame loop are still written out in every kernel.
#pragma once

namespace mtrssm {

using wg_bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using wg_f32x2 = __attribute__((ext_vector_type(2))) float;
using wg_f32x4 = __attribute__((ext_vector_type(4))) float;  // a register quadruple inline asm can name (float4 is a struct)
// two values -> packed bf16 pieces (round to nearest even, as split_bf16): d[s] = piece s of (f0 low half, f1 high half)
template <int SPLIT>
__device__ __forceinline__ void wg_split_pair(const float f0, const float f1, unsigned (&d)[SPLIT]) {
  d[0] = __builtin_bit_cast(unsigned, __builtin_convertvector(wg_f32x2{f0, f1}, wg_bf16x2));
  if constexpr (SPLIT >= 2) {
    const float r0 = f0 - __builtin_bit_cast(float, d[0] << 16), r1 = f1 - __builtin_bit_cast(float, d[0] & 0xffff0000u);  // exact
    d[1] = __builtin_bit_cast(unsigned, __builtin_convertvector(wg_f32x2{r0, r1}, wg_bf16x2));
  }
}

// The layer's activation on a staged value, its switches as lane-uniform selects (no branch inside the MFMA loop: a branch
// ends a scheduling region).  pre == false: the value as it stands.  The switches are the kernel's own locals, read where they
// are used.  (conv1x1_bwd_fused_body always activates and keeps a select of its own without `pre`.)
struct WgActSel {
  const bool& elu;
  const bool& relu;
  const bool& pre;
  __device__ __forceinline__ float operator()(float x) const {
    float e = __expf(x) - 1.f;
    asm volatile("" : "+v"(e));  // computed unconditionally: the compiler would branch around the exponential
    const float neg = elu ? e : (relu ? 0.f : x);
    return (x > 0.f || !pre) ? x : neg;
  }
};

// ---- raw frames: register sets requested ahead -------------------------------------------------------------------------
// A frame's raw values are float4 items per thread: item `it` of an operand = float4 number tid + NT * it of the frame.  The
// requests are inline asm: the compiler sinks its own loads to their uses, a frame later (and then waits for them there).  As
// volatile asm they keep their place among the LDS operations; wg_raw_wait is the matching counter wait.
// One set = [I0 items of operand 0][I1 items of operand 1]; p0 / p1 already point at the thread's float4 of frame 0, fr0 /
// fr1 = float4 per frame.  (conv3x3_wgrad_resident_body, src items first and NT a template value, keeps its own.)
template <int NT, int I0, int I1>
__device__ __forceinline__ void wg_raw_load(wg_f32x4 (&set)[I0 + I1], const float4* const& p0, const size_t fr0, const float4* const& p1, const size_t fr1, const int n) {
#pragma unroll
  for (int it = 0; it < I0 + I1; ++it) {
    const float4* const ptr = it < I0 ? p0 + (size_t)n * fr0 + NT * it : p1 + (size_t)n * fr1 + NT * (it - I0);
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(set[it]) : "v"(ptr));
  }
}
// Waits until at most BEHIND loads are in flight and ties every register of the set to the wait.  BEHIND = the loads issued
// BEHIND the set's own (loads return in order among themselves): with three sets requested two frames ahead the two younger
// sets, 2 * NI; with two sets requested one frame ahead and waited for before the next request, 0; the fused 1x1 backward adds
// its act' operand loads.  (Inline asm takes no parameter pack: one line per item count in use.)
#define MTRSSM_WG_R(i_) "+v"(set[i_])
template <int BEHIND, int NI>
__device__ __forceinline__ void wg_raw_wait(wg_f32x4 (&set)[NI]) {
  static_assert(NI == 3 || NI == 4 || NI == 6 || NI == 8 || NI == 10 || NI == 12, "item counts in use");
  if constexpr (NI == 3) asm volatile("s_waitcnt vmcnt(%3)" : MTRSSM_WG_R(0), MTRSSM_WG_R(1), MTRSSM_WG_R(2) : "n"(BEHIND));
  else if constexpr (NI == 4) asm volatile("s_waitcnt vmcnt(%4)" : MTRSSM_WG_R(0), MTRSSM_WG_R(1), MTRSSM_WG_R(2), MTRSSM_WG_R(3) : "n"(BEHIND));
  else if constexpr (NI == 6)
    asm volatile("s_waitcnt vmcnt(%6)" : MTRSSM_WG_R(0), MTRSSM_WG_R(1), MTRSSM_WG_R(2), MTRSSM_WG_R(3), MTRSSM_WG_R(4), MTRSSM_WG_R(5) : "n"(BEHIND));
  else if constexpr (NI == 8)
    asm volatile("s_waitcnt vmcnt(%8)" : MTRSSM_WG_R(0), MTRSSM_WG_R(1), MTRSSM_WG_R(2), MTRSSM_WG_R(3), MTRSSM_WG_R(4), MTRSSM_WG_R(5), MTRSSM_WG_R(6), MTRSSM_WG_R(7) : "n"(BEHIND));
  else if constexpr (NI == 10)
    asm volatile("s_waitcnt vmcnt(%10)" : MTRSSM_WG_R(0), MTRSSM_WG_R(1), MTRSSM_WG_R(2), MTRSSM_WG_R(3), MTRSSM_WG_R(4), MTRSSM_WG_R(5), MTRSSM_WG_R(6), MTRSSM_WG_R(7),
                 MTRSSM_WG_R(8), MTRSSM_WG_R(9) : "n"(BEHIND));
  else
    asm volatile("s_waitcnt vmcnt(%12)" : MTRSSM_WG_R(0), MTRSSM_WG_R(1), MTRSSM_WG_R(2), MTRSSM_WG_R(3), MTRSSM_WG_R(4), MTRSSM_WG_R(5), MTRSSM_WG_R(6), MTRSSM_WG_R(7),
                 MTRSSM_WG_R(8), MTRSSM_WG_R(9), MTRSSM_WG_R(10), MTRSSM_WG_R(11) : "n"(BEHIND));
}
#undef MTRSSM_WG_R

// ---- MFMAs ---------------------------------------------------------------------------------------------------------------
// The piece products of a SPLIT x SPLIT operand pair that count, smallest first: a[sa] b[sb] for sa + sb = SPLIT - 1 .. 0
// (two pieces: a0 b1, a1 b0, a0 b0; the a1 b1 term is below the fp32 grain), for a wave with one accumulator tile.  (The
// kernels with several tiles run their tile loop innermost, so that consecutive MFMAs go to different accumulators;
// conv3x3s2_wgrad_staged_kernel, conv3x3s2_thin_wgrad_staged_kernel and conv3x3s2c_wgrad_staged_kernel keep the loops
// written out: their two-piece forms schedule differently through a call.)
template <int SPLIT>
__device__ __forceinline__ void wg_mfma_pieces(f32x16& acc, const u32x4 (&qa)[SPLIT], const u32x4 (&qb)[SPLIT]) {
#pragma unroll
  for (int ord = SPLIT - 1; ord >= 0; --ord)
#pragma unroll
    for (int sa = 0; sa <= ord; ++sa)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, qa[sa]), __builtin_bit_cast(bf16x8, qb[ord - sa]), acc, 0, 0, 0);
}

// ---- one-element funnel shifts of a fragment of 8 bf16 -------------------------------------------------------------------
__device__ __forceinline__ unsigned wg_ab(const unsigned hi, const unsigned lo) { return __builtin_amdgcn_alignbit(hi, lo, 16); }
// element x <- x - 1 with `prev` (low half) in front.  (The two k = 4 kernels that also shift the other way, with an element
// behind, keep both funnels written out.)
__device__ __forceinline__ u32x4 wg_shift_in_front(const u32x4 f, const unsigned prev) {
  return u32x4{(f.x << 16) | prev, wg_ab(f.y, f.x), wg_ab(f.z, f.y), wg_ab(f.w, f.z)};
}
// ... of whole image rows (ROWS = 1: one row of 8, ROWS = 2: two rows of 4): zero into every row's first / last element
template <int ROWS>
__device__ __forceinline__ u32x4 wg_rows_shift_in_front(const u32x4 f) {
  return ROWS == 1 ? u32x4{f.x << 16, wg_ab(f.y, f.x), wg_ab(f.z, f.y), wg_ab(f.w, f.z)} : u32x4{f.x << 16, wg_ab(f.y, f.x), f.z << 16, wg_ab(f.w, f.z)};
}
template <int ROWS>
__device__ __forceinline__ u32x4 wg_rows_shift_behind(const u32x4 f) {
  return ROWS == 1 ? u32x4{wg_ab(f.y, f.x), wg_ab(f.z, f.y), wg_ab(f.w, f.z), f.w >> 16} : u32x4{wg_ab(f.y, f.x), f.y >> 16, wg_ab(f.w, f.z), f.w >> 16};
}

// ---- the 32-row accumulator tile -------------------------------------------------------------------------------------------
// register r of lane (il, kl) is row wg_tile_row(r, kl) of column il; `base` = the tile's first row, added first as the
// kernels did (the sum's association is part of their code)
__device__ __forceinline__ int wg_tile_row(const int r, const int kl, const int base = 0) { return base + (r & 3) + 8 * (r >> 2) + 4 * kl; }
// partial-set store in accumulator order: float4 gq (rows 8 gq + 4 kl + {0..3}) 64 float4 behind the one before, so that every
// store instruction of a wave writes 1 KiB in a row
__device__ __forceinline__ void wg_store_tile(float4* const ps, const f32x16& acc) {
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) ps[gq * 64] = make_float4(acc[4 * gq], acc[4 * gq + 1], acc[4 * gq + 2], acc[4 * gq + 3]);
}
// sum over the 16 lanes of a DPP row (the lanes that share a channel while staging)
__device__ __forceinline__ float wg_row16_sum(float v) {
  v += dpp_move<0xB1, 0xF>(0.f, v);   // quad_perm [1, 0, 3, 2]
  v += dpp_move<0x4E, 0xF>(0.f, v);   // quad_perm [2, 3, 0, 1]
  v += dpp_move<0x141, 0xF>(0.f, v);  // row_half_mirror
  v += dpp_move<0x140, 0xF>(0.f, v);  // row_mirror
  return v;
}

// ---- partial-set reduction -------------------------------------------------------------------------------------------
// A staged kernel leaves S partial sets (one per workgroup of a co group: part [cogroups][S][SET4] float4, accumulator
// order) and wgrad_reduce_batch_kernel (conv.hip) sums them into dwp / dbias.  A reduce workgroup of 256 threads is NL
// float4 columns of the set x NG slice groups; a thread walks its group's slices with U loads in flight, the groups meet in
// LDS (`red`, 256 float4 in either shape) and group 0 adds the column into dwp -- a plain read-modify-write: launches that
// accumulate into one dwp chunk are ordered by their stream.  (32, 8, 4) reads 512 contiguous bytes of a set per 32 lanes
// (with 128-byte pieces 147 KB apart the 520 MB of the residual layers' sets streamed at 3 TB/s); the small sets of the
// encoder / decoder layers take (8, 32, .) to have enough workgroups.
//
// What differs per kernel is a Layout:
//   NL, NG, U;  SET4 = float4 per set;  KS = k-parts a set holds per tile column (waves that hold the same tile);
//   column(f, by)  where float4 number f = bx * NL + li of the reduce grid finds its slices (the grid's last x block is the
//                  bias block, launched when dbias != NULL);
//   scatter(f, by, v, cpad, dwp)  the finished tile column into dwp (the inverse of the kernel's tile assignment).
// Slice i of a column = (set i / ks, k-part i % ks), ks = KS for a tile column and 1 for a bias column.  The order of the
// additions (slice walk, pairwise fold of the U accumulators, groups 1 .. NG - 1 onto group 0, then dwp) is fixed: the sums
// are run-to-run and build-to-build identical.
struct WgRedCol {
  size_t start;   // float4 offset of slice 0 within the co group's sets
  int kstride;    // float4 between the k-parts of a set
  int bias_ch;    // >= 0: a bias column (block-uniform), the sums of channels bias_ch .. + 3 of dbias;  -1: a tile column
  bool pad;       // padding of the bias block: nothing to read, nothing to write
};

__device__ __forceinline__ void wg_add4(float4& a, const float4 v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
// rows r .. r + 3 of one accumulator column: four words `rs` apart
__device__ __forceinline__ void wg_red_add_rows(float* const o, const size_t rs, const float4 v) {
  o[0] += v.x; o[rs] += v.y; o[2 * rs] += v.z; o[3 * rs] += v.w;
}

template <class L>
__device__ __forceinline__ void wgrad_reduce_sets(float4* const red /* [NG][NL] */, const float4* __restrict__ part, const int S, const int cpad,
                                                  float* __restrict__ dwp, float* __restrict__ dbias, const int bx, const int by) {
  constexpr int NL = L::NL, NG = L::NG, U = L::U;
  static_assert(NL * NG == 256 && (U == 2 || U == 4), "256 threads");
  const int li = threadIdx.x & (NL - 1), sg = threadIdx.x / NL;
  const int f = bx * NL + li;
  const WgRedCol col = L::column(f, by);
  const int ks = col.bias_ch >= 0 ? 1 : L::KS;
  float4 acc4[U];
#pragma unroll
  for (int u = 0; u < U; ++u) acc4[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!col.pad) {
    const float4* const p = part + (size_t)by * S * L::SET4 + col.start;
    auto slice = [&](const int i) __attribute__((always_inline)) {
      if constexpr (L::KS == 1) return p[(size_t)i * L::SET4];
      else return p[(size_t)(i / ks) * L::SET4 + (size_t)(i % ks) * col.kstride];
    };
    const int slices = S * ks;
    int i = sg;
    for (; i + (U - 1) * NG < slices; i += U * NG) {
#pragma unroll
      for (int u = 0; u < U; ++u) wg_add4(acc4[u], slice(i + NG * u));
    }
    for (; i < slices; i += NG) wg_add4(acc4[0], slice(i));
  }
  wg_add4(acc4[0], acc4[1]);
  if constexpr (U == 4) {
    wg_add4(acc4[2], acc4[3]);
    wg_add4(acc4[0], acc4[2]);
  }
  red[sg * NL + li] = acc4[0];
  __syncthreads();
  if (sg != 0 || col.pad) return;
  float4 v = red[li];
#pragma unroll
  for (int k = 1; k < NG; ++k) wg_add4(v, red[k * NL + li]);
  if (col.bias_ch >= 0) {
    float* const o = dbias + col.bias_ch;
    o[0] += v.x; o[1] += v.y; o[2] += v.z; o[3] += v.w;
  } else {
    L::scatter(f, by, v, cpad, dwp);
  }
}

}  // namespace mtrssm
