// Double-precision reductions over a 16-lane DPP row, shared by the kernels that give a batch row one row of lanes and a sample or
// particle one lane (mtrssm_iw_bound in likelihood_ops.hip, mtrssm_particle_fold in particle_ops.hip).
#pragma once
#include "scan_common.h"

namespace mtrssm {

// One DPP step of a double: both halves move through the same lane permutation.
template <int CTRL>
__device__ __forceinline__ double dpp_move_d(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
// Sum / max over a 16-lane DPP row (every lane of the row gets the result, bitwise the same: each step adds two values that
// the partner lane adds in the other order).  All 64 lanes must be active.
__device__ __forceinline__ double row_sum_d(double v) {
  v += dpp_move_d<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += dpp_move_d<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += dpp_move_d<0x141>(v);  // row_half_mirror
  v += dpp_move_d<0x140>(v);  // row_mirror
  return v;
}
__device__ __forceinline__ double row_max_d(double v) {
  v = fmax(v, dpp_move_d<0xB1>(v));
  v = fmax(v, dpp_move_d<0x4E>(v));
  v = fmax(v, dpp_move_d<0x141>(v));
  v = fmax(v, dpp_move_d<0x140>(v));
  return v;
}

}  // namespace mtrssm
