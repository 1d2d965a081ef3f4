// mpcqp_lu3.h — the pivoted 3x3 solve shared by the torque map (mpcqp_torque.hip: swing legs,
// J tau = km .* f_kin) and the plant stage (mpcqp_plant.hip: J^-1, J^-T and I^-1).  Not installed.
#pragma once
#include "mpcqp_device.h"

namespace mpcqp {
namespace lu3 {

__device__ __forceinline__ void swap_if(bool s, double& x, double& y) {
  const double t = x;
  x = s ? y : x;
  y = s ? t : y;
}

// Eigen PartialPivLU<Matrix3d>(J).solve(b): pivot on the first maximal |a_ik|, swap whole rows
// (L part included), unit-lower forward and upper backward substitution.  Swaps are selects so
// nothing is indexed at run time.  a and b are overwritten.
__device__ __forceinline__ void lu3_solve(double (&a)[9], double (&b)[3], double (&x)[3]) {
#pragma clang fp contract(off)
  {  // column 0
    const double m0 = dabs(a[0]), m1 = dabs(a[3]), m2 = dabs(a[6]);
    const bool p1 = m1 > m0;
    double best = p1 ? m1 : m0;
    const bool p2 = m2 > best;
    best = p2 ? m2 : best;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      swap_if(p2, a[j], a[6 + j]);
      swap_if(!p2 && p1, a[j], a[3 + j]);
    }
    swap_if(p2, b[0], b[2]);
    swap_if(!p2 && p1, b[0], b[1]);
    if (best != 0.0) {
      a[3] /= a[0];
      a[6] /= a[0];
    }
    a[4] -= a[3] * a[1];
    a[5] -= a[3] * a[2];
    a[7] -= a[6] * a[1];
    a[8] -= a[6] * a[2];
  }
  {  // column 1
    const double m1 = dabs(a[4]), m2 = dabs(a[7]);
    const bool q = m2 > m1;
    const double best = q ? m2 : m1;
#pragma unroll
    for (int j = 0; j < 3; ++j) swap_if(q, a[3 + j], a[6 + j]);
    swap_if(q, b[1], b[2]);
    if (best != 0.0) a[7] /= a[4];
    a[8] -= a[7] * a[5];
  }
  const double y0 = b[0], y1 = b[1] - a[3] * y0, y2 = (b[2] - a[6] * y0) - a[7] * y1;
  x[2] = y2 / a[8];
  x[1] = (y1 - a[5] * x[2]) / a[4];
  x[0] = ((y0 - a[1] * x[1]) - a[2] * x[2]) / a[0];
}

}  // namespace lu3
}  // namespace mpcqp
