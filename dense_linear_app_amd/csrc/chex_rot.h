// The arithmetic of chol_chex_tile's right shift (chex.hip, job 1), spelled once: the rotation made from the moved row
// and what it does to another row.  The left shift (job 2) is chud_rot.h's rotation of one vector with sigma = +1 and
// has no arithmetic of its own.  Every sum of a product and a term is one fma, as there; tests/chex_model.py is the
// same arithmetic in numpy (without the fused multiply-adds).
#pragma once
#include "chud_rot.h"

namespace cholmi {

// the pivot of the rotation of column i against the moved row: rho^2 = x^2 + y^2, x = L(l,i), y the pivot of column
// i + 1 (L(l,l) at the start).  -> false when rho^2 is not positive (or NaN): then rho = y
template <typename T>
__device__ __forceinline__ bool chex_pivot(T x, T y, T &rho) {
  const T d2 = chud_fma<T>(x, x, y * y);
  if (!(d2 > T(0))) {
    rho = y;
    return false;
  }
  rho = chud_sqrt<T>(d2);
  return true;
}

// its two quotients: q = 0: cc = y / rho, 1: ss = x / rho
template <typename T>
__device__ __forceinline__ T chex_quotient(int q, T x, T y, T rho) {
  return (q == 0 ? y : x) / rho;
}

// another row r: a = L(r,i), b what the columns right of i left -> the row's entry of the new column i + 1;
// b <- what goes on to column i - 1
template <typename T>
__device__ __forceinline__ T chex_apply(T a, T &b, T cc, T ss) {
  const T out = chud_fma<T>(cc, a, -(ss * b));
  b = chud_fma<T>(ss, a, cc * b);
  return out;
}

}  // namespace cholmi
