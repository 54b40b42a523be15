// The NN block product shared by inverse.hip (the tiled triangular inverse of trtri / potri) and sygst.hip (the
// diagonal-tile products and the deferred left solve of sygst): one workgroup of four waves owns a 128 x 128 output
// block, one wave 64 x 64 of it, the operands read from L2 straight into registers.  See inverse.hip for the
// fragment layout.  Every output element is summed by one lane in a fixed order.
#pragma once
#include "cholmi_internal.h"
#include "mfma_traits.h"

namespace cholmi {

namespace {

// acc += A(i0 .. i0+63, kb .. ke) B(kb .. ke, j0 .. j0+63); A(r,k) at A[r + k lda], B(k,c) at B[k + c ldb];
// kb, ke multiples of 16.  TRA: A is lower triangular (A(r,k) = 0 for k > r), TRB: B is (B(k,c) = 0 for k < c):
// the other triangle is never used, whatever it holds.
template <typename T, bool TRA, bool TRB>
__device__ __forceinline__ void nn_acc(const T *__restrict__ A, int lda, const T *__restrict__ B, int ldb, int i0,
                                       int j0, int kb, int ke, Acc<T> &acc) {
  using vec4_t = typename Tr<T>::acc_t;
  const int lane = threadIdx.x & 63, c = lane & 15, g4 = (lane >> 4) * 4;
  for (int k0 = kb; k0 < ke; k0 += 16) {
    T xa[4][4], xb[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int row = i0 + 16 * a + c;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = k0 + g4 + s;
        xa[a][s] = A[row + (long)k * lda];
        if (TRA && k > row) xa[a][s] = T(0);
      }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int col = j0 + 16 * b + c;
      const vec4_t v = *reinterpret_cast<const vec4_t *>(B + (k0 + g4) + (long)col * ldb);
#pragma unroll
      for (int s = 0; s < 4; ++s) xb[b][s] = (TRB && k0 + g4 + s < col) ? T(0) : v[s];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = Tr<T>::mfma(xb[b][s], xa[a][s], acc[a][b]);
  }
}

// C(i0 + 16a + (lane & 15), j0 + 16b + drow(lane, r)) = alpha acc[a][b][r]
template <typename T>
__device__ __forceinline__ void acc_store(T *C, int ldc, int i0, int j0, const Acc<T> &acc, T alpha) {
  const int lane = threadIdx.x & 63, c = lane & 15;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        C[(i0 + 16 * a + c) + (long)(j0 + 16 * b + Tr<T>::drow(lane, r)) * ldc] = alpha * acc[a][b][r];
}

}  // namespace

}  // namespace cholmi
