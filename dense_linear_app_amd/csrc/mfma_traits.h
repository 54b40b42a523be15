// The fp64 / fp32 16x16x4 MFMA as every kernel of the library sees it: vector types, the builtin, the row of the
// C/D map a lane's accumulator register holds, and the 4 x 4 accumulator of a 64 x 64 wave tile.  Included by
// kernels.hip and by nn_blocks.h (inverse.hip, sygst.hip, sytrf.hip); internal linkage in each unit.
#pragma once
#include <hip/hip_runtime.h>

namespace cholmi {

namespace {

typedef double d4_t __attribute__((ext_vector_type(4)));
typedef double d2_t __attribute__((ext_vector_type(2)));
typedef float f4_t __attribute__((ext_vector_type(4)));

template <typename T>
struct Tr;
template <>
struct Tr<double> {
  using acc_t = d4_t;
  using vec_t = d2_t;  // 16 bytes
  static constexpr int EPV = 2;
  static __device__ __forceinline__ acc_t mfma(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  // row of accumulator register `reg` held by `lane` (f64 16x16x4 C/D map)
  static __device__ __forceinline__ int drow(int lane, int reg) { return (lane >> 4) + 4 * reg; }
};
template <>
struct Tr<float> {
  using acc_t = f4_t;
  using vec_t = f4_t;
  static constexpr int EPV = 4;
  static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int drow(int lane, int reg) { return 4 * (lane >> 4) + reg; }
};

template <typename T>
using Acc = typename Tr<T>::acc_t[4][4];

// (any tile grid: the 4 x 4 above, the 4 x 2 of the eight-wave cores)
template <typename T, int NA, int NB>
__device__ __forceinline__ void acc_zero(typename Tr<T>::acc_t (&acc)[NA][NB]) {
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[a][b][r] = T(0);
}

}  // namespace

}  // namespace cholmi
