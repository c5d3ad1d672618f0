// knn_sq_arith.h -- the roundings of the SQ8 contract (include/knnx.h, "IVF-SQ8"), shared by the IVF-SQ8 kernels (knn_sq_kernels.hip)
// and the SQ8 refine store of IVF-PQ (knn_pqsq_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace knnx {

// The contract fixes where every rounding falls (encode: subtract, then multiply; decode and score: multiply, then add).  hipcc
// contracts a * b + c into one fma by default, so these pin the two-rounding forms.
__device__ __forceinline__ float sq_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float sq_mul_add(float a, float b, float c) {  // c + round(a * b)
#pragma clang fp contract(off)
  const float p = a * b;
  return c + p;
}
__device__ __forceinline__ float sq_sub_mul(float a, float b, float c) {  // round(a - b) * c
#pragma clang fp contract(off)
  const float t = a - b;
  return t * c;
}

}  // namespace knnx
