// norm_kernels.hip -- LayerNorm, the row statistics of the LayerNorm-folded GEMMs, the weight folding, and the fills / conversions
// the handle runs when it carves its weights.  One wave per row; fp32 statistics.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "clip_kernels.h"
#include "gemm_common.h"  // the vector typedefs, ln_rstd_onepass

namespace clipx {

// =============================================================================================
// LayerNorm: one wave per row, fp32 statistics (two-pass in registers)
// =============================================================================================
// Widths are multiples of 128 (D128 = d / 128).  A lane takes 4 consecutive values per step and a wave 256, so an odd D128 (1408 and
// 1664: the ViT-g/14 and ViT-bigG/14 image towers) ends in a half step that only lanes 0 .. 31 take part in (the `D128 % 2 != 0 &&`
// tests below).  For an even D128 the test is the constant false, and the kernels compile to the code they always have.
template <int D128, int OUT>  // d = D128 * 128; OUT 0: f32 (+ optional bf16 copy), 1: bf16, 2: IEEE fp16
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, void* __restrict__ y, int M,
                                                       float eps, bf16* __restrict__ y16) {
  constexpr int d = D128 * 128, NV = (D128 + 1) / 2;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * d);
  float4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    if (D128 % 2 != 0 && e == D128 / 2 && lane >= 32) continue;  // the half step of an odd D128
    v[e] = xr[lane + 64 * e];
    s += (v[e].x + v[e].y) + (v[e].z + v[e].w);
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s * (1.f / d);
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    if (D128 % 2 != 0 && e == D128 / 2 && lane >= 32) continue;  // the half step of an odd D128
    const float a = v[e].x - mean, b = v[e].y - mean, c = v[e].z - mean, dd = v[e].w - mean;
    q += (a * a + b * b) + (c * c + dd * dd);
  }
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  const float rstd = 1.f / sqrtf(q * (1.f / d) + eps);
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    if (D128 % 2 != 0 && e == D128 / 2 && lane >= 32) continue;  // the half step of an odd D128
    const int c4 = lane + 64 * e;
    const float4 g4 = reinterpret_cast<const float4*>(gamma)[c4];
    const float4 b4 = reinterpret_cast<const float4*>(beta)[c4];
    float4 o;
    o.x = (v[e].x - mean) * rstd * g4.x + b4.x;
    o.y = (v[e].y - mean) * rstd * g4.y + b4.y;
    o.z = (v[e].z - mean) * rstd * g4.z + b4.z;
    o.w = (v[e].w - mean) * rstd * g4.w + b4.w;
    if (OUT == 1) {
      bf16x4 ob;
      ob[0] = (bf16)o.x; ob[1] = (bf16)o.y; ob[2] = (bf16)o.z; ob[3] = (bf16)o.w;
      reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(y) + (size_t)row * d)[c4] = ob;
    } else if (OUT == 2) {
      f16x4 oh;
      oh[0] = (_Float16)o.x; oh[1] = (_Float16)o.y; oh[2] = (_Float16)o.z; oh[3] = (_Float16)o.w;
      reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(y) + (size_t)row * d)[c4] = oh;
    } else {
      reinterpret_cast<float4*>(reinterpret_cast<float*>(y) + (size_t)row * d)[c4] = o;
      if (y16) {
        bf16x4 ob;
        ob[0] = (bf16)o.x; ob[1] = (bf16)o.y; ob[2] = (bf16)o.z; ob[3] = (bf16)o.w;
        reinterpret_cast<bf16x4*>(y16 + (size_t)row * d)[c4] = ob;
      }
    }
  }
}

// rstd of the 16-bit shadow rows (see clip_kernels.h: launch_rowstats), two passes in registers: a lane holds 4 consecutive values
// per step of 256, the last step of an odd D128 in lanes 0 .. 31 only
template <int D128, bool F16>  // d = D128 * 128; F16: rows are IEEE fp16, else bf16
__device__ __forceinline__ void rowstats_row(const void* __restrict__ x16, float* __restrict__ rstd, int M, float eps,
                                             int* __restrict__ range_flag) {
  constexpr int d = D128 * 128, NV2 = (D128 + 1) / 2;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const uint2* xr = reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(x16) + (size_t)row * d);
  float v[NV2][4];
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < NV2; ++e) {
    if (D128 % 2 != 0 && e == D128 / 2 && lane >= 32) continue;  // the half step of an odd D128
    const uint2 raw = xr[lane + 64 * e];
    if (F16) {
      const f16x4 h = __builtin_bit_cast(f16x4, raw);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[e][j] = (float)h[j];
    } else {
      const bf16x4 h = __builtin_bit_cast(bf16x4, raw);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[e][j] = (float)h[j];
    }
    s += (v[e][0] + v[e][1]) + (v[e][2] + v[e][3]);
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  // Range guard of the fp16 residual stream (clipx.h: CLIPX_E_RANGE).  The residual epilogues round f32 -> fp16 to nearest, so a
  // value beyond 65 504 is stored as inf; every state of the stream passes through this kernel (or tail_proj_kernel) before it
  // is used, and a row holding inf / NaN has a non-finite sum (d finite fp16 values cannot overflow an f32).  Free: one
  // compare on a value the kernel has anyway.
  if (range_flag && lane == 0 && !(fabsf(s) <= 3.0e38f)) atomicOr(range_flag, 1);
  const float mean = s * (1.f / d);
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < NV2; ++e) {
    if (D128 % 2 != 0 && e == D128 / 2 && lane >= 32) continue;  // the half step of an odd D128
    const float a = v[e][0] - mean, b = v[e][1] - mean, c = v[e][2] - mean, dd = v[e][3] - mean;
    q += (a * a + b * b) + (c * c + dd * dd);
  }
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  if (lane == 0) rstd[row] = 1.f / sqrtf(q * (1.f / d) + eps);
}
// (stamp: the launch belongs to a profiled GEMM that owns its statistics, gemm_common.h stamp_start; null otherwise.  The waves
// past the last row return from rowstats_row early and still reach stamp_end's barrier)
template <int D128, bool F16>
__global__ __launch_bounds__(256) void rowstats_kernel(const void* __restrict__ x16, float* __restrict__ rstd, int M, float eps,
                                                       int* __restrict__ range_flag, StampSlot* stamp) {
  stamp_start(stamp, blockIdx.x);
  rowstats_row<D128, F16>(x16, rstd, M, eps, range_flag);
  stamp_end(stamp, blockIdx.x);
}

// The fp16 stream: ONE pass in the canonical order (gemm_common.h: ln_rstd_onepass) -- four lanes per row (lane = r16 + 16 q4, the
// fragment layout of the 4-wave GEMM kernel, which computes the same sums for the rows it multiplies), lane part q4 takes the 16-B
// chunks q4, q4 + 4, ..; a wave covers 16 rows, a workgroup 64.  Widths that are odd multiples of 128 (1408, 1664: 44 and 52 chunks
// per lane part) keep 4 chunks in flight instead of 8; the sums are one chain per lane part in ascending chunk order whatever the
// number in flight, which is the order of the GEMM's K loop at any K that is a multiple of 128: the same bits at the new widths too.
template <int D128>  // d = D128 * 128
__device__ __forceinline__ void rowstats_f16_rows(const void* __restrict__ x16, float* __restrict__ rstd, int M, float eps,
                                                  int* __restrict__ range_flag) {
  constexpr int d = D128 * 128, NCH = d / 8;
  const int lane = threadIdx.x & 63, q4 = lane >> 4, r16 = lane & 15;
  const int row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + r16;
  const uint4* xr = reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(x16) + (size_t)(row < M ? row : M - 1) * d);
  const unsigned ones2 = __builtin_amdgcn_readfirstlane(0x3c003c00u);
  float s1 = 0.f, s2 = 0.f;
  constexpr int U = D128 % 2 == 0 ? 8 : 4;  // chunks in flight per lane
  static_assert((NCH / 4) % U == 0, "row length");
  for (int j0 = 0; j0 < NCH / 4; j0 += U) {
    uint4 c[U];
#pragma unroll
    for (int u = 0; u < U; ++u) c[u] = xr[q4 + 4 * (j0 + u)];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      CLIPX_DOT2_SQ(s2, c[u].x); CLIPX_DOT2_SQ(s2, c[u].y); CLIPX_DOT2_SQ(s2, c[u].z); CLIPX_DOT2_SQ(s2, c[u].w);
      CLIPX_DOT2_SUM(s1, c[u].x, ones2); CLIPX_DOT2_SUM(s1, c[u].y, ones2); CLIPX_DOT2_SUM(s1, c[u].z, ones2); CLIPX_DOT2_SUM(s1, c[u].w, ones2);
    }
  }
  s1 += __shfl_xor(s1, 16);
  s2 += __shfl_xor(s2, 16);
  s1 += __shfl_xor(s1, 32);
  s2 += __shfl_xor(s2, 32);
  if (row >= M || q4 != 0) return;
  // range guard of the fp16 residual stream (see rowstats_kernel): a row holding inf / NaN has a non-finite sum
  if (range_flag && !(fabsf(s1) <= 3.0e38f)) atomicOr(range_flag, 1);
  rstd[row] = ln_rstd_onepass(s1, s2, 1.f / (float)d, eps);
}
template <int D128>
__global__ __launch_bounds__(256) void rowstats_f16_kernel(const void* __restrict__ x16, float* __restrict__ rstd, int M, float eps,
                                                           int* __restrict__ range_flag, StampSlot* stamp) {
  stamp_start(stamp, blockIdx.x);
  rowstats_f16_rows<D128>(x16, rstd, M, eps, range_flag);
  stamp_end(stamp, blockIdx.x);
}

hipError_t launch_rowstats(const void* x16, float* rstd, int M, int d, float eps, hipStream_t st, int f16, int* range_flag, int canonical,
                           LaunchEvents* events) {
  if (M <= 0) return hipSuccess;
  if (f16 && canonical) {
    const dim3 grid((M + 63) / 64), block(256);
#define RSH_CASE(D128)                                                                                         \
  case D128 * 128:                                                                                             \
    launch_with_events(events, rowstats_f16_kernel<D128>, grid, block, 0, st, x16, rstd, M, eps, range_flag); \
    break;
    switch (d) {
      RSH_CASE(2) RSH_CASE(4) RSH_CASE(6) RSH_CASE(8) RSH_CASE(10) RSH_CASE(12) RSH_CASE(14) RSH_CASE(16)
      RSH_CASE(1) RSH_CASE(3) RSH_CASE(5) RSH_CASE(7) RSH_CASE(9) RSH_CASE(11) RSH_CASE(13) RSH_CASE(15)
      default: return hipErrorInvalidValue;
    }
#undef RSH_CASE
    return hipGetLastError();
  }
  const dim3 grid((M + 3) / 4), block(256);
#define RS_CASE(D128)                                                                                      \
  case D128 * 128:                                                                                         \
    if (f16) launch_with_events(events, rowstats_kernel<D128, true>, grid, block, 0, st, x16, rstd, M, eps, range_flag); \
    else launch_with_events(events, rowstats_kernel<D128, false>, grid, block, 0, st, x16, rstd, M, eps, range_flag);    \
    break;
  switch (d) {
    RS_CASE(2) RS_CASE(4) RS_CASE(6) RS_CASE(8) RS_CASE(10) RS_CASE(12) RS_CASE(14) RS_CASE(16)
    RS_CASE(1) RS_CASE(3) RS_CASE(5) RS_CASE(7) RS_CASE(9) RS_CASE(11) RS_CASE(13) RS_CASE(15)
    default: return hipErrorInvalidValue;
  }
#undef RS_CASE
  return hipGetLastError();
}

// one workgroup per output row n of W [N, K]
__global__ __launch_bounds__(256) void fold_layernorm_kernel(const float* __restrict__ W, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ bias,
                                                            bf16* __restrict__ Wf, float* __restrict__ cf, int K, int f16) {
  __shared__ float red[8];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* w = W + (size_t)n * K;
  float sg = 0.f, sb = 0.f;
  for (int k = tid; k < K; k += 256) {
    sg += w[k] * gamma[k];
    sb += w[k] * beta[k];
  }
  for (int o = 32; o > 0; o >>= 1) { sg += __shfl_xor(sg, o); sb += __shfl_xor(sb, o); }
  if ((tid & 63) == 0) { red[tid >> 6] = sg; red[4 + (tid >> 6)] = sb; }
  __syncthreads();
  const float mean = (red[0] + red[1] + red[2] + red[3]) / (float)K;
  for (int k = tid; k < K; k += 256) {
    const float v = w[k] * gamma[k] - mean;
    if (f16) reinterpret_cast<_Float16*>(Wf)[(size_t)n * K + k] = (_Float16)v;
    else Wf[(size_t)n * K + k] = (bf16)v;
  }
  if (tid == 0) cf[n] = bias[n] + (red[4] + red[5] + red[6] + red[7]);
}
hipError_t launch_fold_layernorm(const float* W, const float* gamma, const float* beta, const float* bias, bf16* Wf, float* cf,
                                 int N, int K, hipStream_t st, int f16) {
  hipLaunchKernelGGL(fold_layernorm_kernel, dim3(N), dim3(256), 0, st, W, gamma, beta, bias, Wf, cf, K, f16);
  return hipGetLastError();
}
__global__ void fill_f32_kernel(float* __restrict__ p, float v, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}
hipError_t launch_fill_f32(float* p, float v, int64_t n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fill_f32_kernel, dim3(256), dim3(256), 0, st, p, v, n);
  return hipGetLastError();
}
__global__ void fill_stamps_kernel(StampEntry* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = StampEntry{STAMP_FILL_START, STAMP_FILL_END};
}
hipError_t launch_fill_stamps(StampSlot* slots, int64_t n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fill_stamps_kernel, dim3(256), dim3(256), 0, st, slots->way, n * STAMP_WAYS);
  return hipGetLastError();
}

hipError_t launch_layernorm(const float* x, const float* gamma, const float* beta, void* y, int out_kind, int M, int d,
                            float eps, hipStream_t st, bf16* y16) {
  if (M <= 0) return hipSuccess;
  const dim3 grid((M + 3) / 4), block(256);
#define LN_CASE(D128)                                                                                         \
  case D128 * 128:                                                                                            \
    if (out_kind == 1) hipLaunchKernelGGL((layernorm_kernel<D128, 1>), grid, block, 0, st, x, gamma, beta, y, M, eps, (bf16*)nullptr); \
    else if (out_kind == 2) hipLaunchKernelGGL((layernorm_kernel<D128, 2>), grid, block, 0, st, x, gamma, beta, y, M, eps, (bf16*)nullptr); \
    else hipLaunchKernelGGL((layernorm_kernel<D128, 0>), grid, block, 0, st, x, gamma, beta, y, M, eps, y16);  \
    break;
  switch (d) {
    LN_CASE(2) LN_CASE(4) LN_CASE(6) LN_CASE(8) LN_CASE(10) LN_CASE(12) LN_CASE(14) LN_CASE(16)
    LN_CASE(1) LN_CASE(3) LN_CASE(5) LN_CASE(7) LN_CASE(9) LN_CASE(11) LN_CASE(13) LN_CASE(15)
    default: return hipErrorInvalidValue;
  }
#undef LN_CASE
  return hipGetLastError();
}

// =============================================================================================
// weight conversion
// =============================================================================================
__global__ void f32_to_bf16_kernel(const float* __restrict__ in, bf16* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (bf16)in[i];
}
hipError_t launch_f32_to_bf16(const float* in, bf16* out, int64_t n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(1024), dim3(256), 0, st, in, out, n);
  return hipGetLastError();
}
__global__ void pad_rows_bf16_kernel(const float* __restrict__ in, bf16* __restrict__ out, int rows, int k, int kp) {
  const int64_t total = (int64_t)rows * kp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / kp), c = (int)(i % kp);
    out[i] = c < k ? (bf16)in[(size_t)r * k + c] : (bf16)0.f;
  }
}
hipError_t launch_pad_rows_bf16(const float* in, bf16* out, int rows, int k, int kp, hipStream_t st) {
  hipLaunchKernelGGL(pad_rows_bf16_kernel, dim3(1024), dim3(256), 0, st, in, out, rows, k, kp);
  return hipGetLastError();
}

}  // namespace clipx
