// tail_kernels.hip -- the end of both towers: pooled row -> LayerNorm -> projection -> L2 normalise -> fp16, and the gather of the
// pooled rows in front of the last block.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "clip_kernels.h"
#include "gemm_common.h"  // the vector typedefs

namespace clipx {

// =============================================================================================
// tail: pool -> LayerNorm -> projection -> L2 normalise -> fp16   (mapper.py:58-59, 66-67)
// =============================================================================================
__device__ __forceinline__ float block_sum_256(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// One pooled row (x[xrow ..], f32 or IEEE fp16) into y [d] (LDS) and its LayerNorm in place, by the 256 threads of a workgroup: one
// body for both projection kernels below, so that a row's y does not depend on which of them computed it.  A thread normalises
// the elements it loaded itself (c = tid, tid + 256, ...): no barrier between the two, and none after the last loop (the caller's).
__device__ __forceinline__ void tail_load_row(const void* __restrict__ x, size_t xrow, float* __restrict__ y, int d, int x_f16) {
  for (int c = threadIdx.x; c < d; c += 256)
    y[c] = x_f16 ? (float)reinterpret_cast<const _Float16*>(x)[xrow + c] : reinterpret_cast<const float*>(x)[xrow + c];
}
__device__ __forceinline__ void tail_layernorm_row(float* __restrict__ y, int d, float eps, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, float* red, int* __restrict__ range_flag) {
  const int tid = threadIdx.x;
  float s = 0.f;
  for (int c = tid; c < d; c += 256) s += y[c];
  const float tot = block_sum_256(s, red);
  if (range_flag && tid == 0 && !(fabsf(tot) <= 3.0e38f)) atomicOr(range_flag, 1);  // the last state of the fp16 stream (rowstats_kernel)
  const float mean = tot / d;
  float q = 0.f;
  for (int c = tid; c < d; c += 256) { const float a = y[c] - mean; q += a * a; }
  const float rstd = 1.f / sqrtf(block_sum_256(q, red) / d + eps);
  for (int c = tid; c < d; c += 256) y[c] = (y[c] - mean) * rstd * gamma[c] + beta[c];
}

// One term of a projection output: acc + y * w with the product ROUNDED before the add.  That is what the projection loop has
// always compiled to (packed multiplies, then a chain of adds), and the embeddings are compared bit for bit across builds and
// across the two projection kernels below, so the choice is pinned here instead of being left to the contraction heuristics.
__device__ __forceinline__ float tail_mul_add(float y, float w, float acc) {
#pragma clang fp contract(off)
  const float p = y * w;
  return acc + p;
}

// Two launches: (E / 64, B) workgroups each LayerNorm the sample's pooled row (recomputed per workgroup: d floats) and
// produce 64 projection outputs with 4 threads per output; a second kernel normalises.  (One workgroup per sample doing the
// whole d x E projection took 79 us -- 3 % of a B = 1 image query, 8 % of a text query.)
__global__ __launch_bounds__(256) void tail_proj_kernel(const void* __restrict__ x, const int32_t* __restrict__ ids,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const bf16* __restrict__ proj, float* __restrict__ o_raw, int T, int d,
                                                       int E, float eps, int x_f16, int* __restrict__ range_flag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* y = reinterpret_cast<float*>(smem);  // [d]
  float* red = y + d;                         // [4]   (all LDS in the one dynamic region: guide G17)
  int* s_posp = reinterpret_cast<int*>(red + 4);
  const int b = blockIdx.y, tid = threadIdx.x;
  if (tid == 0) {
    int best = 0;
    if (ids) {  // EOT token = highest id; first occurrence (torch.argmax semantics of the reference model)
      int bv = ids[(size_t)b * T];
      for (int t = 1; t < T; ++t) {
        const int v = ids[(size_t)b * T + t];
        if (v > bv) { bv = v; best = t; }
      }
    }
    *s_posp = best;
  }
  __syncthreads();
  tail_load_row(x, ((size_t)b * T + *s_posp) * d, y, d, x_f16);
  tail_layernorm_row(y, d, eps, gamma, beta, red, range_flag);
  __syncthreads();
  const int e = blockIdx.x * 64 + (tid >> 2), part = tid & 3;
  const int seg = d >> 2;  // d % 32 == 0
  float acc = 0.f;
  if (e < E) {
    const bf16x8* pr = reinterpret_cast<const bf16x8*>(proj + (size_t)e * d + part * seg);
    const float* yp = y + part * seg;
    for (int c8 = 0; c8 < seg / 8; ++c8) {
      const bf16x8 pw = pr[c8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = tail_mul_add(yp[c8 * 8 + j], (float)pw[j], acc);
    }
  }
  acc += __shfl_xor(acc, 1);
  acc += __shfl_xor(acc, 2);
  if (part == 0 && e < E) o_raw[(size_t)b * E + e] = acc;
}

// The same projection for a batch: one workgroup takes 64 outputs x SB samples.  tail_proj_kernel's (E / 64, B) grid is laid out
// for the latency of a B = 1 query; at B = 256 every one of its workgroups pulls its own 64 x d slice of the projection matrix
// through the L2 (12 x 256 x 128 KiB = 400 MB per call at ViT-L/14) and recomputes the sample's LayerNorm.  Here a workgroup
// LayerNorms its SB pooled rows into the LDS -- row by row with tail_proj_kernel's own code, the same strided loops and the
// same block_sum_256 reduction order -- and then walks its slice of the matrix once: each 16-byte weight load is applied to
// all SB rows.  Per output the arithmetic is tail_proj_kernel's: four partial sums over consecutive quarters of d, each
// accumulated in ascending c by tail_mul_add, combined as (p0 + p1) + (p2 + p3): the two kernels write the same bytes
// (tests/test_tail_batched_gpu.py).
template <int SB>
__global__ __launch_bounds__(256) void tail_proj_batched_kernel(const void* __restrict__ x, const int32_t* __restrict__ ids,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const bf16* __restrict__ proj, float* __restrict__ o_raw, int B, int T,
                                                               int d, int E, float eps, int x_f16, int* __restrict__ range_flag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* ys = reinterpret_cast<float*>(smem);  // [SB][d]
  float* red = ys + (size_t)SB * d;            // [4]
  int* s_pos = reinterpret_cast<int*>(red + 4);  // [SB]
  const int b0 = blockIdx.y * SB, tid = threadIdx.x;
  const int nb = B - b0 < SB ? B - b0 : SB;  // samples of this workgroup (the last one may be short)
  if (tid < nb) {
    int best = 0;
    if (ids) {  // EOT token = highest id; first occurrence (tail_proj_kernel)
      const int32_t* row = ids + (size_t)(b0 + tid) * T;
      int bv = row[0];
      for (int t = 1; t < T; ++t) {
        const int v = row[t];
        if (v > bv) { bv = v; best = t; }
      }
    }
    s_pos[tid] = best;
  }
  __syncthreads();
  for (int sb = 0; sb < nb; ++sb)  // every row's loads are in flight before the first reduction waits for one
    tail_load_row(x, ((size_t)(b0 + sb) * T + s_pos[sb]) * d, ys + (size_t)sb * d, d, x_f16);
  for (int sb = 0; sb < nb; ++sb)  // (nb is uniform over the workgroup: the barriers inside block_sum_256 are safe)
    tail_layernorm_row(ys + (size_t)sb * d, d, eps, gamma, beta, red, range_flag);
  for (int sb = nb; sb < SB; ++sb)  // rows past the batch: finite operands for the accumulators below (never stored)
    for (int c = tid; c < d; c += 256) ys[(size_t)sb * d + c] = 0.f;
  __syncthreads();
  const int e = blockIdx.x * 64 + (tid >> 2), part = tid & 3;
  const int seg = d >> 2;  // d % 32 == 0
  float acc[SB];
#pragma unroll
  for (int sb = 0; sb < SB; ++sb) acc[sb] = 0.f;
  if (e < E) {
    const bf16x8* pr = reinterpret_cast<const bf16x8*>(proj + (size_t)e * d + part * seg);
    const float* yp = ys + part * seg;
    for (int c8 = 0; c8 < seg / 8; ++c8) {
      const bf16x8 pw = pr[c8];
      float wf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) wf[j] = (float)pw[j];
#pragma unroll
      for (int sb = 0; sb < SB; ++sb) {
        const float4 y0 = *reinterpret_cast<const float4*>(yp + (size_t)sb * d + c8 * 8);
        const float4 y1 = *reinterpret_cast<const float4*>(yp + (size_t)sb * d + c8 * 8 + 4);
        float a = acc[sb];
        a = tail_mul_add(y0.x, wf[0], a); a = tail_mul_add(y0.y, wf[1], a);
        a = tail_mul_add(y0.z, wf[2], a); a = tail_mul_add(y0.w, wf[3], a);
        a = tail_mul_add(y1.x, wf[4], a); a = tail_mul_add(y1.y, wf[5], a);
        a = tail_mul_add(y1.z, wf[6], a); a = tail_mul_add(y1.w, wf[7], a);
        acc[sb] = a;
      }
    }
  }
#pragma unroll
  for (int sb = 0; sb < SB; ++sb) {
    float a = acc[sb];
    a += __shfl_xor(a, 1);
    a += __shfl_xor(a, 2);
    if (part == 0 && e < E && sb < nb) o_raw[(size_t)(b0 + sb) * E + e] = a;
  }
}

__global__ __launch_bounds__(256) void tail_norm_kernel(const float* __restrict__ o_raw, uint16_t* __restrict__ out_f16,
                                                       float* __restrict__ out_f32, int E) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  float ss = 0.f;
  for (int e = tid; e < E; e += 256) { const float v = o_raw[(size_t)b * E + e]; ss += v * v; }
  const float nrm = sqrtf(block_sum_256(ss, red));
  for (int e = tid; e < E; e += 256) {
    const float v = o_raw[(size_t)b * E + e] / nrm;  // no epsilon: mapper.py:58 divides by the raw norm
    const _Float16 hv = (_Float16)v;
    out_f16[(size_t)b * E + e] = *reinterpret_cast<const uint16_t*>(&hv);
    if (out_f32) out_f32[(size_t)b * E + e] = v;
  }
}

// The rows the embedding is read from -- token 0 of every image, the EOT token (highest id, first occurrence) of every caption --
// copied out of the [B * T, d] attention output and residual stream into two compact [B, d] buffers: the last block's
// out-proj / MLP then run on B rows instead of B * T (nothing else of that block's output is ever read).
__global__ __launch_bounds__(256) void gather_pooled_kernel(const bf16* __restrict__ att, const _Float16* __restrict__ x,
                                                           const int32_t* __restrict__ ids, bf16* __restrict__ attc,
                                                           _Float16* __restrict__ xc, int T, int d, const int* __restrict__ rows) {
  __shared__ int s_pos;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    int best = 0;
    if (ids && !rows) {
      int bv = ids[(size_t)b * T];
      for (int t = 1; t < T; ++t) {
        const int v = ids[(size_t)b * T + t];
        if (v > bv) { bv = v; best = t; }
      }
    }
    s_pos = best;
  }
  __syncthreads();
  const size_t row = rows ? (size_t)rows[b] : (size_t)b * T + s_pos;  // ragged batches bring the pooled row of every sample
  const uint4* a = reinterpret_cast<const uint4*>(att + row * d);
  const uint4* xs = reinterpret_cast<const uint4*>(x + row * d);
  uint4* ao = reinterpret_cast<uint4*>(attc + (size_t)b * d);
  uint4* xo = reinterpret_cast<uint4*>(xc + (size_t)b * d);
  for (int c = tid; c < d / 8; c += 256) {
    ao[c] = a[c];
    xo[c] = xs[c];
  }
}

hipError_t launch_gather_pooled(const bf16* att, const void* x16, const int32_t* ids_or_null, bf16* attc, void* xc, int B, int T,
                                int d, hipStream_t st, const int* rows_or_null) {
  if (B <= 0) return hipSuccess;
  if (d % 8 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gather_pooled_kernel, dim3(B), dim3(256), 0, st, att, reinterpret_cast<const _Float16*>(x16), ids_or_null, attc,
                     reinterpret_cast<_Float16*>(xc), T, d, rows_or_null);
  return hipGetLastError();
}

// Which projection kernel: the batched one, TAIL_SB samples per workgroup, from B * d * E = TAIL_BATCHED_MIN_WORK multiply-adds on;
// the per-sample one, whose latency is that of a single sample, below (measured: DESIGN 4.7).
constexpr int64_t TAIL_BATCHED_MIN_WORK = (int64_t)1 << 26;
constexpr int TAIL_SB = 8;

static size_t tail_batched_lds(int sb, int d) { return ((size_t)sb * d + 4 + sb) * sizeof(float); }
constexpr size_t TAIL_LDS_MAX = (size_t)128 << 10;
// samples per workgroup launch_tail picks by itself: TAIL_SB, or 0 = the per-sample kernel (small batches; a model so wide that
// TAIL_SB LayerNormed rows do not fit the LDS)
int tail_batched_rows(int B, int d, int E) {
  return (int64_t)B * d * E >= TAIL_BATCHED_MIN_WORK && tail_batched_lds(TAIL_SB, d) <= TAIL_LDS_MAX ? TAIL_SB : 0;
}

hipError_t launch_tail(const void* x, const int32_t* ids_or_null, const float* gamma, const float* beta, const bf16* proj,
                       uint16_t* out_f16, float* out_f32_or_null, float* scratch, int B, int T, int d, int E, float eps,
                       hipStream_t st, int x_f16, int* range_flag, int sb) {
  if (B <= 0) return hipSuccess;
  if (d % 32 != 0 || !scratch) return hipErrorInvalidValue;
  if (sb < 0) sb = tail_batched_rows(B, d, E);
  if (sb != 0 && sb != 8 && sb != 16) return hipErrorInvalidValue;
  const size_t smem_b = tail_batched_lds(sb, d);
  if (sb && smem_b > TAIL_LDS_MAX) return hipErrorInvalidValue;
  if (sb) {
    auto kern = sb == 8 ? tail_proj_batched_kernel<8> : tail_proj_batched_kernel<16>;
    if (smem_b > ((size_t)48 << 10)) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_b);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((E + 63) / 64, (B + sb - 1) / sb), dim3(256), smem_b, st, x, ids_or_null, gamma, beta, proj, scratch,
                       B, T, d, E, eps, x_f16, range_flag);
  } else {
    const size_t smem = (size_t)(d + 8) * sizeof(float);
    hipLaunchKernelGGL(tail_proj_kernel, dim3((E + 63) / 64, B), dim3(256), smem, st, x, ids_or_null, gamma, beta, proj, scratch,
                       T, d, E, eps, x_f16, range_flag);
  }
  hipLaunchKernelGGL(tail_norm_kernel, dim3(B), dim3(256), 0, st, scratch, out_f16, out_f32_or_null, E);
  return hipGetLastError();
}

}  // namespace clipx
