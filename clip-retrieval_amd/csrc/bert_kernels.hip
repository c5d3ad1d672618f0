// bert_kernels.hip -- gfx950 kernels of the multilingual text towers (use_mclip: DistilBERT multilingual, XLM-R): what a post-LN,
// padding-masked BERT encoder needs beyond the CLIP encoder's GEMMs and ragged attention (gemm_launch.hip, attn_block.hip):
//
//   bert_embed_ln_kernel   ids -> LN(word[id] + pos[pos_offset + t]) -> the fp16 residual stream (packed rows of a ragged batch)
//   postln_f16_kernel      the LayerNorm BEHIND a residual add, in place over the fp16 stream.  It cannot be folded into the next GEMM
//                          the way the CLIP towers' pre-LN is (fold_layernorm): its output is also the next residual.
//   bert_pool_proj_kernel  masked mean over a sample's rows -> dense [E, d] in fp32      } the sentence embedding
//   bert_norm_kernel       y / |y|  (|y| = 0 -> 1, the reference's `normalized`)         } (sentence-transformers Pooling + Dense)
//
// All three row kernels keep their statistics in fp32 and in two passes over registers, as layernorm_kernel / rowstats_kernel do: a
// lane holds 4 consecutive values per step of 256, an odd d / 128 ends in a half step of lanes 0 .. 31.  The mean is a true
// division by d: d copies of one fp16 value sum exactly in fp32 (d <= 2048 = 2^11 multiples of an 11-bit mantissa), and a
// correctly rounded s / d then gives the value back, so a row of equal elements centres to exact zeros for every d -- 1 / d is
// not a power of two at d = 768.  No kernel here uses scratch; the only LDS is stated at the launches below.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "bert_kernels.h"
#include "gemm_common.h"

namespace clipx {

// LayerNorm of one row held as v[NV][4] per lane (see above), written as IEEE fp16: 8-byte stores
template <int D128>
__device__ __forceinline__ void bert_ln_row_to_f16(float (&v)[(D128 + 1) / 2][4], float s, int lane, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, float eps, _Float16* __restrict__ out_row) {
  constexpr int d = D128 * 128, NV = (D128 + 1) / 2;
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s / (float)d;
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    if (D128 % 2 != 0 && e == D128 / 2 && lane >= 32) continue;  // the half step of an odd D128
#pragma unroll
    for (int j = 0; j < 4; ++j) v[e][j] -= mean;
    q += (v[e][0] * v[e][0] + v[e][1] * v[e][1]) + (v[e][2] * v[e][2] + v[e][3] * v[e][3]);
  }
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  const float rstd = 1.f / sqrtf(q / (float)d + eps);  // eps = 1e-12 and q = 0: 1e6, finite -- times the exact zeros it is 0
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    if (D128 % 2 != 0 && e == D128 / 2 && lane >= 32) continue;
    const int c4 = lane + 64 * e;
    const float4 g4 = reinterpret_cast<const float4*>(gamma)[c4];
    const float4 b4 = reinterpret_cast<const float4*>(beta)[c4];
    f16x4 oh;
    oh[0] = (_Float16)(v[e][0] * rstd * g4.x + b4.x);
    oh[1] = (_Float16)(v[e][1] * rstd * g4.y + b4.y);
    oh[2] = (_Float16)(v[e][2] * rstd * g4.z + b4.z);
    oh[3] = (_Float16)(v[e][3] * rstd * g4.w + b4.w);
    reinterpret_cast<f16x4*>(out_row)[c4] = oh;
  }
}

// grid (ceil(T / 4), S): workgroup (x, b) takes the tokens 4 x .. 4 x + 3 of sample b, one wave each
template <int D128>
__global__ __launch_bounds__(256) void bert_embed_ln_kernel(const int32_t* __restrict__ ids, int ids_stride, const int* __restrict__ src,
                                                           const int* __restrict__ offs, const int* __restrict__ lens, int rows,
                                                           const float* __restrict__ word, const float* __restrict__ pos, int pos_offset,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           _Float16* __restrict__ out, int vocab, float eps) {
  constexpr int d = D128 * 128, NV = (D128 + 1) / 2;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.y, t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= lens[b]) return;  // the mask: a position past the sample's length is never read
  const int row = offs[b] + t;
  if (row < 0 || row >= rows) return;
  const int s_ = src ? src[b] : b;
  int id = ids_stride > 0 ? ids[(size_t)s_ * ids_stride + t] : ids[offs[s_] + t];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float4* wr = reinterpret_cast<const float4*>(word + (size_t)id * d);
  const float4* pr = reinterpret_cast<const float4*>(pos + (size_t)(pos_offset + t) * d);
  float v[NV][4];
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    if (D128 % 2 != 0 && e == D128 / 2 && lane >= 32) continue;
    const float4 a = wr[lane + 64 * e], p = pr[lane + 64 * e];
    v[e][0] = a.x + p.x; v[e][1] = a.y + p.y; v[e][2] = a.z + p.z; v[e][3] = a.w + p.w;
    s += (v[e][0] + v[e][1]) + (v[e][2] + v[e][3]);
  }
  bert_ln_row_to_f16<D128>(v, s, lane, gamma, beta, eps, out + (size_t)row * d);
}

template <int D128>
__global__ __launch_bounds__(256) void postln_f16_kernel(_Float16* __restrict__ x16, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int M, float eps, int* __restrict__ range_flag) {
  constexpr int d = D128 * 128, NV = (D128 + 1) / 2;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  _Float16* xr = x16 + (size_t)row * d;
  float v[NV][4];
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    if (D128 % 2 != 0 && e == D128 / 2 && lane >= 32) continue;
    const f16x4 h = reinterpret_cast<const f16x4*>(xr)[lane + 64 * e];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[e][j] = (float)h[j];
    s += (v[e][0] + v[e][1]) + (v[e][2] + v[e][3]);
  }
  // every state of the stream passes through here: a row the residual epilogue rounded to inf has a non-finite sum (rowstats_kernel)
  float tot = s;
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
  if (range_flag && lane == 0 && !(fabsf(tot) <= 3.0e38f)) atomicOr(range_flag, 1);
  bert_ln_row_to_f16<D128>(v, s, lane, gamma, beta, eps, xr);  // a wave reads its whole row before it writes any of it
}

// grid (ceil(E / 64), B): the workgroup pools sample b's rows into p [d] (LDS; recomputed by each of the E / 64 workgroups of a
// sample, as tail_proj_kernel recomputes its LayerNorm) and produces 64 outputs, 4 threads per output over consecutive quarters of d
__global__ __launch_bounds__(256) void bert_pool_proj_kernel(const _Float16* __restrict__ x16, const int* __restrict__ offs,
                                                            const int* __restrict__ lens, const float* __restrict__ W,
                                                            const float* __restrict__ bias, float* __restrict__ y_raw, int d, int E) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* p = reinterpret_cast<float*>(smem);  // [d]
  const int b = blockIdx.y, tid = threadIdx.x;
  const int len = lens[b];
  const _Float16* xs = x16 + (size_t)offs[b] * d;
  for (int c = tid; c < d; c += 256) {
    float acc = 0.f;
    for (int t = 0; t < len; ++t) acc += (float)xs[(size_t)t * d + c];  // ascending t: one fixed order
    p[c] = len > 0 ? acc / (float)len : 0.f;
  }
  __syncthreads();
  const int e = blockIdx.x * 64 + (tid >> 2), part = tid & 3;
  const int seg = d >> 2;  // d % 32 == 0
  float acc = 0.f;
  if (e < E) {
    const float4* wr = reinterpret_cast<const float4*>(W + (size_t)e * d + part * seg);
    const float4* pp = reinterpret_cast<const float4*>(p + part * seg);
    for (int c4 = 0; c4 < seg / 4; ++c4) {
      const float4 w = wr[c4], y = pp[c4];
      acc = fmaf(y.x, w.x, acc); acc = fmaf(y.y, w.y, acc); acc = fmaf(y.z, w.z, acc); acc = fmaf(y.w, w.w, acc);
    }
  }
  acc += __shfl_xor(acc, 1);
  acc += __shfl_xor(acc, 2);
  if (part == 0 && e < E) y_raw[(size_t)b * E + e] = acc + (bias ? bias[e] : 0.f);
}

__global__ __launch_bounds__(256) void bert_norm_kernel(const float* __restrict__ y_raw, float* __restrict__ out_f32,
                                                       uint16_t* __restrict__ out_f16, int E) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  float ss = 0.f;
  for (int e = tid; e < E; e += 256) { const float v = y_raw[(size_t)b * E + e]; ss += v * v; }
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  float nrm = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
  if (nrm == 0.f) nrm = 1.f;  // mapper.py's `normalized`: a zero row stays zero
  for (int e = tid; e < E; e += 256) {
    const float v = y_raw[(size_t)b * E + e] / nrm;
    out_f32[(size_t)b * E + e] = v;
    if (out_f16) {
      const _Float16 hv = (_Float16)v;
      out_f16[(size_t)b * E + e] = __builtin_bit_cast(uint16_t, hv);
    }
  }
}

__global__ void f32_to_f16_kernel(const float* __restrict__ in, _Float16* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (_Float16)in[i];
}

#define BERT_D128_SWITCH(d, CASE)                                                                                  \
  switch (d) {                                                                                                     \
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13)      \
    CASE(14) CASE(15) CASE(16)                                                                                     \
    default: return hipErrorInvalidValue;                                                                          \
  }

hipError_t launch_bert_embed(const int32_t* ids, int ids_stride, const int* src, const int* offs, const int* lens, int S, int T, int rows,
                             const float* word, const float* pos, int pos_offset, const float* gamma, const float* beta, void* out_f16,
                             int d, int vocab, float eps, hipStream_t st) {
  if (S <= 0 || T <= 0 || rows <= 0) return hipSuccess;
  if (ids_stride < 0 || pos_offset < 0 || vocab <= 0) return hipErrorInvalidValue;
  const dim3 grid((T + 3) / 4, S), block(256);
  // LDS: none (one wave per row, statistics by cross-lane shuffles)
#define EMB_CASE(D128)                                                                                                          \
  case D128 * 128:                                                                                                              \
    hipLaunchKernelGGL(bert_embed_ln_kernel<D128>, grid, block, 0, st, ids, ids_stride, src, offs, lens, rows, word, pos, pos_offset, \
                       gamma, beta, reinterpret_cast<_Float16*>(out_f16), vocab, eps);                                          \
    break;
  BERT_D128_SWITCH(d, EMB_CASE)
#undef EMB_CASE
  return hipGetLastError();
}

hipError_t launch_postln_f16(void* x16, const float* gamma, const float* beta, int M, int d, float eps, int* range_flag, hipStream_t st) {
  if (M <= 0) return hipSuccess;
  const dim3 grid((M + 3) / 4), block(256);
  // LDS: none (one wave per row, statistics by cross-lane shuffles)
#define PLN_CASE(D128)                                                                                                            \
  case D128 * 128:                                                                                                                \
    hipLaunchKernelGGL(postln_f16_kernel<D128>, grid, block, 0, st, reinterpret_cast<_Float16*>(x16), gamma, beta, M, eps, range_flag); \
    break;
  BERT_D128_SWITCH(d, PLN_CASE)
#undef PLN_CASE
  return hipGetLastError();
}

hipError_t launch_bert_pool(const void* x16, const int* offs, const int* lens, const float* W, const float* bias_or_null, float* y_raw,
                            float* out_f32, uint16_t* out_f16_or_null, int B, int d, int E, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (d <= 0 || d % 32 != 0 || d > 2048 || E <= 0 || !y_raw || !out_f32) return hipErrorInvalidValue;
  // LDS: d floats of dynamic memory (the pooled row; at most 8 KiB), nothing static
  hipLaunchKernelGGL(bert_pool_proj_kernel, dim3((E + 63) / 64, B), dim3(256), (size_t)d * sizeof(float), st,
                     reinterpret_cast<const _Float16*>(x16), offs, lens, W, bias_or_null, y_raw, d, E);
  // LDS: 16 bytes static (the four wave sums of |y|^2)
  hipLaunchKernelGGL(bert_norm_kernel, dim3(B), dim3(256), 0, st, y_raw, out_f32, out_f16_or_null, E);
  return hipGetLastError();
}

hipError_t launch_f32_to_f16(const float* in, void* out_f16, int64_t n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(f32_to_f16_kernel, dim3(1024), dim3(256), 0, st, in, reinterpret_cast<_Float16*>(out_f16), n);
  return hipGetLastError();
}

}  // namespace clipx
