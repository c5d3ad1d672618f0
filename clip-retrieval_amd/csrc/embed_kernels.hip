// embed_kernels.hip -- what turns the inputs of the two towers into rows: im2col (pixels -> patch rows for the conv1 GEMM) and the
// text embedding gather (reference clip_retrieval/clip_inference/mapper.py:57,65: the first ops of encode_image / encode_text).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "clip_kernels.h"
#include "gemm_common.h"  // the vector typedefs

namespace clipx {

// =============================================================================================
// im2col: pixels -> bf16 patch rows (+ the all-zero class-token row), 8 k per thread (16-B stores)
// =============================================================================================
template <int FMT>
__global__ __launch_bounds__(256) void im2col_kernel(const void* __restrict__ pixels, int B, int S, int P, int Kp,
                                                    float m0, float m1, float m2, float i0, float i1, float i2,
                                                    bf16* __restrict__ out) {
  const int gdim = S / P, T = gdim * gdim + 1, PP = P * P, K = 3 * PP, nch = Kp / 8;
  const int64_t total = (int64_t)B * T * nch;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(idx % nch);
    const int64_t row = idx / nch;
    const int t = (int)(row % T), b = (int)(row / T);
    bf16x8 o;
    // the eight loads are unconditional (coordinates clamped, the value discarded afterwards): behind a per-element
    // `if (t > 0 && k < K)` hipcc put every load in its own branch with an s_waitcnt vmcnt(0) -- eight serialised round trips
    const int tp = t > 0 ? t - 1 : 0;
    const int py = tp / gdim, px = tp - py * gdim;
    float raw[8];
    int cc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = ch * 8 + e;
      const int kk = k < K ? k : K - 1;
      const int c = kk / PP, rem = kk - c * PP;
      const int iy = rem / P, ix = rem - iy * P;
      const int yy = py * P + iy, xx = px * P + ix;
      cc[e] = c;
      if (FMT == 0) raw[e] = reinterpret_cast<const float*>(pixels)[(((size_t)b * 3 + c) * S + yy) * S + xx];
      else raw[e] = (float)reinterpret_cast<const unsigned char*>(pixels)[(((size_t)b * S + yy) * S + xx) * 3 + c];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = raw[e];
      if (FMT != 0) {
        const int c = cc[e];
        // torchvision's arithmetic, operation for operation (ToTensor: x / 255; Normalize: (x - mean) / std, IEEE f32 divisions):
        // the f32 value is the reference reader's `image_tensor` element bit for bit (pinned against the reference-held
        // tests/test_clip_inference/test_tensors/*.pkl), so raw uint8 pixels and the reader's f32 tensor give the same patches
        const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? i0 : (c == 1 ? i1 : i2);
        v = __fdiv_rn(__fsub_rn(__fdiv_rn(v, 255.f), mean), sd);
      }
      o[e] = (t > 0 && ch * 8 + e < K) ? (bf16)v : (bf16)0.f;
    }
    *reinterpret_cast<bf16x8*>(out + (size_t)row * Kp + ch * 8) = o;
  }
}

hipError_t launch_im2col(const void* pixels, int fmt, int B, int S, int P, int Kp, const float* mean,
                         const float* stdv, bf16* out, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  const int gdim = S / P, T = gdim * gdim + 1;
  const int64_t total = (int64_t)B * T * (Kp / 8);
  const int blocks = (int)((total + 255) / 256 < 65536 * 4 ? (total + 255) / 256 : 65536 * 4);
  if (fmt == 0)
    hipLaunchKernelGGL(im2col_kernel<0>, dim3(blocks), dim3(256), 0, st, pixels, B, S, P, Kp, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f, out);
  else
    hipLaunchKernelGGL(im2col_kernel<1>, dim3(blocks), dim3(256), 0, st, pixels, B, S, P, Kp, mean[0], mean[1], mean[2],
                       stdv[0], stdv[1], stdv[2], out);
  return hipGetLastError();
}

// =============================================================================================
// text embedding gather
// =============================================================================================
__global__ __launch_bounds__(256) void text_embed_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok,
                                                        const float* __restrict__ pos, float* __restrict__ x, int BT,
                                                        int T, int d, int vocab, void* __restrict__ x16, int x16_f16,
                                                        const int* __restrict__ rowmap) {
  const int d4 = d / 4;
  const int64_t total = (int64_t)BT * d4;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % d4);
    const int row = (int)(idx / d4);
    const int src = rowmap ? rowmap[row] : row;  // ragged: output row `row` is token src = b T + t of the rectangular batch
    int id = ids[src];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const float4 a = reinterpret_cast<const float4*>(tok + (size_t)id * d)[c];
    const float4 p = reinterpret_cast<const float4*>(pos + (size_t)(src % T) * d)[c];
    const float4 o = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
    if (x) reinterpret_cast<float4*>(x + (size_t)row * d)[c] = o;
    if (x16 && x16_f16) {
      f16x4 h;
      h[0] = (_Float16)o.x; h[1] = (_Float16)o.y; h[2] = (_Float16)o.z; h[3] = (_Float16)o.w;
      reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(x16) + (size_t)row * d)[c] = h;
    } else if (x16) {
      bf16x4 h;
      h[0] = (bf16)o.x; h[1] = (bf16)o.y; h[2] = (bf16)o.z; h[3] = (bf16)o.w;
      reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(x16) + (size_t)row * d)[c] = h;
    }
  }
}

hipError_t launch_text_embed(const int32_t* ids, const float* tok_emb, const float* pos_emb, float* x, int B, int T, int d,
                             int vocab, hipStream_t st, void* x16, int x16_f16, const int* rowmap, int nrows) {
  if (B <= 0) return hipSuccess;
  const int rows = rowmap ? nrows : B * T;
  if (rows <= 0) return hipSuccess;
  const int64_t total = (int64_t)rows * (d / 4);
  const int blocks = (int)((total + 255) / 256);
  hipLaunchKernelGGL(text_embed_kernel, dim3(blocks), dim3(256), 0, st, ids, tok_emb, pos_emb, x, rows, T, d, vocab, x16, x16_f16, rowmap);
  return hipGetLastError();
}

}  // namespace clipx
