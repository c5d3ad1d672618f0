// bert_kernels.h -- launchers of the post-LN / mask-shaped kernels of the multilingual text towers (internal; public ABI:
// include/clipx.h, clipx_bert_*).  The GEMMs and the ragged attention are the CLIP encoder's own (clip_kernels.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace clipx {

// Embedding + LayerNorm of a ragged batch: sample b owns the packed rows offs[b] .. offs[b] + lens[b] - 1 of out (IEEE fp16
// [rows, d]); row offs[b] + t = LN(word[id] + pos[pos_offset + t]) gamma + beta, id = the t-th id of sample s = src ? src[b] : b:
// ids[s * ids_stride + t] (ids_stride > 0: rectangular ids, only the first lens[b] of a row are read) or ids[offs[s] + t]
// (ids_stride == 0: packed ids).  An id outside [0, vocab) is clamped into it (launch_text_embed).  fp32 two-pass statistics, one
// wave per row; d % 128 == 0, d <= 2048; T = the longest length of the batch; a row at or past `rows` is not written.
hipError_t launch_bert_embed(const int32_t* ids, int ids_stride, const int* src, const int* offs, const int* lens, int S, int T, int rows,
                             const float* word, const float* pos, int pos_offset, const float* gamma, const float* beta, void* out_f16,
                             int d, int vocab, float eps, hipStream_t st);

// x16[m, :] = fp16(LN(f32(x16[m, :])) gamma + beta) in place over the fp16 residual stream, fp32 two-pass statistics, one wave per
// row; d % 128 == 0, d <= 2048.  A row of equal elements gives exactly fp16(beta).  range_flag (may be null) is raised when a row
// holds inf / NaN (the CLIP encoder's range guard: rowstats_kernel).
hipError_t launch_postln_f16(void* x16, const float* gamma, const float* beta, int M, int d, float eps, int* range_flag, hipStream_t st);

// Sample b: p = mean of its lens[b] rows of x16 (fp32, rows added in ascending order), y = W p (+ bias), W f32 [E, d];
// y_raw f32 [B, E] receives y, out_f32 [B, E] = y / |y| (|y| = 0 -> 1), out_f16 (may be null) its IEEE fp16 rounding.  d % 32 == 0.
hipError_t launch_bert_pool(const void* x16, const int* offs, const int* lens, const float* W, const float* bias_or_null, float* y_raw,
                            float* out_f32, uint16_t* out_f16_or_null, int B, int d, int E, hipStream_t st);

// weights of the fp16-operand GEMMs (QKV, fc1): IEEE fp16 rounding of the f32 matrix
hipError_t launch_f32_to_f16(const float* in, void* out_f16, int64_t n, hipStream_t st);

}  // namespace clipx
