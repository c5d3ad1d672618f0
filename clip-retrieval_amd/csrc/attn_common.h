// attn_common.h -- what the three attention kernel files (attn_block.hip, attn_pk9.hip, attn_long.hip) share: the operand type of
// the two products and the launchers launch_attention (attn_block.hip) dispatches to.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "clip_kernels.h"
#include "gemm_common.h"  // the vector typedefs
#include "clipx_attn_plan.h"

namespace clipx {

// Operand type of the attention products (round 4): q, k, v arrive as IEEE fp16 (the QKV projection's EPI_BIAS_F16 epilogue) and
// the probabilities P are rounded to fp16 as well: v_mfma_f32_32x32x16_f16 issues at the rate of the bf16 form, and the three extra
// mantissa bits of q and k are worth an order of magnitude in the embedding's error where LayerNorm gains are large (the
// logits q.k are where the bf16 rounding hurt most: tools/emulate_fp16_stream.py).  The 16-bit values keep travelling
// through `bf16`-typed pointers and fragments: every load, LDS staging step and transposition moves bits.
__device__ __forceinline__ f32x16 attn_mfma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ unsigned attn_pack_p(float p0, float p1) {  // one v_cvt_pk_f16_f32 (round to nearest even)
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){p0, p1}, f16x2_t));
}

// attn_pk9.hip: the persistent kernel of (dh 64, not causal, 9 key blocks); plan_lds = the bytes clipx_attn_plan.h names for it
hipError_t launch_attention_pk9(const bf16* qkv, bf16* out, int B, int T, int H, hipStream_t st, int q_blocks, size_t plan_lds);
// attn_long.hip: 10 .. 19 key blocks (dh 64, not causal)
hipError_t launch_attention_long(const bf16* qkv, bf16* out, int B, int T, int H, hipStream_t st, int q_blocks, const AttnPlan& plan);

}  // namespace clipx
