// clip_kernels.h -- launchers of the gfx950 CLIP encoder kernels (internal; public ABI: include/clipx.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "clipx_gemm_plan.h"  // GemmEpilogue, GemmVariant, the gemm256_* planner functions
#include "clipx_stamp_slots.h"

namespace clipx {

typedef __bf16 bf16;

// In-kernel timing (the GEMM brackets of clipx_profile_enable, clipx_encode.hip ProfScope): every kernel launch_gemm can issue takes
// a StampSlot* as its last argument (clipx_stamp_slots.h; null = not profiled, the kernel does nothing more than test it) and
// writes its own first start and last end into it.  The dispatch carries nothing: no event, no completion signal, no marker.
// LaunchEvents is where the slots of one launch_gemm call come from, one per kernel.
struct LaunchEvents {
  void* ctx;
  StampSlot* (*next)(void* ctx);  // a filled slot on the device, or null when none is to be had (the kernel then runs unstamped)
};

// hipLaunchKernelGGL with the next slot of `le` (null when le is) appended to the arguments
template <class K, class... Args>
inline void launch_with_events(LaunchEvents* le, K kern, const dim3& grid, const dim3& block, size_t smem, hipStream_t st, Args... args) {
  StampSlot* slot = le ? le->next(le->ctx) : nullptr;
  hipLaunchKernelGGL(kern, grid, block, smem, st, args..., slot);
}

struct GemmArgs {
  const bf16* A;      // activations [M, K] row-major
  const bf16* W;      // weights     [N, K] row-major (torch Linear layout)
  const float* bias;  // [N] or null
  void* out;          // [M, N] bf16 or f32
  const float* table; // [T, N] (EPI_TABLE_F32)
  int T;
  int M, N, K;        // N % 128 == 0, K % 64 == 0
  int epi;
  int variant;        // GemmVariant (clipx_gemm_plan.h): GEMM_V_DEFAULT = whole 256-row m-tiles in the 4-wave 256x256 kernel where it
                      // has the form, the 8-wave one elsewhere, the 128x128 kernel for the rest; 0 / 1 / 3: the forms the tests compare
  int n_cu;           // compute units of the device (the persistent kernels launch one workgroup per CU); 0 = 256
  int row0;           // EPI_TABLE_F32: table row = (row0 + m) % T (set by the launcher when it splits M)
  const float* rowscale;  // bf16-output epilogues: out = act(acc * rowscale[m] + bias[n]); [M] f32, never null (the LayerNorm
                          // 1/std of the row when the LayerNorm is folded into W, launch_rowstats; ones otherwise)
  bf16* out16;            // EPI_BIAS_RESID_F32: also store the new x row as bf16 here (null: do not)
  float* splitk_ws;       // device scratch for split-K partial products (null: never split), splitk_ws_bytes of it
  size_t splitk_ws_bytes;
  int tail_m0, tail_nb;   // set by launch_gemm (from its GemmPlan) for the persistent kernel: rows [tail_m0, tail_m0 + 256) beyond the whole
                          // m-tiles are computed inside the same launch, 32 x (tail_nb x 32) per workgroup (0: none)
  int f16;                // A and W hold IEEE fp16 instead of bf16 (v_mfma_f32_32x32x16_f16, same rate): the LayerNorm-folded
                          // GEMMs, whose A operand is the fp16 residual stream itself.  bf16-output epilogues (0..2) and RAW only.
  float stats_eps;        // > 0 (f16, 16-bit-output epilogues, K = the row length): the GEMM is LayerNorm-folded and rowscale is NOT an
                          // input -- it is the [M] buffer that receives 1 / sqrt(var(A[m, :]) + stats_eps) where a separate pass has to
                          // compute it (launch_gemm runs launch_rowstats on those rows); the rows the 4-wave 256x256 kernel takes get
                          // their statistics from the A fragments inside its K loop instead (gemm256w4.hip, STATS) and are not written
  int* range_flag;        // (stats_eps > 0) raised when a row of A holds inf / NaN (launch_rowstats)
  LaunchEvents* events;   // null, or the source of one stamp slot for every kernel this GEMM launches
};

hipError_t launch_gemm(const GemmArgs& g, hipStream_t st);

// x f32 [M, d] -> y [M, d]; out_kind 0: f32, 1: bf16, 2: IEEE fp16 (ln_pre of the vision tower writes the fp16 residual
// stream); one wave per row; d % 128 == 0, d <= 2048.  y16 (f32 output only, may be null): also the bf16 rounding of y
hipError_t launch_layernorm(const float* x, const float* gamma, const float* beta, void* y, int out_kind, int M,
                            int d, float eps, hipStream_t st, bf16* y16 = nullptr);

// LayerNorm statistics of the 16-bit residual stream rows (f16 != 0: IEEE fp16, else bf16): rstd[m] = 1 / sqrt(var(x16[m, :]) + eps)
// (two-pass, fp32; or, for fp16 rows on request, ONE pass in the canonical order of gemm_common.h ln_rstd_onepass -- the order the
// 4-wave GEMM kernel accumulates the same sums in from its A fragments, so that a row's rstd does not depend on which of the two
// computed it: the CLIPX_LN_FUSED=1 experiment of round 6).  The LayerNorm itself is folded into the GEMM that follows (weights scaled by gamma and row-centred, bias
// absorbs beta: clipx_api.hip carve_layers), whose epilogue multiplies by rstd[m].  One wave per row.
// canonical != 0 (fp16 rows): the one-pass form of a GEMM that owns its statistics (GemmArgs.stats_eps)
hipError_t launch_rowstats(const void* x16, float* rstd, int M, int d, float eps, hipStream_t st, int f16 = 0, int* range_flag = nullptr,
                           int canonical = 0, LaunchEvents* events = nullptr);

// LayerNorm-folded weights: Wf[n, k] = r16(W[n,k] gamma[k] - mean_k(W[n,:] gamma)), cf[n] = bias[n] + sum_k beta[k] W[n,k];
// r16 = bf16 rounding, or IEEE fp16 when f16 != 0
hipError_t launch_fold_layernorm(const float* W, const float* gamma, const float* beta, const float* bias, bf16* Wf, float* cf,
                                 int N, int K, hipStream_t st, int f16 = 0);
hipError_t launch_fill_f32(float* p, float v, int64_t n, hipStream_t st);
// every entry of n stamp slots <- {~0, 0} (clipx_stamp_slots.h: a slot is handed out filled)
hipError_t launch_fill_stamps(StampSlot* slots, int64_t n, hipStream_t st);

// pixels -> bf16 patch matrix [B*T, Kp] (row b*T is the all-zero class-token row; k = c*P*P + iy*P + ix)
// fmt 0: f32 NCHW already normalised (the reference's `image_tensor`); fmt 1: u8 NHWC, normalised here
hipError_t launch_im2col(const void* pixels, int fmt, int B, int S, int P, int Kp, const float* mean,
                         const float* stdv, bf16* out, hipStream_t st);

// qkv bf16 [B*T, 3*H*dh] -> out bf16 [B*T, H*dh]; softmax(q k^T / sqrt(dh) [+ causal]) v, head dim dh = 64, 80, 88 or 104 (88 / 104: not causal, T <= 96 or 257 .. 288)
// q_blocks > 0: only the first q_blocks 32-row query blocks are computed (rows past them are left untouched); 0 = all
// offs / lens (both or neither; head dim 64, T <= 128): ragged batch -- sample b owns rows offs[b] .. offs[b] + lens[b] - 1
hipError_t launch_attention(const bf16* qkv, bf16* out, int B, int T, int H, int dh, int causal, hipStream_t st, int q_blocks = 0,
                            const int* offs = nullptr, const int* lens = nullptr);

// ids int32 [B, T] -> tok_emb[id] + pos_emb[t] as x f32 [B*T, d] (may be null) and / or x16 [B*T, d] (may be null; bf16, or
// IEEE fp16 when x16_f16 != 0: the text tower's residual stream)
hipError_t launch_text_embed(const int32_t* ids, const float* tok_emb, const float* pos_emb, float* x, int B, int T,
                             int d, int vocab, hipStream_t st, void* x16 = nullptr, int x16_f16 = 0, const int* rowmap = nullptr,
                             int nrows = 0);

// pooled row (CLS, or argmax(ids) for text) -> LayerNorm -> @ proj^T [E, d] -> / L2 norm -> fp16 [B, E]
// x: the residual stream, f32 [B*T, d] or (x_f16 != 0) IEEE fp16
// scratch: B * E floats of device memory (the un-normalised projection between the two kernels)
// sb: samples per workgroup of the projection kernel -- -1: chosen by B (per-sample kernel for small batches, batched above),
// 0: the per-sample kernel, 8 / 16: the batched kernel.  Every choice writes the same bytes.
// pooled rows (token 0, or the EOT token of `ids`) of att [B*T, d] bf16 and x16 [B*T, d] fp16 -> attc / xc [B, d]
hipError_t launch_gather_pooled(const bf16* att, const void* x16, const int32_t* ids_or_null, bf16* attc, void* xc, int B, int T,
                                int d, hipStream_t st, const int* rows_or_null = nullptr);
// (an `sb` the batched kernel cannot serve -- not 0 / 8 / 16, or more LDS than a workgroup may have -- is hipErrorInvalidValue,
// never a silent fall-back to the per-sample kernel; tail_batched_rows tells what -1 picks)
int tail_batched_rows(int B, int d, int E);
hipError_t launch_tail(const void* x, const int32_t* ids_or_null, const float* gamma, const float* beta,
                       const bf16* proj, uint16_t* out_f16, float* out_f32_or_null, float* scratch, int B, int T, int d,
                       int E, float eps, hipStream_t st, int x_f16 = 0, int* range_flag = nullptr, int sb = -1);

hipError_t launch_f32_to_bf16(const float* in, bf16* out, int64_t n, hipStream_t st);
// conv weight [width, 3*P*P] f32 -> bf16 [width, Kp] zero padded
hipError_t launch_pad_rows_bf16(const float* in, bf16* out, int rows, int k, int kp, hipStream_t st);

}  // namespace clipx
