// clipx_hooks.hip -- the per-kernel entry points of include/clipx.h that only parity tests and tools call: one GEMM, one
// attention, one LayerNorm / row statistics / projection tail launch each, on the caller's buffers.  No handle, no state beyond
// gemm_hook's per-device vector of ones.

#include <mutex>

#include "clipx_attn_plan.h"
#include "clipx_host.h"

using namespace clipx;

static int gemm_hook(int device, const void* A_bf16, const void* W_bf16, const float* bias, void* out, int M, int N, int K, int epi,
                     const float* rowscale, void* out16, void* stream, int f16 = 0, float stats_eps = 0.f) {
  if (!A_bf16 || !W_bf16 || !out || M <= 0 || N <= 0 || K <= 0) return fail(CLIPX_E_ARG, "bad gemm arguments");
  if (!((epi >= 0 && epi <= 3) || epi == EPI_BIAS_RESID_H16 || epi == EPI_BIAS_F16) || !bias) return fail(CLIPX_E_ARG, "epi must be 0..3, 6 or 7 and bias non-null");
  if (f16 && epi > 2 && epi != EPI_BIAS_F16) return fail(CLIPX_E_ARG, "fp16 operands go with the 16-bit-output epilogues 0..2 and 7 only");
  if (N % 128 || K % 64) return fail(CLIPX_E_UNSUPPORTED, "N must be a multiple of 128 and K of 64");
  HIPCHK(hipSetDevice(device));
  GemmArgs g{};
  g.A = (const bf16*)A_bf16; g.W = (const bf16*)W_bf16; g.bias = bias; g.out = out; g.table = nullptr; g.T = 1;
  g.M = M; g.N = N; g.K = K; g.epi = epi;
  g.rowscale = rowscale;
  g.out16 = epi == 3 ? (bf16*)out16 : nullptr;
  g.f16 = f16;
  g.stats_eps = stats_eps;
  if (stats_eps > 0.f && !g.rowscale) return fail(CLIPX_E_ARG, "a GEMM that owns its LayerNorm statistics needs the [M] row-scale buffer");
  if (!g.rowscale) {  // bf16-output epilogues scale rows (LayerNorm-folded GEMMs of the encoder); a plain GEMM uses ones
    static std::mutex ones_mu;
    static float* ones[64] = {};
    static int ones_n[64] = {};
    std::lock_guard<std::mutex> lk(ones_mu);
    if (device < 0 || device >= 64) return fail(CLIPX_E_ARG, "bad device");
    if (ones_n[device] < M) {
      if (ones[device]) (void)hipFree(ones[device]);
      ones[device] = nullptr;
      ones_n[device] = 0;
      HIPCHK(hipMalloc((void**)&ones[device], (size_t)M * sizeof(float)));
      HIPCHK(launch_fill_f32(ones[device], 1.f, M, (hipStream_t)stream));
      HIPCHK(hipStreamSynchronize((hipStream_t)stream));
      ones_n[device] = M;
    }
    g.rowscale = ones[device];
  }
  const char* gv = getenv("CLIPX_GEMM_VARIANT");
  g.variant = gv ? std::min((int)clipx::GEMM_V_MAX, std::max(0, atoi(gv))) : (int)clipx::GEMM_V_DEFAULT;
  int ncu = 0;
  HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
  g.n_cu = ncu;
  g.row0 = 0;
  HIPCHK(launch_gemm(g, (hipStream_t)stream));
  return CLIPX_OK;
}

extern "C" int clipx_gemm_bf16_device(int device, const void* A_bf16, const void* W_bf16, const float* bias, void* out,
                                      int M, int N, int K, int epi, void* stream) {
  return gemm_hook(device, A_bf16, W_bf16, bias, out, M, N, K, epi, nullptr, nullptr, stream);
}
extern "C" int clipx_gemm_bf16_ex_device(int device, const void* A_bf16, const void* W_bf16, const float* bias, void* out, int M,
                                         int N, int K, int epi, const float* rowscale_or_null, void* out16_or_null, void* stream) {
  return gemm_hook(device, A_bf16, W_bf16, bias, out, M, N, K, epi, rowscale_or_null, out16_or_null, stream);
}

extern "C" int clipx_gemm_f16_device(int device, const void* A_f16, const void* W_f16, const float* bias, void* out_bf16, int M, int N,
                                     int K, int epi, const float* rowscale_or_null, void* stream) {
  return gemm_hook(device, A_f16, W_f16, bias, out_bf16, M, N, K, epi, rowscale_or_null, nullptr, stream, 1);
}

extern "C" int clipx_gemm_f16_ln_device(int device, const void* A_f16, const void* W_f16, const float* bias, void* out_16bit, int M, int N,
                                        int K, int epi, float* rstd_buf, float eps, void* stream) {
  if (!(eps > 0.f)) return fail(CLIPX_E_ARG, "eps must be positive");
  return gemm_hook(device, A_f16, W_f16, bias, out_16bit, M, N, K, epi, rstd_buf, nullptr, stream, 1, eps);
}

// One GEMM through a handle's profiler, exactly as the encoder issues its own (clipx_encode.hip run_gemm: one scope, the handle's
// variant and compute units, 2 M N K flops) -- for the tests of the GEMM brackets, which need every kernel family on a shape of
// their choosing.  Only what a kernel would dereference is validated here (the operands, the bias or the table); which shapes,
// epilogues and operand types have a plan is launch_gemm's business, and what it refuses comes back as CLIPX_E_HIP with the scope
// recorded (that is one of the things tested).
extern "C" int clipx_profile_gemm_device(clipx_handle* h, const void* A, const void* W, const float* bias_or_null, void* out,
                                         const float* table_or_null, int T, int M, int N, int K, int epi, int f16,
                                         const float* rowscale_or_null, void* stream) {
  if (!h || !A || !W || !out || M <= 0 || N <= 0 || K <= 0) return fail(CLIPX_E_ARG, "bad gemm arguments");
  if (epi == EPI_TABLE_F32 ? (!table_or_null || T <= 0) : !bias_or_null)
    return fail(CLIPX_E_ARG, "epilogue 4 needs its table and T > 0, every other epilogue its bias");
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  GemmArgs g{};
  g.A = (const bf16*)A; g.W = (const bf16*)W; g.bias = bias_or_null; g.out = out; g.table = table_or_null; g.T = T;
  g.M = M; g.N = N; g.K = K; g.epi = epi; g.variant = h->gemm_variant; g.n_cu = h->n_cu;
  g.rowscale = rowscale_or_null; g.f16 = f16 ? 1 : 0;
  return profiled_gemm(h, g, (hipStream_t)stream, 2.0 * M * (double)N * K);
}

// the T limits of the attention entry points (clipx_attn_plan.h): nullptr when T is within them, else the message; nothing is launched
static const char* attention_limit(int T, int dh, int causal) {
  if (T > clipx::ATTN_LONG_MAX_T) return "sequence longer than 608 tokens";
  if (T > clipx::ATTN_SHORT_MAX_T && causal) return "causal sequence longer than 288 tokens";
  if (T > clipx::ATTN_SHORT_MAX_T && dh != 64) return "sequence longer than 288 tokens at a head dimension other than 64";
  if (clipx::attn_wide_head(dh) && causal) return "head dimensions 88 and 104 have no causal attention kernel";
  if (dh != 64 && clipx::attn_plan(T, dh, causal).kernel == clipx::ATTN_NONE)
    return "no attention kernel for head dimensions 80, 88 and 104 at 97 .. 256 tokens";
  return nullptr;
}
static bool attention_dh_known(int dh) { return dh == 64 || dh == 80 || clipx::attn_wide_head(dh); }

extern "C" int clipx_attention_device(int device, const void* qkv_bf16, void* out_bf16, int B, int T, int H, int causal,
                                      void* stream) {
  if (!qkv_bf16 || !out_bf16 || B <= 0 || T <= 0 || H <= 0) return fail(CLIPX_E_ARG, "bad attention arguments");
  if (const char* why = attention_limit(T, 64, causal)) return fail(CLIPX_E_UNSUPPORTED, why);
  HIPCHK(hipSetDevice(device));
  HIPCHK(launch_attention((const bf16*)qkv_bf16, (bf16*)out_bf16, B, T, H, 64, causal, (hipStream_t)stream));
  return CLIPX_OK;
}

extern "C" int clipx_attention_dh_device(int device, const void* qkv_bf16, void* out_bf16, int B, int T, int H, int dh,
                                         int causal, void* stream) {
  if (!qkv_bf16 || !out_bf16 || B <= 0 || T <= 0 || H <= 0) return fail(CLIPX_E_ARG, "bad attention arguments");
  if (!attention_dh_known(dh)) return fail(CLIPX_E_UNSUPPORTED, "head dimension must be 64, 80, 88 or 104");
  if (const char* why = attention_limit(T, dh, causal)) return fail(CLIPX_E_UNSUPPORTED, why);
  HIPCHK(hipSetDevice(device));
  hipError_t e = launch_attention((const bf16*)qkv_bf16, (bf16*)out_bf16, B, T, H, dh, causal, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(CLIPX_E_UNSUPPORTED, "no attention kernel for this (T, head dimension)");
  HIPCHK(e);
  return CLIPX_OK;
}

// launch_attention with the encoder's own two extras (run_layers): the pooled last block's q_blocks and the ragged batches' offs /
// lens.  Every refusal is made here, before the device is touched, so launch_attention is never asked for a kernel it has not
extern "C" int clipx_attention_ex_device(int device, const void* qkv_f16, void* out_bf16, int B, int T, int H, int dh, int causal,
                                         int q_blocks, const int32_t* offs, const int32_t* lens, void* stream) {
  if (!qkv_f16 || !out_bf16 || B <= 0 || T <= 0 || H <= 0 || q_blocks < 0) return fail(CLIPX_E_ARG, "bad attention arguments");
  if (!attention_dh_known(dh)) return fail(CLIPX_E_UNSUPPORTED, "head dimension must be 64, 80, 88 or 104");
  if (const char* why = attention_limit(T, dh, causal)) return fail(CLIPX_E_UNSUPPORTED, why);
  if ((offs != nullptr) != (lens != nullptr)) return fail(CLIPX_E_ARG, "offs and lens go together: both or neither");
  if (offs && (dh != 64 || T > 128))
    return fail(CLIPX_E_UNSUPPORTED, "ragged batches (offs / lens) need head dimension 64 and at most 128 tokens");
  HIPCHK(hipSetDevice(device));
  hipError_t e = launch_attention((const bf16*)qkv_f16, (bf16*)out_bf16, B, T, H, dh, causal, (hipStream_t)stream, q_blocks, offs, lens);
  if (e == hipErrorInvalidValue) return fail(CLIPX_E_UNSUPPORTED, "no attention kernel for this (T, head dimension)");
  HIPCHK(e);
  return CLIPX_OK;
}

extern "C" int clipx_layernorm_device(int device, const float* x, const float* gamma, const float* beta, void* y,
                                      int out_bf16, int M, int d, float eps, void* stream) {
  if (!x || !gamma || !beta || !y || M <= 0) return fail(CLIPX_E_ARG, "bad layernorm arguments");
  if (d <= 0 || d % 128 || d > 2048) return fail(CLIPX_E_UNSUPPORTED, "d must be a multiple of 128, <= 2048");
  HIPCHK(hipSetDevice(device));
  HIPCHK(launch_layernorm(x, gamma, beta, y, out_bf16, M, d, eps, (hipStream_t)stream));
  return CLIPX_OK;
}

extern "C" int clipx_rowstats_device(int device, const void* x16, int is_f16, float* rstd, int M, int d, float eps, void* stream) {
  if (!x16 || !rstd || M <= 0) return fail(CLIPX_E_ARG, "bad rowstats arguments");
  if (d <= 0 || d % 128 || d > 2048) return fail(CLIPX_E_UNSUPPORTED, "d must be a multiple of 128, <= 2048");
  HIPCHK(hipSetDevice(device));
  HIPCHK(launch_rowstats(x16, rstd, M, d, eps, (hipStream_t)stream, is_f16 ? 1 : 0, nullptr, is_f16 == 2 ? 1 : 0));
  return CLIPX_OK;
}

extern "C" int clipx_tail_device(int device, const void* x_f16, const float* gamma, const float* beta, const void* proj_bf16,
                                 uint16_t* out_f16, float* out_f32_or_null, float* scratch, int B, int d, int E, float eps,
                                 int rows_per_workgroup, void* stream) {
  if (!x_f16 || !gamma || !beta || !proj_bf16 || !out_f16 || !scratch || B <= 0 || E <= 0) return fail(CLIPX_E_ARG, "bad tail arguments");
  if (d % 32 || d <= 0) return fail(CLIPX_E_UNSUPPORTED, "d must be a multiple of 32");
  HIPCHK(hipSetDevice(device));
  if (rows_per_workgroup < 0) return tail_batched_rows(B, d, E);  // a query: what the encoder's own call picks for this shape
  hipError_t e = launch_tail(x_f16, nullptr, gamma, beta, (const bf16*)proj_bf16, out_f16, out_f32_or_null, scratch, B, 1, d, E, eps,
                             (hipStream_t)stream, 1, nullptr, rows_per_workgroup);
  if (e == hipErrorInvalidValue) return fail(CLIPX_E_UNSUPPORTED, "no projection kernel with this many rows per workgroup for this d");
  HIPCHK(e);
  return CLIPX_OK;
}
