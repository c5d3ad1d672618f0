// gemm_launch.hip -- launch_gemm: validate, plan (clipx_gemm_plan.h), issue the launches the plan names.
//
// The rule that cuts an [M, N] x K GEMM into a persistent 256x256 launch, its ragged m-tile and a 128x128 launch -- and that says
// which rows get their LayerNorm statistics inside the 4-wave kernel -- lives in gemm_plan() and is checked on the CPU
// (tools/gemm_plan_check.cpp); nothing is decided here.  Every kernel produces bit-identical rows, so the cut changes no output.

#include <hip/hip_runtime.h>
#include "clip_kernels.h"
#include "gemm_common.h"

namespace clipx {

hipError_t launch_gemm(const GemmArgs& g, hipStream_t st) {
  const bool stats = g.stats_eps > 0.f;  // a LayerNorm-folded GEMM that owns its row statistics: rowscale is the buffer they go to
  if (gemm_epi_out16(g.epi) && !g.rowscale) return hipErrorInvalidValue;
  const GemmPlan plan = gemm_plan(g.M, g.N, g.K, g.epi, g.f16 != 0, g.variant, g.n_cu, g.row0, stats, g.splitk_ws ? g.splitk_ws_bytes : 0);
  if (!plan.valid) return hipErrorInvalidValue;

  if (plan.stats_rows > 0) {  // the rows the 4-wave kernel does not take the sums of itself (gemm256w4.hip STATS)
    hipError_t e = launch_rowstats(reinterpret_cast<const char*>(g.A) + (size_t)plan.fused_rows * g.K * 2, const_cast<float*>(g.rowscale) + plan.fused_rows,
                                   plan.stats_rows, g.K, g.stats_eps, st, 1, g.range_flag, 1, g.events);
    if (e != hipSuccess) return e;
  }
  if (plan.kernel256 != GEMM256_NONE) {
    GemmArgs b = g;
    b.M = plan.rows256;
    b.tail_m0 = plan.tail_nb > 0 ? plan.rows256 : 0;
    b.tail_nb = plan.tail_nb;
    if (plan.fused_rows == 0) b.stats_eps = 0.f;  // (every row scale is in the buffer: a plain folded GEMM)
    hipError_t e = plan.kernel256 == GEMM256_W4 ? launch_gemm256w4(b, plan, st) : launch_gemm256sp(b, plan, st);
    if (e != hipSuccess) return e;
  }
  if (plan.rows128 > 0) {
    const int m0 = g.M - plan.rows128;
    GemmArgs r = g;
    r.stats_eps = 0.f;  // (the row scales were written above)
    r.A = g.A + (size_t)m0 * g.K;
    r.M = plan.rows128;
    const size_t esz = (g.epi == EPI_BIAS_RESID_F32 || g.epi == EPI_TABLE_F32) ? 4 : 2;  // (EPI_BIAS_RESID_H16: fp16 rows)
    r.out = reinterpret_cast<char*>(g.out) + (size_t)m0 * g.N * esz;
    r.row0 = g.row0 + m0;
    if (g.rowscale) r.rowscale = g.rowscale + m0;
    if (g.out16) r.out16 = g.out16 + (size_t)m0 * g.N;
    return launch_gemm128(r, plan, st);
  }
  return hipSuccess;
}

}  // namespace clipx
