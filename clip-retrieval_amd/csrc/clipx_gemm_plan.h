// clipx_gemm_plan.h -- which kernels one launch_gemm call runs, on which rows (gemm_launch.hip issues what the plan names; gemm128.hip,
// gemm256sp.hip and gemm256w4.hip refuse a launch it did not name).  System headers only, no HIP: plain integer arithmetic, so that
// tools/gemm_plan_check.cpp drives it on the CPU under the sanitizers.
//
// An [M, N] x K GEMM is cut along M:
//   rows [0, rows256)           whole 256-row m-tiles in ONE persistent 256x256 launch -- the 4-wave kernel where it has the form, the
//                               8-wave kernel elsewhere -- when the variant asks for one and the problem is large enough to fill the chip;
//   rows [rows256, + 256)       exactly one m-tile left over (ViT-L/14 at B = 256: 257 m-tiles on 256 CUs) rides inside that launch
//                               as strips of 32 rows x (tail_nb x 32) columns;
//   rows [M - rows128, M)       everything else in the 128x128 kernel: register-staged or LDS-DMA fill, the deep LDS ring where the
//                               offsets fit 32 bits, split along K when the call brought scratch and the problem is tiny (B = 1).
// A LayerNorm-folded GEMM that owns its row statistics (GemmArgs.stats_eps > 0) gets them inside the 4-wave kernel for the rows
// that kernel takes (fused_rows); a separate pass covers the other stats_rows.  Both are decided here, once.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace clipx {

enum GemmEpilogue {
  EPI_BIAS_BF16 = 0,        // out bf16 [M,N] = acc + bias                       (QKV projection)
  EPI_BIAS_QGELU_BF16 = 1,  // out bf16 = quick_gelu(acc + bias)                 (fc1, OpenAI CLIP)
  EPI_BIAS_GELU_BF16 = 2,   // out bf16 = gelu_erf(acc + bias)                   (fc1, open_clip LAION)
  EPI_BIAS_RESID_F32 = 3,   // out f32 [M,N] += acc + bias   (in place residual) (out_proj, fc2)
  EPI_TABLE_F32 = 4,        // out f32 = acc + table[m % T][n]                   (patch embed + cls/pos)
  EPI_RAW_F32 = 5,          // internal (split-K): out f32 [M,N] = acc, no bias; the reduction kernel applies the epilogue
  EPI_BIAS_RESID_H16 = 6,   // out fp16 [M,N] = fp16(f32(out) + (acc + bias)): the encoder's residual stream lives in IEEE fp16
                            // (out_proj, fc2): a third of the bytes of the f32 read-modify-write + bf16 shadow of EPI 3
  EPI_BIAS_F16 = 7          // out IEEE fp16 [M,N] = acc * rowscale + bias: EPI 0 with three more mantissa bits.  The QKV projection
                            // (round 4): q and k feed the softmax logits, where the bf16 rounding of EPI 0 was the largest single
                            // error of the encoder on weights with large LayerNorm gains (tools/emulate_fp16_stream.py)
};
// the 16-bit-output epilogues (bf16, or IEEE fp16 for EPI_BIAS_F16): out = act(acc * rowscale[m] + bias[n])
constexpr bool gemm_epi_out16(int epi) {
  return epi == EPI_BIAS_BF16 || epi == EPI_BIAS_QGELU_BF16 || epi == EPI_BIAS_GELU_BF16 || epi == EPI_BIAS_F16;
}
// the epilogues a caller may ask for (EPI_RAW_F32 is the split-K kernel's own)
constexpr bool gemm_epi_public(int epi) {
  return gemm_epi_out16(epi) || epi == EPI_BIAS_RESID_F32 || epi == EPI_BIAS_RESID_H16 || epi == EPI_TABLE_F32;
}

// GemmArgs.variant (CLIPX_GEMM_VARIANT picks one for the tests and the A/B tools; values in between run as GEMM_V_256_W8_TAIL_APART)
enum GemmVariant {
  GEMM_V_128_REG = 0,            // every row in the 128x128 kernel, register-staged LDS fill: the reference the tests compare against
  GEMM_V_128_DMA = 1,            // every row in the 128x128 kernel, LDS-DMA fill (deep ring / split-K where they apply)
  GEMM_V_256_W8 = 3,             // whole m-tiles in the 8-wave 256x256 kernel (gemm256sp.hip), a single leftover m-tile inside its launch
  GEMM_V_256_W8_TAIL_APART = 4,  // the same with the leftover m-tile always in a 128x128 launch of its own (A/B)
  GEMM_V_256_W4 = 6,             // the default: the 4-wave kernel (gemm256w4.hip) where it has the form, GEMM_V_256_W8 elsewhere
  GEMM_V_DEFAULT = GEMM_V_256_W4,
  GEMM_V_MAX = 6
};

// tiles
constexpr int G_TM = 128, G_TN = 128, G_BK = 64;     // the 128x128 kernel: N % G_TN == 0, K % G_BK == 0 is all launch_gemm asks
constexpr int G256_T = 256, G256_BK = 128;           // the persistent kernels: 256 x 256 output tiles, K % 128 == 0
constexpr int G256_STRIP = 32, G256_STRIP_ROWS = 8;  // a ragged m-tile inside them: 8 row blocks of 32 x column strips of tail_nb x 32
constexpr int G256_STRIP_NB_MAX = 4;                 // (the strip's operands must fit the LDS ring)
constexpr int SPLITK_MAX = 16, SPLITK_MAX_ROWS = 1024;

// workgroups of a persistent launch: one per CU, a multiple of the 8 XCDs
inline int gemm256_grid(int n_cu) {
  const int grid = (n_cu > 0 ? n_cu : 256) & ~7;
  return grid < 8 ? 8 : grid;
}

// How many 256-row m-tiles go to the persistent 256x256 kernel; the rest (ragged rows and the m-tiles that would only add a
// mostly-empty extra round over the CUs) goes to the 128x128 kernel.  ViT-L/14 at bs=256 has M = 257 * 256: 256 m-tiles fill the
// 256 CUs in whole rounds, the 257th (the class-token rows' worth) is peeled.
inline int gemm256_bulk_mtiles(int M, int N, int n_cu) {
  const int mt = M / G256_T, nt = N / G256_T;
  if (mt <= 0 || nt <= 0) return 0;
  const int cu = (n_cu > 0 ? n_cu : 256) & ~7;
  int best = mt;
  double best_cost = 1e30;
  for (int peel = 0; peel <= 8 && peel < mt; ++peel) {
    const int bulk = mt - peel;
    const int rounds = (bulk * nt + cu - 1) / cu;
    // cost in units of one 256x256 tile on one CU; peeled rows run as 128x128 tiles, two resident per CU, at
    // roughly 0.6x the per-CU rate of the big kernel
    const double rest = (double)(peel * 4 * nt) / (2.0 * cu);
    const double cost = rounds + (peel ? 0.25 * (rest > 1.0 ? rest : 1.0) / 0.6 : 0.0);
    if (cost < best_cost - 1e-9) { best_cost = cost; best = bulk; }
  }
  return best;
}

// One ragged m-tile (256 rows) inside the persistent launch: 8 row blocks x (N / 32) column blocks of 32 x 32 are dealt to the
// workgroups as strips of NB consecutive column blocks; NB <= 4, NB | N / 32, and every strip needs a workgroup.  0: not possible.
inline int gemm256_tail_blocks(int N, int K, int n_cu) {
  const int grid = gemm256_grid(n_cu);
  if (N % G256_STRIP || K % G256_BK || (size_t)G256_STRIP * K * 2 >= ((size_t)1 << 31)) return 0;
  const int cb = N / G256_STRIP;
  for (int nb = 1; nb <= G256_STRIP_NB_MAX; ++nb)
    if (cb % nb == 0 && G256_STRIP_ROWS * (cb / nb) <= grid) return nb;
  return 0;
}
inline int gemm256_tail_strips(int N, int tail_nb) { return tail_nb > 0 ? G256_STRIP_ROWS * (N / G256_STRIP / tail_nb) : 0; }

// The dispatch rule: the m-tiles of an [M, N] x K GEMM that run in a 256x256 kernel, 0 when every row goes to the 128x128 kernel in
// one launch (no 256-wide form, or a problem so small -- the query side's M = 257 or 77 rows -- that 256x256 tiles would leave most
// CUs idle and the 128x128 kernel gives it 4x the tiles).  Both kernels produce bit-identical rows.
inline int gemm256_dispatch_mtiles(int M, int N, int K, int variant, int n_cu) {
  if (variant < 2 || N % G256_T != 0 || K % G256_BK != 0 || M < G256_T) return 0;
  const int bulk = gemm256_bulk_mtiles(M, N, n_cu);
  const int cu = (n_cu > 0 ? n_cu : 256);
  return bulk > 0 && (int64_t)bulk * (N / G256_T) >= cu / 2 ? bulk : 0;
}

// Row count a caller that may append rows should bring (the ragged text batches are padded to it: clipx_ragged_plan.h): M rounded up
// to whole 256-row m-tiles where the rounded problem runs in the 256x256 kernel (the leftover rows would otherwise be a second,
// nearly empty 128x128 launch), M itself where every row runs in one 128x128 launch anyway and more rows would only be more work.
inline int gemm256_whole_tile_rows(int M, int N, int K, int variant, int n_cu) {
  const int Mp = (M + G256_T - 1) / G256_T * G256_T;
  return Mp != M && gemm256_dispatch_mtiles(Mp, N, K, variant, n_cu) > 0 ? Mp : M;
}

// the 4-wave 256x256 kernel has this (shape, epilogue, operand type): 16-bit-output epilogues and the fp16 in-place residual, K >= 256
inline bool gemm256w4_supports(int M, int N, int K, int epi, bool f16) {
  if (M <= 0 || M % G256_T != 0 || N % G256_T != 0 || K % G256_BK != 0 || K < 256) return false;
  return gemm_epi_out16(epi) || (!f16 && epi == EPI_BIAS_RESID_H16);
}
// ... and, for a GEMM that owns its LayerNorm statistics, the form that takes them from its own A fragments (STATS)
inline bool gemm256w4_fuses_stats(int M, int N, int K, int epi, bool f16) {
  return f16 && gemm256w4_supports(M, N, K, epi, f16) && gemm_epi_out16(epi);
}

// Number of K splits of an [M, N, K] problem in the 128x128 kernel on n_cu compute units with ws_bytes of scratch (1 = do not split).
// Measured at M = 257 (round 2): every launch has a floor of ~4.5 us, a split GEMM + its reduction cost 9.9 + 5.0 us whatever K is,
// the unsplit kernel 12 us at K = 1024 and 36 us at K = 4096: only long K loops pay.  A single m-tile (the text query, M = 77: 6 .. 24
// workgroups) gains from splitting shorter loops too (0.69 -> 0.62 ms).
inline int gemm_splitk_factor(int M, int N, int K, int epi, int n_cu, size_t ws_bytes) {
  if (ws_bytes == 0 || M > SPLITK_MAX_ROWS || epi == EPI_TABLE_F32 || epi == EPI_RAW_F32) return 1;
  const int nk = K / G_BK;
  if (nk < 8 || (nk < 32 && M > G_TM)) return 1;
  const int cu = n_cu > 0 ? n_cu : 256;
  const int tiles = ((M + G_TM - 1) / G_TM) * (N / G_TN);
  int S = 1;
  // the largest S <= 16 that divides the K loop, leaves each workgroup >= 4 K-tiles, does not go past one workgroup per CU
  // more than needed and fits the scratch
  for (int c = 2; c <= SPLITK_MAX; ++c) {
    if (nk % c != 0 || nk / c < 4) continue;
    if ((size_t)c * M * N * sizeof(float) > ws_bytes) break;
    if (tiles * (c - 1) >= cu) break;  // the previous split already filled the chip
    S = c;
  }
  return S;
}

enum Gemm256Kernel { GEMM256_NONE = 0, GEMM256_W8 = 1, GEMM256_W4 = 2 };  // gemm256sp.hip / gemm256w4.hip
enum Gemm128Fill { GEMM128_NONE = 0, GEMM128_REG = 1, GEMM128_DMA = 2, GEMM128_DMA_DEEP = 3 };

struct GemmPlan {
  bool valid = false;  // false: launch_gemm refuses the call as an invalid value before it launches anything
  // the persistent launch
  int kernel256 = GEMM256_NONE;
  int rows256 = 0;      // rows [0, rows256): bulk_tiles = (rows256 / 256) * (N / 256) tiles on grid256 workgroups
  int grid256 = 0;
  int bulk_tiles = 0;
  int tail_nb = 0;      // > 0: rows [rows256, rows256 + 256) ride inside it, tail_strips strips of 32 x (tail_nb x 32)
  int tail_strips = 0;
  // the 128x128 launch: rows [M - rows128, M)
  int rows128 = 0;
  int fill128 = GEMM128_NONE;
  int splitk = 1;       // > 1: that many K slices (deep ring, raw partial products) + the reduction kernel
  // LayerNorm statistics of a GEMM that owns them: rows [0, fused_rows) inside the 4-wave kernel, rows [fused_rows, M) -- stats_rows
  // of them -- by the statistics pass (both 0 when none were asked for)
  int fused_rows = 0;
  int stats_rows = 0;
};

// stats: the GEMM owns its LayerNorm statistics.  splitk_ws_bytes: the split-K scratch the call brought (0: none).
inline GemmPlan gemm_plan(int M, int N, int K, int epi, bool f16, int variant, int n_cu, int row0, bool stats, size_t splitk_ws_bytes) {
  GemmPlan p;
  if (M <= 0 || K <= 0 || N % G_TN != 0 || K % G_BK != 0 || !gemm_epi_public(epi)) return p;
  const bool out16 = gemm_epi_out16(epi);
  if (f16 && !out16) return p;             // fp16 operands exist for the 16-bit-output epilogues only (the LayerNorm-folded GEMMs)
  if (stats && !(f16 && out16)) return p;
  const int bulk = gemm256_dispatch_mtiles(M, N, K, variant, n_cu);
  int rest = M;
  if (bulk > 0) {
    p.rows256 = bulk * G256_T;
    p.grid256 = gemm256_grid(n_cu);
    p.bulk_tiles = bulk * (N / G256_T);
    p.kernel256 = variant == GEMM_V_256_W4 && gemm256w4_supports(p.rows256, N, K, epi, f16) ? GEMM256_W4 : GEMM256_W8;
    // exactly one m-tile left over: it rides in the same launch instead of a second, nearly empty one
    if (M - p.rows256 == G256_T && (variant == GEMM_V_256_W8 || variant == GEMM_V_256_W4) && row0 == 0) {
      p.tail_nb = gemm256_tail_blocks(N, K, n_cu);
      p.tail_strips = gemm256_tail_strips(N, p.tail_nb);
    }
    if (stats && p.kernel256 == GEMM256_W4 && gemm256w4_fuses_stats(p.rows256, N, K, epi, f16)) p.fused_rows = p.rows256;
    rest = p.tail_nb > 0 ? 0 : M - p.rows256;
  }
  if (stats) p.stats_rows = M - p.fused_rows;
  if (rest > 0) {
    p.rows128 = rest;
    const bool dma = bulk > 0 || variant >= GEMM_V_128_DMA;
    // the deep ring and the split kernel address their operands with 32-bit lane offsets
    const bool small_off = (size_t)rest * K * 2 < ((size_t)1 << 32) && (size_t)N * K * 2 < ((size_t)1 << 32);
    // rows of one large batch are computed the same way whichever kernel they land in: only a call that is one 128x128 launch splits
    if (dma && small_off && bulk == 0) p.splitk = gemm_splitk_factor(rest, N, K, epi, n_cu, splitk_ws_bytes);
    p.fill128 = !dma ? GEMM128_REG : (p.splitk > 1 || (K >= 2 * G_BK && small_off) ? GEMM128_DMA_DEEP : GEMM128_DMA);
  }
  p.valid = true;
  return p;
}

}  // namespace clipx
