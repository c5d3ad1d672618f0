// clipx_ragged_plan.h -- the integer host arithmetic of a ragged text batch, shared by the CLIP text tower (clipx_encode.hip) and
// the multilingual towers (bertx_api.hip).  System headers only, no HIP: tools/ragged_plan_check.cpp runs it under the sanitizers.
//
// Sample b owns lens[b] packed rows.  Where the folded GEMMs of the batch run in the 256x256 kernel the row count M is rounded up
// to Mp, a multiple of 256 (gemm256_whole_tile_rows, clipx_gemm_plan.h: launch_gemm's own rule), so that no GEMM of the tower needs
// a second launch for a handful of leftover rows.  The P = Mp - M extra rows are duplicates of real rows: pseudo-samples that are
// prefixes of the longest sample b* (the first of equal maxima), ceil(P / lens[b*]) of them, the last one shortened so that the
// lengths sum to Mp.  Attention stays inside a sample and everything else is row-wise, so a prefix of a real sample goes through
// exactly the arithmetic of its real rows: every pad row holds the bytes of a real row (nothing a GEMM reads is uninitialised, and
// the fp16 range flag cannot fire where the unpadded batch would not), no real row changes, and no pad row is ever pooled.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace clipx {

constexpr int RAGGED_PAD_MAX = 255;  // most rows a batch is padded by (whole 256-row m-tiles)

// what one handle sizes its buffers by: rows / samples of the largest padded batch (a pseudo-sample owns one pad row at least)
constexpr size_t ragged_max_rows(size_t B, size_t T) { return B * T + RAGGED_PAD_MAX; }
constexpr size_t ragged_max_samples(size_t B) { return B + RAGGED_PAD_MAX; }
// ints of one slot: lens / offs / src [S] and, with_rowmap, the pooled rows [B] and the row map [Mp]
constexpr size_t ragged_slot_ints(size_t B, size_t T, bool with_rowmap) {
  return 3 * ragged_max_samples(B) + (with_rowmap ? B + ragged_max_rows(B, T) : 0);
}

// The pooling rule of the CLIP text tower (launch_tail's / gather_pooled's): the highest id, first occurrence -- torch.argmax of
// the reference model.  The sample's rows end there: length = position + 1.
inline int ragged_pooled_len(const int32_t* row, int T) {
  int best = 0;
  for (int t = 1; t < T; ++t)
    if (row[t] > row[best]) best = t;
  return best + 1;
}

struct RaggedPlan {
  int S = 0;      // samples the attention sees: B + the pseudo-samples that own the pad rows (0: the batch was refused)
  int M = 0;      // the real rows
  int lmax = 0;   // rows of the longest sample
  size_t ints = 0;  // what the slot holds: the upload
  // into the slot, in this order
  int *lens = nullptr, *offs = nullptr;  // [S] rows of sample b / its first row
  int* src = nullptr;                    // [S] the real sample whose rows sample b repeats (b itself for b < B)
  int* pool = nullptr;                   // [B] with_rowmap: the last row of sample b
  int* rowmap = nullptr;                 // [Mp] with_rowmap: packed row -> src * T + t
};

// Completes a batch of B >= 1 samples of real[b] in 1 .. T rows to Mp rows in all, into `slot` (ragged_slot_ints(B, T,
// with_rowmap) ints; `real` may be the slot itself).  Refuses -- S = 0, nothing written -- a pad outside 0 .. RAGGED_PAD_MAX: the
// capacities above hold for no other.
inline RaggedPlan ragged_complete(int* slot, const int* real, int B, int T, int Mp, bool with_rowmap) {
  RaggedPlan p;
  int longest = 0;
  for (int b = 0; b < B; ++b) {
    if (real[b] > real[longest]) longest = b;
    p.M += real[b];
  }
  p.lmax = real[longest];
  const int pad = Mp - p.M;
  if (pad < 0 || pad > RAGGED_PAD_MAX || p.lmax < 1 || p.lmax > T) return p;
  const int S = B + (pad + p.lmax - 1) / p.lmax;
  p.lens = slot, p.offs = slot + S, p.src = slot + 2 * S;
  p.ints = 3 * (size_t)S;
  if (with_rowmap) p.pool = slot + 3 * S, p.rowmap = p.pool + B, p.ints += (size_t)B + Mp;
  for (int b = 0, m = 0, left = pad; b < S; ++b) {
    const int from = b < B ? b : longest, len = b < B ? real[b] : (left < p.lmax ? left : p.lmax);
    if (b >= B) left -= len;
    p.lens[b] = len, p.offs[b] = m, p.src[b] = from;
    if (with_rowmap) {
      for (int t = 0; t < len; ++t) p.rowmap[m + t] = from * T + t;
      if (b < B) p.pool[b] = m + len - 1;
    }
    m += len;
  }
  p.S = S;
  return p;
}

}  // namespace clipx
