// clipx_attn_plan.h -- which attention kernel runs for a (T, head dimension, causal) and with what geometry (attn_block.hip,
// launch_attention).  No device code in here: plain integer arithmetic, so that a host-only program can drive it
// (tools/attn_plan_check.cpp).
//
// Keys and queries are cut into blocks of 32.  NKB = ceil(T / 32) key blocks:
//   NKB <= 9  (T <= 288)  attention_kernel<DH, NKB, NW, QPW, CAUSAL, RECOMP>: one workgroup of NW waves per (batch, head), every wave
//                         keeps the NKB score blocks of a query block in registers (or computes them twice, RECOMP); dh 64 at NKB = 9
//                         and not causal is the persistent attention_pk_kernel (two K/V images of 72 KiB by LDS-DMA).
//   NKB 10 .. 19 (T 289 .. 608), dh 64, not causal: attention_long_kernel, K and V^T whole in the LDS, a run-time loop over the
//                         key blocks with a running softmax, ATTN_LONG_NW waves that own at most ATTN_LONG_QPW query blocks each.
//   everything else       no kernel: the launch is refused (causal or dh 80 above 288 tokens, anything above 608, dh 80 at NKB 4 .. 8).
// Head dimensions 88 and 104 (ViT-g/14, ViT-bigG/14 image towers) have the rows of dh 80 -- NKB 1 .. 3 and NKB 9 (nine waves, RECOMP) --
// and only not causal: 88 and 104 are not multiples of the 16-wide MFMA k-step, so the QK^T product ends in a half step whose upper
// half is zero in both operands (attn_krow_bytes: the K rows carry a zeroed pad chunk for it).
// Ragged batches (offs / lens) ride on the dh 64, NKB <= 4 rows only; that restriction stays in launch_attention.
#pragma once

#include <stddef.h>

namespace clipx {

enum AttnKernel {
  ATTN_NONE = 0,   // refused
  ATTN_BLOCK = 1,  // attention_kernel
  ATTN_PK9 = 2,    // attention_pk_kernel
  ATTN_LONG = 3,   // attention_long_kernel
};

constexpr int ATTN_SHORT_MAX_T = 288;     // 9 key blocks: the register-resident kernels
constexpr int ATTN_LONG_MAX_T = 608;      // 19 key blocks: K + V^T of one head fill the LDS
constexpr int ATTN_LONG_NW = 10;          // waves of a long-sequence workgroup
constexpr int ATTN_LONG_QPW = 2;          // query blocks a wave owns at the most
constexpr size_t ATTN_LDS_LIMIT = 163840;  // bytes of LDS one workgroup can have on gfx950

struct AttnPlan {
  int kernel = ATTN_NONE;
  int nkb = 0;           // key blocks (= query blocks of a full launch)
  int nw = 0;            // waves per workgroup
  int qpw = 0;           // query blocks per wave
  bool recomp = false;   // attention_kernel's RECOMP form
  size_t lds_bytes = 0;  // dynamic LDS of the launch
};

constexpr bool attn_wide_head(int dh) { return dh == 88 || dh == 104; }  // the head dimensions that end QK^T in a half k-step

// Bytes of one K row in the LDS -- the ONE expression the kernels, their launchers and tools/attn_plan_check.cpp take it from.
// dh 64: 128 B, the 16-B chunk position swizzled (XOR).  Every other dh: the 2 ceil(dh / 16) chunks the k-steps read (the last one
// a zeroed pad chunk when dh is not a multiple of 16), made an ODD number of chunks so that the ds_read_b128 of 32 consecutive keys
// spreads over the banks without a swizzle: 11 chunks = 176 B (dh 80), 13 = 208 B (dh 88), 15 = 240 B (dh 104).
constexpr size_t attn_krow_bytes(int dh) { return dh == 64 ? 128 : (size_t)((2 * ((dh + 15) / 16)) | 1) * 16; }
constexpr size_t attn_dv(int dh) { return (size_t)(dh + 31) / 32 * 32; }  // rows of V^T: dh rounded up to the 32-row output block

// LDS of the one-head images: K rows of attn_krow_bytes, V^T rows of nkb * 64 + 8 bytes, DV = dh rounded up to 32
constexpr size_t attn_image_bytes(int dh, int nkb) {
  return (size_t)nkb * 32 * attn_krow_bytes(dh) + attn_dv(dh) * ((size_t)nkb * 64 + 8);
}

inline AttnPlan attn_plan(int T, int dh, int causal) {
  AttnPlan p;
  if (T <= 0 || T > ATTN_LONG_MAX_T || (dh != 64 && dh != 80 && !attn_wide_head(dh))) return p;
  const int nkb = (T + 31) / 32;
  auto block = [&](int nw, int qpw, bool recomp) {
    p.kernel = ATTN_BLOCK;
    p.nkb = nkb, p.nw = nw, p.qpw = qpw, p.recomp = recomp;
    p.lds_bytes = attn_image_bytes(dh, nkb);
  };
  if (T > ATTN_SHORT_MAX_T) {
    if (dh != 64 || causal) return p;
    p.kernel = ATTN_LONG;
    p.nkb = nkb, p.nw = ATTN_LONG_NW, p.qpw = ATTN_LONG_QPW;
    p.lds_bytes = attn_image_bytes(64, nkb);
    return p;
  }
  if (attn_wide_head(dh) && causal) return p;
  if (dh != 64) {  // 80, 88, 104
    if (nkb <= 3) block(nkb, 1, false);
    else if (nkb == 9) block(9, 1, true);
    return p;
  }
  switch (nkb) {
    case 1: case 2: case 3: case 4: block(nkb, 1, false); break;
    case 5: case 6: block(3, 2, false); break;
    case 7: case 8: block(4, 2, false); break;
    default:  // 9
      if (causal) block(3, 3, false);
      else {
        p.kernel = ATTN_PK9;
        p.nkb = 9, p.nw = 6, p.qpw = 2;
        p.lds_bytes = (size_t)2 * (288 * 128 + 2 * 288 * 64);
      }
  }
  return p;
}

// Query blocks are dealt round-robin: slot qi of wave w is block qi * nw + w.  attention_long_kernel calls this very function
// (constexpr, so device code may); attention_kernel holds the same expression; the persistent attention_pk_kernel deals its nine
// blocks by a role table of its own, which these do not describe.
constexpr int attn_query_block(int nw, int w, int qi) { return qi * nw + w; }
inline int attn_wave_of(const AttnPlan& p, int qb) { return p.nw > 0 ? qb % p.nw : -1; }
inline int attn_slot_of(const AttnPlan& p, int qb) { return p.nw > 0 ? qb / p.nw : -1; }
// the query block wave w computes in its slot qi, or -1 when there is none below q_blocks
inline int attn_block_of(const AttnPlan& p, int w, int qi, int q_blocks) {
  const int qb = attn_query_block(p.nw, w, qi);
  return (w >= 0 && w < p.nw && qi >= 0 && qi < p.qpw && qb < q_blocks) ? qb : -1;
}

}  // namespace clipx
