// attn_long.hip -- attention_long_kernel: the flash-style attention of the long image sequences (ViT-L/14@336px, T = 577), and its launcher.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "attn_common.h"

namespace clipx {

// =============================================================================================
// Long sequences (head dim 64, not causal, 10 .. 19 key blocks: T = 289 .. 608, ViT-L/14@336px's T = 577).
// The S^T blocks of a query block no longer fit the registers (19 x 16) and two K/V images no longer fit the LDS, so this is a
// flash-style kernel: one workgroup of ATTN_LONG_NW = 10 waves per (batch, head), K and V^T staged whole in attention_kernel's
// LDS images (K: 128-B rows, chunk XOR swizzle; V^T: row stride TP * 2 + 8) sized from the run-time number of key blocks, and
// every wave walks the key blocks ONCE per query block it owns (blocks w and w + 10) with a running softmax:
//   S^T block = K_kb Q^T (4 MFMAs) -> block max, one exchange with lane ^ 32 -> m' = max(m, block max)
//   when m' > m on any lane of the wave: O, sum *= exp2((m - m') c)   (exactly 0 in the first block, m = -inf; exactly 1 on the
//   lanes whose max did not move, so skipping the rescale where no lane moved changes no bit)
//   P = exp2(S c - m' c) -> fp16 (attn_pack_p), sum += P, O^T += V^T_kb P^T (4 MFMAs)
// and divides by the sum once at the end.  Operation for operation the arithmetic of attention_kernel, except that P is taken
// against the running maximum and O and the sum are rescaled when it moves.  What a query block computes does not depend on
// q_blocks, so the pooled last block (q_blocks = 1) gets the bits of a full launch.
// =============================================================================================
__global__ __launch_bounds__(clipx::ATTN_LONG_NW * 64, (clipx::ATTN_LONG_NW + 3) / 4) void attention_long_kernel(
    const bf16* __restrict__ qkv, bf16* __restrict__ out, int T, int H, int nkb, float scale_log2e, int q_blocks) {
  constexpr int NW = clipx::ATTN_LONG_NW, QPW = clipx::ATTN_LONG_QPW, NT = NW * 64;
  constexpr int DH = 64, CH = 8, KS = 4, KROW = 128, NB = 2;
  const int TP = nkb * 32;
  const int VT_STRIDE = TP * 2 + 8;  // bytes per V^T row: odd multiple of 8 -> conflict-free ds_read_b64
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sK = smem;               // [TP][KROW]
  unsigned char* sVt = smem + TP * KROW;  // [DH][VT_STRIDE]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int hb = lane >> 5, l31 = lane & 31;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int ld = 3 * H * DH;
  const bf16* qbase = qkv + (size_t)b * T * ld + h * DH;
  const bf16* kbase = qbase + H * DH;
  const bf16* vbase = qbase + 2 * H * DH;

  // ---- Q fragments of both query blocks of this wave, requested before the staging (B operand: lane (q = l31, hb) holds
  // Q[q][16s + 8hb .. +8]); rows past T (the pad of the last block, and slot 1 of a wave that has no second block) are clamped
  bf16x8 qf_all[QPW][KS];
#pragma unroll
  for (int qi = 0; qi < QPW; ++qi) {
    const int qpos = clipx::attn_query_block(NW, w, qi) * 32 + l31;
    const int qrow = qpos < T ? qpos : T - 1;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const uint4 v = *reinterpret_cast<const uint4*>(qbase + (size_t)qrow * ld + 16 * s + 8 * hb);
      qf_all[qi][s] = *reinterpret_cast<const bf16x8*>(&v);
    }
  }

  // ---- stage K: 8 lanes cover one key's row; batches of 4 unconditional loads (row clamped, zeroed after)
  for (int base = 0; base < TP * CH; base += NT * 4) {
    uint4 kv[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int i = base + it * NT + tid;
      int key = i >> 3;
      key = key < T ? key : T - 1;
      kv[it] = *reinterpret_cast<const uint4*>(kbase + (size_t)key * ld + (i & 7) * 8);
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int i = base + it * NT + tid;
      const int key = i >> 3, c = i & 7;
      if (i < TP * CH) {
        const uint4 v = key < T ? kv[it] : make_uint4(0u, 0u, 0u, 0u);
        *reinterpret_cast<uint4*>(sK + key * KROW + ((c ^ ((key >> 1) & 7)) << 4)) = v;
      }
    }
  }
  // ---- stage V transposed: a thread takes keys (2kp, 2kp+1) x 8 d and writes 8 packed key-pairs
  for (int base = 0; base < (TP / 2) * CH; base += NT * 2) {
    uint4 v0s[2], v1s[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = base + it * NT + tid;
      const int kp = i >> 3, c = i & 7;
      const int k0 = 2 * kp < T ? 2 * kp : T - 1, k1 = 2 * kp + 1 < T ? 2 * kp + 1 : T - 1;
      v0s[it] = *reinterpret_cast<const uint4*>(vbase + (size_t)k0 * ld + c * 8);
      v1s[it] = *reinterpret_cast<const uint4*>(vbase + (size_t)k1 * ld + c * 8);
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = base + it * NT + tid;
      const int kp = i >> 3, c = i & 7;
      if (i < (TP / 2) * CH) {
        const uint4 v0 = 2 * kp < T ? v0s[it] : make_uint4(0u, 0u, 0u, 0u);
        const uint4 v1 = 2 * kp + 1 < T ? v1s[it] : make_uint4(0u, 0u, 0u, 0u);
        const unsigned a0[4] = {v0.x, v0.y, v0.z, v0.w}, a1[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const unsigned lo = (a0[jj] & 0xffffu) | (a1[jj] << 16);      // d = 8c + 2jj
          const unsigned hi = (a0[jj] >> 16) | (a1[jj] & 0xffff0000u);  // d = 8c + 2jj + 1
          *reinterpret_cast<unsigned*>(sVt + (8 * c + 2 * jj) * VT_STRIDE + kp * 4) = lo;
          *reinterpret_cast<unsigned*>(sVt + (8 * c + 2 * jj + 1) * VT_STRIDE + kp * 4) = hi;
        }
      }
    }
  }
  __syncthreads();

  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  const int ksw = (l31 >> 1) & 7;
  const int tail_keys = T - (nkb - 1) * 32;  // keys of the last key block that exist
#pragma unroll
  for (int qi = 0; qi < QPW; ++qi) {
    const int qb = clipx::attn_query_block(NW, w, qi);  // the dealing the CPU check walks (clipx_attn_plan.h)
    if (qb >= q_blocks) break;  // q_blocks = nkb, or 1 when only the rows of query block 0 are read afterwards
    const int qpos = qb * 32 + l31;
    bf16x8 qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = qf_all[qi][s];
    float mx = -INFINITY;  // running max of the raw logits of this lane's query column (both lane halves hold the same value)
    f32x2_t sum2 = {0.f, 0.f};
    f32x16 oacc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[nb][r] = 0.f;
#pragma unroll 1
    for (int kb = 0; kb < nkb; ++kb) {
      f32x16 sb;
#pragma unroll
      for (int r = 0; r < 16; ++r) sb[r] = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + (kb * 32 + l31) * KROW + (((2 * s + hb) ^ ksw) << 4));
        sb = attn_mfma(kf, qf[s], sb);
      }
      const bool last = kb == nkb - 1;
      if (last) {  // keys past T
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hb;
          sb[r] = key < T ? sb[r] : -INFINITY;
        }
      }
      float bm = sb[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) bm = fmaxf(bm, sb[r]);
      bm = fmaxf(bm, __shfl_xor(bm, 32));
      const float mnew = fmaxf(mx, bm);
      if (__builtin_amdgcn_ballot_w64(mnew > mx) != 0ull) {
        // exp2(-inf) = 0 in the first block (O and the sum are 0 there anyway); a lane whose max stayed gets exactly 1, and
        // -inf against -inf (a column that has seen masked keys only) is 1 as well, never exp2(NaN)
        const float alpha = mnew == mx ? 1.f : __builtin_amdgcn_exp2f((mx - mnew) * scale_log2e);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[nb][r] *= alpha;
        sum2 *= (f32x2_t){alpha, alpha};
        mx = mnew;
      }
      const float nmx = mx == -INFINITY ? 0.f : -mx * scale_log2e;
      // in the last key block only the first `tail_keys` keys exist (T = 577: 1 of 32): when they all sit in the first register
      // quad the other 12 exponentials are skipped (their P is exactly 0)
      const bool short_tail = last && tail_keys <= 4;
      unsigned pw[8];
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        if (short_tail && r >= 4) {
          pw[r >> 1] = 0u;
          continue;
        }
        const f32x2_t e = (f32x2_t){sb[r], sb[r + 1]} * (f32x2_t){scale_log2e, scale_log2e} + (f32x2_t){nmx, nmx};
        const f32x2_t pp = {__builtin_amdgcn_exp2f(e[0]), __builtin_amdgcn_exp2f(e[1])};
        sum2 += pp;
        pw[r >> 1] = attn_pack_p(pp[0], pp[1]);
      }
      bf16x8 pf[2];
      {
        const uint4 w0 = make_uint4(pw[0], pw[1], pw[2], pw[3]), w1 = make_uint4(pw[4], pw[5], pw[6], pw[7]);
        pf[0] = *reinterpret_cast<const bf16x8*>(&w0);
        pf[1] = *reinterpret_cast<const bf16x8*>(&w1);
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          // lane (d = 32nb + l31, hb): keys kb*32 + 16*s2 + 4hb + {0..3} and + 8 + {0..3}
          const unsigned char* vp = sVt + (32 * nb + l31) * VT_STRIDE + (kb * 32 + 16 * s2 + 4 * hb) * 2;
          const uint2 lo = *reinterpret_cast<const uint2*>(vp);
          const uint2 hi = *reinterpret_cast<const uint2*>(vp + 16);
          uint4 vv = make_uint4(lo.x, lo.y, hi.x, hi.y);
          oacc[nb] = attn_mfma(*reinterpret_cast<bf16x8*>(&vv), pf[s2], oacc[nb]);
        }
    }
    float sum = sum2[0] + sum2[1];
    sum += __shfl_xor(sum, 32);
    const float inv = sum > 0.f ? 1.f / sum : 0.f;
    // ---- store: lane owns query qpos, d = 32nb + 8g + 4hb + {0..3}
    if (qpos < T) {
      bf16* orow = out + ((size_t)b * T + qpos) * (H * DH) + h * DH;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (bf16)(oacc[nb][4 * g + e] * inv);
          *reinterpret_cast<bf16x4*>(orow + 32 * nb + 8 * g + 4 * hb) = o;
        }
    }
  }
}

hipError_t launch_attention_long(const bf16* qkv, bf16* out, int B, int T, int H, hipStream_t st, int q_blocks, const AttnPlan& plan) {
  if (plan.kernel != clipx::ATTN_LONG || plan.lds_bytes > clipx::ATTN_LDS_LIMIT) return hipErrorInvalidValue;
  q_blocks = q_blocks > 0 && q_blocks < plan.nkb ? q_blocks : plan.nkb;
  auto kern = attention_long_kernel;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(B * H), dim3(plan.nw * 64), plan.lds_bytes, st, qkv, out, T, H, plan.nkb,
                     (1.f / 8.f) * 1.4426950408889634f, q_blocks);
  return hipGetLastError();
}

}  // namespace clipx
