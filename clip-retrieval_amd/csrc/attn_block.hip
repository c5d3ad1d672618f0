// attn_block.hip -- attention_kernel: one workgroup per (batch, head), every short-sequence form (T <= 288; head dim 64, 80, 88, 104;
// causal, ragged), and launch_attention, the dispatcher of all three attention kernel files (it needs these templates).
// Replaces the MHA inside `model.encode_image` / `model.encode_text` of the reference (clip_retrieval/clip_inference/mapper.py:57,65).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <math.h>
#include "attn_common.h"

namespace clipx {

// =============================================================================================
// Attention (head dim DH = 64, 80, 88 or 104): one workgroup per (batch, head); K (row-major) and V^T in LDS.
//   S^T = K Q^T   (MFMA A = K rows, B = Q rows): a lane holds 16 keys x NKB blocks of ONE query column
//   softmax over the lane's registers + one exchange with lane^32; P stays in registers as the B operand
//   O^T = V^T P^T (MFMA A = V^T rows from LDS, B = P): a lane ends with 4 consecutive d of its query -> 8-B stores
// The MFMA contraction index of the PV product is a permutation of the key index (the order in which the
// S^T accumulator registers hold keys); V^T fragments are read with the same permutation, so no lane
// exchange is needed between the two products.
// LDS images: K rows of DH*2 bytes; DH=64: 128-B rows with the 16-B chunk position XOR ((key>>1)&7); DH=80 (ViT-H/14):
// rows padded to 176 B = 11 chunks, 11 is odd so 16 consecutive rows hit 16 distinct 16-B slots without a swizzle.
// V^T has DV = DH rounded up to 32 rows (rows >= DH are zero: the third 32-row output block of DH=80 is half padding).
// RECOMP: S^T blocks are computed twice (pass 1: row max only, pass 2: exp + PV) instead of being kept in NKB*16
// registers, for configurations where one query block per wave and many waves per workgroup pay.
// =============================================================================================
// TIMER (CLIPX_ATTN_DBG=9, tools/attn_bench): per-wave shader-cycle totals of staging / S + max / exp + PV / store
#ifdef CLIPX_ABLATE
__device__ long long g_attn_phase[8192 * 4];  // tools build: what the TIMER form leaves for clipx_dbg_attn_phase
#endif
// RAGGED (not causal, offs / lens given): a sample shorter than the launch's NKB - 1 blocks has padding keys in EVERY block from
// its own last one on, so the key < T mask runs in all of them -- the plain form masks the last block only, and the zeroed K rows
// of the blocks in between would sit in the softmax at logit 0.  (The causal form masks every block as it is.)
// Waves per SIMD the register budget is sized for: two workgroups per CU up to 9 key blocks; beyond that (tools build: the 19-block
// yardstick) the LDS holds one.  The wide heads (88, 104) say what their LDS allows: at 9 key blocks their images take 113 and
// 141 KiB, one workgroup per CU, and a budget for two would be a budget for an occupancy that cannot happen.
template <int DH, int NKB, int NW>
constexpr int attn_waves_per_simd() {
  return (NKB > 9 || (attn_wide_head(DH) && 2 * attn_image_bytes(DH, NKB) > ATTN_LDS_LIMIT)) ? (NW + 3) / 4 : (2 * NW + 3) / 4;
}
// Head dimensions 88 and 104 (DH % 16 == 8; ViT-g/14, ViT-bigG/14): QK^T takes KS = ceil(DH / 16) k-steps and the last is a HALF
// step -- lane half hb = 0 holds the real columns DH - 8 .. DH - 1, hb = 1 would hold columns DH .. DH + 7, which belong to the next
// head (or lie past the row).  Both operands are exactly zero there: the Q fragment is replaced by zeros (and its load redirected
// to the head's own column 0, so nothing outside the head is ever read), the K rows carry one more 16-B chunk that the staging
// fills with zeros (an unwritten chunk could hold a NaN pattern, and 0 x NaN is NaN).  CH = DH / 8 is whole, so K / V staging
// moves whole chunks; V^T has DV = 96 / 128 rows, rows DH .. DV - 1 zero, and the store is masked to d < DH.
template <int DH, int NKB, int NW, int QPW, bool CAUSAL, bool RECOMP, bool TIMER = false, bool RAGGED = false>
__global__ __launch_bounds__(NW * 64, (attn_waves_per_simd<DH, NKB, NW>())) void attention_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ out, int Tin,
                                                              int H, float scale_log2e, int dbg, int q_blocks,
                                                              const int* __restrict__ offs, const int* __restrict__ lens) {
  constexpr int TP = NKB * 32;
  constexpr int CH = DH / 8;                      // 16-B chunks per key row
  constexpr int KS = (DH + 15) / 16;              // MFMA k-steps of the QK^T product (DH 88 / 104: the last one is a half step)
  constexpr bool HALF = DH % 16 != 0;             // the last k-step has real columns in lane half hb = 0 only
  static_assert(DH % 8 == 0 && (!HALF || attn_wide_head(DH)), "head dimension");
  static_assert(!HALF || (!CAUSAL && !RAGGED), "head dimensions 88 and 104: not causal, not ragged");
  constexpr int KROW = (int)attn_krow_bytes(DH);  // bytes per K row in LDS (clipx_attn_plan.h)
  static_assert(KROW >= 2 * KS * 16, "every chunk a k-step reads lies inside the row");
  constexpr int DV = (int)attn_dv(DH), NB = DV / 32;
  constexpr int VT_STRIDE = TP * 2 + 8;  // bytes per V^T row: odd multiple of 8 -> conflict-free ds_read_b64
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sK = smem;                 // [TP][KROW]
  unsigned char* sVt = smem + TP * KROW;    // [DV][VT_STRIDE]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int hb = lane >> 5, l31 = lane & 31;
  long long tph[4] = {0, 0, 0, 0};
  long long tst = TIMER ? (long long)__builtin_readcyclecounter() : 0;
#define A_STAMP(i) if (TIMER) { const long long n_ = (long long)__builtin_readcyclecounter(); tph[i] += n_ - tst; tst = n_; }
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int ld = 3 * H * DH;  // qkv row stride (elements)
  // ragged batches (the causal text tower: rows past a caption's EOT are never read): sample b owns rows offs[b] .. + lens[b]
  const int T = lens ? lens[b] : Tin;
  const size_t row0 = offs ? (size_t)offs[b] : (size_t)b * Tin;
  const bf16* qbase = qkv + row0 * ld + h * DH;
  const bf16* kbase = qbase + H * DH;
  const bf16* vbase = qbase + 2 * H * DH;
  auto kchunk = [](int key, int c) -> int { return DH == 64 ? (c ^ ((key >> 1) & 7)) : c; };

  // ---- Q fragments of every query block of this wave, requested before the K/V staging so that their HBM
  // latency hides under it (B operand: lane (q = l31, hb) holds Q[q][16s + 8hb .. +8])
  bf16x8 qf_all[QPW][KS];
#pragma unroll
  for (int qi = 0; qi < QPW; ++qi) {
    const int qpos = (qi * NW + w) * 32 + l31;  // query blocks are dealt round-robin to the waves
    const int qrow = qpos < T ? qpos : T - 1;  // padded query rows compute on a valid row and are never stored
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      if constexpr (HALF) {
        // the half step: columns 16 s + 8 hb .. + 8 exist for hb = 0 only -- hb = 1 reads the head's own column 0 and holds zeros
        const bool real = s < KS - 1 || hb == 0;
        uint4 v = *reinterpret_cast<const uint4*>(qbase + (size_t)qrow * ld + (real ? 16 * s + 8 * hb : 0));
        if (!real) v = make_uint4(0u, 0u, 0u, 0u);
        qf_all[qi][s] = *reinterpret_cast<const bf16x8*>(&v);
      } else {
        const uint4 v = *reinterpret_cast<const uint4*>(qbase + (size_t)qrow * ld + 16 * s + 8 * hb);
        qf_all[qi][s] = *reinterpret_cast<const bf16x8*>(&v);
      }
    }
  }

  if (dbg != 2) {  // ablation 2: no staging (garbage results)
  // ---- stage K: CH lanes cover one key's row.  Loads are unconditional (row clamped, zeroed after) and issued as
  // one batch: a per-element `if (key < T) load` makes hipcc branch around every load and drain vmcnt(0) each time.
  {
    constexpr int KIT = (TP * CH + NW * 64 - 1) / (NW * 64);
    uint4 kv[KIT];
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
      const int i = tid + it * NW * 64;
      int key = i / CH;
      const int c = i - key * CH;
      key = key < T ? key : T - 1;
      kv[it] = *reinterpret_cast<const uint4*>(kbase + (size_t)key * ld + c * 8);
    }
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
      const int i = tid + it * NW * 64;
      const int key = i / CH, c = i - key * CH;
      if (i < TP * CH) {
        const uint4 v = key < T ? kv[it] : make_uint4(0u, 0u, 0u, 0u);
        *reinterpret_cast<uint4*>(sK + key * KROW + (kchunk(key, c) << 4)) = v;
      }
    }
    if constexpr (HALF) {  // chunk CH of every row: the hb = 1 half of the last k-step
      for (int key = tid; key < TP; key += NW * 64) *reinterpret_cast<uint4*>(sK + key * KROW + (CH << 4)) = make_uint4(0u, 0u, 0u, 0u);
    }
  }
  // ---- stage V transposed: a thread takes keys (2kp, 2kp+1) x 8 d and writes 8 packed key-pairs
  {
    constexpr int VIT = ((TP / 2) * CH + NW * 64 - 1) / (NW * 64);
    uint4 v0s[VIT], v1s[VIT];
#pragma unroll
    for (int it = 0; it < VIT; ++it) {
      const int i = tid + it * NW * 64;
      const int kp = i / CH, c = i - kp * CH;
      const int k0 = 2 * kp < T ? 2 * kp : T - 1, k1 = 2 * kp + 1 < T ? 2 * kp + 1 : T - 1;
      v0s[it] = *reinterpret_cast<const uint4*>(vbase + (size_t)k0 * ld + c * 8);
      v1s[it] = *reinterpret_cast<const uint4*>(vbase + (size_t)k1 * ld + c * 8);
    }
#pragma unroll
    for (int it = 0; it < VIT; ++it) {
      const int i = tid + it * NW * 64;
      const int kp = i / CH, c = i - kp * CH;
      if (i < (TP / 2) * CH) {
        const uint4 v0 = 2 * kp < T ? v0s[it] : make_uint4(0u, 0u, 0u, 0u);
        const uint4 v1 = 2 * kp + 1 < T ? v1s[it] : make_uint4(0u, 0u, 0u, 0u);
        const unsigned a0[4] = {v0.x, v0.y, v0.z, v0.w}, a1[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const unsigned lo = (a0[jj] & 0xffffu) | (a1[jj] << 16);         // d = 8c + 2jj
          const unsigned hi = (a0[jj] >> 16) | (a1[jj] & 0xffff0000u);     // d = 8c + 2jj + 1
          *reinterpret_cast<unsigned*>(sVt + (8 * c + 2 * jj) * VT_STRIDE + kp * 4) = lo;
          *reinterpret_cast<unsigned*>(sVt + (8 * c + 2 * jj + 1) * VT_STRIDE + kp * 4) = hi;
        }
      }
    }
    if (DV > DH) {  // zero rows DH .. DV-1 of V^T
      for (int i = tid; i < (DV - DH) * (TP / 2); i += NW * 64) {
        const int r = i / (TP / 2), kp = i - r * (TP / 2);
        *reinterpret_cast<unsigned*>(sVt + (DH + r) * VT_STRIDE + kp * 4) = 0u;
      }
    }
  }
  }
  __syncthreads();
  A_STAMP(0)
  if (dbg == 1) return;  // ablation (CLIPX_ATTN_DBG=1): staging only

  const int ksw = (l31 >> 1) & 7;
#pragma unroll
  for (int qi = 0; qi < QPW; ++qi) {
    const int qb = qi * NW + w;
    if (qb >= q_blocks) break;  // q_blocks = NKB, or 1 when only the rows of query block 0 are read afterwards (last block, token 0)
    const int qpos = qb * 32 + l31;
    bf16x8 qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = qf_all[qi][s];
    // ---- S^T blocks; causal rows never look right of the diagonal block (wave-uniform skip)
    auto s_block = [&](int kb) -> f32x16 {
      f32x16 sb;
#pragma unroll
      for (int r = 0; r < 16; ++r) sb[r] = 0.f;
      if (!CAUSAL || kb <= qb) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const int c = 2 * s + hb;
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + (kb * 32 + l31) * KROW + ((DH == 64 ? (c ^ ksw) : c) << 4));
          sb = attn_mfma(kf, qf[s], sb);
        }
      }
      // masking is needed only in the last key block (padding past T) and, for causal, on/after the diagonal
      if (kb == NKB - 1 || CAUSAL || RAGGED) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hb;
          const bool ok = key < T && (!CAUSAL || key <= qpos);
          sb[r] = ok ? sb[r] : -INFINITY;
        }
      }
      return sb;
    };
    f32x16 sacc[RECOMP ? 1 : NKB];
    float mx = -INFINITY;
#pragma unroll(RECOMP ? 1 : NKB)
    for (int kb = 0; kb < NKB; ++kb) {
      const f32x16 sb = s_block(kb);
      if (!RECOMP) sacc[kb] = sb;
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sb[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    if (mx == -INFINITY) mx = 0.f;  // padded query rows
    const float nmx = -mx * scale_log2e;
    if (TIMER) { asm volatile("" : "+v"(mx)); A_STAMP(1) }

    // ---- per key block: P = exp2(S*c - m*c) -> bf16 (stays in registers as the B operand), then O^T += V^T P^T
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    f32x2_t sum2 = {0.f, 0.f};
    const int tail_keys = T - (NKB - 1) * 32;  // keys of the last key block that exist
    f32x16 oacc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[nb][r] = 0.f;
#pragma unroll(RECOMP ? 1 : NKB)
    for (int kb = 0; kb < NKB; ++kb) {
      if (CAUSAL && kb > qb) continue;
      bf16x8 pf[2];
      const f32x16 sb = RECOMP ? s_block(kb) : sacc[RECOMP ? 0 : kb];
      // pairs go through one v_cvt_pk_bf16_f32 (element-wise casts make hipcc convert singly and re-pack with v_perm)
      unsigned pw[8];
      // the scale-and-shift and the row sum run two values per instruction (v_pk_fma_f32 / v_pk_add_f32); in the last key
      // block only the first `tail_keys` keys exist (ViT-L/14: 1 of 32): when they all sit in the first register quad
      // the other 12 exponentials of the block are skipped (their P is exactly 0)
      const bool short_tail = !CAUSAL && kb == NKB - 1 && tail_keys <= 4;
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
    if (TIMER) { asm volatile("" : "+v"(oacc[0]), "+v"(oacc[NB - 1])); A_STAMP(2) }
    // ---- store: lane owns query qpos, d = 32nb + 8g + 4hb + {0..3}
    if (qpos < T) {
      bf16* orow = out + (row0 + qpos) * (H * DH) + h * DH;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          if (32 * nb + 8 * g >= DH) continue;  // padded d of the last block (compile time)
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (bf16)(oacc[nb][4 * g + e] * inv);
          *reinterpret_cast<bf16x4*>(orow + 32 * nb + 8 * g + 4 * hb) = o;
        }
    }
    A_STAMP(3)
  }
#ifdef CLIPX_ABLATE
  if (TIMER && lane == 0 && blockIdx.x * NW + w < 8192) {
#pragma unroll
    for (int i = 0; i < 4; ++i) g_attn_phase[(blockIdx.x * NW + w) * 4 + i] = tph[i];
  }
#endif
#undef A_STAMP
}

#ifdef CLIPX_ABLATE
extern "C" int clipx_dbg_attn_phase(long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_attn_phase), (size_t)n * sizeof(long long));
}
#endif

template <int DH, int NKB, int NW, int QPW, bool RECOMP = false>
static hipError_t launch_attention_cfg(const bf16* qkv, bf16* out, int B, int T, int H, int causal, hipStream_t st, int q_blocks,
                                       const int* offs = nullptr, const int* lens = nullptr, const clipx::AttnPlan* plan = nullptr) {
  q_blocks = q_blocks > 0 && q_blocks < NKB ? q_blocks : NKB;
  const size_t smem = attn_image_bytes(DH, NKB);
  // the rows of the product's dispatch pass the plan (clipx_attn_plan.h): the instantiation launched must be the one it names, so
  // the table the CPU check walks cannot drift from this switch unnoticed (the A/B configurations of the tools build pass none)
  if (plan && (plan->kernel != clipx::ATTN_BLOCK || plan->nkb != NKB || plan->nw != NW || plan->qpw != QPW || plan->recomp != RECOMP ||
               plan->lds_bytes != smem))
    return hipErrorInvalidValue;
  const float scale_log2e = (1.f / sqrtf((float)DH)) * 1.4426950408889634f;
  const dim3 grid(B * H), block(NW * 64);
#ifdef CLIPX_ABLATE
  static const int dbg = getenv("CLIPX_ATTN_DBG") ? atoi(getenv("CLIPX_ATTN_DBG")) : 0;  // ablations (tools build only), see the kernel
#else
  constexpr int dbg = 0;
#endif
  if (causal) {
    if constexpr (!attn_wide_head(DH)) {
      auto kern = attention_kernel<DH, NKB, NW, QPW, true, RECOMP>;
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(kern, grid, block, smem, st, qkv, out, T, H, scale_log2e, dbg, q_blocks, offs, lens);
    } else {
      return hipErrorInvalidValue;  // head dimensions 88 and 104 have no causal form
    }
  } else if (lens) {
    // a ragged batch that is not causal: the form that masks the padding keys of every block (the rows launch_attention gives
    // offs / lens to; the encoder's own ragged batches are the causal text tower's)
    if constexpr (DH == 64 && NKB <= 4 && !RECOMP) {
      auto kern = attention_kernel<DH, NKB, NW, QPW, false, RECOMP, false, true>;
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(kern, grid, block, smem, st, qkv, out, T, H, scale_log2e, dbg, q_blocks, offs, lens);
    } else {
      return hipErrorInvalidValue;
    }
  } else {
    auto kern = attention_kernel<DH, NKB, NW, QPW, false, RECOMP>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, block, smem, st, qkv, out, T, H, scale_log2e, dbg, q_blocks, offs, lens);
  }
  return hipGetLastError();
}

// the rows of the head dimensions other than 64 (80, 88, 104): up to three key blocks one wave each, nine key blocks on nine waves
// with S^T computed twice
template <int DH>
static hipError_t launch_attention_odd(const bf16* qkv, bf16* out, int B, int T, int H, int causal, hipStream_t st, int q_blocks,
                                       const clipx::AttnPlan& plan) {
  switch (plan.nkb) {
    case 1: return launch_attention_cfg<DH, 1, 1, 1>(qkv, out, B, T, H, causal, st, q_blocks, nullptr, nullptr, &plan);
    case 2: return launch_attention_cfg<DH, 2, 2, 1>(qkv, out, B, T, H, causal, st, q_blocks, nullptr, nullptr, &plan);
    case 3: return launch_attention_cfg<DH, 3, 3, 1>(qkv, out, B, T, H, causal, st, q_blocks, nullptr, nullptr, &plan);
    case 9: return launch_attention_cfg<DH, 9, 9, 1, true>(qkv, out, B, T, H, causal, st, q_blocks, nullptr, nullptr, &plan);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_attention(const bf16* qkv, bf16* out, int B, int T, int H, int dh, int causal, hipStream_t st, int q_blocks,
                            const int* offs, const int* lens) {
  if (B <= 0) return hipSuccess;
  if ((offs != nullptr) != (lens != nullptr)) return hipErrorInvalidValue;
  if (offs && (dh != 64 || (T + 31) / 32 > 4)) return hipErrorInvalidValue;  // ragged batches: the short-sequence configurations only
  const int nkb = (T + 31) / 32;
  // which kernel, how many key blocks and how much LDS: clipx_attn_plan.h (checked on the CPU by tools/attn_plan_check.cpp); the
  // switches below hold the template instantiations of its T <= 288 rows
  const clipx::AttnPlan plan = clipx::attn_plan(T, dh, causal);
  if (plan.kernel == clipx::ATTN_NONE) return hipErrorInvalidValue;  // causal or dh 80 above 288 tokens, anything above 608
  if (plan.kernel == clipx::ATTN_LONG) {  // ViT-L/14@336px image (T = 577)
    if (offs) return hipErrorInvalidValue;
#ifdef CLIPX_ABLATE
    // tools build, CLIPX_ATTN_CFG=19: the yardstick -- attention_kernel's RECOMP form at 19 key blocks (S^T computed twice, no
    // running softmax), ten waves of two query blocks: the cross-check and the time the long-sequence kernel has to beat
    // (read at every launch, not once: tools/attn_bench alternates the two kernels inside one process)
    const int cfg19 = getenv("CLIPX_ATTN_CFG") ? atoi(getenv("CLIPX_ATTN_CFG")) : 0;
    if (cfg19 == 19 && nkb == 19) return launch_attention_cfg<64, 19, 10, 2, true>(qkv, out, B, T, H, 0, st, q_blocks);
#endif
    return launch_attention_long(qkv, out, B, T, H, st, q_blocks, plan);
  }
  if (dh == 80) return launch_attention_odd<80>(qkv, out, B, T, H, causal, st, q_blocks, plan);    // ViT-H/14 image tower (T = 257)
  if (dh == 88) return launch_attention_odd<88>(qkv, out, B, T, H, causal, st, q_blocks, plan);    // ViT-g/14 image tower
  if (dh == 104) return launch_attention_odd<104>(qkv, out, B, T, H, causal, st, q_blocks, plan);  // ViT-bigG/14 image tower
  if (dh != 64) return hipErrorInvalidValue;
  switch (nkb) {
    case 1: return launch_attention_cfg<64, 1, 1, 1>(qkv, out, B, T, H, causal, st, q_blocks, offs, lens, &plan);
    case 2: return launch_attention_cfg<64, 2, 2, 1>(qkv, out, B, T, H, causal, st, q_blocks, offs, lens, &plan);   // ViT-B/32 image (T=50)
    case 3: return launch_attention_cfg<64, 3, 3, 1>(qkv, out, B, T, H, causal, st, q_blocks, offs, lens, &plan);   // text (T=77)
    case 4: return launch_attention_cfg<64, 4, 4, 1>(qkv, out, B, T, H, causal, st, q_blocks, offs, lens, &plan);
    case 5: return launch_attention_cfg<64, 5, 3, 2>(qkv, out, B, T, H, causal, st, q_blocks, nullptr, nullptr, &plan);
    case 6: return launch_attention_cfg<64, 6, 3, 2>(qkv, out, B, T, H, causal, st, q_blocks, nullptr, nullptr, &plan);
    case 7: return launch_attention_cfg<64, 7, 4, 2>(qkv, out, B, T, H, causal, st, q_blocks, nullptr, nullptr, &plan);   // ViT-B/16 image (T=197)
    case 8: return launch_attention_cfg<64, 8, 4, 2>(qkv, out, B, T, H, causal, st, q_blocks, nullptr, nullptr, &plan);
    case 9: {  // ViT-L/14 image (T=257)
#ifdef CLIPX_ABLATE
      // tools build: the A/B configurations of tools/attn_bench (no plan: they are not the product's dispatch)
      static const int cfg = getenv("CLIPX_ATTN_CFG") ? atoi(getenv("CLIPX_ATTN_CFG")) : 0;
      if (cfg == 4) return launch_attention_cfg<64, 9, 4, 3>(qkv, out, B, T, H, causal, st, q_blocks);
      if (cfg == 5) return launch_attention_cfg<64, 9, 9, 1, true>(qkv, out, B, T, H, causal, st, q_blocks);   // 9 waves, S recomputed
      if (cfg == 6) return launch_attention_cfg<64, 9, 5, 2>(qkv, out, B, T, H, causal, st, q_blocks);
      if (cfg == 7) return launch_attention_cfg<64, 9, 9, 1>(qkv, out, B, T, H, causal, st, q_blocks);         // 9 waves, S kept (144 regs)
      if (cfg == 8) return launch_attention_cfg<64, 9, 5, 2, true>(qkv, out, B, T, H, causal, st, q_blocks);
      if (cfg == 9 && !causal) {  // phase timer
        constexpr int KROW = 128, DV = 64;
        const size_t smem = (size_t)9 * 32 * KROW + (size_t)DV * (9 * 64 + 8);
        auto kern = attention_kernel<64, 9, 3, 3, false, false, true>;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(B * H), dim3(192), smem, st, qkv, out, T, H, (1.f / 8.f) * 1.4426950408889634f, 0, 9, (const int*)nullptr, (const int*)nullptr);
        return hipGetLastError();
      }
      if (cfg == 10 && !causal) return launch_attention_cfg<64, 9, 3, 3>(qkv, out, B, T, H, causal, st, q_blocks);  // the one-head-per-workgroup kernel (A/B)
#endif
      if (causal) return launch_attention_cfg<64, 9, 3, 3>(qkv, out, B, T, H, causal, st, q_blocks, nullptr, nullptr, &plan);
      if (plan.kernel != clipx::ATTN_PK9) return hipErrorInvalidValue;
      return launch_attention_pk9(qkv, out, B, T, H, st, q_blocks, plan.lds_bytes);
    }
    default: return hipErrorInvalidValue;
  }
}

}  // namespace clipx
