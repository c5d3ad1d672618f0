// gemm128.hip -- the 128x128 GEMM of the CLIP encoder forward (gfx950), its split-K reduction and their launcher.
//
// The linear layers inside `model.encode_image` / `model.encode_text` of the reference (clip_retrieval/clip_inference/mapper.py:57,65)
// that gemm_launch.hip does not hand to a persistent 256x256 kernel: ragged rows, the peeled m-tiles, the B = 1 queries, and the
// variants 0 / 1 the tests use as the reference.  Numerics: bf16 / fp16 MFMA operands, fp32 accumulation.
//
// HBM layouts
//   activations  x    f32  [B*T, d]   residual stream (row = b*T + t)
//                xn   bf16 [B*T, d]   LayerNorm output = GEMM operand
//                qkv  bf16 [B*T, 3d]  (q | k | v, each [H][64])
//                h    bf16 [B*T, mlp]
//   weights      W    bf16 [N, K]     torch nn.Linear layout ("B^T"): both GEMM operands are K-contiguous
//
// GEMM: out[m, n] = sum_k A[m,k] W[n,k].  128x128x64 tiles (G_TM, G_TN, G_BK: clipx_gemm_plan.h), 4 waves (2x2),
// v_mfma_f32_16x16x32 with the WEIGHT rows as the MFMA A operand and the activation rows as the B operand, so a lane's accumulator
// holds four consecutive n of one m: epilogue stores are 8 B (bf16) / 16 B (f32) instead of 2-byte scatters.
// LDS image per operand: [128 rows][8 chunks of 16 B], chunk position XOR ((row>>1)&7): ds_read_b128 fragment
// reads of 16 rows at one k-chunk hit 16 distinct 16-B slots of the 256-B bank row (conflict-free).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gemm_common.h"

namespace clipx {

constexpr int G_STAGE_BYTES = (G_TM + G_TN) * G_BK * 2;  // 32 KiB
constexpr int G_GROUP_M = 8;

// DEEP (GLDS only): 4-deep LDS ring (128 KiB, one workgroup per CU), the DMA of K-tile t+4 issued at K-tile t's barrier, ONE
// barrier per K-tile, software-pipelined fragment reads.  The launches this kernel serves have few workgroups (the peeled
// 257th m-tile of ViT-L/14: 16..64 workgroups; B = 1 queries), so nothing else runs on the CU to hide DMA or LDS latency.
template <int EPI, bool GLDS, bool DEEP = false, bool F16 = false>  // F16: operands are IEEE fp16 (bits travel as "bf16" pointers)
__global__ __launch_bounds__(256, 2) void gemm_bf16_kernel(const bf16* __restrict__ A, const bf16* __restrict__ W,
                                                          const float* __restrict__ bias, void* __restrict__ outp,
                                                          const float* __restrict__ table, int T, int M, int N,
                                                          int K, int row0, const float* __restrict__ rowscale,
                                                          bf16* __restrict__ out16, int kz, StampSlot* stamp) {
  stamp_start(stamp, blockIdx.x + blockIdx.y * gridDim.x);
  // kz > 0 (EPI_RAW_F32, DEEP only): split-K -- workgroup column blockIdx.y multiplies K-tiles [y * kz, (y + 1) * kz) and
  // writes its raw accumulators to outp + y * M * N
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int wn = w & 1, wm = w >> 1;
  const int hb = lane >> 5, l31 = lane & 31;

  // ---- block -> tile: XCD-contiguous runs (block b executes on XCD b%8), grouped 8 m-tiles x all n-tiles
  const int ntm = (M + G_TM - 1) / G_TM, ntn = N / G_TN;
  const int nblk = ntm * ntn;
  const int q8 = nblk >> 3, r8 = nblk & 7;
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  const int per_group = G_GROUP_M * ntn;
  const int grp = logical / per_group, within = logical - grp * per_group;
  const int gm0 = grp * G_GROUP_M;
  const int gsz = (ntm - gm0) < G_GROUP_M ? (ntm - gm0) : G_GROUP_M;
  const int tm = gm0 + within % gsz, tn = within / gsz;
  const int m0 = tm * G_TM, n0 = tn * G_TN;

  // ---- staging map: wave w fills rows [32w, 32w+32) of both operand tiles, 8 rows (1 KiB) per instruction
  const bf16* gW[4];
  const bf16* gA[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (w * 4 + i) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((row >> 1) & 7);
    int am = m0 + row;
    am = am < M ? am : M - 1;
    gW[i] = W + (size_t)(n0 + row) * K + c * 8;
    gA[i] = A + (size_t)am * K + c * 8;
  }
  const int stage_off = (w * 4) * 1024;  // + i*1024 (+ lane*16)

  // ---- fragment read offsets (bytes inside an operand tile), one per 32-deep slab of the BK=64 K-tile (gemm_common.h): row l15 of a
  // 16-row half-block (+ 2 KiB per half), k-chunk 4 s + q4 of slab s.
  // (foff / fW / fA / F0 / F1 are what is left of the deleted 32x32x16 form and are never read.  They stay: without them hipcc
  // numbers the scalar registers of the DEEP kernels differently, and this file's kernels are kept instruction for instruction.)
  int foff[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) foff[kk] = l31 * 128 + (((2 * kk + hb) ^ ((l31 >> 1) & 7)) << 4);
  const int l15 = lane & 15, q4 = lane >> 4;
  int foff16[2];
#pragma unroll
  for (int sl = 0; sl < 2; ++sl) foff16[sl] = l15 * 128 + (((4 * sl + q4) ^ ((l15 >> 1) & 7)) << 4);

  f32x4 acc[2][2][4];  // [weight block i][activation block j][quad g]: one 16 x 16 MFMA block each (gemm_common.h)
#define G_ACC(i, j, g, e) acc[i][j][g][e]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[i][j][g] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = kz > 0 ? kz : K / G_BK;
  const int t0 = kz > 0 ? (int)blockIdx.y * kz : 0;  // first K-tile of this workgroup
  if (EPI == EPI_RAW_F32) outp = reinterpret_cast<float*>(outp) + (size_t)blockIdx.y * M * N;

  auto compute = [&](int buf) {
    const unsigned char* sW = smem + buf * G_STAGE_BYTES + (wn * 64) * 128;
    const unsigned char* sA = smem + buf * G_STAGE_BYTES + G_TN * G_BK * 2 + (wm * 64) * 128;
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
      frag_t wf[2][2], af[2][2];  // [32-row block][16-row half]
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          wf[i][hf] = *reinterpret_cast<const frag_t*>(sW + (i * 32 + hf * 16) * 128 + foff16[sl]);
          af[i][hf] = *reinterpret_cast<const frag_t*>(sA + (i * 32 + hf * 16) * 128 + foff16[sl]);
        }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) mfma_block16<F16>(acc[i][j], wf[i][0], wf[i][1], af[j][0], af[j][1]);
    }
  };

  if (GLDS) {
    auto issue = [&](int t, int buf) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned char* dW = smem + buf * G_STAGE_BYTES + stage_off + i * 1024;
        unsigned char* dA = dW + G_TN * G_BK * 2;
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)(gW[i] + (size_t)t * G_BK), (lds_ptr_t)dW, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)(gA[i] + (size_t)t * G_BK), (lds_ptr_t)dA, 16, 0, 0);
      }
    };
    if (DEEP) {
      // Software-pipelined loop (same scheme as gemm256sp.hip): 4-slot LDS ring, K-tile t+4 is staged right behind the
      // barrier of K-tile t (the slot K-tile t just released), fragments of the next k-step are read (inline-asm
      // ds_read_b128, counted lgkmcnt) while this k-step's 4 MFMAs run, and the one barrier of the K-tile sits before
      // the last k-step's MFMAs with the next K-tile's first fragments read right behind it.  With one wave per SIMD
      // nothing else covers LDS latency: the previous loop (4 reads; lgkmcnt(0); 4 MFMAs, four times per K-tile) took
      // ~1 us per K-tile, this one ~0.35 us.  Needs M * K * 2 and N * K * 2 < 4 GiB (32-bit lane offsets).
      typedef int i32x4 __attribute__((ext_vector_type(4)));
      const int wu = __builtin_amdgcn_readfirstlane(w);
      const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
      const unsigned lds_base = __builtin_amdgcn_readfirstlane(lds0);
      unsigned offW[4], offA[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        offW[i] = (unsigned)(reinterpret_cast<const char*>(gW[i]) - reinterpret_cast<const char*>(W));
        offA[i] = (unsigned)(reinterpret_cast<const char*>(gA[i]) - reinterpret_cast<const char*>(A));
      }
      unsigned fW[4], fA[4];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        fW[kk] = lds0 + (wn * 64) * 128 + foff[kk];
        fA[kk] = lds0 + G_TN * G_BK * 2 + (wm * 64) * 128 + foff[kk];
      }
      i32x4 F0[4], F1[4];
      (void)F0; (void)F1;
#define D_DSREAD(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(off))
      // A K-tile is four units u = 2 * slab + (activation half): unit (sl, ha) multiplies the slab's four weight fragments
      // Wd[sl][2 i + j2] with the two activation fragments Ad[u & 1][j] of half ha -- 8 MFMAs of 16 cycles.
      // fragment read addresses of ring slot 0 (+ 32 KiB per slot): W rows wn*64 + .., A rows wm*64 + ..
      unsigned fW16[2], fA16[2];
#pragma unroll
      for (int sl = 0; sl < 2; ++sl) {
        fW16[sl] = lds0 + (wn * 64) * 128 + foff16[sl];
        fA16[sl] = lds0 + G_TN * G_BK * 2 + (wm * 64) * 128 + foff16[sl];
      }
      i32x4 Wd[2][4], Ad[2][2];
#define D_READ_W(sl, so)                                 \
  D_DSREAD(Wd[sl][0], fW16[sl] + (so), 0);               \
  D_DSREAD(Wd[sl][1], fW16[sl] + (so), 2048);            \
  D_DSREAD(Wd[sl][2], fW16[sl] + (so), 4096);            \
  D_DSREAD(Wd[sl][3], fW16[sl] + (so), 6144);
#define D_READ_A(u, so)                                                \
  D_DSREAD(Ad[(u) & 1][0], fA16[(u) >> 1] + (so), ((u) & 1) * 2048);     \
  D_DSREAD(Ad[(u) & 1][1], fA16[(u) >> 1] + (so), 4096 + ((u) & 1) * 2048);
#define D_READ_U0(so) D_READ_W(0, so) D_READ_A(0, so) __builtin_amdgcn_sched_barrier(0);
#define D_READ_U1(so) D_READ_A(1, so) __builtin_amdgcn_sched_barrier(0);
#define D_READ_U2(so) D_READ_W(1, so) D_READ_A(2, so) __builtin_amdgcn_sched_barrier(0);
#define D_READ_U3(so) D_READ_A(3, so) __builtin_amdgcn_sched_barrier(0);
#define D_WAIT_N(n) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(n) : "memory"); __builtin_amdgcn_sched_barrier(0);
#define D_MFMA_U(u)                                                                                                  \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)                        \
      _Pragma("unroll") for (int j2 = 0; j2 < 2; ++j2)                                                               \
          acc[i][j][2 * ((u) & 1) + j2] =                                                                            \
              mfma_16x16x32<F16>(Wd[(u) >> 1][2 * i + j2], Ad[(u) & 1][j], acc[i][j][2 * ((u) & 1) + j2]);           \
  __builtin_amdgcn_sched_barrier(0);
      // one DMA: M0 = LDS address of the piece (SGPR), 32-bit lane offset, SGPR base of the K-tile
#define D_DMA(off, base, dst)                                                                                         \
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 3\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(off), "s"(base), "s"(dst) : "memory")
      auto stage = [&](int t, int slot) {
        const char* bw = reinterpret_cast<const char*>(W) + (size_t)(t0 + t) * (G_BK * 2);
        const char* ba = reinterpret_cast<const char*>(A) + (size_t)(t0 + t) * (G_BK * 2);
        const unsigned d = lds_base + slot * G_STAGE_BYTES + wu * 4096;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          D_DMA(offW[i], bw, d + i * 1024);
          D_DMA(offA[i], ba, d + G_TN * G_BK * 2 + i * 1024);
        }
        __builtin_amdgcn_sched_barrier(0);
      };
      const int npro = nk < 4 ? nk : 4;
      for (int t = 0; t < npro; ++t) stage(t, t);
      if (npro == 4) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
      else if (npro == 3) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      else if (npro == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      D_READ_U0(0u)
      unsigned so = 0;  // byte offset of the current ring slot
#define D_KT_HEAD()                                   \
  D_READ_U1(so) D_WAIT_N(2) D_MFMA_U(0)                \
  D_READ_U2(so) D_WAIT_N(6) D_MFMA_U(1)                \
  D_READ_U3(so) D_WAIT_N(2) D_MFMA_U(2)                \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  \
  __builtin_amdgcn_sched_barrier(0);
#define D_READ_FIRST(so_) D_READ_U0(so_)
#define D_MFMA_LAST() D_MFMA_U(3)
#define D_SYNC(vm)                                           \
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(vm) : "memory");  \
  __builtin_amdgcn_sched_barrier(0);                         \
  __builtin_amdgcn_s_barrier();                              \
  __builtin_amdgcn_sched_barrier(0);
      int t = 0;
      // steady state: K-tiles t+1 .. t+3 are in flight at the sync (K-tile t+1 is needed: 16 younger DMA), K-tile t+4 exists
      for (; t + 4 < nk; ++t) {
        D_KT_HEAD()
        D_SYNC(16)
        stage(t + 4, t & 3);
        so = (so + G_STAGE_BYTES) & (4 * G_STAGE_BYTES - 1);
        D_READ_FIRST(so)
        D_MFMA_LAST()
      }
      // the last (up to) four K-tiles: nothing left to stage
      for (; t < nk; ++t) {
        const int rem = nk - 1 - t;  // K-tiles after this one (all issued)
        D_KT_HEAD()
        if (rem >= 3) { D_SYNC(16) } else if (rem == 2) { D_SYNC(8) } else { D_SYNC(0) }
        so = (so + G_STAGE_BYTES) & (4 * G_STAGE_BYTES - 1);
        if (rem > 0) { D_READ_FIRST(so) }
        D_MFMA_LAST()
      }
#undef D_DSREAD
#undef D_READ_FIRST
#undef D_MFMA_LAST
#undef D_DMA
#undef D_KT_HEAD
#undef D_SYNC
    } else {
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
      if (t + 1 < nk) issue(t + 1, (t + 1) & 1);
      compute(t & 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    }
  } else {
    // register-staged fill (T14 split): global loads for tile t+1 are issued before the MFMAs of tile t
    // and written to LDS after them, so HBM/L2 latency hides under the compute
    uint4 rw0, rw1, rw2, rw3, ra0, ra1, ra2, ra3;
#define G_LOAD(t)                                                             \
  {                                                                           \
    rw0 = *reinterpret_cast<const uint4*>(gW[0] + (size_t)(t) * G_BK);        \
    rw1 = *reinterpret_cast<const uint4*>(gW[1] + (size_t)(t) * G_BK);        \
    rw2 = *reinterpret_cast<const uint4*>(gW[2] + (size_t)(t) * G_BK);        \
    rw3 = *reinterpret_cast<const uint4*>(gW[3] + (size_t)(t) * G_BK);        \
    ra0 = *reinterpret_cast<const uint4*>(gA[0] + (size_t)(t) * G_BK);        \
    ra1 = *reinterpret_cast<const uint4*>(gA[1] + (size_t)(t) * G_BK);        \
    ra2 = *reinterpret_cast<const uint4*>(gA[2] + (size_t)(t) * G_BK);        \
    ra3 = *reinterpret_cast<const uint4*>(gA[3] + (size_t)(t) * G_BK);        \
  }
#define G_STORE(buf)                                                                        \
  {                                                                                         \
    unsigned char* dW = smem + (buf) * G_STAGE_BYTES + stage_off + lane * 16;               \
    *reinterpret_cast<uint4*>(dW) = rw0;                                                    \
    *reinterpret_cast<uint4*>(dW + 1024) = rw1;                                             \
    *reinterpret_cast<uint4*>(dW + 2048) = rw2;                                             \
    *reinterpret_cast<uint4*>(dW + 3072) = rw3;                                             \
    *reinterpret_cast<uint4*>(dW + G_TN * G_BK * 2) = ra0;                                  \
    *reinterpret_cast<uint4*>(dW + G_TN * G_BK * 2 + 1024) = ra1;                           \
    *reinterpret_cast<uint4*>(dW + G_TN * G_BK * 2 + 2048) = ra2;                           \
    *reinterpret_cast<uint4*>(dW + G_TN * G_BK * 2 + 3072) = ra3;                           \
  }
    G_LOAD(0)
    G_STORE(0)
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
      if (t + 1 < nk) G_LOAD(t + 1)
      compute(t & 1);
      if (t + 1 < nk) G_STORE((t + 1) & 1)
      __syncthreads();
    }
#undef G_LOAD
#undef G_STORE
  }

  // ---- epilogue: quad g of each 32x32 sub-tile = four consecutive n of one m (gemm_common.h: quad_m / quad_n)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int m = m0 + wm * 64 + j * 32 + quad_m(g, lane);
        if (m >= M) continue;
        const int n = n0 + wn * 64 + i * 32 + quad_n(g, lane);
        const float4 v = make_float4(G_ACC(i, j, g, 0), G_ACC(i, j, g, 1), G_ACC(i, j, g, 2), G_ACC(i, j, g, 3));
        gemm_store_quad<EPI>(v, m, n, N, bias, outp, table, T, row0, rowscale, out16);
      }
    }
  }
  stamp_end(stamp, blockIdx.x + blockIdx.y * gridDim.x);
}

template <int EPI, bool F16 = false>
static hipError_t launch_gemm_epi(const GemmArgs& g, int fill, hipStream_t st) {
  const int ntm = (g.M + G_TM - 1) / G_TM, ntn = g.N / G_TN;
  const dim3 grid(ntm * ntn), block(256);
  const size_t smem = (fill == GEMM128_DMA_DEEP ? 4 : 2) * G_STAGE_BYTES;
  auto kern = fill == GEMM128_DMA_DEEP ? gemm_bf16_kernel<EPI, true, true, F16>
              : fill == GEMM128_DMA    ? gemm_bf16_kernel<EPI, true, false, F16>
                                       : gemm_bf16_kernel<EPI, false, false, F16>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  launch_with_events(g.events, kern, grid, block, smem, st, g.A, g.W, g.bias, g.out, g.table, g.T, g.M, g.N, g.K, g.row0, g.rowscale, g.out16, 0);
  return hipGetLastError();
}

// ---- split-K for small M (the B = 1 .. 2 query encodes of KnnService.compute_query, clip_back.py:207-255).  M = 257 rows
// give the 128x128 kernel 24 (N = 1024) .. 96 workgroups, each walking its whole K loop at ~0.5 us per K-tile with nothing
// else on the CU: fc2 (K = 4096) 36 us, out-proj 13 us.  Splitting K over S workgroup columns fills the chip; the S partial
// products (raw f32 accumulators) are summed in FIXED order 0 .. S-1 by a second kernel that applies the very epilogue code of
// the unsplit kernels (gemm_store_quad).  The result is deterministic but not bitwise equal to
// the unsplit sum, so the caller (clipx_encode.hip run_gemm) hands a scratch buffer only to the GEMMs of a single-sample API call: every
// call with >= 2 samples keeps the invariant "a row does not depend on the batch (or chunk) it travels in".
template <int EPI>
__device__ __forceinline__ void splitk_reduce_quad(const float* __restrict__ part, int S, int M, int N, const float* __restrict__ bias,
                                                   void* __restrict__ outp, const float* __restrict__ rowscale, bf16* __restrict__ out16) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;  // quad index
  const int nq4 = N >> 2;
  if (q >= (int64_t)M * nq4) return;
  const int m = (int)(q / nq4), n = (int)(q - (int64_t)m * nq4) * 4;
  float4 v = *reinterpret_cast<const float4*>(part + (size_t)m * N + n);
  for (int z = 1; z < S; ++z) {
    const float4 p = *reinterpret_cast<const float4*>(part + ((size_t)z * M + m) * N + n);
    v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
  }
  gemm_store_quad<EPI>(v, m, n, N, bias, outp, nullptr, 1, 0, rowscale, out16);
}
template <int EPI>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int S, int M, int N,
                                                           const float* __restrict__ bias, void* __restrict__ outp,
                                                           const float* __restrict__ rowscale, bf16* __restrict__ out16, StampSlot* stamp) {
  stamp_start(stamp, blockIdx.x);
  splitk_reduce_quad<EPI>(part, S, M, N, bias, outp, rowscale, out16);  // (threads past the last quad return from it early)
  stamp_end(stamp, blockIdx.x);
}

// (how many splits: gemm_splitk_factor, clipx_gemm_plan.h)
template <int EPI>
static hipError_t launch_splitk_epi(const GemmArgs& g, int S, hipStream_t st) {
  const int ntm = (g.M + G_TM - 1) / G_TM, ntn = g.N / G_TN;
  auto kern = g.f16 ? gemm_bf16_kernel<EPI_RAW_F32, true, true, true> : gemm_bf16_kernel<EPI_RAW_F32, true, true, false>;
  const size_t smem4 = 4 * G_STAGE_BYTES;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem4);
  if (e != hipSuccess) return e;
  launch_with_events(g.events, kern, dim3(ntm * ntn, S), dim3(256), smem4, st, g.A, g.W, nullptr, g.splitk_ws, nullptr, 1, g.M, g.N, g.K, 0,
                     nullptr, nullptr, (g.K / G_BK) / S);
  const int64_t quads = (int64_t)g.M * (g.N / 4);
  launch_with_events(g.events, splitk_reduce_kernel<EPI>, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, g.splitk_ws, S, g.M, g.N,
                     g.bias, g.out, g.rowscale, g.out16);
  return hipGetLastError();
}

hipError_t launch_gemm128(const GemmArgs& g, const GemmPlan& plan, hipStream_t st) {
  if (!plan.valid || g.M != plan.rows128 || plan.fill128 == GEMM128_NONE || (plan.splitk > 1 && !g.splitk_ws)) return hipErrorInvalidValue;
  if (plan.splitk > 1)
    return with_epilogue<EPI_BIAS_BF16, EPI_BIAS_F16, EPI_BIAS_QGELU_BF16, EPI_BIAS_GELU_BF16, EPI_BIAS_RESID_F32, EPI_BIAS_RESID_H16>(
        g.epi, [&](auto E) { return launch_splitk_epi<decltype(E)::value>(g, plan.splitk, st); });
  if (g.f16)  // fp16 operands exist for the 16-bit-output epilogues only (the LayerNorm-folded GEMMs)
    return with_out16_epilogue(g.epi, [&](auto E) { return launch_gemm_epi<decltype(E)::value, true>(g, plan.fill128, st); });
  return with_epilogue<EPI_BIAS_BF16, EPI_BIAS_F16, EPI_BIAS_QGELU_BF16, EPI_BIAS_GELU_BF16, EPI_BIAS_RESID_F32, EPI_BIAS_RESID_H16, EPI_TABLE_F32>(
      g.epi, [&](auto E) { return launch_gemm_epi<decltype(E)::value>(g, plan.fill128, st); });
}

}  // namespace clipx
