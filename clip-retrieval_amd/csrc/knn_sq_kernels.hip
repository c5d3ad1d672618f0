// knn_sq_kernels.hip -- gfx950 kernels of IVF-SQ8: faiss IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, QT_8bit,
// METRIC_INNER_PRODUCT), by_residual = false (include/knnx.h, "IVF-SQ8"; the "IVF65536,SQ8" factory string).
//
// The arena holds ONE BYTE per dimension, list-sorted and tile-padded exactly like the fp16 rows of IVF-Flat (pad rows are
// zero bytes and are never admitted).  Quantiser: vmin[d], vdiff[d]; scale = 255 / vdiff, step = vdiff / 255 derived on the
// host (0 where vdiff == 0).
//   encode   code_j = clamp((int)((f32(x_j) - vmin_j) * scale_j), 0, 255), subtract and multiply rounded separately
//   decode   dec_j  = vmin_j + (f32(code_j) + 0.5) * step_j, multiply and add rounded separately
//   score    <q, dec(row)> = b_q + sum_j u_j code_j, u = q * step, b_q = <q, vmin + step / 2>
//
// List scan (knn_sq_scan_kernel): the structure of knn_scan_kernel<.., IVF = true, QB = 1> (knn_kernels.hip) -- work items
// {tile, query mask, valid rows}, 8 waves x one 32-row tile, the LDS candidate queues and prune of knn_scan_shared.h, the
// multi-block split of ivfm_range, partial lists merged by launch_merge_u32 through idmap.  What differs is the operand
// path: a lane loads 16 code bytes (one dwordx4) per 32 columns and turns them into the half8 A operands of two MFMA k-steps
// in registers: v_perm_b32 places every byte under the exponent byte 0x64 (the half 1024 + c, exact for c <= 1023) and a
// packed subtract of 1024 leaves c -- two vector instructions per four codes, no rounding anywhere.  The 16 bytes of a lane
// are columns 32 t + 16 hb .. + 15, so k-step 2 t + e of lane half hb covers columns 32 t + 16 hb + 8 e .. + 7: the prep
// kernel lays u down in that column order and the ordinary fragment builder (launch_prep_blocks) splits it hi / lo.
// u is tiny (|q| * vdiff / 255 ~ 1e-5, below the fp16 normal range), so every query's u is scaled by a power of two that
// brings its largest component into [1024, 2048) before the split; the kernel multiplies the fp32 sum by the inverse power
// (exact) and adds b_q once, before the threshold compare.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include <math.h>
#include <algorithm>
#include "knn_kernels.h"
#include "knn_scan_shared.h"

namespace knnx {

typedef uint32_t uint4v __attribute__((ext_vector_type(4)));

// The contract fixes where every rounding falls (encode: subtract, then multiply; decode and score: multiply, then add).  hipcc
// contracts a * b + c into one fma by default, so these pin the two-rounding forms.
__device__ __forceinline__ float sq_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float sq_mul_add(float a, float b, float c) {  // c + round(a * b)
#pragma clang fp contract(off)
  const float p = a * b;
  return c + p;
}
__device__ __forceinline__ float sq_sub_mul(float a, float b, float c) {  // round(a - b) * c
#pragma clang fp contract(off)
  const float t = a - b;
  return t * c;
}

// ---------------------------------------------------------------------------------------------
// query preparation: u = q * step in the scan's column order, scaled; b_q; 1 / scale
// ---------------------------------------------------------------------------------------------
// column c of a row sits at position sq_pos(c) of the fragment builder's input: bits 3 and 4 of c swapped (see the head)
__device__ __forceinline__ int sq_pos(int c) { return (c & ~24) | ((c & 8) << 1) | ((c & 16) >> 1); }

// one 256-thread workgroup per query
__global__ __launch_bounds__(256) void sq_prep_kernel(const float* __restrict__ q, int d, const float* __restrict__ vmin,
                                                     const float* __restrict__ step, float* __restrict__ u,
                                                     float* __restrict__ bq, float* __restrict__ inv) {
  __shared__ float s_max[4];
  __shared__ double s_sum[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* qn = q + (size_t)n * d;
  float mx = 0.f;
  double sum = 0.0;
  for (int c = tid; c < d; c += 256) {
    const float uc = sq_mul(qn[c], step[c]);
    mx = fmaxf(mx, fabsf(uc));
    sum += (double)qn[c] * ((double)vmin[c] + 0.5 * (double)step[c]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, o));
    sum += __shfl_xor(sum, o);
  }
  if ((tid & 63) == 0) { s_max[tid >> 6] = mx; s_sum[tid >> 6] = sum; }
  __syncthreads();
  mx = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
  sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
  // 2^sh * max |u| in [1024, 2048); a query whose u is all zero (or not finite) is left alone
  int sh = 0;
  if (mx > 0.f && mx < INFINITY) sh = 10 - ilogbf(mx);
  sh = sh < -100 ? -100 : (sh > 100 ? 100 : sh);
  for (int c = tid; c < d; c += 256) u[(size_t)n * d + sq_pos(c)] = ldexpf(sq_mul(qn[c], step[c]), sh);
  if (tid == 0) {
    bq[n] = (float)sum;
    inv[n] = ldexpf(1.f, -sh);
  }
}

// ---------------------------------------------------------------------------------------------
// the list scan
// ---------------------------------------------------------------------------------------------
// 8 code bytes (two dwords) -> the half8 A operand of one k-step, exactly
__device__ __forceinline__ half8 sq_codes_half8(uint32_t w0, uint32_t w1) {
  uint4v r;
  r[0] = __builtin_amdgcn_perm(0x64646464u, w0, 0x04010400u);  // halves 0x6400 | byte 0, 0x6400 | byte 1
  r[1] = __builtin_amdgcn_perm(0x64646464u, w0, 0x04030402u);
  r[2] = __builtin_amdgcn_perm(0x64646464u, w1, 0x04010400u);
  r[3] = __builtin_amdgcn_perm(0x64646464u, w1, 0x04030402u);
  half8 h = __builtin_bit_cast(half8, r);
  const _Float16 k1024 = (_Float16)1024.f;
  return h - k1024;  // v_pk_add_f16: (1024 + c) - 1024 = c
}

// D = row width in bytes (= columns); LD = dwordx4 loads of one burst (32 LD columns); D / (32 LD) bursts per tile
//
// RANGE = true is the threshold mode (range_search and k > 64 on an index with the threshold-scan switch on): the same work lists,
// operand path, bursts, MFMA order and score arithmetic -- a (query, row) score is the same fp32 value in both modes -- but no
// candidate queues, no prune, no partial lists: the LDS holds the u fragments only (128 D bytes) and the tile loop has no barrier.
// Query NQ blk + q of the pass has the threshold rthr[NQ blk + q]; a valid row of a tile whose mask has the query's bit is a hit when
// score > threshold (strict).  A lane owns 16 rows of ONE query: it counts its hits, takes that many slots of the query's slice
// [rcap] of hit_s / hit_i with ONE atomicAdd on rcnt[NQ blk + q] and writes (score, arena row) while below rcap -- the counter stays
// exact when the slice overflows (the host regrows the pools and scans again).  A threshold of +INFINITY marks a finished query; a
// workgroup whose block has only finished queries returns before it stages the fragments.
template <int D, int LD, bool RANGE>
__device__ __forceinline__ void sq_scan_body(
    unsigned char* smem_raw, const uint8_t* __restrict__ X, const _Float16* __restrict__ qfrag, const float* __restrict__ bq_g,
    const float* __restrict__ inv_g, int nq, int k, int cap, int* __restrict__ thr_g, float* __restrict__ part_s,
    uint32_t* __restrict__ part_i, int* __restrict__ part_n, const uint4* __restrict__ work,
    const unsigned* __restrict__ nwork_ptr, int nblk, unsigned work_stride, const float* __restrict__ rthr,
    unsigned* __restrict__ rcnt, unsigned rcap, float* __restrict__ hit_s, uint32_t* __restrict__ hit_i) {
  constexpr int NQ = 32;
  constexpr int KS = D / 16;
  constexpr int NB = D / (32 * LD);  // bursts per tile
  static_assert(D % (32 * LD) == 0, "whole bursts");
  ScanSmem sm{};
  if constexpr (RANGE) sm.qf = reinterpret_cast<half8*>(smem_raw);
  else sm = carve(smem_raw, D, cap, NQ);

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int q = lane & 31, hb = lane >> 5;

  // which query block this workgroup serves, and as which of that block's workgroups (knn_scan_kernel, IVF && MODE 0)
  int blk = 0, bidx = (int)blockIdx.x, bgrid = (int)gridDim.x;
  const size_t slot = blockIdx.x;
  if (nblk > 1) {
    const int g = (int)blockIdx.x, G = (int)gridDim.x;
    bgrid = 0;
    for (int b = 0; b < nblk; ++b) {
      int s_, e_;
      ivfm_range(nwork_ptr, nblk, G, b, s_, e_);
      if (g >= s_ && g < e_) { blk = b; bidx = g - s_; bgrid = e_ - s_; }
    }
    if (bgrid == 0) return;
    qfrag += (size_t)blk * D * 64;
    nq = nq - NQ * blk < NQ ? nq - NQ * blk : NQ;
    if constexpr (!RANGE) thr_g += NQ * blk;
    work += (size_t)blk * work_stride;
    nwork_ptr += blk;
  }
  // this lane's query: the inverse of its power-of-two scale and its bias (unused where q >= nq)
  const float inv_q = q < nq ? inv_g[NQ * blk + q] : 0.f;
  const float b_q = q < nq ? bq_g[NQ * blk + q] : 0.f;
  // threshold mode: this lane's threshold (queries past nq never hit) and the first entry of its slice of the pools (the launcher
  // checks that the pools' queries x rcap entries are indexed by 32 bits)
  float thr_q = INFINITY;
  unsigned slice_q = 0;
  if constexpr (RANGE) {
    if (q < nq) thr_q = rthr[NQ * blk + q];
    slice_q = (unsigned)(NQ * blk + q) * rcap;
    // (every wave holds all 32 queries of the block: the vote is the same in all 8, so the whole workgroup leaves or stays)
    if (__ballot(thr_q < INFINITY) == 0ull) return;
  }

  {
    const uint4* src = reinterpret_cast<const uint4*>(qfrag);
    uint4* dst = reinterpret_cast<uint4*>(sm.qf);
    for (int i = tid; i < KS * 2 * 64; i += KNN_WG) dst[i] = src[i];
    if constexpr (!RANGE) {
      if (tid < NQ) { sm.cnt[tid] = 0; sm.thr[tid] = enc_f(-INFINITY); }
      if (tid < 4) sm.flag[tid] = 0;
    }
  }
  __syncthreads();

  const int64_t ntile = (int64_t)*nwork_ptr;
  const int64_t ngroup = (ntile + KNN_WAVES - 1) / KNN_WAVES;

  uint4 a0[LD], a1[LD];
  auto item_of = [&](int64_t grp) -> uint4 {
    const int64_t idx = grp * KNN_WAVES + w;
    return (grp < ngroup && idx < ntile) ? work[idx] : make_uint4(0u, 0u, 0u, 0u);
  };
  uint4 it_cur = make_uint4(0u, 0u, 0u, 0u), it_nxt = it_cur, it_n2 = it_cur;
  // (the arena is padded to whole tiles: tile it_nxt.x is always inside it; item {0, 0, 0, 0} reads tile 0 and admits nothing)
  auto row_ptr = [&]() -> const uint4* {
    return reinterpret_cast<const uint4*>(X + ((size_t)it_nxt.x * 32 + q) * D) + hb;
  };
  auto load_burst = [&](uint4 (&buf)[LD], const uint4* xp, int c) {
#pragma unroll
    for (int j = 0; j < LD; ++j) buf[j] = xp[2 * (c * LD + j)];
    __builtin_amdgcn_sched_barrier(0);  // pin the burst (knn_scan_kernel: load_chunk)
  };

  int64_t grp = bidx;
  it_nxt = item_of(grp);
  it_n2 = item_of(grp + bgrid);
  const uint4* xp = row_ptr();
  if (grp < ngroup) load_burst(a0, xp, 0);
  int rnd = 0;

  // one group of 8 tiles.  A holds the tile's first burst on entry; the next group's first burst is in A again when NB is even, in B
  // when it is odd (the caller alternates)
  auto group = [&](uint4 (&A)[LD], uint4 (&B)[LD]) {
    const int64_t gnext = grp + bgrid;
    it_cur = it_nxt;
    it_nxt = it_n2;
    it_n2 = item_of(gnext + bgrid);
    const uint4* xnext = row_ptr();
    float16v acc_h, acc_l;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc_h[r] = 0.f; acc_l[r] = 0.f; }
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      uint4(&cur)[LD] = (c & 1) ? B : A;
      uint4(&nxt)[LD] = (c & 1) ? A : B;
      if (c + 1 < NB) load_burst(nxt, xp, c + 1);
      else load_burst(nxt, xnext, 0);
#pragma unroll
      for (int j = 0; j < LD; ++j) {
        const int s = 2 * (c * LD + j);
        const half8 x0 = sq_codes_half8(cur[j].x, cur[j].y);
        const half8 x1 = sq_codes_half8(cur[j].z, cur[j].w);
        acc_h = __builtin_amdgcn_mfma_f32_32x32x16_f16(x0, sm.qf[(s * 2 + 0) * 64 + lane], acc_h, 0, 0, 0);
        acc_l = __builtin_amdgcn_mfma_f32_32x32x16_f16(x0, sm.qf[(s * 2 + 1) * 64 + lane], acc_l, 0, 0, 0);
        acc_h = __builtin_amdgcn_mfma_f32_32x32x16_f16(x1, sm.qf[(s * 2 + 2) * 64 + lane], acc_h, 0, 0, 0);
        acc_l = __builtin_amdgcn_mfma_f32_32x32x16_f16(x1, sm.qf[(s * 2 + 3) * 64 + lane], acc_l, 0, 0, 0);
      }
    }
    xp = xnext;

    // ---- filter (knn_scan_kernel MODE 0): lane (q, hb) owns rows row0 + (r & 3) + 8 (r >> 2) of query q
    const int64_t row0 = (int64_t)it_cur.x * 32 + 4 * hb;
    const int64_t row_lim = (int64_t)it_cur.x * 32 + (int64_t)it_cur.z;
    const bool q_ok = q < nq && ((it_cur.y >> q) & 1u);
    float sc[16];
    if constexpr (RANGE) {
      unsigned hit = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = sq_mul_add(sq_mul_add(acc_l[r], KNN_LO_INV, acc_h[r]), inv_q, b_q);
        sc[r] = v;
        const int64_t row = row0 + (r & 3) + 8 * (r >> 2);
        if (v > thr_q && row < row_lim && q_ok) hit |= 1u << r;
      }
      if (hit) {
        unsigned at = atomicAdd(&rcnt[NQ * blk + q], (unsigned)__popc(hit));  // (hit != 0 implies q < nq: a query of the pass)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (hit & (1u << r)) {
            if (at < rcap) {
              hit_s[slice_q + at] = sc[r];
              hit_i[slice_q + at] = (uint32_t)(row0 + (r & 3) + 8 * (r >> 2));
            }
            ++at;
          }
        }
      }
      grp = gnext;
      ++rnd;
      return;
    }
    unsigned pend = 0;
    const float thr = dec_f(sm.thr[q]);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = sq_mul_add(sq_mul_add(acc_l[r], KNN_LO_INV, acc_h[r]), inv_q, b_q);
      sc[r] = v;
      const int64_t row = row0 + (r & 3) + 8 * (r >> 2);
      if (v >= thr && row < row_lim && q_ok) pend |= 1u << r;
    }
    const int par = rnd & 1;
    for (;;) {
      bool ovf = false;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (pend & (1u << r)) {
          const int pos = atomicAdd(&sm.cnt[q], 1);
          if (pos < cap) {
            sm.cand_s[(size_t)q * cap + pos] = sc[r];
            sm.cand_i[(size_t)q * cap + pos] = (uint32_t)(row0 + (r & 3) + 8 * (r >> 2));
            pend &= ~(1u << r);
          } else {
            ovf = true;
          }
        }
      }
      if (ovf) sm.flag[par] = 1;
      __syncthreads();  // (A) every append of this attempt has landed
      if (sm.flag[par] == 0) break;
      for (int qq = w; qq < NQ; qq += KNN_WAVES) prune_query(sm, qq, cap, k, lane, thr_g);
      __syncthreads();  // (B) queues pruned, everyone has read flag[par]
      if (tid == 0) sm.flag[par] = 0;
      __syncthreads();  // (C) flag cleared before anyone appends again
      const float thr2 = dec_f(sm.thr[q]);
      unsigned keep = 0;  // scores still at or above the raised threshold
#pragma unroll
      for (int r = 0; r < 16; ++r) keep |= sc[r] >= thr2 ? 1u << r : 0u;
      pend &= keep;
    }
    if ((rnd & 3) == 3 && w == 0 && lane < NQ) {
      const int g = __hip_atomic_load(&thr_g[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      atomicMax(&sm.thr[lane], g);
    }
    grp = gnext;
    ++rnd;
  };

  // (grp, ngroup and bgrid are the same in every wave of the workgroup: the barriers inside group() are met by all of them)
  while (grp < ngroup) {
    group(a0, a1);
    if (NB & 1) {
      if (!(grp < ngroup)) break;
      group(a1, a0);
    }
  }
  if constexpr (RANGE) return;

  __syncthreads();
  for (int qq = w; qq < NQ; qq += KNN_WAVES) prune_query(sm, qq, cap, k, lane, thr_g);
  __syncthreads();
  for (int i = tid; i < NQ * k; i += KNN_WG) {
    const int qq = i / k, j = i - qq * k;
    const int n = sm.cnt[qq];
    const size_t o = (slot * NQ + qq) * k + j;
    if (j < n) {
      part_s[o] = sm.cand_s[(size_t)qq * cap + j];
      part_i[o] = sm.cand_i[(size_t)qq * cap + j];
    }
  }
  if (tid < NQ) part_n[slot * NQ + tid] = sm.cnt[tid];
}

// the two kernels over the one body: top-k (candidate queues, partial lists) and threshold mode
template <int D, int LD>
__global__ __launch_bounds__(KNN_WG, 2) void knn_sq_scan_kernel(
    const uint8_t* __restrict__ X, const _Float16* __restrict__ qfrag, const float* __restrict__ bq_g,
    const float* __restrict__ inv_g, int nq, int k, int cap, int* __restrict__ thr_g, float* __restrict__ part_s,
    uint32_t* __restrict__ part_i, int* __restrict__ part_n, const uint4* __restrict__ work,
    const unsigned* __restrict__ nwork_ptr, int nblk, unsigned work_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  sq_scan_body<D, LD, false>(smem_raw, X, qfrag, bq_g, inv_g, nq, k, cap, thr_g, part_s, part_i, part_n, work, nwork_ptr, nblk, work_stride,
                             nullptr, nullptr, 0u, nullptr, nullptr);
}
// (d = 768 runs bursts of 6 loads, four per tile: with 8 -- three per tile, the tile body unrolled twice -- the compiler takes 222
// VGPRs, more than the 210 of the top-k form; the k-steps, and so the scores, come in the same order whatever the burst length)
constexpr int sq_range_burst(int d) { return d == 768 ? 6 : SQ_BURST; }
template <int D, int LD>
__global__ __launch_bounds__(KNN_WG, 2) void knn_sq_range_scan_kernel(
    const uint8_t* __restrict__ X, const _Float16* __restrict__ qfrag, const float* __restrict__ bq_g,
    const float* __restrict__ inv_g, int nq, const uint4* __restrict__ work, const unsigned* __restrict__ nwork_ptr, int nblk,
    unsigned work_stride, const float* __restrict__ rthr, unsigned* __restrict__ rcnt, unsigned rcap, float* __restrict__ hit_s,
    uint32_t* __restrict__ hit_i) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  sq_scan_body<D, LD, true>(smem_raw, X, qfrag, bq_g, inv_g, nq, 0, 0, nullptr, nullptr, nullptr, nullptr, work, nwork_ptr, nblk, work_stride,
                            rthr, rcnt, rcap, hit_s, hit_i);
}

// ---------------------------------------------------------------------------------------------
// encode + scatter, decode-gather, column min / max
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned sq_encode1(_Float16 x, float vmin, float scale) {
  const float t = sq_sub_mul((float)x, vmin, scale);
  return !(t >= 0.f) ? 0u : (t >= 255.f ? 255u : (unsigned)(int)t);  // (NaN -> 0)
}

// one wave per row: d code bytes into slot tile0[list] * 32 + pos of the arena (tile0 == null: slot = the row's ordinal); lays down
// idmap / inv like ivf_scatter_kernel (ids == null: row i carries id id0 + i)
__global__ __launch_bounds__(256) void sq_encode_kernel(const _Float16* __restrict__ src, int64_t n, int d,
                                                       const int32_t* __restrict__ lists, const int32_t* __restrict__ pos,
                                                       const int64_t* __restrict__ ids, int64_t id0,
                                                       const unsigned* __restrict__ tile0, int64_t id_lo, int64_t n_ids,
                                                       const float* __restrict__ vmin, const float* __restrict__ scale,
                                                       uint8_t* __restrict__ codes, int64_t* __restrict__ idmap,
                                                       uint32_t* __restrict__ inv) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const size_t drow = tile0 ? (size_t)tile0[lists[r]] * 32 + (size_t)pos[r] : (size_t)r;
  const half8* s = reinterpret_cast<const half8*>(src + (size_t)r * d);
  uint2* o = reinterpret_cast<uint2*>(codes + drow * d);
  for (int c = lane; c < d / 8; c += 64) {
    const half8 x = s[c];
    const float4 m0 = reinterpret_cast<const float4*>(vmin)[2 * c], m1 = reinterpret_cast<const float4*>(vmin)[2 * c + 1];
    const float4 s0 = reinterpret_cast<const float4*>(scale)[2 * c], s1 = reinterpret_cast<const float4*>(scale)[2 * c + 1];
    uint2 v;
    v.x = sq_encode1(x[0], m0.x, s0.x) | (sq_encode1(x[1], m0.y, s0.y) << 8) | (sq_encode1(x[2], m0.z, s0.z) << 16) |
          (sq_encode1(x[3], m0.w, s0.w) << 24);
    v.y = sq_encode1(x[4], m1.x, s1.x) | (sq_encode1(x[5], m1.y, s1.y) << 8) | (sq_encode1(x[6], m1.z, s1.z) << 16) |
          (sq_encode1(x[7], m1.w, s1.w) << 24);
    o[c] = v;
  }
  if (lane == 0 && idmap) {
    const int64_t id = ids ? ids[r] : id0 + r;
    idmap[drow] = id;
    if (id >= id_lo && id - id_lo < n_ids) inv[id - id_lo] = (uint32_t)drow;
  }
}

// out[i, :] = decode(codes[inv[ids[i] - id_lo], :]); an id outside [id_lo, id_lo + n_ids) (-1 among them) -> 0xFF bytes
__global__ __launch_bounds__(256) void sq_decode_kernel(const uint8_t* __restrict__ codes, int d, const float* __restrict__ vmin,
                                                       const float* __restrict__ step, int64_t id_lo, int64_t n_ids,
                                                       const uint32_t* __restrict__ inv, const int64_t* __restrict__ ids, int64_t n,
                                                       float* __restrict__ out) {
  const int64_t i = blockIdx.x;
  if (i >= n) return;
  const int64_t id = ids[i];
  const bool ok = id >= id_lo && id - id_lo < n_ids;
  const size_t r = ok ? inv[id - id_lo] : 0;
  for (int c = threadIdx.x; c < d; c += 256)
    out[(size_t)i * d + c] = ok ? sq_mul_add((float)codes[r * d + c] + 0.5f, step[c], vmin[c]) : __int_as_float(-1);
}

// per-column min and max of fp16 rows, order-encoded: omin / omax [d] start at enc(+inf) / enc(-inf); every workgroup folds the
// rows [64 b, 64 b + 64) of its grid-stride share and publishes one atomicMin / atomicMax per column.  d <= 1024.
__global__ __launch_bounds__(256) void sq_colminmax_kernel(const _Float16* __restrict__ X, int64_t n, int d, int* __restrict__ omin,
                                                          int* __restrict__ omax) {
  float mn[4], mx[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { mn[e] = INFINITY; mx[e] = -INFINITY; }
  for (int64_t r0 = (int64_t)blockIdx.x * 64; r0 < n; r0 += (int64_t)gridDim.x * 64) {
    const int64_t r1 = r0 + 64 < n ? r0 + 64 : n;
    for (int64_t r = r0; r < r1; ++r) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = threadIdx.x + 256 * e;
        if (c < d) {
          const float v = (float)X[(size_t)r * d + c];
          mn[e] = fminf(mn[e], v);
          mx[e] = fmaxf(mx[e], v);
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = threadIdx.x + 256 * e;
    if (c < d) {
      atomicMin(&omin[c], enc_f(mn[e]));
      atomicMax(&omax[c], enc_f(mx[e]));
    }
  }
}
__global__ void sq_minmax_init_kernel(int d, int* __restrict__ omin, int* __restrict__ omax) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < d) { omin[c] = enc_f(INFINITY); omax[c] = enc_f(-INFINITY); }
}
__global__ void sq_minmax_decode_kernel(int d, const int* __restrict__ omin, const int* __restrict__ omax, float* __restrict__ vmin,
                                        float* __restrict__ vmax) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < d) { vmin[c] = dec_f(omin[c]); vmax[c] = dec_f(omax[c]); }
}

// rows in the probed lists of every query of a multi-block pass: out[n] = sum of size[l] over the lists l whose mask
// masks[n / 32][l] has bit n % 32 (the descent of a large-k search wants it; the masks stay on the device).  One workgroup per query.
__global__ __launch_bounds__(256) void sq_probed_rows_kernel(const unsigned* __restrict__ masks, const unsigned* __restrict__ size,
                                                            int nlist, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_sum[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const unsigned* mk = masks + (size_t)(n >> 5) * nlist;
  unsigned long long sum = 0;
  for (int l = tid; l < nlist; l += 256)
    if ((mk[l] >> (n & 31)) & 1u) sum += size[l];
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if ((tid & 63) == 0) s_sum[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) out[n] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
}

// ---------------------------------------------------------------------------------------------
// launchers (declared in knn_kernels.h)
// ---------------------------------------------------------------------------------------------
hipError_t launch_sq_prep(const float* q_dev, int nq, int d, const float* vmin, const float* step, float* u, float* bq, float* inv,
                          hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(sq_prep_kernel, dim3(nq), dim3(256), 0, st, q_dev, d, vmin, step, u, bq, inv);
  return hipGetLastError();
}

hipError_t launch_sq_scan(const SqScanArgs& a, hipStream_t st) {
  if (a.nblk < 1 || a.grid < a.nblk || !a.work || !a.nwork) return hipErrorInvalidValue;
  const size_t smem = scan_smem_bytes(a.d, a.cap, 32);
#define SQ_LAUNCH(DD)                                                                                                          \
  {                                                                                                                            \
    auto kern = knn_sq_scan_kernel<DD, SQ_BURST>;                                                                              \
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); \
    if (e != hipSuccess) return e;                                                                                             \
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(KNN_WG), smem, st, a.codes, a.qfrag, a.bq, a.inv, a.nq, a.k, a.cap, a.thr_g,    \
                       a.part_s, a.part_i, a.part_n, a.work, a.nwork, a.nblk, a.work_stride);                                  \
    return hipGetLastError();                                                                                                  \
  }
  switch (a.d) {
    case 256: SQ_LAUNCH(256)
    case 512: SQ_LAUNCH(512)
    case 768: SQ_LAUNCH(768)
    case 1024: SQ_LAUNCH(1024)
    default: return hipErrorInvalidValue;
  }
#undef SQ_LAUNCH
}

// threshold mode over the work lists of the pass: rcnt [32 nblk] is cleared here
hipError_t launch_sq_range_scan(const SqScanArgs& a, hipStream_t st) {
  if (a.nblk < 1 || a.grid < a.nblk || !a.work || !a.nwork || !a.rthr || !a.rcnt || !a.hit_s || !a.hit_i) return hipErrorInvalidValue;
  if (a.nq < 1 || (uint64_t)a.nq * a.rcap > 0xffffffffull) return hipErrorInvalidValue;  // (the kernel indexes the pools with 32 bits)
  const size_t smem = (size_t)a.d * 128;
  hipError_t e = hipMemsetAsync(a.rcnt, 0, (size_t)a.nblk * 32 * sizeof(unsigned), st);
  if (e != hipSuccess) return e;
#define SQ_LAUNCH(DD)                                                                                                          \
  {                                                                                                                            \
    auto kern = knn_sq_range_scan_kernel<DD, sq_range_burst(DD)>;                                                              \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);       \
    if (e != hipSuccess) return e;                                                                                             \
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(KNN_WG), smem, st, a.codes, a.qfrag, a.bq, a.inv, a.nq, a.work, a.nwork,        \
                       a.nblk, a.work_stride, a.rthr, a.rcnt, a.rcap, a.hit_s, a.hit_i);                                       \
    return hipGetLastError();                                                                                                  \
  }
  switch (a.d) {
    case 256: SQ_LAUNCH(256)
    case 512: SQ_LAUNCH(512)
    case 768: SQ_LAUNCH(768)
    case 1024: SQ_LAUNCH(1024)
    default: return hipErrorInvalidValue;
  }
#undef SQ_LAUNCH
}

hipError_t launch_sq_probed_rows(const unsigned* masks, const unsigned* size, int nlist, int nq, unsigned long long* out, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(sq_probed_rows_kernel, dim3(nq), dim3(256), 0, st, masks, size, nlist, out);
  return hipGetLastError();
}

hipError_t launch_sq_encode(const _Float16* src, int64_t n, int d, const int32_t* lists, const int32_t* pos, const int64_t* ids,
                            int64_t id0, const unsigned* tile0, int64_t id_lo, int64_t n_ids, const float* vmin, const float* scale,
                            uint8_t* codes, int64_t* idmap, uint32_t* inv, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (d % 8 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sq_encode_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, src, n, d, lists, pos, ids, id0, tile0, id_lo,
                     n_ids, vmin, scale, codes, idmap, inv);
  return hipGetLastError();
}

hipError_t launch_sq_decode(const uint8_t* codes, int d, const float* vmin, const float* step, int64_t id_lo, int64_t n_ids,
                            const uint32_t* inv, const int64_t* ids, int64_t n, float* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(sq_decode_kernel, dim3((unsigned)n), dim3(256), 0, st, codes, d, vmin, step, id_lo, n_ids, inv, ids, n, out);
  return hipGetLastError();
}

// vmin_dev / vmax_dev: device f32 [d]; enc: device scratch of 2 d ints
hipError_t launch_sq_colminmax(const _Float16* X, int64_t n, int d, int* enc, float* vmin_dev, float* vmax_dev, hipStream_t st) {
  if (d <= 0 || d > 1024 || n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sq_minmax_init_kernel, dim3((d + 255) / 256), dim3(256), 0, st, d, enc, enc + d);
  const int64_t blocks = std::min<int64_t>((n + 63) / 64, 2048);
  hipLaunchKernelGGL(sq_colminmax_kernel, dim3((unsigned)blocks), dim3(256), 0, st, X, n, d, enc, enc + d);
  hipLaunchKernelGGL(sq_minmax_decode_kernel, dim3((d + 255) / 256), dim3(256), 0, st, d, enc, enc + d, vmin_dev, vmax_dev);
  return hipGetLastError();
}

}  // namespace knnx
