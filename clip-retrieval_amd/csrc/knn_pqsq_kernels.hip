// knn_pqsq_kernels.hip -- gfx950 kernels of the SQ8 refine store of IVF-PQ: faiss IndexRefine(IndexIVFPQ, IndexScalarQuantizer(QT_8bit)),
// the ",Refine(SQ8)" factory suffix (include/knnx.h, "Refine store in SQ8").
//
// Next to the M code bytes of a row the index keeps ONE BYTE per column of the un-rotated row, encoded and decoded by the IVF-SQ8 contract
// (sq_encode_kernel / sq_decode_kernel of knn_sq_kernels.hip launched on this arena).  The kc = k x k_factor candidates of the ADC stage
// are a SCATTERED set of arena rows (cand -> inv -> row), so nothing of the IVF-SQ8 list scan applies: that one streams whole 32-row tiles
// through MFMA fragments and needs u split hi / lo and scaled into the fp16 range.  Here a candidate is a dot product of d bytes with a
// query held in registers: plain fp32 lanes, u in column order, no scaling, and the score is
//   <q, dec(row)> = b_q + sum_c u_c code_c,   u_c = q_c * step_c (rounded once),   b_q = <q, vmin + step / 2> (double, rounded once).
//
// Re-score (pqsq_rescore_kernel<D>): a row is D bytes = D / 16 lanes of one dwordx4 each, so a candidate takes a GROUP of 16 / 32 / 64
// lanes (D = 256 / 512 / 768 and 1024; at 768 lanes 48 .. 63 of the group hold zeros) and a wave step serves 4 / 2 / 1 candidates: every
// load instruction of a wave moves 1 KiB whatever the width.  The kernel is bound by the latency of the dependent gather, not by
// bandwidth, so a wave first fetches the ids and arena rows of ALL its steps (two rounds of latency for the whole wave), then keeps
// PQSQ_PF row loads in flight: the load of step s + PQSQ_PF is issued before step s is reduced.  The group's 16 u values per lane stay
// in registers for all candidates of the workgroup.  Bytes are widened by v_cvt_f32_ubyte{0..3} (exact; one instruction per byte next
// to its fma -- the v_perm_b32 / 0x64-exponent form of the list scan yields HALVES, which here would cost a further conversion each).
// Summation order (knnx.h): every lane ONE fmaf chain from 0.f over its 16 columns ascending of u_c * (float)code_c; the lane sums of a
// group meet in the xor butterfly G / 2, .., 2, 1; score = b_q + sum, rounded once.  Nothing in it depends on the batch, the shares of
// the ADC pass or the candidate's position.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include "knn_kernels.h"
#include "knn_sq_arith.h"

namespace knnx {

// ---------------------------------------------------------------------------------------------
// query preparation: one 256-thread workgroup per query.  u is rounded once (sq_mul); b_q is accumulated in double in the order of
// sq_prep_kernel (thread t the columns t, t + 256, .. ascending; xor butterfly 32 .. 1; (w0 + w1) + (w2 + w3)) and rounded once.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pqsq_prep_kernel(const float* __restrict__ q, int d, const float* __restrict__ vmin,
                                                       const float* __restrict__ step, float* __restrict__ u, float* __restrict__ bq) {
  __shared__ double s_sum[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* qn = q + (size_t)n * d;
  double sum = 0.0;
  for (int c = tid; c < d; c += 256) {
    u[(size_t)n * d + c] = sq_mul(qn[c], step[c]);
    sum += (double)qn[c] * ((double)vmin[c] + 0.5 * (double)step[c]);
  }
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if ((tid & 63) == 0) s_sum[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) bq[n] = (float)((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]));
}

// ---------------------------------------------------------------------------------------------
// the code re-score: grid (ceil(kc / PQSQ_WG), nq), 4 waves
// ---------------------------------------------------------------------------------------------
constexpr int PQSQ_WG = 32;  // candidates of one workgroup: kc = 512 of ONE query are 16 workgroups
constexpr int PQSQ_PF = 4;   // row loads a wave keeps in flight

// sum_t u[t] * byte t of the 16 loaded bytes: one chain, columns ascending
__device__ __forceinline__ float pqsq_dot16(const uint4& v, const float (&uv)[16]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  float acc = 0.f;
#pragma unroll
  for (int t = 0; t < 16; ++t) acc = fmaf(uv[t], (float)((w[t >> 2] >> (8 * (t & 3))) & 0xffu), acc);  // v_cvt_f32_ubyte{t & 3}
  return acc;
}

template <int D>
__global__ __launch_bounds__(256) void pqsq_rescore_kernel(const uint8_t* __restrict__ X, const float* __restrict__ u,
                                                          const float* __restrict__ bq, int64_t id_lo, int64_t n_ids,
                                                          const uint32_t* __restrict__ inv, const int64_t* __restrict__ cand, int kc,
                                                          float* __restrict__ es) {
  static_assert(D % 16 == 0 && D / 16 <= 64, "a row is one dwordx4 per lane of ONE wave pass");
  constexpr int G = D <= 256 ? 16 : (D <= 512 ? 32 : 64);  // lanes of one candidate
  constexpr int CPS = 64 / G;                              // candidates of one wave step
  constexpr int NS = PQSQ_WG / (4 * CPS);                  // steps of a wave
  constexpr int PF = NS < PQSQ_PF ? NS : PQSQ_PF;
  const int qi = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int gl = lane & (G - 1), sub = lane / G;
  const bool active = gl < D / 16;  // (D = 768: the last 16 lanes of the group carry zeros into the butterfly)

  float uv[16];
  if (active) {
    const float4* up = reinterpret_cast<const float4*>(u + (size_t)qi * D + (size_t)gl * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 a = up[j];
      uv[4 * j] = a.x; uv[4 * j + 1] = a.y; uv[4 * j + 2] = a.z; uv[4 * j + 3] = a.w;
    }
  } else {
#pragma unroll
    for (int t = 0; t < 16; ++t) uv[t] = 0.f;
  }
  const float b_q = bq[qi];

  // step s of this lane's group scores candidate c0 + s * 4 CPS: first every id, then every arena row (a bad id, or no candidate: no row)
  const int c0 = (int)blockIdx.x * PQSQ_WG + w * CPS + sub;
  if (n_ids <= 0) {  // (uniform) an index without rows has no inv[0] and no arena row 0 to read
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = c0 + s * 4 * CPS;
      if (gl == 0 && c < kc) es[(size_t)qi * kc + c] = -FLT_MAX;
    }
    return;
  }
  int64_t id[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int c = c0 + s * 4 * CPS;
    const int64_t v = cand[(size_t)qi * kc + (c < kc ? c : kc - 1)];
    id[s] = c < kc ? v : -1;
  }
  // Every load below is UNCONDITIONAL, from an address that is always inside its array (an index without rows left above),
  // and what it fetched is simply not used: a group without a candidate reads inv[0] and arena row 0 and reports -FLT_MAX, an idle
  // lane of D = 768 multiplies its group's first 16 bytes by u = 0.  (A load under a lane mask would be waited for alone; these are
  // counted, so the rounds of the gather overlap.)
  bool ok[NS];
  uint32_t row[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    ok[s] = id[s] >= id_lo && id[s] - id_lo < n_ids;
    row[s] = inv[ok[s] ? id[s] - id_lo : 0];
  }
  const size_t col = (size_t)(active ? gl : 0) * 16;
  auto load = [&](int s) -> uint4 { return *reinterpret_cast<const uint4*>(X + (size_t)(ok[s] ? row[s] : 0u) * D + col); };
  uint4 v[PF];
#pragma unroll
  for (int s = 0; s < PF; ++s) v[s] = load(s);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const uint4 cur = v[s % PF];
    if (s + PF < NS) v[s % PF] = load(s + PF);
    __builtin_amdgcn_sched_barrier(0);  // the next load is issued before this step's arithmetic
    float acc = pqsq_dot16(cur, uv);
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    const int c = c0 + s * 4 * CPS;
    if (gl == 0 && c < kc) es[(size_t)qi * kc + c] = ok[s] ? b_q + acc : -FLT_MAX;
  }
}

// ---------------------------------------------------------------------------------------------
// launchers (declared in knn_kernels.h)
// ---------------------------------------------------------------------------------------------
hipError_t launch_pqsq_prep(const float* q, int nq, int d, const float* vmin, const float* step, float* u, float* bq, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(pqsq_prep_kernel, dim3((unsigned)nq), dim3(256), 0, st, q, d, vmin, step, u, bq);
  return hipGetLastError();
}

hipError_t launch_pqsq_rescore(const uint8_t* codes, int d, const float* u, const float* bq, int nq, int64_t id_lo, int64_t n_ids,
                               const uint32_t* inv, const int64_t* cand, int kc, float* es, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  if (kc < 1 || nq > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((kc + PQSQ_WG - 1) / PQSQ_WG), (unsigned)nq);
#define PQSQ_RS(DD) hipLaunchKernelGGL(pqsq_rescore_kernel<DD>, grid, dim3(256), 0, st, codes, u, bq, id_lo, n_ids, inv, cand, kc, es)
  switch (d) {
    case 256: PQSQ_RS(256); break;
    case 512: PQSQ_RS(512); break;
    case 768: PQSQ_RS(768); break;
    case 1024: PQSQ_RS(1024); break;
    default: return hipErrorInvalidValue;
  }
#undef PQSQ_RS
  return hipGetLastError();
}

}  // namespace knnx
