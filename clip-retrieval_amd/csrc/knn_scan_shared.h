// knn_scan_shared.h -- device helpers the list scans share (knn_kernels.hip: the fp16 scan and the merge; knn_sq_kernels.hip: the
// 8-bit scan): the order-preserving score encoding, the result order, the LDS candidate queues with their prune, and the split of a
// multi-block launch over its query blocks.  The scan that publishes partial lists and the merge that reads them compute the SAME
// ivfm_range, so there is one copy of it.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include "knn_kernels.h"

namespace knnx {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float16v __attribute__((ext_vector_type(16)));

// order-preserving float <-> int map (involution), so atomicMax on ints orders floats
__device__ __forceinline__ int enc_f(float f) {
  int b = __float_as_int(f);
  return b >= 0 ? b : (b ^ 0x7fffffff);
}
__device__ __forceinline__ float dec_f(int e) { return __int_as_float(e >= 0 ? e : (e ^ 0x7fffffff)); }

// strict total order of results: score descending, then id ascending
__device__ __forceinline__ bool better(float sa, uint32_t ia, float sb, uint32_t ib) {
  return (sa > sb) || (sa == sb && ia < ib);
}

struct ScanSmem {
  // carved from dynamic LDS in this order (all offsets multiples of 16 B)
  half8* qf;         // [KS*2*64]
  float* cand_s;     // [NQ*cap]
  uint32_t* cand_i;  // [NQ*cap]
  int* cnt;          // [NQ]
  int* thr;          // [NQ]  (encoded)
  int* flag;         // [4]
};

__device__ __forceinline__ ScanSmem carve(unsigned char* base, int d, int cap, int nqs) {
  ScanSmem s;
  size_t off = 0;
  s.qf = reinterpret_cast<half8*>(base + off);
  off += (size_t)d * 128;  // (d/16) * 2 * 64 * 16 B
  s.cand_s = reinterpret_cast<float*>(base + off);
  off += (size_t)nqs * cap * 4;
  s.cand_i = reinterpret_cast<uint32_t*>(base + off);
  off += (size_t)nqs * cap * 4;
  s.cnt = reinterpret_cast<int*>(base + off);
  off += nqs * 4;
  s.thr = reinterpret_cast<int*>(base + off);
  off += nqs * 4;
  s.flag = reinterpret_cast<int*>(base + off);
  return s;
}

// One wave sorts/prunes the queue of query `qq`: keeps the best min(n, k) entries, sorted, and
// raises the threshold to the k-th best.  n <= cap <= 128 (two entries per lane).
__device__ __forceinline__ void prune_query(const ScanSmem& sm, int qq, int cap, int k, int lane,
                                            int* __restrict__ thr_g) {
  int n = sm.cnt[qq];
  n = n < cap ? n : cap;
  float* cs = sm.cand_s + (size_t)qq * cap;
  uint32_t* ci = sm.cand_i + (size_t)qq * cap;
  const int e0 = lane, e1 = lane + 64;
  const bool v0 = e0 < n, v1 = e1 < n;
  const float s0 = v0 ? cs[e0] : 0.f, s1 = v1 ? cs[e1] : 0.f;
  const uint32_t i0 = v0 ? ci[e0] : 0u, i1 = v1 ? ci[e1] : 0u;
  int r0 = 0, r1 = 0;
  for (int j = 0; j < n; ++j) {
    const float sj = cs[j];
    const uint32_t ij = ci[j];
    r0 += better(sj, ij, s0, i0) ? 1 : 0;
    r1 += better(sj, ij, s1, i1) ? 1 : 0;
  }
  // all reads above are complete (in-order LDS queue of this wave) before the writes below issue
  __builtin_amdgcn_wave_barrier();
  if (v0 && r0 < k) { cs[r0] = s0; ci[r0] = i0; }
  if (v1 && r1 < k) { cs[r1] = s1; ci[r1] = i1; }
  if (n >= k) {
    if (v0 && r0 == k - 1) { atomicMax(&sm.thr[qq], enc_f(s0)); atomicMax(&thr_g[qq], enc_f(s0)); }
    if (v1 && r1 == k - 1) { atomicMax(&sm.thr[qq], enc_f(s1)); atomicMax(&thr_g[qq], enc_f(s1)); }
  }
  if (lane == 0) sm.cnt[qq] = n < k ? n : k;
}

// Multi-block IVF pass: the workgroups [s, e) of a G-workgroup launch that serve query block b, given the blocks' work-list
// lengths wk[0 .. nblk): every block owns one workgroup plus a share of the other G - nblk proportional to its tiles (blocks of a
// batch differ by +-10 % in tiles; an equal split leaves the chip waiting for the longest).  The list scan and the merge of its
// partial lists compute the same ranges from the same array.
__device__ __forceinline__ void ivfm_range(const unsigned* __restrict__ wk, int nblk, int G, int b, int& s, int& e) {
  unsigned long long tot = 0, cum = 0, upto = 0;
  for (int i = 0; i < nblk; ++i) {
    const unsigned v = wk[i];
    tot += v;
    if (i < b) cum += v;
    if (i <= b) upto += v;
  }
  const unsigned long long Gf = (unsigned long long)(G - nblk);
  s = b + (tot ? (int)(Gf * cum / tot) : 0);
  e = b + 1 + (tot ? (int)(Gf * upto / tot) : 0);
}

}  // namespace knnx
