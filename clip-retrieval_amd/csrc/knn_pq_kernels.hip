// knn_pq_kernels.hip -- gfx950 kernels of the IVF-PQ index (faiss IndexIVFPQ(IndexFlatIP(d), d, nlist, M, 8), inner product,
// by_residual): encoding, codebook training, the per-query lookup tables, the ADC list scan with top-k, decoding.
//
// Data layout in HBM
//   codes    u8 [capacity][M]: the list-sorted, tile-padded arena of IVF-Flat with M code bytes per row instead of 2 d
//   cb       f32 [M][256][ds], ds = d / M: sub-quantiser m, centroid j, component t
//   lut      f32 [nq][M][256]: LUT[q][m][j] = <q_m, cb[m][j]> (fp32, t in order)
// A row's residual is r = f32(x_f16) - f32(c_list); its code byte m is argmin_j ||r_m - cb[m][j]||^2 (ties -> smaller j); its
// score for a query is <q, c_list> + sum_m LUT[m][code_m] (the sum in m order, then added to the coarse score).
//
// ADC scan: one workgroup per (query, share of its probed lists), 4 waves.  The query's lookup table (M KiB) is loaded into the
// LDS once; every lane scores one row per step (M / 16 16-byte code loads, M LDS lookups).  Each WAVE keeps its own candidate
// queue in the LDS (k + 64 entries, appended through a ballot, pruned to the exact top k by a rank count when full), so the row
// loop has no workgroup barrier; at the end the four queues are ranked together and the workgroup's top k goes to the partial
// lists that knn_merge_kernel (launch_merge_u32 with the id map) merges.

#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include "knn_kernels.h"

namespace knnx {

constexpr int PQ_WQ = PQ_MAX_K + 64;  // entries of one wave's candidate queue

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// strict total order of results: score descending, then id ascending
__device__ __forceinline__ bool pq_better(float sa, long long ia, float sb, long long ib) {
  return (sa > sb) || (sa == sb && ia < ib);
}

// ---------------------------------------------------------------------------------------------
// encode: one row per thread.  Source rows are fp16 with a list id each; the residual is formed in registers.  The workgroup
// stages sub-quantiser m's 256 centroids in the LDS (every lane reads the same address: broadcast), each lane keeps its
// residual sub-vector in registers and walks the 256 centroids.  Destination: arena row tile0[list] * 32 + pos[i] (tile0 == null:
// row i of a plain [n][M] array); idmap / inv written when idmap != null.
// ---------------------------------------------------------------------------------------------
template <int DS>
__global__ __launch_bounds__(256) void pq_encode_kernel(const _Float16* __restrict__ X, int64_t n, int d, int M,
                                                       const int32_t* __restrict__ lists, const _Float16* __restrict__ cent,
                                                       const float* __restrict__ cb, const unsigned* __restrict__ tile0,
                                                       const int32_t* __restrict__ pos, const int64_t* __restrict__ ids, int64_t id0,
                                                       int64_t id_lo, int64_t n_ids, uint8_t* __restrict__ codes,
                                                       int64_t* __restrict__ idmap, uint32_t* __restrict__ inv) {
  extern __shared__ float pq_sc[];  // [256][DS]
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  const int32_t l = live ? lists[i] : 0;
  const _Float16* xr = X + (size_t)(live ? i : 0) * d;
  const _Float16* cr = cent + (size_t)l * d;
  const size_t drow = live ? (tile0 ? (size_t)tile0[l] * 32 + (size_t)pos[i] : (size_t)i) : 0;
  for (int m = 0; m < M; ++m) {
    __syncthreads();
    const float* src = cb + (size_t)m * 256 * DS;
    for (int e = threadIdx.x; e < 256 * DS; e += 256) pq_sc[e] = src[e];
    __syncthreads();
    if (live) {
      float r[DS];
#pragma unroll
      for (int t = 0; t < DS; ++t) r[t] = (float)xr[m * DS + t] - (float)cr[m * DS + t];
      float best = INFINITY;
      int bj = 0;
      for (int j = 0; j < 256; ++j) {
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < DS; ++t) {
          const float df = r[t] - pq_sc[j * DS + t];
          s = fmaf(df, df, s);
        }
        if (s < best) { best = s; bj = j; }
      }
      codes[drow * M + m] = (uint8_t)bj;
    }
  }
  if (live && idmap) {
    const int64_t id = ids ? ids[i] : id0 + i;
    idmap[drow] = id;
    if (id >= id_lo && id - id_lo < n_ids) inv[id - id_lo] = (uint32_t)drow;
  }
}

// ---------------------------------------------------------------------------------------------
// PQ Lloyd update: one 64-thread workgroup per (m, j); lane t sums component t of the residual sub-vectors of the cluster's
// members in order[] order (ascending sample row: a fixed summation order) and writes the mean.  Empty clusters keep their centroid.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pq_update_kernel(const _Float16* __restrict__ X, int d, int M, const int32_t* __restrict__ lists,
                                                      const _Float16* __restrict__ cent, const int32_t* __restrict__ order,
                                                      const int32_t* __restrict__ off, int64_t n, float* __restrict__ cb) {
  const int ds = d / M;
  const int m = blockIdx.x / 256, j = blockIdx.x % 256, t = threadIdx.x;
  const int a = off[m * 257 + j], b = off[m * 257 + j + 1];
  if (b <= a || t >= ds) return;
  const int32_t* ord = order + (size_t)m * n;
  const int c = m * ds + t;
  float s = 0.f;
  for (int e = a; e < b; ++e) {
    const int64_t r = ord[e];
    s += (float)X[(size_t)r * d + c] - (float)cent[(size_t)lists[r] * d + c];
  }
  cb[((size_t)m * 256 + j) * ds + t] = s / (float)(b - a);
}

// codebook entry mj[i] = m * 256 + j := residual sub-vector m of sample row rows[i] (seeding, re-seeding of empty clusters)
__global__ __launch_bounds__(64) void pq_seed_kernel(const _Float16* __restrict__ X, int d, int M, const int32_t* __restrict__ lists,
                                                    const _Float16* __restrict__ cent, const int32_t* __restrict__ mj,
                                                    const int64_t* __restrict__ rows, float* __restrict__ cb) {
  const int ds = d / M, i = blockIdx.x, t = threadIdx.x;
  if (t >= ds) return;
  const int m = mj[i] / 256;
  const int64_t r = rows[i];
  const int c = m * ds + t;
  cb[(size_t)mj[i] * ds + t] = (float)X[(size_t)r * d + c] - (float)cent[(size_t)lists[r] * d + c];
}

// ---------------------------------------------------------------------------------------------
// lookup tables: workgroup (q, m), thread j: LUT[q][m][j] = sum_t q[m ds + t] * cb[m][j][t] (fp32, t in order)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pq_lut_kernel(const float* __restrict__ q, int d, int M, const float* __restrict__ cb,
                                                    float* __restrict__ lut) {
  __shared__ float sq[64];
  const int qi = blockIdx.x, m = blockIdx.y, j = threadIdx.x, ds = d / M;
  if (j < ds) sq[j] = q[(size_t)qi * d + m * ds + j];
  __syncthreads();
  const float* c = cb + ((size_t)m * 256 + j) * ds;
  float s = 0.f;
  for (int t = 0; t < ds; ++t) s = fmaf(sq[t], c[t], s);
  lut[((size_t)qi * M + m) * 256 + j] = s;
}

// ---------------------------------------------------------------------------------------------
// probe lists: the masks of ivf_select_mark_kernel ([nblk][nlist], bit q % 32 of block q / 32) -> per query the ids of its
// probed lists and their coarse scores (any order: the scan's result does not depend on it)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pq_probe_kernel(const unsigned* __restrict__ masks, const float* __restrict__ scores, int nq,
                                                      int nlist, int np, unsigned* __restrict__ pcnt, int* __restrict__ probe,
                                                      float* __restrict__ pscore) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (l >= nlist) return;
  unsigned mk = masks[(size_t)b * nlist + l];
  while (mk) {
    const int bit = __ffs(mk) - 1;
    mk &= mk - 1;
    const int qi = b * 32 + bit;
    if (qi >= nq) continue;
    const unsigned p = atomicAdd(&pcnt[qi], 1u);
    if (p < (unsigned)np) {
      probe[(size_t)qi * np + p] = l;
      pscore[(size_t)qi * np + p] = scores[(size_t)qi * nlist + l];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// M = 256 (PQ256x8): the query's lookup table is 256 KiB and does not fit the LDS, so the ADC stage runs in two halves of m over the
// same shares.  The lower half (pq_adc_lower_kernel) scores every probed row over tables 0 .. 127 and stores the fp32 partial sum; the
// upper half is the UP mode of the three scans below, which starts from that sum and continues over tables 128 .. 255.  A 4-byte store
// and load is exact, so the score is cs + (ONE fp32 chain over m = 0 .. 255 from 0.f), as for every other M.
//
// Partial sums: query q of a sub-group that starts at q0 owns the slab part[(q - q0) * slab ..]; inside it, probe p of the query
// starts at poff[q][p] = the rows of the query's probes before p (pq_probe_offsets_kernel), and row i of the list sits at + i.  slab is
// the sum of the np largest list sizes of the index (knnx_pq_plan.h), so a query's probed lists always fit.
// ---------------------------------------------------------------------------------------------
// exclusive prefix of size[probe[q][p]] over p < min(pcnt[q], np), in probe-list order; one workgroup per query, np of any size
__global__ __launch_bounds__(256) void pq_probe_offsets_kernel(const int* __restrict__ probe, const unsigned* __restrict__ pcnt, int np,
                                                              const unsigned* __restrict__ size, unsigned* __restrict__ poff) {
  __shared__ unsigned sc[256];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int npq = min((int)pcnt[q], np);
  unsigned carry = 0;  // rows before this chunk of 256 probes (the same in every thread)
  for (int p0 = 0; p0 < npq; p0 += 256) {
    const int p = p0 + tid;
    const unsigned mine = p < npq ? size[probe[(size_t)q * np + p]] : 0u;
    sc[tid] = mine;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive scan of the chunk
      const unsigned add = tid >= o ? sc[tid - o] : 0u;
      __syncthreads();
      sc[tid] += add;
      __syncthreads();
    }
    if (p < npq) poff[(size_t)q * np + p] = carry + sc[tid] - mine;
    carry += sc[255];
    __syncthreads();
  }
}

// lower half: grid (nsplit, g), the shares of pq_adc_scan_kernel (any nsplit: a row's slot does not depend on the share that scores
// it).  Tables 0 .. 127 of query q0 + blockIdx.y in the LDS (128 KiB); every lane one row per step: eight 16-byte code loads, 128 LDS
// lookups, one 4-byte store.  No queue, no barrier in the row loop, no id map.  thr (null: none) is the threshold array of a threshold
// scan: a query at +INFINITY is finished and its workgroups return at once, like those of the upper half.
static_assert((size_t)128 * 1024 + 64 <= (size_t)KNN_LDS_BYTES, "M = 256: a half-table exceeds the LDS");
__global__ __launch_bounds__(256) void pq_adc_lower_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ lut,
                                                          const int* __restrict__ probe, const unsigned* __restrict__ pcnt, int np,
                                                          int nsplit, const unsigned* __restrict__ tile0,
                                                          const unsigned* __restrict__ size, const unsigned* __restrict__ poff,
                                                          const float* __restrict__ thr, size_t slab, int q0, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pq_smem[];
  float* s_lut = reinterpret_cast<float*>(pq_smem);  // [128 * 256]
  const int s = blockIdx.x, q = (int)blockIdx.y + q0, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (thr && thr[q] == INFINITY) return;  // (the whole workgroup: q is its query)
  const float4* lq = reinterpret_cast<const float4*>(lut + (size_t)q * 256 * 256);
  for (int e = tid; e < 128 * 64; e += 256) reinterpret_cast<float4*>(s_lut)[e] = lq[e];
  __syncthreads();
  float* slab_q = part + (size_t)blockIdx.y * slab;
  const int npq = min((int)pcnt[q], np);
  for (int p = s; p < npq; p += nsplit) {
    const int l = probe[(size_t)q * np + p];
    const size_t r0 = (size_t)tile0[l] * 32;
    const unsigned sz = size[l];
    const size_t off = poff[(size_t)q * np + p];
    for (unsigned base = (unsigned)w * 64; base < sz; base += 256) {
      const unsigned i = base + lane;
      if (i < sz && off + i < slab) {  // (off + sz <= slab by the definition of slab; checked all the same: this is a store)
        const uint4* cp = reinterpret_cast<const uint4*>(codes + (r0 + i) * 256);
        uint4 cw[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) cw[v] = cp[v];
        float acc = 0.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
          const unsigned ww[4] = {cw[v].x, cw[v].y, cw[v].z, cw[v].w};
#pragma unroll
          for (int b = 0; b < 16; ++b) acc += s_lut[(v * 16 + b) * 256 + ((ww[b >> 2] >> (8 * (b & 3))) & 255u)];
        }
        slab_q[off + i] = acc;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// ADC list scan with top-k (see the head of the file).  grid (nsplit, nq); workgroup (s, q) scans probes s, s + nsplit, ... of
// query q and writes partial list s * nq + q (<= k entries, arena rows) of part_s / part_i / part_n.
// ---------------------------------------------------------------------------------------------
// wave-local prune: the queue (n <= PQ_WQ entries) -> its top min(n, k) in rank order; returns the new count; thr = the k-th score
__device__ __forceinline__ int pq_wave_prune(float* qs, uint32_t* qr, long long* qi, int n, int k, int lane, float& thr) {
  float s0 = 0.f, s1 = 0.f;
  uint32_t r0 = 0, r1 = 0;
  long long i0 = 0, i1 = 0;
  const bool v0 = lane < n, v1 = lane + 64 < n;
  int k0 = 0, k1 = 0;  // ranks
  if (v0) { s0 = qs[lane]; r0 = qr[lane]; i0 = qi[lane]; }
  if (v1) { s1 = qs[lane + 64]; r1 = qr[lane + 64]; i1 = qi[lane + 64]; }
  for (int j = 0; j < n; ++j) {
    const float sj = qs[j];
    const long long ij = qi[j];
    k0 += pq_better(sj, ij, s0, i0) ? 1 : 0;
    k1 += pq_better(sj, ij, s1, i1) ? 1 : 0;
  }
  wave_sync();
  if (v0 && k0 < k) { qs[k0] = s0; qr[k0] = r0; qi[k0] = i0; }
  if (v1 && k1 < k) { qs[k1] = s1; qr[k1] = r1; qi[k1] = i1; }
  wave_sync();
  if (n >= k) thr = qs[k - 1];
  return n < k ? n : k;
}

// The three scans below are written once as a body with a mode: UP = false is the whole scan of an index with M <= 128 code bytes per
// row (acc from 0.f over tables 0 .. M - 1).  UP = true is the UPPER HALF of the M = 256 scan (see pq_adc_lower_kernel): M = 128 tables
// are staged, tables 128 .. 255 of the query's 256, the row's code bytes 128 .. 255 are read, and acc starts from the fp32 partial sum
// the lower half stored for the row -- part[(q - q0) * slab + poff[q][p] + i] -- so that the score is the one ascending chain over
// m = 0 .. 255.  The workgroup's query is q0 + blockIdx.y (a sub-group of the pass); everything else is indexed by q as before.
template <int M, bool UP>
__device__ __forceinline__ void pq_adc_scan_body(const uint8_t* __restrict__ codes, const float* __restrict__ lut,
                                                 const int* __restrict__ probe, const float* __restrict__ pscore,
                                                 const unsigned* __restrict__ pcnt, int np, int nsplit,
                                                 const unsigned* __restrict__ tile0, const unsigned* __restrict__ size,
                                                 const int64_t* __restrict__ idmap, int k, int nq, float* __restrict__ part_s,
                                                 uint32_t* __restrict__ part_i, int* __restrict__ part_n, const float* __restrict__ half,
                                                 const unsigned* __restrict__ poff, size_t slab, int q0) {
  constexpr int ROW = UP ? 256 : M, BYTE0 = UP ? 128 : 0;  // bytes of an arena row, the first one this scan reads
  extern __shared__ __attribute__((aligned(16))) unsigned char pq_smem[];
  float* s_lut = reinterpret_cast<float*>(pq_smem);                  // [M * 256]
  long long* c_id = reinterpret_cast<long long*>(s_lut + M * 256);  // [4][PQ_WQ]
  float* c_s = reinterpret_cast<float*>(c_id + 4 * PQ_WQ);           // [4][PQ_WQ]
  uint32_t* c_r = reinterpret_cast<uint32_t*>(c_s + 4 * PQ_WQ);      // [4][PQ_WQ]
  __shared__ int w_cnt[4];
  const int s = blockIdx.x, q = (int)blockIdx.y + (UP ? q0 : 0), tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float4* lq = reinterpret_cast<const float4*>(lut + ((size_t)q * ROW + BYTE0) * 256);
  for (int e = tid; e < M * 64; e += 256) reinterpret_cast<float4*>(s_lut)[e] = lq[e];
  __syncthreads();
  float* qs = c_s + w * PQ_WQ;
  uint32_t* qr = c_r + w * PQ_WQ;
  long long* qi = c_id + w * PQ_WQ;
  int cnt = 0;
  float thr = -INFINITY;
  const int npq = min((int)pcnt[q], np);
  for (int p = s; p < npq; p += nsplit) {
    const int l = probe[(size_t)q * np + p];
    const float cs = pscore[(size_t)q * np + p];
    const size_t r0 = (size_t)tile0[l] * 32;
    const unsigned sz = size[l];
    const float* hp = UP ? half + (size_t)blockIdx.y * slab + poff[(size_t)q * np + p] : nullptr;  // the list's partial sums
    for (unsigned base = (unsigned)w * 64; base < sz; base += 256) {
      if (cnt > PQ_WQ - 64) cnt = pq_wave_prune(qs, qr, qi, cnt, k, lane, thr);
      const unsigned i = base + lane;
      float sc = -INFINITY;
      bool ok = false;
      size_t row = 0;
      if (i < sz) {
        row = r0 + i;
        const uint4* cp = reinterpret_cast<const uint4*>(codes + row * ROW + BYTE0);
        uint4 cw[M / 16];
#pragma unroll
        for (int v = 0; v < M / 16; ++v) cw[v] = cp[v];
        float acc = UP ? hp[i] : 0.f;
#pragma unroll
        for (int v = 0; v < M / 16; ++v) {
          const unsigned ww[4] = {cw[v].x, cw[v].y, cw[v].z, cw[v].w};
#pragma unroll
          for (int b = 0; b < 16; ++b) acc += s_lut[(v * 16 + b) * 256 + ((ww[b >> 2] >> (8 * (b & 3))) & 255u)];
        }
        sc = cs + acc;
        ok = sc >= thr;
      }
      const unsigned long long bal = __ballot(ok);
      if (ok) {
        const int at = cnt + (int)__popcll(bal & ((1ull << lane) - 1ull));
        qs[at] = sc;
        qr[at] = (uint32_t)row;
        qi[at] = (long long)idmap[row];
      }
      cnt += (int)__popcll(bal);
      wave_sync();
    }
  }
  cnt = pq_wave_prune(qs, qr, qi, cnt, k, lane, thr);
  if (lane == 0) w_cnt[w] = cnt;
  __syncthreads();
  // the four queues (each <= k sorted entries) ranked together: thread (w, lane) holds entry `lane` of queue w
  const bool mine = lane < w_cnt[w];
  const float se = mine ? qs[lane] : 0.f;
  const long long ie = mine ? qi[lane] : 0;
  int rank = 0;
  if (mine) {
    for (int v = 0; v < 4; ++v)
      for (int j = 0; j < w_cnt[v]; ++j) rank += pq_better(c_s[v * PQ_WQ + j], c_id[v * PQ_WQ + j], se, ie) ? 1 : 0;
  }
  const size_t slot = (size_t)s * nq + q;
  if (mine && rank < k) {
    part_s[slot * k + rank] = se;
    part_i[slot * k + rank] = qr[lane];
  }
  if (tid == 0) {
    const int tot = w_cnt[0] + w_cnt[1] + w_cnt[2] + w_cnt[3];
    part_n[slot] = tot < k ? tot : k;
  }
}

template <int M>
__global__ __launch_bounds__(256) void pq_adc_scan_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ lut,
                                                         const int* __restrict__ probe, const float* __restrict__ pscore,
                                                         const unsigned* __restrict__ pcnt, int np, int nsplit,
                                                         const unsigned* __restrict__ tile0, const unsigned* __restrict__ size,
                                                         const int64_t* __restrict__ idmap, int k, int nq, float* __restrict__ part_s,
                                                         uint32_t* __restrict__ part_i, int* __restrict__ part_n) {
  pq_adc_scan_body<M, false>(codes, lut, probe, pscore, pcnt, np, nsplit, tile0, size, idmap, k, nq, part_s, part_i, part_n, nullptr, nullptr, 0,
                             0);
}

// upper half of the M = 256 scan; grid (nsplit, g): queries q0 .. q0 + g - 1 of the pass's nq.  LDS as M = 128: 136 KiB
static_assert((size_t)128 * 1024 + (size_t)4 * PQ_WQ * 16 + 64 <= (size_t)KNN_LDS_BYTES, "M = 256: a half-table + the queues exceed the LDS");
__global__ __launch_bounds__(256) void pq_adc_upper_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ lut,
                                                          const int* __restrict__ probe, const float* __restrict__ pscore,
                                                          const unsigned* __restrict__ pcnt, int np, int nsplit,
                                                          const unsigned* __restrict__ tile0, const unsigned* __restrict__ size,
                                                          const int64_t* __restrict__ idmap, int k, int nq, float* __restrict__ part_s,
                                                          uint32_t* __restrict__ part_i, int* __restrict__ part_n,
                                                          const float* __restrict__ half, const unsigned* __restrict__ poff, size_t slab,
                                                          int q0) {
  pq_adc_scan_body<128, true>(codes, lut, probe, pscore, pcnt, np, nsplit, tile0, size, idmap, k, nq, part_s, part_i, part_n, half, poff, slab,
                              q0);
}

// ---------------------------------------------------------------------------------------------
// Threshold mode of the ADC scan (range_search and k > 64 on an index with the threshold-scan switch on).  Grid, shares, LUT staging
// and the scoring of a row are those of pq_adc_scan_kernel -- the same fp32 values, acc summed in m order, then cs + acc -- but there
// are no candidate queues: a row is a hit when its score is > thr[q] (strict), and hits go to query q's slice of the range pools
// (hit_s / hit_r [q * cap ..], score and ARENA ROW; the ids are resolved by the range sort through idmap).  Appends are aggregated per
// wave: one ballot, ONE atomicAdd of the popcount by lane 0, the base broadcast, every hit lane writes at base + its prefix when that
// is below cap.  With thr = -FLT_MAX every scored row is a hit on one counter per query, which a per-lane atomic would serialise.
// cnt[q] stays exact when the slice overflows (the host regrows the pools and scans again).  A query whose threshold is +INFINITY is
// finished: its workgroups return before they touch the LUT.  LDS: the LUT only, M KiB; no barrier in the row loop.
// ---------------------------------------------------------------------------------------------
static_assert((size_t)128 * 1024 + 64 <= (size_t)KNN_LDS_BYTES, "M = 128: the LUT of the threshold scan exceeds the LDS");

template <int M, bool UP>
__device__ __forceinline__ void pq_range_scan_body(const uint8_t* __restrict__ codes, const float* __restrict__ lut,
                                                   const int* __restrict__ probe, const float* __restrict__ pscore,
                                                   const unsigned* __restrict__ pcnt, int np, int nsplit,
                                                   const unsigned* __restrict__ tile0, const unsigned* __restrict__ size,
                                                   const float* __restrict__ thr, unsigned* __restrict__ cnt, unsigned cap,
                                                   float* __restrict__ hit_s, uint32_t* __restrict__ hit_r, const float* __restrict__ half,
                                                   const unsigned* __restrict__ poff, size_t slab, int q0) {
  constexpr int ROW = UP ? 256 : M, BYTE0 = UP ? 128 : 0;  // bytes of an arena row, the first one this scan reads
  extern __shared__ __attribute__((aligned(16))) unsigned char pq_smem[];
  float* s_lut = reinterpret_cast<float*>(pq_smem);  // [M * 256]
  const int s = blockIdx.x, q = (int)blockIdx.y + (UP ? q0 : 0), tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float th = thr[q];
  if (th == INFINITY) return;  // (the whole workgroup: q is its query)
  const float4* lq = reinterpret_cast<const float4*>(lut + ((size_t)q * ROW + BYTE0) * 256);
  for (int e = tid; e < M * 64; e += 256) reinterpret_cast<float4*>(s_lut)[e] = lq[e];
  __syncthreads();
  float* hs = hit_s + (size_t)q * cap;
  uint32_t* hr = hit_r + (size_t)q * cap;
  const int npq = min((int)pcnt[q], np);
  for (int p = s; p < npq; p += nsplit) {
    const int l = probe[(size_t)q * np + p];
    const float cs = pscore[(size_t)q * np + p];
    const size_t r0 = (size_t)tile0[l] * 32;
    const unsigned sz = size[l];
    const float* hp = UP ? half + (size_t)blockIdx.y * slab + poff[(size_t)q * np + p] : nullptr;  // the list's partial sums
    for (unsigned base = (unsigned)w * 64; base < sz; base += 256) {
      const unsigned i = base + lane;
      float sc = -INFINITY;
      bool ok = false;
      size_t row = 0;
      if (i < sz) {
        row = r0 + i;
        const uint4* cp = reinterpret_cast<const uint4*>(codes + row * ROW + BYTE0);
        uint4 cw[M / 16];
#pragma unroll
        for (int v = 0; v < M / 16; ++v) cw[v] = cp[v];
        float acc = UP ? hp[i] : 0.f;
#pragma unroll
        for (int v = 0; v < M / 16; ++v) {
          const unsigned ww[4] = {cw[v].x, cw[v].y, cw[v].z, cw[v].w};
#pragma unroll
          for (int b = 0; b < 16; ++b) acc += s_lut[(v * 16 + b) * 256 + ((ww[b >> 2] >> (8 * (b & 3))) & 255u)];
        }
        sc = cs + acc;
        ok = sc > th;
      }
      const unsigned long long bal = __ballot(ok);
      if (bal) {  // (wave-uniform)
        unsigned at0 = 0;
        if (lane == 0) at0 = atomicAdd(&cnt[q], (unsigned)__popcll(bal));
        at0 = (unsigned)__shfl((int)at0, 0);
        if (ok) {
          const size_t at = (size_t)at0 + (size_t)__popcll(bal & ((1ull << lane) - 1ull));
          if (at < (size_t)cap) {
            hs[at] = sc;
            hr[at] = (uint32_t)row;
          }
        }
      }
    }
  }
}

template <int M>
__global__ __launch_bounds__(256) void pq_range_scan_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ lut,
                                                           const int* __restrict__ probe, const float* __restrict__ pscore,
                                                           const unsigned* __restrict__ pcnt, int np, int nsplit,
                                                           const unsigned* __restrict__ tile0, const unsigned* __restrict__ size,
                                                           const float* __restrict__ thr, unsigned* __restrict__ cnt, unsigned cap,
                                                           float* __restrict__ hit_s, uint32_t* __restrict__ hit_r) {
  pq_range_scan_body<M, false>(codes, lut, probe, pscore, pcnt, np, nsplit, tile0, size, thr, cnt, cap, hit_s, hit_r, nullptr, nullptr, 0, 0);
}

// upper half of the M = 256 threshold scan; grid (nsplit, g).  LDS as M = 128: 128 KiB
__global__ __launch_bounds__(256) void pq_range_upper_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ lut,
                                                            const int* __restrict__ probe, const float* __restrict__ pscore,
                                                            const unsigned* __restrict__ pcnt, int np, int nsplit,
                                                            const unsigned* __restrict__ tile0, const unsigned* __restrict__ size,
                                                            const float* __restrict__ thr, unsigned* __restrict__ cnt, unsigned cap,
                                                            float* __restrict__ hit_s, uint32_t* __restrict__ hit_r,
                                                            const float* __restrict__ half, const unsigned* __restrict__ poff, size_t slab,
                                                            int q0) {
  pq_range_scan_body<128, true>(codes, lut, probe, pscore, pcnt, np, nsplit, tile0, size, thr, cnt, cap, hit_s, hit_r, half, poff, slab, q0);
}

// ---------------------------------------------------------------------------------------------
// Refine (faiss IndexRefineFlat(IndexIVFPQ)): the kc = k x k_factor best rows by ADC score are re-scored exactly from the resident
// fp16 rows.  For kc <= PQ_MAX_K the candidates come from pq_adc_scan_kernel + knn_merge_kernel above; for 64 < kc <= PQ_REFINE_MAX
// from the three kernels below.  Same scores (same LUT, same summation order), same total order (score descending, id ascending).
//
// Candidate scan: grid and shares as pq_adc_scan_kernel, but ONE queue per workgroup of PQ_CQ (score, arena row) entries -- the id
// is read from idmap only where two scores tie.  Every step the four waves score 256 rows of the current list (uniform trip
// count: a list is walked by the whole workgroup), append what passes the threshold behind a per-wave count exchanged through the
// LDS (one barrier per step; the counts alternate between two sets so that a fast wave cannot overwrite what a slow one still
// reads), and when fewer than 256 slots are free the queue is pruned: bitonic sort of all PQ_CQ slots, O(n log^2 n), keep kc,
// threshold = the kc-th score.  With kc = 512 a prune frees 1280 slots.
// LDS budget (dynamic, 16-byte carves): LUT M KiB + queue PQ_CQ x 8 B = 16 KiB + 32 B of counts
//   M = 16: 32 KiB + 32 B   M = 32: 48 KiB + 32 B   M = 64: 80 KiB + 32 B   M = 128: 144 KiB + 32 B   (of 160 KiB)
// ---------------------------------------------------------------------------------------------
constexpr int PQ_CQ = 2048;             // slots of the workgroup's candidate queue
constexpr unsigned PQ_NOROW = ~0u;      // arena row of an empty queue slot (score -inf)
static_assert(PQ_CQ >= PQ_REFINE_MAX + 256 && (PQ_CQ & (PQ_CQ - 1)) == 0, "the queue holds kc entries and one step, and is sorted as a power of two");
static_assert((size_t)128 * 1024 + (size_t)PQ_CQ * 8 + 32 + 64 <= (size_t)KNN_LDS_BYTES, "M = 128: LUT + queue + counts exceed the LDS");
static_assert((size_t)PQ_SEL_MAX * 8 + 64 <= (size_t)KNN_LDS_BYTES, "the selection holds a query's partial lists in the LDS");

// a before b in the result order; rows index idmap (PQ_NOROW: an empty slot, after everything else)
__device__ __forceinline__ bool pq_row_better(float sa, uint32_t ra, float sb, uint32_t rb, const int64_t* __restrict__ idmap) {
  if (sa != sb) return sa > sb;
  if (ra == rb || ra == PQ_NOROW) return false;
  if (rb == PQ_NOROW) return true;
  return idmap[ra] < idmap[rb];
}

// bitonic sort of n (a power of two) LDS entries into result order, by all threads of the workgroup; barriers inside, so every
// thread calls it with the same n.  Entries written before the call must be followed by a barrier by the caller.
__device__ __forceinline__ void pq_bitonic(float* s, uint32_t* r, int n, const int64_t* __restrict__ idmap, int tid, int nthr) {
  for (int kk = 2; kk <= n; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int p = tid; p < (n >> 1); p += nthr) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));  // the lower index of pair p
        const int l = i | j;
        const float si = s[i], sl = s[l];
        const uint32_t ri = r[i], rl = r[l];
        const bool fwd = (i & kk) == 0;
        const bool sw = fwd ? pq_row_better(sl, rl, si, ri, idmap) : pq_row_better(si, ri, sl, rl, idmap);
        if (sw) { s[i] = sl; r[i] = rl; s[l] = si; r[l] = ri; }
      }
      __syncthreads();
    }
}

template <int M, bool UP>
__device__ __forceinline__ void pq_cand_scan_body(const uint8_t* __restrict__ codes, const float* __restrict__ lut,
                                                  const int* __restrict__ probe, const float* __restrict__ pscore,
                                                  const unsigned* __restrict__ pcnt, int np, int nsplit,
                                                  const unsigned* __restrict__ tile0, const unsigned* __restrict__ size,
                                                  const int64_t* __restrict__ idmap, int kc, int nq, float* __restrict__ part_s,
                                                  uint32_t* __restrict__ part_r, int* __restrict__ part_n, const float* __restrict__ half,
                                                  const unsigned* __restrict__ poff, size_t slab, int q0) {
  constexpr int ROW = UP ? 256 : M, BYTE0 = UP ? 128 : 0;  // bytes of an arena row, the first one this scan reads
  extern __shared__ __attribute__((aligned(16))) unsigned char pq_smem[];
  float* s_lut = reinterpret_cast<float*>(pq_smem);              // [M * 256]
  float* q_s = s_lut + M * 256;                                  // [PQ_CQ]
  uint32_t* q_r = reinterpret_cast<uint32_t*>(q_s + PQ_CQ);      // [PQ_CQ]
  int* s_wc = reinterpret_cast<int*>(q_r + PQ_CQ);               // [2][4]
  const int s = blockIdx.x, q = (int)blockIdx.y + (UP ? q0 : 0), tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float4* lq = reinterpret_cast<const float4*>(lut + ((size_t)q * ROW + BYTE0) * 256);
  for (int e = tid; e < M * 64; e += 256) reinterpret_cast<float4*>(s_lut)[e] = lq[e];
  __syncthreads();
  int cnt = 0, par = 0;  // the same in every thread
  float thr = -INFINITY;
  // queue [0, cnt) -> its best min(cnt, kc) in result order
  auto prune = [&]() {
    __syncthreads();
    for (int e = cnt + tid; e < PQ_CQ; e += 256) { q_s[e] = -INFINITY; q_r[e] = PQ_NOROW; }
    __syncthreads();
    pq_bitonic(q_s, q_r, PQ_CQ, idmap, tid, 256);
    if (cnt >= kc) { cnt = kc; thr = q_s[kc - 1]; }
  };
  const int npq = min((int)pcnt[q], np);
  for (int p = s; p < npq; p += nsplit) {
    const int l = probe[(size_t)q * np + p];
    const float cs = pscore[(size_t)q * np + p];
    const size_t r0 = (size_t)tile0[l] * 32;
    const unsigned sz = size[l];
    const float* hp = UP ? half + (size_t)blockIdx.y * slab + poff[(size_t)q * np + p] : nullptr;  // the list's partial sums
    for (unsigned base = 0; base < sz; base += 256) {
      if (cnt > PQ_CQ - 256) prune();
      const unsigned i = base + (unsigned)tid;
      float sc = -INFINITY;
      bool ok = false;
      size_t row = 0;
      if (i < sz) {
        row = r0 + i;
        const uint4* cp = reinterpret_cast<const uint4*>(codes + row * ROW + BYTE0);
        uint4 cw[M / 16];
#pragma unroll
        for (int v = 0; v < M / 16; ++v) cw[v] = cp[v];
        float acc = UP ? hp[i] : 0.f;
#pragma unroll
        for (int v = 0; v < M / 16; ++v) {
          const unsigned ww[4] = {cw[v].x, cw[v].y, cw[v].z, cw[v].w};
#pragma unroll
          for (int b = 0; b < 16; ++b) acc += s_lut[(v * 16 + b) * 256 + ((ww[b >> 2] >> (8 * (b & 3))) & 255u)];
        }
        sc = cs + acc;
        ok = sc >= thr;
      }
      const unsigned long long bal = __ballot(ok);
      if (lane == 0) s_wc[par * 4 + w] = (int)__popcll(bal);
      __syncthreads();
      const int c0 = s_wc[par * 4], c1 = s_wc[par * 4 + 1], c2 = s_wc[par * 4 + 2], c3 = s_wc[par * 4 + 3];
      if (ok) {
        const int at = cnt + (w > 0 ? c0 : 0) + (w > 1 ? c1 : 0) + (w > 2 ? c2 : 0) + (int)__popcll(bal & ((1ull << lane) - 1ull));
        q_s[at] = sc;
        q_r[at] = (uint32_t)row;
      }
      cnt += c0 + c1 + c2 + c3;
      par ^= 1;
    }
  }
  prune();
  const int keep = min(cnt, kc);
  const size_t slot = (size_t)s * nq + q;
  for (int e = tid; e < keep; e += 256) {
    part_s[slot * kc + e] = q_s[e];
    part_r[slot * kc + e] = q_r[e];
  }
  if (tid == 0) part_n[slot] = keep;
}

template <int M>
__global__ __launch_bounds__(256) void pq_cand_scan_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ lut,
                                                          const int* __restrict__ probe, const float* __restrict__ pscore,
                                                          const unsigned* __restrict__ pcnt, int np, int nsplit,
                                                          const unsigned* __restrict__ tile0, const unsigned* __restrict__ size,
                                                          const int64_t* __restrict__ idmap, int kc, int nq, float* __restrict__ part_s,
                                                          uint32_t* __restrict__ part_r, int* __restrict__ part_n) {
  pq_cand_scan_body<M, false>(codes, lut, probe, pscore, pcnt, np, nsplit, tile0, size, idmap, kc, nq, part_s, part_r, part_n, nullptr, nullptr,
                              0, 0);
}

// upper half of the M = 256 candidate scan; grid (nsplit, g).  LDS as M = 128: 144 KiB + 32 B
__global__ __launch_bounds__(256) void pq_cand_upper_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ lut,
                                                           const int* __restrict__ probe, const float* __restrict__ pscore,
                                                           const unsigned* __restrict__ pcnt, int np, int nsplit,
                                                           const unsigned* __restrict__ tile0, const unsigned* __restrict__ size,
                                                           const int64_t* __restrict__ idmap, int kc, int nq, float* __restrict__ part_s,
                                                           uint32_t* __restrict__ part_r, int* __restrict__ part_n,
                                                           const float* __restrict__ half, const unsigned* __restrict__ poff, size_t slab,
                                                           int q0) {
  pq_cand_scan_body<128, true>(codes, lut, probe, pscore, pcnt, np, nsplit, tile0, size, idmap, kc, nq, part_s, part_r, part_n, half, poff, slab,
                               q0);
}

// selection across a query's shares: one workgroup per query holds its nsplit partial lists (<= PQ_SEL_MAX entries, padded to the
// power of two n2) in the LDS, sorts them and writes the ids of the best kc (-1 behind the last one); grid nq, 1024 threads
__global__ __launch_bounds__(1024) void pq_cand_select_kernel(const float* __restrict__ part_s, const uint32_t* __restrict__ part_r,
                                                             const int* __restrict__ part_n, int nsplit, int nq, int kc, int n2,
                                                             const int64_t* __restrict__ idmap, int64_t* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pq_smem[];
  float* s_s = reinterpret_cast<float*>(pq_smem);            // [n2]
  uint32_t* s_r = reinterpret_cast<uint32_t*>(s_s + n2);     // [n2]
  const int q = blockIdx.x, tid = threadIdx.x;
  for (int e = tid; e < n2; e += 1024) {
    const int sh = e / kc, j = e - sh * kc;
    float sv = -INFINITY;
    uint32_t rv = PQ_NOROW;
    if (sh < nsplit) {
      const size_t slot = (size_t)sh * nq + q;
      if (j < part_n[slot]) { sv = part_s[slot * kc + j]; rv = part_r[slot * kc + j]; }
    }
    s_s[e] = sv;
    s_r[e] = rv;
  }
  __syncthreads();
  pq_bitonic(s_s, s_r, n2, idmap, tid, 1024);
  for (int e = tid; e < kc; e += 1024) {
    const uint32_t rv = e < n2 ? s_r[e] : PQ_NOROW;
    cand[(size_t)q * kc + e] = rv == PQ_NOROW ? -1 : idmap[rv];
  }
}

// exact scores of the candidates: grid (ceil(kc / PQ_RS_WG), nq), 4 waves, one candidate row per wave pass.  The row (d x 2 bytes of
// the refine store, found through inv) is read with one 16-byte load per lane and pass -- lane l of pass p holds columns
// 8 (64 p + l) .. + 7 -- against the ORIGINAL fp32 query held in registers.
// Summation order (knnx.h): every lane one fmaf chain from 0.f over its passes in ascending order and, inside a pass, its 8
// columns in ascending order; then the 64 lane sums meet in the xor butterfly 32, 16, 8, 4, 2, 1 (rot_query_kernel's).  Nothing in
// it depends on the batch, the shares of the ADC pass or the candidate's position.
constexpr int PQ_RS_WG = 16;  // candidates of one workgroup (4 per wave): kc = 512 of ONE query are 32 workgroups
template <int D>
__global__ __launch_bounds__(256) void pq_rescore_kernel(const _Float16* __restrict__ X, const float* __restrict__ q, int64_t id_lo,
                                                        int64_t n_ids, const uint32_t* __restrict__ inv, const int64_t* __restrict__ cand,
                                                        int kc, float* __restrict__ es) {
  constexpr int NP = (D / 8 + 63) / 64;  // passes
  const int qi = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float qv[NP][8];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int g = p * 64 + lane;
    if (g < D / 8) {
      const float4* qp = reinterpret_cast<const float4*>(q + (size_t)qi * D + (size_t)g * 8);
      const float4 a = qp[0], b = qp[1];
      qv[p][0] = a.x; qv[p][1] = a.y; qv[p][2] = a.z; qv[p][3] = a.w;
      qv[p][4] = b.x; qv[p][5] = b.y; qv[p][6] = b.z; qv[p][7] = b.w;
    } else {
#pragma unroll
      for (int t = 0; t < 8; ++t) qv[p][t] = 0.f;
    }
  }
  for (int c = blockIdx.x * PQ_RS_WG + w; c < min(kc, (int)(blockIdx.x + 1) * PQ_RS_WG); c += 4) {
    const int64_t id = cand[(size_t)qi * kc + c];
    float sc = -FLT_MAX;
    if (id >= id_lo && id - id_lo < n_ids) {  // (wave-uniform)
      const _Float16* xr = X + (size_t)inv[id - id_lo] * D;
      float acc = 0.f;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int g = p * 64 + lane;
        if (g < D / 8) {
          const uint4 v = *reinterpret_cast<const uint4*>(xr + (size_t)g * 8);
          const unsigned ww[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            const unsigned short h = (unsigned short)(ww[t >> 1] >> (16 * (t & 1)));
            _Float16 xh;
            __builtin_memcpy(&xh, &h, 2);
            acc = fmaf((float)xh, qv[p][t], acc);
          }
        }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
      sc = acc;
    }
    if (lane == 0) es[(size_t)qi * kc + c] = sc;
  }
}

// top-k of a query's kc <= PQ_REFINE_MAX exact scores by rank counting (score descending, id ascending; candidates with id < 0
// do not count), padded with -FLT_MAX / -1; grid nq, 256 threads
__global__ __launch_bounds__(256) void pq_refine_topk_kernel(const float* __restrict__ es, const int64_t* __restrict__ cand, int kc, int k,
                                                            float* __restrict__ D, int64_t* __restrict__ I) {
  __shared__ __attribute__((aligned(16))) long long s_i[PQ_REFINE_MAX];
  __shared__ __attribute__((aligned(16))) float s_s[PQ_REFINE_MAX];
  __shared__ int s_n;
  const int q = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_n = 0;
  for (int e = tid; e < kc; e += 256) {
    s_i[e] = cand[(size_t)q * kc + e];
    s_s[e] = es[(size_t)q * kc + e];
  }
  __syncthreads();
  for (int e = tid; e < kc; e += 256) {
    const long long ie = s_i[e];
    if (ie < 0) continue;
    const float se = s_s[e];
    int rank = 0;
    for (int j = 0; j < kc; ++j) rank += (s_i[j] >= 0 && pq_better(s_s[j], s_i[j], se, ie)) ? 1 : 0;
    if (rank < k) {
      D[(size_t)q * k + rank] = se;
      I[(size_t)q * k + rank] = ie;
    }
    atomicAdd(&s_n, 1);
  }
  __syncthreads();
  for (int e = min(s_n, k) + tid; e < k; e += 256) {
    D[(size_t)q * k + e] = -FLT_MAX;
    I[(size_t)q * k + e] = -1;
  }
}

// ---------------------------------------------------------------------------------------------
// decode-gather (reconstruct, the coalescer's R): out[i] = f32(c_list) + concat_m cb[m][code_m] of id ids[i]; a bad id -> 0xFF
// bytes.  The list of an arena row is the last list whose first tile is <= the row's tile (binary search over tile0).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pq_decode_kernel(const uint8_t* __restrict__ codes, int d, int M, const float* __restrict__ cb,
                                                       const _Float16* __restrict__ cent, const unsigned* __restrict__ tile0, int nlist,
                                                       int64_t id_lo, int64_t n_ids, const uint32_t* __restrict__ inv,
                                                       const int64_t* __restrict__ ids, int64_t n, float* __restrict__ out) {
  const int64_t i = blockIdx.x;
  if (i >= n) return;
  const int64_t id = ids[i];
  const bool ok = id >= id_lo && id - id_lo < n_ids;
  float* o = out + (size_t)i * d;
  if (!ok) {
    for (int c = threadIdx.x; c < d; c += 256) o[c] = __int_as_float(-1);
    return;
  }
  const size_t row = inv[id - id_lo];
  const unsigned t = (unsigned)(row / 32);
  int lo = 0, hi = nlist;  // first l with tile0[l] > t
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tile0[mid] <= t) lo = mid + 1; else hi = mid;
  }
  const int l = lo > 0 ? lo - 1 : 0;
  const int ds = d / M;
  for (int c = threadIdx.x; c < d; c += 256) {
    const int m = c / ds;
    const unsigned code = codes[row * M + m];
    o[c] = (float)cent[(size_t)l * d + c] + cb[((size_t)m * 256 + code) * ds + (c - m * ds)];
  }
}

// precomputed codes into their arena slots (knnx_ivfpq_add_codes: an index loaded from its saved codes); one thread per row
__global__ __launch_bounds__(256) void pq_scatter_codes_kernel(const uint8_t* __restrict__ src, int64_t n, int M, const int32_t* __restrict__ lists,
                                                              const int32_t* __restrict__ pos, const int64_t* __restrict__ ids,
                                                              const unsigned* __restrict__ tile0, int64_t id_lo, int64_t n_ids,
                                                              uint8_t* __restrict__ codes, int64_t* __restrict__ idmap, uint32_t* __restrict__ inv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t drow = (size_t)tile0[lists[i]] * 32 + (size_t)pos[i];
  const uint4* s = reinterpret_cast<const uint4*>(src + (size_t)i * M);
  uint4* o = reinterpret_cast<uint4*>(codes + drow * M);
  for (int v = 0; v < M / 16; ++v) o[v] = s[v];
  const int64_t id = ids[i];
  idmap[drow] = id;
  if (id >= id_lo && id - id_lo < n_ids) inv[id - id_lo] = (uint32_t)drow;
}

// ---------------------------------------------------------------------------------------------
// OPQ rotation A (f32 [d][d] row-major, y = A x) in front of the index: the small kernels around it.  (The row rotation of the build
// is the MFMA kernel knn_rotate_kernel of knn_rq_kernels.hip.)
// ---------------------------------------------------------------------------------------------
// A [d_out][d] -> W fp16 [2 d_out][d], the streamed operand of knn_rotate_kernel: rows 32 p .. 32 p + 31 of A become tile 2 p (2048 x
// the part fp16 cannot hold) and tile 2 p + 1 (fp16(A)).  One workgroup per row of A (grid = d_out), d = the row length.
__global__ __launch_bounds__(256) void rot_split_kernel(const float* __restrict__ A, int d, _Float16* __restrict__ W) {
  const int j = blockIdx.x;
  const size_t lo_row = (size_t)(j >> 5) * 64 + (j & 31), hi_row = lo_row + 32;
  for (int c = threadIdx.x; c < d; c += 256) {
    const float a = A[(size_t)j * d + c];
    const _Float16 hi = (_Float16)a;
    W[hi_row * d + c] = hi;
    W[lo_row * d + c] = (_Float16)((a - (float)hi) * KNN_LO_SCALE);
  }
}

// queries: out[i][j] = <A[j], q[i]> for nq <= 256 queries, A f32 [DO][D], q rows D wide, out rows DO wide.  Workgroup g owns ROT_QJ
// rows of A (staged in the LDS once per launch: A is read once however many queries there are) and its 4 waves walk the queries; lane
// l sums columns l, l + 64, ... in ascending order (fmaf), then the 64 partial sums meet in a butterfly: a fixed order, so a query's
// rotation does not depend on its batch.
constexpr int ROT_QJ = 4;
template <int D, int DO>
__global__ __launch_bounds__(256) void rot_query_kernel(const float* __restrict__ A, const float* __restrict__ q, int nq,
                                                       float* __restrict__ out) {
  __shared__ float sa[ROT_QJ][D];
  const int j0 = blockIdx.x * ROT_QJ, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int e = tid; e < ROT_QJ * D; e += 256) sa[e / D][e % D] = A[(size_t)j0 * D + e];
  __syncthreads();
  for (int i = w; i < nq; i += 4) {
    float qv[D / 64];
#pragma unroll
    for (int s = 0; s < D / 64; ++s) qv[s] = q[(size_t)i * D + lane + 64 * s];
    float acc[ROT_QJ];
#pragma unroll
    for (int r = 0; r < ROT_QJ; ++r) {
      float a = 0.f;
#pragma unroll
      for (int s = 0; s < D / 64; ++s) a = fmaf(sa[r][lane + 64 * s], qv[s], a);
      acc[r] = a;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
      for (int r = 0; r < ROT_QJ; ++r) acc[r] += __shfl_xor(acc[r], o);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < ROT_QJ; ++r) out[(size_t)i * DO + j0 + r] = acc[r];
    }
  }
}

// back to the original space (reconstruct, the R of a search): out[i] = A^T dec[i], out[i][c] = sum_j A[j][c] dec[i][j] in fp32, j
// ascending over the DO rows of A (fmaf); dec rows are DO wide, out rows D wide.  A workgroup takes ROT_BR decoded rows into the LDS,
// thread c owns columns c, c + 256, ... of all of them: a row of A is read once per ROT_BR output rows, coalesced.  dec rows of a bad id
// are 0xFF bytes (pq_decode_kernel) and stay 0xFF bytes.
constexpr int ROT_BR = 8;
template <int D, int DO>
__global__ __launch_bounds__(256) void rot_back_kernel(const float* __restrict__ A, const float* __restrict__ dec, int64_t n,
                                                      float* __restrict__ out) {
  __shared__ float sy[ROT_BR][DO];
  __shared__ int bad[ROT_BR];
  const int64_t i0 = (int64_t)blockIdx.x * ROT_BR;
  const int tid = threadIdx.x;
  for (int e = tid; e < ROT_BR * DO; e += 256) {
    const int64_t i = i0 + e / DO;
    sy[e / DO][e % DO] = i < n ? dec[(size_t)i * DO + e % DO] : 0.f;
  }
  __syncthreads();
  if (tid < ROT_BR) bad[tid] = __float_as_int(sy[tid][0]) == -1 && __float_as_int(sy[tid][DO - 1]) == -1;
  __syncthreads();
  constexpr int NC = D / 256;
  float acc[ROT_BR][NC];
#pragma unroll
  for (int r = 0; r < ROT_BR; ++r)
#pragma unroll
    for (int u = 0; u < NC; ++u) acc[r][u] = 0.f;
  for (int j = 0; j < DO; ++j) {
    float a[NC];
#pragma unroll
    for (int u = 0; u < NC; ++u) a[u] = A[(size_t)j * D + tid + 256 * u];
#pragma unroll
    for (int r = 0; r < ROT_BR; ++r) {
      const float y = sy[r][j];
#pragma unroll
      for (int u = 0; u < NC; ++u) acc[r][u] = fmaf(a[u], y, acc[r][u]);
    }
  }
#pragma unroll
  for (int r = 0; r < ROT_BR; ++r) {
    if (i0 + r >= n) break;
#pragma unroll
    for (int u = 0; u < NC; ++u) out[(size_t)(i0 + r) * D + tid + 256 * u] = bad[r] ? __int_as_float(-1) : acc[r][u];
  }
}

// OPQ training: G = X^T Y (f32 [d][d]) for fp16 rows X [n][d] and f32 rows Y [n][d] -- the matrix whose SVD gives the Procrustes
// step.  Workgroup (bx, by) owns the 64 x 64 block G[64 by ..][64 bx ..], thread (ty, tx) a 4 x 4 piece of it; the n rows go through
// the LDS 16 at a time and every element is ONE fmaf chain over the rows in ascending order: two runs give the same bits.
__global__ __launch_bounds__(256) void xty_kernel(const _Float16* __restrict__ X, const float* __restrict__ Y, int64_t n, int d,
                                                 float* __restrict__ G) {
  __shared__ float sx[16][64], sy[16][64];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  for (int64_t i0 = 0; i0 < n; i0 += 16) {
    __syncthreads();
    for (int e = tid; e < 16 * 64; e += 256) {
      const int64_t i = i0 + e / 64;
      sx[e / 64][e % 64] = i < n ? (float)X[(size_t)i * d + r0 + e % 64] : 0.f;
      sy[e / 64][e % 64] = i < n ? Y[(size_t)i * d + c0 + e % 64] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      float xv[4], yv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) xv[a] = sx[k][4 * ty + a];
#pragma unroll
      for (int b = 0; b < 4; ++b) yv[b] = sy[k][4 * tx + b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(xv[a], yv[b], acc[a][b]);
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) G[(size_t)(r0 + 4 * ty + a) * d + c0 + 4 * tx + b] = acc[a][b];
}

// ---------------------------------------------------------------------------------------------
// host-side launchers (declared in knn_kernels.h)
// ---------------------------------------------------------------------------------------------
static bool rot_supported(int d) { return d == 256 || d == 512 || d == 768 || d == 1024; }

hipError_t launch_rot_split(const float* A, int d, int d_out, _Float16* W, hipStream_t st) {
  if (!rot_supported(d) || !rot_supported(d_out) || d_out < d) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rot_split_kernel, dim3((unsigned)d_out), dim3(256), 0, st, A, d, W);
  return hipGetLastError();
}

// the ten (d, d_out) pairs: d_out = d and the six rectangular ones, d < d_out
#define ROT_PAIR(CALL, DI, DOUT) \
  if (d == DI && d_out == DOUT) { CALL(DI, DOUT); } else
#define ROT_BY_D(CALL)                                                                                                   \
  ROT_PAIR(CALL, 256, 256) ROT_PAIR(CALL, 512, 512) ROT_PAIR(CALL, 768, 768) ROT_PAIR(CALL, 1024, 1024)                  \
  ROT_PAIR(CALL, 256, 512) ROT_PAIR(CALL, 256, 768) ROT_PAIR(CALL, 256, 1024) ROT_PAIR(CALL, 512, 768)                   \
  ROT_PAIR(CALL, 512, 1024) ROT_PAIR(CALL, 768, 1024) return hipErrorInvalidValue;

hipError_t launch_rot_queries(const float* A, int d, int d_out, const float* q, int nq, float* out, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
#define ROT_Q(DI, DOUT) hipLaunchKernelGGL((rot_query_kernel<DI, DOUT>), dim3((unsigned)(DOUT / ROT_QJ)), dim3(256), 0, st, A, q, nq, out)
  ROT_BY_D(ROT_Q)
#undef ROT_Q
  return hipGetLastError();
}

hipError_t launch_rot_back(const float* A, int d, int d_out, const float* dec, int64_t n, float* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
#define ROT_B(DI, DOUT) \
  hipLaunchKernelGGL((rot_back_kernel<DI, DOUT>), dim3((unsigned)((n + ROT_BR - 1) / ROT_BR)), dim3(256), 0, st, A, dec, n, out)
  ROT_BY_D(ROT_B)
#undef ROT_B
  return hipGetLastError();
}
#undef ROT_BY_D
#undef ROT_PAIR

hipError_t launch_xty(const _Float16* X, const float* Y, int64_t n, int d, float* G, hipStream_t st) {
  if (n <= 0 || !rot_supported(d)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(xty_kernel, dim3((unsigned)(d / 64), (unsigned)(d / 64)), dim3(256), 0, st, X, Y, n, d, G);
  return hipGetLastError();
}

bool pq_supported(int d, int M) {
  if (M == 256) return d == 512 || d == 768 || d == 1024;  // the two-half scan; d / M = 2, 3, 4
  return (M == 16 || M == 32 || M == 64 || M == 128) && d % 256 == 0 && d > 0 && d <= 1024 && d % M == 0 && d / M <= 64;
}

template <int DS>
static hipError_t launch_encode_ds(const _Float16* X, int64_t n, int d, int M, const int32_t* lists, const _Float16* cent, const float* cb,
                                   const unsigned* tile0, const int32_t* pos, const int64_t* ids, int64_t id0, int64_t id_lo, int64_t n_ids,
                                   uint8_t* codes, int64_t* idmap, uint32_t* inv, hipStream_t st) {
  auto kern = pq_encode_kernel<DS>;
  const int smem = 256 * DS * (int)sizeof(float);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)((n + 255) / 256)), dim3(256), smem, st, X, n, d, M, lists, cent, cb, tile0, pos, ids, id0, id_lo,
                     n_ids, codes, idmap, inv);
  return hipGetLastError();
}

hipError_t launch_pq_encode(const _Float16* X, int64_t n, int d, int M, const int32_t* lists, const _Float16* cent, const float* cb,
                            const unsigned* tile0, const int32_t* pos, const int64_t* ids, int64_t id0, int64_t id_lo, int64_t n_ids,
                            uint8_t* codes, int64_t* idmap, uint32_t* inv, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!pq_supported(d, M)) return hipErrorInvalidValue;
#define PQ_ENC(DS) \
  case DS: return launch_encode_ds<DS>(X, n, d, M, lists, cent, cb, tile0, pos, ids, id0, id_lo, n_ids, codes, idmap, inv, st);
  switch (d / M) {
    PQ_ENC(2) PQ_ENC(3) PQ_ENC(4) PQ_ENC(6) PQ_ENC(8) PQ_ENC(12) PQ_ENC(16) PQ_ENC(24) PQ_ENC(32) PQ_ENC(48) PQ_ENC(64)
    default: return hipErrorInvalidValue;
  }
#undef PQ_ENC
}

hipError_t launch_pq_update(const _Float16* X, int d, int M, const int32_t* lists, const _Float16* cent, const int32_t* order,
                            const int32_t* off, int64_t n, float* cb, hipStream_t st) {
  if (!pq_supported(d, M)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pq_update_kernel, dim3((unsigned)(M * 256)), dim3(64), 0, st, X, d, M, lists, cent, order, off, n, cb);
  return hipGetLastError();
}

hipError_t launch_pq_seed(const _Float16* X, int d, int M, const int32_t* lists, const _Float16* cent, const int32_t* mj, const int64_t* rows,
                          int64_t n, float* cb, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!pq_supported(d, M)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pq_seed_kernel, dim3((unsigned)n), dim3(64), 0, st, X, d, M, lists, cent, mj, rows, cb);
  return hipGetLastError();
}

hipError_t launch_pq_lut(const float* q, int nq, int d, int M, const float* cb, float* lut, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  if (!pq_supported(d, M)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pq_lut_kernel, dim3((unsigned)nq, (unsigned)M), dim3(256), 0, st, q, d, M, cb, lut);
  return hipGetLastError();
}

hipError_t launch_pq_probe(const unsigned* masks, const float* scores, int nq, int nlist, int np, unsigned* pcnt, int* probe, float* pscore,
                           hipStream_t st) {
  hipError_t e = hipMemsetAsync(pcnt, 0, (size_t)nq * sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pq_probe_kernel, dim3((unsigned)((nlist + 255) / 256), (unsigned)((nq + 31) / 32)), dim3(256), 0, st, masks, scores, nq,
                     nlist, np, pcnt, probe, pscore);
  return hipGetLastError();
}

size_t pq_scan_smem_bytes(int M) { return (size_t)M * 256 * 4 + (size_t)4 * PQ_WQ * (8 + 4 + 4); }

hipError_t launch_pq_adc_scan(const uint8_t* codes, int M, const float* lut, const int* probe, const float* pscore, const unsigned* pcnt,
                              int np, int nsplit, const unsigned* tile0, const unsigned* size, const int64_t* idmap, int k, int nq,
                              float* part_s, uint32_t* part_i, int* part_n, hipStream_t st) {
  if (k < 1 || k > PQ_MAX_K || nq <= 0 || nsplit <= 0) return hipErrorInvalidValue;
  const size_t smem = pq_scan_smem_bytes(M);
  if (smem + 64 > (size_t)KNN_LDS_BYTES) return hipErrorInvalidValue;
#define PQ_SCAN(MM)                                                                                                               \
  case MM: {                                                                                                                      \
    auto kern = pq_adc_scan_kernel<MM>;                                                                                           \
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); \
    if (e != hipSuccess) return e;                                                                                                \
    hipLaunchKernelGGL(kern, dim3((unsigned)nsplit, (unsigned)nq), dim3(256), smem, st, codes, lut, probe, pscore, pcnt, np, nsplit, \
                       tile0, size, idmap, k, nq, part_s, part_i, part_n);                                                        \
    return hipGetLastError();                                                                                                     \
  }
  switch (M) {
    PQ_SCAN(16) PQ_SCAN(32) PQ_SCAN(64) PQ_SCAN(128)
    default: return hipErrorInvalidValue;
  }
#undef PQ_SCAN
}

// threshold scan of nq queries over the probe lists / LUTs of their pass: thr [nq], cnt [nq] (cleared here), hits to hit_s / hit_r
// [nq][cap]
hipError_t launch_pq_range_scan(const uint8_t* codes, int M, const float* lut, const int* probe, const float* pscore, const unsigned* pcnt,
                                int np, int nsplit, const unsigned* tile0, const unsigned* size, const float* thr, unsigned* cnt,
                                unsigned cap, float* hit_s, uint32_t* hit_r, int nq, hipStream_t st) {
  if (nq <= 0 || nsplit <= 0 || np <= 0 || !thr || !cnt || (cap > 0 && (!hit_s || !hit_r))) return hipErrorInvalidValue;
  const size_t smem = (size_t)M * 256 * 4;
  if (smem + 64 > (size_t)KNN_LDS_BYTES) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(cnt, 0, (size_t)nq * sizeof(unsigned), st);
  if (e != hipSuccess) return e;
#define PQ_RSCAN(MM)                                                                                                              \
  case MM: {                                                                                                                      \
    auto kern = pq_range_scan_kernel<MM>;                                                                                         \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);           \
    if (e != hipSuccess) return e;                                                                                                \
    hipLaunchKernelGGL(kern, dim3((unsigned)nsplit, (unsigned)nq), dim3(256), smem, st, codes, lut, probe, pscore, pcnt, np, nsplit, \
                       tile0, size, thr, cnt, cap, hit_s, hit_r);                                                                 \
    return hipGetLastError();                                                                                                     \
  }
  switch (M) {
    PQ_RSCAN(16) PQ_RSCAN(32) PQ_RSCAN(64) PQ_RSCAN(128)
    default: return hipErrorInvalidValue;
  }
#undef PQ_RSCAN
}

// refine: the candidate scan for 64 < kc <= PQ_REFINE_MAX; part_s / part_r hold nsplit * nq lists of kc entries
hipError_t launch_pq_cand_scan(const uint8_t* codes, int M, const float* lut, const int* probe, const float* pscore, const unsigned* pcnt,
                               int np, int nsplit, const unsigned* tile0, const unsigned* size, const int64_t* idmap, int kc, int nq,
                               float* part_s, uint32_t* part_r, int* part_n, hipStream_t st) {
  if (kc < 1 || kc > PQ_REFINE_MAX || nq <= 0 || nsplit <= 0) return hipErrorInvalidValue;
  const size_t smem = (size_t)M * 1024 + (size_t)PQ_CQ * 8 + 32;
  if (smem + 64 > (size_t)KNN_LDS_BYTES) return hipErrorInvalidValue;
#define PQ_CSCAN(MM)                                                                                                              \
  case MM: {                                                                                                                      \
    auto kern = pq_cand_scan_kernel<MM>;                                                                                          \
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); \
    if (e != hipSuccess) return e;                                                                                                \
    hipLaunchKernelGGL(kern, dim3((unsigned)nsplit, (unsigned)nq), dim3(256), smem, st, codes, lut, probe, pscore, pcnt, np, nsplit, \
                       tile0, size, idmap, kc, nq, part_s, part_r, part_n);                                                       \
    return hipGetLastError();                                                                                                     \
  }
  switch (M) {
    PQ_CSCAN(16) PQ_CSCAN(32) PQ_CSCAN(64) PQ_CSCAN(128)
    default: return hipErrorInvalidValue;
  }
#undef PQ_CSCAN
}

// ---- M = 256: the two halves (queries q0 .. q0 + g - 1 of a pass of nq; half = their partial-sum slabs, g x slab floats) ----
hipError_t launch_pq_probe_offsets(const int* probe, const unsigned* pcnt, int np, const unsigned* size, unsigned* poff, int nq, hipStream_t st) {
  if (nq <= 0 || np <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pq_probe_offsets_kernel, dim3((unsigned)nq), dim3(256), 0, st, probe, pcnt, np, size, poff);
  return hipGetLastError();
}

// sets the dynamic LDS size of a kernel and launches it on grid (nsplit, g)
template <class K, class... A>
static hipError_t pq_launch_half(K kern, size_t smem, int nsplit, int g, hipStream_t st, A... args) {
  if (g <= 0 || nsplit <= 0 || smem + 64 > (size_t)KNN_LDS_BYTES) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)nsplit, (unsigned)g), dim3(256), smem, st, args...);
  return hipGetLastError();
}

hipError_t launch_pq_adc_lower(const uint8_t* codes, const float* lut, const int* probe, const unsigned* pcnt, int np, int nsplit,
                               const unsigned* tile0, const unsigned* size, const unsigned* poff, const float* thr, size_t slab, int q0, int g,
                               float* half, hipStream_t st) {
  return pq_launch_half(pq_adc_lower_kernel, (size_t)128 * 1024, nsplit, g, st, codes, lut, probe, pcnt, np, nsplit, tile0, size, poff, thr,
                        slab, q0, half);
}

hipError_t launch_pq_adc_upper(const uint8_t* codes, const float* lut, const int* probe, const float* pscore, const unsigned* pcnt, int np,
                               int nsplit, const unsigned* tile0, const unsigned* size, const int64_t* idmap, int k, int nq, float* part_s,
                               uint32_t* part_i, int* part_n, const float* half, const unsigned* poff, size_t slab, int q0, int g,
                               hipStream_t st) {
  if (k < 1 || k > PQ_MAX_K || q0 < 0 || q0 + g > nq) return hipErrorInvalidValue;
  return pq_launch_half(pq_adc_upper_kernel, pq_scan_smem_bytes(128), nsplit, g, st, codes, lut, probe, pscore, pcnt, np, nsplit, tile0, size,
                        idmap, k, nq, part_s, part_i, part_n, half, poff, slab, q0);
}

hipError_t launch_pq_cand_upper(const uint8_t* codes, const float* lut, const int* probe, const float* pscore, const unsigned* pcnt, int np,
                                int nsplit, const unsigned* tile0, const unsigned* size, const int64_t* idmap, int kc, int nq, float* part_s,
                                uint32_t* part_r, int* part_n, const float* half, const unsigned* poff, size_t slab, int q0, int g,
                                hipStream_t st) {
  if (kc < 1 || kc > PQ_REFINE_MAX || q0 < 0 || q0 + g > nq) return hipErrorInvalidValue;
  return pq_launch_half(pq_cand_upper_kernel, (size_t)128 * 1024 + (size_t)PQ_CQ * 8 + 32, nsplit, g, st, codes, lut, probe, pscore, pcnt, np,
                        nsplit, tile0, size, idmap, kc, nq, part_s, part_r, part_n, half, poff, slab, q0);
}

// (cnt is NOT cleared here: the caller clears the pass's counters once, before the first sub-group)
hipError_t launch_pq_range_upper(const uint8_t* codes, const float* lut, const int* probe, const float* pscore, const unsigned* pcnt, int np,
                                 int nsplit, const unsigned* tile0, const unsigned* size, const float* thr, unsigned* cnt, unsigned cap,
                                 float* hit_s, uint32_t* hit_r, const float* half, const unsigned* poff, size_t slab, int q0, int g,
                                 hipStream_t st) {
  if (np <= 0 || !thr || !cnt || (cap > 0 && (!hit_s || !hit_r)) || q0 < 0) return hipErrorInvalidValue;
  return pq_launch_half(pq_range_upper_kernel, (size_t)128 * 1024, nsplit, g, st, codes, lut, probe, pscore, pcnt, np, nsplit, tile0, size, thr,
                        cnt, cap, hit_s, hit_r, half, poff, slab, q0);
}

// refine: the ids of the best kc of a query's nsplit partial lists -> cand [nq][kc] (-1 padded); nsplit * kc <= PQ_SEL_MAX
hipError_t launch_pq_cand_select(const float* part_s, const uint32_t* part_r, const int* part_n, int nsplit, int nq, int kc,
                                 const int64_t* idmap, int64_t* cand, hipStream_t st) {
  if (nq <= 0 || nsplit <= 0 || kc < 1 || (size_t)nsplit * kc > (size_t)PQ_SEL_MAX) return hipErrorInvalidValue;
  int n2 = 2;
  while (n2 < nsplit * kc) n2 <<= 1;
  const size_t smem = (size_t)n2 * 8;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pq_cand_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pq_cand_select_kernel, dim3((unsigned)nq), dim3(1024), smem, st, part_s, part_r, part_n, nsplit, nq, kc, n2, idmap, cand);
  return hipGetLastError();
}

// refine: exact scores of cand [nq][kc] from the fp16 rows X (arena order, through inv) against q f32 [nq][d], then the top k of them
hipError_t launch_pq_refine(const _Float16* X, int d, const float* q, int nq, int64_t id_lo, int64_t n_ids, const uint32_t* inv,
                            const int64_t* cand, int kc, int k, float* es, float* D, int64_t* I, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  if (kc < 1 || kc > PQ_REFINE_MAX || k < 1 || k > kc) return hipErrorInvalidValue;
  hipError_t e = launch_pq_rescore(X, d, q, nq, id_lo, n_ids, inv, cand, kc, es, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pq_refine_topk_kernel, dim3((unsigned)nq), dim3(256), 0, st, es, cand, kc, k, D, I);
  return hipGetLastError();
}

// the exact scores alone, any kc >= 1 (the large-k refine search ranks them on the host): es [nq][kc], -FLT_MAX where cand is no id
hipError_t launch_pq_rescore(const _Float16* X, int d, const float* q, int nq, int64_t id_lo, int64_t n_ids, const uint32_t* inv,
                             const int64_t* cand, int kc, float* es, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  if (kc < 1 || nq > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((kc + PQ_RS_WG - 1) / PQ_RS_WG), (unsigned)nq);
#define PQ_RS(DD) hipLaunchKernelGGL(pq_rescore_kernel<DD>, grid, dim3(256), 0, st, X, q, id_lo, n_ids, inv, cand, kc, es)
  switch (d) {
    case 256: PQ_RS(256); break;
    case 512: PQ_RS(512); break;
    case 768: PQ_RS(768); break;
    case 1024: PQ_RS(1024); break;
    default: return hipErrorInvalidValue;
  }
#undef PQ_RS
  return hipGetLastError();
}

hipError_t launch_pq_decode(const uint8_t* codes, int d, int M, const float* cb, const _Float16* cent, const unsigned* tile0, int nlist,
                            int64_t id_lo, int64_t n_ids, const uint32_t* inv, const int64_t* ids, int64_t n, float* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!pq_supported(d, M)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pq_decode_kernel, dim3((unsigned)n), dim3(256), 0, st, codes, d, M, cb, cent, tile0, nlist, id_lo, n_ids, inv, ids, n, out);
  return hipGetLastError();
}

hipError_t launch_pq_scatter_codes(const uint8_t* src, int64_t n, int M, const int32_t* lists, const int32_t* pos, const int64_t* ids,
                                   const unsigned* tile0, int64_t id_lo, int64_t n_ids, uint8_t* codes, int64_t* idmap, uint32_t* inv,
                                   hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(pq_scatter_codes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, n, M, lists, pos, ids, tile0, id_lo,
                     n_ids, codes, idmap, inv);
  return hipGetLastError();
}

}  // namespace knnx
